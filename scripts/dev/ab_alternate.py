"""Alternating A/B of pcs_pure_vle_fast (workspace reset + k_pure_vle<true,false>) for several builds of libpcsaft_hip
(scratch/ab/lib_<name>.so) in ONE process at 1e7 rows: ALT alternations, each LAUNCHES back-to-back launches per library
between two device events.  Prints median / min / max of the per-launch time of every library over the alternations and the
ratio to the first; a library named twice (copy the file under a second name) gives the spread of identical code.
Also compares p_sat / status of every library with the first one's.  Usage: ab_alternate.py [--out FILE.json] names..."""
import ctypes, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))); sys.path.insert(0, ROOT); os.chdir(ROOT)
import numpy as np, torch
from feos_torch_amd.synthetic import pure_batch
argv = sys.argv[1:]
out = None
if argv and argv[0] == "--out":
    out, argv = argv[1], argv[2:]
names = argv
ALT, LAUNCHES = int(os.environ.get("PCS_AB_ALT", "7")), int(os.environ.get("PCS_AB_LAUNCHES", "100"))
n = 10_000_000
P, T = pure_batch(n)
Pd, Td = torch.from_numpy(P).cuda(), torch.from_numpy(T).cuda()
vp = ctypes.c_void_p
libs = {}
for nm in names:
    L = ctypes.CDLL(os.path.abspath(f"scratch/ab/lib_{nm}.so"))
    L.pcs_pure_vle_fast.argtypes = [vp, vp, ctypes.c_int64] + [vp] * 7
    L.pcs_pure_vle_retry.argtypes = [vp, vp, ctypes.c_int64] + [vp] * 7
    libs[nm] = L
p = torch.empty(n, dtype=torch.float64, device="cuda"); st = torch.empty(n, dtype=torch.uint8, device="cuda")
ws = torch.empty(n + 64, dtype=torch.int32, device="cuda")
stream = vp(torch.cuda.current_stream().cuda_stream)
args = (vp(Pd.data_ptr()), vp(Td.data_ptr()), n, vp(p.data_ptr()), None, None, vp(st.data_ptr()), None, vp(ws.data_ptr()), stream)
res = {}
ref = None
for nm in names:  # warm-up, and the results
    p.zero_(); st.zero_()
    assert libs[nm].pcs_pure_vle_fast(*args) == 0
    torch.cuda.synchronize()
    entries = int(ws[0].item())
    assert libs[nm].pcs_pure_vle_retry(*args) == 0
    torch.cuda.synchronize()
    cur = (p.cpu().numpy().copy(), st.cpu().numpy().copy())
    if ref is None: ref = cur
    ok = (ref[1] == 0) & (cur[1] == 0)
    rel = np.abs(cur[0][ok] - ref[0][ok]) / np.abs(ref[0][ok])
    res[nm] = {"failed": int(cur[1].sum()), "list_entries": entries, "status_diff_vs_first": int((cur[1] != ref[1]).sum()),
               "max_rel_vs_first": float(rel.max()), "rows_differing": int((rel > 0).sum())}
    print(nm, res[nm], flush=True)
times = {nm: [] for nm in names}
for alt in range(ALT + 1):
    for nm in (names if alt % 2 == 0 else names[::-1]):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(LAUNCHES): libs[nm].pcs_pure_vle_fast(*args)
        e1.record(); torch.cuda.synchronize()
        if alt >= 1: times[nm].append(e0.elapsed_time(e1) / LAUNCHES)
base = float(np.median(times[names[0]]))
for nm in names:
    t = np.array(times[nm])
    res[nm].update(median_ms=float(np.median(t)), min_ms=float(t.min()), max_ms=float(t.max()), ratio_first_over_this=base / float(np.median(t)),
                   blocks_ms=[round(float(x), 5) for x in t])
    print(f"{nm:10s} median {np.median(t):.4f} ms  range {t.min():.4f} .. {t.max():.4f}  x{base / np.median(t):.4f}", flush=True)
if out:
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    json.dump({"rows": n, "alternations": ALT, "launches_per_block": LAUNCHES, "libs": res}, open(out, "w"), indent=1)
