"""Ceiling of a tile-local row order for k_pure_vle<true, false>: pcs_pure_vle_fast of the built library, in ONE process at
1e7 bench rows, on the batch as it is, on host-permuted copies (rows ordered inside tiles of R rows by class, or by
class and a tau bin) and on the batch fully sorted by class.  Host-permuted inputs are contiguous: the ceiling without
gather cost.  Workgroup b runs on XCD b % 8, so a tile of 8 workgroups ordered by class sends the same class to the same XCD on
every tile: the "xcd" inputs hold, at workgroup b, the rows that the bijective XCD swizzle would give it (a tile's workgroups on
one XCD, every XCD sees every class), on the first floor(n / 256) * 256 rows.  ALT alternations of LAUNCHES back-to-back launches per input, order reversed every other alternation;
median / range per input and the ratio to the unsorted batch.  The unsorted batch is timed twice (two device copies):
the spread of identical work.  Usage: tile_order_ab.py [--out FILE.json]"""
import ctypes, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))); sys.path.insert(0, ROOT); os.chdir(ROOT)
import numpy as np, torch
from feos_torch_amd.synthetic import pure_batch
from feos_torch_amd import _lib
out = sys.argv[2] if len(sys.argv) > 2 and sys.argv[1] == "--out" else None
ALT, LAUNCHES = int(os.environ.get("PCS_AB_ALT", "7")), int(os.environ.get("PCS_AB_LAUNCHES", "50"))
n = int(os.environ.get("PCS_AB_ROWS", "10000000"))
P, T = pure_batch(n)
polar, assoc = P[:, 3] != 0, (P[:, 4] != 0) & ((P[:, 6] != 0) | (P[:, 7] != 0))
cls = np.where(polar, np.where(assoc, 2, 1), np.where(assoc, 3, 0))  # k1_bucket's Gray order
tau = T / (1.28 * P[:, 2] * P[:, 0] ** 0.45)
def tile_order(R, bins, rows=n):
    key = ((np.arange(n) // R) * (4 * bins) + cls * bins)[:rows]
    if bins > 1:
        lo, hi = tau.min(), tau.max()
        key = key + np.clip(((tau - lo) / (hi - lo) * bins).astype(np.int64), 0, bins - 1)[:rows]
    return np.argsort(key, kind="stable")
inputs = {"unsorted": None, "unsorted (copy)": None}
for bins in (1, 4, 8):
    for R in (2048, 4096, 8192):
        inputs[f"R={R} class" + (f", {bins} tau bins" if bins > 1 else "")] = tile_order(R, bins)
inputs["fully sorted by class"] = np.argsort(cls, kind="stable")
inputs["fully sorted by class, tau"] = np.lexsort((tau, cls))
nwg = n // 256
def xcd_grouped(o):  # rows of logical workgroup swz(b) at workgroup b; swz as in the kernel guide (bijective for any nwg)
    b = np.arange(nwg); x, q, r = b % 8, nwg // 8, nwg % 8
    swz = np.where(x < r, x * (q + 1), r * (q + 1) + (x - r) * q) + b // 8
    assert np.array_equal(np.sort(swz), b)
    return o.reshape(nwg, 256)[swz].ravel()
inputs["xcd: unsorted, full blocks only"] = np.arange(nwg * 256)
inputs["xcd: unsorted"] = xcd_grouped(np.arange(nwg * 256))
for bins in (1, 4, 8):
    for R in (2048, 4096, 8192, 16384):
        inputs[f"xcd: R={R} class" + (f", {bins} tau bins" if bins > 1 else "")] = xcd_grouped(tile_order(R, bins, nwg * 256))
vp = ctypes.c_void_p
L = _lib.lib()
p = torch.empty(n, dtype=torch.float64, device="cuda"); st = torch.empty(n, dtype=torch.uint8, device="cuda")
ws = torch.empty(n + 64, dtype=torch.int32, device="cuda")
stream = vp(torch.cuda.current_stream().cuda_stream)
dev, res = {}, {}
for nm, o in inputs.items():
    Pd = torch.from_numpy(P if o is None else np.ascontiguousarray(P[o])).cuda()
    Td = torch.from_numpy(T if o is None else np.ascontiguousarray(T[o])).cuda()
    dev[nm] = (Pd, Td, (vp(Pd.data_ptr()), vp(Td.data_ptr()), len(Td), vp(p.data_ptr()), None, None, vp(st.data_ptr()), None, vp(ws.data_ptr()), stream))
ref = None
for nm, o in inputs.items():  # warm-up, and the results against the unsorted batch (a row's place must not change its bits)
    assert L.pcs_pure_vle_fast(*dev[nm][2]) == 0
    torch.cuda.synchronize()
    entries = int(ws[0].item())
    k = n if o is None else len(o)
    pp, ss = p.cpu().numpy()[:k], st.cpu().numpy()[:k]
    if ref is None: ref = (pp.copy(), ss.copy())
    rp, rs = (ref[0], ref[1]) if o is None else (ref[0][o], ref[1][o])  # position j of this input holds row o[j] of the batch
    ok = ss == 0
    res[nm] = {"rows": k, "list_entries": entries, "status_diff": int((ss != rs).sum()), "p_sat_bits_differing": int((pp[ok] != rp[ok]).sum())}
times = {nm: [] for nm in inputs}
names = list(inputs)
for alt in range(ALT + 1):
    for nm in (names if alt % 2 == 0 else names[::-1]):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(LAUNCHES): L.pcs_pure_vle_fast(*dev[nm][2])
        e1.record(); torch.cuda.synchronize()
        if alt >= 1: times[nm].append(e0.elapsed_time(e1) / LAUNCHES)
base = float(np.median(times[names[0]]))
for nm in names:
    t = np.array(times[nm])
    res[nm].update(median_ms=float(np.median(t)), min_ms=float(t.min()), max_ms=float(t.max()), ratio_unsorted_over_this=base / float(np.median(t)))
    print(f"{nm:34s} median {np.median(t):.4f} ms  range {t.min():.4f} .. {t.max():.4f}  x{base / np.median(t):.4f}  {res[nm]['list_entries']} listed, "
          f"{res[nm]['status_diff']} status / {res[nm]['p_sat_bits_differing']} p_sat differing", flush=True)
if out:
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    json.dump({"rows": n, "alternations": ALT, "launches_per_block": LAUNCHES, "inputs": res}, open(out, "w"), indent=1)
