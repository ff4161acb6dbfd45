"""Alternating A/B of the ordered pressure-only fast stage against the plain one, in ONE process at 1e7 bench rows, in the
manner of ab_alternate.py: ALT alternations of LAUNCHES back-to-back launches per configuration, order reversed every other one.
Libraries: scratch/ab/lib_parent.so, lib_copy.so (a second copy of the parent: the spread of identical code) and the built
library.  Configurations of the built library: its plain entry; pcs_pure_vle_fast_ordered with the order of the inputs; with an
order built from PERTURBED parameters (m, sigma, eps each scaled by an independent U[0.95, 1.05], same T: a fit that has
moved); the parent library's ordered entry with the parent's own orders (own, perturbed: the baseline of a change to
pcs_pure_row_order) and the parent's order fed to the built library; with a class-only order and with class + tau orders of other tile sizes (built on the host); the own order through
scratch/ab/lib_noswz.so when it is there (a copy of csrc/ with the XCD swizzle of ordered_stage compiled out).  A second batch
whose tau range is narrow and shifted (the bench parameters at tau ~ U[0.70, 0.80]): plain against ordered.  Also the time of
pcs_pure_row_order.  p_sat / status of every configuration against the parent's.  Usage: ab_ordered.py [--out FILE.json]"""
import ctypes, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))); sys.path.insert(0, ROOT); os.chdir(ROOT)
import numpy as np, torch
from feos_torch_amd.synthetic import pure_batch
from feos_torch_amd import _lib
out = sys.argv[2] if len(sys.argv) > 2 and sys.argv[1] == "--out" else None
ALT, LAUNCHES = int(os.environ.get("PCS_AB_ALT", "7")), int(os.environ.get("PCS_AB_LAUNCHES", "100"))
n = 10_000_000
P, T = pure_batch(n)
rng = np.random.default_rng(77)
P2 = P.copy(); P2[:, :3] *= rng.uniform(0.95, 1.05, (n, 3))
Pd, Td, P2d = torch.from_numpy(P).cuda(), torch.from_numpy(T).cuda(), torch.from_numpy(P2).cuda()
vp = ctypes.c_void_p
def plain(path):
    L = ctypes.CDLL(os.path.abspath(path))
    L.pcs_pure_vle_fast.argtypes = [vp, vp, ctypes.c_int64] + [vp] * 7
    L.pcs_pure_vle_retry.argtypes = [vp, vp, ctypes.c_int64] + [vp] * 7
    L.pcs_pure_vle_fast_ordered.argtypes = [vp, vp, ctypes.c_int64] + [vp] * 8
    L.pcs_pure_row_order.argtypes = [vp, vp, ctypes.c_int64, vp, vp]
    return L
new = _lib.lib()
p = torch.empty(n, dtype=torch.float64, device="cuda"); st = torch.empty(n, dtype=torch.uint8, device="cuda")
ws = torch.empty(n + 64, dtype=torch.int32, device="cuda")
stream = vp(torch.cuda.current_stream().cuda_stream)
args = (vp(Pd.data_ptr()), vp(Td.data_ptr()), n, vp(p.data_ptr()), None, None, vp(st.data_ptr()), None, vp(ws.data_ptr()))
def device_order(Pt, L=new, Tt=Td):
    o = torch.empty(n, dtype=torch.int32, device="cuda")
    assert L.pcs_pure_row_order(vp(Pt.data_ptr()), vp(Tt.data_ptr()), n, vp(o.data_ptr()), stream) == 0
    return o
polar, assoc = P[:, 3] != 0, (P[:, 4] != 0) & ((P[:, 6] != 0) | (P[:, 7] != 0))
cls = np.where(polar, np.where(assoc, 2, 1), np.where(assoc, 3, 0))
tau = T / (1.28 * P[:, 2] * P[:, 0] ** 0.45)
def host_order(R, bins):
    key = (np.arange(n) // R) * (4 * bins) + cls * bins
    if bins > 1: key = key + np.clip(((tau - 0.55) / 0.35 * bins).astype(np.int64), 0, bins - 1)
    return torch.from_numpy(np.argsort(key, kind="stable").astype(np.int32)).cuda()
orders = {"ordered, own order": device_order(Pd), "ordered, perturbed-parameter order": device_order(P2d),
          "ordered, class only R=16384": host_order(16384, 1), "ordered, R=8192 8 bins": host_order(8192, 8),
          "ordered, R=16384 4 bins": host_order(16384, 4), "ordered, R=32768 8 bins": host_order(32768, 8),
          "ordered, R=16384 16 bins": host_order(16384, 16), "ordered, identity": torch.arange(n, dtype=torch.int32, device="cuda")}
def ordered_call(o, L=new, a=args):
    return lambda: L.pcs_pure_vle_fast_ordered(*a, vp(o.data_ptr()), stream)
parent, copy = plain("scratch/ab/lib_parent.so"), plain("scratch/ab/lib_copy.so")
# the parent's ordered path with the parent's own order is what the benchmark ran before: the baseline of the ordered rows
parent_orders = {"own": device_order(Pd, parent), "perturbed": device_order(P2d, parent)}
configs = {"parent": lambda: parent.pcs_pure_vle_fast(*args, stream),
           "parent (copy)": lambda: copy.pcs_pure_vle_fast(*args, stream),
           "parent, ordered, own order": ordered_call(parent_orders["own"], parent),
           "parent (copy), ordered, own order": ordered_call(parent_orders["own"], copy),
           "parent, ordered, perturbed-parameter order": ordered_call(parent_orders["perturbed"], parent),
           "new, plain entry": lambda: new.pcs_pure_vle_fast(*args, stream),
           "new, ordered, the parent's own order": ordered_call(parent_orders["own"])}
configs.update({nm: ordered_call(o) for nm, o in orders.items()})
if os.path.exists("scratch/ab/lib_noswz.so"):
    NS = ctypes.CDLL(os.path.abspath("scratch/ab/lib_noswz.so"))
    NS.pcs_pure_vle_fast_ordered.argtypes = [vp, vp, ctypes.c_int64] + [vp] * 8
    configs["ordered, own order, swizzle compiled out"] = lambda: NS.pcs_pure_vle_fast_ordered(*args, vp(orders["ordered, own order"].data_ptr()), stream)
# the same parameters at a narrow, shifted tau range: what the tau key is worth when the data do not span 0.55-0.90
T3 = P[:, 2] * 1.28 * P[:, 0] ** 0.45 * np.random.default_rng(78).uniform(0.70, 0.80, n)
T3d = torch.from_numpy(T3).cuda()
args3 = (vp(Pd.data_ptr()), vp(T3d.data_ptr())) + args[2:]
o3 = torch.empty(n, dtype=torch.int32, device="cuda")
assert new.pcs_pure_row_order(vp(Pd.data_ptr()), vp(T3d.data_ptr()), n, vp(o3.data_ptr()), stream) == 0
cls_only = orders["ordered, class only R=16384"]
o3p, o3x = device_order(Pd, parent, T3d), device_order(P2d, new, T3d)
narrow = {"tau 0.70-0.80: new, plain entry": lambda: new.pcs_pure_vle_fast(*args3, stream),
          "tau 0.70-0.80: parent, ordered, own order": ordered_call(o3p, parent, args3),
          "tau 0.70-0.80: ordered, perturbed-parameter order": ordered_call(o3x, new, args3),
          "tau 0.70-0.80: ordered, own order": lambda: new.pcs_pure_vle_fast_ordered(*args3, vp(o3.data_ptr()), stream),
          "tau 0.70-0.80: ordered, class only": lambda: new.pcs_pure_vle_fast_ordered(*args3, vp(cls_only.data_ptr()), stream)}
res, ref = {}, None
for nm, call in list(configs.items()) + list(narrow.items()):  # warm-up, and the results (each batch against its first configuration)
    if nm == next(iter(narrow)): ref = None
    p.zero_(); st.zero_()
    assert call() == 0
    torch.cuda.synchronize()
    entries = int(ws[0].item())
    assert new.pcs_pure_vle_retry(*(args3 if nm in narrow else args), stream) == 0
    torch.cuda.synchronize()
    cur = (p.cpu().numpy().copy(), st.cpu().numpy().copy())
    if ref is None: ref = cur
    res[nm] = {"failed": int(cur[1].sum()), "list_entries": entries, "status_diff_vs_first": int((cur[1] != ref[1]).sum()),
               "p_sat_bits_differing": int((cur[0].view(np.int64) != ref[0].view(np.int64)).sum())}
    print(nm, res[nm], flush=True)
o = torch.empty(n, dtype=torch.int32, device="cuda")
tb = []
for _ in range(5):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10): new.pcs_pure_row_order(vp(Pd.data_ptr()), vp(Td.data_ptr()), n, vp(o.data_ptr()), stream)
    e1.record(); torch.cuda.synchronize(); tb.append(e0.elapsed_time(e1) / 10)
print(f"pcs_pure_row_order: median {np.median(tb):.4f} ms  range {min(tb):.4f} .. {max(tb):.4f}", flush=True)
configs.update(narrow)
names = list(configs)
times = {nm: [] for nm in names}
for alt in range(ALT + 1):
    for nm in (names if alt % 2 == 0 else names[::-1]):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(LAUNCHES): configs[nm]()
        e1.record(); torch.cuda.synchronize()
        if alt >= 1: times[nm].append(e0.elapsed_time(e1) / LAUNCHES)
base, obase = float(np.median(times[names[0]])), float(np.median(times["parent, ordered, own order"]))
for nm in names:
    t = np.array(times[nm])
    res[nm].update(median_ms=float(np.median(t)), min_ms=float(t.min()), max_ms=float(t.max()), ratio_parent_over_this=base / float(np.median(t)),
                   ratio_parent_ordered_over_this=obase / float(np.median(t)), blocks_ms=[round(float(x), 5) for x in t])
    print(f"{nm:50s} median {np.median(t):.4f} ms  range {t.min():.4f} .. {t.max():.4f}  x{base / np.median(t):.4f} (plain parent)  x{obase / np.median(t):.4f} (ordered parent)", flush=True)
if out:
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    json.dump({"rows": n, "alternations": ALT, "launches_per_block": LAUNCHES, "row_order_ms": float(np.median(tb)), "configs": res}, open(out, "w"), indent=1)
