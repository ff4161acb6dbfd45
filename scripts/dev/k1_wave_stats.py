"""Per-wave statistics of the fp32 pre-solve of the pressure-only kernel for the waves as k_pure_vle<true, false> forms them
(256-row counting sort by class) and as k_pure_vle_ordered does (64 consecutive positions of the order of pcs_pure_row_order,
built by the product library), on the 1e7 bench rows.  A lane's own counts do not depend on its wave, so one run of a
diagnostic build gives them per row and the waves are formed here; a wave executes the maximum over its lanes.
  python scripts/dev/k1_wave_stats.py [--out FILE.json] <variant>      (scratch/ab/lib_<variant>.so)
Needs a diagnostic build as k1_nliq.py does (a copy of csrc/ whose vle_fast_lite hands `diag` of vle_presolve_f32 on):
iters = n_liq | coupled iterations << 8 | code << 16 | fp64-finish iterations << 24."""
import ctypes, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))); sys.path.insert(0, ROOT); os.chdir(ROOT)
import numpy as np, torch
from feos_torch_amd import _lib, native
from feos_torch_amd.synthetic import pure_batch
argv = sys.argv[1:]
out = None
if argv and argv[0] == "--out":
    out, argv = argv[1], argv[2:]
n = 10_000_000 // 256 * 256
P, T = pure_batch(10_000_000)
P, T = np.ascontiguousarray(P[:n]), np.ascontiguousarray(T[:n])
Pd, Td = torch.from_numpy(P).cuda(), torch.from_numpy(T).cuda()
rng = np.random.default_rng(77)
P2 = P.copy(); P2[:, :3] *= rng.uniform(0.95, 1.05, (n, 3))  # a fit that has moved, as in ab_ordered.py
polar, assoc = P[:, 3] != 0.0, (P[:, 4] != 0.0) & ((P[:, 6] != 0.0) | (P[:, 7] != 0.0))
bucket = np.where(polar, np.where(assoc, 2, 1), np.where(assoc, 3, 0))
def device_order(Pt):
    o = torch.empty(n, dtype=torch.int32, device="cuda")
    native._call(o.device, "pcs_pure_row_order", Pt, Td, n, o)
    return o.cpu().numpy().astype(np.int64)
orders = {"k_pure_vle<true, false> (256-row class sort)": (np.argsort(bucket.reshape(-1, 256), axis=1, kind="stable") + (np.arange(n // 256) * 256)[:, None]).reshape(-1),
          "k_pure_vle_ordered, own order": device_order(Pd),
          "k_pure_vle_ordered, perturbed-parameter order": device_order(torch.from_numpy(P2).cuda()),
          "k_pure_vle_ordered, class-only order (host)": np.argsort((np.arange(n) // 16384) * 4 + bucket, kind="stable"),
          "batch order, no sort": np.arange(n)}
_lib.LIB_PATH = os.path.abspath(f"scratch/ab/lib_{argv[0]}.so"); _lib._lib = None
r = native.pure_vle(Pd, Td, want_rho_vl=False, want_iters=True)
torch.cuda.synchronize()
it = r["iters"].cpu().numpy()
assert not r["status"].any().item()
nliq, ncpl, nfin = it & 0x3f, (it >> 8) & 0xff, (it >> 24) & 0xff
res = {"rows": n, "per_lane": {"liquid_root_evals": float(nliq.mean()), "coupled_iterations": float(ncpl.mean()), "fp64_finish_iterations": float(nfin.mean())}}
print("per lane", json.dumps(res["per_lane"]), flush=True)
for nm, o in orders.items():
    w = lambda x: x[o].reshape(-1, 64)
    res[nm] = {"liquid_root_evals_per_wave": float(w(nliq).max(axis=1).mean()), "coupled_iterations_per_wave": float(w(ncpl).max(axis=1).mean()),
               "fp64_finish_iterations_per_wave": float(w(nfin).max(axis=1).mean()),
               "waves_with_a_polar_lane": float(w(polar).any(axis=1).mean()), "waves_with_an_associating_lane": float(w(assoc).any(axis=1).mean()),
               "liquid_hist": np.bincount(w(nliq).max(axis=1), minlength=8)[:8].tolist(), "coupled_hist": np.bincount(w(ncpl).max(axis=1), minlength=10)[:10].tolist()}
    print(nm, json.dumps(res[nm]), flush=True)
if out:
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    json.dump(res, open(out, "w"), indent=1)
