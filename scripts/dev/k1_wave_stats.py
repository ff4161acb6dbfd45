"""Per-wave statistics of the fp32 pre-solve of the pressure-only kernel for the waves as k_pure_vle<true, false> forms them
(256-row counting sort by class) and as k_pure_vle_ordered does (64 consecutive positions of the order of pcs_pure_row_order,
built by the product library), on the 1e7 bench rows.  A lane's own counts do not depend on its wave, so one call of
pcs_pure_order_key gives them per row (liquid-root evaluations, coupled iterations, full liquid / vapour evaluations in a
coupled iteration >= 2: no diagnostic build is needed) and the waves are formed here; a wave executes the maximum over its lanes.
  python scripts/dev/k1_wave_stats.py [--out FILE.json]"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))); sys.path.insert(0, ROOT); os.chdir(ROOT)
import numpy as np, torch
from feos_torch_amd import native
from feos_torch_amd.synthetic import pure_batch
argv = sys.argv[1:]
out = argv[1] if len(argv) > 1 and argv[0] == "--out" else None
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
key = torch.empty(n, dtype=torch.int32, device="cuda"); raw = torch.empty((n, 4), dtype=torch.int32, device="cuda")
native._call(key.device, "pcs_pure_order_key", Pd, Td, n, key, raw)
torch.cuda.synchronize()
word = raw[:, 0].cpu().numpy().astype(np.int64) & 0xFFFFFFFF
nliq, ncpl, re2, fv2, usable = word & 0xff, (word >> 8) & 0xff, (word >> 24) & 1, (word >> 25) & 1, (word >> 31) & 1
res = {"rows": n, "unusable_rows": int((usable == 0).sum()),
       "per_lane": {"liquid_root_evals": float(nliq.mean()), "coupled_iterations": float(ncpl.mean()),
                    "full_liquid_eval_in_iteration_ge_2": float(re2.mean()), "full_vapour_eval_in_iteration_ge_2": float(fv2.mean())}}
print("per lane", json.dumps(res["per_lane"]), flush=True)
for nm, o in orders.items():
    w = lambda x: x[o].reshape(-1, 64)
    res[nm] = {"liquid_root_evals_per_wave": float(w(nliq).max(axis=1).mean()), "coupled_iterations_per_wave": float(w(ncpl).max(axis=1).mean()),
               "waves_with_full_liquid_eval_in_iteration_ge_2": float(w(re2).max(axis=1).mean()),
               "waves_with_full_vapour_eval_in_iteration_ge_2": float(w(fv2).max(axis=1).mean()),
               "waves_with_a_polar_lane": float(w(polar).any(axis=1).mean()), "waves_with_an_associating_lane": float(w(assoc).any(axis=1).mean()),
               "liquid_hist": np.bincount(w(nliq).max(axis=1), minlength=8)[:8].tolist(), "coupled_hist": np.bincount(w(ncpl).max(axis=1), minlength=10)[:10].tolist()}
    print(nm, json.dumps(res[nm]), flush=True)
if out:
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    json.dump(res, open(out, "w"), indent=1)
