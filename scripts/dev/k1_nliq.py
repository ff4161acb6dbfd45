# per-lane and per-wave statistics of the fp32 liquid root of k_pure_vle<true> on the first 2e6 bench rows:
#   python scripts/dev/k1_nliq.py [--out FILE.json] <variant> ...      (scratch/ab/lib_<variant>.so)
# Needs a diagnostic build (a copy of csrc/, see README.md) that writes to `iters`
#   n_liq | dense << 6 | coupled iterations << 8 | code << 16 | fp64-finish iterations << 24
# (vle_fast_lite calls vle_presolve_f32<true> with a PreSignature and packs its n_liq, n_cpl and code into the word it adds to
# res.iters; liquid_root_f32 sets bit 6 of n_eval for a lane that restarted on the dense side).  The counts alone, without the
# dense flag and the finish iterations, come from pcs_pure_order_key of the product library: k1_wave_stats.py.
# Waves are the kernel's: the 256 rows of a workgroup in the order of k1_bucket, 64 to a wave.
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))); sys.path.insert(0, ROOT); os.chdir(ROOT)
import numpy as np, torch
from feos_torch_amd import _lib, native
from feos_torch_amd.synthetic import pure_batch
argv = sys.argv[1:]
out = None
if argv and argv[0] == "--out":
    out, argv = argv[1], argv[2:]
n = 2_000_000 // 256 * 256
P, T = pure_batch(10_000_000)
P, T = np.ascontiguousarray(P[:n]), np.ascontiguousarray(T[:n])
Pd, Td = torch.from_numpy(P).cuda(), torch.from_numpy(T).cuda()
polar, assoc = P[:, 3] != 0.0, (P[:, 4] != 0.0) & ((P[:, 6] != 0.0) | (P[:, 7] != 0.0))
bucket = np.where(polar, np.where(assoc, 2, 1), np.where(assoc, 3, 0))
order = (np.argsort(bucket.reshape(-1, 256), axis=1, kind="stable") + (np.arange(n // 256) * 256)[:, None]).reshape(-1)
tau = T / (P[:, 2] * 1.28 * P[:, 0] ** 0.45)
res = {}
for nm in argv:
    _lib.LIB_PATH = os.path.abspath(f"scratch/ab/lib_{nm}.so"); _lib._lib = None
    r = native.pure_vle(Pd, Td, want_rho_vl=False, want_iters=True)
    torch.cuda.synchronize()
    it = r["iters"].cpu().numpy()
    assert not r["status"].any().item()
    nliq, dense, ncpl = it & 0x3f, ((it >> 6) & 1).astype(bool), (it >> 8) & 0xff
    w_liq, w_dense, w_cpl = nliq[order].reshape(-1, 64), dense[order].reshape(-1, 64), ncpl[order].reshape(-1, 64)
    wmax, has_dense = w_liq.max(axis=1), w_dense.any(axis=1)
    # which lane sets the wave maximum: the first lane at the maximum, by dense flag and class
    arg = order.reshape(-1, 64)[np.arange(len(wmax)), w_liq.argmax(axis=1)]
    r_ = {"rows": n, "evals_per_lane": float(nliq.mean()), "lane_hist": np.bincount(nliq, minlength=13)[:13].tolist(),
          "evals_per_wave": float(wmax.mean()), "wave_hist": np.bincount(wmax, minlength=13)[:13].tolist(),
          "dense_lane_share": float(dense.mean()), "dense_lane_evals": float(nliq[dense].mean()) if dense.any() else 0.0,
          "dense_lane_hist": np.bincount(nliq[dense], minlength=13)[:13].tolist(),
          "waves_with_dense_lane": float(has_dense.mean()), "evals_per_wave_with_dense": float(wmax[has_dense].mean()) if has_dense.any() else 0.0,
          "evals_per_wave_without_dense": float(wmax[~has_dense].mean()),
          "wave_max_set_by_dense_lane": float(dense[arg].mean()),
          "coupled_per_lane": float(ncpl.mean()), "coupled_per_wave": float(w_cpl.max(axis=1).mean()),
          "coupled_per_wave_with_dense": float(w_cpl.max(axis=1)[has_dense].mean()) if has_dense.any() else 0.0,
          "coupled_per_wave_without_dense": float(w_cpl.max(axis=1)[~has_dense].mean())}
    # the lanes that set the maximum of the waves WITHOUT a dense lane and a maximum above 2: class and T / T_c estimate
    top = arg[~has_dense & (wmax > 2)]
    r_["ordinary_wave_max_above_2"] = {"waves": int(len(top)), "by_bucket": np.bincount(bucket[top], minlength=4).tolist(),
                                       "tau_quantiles": np.quantile(tau[top], [0, 0.25, 0.5, 0.75, 1]).tolist() if len(top) else [],
                                       "evals_hist": np.bincount(nliq[top], minlength=13)[:13].tolist()}
    r_["tau_quantiles_all"] = np.quantile(tau, [0, 0.25, 0.5, 0.75, 1]).tolist()
    res[nm] = r_
    print(nm, json.dumps(r_), flush=True)
if out:
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    json.dump(res, open(out, "w"), indent=1)
