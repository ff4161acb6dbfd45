#!/usr/bin/env python3
"""Secondary configs of BASELINE.json (not the headline line of bench.py): kernel times measured
with HIP events on the launch stream, inputs resident in HBM.
  config 3: PcSaftPure liquid_density + equilibrium_liquid_density, batch 1e7
  config 4: PcSaftMix bubble / dew point, batch 1e6
  config 5: GcPcSaftMix bubble / dew point, batch 1e6
  stability: tangent-plane stability analysis (pcs_mix_stability / pcs_gc_stability) of the converged bubble and dew
             feeds of configs 4 and 5 (the specified phase at the solution), batch 1e6 minus the failed rows
  critical: PcSaftPure.critical_point kernels, batch 1e6 and 1e7 (forward, forward + backward, vapor_pressure alongside)
  boiling: PcSaftPure.boiling_temperature kernels, batch 1e6 and 1e7 (forward, forward + backward at the same process's
           vapour pressures, vapor_pressure alongside)
  enthalpy: PcSaftPure.enthalpy_of_vaporization kernels, batch 1e6 and 1e7 (forward, forward + backward, vapor_pressure and
            the all-fp64 VLE solve pcs_pure_vle_fp64 alongside, failed rows by class)
  mix_temperature: PcSaftMix.bubble_temperature / dew_temperature kernel (pcs_mix_bubble_dew_temperature), batch 1e6 minus the
            rows bubble_point / dew_point fail on, at the pressures those give at the batch temperatures, started 5 % below
            the answer; bubble_point / dew_point alongside, trial histogram and failed rows
  mix_incipient: the backward kernels of bubble_point / dew_point on the converged rows of config 4: pcs_mix_jacobian (pressure
            gradient, the default) next to pcs_mix_point_jacobian with the pressure block only, the composition block only and
            both (incipient_molefracs=True); the fused call has to cost less than two pcs_mix_jacobian launches
  gc_temperature: GcPcSaftMix.bubble_temperature / dew_temperature kernel (pcs_gc_bubble_dew_temperature), batch 1e6 minus the
            rows bubble_point / dew_point fail on, at the pressures those give at the batch temperatures, started 5 % below
            the answer; bubble_point / dew_point alongside, trial histogram and failed rows
  gc_incipient: the backward kernels of GcPcSaftMix.bubble_point / dew_point on the converged rows of config 5, class-ordered:
            pcs_gc_jacobian next to pcs_gc_point_jacobian (pressure block only, composition block only, both) and
            pcs_gc_segment_gradient next to pcs_gc_point_segment_gradient (gout_p only, gout_y only, both); the comparison is
            against the parent kernels run in the same process
  density: PcSaftMix.liquid_density / vapor_density kernel (pcs_mix_density) on mix_batch(1e6) at 3 x the bubble pressure
            (liquid) / 0.5 x the dew pressure (vapour) of the same process's bubble_point / dew_point (1e5 Pa where those fail);
            pcs_mix_derivatives and the bubble / dew solve alongside, forward + backward through the model class, failed rows
            and the histogram of evaluations per row
  gc_density: GcPcSaftMix.liquid_density / vapor_density kernel (pcs_gc_density) on gc_batch(1e6) in class order at 3 x the
            bubble pressure (liquid) / 0.5 x the dew pressure (vapour) of the same process's bubble_point / dew_point (1e5 Pa
            where those fail); pcs_gc_derivatives and the bubble / dew solve alongside, the same kernel without the class
            order, forward + backward through the model class, failed rows and the histogram of evaluations per row
  henry: PcSaftMix.henrys_law_constant kernel (pcs_mix_henry) on mix_batch(1e6), either solute; next to it what the same number
            costs without it -- pcs_pure_vle_fp64 on the solvent rows plus pcs_mix_derivatives at (rho_L, 0) with the gathers
            between them, and each of the two alone --, forward + backward through the model class, failed rows
  gc_saturation: GcPcSaftMix.vapor_pressure / equilibrium_liquid_density kernel (pcs_gc_pure_vle) on gc_batch(1e6) in class order,
            either component, at 0.7 x the critical-temperature estimate of gc_batch for that molecule; next to it the liquid
            plus the vapour pcs_gc_density call at the resulting p_sat on the same rows (x = 1 / x = 0), forward + backward
            through the model class, failed rows and the histogram of evaluations per row
  gc_henry: GcPcSaftMix.henrys_law_constant kernel (pcs_gc_henry) on gc_batch(1e6) in class order, either solute, at 0.7 x the
            critical-temperature estimate of gc_batch for the SOLVENT; next to it what the same number costs without it --
            pcs_gc_pure_vle on the solvent plus pcs_gc_derivatives at (rho_L, 0) --, forward + backward through the model class,
            failed rows
Prints one JSON object per config."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from feos_torch_amd import native
from feos_torch_amd.gc_pcsaft import build_table, encode_rows
from feos_torch_amd.synthetic import gc_batch, load_segment_table, mix_batch, pure_batch, pure_pressures

d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()


def timed(fn, reps=5):
    fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); out = fn(); e1.record(); torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts)), out


def stability_feeds(r, dew):
    """(row indices, feed partial densities) of the converged rows: the specified phase of the solution"""
    ok = torch.nonzero(~r["status"]).view(-1)
    rho4 = r["rho4"][ok]
    return ok, (rho4[:, 0:2] if dew else rho4[:, 2:4]).contiguous()


which = sys.argv[1:] or ["3", "4", "5"]
if "3" in which:
    n = 10_000_000
    P, T = pure_batch(n); pp = pure_pressures(n)
    Pd, Td, pd = d(P), d(T), d(pp)
    ms, r = timed(lambda: native.pure_liquid_density(Pd, Td, pd))
    ms2, r2 = timed(lambda: native.pure_vle(Pd, Td, want_p=False, want_rho_eq=True))
    print(json.dumps({"config": "PcSaftPure liquid_density batch=1e7", "ms": ms, "rows_per_s": n / ms * 1e3, "failed": int(r["status"].sum())}))
    print(json.dumps({"config": "PcSaftPure equilibrium_liquid_density batch=1e7", "ms": ms2, "rows_per_s": n / ms2 * 1e3, "failed": int(r2["status"].sum())}))
if "4" in which:
    n = 1_000_000
    P, K, T, X, PI = mix_batch(n)
    a = [d(v) for v in (P, K, T, X, PI)]
    for dew in (False, True):
        ms, r = timed(lambda: native.mix_bubble_dew(*a, dew), reps=3)
        print(json.dumps({"config": f"PcSaftMix {'dew' if dew else 'bubble'} point batch=1e6", "ms": ms, "rows_per_s": n / ms * 1e3, "failed": int(r["status"].sum())}))
    r = native.mix_bubble_dew(*a, False)
    ms, _ = timed(lambda: native.mix_jacobian(a[0], a[1], a[2], r["rho4"], False), reps=3)
    print(json.dumps({"config": "PcSaftMix bubble Jacobian batch=1e6", "ms": ms, "rows_per_s": n / ms * 1e3}))
if "5" in which:
    n = 1_000_000
    table = load_segment_table(os.path.join(ROOT, "tests", "data", "sauer2014_hetero.json"))
    b = gc_batch(n, table); ident = [s for s, _ in table]
    from feos_torch_amd.gc_pcsaft import encode_rows_device
    encode_rows_device(ident, b["segment_lists"][:1000], b["bond_lists"][:1000], "cuda")  # warm (allocator, kernels)
    torch.cuda.synchronize()
    t0 = time.time(); rows = encode_rows_device(ident, b["segment_lists"], b["bond_lists"], "cuda"); torch.cuda.synchronize()
    t_enc = time.time() - t0  # host encoding of the distinct molecules + row indices, H2D of 8 B per row, row assembly on the GPU
    seg = torch.tensor(np.stack([v for _, v in table]), dtype=torch.float64)
    kab = torch.zeros((len(ident), len(ident)), dtype=torch.float64)
    for s1, s2, k in b["kab_list"]:
        kab[ident.index(s1), ident.index(s2)] = k; kab[ident.index(s2), ident.index(s1)] = k
    tab = build_table(seg.cuda(), kab.cuda())
    phi, T, x, p0 = d(b["phi"]), d(b["T"]), d(b["x"]), d(b["p_init"])
    order = native.gc_class_order(tab, len(ident), rows)  # once per model, as GcPcSaftMix does
    for dew in (False, True):
        ms, r = timed(lambda: native.gc_bubble_dew(tab, len(ident), rows, phi, T, x, p0, dew, order=order), reps=3)
        print(json.dumps({"config": f"GcPcSaftMix {'dew' if dew else 'bubble'} point batch=1e6", "ms": ms, "rows_per_s": n / ms * 1e3, "failed": int(r["status"].sum()), "host_encode_s": t_enc}))
if "stability" in which:
    n = 1_000_000
    P, K, T, X, PI = mix_batch(n)
    a = [d(v) for v in (P, K, T, X, PI)]
    for dew in (False, True):
        ok, feed = stability_feeds(native.mix_bubble_dew(*a, dew), dew)
        Pk, Kk, Tk = a[0][ok].contiguous(), a[1][ok].contiguous(), a[2][ok].contiguous()
        ms, r = timed(lambda: native.mix_stability(Pk, Kk, Tk, feed), reps=3)
        cnt = torch.bincount(r["status"].long(), minlength=4).tolist()
        print(json.dumps({"config": f"PcSaftMix stability of the {'dew' if dew else 'bubble'} feeds batch={len(ok)}", "ms": ms,
                          "rows_per_s": len(ok) / ms * 1e3, "status_counts": cnt, "flagged_fraction": 1.0 - cnt[0] / len(ok)}))
    table = load_segment_table(os.path.join(ROOT, "tests", "data", "sauer2014_hetero.json"))
    b = gc_batch(n, table); ident = [s for s, _ in table]
    from feos_torch_amd.gc_pcsaft import encode_rows_device
    rows = encode_rows_device(ident, b["segment_lists"], b["bond_lists"], "cuda")
    seg = torch.tensor(np.stack([v for _, v in table]), dtype=torch.float64)
    kab = torch.zeros((len(ident), len(ident)), dtype=torch.float64)
    for s1, s2, k in b["kab_list"]:
        kab[ident.index(s1), ident.index(s2)] = k; kab[ident.index(s2), ident.index(s1)] = k
    tab = build_table(seg.cuda(), kab.cuda())
    phi, T, x, p0 = d(b["phi"]), d(b["T"]), d(b["x"]), d(b["p_init"])
    order = native.gc_class_order(tab, len(ident), rows)
    for dew in (False, True):
        ok, feed = stability_feeds(native.gc_bubble_dew(tab, len(ident), rows, phi, T, x, p0, dew, order=order), dew)
        rows_ok, phi_ok, T_ok = rows[ok].contiguous(), phi[ok].contiguous(), T[ok].contiguous()
        order_ok = native.gc_class_order(tab, len(ident), rows_ok)
        ms, r = timed(lambda: native.gc_stability(tab, len(ident), rows_ok, phi_ok, T_ok, feed, order=order_ok), reps=3)
        cnt = torch.bincount(r["status"].long(), minlength=4).tolist()
        print(json.dumps({"config": f"GcPcSaftMix stability of the {'dew' if dew else 'bubble'} feeds batch={len(ok)}", "ms": ms,
                          "rows_per_s": len(ok) / ms * 1e3, "status_counts": cnt, "flagged_fraction": 1.0 - cnt[0] / len(ok)}))
if "critical" in which:
    # critical points of the pure_batch parameter rows: forward (pcs_pure_critical_point) and forward + backward
    # (+ pcs_pure_critical_point_vjp with all three cotangents), next to vapor_pressure from the same process
    for n in (1_000_000, 10_000_000):
        P, T = pure_batch(n)
        Pd, Td = d(P), d(T)
        g = [torch.ones(n, dtype=torch.float64, device="cuda") for _ in range(3)]
        ms_vp, _ = timed(lambda: native.pure_vapor_pressure(Pd, Td))
        ms, r = timed(lambda: native.pure_critical_point(Pd, want_iters=True), reps=3)

        def fwd_bwd():
            r = native.pure_critical_point(Pd)
            return native.pure_critical_point_vjp(Pd, r["t_c"], r["rho_c"], *g)

        ms_fb, _ = timed(fwd_bwd, reps=3)
        failed = r["status"]
        polar, assoc = Pd[:, 3] != 0, Pd[:, 4] != 0
        by_class = {name: int((failed & (polar == a) & (assoc == b)).sum())
                    for name, a, b in (("plain", False, False), ("polar", True, False), ("assoc", False, True), ("polar+assoc", True, True))}
        it = torch.bincount(r["iters"][~failed].long()).tolist()
        print(json.dumps({"config": f"PcSaftPure critical_point batch={n:.0e}", "ms": ms, "rows_per_s": n / ms * 1e3, "ms_forward_backward": ms_fb,
                          "ms_vapor_pressure": ms_vp, "failed": int(failed.sum()), "failed_by_class": by_class, "newton_iterations": it}))
if "boiling" in which:
    # boiling temperatures of the pure_batch rows at the pressures vapor_pressure gives at the batch temperatures (so every
    # solved row has an answer: the batch temperature): forward (pcs_pure_boiling_temperature) and forward + backward
    # (+ pcs_pure_jacobian_vjp with selector 3), next to vapor_pressure from the same process
    for n in (1_000_000, 10_000_000):
        P, T = pure_batch(n)
        Pd, Td = d(P), d(T)
        g = torch.ones(n, dtype=torch.float64, device="cuda")
        ms_vp, vp = timed(lambda: native.pure_vapor_pressure(Pd, Td))
        keep = torch.nonzero(~vp["status"]).view(-1)
        Pk, Tk, pk, gk = Pd[keep].contiguous(), Td[keep].contiguous(), vp["p_sat"][keep].contiguous(), g[keep].contiguous()
        ms, r = timed(lambda: native.pure_boiling_temperature(Pk, pk, want_iters=True), reps=3)

        def fwd_bwd():
            r = native.pure_boiling_temperature(Pk, pk)
            return native.pure_jacobian_vjp("boiling_temperature", Pk, r["t"], None, r["rho_vl"], gk, (True, False, True))

        ms_fb, _ = timed(fwd_bwd, reps=3)
        ok = ~r["status"]
        err = float(((r["t"][ok] / Tk[ok]) - 1.0).abs().max()) if bool(ok.any()) else float("nan")
        it = torch.bincount(r["iters"][ok].long()).tolist()
        print(json.dumps({"config": f"PcSaftPure boiling_temperature batch={n:.0e}", "rows": len(keep), "ms": ms, "rows_per_s": len(keep) / ms * 1e3,
                          "ms_forward_backward": ms_fb, "ms_vapor_pressure": ms_vp, "failed": int(r["status"].sum()),
                          "max_rel_round_trip": err, "outer_iterations": it}))
if "enthalpy" in which:
    # enthalpies of vaporization of the pure_batch rows at the batch temperatures: forward (pcs_pure_enthalpy_of_vaporization
    # with the densities the backward pass needs) and forward + backward (+ pcs_pure_enthalpy_of_vaporization_vjp), next to
    # vapor_pressure and the all-fp64 VLE solve (the forward pass is that solve plus the polish and two tangent evaluations)
    for n in (1_000_000, 10_000_000):
        P, T = pure_batch(n)
        Pd, Td = d(P), d(T)
        g = torch.ones(n, dtype=torch.float64, device="cuda")
        ms_vp, vp = timed(lambda: native.pure_vapor_pressure(Pd, Td))
        ms_vle, _ = timed(lambda: native.pure_vle(Pd, Td, want_p=True, want_rho_vl=True, all_fp64=True))
        ms, r = timed(lambda: native.pure_enthalpy_of_vaporization(Pd, Td, want_rho_vl=True), reps=3)

        def fwd_bwd():
            r = native.pure_enthalpy_of_vaporization(Pd, Td, want_rho_vl=True)
            return native.pure_enthalpy_of_vaporization_vjp(Pd, Td, r["rho_vl"], g)

        ms_fb, _ = timed(fwd_bwd, reps=3)
        failed = r["status"]
        polar, assoc = Pd[:, 3] != 0, Pd[:, 4] != 0
        by_class = {name: int((failed & (polar == a) & (assoc == b)).sum())
                    for name, a, b in (("plain", False, False), ("polar", True, False), ("assoc", False, True), ("polar+assoc", True, True))}
        print(json.dumps({"config": f"PcSaftPure enthalpy_of_vaporization batch={n:.0e}", "ms": ms, "rows_per_s": n / ms * 1e3,
                          "ms_forward_backward": ms_fb, "ms_vapor_pressure": ms_vp, "ms_vle_fp64": ms_vle, "failed": int(failed.sum()),
                          "failed_by_class": by_class, "failed_vapor_pressure": int(vp["status"].sum()),
                          "failed_here_only": int((failed & ~vp["status"]).sum())}))
if "mix_temperature" in which:
    # bubble / dew temperatures of the mix_batch rows at the pressures bubble_point / dew_point give at the batch temperatures
    # (so every solved row has an answer: the batch temperature), started 5 % below it.  One row per lane, no work queue: a
    # wave pays its slowest row, unlike the pressure solve it is reported next to
    n = 1_000_000
    P, K, T, X, PI = mix_batch(n)
    a = [d(v) for v in (P, K, T, X, PI)]
    for dew in (False, True):
        ms_p, rp = timed(lambda: native.mix_bubble_dew(*a, dew), reps=3)
        keep = torch.nonzero(~rp["status"]).view(-1)
        Pk, Kk, Tk, Xk, pk = a[0][keep].contiguous(), a[1][keep].contiguous(), a[2][keep].contiguous(), a[3][keep].contiguous(), rp["p"][keep].contiguous()
        T0 = 0.95 * Tk
        ms, r = timed(lambda: native.mix_bubble_dew_temperature(Pk, Kk, pk, Xk, T0, dew, want_iters=True), reps=3)
        ok = ~r["status"]
        err = ((r["t"][ok] / Tk[ok]) - 1.0).abs()
        print(json.dumps({"config": f"PcSaftMix {'dew' if dew else 'bubble'} temperature batch={len(keep)}", "ms": ms, "rows_per_s": len(keep) / ms * 1e3,
                          "ms_pressure_solve_1e6": ms_p, "failed": int(r["status"].sum()), "trials": torch.bincount(r["iters"][ok].long()).tolist(),
                          "round_trip_above_1e-9": int((err > 1e-9).sum()), "median_rel_round_trip": float(err.median())}))
if "mix_incipient" in which:
    # gradients at the converged rows of mix_batch(1e6), both problems, median of 3 in this process.  "both" shares the
    # coefficient set, the two phase evaluations and the 3x3 elimination between the blocks; the adjoint passes are per block
    n = 1_000_000
    P, K, T, X, PI = mix_batch(n)
    a = [d(v) for v in (P, K, T, X, PI)]
    for dew in (False, True):
        r = native.mix_bubble_dew(*a, dew)
        keep = torch.nonzero(~r["status"]).view(-1)
        Pk, Kk, Tk, rk = a[0][keep].contiguous(), a[1][keep].contiguous(), a[2][keep].contiguous(), r["rho4"][keep].contiguous()
        ms_jac, _ = timed(lambda: native.mix_jacobian(Pk, Kk, Tk, rk, dew), reps=3)
        ms_p, _ = timed(lambda: native.mix_point_jacobian(Pk, Kk, Tk, rk, dew, want_y=False), reps=3)
        ms_y, _ = timed(lambda: native.mix_point_jacobian(Pk, Kk, Tk, rk, dew, want_p=False), reps=3)
        ms_both, _ = timed(lambda: native.mix_point_jacobian(Pk, Kk, Tk, rk, dew), reps=3)
        print(json.dumps({"config": f"PcSaftMix {'dew' if dew else 'bubble'} point gradients batch={len(keep)}", "ms_mix_jacobian": ms_jac,
                          "ms_point_jacobian_p": ms_p, "ms_point_jacobian_y": ms_y, "ms_point_jacobian_both": ms_both,
                          "both_over_two_mix_jacobian": ms_both / (2.0 * ms_jac), "fused_pays": bool(ms_both < 2.0 * ms_jac)}))
if "gc_temperature" in which:
    # bubble / dew temperatures of the gc_batch rows at the pressures bubble_point / dew_point give at the batch temperatures
    # (so every solved row has an answer: the batch temperature), started 5 % below it, in the class order of the kept rows.
    # One row per lane, no work queue; the pressure solve it is reported next to runs its fast pass + retry list
    n = 1_000_000
    table = load_segment_table(os.path.join(ROOT, "tests", "data", "sauer2014_hetero.json"))
    b = gc_batch(n, table); ident = [s for s, _ in table]
    from feos_torch_amd.gc_pcsaft import encode_rows_device
    rows = encode_rows_device(ident, b["segment_lists"], b["bond_lists"], "cuda")
    seg = torch.tensor(np.stack([v for _, v in table]), dtype=torch.float64)
    kab = torch.zeros((len(ident), len(ident)), dtype=torch.float64)
    for s1, s2, k in b["kab_list"]:
        kab[ident.index(s1), ident.index(s2)] = k; kab[ident.index(s2), ident.index(s1)] = k
    tab, S = build_table(seg.cuda(), kab.cuda()), len(ident)
    phi, T, x, p0 = d(b["phi"]), d(b["T"]), d(b["x"]), d(b["p_init"])
    order = native.gc_class_order(tab, S, rows)
    for dew in (False, True):
        ms_p, rp = timed(lambda: native.gc_bubble_dew(tab, S, rows, phi, T, x, p0, dew, order=order), reps=3)
        keep = torch.nonzero(~rp["status"]).view(-1)
        rk, fk, Tk, xk, pk = rows[keep].contiguous(), phi[keep].contiguous(), T[keep].contiguous(), x[keep].contiguous(), rp["p"][keep].contiguous()
        ok_order = native.gc_class_order(tab, S, rk)
        T0 = 0.95 * Tk
        ms, r = timed(lambda: native.gc_bubble_dew_temperature(tab, S, rk, fk, pk, xk, T0, dew, want_iters=True, order=ok_order), reps=3)
        ms_plain, _ = timed(lambda: native.gc_bubble_dew_temperature(tab, S, rk, fk, pk, xk, T0, dew), reps=3)
        ok = ~r["status"]
        err = ((r["t"][ok] / Tk[ok]) - 1.0).abs()
        print(json.dumps({"config": f"GcPcSaftMix {'dew' if dew else 'bubble'} temperature batch={len(keep)}", "ms": ms, "rows_per_s": len(keep) / ms * 1e3,
                          "ms_without_class_order": ms_plain, "ms_pressure_solve_1e6": ms_p, "failed": int(r["status"].sum()),
                          "trials": torch.bincount(r["iters"][ok].long()).tolist(), "round_trip_above_1e-9": int((err > 1e-9).sum()),
                          "median_rel_round_trip": float(err.median())}))
if "gc_incipient" in which:
    # gradients at the converged rows of gc_batch(1e6) in the class order of the kept rows, both problems, median of 3 in this
    # process.  The per-row kernel shares the coefficient set, both phase evaluations, the elimination and the T direction
    # between the blocks; the table kernel folds both upstream gradients into one (alpha, beta) and runs one pass
    n = 1_000_000
    table = load_segment_table(os.path.join(ROOT, "tests", "data", "sauer2014_hetero.json"))
    b = gc_batch(n, table); ident = [s for s, _ in table]
    from feos_torch_amd.gc_pcsaft import encode_rows_device
    rows = encode_rows_device(ident, b["segment_lists"], b["bond_lists"], "cuda")
    seg = torch.tensor(np.stack([v for _, v in table]), dtype=torch.float64)
    kab = torch.zeros((len(ident), len(ident)), dtype=torch.float64)
    for s1, s2, k in b["kab_list"]:
        kab[ident.index(s1), ident.index(s2)] = k; kab[ident.index(s2), ident.index(s1)] = k
    tab, S = build_table(seg.cuda(), kab.cuda()), len(ident)
    phi, T, x, p0 = d(b["phi"]), d(b["T"]), d(b["x"]), d(b["p_init"])
    for dew in (False, True):
        r = native.gc_bubble_dew(tab, S, rows, phi, T, x, p0, dew, order=native.gc_class_order(tab, S, rows))
        keep = torch.nonzero(~r["status"]).view(-1)
        rk, pk, Tk, r4 = rows[keep].contiguous(), phi[keep].contiguous(), T[keep].contiguous(), r["rho4"][keep].contiguous()
        od = native.gc_class_order(tab, S, rk)
        gp = 1.0 / r["p"][keep].contiguous()
        gy = torch.ones(len(keep), dtype=torch.float64, device="cuda")
        args = (tab, S, rk, pk, Tk, r4, dew)
        ms = {}
        ms["gc_jacobian"], _ = timed(lambda: native.gc_jacobian(*args, order=od), reps=3)
        ms["point_jacobian_p"], _ = timed(lambda: native.gc_point_jacobian(*args, want_y=False, order=od), reps=3)
        ms["point_jacobian_y"], _ = timed(lambda: native.gc_point_jacobian(*args, want_p=False, order=od), reps=3)
        ms["point_jacobian_both"], _ = timed(lambda: native.gc_point_jacobian(*args, order=od), reps=3)
        ms["segment_gradient"], _ = timed(lambda: native.gc_segment_gradient(*args, gout=gp, order=od), reps=3)
        ms["point_segment_gradient_p"], _ = timed(lambda: native.gc_point_segment_gradient(*args, gout_p=gp, order=od), reps=3)
        ms["point_segment_gradient_y"], _ = timed(lambda: native.gc_point_segment_gradient(*args, gout_y=gy, order=od), reps=3)
        ms["point_segment_gradient_both"], _ = timed(lambda: native.gc_point_segment_gradient(*args, gout_p=gp, gout_y=gy, order=od), reps=3)
        print(json.dumps({"config": f"GcPcSaftMix {'dew' if dew else 'bubble'} point gradients batch={len(keep)}",
                          **{"ms_" + k: v for k, v in ms.items()},
                          "jacobian_both_over_two_single": ms["point_jacobian_both"] / (ms["point_jacobian_p"] + ms["point_jacobian_y"]),
                          "jacobian_both_over_two_gc_jacobian": ms["point_jacobian_both"] / (2.0 * ms["gc_jacobian"]),
                          "segment_both_over_two_single": ms["point_segment_gradient_both"] / (ms["point_segment_gradient_p"] + ms["point_segment_gradient_y"]),
                          "segment_both_over_two_segment_gradient": ms["point_segment_gradient_both"] / (2.0 * ms["segment_gradient"])}))
if "density" in which:
    # one row per lane in batch order, no work queue: a wave pays its slowest row.  The neighbours on the same rows: one state
    # evaluation (pcs_mix_derivatives at the root) and the bubble / dew solve that gave the pressure
    from feos_torch_amd import PcSaftMix
    n = 1_000_000
    P, K, T, X, PI = mix_batch(n)
    a = [d(v) for v in (P, K, T, X, PI)]
    for phase, factor in ((0, 3.0), (1, 0.5)):
        ms_point, rp = timed(lambda: native.mix_bubble_dew(*a, bool(phase)), reps=3)
        p = torch.where(rp["status"], torch.full_like(rp["p"], 1e5), factor * rp["p"]).contiguous()
        ms, r = timed(lambda: native.mix_density(a[0], a[1], a[2], p, a[3], phase), reps=5)
        ok = ~r["status"]
        rho2 = torch.stack((a[3] * r["rho"], (1.0 - a[3]) * r["rho"]), dim=1).contiguous()
        rho2[r["status"]] = 5e-3
        ms_deriv, _ = timed(lambda: native.mix_derivatives(a[0], a[1], a[2], rho2), reps=5)

        def fwd_bwd():
            leaves = [v.clone().requires_grad_(True) for v in (a[0], a[1], a[2], p, a[3])]
            m = PcSaftMix(leaves[0], leaves[1])
            rho, _ = (m.vapor_density if phase else m.liquid_density)(*leaves[2:])
            rho.sum().backward()
            return leaves[0].grad
        ms_fb, _ = timed(fwd_bwd, reps=3)
        print(json.dumps({"config": f"PcSaftMix {'vapor' if phase else 'liquid'}_density batch={n:.0e}", "ms": ms, "rows_per_s": n / ms * 1e3,
                          "ms_mix_derivatives": ms_deriv, "ms_bubble_dew_point": ms_point, "ms_forward_backward": ms_fb,
                          "failed": int(r["status"].sum()), "failed_point": int(rp["status"].sum()),
                          "evaluations": torch.bincount(r["iters"][ok].long()).tolist()}))
if "gc_density" in which:
    # one row per lane in class order, no work queue: a wave pays its slowest row.  The neighbours on the same rows: one state
    # evaluation (pcs_gc_derivatives at the root) and the bubble / dew solve that gave the pressure
    from feos_torch_amd import GcPcSaftMix
    n = 1_000_000
    table = load_segment_table(os.path.join(ROOT, "tests", "data", "sauer2014_hetero.json"))
    b = gc_batch(n, table); ident = [s for s, _ in table]
    par = tuple(torch.tensor([v[k] for _, v in table], dtype=torch.float64, requires_grad=True) for k in range(8))
    phi_leaf = d(b["phi"]).requires_grad_(True)
    model = GcPcSaftMix(ident, par, b["segment_lists"], b["bond_lists"], b["kab_list"], phi_leaf)
    tab, S, rows = model._table(), model.S, model.rows
    phi, T, x, p0 = phi_leaf.detach(), d(b["T"]), d(b["x"]), d(b["p_init"])
    order = native.gc_class_order(tab, S, rows)
    for phase, factor in ((0, 3.0), (1, 0.5)):
        ms_point, rp = timed(lambda: native.gc_bubble_dew(tab, S, rows, phi, T, x, p0, bool(phase), order=order), reps=3)
        p = torch.where(rp["status"], torch.full_like(rp["p"], 1e5), factor * rp["p"]).contiguous()
        ms, r = timed(lambda: native.gc_density(tab, S, rows, phi, T, p, x, phase, order=order), reps=5)
        ms_plain, r_plain = timed(lambda: native.gc_density(tab, S, rows, phi, T, p, x, phase), reps=5)
        same = all(torch.equal(r[k], r_plain[k]) for k in ("rho", "dpdrho", "status", "iters"))
        ok = ~r["status"]
        rho2 = torch.stack((x * r["rho"], (1.0 - x) * r["rho"]), dim=1).contiguous()
        rho2[r["status"]] = 5e-3
        ms_deriv, _ = timed(lambda: native.gc_derivatives(tab, S, rows, phi, T, rho2), reps=5)

        def fwd_bwd():
            model.rows, model.phi, model._order = rows, phi_leaf, order  # the call reduces the model: start from all rows
            leaves = [v.clone().requires_grad_(True) for v in (T, p, x)]
            rho, _ = (model.vapor_density if phase else model.liquid_density)(*leaves)
            rho.sum().backward()
            return leaves[0].grad
        ms_fb, _ = timed(fwd_bwd, reps=3)
        print(json.dumps({"config": f"GcPcSaftMix {'vapor' if phase else 'liquid'}_density batch={n:.0e}", "ms": ms, "rows_per_s": n / ms * 1e3,
                          "ms_without_class_order": ms_plain, "same_bits_without_class_order": bool(same), "ms_gc_derivatives": ms_deriv,
                          "ms_bubble_dew_point": ms_point, "ms_forward_backward": ms_fb, "failed": int(r["status"].sum()),
                          "failed_point": int(rp["status"].sum()), "evaluations": torch.bincount(r["iters"][ok].long()).tolist()}))
if "henry" in which:
    # one row per lane in batch order.  What a user pays today for the same number: the all-fp64 pure VLE solve on the solvent
    # rows plus one state evaluation at (rho_L, 0), with the gathers between them (the solvent's parameter row, rho_L into [n,2])
    from feos_torch_amd import PcSaftMix
    n = 1_000_000
    P, K, T, _, _ = mix_batch(n)
    a = [d(v) for v in (P, K, T)]
    for solute in (0, 1):
        v = 1 - solute
        ms, r = timed(lambda: native.mix_henry(*a, solute), reps=5)

        def unfused():
            vle = native.pure_vle(a[0][:, v, :].contiguous(), a[2], all_fp64=True)
            rho2 = torch.zeros((n, 2), dtype=torch.float64, device="cuda")
            rho2[:, v] = torch.where(vle["status"], torch.full_like(a[2], 5e-3), vle["rho_vl"][:, 1])
            return vle, native.mix_derivatives(a[0], a[1], a[2], rho2)
        ms_unfused, (vle, _) = timed(unfused, reps=5)
        Pv = a[0][:, v, :].contiguous()
        ms_vle, _ = timed(lambda: native.pure_vle(Pv, a[2], all_fp64=True), reps=5)
        rho2 = torch.zeros((n, 2), dtype=torch.float64, device="cuda")
        rho2[:, v] = torch.where(r["status"], torch.full_like(a[2], 5e-3), r["rho_vl"][:, 1])
        ms_deriv, _ = timed(lambda: native.mix_derivatives(a[0], a[1], a[2], rho2), reps=5)

        def fwd_bwd():
            leaves = [x.clone().requires_grad_(True) for x in a]
            h, _ = PcSaftMix(leaves[0], leaves[1]).henrys_law_constant(leaves[2], solute=solute)
            h.log().sum().backward()
            return leaves[0].grad
        ms_fb, _ = timed(fwd_bwd, reps=3)
        print(json.dumps({"config": f"PcSaftMix henrys_law_constant solute={solute} batch={n:.0e}", "ms": ms, "rows_per_s": n / ms * 1e3,
                          "ms_vle_fp64_plus_mix_derivatives_with_gathers": ms_unfused, "ms_pure_vle_fp64": ms_vle,
                          "ms_mix_derivatives": ms_deriv, "ms_forward_backward": ms_fb, "failed": int(r["status"].sum()),
                          "failed_pure_vle_fp64": int(vle["status"].sum())}))
if "gc_saturation" in which:
    # one row per lane in class order, no work queue: a wave pays its slowest row, and the solve is the robust one of the pure
    # path (no fp32 pre-solve).  The neighbours on the same rows: the two density roots at the p_sat this kernel returns
    from feos_torch_amd import GcPcSaftMix
    n = 1_000_000
    table = load_segment_table(os.path.join(ROOT, "tests", "data", "sauer2014_hetero.json"))
    b = gc_batch(n, table); ident = [s for s, _ in table]
    par = tuple(torch.tensor([v[k] for _, v in table], dtype=torch.float64, requires_grad=True) for k in range(8))
    phi_leaf = d(b["phi"]).requires_grad_(True)
    model = GcPcSaftMix(ident, par, b["segment_lists"], b["bond_lists"], b["kab_list"], phi_leaf)
    tab, S, rows = model._table(), model.S, model.rows
    phi = phi_leaf.detach()
    order = native.gc_class_order(tab, S, rows)
    seg_par = dict(table)
    tc_of = {}

    def tc_estimate(segs):  # the estimate gc_batch takes its temperatures from, per molecule (the lists are shared objects)
        if id(segs) not in tc_of:
            m = np.array([seg_par[s][0] for s in segs]); e = np.array([seg_par[s][2] for s in segs])
            tc_of[id(segs)] = (m * e).sum() / m.sum() * 1.28 * m.sum() ** 0.45
        return tc_of[id(segs)]
    for component in (0, 1):
        T = d(0.7 * np.array([tc_estimate(row[component]) for row in b["segment_lists"]]))
        ms, r = timed(lambda: native.gc_pure_vle(tab, S, rows, phi, T, component, order=order), reps=5)
        ms_p, _ = timed(lambda: native.gc_pure_vle(tab, S, rows, phi, T, component, order=order, want=("p_sat",)), reps=5)
        ok = ~r["status"]
        p = torch.where(ok, r["p_sat"], torch.full_like(T, 1e5)).contiguous()
        x = torch.full_like(T, 1.0 - component)
        ms_liq, rl = timed(lambda: native.gc_density(tab, S, rows, phi, T, p, x, 0, order=order), reps=5)
        ms_vap, rv = timed(lambda: native.gc_density(tab, S, rows, phi, T, p, x, 1, order=order), reps=5)

        def fwd_bwd(method):
            model.rows, model.phi, model._order = rows, phi_leaf, order  # the call reduces the model: start from all rows
            leaf = T.clone().requires_grad_(True)
            value, _ = getattr(model, method)(leaf, component=component)
            value.sum().backward()
            return leaf.grad
        ms_fb_p, _ = timed(lambda: fwd_bwd("vapor_pressure"), reps=3)
        ms_fb_rho, _ = timed(lambda: fwd_bwd("equilibrium_liquid_density"), reps=3)
        print(json.dumps({"config": f"GcPcSaftMix vapor_pressure component={component} batch={n:.0e}", "ms": ms, "rows_per_s": n / ms * 1e3,
                          "ms_p_sat_only": ms_p, "ms_gc_density_liquid_at_p_sat": ms_liq, "ms_gc_density_vapour_at_p_sat": ms_vap,
                          "over_two_density_calls": ms / (ms_liq + ms_vap), "ms_forward_backward_vapor_pressure": ms_fb_p,
                          "ms_forward_backward_equilibrium_liquid_density": ms_fb_rho, "failed": int(r["status"].sum()),
                          "failed_density_liquid": int((rl["status"] & ok).sum()), "failed_density_vapour": int((rv["status"] & ok).sum()),
                          "evaluations": torch.bincount(r["iters"][ok].long()).tolist()}))
if "gc_henry" in which:
    # the launch shape of gc_saturation; the neighbours on the same rows are the two calls the fused kernel replaces
    from feos_torch_amd import GcPcSaftMix
    n = 1_000_000
    table = load_segment_table(os.path.join(ROOT, "tests", "data", "sauer2014_hetero.json"))
    b = gc_batch(n, table); ident = [s for s, _ in table]
    par = tuple(torch.tensor([v[k] for _, v in table], dtype=torch.float64, requires_grad=True) for k in range(8))
    phi_leaf = d(b["phi"]).requires_grad_(True)
    model = GcPcSaftMix(ident, par, b["segment_lists"], b["bond_lists"], b["kab_list"], phi_leaf)
    tab, S, rows = model._table(), model.S, model.rows
    phi = phi_leaf.detach()
    order = native.gc_class_order(tab, S, rows)
    seg_par = dict(table)
    tc_of = {}

    def tc_estimate(segs):  # as in the gc_saturation mode
        if id(segs) not in tc_of:
            m = np.array([seg_par[s][0] for s in segs]); e = np.array([seg_par[s][2] for s in segs])
            tc_of[id(segs)] = (m * e).sum() / m.sum() * 1.28 * m.sum() ** 0.45
        return tc_of[id(segs)]
    for solute in (0, 1):
        v = 1 - solute
        T = d(0.7 * np.array([tc_estimate(row[v]) for row in b["segment_lists"]]))
        ms, r = timed(lambda: native.gc_henry(tab, S, rows, phi, T, solute, order=order), reps=5)
        ms_h, _ = timed(lambda: native.gc_henry(tab, S, rows, phi, T, solute, order=order, want=()), reps=5)
        ms_vle, vle = timed(lambda: native.gc_pure_vle(tab, S, rows, phi, T, v, order=order), reps=5)
        zero = torch.zeros_like(T)
        rho = torch.stack((zero, vle["rho_vl"][:, 1]) if solute == 0 else (vle["rho_vl"][:, 1], zero), dim=1).contiguous()
        ms_deriv, _ = timed(lambda: native.gc_derivatives(tab, S, rows, phi, T, rho), reps=5)

        def fwd_bwd():
            model.rows, model.phi, model._order = rows, phi_leaf, order  # the call reduces the model: start from all rows
            leaf = T.clone().requires_grad_(True)
            h, _ = model.henrys_law_constant(leaf, solute=solute)
            h.log().sum().backward()
            return leaf.grad
        ms_fb, _ = timed(fwd_bwd, reps=3)
        print(json.dumps({"config": f"GcPcSaftMix henrys_law_constant solute={solute} batch={n:.0e}", "ms": ms, "rows_per_s": n / ms * 1e3,
                          "ms_h_only": ms_h, "ms_gc_pure_vle_solvent": ms_vle, "ms_gc_derivatives_at_rho_l": ms_deriv,
                          "over_the_two_calls": ms / (ms_vle + ms_deriv), "ms_forward_backward": ms_fb, "failed": int(r["status"].sum()),
                          "failed_gc_pure_vle": int(vle["status"].sum())}))
