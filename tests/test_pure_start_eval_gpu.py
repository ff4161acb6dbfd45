"""GPU: the first evaluation of the fp32 liquid root in closed form at the fixed packing fraction eta0 = 0.5
(pure_eval_start_f32, csrc/pure_f32.hpp) and the root with its first iteration peeled (liquid_root_f32).

Newton converges from a wrong start as well, only later, so a wrong constant of the fixed form would hide behind the
solve: the start is pinned directly.  pcs_pure_start_probe returns (a, p, dp/drho, a') at rho = 0.5 / ceta from the
generic evaluation (pure_eval_f32) and from the fixed form; both are compared with the oracle at the same state.

The batch: 512 rows (two workgroups) of synthetic.pure_batch(seed 9107).  Rows 0-255 cycle the four classes non-polar,
polar, polar + associating, associating lane by lane (every wave is mixed), rows 256-511 are sorted by class (every wave is
class-uniform).  Every class has rows with m < 2 and m > 2 (the dipole clamp), and some associating rows carry na = 0 or
nb = 0 next to eps_AB != 0 (na nb = 0: the association branch runs, its energy vanishes).

Reference of the probe: a, p and a' from the oracle's long-double evaluation (mixn_derivatives with one component, prec=1);
dp/drho from its fp64 evaluation (pure_derivatives, written before that function had prec=1; its rounding, ~1e-13, is
seven orders below the fp32 figures compared here).  The two evaluations are required to agree on a and p to 1e-10.  ceta
from the oracle's formula in long double, rho = 0.5 / ceta rounded to double.

  E_gen, E_fix: largest deviation over the batch of the generic / the fixed form, scaled by |a| (a), rho (1 + |a'|) (p),
  |dp| (dp) and 1 + |a'| (a').  Required: E_fix <= 2 E_gen per quantity -- another rounding order, not another formula.

End to end on the same rows: p_sat of the pressure-only kernel, of pcs_pure_vapor_pressure with densities and of
pcs_pure_vle_fp64, and pcs_pure_liquid_density at 1 bar, against the long-double oracle: status equal to the oracle's mask,
values within the bars of tests/test_saturation_line_gpu.py (P_BAR; densities: saturation_grid.bar at the grid's next
reduced temperature at or above the row's own, T_c from the oracle scan).  The same for the first 1, 255 and 257 rows
(the tail clamp of the staging with the peeled iteration).

Figures (MI355X) for a: E_gen 3.218e-03, E_fix 3.218e-03 (ratio 1.00; one polar + associating row of the mixed waves whose
|a| nearly vanishes, the same deviation in both forms); by class, generic / fixed: non-polar 4.650e-04 / 3.437e-04, polar
1.343e-03 / 1.251e-04, polar + associating 3.218e-03 / 3.218e-03, associating 2.607e-05 / 2.253e-05; the two forms differ by
at most 1.218e-03 of |a|.  p, dp/drho and a' are printed by the test.  From the CPU alone: a double-precision restatement of
the fixed form is within 7e-12 (a, p, a') and 6e-10 (dp/drho, association rows) of the oracle on these rows; the oracle's own
fp64 solve differs from its long-double one by 1.21e-10 in p_sat and rho_V on row 75 (all other rows below 1e-10), so that
row sits at P_BAR by its conditioning alone.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import critical_referee as cr  # noqa: E402
import saturation_grid as sg  # noqa: E402
import test_saturation_line_gpu as saturation_line  # noqa: E402

pytestmark = pytest.mark.gpu

P_BAR = saturation_line.P_BAR
SEED, POOL, N = 9107, 4096, 512
CLASSES = ("non-polar", "polar", "polar+assoc", "assoc")  # the kernels' bucket order
VARIANTS = ("vle_p", "vp_rho", "vle_fp64")
PREFIXES = (1, 255, 257)
P_LIQ = 1e5  # Pa
QUANTITIES = ("a", "p", "dp", "mu")


def batch():
    """-> P [512, 8], T [512], class index [512] (order of CLASSES)."""
    from feos_torch_amd.synthetic import pure_batch

    P, T = pure_batch(POOL, seed=SEED)
    polar, assoc = P[:, 3] != 0.0, P[:, 4] != 0.0
    cls = np.where(polar, np.where(assoc, 2, 1), np.where(assoc, 3, 0))
    per = N // 4
    rows = [np.flatnonzero(cls == k)[:per] for k in range(4)]
    assert all(len(r) == per for r in rows)
    for r in rows:  # both sides of the dipole clamp (m = 2) in both halves of every class
        for half in (r[:per // 2], r[per // 2:]):
            assert (P[half, 0] < 2.0).any() and (P[half, 0] > 2.0).any()
    mixed = np.stack([r[:per // 2] for r in rows], axis=1).reshape(-1)  # class = row % 4
    uniform = np.concatenate([r[per // 2:] for r in rows])              # 64 rows = one wave per class
    idx = np.concatenate([mixed, uniform])
    P, T, cls = P[idx].copy(), T[idx].copy(), cls[idx]
    sites = np.flatnonzero(P[:, 4] != 0.0)
    P[sites[0::8], 6] = 0.0  # na = 0, nb != 0, eps_AB != 0
    P[sites[4::8], 7] = 0.0  # nb = 0, na != 0
    assert ((P[:, 6] * P[:, 7] == 0.0) & (P[:, 5] != 0.0) & ((P[:, 6] != 0.0) | (P[:, 7] != 0.0))).sum() >= 32
    assert np.array_equal(cls[:N // 2], np.arange(N // 2) % 4) and (np.diff(cls[N // 2:]) >= 0).all()
    return np.ascontiguousarray(P), np.ascontiguousarray(T), cls


def start_reference(orc, P, T):
    """The oracle at rho = 0.5 / ceta -> rho and dict(a, p, dp, mu) (mu = a')."""
    ld = np.longdouble
    m, sigma, eps = P[:, 0].astype(ld), P[:, 1].astype(ld), P[:, 2].astype(ld)
    d = sigma * (1 - ld("0.12") * np.exp(-3 * eps / T.astype(ld)))
    ceta = (4 * np.arctan(ld(1)) / 6) * m * d ** 3
    rho = (ld("0.5") / ceta).astype(np.float64)
    a, p, mu, _ = orc.mixn_derivatives(P[:, None, :], T, rho[:, None], prec=1)
    a64, p64, dp64 = orc.pure_derivatives(P, T, rho)
    scale = rho * (1.0 + np.abs(mu[:, 0]))
    assert np.abs(a64 - a).max() <= 1e-10 * np.abs(a).max() and (np.abs(p64 - p) <= 1e-10 * scale).all()
    return rho, {"a": a, "p": p, "dp": dp64, "mu": mu[:, 0]}


def probe(hip_lib, Pd, Td):
    n = Td.shape[0]
    out = torch.full((n, 8), float("nan"), dtype=torch.float32, device=Td.device)
    vp = ctypes.c_void_p
    rc = hip_lib.pcs_pure_start_probe(vp(Pd.data_ptr()), vp(Td.data_ptr()), n, vp(out.data_ptr()),
                                      vp(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, hip_lib.pcs_last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy().astype(np.float64)


def run_variant(name, P, T):
    from feos_torch_amd import native

    if name == "liq":
        r = native.pure_liquid_density(P, T, torch.full_like(T, P_LIQ))
        return {"status": r["status"].cpu().numpy().astype(bool), "rho": r["rho"].cpu().numpy()}
    if name == "vle_p":
        r = native.pure_vle(P, T, want_rho_vl=False)
    elif name == "vp_rho":
        r = native.pure_vapor_pressure(P, T, want_rho_vl=True)
    else:
        r = native.pure_vle(P, T, all_fp64=True)
    out = {"status": r["status"].cpu().numpy().astype(bool), "p_sat": r["p_sat"].cpu().numpy()}
    if r["rho_vl"] is not None:
        rho = r["rho_vl"].cpu().numpy()
        out["rho_v"], out["rho_l"] = rho[:, 0].copy(), rho[:, 1].copy()
    return out


class Ctx:
    pass


@pytest.fixture(scope="module")
def ctx(oracle, hip_lib):
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    c = Ctx()
    c.P, c.T, c.cls = batch()
    c.rho, c.start = start_reference(oracle, c.P, c.T)
    c.want, c.mask = {}, {}
    c.want["p_sat"], c.mask["p_sat"] = oracle.pure_vapor_pressure(c.P, c.T, prec=1)
    c.want["rho_v"], c.want["rho_l"], c.mask["vle"], _, _ = oracle.pure_vle(c.P, c.T, prec=1)
    c.want["rho"], c.mask["liq"] = oracle.pure_liquid_density(c.P, c.T, np.full(N, P_LIQ), prec=1)
    # the density bars live on the saturation grid's reduced temperatures: the row's own T / T_c, rounded up to the grid
    Tc = cr.oracle_scan(oracle, c.P)[0]
    theta = c.T / Tc
    assert (theta > 0.0).all() and (theta < max(sg.SUB)).all()
    grid_theta = np.asarray(sg.SUB)
    c.theta_up = grid_theta[np.searchsorted(grid_theta, theta)]
    c.cond = sg.reference(orc=oracle)["cond"]  # cached: shared with tests/test_saturation_line_gpu.py in one session
    c.Pd, c.Td = torch.from_numpy(c.P).cuda(), torch.from_numpy(c.T).cuda()
    return c


def check_against_oracle(c, variant, r, n):
    """Status and values of the first n rows of a run against the oracle; -> list of failures."""
    bad = []
    keys = {"liq": (("rho", "liq", "rho_psat"),)}.get(variant, (("p_sat", "p_sat", None), ("rho_v", "vle", "rho_v"), ("rho_l", "vle", "rho_l")))
    mask = c.mask["liq" if variant == "liq" else "p_sat"][:n]
    diff = r["status"] != mask
    print("%-8s n %3d: status differs from the oracle's mask on %d rows, oracle fails %d" % (variant, n, diff.sum(), mask.sum()))
    if diff.any():
        bad.append((variant, n, "mask", np.flatnonzero(diff)[:8].tolist()))
    for key, mkey, cond_key in keys:
        if key not in r:
            continue
        ok = ~r["status"] & ~c.mask[mkey][:n]
        err = np.abs(r[key] / c.want[key][:n] - 1.0)
        bar = np.full(n, P_BAR) if cond_key is None else np.array([sg.bar(c.cond[cond_key], th) for th in c.theta_up[:n]])
        worst = float(err[ok].max()) if ok.any() else 0.0
        over = ok & ~(err <= bar)
        print("%-8s n %3d: %-6s measured %.2e (bar %.2e .. %.2e) rows %d %s" % (variant, n, key, worst, bar.min(), bar.max(), ok.sum(), "EXCEEDED" if over.any() else ""))
        if over.any():
            k = int(np.flatnonzero(over)[0])
            bad.append((variant, n, key, int(over.sum()), k, float(err[k]), float(bar[k])))
    return bad


def test_batch_mixes_and_sorts_the_classes(ctx):
    c = ctx
    for w in range(4):  # waves 0-3: all four classes in every wave; waves 4-7: one class each
        assert len(set(c.cls[64 * w:64 * w + 64])) == 4
        assert len(set(c.cls[256 + 64 * w:256 + 64 * w + 64])) == 1


def test_start_evaluation_against_the_oracle(ctx, hip_lib):
    c = ctx
    assert hip_lib.pcs_abi_version() >= 107
    out = probe(hip_lib, c.Pd, c.Td)
    assert np.isfinite(out).all()
    ref = c.start
    scale = {"a": np.abs(ref["a"]), "p": c.rho * (1.0 + np.abs(ref["mu"])), "dp": np.abs(ref["dp"]), "mu": 1.0 + np.abs(ref["mu"])}
    bad = []
    for k, q in enumerate(QUANTITIES):
        e_gen = np.abs(out[:, k] - ref[q]) / scale[q]
        e_fix = np.abs(out[:, 4 + k] - ref[q]) / scale[q]
        for name, rows in (("mixed waves", slice(0, N // 2)), ("uniform waves", slice(N // 2, N))) + tuple(
                (CLASSES[j], c.cls == j) for j in range(4)):
            print("start %-3s %-13s E_gen %.3e E_fix %.3e" % (q, name, e_gen[rows].max(), e_fix[rows].max()))
        E_gen, E_fix = float(e_gen.max()), float(e_fix.max())
        print("start %-3s %-13s E_gen %.3e E_fix %.3e ratio %.2f (largest |fix - gen| %.3e)" % (
            q, "all", E_gen, E_fix, E_fix / E_gen, (np.abs(out[:, 4 + k] - out[:, k]) / scale[q]).max()))
        # Same-state check (not the bound under test): the generic form must sit at the oracle's state at all.  Its scale
        # is one that cannot vanish -- |a| passes through zero where repulsion and attraction cancel at eta = 0.5 (measured:
        # 3.2e-3 of |a| on a polar + associating row, identically in both forms), so a is taken against rho (1 + |a'|) here,
        # the size of its terms.  fp32 rounding (6e-8) times the cancellation of the terms (up to ~50 x the scale) and the
        # ~1e-6 of the fp32 ceta, amplified by dp/drho ~ 50, stay below 1e-4; 1e-3 separates that from another state.
        same = np.abs(out[:, k] - ref[q]) / (scale["p"] if q == "a" else scale[q])
        if not same.max() < 1e-3:
            bad.append((q, "generic form not at the oracle's state", float(same.max())))
        if not E_fix <= 2.0 * E_gen:
            bad.append((q, E_gen, E_fix))
    assert not bad, bad


def test_probe_tail_rows(ctx, hip_lib):
    """A grid that does not end on a workgroup: the rows past n are neither read nor written."""
    c = ctx
    whole = probe(hip_lib, c.Pd, c.Td)
    for n in PREFIXES:
        assert np.array_equal(probe(hip_lib, c.Pd[:n].contiguous(), c.Td[:n].contiguous()), whole[:n])


@pytest.mark.parametrize("variant", VARIANTS + ("liq",))
def test_solves_against_the_long_double_oracle(ctx, variant):
    c = ctx
    bad = check_against_oracle(c, variant, run_variant(variant, c.Pd, c.Td), N)
    for n in PREFIXES:
        bad += check_against_oracle(c, variant, run_variant(variant, c.Pd[:n].contiguous(), c.Td[:n].contiguous()), n)
    assert not bad, bad
