"""GPU: pcs_mix_henry and PcSaftMix.henrys_law_constant against the long-double referee of tests/tools/henry_referee.py.

Rows: the first n of synthetic.mix_batch(720) for n = 1, 63, 64, 65, 257, 720 (64-lane workgroups: a single lane, a ragged
wave, more than one workgroup), both choices of the solute; the referee and its fp64 twin are computed once on the 720 rows.

Bars.  Value: |ln H - ln H_ref| <= max(1e-10, 10 x |twin - referee|) per row on every row the referee solves (all 720).
Gradient: d ln H / d(16 parameters, k_ij, eps_AiBj, T) from torch.autograd.grad of H.sum(), every column, error relative to the
row's largest referee component <= max(1e-10, 10 x the twin's).  rho_vl / p_sat: 2e-10 against pcs_pure_vle_fp64 and
PcSaftPure.vapor_pressure on the solvent rows -- each of those kernels is held to 1e-10 against the long-double oracle
(tests/test_large_parity_gpu.py), so two of them differ by at most twice that.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import henry_referee as hr  # noqa: E402
from dilute_grid import henry_error  # noqa: E402

pytestmark = pytest.mark.gpu

N = 720
SHAPES = (1, 63, 64, 65, 257, N)
SOLUTES = (0, 1)
f64 = torch.float64


def _d(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _np(x):
    return x.detach().cpu().numpy()


def _bits(x):
    x = _np(x)
    return x.view(np.int64) if x.dtype == np.float64 else x


class Ctx:
    pass


@pytest.fixture(scope="module")
def ctx(oracle, hip_lib):
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from feos_torch_amd import native
    from feos_torch_amd.synthetic import mix_batch

    c = Ctx()
    c.P, c.K, c.T = mix_batch(N)[:3]
    c.dev = [_d(v) for v in (c.P, c.K, c.T)]
    c.ref = {s: hr.reference(oracle, c.P, c.K, c.T, s) for s in SOLUTES}
    c.full = {s: native.mix_henry(*c.dev, s) for s in SOLUTES}
    return c


@pytest.mark.parametrize("solute", SOLUTES)
@pytest.mark.parametrize("n", SHAPES)
def test_values_against_the_referee(ctx, n, solute):
    from feos_torch_amd import native

    ref = ctx.ref[solute]
    assert not ref["failed"].any()  # the referee keeps every row (tests/test_henry_referee.py)
    r = native.mix_henry(*(v[:n].contiguous() for v in ctx.dev), solute)
    assert not _np(r["status"]).any(), np.nonzero(_np(r["status"]))[0]
    err = np.abs(np.log(_np(r["h"])) - ref["lnh"][:n])
    bar = np.maximum(1e-10, 10.0 * ref["d_lnh"][:n])
    tight = bar == 1e-10
    print("n = %d, solute %d: max |ln H - ln H_ref| = %.2e on the %d rows with a bar of 1e-10, max err / bar = %.2e on all rows"
          % (n, solute, err[tight].max() if tight.any() else 0.0, tight.sum(), (err / bar).max()))
    assert (err <= bar).all(), np.nonzero(err > bar)[0]
    # a row's result does not depend on the rows it shares a wave or a launch with
    for key in ("h", "rho_vl", "p_sat", "dlnh_drho", "status"):
        assert np.array_equal(_bits(r[key]), _bits(ctx.full[solute][key])[:n]), key


@pytest.mark.parametrize("solute", SOLUTES)
def test_solvent_state_agrees_with_the_pure_kernels(ctx, solute):
    from feos_torch_amd import PcSaftPure, native

    r = ctx.full[solute]
    Pv = ctx.dev[0][:, 1 - solute, :].contiguous()
    vle = native.pure_vle(Pv, ctx.dev[2], all_fp64=True)
    assert not _np(vle["status"]).any()
    e_rho = np.abs(_np(r["rho_vl"]) / _np(vle["rho_vl"]) - 1.0).max(axis=0)
    nans, p_sat = PcSaftPure(Pv).vapor_pressure(ctx.dev[2])
    assert not _np(nans).any()
    e_p = np.abs(_np(r["p_sat"]) / _np(p_sat) - 1.0).max()
    e_p64 = np.abs(_np(r["p_sat"]) / _np(vle["p_sat"]) - 1.0).max()
    ref = ctx.ref[solute]
    e_ref = max(np.abs(_np(r["rho_vl"])[:, 0] / ref["rho_v"] - 1.0).max(), np.abs(_np(r["rho_vl"])[:, 1] / ref["rho_l"] - 1.0).max())
    print("solute %d: rho_V %.2e, rho_L %.2e against pcs_pure_vle_fp64; p_sat %.2e against PcSaftPure.vapor_pressure, %.2e against "
          "pcs_pure_vle_fp64; densities against the long-double referee %.2e (bars 2e-10)" % (solute, e_rho[0], e_rho[1], e_p, e_p64, e_ref))
    assert e_rho.max() <= 2e-10 and e_p <= 2e-10 and e_p64 <= 2e-10
    # dlnh_drho is the weight of the backward pass and is held through the gradient test, in which it multiplies every solvent
    # column; its own relative error is printed only: the mixed second derivative comes out of the (zeta_3, rho_2) coordinates
    # of the T2 evaluation as c0 (c1 a_uu + a_uw), a difference the referee's nested duals do not form
    e_w = np.abs(_np(r["dlnh_drho"]) / ref["dlnh_drho"] - 1.0)
    print("solute %d: dlnh_drho max relative error %.2e (row %d)" % (solute, e_w.max(), int(e_w.argmax())))


@pytest.mark.parametrize("solute", SOLUTES)
@pytest.mark.parametrize("n", (65, N))
def test_gradient_against_the_referee(ctx, n, solute):
    from feos_torch_amd import PcSaftMix

    ref = ctx.ref[solute]
    P, K, T = (v[:n].clone().requires_grad_(True) for v in ctx.dev)
    H, nans = PcSaftMix(P, K).henrys_law_constant(T, solute=solute)
    assert not _np(nans).any() and H.shape == (n,)
    gP, gK, gT = torch.autograd.grad(H.sum(), (P, K, T))
    g = torch.cat((gP.reshape(n, 16), gK, gT[:, None]), dim=1) / H.detach()[:, None]  # d ln H per row
    assert np.array_equal(_bits(H), _bits(ctx.full[solute]["h"])[:n])
    exact = ref["grad"][:n]
    err = np.abs(_np(g) - exact).max(axis=1) / np.abs(exact).max(axis=1)
    bar = np.maximum(1e-10, 10.0 * ref["d_grad"][:n])
    tight = bar == 1e-10
    col = np.abs(_np(g) - exact) / np.abs(exact).max(axis=1)[:, None]
    print("n = %d, solute %d: gradient error %.2e of the row's largest component on the %d rows with a bar of 1e-10, max err / bar "
          "%.2e on all rows; worst column %d" % (n, solute, err[tight].max(), tight.sum(), (err / bar).max(), int(col.max(axis=0).argmax())))
    assert np.isfinite(_np(g)).all()
    assert (err <= bar).all(), (np.nonzero(err > bar)[0], err[err > bar], bar[err > bar])


def test_failure_mask_and_model_reduction(ctx):
    """T above the solvent's critical temperature, T = NaN, a solute with sigma = 0 and a valid neighbour in one wave."""
    from feos_torch_amd import PcSaftMix, PcSaftPure

    solute, row = 1, 0
    P = ctx.dev[0][row:row + 1].repeat(4, 1, 1)
    K = ctx.dev[1][row:row + 1].repeat(4, 1)
    T = ctx.dev[2][row:row + 1].repeat(4)
    nans_c, t_c, _, _ = PcSaftPure(P[:1, 0, :].contiguous()).critical_point()
    assert not _np(nans_c).any()
    T[0] = 1.05 * t_c[0]
    T[1] = float("nan")
    P[2, 1, 1] = 0.0
    eos = PcSaftMix(P, K)
    H, nans = eos.henrys_law_constant(T, solute=solute)
    assert _np(nans).tolist() == [True, True, True, False]
    assert H.shape == (1,) and np.array_equal(_bits(H), _bits(ctx.full[solute]["h"])[row:row + 1])
    # the model is reduced to the surviving row, and so are later calls
    assert eos._par.shape == (1, 2, 8) and eos.kij.shape == (1, 2)
    assert torch.equal(eos._par, P[3:4]) and torch.equal(eos.kij, K[3:4])
    H2, nans2 = eos.henrys_law_constant(T[3:4], solute=solute)
    assert _np(nans2).tolist() == [False] and np.array_equal(_bits(H2), _bits(H))
    from feos_torch_amd import native

    r = native.mix_henry(P, K, T, solute)
    for key in ("h", "rho_vl", "p_sat", "dlnh_drho"):
        assert (_np(r[key])[:3] == 0.0).all(), key
    # invalid kij, and an invalid SOLVENT parameter
    K2, P2 = K.clone(), P.clone()
    K2[3, 0] = float("inf")
    assert _np(native.mix_henry(P, K2, T, solute)["status"]).all()
    P2[3, 0, 2] = -1.0
    assert _np(native.mix_henry(P2, K, T, solute)["status"]).all()


def test_supercritical_solute_is_an_ordinary_row(ctx, oracle):
    """Rows without dipoles and association (T_c scales with epsilon_k): the solute's epsilon_k is scaled so that T = 3 T_c of
    the solute; the rows are solved and meet the value bar."""
    from feos_torch_amd import PcSaftPure, native

    solute = 1
    rows = np.arange(0, 384, 6)  # class 0 of synthetic.mix_batch: 64 rows
    P, K, T = ctx.P[rows].copy(), ctx.K[rows].copy(), ctx.T[rows].copy()
    assert (P[:, :, 3:] == 0.0).all()
    nans, t_c, _, _ = PcSaftPure(_d(P[:, solute, :])).critical_point()
    assert not _np(nans).any()
    P[:, solute, 2] *= T / (3.0 * _np(t_c))
    nans, t_c, _, _ = PcSaftPure(_d(P[:, solute, :])).critical_point()
    ratio = T / _np(t_c)
    assert not _np(nans).any() and np.abs(ratio - 3.0).max() < 1e-6
    r = native.mix_henry(_d(P), _d(K), _d(T), solute)
    assert not _np(r["status"]).any()
    ref = hr.reference(oracle, P, K, T, solute)
    assert not ref["failed"].any()
    err = np.abs(np.log(_np(r["h"])) - ref["lnh"])
    bar = np.maximum(1e-10, 10.0 * ref["d_lnh"])
    print("solute at 3 T_c: %d rows solved, max |ln H - ln H_ref| = %.2e, max err / bar %.2e" % (len(rows), err.max(), (err / bar).max()))
    assert (err <= bar).all()


def test_dilute_bubble_points_approach_the_henry_constant(ctx, oracle):
    """y_s p phi_s^V / x_s of the EXISTING solver at x_s = 2^-30 (bubble_point with the incipient composition, phi from
    `derivatives` at the density of `vapor_density`) against H, on the rows that dilute_grid.henry_error judges linear (the
    oracle's bubble pressures at 2^-30 and 2^-20 within 1e-4 of p_sat).  Bar: 10 x what the oracle's own mix_bubble_dew gives for
    the same expression against the referee's H, floor 1e-8.  Measured on an MI355X: see DESIGN.md section 4n."""
    from feos_torch_amd import PcSaftMix

    n, d_lo, d_hi = 360, 2.0**-30, 2.0**-20
    for solute in SOLUTES:
        # the solute is made component 1 (index 0) of the solved model: bubble_point hands out the incipient mole fraction of
        # that component, and 1 - y of a trace component has no digits left.  H itself is taken in the rows' own labelling
        order = [solute, 1 - solute]
        P, K, T = np.ascontiguousarray(ctx.P[:n][:, order, :]), ctx.K[:n], ctx.T[:n]
        ref = ctx.ref[solute]
        p_sat, pst = oracle.pure_vapor_pressure(np.ascontiguousarray(P[:, 1, :]), T, prec=1)
        p_lo, rho4, st_lo = oracle.mix_bubble_dew(P, K, T, np.full(n, d_lo), p_sat, False, prec=1)
        p_hi, _, st_hi = oracle.mix_bubble_dew(P, K, T, np.full(n, d_hi), p_sat, False, prec=1)
        _, judged = henry_error(p_lo, p_lo, p_hi, d_lo, d_lo, d_hi, p_sat)
        sel = judged & ~pst & ~st_lo & ~st_hi
        assert sel.sum() >= 0.3 * n, sel.sum()
        # the oracle's value of the expression: y_s p phi_s = rho_s^V k_B T exp(mu_s^V)
        mu_v = oracle.mix_derivatives_exact(P, K, T, rho4[:, 0:2])[2][:, 0]
        with np.errstate(invalid="ignore", divide="ignore"):
            e_orc = np.abs(np.log(rho4[:, 0] * T * hr.KT_A3 / d_lo) + mu_v - ref["lnh"][:n])
        # the class on the GPU
        idx = np.nonzero(sel)[0]
        Pd, Kd, Td = _d(P[idx]), _d(K[idx]), _d(T[idx])
        eos = PcSaftMix(Pd, Kd)
        p, nans, y = eos.bubble_point(Td, _d(np.full(len(idx), d_lo)), _d(p_sat[idx]), incipient_molefracs=True)
        assert not _np(nans).any()
        rho, nans = eos.vapor_density(Td, p, y)
        assert not _np(nans).any()
        rho = rho * hr.RHO_UNIT
        _, p_red, mu, _ = eos.derivatives(Td, torch.stack((y * rho, (1.0 - y) * rho), dim=1))
        ln_est = torch.log(y * p / d_lo) + mu[:, 0] - torch.log(p_red / rho)
        H = ctx.full[solute]["h"][:n][torch.from_numpy(idx).cuda()]
        Hs, nans = eos.henrys_law_constant(Td, solute=0)
        assert not _np(nans).any()
        e_label = np.abs(_np(torch.log(Hs)) - _np(torch.log(H))).max()
        e_gpu = np.abs(_np(ln_est) - _np(torch.log(H)))
        bar = np.maximum(1e-8, 10.0 * e_orc[idx])
        print("solute %d: %d of %d rows judged linear; |ln(y p phi / x) - ln H| at x = 2^-30: class max %.2e (median %.1e), oracle "
              "max %.2e (median %.1e); max err / bar %.2e; H with the components relabelled: %.2e"
              % (solute, len(idx), n, e_gpu.max(), np.median(e_gpu), e_orc[idx].max(), np.median(e_orc[idx]), (e_gpu / bar).max(), e_label))
        assert e_label <= 1e-10
        assert (e_gpu <= bar).all(), (idx[e_gpu > bar], e_gpu[e_gpu > bar], bar[e_gpu > bar])


def test_a_following_bubble_point_is_unchanged(ctx):
    from feos_torch_amd import PcSaftMix
    from feos_torch_amd.synthetic import mix_batch

    n = 257
    _, _, _, x, p0 = mix_batch(N)
    P, K, T = (v[:n].contiguous() for v in ctx.dev)
    xs, ps = _d(x[:n]), _d(p0[:n])
    fresh = PcSaftMix(P.clone(), K.clone()).bubble_point(T, xs, ps)
    eos = PcSaftMix(P.clone(), K.clone())
    _, nans = eos.henrys_law_constant(T, solute=1)
    assert not _np(nans).any()
    after = eos.bubble_point(T, xs, ps)
    for a, b in zip(fresh, after):
        assert np.array_equal(_bits(a), _bits(b))
