"""GPU: pcs_mix_density and PcSaftMix.liquid_density / vapor_density against the long-double referee of
tests/tools/mix_density_referee.py (root definitions restated there on a fixed packing-fraction grid, independent of the kernel).

Bars.  Values: |rho / rho_ref - 1| <= 1e-10 on every kept row, the project's bar for values against the long-double oracle
(tests/test_large_parity_gpu.py); dpdrho 1e-9.  Gradients: all 21 quantities (16 parameters, k_ij, eps_AiBj, T, p, x) of every
kept row, error relative to the row's largest exact component <= max(1e-10, 10 x the error of the referee's fp64 twin), and the
same per class and column (the rule of tests/test_mix_point_exact_gpu.py).  Input set: 2,880 liquid + 1,728 vapour rows.

Measured (MI355X): liquid max |rho/rho_ref - 1| 1.3e-15, dpdrho 8.3e-14; vapour 4.4e-16 / 2.2e-16; gradients 8.7e-14 / 1.6e-13 of
the row maximum on the rows with a bar of 1e-10; 3 - 7 evaluations per row (see README).
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import mix_density_referee as ref  # noqa: E402
import mix_point_exact as ex  # noqa: E402

pytestmark = pytest.mark.gpu

PHASES = (ref.LIQUID, ref.VAPOUR)
WORKGROUP = 64  # DBLOCK of csrc/mix_density.hip
SHAPES = (1, 63, 64, 65, WORKGROUP - 1, WORKGROUP, WORKGROUP + 1, 5 * WORKGROUP + 17)
COLUMNS = ex.COLUMNS + ("p", "x")
C_UNIT = 1.0 / (1e3 * (6.02214076e23 * (1e-10 * 1e-10 * 1e-10)))  # A^-3 -> kmol/m3
name = lambda phase: "vapour" if phase else "liquid"


class Ctx:
    pass


def _d(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _np(x):
    return x.detach().cpu().numpy()


def _bits(x):
    x = _np(x)
    return x.view(np.int64) if x.dtype == np.float64 else x


def kernel_gradient(native, P, K, T, p, x, rho, dpdrho):
    """[n,21] d rho [A^-3] / d(16 parameters, kij0, kij1, T, p, x) the way the autograd Function forms it: one
    native.mix_derivatives_vjp call with g_p = -1 / dpdrho (tensors on the GPU)"""
    w = -1.0 / dpdrho
    G = native.mix_derivatives_vjp(P, K, T, torch.stack((x * rho, (1.0 - x) * rho), dim=1), g_p=w)
    unit = ref.P_RED / T
    return torch.cat((G[:, :18], (G[:, 18] + w * p * unit / T)[:, None], (-w * unit)[:, None], (rho * (G[:, 19] - G[:, 20]))[:, None]), dim=1)


@pytest.fixture(scope="module")
def ctx(oracle, hip_lib):
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from feos_torch_amd import native

    out = {}
    for phase in PHASES:
        c = ref.inputs(oracle, phase)
        g = Ctx()
        g.c, g.phase = c, phase
        g.perm = ref.interleave(c.n, c.nblocks)  # classes, temperature and pressure factors mix within a wave
        g.dev = [_d(v[g.perm]) for v in (c.P, c.K, c.T, c.p, c.x)]
        g.r = native.mix_density(*g.dev, phase)
        back = np.empty(c.n, dtype=np.int64)
        back[g.perm] = np.arange(c.n)
        g.rho, g.dpdrho, g.status, g.iters = (_np(g.r[k])[back] for k in ("rho", "dpdrho", "status", "iters"))
        safe_rho = torch.where(g.r["status"], torch.full_like(g.r["rho"], 5e-3), g.r["rho"])
        safe_dp = torch.where(g.r["status"], torch.ones_like(g.r["rho"]), g.r["dpdrho"])
        g.grad = _np(kernel_gradient(native, *g.dev, safe_rho, safe_dp))[back]
        out[phase] = g
    return out


@pytest.mark.parametrize("phase", PHASES)
def test_values_against_the_referee(ctx, phase):
    g = ctx[phase]
    c, k = g.c, g.c.keep
    assert not g.status[k].any(), np.nonzero(k & g.status)[0]
    e_rho = np.abs(g.rho[k] / c.rho[k] - 1.0)
    e_dp = np.abs(g.dpdrho[k] / c.dpdrho[k] - 1.0)
    print("%s: %d kept rows of %d, max |rho/rho_ref - 1| = %.2e (bar 1e-10), max |dpdrho/ref - 1| = %.2e (bar 1e-9); evaluations "
          "per converged row: median %d, max %d; %d rows failed" % (name(phase), k.sum(), c.n, e_rho.max(), e_dp.max(),
                                                                      np.median(g.iters[~g.status]), g.iters.max(), g.status.sum()))
    assert e_rho.max() <= 1e-10
    assert e_dp.max() <= 1e-9
    assert (g.iters[~g.status] >= 1).all() and (g.iters[g.status] == -1).all()
    assert (g.rho[g.status] == 0.0).all() and (g.dpdrho[g.status] == 0.0).all()
    # where the referee decides that there is no root on the branch, the kernel returns none either
    gone = (c.status == ref.ENDS) | (c.status == ref.NONE)
    assert g.status[gone].all()


def test_failure_mask(ctx, oracle):
    """One invalid row per rule inside waves of valid rows: status 1, zero outputs, neighbours bit-identical to the run without them."""
    from feos_torch_amd import native

    g = ctx[ref.LIQUID]
    n = 256
    P, K, T, p, x = (v[:n].clone() for v in g.dev)
    bad = {5: (0, np.nan), 37: (0, np.inf), 70: (0, 0.0), 71: (0, -300.0), 100: (1, np.nan), 129: (1, np.inf), 130: (1, 0.0),
           163: (1, -1e5), 190: (2, np.nan), 200: (2, -1e-3), 201: (2, 1.0 + 1e-9), 255: (2, np.inf)}
    for row, (which, value) in bad.items():
        (T, p, x)[which][row] = value
    r = native.mix_density(P, K, T, p, x, ref.LIQUID)
    rows = np.array(sorted(bad))
    others = np.setdiff1d(np.arange(n), rows)
    assert _np(r["status"])[rows].all()
    assert (_np(r["rho"])[rows] == 0.0).all() and (_np(r["dpdrho"])[rows] == 0.0).all() and (_np(r["iters"])[rows] == -1).all()
    for key in ("rho", "dpdrho", "status", "iters"):
        assert np.array_equal(_bits(r[key])[others], _bits(g.r[key])[:n][others]), key
    # x = 0 and x = 1 are valid: the pure-limit blocks of the liquid set converge
    c = g.c
    ends = c.keep & ((c.x == 0.0) | (c.x == 1.0))
    assert ends.sum() >= 1000 and not g.status[ends].any()


def test_pressure_above_the_vapour_branch_fails(ctx, oracle):
    """Vapour at 50 x the dew pressure, rows at 1.2 T_batch: where the referee reports that the branch ends below p_spec the
    kernel fails too -- it never returns the liquid root -- each such row inside a wave of valid rows."""
    from feos_torch_amd import native

    g = ctx[ref.VAPOUR]
    c = g.c
    rows = np.nonzero(c.keep & (c.block == 0) & (c.factor == 2))[0]
    p50 = 50.0 * c.p[rows]
    _, _, st = ref.solve(oracle, c.P[rows], c.K[rows], c.T[rows], p50, c.x[rows], ref.VAPOUR)
    gone = st == ref.ENDS
    print("vapour at 50 x p_dew, 1.2 T_batch: the referee reports 'branch ends' for %d of %d rows" % (gone.sum(), len(rows)))
    assert gone.sum() >= 10
    # a wave-mixed batch: the valid rows at their own pressure, every third one at 50 x
    pick = np.arange(len(rows)) % 3 == 0
    p = np.where(pick, p50, c.p[rows])
    r = native.mix_density(_d(c.P[rows]), _d(c.K[rows]), _d(c.T[rows]), _d(p), _d(c.x[rows]), ref.VAPOUR)
    status, rho = _np(r["status"]), _np(r["rho"])
    assert status[pick & gone].all() and (rho[pick & gone] == 0.0).all()
    assert not status[~pick].any()
    assert np.array_equal(rho[~pick].view(np.int64), g.rho[rows][~pick].view(np.int64))
    # and the rows with a root at 50 x agree with the referee's
    keep = pick & (st == ref.OK)
    if keep.any():
        want, slope, _ = ref.solve(oracle, c.P[rows][keep], c.K[rows][keep], c.T[rows][keep], p50[keep], c.x[rows][keep], ref.VAPOUR)
        tight = slope >= ref.MIN_SLOPE
        assert not status[keep][tight].any()
        assert np.abs(rho[keep][tight] / want[tight] - 1.0).max(initial=0.0) <= 1e-10


@pytest.mark.parametrize("phase", PHASES)
def test_shapes(ctx, phase):
    """Prefixes of the big batch -- below, at and past one wave / workgroup, several workgroups with a ragged tail -- carry the
    bits of the same rows inside it; an empty batch returns empty outputs."""
    from feos_torch_amd import native

    g = ctx[phase]
    for n in sorted(set(SHAPES)):
        r = native.mix_density(*(v[:n] for v in g.dev), phase)
        for key in ("rho", "dpdrho", "status", "iters"):
            assert r[key].shape == (n,)
            assert np.array_equal(_bits(r[key]), _bits(g.r[key])[:n]), (n, key)
    r = native.mix_density(*(v[:0] for v in g.dev), phase)
    assert all(r[key].shape == (0,) for key in ("rho", "dpdrho", "status", "iters"))


def test_identical_components_give_the_pure_density(ctx):
    """Both components the same pure_batch row (all four polar / associating combinations), k_ij = 0, random x:
    liquid_density is PcSaftPure.liquid_density at the same (T, p) to 1e-10."""
    from feos_torch_amd import PcSaftMix, PcSaftPure
    from feos_torch_amd.synthetic import pure_batch, pure_pressures

    n = 64
    par, T = pure_batch(4000, 77)
    polar, assoc = par[:, 3] != 0, par[:, 6] != 0
    pick = np.concatenate([np.nonzero((polar == a) & (assoc == b))[0][:16] for a in (False, True) for b in (False, True)])
    assert len(pick) == n
    par, T, p = par[pick], T[pick], pure_pressures(n, 78)
    x = np.random.default_rng(79).uniform(0.0, 1.0, n)
    nans_pure, rho_pure = PcSaftPure(_d(par)).liquid_density(_d(T), _d(p))
    mix = PcSaftMix(_d(np.stack((par, par), axis=1)), _d(np.zeros((n, 2))))
    rho_mix, nans_mix = mix.liquid_density(_d(T), _d(p), _d(x))
    nans_pure, nans_mix = _np(nans_pure), _np(nans_mix)
    both = ~nans_pure & ~nans_mix
    a = _np(rho_pure)[both[~nans_pure]]
    b = _np(rho_mix)[both[~nans_mix]]
    err = np.abs(b / a - 1.0)
    print("identical components: %d of %d rows converge in both (pure fails %d, mixture %d), max |rho_mix / rho_pure - 1| = %.2e" % (
        both.sum(), n, nans_pure.sum(), nans_mix.sum(), err.max()))
    assert both.sum() >= 48 and not (nans_mix & ~nans_pure).any()  # the mixture converges wherever the pure kernel does
    assert err.max() <= 1e-10


@pytest.mark.parametrize("phase", PHASES)
def test_gradients_row_by_row(ctx, phase):
    g = ctx[phase]
    c, k = g.c, g.c.keep
    assert np.isfinite(g.grad[k]).all()
    err, noise = ex.row_error(g.grad, c.grad), ex.row_error(c.grad64, c.grad)
    bar = np.maximum(1e-10, 10.0 * noise)
    tight = k & (noise <= 1e-11)
    print("%s gradients, row by row: %d kept rows, max error %.2e of the row maximum on the %d rows with a bar of 1e-10, largest "
          "err / bar %.3f (twin: max %.2e)" % (name(phase), k.sum(), err[tight].max(), tight.sum(), np.max(err[k] / bar[k]), noise[k].max()))
    assert (err[k] <= bar[k]).all(), np.nonzero(k & ~(err <= bar))[0]


@pytest.mark.parametrize("phase", PHASES)
def test_gradients_per_class_and_column(ctx, phase):
    """Each of the 21 columns in its own measure over the kept rows of a class, zero-valued parameters included; columns the
    exact gradient leaves identically zero over a class are exactly 0.0."""
    g = ctx[phase]
    c = g.c
    fails, worst, n_zero = [], (0.0, 0.0, None), 0
    for cls in range(6):
        rows = c.keep & (c.cls == cls)
        err, noise = ex.column_error(g.grad, c.grad, rows), ex.column_error(c.grad64, c.grad, rows)
        bar = np.maximum(1e-10, 10.0 * noise)
        j = int(np.argmax(err / bar))
        if err[j] / bar[j] > worst[1]:
            worst = (float(err[j]), float(err[j] / bar[j]), (cls, COLUMNS[j]))
        fails += [(cls, COLUMNS[j], float(err[j]), float(bar[j])) for j in np.nonzero(~(err <= bar))[0]]
        for j in np.nonzero((c.grad[rows] == 0.0).all(axis=0))[0]:
            n_zero += 1
            if not (g.grad[rows, j] == 0.0).all():
                fails.append((cls, COLUMNS[j], "must be exactly zero", float(np.abs(g.grad[rows, j]).max())))
    zero_par = c.keep[:, None] & (c.P.reshape(c.n, 16) == 0.0) & (c.grad[:, :16] != 0.0)
    print("%s gradients, per class and column: largest err / bar %.3f (err %.2e, class and column %s); %d (class, column) pairs "
          "exactly zero; %d entries with a zero parameter and a non-zero derivative" % (name(phase), worst[1], worst[0], worst[2], n_zero, zero_par.sum()))
    assert zero_par.sum() >= 400
    assert not fails, fails


@pytest.mark.parametrize("phase", PHASES)
def test_autograd(ctx, phase):
    """liquid_density / vapor_density with requires_grad on all five inputs, on a batch in which rows fail: the gradients of the
    kept rows are the kernel-level ones, those of dropped rows are zero, the model is reduced; one input alone works."""
    from feos_torch_amd import PcSaftMix

    g = ctx[phase]
    n = 320
    P, K, T, p, x = (v[:n].clone() for v in g.dev)
    T[7], p[64], x[130] = np.nan, -1.0, 2.0
    if phase == ref.VAPOUR:
        p[200] = p[200] * 1e4  # far above the vapour branch
    leaves = [v.clone().requires_grad_(True) for v in (P, K, T, p, x)]
    mix = PcSaftMix(leaves[0], leaves[1])
    call = lambda m, *a: (m.vapor_density if phase else m.liquid_density)(*a)
    rho, nans = call(mix, *leaves[2:])
    nans_np = _np(nans)
    assert nans_np[[7, 64, 130]].all() and (phase == ref.LIQUID or nans_np[200])
    expected = _np(g.r["status"])[:n].copy()
    expected[[7, 64, 130] + ([200] if phase else [])] = True
    assert np.array_equal(nans_np, expected)
    ok = ~nans_np
    assert rho.shape == (ok.sum(),) and mix._par.shape[0] == ok.sum() and mix.kij.shape[0] == ok.sum()
    assert not nans.requires_grad
    assert np.array_equal(_bits(rho), _bits(g.r["rho"][:n] * C_UNIT)[ok])
    w = torch.linspace(0.5, 1.5, int(ok.sum()), dtype=torch.float64, device=rho.device)
    (rho * w).sum().backward()
    got = np.concatenate([_np(v.grad).reshape(n, -1) for v in leaves], axis=1)
    assert (got[~ok] == 0.0).all()
    back = np.empty(g.c.n, dtype=np.int64)
    back[g.perm] = np.arange(g.c.n)
    want = g.grad[g.perm][:n][ok] * (C_UNIT * _np(w))[:, None]
    scale = np.abs(want).max(axis=1)
    err = (np.abs(got[ok] - want).max(axis=1) / scale).max()
    print("%s autograd: %d of %d rows kept, largest difference to the kernel-level gradient %.2e of the row maximum" % (
        name(phase), ok.sum(), n, err))
    assert err <= 1e-12  # the same kernel results, combined in another order: a few roundings
    # one input alone
    for j in range(5):
        one = [v.clone().requires_grad_(k == j) for k, v in enumerate((P, K, T, p, x))]
        m1 = PcSaftMix(one[0], one[1])
        r1, _ = call(m1, *one[2:])
        (r1 * w).sum().backward()
        assert np.array_equal(_bits(one[j].grad), _bits(leaves[j].grad)), j
        assert all(v.grad is None for k, v in enumerate(one) if k != j)
    # no graph when nothing requires a gradient
    r0, _ = call(PcSaftMix(P, K), T, p, x)
    assert not r0.requires_grad and np.array_equal(_bits(r0), _bits(rho))


def test_three_components_raise():
    from feos_torch_amd import PcSaftMix

    par = torch.zeros((4, 3, 8), dtype=torch.float64)
    par[:, :, 0], par[:, :, 1], par[:, :, 2] = 1.5, 3.5, 250.0
    t = torch.full((4,), 300.0, dtype=torch.float64)
    for method in ("liquid_density", "vapor_density"):
        with pytest.raises(Exception, match="binary"):
            getattr(PcSaftMix(par), method)(t, t * 1e3, t * 0 + 0.5)


def test_round_trip_with_bubble_point(ctx):
    """liquid_density(T, p_bubble, x) at the pressure bubble_point returns: the pressure of `derivatives` at that density is
    p_bubble to 1e-10, and the density is that call's own liquid.  The measure of the pressure is the sum it is computed
    from, p = rho - a + sum rho_i mu_i: |p(rho x) - p_bubble| <= 1e-10 max(p_bubble, rho) in reduced units.  Relative to
    p_bubble itself no fp64 evaluation can be held to 1e-10: a liquid's p is the difference of terms of the size of rho and
    larger, p_bubble / rho goes down to 1e-40 on these rows, and `derivatives` at ANY density carries ~1e-16 rho of rounding
    (measured: 5.8e-5 relative to p_bubble on the worst row while the density agrees with the bubble point's own liquid to
    4e-14); that figure is printed, not asserted."""
    from feos_torch_amd import PcSaftMix, native
    from feos_torch_amd.synthetic import mix_batch

    P, K, T, x, p0 = (_d(v) for v in mix_batch(192, 2024))
    mix = PcSaftMix(P, K)
    p_b, nans = mix.bubble_point(T, x, p0)
    T_ok, x_ok = T[~nans], x[~nans]
    bubble = native.mix_bubble_dew(mix._par, mix.kij, T_ok, x_ok, p0[~nans], False)
    rho, nans2 = mix.liquid_density(T_ok, p_b, x_ok)
    assert not nans2.any() and rho.shape == p_b.shape
    rho_a = rho / C_UNIT
    p_red = mix.derivatives(T_ok, torch.stack((x_ok * rho_a, (1.0 - x_ok) * rho_a), dim=1))[1]
    want = p_b * ref.P_RED / T_ok
    e_p = _np(((p_red - want).abs() / torch.maximum(want, rho_a))).max()
    e_rel = _np((p_red / want - 1.0).abs()).max()
    e_rho = _np((rho_a / bubble["rho4"][:, 2:4].sum(dim=1) - 1.0).abs()).max()
    print("round trip: %d rows, max |p(rho x) - p_bubble| / max(p_bubble, rho) = %.2e (bar 1e-10), relative to p_bubble %.2e, "
          "max |rho / rho_liquid(bubble) - 1| = %.2e" % (len(T_ok), e_p, e_rel, e_rho))
    assert e_p <= 1e-10
    assert e_rho <= 1e-10
