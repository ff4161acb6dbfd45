"""GPU: the gradient blocks of the binary bubble / dew kernels against the exact implicit-function referee, all 19 columns.

  pcs_mix_jacobian (csrc/mix_jacobian.hpp)          jac [n,19]   = dp/d(16 parameters, k_ij, eps_AiBj, T)
  pcs_mix_point_jacobian (csrc/mix_incipient.hpp)   jac_p [n,19] the same block, jac_y [n,19] = dy/d(...), y = mole fraction of
                                                    component 1 in the incipient phase; requested together and jac_y alone

Referee (tests/tools/mix_point_exact.py, checked on the CPU by tests/test_mix_point_exact_referee.py): the implicit-function
theorem over oracle.mix_derivatives_vjp_exact in long double.  The kernels are fed the oracle's rho4 -- the doubles the referee
used -- so the comparison is arithmetic alone; rows the input set does not keep ride along as wave mates with placeholder
densities and are not compared.  Input set: mix_temperature_referee.inputs, 192 parameter rows x 3 temperature factors, 566
(bubble) / 576 (dew) kept rows.

Bars, from the referee and its fp64 twin alone.  Per row: max(1e-10, 10 e_row), e_row = twin against referee relative to the
row's largest exact component; 1e-10 on all but 7 / 3 (bubble p / y) and 9 / 12 (dew) rows, all of class 2.  Per class and
column on the tight rows: max_i |got - want| / max_i |want| <= max(1e-10, 10 x the twin's same measure); a column that is
identically zero in the exact block of a class must be exactly 0.0 in the kernel's.  No `checked` mask: the 3063 (bubble) /
3150 (dew) entries per block whose parameter is zero -- which the Richardson referee of tests/test_mix_incipient_gpu.py cannot
displace -- are compared like every other; 468 / 480 of them are non-zero in the exact y block and in 40 / 28 rows one of them
is the row's largest component (kappa_ab, eps_ab, na, nb of a site-less component next to an associating one).

Measured on an MI355X, error relative to the row's largest exact component, largest over the tight rows (bubble / dew):
pcs_mix_jacobian and the p block of pcs_mix_point_jacobian 2.9e-14 / 8.7e-14 (the two kernels agree to the printed digits),
y block 1.8e-14 / 4.2e-13, alone or together with p; medians 7e-16 ... 9e-16; on the rows with a wider bar at most 0.004 of it.
Per class and column: p 3.2e-14 / 2.6e-14, y 4.8e-14 / 2.1e-13 (at most 0.002 of the bar); 23 (class, column) pairs are
identically zero in the exact block and exactly 0.0 in the kernel's.  Zero-parameter entries, 468 / 480 per block: y 3.4e-15 /
3.5e-13 of the row maximum, the row's largest component in 40 / 28 rows (p block: 62 / 32 rows).  Through the model classes,
64 rows: at most 0.002 of the tolerance; the referee moves by 2.0e-14 / 5.2e-13 between the oracle's densities and the kernel's.

Sensitivity, tried on scratch builds and not kept (what this module printed; the suite as it was before this module stayed
green wherever it compares with a reference):
  a. jac_y[na_2] = 0 where na_2 = 0 (mix_point_jacobian's store): row test 1.0 of the row maximum (1e10 bars), column
     na_2 of class 2 0.84 / 1.0, zero-parameter line 1.0: red.  Every earlier test of the kernel green (tests/test_mix_incipient_gpu.py,
     test_mix_incipient_abi.py, test_point_shell_gpu.py: the Richardson referee skips the direction, the pinned rows have none).
  b. the eps_ab_1 column of both blocks x (1 + 1e-6): column eps_ab_1 1.0e-6 in classes 2, 4, 5 (1e4 bars), rows up to 3.4e-10 (p) /
     4.6e-10 (y): red.  tests/test_mix_incipient_gpu.py green (bars 1e-8 and 2.5e-7 / 9.5e-8 of the row maximum); only the bit
     pins of tests/test_point_shell_gpu.py notice that the bits moved.
  c. wy[1] x (1 + 1e-9) after solve3_pair: y block 1.1e-8 / 7.1e-8 on the tight rows (111 / 707 bars), column sigma_1 3.8e-8 /
     6.8e-8, p block unchanged: red.  tests/test_mix_incipient_gpu.py green; only the bit pins of tests/test_point_shell_gpu.py
     notice.
In all three test_geometry stays green, as it must: it compares the kernel with itself.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import mix_point_exact as ex  # noqa: E402
import mix_temperature_referee as tref  # noqa: E402

pytestmark = pytest.mark.gpu

PROBLEMS = (False, True)
PREFIXES = (1, 63, 64, 65, 129, 577)
N_GEOMETRY = 640  # the set and its first 64 rows again: ten full waves, so that a 577-row prefix exists
N_MODEL = 64
PLACEHOLDER = np.array([1e-6, 1e-6, 5e-3, 5e-3])  # densities of the rows that are not compared (mix_temperature_referee)
f64 = torch.float64
name = lambda dew: "dew" if dew else "bubble"


class Ctx:
    pass


def _d(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _np(x):
    return x.detach().cpu().numpy()


def _same_bits(a, b):
    a, b = a.contiguous(), b.contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.int64), b.view(torch.int64))


@pytest.fixture(scope="module")
def ctx(oracle, hip_lib):
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from feos_torch_amd import native

    out = {}
    for dew in PROBLEMS:
        c = ex.inputs(oracle, dew)
        g = Ctx()
        g.c, g.dew = c, dew
        g.rho4 = np.where(c.keep[:, None], c.rho4, PLACEHOLDER)
        g.dev = [_d(v) for v in (c.P, c.K, c.T, g.rho4)]
        g.jac = _np(native.mix_jacobian(*g.dev, dew))
        jp, jy = native.mix_point_jacobian(*g.dev, dew)
        g.jp, g.jy = _np(jp), _np(jy)
        g.jy_alone = _np(native.mix_point_jacobian(*g.dev, dew, want_p=False)[1])
        # (label, kernel block, exact block, twin block, row bar, tight rows)
        g.blocks = (("pcs_mix_jacobian p", g.jac, c.Jp, c.Jp64, c.bar_p, c.tight_p),
                    ("pcs_mix_point_jacobian p", g.jp, c.Jp, c.Jp64, c.bar_p, c.tight_p),
                    ("pcs_mix_point_jacobian y", g.jy, c.Jy, c.Jy64, c.bar_y, c.tight_y),
                    ("pcs_mix_point_jacobian y alone", g.jy_alone, c.Jy, c.Jy64, c.bar_y, c.tight_y))
        out[dew] = g
    return out


@pytest.mark.parametrize("dew", PROBLEMS)
def test_blocks_against_the_exact_referee_row_by_row(ctx, dew):
    """Every kept row, all 19 columns, error relative to the row's largest exact component <= bar_row."""
    g = ctx[dew]
    c = g.c
    k = c.keep
    fails = []
    for label, got, want, _, bar, tight in g.blocks:
        assert got.shape == (c.n, ex.N_DIRS) and np.isfinite(got[k]).all(), label
        err = ex.row_error(got, want)
        print("%-6s %-31s vs exact: max %.2e on the %d tight rows (bar 1e-10), median %.2e; largest err / bar %.3f on all %d rows" % (
            name(dew), label, err[tight].max(), tight.sum(), np.median(err[k]), np.max(err[k] / bar[k]), k.sum()))
        if not (err[k] <= bar[k]).all():
            fails.append((label, np.nonzero(k & ~(err <= bar))[0], float(np.max(err[k] / bar[k]))))
    assert not fails, fails


@pytest.mark.parametrize("dew", PROBLEMS)
def test_blocks_per_class_and_column(ctx, dew):
    """Tight rows of every class: each column in its own measure, so that a small column cannot hide behind the row maximum;
    columns the exact block leaves identically zero over a class are exactly 0.0 in the kernel's, over all kept rows of it."""
    g = ctx[dew]
    c = g.c
    fails = []
    for label, got, want, twin, _, tight in g.blocks:
        worst, n_zero = (0.0, 0.0, None), 0
        for cls in range(tref.N_CLASSES):
            rows = tight & (c.cls == cls)
            err, noise = ex.column_error(got, want, rows), ex.column_error(twin, want, rows)
            bar = np.maximum(ex.BAR_FLOOR, 10.0 * noise)
            j = int(np.argmax(err / bar))
            if err[j] / bar[j] > worst[1]:
                worst = (float(err[j]), float(err[j] / bar[j]), (cls, ex.COLUMNS[j]))
            for j in np.nonzero(~(err <= bar))[0]:
                fails.append((label, cls, ex.COLUMNS[j], float(err[j]), float(bar[j])))
            every = c.keep & (c.cls == cls)
            for j in np.nonzero((want[every] == 0.0).all(axis=0))[0]:
                n_zero += 1
                if not (got[every, j] == 0.0).all():
                    fails.append((label, cls, ex.COLUMNS[j], "must be exactly zero", float(np.abs(got[every, j]).max())))
        print("%-6s %-31s per class and column: largest err / bar %.3f (err %.2e, class and column %s); %d (class, column) pairs "
              "exactly zero" % (name(dew), label, worst[1], worst[0], worst[2], n_zero))
        assert n_zero >= 20  # class 0 alone has 10: the dipole and the association columns of both components and eps_AiBj
    assert not fails, fails


@pytest.mark.parametrize("dew", PROBLEMS)
def test_zero_parameter_entries(ctx, dew):
    """The entries whose parameter is 0 and whose exact derivative is not, on their own: held to the row bars and, per column
    over the tight rows that have such an entry, to the column bars."""
    g = ctx[dew]
    c = g.c
    k = c.keep
    fails = []
    for label, got, want, twin, bar, tight in g.blocks:
        z = (c.zero_entry_y if want is c.Jy else c.zero_entry_p) & k[:, None]
        assert z.sum() >= 400
        scale = np.abs(np.where(k[:, None], want, 1.0)).max(axis=1)
        err = np.where(z, np.abs(got - want), 0.0) / scale[:, None]
        lead = z[np.arange(c.n), np.abs(np.where(k[:, None], want, 0.0)).argmax(axis=1)]
        print("%-6s %-31s zero-parameter entries: %d, largest error %.2e of the row maximum (err / bar %.3f), the row's largest "
              "component in %d rows" % (name(dew), label, z.sum(), err.max(), np.max(err.max(axis=1)[k] / bar[k]), lead.sum()))
        if not (err.max(axis=1)[k] <= bar[k]).all():
            fails.append((label, "row", np.nonzero(k & ~(err.max(axis=1) <= bar))[0]))
        assert not (got[z] == 0.0).any(), label
        for j in np.nonzero(z.any(axis=0))[0]:
            rows = tight & z[:, j]
            e, noise = ex.column_error(got, want, rows)[j], ex.column_error(twin, want, rows)[j]
            if not e <= max(ex.BAR_FLOOR, 10.0 * noise):
                fails.append((label, ex.COLUMNS[j], float(e), float(noise)))
    assert not fails, fails


def _raw(fn, dew, a, n, n_out, workspace):
    """The ABI call `fn` on the first n rows with NaN-filled outputs; workspace None: rows bucketed inside the workgroup."""
    from feos_torch_amd import _lib, native

    a = [v[:n].contiguous() for v in a]
    out = [torch.full((n, 19), float("nan"), dtype=f64, device="cuda") for _ in range(n_out)]
    ws = native._workspace(n, a[0].device) if workspace else None
    rc = getattr(_lib.lib(), fn)(int(dew), *(_lib.ptr(v) for v in a), n, *(_lib.ptr(o) for o in out), _lib.ptr(ws),
                                 _lib.current_stream_ptr(a[0].device))
    _lib.check(rc, fn)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("dew", PROBLEMS)
def test_geometry(ctx, dew):
    """The blocks of the first n rows are bit for bit those of the full launch, with and without the class-order workspace."""
    g = ctx[dew]
    rows = np.arange(N_GEOMETRY) % g.c.n
    a = [v[torch.from_numpy(rows).cuda()].contiguous() for v in g.dev]
    keep = torch.from_numpy(g.c.keep[rows]).cuda()
    for fn, n_out in (("pcs_mix_jacobian", 1), ("pcs_mix_point_jacobian", 2)):
        full = _raw(fn, dew, a, N_GEOMETRY, n_out, True)
        plain = _raw(fn, dew, a, N_GEOMETRY, n_out, False)
        ours = (g.jac,) if n_out == 1 else (g.jp, g.jy)
        for f, p, o in zip(full, plain, ours):
            assert torch.isfinite(f[keep]).all() and _same_bits(f[keep], p[keep]), fn
            assert _same_bits(f[:g.c.n][keep[:g.c.n]], _d(o)[keep[:g.c.n]]), fn  # the launch the referee was compared with
        for n in PREFIXES:
            for ws in (True, False):
                part = _raw(fn, dew, a, n, n_out, ws)
                for f, p in zip(full, part):
                    assert p.shape[0] == n and _same_bits(p[keep[:n]], f[:n][keep[:n]]), (fn, n, ws)


@pytest.mark.parametrize("dew", PROBLEMS)
def test_gradients_through_the_model_classes(ctx, oracle, dew):
    """bubble_point / dew_point(incipient_molefracs=True) on 64 rows that all converge, upstream weights w_p, w_y ~ N(0, 1): row i
    of parameters.grad, kij.grad and T.grad under the loss w_p[i] p[i] + w_y[i] y[i] is w_p[i] J_p[i] + w_y[i] J_y[i] with the
    exact blocks at the kernel's own solved densities, every other row exactly zero.  Tolerance per row: the row bars, plus the
    referee's own change between the oracle's densities and the kernel's."""
    from feos_torch_amd import PcSaftMix, native

    g = ctx[dew]
    c = g.c
    p0 = _d(np.full(c.n, 1e5))
    r = native.mix_bubble_dew(g.dev[0], g.dev[1], g.dev[2], _d(c.z), p0, dew)
    idx = np.nonzero(c.keep & ~_np(r["status"]))[0][:N_MODEL]
    assert len(idx) == N_MODEL and set(c.cls[idx]) == set(range(tref.N_CLASSES))
    sel = torch.from_numpy(idx).cuda()
    r = native.mix_bubble_dew(g.dev[0][sel], g.dev[1][sel], g.dev[2][sel], _d(c.z[idx]), p0[:N_MODEL], dew)  # the model's own launch
    assert not r["status"].any().item()
    rho4 = _np(r["rho4"])
    Jp, Jy = ex.blocks(oracle, c.P[idx], c.K[idx], c.T[idx], rho4, dew, prec=1)
    rng = np.random.default_rng(11)
    wp, wy = rng.normal(size=N_MODEL), rng.normal(size=N_MODEL)
    want = wp[:, None] * Jp + wy[:, None] * Jy
    top_p, top_y = np.abs(c.Jp[idx]).max(axis=1), np.abs(c.Jy[idx]).max(axis=1)
    moved_p, moved_y = np.abs(Jp - c.Jp[idx]).max(axis=1), np.abs(Jy - c.Jy[idx]).max(axis=1)
    tol = np.abs(wp) * (c.bar_p[idx] * top_p + moved_p) + np.abs(wy) * (c.bar_y[idx] * top_y + moved_y)
    P, K, T = (_d(v[idx]).requires_grad_(True) for v in (c.P, c.K, c.T))
    p, nans, y = (PcSaftMix(P, K).dew_point if dew else PcSaftMix(P, K).bubble_point)(T, _d(c.z[idx]), p0[:N_MODEL], incipient_molefracs=True)
    assert not nans.any().item() and p.shape == y.shape == (N_MODEL,)
    assert _same_bits(p.detach(), r["p"])  # the densities above are the ones behind this call
    loss = _d(wp) * p + _d(wy) * y
    got = np.empty((N_MODEL, ex.N_DIRS))
    for i in range(N_MODEL):
        gP, gK, gT = torch.autograd.grad(loss[i], (P, K, T), retain_graph=True)
        full = torch.cat((gP.reshape(N_MODEL, 16), gK, gT[:, None]), dim=1)
        got[i] = _np(full[i])
        full[i] = 0.0
        assert not full.any().item(), i  # the other rows receive exactly zero
    err = np.abs(got - want).max(axis=1)
    scale = np.abs(want).max(axis=1)
    print("%-6s through the model, %d rows: largest |grad - exact| %.2e of the row's largest component, largest err / tol %.3f; "
          "moved by the densities: p %.2e, y %.2e of the block's row maximum" % (
              name(dew), N_MODEL, np.max(err / scale), np.max(err / tol), np.max(moved_p / top_p), np.max(moved_y / top_y)))
    assert (err <= tol).all(), (np.nonzero(~(err <= tol))[0], float(np.max(err / tol)))
