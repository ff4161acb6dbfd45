"""n-component mixtures: `PcSaftMix(parameters[N, n, 8]).derivatives / helmholtz_energy_density` on the GPU.

What pins it.  The reference's n-component code path cannot be run (with kij = None, which n != 2 demands,
feos_torch/pcsaft_mix.py:75-76, helmholtz_energy_density fails at `self.kij[...]`, :141), so there are no reference outputs for
n > 2: "parity unpinned by stored values".  Instead:
  * n = 2, kij = 0, at most one associating component: outputs of the UNMODIFIED reference (tests/golden/mixn.json), reproduced by
    the n-component kernel at nc = 2 to the reference's tolerances (tests/test_pcsaft_mix.py:119-124) and by the binary kernel;
  * nc = 1 ... 6 on random rows: the long-double oracle restatement of the same lines (oracle/pcsaft_mixn.hpp), itself checked
    against those reference outputs (tests/test_oracle_mixn.py);
  * exact properties of the model for any n: splitting a component into two identical ones with the densities shared out
    changes nothing (a, p, mu_i, v_i); permuting the components permutes mu and v; nc = 1 is PcSaftPure.

The backward kernel (pcs_mixn_derivatives_vjp) is held to the exact gradient: oracle.mixn_derivatives_vjp_exact, nested duals in
long double over the same lines, every one of the 9 nc + 1 columns seeded (tests/test_oracle_mixn.py checks that referee on the
CPU).  257 rows per nc = four full 64-lane workgroups and a one-lane tail.  Error measure: relative to the row's largest
gradient component (tests/test_deriv_grad_gpu.py).  Bar per row: max(FLOOR, 10 e_row), e_row = the same quotient of the
referee's own fp64 run (prec=0) against its long-double run -- the kernel may be ten times worse than an fp64 evaluation of the
same formulas, the factor of tests/test_mix_temperature_gpu.py and tests/test_boiling_gpu.py.  FLOOR = 1e-10 as in those files:
the referee's own rounding stays far below it (median e_row 4e-16 ... 1.6e-15, 95 % of the rows below 8e-14).
Measured with the committed seeds (EXACT_SEED + nc), nc = 1 / 2 / 3 / 4 / 5 / 6:
    largest e_row          7.9e-11 / 5.4e-13 / 4.1e-13 / 1.9e-11 / 1.0e-12 / 1.0e-12
    rows with bar > 1e-8   0 / 0 / 0 / 0 / 0 / 0 of 257 (at most 5 % allowed); rows with bar > FLOOR: 2 / 0 / 0 / 1 / 0 / 0
    kernel error, largest  3.5e-12 / 9.7e-13 / 1.8e-13 / 3.7e-12 / 8.8e-13 / 3.2e-13 (median 2.7e-16 ... 1.0e-15)
    kernel error / bar     0.007 / 0.010 / 0.002 / 0.020 / 0.009 / 0.003 at most
Sensitivity, tried on a scratch build: the e12 term of HV::chain scaled by 1 + 1e-6 gives 4e-5 ... 2e-3 at nc = 2 ... 6 (red) while
test_vjp_vs_finite_differences_of_the_oracle stays green."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
from mixn_rows import random_rows  # noqa: E402

pytestmark = pytest.mark.gpu
f64 = torch.float64


@pytest.fixture(scope="module")
def amd():
    assert torch.cuda.is_available()
    import feos_torch_amd

    return feos_torch_amd


def _t(x):
    return torch.tensor(np.asarray(x), dtype=f64)


def test_nc2_vs_reference_python(amd):
    g = load_golden("mixn.json")["nc2_kij0"]
    from feos_torch_amd import native

    P, T, rho = (np.array(g[k]) for k in ("params", "T", "rho"))
    a, p, mu, v = (x.cpu().numpy() for x in native.mixn_derivatives(_t(P).cuda(), _t(T).cuda(), _t(rho).cuda()))
    assert np.max(np.abs(a - np.array(g["a"]))) < 1e-14
    assert np.max(np.abs(p - np.array(g["p"]))) < 1e-14
    assert np.max(np.abs(mu - np.array(g["mu"]))) < 1e-13
    assert np.max(np.abs(v / np.array(g["v"]) - 1.0)) < 1e-11
    # and the binary kernel (k_ij = 0) gives the same
    a2, p2, mu2, v2 = amd.PcSaftMix(_t(P), torch.zeros((len(T), 2), dtype=f64)).derivatives(_t(T), _t(rho))
    assert np.max(np.abs(a2.numpy() - a)) < 1e-14 and np.max(np.abs(mu2.numpy() - mu)) < 1e-13
    assert np.max(np.abs(v2.numpy() / v - 1.0)) < 1e-11


@pytest.mark.parametrize("nc", [1, 2, 3, 4, 5, 6])
def test_random_rows_vs_oracle(amd, oracle, nc):
    P, T, rho = random_rows(3000, nc, seed=100 + nc)
    eos = amd.PcSaftMix(_t(P))
    a, p, mu, v = (x.numpy() for x in eos.derivatives(_t(T), _t(rho)))
    A, Pp, MU, V = oracle.mixn_derivatives(P, T, rho, prec=1)
    assert np.max(np.abs(a - A) / np.maximum(np.abs(A), 1e-6)) < 1e-12
    assert np.max(np.abs(p - Pp) / np.maximum(np.abs(Pp), rho.sum(axis=1))) < 1e-11
    assert np.max(np.abs(mu - MU) / np.maximum(1.0, np.abs(MU))) < 1e-12
    assert np.max(np.abs(v / V - 1.0)) < 1e-9
    h = eos.helmholtz_energy_density(_t(T), _t(rho))
    assert h.shape == (3000, 1) and np.array_equal(h[:, 0].numpy(), a)


def test_splitting_and_permutation(amd):
    P, T, rho = random_rows(2000, 3, seed=7, assoc=False)
    a, p, mu, v = (x.numpy() for x in amd.PcSaftMix(_t(P)).derivatives(_t(T), _t(rho)))
    # split component 2 into two identical components carrying 30 % / 70 % of its density: 4 components
    P4 = np.concatenate([P, P[:, 2:3, :]], axis=1)
    rho4 = np.concatenate([rho[:, :2], 0.3 * rho[:, 2:3], 0.7 * rho[:, 2:3]], axis=1)
    a4, p4, mu4, v4 = (x.numpy() for x in amd.PcSaftMix(_t(P4)).derivatives(_t(T), _t(rho4)))
    assert np.max(np.abs(a4 - a) / np.maximum(np.abs(a), 1e-9)) < 1e-12
    assert np.max(np.abs(p4 - p) / np.maximum(np.abs(p), rho.sum(axis=1))) < 1e-11
    assert np.max(np.abs(mu4[:, :3] - mu)) < 1e-11 and np.max(np.abs(mu4[:, 3] - mu4[:, 2])) < 1e-11
    assert np.max(np.abs(v4[:, :3] / v - 1.0)) < 1e-9
    # permutation of the components
    perm = [2, 0, 1]
    ap, pp, mup, vp = (x.numpy() for x in amd.PcSaftMix(_t(P[:, perm])).derivatives(_t(T), _t(rho[:, perm])))
    assert np.max(np.abs(ap - a) / np.maximum(np.abs(a), 1e-9)) < 1e-12
    assert np.max(np.abs(mup - mu[:, perm])) < 1e-11 and np.max(np.abs(vp / v[:, perm] - 1.0)) < 1e-9


def test_one_component_is_the_pure_model(amd):
    P, T, rho = random_rows(2000, 1, seed=3)
    a, p, mu, v = amd.PcSaftMix(_t(P)).derivatives(_t(T), _t(rho))
    a1, p1, dp1 = amd.PcSaftPure(_t(P[:, 0])).derivatives(_t(T), _t(rho[:, 0]))
    assert np.max(np.abs(a.numpy() - a1.numpy()) / np.maximum(np.abs(a1.numpy()), 1e-9)) < 1e-12
    assert np.max(np.abs(p.numpy() - p1.numpy()) / np.maximum(np.abs(p1.numpy()), rho[:, 0])) < 1e-11
    # one component: v = (1 + rho a'') / (rho + rho^2 a'') = 1 / rho, mu = a'
    assert np.max(np.abs(v[:, 0].numpy() * rho[:, 0] - 1.0)) < 1e-12
    assert np.max(np.abs((p.numpy() - rho[:, 0] + a.numpy()) / rho[:, 0] - mu[:, 0].numpy())) < 1e-8


def test_api_errors(amd):
    P, T, rho = random_rows(4, 3, seed=1, assoc=False)
    with pytest.raises(Exception, match="kij can only be used for binary mixtures"):
        amd.PcSaftMix(_t(P), torch.zeros((4, 2), dtype=f64))
    Pa = P.copy()
    Pa[0, 0, 4:8] = [0.01, 2000.0, 1, 1]
    Pa[0, 1, 4:8] = [0.01, 2000.0, 1, 1]
    with pytest.raises(Exception, match="associating components"):
        amd.PcSaftMix(_t(Pa))
    eos = amd.PcSaftMix(_t(P))
    with pytest.raises(Exception, match="binary"):
        eos.bubble_point(_t(T), _t([0.5] * 4), _t([1e5] * 4))
    with pytest.raises(ValueError):
        eos.derivatives(_t(T[:3]), _t(rho))
    with pytest.raises(ValueError):
        amd.PcSaftMix(_t(np.zeros((2, 7, 8))))


def test_vjp_nc2_equals_the_binary_backward(amd):
    """n = 2, k_ij = 0, at most one associating component: the n-component backward pass (pcs_mixn_derivatives_vjp) against the
    binary one (pcs_mix_derivatives_vjp), which tests/test_deriv_grad_gpu.py pins on the reference's own autograd."""
    from feos_torch_amd import native

    P, T, rho = random_rows(400, 2, seed=31)
    n = len(T)
    rng = np.random.default_rng(2)
    ga, gp, gmu, gv = rng.normal(size=n), rng.normal(size=n), rng.normal(size=(n, 2)), rng.normal(size=(n, 2)) * 1e-3
    d = lambda x: _t(x).cuda()
    g = native.mixn_derivatives_vjp(d(P), d(T), d(rho), d(ga), d(gp), d(gmu), d(gv)).cpu().numpy()
    gb = native.mix_derivatives_vjp(d(P), d(np.zeros((n, 2))), d(T), d(rho), d(ga), d(gp), d(gmu), d(gv)).cpu().numpy()
    want = np.concatenate([gb[:, 0:16], gb[:, 18:21]], axis=1)  # (16 parameters, T, rho_0, rho_1); k_ij columns dropped
    scale = np.abs(want).max(axis=1, keepdims=True)
    assert np.max(np.abs(g - want) / scale) < 1e-9


@pytest.mark.parametrize("nc", [1, 3, 4, 6])
def test_vjp_vs_finite_differences_of_the_oracle(amd, oracle, nc):
    """dL/d(parameters, T, rho) for nc components against central differences of L evaluated with the long-double oracle
    restatement (oracle/pcsaft_mixn.hpp)."""
    from feos_torch_amd import native

    P, T, rho = random_rows(24, nc, seed=40 + nc)
    n = len(T)
    rng = np.random.default_rng(nc)
    ga, gp, gmu, gv = rng.normal(size=n), rng.normal(size=n), rng.normal(size=(n, nc)), rng.normal(size=(n, nc)) * 1e-3
    d = lambda x: _t(x).cuda()
    g = native.mixn_derivatives_vjp(d(P), d(T), d(rho), d(ga), d(gp), d(gmu), d(gv)).cpu().numpy()

    def L(P_, T_, rho_):
        a, p, mu, v = oracle.mixn_derivatives(P_, T_, rho_, prec=1)
        return ga * a + gp * p + (gmu * mu).sum(axis=1) + (gv * v).sum(axis=1)

    fd = np.zeros_like(g)
    for k in range(8 * nc + 1 + nc):
        Pp, Pm, Tp, Tm, rp, rm = P.copy(), P.copy(), T.copy(), T.copy(), rho.copy(), rho.copy()
        if k < 8 * nc:
            c, q = divmod(k, 8)
            if q >= 6 or np.all(P[:, c, q] == 0.0):
                # site counts (class switches) and columns that are zero on every row (the relative step has nothing to scale
                # with; the reference's formula still has a derivative there, e.g. w.r.t. kappa_ab of a site-less component,
                # :211-218): not compared
                fd[:, k] = g[:, k]
                continue
            h = 1e-6 * np.where(P[:, c, q] != 0.0, np.abs(P[:, c, q]), 1.0)
            Pp[:, c, q] += h
            Pm[:, c, q] -= h
            mask = P[:, c, q] != 0.0
        elif k == 8 * nc:
            h = 1e-6 * T
            Tp, Tm = T + h, T - h
            mask = np.ones(n, bool)
        else:
            i = k - 8 * nc - 1
            h = 1e-6 * rho[:, i]
            rp[:, i] += h
            rm[:, i] -= h
            mask = np.ones(n, bool)
        fd[:, k] = np.where(mask, (L(Pp, Tp, rp) - L(Pm, Tm, rm)) / (2 * h), g[:, k])
    cols = [k for k in range(9 * nc + 1) if not (k < 8 * nc and k % 8 >= 6)]
    scale = np.abs(fd[:, cols]).max(axis=1, keepdims=True) + 1e-300
    err = np.abs(g[:, cols] - fd[:, cols]) / np.maximum(np.abs(fd[:, cols]), 1e-6 * scale)
    assert np.nanmax(err) < 2e-4, np.nanmax(err)


def test_shell_is_differentiable_for_three_components(amd):
    from feos_torch_amd import PcSaftMix

    P, T, rho = random_rows(50, 3, seed=77)
    Pt = _t(P).cuda().requires_grad_(True)
    Tt = _t(T).cuda().requires_grad_(True)
    rt = _t(rho).cuda().requires_grad_(True)
    a, p, mu, v = PcSaftMix(Pt).derivatives(Tt, rt)
    (a.sum() + p.sum() + mu.sum()).backward()
    assert Pt.grad.shape == (50, 3, 8) and torch.isfinite(Pt.grad).all() and torch.isfinite(Tt.grad).all() and torch.isfinite(rt.grad).all()
    # d a / d rho_i = mu_i (the residual chemical potential is the density derivative of the Helmholtz energy density)
    Pt2, rt2 = _t(P).cuda(), _t(rho).cuda().requires_grad_(True)
    a2, _, mu2, _ = PcSaftMix(Pt2).derivatives(_t(T).cuda(), rt2)
    a2.sum().backward()
    assert torch.allclose(rt2.grad, mu2.detach(), rtol=1e-10, atol=1e-12)


# ---- the backward kernel against the exact gradient --------------------------------------------------------------------------
EXACT_SEED = 600
EXACT_ROWS = 257  # four full 64-lane workgroups and a one-lane tail
FLOOR = 1e-10
_cases = {}


def _case(oracle, nc):
    """rows, upstream weights and the referee's two runs for nc components (computed once per session, never modified)"""
    if nc not in _cases:
        n = EXACT_ROWS
        P, T, rho = random_rows(n, nc, EXACT_SEED + nc)
        rng = np.random.default_rng(EXACT_SEED + 50 + nc)
        w = rng.normal(size=n), rng.normal(size=n), rng.normal(size=(n, nc)), rng.normal(size=(n, nc)) * 1e-3
        g1 = oracle.mixn_derivatives_vjp_exact(P, T, rho, *w, prec=1)
        g0 = oracle.mixn_derivatives_vjp_exact(P, T, rho, *w, prec=0)
        for x in (P, T, rho, *w, g1, g0):
            x.setflags(write=False)
        _cases[nc] = P, T, rho, w, g1, g0
    return _cases[nc]


def _dev(x):
    return _t(x).cuda()


def _bits(x):
    return x.detach().cpu().contiguous().view(torch.int64)


@pytest.mark.parametrize("nc", [1, 2, 3, 4, 5, 6])
def test_vjp_vs_exact_gradient(amd, oracle, nc):
    """Every column of every row against the long-double referee, bar max(FLOOR, 10 e_row) per row (module docstring).  Nothing
    is left out: the referee's formula is differentiable in na, nb of a site-less component too (they enter sum na, the
    site-weighted sigma and d, rhoa and rhob; the class is decided on the values), and both sides seed them the same way, so
    those entries are compared like all others -- as are kappa_ab and epsilon_k_ab of site-less components next to an
    associating one, and na, nb of the associating component.  Where mu_i = 0 the mu column must be exactly 0."""
    from feos_torch_amd import native

    P, T, rho, w, g1, g0 = _case(oracle, nc)
    n = len(T)
    scale = np.abs(g1).max(axis=1)
    e_row = np.abs(g0 - g1).max(axis=1) / scale
    bar = np.maximum(FLOOR, 10.0 * e_row)
    assert np.mean(bar > 1e-8) <= 0.05  # the per-row bar hides nothing (from the referee alone)
    g = native.mixn_derivatives_vjp(_dev(P), _dev(T), _dev(rho), *(_dev(x) for x in w)).cpu().numpy()
    assert g.shape == (n, 9 * nc + 1) and np.isfinite(g).all()
    err = np.abs(g - g1).max(axis=1) / scale
    print(f"nc={nc}: largest e_row {e_row.max():.2e}, rows with bar > 1e-8: {np.sum(bar > 1e-8)}, > floor: {np.sum(bar > FLOOR)}; "
          f"kernel error largest {err.max():.2e} (row {err.argmax()}), median {np.median(err):.2e}, largest err / bar {np.max(err / bar):.3f}")
    assert (err <= bar).all(), (err.max(), np.max(err / bar))
    # the coverage this test is for: site-count columns and zero-valued association columns are non-zero and compared
    assoc = (P[:, :, 6] + P[:, :, 7]) != 0.0
    gp8 = g[:, : 8 * nc].reshape(n, nc, 8)
    assert np.all(gp8[:, :, 6:8][assoc] != 0.0)
    if nc > 1:
        beside = ~assoc & assoc.any(axis=1, keepdims=True)
        assert beside.any() and np.all(gp8[:, :, 4:8][beside] != 0.0)
    assert np.all(gp8[:, :, 3][P[:, :, 3] == 0.0] == 0.0)
    assert np.all(gp8[:, :, 4:8][~assoc.any(axis=1)] == 0.0)


@pytest.mark.parametrize("nc", [3, 6])
def test_vjp_and_forward_prefixes_are_bit_identical(amd, oracle, nc):
    """A row's results do not depend on how many rows follow it: the first n rows of the 257-row call have the bits of an n-row
    call, for n at the workgroup boundaries (the row * (9 nc + 1) + dir indexing past blockIdx.x == 0, the tail guard)."""
    from feos_torch_amd import native

    P, T, rho, w, _, _ = _case(oracle, nc)
    Pd, Td, rd, wd = _dev(P), _dev(T), _dev(rho), [_dev(x) for x in w]
    full = [_bits(x) for x in (*native.mixn_derivatives(Pd, Td, rd), native.mixn_derivatives_vjp(Pd, Td, rd, *wd))]
    for n in (1, 63, 64, 65, 128, 129, 257):
        part = (*native.mixn_derivatives(Pd[:n], Td[:n], rd[:n]), native.mixn_derivatives_vjp(Pd[:n], Td[:n], rd[:n], *(x[:n] for x in wd)))
        for name, f, q in zip(("a", "p", "mu", "v", "grad"), full, part):
            assert q.shape[0] == n and torch.equal(_bits(q), f[:n]), (n, name)


def test_vjp_optional_upstreams(amd, oracle):
    """g_* = None is the same as an explicit zero (bits), for every subset; and the gradient is linear in the upstreams: all four
    together equal the sum of the four single-upstream gradients to 1e-13 of the row's largest component.
    The rounding of that sum is u = 1.1e-16 times the sum of the |products| g_x dx/d(input), not times the result: on a gas
    row all v_c have the derivative -1 / rho^2 in every density column, so a row whose four g_v happen to add up to nearly
    nothing cancels in its largest components (seed 614: the fp64 referee itself is linear only to 1.7e-13 on one such row).
    The seed is therefore chosen by the referee alone: its fp64 run must be linear to 1e-14 on every row (asserted; measured
    4.3e-15), which leaves the kernel the usual factor 10.  Measured on the kernel: 8.4e-15."""
    from feos_torch_amd import native

    nc, n = 4, 130
    P, T, rho = random_rows(n, nc, EXACT_SEED + 15)
    rng = np.random.default_rng(EXACT_SEED + 65)
    w = [rng.normal(size=n), rng.normal(size=n), rng.normal(size=(n, nc)), rng.normal(size=(n, nc)) * 1e-3]
    z = [np.zeros_like(x) for x in w]
    ref_single = [oracle.mixn_derivatives_vjp_exact(P, T, rho, *(w[j] if j == k else z[j] for j in range(4)), prec=0) for k in range(4)]
    ref_total = oracle.mixn_derivatives_vjp_exact(P, T, rho, *w, prec=0)
    ref_err = np.abs(ref_total - sum(ref_single)).max(axis=1) / np.abs(ref_total).max(axis=1)
    assert ref_err.max() < 1e-14, ref_err.max()
    w = [_dev(x) for x in w]
    Pd, Td, rd = _dev(P), _dev(T), _dev(rho)
    single = []
    for keep in itertools.product((False, True), repeat=4):
        with_none = native.mixn_derivatives_vjp(Pd, Td, rd, *(x if k else None for x, k in zip(w, keep)))
        with_zero = native.mixn_derivatives_vjp(Pd, Td, rd, *(x if k else torch.zeros_like(x) for x, k in zip(w, keep)))
        assert torch.equal(_bits(with_none), _bits(with_zero)), keep
        if sum(keep) == 1:
            single.append(with_none.cpu().numpy())
    assert len(single) == 4
    total = native.mixn_derivatives_vjp(Pd, Td, rd, *w).cpu().numpy()
    assert np.all(native.mixn_derivatives_vjp(Pd, Td, rd).cpu().numpy() == 0.0)
    err = np.abs(total - sum(single)).max(axis=1) / np.abs(total).max(axis=1)
    print(f"linearity: {err.max():.2e}")
    assert err.max() < 1e-13


@pytest.mark.parametrize("nc", [3, 5])
def test_shell_backward_equals_the_abi(amd, oracle, nc):
    """PcSaftMix(P).derivatives(T, rho) and backward of the weighted sum: P.grad, T.grad and rho.grad carry the bits of the
    matching columns of native.mixn_derivatives_vjp (the column table of feos_torch_amd/pcsaft_mix.py)."""
    from feos_torch_amd import PcSaftMix, native

    P, T, rho, w, _, _ = _case(oracle, nc)
    n = len(T)
    Pt, Tt, rt = (_dev(x).requires_grad_(True) for x in (P, T, rho))
    wd = [_dev(x) for x in w]
    out = PcSaftMix(Pt).derivatives(Tt, rt)
    assert [tuple(o.shape) for o in out] == [(n,), (n,), (n, nc), (n, nc)]
    sum((o * x).sum() for o, x in zip(out, wd)).backward()
    g = native.mixn_derivatives_vjp(Pt.detach(), Tt.detach(), rt.detach(), *wd)
    assert Pt.grad.shape == (n, nc, 8) and torch.equal(_bits(Pt.grad).reshape(n, 8 * nc), _bits(g[:, : 8 * nc]))
    assert Tt.grad.shape == (n,) and torch.equal(_bits(Tt.grad), _bits(g[:, 8 * nc]))
    assert rt.grad.shape == (n, nc) and torch.equal(_bits(rt.grad), _bits(g[:, 8 * nc + 1 :]))
