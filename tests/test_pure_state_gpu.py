"""GPU: the pure-component state functions and their backward kernel against long-double referees, beyond one workgroup.

pcs_pure_derivatives (k_pure_derivatives) and pcs_pure_derivatives_vjp (k_pure_derivatives_vjp, pure_jacobian.hpp::
pure_derivatives_vjp: third order in the density, dp/drho is an output) behind PcSaftPure.derivatives / helmholtz_energy, on the
rows of tests/tools/state_rows.py::pure_rows: pure_batch(700, seed=5) solved by the oracle's long-double pure_vle (none dropped;
341 polar, 361 associating) -- two full 256-lane workgroups and a ragged third -- each at its vapour, its liquid and that liquid
compressed by 1.15.

Backward: all 10 columns of every row against oracle.pure_derivatives_vjp_exact (nested duals in long double, checked on the CPU by
tests/test_oracle_state_grad.py).  Error per row and INPUT GROUP (parameters[8], T, rho) relative to the group's largest exact
component in that row; bar max(1e-10, 10 e), e = the referee's fp64 run against its long-double run in the same measure
(tests/test_mixn_gpu.py).  From the referee alone: largest e 1.7e-7 (one compressed-liquid row's T column, where the three weighted
terms cancel), every vapour group at most 9.0e-15; rows with a bar above 1e-8: at most 0.57 % of a group and state (5 % allowed).
Forward: a, p at (1e-13, 1e-12) in the measures of tests/test_mix_gpu.py::test_derivatives_random_rows (p scale max(|p|, rho))
plus 10 x the fp64 oracle's error on the same row; dp/drho, for which the project has no floor, at max(DP_FLOOR, 10 x the fp64
oracle's error on the same row) in |d dp| / max(|dp|, 1), DP_FLOOR = 10 x the largest such error of the fp64 oracle over the vapour
rows = 8.3e-15 (computed in the test); at most 10 % of the rows may need more than the floors.
Measured kernel error: at most 1.6e-12, at most 0.016 of its bar (table in test_backward_vs_exact_gradient).
Sensitivity, tried on a scratch build and not kept: the (gdp rho) a2-tangent term of pure_derivatives_vjp scaled by 1 + 1e-6 gives
1.0e-6 in the parameter and T groups and 2.4e-7 in rho (10^4 bars: red; tests/test_deriv_grad_gpu.py is red too, its weights put
the same term above its 1e-7)."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import state_rows as sr  # noqa: E402

pytestmark = pytest.mark.gpu
f64 = torch.float64
FWD_TOL = (1e-13, 1e-12)
BLOCK = sr.pure_block()
CUTS = (1, 63, 64, 65, 128, 129, BLOCK - 1, BLOCK, BLOCK + 1)


@pytest.fixture(scope="module")
def amd():
    assert torch.cuda.is_available()
    import feos_torch_amd

    return feos_torch_amd


def _dev(x):
    return torch.tensor(np.asarray(x), dtype=f64).cuda()


def _bits(x):
    return x.detach().cpu().contiguous().view(torch.int64)


def _np(x):
    return x.detach().cpu().numpy()


def _vjp(native, *args):
    """pcs_pure_derivatives_vjp as one [n, 10] array: 8 parameters, T, rho"""
    gp, gt, gr = native.pure_derivatives_vjp(*args)
    return torch.cat([gp, gt[:, None], gr[:, None]], dim=1)


def test_row_set(oracle):
    """At least two full workgroups of k_pure_derivatives_vjp and a ragged one; both kinds of rows present."""
    q = sr.pure_rows(oracle)
    n, P = q["n"], q["P"]
    polar, assoc = int((P[:, 3] != 0.0).sum()), int(((P[:, 6] + P[:, 7]) != 0.0).sum())
    print(f"\n{n} rows ({q['dropped']} dropped), BLOCK {BLOCK}: {polar} polar, {assoc} associating")
    assert BLOCK % 64 == 0 and n > 2 * BLOCK and n % BLOCK != 0
    assert q["dropped"] <= 0.03 * 700 and polar > 0 and assoc > 0 and polar < n and assoc < n


def test_backward_vs_exact_gradient(amd, oracle):
    """Every row, state and column; nothing left out.  Also: the mu column is exactly 0 where mu = 0, the four association columns
    are exactly 0 on rows without sites and na, nb columns are non-zero on rows with them.

    Measured on an MI355X, kernel error largest (largest err / bar), parameters / T / rho:
      vapour     1.95e-15 (0.000)  1.87e-15 (0.000)  1.67e-15 (0.000)
      liquid     2.51e-14 (0.000)  1.61e-12 (0.016)  5.24e-15 (0.000)
      compressed 2.08e-14 (0.000)  3.91e-13 (0.004)  7.94e-15 (0.000)
    the referee's own e (fp64 against long double), largest: 8.6e-15 / 2.2e-15 / 9.0e-15 (vapour), 1.1e-8 / 3.0e-8 / 2.7e-9
    (liquid), 4.0e-9 / 1.7e-7 / 3.3e-9 (compressed); rows with a bar above 1e-8: 0.57 % at most."""
    from feos_torch_amd import native

    q = sr.pure_rows(oracle)
    n, P = q["n"], q["P"]
    bars = sr.bars(q, sr.PURE_GROUPS)
    for state in sr.STATES:  # the bars hide nothing: from the referee alone, before the kernel is looked at
        for g, (e, bar) in bars[state].items():
            assert np.isfinite(e).all() and np.mean(bar > 1e-8) <= 0.05, (state, g, float(np.mean(bar > 1e-8)))
    Pd, Td = _dev(P), _dev(q["T"])
    sites = (P[:, 6] + P[:, 7]) != 0.0
    print()
    for state in sr.STATES:
        want = q["exact"][state]
        got = _np(_vjp(native, Pd, Td, _dev(q["states"][state]), *(_dev(x) for x in q["w"][state])))
        assert got.shape == (n, 10) and np.isfinite(got).all()
        err = sr.group_error(got, want, sr.PURE_GROUPS)
        line = []
        for g, (e, bar) in bars[state].items():
            line.append(f"{g} {err[g].max():.2e} ({np.max(err[g] / bar):.3f}; e {e.max():.2e}, bar > 1e-8: {100 * np.mean(bar > 1e-8):.2f} %)")
        print(f"   {state:10s} " + "  ".join(line))
        for g, (e, bar) in bars[state].items():
            assert (err[g] <= bar).all(), (state, g, int(np.argmax(err[g] / bar)), float(err[g].max()), float(np.max(err[g] / bar)))
        for side in (got, want):
            assert np.all(side[:, 3][P[:, 3] == 0.0] == 0.0)
            assert np.all(side[:, 4:8][~sites] == 0.0)
            assert np.all(side[:, 6:8][sites] != 0.0)


def _fwd_errors(a, p, dp, A, Pp, DP, rho):
    return (np.abs(a - A) / np.maximum(np.abs(A), 1e-6), np.abs(p - Pp) / np.maximum(np.abs(Pp), rho),
            np.abs(dp - DP) / np.maximum(np.abs(DP), 1.0))


def test_forward_vs_long_double_oracle(amd, oracle):
    """a, p, dp/drho of every row and state through PcSaftPure.derivatives against pure_derivatives(prec=1); helmholtz_energy is
    `a` bit for bit.  DP_FLOOR comes from the fp64 oracle on the vapour rows (module docstring): measured 8.33e-15.

    Measured on an MI355X, worst (a, p, dp) per state, and the fp64 oracle against the same values:
      vapour     2.54e-14 3.72e-16 4.44e-16   (4.12e-14 4.72e-16 8.33e-16)
      liquid     2.13e-15 4.42e-14 8.64e-15   (3.89e-11 4.38e-09 2.24e-10)
      compressed 2.49e-15 1.27e-14 6.58e-15   (6.57e-11 2.61e-10 1.34e-09)
    2 of 700 rows needed more than the floors (0.29 %, cap 10 %)."""
    q = sr.pure_rows(oracle)
    n = q["n"]
    eos = amd.PcSaftPure(_dev(q["P"]))
    T = _dev(q["T"])
    exact = {s: oracle.pure_derivatives(q["P"], q["T"], rho, prec=1) for s, rho in q["states"].items()}
    noise = {s: _fwd_errors(*oracle.pure_derivatives(q["P"], q["T"], rho), *exact[s], rho) for s, rho in q["states"].items()}
    dp_floor = 10.0 * noise["vapour"][2].max()
    print(f"\n   DP_FLOOR = {dp_floor:.2e}")
    assert 0.0 < dp_floor < 1e-13  # ten times a few roundings of a number of size 1
    need = np.zeros(n, bool)
    for state, rho in q["states"].items():
        a, p, dp = eos.derivatives(T, _dev(rho))
        h = eos.helmholtz_energy(T, _dev(rho))
        assert h.shape == (n,) and torch.equal(_bits(h), _bits(a))
        errs = _fwd_errors(_np(a), _np(p), _np(dp), *exact[state], rho)
        nz = noise[state]
        print(f"   {state:10s} a {errs[0].max():.2e} p {errs[1].max():.2e} dp {errs[2].max():.2e}   "
              f"(fp64 oracle: {nz[0].max():.2e} {nz[1].max():.2e} {nz[2].max():.2e})")
        for k, name in enumerate(("a", "p")):
            assert np.isfinite(errs[k]).all() and np.all(errs[k] <= FWD_TOL[k] + 10.0 * nz[k]), (state, name, float(errs[k].max()))
            need |= ~(errs[k] < FWD_TOL[k])
        assert np.isfinite(errs[2]).all() and np.all(errs[2] <= np.maximum(dp_floor, 10.0 * nz[2])), (state, "dp", float(errs[2].max()))
        need |= ~(errs[2] <= dp_floor)
    print(f"   rows that needed more than the floors: {need.sum()} of {n} ({100 * need.mean():.2f} %)")
    assert need.mean() <= 0.10


def test_results_do_not_depend_on_batch(amd, oracle):
    """The first n rows of the 700-row call have the bits of an n-row call, forward and backward, in every state: n = one lane, a
    wave +- 1, two waves + 1, a workgroup +- 1 (the staged parameter tile, the repeated last row of a ragged workgroup)."""
    from feos_torch_amd import native

    q = sr.pure_rows(oracle)
    n = q["n"]
    Pd, Td = _dev(q["P"]), _dev(q["T"])
    for state in sr.STATES:
        rd, wd = _dev(q["states"][state]), [_dev(x) for x in q["w"][state]]
        full = [_bits(x) for x in (*native.pure_derivatives(Pd, Td, rd), _vjp(native, Pd, Td, rd, *wd))]
        for k in (*CUTS, n):
            part = (*native.pure_derivatives(Pd[:k], Td[:k], rd[:k]), _vjp(native, Pd[:k], Td[:k], rd[:k], *(x[:k] for x in wd)))
            for name, f, g in zip(("a", "p", "dp", "grad"), full, part):
                assert g.shape[0] == k and torch.equal(_bits(g), f[:k]), (state, k, name)


LINEAR_ROWS = 130  # two waves and a two-lane tail of one workgroup; half the rows polar, half associating


def _linear_case(oracle):
    """Rows, states and the seed of the upstream weights of test_optional_upstreams: the first 130 rows, row i in state i % 3.
    The seed is the first from 5100 on for which the fp64 REFEREE is linear to 1e-14 on every row
    (tests/test_mixn_gpu.py::test_vjp_optional_upstreams)."""
    q = sr.pure_rows(oracle)
    n = LINEAR_ROWS
    P, T = q["P"][:n], q["T"][:n]
    rho = np.array([q["states"][sr.STATES[i % 3]][i] for i in range(n)])
    for seed in range(5100, 5200):
        rng = np.random.default_rng(seed)
        w = [rng.normal(size=n), rng.normal(size=n), rng.normal(size=n)]
        z = np.zeros(n)
        single = [oracle.pure_derivatives_vjp_exact(P, T, rho, *(w[j] if j == k else z for j in range(3)), prec=0) for k in range(3)]
        total = oracle.pure_derivatives_vjp_exact(P, T, rho, *w, prec=0)
        ref_err = np.abs(total - sum(single)).max(axis=1) / np.abs(total).max(axis=1)
        if ref_err.max() < 1e-14:
            return P, T, rho, w, seed, float(ref_err.max())
    raise AssertionError("no seed with a linear fp64 referee")


def test_optional_upstreams(amd, oracle):
    """g_* = None is an explicit zero (bits) for every subset, all None gives zeros, and the gradient is linear in the upstreams:
    all three together equal the sum of the three single-upstream gradients to 1e-13 of the row's largest component.
    Measured: seed 5100 (the first tried), fp64 referee linear to 0, kernel to 2.4e-16."""
    from feos_torch_amd import native

    P, T, rho, w, seed, ref_err = _linear_case(oracle)
    assert ref_err < 1e-14
    Pd, Td, rd = _dev(P), _dev(T), _dev(rho)
    w = [_dev(x) for x in w]
    single = []
    for keep in itertools.product((False, True), repeat=3):
        with_none = _vjp(native, Pd, Td, rd, *(x if k else None for x, k in zip(w, keep)))
        with_zero = _vjp(native, Pd, Td, rd, *(x if k else torch.zeros_like(x) for x, k in zip(w, keep)))
        assert torch.equal(_bits(with_none), _bits(with_zero)), keep
        if sum(keep) == 1:
            single.append(_np(with_none))
    assert len(single) == 3
    assert np.all(_np(_vjp(native, Pd, Td, rd)) == 0.0)
    total = _np(_vjp(native, Pd, Td, rd, *w))
    err = np.abs(total - sum(single)).max(axis=1) / np.abs(total).max(axis=1)
    print(f"\n   seed {seed}: fp64 referee linear to {ref_err:.2e}, kernel to {err.max():.2e} (row {err.argmax()})")
    assert err.max() < 1e-13


def test_shell_backward_equals_the_abi(amd, oracle):
    """PcSaftPure(P).derivatives(T, rho) and backward of the weighted sum: P.grad, T.grad and rho.grad carry the bits of
    native.pure_derivatives_vjp; backward of helmholtz_energy is the g_a-only call."""
    from feos_torch_amd import PcSaftPure, native

    q = sr.pure_rows(oracle)
    n = q["n"]
    for state in ("vapour", "compressed"):
        wd = [_dev(x) for x in q["w"][state]]
        Pt, Tt, rt = (_dev(x).requires_grad_(True) for x in (q["P"], q["T"], q["states"][state]))
        out = PcSaftPure(Pt).derivatives(Tt, rt)
        assert [tuple(o.shape) for o in out] == [(n,), (n,), (n,)]
        sum((o * x).sum() for o, x in zip(out, wd)).backward()
        gp, gt, gr = native.pure_derivatives_vjp(Pt.detach(), Tt.detach(), rt.detach(), *wd)
        assert Pt.grad.shape == (n, 8) and torch.equal(_bits(Pt.grad), _bits(gp))
        assert Tt.grad.shape == (n,) and torch.equal(_bits(Tt.grad), _bits(gt))
        assert rt.grad.shape == (n,) and torch.equal(_bits(rt.grad), _bits(gr))
        Pt, Tt, rt = (_dev(x).requires_grad_(True) for x in (q["P"], q["T"], q["states"][state]))
        (PcSaftPure(Pt).helmholtz_energy(Tt, rt) * wd[0]).sum().backward()
        gp, gt, gr = native.pure_derivatives_vjp(Pt.detach(), Tt.detach(), rt.detach(), wd[0])
        assert torch.equal(_bits(Pt.grad), _bits(gp)) and torch.equal(_bits(Tt.grad), _bits(gt)) and torch.equal(_bits(rt.grad), _bits(gr))
