"""GPU: the binary state functions and their backward kernel against long-double referees, beyond one wave.

pcs_mix_derivatives (k_mix_derivatives) and pcs_mix_derivatives_vjp (k_mix_derivatives_vjp, mix_jacobian.hpp::mix_derivatives_vjp)
behind PcSaftMix(parameters, kij).derivatives / helmholtz_energy_density, on the rows of tests/tools/state_rows.py::mix_rows:
mix_batch(700, seed=701) where the oracle's long-double bubble point converges -- 698 rows = ten full 64-lane waves and a 58-lane
tail; 233 without an associating component, 117 with one, 348 with two (233 cross-, 115 induced-associating), 465 polar, 116
with an explicit eps_AiBj, every one with k_ij != 0 -- each at its vapour, its liquid and that liquid compressed by 1.15.

Backward: every one of the 21 columns of every row against oracle.mix_derivatives_vjp_exact (nested duals in long double,
checked on the CPU by tests/test_oracle_state_grad.py).  Error per row and INPUT GROUP (parameters[16], kij[2], T, rho[2]),
relative to the largest exact component of that group in that row; bar max(1e-10, 10 e), e = the referee's own fp64 run against
its long-double run in the same measure (the rule of tests/test_mixn_gpu.py).  From the referee alone: largest e 4.1e-9
(compressed, parameters); rows with a bar above 1e-8: at most 0.29 % of a group and state (5 % allowed).
Measured kernel error: at most 1.8e-12, at most 0.011 of its bar (table in test_backward_vs_exact_gradient).
Sensitivity, tried on scratch builds and not kept: the tangent of (1 - k_ij) in mix_coef_dispersion scaled by 1 + 1e-6 gives
1.0e-6 in the kij group (10^4 bars: red; tests/test_deriv_grad_gpu.py is red too, its 1e-7 sees a 1e-6 error of the k_ij column);
the tangent of the explicit eps_AiBj in mix_coef_assoc scaled by 1 + 1e-6 gives 1.0e-6 in the kij group on the vapour rows, where
that column is the larger of the two (10^4 bars: red) while tests/test_deriv_grad_gpu.py stays green.
Forward: a, p, mu, v against oracle.mix_derivatives_exact at (1e-13, 1e-12, 1e-13, 1e-10) in the measures of
tests/test_mix_gpu.py::test_derivatives_random_rows, plus 10 x the fp64 oracle's (robust=True) error on the same row; at most
10 % of the rows may need that allowance (tests/test_gc_state_gpu.py)."""
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
FWD_TOL = (1e-13, 1e-12, 1e-13, 1e-10)
CUTS = (1, 63, 64, 65, 128, 129)


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


def test_row_set(oracle):
    """What the row set is for: more than four waves with a ragged tail, every class present."""
    m = sr.mix_rows(oracle)
    n, c = m["n"], m["classes"]
    assert n > 4 * 64 and n % 64 != 0, n
    counts = {k: int(v.sum()) for k, v in c.items()}
    print(f"\n{n} rows: {counts}")
    assert all(counts[k] > 0 for k in ("none", "one", "two", "cross", "induced", "polar", "eps_aibj"))
    assert counts["kij"] == n and counts["two"] >= n // 3
    assert int((c["cross"] & c["eps_aibj"]).sum()) == counts["eps_aibj"]


def test_backward_vs_exact_gradient(amd, oracle):
    """Every row, state and column; nothing left out.  Also: the mu column is exactly 0 where mu = 0; the association columns are
    exactly 0 on rows without sites; the eps_AiBj column is exactly 0 unless the row is cross-associating with kij[:, 1] != 0 and
    non-zero there; na, nb columns are non-zero for every component with sites, and -- like kappa_ab and epsilon_k_ab -- for the
    site-less component next to a self-associating one (the formula sums them, pcsaft_mix.py:211-218).

    Measured on an MI355X, kernel error largest (largest err / bar), parameters / kij / T / rho:
      vapour     7.02e-13 (0.007)  4.31e-13 (0.004)  1.76e-12 (0.008)  8.40e-14 (0.001)
      liquid     1.69e-14 (0.000)  1.41e-14 (0.000)  1.15e-12 (0.011)  2.22e-14 (0.000)
      compressed 6.81e-14 (0.001)  2.41e-13 (0.002)  6.63e-14 (0.001)  4.20e-14 (0.000)
    the referee's own e (fp64 against long double), largest: 6.4e-12 / 4.0e-12 / 2.4e-11 / 5.4e-14 (vapour), 5.1e-10 / 7.5e-14 /
    4.1e-9 / 4.0e-10 (liquid), 4.1e-9 / 3.7e-13 / 3.2e-9 / 1.7e-10 (compressed); rows with a bar above 1e-8: 0.29 % at most."""
    from feos_torch_amd import native

    m = sr.mix_rows(oracle)
    n, P, K, c = m["n"], m["P"], m["K"], m["classes"]
    bars = sr.bars(m, sr.MIX_GROUPS)
    for state in sr.STATES:  # the bars hide nothing: from the referee alone, before the kernel is looked at
        for g, (e, bar) in bars[state].items():
            assert np.isfinite(e).all() and np.mean(bar > 1e-8) <= 0.05, (state, g, float(np.mean(bar > 1e-8)))
    Pd, Kd, Td = _dev(P), _dev(K), _dev(m["T"])
    sites = (P[:, :, 6] + P[:, :, 7]) != 0.0
    self_assoc = (P[:, :, 6] * P[:, :, 7]) != 0.0
    beside = ~sites & self_assoc.any(axis=1, keepdims=True) & (sites.sum(axis=1, keepdims=True) == 1)
    eps_used = c["cross"] & c["eps_aibj"]
    print()
    for state in sr.STATES:
        want = m["exact"][state]
        got = _np(native.mix_derivatives_vjp(Pd, Kd, Td, _dev(m["states"][state]), *(_dev(x) for x in m["w"][state])))
        assert got.shape == (n, 21) and np.isfinite(got).all()
        err = sr.group_error(got, want, sr.MIX_GROUPS)
        line = []
        for g, (e, bar) in bars[state].items():
            line.append(f"{g} {err[g].max():.2e} ({np.max(err[g] / bar):.3f}; e {e.max():.2e}, bar > 1e-8: {100 * np.mean(bar > 1e-8):.2f} %)")
        print(f"   {state:10s} " + "  ".join(line))
        for g, (e, bar) in bars[state].items():
            assert (err[g] <= bar).all(), (state, g, int(np.argmax(err[g] / bar)), float(err[g].max()), float(np.max(err[g] / bar)))
        for side in (got, want):
            p8 = side[:, :16].reshape(n, 2, 8)
            assert np.all(p8[:, :, 3][P[:, :, 3] == 0.0] == 0.0)
            assert np.all(p8[:, :, 4:8][c["none"]] == 0.0)
            assert np.all(side[~eps_used, 17] == 0.0) and np.all(side[eps_used, 17] != 0.0)
            assert np.all(p8[:, :, 6:8][sites] != 0.0)
            assert beside.any() and np.all(p8[:, :, 4:8][beside] != 0.0)
            assert np.all(side[:, 16] != 0.0)


def _fwd_errors(a, p, mu, v, A, Pp, MU, V, rho):
    return (np.abs(a - A) / np.maximum(np.abs(A), 1e-6), np.abs(p - Pp) / np.maximum(np.abs(Pp), rho.sum(axis=1)),
            (np.abs(mu - MU) / np.maximum(1.0, np.abs(MU))).max(axis=1), np.abs(v / V - 1.0).max(axis=1))


def test_forward_vs_long_double_oracle(amd, oracle):
    """a, p, mu, v of every row and state through PcSaftMix.derivatives; helmholtz_energy_density is a[:, None] bit for bit.

    Measured on an MI355X, worst (a, p, mu, v) per state, and the fp64 oracle (robust=True) against the same values:
      vapour     7.71e-15 7.77e-16 9.37e-16 8.60e-13   (7.71e-15 2.21e-16 9.52e-16 6.25e-14)
      liquid     1.59e-15 7.71e-14 1.21e-14 6.42e-14   (5.06e-12 1.51e-09 2.98e-10 5.60e-10)
      compressed 2.43e-15 1.23e-14 1.31e-13 4.04e-14   (1.45e-11 1.52e-10 1.21e-09 8.64e-10)
    3 of 698 rows needed the fp64-noise allowance (0.43 %, cap 10 %)."""
    m = sr.mix_rows(oracle)
    n = m["n"]
    eos = amd.PcSaftMix(_dev(m["P"]), _dev(m["K"]))
    T = _dev(m["T"])
    need = np.zeros(n, bool)
    print()
    for state, rho in m["states"].items():
        exact = oracle.mix_derivatives_exact(m["P"], m["K"], m["T"], rho)
        noise = _fwd_errors(*oracle.mix_derivatives(m["P"], m["K"], m["T"], rho, robust=True), *exact, rho)
        a, p, mu, v = eos.derivatives(T, _dev(rho))
        h = eos.helmholtz_energy_density(T, _dev(rho))
        assert h.shape == (n, 1) and torch.equal(_bits(h), _bits(a)[:, None])
        errs = _fwd_errors(_np(a), _np(p), _np(mu), _np(v), *exact, rho)
        print(f"   {state:10s} a {errs[0].max():.2e} p {errs[1].max():.2e} mu {errs[2].max():.2e} v {errs[3].max():.2e}   "
              f"(fp64 oracle: {noise[0].max():.2e} {noise[1].max():.2e} {noise[2].max():.2e} {noise[3].max():.2e})")
        for e, nz, tol, name in zip(errs, noise, FWD_TOL, "a p mu v".split()):
            assert np.isfinite(e).all() and np.all(e <= tol + 10.0 * nz), (state, name, tol, float(e.max()))
            need |= ~(e < tol)
    print(f"   rows that needed the fp64-noise allowance: {need.sum()} of {n} ({100 * need.mean():.2f} %)")
    assert need.mean() <= 0.10


def _vjp_no_workspace(P, K, T, rho, w):
    """pcs_mix_derivatives_vjp with workspace = NULL: rows in batch order, no class order (the wrapper always passes one)"""
    from feos_torch_amd import _lib

    n = T.shape[0]
    grad = torch.empty((n, 21), dtype=f64, device=T.device)
    L = _lib.lib()
    _lib.check(L.pcs_mix_derivatives_vjp(_lib.ptr(P), _lib.ptr(K), _lib.ptr(T), _lib.ptr(rho), n, *(_lib.ptr(x) for x in w), _lib.ptr(grad),
                                         None, _lib.current_stream_ptr(grad.device)), "pcs_mix_derivatives_vjp")
    torch.cuda.synchronize()
    return grad


def test_results_do_not_depend_on_batch_or_schedule(amd, oracle):
    """A row's results do not depend on how many rows follow it or on the order the waves take them in: the first n rows of the
    698-row call have the bits of an n-row call (n = one lane, a wave +- 1, two waves + 1), forward and backward, in every state;
    and pcs_mix_derivatives_vjp without a workspace (batch order, waves of mixed classes: no direction is skipped wave-wide)
    has the bits of the call with one (batch-wide class order) on every row."""
    from feos_torch_amd import native

    m = sr.mix_rows(oracle)
    n = m["n"]
    Pd, Kd, Td = _dev(m["P"]), _dev(m["K"]), _dev(m["T"])
    for state in sr.STATES:
        rd, wd = _dev(m["states"][state]), [_dev(x) for x in m["w"][state]]
        full = [_bits(x) for x in (*native.mix_derivatives(Pd, Kd, Td, rd), native.mix_derivatives_vjp(Pd, Kd, Td, rd, *wd))]
        assert torch.equal(_bits(_vjp_no_workspace(Pd, Kd, Td, rd, wd)), full[4]), state
        for k in (*CUTS, n):
            part = (*native.mix_derivatives(Pd[:k], Kd[:k], Td[:k], rd[:k]),
                    native.mix_derivatives_vjp(Pd[:k], Kd[:k], Td[:k], rd[:k], *(x[:k] for x in wd)))
            for name, f, q in zip(("a", "p", "mu", "v", "grad"), full, part):
                assert q.shape[0] == k and torch.equal(_bits(q), f[:k]), (state, k, name)
            assert torch.equal(_bits(_vjp_no_workspace(Pd[:k], Kd[:k], Td[:k], rd[:k], [x[:k].contiguous() for x in wd])), full[4][:k]), (state, k)


LINEAR_ROWS = 130  # two waves and a two-lane tail; the kept rows keep mix_batch's class cycle, so every class is there ~ 21 times


def _linear_case(oracle):
    """Rows, states and the seed of the upstream weights of test_optional_upstreams: the first 130 rows, row i in state i % 3.
    The seed is the first from 7100 on for which the fp64 REFEREE is linear to 1e-14 on every row (a gas row whose two g_v nearly
    cancel loses its largest components, the -g_v / rho^2 density entries: tests/test_mixn_gpu.py::test_vjp_optional_upstreams)."""
    m = sr.mix_rows(oracle)
    n = LINEAR_ROWS
    P, K, T = m["P"][:n], m["K"][:n], m["T"][:n]
    rho = np.stack([m["states"][sr.STATES[i % 3]][i] for i in range(n)])
    for seed in range(7100, 7200):
        rng = np.random.default_rng(seed)
        w = [rng.normal(size=n), rng.normal(size=n), rng.normal(size=(n, 2)), rng.normal(size=(n, 2)) * 1e-3]
        z = [np.zeros_like(x) for x in w]
        single = [oracle.mix_derivatives_vjp_exact(P, K, T, rho, *(w[j] if j == k else z[j] for j in range(4)), prec=0) for k in range(4)]
        total = oracle.mix_derivatives_vjp_exact(P, K, T, rho, *w, prec=0)
        ref_err = np.abs(total - sum(single)).max(axis=1) / np.abs(total).max(axis=1)
        if ref_err.max() < 1e-14:
            return P, K, T, rho, w, seed, float(ref_err.max())
    raise AssertionError("no seed with a linear fp64 referee")


def test_optional_upstreams(amd, oracle):
    """g_* = None is an explicit zero (bits) for every subset, all None gives zeros, and the gradient is linear in the upstreams:
    all four together equal the sum of the four single-upstream gradients to 1e-13 of the row's largest component.
    Measured: seed 7100 (the first tried), fp64 referee linear to 1.3e-15, kernel to 1.5e-15."""
    from feos_torch_amd import native

    P, K, T, rho, w, seed, ref_err = _linear_case(oracle)
    assert ref_err < 1e-14
    Pd, Kd, Td, rd = _dev(P), _dev(K), _dev(T), _dev(rho)
    w = [_dev(x) for x in w]
    single = []
    for keep in itertools.product((False, True), repeat=4):
        with_none = native.mix_derivatives_vjp(Pd, Kd, Td, rd, *(x if k else None for x, k in zip(w, keep)))
        with_zero = native.mix_derivatives_vjp(Pd, Kd, Td, rd, *(x if k else torch.zeros_like(x) for x, k in zip(w, keep)))
        assert torch.equal(_bits(with_none), _bits(with_zero)), keep
        if sum(keep) == 1:
            single.append(_np(with_none))
    assert len(single) == 4
    assert np.all(_np(native.mix_derivatives_vjp(Pd, Kd, Td, rd)) == 0.0)
    total = _np(native.mix_derivatives_vjp(Pd, Kd, Td, rd, *w))
    err = np.abs(total - sum(single)).max(axis=1) / np.abs(total).max(axis=1)
    print(f"\n   seed {seed}: fp64 referee linear to {ref_err:.2e}, kernel to {err.max():.2e} (row {err.argmax()})")
    assert err.max() < 1e-13


def test_shell_backward_equals_the_abi(amd, oracle):
    """PcSaftMix(P, kij).derivatives(T, rho) and backward of the weighted sum: P.grad, kij.grad (both columns), T.grad and rho.grad
    carry the bits of the matching columns of native.mix_derivatives_vjp; backward of helmholtz_energy_density is the g_a-only
    call."""
    from feos_torch_amd import PcSaftMix, native

    m = sr.mix_rows(oracle)
    n = m["n"]
    for state in ("vapour", "compressed"):
        Pt, Kt, Tt, rt = (_dev(x).requires_grad_(True) for x in (m["P"], m["K"], m["T"], m["states"][state]))
        wd = [_dev(x) for x in m["w"][state]]
        out = PcSaftMix(Pt, Kt).derivatives(Tt, rt)
        assert [tuple(o.shape) for o in out] == [(n,), (n,), (n, 2), (n, 2)]
        sum((o * x).sum() for o, x in zip(out, wd)).backward()
        g = native.mix_derivatives_vjp(Pt.detach(), Kt.detach(), Tt.detach(), rt.detach(), *wd)
        assert Pt.grad.shape == (n, 2, 8) and torch.equal(_bits(Pt.grad).reshape(n, 16), _bits(g[:, :16]))
        assert Kt.grad.shape == (n, 2) and torch.equal(_bits(Kt.grad), _bits(g[:, 16:18]))
        assert Tt.grad.shape == (n,) and torch.equal(_bits(Tt.grad), _bits(g[:, 18]))
        assert rt.grad.shape == (n, 2) and torch.equal(_bits(rt.grad), _bits(g[:, 19:21]))
        Pt, Kt, Tt, rt = (_dev(x).requires_grad_(True) for x in (m["P"], m["K"], m["T"], m["states"][state]))
        h = PcSaftMix(Pt, Kt).helmholtz_energy_density(Tt, rt)
        (h[:, 0] * wd[0]).sum().backward()
        g = native.mix_derivatives_vjp(Pt.detach(), Kt.detach(), Tt.detach(), rt.detach(), wd[0])
        for got, cols in ((Pt.grad.reshape(n, 16), slice(0, 16)), (Kt.grad, slice(16, 18)), (Tt.grad[:, None], slice(18, 19)), (rt.grad, slice(19, 21))):
            assert torch.equal(_bits(got), _bits(g[:, cols])), (state, cols)
