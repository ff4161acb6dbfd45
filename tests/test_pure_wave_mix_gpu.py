"""A row's vapour pressure does not depend on the rows it shares a wave with, and the corner cases of the association flag.

The kernels bucket the rows of a workgroup by model class and skip the dipole and association blocks per lane, and a wave
leaves its loops on a ballot; none of that may leak from one row into another.  The pressure-only kernel solves the same
rows in batch order, under seeded permutations that put different classes (none, polar, associating, both) side by side,
and with row counts that are no multiple of the 256-row workgroup; p_sat and status must be bit-identical row for row (this
is what a wave-uniform shortcut in the coefficient set, such as skipping the association prefactor for a whole wave, has to
pass).  Rows with sites but kappa_ab = 0 or epsilon_k_ab = 0, and rows with kappa_ab != 0 but no sites,
are compared with the long-double oracle at the 1e-10 of tests/test_large_parity_gpu.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N = 200_000  # >= 1e5 rows of pure_batch
TOL = 1e-10


@pytest.fixture(scope="module")
def amd():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    import feos_torch_amd

    return feos_torch_amd


def _d(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _solve(P, T):
    from feos_torch_amd import native

    r = native.pure_vle(_d(P), _d(T), want_rho_vl=False)  # the pressure-only kernel + fallback + robust pass
    return r["p_sat"].cpu().numpy(), r["status"].cpu().numpy().astype(bool)


def _same_bits(p, st, p_ref, st_ref, what):
    assert np.array_equal(st, st_ref), f"{what}: status differs on {(st != st_ref).sum()} rows"
    ok = ~st_ref
    diff = p[ok].view(np.uint64) != p_ref[ok].view(np.uint64)
    assert not diff.any(), f"{what}: p_sat differs in its bits on {diff.sum()} rows, first {np.nonzero(ok)[0][diff][:8].tolist()}"


def _class_of(P):
    polar = P[:, 3] != 0.0
    assoc = (P[:, 6] != 0.0) | (P[:, 7] != 0.0)
    return polar.astype(int) + 2 * assoc.astype(int)


def test_result_independent_of_wave_mates(amd):
    from feos_torch_amd.synthetic import pure_batch

    P, T = pure_batch(N, seed=4242)
    cls = _class_of(P)
    assert all((cls == k).sum() > N // 8 for k in range(4))  # the four classes are all there
    p0, st0 = _solve(P, T)
    assert st0.mean() < 0.01
    rng = np.random.default_rng(4243)
    # 1. a random permutation: every wave gets another mix of classes and another set of neighbours
    # 2. sorted by class: pure waves (except at the three class boundaries), the other extreme
    # 3. round-robin over the classes: all four in every wave, even after the bucketing inside the workgroup
    by_class = np.argsort(cls, kind="stable")
    lanes = np.concatenate([np.arange((cls == k).sum()) * 4 + k for k in range(4)])  # position of the j-th row of class k
    round_robin = by_class[np.argsort(lanes, kind="stable")]
    for what, perm in (("random permutation", rng.permutation(N)), ("sorted by class", by_class), ("round robin", round_robin)):
        assert sorted(perm.tolist()) == list(range(N))
        p, st = _solve(P[perm], T[perm])
        _same_bits(p, st, p0[perm], st0[perm], what)
    # row counts that are no multiple of the workgroup (256) or the wave (64): the last workgroup is partly filled
    for n in (N - 1, N - 191, 100_003):
        p, st = _solve(P[:n], T[:n])
        _same_bits(p, st, p0[:n], st0[:n], f"first {n} rows")
    # a single associating row in a workgroup of site-free rows, and the reverse
    free, sites = np.nonzero(cls < 2)[0], np.nonzero(cls >= 2)[0]
    for what, many, one in (("one associating row among site-free rows", free, sites), ("one site-free row among associating rows", sites, free)):
        idx = many[:1000].copy()
        idx[::97] = one[: len(idx[::97])]
        p, st = _solve(P[idx], T[idx])
        _same_bits(p, st, p0[idx], st0[idx], what)


def test_association_flag_corner_cases(amd, oracle):
    """Sites without association strength (kappa_ab = 0 or epsilon_k_ab = 0) and association parameters without sites."""
    from feos_torch_amd.synthetic import pure_batch

    n = 40_000
    P, T = pure_batch(n, seed=4244)
    sites = (P[:, 6] != 0.0) | (P[:, 7] != 0.0)
    P = P.copy()
    k = np.arange(n) % 4
    P[sites & (k == 0), 4] = 0.0                    # sites, kappa_ab = 0: da = 0, no association
    P[sites & (k == 1), 5] = 0.0                    # sites, epsilon_k_ab = 0: exp(0) - 1 = 0, no association
    P[sites & (k == 2), 6:8] = 0.0                  # kappa_ab, epsilon_k_ab != 0 but na = nb = 0
    both0 = sites & (k == 3) & (np.arange(n) % 8 == 3)
    P[both0, 4] = 0.0                               # sites, kappa_ab = epsilon_k_ab = 0
    P[both0, 5] = 0.0
    cases = {"kappa_ab = 0": sites & (k == 0), "epsilon_k_ab = 0": sites & (k == 1), "na = nb = 0": sites & (k == 2),
             "kappa_ab = epsilon_k_ab = 0": both0, "untouched": ~sites | ((k == 3) & ~both0)}
    got, st_g = _solve(P, T)
    want, st_o = oracle.pure_vapor_pressure(P, T, prec=1)
    assert st_g.sum() <= st_o.sum()
    for what, sel in cases.items():
        assert sel.sum() > 1000, what
        both = sel & ~st_g & ~st_o
        rel = np.abs(got[both] - want[both]) / np.abs(want[both])
        print(f"{what}: rows {sel.sum()} both converged {both.sum()} max rel {rel.max():.3e}")
        assert both.sum() > 0.99 * sel.sum(), what
        assert rel.max() <= TOL, f"{what}: max rel {rel.max():.3e}"
    # the three ways of switching association off give the row the pressure of the same row without any association parameters
    Q = P.copy()
    off = cases["kappa_ab = 0"] | cases["epsilon_k_ab = 0"] | cases["na = nb = 0"] | both0
    Q[off, 4:8] = 0.0
    got_q, st_q = _solve(Q, T)
    _same_bits(got, st_g, got_q, st_q, "association switched off vs no association parameters")
