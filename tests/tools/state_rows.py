"""Row sets of tests/test_oracle_state_grad.py, tests/test_mix_state_gpu.py and tests/test_pure_state_gpu.py: binary and
pure-component state points with seeded upstream weights and the oracle's exact gradients, computed once per session and never
modified (every array is read-only).

States per row, as tests/test_gc_state_gpu.py: the vapour and the liquid of the oracle's long-double equilibrium at the row's
temperature, and that liquid compressed by 1.15.  Upstream weights ga, gp, gmu ~ N(0,1), gv ~ 1e-3 N(0,1) (v ~ 1 / rho is
large in the vapour), pure gdp ~ N(0,1).

Error measure of the gradients ("same row and input", tests/test_deriv_grad_gpu.py): per row and per input GROUP, the largest
|difference| of the group's columns over the largest |exact| component of the group.  A single row-wide scale would let the
-gv / rho^2 density entries of the gas rows hide the parameter columns."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
STATES = ("vapour", "liquid", "compressed")
MIX_GROUPS = {"parameters": slice(0, 16), "kij": slice(16, 18), "T": slice(18, 19), "rho": slice(19, 21)}
PURE_GROUPS = {"parameters": slice(0, 8), "T": slice(8, 9), "rho": slice(9, 10)}
FLOOR = 1e-10  # of the bar max(FLOOR, 10 e): tests/test_mixn_gpu.py
_cache = {}


def _freeze(x):
    if isinstance(x, np.ndarray):
        x.setflags(write=False)
    elif isinstance(x, dict):
        for v in x.values():
            _freeze(v)
    elif isinstance(x, (tuple, list)):
        for v in x:
            _freeze(v)
    return x


def group_error(got, want, groups):
    """{group: [n]} largest |got - want| over the group's columns / largest |want| of the group in that row (0 / 0 = 0: a
    group that is exactly zero on both sides agrees)."""
    out = {}
    for name, sl in groups.items():
        num = np.abs(got[:, sl] - want[:, sl]).max(axis=1)
        den = np.abs(want[:, sl]).max(axis=1)
        out[name] = np.where(den == 0.0, np.where(num == 0.0, 0.0, np.inf), num / np.where(den == 0.0, 1.0, den))
    return out


def pure_block():
    """BLOCK of k_pure_derivatives_vjp, read from the sources (pure_kernels.hip names pure_stage.hpp's STAGE_BLOCK)."""
    csrc = os.path.join(ROOT, "feos_torch_amd", "csrc")
    val = re.search(r"constexpr int BLOCK = (\w+);", open(os.path.join(csrc, "pure_kernels.hip")).read()).group(1)
    if not val.isdigit():
        val = re.search(rf"constexpr int {val} = (\d+);", open(os.path.join(csrc, "pure_stage.hpp")).read()).group(1)
    return int(val)


def mix_classes(P, K):
    """Boolean row masks of a binary batch: none / one / two associating components, cross (both self-associating), induced,
    polar, explicit eps_AiBj."""
    sites = (P[:, :, 6] + P[:, :, 7]) != 0.0
    self_assoc = (P[:, :, 6] * P[:, :, 7]) != 0.0
    n_assoc, n_self = sites.sum(axis=1), self_assoc.sum(axis=1)
    return {"none": n_assoc == 0, "one": n_assoc == 1, "two": n_assoc == 2, "cross": (n_assoc == 2) & (n_self == 2),
            "induced": (n_assoc == 2) & (n_self == 1), "self": (n_assoc == 1) & (n_self == 1),
            "polar": (P[:, :, 3] != 0.0).any(axis=1), "eps_aibj": K[:, 1] != 0.0, "kij": K[:, 0] != 0.0}


def mix_rows(oracle):
    """mix_batch(700, seed=701) rows on which the oracle's long-double bubble point converges: dict(P [n,2,8], K [n,2], T [n],
    states {name: rho [n,2]}, w {name: (ga, gp, gmu, gv)}, exact / fp64 {name: grad [n,21]} (prec = 1 / 0), classes)."""
    if "mix" not in _cache:
        from feos_torch_amd.synthetic import mix_batch

        P, K, T, X, PI = mix_batch(700, seed=701)
        _, rho4, st = oracle.mix_bubble_dew(P, K, T, X, PI, False, prec=1)
        keep = np.nonzero(~st)[0]
        P, K, T = (np.ascontiguousarray(x[keep]) for x in (P, K, T))
        n = len(keep)
        liq = np.ascontiguousarray(rho4[keep, 2:4])
        states = {"vapour": np.ascontiguousarray(rho4[keep, 0:2]), "liquid": liq, "compressed": 1.15 * liq}
        w, exact, fp64 = {}, {}, {}
        for k, (name, rho) in enumerate(states.items()):
            rng = np.random.default_rng(7010 + k)
            w[name] = (rng.normal(size=n), rng.normal(size=n), rng.normal(size=(n, 2)), 1e-3 * rng.normal(size=(n, 2)))
            exact[name] = oracle.mix_derivatives_vjp_exact(P, K, T, rho, *w[name], prec=1)
            fp64[name] = oracle.mix_derivatives_vjp_exact(P, K, T, rho, *w[name], prec=0)
        _cache["mix"] = _freeze({"P": P, "K": K, "T": T, "n": n, "states": states, "w": w, "exact": exact, "fp64": fp64,
                                 "classes": mix_classes(P, K)})
    return _cache["mix"]


def pure_rows(oracle):
    """pure_batch(700, seed=5) rows solved by pure_vle(prec=1): dict(P [n,8], T [n], states {name: rho [n]},
    w {name: (ga, gp, gdp)}, exact / fp64 {name: grad [n,10]} (prec = 1 / 0), dropped)."""
    if "pure" not in _cache:
        from feos_torch_amd.synthetic import pure_batch

        P, T = pure_batch(700, seed=5)
        rv, rl, st, _, _ = oracle.pure_vle(P, T, prec=1)
        keep = np.nonzero(~st)[0]
        P, T = np.ascontiguousarray(P[keep]), np.ascontiguousarray(T[keep])
        n = len(keep)
        liq = np.ascontiguousarray(rl[keep])
        states = {"vapour": np.ascontiguousarray(rv[keep]), "liquid": liq, "compressed": 1.15 * liq}
        w, exact, fp64 = {}, {}, {}
        for k, (name, rho) in enumerate(states.items()):
            rng = np.random.default_rng(50 + k)
            w[name] = (rng.normal(size=n), rng.normal(size=n), rng.normal(size=n))
            exact[name] = oracle.pure_derivatives_vjp_exact(P, T, rho, *w[name], prec=1)
            fp64[name] = oracle.pure_derivatives_vjp_exact(P, T, rho, *w[name], prec=0)
        _cache["pure"] = _freeze({"P": P, "T": T, "n": n, "dropped": int(st.sum()), "states": states, "w": w, "exact": exact,
                                  "fp64": fp64})
    return _cache["pure"]


def bars(rows, groups):
    """{state: {group: (e [n], bar [n])}}: e = the fp64 referee against the long-double one in the group measure,
    bar = max(FLOOR, 10 e) -- from the referee alone."""
    out = {}
    for name in rows["states"]:
        e = group_error(rows["fp64"][name], rows["exact"][name], groups)
        out[name] = {g: (e[g], np.maximum(FLOOR, 10.0 * e[g])) for g in groups}
    return out
