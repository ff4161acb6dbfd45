"""The rows of tests/test_pure_fast_math_gpu.py (and the CPU check of them in tests/test_fast_math_cpu.py): 2,048 rows, 512
of each of the four classes, each at its own T / T_c in 0.45 ... 0.95.

Parameter rows and critical temperatures are those of tests/tools/saturation_grid.py (800 rows of all four classes, T_c from
critical_referee.oracle_scan: independent of every VLE solver, and cached, so one session scans once).  Every class takes
its parameter rows cyclically and a seeded permutation of 512 evenly spaced reduced temperatures, so a class covers the whole
temperature range and a parameter row appears at two or three temperatures.  The classes alternate row by row: bucketed
waves of every class occur in each of the 8 workgroups.

Strong association.  The square root under test has the argument aux^2 + 4 rho Delta (csrc/pure_model.hpp); where 4 rho
Delta is large against 1 the site fractions are taken in the conjugate forms, whose numerator sq - aux cancels, so an error
of sq is amplified.  Half of the rows of each associating class are therefore taken from the (parameter row, temperature)
pairs with the LARGEST association strength: the class's parameter rows ranked by S = kappa_ab (exp(eps_ab / T) - 1) / m at
T / T_c = 0.45 (4 rho Delta = 4 n_b rho sigma^3 kappa_ab (exp(eps_ab/T) - 1) h(eta), and rho sigma^3 ~ 1/m on the liquid
side), the upper eighth of them placed on the LOWER half of the temperatures.  `strength` gives 4 n_b rho_L Delta of a row at
a liquid density, for the CPU test to check what was picked.  Nothing here touches the GPU.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import saturation_grid as sg  # noqa: E402

N, PER_CLASS, SEED = 2048, 512, 707
THETA_LO, THETA_HI = 0.45, 0.95
PARTIAL = N - 37  # a batch whose last workgroup is partial
STRONG = 40.0     # 4 n_b rho_L Delta from which a row is called strongly associating: site fraction 2 / (1 + sqrt 41) < 0.28


def rows(orc=None):
    """-> P [N, 8], T [N], theta [N], class [N], strong-slot mask [N] (the rows placed as strongly associating)."""
    g = sg.grid(orc=orc)
    P0, Tc = g.P[:sg.N_ROWS], g.Tc[:sg.N_ROWS]
    cls0 = sg.classes(P0)
    rng = np.random.default_rng(SEED)
    line = THETA_LO + (THETA_HI - THETA_LO) * (np.arange(PER_CLASS) + 0.5) / PER_CLASS
    P = np.empty((N, 8))
    T, theta, cls, strong = np.empty(N), np.empty(N), np.empty(N, dtype=np.int64), np.zeros(N, dtype=bool)
    for k in range(4):
        idx = np.flatnonzero(cls0 == k)
        th = rng.permutation(line)
        pick = idx[np.arange(PER_CLASS) % len(idx)]
        s = np.zeros(PER_CLASS, dtype=bool)
        if k >= 2:
            S = P0[idx, 4] * np.expm1(P0[idx, 5] / (THETA_LO * Tc[idx])) / P0[idx, 0]
            top = idx[np.argsort(S)[::-1][:max(1, len(idx) // 8)]]
            half = PER_CLASS // 2
            th = np.concatenate([rng.permutation(line[:half]), rng.permutation(line[half:])])
            pick[:half] = top[np.arange(half) % len(top)]
            s[:half] = True
        # every row must have a saturation state the long-double oracle finds (a strongly polar row can have none it
        # solves at a temperature between two it does): such a slot takes the class's next parameter row
        orc = orc or sg._oracle()
        pool = top if k >= 2 else idx
        for _ in range(8):
            bad = orc.pure_vapor_pressure(P0[pick], th * Tc[pick], prec=1)[1] | orc.pure_vle(P0[pick], th * Tc[pick], prec=1)[2]
            if not bad.any():
                break
            for j in np.flatnonzero(bad):
                src = pool if s[j] else idx
                pick[j] = src[(int(np.flatnonzero(src == pick[j])[0]) + 1) % len(src)]
        sl = slice(k, N, 4)  # classes alternate row by row
        P[sl], T[sl], theta[sl], cls[sl], strong[sl] = P0[pick], th * Tc[pick], th, k, s
    return np.ascontiguousarray(P), T, theta, cls, strong


def strength(P, T, rho):
    """4 n_b rho Delta at density rho [A^-3] (csrc/pure_model.hpp: Delta = da h(eta), da = sigma^3 kappa_ab (exp(eps_ab/T) - 1))."""
    d = P[:, 1] * (1.0 - 0.12 * np.exp(-3.0 * P[:, 2] / T))
    eta = np.pi / 6.0 * P[:, 0] * d ** 3 * rho
    u = 1.0 / (1.0 - eta)
    h = u * (1.0 + eta * u * (1.5 + 0.5 * eta * u))
    return 4.0 * np.maximum(P[:, 6], P[:, 7]) * rho * P[:, 1] ** 3 * P[:, 4] * np.expm1(P[:, 5] / T) * h
