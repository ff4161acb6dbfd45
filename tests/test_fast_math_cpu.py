"""CPU: the two fp64 refinements of the pure-component unit (csrc/dual.hpp) restated on the host, and the rows of the GPU test.

  * tests/tools/fast_math_check.cpp restates the third-order reciprocal step (PCS_FAST_RCP == 1) and the coupled square-root
    refinement (PCS_FAST_SQRT) with std::fma and feeds them seeds with an injected relative error up to 2^-22 of both signs
    and its two extreme values (the hardware estimates do not exist on the host; the ISA text bounds them by 2^-23 at the
    loosest): 1e6 arguments log-uniform in 1e-300 ... 1e300 and 1e5 next to the powers of two in [1, 2].  Every reciprocal
    must be within 1 ulp of the long-double quotient and every square root within 2 ulp of the long-double root; 0,
    subnormal, infinite, NaN (and, for the root, negative) arguments must not come out finite.  Built with the host compiler
    and run twice: plainly, and once under AddressSanitizer + UBSan as a stand-alone binary.
  * the 2,048 rows of tests/test_pure_fast_math_gpu.py (tests/tools/fast_math_rows.py): 512 of each class, T / T_c over
    0.45 ... 0.95, half of the associating rows strongly associating, and EVERY row with a saturation state and a liquid at
    2 p_sat by the oracle alone, so the GPU test leaves no row out by construction.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "tools"))
import fast_math_rows as fr  # noqa: E402

SRC = os.path.join(HERE, "tools", "fast_math_check.cpp")
N_LOG, N_POW2 = 1_000_000, 100_000


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "asan-ubsan"])
def test_refinements_hold_their_ulp_bounds(tmp_path, flags):
    exe = str(tmp_path / "fast_math_check")
    subprocess.check_call(["g++", "-std=c++17"] + flags + ["-o", exe, SRC])
    r = subprocess.run([exe, str(N_LOG), str(N_POW2)], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    out = dict(re.findall(r"^(\w+) (.*)$", r.stdout, flags=re.M))
    assert int(re.search(r"^arguments (\d+)", r.stdout, flags=re.M).group(1)) == N_LOG + N_POW2  # no case left out
    assert int(re.search(r"cases (\d+)", r.stdout).group(1)) == 3 * (N_LOG + N_POW2)
    rcp = re.match(r"max_ulp (\S+) at \S+ over_1ulp (\d+)", out["recip"])
    sq = re.match(r"max_ulp (\S+) at \S+ over_2ulp (\d+)", out["sqrt"])
    assert float(rcp.group(1)) <= 1.0 and int(rcp.group(2)) == 0, out["recip"]
    assert float(sq.group(1)) <= 2.0 and int(sq.group(2)) == 0, out["sqrt"]
    assert out["special"] == "finite 0", out["special"]
    assert r.returncode == 0, r.stderr


def test_every_row_of_the_gpu_test_has_a_saturation_state(oracle):
    P, T, theta, cls, strong = fr.rows(oracle)
    assert P.shape == (fr.N, 8) and fr.N == 2048 and fr.PARTIAL == 2048 - 37
    assert np.bincount(cls, minlength=4).tolist() == [512] * 4
    assert np.array_equal(cls, fr.sg.classes(P))
    assert theta.min() >= 0.45 and theta.max() <= 0.95
    for k in range(4):  # every class covers the range: each tenth of it holds rows of the class
        assert (np.histogram(theta[cls == k], bins=10, range=(0.45, 0.95))[0] > 0).all()
    p, st_p = oracle.pure_vapor_pressure(P, T, prec=1)
    rho_v, rho_l, st_v, _, _ = oracle.pure_vle(P, T, prec=1)
    _, st_l = oracle.pure_liquid_density(P, T, 2.0 * p, prec=1)
    print("oracle failures: p_sat %d, vle %d, liquid at 2 p_sat %d of %d rows" % (st_p.sum(), st_v.sum(), st_l.sum(), fr.N))
    assert not st_p.any() and not st_v.any() and not st_l.any()
    assert np.isfinite(p).all() and (p > 0).all() and (rho_v < rho_l).all()
    s = fr.strength(P, T, rho_l)
    for k in (2, 3):
        m = cls == k
        print("class %d: 4 rho Delta of the strong half min %.3g median %.3g max %.3g, of the other half median %.3g"
              % (k, s[m & strong].min(), np.median(s[m & strong]), s[m & strong].max(), np.median(s[m & ~strong])))
        assert (m & strong).sum() == 256 and (s[m & strong] >= fr.STRONG).all()
    assert not strong[cls < 2].any()
    # both conjugate branches of the site fractions occur (|t| > 0.5 with n_a != n_b) next to the plain form
    uneven = (cls >= 2) & (P[:, 6] != P[:, 7]) & (s > 2.0)
    assert (uneven & (P[:, 6] < P[:, 7])).sum() >= 50 and (uneven & (P[:, 6] > P[:, 7])).sum() >= 50
