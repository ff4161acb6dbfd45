"""The dilute-limit grid shared by tests/test_oracle_dilute.py (CPU) and tests/test_dilute_gpu.py (GPU)."""
import numpy as np

# a trace amount of component 1 (small z) or of component 2 (z near 1); powers of two near 1 so that 1 - z is exact
DILUTE_Z = (2.0**-46, 2.0**-30, 2.0**-20, 1e-4, 1.0 - 2.0**-20, 1.0 - 2.0**-40)
KT_A3 = 1.380649e-23 * 1e30  # p [Pa] = reduced p [A^-3] * KT_A3 * T [K]


def grid(n, zs):
    """Row index and z of every (row, z) pair, row-major: reshape results to [n, len(zs)]."""
    return np.repeat(np.arange(n), len(zs)), np.tile(np.asarray(zs, dtype=np.float64), n)


def henry_error(p_tiny, p_lo, p_hi, d_tiny, d_lo, d_hi, p_sat):
    """Pure-component limit in the Henry-linear form p(d) = p_sat + s d (d = mole fraction of the trace component), with s the
    chord through the two larger d (d_lo < d_hi), checked at d_tiny <= d_lo.  -> (|p(d_tiny) - p_sat - s d_tiny| / p_sat,
    judged).  A row is judged where p stays within 1e-4 of p_sat up to d_hi: the curvature then moves the check by at most
    ~1e-4 d_lo / d_hi <= 1e-10.  Rows with a large Henry slope (p / p_sat up to 1e5 at d = 1e-12) or a dew point whose 1 / p
    (not p) is linear in d are physical, but not linear in p at these d."""
    s = (p_hi - p_lo) / (d_hi - d_lo)
    dev = np.maximum(np.abs(p_tiny / p_sat - 1.0), np.abs(p_hi / p_sat - 1.0))
    return np.abs(p_tiny - (p_sat + s * d_tiny)) / p_sat, dev <= 1e-4


def trace_index(z):
    """Index of the trace component: 0 where z < 1/2, else 1."""
    return (np.asarray(z) > 0.5).astype(np.int64)


def trace_fraction_error(rho, z):
    """Relative error of the trace component's mole fraction in a phase of partial densities rho [n,2] against z [n]."""
    tr = trace_index(z)
    frac = rho[np.arange(len(rho)), tr] / rho.sum(axis=1)
    return np.abs(frac / np.where(tr == 1, 1.0 - z, z) - 1.0)
