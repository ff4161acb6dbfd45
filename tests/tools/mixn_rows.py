"""Random n-component state points shared by tests/test_mixn_gpu.py and tests/test_oracle_mixn.py: parameters [n, nc, 8], T [n],
partial densities [n, nc].  About 40 % of the components are polar; with assoc=True every third row has exactly one associating
component (2B, 3B with either site in excess); half of the rows are liquid-like (packing fraction 0.2 ... 0.42), half gas-like
(1e-7 ... 1e-2).  The draws are pinned by the seed: tests quote measured figures for them."""
import numpy as np


def random_rows(n, nc, seed, assoc=True):
    rng = np.random.default_rng(seed)
    P = np.zeros((n, nc, 8))
    P[:, :, 0] = rng.uniform(1.0, 3.5, (n, nc))
    P[:, :, 1] = rng.uniform(2.8, 4.2, (n, nc))
    P[:, :, 2] = rng.uniform(150.0, 350.0, (n, nc))
    P[:, :, 3] = np.where(rng.random((n, nc)) < 0.4, rng.uniform(0.5, 3.0, (n, nc)), 0.0)
    if assoc:
        for r in range(0, n, 3):
            c = rng.integers(0, nc)
            P[r, c, 4:8] = [rng.uniform(0.001, 0.05), rng.uniform(1000.0, 3000.0), *[(1, 1), (2, 1), (1, 2)][rng.integers(0, 3)]]
    T = rng.uniform(200.0, 450.0, n)
    d = P[:, :, 1] * (1 - 0.12 * np.exp(-3 * P[:, :, 2] / T[:, None]))
    x = rng.dirichlet(np.ones(nc), n)
    eta = np.where(rng.random(n) < 0.5, rng.uniform(0.2, 0.42, n), 10.0 ** rng.uniform(-7, -2, n))
    rho = x * (eta / (np.pi / 6 * (x * P[:, :, 0] * d**3).sum(axis=1)))[:, None]
    return P, T, rho
