"""GPU: every pure-VLE entry point reaches the stage-1 kernel its output set asks for (vle_main_kernel, csrc/pure_kernels.hip),
followed by the fallback and the robust pass.

What is asserted are the bit relations between the entry points, on one batch:
  (a) p_sat and status are the same from pcs_pure_vle (pressure only), pcs_pure_vapor_pressure without and with densities, and
      pcs_pure_row_order + pcs_pure_vle_fast_ordered + pcs_pure_vle_retry: k_pure_vle<true, false>, k_pure_vle_rho and
      k_pure_vle_ordered run one solve;
  (b) pcs_pure_vle_fast + pcs_pure_vle_retry give every output of pcs_pure_vle, for pressure only, rho_eq and rho_vl: the
      staged entries choose the kernel as the whole call does;
  (c) pcs_pure_vle with rho_vl gives every output of pcs_pure_vle_fp64 with rho_vl: both launch k_pure_vle<false>.

The batch: n = 2 * 256 + 37 rows (three workgroups, the last one partial), the four model classes interleaved, and two bands
with T_c from pcs_pure_critical_point, so that the all-fp64 fallback and the robust pass both have rows (without them a wrong
argument of those two launches would go unseen):
  * 160 rows across the first workgroup boundary at T / T_c = 0.97 ... 1.02: all of them reach the robust pass;
  * 64 rows in the last workgroups at T / T_c = 0.82 ... 0.92 whose associating rows are short chains with strong association
    (kappa_ab 0.04 ... 0.05, epsilon_k_ab 2500 ... 3000 K): rows k_pure_vle_fallback solves.  The band at 0.97 ... 1.02 alone
    leaves that list empty: on 400,000 interleaved rows at T / T_c = 0.80 ... 1.02 the fallback kernel solved rows at 0.80 ...
    0.955 only (0.5 % of them, strongly associating ones first), above that the all-fp64 fast path gives up as well.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_pure_row_order_gpu as row_order  # noqa: E402

pytestmark = pytest.mark.gpu

N = 2 * 256 + 37
BAND = slice(176, 336)  # 160 rows, 80 on either side of the first workgroup boundary
STRONG = slice(470, 534)  # 64 rows across the second boundary
SEED = 4100
SETS = {"pressure": (), "rho_eq": ("rho_eq",), "rho_vl": ("rho_vl",)}


def band_batch(seed=SEED):
    """-> (P [N, 8], T [N]) on the GPU"""
    from feos_torch_amd import native

    P, T = row_order.interleaved_batch(N, seed)
    rng = np.random.default_rng(seed)
    n_band, n_strong = BAND.stop - BAND.start, STRONG.stop - STRONG.start
    assoc = P[STRONG, 4] != 0.0
    P[STRONG, 0] = np.where(assoc, rng.uniform(1.0, 1.6, n_strong), P[STRONG, 0])
    P[STRONG, 4] = np.where(assoc, rng.uniform(0.04, 0.05, n_strong), 0.0)
    P[STRONG, 5] = np.where(assoc, rng.uniform(2500.0, 3000.0, n_strong), 0.0)
    Pd = torch.from_numpy(P).cuda()
    cp = native.pure_critical_point(Pd)
    assert not cp["status"].any().item()
    t_c = cp["t_c"].cpu().numpy()
    T[BAND] = t_c[BAND] * np.linspace(0.97, 1.02, n_band)[rng.permutation(n_band)]
    T[STRONG] = t_c[STRONG] * rng.uniform(0.82, 0.92, n_strong)
    return Pd, torch.from_numpy(np.ascontiguousarray(T)).cuda()


def solve(Pd, Td, entries, outputs=()):
    """The entry points `entries` in sequence on one set of pre-filled outputs -> {name: bits as a numpy array}"""
    from feos_torch_amd import native

    dev = Pd.device
    out = {"p_sat": torch.full((N,), float("nan"), dtype=torch.float64, device=dev),
           "rho_eq": torch.full((N,), float("nan"), dtype=torch.float64, device=dev) if "rho_eq" in outputs else None,
           "rho_vl": torch.full((N, 2), float("nan"), dtype=torch.float64, device=dev) if "rho_vl" in outputs else None,
           "status": torch.full((N,), 7, dtype=torch.uint8, device=dev),
           "iters": torch.full((N,), -7, dtype=torch.int32, device=dev)}
    ws = native._workspace(N, dev)
    ws.fill_(0x7FFFFFF0)  # a stale list: stage 1 has to reset it
    for name in entries:
        if name == "pcs_pure_vapor_pressure":
            out["iters"] = None
            native._call(dev, name, Pd, Td, N, out["p_sat"], out["rho_vl"], out["status"], ws)
        elif name == "pcs_pure_vle_fast_ordered":
            native._call(dev, name, Pd, Td, N, out["p_sat"], None, None, out["status"], out["iters"], ws, row_order.row_order(Pd, Td))
        else:
            native._call(dev, name, Pd, Td, N, out["p_sat"], out["rho_eq"], out["rho_vl"], out["status"], out["iters"], ws)
    torch.cuda.synchronize()
    return {k: (v.view(torch.int64) if v.dtype == torch.float64 else v).cpu().numpy() for k, v in out.items() if v is not None}


def assert_same_bits(got, want, keys, what):
    for key in keys:
        differ = np.flatnonzero((got[key] != want[key]).reshape(N, -1).any(axis=1))
        print("%s: %s differs on %d rows" % (what, key, len(differ)))
        assert len(differ) == 0, (what, key, differ[:8].tolist())


@pytest.fixture(scope="module")
def batch(hip_lib):
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return band_batch()


@pytest.fixture(scope="module")
def whole(batch):
    """pcs_pure_vle for each output set, computed once"""
    return {name: solve(*batch, ["pcs_pure_vle"], outputs) for name, outputs in SETS.items()}


def test_the_fallback_and_the_robust_pass_both_have_rows(batch):
    from feos_torch_amd import native

    for kind in ({}, {"want_rho_eq": True}, {"want_rho_vl": True}):
        plan = native.PureVlePlan(N, "cuda", ordered=False, **kind)
        plan.run_fast(*batch)
        torch.cuda.synchronize()
        fallback, robust = plan.retry_count()
        print("main-kernel lists %s: fallback %d, robust %d" % (kind, fallback, robust))
        assert fallback > 0 and robust > 0, (kind, fallback, robust)


def test_pressure_only_entries_share_p_sat_and_status(batch, whole):
    want = whole["pressure"]
    assert (want["status"] == 0).sum() > N // 2 and (want["status"] == 1).any()  # solved rows and super-critical ones
    for what, entries, outputs in (("vapor_pressure", ["pcs_pure_vapor_pressure"], ()),
                                   ("vapor_pressure + rho_vl", ["pcs_pure_vapor_pressure"], ("rho_vl",)),
                                   ("fast_ordered + retry", ["pcs_pure_vle_fast_ordered", "pcs_pure_vle_retry"], ())):
        assert_same_bits(solve(*batch, entries, outputs), want, ("p_sat", "status"), what)


@pytest.mark.parametrize("name", list(SETS))
def test_fast_then_retry_is_the_whole_call(batch, whole, name):
    got = solve(*batch, ["pcs_pure_vle_fast", "pcs_pure_vle_retry"], SETS[name])
    assert_same_bits(got, whole[name], ("p_sat", "status", "iters") + SETS[name], name)


def test_rho_vl_of_the_default_entry_is_the_all_fp64_kernel(batch, whole):
    got = solve(*batch, ["pcs_pure_vle_fp64"], SETS["rho_vl"])
    assert_same_bits(got, whole["rho_vl"], ("p_sat", "status", "iters", "rho_vl"), "pcs_pure_vle_fp64")
