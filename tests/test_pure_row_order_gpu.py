"""GPU: the reusable tile-local row order of the pressure-only pure VLE (pcs_pure_row_order, pcs_pure_vle_fast_ordered,
native.PureVlePlan's kept order).

  * order: every tile of 16384 rows of pcs_pure_row_order's output is a permutation of that tile's indices, with the model
    classes (k1_bucket's Gray order) non-decreasing along the tile.  The tau-bin edges are computed in fp32 on the device and
    are not asserted;
  * result independence: p_sat and status of pcs_pure_vle_fast_ordered + pcs_pure_vle_retry are bit for bit those of
    pcs_pure_vle_fast + pcs_pure_vle_retry with the batch's own order, with an order built from another batch (other
    classes, other T: a stale hint) and with the identity; on the batch of tests/test_pure_lean_presolve_gpu.py (rows that
    leave through the fallback and robust lists) the lists hold the same entries and retry_count() is the same;
  * capture: a hipGraph capture of PureVlePlan.run on a plan whose order is built, replayed behind pending work, equals eager.

Shapes: 1, 255, 257 (around one workgroup), R - 1, R + 3, 2 R + 5 (around one and two tiles, R = 16384), rows of the four
classes interleaved.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

R = 16384  # ORDER_TILE of csrc/pure_kernels.hip
SHAPES = (1, 255, 257, R - 1, R + 3, 2 * R + 5)


def interleaved_batch(n, seed):
    """pure_batch rows with the class set by the row index: none, polar, polar + associating, associating, ..."""
    from feos_torch_amd.synthetic import pure_batch

    P, T = pure_batch(n, seed=seed)
    rng = np.random.default_rng(seed + 1)
    k = np.arange(n) % 4
    polar, assoc = (k == 1) | (k == 2), (k == 2) | (k == 3)
    P[:, 3] = np.where(polar, rng.uniform(0.5, 3.0, n), 0.0)
    P[:, 4] = np.where(assoc, rng.uniform(0.001, 0.05, n), 0.0)
    P[:, 5] = np.where(assoc, rng.uniform(1000.0, 3000.0, n), 0.0)
    P[:, 6] = np.where(assoc, 1.0, 0.0)
    P[:, 7] = np.where(assoc, 1.0, 0.0)
    return np.ascontiguousarray(P), T


def classes(P):
    polar, assoc = P[:, 3] != 0, (P[:, 4] != 0) & ((P[:, 6] != 0) | (P[:, 7] != 0))
    return np.where(polar, np.where(assoc, 2, 1), np.where(assoc, 3, 0))


def row_order(Pd, Td):
    from feos_torch_amd import native

    order = torch.full((Td.shape[0],), -1, dtype=torch.int32, device=Pd.device)
    native._call(Pd.device, "pcs_pure_row_order", Pd, Td, Td.shape[0], order)
    return order


def solve(Pd, Td, order=None):
    """fast (ordered when an order is given) + retry -> (p_sat bits, status, list entries after the fast stage, retry_count)"""
    from feos_torch_amd import native

    n = Td.shape[0]
    plan = native.PureVlePlan(n, Pd.device, ordered=False)
    plan.p_sat.zero_()
    plan.status.fill_(7)
    if order is None:
        plan.run_fast(Pd, Td)
    else:
        native._call(Pd.device, "pcs_pure_vle_fast_ordered", Pd, Td, n, plan.p_sat, None, None, plan.status, None, plan.ws, order)
    torch.cuda.synchronize()
    counts = plan.retry_count()
    entries = np.sort(plan.ws[1:1 + sum(counts)].cpu().numpy())
    plan.run_retry(Pd, Td)
    torch.cuda.synchronize()
    return plan.p_sat.view(torch.int64).cpu().numpy(), plan.status.cpu().numpy(), entries, counts


@pytest.fixture(scope="module")
def batches(hip_lib):
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    out = {}
    for n in SHAPES:
        P, T = interleaved_batch(n, seed=700 + n % 97)
        out[n] = (P, T, torch.from_numpy(P).cuda(), torch.from_numpy(T).cuda())
    return out


@pytest.mark.parametrize("n", SHAPES)
def test_every_tile_is_a_permutation_with_classes_in_order(batches, n):
    P, T, Pd, Td = batches[n]
    order = row_order(Pd, Td).cpu().numpy().astype(np.int64)
    cls = classes(P)
    for t0 in range(0, n, R):
        tile = order[t0:t0 + R]
        assert np.array_equal(np.sort(tile), np.arange(t0, min(t0 + R, n))), t0
        assert (np.diff(cls[tile]) >= 0).all(), t0


@pytest.mark.parametrize("n", SHAPES)
def test_results_do_not_depend_on_the_order(batches, n):
    P, T, Pd, Td = batches[n]
    want = solve(Pd, Td)
    P2, T2 = interleaved_batch(n, seed=9000 + n % 89)
    P2, T2 = np.roll(P2, 1, axis=0), T2 * 0.93  # other classes at every row, other T
    orders = {"own": row_order(Pd, Td), "stale": row_order(torch.from_numpy(np.ascontiguousarray(P2)).cuda(), torch.from_numpy(T2).cuda()),
              "identity": torch.arange(n, dtype=torch.int32, device=Pd.device)}
    for name, order in orders.items():
        got = solve(Pd, Td, order)
        assert np.array_equal(got[0], want[0]), (name, "p_sat")
        assert np.array_equal(got[1], want[1]), (name, "status")
        assert np.array_equal(got[2], want[2]) and got[3] == want[3], (name, "lists")


def test_rows_that_leave_through_the_lists(oracle, hip_lib):
    """The batch of tests/test_pure_lean_presolve_gpu.py: 5 fallback rows, 2,403 robust rows."""
    import saturation_grid as sg
    import test_pure_lean_presolve_gpu as lean

    g = sg.grid(orc=oracle)
    sel = np.isin(g.theta, lean.THETAS)
    Pc, Tc = lean.corner_rows()
    P = np.ascontiguousarray(np.concatenate([g.P[sel], Pc]))
    T = np.ascontiguousarray(np.concatenate([g.T[sel], Tc]))
    Pd, Td = torch.from_numpy(P).cuda(), torch.from_numpy(T).cuda()
    want = solve(Pd, Td)
    assert want[3][0] > 0 and want[3][1] > 0  # both lists have work
    stale = row_order(torch.flip(Pd, [0]).contiguous(), torch.flip(Td, [0]).contiguous())
    for name, order in (("own", row_order(Pd, Td)), ("stale", stale), ("identity", torch.arange(len(T), dtype=torch.int32, device="cuda"))):
        got = solve(Pd, Td, order)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), name
        assert np.array_equal(got[2], want[2]) and got[3] == want[3], (name, got[3], want[3])


def test_a_foreign_order_array_is_bounded(batches):
    """Entries out of range stand for their own position: nothing is read or written outside the batch."""
    n = 257
    P, T, Pd, Td = batches[n]
    want = solve(Pd, Td)
    order = torch.arange(n, dtype=torch.int32, device="cuda")
    order[3], order[100], order[256] = -5, n, 0x7FFFFFF0
    got = solve(Pd, Td, order)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_plan_keeps_its_order_and_matches_the_plain_plan(batches):
    from feos_torch_amd import native

    n = 2 * R + 5
    P, T, Pd, Td = batches[n]
    plain = native.PureVlePlan(n, "cuda", ordered=False)
    assert plain.order is None
    plain.run(Pd, Td)
    plan = native.PureVlePlan(n, "cuda")
    assert plan.ordered and not plan.order_built and plan.order.shape == (n,)
    plan.run_fast(Pd, Td)
    assert plan.order_built
    kept = plan.order.clone()
    plan.run(Pd * 1.0, Td * 0.99)  # the order stays
    assert torch.equal(plan.order, kept)
    plan.run(Pd, Td)
    torch.cuda.synchronize()
    assert torch.equal(plan.p_sat.view(torch.int64), plain.p_sat.view(torch.int64)) and torch.equal(plan.status, plain.status)
    plan.reorder(Pd, Td * 0.9)
    assert np.array_equal(np.sort(plan.order.cpu().numpy()), np.arange(n))
    for kind in ({"want_rho_vl": True}, {"want_rho_eq": True}, {"all_fp64": True}):
        assert native.PureVlePlan(8, "cuda", **kind).order is None


def test_hipgraph_replay_of_an_ordered_plan_behind_pending_work_equals_eager(hip_lib):
    from feos_torch_amd import native
    from feos_torch_amd.synthetic import pure_batch

    n = 300_000
    P, T = pure_batch(n, seed=611)
    T[:25] *= 1.5   # super-critical rows (fail in every pass)
    T[25:80] *= 1.2  # near-critical rows: the fallback and robust passes have work
    dev = torch.device("cuda:0")
    par, tem = torch.from_numpy(P).to(dev), torch.from_numpy(T).to(dev)
    plan = native.PureVlePlan(n, dev)
    plan.run(par, tem)
    torch.cuda.synchronize()
    assert plan.order_built
    ref = [t.clone() for t in (plan.p_sat, plan.status)]

    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):  # warm-up on the capture stream, as torch recommends
        plan.run(par, tem)
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        plan.run(par, tem)
    other = native.PureVlePlan(n, dev, want_rho_vl=True)
    for rep in range(3):
        plan.p_sat.fill_(float("nan"))
        plan.status.fill_(7)
        plan.ws.fill_(0x7FFFFFF0)  # stale list: a consumer that ran before the reset would see it
        for _ in range(4):  # pending work ahead of the replay
            other.run(par, tem)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(plan.status, ref[1]), rep
        ok = ref[1] == 0  # p_sat of a failed row is not written
        assert torch.equal(plan.p_sat[ok].view(torch.int64), ref[0][ok].view(torch.int64)), rep
