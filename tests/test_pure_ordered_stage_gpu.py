"""GPU: the staging of k_pure_vle_ordered (csrc/pure_vle_rows.hpp, ordered_stage) -- scalar workgroup values, 32-bit
per-lane indices, one bounded read of order[] per lane -- leaves every result where the plain entry puts it.

Every case compares p_sat, status, the list's entries and its counters after pcs_pure_vle_fast_ordered (+ the retry stage)
bit for bit with native.PureVlePlan(n, ordered=False) on the same inputs.

Sizes: 1, 255, 256, 257 (around one workgroup: the clamp of positions past n), 8 * 256 (the swizzle's rem = 0), 9 * 256 + 1
(ten workgroups, nwg % 8 = 2: both arms of the swizzle), 16383, 16387, 2 * 16384 + 5 (around one and two order tiles).
Orders: the plan's own (pcs_pure_row_order), the identity, every 16384-row tile reversed, and a foreign array: the reversed
order with -1, n, INT32_MIN and INT32_MAX sprinkled over it (an entry out of range stands for its own position, so the
valid entries are a reversal of the remaining positions and every row is still solved exactly once).
Rows of the four model classes are interleaved (the batches of tests/test_pure_row_order_gpu.py); one more batch has rows
that leave through the fallback and robust lists (that of test_rows_that_leave_through_the_lists).
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_pure_row_order_gpu as row_order_tests  # noqa: E402

pytestmark = pytest.mark.gpu

R = row_order_tests.R
SIZES = (1, 255, 256, 257, 8 * 256, 9 * 256 + 1, R - 1, R + 3, 2 * R + 5)
ORDERS = ("own", "identity", "reversed", "foreign")
BAD = (-1, None, -2 ** 31, 2 ** 31 - 1)  # None: n


def reversed_tiles(positions):
    """`positions` (ascending) with the members of every R-row tile in descending order"""
    out = positions.copy()
    tile = positions // R
    for k in np.unique(tile):
        sel = tile == k
        out[sel] = positions[sel][::-1]
    return out


def build_order(kind, Pd, Td):
    n = Td.shape[0]
    if kind == "own":
        return row_order_tests.row_order(Pd, Td)
    pos = np.arange(n, dtype=np.int64)
    if kind == "identity":
        order = pos
    elif kind == "reversed":
        order = reversed_tiles(pos)
    else:
        bad = (pos % 7 == 3) | (pos == n - 1)  # the last position too: its entry is the one the clamped lanes read
        order = pos.copy()
        order[~bad] = reversed_tiles(pos[~bad])
        order[bad] = [n if BAD[k % 4] is None else BAD[k % 4] for k in range(int(bad.sum()))]
    return torch.from_numpy(order.astype(np.int32)).to(Pd.device)


def assert_same(got, want, what):
    assert np.array_equal(got[0], want[0]), (what, "p_sat", int((got[0] != want[0]).sum()))
    assert np.array_equal(got[1], want[1]), (what, "status", int((got[1] != want[1]).sum()))
    assert got[3] == want[3], (what, "list counters", got[3], want[3])
    assert np.array_equal(got[2], want[2]), (what, "list entries")


@pytest.fixture(scope="module")
def batches(hip_lib):
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    out = {}
    for n in SIZES:
        P, T = row_order_tests.interleaved_batch(n, seed=1300 + n % 101)
        Pd, Td = torch.from_numpy(P).cuda(), torch.from_numpy(T).cuda()
        out[n] = (Pd, Td, row_order_tests.solve(Pd, Td))
    return out


@pytest.mark.parametrize("kind", ORDERS)
@pytest.mark.parametrize("n", SIZES)
def test_ordered_entry_equals_the_plain_plan(batches, n, kind):
    Pd, Td, want = batches[n]
    assert_same(row_order_tests.solve(Pd, Td, build_order(kind, Pd, Td)), want, (n, kind))


def test_rows_that_leave_through_the_lists(oracle, hip_lib):
    import saturation_grid as sg
    import test_pure_lean_presolve_gpu as lean

    g = sg.grid(orc=oracle)
    sel = np.isin(g.theta, lean.THETAS)
    Pc, Tc = lean.corner_rows()
    P = np.ascontiguousarray(np.concatenate([g.P[sel], Pc]))
    T = np.ascontiguousarray(np.concatenate([g.T[sel], Tc]))
    Pd, Td = torch.from_numpy(P).cuda(), torch.from_numpy(T).cuda()
    want = row_order_tests.solve(Pd, Td)
    assert want[3][0] > 0 and want[3][1] > 0  # both lists have work
    for kind in ORDERS:
        assert_same(row_order_tests.solve(Pd, Td, build_order(kind, Pd, Td)), want, kind)
