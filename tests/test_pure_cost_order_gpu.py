"""GPU: the row order keyed on what the fp32 pre-solve does (k_pure_order_key + k_pure_row_order behind pcs_pure_row_order,
the probe pcs_pure_order_key).

  * the order is sorted by the exported key: inside every tile of 16384 rows the rows of pcs_pure_row_order's output are
    non-decreasing in the key pcs_pure_order_key returns (class * 64 + sub-key); the key is the documented function of the
    raw signature fields (csrc/pure_kernels.hip, order_subkey), repeated here bit for bit; the counts lie within the
    pre-solve's caps (liquid root 1..12 evaluations, coupled iteration 0..8);
  * the key belongs to the row: the same alone, in a batch of 257, at another position of a batch of 2 * 16384 + 5, and on
    a second run;
  * invalid rows (NaN / zero / negative temperatures and parameters) carry the last sub-key of their class, the tiles stay
    permutations, and the solve through that order has the bits of the plain entry;
  * on the batch of tests/test_pure_lean_presolve_gpu.py every row whose pre-solve fails carries the last sub-key, and the
    ordered solve agrees with the plain one bit for bit, lists and retry_count() included;
  * capture: PureVlePlan.run whose FIRST call (the one that builds the order, two kernels) sits inside the capture, replayed
    behind pending work, equals eager.

Shapes: 1, 255, 257 (around one workgroup), 16383, 16387, 2 * 16384 + 5 (around one and two tiles), classes interleaved.
"""
import numpy as np
import pytest
import torch

from test_pure_row_order_gpu import R, SHAPES, classes, interleaved_batch, row_order, solve

pytestmark = pytest.mark.gpu

SUB = 64  # ORDER_SUB of csrc/pure_kernels.hip


def probe(Pd, Td):
    """-> (key [n], raw [n, 4]) of pcs_pure_order_key, as numpy"""
    from feos_torch_amd import native

    n = Td.shape[0]
    key = torch.full((n,), -1, dtype=torch.int32, device=Pd.device)
    raw = torch.full((n, 4), -1, dtype=torch.int32, device=Pd.device)
    native._call(Pd.device, "pcs_pure_order_key", Pd, Td, n, key, raw)
    torch.cuda.synchronize()
    return key.cpu().numpy(), raw.cpu().numpy()


def fields(raw):
    w = raw[:, 0].astype(np.int64) & 0xFFFFFFFF
    m = np.ascontiguousarray(raw[:, 1:]).view(np.float32)
    return {"n_liq": w & 0xFF, "n_cpl": (w >> 8) & 0xFF, "code": (w >> 16) & 0xFF, "flags": (w >> 24) & 0x7F, "usable": (w >> 31) & 1,
            "m_liq": m[:, 0], "m_l": m[:, 1], "m_v": m[:, 2]}


def exponent(x):
    return ((x.astype(np.float32).view(np.int32) >> 23) & 0xFF).astype(np.int64) - 127


def documented_key(P, f):
    """class * 64 + (usable ? order_subkey : 63), order_subkey as the comment in csrc/pure_kernels.hip states it"""
    lo, hi = np.float32(0.03125), np.float32(32.0)
    c = np.minimum(np.maximum(np.fmax(f["m_l"], f["m_v"]), lo), hi).astype(np.float32)
    q = np.minimum(np.maximum(f["m_liq"], lo), hi).astype(np.float32)
    major = np.clip(exponent(c * c) + 8, 0, 15)
    minor = np.clip((exponent(q) + 4) >> 1, 0, 3)
    sub = major * 4 + np.where(major % 2 == 1, 3 - minor, minor)
    return classes(P) * SUB + np.where(f["usable"] == 1, sub, SUB - 1)


@pytest.fixture(scope="module")
def batches(hip_lib):
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    out = {}
    for n in SHAPES:
        P, T = interleaved_batch(n, seed=700 + n % 97)
        Pd, Td = torch.from_numpy(P).cuda(), torch.from_numpy(T).cuda()
        out[n] = (P, T, Pd, Td, probe(Pd, Td))
    return out


@pytest.mark.parametrize("n", SHAPES)
def test_the_order_is_sorted_by_the_exported_key(batches, n):
    P, T, Pd, Td, (key, raw) = batches[n]
    f = fields(raw)
    assert np.array_equal(key, documented_key(P, f))
    assert ((f["n_liq"] >= 1) & (f["n_liq"] <= 12)).all() and (f["n_cpl"] <= 8).all()
    assert n < 255 or (f["usable"] == 1).mean() > 0.9  # the synthetic rows are ordinary sub-critical states
    assert len(np.unique(key % SUB)) > 4 or n < 255  # more than a handful of sub-keys are in use
    order = row_order(Pd, Td).cpu().numpy().astype(np.int64)
    for t0 in range(0, n, R):
        tile = order[t0:t0 + R]
        assert np.array_equal(np.sort(tile), np.arange(t0, min(t0 + R, n))), t0
        assert (np.diff(key[tile]) >= 0).all(), t0


def test_the_key_belongs_to_the_row(batches):
    big = 2 * R + 5
    P, T, Pd, Td, (key, raw) = batches[big]
    again = probe(Pd, Td)
    assert np.array_equal(again[0], key) and np.array_equal(again[1], raw)
    rows = np.array([0, 1, 2, 3, 255, 256, 257, R - 1, R, R + 1, 2 * R - 1, 2 * R, 2 * R + 4])
    for r in rows:  # alone
        k1, r1 = probe(Pd[r:r + 1].contiguous(), Td[r:r + 1].contiguous())
        assert k1[0] == key[r] and np.array_equal(r1[0], raw[r]), r
    # in a batch of 257, at other positions and behind other neighbours
    pick = np.concatenate([rows, np.random.default_rng(5).choice(big, 257 - len(rows), replace=False)])
    k2, r2 = probe(Pd[pick].contiguous(), Td[pick].contiguous())
    assert np.array_equal(k2, key[pick]) and np.array_equal(r2, raw[pick])
    # at another position of the large batch
    shift = 12345
    k3, r3 = probe(torch.roll(Pd, shift, 0).contiguous(), torch.roll(Td, shift, 0).contiguous())
    assert np.array_equal(np.roll(key, shift), k3) and np.array_equal(np.roll(raw, shift, axis=0), r3)


def test_invalid_rows_take_the_last_sub_key_and_do_not_disturb_the_order(hip_lib):
    n = R + 3
    P, T = interleaved_batch(n, seed=811)
    rng = np.random.default_rng(9)
    bad = rng.choice(n, 600, replace=False)  # the kinds of tests/test_pure_gpu.py::test_wide_temperature_range_and_bad_inputs
    T[bad[:100]] = np.nan
    T[bad[100:200]] = 0.0
    T[bad[200:300]] = -50.0
    P[bad[300:400], 0] = np.nan
    P[bad[400:500], 1] = 0.0
    P[bad[500:600], 2] = np.inf
    Pd, Td = torch.from_numpy(P).cuda(), torch.from_numpy(T).cuda()
    key, raw = probe(Pd, Td)
    assert np.array_equal(key[bad], classes(P)[bad] * SUB + SUB - 1)
    assert (fields(raw)["usable"][bad] == 0).all()
    order = row_order(Pd, Td)
    o = order.cpu().numpy().astype(np.int64)
    for t0 in range(0, n, R):
        assert np.array_equal(np.sort(o[t0:t0 + R]), np.arange(t0, min(t0 + R, n))), t0
        assert (np.diff(key[o[t0:t0 + R]]) >= 0).all(), t0
    want, got = solve(Pd, Td), solve(Pd, Td, order)
    assert want[1][bad].all()
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(got[2], want[2]) and got[3] == want[3]


def test_rows_that_leave_the_main_kernel_carry_the_failure_sub_key(oracle, hip_lib):
    """The batch of tests/test_pure_lean_presolve_gpu.py: 5 fallback rows, 2,403 robust rows."""
    import saturation_grid as sg
    import test_pure_lean_presolve_gpu as lean

    g = sg.grid(orc=oracle)
    sel = np.isin(g.theta, lean.THETAS)
    Pc, Tc = lean.corner_rows()
    P = np.ascontiguousarray(np.concatenate([g.P[sel], Pc]))
    T = np.ascontiguousarray(np.concatenate([g.T[sel], Tc]))
    Pd, Td = torch.from_numpy(P).cuda(), torch.from_numpy(T).cuda()
    key, raw = probe(Pd, Td)
    f = fields(raw)
    failed = f["code"] != 0
    assert failed.any()
    assert (f["usable"][failed] == 0).all() and np.array_equal(key[failed], classes(P)[failed] * SUB + SUB - 1)
    want = solve(Pd, Td)
    assert want[3][0] > 0 and want[3][1] > 0  # both lists have work
    # rows without a usable fp32 pre-solve are the ones the main kernel lists for the fallback (bit 31; the fallback kernel
    # clears it on the rows it hands on to the robust pass)
    listed = want[2].astype(np.int64)
    assert np.isin(np.flatnonzero(failed), listed & 0x7FFFFFFF).all()
    assert failed[listed[listed < 0] & 0x7FFFFFFF].all()
    got = solve(Pd, Td, row_order(Pd, Td))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(got[2], want[2]) and got[3] == want[3], (got[3], want[3])


def test_capture_of_the_run_that_builds_the_order_equals_eager(hip_lib):
    from feos_torch_amd import native
    from feos_torch_amd.synthetic import pure_batch

    n = 2 * R + 5
    P, T = pure_batch(n, seed=611)
    T[:25] *= 1.5   # super-critical rows (fail in every pass)
    T[25:80] *= 1.2  # near-critical rows: the fallback and robust passes have work
    dev = torch.device("cuda:0")
    par, tem = torch.from_numpy(P).to(dev), torch.from_numpy(T).to(dev)
    eager = native.PureVlePlan(n, dev)
    eager.run(par, tem)
    torch.cuda.synchronize()
    ref = [t.clone() for t in (eager.p_sat, eager.status, eager.order)]

    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):  # warm-up on the capture stream with ANOTHER plan: this one's order stays unbuilt
        native.PureVlePlan(n, dev).run(par, tem)
    torch.cuda.current_stream(dev).wait_stream(side)
    plan = native.PureVlePlan(n, dev)
    assert not plan.order_built
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        plan.run(par, tem)  # both order kernels + the solve
    assert plan.order_built
    other = native.PureVlePlan(n, dev, want_rho_vl=True)
    for rep in range(3):
        plan.p_sat.fill_(float("nan"))
        plan.status.fill_(7)
        plan.ws.fill_(0x7FFFFFF0)
        plan.order.fill_(-1)  # the replay rebuilds it
        for _ in range(4):  # pending work ahead of the replay
            other.run(par, tem)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(plan.status, ref[1]), rep
        ok = ref[1] == 0  # p_sat of a failed row is not written
        assert torch.equal(plan.p_sat[ok].view(torch.int64), ref[0][ok].view(torch.int64)), rep
        o, k = plan.order.cpu().numpy().astype(np.int64), probe(par, tem)[0]
        for t0 in range(0, n, R):
            assert np.array_equal(np.sort(o[t0:t0 + R]), np.arange(t0, min(t0 + R, n))), (rep, t0)
            assert (np.diff(k[o[t0:t0 + R]]) >= 0).all(), (rep, t0)
