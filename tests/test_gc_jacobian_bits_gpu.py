"""GPU: the bits of the per-row gradient of a converged gc bubble / dew point, jac [n,7] = dp/d(A00, A01, A11, B00, B01, B11, T)
and agg [n,6], row by row against tests/golden/gc_jacobian_bits.json.

The file was recorded at commit ee50bd7 (tests/golden/make_golden_gc_jacobian_bits.py), the last one in which pcs_gc_jacobian
had a kernel of its own, k_gc_jacobian, next to k_gc_point_jacobian<WANT_P, WANT_Y>, which was kept bit-equal to it by hand.
Since then pcs_gc_jacobian launches k_gc_point_jacobian<true, false>, and this recording stands for the kernel that left: the
unit is compiled with -fassociative-math, where a shared subexpression or a guard around a store moves the pressure columns
by 1e-13 (csrc/gc_incipient.hip).  The module passes unchanged at ee50bd7 and after it.

Inputs: the batch of the `ctx` fixture of tests/test_gc_incipient_gpu.py -- the 720 rows of tests/tools/gc_point_rows.py (every
model class; three workgroups of 256 with a ragged last one) at the oracle's converged densities, bubble and dew.  Stored per
problem: a digest of the inputs (a failure then says whether the inputs or the kernel moved) and per row the first 16 hex digits
of the SHA-256 of the row's 7 jac doubles followed by its 6 agg doubles as raw little-endian bytes, so a failure names its rows.

Every row must match for each way the pressure block is reached: native.gc_jacobian without and with the class order,
native.gc_point_jacobian(want_y=False), and jac_p / agg of native.gc_point_jacobian() next to the composition block."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "tools"))
import gc_point_rows as gp  # noqa: E402
from test_gc_incipient_gpu import _device_rows  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(HERE, "golden", "gc_jacobian_bits.json")
PROBLEMS = (False, True)
CALLS = ("gc_jacobian", "gc_jacobian, class order", "gc_point_jacobian(want_y=False)", "gc_point_jacobian()")
HEX = 16  # digits kept of a row's SHA-256
name = lambda dew: "dew" if dew else "bubble"


def batch(oracle, dew):
    """Device arrays of the 720 rows (table, S, rows, phi, T, rho4, ...), as the ctx fixture of test_gc_incipient_gpu builds them"""
    return _device_rows(gp.table(), gp.solved(oracle, dew))


def _bytes(x, dtype):
    return np.ascontiguousarray(x.detach().cpu().numpy()).astype(dtype).tobytes()


def input_digest(b):
    h = hashlib.sha256()
    for key, dtype in (("table", "<f8"), ("rows", "u1"), ("phi", "<f8"), ("T", "<f8"), ("rho4", "<f8")):
        h.update(_bytes(b[key], dtype))
    return h.hexdigest()[:HEX]


def row_digests(jac, agg):
    """[n] hex strings: SHA-256 of each row's 7 jac doubles followed by its 6 agg doubles, little-endian"""
    assert jac.shape[1:] == (7,) and agg.shape == (jac.shape[0], 6) and jac.dtype == agg.dtype == torch.float64
    both = np.concatenate([jac.detach().cpu().numpy(), agg.detach().cpu().numpy()], axis=1).astype("<f8")
    return [hashlib.sha256(np.ascontiguousarray(r).tobytes()).hexdigest()[:HEX] for r in both]


def run(native, b, dew, call):
    """(jac, agg) of the pressure block through one of CALLS"""
    args = (b["table"], b["S"], b["rows"], b["phi"], b["T"], b["rho4"], dew)
    if call == "gc_jacobian":
        return native.gc_jacobian(*args)
    if call == "gc_jacobian, class order":
        return native.gc_jacobian(*args, order=native.gc_class_order(b["table"], b["S"], b["rows"]))
    if call == "gc_point_jacobian(want_y=False)":
        jac_p, jac_y, agg = native.gc_point_jacobian(*args, want_y=False)
        assert jac_y is None
        return jac_p, agg
    jac_p, jac_y, agg = native.gc_point_jacobian(*args)
    assert jac_y is not None
    return jac_p, agg


@pytest.fixture(scope="module")
def batches(oracle, hip_lib):
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return {dew: batch(oracle, dew) for dew in PROBLEMS}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("dew", PROBLEMS)
def test_every_row_has_the_recorded_bits(batches, golden, dew, call):
    from feos_torch_amd import native

    b, rec = batches[dew], golden[name(dew)]
    want = [rec["rows"][k:k + HEX] for k in range(0, len(rec["rows"]), HEX)]
    assert b["n"] == gp.N == golden["n"] == len(want)
    assert input_digest(b) == rec["inputs"], "the inputs of the recording have moved (row set, oracle densities or table), not the kernel"
    jac, agg = run(native, b, dew, call)
    assert bool(torch.isfinite(jac).all()) and bool(torch.isfinite(agg).all())
    got = row_digests(jac, agg)
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, "%s, %s: %d of %d rows differ from commit %s, first rows %s" % (
        name(dew), call, len(bad), len(want), golden["commit"], bad[:16])
