"""A row's result must not depend on where the row sits in its workgroup.

Every kernel that buckets the rows of a workgroup by model class (csrc/block_order.hpp) hands lane t the row at sorted
position t; rows are independent, so the outputs of a batch and of the same batch in reverse order must be bit-identical
after undoing the reversal, status included.  Sizes per kernel, B = its workgroup size: 1 (one live row, fewer rows than
bins), B - 1 and B + 1 (ragged last block), 2 B + 3 (several blocks).  The batches are the seeded synthetic ones, which
contain every model class."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PURE_SIZES = [1, 255, 257, 515]  # B = 256 (pure_kernels.hip)
MIX_SIZES = [1, 127, 129, 259]   # B = 128 (mix_kernels.hip, stability_kernels.hip, gc_kernels.hip)


@pytest.fixture(scope="module")
def native():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from feos_torch_amd import native

    return native


def _d(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _rev(x):
    return None if x is None else x.flip(0).contiguous()


def _assert_same_bits(name, forward, backward, solved=(0,)):
    """forward: outputs of the batch; backward: outputs of the reversed batch.  The status must agree on every row, the other
    outputs on every row whose status is in `solved` (a kernel does not write the values of a row it gives up on)."""
    rows = None
    if "status" in forward:
        st, st_b = forward["status"].view(torch.uint8), backward["status"].view(torch.uint8).flip(0)
        assert torch.equal(st, st_b), f"{name}: status differs on {int((st != st_b).sum())} rows"
        rows = torch.zeros_like(st, dtype=torch.bool)
        for code in solved:
            rows |= st == code
    for key in forward:
        a, b = forward[key], backward[key]
        if a is None:
            assert b is None
            continue
        n = a.shape[0]
        a = a.contiguous().reshape(n, -1).view(torch.uint8)  # bits: NaN rows compare too
        b = b.flip(0).contiguous().reshape(n, -1).view(torch.uint8)
        if rows is not None:
            a, b = a[rows], b[rows]
        assert torch.equal(a, b), f"{name}: {key} differs on {int((a != b).any(dim=1).sum())} rows"


@pytest.fixture(scope="module")
def pure_rows():
    from feos_torch_amd.synthetic import pure_batch, pure_pressures

    n = max(PURE_SIZES)
    P, T = pure_batch(n, seed=4101)
    classes = {(bool(r[3] != 0.0), bool(r[4] != 0.0)) for r in P}
    assert len(classes) == 4  # none, polar, associating, both
    return _d(P), _d(T), _d(pure_pressures(n, seed=4102))


@pytest.mark.parametrize("n", PURE_SIZES)
def test_pure_vle_kernels(native, pure_rows, n):
    P, T, _ = (x[:n].contiguous() for x in pure_rows)
    for name, call in (
        ("pure_vapor_pressure", lambda p, t: native.pure_vapor_pressure(p, t)),
        ("pure_vapor_pressure + rho_vl", lambda p, t: native.pure_vapor_pressure(p, t, want_rho_vl=True)),
        ("pure_vle rho_eq", lambda p, t: native.pure_vle(p, t, want_rho_eq=True, want_rho_vl=False)),
        ("pure_vle rho_vl", lambda p, t: native.pure_vle(p, t)),
    ):
        _assert_same_bits(name, call(P, T), call(_rev(P), _rev(T)))


@pytest.mark.parametrize("n", PURE_SIZES)
def test_pure_liquid_density_and_jacobians(native, pure_rows, n):
    P, T, pr = (x[:n].contiguous() for x in pure_rows)
    fw = native.pure_liquid_density(P, T, pr)
    _assert_same_bits("pure_liquid_density", fw, native.pure_liquid_density(_rev(P), _rev(T), _rev(pr)))
    # Jacobians at fixed densities: the forward results are the input of both orders (failed rows carry zeros -> NaN rows)
    rho_vl = torch.stack([torch.zeros_like(fw["rho_root"]), fw["rho_root"]], dim=1).contiguous()
    j = native.pure_jacobian("liquid_density", P, T, pr, rho_vl)
    _assert_same_bits("pure_jacobian liquid_density", {"jac": j},
                      {"jac": native.pure_jacobian("liquid_density", _rev(P), _rev(T), _rev(pr), _rev(rho_vl))})
    rho_vl = native.pure_vle(P, T)["rho_vl"]
    j = native.pure_jacobian("equilibrium_liquid_density", P, T, None, rho_vl)
    _assert_same_bits("pure_jacobian equilibrium_liquid_density", {"jac": j},
                      {"jac": native.pure_jacobian("equilibrium_liquid_density", _rev(P), _rev(T), None, _rev(rho_vl))})


@pytest.fixture(scope="module")
def mix_rows():
    from feos_torch_amd.synthetic import mix_batch

    P, K, T, X, PI = mix_batch(max(MIX_SIZES), seed=4103)  # classes by row index mod 6: every prefix >= 6 has them all
    # feed states for the stability analysis: liquid-like (eta 0.3) and vapour-like (eta 1e-3) rows alternate
    vol = np.pi / 6.0 * (np.stack([X, 1.0 - X], axis=1) * P[:, :, 0] * P[:, :, 1] ** 3).sum(axis=1)
    eta = np.where(np.arange(len(X)) % 2 == 0, 0.3, 1e-3)
    rho = (eta / vol)[:, None] * np.stack([X, 1.0 - X], axis=1)
    return _d(P), _d(K), _d(T), _d(X), _d(PI), _d(rho)


def _mix_bubble_dew_no_workspace(native, dew, P, K, T, X, PI):
    """pcs_mix_bubble_dew with a null workspace: the one-row-per-lane kernel that buckets inside the workgroup"""
    from feos_torch_amd import _lib

    n, dev = T.shape[0], T.device
    p = torch.empty(n, dtype=torch.float64, device=dev)
    rho4 = torch.empty((n, 4), dtype=torch.float64, device=dev)
    status = torch.empty(n, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.lib().pcs_mix_bubble_dew(int(dew), _lib.ptr(P), _lib.ptr(K), _lib.ptr(T), _lib.ptr(X), _lib.ptr(PI), n,
                                           _lib.ptr(p), _lib.ptr(rho4), _lib.ptr(status), None, None,
                                           _lib.current_stream_ptr(dev))
    _lib.check(rc, "pcs_mix_bubble_dew")
    return {"p": p, "rho4": rho4, "status": status}


def _mix_jacobian_no_workspace(native, dew, P, K, T, rho4):
    from feos_torch_amd import _lib

    n, dev = T.shape[0], T.device
    jac = torch.empty((n, 19), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        rc = _lib.lib().pcs_mix_jacobian(int(dew), _lib.ptr(P), _lib.ptr(K), _lib.ptr(T), _lib.ptr(rho4), n, _lib.ptr(jac), None,
                                         _lib.current_stream_ptr(dev))
    _lib.check(rc, "pcs_mix_jacobian")
    return {"jac": jac}


@pytest.mark.parametrize("n", MIX_SIZES)
def test_mix_kernels(native, mix_rows, n):
    P, K, T, X, PI, rho = (x[:n].contiguous() for x in mix_rows)
    for dew in (False, True):
        fw = _mix_bubble_dew_no_workspace(native, dew, P, K, T, X, PI)
        _assert_same_bits(f"pcs_mix_bubble_dew dew={dew}", fw,
                          _mix_bubble_dew_no_workspace(native, dew, _rev(P), _rev(K), _rev(T), _rev(X), _rev(PI)))
        ok = fw["status"] == 0
        rho4 = torch.where(ok[:, None], fw["rho4"], torch.tensor([1e-6, 1e-6, 5e-3, 5e-3], dtype=torch.float64, device="cuda")).contiguous()
        _assert_same_bits(f"pcs_mix_jacobian dew={dew}", _mix_jacobian_no_workspace(native, dew, P, K, T, rho4),
                          _mix_jacobian_no_workspace(native, dew, _rev(P), _rev(K), _rev(T), _rev(rho4)))
    _assert_same_bits("mix_stability", native.mix_stability(P, K, T, rho),
                      native.mix_stability(_rev(P), _rev(K), _rev(T), _rev(rho)), solved=(0, 1, 2))  # 3: invalid feed


@pytest.fixture(scope="module")
def gc_rows():
    from feos_torch_amd.gc_pcsaft import build_table, encode_rows
    from feos_torch_amd.synthetic import gc_batch, load_segment_table

    table = load_segment_table(os.path.join(ROOT, "tests", "data", "sauer2014_hetero.json"))
    b = gc_batch(max(MIX_SIZES), table, seed=4104)
    ident = [s for s, _ in table]
    rows = _d(encode_rows(ident, b["segment_lists"], b["bond_lists"]))
    seg = torch.tensor(np.stack([v for _, v in table]), dtype=torch.float64)
    kab = torch.zeros((len(ident), len(ident)), dtype=torch.float64)
    for s1, s2, k in b["kab_list"]:
        kab[ident.index(s1), ident.index(s2)] = k
        kab[ident.index(s2), ident.index(s1)] = k
    return build_table(seg.cuda(), kab.cuda()), len(ident), rows, _d(b["phi"]), _d(b["T"]), _d(b["x"]), _d(b["p_init"])


@pytest.mark.parametrize("n", MIX_SIZES)
def test_gc_bubble_dew(native, gc_rows, n):
    tab, S = gc_rows[0], gc_rows[1]
    rows, phi, T, X, PI = (x[:n].contiguous() for x in gc_rows[2:])
    for dew in (False, True):
        fw = native.gc_bubble_dew(tab, S, rows, phi, T, X, PI, dew, order=None)
        bw = native.gc_bubble_dew(tab, S, _rev(rows), _rev(phi), _rev(T), _rev(X), _rev(PI), dew, order=None)
        _assert_same_bits(f"gc_bubble_dew dew={dew}", fw, bw)
