"""``GcPcSaftMix`` / ``GcPcSaft`` — drop-ins for the reference's heterosegmented gc-PC-SAFT classes
(feos_torch/gc_pcsaft.py:13-528, src/gc_pcsaft.rs:15-171) backed by the gfx950 kernels.

Constructor arguments, method names, return order ``(pressure [Pa], nans)`` and the mutate-on-call
semantics follow the reference.  Instead of its dense ``[N,2,S]`` / ``[N,2,S,S]`` tensors the
molecule structures are encoded once into 80 bytes per row (see include/pcsaft_hip.h); identical
molecules are encoded once and re-used.

Gradients: the eight segment parameter vectors, ``k_ab`` (the tensors inside ``binary_segment_records``),
``phi`` and ``temperature`` — everything the reference's autograd reaches (feos_torch/gc_pcsaft.py:14-22,
:54-86).  k_ab and phi enter the model only through the six dispersion aggregates of a row (:177-194);
the kernel returns dp/d(aggregates) and this module chains them with two [S,N]x[N,S] products.  The
segment parameters enter through 26 molecule-level sums, the dispersion double sums and the bond
diameters; ``pcs_gc_segment_gradient`` differentiates through all of them on the device and reduces
g_i dp_i/d(table) over the rows into one [S,8] array.  (The reference's own d/dphi and d/depsilon_k are
NaN whenever the table holds a segment with epsilon_k = 0 such as '>C<' — sqrt(0) under autograd; here
that one non-differentiable term is left out and everything else is finite.)
"""
import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _shell, native
from .native import _detached
from .pcsaft_mix import _incipient_molefrac, _outputs

MAXE = 8  # distinct segment types / bond types per molecule in the 80-byte row encoding


def _encode_molecule(segs, bonds, idx):
    """40 bytes: seg_id[8], seg_cnt[8], bond_a[8], bond_b[8], bond_cnt[8] (counts 0 = unused)."""
    ids = [idx[s] for s in segs]
    scount = {}
    for a in ids:
        scount[a] = scount.get(a, 0) + 1
    bcount = {}
    for i, j in bonds:
        a, b = ids[i], ids[j]
        key = (a, b) if a >= b else (b, a)  # larger index first (feos_torch/gc_pcsaft.py:35)
        bcount[key] = bcount.get(key, 0) + 1
    if len(scount) > MAXE or len(bcount) > MAXE:
        raise ValueError(f"a molecule may use at most {MAXE} distinct segment types and {MAXE} distinct bond types")
    if max(list(scount.values()) + list(bcount.values()) + [0]) > 255:
        raise ValueError("segment / bond multiplicity above 255")
    out = np.zeros(40, dtype=np.uint8)
    for k, (a, c) in enumerate(sorted(scount.items())):
        out[k] = a
        out[8 + k] = c
    for k, ((a, b), c) in enumerate(sorted(bcount.items())):
        out[16 + k] = a
        out[24 + k] = b
        out[32 + k] = c
    return out


def _encoder():
    """The native encoder (csrc_host/gc_encode.cpp, built by feos_torch_amd.build.build_host / __graft_entry__.build)."""
    try:
        from . import _gc_encode
    except ImportError as e:  # pragma: no cover
        raise ImportError("feos_torch_amd._gc_encode is not built: run `python -m feos_torch_amd.build`") from e
    return _gc_encode


def encode_rows(segment_identifier, segment_lists, bond_lists):
    """[N, 80] uint8 row encoding (layout of include/pcsaft_hip.h), by the native encoder."""
    rows = np.zeros((len(segment_lists), 80), dtype=np.uint8)
    _encoder().encode_rows(list(segment_identifier), segment_lists, bond_lists, rows)
    return rows


def encode_rows_device(segment_identifier, segment_lists, bond_lists, device):
    """[N, 80] uint8 row encoding ON THE DEVICE: the host (csrc_host/gc_encode.cpp::encode_indices) encodes every distinct
    molecule once into a 40-byte table entry and writes two int32 per row; the 80-byte rows are gathered from the table on the
    GPU.  8 instead of 80 bytes per row cross the host memory and the PCIe link (1e6 rows: ~0.03 s of host time)."""
    n = len(segment_lists)
    idx = np.empty((n, 2), dtype=np.int32)
    table = np.frombuffer(_encoder().encode_indices(list(segment_identifier), segment_lists, bond_lists, idx), dtype=np.int64)
    if n == 0:
        return torch.zeros((0, 80), dtype=torch.uint8, device=device)
    tab = torch.from_numpy(table.reshape(-1, 5).copy()).to(device)  # [U, 5] 8-byte fields: seg_id, seg_cnt, bond_a, bond_b, bond_cnt
    ix = torch.from_numpy(idx).to(device).long()
    # rows[r] = (field f of molecule 0, field f of molecule 1) for f = 0..4  (layout of include/pcsaft_hip.h)
    return tab[ix].permute(0, 2, 1).contiguous().view(torch.uint8).view(n, 80)


def encode_rows_py(segment_identifier, segment_lists, bond_lists):
    """Pure-Python specification of encode_rows (tests compare the native encoder against it)."""
    idx = {s: i for i, s in enumerate(segment_identifier)}
    cache, id_cache = {}, {}
    n = len(segment_lists)
    rows = np.zeros((n, 80), dtype=np.uint8)
    for r in range(n):
        for c in range(2):
            segs, bonds = segment_lists[r][c], bond_lists[r][c]
            # batches usually re-use the same list objects for the same molecule: identity first
            enc = id_cache.get((id(segs), id(bonds)))
            if enc is None:
                key = (tuple(segs), tuple(map(tuple, bonds)))
                enc = cache.get(key)
                if enc is None:
                    enc = _encode_molecule(segs, bonds, idx)
                    cache[key] = enc
                id_cache[(id(segs), id(bonds))] = enc
            rows[r, 8 * c:8 * c + 8] = enc[0:8]
            rows[r, 16 + 8 * c:16 + 8 * c + 8] = enc[8:16]
            rows[r, 32 + 8 * c:32 + 8 * c + 8] = enc[16:24]
            rows[r, 48 + 8 * c:48 + 8 * c + 8] = enc[24:32]
            rows[r, 64 + 8 * c:64 + 8 * c + 8] = enc[32:40]
    return rows


def build_table(seg, kab):
    """seg [S,8], kab [S,S] (detached, any device) -> flat table [S*8 + 3*S*S] (see include/pcsaft_hip.h)."""
    sigma, eps = seg[:, 1], seg[:, 2]
    s3 = (0.5 * (sigma[:, None] + sigma[None, :])) ** 3
    ee = eps[:, None] * eps[None, :]
    return torch.cat([seg.reshape(-1), (ee.sqrt() * s3).reshape(-1), (ee * s3).reshape(-1), (1.0 - kab).reshape(-1)]).contiguous()


def _device_table(seg, kab, device):
    """build_table on `device` from a model's host copy of the segment parameters and its k_ab matrix (detached here)."""
    return build_table(seg.to(device), kab.detach().to(device, torch.float64))


def _class_order(model, table):
    """Class order of the rows of a GcPcSaftMix / GcPcSaft for the kernels' schedule (native.gc_class_order), kept on the
    model: computed on first use and again after `reduce` — the rows are fixed in between."""
    if model._order is None or model._order.shape[0] != model.rows.shape[0]:
        model._order = native.gc_class_order(table, model.S, model.rows)
    return model._order


def _kab_gradient(table, S, rows, ph, T, dA01, dB01):
    """[S,S] gradient w.r.t. k_ab from the per-row derivatives w.r.t. the mixed aggregates A01, B01 (upstream gradient
    already folded in): d A01 / d K_ab = 2 sqrt(phi0 phi1)/T m0a m1b E1_ab, d B01 / d K_ab = 4 phi0 phi1/T^2 m0a m1b E2_ab K_ab
    with K = 1 - k_ab (feos_torch/gc_pcsaft.py:177-194)."""
    seg_m = table[: S * 8].view(S, 8)[:, 0]
    E1 = table[S * 8: S * 8 + S * S].view(S, S)
    E2 = table[S * 8 + S * S: S * 8 + 2 * S * S].view(S, S)
    K = table[S * 8 + 2 * S * S:].view(S, S)
    M = []
    for c in range(2):  # m-weighted dense counts, built on the device from the row encoding
        ids = rows[:, 8 * c:8 * c + 8].long()
        cnt = rows[:, 16 + 8 * c:16 + 8 * c + 8].to(torch.float64)
        Mc = torch.zeros((rows.shape[0], S), dtype=torch.float64, device=rows.device)
        Mc.scatter_add_(1, ids, cnt * seg_m[ids])
        M.append(Mc)
    pp = ph[:, 0] * ph[:, 1]
    w1 = dA01 * 2.0 * pp.sqrt() / T
    w2 = dB01 * 4.0 * pp / (T * T)
    G1 = M[0].t() @ (w1[:, None] * M[1])
    G2 = M[0].t() @ (w2[:, None] * M[1])
    return -(E1 * G1) - (E2 * K) * G2


def _phi_gradient(dAB, agg, ph):
    """[n,2] gradient w.r.t. phi from the per-row derivatives dAB [n,6] w.r.t. the aggregates (A ~ phi_i, sqrt(phi_0 phi_1),
    B ~ phi_i^2, phi_0 phi_1)."""
    A00, A01, A11, B00, B01, B11 = (agg[:, k] for k in range(6))
    d0 = dAB[:, 0] * A00 + 0.5 * dAB[:, 1] * A01 + 2.0 * dAB[:, 3] * B00 + dAB[:, 4] * B01
    d1 = dAB[:, 2] * A11 + 0.5 * dAB[:, 1] * A01 + 2.0 * dAB[:, 5] * B11 + dAB[:, 4] * B01
    return torch.stack([d0 / ph[:, 0], d1 / ph[:, 1]], dim=1)


class _GcDerivatives(torch.autograd.Function):
    """(a, p, mu, v) = derivatives(...) with gradients to k_ab, phi, temperature, density and the eight segment parameter
    vectors (feos_torch/gc_pcsaft.py:116-253, :443-468 are torch graphs in the reference)."""

    COLUMNS = ((6, 1, (-1,)), (7, 2, (-1, 2)))  # temperature, density in jac9 [n,9]

    @staticmethod
    def forward(ctx, model, kab, phi, temperature, density, *segment_parameters):
        dev = model.device
        table = _device_table(model.seg, kab, dev)
        ph = native._prep(phi, dev, (2,))
        T = native._prep(temperature, dev)
        rho = native._prep(density, dev, (2,))
        ctx.S = model.S
        return _shell.save_state(ctx, (phi, kab, temperature, density, *segment_parameters), (table, model.rows, ph, T, rho),
                                 native.gc_derivatives(table, model.S, model.rows, ph, T, rho))

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        need, devs = ctx.needs_input_grad, ctx.in_devices  # devs: phi, kab, temperature, density, segment parameters
        if all(g is None for g in grads):
            return (None,) * len(need)
        table, rows, ph, T, rho = ctx.saved_tensors
        gseg, jac9, agg = native.gc_derivatives_vjp(table, ctx.S, rows, ph, T, rho, *grads)
        gk = _kab_gradient(table, ctx.S, rows, ph, T, jac9[:, 1], jac9[:, 4]).to(devs[1]) if need[1] else None
        gphi = _phi_gradient(jac9, agg, ph).to(devs[0]) if need[2] else None
        gs = [gseg[:, k].to(dev) if nd else None for k, (dev, nd) in enumerate(zip(devs[4:], need[5:]))]
        return (None, gk, gphi, *_shell.split(jac9, _GcDerivatives.COLUMNS, need[3:5], devs[2:4]), *gs)


class _GcBubbleDew(torch.autograd.Function):
    """value[n_ok], nans[n][, stable[n_ok]], plan = bubble / dew pressure at the temperature `given`, or (solve_t) bubble / dew
    temperature at the pressure `given`, in one kernel (csrc/gc_temperature.hip); `start` is the initial pressure / the first
    iterate of the temperature.  Dense solve, one compaction plan (its 4-byte row count is the call's only host
    synchronisation), single-kernel gathers only when rows were dropped (native.Compaction; the reference drops them inside
    the native call, src/gc_pcsaft.rs:103-171).  A temperature's gradient is the implicit-function theorem on
    p(theta, T) = p_spec: with J_T = dp/dT (column 6 of pcs_gc_jacobian at the solved state) an upstream gradient g of T is the
    upstream gradient g' = -g / J_T of the pressure for k_ab, phi and the segment table -- the pressure's own backward
    kernels -- and dT/dp_spec = 1 / J_T.
    incipient: the outputs gain y [n_ok] behind the flags, the mole fraction of component 1 in the incipient phase (free: rho4
    of the solve), differentiable like the value.  Forward then takes BOTH per-row blocks jac_p, jac_y [n_ok,7] from one
    pcs_gc_point_jacobian; backward chains k_ab and phi from the weighted block g_p jac_p + g_y jac_y (both host chains are
    linear in the block) and makes one pcs_gc_point_segment_gradient call under the weights (g_p, g_y).  Along constant
    pressure, with J_yT = jac_y[:, 6]: g_p = -(g_T + g_y J_yT) / J_T, g_y stays, and dL/dp_spec = (g_T + g_y J_yT) / J_T."""

    @staticmethod
    def forward(ctx, dew, model, kab, phi, given, molefracs, start, check, solve_t, incipient, *segment_parameters):
        dev, S = model.device, model.S
        table = _device_table(model.seg, kab, dev)
        ph = native._prep(phi, dev, (2,))
        known = native._prep(given, dev)
        args = (table, S, model.rows, ph, known, native._prep(molefracs, dev), native._prep(start, dev), dew)
        order = _class_order(model, table)
        r = native.gc_bubble_dew_temperature(*args, order=order) if solve_t else native.gc_bubble_dew(*args, order=order)
        comp = native.Compaction(r["status"])
        value = comp.gather(r["t" if solve_t else "p"])
        at = (lambda: value) if solve_t else (lambda: comp.gather(known))  # temperature of the kept rows: solved or given
        ctx.needs = list(ctx.needs_input_grad[2:5])  # k_ab, phi, `given`
        ctx.seg_needs = list(ctx.needs_input_grad[10:])
        ctx.incipient = incipient
        values, rho4_ok = [value], None
        if incipient:
            rho4_ok = comp.gather(r["rho4"])
            values.append(_incipient_molefrac(rho4_ok, dew))
            ctx.set_materialize_grads(False)  # either upstream gradient may be absent
        if not comp.all_ok:  # the class order belongs to the uncompacted rows: used when every row converged
            order = None
        ctx.comp = None
        if any(ctx.needs) or any(ctx.seg_needs):
            keep = {"table": table, "rows": comp.gather(model.rows), "ph": comp.gather(ph), "T": at()}
            if rho4_ok is None:
                rho4_ok = comp.gather(r["rho4"])
            if solve_t or any(ctx.needs):  # per-row Jacobians for k_ab, phi and T (dp/dT: in every gradient of a temperature)
                if incipient:
                    keep["jac"], keep["jac_y"], keep["agg"] = native.gc_point_jacobian(table, S, keep["rows"], keep["ph"], keep["T"],
                                                                                       rho4_ok, dew, order=order)
                else:
                    keep["jac"], keep["agg"] = native.gc_jacobian(table, S, keep["rows"], keep["ph"], keep["T"], rho4_ok, dew, order=order)
            if any(ctx.seg_needs):  # the segment gradient runs in backward, at the densities
                keep["rho4"] = rho4_ok
                if order is not None:
                    keep["order"] = order
            ctx.kept = tuple(keep)  # what was saved, by name
            ctx.save_for_backward(*keep.values())
            ctx.comp = comp
        ctx.dew, ctx.S, ctx.solve_t = bool(dew), S, solve_t
        ctx.seg_devs = [p.device for p in segment_parameters]
        ctx.devs = (kab.device, phi.device, given.device)
        flags = ()
        if check:
            flags = (_shell.stable_at_solution(comp, r["rho4"], dew, lambda feed: native.gc_stability(
                table, S, comp.gather(model.rows), comp.gather(ph), at(), feed, order=order)),)
        return _outputs(ctx, phi.device, values, r["status"], flags, comp)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_value, *g_rest):
        nseg = len(ctx.seg_needs)
        comp, S = ctx.comp, ctx.S
        if comp is None:  # nothing the value depends on required a gradient
            return (None,) * (10 + nseg)
        if ctx.incipient:  # outputs: value, nans[, stable], y, plan
            return _GcBubbleDew._backward_incipient(ctx, g_value, g_rest[-2])
        kept = dict(zip(ctx.kept, ctx.saved_tensors))
        table, rows, ph, T, jac = kept["table"], kept["rows"], kept["ph"], kept["T"], kept.get("jac")
        g = gp = g_value.to(table.device).contiguous()
        if ctx.solve_t:
            inv = 1.0 / jac[:, 6]
            gp = -g * inv  # upstream gradient of the pressure along p(theta, T) = p_spec
        gk = gphi = ggiven = None
        if ctx.needs[0]:
            gk = _kab_gradient(table, S, rows, ph, T, gp * jac[:, 1], gp * jac[:, 4]).to(ctx.devs[0])
        if ctx.needs[1]:
            gphi = comp.expand(_phi_gradient(jac, kept["agg"], ph), gp).to(ctx.devs[1])
        if ctx.needs[2]:  # dp/dT, or dT/dp_spec = 1 / J_T
            ggiven = (comp.expand(inv, g) if ctx.solve_t else comp.expand(jac, g, 6, 1)).view(comp.n).to(ctx.devs[2])
        gseg = [None] * nseg
        if any(ctx.seg_needs):
            # the whole table in one kernel: sum_i g_i dp_i/d seg[S,8] (the segment-parameter gradient is lazy: it needs
            # the upstream gradient, so unlike the per-row Jacobians above it runs here, not in forward)
            G = native.gc_segment_gradient(table, S, rows, ph, T, kept["rho4"], ctx.dew, gout=gp, order=kept.get("order"))
            gseg = [G[:, k].to(ctx.seg_devs[k]) if need else None for k, need in enumerate(ctx.seg_needs)]
        return (None, None, gk, gphi, ggiven, None, None, None, None, None, *gseg)

    @staticmethod
    def _backward_incipient(ctx, g_value, g_y):
        nseg = len(ctx.seg_needs)
        comp, S = ctx.comp, ctx.S
        if g_value is None and g_y is None:
            return (None,) * (10 + nseg)
        kept = dict(zip(ctx.kept, ctx.saved_tensors))
        table, rows, ph, T = kept["table"], kept["rows"], kept["ph"], kept["T"]
        jac_p, jac_y = kept.get("jac"), kept.get("jac_y")
        gp, gy = (None if g is None else g.to(table.device).contiguous() for g in (g_value, g_y))
        if ctx.solve_t:  # along p(theta, T) = p_spec: the temperature's and y's own T column act through the pressure's gradients
            g_total = gp if gy is None else gy * jac_y[:, 6] if gp is None else gp + gy * jac_y[:, 6]
            dgiven = g_total / jac_p[:, 6]  # dL/dp_spec
            gp = -dgiven
        gk = gphi = ggiven = None
        if any(ctx.needs):
            block = sum(g[:, None] * j for g, j in ((gp, jac_p), (gy, jac_y)) if g is not None)  # [n_ok,7], weights folded in
            if ctx.needs[0]:
                gk = _kab_gradient(table, S, rows, ph, T, block[:, 1], block[:, 4]).to(ctx.devs[0])
            if ctx.needs[1]:
                gphi = comp.expand(_phi_gradient(block, kept["agg"], ph)).to(ctx.devs[1])
            if ctx.needs[2]:
                ggiven = comp.expand(dgiven if ctx.solve_t else block[:, 6].contiguous()).view(comp.n).to(ctx.devs[2])
        gseg = [None] * nseg
        if any(ctx.seg_needs):  # one pass of the table kernel for both functionals
            G = native.gc_point_segment_gradient(table, S, rows, ph, T, kept["rho4"], ctx.dew, gout_p=gp, gout_y=gy,
                                                 order=kept.get("order"))
            gseg = [G[:, k].to(ctx.seg_devs[k]) if need else None for k, need in enumerate(ctx.seg_needs)]
        return (None, None, gk, gphi, ggiven, None, None, None, None, None, *gseg)


class _GcDensity(torch.autograd.Function):
    """rho [n_ok, kmol/m3], nans [n], plan = liquid (phase 0) / vapour (phase 1) density at (T, p, x) in one kernel
    (csrc/gc_density.hip), compacted like _GcBubbleDew.  Gradient to every input by the implicit-function theorem on
    p_model(theta, T, rho x) = p [Pa] 1e-30 / (k_B T): ONE pcs_gc_derivatives_vjp call at the root with the per-row weight
    g_p = w = -g c / (dp/drho) (c = the unit factor) and no other weight -> grad_seg [S,8], jac9 [n_ok,9], agg [n_ok,6]:
        segment vectors: the columns of grad_seg;  k_ab, phi: the pressure's own chains on jac9[:, :6];
        T: jac9[:, 6] + w p_spec / T (the specified reduced pressure depends on T itself);  p: -w 1e-30 / (k_B T);
        x: rho (jac9[:, 7] - jac9[:, 8]).
    The class order is the model's (used by the solve; by the backward call only when no row was dropped)."""

    C = 1.0 / (1e3 * (6.02214076e23 * (1e-10 * 1e-10 * 1e-10)))  # A^-3 -> kmol/m3, as _MixDensity.C
    P_RED = 1e-30 / 1.380649e-23            # p_spec = p [Pa] P_RED / T

    @staticmethod
    def forward(ctx, phase, model, kab, phi, temperature, pressure, molefracs, *segment_parameters):
        dev, S = model.device, model.S
        table = _device_table(model.seg, kab, dev)
        ph = native._prep(phi, dev, (2,))
        T, p, x = native._prep(temperature, dev), native._prep(pressure, dev), native._prep(molefracs, dev)
        order = _class_order(model, table)
        r = native.gc_density(table, S, model.rows, ph, T, p, x, phase, order=order)
        comp = native.Compaction(r["status"])
        rho = comp.gather(r["rho"])
        ctx.needs = list(ctx.needs_input_grad[2:7])  # k_ab, phi, temperature, pressure, molefracs
        ctx.seg_needs = list(ctx.needs_input_grad[7:])
        ctx.set_materialize_grads(False)
        ctx.comp = None
        if any(ctx.needs) or any(ctx.seg_needs):
            x_ok = comp.gather(x)
            keep = {"table": table, "rows": comp.gather(model.rows), "ph": comp.gather(ph), "T": comp.gather(T),
                    "rho2": torch.stack((x_ok * rho, (1.0 - x_ok) * rho), dim=1), "dpdrho": comp.gather(r["dpdrho"]), "p": comp.gather(p)}
            if comp.all_ok:  # the class order belongs to the uncompacted rows
                keep["order"] = order
            ctx.kept = tuple(keep)
            ctx.save_for_backward(*keep.values())
            ctx.comp = comp
        ctx.S = S
        ctx.seg_devs = [q.device for q in segment_parameters]
        ctx.devs = tuple(t.device for t in (kab, phi, temperature, pressure, molefracs))
        return (*_shell.finish(ctx, phi.device, [rho * _GcDensity.C], r["status"]), comp)

    @staticmethod
    @once_differentiable
    def backward(ctx, g, *_):
        nseg = len(ctx.seg_needs)
        comp, S = ctx.comp, ctx.S
        if g is None or comp is None:
            return (None,) * (7 + nseg)
        kept = dict(zip(ctx.kept, ctx.saved_tensors))
        table, rows, ph, T, rho2 = kept["table"], kept["rows"], kept["ph"], kept["T"], kept["rho2"]
        w = -(g.to(table.device) * _GcDensity.C) / kept["dpdrho"]  # g_p
        gseg, jac9, agg = native.gc_derivatives_vjp(table, S, rows, ph, T, rho2, g_p=w, order=kept.get("order"))
        unit = _GcDensity.P_RED / T
        gk = gphi = gT = gp = gx = None
        if ctx.needs[0]:
            gk = _kab_gradient(table, S, rows, ph, T, jac9[:, 1], jac9[:, 4]).to(ctx.devs[0])
        if ctx.needs[1]:
            gphi = comp.expand(_phi_gradient(jac9, agg, ph)).to(ctx.devs[1])
        if ctx.needs[2]:
            gT = comp.expand(jac9[:, 6] + w * kept["p"] * unit / T).view(comp.n).to(ctx.devs[2])
        if ctx.needs[3]:
            gp = comp.expand(-w * unit).view(comp.n).to(ctx.devs[3])
        if ctx.needs[4]:
            gx = comp.expand((rho2[:, 0] + rho2[:, 1]) * (jac9[:, 7] - jac9[:, 8])).view(comp.n).to(ctx.devs[4])
        gs = [gseg[:, k].to(dev) if need else None for k, (dev, need) in enumerate(zip(ctx.seg_devs, ctx.seg_needs))]
        return (None, None, gk, gphi, gT, gp, gx, *gs)


class _GcSaturation(torch.autograd.Function):
    """value [n_ok], nans [n], plan = saturation pressure [Pa] (which 0) or saturated liquid density [kmol/m3] (which 1) of
    molecule `component` of every row taken as a pure fluid, in one kernel (csrc/gc_saturation.hip), compacted like _GcDensity.

    Backward: no kernel of its own, two pcs_gc_derivatives_vjp calls -- at the vapour (rho_V, 0) and at the liquid (rho_L, 0),
    component 1: (0, rho) -- that add into one grad_seg; their jac9 blocks are added too (the k_ab, phi and T chains are linear
    in them, and agg does not depend on the density).  Notation: a the reduced residual Helmholtz energy density, p the reduced
    pressure (the vjp's own a and p), @ a partial derivative at fixed densities, dv = 1/rho_V - 1/rho_L, theta any parameter.
      p_sat.  The reduced equal-area pressure p* = -(a_V/rho_V - a_L/rho_L + ln(rho_V/rho_L)) / dv is stationary in both
        densities at the solution (d p*/d rho_k = (p* - p_k) / (rho_k^2 dv) = 0), so
            dp*/dtheta = -(@a_V/@theta / rho_V - @a_L/@theta / rho_L) / dv.
        With p_sat = p* T k_B 1e30 and an upstream gradient g: w = g T k_B 1e30,
            g_a = -w / (rho_V dv) on the vapour call,   g_a = +w / (rho_L dv) on the liquid call,
        and d p_sat/dT = g k_B 1e30 p* (= g p_sat / T) + the summed jac9[:, 6].
      rho_L.  It is defined by p_L(rho_L, theta) = p*(theta), so with p'_L = dp/drho along the line at the liquid root
            d rho_L/dtheta = (dp*/dtheta - @p_L/@theta) / p'_L:
        the weights of p_sat with w = g c / p'_L (c = A^-3 -> kmol/m3), and g_p = -g c / p'_L on the liquid call as well.  Both
        p* and p_L are reduced pressures of one T: the temperature column is the summed jac9[:, 6], no p/T term appears.
    The segment vectors are the columns of grad_seg; k_ab and phi are the pressure's own chains on the summed jac9[:, :6]
    (_kab_gradient, _phi_gradient), as in _GcDensity.backward.  The class order is used by the backward calls only when no
    row was dropped."""

    @staticmethod
    def forward(ctx, which, component, model, kab, phi, temperature, *segment_parameters):
        dev, S = model.device, model.S
        table = _device_table(model.seg, kab, dev)
        ph = native._prep(phi, dev, (2,))
        T = native._prep(temperature, dev)
        order = _class_order(model, table)
        r = native.gc_pure_vle(table, S, model.rows, ph, T, component, order=order, want=("p_sat", "rho_vl", "dpdrho_vl"))
        comp = native.Compaction(r["status"])
        value = comp.gather(r["p_sat"]) if which == 0 else comp.gather(r["rho_vl"])[:, 1] * _GcDensity.C
        ctx.needs = list(ctx.needs_input_grad[3:6])  # k_ab, phi, temperature
        ctx.seg_needs = list(ctx.needs_input_grad[6:])
        ctx.set_materialize_grads(False)
        ctx.comp = None
        if any(ctx.needs) or any(ctx.seg_needs):
            keep = {"table": table, "rows": comp.gather(model.rows), "ph": comp.gather(ph), "T": comp.gather(T),
                    "rho_vl": comp.gather(r["rho_vl"]), "aux": value if which == 0 else comp.gather(r["dpdrho_vl"])[:, 1].contiguous()}
            if comp.all_ok:  # the class order belongs to the uncompacted rows
                keep["order"] = order
            ctx.kept = tuple(keep)
            ctx.save_for_backward(*keep.values())
            ctx.comp = comp
        ctx.S, ctx.which, ctx.component = S, which, component
        ctx.seg_devs = [q.device for q in segment_parameters]
        ctx.devs = tuple(t.device for t in (kab, phi, temperature))
        return (*_shell.finish(ctx, phi.device, [value], r["status"]), comp)

    @staticmethod
    @once_differentiable
    def backward(ctx, g, *_):
        nseg = len(ctx.seg_needs)
        comp, S = ctx.comp, ctx.S
        if g is None or comp is None:
            return (None,) * (6 + nseg)
        kept = dict(zip(ctx.kept, ctx.saved_tensors))
        table, rows, ph, T, aux = kept["table"], kept["rows"], kept["ph"], kept["T"], kept["aux"]
        rv, rl = kept["rho_vl"][:, 0], kept["rho_vl"][:, 1]
        g = g.to(table.device)
        dv = 1.0 / rv - 1.0 / rl
        if ctx.which == 0:
            w, g_p = g * T / _GcDensity.P_RED, None
        else:
            w = g * _GcDensity.C / aux  # aux: dp/drho at the liquid root
            g_p = -w
        zero = torch.zeros_like(rv)
        at = lambda rho: torch.stack((rho, zero) if ctx.component == 0 else (zero, rho), dim=1)
        gseg, jac_v, agg = native.gc_derivatives_vjp(table, S, rows, ph, T, at(rv), g_a=-w / (rv * dv), order=kept.get("order"))
        gseg, jac_l, _ = native.gc_derivatives_vjp(table, S, rows, ph, T, at(rl), g_a=w / (rl * dv), g_p=g_p, order=kept.get("order"),
                                                   grad_seg=gseg)
        jac9 = jac_v + jac_l
        gk = gphi = gT = None
        if ctx.needs[0]:
            gk = _kab_gradient(table, S, rows, ph, T, jac9[:, 1], jac9[:, 4]).to(ctx.devs[0])
        if ctx.needs[1]:
            gphi = comp.expand(_phi_gradient(jac9, agg, ph)).to(ctx.devs[1])
        if ctx.needs[2]:
            dT = jac9[:, 6] + g * aux / T if ctx.which == 0 else jac9[:, 6].contiguous()  # aux: p_sat [Pa]
            gT = comp.expand(dT).view(comp.n).to(ctx.devs[2])
        gs = [gseg[:, k].to(dev) if need else None for k, (dev, need) in enumerate(zip(ctx.seg_devs, ctx.seg_needs))]
        return (None, None, None, gk, gphi, gT, *gs)


class _GcHenry(torch.autograd.Function):
    """H [n_ok, Pa], nans [n], plan = Henry's law constant of molecule `solute` of every row at infinite dilution in the other,
    pure and saturated, molecule (the solvent v = 1 - solute) in one kernel (csrc/gc_henry.hip), compacted like _GcSaturation.
    H = rho_L k_B T exp(mu_s), rho_L the solvent's saturated liquid density, mu_s the solute's residual chemical potential at
    the partial densities rho_v = rho_L, rho_s = 0.

    Backward: no kernel of its own, the two pcs_gc_derivatives_vjp calls of _GcSaturation (which 1) -- at the solvent's vapour
    (rho_V on column v, 0) and liquid (rho_L on column v, 0) -- adding into one grad_seg, with one more weight.  For any
    parameter theta, at fixed T,
        d ln H/dtheta = @mu_s/@theta + dlnh_drho d rho_L/dtheta,    dlnh_drho = 1/rho_L + @mu_s/@rho_v (the kernel's output),
    and d rho_L/dtheta = (dp*/dtheta - @p_L/@theta) / p'_L with p* stationary in both densities, as _GcSaturation derives it.
    With gH = g H for an upstream gradient g of H, dv = 1/rho_V - 1/rho_L and w = gH dlnh_drho / p'_L:
        vapour call: g_a = -w / (rho_V dv);      liquid call: g_a = +w / (rho_L dv), g_p = -w, g_mu[:, s] = gH.
    T has the explicit factor of H = rho_L T k_B 1e30 exp(mu_s) on top: the summed jac9[:, 6] + gH / T.  The segment vectors are
    the columns of grad_seg; k_ab and phi are the chains on the summed jac9[:, :6] -- unlike the pure methods both phi columns
    and k_ab receive gradients here, through @mu_s/@theta.  The class order is used by the backward calls only when no row was
    dropped."""

    @staticmethod
    def forward(ctx, solute, model, kab, phi, temperature, *segment_parameters):
        dev, S = model.device, model.S
        table = _device_table(model.seg, kab, dev)
        ph = native._prep(phi, dev, (2,))
        T = native._prep(temperature, dev)
        order = _class_order(model, table)
        r = native.gc_henry(table, S, model.rows, ph, T, solute, order=order, want=("rho_vl", "dlnh_drho", "dpdrho_l"))
        comp = native.Compaction(r["status"])
        h = comp.gather(r["h"])
        ctx.needs = list(ctx.needs_input_grad[2:5])  # k_ab, phi, temperature
        ctx.seg_needs = list(ctx.needs_input_grad[5:])
        ctx.set_materialize_grads(False)
        ctx.comp = None
        if any(ctx.needs) or any(ctx.seg_needs):
            keep = {"table": table, "rows": comp.gather(model.rows), "ph": comp.gather(ph), "T": comp.gather(T),
                    "rho_vl": comp.gather(r["rho_vl"]), "h": h, "dlnh_drho": comp.gather(r["dlnh_drho"]),
                    "dpdrho_l": comp.gather(r["dpdrho_l"])}
            if comp.all_ok:  # the class order belongs to the uncompacted rows
                keep["order"] = order
            ctx.kept = tuple(keep)
            ctx.save_for_backward(*keep.values())
            ctx.comp = comp
        ctx.S, ctx.solute = S, solute
        ctx.seg_devs = [q.device for q in segment_parameters]
        ctx.devs = tuple(t.device for t in (kab, phi, temperature))
        return (*_shell.finish(ctx, phi.device, [h], r["status"]), comp)

    @staticmethod
    @once_differentiable
    def backward(ctx, g, *_):
        nseg = len(ctx.seg_needs)
        comp, S = ctx.comp, ctx.S
        if g is None or comp is None:
            return (None,) * (5 + nseg)
        kept = dict(zip(ctx.kept, ctx.saved_tensors))
        table, rows, ph, T = kept["table"], kept["rows"], kept["ph"], kept["T"]
        rv, rl = kept["rho_vl"][:, 0], kept["rho_vl"][:, 1]
        gh = g.to(table.device) * kept["h"]
        dv = 1.0 / rv - 1.0 / rl
        w = gh * kept["dlnh_drho"] / kept["dpdrho_l"]
        zero = torch.zeros_like(rv)
        at = lambda rho: torch.stack((zero, rho) if ctx.solute == 0 else (rho, zero), dim=1)  # rho on the solvent's column
        g_mu = torch.stack((gh, zero) if ctx.solute == 0 else (zero, gh), dim=1)
        gseg, jac_v, agg = native.gc_derivatives_vjp(table, S, rows, ph, T, at(rv), g_a=-w / (rv * dv), order=kept.get("order"))
        gseg, jac_l, _ = native.gc_derivatives_vjp(table, S, rows, ph, T, at(rl), g_a=w / (rl * dv), g_p=-w, g_mu=g_mu,
                                                   order=kept.get("order"), grad_seg=gseg)
        jac9 = jac_v + jac_l
        gk = gphi = gT = None
        if ctx.needs[0]:
            gk = _kab_gradient(table, S, rows, ph, T, jac9[:, 1], jac9[:, 4]).to(ctx.devs[0])
        if ctx.needs[1]:
            gphi = comp.expand(_phi_gradient(jac9, agg, ph)).to(ctx.devs[1])
        if ctx.needs[2]:
            gT = comp.expand(jac9[:, 6] + gh / T).view(comp.n).to(ctx.devs[2])
        gs = [gseg[:, k].to(dev) if need else None for k, (dev, need) in enumerate(zip(ctx.seg_devs, ctx.seg_needs))]
        return (None, None, gk, gphi, gT, *gs)


class GcPcSaftMix(_shell.Reducible):
    def __init__(self, segment_identifier, parameter, segment_lists, bond_lists, binary_segment_records, phi=None):
        """Arguments as the reference (feos_torch/gc_pcsaft.py:14-22): segment identifiers [S], the
        8 segment parameter vectors (m, sigma, epsilon_k, mu, kappa_ab, epsilon_k_ab, na, nb), per-row
        [segments of molecule 1, of molecule 2], per-row bond index pairs, [(s1, s2, k_ab)], phi [N,2]."""
        parameter = tuple(parameter)
        if len(parameter) != 8:
            raise ValueError("parameter must hold the 8 segment parameter vectors (m, sigma, epsilon_k, mu, kappa_ab, epsilon_k_ab, na, nb)")
        self.segment_identifier = list(segment_identifier)
        self.S = len(self.segment_identifier)
        if self.S > 32:
            raise ValueError("at most 32 segment types per table")
        self.device = _first_gpu(phi, *parameter)
        # the caller's tensors stay attached to the model: they are inputs of the autograd Function of every property
        self._segment_parameters = tuple(p if isinstance(p, torch.Tensor) else torch.as_tensor(p, dtype=torch.float64)
                                         for p in parameter)
        for p in self._segment_parameters:
            if p.dtype != torch.float64 or tuple(p.shape) != (self.S,):
                raise ValueError(f"every segment parameter vector must be float64 of shape [{self.S}]")
        self.seg = torch.stack([p.detach().cpu() for p in self._segment_parameters], dim=1).contiguous()
        n = len(segment_lists)
        self.rows = encode_rows_device(self.segment_identifier, segment_lists, bond_lists, self.device)
        # "Only up to one associating segment per component is allowed!" (:76-80)
        is_assoc = ((self.seg[:, 4] * self.seg[:, 5]) != 0).to(self.device)
        for c in range(2):
            cnt = (self.rows[:, 16 + 8 * c:16 + 8 * c + 8] * is_assoc[self.rows[:, 8 * c:8 * c + 8].long()]).sum(dim=1)
            if bool((cnt > 1).any()):
                raise Exception("Only up to one associating segment per component is allowed!")
        self._order = None  # class order of the rows, see _class_order
        self.kab = _kab_matrix(self.segment_identifier, binary_segment_records)  # keeps autograd history
        self.phi = torch.ones((n, 2), dtype=torch.float64) if phi is None else phi
        self.gc_pcsaft = GcPcSaft._from_model(self)

    def _table(self):
        return _device_table(self.seg, self.kab, self.device)

    def helmholtz_energy_density(self, temperature, density, kab=None):
        """a(T, rho_1, rho_2) [A^-3], shape [N, 1] (:116-253); differentiable."""
        return self.derivatives(temperature, density)[0][:, None]

    def derivatives(self, temperature, density):
        """(a, p, mu [N,2], v [N,2]) (:443-468); differentiable w.r.t. the segment parameters, k_ab, phi, temperature and
        density (pcs_gc_derivatives_vjp is the backward pass)."""
        temperature = torch.as_tensor(temperature, dtype=torch.float64)
        density = torch.as_tensor(density, dtype=torch.float64)
        return _GcDerivatives.apply(self, self.kab, self.phi, temperature, density, *self._segment_parameters)

    def bubble_point(self, temperature, liquid_molefracs, pressure, check_stability=False, incipient_molefracs=False):
        """(p [Pa], nans) (:470-490).  check_stability=True: (p, nans, stable) as PcSaftMix.bubble_point.
        incipient_molefracs=True: the tuple gains a LAST element y [float64, aligned with p], the mole fraction of component 1
        in the incipient vapour -- (p, nans, y) or (p, nans, stable, y), the contract of PcSaftMix.bubble_point --
        differentiable w.r.t. the eight segment parameter vectors, k_ab, phi and temperature like p (pcs_gc_point_jacobian,
        pcs_gc_point_segment_gradient); the other elements are those of the default call, bit for bit."""
        return self._point(False, False, temperature, liquid_molefracs, pressure, check_stability, incipient_molefracs)

    def dew_point(self, temperature, vapor_molefracs, pressure, check_stability=False, incipient_molefracs=False):
        """(p [Pa], nans) (:492-512).  check_stability=True: (p, nans, stable) as PcSaftMix.dew_point.
        incipient_molefracs=True: a last element x, the mole fraction of component 1 in the incipient liquid (see bubble_point)."""
        return self._point(False, True, temperature, vapor_molefracs, pressure, check_stability, incipient_molefracs)

    def _point(self, solve_t, dew, given, molefracs, start, check_stability, incipient_molefracs=False):
        """bubble / dew pressure at the temperature `given`, or (solve_t) temperature at the pressure `given`;
        incipient_molefracs: the tuple gains y as its last element, for the temperature solve too (y then differentiable
        w.r.t. the segment vectors, k_ab, phi and the pressure along p(theta, T) = p_spec)"""
        if solve_t:
            given = torch.as_tensor(given, dtype=torch.float64)
        # the mole fractions do not enter the reference's final formula (:483-490) and the initial pressure / first iterate
        # only starts the search: no gradient flows to either
        *out, comp = _GcBubbleDew.apply(dew, self, self.kab, self.phi, given, _detached(molefracs), _detached(start),
                                        bool(check_stability), solve_t, bool(incipient_molefracs), *self._segment_parameters)
        self._reduce(comp)
        return tuple(out)

    def bubble_temperature(self, pressure, liquid_molefracs, temperature, check_stability=False):
        """(T [K], nans): the temperature at which the liquid of mole fraction `liquid_molefracs` (component 1) starts to boil
        at `pressure` [Pa], i.e. bubble_point(T, x, .) = pressure, solved in one kernel (csrc/gc_temperature.hpp) from the
        mandatory first iterate `temperature` [K].  Values for the converged rows only, the model is reduced like bubble_point
        does.  Differentiable w.r.t. the eight segment parameter vectors, k_ab, phi and pressure (implicit-function theorem on
        the pressure's gradients: dT/dp = 1 / (dp/dT)); mole fractions and first iterate receive no gradient.  A row fails
        where no trial temperature near the first iterate has an equilibrium, where the pressure lies above the bubble line,
        or on a branch on which the pressure falls with the temperature (include/pcsaft_hip.h, pcs_gc_bubble_dew_temperature).
        check_stability=True: (T, nans, stable) as for bubble_point.  Not part of the reference's class.
        (The parameter list of this method and of dew_temperature is pinned, so they do not take incipient_molefracs; the
        composition at the solved temperature, differentiable along the line of constant pressure, is
        _point(True, dew, pressure, molefracs, temperature, check_stability, incipient_molefracs=True) -> (T, nans[, stable], y),
        or, through the public methods, bubble_point(T, x, pressure, incipient_molefracs=True) at the T returned here, whose
        autograd graph carries dT/dtheta.)"""
        return self._point(True, False, pressure, liquid_molefracs, temperature, check_stability)

    def dew_temperature(self, pressure, vapor_molefracs, temperature, check_stability=False):
        """(T [K], nans): the temperature at which the vapour of mole fraction `vapor_molefracs` starts to condense at
        `pressure` [Pa] (see bubble_temperature).  The retrograde dew branch near a mixture critical point is not served:
        such rows fail.  check_stability=True: (T, nans, stable) with the stability of the vapour at the solution."""
        return self._point(True, True, pressure, vapor_molefracs, temperature, check_stability)

    def _density(self, phase, temperature, pressure, molefracs):
        as64 = lambda t: t if isinstance(t, torch.Tensor) else torch.as_tensor(t, dtype=torch.float64)
        rho, nans, comp = _GcDensity.apply(phase, self, self.kab, self.phi, as64(temperature), as64(pressure), as64(molefracs),
                                           *self._segment_parameters)
        self._reduce(comp)
        return rho, nans

    def liquid_density(self, temperature, pressure, liquid_molefracs):
        """(rho [kmol/m3], nans): total molar density of the liquid at T [K], p [Pa] and the mole fraction of component 1, the
        contract of PcSaftMix.liquid_density on the gc model: the largest root of p(rho) = p at or below the packing
        fraction 0.5 that is reached from there with dp/drho > 0 throughout, or, where the pressure at 0.5 is below p, the first
        root above it (below 0.74) -- in one kernel (include/pcsaft_hip.h, pcs_gc_density).  Values for the converged rows
        only; the model is reduced like bubble_point does.  A row fails where T, p or x is not finite, T <= 0, p <= 0, x outside
        [0, 1] (x = 0 and x = 1 are valid: a pure gc fluid), phi is not finite, or where the liquid branch ends (dp/drho = 0)
        before it reaches p.  Differentiable w.r.t. the eight segment parameter vectors, k_ab, phi, temperature, pressure and
        the mole fractions (implicit-function theorem, one pcs_gc_derivatives_vjp call).  Not part of the reference's class."""
        return self._density(0, temperature, pressure, liquid_molefracs)

    def vapor_density(self, temperature, pressure, vapor_molefracs):
        """(rho [kmol/m3], nans): total molar density of the vapour at T [K], p [Pa] and the mole fraction of component 1: the
        smallest root of p(rho) = p, reached from the ideal gas with dp/drho > 0 throughout; a row fails where the vapour
        branch ends below p (and for the invalid inputs of liquid_density).  Tuple order, reduction and gradients as for
        liquid_density."""
        return self._density(1, temperature, pressure, vapor_molefracs)

    def _saturation(self, which, temperature, component):
        _molecule_index(component, "component", "taken as a pure fluid")
        temperature = temperature if isinstance(temperature, torch.Tensor) else torch.as_tensor(temperature, dtype=torch.float64)
        value, nans, comp = _GcSaturation.apply(which, int(component), self, self.kab, self.phi, temperature, *self._segment_parameters)
        self._reduce(comp)
        return value, nans

    def vapor_pressure(self, temperature, component=0):
        """(p_sat [Pa], nans): saturation pressure at T [K] of molecule `component` (index 0 or 1, the convention of
        PcSaftMix.henrys_law_constant(solute=...)) of every row taken as a pure fluid -- the contract of
        PcSaftPure.vapor_pressure on the gc model, in one kernel (include/pcsaft_hip.h, pcs_gc_pure_vle).  Values for the solved
        rows only; the model is reduced like liquid_density does.  A row fails where T is not finite or T <= 0, phi is not
        finite, or the pure fluid has no vapour-liquid equilibrium at T (every T at or above its critical temperature); a
        failed row never carries the trivial solution rho_V = rho_L or an "equilibrium" between two dense states.
        Differentiable w.r.t. the eight segment parameter vectors, k_ab, phi and temperature (two pcs_gc_derivatives_vjp calls,
        see _GcSaturation).  The model applies k_ab between segments of unlike molecules only (feos_torch/gc_pcsaft.py:177-194),
        so the k_ab gradient of a pure fluid is exactly zero, as is that of the other molecule's phi.  Any other `component`,
        including True, None or 0.5, raises ValueError.  Not part of the reference's class."""
        return self._saturation(0, temperature, component)

    def equilibrium_liquid_density(self, temperature, component=0):
        """(rho_L [kmol/m3], nans): saturated liquid density at T [K] of molecule `component` of every row taken as a pure
        fluid, the contract of PcSaftPure.equilibrium_liquid_density on the gc model; kernel, failure rules, reduction and
        gradients as for vapor_pressure."""
        return self._saturation(1, temperature, component)

    def henrys_law_constant(self, temperature, solute=1):
        """(H [Pa], nans): Henry's law constant at T [K] of molecule `solute` (index 0 or 1) of every row at infinite dilution in
        the other molecule of the row, taken as a pure, saturated liquid (the solvent v) -- the contract of
        PcSaftMix.henrys_law_constant on the gc model: H = rho_L k_B T exp(mu_s), with rho_L the solvent's saturated liquid
        density (that of equilibrium_liquid_density(T, component=v)) and mu_s the solute's residual chemical potential at the
        partial densities rho_v = rho_L, rho_s = 0 (derivatives).  It is the fugacity-based constant; the K-factor form y p / x
        is not computed.  One kernel (include/pcsaft_hip.h, pcs_gc_henry).  Values for the solved rows only; the model is
        reduced like vapor_pressure does.  A row fails where T is not finite or T <= 0, phi is not finite, the solvent has no
        vapour-liquid equilibrium at T (every failure of vapor_pressure), or H is not finite or <= 0; a supercritical solute is
        an ordinary row.  Differentiable w.r.t. the eight segment parameter vectors, k_ab, phi and temperature (two
        pcs_gc_derivatives_vjp calls, see _GcHenry); unlike the pure methods k_ab and both phi columns receive non-zero
        gradients, which is what makes infinite-dilution data a target for fitting k_ab.  Any other `solute`, including True,
        None or 0.5, raises ValueError.  Not part of the reference's class."""
        _molecule_index(solute, "solute", "infinitely dilute")
        temperature = temperature if isinstance(temperature, torch.Tensor) else torch.as_tensor(temperature, dtype=torch.float64)
        h, nans, comp = _GcHenry.apply(int(solute), self, self.kab, self.phi, temperature, *self._segment_parameters)
        self._reduce(comp)
        return h, nans

    def stability_analysis(self, temperature, density):
        """Tangent-plane stability of the model's rows at T [K] and partial densities density [N,2] (A^-3), without reduction
        or autograd graph: (stable bool [N], tpd [N], trial_density [N,2]) as PcSaftMix.stability_analysis."""
        with torch.no_grad():
            table = self._table()
            r = native.gc_stability(table, self.S, self.rows, self.phi, torch.as_tensor(temperature, dtype=torch.float64),
                                    torch.as_tensor(density, dtype=torch.float64), order=_class_order(self, table))
            out = self.phi.device
            return (r["status"] == 0).to(out), r["tpd"].to(out), r["rho_trial"].to(out)

    def _reduce(self, comp):  # `reduce(nans)` (:514-528) is _shell.Reducible's
        if comp.all_ok:
            return
        self.rows = comp.gather(self.rows)
        self.phi = native.compact_rows(comp, self.phi)
        self._order = None

    def _compute_device(self):
        return self.device


def _molecule_index(value, name, role):
    """the check of `component` / `solute`: a plain integer 0 or 1 (not True, None or 0.5), before anything touches the device"""
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or value not in (0, 1):
        raise ValueError(f"{name} must be 0 or 1 (the index of the molecule of each row that is {role})")


def _kab_matrix(identifier, binary_segment_records, value=lambda k: k):
    """Symmetric [S,S] k_ab matrix built exactly as the reference does (feos_torch/gc_pcsaft.py:60-63): on the CPU, entry by
    entry, so that tensor entries of the records keep their autograd history."""
    idx = {s: i for i, s in enumerate(identifier)}
    kab = torch.zeros((len(identifier), len(identifier)), dtype=torch.float64)
    for s1, s2, k in binary_segment_records:
        kab[idx[s1], idx[s2]] = value(k)
        kab[idx[s2], idx[s1]] = value(k)
    return kab


def _first_gpu(*tensors):
    """The GPU a gc model computes on: the device of the first CUDA tensor among its inputs (phi, segment parameters), else the
    current GPU -- not a device pinned at import or construction time of some other model."""
    for t in tensors:
        if isinstance(t, torch.Tensor) and t.is_cuda:
            return t.device
    return native._dev()


class GcPcSaft:
    """Mirror of the reference's Rust pyclass ``GcPcSaft`` (src/gc_pcsaft.rs:15-99): built from
    segment records, per-row molecule structures, binary segment records and phi; ``bubble_point``
    / ``dew_point`` take numpy arrays and return ``(rho[n_ok,4], status[N])``."""

    def __init__(self, segment_records, segments, bonds, binary_segment_records, phi):
        ident = [s for s, _ in segment_records]
        par = np.stack([np.asarray(v, dtype=np.float64) for _, v in segment_records], axis=0)
        self.S = len(ident)
        self.device = _first_gpu(phi)
        self.seg = torch.from_numpy(par).contiguous()
        self.rows = encode_rows_device(ident, segments, bonds, self.device)
        self.table = _device_table(self.seg, _kab_matrix(ident, binary_segment_records, float), self.device)
        self.phi = torch.as_tensor(np.asarray(phi, dtype=np.float64))
        self._order = None

    @classmethod
    def _from_model(cls, model):
        obj = cls.__new__(cls)
        obj.S, obj.device, obj.seg, obj.rows = model.S, model.device, model.seg, model.rows
        obj.table = model._table()
        obj.phi = model.phi.detach()
        obj._order = None
        return obj

    def _solve(self, temperature, molefracs, pressure, dew):
        t, x, p = (native._as_f64(v, 1) for v in (temperature, molefracs, pressure))
        r = native.gc_bubble_dew(self.table, self.S, self.rows, self.phi, torch.from_numpy(t), torch.from_numpy(x),
                                 torch.from_numpy(p), dew, order=_class_order(self, self.table))
        return native.Compaction(r["status"]).gather(r["rho4"]).cpu().numpy(), r["status"].cpu().numpy()

    def bubble_point(self, temperature, liquid_molefracs, pressure):
        return self._solve(temperature, liquid_molefracs, pressure, False)

    def dew_point(self, temperature, vapor_molefracs, pressure):
        return self._solve(temperature, vapor_molefracs, pressure, True)
