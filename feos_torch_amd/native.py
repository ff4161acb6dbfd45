"""Device-level wrappers over the C ABI (``include/pcsaft_hip.h``) and the host-side mirror of
the reference's PyO3 class ``PcSaft`` (src/pcsaft.rs:13-80).

Two layers:
  * ``pure_vle`` / ``pure_liquid_density`` / ... : torch CUDA(=HIP) tensors in, dense torch
    tensors out (status mask instead of dropped rows).  Used by the model classes.
  * ``PcSaft``: numpy in / numpy out with exactly the reference extension's signatures and
    output layout (failed rows dropped, ``status`` True = failed), so code written against
    ``feos_torch.feos_torch.PcSaft`` runs unchanged.
"""
import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _lib

_F64 = torch.float64


def _dev(device=None):
    if not torch.cuda.is_available():
        raise _lib.PcsError(
            "feos_torch_amd needs an AMD GPU (torch.cuda.is_available() is False); there is no CPU fallback."
        )
    return torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)


def _prep(x, device, shape_tail=None):
    """float64, contiguous, on `device`, detached."""
    if not isinstance(x, torch.Tensor):
        x = torch.as_tensor(np.asarray(x, dtype=np.float64))
    x = x.detach()
    if x.dtype != _F64:
        raise TypeError(f"expected float64, got {x.dtype}")  # reference: PyReadonlyArray<f64> type error
    x = x.to(device).contiguous()
    if shape_tail is not None and tuple(x.shape[1:]) != tuple(shape_tail):
        raise ValueError(f"expected trailing shape {shape_tail}, got {tuple(x.shape)}")
    return x


def _same_rows(n, **named):
    """Every row-wise argument must have n rows: the kernels launch n lanes over all of them (the reference raises a
    shape error in the same situation, e.g. a model reduced by an earlier property call used with the original T)."""
    for name, t in named.items():
        if t is not None and t.shape[0] != n:
            raise ValueError(f"{name} has {t.shape[0]} rows, expected {n}")


def _device_of(x):
    """The device of a GPU tensor, else the current GPU (host inputs are copied there by _prep)."""
    return x.device if isinstance(x, torch.Tensor) and x.is_cuda else _dev()


def _check_order(order, n, device):
    if order is not None and (order.dtype != torch.int32 or order.shape != (n,) or order.device != device or not order.is_contiguous()):
        raise ValueError("order must be a contiguous int32 tensor [n] on the device of the table")


def _call(device, name, *args):
    """One C-ABI call on `device`: tensors and None become pointers, the current stream is appended, a non-zero return
    code raises PcsError with the library's message."""
    with torch.cuda.device(device):
        rc = getattr(_lib.lib(), name)(*[_lib.ptr(a) if a is None or isinstance(a, torch.Tensor) else a for a in args],
                                       _lib.current_stream_ptr(device))
    _lib.check(rc, name)


def _detached(x):
    return x.detach() if isinstance(x, torch.Tensor) else x


def _order_or_none(order, n):
    """A class order of another length than the batch (it belongs to the uncompacted rows) is not used."""
    return order if order is not None and order.shape[0] == n else None


def _new(device, shape, dtype=_F64):
    """Uninitialised output on `device`; shape: a row count or a tuple."""
    return torch.empty(shape, dtype=dtype, device=device)


def _news(device, *shapes):
    """One uninitialised float64 output per shape."""
    return [torch.empty(shape, dtype=_F64, device=device) for shape in shapes]


def _workspace(n, device, mix=False):
    """int32 workspace of pcs_workspace_bytes(n) (mix: pcs_mix_workspace_bytes)"""
    L = _lib.lib()
    nbytes = L.pcs_mix_workspace_bytes(n) if mix else L.pcs_workspace_bytes(n)
    return _new(device, max(1, nbytes // 4), dtype=torch.int32)


def pure_vle(params, temperature, want_p=True, want_rho_eq=False, want_iters=False, want_rho_vl=True, all_fp64=False):
    """Pure VLE on the GPU.  -> dict(p_sat [Pa], rho_eq [kmol/m3], rho_vl [n,2] A^-3, status bool, iters).
    want_rho_vl=False with want_rho_eq=False selects the pressure-only kernel (fp64 finish with the fp32
    pre-solve's dp/drho; densities not returned); rho_vl: the all-fp64 kernel; rho_eq: pressure-only kernel + one exact fp64
    Newton update of the densities.
    all_fp64: the validation twin (pcs_pure_vle_fp64: fp64 second derivatives in every iteration)."""
    device = _device_of(params)
    params = _prep(params, device, (8,))
    temperature = _prep(temperature, device)
    n = temperature.shape[0]
    if params.shape[0] != n:
        raise ValueError("parameters and temperature differ in length")
    p_sat = _new(device, n) if want_p else None
    rho_eq = _new(device, n) if want_rho_eq else None
    rho_vl = _new(device, (n, 2)) if want_rho_vl else None
    status = _new(device, n, dtype=torch.uint8)
    iters = _new(device, n, dtype=torch.int32) if want_iters else None
    ws = _workspace(n, device)
    _call(device, "pcs_pure_vle_fp64" if all_fp64 else "pcs_pure_vle", params, temperature, n, p_sat, rho_eq, rho_vl,
          status, iters, ws)
    return {"p_sat": p_sat, "rho_eq": rho_eq, "rho_vl": rho_vl, "status": status.view(torch.bool), "iters": iters}


def pure_vapor_pressure(params, temperature, want_rho_vl=False):
    """PcSaftPure.vapor_pressure in one call (pcs_pure_vapor_pressure): always the pressure-only kernel, so p_sat has the
    same bits with and without the densities.  -> dict(p_sat [Pa], rho_vl [n,2] A^-3 or None, status bool)."""
    device = _device_of(params)
    params = _prep(params, device, (8,))
    temperature = _prep(temperature, device)
    n = temperature.shape[0]
    _same_rows(n, parameters=params)
    p_sat = _new(device, n)
    rho_vl = _new(device, (n, 2)) if want_rho_vl else None
    status = _new(device, n, dtype=torch.uint8)
    ws = _workspace(n, device)
    _call(device, "pcs_pure_vapor_pressure", params, temperature, n, p_sat, rho_vl, status, ws)
    return {"p_sat": p_sat, "rho_eq": None, "rho_vl": rho_vl, "status": status.view(torch.bool), "iters": None}


class Compaction:
    """Plan of one status mask (K8, csrc/compact_kernels.hip): which rows a property call keeps, in order.  Building it costs
    two small kernels and ONE 4-byte read-back (`n_ok`) -- the only host synchronisation of a property call; `gather` /
    `expand` are single kernels (no boolean-index gathers, no nonzero)."""

    def __init__(self, status):
        """status: bool or uint8 [n] on the GPU, True / 1 = dropped."""
        if status.dtype == torch.bool:
            status = status.view(torch.uint8)
        if status.dtype != torch.uint8 or status.dim() != 1 or not status.is_cuda:
            raise ValueError("status must be a bool / uint8 vector on the GPU")
        self.status = status.contiguous()
        self.n = int(status.shape[0])
        self.device = status.device
        self.cws = _new(self.device, max(1, _lib.lib().pcs_compact_workspace_bytes(self.n) // 4), dtype=torch.int32)
        _call(self.device, "pcs_compact_plan", self.status, self.n, self.cws)
        self.n_ok = int(self.cws[0].item()) if self.n else 0
        self.all_ok = self.n_ok == self.n

    def gather(self, x):
        """Rows of x ([n] or [n, ...] float64, or uint8 rows of a multiple of 8 bytes) that are kept, in order."""
        if self.all_ok:
            return x
        if x.shape[0] != self.n:
            raise ValueError(f"tensor has {x.shape[0]} rows, the mask {self.n}")
        x = x.contiguous()
        tail = tuple(x.shape[1:])
        if x.dtype == torch.uint8:
            flat = x.view(self.n, -1)
            if flat.shape[1] % 8:
                raise ValueError("uint8 rows must be a multiple of 8 bytes")
            return self.gather(flat.view(_F64)).view(torch.uint8).view((self.n_ok,) + tail)
        if x.dtype != _F64:
            raise TypeError(f"expected float64, got {x.dtype}")
        width = 1
        for d in tail:
            width *= int(d)
        out = _new(self.device, (self.n_ok,) + tail)
        if self.n_ok and width:
            _call(self.device, "pcs_compact_rows", self.status, self.n, self.cws, x, width, out, None)
        return out

    def index(self):
        """int32 [n_ok]: original row of every kept row."""
        out = _new(self.device, self.n_ok, dtype=torch.int32)
        if self.n_ok:
            _call(self.device, "pcs_compact_rows", self.status, self.n, self.cws, None, 1, None, out)
        return out

    def expand(self, src, g=None, col0=0, ncol=None):
        """Dense [n, ncol]: g[j] * src[j, col0:col0+ncol] in the row of the j-th kept entry, 0 in dropped rows (the scatter of
        a backward pass fused with its Jacobian product).  src [n_ok] or [n_ok, k] float64; 1-D src gives a 1-D result."""
        one_d = src.dim() == 1
        stride = 1
        for d in src.shape[1:]:
            stride *= int(d)
        src2 = src.contiguous().view(src.shape[0], stride)
        ncol = stride - col0 if ncol is None else ncol
        if src2.shape[0] != self.n_ok or (g is not None and g.shape[0] != self.n_ok):
            raise ValueError("src / g must have one row per kept row")
        if self.n_ok == 0:  # nothing kept: all zeros (an empty tensor has no data pointer to hand to the kernel)
            out = torch.zeros((self.n, ncol), dtype=_F64, device=self.device)
            return out.view(self.n) if (one_d and ncol == 1) else out
        out = _new(self.device, (self.n, ncol))
        if self.n:
            _call(self.device, "pcs_expand_rows", None if self.all_ok else self.status, self.n, self.cws,
                  None if g is None else g.contiguous(), src2, stride, col0, ncol, out)
        return out.view(self.n) if (one_d and ncol == 1) else out


class _CompactRows(torch.autograd.Function):
    """Differentiable row filter of a model (`reduce`): keeps the graph to the caller's parameter tensor like the reference's
    boolean indexing (feos_torch/pcsaft_pure.py:235-243) without its nonzero / index kernels."""

    @staticmethod
    def forward(ctx, comp, x):
        ctx.comp = comp
        ctx.in_device = x.device
        ctx.shape = tuple(x.shape)
        return comp.gather(x.detach().to(comp.device)).to(x.device)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        comp = ctx.comp
        g = g.to(comp.device).contiguous()
        out = comp.expand(g.view(g.shape[0], -1) if g.dim() > 1 else g)
        return None, out.view(ctx.shape).to(ctx.in_device)


def compact_rows(comp, x):
    """x[kept rows] with autograd (identity when every row is kept)."""
    return x if comp.all_ok else _CompactRows.apply(comp, x)


def pure_liquid_density(params, temperature, pressure):
    """-> dict(rho [kmol/m3], rho_root [A^-3], status bool)"""
    device = _device_of(params)
    params = _prep(params, device, (8,))
    temperature = _prep(temperature, device)
    pressure = _prep(pressure, device)
    n = temperature.shape[0]
    if params.shape[0] != n or pressure.shape[0] != n:
        raise ValueError("parameters, temperature and pressure differ in length")
    rho, root = _news(device, n, n)
    status = _new(device, n, dtype=torch.uint8)
    _call(device, "pcs_pure_liquid_density", params, temperature, pressure, n, rho, root, status)
    return {"rho": rho, "rho_root": root, "status": status.view(torch.bool)}


def pure_derivatives(params, temperature, density):
    """(a, p, dp) reduced — PcSaftPure.derivatives (feos_torch/pcsaft_pure.py:180-182)."""
    device = _device_of(params)
    params = _prep(params, device, (8,))
    temperature = _prep(temperature, device)
    density = _prep(density, device)
    n = temperature.shape[0]
    _same_rows(n, parameters=params, density=density)
    a, p, dp = _news(device, n, n, n)
    _call(device, "pcs_pure_derivatives", params, temperature, density, n, a, p, dp)
    return a, p, dp


_WHICH = {"vapor_pressure": 0, "liquid_density": 1, "equilibrium_liquid_density": 2, "boiling_temperature": 3}


JAC_POLISH = 0x100  # PCS_JAC_POLISH (include/pcsaft_hip.h)


def pure_jacobian(which, params, temperature, pressure, rho_vl, polish=False):
    """[n,10] Jacobian w.r.t. (8 parameters, T, p) at fixed densities.  polish: rho_vl are the pressure-only kernel's
    densities (pure_vapor_pressure) and take one fp64 Newton step first.  "boiling_temperature": temperature and rho_vl
    are the outputs of pure_boiling_temperature, pressure may be None; column 8 is zero (T is the property)."""
    device = rho_vl.device
    params = _prep(params, device, (8,))
    temperature = _prep(temperature, device)
    pressure = None if pressure is None else _prep(pressure, device)
    rho_vl = _prep(rho_vl, device, (2,))
    n = temperature.shape[0]
    _same_rows(n, parameters=params, pressure=pressure, rho_vl=rho_vl)
    jac = _new(device, (n, 10))
    _call(device, "pcs_pure_jacobian", _WHICH[which] | (JAC_POLISH if polish else 0), params, temperature, pressure,
          rho_vl, n, jac)
    return jac


def pure_jacobian_vjp(which, params, temperature, pressure, rho_vl, gout, need=(True, True, True), polish=False):
    """Backward pass of a pure-component property on rows that all converged: (grad_params [n,8], grad_T [n], grad_p [n]) =
    gout[:, None] * Jacobian, produced by the Jacobian kernel itself (pcs_pure_jacobian_vjp)."""
    device = rho_vl.device
    params = _prep(params, device, (8,))
    temperature = _prep(temperature, device)
    pressure = None if pressure is None else _prep(pressure, device)
    rho_vl = _prep(rho_vl, device, (2,))
    gout = _prep(gout, device)
    n = temperature.shape[0]
    _same_rows(n, parameters=params, pressure=pressure, rho_vl=rho_vl, gout=gout)
    gp = _new(device, (n, 8)) if need[0] else None
    gt = _new(device, n) if need[1] else None
    gpr = _new(device, n) if (need[2] and (pressure is not None or which == "boiling_temperature")) else None
    _call(device, "pcs_pure_jacobian_vjp", _WHICH[which] | (JAC_POLISH if polish else 0), params, temperature, pressure,
          rho_vl, gout, n, gp, gt, gpr)
    return gp, gt, gpr


def pure_boiling_temperature(parameters, pressure, initial_temperature=None, want_rho_vl=True, want_iters=False):
    """Boiling temperature of every parameter row at `pressure` [Pa] (pcs_pure_boiling_temperature).
    -> dict(t [K], rho_vl [n,2] A^-3 at t or None, status bool (True = failed), iters int32 or None)."""
    device = _device_of(parameters)
    parameters = _prep(parameters, device, (8,))
    pressure = _prep(pressure, device)
    t_init = None if initial_temperature is None else _prep(initial_temperature, device)
    n = parameters.shape[0]
    _same_rows(n, pressure=pressure, initial_temperature=t_init)
    t = _new(device, n)
    rho_vl = _new(device, (n, 2)) if want_rho_vl else None
    status = _new(device, n, dtype=torch.uint8)
    iters = _new(device, n, dtype=torch.int32) if want_iters else None
    _call(device, "pcs_pure_boiling_temperature", parameters, pressure, t_init, n, t, rho_vl, status, iters)
    return {"t": t, "rho_vl": rho_vl, "status": status.view(torch.bool), "iters": iters}


def pure_enthalpy_of_vaporization(parameters, temperature, want_rho_vl=False):
    """Enthalpy of vaporization of every parameter row at `temperature` [K] (pcs_pure_enthalpy_of_vaporization).
    -> dict(dh [kJ/mol], status bool (True = failed)[, rho_vl [n,2] A^-3 at the converged equilibrium])."""
    device = _device_of(parameters)
    parameters = _prep(parameters, device, (8,))
    temperature = _prep(temperature, device)
    n = parameters.shape[0]
    _same_rows(n, temperature=temperature)
    dh = _new(device, n)
    rho_vl = _new(device, (n, 2)) if want_rho_vl else None
    status = _new(device, n, dtype=torch.uint8)
    _call(device, "pcs_pure_enthalpy_of_vaporization", parameters, temperature, n, dh, rho_vl, status)
    out = {"dh": dh, "status": status.view(torch.bool)}
    if want_rho_vl:
        out["rho_vl"] = rho_vl
    return out


def pure_enthalpy_of_vaporization_vjp(parameters, temperature, rho_vl, gout, needs=(True, True)):
    """Backward pass of pure_enthalpy_of_vaporization on solved rows: (g_params [n,8] or None, g_temp [n] or None) =
    gout * d dh / d(parameters, T) along the saturation line (pcs_pure_enthalpy_of_vaporization_vjp)."""
    device = _device_of(rho_vl)
    parameters = _prep(parameters, device, (8,))
    temperature = _prep(temperature, device)
    rho_vl = _prep(rho_vl, device, (2,))
    gout = _prep(gout, device)
    n = parameters.shape[0]
    _same_rows(n, temperature=temperature, rho_vl=rho_vl, gout=gout)
    gp = _new(device, (n, 8)) if needs[0] else None
    gt = _new(device, n) if needs[1] else None
    _call(device, "pcs_pure_enthalpy_of_vaporization_vjp", parameters, temperature, rho_vl, n, gout, gp, gt)
    return gp, gt


def pure_critical_point(params, initial_temperature=None, want_iters=False):
    """Critical point of every parameter row (pcs_pure_critical_point).
    -> dict(t_c [K], p_c [Pa], rho_c [kmol/m3], status bool (True = failed), iters int32 or None)."""
    device = _device_of(params)
    params = _prep(params, device, (8,))
    t_init = None if initial_temperature is None else _prep(initial_temperature, device)
    n = params.shape[0]
    _same_rows(n, initial_temperature=t_init)
    tc, pc, rhoc = _news(device, n, n, n)
    status = _new(device, n, dtype=torch.uint8)
    iters = _new(device, n, dtype=torch.int32) if want_iters else None
    _call(device, "pcs_pure_critical_point", params, t_init, n, tc, pc, rhoc, status, iters)
    return {"t_c": tc, "p_c": pc, "rho_c": rhoc, "status": status.view(torch.bool), "iters": iters}


def pure_critical_point_vjp(params, t_c, rho_c, g_tc=None, g_pc=None, g_rhoc=None):
    """Backward pass of pure_critical_point on converged rows: grad_params [n,8] (pcs_pure_critical_point_vjp)."""
    device = _device_of(t_c)
    params = _prep(params, device, (8,))
    t_c = _prep(t_c, device)
    rho_c = _prep(rho_c, device)
    g_tc = None if g_tc is None else _prep(g_tc, device)
    g_pc = None if g_pc is None else _prep(g_pc, device)
    g_rhoc = None if g_rhoc is None else _prep(g_rhoc, device)
    n = t_c.shape[0]
    _same_rows(n, parameters=params, rho_c=rho_c, g_tc=g_tc, g_pc=g_pc, g_rhoc=g_rhoc)
    gp = _new(device, (n, 8))
    _call(device, "pcs_pure_critical_point_vjp", params, t_c, rho_c, n, g_tc, g_pc, g_rhoc, gp)
    return gp


def _as_f64(x, ndim):
    x = np.asarray(x)
    if x.dtype != np.float64:
        raise TypeError(f"argument must be a float64 array, got {x.dtype}")  # PyReadonlyArray<f64>
    if x.ndim != ndim:
        raise TypeError(f"argument must be {ndim}-dimensional, got {x.ndim}")
    return np.ascontiguousarray(x)


class PureVlePlan:
    """Pre-allocated launch plan for repeated pure-VLE solves on a fixed number of rows: all
    outputs and the retry workspace are allocated once; ``run`` only enqueues kernels on the
    current HIP stream (no allocation, no host synchronisation), so steps can be timed with
    HIP events.

    A pressure-only plan (the default) keeps a tile-local row order (``pcs_pure_row_order``: model class, then bins of how close
    the fp32 pre-solve, which the order kernel runs once on every row, came to needing a third coupled iteration and a third
    liquid-root evaluation) and solves through ``pcs_pure_vle_fast_ordered``: waves of one class and like iteration counts.
    The order is built by the first ``run`` / ``run_fast`` with usable inputs and kept: it is a scheduling hint, results
    do not depend on it, and in a parameter fit the classes and temperatures of the data points stay while the parameters
    move.  ``reorder`` rebuilds it; ``ordered=False`` gives the plain entries.

    The kept order belongs to the ROWS of the first call.  Moved parameters cost it part of its gain (measured x1.19 instead of
    x1.22 against the plain path after a +-5 % move of m, sigma, epsilon), but a plan reused for a DIFFERENT batch of the same n
    (minibatches, streaming) runs with an order that carries no information, and the ordered kernel does not sort by itself:
    that measured 15 % SLOWER than the plain path.  Results are right either way.  Such callers pass ``ordered=False``.
    ``reorder`` is no remedy for them: it is two kernels and costs 0.60 ms per 1e7 rows, 1.1 ordered solves (it runs the
    pre-solve on unsorted rows), against 0.12 ms that an ordered solve saves, so it pays only from the fifth launch on the
    same rows -- a fit, or a batch that comes back."""

    def __init__(self, n, device, want_rho_eq=False, want_rho_vl=False, all_fp64=False, ordered=True):
        self.all_fp64 = bool(all_fp64)
        self.n = int(n)
        self.device = torch.device(device)
        self.p_sat = _new(self.device, self.n)
        self.rho_eq = _new(self.device, self.n) if want_rho_eq else None
        self.rho_vl = _new(self.device, (self.n, 2)) if want_rho_vl else None
        self.status = _new(self.device, self.n, dtype=torch.uint8)
        self.ws = _workspace(self.n, self.device)
        # allocated here: the first run may sit inside a hipGraph capture
        self.ordered = bool(ordered) and not (want_rho_eq or want_rho_vl or all_fp64)
        self.order = _new(self.device, max(1, self.n), dtype=torch.int32) if self.ordered else None
        self.order_built = False

    def _run(self, name, params, temperature):
        _call(self.device, name, params, temperature, self.n, self.p_sat, self.rho_eq, self.rho_vl, self.status, None, self.ws)

    def _usable(self, params, temperature):
        """What the order kernel may read: the n float64 rows and temperatures on the plan's device."""
        return all(isinstance(x, torch.Tensor) and x.dtype == _F64 and x.device == self.p_sat.device and x.is_contiguous()
                   for x in (params, temperature)) and tuple(params.shape) == (self.n, 8) and tuple(temperature.shape) == (self.n,)

    def reorder(self, params, temperature):
        """Rebuild the row order from these parameters and temperatures (two kernels on the current stream)."""
        if not self.ordered:
            raise ValueError("this plan keeps no row order")
        if not self._usable(params, temperature):
            raise ValueError(f"reorder needs float64 [{self.n}, 8] parameters and [{self.n}] temperatures on {self.device}")
        _call(self.device, "pcs_pure_row_order", params, temperature, self.n, self.order)
        self.order_built = True

    def _run_fast_ordered(self, params, temperature):
        """-> False when the plain entry has to be called (no order kept, or inputs the order kernel cannot take: the
        plain entry then names what is wrong with them)."""
        if not self.ordered or not self._usable(params, temperature):
            return False
        if not self.order_built:
            self.reorder(params, temperature)
        _call(self.device, "pcs_pure_vle_fast_ordered", params, temperature, self.n, self.p_sat, None, None, self.status, None,
              self.ws, self.order)
        return True

    def run(self, params, temperature):
        if self._run_fast_ordered(params, temperature):
            self.run_retry(params, temperature)
        else:
            self._run("pcs_pure_vle_fp64" if self.all_fp64 else "pcs_pure_vle", params, temperature)

    def run_fast(self, params, temperature):
        if not self._run_fast_ordered(params, temperature):
            self._run("pcs_pure_vle_fast", params, temperature)

    def run_retry(self, params, temperature):
        self._run("pcs_pure_vle_retry", params, temperature)

    def retry_count(self):
        """Rows of the last run that left the main kernel: (all-fp64 fallback rows, robust-pass rows)."""
        cnt = int(self.ws[0].item())
        entries = self.ws[1:1 + cnt]
        fallback = int((entries < 0).sum().item())  # bit 31 set
        return fallback, cnt - fallback


# ------------------------------------------------------------------------------------------
# binary mixtures
# ------------------------------------------------------------------------------------------
def mix_bubble_dew(params, kij, temperature, molefracs, pressure, dew, want_iters=False):
    """Bubble (dew=False) / dew (dew=True) points.  -> dict(p [Pa], rho4 [n,4] A^-3 = (rhoV_1, rhoV_2,
    rhoL_1, rhoL_2), status bool, iters)."""
    device = _device_of(params)
    params = _prep(params, device, (2, 8))
    kij = _prep(kij, device, (2,))
    temperature = _prep(temperature, device)
    molefracs = _prep(molefracs, device)
    pressure = _prep(pressure, device)
    n = temperature.shape[0]
    if not (params.shape[0] == kij.shape[0] == molefracs.shape[0] == pressure.shape[0] == n):
        raise ValueError("inputs differ in length")
    p, rho4 = _news(device, n, (n, 4))
    status = _new(device, n, dtype=torch.uint8)
    iters = _new(device, n, dtype=torch.int32) if want_iters else None
    ws = _workspace(n, device, mix=True)
    _call(device, "pcs_mix_bubble_dew", int(bool(dew)), params, kij, temperature, molefracs, pressure, n, p, rho4, status,
          iters, ws)
    return {"p": p, "rho4": rho4, "status": status.view(torch.bool), "iters": iters}


def mix_bubble_dew_temperature(params, kij, pressure, molefracs, temperature, dew, want_iters=False, workspace=True):
    """Bubble (dew=False) / dew (dew=True) temperatures at `pressure` [Pa] from the first iterate `temperature` [K]
    (pcs_mix_bubble_dew_temperature).  workspace=False: rows bucketed by class inside each workgroup instead of the
    batch-wide class order (same results).
    -> dict(t [K], rho4 [n,4] A^-3 = (rhoV_1, rhoV_2, rhoL_1, rhoL_2) at t, status bool (True = failed), iters int32 or None)."""
    device = _device_of(params)
    params = _prep(params, device, (2, 8))
    kij = _prep(kij, device, (2,))
    pressure = _prep(pressure, device)
    molefracs = _prep(molefracs, device)
    temperature = _prep(temperature, device)
    n = params.shape[0]
    _same_rows(n, kij=kij, pressure=pressure, molefracs=molefracs, temperature=temperature)
    t, rho4 = _news(device, n, (n, 4))
    status = _new(device, n, dtype=torch.uint8)
    iters = _new(device, n, dtype=torch.int32) if want_iters else None
    ws = _workspace(n, device) if workspace else None
    _call(device, "pcs_mix_bubble_dew_temperature", int(bool(dew)), params, kij, pressure, molefracs, temperature, n, t, rho4,
          status, iters, ws)
    return {"t": t, "rho4": rho4, "status": status.view(torch.bool), "iters": iters}


def mix_derivatives(params, kij, temperature, density):
    """(a [n], p [n], mu [n,2], v [n,2]) — PcSaftMix.derivatives (feos_torch/pcsaft_mix.py:395-420)."""
    device = _device_of(params)
    params = _prep(params, device, (2, 8))
    kij = _prep(kij, device, (2,))
    temperature = _prep(temperature, device)
    density = _prep(density, device, (2,))
    n = temperature.shape[0]
    _same_rows(n, parameters=params, kij=kij, density=density)
    a, p, mu, v = _news(device, n, n, (n, 2), (n, 2))
    _call(device, "pcs_mix_derivatives", params, kij, temperature, density, n, a, p, mu, v)
    return a, p, mu, v


def mix_density(params, kij, temperature, pressure, molefracs, phase):
    """Density root of binary mixtures at (T [K], p [Pa], x = mole fraction of component 1), phase 0 = liquid, 1 = vapour
    (pcs_mix_density).  -> dict(rho [n] total density A^-3, dpdrho [n] reduced dp/drho along x at the root, status bool,
    iters int32 evaluations, -1 for failed rows); outputs of failed rows are 0."""
    if phase not in (0, 1):
        raise ValueError("phase must be 0 (liquid) or 1 (vapour)")
    device = _device_of(params)
    params = _prep(params, device, (2, 8))
    kij = _prep(kij, device, (2,))
    temperature, pressure, molefracs = _prep(temperature, device), _prep(pressure, device), _prep(molefracs, device)
    n = temperature.shape[0]
    _same_rows(n, parameters=params, kij=kij, pressure=pressure, molefracs=molefracs)
    rho, dpdrho = _news(device, n, n)
    status = _new(device, n, dtype=torch.uint8)
    iters = _new(device, n, dtype=torch.int32)
    # no workspace: the entry point accepts the batch-wide class order and does not use it (include/pcsaft_hip.h)
    _call(device, "pcs_mix_density", int(phase), params, kij, temperature, pressure, molefracs, n, rho, dpdrho, status, iters, None)
    return {"rho": rho, "dpdrho": dpdrho, "status": status.view(torch.bool), "iters": iters}


def mix_henry(params, kij, temperature, solute):
    """Henry's law constant of component `solute` (0 or 1) at infinite dilution in the other, pure and saturated, component at
    T [K] (pcs_mix_henry).  -> dict(h [n] Pa, rho_vl [n,2] A^-3 and p_sat [n] Pa of the pure solvent, dlnh_drho [n] A^3 =
    d ln H / d rho_L, status bool); outputs of failed rows are 0."""
    if solute not in (0, 1):
        raise ValueError("solute must be 0 or 1 (component index)")
    device = _device_of(params)
    params = _prep(params, device, (2, 8))
    kij = _prep(kij, device, (2,))
    temperature = _prep(temperature, device)
    n = temperature.shape[0]
    _same_rows(n, parameters=params, kij=kij)
    h, rho_vl, p_sat, dlnh_drho = _news(device, n, (n, 2), n, n)
    status = _new(device, n, dtype=torch.uint8)
    _call(device, "pcs_mix_henry", int(solute), params, kij, temperature, n, h, rho_vl, p_sat, dlnh_drho, status)
    return {"h": h, "rho_vl": rho_vl, "p_sat": p_sat, "dlnh_drho": dlnh_drho, "status": status.view(torch.bool)}


def mix_stability(params, kij, temperature, density):
    """Tangent-plane stability analysis of binary feed states (include/pcsaft_hip.h, pcs_mix_stability) at partial densities
    density [n,2] (A^-3).  -> dict(tpd [n], rho_trial [n,2], status uint8 [n]: 0 stable, 1 unstable, 2 locally unstable,
    3 invalid feed)."""
    device = _device_of(params)
    params = _prep(params, device, (2, 8))
    kij = _prep(kij, device, (2,))
    temperature = _prep(temperature, device)
    density = _prep(density, device, (2,))
    n = temperature.shape[0]
    _same_rows(n, parameters=params, kij=kij, density=density)
    tpd, rho_trial = _news(device, n, (n, 2))
    status = _new(device, n, dtype=torch.uint8)
    _call(device, "pcs_mix_stability", params, kij, temperature, density, n, tpd, rho_trial, status)
    return {"tpd": tpd, "rho_trial": rho_trial, "status": status}


def _pcsaft_bubble_dew(parameters, kij, temperature, molefracs, pressure, dew):
    parameters = _as_f64(parameters, 3)
    kij = _as_f64(kij, 2)
    temperature, molefracs, pressure = _as_f64(temperature, 1), _as_f64(molefracs, 1), _as_f64(pressure, 1)
    r = mix_bubble_dew(torch.from_numpy(parameters), torch.from_numpy(kij), torch.from_numpy(temperature),
                       torch.from_numpy(molefracs), torch.from_numpy(pressure), dew)
    return Compaction(r["status"]).gather(r["rho4"]).cpu().numpy(), r["status"].cpu().numpy()  # filter_binary (:216-231)


class PcSaft:
    """Mirror of the reference's Rust pyclass ``PcSaft`` (src/pcsaft.rs:13-80): static methods,
    float64 numpy arrays in, ``(rho, status)`` numpy arrays out, failed rows dropped from ``rho``."""

    @staticmethod
    def vapor_pressure(parameters, temperature):
        """src/pcsaft.rs:18-26 — rho[n_ok, 4]: col 0 = rho_V, col 1 = rho_L, cols 2-3 zero (:94-101)."""
        parameters = _as_f64(parameters, 2)
        temperature = _as_f64(temperature, 1)
        r = pure_vle(torch.from_numpy(parameters), torch.from_numpy(temperature), want_p=False)
        comp = Compaction(r["status"])  # failed rows dropped on the device (:93-101)
        rho = np.zeros((comp.n_ok, 4))
        rho[:, 0:2] = comp.gather(r["rho_vl"]).cpu().numpy()
        return rho, r["status"].cpu().numpy()

    @staticmethod
    def liquid_density(parameters, temperature, pressure):
        """src/pcsaft.rs:28-41 — rho[n_ok]."""
        parameters = _as_f64(parameters, 2)
        temperature = _as_f64(temperature, 1)
        pressure = _as_f64(pressure, 1)
        r = pure_liquid_density(torch.from_numpy(parameters), torch.from_numpy(temperature),
                                torch.from_numpy(pressure))
        return Compaction(r["status"]).gather(r["rho_root"]).cpu().numpy(), r["status"].cpu().numpy()

    @staticmethod
    def bubble_point(parameters, kij, temperature, liquid_molefracs, pressure):
        """src/pcsaft.rs:43-60 — rho[n_ok, 4] = (rhoV_1, rhoV_2, rhoL_1, rhoL_2), status[N]."""
        return _pcsaft_bubble_dew(parameters, kij, temperature, liquid_molefracs, pressure, False)

    @staticmethod
    def dew_point(parameters, kij, temperature, vapor_molefracs, pressure):
        """src/pcsaft.rs:62-79."""
        return _pcsaft_bubble_dew(parameters, kij, temperature, vapor_molefracs, pressure, True)


def mix_jacobian(params, kij, temperature, rho4, dew):
    """[n,19] gradient of the bubble/dew pressure w.r.t. (params[0,:], params[1,:], kij[0], kij[1], T)."""
    device = rho4.device
    params = _prep(params, device, (2, 8))
    kij = _prep(kij, device, (2,))
    temperature = _prep(temperature, device)
    rho4 = _prep(rho4, device, (4,))
    n = temperature.shape[0]
    _same_rows(n, parameters=params, kij=kij, rho4=rho4)
    jac = _new(device, (n, 19))
    ws = _workspace(n, device)
    _call(device, "pcs_mix_jacobian", int(bool(dew)), params, kij, temperature, rho4, n, jac, ws)
    return jac


def mix_point_jacobian(params, kij, temperature, rho4, dew, want_p=True, want_y=True):
    """(jac_p [n,19] or None, jac_y [n,19] or None): gradients of the bubble/dew pressure [Pa] and of the incipient phase's
    mole fraction of component 1 w.r.t. (params[0,:], params[1,:], kij[0], kij[1], T), one kernel for both
    (pcs_mix_point_jacobian)."""
    if not (want_p or want_y):
        raise ValueError("at least one of want_p / want_y is required")
    device = rho4.device
    params = _prep(params, device, (2, 8))
    kij = _prep(kij, device, (2,))
    temperature = _prep(temperature, device)
    rho4 = _prep(rho4, device, (4,))
    n = temperature.shape[0]
    _same_rows(n, parameters=params, kij=kij, rho4=rho4)
    jac_p = _new(device, (n, 19)) if want_p else None
    jac_y = _new(device, (n, 19)) if want_y else None
    ws = _workspace(n, device)
    _call(device, "pcs_mix_point_jacobian", int(bool(dew)), params, kij, temperature, rho4, n, jac_p, jac_y, ws)
    return jac_p, jac_y


# ------------------------------------------------------------------------------------------
# heterosegmented gc-PC-SAFT
# ------------------------------------------------------------------------------------------
def _check_gc(table, S, rows, n):
    """table / row encoding of include/pcsaft_hip.h on one device, n rows."""
    S = int(S)
    if table.dtype != _F64 or table.dim() != 1 or table.shape[0] != S * 8 + 3 * S * S or not table.is_contiguous():
        raise ValueError(f"table must be a contiguous float64 tensor of {S * 8 + 3 * S * S} elements for S = {S}")
    if rows.dtype != torch.uint8 or rows.dim() != 2 or rows.shape[1] != 80 or not rows.is_contiguous():
        raise ValueError("rows must be a contiguous uint8 tensor [n, 80]")
    if rows.device != table.device:
        raise ValueError(f"rows live on {rows.device}, the segment table on {table.device}")
    _same_rows(n, rows=rows)


def gc_class_order(table, S, rows):
    """Permutation (position -> row, int32 on the device) that sorts the rows of a gc model by model class — association
    class x polarity, expensive classes first — for the `order` argument of gc_bubble_dew.  The rows of a model are
    fixed, so this is computed once per model (and again after `reduce`)."""
    n = rows.shape[0]
    seg = table[: S * 8].view(S, 8)
    ids = rows[:, 0:16].long()
    cnt = rows[:, 16:32].to(_F64)
    par = seg[ids]  # [n,16,8]

    def per_molecule(v):
        return (cnt * v).view(n, 2, 8).sum(dim=2)

    ka, eab = per_molecule(par[:, :, 4]), per_molecule(par[:, :, 5])
    na, nb = per_molecule(par[:, :, 6]), per_molecule(par[:, :, 7])
    mu2 = per_molecule(par[:, :, 3] ** 2)
    associating = ((ka * eab) != 0).sum(dim=1)
    self_assoc = ((na * nb) != 0).sum(dim=1)
    cls = torch.zeros(n, dtype=torch.int64, device=rows.device)
    cls[(associating == 1) & (self_assoc == 1)] = 1
    cls[(associating == 2) & (self_assoc == 1)] = 2
    cls[(associating == 2) & (self_assoc == 2)] = 3
    key = 2 * cls + (mu2 > 0).any(dim=1).long()
    # inside a class: by the number of bond-type and segment-type entries (the trip counts of the per-row loops);
    # measured with host-sorted rows, 1e6 rows: class only 2.09 / 5.65 ms (bubble / dew), with these 2.01 / 5.33 ms
    bonds = (rows[:, 64:80] > 0).view(n, 2, 8).sum(dim=2).max(dim=1).values.long()
    segs = (rows[:, 16:32] > 0).sum(dim=1).long()
    key = (key * 9 + bonds) * 17 + segs
    return torch.argsort(key, descending=True, stable=True).to(torch.int32)


def gc_bubble_dew(table, S, rows, phi, temperature, molefracs, pressure, dew, want_iters=False, order=None):
    """table [S*8+3*S*S] f64, rows [n,80] u8 (include/pcsaft_hip.h); order: optional class order of the rows
    (gc_class_order).  -> dict(p, rho4, status, iters)."""
    device = table.device
    phi = _prep(phi, device, (2,))
    temperature = _prep(temperature, device)
    molefracs = _prep(molefracs, device)
    pressure = _prep(pressure, device)
    n = temperature.shape[0]
    _check_gc(table, S, rows, n)
    _same_rows(n, phi=phi, molefracs=molefracs, pressure=pressure)
    _check_order(order, n, device)
    p, rho4 = _news(device, n, (n, 4))
    status = _new(device, n, dtype=torch.uint8)
    iters = _new(device, n, dtype=torch.int32) if want_iters else None
    ws = _workspace(n, device)
    _call(device, "pcs_gc_bubble_dew", int(bool(dew)), table, int(S), rows, phi, temperature, molefracs, pressure, n, p,
          rho4, status, iters, order, ws)
    return {"p": p, "rho4": rho4, "status": status.view(torch.bool), "iters": iters}


def gc_bubble_dew_temperature(table, S, rows, phi, pressure, molefracs, temperature, dew, want_iters=False, order=None):
    """Bubble (dew=False) / dew (dew=True) temperatures of gc rows at `pressure` [Pa] from the first iterate `temperature` [K]
    (pcs_gc_bubble_dew_temperature).  table / rows / order as for gc_bubble_dew (order None: rows bucketed by class inside
    each workgroup, same results).
    -> dict(t [K], rho4 [n,4] A^-3 = (rhoV_1, rhoV_2, rhoL_1, rhoL_2) at t, status bool (True = failed)[, iters int32])."""
    device = table.device
    phi = _prep(phi, device, (2,))
    pressure = _prep(pressure, device)
    molefracs = _prep(molefracs, device)
    temperature = _prep(temperature, device)
    n = pressure.shape[0]
    _check_gc(table, S, rows, n)
    _same_rows(n, phi=phi, molefracs=molefracs, temperature=temperature)
    _check_order(order, n, device)
    t, rho4 = _news(device, n, (n, 4))
    status = _new(device, n, dtype=torch.uint8)
    iters = _new(device, n, dtype=torch.int32) if want_iters else None
    _call(device, "pcs_gc_bubble_dew_temperature", int(bool(dew)), table, int(S), rows, phi, pressure, molefracs, temperature, n,
          t, rho4, status, iters, order)
    out = {"t": t, "rho4": rho4, "status": status.view(torch.bool)}
    if want_iters:
        out["iters"] = iters
    return out


def gc_derivatives(table, S, rows, phi, temperature, density):
    device = table.device
    phi = _prep(phi, device, (2,))
    temperature = _prep(temperature, device)
    density = _prep(density, device, (2,))
    n = temperature.shape[0]
    _check_gc(table, S, rows, n)
    _same_rows(n, phi=phi, density=density)
    a, p, mu, v = _news(device, n, n, (n, 2), (n, 2))
    _call(device, "pcs_gc_derivatives", table, int(S), rows, phi, temperature, density, n, a, p, mu, v)
    return a, p, mu, v


def gc_density(table, S, rows, phi, temperature, pressure, molefracs, phase, order=None):
    """Density root of gc rows at (T [K], p [Pa], x = mole fraction of component 1), phase 0 = liquid, 1 = vapour
    (pcs_gc_density).  table / rows / order as for gc_bubble_dew (order None: rows bucketed by class inside each workgroup,
    same results).  -> dict(rho [n] total density A^-3, dpdrho [n] reduced dp/drho along x at the root, status bool,
    iters int32 evaluations, -1 for failed rows); outputs of failed rows are 0."""
    if phase not in (0, 1):
        raise ValueError("phase must be 0 (liquid) or 1 (vapour)")
    device = table.device
    phi = _prep(phi, device, (2,))
    temperature, pressure, molefracs = _prep(temperature, device), _prep(pressure, device), _prep(molefracs, device)
    n = temperature.shape[0]
    _check_gc(table, S, rows, n)
    _same_rows(n, phi=phi, pressure=pressure, molefracs=molefracs)
    _check_order(order, n, device)
    rho, dpdrho = _news(device, n, n)
    status = _new(device, n, dtype=torch.uint8)
    iters = _new(device, n, dtype=torch.int32)
    _call(device, "pcs_gc_density", int(phase), table, int(S), rows, phi, temperature, pressure, molefracs, n, rho, dpdrho, status,
          iters, order)
    return {"rho": rho, "dpdrho": dpdrho, "status": status.view(torch.bool), "iters": iters}


def gc_pure_vle(table, S, rows, phi, temperature, component=0, order=None, want=("p_sat", "rho_vl", "dpdrho_vl", "iters")):
    """Vapour-liquid equilibrium of molecule `component` (0 or 1) of every gc row as a pure fluid at T [K] (pcs_gc_pure_vle).
    table / rows / order as for gc_bubble_dew.  -> dict(p_sat [n] Pa, rho_vl [n,2] (rho_V, rho_L) A^-3, dpdrho_vl [n,2] reduced
    dp/drho at the two roots, status bool, iters int32 evaluations, -1 for failed rows); outputs of failed rows are 0.  want:
    the optional outputs to compute (the others are passed as NULL and left out of the dict)."""
    if isinstance(component, bool) or component not in (0, 1):
        raise ValueError("component must be 0 or 1 (molecule index)")
    device = table.device
    phi = _prep(phi, device, (2,))
    temperature = _prep(temperature, device)
    n = temperature.shape[0]
    _check_gc(table, S, rows, n)
    _same_rows(n, phi=phi)
    _check_order(order, n, device)
    out = {"p_sat": _new(device, n) if "p_sat" in want else None,
           "rho_vl": _new(device, (n, 2)) if "rho_vl" in want else None,
           "dpdrho_vl": _new(device, (n, 2)) if "dpdrho_vl" in want else None}
    status = _new(device, n, dtype=torch.uint8)
    iters = _new(device, n, dtype=torch.int32) if "iters" in want else None
    _call(device, "pcs_gc_pure_vle", int(component), table, int(S), rows, phi, temperature, n, out["p_sat"], out["rho_vl"],
          out["dpdrho_vl"], status, iters, order)
    out = {k: v for k, v in out.items() if v is not None}
    out["status"] = status.view(torch.bool)
    if iters is not None:
        out["iters"] = iters
    return out


def gc_henry(table, S, rows, phi, temperature, solute=1, order=None, want=("rho_vl", "p_sat", "dlnh_drho", "dpdrho_l", "iters")):
    """Henry's law constant of molecule `solute` (0 or 1) of every gc row at infinite dilution in the other, pure and saturated,
    molecule at T [K] (pcs_gc_henry).  table / rows / order as for gc_bubble_dew.  -> dict(h [n] Pa, rho_vl [n,2] (rho_V, rho_L)
    A^-3 and p_sat [n] Pa of the pure solvent, dlnh_drho [n] A^3 = d ln H / d rho_L, dpdrho_l [n] reduced dp/drho at the liquid
    root, status bool, iters int32 evaluations, -1 for failed rows); outputs of failed rows are 0.  want: the optional outputs to
    compute (the others are passed as NULL and left out of the dict); h is always computed."""
    if isinstance(solute, bool) or solute not in (0, 1):
        raise ValueError("solute must be 0 or 1 (molecule index)")
    device = table.device
    phi = _prep(phi, device, (2,))
    temperature = _prep(temperature, device)
    n = temperature.shape[0]
    _check_gc(table, S, rows, n)
    _same_rows(n, phi=phi)
    _check_order(order, n, device)
    out = {"h": _new(device, n),
           "rho_vl": _new(device, (n, 2)) if "rho_vl" in want else None,
           "p_sat": _new(device, n) if "p_sat" in want else None,
           "dlnh_drho": _new(device, n) if "dlnh_drho" in want else None,
           "dpdrho_l": _new(device, n) if "dpdrho_l" in want else None}
    status = _new(device, n, dtype=torch.uint8)
    iters = _new(device, n, dtype=torch.int32) if "iters" in want else None
    _call(device, "pcs_gc_henry", int(solute), table, int(S), rows, phi, temperature, n, out["h"], out["rho_vl"], out["p_sat"],
          out["dlnh_drho"], out["dpdrho_l"], status, iters, order)
    out = {k: v for k, v in out.items() if v is not None}
    out["status"] = status.view(torch.bool)
    if iters is not None:
        out["iters"] = iters
    return out


def gc_stability(table, S, rows, phi, temperature, density, order=None):
    """mix_stability for gc rows (pcs_gc_stability); order: optional class order of the rows (gc_class_order), schedule
    only.  -> dict(tpd, rho_trial, status)."""
    device = table.device
    phi = _prep(phi, device, (2,))
    temperature = _prep(temperature, device)
    density = _prep(density, device, (2,))
    n = temperature.shape[0]
    _check_gc(table, S, rows, n)
    _same_rows(n, phi=phi, density=density)
    _check_order(order, n, device)
    tpd, rho_trial = _news(device, n, (n, 2))
    status = _new(device, n, dtype=torch.uint8)
    _call(device, "pcs_gc_stability", table, int(S), rows, phi, temperature, density, n, tpd, rho_trial, status, order)
    return {"tpd": tpd, "rho_trial": rho_trial, "status": status}


def gc_jacobian(table, S, rows, phi, temperature, rho4, dew, order=None):
    """-> jac [n,7] = dp/d(A00, A01, A11, B00, B01, B11, T), agg [n,6].  order: optional class order (gc_class_order)."""
    device = table.device
    phi = _prep(phi, device, (2,))
    temperature = _prep(temperature, device)
    rho4 = _prep(rho4, device, (4,))
    n = temperature.shape[0]
    _check_gc(table, S, rows, n)
    _same_rows(n, phi=phi, rho4=rho4)
    jac, agg = _news(device, (n, 7), (n, 6))
    _call(device, "pcs_gc_jacobian", int(bool(dew)), table, int(S), rows, phi, temperature, rho4, n, jac, agg,
          _order_or_none(order, n))
    return jac, agg


def gc_segment_gradient(table, S, rows, phi, temperature, rho4, dew, gout=None, order=None):
    """[S,8] = sum_i gout[i] * d p_i / d (segment parameter table) at the converged densities rho4 (gout None = 1)."""
    device = table.device
    phi = _prep(phi, device, (2,))
    temperature = _prep(temperature, device)
    rho4 = _prep(rho4, device, (4,))
    gout = None if gout is None else _prep(gout, device)
    n = temperature.shape[0]
    _check_gc(table, S, rows, n)
    _same_rows(n, phi=phi, rho4=rho4, gout=gout)
    grad = torch.zeros((int(S), 8), dtype=_F64, device=device)
    _call(device, "pcs_gc_segment_gradient", int(bool(dew)), table, int(S), rows, phi, temperature, rho4, n, gout, grad,
          _order_or_none(order, n))
    return grad


def _opt(x, device, shape_tail=None):
    return None if x is None else _prep(x, device, shape_tail)


def gc_point_jacobian(table, S, rows, phi, temperature, rho4, dew, want_p=True, want_y=True, order=None):
    """(jac_p [n,7] or None, jac_y [n,7] or None, agg [n,6]): gradients of the gc bubble / dew pressure [Pa] (gc_jacobian's jac,
    bit for bit) and of the incipient phase's mole fraction of component 1 w.r.t. (A00, A01, A11, B00, B01, B11, T), one kernel
    for both (pcs_gc_point_jacobian).  order: optional class order (gc_class_order)."""
    if not (want_p or want_y):
        raise ValueError("at least one of want_p / want_y is required")
    device = table.device
    phi = _prep(phi, device, (2,))
    temperature = _prep(temperature, device)
    rho4 = _prep(rho4, device, (4,))
    n = temperature.shape[0]
    _check_gc(table, S, rows, n)
    _same_rows(n, phi=phi, rho4=rho4)
    jac_p = _new(device, (n, 7)) if want_p else None
    jac_y = _new(device, (n, 7)) if want_y else None
    agg = _new(device, (n, 6))
    _call(device, "pcs_gc_point_jacobian", int(bool(dew)), table, int(S), rows, phi, temperature, rho4, n, jac_p, jac_y, agg,
          _order_or_none(order, n))
    return jac_p, jac_y, agg


def gc_point_segment_gradient(table, S, rows, phi, temperature, rho4, dew, gout_p=None, gout_y=None, order=None):
    """[S,8] = sum_i (gout_p[i] * d p_i + gout_y[i] * d y_i) / d (segment parameter table) at the converged densities rho4, one
    pass of the kernel for both functionals (pcs_gc_point_segment_gradient); a weight vector that is None is 0, one is required."""
    if gout_p is None and gout_y is None:
        raise ValueError("at least one of gout_p / gout_y is required")
    device = table.device
    phi = _prep(phi, device, (2,))
    temperature = _prep(temperature, device)
    rho4 = _prep(rho4, device, (4,))
    gout_p, gout_y = _opt(gout_p, device), _opt(gout_y, device)
    n = temperature.shape[0]
    _check_gc(table, S, rows, n)
    _same_rows(n, phi=phi, rho4=rho4, gout_p=gout_p, gout_y=gout_y)
    grad = torch.zeros((int(S), 8), dtype=_F64, device=device)
    _call(device, "pcs_gc_point_segment_gradient", int(bool(dew)), table, int(S), rows, phi, temperature, rho4, n, gout_p, gout_y,
          grad, _order_or_none(order, n))
    return grad


def pure_derivatives_vjp(params, temperature, density, g_a=None, g_p=None, g_dp=None):
    """Backward of PcSaftPure.derivatives: -> (grad_params [n,8], grad_T [n], grad_rho [n])."""
    device = _device_of(params)
    params = _prep(params, device, (8,))
    temperature, density = _prep(temperature, device), _prep(density, device)
    g_a, g_p, g_dp = _opt(g_a, device), _opt(g_p, device), _opt(g_dp, device)
    n = temperature.shape[0]
    _same_rows(n, parameters=params, density=density, g_a=g_a, g_p=g_p, g_dp=g_dp)
    gpar, gT, grho = _news(device, (n, 8), n, n)
    _call(device, "pcs_pure_derivatives_vjp", params, temperature, density, n, g_a, g_p, g_dp, gpar, gT, grho)
    return gpar, gT, grho


def mix_derivatives_vjp(params, kij, temperature, density, g_a=None, g_p=None, g_mu=None, g_v=None):
    """Backward of PcSaftMix.derivatives: -> grad [n,21] = dL/d(16 parameters, kij0, kij1, T, rho_0, rho_1)."""
    device = _device_of(params)
    params = _prep(params, device, (2, 8))
    kij = _prep(kij, device, (2,))
    temperature, density = _prep(temperature, device), _prep(density, device, (2,))
    g_a, g_p, g_mu, g_v = _opt(g_a, device), _opt(g_p, device), _opt(g_mu, device, (2,)), _opt(g_v, device, (2,))
    n = temperature.shape[0]
    _same_rows(n, parameters=params, kij=kij, density=density, g_a=g_a, g_p=g_p, g_mu=g_mu, g_v=g_v)
    grad = _new(device, (n, 21))
    ws = _workspace(n, device)
    _call(device, "pcs_mix_derivatives_vjp", params, kij, temperature, density, n, g_a, g_p, g_mu, g_v, grad, ws)
    return grad


def gc_derivatives_vjp(table, S, rows, phi, temperature, density, g_a=None, g_p=None, g_mu=None, g_v=None, order=None,
                       grad_seg=None):
    """Backward of GcPcSaftMix.derivatives: -> (grad_seg [S,8], jac9 [n,9] = dL/d(6 aggregates, T, rho_0, rho_1), agg [n,6]).
    grad_seg: an earlier call's [S,8] sum on the device of the table, which this call adds to and returns (None: a new one)."""
    device = table.device
    phi = _prep(phi, device, (2,))
    temperature, density = _prep(temperature, device), _prep(density, device, (2,))
    g_a, g_p, g_mu, g_v = _opt(g_a, device), _opt(g_p, device), _opt(g_mu, device, (2,)), _opt(g_v, device, (2,))
    n = temperature.shape[0]
    _check_gc(table, S, rows, n)
    _same_rows(n, phi=phi, density=density, g_a=g_a, g_p=g_p, g_mu=g_mu, g_v=g_v)
    if grad_seg is None:
        gseg = torch.zeros((int(S), 8), dtype=_F64, device=device)
    else:
        gseg = grad_seg
        if gseg.dtype != _F64 or tuple(gseg.shape) != (int(S), 8) or gseg.device != device or not gseg.is_contiguous():
            raise ValueError(f"grad_seg must be a contiguous float64 tensor [{int(S)}, 8] on the device of the table")
    jac9, agg = _news(device, (n, 9), (n, 6))
    _call(device, "pcs_gc_derivatives_vjp", table, int(S), rows, phi, temperature, density, n, g_a, g_p, g_mu, g_v, gseg,
          jac9, agg, _order_or_none(order, n))
    return gseg, jac9, agg


def mixn_derivatives(params, temperature, density):
    """n-component PcSaftMix.derivatives without k_ij: params [n, nc, 8], density [n, nc] -> (a [n], p [n], mu [n,nc], v [n,nc])."""
    device = _device_of(params)
    if params.dim() != 3 or params.shape[2] != 8 or not 1 <= params.shape[1] <= 6:
        raise ValueError("parameters must have shape [N, n, 8] with 1 <= n <= 6 components")
    nc = int(params.shape[1])
    params = _prep(params, device, (nc, 8))
    temperature = _prep(temperature, device)
    density = _prep(density, device, (nc,))
    n = temperature.shape[0]
    _same_rows(n, parameters=params, density=density)
    a, p, mu, v = _news(device, n, n, (n, nc), (n, nc))
    _call(device, "pcs_mixn_derivatives", params, temperature, density, nc, n, a, p, mu, v)
    return a, p, mu, v


def mixn_derivatives_vjp(params, temperature, density, g_a=None, g_p=None, g_mu=None, g_v=None):
    """Backward of the n-component derivatives: grad [n, 9 nc + 1] = dL/d(parameters [nc][8], T, rho [nc])."""
    device = _device_of(params)
    nc = int(params.shape[1])
    params = _prep(params, device, (nc, 8))
    temperature = _prep(temperature, device)
    density = _prep(density, device, (nc,))
    g_a, g_p, g_mu, g_v = _opt(g_a, device), _opt(g_p, device), _opt(g_mu, device, (nc,)), _opt(g_v, device, (nc,))
    n = temperature.shape[0]
    _same_rows(n, parameters=params, density=density, g_a=g_a, g_p=g_p, g_mu=g_mu, g_v=g_v)
    grad = _new(device, (n, 9 * nc + 1))
    _call(device, "pcs_mixn_derivatives_vjp", params, temperature, density, nc, n, g_a, g_p, g_mu, g_v, grad)
    return grad
