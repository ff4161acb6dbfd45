"""``PcSaftPure`` — drop-in for the reference class of the same name
(feos_torch/pcsaft_pure.py:89-243) backed by the gfx950 kernels.

Same constructor, method names, argument meaning, return-tuple order ``(nans, value)``, units,
row filtering (values only for converged rows, ``nans`` True = failed) and the reference's
quirk of MUTATING the model on every property call (``reduce``, :235-243).

What differs in mechanism, not in results:
  * the solve (Rust/feos in the reference) and the Python tail (:212-215 etc.) are one kernel;
  * gradients w.r.t. parameters / temperature / pressure come from a forward-mode Jacobian
    kernel evaluated at the converged densities instead of torch reverse mode through the
    tail — the same partial derivatives (the densities are detached in the reference too).
Tensors may live on any device; the computation runs on the current AMD GPU and results come
back on the device of ``parameters``.
"""
import torch
from torch.autograd.function import once_differentiable

from . import _shell, native


_COLUMNS = ((0, 8, (-1, 8)), (8, 1, (-1,)), (9, 1, (-1,)))  # parameters, temperature, pressure in the [n,10] Jacobian


class _PureProperty(torch.autograd.Function):
    """value[n_ok], nans[n], plan = property(parameters[n,8], temperature[n], pressure[n] or None)
    ("boiling_temperature": the temperature argument is the optional first iterate and receives no gradient; the value is T)

    One solve (dense outputs + status byte per row), one compaction plan whose 4-byte row count is the call's only host
    synchronisation, then -- only if rows were dropped -- single-kernel gathers (native.Compaction; the reference drops
    the rows inside its native call, src/pcsaft.rs:93-101).  The forward value does not depend on whether a gradient is
    requested: the vapour pressure always comes from the pressure-only kernel (pcs_pure_vapor_pressure)."""

    @staticmethod
    def forward(ctx, which, parameters, temperature, pressure):
        dev = native._device_of(parameters)
        par = native._prep(parameters, dev, (8,))
        T = None if temperature is None else native._prep(temperature, dev)
        P = None
        needs = list(ctx.needs_input_grad[1:4])
        if which == "boiling_temperature":
            needs[1] = False
            P = native._prep(pressure, dev)
            r = native.pure_boiling_temperature(par, P, T, want_rho_vl=any(needs))
            value = T = r["t"]  # the Jacobian is taken at the solved temperature
        elif which == "liquid_density":
            P = native._prep(pressure, dev)
            r = native.pure_liquid_density(par, T, P)
            value = r["rho"]
        elif which == "vapor_pressure":
            r = native.pure_vapor_pressure(par, T, want_rho_vl=any(needs))
            value = r["p_sat"]
        else:
            r = native.pure_vle(par, T, want_p=False, want_rho_eq=True, want_rho_vl=any(needs))
            value = r["rho_eq"]
        comp = native.Compaction(r["status"])
        value = comp.gather(value)
        if any(needs):
            # Jacobian only on converged rows (dense kernel on the compacted inputs)
            if which == "liquid_density":
                root = comp.gather(r["rho_root"])
                rho_vl = torch.stack([torch.zeros_like(root), root], dim=1)
            else:
                rho_vl = comp.gather(r["rho_vl"])
            if comp.all_ok:
                # every row converged (the common case): the Jacobian kernel runs in backward, in vector-Jacobian form, and
                # writes g * d value / d (parameters, T, p) straight into the gradient arrays
                ctx.save_for_backward(par, T, rho_vl) if P is None else ctx.save_for_backward(par, T, rho_vl, P)
            else:
                jac = native.pure_jacobian(which, comp.gather(par), comp.gather(T), None if P is None else comp.gather(P), rho_vl,
                                           polish=(which == "vapor_pressure"))
                ctx.save_for_backward(jac)
            ctx.comp = comp
            ctx.which = which
        ctx.needs = needs
        ctx.in_devices = tuple(None if x is None else x.device for x in (parameters, temperature, pressure))
        return (*_shell.finish(ctx, parameters.device, [value], r["status"]), comp)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_value, _g_nans, _g_plan):
        comp = ctx.comp
        if comp.all_ok:
            par, T, rho_vl, *rest = ctx.saved_tensors
            grads = native.pure_jacobian_vjp(ctx.which, par, T, rest[0] if rest else None, rho_vl,
                                             g_value.to(comp.device).contiguous(), ctx.needs, polish=(ctx.which == "vapor_pressure"))
            return (None, *(None if g is None else g.to(dev) for g, dev in zip(grads, ctx.in_devices)))
        (jac,) = ctx.saved_tensors
        return (None, *_shell.scatter(comp, jac, g_value, _COLUMNS, ctx.needs, ctx.in_devices))


class _PureDerivatives(torch.autograd.Function):
    """(a, p, dp) = derivatives(parameters[n,8], temperature[n], density[n]) with the reference's autograd behaviour
    (feos_torch/pcsaft_pure.py:106-182 are torch graphs): gradients to parameters, temperature and density."""

    @staticmethod
    def forward(ctx, parameters, temperature, density):
        dev = native._device_of(parameters)
        saved = (native._prep(parameters, dev, (8,)), native._prep(temperature, dev), native._prep(density, dev))
        return _shell.save_state(ctx, (parameters, temperature, density), saved, native.pure_derivatives(*saved))

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        if all(g is None for g in grads):
            return None, None, None
        pieces = native.pure_derivatives_vjp(*ctx.saved_tensors, *grads)
        return tuple(g.to(dev) if need else None for g, dev, need in zip(pieces, ctx.in_devices, ctx.needs_input_grad))


class _PureCritical(torch.autograd.Function):
    """t_c[n_ok], p_c[n_ok], rho_c[n_ok], nans[n], plan = critical_point(parameters[n,8], initial temperature[n] or None)

    One solve, one compaction plan (its 4-byte count is the call's only host synchronisation); the backward pass is the
    implicit-function kernel on the converged rows (pcs_pure_critical_point_vjp), dropped rows receive zero gradient."""

    @staticmethod
    def forward(ctx, parameters, initial_temperature):
        dev = native._device_of(parameters)
        par = native._prep(parameters, dev, (8,))
        t0 = None if initial_temperature is None else native._prep(initial_temperature, dev)
        r = native.pure_critical_point(par, t0)
        comp = native.Compaction(r["status"])
        tc, pc, rhoc = comp.gather(r["t_c"]), comp.gather(r["p_c"]), comp.gather(r["rho_c"])
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(comp.gather(par), tc, rhoc)
            ctx.comp = comp
        ctx.set_materialize_grads(False)
        ctx.in_device = parameters.device
        return (*_shell.finish(ctx, parameters.device, [tc, pc, rhoc], r["status"]), comp)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_tc, g_pc, g_rhoc, _g_nans, _g_plan):
        if g_tc is None and g_pc is None and g_rhoc is None:
            return None, None
        par, tc, rhoc = ctx.saved_tensors
        comp = ctx.comp
        if comp.n_ok == 0:
            return torch.zeros((comp.n, 8), dtype=torch.float64, device=ctx.in_device), None
        on = lambda g: None if g is None else g.to(comp.device).contiguous()
        gp = native.pure_critical_point_vjp(par, tc, rhoc, on(g_tc), on(g_pc), on(g_rhoc))
        if not comp.all_ok:
            gp = comp.expand(gp)
        return gp.to(ctx.in_device), None


class _PureEnthalpy(torch.autograd.Function):
    """dh[n_ok], nans[n], plan = enthalpy_of_vaporization(parameters[n,8], temperature[n])

    One solve, one compaction plan (its 4-byte count is the call's only host synchronisation); the backward pass is the
    implicit-function kernel on the converged rows (pcs_pure_enthalpy_of_vaporization_vjp), dropped rows receive zero gradient."""

    @staticmethod
    def forward(ctx, parameters, temperature):
        dev = native._device_of(parameters)
        par = native._prep(parameters, dev, (8,))
        T = native._prep(temperature, dev)
        needs = tuple(ctx.needs_input_grad[0:2])
        r = native.pure_enthalpy_of_vaporization(par, T, want_rho_vl=any(needs))
        comp = native.Compaction(r["status"])
        dh = comp.gather(r["dh"])
        if any(needs):
            ctx.save_for_backward(comp.gather(par), comp.gather(T), comp.gather(r["rho_vl"]))
            ctx.comp = comp
        ctx.needs = needs
        ctx.set_materialize_grads(False)
        ctx.in_devices = (parameters.device, temperature.device)
        return (*_shell.finish(ctx, parameters.device, [dh], r["status"]), comp)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_dh, _g_nans, _g_plan):
        if g_dh is None or not any(ctx.needs):
            return None, None
        par, T, rho_vl = ctx.saved_tensors
        comp = ctx.comp
        shapes = ((comp.n, 8), (comp.n,))
        if comp.n_ok == 0:
            return tuple(torch.zeros(s, dtype=torch.float64, device=d) if need else None
                         for s, d, need in zip(shapes, ctx.in_devices, ctx.needs))
        grads = native.pure_enthalpy_of_vaporization_vjp(par, T, rho_vl, g_dh.to(comp.device).contiguous(), ctx.needs)
        if not comp.all_ok:
            grads = [None if g is None else comp.expand(g) for g in grads]
        return tuple(None if g is None else g.to(d) for g, d in zip(grads, ctx.in_devices))


class PcSaftPure(_shell.Reducible):
    def __init__(self, parameters):
        """parameters: [N, 8] float64 — m, sigma, epsilon_k, mu, kappa_ab, epsilon_k_ab, na, nb
        (feos_torch/pcsaft_pure.py:90-104, README.md:12)."""
        if parameters.dim() != 2 or parameters.shape[1] != 8:
            raise ValueError("parameters must have shape [N, 8]")
        self._par = parameters

    # attribute views of the reference (:91-104), computed on access: the kernels read the [N,8] array itself, and
    # `mu2` alone is six strided passes over it (0.6 ms per 1e7 rows on every construction and every `reduce` if eager)
    m = property(lambda self: self._par[:, 0])
    sigma = property(lambda self: self._par[:, 1])
    epsilon_k = property(lambda self: self._par[:, 2])
    kappa_ab = property(lambda self: self._par[:, 4])
    epsilon_k_ab = property(lambda self: self._par[:, 5])
    na = property(lambda self: self._par[:, 6])
    nb = property(lambda self: self._par[:, 7])

    @property
    def mu2(self):
        """mu^2 / (m sigma^3 epsilon_k) * 1e-19 / k_B (:94-99)."""
        p = self._par
        return p[:, 3] ** 2 / (p[:, 0] * p[:, 1] ** 3 * p[:, 2]) * 1e-19 * (1.0 / 1.380649e-23)

    @property
    def parameters(self):
        """numpy copy of the (current, possibly reduced) parameter rows (:104)."""
        return self._par.detach().cpu().numpy()

    # -- state functions -------------------------------------------------------------------
    def helmholtz_energy(self, temperature, density):
        """Reduced residual Helmholtz energy density a(T, rho) [A^-3] (:106-178); differentiable w.r.t. parameters,
        temperature and density like the reference's torch graph."""
        return self.derivatives(temperature, density)[0]

    def derivatives(self, temperature, density):
        """(a, p, dp/drho), all reduced (:180-182); differentiable (pcs_pure_derivatives_vjp is the backward pass)."""
        temperature = torch.as_tensor(temperature, dtype=torch.float64)
        density = torch.as_tensor(density, dtype=torch.float64)
        return _PureDerivatives.apply(self._par, temperature, density)

    # -- properties ------------------------------------------------------------------------
    def _property(self, which, temperature, pressure):
        value, nans, comp = _PureProperty.apply(which, self._par, temperature, pressure)
        self._reduce(comp)
        return nans, value

    def liquid_density(self, temperature, pressure):
        """(nans, rho [kmol/m3]) at (T [K], p [Pa]) (:184-199)."""
        return self._property("liquid_density", temperature, pressure)

    def vapor_pressure(self, temperature):
        """(nans, p_sat [Pa]) at T [K] (:201-215)."""
        return self._property("vapor_pressure", temperature, None)

    def equilibrium_liquid_density(self, temperature):
        """(nans, saturated liquid density [kmol/m3]) at T [K] (:217-233)."""
        return self._property("equilibrium_liquid_density", temperature, None)

    def critical_point(self, initial_temperature=None):
        """(nans, T_c [K], p_c [Pa], rho_c [kmol/m3]): the vapour-liquid critical point of every row (the end of the region in
        which `vapor_pressure` has an answer), values for the converged rows only, differentiable w.r.t. the parameters.
        `vapor_pressure` answers on every row up to 0.999 T_c and on a shrinking share above.
        initial_temperature [N] (optional): where the search for T_c starts.  Not part of the reference's class."""
        if initial_temperature is not None:
            initial_temperature = torch.as_tensor(initial_temperature, dtype=torch.float64)
        t_c, p_c, rho_c, nans, comp = _PureCritical.apply(self._par, initial_temperature)
        self._reduce(comp)
        return nans, t_c, p_c, rho_c

    def boiling_temperature(self, pressure, initial_temperature=None):
        """(nans, T [K]): the temperature at which every row boils at `pressure` [Pa], i.e. p_sat(T) = pressure -- the inverse
        of `vapor_pressure`, solved in one kernel (csrc/pure_boiling.hpp).  Values for the converged rows only; a row fails when
        its pressure is not below its critical pressure (or on the last 0.05 % of the saturation line below it, where part of
        the rows fail), non-positive or non-finite.  Differentiable w.r.t. the parameters and the pressure (implicit-function
        theorem on the vapour-pressure Jacobian: dT/dp = 1 / (dp_sat/dT)).
        initial_temperature [N] (optional): first iterate of the search; it receives no gradient.
        Not part of the reference's class."""
        pressure = torch.as_tensor(pressure, dtype=torch.float64)
        if initial_temperature is not None:
            initial_temperature = torch.as_tensor(initial_temperature, dtype=torch.float64)
        return self._property("boiling_temperature", initial_temperature, pressure)

    def enthalpy_of_vaporization(self, temperature):
        """(nans, dh_vap [kJ/mol]) at T [K]: dh_vap = T (v_V - v_L) dp_sat/dT at the saturated densities of T, solved and
        evaluated in one kernel (csrc/pure_enthalpy.hpp).  Values for the converged rows only; a row fails where `vapor_pressure`
        fails: every T >= T_c (and part of the rows on the last 0.05 % of the saturation line below it), a
        temperature that is non-positive or non-finite.  Differentiable w.r.t. the parameters and the temperature ALONG the
        saturation line: the response of both saturated densities is carried (implicit-function theorem on equal pressure and
        chemical potential), since dh_vap, unlike p_sat, is not stationary in them.
        Not part of the reference's class."""
        temperature = torch.as_tensor(temperature, dtype=torch.float64)
        dh, nans, comp = _PureEnthalpy.apply(self._par, temperature)
        self._reduce(comp)
        return nans, dh

    def _reduce(self, comp):  # `reduce(nans)` (:235-243) is _shell.Reducible's
        if not comp.all_ok:
            self._par = native.compact_rows(comp, self._par)
