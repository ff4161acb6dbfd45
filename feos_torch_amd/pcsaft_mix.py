"""``PcSaftMix`` — drop-in for the reference class of the same name
(feos_torch/pcsaft_mix.py:12-479) backed by the gfx950 kernels.

Same constructor ``PcSaftMix(parameters[N,2,8], kij[N,2])``, methods ``bubble_point`` /
``dew_point(temperature, molefracs, pressure)`` returning ``(pressure [Pa], nans)`` — note the
tuple order is the opposite of ``PcSaftPure`` in the reference too (:444, :468) — values only
for converged rows, and the model is reduced (mutated) by every property call (:470-479).
Gradients flow to ``parameters``, ``kij`` and ``temperature`` (the reference's final formula
does not depend on the mole fractions or the initial pressure explicitly, so those receive
zero gradient there; here they receive none).
"""
import torch
from torch.autograd.function import once_differentiable

from . import _shell, native
from .native import _detached


_COLUMNS = ((0, 16, (-1, 2, 8)), (16, 2, (-1, 2)), (18, 1, (-1,)))  # parameters, kij, temperature (pressure) in the [n,19] Jacobian (quotient)


def _incipient_molefrac(rho4, dew):
    """y [n]: mole fraction of component 1 in the incipient phase (vapour for bubble, liquid for dew) of rho4 [n,4]"""
    inc = rho4[:, 2:4] if dew else rho4[:, 0:2]
    return inc[:, 0] / (inc[:, 0] + inc[:, 1])


def _weighted(blocks, grads):
    """sum of g[:, None] * block over the upstream gradients that are present (at least one is) -> (Jacobian, g) for
    _shell.scatter: a single block keeps its g for the fused product of the scatter kernel"""
    present = [(b, g.to(b.device)) for b, g in zip(blocks, grads) if g is not None]
    if len(present) == 1:
        return present[0]
    return sum(g[:, None] * b for b, g in present), None


def _outputs(ctx, device, values, status, flags, comp):
    """(value, nans[, stable][, y], plan): _shell.finish, then the incipient composition moved behind the flags"""
    out = _shell.finish(ctx, device, values, status, *flags)
    return (out[0], *out[len(values):], *out[1:len(values)], comp)


def _along_pressure(jac_p, jac_y=None):
    """Blocks [n,19] of (p[, y]) w.r.t. (parameters, kij, T) -> those of (T[, y]) w.r.t. (parameters, kij, p_spec) along the
    line p(theta, T) = p_spec (implicit-function theorem, elementwise on the kept rows): dT/dtheta = -J_p[:, :18] / J_p[:, 18],
    dT/dp_spec = 1 / J_p[:, 18]; dy/dtheta|_p = J_y[:, :18] - J_y[:, 18] J_p[:, :18] / J_p[:, 18], dy/dp_spec = J_y[:, 18] / J_p[:, 18]"""
    inv = 1.0 / jac_p[:, 18:19]
    out = [torch.cat((-jac_p[:, :18] * inv, inv), dim=1)]
    if jac_y is not None:
        dy_dp = jac_y[:, 18:19] * inv
        out.append(torch.cat((jac_y[:, :18] - dy_dp * jac_p[:, :18], dy_dp), dim=1))
    return out


class _BubbleDew(torch.autograd.Function):
    """value[n_ok], nans[n][, stable[n_ok]][, y[n_ok]], plan = bubble / dew pressure at the temperature `given`, or
    (solve_t) bubble / dew temperature at the pressure `given`, in one kernel (csrc/mix_temperature.hip); `start` is the
    initial pressure / the first iterate of the temperature.  Dense solve, one compaction plan (its 4-byte row count is the
    call's only host synchronisation), single-kernel gathers only when rows were dropped (native.Compaction; the reference
    drops them inside the native call, src/pcsaft.rs:216-231).  Gradient to parameters, kij and `given`: pcs_mix_jacobian at
    the solution, for a temperature turned into the quotients of _along_pressure.  incipient: y = mole fraction of component 1
    in the incipient phase, differentiable like the value; the backward pass then takes both Jacobian blocks from ONE
    pcs_mix_point_jacobian call instead of pcs_mix_jacobian."""

    @staticmethod
    def forward(ctx, dew, parameters, kij, given, molefracs, start, check=False, incipient=False, solve_t=False):
        dev = native._device_of(parameters)
        par = native._prep(parameters, dev, (2, 8))
        k = native._prep(kij, dev, (2,))
        known = native._prep(given, dev)
        args = (par, k, known, native._prep(molefracs, dev), native._prep(start, dev), dew)
        r = native.mix_bubble_dew_temperature(*args) if solve_t else native.mix_bubble_dew(*args)
        comp = native.Compaction(r["status"])
        value = comp.gather(r["t" if solve_t else "p"])
        values = [value]
        # the kept rows' model and temperature (the solved one, or the given one), for the Jacobian and the stability check
        kept = lambda: (comp.gather(par), comp.gather(k), value if solve_t else comp.gather(known))
        ctx.needs = list(ctx.needs_input_grad[1:4])
        ctx.incipient = incipient
        blocks = None
        if incipient:
            rho4 = comp.gather(r["rho4"])
            values.append(_incipient_molefrac(rho4, dew))
            ctx.set_materialize_grads(False)  # either upstream gradient may be absent
            if any(ctx.needs):
                blocks = native.mix_point_jacobian(*kept(), rho4, dew)
        elif any(ctx.needs):
            blocks = (native.mix_jacobian(*kept(), comp.gather(r["rho4"]), dew),)
        if blocks is not None:
            ctx.save_for_backward(*(_along_pressure(*blocks) if solve_t else blocks))
            ctx.comp = comp
        ctx.in_devices = (parameters.device, kij.device, given.device)
        flags = ()
        if check:
            flags = (_shell.stable_at_solution(comp, r["rho4"], dew, lambda feed: native.mix_stability(*kept(), feed)),)
        return _outputs(ctx, parameters.device, values, r["status"], flags, comp)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_value, *g_rest):
        if ctx.incipient:
            if g_value is None and g_rest[-2] is None:
                return (None,) * 9
            jac, g = _weighted(ctx.saved_tensors, (g_value, g_rest[-2]))  # outputs: value, nans[, stable], y, plan
        else:
            (jac,), g = ctx.saved_tensors, g_value
        return (None, *_shell.scatter(ctx.comp, jac, g, _COLUMNS, ctx.needs, ctx.in_devices), None, None, None, None, None)


class _MixDensity(torch.autograd.Function):
    """rho [n_ok, kmol/m3], nans [n], plan = liquid (phase 0) / vapour (phase 1) density at (T, p, x) in one kernel
    (csrc/mix_density.hip), compacted like _BubbleDew.  Gradient to all five inputs by the implicit-function theorem on
    p_model(theta, T, rho x) = p [Pa] 1e-30 / (k_B T): ONE pcs_mix_derivatives_vjp call at the root with the per-row weight
    g_p = -g c / (dp/drho) (c = the unit factor), G [n_ok, 21]:
        parameters, kij: G[:, :18];  T: G[:, 18] + g_p p_spec / T (the specified reduced pressure depends on T itself);
        p: -g_p 1e-30 / (k_B T);  x: rho (G[:, 19] - G[:, 20])."""

    COLUMNS = ((0, 16, (-1, 2, 8)), (16, 2, (-1, 2)), (18, 1, (-1,)), (19, 1, (-1,)), (20, 1, (-1,)))  # of the packed gradient [n_ok,21]
    C = 1.0 / (1e3 * (6.02214076e23 * (1e-10 * 1e-10 * 1e-10)))  # A^-3 -> kmol/m3: 1 / RHO_UNIT of csrc/pcsaft_consts.hpp, as PcSaftPure.liquid_density
    P_RED = 1e-30 / 1.380649e-23            # p_spec = p [Pa] P_RED / T

    @staticmethod
    def forward(ctx, phase, parameters, kij, temperature, pressure, molefracs):
        dev = native._device_of(parameters)
        par = native._prep(parameters, dev, (2, 8))
        k = native._prep(kij, dev, (2,))
        T, p, x = native._prep(temperature, dev), native._prep(pressure, dev), native._prep(molefracs, dev)
        r = native.mix_density(par, k, T, p, x, phase)
        comp = native.Compaction(r["status"])
        rho = comp.gather(r["rho"])
        ctx.needs = list(ctx.needs_input_grad[1:6])
        ctx.set_materialize_grads(False)
        if any(ctx.needs):
            x_ok = comp.gather(x)
            ctx.save_for_backward(comp.gather(par), comp.gather(k), comp.gather(T), torch.stack((x_ok * rho, (1.0 - x_ok) * rho), dim=1),
                                  comp.gather(r["dpdrho"]), comp.gather(p))
            ctx.comp = comp
        ctx.in_devices = tuple(t.device for t in (parameters, kij, temperature, pressure, molefracs))
        return (*_shell.finish(ctx, parameters.device, [rho * _MixDensity.C], r["status"]), comp)

    @staticmethod
    @once_differentiable
    def backward(ctx, g, *_):
        if g is None:
            return (None,) * 6
        par, k, T, rho2, dpdrho, p = ctx.saved_tensors
        w = -(g.to(T.device) * _MixDensity.C) / dpdrho  # g_p
        G = native.mix_derivatives_vjp(par, k, T, rho2, g_p=w)
        unit = _MixDensity.P_RED / T
        packed = torch.cat((G[:, :18], (G[:, 18] + w * p * unit / T)[:, None], (-w * unit)[:, None],
                            ((rho2[:, 0] + rho2[:, 1]) * (G[:, 19] - G[:, 20]))[:, None]), dim=1)
        return (None, *_shell.scatter(ctx.comp, packed, None, _MixDensity.COLUMNS, ctx.needs, ctx.in_devices))


class _MixHenry(torch.autograd.Function):
    """H [n_ok, Pa], nans [n], plan = Henry's law constant of component `solute` at infinite dilution in the other, pure and
    saturated, component (the solvent v) in one kernel (csrc/mix_henry.hip), compacted like _BubbleDew.  H = rho_L k_B T
    exp(mu_s(T, rho_v = rho_L, rho_s = 0)), so with gH = g H the gradient to parameters, kij and T is
        explicit part: ONE pcs_mix_derivatives_vjp call at (rho_L, 0) with g_mu = gH on the solute's column, G[:, :19];
        response of rho_L(theta_v, T): ONE pcs_pure_jacobian_vjp call (selector 2, the total derivative of the saturated
            liquid density in kmol/m3) on the solvent's row with gout = gH (1/rho_L + d mu_s/d rho_v) RHO_UNIT, added to the
            solvent's 8 columns and to T -- the weight is the forward kernel's dlnh_drho, so the two calls are independent;
        and gH / T.
    No gradient flows to rho_s."""

    RHO_UNIT = 1e3 * (6.02214076e23 * (1e-10 * 1e-10 * 1e-10))  # kmol/m3 -> A^-3 (csrc/pcsaft_consts.hpp)

    @staticmethod
    def forward(ctx, solute, parameters, kij, temperature):
        dev = native._device_of(parameters)
        par = native._prep(parameters, dev, (2, 8))
        k = native._prep(kij, dev, (2,))
        T = native._prep(temperature, dev)
        r = native.mix_henry(par, k, T, solute)
        comp = native.Compaction(r["status"])
        h = comp.gather(r["h"])
        ctx.needs = list(ctx.needs_input_grad[1:4])
        ctx.set_materialize_grads(False)
        if any(ctx.needs):
            ctx.save_for_backward(comp.gather(par), comp.gather(k), comp.gather(T), comp.gather(r["rho_vl"]), h,
                                  comp.gather(r["dlnh_drho"]))
            ctx.comp = comp
            ctx.solute = solute
        ctx.in_devices = (parameters.device, kij.device, temperature.device)
        return (*_shell.finish(ctx, parameters.device, [h], r["status"]), comp)

    @staticmethod
    @once_differentiable
    def backward(ctx, g, *_):
        if g is None:
            return (None,) * 4
        par, k, T, rho_vl, h, dlnh = ctx.saved_tensors
        s, v = ctx.solute, 1 - ctx.solute
        gh = g.to(T.device) * h
        zero = torch.zeros_like(gh)
        rho2 = torch.stack((zero, rho_vl[:, 1]) if s == 0 else (rho_vl[:, 1], zero), dim=1)
        g_mu = torch.stack((gh, zero) if s == 0 else (zero, gh), dim=1)
        packed = native.mix_derivatives_vjp(par, k, T, rho2, g_mu=g_mu)[:, :19].contiguous()
        g_par, g_T, _ = native.pure_jacobian_vjp("equilibrium_liquid_density", par[:, v, :], T, None, rho_vl,
                                                 gh * dlnh * _MixHenry.RHO_UNIT, need=(True, True, False))
        packed[:, 8 * v:8 * v + 8] += g_par
        packed[:, 18] += g_T + gh / T
        return (None, *_shell.scatter(ctx.comp, packed, None, _COLUMNS, ctx.needs, ctx.in_devices))


class _MixDerivatives(torch.autograd.Function):
    """(a, p, mu, v) = derivatives(parameters[n,2,8], kij[n,2], temperature[n], density[n,2]) with gradients to all four
    inputs (feos_torch/pcsaft_mix.py:31-154, :395-420 are torch graphs in the reference)."""

    COLUMNS = ((0, 16, (-1, 2, 8)), (16, 2, (-1, 2)), (18, 1, (-1,)), (19, 2, (-1, 2)))  # of the packed gradient [n,21]

    @staticmethod
    def forward(ctx, parameters, kij, temperature, density):
        dev = native._device_of(parameters)
        saved = (native._prep(parameters, dev, (2, 8)), native._prep(kij, dev, (2,)), native._prep(temperature, dev),
                 native._prep(density, dev, (2,)))
        return _shell.save_state(ctx, (parameters, kij, temperature, density), saved, native.mix_derivatives(*saved))

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        if all(g is None for g in grads):
            return None, None, None, None
        g = native.mix_derivatives_vjp(*ctx.saved_tensors, *grads)
        return _shell.split(g, _MixDerivatives.COLUMNS, ctx.needs_input_grad, ctx.in_devices)


class _MixnDerivatives(torch.autograd.Function):
    """n-component (a, p, mu, v) with gradients to parameters [n,nc,8], temperature and density [n,nc] (the reference's model is
    a torch graph for any number of components, feos_torch/pcsaft_mix.py:31-154, :395-420)."""

    @staticmethod
    def forward(ctx, parameters, temperature, density):
        dev = native._device_of(parameters)
        nc = int(parameters.shape[1])
        saved = (native._prep(parameters, dev, (nc, 8)), native._prep(temperature, dev), native._prep(density, dev, (nc,)))
        return _shell.save_state(ctx, (parameters, temperature, density), saved, native.mixn_derivatives(*saved))

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        if all(g is None for g in grads):
            return None, None, None
        nc = ctx.saved_tensors[2].shape[1]
        g = native.mixn_derivatives_vjp(*ctx.saved_tensors, *grads)  # [n, 9 nc + 1]
        columns = ((0, 8 * nc, (-1, nc, 8)), (8 * nc, 1, (-1,)), (8 * nc + 1, nc, (-1, nc)))
        return _shell.split(g, columns, ctx.needs_input_grad, ctx.in_devices)


class PcSaftMix(_shell.Reducible):
    def __init__(self, parameters, kij=None):
        """parameters: [N, 2, 8] float64 (component rows as for PcSaftPure); kij: [N, 2] with
        kij[:,0] = k_ij and kij[:,1] = explicit cross-association energy eps_AiBj/k or 0
        (feos_torch/pcsaft_mix.py:13-29; effectively mandatory in the reference, :141/:477)."""
        if parameters.dim() != 3 or parameters.shape[2] != 8:
            raise ValueError("parameters must have shape [N, n, 8]")
        self.ncomp = int(parameters.shape[1])
        if self.ncomp != 2:
            # n-component mixtures (the reference's hs / hc / dispersion / dipole / self-association code is general, :31-154):
            # state functions only, no k_ij (":75-76 kij can only be used for binary mixtures!"), bubble / dew points are binary
            if kij is not None:
                raise Exception("kij can only be used for binary mixtures!")
            if not 1 <= self.ncomp <= 6:
                raise ValueError("between 1 and 6 components are supported")
            if bool((((parameters[:, :, 6] + parameters[:, :, 7]) != 0).sum(dim=1) > 1).any()):
                raise Exception("Only up to two associating components are allowed, and two only for binary mixtures!")
        elif kij is None:
            kij = torch.zeros((parameters.shape[0], 2), dtype=parameters.dtype, device=parameters.device)
        self._set(parameters, kij)

    def _set(self, parameters, kij):
        self._par = parameters
        self.kij = kij

    # attribute views of the reference (:14-29), computed on access (the kernels read the [N,2,8] array itself)
    m = property(lambda self: self._par[:, :, 0])
    sigma = property(lambda self: self._par[:, :, 1])
    epsilon_k = property(lambda self: self._par[:, :, 2])
    kappa_ab = property(lambda self: self._par[:, :, 4])
    epsilon_k_ab = property(lambda self: self._par[:, :, 5])
    na = property(lambda self: self._par[:, :, 6])
    nb = property(lambda self: self._par[:, :, 7])

    @property
    def mu2(self):
        p = self._par
        return p[:, :, 3] ** 2 / (p[:, :, 0] * p[:, :, 1] ** 3 * p[:, :, 2]) * 1e-19 * (1.0 / 1.380649e-23)

    @property
    def parameters(self):
        return self._par.detach().cpu().numpy()

    @property
    def kij_np(self):
        return None if self.kij is None else self.kij.detach().cpu().numpy()

    def helmholtz_energy_density(self, temperature, density):
        """a(T, rho_1, rho_2) [A^-3], shape [N, 1] like the reference (:31-154); differentiable."""
        return self.derivatives(temperature, density)[0][:, None]

    def derivatives(self, temperature, density):
        """(a [N], p [N], mu [N,n], v [N,n]) (:395-420); differentiable w.r.t. parameters, kij, temperature and density
        (pcs_mix_derivatives_vjp / pcs_mixn_derivatives_vjp are the backward passes)."""
        temperature = torch.as_tensor(temperature, dtype=torch.float64)
        density = torch.as_tensor(density, dtype=torch.float64)
        if self.ncomp != 2:
            return _MixnDerivatives.apply(self._par, temperature, density)
        return _MixDerivatives.apply(self._par, self.kij, temperature, density)

    def _point(self, solve_t, dew, given, molefracs, start, check_stability, incipient_molefracs):
        """bubble / dew pressure at the temperature `given`, or (solve_t) temperature at the pressure `given`"""
        if self.ncomp != 2:
            raise Exception("bubble and dew points are implemented for binary mixtures (src/pcsaft.rs:43-79 takes [N,2,8])")
        if solve_t:
            given = torch.as_tensor(given, dtype=torch.float64)
        # the mole fractions do not enter the reference's final formula (:435-444) and the initial pressure / first iterate
        # only starts the search: no gradient flows to either
        *out, comp = _BubbleDew.apply(dew, self._par, self.kij, given, _detached(molefracs), _detached(start),
                                      bool(check_stability), bool(incipient_molefracs), solve_t)
        self._reduce(comp)
        return tuple(out)

    def bubble_point(self, temperature, liquid_molefracs, pressure, check_stability=False, incipient_molefracs=False):
        """(p [Pa], nans) at T [K], liquid mole fraction of component 1, initial pressure [Pa] (:422-444).
        check_stability=True: (p, nans, stable), stable [bool, aligned with p] = the liquid at the solution passed
        stability_analysis (False: a metastable or unstable root, e.g. inside a liquid-liquid split).  p, nans, the gradients
        and the model reduction are those of the default call.
        incipient_molefracs=True: the tuple gains a LAST element y [float64, aligned with p], the mole fraction of component 1
        in the incipient vapour -- (p, nans, y) or (p, nans, stable, y) -- differentiable w.r.t. parameters, kij and
        temperature like p (both gradients from one kernel, pcs_mix_point_jacobian); the other elements are those of the
        default call, bit for bit.  Not part of the reference's class."""
        return self._point(False, False, temperature, liquid_molefracs, pressure, check_stability, incipient_molefracs)

    def dew_point(self, temperature, vapor_molefracs, pressure, check_stability=False, incipient_molefracs=False):
        """(p [Pa], nans) at T [K], vapour mole fraction of component 1, initial pressure [Pa] (:446-468).
        check_stability=True: (p, nans, stable) with the stability of the vapour at the solution (see bubble_point).
        incipient_molefracs=True: a last element x, the mole fraction of component 1 in the incipient liquid (see bubble_point)."""
        return self._point(False, True, temperature, vapor_molefracs, pressure, check_stability, incipient_molefracs)

    def bubble_temperature(self, pressure, liquid_molefracs, temperature, check_stability=False, incipient_molefracs=False):
        """(T [K], nans): the temperature at which the liquid of mole fraction `liquid_molefracs` (component 1) starts to boil
        at `pressure` [Pa], i.e. bubble_point(T, x, .) = pressure, solved in one kernel (csrc/mix_temperature.hpp) from the
        mandatory first iterate `temperature` [K].  Values for the converged rows only, the model is reduced like
        bubble_point does.  Differentiable w.r.t. parameters, kij and pressure (implicit-function theorem on the pressure
        Jacobian: dT/dp = 1 / (dp/dT)); mole fractions and first iterate receive no gradient.  A row fails where no trial
        temperature near the first iterate has an equilibrium, where the pressure lies above the bubble line, or on a branch
        on which the pressure falls with the temperature (include/pcsaft_hip.h, pcs_mix_bubble_dew_temperature).
        check_stability=True: (T, nans, stable) as for bubble_point.  incipient_molefracs=True: a last element y [aligned with
        T], the mole fraction of component 1 in the incipient vapour at the solution, differentiable w.r.t. parameters, kij and
        pressure along the line p(theta, T) = pressure.  Not part of the reference's class."""
        return self._point(True, False, pressure, liquid_molefracs, temperature, check_stability, incipient_molefracs)

    def dew_temperature(self, pressure, vapor_molefracs, temperature, check_stability=False, incipient_molefracs=False):
        """(T [K], nans): the temperature at which the vapour of mole fraction `vapor_molefracs` starts to condense at
        `pressure` [Pa] (see bubble_temperature).  The retrograde dew branch near a mixture critical point is not served:
        such rows fail.  check_stability=True: (T, nans, stable) with the stability of the vapour at the solution.
        incipient_molefracs=True: a last element x, the mole fraction of component 1 in the incipient liquid."""
        return self._point(True, True, pressure, vapor_molefracs, temperature, check_stability, incipient_molefracs)

    def _density(self, phase, temperature, pressure, molefracs):
        if self.ncomp != 2:
            raise Exception("liquid_density and vapor_density are implemented for binary mixtures")
        as64 = lambda t: t if isinstance(t, torch.Tensor) else torch.as_tensor(t, dtype=torch.float64)
        rho, nans, comp = _MixDensity.apply(phase, self._par, self.kij, as64(temperature), as64(pressure), as64(molefracs))
        self._reduce(comp)
        return rho, nans

    def liquid_density(self, temperature, pressure, liquid_molefracs):
        """(rho [kmol/m3], nans): total molar density of the liquid at T [K], p [Pa] and the mole fraction of component 1 --
        the tuple order of this class's bubble_point, (value, nans), not PcSaftPure.liquid_density's.  With eta the packing
        fraction along the composition line: the largest root of p(rho) = p at or below eta = 0.5 that is reached from there
        with dp/drho > 0 throughout, or, where the pressure at eta = 0.5 is below p, the first root above it (eta < 0.74) --
        the liquid root of the bubble-point initialisation, converged to rounding (include/pcsaft_hip.h, pcs_mix_density).
        Values for the converged rows only; the model is reduced like bubble_point does.  A row fails where T, p or x is not
        finite, T <= 0, p <= 0, x outside [0, 1] (x = 0 and x = 1 are valid), or where the liquid branch ends (dp/drho = 0)
        before it reaches p.  Differentiable w.r.t. parameters, kij, temperature, pressure and the mole fractions
        (implicit-function theorem, one pcs_mix_derivatives_vjp call).  Not part of the reference's class."""
        return self._density(0, temperature, pressure, liquid_molefracs)

    def vapor_density(self, temperature, pressure, vapor_molefracs):
        """(rho [kmol/m3], nans): total molar density of the vapour at T [K], p [Pa] and the mole fraction of component 1:
        the smallest root of p(rho) = p, reached from the ideal gas with dp/drho > 0 throughout; a row fails where the
        vapour branch ends below p (and for the invalid inputs of liquid_density).  Tuple order, reduction and gradients as
        for liquid_density."""
        return self._density(1, temperature, pressure, vapor_molefracs)

    def henrys_law_constant(self, temperature, solute=1):
        """(H [Pa], nans): Henry's law constant of component `solute` (index 0 or 1) at infinite dilution in the other
        component, the solvent, at T [K]:  H = lim_{x_s -> 0} f_s / x_s = rho_L k_B T exp(mu_s^res), with rho_L the saturated
        liquid density of the PURE solvent and mu_s^res the solute's residual chemical potential at (rho_solvent = rho_L,
        rho_solute = 0) -- the fugacity-based constant; the K-factor form y p / x differs from it by the solute's
        vapour-phase fugacity coefficient.  One kernel (include/pcsaft_hip.h, pcs_mix_henry).  This class's (value, nans)
        order; values for the solved rows only; the model is reduced like bubble_point does.  A row fails where a parameter
        of either component or kij is invalid, T is not finite and positive, the solvent has no vapour-liquid equilibrium at
        T (T >= T_c of the solvent), or H is not finite and positive; a supercritical solute is an ordinary row.
        Differentiable w.r.t. parameters, kij and temperature (the solvent's saturated density responds to its parameters
        and T: pcs_mix_derivatives_vjp plus pcs_pure_jacobian_vjp, no kernel of its own).  Not part of the reference's class."""
        if self.ncomp != 2:
            raise Exception("henrys_law_constant is implemented for binary mixtures")
        if isinstance(solute, bool) or solute not in (0, 1):
            raise ValueError("solute must be 0 or 1 (component index)")
        temperature = temperature if isinstance(temperature, torch.Tensor) else torch.as_tensor(temperature, dtype=torch.float64)
        h, nans, comp = _MixHenry.apply(int(solute), self._par, self.kij, temperature)
        self._reduce(comp)
        return h, nans

    def stability_analysis(self, temperature, density):
        """Tangent-plane stability of binary feed states at T [K] and partial densities density [N,2] (A^-3) -- the model's
        rows as they are (no reduction, no autograd graph).  -> (stable bool [N], tpd [N] smallest tangent-plane distance found
        [kT per mole of trial phase], trial_density [N,2] its trial phase).  Definitions and the status codes behind `stable`:
        include/pcsaft_hip.h, pcs_mix_stability (tpd = -inf: the feed itself is locally unstable; NaN: invalid feed)."""
        if self.ncomp != 2:
            raise Exception("stability analysis is implemented for binary mixtures only")
        with torch.no_grad():
            temperature = torch.as_tensor(temperature, dtype=torch.float64)
            density = torch.as_tensor(density, dtype=torch.float64)
            r = native.mix_stability(self._par, self.kij, temperature, density)
            out = self._par.device
            return (r["status"] == 0).to(out), r["tpd"].to(out), r["rho_trial"].to(out)

    def _reduce(self, comp):  # `reduce(nans)` (:470-479) is _shell.Reducible's
        if not comp.all_ok:
            self._set(native.compact_rows(comp, self._par), None if self.kij is None else native.compact_rows(comp, self.kij))
