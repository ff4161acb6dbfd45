"""GPU: the pure-component kernels along the whole saturation line, theta = T / T_c from 0.45 to 1.03.

The grid (tests/tools/saturation_grid.py): 800 parameter rows of all four classes at every theta of SUB (the oracle solves
all of them, tests/test_saturation_grid.py) and of SUPER (no equilibrium exists), 12,000 rows as ONE batch, in two row
orders: theta-major (whole waves at one theta) and interleaved (a wave mixes 0.45 ... 1.03 and all classes).

  a. values of every forward variant against the long-double oracle: p_sat at the project's rel 1e-10 on every sub-critical
     row; the densities at max(1e-10, 10 x the oracle's own fp64-vs-long-double discrepancy at that theta);
  b. failure masks: every row up to theta = 0.999 solved and every super-critical row flagged, by every VLE variant
     (liquid_density: the oracle's mask and values above T_c, where a dense root exists); at 0.9995
     and 0.9999 the VLE variants do not solve every row yet (SOLVE_ALL_THETA), the solved share is printed;
  c. never wrong: a row reported solved is finite, positive, rho_V < rho_c < rho_L, p_sat < p_c, rho_eq > rho_c;
  d. which pass did the work (printed), run_fast + run_retry == run bit for bit, unsolved rows == the robust work list;
  e. schedule independence: both row orders and the prefixes 1, 63, 64, 65, 257 give bit-identical rows;
  f. gradients: the plain Jacobian against the oracle's exact gradient at the same densities, the vector-Jacobian kernel
     against gout * Jacobian bit for bit, both autograd routes of PcSaftPure (every row solved; rows dropped, on the whole
     sub-critical grid) against the direct calls, and the polished vapour-pressure gradient against the exact gradient at the oracle's long-double root.
"""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import saturation_grid as sg  # noqa: E402

pytestmark = pytest.mark.gpu

RHO_UNIT = 1e3 * 6.02214076e23 * 1e-30  # kmol/m3 per A^-3 is 1 / RHO_UNIT
P_BAR = 1e-10            # the project's bar for properties (tests/test_large_parity_gpu.py)
VP_GRAD_BAR = 1e-12      # tests/test_pure_gpu.py::test_jacobian_vs_oracle
RHO_GRAD_BAR = 1e-8
VLE_VARIANTS = ("vle_p", "vp_rho", "vle", "vle_fp64", "vle_eq", "api_vp", "api_eq")
LIQ_VARIANTS = ("liq_psat", "liq_pc", "api_liq_psat", "api_liq_pc")
ORDERS = ("theta-major", "interleaved")
# The highest theta at which every VLE variant solves every row.  Measured on the MI355X, identical for all seven VLE
# variants and both row orders: 800/800 up to 0.999, 617/800 at 0.9995 (non-polar 134/181, polar 160/193, associating
# 160/222, polar + associating 163/204), 285/800 at 0.9999 (57/181, 77/193, 76/222, 75/204); from theta = 0.95 upward every
# row is solved by the robust pass, which is the pass that gives these rows up.  The oracle solves them all, so this is a
# limit of the robust pass (README), not of the grid: above SOLVE_ALL_THETA the tests assert that a row
# reported solved is never wrong (test_solved_rows_are_never_wrong) and within its bar, and print the share.
SOLVE_ALL_THETA = 0.999


def _dense(nans, val):
    out = torch.zeros(nans.shape[0], dtype=torch.float64, device=val.device)
    out[~nans] = val
    return out


def run_variant(name, P, T, p_psat, p_pc):
    """-> dict of dense GPU tensors: status (True = failed) and what the variant returns of p_sat [Pa], rho_v, rho_l [A^-3],
    rho_eq [kmol/m3], rho [kmol/m3] (liquid_density), root [A^-3]."""
    from feos_torch_amd import PcSaftPure, native

    def vle(r):
        out = {"status": r["status"]}
        if r["p_sat"] is not None:
            out["p_sat"] = r["p_sat"]
        if r["rho_eq"] is not None:
            out["rho_eq"] = r["rho_eq"]
        if r["rho_vl"] is not None:
            out["rho_v"], out["rho_l"] = r["rho_vl"][:, 0].clone(), r["rho_vl"][:, 1].clone()
        return out

    if name == "vle_p":
        return vle(native.pure_vle(P, T, want_rho_vl=False))
    if name == "vp_rho":
        return vle(native.pure_vapor_pressure(P, T, want_rho_vl=True))
    if name == "vle":
        return vle(native.pure_vle(P, T))
    if name == "vle_fp64":
        return vle(native.pure_vle(P, T, all_fp64=True))
    if name == "vle_eq":
        return vle(native.pure_vle(P, T, want_p=False, want_rho_eq=True))
    if name in ("liq_psat", "liq_pc"):
        r = native.pure_liquid_density(P, T, p_psat if name == "liq_psat" else p_pc)
        return {"status": r["status"], "rho": r["rho"], "root": r["rho_root"]}
    if name == "api_vp":
        nans, v = PcSaftPure(P).vapor_pressure(T)
        return {"status": nans, "p_sat": _dense(nans, v)}
    if name == "api_eq":
        nans, v = PcSaftPure(P).equilibrium_liquid_density(T)
        return {"status": nans, "rho_eq": _dense(nans, v)}
    if name in ("api_liq_psat", "api_liq_pc"):
        nans, v = PcSaftPure(P).liquid_density(T, p_psat if name == "api_liq_psat" else p_pc)
        return {"status": nans, "rho": _dense(nans, v)}
    raise KeyError(name)


class Ctx:
    pass


@pytest.fixture(scope="module")
def ctx(oracle, hip_lib):
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    c = Ctx()
    c.g = sg.grid(orc=oracle)
    c.ref = sg.reference(orc=oracle)
    c.n = len(c.g.T)
    c.perm = sg.interleave(c.n)
    c.sub = sg.sub_mask(c.g)
    c.cls = sg.classes(c.g.P)
    dev = torch.device("cuda")
    c.dev = dev
    c.inputs = {}
    for order in ORDERS:
        idx = np.arange(c.n) if order == "theta-major" else c.perm
        c.inputs[order] = tuple(torch.from_numpy(np.ascontiguousarray(x[idx])).to(dev)
                                for x in (c.g.P, c.g.T, c.ref["p_psat"], c.ref["p_pc"]))
    c.res = {order: {v: run_variant(v, *c.inputs[order]) for v in VLE_VARIANTS + LIQ_VARIANTS} for order in ORDERS}
    torch.cuda.synchronize()
    return c


def _major(c, order, x):
    """numpy, in theta-major row order."""
    x = x.cpu().numpy()
    if order == "theta-major":
        return x
    out = np.empty_like(x)
    out[c.perm] = x
    return out


def _want(c, key, variant):
    ld = c.ref["ld"]
    if key == "p_sat":
        return ld["p_sat"], "p_sat"
    if key in ("rho_v", "rho_l", "rho_eq"):
        return ld[key], key
    case = "psat" if variant.endswith("psat") else "pc"
    return ld[("rho_" if key == "rho" else "root_") + case], "rho_" + case


def _bar(c, cond_key, th):
    return P_BAR if cond_key == "p_sat" else sg.bar(c.ref["cond"][cond_key], th)


# ------------------------------------------------------------------------------------------------------------------------
# a. values
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
def test_values_against_the_long_double_oracle(ctx, order):
    c = ctx
    bad = []
    for variant in VLE_VARIANTS + LIQ_VARIANTS:
        r = c.res[order][variant]
        st = _major(c, order, r["status"])
        for key in ("p_sat", "rho_v", "rho_l", "rho_eq", "rho", "root"):
            if key not in r:
                continue
            got = _major(c, order, r[key])
            want, cond_key = _want(c, key, variant)
            for th, sl in sg.theta_slices(c.g):
                if th > 1.0 and variant in VLE_VARIANTS:
                    continue  # no equilibrium; liquid_density has a dense root above T_c too and is compared there as well
                ok = ~st[sl]
                err = np.abs(got[sl][ok] / want[sl][ok] - 1.0)
                e = float(err.max()) if len(err) else 0.0
                bar = _bar(c, cond_key, th)
                print("values %-11s %-12s %-6s theta %-7g bar %.2e measured %.2e solved %d/%d %s"
                      % (order, variant, key, th, bar, e, ok.sum(), len(ok), "" if e <= bar else "EXCEEDED"))
                if not e <= bar:
                    bad.append((variant, key, th, e, bar))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------------------
# b. failure masks
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
def test_failure_masks(ctx, order):
    """Every variant solves every row up to SOLVE_ALL_THETA (liquid_density: every sub-critical row) and flags every
    super-critical row of all four classes; in between the solved share per theta, class and variant is printed.
    liquid_density has a dense root above T_c too (the oracle returns it): its mask is clean below T_c and equals the
    long-double oracle's above (the values there are compared in test_values_against_the_long_double_oracle)."""
    c = ctx
    bad = []
    for variant in VLE_VARIANTS + LIQ_VARIANTS:
        st = _major(c, order, c.res[order][variant]["status"])
        for th, sl in sg.theta_slices(c.g):
            s, cl = st[sl], c.cls[sl]
            share = " ".join("%s %d/%d" % (sg.CLASS_NAMES[k], (~s[cl == k]).sum(), (cl == k).sum()) for k in range(4))
            print("solved %-11s %-12s theta %-7g %5d/%d  %s" % (order, variant, th, (~s).sum(), len(s), share))
            if (th <= SOLVE_ALL_THETA or (th < 1.0 and variant in LIQ_VARIANTS)) and s.any():
                bad.append((variant, th, "unsolved", int(s.sum())))
            if th > 1.0 and variant in VLE_VARIANTS and not s.all():
                bad.append((variant, th, "reported solved above T_c", int((~s).sum())))
            if th > 1.0 and variant in LIQ_VARIANTS:
                want = c.ref["ld"]["st_psat" if variant.endswith("psat") else "st_pc"][sl]
                if not np.array_equal(s.astype(bool), want):
                    bad.append((variant, th, "mask differs from the oracle's above T_c", int((s.astype(bool) != want).sum())))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------------------
# c. never wrong
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
def test_solved_rows_are_never_wrong(ctx, order):
    """On every row reported solved, at any theta: finite, positive, rho_V < rho_c < rho_L, p_sat < p_c, rho_eq > rho_c (a
    converged trivial root rho_V = rho_L fails the ordering); liquid_density > rho_c below T_c."""
    c, g = ctx, ctx.g
    bad = []
    for variant in VLE_VARIANTS + LIQ_VARIANTS:
        r = c.res[order][variant]
        ok = ~_major(c, order, r["status"])
        for key in r:
            if key == "status":
                continue
            x = _major(c, order, r[key])[ok]
            if not (np.isfinite(x).all() and (x > 0).all()):
                bad.append((variant, key, "not finite and positive"))
        get = lambda key: _major(c, order, r[key])
        if "p_sat" in r and not (get("p_sat")[ok] < g.pc[ok]).all():
            bad.append((variant, "p_sat >= p_c", g.theta[ok][get("p_sat")[ok] >= g.pc[ok]]))
        if "rho_v" in r and not ((get("rho_v")[ok] < g.rhoc_red[ok]) & (g.rhoc_red[ok] < get("rho_l")[ok])).all():
            wrong = ~((get("rho_v")[ok] < g.rhoc_red[ok]) & (g.rhoc_red[ok] < get("rho_l")[ok]))
            bad.append((variant, "not rho_V < rho_c < rho_L", g.theta[ok][wrong]))
        if "rho_eq" in r and not (get("rho_eq")[ok] > g.rhoc[ok]).all():
            bad.append((variant, "rho_eq <= rho_c", g.theta[ok][get("rho_eq")[ok] <= g.rhoc[ok]]))
        if "rho" in r and not (get("rho")[ok & c.sub] > g.rhoc[ok & c.sub]).all():
            bad.append((variant, "liquid density <= rho_c below T_c"))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------------------
# d. which pass did the work
# ------------------------------------------------------------------------------------------------------------------------
PLAN_KINDS = ({}, {"want_rho_vl": True}, {"want_rho_eq": True, "want_rho_vl": True})


def _work_list(plan):
    cnt = int(plan.ws[0].item())
    entries = plan.ws[1:1 + cnt].cpu().numpy()
    return entries.view(np.uint32) & np.uint32(0x7FFFFFFF), entries < 0  # row, bit 31 (solved by the fp64 fallback kernel)


def test_pass_shares_per_theta(ctx):
    from feos_torch_amd import native

    c = ctx
    P, T, _, _ = c.inputs["theta-major"]
    for kind in PLAN_KINDS:
        plan = native.PureVlePlan(c.n, c.dev, **kind)
        plan.run_fast(P, T)
        torch.cuda.synchronize()
        rows, fb = _work_list(plan)
        assert plan.retry_count() == (int(fb.sum()), int((~fb).sum()))
        for k, (th, sl) in enumerate(sg.theta_slices(c.g)):
            here = rows // sg.N_ROWS == k
            print("passes %-44s theta %-7g main %4d fallback %4d robust %4d" % (
                kind or "pressure only", th, sg.N_ROWS - here.sum(), (here & fb).sum(), (here & ~fb).sum()))


@pytest.mark.parametrize("kind", PLAN_KINDS, ids=["p", "rho_vl", "rho_eq"])
def test_fast_plus_retry_is_run_on_the_near_critical_rows(ctx, kind):
    """theta >= 0.99 alone as a batch (the fallback and robust passes' real customers): run_fast + run_retry == run bit
    for bit, and the rows run_fast leaves unsolved are exactly the entries of the work list the robust pass will take."""
    from feos_torch_amd import native

    c = ctx
    P, T, _, _ = c.inputs["interleaved"]
    near = torch.from_numpy(c.g.theta[c.perm] >= 0.99).to(c.dev)
    P, T = P[near].contiguous(), T[near].contiguous()
    n = T.shape[0]
    assert n == 9 * sg.N_ROWS
    outs = lambda pl: [t for t in (pl.p_sat, pl.rho_eq, pl.rho_vl, pl.status) if t is not None]
    whole = native.PureVlePlan(n, c.dev, **kind)
    for t in outs(whole):
        t.zero_()
    whole.run(P, T)
    torch.cuda.synchronize()
    plan = native.PureVlePlan(n, c.dev, **kind)
    for t in outs(plan):
        t.zero_()
    plan.run_fast(P, T)
    torch.cuda.synchronize()
    rows, fb = _work_list(plan)
    assert len(np.unique(rows)) == len(rows) and (rows < n).all()
    unsolved = np.flatnonzero(plan.status.cpu().numpy() != 0)
    assert np.array_equal(unsolved, np.sort(rows[~fb]))
    assert len(rows[~fb]) >= 4 * sg.N_ROWS  # at least the super-critical rows
    plan.run_retry(P, T)
    torch.cuda.synchronize()
    for got, want in zip(outs(plan), outs(whole)):
        assert torch.equal(got.view(torch.uint8), want.view(torch.uint8))


# ------------------------------------------------------------------------------------------------------------------------
# e. schedule independence
# ------------------------------------------------------------------------------------------------------------------------
_INT_OF_SIZE = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _same_bits(a, b):
    """Equal bit patterns.  Compared as integers of the element's own size: such a view needs no unit stride, which a
    one-row slice of a column (a prefix of n = 1) does not have even after .contiguous()."""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    return torch.equal(a.view(_INT_OF_SIZE[a.element_size()]), b.view(_INT_OF_SIZE[b.element_size()]))


def test_row_order_does_not_change_a_bit(ctx):
    c = ctx
    perm = torch.from_numpy(c.perm).to(c.dev)
    bad = []
    for variant in VLE_VARIANTS + LIQ_VARIANTS:
        a, b = c.res["theta-major"][variant], c.res["interleaved"][variant]
        for key in a:
            if not _same_bits(a[key][perm], b[key]):
                diff = (a[key][perm] != b[key]).cpu().numpy()
                bad.append((variant, key, int(diff.sum()), sorted(set(c.g.theta[c.perm][diff]))))
    assert not bad, bad


@pytest.mark.parametrize("n", sg.PREFIXES)
def test_prefixes_of_the_interleaved_order(ctx, n):
    c = ctx
    part_in = tuple(x[:n].contiguous() for x in c.inputs["interleaved"])
    bad = []
    for variant in VLE_VARIANTS + LIQ_VARIANTS:
        part, full = run_variant(variant, *part_in), c.res["interleaved"][variant]
        for key in full:
            if not _same_bits(part[key], full[key][:n]):
                bad.append((variant, key))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------------------------
# f. gradients
# ------------------------------------------------------------------------------------------------------------------------
def _grad_err(got, want):
    return np.abs(got - want).max(axis=1) / np.abs(want).max(axis=1)


def _jac_inputs(c, prop):
    """(which, P, T, p or None, rho_vl [n,2], solved) in theta-major order, densities as the property's own forward leaves
    them: the lite + polish densities for the vapour pressure, the rho_eq route's for the equilibrium liquid density."""
    P, T, p_psat, p_pc = c.inputs["theta-major"]
    res = c.res["theta-major"]
    if prop == "vapor_pressure":
        r = res["vp_rho"]
        return prop, P, T, None, torch.stack([r["rho_v"], r["rho_l"]], dim=1), ~r["status"]
    if prop == "equilibrium_liquid_density":
        r = res["vle_eq"]
        return prop, P, T, None, torch.stack([r["rho_v"], r["rho_l"]], dim=1), ~r["status"]
    r = res["liq_psat" if prop == "liquid_density_psat" else "liq_pc"]
    return ("liquid_density", P, T, p_psat if prop == "liquid_density_psat" else p_pc,
            torch.stack([torch.zeros_like(r["root"]), r["root"]], dim=1), ~r["status"])


JAC_PROPS = ("vapor_pressure", "equilibrium_liquid_density", "liquid_density_psat", "liquid_density_pc")


@pytest.mark.parametrize("prop", JAC_PROPS)
def test_plain_jacobian_against_the_exact_gradient_at_the_same_densities(ctx, oracle, prop):
    from feos_torch_amd import native

    c, g = ctx, ctx.g
    which, P, T, p, rho_vl, ok = _jac_inputs(c, prop)
    if prop == "vapor_pressure":  # plain = no polish step: the converged densities of the default pure_vle
        r = c.res["theta-major"]["vle"]
        rho_vl, ok = torch.stack([r["rho_v"], r["rho_l"]], dim=1), ~r["status"]
    ok = ok.cpu().numpy() & c.sub
    J = native.pure_jacobian(which, P, T, p, rho_vl).cpu().numpy()
    rho = rho_vl.cpu().numpy()
    safe = lambda x, f: np.where(ok, x, f * g.rhoc_red)
    _, want = oracle.pure_property_grad(which, g.P, g.T, None if p is None else p.cpu().numpy(), safe(rho[:, 0], 0.5),
                                        safe(rho[:, 1], 2.0), exact=True)
    bar = VP_GRAD_BAR if prop == "vapor_pressure" else RHO_GRAD_BAR
    bad = []
    for th, sl in sg.theta_slices(g):
        if th > 1.0:
            continue
        e = _grad_err(J[sl][ok[sl]], want[sl][ok[sl]])
        e = float(e.max()) if len(e) else 0.0
        print("jacobian %-28s theta %-7g bar %.1e measured %.2e rows %d" % (prop, th, bar, e, ok[sl].sum()))
        if not e <= bar:
            bad.append((th, e))
    assert not bad, bad


@pytest.mark.parametrize("prop", JAC_PROPS)
def test_vjp_kernel_is_the_jacobian_kernel_with_another_store(ctx, prop):
    """pcs_pure_jacobian_vjp (the backward pass whenever every row converged) == gout[:, None] * pcs_pure_jacobian, bit for
    bit, for every `need` combination and the polish flag both ways."""
    from feos_torch_amd import native

    c = ctx
    which, P, T, p, rho_vl, ok = _jac_inputs(c, prop)
    ok = ok & torch.from_numpy(c.sub).to(c.dev)
    P, T, rho_vl = P[ok].contiguous(), T[ok].contiguous(), rho_vl[ok].contiguous()
    p = None if p is None else p[ok].contiguous()
    n = T.shape[0]
    assert n >= 9 * sg.N_ROWS
    gout = torch.from_numpy(np.random.default_rng(3).normal(size=n)).to(c.dev)
    for polish in (False, True):
        J = native.pure_jacobian(which, P, T, p, rho_vl, polish=polish)
        assert torch.isfinite(J).all()
        want = gout[:, None] * J
        for need in itertools.product((False, True), repeat=3):
            gp, gt, gpr = native.pure_jacobian_vjp(which, P, T, p, rho_vl, gout, need, polish=polish)
            assert (gp is not None) == need[0] and (gt is not None) == need[1]
            assert (gpr is not None) == (need[2] and p is not None)
            if gp is not None:
                assert _same_bits(gp, want[:, :8]), (polish, need)
            if gt is not None:
                assert _same_bits(gt, want[:, 8]), (polish, need)
            if gpr is not None:
                assert _same_bits(gpr, want[:, 9]), (polish, need)


@pytest.mark.parametrize("prop", JAC_PROPS)
def test_autograd_takes_the_vjp_route_on_the_sub_critical_grid(ctx, prop):
    """PcSaftPure with requires_grad on the sub-critical grid alone (the two VLE properties: up to SOLVE_ALL_THETA, beyond
    which rows fail and the call takes the other route): every row converges, so backward is the direct
    pcs_pure_jacobian_vjp call on the forward's own densities; .grad must be exactly that."""
    from feos_torch_amd import PcSaftPure, native

    c = ctx
    top = 1.0 if prop.startswith("liquid_density") else SOLVE_ALL_THETA
    sub = torch.from_numpy(c.g.theta[c.perm] <= top).to(c.dev)
    P, T, p_psat, p_pc = (x[sub].contiguous() for x in c.inputs["interleaved"])
    n = T.shape[0]
    gout = torch.from_numpy(np.random.default_rng(4).normal(size=n)).to(c.dev)
    par, tem = P.clone().requires_grad_(True), T.clone().requires_grad_(True)
    if prop == "vapor_pressure":
        prs = None
        nans, val = PcSaftPure(par).vapor_pressure(tem)
        rho_vl = native.pure_vapor_pressure(P, T, want_rho_vl=True)["rho_vl"]
    elif prop == "equilibrium_liquid_density":
        prs = None
        nans, val = PcSaftPure(par).equilibrium_liquid_density(tem)
        rho_vl = native.pure_vle(P, T, want_p=False, want_rho_eq=True, want_rho_vl=True)["rho_vl"]
    else:
        prs = (p_psat if prop == "liquid_density_psat" else p_pc).clone().requires_grad_(True)
        nans, val = PcSaftPure(par).liquid_density(tem, prs)
        root = native.pure_liquid_density(P, T, prs.detach())["rho_root"]
        rho_vl = torch.stack([torch.zeros_like(root), root], dim=1)
    assert not nans.any().item(), int(nans.sum().item())  # the all_ok route
    val.backward(gout)
    which = "liquid_density" if prs is not None else prop
    gp, gt, gpr = native.pure_jacobian_vjp(which, P, T, None if prs is None else prs.detach(), rho_vl, gout,
                                           (True, True, True), polish=(prop == "vapor_pressure"))
    assert torch.isfinite(gp).all()
    assert _same_bits(par.grad, gp) and _same_bits(tem.grad, gt)
    if prs is not None:
        assert _same_bits(prs.grad, gpr)


@pytest.mark.parametrize("prop", ("vapor_pressure", "equilibrium_liquid_density"))
def test_autograd_with_dropped_rows_on_the_whole_sub_critical_grid(ctx, prop):
    """The other backward route, the one a near-critical batch takes: on the WHOLE sub-critical grid rows above
    SOLVE_ALL_THETA are dropped, so the forward keeps the Jacobian of the solved rows and backward scatters gout * Jacobian
    to their places.  .grad of a solved row must be exactly gout * pcs_pure_jacobian at the forward's own densities, .grad
    of a dropped row exactly zero, and the dropped rows are those the kernel flags."""
    from feos_torch_amd import PcSaftPure, native

    c = ctx
    sub = torch.from_numpy(c.g.theta[c.perm] < 1.0).to(c.dev)
    P, T = (x[sub].contiguous() for x in c.inputs["interleaved"][:2])
    par, tem = P.clone().requires_grad_(True), T.clone().requires_grad_(True)
    if prop == "vapor_pressure":
        nans, val = PcSaftPure(par).vapor_pressure(tem)
        r = native.pure_vapor_pressure(P, T, want_rho_vl=True)
    else:
        nans, val = PcSaftPure(par).equilibrium_liquid_density(tem)
        r = native.pure_vle(P, T, want_p=False, want_rho_eq=True, want_rho_vl=True)
    ok = ~nans
    assert torch.equal(nans, r["status"].bool())
    assert 0 < int(nans.sum().item()) < 2 * sg.N_ROWS  # rows are dropped (not the all_ok route), all of them above 0.999
    assert not nans[torch.from_numpy(c.g.theta[c.perm][c.g.theta[c.perm] < 1.0] <= SOLVE_ALL_THETA).to(c.dev)].any()
    gout = torch.from_numpy(np.random.default_rng(6).normal(size=int(ok.sum().item()))).to(c.dev)
    val.backward(gout)
    J = native.pure_jacobian(prop, P[ok].contiguous(), T[ok].contiguous(), None, r["rho_vl"][ok].contiguous(),
                             polish=(prop == "vapor_pressure"))
    assert torch.isfinite(J).all()
    want = gout[:, None] * J
    assert _same_bits(par.grad[ok], want[:, :8]) and _same_bits(tem.grad[ok], want[:, 8])
    assert not par.grad[nans].any() and not tem.grad[nans].any()


def test_polished_vapour_pressure_gradient_against_the_exact_gradient_at_the_exact_root(ctx):
    """PCS_JAC_POLISH at the densities of pure_vapor_pressure(want_rho_vl=True) against the oracle's exact gradient at ITS
    long-double root.  Bar per theta: max(1e-12, 10 x the change of the oracle's exact gradient between its long-double and
    its fp64 root) -- a reference-only measure of how much a rounding-level density difference moves this gradient."""
    from feos_torch_amd import native

    c, g = ctx, ctx.g
    which, P, T, _, rho_vl, ok = _jac_inputs(c, "vapor_pressure")
    ok = ok.cpu().numpy() & c.sub
    J = native.pure_jacobian(which, P, T, None, rho_vl, polish=True).cpu().numpy()
    want = c.ref["grad"]["vapor_pressure"]
    bad = []
    for th, sl in sg.theta_slices(g):
        if th > 1.0:
            continue
        bar = sg.bar(c.ref["cond"]["grad_vapor_pressure"], th, floor=VP_GRAD_BAR)
        e = _grad_err(J[sl][ok[sl]], want[sl][ok[sl]])
        e = float(e.max()) if len(e) else 0.0
        print("polished vapour-pressure gradient theta %-7g bar %.2e measured %.2e rows %d" % (th, bar, e, ok[sl].sum()))
        if not e <= bar:
            bad.append((th, e, bar))
    assert not bad, bad
