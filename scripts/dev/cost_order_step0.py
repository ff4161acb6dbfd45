"""Go / no-go of a row order keyed on what the fp32 pre-solve does, in ONE process at 1e7 bench rows.
pcs_pure_order_key of the built library gives, per row, the pre-solve's counts, flags and decision margins; candidate keys
(class-major inside 16384-row tiles, at most 64 sub-keys per class) are formed from them HERE, sorted into orders, and
  * the waves of k_pure_vle_ordered (64 consecutive positions) are formed on the host side of the arrays: liquid-root
    evaluations, coupled iterations, full liquid / vapour evaluations in a coupled iteration >= 2 that a wave executes;
  * pcs_pure_vle_fast_ordered is timed with each order, alternating as ab_ordered.py does (the kernel only reads order[]:
    what a device-built order of the same key would cost), against scratch/ab/lib_parent.so, its copy lib_copy.so and the
    parent's own (class, tau bin) order.
Every key is taken twice: from the batch's own parameters, and from PERTURBED parameters (m, sigma, eps each scaled by an
independent U[0.95, 1.05], seed 77: a fit that has moved) applied to the unperturbed rows.  Second batch: the bench
parameters at tau ~ U[0.70, 0.80] (seed 78).  Usage: cost_order_step0.py [--out FILE.json]"""
import ctypes, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))); sys.path.insert(0, ROOT); os.chdir(ROOT)
import numpy as np, torch
from feos_torch_amd.synthetic import pure_batch
from feos_torch_amd import _lib
out = sys.argv[2] if len(sys.argv) > 2 and sys.argv[1] == "--out" else None
ALT, LAUNCHES = int(os.environ.get("PCS_AB_ALT", "7")), int(os.environ.get("PCS_AB_LAUNCHES", "100"))
n = int(os.environ.get("PCS_AB_ROWS", "10000000"))
R = 16384
P, T = pure_batch(n)
rng = np.random.default_rng(77)
P2 = P.copy(); P2[:, :3] *= rng.uniform(0.95, 1.05, (n, 3))
T3 = P[:, 2] * 1.28 * P[:, 0] ** 0.45 * np.random.default_rng(78).uniform(0.70, 0.80, n)
Pd, P2d, Td, T3d = (torch.from_numpy(x).cuda() for x in (P, P2, T, T3))
vp = ctypes.c_void_p
new = _lib.lib()
def plain(path):
    L = ctypes.CDLL(os.path.abspath(path))
    L.pcs_pure_vle_fast.argtypes = [vp, vp, ctypes.c_int64] + [vp] * 7
    L.pcs_pure_row_order.argtypes = [vp, vp, ctypes.c_int64, vp, vp]
    return L
parent, copy = plain("scratch/ab/lib_parent.so"), plain("scratch/ab/lib_copy.so")
stream = vp(torch.cuda.current_stream().cuda_stream)
polar, assoc = Pd[:, 3] != 0, (Pd[:, 4] != 0) & ((Pd[:, 6] != 0) | (Pd[:, 7] != 0))
cls = torch.where(polar, torch.where(assoc, 2, 1), torch.where(assoc, 3, 0)).to(torch.int64)
tile = torch.arange(n, device="cuda") // R

def probe(Pt, Tt):
    key = torch.empty(n, dtype=torch.int32, device="cuda"); raw = torch.empty((n, 4), dtype=torch.int32, device="cuda")
    assert new.pcs_pure_order_key(vp(Pt.data_ptr()), vp(Tt.data_ptr()), n, vp(key.data_ptr()), vp(raw.data_ptr()), stream) == 0, new.pcs_last_error()
    torch.cuda.synchronize()
    w = raw[:, 0].to(torch.int64) & 0xFFFFFFFF
    m = raw[:, 1:].contiguous().view(torch.float32)
    tau = (Tt / (1.28 * Pt[:, 2] * Pt[:, 0] ** 0.45)).float()
    return {"nl": w & 0xFF, "nc": (w >> 8) & 0xFF, "code": (w >> 16) & 0xFF, "re": (w >> 24) & 1, "fv": (w >> 25) & 1, "ok": (w >> 31) & 1,
            "mq": m[:, 0], "ml": m[:, 1], "mv": m[:, 2], "tau": tau, "key": key.to(torch.int64)}

def qlog(m, w, nb):  # nb (even) equal bins of log2(m) over [-w, w]: the threshold m = 1 is an edge
    lg = torch.log2(m.clamp(min=1e-30, max=1e30))
    return ((lg + w) / (2 * w) * nb).floor().clamp(0, nb - 1).to(torch.int64)
def lex(major, nmaj, minor, nmin):  # minor runs backwards in every other major bin: neighbours across a major edge stay alike
    return major * nmin + torch.where(major % 2 == 1, nmin - 1 - minor, minor)
def taubin(f, nb):
    lo, hi = 0.55, 0.90
    return ((f["tau"] - lo) / (hi - lo) * nb).floor().clamp(0, nb - 1).to(torch.int64)
mc = lambda f: torch.maximum(f["ml"], f["mv"])
CANDIDATES = {
    "b: counts, coupled major": lambda f: (f["nc"] - 2).clamp(0, 3) * 8 + (f["nl"] - 2).clamp(0, 7),
    "b: counts, liquid major": lambda f: lex((f["nl"] - 2).clamp(0, 7), 8, (f["nc"] - 2).clamp(0, 3), 4),
    "c: counts + 8 tau bins": lambda f: lex((f["nc"] - 2).clamp(0, 3) * 2 + (f["nl"] >= 3), 8, taubin(f, 8), 8),
    "c: decisions + 16 tau bins": lambda f: lex(2 * (f["nl"] >= 3) + ((f["nc"] >= 3) ^ (f["nl"] >= 3)), 4, taubin(f, 16), 16),
    "d: margins w=6, liquid 2 x coupled 32": lambda f: lex(qlog(f["mq"], 6, 2), 2, qlog(mc(f), 6, 32), 32),
    "d: margins w=6, liquid 4 x coupled 16": lambda f: lex(qlog(f["mq"], 6, 4), 4, qlog(mc(f), 6, 16), 16),
    "d: margins w=4, liquid 4 x coupled 16": lambda f: lex(qlog(f["mq"], 4, 4), 4, qlog(mc(f), 4, 16), 16),
    "d: margins w=2, liquid 4 x coupled 16": lambda f: lex(qlog(f["mq"], 2, 4), 4, qlog(mc(f), 2, 16), 16),
    "d: margins w=4, liquid 8 x coupled 8": lambda f: lex(qlog(f["mq"], 4, 8), 8, qlog(mc(f), 4, 8), 8),
    "d: margins w=4, coupled 16 x liquid 4": lambda f: lex(qlog(mc(f), 4, 16), 16, qlog(f["mq"], 4, 4), 4),
    "d: coupled margin only, w=6, 64 bins": lambda f: qlog(mc(f), 6, 64),
    "d: liquid 2 x vapour 8 x liquid-side 4 (w=4)": lambda f: lex(lex(qlog(f["mq"], 4, 2), 2, qlog(f["mv"], 4, 8), 8), 16, qlog(f["ml"], 4, 4), 4),
    "e: margins w=4 liquid 4 x coupled 8 x 2 tau": lambda f: lex(lex(qlog(f["mq"], 4, 4), 4, qlog(mc(f), 4, 8), 8), 32, taubin(f, 2), 2),
}
def order_of(sub, f):
    sub = torch.where(f["ok"] == 1, sub.clamp(0, 63), torch.full_like(sub, 63))
    return torch.argsort(tile * 256 + cls * 64 + sub, stable=True).to(torch.int32)
def tau_order(Pt, Tt):
    o = torch.empty(n, dtype=torch.int32, device="cuda")
    assert parent.pcs_pure_row_order(vp(Pt.data_ptr()), vp(Tt.data_ptr()), n, vp(o.data_ptr()), stream) == 0
    torch.cuda.synchronize()
    return o
def wave_stats(o, f):
    k = n // 64 * 64
    w = lambda x: x[o.long()[:k]].reshape(-1, 64)
    nl, nc = w(f["nl"]).max(dim=1).values, w(f["nc"]).max(dim=1).values
    return {"liquid_root_evals_per_wave": float(nl.double().mean()), "coupled_iterations_per_wave": float(nc.double().mean()),
            "waves_with_full_liquid_eval_in_iteration_ge_2": float(w(f["re"]).max(dim=1).values.double().mean()),
            "waves_with_full_vapour_eval_in_iteration_ge_2": float(w(f["fv"]).max(dim=1).values.double().mean()),
            "waves_with_3rd_liquid_eval": float((nl >= 3).double().mean()), "waves_with_3rd_coupled_iteration": float((nc >= 3).double().mean())}

res = {"rows": n, "alternations": ALT, "launches_per_block": LAUNCHES, "batches": {}}
p = torch.empty(n, dtype=torch.float64, device="cuda"); st = torch.empty(n, dtype=torch.uint8, device="cuda")
ws = torch.empty(n + 64, dtype=torch.int32, device="cuda")
for bname, Tt in (("bench", Td), ("tau 0.70-0.80", T3d)):
    own, per = probe(Pd, Tt), probe(P2d, Tt)
    args = (vp(Pd.data_ptr()), vp(Tt.data_ptr()), n, vp(p.data_ptr()), None, None, vp(st.data_ptr()), None, vp(ws.data_ptr()))
    lane = {"liquid_root_evals": float(own["nl"].double().mean()), "coupled_iterations": float(own["nc"].double().mean()),
            "lanes_with_3rd_liquid_eval": float((own["nl"] >= 3).double().mean()), "lanes_with_3rd_coupled_iteration": float((own["nc"] >= 3).double().mean()),
            "lanes_full_liquid_eval_ge_2": float(own["re"].double().mean()), "lanes_full_vapour_eval_ge_2": float(own["fv"].double().mean()),
            "unusable_rows": int((own["ok"] == 0).sum()),
            "decision_flips_under_perturbation": {"3rd_liquid_eval": float(((own["nl"] >= 3) != (per["nl"] >= 3)).double().mean()),
                                                   "3rd_coupled_iteration": float(((own["nc"] >= 3) != (per["nc"] >= 3)).double().mean())},
            "log2_margin_quantiles_1_10_50_90_99": {k: [float(x) for x in torch.quantile(torch.log2(own[k].clamp(1e-30, 1e30))[::97].double(), torch.tensor([0.01, 0.1, 0.5, 0.9, 0.99], dtype=torch.float64, device="cuda"))] for k in ("mq", "ml", "mv")},
            "margin_below_1_agrees_with_count": {"liquid": float(((own["mq"] <= 1) == (own["nl"] <= 2))[own["ok"] == 1].double().mean()),
                                                 "coupled": float(((mc(own) <= 1) == (own["nc"] <= 2))[own["ok"] == 1].double().mean())}}
    print(bname, "per lane", json.dumps(lane), flush=True)
    orders = {"a: parent's (class, 8 tau bins) order | own": tau_order(Pd, Tt), "a: parent's (class, 8 tau bins) order | perturbed": tau_order(P2d, Tt)}
    for nm, fn in CANDIDATES.items():
        orders[nm + " | own"] = order_of(fn(own), own)
        orders[nm + " | perturbed"] = order_of(fn(per), per)
    orders["device key of the built library | own"] = order_of(own["key"] % 64, own)
    orders["device key of the built library | perturbed"] = order_of(per["key"] % 64, per)
    orders["identity"] = torch.arange(n, dtype=torch.int32, device="cuda")
    stats = {nm: wave_stats(o, own) for nm, o in orders.items()}
    for nm, s_ in stats.items(): print(f"{nm:66s} liq {s_['liquid_root_evals_per_wave']:.3f} cpl {s_['coupled_iterations_per_wave']:.3f} re {s_['waves_with_full_liquid_eval_in_iteration_ge_2']:.3f} fv {s_['waves_with_full_vapour_eval_in_iteration_ge_2']:.3f}", flush=True)
    def ordered_call(o): return lambda: new.pcs_pure_vle_fast_ordered(*args, vp(o.data_ptr()), stream)
    configs = {"parent, plain entry": lambda: parent.pcs_pure_vle_fast(*args, stream), "parent (copy), plain entry": lambda: copy.pcs_pure_vle_fast(*args, stream)}
    configs.update({nm: ordered_call(o) for nm, o in orders.items()})
    ref, check = None, {}
    for nm, call in configs.items():
        p.zero_(); st.fill_(7)
        assert call() == 0
        torch.cuda.synchronize()
        cur = (p.clone(), st.clone(), int(ws[0].item()))
        if ref is None: ref = cur
        check[nm] = {"p_sat_bits_differing": int((cur[0].view(torch.int64) != ref[0].view(torch.int64)).sum()), "status_differing": int((cur[1] != ref[1]).sum()), "list_entries": cur[2]}
        assert check[nm]["p_sat_bits_differing"] == 0 and check[nm]["status_differing"] == 0 and cur[2] == ref[2], (nm, check[nm])
    names = list(configs)
    times = {nm: [] for nm in names}
    for alt in range(ALT + 1):
        for nm in (names if alt % 2 == 0 else names[::-1]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(LAUNCHES): configs[nm]()
            e1.record(); torch.cuda.synchronize()
            if alt >= 1: times[nm].append(e0.elapsed_time(e1) / LAUNCHES)
    base = float(np.median(times["a: parent's (class, 8 tau bins) order | own"]))
    b = {"per_lane": lane, "configs": {}}
    for nm in names:
        t = np.array(times[nm])
        b["configs"][nm] = dict(check[nm], **stats.get(nm, {}), median_ms=float(np.median(t)), min_ms=float(t.min()), max_ms=float(t.max()),
                                ratio_parent_own_order_over_this=base / float(np.median(t)))
        print(f"{nm:66s} median {np.median(t):.4f} ms  range {t.min():.4f} .. {t.max():.4f}  x{base / np.median(t):.4f}", flush=True)
    res["batches"][bname] = b
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        json.dump(res, open(out, "w"), indent=1)
