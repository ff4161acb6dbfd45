"""Row set of tests/test_gc_point_grad_gpu.py and of the referee checks in tests/test_oracle_gc.py: the rows of
gc_batch(N, seed=SEED) on which the oracle's long-double bubble (dew) point converges, with the converged densities rho4, seeded
upstream weights w ~ U(0.5, 1.5) and the exact gradients of oracle.gc_bubble_dew_vjp_exact -- per model class and for the whole
set, computed once per session and never modified (every array is read-only).

Model classes: native.gc_class_order's key, 2 * association class + polar, restated here on the oracle's dense encoding so that
the row set can be judged without a GPU.  Association class: 0 = none, 1 = one self-associating molecule, 2 = induced
association (two molecules with sites, one of them self-associating), 3 = two self-associating molecules."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
N, SEED = 720, 2041
TILE = 192  # rows per workgroup of k_gc_segment_gradient<0, 192>, the only block MODE 0 can take
FLOOR = 1e-10  # of the bars max(FLOOR, 10 e): tests/test_mixn_gpu.py
CLASS_NAMES = {0: "none", 1: "none, polar", 2: "self", 3: "self, polar", 4: "induced", 5: "induced, polar", 6: "cross",
               7: "cross, polar"}
_cache = {}


def _freeze(x):
    if isinstance(x, np.ndarray):
        x.setflags(write=False)
    elif isinstance(x, dict):
        for v in x.values():
            _freeze(v)
    elif isinstance(x, (tuple, list)):
        for v in x:
            _freeze(v)
    return x


def table():
    if "table" not in _cache:
        from feos_torch_amd.synthetic import load_segment_table

        _cache["table"] = load_segment_table(os.path.join(ROOT, "tests", "data", "sauer2014_hetero.json"))
    return _cache["table"]


def class_key(seg, counts):
    """[n] 2 * association class + polar of rows with dense segment counts [n,2,S] on the table seg [S,8]: the class part of the
    sort key of native.gc_class_order."""
    per = lambda v: counts @ v  # [n,2] molecule-level sums
    associating = ((per(seg[:, 4]) * per(seg[:, 5])) != 0).sum(axis=1)
    self_assoc = ((per(seg[:, 6]) * per(seg[:, 7])) != 0).sum(axis=1)
    cls = np.zeros(counts.shape[0], dtype=np.int64)
    cls[(associating == 1) & (self_assoc == 1)] = 1
    cls[(associating == 2) & (self_assoc == 1)] = 2
    cls[(associating == 2) & (self_assoc == 2)] = 3
    return 2 * cls + (per(seg[:, 3] ** 2) > 0).any(axis=1)


def batch():
    if "batch" not in _cache:
        from feos_torch_amd.synthetic import gc_batch

        _cache["batch"] = gc_batch(N, table(), seed=SEED)
    return _cache["batch"]


def solved(oracle, dew, n=None, seed=None):
    """The rows of gc_batch(n, seed) the oracle's long-double solver converges, bubble (dew = False) or dew: dict(segs, bonds,
    kab_list, phi, T, x, enc (kept rows), rho4, keep (indices into the batch), dropped (fraction), m, cls [m], w [m])."""
    key = ("solved", bool(dew), n, seed)
    if key not in _cache:
        from feos_torch_amd.synthetic import gc_batch

        b = batch() if n is None else gc_batch(n, table(), seed=seed)
        enc = oracle.gc_encode(table(), b["segment_lists"], b["bond_lists"], b["kab_list"])
        _, rho4, st = oracle.gc_bubble_dew(enc, b["phi"], b["T"], b["x"], b["p_init"], dew, prec=1)
        keep = np.nonzero(~st)[0]
        enc = dict(enc, counts=np.ascontiguousarray(enc["counts"][keep]), bonds=np.ascontiguousarray(enc["bonds"][keep]))
        m = len(keep)
        _cache[key] = _freeze({
            "segs": [b["segment_lists"][k] for k in keep], "bonds": [b["bond_lists"][k] for k in keep], "kab_list": b["kab_list"],
            "pick": b["pick"][keep], "phi": np.ascontiguousarray(b["phi"][keep]), "T": np.ascontiguousarray(b["T"][keep]),
            "x": np.ascontiguousarray(b["x"][keep]), "enc": enc, "rho4": np.ascontiguousarray(rho4[keep]), "keep": keep,
            "dropped": float(st.mean()), "m": m, "cls": class_key(enc["seg"], enc["counts"]),
            "w": np.random.default_rng(SEED + 1 + int(bool(dew))).uniform(0.5, 1.5, m)})
    return _cache[key]


def groups(rows):
    """{name: weight vector [m]}: 'all' and one entry per model class present, w * 1[class]."""
    out = {"all": rows["w"]}
    for c in sorted(set(rows["cls"].tolist())):
        out[CLASS_NAMES[c]] = rows["w"] * (rows["cls"] == c)
    return out


def referee(oracle, dew):
    """{group: dict(value, grad_row, grad_kab, grad_seg, seg_self_error, kab64, row64)} of the row set: the long-double referee
    under the group's weights, and the dual part once more in fp64 (kab64 [S,S], row64 [m,3]) for the bars."""
    key = ("referee", bool(dew))
    if key not in _cache:
        r = solved(oracle, dew)
        out = {}
        for name, w in groups(r).items():
            val, grow, gkab, gseg, err = oracle.gc_bubble_dew_vjp_exact(r["enc"], r["phi"], r["T"], r["rho4"], dew, w)
            _, row64, kab64, _, _ = oracle.gc_bubble_dew_vjp_exact(r["enc"], r["phi"], r["T"], r["rho4"], dew, w, prec=0, segments=False)
            out[name] = {"value": val, "grad_row": grow, "grad_kab": gkab, "grad_seg": gseg, "seg_self_error": err, "kab64": kab64,
                         "row64": row64}
        _cache[key] = _freeze(out)
    return _cache[key]


def kab_records(rows, gkab):
    """The entries of an [S,S] k_ab gradient that belong to the binary segment records of the batch, in their order."""
    ident = rows["enc"]["ident"]
    return np.array([gkab[ident.index(k[0]), ident.index(k[1])] for k in rows["kab_list"]])


def row_error(got, want):
    """{group: [m]} of an [m,3] per-row gradient (phi_0, phi_1, T): largest |got - want| of the group over the largest |want| of
    the group in that row."""
    out = {}
    for name, sl in (("phi", slice(0, 2)), ("T", slice(2, 3))):
        den = np.abs(want[:, sl]).max(axis=1)
        out[name] = np.abs(got[:, sl] - want[:, sl]).max(axis=1) / np.where(den == 0.0, 1.0, den)
    return out


def row_bars(ref):
    """{group: (e [m], bar [m])} from the referee alone: e = its fp64 run against its long-double run."""
    e = row_error(ref["row64"], ref["grad_row"])
    return {g: (e[g], np.maximum(FLOOR, 10.0 * e[g])) for g in e}


def kab_error(rows, got, want):
    """Largest |got - want| over the four k_ab records relative to the largest exact record ([S,S] inputs)."""
    g, w = kab_records(rows, got), kab_records(rows, want)
    return float(np.max(np.abs(g - w)) / np.max(np.abs(w)))


def seg_error(rows, got, want, mask_rows=None):
    """[8] per parameter column: largest |got - want| over the entries the referee reports (used segment, parameter != 0)
    relative to the largest exact entry of the column; NaN for a column without a reported entry.  mask_rows: the rows that
    carry weight (default: all)."""
    seg, counts = rows["enc"]["seg"], rows["enc"]["counts"]
    used = (counts if mask_rows is None else counts[mask_rows]).sum(axis=(0, 1)) > 0
    out = np.full(8, np.nan)
    for k in range(8):
        mask = used & (seg[:, k] != 0.0)
        scale = np.max(np.abs(want[mask, k])) if mask.any() else 0.0
        if scale > 0.0:
            out[k] = np.max(np.abs(got[mask, k] - want[mask, k])) / scale
    return out, used
