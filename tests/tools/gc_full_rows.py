"""Rows whose molecules fill the later slots of the 80-byte gc row encoding (8 (segment type, count) and 8 (bond type pair, count)
entries per molecule) and carry segment indices up to 31, for tests/test_gc_full_rows_cpu.py and tests/test_gc_full_rows_gpu.py.
Everything here is built once per session and frozen (read-only arrays).

Both tables have S = 32 rows: the 23 segments of tests/data/sauer2014_hetero.json followed by the nine pads of PADS, indices
23 CH3#1, 24 CH3#2, 25 CH2#1, 26 CH2#2, 27 CH2#3, 28 OH#1, 29 NH2#1, 30 >CH#1, 31 CH=O#1.

ALIAS TABLE (alias_table): every pad is an exact copy of its original and kab_list(identifiers) gives every pair of variants the k_ab
of the originals, so an aliased molecule IS the plain molecule; its bubble and dew points are the plain molecule's.
alias(molecule) spreads the occurrences of a segment over the original and its pads.

  How full an aliased molecule can be.  A molecule with c occurrences of a segment that has v variants (itself and its pads) can
  show at most min(c, v) of them, and a molecule with b bonds at most b bond types.  With the nine pads prescribed (two of CH3,
  three of CH2, one each of OH, NH2, >CH, CH=O: they use up all 32 - 23 places) no molecule of gc_molecule_library() gets past
  6 segment types (C10: 2 CH3 + 4 CH2 variants; C6OH: 1 + 4 + 1), and only C9 and C10 have the 8 bonds that 8 bond types need.
  So the library's own molecules reach at most 6 / 8 (C9, C10) and 6 / 6 (C6OH, C6NH2); they are in the row set as such.
  8 / 8 needs a methyl branch on a longer chain.  EXTRA holds six such molecules of the library's homologous series (branched
  alkanes, 1-alcohols, a 1-amine and an aldehyde with one methyl branch, 10 to 12 segments), and alias() brings all six to
  8 segment types and 8 bond types: 6 molecules reach 8 / 8 (asserted in tests/test_gc_full_rows_cpu.py).  Together with the four
  small library molecules of SMALL their ordered pairs reach every class key the library reaches (0, 1, 2, 3, 5, 6).

HETEROGENEOUS TABLE (hetero_table): the same 32 identifiers, pad k (k = 0..8) a perturbed copy of its original: m, sigma,
epsilon_k times 1 + 0.02 (k + 1); mu, kappa_ab, epsilon_k_ab times 1 + 0.01 (k + 1) where non-zero; na, nb unchanged.  No two slots
of a row carry the same numbers, so a kernel that read a neighbouring slot's id or count gives another value (exact aliases
would mask that).  HETERO holds nine hand-written molecules with exactly 8 segment types and 8 bond types each, multiplicities
1 to 12, a bond CH2#2-CH2#2 (index 26 with itself), and the classes none, polar only, self-associating, induced ('IA'); 'h3' and
'h3b' use the same 8 types with other counts.  Rows: all ordered pairs of HETERO + SMALL.
"""
import numpy as np

import gc_point_rows as gp

PADS = (("CH3", "CH3#1"), ("CH3", "CH3#2"), ("CH2", "CH2#1"), ("CH2", "CH2#2"), ("CH2", "CH2#3"), ("OH", "OH#1"), ("NH2", "NH2#1"),
        (">CH", ">CH#1"), ("CH=O", "CH=O#1"))
SMALL = ("C3", "C2OH", "HCOOC2", "C3IA")  # sparse partners: none, self, polar (the only HCOO of the rows), induced
N_ROWS = 700  # two 256-row tiles and a ragged one; three 192-row tiles and a ragged one
_cache = {}
_freeze = gp._freeze


def _mol(*spec):
    """(segments, bonds) of a chain: 'X' the next chain segment, ('X', k) k of them in a row, ['X'] a substituent on the last
    chain segment."""
    segs, bonds, prev = [], [], None
    for t in spec:
        if isinstance(t, list):
            segs.append(t[0])
            bonds.append([prev, len(segs) - 1])
            continue
        name, k = t if isinstance(t, tuple) else (t, 1)
        for _ in range(k):
            segs.append(name)
            if prev is not None:
                bonds.append([prev, len(segs) - 1])
            prev = len(segs) - 1
    return segs, bonds


# one methyl branch next to the chain end, the library's building blocks only
EXTRA = (
    ("2-methylnonane",) + _mol("CH3", ">CH", ["CH3"], ("CH2", 6), "CH3"),
    ("2-methyldecane",) + _mol("CH3", ">CH", ["CH3"], ("CH2", 7), "CH3"),
    ("7-methyloctan-1-ol",) + _mol("CH3", ">CH", ["CH3"], ("CH2", 6), "OH"),
    ("8-methylnonan-1-ol",) + _mol("CH3", ">CH", ["CH3"], ("CH2", 7), "OH"),
    ("7-methyloctan-1-amine",) + _mol("CH3", ">CH", ["CH3"], ("CH2", 6), "NH2"),
    ("8-methylnonanal",) + _mol("CH3", ">CH", ["CH3"], ("CH2", 6), "CH=O"),
)
ALIASED_LIBRARY = ("C9", "C10", "C6OH", "C6NH2")  # as full as the nine pads let them be: 6/8, 6/8, 6/6, 6/6

# every molecule: A - B - C - D x k - E(F) - G - H, eight types and eight bond types
HETERO = (
    ("h1", *_mol("CH3", "CH2", "CH2#1", ("CH2#2", 12), ">CH#1", ["CH3#1"], "CH2#3", "CH3#2")),                  # none, 19 segments
    ("h2", *_mol("CH3#1", ("CH2#1", 3), ">C=O", "CH2#3", ">CH", ["CH3"], "CH2", "CH=O#1")),                    # polar
    ("h3", *_mol("CH3", "CH2", "CH2#1", ("CH2#2", 4), ">CH#1", ["CH3#2"], "CH2#3", "OH#1")),                   # self (OH#1)
    ("h3b", *_mol("CH3#2", "CH2#3", "CH2#2", ("CH2#1", 3), ">CH#1", ["CH3"], "CH2", "OH#1")),                  # self, h3's types
    ("h5", *_mol("CH3#1", "CH2#2", "CH2", ("CH2#3", 5), ">CH", ["CH3#2"], "CH2#1", "NH2#1")),                  # self (NH2#1)
    ("h6", *_mol("CH3", "CH2#1", ">C=O", ("CH2#2", 2), ">CH#1", ["CH3#1"], "CH2#3", "NH2")),                   # self and polar
    ("h7", *_mol("CH3#2", "CH2", "CH2#2", ("CH2#1", 2), ">CH", ["CH3"], "CH2#3", "IA")),                       # acceptor sites only
    ("h8", *_mol("CH3#1", "CH2#3", "CH2#2", ("CH2#1", 2), ">C<", ["CH3"], ["CH3"], "CH2", "CH3#2")),           # none, epsilon_k = 0
    ("h9", *_mol("CH3#2", "CH2#1", "CH2", ("CH2#3", 2), ">CH#1", ["CH3"], "CH2#2", "CH3#1")),                  # none
)


def base_table():
    return gp.table()


def alias_table():
    """[(identifier, array(8))] x 32: the 23-segment table and the nine exact copies of PADS."""
    if "alias_table" not in _cache:
        par = dict(base_table())
        _cache["alias_table"] = list(base_table()) + [(pad, par[orig].copy()) for orig, pad in PADS]
    return _cache["alias_table"]


def hetero_table():
    """[(identifier, array(8))] x 32: pad k perturbed as the module docstring says."""
    if "hetero_table" not in _cache:
        par = dict(base_table())
        out = list(base_table())
        for k, (orig, pad) in enumerate(PADS):
            v = par[orig].copy()
            v[0:3] *= 1.0 + 0.02 * (k + 1)
            v[3:6] *= 1.0 + 0.01 * (k + 1)  # zero entries stay zero
            out.append((pad, v))
        _cache["hetero_table"] = out
    return _cache["hetero_table"]


def variants(segment):
    return [segment] + [pad for orig, pad in PADS if orig == segment]


def original(segment):
    return dict((pad, orig) for orig, pad in PADS).get(segment, segment)


def kab_list(table_identifiers=None):
    """GC_KAB, or, for a table with these identifiers, GC_KAB on every pair of variants of its records that the table holds."""
    from feos_torch_amd.synthetic import GC_KAB

    if table_identifiers is None:
        return list(GC_KAB)
    have = set(table_identifiers)
    return [(a, b, k) for s1, s2, k in GC_KAB for a in variants(s1) for b in variants(s2) if a in have and b in have]


def type_counts(segs, bonds):
    """(distinct segment types, distinct bond types) of a molecule"""
    return len(set(segs)), len({frozenset((segs[i], segs[j])) if segs[i] != segs[j] else (segs[i],) for i, j in bonds})


def alias(molecule):
    """(name, segments, bonds) with the occurrences of every segment spread over the segment and its pads: among 4000 seeded
    random assignments the first with the most segment types (at most 8), then the most bond types (at most 8); a segment that
    occurs once becomes its pad where it has one.  Bonds and the order of the segments are the molecule's."""
    name, segs, bonds = molecule
    rng = np.random.default_rng(sum(map(ord, name)))
    best, best_key = None, (-1, -1)
    cap = min(8, sum(min(segs.count(s), len(variants(s))) for s in set(segs)))
    for _ in range(4000):
        new = [variants(s)[-1] if segs.count(s) == 1 else variants(s)[rng.integers(len(variants(s)))] for s in segs]
        ns, nb = type_counts(new, bonds)
        if ns <= 8 and nb <= 8 and (ns, nb) > best_key:
            best, best_key = new, (ns, nb)
            if best_key == (cap, min(8, len(bonds))):
                break
    assert best is not None, name
    return name, best, bonds


def _library(names):
    from feos_torch_amd.synthetic import gc_molecule_library

    lib = {m[0]: m for m in gc_molecule_library()}
    return [lib[n] for n in names]


def alias_molecules():
    """(plain, aliased): the same 14 molecules -- EXTRA, ALIASED_LIBRARY (both aliased) and SMALL (left as they are)."""
    if "alias_molecules" not in _cache:
        plain = list(EXTRA) + _library(ALIASED_LIBRARY) + _library(SMALL)
        _cache["alias_molecules"] = (plain, [alias(m) for m in plain[:-len(SMALL)]] + plain[-len(SMALL):])
    return _cache["alias_molecules"]


def hetero_molecules():
    return list(HETERO) + _library(SMALL)


def tc_estimate(table, segs):
    """the critical-temperature estimate of synthetic.gc_batch for one molecule"""
    par = dict(table)
    m = np.array([par[s][0] for s in segs])
    e = np.array([par[s][2] for s in segs])
    return (m * e).sum() / m.sum() * 1.28 * m.sum() ** 0.45


def _pairs(mols, n, seed, table):
    """n rows over all ordered pairs of mols (row i is pair i % len(pairs)): lists, names, phi ~ U[0.9, 1.1]^2, T = 0.6 x the
    lower critical-temperature estimate, x ~ U[0.1, 0.9], p_init = 1e5 Pa as synthetic.gc_batch."""
    rng = np.random.default_rng(seed)
    pairs = [(a, b) for a in range(len(mols)) for b in range(len(mols))]
    pick = np.array([pairs[i % len(pairs)] for i in range(n)])
    tc = np.array([tc_estimate(table, m[1]) for m in mols])
    return {"pick": pick, "segs": [[mols[a][1], mols[b][1]] for a, b in pick], "bonds": [[mols[a][2], mols[b][2]] for a, b in pick],
            "phi": rng.uniform(0.9, 1.1, size=(n, 2)), "x": rng.uniform(0.1, 0.9, n), "T": 0.6 * tc[pick].min(axis=1),
            "p_init": np.full(n, 1e5), "n": n, "n_pairs": len(pairs)}


def alias_rows(n=N_ROWS, seed=2051):
    """{"plain", "aliased"}: the same n rows (phi, T, x, p_init identical) as plain molecules on the 23-row table and as aliased
    molecules on the alias table."""
    key = ("alias_rows", n, seed)
    if key not in _cache:
        plain, aliased = alias_molecules()
        p = _pairs(plain, n, seed, base_table())
        a = dict(p, segs=[[aliased[i][1], aliased[j][1]] for i, j in p["pick"]])
        p["table"], p["kab_list"] = base_table(), kab_list()
        a["table"], a["kab_list"] = alias_table(), kab_list([s for s, _ in alias_table()])
        _cache[key] = _freeze({"plain": p, "aliased": a})
    return _cache[key]


def hetero_rows(n=N_ROWS, seed=2052):
    """n rows over the ordered pairs of HETERO + SMALL on the heterogeneous table."""
    key = ("hetero_rows", n, seed)
    if key not in _cache:
        r = _pairs(hetero_molecules(), n, seed, hetero_table())
        r["table"], r["kab_list"] = hetero_table(), kab_list([s for s, _ in hetero_table()])
        _cache[key] = _freeze(r)
    return _cache[key]


def encode(oracle, rows):
    """the oracle's dense encoding of a row set (cached on the set)"""
    key = ("enc", id(rows))
    if key not in _cache:
        _cache[key] = (rows, _freeze(oracle.gc_encode(rows["table"], rows["segs"], rows["bonds"], rows["kab_list"])))
    return _cache[key][1]


def classes(oracle, rows):
    enc = encode(oracle, rows)
    return gp.class_key(enc["seg"], enc["counts"])


ETAS = (1e-3, 0.30, 0.42)
XS = (0.3, 0.7)


def state_points(rows):
    """rho [n,2] of the state-function tests: row i at the packing fraction ETAS[j % 3] of sum_i x_i sum n m sigma^3 and the mole
    fraction XS[j // 3], j = (i // number of pairs + i) % 6 -- every pair meets several of the six, every one of the six is met
    by every molecule."""
    par = dict(rows["table"])
    vol = np.array([[sum(par[s][0] * par[s][1] ** 3 for s in mol) for mol in row] for row in rows["segs"]])  # [n,2]
    i = np.arange(rows["n"])
    j = (i // rows["n_pairs"] + i) % 6
    x = np.array(XS)[j // 3]
    eta = np.array(ETAS)[j % 3]
    xs = np.stack([x, 1.0 - x], axis=1)
    rho = eta / (np.pi / 6.0 * (xs * vol).sum(axis=1))
    return np.ascontiguousarray(xs * rho[:, None])


def solved(oracle, rows, dew):
    """gc_point_rows.solved for a row set of this module: the rows the oracle's long-double solver keeps, their densities, classes
    and seeded weights w ~ U(0.5, 1.5)."""
    key = ("solved", id(rows), bool(dew))
    if key not in _cache:
        enc = encode(oracle, rows)
        p, rho4, st = oracle.gc_bubble_dew(enc, rows["phi"], rows["T"], rows["x"], rows["p_init"], dew, prec=1)
        keep = np.nonzero(~st)[0]
        sub = dict(enc, counts=np.ascontiguousarray(enc["counts"][keep]), bonds=np.ascontiguousarray(enc["bonds"][keep]))
        _cache[key] = (rows, _freeze({
            "segs": [rows["segs"][k] for k in keep], "bonds": [rows["bonds"][k] for k in keep], "kab_list": rows["kab_list"],
            "pick": rows["pick"][keep], "phi": np.ascontiguousarray(rows["phi"][keep]), "T": np.ascontiguousarray(rows["T"][keep]),
            "x": np.ascontiguousarray(rows["x"][keep]), "enc": sub, "rho4": np.ascontiguousarray(rho4[keep]),
            "p": np.ascontiguousarray(p[keep]), "keep": keep, "status": st, "dropped": float(st.mean()), "m": len(keep),
            "cls": gp.class_key(sub["seg"], sub["counts"]),
            "w": np.random.default_rng(2053 + int(bool(dew))).uniform(0.5, 1.5, len(keep))}))
    return _cache[key][1]


def decode(rows80, S):
    """dense counts [n,2,S] and bonds [n,2,S,S] (larger index first) of 80-byte rows"""
    n = rows80.shape[0]
    counts, bonds = np.zeros((n, 2, S)), np.zeros((n, 2, S, S))
    for r in range(n):
        for c in range(2):
            for k in range(8):
                if rows80[r, 16 + 8 * c + k]:
                    counts[r, c, rows80[r, 8 * c + k]] += rows80[r, 16 + 8 * c + k]
                if rows80[r, 64 + 8 * c + k]:
                    bonds[r, c, rows80[r, 32 + 8 * c + k], rows80[r, 48 + 8 * c + k]] += rows80[r, 64 + 8 * c + k]
    return counts, bonds


def fold_matrix(identifiers32, identifiers23):
    """[23,32] 0/1: row a sums the variants of segment a"""
    F = np.zeros((len(identifiers23), len(identifiers32)))
    for j, s in enumerate(identifiers32):
        F[identifiers23.index(original(s)), j] = 1.0
    return F


def state_errors(a, p, mu, v, A, Pp, MU, V, rho):
    """[4] x [n]: the measures of tests/test_gc_state_gpu.py for (a, p, mu, v) against (A, Pp, MU, V)"""
    return (np.abs(a - A) / np.maximum(np.abs(A), 1e-6), np.abs(p - Pp) / np.maximum(np.abs(Pp), rho.sum(axis=1)),
            (np.abs(mu - MU) / np.maximum(1.0, np.abs(MU))).max(axis=1), np.abs(v / V - 1.0).max(axis=1))


def fold_records(rows_plain, gkab32, identifiers32):
    """the entries of an [32,32] k_ab gradient summed over the variants of each record of GC_KAB, in the records' order"""
    ix = identifiers32.index
    return np.array([sum(gkab32[ix(a), ix(b)] for a in variants(s1) for b in variants(s2)) for s1, s2, _ in rows_plain["kab_list"]])


def alias_noise(oracle):
    """How far re-associating the sums moves the ORACLE: its own values on the aliased rows (alias table) against the plain rows
    (23-row table), largest difference per quantity.  Keys: 'state_ld' / 'state' [4] (a, p, mu, v in the measures of
    state_errors, over the three packing fractions; long double / fp64), and per problem ('bubble', 'dew') with the fp64 oracle:
    'p', 'rho4' (relative, rows both runs solve), 'status' (rows on which the two runs disagree), 'phi', 'T' (gc_point_rows.row_error
    of dp/dphi, dp/dT at the long-double densities) and 'kab' (the folded records relative to the largest record)."""
    if "alias_noise" not in _cache:
        ar = alias_rows()
        pl, al = ar["plain"], ar["aliased"]
        ep, ea = encode(oracle, pl), encode(oracle, al)
        rho = state_points(pl)
        out = {}
        for name, kw in (("state_ld", {"prec": 1}), ("state", {"prec": 0, "robust": True})):
            want = oracle.gc_derivatives(ep, pl["phi"], pl["T"], rho, **kw)
            got = oracle.gc_derivatives(ea, al["phi"], al["T"], rho, **kw)
            out[name] = np.array([float(e.max()) for e in state_errors(*got, *want, rho)])
        for name, dew in (("bubble", False), ("dew", True)):
            s = solved(oracle, pl, dew)
            p0, r0, st0 = oracle.gc_bubble_dew(ep, pl["phi"], pl["T"], pl["x"], pl["p_init"], dew, prec=0)
            p1, r1, st1 = oracle.gc_bubble_dew(ea, al["phi"], al["T"], al["x"], al["p_init"], dew, prec=0)
            both = ~st0 & ~st1
            k = s["keep"]
            sub = dict(ea, counts=np.ascontiguousarray(ea["counts"][k]), bonds=np.ascontiguousarray(ea["bonds"][k]))
            _, row0, kab0, _, _ = oracle.gc_bubble_dew_vjp_exact(s["enc"], s["phi"], s["T"], s["rho4"], dew, s["w"], prec=0, segments=False)
            _, row1, kab1, _, _ = oracle.gc_bubble_dew_vjp_exact(sub, s["phi"], s["T"], s["rho4"], dew, s["w"], prec=0, segments=False)
            e = gp.row_error(row1, row0)
            rec0 = gp.kab_records(s, kab0)
            rec1 = fold_records(pl, kab1, ea["ident"])
            out[name] = {"p": float(np.max(np.abs(p1[both] / p0[both] - 1.0))), "rho4": float(np.max(np.abs(r1[both] / r0[both] - 1.0))),
                         "status": int((st0 != st1).sum()), "phi": float(e["phi"].max()), "T": float(e["T"].max()),
                         "kab": float(np.max(np.abs(rec1 - rec0)) / np.max(np.abs(rec0)))}
        _cache["alias_noise"] = out
    return _cache["alias_noise"]


def bar(noise, floor=1e-12):
    """max(floor, 10 x the oracle's own aliased-versus-plain difference): the bar of an alias comparison"""
    return max(floor, 10.0 * float(noise))
