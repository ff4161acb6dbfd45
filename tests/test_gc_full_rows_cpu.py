"""CPU: the row builders of tests/tools/gc_full_rows.py (molecules that fill the 8 segment and 8 bond slots of the 80-byte gc row,
segment indices up to 31), the three encoders on their rows, and what the oracle says about them -- everything
tests/test_gc_full_rows_gpu.py relies on, asserted here without a GPU.

Figures of this file (x86-64, 80-bit long double), printed by the tests with -s:
  oracle, aliased rows against plain rows, 700 rows x 3 packing fractions, worst (a, p, mu, v) in the measures of
  tests/test_gc_state_gpu.py:   long double 2.2e-16 1.9e-15 1.2e-15 7.4e-14;   fp64 7.0e-15 6.9e-14 3.8e-14 1.5e-12
  fp64 oracle, bubble: p 1.3e-13, rho4 1.8e-13, dp/dphi 1.6e-14, dp/dT 2.0e-14, folded k_ab records 1.8e-16; dew: 9.6e-14,
  2.4e-13, 3.8e-15, 7.6e-15, 9.7e-18; no row changes its status.
  oracle's long-double solver: alias rows 0 of 700 dropped (bubble and dew); heterogeneous rows 0 of 700 dropped (bubble and
  dew), kept per class key 0..7: 68, 202, 132, 118, 0, 80, 64, 36.

tests/golden/gc_full_rows.json (written by tests/golden/make_golden_gc_full_rows.py) holds helmholtz_energy_density of the
unmodified reference for four heterogeneous rows with both molecules full; the oracle agrees with it to 5.0e-15 in the measure
and at the bar (1e-10) of tests/test_oracle_gc.py's random rows."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
import gc_full_rows as fr  # noqa: E402
import gc_point_rows as gp  # noqa: E402

from feos_torch_amd.gc_pcsaft import _encode_molecule, _encoder, encode_rows, encode_rows_device, encode_rows_py  # noqa: E402

LIBRARY_CLASSES = {0, 1, 2, 3, 5, 6}  # tests/test_gc_point_grad_gpu.py::test_row_set works them out from all library pairs


def _row_sets():
    ar = fr.alias_rows()
    return {"plain": ar["plain"], "aliased": ar["aliased"], "hetero": fr.hetero_rows()}


def _full(names):
    return lambda rows, mols: np.array([[mols[a][0] in names, mols[b][0] in names] for a, b in rows["pick"]])


def test_alias_builder(oracle):
    """The alias table is the 23-row table plus nine exact copies (two CH3, three CH2, one each of OH, NH2, >CH, CH=O) and its
    k_ab records are GC_KAB's on every pair of variants; alias() keeps the molecule (de-aliased it is the plain one, bond list
    untouched); the six molecules of EXTRA reach 8 segment types and 8 bond types, the four library molecules what the nine pads
    admit (6 / 8, 6 / 8, 6 / 6, 6 / 6 -- the module docstring of the builder has the arithmetic); every pad is used; the rows
    reach every class key the library reaches, each with both molecules at 8 / 8 in at least one row or, for induced
    association (only C3IA has the sites), with the full molecule in either place."""
    base, tab = fr.base_table(), fr.alias_table()
    ident = [s for s, _ in tab]
    assert len(tab) == 32 and ident[:23] == [s for s, _ in base] and len(set(ident)) == 32
    par = dict(base)
    copies = {}
    for (orig, pad), (name, v) in zip(fr.PADS, tab[23:]):
        assert name == pad and np.array_equal(v, par[orig])
        copies[orig] = copies.get(orig, 0) + 1
    assert copies == {"CH3": 2, "CH2": 3, "OH": 1, "NH2": 1, ">CH": 1, "CH=O": 1}
    enc = oracle.gc_encode(tab, [], [], fr.kab_list(ident))
    enc0 = oracle.gc_encode(base, [], [], fr.kab_list())
    orig_ix = [[s for s, _ in base].index(fr.original(s)) for s in ident]
    assert np.array_equal(enc["kab"], enc0["kab"][np.ix_(orig_ix, orig_ix)])
    plain, aliased = fr.alias_molecules()
    counts = {}
    for p, a in zip(plain, aliased):
        assert a[0] == p[0] and [fr.original(s) for s in a[1]] == list(p[1]) and a[2] == p[2]
        counts[p[0]] = fr.type_counts(a[1], a[2])
    full = [n for n, c in counts.items() if c == (8, 8)]
    print("\n   aliased molecules (segment types, bond types):", counts)
    assert len(full) >= 6 and set(full) == {m[0] for m in fr.EXTRA}
    assert [counts[n] for n in fr.ALIASED_LIBRARY] == [(6, 8), (6, 8), (6, 6), (6, 6)]
    assert {s for m in aliased for s in m[1]} >= {pad for _, pad in fr.PADS}
    rows = fr.alias_rows()["aliased"]
    assert rows["n"] == fr.N_ROWS == 700 and rows["n"] > 3 * rows["n_pairs"]
    cls = fr.classes(oracle, rows)
    assert np.array_equal(cls, fr.classes(oracle, fr.alias_rows()["plain"]))
    is_full = _full(set(full))(rows, aliased)
    assert set(cls.tolist()) == LIBRARY_CLASSES
    assert set(cls[is_full.all(axis=1)].tolist()) == LIBRARY_CLASSES - {5} and 5 in set(cls[is_full.any(axis=1)].tolist())


def test_hetero_builder(oracle):
    """Pad k of the heterogeneous table is its original with m, sigma, epsilon_k times 1 + 0.02 (k + 1) and the non-zero mu,
    kappa_ab, epsilon_k_ab times 1 + 0.01 (k + 1), na and nb unchanged: no two of the 32 rows are equal.  Nine hand-written molecules
    with exactly 8 segment types and 8 bond types from real and perturbed segments, multiplicities from 1 to 12, a bond between
    two segments of one type at an index >= 23, a pair on the same 8 types; rows = all ordered pairs with four small library
    molecules; classes none, polar only, one and two self-associating molecules and induced association, each with both
    molecules full in some row."""
    base, tab = fr.base_table(), fr.hetero_table()
    ident = [s for s, _ in tab]
    par = dict(base)
    for k, ((orig, pad), (name, v)) in enumerate(zip(fr.PADS, tab[23:])):
        want = par[orig] * np.array([1 + 0.02 * (k + 1)] * 3 + [1 + 0.01 * (k + 1)] * 3 + [1.0, 1.0])
        assert name == pad and np.array_equal(v, want) and np.array_equal(v == 0.0, par[orig] == 0.0)
    assert len({tuple(v) for _, v in tab if tuple(v) != tuple(par["NH2"])}) == 31  # 'IA' shares six numbers with NH2, not eight
    assert len({tuple(v) for _, v in tab}) == 32
    assert len(fr.HETERO) >= 8
    mult, same_type_high = set(), False
    for name, segs, bonds in fr.HETERO:
        assert fr.type_counts(segs, bonds) == (8, 8), name
        assert any(ident.index(s) >= 23 for s in segs) and any(ident.index(s) < 23 for s in segs), name
        mult |= {segs.count(s) for s in set(segs)}
        same_type_high |= any(segs[i] == segs[j] and ident.index(segs[i]) >= 23 for i, j in bonds)
    assert min(mult) == 1 and max(mult) == 12 and same_type_high
    h = {m[0]: m for m in fr.HETERO}
    assert set(h["h3"][1]) == set(h["h3b"][1]) and sorted(h["h3"][1]) != sorted(h["h3b"][1])
    rows, mols = fr.hetero_rows(), fr.hetero_molecules()
    assert rows["n"] == 700 and rows["n_pairs"] == 13 * 13 and [m[0] for m in mols[-4:]] == list(fr.SMALL)
    cls = fr.classes(oracle, rows)
    both_full = _full(set(h))(rows, mols).all(axis=1)
    print("\n   heterogeneous rows per class key 0..7:", np.bincount(cls, minlength=8), " both molecules full:",
          np.bincount(cls[both_full], minlength=8))
    assert {0, 1, 2, 5, 6} <= set(cls[both_full].tolist())  # none, polar only, one self, induced ('IA'), two self
    assert np.any((rows["pick"][:, 0] == 2) & (rows["pick"][:, 1] == 3))  # h3 x h3b: i != j on equal indices


@pytest.mark.parametrize("which", ["plain", "aliased", "hetero"])
def test_encoders_agree_on_full_rows(oracle, which):
    """encode_rows (native), encode_rows_py (specification), the 40-byte molecule table of encode_indices and the rows gathered
    from it agree byte for byte; a full molecule has 8 non-zero segment counts and 8 non-zero bond counts with sorted ids; the
    rows decoded back to dense counts / bond matrices are oracle.gc_encode's (which knows nothing of the 8 slots)."""
    rows = _row_sets()[which]
    ident = [s for s, _ in rows["table"]]
    S = len(ident)
    got = encode_rows(ident, rows["segs"], rows["bonds"])
    assert got.shape == (rows["n"], 80) and got.dtype == np.uint8
    assert np.array_equal(got, encode_rows_py(ident, rows["segs"], rows["bonds"]))
    assert np.array_equal(got, encode_rows_device(ident, rows["segs"], rows["bonds"], "cpu").numpy())
    idx = np.empty((rows["n"], 2), dtype=np.int32)
    tab40 = np.frombuffer(_encoder().encode_indices(ident, rows["segs"], rows["bonds"], idx), dtype=np.uint8).reshape(-1, 40)
    index_of = {s: i for i, s in enumerate(ident)}
    assert idx.min() == 0 and idx.max() == tab40.shape[0] - 1
    for r in range(rows["n"]):
        for c in range(2):
            assert np.array_equal(tab40[idx[r, c]], _encode_molecule(rows["segs"][r][c], rows["bonds"][r][c], index_of)), (r, c)
    enc = fr.encode(oracle, rows)
    counts, bonds = fr.decode(got, S)
    assert np.array_equal(counts, enc["counts"]) and np.array_equal(bonds, enc["bonds"])
    if which == "plain":
        assert got[:, 0:16].max() < 23 and not got[:, 20:24].any() and not got[:, 28:32].any()  # what the suite had so far: 4 slots
        return
    nseg = (got[:, 16:32].reshape(-1, 2, 8) > 0).sum(axis=2)
    nbond = (got[:, 64:80].reshape(-1, 2, 8) > 0).sum(axis=2)
    full = (nseg == 8) & (nbond == 8)
    names = {m[0] for m in (fr.EXTRA if which == "aliased" else fr.HETERO)}
    mols = fr.alias_molecules()[1] if which == "aliased" else fr.hetero_molecules()
    assert np.array_equal(full, _full(names)(rows, mols))
    assert full.all(axis=1).sum() >= 100 and got[:, 0:16].max() == 31
    for c in range(2):
        f = full[:, c]
        ids = got[f, 8 * c:8 * c + 8].astype(int)
        assert np.all(np.diff(ids, axis=1) > 0)  # sorted, distinct
        pair = got[f, 32 + 8 * c:40 + 8 * c].astype(int) * 256 + got[f, 48 + 8 * c:56 + 8 * c].astype(int)
        assert np.all(np.diff(pair, axis=1) > 0) and np.all(got[f, 32 + 8 * c:40 + 8 * c] >= got[f, 48 + 8 * c:56 + 8 * c])


def test_capacity_of_a_row():
    """Exactly 8 segment types with exactly 8 bond types are accepted by all encoders; a ninth segment type or a ninth bond type
    is rejected by all of them."""
    ident = [s for s, _ in fr.hetero_table()]
    name, segs, bonds = fr.HETERO[0]
    small = (["CH3", "CH3"], [[0, 1]])
    ok = encode_rows(ident, [[segs, small[0]]], [[bonds, small[1]]])
    assert (ok[0, 16:24] > 0).all() and (ok[0, 64:72] > 0).all()
    nine_segments = (segs + ["OH"], bonds + [[0, len(segs)]])  # a ninth segment type (and a ninth bond type with it)
    assert fr.type_counts(*nine_segments)[0] == 9
    ring = (segs, bonds + [[0, len(segs) - 1]])  # the same 8 segment types, a ninth bond type CH3-CH3#2
    assert fr.type_counts(*ring) == (8, 9)
    for s, b in (nine_segments, ring):
        for first in (True, False):
            sl, bl = ([[s, small[0]]], [[b, small[1]]]) if first else ([[small[0], s]], [[small[1], b]])
            with pytest.raises(ValueError):
                encode_rows(ident, sl, bl)
            with pytest.raises(ValueError):
                encode_rows_py(ident, sl, bl)
            with pytest.raises(ValueError):
                encode_rows_device(ident, sl, bl, "cpu")


def test_alias_invariance_of_the_oracle(oracle):
    """The oracle on the aliased rows (alias table) against the plain rows (23-row table): an aliased molecule is the plain
    molecule, so only the order of the sums differs.  The long-double values agree to 1e-12 in every measure; the fp64 figures
    are the floor of every alias comparison of tests/test_gc_full_rows_gpu.py (its bars are 10 x these, at least 1e-12), so
    they are held to 1e-10 here: a looser referee would make those bars empty.  Figures: module docstring."""
    nz = fr.alias_noise(oracle)
    print("\n   oracle, aliased against plain (a, p, mu, v): long double", " ".join(f"{e:.1e}" for e in nz["state_ld"]),
          "  fp64", " ".join(f"{e:.1e}" for e in nz["state"]))
    assert (nz["state_ld"] < 1e-12).all() and (nz["state"] < 1e-10).all()
    for name in ("bubble", "dew"):
        d = nz[name]
        print(f"   fp64 oracle, {name}: p {d['p']:.1e} rho4 {d['rho4']:.1e} dp/dphi {d['phi']:.1e} dp/dT {d['T']:.1e} "
              f"k_ab records {d['kab']:.1e}; rows that change status {d['status']}")
        assert d["status"] == 0 and max(d[k] for k in ("p", "rho4", "phi", "T", "kab")) < 1e-10


def test_solver_rows(oracle):
    """What the oracle's long-double solver keeps.  Alias rows: at most 3 % dropped (the cap of tests/test_gc_state_gpu.py) and
    the same rows as plain and as aliased molecules.  Heterogeneous rows: the oracle decides which rows have a bubble / dew
    point; at T = 0.6 x the lower critical-temperature estimate and x ~ U[0.1, 0.9] it keeps at least half (all of them), and
    every class present keeps at least 8 rows."""
    ar = fr.alias_rows()
    print()
    for name, dew in (("bubble", False), ("dew", True)):
        a, p = fr.solved(oracle, ar["aliased"], dew), fr.solved(oracle, ar["plain"], dew)
        assert a["dropped"] <= 0.03 and p["dropped"] <= 0.03 and np.array_equal(a["status"], p["status"])
        h = fr.solved(oracle, fr.hetero_rows(), dew)
        kept = np.bincount(h["cls"], minlength=8)
        present = np.bincount(fr.classes(oracle, fr.hetero_rows()), minlength=8)
        print(f"   {name}: alias rows dropped {100 * a['dropped']:.2f} %; heterogeneous rows kept {h['m']} of 700, per class key 0..7: "
              + ", ".join(map(str, kept)))
        assert h["m"] >= 350 and h["m"] > 3 * gp.TILE and h["m"] % gp.TILE != 0
        assert all(k >= 8 for k, n in zip(kept, present) if n), kept
        assert {0, 1, 2, 3, 5, 6} <= {c for c, k in enumerate(kept) if k}


def test_oracle_against_the_reference_on_full_rows(oracle):
    """tests/golden/gc_full_rows.json: the unmodified reference's helmholtz_energy_density on four heterogeneous rows in which
    both molecules have 8 segment types and 8 bond types (polar only; two self-associating molecules on the same 8 types; two
    self-associating, polar; induced association).  The fixture's rows are the builder's (table, molecules, phi, T, rho equal),
    and the oracle, long double and fp64, agrees with the reference to 1e-10 of max(|a|, 1e-6), the bar of
    tests/test_oracle_gc.py for random library rows."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gc_full_rows.json")) as f:
        g = json.load(f)
    rows = fr.hetero_rows()
    idx = g["row_index"]
    assert len(idx) == 4 and g["identifiers"] == [s for s, _ in rows["table"]]
    assert np.array_equal(np.array(g["table"]), np.stack([v for _, v in rows["table"]]))
    assert g["segment_lists"] == [rows["segs"][i] for i in idx] and g["bond_lists"] == [rows["bonds"][i] for i in idx]
    assert [tuple(k) for k in g["kab_list"]] == [tuple(k) for k in rows["kab_list"]]
    rho = np.array(g["rho"])
    assert np.array_equal(rho, fr.state_points(rows)[idx]) and np.array_equal(np.array(g["phi"]), rows["phi"][idx])
    assert np.array_equal(np.array(g["T"]), rows["T"][idx])
    table = [(s, np.array(v)) for s, v in zip(g["identifiers"], g["table"])]
    enc = oracle.gc_encode(table, g["segment_lists"], g["bond_lists"], [tuple(k) for k in g["kab_list"]])
    assert (enc["counts"] > 0).sum(axis=2).min() == 8 and (enc["bonds"] > 0).sum(axis=(2, 3)).min() == 8
    want = np.array(g["helmholtz_energy_density"])
    for kw in ({"prec": 1}, {"prec": 0, "robust": True}):
        a = oracle.gc_derivatives(enc, np.array(g["phi"]), np.array(g["T"]), rho, **kw)[0]
        err = float(np.max(np.abs(a - want) / np.maximum(1e-6, np.abs(want))))
        print(f"\n   oracle {kw} against the reference: {err:.1e}")
        assert err < 1e-10
