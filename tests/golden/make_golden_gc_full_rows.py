"""Generate gc_full_rows.json: helmholtz_energy_density of the UNMODIFIED reference (GcPcSaftMix) for four heterogeneous rows of
tests/tools/gc_full_rows.py in which both molecules fill all 8 segment and 8 bond slots, at the state points of the GPU tests.
The import recipe (stand-in `si_units` / `feos_torch.feos_torch`, then the reference's package) is make_golden.py's; like it this
never runs on the GPU box and no test imports it.  The JSON holds data only: the 32-row table, the molecules, k_ab records,
phi, T, rho and the reference's values.

Usage:  python3 -B tests/golden/make_golden_gc_full_rows.py
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))

import make_golden as mg  # noqa: E402  (registers the stand-ins and imports the reference)
import gc_full_rows as fr  # noqa: E402

PAIRS = (("h1", "h2"), ("h3", "h3b"), ("h5", "h6"), ("h7", "h3"))  # polar only; two self on equal types; two self, polar; induced


def main():
    rows = fr.hetero_rows()
    names = [m[0] for m in fr.hetero_molecules()]
    pick = [tuple(p) for p in rows["pick"].tolist()]
    idx = [pick.index((names.index(a), names.index(b))) for a, b in PAIRS]
    rho = fr.state_points(rows)[idx]
    table = rows["table"]
    ident = [s for s, _ in table]
    cols = tuple(torch.tensor([float(v[k]) for _, v in table], dtype=mg.f64) for k in range(8))
    segs, bonds = [rows["segs"][i] for i in idx], [rows["bonds"][i] for i in idx]
    eos = mg.GcPcSaftMix(ident, cols, segs, bonds, rows["kab_list"], torch.tensor(rows["phi"][idx], dtype=mg.f64))
    a = eos.helmholtz_energy_density(torch.tensor(rows["T"][idx], dtype=mg.f64), torch.tensor(rho, dtype=mg.f64))
    assert tuple(a.shape) == (len(idx), 1)
    mg.dump("gc_full_rows.json", {
        "pairs": [list(p) for p in PAIRS], "row_index": idx, "identifiers": ident, "table": [v.tolist() for _, v in table],
        "segment_lists": segs, "bond_lists": bonds, "kab_list": [list(k) for k in rows["kab_list"]], "phi": rows["phi"][idx].tolist(),
        "T": rows["T"][idx].tolist(), "rho": rho.tolist(), "helmholtz_energy_density": mg.tl(a[:, 0])})


if __name__ == "__main__":
    main()
