"""
Reader for the reference's dataset files: a pandas-style JSON whose ``structure`` column holds pymatgen
``Structure.as_dict()`` records and whose other columns hold the targets (the reference loads it with
``pd.read_json`` + ``Structure.from_dict``, dataset/structure_scalar_tensor.py:229-243).  pymatgen and pandas are not
needed: only the lattice matrix, the Cartesian site coordinates and the element of each (ordered) site are used.
A pymatgen ``Molecule.as_dict()`` record (sites without a ``lattice``) is read as an open structure.
"""
import json
from typing import Dict, List

import numpy as np

_SYMBOLS = (
    "H He Li Be B C N O F Ne Na Mg Al Si P S Cl Ar K Ca Sc Ti V Cr Mn Fe Co Ni Cu Zn Ga Ge As Se Br Kr Rb Sr Y Zr Nb Mo "
    "Tc Ru Rh Pd Ag Cd In Sn Sb Te I Xe Cs Ba La Ce Pr Nd Pm Sm Eu Gd Tb Dy Ho Er Tm Yb Lu Hf Ta W Re Os Ir Pt Au Hg Tl "
    "Pb Bi Po At Rn Fr Ra Ac Th Pa U Np Pu Am Cm Bk Cf Es Fm Md No Lr Rf Db Sg Bh Hs Mt Ds Rg Cn Nh Fl Mc Lv Ts Og"
).split()
ATOMIC_NUMBER = {sym: z for z, sym in enumerate(_SYMBOLS, start=1)}


def structures_from_json(path: str, target_columns=("elastic_tensor_full",),
                         honor_lattice_pbc: bool = False, bool_columns=()) -> List[Dict[str, np.ndarray]]:
    """-> one dict per row, in row order: lattice [3,3], cart_coords [n,3], atomic_numbers [n] (+ the target columns
    that are present).  These dicts are what ``matten_amd.predict.predict`` accepts in place of pymatgen structures.

    ``bool_columns``: columns of true / false flags (the per-atom ``atom_selector`` of the reference's
    datasets/si_nmr_data.json), read as ``bool`` arrays; a value that is not a flag is a ``ValueError`` naming the row.

    A ``Molecule`` record has no lattice: its dict has none either and carries ``pbc = (False, False, False)``.  A
    ``Structure`` record is fully periodic, as in the reference (``from_pymatgen`` ignores ``lattice.pbc``), unless
    ``honor_lattice_pbc`` asks for the flags the record stores."""
    with open(path) as f:
        table = json.load(f)
    rows = sorted(table["structure"], key=int)
    out = []
    for r in rows:
        rec = table["structure"][r]
        sites = rec["sites"]
        if any(len(site["species"]) != 1 for site in sites):
            raise ValueError(f"row {r}: disordered sites are not supported")
        item = {
            "cart_coords": np.asarray([site["xyz"] for site in sites], dtype=np.float64).reshape(-1, 3),
            "atomic_numbers": np.asarray([ATOMIC_NUMBER[site["species"][0]["element"]] for site in sites], dtype=np.int64),
        }
        if rec.get("lattice") is None:
            item["pbc"] = (False, False, False)
        else:
            item = {"lattice": np.asarray(rec["lattice"]["matrix"], dtype=np.float64), **item}
            if honor_lattice_pbc and "pbc" in rec["lattice"]:
                item["pbc"] = tuple(bool(p) for p in rec["lattice"]["pbc"])
        for col in target_columns:
            if col in table:
                item[col] = np.asarray(table[col][r], dtype=np.float64)
        for col in bool_columns:
            if col in table:
                flags = np.asarray(table[col][r])
                if flags.dtype != np.bool_ and not (flags.dtype.kind in "iu" and np.isin(flags, (0, 1)).all()):
                    raise ValueError(f"row {r}: column '{col}' holds values that are not true / false flags")
                item[col] = flags.astype(np.bool_).reshape(-1)
        out.append(item)
    return out
