"""
Host tests of the symmetry search (no GPU): the numpy restatement ``find_symmetry_host`` against the table of
tests/spacegroup_cases.py (exact and with noise of symprec / 10), every returned operation checked directly (it maps the
crystal onto itself under the minimum image, independent of the search), the group property, atom orbits, the host twins'
idempotence, and the library's new entries with their argument checks (nothing is launched).
"""
import functools
import os

import numpy as np
import pytest

import spacegroup_cases as sc

NEW_ENTRIES = ("matten_lattice_group", "matten_crystal_symmetry", "matten_irreps_average_atoms")


@functools.lru_cache(maxsize=None)
def host_symmetry(name, noisy=False):
    from matten_amd.symmetry import find_symmetry_host

    return find_symmetry_host(**sc.pack([sc.crystal(name, noisy)]), symprec=sc.SYMPREC)


@pytest.mark.parametrize("noisy", [False, True], ids=["exact", "noisy"])
@pytest.mark.parametrize("name", sc.NAMES)
def test_host_search_reproduces_the_table(name, noisy):
    from matten_amd.symmetry import group_closure

    h = host_symmetry(name, noisy)
    order, n_trans = sc.expected(name)
    assert (int(h.n_rot[0]), int(h.n_trans[0]), int(h.flags[0])) == (order, n_trans, 0)
    cell, pos, Z = sc.crystal(name, noisy)
    c = h.crystals[0]
    assert np.array_equal(c["rotations_int"][0], np.eye(3)) and np.abs(c["translations"][0]).max() == 0.0
    worst = 0.0
    for R, t, src in zip(c["rotations"], c["translations"], c["src"]):
        assert np.abs(R.T @ R - np.eye(3)).max() <= 1e-12
        worst = max(worst, sc.maps_onto_itself(cell, pos, Z, R, t, src))
    for t, src in zip(c["pure_translations"], c["tsrc"]):
        worst = max(worst, sc.maps_onto_itself(cell, pos, Z, np.eye(3), t, src))
    assert worst <= sc.SYMPREC, worst
    assert (h.src[order:] == -1).all() and (h.tsrc[n_trans:] == -1).all()
    # the operations are a group: closing them under multiplication adds nothing
    assert len(group_closure(c["rotations"], tol=1e-3)) == order


def test_lattice_order_and_flags():
    from matten_amd.symmetry import SYM_NOT_FINITE, SYM_RANGE, lattice_group_host

    cells = np.stack([sc.crystal("simple_cubic")[0], sc.RANGE_CELL, np.zeros((3, 3)), sc.crystal("cubic_skew")[0]])
    N, n_lat, flags = lattice_group_host(cells, sc.SYMPREC)
    assert n_lat.tolist() == [48, 1, 1, 48] and flags.tolist() == [0, SYM_RANGE, SYM_NOT_FINITE, 0]
    for b in (0, 3):
        assert np.array_equal(N[b, 0], np.eye(3, dtype=np.int8).reshape(9))
        rest = [tuple(r) for r in N[b, 1:]]
        assert rest == sorted(rest) and len(set(rest)) == 47                      # ascending in the nine entries row-major
        G = cells[b] @ cells[b].T
        for r in N[b]:
            assert np.abs(r.reshape(3, 3) @ G @ r.reshape(3, 3).T - G).max() <= 1e-9
    assert np.array_equal(N[1, 0], np.eye(3, dtype=np.int8).reshape(9)) and not N[1, 1:].any()


def test_equivalent_atoms():
    rutile = host_symmetry("rutile").equivalent_atoms()
    assert rutile.tolist() == [0, 0, 2, 2, 2, 2]                                   # Ti, O
    wurtzite = host_symmetry("wurtzite").equivalent_atoms()
    assert wurtzite.tolist() == [0, 0, 2, 2]                                       # the 6_3 screw axis pairs each species
    assert host_symmetry("fcc_2x2x2").equivalent_atoms().tolist() == [0] * 32
    assert host_symmetry("triclinic_random5").equivalent_atoms().tolist() == [0, 1, 2, 3, 4]


def test_host_flags():
    from matten_amd import symmetry as S

    good = sc.crystal("diamond")
    cell, pos, Z = sc.crystal("wurtzite")
    nan = pos.copy()
    nan[1, 2] = np.nan
    close = (cell, np.concatenate([pos, pos[:1] + 1e-4]), np.concatenate([Z, Z[:1]]))
    crystals = [good, (sc.RANGE_CELL, np.zeros((1, 3)), np.array([13])), good, (cell, nan, Z), close, sc.random_triclinic(1025, 3), good]
    h = S.find_symmetry_host(**sc.pack(crystals))
    assert h.flags.tolist() == [0, S.SYM_RANGE, 0, S.SYM_NOT_FINITE, S.SYM_AMBIGUOUS, S.SYM_TOO_LARGE, 0]
    assert h.n_rot.tolist() == [48, 1, 48, 1, 1, 1, 48] and h.n_trans.tolist() == [4, 1, 4, 1, 1, 1, 4]
    for b in (1, 3, 4, 5):
        lo, hi = h.ptr[b], h.ptr[b + 1]
        assert np.array_equal(h.src[0, lo:hi], np.arange(lo, hi)) and (h.src[1:, lo:hi] == -1).all()
        assert np.array_equal(h.tsrc[0, lo:hi], np.arange(lo, hi)) and (h.tsrc[1:, lo:hi] == -1).all()
    open_axis = S.find_symmetry_host(**sc.pack([good]), pbc=(True, True, False))
    assert open_axis.flags.tolist() == [S.SYM_NOT_PERIODIC] and open_axis.n_rot.tolist() == [1]
    big = sc.fcc_primitive_4x4x4()
    full, cut = S.find_symmetry_host(**sc.pack([big])), S.find_symmetry_host(**sc.pack([big]), max_trans=32)
    assert (full.n_rot[0], full.n_trans[0], full.flags[0]) == (48, 64, 0)
    assert (cut.n_rot[0], cut.n_trans[0], cut.flags[0]) == (48, 64, S.SYM_TRUNC) and cut.tsrc.shape == (32, 64)
    with pytest.raises(ValueError, match="TRUNC|translations"):
        S.CrystalSymmetry.raise_for_flags(_Flags(cut.flags))


class _Flags:
    """what raise_for_flags reads of a CrystalSymmetry"""
    def __init__(self, flags):
        import torch

        self.flags = torch.as_tensor(flags)


def test_host_twins_are_idempotent():
    """projections: a second application changes nothing (1e-12 |x|, fp64)"""
    from matten_amd.symmetry import average_irreps_host, irreps_of, symmetrize_atoms_host

    rng = np.random.default_rng(5)
    for name in ("rutile", "wurtzite", "zincblende"):
        h = host_symmetry(name)
        n = len(h.row_struct)
        for spec in ("ij=ji", "ij", "2x0e+1o+2x2e+1e"):
            x = rng.standard_normal((n, irreps_of(spec).dim))
            once, dev = symmetrize_atoms_host(x, spec, h)
            twice, dev2 = symmetrize_atoms_host(once, spec, h)
            scale = np.linalg.norm(x, axis=1).max()
            assert np.abs(twice - once).max() <= 1e-12 * scale and dev2.max() <= 1e-12 and dev.max() > 1e-3
            labels = h.equivalent_atoms()
            inv = once[:, :1] if spec != "2x0e+1o+2x2e+1e" else once[:, :2]          # scalars agree within an orbit
            for a in np.unique(labels):
                assert np.abs(inv[labels == a] - inv[labels == a][0]).max() <= 1e-12 * scale
        # the crystal-level projection that symmetrize_graphs(..., ops="find") applies
        R = h.crystals[0]["rotations"]
        y = rng.standard_normal((1, 21))
        once, dev = average_irreps_host(y, "ijkl=jikl=klij", R)
        twice, dev2 = average_irreps_host(once, "ijkl=jikl=klij", R)
        assert np.abs(twice - once).max() <= 1e-12 * np.linalg.norm(y) and dev2[0] <= 1e-12 < dev[0]


def test_library_exports_the_symmetry_entries():
    from matten_amd import _lib, ops, predict, symmetry

    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "matten_hip.h")).read()
    for name in NEW_ENTRIES:
        assert name in _lib.SIGNATURES and hasattr(lib, name) and header.count("int " + name + "(") == 1, name
    assert _lib.ABI_VERSION == 47 == lib.matten_abi_version()   # entries were only added
    for name, bit in (("NOT_FINITE", 1), ("RANGE", 2), ("TOO_LARGE", 4), ("AMBIGUOUS", 8), ("TRUNC", 16), ("NOT_PERIODIC", 32)):
        assert f"#define MATTEN_SYM_{name} {bit}\n" in header and getattr(symmetry, "SYM_" + name) == bit
    assert "#define MATTEN_SYM_MAX_ATOMS 1024\n" in header and ops.SYM_MAX_ATOMS == 1024 and ops.SYM_MAX_OPS == 48
    for fn in (ops.lattice_group, ops.crystal_symmetry, ops.irreps_average_atoms, symmetry.find_symmetry, symmetry.find_symmetry_host,
               symmetry.symmetrize_atoms, symmetry.symmetrize_atoms_host, predict.symmetry_report):
        assert callable(fn)
    import torch

    with pytest.raises(_lib.MattenHipError, match="no CPU fallback"):
        ops.lattice_group(torch.eye(3, dtype=torch.float64)[None])


P = 4096   # a fake non-NULL pointer: never dereferenced on the host, nothing is launched when the call is refused


def _lattice(lib, **kw):
    a = dict(cell=P, B=3, symprec=1e-3, N=P, n_lat=P, flags=P)
    a.update(kw)
    return lib.matten_lattice_group(a["cell"], a["B"], a["symprec"], a["N"], a["n_lat"], a["flags"], None)


def _crystal(lib, **kw):
    a = dict(pos=P, cell=P, Z=P, ptr=P, pbc=None, B=3, n=8, symprec=1e-3, max_trans=64, N_in=P, n_lat=P, lat_flags=P, rot=P, rot_int=P,
             trans=P, n_rot=P, src=P, n_trans=P, ttrans=P, tsrc=P, flags=P)
    a.update(kw)
    return lib.matten_crystal_symmetry(a["pos"], a["cell"], a["Z"], a["ptr"], a["pbc"], a["B"], a["n"], a["symprec"], a["max_trans"],
                                       a["N_in"], a["n_lat"], a["lat_flags"], a["rot"], a["rot_int"], a["trans"], a["n_rot"], a["src"],
                                       a["n_trans"], a["ttrans"], a["tsrc"], a["flags"], None)


def _atoms(lib, **kw):
    layout = np.array([[0, 1, 0, 1], [1, 1, 2, 1]], dtype=np.int32)
    a = dict(x=P, is_fp64=1, n=8, dim=6, layout=layout.ctypes.data, K=2, D=P, flags=P, B=3, G_cap=48, n_ops=P, row_struct=P, src=P,
             out=2 * P)
    a.update(kw)
    return lib.matten_irreps_average_atoms(a["x"], a["is_fp64"], a["n"], a["dim"], a["layout"], a["K"], a["D"], a["flags"], a["B"],
                                           a["G_cap"], a["n_ops"], a["row_struct"], a["src"], a["out"], None)


@pytest.mark.parametrize("call,bad", [
    (_lattice, dict(cell=None)), (_lattice, dict(N=None)), (_lattice, dict(n_lat=None)), (_lattice, dict(flags=None)),
    (_lattice, dict(B=-1)), (_lattice, dict(symprec=0.0)), (_lattice, dict(symprec=-1e-3)), (_lattice, dict(symprec=float("inf"))),
    (_lattice, dict(symprec=float("nan"))),
    (_crystal, dict(pos=None)), (_crystal, dict(cell=None)), (_crystal, dict(Z=None)), (_crystal, dict(ptr=None)),
    (_crystal, dict(N_in=None)), (_crystal, dict(n_lat=None)), (_crystal, dict(lat_flags=None)), (_crystal, dict(rot=None)),
    (_crystal, dict(rot_int=None)), (_crystal, dict(trans=None)), (_crystal, dict(n_rot=None)), (_crystal, dict(src=None)),
    (_crystal, dict(n_trans=None)), (_crystal, dict(ttrans=None)), (_crystal, dict(tsrc=None)), (_crystal, dict(flags=None)),
    (_crystal, dict(B=-1)), (_crystal, dict(n=-1)), (_crystal, dict(max_trans=0)), (_crystal, dict(symprec=0.0)),
    (_crystal, dict(symprec=float("nan"))), (_crystal, dict(n=1 << 31)),
    (_atoms, dict(x=None)), (_atoms, dict(out=None)), (_atoms, dict(out=P)), (_atoms, dict(n_ops=None)), (_atoms, dict(row_struct=None)),
    (_atoms, dict(src=None)), (_atoms, dict(flags=None)), (_atoms, dict(n=-1)), (_atoms, dict(dim=-1)), (_atoms, dict(K=17)),
    (_atoms, dict(K=-1)), (_atoms, dict(layout=None)), (_atoms, dict(dim=5)), (_atoms, dict(G_cap=0)), (_atoms, dict(B=-1)),
    (_atoms, dict(is_fp64=2)),
], ids=lambda v: v.__name__.strip("_") if callable(v) else "-".join(f"{k}={x}" for k, x in v.items()))
def test_entries_refuse_bad_arguments(call, bad):
    from matten_amd import _lib

    assert call(_lib.load(), **bad) == -1
