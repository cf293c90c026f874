"""
The symmetry search on the GPU (csrc/spacegroup.hip and rot_average_atoms_kernel of csrc/rotate.hip through
matten_amd/symmetry.py), held to the numpy restatement ``find_symmetry_host`` (every integer matrix enumerated, every
(operation, translation) pair tested in full: not the kernels' method) on the crystals of tests/spacegroup_cases.py.

Integers (orders, integer matrices, atom maps, flags) must agree exactly.  Cartesian matrices and translations: 1e-10 --
both sides take the polar factor of the same near-orthogonal matrix in fp64 (cells with condition numbers below 10, so
agreement is expected near 1e-13); 1e-10 is seven orders below the symprec / a scale at which a wrong matrix would show.
Rows: 2^-23 |x_r| in fp32, 1e-12 |x_r| in fp64, as in tests/test_gpu_symmetry.py (unit weights: no condition factor); a
per-atom row is a mean of rows of other atoms of its crystal, so there |x_r| is the crystal's largest row norm.
Shapes: 1 to 8 atoms for the table, 32 / 64 / 65 / 300 atoms for lanes, waves and passes that do not divide evenly, and 1025
for the size limit.
"""
import functools
import os

import numpy as np
import pytest
import torch

import spacegroup_cases as sc
from common import EQUIV_TEST, build_pair

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROW_TOL = {torch.float32: 2.0 ** -23, torch.float64: 1e-12}
MAT_TOL = 1e-10
ATOM_SPECS = ("ij=ji", "ij", "2x0e+1o+2x2e+1e+3o")
ATOM_CRYSTALS = ("rutile", "wurtzite", "zincblende", "fcc_2x2x2", "interstitial_65")


def crystal_of(key):
    """a case name, (name, "noisy"), or one of the extra crystals by name"""
    if isinstance(key, tuple):
        return sc.crystal(key[0], noisy=True)
    if key in sc.CASES:
        return sc.crystal(key)
    if key.startswith("random_"):
        return sc.random_triclinic(int(key.split("_")[1]), seed=7)
    if key.startswith("displaced_"):
        return sc.displaced_diamond(float(key.split("_")[1]) * sc.SYMPREC)
    cell, pos, Z = sc.crystal("wurtzite")
    if key == "nan":
        pos = pos.copy()
        pos[1, 2] = np.nan
        return cell, pos, Z
    if key == "close_pair":
        return cell, np.concatenate([pos, pos[:1] + 1e-4]), np.concatenate([Z, Z[:1]])
    if key == "range":
        return sc.RANGE_CELL, np.zeros((1, 3)), np.array([13])
    return {"fcc_4x4x4": sc.fcc_primitive_4x4x4, "interstitial_65": sc.interstitial_65}[key]()


@functools.lru_cache(maxsize=None)
def host_one(key, max_trans=64, pbc=None):
    """the restatement's answer for one crystal alone, computed once and shared"""
    from matten_amd.symmetry import find_symmetry_host

    return find_symmetry_host(**sc.pack([crystal_of(key)]), symprec=sc.SYMPREC, max_trans=max_trans, pbc=pbc)


def find(keys, max_trans=64, pbc=None):
    from matten_amd.symmetry import find_symmetry

    return find_symmetry(**sc.pack([crystal_of(k) for k in keys]), symprec=sc.SYMPREC, max_trans=max_trans, pbc=pbc, device=DEV)


def assert_crystal(got, b, want, what):
    """crystal b of the batch result ``got`` (a HostSymmetry read back) against ``want``, the restatement's single-crystal
    answer: integers exactly (atom indices relative to the crystal's first atom), matrices and translations to MAT_TOL"""
    lo, hi = int(got.ptr[b]), int(got.ptr[b + 1])
    assert hi - lo == len(want.row_struct), what

    def local(a):
        return np.where(a < 0, -1, a - lo)

    assert (int(got.n_rot[b]), int(got.n_trans[b]), int(got.flags[b])) == (int(want.n_rot[0]), int(want.n_trans[0]), int(want.flags[0])), what
    assert np.array_equal(got.rotations_int[b], want.rotations_int[0]), what
    assert np.array_equal(local(got.src[:, lo:hi]), want.src), what
    assert np.array_equal(local(got.tsrc[:, lo:hi]), want.tsrc), what
    assert (got.row_struct[lo:hi] == b).all(), what
    assert np.abs(got.rotations[b] - want.rotations[0]).max() <= MAT_TOL, what
    for a, w in ((got.translations[b], want.translations[0]), (got.pure_translations[b], want.pure_translations[0])):
        d = a - w
        assert np.abs(d - np.round(d)).max() <= MAT_TOL, what
    R = got.rotations[b, :int(got.n_rot[b])]
    assert np.abs(np.einsum("gki,gkj->gij", R, R) - np.eye(3)).max() <= 1e-12, what


ALL_KEYS = tuple(sc.NAMES) + tuple((n, "noisy") for n in sc.NAMES)


# ----------------------------------------------------------------------------------------------------------------------
# 1, 2: the lattice step and the search against the restatement
# ----------------------------------------------------------------------------------------------------------------------
def test_lattice_group_matches_the_restatement():
    from matten_amd import ops
    from matten_amd.symmetry import lattice_group_host

    cells = np.stack([crystal_of(k)[0] for k in ALL_KEYS] + [sc.RANGE_CELL, np.zeros((3, 3))])
    N, n_lat, flags = ops.lattice_group(torch.as_tensor(cells, device=DEV), sc.SYMPREC)
    Nh, nh, fh = lattice_group_host(cells, sc.SYMPREC)
    assert np.array_equal(n_lat.cpu().numpy(), nh) and np.array_equal(flags.cpu().numpy(), fh)
    assert np.array_equal(N.cpu().numpy(), Nh)                            # order included
    assert fh[-2:].tolist() == [2, 1] and set(nh[:len(sc.NAMES)]) == {48, 24, 16, 8, 4, 2}


@pytest.mark.parametrize("key", ALL_KEYS, ids=lambda k: k if isinstance(k, str) else k[0] + "-noisy")
def test_single_crystal_matches_the_restatement(key):
    name = key if isinstance(key, str) else key[0]
    want = host_one(key)
    assert (int(want.n_rot[0]), int(want.n_trans[0])) == sc.expected(name)
    assert_crystal(find([key]).host(), 0, want, key)


@pytest.mark.parametrize("order", ["forward", "shuffled"])
def test_batch_matches_the_restatement_whatever_the_order(order):
    keys = list(ALL_KEYS)
    if order == "shuffled":
        keys = [keys[i] for i in np.random.default_rng(3).permutation(len(keys))]
    got = find(keys).host()
    for b, key in enumerate(keys):
        assert_crystal(got, b, host_one(key), (order, b, key))


# ----------------------------------------------------------------------------------------------------------------------
# 3: broken symmetry
# ----------------------------------------------------------------------------------------------------------------------
def test_a_displaced_atom_breaks_the_symmetry():
    got = find(["displaced_10.0", "displaced_0.1", "diamond"]).host()
    moved, whole = host_one("displaced_10.0"), host_one("diamond")
    assert int(moved.n_rot[0]) < 48 and int(moved.n_trans[0]) == 1
    assert_crystal(got, 0, moved, "10 symprec")
    assert_crystal(got, 2, whole, "diamond")
    # a tenth of symprec: the undisplaced answer (the translations move with the atom by 1e-4 at the most)
    assert int(got.n_rot[1]) == 48 and int(got.n_trans[1]) == 4 and int(got.flags[1]) == 0
    assert np.array_equal(got.rotations_int[1], whole.rotations_int[0])
    assert np.array_equal(got.src[:, 8:16] - 8, whole.src) and np.array_equal(np.where(got.tsrc[:, 8:16] < 0, -1, got.tsrc[:, 8:16] - 8), whole.tsrc)
    assert np.abs(got.rotations[1] - whole.rotations[0]).max() <= MAT_TOL


# ----------------------------------------------------------------------------------------------------------------------
# 4: flags, each flagged crystal between two good ones
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,flag", [("range", 2), ("random_1025", 4), ("nan", 1), ("close_pair", 8)])
def test_flagged_crystal_between_two_good_ones(key, flag):
    got = find(["diamond", key, "wurtzite"]).host()
    assert got.flags.tolist() == [0, flag, 0] and got.n_rot.tolist() == [48, 1, 12] and got.n_trans.tolist() == [4, 1, 1]
    for b, k in enumerate(["diamond", key, "wurtzite"]):
        assert_crystal(got, b, host_one(k), (key, b))


def test_open_axis_is_flagged():
    pbc = np.array([[True, True, True], [True, True, False], [True, True, True]])
    got = find(["diamond", "rutile", "wurtzite"], pbc=pbc).host()
    assert got.flags.tolist() == [0, 32, 0] and got.n_rot.tolist() == [48, 1, 12]
    assert_crystal(got, 0, host_one("diamond"), "diamond")
    assert_crystal(got, 1, host_one("rutile", pbc=(True, True, False)), "rutile, open")
    assert_crystal(got, 2, host_one("wurtzite"), "wurtzite")


@pytest.mark.parametrize("max_trans,flag", [(64, 0), (32, 16)])
def test_translation_list_capacity(max_trans, flag):
    keys = ["diamond", "fcc_4x4x4", "wurtzite"]
    got = find(keys, max_trans=max_trans).host()
    assert got.flags.tolist() == [0, flag, 0] and got.n_rot.tolist() == [48, 48, 12] and got.n_trans.tolist() == [4, 64, 1]
    assert got.tsrc.shape[0] == max_trans
    for b, k in enumerate(keys):
        assert_crystal(got, b, host_one(k, max_trans=max_trans), (max_trans, k))


# ----------------------------------------------------------------------------------------------------------------------
# 5: sizes that are no multiple of a wave or a block
# ----------------------------------------------------------------------------------------------------------------------
def test_odd_sizes():
    keys = ["simple_cubic", "interstitial_65", "random_300", "fcc_2x2x2", "fcc_primitive"]
    got = find(keys).host()
    assert got.n_rot.tolist() == [48, 1, 1, 48, 48] and got.n_trans.tolist() == [1, 1, 1, 32, 1] and not got.flags.any()
    for b, k in enumerate(keys):
        assert_crystal(got, b, host_one(k), k)


# ----------------------------------------------------------------------------------------------------------------------
# 6: crystal-level tensors
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("formula", ["ijkl=jikl=klij", "ij=ji"])
def test_crystal_rows_over_the_found_point_groups(formula, dtype):
    from matten_amd.symmetry import average_irreps, average_irreps_host, irreps_of, symmetry_deviation

    keys = list(sc.NAMES)
    sym = find(keys)
    dim = irreps_of(formula).dim
    xh = np.random.default_rng(11).standard_normal((len(keys), dim))
    x = torch.as_tensor(xh, dtype=dtype, device=DEV)
    xh = x.double().cpu().numpy()
    R, op_ptr, op_idx = sym.op_csr()
    avg, dev = average_irreps(x, formula, R, op_ptr, op_idx)
    hosts = [host_one(k) for k in keys]
    Rh = np.concatenate([h.crystals[0]["rotations"] for h in hosts])
    ptr_h = np.concatenate([[0], np.cumsum([int(h.n_rot[0]) for h in hosts])])
    want, want_dev = average_irreps_host(xh, formula, Rh, ptr_h, np.arange(ptr_h[-1]))
    err = np.abs(avg.double().cpu().numpy() - want).max(axis=1) / np.linalg.norm(xh, axis=1)
    print(f"{formula} {dtype}: worst row error {err.max():.2e} of |x_r| (bound {ROW_TOL[dtype]:.2e})")
    assert err.max() <= ROW_TOL[dtype]
    if dtype == torch.float64:
        assert np.abs(dev.cpu().numpy() - want_dev).max() <= 1e-12
        again = symmetry_deviation(avg, formula, R, op_ptr, op_idx)
        assert float(again.max()) <= 1e-12
        # un-collated host graphs through ops="find": the same rows; a second pass changes nothing
        from matten_amd.symmetry import symmetrize_graphs

        graphs = []
        for k, row in zip(keys, xh):
            cell, pos, Z = crystal_of(k)
            graphs.append({"pos": torch.as_tensor(pos), "cell": torch.as_tensor(cell), "atomic_numbers": torch.as_tensor(Z),
                           "y": torch.as_tensor(row)})
        d1 = symmetrize_graphs(graphs, "y", formula, "find", device=DEV, symprec=sc.SYMPREC)
        rows = np.stack([g["y"].numpy() for g in graphs])
        assert np.array_equal(rows, avg.cpu().numpy()) and np.array_equal(d1, dev.cpu().numpy())
        d2 = symmetrize_graphs(graphs, "y", formula, "find", device=DEV, symprec=sc.SYMPREC)
        assert d2.max() <= 1e-12 and np.abs(np.stack([g["y"].numpy() for g in graphs]) - rows).max() <= 1e-12 * np.abs(xh).max()


# ----------------------------------------------------------------------------------------------------------------------
# 7: per-atom tensors
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("spec", ATOM_SPECS)
def test_per_atom_rows_over_the_found_symmetry(spec, dtype):
    from matten_amd.symmetry import _host_D, irreps_of, symmetrize_atoms, symmetrize_atoms_host

    keys = list(ATOM_CRYSTALS)
    sym = find(keys)
    hosts = [host_one(k) for k in keys]
    n = int(sym.row_struct.shape[0])
    xh = np.random.default_rng(13).standard_normal((n, irreps_of(spec).dim))
    x = torch.as_tensor(xh, dtype=dtype, device=DEV)
    xh = x.double().cpu().numpy()
    out, dev = symmetrize_atoms(x, spec, sym)
    assert out.dtype == dtype and dev.dtype == torch.float64
    got, ptr = out.double().cpu().numpy(), sym.ptr.cpu().numpy()
    labels = sym.equivalent_atoms().cpu().numpy()
    worst = 0.0
    for b, h in enumerate(hosts):
        lo, hi = int(ptr[b]), int(ptr[b + 1])
        want, want_dev = symmetrize_atoms_host(xh[lo:hi], spec, h)
        # an output row is a mean of rotated rows of its crystal: the scale of its rounding is the largest of their norms.
        # fp32 rows are rounded twice (after the representatives, after the translations), 2^-24 of that scale each.
        scale = np.full(hi - lo, np.linalg.norm(xh[lo:hi], axis=1).max())
        worst = max(worst, float((np.abs(got[lo:hi] - want).max(axis=1) / scale).max()))
        assert np.array_equal(labels[lo:hi] - lo, h.equivalent_atoms())
        if dtype == torch.float64:
            assert np.abs(dev.cpu().numpy()[lo:hi] - want_dev).max() <= 1e-12
            # invariance under every representative and every pure translation of the restatement, hence under the full group
            c, y, big = h.crystals[0], got[lo:hi], scale.max()
            for D, src in zip(_host_D(spec, c["rotations"]), c["src"]):
                assert np.abs(y[src] @ D.T - y).max() <= 1e-12 * big
                assert np.array_equal(labels[lo:hi][src], labels[lo:hi])          # orbits are closed under the operations
            for tsrc in c["tsrc"]:
                assert np.abs(y[tsrc] - y).max() <= 1e-12 * big and np.array_equal(labels[lo:hi][tsrc], labels[lo:hi])
            # rows of one orbit are related by the operations: some (g, tau) takes the orbit's first atom a to atom k, i.e.
            # tsrc[tau, src[g,k]] = a, and then out[k] = D(M_g) out[a]
            first = labels[lo:hi] - lo
            lands = (c["tsrc"][:, c["src"]] == first[None, None, :]).any(axis=0)      # [G,n]
            assert lands.any(axis=0).all()
            Dg = _host_D(spec, c["rotations"])[lands.argmax(axis=0)]                # [n,dim,dim]
            assert np.abs(np.einsum("kij,kj->ki", Dg, y[first]) - y).max() <= 1e-12 * big
    print(f"{spec} {dtype}: worst row error {worst:.2e} of max|x_r| (bound {ROW_TOL[dtype]:.2e})")
    assert worst <= ROW_TOL[dtype]
    if dtype == torch.float64:
        twice, dev2 = symmetrize_atoms(out, spec, sym)
        assert float((twice - out).abs().max()) <= 1e-12 * np.linalg.norm(xh, axis=1).max() and float(dev2.max()) <= 1e-12


def test_truncated_translations_give_nan_rows():
    from matten_amd.symmetry import symmetrize_atoms

    sym = find(["wurtzite", "fcc_4x4x4"], max_trans=32)
    x = torch.as_tensor(np.random.default_rng(17).standard_normal((68, 6)), device=DEV)
    out, dev = symmetrize_atoms(x, "ij=ji", sym)
    assert bool(torch.isfinite(out[:4]).all()) and bool(torch.isnan(out[4:]).all()) and bool(torch.isnan(dev[4:]).all())
    out, dev = symmetrize_atoms(x, "ij=ji", sym, translations=False)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(dev).all())


# ----------------------------------------------------------------------------------------------------------------------
# 8: reproducible and capturable
# ----------------------------------------------------------------------------------------------------------------------
def test_captured_graph_replays_bit_for_bit():
    from matten_amd import ops
    from matten_amd.symmetry import irreps_layout

    packs = [sc.pack([crystal_of(k), crystal_of("rutile")]) for k in ("diamond", "displaced_10.0")]
    t = {k: torch.as_tensor(v, device=DEV) for k, v in packs[0].items()}
    layout = irreps_layout("ij=ji")
    x = torch.as_tensor(np.random.default_rng(19).standard_normal((14, 6)), device=DEV)
    row_struct = torch.as_tensor([0] * 8 + [1] * 6, dtype=torch.int32, device=DEV)
    lattice = ops.lattice_group(t["cell"], sc.SYMPREC)

    def run(out=None):
        res = ops.crystal_symmetry(t["pos"], t["cell"], t["Z"], t["ptr"], lattice, None, sc.SYMPREC, 64, out=None if out is None else out[0])
        D = ops.wigner_d(res[0].view(-1, 9), 2, out=None if out is None else out[1])
        y = ops.irreps_average_atoms(x, layout, D[0], D[1], res[3], row_struct, res[4], out=None if out is None else out[2])
        return res, D, y

    def parts(r):
        """every output as bytes (NaN rows of D included); of the D table the blocks up to l = 2 that were asked for"""
        res, D, y = r
        return [u.contiguous().view(torch.uint8).clone() for u in res + (D[0][:, :35], D[1], y)]

    eager = []
    for p in packs:
        t["pos"].copy_(torch.as_tensor(p["pos"], device=DEV))
        a, b = run(), run()
        for u, v in zip(parts(a), parts(b)):
            assert torch.equal(u, v)                                                  # two runs, bit for bit
        eager.append(parts(a) + [a[0][3].clone()])
    assert int(eager[0].pop()[0]) == 48 and int(eager[1].pop()[0]) < 48
    bufs = run()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(bufs)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run(bufs)
    for p, want in zip(packs, eager):
        t["pos"].copy_(torch.as_tensor(p["pos"], device=DEV))
        graph.replay()
        for u, v in zip(parts(bufs), want):
            assert torch.equal(u, v)


# ----------------------------------------------------------------------------------------------------------------------
# 9: the report
# ----------------------------------------------------------------------------------------------------------------------
def test_symmetry_report(golden_dir):
    """Orders, translation counts and flags as the restatement's; the deviation bit for bit what the public functions give
    on the same predictions.  How far an fp32 equivariant model's prediction lies from its symmetrised self has no bound
    here: it is printed (docs/LAB_NOTES.md records the run)."""
    from matten_amd.predict import symmetry_report
    from matten_amd.symmetry import find_symmetry_host, symmetry_deviation
    from oracle.matten_ref.data import structures_from_json

    structures = list(structures_from_json(os.path.join(golden_dir, "elastic_tensor_one.json")))
    for name in ("diamond", "wurtzite"):
        cell, pos, Z = sc.crystal(name)
        structures.append({"cart_coords": pos, "lattice": cell, "atomic_numbers": Z})
    species = sorted({int(z) for s in structures for z in s["atomic_numbers"]})
    _, model = build_pair(EQUIV_TEST, {"allowed_species": species})
    rep = symmetry_report(model, structures, symprec=sc.SYMPREC, r_cut=5.0)
    want = find_symmetry_host(structures, symprec=sc.SYMPREC)
    assert rep["order"].tolist() == want.n_rot.tolist() and rep["n_trans"].tolist() == want.n_trans.tolist()
    assert rep["flags"].tolist() == want.flags.tolist() == [0] * len(structures)
    assert rep["order"][-2:].tolist() == [48, 12]
    R, op_ptr, op_idx = rep["symmetry"].op_csr()
    apart = symmetry_deviation(rep["predictions"], "ijkl=jikl=klij", R, op_ptr, op_idx).cpu().numpy()
    assert np.array_equal(rep["deviation"], apart) and np.isfinite(rep["deviation"]).all()
    assert rep["worst"] == rep["deviation"].max() and rep["worst_structure"] == int(rep["deviation"].argmax())
    print(f"symmetry_report: orders {rep['order'].tolist()}, deviation {rep['deviation']}")


def test_symmetry_report_of_per_atom_tensors():
    from common import ATOMIC
    from matten_amd.predict import symmetry_report
    from matten_amd.symmetry import symmetrize_atoms
    from test_atom_targets_host import fixture_dataset_hparams, fixture_graphs

    g = fixture_graphs("compact")[9]
    s = {"cart_coords": g["pos"].double().numpy(), "lattice": g["cell"].double().numpy().reshape(3, 3),
         "atomic_numbers": g["atomic_numbers"].numpy()}
    _, model = build_pair(dict(ATOMIC), fixture_dataset_hparams(), randomize_bn=True, atomic=True)
    rep = symmetry_report(model, [s], r_cut=5.0, formula="ij=ji", is_atomic_tensor=True)
    _, per_atom = symmetrize_atoms(rep["predictions"], "ij=ji", rep["symmetry"])
    assert rep["deviation"].shape == (1,) and rep["deviation"][0] == float(per_atom.max()) and np.isfinite(rep["deviation"]).all()
    assert rep["flags"].tolist() == [0] and rep["order"][0] >= 1
    print(f"per-atom symmetry_report: order {rep['order']}, n_trans {rep['n_trans']}, deviation {rep['deviation']}")
