"""
Rotations and symmetry averages of irreps tensors on the GPU (csrc/rotate.hip through matten_amd/symmetry.py), held to the
numpy restatements of tests/test_symmetry_host.py (the Kronecker definition D_f(M) = Qf (M x ... x M) Qf^T, not the
kernels' method).  Shapes are the smallest that can go wrong: one rotation and 67 (no multiple of a wave), 1 / 3 / 257
rows (more than one block of 128), every formula of tests/symmetry_cases.py and a column-mixed irreps string.

Tolerances.  D entries: 1e-12 -- they are bounded by 1 and come from fewer than 1e3 fp64 operations times the condition
(<= 5) of the direction sets, about 6e-13.  Rows: per row 2^-23 |x_r|_2 in fp32 (one rounding of values bounded by |x_r|,
with a factor 2) and 1e-12 |x_r|_2 in fp64, times sum|w| / |sum w| for an average.
"""
import os

import numpy as np
import pytest
import torch

import symmetry_cases as cases
from common import ATOMIC, EQUIV_TEST, build_pair

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROW_TOL = {torch.float32: 2.0 ** -23, torch.float64: 1e-12}
SPECS = cases.FORMULAS + (cases.MIXED_IRREPS,)
N_ROWS = (1, 3, 257)
_CACHE = {}


def dev(a, dtype=torch.float64):
    return torch.as_tensor(np.array(a), dtype=dtype, device=DEV)       # (a copy: the shared groups are read-only arrays)


def host_D(spec):
    """the restatement's matrices of the 257 shared rotations for one spec, computed once"""
    from matten_amd.symmetry import _host_D

    if spec not in _CACHE:
        _CACHE[spec] = _host_D(spec, cases.rotations(257, seed=11))
    return _CACHE[spec]


def row_err(got, want, x):
    """max over rows of max|got - want| / |x_r|_2 (rows of x are never zero here)"""
    got, x = got.detach().cpu().double().numpy(), np.asarray(x, dtype=np.float64)
    return float((np.abs(got - want).max(axis=1) / np.linalg.norm(x, axis=1)).max())


# ----------------------------------------------------------------------------------------------------------------------
# the D table
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [1, 67])
def test_wigner_table_against_the_restatement(G):
    from matten_amd import ops
    from matten_amd.symmetry import wigner_D, wigner_D_host

    R = cases.rotations(67, seed=2)[5:6] if G == 1 else cases.rotations(67, seed=2)
    D, flags = ops.wigner_d(dev(R), 4)
    assert D.shape == (G, 165) and D.dtype == torch.float64 and flags.dtype == torch.int32
    assert flags.cpu().tolist() == [4 if d < 0 else 0 for d in np.linalg.det(R)]
    Dh = D.cpu().numpy()
    lo = 0
    for l in range(5):
        n = 2 * l + 1
        block = Dh[:, lo:lo + n * n].reshape(G, n, n)
        lo += n * n
        err = np.abs(block - wigner_D_host(l, R)).max()
        orth = np.abs(np.einsum("gik,gjk->gij", block, block) - np.eye(n)).max()
        print(f"G={G} l={l}: max|D - host| {err:.2e}, max|D D^T - I| {orth:.2e}")
        assert err <= 1e-12 and orth <= 1e-12
        for p in (None, 1, -1):
            assert np.abs(wigner_D(l, dev(R), p).cpu().numpy() - wigner_D_host(l, R, p)).max() <= 1e-12
    assert lo == 165
    # lmax below 4: the same leading blocks, the row stride stays 165 and the blocks above are not written
    out = (torch.full((G, 165), 7.0, dtype=torch.float64, device=DEV), torch.zeros(G, dtype=torch.int32, device=DEV))
    D2, f2 = ops.wigner_d(dev(R), 2, out=out)
    assert torch.equal(D2[:, :35], D[:, :35]) and bool((D2[:, 35:] == 7.0).all()) and torch.equal(f2, flags)


def test_wigner_flags():
    from matten_amd import ops
    from matten_amd.symmetry import wigner_D_host

    good = cases.random_rotations(1, seed=8)[0]
    nan, inf = good.copy(), good.copy()
    nan[1, 2], inf[0, 0] = np.nan, np.inf
    near = cases.nearly_orthogonal()
    R = np.stack([nan, cases.skewed(), -good, near, inf, good])
    D, flags = ops.wigner_d(dev(R), 4)
    assert flags.cpu().tolist() == [1, 2, 4, 0, 1, 0]
    Dh = D.cpu().numpy()
    assert np.isnan(Dh[[0, 1, 4]]).all() and np.isfinite(Dh[[2, 3, 5]]).all()
    assert np.array_equal(Dh[2], Dh[5])                                   # the proper part of -R is R
    # 1e-7 off orthogonal passes at the default orth_tol = 1e-6 (its D is the Kronecker form's to first order in 1e-7: the
    # harmonics normalise their argument, the Kronecker form does not; l (l + 1) / 2 <= 10 times 1e-7) and is flagged at 1e-8
    lo = 0
    for l in range(5):
        n = 2 * l + 1
        assert np.abs(Dh[3, lo:lo + n * n].reshape(n, n) - wigner_D_host(l, near)[0]).max() <= 1e-5
        lo += n * n
    _, strict = ops.wigner_d(dev(R), 4, orth_tol=1e-8)
    assert strict.cpu().tolist() == [1, 2, 4, 2, 1, 0]


# ----------------------------------------------------------------------------------------------------------------------
# rotate_irreps
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("spec", SPECS)
def test_rotate_irreps_against_the_restatement(spec, dtype):
    from matten_amd.symmetry import irreps_of, rotate_irreps

    R = cases.rotations(257, seed=11)
    assert (np.linalg.det(R) < 0).sum() > 50                      # improper rotations throughout: the parity factor matters
    D = host_D(spec)
    dim = irreps_of(spec).dim
    tol, worst = ROW_TOL[dtype], 0.0
    for n in N_ROWS:
        x = dev(cases.rows(n, dim, seed=n), dtype)
        xh = x.cpu().double().numpy()
        scattered = np.random.default_rng(n).integers(0, 12, n)
        for what, Rs, index, Ds in (("one rotation", R[7], None, D[np.full(n, 7)]),
                                    ("one per row", R[:n], None, D[:n]),
                                    ("identity index", R[:n], torch.arange(n, device=DEV), D[:n]),
                                    ("scattered index", R[:12], dev(scattered, torch.int64), D[scattered])):
            got = rotate_irreps(x, spec, dev(Rs), index=index)
            assert got.dtype == dtype and got.shape == x.shape
            err = row_err(got, np.einsum("nij,nj->ni", Ds, xh), xh)
            worst = max(worst, err)
            assert err <= tol, (spec, n, what, err)
    print(f"{spec} {dtype}: worst row error {worst:.2e} of |x_r| (bound {tol:.2e})")
    # an unbatched row
    one = rotate_irreps(x[0], spec, dev(R[7]))
    assert one.shape == (dim,) and torch.equal(one, rotate_irreps(x[:1], spec, dev(R[7]))[0])


def test_improper_rotations_and_bad_indices():
    from matten_amd.symmetry import rotate_irreps, rotate_irreps_host

    inv = dev(-np.eye(3))
    x = dev(cases.rows(5, 3, seed=1))
    # (D^1 of the identity comes out of the harmonics like any other: the identity to rounding, held to the fp64 row bound)
    xh = x.cpu().numpy()
    assert row_err(rotate_irreps(x, "ij=-ji", inv), xh, xh) <= 1e-12       # 1e: an axial vector does not see the inversion
    assert row_err(rotate_irreps(x, "i", inv), -xh, xh) <= 1e-12           # 1o
    M = -cases.random_rotations(1, seed=5)[0]
    for f in ("ijk=ikj", "ij=-ji"):
        xs = cases.rows(3, 18 if f == "ijk=ikj" else 3, seed=2)
        got, proper = rotate_irreps(dev(xs), f, dev(M)), rotate_irreps(dev(xs), f, dev(-M))
        assert row_err(got, rotate_irreps_host(xs, f, M), xs) <= 1e-12
        # every irrep of ijk=ikj is odd (2x1o+2o+3o): the improper rotation is minus its proper part; 1e does not see the sign
        assert torch.equal(got, -proper if f == "ijk=ikj" else proper)
    # a flagged rotation and an index outside R give NaN rows, the others are untouched by it
    R = dev(np.stack([np.eye(3), cases.skewed()]))
    out = rotate_irreps(x, "i", R, index=dev([0, 1, 2, -1, 0], torch.int64))
    assert row_err(out[[0, 4]], xh[[0, 4]], xh[[0, 4]]) <= 1e-12 and bool(torch.isnan(out[1:4]).all())


def test_model_harmonics_rotate_with_the_table():
    """Y(R v) = D^l Y(v) with the device's own harmonics: edge vectors v and R v through the edge-geometry kernel (fp32).
    Both sides carry the harmonics' error, so the bound is twice that of
    test_gpu_parity.py::test_edge_geometry_sh_and_bessel_vs_oracle (2e-6 of the largest magnitude)."""
    from matten_amd import ops
    from matten_amd.symmetry import wigner_D

    rng = np.random.default_rng(4)
    v = (rng.standard_normal((7, 3)) * rng.uniform(0.5, 3.0, (7, 1))).astype(np.float32).astype(np.float64)
    R = cases.random_rotations(1, seed=6)[0]
    pos = np.concatenate([np.zeros((1, 3)), v, v @ R.T])
    ei = torch.stack([torch.zeros(14, dtype=torch.int64), torch.arange(1, 15)]).to(DEV)
    cell, shift = dev(100.0 * np.eye(3), torch.float32), torch.zeros(14, 3, dtype=torch.float32, device=DEV)
    sh = ops.edge_geom(dev(pos, torch.float32), ei, shift, cell, None, None, 4)["sh_sorted"][:, :25].cpu().double().numpy()
    Y, YR = sh[:7], sh[7:]
    assert np.abs(Y[:, 0] - 1.0).max() == 0.0
    scale = np.abs(sh).max()
    for l in range(1, 5):
        D = wigner_D(l, dev(R))[0].cpu().numpy()
        err = np.abs(YR[:, l * l:(l + 1) ** 2] - Y[:, l * l:(l + 1) ** 2] @ D.T).max()
        print(f"l={l}: max|Y(Rv) - D Y(v)| {err:.2e} (scale {scale:.2f})")
        assert err <= 4e-6 * scale


# ----------------------------------------------------------------------------------------------------------------------
# average_irreps
# ----------------------------------------------------------------------------------------------------------------------
def _average_case():
    cubic, hexagonal = cases.group("cubic"), cases.group("hexagonal")
    R = np.concatenate([cubic, hexagonal, cases.random_rotations(1, seed=3), cases.skewed()[None]])      # 48 + 24 + 1 + 1
    lists = [[], [72], list(range(48, 72)), list(range(48)), list(range(48)), [0, 73, 5], [3, 4], list(range(48)),
             [2, -1], [74, 1], [6, 7, 8]]                      # rows 8, 9: an op_idx below 0 and one at G = 74; row 10: see w
    op_ptr = np.concatenate([[0], np.cumsum([len(v) for v in lists])]).astype(np.int64)
    op_idx = np.concatenate([np.asarray(v, dtype=np.int32) for v in lists])
    x = cases.rows(len(lists), 21, seed=21)
    x[7] = 0.0
    rng = np.random.default_rng(22)
    w = rng.uniform(0.1, 2.0, len(op_idx))
    w[op_ptr[6]:op_ptr[7]] = [1.0, -1.0]                       # row 6: the weights sum to zero
    w[op_ptr[10] + 1] = np.inf                                 # row 10: a weight that is not finite
    return R, op_ptr, op_idx, x, w


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_average_irreps_against_the_restatement(dtype, weighted):
    """rows with 0, 1, 24 and 48 operations in one call, two rows sharing the same 48; a flagged operation, an op_idx
    below 0 and one at G, weights that sum to zero, a weight that is not finite, a zero row.  ``out`` and ``deviation`` are
    held to the same bound: the deviation is formed in fp64 from ``out`` as stored, so it differs from the host's by at most
    |fl(out) - out|_2 / |x|_2, one rounding of the row."""
    from matten_amd import o3
    from matten_amd.symmetry import average_irreps, average_irreps_host

    f = "ijkl=jikl=klij"
    R, op_ptr, op_idx, x, w = _average_case()
    w = w if weighted else None
    xd = dev(x, dtype)
    xh = xd.cpu().double().numpy()
    want, want_dev = average_irreps_host(xh, f, R, op_ptr, op_idx, w)
    got, got_dev = average_irreps(xd, f, dev(R), dev(op_ptr, torch.int64), dev(op_idx, torch.int32), None if w is None else dev(w))
    assert got.dtype == dtype and got_dev.dtype == torch.float64 and got_dev.shape == (11,)
    g, gd = got.cpu().double().numpy(), got_dev.cpu().numpy()

    assert np.array_equal(g[0], xh[0]) and gd[0] == 0.0                         # the empty list: the trivial group
    assert np.isnan(g[5]).all() and np.isnan(gd[5])                             # a flagged operation
    assert np.array_equal(g[7], xh[7]) and gd[7] == 0.0                         # a zero row
    assert np.isnan(g[[8, 9]]).all() and np.isnan(gd[[8, 9]]).all()             # an op_idx outside [0, G): nothing is read
    assert np.isnan(want[[8, 9]]).all() and np.isnan(want_dev[[8, 9]]).all()
    live = [1, 2, 3, 4] if weighted else [1, 2, 3, 4, 6, 10]
    if weighted:
        assert np.isnan(g[6]).all() and np.isnan(gd[6])                         # sum of weights 0
        assert np.isnan(g[10]).all() and np.isnan(gd[10]) and np.isnan(want[10]).all()      # a weight that is not finite
    assert np.isnan(want[5]).all() and (not weighted or np.isnan(want[6]).all())
    for r in live:
        ws = np.ones(op_ptr[r + 1] - op_ptr[r]) if w is None else w[op_ptr[r]:op_ptr[r + 1]]
        bound = ROW_TOL[dtype] * np.abs(ws).sum() / abs(ws.sum())
        err = np.abs(g[r] - want[r]).max() / np.linalg.norm(xh[r])
        derr = abs(gd[r] - want_dev[r])
        print(f"row {r} ({len(ws)} operations): row error {err:.2e} (bound {bound:.2e}), deviation {gd[r]:.4f} off by {derr:.2e}")
        assert err <= bound and derr <= bound
    assert 0.1 < gd[3] < 1.0 and 0.1 < gd[2] < 1.0

    # a second call gives the same bits
    again, again_dev = average_irreps(xd, f, dev(R), dev(op_ptr, torch.int64), dev(op_idx, torch.int32), None if w is None else dev(w))
    assert torch.equal(again.view(torch.int64 if dtype == torch.float64 else torch.int32),
                       got.view(torch.int64 if dtype == torch.float64 else torch.int32))
    assert torch.equal(again_dev.view(torch.int64), got_dev.view(torch.int64))

    if not weighted:
        # the cubic projection has the Voigt pattern, and feeding it back changes nothing
        _, Q = o3.cartesian_tensor_basis(f)
        C = np.einsum("qijkl,q->ijkl", Q, g[3])
        voigt = [(0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1)]
        V = np.array([[C[a + b] for b in voigt] for a in voigt])
        # (a Cartesian component is an orthonormal combination of the 21: off by at most sqrt(21) times the row bound, twice
        # that for a difference of two)
        tol = 2.0 * np.sqrt(21.0) * ROW_TOL[dtype] * np.linalg.norm(xh[3])
        assert abs(V[0, 0] - V[1, 1]) <= tol and abs(V[0, 0] - V[2, 2]) <= tol
        assert abs(V[0, 1] - V[0, 2]) <= tol and abs(V[0, 1] - V[1, 2]) <= tol
        assert abs(V[3, 3] - V[4, 4]) <= tol and abs(V[3, 3] - V[5, 5]) <= tol
        rest = V.copy()
        rest[:3, :3] = 0.0
        rest[[3, 4, 5], [3, 4, 5]] = 0.0
        assert np.abs(rest).max() <= tol
        from matten_amd.symmetry import symmetrize_irreps, symmetry_deviation

        cubic = dev(cases.group("cubic"))
        back = symmetry_deviation(got[3:5], f, cubic)
        # (the stored row is P x to one rounding, and the second call rounds once more: two roundings of the row, the bound)
        print(f"deviation of the projected rows fed back: {float(back.max()):.2e} (bound {ROW_TOL[dtype]:.2e})")
        assert float(back.max()) <= ROW_TOL[dtype]
        # the same list for every row, and the per-row list form, agree with the CSR form bit for bit
        same = symmetrize_irreps(xd[3:5], f, cubic)
        assert torch.equal(same, got[3:5])
        listed, _ = average_irreps(xd[2:4], f, [cases.group("hexagonal"), cases.group("cubic")])
        assert torch.equal(listed, got[2:4])


def test_average_with_every_list_empty():
    """G > 0 and nnz = 0: an empty op_idx has no address; the rows come back as they are, deviation 0"""
    from matten_amd.symmetry import average_irreps

    x = dev(cases.rows(5, 21, seed=3), torch.float32)
    avg, deviation = average_irreps(x, "ijkl=jikl=klij", dev(cases.group("cubic")), op_ptr=torch.zeros(6, dtype=torch.int64),
                                    op_idx=torch.zeros(0, dtype=torch.int32))
    assert torch.equal(avg, x) and bool((deviation == 0).all())


def test_symmetrize_graphs_cleans_labels_in_one_call():
    from matten_amd.symmetry import average_irreps_host, symmetrize_graphs

    f = "ijkl=jikl=klij"
    x = cases.rows(3, 21, seed=5).astype(np.float32)
    graphs = [{"elastic_tensor_full": torch.from_numpy(x[i:i + 1].copy())} for i in range(3)]
    ops_per = [cases.group("cubic"), np.zeros((0, 3, 3)), cases.group("hexagonal")]
    deviation = symmetrize_graphs(graphs, "elastic_tensor_full", f, ops_per, device=DEV)
    assert deviation.shape == (3,) and deviation[1] == 0.0 and torch.equal(graphs[1]["elastic_tensor_full"], torch.from_numpy(x[1:2]))
    for i in (0, 2):
        want, want_dev = average_irreps_host(x[i], f, ops_per[i])
        got = graphs[i]["elastic_tensor_full"]
        assert got.shape == (1, 21) and got.dtype == torch.float32
        assert np.abs(got.double().numpy() - want).max() <= 2.0 ** -23 * np.linalg.norm(x[i])
        assert abs(deviation[i] - want_dev[0]) <= 2.0 ** -23


# ----------------------------------------------------------------------------------------------------------------------
# adjoint, autograd, capture
# ----------------------------------------------------------------------------------------------------------------------
def test_adjoint_identity_and_autograd():
    from matten_amd import ops
    from matten_amd.symmetry import average_irreps, irreps_layout, rotate_irreps

    spec = cases.MIXED_IRREPS
    layout = irreps_layout(spec)
    n, dim = 37, 32
    R = dev(cases.rotations(12, seed=3))
    index = dev(np.random.default_rng(0).integers(0, 12, n), torch.int32)
    x, g = dev(cases.rows(n, dim, seed=1)), dev(cases.rows(n, dim, seed=2))
    D, flags = ops.wigner_d(R, 4)

    Dx = ops.irreps_rotate(x, layout, D, flags, index)
    Dtg = ops.irreps_rotate(g, layout, D, flags, index, transpose=True)
    lhs, rhs = (Dx * g).sum(dim=1), (x * Dtg).sum(dim=1)
    scale = x.norm(dim=1) * g.norm(dim=1)
    assert float(((lhs - rhs).abs() / scale).max()) <= 1e-12

    op_ptr = dev(np.concatenate([[0], np.cumsum(np.arange(n) % 4)]), torch.int64)          # lists of 0..3 operations
    nnz = int(op_ptr[-1])
    op_idx = dev(np.random.default_rng(1).integers(0, 12, nnz), torch.int32)
    w = dev(np.random.default_rng(2).uniform(0.2, 1.0, nnz))
    Ax, _ = ops.irreps_average(x, layout, D, flags, op_ptr, op_idx, w)
    Atg, none = ops.irreps_average(g, layout, D, flags, op_ptr, op_idx, w, transpose=True, want_deviation=False)
    assert none is None
    lhs, rhs = (Ax * g).sum(dim=1), (x * Atg).sum(dim=1)
    assert float(((lhs - rhs).abs() / scale).max()) <= 1e-12

    # autograd through both Functions is the transpose call, bit for bit
    xr = x.clone().requires_grad_(True)
    rotate_irreps(xr, spec, R, index=index).backward(g)
    assert torch.equal(xr.grad.view(torch.int64), Dtg.view(torch.int64))
    xa = x.clone().requires_grad_(True)
    avg, deviation = average_irreps(xa, spec, R, op_ptr, op_idx, w)
    assert not deviation.requires_grad and avg.requires_grad
    avg.backward(g)
    assert torch.equal(xa.grad.view(torch.int64), Atg.view(torch.int64))


def test_capture_and_replay_on_new_values():
    """wigner_D -> rotate -> average in one captured graph (a single chain, no parallel branches), replayed after x and R
    were overwritten in place: the same bits as the eager calls on the new values"""
    from matten_amd import ops
    from matten_amd.symmetry import irreps_layout

    f = "ijkl=jikl=klij"
    layout = irreps_layout(f)
    n, G = 50, 9
    R = dev(cases.rotations(G, seed=1))
    x = dev(cases.rows(n, 21, seed=1), torch.float32)
    index = dev(np.arange(n) % G, torch.int32)
    op_ptr = dev(np.arange(n + 1) * 2, torch.int64)
    op_idx = dev(np.arange(2 * n) % G, torch.int32)
    D, flags = torch.empty(G, 165, dtype=torch.float64, device=DEV), torch.empty(G, dtype=torch.int32, device=DEV)
    y, z = torch.empty_like(x), torch.empty_like(x)

    def chain():
        ops.wigner_d(R, 4, out=(D, flags))
        ops.irreps_rotate(x, layout, D, flags, index, out=y)
        return ops.irreps_average(y, layout, D, flags, op_ptr, op_idx, out=z)[1]

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        deviation = chain()
    R.copy_(dev(cases.rotations(G, seed=2)))
    x.copy_(dev(cases.rows(n, 21, seed=2), torch.float32))
    graph.replay()
    torch.cuda.synchronize()
    replayed = (y.clone(), z.clone(), deviation.clone(), D.clone())
    eager_dev = chain()
    for a, b in zip(replayed, (y, z, eager_dev, D)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert bool(torch.isfinite(z).all()) and float(eager_dev.max()) > 0.0


# ----------------------------------------------------------------------------------------------------------------------
# end to end
# ----------------------------------------------------------------------------------------------------------------------
def test_reference_equivariance_test_in_the_irreps_basis(golden_dir):
    """The fixture, seed and atol of test_gpu_parity.py::test_reference_equivariance_test_on_gpu, with the rotation applied
    on the device in the irreps basis.  In the report the irreps components are orthonormal combinations of the 81
    Cartesian ones, so |delta_irreps| <= |delta_cart|_F <= 9 max|delta_cart|: nine times allclose's atol + rtol max|y|."""
    from matten_amd.data.graph import collate, crystal_graph
    from matten_amd.predict import equivariance_report
    from matten_amd.symmetry import rotate_irreps
    from matten_amd.utils import ToCartesian
    from oracle.e3nn_lite import o3 as ro3
    from oracle.matten_ref.data import structures_from_json

    s = structures_from_json(os.path.join(golden_dir, "elastic_tensor_one.json"))[0]
    torch.manual_seed(35)
    Q = ro3.rand_matrix().double()
    g1 = crystal_graph(s["cart_coords"], s["lattice"], s["atomic_numbers"], 5.0)
    g2 = crystal_graph(s["cart_coords"] @ Q.numpy().T, s["lattice"] @ Q.numpy().T, s["atomic_numbers"], 5.0)
    _, model = build_pair(EQUIV_TEST, {"allowed_species": [8, 52]})
    f = "ijkl=jikl=klij"
    tc = ToCartesian(f)
    with torch.no_grad():
        y1 = model.backbone(collate([g1], device=DEV))["my_model_output"]
        y2 = model.backbone(collate([g2], device=DEV))["my_model_output"]
        assert y1.shape == (1, 21)
        x, o2 = tc(rotate_irreps(y1, f, Q.to(DEV)))[0].cpu(), tc(y2)[0].cpu()
    print(f"max|to_cartesian(D y1) - to_cartesian(y2)| = {(x - o2).abs().max():.3e} (max|y2| {o2.abs().max():.3e})")
    assert torch.allclose(x, o2, atol=1e-4)

    bound = 9.0 * (1e-4 + 1e-5 * float(o2.abs().max()))
    rep = equivariance_report(model, [s], rotations=Q.numpy()[None], r_cut=5.0, formula=f)
    print(f"report: worst_abs {rep['worst_abs']:.3e}, worst_rel {rep['worst_rel']:.3e} (bound on worst_abs {bound:.3e})")
    assert rep["max_abs"].shape == (1, 1) and rep["worst"] == (0, 0) and 0.0 < rep["worst_abs"] <= bound
    default = equivariance_report(model, s, formula=f)                 # two seeded proper rotations and an improper one
    print(f"default rotations: max_abs {default['max_abs']}, max_rel {default['max_rel']}")
    assert default["max_abs"].shape == (1, 3) and np.linalg.det(default["rotations"]).round().tolist() == [1.0, 1.0, -1.0]
    assert np.isfinite(default["max_abs"]).all() and default["worst_abs"] <= bound


def test_equivariance_report_of_per_atom_tensors():
    """One structure of the per-atom fixture (6 atoms) through the ATOMIC model and the per-atom ``index`` path, an
    improper rotation included.  Each of the two fp32 forwards lies within the parity tests' 2e-4 of the largest
    magnitude of the exact result, so the two differ by at most 4e-4 of it."""
    from matten_amd.predict import equivariance_report
    from test_atom_targets_host import fixture_dataset_hparams, fixture_graphs

    g = fixture_graphs("compact")[9]
    s = {"cart_coords": g["pos"].double().numpy(), "lattice": g["cell"].double().numpy().reshape(3, 3),
         "atomic_numbers": g["atomic_numbers"].numpy()}
    _, model = build_pair(dict(ATOMIC), fixture_dataset_hparams(), randomize_bn=True, atomic=True)
    rep = equivariance_report(model, [s], r_cut=5.0, formula="ij=ji", is_atomic_tensor=True)
    print(f"per-atom: max_abs {rep['max_abs']}, max_rel {rep['max_rel']}")
    assert rep["max_abs"].shape == (1, 3) and np.linalg.det(rep["rotations"][2]) < 0
    assert np.isfinite(rep["max_rel"]).all() and 0.0 < rep["worst_rel"] <= 4e-4
