"""
CPU tests of the rotations and symmetry averages of irreps tensors (matten_amd/symmetry.py): the library's three entries
(declared, bound, exported, ABI 47, bad arguments refused without a device), ``group_closure``, the numpy restatements
built on the Kronecker definition D_f(M) = Qf (M x ... x M) Qf^T against the oracle's least-squares Wigner-D, the
projections onto cubic and hexagonal symmetry, the constants of csrc/rotate.hip, and the argument checks.  The GPU tests
(tests/test_gpu_symmetry.py) hold the kernels to the restatements tested here and share tests/symmetry_cases.py.
"""
import os
import re

import numpy as np
import pytest
import torch

import symmetry_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("matten_wigner_d", "matten_irreps_rotate", "matten_irreps_average")


# ----------------------------------------------------------------------------------------------------------------------
# the library
# ----------------------------------------------------------------------------------------------------------------------
def test_library_declares_binds_and_exports_the_entries():
    from matten_amd import _lib

    header = open(os.path.join(ROOT, "include", "matten_hip.h")).read()
    declared = set(re.findall(r"\b(matten_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for name in ENTRIES:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert _lib.ABI_VERSION == 47 and lib.matten_abi_version() == 47          # entries were only added
    assert [len(_lib.SIGNATURES[n][1]) for n in ENTRIES] == [7, 13, 16]
    assert "rotate.hip" in open(os.path.join(ROOT, "matten_amd", "csrc", "Makefile")).read()
    assert "tests/model/test_tfn_tensor.py:98-139" in header and "utils.py:110-133" in header


def test_bad_arguments_come_back_without_a_device():
    from matten_amd import _lib

    lib = _lib.load()
    wig, rot, avg = lib.matten_wigner_d, lib.matten_irreps_rotate, lib.matten_irreps_average
    p = 4096      # never dereferenced: every call below returns from the checks
    lay = (np.array([[0, 2, 0, 1], [2, 2, 2, 1], [12, 1, 4, 1]], dtype=np.int32))          # 2x0e+2x2e+4e, dim 21
    L = lay.ctypes.data

    # no-ops
    assert wig(None, 0, 4, 1e-6, None, None, None) == 0
    assert rot(None, 1, 0, 21, L, 3, None, None, None, 1, 0, None, None) == 0
    assert rot(p, 1, 5, 21, L, 3, None, None, None, 0, 0, p, None) == 0                  # G = 0
    assert avg(None, 1, 0, 21, L, 3, None, None, 0, None, None, None, 0, None, None, None) == 0

    # matten_wigner_d
    for bad in ((p, -1, 4, 1e-6, p, p), (p, 3, -1, 1e-6, p, p), (p, 3, 5, 1e-6, p, p), (p, 3, 4, float("nan"), p, p),
                (None, 3, 4, 1e-6, p, p), (p, 3, 4, 1e-6, None, p), (p, 3, 4, 1e-6, p, None)):
        assert wig(*bad, None) == -1, bad

    # matten_irreps_rotate: x, is_fp64, n, dim, layout, K, D, flags, index, G, transpose, out
    good = [p, 1, 5, 21, L, 3, p, p, None, 1, 0, p]
    for k, v in ((1, 2), (1, -1), (2, -1), (3, -1), (5, -1), (5, 17), (9, -1), (10, 2), (10, -1), (0, None), (6, None),
                 (7, None), (11, None), (4, None), (9, 3), (3, 20)):      # (9, 3): no index and G neither 1 nor n; dim 20: 4e past dim
        args = list(good)
        args[k] = v
        assert rot(*args, None) == -1, (k, v)
    for two in ([[0, 2, 2, 1], [9, 1, 4, 1]], [[0, 1, 4, 1], [0, 1, 0, 1]], [[5, 1, 1, -1], [3, 1, 1, 1]]):      # overlapping rows
        both = np.array(two, dtype=np.int32)
        assert rot(p, 1, 5, 21, both.ctypes.data, 2, p, p, None, 1, 0, p, None) == -1, two
        assert avg(p, 1, 5, 21, both.ctypes.data, 2, p, p, 4, p, p, None, 0, p, None, None) == -1, two
    touching = np.array([[0, 0, 4, 1], [0, 2, 2, 1], [10, 1, 4, 1]], dtype=np.int32)      # an empty row and neighbours: fine
    assert rot(p, 1, 0, 21, touching.ctypes.data, 3, p, p, None, 1, 0, p, None) == 0
    for row in ([0, 1, 5, 1], [0, 1, -1, 1], [0, 1, 2, 0], [0, 1, 2, 2], [-1, 1, 2, 1], [0, -1, 2, 1], [20, 1, 1, -1]):
        one = np.array([row], dtype=np.int32)
        assert rot(p, 1, 5, 21, one.ctypes.data, 1, p, p, None, 1, 0, p, None) == -1, row
        assert avg(p, 1, 5, 21, one.ctypes.data, 1, p, p, 4, p, p, None, 0, p, None, None) == -1, row

    # matten_irreps_average: x, is_fp64, n, dim, layout, K, D, flags, G, op_ptr, op_idx, weights, transpose, out, deviation
    good = [p, 0, 5, 21, L, 3, p, p, 4, p, p, None, 0, p, None]
    for k, v in ((1, 2), (2, -1), (3, -1), (5, -1), (5, 17), (8, -1), (12, 2), (0, None), (6, None), (7, None), (9, None),
                 (10, None), (13, None), (4, None)):
        args = list(good)
        args[k] = v
        assert avg(*args, None) == -1, (k, v)


def test_rotate_hip_constants_invert_the_harmonics():
    """The points P and the matrices W of csrc/rotate.hip, read from the source: W must be the inverse transpose of
    A[k][i] = Y_l,i(p_k) (the oracle's harmonics), and D = B^T W with B[k][i] = Y_l,i(R p_k) -- the kernel's method, in
    numpy -- must agree with the Kronecker restatement.  Conditioning as the file says (<= 5)."""
    from matten_amd.symmetry import wigner_D_host
    from oracle.e3nn_lite import o3 as ro3

    src = open(os.path.join(ROOT, "matten_amd", "csrc", "rotate.hip")).read()
    R = cases.rotations(12, seed=1)
    R = R[np.linalg.det(R) > 0]
    for l in (1, 2, 3, 4):
        n = 2 * l + 1
        body = re.search(r"struct RotTab<%d> \{(.*?)\n\};" % l, src, re.S).group(1)
        P = re.search(r"P\[%d\]\[3\] = \{(.*?)\n    \};" % n, body, re.S).group(1)
        W = re.search(r"W\[%d\]\[%d\] = \{(.*?)\n    \};" % (n, n), body, re.S).group(1)
        P = np.array([float(v) for v in re.findall(r"-?\d\.?\d*(?:e-?\d+)?", P)]).reshape(n, 3)
        W = np.array([float(v) for v in re.findall(r"-?\d\.?\d*(?:e-?\d+)?", W)]).reshape(n, n)
        assert np.abs(np.linalg.norm(P, axis=1) - 1.0).max() < 1e-15

        def Y(v):
            return ro3.spherical_harmonics([l], torch.from_numpy(v), True, "component").numpy()

        A = Y(P)
        assert np.linalg.cond(A) <= 5.0
        assert np.abs(A.T @ W - np.eye(n)).max() < 1e-14
        for M in R:
            D = Y(P @ M.T).T @ W
            assert np.abs(D - wigner_D_host(l, M)[0]).max() < 1e-13, l


# ----------------------------------------------------------------------------------------------------------------------
# group_closure
# ----------------------------------------------------------------------------------------------------------------------
def test_group_closure_orders_and_polish():
    from matten_amd.symmetry import group_closure

    for name, (gens, order) in cases.GENERATORS.items():
        ops = cases.group(name)
        assert ops.shape == (order, 3, 3) and np.array_equal(ops[0], np.eye(3)), name
        assert np.abs(np.einsum("gki,gkj->gij", ops, ops) - np.eye(3)).max() <= 1e-15, name
        # closed: every product is an element
        prod = np.einsum("aij,bjk->abik", ops, ops).reshape(-1, 1, 3, 3)
        assert (np.abs(prod - ops[None]).max(axis=(2, 3)).min(axis=1) < 1e-12).all(), name
    # generators as read from a file at 1e-6 come back orthogonal to rounding, in the same order
    rng = np.random.default_rng(0)
    noisy = [g + 1e-6 * rng.uniform(-1, 1, (3, 3)) for g in cases.GENERATORS["cubic"][0]]
    ops = group_closure(noisy, tol=1e-4)
    assert len(ops) == 48 and np.abs(np.einsum("gki,gkj->gij", ops, ops) - np.eye(3)).max() <= 1e-15
    # a rotation by an angle incommensurate with pi never closes
    with pytest.raises(ValueError, match="max_order"):
        group_closure([cases.rot_z(1.0)], max_order=192)
    with pytest.raises(ValueError, match="max_order"):
        group_closure(cases.GENERATORS["cubic"][0], max_order=47)
    with pytest.raises(ValueError, match="orthogonal"):
        group_closure([np.diag([1.0, 2.0, 1.0])], orthonormalize=False)


# ----------------------------------------------------------------------------------------------------------------------
# the restatements
# ----------------------------------------------------------------------------------------------------------------------
def test_host_restatement_is_block_diagonal_with_the_parity_rule():
    """D_f(M) of every formula, proper and improper M, is block diagonal over the irreps, and the block of (l, p) is
    p^[det M < 0] D^l(det(M) M) with D^l the oracle's least-squares Wigner-D of the model's harmonics, at 1e-12."""
    from matten_amd.symmetry import formula_D_host, irreps_D_host, irreps_of, wigner_D_host
    from oracle.e3nn_lite import o3 as ro3

    R = cases.rotations(10, seed=2)
    assert (np.linalg.det(R) < 0).sum() >= 3
    sh = {(l, k): ro3.wigner_D_from_sh(l, torch.from_numpy(np.linalg.det(M) * M)).numpy() for l in range(5) for k, M in enumerate(R)}
    seen = set()
    for f in cases.FORMULAS:
        irreps = irreps_of(f)
        D = formula_D_host(f, R)
        mask = np.zeros((irreps.dim, irreps.dim), dtype=bool)
        for off, b in zip(irreps.offsets(), irreps):
            for u in range(b.mul):
                lo, hi = off + u * b.ir.dim, off + (u + 1) * b.ir.dim
                mask[lo:hi, lo:hi] = True
                seen.add((b.ir.l, b.ir.p))
                for k, M in enumerate(R):
                    want = sh[b.ir.l, k] * (b.ir.p if np.linalg.det(M) < 0 else 1)
                    assert np.abs(D[k, lo:hi, lo:hi] - want).max() <= 1e-12, (f, b, k)
        assert np.abs(D[:, ~mask]).max(initial=0.0) <= 1e-14, f
        assert np.abs(D - irreps_D_host(f, R)).max() <= 1e-14, f
    assert {(2, -1), (1, 1), (3, -1)} <= seen          # the determinant factor is exercised: 2o, 1e, 3o
    for l in range(5):
        for p in (1, -1):
            got = wigner_D_host(l, R, p)
            for k, M in enumerate(R):
                assert np.abs(got[k] - sh[l, k] * (p if np.linalg.det(M) < 0 else 1)).max() <= 1e-12


def test_homomorphism_and_orthogonality():
    from matten_amd.symmetry import irreps_D_host, wigner_D_host

    R = cases.rotations(9, seed=5)
    for l in range(5):
        for p in (None, 1, -1):
            D = wigner_D_host(l, R, p)
            assert np.abs(np.einsum("gki,gkj->gij", D, D) - np.eye(2 * l + 1)).max() <= 1e-13
            for a in range(len(R)):
                b = (a + 3) % len(R)
                assert np.abs(wigner_D_host(l, R[a] @ R[b], p)[0] - D[a] @ D[b]).max() <= 1e-13, (l, p, a)
    D = irreps_D_host(cases.MIXED_IRREPS, R)
    assert np.abs(irreps_D_host(cases.MIXED_IRREPS, R[1] @ R[5])[0] - D[1] @ D[5]).max() <= 1e-13


def test_cubic_and_hexagonal_projections_of_an_elastic_tensor():
    from matten_amd import o3
    from matten_amd.symmetry import average_irreps_host, formula_D_host

    f = "ijkl=jikl=klij"
    _, Q = o3.cartesian_tensor_basis(f)
    x = cases.rows(1, 21, seed=7)
    for name, rank in (("cubic", 3), ("hexagonal", 5)):
        ops = cases.group(name)
        P = formula_D_host(f, ops).mean(axis=0)
        assert np.linalg.matrix_rank(P, tol=1e-10) == rank, name
        assert np.abs(P @ P - P).max() <= 1e-13 and np.abs(P - P.T).max() <= 1e-13          # an orthogonal projection
        avg, dev = average_irreps_host(x, f, ops)
        assert np.abs(avg[0] - P @ x[0]).max() <= 1e-12 * np.linalg.norm(x)
        again, dev2 = average_irreps_host(avg, f, ops)
        assert np.abs(again - avg).max() <= 1e-12 * np.linalg.norm(x) and dev2[0] <= 1e-12 and 0.1 < dev[0] < 1.0   # idempotent
        for M in ops[1::7]:
            assert np.abs(formula_D_host(f, M)[0] @ avg[0] - avg[0]).max() <= 1e-12 * np.linalg.norm(x)              # invariant
    avg, _ = average_irreps_host(x, f, cases.group("cubic"))
    C = np.einsum("qijkl,q->ijkl", Q, avg[0])
    voigt = [(0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1)]
    V = np.array([[C[a + b] for b in voigt] for a in voigt])
    tol = 1e-12 * np.abs(V).max()
    assert abs(V[0, 0] - V[1, 1]) <= tol and abs(V[0, 0] - V[2, 2]) <= tol
    assert abs(V[0, 1] - V[0, 2]) <= tol and abs(V[0, 1] - V[1, 2]) <= tol
    assert abs(V[3, 3] - V[4, 4]) <= tol and abs(V[3, 3] - V[5, 5]) <= tol
    rest = V.copy()
    rest[:3, :3] = 0.0
    rest[[3, 4, 5], [3, 4, 5]] = 0.0
    assert np.abs(rest).max() <= tol and min(abs(V[0, 0]), abs(V[0, 1]), abs(V[3, 3])) > 1e3 * tol


def test_average_host_row_states_and_weights():
    from matten_amd.symmetry import average_irreps_host, rotate_irreps_host

    f = "ij=ji"
    x = cases.rows(6, 6, seed=9)
    x[5] = 0.0
    R = np.concatenate([cases.rotations(8, seed=1), cases.skewed()[None]])
    op_ptr = np.array([0, 0, 1, 3, 5, 7, 9])
    op_idx = np.array([2, 3, 4, 5, 8, 6, 7, 0, 1])
    w = np.array([2.0, 1.0, 3.0, 1.0, 1.0, 1.0, -1.0, 0.5, 0.5])
    avg, dev = average_irreps_host(x, f, R, op_ptr, op_idx, w)
    assert np.array_equal(avg[0], x[0]) and dev[0] == 0.0                                    # the trivial group
    assert np.allclose(avg[1], rotate_irreps_host(x[1], f, R[2])[0], rtol=0, atol=1e-12 * np.linalg.norm(x[1]))
    want = (rotate_irreps_host(x[2], f, R[3])[0] + 3.0 * rotate_irreps_host(x[2], f, R[4])[0]) / 4.0
    assert np.allclose(avg[2], want, rtol=0, atol=1e-12 * np.linalg.norm(x[2]))
    assert np.isnan(avg[3]).all() and np.isnan(dev[3])                                       # a flagged operation
    assert np.isnan(avg[4]).all() and np.isnan(dev[4])                                       # sum of weights 0
    assert np.array_equal(avg[5], x[5]) and dev[5] == 0.0                                    # a zero row
    bad = w.copy()
    bad[1] = np.inf
    assert np.isnan(average_irreps_host(x, f, R, op_ptr, op_idx, bad)[0][2]).all()
    for outside in (-1, len(R)):                                                             # an operation outside R
        idx = op_idx.copy()
        idx[1] = outside
        a, d = average_irreps_host(x, f, R, op_ptr, idx, w)
        assert np.isnan(a[2]).all() and np.isnan(d[2]) and np.isfinite(a[1]).all()


# ----------------------------------------------------------------------------------------------------------------------
# layouts and argument checks
# ----------------------------------------------------------------------------------------------------------------------
def test_layout_matches_the_irreps_offsets():
    from matten_amd import o3
    from matten_amd.symmetry import irreps_layout, irreps_of

    for spec in cases.FORMULAS + (cases.MIXED_IRREPS, "32x0o+32x0e+16x1o"):
        irreps = irreps_of(spec)
        lay = irreps_layout(spec)
        assert lay.dtype == np.int32 and lay.shape == (len(irreps), 4)
        assert lay[:, 0].tolist() == irreps.offsets()
        assert [tuple(r[1:]) for r in lay.tolist()] == [(b.mul, b.ir.l, b.ir.p) for b in irreps]
        assert lay[-1, 0] + lay[-1, 1] * (2 * lay[-1, 2] + 1) == irreps.dim
    assert irreps_of("ijkl=jikl=klij") == o3.Irreps("2x0e+2x2e+4e") and irreps_of(o3.Irreps("1o")) == o3.Irreps("1o")
    with pytest.raises(ValueError, match="l > 4"):
        irreps_layout("2x5e")


def test_cpu_tensors_are_refused():
    from matten_amd import _lib
    from matten_amd.symmetry import average_irreps, rotate_irreps, symmetrize_irreps, wigner_D

    R = torch.from_numpy(cases.rotations(8))
    x = torch.zeros(4, 21)
    with pytest.raises(_lib.MattenHipError, match="no CPU fallback"):
        wigner_D(2, R)
    with pytest.raises(_lib.MattenHipError, match="no CPU fallback"):
        rotate_irreps(x, "ijkl=jikl=klij", R[0])
    with pytest.raises(_lib.MattenHipError, match="no CPU fallback"):
        average_irreps(x, "ijkl=jikl=klij", R)
    with pytest.raises(_lib.MattenHipError, match="no CPU fallback"):
        symmetrize_irreps(x, "ijkl=jikl=klij", R)
    with pytest.raises(ValueError, match="columns"):
        rotate_irreps(torch.zeros(4, 6), "ijkl=jikl=klij", R[0])
    with pytest.raises(ValueError, match="0..4"):
        wigner_D(5, R)
    import matten.symmetry as alias
    import matten_amd.symmetry as real

    assert alias is real


def test_equivariance_report_signature():
    import inspect

    from matten_amd import predict as P

    params = inspect.signature(P.equivariance_report).parameters
    assert list(params) == ["model", "structures", "rotations", "n_random", "seed", "r_cut", "formula", "is_atomic_tensor"]
    assert params["rotations"].default is None and params["n_random"].default == 2 and params["seed"].default == 0
    assert params["is_atomic_tensor"].default is False
