"""Shared inputs of tests/test_symmetry_host.py and tests/test_gpu_symmetry.py: the Cartesian formulas, three point groups
from their generators, and seeded rotations with the edge cases (identity, inversion, a rotation by pi, improper ones, one
1e-7 off orthogonal)."""
import functools

import numpy as np

FORMULAS = ("ijkl=jikl=klij", "ij=ji", "ij", "ij=-ji", "ijk=ikj", "ijk=jik", "i")
MIXED_IRREPS = "3x0e+2x1o+1x2o+2x4e"      # columns of several degrees, multiplicities and parities, no l = 3


def rot_z(t: float) -> np.ndarray:
    c, s = np.cos(t), np.sin(t)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


C3_111 = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])      # the 3-fold axis [111]
C2_X = np.diag([1.0, -1.0, -1.0])
INVERSION = -np.eye(3)

GENERATORS = {
    "cubic": ([rot_z(np.pi / 2), C3_111, INVERSION], 48),           # m-3m
    "hexagonal": ([rot_z(np.pi / 3), C2_X, INVERSION], 24),         # 6/mmm
    "tetrahedral": ([rot_z(np.pi), C3_111], 12),                    # 23
}


@functools.lru_cache(maxsize=None)
def group(name: str) -> np.ndarray:
    from matten_amd.symmetry import group_closure

    ops = group_closure(GENERATORS[name][0])
    ops.setflags(write=False)
    return ops


def random_rotations(n: int, seed: int) -> np.ndarray:
    """n proper rotations (QR of Gaussian matrices, signs fixed), [n,3,3] fp64"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        q, r = np.linalg.qr(rng.standard_normal((3, 3)))
        q = q * np.sign(np.diag(r))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
        out.append(q)
    return np.stack(out)


def rotations(n: int, seed: int = 0) -> np.ndarray:
    """n >= 8 orthogonal matrices: the identity, -1, a rotation by pi about a skew axis, a mirror, then random proper and
    (every third) improper ones"""
    assert n >= 8
    axis = np.array([1.0, 2.0, -2.0]) / 3.0
    fixed = [np.eye(3), INVERSION, 2.0 * np.outer(axis, axis) - np.eye(3), np.diag([1.0, 1.0, -1.0])]
    R = random_rotations(n - len(fixed), seed)
    R[::3] *= -1.0
    return np.concatenate([np.stack(fixed), R])


def nearly_orthogonal(seed: int = 3) -> np.ndarray:
    """a rotation with one entry 1e-7 off: inside the default orth_tol = 1e-6"""
    M = random_rotations(1, seed)[0].copy()
    M[0, 1] += 1e-7
    return M


def skewed(seed: int = 4) -> np.ndarray:
    """a rotation with one entry 1e-3 off: flagged"""
    M = random_rotations(1, seed)[0].copy()
    M[2, 0] += 1e-3
    return M


def rows(n: int, dim: int, seed: int) -> np.ndarray:
    """n rows of irreps components with row norms spread over six decades"""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, dim)) * 10.0 ** rng.uniform(-3, 3, (n, 1))
