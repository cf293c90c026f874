"""
The tensors the polycrystal tests share (tests/test_polycrystal_host.py, tests/test_gpu_polycrystal.py): closed-form cases and
the one batch of 257 Voigt matrices the device is compared on.  numpy only.
"""
import numpy as np

# copper-like cubic constants (c11, c12, c44) and the closed forms that go with them
COPPER = (168.4, 121.4, 75.4)


def cubic(c11, c12, c44):
    C = np.zeros((6, 6))
    C[:3, :3] = c12
    C[[0, 1, 2], [0, 1, 2]] = c11
    C[[3, 4, 5], [3, 4, 5]] = c44
    return C


def isotropic(K, G):
    return cubic(K + 4.0 * G / 3.0, K - 2.0 * G / 3.0, G)


def hexagonal(c11, c12, c13, c33, c44):
    C = np.zeros((6, 6))
    C[0, 0] = C[1, 1] = c11
    C[0, 1] = C[1, 0] = c12
    C[0, 2] = C[2, 0] = C[1, 2] = C[2, 1] = c13
    C[2, 2] = c33
    C[3, 3] = C[4, 4] = c44
    C[5, 5] = 0.5 * (c11 - c12)
    return C


def cubic_closed_forms(c11, c12, c44):
    """-> (K, mu1, mu2, F_G(K, mu1), F_G(K, mu2), g_sc): Hashin & Shtrikman's closed forms for a cubic crystal and the root
    of Kroener's cubic 8G^3 + (9K + 4 mu1) G^2 - 3 mu2 (K + 4 mu1) G - 6 K mu1 mu2 = 0"""
    K, m1, m2 = (c11 + 2.0 * c12) / 3.0, 0.5 * (c11 - c12), c44
    b1 = -3.0 * (K + 2.0 * m1) / (5.0 * m1 * (3.0 * K + 4.0 * m1))
    b2 = -3.0 * (K + 2.0 * m2) / (5.0 * m2 * (3.0 * K + 4.0 * m2))
    g1 = m1 + 3.0 / (5.0 / (m2 - m1) - 4.0 * b1)
    g2 = m2 + 2.0 / (5.0 / (m1 - m2) - 6.0 * b2)
    roots = np.roots([8.0, 9.0 * K + 4.0 * m1, -3.0 * m2 * (K + 4.0 * m1), -6.0 * K * m1 * m2])
    g_sc = float(max(r.real for r in roots if abs(r.imag) < 1e-9 * abs(r.real) and r.real > 0.0))
    return K, m1, m2, g1, g2, g_sc


def random_definite(n: int, seed: int) -> np.ndarray:
    """n positive definite matrices A A^T + s 1, s in 10^[-2, 1]: condition numbers up to several hundred"""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((n, 6, 6))
    s = 10.0 ** rng.uniform(-2.0, 1.0, size=n)
    return A @ A.transpose(0, 2, 1) + s[:, None, None] * np.eye(6)


def rotation_voigt(R):
    """the 6x6 matrix that rotates a Voigt stiffness matrix: C' = Q C Q^T (Bond's matrix for the stress)"""
    Q = np.zeros((6, 6))
    pairs = ((0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1))
    for I, (i, j) in enumerate(pairs):
        for J, (k, l) in enumerate(pairs):
            Q[I, J] = R[i, k] * R[j, l] if k == l else R[i, k] * R[j, l] + R[i, l] * R[j, k]
    return Q


N_BATCH = 257          # more than one workgroup of 64, not a multiple of the wave
ROW_ISOTROPIC, ROW_CUBIC, ROW_CUBIC_SWAPPED, ROW_HEXAGONAL, ROW_TRICLINIC = 0, 1, 2, 3, 4
ROW_NEAR_SINGULAR, ROW_NOT_PD, ROW_NAN = 254, 255, 256


def batch() -> np.ndarray:
    """[257,6,6]: the isotropic tensor, both cubic cases (mu1 < mu2 and mu1 > mu2), a hexagonal tensor (zinc-like), 250
    seeded triclinic tensors, one near-singular row (condition number 1e6), one row that is not positive definite and one
    NaN row"""
    C = np.empty((N_BATCH, 6, 6))
    C[ROW_ISOTROPIC] = isotropic(160.0, 80.0)
    C[ROW_CUBIC] = cubic(*COPPER)
    C[ROW_CUBIC_SWAPPED] = cubic(250.0, 60.0, 40.0)
    C[ROW_HEXAGONAL] = hexagonal(165.0, 31.1, 50.0, 61.8, 39.6)
    C[ROW_TRICLINIC:ROW_NEAR_SINGULAR] = random_definite(250, 20240)
    rng = np.random.default_rng(7)
    Q, _ = np.linalg.qr(rng.standard_normal((6, 6)))
    C[ROW_NEAR_SINGULAR] = (Q * np.array([1e-6, 0.3, 0.5, 0.7, 0.9, 1.0])) @ Q.T * 100.0
    C[ROW_NOT_PD] = (Q * np.array([-0.2, 0.3, 0.5, 0.7, 0.9, 1.0])) @ Q.T * 100.0
    C[ROW_NAN] = C[ROW_CUBIC]
    C[ROW_NAN, 2, 3] = np.nan
    return 0.5 * (C + C.transpose(0, 2, 1))
