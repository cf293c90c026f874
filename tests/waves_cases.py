"""
The crystals of the acoustic-wave tests (test_waves_host.py, test_gpu_waves.py) and the error bounds the device result is
held to.  One builder, so both files talk about the same six tensors:

  two random triclinic tensors   symmetric 6x6, unit Gaussian entries plus 6 on the diagonal (seed 0)
  cubic Cu                       c11, c12, c44 = 168.4, 121.4, 75.4
  cubic Al                       107.3, 60.9, 28.3
  a hexagonal tensor             c11 165, c12 31, c13 50, c33 62, c44 40, c66 = (c11 - c12) / 2
  nearly isotropic W             522.4, 204.4, 160.6

all at density 1 kg/m^3 and modulus_unit 1 unless a test says otherwise.

Error bounds (derived, not measured; eps = 2^-52, FACTOR = 64; M = max|C_IJ|, s = modulus_unit / density,
D_km = |lambda_k - lambda_m|, D_k = gap_k lambda_2 = min_m D_km).  Two sizes of a contraction of C with unit vectors a, b, c:
  R = 9 M      bounds sum |C_ijkl| |a_j| |b_k| |c_l| per component, so FACTOR eps R is the rounding of one contraction
  N = mu_max   the largest |Kelvin modulus| (eigenvalue of the Mandel matrix) bounds its 2-norm: sym(a b) has Frobenius
               norm <= 1, so |C : sym(a b)|_F <= mu_max, and so is that stress applied to c.  |Gamma| <= N, |dGamma| <= 2 N.
Jacobi and LAPACK are both backward stable, so, as in test_gpu_elastic_pair.py,
  eigenvalues          |d lam|  <= FACTOR eps R                                                   =: dl
  eigenvectors         |d u_k|  <= 2 dl / D_k                                                     =: du_k
and everything else is these two carried through the formulas, first order, each contraction also rounded (r = FACTOR
eps R times the unit vectors' sizes):
  v = sqrt(lam s)      rel      <= dl / (2 lam_k) + 2 eps                                          =: rv
  character (u.n)^2    |d|      <= 2 du_k
  P = C u u n          |d P|    <= 2 N du_k + r
  g = (s / v) P        |d g|    <= (s / v) |d P| + |g| rv                                          =: dg  (also of |g|)
  psi = acos(c), c = min(1, v / |g|):  |d c| <= c (rv + dg / |g|) =: dc, and acos on [0, 1] moves by at most
                       min(dc / sqrt(1 - min(1, c + dc)^2), acos(1 - dc))  (mean value; the steepest stretch ends at 1)
  du = sum_m u_m (u_m^T dGamma u_k) / (lam_k - lam_m),  |du| <= sum_m 2 N / D_km =: A
                       |d du|   <= sum_m ((2 N / D_km) (2 du_m + du_k + 2 dl / D_km) + 2 r / D_km)  =: ddu
                       (the 1 / (lam_k - lam_m) of du once more: in du_m, du_k and in the denominators)
  dlam = u^T dGamma u  |d|      <= 2 N 2 du_k + 2 r;   dv = s dlam / (2 v), |dv| <= s N / v,
                       |d dv|   <= s |d dlam| / (2 v) + (s N / v) rv
  dP                   |dP|     <= N (2 A + 1),   |d dP| <= 2 N (ddu + A du_k) + 2 N du_k + r (2 A + 1)
  dg = s dP / v - g dv / v     |dg'| <= (s / v) N (2 A + 1) + |g| s N / v^2 =: Gd,
                       |d dg'|  <= (s / v) |d dP| + (s / v) N (2 A + 1) rv + (dg s N / v + |g| |d dv|) / v
                                   + |g| (s N / v^2) rv + FACTOR eps Gd
  g^ = g / |g|         |d g^|   <= 2 dg / |g|
  dg^ = (dg' - g^ (g^.dg')) / |g|    |dg^| <= Gd / |g| =: H,
                       |d dg^|  <= (2 |d dg'| + 2 |d g^| Gd) / |g| + H dg / |g| + FACTOR eps H
  J = g^ . (d1 g^ x d2 g^)     |d J| <= |d g^| H^2 + 2 H |d dg^| + FACTOR eps H^2
A branch k whose two partners are degenerate with each other (the longitudinal branch of an isotropic tensor): u_m, m != k,
are then arbitrary in their plane and du_m says nothing, but du_k needs only their projector,
sum_m u_m u_m^T / (lam_k - lam_m) = (1 - u_k u_k^T) / (lam_k - lam_t) up to the partners' split (<= 2 dl, the 2 dl / D_km
above), and 1 - u_k u_k^T moves by 2 du_k plus the orthonormality of Jacobi's U (15 rotations of a few eps: 4 FACTOR eps).
``bounds(..., partners_degenerate=True)`` puts du_k + 4 FACTOR eps where du_m stands in ddu.
"""
import numpy as np

EPS = 2.0 ** -52
FACTOR = 64.0
DEG_TOL = 1e-6
NAMES = ("tri0", "tri1", "Cu", "Al", "hex", "W")


def cubic(c11, c12, c44):
    C = np.zeros((6, 6))
    C[:3, :3] = c12
    C[np.arange(3), np.arange(3)] = c11
    C[np.arange(3, 6), np.arange(3, 6)] = c44
    return C


def hexagonal(c11, c12, c13, c33, c44):
    C = np.zeros((6, 6))
    C[0, 0] = C[1, 1] = c11
    C[0, 1] = C[1, 0] = c12
    C[0, 2] = C[2, 0] = C[1, 2] = C[2, 1] = c13
    C[2, 2] = c33
    C[3, 3] = C[4, 4] = c44
    C[5, 5] = 0.5 * (c11 - c12)
    return C


def isotropic(K, G):
    return cubic(K + 4.0 * G / 3.0, K - 2.0 * G / 3.0, G)


def random_triclinic(n, seed=0):
    X = np.random.default_rng(seed).standard_normal((n, 6, 6))
    return 0.5 * (X + X.transpose(0, 2, 1)) + 6.0 * np.eye(6)


def crystals():
    """[6,6,6] fp64 Voigt matrices in the order of NAMES"""
    tri = random_triclinic(2)
    return np.stack([tri[0], tri[1], cubic(168.4, 121.4, 75.4), cubic(107.3, 60.9, 28.3),
                     hexagonal(165.0, 31.0, 50.0, 62.0, 40.0), cubic(522.4, 204.4, 160.6)])


def bounds(C, s, host, b=None, partners_degenerate=False):
    """The error bounds of the module docstring for crystal C [6,6] at scale s, from the host result (row b of a batched
    one) -> dict of arrays [D,3]: lam, u, v (absolute), character, g, psi, J"""
    pick = (lambda a: a) if b is None else (lambda a: a[b])
    v = pick(host["phase_velocity"])
    g_abs, psi = pick(host["group_speed"]), pick(host["power_flow_angle"])
    lam = v * v / s
    R = 9.0 * np.abs(C).max()
    w = np.where(np.arange(6) < 3, 1.0, np.sqrt(2.0))
    N = np.abs(np.linalg.eigvalsh(w[:, None] * (0.5 * (C + C.T)) * w[None, :])).max()
    fe = FACTOR * EPS
    dl, r = fe * R, fe * R
    D = np.abs(lam[:, :, None] - lam[:, None, :])                       # [D,k,m]
    D = np.where(np.eye(3, dtype=bool)[None], np.inf, D)
    du = 2.0 * dl / D.min(axis=2)                                       # [D,k]
    rv = dl / (2.0 * lam) + 2.0 * EPS
    dP = 2.0 * N * du + r
    dg = (s / v) * dP + g_abs * rv
    c = np.minimum(1.0, v / g_abs)
    dc = c * (rv + dg / g_abs)
    with np.errstate(divide="ignore", invalid="ignore"):
        slope = dc / np.sqrt(1.0 - np.minimum(1.0, c + dc) ** 2)
    dpsi = np.minimum(slope, np.arccos(np.maximum(-1.0, 1.0 - dc)))
    A = (2.0 * N / D).sum(axis=2)
    du_m = du[:, :, None] + 4.0 * fe if partners_degenerate else du[:, None, :]
    ddu = ((2.0 * N / D) * (2.0 * du_m + du[:, :, None] + 2.0 * dl / D) + 2.0 * r / D).sum(axis=2)
    d_dlam = 4.0 * N * du + 2.0 * r
    d_dv = s * d_dlam / (2.0 * v) + (s * N / v) * rv
    d_dP = 2.0 * N * (ddu + A * du) + 2.0 * N * du + r * (2.0 * A + 1.0)
    Gd = (s / v) * N * (2.0 * A + 1.0) + g_abs * s * N / (v * v)
    d_dg = ((s / v) * d_dP + (s / v) * N * (2.0 * A + 1.0) * rv + (dg * s * N / v + g_abs * d_dv) / v
            + g_abs * (s * N / (v * v)) * rv + fe * Gd)
    dgh = 2.0 * dg / g_abs
    H = Gd / g_abs
    d_dgh = (2.0 * d_dg + 2.0 * dgh * Gd) / g_abs + H * dg / g_abs + fe * H
    dJ = dgh * H * H + 2.0 * H * d_dgh + fe * H * H
    return dict(lam=np.full_like(lam, dl), u=du, v=v * rv, character=2.0 * du, g=dg, psi=dpsi, J=dJ, R=R, N=N)
