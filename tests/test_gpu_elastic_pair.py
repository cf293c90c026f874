"""
Shear modulus and Poisson's ratio over pairs of perpendicular directions (matten_elastic_pair) and the Christoffel sound
velocities (matten_elastic_acoustic) on the GPU against numpy fp64.

As in test_gpu_elastic.py the reference is written out here -- np.linalg.inv, np.linalg.eigvalsh and the textbook
formulas -- and shares no code with matten_amd.elastic; closed forms of isotropic and cubic crystals pin the formulas.

Tolerances (derived, not measured; eps = 2^-52, FACTOR = 64, cond and S from numpy per crystal).  test_gpu_elastic.py
argues that both compliances lie within FACTOR eps cond max|S| of the true one, entry by entry.  Then
  1/G = w^T S w                   |d|       <= 16 FACTOR eps cond max|S|              (sum_I |w_I| <= 4)
  v(n)^T S v(m), v(n)^T S v(n)    |d|       <= 4 FACTOR eps cond max|S|  =: t         (sum_I |v_I| <= 2)
  nu = -num / den                 |d nu|    <= t (1 + |nu_ref|) E_ref(n)              (E_ref = 1 / den > 0 on the sets used)
  Christoffel eigenvalues         |d lam|   <= FACTOR eps 9 max|C_IJ|                 (|Gamma_ik| <= 3 max|C|, so
                                  ||Gamma||_2 <= 9 max|C|; Jacobi and LAPACK are both backward stable)
  velocities                      rel       <= 1/2 d lam / lam
  v_mean                          rel       <= 1/2 max_d (d lam / lam_min(d)) + D eps
  sum of v^-3                     rel       <= 3 times that of v_mean                  (d v^-3 / v^-3 = 3 dv / v)
The Debye temperature is three roundings and a cube root away from v_mean: 16 eps relative.
"""
import json
import os

import numpy as np
import pytest
import torch

from common import LMAX2

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EPS = 2.0 ** -52
FACTOR = 64.0
PAIRS = ((0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1))     # pymatgen's Voigt order: xx, yy, zz, yz, xz, xy
VOIGT = np.array([[0, 5, 4], [5, 1, 3], [4, 3, 2]])          # Cartesian pair -> Voigt index
UNIT = 1e9                                                   # Pa per unit of the tensors (GPa)
HBAR, K_B = 6.62607015e-34 / (2 * np.pi), 1.380649e-23       # exact SI

PAIR_FIELDS = ("shear_min", "shear_max", "poisson_min", "poisson_max")
PAIR_MAPS = ("shear_dir_min", "shear_dir_max", "poisson_dir_min", "poisson_dir_max")
ACOUSTIC_FIELDS = ("v_slow_min", "v_fast_max", "sum_inv_v3", "v_mean")
# the keys of to_dict() before the pair and acoustic properties existed
OLD_KEYS = ("voigt", "compliance", "k_voigt", "g_voigt", "k_reuss", "g_reuss", "k_vrh", "g_vrh", "y_mod", "homogeneous_poisson",
            "universal_anisotropy", "pugh_ratio", "flags", "is_stable", "is_singular")
OLD_DIRECTIONAL_KEYS = ("young", "compressibility", "young_min", "young_max", "young_argmin", "young_argmax",
                        "compressibility_min", "compressibility_max", "compressibility_argmin", "compressibility_argmax",
                        "directions")
PAIR_KEYS = ("angles",) + PAIR_FIELDS + tuple(f + s for f in PAIR_FIELDS for s in ("_direction", "_angle")) + PAIR_MAPS
ACOUSTIC_KEYS = ACOUSTIC_FIELDS + ("velocities", "v_slow_min_direction", "v_fast_max_direction", "acoustic_unstable_directions")


# ---------------------------------------------------------------------------------------------------
# the reference: numpy fp64
# ---------------------------------------------------------------------------------------------------
def voigt_picks(c4):
    return np.array([[c4[i, j, k, l] for (k, l) in PAIRS] for (i, j) in PAIRS], dtype=np.float64)


def six(a):
    """v(a) [..,6] of vectors a [..,3]"""
    return np.stack([a[..., 0] ** 2, a[..., 1] ** 2, a[..., 2] ** 2, a[..., 1] * a[..., 2], a[..., 0] * a[..., 2],
                     a[..., 0] * a[..., 1]], axis=-1)


def six_pair(n, m):
    """w(n, m) [..,6]"""
    return np.stack([2 * n[..., 0] * m[..., 0], 2 * n[..., 1] * m[..., 1], 2 * n[..., 2] * m[..., 2],
                     n[..., 1] * m[..., 2] + n[..., 2] * m[..., 1], n[..., 0] * m[..., 2] + n[..., 2] * m[..., 0],
                     n[..., 0] * m[..., 1] + n[..., 1] * m[..., 0]], axis=-1)


def ref_frame(n):
    """the branch-free orthonormal frame (e1, e2) of unit vectors n [D,3]"""
    n1, n2, n3 = n[:, 0], n[:, 1], n[:, 2]
    s = np.where(n3 >= 0, 1.0, -1.0)
    a = -1.0 / (s + n3)
    b = n1 * n2 * a
    return (np.stack([1 + s * n1 * n1 * a, s * b, -s * n1], axis=1), np.stack([b, s + n2 * n2 * a, -n2], axis=1))


def ref_angles(M):
    chi = np.pi * np.arange(M, dtype=np.float64) / M
    return chi, np.stack([np.cos(chi), np.sin(chi)], axis=1)


def ref_pairs(S, n, table):
    """S [6,6], n [D,3], table [M,2] = (cos, sin) -> (1/G [D,M], nu [D,M], 1/E [D])"""
    e1, e2 = ref_frame(n)
    m = table[None, :, 0, None] * e1[:, None, :] + table[None, :, 1, None] * e2[:, None, :]        # [D,M,3]
    nn = np.broadcast_to(n[:, None, :], m.shape)
    w = six_pair(nn, m)
    vn, vm = six(n), six(m)
    q = np.einsum("di,ij,dj->d", vn, S, vn)
    return np.einsum("dki,ij,dkj->dk", w, S, w), -np.einsum("di,ij,dkj->dk", vn, S, vm) / q[:, None], q


def ref_christoffel(C, n):
    """C [6,6], n [D,3] -> the eigenvalues of Gamma_ik = C_ijkl n_j n_l, ascending [D,3]"""
    c4 = C[VOIGT[:, :, None, None], VOIGT[None, None, :, :]]
    return np.linalg.eigvalsh(np.einsum("ijkl,dj,dl->dik", c4, n, n))


def tol_inv_g(C):
    return 16 * FACTOR * EPS * np.linalg.cond(C) * np.abs(np.linalg.inv(C)).max()


def tol_nu(C, nu_ref, q_ref):
    """[D,M] for nu_ref [D,M] and q_ref = 1 / E_ref [D]"""
    return 4 * FACTOR * EPS * np.linalg.cond(C) * np.abs(np.linalg.inv(C)).max() * (1 + np.abs(nu_ref)) / q_ref[:, None]


def tol_lambda(C):
    return FACTOR * EPS * 9 * np.abs(C).max()


def velocities_of(lam, rho):
    return np.sqrt(lam * UNIT / rho)


def check_pair_maps(d, b, C, n, M, what):
    """the kept per-direction maps of row b against the reference; the crystal's extremes against the maps"""
    S = np.linalg.inv(C)
    h, nu, q = ref_pairs(S, n, ref_angles(M)[1])
    assert (q > 0).all() and (h > 0).all(), what
    tg, tn = tol_inv_g(C), tol_nu(C, nu, q)
    err_g = max(np.abs(1 / d["shear_dir_min"][b] - h.max(axis=1)).max(), np.abs(1 / d["shear_dir_max"][b] - h.min(axis=1)).max())
    err_n = max((np.abs(d["poisson_dir_min"][b] - nu.min(axis=1)) / tn.max(axis=1)).max(),
                (np.abs(d["poisson_dir_max"][b] - nu.max(axis=1)) / tn.max(axis=1)).max())
    print(f"{what} row {b}: 1/G error {err_g / tg:.3g} of its bound, nu error {err_n:.3g} of its bound")
    assert err_g <= tg, (what, b, err_g, tg)
    assert err_n <= 1.0, (what, b, err_n)
    # the extremes are entries of the maps, numpy's first occurrence; the pair reported is right: the reference there
    # lies within the bound of the reference's extreme
    for name, ref, ref_pick, tol in (("shear_min", h, np.max, tg), ("shear_max", h, np.min, tg),
                                     ("poisson_min", nu, np.min, None), ("poisson_max", nu, np.max, None)):
        arr = d[name.replace("_m", "_dir_m")][b]
        at_d, at_k = int(d[name + "_direction"][b]), int(d[name + "_angle"][b])
        assert 0 <= at_d < n.shape[0] and 0 <= at_k < M, (what, b, name)
        assert d[name][b] == (arr.min() if name.endswith("min") else arr.max()), (what, b, name)
        assert at_d == int(np.argmin(arr) if name.endswith("min") else np.argmax(arr)), (what, b, name)
        assert abs(ref[at_d, at_k] - ref_pick(ref)) <= (tn[at_d, at_k] if tol is None else tol), (what, b, name)


def check_velocity_maps(d, b, C, n, rho, what):
    lam = ref_christoffel(C, n)
    assert (lam > 0).all(), what
    tl = tol_lambda(C)
    want = velocities_of(lam, rho)
    got = d["velocities"][b]
    rel = np.abs(got - want) / want
    print(f"{what} row {b}: velocity error {(rel / (0.5 * tl / lam)).max():.3g} of its bound")
    assert (rel <= 0.5 * tl / lam).all(), (what, b)
    assert (np.diff(got, axis=1) >= 0).all()                                    # ascending
    D = n.shape[0]
    assert d["v_slow_min"][b] == got[:, 0].min() and d["v_slow_min_direction"][b] == int(np.argmin(got[:, 0]))
    assert d["v_fast_max"][b] == got[:, 2].max() and d["v_fast_max_direction"][b] == int(np.argmax(got[:, 2]))
    assert d["acoustic_unstable_directions"][b] == 0
    v_mean = ((want ** -3.0).sum() / (3 * D)) ** (-1.0 / 3.0)
    tm = 0.5 * (tl / lam[:, 0]).max() + D * EPS
    assert abs(d["v_mean"][b] - v_mean) <= tm * v_mean, (what, b, d["v_mean"][b], v_mean)
    assert abs(d["sum_inv_v3"][b] - (want ** -3.0).sum()) <= 3 * tm * (want ** -3.0).sum()


# ---------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture_set(golden_dir):
    """the 100 tensors of the example data set, rounded to fp32: (Cartesian fp32 [100,3,3,3,3], Voigt fp64 [100,6,6]),
    and a density per crystal (2 to 12 g/cm^3, in kg/m^3)"""
    raw = json.load(open(os.path.join(golden_dir, "example_crystal_elasticity_tensor_n100.json")))
    keys = sorted(raw["elastic_tensor_full"], key=int)
    full = np.array([raw["elastic_tensor_full"][k] for k in keys], dtype=np.float64)
    cart32 = full.astype(np.float32)
    C = np.stack([voigt_picks(t) for t in cart32.astype(np.float64)])
    assert all(np.array_equal(c, c.T) and np.linalg.eigvalsh(c).min() > 0 for c in C)
    rho = 2000.0 + 101.0 * np.arange(100)
    return cart32, C, rho


def _elastic():
    from matten_amd import elastic

    return elastic


def _cubic(c11, c12, c44):
    C = np.zeros((6, 6))
    C[:3, :3] = c12
    C[[0, 1, 2], [0, 1, 2]] = c11
    C[[3, 4, 5], [3, 4, 5]] = c44
    return C


def _same(a, b, keys=None, rows=None):
    """bit-identical dicts (NaN = NaN), optionally rows `rows` of a against b"""
    for k in (keys or a):
        x, y = a[k], b[k]
        if x is None or y is None:
            assert x is None and y is None, k
            continue
        if rows is not None and k not in ("directions", "angles"):
            x = x[rows]
        assert np.array_equal(x, y, equal_nan=x.dtype.kind == "f"), k


def pair_values(C, n, chi):
    """G and nu at the explicit pairs (n_d, m = cos chi e1(n_d) + sin chi e2(n_d)): the kernel with a one-row angle table,
    whose per-direction minimum and maximum are then the value itself -> (G [B,D], nu [B,D])"""
    from matten_amd import ops

    p = _elastic().elastic_properties(C)
    table = torch.tensor([[np.cos(chi), np.sin(chi)]], dtype=torch.float64, device=DEV)
    maps, _, arg = ops.elastic_pair(p.compliance, p.flags, torch.from_numpy(np.ascontiguousarray(n)).to(DEV), table, keep=True)
    maps = maps.cpu().numpy()
    assert np.array_equal(maps[:, :, 0], maps[:, :, 1]) and np.array_equal(maps[:, :, 2], maps[:, :, 3])
    return maps[:, :, 0], maps[:, :, 2]


# ---------------------------------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3, 100])
def test_fixture_set(fixture_set, B):
    E = _elastic()
    cart32, C, rho = fixture_set
    D, M = 65, 7
    p = E.elastic_properties(cart32[:B], directions=D, keep_directional=True, angles=M, density=rho[:B])
    on = torch.device(DEV).type                                                 # the results stay on the device
    assert p.shear_min.device.type == on and p.velocities.device.type == on
    assert p.shear_dir_min.shape == (B, D) and p.velocities.shape == (B, D, 3)
    d = p.to_dict()
    n = d["directions"]
    assert np.array_equal(d["angles"], ref_angles(M)[0])
    for b in range(B):
        check_pair_maps(d, b, C[b], n, M, f"fixture set, B={B}")
        check_velocity_maps(d, b, C[b], n, rho[b], f"fixture set, B={B}")
    if B == 100:
        assert (d["poisson_min"] < 0).any()          # auxetic directions exist in the example data set
        print(f"fixture set: poisson_min down to {d['poisson_min'].min():.3f}, {(d['poisson_min'] < 0).sum()} crystals below 0")
    # the Voigt route on the device gives the same maps within the bounds (checked against the same reference)
    q = E.elastic_properties(torch.from_numpy(C[:B]).to(DEV), directions=D, keep_directional=True, angles=M,
                             density=torch.from_numpy(rho[:B]).to(DEV)).to_dict()
    for b in range(min(B, 3)):
        check_pair_maps(q, b, C[b], n, M, f"fixture set (Voigt fp64), B={B}")
        check_velocity_maps(q, b, C[b], n, rho[b], f"fixture set (Voigt fp64), B={B}")
    # an unbatched tensor: no leading dimension, a scalar density
    one = E.elastic_properties(cart32[0], directions=D, keep_directional=True, angles=M, density=float(rho[0]),
                               number_density=5e28)
    assert one.shear_min.shape == () and one.shear_dir_min.shape == (D,) and one.velocities.shape == (D, 3)
    assert one.angles.shape == (M,) and one.debye_temperature.shape == ()
    assert float(one.shear_min) == d["shear_min"][0] and float(one.v_mean) == d["v_mean"][0]


@pytest.mark.parametrize("M", [1, 2, 7])
@pytest.mark.parametrize("D", [1, 63, 64, 65, 256, 257])
def test_loop_edges(fixture_set, D, M):
    """the wave (64) and workgroup (256) edges of the direction loop, and the shortest angle loops"""
    E = _elastic()
    C, rho = fixture_set[1][[0, 17, 58]], fixture_set[2][[0, 17, 58]]
    nd = np.array([4.0e28, 6.5e28, 9.0e28])
    kw = dict(directions=D, angles=M, density=rho, number_density=nd)
    d = E.elastic_properties(C, keep_directional=True, **kw).to_dict()
    assert set(d) == set(OLD_KEYS + OLD_DIRECTIONAL_KEYS + PAIR_KEYS + ACOUSTIC_KEYS + ("debye_temperature",))
    n = d["directions"]
    for b in range(3):
        check_pair_maps(d, b, C[b], n, M, f"D={D} M={M}")
        check_velocity_maps(d, b, C[b], n, rho[b], f"D={D} M={M}")
    # a second run gives the same bits; without keep_directional the maps are not kept and the rest is the same bits
    _same(d, E.elastic_properties(C, keep_directional=True, **kw).to_dict())
    lean = E.elastic_properties(C, **kw)
    kept = PAIR_MAPS + ("velocities", "young", "compressibility")
    assert all(getattr(lean, k) is None for k in kept)
    _same(d, lean.to_dict(), keys=[k for k in d if k not in kept])
    # a row alone is the same row inside the batch, the sums included
    for b in range(3):
        alone = E.elastic_properties(C[b : b + 1], keep_directional=True, directions=D, angles=M, density=rho[b : b + 1],
                                     number_density=nd[b : b + 1]).to_dict()
        _same(d, alone, rows=slice(b, b + 1))


def test_ties_resolve_to_the_lowest_flat_index(fixture_set):
    E = _elastic()
    C, rho = fixture_set[1][[5, 23, 77]], fixture_set[2][[5, 23, 77]]
    base = E.fibonacci_hemisphere(150)
    n = np.concatenate([base, base, base[:40]])              # 340 directions: copies in other waves and other strides
    M = 3
    d = E.elastic_properties(C, directions=n, keep_directional=True, angles=M, density=rho).to_dict()
    for b in range(3):
        for k in PAIR_MAPS:
            assert np.array_equal(d[k][b][:150], d[k][b][150:300])
        assert np.array_equal(d["velocities"][b][:150], d["velocities"][b][150:300])
        for name in PAIR_FIELDS:
            arr = d[name.replace("_m", "_dir_m")][b]
            first = int(np.argmin(arr) if name.endswith("min") else np.argmax(arr))
            assert d[name + "_direction"][b] == first < 150, (b, name)
        assert d["v_slow_min_direction"][b] == int(np.argmin(d["velocities"][b][:, 0])) < 150
        assert d["v_fast_max_direction"][b] == int(np.argmax(d["velocities"][b][:, 2])) < 150
    # all directions the same: the lowest direction wins everywhere, and the angle is the first of its kind
    same = E.elastic_properties(C, directions=np.tile([[0.3, -0.5, 0.8]], (300, 1)), angles=M, density=rho).to_dict()
    one = E.elastic_properties(C, directions=np.array([[0.3, -0.5, 0.8]]), angles=M, density=rho).to_dict()
    for name in PAIR_FIELDS:
        assert (same[name + "_direction"] == 0).all(), name
        assert np.array_equal(same[name + "_angle"], one[name + "_angle"]) and np.array_equal(same[name], one[name]), name
    assert (same["v_slow_min_direction"] == 0).all() and (same["v_fast_max_direction"] == 0).all()
    # one direction 70 times over and one angle three times over (the table itself repeats its row): flat index 0 wins
    from matten_amd import ops

    p = E.elastic_properties(_cubic(168.0, 121.0, 75.0)[None])
    table = torch.tensor([[0.6, 0.8], [0.6, 0.8], [0.6, 0.8]], dtype=torch.float64, device=DEV)
    nn = torch.tensor(np.tile([[0.0, 0.6, 0.8]], (70, 1)), dtype=torch.float64, device=DEV)
    _, _, arg = ops.elastic_pair(p.compliance, p.flags, nn, table)
    assert (arg.cpu().numpy() == 0).all()


def test_closed_forms_isotropic():
    E = _elastic()
    KG = [(160.0, 80.0), (75.5, 26.0), (3.0, 11.0), (1234.5, 0.75)]
    C = np.stack([_cubic(K + 4 * G / 3, K - 2 * G / 3, G) for K, G in KG])
    rho = np.array([2700.0, 7800.0, 1850.0, 11340.0])
    nd = np.array([6.0e28, 8.5e28, 1.2e29, 3.3e28])
    D = 65
    p = E.elastic_properties(C, directions=D, keep_directional=True, angles=7, density=rho, number_density=nd).to_dict()
    for b, (K, G) in enumerate(KG):
        nu = (3 * K - 2 * G) / (2 * (3 * K + G))
        young = 9 * K * G / (3 * K + G)
        tg = tol_inv_g(C[b])
        tn = tol_inv_g(C[b]) / 4 * (1 + abs(nu)) * young
        for k in ("shear_dir_min", "shear_dir_max"):
            assert np.abs(1 / p[k][b] - 1 / G).max() <= tg, (b, k)
        for k in ("poisson_dir_min", "poisson_dir_max"):
            assert np.abs(p[k][b] - nu).max() <= tn, (b, k)
        assert abs(1 / p["shear_min"][b] - 1 / G) <= tg and abs(1 / p["shear_max"][b] - 1 / G) <= tg
        assert abs(p["poisson_min"][b] - nu) <= tn and abs(p["poisson_max"][b] - nu) <= tn
        # rho v^2 = G, G, K + 4G/3 in every direction
        lam = np.array([G, G, K + 4 * G / 3])
        want = velocities_of(lam, rho[b])
        tl = tol_lambda(C[b])
        assert (np.abs(p["velocities"][b] - want) <= 0.5 * tl / lam * want).all(), b
        vt, vl = want[0], want[2]
        v_mean = ((2 / vt ** 3 + 1 / vl ** 3) / 3) ** (-1.0 / 3.0)
        tm = 0.5 * tl / lam[0] + D * EPS
        assert abs(p["v_mean"][b] - v_mean) <= tm * v_mean, (b, p["v_mean"][b], v_mean)
        assert abs(p["v_slow_min"][b] - vt) <= 0.5 * tl / lam[0] * vt and abs(p["v_fast_max"][b] - vl) <= 0.5 * tl / lam[2] * vl
        assert p["acoustic_unstable_directions"][b] == 0
        theta = (HBAR / K_B) * (6 * np.pi ** 2 * nd[b]) ** (1.0 / 3.0)
        assert abs(p["debye_temperature"][b] - theta * p["v_mean"][b]) <= 16 * EPS * theta * p["v_mean"][b]
        assert abs(p["debye_temperature"][b] - theta * v_mean) <= (tm + 16 * EPS) * theta * v_mean
    # modulus_unit: the same tensors in Pa with modulus_unit = 1 give the same velocities within the bound
    q = E.elastic_properties(C * 1e9, directions=D, keep_directional=True, density=rho, modulus_unit=1.0).to_dict()
    for b, (K, G) in enumerate(KG):
        assert (np.abs(q["velocities"][b] - p["velocities"][b]) <= tol_lambda(C[b]) / G * p["velocities"][b]).all()


def test_closed_forms_cubic():
    E = _elastic()
    cubic = [(168.0, 121.0, 75.0), (108.0, 62.0, 28.0), (250.0, 20.0, 130.0), (50.0, 30.0, 4.0)]
    C = np.stack([_cubic(*c) for c in cubic])
    rho = np.array([8960.0, 2700.0, 3500.0, 970.0])
    r2, r3 = np.sqrt(0.5), np.sqrt(1.0 / 3.0)
    n = np.array([[1.0, 0.0, 0.0], [r2, r2, 0.0], [r3, r3, r3]])
    # the frames: e2([100]) = [010]; ([110]/sqrt 2)'s e1 - e2 is [1-10], i.e. m at chi = 3 pi / 4 is -[1-10]/sqrt 2
    e1, e2 = ref_frame(n)
    assert np.allclose(e2[0], [0, 1, 0], atol=1e-15)
    assert np.allclose((np.cos(0.75 * np.pi) * e1[1] + np.sin(0.75 * np.pi) * e2[1]), [-r2, r2, 0], atol=1e-15)
    g_a, nu_a = pair_values(C, n, 0.5 * np.pi)
    g_b, nu_b = pair_values(C, n, 0.75 * np.pi)
    vel = E.elastic_properties(C, directions=n, keep_directional=True, density=rho).to_dict()["velocities"]
    for b, (c11, c12, c44) in enumerate(cubic):
        det = (c11 - c12) * (c11 + 2 * c12)
        s11, s12, s44 = (c11 + c12) / det, -c12 / det, 1 / c44
        tg = tol_inv_g(C[b])
        t = tg / 4
        # G([100],[010]) = c44, G([110],[1-10]) = (c11 - c12) / 2
        assert abs(1 / g_a[b, 0] - 1 / c44) <= tg, (b, g_a[b, 0])
        assert abs(1 / g_b[b, 1] - 2 / (c11 - c12)) <= tg, (b, g_b[b, 1])
        # nu([100],[010]) = c12 / (c11 + c12), nu([110],[1-10]) = -(S11 + S12 - S44/2) / (S11 + S12 + S44/2)
        want = c12 / (c11 + c12)
        assert abs(nu_a[b, 0] - want) <= t * (1 + abs(want)) / s11, (b, nu_a[b, 0], want)
        want = -(s11 + s12 - s44 / 2) / (s11 + s12 + s44 / 2)
        assert abs(nu_b[b, 1] - want) <= t * (1 + abs(want)) / (0.5 * (s11 + s12 + s44 / 2)), (b, nu_b[b, 1], want)
        # rho v^2 along [100], [110], [111]
        tl = tol_lambda(C[b])
        for dd, lam in ((0, [c44, c44, c11]), (1, [c44, (c11 - c12) / 2, (c11 + c12 + 2 * c44) / 2]),
                        (2, [(c11 - c12 + c44) / 3, (c11 - c12 + c44) / 3, (c11 + 2 * c12 + 4 * c44) / 3])):
            lam = np.sort(np.array(lam))
            want = velocities_of(lam, rho[b])
            assert (np.abs(vel[b, dd] - want) <= 0.5 * tl / lam * want).all(), (b, dd, vel[b, dd], want)
    # the public route with angles = 4 holds both pairs: [110]'s extremes over chi bracket the anchor
    p = E.elastic_properties(C, directions=n, keep_directional=True, angles=4).to_dict()
    for b, (c11, c12, c44) in enumerate(cubic):
        tg = tol_inv_g(C[b])
        assert abs(1 / p["shear_dir_min"][b, 0] - 1 / c44) <= tg and abs(1 / p["shear_dir_max"][b, 0] - 1 / c44) <= tg
        lo, hi = sorted([1 / c44, 2 / (c11 - c12)])
        assert abs(1 / p["shear_dir_max"][b, 1] - lo) <= tg and abs(1 / p["shear_dir_min"][b, 1] - hi) <= tg


def _rotation(seed):
    q, r = np.linalg.qr(np.random.default_rng(seed).standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def test_rotation_invariance(fixture_set):
    """the tensor and the directions rotated together.  The frame of a rotated n is not the rotated frame, so G and nu are
    compared at explicit pairs: (n, m = e1(n)) against (R n, R m), R m expressed by its angle in the frame of R n."""
    E = _elastic()
    n = E.fibonacci_hemisphere(48)
    for b, seed in ((3, 1), (41, 2)):
        t = fixture_set[0][b].astype(np.float64)
        C, rho = fixture_set[1][b], fixture_set[2][b]
        R = _rotation(seed)
        rot = np.einsum("ia,jb,kc,ld,abcd->ijkl", R, R, R, R, t)
        nr = n @ R.T
        p = E.elastic_properties(t, directions=n, keep_directional=True, density=rho).to_dict()
        q = E.elastic_properties(rot, directions=nr, keep_directional=True, density=rho).to_dict()
        # the rotated tensor is itself rounded (81-term sums, a few eps of max|C|): the same bounds cover it
        lam = ref_christoffel(C, n)
        tl = tol_lambda(C)
        assert (np.abs(p["velocities"] - q["velocities"]) <= 0.5 * tl / lam * p["velocities"]).all()
        tm = 0.5 * (tl / lam[:, 0]).max() + 48 * EPS
        assert abs(p["v_mean"] - q["v_mean"]) <= tm * p["v_mean"]
        assert abs(p["v_slow_min"] - q["v_slow_min"]) <= 0.5 * (tl / lam[:, 0]).max() * p["v_slow_min"]
        assert abs(p["v_fast_max"] - q["v_fast_max"]) <= 0.5 * (tl / lam[:, 2]).max() * p["v_fast_max"]
        # pairs
        S = np.linalg.inv(C)
        h, nu, den = ref_pairs(S, n, np.array([[1.0, 0.0]]))
        tg, tn = tol_inv_g(C), tol_nu(C, nu, den)
        g0, nu0 = pair_values(t[None], n, 0.0)
        e1, _ = ref_frame(n)
        f1, f2 = ref_frame(nr)
        mr = e1 @ R.T
        chi = np.arctan2((mr * f2).sum(axis=1), (mr * f1).sum(axis=1))
        for dd in (0, 7, 19, 30, 47):
            g1, nu1 = pair_values(rot[None], nr[dd : dd + 1], chi[dd])
            assert abs(1 / g1[0, 0] - 1 / g0[0, dd]) <= tg, (b, dd)
            assert abs(nu1[0, 0] - nu0[0, dd]) <= tn[dd, 0], (b, dd)
            assert abs(1 / g0[0, dd] - h[dd, 0]) <= tg and abs(nu0[0, dd] - nu[dd, 0]) <= tn[dd, 0]


def test_singular_non_finite_and_indefinite_rows(fixture_set):
    E = _elastic()
    Cs, rho_all = fixture_set[1], fixture_set[2]
    # row 1 singular, row 3 non-finite, row 5 indefinite in some directions only ((c11 - c12) / 2 < 0 along [110])
    C = np.stack([Cs[0], np.zeros((6, 6)), Cs[1], Cs[4].copy(), Cs[2], _cubic(100.0, 120.0, 50.0), Cs[3]])
    C[3, 2, 4] = C[3, 4, 2] = np.nan
    rho = rho_all[:7].copy()
    nd = np.full(7, 5e28)
    D, M = 70, 3
    n = np.concatenate([np.eye(3), np.array([[1.0, 1.0, 0.0], [1.0, 1.0, 1.0]]), E.fibonacci_hemisphere(D - 5)])
    kw = dict(directions=n, keep_directional=True, angles=M)
    d = E.elastic_properties(C, density=rho, number_density=nd, **kw).to_dict()
    n = d["directions"]
    assert list(d["flags"] & 1) == [0, 1, 0, 1, 0, 0, 0]
    for b in (1, 3):
        for k in PAIR_FIELDS + PAIR_MAPS + ACOUSTIC_FIELDS + ("velocities", "debye_temperature"):
            assert np.isnan(d[k][b]).all(), (b, k)
        for k in tuple(f + s for f in PAIR_FIELDS for s in ("_direction", "_angle")) + \
                ("v_slow_min_direction", "v_fast_max_direction", "acoustic_unstable_directions"):
            assert d[k][b] == -1, (b, k)
    # the indefinite row: unstable directions are counted and NaN, the extremes run over the finite velocities only
    lam = ref_christoffel(C[5], n)
    tl = tol_lambda(C[5])
    surely_bad, maybe_bad = (lam[:, 0] < -tl), (lam[:, 0] <= tl)
    assert surely_bad[3] and not maybe_bad[0]                                    # [110] is unstable, [100] is not
    bad = np.isnan(d["velocities"][5]).any(axis=1)
    assert np.array_equal(bad, np.isnan(d["velocities"][5]).all(axis=1))
    assert (bad[surely_bad]).all() and not (bad[~maybe_bad]).any()
    assert d["acoustic_unstable_directions"][5] == bad.sum() > 0
    assert np.isnan(d["v_mean"][5]) and np.isnan(d["sum_inv_v3"][5]) and np.isnan(d["debye_temperature"][5])
    v = d["velocities"][5]
    assert d["v_slow_min"][5] == np.nanmin(v[:, 0]) and d["v_slow_min_direction"][5] == int(np.nanargmin(v[:, 0]))
    assert d["v_fast_max"][5] == np.nanmax(v[:, 2]) and d["v_fast_max_direction"][5] == int(np.nanargmax(v[:, 2]))
    good = ~bad
    want = velocities_of(lam[good], rho[5])
    assert (np.abs(v[good] - want) <= 0.5 * tl / lam[good] * want).all()
    assert (d["flags"][5] & 2) and np.isfinite(d["shear_min"][5]) and np.isfinite(d["poisson_max"][5])
    # the valid rows next to them are what they are on their own
    rows = [0, 2, 4, 6]
    alone = E.elastic_properties(C[rows], density=rho[rows], number_density=nd[rows], **kw).to_dict()
    _same(d, alone, rows=rows)
    for i, b in enumerate(rows):
        check_pair_maps(alone, i, C[b], n, M, "rows next to singular ones")
        check_velocity_maps(alone, i, C[b], n, rho[b], "rows next to singular ones")
    # a density on the device is not checked on the host: a bad entry makes its row's acoustic fields NaN and -1, nothing else
    bad_rho = torch.tensor([rho[0], -1.0, float("nan"), float("inf"), 0.0], dtype=torch.float64, device=DEV)
    e = E.elastic_properties(Cs[:5], density=bad_rho, **kw).to_dict()
    f = E.elastic_properties(Cs[:5], density=np.full(5, rho[0]), **kw).to_dict()
    for b in range(1, 5):
        for k in ACOUSTIC_FIELDS + ("velocities",):
            assert np.isnan(e[k][b]).all(), (b, k)
        for k in ("v_slow_min_direction", "v_fast_max_direction", "acoustic_unstable_directions"):
            assert e[k][b] == -1, (b, k)
    _same(e, f, keys=[k for k in e if k not in ACOUSTIC_KEYS])
    for k in ACOUSTIC_KEYS:
        assert np.array_equal(e[k][0], f[k][0]), k


def test_predict_with_pair_and_acoustic_properties(golden_dir):
    import warnings as W

    from matten_amd import predict as P
    from matten_amd.model_factory.tfn_scalar_tensor import ScalarTensorModel
    from oracle.matten_ref import data as rdata

    E = _elastic()
    structs = rdata.structures_from_json(os.path.join(golden_dir, "example_crystal_elasticity_tensor_n100.json"))
    structs = sorted(structs, key=lambda s: len(s["atomic_numbers"]))[:4]
    structs = [{k: s[k] for k in ("lattice", "cart_coords", "atomic_numbers")} for s in structs]
    z0 = int(structs[0]["atomic_numbers"][0])
    edgeless = {"lattice": 50.0 * np.eye(3), "cart_coords": np.zeros((1, 3)), "atomic_numbers": np.array([z0])}
    structs = structs[:2] + [edgeless] + structs[2:]
    rho = [2330.0, 5320.0, 1000.0, 7870.0, 3510.0]
    ds = {"allowed_species": list(range(1, 95)), "average_num_neighbors": 18.0}
    torch.manual_seed(35)
    model = ScalarTensorModel(backbone_hparams=dict(LMAX2), dataset_hparams=ds).to(DEV).eval()
    cfg = {"data": {"r_cut": 5.0, "tensor_target_name": "elastic_tensor_full", "tensor_target_formula": "ijkl=jikl=klij"}}
    kw = dict(directions=33, angles=5, density=rho)
    with W.catch_warnings():
        W.simplefilter("ignore")
        plain = P.predict(structs, model=model, config=cfg)
        tensors, props = P.predict(structs, model=model, config=cfg, properties=True, **kw)
        with_rho = [dict(s, density=r) for s, r in zip(structs, rho)]
        _, from_structs = P.predict(with_rho, model=model, config=cfg, properties=True, directions=33, angles=5,
                                    density="structure", number_density=[5e28] * 5)
    assert len(plain) == len(tensors) == 5 and plain[2] is None and tensors[2] is None
    for i in (0, 1, 3, 4):
        assert type(tensors[i]) is type(plain[i]) and np.array_equal(np.asarray(tensors[i]), np.asarray(plain[i]))
    want = E.elastic_properties([None if t is None else np.asarray(t) for t in plain], **kw).to_dict()
    got = props.to_dict()
    assert set(got) == set(want) == set(OLD_KEYS + OLD_DIRECTIONAL_KEYS + PAIR_KEYS + ACOUSTIC_KEYS)
    _same(got, want)
    assert got["flags"][2] & 4 and got["flags"][2] & 1 and not (got["flags"][[0, 1, 3, 4]] & 5).any()
    for k in PAIR_FIELDS + ACOUSTIC_FIELDS:
        assert np.isnan(got[k][2]), k
    for k in ("shear_min_direction", "poisson_max_angle", "v_fast_max_direction", "acoustic_unstable_directions"):
        assert got[k][2] == -1, k
    assert np.isfinite(got["shear_min"][[0, 1, 3, 4]]).all()
    # density="structure" reads the dicts' "density": the same bits, and the Debye temperature on top
    second = from_structs.to_dict()
    _same(got, second, keys=list(got))
    assert "debye_temperature" in second and np.isnan(second["debye_temperature"][2])
    with pytest.raises(ValueError, match=r"\[1, 4\]"):
        P.predict([with_rho[0], structs[1], with_rho[2], with_rho[3], structs[4]], model=model, config=cfg, properties=True,
                  directions=33, density="structure")


def test_without_the_new_arguments_nothing_changes(fixture_set):
    """the keys of to_dict() are the earlier ones unless angles / density are given; each new argument adds its own"""
    E = _elastic()
    C, rho = fixture_set[1][:4], fixture_set[2][:4]
    assert tuple(E.elastic_properties(C).to_dict()) == OLD_KEYS
    base = E.elastic_properties(C, directions=9, keep_directional=True).to_dict()
    assert tuple(base) == OLD_KEYS + OLD_DIRECTIONAL_KEYS
    pair = E.elastic_properties(C, directions=9, keep_directional=True, angles=2).to_dict()
    assert set(pair) == set(OLD_KEYS + OLD_DIRECTIONAL_KEYS + PAIR_KEYS)
    ac = E.elastic_properties(C, directions=9, keep_directional=True, density=rho).to_dict()
    assert set(ac) == set(OLD_KEYS + OLD_DIRECTIONAL_KEYS + ACOUSTIC_KEYS)
    # and the earlier fields keep their bits next to the new ones
    _same(base, pair, keys=list(base))
    _same(base, ac, keys=list(base))
