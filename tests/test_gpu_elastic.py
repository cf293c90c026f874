"""
Derived elastic properties on the GPU (matten_amd/elastic.py over csrc/elastic.hip) against numpy fp64.

The reference for every number is written out here -- np.linalg.inv and the textbook formulas -- and shares no code
with matten_amd.elastic; closed forms of isotropic and cubic crystals, which need no inverse at all, pin the formulas.

Tolerance (derived, not measured).  Gaussian elimination with partial pivoting on a 6x6 is backward stable, and so is
LAPACK's: each inverse is the exact inverse of a matrix within a few eps of C, so both lie within c eps cond(C) of the
true compliance, c a small multiple of the dimension.  With eps = 2^-52 and cond(C) from numpy per crystal:
  compliance entries              |dS|  <= 64 eps cond max|S|
  every scalar but the anisotropy  rel  <= 64 eps cond
  universal_anisotropy (a difference that vanishes for isotropic crystals)
                                  |dA|  <= 64 eps cond (5 |g_voigt / g_reuss| + |k_voigt / k_reuss| + 6)
  v^T S v and beta(n)             |d|   <= 4 * 64 eps cond max|S|     (sum_I |v_I| <= 2, so sum_IJ |v_I||v_J| <= 4)
numpy against 50-digit arithmetic stays within 4.6 eps cond on these inputs; the factor 64 is room for another
elimination order.  fp32 inputs convert to fp64 exactly, so the reference is given the same fp32-rounded values.
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
NAMES = ("k_voigt", "g_voigt", "k_reuss", "g_reuss", "k_vrh", "g_vrh", "y_mod", "homogeneous_poisson",
         "universal_anisotropy", "pugh_ratio")


# ---------------------------------------------------------------------------------------------------
# the reference: numpy fp64
# ---------------------------------------------------------------------------------------------------
def voigt_picks(c4):
    return np.array([[c4[i, j, k, l] for (k, l) in PAIRS] for (i, j) in PAIRS], dtype=np.float64)


def symmetrise_cartesian(c4):
    c4 = np.asarray(c4, dtype=np.float64)
    s = c4 + c4.transpose(1, 0, 2, 3)
    s = s + s.transpose(0, 1, 3, 2)
    s = s + s.transpose(2, 3, 0, 1)
    return s / 8.0


def ref_scalars(C):
    """C [6,6] fp64 symmetric -> (S, dict of the ten scalars)"""
    S = np.linalg.inv(C)
    cd, co, cs = C[0, 0] + C[1, 1] + C[2, 2], C[0, 1] + C[0, 2] + C[1, 2], C[3, 3] + C[4, 4] + C[5, 5]
    sd, so, ss = S[0, 0] + S[1, 1] + S[2, 2], S[0, 1] + S[0, 2] + S[1, 2], S[3, 3] + S[4, 4] + S[5, 5]
    p = {"k_voigt": (cd + 2 * co) / 9, "g_voigt": (cd - co + 3 * cs) / 15, "k_reuss": 1 / (sd + 2 * so),
         "g_reuss": 15 / (4 * sd - 4 * so + 3 * ss)}
    K, G = (p["k_voigt"] + p["k_reuss"]) / 2, (p["g_voigt"] + p["g_reuss"]) / 2
    p.update(k_vrh=K, g_vrh=G, y_mod=9 * K * G / (3 * K + G), homogeneous_poisson=(3 * K - 2 * G) / (2 * (3 * K + G)),
             universal_anisotropy=5 * p["g_voigt"] / p["g_reuss"] + p["k_voigt"] / p["k_reuss"] - 6, pugh_ratio=K / G)
    return S, p


def ref_directional(S, n):
    """S [6,6], unit vectors n [D,3] -> (v^T S v [D] = 1 / E, beta [D])"""
    v = np.stack([n[:, 0] ** 2, n[:, 1] ** 2, n[:, 2] ** 2, n[:, 1] * n[:, 2], n[:, 0] * n[:, 2], n[:, 0] * n[:, 1]], axis=1)
    return np.einsum("di,ij,dj->d", v, S, v), v @ S[:, :3].sum(axis=1)


def check_rows(props, Cs, what, factor=FACTOR, eps=EPS):
    """every output row of `props` (a batched ElasticProperties) against the reference of the symmetric matrices Cs"""
    d = props.to_dict()
    worst = 0.0
    for b, C in enumerate(Cs):
        cond = np.linalg.cond(C)
        S, want = ref_scalars(C)
        tol = factor * eps * cond
        assert np.array_equal(d["voigt"][b], C), (what, b, "voigt")          # picks and means of exact values: no rounding
        err = np.abs(d["compliance"][b] - S).max() / np.abs(S).max()
        worst = max(worst, err / (eps * cond))
        assert err <= tol, (what, b, "compliance", err, tol)
        for name in NAMES:
            got = d[name][b]
            if name == "universal_anisotropy":
                scale = 5 * abs(want["g_voigt"] / want["g_reuss"]) + abs(want["k_voigt"] / want["k_reuss"]) + 6
                err = abs(got - want[name]) / scale
            else:
                err = abs(got - want[name]) / abs(want[name])
            worst = max(worst, err / (eps * cond))
            assert err <= tol, (what, b, name, got, want[name], err, tol)
    print(f"{what}: worst error {worst:.2f} eps cond (allowed {factor:g})")
    return worst


# ---------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture_set(golden_dir):
    """the 100 tensors of the example data set, rounded to fp32: (Cartesian fp32 [100,3,3,3,3], Voigt fp64 [100,6,6])"""
    raw = json.load(open(os.path.join(golden_dir, "example_crystal_elasticity_tensor_n100.json")))
    keys = sorted(raw["elastic_tensor_full"], key=int)
    full = np.array([raw["elastic_tensor_full"][k] for k in keys], dtype=np.float64)
    voigt_field = np.array([raw["elastic_tensor_voigt"][k] for k in keys], dtype=np.float64)
    assert full.shape == (100, 3, 3, 3, 3)
    picks = np.stack([voigt_picks(t) for t in full])
    assert np.array_equal(picks, voigt_field)                  # the data set's own Voigt field: a free check of the map
    cart32 = full.astype(np.float32)
    C = np.stack([voigt_picks(t) for t in cart32.astype(np.float64)])
    for t, c in zip(cart32.astype(np.float64), C):
        assert np.array_equal(symmetrise_cartesian(t), t) and np.array_equal(c, c.T)
        assert np.linalg.eigvalsh(c).min() > 0 and np.linalg.cond(c) <= 44.5
    return cart32, C


@pytest.fixture(scope="module")
def synthetic_set():
    """60 symmetric 6x6 matrices of condition numbers up to 1e6, every third indefinite, rounded to fp32"""
    rng = np.random.default_rng(20261018)
    out, indefinite = [], []
    for m in range(60):
        Q, _ = np.linalg.qr(rng.standard_normal((6, 6)))
        lam = 10.0 * np.exp(rng.uniform(0.0, np.log(10.0 ** rng.uniform(0.0, 6.0)), size=6))
        if m % 3 == 2:
            lam[rng.integers(6)] *= -1.0
        C = (Q * lam) @ Q.T
        C = (0.5 * (C + C.T)).astype(np.float32).astype(np.float64)
        out.append(C)
        indefinite.append(m % 3 == 2)
    C, indefinite = np.stack(out), np.array(indefinite)
    eig = np.linalg.eigvalsh(C)
    assert np.array_equal(eig.min(axis=1) < 0, indefinite)     # fp32 rounding moved no eigenvalue across zero
    assert max(np.linalg.cond(c) for c in C) <= 1.2e6
    return C, indefinite


def _elastic():
    from matten_amd import elastic

    return elastic


# ---------------------------------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3, 100])
def test_fixture_set_through_both_routes(fixture_set, B):
    E = _elastic()
    cart32, C = fixture_set
    a = E.elastic_properties(cart32[:B])                                       # host fp32 Cartesian
    b = E.elastic_properties(torch.from_numpy(C[:B]).to(DEV))                  # device fp64 Voigt
    assert a.voigt.shape == (B, 6, 6) and a.k_vrh.shape == (B,) and a.voigt.dtype == torch.float64
    check_rows(a, C[:B], f"Cartesian fp32, B={B}")
    check_rows(b, C[:B], f"Voigt fp64, B={B}")
    for p in (a, b):
        assert not p.flags.any() and p.is_stable.all() and not p.is_singular.any()
    # the two routes see the same symmetric matrix (the mean of 8 equal values, (C + C^T) / 2 of a symmetric C): they agree
    # within the bound
    da, db = a.to_dict(), b.to_dict()
    assert np.array_equal(da["voigt"], db["voigt"]) and np.array_equal(da["flags"], db["flags"])
    for r in range(B):
        tol = FACTOR * EPS * np.linalg.cond(C[r])
        assert np.abs(da["compliance"][r] - db["compliance"][r]).max() <= tol * np.abs(db["compliance"][r]).max()
        for name in NAMES:
            scale = abs(db[name][r]) if name != "universal_anisotropy" else \
                5 * abs(db["g_voigt"][r] / db["g_reuss"][r]) + abs(db["k_voigt"][r] / db["k_reuss"][r]) + 6
            assert abs(da[name][r] - db[name][r]) <= tol * scale, (r, name)
    # an unbatched tensor gives the row without the leading dimension; a list is stacked
    one = E.elastic_properties(cart32[0])
    assert one.voigt.shape == (6, 6) and one.k_vrh.shape == () and one.flags.shape == ()
    assert float(one.k_vrh) == float(a.k_vrh[0])
    lst = E.elastic_properties([cart32[i].astype(np.float64) for i in range(B)])
    check_rows(lst, C[:B], f"list of fp64 Cartesian tensors, B={B}")
    host = a.cpu()
    assert not host.voigt.is_cuda and torch.equal(host.g_vrh, a.g_vrh.cpu())
    assert a.voigt.is_cuda and b.compliance.is_cuda                      # the results stay on the device


def test_synthetic_set_flags_and_values(synthetic_set):
    E = _elastic()
    C, indefinite = synthetic_set
    p = E.elastic_properties(C.astype(np.float32))                            # Voigt fp32
    flags = p.flags.cpu().numpy()
    assert np.array_equal((flags & 2) != 0, indefinite)
    assert not (flags & 1).any() and not (flags & 4).any()
    assert np.array_equal(p.is_stable.cpu().numpy(), ~indefinite)
    check_rows(p, C, "synthetic, Voigt fp32")
    check_rows(E.elastic_properties(C), C, "synthetic, Voigt fp64")


def test_singular_and_non_finite_rows(synthetic_set, fixture_set):
    E = _elastic()
    C = np.stack([fixture_set[1][0], np.zeros((6, 6)), fixture_set[1][1], synthetic_set[0][0], fixture_set[1][2]])
    C[3, 2, 4] = C[3, 4, 2] = np.nan
    p = E.elastic_properties(C, directions=7, keep_directional=True)
    d = p.to_dict()
    assert list(d["flags"] & 1) == [0, 1, 0, 1, 0]
    assert list(d["is_singular"]) == [False, True, False, True, False]
    for b in (1, 3):
        for k in ("voigt", "compliance", "young", "compressibility", "young_min", "young_max", "compressibility_min",
                  "compressibility_max") + NAMES:
            assert np.isnan(d[k][b]).all(), (b, k)
        for k in ("young_argmin", "young_argmax", "compressibility_argmin", "compressibility_argmax"):
            assert d[k][b] == -1
    # the neighbouring valid rows are what they are on their own
    alone = E.elastic_properties(C[[0, 2, 4]], directions=7, keep_directional=True).to_dict()
    for k in d:
        if k != "directions":
            assert np.array_equal(d[k][[0, 2, 4]], alone[k]), k
    check_rows(E.elastic_properties(C[[0, 2, 4]]), C[[0, 2, 4]], "rows next to singular ones")
    # the Cartesian route flags a NaN as well
    t = np.array(fixture_set[0][:2])
    t[1, 0, 1, 2, 2] = np.inf
    q = E.elastic_properties(t)
    assert list(q.flags.cpu().numpy() & 1) == [0, 1] and bool(torch.isnan(q.k_vrh[1])) and not bool(torch.isnan(q.k_vrh[0]))


def _cubic(c11, c12, c44):
    C = np.zeros((6, 6))
    C[:3, :3] = c12
    C[[0, 1, 2], [0, 1, 2]] = c11
    C[[3, 4, 5], [3, 4, 5]] = c44
    return C


def _cubic_compliance(c11, c12, c44):
    """S11, S12, S44 of a cubic crystal in closed form"""
    det = (c11 - c12) * (c11 + 2 * c12)
    return (c11 + c12) / det, -c12 / det, 1 / c44


def test_closed_forms_isotropic():
    E = _elastic()
    KG = [(160.0, 80.0), (75.5, 26.0), (3.0, 11.0), (1234.5, 0.75)]
    C = np.stack([_cubic(K + 4 * G / 3, K - 2 * G / 3, G) for K, G in KG])
    p = E.elastic_properties(C, directions=65, keep_directional=True).to_dict()
    for b, (K, G) in enumerate(KG):
        tol = FACTOR * EPS * np.linalg.cond(C[b])
        for name, want in (("k_voigt", K), ("k_reuss", K), ("k_vrh", K), ("g_voigt", G), ("g_reuss", G), ("g_vrh", G),
                           ("y_mod", 9 * K * G / (3 * K + G)), ("homogeneous_poisson", (3 * K - 2 * G) / (2 * (3 * K + G))),
                           ("pugh_ratio", K / G)):
            assert abs(p[name][b] - want) <= tol * abs(want), (b, name, p[name][b], want)
        assert abs(p["universal_anisotropy"][b]) <= tol * 12
        young = 9 * K * G / (3 * K + G)
        atol = 4 * tol * max(abs(s) for s in _cubic_compliance(K + 4 * G / 3, K - 2 * G / 3, G))
        assert np.abs(1 / p["young"][b] - 1 / young).max() <= atol
        assert np.abs(p["compressibility"][b] - 1 / (3 * K)).max() <= atol
        assert abs(1 / p["young_min"][b] - 1 / young) <= atol and abs(1 / p["young_max"][b] - 1 / young) <= atol
        assert p["flags"][b] == 0


def test_closed_forms_cubic():
    E = _elastic()
    cubic = [(168.0, 121.0, 75.0), (108.0, 62.0, 28.0), (250.0, 20.0, 130.0), (50.0, 30.0, 4.0)]
    C = np.stack([_cubic(*c) for c in cubic])
    n = np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [1.0, 1.0, 1.0], [1.0, -1.0, 1.0], [1.0, 1.0, 0.0]])
    p = E.elastic_properties(C, directions=n, keep_directional=True).to_dict()
    for b, (c11, c12, c44) in enumerate(cubic):
        tol = FACTOR * EPS * np.linalg.cond(C[b])
        K = (c11 + 2 * c12) / 3
        gv = (c11 - c12 + 3 * c44) / 5
        gr = 5 * (c11 - c12) * c44 / (4 * c44 + 3 * (c11 - c12))
        G = (gv + gr) / 2
        for name, want in (("k_voigt", K), ("k_reuss", K), ("k_vrh", K), ("g_voigt", gv), ("g_reuss", gr), ("g_vrh", G),
                           ("y_mod", 9 * K * G / (3 * K + G)), ("pugh_ratio", K / G)):
            assert abs(p[name][b] - want) <= tol * abs(want), (b, name, p[name][b], want)
        assert abs(p["universal_anisotropy"][b] - (5 * gv / gr - 5)) <= tol * (5 * gv / gr + 7)
        s11, s12, s44 = _cubic_compliance(c11, c12, c44)
        smax = max(abs(s11), abs(s12), abs(s44))
        e100 = (c11 - c12) * (c11 + 2 * c12) / (c11 + c12)
        inv_e111 = s11 - (2.0 / 3.0) * (s11 - s12 - s44 / 2)
        inv_e110 = s11 - 0.5 * (s11 - s12 - s44 / 2)
        atol = 4 * tol * smax
        got = 1.0 / p["young"][b]
        for d, want in ((0, 1 / e100), (1, 1 / e100), (2, inv_e111), (3, inv_e111), (4, inv_e110)):
            assert abs(got[d] - want) <= atol, (b, d, got[d], want)
        assert np.abs(p["compressibility"][b] - 1 / (3 * K)).max() <= atol
        # E is extremal along <100> and <111> (the two directions of each family agree to rounding only: either may win)
        lo, hi = ((0, 1), (2, 3)) if inv_e111 < 1 / e100 else ((2, 3), (0, 1))
        assert p["young_argmin"][b] in lo and p["young_argmax"][b] in hi
        assert p["young_min"][b] == p["young"][b].min() and p["young_max"][b] == p["young"][b].max()


def _rotation(seed):
    q, r = np.linalg.qr(np.random.default_rng(seed).standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def test_rotation_invariance(fixture_set):
    E = _elastic()
    n = E.fibonacci_hemisphere(48)
    for b, seed in ((3, 1), (41, 2)):
        t = fixture_set[0][b].astype(np.float64)
        R = _rotation(seed)
        assert abs(np.linalg.det(R) - 1) < 1e-14
        rot = np.einsum("ia,jb,kc,ld,abcd->ijkl", R, R, R, R, t)
        p = E.elastic_properties(t, directions=n, keep_directional=True).to_dict()
        q = E.elastic_properties(rot, directions=n @ R.T, keep_directional=True).to_dict()
        C = fixture_set[1][b]
        cond, smax = np.linalg.cond(C), np.abs(np.linalg.inv(C)).max()
        # the rotated tensor is itself rounded (81-term sums, a few eps of max|C|): the same bound covers it
        tol = FACTOR * EPS * cond
        for name in NAMES:
            scale = abs(p[name]) if name != "universal_anisotropy" else \
                5 * abs(p["g_voigt"] / p["g_reuss"]) + abs(p["k_voigt"] / p["k_reuss"]) + 6
            assert abs(p[name] - q[name]) <= tol * scale, (b, name, p[name], q[name])
        assert np.abs(1 / p["young"] - 1 / q["young"]).max() <= 4 * tol * smax
        assert np.abs(p["compressibility"] - q["compressibility"]).max() <= 4 * tol * smax


def test_unsymmetric_input_is_symmetrised(fixture_set):
    E = _elastic()
    rng = np.random.default_rng(11)
    t = fixture_set[0][:3].astype(np.float64)
    noisy = (t + 0.01 * np.abs(t).max() * rng.standard_normal(t.shape)).astype(np.float32)
    sym = np.stack([symmetrise_cartesian(x) for x in noisy])
    C = np.stack([voigt_picks(x) for x in sym])
    assert np.abs(noisy - noisy.transpose(0, 2, 1, 3, 4)).max() > 0
    p = E.elastic_properties(noisy)
    d = p.to_dict()
    # (the mean of 8 fp32 values in fp64: exact up to the last bit, whatever the order of the additions)
    assert np.abs(d["voigt"] - C).max() <= 4 * EPS * np.abs(C).max()
    check_rows(p, d["voigt"], "symmetrised Cartesian")       # everything else follows from the symmetrised matrix
    # the Voigt route: (C + C^T) / 2
    V = C + 0.01 * np.abs(C).max() * rng.standard_normal(C.shape)
    r = E.elastic_properties(V).to_dict()
    Vs = 0.5 * (V + V.transpose(0, 2, 1))
    assert np.array_equal(r["voigt"], Vs)
    check_rows(E.elastic_properties(V), Vs, "symmetrised Voigt")


@pytest.mark.parametrize("D", [1, 63, 64, 65, 256, 257])
def test_directional_maps_and_extremes(fixture_set, D):
    """the wave (64) and workgroup (256) edges of the direction loop"""
    E = _elastic()
    C = fixture_set[1][[0, 17, 58]]
    p = E.elastic_properties(C, directions=D, keep_directional=True)
    d = p.to_dict()
    n = d["directions"]
    assert np.array_equal(n, E.fibonacci_hemisphere(D)) and d["young"].shape == (3, D)
    for b in range(3):
        S = np.linalg.inv(C[b])
        atol = 4 * FACTOR * EPS * np.linalg.cond(C[b]) * np.abs(S).max()
        q, beta = ref_directional(S, n)
        assert (q > 0).all()
        assert np.abs(1 / d["young"][b] - q).max() <= atol
        assert np.abs(d["compressibility"][b] - beta).max() <= atol
        # the extremes are entries of the maps, at the indices reported, and those indices are right: the reference's
        # value there lies within the tolerance of the reference's extreme
        for name, arr, ref, pick in (("young_min", d["young"][b], q, np.max), ("young_max", d["young"][b], q, np.min),
                                     ("compressibility_min", d["compressibility"][b], beta, np.min),
                                     ("compressibility_max", d["compressibility"][b], beta, np.max)):
            at = int(d[name.replace("_m", "_argm")][b])
            assert 0 <= at < D and d[name][b] == arr[at], (b, name)
            assert d[name][b] == (arr.min() if name.endswith("min") else arr.max()), (b, name)
            assert abs(ref[at] - pick(ref)) <= atol, (b, name, at)
            first = int(np.argmin(arr) if name.endswith("min") else np.argmax(arr))      # numpy: the first occurrence
            assert at == first, (b, name, at, first)
    # without keep_directional the maps are not kept and the extremes are the same bits; a second run too
    again = E.elastic_properties(C, directions=D, keep_directional=True).to_dict()
    lean = E.elastic_properties(C, directions=D)
    assert lean.young is None and lean.compressibility is None
    lean = lean.to_dict()
    for k in d:
        assert np.array_equal(d[k], again[k], equal_nan=True), k
        if k not in ("young", "compressibility"):
            assert np.array_equal(d[k], lean[k]), k


def test_duplicated_directions_resolve_to_the_lowest_index(fixture_set):
    E = _elastic()
    C = fixture_set[1][[5, 23, 77]]
    base = E.fibonacci_hemisphere(150)
    n = np.concatenate([base, base, base[:40]])              # 340 directions: copies in other waves and other strides
    d = E.elastic_properties(C, directions=n, keep_directional=True).to_dict()
    assert np.array_equal(d["directions"][:150], d["directions"][150:300])
    for b in range(3):
        assert np.array_equal(d["young"][b][:150], d["young"][b][150:300])
        for name, arr in (("young", d["young"][b]), ("compressibility", d["compressibility"][b])):
            assert d[name + "_argmin"][b] == int(np.argmin(arr)) < 150
            assert d[name + "_argmax"][b] == int(np.argmax(arr)) < 150
    # all directions the same: index 0 wins everywhere
    same = E.elastic_properties(C, directions=np.tile([[0.3, -0.5, 0.8]], (300, 1))).to_dict()
    for k in ("young_argmin", "young_argmax", "compressibility_argmin", "compressibility_argmax"):
        assert (same[k] == 0).all(), k


def _directional_of_identity(dirs):
    """ops.elastic_directional(keep=True) of two unflagged crystals whose compliance is the 6x6 identity"""
    from matten_amd import ops
    S = torch.eye(6, dtype=torch.float64, device=DEV).repeat(2, 1, 1)
    flags = torch.zeros(2, dtype=torch.int32, device=DEV)
    return [t.cpu().numpy() for t in ops.elastic_directional(S, flags, torch.from_numpy(dirs).to(DEV), keep=True)]


@pytest.mark.parametrize("D", [1, 65, 257])
def test_directional_without_a_comparable_value_keeps_the_sentinel(D):
    """An unflagged row of which no direction gives a comparable value (every direction NaN): the maps are NaN and the
    extremes are what the reduction started from, +-inf with the index 0x7fffffff -- not the NaN / -1 that the pair and
    the acoustic kernel write in this corner.  The expectation is read from the kernel's code (a NaN candidate fails
    both comparisons of `better`, so no lane, wave or workgroup merge replaces the start value) and was confirmed on the
    build before the reduction moved into block_best, which gives exactly these values: they are that build's output."""
    young, beta, ext, arg = _directional_of_identity(np.full((D, 3), np.nan))
    assert young.shape == beta.shape == (2, D) and np.isnan(young).all() and np.isnan(beta).all()
    assert np.array_equal(ext, np.tile([np.inf, -np.inf, np.inf, -np.inf], (2, 1)))
    assert arg.dtype == np.int32 and (arg == 2147483647).all()


def test_directional_lone_comparable_value_in_the_second_wave():
    """D = 65, every direction NaN but the last, (0, 0, 1): lane 0 of the second wave holds the only candidate, so all
    four extremes reach the output through the cross-wave merge in LDS.  With S = 1: 1 / E = v . v = 1 and beta = the
    first three entries of v summed = 1, exactly."""
    dirs = np.full((65, 3), np.nan)
    dirs[64] = (0.0, 0.0, 1.0)
    young, beta, ext, arg = _directional_of_identity(dirs)
    assert np.isnan(young[:, :64]).all() and np.isnan(beta[:, :64]).all()
    assert (young[:, 64] == 1.0).all() and (beta[:, 64] == 1.0).all()
    assert np.array_equal(ext, np.ones((2, 4))) and np.array_equal(arg, np.full((2, 4), 64))


def test_from_irreps_matches_the_cartesian_route(fixture_set):
    """Both routes run the same 21-term fp32 dot product per entry (ops.dense_rows) with basis values that are the same
    fp64 numbers rounded to fp32: voigt_basis copies columns of the Cartesian basis.  The Voigt route keeps ONE of the
    eight equivalent Cartesian entries, the Cartesian route their mean; the eight agree except where the basis entries of
    equivalent positions -- equal to ~1e-16 -- straddle an fp32 rounding boundary, one fp32 ulp of a term.  So the two
    Voigt matrices differ by at most 2^-24 relative, and the compliance and the scalars by cond(C) times that."""
    from matten_amd import o3
    from matten_amd.utils import ToCartesian

    E = _elastic()
    B = 24
    _, Q = o3.cartesian_tensor_basis("ijkl=jikl=klij")
    x = (fixture_set[0][:B].astype(np.float64).reshape(B, 81) @ Q.reshape(21, 81).T / (Q.reshape(21, 81) ** 2).sum(1))
    x = torch.from_numpy(x.astype(np.float32)).to(DEV)
    cart = ToCartesian("ijkl=jikl=klij")(x)
    assert cart.shape == (B, 3, 3, 3, 3) and cart.dtype == torch.float32
    a = E.elastic_properties(cart).to_dict()
    b = E.elastic_properties_from_irreps(x).to_dict()
    assert np.abs(a["voigt"] - fixture_set[1][:B]).max() <= 1e-5 * np.abs(fixture_set[1][:B]).max()   # (the set itself)
    worst = 0.0
    for r in range(B):
        cond = np.linalg.cond(a["voigt"][r])
        tol = 2.0 ** -24 * cond
        assert np.abs(a["voigt"][r] - b["voigt"][r]).max() <= 2.0 ** -24 * np.abs(a["voigt"][r]).max()
        err = np.abs(a["compliance"][r] - b["compliance"][r]).max() / np.abs(a["compliance"][r]).max()
        assert err <= tol
        worst = max(worst, err / tol)
        for name in NAMES:
            scale = abs(a[name][r]) if name != "universal_anisotropy" else \
                5 * abs(a["g_voigt"][r] / a["g_reuss"][r]) + abs(a["k_voigt"][r] / a["k_reuss"][r]) + 6
            err = abs(a[name][r] - b[name][r]) / scale
            worst = max(worst, err / tol)
            assert err <= tol, (r, name, a[name][r], b[name][r])
        assert a["flags"][r] == b["flags"][r] == 0
    print(f"irreps route vs Cartesian route: worst {worst:.3g} of 2^-24 cond")
    one = E.elastic_properties_from_irreps(x[0], directions=5)
    assert one.voigt.shape == (6, 6) and float(one.k_vrh) == b["k_vrh"][0] and one.young_min.shape == ()


def test_predict_with_properties(golden_dir):
    """predict(..., properties=True): the usual return value plus one row of properties per structure"""
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
    ds = {"allowed_species": list(range(1, 95)), "average_num_neighbors": 18.0}
    torch.manual_seed(35)
    model = ScalarTensorModel(backbone_hparams=dict(LMAX2), dataset_hparams=ds).to(DEV).eval()
    cfg = {"data": {"r_cut": 5.0, "tensor_target_name": "elastic_tensor_full", "tensor_target_formula": "ijkl=jikl=klij"}}
    with W.catch_warnings():
        W.simplefilter("ignore")
        plain = P.predict(structs, model=model, config=cfg)
        tensors, props = P.predict(structs, model=model, config=cfg, properties=True, directions=33)
        off = P.predict(structs, model=model, config=cfg, properties=False)
    assert len(plain) == len(tensors) == len(off) == 5 and plain[2] is None and tensors[2] is None and off[2] is None
    for i in (0, 1, 3, 4):
        assert type(tensors[i]) is type(plain[i]) and np.array_equal(np.asarray(tensors[i]), np.asarray(plain[i]))
        assert np.array_equal(np.asarray(off[i]), np.asarray(plain[i]))
    want = E.elastic_properties([None if t is None else np.asarray(t) for t in plain], directions=33).to_dict()
    got = props.to_dict()
    assert set(got) == set(want) and got["flags"].shape == (5,)
    for k in got:
        if got[k] is None:
            assert want[k] is None
        else:
            assert np.array_equal(got[k], want[k], equal_nan=True), k
    assert got["flags"][2] & 4 and got["flags"][2] & 1 and not (got["flags"][[0, 1, 3, 4]] & 5).any()
    for k in NAMES + ("voigt", "compliance", "young_min", "compressibility_max"):
        assert np.isnan(got[k][2]).all() and not np.isnan(got[k][[0, 1, 3, 4]]).any(), k
    assert got["young_argmin"][2] == -1
    # values: the kernel's own input against the reference (a random-init model: tensors of any signature)
    C = np.stack([voigt_picks(symmetrise_cartesian(np.asarray(plain[i], dtype=np.float64))) for i in (0, 1, 3, 4)])
    assert np.abs(got["voigt"][[0, 1, 3, 4]] - C).max() <= 4 * EPS * np.abs(C).max()
    # a single structure: no leading dimension
    with W.catch_warnings():
        W.simplefilter("ignore")
        t1, p1 = P.predict(structs[0], model=model, config=cfg, properties=True)
    assert np.array_equal(np.asarray(t1), np.asarray(plain[0])) and p1.voigt.shape == (6, 6)
    assert float(p1.k_voigt) == got["k_voigt"][0]
    with pytest.raises(ValueError, match="is_atomic_tensor"):
        P.predict(structs, model=model, config=cfg, is_atomic_tensor=True, properties=True)
