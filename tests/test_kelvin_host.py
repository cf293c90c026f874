"""
CPU tests of the Kelvin (eigen-stiffness) decomposition (matten_amd/elastic.py over csrc/kelvin.hip): the numpy restatement
``kelvin_host`` against known answers and the two invariants of the Mandel map, its adjoint ``kelvin_bwd_host`` against
central differences, ``nearest_stable_host``, the library's three entries (exported, ABI 47, bad arguments refused without a
device) and the argument checks of the host layers.  The GPU tests (tests/test_gpu_kelvin.py) hold the kernels to the
restatement tested here and share this file's generators and its pool of 257 rows.
"""
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N100 = os.path.join(ROOT, "tests", "golden", "example_crystal_elasticity_tensor_n100.json")
# The gap test: every modulus at least GAP max|C^| away from its neighbours.  An eigenvector moves by |E| / gap under a
# perturbation E of C^, so with GAP = 0.02 the per-modulus central differences (step 1e-5 max|C^|) have a truncation error
# of (step / gap)^2 = 2.5e-7, and two decompositions within 8e-15 max|C^| of each other give dilatations within
# 2 * 8e-15 / 0.02 = 8e-13 < 1e-12.
GAP = 0.02
PREFIXES = (1, 63, 64, 65, 257)
NAN_ROW, INF_ROW, ZERO_ROW = 10, 40, 128
D = np.array([1.0, 1.0, 1.0, np.sqrt(2.0), np.sqrt(2.0), np.sqrt(2.0)])


# ----------------------------------------------------------------------------------------------------------------------
# generators
# ----------------------------------------------------------------------------------------------------------------------
def isotropic(K, G):
    C = np.zeros((6, 6))
    C[:3, :3] = K - 2.0 * G / 3.0
    C[range(3), range(3)] = K + 4.0 * G / 3.0
    C[range(3, 6), range(3, 6)] = G
    return C


def cubic(c11, c12, c44):
    C = np.zeros((6, 6))
    C[:3, :3] = c12
    C[range(3), range(3)] = c11
    C[range(3, 6), range(3, 6)] = c44
    return C


def mandel_weight():
    w = np.outer(D, D)
    w[3:, 3:] = 2.0
    return w


def from_spectrum(lam, rng):
    """the Voigt matrix whose Mandel matrix is Q diag(lam) Q^T for a random orthogonal Q (6 x 6: a mixture in Mandel
    space, not a rotation of space), symmetric to the last bit"""
    Q, _ = np.linalg.qr(rng.standard_normal((6, 6)))
    M = (Q * np.asarray(lam, dtype=np.float64)) @ Q.T
    return (0.5 * (M + M.T)) / mandel_weight()


# nearly degenerate clusters: the spectra that cyclic Jacobi takes longest on (csrc/sym6.h)
NEARLY_BASES = ([130.0, 130.0, 160.0, 160.0, 160.0, 490.0], [80.0] * 5 + [300.0], [100.0] * 3 + [250.0] * 3, [5.0] * 6)
# (base, relative split, seed); on the first six a numpy run of the kernel's rotation leaves an off-diagonal of 8.8e-9,
# 1.4e-9, 6.3e-10, 2.7e-10, 2.4e-10 and 1.3e-10 max|C^| after seven sweeps, and still 1.3e-14 on the second after eight
NEARLY = ((2, 1e-11, 2369), (2, 1e-11, 595), (2, 1e-11, 2281), (2, 1e-11, 1241), (2, 1e-10, 595), (2, 1e-10, 783),
          (0, 1e-10, 1), (0, 1e-12, 2), (1, 1e-9, 3), (1, 1e-6, 4), (3, 1e-10, 5), (0, 1e-4, 6))


def nearly_degenerate(base: int, split: float, seed: int):
    """NEARLY_BASES[base] with every modulus moved by a relative `split` (Gaussian), mixed in Mandel space"""
    rng = np.random.default_rng(seed)
    lam = np.array(NEARLY_BASES[base]) * (1.0 + split * rng.standard_normal(6))
    return from_spectrum(lam, rng)


def rotated(C, rng):
    """the Voigt matrix of the tensor C_ijkl rotated in space by a random proper rotation"""
    from matten_amd.elastic import VOIGT_PAIRS, voigt_to_cartesian

    R, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    R = R * np.sign(np.linalg.det(R))
    c4 = np.einsum("ai,bj,ck,dl,ijkl->abcd", R, R, R, R, voigt_to_cartesian(C))
    V = np.array([[c4[i, j, k, l] for (k, l) in VOIGT_PAIRS] for (i, j) in VOIGT_PAIRS])
    return 0.5 * (V + V.T)


def random_symmetric(n, scale, seed, shift=0.0):
    """n symmetric matrices with Gaussian entries of size `scale` plus `shift` on the diagonal: eigenvalues that repel
    (a spectrum drawn at random and mixed does not: a fifth of such rows fails the gap test)"""
    rng = np.random.default_rng(seed)
    X = scale * rng.standard_normal((n, 6, 6))
    return 0.5 * (X + X.transpose(0, 2, 1)) + shift * np.eye(6)


def n100_voigt():
    raw = json.load(open(N100))
    keys = sorted(raw["elastic_tensor_voigt"], key=int)
    C = np.array([raw["elastic_tensor_voigt"][k] for k in keys], dtype=np.float64)
    assert C.shape == (100, 6, 6)
    return C


_POOL = None


def kelvin_pool():
    """The pool of the GPU tests, [257,6,6] fp64 Voigt matrices, with a dict of row-index arrays by kind.  The 100 tensors of
    the example data set; isotropic and cubic tensors, the cubic ones also rotated in space; 5-fold degenerate spectra
    [80 x 5, 300] mixed by a random orthogonal 6 x 6 matrix in Mandel space -- they stand in for the "rotated isotropic
    tensor" one would name first: an isotropic tensor rotated in space is the same tensor, and a dense matrix with a 5-fold
    degenerate modulus is the case that is meant; nearly degenerate clusters (NEARLY: relative splits of 1e-12 to 1e-4, six
    of them rows that seven Jacobi sweeps leave unconverged); indefinite rows; one row with a modulus of 0 (ZERO_ROW); spectra graded over 1e-6 to 1e3, a quarter of
    them with one sign turned; definite and indefinite random rows at entry scales 1e-3, 1 and 300; a NaN row (NAN_ROW) and
    an Inf row (INF_ROW) among the first 63."""
    global _POOL
    if _POOL is not None:
        return _POOL[0].copy(), _POOL[1]
    rng = np.random.default_rng(20261020)
    rows, kinds = [], {}

    def add(kind, mats):
        kinds.setdefault(kind, []).extend(range(len(rows), len(rows) + len(mats)))
        rows.extend(mats)

    add("n100", list(n100_voigt()))
    iso = [isotropic(100.0, 40.0), isotropic(1.0, 1.0), isotropic(300.0, 1e-3), isotropic(1e-3, 200.0), isotropic(50.0, 75.0),
           isotropic(160.0, 80.0)]
    cub = [cubic(250.0, 120.0, 80.0), cubic(1.0, 0.5, 0.2), cubic(300.0, 299.0, 1e-2), cubic(100.0, -20.0, 60.0),
           cubic(165.7, 63.9, 79.6), cubic(100.0, 150.0, 80.0)]
    add("isotropic", iso)
    add("cubic", cub)
    add("rotated", [rotated(c, rng) for c in cub] + [rotated(c, rng) for c in cub[:2]])          # 8
    add("degenerate", [from_spectrum([80.0] * 5 + [300.0], rng) for _ in range(4)]
        + [from_spectrum([2.0] + [5.0] * 5, rng) for _ in range(2)] + [from_spectrum([-3.0] * 2 + [7.0] * 4, rng) for _ in range(2)])
    assert len(rows) == ZERO_ROW
    add("zero", [from_spectrum([0.0, 20.0, 45.0, 70.0, 110.0, 260.0], rng)])
    for scale in (1e-3, 1.0, 300.0):
        add("indefinite", [from_spectrum(scale * rng.uniform(0.1, 1.0, 6) * np.where(np.arange(6) < 1 + m % 3, -1.0, 1.0), rng)
                           for m in range(10)])
        add("definite", list(random_symmetric(12, scale, int(rng.integers(1 << 30)), shift=6.0 * scale)))
        add("random", list(random_symmetric(6, scale, int(rng.integers(1 << 30)))))
    graded = []
    for m in range(32):
        lo = rng.uniform(-6.0, -3.0)
        lam = 10.0 ** np.linspace(lo, min(lo + 9.0, 3.0), 6)
        if m % 4 == 3:
            lam[int(rng.integers(6))] *= -1.0
        graded.append(from_spectrum(lam, rng))
    add("graded", graded)
    add("nearly", [nearly_degenerate(*a) for a in NEARLY])
    C = np.stack(rows)
    assert C.shape == (257, 6, 6), C.shape
    C[NAN_ROW, 2, 4] = np.nan
    C[INF_ROW, 0, 0] = np.inf
    kinds = {k: np.array(v) for k, v in kinds.items()}
    kinds["bad"] = np.array([NAN_ROW, INF_ROW])
    _POOL = (C, kinds)
    return C.copy(), kinds


def gap_ok(C) -> np.ndarray:
    """rows whose six moduli are at least GAP max|C^| apart: the condition of the per-modulus gradient checks and of the
    comparison of eigenvector-dependent quantities"""
    from matten_amd.elastic import kelvin_host

    h = kelvin_host(C)
    with np.errstate(invalid="ignore"):
        big = np.abs(h["mandel"]).max(axis=(1, 2))
        return np.isfinite(big) & (np.diff(h["kelvin_moduli"], axis=1).min(axis=1) >= GAP * big)


def penalty(C, margin):
    """sum_k max(margin - l_k, 0)^2 per row: the squared stability penalty"""
    from matten_amd.elastic import kelvin_host

    return (np.maximum(margin[:, None] - kelvin_host(C)["kelvin_moduli"], 0.0) ** 2).sum(axis=1)


def central_differences(fn, C, step) -> np.ndarray:
    """d fn / d C [n,6,6] over the 36 entries taken as independent, one step per row"""
    g = np.zeros_like(C)
    for i in range(6):
        for j in range(6):
            d = np.zeros_like(C)
            d[:, i, j] = step
            g[:, i, j] = (fn(C + d) - fn(C - d)) / (2.0 * step)
    return g


# ----------------------------------------------------------------------------------------------------------------------
# kelvin_host
# ----------------------------------------------------------------------------------------------------------------------
def test_known_answers():
    from matten_amd.elastic import KELVIN_NAMES, eigenstrains, kelvin_host

    h = kelvin_host(np.stack([isotropic(100.0, 40.0), cubic(250.0, 120.0, 80.0)]))
    want = np.array([[80.0, 80.0, 80.0, 80.0, 80.0, 300.0], [130.0, 130.0, 160.0, 160.0, 160.0, 490.0]])
    assert np.abs(h["kelvin_moduli"] - want).max() <= 1e-12
    assert set(KELVIN_NAMES) <= set(h)
    assert np.abs(h["stability_margin"] - [80.0, 130.0]).max() <= 1e-12
    assert np.abs(h["kelvin_condition"] - [3.75, 490.0 / 130.0]).max() <= 1e-12
    # the stiffest mode of both is the volumetric one, the others are isochoric
    assert np.abs(h["kelvin_dilatation"] - [0, 0, 0, 0, 0, 1]).max() <= 1e-12
    eps = eigenstrains(h["kelvin_vectors"])
    assert eps.shape == (2, 6, 3, 3) and np.array_equal(eps, eps.transpose(0, 1, 3, 2))
    assert np.abs((eps ** 2).sum(axis=(2, 3)) - 1.0).max() <= 1e-14
    assert np.abs(np.abs(eps[:, 5]) - np.eye(3) / np.sqrt(3.0)).max() <= 1e-14
    tr = np.trace(eps, axis1=2, axis2=3)
    assert np.abs(tr * tr / 3.0 - h["kelvin_dilatation"]).max() <= 1e-14
    one = kelvin_host(cubic(250.0, 120.0, 80.0))                        # unbatched
    assert one["kelvin_moduli"].shape == (6,) and one["stability_margin"].shape == ()
    # an unstable cubic crystal (c12 > c11): margin c11 - c12, condition NaN
    bad = kelvin_host(cubic(100.0, 150.0, 80.0))
    assert abs(bad["stability_margin"] + 50.0) <= 1e-12 and np.isnan(bad["kelvin_condition"])


def test_trace_and_frobenius_norm_on_the_pool():
    """sum of the moduli = trace of C^; sum of their squares = the squared Frobenius norm of the rank-4 tensor (the Mandel
    map is an isometry): both to 64 eps of the sum of the magnitudes"""
    from matten_amd.elastic import kelvin_host, voigt_to_cartesian

    C, kinds = kelvin_pool()
    h = kelvin_host(C)
    ok = np.ones(len(C), dtype=bool)
    ok[kinds["bad"]] = False
    assert np.isnan(h["kelvin_moduli"][~ok]).all() and np.isnan(h["kelvin_vectors"][~ok]).all()
    assert np.isnan(h["stability_margin"][~ok]).all() and np.isnan(h["kelvin_condition"][~ok]).all()
    lam, Ch, c4 = h["kelvin_moduli"][ok], h["mandel"][ok], voigt_to_cartesian(C[ok])
    assert c4.shape == (255, 3, 3, 3, 3)
    eps = 2.0 ** -52
    assert (np.abs(lam.sum(1) - np.trace(Ch, axis1=1, axis2=2)) <= 64 * eps * np.abs(lam).sum(1)).all()
    assert (np.abs((lam ** 2).sum(1) - (c4 ** 2).sum(axis=(1, 2, 3, 4))) <= 64 * eps * (lam ** 2).sum(1)).all()
    assert (np.diff(lam, axis=1) >= 0).all()
    # the deliberate zero: one modulus at rounding distance of 0, and the only row of the pool that close to it
    big = np.abs(Ch).max(axis=(1, 2))
    near = np.abs(lam[:, 0]) <= 1e-10 * big
    assert near.sum() == 1 and np.nonzero(ok)[0][near][0] == ZERO_ROW


def test_flags_exclude_rows():
    from matten_amd.elastic import kelvin_bwd_host, kelvin_host

    C = np.stack([isotropic(100.0, 40.0), cubic(250.0, 120.0, 80.0), cubic(1.0, 0.5, 0.2)])
    h = kelvin_host(C, flags=np.array([0, 1, 2], dtype=np.int32))        # bit 1 alone does not exclude
    assert np.isnan(h["kelvin_moduli"][1]).all() and np.isfinite(h["kelvin_moduli"][[0, 2]]).all()
    g = kelvin_bwd_host(C, np.full((3, 6), np.nan), flags=np.array([1, 1, 1]))
    assert (g == 0).all() and not np.signbit(g).any()
    with pytest.raises(ValueError, match="flags"):
        kelvin_host(C, flags=np.zeros(2, dtype=np.int32))
    with pytest.raises(ValueError, match="voigt"):
        kelvin_host(np.zeros((3, 3, 3, 3)))


# ----------------------------------------------------------------------------------------------------------------------
# kelvin_bwd_host against central differences
# ----------------------------------------------------------------------------------------------------------------------
def test_adjoint_of_the_penalty_on_all_rows():
    """The squared penalty sum_k max(m - l_k, 0)^2 with m = (l_1 + l_6) / 2 + max|C^| / 10 (some modes active on every row, a multiple of the identity included), on every finite row of the
    pool -- degenerate moduli included: a spectral function, its gradient U diag(-2 max(m - l, 0)) U^T does not depend on
    the basis.  Central differences with steps of 1e-5 and 2e-5 max|C^|; the function is C^1 with a kink in the second
    derivative where a modulus crosses m: a row with a modulus within a step of m has an error of first order in the
    step, up to 2e-5 of max|g|, which is the bound (the noise is held to it too).  Measured on this pool, where no modulus
    lies that close to m: noise (fine against coarse) 4.4e-9, analytic against fine 1.5e-9."""
    from matten_amd.elastic import kelvin_bwd_host, kelvin_host

    C, kinds = kelvin_pool()
    ok = np.ones(len(C), dtype=bool)
    ok[kinds["bad"]] = False
    C = C[ok]
    h = kelvin_host(C)
    lam = h["kelvin_moduli"]
    margin = 0.5 * (lam[:, 0] + lam[:, 5]) + 0.1 * np.abs(h["mandel"]).max(axis=(1, 2))
    got = kelvin_bwd_host(C, -2.0 * np.maximum(margin[:, None] - lam, 0.0))
    assert np.array_equal(got, got.transpose(0, 2, 1))
    step = 1e-5 * np.abs(h["mandel"]).max(axis=(1, 2))
    fine = central_differences(lambda X: penalty(X, margin), C, step)
    coarse = central_differences(lambda X: penalty(X, margin), C, 2.0 * step)
    scale = np.abs(got).max(axis=(1, 2))
    assert (scale > 0).all()
    noise = (np.abs(fine - coarse).max(axis=(1, 2)) / scale).max()
    err = (np.abs(got - fine).max(axis=(1, 2)) / scale).max()
    print(f"penalty: finite-difference noise {noise:.2e}, analytic against the finer difference {err:.2e} (of max|g| per row)")
    assert noise <= 2e-5 and err <= 2e-5


def test_adjoint_per_modulus_on_separated_rows():
    """A random linear functional of the six moduli on random symmetric matrices at entry scales 1e-3, 1 and 300, indefinite
    and shifted to definite, kept where the gap test passes (GAP = 0.02 of max|C^|; at most 10 % may be left out).  Steps
    of 1e-5 and 2e-5 max|C^|: truncation (step / gap)^2 <= 1e-6.  Measured: noise 1.6e-7, analytic against fine 5.2e-8, of
    the row's max|g|; bound 1e-5 as in tests/test_rank2_host.py, and the noise is held to it too."""
    from matten_amd.elastic import kelvin_bwd_host, kelvin_host

    C = np.concatenate([random_symmetric(100, s, seed, shift) for seed, (s, shift) in
                        enumerate(((1e-3, 0.0), (1.0, 0.0), (300.0, 0.0), (1e-3, 6e-3), (1.0, 6.0), (300.0, 1800.0)))])
    keep = gap_ok(C)
    print(f"kept {keep.mean():.3f} of {len(C)} draws")
    assert keep.mean() >= 0.9
    C = C[keep]
    assert (np.linalg.eigvalsh(C[-50:] * mandel_weight()) > 0).all() and (np.linalg.eigvalsh(C[:50] * mandel_weight())[:, 0] < 0).all()
    rng = np.random.default_rng(3)
    c = rng.standard_normal((len(C), 6))
    got = kelvin_bwd_host(C, c)
    step = 1e-5 * np.abs(kelvin_host(C)["mandel"]).max(axis=(1, 2))

    def fn(X):
        return (kelvin_host(X)["kelvin_moduli"] * c).sum(axis=1)

    fine, coarse = central_differences(fn, C, step), central_differences(fn, C, 2.0 * step)
    scale = np.abs(got).max(axis=(1, 2))
    noise = (np.abs(fine - coarse).max(axis=(1, 2)) / scale).max()
    err = (np.abs(got - fine).max(axis=(1, 2)) / scale).max()
    print(f"per modulus: finite-difference noise {noise:.2e}, analytic against the finer difference {err:.2e} (of max|g| per row)")
    assert noise <= 1e-5 and err <= 1e-5
    # the trace's gradient is D^2 on the diagonal, whatever the basis; given vectors are used as they are
    ones = kelvin_bwd_host(C, np.ones((len(C), 6)))
    assert np.abs(ones - np.diag(D * D)).max() <= 1e-14
    U = kelvin_host(C)["kelvin_vectors"]
    assert np.array_equal(kelvin_bwd_host(C, c, vectors=U), got)
    assert np.array_equal(kelvin_bwd_host(C, c, vectors=-U), got)


def test_pool_share_passing_the_gap_test():
    """what the GPU tests compare eigenvector-dependent quantities on: the rows of the pool that pass the gap test (the
    degenerate, graded and many data-set rows cannot; at least a quarter of the pool does)"""
    C, kinds = kelvin_pool()
    keep = gap_ok(C)
    print(f"{keep.sum()} of {len(C)} pool rows pass the gap test")
    assert not keep[kinds["bad"]].any() and not keep[kinds["isotropic"]].any() and not keep[kinds["degenerate"]].any()
    assert keep.sum() >= 64 and keep[kinds["definite"]].mean() >= 0.8


# ----------------------------------------------------------------------------------------------------------------------
# nearest_stable_host
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("floor_rel", [0.0, 1e-6, 0.05])
def test_nearest_stable_host(floor_rel):
    from matten_amd.elastic import kelvin_host, nearest_stable_host

    C, kinds = kelvin_pool()
    h = kelvin_host(C)
    big = np.abs(h["mandel"]).max(axis=(1, 2))                             # (NaN on the two bad rows)
    bad = kinds["bad"]
    for b in range(0, len(C), 16):      # (one floor per call: a few rows each, in the units of each row)
        rows = np.arange(b, min(b + 16, len(C)))
        for r in rows:
            floor = floor_rel * big[r] if np.isfinite(big[r]) else 1.0
            V, cart, changed = nearest_stable_host(C[r], floor)
            assert V.shape == (6, 6) and cart.shape == (3, 3, 3, 3) and changed.shape == ()
            if r in bad:
                assert np.isnan(V).all() and not changed
                continue
            lam = h["kelvin_moduli"][r]
            assert bool(changed) == bool((lam < floor).any())
            if not changed:
                assert np.array_equal(V, C[r])                            # identity on stable input, bit for bit
            assert np.array_equal(V, V.T) and cart[0, 1, 2, 2] == V[5, 2] and cart[1, 2, 0, 2] == V[3, 4]
            after = kelvin_host(V)["kelvin_moduli"]
            assert after[0] >= floor - 1e-13 * big[r]                       # min modulus >= floor
            assert np.abs(after - np.maximum(lam, floor)).max() <= 1e-13 * big[r]
            again, _, _ = nearest_stable_host(V, floor)                     # idempotent
            assert np.abs(again - V).max() <= 1e-13 * big[r]
    # it is the nearest: the distance to the input is the norm of the clipped part of the spectrum
    V, cart, changed = nearest_stable_host(C, 0.0)
    assert V.shape == (257, 6, 6) and cart.shape == (257, 3, 3, 3, 3) and changed.dtype == bool
    ok = np.setdiff1d(np.arange(len(C)), bad)
    from matten_amd.elastic import voigt_to_cartesian

    dist = np.sqrt(((cart[ok] - voigt_to_cartesian(C[ok])) ** 2).sum(axis=(1, 2, 3, 4)))
    want = np.sqrt((np.minimum(h["kelvin_moduli"][ok], 0.0) ** 2).sum(axis=1))
    assert (np.abs(dist - want) <= 1e-13 * big[ok]).all()
    assert changed[kinds["indefinite"]].all() and not changed[kinds["n100"]].any() and not changed[bad].any()


# ----------------------------------------------------------------------------------------------------------------------
# the library
# ----------------------------------------------------------------------------------------------------------------------
ENTRIES = ("matten_elastic_kelvin", "matten_elastic_kelvin_bwd", "matten_elastic_kelvin_clamp")


def test_library_declares_binds_and_exports_the_kelvin_entries():
    from matten_amd import _lib

    header = open(os.path.join(ROOT, "include", "matten_hip.h")).read()
    declared = set(re.findall(r"\b(matten_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for name in ENTRIES:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert _lib.ABI_VERSION == 47 and lib.matten_abi_version() == 47          # entries were only added
    assert [len(_lib.SIGNATURES[n][1]) for n in ENTRIES] == [7, 6, 7]
    csrc = os.path.join(ROOT, "matten_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "kelvin.hip" in mk and "sym6.h" in mk
    # one copy of the rotation: sym6.h builds on sym3.h's, kelvin.hip on sym6.h
    sym6, kelvin = open(os.path.join(csrc, "sym6.h")).read(), open(os.path.join(csrc, "kelvin.hip")).read()
    assert '#include "sym3.h"' in sym6 and "void jacobi_rotate" not in sym6 and "void jacobi_turn" not in sym6
    assert "jacobi_rotate(" in sym6 and "jacobi_turn(" in sym6
    assert '#include "sym6.h"' in kelvin and "void jacobi" not in kelvin


def test_bad_arguments_come_back_without_a_device():
    from matten_amd import _lib

    lib = _lib.load()
    fwd, bwd, clamp = (getattr(lib, n) for n in ENTRIES)
    p = 4096      # never dereferenced: every call below returns from the checks
    assert fwd(None, None, 0, None, None, None, None) == 0 and bwd(None, None, None, 0, None, None) == 0
    assert clamp(None, None, None, 0.0, 0, None, None) == 0
    assert fwd(p, p, -1, p, p, p, None) == -1 and bwd(p, p, p, -1, p, None) == -1 and clamp(p, p, p, 0.0, -1, p, None) == -1
    too_many = (2 ** 31 - 1) * 64 + 1
    assert fwd(p, p, too_many, p, p, p, None) == -1 and bwd(p, p, p, too_many, p, None) == -1
    assert clamp(p, p, p, 0.0, too_many, p, None) == -1
    good = [p, p, 5, p, p, p, None]
    for k in (0, 1, 3):                         # voigt, flags, moduli (vectors and dilatation may be NULL)
        args = list(good)
        args[k] = None
        assert fwd(*args) == -1, k
    good = [p, p, p, 5, p, None]
    for k in (0, 1, 2, 4):                      # vectors, flags, g_moduli, g_voigt
        args = list(good)
        args[k] = None
        assert bwd(*args) == -1, k
    good = [p, p, p, 0.0, 5, p, None]
    for k in (0, 1, 2, 5):                      # voigt, moduli, vectors, out
        args = list(good)
        args[k] = None
        assert clamp(*args) == -1, k
    for floor in (-1e-300, float("nan"), float("inf")):
        assert clamp(p, p, p, floor, 5, p, None) == -1, floor


# ----------------------------------------------------------------------------------------------------------------------
# argument checks of the host layers
# ----------------------------------------------------------------------------------------------------------------------
CFG = {"data": {"r_cut": 5.0, "tensor_target_formula": "ijkl=jikl=klij", "tensor_target_name": "elastic_tensor_full"}}


def test_the_kelvin_keyword_is_validated_everywhere():
    from matten_amd import elastic
    from matten_amd import predict as P

    C = np.stack([np.eye(6)] * 2)
    x = torch.zeros(2, 21)
    for fn, arg in ((elastic.elastic_properties, C), (elastic.elastic_properties_from_irreps, x),
                    (elastic.elastic_moduli, torch.zeros(2, 6, 6)), (elastic.elastic_moduli_from_irreps, x)):
        assert inspect.signature(fn).parameters["kelvin"].default is False
        for bad in ("yes", 1, None, 0.0):
            with pytest.raises(ValueError, match="kelvin"):
                fn(arg, kelvin=bad)
    # the differentiable pair still refuses host tensors, with the keyword as without
    with pytest.raises(ValueError, match="elastic_properties"):
        elastic.elastic_moduli(torch.zeros(2, 6, 6), kelvin=True)
    with pytest.raises(ValueError, match="elastic_properties_from_irreps"):
        elastic.elastic_moduli_from_irreps(x, kelvin=True)
    s = {"lattice": 3.0 * np.eye(3), "cart_coords": np.zeros((1, 3)), "atomic_numbers": np.array([13])}
    assert inspect.signature(P.predict).parameters["kelvin"].default is False
    with pytest.raises(ValueError, match="kelvin.*properties=True"):
        P.predict([dict(s)], model=object(), config=CFG, kelvin=True)
    with pytest.raises(ValueError, match="kelvin"):      # (object(): no forward can run)
        P.predict([dict(s)], model=object(), config=CFG, properties=True, kelvin="yes")
    # per-atom models keep raising
    with pytest.raises(ValueError, match="is_atomic_tensor"):
        P.predict([dict(s)], model=object(), config=CFG, is_atomic_tensor=True, properties=True, kelvin=True)
    with pytest.raises(ValueError, match="kelvin.*properties=True"):
        P.predict([dict(s)], model=object(), config=CFG, is_atomic_tensor=True, kelvin=True)


def test_nearest_stable_and_penalty_validate():
    from matten_amd import elastic
    from matten_amd.graphs import stability_penalized, valid_mean_loss

    for bad in (-1.0, float("nan"), float("inf"), "0", None, True):
        with pytest.raises(ValueError, match="floor"):
            elastic.nearest_stable(np.eye(6), floor=bad)
        with pytest.raises(ValueError, match="floor"):
            elastic.nearest_stable_host(np.eye(6), floor=bad)
    with pytest.raises(ValueError, match="tensors"):
        elastic.nearest_stable(np.zeros((4, 5, 5)))
    assert inspect.signature(elastic.nearest_stable).parameters["floor"].default == 0.0
    p = elastic.StabilityPenalty()
    assert p.margin == 0.0 and p.kind == "squared" and elastic.StabilityPenalty(2, "hinge").margin == 2.0
    for bad in (dict(margin=float("nan")), dict(margin=float("inf")), dict(margin="1"), dict(margin=True), dict(kind="l1"),
                dict(kind="mse")):
        with pytest.raises(ValueError):
            elastic.StabilityPenalty(**bad)
    with pytest.raises(ValueError, match="kelvin=True"):
        p(elastic.ElasticProperties(flags=torch.zeros(2, dtype=torch.int32)))
    with pytest.raises(ValueError, match="kelvin=True"):
        elastic.eigenstrains(elastic.ElasticProperties(flags=torch.zeros(2, dtype=torch.int32)))
    base = valid_mean_loss("mse", "elastic_tensor_full")
    fn = stability_penalized(base, 0.1, margin=1.0, kind="hinge", key="elastic_tensor_full")
    assert fn.wants_batch
    for bad in (dict(weight=-1.0), dict(weight=float("nan")), dict(weight="1"), dict(weight=1.0, margin=float("inf")),
                dict(weight=1.0, kind="l2"), dict(weight=1.0, formula="ij=ji"), dict(weight=1.0, inverse=3)):
        with pytest.raises(ValueError):
            stability_penalized(base, **bad)
    with pytest.raises(ValueError, match="base_loss"):
        stability_penalized(None, 1.0)
    # numpy scalars are numbers to all three checks alike
    assert stability_penalized(base, np.float32(0.1), margin=np.float64(1.0)).wants_batch
    assert elastic.StabilityPenalty(np.float32(0.5)).margin == 0.5 and elastic.StabilityPenalty(np.int64(2)).margin == 2.0
    assert not elastic.nearest_stable_host(np.eye(6), floor=np.float32(0.5))[2]
    for entry in (elastic.elastic_moduli, elastic.elastic_moduli_from_irreps):
        assert inspect.signature(entry).parameters["kelvin_dilatation"].default is True
    with pytest.raises(ValueError, match="_amd_n_valid"):      # the base loss's own check comes first
        fn({"elastic_tensor_full": torch.zeros(4, 21)}, torch.zeros(4, 21), {})


def test_penalty_on_host_moduli():
    """``StabilityPenalty`` without ``n_valid`` is a torch expression: on host moduli it is the definition"""
    from matten_amd import elastic

    lam = torch.tensor([[-2.0, 1.0, 2.0, 3.0, 4.0, 5.0], [float("nan")] * 6, [3.0, 3.0, 3.0, 3.0, 3.0, 9.0]],
                       dtype=torch.float64, requires_grad=True)
    props = elastic.ElasticProperties(kelvin_moduli=lam, flags=torch.tensor([2, 1, 0], dtype=torch.int32))
    sq = elastic.StabilityPenalty(1.5, "squared")(props)
    assert sq.dtype == torch.float64 and abs(float(sq.detach()) - (3.5 ** 2 + 0.5 ** 2) / 18.0) <= 1e-15
    hinge = elastic.StabilityPenalty(1.5, "hinge")(props)
    assert abs(float(hinge.detach()) - 4.0 / 18.0) <= 1e-15
    (g,) = torch.autograd.grad(sq, lam)
    want = torch.zeros(3, 6, dtype=torch.float64)
    want[0, 0], want[0, 1] = -2.0 * 3.5 / 18.0, -2.0 * 0.5 / 18.0
    assert torch.allclose(g, want, rtol=1e-15, atol=0.0) and not g[1:].any()     # the NaN row: exact zeros
    zero = elastic.StabilityPenalty(-5.0, "squared")(props)
    assert float(zero.detach()) == 0.0 and not torch.autograd.grad(zero, lam)[0].any()


def test_field_names_with_and_without_kelvin(monkeypatch):
    """the kernels replaced by host stand-ins: which fields exist, in which order, and that nothing else moves"""
    from matten_amd import elastic, ops

    def props(rows, layout):
        B = rows.shape[0]
        return rows.reshape(B, 6, 6).to(torch.float64), torch.zeros(B, 6, 6, dtype=torch.float64), \
            torch.zeros(B, 10, dtype=torch.float64), torch.zeros(B, dtype=torch.int32)

    def kelvin(voigt, flags, want_vectors=True, want_dilatation=True):
        h = elastic.kelvin_host(voigt, flags)
        return tuple(torch.from_numpy(h[k]) for k in ("kelvin_moduli", "kelvin_vectors", "kelvin_dilatation"))

    monkeypatch.setattr(ops, "elastic_props", props)
    monkeypatch.setattr(ops, "elastic_kelvin", kelvin)
    monkeypatch.setattr(elastic, "_upload", lambda rows: rows)
    C = np.stack([isotropic(100.0, 40.0), cubic(100.0, 150.0, 80.0)])
    plain, with_k = elastic.elastic_properties(C), elastic.elastic_properties(C, kelvin=True)
    assert list(with_k._names) == list(plain._names) + list(elastic.KELVIN_NAMES)
    for name in plain._names:
        assert torch.equal(getattr(plain, name), getattr(with_k, name)), name
    assert with_k.kelvin_moduli.shape == (2, 6) and with_k.kelvin_vectors.shape == (2, 6, 6)
    assert with_k.kelvin_dilatation.shape == (2, 6) and with_k.stability_margin.shape == (2,)
    assert abs(float(with_k.stability_margin[1]) + 50.0) <= 1e-12
    assert abs(float(with_k.kelvin_condition[0]) - 3.75) <= 1e-12 and bool(torch.isnan(with_k.kelvin_condition[1]))
    eps = elastic.eigenstrains(with_k)
    assert eps.shape == (2, 6, 3, 3)
    assert np.array_equal(eps.numpy(), elastic.eigenstrains(with_k.kelvin_vectors.numpy()))
    one = elastic.elastic_properties(C[0], kelvin=True)                     # unbatched: no leading dimension
    assert one.kelvin_moduli.shape == (6,) and one.kelvin_vectors.shape == (6, 6) and one.stability_margin.shape == ()
    assert elastic.eigenstrains(one).shape == (6, 3, 3)
    d = with_k.to_dict()
    assert list(d) == list(with_k._names) and d["kelvin_moduli"].dtype == np.float64
