"""
CPU tests of the polycrystal moduli (matten_amd/elastic.py over csrc/polycrystal.hip): the numpy statement of the algorithm,
``polycrystal_host`` / ``polycrystal_bwd_host``, against closed forms, limits, the ordering chain, rotations and a dense scan;
the library's two entries (exported, bad arguments refused without a device); the argument checks of the host layers.  The
GPU tests (tests/test_gpu_polycrystal.py) hold the kernels to the statement tested here; both share tests/polycrystal_cases.py.

The adjoint against central differences.  Step: FD_STEP = 1e-5 max|C| on one symmetric pair of entries, with the fixed
point iterated to sc_tol = 1e-15 on both sides.  Truncation is (step / scale)^2 = 1e-10 times the ratio of third to first
derivative, rounding eps * condition / step: with condition numbers up to ~600 in the seeded tensors that is 1e-16 * 600 /
1e-5 = 6e-9.  FD_TOL = 1e-7 of the largest entry of the row's gradient leaves a factor ~15; measured on this file's 8 rows
x 21 entries: 9.9e-9.
"""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import polycrystal_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FD_STEP, FD_TOL = 1e-5, 1e-7
NAMES6 = ("k_hs_lower", "g_hs_lower", "k_sc", "g_sc", "k_hs_upper", "g_hs_upper")


def mandel(C):
    from matten_amd import elastic

    return elastic.MANDEL_WEIGHT * C


def voigt_reuss(C):
    S = np.linalg.inv(C)
    kv = C[..., :3, :3].sum(axis=(-2, -1)) / 9.0
    kr = 1.0 / S[..., :3, :3].sum(axis=(-2, -1))
    tr = lambda A, idx: sum(A[..., i, i] for i in idx)      # noqa: E731
    off = lambda A: A[..., 0, 1] + A[..., 0, 2] + A[..., 1, 2]      # noqa: E731
    gv = (tr(C, (0, 1, 2)) - off(C) + 3.0 * tr(C, (3, 4, 5))) / 15.0
    gr = 15.0 / (4.0 * tr(S, (0, 1, 2)) - 4.0 * off(S) + 3.0 * tr(S, (3, 4, 5)))
    return kv, gv, kr, gr


@pytest.fixture(scope="module")
def seeded():
    """the 40 seeded positive definite tensors and their polycrystal moduli, computed once"""
    from matten_amd import elastic

    C = pc.random_definite(40, 11)
    return C, elastic.polycrystal_host(C)


# ----------------------------------------------------------------------------------------------------------------------
# closed forms and limits
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("constants", [pc.COPPER, (250.0, 60.0, 40.0)], ids=["mu1<mu2", "mu1>mu2"])
def test_cubic_closed_forms(constants):
    """Hashin & Shtrikman's two closed forms are F at the media (K, mu1) and (K, mu2), Kroener's cubic is the fixed point:
    1e-10 relative.  The medium with the smaller mu is on the lower frontier (2 mu = l_min), so g_hs_lower is its closed
    form; with mu1 > mu2 the two swap roles.  K comes back as K everywhere."""
    from matten_amd import elastic

    K, m1, m2, g1, g2, g_sc = pc.cubic_closed_forms(*constants)
    C = pc.cubic(*constants)
    for mu, want in ((m1, g1), (m2, g2)):
        fk, fg = elastic.polycrystal_F(mandel(C), K, mu)
        assert abs(fg / want - 1.0) <= 1e-10 and abs(fk / K - 1.0) <= 1e-10, (mu, fg, want)
    if constants == pc.COPPER:      # the figures of the issue
        assert abs(g1 - 45.96371053475) <= 1e-10 and abs(g2 - 49.44518428050) <= 1e-10 and abs(g_sc - 48.17198425186) <= 1e-10
    r = elastic.polycrystal_host(C)
    assert r["sc_status"] == 0 and 1 <= r["sc_iterations"] <= 20
    assert abs(r["g_sc"] / g_sc - 1.0) <= 1e-10 and abs(r["k_sc"] / K - 1.0) <= 1e-10
    assert abs(r["g_hs_lower"] / min(g1, g2) - 1.0) <= 1e-10
    assert min(g1, g2) < g_sc < max(g1, g2) <= r["g_hs_upper"] * (1.0 + 1e-12)
    for name in ("k_hs_lower", "k_hs_upper"):
        assert abs(r[name] / K - 1.0) <= 1e-10
    assert abs(r["y_sc"] - 9.0 * K * g_sc / (3.0 * K + g_sc)) <= 1e-9 * r["y_sc"]
    assert abs(r["poisson_sc"] - (3.0 * K - 2.0 * g_sc) / (6.0 * K + 2.0 * g_sc)) <= 1e-10


def test_isotropic_returns_k_g_six_times():
    from matten_amd import elastic

    r = elastic.polycrystal_host(pc.isotropic(160.0, 80.0))
    for q, name in enumerate(NAMES6):
        want = (160.0, 80.0)[q % 2]
        assert abs(r[name] / want - 1.0) <= 1e-12, (name, r[name])
    assert r["sc_status"] == 0 and r["hs_media"].shape == (4, 2) and np.isfinite(r["hs_media"]).all()


def test_f_tends_to_reuss_and_voigt(seeded):
    """C0 = 1e-9 and 1e9 times a medium of the tensor's own size (the Voigt pair): F is Reuss and Voigt.  The distance is
    of first order in the ratio of the medium to the crystal, which along the softest (stiffest) mode is 1e-9 times up to
    the condition number of C^: the bound is 10 * 1e-9 * l_max / l_min per row."""
    from matten_amd import elastic

    C = seeded[0]
    kv, gv, kr, gr = voigt_reuss(C)
    lam = np.linalg.eigvalsh(mandel(C))
    tol = 10.0 * 1e-9 * lam[:, 5] / lam[:, 0]
    fk, fg = elastic.polycrystal_F(mandel(C), 1e-9 * kv, 1e-9 * gv)
    assert (np.abs(fk / kr - 1.0) <= tol).all() and (np.abs(fg / gr - 1.0) <= tol).all()
    fk, fg = elastic.polycrystal_F(mandel(C), 1e9 * kv, 1e9 * gv)
    assert (np.abs(fk / kv - 1.0) <= tol).all() and (np.abs(fg / gv - 1.0) <= tol).all()


def test_ordering_chain(seeded):
    """Reuss <= HS- <= SC <= HS+ <= Voigt for K and for G on 40 seeded tensors (1e-12 relative slack for rounding)"""
    C, r = seeded
    kv, gv, kr, gr = voigt_reuss(C)
    slack = 1.0 + 1e-12
    for lo, hsl, sc, hsu, hi in ((kr, r["k_hs_lower"], r["k_sc"], r["k_hs_upper"], kv),
                                 (gr, r["g_hs_lower"], r["g_sc"], r["g_hs_upper"], gv)):
        assert (lo <= hsl * slack).all() and (hsl <= sc * slack).all() and (sc <= hsu * slack).all() and (hsu <= hi * slack).all()
    assert (r["sc_status"] == 0).all() and r["sc_iterations"].max() <= 60
    # the bounds are tighter than Voigt - Reuss on every tensor, and the optimum is interior on most upper frontiers
    assert ((r["g_hs_upper"] - r["g_hs_lower"]) < (gv - gr)).all()
    lam = np.linalg.eigvalsh(mandel(C))
    assert (r["hs_media"][:, 3, 1] > 0.5 * lam[:, 5] * (1.0 + 1e-9)).mean() > 0.5
    # every medium is feasible: C^ - iso(lower medium) and iso(upper medium) - C^ are positive semi-definite
    from matten_amd import elastic

    for q, sign in ((0, 1.0), (1, 1.0), (2, -1.0), (3, -1.0)):
        gap = sign * (mandel(C) - elastic.iso_mandel(r["hs_media"][:, q, 0], r["hs_media"][:, q, 1]))
        assert (np.linalg.eigvalsh(gap)[:, 0] >= -1e-9 * lam[:, 5]).all(), q


def test_invariance_under_rotation(seeded):
    from matten_amd import elastic

    C, r = seeded
    rng = np.random.default_rng(5)
    R, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    Q = pc.rotation_voigt(R)
    r2 = elastic.polycrystal_host(Q @ C[:8] @ Q.T)
    for name in NAMES6:
        assert np.abs(r2[name] / r[name][:8] - 1.0).max() <= 1e-9, name


def test_search_is_never_worse_than_a_dense_scan(seeded):
    """the grid + golden-section result against a 20 001-point scan of the same frontier (10 tensors): never worse, to
    rounding (1e-12 relative)"""
    from matten_amd import elastic

    C, r = seeded
    C = C[:10]
    Ch, lam, w, *_ = elastic._polycrystal_rows(C, None)
    M = 20001
    scan = {n: np.full(10, -np.inf if "lower" in n else np.inf) for n in ("k_hs_lower", "g_hs_lower", "k_hs_upper", "g_hs_upper")}
    for upper in (False, True):
        for i in range(0 if upper else 1, M if upper else M + 1):
            G0 = elastic._hs_grid_g0(lam, np.full(10, float(i)), M, upper)
            fk, fg = elastic.polycrystal_F(Ch, elastic._hs_frontier_k0(lam, w, G0, upper), G0)
            if upper:
                scan["k_hs_upper"], scan["g_hs_upper"] = np.minimum(scan["k_hs_upper"], fk), np.minimum(scan["g_hs_upper"], fg)
            else:
                scan["k_hs_lower"], scan["g_hs_lower"] = np.maximum(scan["k_hs_lower"], fk), np.maximum(scan["g_hs_lower"], fg)
    for name, best in scan.items():
        if "lower" in name:
            assert (r[name][:10] >= best * (1.0 - 1e-12)).all(), name
        else:
            assert (r[name][:10] <= best * (1.0 + 1e-12)).all(), name


# ----------------------------------------------------------------------------------------------------------------------
# the adjoint
# ----------------------------------------------------------------------------------------------------------------------
def test_adjoint_against_central_differences(seeded):
    from matten_amd import elastic

    C = seeded[0][:8]
    rng = np.random.default_rng(3)
    g = rng.standard_normal((8, 2))
    got = elastic.polycrystal_bwd_host(C, g, sc_tol=1e-15, sc_max_iter=2000)
    assert got.shape == (8, 6, 6) and np.array_equal(got, got.transpose(0, 2, 1))

    def value(Cx):
        rows = elastic._polycrystal_rows(Cx, None)
        K, G, _, _ = elastic._sc_iterate(rows[0], rows[1], rows[2], 1e-15, 2000)
        return g[:, 0] * K + g[:, 1] * G

    h = FD_STEP * np.abs(C).max(axis=(1, 2))
    worst = 0.0
    for i in range(6):
        for j in range(i, 6):
            E = np.zeros((6, 6))
            E[i, j] = E[j, i] = 1.0
            fd = (value(C + h[:, None, None] * E) - value(C - h[:, None, None] * E)) / (2.0 * h)
            an = got[:, i, j] * (1.0 if i == j else 2.0)
            worst = max(worst, (np.abs(fd - an) / np.abs(got).max(axis=(1, 2))).max())
    print(f"adjoint vs central differences: {worst:.2e} of the row's largest entry")
    assert worst <= FD_TOL


def test_adjoint_rows_without_a_value_are_zero():
    from matten_amd import elastic

    C = pc.batch()[[pc.ROW_CUBIC, pc.ROW_NOT_PD, pc.ROW_NAN]]
    g = elastic.polycrystal_bwd_host(C, np.ones((3, 2)))
    assert np.abs(g[0]).max() > 0 and (g[1:] == 0.0).all()


# ----------------------------------------------------------------------------------------------------------------------
# row states and arguments
# ----------------------------------------------------------------------------------------------------------------------
def test_status_codes():
    from matten_amd import elastic

    C = pc.batch()[[pc.ROW_CUBIC, pc.ROW_CUBIC, pc.ROW_NOT_PD, pc.ROW_NAN, pc.ROW_HEXAGONAL]]
    r = elastic.polycrystal_host(C, flags=np.array([0, 1, 0, 0, 2]))      # row 1: flagged singular; row 4: flagged not PD
    assert list(r["sc_status"]) == [0, -1, 2, -1, 2] and list(r["sc_iterations"][1:]) == [0, 0, 0, 0]
    for name in NAMES6 + ("y_sc", "poisson_sc"):
        assert np.isfinite(r[name][0]) and np.isnan(r[name][1:]).all(), name
    assert np.isnan(r["hs_media"][1:]).all()
    capped = elastic.polycrystal_host(pc.cubic(*pc.COPPER), sc_max_iter=2)
    full = elastic.polycrystal_host(pc.cubic(*pc.COPPER))
    assert capped["sc_status"] == 1 and capped["sc_iterations"] == 2 and full["sc_status"] == 0
    assert full["g_sc"] < capped["g_sc"] < voigt_reuss(pc.cubic(*pc.COPPER))[1]      # on its way down from Voigt
    assert capped["g_hs_lower"] == full["g_hs_lower"]


def test_argument_errors():
    from matten_amd import elastic
    from matten_amd import predict as P

    C = np.stack([pc.cubic(*pc.COPPER)] * 2)
    x = torch.zeros(2, 21)
    bad = (dict(hs_grid=1), dict(hs_grid=2.5), dict(hs_grid=True), dict(sc_tol=0.0), dict(sc_tol=float("nan")),
           dict(sc_tol=float("inf")), dict(sc_tol=-1e-12), dict(sc_max_iter=0), dict(sc_max_iter=1.5))
    for kw in bad:
        with pytest.raises(ValueError, match=next(iter(kw))):
            elastic.polycrystal_host(C, **kw)
        for fn, arg in ((elastic.elastic_properties, C), (elastic.elastic_properties_from_irreps, x),
                        (elastic.elastic_moduli, torch.zeros(2, 6, 6)), (elastic.elastic_moduli_from_irreps, x)):
            with pytest.raises(ValueError, match=next(iter(kw))):      # before anything is uploaded: no device here
                fn(arg, polycrystal=True, **kw)
    for fn, arg in ((elastic.elastic_properties, C), (elastic.elastic_moduli_from_irreps, x)):
        with pytest.raises(ValueError, match="polycrystal"):
            fn(arg, polycrystal=1)
    with pytest.raises(ValueError, match="properties=True"):
        P.predict([{}], polycrystal=True)
    for fn in (elastic.elastic_properties, elastic.elastic_properties_from_irreps, elastic.elastic_moduli,
               elastic.elastic_moduli_from_irreps, P.predict):
        sig = inspect.signature(fn).parameters
        assert sig["polycrystal"].default is False and sig["hs_grid"].default == 64
        assert sig["sc_tol"].default == 1e-12 and sig["sc_max_iter"].default == 200


def test_moduli_loss_names():
    from matten_amd import elastic

    assert tuple(elastic.POLYCRYSTAL_NAMES) == ("k_sc", "g_sc", "y_sc", "poisson_sc")
    assert elastic.PROP_NAMES == ("k_voigt", "g_voigt", "k_reuss", "g_reuss", "k_vrh", "g_vrh", "y_mod", "homogeneous_poisson",
                                  "universal_anisotropy", "pugh_ratio")
    loss = elastic.ModuliLoss(("k_sc", "g_sc", "y_sc", "poisson_sc", "k_vrh"))
    assert loss.names[:2] == ("k_sc", "g_sc")
    with pytest.raises(ValueError, match="k_hs_lower"):
        elastic.ModuliLoss(("k_hs_lower",))
    props = elastic.ElasticProperties(flags=torch.zeros(2, dtype=torch.int32), k_vrh=torch.ones(2, dtype=torch.float64))
    with pytest.raises(ValueError, match="polycrystal=True"):
        elastic.ModuliLoss(("k_sc",))(props, {"k_sc": torch.ones(2)})
    # a row without a value (not positive definite: NaN, flag bit 0 clear) is excluded, never multiplied away
    k = torch.tensor([2.0, float("nan")], dtype=torch.float64, requires_grad=True)
    props = elastic.ElasticProperties(flags=torch.zeros(2, dtype=torch.int32), k_sc=k)
    value = elastic.ModuliLoss(("k_sc",))(props, {"k_sc": torch.tensor([1.0, 1.0], dtype=torch.float64)})
    value.backward()
    assert value.item() == 1.0 and k.grad.tolist() == [1.0, 0.0]


def test_without_the_flag_nothing_changes():
    """the fields of a result made without ``polycrystal`` (here: the field list ``_from_rows`` builds, read off its source,
    since no device is at hand) hold none of the new names; with it they are exactly ``POLYCRYSTAL_FIELDS``"""
    from matten_amd import elastic

    fields = elastic._polycrystal_fields(torch.zeros(3, 6, dtype=torch.float64), torch.zeros(3, 8, dtype=torch.float64),
                                         torch.zeros(3, 2, dtype=torch.int32))
    assert set(fields) == set(elastic.POLYCRYSTAL_FIELDS) and fields["hs_media"].shape == (3, 4, 2)
    src = inspect.getsource(elastic._from_rows) + inspect.getsource(elastic._moduli_fields)
    assert src.count("if polycrystal:") == 2 and src.count("_polycrystal_fields(") == 2
    base = elastic.ElasticProperties(flags=torch.zeros(2, dtype=torch.int32), k_vrh=torch.ones(2))
    assert not set(base.to_dict()) & set(elastic.POLYCRYSTAL_FIELDS)


# ----------------------------------------------------------------------------------------------------------------------
# the library
# ----------------------------------------------------------------------------------------------------------------------
ENTRIES = ("matten_elastic_polycrystal", "matten_elastic_polycrystal_bwd")


def test_library_declares_binds_and_exports_the_entries():
    from matten_amd import _lib

    header = open(os.path.join(ROOT, "include", "matten_hip.h")).read()
    declared = set(re.findall(r"\b(matten_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for name in ENTRIES:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.matten_abi_version() == _lib.ABI_VERSION
    assert [len(_lib.SIGNATURES[n][1]) for n in ENTRIES] == [12, 8]
    assert "polycrystal.hip" in open(os.path.join(ROOT, "matten_amd", "csrc", "Makefile")).read()


def test_bad_arguments_come_back_without_a_device():
    from matten_amd import _lib

    lib = _lib.load()
    fwd, bwd = (getattr(lib, n) for n in ENTRIES)
    p = 4096      # never dereferenced: every call below returns from the checks
    assert fwd(None, None, None, None, 0, 64, 1e-12, 200, None, None, None, None) == 0
    assert bwd(None, None, None, None, None, 0, None, None) == 0
    good = [p, p, p, p, 5, 64, 1e-12, 200, p, p, p, None]
    too_many = (2 ** 31 - 1) * 64 + 1
    for k, value in ((4, -1), (4, too_many), (5, 1), (5, 0), (5, -3), (6, 0.0), (6, -1e-12), (6, float("nan")),
                     (6, float("inf")), (7, 0), (7, -1), (0, None), (1, None), (2, None), (3, None), (8, None), (10, None)):
        args = list(good)
        args[k] = value
        assert fwd(*args) == -1, (k, value)
    good = [p, p, p, p, p, 5, p, None]
    for k, value in ((5, -1), (5, too_many), (0, None), (1, None), (2, None), (3, None), (4, None), (6, None)):
        args = list(good)
        args[k] = value
        assert bwd(*args) == -1, (k, value)
