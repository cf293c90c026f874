"""
Group velocities, polarisations and phonon focusing without a device: the C entry's export and argument checks, and
``acoustic_waves_host`` -- the numpy statement of the definitions that test_gpu_waves.py holds the kernel to -- against what
does not depend on it: the eigen-equation, Euler's identity g.n = v, central differences of omega(q) and of the unit group
direction, and the closed forms of isotropic and cubic crystals.

Finite-difference tolerances (K = 9 max|C|, dl = FACTOR eps K the eigenvalue error, D_k the branch's eigenvalue gap):
  g against (omega(q + h e_a) - omega(q - h e_a)) / 2h, h = 1e-6: rounding 2 (dl s / 2 omega) / 2h, truncation
  h^2 |omega'''| / 6 with |lambda'''| / 6 <= 4 (2 K)^3 / D_k^2 (third-order perturbation theory, Gamma(q) quadratic in q),
  carried to omega by s / 2 omega.  Near an acoustic axis the bound is useless and says so; elsewhere it is ~1e-7 |g|.
  J against central differences of g^ along e1 and e2, h = 1e-5, on modes with relative gap >= 1e-2: rtol 1e-5.  A
  gross-error check: a wrong term of the derivative is an O(1) error.
"""
import inspect
import os
import re

import numpy as np
import pytest

import waves_cases as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "matten_elastic_waves"
VOIGT = np.array([[0, 5, 4], [5, 1, 3], [4, 3, 2]])


def _waves():
    from matten_amd import waves

    return waves


def cart(C):
    return C[VOIGT[:, :, None, None], VOIGT[None, None, :, :]]


@pytest.fixture(scope="module")
def host65():
    W = _waves()
    return W.acoustic_waves_host(wc.crystals(), np.ones(6), 65, modulus_unit=1.0, deg_tol=wc.DEG_TOL)


def test_entry_is_exported_and_bound():
    from matten_amd import _lib, ops

    header = open(os.path.join(ROOT, "include", "matten_hip.h")).read()
    declared = set(re.findall(r"\b(matten_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    assert ENTRY in declared and ENTRY in _lib.SIGNATURES and hasattr(lib, ENTRY)
    assert lib.matten_abi_version() == _lib.ABI_VERSION == 47          # entries were only added
    assert len(_lib.SIGNATURES[ENTRY][1]) == 16
    assert "waves.hip" in open(os.path.join(ROOT, "matten_amd", "csrc", "Makefile")).read()
    assert callable(ops.elastic_waves)


def test_bad_arguments_come_back_without_a_device():
    from matten_amd import _lib

    fn = getattr(_lib.load(), ENTRY)
    p = 4096      # never dereferenced: every call below returns from the checks
    assert fn(None, None, None, None, 0, 1, 1.0, 1e-6, None, None, None, None, None, None, None, None) == 0
    good = [p, p, p, p, 3, 7, 1e9, 1e-6, None, None, None, p, p, p, p, None]
    for k, value in ((4, -1), (5, 0), (5, -3), (5, 2 ** 31), (7, -1e-9), (7, float("nan")), (7, float("inf")), (0, None),
                     (1, None), (2, None), (3, None), (11, None), (12, None), (13, None), (14, None)):
        args = list(good)
        args[k] = value
        assert fn(*args) == -1, (k, value)


@pytest.mark.parametrize("D", [65, 200])
def test_no_fixture_mode_is_near_the_degeneracy_threshold(D):
    W = _waves()
    extra = wc.random_triclinic(64)
    for C in (wc.crystals(), extra[:8] if D == 200 else extra):
        out = W.acoustic_waves_host(C, np.ones(len(C)), D, modulus_unit=1.0, deg_tol=wc.DEG_TOL)
        assert (out["n_degenerate"] == 0).all() and (out["n_unstable"] == 0).all()
        assert out["relative_gap"].min() >= 3.0 * wc.DEG_TOL
        assert np.isfinite(out["focusing_jacobian"]).all() and np.isfinite(out["group_velocity"]).all()


def test_eigen_equation_and_euler_identity(host65):
    C, n = wc.crystals(), host65["directions"]
    for b in range(6):
        G = np.einsum("ijkl,dj,dl->dik", cart(C[b]), n, n)
        u, v, g = host65["polarisation"][b], host65["phase_velocity"][b], host65["group_velocity"][b]
        lam = v * v
        assert (np.diff(lam, axis=1) >= 0).all()
        resid = np.einsum("dik,dmk->dmi", G, u) - lam[:, :, None] * u
        assert np.abs(resid).max() <= wc.FACTOR * wc.EPS * 9 * np.abs(C[b]).max()
        assert np.abs(np.linalg.norm(u, axis=2) - 1).max() <= 8 * wc.EPS
        assert (np.einsum("dmi,di->dm", u, n) >= -1e-9).all()
        np.testing.assert_allclose(np.einsum("dmi,di->dm", g, n), v, rtol=wc.FACTOR * wc.EPS, atol=0)
        np.testing.assert_allclose(host65["group_speed"][b], np.linalg.norm(g, axis=2), rtol=4 * wc.EPS)
        assert (host65["group_speed"][b] >= v * (1 - 4 * wc.EPS)).all()
        np.testing.assert_allclose(host65["longitudinal_character"][b].sum(axis=1), 1.0, rtol=0, atol=16 * wc.EPS)
        with np.errstate(divide="ignore"):
            assert np.array_equal(host65["enhancement"][b], 1.0 / np.abs(host65["focusing_jacobian"][b]))


def test_group_velocity_is_the_gradient_of_omega(host65):
    C, n, h = wc.crystals(), host65["directions"], 1e-6
    for b in range(6):
        c4 = cart(C[b])

        def omega(q):
            return np.sqrt(np.linalg.eigvalsh(np.einsum("ijkl,dj,dl->dik", c4, q, q)))      # [D,3]

        fd = np.stack([(omega(n + h * e) - omega(n - h * e)) / (2 * h) for e in np.eye(3)], axis=2)      # [D,3 branches,3]
        v = host65["phase_velocity"][b]
        K = 9 * np.abs(C[b]).max()
        gap = host65["relative_gap"][b] * (v[:, 2:3] ** 2)
        tol = (wc.FACTOR * wc.EPS * K / (2 * v)) / h + h * h * 4 * (2 * K) ** 3 / gap ** 2 / (2 * v)
        err = np.abs(fd - host65["group_velocity"][b]).max(axis=2)
        assert (err <= tol).all(), (wc.NAMES[b], float((err / tol).max()))
        tight = host65["relative_gap"][b] >= 1e-2
        assert tight[:, 2].all() and (err[tight] <= 1e-6 * host65["group_speed"][b][tight]).all()


def test_focusing_jacobian_against_differences_of_the_group_direction(host65):
    W = _waves()
    from matten_amd.elastic import pair_frame

    C, n, h = wc.crystals(), host65["directions"], 1e-5
    frames = [pair_frame(x) for x in n]
    moved = []
    for axis in (0, 1):
        for sign in (1.0, -1.0):
            moved.append(np.stack([x + sign * h * f[axis] for x, f in zip(n, frames)]))
    shifted = [W.acoustic_waves_host(C, np.ones(6), m, modulus_unit=1.0, deg_tol=wc.DEG_TOL) for m in moved]

    def unit(out):
        return out["group_velocity"] / out["group_speed"][..., None]

    # (check_directions normalises n +- h e: a second-order change of the step)
    d1 = (unit(shifted[0]) - unit(shifted[1])) / (2 * h)
    d2 = (unit(shifted[2]) - unit(shifted[3])) / (2 * h)
    J_fd = np.einsum("bdki,bdki->bdk", unit(host65), np.cross(d1, d2))
    J = host65["focusing_jacobian"]
    tight = host65["relative_gap"] >= 1e-2
    assert tight.sum() >= 600
    rel = np.abs(J - J_fd)[tight] / np.abs(J)[tight]
    print("J against differences: largest relative error", float(rel.max()), "smallest |J|", float(np.abs(J)[tight].min()))
    assert (rel <= 1e-5).all(), float(rel.max())


def test_isotropic_closed_form():
    W = _waves()
    K, G, rho, D = 100.0, 40.0, 2.5, 33
    out = W.acoustic_waves_host(wc.isotropic(K, G), rho, D, modulus_unit=1.0, deg_tol=1e-6)
    n = out["directions"]
    assert np.array_equal(out["n_degenerate"], [D, D, 0]) and out["n_unstable"] == 0
    for name in ("group_speed", "power_flow_angle", "longitudinal_character", "focusing_jacobian", "enhancement"):
        assert np.isnan(out[name][:, :2]).all(), name
    assert np.isnan(out["polarisation"][:, :2]).all() and np.isnan(out["group_velocity"][:, :2]).all()
    tol = wc.FACTOR * wc.EPS
    vt, vl = np.sqrt(G / rho), np.sqrt((K + 4 * G / 3) / rho)
    np.testing.assert_allclose(out["phase_velocity"][:, :2], vt, rtol=tol)
    np.testing.assert_allclose(out["phase_velocity"][:, 2], vl, rtol=tol)
    np.testing.assert_allclose(out["group_velocity"][:, 2], vl * n, rtol=0, atol=tol * vl)
    np.testing.assert_allclose(out["polarisation"][:, 2], n, rtol=0, atol=tol)
    # psi = acos(c) with c within 64 eps of 1: at most acos(1 - 64 eps)
    assert (out["power_flow_angle"][:, 2] <= np.arccos(1 - tol)).all()
    np.testing.assert_allclose(out["longitudinal_character"][:, 2], 1.0, rtol=0, atol=tol)
    np.testing.assert_allclose(out["focusing_jacobian"][:, 2], 1.0, rtol=0, atol=tol)
    assert np.isnan(out["power_flow_angle_max"][:2]).all() and (out["power_flow_angle_max_index"][:2] == -1).all()
    assert np.isnan(out["focusing_min_jacobian"][:2]).all() and (out["focusing_min_jacobian_index"][:2] == -1).all()
    assert out["focusing_min_jacobian_index"][2] >= 0


@pytest.mark.parametrize("c11,c12,c44", [(168.4, 121.4, 75.4), (107.3, 60.9, 28.3)])
def test_cubic_along_110(c11, c12, c44):
    W = _waves()
    rho = 8.96
    r = np.sqrt(0.5)
    out = W.acoustic_waves_host(wc.cubic(c11, c12, c44), rho, np.array([[1.0, 1.0, 0.0]]), modulus_unit=1.0)
    tol = wc.FACTOR * wc.EPS
    modes = sorted([((c11 + c12 + 2 * c44) / 2, [r, r, 0.0]), (c44, [0.0, 0.0, 1.0]), ((c11 - c12) / 2, [r, -r, 0.0])])
    np.testing.assert_allclose(out["phase_velocity"][0], [np.sqrt(m / rho) for m, _ in modes], rtol=tol)
    for k, (_, u) in enumerate(modes):
        got = out["polarisation"][0, k]
        assert abs(abs(got @ np.array(u)) - 1) <= tol
        assert np.array_equal(got, W.sign_rule(got, out["directions"][0]))      # (the rule is idempotent)
    # a transverse mode with u.n = 0 exactly or to rounding: the rule falls through to e1 / e2 and still fixes one sign
    assert (out["power_flow_angle"][0] <= np.arccos(1 - tol)).all()
    np.testing.assert_allclose(out["longitudinal_character"][0], [(np.array(u) @ out["directions"][0]) ** 2 for _, u in modes],
                               atol=tol)


def test_sign_rule_falls_through_the_frame():
    W = _waves()
    from matten_amd.elastic import pair_frame

    n = np.array([0.0, 0.0, 1.0])
    e1, e2 = pair_frame(n)
    assert np.allclose(np.cross(e1, e2), n)
    assert np.array_equal(W.sign_rule(-n, n), n)
    assert np.array_equal(W.sign_rule(-e1, n), e1) and np.array_equal(W.sign_rule(e1, n), e1)
    assert np.array_equal(W.sign_rule(-e2, n), e2) and np.array_equal(W.sign_rule(e2 + 1e-10 * e1, n), e2 + 1e-10 * e1)
    assert np.array_equal(W.sign_rule(-(e2 + 1e-10 * e1), n), e2 + 1e-10 * e1)


def test_bad_rows_unstable_directions_and_single_input():
    W = _waves()
    C = wc.crystals()[[2, 2, 2, 2]].copy()
    C[1, 0, 3] = np.nan
    C[2] = wc.cubic(100.0, 50.0, -60.0)           # negative shear modulus: every direction has a negative eigenvalue
    out = W.acoustic_waves_host(C, [8960.0, 1.0, 1.0, -1.0], 9, flags=[0, 1, 2, 0])
    for b in (1, 3):
        assert np.isnan(out["phase_velocity"][b]).all() and np.isnan(out["focusing_min_jacobian"][b]).all()
        assert (out["n_degenerate"][b] == -1).all() and out["n_unstable"][b] == -1
        assert (out["power_flow_angle_max_index"][b] == -1).all()
    assert out["n_unstable"][2] == 9 and (out["n_degenerate"][2] == 0).all() and np.isnan(out["phase_velocity"][2]).all()
    assert np.isfinite(out["group_velocity"][0]).all() and out["n_unstable"][0] == 0
    one = W.acoustic_waves_host(C[0], 8960.0, 9)
    for k, v in one.items():
        if k != "directions":
            assert np.array_equal(v, out[k][0], equal_nan=True), k


def test_argument_errors_before_any_work():
    W = _waves()
    from matten_amd import predict as P

    C = wc.crystals()
    for bad in (-1e-9, float("nan"), float("inf"), "1e-6", True, None):
        with pytest.raises(ValueError, match="deg_tol"):
            W.acoustic_waves_host(C, np.ones(6), 5, deg_tol=bad)
        with pytest.raises(ValueError, match="deg_tol"):
            W.acoustic_waves(C, np.ones(6), 5, deg_tol=bad)
    with pytest.raises(ValueError, match="density"):
        W.acoustic_waves(C, np.ones(5), 5)
    with pytest.raises(ValueError, match="density"):
        W.acoustic_waves(C, -np.ones(6), 5)
    with pytest.raises(ValueError, match="directions"):
        W.acoustic_waves(C, np.ones(6), np.zeros((2, 3)))
    s = {"lattice": 4.0 * np.eye(3), "cart_coords": np.zeros((1, 3)), "atomic_numbers": np.array([14])}
    with pytest.raises(ValueError, match="direction"):
        P.predict([s], properties=True, waves=True, density=[2330.0])
    with pytest.raises(ValueError, match="waves.*direction"):
        P.predict([s], properties=True, waves=True)
    with pytest.raises(ValueError, match="waves.*density"):
        P.predict([s], properties=True, waves=True, directions=9)
    with pytest.raises(ValueError, match="waves.*properties=True"):
        P.predict([s], waves=True)
    with pytest.raises(ValueError, match="deg_tol"):
        P.predict([s], properties=True, waves=True, directions=9, density=[2330.0], deg_tol=-1.0)
    with pytest.raises(ValueError, match="waves"):
        P.predict([s], properties=True, waves="yes", directions=9, density=[2330.0])


def test_the_new_arguments_are_off_by_default():
    from matten_amd import elastic as E
    from matten_amd import predict as P

    names = list(inspect.signature(P.predict).parameters)
    # (behind the other derived-property arguments; ``shielding`` stays the last one, as test_rank2_host.py pins it)
    assert names[-3:] == ["waves", "deg_tol", "shielding"] and names[-4] == "sc_max_iter"
    assert inspect.signature(P.predict).parameters["waves"].default is False
    for fn in (E.elastic_properties, E.elastic_properties_from_irreps, E.elastic_moduli):
        assert "waves" not in inspect.signature(fn).parameters
