"""
CPU tests of the refinement of the directional elastic extremes (``refine=True``, matten_elastic_refine): the C entry's
declaration and binding, ``elastic.refine_extremes_host`` -- the numpy statement of the iteration the kernel runs -- against
closed forms of cubic crystals and against an independent optimiser (scipy BFGS on a spherical parametrisation), its
contract on isotropic, indefinite and singular rows, the argument errors, and the field names with and without ``refine``.
No kernel is launched.
"""
import inspect
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = {"data": {"r_cut": 5.0, "tensor_target_name": "elastic_tensor_full", "tensor_target_formula": "ijkl=jikl=klij"}}
D, M = 64, 16

# the field names of ElasticProperties before the refinement existed, in order, per group of arguments
BASE_FIELDS = ["voigt", "compliance", "k_voigt", "g_voigt", "k_reuss", "g_reuss", "k_vrh", "g_vrh", "y_mod",
               "homogeneous_poisson", "universal_anisotropy", "pugh_ratio", "flags", "is_stable", "is_singular"]
DIR_FIELDS = ["young", "compressibility", "young_min", "young_max", "young_argmin", "young_argmax", "compressibility_min",
              "compressibility_max", "compressibility_argmin", "compressibility_argmax", "directions"]
PAIR_FIELDS = (["angles"] + [n + s for n in ("shear_min", "shear_max", "poisson_min", "poisson_max")
                             for s in ("", "_direction", "_angle")]
               + ["shear_dir_min", "shear_dir_max", "poisson_dir_min", "poisson_dir_max"])
ACOUSTIC_FIELDS = ["velocities", "v_slow_min", "v_fast_max", "v_slow_min_direction", "v_fast_max_direction", "sum_inv_v3",
                   "v_mean", "acoustic_unstable_directions", "debye_temperature"]


def cubic(c11, c12, c44):
    C = np.zeros((6, 6))
    C[:3, :3] = c12
    C[[0, 1, 2], [0, 1, 2]] = c11
    C[[3, 4, 5], [3, 4, 5]] = c44
    return C


def isotropic(K, G):
    return cubic(K + 4.0 * G / 3.0, K - 2.0 * G / 3.0, G)


def random_spd(rng):
    A = rng.normal(size=(6, 6))
    return A @ A.T + 6.0 * rng.uniform(0.2, 2.0) * np.eye(6)


def sign_of(name):
    return 1.0 if name.endswith("_max") else -1.0


def test_library_declares_and_binds_the_refine_entry():
    from matten_amd import _lib, ops

    header = open(os.path.join(ROOT, "include", "matten_hip.h")).read()
    declared = set(re.findall(r"\b(matten_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    assert "matten_elastic_refine" in declared and "matten_elastic_refine" in _lib.SIGNATURES
    assert hasattr(lib, "matten_elastic_refine") and callable(ops.elastic_refine)
    assert _lib.ABI_VERSION == 47 and lib.matten_abi_version() == 47          # entries were only added
    # host-detectable argument errors, no GPU touched: (n, n_dirs, n_angles, tol, max_iter)
    call = lambda n, nd, na, tol=1e-9, it=32: lib.matten_elastic_refine(None, None, None, None, None, None, None, None, n, nd, na,
                                                                         tol, it, None, None, None, None, None, None)
    assert call(0, 5, 3) == 0 and call(0, 5, 0) == 0                          # n == 0 is fine, with and without angles
    assert call(2, 5, 3) == -1                                                # null pointers
    assert call(0, 0, 3) == -1 and call(0, 5, -1) == -1 and call(-1, 5, 3) == -1
    assert call(0, 1 << 20, 1 << 11) == -1 and call(0, 1 << 20, (1 << 11) - 1) == 0      # D M <= 2^31 - 1
    assert call(0, 5, 3, 0.0) == -1 and call(0, 5, 3, float("nan")) == -1 and call(0, 5, 3, float("inf")) == -1
    assert call(0, 5, 3, 1e-9, -1) == -1 and call(0, 5, 3, 1e-9, 0) == 0


# Zener anisotropy A = 2 c44 / (c11 - c12) above and below 1 (copper-like 3.19, and 0.6, 0.48, 1.5, 2.8)
CUBIC = [(168.0, 121.0, 75.0), (300.0, 100.0, 60.0), (250.0, 50.0, 150.0), (210.0, 45.0, 40.0), (120.0, 70.0, 70.0)]


@pytest.mark.parametrize("c11,c12,c44", CUBIC)
def test_host_refinement_meets_the_closed_forms_of_cubic_crystals(c11, c12, c44):
    from matten_amd import elastic

    C = cubic(c11, c12, c44)
    S = np.linalg.inv(C)
    r = elastic.refine_extremes_host(S, D, M)
    s11, s12, s44 = S[0, 0], S[0, 1], S[3, 3]
    J = s11 - s12 - 0.5 * s44
    young = (1.0 / s11, 1.0 / (s11 - 2.0 * J / 3.0))
    shear = (c44, 0.5 * (c11 - c12))
    want = {"young_min": min(young), "young_max": max(young), "shear_min": min(shear), "shear_max": max(shear),
            "compressibility_min": s11 + 2.0 * s12, "compressibility_max": s11 + 2.0 * s12}
    for name, exact in want.items():
        got = r[name]
        print(f"A={2 * c44 / (c11 - c12):.2f} {name}: refined {got['value']!r} exact {exact!r} grid {got['grid_value']!r} "
              f"iterations {got['iterations']}")
        assert got["status"] == elastic.REFINE_CONVERGED and got["iterations"] <= 12
        assert abs(got["value"] - exact) <= 1e-10 * abs(exact)
    for name in ("young_min", "young_max", "shear_min", "shear_max"):      # the grid alone misses them
        if r[name]["iterations"] > 0:
            assert abs(r[name]["grid_value"] - want[name]) > 1e-6 * abs(want[name])


def _evaluate(name, S, n, m):
    from matten_amd import elastic

    kind = 0 if name.startswith("young") else 1 if name.startswith("shear") else 2
    return elastic._refine_eval(kind, S, n, m)[0]


def _bfgs(name, S, n0, m0):
    """the extreme of the same basin by scipy's BFGS over (theta, phi, psi): n on the sphere in a basis that puts the start on
    the equator (phi = 0), m at the angle psi in n's tangent frame (e_theta, e_phi); the start pair is (pi/2, 0, pi/2)"""
    from scipy.optimize import minimize

    Q = np.stack([n0, m0, np.cross(n0, m0)], axis=1)
    sign = sign_of(name)
    scale = abs(_evaluate(name, S, n0, m0))

    def pair(x):
        th, ph, ps = x
        n = Q @ np.array([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)])
        e_th = Q @ np.array([np.cos(th) * np.cos(ph), np.cos(th) * np.sin(ph), -np.sin(th)])
        e_ph = Q @ np.array([-np.sin(ph), np.cos(ph), 0.0])
        return n, np.cos(ps) * e_th + np.sin(ps) * e_ph

    x = np.array([0.5 * np.pi, 0.0, 0.5 * np.pi])
    assert np.allclose(pair(x)[0], n0, atol=1e-15) and np.allclose(pair(x)[1], m0, atol=1e-15)
    objective = lambda x: -sign * _evaluate(name, S, *pair(x)) / scale
    for _ in range(3):      # (restarts rebuild the inverse Hessian; finite-difference gradients stall a single run early)
        x = minimize(objective, x, method="BFGS", options={"gtol": 1e-9, "maxiter": 500}).x
    return -sign * objective(x) * scale, pair(x)


def test_host_refinement_agrees_with_an_independent_optimiser():
    from matten_amd import elastic

    rng = np.random.default_rng(20260)
    worst = {}
    for t in range(24):
        S = np.linalg.inv(random_spd(rng))
        r = elastic.refine_extremes_host(S, D, M)
        dirs, table = elastic.fibonacci_hemisphere(D), elastic.angle_table(M)
        for name in ("young_min", "young_max", "shear_min", "shear_max", "poisson_min", "poisson_max"):
            got = r[name]
            assert got["status"] == elastic.REFINE_CONVERGED and got["iterations"] <= 12, (t, name, got)
            n0 = dirs[got["grid_direction"]]
            e1, e2 = elastic.pair_frame(n0)
            k = got["grid_angle"] if name.startswith(("shear", "poisson")) else 0
            m0 = table[k, 0] * e1 + table[k, 1] * e2
            assert _evaluate(name, S, n0, m0) == pytest.approx(got["grid_value"], rel=1e-13)   # the start is the grid winner
            want, _ = _bfgs(name, S, n0, m0)
            err = abs(got["value"] - want) / (1.0 if name.startswith("poisson") else abs(want))
            worst[name] = max(worst.get(name, 0.0), err)
            assert err <= 1e-9, (t, name, got["value"], want)
            assert sign_of(name) * got["value"] >= sign_of(name) * got["grid_value"]
    print("largest |restatement - BFGS| (relative; absolute for poisson):", worst)


def _contract_batch():
    rng = np.random.default_rng(3)
    C = [random_spd(rng) for _ in range(4)] + [cubic(168.0, 121.0, 75.0), isotropic(100.0, 40.0),
                                               np.diag([5.0, 4.0, 3.0, 2.0, 1.0, -1.0])]
    S = np.array([np.linalg.inv(c) for c in C] + [np.full((6, 6), np.nan)])
    return S, 5, 6, 7          # (compliances, index of the isotropic, the indefinite and the singular row)


def test_host_refinement_contract():
    from matten_amd import elastic

    S, iso, indefinite, singular = _contract_batch()
    r = elastic.refine_extremes_host(S, D, M)
    assert tuple(r) == elastic.REFINE_NAMES
    assert tuple(elastic.refine_extremes_host(S, D)) == elastic.REFINE_NAMES[:4]          # without angles: E and beta only
    dirs = elastic.fibonacci_hemisphere(D)
    for name, o in r.items():
        sign = sign_of(name)
        # isotropic: no gradient at all
        assert o["status"][iso] == 0 and o["iterations"][iso] == 0
        assert abs(o["value"][iso] - o["grid_value"][iso]) <= 1e-14 * abs(o["grid_value"][iso])
        # indefinite: nothing is followed, grid value and pair bit for bit
        assert o["status"][indefinite] == 2 and o["iterations"][indefinite] == 0
        assert o["value"][indefinite].tobytes() == o["grid_value"][indefinite].tobytes()
        assert o["n"][indefinite].tobytes() == dirs[o["grid_direction"][indefinite]].tobytes()
        # singular: NaN
        assert o["status"][singular] == -1 and o["iterations"][singular] == 0
        assert np.isnan(o["value"][singular]) and np.isnan(o["n"][singular]).all() and np.isnan(o["m"][singular]).all()
        ok = np.arange(len(S)) != singular
        assert (sign * o["value"][ok] >= sign * o["grid_value"][ok]).all()              # never worse than the grid
        assert (o["iterations"] <= 32).all() and set(o["status"].tolist()) <= {0, 2, -1}
        assert np.allclose(np.linalg.norm(o["n"][ok], axis=1), 1.0, atol=1e-12, rtol=0)
        assert np.allclose(np.linalg.norm(o["m"][ok], axis=1), 1.0, atol=1e-12, rtol=0)
        assert (np.abs(np.einsum("bi,bi->b", o["n"][ok], o["m"][ok])) <= 1e-12).all()
    for b in range(5):          # beta: the extreme eigenvalues of B_ij = sum_k S_ijkk
        Ssym = 0.5 * (S[b] + S[b].T)
        ev = np.linalg.eigvalsh(elastic.compressibility_matrix(Ssym))
        assert abs(r["compressibility_min"]["value"][b] - ev[0]) <= 1e-13 * np.abs(ev).max()
        assert abs(r["compressibility_max"]["value"][b] - ev[2]) <= 1e-13 * np.abs(ev).max()
        n = r["compressibility_max"]["n"][b]
        assert n @ elastic.compressibility_matrix(Ssym) @ n == pytest.approx(ev[2], rel=1e-13)
    # an unbatched compliance gives the same without the leading dimension
    one = elastic.refine_extremes_host(S[0], D, M)
    assert one["poisson_min"]["value"] == r["poisson_min"]["value"][0] and one["young_max"]["n"].shape == (3,)
    # the iteration cap: status 1, the value between the grid's and the converged one
    capped = elastic.refine_extremes_host(S[:4], 16, 4, max_iter=1)
    full = elastic.refine_extremes_host(S[:4], 16, 4)
    for name in ("young_max", "shear_min", "poisson_max"):
        sign = sign_of(name)
        assert (capped[name]["iterations"] <= 1).all() and (capped[name]["status"] == 1).any()
        assert (sign * capped[name]["value"] >= sign * capped[name]["grid_value"]).all()
        assert (sign * full[name]["value"] >= sign * capped[name]["value"] - 1e-12 * np.abs(full[name]["value"])).all()


def test_argument_errors_are_raised_on_the_host():
    from matten_amd import elastic
    from matten_amd import predict as P

    C = np.stack([np.eye(6), 2 * np.eye(6), 3 * np.eye(6)])
    x = torch.zeros(3, 21)
    for call in (lambda **kw: elastic.elastic_properties(C, **kw), lambda **kw: elastic.elastic_properties_from_irreps(x, **kw)):
        with pytest.raises(ValueError, match="refine.*directions"):
            call(refine=True)
        for bad in (0.0, -1e-9, float("nan"), float("inf"), "tight", True):
            with pytest.raises(ValueError, match="refine_tol"):
                call(refine=True, directions=5, refine_tol=bad)
        for bad in (-1, 2.5, True, None):
            with pytest.raises(ValueError, match="refine_max_iter"):
                call(refine=True, directions=5, refine_max_iter=bad)
    s = {"lattice": 3.0 * np.eye(3), "cart_coords": np.zeros((1, 3)), "atomic_numbers": np.array([13])}
    with pytest.raises(ValueError, match="refine.*properties=True"):
        P.predict([dict(s)], model=object(), config=CFG, refine=True, directions=5)
    with pytest.raises(ValueError, match="refine.*directions"):      # (object(): no forward can run)
        P.predict([dict(s)], model=object(), config=CFG, properties=True, refine=True)
    with pytest.raises(ValueError, match="refine_tol"):
        P.predict([dict(s)], model=object(), config=CFG, properties=True, directions=5, refine=True, refine_tol=0.0)
    # the differentiable entries do not take it
    for fn in (elastic.elastic_moduli, elastic.elastic_moduli_from_irreps):
        assert "refine" not in inspect.signature(fn).parameters
    for fn in (elastic.elastic_properties, elastic.elastic_properties_from_irreps, P.predict):
        p = inspect.signature(fn).parameters
        assert p["refine"].default is False and p["refine_tol"].default == 1e-9 and p["refine_max_iter"].default == 32


def test_field_names_with_and_without_refine(monkeypatch):
    """the kernels replaced by host stand-ins of the right shapes: which fields exist, and in which order"""
    from matten_amd import elastic, ops

    calls = []

    def props(rows, layout):
        B = rows.shape[0]
        return torch.zeros(B, 6, 6, dtype=torch.float64), torch.zeros(B, 6, 6, dtype=torch.float64), \
            torch.zeros(B, 10, dtype=torch.float64), torch.zeros(B, dtype=torch.int32)

    def directional(compliance, flags, dirs, keep=False):
        B = flags.shape[0]
        return None, None, torch.zeros(B, 4, dtype=torch.float64), torch.zeros(B, 4, dtype=torch.int32)

    def pair(compliance, flags, dirs, cos_sin, keep=False):
        B = flags.shape[0]
        return None, torch.zeros(B, 4, dtype=torch.float64), torch.zeros(B, 4, dtype=torch.int32)

    def acoustic(voigt, flags, density, dirs, modulus_unit=1e9, keep=False):
        B = flags.shape[0]
        return None, torch.ones(B, 3, dtype=torch.float64), torch.zeros(B, 2, dtype=torch.int32), torch.zeros(B, dtype=torch.int32)

    def refine(compliance, flags, dirs, ext_dir, arg_dir, cos_sin=None, ext_pair=None, arg_pair=None, tol=1e-9, max_iter=32):
        calls.append((cos_sin is not None, tol, max_iter))
        Q, B = (8 if cos_sin is not None else 4), flags.shape[0]
        return (torch.zeros(Q, B, dtype=torch.float64), torch.zeros(Q, B, 3, dtype=torch.float64),
                torch.zeros(Q, B, 3, dtype=torch.float64), torch.zeros(Q, B, dtype=torch.int32),
                torch.zeros(Q, B, dtype=torch.int32))

    for name, fn in (("elastic_props", props), ("elastic_directional", directional), ("elastic_pair", pair),
                     ("elastic_acoustic", acoustic), ("elastic_refine", refine)):
        monkeypatch.setattr(ops, name, fn)
    monkeypatch.setattr(elastic, "_upload", lambda rows: rows)
    C = np.stack([np.eye(6)] * 3)
    rho, nd = [1000.0] * 3, [5e28] * 3

    assert list(elastic.elastic_properties(C)._names) == BASE_FIELDS
    assert list(elastic.elastic_properties(C, directions=5)._names) == BASE_FIELDS + DIR_FIELDS
    assert list(elastic.elastic_properties(C, directions=5, angles=3)._names) == BASE_FIELDS + DIR_FIELDS + PAIR_FIELDS
    everything = elastic.elastic_properties(C, directions=5, angles=3, density=rho, number_density=nd)
    assert list(everything._names) == BASE_FIELDS + DIR_FIELDS + PAIR_FIELDS + ACOUSTIC_FIELDS
    assert list(everything.to_dict()) == list(everything._names) and not calls            # refine=False: no launch, no new key

    def refined(names):
        return [n + s for n in names for s in (("_refined", "_refined_n", "_refined_m", "_refined_status", "_refined_iterations")
                                               if n.startswith(("shear", "poisson"))
                                               else ("_refined", "_refined_n", "_refined_status", "_refined_iterations"))]

    p = elastic.elastic_properties(C, directions=5, refine=True)
    assert list(p._names) == BASE_FIELDS + DIR_FIELDS + refined(elastic.REFINE_NAMES[:4])
    p = elastic.elastic_properties(C, directions=5, angles=3, density=rho, refine=True, refine_tol=1e-7, refine_max_iter=9)
    assert list(p._names) == BASE_FIELDS + DIR_FIELDS + PAIR_FIELDS + refined(elastic.REFINE_NAMES) + ACOUSTIC_FIELDS[:-1]
    assert calls == [(False, 1e-9, 32), (True, 1e-7, 9)]
    assert p.shear_max_refined.shape == (3,) and p.shear_max_refined_m.shape == (3, 3)
    assert p.young_min_refined_status.dtype == torch.int32 and p.young_min_refined_iterations.dtype == torch.int32
    assert not hasattr(p, "young_min_refined_m")
    one = elastic.elastic_properties(np.eye(6), directions=5, angles=3, refine=True)      # unbatched: no leading dimension
    assert one.poisson_min_refined.shape == () and one.poisson_min_refined_n.shape == (3,)
