"""
Polarisations, group velocities, power-flow angles and focusing Jacobians (matten_elastic_waves) on the GPU against
``acoustic_waves_host`` (numpy fp64, ``numpy.linalg.eigh`` per direction), which test_waves_host.py holds to finite
differences and closed forms.

Tolerances (derived, not measured; eps = 2^-52, FACTOR = 64): the module docstring of waves_cases.py derives them and
``waves_cases.bounds`` evaluates them per crystal, direction and branch.  In short: |d lam| <= FACTOR eps 9 max|C| (the
project's bound for Christoffel eigenvalues, Jacobi against LAPACK), |d u_k| <= 2 |d lam| / (gap_k lam_2), and v, g, |g|, psi,
the character and J carry those two through their formulas, J with the 1 / (lam_k - lam_m) of du once more.  No fixture
mode is excluded from the value checks: each item's tolerance carries its own gap.  What the tests add on top:
  polarisations   compared after the sign rule; where |u.n| < 1e-6 the rule's decision is itself within rounding of a tie,
                  so u is compared up to its sign there
  extremes        max_d / min_d of values that each moved by at most their bound: the device's winner must be a direction
                  whose host value is within (its bound + the host winner's bound) of the host's extreme, and the device's
                  extreme must be within that direction's bound of the host's value there; the extreme is bitwise the map's
                  entry at the device's index
  identities      g.n - v = (s / v) (u^T Gamma u - lam_k) + rounding, and a Rayleigh quotient is second order in du:
                  |u^T Gamma u - lam_k| <= 2 K du^2, so |g.n - v| <= (s / v) K (2 du^2 + FACTOR eps) + v rv;
                  U^T U - 1 and sum_k (u_k.n)^2 - 1: 15 rotations of a few eps each, 4 FACTOR eps
  rotation        both sides carry their own error and the rotated tensor is rounded once more (81 products per entry,
                  within the FACTOR eps max|C| that d lam already allows): 4 times the bound
"""
import os
import warnings

import numpy as np
import pytest
import torch

import waves_cases as wc
from common import LMAX2

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
UNIT = 1e9
VOIGT = np.array([[0, 5, 4], [5, 1, 3], [4, 3, 2]])
PAIRS = ((0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1))
MAPS = ("phase_velocity", "group_speed", "power_flow_angle", "longitudinal_character", "focusing_jacobian", "enhancement",
        "polarisation", "group_velocity")
ROW_FIELDS = ("power_flow_angle_max", "power_flow_angle_max_index", "focusing_min_jacobian", "focusing_min_jacobian_index",
              "n_degenerate", "n_unstable")


def _waves():
    from matten_amd import waves

    return waves


def cart(C):
    return C[..., VOIGT[:, :, None, None], VOIGT[None, None, :, :]]


def tensors_of(rows, dtype, layout):
    """the fixture rows as the input the case asks for, and the fp64 Voigt matrices that input holds"""
    C = wc.crystals()[list(rows)].astype(dtype)
    t = torch.from_numpy(cart(C) if layout == "cartesian" else C)
    return t, C.astype(np.float64)


_HOST = {}


def host_of(rows, dtype, D, rho):
    key = (tuple(rows), np.dtype(dtype).name, D, tuple(rho))
    if key not in _HOST:
        C = wc.crystals()[list(rows)].astype(dtype).astype(np.float64)
        out = _waves().acoustic_waves_host(C, np.asarray(rho), D, modulus_unit=UNIT, deg_tol=wc.DEG_TOL)
        for v in out.values():
            v.setflags(write=False)
        _HOST[key] = out
    return _HOST[key]


def same_nan(a, b, what):
    assert np.array_equal(np.isnan(a), np.isnan(b)), what


def check_against_host(dev, host, C, rho):
    """every field of the device result (to_dict()) against the host's, within waves_cases.bounds"""
    n = host["directions"]
    assert np.array_equal(dev["directions"], n)
    assert np.array_equal(dev["n_degenerate"], host["n_degenerate"]) and np.array_equal(dev["n_unstable"], host["n_unstable"])
    for name in MAPS:
        same_nan(dev[name], host[name], name)
    for b in range(len(C)):
        s = UNIT / rho[b]
        if host["n_unstable"][b] == -1:      # a NaN row: the masks above are the whole comparison of its maps
            for col in ("power_flow_angle_max", "focusing_min_jacobian"):
                assert np.isnan(dev[col][b]).all() and (dev[col + "_index"][b] == -1).all(), (col, b)
            continue
        with np.errstate(all="ignore"):      # (unstable directions: no bound, and nothing is compared there)
            t = wc.bounds(C[b], s, host, b)
        ok = ~np.isnan(host["focusing_jacobian"][b])                                  # [D,3]: the mode is defined

        def close(name, tol, what=None):
            err = np.abs(dev[name][b] - host[name][b])
            err = err.max(axis=-1) if err.ndim == 3 else err
            bad = ok & ~(err <= tol)
            assert not bad.any(), (what or name, wc.NAMES[b] if len(C) == 6 else b, float(np.nanmax(np.where(ok, err / tol, 0))))

        vok = ~np.isnan(host["phase_velocity"][b])
        assert (np.abs(dev["phase_velocity"][b] - host["phase_velocity"][b])[vok] <= t["v"][vok]).all()
        close("group_speed", t["g"])
        close("group_velocity", t["g"])
        close("power_flow_angle", t["psi"])
        close("longitudinal_character", t["character"])
        close("focusing_jacobian", t["J"])
        with np.errstate(divide="ignore"):
            assert np.array_equal(dev["enhancement"][b], 1.0 / np.abs(dev["focusing_jacobian"][b]), equal_nan=True)
        # polarisations: up to the sign where the sign rule decides on a value within rounding of zero
        ud, uh = dev["polarisation"][b], host["polarisation"][b]
        un = np.abs(np.einsum("dki,di->dk", uh, n))
        direct = np.linalg.norm(ud - uh, axis=2)
        either = np.minimum(direct, np.linalg.norm(ud + uh, axis=2))
        err = np.where(un < 1e-6, either, direct)
        assert not (ok & ~(err <= t["u"] + 4 * wc.EPS)).any(), ("polarisation", b, float(np.nanmax(np.where(ok, err / t["u"], 0))))
        # extremes
        for k in range(3):
            for q, name, col, tol, largest in ((k, "power_flow_angle", "power_flow_angle_max", t["psi"][:, k], True),
                                               (k, "focusing_jacobian", "focusing_min_jacobian", t["J"][:, k], False)):
                value, index = dev[col][b, k], int(dev[col + "_index"][b, k])
                h_index = int(host[col + "_index"][b, k])
                assert (index == -1) == (h_index == -1), (col, b, k)
                if h_index == -1:
                    assert np.isnan(value)
                    continue
                h_map = np.abs(host[name][b, :, k])
                assert abs(h_map[index] - h_map[h_index]) <= tol[index] + tol[h_index], (col, b, k, index, h_index)
                assert abs(value - h_map[index]) <= tol[index], (col, b, k)
                assert value == np.abs(dev[name][b, index, k]), (col, b, k)


CASES = [
    # rows of the fixture, directions, input dtype, layout, densities
    ((0,), 1, np.float64, "voigt", (1.0,)),
    ((1, 2, 5), 63, np.float32, "cartesian", (1.0, 8960.0, 19250.0)),
    ((0, 1, 2, 3, 4, 5), 64, np.float64, "cartesian", (1.0,) * 6),
    ((0, 1, 2, 3, 4, 5), 65, np.float32, "voigt", (1.0, 2.0, 8960.0, 2700.0, 4500.0, 19250.0)),
    ((0, 1, 2, 3, 4, 5), 200, np.float64, "voigt", (1.0,) * 6),
]


@pytest.mark.parametrize("rows,D,dtype,layout,rho", CASES, ids=["1x1", "3x63", "6x64", "6x65", "6x200"])
def test_device_against_host(rows, D, dtype, layout, rho):
    W = _waves()
    host = host_of(rows, dtype, D, rho)
    # the margin of the fixtures: nothing is flagged degenerate, nothing lies within a factor 3 of the threshold
    assert (host["n_degenerate"] == 0).all() and (host["n_unstable"] == 0).all()
    assert host["relative_gap"].min() >= 3 * wc.DEG_TOL
    t, C = tensors_of(rows, dtype, layout)
    out = W.acoustic_waves(t.to(DEV), np.asarray(rho), D, modulus_unit=UNIT, deg_tol=wc.DEG_TOL)
    assert out.group_velocity.is_cuda and out.group_velocity.shape == (len(rows), D, 3, 3)
    assert out.polarisation.shape == (len(rows), D, 3, 3) and out.focusing_jacobian.shape == (len(rows), D, 3)
    assert out.power_flow_angle_max.shape == (len(rows), 3) and out.n_degenerate.dtype == torch.int32
    dev = out.cpu().to_dict()
    assert not (dev["flags"] & 1).any()
    check_against_host(dev, host, C, rho)


def test_degenerate_modes_of_an_isotropic_tensor():
    """both transverse branches are degenerate in every direction: their phase velocity is kept, everything else of them is
    NaN, counted, and kept out of the extremes; the longitudinal branch has g = v n, psi = 0, character 1 and J = 1, within
    the bounds of waves_cases (``partners_degenerate``: its partners' eigenvectors are arbitrary, their projector is not)"""
    W = _waves()
    K, G, rho, D = 100.0, 40.0, 2.5, 65
    C = np.stack([wc.isotropic(K, G), wc.crystals()[2]])      # (a healthy anisotropic row beside it)
    out = W.acoustic_waves(torch.from_numpy(C).to(DEV), np.array([rho, rho]), D, modulus_unit=UNIT, deg_tol=wc.DEG_TOL)
    dev = out.to_dict()
    host = W.acoustic_waves_host(C, np.array([rho, rho]), D, modulus_unit=UNIT, deg_tol=wc.DEG_TOL)
    assert np.array_equal(host["n_degenerate"], [[D, D, 0], [0, 0, 0]])
    assert np.array_equal(dev["n_degenerate"], host["n_degenerate"]) and np.array_equal(dev["n_unstable"], [0, 0])
    for name in MAPS:
        same_nan(dev[name], host[name], name)
        if name != "phase_velocity":
            assert np.isnan(dev[name][0][:, :2]).all() and np.isfinite(dev[name][0][:, 2]).all(), name
    assert np.isfinite(dev["phase_velocity"]).all()
    for col in ("power_flow_angle_max", "focusing_min_jacobian"):
        assert np.isnan(dev[col][0, :2]).all() and (dev[col + "_index"][0, :2] == -1).all(), col
        assert np.isfinite(dev[col][0, 2]) and 0 <= dev[col + "_index"][0, 2] < D, col
    s, n = UNIT / rho, host["directions"]
    with np.errstate(all="ignore"):
        t = wc.bounds(C[0], s, host, 0, partners_degenerate=True)
    vt, vl = np.sqrt(G * s), np.sqrt((K + 4 * G / 3) * s)
    assert (np.abs(dev["phase_velocity"][0][:, :2] - vt) <= t["v"][:, :2] + 4 * wc.EPS * vt).all()
    assert (np.abs(dev["phase_velocity"][0][:, 2] - vl) <= t["v"][:, 2] + 4 * wc.EPS * vl).all()
    lo = dict(g=t["g"][:, 2], u=t["u"][:, 2], psi=t["psi"][:, 2], character=t["character"][:, 2], J=t["J"][:, 2])
    assert np.isfinite(lo["J"]).all() and lo["J"].max() < 1e-6      # (the bound says something)
    assert (np.linalg.norm(dev["group_velocity"][0][:, 2] - vl * n, axis=1) <= lo["g"] + 4 * wc.EPS * vl).all()
    assert (np.linalg.norm(dev["polarisation"][0][:, 2] - n, axis=1) <= lo["u"] + 4 * wc.EPS).all()
    assert (dev["power_flow_angle"][0][:, 2] <= lo["psi"]).all()
    assert (np.abs(dev["longitudinal_character"][0][:, 2] - 1) <= lo["character"] + 4 * wc.EPS).all()
    assert (np.abs(dev["focusing_jacobian"][0][:, 2] - 1) <= lo["J"]).all(), float(np.abs(dev["focusing_jacobian"][0][:, 2] - 1).max())
    k = int(dev["focusing_min_jacobian_index"][0, 2])
    assert dev["focusing_min_jacobian"][0, 2] == abs(dev["focusing_jacobian"][0, k, 2])
    k = int(dev["power_flow_angle_max_index"][0, 2])
    assert dev["power_flow_angle_max"][0, 2] == dev["power_flow_angle"][0, k, 2]
    # the anisotropic row beside it is held to the host like any other
    check_against_host({k_: (v if k_ == "directions" else v[1:]) for k_, v in dev.items()},
                       {k_: (v if k_ == "directions" else v[1:]) for k_, v in host.items()}, C[1:], [rho])


def test_identities_on_the_device_output():
    W = _waves()
    rows, D = (0, 1, 2, 3, 4, 5), 200
    host = host_of(rows, np.float64, D, (1.0,) * 6)
    t, C = tensors_of(rows, np.float64, "voigt")
    dev = W.acoustic_waves(t.to(DEV), np.ones(6), D, modulus_unit=UNIT, deg_tol=wc.DEG_TOL).to_dict()
    n = dev["directions"]
    fe = wc.FACTOR * wc.EPS
    for b in range(6):
        tb = wc.bounds(C[b], UNIT, host, b)
        v, g, u = dev["phase_velocity"][b], dev["group_velocity"][b], dev["polarisation"][b]
        K = 9 * np.abs(C[b]).max()
        tol = (UNIT / v) * K * (2 * tb["u"] ** 2 + fe) + tb["v"]
        gn = np.einsum("dki,di->dk", g, n)
        assert (np.abs(gn - v) <= tol).all(), (wc.NAMES[b], float((np.abs(gn - v) / tol).max()))
        assert (dev["group_speed"][b] >= v - tol).all()
        assert np.abs(dev["longitudinal_character"][b].sum(axis=1) - 1).max() <= 4 * fe
        gram = np.einsum("dki,dmi->dkm", u, u)
        assert np.abs(gram - np.eye(3)).max() <= 4 * fe
        assert (np.einsum("dki,di->dk", u, n) >= -1e-9).all()
        assert (dev["power_flow_angle"][b] >= 0).all() and (dev["longitudinal_character"][b] <= 1 + 4 * fe).all()


def test_rotation_covariance():
    W = _waves()
    rows, D = (0, 1, 2, 3, 4, 5), 33
    C = wc.crystals()
    rng = np.random.default_rng(7)
    R, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    R = R * np.sign(np.linalg.det(R))
    c4 = np.einsum("ai,bj,ck,dl,nijkl->nabcd", R, R, R, R, cart(C))
    C_rot = np.array([[[c[i, j, k, l] for (k, l) in PAIRS] for (i, j) in PAIRS] for c in c4])
    host = host_of(rows, np.float64, D, (1.0,) * 6)
    n = host["directions"]
    a = W.acoustic_waves(torch.from_numpy(C).to(DEV), np.ones(6), n, modulus_unit=UNIT, deg_tol=wc.DEG_TOL).to_dict()
    b = W.acoustic_waves(torch.from_numpy(C_rot).to(DEV), np.ones(6), n @ R.T, modulus_unit=UNIT, deg_tol=wc.DEG_TOL).to_dict()
    assert np.array_equal(a["n_degenerate"], b["n_degenerate"]) and (a["n_degenerate"] == 0).all()
    for x in range(6):
        t = wc.bounds(C[x], UNIT, host, x)
        for name, tol in (("phase_velocity", t["v"]), ("group_speed", t["g"]), ("power_flow_angle", t["psi"]),
                          ("longitudinal_character", t["character"]), ("focusing_jacobian", t["J"])):
            err = np.abs(a[name][x] - b[name][x])
            assert (err <= 4 * tol).all(), (name, wc.NAMES[x], float((err / tol).max()))
        err = np.linalg.norm(a["group_velocity"][x] @ R.T - b["group_velocity"][x], axis=2)
        assert (err <= 4 * t["g"]).all(), ("group_velocity", wc.NAMES[x], float((err / t["g"]).max()))
        ua, ub = a["polarisation"][x] @ R.T, b["polarisation"][x]
        direct = np.linalg.norm(ua - ub, axis=2)
        either = np.minimum(direct, np.linalg.norm(ua + ub, axis=2))
        un = np.abs(np.einsum("dki,di->dk", a["polarisation"][x], n))
        err = np.where(un < 1e-6, either, direct)
        assert (err <= 4 * t["u"] + 16 * wc.EPS).all(), ("polarisation", wc.NAMES[x], float((err / t["u"]).max()))


def test_bad_rows_and_unstable_directions_do_not_poison_their_neighbours():
    W = _waves()
    fix = wc.crystals()
    D = 65
    nan_row = fix[3].copy()
    nan_row[1, 4] = nan_row[4, 1] = np.nan
    C = np.stack([fix[2], np.zeros((6, 6)), fix[0], nan_row, wc.cubic(100.0, 50.0, -20.0), fix[4], fix[5]])
    rho = np.array([8960.0, 1.0, 1.0, 2700.0, 1.0, -4500.0, 19250.0])
    healthy = [0, 2, 6]
    out = W.acoustic_waves(torch.from_numpy(C).to(DEV), torch.from_numpy(rho).to(DEV), D, modulus_unit=UNIT, deg_tol=wc.DEG_TOL)
    dev = out.to_dict()
    assert (dev["flags"][[1, 3]] & 1).all() and not (dev["flags"][[0, 2, 4, 5, 6]] & 1).any()
    host = W.acoustic_waves_host(C, rho, D, modulus_unit=UNIT, deg_tol=wc.DEG_TOL, flags=dev["flags"])
    for b in (1, 3, 5):      # singular, non-finite, negative density
        for name in MAPS + ("power_flow_angle_max", "focusing_min_jacobian"):
            assert np.isnan(dev[name][b]).all(), (name, b)
        for name in ("power_flow_angle_max_index", "focusing_min_jacobian_index", "n_degenerate", "n_unstable"):
            assert (dev[name][b] == -1).all(), (name, b)
    # the indefinite row: some directions are unstable, counted, NaN; the others are held to the host like any row
    assert 0 < host["n_unstable"][4] < D and dev["n_unstable"][4] == host["n_unstable"][4]
    gone = np.isnan(host["phase_velocity"][4]).all(axis=1)
    assert gone.sum() == host["n_unstable"][4]
    for name in MAPS:
        assert np.isnan(dev[name][4][gone]).all(), name
    check_against_host(dev, host, C, rho)
    # the healthy rows are bitwise what they are on their own
    alone = W.acoustic_waves(torch.from_numpy(C[healthy]).to(DEV), rho[healthy], D, modulus_unit=UNIT, deg_tol=wc.DEG_TOL).to_dict()
    for name in MAPS + ROW_FIELDS:
        assert np.array_equal(dev[name][healthy], alone[name], equal_nan=True), name
    assert (alone["n_unstable"] == 0).all() and np.isfinite(alone["group_velocity"]).all()


def test_two_calls_and_the_extremes_alone_give_the_same_bits():
    W = _waves()
    t, _ = tensors_of((0, 1, 2, 3, 4, 5), np.float64, "voigt")
    t = t.to(DEV)
    first = W.acoustic_waves(t, np.ones(6), 200, modulus_unit=UNIT).to_dict()
    second = W.acoustic_waves(t, np.ones(6), 200, modulus_unit=UNIT).to_dict()
    for name in MAPS + ROW_FIELDS:
        assert np.array_equal(first[name], second[name], equal_nan=True), name
    lean = W.acoustic_waves(t, np.ones(6), 200, modulus_unit=UNIT, keep_directional=False)
    for name in MAPS:
        assert getattr(lean, name) is None, name
    lean = lean.to_dict()
    for name in ROW_FIELDS:
        assert np.array_equal(first[name], lean[name], equal_nan=True), name


def test_the_entry_captures_into_a_graph():
    from matten_amd import ops

    fix = torch.from_numpy(wc.crystals()).to(DEV)
    voigt = fix.clone()
    flags = torch.zeros(6, dtype=torch.int32, device=DEV)
    rho = torch.ones(6, dtype=torch.float64, device=DEV)
    from matten_amd.elastic import fibonacci_hemisphere

    dirs = torch.from_numpy(fibonacci_hemisphere(65)).to(DEV)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.elastic_waves(voigt, flags, rho, dirs, UNIT, wc.DEG_TOL)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = ops.elastic_waves(voigt, flags, rho, dirs, UNIT, wc.DEG_TOL)
    for scale in (1.0, 0.5):
        voigt.copy_(fix * scale)
        graph.replay()
        torch.cuda.synchronize()
        eager = ops.elastic_waves(voigt, flags, rho, dirs, UNIT, wc.DEG_TOL)
        for a, b in zip(captured, eager):
            assert torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a,
                               b.view(torch.int64) if b.dtype == torch.float64 else b)
        assert torch.isfinite(captured[1]).all()


def test_predict_with_waves(golden_dir):
    from matten_amd import predict as P
    from matten_amd.model_factory.tfn_scalar_tensor import ScalarTensorModel
    from oracle.matten_ref import data as rdata

    W = _waves()
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
    kw = dict(model=model, config=cfg, properties=True, density=rho, directions=65)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        tensors0, props0 = P.predict(structs, **kw)
        tensors, props, waves = P.predict(structs, waves=True, **kw)
    assert isinstance(waves, W.AcousticWaves)
    assert len(tensors) == len(tensors0) == 5 and tensors[2] is None and tensors0[2] is None
    for i in (0, 1, 3, 4):
        assert type(tensors[i]) is type(tensors0[i]) and np.array_equal(np.asarray(tensors[i]), np.asarray(tensors0[i]))
    a, b = props0.to_dict(), props.to_dict()
    assert list(a) == list(b)
    for k in a:
        assert (a[k] is None and b[k] is None) or np.array_equal(a[k], b[k], equal_nan=True), k
    w = waves.to_dict()
    assert w["group_velocity"].shape == (5, 65, 3, 3) and np.array_equal(w["flags"], a["flags"])
    assert np.isnan(w["group_velocity"][2]).all() and (w["n_unstable"][2] == -1) and (w["n_degenerate"][2] == -1).all()
    # the phase velocities are those of the acoustic kernel, to the eigenvalue bound (both within it of the truth)
    from matten_amd.elastic import elastic_properties

    kept = elastic_properties([None if t is None else np.asarray(t) for t in tensors0], density=rho, directions=65,
                              keep_directional=True).to_dict()
    assert np.array_equal(kept["v_fast_max"], a["v_fast_max"], equal_nan=True)
    same_nan(w["phase_velocity"], kept["velocities"], "phase_velocity")
    for i in (0, 1, 3, 4):
        v = kept["velocities"][i]
        dl = wc.FACTOR * wc.EPS * 9 * np.abs(a["voigt"][i]).max()
        lam = v * v * rho[i] / UNIT
        tol = v * (2 * dl / (2 * lam) + 4 * wc.EPS)
        ok = ~np.isnan(v)
        assert (np.abs(w["phase_velocity"][i] - v)[ok] <= tol[ok]).all(), i
        assert w["n_unstable"][i] == a["acoustic_unstable_directions"][i]
        stable = ~np.isnan(w["phase_velocity"][i]).any(axis=1)
        defined = ~np.isnan(w["focusing_jacobian"][i])
        assert np.isfinite(w["group_velocity"][i][defined]).all()
        assert defined[stable].sum() == 3 * stable.sum() - w["n_degenerate"][i].sum()
