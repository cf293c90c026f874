"""
CPU tests of the per-atom shielding parameters (matten_amd/rank2.py): the numpy restatement ``rank2_host`` against closed
forms, its adjoint ``rank2_bwd_host`` against central differences, the library's two entries (exported, ABI 47, bad
arguments refused without a device), the argument checks of ``Rank2Loss`` / ``rank2_selected_loss`` / ``predict`` and the
flattened irreps basis.  The GPU tests (tests/test_gpu_rank2.py) hold the kernels to the restatement tested here and
share this file's generators.
"""
import json
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "si_nmr_n12.json")
GAP = 0.05      # the condition of the gradient checks: min(l2 - l1, l3 - l2) / span and |skew| at least this


def fixture_tensors() -> np.ndarray:
    """the 20 labelled Si shielding tensors of the fixture, [20,3,3] fp64 (not symmetric)"""
    with open(FIXTURE) as f:
        data = json.load(f)
    column = data["nmr_tensor"]      # structure index -> the tensors of its selected atoms
    T = np.concatenate([np.asarray(column[k], dtype=np.float64).reshape(-1, 3, 3) for k in sorted(column, key=int)])
    assert T.shape == (20, 3, 3)
    return T


def random_tensors(n: int, scale: float, seed: int) -> np.ndarray:
    """n general (not symmetric) tensors: an isotropic part in +-500 plus entries of size `scale`"""
    rng = np.random.default_rng(seed)
    return rng.uniform(-500.0, 500.0, n)[:, None, None] * np.eye(3) + scale * rng.standard_normal((n, 3, 3))


def gap_ok(T) -> np.ndarray:
    """rows whose eigenvalues and Haeberlen branch are well separated: the condition of the gradient checks"""
    from matten_amd.rank2 import rank2_host

    h = rank2_host(T)
    lam, span = h["principal_values"], h["span"]
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.minimum(lam[:, 1] - lam[:, 0], lam[:, 2] - lam[:, 1]) / span
        return (h["flags"] == 0) & (rel >= GAP) & (np.abs(h["skew"]) >= GAP)


def functional(T, c_vals, c_props) -> np.ndarray:
    """sum_k c_vals[k] l_k + sum_q c_props[q] props_q per row: the scalar whose gradient rank2_bwd_host(T, c_vals, c_props) is"""
    from matten_amd.rank2 import RANK2_NAMES, rank2_host

    h = rank2_host(T)
    return (h["principal_values"] * c_vals).sum(1) + sum(c_props[:, q] * h[name] for q, name in enumerate(RANK2_NAMES))


def central_differences(T, c_vals, c_props, step) -> np.ndarray:
    """d functional / d T [n,3,3] by central differences with one step per row, step [n]"""
    g = np.zeros_like(T)
    for i in range(3):
        for j in range(3):
            d = np.zeros_like(T)
            d[:, i, j] = step
            g[:, i, j] = (functional(T + d, c_vals, c_props) - functional(T - d, c_vals, c_props)) / (2.0 * step)
    return g


# ----------------------------------------------------------------------------------------------------------------------
# rank2_host against closed forms
# ----------------------------------------------------------------------------------------------------------------------
def test_diagonal_tensor():
    from matten_amd.rank2 import rank2_host

    h = rank2_host(np.diag([4.0, 1.0, 2.0]))
    assert np.array_equal(h["principal_values"], [[1.0, 2.0, 4.0]])
    iso = 7.0 / 3.0
    assert h["iso"][0] == iso and h["span"][0] == 3.0 and h["flags"][0] == 0 and not h["is_isotropic"][0]
    assert abs(h["skew"][0] - 3.0 * (2.0 - iso) / 3.0) < 1e-15 and h["skew"][0] < 0      # -1/3: z is l3
    assert abs(h["zeta"][0] - (4.0 - iso)) < 1e-15 and abs(h["anisotropy"][0] - 1.5 * (4.0 - iso)) < 1e-15
    assert abs(h["eta"][0] - (2.0 - 1.0) / (4.0 - iso)) < 1e-15 and 0.0 <= h["eta"][0] <= 1.0
    U = h["principal_axes"][0]                                                         # columns: e_y, e_z, e_x up to sign
    assert np.array_equal(np.abs(U), np.array([[0, 0, 1.0], [1.0, 0, 0], [0, 1.0, 0]]))
    # z on the low side: the mirror image
    m = rank2_host(-np.diag([4.0, 1.0, 2.0]))
    assert np.array_equal(m["principal_values"], [[-4.0, -2.0, -1.0]]) and m["skew"][0] > 0
    assert abs(m["zeta"][0] + h["zeta"][0]) < 1e-15 and abs(m["eta"][0] - h["eta"][0]) < 1e-15


def test_axially_symmetric_tensor():
    from matten_amd.rank2 import rank2_host

    h = rank2_host(np.stack([np.diag([1.0, 1.0, 5.0]), np.diag([5.0, 5.0, 1.0])]))
    assert np.allclose(h["skew"], [-1.0, 1.0], atol=1e-15) and np.allclose(h["eta"], 0.0, atol=1e-15)
    assert np.allclose(h["zeta"], [5.0 - 7.0 / 3.0, 1.0 - 11.0 / 3.0], atol=1e-15) and np.array_equal(h["span"], [4.0, 4.0])
    assert (h["flags"] == 0).all()


def test_multiple_of_the_identity_and_bad_rows():
    from matten_amd.rank2 import FLAG_ISOTROPIC, FLAG_NOT_FINITE, rank2_host

    bad = np.eye(3)
    bad[0, 2] = np.nan
    inf = np.eye(3)
    inf[1, 1] = np.inf
    h = rank2_host(np.stack([-37.5 * np.eye(3), bad, np.diag([1.0, 2.0, 3.0]), inf]))
    assert h["flags"].tolist() == [FLAG_ISOTROPIC, FLAG_NOT_FINITE, 0, FLAG_NOT_FINITE] and h["flags"].dtype == np.int32
    assert h["is_isotropic"].tolist() == [True, False, False, False]
    assert h["skew"][0] == 0.0 and h["eta"][0] == 0.0 and h["span"][0] == 0.0 and h["iso"][0] == -37.5
    for k in ("principal_values", "principal_axes", "iso", "span", "skew", "zeta", "anisotropy", "eta"):
        assert np.isnan(h[k][1]).all() and np.isnan(h[k][3]).all() and np.isfinite(h[k][2]).all(), k


def test_rotated_tensor_and_symmetrisation():
    from matten_amd.rank2 import rank2_host

    rng = np.random.default_rng(5)
    R, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    lam = np.array([-3.0, 0.5, 11.0])
    A = R @ np.diag(lam) @ R.T
    h = rank2_host(A)
    assert np.allclose(h["principal_values"][0], lam, atol=1e-13)
    U = h["principal_axes"][0]
    assert np.allclose(np.abs(U.T @ R), np.eye(3), atol=1e-13)
    # the antisymmetric part does not enter
    K = rng.standard_normal((3, 3))
    g = rank2_host(A + 7.0 * (K - K.T))
    for k in ("principal_values", "iso", "span", "skew", "zeta", "eta"):
        assert np.allclose(g[k], h[k], atol=1e-12), k
    # list, torch and unbatched inputs
    assert np.array_equal(rank2_host([A, A])["iso"], np.repeat(h["iso"], 2))
    assert np.array_equal(rank2_host(torch.from_numpy(A))["iso"], h["iso"])
    with pytest.raises(ValueError, match=r"\[N,3,3\]"):
        rank2_host(np.zeros((2, 3)))


def test_fixture_tensors_are_general_and_well_separated():
    T = fixture_tensors()
    anti = np.abs(T - T.transpose(0, 2, 1)).max()
    assert 20.0 < anti < 30.0          # T_ij and T_ji differ by up to 25 ppm: the symmetrisation matters
    from matten_amd.rank2 import rank2_host

    h = rank2_host(T)
    assert (h["flags"] == 0).all() and (np.abs(h["skew"]) >= 1e-6).all()
    assert ((h["eta"] >= 0) & (h["eta"] <= 1)).all() and (np.abs(h["zeta"]) >= h["span"] / 2 - 1e-12).all()


# ----------------------------------------------------------------------------------------------------------------------
# rank2_bwd_host against central differences
# ----------------------------------------------------------------------------------------------------------------------
def test_adjoint_against_central_differences():
    """Random general tensors at entry scales 1e-2, 1 and 30 around isotropic parts in +-500, kept where the relative gaps
    and |skew| are >= 0.05 (the generator keeps >= 80 %), a random linear functional of the three values and five scalars.
    The central difference is taken with a step of 1e-4 of the row's span and again with twice that step; the two differ
    by the finite-difference noise (truncation (h / gap)^2 and the rounding of +-500 over h): measured here 1.4e-6 of the
    row's max|g_T| at worst, and the analytic gradient lies within 4.7e-7 of the finer one.  The bound is 1e-5 of max|g_T|
    per row, seven times the measured noise; and, so that the bound cannot outlive the noise it came from, the noise is
    asserted to be below it too."""
    from matten_amd.rank2 import rank2_bwd_host, rank2_host

    T = np.concatenate([random_tensors(400, s, seed) for seed, s in enumerate((1e-2, 1.0, 30.0))])
    keep = gap_ok(T)
    print(f"kept {keep.mean():.3f} of {len(T)} draws")
    assert keep.mean() >= 0.8
    T = T[keep]
    rng = np.random.default_rng(11)
    c_vals, c_props = rng.standard_normal((len(T), 3)), rng.standard_normal((len(T), 5))
    got = rank2_bwd_host(T, c_vals, c_props)
    assert np.array_equal(got, got.transpose(0, 2, 1))
    step = 1e-4 * rank2_host(T)["span"]
    fine, coarse = central_differences(T, c_vals, c_props, step), central_differences(T, c_vals, c_props, 2.0 * step)
    # (the functional sees the symmetrised tensor, so its derivative with respect to T is already symmetric)
    scale = np.abs(got).max(axis=(1, 2))
    noise = (np.abs(fine - coarse).max(axis=(1, 2)) / scale).max()
    err = (np.abs(got - fine).max(axis=(1, 2)) / scale).max()
    print(f"finite-difference noise {noise:.2e}, analytic against the finer difference {err:.2e} (of max|g_T| per row)")
    assert noise <= 1e-5 and err <= 1e-5
    # each part alone, and None = zero
    zero3, zero5 = np.zeros_like(c_vals), np.zeros_like(c_props)
    assert np.array_equal(rank2_bwd_host(T, c_vals, None), rank2_bwd_host(T, c_vals, zero5))
    assert np.array_equal(rank2_bwd_host(T, None, c_props), rank2_bwd_host(T, zero3, c_props))
    assert np.allclose(rank2_bwd_host(T, c_vals, None) + rank2_bwd_host(T, None, c_props), got, rtol=0, atol=1e-12 * scale.max())
    # the isotropic value's gradient is the identity over three, whatever the basis
    only_iso = np.zeros((len(T), 5))
    only_iso[:, 0] = 1.0
    assert np.allclose(rank2_bwd_host(T, None, only_iso), np.eye(3) / 3.0, atol=1e-15)


def test_adjoint_of_excluded_rows():
    from matten_amd.rank2 import rank2_bwd_host

    bad = np.eye(3)
    bad[2, 0] = np.nan
    T = np.stack([np.diag([1.0, 2.0, 4.0]), bad, 3.0 * np.eye(3)])
    g_vals, g_props = np.full((3, 3), np.nan), np.full((3, 5), np.nan)
    g_vals[0], g_props[0] = 1.0, 1.0
    g_vals[2], g_props[2] = [1.0, 2.0, 3.0], [3.0, 0.5, np.nan, 0.25, np.nan]      # skew / eta upstream ignored on c I
    g = rank2_bwd_host(T, g_vals, g_props)
    assert np.isfinite(g).all() and (g[1] == 0).all() and not np.signbit(g[1]).any()
    again = g_props.copy()
    again[2, 2], again[2, 4] = 7.0, -9.0
    assert np.array_equal(rank2_bwd_host(T, g_vals, again)[2], g[2])
    assert abs(np.trace(g[2]) - (6.0 + 3.0)) < 1e-14                     # sum of w: the values' 6, iso's 3, span and zeta 0


# ----------------------------------------------------------------------------------------------------------------------
# the library
# ----------------------------------------------------------------------------------------------------------------------
def test_library_declares_binds_and_exports_the_rank2_entries():
    from matten_amd import _lib

    header = open(os.path.join(ROOT, "include", "matten_hip.h")).read()
    declared = set(re.findall(r"\b(matten_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for name in ("matten_rank2_props", "matten_rank2_props_bwd"):
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert _lib.ABI_VERSION == 47 and lib.matten_abi_version() == 47          # entries were only added
    assert len(_lib.SIGNATURES["matten_rank2_props"][1]) == 8 and len(_lib.SIGNATURES["matten_rank2_props_bwd"][1]) == 10
    mk = open(os.path.join(ROOT, "matten_amd", "csrc", "Makefile")).read()
    assert "rank2.hip" in mk and "sym3.h" in mk
    # one copy of the rotation
    csrc = os.path.join(ROOT, "matten_amd", "csrc")
    for f in ("elastic.hip", "rank2.hip"):
        src = open(os.path.join(csrc, f)).read()
        assert '#include "sym3.h"' in src and "void jacobi_rotate" not in src, f
    assert "void jacobi_rotate" in open(os.path.join(csrc, "sym3.h")).read()


def test_bad_arguments_come_back_without_a_device():
    from matten_amd import _lib

    lib = _lib.load()
    fwd, bwd = lib.matten_rank2_props, lib.matten_rank2_props_bwd
    p = 4096      # never dereferenced: every call below returns from the checks
    assert fwd(None, 1, 0, None, None, None, None, None) == 0 and bwd(None, None, None, None, None, None, 0, 0, None, None) == 0
    assert fwd(p, 1, -1, p, p, p, p, None) == -1 and bwd(p, p, p, p, p, p, 1, -1, p, None) == -1
    assert fwd(p, 2, 5, p, p, p, p, None) == -1 and bwd(p, p, p, p, p, p, -1, 5, p, None) == -1
    good = [p, 1, 5, p, p, p, p, None]
    for k in (0, 3, 5, 6):                      # t, vals, props, flags (axes may be NULL)
        args = list(good)
        args[k] = None
        assert fwd(*args) == -1, k
    good = [p, p, p, p, p, p, 0, 5, p, None]
    for k in (0, 1, 2, 3, 8):                   # vals, axes, props, flags, g_t (g_vals / g_props may be NULL)
        args = list(good)
        args[k] = None
        assert bwd(*args) == -1, k


# ----------------------------------------------------------------------------------------------------------------------
# argument checks of the host layers
# ----------------------------------------------------------------------------------------------------------------------
def test_rank2_loss_validates_like_moduli_loss():
    from matten_amd.graphs import rank2_selected_loss
    from matten_amd.rank2 import RANK2_NAMES, Rank2Loss

    assert RANK2_NAMES == ("iso", "span", "skew", "zeta", "eta")
    loss = Rank2Loss(("iso", "span"), weights=[1.0, 4.0], kind="mse")
    assert loss.names == ("iso", "span") and loss.weights == {"iso": 1.0, "span": 4.0} and loss._scales["span"] == 2.0
    assert Rank2Loss("iso").names == ("iso",) and Rank2Loss(kind="l1", weights={"iso": 3.0})._scales == {"iso": 3.0}
    for bad in (dict(names=()), dict(names=("iso", "k_vrh")), dict(names=("iso", "iso")), dict(kind="mae"),
                dict(names=("iso",), weights=[1.0, 2.0]), dict(names=("iso",), weights={"span": 1.0}),
                dict(names=("iso",), weights=[-1.0]), dict(names=("iso",), weights=[float("nan")])):
        with pytest.raises(ValueError):
            Rank2Loss(**bad)
    with pytest.raises(ValueError, match="not in"):
        rank2_selected_loss(("sigma",), "mse")
    with pytest.raises(ValueError, match="kind"):
        rank2_selected_loss(("iso",), "huber")
    with pytest.raises(ValueError, match="symmetric rank-2"):
        rank2_selected_loss(("iso",), "mse", formula="ijkl=jikl=klij")
    fn = rank2_selected_loss(("iso",), "mse", key="nmr_tensor")
    assert fn.wants_batch
    with pytest.raises(ValueError, match="atom_selector"):
        fn({"nmr_tensor": torch.zeros(4, 6)}, torch.zeros(4, 1), {})


def test_host_tensors_are_not_differentiated():
    from matten_amd.rank2 import rank2_invariants, rank2_invariants_from_irreps, rank2_properties_from_irreps

    with pytest.raises(ValueError, match="rank2_properties"):
        rank2_invariants(torch.zeros(4, 3, 3))
    with pytest.raises(ValueError, match="rank2_properties"):
        rank2_invariants(np.zeros((4, 3, 3)))
    with pytest.raises(ValueError, match="rank2_properties_from_irreps"):
        rank2_invariants_from_irreps(torch.zeros(4, 6))
    with pytest.raises(ValueError, match="6 irreps components"):
        rank2_invariants_from_irreps(torch.zeros(4, 9))
    for formula in ("ijkl=jikl=klij", "ij=-ji", "ij"):
        with pytest.raises(ValueError, match="symmetric rank-2"):
            rank2_properties_from_irreps(torch.zeros(4, 6), formula=formula)


def test_predict_checks_shielding_before_any_forward():
    from matten_amd import predict as P

    cfg = {"data": {"r_cut": 5.0, "tensor_target_formula": "ij=ji", "tensor_target_name": "nmr_tensor"}}
    with pytest.raises(ValueError, match="is_atomic_tensor=True"):
        P.predict([], model=object(), config=cfg, shielding=True)
    with pytest.raises(ValueError, match="is_atomic_tensor=True"):
        P.predict([], model=object(), config=cfg, is_atomic_tensor=False, is_elasticity_tensor=False, shielding=True)
    wrong = {"data": dict(cfg["data"], tensor_target_formula="ijkl=jikl=klij")}
    with pytest.raises(ValueError, match="symmetric rank-2"):
        P.predict([], model=object(), config=wrong, is_atomic_tensor=True, shielding=True)
    # the refusal of properties=True for per-atom tensors stands, with or without the new keyword
    with pytest.raises(ValueError, match="is_atomic_tensor"):
        P.predict([], model=object(), config=cfg, is_atomic_tensor=True, properties=True, shielding=True)
    import inspect

    params = list(inspect.signature(P.predict).parameters)
    assert params[-1] == "shielding" and inspect.signature(P.predict).parameters["shielding"].default is False
    assert inspect.signature(P.evaluate_atomic).parameters["sink"].default is None


# ----------------------------------------------------------------------------------------------------------------------
# the irreps basis
# ----------------------------------------------------------------------------------------------------------------------
def test_flattened_basis_is_to_cartesian():
    from matten_amd import o3
    from matten_amd.rank2 import rank2_basis

    B = rank2_basis("ij=ji")
    assert B.shape == (6, 9) and B.dtype == np.float64 and not B.flags.writeable
    _, Q = o3.cartesian_tensor_basis("ij=ji")
    x = np.random.default_rng(2).standard_normal((17, 6))
    cart = np.einsum("qij,bq->bij", Q, x)                      # CartesianTensor.to_cartesian (o3.cartesian_tensor_basis)
    assert np.array_equal((x @ B).reshape(17, 3, 3), cart) or np.allclose((x @ B).reshape(17, 3, 3), cart, rtol=0, atol=1e-15)
    assert np.allclose(cart, cart.transpose(0, 2, 1), atol=1e-15)
    # orthonormal rows: from_cartesian is the transpose
    assert np.allclose(B @ B.T, np.eye(6), atol=1e-12)
    import matten.rank2 as alias
    import matten_amd.rank2 as real

    assert alias is real
