"""
CPU tests of the gradients through the directional and acoustic elastic properties (matten_elastic_directional_bwd,
matten_elastic_acoustic_bwd; elastic_moduli(..., directions=, density=, number_density=); ModuliLoss on the directional
names): declarations and bindings, argument validation, the loss's exclusion of non-finite values, and the two statements of
the forwards that tests/test_gpu_elastic_dir_grad.py leans on.  No kernel is launched.

Two statements, neither shares code with matten_amd.elastic:
  * the REFERENCE, torch fp64, differentiable: E = 1 / (v^T S v), beta = r . v from the symmetrised compliance;
    Gamma_ik = C_ijkl n_j n_l from the symmetrised Voigt matrix, torch.linalg.eigvalsh (LAPACK), v_k = sqrt(lambda_k s).
    Its autograd is tied to central finite differences here (torch.autograd.gradcheck).
  * the ARBITER, numpy longdouble, the adjoint formulas written out: cyclic Jacobi with eigenvectors run to convergence,
    Hc = sum_d sum_k w_k a_k a_k^T with a_k[V(i,j)] = sum over the pair's orderings of u_k,i n_j (the contraction
    Gbar_ik n_j n_l collapses to that rank-one form: another arrangement than the kernel's).  It also returns the
    ABSOLUTE-SUM gradient: the same accumulation with every per-direction (and per-mode) contribution replaced by its
    magnitude, the scale in which errors are counted (cancellation between directions does not shrink it).  A mode's share
    is weighted by 1 + lambda_max / gap (gap = the distance to the nearest other eigenvalue) for the per-mode upstream
    gradients (velocity map, slow / fast extremes: an eigenvector moves by eps lambda_max / gap) and by
    1 + lambda_max / lambda_min for the sum of v^-3 (a function of the whole matrix: no gap enters).
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from test_elastic_grad_host import fake_props

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52
V_OF = ((0, 5, 4), (5, 1, 3), (4, 3, 2))          # Cartesian pair -> Voigt index
UNIT = 1e9                                         # Pa per unit of the tensors (GPa)
NEW_NAMES = ("young_min", "young_max", "compressibility_min", "compressibility_max", "v_slow_min", "v_fast_max", "v_mean",
             "debye_temperature")
SUM_SCALE = 1e14      # lifts the gradient of sum v^-3 (v ~ 5e3 m/s: 3 v^-4 dv/dC ~ 1e-14) to the size of the others


# ---------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------
def generic_tensors(seed):
    """six Voigt matrices [6,6,6] fp64: C = 30 (A A^T + 6 I), A standard normal, plus 0.01-scale unsymmetric noise"""
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((6, 6, 6))
    C = 30.0 * (A @ A.transpose(0, 2, 1) + 6.0 * np.eye(6))
    return C + 0.01 * rng.standard_normal((6, 6, 6))


def densities(B):
    """kg/m^3, different per row"""
    return 2500.0 + 730.0 * np.arange(B, dtype=np.float64)


def cubic(c11, c12, c44):
    C = np.zeros((6, 6))
    C[:3, :3] = c12
    for i in range(3):
        C[i, i], C[3 + i, 3 + i] = c11, c44
    return C


def v_of(n):
    """directions [D,3] -> v(n) [D,6] = (n1^2, n2^2, n3^2, n2 n3, n1 n3, n1 n2); numpy or torch"""
    n1, n2, n3 = n[:, 0], n[:, 1], n[:, 2]
    stack = torch.stack if isinstance(n, torch.Tensor) else np.stack
    return stack([n1 * n1, n2 * n2, n3 * n3, n2 * n3, n1 * n3, n1 * n2], 1)


# ---------------------------------------------------------------------------------------------------
# the reference: torch fp64, differentiable
# ---------------------------------------------------------------------------------------------------
def ref_directional(s, dirs):
    """compliance s [B,6,6] (as stored: not trusted to be symmetric), dirs [D,3] -> (E [B,D], beta [B,D])"""
    S = 0.5 * (s + s.transpose(1, 2))
    v = v_of(dirs)
    q = torch.einsum("di,bij,dj->bd", v, S, v)
    return 1.0 / q, torch.einsum("bi,di->bd", S[:, :, :3].sum(dim=2), v)


def ref_christoffel(c, dirs):
    """Voigt c [B,6,6], dirs [D,3] -> Gamma [B,D,3,3]"""
    C = 0.5 * (c + c.transpose(1, 2))
    idx = torch.tensor(V_OF)
    C4 = C[:, idx[:, :, None, None], idx[None, None, :, :]]            # [B,3,3,3,3] = C_ijkl
    return torch.einsum("bijkl,dj,dl->bdik", C4, dirs, dirs)


def ref_acoustic(c, rho, dirs, unit=UNIT):
    """-> (vel [B,D,3] ascending, NaN where a direction has a non-positive eigenvalue; ok [B,D]; lam [B,D,3])"""
    lam = torch.linalg.eigvalsh(ref_christoffel(c, dirs))
    ok = (lam > 0).all(dim=2)
    safe = torch.where(ok[:, :, None], lam, torch.ones_like(lam))
    vel = torch.sqrt(safe * (unit / rho)[:, None, None])
    return torch.where(ok[:, :, None], vel, torch.full_like(vel, float("nan"))), ok, lam


def _pick(values, index):
    """values [B,D], index [B] (-1: none) -> the entries [B], 0 where there is none"""
    got = values.gather(1, index.clamp(min=0).long()[:, None])[:, 0]
    return torch.where(index >= 0, got, torch.zeros_like(got))


def ref_directional_grad(s, dirs, g_young, g_beta, g_ext, arg):
    """autograd of sum(g . outputs) -> the gradient of s [B,6,6]; the extremes are the values at the recorded directions"""
    s = s.clone().requires_grad_()
    E, beta = ref_directional(s, dirs)
    f = (E * 0).sum()
    if g_young is not None:
        f = f + (E * g_young).sum()
    if g_beta is not None:
        f = f + (beta * g_beta).sum()
    if g_ext is not None:
        for q, m in enumerate((E, E, beta, beta)):
            f = f + (_pick(m, arg[:, q]) * g_ext[:, q]).sum()
    f.backward()
    return s.grad


def ref_acoustic_grad(c, rho, dirs, g_vel, g_ext, arg, unit=UNIT):
    """the same for the acoustic outputs; directions with a non-positive eigenvalue are masked out (torch.where)"""
    c = c.clone().requires_grad_()
    vel, ok, _ = ref_acoustic(c, rho, dirs, unit)
    zero = torch.zeros_like(vel)
    vel0 = torch.where(ok[:, :, None], vel, zero)
    f = (vel0 * 0).sum()
    if g_vel is not None:
        f = f + (vel0 * torch.where(ok[:, :, None], g_vel, zero)).sum()
    if g_ext is not None:
        f = f + (_pick(vel0[:, :, 0], arg[:, 0]) * g_ext[:, 0]).sum() + (_pick(vel0[:, :, 2], arg[:, 1]) * g_ext[:, 1]).sum()
        inv3 = torch.where(ok[:, :, None], torch.where(ok[:, :, None], vel, torch.ones_like(vel)) ** -3.0, zero)
        f = f + (inv3.sum(dim=(1, 2)) * g_ext[:, 2]).sum()
    f.backward()
    return c.grad


# ---------------------------------------------------------------------------------------------------
# the arbiter: numpy longdouble, the adjoint formulas written out
# ---------------------------------------------------------------------------------------------------
LD = np.longdouble


def _ld(t):
    return None if t is None else np.asarray(t.detach().numpy() if isinstance(t, torch.Tensor) else t).astype(LD)


def _hot(arg_col, D):
    """[B] indices -> [B,D] bool (nothing where the index is -1)"""
    return np.arange(D)[None, :] == np.asarray(arg_col)[:, None]


def arb_directional(s, dirs, g_young, g_beta, g_ext, arg):
    """-> (gradient [B,6,6], absolute-sum gradient [B,6,6]) in longdouble"""
    s, dirs, g_young, g_beta, g_ext = _ld(s), _ld(dirs), _ld(g_young), _ld(g_beta), _ld(g_ext)
    B, D = s.shape[0], dirs.shape[0]
    S = (s + s.transpose(0, 2, 1)) / 2
    v = v_of(dirs)
    q = ((v[None, :, :, None] * S[:, None, :, :]) * v[None, :, None, :]).sum(axis=(2, 3))
    E = 1 / q
    gE, gb = np.zeros((B, D), LD), np.zeros((B, D), LD)
    if g_young is not None:
        gE = gE + g_young
    if g_beta is not None:
        gb = gb + g_beta
    if g_ext is not None:
        arg = np.asarray(arg)
        gE = gE + _hot(arg[:, 0], D) * g_ext[:, 0:1] + _hot(arg[:, 1], D) * g_ext[:, 1:2]
        gb = gb + _hot(arg[:, 2], D) * g_ext[:, 2:3] + _hot(arg[:, 3], D) * g_ext[:, 3:4]
    e = np.array([1, 1, 1, 0, 0, 0], LD)
    vv = v[:, :, None] * v[:, None, :]                                             # [D,6,6]
    H = ((-gE * E * E)[:, :, None, None] * vv[None]).sum(axis=1) + (gb[:, :, None, None] * (v[:, :, None] * e)[None]).sum(axis=1)
    Ha = ((np.abs(gE) * E * E)[:, :, None, None] * np.abs(vv)[None]).sum(axis=1) \
        + (np.abs(gb)[:, :, None, None] * (np.abs(v)[:, :, None] * e)[None]).sum(axis=1)
    return (H + H.transpose(0, 2, 1)) / 2, (Ha + Ha.transpose(0, 2, 1)) / 2


def _rotate(a, u, p, q, r):
    """one Jacobi rotation on dicts of [B,D] arrays: a[(i,j)] the symmetric matrix (i <= j), u[(row, col)] the vectors"""
    key = lambda i, j: (min(i, j), max(i, j))
    app, aqq, apq = a[(p, p)], a[(q, q)], a[key(p, q)]
    with np.errstate(all="ignore"):
        theta = (aqq - app) / (2 * apq)
        tn = np.copysign(LD(1), theta) / (np.abs(theta) + np.sqrt(theta * theta + 1))
    tn = np.where(apq == 0, LD(0), tn)
    c = 1 / np.sqrt(tn * tn + 1)
    sn = tn * c
    tau = sn / (1 + c)
    h = tn * apq
    a[(p, p)], a[(q, q)], a[key(p, q)] = app - h, aqq + h, np.zeros_like(apq)
    g, f = a[key(r, p)], a[key(r, q)]
    a[key(r, p)], a[key(r, q)] = g - sn * (f + g * tau), f + sn * (g - f * tau)
    for i in range(3):
        g, f = u[(i, p)], u[(i, q)]
        u[(i, p)], u[(i, q)] = g - sn * (f + g * tau), f + sn * (g - f * tau)


def arb_eigh(G):
    """symmetric [B,D,3,3] longdouble -> (lam [B,D,3] ascending, U [B,D,3,3] with column k = u_k): cyclic Jacobi until no
    off-diagonal entry is left (at most 40 sweeps)"""
    a = {(i, j): G[..., i, j].copy() for i in range(3) for j in range(i, 3)}
    u = {(i, j): np.full(G.shape[:2], LD(i == j)) for i in range(3) for j in range(3)}
    for _ in range(40):
        _rotate(a, u, 0, 1, 2)
        _rotate(a, u, 0, 2, 1)
        _rotate(a, u, 1, 2, 0)
        off = np.abs(a[(0, 1)]) + np.abs(a[(0, 2)]) + np.abs(a[(1, 2)])
        big = np.abs(a[(0, 0)]) + np.abs(a[(1, 1)]) + np.abs(a[(2, 2)])
        if (off <= LD(1e-30) * big).all():
            break
    lam = np.stack([a[(0, 0)], a[(1, 1)], a[(2, 2)]], -1)
    U = np.stack([np.stack([u[(i, k)] for k in range(3)], -1) for i in range(3)], -2)     # [B,D,row,col]
    order = np.argsort(lam, axis=-1, kind="stable")
    return np.take_along_axis(lam, order, -1), np.take_along_axis(U, order[..., None, :], -1)


def arb_acoustic(c, rho, dirs, g_vel, g_ext, arg, unit=UNIT):
    """-> (gradient [B,6,6], absolute-sum gradient [B,6,6], lam [B,D,3], ok [B,D]) in longdouble; unstable directions
    contribute to neither"""
    c, rho, dirs, g_vel, g_ext = _ld(c), _ld(rho), _ld(dirs), _ld(g_vel), _ld(g_ext)
    B, D = c.shape[0], dirs.shape[0]
    C = (c + c.transpose(0, 2, 1)) / 2
    G = np.zeros((B, D, 3, 3), LD)
    for i in range(3):
        for k in range(3):
            for j in range(3):
                for l in range(3):
                    G[:, :, i, k] += C[:, V_OF[i][j], V_OF[k][l]][:, None] * (dirs[:, j] * dirs[:, l])[None, :]
    lam, U = arb_eigh(G)
    ok = (lam > 0).all(axis=-1)
    scale = (LD(unit) / rho)[:, None, None]
    with np.errstate(all="ignore"):
        vel = np.sqrt(np.where(ok[..., None], lam, LD(1)) * scale)
    g_mode, g_sum = np.zeros((B, D, 3), LD), np.zeros((B, D, 3), LD)
    if g_vel is not None:
        g_mode = g_mode + np.where(ok[..., None], g_vel, LD(0))
    if g_ext is not None:
        arg = np.asarray(arg)
        g_mode[:, :, 0] += _hot(arg[:, 0], D) * g_ext[:, 0:1]
        g_mode[:, :, 2] += _hot(arg[:, 1], D) * g_ext[:, 1:2]
        g_sum = -3 * g_ext[:, 2][:, None, None] * vel ** -4
    dv = scale / (2 * vel)                                                            # d v_k / d lambda_k
    w = (g_mode + g_sum) * dv
    lmax, lmin = lam[..., 2:3], lam[..., 0:1]
    with np.errstate(all="ignore"):
        gap = np.stack([lam[..., 1] - lam[..., 0], np.minimum(lam[..., 1] - lam[..., 0], lam[..., 2] - lam[..., 1]),
                        lam[..., 2] - lam[..., 1]], -1)
        w_abs = (np.abs(g_mode) * (1 + lmax / gap) + np.abs(g_sum) * (1 + lmax / lmin)) * dv
    w_abs = np.where(np.abs(g_mode) == 0, np.abs(g_sum) * (1 + lmax / lmin) * dv, w_abs)   # (0 x inf at a degenerate gap)
    n = dirs
    # a_k[I] = sum over the orderings (i,j) of the Voigt pair I of u_k,i n_j   -> [B,D,6,mode]
    a = np.stack([U[:, :, 0, :] * n[None, :, 0, None], U[:, :, 1, :] * n[None, :, 1, None], U[:, :, 2, :] * n[None, :, 2, None],
                  U[:, :, 1, :] * n[None, :, 2, None] + U[:, :, 2, :] * n[None, :, 1, None],
                  U[:, :, 0, :] * n[None, :, 2, None] + U[:, :, 2, :] * n[None, :, 0, None],
                  U[:, :, 0, :] * n[None, :, 1, None] + U[:, :, 1, :] * n[None, :, 0, None]], 2)
    okw = ok[:, :, None]
    w, w_abs = np.where(okw, w, LD(0)), np.where(okw, w_abs, LD(0))
    Hc = np.einsum("bdk,bdik,bdjk->bij", w, a, a)
    Ha = np.einsum("bdk,bdik,bdjk->bij", w_abs, np.abs(a), np.abs(a))
    return (Hc + Hc.transpose(0, 2, 1)) / 2, (Ha + Ha.transpose(0, 2, 1)) / 2, lam, ok


def error_in_units(got, want, absum):
    """max over a row's 36 entries of |got - want| / (eps max|absolute-sum gradient|) -> [B] (0 where the scale is 0 and
    the two agree exactly)"""
    got, want, absum = (np.asarray(x, dtype=LD) for x in (got, want, absum))
    err = np.abs(got - want).reshape(got.shape[0], -1).max(axis=1)
    unit = LD(EPS) * absum.reshape(absum.shape[0], -1).max(axis=1)
    with np.errstate(all="ignore"):
        return np.where(err == 0, LD(0), err / unit).astype(np.float64)


# ---------------------------------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------------------------------
def test_library_declares_and_binds_the_two_adjoint_entries():
    from matten_amd import _lib, autograd, ops

    header = open(os.path.join(ROOT, "include", "matten_hip.h")).read()
    declared = set(re.findall(r"\b(matten_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for name in ("matten_elastic_directional_bwd", "matten_elastic_acoustic_bwd"):
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.ABI_VERSION == 47 and lib.matten_abi_version() == 47          # entries were only added
    assert callable(ops.elastic_directional_bwd) and callable(ops.elastic_acoustic_bwd)
    assert issubclass(autograd.ElasticDirectionalFn, torch.autograd.Function)
    assert issubclass(autograd.ElasticAcousticFn, torch.autograd.Function)


def test_entries_check_their_arguments_like_the_forwards():
    from matten_amd import _lib

    lib = _lib.load()
    d, a = lib.matten_elastic_directional_bwd, lib.matten_elastic_acoustic_bwd
    # (compliance, flags, dirs, n, n_dirs, g_young, g_beta, g_ext, arg, g_compliance, stream)
    assert d(None, None, None, -1, 4, None, None, None, None, None, None) == -1       # negative n
    assert d(None, None, None, 0, 0, None, None, None, None, None, None) == -1        # n_dirs < 1
    assert d(None, None, None, 0, 0x7fffffff // 3 + 1, None, None, None, None, None, None) == -1
    assert d(None, None, None, 2 ** 31, 4, None, None, None, None, None, None) == -1
    assert d(None, None, None, 3, 4, None, None, None, None, None, None) == -1        # null required pointers
    assert d(None, None, None, 0, 4, None, None, None, None, None, None) == 0         # n == 0: nothing to do
    # (voigt, flags, density, dirs, n, n_dirs, modulus_unit, g_vel, g_ext, arg, g_voigt, stream)
    assert a(None, None, None, None, -1, 4, 1e9, None, None, None, None, None) == -1
    assert a(None, None, None, None, 0, 0, 1e9, None, None, None, None, None) == -1
    assert a(None, None, None, None, 0, 0x7fffffff // 3 + 1, 1e9, None, None, None, None, None) == -1
    assert a(None, None, None, None, 2 ** 31, 4, 1e9, None, None, None, None, None) == -1
    assert a(None, None, None, None, 3, 4, 1e9, None, None, None, None, None) == -1
    assert a(None, None, None, None, 0, 4, 1e9, None, None, None, None, None) == 0
    # the extremes' gradient without the recorded directions (a host buffer: nothing is launched for n == 0)
    buf = (ctypes.c_double * 4)()
    idx = (ctypes.c_int32 * 4)()
    p, i = ctypes.addressof(buf), ctypes.addressof(idx)
    assert d(None, None, None, 0, 4, None, None, p, None, None, None) == -1
    assert d(None, None, None, 0, 4, None, None, p, i, None, None) == 0
    assert a(None, None, None, None, 0, 4, 1e9, None, p, None, None, None) == -1
    assert a(None, None, None, None, 0, 4, 1e9, None, p, i, None, None) == 0


def test_elastic_moduli_validates_the_directional_arguments_before_touching_the_device():
    """host tensors throughout: each call must fail on the directional argument, not reach the 'device tensors only' error"""
    from matten_amd import elastic

    c = torch.zeros(3, 6, 6, dtype=torch.float64)
    x = torch.zeros(3, 21)
    for fn, t in ((elastic.elastic_moduli, c), (elastic.elastic_moduli_from_irreps, x)):
        with pytest.raises(ValueError, match="pair quantities carry no gradient"):
            fn(t, directions=8, angles=4)
        with pytest.raises(ValueError, match="pair quantities carry no gradient"):
            fn(t, angles=4)
        with pytest.raises(ValueError, match="directions"):
            fn(t, directions=0)
        with pytest.raises(ValueError, match="directions"):
            fn(t, directions=np.zeros((4, 2)))
        with pytest.raises(ValueError, match="zero vector at index 1"):
            fn(t, directions=np.array([[1.0, 0, 0], [0, 0, 0]]))
        with pytest.raises(ValueError, match="density: .*pass directions"):
            fn(t, density=[1.0, 2.0, 3.0])
        with pytest.raises(ValueError, match="number_density: .*pass density"):
            fn(t, directions=8, number_density=[1.0, 2.0, 3.0])
        with pytest.raises(ValueError, match="density: expected 3 value"):
            fn(t, directions=8, density=[1.0, 2.0])
        with pytest.raises(ValueError, match=r"density: expected finite positive values, got -2\.0 at index 1"):
            fn(t, directions=8, density=[1.0, -2.0, float("nan")])
        with pytest.raises(ValueError, match="number_density: expected finite positive values, got nan at index 2"):
            fn(t, directions=8, density=[1.0, 2.0, 3.0], number_density=[1e28, 1e28, float("nan")])
        # everything valid: only now the host tensor itself is refused
        with pytest.raises(ValueError, match="device tensors only"):
            fn(t, directions=8, density=[1.0, 2.0, 3.0], number_density=[1e28, 2e28, 3e28], keep_directional=True)
    with pytest.raises(ValueError, match="density: expected 1 value"):
        elastic.elastic_moduli(torch.zeros(6, 6), directions=4, density=[1.0, 2.0])


def test_moduli_loss_accepts_the_directional_names_and_names_the_missing_argument():
    from matten_amd.elastic import DIRECTIONAL_NAMES, PROP_NAMES, ModuliLoss

    assert tuple(DIRECTIONAL_NAMES) == NEW_NAMES and not set(NEW_NAMES) & set(PROP_NAMES)
    loss = ModuliLoss(names=NEW_NAMES + ("k_vrh",))
    assert loss.names == NEW_NAMES + ("k_vrh",) and loss.weights["debye_temperature"] == 1.0
    with pytest.raises(ValueError, match="bulk"):
        ModuliLoss(names=("young_max", "bulk"))
    with pytest.raises(ValueError, match="shear_max"):                       # a pair quantity: no gradient, not a name
        ModuliLoss(names=("shear_max",))
    with pytest.raises(ValueError, match="young"):                           # the [B,D] map is not a [B] name
        ModuliLoss(names=("young",))
    with pytest.raises(ValueError):
        ModuliLoss(names=("v_mean", "v_mean"))
    p = fake_props()                                                         # the ten scalars only
    zeros = torch.zeros(5, dtype=torch.float64)
    for name, argument in (("young_max", "directions"), ("compressibility_min", "directions"), ("v_fast_max", "density"),
                           ("v_mean", "density"), ("debye_temperature", "number_density")):
        with pytest.raises(ValueError, match=rf"{name}.*pass {argument}\b"):
            ModuliLoss(names=(name,))(p, {name: zeros})
    with pytest.raises(ValueError, match="v_mean"):                          # a target is missing
        ModuliLoss(names=("k_vrh", "v_mean"))(p, {"k_vrh": zeros})


@pytest.mark.parametrize("kind", ["l1", "mse"])
def test_moduli_loss_excludes_non_finite_values_of_the_directional_names(kind):
    from matten_amd.elastic import ModuliLoss

    B = 5
    flags = torch.tensor([0, 0, 1, 0, 0], dtype=torch.int32)                  # row 2 singular
    leaf = lambda vals: torch.tensor(vals, dtype=torch.float64, requires_grad=True)
    nan, inf = float("nan"), float("inf")
    theta = leaf([300.0, nan, nan, 320.0, 330.0])                            # row 1: unstable directions
    ymax = leaf([200.0, 210.0, nan, inf, 240.0])                             # row 3: a direction with q = 0
    p = fake_props(B, flags=flags, debye_temperature=theta, young_max=ymax)
    with torch.no_grad():
        p.k_vrh[2] = nan
    targets = {"debye_temperature": torch.tensor([310.0, 311.0, 312.0, nan, 335.0], dtype=torch.float64),
               "young_max": torch.full((B,), 205.0, dtype=torch.float64), "k_vrh": torch.full((B,), 45.0, dtype=torch.float64)}
    loss = ModuliLoss(names=("debye_temperature", "young_max", "k_vrh"), weights=(1.0, 0.5, 2.0), kind=kind)(p, targets)
    f = (lambda d: abs(d)) if kind == "l1" else (lambda d: d * d)
    k = p.k_vrh.detach()
    # debye: rows 0, 4; young_max: rows 0, 1, 4; k_vrh: rows 0, 1, 3, 4 -> nine entries
    want = (f(300.0 - 310.0) + f(330.0 - 335.0) + 0.5 * (f(200.0 - 205.0) + f(210.0 - 205.0) + f(240.0 - 205.0))
            + 2.0 * sum(f(k[r].item() - 45.0) for r in (0, 1, 3, 4))) / 9.0
    assert torch.isfinite(loss) and abs(loss.item() - want) <= 1e-12 * abs(want)
    loss.backward()
    for g in (theta.grad, ymax.grad, p.k_vrh.grad):
        assert torch.isfinite(g).all()
    assert torch.equal(theta.grad[[1, 2, 3]], torch.zeros(3, dtype=torch.float64)) and (theta.grad[[0, 4]] != 0).all()
    assert torch.equal(ymax.grad[[2, 3]], torch.zeros(2, dtype=torch.float64)) and (ymax.grad[[0, 1, 4]] != 0).all()
    assert p.k_vrh.grad[2] == 0 and (p.k_vrh.grad[[0, 1, 3, 4]] != 0).all()
    # the ten scalar names keep their behaviour: a non-finite VALUE on an unflagged row is not excluded for them
    q = fake_props(3)
    with torch.no_grad():
        q.g_vrh[1] = nan
    assert torch.isnan(ModuliLoss(names=("g_vrh",))(q, {"g_vrh": torch.zeros(3, dtype=torch.float64)}))


def test_reference_forwards_pass_gradcheck_and_match_numpy():
    """the reference the GPU tests lean on: its values against plain numpy loops, its autograd against central finite
    differences, on three generic tensors (unsymmetric noise included, so both symmetrisations are exercised)"""
    from matten_amd.elastic import fibonacci_hemisphere

    dirs_n = fibonacci_hemisphere(7)
    dirs = torch.tensor(dirs_n)
    for seed, row in ((0, 0), (1, 3), (4, 5)):
        c_n = generic_tensors(seed)[row]
        assert np.abs(c_n - c_n.T).max() > 1e-3
        C = 0.5 * (c_n + c_n.T)
        s_n = np.linalg.inv(C) + 1e-6 * np.random.default_rng(seed).standard_normal((6, 6))
        S = 0.5 * (s_n + s_n.T)
        c, s, rho = torch.tensor(c_n)[None], torch.tensor(s_n)[None], torch.tensor([3100.0], dtype=torch.float64)
        E, beta = ref_directional(s, dirs)
        vel, ok, lam = ref_acoustic(c, rho, dirs)
        assert ok.all()
        for d, n in enumerate(dirs_n):
            v = np.array([n[0] ** 2, n[1] ** 2, n[2] ** 2, n[1] * n[2], n[0] * n[2], n[0] * n[1]])
            assert abs(E[0, d].item() - 1.0 / (v @ S @ v)) <= 1e-13 * abs(E[0, d].item())
            assert abs(beta[0, d].item() - sum(S[i, j] * v[i] for i in range(6) for j in range(3))) <= 1e-13 * np.abs(S).max()
            G = np.array([[sum(C[V_OF[i][j], V_OF[k][l]] * n[j] * n[l] for j in range(3) for l in range(3)) for k in range(3)]
                          for i in range(3)])
            want = np.sqrt(np.linalg.eigvalsh(G) * UNIT / 3100.0)
            assert np.abs(vel[0, d].numpy() - want).max() <= 1e-12 * want.max()

        def fn_dir(x):
            E, beta = ref_directional(x, dirs)
            return torch.cat([E.reshape(-1) * 1e-2, beta.reshape(-1) * 1e3])      # E ~ 1e2, beta ~ 1e-3: lifted to O(1)

        def fn_ac(x):
            vel, _, _ = ref_acoustic(x, rho, dirs)
            return torch.cat([vel.reshape(-1) * 1e-3, (vel ** -3.0).sum().reshape(1) * 1e11])

        assert torch.autograd.gradcheck(fn_dir, (s.clone().requires_grad_(),), eps=1e-7, atol=1e-5, rtol=1e-5)
        assert torch.autograd.gradcheck(fn_ac, (c.clone().requires_grad_(),), eps=1e-3, atol=1e-6, rtol=1e-5)


def test_arbiter_agrees_with_the_reference_autograd():
    """the longdouble arbiter (Jacobi with eigenvectors, the rank-one form of the adjoint) against fp64 autograd through
    LAPACK's eigvalsh, in units of eps times the absolute-sum gradient: two independent statements of the same derivative"""
    from matten_amd.elastic import fibonacci_hemisphere

    c_n = generic_tensors(2)
    B, D = 6, 65
    dirs = torch.tensor(fibonacci_hemisphere(D))
    c, rho = torch.tensor(c_n), torch.tensor(densities(B))
    s = torch.linalg.inv(0.5 * (c + c.transpose(1, 2)))
    g = torch.Generator().manual_seed(7)
    rnd = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float64)
    E, beta = ref_directional(s, dirs)
    arg_d = torch.stack([E.argmin(1), E.argmax(1), beta.argmin(1), beta.argmax(1)], 1).int()
    gy, gb, gx = rnd(B, D), 1e5 * rnd(B, D), torch.cat([rnd(B, 2), 1e5 * rnd(B, 2)], 1)
    got, absum = arb_directional(s, dirs, gy, gb, gx, arg_d)
    worst_d = error_in_units(ref_directional_grad(s, dirs, gy, gb, gx, arg_d).numpy(), got, absum).max()
    vel, ok, lam = ref_acoustic(c, rho, dirs)
    assert ok.all()
    arg_a = torch.stack([vel[:, :, 0].argmin(1), vel[:, :, 2].argmax(1)], 1).int()
    gv, ga = rnd(B, D, 3), torch.cat([rnd(B, 2), SUM_SCALE * rnd(B, 1)], 1)
    got, absum, lam_a, ok_a = arb_acoustic(c, rho, dirs, gv, ga, arg_a)
    assert ok_a.all() and np.abs(lam_a.astype(np.float64) - lam.numpy()).max() <= 1e-12 * lam.max().item()
    worst_a = error_in_units(ref_acoustic_grad(c, rho, dirs, gv, ga, arg_a).numpy(), got, absum).max()
    print(f"reference against the arbiter: directional {worst_d:.3f}, acoustic {worst_a:.3f} units")
    # either statement takes a contribution through fewer than 16 rounded operations, each worth at most one unit
    assert worst_d <= 16.0 and worst_a <= 16.0
