"""
Gradients through the directional and acoustic elastic properties on the GPU (matten_elastic_directional_bwd,
matten_elastic_acoustic_bwd; elastic_moduli / elastic_moduli_from_irreps with directions, density and number_density;
ModuliLoss on the directional names) against the two CPU statements of tests/test_elastic_dir_grad_host.py: the fp64 torch
REFERENCE (autograd through LAPACK's eigvalsh, gradcheck'ed there) and the numpy longdouble ARBITER (the adjoint formulas
written out, cyclic Jacobi with eigenvectors run to convergence).

Accuracy contract of the two kernels (tests 1-3), in the manner of tests/test_gpu_elastic_grad.py: no constant is picked in
advance.  Per output row the unit is  eps max|absolute-sum gradient|,  eps = 2^-52: the same accumulation with every
per-direction contribution replaced by its magnitude, so cancellation between directions does not shrink the scale; for the
acoustic kernel a mode's share is further weighted by 1 + lambda_max / gap (gap: the distance to the nearest other
eigenvalue) for per-mode upstream gradients and by 1 + lambda_max / lambda_min for the sum of v^-3 (the host file's header).
In these units the reference's own error against the arbiter, on exactly the inputs and upstream gradients of tests 1-3
(`python tests/test_gpu_elastic_dir_grad.py` measures it on the CPU, no GPU needed), is at most
    directional  REF_DIR = 6.8863   (worst: everything random on test 3's indefinite row, where v^T S v nearly cancels
                                     along some directions; generic tensors 4.2126, one-hot on young_min, seed 4, D = 255)
    acoustic     REF_AC  = 2.4264   (worst: the sum of v^-3 alone, seed 2, D = 1; test 3's indefinite row 0.3184)
and the device is allowed 16x that -- the project's margin for another evaluation order and Jacobi instead of LAPACK:
    C_DIR = 16 REF_DIR = 110.18,  C_AC = 16 REF_AC = 38.82.
The device is compared with the arbiter (the judge), so the reference's own error is not spent twice.
Measured on MI355X (printed by the tests): directional at most 3.71 units on generic tensors (one-hot on young_min; random
gradients on everything 1.89) and 4.61 on the indefinite row; acoustic at most 1.46 (the sum alone, D = 1; everything random
0.96), 0.14 at exactly degenerate modes, 0.18 on the indefinite row; end to end 1.8e-6 of the tensor scale.

Inputs of tests 1, 3, 4: C = 30 (A A^T + 6 I), A 6x6 standard normal of numpy.random.default_rng(seed), seeds 0..4, six rows
each, plus 0.01-scale unsymmetric noise on the Voigt input: cond(C) < 5, every Christoffel eigenvalue positive on every
Fibonacci set used, relative mode gap (gap / lambda_max) >= 1.04e-3 (worst at seed 1).  Each case asserts cond < 5,
positivity and a gap of at least 1e-4 on its reference as a condition of the inputs.  The compliance of the directional
kernel is the inverse of the symmetrised matrix, fp64 on the CPU, uploaded; both kernels are tested on their own through ops.

Wiring (test 5) is BITWISE: every accumulation autograd performs there has two non-zero terms (a + b = b + a) or adds
zeros, so c.grad equals the three adjoints called by hand bit for bit; no allowance is needed.
End to end (test 6): parameter gradients against the oracle's autograd within the project's _close(..., 3e-3), the loss
within 2e-3 relative.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path[:0] = [os.path.dirname(os.path.abspath(__file__)), os.path.dirname(os.path.dirname(os.path.abspath(__file__)))]
from test_elastic_grad_host import NAMES as PROPS      # noqa: E402  (the ten scalars)
from test_elastic_dir_grad_host import (SUM_SCALE, UNIT, arb_acoustic, arb_directional, cubic, densities,   # noqa: E402
                                        error_in_units, generic_tensors, ref_acoustic, ref_acoustic_grad, ref_christoffel,
                                        ref_directional, ref_directional_grad)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
REF_DIR, REF_AC = 6.8863, 2.4264     # measured on the CPU: the header, measure_reference()
C_DIR, C_AC = 16.0 * REF_DIR, 16.0 * REF_AC
D_SET = (1, 63, 64, 65, 255, 256, 257, 600)        # lane, wave and workgroup-stride boundaries
SEEDS = (0, 1, 2, 3, 4)
DIR_MODES = ("map", "beta", "young_min", "young_max", "beta_min", "beta_max", "all")
AC_MODES = ("map", "slow_min", "fast_max", "sum", "all")
BETA_SCALE = 1e5      # beta ~ 1e-3, E ~ 1e2: lifts the compressibility's gradients to the size of Young's


def fib(D):
    from matten_amd.elastic import fibonacci_hemisphere

    return torch.tensor(fibonacci_hemisphere(D))


# ---------------------------------------------------------------------------------------------------
# upstream gradients and CPU cases, made once and shared (B = 1 is row 0 of the six)
# ---------------------------------------------------------------------------------------------------
def dir_upstream(mode, seed, D, B=6):
    """(g_young [B,D], g_beta [B,D], g_ext [B,4]) fp64, absent ones None"""
    g = torch.Generator().manual_seed(1000 * seed + 10 * D + DIR_MODES.index(mode))
    rnd = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float64)
    if mode == "map":
        return rnd(B, D), None, None
    if mode == "beta":
        return None, BETA_SCALE * rnd(B, D), None
    if mode == "all":
        return rnd(B, D), BETA_SCALE * rnd(B, D), torch.cat([rnd(B, 2), BETA_SCALE * rnd(B, 2)], 1)
    gx = torch.zeros(B, 4, dtype=torch.float64)
    gx[:, DIR_MODES.index(mode) - 2] = 1.0
    return None, None, gx


def ac_upstream(mode, seed, D, B=6):
    """(g_vel [B,D,3], g_ext [B,3]) fp64, absent ones None"""
    g = torch.Generator().manual_seed(2000 * seed + 10 * D + AC_MODES.index(mode))
    rnd = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float64)
    if mode == "map":
        return rnd(B, D, 3), None
    if mode == "all":
        return rnd(B, D, 3), torch.cat([rnd(B, 2), SUM_SCALE * rnd(B, 1)], 1)
    gx = torch.zeros(B, 3, dtype=torch.float64)
    gx[:, AC_MODES.index(mode) - 1] = SUM_SCALE if mode == "sum" else 1.0
    return None, gx


_CASES = {}


def dir_case(seed, D):
    """-> dict(s, dirs, arg, modes: mode -> (upstreams, arbiter gradient, absolute-sum gradient))"""
    key = ("dir", seed, D)
    if key not in _CASES:
        c = torch.tensor(generic_tensors(seed))
        C = 0.5 * (c + c.transpose(1, 2))
        assert torch.linalg.cond(C).max() < 5
        s, dirs = torch.linalg.inv(C), fib(D)
        E, beta = ref_directional(s, dirs)
        arg = torch.stack([E.argmin(1), E.argmax(1), beta.argmin(1), beta.argmax(1)], 1).int()
        modes = {}
        for mode in DIR_MODES:
            ups = dir_upstream(mode, seed, D)
            modes[mode] = (ups,) + arb_directional(s, dirs, *ups, arg)
        _CASES[key] = dict(s=s, dirs=dirs, arg=arg, modes=modes)
    return _CASES[key]


def ac_case(seed, D):
    key = ("ac", seed, D)
    if key not in _CASES:
        c, dirs, rho = torch.tensor(generic_tensors(seed)), fib(D), torch.tensor(densities(6))
        assert torch.linalg.cond(0.5 * (c + c.transpose(1, 2))).max() < 5
        vel, ok, lam = ref_acoustic(c, rho, dirs)
        gap = torch.minimum(lam[..., 1] - lam[..., 0], lam[..., 2] - lam[..., 1]) / lam[..., 2]
        assert ok.all() and lam.min() > 0 and gap.min() >= 1e-4, (seed, D, gap.min().item())      # a condition of the inputs
        arg = torch.stack([vel[:, :, 0].argmin(1), vel[:, :, 2].argmax(1)], 1).int()
        modes = {}
        for mode in AC_MODES:
            ups = ac_upstream(mode, seed, D)
            modes[mode] = (ups,) + arb_acoustic(c, rho, dirs, *ups, arg)[:2]
        _CASES[key] = dict(c=c, dirs=dirs, rho=rho, arg=arg, modes=modes)
    return _CASES[key]


def dev(t, rows=None):
    if t is None:
        return None
    return (t if rows is None else t[rows]).contiguous().to(DEV)


def zero_flags(B):
    return torch.zeros(B, dtype=torch.int32, device=DEV)


def run_directional(s, dirs, ups, flags=None):
    """forward (for the recorded directions) and adjoint through ops -> (g_compliance on the host, arg on the host)"""
    from matten_amd import ops

    s, dirs = s.to(DEV), dirs.to(DEV)
    flags = zero_flags(s.shape[0]) if flags is None else flags
    _, _, _, arg = ops.elastic_directional(s, flags, dirs)
    gy, gb, gx = (dev(t) for t in ups)
    got = ops.elastic_directional_bwd(s, flags, dirs, gy, gb, gx, None if gx is None else arg)
    return got.cpu(), arg.cpu()


def run_acoustic(c, rho, dirs, ups, flags=None):
    from matten_amd import ops

    c, rho, dirs = c.to(DEV), rho.to(DEV), dirs.to(DEV)
    flags = zero_flags(c.shape[0]) if flags is None else flags
    _, _, arg, n_unstable = ops.elastic_acoustic(c, flags, rho, dirs, UNIT)
    gv, gx = (dev(t) for t in ups)
    got = ops.elastic_acoustic_bwd(c, flags, rho, dirs, UNIT, gv, gx, None if gx is None else arg)
    return got.cpu(), arg.cpu(), n_unstable.cpu()


# ---------------------------------------------------------------------------------------------------
# 1. the adjoints against the arbiter
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 6])
@pytest.mark.parametrize("D", D_SET)
def test_directional_adjoint(D, B):
    worst = {m: 0.0 for m in DIR_MODES}
    for seed in SEEDS:
        case = dir_case(seed, D)
        for mode in DIR_MODES:
            ups, want, absum = case["modes"][mode]
            got, arg = run_directional(case["s"][:B], case["dirs"], [None if t is None else t[:B] for t in ups])
            assert torch.equal(arg, case["arg"][:B]), (seed, mode)
            assert got.shape == (B, 6, 6) and torch.isfinite(got).all()
            worst[mode] = max(worst[mode], error_in_units(got.numpy(), want[:B], absum[:B]).max())
    top = max(worst, key=worst.get)
    print(f"directional adjoint D={D} B={B}: worst error {worst[top]:.3f} units at {top} (allowed {C_DIR:.3f}); "
          + " ".join(f"{m}={v:.2f}" for m, v in worst.items()))
    assert worst[top] <= C_DIR, worst


@pytest.mark.parametrize("B", [1, 6])
@pytest.mark.parametrize("D", D_SET)
def test_acoustic_adjoint(D, B):
    worst = {m: 0.0 for m in AC_MODES}
    for seed in SEEDS:
        case = ac_case(seed, D)
        for mode in AC_MODES:
            ups, want, absum = case["modes"][mode]
            got, arg, n_unstable = run_acoustic(case["c"][:B], case["rho"][:B], case["dirs"],
                                                [None if t is None else t[:B] for t in ups])
            assert torch.equal(arg, case["arg"][:B]) and not n_unstable.any(), (seed, mode)
            assert got.shape == (B, 6, 6) and torch.isfinite(got).all()
            worst[mode] = max(worst[mode], error_in_units(got.numpy(), want[:B], absum[:B]).max())
    top = max(worst, key=worst.get)
    print(f"acoustic adjoint D={D} B={B}: worst error {worst[top]:.3f} units at {top} (allowed {C_AC:.3f}); "
          + " ".join(f"{m}={v:.2f}" for m, v in worst.items()))
    assert worst[top] <= C_AC, worst


def test_all_upstream_pointers_null_write_zeros():
    case_d, case_a = dir_case(0, 65), ac_case(0, 65)
    got, _ = run_directional(case_d["s"], case_d["dirs"], (None, None, None))
    assert torch.equal(got, torch.zeros(6, 6, 6, dtype=torch.float64))
    got, _, _ = run_acoustic(case_a["c"], case_a["rho"], case_a["dirs"], (None, None))
    assert torch.equal(got, torch.zeros(6, 6, 6, dtype=torch.float64))


# ---------------------------------------------------------------------------------------------------
# 2. degenerate modes
# ---------------------------------------------------------------------------------------------------
def degenerate_inputs():
    c = torch.tensor(np.stack([cubic(165.0, 64.0, 79.0), cubic(250.0, 110.0, 70.0)]))      # cubic; isotropic (c11 - c12 = 2 c44)
    special = np.array([[1.0, 0, 0], [1, 1, 0], [1, 1, 1]])
    special /= np.linalg.norm(special, axis=1, keepdims=True)
    dirs = torch.cat([torch.tensor(special), fib(64)])
    return c, torch.tensor([2330.0, 7800.0], dtype=torch.float64), dirs


def test_degenerate_modes_sum_gradient_is_right_and_per_mode_gradients_stay_finite():
    c, rho, dirs = degenerate_inputs()
    B, D = 2, dirs.shape[0]
    lam = torch.linalg.eigvalsh(ref_christoffel(c, dirs))
    assert (lam[0, 0, 2] - lam[0, 0, 1]).abs() <= 1e-12 * lam[0, 0, 2] or (lam[0, 0, 1] - lam[0, 0, 0]).abs() <= 1e-12 * lam[0, 0, 2]
    assert ((lam[1, :, 1] - lam[1, :, 0]) <= 1e-12 * lam[1, :, 2]).all()                 # isotropic: two equal shear modes
    gx = torch.zeros(B, 3, dtype=torch.float64)
    gx[:, 2] = SUM_SCALE
    got, arg, n_unstable = run_acoustic(c, rho, dirs, (None, gx))
    assert not n_unstable.any() and torch.isfinite(got).all()
    want, absum, _, ok = arb_acoustic(c, rho, dirs, None, gx, arg)
    assert ok.all() and np.isfinite(absum.astype(np.float64)).all()
    units = error_in_units(got.numpy(), want, absum)
    print(f"degenerate modes, sum of v^-3 alone: worst error {units.max():.3f} units (allowed {C_AC:.3f}); "
          f"cubic {units[0]:.2f} isotropic {units[1]:.2f}")
    assert units.max() <= C_AC
    # the reference (LAPACK, any basis of the degenerate pair) agrees too: the sum's gradient does not depend on the basis
    ref = ref_acoustic_grad(c, rho, dirs, None, gx, arg)
    assert error_in_units(ref.numpy(), want, absum).max() <= C_AC
    # per-mode upstream gradients: no defined derivative at the degenerate directions, the result is merely finite
    gv, gx_all = ac_upstream("all", 9, D, B)
    got, _, _ = run_acoustic(c, rho, dirs, (gv, gx_all))
    assert torch.isfinite(got).all()
    got, _, _ = run_acoustic(c, rho, dirs, (gv, None))
    assert torch.isfinite(got).all() and got.abs().max() > 0


# ---------------------------------------------------------------------------------------------------
# 3. excluded entries
# ---------------------------------------------------------------------------------------------------
def indefinite_tensor():
    C = np.diag([200.0, 180.0, 150.0, 60.0, -40.0, 50.0])       # a negative shear constant: unstable along some directions
    C[0, 1] = C[1, 0] = 70.0
    return C


def excluded_acoustic_batch(D=65):
    """flagged | rho = 0 | rho < 0 | rho = NaN | indefinite, each between good neighbours
    -> (c [11,6,6], rho [11], flags [11], dirs, kinds)"""
    case = ac_case(3, D)
    good, nan = case["c"], float("nan")
    kinds = ["good", "flag", "good", "rho", "good", "rho", "good", "rho", "good", "indef", "good"]
    c = torch.stack([good[0], torch.full((6, 6), nan, dtype=torch.float64), good[1], good[1], good[2], good[2], good[3], good[3],
                     good[4], torch.tensor(indefinite_tensor()), good[5]])
    rho = torch.tensor(densities(len(kinds)))
    rho[3], rho[5], rho[7] = 0.0, -2700.0, nan
    flags = torch.tensor([1 if k == "flag" else 0 for k in kinds], dtype=torch.int32)
    return c, rho, flags, case["dirs"], kinds


def test_acoustic_excluded_rows_and_directions():
    D = 65
    c, rho, flags, dirs, kinds = excluded_acoustic_batch(D)
    B, nan = c.shape[0], float("nan")
    bad_rows = [i for i, k in enumerate(kinds) if k in ("flag", "rho")]
    good_rows = [i for i, k in enumerate(kinds) if k == "good"]
    indef = kinds.index("indef")

    from matten_amd import ops

    vel, ext, arg, n_unstable = ops.elastic_acoustic(c.to(DEV), flags.to(DEV), rho.to(DEV), dirs.to(DEV), UNIT, keep=True)
    vel, arg, n_unstable = vel.cpu(), arg.cpu(), n_unstable.cpu()
    assert n_unstable[bad_rows].tolist() == [-1] * 4 and not n_unstable[good_rows].any()
    assert 0 < n_unstable[indef] < D
    unstable = torch.isnan(vel[indef, :, 0])
    assert int(unstable.sum()) == int(n_unstable[indef])

    gv, gx = ac_upstream("all", 3, D, B)
    gv[bad_rows], gx[bad_rows] = nan, nan                  # NaN at every excluded row ...
    gv[indef, unstable] = nan                              # ... and direction
    got = ops.elastic_acoustic_bwd(c.to(DEV), flags.to(DEV), rho.to(DEV), dirs.to(DEV), UNIT, gv.to(DEV), gx.to(DEV),
                                   arg.to(DEV)).cpu()
    assert not torch.isnan(got).any() and torch.isfinite(got).all()
    assert torch.equal(got[bad_rows], torch.zeros(4, 6, 6, dtype=torch.float64))
    # the indefinite row: its unstable directions contribute nothing -- the arbiter with those directions masked
    one = slice(indef, indef + 1)
    want, absum, _, ok = arb_acoustic(c[one], rho[one], dirs, gv[one], gx[one], arg[one])
    assert np.array_equal(~ok[0], unstable.numpy())
    units = error_in_units(got[one].numpy(), want, absum)
    print(f"indefinite row, {int(n_unstable[indef])} of {D} directions unstable: error {units.max():.3f} units (allowed {C_AC:.3f})")
    assert units.max() <= C_AC and np.abs(want).max() > 0
    ref = ref_acoustic_grad(c[one], rho[one], dirs, torch.nan_to_num(gv[one]), gx[one], arg[one])
    assert error_in_units(ref.numpy(), want, absum).max() <= C_AC
    # the neighbours: bitwise what they are in a batch without the bad rows
    keep = good_rows
    alone = ops.elastic_acoustic_bwd(dev(c, keep), zero_flags(len(keep)), dev(rho, keep), dirs.to(DEV), UNIT, dev(gv, keep),
                                     dev(gx, keep), dev(arg, keep)).cpu()
    assert torch.equal(got[keep], alone) and (alone.abs().amax(dim=(1, 2)) > 0).all()
    # null upstream pointers on the same batch: zeros everywhere, excluded rows included
    none = ops.elastic_acoustic_bwd(c.to(DEV), flags.to(DEV), rho.to(DEV), dirs.to(DEV), UNIT).cpu()
    assert torch.equal(none, torch.zeros(B, 6, 6, dtype=torch.float64))


def test_directional_excluded_rows():
    D = 65
    case = dir_case(3, D)
    good, dirs = case["s"], case["dirs"]
    nan = float("nan")
    s = torch.stack([good[0], torch.full((6, 6), nan, dtype=torch.float64), good[1],
                     torch.tensor(np.linalg.inv(indefinite_tensor())), good[2]])
    flags = torch.tensor([0, 1, 0, 2, 0], dtype=torch.int32)
    gy, gb, gx = dir_upstream("all", 3, D, 5)
    for t in (gy, gb, gx):
        t[1] = nan
    from matten_amd import ops

    _, _, _, arg = ops.elastic_directional(s.to(DEV), flags.to(DEV), dirs.to(DEV))
    assert arg[1].cpu().tolist() == [-1] * 4
    got = ops.elastic_directional_bwd(s.to(DEV), flags.to(DEV), dirs.to(DEV), gy.to(DEV), gb.to(DEV), gx.to(DEV), arg).cpu()
    assert torch.isfinite(got).all() and torch.equal(got[1], torch.zeros(6, 6, dtype=torch.float64))
    # the indefinite row is differentiated like any other
    want, absum = arb_directional(s[3:4], dirs, gy[3:4], gb[3:4], gx[3:4], arg[3:4].cpu())
    units = error_in_units(got[3:4].numpy(), want, absum)
    print(f"directional, indefinite row: error {units.max():.3f} units (allowed {C_DIR:.3f})")
    assert units.max() <= C_DIR
    keep = [0, 2, 4]
    alone = ops.elastic_directional_bwd(dev(s, keep), zero_flags(3), dirs.to(DEV), dev(gy, keep), dev(gb, keep), dev(gx, keep),
                                        arg[keep].contiguous()).cpu()
    assert torch.equal(got[keep], alone) and (alone.abs().amax(dim=(1, 2)) > 0).all()
    # an extreme recorded as -1 (or anything outside the direction set) adds nothing, whatever its gradient holds
    arg_none = torch.full((3, 4), -1, dtype=torch.int32, device=DEV)
    poisoned = torch.full((3, 4), nan, dtype=torch.float64, device=DEV)
    a = ops.elastic_directional_bwd(dev(s, keep), zero_flags(3), dirs.to(DEV), dev(gy, keep), dev(gb, keep), poisoned, arg_none)
    b = ops.elastic_directional_bwd(dev(s, keep), zero_flags(3), dirs.to(DEV), dev(gy, keep), dev(gb, keep))
    assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------
# 4. the same bits twice
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [65, 600])
def test_two_launches_and_two_batch_positions_give_the_same_bits(D):
    cd, ca = dir_case(1, D), ac_case(1, D)
    ups_d, ups_a = cd["modes"]["all"][0], ca["modes"]["all"][0]
    a, _ = run_directional(cd["s"], cd["dirs"], ups_d)
    b, _ = run_directional(cd["s"], cd["dirs"], ups_d)
    alone, _ = run_directional(cd["s"][3:4], cd["dirs"], [t[3:4] for t in ups_d])
    assert torch.equal(a, b) and torch.equal(a[3:4], alone)
    a, _, _ = run_acoustic(ca["c"], ca["rho"], ca["dirs"], ups_a)
    b, _, _ = run_acoustic(ca["c"], ca["rho"], ca["dirs"], ups_a)
    alone, _, _ = run_acoustic(ca["c"][3:4], ca["rho"][3:4], ca["dirs"], [t[3:4] for t in ups_a])
    assert torch.equal(a, b) and torch.equal(a[3:4], alone)
    # both outputs are symmetric exactly: every entry and its mirror come from the same sums
    assert torch.equal(a, a.transpose(1, 2))


# ---------------------------------------------------------------------------------------------------
# 5. wiring: elastic_moduli / elastic_moduli_from_irreps against the three adjoints called by hand
# ---------------------------------------------------------------------------------------------------
MAPS = ("young", "compressibility", "velocities")
EXT_D = ("young_min", "young_max", "compressibility_min", "compressibility_max")
SCALARS = ("voigt", "compliance") + MAPS + EXT_D + ("v_slow_min", "v_fast_max", "sum_inv_v3", "v_mean", "debye_temperature")
INTEGERS = ("flags", "young_argmin", "young_argmax", "compressibility_argmin", "compressibility_argmax", "v_slow_min_direction",
            "v_fast_max_direction", "acoustic_unstable_directions")


def loss_weights(p, names):
    g = torch.Generator().manual_seed(77)
    return {n: torch.randn(getattr(p, n).shape, generator=g, dtype=torch.float64).to(DEV) for n in names}


def by_hand(rows, dtype, dirs, rho, nd, w):
    """the same loss through ops alone: forwards, the upstream gradients of each kernel's outputs, the three adjoints"""
    from matten_amd import ops
    from matten_amd.elastic import HBAR, K_B

    D = dirs.shape[0]
    voigt, compliance, props, flags = ops.elastic_props(rows, 1)
    _, _, ext_d, arg_d = ops.elastic_directional(compliance, flags, dirs, keep=True)
    _, ext_a, arg_a, _ = ops.elastic_acoustic(voigt, flags, rho, dirs, UNIT, keep=True)
    # sum v^-3 feeds three fields: its own, v_mean and the Debye temperature (torch expressions, as in the module)
    e = ext_a[:, 2].clone().requires_grad_()
    v_mean = (e / (3.0 * D)) ** (-1.0 / 3.0)
    theta = (HBAR / K_B) * (6.0 * np.pi ** 2 * nd) ** (1.0 / 3.0) * v_mean
    ((e * w["sum_inv_v3"]).sum() + (v_mean * w["v_mean"]).sum() + (theta * w["debye_temperature"]).sum()).backward()
    g_ext_a = torch.stack([w["v_slow_min"], w["v_fast_max"], e.grad], 1)
    g_ext_d = torch.stack([w[n] for n in EXT_D], 1)
    g_voigt = w["voigt"] + ops.elastic_acoustic_bwd(voigt, flags, rho, dirs, UNIT, w["velocities"], g_ext_a, arg_a)
    g_compliance = w["compliance"] + ops.elastic_directional_bwd(compliance, flags, dirs, w["young"], w["compressibility"],
                                                                 g_ext_d, arg_d)
    g_props = torch.stack([w[n] for n in PROPS], 1)
    return ops.elastic_props_bwd(voigt, compliance, props, flags, g_props, g_voigt, g_compliance, 1, dtype)


def test_wiring_is_bitwise_the_three_adjoints_called_by_hand():
    from matten_amd import elastic, ops
    from test_gpu_elastic_grad import example_irreps

    D, B = 65, 6
    rho, nd = torch.tensor(densities(B)).to(DEV), torch.tensor(5e28 + 1e28 * np.arange(B)).to(DEV)
    c = torch.tensor(generic_tensors(2), device=DEV, requires_grad=True)
    kw = dict(directions=D, density=rho, number_density=nd, keep_directional=True)
    p = elastic.elastic_moduli(c, **kw)
    q = elastic.elastic_properties(c.detach(), **kw)
    for n in SCALARS + PROPS:
        assert getattr(p, n).grad_fn is not None and getattr(q, n).grad_fn is None, n
        assert torch.equal(getattr(p, n).detach(), getattr(q, n)), n
    for n in INTEGERS + ("is_stable", "is_singular", "directions"):
        assert not getattr(p, n).requires_grad and torch.equal(getattr(p, n), getattr(q, n)), n
    assert not p.flags.any() and not p.acoustic_unstable_directions.any()
    w = loss_weights(p, SCALARS + PROPS)
    sum((getattr(p, n) * w[n]).sum() for n in SCALARS + PROPS).backward()
    want = by_hand(c.detach().reshape(B, 36), torch.float64, p.directions, rho, nd, w)
    assert c.grad.shape == (B, 6, 6) and torch.isfinite(c.grad).all() and c.grad.abs().max() > 0
    assert torch.equal(c.grad.reshape(B, 36), want)
    # the defaults: no directional field, the graph of before
    p0 = elastic.elastic_moduli(c)
    assert not p0.has_directions and not hasattr(p0, "young_max") and not hasattr(p0, "v_mean")
    # an unbatched tensor
    one = elastic.elastic_moduli(c[0], directions=D, density=float(rho[0]), number_density=float(nd[0]), keep_directional=True)
    assert one.young.shape == (D,) and one.velocities.shape == (D, 3) and one.debye_temperature.shape == ()
    assert one.directions.shape == (D, 3) and one.debye_temperature.item() == p.debye_temperature[0].item()
    # unused outputs reach the kernels as null pointers: a loss on one extreme alone
    c2 = c.detach().clone().requires_grad_()
    elastic.elastic_moduli(c2, directions=D, density=rho).v_fast_max.sum().backward()
    assert torch.isfinite(c2.grad).all() and c2.grad.abs().max() > 0

    # ---- the irreps route: fp32 rows in, fp32 gradient out
    x0, _ = example_irreps(B)
    x = x0.to(DEV).requires_grad_()
    p = elastic.elastic_moduli_from_irreps(x, **kw)
    q = elastic.elastic_properties_from_irreps(x.detach(), **kw)
    for n in SCALARS + PROPS:
        assert torch.equal(getattr(p, n).detach(), getattr(q, n)), n
    for n in INTEGERS:
        assert torch.equal(getattr(p, n), getattr(q, n)), n
    assert not p.flags.any() and not p.acoustic_unstable_directions.any()
    sum((getattr(p, n) * w[n]).sum() for n in SCALARS + PROPS).backward()
    Q = torch.tensor(elastic.voigt_basis(), dtype=torch.float32, device=DEV)
    g_rows = by_hand(ops.dense_rows(x.detach(), Q), torch.float32, p.directions, rho, nd, w)
    assert x.grad.dtype == torch.float32 and x.grad.shape == (B, 21)
    assert torch.equal(x.grad, ops.dense_rows(g_rows, Q.t().contiguous()))


# ---------------------------------------------------------------------------------------------------
# 6. end to end: a model trained on acoustic data
# ---------------------------------------------------------------------------------------------------
A_SCALE = 100.0      # as tests/test_gpu_elastic_grad.py: a perturbation of ~4 GPa around the example tensors
# standard atomic weights (u) of the species in the first eight example structures
ATOMIC_WEIGHT = {3: 6.94, 7: 14.007, 8: 15.999, 13: 26.982, 14: 28.085, 21: 44.956, 25: 54.938, 29: 63.546, 30: 65.38, 31: 69.723,
                 33: 74.922, 40: 91.224, 45: 102.906, 48: 112.414, 49: 114.818, 56: 137.327, 58: 140.116, 59: 140.908, 66: 162.500,
                 76: 190.23, 79: 196.967}
AMU = 1.66053906660e-27


def example_densities(golden_dir, n):
    """(kg/m^3 [n], atoms/m^3 [n]) of the first n example structures, from their cells"""
    from oracle.matten_ref.data import structures_from_json

    structs = structures_from_json(os.path.join(golden_dir, "example_crystal_elasticity_tensor_n100.json"))[:n]
    volume = np.array([abs(np.linalg.det(np.array(s["lattice"], dtype=np.float64))) for s in structs]) * 1e-30
    mass = np.array([sum(ATOMIC_WEIGHT[int(z)] for z in s["atomic_numbers"]) for s in structs]) * AMU
    count = np.array([len(s["atomic_numbers"]) for s in structs], dtype=np.float64)
    return mass / volume, count / volume


def oracle_fields(rows, dirs, rho, nd):
    """the three trained quantities by the reference formulas (torch fp64, differentiable) from Voigt rows [B,36]"""
    from matten_amd.elastic import HBAR, K_B

    c = rows.reshape(-1, 6, 6)
    s = torch.linalg.inv(0.5 * (c + c.transpose(1, 2)))
    E, _ = ref_directional(s, dirs)
    vel, ok, _ = ref_acoustic(c, rho, dirs)
    v_mean = ((vel ** -3.0).sum(dim=(1, 2)) / (3.0 * dirs.shape[0])) ** (-1.0 / 3.0)
    theta = (HBAR / K_B) * (6.0 * np.pi ** 2 * nd) ** (1.0 / 3.0) * v_mean
    return dict(debye_temperature=theta, young_max=E.max(dim=1).values, v_fast_max=vel[:, :, 2].max(dim=1).values), ok


def test_model_trained_on_acoustic_data_matches_the_oracle_and_three_steps_lower_the_loss(golden_dir):
    from common import LMAX2, build_pair
    from matten_amd import elastic
    from matten_amd.data.graph import collate
    from matten_amd.model import freeze_batchnorm
    from matten_amd.optim import FlatAdam
    from test_gpu_elastic_grad import example_irreps
    from test_gpu_radial_depth import _close
    from test_gpu_training import _graphs

    n, D = 8, 16
    names = ("debye_temperature", "young_max", "v_fast_max")
    graphs, ds = _graphs(golden_dir, n)
    ref, model = build_pair(LMAX2, ds, randomize_bn=True)
    x0, V = example_irreps(n)
    rho_n, nd_n = example_densities(golden_dir, n)
    assert (rho_n > 1500).all() and (rho_n < 25000).all() and (nd_n > 2e28).all() and (nd_n < 2e29).all()
    rho, nd, dirs = torch.tensor(rho_n), torch.tensor(nd_n), fib(D)
    with torch.no_grad():
        targets, ok0 = oracle_fields(x0.double() @ V, dirs, rho, nd)          # the example set's own values
    assert ok0.all()
    loss_fn = elastic.ModuliLoss(names=names)

    # ---- the oracle: eval mode (frozen statistics), fp32 model, the properties in fp64 by the reference formulas
    ref.eval()
    rows = ((A_SCALE * ref.decode(collate(graphs)) + x0) @ V.float()).double()
    fields, ok = oracle_fields(rows, dirs, rho, nd)
    assert ok.all() and all(torch.isfinite(v).all() for v in fields.values())      # no entry is excluded
    loss_r = loss_fn(elastic.ElasticProperties(flags=torch.zeros(n, dtype=torch.int32), **fields), targets)
    loss_r.backward()
    grads_r = {k: p.grad.clone() for k, p in ref.named_parameters() if p.grad is not None}
    assert loss_r.item() > 0 and any(g.abs().max() > 0 for g in grads_r.values())

    # ---- the product
    freeze_batchnorm(model).train()
    batch = collate(graphs, device=DEV)
    targets_d = {k: v.to(DEV) for k, v in targets.items()}
    rho_d, nd_d = rho.to(DEV), nd.to(DEV)

    def loss_of():
        x = model(dict(batch))[0]["elastic_tensor_full"]
        p = elastic.elastic_moduli_from_irreps(A_SCALE * x + x0.to(DEV), directions=D, density=rho_d, number_density=nd_d)
        return loss_fn(p, targets_d), p

    model.zero_grad(set_to_none=True)
    loss_m, p = loss_of()
    assert not p.flags.any() and not p.acoustic_unstable_directions.any()
    assert all(torch.isfinite(getattr(p, k)).all() for k in names)
    loss_m.backward()
    print(f"acoustic loss: product {loss_m.item():.6f} oracle {loss_r.item():.6f}")
    assert abs(loss_m.item() - loss_r.item()) <= 2e-3 * abs(loss_r.item())
    named = dict(model.named_parameters())
    worst = 0.0
    for k, g in grads_r.items():
        assert named[k].grad is not None, k
        _close(named[k].grad, g, 3e-3, f"acoustic loss: grad {k}")
        worst = max(worst, (named[k].grad.cpu().double() - g.double()).abs().max().item() / max(1e-12, g.abs().max().item()))
    print(f"acoustic loss: worst gradient error / tensor scale {worst:.2e} (allowed 3e-3)")

    # ---- three FlatAdam steps lower the loss, everything stays finite
    opt = FlatAdam(model.parameters(), lr=1e-3)
    losses = [loss_m.item()]
    for _ in range(3):
        opt.zero_grad()
        loss, _ = loss_of()
        loss.backward()
        opt.step()
    with torch.no_grad():
        last, p = loss_of()
    losses.append(last.item())
    print(f"acoustic loss: {losses[0]:.5f} -> {losses[1]:.5f} after three FlatAdam steps")
    assert losses[1] < losses[0]
    assert all(torch.isfinite(q).all() for q in model.parameters())
    assert all(torch.isfinite(getattr(p, k)).all() for k in names)


# ---------------------------------------------------------------------------------------------------
# the CPU measurement behind REF_DIR / REF_AC (no GPU): python tests/test_gpu_elastic_dir_grad.py
# ---------------------------------------------------------------------------------------------------
def measure_reference():
    worst_d, worst_a = (0.0, None), (0.0, None)
    for seed in SEEDS:
        for D in D_SET:
            cd, ca = dir_case(seed, D), ac_case(seed, D)
            for mode in DIR_MODES:
                ups, want, absum = cd["modes"][mode]
                u = error_in_units(ref_directional_grad(cd["s"], cd["dirs"], *ups, cd["arg"]).numpy(), want, absum).max()
                worst_d = max(worst_d, (u, f"{mode}, seed {seed}, D = {D}"))
            for mode in AC_MODES:
                ups, want, absum = ca["modes"][mode]
                u = error_in_units(ref_acoustic_grad(ca["c"], ca["rho"], ca["dirs"], *ups, ca["arg"]).numpy(), want, absum).max()
                worst_a = max(worst_a, (u, f"{mode}, seed {seed}, D = {D}"))
    # test 2's input (the sum of v^-3 alone) and test 3's indefinite rows
    c, rho, dirs = degenerate_inputs()
    gx = torch.zeros(2, 3, dtype=torch.float64)
    gx[:, 2] = SUM_SCALE
    vel, _, _ = ref_acoustic(c, rho, dirs)
    arg = torch.stack([vel[:, :, 0].argmin(1), vel[:, :, 2].argmax(1)], 1).int()
    want, absum, _, _ = arb_acoustic(c, rho, dirs, None, gx, arg)
    u = error_in_units(ref_acoustic_grad(c, rho, dirs, None, gx, arg).numpy(), want, absum).max()
    worst_a = max(worst_a, (u, "sum, degenerate modes"))
    c, rho, _, dirs, kinds = excluded_acoustic_batch()
    one = slice(kinds.index("indef"), kinds.index("indef") + 1)
    gv, gx = ac_upstream("all", 3, 65, len(kinds))
    vel, ok, _ = ref_acoustic(c[one], rho[one], dirs)
    assert 0 < int((~ok).sum()) < 65
    v0, v2 = torch.nan_to_num(vel[:, :, 0], nan=float("inf")), torch.nan_to_num(vel[:, :, 2], nan=-float("inf"))
    arg = torch.stack([v0.argmin(1), v2.argmax(1)], 1).int()
    want, absum, _, _ = arb_acoustic(c[one], rho[one], dirs, gv[one], gx[one], arg)
    u = error_in_units(ref_acoustic_grad(c[one], rho[one], dirs, gv[one], gx[one], arg).numpy(), want, absum).max()
    indef_a = u
    s = torch.tensor(np.linalg.inv(indefinite_tensor()))[None]
    dirs = fib(65)
    gy, gb, gx = (t[3:4] for t in dir_upstream("all", 3, 65, 5))
    E, beta = ref_directional(s, dirs)
    arg = torch.stack([E.argmin(1), E.argmax(1), beta.argmin(1), beta.argmax(1)], 1).int()
    want, absum = arb_directional(s, dirs, gy, gb, gx, arg)
    u = error_in_units(ref_directional_grad(s, dirs, gy, gb, gx, arg).numpy(), want, absum).max()
    print(f"REF_DIR = {worst_d[0]:.4f} ({worst_d[1]})\nREF_AC = {worst_a[0]:.4f} ({worst_a[1]})\n"
          f"the indefinite rows of test 3: REF_DIR_INDEF = {u:.4f}, REF_AC_INDEF = {indef_a:.4f}")


if __name__ == "__main__":
    measure_reference()
