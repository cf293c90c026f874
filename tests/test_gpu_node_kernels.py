"""
The node-wise training kernels (csrc/backward.hip, csrc/node.hip), each on its own against fp64 autograd of the oracle's
module, per irrep block over the whole batch:

    matten_gate_bwd                 GateFn            oracle ActivationLayer("gate") without normalisation
    matten_norm_act / _bwd          NormActFn         oracle ActivationLayer("norm") = e3nn NormActivation
    matten_instance_norm_fwd/_bwd   InstanceNormFn    oracle InstanceNorm, crystals of [1, 2, 0, 7, 1000, 64, 1] atoms
    matten_segment_reduce(_bwd)     SegmentReduceFn   index_add_ (the oracle's scatter), segments [0, 1, 7, 8, 9, 64, 1000]
    matten_segment_minmax(_bwd)     SegmentMinMaxFn   exact: amin / amax, first index of the extreme, scatter of dy
    matten_gather_scale             ops.gather_scale  exact: src[idx] * scale[...], one multiply
(the one-workgroup-per-channel BatchNorm below 2048 rows: test_batchnorm_training_reductions_at_large_row_counts in
tests/test_gpu_training.py, whose row counts now start at 1.)

Every case runs twice (bit-identical) and once with torch.empty / torch.empty_like handing out NaN-filled buffers, which
must leave no NaN in any result: gate_bwd and norm_act_bwd allocate dx with empty_like on the claim that every input
column is written.

Bounds.  Each is 4 x the worst error of an fp32 torch evaluation of the same reference expression against its fp64
evaluation on this file's inputs (worst over the cases, relative to the largest |reference| of the irrep block compared,
taken over the whole batch); the factor covers another summation order and FMA contraction, not other arithmetic.  A block
whose reference is identically 0 must be exactly 0.  `python tests/test_gpu_node_kernels.py` prints the fp32-torch errors
(CPU only); they differ a little between ATen's CPU code paths (ATEN_CPU_CAPABILITY = default / avx2 / avx512), CONSTANTS
holds the largest figure over them, rounded up.
    fp32 torch vs fp64, worst:  gate y 1.90e-7 dx 2.85e-7   norm activation y 1.44e-7 dx 2.94e-7   segment sum / mean 1.25e-6
                                instance norm y 1.10e-6 dx 1.19e-6 dweight 3.46e-6 dbias 1.21e-7
Worst error / allowed of the kernels, measured on MI355X:
    gate y 0.25 dx 0.25   norm activation y 0.28 dx 0.25   segment sum / mean 0.19
    instance norm y 0.044 dx 0.36 dweight 0.015 dbias 0.15

Planted inputs.  Gate: exact zeros in every `abs` gate column of one row (37 and 1030 rows), +-25 and +-90 in every scalar
and gate column of four rows (1030 rows only, so that the 37-row blocks keep the scale of ordinary values): the ssp v > 20
branch, expf overflow in silu / sigmoid.  The "odd_gates" layout has no path to 0e, so its gates are 0o: the only way to
the `abs` (ActivationLayer defaults) and `tanh` (conv defaults) gate activations; with it the two activation sets reach the
codes 1-5.  A single row keeps |x| >= 0.25 (ssp cancels near 0 in the reference as well, and one value would be the whole
block's scale).  NormActivation: silu -- an all-zero row, a row of channel norms 3e-8 (above epsilon = 1e-8) and one of 1e-9
(below); ssp -- norms kept >= 1.5e-2 (log1p(e^n) - ln 2 cancels in fp32 in the reference as well) and one all-zero row, for
which y == 0 exactly and dx finite are asserted and nothing else.
"""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from test_gpu_edge_geom import nan_filled_empty  # noqa: E402
from test_gpu_eval_grad import LAYOUTS, _blocks, _chan_blocks, _per_block  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# fp32 torch vs fp64, worst error / block scale (module docstring); the bounds are 4 x these
CONSTANTS = {
    "gate_y": 1.90e-7, "gate_dx": 2.85e-7,
    "norm_y": 1.44e-7, "norm_dx": 2.94e-7,
    "inorm_y": 1.10e-6, "inorm_dx": 1.19e-6, "inorm_dweight": 3.46e-6, "inorm_dbias": 1.21e-7,
    "segsum": 1.25e-6,
}
RTOL = {k: 4 * v for k, v in CONSTANTS.items()}

GATE_LAYOUTS = dict(LAYOUTS, odd_gates=("4x0o+3x1e", "0e+1o", "4x0o+3x1e+2x1o"))
ACT_SETS = {
    "conv": ({"e": "silu", "o": "tanh"}, {"e": "sigmoid", "o": "tanh"}),   # PointConvWithActivation's defaults
    "layer": (None, None),                                                 # ActivationLayer's: ssp / tanh, ssp / abs
}
ROWS = (1, 37, 1030)
BIG = (25.0, -25.0, 90.0, -90.0)
ONE_ROW_MIN = 0.25
GATE_CASES = [(layout, acts, n) for layout in GATE_LAYOUTS for acts in ACT_SETS for n in ROWS]
NORM_CASES = [(layout, act, n) for layout in LAYOUTS for act in ("silu", "ssp") for n in ROWS]
NORM_EPS = 1e-8
SSP_MIN_NORM = 1.5e-2

IN_IRREPS = "8x0e+4x0o+5x1o+3x2e"
IN_SIZES = [1, 2, 0, 7, 1000, 64, 1]
IN_SCALAR_COLS = 12            # 8x0e + 4x0o: every l = 0 channel is centred and biased
POOL_SEGMENTS = [0, 1, 7, 8, 9, 64, 1000]
POOL_WIDTHS = (1, 21, 42)
POOL_CASES = [(w, mean) for w in POOL_WIDTHS for mean in (False, True)]
MINMAX_CASES = [(w, take_max) for w in POOL_WIDTHS for take_max in (False, True)]
GS_PERIOD = 37
GS_CASES = ([(n, p, by_src, False) for n, p in ((1, 7), (255, 7), (257, 7), (4 * GS_PERIOD, GS_PERIOD)) for by_src in (False, True)]
            + [(n, p, by_src, True) for n, p in ((1, 1), (255, 51), (257, 257), (4 * GS_PERIOD, GS_PERIOD)) for by_src in (False, True)])


def _rel(err, scale):
    return err / scale if scale else (0.0 if err == 0 else math.inf)


def _block_errors(got, want, blocks):
    """worst max |got - want| / max |want| over the blocks (columns lo:hi of the last axis)"""
    got, want = got.detach().double(), want.detach().double()
    return max([_rel((got[..., lo:hi] - want[..., lo:hi]).abs().max().item(), want[..., lo:hi].abs().max().item())
                for lo, hi, _ in blocks] + [0.0])


def _ptr_batch(sizes):
    ptr = torch.tensor([0] + sizes).cumsum(0)
    return ptr, torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))


# ---------------------------------------------------------------------------------------------------------------------
# Gate
# ---------------------------------------------------------------------------------------------------------------------
def _act_kwargs(acts):
    scal, gat = ACT_SETS[acts]
    return {} if scal is None else dict(activation_scalars=scal, activation_gates=gat)


def _gate_columns(layout, acts):
    """(scalar input columns, gate input columns, `abs` gate input columns) of the layer's input layout"""
    from matten_amd.nn.utils import ActivationLayer
    from matten_amd.plan import ACT_CODE

    meta = ActivationLayer(*GATE_LAYOUTS[layout], activation_type="gate", **_act_kwargs(acts)).plan.meta
    scal = sorted({int(r[0]) for r in meta if r[1] < 0})
    gates = sorted({int(r[1]) for r in meta if r[1] >= 0})
    abs_gates = sorted({int(r[1]) for r in meta if r[1] >= 0 and ((int(r[2]) >> 8) & 0xff) == ACT_CODE["abs"]})
    return scal, gates, abs_gates


def _gate_inputs(case):
    from oracle.matten_ref import nn as rnn

    layout, acts, n = case
    gen = torch.Generator().manual_seed(8000 + GATE_CASES.index(case))
    ref = rnn.ActivationLayer(*GATE_LAYOUTS[layout], activation_type="gate", **_act_kwargs(acts))
    x = torch.randn(n, ref.irreps_in.dim, generator=gen) * 1.5
    dy = torch.randn(n, ref.irreps_out.dim, generator=gen)
    scal, gates, abs_gates = _gate_columns(layout, acts)
    planted = dict(abs_zero_rows=[], big_rows=[])
    if n == 1:   # one row is all a block has: ssp(v) = log1p(e^v) - ln 2 cancels near 0 in fp32 in the reference as well,
        x = torch.where(x.abs() < ONE_ROW_MIN, ONE_ROW_MIN * torch.where(x < 0, -1.0, 1.0), x)   # and would be its own scale
    if n >= 37 and abs_gates:
        x[2, abs_gates] = 0.0
        planted["abs_zero_rows"] = [2]
    if n >= 1030:
        for r, v in zip((3, 4, 5, 6), BIG):
            x[r, scal] = v
            x[r, gates] = -v
        planted["big_rows"] = [3, 4, 5, 6]
    return dict(name="-".join(map(str, case)), ref=ref, x=x, dy=dy, scal=scal, gates=gates, abs_gates=abs_gates, planted=planted)


def _module_reference(mod, x, dy, dtype):
    """(y, dx) of L = <dy, mod(x)> by autograd in `dtype`"""
    xr = x.to(dtype).clone().requires_grad_(True)
    y = mod(xr)
    return y.detach(), torch.autograd.grad((y * dy.to(dtype)).sum(), xr)[0].detach()


def _runs(run, monkeypatch):
    """run() twice and once on NaN-filled torch.empty: the three results are the same bits and hold no NaN"""
    first, second = run(), run()
    with monkeypatch.context() as m:
        nan_filled_empty(m)
        assert torch.isnan(torch.empty(4, device=DEV)).all() and torch.isnan(torch.empty_like(first[0])).all()
        third = run()
        torch.cuda.synchronize()
    for a, b, c in zip(first, second, third):
        assert not torch.isnan(c).any(), "a NaN of the uninitialised buffers survived"
        assert torch.equal(a, b) and torch.equal(a, c), "not bitwise repeatable"
    return first


def _apply_and_grad(fn, x, dy):
    xd = x.to(DEV).requires_grad_(True)
    y = fn(xd)
    y.backward(dy.to(DEV))
    return y.detach(), xd.grad


@pytest.mark.parametrize("case", GATE_CASES, ids=["-".join(map(str, c)) for c in GATE_CASES])
def test_gate_adjoint_matches_fp64_autograd(case, monkeypatch):
    from matten_amd import autograd as ag
    from matten_amd.nn.utils import ActivationLayer

    d = _gate_inputs(case)
    mod = ActivationLayer(*GATE_LAYOUTS[case[0]], activation_type="gate", **_act_kwargs(case[1]))
    assert mod.irreps_in.dim == d["ref"].irreps_in.dim and mod.irreps_out.dim == d["ref"].irreps_out.dim
    y_ref, dx_ref = _module_reference(d["ref"], d["x"], d["dy"], torch.float64)
    y, dx = _runs(lambda: _apply_and_grad(lambda t: ag.GateFn.apply(t, mod), d["x"], d["dy"]), monkeypatch)
    assert torch.isfinite(y).all() and torch.isfinite(dx).all()
    e_y = _per_block(y, y_ref, _blocks(mod.irreps_out), RTOL["gate_y"], f"gate {d['name']} y")
    e_dx = _per_block(dx, dx_ref, _blocks(mod.irreps_in), RTOL["gate_dx"], f"gate {d['name']} dx")
    print(f"\nNODE_KERNELS gate {d['name']} y {e_y / RTOL['gate_y']:.3g} dx {e_dx / RTOL['gate_dx']:.3g}")
    for r in d["planted"]["abs_zero_rows"]:
        assert (dx[r, d["abs_gates"]] == 0).all(), "abs at 0: derivative 0 on both sides"


# ---------------------------------------------------------------------------------------------------------------------
# NormActivation (training form, no BatchNorm)
# ---------------------------------------------------------------------------------------------------------------------
def _norm_channels(layout):
    from matten_amd.nn.utils import ActivationLayer

    mod = ActivationLayer(*LAYOUTS[layout], activation_type="norm", activation_scalars={"e": "silu", "o": "tanh"})
    return [(int(c[0]), int(c[1])) for c in mod.plan.chan]


def _norm_inputs(case):
    from oracle.matten_ref import nn as rnn

    layout, act, n = case
    gen = torch.Generator().manual_seed(9000 + NORM_CASES.index(case))
    ref = rnn.ActivationLayer(*LAYOUTS[layout], activation_type="norm", activation_scalars={"e": act, "o": "tanh"})
    chans = _norm_channels(layout)
    x = torch.randn(n, ref.irreps_in.dim, generator=gen) * 1.5
    dy = torch.randn(n, ref.irreps_out.dim, generator=gen)

    def set_norms(row, value):
        for off, dim in chans:
            x[row, off:off + dim] *= value / x[row, off:off + dim].norm()

    rows = dict(zero=[], above=[], below=[])
    if act == "ssp":
        for off, dim in chans:
            nrm = x[:, off:off + dim].norm(dim=1, keepdim=True)
            x[:, off:off + dim] *= torch.where(nrm < SSP_MIN_NORM, SSP_MIN_NORM / nrm, torch.ones_like(nrm))
    if n >= 37:
        x[1] = 0.0
        rows["zero"] = [1]
        if act == "silu":
            set_norms(2, 3e-8)
            set_norms(3, 1e-9)
            rows["above"], rows["below"] = [2], [3]
    compared = torch.ones(n, dtype=torch.bool)
    if act == "ssp":
        compared[rows["zero"]] = False
    return dict(name="-".join(map(str, case)), ref=ref, x=x, dy=dy, chans=chans, rows=rows, compared=compared)


@pytest.mark.parametrize("case", NORM_CASES, ids=["-".join(map(str, c)) for c in NORM_CASES])
def test_norm_activation_adjoint_matches_fp64_autograd(case, monkeypatch):
    from matten_amd import autograd as ag
    from matten_amd.nn.utils import ActivationLayer

    d = _norm_inputs(case)
    mod = ActivationLayer(*LAYOUTS[case[0]], activation_type="norm", activation_scalars={"e": case[1], "o": "tanh"})
    assert mod.irreps_in.dim == d["ref"].irreps_in.dim and mod.plan.epsilon == NORM_EPS
    y_ref, dx_ref = _module_reference(d["ref"], d["x"], d["dy"], torch.float64)
    y, dx = _runs(lambda: _apply_and_grad(lambda t: ag.NormActFn.apply(t, mod), d["x"], d["dy"]), monkeypatch)
    assert torch.isfinite(y).all() and torch.isfinite(dx).all()
    ok = d["compared"]
    e_y = _per_block(y.cpu()[ok], y_ref[ok], _blocks(mod.irreps_out), RTOL["norm_y"], f"norm {d['name']} y")
    e_dx = _per_block(dx.cpu()[ok], dx_ref[ok], _blocks(mod.irreps_in), RTOL["norm_dx"], f"norm {d['name']} dx")
    print(f"\nNODE_KERNELS norm {d['name']} y {e_y / RTOL['norm_y']:.3g} dx {e_dx / RTOL['norm_dx']:.3g}")
    for r in d["rows"]["zero"]:
        assert (y[r] == 0).all(), "an all-zero row stays zero"


# ---------------------------------------------------------------------------------------------------------------------
# instance normalisation
# ---------------------------------------------------------------------------------------------------------------------
def _inorm_inputs():
    from oracle.e3nn_lite.o3 import Irreps

    gen = torch.Generator().manual_seed(9500)
    irreps = Irreps(IN_IRREPS)
    ptr, batch = _ptr_batch(IN_SIZES)
    n = int(ptr[-1])
    x = torch.randn(n, irreps.dim, generator=gen)
    x[:, :8] += 5.0
    dy = torch.randn(n, irreps.dim, generator=gen)
    weight = 0.5 + torch.rand(irreps.num_irreps, generator=gen)
    bias = torch.randn(IN_SCALAR_COLS, generator=gen)
    return dict(irreps=irreps, ptr=ptr, batch=batch, x=x, dy=dy, weight=weight, bias=bias,
                lone_rows=[int(ptr[i]) for i, s in enumerate(IN_SIZES) if s == 1])


def _inorm_reference(d, dtype):
    """(y, dx, dweight, dbias) of L = <dy, InstanceNorm(x)> by autograd in `dtype`"""
    from oracle.matten_ref.nn import InstanceNorm

    ref = InstanceNorm(IN_IRREPS).to(dtype)
    with torch.no_grad():
        ref.weight.copy_(d["weight"]), ref.bias.copy_(d["bias"])
    x = d["x"].to(dtype).clone().requires_grad_(True)
    y = ref(x, d["batch"])
    gx, gw, gb = torch.autograd.grad((y * d["dy"].to(dtype)).sum(), (x, ref.weight, ref.bias))
    return y.detach(), gx.detach(), gw.detach(), gb.detach()


def _inorm_blocks(irreps):
    scalars = [(lo, hi, name) for (lo, hi, name), (_, ir) in zip(_chan_blocks(irreps), irreps) if ir.l == 0]
    return _blocks(irreps), _chan_blocks(irreps), scalars


def test_instance_norm_matches_fp64_autograd(monkeypatch):
    from matten_amd import autograd as ag
    from matten_amd.nn.utils import _IrrepInstanceNorm
    from matten_amd.o3 import Irreps

    d = _inorm_inputs()
    y_ref, dx_ref, dw_ref, db_ref = _inorm_reference(d, torch.float64)
    norm = _IrrepInstanceNorm(Irreps(IN_IRREPS)).to(DEV)
    with torch.no_grad():
        norm.weight.copy_(d["weight"]), norm.bias.copy_(d["bias"])
    ptr, batch = d["ptr"].to(DEV), d["batch"].to(DEV)

    def run():
        norm.weight.grad = norm.bias.grad = None
        y, dx = _apply_and_grad(lambda t: ag.InstanceNormFn.apply(t, norm.weight, norm.bias, norm, ptr, batch), d["x"], d["dy"])
        return y, dx, norm.weight.grad.clone(), norm.bias.grad.clone()

    y, dx, dw, db = _runs(run, monkeypatch)
    blocks, chans, scalars = _inorm_blocks(d["irreps"])
    assert scalars[-1][1] == IN_SCALAR_COLS == db.numel()
    e = [_per_block(y, y_ref, blocks, RTOL["inorm_y"], "instance norm y") / RTOL["inorm_y"],
         _per_block(dx, dx_ref, blocks, RTOL["inorm_dx"], "instance norm dx") / RTOL["inorm_dx"],
         _per_block(dw, dw_ref, chans, RTOL["inorm_dweight"], "instance norm dweight") / RTOL["inorm_dweight"],
         _per_block(db, db_ref, scalars, RTOL["inorm_dbias"], "instance norm dbias") / RTOL["inorm_dbias"]]
    print("\nNODE_KERNELS instance norm y {:.3g} dx {:.3g} dweight {:.3g} dbias {:.3g}".format(*e))
    for r in d["lone_rows"]:   # a crystal of one atom: its scalars are their own mean
        assert (dx_ref[r, :IN_SCALAR_COLS] == 0).all() and (dx[r, :IN_SCALAR_COLS] == 0).all()
        assert torch.equal(y[r, :IN_SCALAR_COLS].cpu(), d["bias"])


# ---------------------------------------------------------------------------------------------------------------------
# pooling
# ---------------------------------------------------------------------------------------------------------------------
def _pool_inputs(width):
    gen = torch.Generator().manual_seed(9600 + width)
    ptr, batch = _ptr_batch(POOL_SEGMENTS)
    x = torch.randn(int(ptr[-1]), width, generator=gen)
    dy = torch.randn(len(POOL_SEGMENTS), width, generator=gen)
    return dict(ptr=ptr, batch=batch, x=x, dy=dy)


def _segment_reference(d, mean, dtype):
    """the oracle's scatter (index_add_ in row order), `mean` divides by max(count, 1)"""
    from oracle.e3nn_lite.scatter import scatter

    return scatter(d["x"].to(dtype), d["batch"], dim=0, dim_size=len(POOL_SEGMENTS), reduce="mean" if mean else "sum")


@pytest.mark.parametrize("case", POOL_CASES, ids=[f"w{w}-{'mean' if m else 'sum'}" for w, m in POOL_CASES])
def test_segment_reduce_and_adjoint(case, monkeypatch):
    from matten_amd import autograd as ag

    width, mean = case
    d = _pool_inputs(width)
    ptr = d["ptr"].to(DEV)
    out, dx = _runs(lambda: _apply_and_grad(lambda t: ag.SegmentReduceFn.apply(t, ptr, mean), d["x"], d["dy"]), monkeypatch)
    ref = _segment_reference(d, mean, torch.float64)
    assert out.shape == ref.shape and (out[0] == 0).all() and (ref[0] == 0).all(), "the empty segment gives 0"
    err, scale = (out.cpu().double() - ref).abs().max().item(), ref.abs().max().item()
    print(f"\nNODE_KERNELS segment_reduce {case} {err / (RTOL['segsum'] * scale):.3g}")
    assert err <= RTOL["segsum"] * scale, f"segment_reduce {case}: err {err:.3e} vs scale {scale:.3e}"
    # the adjoint is one division per element
    count = torch.tensor(POOL_SEGMENTS, dtype=torch.float64).clamp(min=1)
    want = d["dy"].double()[d["batch"]] / (count[d["batch"]][:, None] if mean else 1.0)
    assert dx.shape == want.shape
    assert ((dx.cpu().double() - want).abs() <= 2.0 ** -22 * want.abs()).all()


def _minmax_inputs(width):
    """ties in column 0: +10 twice and -10 twice in the 7-row segment; -0.0 before 0.0 as the minimum of the 8-row
    segment; 0.0 before -0.0 as the maximum of the 9-row segment"""
    gen = torch.Generator().manual_seed(9700 + width)
    ptr, batch = _ptr_batch(POOL_SEGMENTS)
    x = torch.randn(int(ptr[-1]), width, generator=gen)
    dy = torch.randn(len(POOL_SEGMENTS), width, generator=gen)
    s7, s8, s9 = int(ptr[2]), int(ptr[3]), int(ptr[4])
    x[s7 + 1, 0] = x[s7 + 4, 0] = 10.0
    x[s7 + 2, 0] = x[s7 + 5, 0] = -10.0
    x[s8:s8 + 8, 0] = 1.0 + torch.rand(8, generator=gen)
    x[s8 + 1, 0], x[s8 + 4, 0] = -0.0, 0.0
    x[s9:s9 + 9, 0] = -1.0 - torch.rand(9, generator=gen)
    x[s9 + 2, 0], x[s9 + 5, 0] = 0.0, -0.0
    ties = {(2, True): s7 + 1, (2, False): s7 + 2, (3, False): s8 + 1, (4, True): s9 + 2}   # (segment, take_max) -> first row
    return dict(ptr=ptr, batch=batch, x=x, dy=dy, ties=ties)


def _minmax_reference(d, take_max):
    """(values, first row of the extreme) per segment and column; the empty segment gives 0 and -1"""
    x, ptr = d["x"], d["ptr"]
    vals = torch.zeros(len(POOL_SEGMENTS), x.shape[1])
    arg = torch.full((len(POOL_SEGMENTS), x.shape[1]), -1, dtype=torch.int64)
    for b in range(len(POOL_SEGMENTS)):
        lo, hi = int(ptr[b]), int(ptr[b + 1])
        if hi > lo:
            seg = x[lo:hi]
            vals[b] = seg.amax(0) if take_max else seg.amin(0)
            rows = torch.arange(lo, hi)[:, None].expand_as(seg)
            arg[b] = torch.where(seg == vals[b][None], rows, torch.full_like(rows, hi)).amin(0)
    return vals, arg


@pytest.mark.parametrize("case", MINMAX_CASES, ids=[f"w{w}-{'max' if m else 'min'}" for w, m in MINMAX_CASES])
def test_segment_minmax_and_adjoint(case, monkeypatch):
    from matten_amd import autograd as ag, ops

    width, take_max = case
    d = _minmax_inputs(width)
    ptr = d["ptr"].to(DEV)
    vals, arg = _minmax_reference(d, take_max)

    def run():
        out, dx = _apply_and_grad(lambda t: ag.SegmentMinMaxFn.apply(t, ptr, take_max), d["x"], d["dy"])
        out2, got_arg = ops.segment_minmax(d["x"].to(DEV), ptr, take_max, want_arg=True)
        return out, dx, out2, got_arg

    out, dx, out2, got_arg = _runs(run, monkeypatch)
    assert torch.equal(out.cpu(), vals) and torch.equal(out2, out)
    assert torch.equal(got_arg.cpu(), arg)
    assert (out[0] == 0).all() and (got_arg[0] == -1).all(), "the empty segment gives 0 and row -1"
    for (b, mx), row in d["ties"].items():
        if mx == take_max:
            assert int(got_arg[b, 0]) == row, "the first of equal values"
    want = torch.zeros_like(d["x"])
    cols = torch.arange(width)[None].expand_as(arg)
    want[arg[arg >= 0], cols[arg >= 0]] = d["dy"][arg >= 0]
    assert torch.equal(dx.cpu(), want)


# ---------------------------------------------------------------------------------------------------------------------
# gather_scale
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", GS_CASES, ids=[f"n{n}-p{p}-{'src' if s else 'out'}-{'perm2' if q else 'plain'}" for n, p, s, q in GS_CASES])
def test_gather_scale_is_one_multiply(case, monkeypatch):
    from matten_amd import ops

    n, period, by_source, permuted = case
    gen = torch.Generator().manual_seed(9800 + GS_CASES.index(case))
    src = torch.randn(300, generator=gen)
    idx = torch.randint(300, (n // period, period) if permuted else (n,), generator=gen)
    scale = torch.randn(period, generator=gen)
    perm2 = torch.randperm(period, generator=gen) if permuted else None
    flat = idx.reshape(-1)
    want = (src[flat] * scale[(flat if by_source else torch.arange(n)) % period]).reshape(idx.shape)

    def run():
        out = ops.gather_scale(src.to(DEV), idx.to(DEV), scale.to(DEV), by_source, None if perm2 is None else perm2.to(DEV))
        return out if permuted else (out,)

    got = _runs(run, monkeypatch)
    assert torch.equal(got[0].cpu(), want)
    if permuted:
        assert torch.equal(got[1].cpu(), want[:, perm2])


# ---------------------------------------------------------------------------------------------------------------------
# the fp32-torch errors behind the bounds (CPU only)
# ---------------------------------------------------------------------------------------------------------------------
def fp32_torch_errors():
    """worst fp32-torch error / block scale over the cases, keyed like CONSTANTS"""
    from oracle.e3nn_lite.o3 import Irreps

    w = {k: 0.0 for k in CONSTANTS}
    for case in GATE_CASES:
        d = _gate_inputs(case)
        (y32, dx32), (y64, dx64) = (_module_reference(d["ref"], d["x"], d["dy"], t) for t in (torch.float32, torch.float64))
        w["gate_y"] = max(w["gate_y"], _block_errors(y32, y64, _blocks(d["ref"].irreps_out)))
        w["gate_dx"] = max(w["gate_dx"], _block_errors(dx32, dx64, _blocks(d["ref"].irreps_in)))
    for case in NORM_CASES:
        d = _norm_inputs(case)
        (y32, dx32), (y64, dx64) = (_module_reference(d["ref"], d["x"], d["dy"], t) for t in (torch.float32, torch.float64))
        ok = d["compared"]
        w["norm_y"] = max(w["norm_y"], _block_errors(y32[ok], y64[ok], _blocks(d["ref"].irreps_out)))
        w["norm_dx"] = max(w["norm_dx"], _block_errors(dx32[ok], dx64[ok], _blocks(d["ref"].irreps_in)))
    d = _inorm_inputs()
    blocks, chans, scalars = _inorm_blocks(Irreps(IN_IRREPS))
    r32, r64 = _inorm_reference(d, torch.float32), _inorm_reference(d, torch.float64)
    for key, a, b, bl in zip(("inorm_y", "inorm_dx", "inorm_dweight", "inorm_dbias"), r32, r64, (blocks, blocks, chans, scalars)):
        w[key] = _block_errors(a, b, bl)
    for width, mean in POOL_CASES:
        d = _pool_inputs(width)
        r64 = _segment_reference(d, mean, torch.float64)
        w["segsum"] = max(w["segsum"], _rel((_segment_reference(d, mean, torch.float32).double() - r64).abs().max().item(),
                                            r64.abs().max().item()))
    return w


if __name__ == "__main__":
    for k, v in fp32_torch_errors().items():
        print(f"{k}: {v:.2e}")
