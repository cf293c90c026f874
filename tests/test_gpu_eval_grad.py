"""
Backpropagation through eval-mode BatchNorm (fine-tuning with frozen statistics) on the GPU.

Kernel level: matten_gate_bn_eval_bwd / matten_norm_act_bn_eval_bwd through `ops` against fp64 autograd of the oracle's
Gate / NormActivation followed by its BatchNorm in eval mode.  Bounds (fp32 elementwise arithmetic with expf / tanhf /
log1pf, a gate's gradient summed over <= 9 components, parameter gradients summed over up to 9652 x 9 terms in a fixed
order; the constants are those of tests/test_gpu_tp_adjoint.py for the same kind of comparison):
    dx        5e-5 of the largest |reference| of ITS input irrep block
    dweight   2e-5 of the largest of its BatchNorm irrep block, compared as dweight * sqrt(running_var + eps) -- the
              plain sum over rows -- so that the channel with running_var ~ 0 (factor 316) cannot loosen its neighbours
    dbias     2e-5 of the largest of its block
Model level: every parameter gradient of an MSE loss against the oracle's autograd with the oracle's BatchNorm in eval
mode, with the comparison helper and the tolerances of tests/test_gpu_training.py (forward 5e-4, gradients 3e-3 of the
tensor's largest magnitude).

Measured on MI355X, worst error / allowed over all cases: kernel dx 8.1e-7 / 5e-5, dweight 1.4e-6 / 2e-5, dbias 2.9e-7 / 2e-5;
model gradients 2.1e-6 / 3e-3 (norm activation; lmax2 8.8e-7, paper 1.6e-6), the same in eval and in mixed mode.
"""
import pytest
import torch

from common import ATOMIC, LMAX2, PAPER, build_pair
from test_gpu_parity import close_blocks
from test_gpu_training import _close, _graphs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DX_RTOL, DP_RTOL = 5e-5, 2e-5
FWD_RTOL = 2e-5
ACT_SCALARS, ACT_GATES = {"e": "silu", "o": "tanh"}, {"e": "sigmoid", "o": "tanh"}   # the conv layer's defaults

# name -> (tp_irreps_in1, tp_irreps_in2, tp_irreps_out)
LAYOUTS = {
    "lmax2": (LMAX2["conv_layer_irreps"], LMAX2["irreps_edge_sh"], LMAX2["conv_layer_irreps"]),
    "paper": (PAPER["conv_layer_irreps"], PAPER["irreps_edge_sh"], PAPER["conv_layer_irreps"]),
    "ragged": ("3x0e+5x0o+7x1o+3x1e+5x2e", "0e+1o+2e", "3x0e+5x0o+7x1o+1x1e+3x2e+1x2o"),
    "scalars_only": ("5x0e+3x0o", "0e+1o", "5x0e+3x0o"),   # no gated irrep, no gate
}
ROWS = (1, 37, 9652)


def _blocks(irreps):
    out, off = [], 0
    for mul, ir in irreps:
        out.append((off, off + mul * ir.dim, f"{mul}x{ir}"))
        off += mul * ir.dim
    return out


def _chan_blocks(irreps, scalars_only=False):
    out, off = [], 0
    for mul, ir in irreps:
        if scalars_only and not ir.is_scalar():
            continue
        out.append((off, off + mul, f"{mul}x{ir}"))
        off += mul
    return out


def _per_block(got, want, blocks, rtol, what):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite values"
    assert (blocks[-1][1] if blocks else 0) == want.shape[-1], what
    worst = 0.0
    for lo, hi, name in blocks:
        scale = want[..., lo:hi].abs().max().item()
        err = (got[..., lo:hi] - want[..., lo:hi]).abs().max().item()
        assert err <= rtol * scale, f"{what} block {name}: max err {err:.3e} vs block scale {scale:.3e} (allowed {rtol:.0e})"
        worst = max(worst, err / max(scale, 1e-300))
    return worst


def _padded(t):
    """the tensor as a prefix of a NaN buffer: an index past its end reads NaN"""
    buf = torch.full((t.numel() + 16,), float("nan"), dtype=torch.float32, device=DEV)
    buf[: t.numel()] = t.to(DEV)
    return buf[: t.numel()]


def _bn_state(bn_irreps, gen):
    """randomised running statistics and affine; one 0e channel and the last channel have running_var ~ 0"""
    n_feat = bn_irreps.num_irreps
    n_scal = sum(m for m, ir in bn_irreps if ir.is_scalar())
    rm = 0.1 * torch.randn(n_scal, generator=gen)
    rv = 0.5 + torch.rand(n_feat, generator=gen)
    rv[min(1, n_feat - 1)] = 1e-9
    rv[n_feat - 1] = 3e-8
    w = 0.5 + torch.rand(n_feat, generator=gen)
    b = 0.1 * torch.randn(n_scal, generator=gen)
    return rm, rv, w, b


def _oracle(kind, layout, x, dy, state):
    """fp64 autograd of BatchNorm_eval(activation(x)) -> y, dx, dweight, dbias"""
    from oracle.e3nn_lite.nn import BatchNorm
    from oracle.matten_ref import nn as rnn

    act = rnn.ActivationLayer(*LAYOUTS[layout], activation_type=kind, activation_scalars=ACT_SCALARS,
                              activation_gates=ACT_GATES)
    bn = BatchNorm(act.irreps_out).double().eval()
    rm, rv, w, b = state
    with torch.no_grad():
        bn.running_mean.copy_(rm), bn.running_var.copy_(rv), bn.weight.copy_(w), bn.bias.copy_(b)
    x64 = x.double().requires_grad_(True)
    y = bn(act(x64))
    gx, gw, gb = torch.autograd.grad((y * dy.double()).sum(), (x64, bn.weight, bn.bias), allow_unused=True)
    return y.detach(), gx, gw, (gb if gb is not None else torch.zeros_like(bn.bias))


@pytest.mark.parametrize("n_rows", ROWS)
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("kind", ["gate", "norm"])
def test_eval_adjoint_kernels_match_fp64_autograd(kind, layout, n_rows):
    from matten_amd import ops
    from matten_amd.nn.utils import ActivationLayer, _IrrepBatchNorm

    gen = torch.Generator().manual_seed(1000 * n_rows + len(layout) + (7 if kind == "norm" else 0))
    mod = ActivationLayer(*LAYOUTS[layout], activation_type=kind, activation_scalars=ACT_SCALARS, activation_gates=ACT_GATES)
    bn = _IrrepBatchNorm(mod.irreps_out)
    d_in, d_out = mod.irreps_in.dim, mod.irreps_out.dim
    x = torch.randn(n_rows, d_in, generator=gen) * 1.5
    if kind == "norm" and n_rows > 1:
        x[1] = 0.0                       # every channel's norm clamped: a constant, no gradient through it
    dy = torch.randn(n_rows, d_out, generator=gen)
    state = _bn_state(bn.irreps, gen)
    y_ref, dx_ref, dw_ref, db_ref = _oracle(kind, layout, x, dy, state)

    rm, rv, w, b = (_padded(t) for t in state)
    xd, dyd = x.to(DEV), dy.to(DEV)
    n_bias = state[0].numel()
    if kind == "gate":
        meta, cst = mod._tables.get("meta", DEV), mod._tables.get("act_cst", DEV)
        y = ops.gate_bn(xd, meta, cst, rm, rv, w, b, eps=bn.eps)
        run = lambda pg: ops.gate_bn_eval_bwd(xd, meta, cst, bn._tables.get("chan", DEV), rm, rv, w, bn.eps, dyd, n_bias,
                                              param_grads=pg)
    else:
        chan = mod._tables.get("chan", DEV)
        y = ops.norm_act(xd, chan, mod.plan.act_code, mod.plan.epsilon, rm, rv, w, b, bn.eps)
        run = lambda pg: ops.norm_act_bn_eval_bwd(xd, dyd, chan, mod.plan.act_code, mod.plan.epsilon, rm, rv, w, bn.eps,
                                                  n_bias, param_grads=pg)
    dx, dw, db = run(True)
    torch.cuda.synchronize()
    _per_block(y, y_ref, _blocks(mod.irreps_out), FWD_RTOL, f"{kind} {layout} N={n_rows} forward")
    e_dx = _per_block(dx, dx_ref, _blocks(mod.irreps_in), DX_RTOL, f"{kind} {layout} N={n_rows} dx")
    rs = torch.sqrt(state[1].double() + bn.eps)
    e_dw = _per_block(dw.cpu().double() * rs, dw_ref * rs, _chan_blocks(bn.irreps), DP_RTOL, f"{kind} {layout} N={n_rows} dweight")
    assert db.shape == db_ref.shape
    e_db = _per_block(db, db_ref, _chan_blocks(bn.irreps, scalars_only=True), DP_RTOL,
                      f"{kind} {layout} N={n_rows} dbias") if n_bias else 0.0
    print(f"{kind} {layout} N={n_rows}: worst error / block scale  dx {e_dx:.2e}  dweight {e_dw:.2e}  dbias {e_db:.2e}")
    # bitwise reproducible; dx does not depend on whether the parameter gradients are asked for
    dx2, dw2, db2 = run(True)
    dx3, none_w, none_b = run(False)
    assert torch.equal(dx, dx2) and torch.equal(dw, dw2) and torch.equal(db, db2)
    assert torch.equal(dx, dx3) and none_w is None and none_b is None
    # the operands were only read
    for t, ref in zip((rm, rv, w, b), state):
        assert torch.equal(t.cpu(), ref)


# ---- model level -------------------------------------------------------------------------------------------------------
MODELS = {
    "lmax2": (LMAX2, False, 10),
    "paper": (PAPER, False, 6),
    "norm": (dict(LMAX2, nonlinearity_type="norm"), False, 8),
    "atomic": (ATOMIC, True, 8),
    "layers1": (dict(LMAX2, invariant_layers=1), False, 8),
    "layers3": (dict(LMAX2, invariant_layers=3), False, 8),
}
_ORACLE_CACHE = {}


def _set_mode(model, mode):
    from matten_amd.nn.utils import _IrrepBatchNorm

    if mode == "eval":
        return model.eval()
    model.train()                                  # mixed: convolutions and linears train, BatchNorm evaluates
    for m in model.modules():
        if isinstance(m, _IrrepBatchNorm):
            m.eval()
    return model


def _oracle_case(name, golden_dir):
    """(graphs, dataset hparams, target, oracle output, oracle gradients, state_dict) with the oracle's BatchNorm in eval"""
    from matten_amd.data.graph import collate

    if name not in _ORACLE_CACHE:
        hp, atomic, n = MODELS[name]
        graphs, ds = _graphs(golden_dir, n)
        ref, _ = build_pair(hp, ds, randomize_bn=True, device=None, atomic=atomic)
        ref.eval()
        out = ref.decode(collate(graphs))
        target = torch.randn(out.shape, generator=torch.Generator().manual_seed(7))
        torch.nn.functional.mse_loss(out, target).backward()
        grads = {k: p.grad.clone() for k, p in ref.named_parameters() if p.grad is not None}
        _ORACLE_CACHE[name] = (graphs, ds, target, out.detach(), grads, ref)
    return _ORACLE_CACHE[name]


def _product_grads(model, graphs, target, atomic):
    from matten_amd.data.graph import collate

    task = "nmr_tensor" if atomic else "elastic_tensor_full"
    model.zero_grad(set_to_none=True)
    out = model(collate(graphs, device=DEV), task_name=task)[0][task]
    loss = torch.nn.functional.mse_loss(out, target.to(DEV))
    loss.backward()
    return out.detach(), {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("mode", ["eval", "mixed"])
@pytest.mark.parametrize("name", list(MODELS))
def test_eval_mode_gradients_match_oracle_autograd(name, mode, golden_dir):
    hp, atomic, _ = MODELS[name]
    graphs, ds, target, out_r, grads_r, ref = _oracle_case(name, golden_dir)
    _, model = build_pair(hp, ds, randomize_bn=True, atomic=atomic)
    _set_mode(model, mode)
    stats = {k: v.clone() for k, v in model.named_buffers()}
    out_m, grads_m = _product_grads(model, graphs, target, atomic)
    _close(out_m, out_r, 5e-4, f"{name} {mode}: forward")
    bn_keys = [k for k in grads_r if ".norm.n." in k]
    assert len(bn_keys) == 2 * hp["num_layers"]      # the BatchNorm affine is part of the comparison
    worst = 0.0
    for k, g in grads_r.items():
        assert k in grads_m, k
        _close(grads_m[k], g, 3e-3, f"{name} {mode}: grad {k}")
        worst = max(worst, (grads_m[k].cpu().double() - g.double()).abs().max().item() / max(1e-12, g.abs().max().item()))
    print(f"{name} {mode}: worst gradient error / tensor scale {worst:.2e}")
    for k, v in model.named_buffers():
        assert torch.equal(v, stats[k]), f"{k} was written"
    # bitwise reproducible
    out_2, grads_2 = _product_grads(model, graphs, target, atomic)
    assert torch.equal(out_m, out_2)
    assert all(torch.equal(grads_m[k], grads_2[k]) for k in grads_m)


@pytest.mark.parametrize("name", ["lmax2", "paper", "norm"])
def test_eval_forward_in_grad_mode_matches_the_no_grad_forward(name, golden_dir):
    from matten_amd.data.graph import collate

    hp, atomic, n = MODELS[name]
    graphs, ds = _graphs(golden_dir, n)
    _, model = build_pair(hp, ds, randomize_bn=True)
    model.eval()
    with torch.no_grad():
        want = model(collate(graphs, device=DEV))[0]["elastic_tensor_full"]
    got = model(collate(graphs, device=DEV))[0]["elastic_tensor_full"]
    assert got.requires_grad and not want.requires_grad
    # (floor: two HIP paths against each other -- the pooled 2e / 4e blocks of these crystals nearly vanish by symmetry and
    # carry the rounding of their per-atom terms; the allowance close_blocks documents for that, as in "paths vs fused")
    close_blocks(got, want, what=f"{name}: eval forward, grad mode vs no_grad", floor=2e-6)


# ---- fine-tuning step ----------------------------------------------------------------------------------------------------
def _finetune_batch(golden_dir, n=8):
    from matten_amd.data.graph import collate

    graphs, ds = _graphs(golden_dir, n)
    target = torch.randn(n, 21, generator=torch.Generator().manual_seed(7))
    return graphs, ds, target, dict(collate(graphs, device=DEV), elastic_tensor_full=target.to(DEV))


@pytest.mark.parametrize("freeze", ["statistics", "affine"])
def test_trainer_flat_adam_step_with_frozen_batchnorm(freeze, golden_dir):
    """one Trainer.fit step (FlatAdam from optimizer_hparams, freeze_batchnorm set): the BatchNorm buffers are bit-identical
    afterwards, the parameters follow a torch.optim.Adam step on the oracle's eval-mode gradients (the check of the
    training-step test: compared where the gradient is well above rounding, within +- 2 lr everywhere)."""
    from matten_amd.data.graph import collate
    from matten_amd.model.trainer import Trainer

    graphs, ds, target, batch = _finetune_batch(golden_dir)
    ref, model = build_pair(LMAX2, ds, randomize_bn=True)
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    model.optimizer_hparams = {"class_path": "matten_amd.optim.FlatAdam", "init_args": {"lr": 1e-2, "weight_decay": 1e-5},
                               "freeze_batchnorm": True if freeze == "statistics" else "affine"}
    model.lr_scheduler_hparams = None
    Trainer(max_epochs=1).fit(model, train_dataloaders=[batch])
    assert model.training and not any(m.training for m in model.modules() if type(m).__name__ == "_IrrepBatchNorm")
    after = model.state_dict()
    for k, v in before.items():
        if k.endswith(("running_mean", "running_var", "num_batches_tracked")):
            assert torch.equal(after[k], v), f"{k} changed under frozen statistics"
        if freeze == "affine" and ".norm.n." in k:
            assert torch.equal(after[k], v), f"{k} changed under a frozen affine"

    ref.eval()
    ps = [p for k, p in ref.named_parameters() if not (freeze == "affine" and ".norm.n." in k)]
    opt_r = torch.optim.Adam(ps, lr=1e-2, weight_decay=1e-5)
    torch.nn.functional.mse_loss(ref.decode(collate(graphs)), target).backward()
    grads_r = {k: p.grad.clone() for k, p in ref.named_parameters() if p.grad is not None}
    opt_r.step()
    named = dict(model.named_parameters())
    moved = 0
    for k, p in ref.named_parameters():
        if k not in grads_r or (freeze == "affine" and ".norm.n." in k):
            continue
        g = grads_r[k] + 1e-5 * p.detach()
        solid = (g.abs() >= 1e-2 * grads_r[k].abs().max()).to(DEV)
        got, want = named[k].detach(), p.detach().to(DEV)
        _close(torch.where(solid, got, want), want, 2e-3, f"param after the fine-tune step {k}")
        assert ((got - want).abs() <= 2.0 * 1e-2 + 1e-6).all(), k
        moved += int(not torch.equal(got, before[k]))
    assert moved > 0
    if freeze == "statistics":
        assert any(not torch.equal(after[k], before[k]) for k in before if k.endswith(".norm.n.weight"))


def test_frozen_step_replays_from_a_hipgraph_bit_for_bit(golden_dir):
    """GraphedTrainStep over a frozen-BatchNorm model: the replayed steps give exactly the eager steps' parameters, the
    running statistics stay as they were."""
    from matten_amd.graphs import GraphedTrainStep
    from matten_amd.model import freeze_batchnorm
    from matten_amd.optim import FlatAdam

    graphs, ds, target, batch = _finetune_batch(golden_dir)
    batch.pop("elastic_tensor_full")
    target = target.to(DEV)

    def make():
        _, m = build_pair(LMAX2, ds, randomize_bn=True)
        freeze_batchnorm(m).train()
        return m, FlatAdam(m.parameters(), lr=1e-2, weight_decay=1e-5)

    def loss_fn(preds, t):
        return torch.nn.functional.mse_loss(preds["elastic_tensor_full"], t)

    eager, opt_e = make()
    graphed, opt_g = make()
    stats = {k: v.clone() for k, v in graphed.named_buffers()}
    step = GraphedTrainStep(graphed, opt_g, loss_fn, batch, target, warmup=2)
    for _ in range(3):
        le = loss_fn(eager(dict(batch))[0], target)
        opt_e.zero_grad()
        le.backward()
        opt_e.step()
        lg = step.step(batch, target)
        assert torch.equal(lg, le.detach())
    for (k, pe), (_, pg) in zip(eager.named_parameters(), graphed.named_parameters()):
        assert torch.equal(pe, pg), f"{k}: replayed step differs from the eager step"
    for k, v in graphed.named_buffers():
        assert torch.equal(v, stats[k]), f"{k} was written"


def test_train_mode_step_and_no_grad_forward_are_reproducible_next_to_the_new_route(golden_dir):
    """the routes that must not change: a train-mode step (batch statistics, running averages updated) and the no-grad eval
    forward give the same bits before and after eval-mode gradient steps on the same model"""
    from matten_amd.data.graph import collate

    graphs, ds = _graphs(golden_dir, 8)
    target = torch.randn(8, 21, generator=torch.Generator().manual_seed(7))
    _, a = build_pair(LMAX2, ds, randomize_bn=True)
    _, b = build_pair(LMAX2, ds, randomize_bn=True)
    with torch.no_grad():
        want = a(collate(graphs, device=DEV))[0]["elastic_tensor_full"]
    _product_grads(b.eval(), graphs, target, False)          # the new route ran on b only
    with torch.no_grad():
        assert torch.equal(b(collate(graphs, device=DEV))[0]["elastic_tensor_full"], want)
    out_a, grads_a = _product_grads(a.train(), graphs, target, False)
    out_b, grads_b = _product_grads(b.train(), graphs, target, False)
    assert torch.equal(out_a, out_b) and all(torch.equal(grads_a[k], grads_b[k]) for k in grads_a)
    for (k, u), (_, v) in zip(a.named_buffers(), b.named_buffers()):
        assert torch.equal(u, v), k
