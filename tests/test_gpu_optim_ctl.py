"""
FlatAdam's device-control route on the GPU (matten_adam_step_ctl): the gradient norm against numpy fp64, clipped Adam /
AdamW trajectories against torch in fp64, the non-finite guard, the EMA, a hipGraph replay that follows a changed learning
rate, state_dict round trips and the Trainer's gradient_clip_val.

The parameter shapes give slot tails that are no multiple of four and, with the 70 001-element tensor, 69 workgroups of
the norm pass (1024 floats per workgroup and round).  The norm pass stops adding workgroups at 1024 of them (1024 * 1024
floats: lanes start on their second load) and starts a second trip of its four-load loop at 4 * 1024 * 1024 floats: the
norm is checked just above both.
"""
import copy

import numpy as np
import pytest
import torch

from common import LMAX2, build_pair
from test_gpu_training import _close, _graphs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(7,), (3, 5), (1,), (33, 2), (64,), (70001,)]
CAP = 1024 * 1024                       # floats: 1024 workgroups x 1024 floats
MAX_NORM = 265.0                        # ~ the norm of a standard normal gradient over the 70 185 elements of SHAPES
FACTORS = (0.5, 2.0, 0.25, 3.0, 1.5)    # gradient scale per step: norms ~ 132, 530, 66, 795, 397 -> clipped at steps 1, 3, 4


def _params(shapes, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g) for s in shapes]


def _fresh(values):
    return [torch.nn.Parameter(v.clone().to(DEV)) for v in values]


def _set_grads(opt, ps, grads):
    """the gradients land where autograd would put them: in the views of the flat buffer (the padding stays zero)"""
    opt.zero_grad()
    with torch.no_grad():
        for p, g in zip(ps, grads):
            p.grad.copy_(g)


def _grads(shapes, seed, steps=5, factors=FACTORS):
    g = torch.Generator().manual_seed(seed)
    return [[f * torch.randn(s, generator=g) for s in shapes] for f, _ in zip(factors, range(steps))]


def _run(opt, ps, grads, watch=None):
    for gr in grads:
        _set_grads(opt, ps, gr)
        opt.step()
        if watch is not None:
            watch(opt)


# ---------------------------------------------------------------------------------------------------
# 1. the norm
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["shapes", "zero", "single", "above_cap", "above_second_trip"])
def test_grad_norm_matches_numpy_fp64(case):
    """the squares of fp32 values are exact in fp64 and the sum runs in fp64: what is left is one rounding to fp32 and the
    square root -> 5e-7 relative"""
    from matten_amd.optim import FlatAdam

    shapes = {"shapes": SHAPES, "zero": SHAPES, "single": [(1,)], "above_cap": [(CAP + 5,)],
              "above_second_trip": [(4 * CAP + 5,), (3,)]}[case]
    ps = _fresh(_params(shapes, 1))
    before = [p.detach().clone() for p in ps]
    max_norm = 0.37
    opt = FlatAdam(ps, lr=1e-2, max_grad_norm=max_norm)
    grads = _grads(shapes, 2, steps=1, factors=(1.0,))[0]
    if case == "zero":
        grads = [torch.zeros(s) for s in shapes]
    _set_grads(opt, ps, grads)
    opt.step()
    want = float(np.sqrt(sum(np.square(g.numpy().astype(np.float64)).sum() for g in grads)))
    got, scale = opt.last_grad_norm, opt.last_clip_scale
    print(f"{case}: norm {got!r} (fp64 {want!r}), scale {scale!r}")
    assert abs(got - want) <= 5e-7 * want
    if case == "zero":
        assert got == 0.0 and scale == 1.0                  # max_norm / (0 + 1e-6) clamps to 1: no NaN
        assert all(torch.equal(p, b) for p, b in zip(ps, before))
    else:
        # from the fp64 norm: the norm's own 5e-7, the fp32 roundings of max_norm, of the sum and of the quotient (6e-8 each)
        want_scale = min(1.0, max_norm / (want + 1e-6))
        assert abs(scale - want_scale) <= 7e-7 * want_scale
    assert all(torch.isfinite(p).all() for p in ps) and opt.skipped_steps == 0 and float(opt.step_count) == 1.0


# ---------------------------------------------------------------------------------------------------
# 2. / 7. clipped trajectories against torch in fp64; reproducibility
# ---------------------------------------------------------------------------------------------------
def _clipped_run(decoupled):
    from matten_amd.optim import FlatAdam

    ps = _fresh(_params(SHAPES, 3))
    opt = FlatAdam(ps, lr=1e-2, weight_decay=1e-2, max_grad_norm=MAX_NORM, decoupled_weight_decay=decoupled)
    scales = []
    _run(opt, ps, _grads(SHAPES, 4), watch=lambda o: scales.append(o.last_clip_scale))
    return ps, opt, scales


@pytest.mark.parametrize("decoupled", [False, True])
def test_clipped_trajectory_follows_torch(decoupled):
    ps, opt, scales = _clipped_run(decoupled)
    ref = [torch.nn.Parameter(v.double()) for v in _params(SHAPES, 3)]
    opt_r = (torch.optim.AdamW if decoupled else torch.optim.Adam)(ref, lr=1e-2, weight_decay=1e-2)
    for gr in _grads(SHAPES, 4):
        for r, g in zip(ref, gr):
            r.grad = g.double()
        torch.nn.utils.clip_grad_norm_(ref, MAX_NORM)
        opt_r.step()
    print("clip scales:", scales)
    assert [s < 1.0 for s in scales] == [False, True, False, True, True]
    assert all(s == 1.0 or s < 0.7 for s in scales)
    for p, r in zip(ps, ref):
        _close(p, r, 1e-6, f"clipped {'AdamW' if decoupled else 'Adam'} parameter")
    assert float(opt.step_count) == 5.0


@pytest.mark.parametrize("decoupled", [False, True])
def test_two_fresh_runs_end_with_the_same_bits(decoupled):
    (_, a, _), (_, b, _) = _clipped_run(decoupled), _clipped_run(decoupled)
    assert a.flat_params.data_ptr() != b.flat_params.data_ptr()
    assert torch.equal(a.flat_params, b.flat_params) and torch.equal(a.exp_avg_sq, b.exp_avg_sq)
    assert a.last_grad_norm == b.last_grad_norm


# ---------------------------------------------------------------------------------------------------
# 3. clipping off
# ---------------------------------------------------------------------------------------------------
def test_unreachable_bound_follows_the_default_optimiser():
    from matten_amd import _lib
    from matten_amd.optim import FlatAdam

    init, grads = _params(SHAPES, 5), _grads(SHAPES, 6)
    pa, pb = _fresh(init), _fresh(init)
    a = FlatAdam(pa, lr=1e-2, weight_decay=1e-5, max_grad_norm=1e30)
    b = FlatAdam(pb, lr=1e-2, weight_decay=1e-5)
    assert a.device_control and not b.device_control
    assert set(b.state[pb[0]]) == {"step", "exp_avg", "exp_avg_sq"}          # the default layout is what it was
    assert {"ctl", "counters", "workspace"} <= set(a.state[pa[0]])
    _run(a, pa, grads)
    _run(b, pb, grads)
    for p, q in zip(pa, pb):
        _close(p, q, 1e-6, "parameter with the bound out of reach")
    assert a.last_clip_scale == 1.0 and float(a.step_count) == float(b.step_count) == 5.0
    # the default optimiser keeps no such state, and cannot change route once it has stepped
    with pytest.raises(_lib.MattenHipError, match="device_lr"):
        b.last_grad_norm
    with pytest.raises(_lib.MattenHipError, match="already stepped"):
        b.set_max_grad_norm(1.0)
    # device_lr alone: no norm is taken
    pc = _fresh(init)
    c = FlatAdam(pc, lr=1e-2, weight_decay=1e-5, device_lr=True)
    _run(c, pc, grads)
    for p, q in zip(pc, pb):
        _close(p, q, 1e-6, "parameter with device_lr only")
    assert np.isnan(c.last_grad_norm) and c.last_clip_scale == 1.0 and c.skipped_steps == 0


# ---------------------------------------------------------------------------------------------------
# 4. the guard
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_guard_drops_a_step_with_a_non_finite_gradient(bad):
    from matten_amd.optim import FlatAdam

    init, grads = _params(SHAPES, 7), _grads(SHAPES, 8, steps=3, factors=(1.0, 2.0, 1.0))
    poisoned = [g.clone() for g in grads[1]]
    poisoned[5][12345] = bad
    kw = dict(lr=1e-2, weight_decay=1e-5, max_grad_norm=MAX_NORM, ema_decay=0.9, skip_nonfinite=True)
    pa, pb = _fresh(init), _fresh(init)
    a, b = FlatAdam(pa, **kw), FlatAdam(pb, **kw)
    _run(a, pa, grads[:1])
    _run(b, pb, grads[:1])
    names = ("flat_params", "exp_avg", "exp_avg_sq", "ema_params", "step_count")
    before = {k: getattr(a, k).clone() for k in names}
    _run(a, pa, [poisoned])
    for k in names:
        assert torch.equal(getattr(a, k).view(torch.int32), before[k].view(torch.int32)), k
    assert a.skipped_steps == 1 and b.skipped_steps == 0 and float(a.step_count) == 1.0
    assert not np.isfinite(a.last_grad_norm)
    _run(a, pa, grads[2:])                  # a clean step: as if the bad one had never been seen
    _run(b, pb, grads[2:])
    for k in names:
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert a.skipped_steps == 1 and float(a.step_count) == 2.0 and int(a.counters[1]) == 0
    assert all(torch.isfinite(p).all() for p in pa)
    # without the guard the scale is NaN (0 for an infinite norm) and the parameters go bad, as under torch
    pc = _fresh(init)
    c = FlatAdam(pc, lr=1e-2, weight_decay=1e-5, max_grad_norm=MAX_NORM)
    _run(c, pc, [poisoned])
    if np.isnan(bad):
        assert all(torch.isnan(p).all() for p in pc)
    else:
        assert c.last_clip_scale == 0.0 and torch.isnan(pc[5][12345])
    assert c.skipped_steps == 0 and float(c.step_count) == 1.0


# ---------------------------------------------------------------------------------------------------
# 5. EMA
# ---------------------------------------------------------------------------------------------------
def test_ema_follows_the_recurrence_and_swaps_in_and_out():
    from matten_amd.nn._tables import weights_epoch
    from matten_amd.optim import FlatAdam

    d = 0.9
    ps = _fresh(_params(SHAPES, 9))
    opt = FlatAdam(ps, lr=1e-2, ema_decay=d)
    assert torch.equal(opt.ema_params, opt.flat_params) and opt.ema_params.data_ptr() != opt.flat_params.data_ptr()
    # the decay reaches the kernel as an fp32 argument: the fp64 recurrence runs with that value
    d32 = float(np.float32(d))
    ema = opt.flat_params.double().cpu()
    size = ema.abs()
    trajectory = []
    _run(opt, ps, _grads(SHAPES, 10), watch=lambda o: trajectory.append(o.flat_params.double().cpu()))
    for p in trajectory:
        ema = d32 * ema + (1.0 - d32) * p
        size = torch.maximum(size, p.abs())
    # at most 5 fp32 roundings of a convex combination (~5 x 6e-8), each relative to the size of what is combined: per
    # element, against the largest magnitude that element's parameter took (an EMA that passes through zero has no
    # relative accuracy of its own)
    err = (opt.ema_params.double().cpu() - ema).abs()
    worst = (err / size.clamp(min=1e-30)).max().item()
    print(f"EMA after 5 steps: max error / element size {worst:.3e}")
    assert (err <= 1e-6 * size).all(), worst
    _close(opt.ema_params, ema, 1e-6, "EMA after 5 steps")
    assert not torch.equal(opt.ema_params, opt.flat_params)
    train = opt.flat_params.clone()
    e0 = weights_epoch()
    with opt.ema_weights():
        e1 = weights_epoch()
        for p, o in zip(ps, opt._offs):
            assert torch.equal(p.detach().reshape(-1), opt.ema_params[o:o + p.numel()])
    assert e0 < e1 < weights_epoch()
    assert torch.equal(opt.flat_params.view(torch.int32), train.view(torch.int32))
    assert all(p.data_ptr() == opt.flat_params.data_ptr() + 4 * o for p, o in zip(ps, opt._offs))
    target = torch.nn.ParameterList(_fresh(_params(SHAPES, 11)))
    opt.copy_ema_to(target)
    for q, p, o in zip(target, ps, opt._offs):
        assert torch.equal(q.detach().reshape(-1), opt.ema_params[o:o + p.numel()])
    with pytest.raises(ValueError, match="do not match"):
        opt.copy_ema_to(_fresh(_params(SHAPES[:-1], 11)))


# ---------------------------------------------------------------------------------------------------
# 6. hipGraph replay follows a scheduler
# ---------------------------------------------------------------------------------------------------
def test_replayed_step_matches_eager_bitwise_and_follows_the_learning_rate(golden_dir):
    from matten_amd.data.graph import collate
    from matten_amd.graphs import GraphedTrainStep
    from matten_amd.optim import FlatAdam

    graphs, ds = _graphs(golden_dir, 8)
    batch = collate(graphs, device=DEV)
    target = torch.randn(8, 21, generator=torch.Generator().manual_seed(12)).to(DEV)

    def loss_fn(preds, t):
        return torch.nn.functional.mse_loss(preds["elastic_tensor_full"], t)

    def make():
        _, m = build_pair(LMAX2, ds, randomize_bn=True)
        m.train()
        return m, FlatAdam(m.parameters(), lr=1e-2, weight_decay=1e-5, max_grad_norm=1.0, ema_decay=0.99, skip_nonfinite=True)

    def eager(m, o):
        loss = loss_fn(m(dict(batch))[0], target)
        o.zero_grad()
        loss.backward()
        o.step()

    (mg, og), (me, oe), (ms, os_) = make(), make(), make()
    init = og.flat_params.clone()
    assert torch.equal(init, oe.flat_params)
    step = GraphedTrainStep(mg, og, loss_fn, batch, target, warmup=2)
    # the warm-up steps were real ones: learning rate, EMA, counters and step count are back where they were
    assert og.skipped_steps == 0 and float(og.step_count) == 0.0 and float(og.ctl[0]) == float(np.float32(1e-2))
    assert torch.equal(og.ema_params, init) and torch.equal(og.flat_params, init)
    for _ in range(2):
        step.step(batch, target)
        eager(me, oe)
        eager(ms, os_)
    assert torch.equal(og.flat_params, oe.flat_params) and torch.equal(og.ema_params, oe.ema_params)
    assert float(og.step_count) == 2.0 and og.last_grad_norm == oe.last_grad_norm and og.last_clip_scale <= 1.0
    for o in (og, oe):                      # what ReduceLROnPlateau does
        o.param_groups[0]["lr"] *= 0.5
    step.step(batch, target)
    eager(me, oe)
    eager(ms, os_)                          # this twin keeps the learning rate the graph was captured with
    assert float(og.ctl[0]) == float(np.float32(5e-3))
    assert torch.equal(og.flat_params, oe.flat_params) and torch.equal(og.ema_params, oe.ema_params)
    assert not torch.equal(og.flat_params, os_.flat_params)
    assert og.skipped_steps == 0 and float(og.step_count) == 3.0 and torch.isfinite(og.flat_params).all()


# ---------------------------------------------------------------------------------------------------
# 8. state_dict
# ---------------------------------------------------------------------------------------------------
def test_state_dict_round_trip_with_ema_and_counters():
    from matten_amd.optim import FlatAdam

    shapes = SHAPES[:5]
    init = _params(shapes, 13)
    grads = _grads(shapes, 14, steps=5, factors=(1.0, 1.0, 1.0, 1.0, 1.0))
    grads[1][3][4, 1] = float("nan")                          # the second step is skipped
    kw = dict(weight_decay=1e-5, max_grad_norm=5.0, ema_decay=0.9, skip_nonfinite=True)
    pa = _fresh(init)
    a = FlatAdam(pa, lr=1e-2, **kw)
    _run(a, pa, grads[:3])
    assert a.skipped_steps == 1 and float(a.step_count) == 2.0
    sd = copy.deepcopy(a.state_dict())
    pb = _fresh([p.detach().cpu() for p in pa])
    b = FlatAdam(pb, lr=1e-3, **kw)
    b.load_state_dict(sd)
    assert b.param_groups[0]["lr"] == 1e-2 and float(b.ctl[0]) == float(np.float32(1e-2))
    assert b.skipped_steps == 1 and float(b.step_count) == 2.0 and b.last_grad_norm == a.last_grad_norm
    assert torch.equal(b.ema_params, a.ema_params) and not torch.equal(b.ema_params, b.flat_params)
    assert b.state[pb[0]]["ema"].data_ptr() == b.ema_params.data_ptr()
    _run(a, pa, grads[3:])
    _run(b, pb, grads[3:])
    assert torch.equal(a.flat_params, b.flat_params) and torch.equal(a.ema_params, b.ema_params)
    # a state saved by a default FlatAdam: moments and step come back, the EMA starts from the current parameters
    pc = _fresh(init)
    c = FlatAdam(pc, lr=1e-2, weight_decay=1e-5)
    _run(c, pc, grads[2:4])
    sd_c = copy.deepcopy(c.state_dict())
    pd = _fresh([p.detach().cpu() for p in pc])
    e = FlatAdam(pd, lr=1e-3, weight_decay=1e-5, ema_decay=0.9)
    with torch.no_grad():
        e.ema_params.fill_(7.0)
    e.load_state_dict(sd_c)
    assert torch.equal(e.ema_params, e.flat_params) and e.skipped_steps == 0 and float(e.step_count) == 2.0
    assert float(e.ctl[0]) == float(np.float32(1e-2)) and torch.equal(e.exp_avg, c.exp_avg)
    _run(c, pc, grads[4:])
    _run(e, pd, grads[4:])
    for p, q in zip(pd, pc):
        _close(p, q, 1e-6, "parameter after resuming from a default FlatAdam state")


# ---------------------------------------------------------------------------------------------------
# 9. Trainer(gradient_clip_val=...)
# ---------------------------------------------------------------------------------------------------
def test_trainer_clips_through_flat_adam(golden_dir):
    from matten.dataset.structure_scalar_tensor import TensorDataModule
    from matten.model.trainer import Trainer
    from matten.model_factory.task import TensorRegressionTask
    from matten.model_factory.tfn_scalar_tensor import ScalarTensorModel
    from matten_amd.optim import FlatAdam

    name = "example_crystal_elasticity_tensor_n100.json"
    dm = TensorDataModule(trainset_filename=name, valset_filename=name, testset_filename=name, root=golden_dir, r_cut=5.0,
                          tensor_target_name="elastic_tensor_full", tensor_target_scale=1e-2,
                          loader_kwargs={"batch_size": 32, "shuffle": False}, device=DEV)
    dm.prepare_data()
    dm.setup()
    torch.manual_seed(35)
    model = ScalarTensorModel(
        tasks=TensorRegressionTask(name="elastic_tensor_full"), backbone_hparams=dict(LMAX2),
        dataset_hparams=dm.get_to_model_info(),
        optimizer_hparams={"class_path": "matten_amd.optim.FlatAdam",
                           "init_args": {"lr": 0.01, "weight_decay": 0.00001, "ema_decay": 0.999, "skip_nonfinite": True}},
        lr_scheduler_hparams={"class_path": "torch.optim.lr_scheduler.ReduceLROnPlateau",
                              "init_args": {"mode": "min", "factor": 0.5, "patience": 50}},
    ).to(DEV)
    trainer = Trainer(max_epochs=1, limit_train_batches=1, gradient_clip_val=0.05)
    trainer.fit(model, datamodule=dm)
    (opt,) = trainer.optimizers
    assert isinstance(opt, FlatAdam) and opt.max_grad_norm == 0.05 and float(opt.step_count) == 1.0
    norm, scale = opt.last_grad_norm, opt.last_clip_scale
    print(f"Trainer step: gradient norm {norm:.4e}, clip scale {scale:.4e}")
    assert np.isfinite(norm) and 0.0 < scale <= 1.0 and opt.skipped_steps == 0
    assert torch.isfinite(opt.flat_params).all() and torch.isfinite(opt.ema_params).all()
    assert np.isfinite(trainer.history[0]["val/score"])
