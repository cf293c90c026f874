"""Padded, shape-bucketed device batches on the GPU: matten_batch_gather_padded against its host restatement
(GraphStoreHost.padded_reference), training-mode BatchNorm over the valid rows (matten_bn_train_fwd_valid / _bwd_valid)
against fp64, a training step on a padded batch against the oracle on the unpadded one, and an epoch of
BucketedTrainStep against eager steps."""
import copy
import os

import pytest
import torch

from common import LMAX2, build_pair
from store_cases import TARGET, golden_graphs, many_key_graphs, store_graphs, streams_needed

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CSR_KEYS = ("_amd_perm", "_amd_rowptr", "_amd_src_sorted")
TRAIN_KEYS = ("_amd_dst_sorted", "_amd_out_ptr", "_amd_out_perm")


def _close(got, want, rtol, what):
    """the measure of tests/test_gpu_training.py: the largest error against the largest reference magnitude"""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    scale = max(1e-12, want.abs().max().item())
    err = (got - want).abs().max().item()
    print(f"{what}: max err {err:.3e} vs scale {scale:.3e} (bound {rtol:.0e})")
    assert err <= rtol * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e}"


def _round_up(v, q):
    return q * -(-v // q)


# ----------------------------------------------------------------------------------------------------------------------
# 1. the gather
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def store():
    from matten.data.store import DeviceGraphStore

    return DeviceGraphStore.from_graphs(store_graphs(), DEV)


def _check_padded(store, idx, pad_to, training=True, **kw):
    from matten_amd import ops
    from matten_amd.nn._nequip import ensure_training_edge_tensors

    got = store.batch(idx, training=training, pad_to=pad_to, **kw)
    want = store.host.padded_reference(idx, pad_to, training=training, **kw)
    assert list(got.keys()) == list(want.keys())
    for k, v in want.items():
        g = got[k]
        assert g.dtype == v.dtype and g.shape == v.shape, (k, g.dtype, v.dtype, g.shape, v.shape)
        assert g.device == torch.device(DEV) and g.is_contiguous(), k
        assert torch.equal(g.cpu(), v), k
    n_b, e_b, b_b = pad_to
    assert got["pos"].shape[0] == n_b and got["edge_index"].shape[1] == e_b and got["ptr"].shape[0] == b_b + 1
    # the whole-batch CSR keys are ops.csr_build of the padded edge_index
    perm, rowptr, src, _ = ops.csr_build(got["edge_index"], n_b)
    for k, v in zip(CSR_KEYS, (perm, rowptr, src)):
        assert got[k].dtype == v.dtype and torch.equal(got[k], v), k
    if training:
        public = {k: v for k, v in got.items() if not k.startswith("_amd_")}
        ref = ensure_training_edge_tensors(public)
        out_ptr, out_perm = ref["_amd_out_csr"]
        for k, v in zip(TRAIN_KEYS, (ref["_amd_dst_sorted"], out_ptr, out_perm)):
            assert got[k].dtype == v.dtype and torch.equal(got[k], v), k
    else:
        assert not any(k in got for k in TRAIN_KEYS)
    return got


def _sizes(store, idx):
    _, n, e = store.host.plan(idx)
    return n, e


def _same_as_plain(got, plain, e):
    """the first B crystals of the padded batch `got` are bit for bit the unpadded batch `plain` of e edges"""
    for k, v in plain.items():
        part = got[k][:, :e] if k == "edge_index" else got[k][:v.shape[0]]
        if k in ("_amd_rowptr", "_amd_out_ptr", "ptr"):
            part, v = part[:-1], v[:-1]   # (the closing entry of the unpadded batch is the first padding row's start)
        assert torch.equal(part, v), k


def test_gather_16_crystals_to_the_next_bucket(store):
    idx = list(range(40, 56))
    n, e = _sizes(store, idx)
    got = _check_padded(store, idx, (_round_up(n + 1, 64), _round_up(e, 1024), 17))
    assert got["_amd_n_valid"].tolist() == [n, e, 16]
    _same_as_plain(got, store.batch(idx), e)


def test_gather_without_padding_edges(store):
    idx = [3, 1, 4, 1, 5, 102, 100]
    n, e = _sizes(store, idx)
    _check_padded(store, idx, (n + 7, e, len(idx) + 1))


def test_gather_one_hub(store):
    """P == 1: one padding node owns 300 self-image edges"""
    idx = [9, 2, 6]
    n, e = _sizes(store, idx)
    got = _check_padded(store, idx, (n + 1, e + 300, 4))
    assert got["num_neigh"][n:].tolist() == [300.0] and got["_amd_rowptr"][n:].tolist() == [e, e + 300]


def test_gather_three_padding_crystals(store):
    idx = [5, 99, 0, 17, 101]
    n, e = _sizes(store, idx)
    got = _check_padded(store, idx, (n + 10, e + 23, len(idx) + 3), pad_species=13, pad_length=1.5)
    assert got["ptr"][-4:].tolist() == [n, n + 8, n + 9, n + 10] and got["batch"][-3:].tolist() == [5, 6, 7]
    assert (got["atomic_numbers"][n:] == 13).all()


def test_gather_without_training_keys(store):
    idx = [30, 31, 100, 32]
    n, e = _sizes(store, idx)
    _check_padded(store, idx, (_round_up(n + 2, 64), _round_up(e, 1024), 6), training=False)


def test_gather_table_beyond_lds(store):
    """more than 1023 crystals: the running sums are searched in global memory (as test_table_in_lds_and_beyond)"""
    from matten_amd import _lib

    cap = _lib.load().matten_batch_gather_lds_rows()
    g = torch.Generator().manual_seed(5)
    for b, k in ((cap - 2, 1), (cap + 76, 2)):   # B_b + 1 == cap: the last table in LDS; B_b + 1 > cap
        idx = torch.randint(0, 100, (b,), generator=g).tolist()
        n, e = _sizes(store, idx)
        got = _check_padded(store, idx, (_round_up(n + k, 64), _round_up(e, 1024), b + k))
    # above the cap too, the real rows are bit for bit the unpadded batch (as test_gather_16_crystals_to_the_next_bucket)
    assert b + k + 1 > cap
    _same_as_plain(got, store.batch(idx), e)


def test_gather_extra_keys():
    """per-crystal, per-node and per-edge extra keys (4- and 8-byte elements): zero on the padding rows"""
    from matten.data.store import DeviceGraphStore

    rng = torch.Generator().manual_seed(3)
    graphs = []
    for g in store_graphs()[88:]:
        n, e = g["pos"].shape[0], g["edge_index"].shape[1]
        graphs.append(dict(g, node_tensor=torch.randn(n, 9, generator=rng),
                           edge_tag=torch.randint(-2 ** 40, 2 ** 40, (e,), generator=rng),
                           crystal_pair=torch.randn(1, 2, generator=rng, dtype=torch.float64)))
    s = DeviceGraphStore.from_graphs(graphs, DEV)
    idx = [13, 0, 12, 14, 5, 5]
    n, e = _sizes(s, idx)
    got = _check_padded(s, idx, (n + 5, e + 11, len(idx) + 2))
    assert got["crystal_pair"].shape == (8, 2) and got["crystal_pair"].dtype == torch.float64
    assert not got["crystal_pair"][6:].any() and not got[TARGET][6:].any()
    assert not got["node_tensor"][n:].any() and not got["edge_tag"][e:].any()
    assert got["crystal_pair"][:6].abs().min() > 0


def test_gather_more_streams_than_one_launch_takes():
    """18 extra keys: a training batch is 34 streams, two launches of the padded entry; every extra key zero on its
    padding rows, n_valid written"""
    from matten.data.store import CRYSTAL, EDGE, NODE, DeviceGraphStore
    from matten_amd import _lib

    s = DeviceGraphStore.from_graphs(many_key_graphs(), DEV)
    cap = _lib.load().matten_batch_gather_max_streams()
    assert cap < streams_needed(s.host) <= 2 * cap
    idx = [13, 0, 12, 14, 5, 5]
    n, e = _sizes(s, idx)
    got = _check_padded(s, idx, (n + 5, e + 11, len(idx) + 2))
    assert got["_amd_n_valid"].tolist() == [n, e, len(idx)]
    first_pad = {NODE: n, EDGE: e, CRYSTAL: len(idx)}
    extra = [k for k in s.host.keys if "_extra" in k]
    assert len(extra) == 18
    for k in extra:
        real, pad = got[k][:first_pad[s.host.classes[k]]], got[k][first_pad[s.host.classes[k]]:]
        assert pad.shape[0] > 0 and not pad.any() and bool((real != 0).all()), k


# ----------------------------------------------------------------------------------------------------------------------
# 2. BatchNorm over the valid rows
# ----------------------------------------------------------------------------------------------------------------------
def _bn_case(n_rows):
    from matten_amd.nn.utils import _IrrepBatchNorm
    from matten_amd.o3 import Irreps

    irreps = Irreps("8x0e+4x0o+5x1o+3x2e")
    gen = torch.Generator(device=DEV).manual_seed(5)
    bn = _IrrepBatchNorm(irreps).to(DEV)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(bn.weight.shape, device=DEV, generator=gen) + 0.5)
        bn.bias.copy_(torch.randn(bn.bias.shape, device=DEV, generator=gen))
    x = torch.randn(n_rows, irreps.dim, device=DEV, generator=gen)
    x[:, :8] += 50.0
    gy = torch.randn(n_rows, irreps.dim, device=DEV, generator=gen)
    return irreps, bn, x, gy, gen


def _bn_run(bn, x, gy, n_valid):
    """-> [y, dx, dweight, dbias, running_mean, running_var] of one training forward and backward"""
    bn.running_mean.zero_(), bn.running_var.fill_(1.0)
    bn.weight.grad = bn.bias.grad = None
    x = x.detach().clone().requires_grad_(True)
    y = bn.forward_train(x, n_valid) if n_valid is not None else bn.forward_train(x)
    y.backward(gy)
    return [t.detach().clone() for t in (y, x.grad, bn.weight.grad, bn.bias.grad, bn.running_mean, bn.running_var)]


@pytest.mark.parametrize("n_valid,n_rows", [(300, 384), (2047, 2304), (2100, 2304), (5003, 5120)])
def test_batchnorm_over_the_valid_rows(n_valid, n_rows):
    """both routes (one launch below 2048 padded rows, the two-stage column form from there on), the route being set by the
    padded count ((2047, 2304): 2047 valid rows on the column route): against the e3nn BatchNorm arithmetic in fp64 over
    x[:n_valid], at the tolerances of test_batchnorm_training_reductions_at_large_row_counts"""
    irreps, bn, x, gy, gen = _bn_case(n_rows)
    N = n_valid
    count = torch.tensor([N, 0, 0], dtype=torch.int64, device=DEV)
    runs = []
    for seed_scale in (1e6, -3e6):   # different finite junk in the padding rows of x and dy
        xj, gj = x.clone(), gy.clone()
        xj[N:] = seed_scale * torch.randn(n_rows - N, irreps.dim, device=DEV, generator=gen)
        gj[N:] = seed_scale * torch.randn(n_rows - N, irreps.dim, device=DEV, generator=gen)
        y, dx, dw, db, rm, rv = _bn_run(bn, xj, gj, count)
        assert torch.isfinite(y).all()
        assert (dx[N:] == 0).all(), "dx of the padding rows is exactly zero"
        runs.append([y[:N], dx[:N], dw, db, rm, rv])
    for a, b in zip(*runs):
        assert torch.equal(a, b), "results must not depend on the padding rows"

    xr = x[:N].detach().cpu().double().requires_grad_(True)
    w = bn.weight.detach().cpu().double().requires_grad_(True)
    b = bn.bias.detach().cpu().double().requires_grad_(True)
    cols, means, nus = [], [], []
    off = ic = ib = 0
    for mul, ir in irreps:
        blk = xr[:, off:off + mul * ir.dim].reshape(N, mul, ir.dim)
        if ir.is_scalar():
            mu = blk.mean(dim=(0, 2))
            blk = blk - mu[None, :, None]
            means.append(mu)
        nu = blk.pow(2).mean(dim=(0, 2))
        nus.append(nu)
        blk = blk * (w[ic:ic + mul] / (nu + bn.eps).sqrt())[None, :, None]
        if ir.is_scalar():
            blk = blk + b[ib:ib + mul][None, :, None]
            ib += mul
        cols.append(blk.reshape(N, -1))
        off += mul * ir.dim
        ic += mul
    yr = torch.cat(cols, 1)
    yr.backward(gy[:N].cpu().double())
    y, dx, dw, db, rm, rv = runs[0]
    _close(y, yr, 2e-5, "y")
    _close(dx, xr.grad, 2e-5, "dL/dx")
    _close(dw, w.grad, 2e-5, "dL/dweight")
    _close(db, b.grad, 2e-5, "dL/dbias")
    _close(rm, 0.1 * torch.cat(means), 1e-6, "running_mean")
    _close(rv, 0.9 + 0.1 * torch.cat(nus), 1e-5, "running_var")


@pytest.mark.parametrize("n_rows", [384, 2304])
def test_batchnorm_all_rows_valid_gives_the_bits_of_the_plain_entry(n_rows):
    _, bn, x, gy, _ = _bn_case(n_rows)
    plain = _bn_run(bn, x, gy, None)
    valid = _bn_run(bn, x, gy, torch.tensor([n_rows, 0, 0], dtype=torch.int64, device=DEV))
    for a, b, name in zip(plain, valid, ("y", "dx", "dweight", "dbias", "running_mean", "running_var")):
        assert torch.equal(a, b), name


@pytest.mark.parametrize("n_rows", [384, 2304])
def test_batchnorm_without_a_valid_row(n_rows):
    """*n_valid == 0 on both routes: zero statistics, finite output, the running averages stay, nothing flows back"""
    _, bn, x, gy, _ = _bn_case(n_rows)
    y, dx, dw, db, rm, rv = _bn_run(bn, x, gy, torch.zeros(3, dtype=torch.int64, device=DEV))
    assert torch.isfinite(y).all() and not dx.any()
    assert torch.isfinite(dw).all() and torch.isfinite(db).all()
    assert not rm.any() and (rv == 1.0).all()


# ----------------------------------------------------------------------------------------------------------------------
# 3. a training step on a padded batch against the oracle on the unpadded one
# ----------------------------------------------------------------------------------------------------------------------
def _first_graphs(golden_dir, n=10):
    from matten_amd.data.graph import average_num_neighbors, crystal_graph
    from oracle.matten_ref.data import structures_from_json

    structs = structures_from_json(os.path.join(golden_dir, "example_crystal_elasticity_tensor_n100.json"))[:n]
    graphs = [crystal_graph(s["cart_coords"], s["lattice"], s["atomic_numbers"], 5.0) for s in structs]
    species = sorted({int(z) for s in structs for z in s["atomic_numbers"]})
    return graphs, {"allowed_species": species, "average_num_neighbors": average_num_neighbors(graphs)}


@pytest.mark.parametrize("k", [1, 3])
def test_padded_training_step_matches_oracle_autograd(golden_dir, k):
    """The device side runs the store's padded batch (quanta (64, 1024), K padding crystals), the oracle the plain collate of
    the 10 real crystals, at the tolerances of test_training_step_matches_oracle_autograd.  Without the valid-rows
    BatchNorm the padding atoms enter the batch statistics: running statistics and gradients are then off."""
    from matten.data.store import DeviceGraphStore
    from matten_amd.data.graph import collate
    from matten_amd.graphs import padded_mean_loss

    graphs, ds = _first_graphs(golden_dir, 10)
    ref, model = build_pair(LMAX2, ds, randomize_bn=True)
    ref.train()
    model.train()
    B = len(graphs)
    target = torch.randn(B, 21, generator=torch.Generator().manual_seed(7))

    out_r = ref.decode(collate(graphs))
    loss_r = torch.nn.functional.mse_loss(out_r, target)
    ref.zero_grad()
    loss_r.backward()
    grads_r = {name: p.grad.clone() for name, p in ref.named_parameters() if p.grad is not None}

    store = DeviceGraphStore.from_graphs(graphs, DEV)
    n, e = _sizes(store, list(range(B)))
    batch = store.batch(list(range(B)), pad_to=(_round_up(n + k, 64), _round_up(e, 1024), B + k))
    assert batch["pos"].shape[0] >= n + k and batch["edge_index"].shape[1] > e   # padding atoms and edges are present
    padded_target = torch.zeros(B + k, 21, device=DEV)
    padded_target[:B] = target.to(DEV)
    loss_fn = padded_mean_loss(lambda p, t: (p - t) ** 2, key=TARGET)
    preds, _ = model(dict(batch))
    out_m = preds[TARGET]
    loss_m = loss_fn(preds, padded_target, batch)
    model.zero_grad()
    loss_m.backward()

    assert out_m.shape == (B + k, 21) and torch.isfinite(out_m).all()   # the padding crystals' predictions are finite
    _close(out_m[:B], out_r, 5e-4, "train-mode forward [B,21]")
    _close(loss_m, loss_r, 1e-4, "loss")
    named = dict(model.named_parameters())
    assert set(grads_r) <= set(named)
    for name, g in grads_r.items():
        assert named[name].grad is not None, name
        _close(named[name].grad, g, 3e-3, f"grad {name}")
    bufs_m = dict(model.named_buffers())
    checked = 0
    for name, buf in ref.named_buffers():
        if name.endswith(("running_mean", "running_var")):
            _close(bufs_m[name], buf, 1e-4, name)
            checked += 1
    assert checked > 0


def test_padded_mean_loss_ignores_the_padding_rows():
    from matten_amd.graphs import padded_mean_loss

    loss_fn = padded_mean_loss(lambda p, t: (p - t) ** 2, key=TARGET)
    assert loss_fn.wants_batch
    pred = torch.randn(7, 21, device=DEV, requires_grad=True)
    target = torch.randn(7, 21, device=DEV)
    junk = pred.detach().clone()
    junk[4:] = float("nan")
    junk.requires_grad_(True)
    batch = {"_amd_n_valid": torch.tensor([0, 0, 4], dtype=torch.int64, device=DEV)}
    want = torch.nn.functional.mse_loss(pred[:4], target[:4])
    got, got_junk = loss_fn({TARGET: pred}, target, batch), loss_fn({TARGET: junk}, target, batch)
    assert torch.allclose(got, want, rtol=1e-6, atol=0) and torch.equal(got, got_junk)
    got.backward()
    assert (pred.grad[4:] == 0).all() and pred.grad[:4].abs().min() > 0


# ----------------------------------------------------------------------------------------------------------------------
# 4. an epoch of bucketed, captured steps
# ----------------------------------------------------------------------------------------------------------------------
def _species_hparams(graphs):
    from matten_amd.data.graph import average_num_neighbors

    species = sorted({int(z) for g in graphs for z in g["atomic_numbers"].tolist()})
    return {"allowed_species": species, "average_num_neighbors": average_num_neighbors(graphs)}


def _model(ds, state=None):
    from matten_amd.model_factory.tfn_scalar_tensor import ScalarTensorModel

    torch.manual_seed(35)
    m = ScalarTensorModel(backbone_hparams=copy.deepcopy(LMAX2), dataset_hparams=ds)
    if state is not None:
        m.load_state_dict(state)
    return m.to(DEV)


def test_bucketed_epochs_follow_the_eager_steps():
    """100 crystals, batch_size 32 (three full batches and one of 4: K = 29), quanta (64, 2048), two epochs"""
    from matten.data.store import DeviceGraphStore
    from matten.dataset.structure_scalar_tensor import _DeviceLoader
    from matten_amd.graphs import BucketedTrainStep, padded_mean_loss
    from matten_amd.optim import FlatAdam

    graphs = list(golden_graphs())
    golden_store = DeviceGraphStore.from_graphs(graphs, DEV)
    ds = _species_hparams(graphs)
    state = copy.deepcopy(_model(ds).state_dict())
    kw = dict(batch_size=32, shuffle=True, seed=3, training=True)
    padded_loss = padded_mean_loss(lambda p, t: (p - t) ** 2, key=TARGET)

    def fresh():
        model = _model(ds, state).train()
        return model, FlatAdam(model.parameters(), lr=1e-2, weight_decay=1e-5, device_lr=True)

    def eager(loader, loss_of):
        model, opt = fresh()
        losses = []
        for _ in range(2):
            for batch in loader:
                loss = loss_of(model(dict(batch))[0], batch)
                opt.zero_grad()
                loss.backward()
                opt.step()
                losses.append(float(loss.detach()))
        return losses, [p.detach().clone() for p in model.parameters()]

    def run_bucketed(max_graphs):
        model, opt = fresh()
        step = BucketedTrainStep(model, opt, padded_loss, max_graphs=max_graphs, warmup=2, task_name=TARGET)
        loader = _DeviceLoader(golden_store, pad=(64, 2048), **kw)
        losses, buckets = [], []
        for _ in range(2):
            for batch in loader:
                assert batch["ptr"].shape[0] == 34 and batch["pos"].shape[0] % 64 == 0 and batch["edge_index"].shape[1] % 2048 == 0
                buckets.append(step.bucket(batch))
                losses.append(float(step.step(batch, batch[TARGET]).detach()))
        return step, losses, buckets, [p.detach().clone() for p in model.parameters()]

    want, p_want = eager(_DeviceLoader(golden_store, pad=(64, 2048), **kw), lambda preds, b: padded_loss(preds, b[TARGET], b))
    step, got, buckets, p_got = run_bucketed(8)
    print(f"buckets {buckets}\neager on the padded batches {want}\nbucketed {got}")
    print(f"captures {step.captures}, replays {step.replays}, eager steps {step.eager_steps}")
    assert len(want) == len(got) == 8 and want[0] != want[-1]
    assert got == want, "the same kernels on the same shapes"
    assert step.captures == len(set(buckets)) <= 8 and step.eager_steps == 0
    assert step.captures + step.replays + step.eager_steps == 8
    assert [len(i) for i in _DeviceLoader(golden_store, **kw).batch_indices()] == [32, 32, 32, 4]   # K = 29 is exercised
    assert len(set(buckets)) > 1

    plain, p_plain = eager(_DeviceLoader(golden_store, **kw),
                           lambda preds, b: torch.nn.functional.mse_loss(preds[TARGET], b[TARGET]))
    for i, (a, b) in enumerate(zip(got, plain)):
        _close(torch.tensor(a), torch.tensor(b), 2e-3, f"loss at step {i} against the unpadded eager step")
    for i, (a, b) in enumerate(zip(p_got, p_plain)):
        _close(a, b, 5e-3, f"parameter {i} after two epochs against the unpadded eager run")

    one, got_one, buckets_one, _ = run_bucketed(1)
    print(f"max_graphs=1: captures {one.captures}, replays {one.replays}, eager steps {one.eager_steps}; losses {got_one}")
    assert buckets_one == buckets and one.captures == 1
    assert one.eager_steps == sum(b != buckets[0] for b in buckets) and one.captures + one.replays + one.eager_steps == 8
    assert one.eager_steps > 0
    assert got_one == want
