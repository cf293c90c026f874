"""Radial networks of 1 to 4 hidden layers (invariant_layers) on the GPU: the _deep kernels against fp64 autograd of the
plain formula, the n_mid = 1 instantiations against the original entries bit for bit, whole models against the oracle, and
training (gradients against the oracle's autograd, reproducibility, FlatAdam, hipGraph)."""
import os

import pytest
import torch

from common import ATOMIC, LMAX2, PAPER, build_pair
from test_gpu_parity import _fcc, _fp64, _to64, close, close_blocks

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _close(got, want, rtol, what):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    scale = max(1e-12, want.abs().max().item())
    err = (got - want).abs().max().item()
    assert err <= rtol * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e}"


def _h2s_features(h2s):
    """h2s [E,2,32] fp16 hi/lo -> the 32 features in natural order (column g*8+kk holds 16*(kk>>2) + 4*g + (kk&3))"""
    v = h2s[:, 0].float() + h2s[:, 1].float() / 2048.0
    perm = torch.tensor([16 * (kk >> 2) + 4 * g + (kk & 3) for g in range(4) for kk in range(8)], device=h2s.device)
    out = torch.empty_like(v)
    out[:, perm] = v
    return out


# (1 edge and 48 columns: two-kernel adjoint; 330 columns: one-kernel adjoint where the depth admits it; 70 001 edges:
# several tiles per wave, ragged tail)
@pytest.mark.parametrize("n_mid", [0, 1, 2, 3])
@pytest.mark.parametrize("n_edges,W,nb", [(1, 48, 3), (37, 330, 8), (70001, 842, 16), (5000, 216, 8)])
def test_deep_radial_kernels_forward_and_adjoint(n_mid, n_edges, W, nb):
    from matten_amd import ops
    from matten_amd.nn._activation import normalize2mom_const
    from oracle.e3nn_lite.math import soft_one_hot_linspace

    g = torch.Generator().manual_seed(n_edges + W + 7 * n_mid)
    c = normalize2mom_const("silu")
    w0 = torch.randn(nb, 32, generator=g)
    wm = torch.randn(n_mid, 32, 32, generator=g)
    w2 = torch.randn(32, W, generator=g)
    lens = torch.rand(n_edges, generator=g, dtype=torch.float64) * 5.4 + 0.05
    if n_edges > 3:
        lens[1], lens[2] = 5.0, 6.5      # at / beyond the cutoff: zero embedding
    geom = torch.zeros(n_edges, 4, device=DEV)
    geom[:, 3] = lens.float().to(DEV)
    w_pad = (W + 15) // 16 * 16
    gout = torch.randn(n_edges, w_pad, generator=g).to(DEV)
    scales = (1.0 / nb**0.5, c / 32**0.5, c / 32**0.5)
    d0_, dm_, d2_ = (w.to(DEV) for w in (w0, wm, w2))

    def run():
        w0p, wmp, w2p = ops.radial_pack_deep(d0_, dm_, d2_, scales)
        hs = ops.radial_h_scale_deep(d0_, dm_, 0.0, 5.0, c)
        w = ops.radial_mlp_deep(geom, nb, 0.0, 5.0, w0p, wmp, w2p)
        wb = ops.radial_mlp_deep(geom, nb, 0.0, 5.0, w0p, wmp, w2p, out_dtype=torch.bfloat16)
        h2s = ops.radial_hidden_deep(geom, nb, 0.0, 5.0, w0p, wmp, hs)
        multi = ops.radial_hidden_multi_deep(geom, nb, 0.0, 5.0, [w0p, w0p * 0.5], [wmp, wmp], [hs, hs])
        grads = ops.radial_mlp_bwd_deep(geom, nb, 0.0, 5.0, w0p, wmp, w2p, W, gout, scales=scales)
        return dict(packed=(w0p, wmp, w2p), hs=hs, w=w, wb=wb, h2s=h2s, multi=multi, grads=grads)

    a, b = run(), run()
    for k in ("w", "wb", "h2s", "hs"):
        assert torch.equal(a[k], b[k]), k
    assert all(torch.equal(x, y) for x, y in zip(a["multi"], b["multi"]))
    assert all(torch.equal(x, y) for x, y in zip(a["grads"], b["grads"]))

    # fp64 autograd of the plain formula (e3nn FullyConnectedNet([nb] + L*[32] + [W], silu))
    ws = [w.double().requires_grad_(True) for w in (w0, *wm.unbind(0), w2)]
    x = soft_one_hot_linspace(lens.float().double(), 0.0, 5.0, nb, "bessel", True) * nb**0.5
    h = torch.nn.functional.silu(x @ (ws[0] / nb**0.5)) * c
    for w in ws[1:-1]:
        h = torch.nn.functional.silu(h @ (w / 32**0.5)) * c
    want = h @ (ws[-1] / 32**0.5)
    (want * gout[:, :W].cpu().double()).sum().backward()

    _close(a["w"][:, :W], want, 2e-6, "radial weights fp32")
    assert torch.all(a["w"][:, W:] == 0)
    _close(a["wb"][:, :W].float(), want, 8e-3, "radial weights bf16")
    s = float(a["hs"][0])
    assert 0.0 < s <= 1.0 and float(a["hs"][1]) == 1.0 / s
    h_last = h.detach() / c      # (the kernels fold the last activation's constant into the last layer)
    _close(_h2s_features(a["h2s"]), h_last * s, 2e-6, "last hidden layer (h2s)")
    _close(_h2s_features(a["multi"][0]), h_last * s, 2e-6, "last hidden layer (multi launch, first MLP)")
    w0p, wmp, _ = a["packed"]
    alone = ops.radial_hidden_deep(geom, nb, 0.0, 5.0, w0p * 0.5, wmp, a["hs"])
    _close(_h2s_features(a["multi"][1]), _h2s_features(alone), 1e-6, "multi launch, second MLP")
    d0, dm, d2 = a["grads"]
    assert dm.shape == (n_mid, 32, 32)
    got = [d0[:nb], *dm.unbind(0), d2[:, :W]]
    for i, (gw, w) in enumerate(zip(got, ws)):
        _close(gw, w.grad, 2e-5, f"dW layer{i}")

    # the host bound of nn.utils.RadialMLP and the device one pick the same power of two
    from matten_amd.nn.utils import RadialMLP

    mlp = RadialMLP([nb] + (n_mid + 1) * [32] + [W]).to(DEV)
    with torch.no_grad():
        for p, w in zip(mlp.weights(), (w0, *wm.unbind(0), w2)):
            p.copy_(w)
    assert torch.equal(mlp.h_scale(0.0, 5.0), a["hs"])

    if n_mid == 1:   # the _deep entries at n_mid = 1 run the original entries' kernels
        w0p1, w1p1, w2p1 = ops.radial_pack(d0_, dm_[0], d2_, scales)
        assert torch.equal(w0p1, w0p) and torch.equal(w1p1, wmp[0])
        assert torch.equal(ops.radial_mlp(geom, nb, 0.0, 5.0, w0p1, w1p1, w2p1), a["w"])
        assert torch.equal(ops.radial_mlp(geom, nb, 0.0, 5.0, w0p1, w1p1, w2p1, out_dtype=torch.bfloat16), a["wb"])
        assert torch.equal(ops.radial_hidden(geom, nb, 0.0, 5.0, w0p1, w1p1, a["hs"]), a["h2s"])
        m1 = ops.radial_hidden_multi(geom, nb, 0.0, 5.0, [w0p1, w0p1 * 0.5], [w1p1, w1p1], [a["hs"], a["hs"]])
        assert all(torch.equal(x, y) for x, y in zip(m1, a["multi"]))
        o0, o1, o2 = ops.radial_mlp_bwd(geom, nb, 0.0, 5.0, w0p1, w1p1, w2p1, W, gout, scales=scales)
        assert torch.equal(o0, d0) and torch.equal(o1, dm[0]) and torch.equal(o2, d2)


def test_deep_entries_refuse_depths_outside_the_envelope():
    from matten_amd import _lib

    lib = _lib.load()
    g = torch.zeros(16, 4, device=DEV)
    w = torch.zeros(4 * 32 * 32 + 64 * 32, device=DEV)
    out = torch.empty(16, 64, device=DEV)
    for n_mid in (-1, 4):
        assert lib.matten_radial_mlp_deep(g.data_ptr(), 16, 8, 0.0, 5.0, w.data_ptr(), 8, w.data_ptr(), n_mid, w.data_ptr(),
                                          32, 64, 1.0, out.data_ptr(), 0, None) == -1
        assert lib.matten_radial_h_scale_deep(w.data_ptr(), w.data_ptr(), n_mid, 8, 0.0, 5.0, 1.0, out.data_ptr(), None) == -1
    torch.cuda.synchronize()


def _n100(golden_dir, n=None):
    from matten_amd.data.graph import average_num_neighbors, crystal_graph
    from oracle.matten_ref.data import structures_from_json

    structs = structures_from_json(os.path.join(golden_dir, "example_crystal_elasticity_tensor_n100.json"))[:n]
    graphs = [crystal_graph(s["cart_coords"], s["lattice"], s["atomic_numbers"], 5.0) for s in structs]
    species = sorted({int(z) for s in structs for z in s["atomic_numbers"]})
    return graphs, {"allowed_species": species, "average_num_neighbors": average_num_neighbors(graphs)}


def _pair_out(ref, model, graphs, n_ref=None):
    """(HIP output of the whole batch, oracle fp32 and fp64 outputs of its first n_ref crystals)"""
    from matten_amd.data.graph import collate

    sub = graphs[:n_ref]
    with torch.no_grad():
        got = model(collate(graphs, device=DEV))[0]["elastic_tensor_full"]
        want = ref.decode(collate(sub))
        want64 = _fp64(ref).decode(_to64(collate(sub)))
    return got[: len(sub)], want, want64


@pytest.mark.parametrize("layers", [1, 3, 4])
@pytest.mark.parametrize("hp_name", ["lmax2", "paper"])
def test_deep_models_match_the_oracle(layers, hp_name, golden_dir):
    """fcc-64 crystals -- a batch above AGG_KM_MIN_ROWS nodes too (fused agg_linear + gate epilogue) -- and the n100
    sample (hub segments walked in pieces), every irrep block against the oracle's"""
    from matten_amd.nn import conv as pconv

    hp = dict({"lmax2": LMAX2, "paper": PAPER}[hp_name], invariant_layers=layers)
    graphs, ds = _fcc(pconv.AGG_KM_MIN_ROWS // 64 + 2)
    ref, model = build_pair(hp, ds, randomize_bn=True)
    assert all(m.n_mid == layers - 1 for m in model.modules() if type(m).__name__ == "RadialMLP")
    got, want, want64 = _pair_out(ref, model, graphs[:6])
    close_blocks(got, want, what=f"L={layers} fcc64 x6", want64=want64)
    got, want, want64 = _pair_out(ref, model, graphs, n_ref=3)
    close_blocks(got, want, what=f"L={layers} fcc64 x{len(graphs)} (first 3)", want64=want64)
    graphs, ds = _n100(golden_dir, 40)
    ref, model = build_pair(hp, ds, randomize_bn=True)
    got, want, want64 = _pair_out(ref, model, graphs)
    close_blocks(got, want, what=f"L={layers} n100[:40]", want64=want64)


@pytest.mark.parametrize("layers", [1, 3])
def test_deep_dead_output_view_and_path_kernels(layers, monkeypatch):
    """the dead-output view shares every hidden radial layer and slices the last one; MATTEN_TP_IMPL=paths (materialised
    w, reference column order) agrees with the fused kernel"""
    from matten_amd.data.graph import collate
    from matten_amd.nn import conv as pconv

    hp = dict(PAPER, invariant_layers=layers)
    graphs, ds = _fcc(3)
    ref, model = build_pair(hp, ds, randomize_bn=True)
    last = model.backbone._modules["conv_layer_last"]
    assert last._view is not None
    assert sum(p.numel() for p in last._view.parameters()) == last.lin1.weight.numel() + sum(
        w.numel() for w in last.tp.weight_nn.weights()[:-1])
    outs = {}
    for enabled in (True, False):
        monkeypatch.setattr(pconv, "DEAD_PATH_ELIMINATION", enabled)
        with torch.no_grad():
            outs[enabled] = model(collate(graphs, device=DEV))[0]["elastic_tensor_full"]
    close(outs[True], outs[False], 2e-6, "model output with / without dead-output elimination")
    with torch.no_grad():
        getattr(last.tp.weight_nn, f"layer{layers}").weight.mul_(0.5)
        getattr(ref.backbone.conv_layer_last.tp.weight_nn, f"layer{layers}").weight.mul_(0.5)
        got = model(collate(graphs, device=DEV))[0]["elastic_tensor_full"]
        want = ref.decode(collate(graphs))
    close_blocks(got, want, what="view after an update of the last radial layer", want64=_fp64(ref).decode(_to64(collate(graphs))))
    monkeypatch.setenv("MATTEN_TP_IMPL", "paths")
    _, paths = build_pair(hp, ds, randomize_bn=True)
    with torch.no_grad():
        got = paths(collate(graphs, device=DEV))[0]["elastic_tensor_full"]
    close_blocks(got, outs[True], what="paths vs fused", floor=2e-6)


@pytest.mark.parametrize("layers", [1, 3])
def test_deep_atomic_tensor_model(layers, golden_dir):
    from matten_amd.data.graph import collate

    graphs, ds = _n100(golden_dir, 12)
    ref, model = build_pair(dict(ATOMIC, invariant_layers=layers), ds, randomize_bn=True, atomic=True)
    cpu = collate(graphs)
    with torch.no_grad():
        want = ref.decode(cpu)
        got = model(dict(collate(graphs, device=DEV), atom_selector=(cpu["atomic_numbers"] % 2 == 0).to(DEV)),
                    task_name="nmr_tensor")[0]["nmr_tensor"]
    close(got, want, 2e-4, f"L={layers} per-atom irreps")


def test_huge_radial_weights_at_four_layers():
    from matten_amd.data.graph import collate

    graphs, ds = _fcc(4)
    ref, model = build_pair(dict(PAPER, invariant_layers=4), ds, randomize_bn=True)
    mlps = [m for m in model.modules() if type(m).__name__ == "RadialMLP"]
    with torch.no_grad():
        for k, p in ref.named_parameters():
            if ".weight_nn.layer4." in k:
                p.mul_(1e-16)   # keeps the per-edge weights O(1)
            elif ".weight_nn.layer" in k:
                p.mul_(1e4)
    model.load_state_dict(ref.state_dict(), strict=False)
    scales = [float(m.h_scale(0.0, 5.0)[0]) for m in mlps]
    assert all(0.0 < s < 2.0**-30 for s in scales), scales
    with torch.no_grad():
        want = ref.decode(collate(graphs))
        got = model(collate(graphs, device=DEV))[0]["elastic_tensor_full"]
    assert torch.isfinite(got).all()
    close_blocks(got, want, rtol=1e-4, what="radial hidden layers x 1e4 at L = 4")


def _train_grads(model, graphs, target):
    from matten_amd.data.graph import collate

    model.zero_grad(set_to_none=True)
    out = model(collate(graphs, device=DEV))[0]["elastic_tensor_full"]
    torch.nn.functional.mse_loss(out, target.to(DEV)).backward()
    return {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("layers", [1, 3])
@pytest.mark.parametrize("mode", ["fused", "paths"])
def test_deep_training_gradients_match_oracle_autograd(layers, mode, golden_dir, monkeypatch):
    """every parameter's gradient against the oracle's autograd, on the production kernel (fused) and on the path
    kernels; two evaluations are bit-identical"""
    import copy

    from matten_amd.data.graph import collate

    monkeypatch.setenv("MATTEN_TRAIN_TP", mode)
    graphs, ds = _n100(golden_dir, 8)
    target = torch.randn(len(graphs), 21, generator=torch.Generator().manual_seed(11))
    ref, model = build_pair(dict(LMAX2, invariant_layers=layers), ds, randomize_bn=True)
    ref.train(), model.train()
    bufs = copy.deepcopy({k: v.clone() for k, v in model.named_buffers()})
    g1 = _train_grads(model, graphs, target)
    with torch.no_grad():
        for k, v in model.named_buffers():
            v.copy_(bufs[k])
    g2 = _train_grads(model, graphs, target)
    assert g1.keys() == g2.keys() and all(torch.equal(g1[k], g2[k]) for k in g1), "gradients differ between two evaluations"
    torch.nn.functional.mse_loss(ref.decode(collate(graphs)), target).backward()
    radial = 0
    for k, p in ref.named_parameters():
        if p.grad is not None:
            _close(g1[k], p.grad, 3e-3, f"[{mode}] grad {k}")
            radial += ".weight_nn.layer" in k
    assert radial == 4 * (layers + 1)


@pytest.mark.parametrize("layers", [1, 3])
def test_deep_flat_adam_step(layers, golden_dir):
    from matten_amd.data.graph import collate
    from matten_amd.optim import FlatAdam

    graphs, ds = _n100(golden_dir, 8)
    _, model = build_pair(dict(LMAX2, invariant_layers=layers), ds, randomize_bn=True)
    model.train()
    opt = FlatAdam(model.parameters(), lr=1e-2, weight_decay=1e-5)
    batch, target = collate(graphs, device=DEV), torch.randn(len(graphs), 21, device=DEV)
    w = {k: p.detach().clone() for k, p in model.named_parameters()}
    losses = []
    for _ in range(3):
        loss = torch.nn.functional.mse_loss(model(dict(batch))[0]["elastic_tensor_full"], target)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss))
    assert all(torch.isfinite(torch.tensor(losses)))
    moved = [k for k, p in model.named_parameters() if ".weight_nn.layer" in k and not torch.equal(p, w[k])]
    assert len(moved) == 4 * (layers + 1)


def test_deep_hipgraph_forward_is_bit_identical_to_eager():
    from matten_amd.data import synthetic
    from matten_amd.data.graph import collate
    from matten_amd.graphs import GraphedForward

    ds = {"allowed_species": list(synthetic.FCC_METALS), "average_num_neighbors": 18.0}
    _, model = build_pair(dict(PAPER, invariant_layers=3), ds, randomize_bn=True)
    a, b = collate(synthetic.fcc64_graphs(4), device=DEV), collate(synthetic.fcc64_graphs(4, seed=99), device=DEV)
    g = GraphedForward(model, a)
    with torch.no_grad():
        for batch in (a, b, a):
            want = model(dict(batch))[0]["elastic_tensor_full"]
            assert torch.equal(g(batch), want)
