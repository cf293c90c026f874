"""
GPU parity: the HIP path (through the C ABI) against the CPU oracle on identical inputs.
Tolerances are fp32: the kernels reorder sums (CSR order, MFMA k-order, folded constants), so
agreement is to a few ulp of the accumulated magnitude, not bitwise; integer/index outputs are
compared exactly.
"""
import os

import numpy as np
import pytest
import torch

from common import EQUIV_TEST, LMAX2, PAPER, build_pair

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RTOL = 2e-4  # relative to the largest magnitude of the compared tensor


def close(got, want, rtol=RTOL, what=""):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    scale = max(1e-6, want.abs().max().item())
    err = (got - want).abs().max().item()
    assert err <= rtol * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e}"


BLOCK_RTOL = 2e-5  # end-to-end outputs: each irrep block against ITS OWN largest magnitude
ELASTIC_BLOCKS = ((0, 2, "2x0e"), (2, 12, "2x2e"), (12, 21, "4e"))   # CartesianTensor("ijkl=jikl=klij") = 2x0e+2x2e+4e


def close_blocks(got, want, blocks=ELASTIC_BLOCKS, rtol=BLOCK_RTOL, what="", want64=None, floor=0.0):
    """A weak path (the single 4e block is ~1e-2 of the 0e magnitude at random init) must not hide inside a tolerance
    taken from the whole tensor's maximum: every irrep block is compared relative to its own maximum.
    want64: the same oracle evaluated in fp64.  A block that (nearly) vanishes by crystal symmetry -- the pooled 2e / 4e
    parts of a cubic cell are sums of per-atom terms that cancel -- carries the rounding of those terms, not of its own
    size; there the fp32 oracle's own distance from the fp64 one sets the scale: the HIP path may be at most 4x as far
    from the fp64 result as the fp32 oracle is.  floor (where no fp64 oracle is at hand: committed fp32 golden
    vectors, two HIP paths against each other): the same allowance as a fraction of the whole tensor's maximum."""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert blocks[-1][1] == want.shape[-1]
    for lo, hi, name in blocks:
        scale = want[..., lo:hi].abs().max().item()
        tol = max(rtol * scale, floor * want.abs().max().item())
        ref = want[..., lo:hi]
        if want64 is not None:
            ref = want64.detach().cpu().double()[..., lo:hi]
            tol = max(tol, 4.0 * (want[..., lo:hi] - ref).abs().max().item())
        err = (got[..., lo:hi] - ref).abs().max().item()
        assert scale > 0 or err == 0, f"{what} block {name}: empty reference block"
        assert err <= tol, f"{what} block {name}: max err {err:.3e} vs block scale {scale:.3e} (rel {err / max(scale, 1e-300):.2e}, allowed {tol:.3e})"


def _fp64(ref):
    import copy

    return copy.deepcopy(ref).double()


def _to64(batch):
    return {k: (v.double() if isinstance(v, torch.Tensor) and v.is_floating_point() else v) for k, v in batch.items()}


def _fcc(n):
    from matten_amd.data import synthetic

    return synthetic.fcc64_graphs(n), {"allowed_species": list(synthetic.FCC_METALS), "average_num_neighbors": 18.0}


def _to(d, dev):
    return {k: v.to(dev) for k, v in d.items()}


def test_csr_is_stable_sort_by_dst():
    from matten_amd import ops
    from matten_amd.data.graph import collate

    graphs, _ = _fcc(3)
    b = collate(graphs, device=DEV)
    N = b["pos"].shape[0]
    perm, rowptr, src, err = ops.csr_build(b["edge_index"], N)
    ei = b["edge_index"].cpu()
    want_perm = torch.sort(ei[1], stable=True).indices
    assert torch.equal(perm.cpu().long(), want_perm)
    counts = torch.bincount(ei[1], minlength=N)
    assert torch.equal(rowptr.cpu().long()[1:] - rowptr.cpu().long()[:-1], counts)
    assert torch.equal(src.cpu().long(), ei[0][want_perm])
    assert int(err.item()) == 0


@pytest.mark.parametrize("n_nodes,n_edges", [(50, 600), (7, 2000), (1000, 300), (3, 1)])
def test_csr_counting_and_radix_builds_agree_with_a_stable_sort(n_nodes, n_edges):
    """sparse graphs (<= 64 edges per node on average) take the counting build, dense ones the radix sort: the same
    stable order either way; isolated nodes, a hub node and repeated edges included"""
    from matten_amd import ops

    g = torch.Generator().manual_seed(n_nodes * 7 + n_edges)
    ei = torch.randint(0, n_nodes, (2, n_edges), generator=g)
    ei[1, : n_edges // 3] = 0                                   # a hub: a third of the edges end in node 0
    perm, rowptr, src, err = ops.csr_build(ei.to(DEV), n_nodes)
    want_perm = torch.sort(ei[1], stable=True).indices
    assert torch.equal(perm.cpu().long(), want_perm)
    assert torch.equal(src.cpu().long(), ei[0][want_perm])
    assert torch.equal(rowptr.cpu().long(), torch.cat([torch.zeros(1, dtype=torch.long),
                                                       torch.bincount(ei[1], minlength=n_nodes).cumsum(0)]))
    assert int(err.item()) == 0


def test_csr_hub_segments_in_a_sparse_graph():
    """a sparse graph (counting build) with hub nodes far above the 16-lane ranking's threshold: the hub segments are
    sorted by a workgroup (csr.hip csr_hub_kernel) into the same stable order; lengths that are no power of two"""
    from matten_amd import ops

    g = torch.Generator().manual_seed(5)
    n_nodes, n_edges = 4000, 60000
    ei = torch.randint(0, n_nodes, (2, n_edges), generator=g)
    hub = torch.randperm(n_edges, generator=g)
    ei[1, hub[:20011]] = 17          # 20 011 + a few edges end in node 17
    ei[1, hub[20011:20011 + 2049]] = 3999
    ei[1, hub[23000:23000 + 4096]] = 0
    assert n_edges <= 64 * n_nodes
    perm, rowptr, src, err = ops.csr_build(ei.to(DEV), n_nodes)
    want_perm = torch.sort(ei[1], stable=True).indices
    assert torch.equal(perm.cpu().long(), want_perm)
    assert torch.equal(src.cpu().long(), ei[0][want_perm])
    assert int(err.item()) == 0


def test_csr_properties_at_full_size():
    """BASELINE configs[2] size (1000 fcc-64 crystals, 1.15 M edges): the CSR is a permutation, sorted by destination,
    stable inside a destination, and rowptr / src_sorted agree with it (size-independent properties, checked on device)"""
    from matten_amd import ops
    from matten_amd.data import synthetic
    from matten_amd.data.graph import collate

    graphs = synthetic.fcc64_graphs(64)
    b = collate([graphs[i % 64] for i in range(1000)], device=DEV)
    ei, N = b["edge_index"], b["pos"].shape[0]
    E = ei.shape[1]
    assert E == 1152 * 1000
    perm, rowptr, src, err = ops.csr_build(ei, N)
    p = perm.long()
    assert int(err.item()) == 0
    assert torch.equal(torch.sort(p).values, torch.arange(E, device=DEV))            # a permutation
    dst = ei[1][p]
    assert bool((dst[1:] >= dst[:-1]).all())                                          # sorted by destination
    same = dst[1:] == dst[:-1]
    assert bool((p[1:][same] > p[:-1][same]).all())                                   # stable inside a destination
    assert torch.equal(rowptr.long(), torch.cat([torch.zeros(1, dtype=torch.long, device=DEV),
                                                 torch.bincount(ei[1], minlength=N).cumsum(0)]))
    assert torch.equal(src.long(), ei[0][p])
    again = ops.csr_build(ei, N)
    assert all(torch.equal(x, y) for x, y in zip((perm, rowptr, src), again[:3]))     # atomics inside, same result


def test_csr_empty_and_bad_index():
    from matten_amd import ops

    perm, rowptr, src, err = ops.csr_build(torch.zeros(2, 0, dtype=torch.int64, device=DEV), 5)
    assert rowptr.cpu().tolist() == [0] * 6
    ei = torch.tensor([[0, 1, 2], [1, 7, 0]], dtype=torch.int64, device=DEV)
    *_, err = ops.csr_build(ei, 3)
    assert int(err.item()) & 1


def test_group_by_key_is_a_stable_sort():
    from matten_amd import ops

    g = torch.Generator().manual_seed(3)
    key = torch.randint(0, 7, (1000,), generator=g)
    order, seg, err = ops.group_by_key(key.to(DEV), 7)
    assert torch.equal(order.cpu().long(), torch.sort(key, stable=True).indices)
    assert seg.cpu().tolist() == [0] + torch.cumsum(torch.bincount(key, minlength=7), 0).tolist()
    assert int(err.item()) == 0
    *_, err = ops.group_by_key(torch.tensor([0, 9, 1], device=DEV), 3)
    assert int(err.item()) & 1
    _, seg, _ = ops.group_by_key(torch.zeros(0, dtype=torch.int64, device=DEV), 4)
    assert seg.cpu().tolist() == [0] * 5
    # both forms (<= 256 keys: counting; more: radix sort), ragged sizes, more keys than items, empty keys
    for n, n_keys in ((1, 3), (63, 100), (64, 2), (65, 256), (4097, 86), (5000, 300), (70000, 10)):
        key = torch.randint(0, n_keys, (n,), generator=g)
        key[key == 1] = 0                                   # key 1 stays empty
        order, seg, err = ops.group_by_key(key.to(DEV), n_keys)
        assert torch.equal(order.cpu().long(), torch.sort(key, stable=True).indices), (n, n_keys)
        assert seg.cpu().tolist() == [0] + torch.cumsum(torch.bincount(key, minlength=n_keys), 0).tolist()
        assert int(err.item()) == 0


def test_malformed_edge_index_raises_like_the_reference():
    """reference nn/_nequip.py:238 gathers pos[edge_index] and raises IndexError on an id outside the batch; the kernels
    clamp, so the backbone has to check: the check rides on the species check's host sync"""
    from matten_amd.data.graph import collate

    graphs, ds = _fcc(2)
    _, model = build_pair(dict(LMAX2, num_layers=1), ds, device=DEV)
    good = collate(graphs, device=DEV)
    with torch.no_grad():
        model(dict(good))  # a well-formed batch passes
        for bad_id in (good["pos"].shape[0], -1):
            bad = dict(good)
            bad["edge_index"] = good["edge_index"].clone()
            bad["edge_index"][0, 5] = bad_id
            with pytest.raises(IndexError, match="edge_index"):
                model(bad)


def test_edge_geometry_sh_and_bessel_vs_oracle():
    from matten_amd import ops
    from matten_amd.data.graph import collate
    from oracle.matten_ref import nn as rnn

    graphs, _ = _fcc(2)
    cpu = collate(graphs)
    ref = dict(cpu)
    rnn.SphericalHarmonicEdgeAttrs(4)(ref)
    rnn.EdgeLengthEmbedding(num_basis=8, start=0.0, end=5.0)(ref)
    g = _to(cpu, DEV)
    out = ops.edge_geom(g["pos"], g["edge_index"], g["edge_cell_shift"], g["cell"], g["batch"], None, 4, 8, 0.0, 5.0,
                        want_vectors=True, want_lengths=True, want_attrs=True, want_embedding=True)
    close(out["edge_vectors"], ref["edge_vectors"], 1e-6, "edge_vectors")
    close(out["edge_lengths"], ref["edge_lengths"], 1e-6, "edge_lengths")
    close(out["edge_attrs"], ref["edge_attrs"], 2e-6, "edge_attrs")
    close(out["edge_embedding"], ref["edge_embedding"], 5e-6, "edge_embedding")
    # perm == None means identity order
    close(out["sh_sorted"][:, :25], ref["edge_attrs"], 2e-6, "sh_sorted")
    close(out["geom_sorted"][:, 3], ref["edge_lengths"], 1e-6, "geom len")


def test_species_embedding_known_answer_and_errors():
    from matten_amd.nn.embedding import SpeciesEmbedding, _AtomicNumberToIndex

    # reference tests/nn/test_embedding.py:7-13 (runs anywhere)
    n2i = _AtomicNumberToIndex([6, 1, 8]).to(DEV)
    idx = n2i(torch.tensor([6, 6, 8, 1, 8], device=DEV))
    assert idx.dtype == torch.long and idx.cpu().tolist() == [1, 1, 2, 0, 2]

    emb = SpeciesEmbedding(embedding_dim=16, allowed_species=[6, 1, 8], materialize=True).to(DEV)
    data = emb({"atomic_numbers": torch.tensor([6, 6, 8, 1, 8], device=DEV)})
    assert data["species_index"].cpu().tolist() == [1, 1, 2, 0, 2]
    want = torch.nn.functional.one_hot(torch.tensor([1, 1, 2, 0, 2]), 3).float()
    assert torch.equal(data["node_attrs"].cpu(), want)
    close(data["node_features"], want @ emb.linear.weight.cpu().T + emb.linear.bias.cpu(), 1e-6, "embedding")
    with pytest.raises(RuntimeError, match="Invalid atomic numbers"):
        emb({"atomic_numbers": torch.tensor([6, 9], device=DEV)})
    with pytest.raises(RuntimeError, match="got invalid atomic numbers `7`"):
        emb({"atomic_numbers": torch.tensor([6, 7], device=DEV)})


@pytest.mark.parametrize("w_out", [80, 452, 842, 1216])
def test_radial_mlp_mfma_vs_oracle(w_out):
    from matten_amd.nn.utils import RadialMLP
    from oracle.e3nn_lite.math import soft_one_hot_linspace
    from oracle.e3nn_lite.nn import FullyConnectedNet

    torch.manual_seed(w_out)
    E = 1000 + w_out % 7  # ragged tail
    ref = FullyConnectedNet([8, 32, 32, w_out], act=torch.nn.functional.silu)
    mlp = RadialMLP([8, 32, 32, w_out], act="silu")
    mlp.load_state_dict(ref.state_dict())
    mlp = mlp.to(DEV)
    r = torch.rand(E) * 5.5 + 0.3  # includes lengths beyond the cutoff (embedding == 0)
    geom = torch.zeros(E, 4)
    geom[:, 3] = r
    emb = soft_one_hot_linspace(r, 0.0, 5.0, 8, basis="bessel", cutoff=True) * 8**0.5
    want = ref(emb)
    got = mlp(geom.to(DEV), 8, 0.0, 5.0)
    assert got.shape[1] % 16 == 0
    close(got[:, :w_out], want, 5e-5, "radial mlp")


@pytest.mark.parametrize("hp_name", ["paper", "lmax2"])
def test_conv_layers_vs_oracle(hp_name):
    """Layer-by-layer node features of the backbone on fcc-64 crystals."""
    from matten_amd.data.graph import collate

    hp = {"paper": PAPER, "lmax2": LMAX2}[hp_name]
    graphs, ds = _fcc(2)
    ref, model = build_pair(hp, ds, randomize_bn=True)
    cpu = collate(graphs)
    gpu = collate(graphs, device=DEV)
    from matten_amd.nn import conv as pconv

    with torch.no_grad():
        for (name, rmod), (_, pmod) in zip(ref.backbone.named_children(), model.backbone.named_children()):
            cpu = rmod(cpu)
            gpu = pmod(gpu)
            if "node_features" in cpu:
                want = cpu["node_features"]
                if gpu.get(pconv.KEPT_ONLY):   # the last conv layer ran for the irreps its consumer reads only
                    want = want[:, _kept_columns(model.backbone._modules["conv_layer_last"])]
                close(gpu["node_features"], want, RTOL, f"{hp_name}:{name}:node_features")
        close(gpu["my_model_output"], cpu["my_model_output"], RTOL, "pooled")


def _kept_columns(conv):
    """columns of the full output row of ``conv`` that its inference view emits, in the view's order"""
    from matten_amd.data.irreps import DataKey

    full = conv.irreps_out[DataKey.NODE_FEATURES]
    offs = full.offsets()
    cols = []
    for m, ir in conv._view.sc.irreps_out:
        (i,) = [i for i, (m2, ir2) in enumerate(full) if ir2 == ir and m2 == m]
        cols += list(range(offs[i], offs[i] + m * ir.dim))
    return torch.as_tensor(cols)


@pytest.mark.parametrize("hp_name", ["paper", "lmax2"])
def test_dead_output_elimination_matches_the_full_layer(hp_name, monkeypatch):
    """Inference runs the last conv layer for the irreps the output head reads only (model_factory.eliminate_dead_outputs):
    its node features equal the kept columns of the full layer's, the model output is unchanged, the full layer is
    compared with the oracle column for column, and neither the parameters nor the state_dict know about the view."""
    from matten_amd.data.graph import collate
    from matten_amd.nn import conv as pconv

    hp = {"paper": PAPER, "lmax2": LMAX2}[hp_name]
    graphs, ds = _fcc(3)
    ref, model = build_pair(hp, ds, randomize_bn=True)
    last = model.backbone._modules["conv_layer_last"]
    assert last._view is not None and not any("view" in k for k in model.state_dict())
    assert sum(p.numel() for p in last._view.parameters()) == last.lin1.weight.numel() + sum(
        getattr(last.tp.weight_nn, f"layer{i}").weight.numel() for i in (0, 1))   # shared modules only
    kept = _kept_columns(last).to(DEV)
    assert 0 < kept.numel() < last.irreps_out["node_features"].dim
    if hp_name == "paper":
        # the view's vector / l = 2 / l = 4 input blocks keep even-l3 couplings only: they run on the ALTERNATIVE coupling groups
        # (plan._ALT_GROUPS: one entry per block chunk, no dead weight columns), the full layer on the regular ones -- this test
        # compares the two families of generated code column for column
        from matten_amd import plan as mplan

        def kinds(p):
            e = np.asarray(p.group_entries).reshape(-1, 32)
            return {((int(k) & 255) // mplan.TP_KIND_STRIDE, (int(k) & 255) % mplan.TP_KIND_STRIDE) for k in e[:, 0] if k >= 0}
        alt = {(l1, gi) for (l1, gi) in kinds(last._view.tp.plan) if gi >= mplan.TP_GROUPS_REGULAR[l1]}
        assert {l1 for l1, _ in alt} == {1, 2, 3, 4} and not any(gi >= mplan.TP_GROUPS_REGULAR[l1] for l1, gi in kinds(last.tp.plan))

    def run(enabled):
        monkeypatch.setattr(pconv, "DEAD_PATH_ELIMINATION", enabled)
        data = collate(graphs, device=DEV)
        with torch.no_grad():
            for name, mod in model.backbone.named_children():
                data = mod(data)
                if name == "conv_layer_last":
                    feats = data["node_features"].clone()
                    assert bool(data.get(pconv.KEPT_ONLY, False)) == enabled
        return feats, data["my_model_output"].clone()

    f_on, out_on = run(True)
    f_off, out_off = run(False)
    assert f_on.shape == (f_off.shape[0], kept.numel()) and f_off.shape[1] == last.irreps_out["node_features"].dim
    close(f_on, f_off[:, kept], 2e-6, "kept columns of the last conv layer")
    close(out_on, out_off, 2e-6, "model output with / without dead-output elimination")
    with torch.no_grad():
        cpu = collate(graphs)
        for name, rmod in ref.backbone.named_children():
            cpu = rmod(cpu)
            if name == "conv_layer_last":
                close(f_off, cpu["node_features"], RTOL, "full last conv layer vs oracle")
    # a parameter update reaches the view (index-selected copies follow the parameters' versions)
    with torch.no_grad():
        last.lin2.weight.mul_(1.5)
        last.tp.weight_nn.layer2.weight.mul_(0.5)
    f_on2, out_on2 = run(True)
    f_off2, out_off2 = run(False)
    close(f_on2, f_off2[:, kept], 2e-6, "kept columns after a parameter update")
    assert (out_on2 - out_on).abs().max().item() > 0
    # under autograd the view runs too (index_select nodes): the kept blocks' gradients equal the full layer's, the
    # weights of paths that never reach the loss get exact zeros -- as from the reference's autograd
    model.train()
    target = torch.randn(len(graphs), 21, generator=torch.Generator().manual_seed(2)).to(DEV)
    grads = {}
    for enabled in (True, False):
        monkeypatch.setattr(pconv, "DEAD_PATH_ELIMINATION", enabled)
        model.zero_grad(set_to_none=True)
        bufs = {k: v.clone() for k, v in model.named_buffers()}
        data = collate(graphs, device=DEV)
        for name, mod in model.backbone.named_children():
            data = mod(data)
            if name == "conv_layer_last":
                assert bool(data.get(pconv.KEPT_ONLY, False)) == enabled
                assert data["node_features"].shape[1] == (kept.numel() if enabled else f_off.shape[1])
        out = model.extra_layers_dict["out_layer"](data["my_model_output"])
        torch.nn.functional.mse_loss(out, target).backward()
        grads[enabled] = {k: p.grad.clone() for k, p in model.named_parameters()}
        with torch.no_grad():
            for k, v in model.named_buffers():
                v.copy_(bufs[k])
    assert grads[True].keys() == grads[False].keys()
    for k in grads[True]:
        close(grads[True][k], grads[False][k], 2e-5, f"grad {k} with / without dead-output elimination")
    w2 = grads[True]["backbone.conv_layer_last.tp.weight_nn.layer2.weight"]
    dead = (grads[False]["backbone.conv_layer_last.tp.weight_nn.layer2.weight"] == 0).all(dim=0)
    assert 0 < int(dead.sum()) < w2.shape[1] and bool((w2[:, dead] == 0).all())


def _run_pair(ref, model, graphs):
    from matten_amd.data.graph import collate

    with torch.no_grad():
        want = ref.decode(collate(graphs))
        preds, _ = model(collate(graphs, device=DEV))
    return preds["elastic_tensor_full"], want


def _want64(ref, graphs):
    from matten_amd.data.graph import collate

    with torch.no_grad():
        return _fp64(ref).decode(_to64(collate(graphs)))


def test_config3_fcc64_end_to_end():
    graphs, ds = _fcc(8)
    ref, model = build_pair(PAPER, ds, randomize_bn=True)
    got, want = _run_pair(ref, model, graphs)
    assert got.shape == (8, 21)
    close_blocks(got, want, what="fcc64 [B,21]", want64=_want64(ref, graphs))


def test_config2_n100_end_to_end(golden_dir):
    from matten_amd.data.graph import average_num_neighbors, crystal_graph
    from oracle.matten_ref.data import structures_from_json

    structs = structures_from_json(os.path.join(golden_dir, "example_crystal_elasticity_tensor_n100.json"))
    graphs = [crystal_graph(s["cart_coords"], s["lattice"], s["atomic_numbers"], 5.0) for s in structs]
    species = sorted({int(z) for s in structs for z in s["atomic_numbers"]})
    assert len(species) == 73 and sum(g["edge_index"].shape[1] for g in graphs) == 14380
    ds = {"allowed_species": species, "average_num_neighbors": average_num_neighbors(graphs)}
    assert abs(ds["average_num_neighbors"] - 30.4017) < 1e-3
    ref, model = build_pair(PAPER, ds, randomize_bn=True)
    got, want = _run_pair(ref, model, graphs)
    assert got.shape == (100, 21)
    close_blocks(got, want, what="n100 [B,21]", want64=_want64(ref, graphs))


def test_gpu_matches_committed_golden_vectors(golden_dir):
    """tests/golden/oracle_golden.npz (make_golden.py: the TeO fixture with the reference's test hparams and seed 35,
    the first six n100 crystals with the paper hparams) against the HIP path -- the committed numbers, not an oracle
    evaluated in this process."""
    from matten_amd.data.graph import collate, crystal_graph
    from matten_amd.model_factory.tfn_scalar_tensor import ScalarTensorModel
    from matten_amd.utils import CartesianTensorWrapper
    from oracle.matten_ref.data import structures_from_json
    from oracle.matten_ref.model import ScalarTensorOracle

    golden = np.load(os.path.join(golden_dir, "oracle_golden.npz"))

    def hip_model(hp, ds):
        # same construction order and seed as make_golden.py, weights moved over by state_dict
        torch.manual_seed(35)
        ref = ScalarTensorOracle(dict(hp), ds).eval()
        m = ScalarTensorModel(backbone_hparams=dict(hp), dataset_hparams=ds)
        missing, _ = m.load_state_dict(ref.state_dict(), strict=False)
        assert not missing
        return m.to(DEV).eval()

    s = structures_from_json(os.path.join(golden_dir, "elastic_tensor_one.json"))[0]
    g = crystal_graph(s["cart_coords"], s["lattice"], s["atomic_numbers"], 5.0)
    assert np.array_equal(g["edge_index"].numpy(), golden["teo_edge_index"])
    model = hip_model(EQUIV_TEST, {"allowed_species": [8, 52]})
    with torch.no_grad():
        cart = model(collate([g], device=DEV))[0]["elastic_tensor_full"]      # output_format "cartesian": [1,3,3,3,3]
    want = torch.as_tensor(golden["teo_cartesian"])
    assert cart.shape == want.shape == (1, 3, 3, 3, 3)
    ct = CartesianTensorWrapper("ijkl=jikl=klij")
    close_blocks(ct.from_cartesian(cart.cpu().double()), ct.from_cartesian(want.double()), what="golden TeO (irreps view)", floor=1e-6)
    close(cart, want, 2e-5, "golden TeO Cartesian")

    structs = structures_from_json(os.path.join(golden_dir, "example_crystal_elasticity_tensor_n100.json"))[:6]
    graphs = [crystal_graph(t["cart_coords"], t["lattice"], t["atomic_numbers"], 5.0) for t in structs]
    ds = {"allowed_species": [int(z) for z in golden["n100_species"]],
          "average_num_neighbors": float(golden["n100_avg_num_neigh"])}
    model = hip_model(PAPER, ds)
    with torch.no_grad():
        got = model(collate(graphs, device=DEV))[0]["elastic_tensor_full"]
    close_blocks(got, torch.as_tensor(golden["n100_first6_irreps"]), what="golden n100 first six", floor=1e-6)


def test_component_major_conv_matches_mul_ir_path(monkeypatch, golden_dir):
    """The production conv writes its neighbour sums component-major and applies lin2 with matten_agg_linear
    (plan.plan_agg_linear); MATTEN_AGG_LAYOUT=mul_ir keeps the reference's [channel][component] row and the
    segment-table linear.  Same weights, same batch: per conv layer and end to end the two agree to fp32 rounding, on
    the fcc batch (10 species, whole 128-row workgroups) and on the n100 sample (73 species, ragged species groups,
    groups smaller than one wave)."""
    from matten_amd.data.graph import average_num_neighbors, collate, crystal_graph
    from matten_amd.model_factory.tfn_scalar_tensor import ScalarTensorModel
    from oracle.matten_ref.data import structures_from_json

    structs = structures_from_json(os.path.join(golden_dir, "example_crystal_elasticity_tensor_n100.json"))[:40]
    g100 = [crystal_graph(s["cart_coords"], s["lattice"], s["atomic_numbers"], 5.0) for s in structs]
    ds100 = {"allowed_species": sorted({int(z) for s in structs for z in s["atomic_numbers"]}),
             "average_num_neighbors": average_num_neighbors(g100)}
    gf, dsf = _fcc(5)
    import matten_amd.nn.conv as conv_mod
    monkeypatch.setattr(conv_mod, "AGG_KM_MIN_ROWS", 0)      # production takes the new path from 8192 rows: force it here
    monkeypatch.setattr(conv_mod, "GATE_FUSE", False)        # (this test looks at lin2's own output, before the Gate)
    # (EQUIV_TEST: the reference's own test hparams -- 8 / 4-channel high-l blocks incl. 4x4o, no BatchNorm, Cartesian output)
    for graphs, ds, hp in ((gf, dsf, PAPER), (g100, ds100, PAPER), (g100, ds100, LMAX2), (g100, ds100, EQUIV_TEST)):
        torch.manual_seed(11)
        monkeypatch.setenv("MATTEN_AGG_LAYOUT", "km")
        new = ScalarTensorModel(backbone_hparams=dict(hp), dataset_hparams=ds).to(DEV).eval()
        monkeypatch.setenv("MATTEN_AGG_LAYOUT", "mul_ir")
        old = ScalarTensorModel(backbone_hparams=dict(hp), dataset_hparams=ds).to(DEV).eval()
        old.load_state_dict(new.state_dict())
        convs_new = [m for m in new.modules() if type(m).__name__ == "PointConv"]
        convs_old = [m for m in old.modules() if type(m).__name__ == "PointConv"]
        assert all(m.agg_plan is not None for m in convs_new) and all(m.agg_plan is None for m in convs_old)
        feats = {}
        for tag, convs in (("new", convs_new), ("old", convs_old)):
            for i, m in enumerate(convs):
                m.register_forward_hook(lambda mod, inp, out, key=(tag, i): feats.__setitem__(key, out["node_features"].clone()))
        with torch.no_grad():
            b = collate(graphs, device=DEV)
            y_new = new(dict(b))[0]["elastic_tensor_full"]
            y_old = old(dict(b))[0]["elastic_tensor_full"]
        for i in range(len(convs_new)):
            close(feats[("new", i)], feats[("old", i)], 2e-6, f"conv layer {i} node features")
        if y_new.dim() == 2:
            close_blocks(y_new, y_old, rtol=5e-6, what="end to end", floor=5e-7)
        else:
            close(y_new, y_old, 2e-6, "end to end (Cartesian)")


@pytest.mark.parametrize("hp_name", ["paper", "lmax2", "equiv"])
def test_gate_and_batchnorm_inside_the_lin2_kernel(monkeypatch, golden_dir, hp_name):
    """matten_agg_linear_gate: the conv layer's Gate and eval-mode BatchNorm applied in lin2's epilogue (gate scalars kept
    in registers, exchanged by ds_bpermute) against the separate lin2 + gate kernels, per gated layer and end to end,
    with randomised BatchNorm statistics / without BatchNorm; ragged species groups, groups smaller than one wave."""
    from matten_amd.data.graph import average_num_neighbors, collate, crystal_graph
    from matten_amd.model_factory.tfn_scalar_tensor import ScalarTensorModel
    from oracle.matten_ref.data import structures_from_json
    import matten_amd.nn.conv as conv_mod

    hp = {"paper": PAPER, "lmax2": LMAX2, "equiv": EQUIV_TEST}[hp_name]
    structs = structures_from_json(os.path.join(golden_dir, "example_crystal_elasticity_tensor_n100.json"))[:40]
    graphs = [crystal_graph(s["cart_coords"], s["lattice"], s["atomic_numbers"], 5.0) for s in structs]
    ds = {"allowed_species": sorted({int(z) for s in structs for z in s["atomic_numbers"]}),
          "average_num_neighbors": average_num_neighbors(graphs)}
    monkeypatch.setattr(conv_mod, "AGG_KM_MIN_ROWS", 0)
    torch.manual_seed(5)
    model = ScalarTensorModel(backbone_hparams=dict(hp), dataset_hparams=ds).to(DEV).eval()
    gen = torch.Generator().manual_seed(6)
    with torch.no_grad():
        for k, b in model.named_buffers():
            if k.endswith("running_mean"):
                b.copy_(0.1 * torch.randn(b.shape, generator=gen))
            if k.endswith("running_var"):
                b.copy_(0.5 + torch.rand(b.shape, generator=gen))
        for k, p in model.named_parameters():
            if ".norm.n.weight" in k:
                p.copy_(0.5 + torch.rand(p.shape, generator=gen))
            if ".norm.n.bias" in k:
                p.copy_(0.1 * torch.randn(p.shape, generator=gen))
    layers = [m for m in model.modules() if type(m).__name__ == "PointConvWithActivation"]
    assert layers and all(m._gate_fuse_args(torch.device(DEV)) is not None for m in layers)
    feats = {}
    outs = {}
    for fused in (True, False):
        monkeypatch.setattr(conv_mod, "GATE_FUSE", fused)
        hooks = [m.register_forward_hook(lambda mod, inp, out, key=(fused, i): feats.__setitem__(key, out["node_features"].clone()))
                 for i, m in enumerate(layers)]
        with torch.no_grad():
            outs[fused] = model(collate(graphs, device=DEV))[0]["elastic_tensor_full"]
        for h in hooks:
            h.remove()
    for i in range(len(layers)):
        close(feats[(True, i)], feats[(False, i)], 2e-6, f"{hp_name}: activated features of gated layer {i}")
    if outs[True].dim() == 2:
        close_blocks(outs[True], outs[False], rtol=5e-6, floor=5e-7, what=f"{hp_name}: end to end")
    else:
        close(outs[True], outs[False], 2e-6, f"{hp_name}: end to end (Cartesian)")


def test_huge_radial_weights_stay_inside_the_fp16_split_range():
    """The fused kernel feeds the hidden radial features to the matrix cores as fp16 hi/lo pieces (csrc/tp_fused.hip):
    a checkpoint whose first two radial layers are 10^4 x larger (hidden features ~10^8, far beyond fp16's 65504) must
    still give the oracle's numbers.  The host bounds |h2| from the weights and hands the kernels a power-of-two scale
    (RadialMLP.h_scale); for the normally scaled model that scale is exactly 1."""
    from matten_amd.data.graph import collate

    graphs, ds = _fcc(4)
    ref, model = build_pair(PAPER, ds, randomize_bn=True)
    mlps = [m for m in model.modules() if type(m).__name__ == "RadialMLP"]
    assert len(mlps) == 4 and all(float(m.h_scale(0.0, 5.0)[0]) == 1.0 for m in mlps)
    with torch.no_grad():
        for k, p in ref.named_parameters():
            if ".weight_nn.layer0." in k or ".weight_nn.layer1." in k:
                p.mul_(1e4)
            elif ".weight_nn.layer2." in k:
                p.mul_(1e-8)   # keeps the per-edge weights O(1): four conv layers of 10^12 would leave fp32 itself
    model.load_state_dict(ref.state_dict(), strict=False)
    scales = [float(m.h_scale(0.0, 5.0)[0]) for m in mlps]
    assert all(0.0 < s < 2.0**-10 for s in scales), scales
    with torch.no_grad():
        want = ref.decode(collate(graphs))
        got = model(collate(graphs, device=DEV))[0]["elastic_tensor_full"]
    assert torch.isfinite(got).all()
    close_blocks(got, want, rtol=1e-4, what="radial hidden layers x 1e4")


def test_config1_si_diamond_cubic_symmetry():
    """README Si cell (reference README.md:34-40): E=56, and the prediction has cubic structure."""
    from matten_amd.data.graph import crystal_graph
    from matten_amd.utils import CartesianTensorWrapper

    a = 5.46
    lat = np.array([[0, a / 2, a / 2], [a / 2, 0, a / 2], [a / 2, a / 2, 0]])
    pos = np.array([[0.0, 0.0, 0.0], [0.25, 0.25, 0.25]]) @ lat
    g = crystal_graph(pos, lat, [14, 14], 5.0)
    assert g["edge_index"].shape[1] == 56
    ds = {"allowed_species": [14], "average_num_neighbors": 28.0}
    ref, model = build_pair(PAPER, ds)
    got, want = _run_pair(ref, model, [g])
    close_blocks(got, want, what="Si [1,21]", want64=_want64(ref, [g]))
    C = CartesianTensorWrapper("ijkl=jikl=klij").to_cartesian(got)[0].cpu().double()
    scale = C.abs().max().item()
    c11, c22, c33 = C[0, 0, 0, 0], C[1, 1, 1, 1], C[2, 2, 2, 2]
    c12, c13, c23 = C[0, 0, 1, 1], C[0, 0, 2, 2], C[1, 1, 2, 2]
    c44, c55, c66 = C[1, 2, 1, 2], C[0, 2, 0, 2], C[0, 1, 0, 1]
    for x, y in [(c11, c22), (c11, c33), (c12, c13), (c12, c23), (c44, c55), (c44, c66)]:
        assert abs(x - y) <= 1e-4 * scale


def test_reference_equivariance_test_on_gpu(golden_dir):
    """reference tests/model/test_tfn_tensor.py:98-139, run through the HIP backbone."""
    from matten_amd.data.graph import collate, crystal_graph
    from matten_amd.utils import ToCartesian
    from oracle.e3nn_lite import o3 as ro3
    from oracle.matten_ref.data import structures_from_json

    s = structures_from_json(os.path.join(golden_dir, "elastic_tensor_one.json"))[0]
    torch.manual_seed(35)
    Q = ro3.rand_matrix().double()
    g1 = crystal_graph(s["cart_coords"], s["lattice"], s["atomic_numbers"], 5.0)
    g2 = crystal_graph(s["cart_coords"] @ Q.numpy().T, s["lattice"] @ Q.numpy().T, s["atomic_numbers"], 5.0)
    assert g1["edge_index"].shape[1] == 252
    ref, model = build_pair(EQUIV_TEST, {"allowed_species": [8, 52]})
    tc = ToCartesian("ijkl=jikl=klij")
    with torch.no_grad():
        o1 = tc(model.backbone(collate([g1], device=DEV))["my_model_output"])[0].cpu()
        o2 = tc(model.backbone(collate([g2], device=DEV))["my_model_output"])[0].cpu()
        w1 = ref.backbone(collate([g1]))["my_model_output"]
    close_blocks(model.backbone(collate([g1], device=DEV))["my_model_output"], w1, what="TeO fixture", floor=1e-6)
    assert torch.allclose(o1, o1.swapaxes(0, 1))
    assert torch.allclose(o1, o1.swapaxes(2, 3))
    assert torch.allclose(o1, o1.swapaxes(0, 2).swapaxes(1, 3))
    Qf = Q.float()
    x = torch.einsum("im,jn,kp,lq,mnpq->ijkl", Qf, Qf, Qf, Qf, o1)
    assert torch.allclose(x, o2, atol=1e-4)


def test_edge_order_invariance_and_determinism():
    """Permuting the edge list must not change the result beyond fp32 reordering; same input twice is bitwise equal."""
    from matten_amd.data.graph import collate

    graphs, ds = _fcc(2)
    _, model = build_pair(PAPER, ds)
    b = collate(graphs, device=DEV)
    with torch.no_grad():
        y1 = model.decode(dict(b))["elastic_tensor_full"]
        y1b = model.decode(dict(b))["elastic_tensor_full"]
        E = b["edge_index"].shape[1]
        p = torch.randperm(E, generator=torch.Generator().manual_seed(0)).to(DEV)
        b2 = dict(b)
        b2["edge_index"] = b["edge_index"][:, p].contiguous()
        b2["edge_cell_shift"] = b["edge_cell_shift"][p].contiguous()
        y2 = model.decode(b2)["elastic_tensor_full"]
    assert torch.equal(y1, y1b)
    close(y2, y1, 1e-4, "edge permutation")


def test_cpu_tensors_are_rejected_loudly():
    from matten_amd import _lib
    from matten_amd.data.graph import collate

    graphs, ds = _fcc(1)
    _, model = build_pair(PAPER, ds)
    with pytest.raises(_lib.MattenHipError, match="no CPU fallback"):
        model.backbone(collate(graphs))


@pytest.mark.parametrize("per_node_norm", [False, True])
def test_tp_kernels_agree_and_match_oracle(per_node_norm, monkeypatch):
    """The block-fused and per-path kernels (literal CG) and the table-driven kernel are three
    implementations of the same operator: all must match the oracle's TensorProduct + scatter on ragged
    n100 crystals."""
    from matten_amd import ops, plan as mplan
    from matten_amd.data.graph import collate, crystal_graph
    from matten_amd.nn._tables import DeviceTables
    from matten_amd.o3 import Irreps
    from oracle.e3nn_lite.scatter import scatter
    from oracle.matten_ref import nn as rnn
    from oracle.matten_ref.data import structures_from_json

    structs = structures_from_json(os.path.join(os.path.dirname(__file__), "golden",
                                                "example_crystal_elasticity_tensor_n100.json"))[:12]
    graphs = [crystal_graph(s["cart_coords"], s["lattice"], s["atomic_numbers"], 5.0) for s in structs]
    cpu = collate(graphs)
    irreps_in = "32x0o+32x0e+16x1o+16x1e+4x2o+4x2e+2x3o+2x3e+2x4e"
    sh = Irreps.spherical_harmonics(4)
    torch.manual_seed(3)
    ref_tp = rnn.UVUTensorProduct(irreps_in, str(sh), irreps_in, mlp_input_size=8, mlp_hidden_size=32,
                                  mlp_num_hidden_layers=2, mlp_activation=torch.nn.functional.silu)
    N, E = cpu["pos"].shape[0], cpu["edge_index"].shape[1]
    x = torch.randn(N, ref_tp.tp.irreps_in1.dim)
    w = torch.randn(E, ref_tp.tp.weight_numel)
    ref = dict(cpu)
    rnn.SphericalHarmonicEdgeAttrs(4)(ref)
    msg = ref_tp.tp(x[cpu["edge_index"][0]], ref["edge_attrs"], w)
    want = scatter(msg, cpu["edge_index"][1], dim_size=N)
    want = want / (cpu["num_neigh"].reshape(-1, 1) ** 0.5 if per_node_norm else 18.0**0.5)

    p = mplan.plan_uvu(irreps_in, sh, irreps_in)
    assert p.weight_numel == ref_tp.tp.weight_numel and p.d_mid == msg.shape[1]
    t = DeviceTables(entries=p.path_entries, unit_start=p.unit_start, gentries=p.group_entries, gumap=p.fused_unit_map)
    g = _to(cpu, DEV)
    perm, rowptr, src, _ = ops.csr_build(g["edge_index"], N)
    geo = ops.edge_geom(g["pos"], g["edge_index"], g["edge_cell_shift"], g["cell"], g["batch"], perm, 4)
    w_pad = (p.weight_numel + 15) // 16 * 16
    w_sorted = torch.zeros(E, w_pad, device=DEV)
    w_sorted[:, : p.weight_numel] = w.to(DEV)[perm.long()]
    avg = 0.0 if per_node_norm else 18.0
    nn_ = g["num_neigh"] if per_node_norm else None
    a = ops.tp_paths(x.to(DEV), w_sorted, geo["sh_sorted"], rowptr, src, t.get("entries", DEV),
                     t.get("unit_start", DEV), p.units_per_tile, p.d_mid, avg, nn_)
    cols = torch.as_tensor(p.fused_cols, device=DEV)
    # fused: w = h2 @ W2 evaluated inside the kernel; feed it a rank-deficient factorisation of the same w
    h2 = torch.randn(E, 32, device=DEV)
    w2 = torch.randn(32, p.weight_numel, device=DEV) / 32**0.5
    w_lr = h2 @ w2                                      # [E(original order), W] reference-layout weights
    msg_lr = ref_tp.tp(x[cpu["edge_index"][0]], ref["edge_attrs"], w_lr.cpu())
    want_lr = scatter(msg_lr, cpu["edge_index"][1], dim_size=N)
    want_lr = want_lr / (cpu["num_neigh"].reshape(-1, 1) ** 0.5 if per_node_norm else 18.0**0.5)
    w2f = torch.where(cols[None, :] >= 0, w2[:, cols.clamp(min=0)], w2.new_zeros(()))
    w2f = torch.nn.functional.pad(w2f, (0, (-w2f.shape[1]) % 16 + 16)).contiguous()
    # h2p column g*8+kk <-> hidden feature 16*(kk>>2) + 4*g + (kk&3)
    feat = torch.tensor([16 * (kk >> 2) + 4 * g + (kk & 3) for g in range(4) for kk in range(8)], device=DEV)
    h2p = ops.split_hidden(h2[perm.long()][:, feat].contiguous())
    f = ops.tp_fused(x.to(DEV), h2p, w2f, geo["sh_sorted"], rowptr, src, t.get("gentries", DEV), t.get("gumap", DEV),
                     len(p.fused_unit_map), p.fused_lds_floats_per_wave, p.d_mid, avg, nn_)
    close(f, want_lr, 5e-5, "tp_fused vs oracle")
    # host-built MFMA fragments of the last layer (production path) == the kernel's own split of w2p, bit for bit
    f_pre = ops.tp_fused(x.to(DEV), h2p, w2f, geo["sh_sorted"], rowptr, src, t.get("gentries", DEV), t.get("gumap", DEV),
                         len(p.fused_unit_map), p.fused_lds_floats_per_wave, p.d_mid, avg, nn_,
                         a_split=ops.split_a_tiles(w2f, p.group_entries))
    assert torch.equal(f, f_pre)
    # the unshared walk (entry-major unit map: every wave fetches its own rows) is the same arithmetic in the same order
    umap_plain = torch.from_numpy(mplan.fused_unit_map(p.group_entries, "entry")).to(DEV)
    f_plain = ops.tp_fused(x.to(DEV), h2p, w2f, geo["sh_sorted"], rowptr, src, t.get("gentries", DEV), umap_plain,
                           umap_plain.numel(), p.fused_lds_floats_per_wave, p.d_mid, avg, nn_)
    # ... except for the vector (l1 = 1) input blocks, whose shared walk contracts the two edge slots of a pair in one pass
    # (the pair products of both edges are added before the coupling coefficients: cg_gen.h CG2): same sum, another association
    l1_cols = torch.zeros(p.d_mid, dtype=torch.bool)
    for pth in p.paths:
        if pth.l1 == 1:
            l1_cols[pth.out_off: pth.out_off + pth.mul * (2 * pth.l3 + 1)] = True
    assert l1_cols.any() and not l1_cols.all()
    assert torch.equal(f[:, ~l1_cols.to(DEV)], f_plain[:, ~l1_cols.to(DEV)])
    close(f[:, l1_cols.to(DEV)], f_plain[:, l1_cols.to(DEV)].cpu(), 2e-6, "pair-summed l1 = 1 blocks vs the edge-by-edge walk")
    # persistent units (a wave walks 1, 2, 4 or 8 node groups of its tile in turn; plan.fused_persist) change which wave
    # visits a node, never the order in which a node's edges are summed: bit-identical for every repeat count
    for spec in ("", "16:2,8:2,4:2,2:2", "16:8,8:8,4:4,2:2"):
        monkeypatch.setenv("MATTEN_TP_PERSIST", spec)
        um = torch.from_numpy(mplan.fused_unit_map(p.group_entries)).to(DEV)
        monkeypatch.delenv("MATTEN_TP_PERSIST")
        f_rep = ops.tp_fused(x.to(DEV), h2p, w2f, geo["sh_sorted"], rowptr, src, t.get("gentries", DEV), um, um.numel(),
                             p.fused_lds_floats_per_wave, p.d_mid, avg, nn_)
        assert torch.equal(f, f_rep), f"persistent units {spec!r} changed the result"
    close(a, want, 2e-5, "tp_paths vs oracle")


def test_predict_api_end_to_end(tmp_path):
    """matten.predict semantics (reference predict.py:151-245): list in -> list out in order, None for
    structures whose graph cannot be built, single structure -> single tensor; values == oracle."""
    import yaml

    from matten_amd import predict as P
    from matten_amd.data import synthetic
    from oracle.matten_ref import data as rdata
    from oracle.matten_ref.model import ToCartesian

    ds = {"allowed_species": list(synthetic.FCC_METALS), "average_num_neighbors": 18.0}
    hp = dict(PAPER)
    ref, model = build_pair(hp, ds, randomize_bn=True, device=None)
    torch.save({"state_dict": model.state_dict(),
                "hyper_parameters": {"backbone_hparams": hp, "dataset_hparams": ds, "tasks": None}},
               tmp_path / "model_final.ckpt")
    cfg = {"data": {"r_cut": 5.0, "tensor_target_name": "elastic_tensor_full",
                    "tensor_target_formula": "ijkl=jikl=klij", "tensor_target_format": "irreps"}}
    (tmp_path / "config_final.yaml").write_text(yaml.safe_dump(cfg))

    structs = synthetic.fcc64_structures(3)
    bad = {"lattice": 50.0 * np.eye(3), "cart_coords": np.zeros((1, 3)), "atomic_numbers": np.array([29])}
    with pytest.warns(UserWarning):
        out = P.predict([structs[0], bad, structs[1], structs[2]], model_identifier=str(tmp_path), batch_size=2)
    assert len(out) == 4 and out[1] is None
    graphs = [rdata.crystal_graph(s["cart_coords"], s["lattice"], s["atomic_numbers"], 5.0) for s in structs]
    with torch.no_grad():
        want = ToCartesian("ijkl=jikl=klij")(ref.decode(rdata.collate(graphs)))
    got = torch.as_tensor(np.stack([np.asarray(out[i]) for i in (0, 2, 3)]))
    assert got.shape == (3, 3, 3, 3, 3)
    close(got, want, RTOL, "predict() Cartesian tensors")
    one = P.predict(structs[0], model_identifier=str(tmp_path))
    close(torch.as_tensor(np.asarray(one)), want[0], RTOL, "single structure")
    with pytest.raises(RuntimeError, match="not supported by the model"):
        P.predict({"lattice": 3.0 * np.eye(3), "cart_coords": np.zeros((1, 3)), "atomic_numbers": [8]},
                  model_identifier=str(tmp_path))


def test_predict_packs_in_slabs_behind_the_device(monkeypatch):
    """predict() packs PREDICT_SLAB structures at a time while the device runs the previous slab's forwards: the same list
    in slabs of 3 and in one slab gives the same tensors, the None holes (malformed, edgeless, a slab without one usable
    structure) sit at the structures' own indices, the warnings name those indices, an unsupported species in a later
    slab raises like the reference."""
    import warnings as W

    from matten_amd import predict as P
    from matten_amd.data import synthetic
    from matten_amd.model_factory.tfn_scalar_tensor import ScalarTensorModel

    ds = {"allowed_species": list(synthetic.FCC_METALS), "average_num_neighbors": 18.0}
    model = ScalarTensorModel(backbone_hparams=dict(PAPER), dataset_hparams=ds).to(DEV).eval()
    cfg = {"data": {"r_cut": 5.0, "tensor_target_name": "elastic_tensor_full", "tensor_target_formula": "ijkl=jikl=klij"}}
    good = synthetic.fcc64_structures(8)
    edgeless = {"lattice": 50.0 * np.eye(3), "cart_coords": np.zeros((1, 3)), "atomic_numbers": np.array([29])}
    malformed = {"lattice": np.eye(3), "cart_coords": np.zeros((2, 3)), "atomic_numbers": np.array([29])}
    structs = [good[0], edgeless, good[1], good[2], malformed, good[3], malformed, malformed, malformed, good[4],
               good[5], good[6], edgeless, good[7]]          # slabs of 3: [0 1 2] [3 4 5] [6 7 8: none usable] [9 10 11] [12 13]
    holes = [1, 4, 6, 7, 8, 12]
    with W.catch_warnings(record=True) as w1:
        W.simplefilter("always")
        one = P.predict(structs, model=model, config=cfg, batch_size=2)
    monkeypatch.setattr(P, "PREDICT_SLAB", 3)
    with W.catch_warnings(record=True) as w3:
        W.simplefilter("always")
        three = P.predict(structs, model=model, config=cfg, batch_size=2)
    for out in (one, three):
        assert len(out) == len(structs) and [i for i, t in enumerate(out) if t is None] == holes
    for i in range(len(structs)):
        if i not in holes:
            a, b = np.asarray(one[i]), np.asarray(three[i])
            assert a.shape == (3, 3, 3, 3) and np.abs(a - b).max() <= 2e-6 * np.abs(a).max()
    for w in (w1, w3):
        text = " ".join(str(m.message) for m in w)
        for i in holes:
            assert f"structure {i}," in text, (i, text)
        assert f"{holes}" in text
    bad_species = dict(good[0], atomic_numbers=np.full(64, 8))
    with pytest.raises(RuntimeError, match="structure 4. It contains species 8 not supported"):
        P.predict(structs[:4] + [bad_species], model=model, config=cfg)


def _assert_emitted_csr(batch):
    """SURVEY 8(f)-1, last clause: the device search emits the destination-sorted CSR itself (private keys of the batch
    dict); it must be, bit for bit, what matten_csr_build derives from the finished edge list -- which in turn is pinned to
    torch.sort(stable=True) -- and the keys are popped so that the dict compares equal to the oracle's collate."""
    from matten_amd import ops
    from matten_amd.data._key import AMD_PERM, AMD_ROWPTR, AMD_SRC

    perm, rowptr, src = batch.pop(AMD_PERM), batch.pop(AMD_ROWPTR), batch.pop(AMD_SRC)
    n = batch["pos"].shape[0]
    perm2, rowptr2, src2, err = ops.csr_build(batch["edge_index"], n)
    assert int(err.item()) == 0
    assert perm.dtype == rowptr.dtype == src.dtype == torch.int32
    assert torch.equal(rowptr, rowptr2) and torch.equal(perm, perm2) and torch.equal(src, src2)
    order = torch.sort(batch["edge_index"][1], stable=True).indices
    assert torch.equal(perm.long(), order) and torch.equal(src.long(), batch["edge_index"][0][order])


def test_gpu_neighbor_list_is_identical_to_oracle_builder(golden_dir):
    """the device neighbour search emits exactly the (i, j, S) list of the oracle's
    brute-force builder (oracle/matten_ref/data.py, ASE contract of data/data.py:285-413) in canonical order:
    index work, compared bit for bit, on the reference's n=100 sample (triclinic, skewed, unwrapped cells),
    jittered fcc-64 and a 1-atom cell that only has image neighbours."""
    from matten_amd.data import synthetic
    from matten_amd.data.graph import EdgelessStructures, batch_graphs_gpu
    from oracle.matten_ref import data as rdata

    structs = rdata.structures_from_json(os.path.join(golden_dir, "example_crystal_elasticity_tensor_n100.json"))
    structs = structs + synthetic.fcc64_structures(4)
    structs.append({"lattice": 3.0 * np.eye(3), "cart_coords": np.array([[0.3, 7.1, -2.2]]), "atomic_numbers": [14]})
    triples = [(s["cart_coords"], s["lattice"], s["atomic_numbers"]) for s in structs]
    got = batch_graphs_gpu(triples, 5.0, DEV)
    want = rdata.collate([rdata.crystal_graph(s["cart_coords"], s["lattice"], s["atomic_numbers"], 5.0) for s in structs])
    _assert_emitted_csr(got)
    assert set(got) == set(want)
    for k in want:
        g = got[k].cpu()
        assert g.dtype == want[k].dtype and g.shape == want[k].shape, k
        assert torch.equal(g, want[k]), k

    with pytest.raises(EdgelessStructures) as ei:
        batch_graphs_gpu([triples[0], (np.zeros((1, 3)), 50.0 * np.eye(3), [14]), triples[1]], 5.0, DEV)
    assert ei.value.indices == [1]


def test_gpu_neighbor_list_on_random_cells():
    """The per-pair image bound of the device search (|S_k + df_k| <= r_cut |inv[:, k]|) only prunes: on 400 random cells
    -- thin, skewed, nearly flat, atoms up to three cells outside the box, one to eight atoms, cutoffs 2.5 to 6.5 -- the
    edge list, the shifts and num_neigh equal the oracle's brute-force builder bit for bit."""
    from matten_amd.data.graph import batch_graphs_gpu
    from oracle.matten_ref import data as rdata

    rng = np.random.default_rng(77)
    for r_cut in (2.5, 5.0, 6.5):
        triples = []
        while len(triples) < 134:
            lengths = rng.choice([1.6, 2.5, 4.0, 7.0, 12.0], size=3)
            cell = np.diag(lengths) + rng.normal(0.0, 0.35, (3, 3)) * lengths[:, None]
            if rng.random() < 0.3:
                cell[2] = 0.9 * cell[0] + 0.5 * cell[1] + rng.normal(0.0, 1.0, 3) * 0.5   # a nearly flat cell
            vol = abs(np.linalg.det(cell))
            if vol < 4.0:
                continue
            n = int(rng.integers(1, 9))
            frac = rng.uniform(-3.0, 4.0, (n, 3)) if rng.random() < 0.5 else rng.random((n, 3))
            try:
                rdata.neighbor_list(frac @ cell, cell, r_cut)
            except ValueError:
                continue   # no edge at all: covered by the edgeless test
            triples.append((frac @ cell, cell, rng.integers(1, 90, n)))
        got = batch_graphs_gpu(triples, r_cut, DEV)
        want = rdata.collate([rdata.crystal_graph(p, c, z, r_cut) for p, c, z in triples])
        _assert_emitted_csr(got)
        for k in ("edge_index", "edge_cell_shift", "num_neigh", "batch", "ptr", "pos", "cell"):
            assert torch.equal(got[k].cpu(), want[k]), (r_cut, k)


def _species_linear_case(irreps_in, irreps_out, S, N, with_add, gen):
    """The product's species-indexed linear (nn.utils.SpeciesLinear -> matten_species_linear[_rows]) against the
    ORACLE's FullyConnectedTensorProduct(x, one_hot(species)) (oracle/e3nn_lite/o3.py, e3nn semantics: instruction
    order, 'uvw' weights [mul_in, S, mul_out] flat, element path normalisation) holding the same flat weight vector,
    evaluated in fp64.  -> largest error relative to the output's largest magnitude."""
    from matten_amd import ops
    from matten_amd.nn.utils import SpeciesLinear
    from oracle.e3nn_lite import o3 as ro3

    mod = SpeciesLinear(irreps_in, S, irreps_out).to(DEV)
    ref = ro3.FullyConnectedTensorProduct(irreps_in, f"{S}x0e", irreps_out)
    assert ref.weight.numel() == mod.weight.numel(), (irreps_in, irreps_out, ref.weight.numel(), mod.weight.numel())
    w = torch.randn(mod.weight.numel(), device=DEV, generator=gen)
    x = torch.randn(N, mod.plan.d_in, device=DEV, generator=gen)
    add = torch.randn(N, mod.plan.d_out, device=DEV, generator=gen) if with_add else None
    species = torch.randint(0, S, (N,), device=DEV, generator=gen)
    order, seg, _ = ops.group_by_key(species, S)
    with torch.no_grad():
        mod.weight.copy_(w)
        ref.weight.copy_(w.cpu())
        got = mod(x, (order, seg), add=add)
        ref = ref.double()
        want = ref(x.cpu().double(), torch.nn.functional.one_hot(species.cpu(), S).double())
        if with_add:
            want = want + add.cpu().double()
    assert got.shape == want.shape
    return (got.cpu().double() - want).abs().max().item() / max(1e-6, want.abs().max().item())


def test_species_linear_shape_sweep():
    """Row-streaming MFMA kernel over the shapes that stress its chunking: every conv-layer shape of the paper
    model, output multiplicities across the 16/32-channel tile boundaries (with and without the streamed addend),
    input multiplicities across the 16-channel step and 160-float window boundaries, all l <= 4, ragged species
    groups.  Reference: the oracle's FullyConnectedTensorProduct(x, one_hot(species)) with the same flat weights, in
    fp64 (not the plan's own segment tables: the plan is part of what is under test).

    Which kernel each family reaches under today's routing (ops.species_linear_route; recomputed on the CPU by
    test_species_linear_host.py::test_shape_sweep_routing_is_what_its_docstring_records): the output-multiplicity sweep
    runs on the ROWS kernel in all 159 cases, the input-multiplicity sweep on the rows kernel in 99 cases and on the
    streaming kernel in 16 (mi >= 159 at l >= 2, mi = 321 at l >= 1), the two "big W" cases on the streaming kernel with
    the A operand in global memory.  The streaming kernel's tile boundaries, chunk boundaries and cross-block walk are
    forced in tests/test_gpu_species_linear.py."""
    from matten_amd.model_factory.tfn_scalar_tensor import create_model
    from matten_amd.data import synthetic

    gen = torch.Generator(device=DEV).manual_seed(7)
    worst = {}
    m = create_model(dict(PAPER), {"allowed_species": list(synthetic.FCC_METALS), "average_num_neighbors": 18.0})
    for name, mod in m.named_modules():
        if type(mod).__name__ == "SpeciesLinear" and mod.n_species is not None:
            for N in (1, 200):
                for add in (False, True):
                    worst[(name, N, add)] = _species_linear_case(str(mod.irreps_in), str(mod.irreps_out), mod.n_species,
                                                                 N, add, gen)
    for mo in list(range(1, 40)) + [63, 64, 65, 70, 78, 79, 80, 81, 96, 97, 127, 128, 129, 161]:
        for l, mi in ((0, 8), (1, 5), (2, 3)):
            ir = f"{l}{'e' if l % 2 == 0 else 'o'}"
            worst[("mo", mo, l)] = _species_linear_case(f"{mi}x{ir}", f"{mo}x{ir}", 2, 37, True, gen)
    for mi in list(range(1, 36, 2)) + [159, 160, 161, 170, 321]:
        for l in range(5):
            ir = f"{l}{'e' if l % 2 == 0 else 'o'}"
            worst[("mi", mi, l)] = _species_linear_case(f"{mi}x{ir}+3x0e", f"5x{ir}+2x0e", 3, 50, bool(mi % 2), gen)
    # a packed table too large for LDS (400 x 90 floats = 144 KB per species): the global-memory A-operand variant
    worst[("big W", 0)] = _species_linear_case("400x0e+20x1o", "90x0e+7x1o", 3, 130, True, gen)
    worst[("big W", 1)] = _species_linear_case("330x1o", "100x1o", 2, 70, False, gen)
    bad = {k: v for k, v in worst.items() if not v < 2e-6}
    assert not bad, f"{len(bad)} of {len(worst)} shapes off: {sorted(bad.items(), key=lambda kv: -kv[1])[:8]}"


def test_atomic_tensor_model_vs_oracle_and_predict(tmp_path, golden_dir):
    """AtomicTensorModel (model_factory/tfn_atomic_tensor.py) -- per-atom ij=ji tensors against
    the oracle on the n=100 sample, the atom_selector step of the reference's shared_step, and
    predict(is_atomic_tensor=True) returning one flat list of per-atom tensors (predict.py:196-242)."""
    import yaml

    from common import ATOMIC
    from matten_amd import predict as P
    from matten_amd.data.graph import average_num_neighbors, collate, crystal_graph
    from oracle.matten_ref import data as rdata
    from oracle.matten_ref.model import ToCartesian

    structs = rdata.structures_from_json(os.path.join(golden_dir, "example_crystal_elasticity_tensor_n100.json"))[:12]
    graphs = [crystal_graph(s["cart_coords"], s["lattice"], s["atomic_numbers"], 5.0) for s in structs]
    ds = {"allowed_species": sorted({int(z) for s in structs for z in s["atomic_numbers"]}),
          "average_num_neighbors": average_num_neighbors(graphs)}
    ref, model = build_pair(dict(ATOMIC), ds, randomize_bn=True, atomic=True)
    cpu = collate(graphs)
    with torch.no_grad():
        want = ref.decode(cpu)
        preds, labels = model(dict(collate(graphs, device=DEV), atom_selector=(cpu["atomic_numbers"] % 2 == 0).to(DEV)),
                              task_name="nmr_tensor")
    got = preds["nmr_tensor"]
    assert got.shape == (cpu["pos"].shape[0], 6)
    close(got, want, RTOL, "per-atom irreps")
    sel = model.select_atoms(preds, labels)["nmr_tensor"]
    assert sel.shape[0] == int((cpu["atomic_numbers"] % 2 == 0).sum()) and "atom_selector" in labels
    close(sel, want[cpu["atomic_numbers"] % 2 == 0], RTOL, "selected atoms")

    torch.save({"state_dict": model.state_dict(),
                "hyper_parameters": {"backbone_hparams": dict(ATOMIC), "dataset_hparams": ds, "tasks": "nmr_tensor"}},
               tmp_path / "model_final.ckpt")
    cfg = {"data": {"r_cut": 5.0, "tensor_target_name": "nmr_tensor", "tensor_target_formula": "ij=ji"}}
    (tmp_path / "config_final.yaml").write_text(yaml.safe_dump(cfg))
    out = P.predict(structs, model_identifier=str(tmp_path), is_atomic_tensor=True, batch_size=5)
    assert len(out) == cpu["pos"].shape[0] and out[0].shape == (3, 3)
    close(torch.as_tensor(np.stack(out)), ToCartesian("ij=ji")(want), RTOL, "predict() per-atom Cartesian tensors")
    one = P.predict(structs[0], model_identifier=str(tmp_path), is_atomic_tensor=True)
    assert isinstance(one, list) and len(one) == len(structs[0]["atomic_numbers"])


def test_config3_full_size_batch_properties():
    """BASELINE configs[2] at its full size (1000 fcc-64 crystals, 64 000 atoms, 1 152 000 edges -- the bench workload),
    checked through size-independent properties: (a) a crystal's prediction does not depend on what else is in the
    batch (bitwise: the per-node summation order is fixed), which ties the full-size run to the 8-crystal batches the
    oracle can afford; (b) the oracle itself on 6 crystals picked from the big batch; (c) permuting the crystals
    permutes the rows; (d) rotating every crystal rotates every elasticity tensor; (e) bitwise determinism."""
    from matten_amd.data import synthetic
    from matten_amd.data.graph import batch_graphs_gpu, collate, crystal_graph
    from oracle.e3nn_lite import o3
    from oracle.matten_ref.model import ToCartesian

    n = 1000
    structs = synthetic.fcc64_structures(n)
    ds = {"allowed_species": list(synthetic.FCC_METALS), "average_num_neighbors": 18.0}
    ref, model = build_pair(PAPER, ds, randomize_bn=True)
    triples = [(s["cart_coords"], s["lattice"], s["atomic_numbers"]) for s in structs]
    big = batch_graphs_gpu(triples, 5.0, DEV)
    assert big["pos"].shape[0] == 64 * n and big["edge_index"].shape[1] == 1152 * n
    with torch.no_grad():
        y = model.decode(dict(big))["elastic_tensor_full"]
        y_again = model.decode(dict(big))["elastic_tensor_full"]
    assert y.shape == (n, 21) and torch.isfinite(y).all()
    assert torch.equal(y, y_again)                                                   # (e)

    pick = [0, 1, 137, 500, 998, 999]
    # (a) bitwise against another batch on the same kernel path (>= nn.conv.AGG_KM_MIN_ROWS nodes: lin2 streams
    # component-major rows), to 2e-6 against the 6-crystal batch, whose lin2 runs on the row-resident kernel (same
    # products, another summation order inside the matrix instructions' K loop)
    mid_ids = sorted(set(pick) | set(range(300, 444)))
    mid = batch_graphs_gpu([triples[i] for i in mid_ids], 5.0, DEV)
    small = batch_graphs_gpu([triples[i] for i in pick], 5.0, DEV)
    with torch.no_grad():
        y_mid = model.decode(dict(mid))["elastic_tensor_full"]
        y_small = model.decode(dict(small))["elastic_tensor_full"]
        want = ref.decode(collate([crystal_graph(*triples[i], 5.0) for i in pick]))
    assert mid["pos"].shape[0] >= 8192 and torch.equal(y[mid_ids], y_mid)            # (a)
    close_blocks(y[pick], y_small, rtol=2e-6, floor=2e-6, what="full-size batch vs the same crystals in a 6-crystal batch")
    close_blocks(y[pick], want, what="full-size batch vs oracle on 6 crystals",      # (b)
                 want64=_want64(ref, [crystal_graph(*triples[i], 5.0) for i in pick]))

    perm = torch.randperm(n, generator=torch.Generator().manual_seed(1)).tolist()
    with torch.no_grad():
        y_perm = model.decode(dict(batch_graphs_gpu([triples[i] for i in perm], 5.0, DEV)))["elastic_tensor_full"]
    assert torch.equal(y_perm, y[perm])                                              # (c)

    torch.manual_seed(35)
    Q = o3.rand_matrix().double().numpy()
    rotated = [(p @ Q.T, c @ Q.T, z) for (p, c, z) in triples]
    with torch.no_grad():
        y_rot = model.decode(dict(batch_graphs_gpu(rotated, 5.0, DEV)))["elastic_tensor_full"]
    to_cart = ToCartesian("ijkl=jikl=klij")
    t, t_rot = to_cart(y.cpu()), to_cart(y_rot.cpu())
    Qt = torch.as_tensor(Q, dtype=t.dtype)
    want_rot = torch.einsum("ia,jb,kc,ld,nabcd->nijkl", Qt, Qt, Qt, Qt, t)
    close(t_rot, want_rot, 5e-4, "rotation equivariance of 1000 crystals")           # (d)


def test_operands_beyond_4GB(monkeypatch):
    """Maximum sizes: with 4200 fcc-64 crystals the neighbour-sum output of the FULL last conv layer is 4.5 GB, past
    the 4 GB a buffer descriptor / 32-bit byte offset can address (the lin2 kernels re-base their descriptors per wave,
    the TP kernels use 64-bit row offsets); dead-output elimination is switched off here so that the full layer runs.
    Property: predictions are bitwise those of a 150-crystal batch (same kernel path), and within 2e-6 of a 4-crystal
    batch (row-resident lin2: another summation order)."""
    from matten_amd.data import synthetic
    from matten_amd.data.graph import batch_graphs_gpu
    from matten_amd.nn import conv as pconv

    monkeypatch.setattr(pconv, "DEAD_PATH_ELIMINATION", False)
    n = 4200
    uniq = synthetic.fcc64_structures(100)
    triples = [(uniq[i % 100]["cart_coords"], uniq[i % 100]["lattice"], uniq[i % 100]["atomic_numbers"]) for i in range(n)]
    ds = {"allowed_species": list(synthetic.FCC_METALS), "average_num_neighbors": 18.0}
    _, model = build_pair(PAPER, ds, randomize_bn=True)
    assert 64 * n * model.backbone.conv_layer_last.tp.plan.d_mid * 4 > 2**32
    with torch.no_grad():
        y = model.decode(dict(batch_graphs_gpu(triples, 5.0, DEV)))["elastic_tensor_full"]
        pick = [0, 1, n // 2, n - 1]
        mid_ids = sorted(set(pick) | set(range(1000, 1146)))
        ym = model.decode(dict(batch_graphs_gpu([triples[i] for i in mid_ids], 5.0, DEV)))["elastic_tensor_full"]
        ys = model.decode(dict(batch_graphs_gpu([triples[i] for i in pick], 5.0, DEV)))["elastic_tensor_full"]
    assert torch.isfinite(y).all() and torch.equal(y[mid_ids], ym)
    close_blocks(y[pick], ys, rtol=2e-6, floor=2e-6, what="4200-crystal batch vs a 4-crystal batch")
    # copies of one crystal give identical rows wherever they sit in the batch
    assert torch.equal(y[0], y[100]) and torch.equal(y[7], y[4107])


def test_random_small_models_vs_oracle():
    """Generality of the plan / kernel tables beyond the shipped configs: six random models (lmax 1-4, odd and unit
    multiplicities, missing parities, 1-3 gated layers, with and without BatchNorm / fixed neighbour normalisation) on
    random triclinic cells against the oracle (tests/fuzz_models.py runs the same generator for as many cases as wanted;
    104 cases were clean when this test was written)."""
    import subprocess
    import sys as _sys

    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([_sys.executable, os.path.join(here, "fuzz_models.py"), "6", "11"], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "bad 0" in r.stdout
    # the same generator with gradients: training forward + every parameter gradient of a random MSE loss, activation type
    # (gate / norm), normalisation (batch / instance / none) and pooling (mean / sum / max) randomised too
    r = subprocess.run([_sys.executable, os.path.join(here, "fuzz_models.py"), "8", "5", "grad"], capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "bad 0" in r.stdout


def test_isolated_atom_and_ragged_degrees():
    """An atom without any neighbour inside the cutoff (degree 0) next to bonded ones, in a batch with a dense crystal:
    empty CSR segments, ragged degrees (0 / 1 / 18+), fixed neighbour normalisation -- against the oracle."""
    from matten_amd.data import synthetic
    from matten_amd.data.graph import collate, crystal_graph

    lone = crystal_graph(np.array([[0.0, 0, 0], [1.5, 0, 0], [6.0, 6.0, 6.0]]), 12.0 * np.eye(3), [29, 79, 29], 5.0)
    assert lone["num_neigh"].tolist() == [1.0, 1.0, 0.0]
    graphs = [lone] + synthetic.fcc64_graphs(1) + [lone]
    ds = {"allowed_species": list(synthetic.FCC_METALS), "average_num_neighbors": 18.0}
    ref, model = build_pair(PAPER, ds, randomize_bn=True)
    got, want = _run_pair(ref, model, graphs)
    assert torch.isfinite(got).all()
    close(got, want, RTOL, "batch with an isolated atom")
    assert torch.equal(got[0], got[2])


def test_neighbor_list_slabs_match_single_launch(monkeypatch):
    """More crystals than one launch of the neighbour kernels takes (65535, blockIdx.y): the slab path must give the
    same batch; exercised by lowering the limit."""
    from matten_amd.data import graph, synthetic

    structs = synthetic.fcc64_structures(7)
    triples = [(s["cart_coords"], s["lattice"], s["atomic_numbers"]) for s in structs]
    want = graph.batch_graphs_gpu(triples, 5.0, DEV)
    monkeypatch.setattr(graph, "_MAX_CRYSTALS_PER_LAUNCH", 3)
    got = graph.batch_graphs_gpu(triples, 5.0, DEV)
    # (a single launch also emits its destination-sorted CSR as private keys; slabs leave it to the forward)
    assert set(got) == {k for k in want if not k.startswith("_amd_")}
    for k in got:
        assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), k


def test_debug_mode_catches_nan_on_device():
    """log level DEBUG: the DetectAnomaly layers (reference nn/utils.py:370-394) name the first layer whose output holds
    a NaN; the same batch passes silently (NaN output) without them"""
    from matten_amd import log
    from matten_amd.data.graph import collate

    graphs, ds = _fcc(1)
    log.set_logger("DEBUG", stderr=False)
    try:
        _, model = build_pair(dict(LMAX2, num_layers=1), ds, device=DEV)
    finally:
        log.set_logger("ERROR", stderr=False)
    good = collate(graphs, device=DEV)
    with torch.no_grad():
        out = model(dict(good))[0]["elastic_tensor_full"]
        assert torch.isfinite(out).all()
        bad = dict(good)
        bad["pos"] = good["pos"].clone()
        bad["pos"][3, 1] = float("nan")
        with pytest.raises(ValueError, match="Anomaly detected for pos of one_hot"):
            model(bad)


def test_deferred_input_checks_raise_one_forward_late():
    """model.set_input_checks("deferred"): the species / edge_index flags of a forward are read when the next forward is
    enqueued (or at finish_input_checks()), so loops run without a host wait; results are unchanged and a malformed
    batch still raises the reference's errors, one call late."""
    from matten_amd.data.graph import collate

    graphs, ds = _fcc(2)
    _, model = build_pair(PAPER, ds)
    good = collate(graphs, device=DEV)
    bad = dict(good)
    bad["edge_index"] = good["edge_index"].clone()
    bad["edge_index"][1, 5] = good["pos"].shape[0] + 3
    unknown = dict(good)
    unknown["atomic_numbers"] = good["atomic_numbers"].clone()
    unknown["atomic_numbers"][0] = 3          # lithium is not in the model's species list
    with torch.no_grad():
        want = model(dict(good))[0]["elastic_tensor_full"]
        with pytest.raises(IndexError):
            model(dict(bad))
        model.set_input_checks("deferred")
        assert torch.equal(model(dict(good))[0]["elastic_tensor_full"], want)
        model(dict(bad))                                   # not yet
        with pytest.raises(IndexError, match="edge_index holds node ids outside"):
            model(dict(good))                              # ... now
        model(dict(unknown))
        with pytest.raises((RuntimeError, ValueError)):
            model.finish_input_checks()
        model.finish_input_checks()                        # nothing pending: no-op
        model.set_input_checks(True)
        assert torch.equal(model(dict(good))[0]["elastic_tensor_full"], want)


def test_atom_feats_ride_behind_the_species_embedding(golden_dir):
    """use_atom_feats=True (reference nn/embedding.py:59-68,103-105): data["atom_feats"] [n_atoms, F] is stacked behind
    the species embedding, so the first conv layer sees (16 + F)x0e -- forward against the oracle, and one training
    step's gradients (the features enter lin1 / self-connection of the first layer)."""
    from matten_amd.data.graph import average_num_neighbors, collate, crystal_graph
    from oracle.matten_ref import data as rdata

    structs = rdata.structures_from_json(os.path.join(golden_dir, "example_crystal_elasticity_tensor_n100.json"))[:7]
    graphs = [crystal_graph(s["cart_coords"], s["lattice"], s["atomic_numbers"], 5.0) for s in structs]
    gen = torch.Generator().manual_seed(3)
    F = 5
    for g in graphs:
        g["atom_feats"] = torch.randn(g["pos"].shape[0], F, generator=gen)
    ds = {"allowed_species": sorted({int(z) for s in structs for z in s["atomic_numbers"]}),
          "average_num_neighbors": average_num_neighbors(graphs), "atom_feats_size": F}
    ref, model = build_pair(dict(LMAX2, use_atom_feats=True), ds, randomize_bn=True)
    assert str(model.backbone.one_hot.irreps_out["node_features"]) == f"{16 + F}x0e"
    with torch.no_grad():
        want = ref.decode(collate(graphs))
        got = model(collate(graphs, device=DEV))[0]["elastic_tensor_full"]
    close(got[:, :12], want[:, :12], RTOL, "forward with atom features")       # (lmax 2: the 4e block has no path)
    ref.train(), model.train()
    target = torch.randn(len(graphs), 21, generator=gen)
    torch.nn.functional.mse_loss(ref.decode(collate(graphs)), target).backward()
    torch.nn.functional.mse_loss(model(collate(graphs, device=DEV))[0]["elastic_tensor_full"], target.to(DEV)).backward()
    named = dict(model.named_parameters())
    for k, p in ref.named_parameters():
        if p.grad is not None and "layer0_convnet.conv" in k:
            close(named[k].grad, p.grad, 3e-3, f"grad {k}")


def test_kernel_path_switch_at_the_streaming_threshold():
    """Batches just below / at / above nn.conv.AGG_KM_MIN_ROWS nodes take different lin2 / Gate kernels (row-resident +
    gate kernel vs streaming lin2 with the Gate in its epilogue): the same crystals give the same predictions (2e-6 per
    irrep block) whichever side of the switch their batch falls on, and the oracle's on the crystals it is run for."""
    from matten_amd.data import synthetic
    from matten_amd.data.graph import batch_graphs_gpu, collate, crystal_graph
    import matten_amd.nn.conv as conv_mod

    assert conv_mod.AGG_KM_MIN_ROWS == 8192
    structs = synthetic.fcc64_structures(130)
    triples = [(s["cart_coords"], s["lattice"], s["atomic_numbers"]) for s in structs]
    ds = {"allowed_species": list(synthetic.FCC_METALS), "average_num_neighbors": 18.0}
    ref, model = build_pair(PAPER, ds, randomize_bn=True)
    outs = {}
    with torch.no_grad():
        for n in (127, 128, 129):   # 8128 / 8192 / 8256 nodes
            outs[n] = model.decode(dict(batch_graphs_gpu(triples[:n], 5.0, DEV)))["elastic_tensor_full"]
        want = ref.decode(collate([crystal_graph(*triples[i], 5.0) for i in (0, 63, 126)]))
    close_blocks(outs[128][:127], outs[127], rtol=2e-6, floor=2e-6, what="8192-node batch vs 8128-node batch")
    close_blocks(outs[129][:128], outs[128], rtol=2e-6, floor=2e-6, what="8256-node batch vs 8192-node batch")
    close_blocks(outs[127][[0, 63, 126]], want, what="8128-node batch vs oracle",
                 want64=_want64(ref, [crystal_graph(*triples[i], 5.0) for i in (0, 63, 126)]))
    close_blocks(outs[129][[0, 63, 126]], want, what="8256-node batch vs oracle",
                 want64=_want64(ref, [crystal_graph(*triples[i], 5.0) for i in (0, 63, 126)]))


def test_non_power_of_two_multiplicities_keep_the_mul_ir_row(monkeypatch):
    """A piece of the component-major neighbour-sum row whose channel count is not a power of two would leave alignment
    holes that no kernel writes and the streaming lin2 multiplies by structural-zero weights (0 x garbage): such layers
    must not get an AggLinearPlan.  Forced onto the streaming path's batch size with NaN-filled buffers the model still
    matches the oracle (found by tests/fuzz_models.py with NAN_EMPTY=1)."""
    from matten_amd.data import synthetic
    from matten_amd.data.graph import collate
    import matten_amd.nn.conv as conv_mod

    monkeypatch.setattr(conv_mod, "AGG_KM_MIN_ROWS", 0)
    _empty = torch.empty
    monkeypatch.setattr(torch, "empty", lambda *a, **k: (lambda t: t.fill_(float("nan")) if t.is_floating_point() and t.is_cuda else t)(_empty(*a, **k)))
    hp = dict(PAPER, conv_layer_irreps="5x0o+3x0e+17x1o+8x3o+32x3e+4x4e", num_layers=2)
    graphs, ds = _fcc(2)
    ref, model = build_pair(hp, ds, randomize_bn=True)
    convs = [m for m in model.modules() if type(m).__name__ == "PointConv"]
    assert any(m.agg_plan is None for m in convs)          # 5, 3, 17 channels: holes -> no component-major plan
    got, want = _run_pair(ref, model, graphs)
    assert torch.isfinite(got).all()
    close_blocks(got, want, what="odd multiplicities at the streaming batch size", want64=_want64(ref, graphs))


def test_species_linear_selfcheck_runs_and_detects_a_wrong_result(monkeypatch):
    """matten_amd/selfcheck.py: the first species-linear call on a device runs both inline-asm MFMA kernels on
    integer-valued cases whose fp32 result is exact and compares bit for bit with an int64 evaluation on the host; a
    library whose kernels miscompute (the stale-accumulator miscompile of a build without
    -mllvm -simplifycfg-sink-common=false, csrc/Makefile) must be refused, not used."""
    from matten_amd import _lib, selfcheck

    selfcheck._done.clear()
    selfcheck.check_species_linear(DEV)            # the real kernels: exact
    assert selfcheck._done[0] is True
    # every case of both variants really went through the kernels and matched
    gen = torch.Generator().manual_seed(1)
    from matten_amd import ops, plan as mplan

    for variant in ("rows", "stream"):
        got, want = selfcheck._case(ops, mplan, "8x0e", "33x0e", 2, 37, DEV, gen, variant)
        assert torch.equal(got.cpu(), want.float())
    real_case = selfcheck._case

    def broken(*a, **k):                           # one stale accumulator element in one case
        got, want = real_case(*a, **k)
        if a[2] == "8x0e" and a[3] == "78x0e":
            got = got.clone()
            got[5, 70] += 1.0
        return got, want

    monkeypatch.setattr(selfcheck, "_case", broken)
    selfcheck._done.clear()
    with pytest.raises(_lib.MattenHipError, match="self-check FAILED"):
        selfcheck.check_species_linear(DEV)
    assert not selfcheck._done.get(0)
    monkeypatch.setattr(selfcheck, "_case", real_case)
    selfcheck.check_species_linear(DEV)


@pytest.mark.parametrize("mode", ["streaming_lin2", "hub_pieces_of_3", "fused_training"])
def test_fuzzed_models_on_poisoned_buffers(mode):
    """tests/fuzz_models.py (random irreps / multiplicities incl. non-powers of two / depth / normalisation on random small
    crystals, product vs oracle) with every torch.empty buffer starting as NaN (NAN_EMPTY=1) and one opt-in or
    size-dependent path forced for every layer and batch size:
      streaming_lin2   component-major neighbour sums + matten_agg_linear (the mode that found the alignment holes of
                       non-power-of-two multiplicities, plan.plan_agg_linear; MATTEN_AGG_KM_MIN_ROWS=0)
      hub_pieces_of_3  every CSR segment walked in pieces of 3 edges (MATTEN_HUB_SPLIT_LEN=3)
      fused_training   training forward on matten_tp_fused + the w-free adjoint (MATTEN_TRAIN_TP=fused: the default from 65 536 edges
                       on) with every parameter gradient against the fp64 oracle -- odd multiplicities, alternative coupling
                       groups, paths of a block taken in rounds"""
    import subprocess
    import sys

    extra = {"streaming_lin2": {"MATTEN_AGG_KM_MIN_ROWS": "0"},
             "hub_pieces_of_3": {"MATTEN_HUB_SPLIT_LEN": "3"},
             "fused_training": {"MATTEN_TRAIN_TP": "fused"}}[mode]
    env = dict(os.environ, NAN_EMPTY="1", **extra)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    args = ["16", "7", "grad"] if mode == "fused_training" else ["24", "4"]
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "fuzz_models.py"), *args], env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "bad 0" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_hub_segments_are_walked_in_pieces(golden_dir, monkeypatch):
    """Small batches cut every CSR segment into virtual nodes of at most hub_split_len(n_rows) edges (matten_csr_split) so that
    a hub -- the n100 sample has atoms with 80 neighbours, the average is 30 -- does not set the duration of every
    tensor-product launch; the real node's neighbour sum is the ordered sum of its pieces.  Checked: the split tables
    against a host evaluation (ragged degrees, empty segments, bound padding), the n100 forward with pieces of 32 / 5 /
    whole segments against each other and the oracle, per-node neighbour normalisation, and that a crystal's result does
    not depend on its batch mates (bitwise at equal piece length; the default length grows with the batch: 8 / 16 / 32)."""
    from matten_amd import ops
    from matten_amd.data.graph import average_num_neighbors, collate, crystal_graph
    from matten_amd.nn import utils as nnu
    from oracle.matten_ref import data as rdata

    # ---- the tables
    deg = torch.tensor([0, 3, 70, 32, 33, 1, 0, 64, 5], dtype=torch.int64)
    rowptr = torch.zeros(len(deg) + 1, dtype=torch.int32)
    rowptr[1:] = torch.cumsum(deg, 0).to(torch.int32)
    E = int(rowptr[-1])
    nn_host = torch.arange(1, len(deg) + 1, dtype=torch.float32)
    vrow, vseg, vnn = ops.csr_split(rowptr.to(DEV), E, 32, nn_host.to(DEV))
    vrow, vseg, vnn = vrow.cpu(), vseg.cpu(), vnn.cpu()
    bound = len(deg) + E // 32
    assert vrow.shape[0] == bound + 1 and vseg.shape[0] == len(deg) + 1
    want_rows, want_seg = [], [0]
    for n, d in enumerate(deg.tolist()):
        k = max(1, -(-d // 32))
        want_rows += [int(rowptr[n]) + i * d // k for i in range(k)]   # balanced: 70 edges = 23 + 23 + 24, 33 = 16 + 17
        want_seg.append(want_seg[-1] + k)
    nv = want_seg[-1]
    assert vseg.tolist() == want_seg and vrow[:nv].tolist() == want_rows and (vrow[nv:] == E).all()
    for n in range(len(deg)):
        assert (vnn[want_seg[n]:want_seg[n + 1]] == nn_host[n]).all()
    # pieces tile the edge list: consecutive, each at most 32 long, the last of a node ending where the next node starts
    lens = (vrow[1:nv + 1] - vrow[:nv])
    assert int(lens.max()) <= 32 and int(lens.sum()) == E

    # ---- the forward
    structs = rdata.structures_from_json(os.path.join(golden_dir, "example_crystal_elasticity_tensor_n100.json"))
    graphs = [crystal_graph(s["cart_coords"], s["lattice"], s["atomic_numbers"], 5.0) for s in structs]
    assert max(int(g["num_neigh"].max()) for g in graphs) > 64      # (80: more than twice the average of 30)
    species = sorted({int(z) for s in structs for z in s["atomic_numbers"]})
    for avg in (average_num_neighbors(graphs), None):
        hp = dict(PAPER, average_num_neighbors="auto" if avg else None)
        ref, model = build_pair(hp, {"allowed_species": species, "average_num_neighbors": avg}, randomize_bn=True)
        batch = collate(graphs, device=DEV)
        outs = {}
        with torch.no_grad():
            outs["auto"] = model(dict(batch))[0]["elastic_tensor_full"].clone()   # the length hub_split_len() picks (8 here)
            for L in (32, 16, 5, 0):
                monkeypatch.setattr(nnu, "hub_split_len", lambda n_rows, L=L: L)
                outs[L] = model(dict(batch))[0]["elastic_tensor_full"].clone()
            want = ref.decode(collate(graphs))
            monkeypatch.setattr(nnu, "hub_split_len", lambda n_rows: 32)
            sub = model(dict(collate(graphs[40:57], device=DEV)))[0]["elastic_tensor_full"]
        close_blocks(outs["auto"], outs[0].cpu(), rtol=5e-6, floor=2e-6, what="default piece length vs whole segments")
        close_blocks(outs[32], outs[0].cpu(), rtol=5e-6, floor=2e-6, what="pieces of 32 vs whole segments")
        close_blocks(outs[16], outs[0].cpu(), rtol=5e-6, floor=2e-6, what="pieces of 16 vs whole segments")
        close_blocks(outs[5], outs[0].cpu(), rtol=5e-6, floor=2e-6, what="pieces of 5 vs whole segments")
        close_blocks(outs[32], want, what="n100 with hub splitting vs oracle", want64=_want64(ref, graphs))
        assert torch.equal(sub, outs[32][40:57]), "a crystal's rows depend on its batch mates"

