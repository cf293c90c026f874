"""
Narrowed neighbour sums on the GPU (matten_tp_fused_narrow + the unchanged matten_agg_linear; plan.plan_agg_narrow): the entry's
lanes apply their slice of lin2 to their own sums wherever lin2 has fewer output than input channels, and the row between the
two kernels carries mo floats per component instead of mul.  test_agg_narrow_host.py walks the same plan on the host.

One conv layer at the paper irreps with Gate and eval-mode BatchNorm (layer 3 of a four-layer paper model: the first layer
whose input row holds every irrep of conv_layer_irreps -- 0o appears behind layer 2), and the inference view of the last conv layer (the irreps the head reads: 32x0e+4x2e+2x4e), on 70 nodes -- one full 64-node tile and a partial
one -- with in-degrees 0, 1, 5, 19 and 40 mixed (an empty segment, less than one chunk, more than the 16-lane kind's 4 slots x
4 chunks), three species in interleaved order, every torch.empty buffer (the neighbour-sum row among them) starting as NaN,
and the streaming lin2 forced onto the small batch (AGG_KM_MIN_ROWS = 0, as test_gpu_parity does).

Accuracy: the layer output against the fp64 oracle ON THE SAME fp32 INPUT ROWS per irrep block, with test_gpu_parity's helper
and its 2e-5 block tolerance, for the narrowed layer and for the MATTEN_AGG_NARROW=0 build of the same layer in the same test.
Determinism: two launches give the same bits.  Walk forms: the workgroup-shared / paired walk and the plain walk (entry-major
unit map) with the mechanism of test_gpu_tp_forward.test_launch_variants_are_bit_identical: identical bits in every slot but
those of the vector input blocks, the scalar blocks' narrowed ones included; the vector input blocks' shared walk sums edge pairs in another
association by design (PAIR_SUM_RTOL there), and their slots -- narrowed or not -- are held to that same bound here.
"""
import copy
import os

import numpy as np
import pytest
import torch

from common import PAPER, build_pair
from test_gpu_parity import BLOCK_RTOL, close_blocks
from test_gpu_tp_forward import PAIR_SUM_RTOL

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N_NODES = 70
DEGREES = (0, 1, 5, 19, 40)
SPECIES = (13, 29, 79)
NF = "node_features"
FRONT, LAYER = "layer2_convnet", "layer3_convnet"     # the layers in front of the tested one; the tested one


def _graph():
    """70 atoms in a 2.4 A box (every pair inside the 5 A cutoff, none closer than 0.5 A), node n with DEGREES[n % 5] incoming
    edges from random other nodes, species interleaved"""
    rng = np.random.default_rng(7)
    pos = []
    while len(pos) < N_NODES:
        cand = rng.uniform(0.0, 2.4, size=3)
        if all(np.linalg.norm(cand - q) >= 0.5 for q in pos):
            pos.append(cand)
    deg = np.array([DEGREES[n % len(DEGREES)] for n in range(N_NODES)])
    dst = np.repeat(np.arange(N_NODES), deg)
    src = (dst + rng.integers(1, N_NODES, size=dst.size)) % N_NODES      # never the node itself
    order = rng.permutation(dst.size)
    edge_index = np.stack([src[order], dst[order]]).astype(np.int64)
    g = {
        "pos": torch.as_tensor(np.asarray(pos), dtype=torch.float32),
        "edge_index": torch.as_tensor(edge_index),
        "edge_cell_shift": torch.zeros(dst.size, 3),
        "cell": torch.zeros(3, 3),
        "num_neigh": torch.as_tensor(np.bincount(edge_index[0], minlength=N_NODES), dtype=torch.float32),
        "atomic_numbers": torch.as_tensor(np.array([SPECIES[n % 3] for n in range(N_NODES)], dtype=np.int64)),
    }
    assert sorted(set(np.bincount(edge_index[1], minlength=N_NODES).tolist())) == sorted(DEGREES)
    return g


def _blocks(irreps):
    out, off = [], 0
    for mul, ir in irreps:
        out.append((off, off + mul * ir.dim, f"{mul}x{ir}"))
        off += mul * ir.dim
    return tuple(out)


def _run_front(backbone, data, upto):
    """the modules of a backbone in order up to and including `upto` -> the batch dict"""
    for name, m in backbone.named_children():
        data = m(data)
        if name == upto:
            return data
    raise KeyError(upto)


class Setup:
    pass


@pytest.fixture(scope="module")
def setup():
    import matten_amd.nn.conv as conv_mod
    from matten_amd.data.graph import collate

    s = Setup()
    hp = dict(PAPER, num_layers=4)
    ds = {"allowed_species": list(SPECIES), "average_num_neighbors": 18.0}
    old_rows, old_env = conv_mod.AGG_KM_MIN_ROWS, os.environ.get("MATTEN_AGG_NARROW")
    conv_mod.AGG_KM_MIN_ROWS = 0
    try:
        os.environ.pop("MATTEN_AGG_NARROW", None)
        s.ref, s.model = build_pair(hp, ds, randomize_bn=True)
        os.environ["MATTEN_AGG_NARROW"] = "0"
        _, s.model_plain = build_pair(hp, ds, randomize_bn=True)      # (the same seed: the same parameters)
    finally:
        if old_env is None:
            os.environ.pop("MATTEN_AGG_NARROW", None)
        else:
            os.environ["MATTEN_AGG_NARROW"] = old_env
    try:
        g = _graph()
        s.batch = collate([g])
        ref64 = copy.deepcopy(s.ref).double()
        to64 = lambda b: {k: (v.double() if isinstance(v, torch.Tensor) and v.is_floating_point() else v) for k, v in b.items()}
        with torch.no_grad():
            # fp64 oracle, every layer fed the fp32-rounded rows the product is fed
            d = _run_front(ref64.backbone, to64(s.batch), FRONT)
            s.x0 = d[NF].float()
            d = dict(d)
            d[NF] = s.x0.double()
            d = getattr(ref64.backbone, LAYER)(d)
            s.want1 = d[NF].clone()
            s.x1 = d[NF].float()
            d = dict(d)
            d[NF] = s.x1.double()
            s.want_last = ref64.backbone.conv_layer_last(d)[NF].clone()
            # the product's own front end fills the batch dict (CSR, geometry, harmonics, species order)
            s.front = {}
            for key, m in (("narrow", s.model), ("plain", s.model_plain)):
                s.front[key] = _run_front(m.backbone, collate([g], device=DEV), FRONT)
        yield s
    finally:
        conv_mod.AGG_KM_MIN_ROWS = old_rows
        torch.cuda.synchronize()


@pytest.fixture()
def nan_empty(monkeypatch):
    _empty = torch.empty
    monkeypatch.setattr(torch, "empty", lambda *a, **k: (lambda t: t.fill_(float("nan")) if t.is_floating_point() and t.is_cuda else t)(_empty(*a, **k)))


def _layer1(s, key):
    m = s.model if key == "narrow" else s.model_plain
    d = dict(s.front[key])
    d[NF] = s.x0.to(DEV)
    with torch.no_grad():
        return getattr(m.backbone, LAYER)(d)[NF]


def test_the_two_builds_launch_the_two_layouts(setup):
    s = setup
    conv_n, conv_p = getattr(s.model.backbone, LAYER).conv, getattr(s.model_plain.backbone, LAYER).conv
    assert conv_n.agg_plan.narrow is not None and conv_n.agg_plan.ld == 2560
    assert conv_p.agg_plan.narrow is None and conv_p.agg_plan.ld == 4352
    view = s.model.backbone.conv_layer_last._view
    assert view is not None and view.agg_plan.narrow is not None and s.model_plain.backbone.conv_layer_last._view.agg_plan.narrow is None
    for a, b in zip(s.model.state_dict().values(), s.model_plain.state_dict().values()):
        assert torch.equal(a, b)


def test_gated_layer_matches_the_fp64_oracle_per_block(setup, nan_empty):
    s = setup
    blocks = _blocks(getattr(s.model.backbone, LAYER).irreps_out[NF])
    assert blocks[-1][1] == s.want1.shape[1]
    for key in ("narrow", "plain"):
        got = _layer1(s, key)
        assert torch.isfinite(got).all(), key
        close_blocks(got, s.want1, blocks=blocks, rtol=BLOCK_RTOL, what=f"{LAYER} ({key} rows)")


def test_two_launches_give_identical_bits(setup, nan_empty):
    a, b = _layer1(setup, "narrow"), _layer1(setup, "narrow")
    assert torch.equal(a, b)


def test_inference_view_matches_the_fp64_oracle_per_block(setup, nan_empty):
    from matten_amd.o3 import Irreps

    s = setup
    full = Irreps(PAPER["conv_layer_irreps"])
    head = {str(ir) for _, ir in Irreps(PAPER["conv_to_output_hidden_irreps_out"])}
    cols, kept, off = [], [], 0
    for mul, ir in full:
        if str(ir) in head:
            cols += list(range(off, off + mul * ir.dim))
            kept.append((mul, ir))
        off += mul * ir.dim
    want = s.want_last[:, cols]
    for key in ("narrow", "plain"):
        m = s.model if key == "narrow" else s.model_plain
        d = dict(s.front[key])
        d[NF] = s.x1.to(DEV)
        with torch.no_grad():
            got = m.backbone.conv_layer_last(d)[NF]
        assert got.shape == want.shape and torch.isfinite(got).all(), (key, got.shape, want.shape)
        close_blocks(got, want, blocks=_blocks(kept), rtol=BLOCK_RTOL, what=f"last layer's view ({key} rows)")


def test_walk_forms_write_the_same_narrowed_rows(setup, nan_empty):
    from matten_amd import ops, plan as mplan
    from matten_amd.data.irreps import DataKey

    s = setup
    conv = getattr(s.model.backbone, LAYER).conv
    tp, ap, p = conv.tp, conv.agg_plan, conv.tp.plan
    data = s.front["narrow"]
    nb, r0, r1 = data[DataKey.AMD_RBF].tolist()
    x1 = torch.randn(N_NODES, p.d_in, generator=torch.Generator().manual_seed(3)).to(DEV)
    with torch.no_grad():
        h2p, w2p = tp.weight_nn.hidden(data[DataKey.AMD_GEOM], int(nb), r0, r1, data)
        entries, ld, narrow = conv._agg_out_layout(data, DEV)     # (the plan.narrow_blob buffer, row stride, (species per node, entries))
        assert narrow[0].dtype == torch.int32 and narrow[0].numel() == N_NODES and entries.dim() == 1 and narrow[1] == len(ap.entries)

        def run(umap):
            return ops.tp_fused(x1, h2p, w2p, data[DataKey.AMD_SH], data[DataKey.AMD_ROWPTR], data[DataKey.AMD_SRC], entries,
                                umap, umap.numel(), p.fused_lds_floats_per_wave, ld, 18.0, None, a_split=tp.a_split(r0, r1),
                                narrow=narrow)

        shared = run(torch.from_numpy(np.asarray(p.fused_unit_map)).to(DEV))
        plain = run(torch.from_numpy(mplan.fused_unit_map(p.group_entries, "entry")).to(DEV))
    # the slots the entries write: l1 = those of the vector input blocks, l0 = every other one; everything else is still NaN
    l0, l1, narrowed = (torch.zeros(ld, dtype=torch.bool) for _ in range(3))
    for e, paths in enumerate(p.group_entry_paths):
        mul = int(p.group_entry_mul[e])
        for c, pi in paths.items():
            ks, o, nw, _ = mplan.narrow_unpack(ap.entries[e][8 + c], ap.entries[e][20 + c])    # nw: mo of a narrowed coupling, else 0
            width = nw if nw else mul
            for k in range(2 * p.paths[pi].l3 + 1):
                sl = slice(o + k * ks, o + k * ks + width)
                (l1 if p.paths[pi].l1 == 1 else l0)[sl] = True
                if nw:
                    narrowed[sl] = True
    written = l0 | l1
    assert (l0 & narrowed).any() and (l1 & narrowed).any() and not (l0 & l1).any()
    shared, plain = shared.cpu(), plain.cpu()
    for name, t in (("shared", shared), ("plain", plain)):
        assert torch.isfinite(t[:, written]).all() and torch.isnan(t[:, ~written]).all(), name
    assert (shared[::5][:, written] == 0).all()                       # nothing arrives at nodes 0, 5, ...: exact zeros
    assert torch.equal(shared[:, l0], plain[:, l0]), "every block but the vector input blocks: the walk form changed the bits"
    # vector input blocks.  Un-narrowed slots: the bound of test_launch_variants_are_bit_identical, PAIR_SUM_RTOL of the largest
    # sum.  A narrowed slot is sum_u Wn[u][v] * sum[u][k] over the node's 8 lanes: the two walks' sums differ by at most
    # PAIR_SUM_RTOL x A each (A = the largest un-narrowed sum of these blocks, taken from the mul_ir row of the same operands),
    # which the slot sees times sum_u |Wn[u][v]|, plus the rounding of its own three levels of additions and one product,
    # 4 x 2^-24 of the same magnitude
    plain_only = l1 & ~narrowed
    err = (shared[:, plain_only].double() - plain[:, plain_only].double()).abs().max().item()
    assert err <= PAIR_SUM_RTOL * shared[:, plain_only].abs().max().item(), f"vector input blocks, un-narrowed slots: {err:.3e}"
    with torch.no_grad():
        um = torch.from_numpy(np.asarray(p.fused_unit_map)).to(DEV)
        mul_ir = ops.tp_fused(x1, h2p, w2p, data[DataKey.AMD_SH], data[DataKey.AMD_ROWPTR], data[DataKey.AMD_SRC],
                              tp._tables.get("gentries", DEV), um, um.numel(), p.fused_lds_floats_per_wave, p.d_mid, 18.0, None,
                              a_split=tp.a_split(r0, r1)).cpu()
    A = max(mul_ir[:, q.out_off: q.out_off + q.mul * (2 * q.l3 + 1)].abs().max().item() for q in p.paths if q.l1 == 1)
    n_ent = len(ap.entries)
    wn = entries[32 * n_ent:].cpu().view(torch.float32)     # the writer's weights behind the entries
    wsum = 0.0
    for e, paths in enumerate(p.group_entry_paths):
        if (int(ap.entries[e][0]) & 255) // mplan.TP_KIND_STRIDE != 1:
            continue
        for c in paths:
            nw = int(ap.narrow[e][c])
            if nw:
                mo, mul = nw & 255, int(p.group_entry_mul[e])
                off = nw >> 8
                blk = wn[off: off + len(SPECIES) * mul * mo].reshape(len(SPECIES), mul, mo)
                wsum = max(wsum, blk.abs().sum(1).max().item())
    assert A > 0 and wsum > 0
    sel = l1 & narrowed
    err_n = (shared[:, sel].double() - plain[:, sel].double()).abs().max().item()
    bound = (PAIR_SUM_RTOL + 4 * 2.0 ** -24) * wsum * A
    assert err_n <= bound, f"vector input blocks, narrowed slots: {err_n:.3e} > {bound:.3e}"
