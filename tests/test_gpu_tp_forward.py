"""
The fused tensor-product forward (csrc/tp_fused.hip, tp_walk.h, the generated cg_gen.h) at the operator level, per coupling
kind and per path, against a plain fp64 reference.

    agg[n] = norm(n) * sum_{e: dst(e) = n} uvu(x[src(e)], Y[e], w[e]),   w[e] = h2_eff[e] @ W2,
    norm(n) = 1/sqrt(avg) or 1/sqrt(num_neigh[n])  (a node nothing arrives at: agg[n] = 0 exactly)

Reference: the oracle's TensorProduct in fp64 + scatter + the normalisation.  h2_eff = hi + lo / 2048 is rebuilt in fp64 from
the kernel's own fp16 operands (ops.split_hidden), columns un-permuted by FEAT: the fp16 representation of the hidden
features is not kernel error.  W2 is uniform over its columns (the A fragments are scaled per entry by design).

Irreps (IRREPS) are chosen so that together they reach every generated kind of plan.TP_GROUPS (asserted by the `built`
fixture: a new kind must not arrive without a case), merged 2+2 entries, ragged last channel chunks, loader-only padding
waves, paired and shared workgroups.  Graphs: `ladder` (every in-degree 0..35 in varying positions of a 64-node tile, one
node with 600 in-edges in a ragged last tile of 8 nodes after which nothing arrives) and `tiny` (one edge); both
normalisations.

Every path's output block is compared with ITS OWN largest |reference| so that one wrong coefficient, a swapped pair of
output offsets or one lost edge slot of a weak coupling cannot hide under a strong neighbour.  Allowed per block:
min(2e-5, 8 r32) x the block's maximum, where r32 is the distance of the SAME oracle evaluated in fp32 on the CPU from the
fp64 one (largest over the paths, relative to the path block's maximum): 4x for the kernel's 22-bit split-fp16 products (two
bits fewer than fp32, the lo.lo term dropped), 2x for another summation order; 2e-5 is the project's per-path-block bound of
this operator (FWD_RTOL of the adjoint file).  Nothing here is derived from the kernel's own error.

r32 (it does not depend on the kernel): 0.9e-6 .. 1.5e-6 on the ladder graph with the fixed normalisation (the 600-edge sum
sets it), 0.4e-6 .. 0.65e-6 with the per-node one, 0.2e-6 .. 2.4e-6 on the single edge, i.e. 1.6e-6 .. 2e-5 of a block's
maximum allowed.  Both references sum a node's edges in one pass (REF_CHUNK).

Worst error / allowed per case family, measured on MI355X (whole / in pieces of 16 / of 3 edges; tp_paths at 2e-5):
                  ladder-avg             ladder-node            tiny-avg   tiny-node    tp_paths (worst of the four)
    paper         0.24 / 0.049 / 0.063   0.27 / 0.082 / 0.057   0.097      0.093        0.14
    paper_even    0.56 / 0.045 / 0.071   0.34 / 0.089 / 0.082   0.073      0.33         0.23
    lmax2         0.16 / 0.038 / 0.070   0.20 / 0.081 / 0.074   0.053      0.19         0.086
    ragged        0.40 / 0.066 / 0.069   0.43 / 0.11  / 0.093   0.33       0.089        0.18
    ragged_even   0.51 / 0.059 / 0.082   0.22 / 0.11  / 0.067   0.15       0.51         0.19
On the ladder the worst row of every case is the 600-edge node: 1e-6 .. 5e-6 of a block's maximum there against 1e-7 .. 5e-7
on the rows of 35 edges and fewer, the same in tp_paths and in the entry-major walk -- the rounding of one fp32 accumulator
over 600 terms; pieces summed afterwards are 5 .. 10 times closer.  The split-fp16 representation of W2 alone is 1e-7 of a
block's maximum (host emulation).  On the single edge the worst blocks are weak ones (block maximum 0.004 .. 0.03).

Found while writing the zero-row assertion, and fixed: with per-node normalisation a node nothing arrives at has
num_neigh = 0, and its empty sum is 0, not 0 x 1/sqrt(0) = NaN (the epilogues of tp_fused.hip and tp_path.hip select
norm = 0 there; "exactly 0" and "non-finite output" in _check_blocks, all *-node cases and test_hub_pieces).

Each of these fails the file (test_forward_matches_fp64_per_path's check on in-bounds mutations of the tables and operands
handed to the unchanged kernel, run once on MI355X; the unmutated launches of the same cases pass at 0.56 / 0.24 / 0.27):
    out_off words of couplings (1,2) and (3,2) of an alternative-kind entry (kind 1,2) swapped, paper_even-ladder-avg:
        block of path 1,1,2 at 1.5e5 x allowed
    one mask bit of a kind-2,0 entry cleared, paper-ladder-avg: "non-finite output" (4000 values: the block is never written and
        the NaN prefill shows; _nan_prefill checks itself that the allocator hands the NaN block back)
    num_neigh permuted among nodes 1..35, paper-ladder-node: block of path 0,0,0 at 3.3e5 x allowed
    lo half of h2p zeroed, paper-ladder-avg: block of path 0,0,0 at 15 x allowed
    one unit of a shared workgroup replaced by a copy of its neighbour (same node group), paper-ladder-avg: "non-finite
        output" (14336 values: that entry's node groups are never written)
"""
import copy
import math

import numpy as np
import pytest
import torch

from common import LMAX2, PAPER

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
AVG = 18.0
SH_STRIDE = 32            # production row stride of the harmonics (ops.SH_STRIDE); the columns past sh_dim hold NaN here
FWD_RTOL = 2e-5           # the project's per-path-block bound of this operator (test_gpu_tp_adjoint.FWD_RTOL)
R32_FACTOR = 8.0          # 4x (22-bit split-fp16 products, lo.lo dropped) x 2x (summation order): see the module docstring
PAIR_SUM_RTOL = 2e-6      # shared walk of the l1 = 1 blocks against the edge-by-edge walk (test_tp_kernels_agree_and_match_oracle)
REF_CHUNK = 8192          # edges per chunk of the references, as in test_gpu_tp_adjoint: a node's edges are summed in ONE pass.
                          # (Smaller chunks hand the fp32 oracle partial sums of the 600-edge segment -- a pairwise summation that no
                          # kernel walking a CSR segment front to back has -- and r32 drops to 0.4 of its value.)

# name -> (input irreps, sh lmax, target irreps or None = the input irreps)
IRREPS = {
    "paper": (PAPER["conv_layer_irreps"], 4, None),                  # the regular kinds; 2 merged entries; shared + paired
    "paper_even": (PAPER["conv_layer_irreps"], 4, "2x0e+2x2e+2x4e"),  # alternatives; a 3-entry workgroup (one loader-only wave)
    "lmax2": (LMAX2["conv_layer_irreps"], 2, None),                  # the lmax-2 alternatives (0,1) (1,4) (2,4)
    "ragged": ("1x0e+3x0o+5x1o+17x1e+33x2e+3x3o+1x4e", 4, None),     # channel chunks of 1, 3, 5: idle lanes, ragged last chunks
    "ragged_even": ("1x0e+3x0o+5x1o+17x1e+33x2e+3x3o+1x4e+2x3e+3x4o", 4, "0e+2e+4e"),   # (4,2); alternatives at odd multiplicities
}
COMPONENT_MAJOR = ("paper", "paper_even", "lmax2")   # plan.plan_agg_linear(p, 1, target) exists for these
CASES = [(i, g, n) for g in ("ladder", "tiny") for i in IRREPS for n in ("avg", "node")]
# h2s column g * 8 + kk <-> hidden feature 16 * (kk >> 2) + 4 * g + (kk & 3) (the MFMA B operand layout)
FEAT = [16 * (kk >> 2) + 4 * g + (kk & 3) for g in range(4) for kk in range(8)]


def _ids(cases):
    return ["-".join(c) for c in cases]


def _sh_irreps(lmax):
    from matten_amd.o3 import Irreps

    return Irreps.spherical_harmonics(lmax)


def _plan_of(irreps_in, lmax, target):
    from matten_amd import plan as mplan

    return mplan.plan_uvu(irreps_in, _sh_irreps(lmax), target or irreps_in)


def _plan(name):
    return _plan_of(*IRREPS[name])


def _kinds(p):
    """the generated kinds (l1, coupling group) a plan's entries run on"""
    from matten_amd import plan as mplan

    e = np.asarray(p.group_entries).reshape(-1, 32)
    return {((int(k) & 255) // mplan.TP_KIND_STRIDE, (int(k) & 255) % mplan.TP_KIND_STRIDE) for k in e[:, 0] if k >= 0}


def _assert_every_kind_has_a_case():
    from matten_amd import plan as mplan

    want = {(l1, gi) for l1, g in mplan.TP_GROUPS.items() for gi in range(len(g))}
    got = set().union(*(_kinds(_plan(name)) for name in IRREPS))
    assert got == want, f"kinds without a case here: {sorted(want - got)}; unknown kinds: {sorted(got - want)}"


def _graph(kind, gen):
    """-> (edge_index [2, E] int64, N) on the host"""
    if kind == "tiny":
        return torch.tensor([[3], [1]], dtype=torch.int64), 5
    # ladder: node n < 180 has in-degree n % 36 (0..35: odd ones, 15/16/17 and 31/32/33 around the 16-edge chunk, in varying
    # positions of a 64-node tile and of 16- and 32-node wave groups), node 180 has 600 in-edges, nothing arrives at 181..199
    # (with 180: the ragged last tile, 8 of 64 nodes); random sources, shuffled edge order
    N = 200
    deg = torch.tensor([n % 36 for n in range(180)] + [600] + [0] * 19)
    dst = torch.repeat_interleave(torch.arange(N), deg)
    assert dst.numel() == 3750
    src = torch.randint(N, (dst.numel(),), generator=gen)
    order = torch.randperm(dst.numel(), generator=gen)
    return torch.stack([src[order], dst[order]]), N


def _oracle_tp(name):
    return _oracle_tp_of(*IRREPS[name])


def _oracle_tp_of(irreps_in, lmax, target):
    """(fp64, fp32) copies of the oracle's tensor product (test_gpu_tp_narrow.py builds its own irreps with it)"""
    from oracle.matten_ref import nn as rnn

    ref = rnn.UVUTensorProduct(irreps_in, str(_sh_irreps(lmax)), target or irreps_in, mlp_input_size=8,
                               mlp_hidden_size=32, mlp_num_hidden_layers=2, mlp_activation=torch.nn.functional.silu)
    return copy.deepcopy(ref.tp).double(), copy.deepcopy(ref.tp).float()


def _reference(tp, x, Y, w, edge_index, N, nrm):
    """agg = scatter(tp(x[src], Y, w)) * nrm in the dtype of the operands, in edge chunks"""
    from oracle.e3nn_lite.scatter import scatter

    src, dst = edge_index
    agg = None
    for c0 in range(0, src.numel(), REF_CHUNK):
        sl = slice(c0, min(src.numel(), c0 + REF_CHUNK))
        part = scatter(tp(x[src[sl]], Y[sl], w[sl]), dst[sl], dim_size=N)
        agg = part if agg is None else agg + part
    return agg * nrm[:, None]


class Case:
    pass


def _build(param, shared):
    from matten_amd.nn._tables import DeviceTables

    irreps_name, graph, norm = param
    _, lmax, target = IRREPS[irreps_name]
    if irreps_name not in shared:
        p = _plan(irreps_name)
        tp64, tp32 = _oracle_tp(irreps_name)
        assert tp64.weight_numel == p.weight_numel and p.d_in == tp64.irreps_in1.dim
        shared[irreps_name] = (p, tp64, tp32, DeviceTables(gentries=p.group_entries, gumap=p.fused_unit_map,
                                                           path_entries=p.path_entries, unit_start=p.unit_start))
    p, tp64, tp32, tables = shared[irreps_name]
    gen = torch.Generator().manual_seed(2000 + CASES.index(param))
    c = Case()
    c.name, c.irreps_name, c.graph, c.norm = "-".join(param), irreps_name, graph, norm
    c.p, c.t = p, tables
    c.target = target or IRREPS[irreps_name][0]
    edge_index, N = _graph(graph, gen)
    x, Y, w64, w32 = _operands(c, lmax, edge_index, N, gen)
    num_neigh = c.in_deg.float()                          # 0 where nothing arrives, as in production
    c.avg = AVG if norm == "avg" else 0.0
    nrm = torch.full((N,), AVG ** -0.5, dtype=torch.float64) if norm == "avg" else \
        torch.where(c.rows_in, num_neigh.double().clamp(min=1) ** -0.5, torch.zeros((), dtype=torch.float64))
    c.nn = num_neigh.to(DEV) if norm == "node" else None

    # ---- the references: fp64, and the same oracle in fp32 whose distance from it sets the scale of the tolerance ----
    c.ref = _reference(tp64, x.double(), Y.double(), w64, edge_index, N, nrm)
    assert c.ref.shape == (N, p.d_mid)
    c.ref32 = ref32 = _reference(tp32, x, Y, w32, edge_index, N, nrm.float()).double()
    c.blocks = [(f"{q.l1},{q.l2},{q.l3}", slice(q.out_off, q.out_off + q.mul * (2 * q.l3 + 1))) for q in p.paths]
    c.r32 = max(_ratio((ref32[c.rows_in][:, sl] - c.ref[c.rows_in][:, sl]).abs().max().item(),
                       c.ref[c.rows_in][:, sl].abs().max().item()) for _, sl in c.blocks)
    assert 0 < c.r32 < 1e-5, c.r32                            # an fp32 evaluation of a few hundred terms per output
    c.rtol = min(FWD_RTOL, R32_FACTOR * c.r32)
    c.results = {}
    return c


def _operands(c, lmax, edge_index, N, gen):
    """the operands of one launch of plan c.p on a graph, set on c: everything but the normalisation.  -> the host values
    (x, Y, w fp64, w fp32 in the original edge order) the references are evaluated on (test_gpu_tp_narrow.py builds its
    cases with this too)"""
    from matten_amd import ops
    from oracle.e3nn_lite.o3 import spherical_harmonics

    p = c.p
    E, W = edge_index.shape[1], p.weight_numel
    c.N, c.E, c.W = N, E, W
    src, dst = edge_index
    c.in_deg = torch.bincount(dst, minlength=N)
    out_deg = torch.bincount(src, minlength=N)
    c.rows_in = c.in_deg > 0

    # ---- host operands (fp32 values; the references see exactly these values) ----
    x = torch.randn(N, p.d_in, generator=gen)
    vec = torch.randn(E, 3, generator=gen, dtype=torch.float64)
    Y = spherical_harmonics(list(range(lmax + 1)), vec, True, "component").float()
    assert Y.shape[1] == p.sh_dim
    h2 = torch.randn(E, 32, generator=gen)
    W2 = torch.randn(32, W, generator=gen) / 32 ** 0.5    # uniform over columns: the A fragments are scaled per entry

    # ---- device operands, built the way production builds them ----
    perm, rowptr, src_sorted, err = ops.csr_build(edge_index.to(DEV), N)
    assert int(err.item()) == 0
    c.perm = perm.long().cpu()
    c.rowptr, c.src = rowptr, src_sorted
    nan = float("nan")
    xd = x.clone()
    xd[out_deg == 0] = nan            # never read: no edge leaves these nodes
    c.x = xd.to(DEV)
    Yd = torch.full((E, SH_STRIDE), nan)
    Yd[:, : p.sh_dim] = Y
    c.Y = Yd[c.perm].to(DEV)
    cols = torch.as_tensor(p.fused_cols)
    w2f = torch.where(cols[None, :] >= 0, W2[:, cols.clamp(min=0)], W2.new_zeros(()))
    c.w2f = torch.nn.functional.pad(w2f, (0, (-w2f.shape[1]) % 16 + 16)).contiguous().to(DEV)   # >= 16 zero pad columns
    c.h2p = ops.split_hidden(h2[c.perm][:, FEAT].contiguous().to(DEV))
    c.a_split = ops.split_a_tiles(c.w2f, p.group_entries)

    # ---- the weights the kernel is given, in fp64: w = (hi + lo / 2048) @ W2 ----
    pieces = c.h2p.float().cpu().double()
    h2_eff = torch.empty(E, 32, dtype=torch.float64)
    h2_eff[:, FEAT] = pieces[:, 0] + pieces[:, 1] / 2048.0    # (sorted edge order)
    assert torch.equal(h2_eff.float().double(), h2_eff)       # 22 bits: the fp32 oracle below sees the same values
    h2_orig = torch.empty_like(h2_eff)
    h2_orig[c.perm] = h2_eff
    w64 = h2_orig @ W2.double()
    w32 = h2_orig.float() @ W2
    c.w_pad = (W + 16) // 16 * 16   # a multiple of 16 (tp_paths) with at least one pad column
    wd = torch.full((E, c.w_pad), nan)
    wd[:, :W] = w32
    c.w32 = wd[c.perm].to(DEV)
    return x, Y, w64, w32


@pytest.fixture(scope="module")
def built():
    """cases built so far (a test on a subset of CASES must not make pytest build a case twice)"""
    _assert_every_kind_has_a_case()
    cache = {"cases": {}, "shared": {}}
    yield cache
    cache.clear()
    torch.cuda.synchronize()


@pytest.fixture(scope="module", params=CASES, ids=_ids(CASES))
def case(request, built):
    if request.param not in built["cases"]:
        built["cases"][request.param] = _build(request.param, built["shared"])
    return built["cases"][request.param]


def _only(pred):
    cases = [c for c in CASES if pred(*c)]
    return pytest.mark.parametrize("case", cases, indirect=True, ids=_ids(cases))


def _ratio(err, allowed):
    """error / allowed; an exactly zero reference block allows no error at all"""
    if allowed > 0:
        return err / allowed
    return 0.0 if err == 0 else math.inf


def _nan_prefill(rows, cols):
    """NaN in the block the caching allocator hands out next for an output of this shape: what nobody writes must not pass
    as zeros.  Self-checking: the next torch.empty of the shape does get the NaN block back."""
    torch.full((rows, cols), float("nan"), device=DEV)
    probe = torch.empty(rows, cols, dtype=torch.float32, device=DEV)
    assert torch.isnan(probe).all(), "the allocator did not hand the freed NaN block back: the prefill checks nothing"
    del probe


def _fused(c, entries=None, umap=None, d_mid=None, a_split="host", rowptr=None, num_neigh="case", x=None, h2p=None):
    """ops.tp_fused on the case's operands: the production launch unless an argument replaces a table or an operand"""
    from matten_amd import ops

    p = c.p
    entries = c.t.get("gentries", DEV) if entries is None else entries
    umap = c.t.get("gumap", DEV) if umap is None else umap
    rowptr = c.rowptr if rowptr is None else rowptr
    d_mid = p.d_mid if d_mid is None else d_mid
    _nan_prefill(rowptr.shape[0] - 1, d_mid)
    return ops.tp_fused(c.x if x is None else x, c.h2p if h2p is None else h2p, c.w2f, c.Y, rowptr, c.src, entries, umap,
                        umap.numel(), p.fused_lds_floats_per_wave, d_mid, c.avg, c.nn if isinstance(num_neigh, str) else num_neigh,
                        a_split=c.a_split if isinstance(a_split, str) else a_split)


def _production(c):
    """the production launch (host-built A fragments, the plan's unit map), once per case"""
    if "production" not in c.results:
        c.results["production"] = _fused(c)
    return c.results["production"]


def _check_blocks(c, agg, what, rtol):
    """every path's output block against that block's own largest |reference| over the rows with in-edges; the rows
    without are exactly 0 and everything is finite -> (worst error / allowed, its path)"""
    assert agg.shape == (c.N, c.p.d_mid) and agg.dtype == torch.float32, (what, agg.shape, agg.dtype)
    got = agg.double().cpu()
    assert torch.isfinite(got).all(), f"{what}: non-finite output ({int((~torch.isfinite(got)).sum())} values)"
    assert (got[~c.rows_in] == 0).all(), f"{what}: a row without in-edges is not exactly 0"
    got, ref = got[c.rows_in], c.ref[c.rows_in]
    worst = (0.0, "-")
    for label, sl in c.blocks:
        scale = ref[:, sl].abs().max().item()
        r = _ratio((got[:, sl] - ref[:, sl]).abs().max().item(), rtol * scale)
        assert r <= 1.0, (f"{what}: block of path {label} (columns {sl.start}:{sl.stop}): error / allowed = {r:.3g} "
                          f"(block max {scale:.3e}, allowed {rtol:.3g} of it, r32 {c.r32:.3g})")
        worst = max(worst, (r, label))
    return worst


def test_forward_matches_fp64_per_path(case):
    c = case
    r, label = _check_blocks(c, _production(c), f"{c.name} tp_fused", c.rtol)
    print(f"\nTP_FORWARD_RATIO {c.name} {r:.3g} {label}   (r32 {c.r32:.3g}, allowed {c.rtol:.3g} of a block's maximum)")


def test_tp_paths_on_the_same_operands(case):
    """an independent kernel (one wave per path over a materialised w) on the same reference: an oracle-side mistake
    shows as both this and the fused test failing"""
    from matten_amd import ops

    c = case
    p, t = c.p, c.t
    _nan_prefill(c.N, p.d_mid)
    agg = ops.tp_paths(c.x, c.w32, c.Y, c.rowptr, c.src, t.get("path_entries", DEV), t.get("unit_start", DEV),
                       p.units_per_tile, p.d_mid, c.avg, c.nn)
    r, label = _check_blocks(c, agg, f"{c.name} tp_paths", FWD_RTOL)
    print(f"\nTP_PATHS_RATIO {c.name} {r:.3g} {label}")


def test_launch_variants_are_bit_identical(case, monkeypatch):
    """what must not depend on the launch: who splits the last layer into fp16 fragments, how many node groups a persistent
    unit walks, and -- but for the pair-summed vector blocks -- whether a workgroup shares its stage"""
    from matten_amd import plan as mplan

    c = case
    p = c.p
    f = _production(c)
    # host-built MFMA fragments of the last layer (production) == the kernel's own split of w2f
    assert torch.equal(_fused(c, a_split=None), f), "the kernel's own split of w2f"
    # persistent units change which wave visits a node, never the order in which a node's edges are summed
    for spec in ("", "16:2,8:2,4:2,2:2", "16:8,8:8,4:4,2:2"):
        monkeypatch.setenv("MATTEN_TP_PERSIST", spec)
        um = torch.from_numpy(mplan.fused_unit_map(p.group_entries)).to(DEV)
        monkeypatch.delenv("MATTEN_TP_PERSIST")
        assert torch.equal(_fused(c, umap=um), f), f"persistent units {spec!r} changed the result"
    # the unshared walk (entry-major unit map: every wave fetches its own rows) is the same arithmetic in the same order ...
    um = torch.from_numpy(mplan.fused_unit_map(p.group_entries, "entry")).to(DEV)
    f_plain = _fused(c, umap=um)
    # ... except for the vector (l1 = 1) input blocks, whose shared walk contracts the two edge slots of a pair in one pass
    # (the pair products of both edges are added before the coupling coefficients: cg_gen.h CG2): same sum, another association
    l1_cols = torch.zeros(p.d_mid, dtype=torch.bool)
    for pth in p.paths:
        if pth.l1 == 1:
            l1_cols[pth.out_off: pth.out_off + pth.mul * (2 * pth.l3 + 1)] = True
    assert l1_cols.any() and not l1_cols.all()
    l1_cols = l1_cols.to(DEV)
    assert torch.equal(f[:, ~l1_cols], f_plain[:, ~l1_cols]), "entry-major unit order"
    assert torch.isfinite(f_plain).all()
    want = f[:, l1_cols].double()
    err = (f_plain[:, l1_cols].double() - want).abs().max().item()
    assert err <= PAIR_SUM_RTOL * want.abs().max().item(), f"pair-summed l1 = 1 blocks vs the edge-by-edge walk: {err:.3e}"


@_only(lambda i, g, n: i in COMPONENT_MAJOR)
def test_component_major_rows(case):
    """the component-major row that production writes from 8192 nodes up (plan.AggLinearPlan.entries): slot
    out_off[c] + u + k * t_off[c] holds path c of the entry, channel u0 + u, component k -- the very numbers of the mul_ir row"""
    from matten_amd import plan as mplan

    c = case
    p = c.p
    ap = mplan.plan_agg_linear(p, 1, c.target)
    assert ap is not None and ap.ld >= p.d_mid
    ent = ap.entries
    slots, cols = [], []
    for e in range(len(ent)):
        for cc, pi in p.group_entry_paths[e].items():
            pth = p.paths[pi]
            d3 = 2 * pth.l3 + 1
            o, ks = int(ent[e][20 + cc]), int(ent[e][8 + cc])
            for u in range(int(p.group_entry_mul[e])):
                for k in range(d3):
                    slots.append(o + u + k * ks)
                    cols.append(pth.out_off + (p.group_entry_u0[e] + u) * d3 + k)
    # a bijection between the reference row and the used slots
    assert len(set(slots)) == len(slots) == p.d_mid and sorted(cols) == list(range(p.d_mid))
    assert 0 <= min(slots) and max(slots) < ap.ld
    got = _fused(c, entries=torch.from_numpy(np.ascontiguousarray(ent)).to(DEV), d_mid=ap.ld)
    assert got.shape == (c.N, ap.ld)
    assert torch.equal(got[:, torch.as_tensor(slots, device=DEV)], _production(c)[:, torch.as_tensor(cols, device=DEV)])


@_only(lambda i, g, n: g == "ladder")
@pytest.mark.parametrize("piece", [16, 3])
def test_hub_pieces(case, piece):
    """CSR segments walked in pieces as virtual nodes (ops.csr_split) and summed in order (ops.segment_reduce), as small
    batches run: 16 = the training forward's length; 3 gives node 180 two hundred pieces and every degree >= 4 a cut"""
    from matten_amd import ops

    c = case
    vrowptr, vseg, vnn = ops.csr_split(c.rowptr, c.E, piece, c.nn)
    assert (vnn is None) == (c.nn is None)
    n_virtual = int(vseg[-1].item())
    assert n_virtual == int(torch.clamp((c.in_deg + piece - 1) // piece, min=1).sum()) <= vrowptr.shape[0] - 1
    agg_v = _fused(c, rowptr=vrowptr, num_neigh=vnn)
    agg = ops.segment_reduce(agg_v, vseg, mean=False)
    r, label = _check_blocks(c, agg, f"{c.name} pieces of {piece}", c.rtol)
    print(f"\nTP_FORWARD_RATIO {c.name}-pieces{piece} {r:.3g} {label}")


@_only(lambda i, g, n: (i, g, n) == ("paper", "ladder", "avg"))
def test_strided_input_rows(case):
    """x as a column slice of a wider buffer (ops.tp_fused honours the row stride), the rest of the buffer NaN"""
    c = case
    wide = torch.full((c.N, 2 * c.p.d_in), float("nan"), device=DEV)
    wide[:, c.p.d_in:] = c.x
    xs = wide[:, c.p.d_in:]
    assert not xs.is_contiguous() and xs.stride(0) == 2 * c.p.d_in
    assert torch.equal(_fused(c, x=xs), _production(c))
