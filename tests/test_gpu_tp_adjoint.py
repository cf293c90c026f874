"""
The tensor-product adjoint (csrc/tp_backward.hip) at the operator level, per edge and per path, against a plain fp64 reference.

    agg[n] = norm(n) * sum_{e: dst(e) = n} uvu(x[src(e)], Y[e], w[e]),   norm(n) = 1/sqrt(avg) or 1/sqrt(num_neigh[n])

Given g = dL/dagg every route returns dx [N, d_in] and dw [E, ld] (destination-sorted edges).  Routes (test ids):
    lit-atomic / lit-ordered        matten_tp_backward_lit on a materialised w; dx by atomics / summed per source node in a
                                    fixed order (out_csr, rows_segment_sum_kernel)
    wfree-atomic / wfree-ordered    matten_tp_backward_lit_wfree: w re-evaluated on the matrix cores from fp16-split hidden
                                    features, paths taken in LDS rounds
    table-column / table-grouped    matten_tp_backward per weight column / grouped by input channel (in_ptr, in_cols)

Reference: the oracle's TensorProduct in fp64 + scatter + the normalisation, <g, agg> differentiated by autograd.  dw does not
depend on w, so every route has the same dw reference; dx of the w-free route uses w = (hi + lo / 2048) @ W2 rebuilt from the
kernel's own fp16 operands (the representation of h2 is not kernel error).

Every dw path is compared with ITS OWN largest |reference| and every dx input block with its own, so that one wrong coupling,
one wrong edge or a lost low half of the fp16 split cannot hide under a large neighbour.  Worst error / allowed over all cases,
measured on MI355X:
    fp32 dw, 2e-5 of the path max                       lit 0.022   wfree 0.022   table 0.017
    fp32 dx, 5e-5 of the block max                      lit 0.027   wfree 0.033   table 0.077
    bf16 dw, 2^-8 |ref| + 2e-5 of the path max          lit 0.986   wfree 0.986   table 0.986
    bf16 dx, bf16-rounded w, 5e-5 of the block max      lit 0.036   wfree 0.041   table 0.068
(bf16 dw is tight by construction: round-to-nearest to 8 significant bits errs by up to 2^-8 of a value just above a power of
two; the fp32 part of the error is what the 2e-5 term covers.)  Each of these fails the file: the w-free weights without the
low half of their fp16 split, num_neigh[src] for num_neigh[dst] in the literal kernel, two coupling cases of one l1 swapped.
"""
import copy
import math

import pytest
import torch

from common import LMAX2, PAPER

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
AVG = 18.0
SH_STRIDE = 32            # production row stride of the harmonics (ops.SH_STRIDE); the columns past sh_dim hold NaN here
DW_RTOL, DX_RTOL = 2e-5, 5e-5
BF16_REL = 2.0 ** -8
WFREE_VS_LIT_RTOL = 2e-6  # w-free dx against the literal route fed the same w in fp32
IDENTITY_RTOL = 1e-5
FWD_RTOL = 2e-5           # tp_paths per output path block
REF_CHUNK = 8192          # edges per chunk of the fp64 reference

# name -> (input irreps, sh lmax, target irreps or None = the input irreps)
IRREPS = {
    "lmax2": (LMAX2["conv_layer_irreps"], 2, None),               # the kernels' LMAX = 2 instantiation
    "paper": (PAPER["conv_layer_irreps"], 4, None),               # LMAX = 4, l1 = 3 and 4 blocks
    "ragged": ("1x0e+3x0o+5x1o+17x1e+33x2e+3x3o+1x4e", 3, None),  # idle lanes: channels below the lanes per edge
    "wide256": ("256x0e+4x1o", 2, None),                          # one edge per w-free workgroup
    "wide200": ("200x0e+7x1e+9x2o", 2, None),                     # a non-power-of-two block at 256 lanes
    "uncovered": ("4x0e+3x1o+4x4e", 1, "4x0e+3x1o"),              # the 4e block has no path: blocks_cover_input False
}
CASES = ([(i, g, n, "fp32") for i in IRREPS for g in ("hubs", "tiny", "empty") for n in ("avg", "node")]
         + [("lmax2", "large", n, "fp32") for n in ("avg", "node")]
         + [(i, "hubs", n, "bf16") for i in ("lmax2", "paper") for n in ("avg", "node")])
ROUTES = ("lit-atomic", "lit-ordered", "wfree-atomic", "wfree-ordered", "table-column", "table-grouped")
# h2s column g * 8 + kk <-> hidden feature 16 * (kk >> 2) + 4 * g + (kk & 3) (the MFMA B operand layout)
FEAT = [16 * (kk >> 2) + 4 * g + (kk & 3) for g in range(4) for kk in range(8)]


def _graph(kind, gen):
    """-> (edge_index [2, E] int64, N) on the host"""
    if kind == "empty":
        return torch.zeros(2, 0, dtype=torch.int64), 7
    if kind == "tiny":
        return torch.tensor([[3], [1]], dtype=torch.int64), 5
    if kind == "large":
        N = 4000
        return torch.randint(N, (2, 70_001), generator=gen), N
    # hubs: 300 nodes, 5000 edges; nodes[:30] have no edge at all, nodes[30:40] only send, nodes[40:50] only receive; one
    # destination with 600 in-edges, one source with 900 out-edges, 40 self-loops
    N = 300
    nodes = torch.randperm(N, generator=gen)
    src_pool, dst_pool, both = torch.cat([nodes[30:40], nodes[50:]]), nodes[40:], nodes[50:]
    hub_dst, hub_src = nodes[50], nodes[51]

    def pick(pool, n):
        return pool[torch.randint(len(pool), (n,), generator=gen)]

    n_rand, loops = 5000 - 600 - 900 - 40, pick(both, 40)
    src = torch.cat([pick(src_pool, 600), hub_src.repeat(900), pick(src_pool, n_rand), loops])
    dst = torch.cat([hub_dst.repeat(600), pick(dst_pool, 900), pick(dst_pool, n_rand), loops])
    order = torch.randperm(src.numel(), generator=gen)
    return torch.stack([src[order], dst[order]]), N


def _oracle_tp(irreps_in, lmax, target):
    from oracle.matten_ref import nn as rnn

    ref = rnn.UVUTensorProduct(irreps_in, str(_sh_irreps(lmax)), target or irreps_in, mlp_input_size=8,
                               mlp_hidden_size=32, mlp_num_hidden_layers=2, mlp_activation=torch.nn.functional.silu)
    return copy.deepcopy(ref.tp).double()


def _sh_irreps(lmax):
    from matten_amd.o3 import Irreps

    return Irreps.spherical_harmonics(lmax)


def _reference(tp, x, Y, ws, g, edge_index, N, nrm):
    """fp64: agg = scatter(tp(x[src], Y, w)) * nrm, then dL/dx [N, d_in] and dL/dw [E, W] (original edge order) of
    L = <g, agg> for each w in ws, in edge chunks -> ([agg], [dx], dw): dw from the first w (it does not depend on w)"""
    from oracle.e3nn_lite.scatter import scatter

    src, dst = edge_index
    E = src.numel()
    aggs = [torch.zeros(N, g.shape[1], dtype=torch.float64) for _ in ws]
    dxs = [torch.zeros_like(x) for _ in ws]
    dw = torch.zeros(E, ws[0].shape[1], dtype=torch.float64)
    for c0 in range(0, E, REF_CHUNK):
        sl = slice(c0, min(E, c0 + REF_CHUNK))
        for k, w in enumerate(ws):
            xl = x.clone().requires_grad_(True)
            wl = w[sl].clone().requires_grad_(True)
            agg = scatter(tp(xl[src[sl]], Y[sl], wl), dst[sl], dim_size=N) * nrm[:, None]
            gx, gw = torch.autograd.grad((g * agg).sum(), (xl, wl))
            aggs[k] += agg.detach()
            dxs[k] += gx
            if k == 0:
                dw[sl] = gw
            else:
                # the reference's own consistency: dw is the same for every w
                assert torch.allclose(gw, dw[sl], rtol=1e-12, atol=1e-12)
    return aggs, dxs, dw


class Case:
    pass


@pytest.fixture(scope="module", params=CASES, ids=["-".join(c) for c in CASES])
def case(request):
    from matten_amd import ops, plan as mplan
    from matten_amd.nn._tables import DeviceTables
    from oracle.e3nn_lite.o3 import spherical_harmonics

    irreps_name, graph, norm, storage = request.param
    irreps_in, lmax, target = IRREPS[irreps_name]
    gen = torch.Generator().manual_seed(1000 + CASES.index(request.param))
    c = Case()
    c.name, c.bf16 = "-".join(request.param), storage == "bf16"
    c.p = p = mplan.plan_uvu(irreps_in, _sh_irreps(lmax), target or irreps_in)
    tp = _oracle_tp(irreps_in, lmax, target)
    assert tp.weight_numel == p.weight_numel and p.d_in == tp.irreps_in1.dim
    c.tp = tp
    c.t = DeviceTables(**{k: getattr(p, k) for k in ("bw_blocks", "bw_paths", "bw_col_meta", "bw_nnz_ijk", "bw_nnz_c",
                                                      "bw_in_ptr", "bw_in_cols", "bw_w_entries", "path_entries",
                                                      "unit_start")})
    edge_index, N = _graph(graph, gen)
    E, W = edge_index.shape[1], p.weight_numel
    c.N, c.E, c.W = N, E, W
    c.w_pad = (W + 16) // 16 * 16   # a multiple of 16 (tp_paths) with at least one pad column
    src, dst = edge_index
    c.in_deg = torch.bincount(dst, minlength=N)
    c.out_deg = torch.bincount(src, minlength=N)

    # ---- host operands (fp32 values; the reference sees exactly these values in fp64) ----
    x = torch.randn(N, p.d_in, generator=gen)
    g = torch.randn(N, p.d_mid, generator=gen)
    vec = torch.randn(E, 3, generator=gen, dtype=torch.float64)
    Y = spherical_harmonics(list(range(lmax + 1)), vec, True, "component").float()
    assert Y.shape[1] == p.sh_dim
    w = torch.randn(E, W, generator=gen)
    if c.bf16:
        w = w.bfloat16().float()    # the reference of the materialised routes uses the stored (rounded) weights
    h2 = torch.randn(E, 32, generator=gen)
    W2 = torch.randn(32, W, generator=gen) / 32 ** 0.5
    num_neigh = c.in_deg.float()      # 0 where nothing arrives, as in production
    c.avg = AVG if norm == "avg" else 0.0
    nrm = torch.full((N,), AVG ** -0.5, dtype=torch.float64) if norm == "avg" else \
        torch.where(c.in_deg > 0, num_neigh.double().clamp(min=1) ** -0.5, torch.zeros((), dtype=torch.float64))

    # ---- device operands, built the way production builds them ----
    ei = edge_index.to(DEV)
    perm, rowptr, src_sorted, err = ops.csr_build(ei, N)
    assert int(err.item()) == 0
    c.perm = perm.long().cpu()
    c.rowptr, c.src = rowptr, src_sorted
    c.dst = ei[1][perm.long()].to(torch.int32).contiguous()
    pairs = torch.stack([src_sorted.long(), src_sorted.long()])
    out_perm, out_ptr, _, _ = ops.csr_build(pairs, N)
    c.out_csr = (out_ptr, out_perm)
    c.covered = int(p.bw_blocks[:, 1].dot(2 * p.bw_blocks[:, 2] + 1)) == p.d_in   # (autograd.py)
    nan = float("nan")
    xd = x.clone()
    xd[c.out_deg == 0] = nan          # never read: no edge leaves these nodes
    gd = g.clone()
    gd[c.in_deg == 0] = nan           # never read: no edge arrives
    c.x, c.g = xd.to(DEV), gd.to(DEV)
    Yd = torch.full((E, SH_STRIDE), nan)
    Yd[:, : p.sh_dim] = Y
    c.Y = Yd[c.perm].to(DEV)
    wd = torch.full((E, c.w_pad), nan)
    wd[:, :W] = w
    c.w = wd[c.perm].to(DEV, torch.bfloat16 if c.bf16 else torch.float32)
    c.nn = num_neigh.to(DEV) if norm == "node" else None
    # w-free operands: the hidden features split to fp16 pieces, the last layer's A fragments per path
    c.h2s = ops.split_hidden(h2[c.perm][:, FEAT].contiguous().to(DEV)) if E else \
        torch.empty(0, 2, 32, dtype=torch.float16, device=DEV)
    W2p = torch.zeros(32, c.w_pad)
    W2p[:, :W] = W2
    c.frag, c.inv = ops.split_a_tiles_dev(W2p.to(DEV), c.t.get("bw_w_entries", DEV), p.bw_a_tiles)
    pieces = c.h2s.float().cpu().double()
    h2_eff = torch.empty(E, 32, dtype=torch.float64)
    h2_eff[:, FEAT] = pieces[:, 0] + pieces[:, 1] / 2048.0    # (sorted edge order)
    w_wf = torch.empty(E, W, dtype=torch.float64)
    w_wf[c.perm] = h2_eff @ W2.double()
    c.w_wf32 = torch.full((E, c.w_pad), nan)
    c.w_wf32[:, :W] = w_wf.float()
    c.w_wf32 = c.w_wf32[c.perm].to(DEV)

    # ---- fp64 reference, mapped to the kernels' destination-sorted edge order ----
    (agg, agg_wf), (dx, dx_wf), dw = _reference(tp, x.double(), Y.double(), [w.double(), w_wf], g.double(), edge_index, N, nrm)
    c.ref_agg, c.ref_agg_wf = agg, agg_wf
    c.ref_dx, c.ref_dx_wf = dx, dx_wf
    c.ref_dw = dw[c.perm]
    yield c
    torch.cuda.synchronize()


def _run(c, route, lds_floats=None, w=None):
    """-> (dx, dw) of one route through matten_amd.ops"""
    from matten_amd import ops

    p, t = c.p, c.t
    kind, mode = route.split("-")
    w = c.w if w is None else w
    # NaN in the block the caching allocator hands out next for dx: output nobody writes (the ordered route's dx is
    # torch.empty) must not pass by being zero memory
    torch.full((c.N, p.d_in), float("nan"), device=DEV)
    if kind == "table":
        groups = (t.get("bw_in_ptr", DEV), t.get("bw_in_cols", DEV)) if mode == "grouped" else None
        return ops.tp_backward(c.x, w, c.Y, c.src, c.dst, t.get("bw_col_meta", DEV), t.get("bw_nnz_ijk", DEV),
                               t.get("bw_nnz_c", DEV), c.g, c.avg, c.nn, in_groups=groups)
    common = dict(out_csr=c.out_csr if mode == "ordered" else None, blocks_cover_input=c.covered, max_l=p.bw_max_l)
    if kind == "lit":
        return ops.tp_backward_lit(c.x, w, c.Y, c.src, c.dst, t.get("bw_blocks", DEV), t.get("bw_paths", DEV),
                                   p.bw_sum_lanes, c.g, c.avg, c.nn, **common)
    assert kind == "wfree"
    return ops.tp_backward_lit(c.x, None, c.Y, c.src, c.dst, t.get("bw_blocks", DEV), t.get("bw_paths", DEV), p.bw_sum_lanes,
                               c.g, c.avg, c.nn, wfree=(c.h2s, c.frag, c.inv),
                               dw_shape=((c.E, c.w_pad), torch.bfloat16 if c.bf16 else torch.float32),
                               lds_floats=lds_floats or p.bw_wfree_lds_floats, max_mul=p.bw_max_mul, **common)


def _ratio(err, allowed):
    """error / allowed; an exactly zero reference block allows no error at all"""
    if allowed > 0:
        return err / allowed
    return 0.0 if err == 0 else math.inf


def _check_dw(c, dw, what):
    """each path's columns against that path's largest |reference| -> worst error / allowed"""
    assert dw.shape == (c.E, c.w_pad) and dw.dtype == (torch.bfloat16 if c.bf16 else torch.float32), (what, dw.shape, dw.dtype)
    got = dw[:, : c.W].double().cpu()
    assert torch.isfinite(got).all(), f"{what}: non-finite dw"
    worst = 0.0
    if c.E == 0:
        return worst
    for pth in c.p.paths:
        sl = slice(pth.w_off, pth.w_off + pth.mul)
        ref, err = c.ref_dw[:, sl], (got[:, sl] - c.ref_dw[:, sl]).abs()
        scale = ref.abs().max().item()
        if c.bf16:
            allowed = BF16_REL * ref.abs() + DW_RTOL * scale
            r = 0.0 if scale == 0 and err.max().item() == 0 else (err / allowed).max().item()
        else:
            r = _ratio(err.max().item(), DW_RTOL * scale)
        assert r <= 1.0, (f"{what}: dw of path {pth.l1},{pth.l2},{pth.l3} (w_off {pth.w_off}, {pth.mul} channels): "
                          f"error / allowed = {r:.3g} (path max {scale:.3e})")
        worst = max(worst, r)
    return worst


def _check_dx(c, dx, ref, what, rtol=DX_RTOL):
    """each input irrep block against its own largest |reference| -> worst error / allowed"""
    assert dx.shape == (c.N, c.p.d_in) and dx.dtype == torch.float32, (what, dx.shape)
    got = dx.double().cpu()
    assert torch.isfinite(got).all(), f"{what}: non-finite dx"
    assert (got[c.out_deg == 0] == 0).all(), f"{what}: dx of a node without out-edges is not exactly 0"
    worst = 0.0
    for (mul, ir), sl in zip(c.tp.irreps_in1, c.tp.irreps_in1.slices()):
        err = (got[:, sl] - ref[:, sl]).abs().max().item()
        r = _ratio(err, rtol * ref[:, sl].abs().max().item())
        assert r <= 1.0, f"{what}: dx of block {mul}x{ir}: error / allowed = {r:.3g}"
        worst = max(worst, r)
    return worst


@pytest.mark.parametrize("route", ROUTES)
def test_adjoint_matches_fp64_per_edge_and_path(case, route):
    c = case
    dx, dw = _run(c, route)
    ref_dx = c.ref_dx_wf if route.startswith("wfree") else c.ref_dx
    r_dw = _check_dw(c, dw, f"{c.name} {route}")
    r_dx = _check_dx(c, dx, ref_dx, f"{c.name} {route}")
    if not c.covered:
        # the input block without a path gets exactly nothing on every route
        sl = c.tp.irreps_in1.slices()[-1]
        assert (dx[:, sl] == 0).all()
    print(f"\nTP_ADJOINT_RATIO {route} {c.name} dw {r_dw:.3g} dx {r_dx:.3g}")


def test_routes_agree_bit_for_bit(case):
    """what must not depend on the route: dw of the literal and w-free kernels (the same code; dw does not read w), of atomic
    and ordered dx, and a repeated ordered call (dx and dw); the w-free dx equals the literal route fed the same w"""
    c = case
    lit_a, lit_o, wf_a, wf_o = (_run(c, r) for r in ("lit-atomic", "lit-ordered", "wfree-atomic", "wfree-ordered"))
    assert torch.equal(lit_a[1][:, : c.W], lit_o[1][:, : c.W])
    assert torch.equal(wf_a[1][:, : c.W], wf_o[1][:, : c.W])
    assert torch.equal(lit_o[1][:, : c.W], wf_o[1][:, : c.W])
    for route, first in (("lit-ordered", lit_o), ("wfree-ordered", wf_o)):
        again = _run(c, route)
        assert torch.equal(again[0], first[0]) and torch.equal(again[1][:, : c.W], first[1][:, : c.W]), route
    # the operand convention of the w-free kernel (h2s column order, fragment scale): its dx is the literal route's on
    # w = h2_eff @ W2 in fp32, up to the rounding of w (fp32 storage: a bf16 w would round it further)
    if not c.bf16:
        lit_wf = _run(c, "lit-ordered", w=c.w_wf32)
        _check_dx(c, wf_o[0], lit_wf[0].double().cpu(), f"{c.name} wfree vs lit on the same w", rtol=WFREE_VS_LIT_RTOL)


def _rounds(p, lds_floats):
    """LDS rounds of every input block in matten_tp_backward_lit_wfree (lit_block_wfree's per_round)"""
    out = []
    for _x, mul, _l1, w in p.bw_blocks:
        cu = 1 << max(0, (int(mul) - 1).bit_length())
        epw, tw, n_paths = 256 // cu, (int(mul) + 3) // 4 * 4, int(w) >> 16
        per = max(1, (lds_floats // epw - 4) // tw)
        out.append(-(-n_paths // per))
    return out


def test_wfree_narrow_tile_is_bit_identical(case):
    """paths taken in more LDS rounds (the library's smallest tile, 2048 floats) change nothing: dx accumulates in the same
    order and every w is evaluated by the same matrix instructions"""
    c = case
    p = c.p
    name = c.name.split("-")[0]
    if name == "lmax2":
        assert p.bw_wfree_lds_floats == 2048
    if name in ("paper", "ragged"):
        assert _rounds(p, 2048) != _rounds(p, p.bw_wfree_lds_floats), "2048 floats should move some block to more rounds"
    dx, dw = _run(c, "wfree-ordered")
    dx2, dw2 = _run(c, "wfree-ordered", lds_floats=2048)
    assert torch.equal(dx, dx2)
    assert torch.equal(dw[:, : c.W], dw2[:, : c.W])


def test_adjoint_identity_and_forward(case):
    """<g, agg> = <dx, x> = <dw, w> for every route, independent of the oracle, with agg from the forward kernel
    (ops.tp_paths) on the same operands; the forward itself per output path block against the fp64 agg"""
    from matten_amd import ops

    c = case
    p, t = c.p, c.t
    rows_in, rows_out = c.in_deg > 0, c.out_deg > 0
    if c.E == 0:
        # no edge: nothing to aggregate and nothing to differentiate (the forward's entry wants edge buffers)
        for route in ROUTES:
            dx, dw = _run(c, route)
            assert (dx == 0).all() and dw.shape[0] == 0, route
        return
    aggs = {}
    for key, w_dev, ref in (("w", c.w, c.ref_agg), ("w_wf", c.w_wf32, c.ref_agg_wf)):
        agg = ops.tp_paths(c.x, w_dev, c.Y, c.rowptr, c.src, t.get("path_entries", DEV), t.get("unit_start", DEV),
                           p.units_per_tile, p.d_mid, c.avg, c.nn).double().cpu()[rows_in]
        ref = ref[rows_in]
        for pth in p.paths:
            sl = slice(pth.out_off, pth.out_off + pth.mul * (2 * pth.l3 + 1))
            err = (agg[:, sl] - ref[:, sl]).abs().max().item()
            r = _ratio(err, FWD_RTOL * ref[:, sl].abs().max().item())
            assert r <= 1.0, f"{c.name}: tp_paths on {key}, block of path {pth.l1},{pth.l2},{pth.l3}: error / allowed = {r:.3g}"
        aggs[key] = (w_dev, agg)
    gs = c.g.double().cpu()[rows_in]
    xs = c.x.double().cpu()[rows_out]
    for route in ROUTES:
        w_dev, agg = aggs["w_wf" if route.startswith("wfree") else "w"]
        dx, dw = _run(c, route)
        ga = (gs * agg).sum().item()
        tol = IDENTITY_RTOL * (gs.abs() * agg.abs()).sum().item()
        xdx = (xs * dx.double().cpu()[rows_out]).sum().item()
        wdw_terms = w_dev.double().cpu()[:, : c.W] * dw.double().cpu()[:, : c.W]
        wdw = wdw_terms.sum().item()
        assert abs(xdx - ga) <= tol, f"{c.name} {route}: <dx, x> = {xdx:.9e} vs <g, agg> = {ga:.9e} (allowed {tol:.3e})"
        # bf16 dw: every value rounded to 8 bits, i.e. by at most 2^-9 of itself
        tol_w = tol + (BF16_REL * wdw_terms.abs().sum().item() if c.bf16 else 0.0)
        assert abs(wdw - ga) <= tol_w, f"{c.name} {route}: <dw, w> = {wdw:.9e} vs <g, agg> = {ga:.9e} (allowed {tol_w:.3e})"


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """The argument contract of matten_tp_backward_lit, _lit_wfree (one launcher body behind both) and _sh, called through the
    C ABI on the `uncovered` plan with E = 4, N = 3 and every buffer valid: each bad argument alone gives MATTEN_EINVAL with
    dx / dw / dy untouched; an empty batch zeroes dx in the ordered mode (out_ptr marks it) and touches nothing otherwise."""
    from matten_amd import _lib, ops, plan as mplan
    from matten_amd.nn._tables import DeviceTables

    lib = _lib.load()
    irreps_in, lmax, target = IRREPS["uncovered"]
    p = mplan.plan_uvu(irreps_in, _sh_irreps(lmax), target)
    t = DeviceTables(bw_blocks=p.bw_blocks, bw_paths=p.bw_paths, bw_w_entries=p.bw_w_entries)
    blocks, paths = t.get("bw_blocks", DEV), t.get("bw_paths", DEV)
    E, N, W = 4, 3, p.weight_numel
    ld = (W + 16) // 16 * 16
    gen = torch.Generator().manual_seed(7)
    rnd = lambda *shape: torch.randn(*shape, generator=gen).to(DEV)
    x, g, w, Y = rnd(N, p.d_in), rnd(N, p.d_mid), rnd(E, ld), rnd(E, SH_STRIDE)
    src = torch.tensor([0, 1, 1, 2], dtype=torch.int32, device=DEV)
    dst = torch.tensor([0, 0, 1, 2], dtype=torch.int32, device=DEV)
    out_ptr = torch.tensor([0, 1, 3, 4], dtype=torch.int32, device=DEV)
    out_perm = torch.arange(E, dtype=torch.int32, device=DEV)
    num_neigh = torch.tensor([2.0, 1.0, 1.0], device=DEV)
    h2s = ops.split_hidden(rnd(E, 32))
    W2p = torch.zeros(32, ld)
    W2p[:, :W] = torch.randn(32, W, generator=gen)
    frag, w_inv = ops.split_a_tiles_dev(W2p.to(DEV), t.get("bw_w_entries", DEV), p.bw_a_tiles)
    SENTINEL = 7.0
    dx, dx_edges = torch.empty(N, p.d_in, device=DEV), torch.zeros(E, p.d_in, device=DEV)   # (zeros: the 4e block has no path)
    dw, dy = torch.empty(E, ld, device=DEV), torch.empty(E, SH_STRIDE, device=DEV)
    outs = (dx, dw, dy)
    ptr = lambda v: v.data_ptr() if isinstance(v, torch.Tensor) else v

    shared = dict(sh=Y, sh_stride=SH_STRIDE, src=src, dst=dst, blocks=blocks, n_blocks=blocks.shape[0], sum_lanes=p.bw_sum_lanes,
                  paths=paths, n_paths=paths.shape[0], g_agg=g, d_mid=p.d_mid, avg=AVG, num_neigh=num_neigh, n_edges=E, dx=dx,
                  dw=dw, dw_ld=ld, bf16=0, n_nodes=N, out_ptr=out_ptr, out_perm=out_perm, dx_edges=dx_edges)
    base = {
        "lit": dict(x=x, d_in=p.d_in, w_edge=w, w_ld=ld, **shared, max_l=p.bw_max_l),
        "wfree": dict(x=x, d_in=p.d_in, h2s=h2s, frag=frag, w_inv=w_inv, **shared, lds_floats=p.bw_wfree_lds_floats,
                      max_l=p.bw_max_l, max_mul=p.bw_max_mul),
        "sh": dict(x=x, d_in=p.d_in, w_edge=w, w_ld=ld, src=src, dst=dst, blocks=blocks, n_blocks=blocks.shape[0],
                   max_mul=p.bw_max_mul, paths=paths, n_paths=paths.shape[0], g_agg=g, d_mid=p.d_mid, avg=AVG,
                   num_neigh=num_neigh, n_edges=E, bf16=0, dy=dy, sh_stride=SH_STRIDE, max_l=p.bw_max_l),
    }
    entry = {"lit": lib.matten_tp_backward_lit, "wfree": lib.matten_tp_backward_lit_wfree, "sh": lib.matten_tp_backward_sh}

    def call(kind, **change):
        """-> the entry's return code with `change` applied to the valid arguments; the outputs start as the sentinel"""
        for o in outs:
            o.fill_(SENTINEL)
        args = dict(base[kind], **change)
        rc = entry[kind](*(ptr(v) for v in args.values()), ops._stream())
        torch.cuda.synchronize()
        return rc

    def untouched():
        return all(bool((o == SENTINEL).all()) for o in outs)

    n_blocks = blocks.shape[0]
    both = [dict(n_blocks=0), dict(n_paths=0), dict(d_mid=0), dict(dw_ld=0), dict(sum_lanes=0), dict(out_ptr=None),
            dict(avg=0.0, num_neigh=None)]
    bad = {
        "lit": both + [dict(w_ld=0), dict(sum_lanes=4096 * n_blocks + 1), dict(w_edge=None)],
        "wfree": both + [dict(sum_lanes=256 * n_blocks + 1), dict(lds_floats=2047), dict(lds_floats=15 * 1024 + 1),
                         dict(max_mul=0), dict(max_mul=257), dict(h2s=None), dict(frag=None), dict(w_inv=None)],
        "sh": [dict(sh_stride=8, max_l=2), dict(sh_stride=24, max_l=3), dict(max_l=5), dict(max_mul=0)],
    }
    for kind, changes in bad.items():
        for change in changes:
            assert call(kind, **change) == -1, (kind, change)          # MATTEN_EINVAL
            assert untouched(), (kind, change)
    for kind in ("lit", "wfree"):
        assert call(kind, n_edges=0) == 0, kind                        # ordered mode: nobody else initialises dx
        assert bool((dx == 0).all()) and bool((dw == SENTINEL).all()), kind
        assert call(kind, n_edges=0, out_ptr=None, out_perm=None, dx_edges=None) == 0, kind
        assert untouched(), kind
    # the valid arguments themselves are accepted, so each refusal above is the changed argument's
    for kind, out in (("lit", dx), ("wfree", dx), ("sh", dy)):
        assert call(kind) == 0, kind
        assert not bool((out == SENTINEL).any()), kind
