"""
torch.autograd bindings of the HIP operators for the training step.

The reference trains by autograd through e3nn's einsums and torch_scatter (model/model.py:276-372).  Here
each operator's adjoint is a hand-written kernel (matten_amd/csrc/tp_backward.hip, backward.hip); autograd only chains them
and carries the cheap differentiable re-packings of the parameters (index + scale).  The radial MLP runs forward
(matten_radial_mlp) and backward (matten_radial_mlp_bwd) on this library's own fp32-MFMA kernels; no library GEMM is
left on the step (the 16-wide species embedding is an index lookup).
"""
from typing import Optional

import os

import torch

from . import ops


class SpeciesEmbedFn(torch.autograd.Function):
    """node features of the one-hot embedding, ``feats`` as the species_embed kernel computed them; the adjoint sums the
    incoming gradient per species with the weight-gradient kernel of the species linear (input = the constant 1:
    dWp[s, w] = sum over the species' rows of dy[n, w]; ordered partial sums, no atomics, no index sort)."""

    @staticmethod
    def forward(ctx, weight, bias, feats, species_order, segs):
        ctx.species_order, ctx.segs = species_order, segs   # segs: int32 [[0, 1, 1, 0, dim, 0, 0, 0]] on the device
        ctx.n_species = weight.shape[1]
        return feats.view_as(feats)

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        n, dim = g.shape
        ones = torch.ones(n, 1, dtype=torch.float32, device=g.device)
        per_species = ops.species_linear_wgrad(ones, g, ctx.species_order, ctx.n_species, [ctx.segs], dim)   # [S, dim]
        return per_species.t(), per_species.sum(0), None, None, None


class SpeciesLinearFn(torch.autograd.Function):
    """out = add + x W_species  (matten_species_linear) from the flat e3nn ``weight``.
    The per-species packing packed[s, j] = weight[gather[s, j]] * scale[j] is part of this node (one autograd node and
    one Function.apply per linear instead of two: the eager step is bound by that host work at small batches): forward
    packs (and, when x needs a gradient, emits the per-path transposed packing from the same launch), backward runs
    the same kernel with W^T for dx, the weight-gradient kernel for the packed gradient, and maps that back through
    the inverse permutation (``gather`` is a bijection: no index sort, no atomics)."""

    @staticmethod
    def forward(ctx, x, weight, add, mod, species_order):
        plan, dev, t = mod.plan, x.device, mod._tables
        gather, scale = t.get("gather", dev), t.get("scale", dev)
        if ctx.needs_input_grad[0]:
            wp, wpt = ops.gather_scale(weight, gather, scale, perm2=t.get("perm_t", dev))
        else:
            wp, wpt = ops.gather_scale(weight, gather, scale), None
        segs = [t.get(f"meta{i}", dev) for i in range(len(plan.passes))]
        ctx.mod, ctx.species_order, ctx.wpt = mod, species_order, wpt
        ctx.save_for_backward(x, wp)
        ctx.has_add = add is not None
        return ops.species_linear(x, species_order, wp, plan.w_stride, segs, plan.d_out, add, plan.fully_covered)

    @staticmethod
    def backward(ctx, g):
        x, wp = ctx.saved_tensors
        mod, plan, dev = ctx.mod, ctx.mod.plan, g.device
        t = mod._tables
        g = g.contiguous()
        dx = dweight = None
        if ctx.needs_input_grad[0]:
            segs_t = [t.get(f"meta_t{i}", dev) for i in range(len(plan.passes_t))]
            dx = ops.species_linear(g, ctx.species_order, ctx.wpt, plan.w_stride, segs_t, plan.d_in, None,
                                    plan.input_covered)
        if ctx.needs_input_grad[1]:
            segs = [t.get(f"meta{i}", dev) for i in range(len(plan.passes))]
            n_species = wp.shape[0] if wp.dim() == 2 else 1
            dwp = ops.species_linear_wgrad(x, g, ctx.species_order, n_species, segs, plan.w_stride)
            dweight = ops.gather_scale(dwp.reshape(-1), t.get("gather_inv", dev), t.get("scale", dev), scale_by_source=True)
        return dx, dweight, (g if ctx.has_add else None), None, None


# Storage type of the two per-edge tensors of a training step, the radial weights w[E, W] and their gradient -- at
# large batches the step's dominant memory traffic (BASELINE.json configs[3] names bf16 storage; the reference itself
# is fp32 throughout, data/_dtype.py:3).  bf16 is opt-in (MATTEN_EDGE_STORAGE=bf16 or set_edge_storage_dtype): the MLP
# kernel rounds w to bf16 on the store (nearest even), every kernel computes and accumulates in fp32, node features,
# neighbour sums, BatchNorm statistics and all parameters stay fp32.
EDGE_STORAGE_DTYPE = torch.bfloat16 if os.environ.get("MATTEN_EDGE_STORAGE", "fp32").lower() == "bf16" else torch.float32


def set_edge_storage_dtype(dtype) -> None:
    global EDGE_STORAGE_DTYPE
    if dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("edge storage is fp32 or bf16")
    EDGE_STORAGE_DTYPE = dtype


# The radial MLP of any depth (nn.utils.RadialMLP: layer0 .. layer{L}): the shipped L = 2 on the original entries (one
# middle layer w1), every other depth on the _deep ones (the middle layers as one [L-1, 32, 32] tensor).
def _radial_pack(mlp, ws):
    """raw layers -> (w0p, middle layers packed, w2p) in the reference's column order, one launch"""
    if not mlp.deep:
        return ops.radial_pack(*ws, mlp.pack_scales())
    return ops.radial_pack_deep(ws[0], _stack_mid(ws), ws[-1], mlp.pack_scales())


def _stack_mid(ws):
    return torch.stack(ws[1:-1]) if len(ws) > 2 else ws[0].new_zeros(0, 32, 32)


def _radial_mlp(mlp, geom, rbf, w0p, w1p, w2p):
    return (ops.radial_mlp_deep if mlp.deep else ops.radial_mlp)(geom, *rbf, w0p, w1p, w2p, out_dtype=EDGE_STORAGE_DTYPE)


def _radial_mlp_bwd(mlp, geom, rbf, w0p, w1p, w2p, dw, scales) -> tuple:
    """one gradient per raw layer (layer0 .. layer{L})"""
    nb, W = mlp.hs[0], mlp.hs[-1]
    # the kernels multiply their partial sums by the packing factors: gradients w.r.t. the raw layers come back
    if not mlp.deep:
        d0, d1, d2 = ops.radial_mlp_bwd(geom, *rbf, w0p, w1p, w2p, W, dw, scales=scales)
        return d0[:nb], d1, d2[:, :W]
    d0, dm, d2 = ops.radial_mlp_bwd_deep(geom, *rbf, w0p, w1p, w2p, W, dw, scales=scales)
    return (d0[:nb], *dm.unbind(0), d2[:, :W])


class RadialMLPFn(torch.autograd.Function):
    """w[E, w_pad] = MLP(bessel(|edge|)) in the reference's weight-column order (pad columns zero); the adjoint maps
    dL/dw back to the raw weight matrices ws = (layer0 .. layer{L}) (the packing is a per-layer scale and a row padding)."""

    @staticmethod
    def forward(ctx, mod, geom_sorted, n_basis, r_start, r_end, *ws):
        w0p, w1p, w2p = _radial_pack(mod, ws)          # one launch for all layers
        ctx.mod, ctx.rbf = mod, (int(n_basis), float(r_start), float(r_end))
        ctx.save_for_backward(geom_sorted, w0p, w1p, w2p)
        return _radial_mlp(mod, geom_sorted, ctx.rbf, w0p, w1p, w2p)

    @staticmethod
    def backward(ctx, g):
        geom, w0p, w1p, w2p = ctx.saved_tensors
        mod = ctx.mod
        g = g.contiguous()
        dgeom = None
        if ctx.needs_input_grad[1]:
            # geometry gradients: only the length column of geom_sorted feeds the MLP (matten_radial_mlp_bwd_len)
            dgeom = torch.zeros_like(geom)
            dgeom[:, 3] = ops.radial_mlp_bwd_len(geom, *ctx.rbf, w0p, w1p, w2p, mod.hs[-1], g)
        if any(ctx.needs_input_grad[5:]):
            grads = _radial_mlp_bwd(mod, geom, ctx.rbf, w0p, w1p, w2p, g, mod.pack_scales())
        else:   # every layer frozen (saliency)
            grads = (None,) * (len(ctx.needs_input_grad) - 5)
        return (None, dgeom, None, None, None) + grads


class EdgeGeomFn(torch.autograd.Function):
    """(geom_sorted, sh_sorted) = matten_edge_geom(pos, cell) with its adjoint kernel (matten_edge_geom_bwd): gradients
    for positions and cells.  ``graph`` = (edge_index, edge_cell_shift, batch, perm, rowptr, (out_ptr, out_perm), ptr);
    the requested original-order tensors (edge_vectors, ...) land in ``extras`` and carry no gradient.  The backward
    receives the sums over all conv layers of dL/dgeom (only its length column is ever non-zero) and dL/dsh.  Once
    differentiable."""

    @staticmethod
    def forward(ctx, pos, cell, graph, lmax, rbf, wants, extras):
        edge_index, shift, batch, perm, rowptr, out_csr, ptr = graph
        out = ops.edge_geom(pos, edge_index, shift, cell, batch, perm, lmax, *rbf, **wants)
        geom, sh = out.pop("geom_sorted"), out.pop("sh_sorted")
        extras.update(out)
        ctx.graph, ctx.lmax, ctx.n_nodes = (shift, perm, rowptr, out_csr, ptr), lmax, pos.shape[0]
        ctx.cell_shape = None if cell is None else cell.shape
        ctx.save_for_backward(geom)
        ctx.set_materialize_grads(False)
        return geom, sh

    @staticmethod
    def backward(ctx, dgeom, dsh):
        (geom,) = ctx.saved_tensors
        shift, perm, rowptr, out_csr, ptr = ctx.graph
        want_cell = ctx.cell_shape is not None and ctx.needs_input_grad[1]
        n_cells = ctx.cell_shape.numel() // 9 if want_cell else 0   # (ops.edge_geom reads the cells as [-1, 3, 3])
        dlen = None if dgeom is None else dgeom[:, 3].contiguous()
        dpos, dcell = ops.edge_geom_bwd(geom, None if dsh is None else dsh.contiguous(), dlen, ctx.lmax, ctx.n_nodes, rowptr,
                                        out_csr, perm, shift if want_cell else None, n_cells, ptr)
        if dcell is not None:
            dcell = dcell.reshape(ctx.cell_shape)
        return dpos, dcell, None, None, None, None, None


# training forward: batches below this many nodes walk their CSR segments in pieces (see TensorProductScatterFn.forward)
TRAIN_HUB_SPLIT_MAX_ROWS = int(os.environ.get("MATTEN_HUB_SPLIT_MAX_ROWS_TRAIN", "65536"))


class TensorProductScatterFn(torch.autograd.Function):
    """agg = sum_{edges -> n} uvu(x[src], Y, w) * norm   with w[E,W] in the reference column order.  Y (``sh``, the batch's
    harmonics) is an input: when it requires grad (geometry gradients) the backward returns dL/dY as well
    (matten_tp_backward_sh); autograd adds the conv layers' contributions."""

    @staticmethod
    def forward(ctx, x, w_edge, sh, mod, data, avg, num_neigh):
        from .data.irreps import DataKey

        dev = x.device
        p = mod.plan
        ctx.mod, ctx.avg, ctx.num_neigh = mod, avg, num_neigh
        ctx.graph = (data[DataKey.AMD_SRC], data["_amd_dst_sorted"])
        ctx.out_csr = data.get("_amd_out_csr")
        ctx.save_for_backward(x, w_edge, sh)   # sh: the batch's harmonics, an input so that autograd sees the dependency
        # the forward walks a destination node's CSR segment serially: irregular batches (real crystals: 30 neighbours on
        # average, 80 in the one-atom cells) are cut into pieces of <= HUB_SPLIT_LEN edges and summed in order afterwards,
        # like the inference forward of small batches (nn/utils.py); the adjoint is per edge and does not care
        from .nn import utils as nnu

        rowptr, split = data[DataKey.AMD_ROWPTR], None
        if nnu.HUB_SPLIT_LEN > 0 and x.shape[0] < TRAIN_HUB_SPLIT_MAX_ROWS:
            # (its own cache key: the inference forward cuts the same rowptr into pieces of another length)
            key = ("_amd_csr_split", nnu.HUB_SPLIT_LEN, num_neigh is None)
            split = data.get(key)
            if split is None or split[3] is not rowptr:
                split = ops.csr_split(rowptr, data[DataKey.AMD_SRC].shape[0], nnu.HUB_SPLIT_LEN, num_neigh) + (rowptr,)
                data[key] = split
        agg = ops.tp_paths(x, w_edge, sh, rowptr if split is None else split[0], data[DataKey.AMD_SRC],
                           mod._tables.get("entries", dev), mod._tables.get("unit_start", dev), p.units_per_tile,
                           p.d_mid, avg, num_neigh if split is None else split[2])
        return agg if split is None else ops.segment_reduce(agg, split[1], mean=False)

    @staticmethod
    def backward(ctx, g):
        x, w_edge, sh = ctx.saved_tensors
        mod, dev = ctx.mod, g.device
        src, dst = ctx.graph
        impl = os.environ.get("MATTEN_TP_BWD", "lit")   # "lit": literal-coefficient kernel; "table": the table-driven ones
        dsh = None
        if ctx.needs_input_grad[2]:   # geometry gradients: the third adjoint, on the tables of the literal kernel
            if impl != "lit":
                raise NotImplementedError("MATTEN_TP_BWD=table has no adjoint for the edge harmonics: geometry gradients "
                                          "need MATTEN_TP_BWD=lit (the default)")
            dsh = ops.tp_backward_sh(x, w_edge, src, dst, mod._tables.get("bw_blocks", dev), mod._tables.get("bw_paths", dev),
                                     mod.plan.bw_max_mul, g.contiguous(), ctx.avg, ctx.num_neigh, max_l=mod.plan.bw_max_l,
                                     sh_stride=sh.shape[1])
        if impl == "lit":
            # dx summed per source node in a fixed order (MATTEN_TP_BWD_DX=atomic: fp32 atomics, order not fixed)
            out_csr = ctx.out_csr if os.environ.get("MATTEN_TP_BWD_DX", "ordered") != "atomic" else None
            dx, dw = ops.tp_backward_lit(x, w_edge, sh, src, dst, mod._tables.get("bw_blocks", dev),
                                         mod._tables.get("bw_paths", dev), mod.plan.bw_sum_lanes, g.contiguous(), ctx.avg,
                                         ctx.num_neigh, out_csr=out_csr, max_l=mod.plan.bw_max_l,
                                         blocks_cover_input=int(mod.plan.bw_blocks[:, 1].dot(2 * mod.plan.bw_blocks[:, 2] + 1))
                                         == mod.plan.d_in)
            return dx, dw, dsh, None, None, None, None
        dx, dw = ops.tp_backward(x, w_edge, sh, src, dst, mod._tables.get("bw_col_meta", dev),
                                 mod._tables.get("bw_nnz_ijk", dev), mod._tables.get("bw_nnz_c", dev), g.contiguous(),
                                 ctx.avg, ctx.num_neigh,
                                 in_groups=None if os.environ.get("MATTEN_TP_BWD_GROUPED", "1") == "0" else
                                 (mod._tables.get("bw_in_ptr", dev), mod._tables.get("bw_in_cols", dev)))
        return dx, dw, None, None, None, None, None


# training on the fused forward: the adjoint re-evaluates w inside its workgroups (0 = matten_radial_mlp writes it for one layer
# at a time inside the backward, the round-3 form)
W_FREE_ADJOINT = os.environ.get("MATTEN_TP_BWD_WFREE", "1") != "0"


class FusedTensorProductFn(torch.autograd.Function):
    """The training tensor product on the PRODUCTION kernel (MATTEN_TRAIN_TP=fused): forward = matten_tp_fused -- the last
    radial layer on the matrix cores inside the kernel, the per-edge weights w[E, W] never reach memory -- and nothing
    per-edge is kept for the backward except what the batch already holds (geometry, harmonics).  The backward
    re-evaluates w for THIS layer with matten_radial_mlp (0.1 ms per layer at 290 k edges), runs the literal adjoint and
    the radial MLP's adjoint, and drops w again: w exists for one layer at a time, inside the backward only (at batch
    2048 that is 4 x 1 GB less live memory between the passes).  The fused kernel's operands (weights in fused column
    order, range scale, fp16 hi/lo fragments) come from the raw layers through three small kernels
    (ops.fused_operands), so the step stays capturable."""

    @staticmethod
    def forward(ctx, x, mod, data, avg, num_neigh, *ws):
        from .data.irreps import DataKey

        dev = x.device
        p, mlp = mod.plan, mod.weight_nn
        nb, r0, r1 = data[DataKey.AMD_RBF].tolist()
        ctx.mod, ctx.avg, ctx.num_neigh = mod, avg, num_neigh
        ctx.rbf = (int(nb), float(r0), float(r1))
        ctx.graph = (data[DataKey.AMD_GEOM], data[DataKey.AMD_SH], data[DataKey.AMD_SRC], data["_amd_dst_sorted"])
        ctx.out_csr = data.get("_amd_out_csr")
        ctx.save_for_backward(x, *ws)
        # the fused kernel's operands from the raw layers: four small launches, nothing read on the host (the inference
        # path derives them once with library ops and caches them; here the parameters change every step)
        gent = mod._tables.get("gentries", dev)
        if mlp.deep:
            w0p, w1p, w2p, hs, frag, inv = ops.fused_operands_deep(ws[0], _stack_mid(ws), ws[-1], mlp.pack_scales(),
                                                                   mod._tables.get("fused_cols", dev), gent, p.fused_a_tiles,
                                                                   r0, r1, mlp.act_cst)
            h2p = ops.radial_hidden_deep(data[DataKey.AMD_GEOM], int(nb), r0, r1, w0p, w1p, hs)
        else:
            w0p, w1p, w2p, hs, frag, inv = ops.fused_operands(*ws, mlp.pack_scales(), mod._tables.get("fused_cols", dev),
                                                              gent, p.fused_a_tiles, r0, r1, mlp.act_cst)
            h2p = ops.radial_hidden(data[DataKey.AMD_GEOM], int(nb), r0, r1, w0p, w1p, hs)
        # the hidden features (128 B per edge) are what the backward re-evaluates w from; a layer with an input block wider
        # than the w-free kernel's workgroup (ops.WFREE_MAX_MUL channels) keeps the adjoint on a materialised w instead
        if W_FREE_ADJOINT and p.bw_max_mul <= ops.WFREE_MAX_MUL:
            ctx.h2p, ctx.hs = h2p, hs
        return ops.tp_fused(x, h2p, w2p, data[DataKey.AMD_SH], data[DataKey.AMD_ROWPTR], data[DataKey.AMD_SRC], gent,
                            mod._tables.get("gumap", dev), len(p.fused_unit_map), p.fused_lds_floats_per_wave, p.d_mid, avg,
                            num_neigh, a_split=(frag, inv))

    @staticmethod
    def backward(ctx, g):
        x, *ws = ctx.saved_tensors
        mod, dev = ctx.mod, g.device
        mlp = mod.weight_nn
        geom, sh, src, dst = ctx.graph
        scales = mlp.pack_scales()
        w0p, w1p, w2p = _radial_pack(mlp, ws)                                     # reference column order
        out_csr = ctx.out_csr if os.environ.get("MATTEN_TP_BWD_DX", "ordered") != "atomic" else None
        covered = int(mod.plan.bw_blocks[:, 1].dot(2 * mod.plan.bw_blocks[:, 2] + 1)) == mod.plan.d_in
        h2p = getattr(ctx, "h2p", None)
        if h2p is not None:
            # w-free: every workgroup of the adjoint re-evaluates its weights on the matrix cores from the forward's hidden
            # features and the last layer's A fragments in reference column order (one small launch); w never exists
            frag, inv = ops.split_a_tiles_dev(w2p, mod._tables.get("bw_w_entries", dev), mod.plan.bw_a_tiles, ctx.hs)
            dx, dw = ops.tp_backward_lit(x, None, sh, src, dst, mod._tables.get("bw_blocks", dev),
                                         mod._tables.get("bw_paths", dev), mod.plan.bw_sum_lanes, g.contiguous(), ctx.avg,
                                         ctx.num_neigh, out_csr=out_csr, blocks_cover_input=covered, wfree=(h2p, frag, inv),
                                         dw_shape=((geom.shape[0], w2p.shape[1]), EDGE_STORAGE_DTYPE),
                                         lds_floats=mod.plan.bw_wfree_lds_floats, max_l=mod.plan.bw_max_l,
                                         max_mul=mod.plan.bw_max_mul)
            # (h2p stays on the ctx until autograd releases it: a second backward under retain_graph takes the same route)
        else:
            w_edge = _radial_mlp(mlp, geom, ctx.rbf, w0p, w1p, w2p)   # transient
            dx, dw = ops.tp_backward_lit(x, w_edge, sh, src, dst, mod._tables.get("bw_blocks", dev),
                                         mod._tables.get("bw_paths", dev), mod.plan.bw_sum_lanes, g.contiguous(), ctx.avg,
                                         ctx.num_neigh, out_csr=out_csr, blocks_cover_input=covered, max_l=mod.plan.bw_max_l)
            del w_edge
        return (dx, None, None, None, None) + _radial_mlp_bwd(mlp, geom, ctx.rbf, w0p, w1p, w2p, dw, scales)


class GateFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mod):
        dev = x.device
        ctx.mod = mod
        ctx.save_for_backward(x)
        return ops.gate_bn(x, mod._tables.get("meta", dev), mod._tables.get("act_cst", dev))

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        mod, dev = ctx.mod, g.device
        return ops.gate_bwd(x, mod._tables.get("meta", dev), mod._tables.get("act_cst", dev), g.contiguous()), None


class NormActFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mod):
        ctx.mod = mod
        ctx.save_for_backward(x)
        return ops.norm_act(x, mod._tables.get("chan", x.device), mod.plan.act_code, mod.plan.epsilon)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        mod = ctx.mod
        return ops.norm_act_bwd(x, g.contiguous(), mod._tables.get("chan", g.device), mod.plan.act_code,
                                mod.plan.epsilon), None


class GateBnEvalFn(torch.autograd.Function):
    """BatchNorm(Gate(x)) with the BatchNorm in eval mode (frozen running statistics): the forward is the inference kernel
    (matten_gate_bn with the running statistics), the adjoint re-evaluates the activated value from x
    (matten_gate_bn_eval_bwd) -- gradients for x and the affine parameters, the running statistics are only read."""

    @staticmethod
    def forward(ctx, x, weight, bias, mod, bn):
        dev = x.device
        ctx.mod, ctx.bn = mod, bn
        ctx.save_for_backward(x, weight, bn.running_mean, bn.running_var)
        return ops.gate_bn(x, mod._tables.get("meta", dev), mod._tables.get("act_cst", dev), bn.running_mean,
                           bn.running_var, weight, bias, eps=bn.eps)

    @staticmethod
    def backward(ctx, g):
        x, weight, rm, rv = ctx.saved_tensors
        mod, bn, dev = ctx.mod, ctx.bn, g.device
        dx, dweight, dbias = ops.gate_bn_eval_bwd(
            x, mod._tables.get("meta", dev), mod._tables.get("act_cst", dev), bn._tables.get("chan", dev), rm, rv, weight,
            bn.eps, g, bn.bias.numel(), param_grads=ctx.needs_input_grad[1] or ctx.needs_input_grad[2])
        return dx, dweight, dbias, None, None


class NormActBnEvalFn(torch.autograd.Function):
    """BatchNorm(NormActivation(x)) with the BatchNorm in eval mode: matten_norm_act with the running statistics forward,
    matten_norm_act_bn_eval_bwd backward (see GateBnEvalFn)."""

    @staticmethod
    def forward(ctx, x, weight, bias, mod, bn):
        ctx.mod, ctx.bn = mod, bn
        ctx.save_for_backward(x, weight, bn.running_mean, bn.running_var)
        return ops.norm_act(x, mod._tables.get("chan", x.device), mod.plan.act_code, mod.plan.epsilon, bn.running_mean,
                            bn.running_var, weight, bias, bn.eps)

    @staticmethod
    def backward(ctx, g):
        x, weight, rm, rv = ctx.saved_tensors
        mod, bn = ctx.mod, ctx.bn
        dx, dweight, dbias = ops.norm_act_bn_eval_bwd(
            x, g, mod._tables.get("chan", g.device), mod.plan.act_code, mod.plan.epsilon, rm, rv, weight, bn.eps,
            bn.bias.numel(), param_grads=ctx.needs_input_grad[1] or ctx.needs_input_grad[2])
        return dx, dweight, dbias, None, None


class BatchNormTrainFn(torch.autograd.Function):
    """e3nn BatchNorm with batch statistics; the running averages are updated in place by the statistics kernel
    (running = (1 - momentum) running + momentum batch), so the step needs no small library launches for them.
    n_valid (optional): the device word of a padded batch (``_amd_n_valid``); the statistics, the running averages and
    the adjoint's reductions then run over the rows in front of it only."""

    @staticmethod
    def forward(ctx, x, weight, bias, bn, n_valid=None):
        dev = x.device
        y, mean, nu = ops.bn_train_fwd(x, bn._tables.get("col2chan", dev), bn._tables.get("chan", dev), weight, bias,
                                       bn.eps, bn.running_mean, bn.running_var, bn.momentum, n_valid=n_valid)
        ctx.bn = bn
        ctx.save_for_backward(x, weight, mean, nu, n_valid)
        return y

    @staticmethod
    def backward(ctx, g):
        x, weight, mean, nu, n_valid = ctx.saved_tensors
        bn, dev = ctx.bn, g.device
        dx, dweight, dbias = ops.bn_train_bwd(x, g.contiguous(), bn._tables.get("col2chan", dev),
                                              bn._tables.get("chan", dev), mean, nu, weight, bn.eps, bn.bias.numel(),
                                              n_valid=n_valid)
        return dx, dweight, dbias, None, None


class InstanceNormFn(torch.autograd.Function):
    """the reference's InstanceNorm (per-crystal statistics; same arithmetic as BatchNormTrainFn per crystal)"""

    @staticmethod
    def forward(ctx, x, weight, bias, norm, ptr, batch):
        dev = x.device
        y, mean, nu = ops.instance_norm_fwd(x, ptr, batch, norm._tables.get("col2chan", dev), norm._tables.get("chan", dev),
                                            weight, bias, norm.eps)
        ctx.norm = norm
        ctx.save_for_backward(x, weight, mean, nu, ptr, batch)
        return y

    @staticmethod
    def backward(ctx, g):
        x, weight, mean, nu, ptr, batch = ctx.saved_tensors
        norm, dev = ctx.norm, g.device
        dx, A, B = ops.instance_norm_bwd(x, g.contiguous(), ptr, batch, norm._tables.get("col2chan", dev),
                                         norm._tables.get("chan", dev), mean, nu, weight, norm.eps)
        dweight = (A * torch.rsqrt(nu + norm.eps)).sum(0)
        dbias = B.sum(0)[norm._tables.get("scalar_chan", dev)]
        return dx, dweight, dbias, None, None, None


class SegmentReduceFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, ptr, mean):
        ctx.ptr, ctx.mean, ctx.n = ptr, mean, x.shape[0]
        return ops.segment_reduce(x, ptr, mean)

    @staticmethod
    def backward(ctx, g):
        return ops.segment_reduce_bwd(g.contiguous(), ctx.ptr, ctx.n, ctx.mean), None, None


class SegmentMinMaxFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, ptr, take_max):
        out, arg = ops.segment_minmax(x, ptr, take_max, want_arg=True)
        ctx.n = x.shape[0]
        ctx.save_for_backward(arg)
        return out

    @staticmethod
    def backward(ctx, g):
        (arg,) = ctx.saved_tensors
        return ops.segment_minmax_bwd(g.contiguous(), arg, ctx.n), None, None


class ElasticPropsFn(torch.autograd.Function):
    """(voigt, compliance, props, flags) = matten_elastic_props(c) with its adjoint kernel (matten_elastic_props_bwd): the
    backward works from the four outputs alone, so the input is not kept.  An output that nothing downstream used
    reaches the kernel as a null pointer, not as a zero tensor; ``flags`` carries no gradient."""

    @staticmethod
    def forward(ctx, c, layout):
        voigt, compliance, props, flags = ops.elastic_props(c, layout)
        ctx.layout, ctx.dtype = layout, c.dtype
        ctx.save_for_backward(voigt, compliance, props, flags)
        ctx.mark_non_differentiable(flags)
        ctx.set_materialize_grads(False)
        return voigt, compliance, props, flags

    @staticmethod
    def backward(ctx, g_voigt, g_compliance, g_props, _g_flags):
        voigt, compliance, props, flags = ctx.saved_tensors
        if g_props is None:
            g_props = torch.zeros_like(props)
        return ops.elastic_props_bwd(voigt, compliance, props, flags, g_props, g_voigt, g_compliance, ctx.layout,
                                     ctx.dtype), None


class ElasticDirectionalFn(torch.autograd.Function):
    """(young, beta, ext, arg) = matten_elastic_directional(compliance) with its adjoint kernel
    (matten_elastic_directional_bwd), which works from the compliance and the recorded direction indices alone.  Only the
    compliance receives a gradient; ``arg`` carries none; an output that nothing downstream used reaches the kernel as a
    null pointer."""

    @staticmethod
    def forward(ctx, compliance, flags, dirs, keep):
        young, beta, ext, arg = ops.elastic_directional(compliance, flags, dirs, keep=keep)
        ctx.save_for_backward(compliance, flags, dirs, arg)
        ctx.mark_non_differentiable(arg)
        ctx.set_materialize_grads(False)
        return young, beta, ext, arg

    @staticmethod
    def backward(ctx, g_young, g_beta, g_ext, _g_arg):
        compliance, flags, dirs, arg = ctx.saved_tensors
        return ops.elastic_directional_bwd(compliance, flags, dirs, g_young, g_beta, g_ext, arg), None, None, None


class ElasticAcousticFn(torch.autograd.Function):
    """(vel, ext, arg, n_unstable) = matten_elastic_acoustic(voigt) with its adjoint kernel (matten_elastic_acoustic_bwd),
    which runs the Jacobi sweeps again with eigenvectors.  Only the Voigt matrix receives a gradient (not the density,
    not the directions); ``arg`` and ``n_unstable`` carry none."""

    @staticmethod
    def forward(ctx, voigt, flags, density, dirs, modulus_unit, keep):
        vel, ext, arg, n_unstable = ops.elastic_acoustic(voigt, flags, density, dirs, modulus_unit, keep=keep)
        ctx.modulus_unit = modulus_unit
        ctx.save_for_backward(voigt, flags, density, dirs, arg)
        ctx.mark_non_differentiable(arg, n_unstable)
        ctx.set_materialize_grads(False)
        return vel, ext, arg, n_unstable

    @staticmethod
    def backward(ctx, g_vel, g_ext, _g_arg, _g_unstable):
        voigt, flags, density, dirs, arg = ctx.saved_tensors
        return (ops.elastic_acoustic_bwd(voigt, flags, density, dirs, ctx.modulus_unit, g_vel, g_ext, arg), None, None, None,
                None, None)


class ElasticKelvinFn(torch.autograd.Function):
    """(moduli, vectors, dilatation) = matten_elastic_kelvin(voigt, flags) with its adjoint kernel
    (matten_elastic_kelvin_bwd): the backward works from the forward's vectors alone, so the input is not kept and Jacobi
    is not run again.  Only the moduli are differentiated, and only ``voigt`` receives a gradient; ``vectors`` and
    ``dilatation`` carry none.  ``want_dilatation=False`` (a loss that reads the moduli alone) hands the kernel a null pointer
    for the dilatation, which then comes back as None; the vectors are always written, the adjoint needs them.  When nothing
    downstream used the moduli no kernel runs and no zero tensor is made."""

    @staticmethod
    def forward(ctx, voigt, flags, want_dilatation=True):
        moduli, vectors, dilatation = ops.elastic_kelvin(voigt, flags, want_dilatation=bool(want_dilatation))
        ctx.save_for_backward(vectors, flags)
        ctx.mark_non_differentiable(*(t for t in (vectors, dilatation) if t is not None))
        ctx.set_materialize_grads(False)
        return moduli, vectors, dilatation

    @staticmethod
    def backward(ctx, g_moduli, _g_vectors, _g_dilatation):
        if g_moduli is None:
            return None, None, None
        vectors, flags = ctx.saved_tensors
        return ops.elastic_kelvin_bwd(vectors, flags, g_moduli.contiguous()), None, None


class ElasticPolycrystalFn(torch.autograd.Function):
    """(out, media, status) = matten_elastic_polycrystal(voigt, flags, moduli, vectors) with its adjoint kernel
    (matten_elastic_polycrystal_bwd).  Of ``out`` only the self-consistent pair (columns 2 and 3) is differentiated -- the
    Hashin-Shtrikman columns carry no gradient, whatever arrives for them is dropped -- and only ``voigt`` receives one:
    ``moduli`` and ``vectors`` are the decomposition of that same ``voigt``, the adjoint is the total derivative with respect
    to it.  When nothing downstream used ``out`` no kernel runs."""

    @staticmethod
    def forward(ctx, voigt, flags, moduli, vectors, hs_grid, sc_tol, sc_max_iter):
        out, media, status = ops.elastic_polycrystal(voigt, flags, moduli, vectors, hs_grid, sc_tol, sc_max_iter)
        ctx.save_for_backward(voigt, flags, out, status)
        ctx.mark_non_differentiable(media, status)
        ctx.set_materialize_grads(False)
        return out, media, status

    @staticmethod
    def backward(ctx, g_out, _g_media, _g_status):
        if g_out is None:
            return None, None, None, None, None, None, None
        voigt, flags, out, status = ctx.saved_tensors
        return (ops.elastic_polycrystal_bwd(voigt, flags, out, status, g_out[:, 2:4].contiguous()), None, None, None, None,
                None, None)


class TextureAverageFn(torch.autograd.Function):
    """(out, status) = matten_texture_average(voigt, flags, moduli, vectors, ...) with its adjoint
    (matten_texture_average_bwd).  Only ``voigt`` receives a gradient -- ``moduli`` and ``vectors`` are the decomposition of
    that same ``voigt``, the adjoint is the total derivative with respect to it --; the operators, the member lists and the
    fractions carry none.  ``crystal_ptr`` / ``crystal_member`` are the inverse of ``member_crystal``, built once by the
    caller.  When nothing downstream used ``out`` no kernel runs."""

    @staticmethod
    def forward(ctx, voigt, flags, moduli, vectors, op, tex_flags, member_crystal, member_texture, member_fraction, agg_ptr,
                crystal_ptr, crystal_member):
        out, status = ops.texture_average(voigt, flags, moduli, vectors, op, tex_flags, member_crystal, member_texture,
                                          member_fraction, agg_ptr)
        ctx.save_for_backward(moduli, vectors, op, tex_flags, member_crystal, member_texture, member_fraction, agg_ptr, out,
                              status, crystal_ptr, crystal_member)
        ctx.mark_non_differentiable(status)
        ctx.set_materialize_grads(False)
        return out, status

    @staticmethod
    def backward(ctx, g_out, _g_status):
        if g_out is None:
            return (None,) * 12
        moduli, vectors, op, tex_flags, mc, mt, mf, agg_ptr, out, status, crystal_ptr, crystal_member = ctx.saved_tensors
        g = ops.texture_average_bwd(moduli, vectors, op, tex_flags, mc, mt, mf, agg_ptr, out, status, g_out.contiguous(),
                                    crystal_ptr, crystal_member)
        return (g,) + (None,) * 11


class Rank2PropsFn(torch.autograd.Function):
    """(vals, axes, props, flags) = matten_rank2_props(t) with its adjoint kernel (matten_rank2_props_bwd): the backward
    works from the four outputs alone, so the input is not kept and Jacobi is not run again.  An output that nothing
    downstream used reaches the kernel as a null pointer; ``axes`` and ``flags`` carry no gradient."""

    @staticmethod
    def forward(ctx, t):
        vals, axes, props, flags = ops.rank2_props(t)
        ctx.dtype = t.dtype
        ctx.save_for_backward(vals, axes, props, flags)
        ctx.mark_non_differentiable(axes, flags)
        ctx.set_materialize_grads(False)
        return vals, axes, props, flags

    @staticmethod
    def backward(ctx, g_vals, _g_axes, g_props, _g_flags):
        vals, axes, props, flags = ctx.saved_tensors
        return ops.rank2_props_bwd(vals, axes, props, flags, g_vals, g_props, ctx.dtype)


class IrrepsRotateFn(torch.autograd.Function):
    """out = matten_irreps_rotate(x): linear in x, the backward is the same kernel with transpose = 1.  The rotation table
    (D, flags), the layout and the index carry no gradient."""

    @staticmethod
    def forward(ctx, x, layout, D, flags, index):
        ctx.layout = layout
        ctx.save_for_backward(D, flags, index)
        return ops.irreps_rotate(x, layout, D, flags, index)

    @staticmethod
    def backward(ctx, g):
        D, flags, index = ctx.saved_tensors
        return ops.irreps_rotate(g.contiguous(), ctx.layout, D, flags, index, transpose=True), None, None, None, None


class IrrepsAverageFn(torch.autograd.Function):
    """(out, deviation) = matten_irreps_average(x): out is linear in x, its backward the same kernel with transpose = 1 and
    the same lists and weights.  ``deviation`` is a diagnostic and carries no gradient, nor do the rotations and weights."""

    @staticmethod
    def forward(ctx, x, layout, D, flags, op_ptr, op_idx, weights):
        ctx.layout = layout
        ctx.save_for_backward(D, flags, op_ptr, op_idx, weights)
        out, deviation = ops.irreps_average(x, layout, D, flags, op_ptr, op_idx, weights)
        ctx.mark_non_differentiable(deviation)
        return out, deviation

    @staticmethod
    def backward(ctx, g, _g_deviation):
        D, flags, op_ptr, op_idx, weights = ctx.saved_tensors
        g_x, _ = ops.irreps_average(g.contiguous(), ctx.layout, D, flags, op_ptr, op_idx, weights, transpose=True,
                                    want_deviation=False)
        return g_x, None, None, None, None, None, None


class DenseRowsFn(torch.autograd.Function):
    """out = x @ q (matten_dense_rows) for a constant q [n_in, n_out]; the adjoint is the same kernel with q^T, which the
    caller keeps next to q (``qt`` [n_out, n_in])."""

    @staticmethod
    def forward(ctx, x, q, qt):
        ctx.save_for_backward(qt)
        return ops.dense_rows(x, q)

    @staticmethod
    def backward(ctx, g):
        (qt,) = ctx.saved_tensors
        return ops.dense_rows(g.contiguous(), qt), None, None


class SelectedLossFn(torch.autograd.Function):
    """(loss, count, sum) = matten_selected_loss(pred, target, selector, kind): the mean loss over the rows whose int32
    selector word is nonzero, with its adjoint kernel (matten_selected_loss_bwd).  Only ``pred`` receives a gradient;
    ``count`` (int64) and ``sum`` (fp64) carry none.  Nothing is read back: the upstream gradient and the count reach the
    adjoint as device words, so forward and backward capture into a hipGraph."""

    @staticmethod
    def forward(ctx, pred, target, selector, kind):
        loss, total, count = ops.selected_loss(pred, target, selector, kind)
        ctx.kind = kind
        ctx.save_for_backward(pred, target, selector, count)
        ctx.mark_non_differentiable(count, total)
        return loss, count, total

    @staticmethod
    def backward(ctx, g, _g_count, _g_sum):
        pred, target, selector, count = ctx.saved_tensors
        return ops.selected_loss_bwd(pred, target, selector, ctx.kind, g.contiguous(), count), None, None, None


class ValidLossFn(torch.autograd.Function):
    """(loss, sums, count) = matten_valid_loss(pred, target, n_valid, kind): the mean loss over the rows [0, *n_valid) of a
    padded crystal batch, with its adjoint kernel (matten_valid_loss_bwd).  ``n_valid`` is the device word
    ``batch["_amd_n_valid"][2:3]``.  Only ``pred`` receives a gradient; ``sums`` (fp64 [2]: squared, absolute -- what the
    mean-absolute-error metric adds) and ``count`` (int64) carry none.  Nothing is read back, so forward and backward
    capture into a hipGraph and a replay follows the refreshed word."""

    @staticmethod
    def forward(ctx, pred, target, n_valid, kind):
        loss, sums, count = ops.valid_loss(pred, target, n_valid, kind)
        ctx.kind = kind
        ctx.save_for_backward(pred, target, n_valid, count)
        ctx.mark_non_differentiable(sums, count)
        return loss, sums, count

    @staticmethod
    def backward(ctx, g, _g_sums, _g_count):
        pred, target, n_valid, count = ctx.saved_tensors
        return ops.valid_loss_bwd(pred, target, n_valid, ctx.kind, g.contiguous(), count), None, None, None


def needs_grad(*tensors: Optional[torch.Tensor]) -> bool:
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def params_of(module) -> tuple:
    """the module's parameters as a tuple, built once (module.parameters() walks the module tree: ~15 us per call for a
    conv layer, called several times per forward).  The Parameter objects are stable -- FlatAdam re-homes their storage,
    not the objects -- and their requires_grad flags are read live."""
    cached = module.__dict__.get("_amd_params")
    if cached is None:
        cached = tuple(module.parameters())
        module.__dict__["_amd_params"] = cached
    return cached


def needs_grad_lazy(tensors) -> bool:
    """needs_grad over the tuple ``tensors()`` returns, which is only built with autograd on (walking a module's
    parameters() a dozen times per forward is 0.1 ms of host time that an inference forward of a small batch feels)"""
    return torch.is_grad_enabled() and needs_grad(*tensors())
