"""
The register hand-over of the radial weights in the fused tensor-product forward (csrc/tp_walk.h, template parameter WR;
plan.TP_KIND_WREG): entries of the scalar and vector input blocks at 16 or 8 lanes per node have their weight columns
coupling-major, the matrix phase takes the chunk's edge rows as M and the weight columns as N, and a lane's D fragment is
the w[coupling][slot] it contracts -- nothing of w passes through LDS.

Every case runs ops.tp_fused twice in one process, on a plan built with MATTEN_TP_WREG=1 and on one built with
MATTEN_TP_WREG=0 (the [u][c] columns and the LDS tile), and compares both per output block with the fp64 reference of
tests/test_gpu_tp_forward.py under that file's tolerance rule, min(FWD_RTOL, R32_FACTOR x r32) of a block's maximum.  The
two outputs are expected to be bit-identical (the same three products summed over the same k by the same instruction, then
the same contraction in the same edge order) and are asserted so; the largest ulp distance is printed (WREG_ULP).

Graph: 70 nodes (one full 64-node tile and a partial one), in-degrees cycling through 0, 1, 2, 3, 4, 5, 7, 16, 17, 18, 33
(an empty segment, degrees that are no multiple of 2 or 4, more than one chunk at 2 and at 4 slots per chunk), random
sources, shuffled edge order.  Cases (name: what the plan makes of it, asserted in `_build`):
    scalar64     64x0e -> every degree: four 16-lane scalar entries in one shared workgroup with persistent node groups, five
                 tiles, the chunk-deep walk
    first        16x0e, the paper model's first layer: two 8-lane scalar entries in a paired workgroup, NC = 5 (the last tile
                 half empty)
    vector       16x1o+16x1e -> the paper model's layer irreps: the 8-lane kinds (1,0), (1,1), odd NC, the two-deep walk with
                 the pair contraction, the half-row exchange
    last         the paper model's last conv layer: the 16-lane vector kinds (1,2), (1,3) of the alternative coupling groups
    missing      a target without 2o / 1e / 0e: coupling masks that are no compile-time mask of their kind (run-time mask,
                 zero columns)
    vector_pair  8x1o: two 8-lane vector entries in a paired workgroup (the plain walk, one row in flight)
and the kernel's own split of the last layer (a_split=None) on `vector`.

Found with the `missing` case and fixed (tp_walk.h stage_safe_row): the stage rows of an EMPTY segment were read from the start
of the weight table; a weight's low half read as fp16 is inf or NaN one time in 32, the pair pass of the vector input blocks
contracts a slot past a segment's end with x = 0, and 0 x NaN left NaN in the seven rows nothing arrives at (LDS path and
register hand-over alike; it depended on the first four weights only).  Every case now plants fp16 NaN patterns in the low
halves of the first weight row, so the rows without in-edges ("exactly 0" in _check_blocks) test this deterministically.
"""
import copy

import numpy as np
import pytest
import torch

import test_gpu_tp_forward as fwd
from common import PAPER

pytestmark = pytest.mark.gpu

DEV = fwd.DEV
DEGREES = (0, 1, 2, 3, 4, 5, 7, 16, 17, 18, 33)
N_NODES = 70
CONV = PAPER["conv_layer_irreps"]
# name -> (input irreps, target irreps, {(l1, group, lanes per node)} that must carry the flag, workgroup modes of those)
CASES = {
    "scalar64": ("64x0e", "0e+1o+2e+3o+4e", {(0, 0, 16)}, {"shared"}),
    "first": ("16x0e", CONV, {(0, 0, 8)}, {"paired"}),
    "vector": ("16x1o+16x1e", CONV, {(1, 0, 8), (1, 1, 8)}, {"shared"}),
    "last": (CONV, "32x0e+4x2e+2x4e", {(0, 0, 16), (1, 2, 16), (1, 3, 16)}, {"shared"}),
    "missing": ("16x1o+16x1e", "0e+0o+1o+1e+2e+3o+3e+4e", {(1, 0, 8), (1, 1, 8)}, {"shared"}),
    "vector_pair": ("8x1o", CONV, {(1, 0, 8), (1, 1, 8)}, {"paired"}),
}
# masks the kernel knows at compile time (tp_walk.h HotMask) for the kinds above: `missing` must have others
HOT_MASKS = {(1, 0): {0x7F}, (1, 1): {0x1B, 0xF}}


def _graph(gen):
    deg = torch.tensor([DEGREES[n % len(DEGREES)] for n in range(N_NODES)])
    dst = torch.repeat_interleave(torch.arange(N_NODES), deg)
    src = torch.randint(N_NODES, (dst.numel(),), generator=gen)
    order = torch.randperm(dst.numel(), generator=gen)
    return torch.stack([src[order], dst[order]])


def _plan(name, wreg, monkeypatch):
    from matten_amd import plan as mplan

    monkeypatch.setenv("MATTEN_TP_WREG", "1" if wreg else "0")
    irreps_in, target, _, _ = CASES[name]
    p = mplan.plan_uvu(irreps_in, fwd._sh_irreps(4), target)
    monkeypatch.delenv("MATTEN_TP_WREG")
    return p


def _flagged(p):
    """-> ({(l1, group, lanes per node)} of the entries with TP_KIND_WREG, their workgroup modes, their (kind, mask) pairs)"""
    from matten_amd import plan as mplan

    ent = np.asarray(p.group_entries).reshape(-1, 32)
    kinds, modes, masks = set(), set(), set()
    for cu_log2, blk, mode in mplan.fused_workgroups(ent):
        for e in blk:
            k = int(ent[e][0])
            if k & mplan.TP_KIND_WREG:
                kind = ((k & 255) // mplan.TP_KIND_STRIDE, (k & 255) % mplan.TP_KIND_STRIDE)
                kinds.add(kind + (1 << cu_log2,))
                modes.add(mode)
                masks.add((kind, int(ent[e][4])))
    return kinds, modes, masks


class Case:
    pass


def _build(name, monkeypatch):
    from matten_amd import ops
    from matten_amd.nn._tables import DeviceTables
    from oracle.e3nn_lite.o3 import spherical_harmonics
    from oracle.matten_ref import nn as rnn

    irreps_in, target, want_kinds, want_modes = CASES[name]
    gen = torch.Generator().manual_seed(7000 + list(CASES).index(name))
    c = Case()
    c.name = name
    c.plans = {wreg: _plan(name, wreg, monkeypatch) for wreg in (True, False)}
    kinds, modes, masks = _flagged(c.plans[True])
    assert kinds == want_kinds and modes == want_modes, (name, kinds, modes)
    assert _flagged(c.plans[False])[0] == set(), "MATTEN_TP_WREG=0 must clear the flag"
    if name == "missing":
        assert all(m not in HOT_MASKS[k] for k, m in masks if k == (1, 0)) and any(m not in HOT_MASKS[k] for k, m in masks if k == (1, 1))
    p = c.plans[True]
    ref_mod = rnn.UVUTensorProduct(irreps_in, str(fwd._sh_irreps(4)), target, mlp_input_size=8, mlp_hidden_size=32,
                                   mlp_num_hidden_layers=2, mlp_activation=torch.nn.functional.silu)
    tp64, tp32 = copy.deepcopy(ref_mod.tp).double(), copy.deepcopy(ref_mod.tp).float()
    assert tp64.weight_numel == p.weight_numel and p.d_in == tp64.irreps_in1.dim

    edge_index = _graph(gen)
    N, E, W = N_NODES, edge_index.shape[1], p.weight_numel
    src, dst = edge_index
    in_deg = torch.bincount(dst, minlength=N)
    assert sorted(set(in_deg.tolist())) == sorted(DEGREES)
    c.N, c.rows_in = N, in_deg > 0
    x = torch.randn(N, p.d_in, generator=gen)
    vec = torch.randn(E, 3, generator=gen, dtype=torch.float64)
    Y = spherical_harmonics(list(range(5)), vec, True, "component").float()
    h2 = torch.randn(E, 32, generator=gen)
    W2 = torch.randn(32, W, generator=gen) / 32 ** 0.5
    # the low halves of the first row read as fp16 are NaN (fp32 values finite and used as they are by the references): what a
    # stage loader fetches for the rows of an empty segment must not be weights -- 0 x NaN in the pair pass of the vector blocks
    W2[0] = ((W2[0].view(torch.int32) & -65536) | 0x7E00).view(torch.float32)
    nrm = torch.full((N,), fwd.AVG ** -0.5, dtype=torch.float64)

    perm, c.rowptr, c.src, err = ops.csr_build(edge_index.to(DEV), N)
    assert int(err.item()) == 0
    perm = perm.long().cpu()
    c.x = x.to(DEV)
    Yd = torch.full((E, fwd.SH_STRIDE), float("nan"))
    Yd[:, : p.sh_dim] = Y
    c.Y = Yd[perm].to(DEV)
    c.h2p = ops.split_hidden(h2[perm][:, fwd.FEAT].contiguous().to(DEV))
    c.ops = {}
    for wreg, q in c.plans.items():
        assert q.weight_numel == W and q.d_mid == p.d_mid and len(q.fused_cols) == len(p.fused_cols)
        assert np.array_equal(np.asarray(q.group_entries)[:, 1:], np.asarray(p.group_entries)[:, 1:]), "only the flag differs"
        cols = torch.as_tensor(q.fused_cols)
        assert sorted(cols[cols >= 0].tolist()) == sorted(torch.as_tensor(p.fused_cols)[torch.as_tensor(p.fused_cols) >= 0].tolist())
        w2f = torch.where(cols[None, :] >= 0, W2[:, cols.clamp(min=0)], W2.new_zeros(()))
        w2f = torch.nn.functional.pad(w2f, (0, (-w2f.shape[1]) % 16 + 16)).contiguous().to(DEV)
        t = DeviceTables(gentries=q.group_entries, gumap=q.fused_unit_map)
        c.ops[wreg] = (q, t, w2f, ops.split_a_tiles(w2f, q.group_entries))

    pieces = c.h2p.float().cpu().double()
    h2_eff = torch.empty(E, 32, dtype=torch.float64)
    h2_eff[:, fwd.FEAT] = pieces[:, 0] + pieces[:, 1] / 2048.0
    h2_orig = torch.empty_like(h2_eff)
    h2_orig[perm] = h2_eff
    w64 = h2_orig @ W2.double()
    c.ref = fwd._reference(tp64, x.double(), Y.double(), w64, edge_index, N, nrm)
    ref32 = fwd._reference(tp32, x, Y, h2_orig.float() @ W2, edge_index, N, nrm.float()).double()
    c.blocks = [(f"{q.l1},{q.l2},{q.l3}", slice(q.out_off, q.out_off + q.mul * (2 * q.l3 + 1))) for q in p.paths]
    c.r32 = max(fwd._ratio((ref32[c.rows_in][:, sl] - c.ref[c.rows_in][:, sl]).abs().max().item(),
                           c.ref[c.rows_in][:, sl].abs().max().item()) for _, sl in c.blocks)
    assert 0 < c.r32 < 1e-5, c.r32
    c.rtol = min(fwd.FWD_RTOL, fwd.R32_FACTOR * c.r32)
    c.p = p
    return c


@pytest.fixture(scope="module")
def built():
    cache = {}
    yield cache
    cache.clear()
    torch.cuda.synchronize()


def _case(name, built, monkeypatch):
    if name not in built:
        built[name] = _build(name, monkeypatch)
    return built[name]


def _fused(c, wreg, a_split="host"):
    from matten_amd import ops

    q, t, w2f, frags = c.ops[wreg]
    um = t.get("gumap", DEV)
    fwd._nan_prefill(c.N, q.d_mid)
    return ops.tp_fused(c.x, c.h2p, w2f, c.Y, c.rowptr, c.src, t.get("gentries", DEV), um, um.numel(),
                        q.fused_lds_floats_per_wave, q.d_mid, fwd.AVG, None, a_split=frags if a_split == "host" else None)


def _ulp(a, b):
    """largest distance in units of the last place between two fp32 tensors of equal sign pattern (else a large number)"""
    ia, ib = a.contiguous().view(torch.int32).long(), b.contiguous().view(torch.int32).long()
    ia, ib = torch.where(ia < 0, -(ia & 0x7FFFFFFF), ia), torch.where(ib < 0, -(ib & 0x7FFFFFFF), ib)
    return int((ia - ib).abs().max().item())


def _both(c, monkeypatch, a_split="host"):
    out = {}
    for wreg in (True, False):
        monkeypatch.setenv("MATTEN_TP_WREG", "1" if wreg else "0")   # (ops.tp_fused checks the library against the setting)
        out[wreg] = _fused(c, wreg, a_split)
        monkeypatch.delenv("MATTEN_TP_WREG")
    for wreg, agg in out.items():
        r, label = fwd._check_blocks(c, agg, f"{c.name} MATTEN_TP_WREG={int(wreg)}", c.rtol)
        print(f"\nWREG_RATIO {c.name} wreg={int(wreg)} {r:.3g} {label}   (r32 {c.r32:.3g}, allowed {c.rtol:.3g} of a block's maximum)")
    ulp = _ulp(out[True], out[False])
    print(f"WREG_ULP {c.name} {ulp}")
    assert torch.equal(out[True], out[False]), f"{c.name}: register hand-over vs LDS tile differ by up to {ulp} ulp"
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_register_handover_matches_fp64_and_the_lds_path(name, built, monkeypatch):
    _both(_case(name, built, monkeypatch), monkeypatch)


def test_in_kernel_split(built, monkeypatch):
    """a_split = None: every wave splits its own weight columns -- the column order is the plan's, not the kernel's"""
    c = _case("vector", built, monkeypatch)
    out = _both(c, monkeypatch, a_split=None)
    assert torch.equal(out[True], _fused(c, True)), "the kernel's own split of w2f"
