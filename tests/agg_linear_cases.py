"""Single-layer cases for the streaming lin2 (matten_agg_linear / matten_agg_linear_gate): planned with no model and no
GPU, shared by test_agg_linear_host.py (numpy emulation of the kernel's walk) and test_gpu_agg_linear.py (the kernel).

Per case: the fp64 reference (the oracle's FullyConnectedTensorProduct on the reference-layout neighbour sums, then the
oracle's Gate and eval-mode BatchNorm for the gated cases), the component-major row the kernel reads -- every float no
group entry writes is NaN -- and the A-fragment table built the way PointConv._pack_agg_weights builds it."""
import functools
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np
import torch

from matten_amd import plan as mplan

SH4 = "0e+1o+2e+3o+4e"
ACT_SCALARS, ACT_GATES = {1: "silu", -1: "tanh"}, {1: "sigmoid", -1: "tanh"}

# id -> (irreps_in1, irreps_out of lin2, spherical harmonics): the smallest layouts that reach each branch of the kernel
CASES = {
    "paper_like": ("32x0e+16x1o+4x2e", "32x0e+16x1o+16x1e+4x2e+4x2o+2x3o+2x3e+2x4e", SH4),  # T 2, 4, 5; n_mt 2; kk 2 + 1; cw 2, 4
    "wide_scalars": ("64x0e+32x1o", "80x0e+16x1o", SH4),             # one irrep in three table rows (32, 32, 16); T 6, 8
    "mo17": ("16x0e+8x1o", "17x0e+17x1o+5x2e", SH4),                 # second tile holds one channel; kk = 1 rows; cw 5
    "mo33": ("32x0e", "33x0e+32x1o", SH4),                           # a table row with mo = 1 behind a full one
    "mo12_d3": ("8x0e+4x1o+2x2e", "12x0e+12x1o+7x2e+3x4e", SH4),     # cw 12, 7, 3; K 14, 20, 22: pad slots in the last chunk
    "K_small": ("2x0e", "31x0e+11x1o+7x2e", "0e+1o+2e"),             # K = 2: 14 of 16 slots of every chunk masked
    "K_big": ("128x0e+64x1o+32x2e", "16x0e+8x1o+8x2e+4x3o+4x4e", SH4),   # T 14..22: five to six blocks per unit
    "odd": ("8x0e+8x0o+4x1o+4x1e", "8x0e+8x0o+8x1o+8x1e+2x2e+2x2o", SH4),   # both parities of every degree
    "tiny": ("1x0e", "1x0e+1x1o", "0e+1o"),                          # one channel, one slot per chunk
    "lds_79k": ("128x0e+64x1o+32x2e", "32x0e+8x1o+8x2e+4x3o+4x4e", SH4),    # 78 944 bytes of LDS: above the 64 KB default
}
LDS_79K_BYTES = 78944
LDS_OVER = ("128x0e+64x1o+32x2e", "48x0e+8x1o+8x2e+4x3o+4x4e", SH4)   # 93 376 bytes: above the kernel's 80 KB cap
LDS_OVER_BYTES = 93376

# id -> (irreps_in1, target of the activation layer, spherical harmonics); lin2 then produces plan_gate(...).irreps_in
GATED = {
    "paper_like": CASES["paper_like"],                                # 46 gates in sets 0, 1
    "gates_65": ("16x0e+8x1o", "8x0e+32x1o+33x2e", SH4),              # all three register sets
    "gates_33": ("16x0e+8x1o", "8x0e+20x1o+13x2e", SH4),              # 8 scalars + 24 gates in one table row, 9 gates in the next
    "gates_25": ("16x0e+8x1o", "8x0e+20x1o+5x2e", SH4),               # ... and 1: a set holding one gate (a table row with mo = 1)
    "odd_scalars": ("8x0e+8x0o+4x1o+4x1e", "8x0e+8x0o+8x1o+8x1e+2x2e", SH4),   # tanh scalars (0o), sigmoid gates
    "no_scalars": ("4x0e+4x1o", "6x1o+3x2e", SH4),                    # no type-1 column at all
    "scalars_only": ("16x0e+8x1o", "40x0e", SH4),                     # no gate at all
    "tiny": ("1x0e", "1x0e+1x1o", "0e+1o"),                           # one gate
}
REFUSED_GATE = ("16x0e+8x1o", "8x0e+64x1o+33x2e", SH4)   # 97 gates exceed 3 sets of 32: plan_agg_gate -> None
REFUSED_AGG = ("3x0e+3x1o", "4x0e+4x1o", SH4)            # alignment holes: plan_agg_linear -> None

# rows per species; the row order is shuffled so that `order` is not the identity
ROW_PATTERNS = {
    "ragged": (0, 1, 15, 16, 17, 0),        # empty first and last species; groups below, at and above one wave
    "blocks": (127, 128, 129, 0, 257),      # groups below, at and above one and two workgroups
}


@dataclass
class Layer:
    name: str
    S: int
    uvu: "mplan.UVUPlan"
    ap: Optional["mplan.AggLinearPlan"]
    irreps_out: object                 # lin2's output irreps (the Gate's input irreps for a gated case)
    gate: Optional["mplan.GatePlan"]
    cmeta: Optional[np.ndarray]


def irrep_blocks(irreps) -> List[Tuple[int, int, str]]:
    """(lo, hi, name) per irrep of a row"""
    out, off = [], 0
    for mul, ir in irreps:
        out.append((off, off + mul * ir.dim, f"{mul}x{ir}"))
        off += mul * ir.dim
    return out


def plan_case(in1, out, sh, S, gated=False, name="") -> Layer:
    gate = None
    if gated:
        gate = mplan.plan_gate(in1, sh, out, ACT_SCALARS, ACT_GATES)
        out = gate.irreps_in
    uvu = mplan.plan_uvu(in1, sh, out)
    irreps_out = mplan.Irreps(out).simplify()
    ap = mplan.plan_agg_linear(uvu, S, irreps_out)
    cmeta = mplan.plan_agg_gate(ap, gate) if gated and ap is not None else None
    return Layer(name, S, uvu, ap, irreps_out, gate, cmeta)


@functools.lru_cache(maxsize=None)
def layer(name: str, S: int, gated: bool = False) -> Layer:
    lay = plan_case(*(GATED if gated else CASES)[name], S, gated, name)
    assert lay.ap is not None and (not gated or lay.cmeta is not None), name
    return lay


def species_rows(counts, seed=0) -> np.ndarray:
    """species index per row for `counts` rows per species, shuffled"""
    sp = np.repeat(np.arange(len(counts)), counts)
    return np.random.default_rng(seed).permutation(sp)


def order_seg(species, S, reverse=False):
    """(order[N], seg[S + 1]) int32 as the embedding builds them: rows sorted by species (stable); reverse: the rows of
    every species in descending order instead"""
    species = np.asarray(species)
    order = np.argsort(species, kind="stable")
    seg = np.concatenate([[0], np.cumsum(np.bincount(species, minlength=S))])
    if reverse:
        order = np.concatenate([order[seg[s]:seg[s + 1]][::-1] for s in range(S)]) if len(order) else order
    return order.astype(np.int32), seg.astype(np.int32)


def make_inputs(lay: Layer, species, seed=0):
    """(agg[N, d_mid] in the reference layout, flat lin2 weight): fp32 values, so that every precision reads the same"""
    rng = np.random.default_rng(seed)
    agg = rng.standard_normal((len(species), lay.uvu.d_mid)).astype(np.float32)
    w = rng.standard_normal(weight_numel(lay)).astype(np.float32)
    return agg, w


def weight_numel(lay: Layer) -> int:
    mid = lay.uvu.irreps_out
    return sum(mi * lay.S * mo for mi, ir in mid for mo, iro in lay.irreps_out if iro == ir)


def scatter_rows(lay: Layer, agg: np.ndarray):
    """what matten_tp_fused's epilogue does with the plan's entries: channel u, component k of coupling c of a group entry
    lands at out_off[c] + u + k * t_off[c].  -> (row[N, ld], writes per float of the row); every float no entry writes is
    NaN: the pad slots past a region's K and the tail between 16 * n_chunks and ld"""
    uvu, ap = lay.uvu, lay.ap
    row = np.full((agg.shape[0], ap.ld), np.nan, dtype=agg.dtype)
    written = np.zeros(ap.ld, dtype=np.int64)
    ent = ap.entries
    for e in range(len(ent)):
        mul = int(uvu.group_entry_mul[e])    # channels of the record's OWN block (merged entries: 2 + 2 over two records)
        u = np.arange(mul)
        for c, pi in uvu.group_entry_paths[e].items():
            pth = uvu.paths[pi]
            d3 = 2 * pth.l3 + 1
            o, ks = int(ent[e][20 + c]), int(ent[e][8 + c])
            for k in range(d3):
                row[:, o + u + k * ks] = agg[:, pth.out_off + (uvu.group_entry_u0[e] + u) * d3 + k]
                np.add.at(written, o + u + k * ks, 1)
    return row, written


def make_wtab(ap, w: np.ndarray) -> np.ndarray:
    """[S, w_stride] fp32 A fragments, as PointConv._pack_agg_weights: gathered from the flat weight, scaled in fp32"""
    w = np.asarray(w, dtype=np.float32)
    return np.where(ap.gather >= 0, w[np.clip(ap.gather, 0, None)] * ap.scale[None, :].astype(np.float32),
                    np.float32(0)).astype(np.float32)


def unpack_io(r):
    c0, T, K, packed, a_off, out_off, mo, k0 = (int(x) for x in r)
    return dict(c0=c0, T=T, K=K, d3=packed & 255, n_mt=(packed >> 8) & 255, cw=(packed >> 16) & 255,
                kk=(packed >> 24) & 255, a_off=a_off, out_off=out_off, mo=mo, k0=k0)


def emulate(ap, row: np.ndarray, wtab: np.ndarray, species: np.ndarray, add=None):
    """matten_agg_linear in numpy (fp64 sums): the block list is walked in order, every chunk multiplied with the A
    fragments [t][mt][g][c][s], slots >= K selected away, a unit parked in the table row's stage when its last block
    closes and the stage written out (+ addend) when the table row's last unit closes.  Asserts the tables' invariants
    on the way and that no slot read as data is NaN.  -> (out[N, d_out], stores per output column)"""
    N = row.shape[0]
    out = np.full((N, ap.d_out), np.nan)
    stores = np.zeros(ap.d_out, dtype=np.int64)
    wsp = wtab.astype(np.float64)[species]                     # [N, w_stride]
    j16 = np.arange(16)
    g_, s_ = j16 // 4, j16 % 4                                 # float j of a chunk = slot 4 g + s of its matrix steps
    acc = stage = None
    blocks = ap.blocks.tolist()
    for j, (chunk, info, t0, _) in enumerate(blocks):
        n, first, last, last_row = info & 255, (info >> 8) & 1, (info >> 9) & 1, (info >> 10) & 1
        k, ii = (info >> 12) & 255, (info >> 20) & 4095
        r = unpack_io(ap.io_table[ii])
        T, K, d3, n_mt, cw, kk, mo, k0 = r["T"], r["K"], r["d3"], r["n_mt"], r["cw"], r["kk"], r["mo"], r["k0"]
        assert mo * kk <= mplan.AGG_STAGE_W and 1 <= n_mt <= mplan.AGG_MAX_MT and 1 <= n <= mplan.AGG_BLOCK
        assert k0 <= k < k0 + kk <= d3   # the row's component range (a wide irrep is cut by component: no chunk read twice)
        assert chunk == r["c0"] + k * T + t0 and t0 + n <= T and 16 * (T - 1) < K <= 16 * T
        assert cw == min(mo, 16) and n_mt == -(-mo // 16) and 16 * (chunk + n) <= ap.ld
        assert first == (t0 == 0) and last == (t0 + n == T) and last_row == (last and k == k0 + kk - 1)
        if first:
            assert acc is None
            acc = np.zeros((N, mo))
        if stage is None:
            stage = np.full((N, mo * kk), np.nan)
        mt_, c_ = np.meshgrid(np.arange(n_mt), np.arange(cw), indexing="ij")
        v = (16 * mt_ + c_).reshape(-1)
        keep = v < mo
        for i in range(n):
            t = t0 + i
            ok = 16 * t + j16 < K                                              # masked by the kernel (select, not multiply)
            b = row[:, 16 * (chunk + i) + j16[ok]].astype(np.float64)
            assert not np.isnan(b).any(), ("a pad slot is read as data", ii, k, t)
            # A[t][mt][g][c][s] for the kept slots x (mt, c)
            a_idx = r["a_off"] + ((((t * n_mt + mt_.reshape(-1)[None, :]) * 4 + g_[ok][:, None]) * cw
                                   + c_.reshape(-1)[None, :]) * 4 + s_[ok][:, None])
            assert a_idx.max() < ap.w_stride
            acc[:, v[keep]] += np.einsum("nj,njv->nv", b, wsp[:, a_idx[:, keep]])
        if last:
            stage[:, np.arange(mo) * kk + (k - k0)] = acc
            acc = None
            if last_row:
                assert not np.isnan(stage).any()
                pos = np.arange(mo * kk)
                col = r["out_off"] + (pos // kk) * d3 + k0 + pos % kk
                out[:, col] = stage + (0.0 if add is None else add[:, col])
                stores[col] += 1
                stage = None
        else:
            assert j + 1 < len(blocks)
    assert acc is None and stage is None
    return out, stores


def emulate_gate(lay: Layer, conv_out: np.ndarray, bn_scale=None, bn_shift=None) -> np.ndarray:
    """the Gate epilogue of matten_agg_linear_gate from cmeta, table row by table row: a gate scalar must have been parked
    (register set, lane) by an EARLIER table row than the first one that fetches it"""
    from matten_amd.nn._activation import act_const_table

    funcs = {0: lambda x: x, 1: lambda x: x / (1 + np.exp(-x)), 2: np.tanh, 3: lambda x: 1 / (1 + np.exp(-x))}
    cst = act_const_table().numpy().astype(np.float64)
    cm, ap = lay.cmeta, lay.ap
    N = conv_out.shape[0]
    out = np.full((N, lay.gate.irreps_out.dim), np.nan)
    stores = np.zeros(out.shape[1], dtype=np.int64)
    regs = {}
    for row in ap.io_table:
        r = unpack_io(row)
        pos = np.arange(r["mo"] * r["kk"])
        cols = r["out_off"] + (pos // r["kk"]) * r["d3"] + r["k0"] + pos % r["kk"]
        parked = {}
        for p, col in zip(pos, cols):
            typ, code = int(cm[col][0]) & 255, (int(cm[col][0]) >> 8) & 255
            y, lane, st = (int(x) for x in cm[col][1:])
            v = conv_out[:, col]
            if typ == 2:
                assert lane == p and 0 <= st < mplan.AGG_GATE_SETS and lane < 32
                parked[(st, lane)] = funcs[code](v) * cst[code]
                continue
            assert typ in (1, 3), (col, typ)
            res = funcs[code](v) * cst[code] if typ == 1 else v * regs[(st, lane)]
            if bn_scale is not None:
                res = res * bn_scale[y] + bn_shift[y]
            out[:, y] = res
            stores[y] += 1
        regs.update(parked)     # (the lanes of one table row exchange before any of them parks)
    assert (stores == 1).all()
    return out


# ---- references -------------------------------------------------------------------------------------------------------
def reference_lin2(lay: Layer, agg, species, w, dtype=torch.float64) -> torch.Tensor:
    """the oracle's FullyConnectedTensorProduct(irreps_mid, Sx0e, irreps_out) with the same flat weight"""
    from oracle.e3nn_lite import o3 as ro3

    ref = ro3.FullyConnectedTensorProduct(str(lay.uvu.irreps_out), f"{lay.S}x0e", str(lay.irreps_out)).to(dtype)
    with torch.no_grad():
        assert ref.weight.numel() == len(w)
        ref.weight.copy_(torch.as_tensor(w).to(dtype))
        one_hot = torch.nn.functional.one_hot(torch.as_tensor(np.asarray(species)).long(), lay.S).to(dtype)
        return ref(torch.as_tensor(agg).to(dtype), one_hot)


@functools.lru_cache(maxsize=None)
def _activation_layer(name: str):
    from oracle.matten_ref.nn import ActivationLayer

    in1, target, sh = GATED[name]
    return ActivationLayer(in1, sh, target, activation_type="gate", activation_scalars={"e": "silu", "o": "tanh"},
                           activation_gates={"e": "sigmoid", "o": "tanh"})


def oracle_gate(lay: Layer):
    """the oracle's Gate for the case, built as oracle.matten_ref.nn.ActivationLayer builds it (a fresh copy: .double()
    converts a module in place)"""
    import copy

    act = copy.deepcopy(_activation_layer(lay.name))
    assert str(act.irreps_in) == str(lay.gate.irreps_in) and str(act.irreps_out) == str(lay.gate.irreps_out)
    return act


def oracle_batchnorm(lay: Layer, seed=0):
    """the oracle's BatchNorm over the activated row in eval mode, running statistics and affine parameters randomised"""
    from oracle.e3nn_lite.nn import BatchNorm

    bn = BatchNorm(str(lay.gate.irreps_out)).eval()
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        bn.running_mean.copy_(0.1 * torch.randn(bn.running_mean.shape, generator=g))
        bn.running_var.copy_(0.5 + torch.rand(bn.running_var.shape, generator=g))
        bn.weight.copy_(0.5 + torch.rand(bn.weight.shape, generator=g))
        bn.bias.copy_(0.1 * torch.randn(bn.bias.shape, generator=g))
    return bn


def fold_batchnorm(lay: Layer, bn):
    """eval-mode BatchNorm as per-column (scale, shift) of the activated row, from the oracle BatchNorm's own buffers:
    column o belongs to channel meta[o, 3] & 0xFFFF; 0e columns also carry the index of their mean / bias"""
    meta = torch.as_tensor(np.asarray(lay.gate.meta).reshape(-1, 4)[:, 3].astype(np.int64))
    bn_idx, mean_idx = meta & 0xFFFF, (meta >> 16) & 0xFFFF
    scale = (bn.weight.detach() / torch.sqrt(bn.running_var + bn.eps))[bn_idx]
    has_mean = mean_idx != 0xFFFF
    shift = torch.zeros_like(scale)                # (a row without 0e channels has no mean and no bias at all)
    mi = mean_idx[has_mean]
    shift[has_mean] = bn.bias.detach()[mi] - bn.running_mean[mi] * scale[has_mean]
    return scale.float().contiguous(), shift.float().contiguous()


def reference_gated(lay: Layer, agg, species, w, add=None, bn=None, dtype=torch.float64) -> torch.Tensor:
    """lin2 (+ the self-connection) -> Gate (-> BatchNorm), all in `dtype`"""
    import copy

    x = reference_lin2(lay, agg, species, w, dtype)
    if add is not None:
        x = x + torch.as_tensor(add).to(dtype)
    with torch.no_grad():
        x = oracle_gate(lay).to(dtype)(x)
        if bn is not None:
            x = copy.deepcopy(bn).to(dtype)(x)
    return x


def block_errors(got, want64, want32, species, blocks, rtol=2e-6):
    """per output block and per species: (max |got - fp64|, allowed) with allowed = max(rtol x the block's maximum over
    the species' rows, 4 x the fp32 oracle's own distance from the fp64 one there) -- the want64 rule of close_blocks"""
    got, want64, want32 = (np.asarray(t, dtype=np.float64) for t in (got, want64, want32))
    assert got.shape == want64.shape == want32.shape, (got.shape, want64.shape, want32.shape)
    assert blocks[-1][1] == want64.shape[1]
    res = {}
    for s in np.unique(species):
        rows = np.nonzero(np.asarray(species) == s)[0]
        for lo, hi, name in blocks:
            ref = want64[rows, lo:hi]
            scale = np.abs(ref).max()
            assert scale > 0, f"block {name} species {s}: empty reference block"
            d32 = np.abs(want32[rows, lo:hi] - ref).max()
            res[(name, int(s))] = (np.abs(got[rows, lo:hi] - ref).max(), max(rtol * scale, 4.0 * d32), scale)
    return res
