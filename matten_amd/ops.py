"""
Thin tensor-level wrappers over the C ABI (include/matten_hip.h).

PyTorch is plumbing here: it owns device memory and the HIP stream; all arithmetic happens in
libmatten_hip.so.  Every wrapper insists on contiguous CUDA(=HIP) tensors of the right dtype and
raises if handed anything else -- there is deliberately no CPU path.
"""
from __future__ import annotations

from typing import Optional, Tuple

import os

import numpy as np

import torch

from . import _lib
from .nn._tables import bump_weights_epoch


# ---- optional HIP-event timing of individual launches (used by bench.py for the roofline line) ----
_EVENTS = None  # name -> list of (start_event, end_event) recorded on the launch stream
_EVENTS_ONLY = None  # name prefixes to time, or None: every timed launch


def enable_event_timing(flag: bool = True, only=None) -> None:
    """only: time just the launches whose name starts with one of these prefixes (an event pair costs a few us of queue
    time per launch: a benchmark that needs one kernel's duration should not pay for nine)"""
    global _EVENTS, _EVENTS_ONLY
    _EVENTS = {} if flag else None
    _EVENTS_ONLY = tuple(only) if (flag and only) else None


def event_timings_ms():
    """name -> list of elapsed milliseconds (call after torch.cuda.synchronize())."""
    if _EVENTS is None:
        return {}
    return {k: [a.elapsed_time(b) for a, b in v] for k, v in _EVENTS.items()}


class _timed:
    def __init__(self, name: str):
        self.name = name

    def __enter__(self):
        self.on = _EVENTS is not None and (_EVENTS_ONLY is None or self.name.startswith(_EVENTS_ONLY))
        if self.on:
            self.a = torch.cuda.Event(enable_timing=True)
            self.a.record(torch.cuda.current_stream())
        return self

    def __exit__(self, *exc):
        if self.on and _EVENTS is not None:
            b = torch.cuda.Event(enable_timing=True)
            b.record(torch.cuda.current_stream())
            _EVENTS.setdefault(self.name, []).append((self.a, b))
        return False


SH_STRIDE = 32  # floats per row of sh_sorted


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream() -> int:
    """the current HIP stream of the current device as a raw handle (the private getter skips the Stream object that
    torch.cuda.current_stream() builds: ~4 us per launch, 40+ launches per forward)"""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def _need(t: torch.Tensor, dtype, name: str) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name}: expected a tensor, got {type(t)}")
    if not t.is_cuda:
        raise _lib.MattenHipError(
            f"{name} is on {t.device}: matten_amd runs on MI355X only (no CPU fallback). Move the batch to cuda."
        )
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    return t if t.is_contiguous() else t.contiguous()


def _need_rows(t: torch.Tensor, dtype, name: str) -> torch.Tensor:
    """like _need, but a column slice of a wider row-major matrix (unit column stride) is passed through as is: the
    kernels that take it address rows by the tensor's own row stride"""
    if isinstance(t, torch.Tensor) and t.dim() == 2 and t.stride(1) == 1 and t.stride(0) >= t.shape[1] and t.is_cuda \
            and t.dtype == dtype:
        return t
    return _need(t, dtype, name)


def _err_flag(err, dev) -> torch.Tensor:
    """a zeroed int32[1] flag word, or the caller's (one allocation + one memset for several kernels' flags)"""
    if err is None:
        return torch.zeros(1, dtype=torch.int32, device=dev)
    if err.dtype != torch.int32 or err.numel() != 1 or err.device != dev:
        raise ValueError("err must be an int32 tensor of one element on the inputs' device")
    return err


def csr_build(edge_index: torch.Tensor, n_nodes: int, err: torch.Tensor = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """-> (perm[E] i32, rowptr[N+1] i32, src_sorted[E] i32, err_flag[1] i32)"""
    lib = _lib.load()
    edge_index = _need(edge_index, torch.int64, "edge_index")
    E = edge_index.shape[1]
    dev = edge_index.device
    perm = torch.empty(E, dtype=torch.int32, device=dev)
    rowptr = torch.empty(n_nodes + 1, dtype=torch.int32, device=dev)
    src = torch.empty(E, dtype=torch.int32, device=dev)
    err = _err_flag(err, dev)
    nbytes = lib.matten_csr_workspace_bytes(E, n_nodes)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    _lib.check(
        lib.matten_csr_build(_ptr(edge_index), E, n_nodes, _ptr(perm), _ptr(rowptr), _ptr(src), _ptr(ws), nbytes,
                             _ptr(err), _stream()),
        "matten_csr_build",
    )
    return perm, rowptr, src, err


def csr_split(rowptr: torch.Tensor, n_edges: int, max_len: int, num_neigh: torch.Tensor = None):
    """-> (vrowptr[bound+1] i32, vseg[N+1] i64, vnn[bound] f32 or None): every CSR segment cut into virtual nodes of at
    most max_len edges (include/matten_hip.h matten_csr_split); bound = N + E // max_len, no host sync"""
    lib = _lib.load()
    rowptr = _need(rowptr, torch.int32, "rowptr")
    N = rowptr.shape[0] - 1
    bound = int(lib.matten_csr_split_bound(N, n_edges, max_len))
    dev = rowptr.device
    vrowptr = torch.empty(bound + 1, dtype=torch.int32, device=dev)
    vseg = torch.empty(N + 1, dtype=torch.int64, device=dev)
    vnn = None
    if num_neigh is not None:
        num_neigh = _need(num_neigh, torch.float32, "num_neigh")
        vnn = torch.empty(bound, dtype=torch.float32, device=dev)
    _lib.check(lib.matten_csr_split(_ptr(rowptr), N, n_edges, max_len, _ptr(vrowptr), _ptr(vseg), _ptr(num_neigh), _ptr(vnn),
                                    _stream()), "matten_csr_split")
    return vrowptr, vseg, vnn


def group_by_key(key: torch.Tensor, n_keys: int, err: torch.Tensor = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """-> (order[n] i32: positions stably sorted by key, seg[n_keys+1] i32, err_flag[1] i32)"""
    lib = _lib.load()
    key = _need(key, torch.int64, "key")
    n = key.shape[0]
    dev = key.device
    order = torch.empty(n, dtype=torch.int32, device=dev)
    seg = torch.empty(n_keys + 1, dtype=torch.int32, device=dev)
    err = _err_flag(err, dev)
    nbytes = lib.matten_group_workspace_bytes(n, n_keys)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    _lib.check(lib.matten_group_by_key(_ptr(key), n, n_keys, _ptr(order), _ptr(seg), _ptr(ws), nbytes, _ptr(err),
                                       _stream()), "matten_group_by_key")
    return order, seg, err


def species_embed(atomic_numbers, z_to_index, min_z: int, max_z: int, n_species: int, weight, bias,
                  want_attrs: bool = False, err: torch.Tensor = None):
    """-> (species_index i64 [N], species_i32 [N], node_feats [N,dim], node_attrs [N,S] | None, err_flag)"""
    lib = _lib.load()
    Z = _need(atomic_numbers, torch.int64, "atomic_numbers")
    lut = _need(z_to_index, torch.int64, "_Z_to_index")
    W = _need(weight, torch.float32, "linear.weight")
    b = _need(bias, torch.float32, "linear.bias")
    N, dim = Z.shape[0], W.shape[0]
    dev = Z.device
    sidx = torch.empty(N, dtype=torch.int64, device=dev)
    s32 = torch.empty(N, dtype=torch.int32, device=dev)
    feats = torch.empty(N, dim, dtype=torch.float32, device=dev)
    attrs = torch.empty(N, n_species, dtype=torch.float32, device=dev) if want_attrs else None
    err = _err_flag(err, dev)
    _lib.check(
        lib.matten_species_embed(_ptr(Z), N, _ptr(lut), min_z, max_z, n_species, _ptr(W), _ptr(b), dim, _ptr(sidx),
                                 _ptr(s32), _ptr(feats), _ptr(attrs), _ptr(err), _stream()),
        "matten_species_embed",
    )
    return sidx, s32, feats, attrs, err


def edge_geom(pos, edge_index, edge_cell_shift, cell, batch, perm, lmax: int, n_basis: int = 0, r_start: float = 0.0,
              r_end: float = 1.0, want_vectors=False, want_lengths=False, want_attrs=False, want_embedding=False):
    """-> dict(geom_sorted [E,4], sh_sorted [E,(lmax+1)^2], + requested original-order tensors)"""
    lib = _lib.load()
    pos = _need(pos, torch.float32, "pos")
    edge_index = _need(edge_index, torch.int64, "edge_index")
    E = edge_index.shape[1]
    dev = pos.device
    n_cells = 0
    if cell is not None:
        cell = _need(cell, torch.float32, "cell").reshape(-1, 3, 3)
        n_cells = cell.shape[0]
        edge_cell_shift = _need(edge_cell_shift, torch.float32, "edge_cell_shift")
        if n_cells > 1:
            batch = _need(batch, torch.int64, "batch")
    sh_dim = (lmax + 1) ** 2
    geom = torch.empty(E, 4, dtype=torch.float32, device=dev)
    # rows padded to 32 floats: one 128-byte line per edge, and the fused TP kernel may read any l2 <= 4
    # (the kernel writes the padding columns as zeros itself)
    sh = torch.empty(E, SH_STRIDE, dtype=torch.float32, device=dev)
    out = {"geom_sorted": geom, "sh_sorted": sh}
    ev = torch.empty(E, 3, dtype=torch.float32, device=dev) if want_vectors else None
    el = torch.empty(E, dtype=torch.float32, device=dev) if want_lengths else None
    ea = torch.empty(E, sh_dim, dtype=torch.float32, device=dev) if want_attrs else None
    ee = torch.empty(E, n_basis, dtype=torch.float32, device=dev) if want_embedding else None
    _lib.check(
        lib.matten_edge_geom(_ptr(pos), _ptr(edge_index), _ptr(edge_cell_shift), _ptr(cell), n_cells, _ptr(batch),
                             _ptr(perm), E, pos.shape[0], lmax, n_basis, r_start, r_end, _ptr(geom), _ptr(sh), SH_STRIDE, _ptr(ev),
                             _ptr(el),
                             _ptr(ea), _ptr(ee), _stream()),
        "matten_edge_geom",
    )
    out.update(edge_vectors=ev, edge_lengths=el, edge_attrs=ea, edge_embedding=ee)
    return out


def _edge_dtype(t: torch.Tensor, name: str) -> torch.Tensor:
    """per-edge training tensors (radial weights, their gradient): fp32 or, opt-in, bf16 storage"""
    if not isinstance(t, torch.Tensor) or t.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"{name}: expected an fp32 or bf16 tensor")
    return _need(t, t.dtype, name)


def radial_mlp(geom_sorted, n_basis: int, r_start: float, r_end: float, w0p, w1p, w2p, out_dtype=torch.float32) -> torch.Tensor:
    lib = _lib.load()
    geom_sorted = _need(geom_sorted, torch.float32, "geom_sorted")
    w0p, w1p, w2p = (_need(w, torch.float32, n) for w, n in ((w0p, "w0p"), (w1p, "w1p"), (w2p, "w2p")))
    E = geom_sorted.shape[0]
    nb_pad, hidden = w0p.shape
    w_pad = w2p.shape[1]
    if out_dtype not in (torch.float32, torch.bfloat16):
        raise TypeError("radial_mlp: out_dtype must be fp32 or bf16")
    out = torch.empty(E, w_pad, dtype=out_dtype, device=geom_sorted.device)
    with _timed(f"radial_mlp/w_pad={w_pad}"):
        rc = lib.matten_radial_mlp(_ptr(geom_sorted), E, n_basis, r_start, r_end, _ptr(w0p), nb_pad, _ptr(w1p),
                                   _ptr(w2p), hidden, w_pad, 1.0, _ptr(out), int(out_dtype == torch.bfloat16), _stream())
    _lib.check(rc, "matten_radial_mlp")
    return out


def radial_pack(w0, w1, w2, scales):
    """raw radial layers -> (w0p [nb_pad,32], w1p [32,32], w2p [32,w_pad]) = the operands of radial_mlp in the reference's
    column order, each multiplied by its scale, in one launch"""
    lib = _lib.load()
    w0, w1, w2 = (_need(w, torch.float32, n) for w, n in ((w0, "layer0.weight"), (w1, "layer1.weight"), (w2, "layer2.weight")))
    nb, h = w0.shape
    W = w2.shape[1]
    nb_pad, w_pad = (nb + 3) // 4 * 4, (W + 15) // 16 * 16
    dev = w0.device
    w0p = torch.empty(nb_pad, h, dtype=torch.float32, device=dev)
    w1p = torch.empty(h, h, dtype=torch.float32, device=dev)
    w2p = torch.empty(h, w_pad, dtype=torch.float32, device=dev)
    _lib.check(lib.matten_radial_pack(_ptr(w0), _ptr(w1), _ptr(w2), nb, nb_pad, W, w_pad, float(scales[0]), float(scales[1]),
                                      float(scales[2]), _ptr(w0p), _ptr(w1p), _ptr(w2p), _stream()), "matten_radial_pack")
    return w0p, w1p, w2p


def fused_operands(w0, w1, w2, scales, cols, group_entries, n_tiles: int, r_start: float, r_end: float, act_cst: float):
    """Everything matten_radial_hidden + matten_tp_fused need, derived from the RAW radial layers by four small launches
    and no host reads (capturable): -> (w0p, w1p, w2p in fused column order, h_scale [2], a_split fragments, a_scale_inv)"""
    lib = _lib.load()
    w0, w1, w2 = (_need(w, torch.float32, n) for w, n in ((w0, "layer0.weight"), (w1, "layer1.weight"), (w2, "layer2.weight")))
    cols = _need(cols, torch.int64, "fused_cols")
    group_entries = _need(group_entries, torch.int32, "group_entries")
    nb, h = w0.shape
    W, n_cols = w2.shape[1], cols.numel()
    nb_pad, w_pad = (nb + 3) // 4 * 4, (n_cols + 15) // 16 * 16 + 16   # +16: whole tiles may start at any entry
    dev = w0.device
    w0p = torch.empty(nb_pad, h, dtype=torch.float32, device=dev)
    w1p = torch.empty(h, h, dtype=torch.float32, device=dev)
    w2p = torch.empty(h, w_pad, dtype=torch.float32, device=dev)
    hs = torch.empty(2, dtype=torch.float32, device=dev)
    n_ent = group_entries.shape[0]
    frag = torch.empty(n_tiles, 64, 16, dtype=torch.float16, device=dev)
    inv = torch.empty(n_ent, dtype=torch.float32, device=dev)
    st = _stream()
    _lib.check(lib.matten_radial_pack_cols(_ptr(w0), _ptr(w1), _ptr(w2), nb, nb_pad, W, _ptr(cols), n_cols, w_pad,
                                           float(scales[0]), float(scales[1]), float(scales[2]), _ptr(w0p), _ptr(w1p),
                                           _ptr(w2p), st), "matten_radial_pack_cols")
    _lib.check(lib.matten_radial_h_scale(_ptr(w0), _ptr(w1), nb, float(r_start), float(r_end), float(act_cst), _ptr(hs), st),
               "matten_radial_h_scale")
    _lib.check(lib.matten_split_a_tiles(_ptr(w2p), w_pad, _ptr(group_entries), n_ent, _ptr(hs), _ptr(frag), _ptr(inv), st),
               "matten_split_a_tiles")
    return w0p, w1p, w2p, hs, frag, inv


# ---- radial MLPs of any depth (invariant_layers = L in 1..4): the _deep entries of the C ABI ---------------------------
# The middle layers (32 -> 32, L - 1 of them) travel as ONE tensor w_mid [L-1, 32, 32] (raw or packed); L = 2 models keep
# the entries above (the _deep ones with n_mid = 1 run the same kernels).
RADIAL_MAX_MID = 3


def _mid(w_mid, name: str):
    """-> (contiguous fp32 [n_mid, 32, 32] or None when empty, n_mid)"""
    if not isinstance(w_mid, torch.Tensor) or w_mid.dim() != 3 or tuple(w_mid.shape[1:]) != (32, 32):
        raise ValueError(f"{name}: expected [n_mid, 32, 32]")
    n_mid = w_mid.shape[0]
    if n_mid > RADIAL_MAX_MID:
        raise ValueError(f"{name}: at most {RADIAL_MAX_MID} middle layers (invariant_layers <= {RADIAL_MAX_MID + 1})")
    return (_need(w_mid, torch.float32, name) if n_mid else None), n_mid


def radial_mlp_deep(geom_sorted, n_basis: int, r_start: float, r_end: float, w0p, w_mid, w2p,
                    out_dtype=torch.float32) -> torch.Tensor:
    """radial_mlp with w_mid [n_mid, 32, 32] packed middle layers in place of w1p"""
    lib = _lib.load()
    geom_sorted = _need(geom_sorted, torch.float32, "geom_sorted")
    w0p, w2p = _need(w0p, torch.float32, "w0p"), _need(w2p, torch.float32, "w2p")
    w_mid, n_mid = _mid(w_mid, "w_mid")
    E = geom_sorted.shape[0]
    nb_pad, hidden = w0p.shape
    w_pad = w2p.shape[1]
    if out_dtype not in (torch.float32, torch.bfloat16):
        raise TypeError("radial_mlp: out_dtype must be fp32 or bf16")
    out = torch.empty(E, w_pad, dtype=out_dtype, device=geom_sorted.device)
    with _timed(f"radial_mlp/w_pad={w_pad}"):
        rc = lib.matten_radial_mlp_deep(_ptr(geom_sorted), E, n_basis, r_start, r_end, _ptr(w0p), nb_pad, _ptr(w_mid), n_mid,
                                        _ptr(w2p), hidden, w_pad, 1.0, _ptr(out), int(out_dtype == torch.bfloat16), _stream())
    _lib.check(rc, "matten_radial_mlp_deep")
    return out


def radial_pack_deep(w0, w_mid, w2, scales):
    """radial_pack with the raw middle layers w_mid [n_mid, 32, 32] in place of w1 -> (w0p, w_mid_p, w2p)"""
    lib = _lib.load()
    w0, w2 = _need(w0, torch.float32, "layer0.weight"), _need(w2, torch.float32, "last layer weight")
    w_mid, n_mid = _mid(w_mid, "middle layer weights")
    nb, h = w0.shape
    W = w2.shape[1]
    nb_pad, w_pad = (nb + 3) // 4 * 4, (W + 15) // 16 * 16
    dev = w0.device
    w0p = torch.empty(nb_pad, h, dtype=torch.float32, device=dev)
    wmp = torch.empty(n_mid, h, h, dtype=torch.float32, device=dev)
    w2p = torch.empty(h, w_pad, dtype=torch.float32, device=dev)
    _lib.check(lib.matten_radial_pack_deep(_ptr(w0), _ptr(w_mid), n_mid, _ptr(w2), nb, nb_pad, W, w_pad, float(scales[0]),
                                           float(scales[1]), float(scales[2]), _ptr(w0p), _ptr(wmp) if n_mid else None,
                                           _ptr(w2p), _stream()), "matten_radial_pack_deep")
    return w0p, wmp, w2p


def radial_h_scale_deep(w0, w_mid, r_start: float, r_end: float, act_cst: float) -> torch.Tensor:
    """[s, 1/s] of RadialMLP._fp16_scale computed on the device from the RAW layers (w0 [nb, 32], w_mid [n_mid, 32, 32])"""
    lib = _lib.load()
    w0 = _need(w0, torch.float32, "layer0.weight")
    w_mid, n_mid = _mid(w_mid, "middle layer weights")
    hs = torch.empty(2, dtype=torch.float32, device=w0.device)
    _lib.check(lib.matten_radial_h_scale_deep(_ptr(w0), _ptr(w_mid), n_mid, w0.shape[0], float(r_start), float(r_end),
                                              float(act_cst), _ptr(hs), _stream()), "matten_radial_h_scale_deep")
    return hs


def fused_operands_deep(w0, w_mid, w2, scales, cols, group_entries, n_tiles: int, r_start: float, r_end: float,
                        act_cst: float):
    """fused_operands with the raw middle layers w_mid [n_mid, 32, 32] in place of w1 -> (w0p, w_mid_p, w2p, h_scale,
    a_split fragments, a_scale_inv)"""
    lib = _lib.load()
    w0, w2 = _need(w0, torch.float32, "layer0.weight"), _need(w2, torch.float32, "last layer weight")
    w_mid, n_mid = _mid(w_mid, "middle layer weights")
    cols = _need(cols, torch.int64, "fused_cols")
    group_entries = _need(group_entries, torch.int32, "group_entries")
    nb, h = w0.shape
    W, n_cols = w2.shape[1], cols.numel()
    nb_pad, w_pad = (nb + 3) // 4 * 4, (n_cols + 15) // 16 * 16 + 16   # +16: whole tiles may start at any entry
    dev = w0.device
    w0p = torch.empty(nb_pad, h, dtype=torch.float32, device=dev)
    wmp = torch.empty(n_mid, h, h, dtype=torch.float32, device=dev)
    w2p = torch.empty(h, w_pad, dtype=torch.float32, device=dev)
    hs = torch.empty(2, dtype=torch.float32, device=dev)
    n_ent = group_entries.shape[0]
    frag = torch.empty(n_tiles, 64, 16, dtype=torch.float16, device=dev)
    inv = torch.empty(n_ent, dtype=torch.float32, device=dev)
    st = _stream()
    _lib.check(lib.matten_radial_pack_cols_deep(_ptr(w0), _ptr(w_mid), n_mid, _ptr(w2), nb, nb_pad, W, _ptr(cols), n_cols,
                                                w_pad, float(scales[0]), float(scales[1]), float(scales[2]), _ptr(w0p),
                                                _ptr(wmp) if n_mid else None, _ptr(w2p), st), "matten_radial_pack_cols_deep")
    _lib.check(lib.matten_radial_h_scale_deep(_ptr(w0), _ptr(w_mid), n_mid, nb, float(r_start), float(r_end), float(act_cst),
                                              _ptr(hs), st), "matten_radial_h_scale_deep")
    _lib.check(lib.matten_split_a_tiles(_ptr(w2p), w_pad, _ptr(group_entries), n_ent, _ptr(hs), _ptr(frag), _ptr(inv), st),
               "matten_split_a_tiles")
    return w0p, wmp, w2p, hs, frag, inv


def radial_mlp_bwd_deep(geom_sorted, n_basis: int, r_start: float, r_end: float, w0p, w_mid, w2p, w_cols: int, dw,
                        scales=(1.0, 1.0, 1.0)):
    """radial_mlp_bwd with the packed middle layers w_mid [n_mid, 32, 32] in place of w1p
    -> (dW0 [nb_pad,32], dWmid [n_mid,32,32], dW2 [32,w_pad])"""
    lib = _lib.load()
    geom_sorted = _need(geom_sorted, torch.float32, "geom_sorted")
    w0p, w2p = _need(w0p, torch.float32, "w0p"), _need(w2p, torch.float32, "w2p")
    w_mid, n_mid = _mid(w_mid, "w_mid")
    if dw.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError("dw must be fp32 or bf16")
    dw = _need(dw, dw.dtype, "dw")
    E = geom_sorted.shape[0]
    nb_pad, hidden = w0p.shape
    w_pad = w2p.shape[1]
    dev = geom_sorted.device
    small_len = nb_pad * hidden + n_mid * hidden * hidden
    if E == 0:
        return w0p.new_zeros(nb_pad, hidden), w0p.new_zeros(n_mid, hidden, hidden), w2p.new_zeros(hidden, w_pad)
    n_small, n_rng = lib.matten_radial_mlp_bwd_small_slices(E), lib.matten_radial_mlp_bwd_w2_ranges_deep(E, w_pad, n_mid)
    h2 = torch.empty(E, hidden, dtype=torch.float32, device=dev)
    part_small = torch.empty(max(n_small, 1), small_len, dtype=torch.float32, device=dev)
    part_w2 = torch.empty(max(n_rng, 1), hidden, w_pad, dtype=torch.float32, device=dev)
    small = torch.empty(small_len, dtype=torch.float32, device=dev)
    d2 = torch.empty(hidden, w_pad, dtype=torch.float32, device=dev)
    with _timed(f"radial_mlp_bwd/w_pad={w_pad}"):
        rc = lib.matten_radial_mlp_bwd_deep(_ptr(geom_sorted), E, n_basis, r_start, r_end, _ptr(w0p), nb_pad, _ptr(w_mid),
                                            n_mid, _ptr(w2p), hidden, w_pad, int(w_cols), _ptr(dw), dw.shape[1],
                                            int(dw.dtype == torch.bfloat16), _ptr(h2), _ptr(part_small), _ptr(part_w2),
                                            float(scales[0]), float(scales[1]), float(scales[2]), _ptr(small), _ptr(d2),
                                            _stream())
    _lib.check(rc, "matten_radial_mlp_bwd_deep")
    return small[: nb_pad * hidden].reshape(nb_pad, hidden), small[nb_pad * hidden:].reshape(n_mid, hidden, hidden), d2


def gather_scale(src, idx, scale, scale_by_source: bool = False, perm2=None):
    """out[i] = src.flat[idx.flat[i]] * scale[(idx.flat[i] if scale_by_source else i) % len(scale)], shaped like idx.
    perm2 (int64 [len(scale)]): also return out2[r, q] = out[r, perm2[q]] (the same launch)"""
    lib = _lib.load()
    src = _need(src, torch.float32, "src")
    idx = _need(idx, torch.int64, "idx")
    scale = _need(scale, torch.float32, "scale")
    out = torch.empty(idx.shape, dtype=torch.float32, device=src.device)
    out2 = None
    if perm2 is not None:
        perm2 = _need(perm2, torch.int64, "perm2")
        out2 = torch.empty(idx.shape, dtype=torch.float32, device=src.device)
    _lib.check(lib.matten_gather_scale(_ptr(src), _ptr(idx), _ptr(scale), idx.numel(), scale.numel(), int(scale_by_source),
                                       _ptr(out), _ptr(perm2), _ptr(out2), _stream()), "matten_gather_scale")
    return out if perm2 is None else (out, out2)


def radial_mlp_bwd(geom_sorted, n_basis: int, r_start: float, r_end: float, w0p, w1p, w2p, w_cols: int, dw,
                   scales=(1.0, 1.0, 1.0)):
    """Adjoint of radial_mlp -> (dW0 [nb_pad,32], dW1 [32,32], dW2 [32,w_pad]): gradients w.r.t. the packed weights
    times `scales`, i.e. w.r.t. the raw layers when `scales` are the factors radial_pack applied.
    dw [E, ld >= w_pad] fp32 or bf16: dL/dw from tp_backward (pad columns are never read as data)."""
    lib = _lib.load()
    geom_sorted = _need(geom_sorted, torch.float32, "geom_sorted")
    w0p, w1p, w2p = (_need(w, torch.float32, n) for w, n in ((w0p, "w0p"), (w1p, "w1p"), (w2p, "w2p")))
    if dw.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError("dw must be fp32 or bf16")
    dw = _need(dw, dw.dtype, "dw")
    E = geom_sorted.shape[0]
    nb_pad, hidden = w0p.shape
    w_pad = w2p.shape[1]
    dev = geom_sorted.device
    n_small, n_rng = lib.matten_radial_mlp_bwd_small_slices(E), lib.matten_radial_mlp_bwd_w2_ranges(E, w_pad)
    h2 = torch.empty(E, hidden, dtype=torch.float32, device=dev)
    part_small = torch.empty(max(n_small, 1), nb_pad * hidden + hidden * hidden, dtype=torch.float32, device=dev)
    part_w2 = torch.empty(max(n_rng, 1), hidden, w_pad, dtype=torch.float32, device=dev)
    if E == 0:
        return w0p.new_zeros(nb_pad, hidden), w1p.new_zeros(hidden, hidden), w2p.new_zeros(hidden, w_pad)
    small = torch.empty(nb_pad * hidden + hidden * hidden, dtype=torch.float32, device=dev)
    d2 = torch.empty(hidden, w_pad, dtype=torch.float32, device=dev)
    with _timed(f"radial_mlp_bwd/w_pad={w_pad}"):
        # (the per-wave / per-range partial sums are added in a fixed order by the call's last launch: no atomics)
        rc = lib.matten_radial_mlp_bwd(_ptr(geom_sorted), E, n_basis, r_start, r_end, _ptr(w0p), nb_pad, _ptr(w1p),
                                       _ptr(w2p), hidden, w_pad, int(w_cols), _ptr(dw), dw.shape[1],
                                       int(dw.dtype == torch.bfloat16), _ptr(h2), _ptr(part_small), _ptr(part_w2),
                                       float(scales[0]), float(scales[1]), float(scales[2]), _ptr(small), _ptr(d2),
                                       _stream())
    _lib.check(rc, "matten_radial_mlp_bwd")
    return small[: nb_pad * hidden].reshape(nb_pad, hidden), small[nb_pad * hidden:].reshape(hidden, hidden), d2


def tp_paths(x, w_edge, sh_sorted, rowptr, src_sorted, entries, unit_start, units_per_tile: int, d_mid: int,
             avg_num_neighbors: float, num_neigh=None) -> torch.Tensor:
    lib = _lib.load()
    from .plan import TP_TILE_NODES

    if lib.matten_tp_tile_nodes() != TP_TILE_NODES:
        raise _lib.MattenHipError("plan.TP_TILE_NODES does not match the library's node tile")
    x = _need(x, torch.float32, "node_features")
    w_edge = _edge_dtype(w_edge, "w_edge")
    sh_sorted = _need(sh_sorted, torch.float32, "sh_sorted")
    # destination rows = segments of rowptr (virtual nodes when the segments were cut by ops.csr_split); x rows are sources
    N, d_in = rowptr.shape[0] - 1, x.shape[1]
    if num_neigh is not None:
        num_neigh = _need(num_neigh, torch.float32, "num_neigh")
    agg = torch.empty(N, d_mid, dtype=torch.float32, device=x.device)
    with _timed(f"tp_scatter/d_mid={d_mid}"):
        rc = lib.matten_tp_paths(_ptr(x), d_in, _ptr(w_edge), w_edge.shape[1], _ptr(sh_sorted), sh_sorted.shape[1],
                                 _ptr(rowptr), _ptr(src_sorted), N, _ptr(entries), _ptr(unit_start),
                                 entries.shape[0], units_per_tile, d_mid, float(avg_num_neighbors or 0.0),
                                 _ptr(num_neigh), _ptr(agg), int(w_edge.dtype == torch.bfloat16), _stream())
    _lib.check(rc, "matten_tp_paths")
    return agg


def split_hidden(h2p: torch.Tensor) -> torch.Tensor:
    """fp32 [E,32] (already in the permuted column order) -> the split fp16 form [E,2,32] matten_tp_fused consumes:
    v = hi + 2^-11 lo.  Test/tool helper: the production path gets this form from matten_radial_hidden."""
    tiny = 2.0 ** -14
    hi = torch.where(h2p.abs() < tiny, torch.zeros_like(h2p), h2p.half().float())
    lo = (h2p - hi) * 2048.0
    lo = torch.where(lo.abs() < tiny, torch.zeros_like(lo), lo)
    return torch.stack([hi.half(), lo.half()], dim=1).contiguous()


def radial_hidden(geom_sorted, n_basis: int, r_start: float, r_end: float, w0p, w1p, h_scale=None) -> torch.Tensor:
    """-> h2s [E,2,32] fp16 (hi | lo pieces of the 32 hidden features, see include/matten_hip.h).
    h_scale: optional fp32 device tensor whose first element is the power-of-two output scale (RadialMLP.h_scale)"""
    lib = _lib.load()
    geom_sorted = _need(geom_sorted, torch.float32, "geom_sorted")
    w0p, w1p = _need(w0p, torch.float32, "w0p"), _need(w1p, torch.float32, "w1p")
    E = geom_sorted.shape[0]
    h2p = torch.empty(E, 2, 32, dtype=torch.float16, device=geom_sorted.device)
    with _timed("radial_hidden"):
        if h_scale is not None:
            h_scale = _need(h_scale, torch.float32, "h_scale")
        rc = lib.matten_radial_hidden(_ptr(geom_sorted), E, n_basis, r_start, r_end, _ptr(w0p), w0p.shape[0],
                                      _ptr(w1p), w0p.shape[1], _ptr(h2p), _ptr(h_scale), _stream())
    _lib.check(rc, "matten_radial_hidden")
    return h2p


def radial_hidden_multi(geom_sorted, n_basis: int, r_start: float, r_end: float, w0ps, w1ps, h_scales=None):
    """h2s of several radial MLPs over the same edges in one launch -> list of [E,2,32] fp16"""
    import ctypes

    lib = _lib.load()
    geom_sorted = _need(geom_sorted, torch.float32, "geom_sorted")
    w0ps = [_need(w, torch.float32, "w0p") for w in w0ps]
    w1ps = [_need(w, torch.float32, "w1p") for w in w1ps]
    L, E = len(w0ps), geom_sorted.shape[0]
    if not 1 <= L <= 8 or len(w1ps) != L or any(w.shape != w0ps[0].shape for w in w0ps):
        raise ValueError("radial_hidden_multi: 1..8 layers with equal basis / hidden sizes")
    out = [torch.empty(E, 2, 32, dtype=torch.float16, device=geom_sorted.device) for _ in range(L)]
    arr = lambda ts: (ctypes.c_void_p * L)(*[t.data_ptr() for t in ts])
    if h_scales is not None:
        h_scales = [_need(h, torch.float32, "h_scale") for h in h_scales]
        if len(h_scales) != L:
            raise ValueError("one h_scale per layer")
    with _timed("radial_hidden_multi"):
        rc = lib.matten_radial_hidden_multi(_ptr(geom_sorted), E, n_basis, r_start, r_end, arr(w0ps), w0ps[0].shape[0],
                                            arr(w1ps), w0ps[0].shape[1], arr(out),
                                            arr(h_scales) if h_scales is not None else None, L, _stream())
    _lib.check(rc, "matten_radial_hidden_multi")
    return out


def radial_hidden_deep(geom_sorted, n_basis: int, r_start: float, r_end: float, w0p, w_mid, h_scale=None) -> torch.Tensor:
    """radial_hidden with the packed middle layers w_mid [n_mid, 32, 32] in place of w1p: h2s [E,2,32] fp16 of the LAST
    hidden layer"""
    lib = _lib.load()
    geom_sorted = _need(geom_sorted, torch.float32, "geom_sorted")
    w0p = _need(w0p, torch.float32, "w0p")
    w_mid, n_mid = _mid(w_mid, "w_mid")
    E = geom_sorted.shape[0]
    h2p = torch.empty(E, 2, 32, dtype=torch.float16, device=geom_sorted.device)
    with _timed("radial_hidden"):
        if h_scale is not None:
            h_scale = _need(h_scale, torch.float32, "h_scale")
        rc = lib.matten_radial_hidden_deep(_ptr(geom_sorted), E, n_basis, r_start, r_end, _ptr(w0p), w0p.shape[0],
                                           _ptr(w_mid), n_mid, w0p.shape[1], _ptr(h2p), _ptr(h_scale), _stream())
    _lib.check(rc, "matten_radial_hidden_deep")
    return h2p


def radial_hidden_multi_deep(geom_sorted, n_basis: int, r_start: float, r_end: float, w0ps, w_mids, h_scales=None):
    """radial_hidden_multi for MLPs of one depth: w_mids = their packed middle layers [n_mid, 32, 32]"""
    import ctypes

    lib = _lib.load()
    geom_sorted = _need(geom_sorted, torch.float32, "geom_sorted")
    w0ps = [_need(w, torch.float32, "w0p") for w in w0ps]
    mids = [_mid(w, "w_mid") for w in w_mids]
    L, E = len(w0ps), geom_sorted.shape[0]
    if not 1 <= L <= 8 or len(mids) != L or any(w.shape != w0ps[0].shape for w in w0ps) or \
            any(m[1] != mids[0][1] for m in mids):
        raise ValueError("radial_hidden_multi_deep: 1..8 layers with equal basis / hidden sizes and depth")
    n_mid = mids[0][1]
    out = [torch.empty(E, 2, 32, dtype=torch.float16, device=geom_sorted.device) for _ in range(L)]
    arr = lambda ts: (ctypes.c_void_p * L)(*[t.data_ptr() for t in ts])
    if h_scales is not None:
        h_scales = [_need(h, torch.float32, "h_scale") for h in h_scales]
        if len(h_scales) != L:
            raise ValueError("one h_scale per layer")
    with _timed("radial_hidden_multi"):
        rc = lib.matten_radial_hidden_multi_deep(_ptr(geom_sorted), E, n_basis, r_start, r_end, arr(w0ps), w0ps[0].shape[0],
                                                 arr([m[0] for m in mids]) if n_mid else None, n_mid, w0ps[0].shape[1],
                                                 arr(out), arr(h_scales) if h_scales is not None else None, L, _stream())
    _lib.check(rc, "matten_radial_hidden_multi_deep")
    return out


def split_a_tiles(w2p: torch.Tensor, group_entries) -> Tuple[torch.Tensor, torch.Tensor]:
    """w2p [32, w_pad] -> (a_split [n_tiles, 64, 16] fp16, a_scale_inv [n_entries] fp32): the last radial layer as the
    MFMA A fragments matten_tp_fused consumes (layout: include/matten_hip.h), per entry scaled by the power of two
    that puts its largest magnitude in [2^13, 2^14) and split v = hi + 2^-11 lo like ops.split_hidden.  Runs on the
    device without a host sync; cached by the caller until the weights change."""
    dev = w2p.device
    g = torch.arange(4, device=dev)[:, None]
    kk = torch.arange(8, device=dev)[None, :]
    k_idx = 16 * (kk >> 2) + 4 * g + (kk & 3)                       # [4 (g), 8 (kk)]
    tiny = 2.0 ** -14
    tiles, inv = [], []
    for row in np.asarray(group_entries).reshape(-1, 32):
        w_base, n_mt = int(row[5]), int(row[7])
        if int(row[0]) < 0 or n_mt == 0:   # second-half record of a merged entry (plan.TP_KIND_MERGED): no tiles of its own
            inv.append(torch.ones((), device=dev))
            continue
        A = w2p[k_idx][:, :, w_base:w_base + 16 * n_mt]              # [g, kk, mt*16 + c]
        A = A.reshape(4, 8, n_mt, 16).permute(2, 0, 3, 1)            # [mt, g, c, kk]
        amax = A.abs().max()
        e = torch.where(amax > 0, (torch.frexp(amax)[1] - 1).clamp(-100, 100), torch.full_like(amax, 13, dtype=torch.int32))
        scale = torch.ldexp(torch.ones_like(amax), 13 - e)
        inv.append(torch.ldexp(torch.ones_like(amax), e - 13))
        v = A * scale
        hi = torch.where(v.abs() < tiny, torch.zeros_like(v), v.half().float())
        lo = (v - hi) * 2048.0
        lo = torch.where(lo.abs() < tiny, torch.zeros_like(lo), lo)
        tiles.append(torch.cat([hi.half(), lo.half()], dim=-1).reshape(n_mt, 64, 16))
    return torch.cat(tiles).contiguous(), torch.stack(inv).float().contiguous()


_GROUPS_CHECKED = False


def tp_fused(x, h2p, w2p, sh_sorted, rowptr, src_sorted, entries, unit_map, units_per_tile: int,
             lds_floats_per_wave: int, d_mid: int, avg_num_neighbors: float, num_neigh=None,
             a_split=None, narrow=None) -> torch.Tensor:
    """a_split: optional (fragments, scale_inv) from split_a_tiles(w2p, plan.group_entries)
    narrow: optional (species index i32 [N], number of group entries) for a plan of plan.plan_agg_narrow: `entries` is then
    the 1-D int32 buffer of plan.narrow_blob (that plan's entries and the writer's weights), and the narrowed couplings
    leave with lin2 applied (matten_tp_fused_narrow)"""
    lib = _lib.load()
    from .plan import TP_TILE_NODES

    if lib.matten_tp_tile_nodes() != TP_TILE_NODES:
        raise _lib.MattenHipError("plan.TP_TILE_NODES does not match the library's node tile")
    from .plan import TP_MAX_COLS, TP_MAX_COLS_L0, TP_MAX_COLS_L1
    if (lib.matten_tp_max_cols() != TP_MAX_COLS or lib.matten_tp_max_cols_l0() != TP_MAX_COLS_L0
            or lib.matten_tp_max_cols_l1() != TP_MAX_COLS_L1):
        raise _lib.MattenHipError("plan.TP_MAX_COLS does not match the library's entry width (-DTPF_MAX_COLS)")
    from .plan import TP_WREG_MAX_L1, tp_wreg
    if tp_wreg() and lib.matten_tp_wreg() != TP_WREG_MAX_L1 + 1:
        raise _lib.MattenHipError("plans mark coupling-major entries (plan.TP_KIND_WREG) that this library was not built for "
                                  "(-DTPF_WREG=0 / -DTPF_WREG_MAX_L1): set MATTEN_TP_WREG=0")
    global _GROUPS_CHECKED
    from .plan import tp_groups_hash
    if not _GROUPS_CHECKED and lib.matten_tp_groups_hash() != tp_groups_hash():
        raise _lib.MattenHipError("the library's coupling code (cg_gen.h) was generated for other coupling groups than plan.TP_GROUPS "
                                  "(MATTEN_TP_GROUPS / an interrupted tools/*.sh A/B build?): make -C matten_amd/csrc clean all")
    _GROUPS_CHECKED = True   # (one library per process: checked at the first call)
    x = _need_rows(x, torch.float32, "node_features")  # a column slice is fine: d_in below is the row stride
    h2p = _need(h2p, torch.float16, "h2s")
    if h2p.dim() != 3 or h2p.shape[1:] != (2, 32):
        raise ValueError(f"h2s must be [E,2,32] fp16 (ops.split_hidden / ops.radial_hidden), got {tuple(h2p.shape)}")
    w2p = _need(w2p, torch.float32, "w2p")
    sh_sorted = _need(sh_sorted, torch.float32, "sh_sorted")
    # destination rows = segments of rowptr (virtual nodes when the segments were cut by ops.csr_split); x rows are sources
    N, d_in = rowptr.shape[0] - 1, x.stride(0)
    n_entries = entries.shape[0] if narrow is None else int(narrow[1])
    if num_neigh is not None:
        num_neigh = _need(num_neigh, torch.float32, "num_neigh")
    if a_split is not None:
        a_split = (_need(a_split[0], torch.float16, "a_split"), _need(a_split[1], torch.float32, "a_scale_inv"))
        if a_split[1].numel() != n_entries:
            raise ValueError("a_scale_inv needs one value per group entry")
    if unit_map.numel() != units_per_tile:
        raise ValueError(f"unit_map has {unit_map.numel()} units, expected {units_per_tile} (plan.fused_unit_map)")
    agg = torch.empty(N, d_mid, dtype=torch.float32, device=x.device)
    if narrow is not None:
        from .plan import AGG_NARROW_MAX_L1
        if lib.matten_tp_narrow_max_l1() != AGG_NARROW_MAX_L1:
            raise _lib.MattenHipError("plan.AGG_NARROW_MAX_L1 does not match the library (-DTPF_NARROW_MAX_L1)")
        sp = _need(narrow[0], torch.int32, "species")
        if sp.numel() != N or d_mid % 4 or entries.dim() != 1 or entries.numel() <= n_entries * 32:
            raise ValueError("narrow: one species index per destination row, d_mid a multiple of 4, and `entries` the buffer of "
                             "plan.narrow_blob (entries | weights)")
        with _timed(f"tp_scatter/d_mid={d_mid}/d_in={x.shape[1]}"):
            rc = lib.matten_tp_fused_narrow(_ptr(x), d_in, _ptr(h2p), _ptr(w2p), w2p.shape[1], _ptr(sh_sorted),
                                            sh_sorted.shape[1], _ptr(rowptr), _ptr(src_sorted), N, _ptr(entries),
                                            _ptr(unit_map), n_entries, units_per_tile, lds_floats_per_wave, d_mid,
                                            float(avg_num_neighbors or 0.0), _ptr(num_neigh),
                                            _ptr(a_split[0]) if a_split is not None else None,
                                            _ptr(a_split[1]) if a_split is not None else None, _ptr(sp), _ptr(agg), _stream())
        _lib.check(rc, "matten_tp_fused_narrow")
        return agg
    with _timed(f"tp_scatter/d_mid={d_mid}/d_in={x.shape[1]}"):
        rc = lib.matten_tp_fused(_ptr(x), d_in, _ptr(h2p), _ptr(w2p), w2p.shape[1], _ptr(sh_sorted),
                                 sh_sorted.shape[1], _ptr(rowptr), _ptr(src_sorted), N, _ptr(entries),
                                 _ptr(unit_map), entries.shape[0], units_per_tile, lds_floats_per_wave, d_mid,
                                 float(avg_num_neighbors or 0.0), _ptr(num_neigh),
                                 _ptr(a_split[0]) if a_split is not None else None,
                                 _ptr(a_split[1]) if a_split is not None else None, _ptr(agg), _stream())
    _lib.check(rc, "matten_tp_fused")
    return agg


def agg_linear(agg, species_order, wtab, io_table, blocks, d_out: int, add=None) -> torch.Tensor:
    """out[N, d_out] = add + lin2(agg) for component-major neighbour sums (include/matten_hip.h matten_agg_linear;
    tables from plan.plan_agg_linear).  species_order: (order, seg) or None for a single species."""
    lib = _lib.load()
    from .plan import AGG_BLOCK, AGG_MAX_MT
    if lib.matten_agg_linear_block_chunks() != AGG_BLOCK or lib.matten_agg_linear_max_mt() != AGG_MAX_MT:
        raise _lib.MattenHipError("plan.AGG_BLOCK / AGG_MAX_MT do not match the library (-DAL_BLK_CHUNKS)")
    agg = _need(agg, torch.float32, "agg")
    wtab = _need(wtab, torch.float32, "A fragments")
    n_rows, ld = agg.shape
    order, seg = species_order if species_order is not None else (None, None)
    n_species = wtab.shape[0] if wtab.dim() == 2 else 1
    if add is not None:
        add = _need_rows(add, torch.float32, "add")
    out = torch.empty(n_rows, d_out, dtype=torch.float32, device=agg.device)
    with _timed(f"agg_linear/ld={ld}"):
        rc = lib.matten_agg_linear(_ptr(agg), ld, _ptr(order), _ptr(seg), n_species, _ptr(wtab), wtab.shape[-1],
                                   _ptr(io_table), io_table.shape[0], _ptr(blocks), blocks.shape[0], _ptr(add),
                                   add.stride(0) if add is not None else d_out, d_out, n_rows, _ptr(out), _stream())
    _lib.check(rc, "matten_agg_linear")
    return out


def agg_linear_gate(agg, species_order, wtab, io_table, blocks, d_out: int, cmeta, act_cst, d_act: int, add=None,
                    bn_scale=None, bn_shift=None) -> torch.Tensor:
    """agg_linear + the layer's Gate (+ eval-mode BatchNorm as per-column scale / shift) in one launch ->
    the activated row [N, d_act] (include/matten_hip.h matten_agg_linear_gate; cmeta from plan.plan_agg_gate)"""
    lib = _lib.load()
    from .plan import AGG_BLOCK, AGG_GATE_SETS, AGG_MAX_MT
    if (lib.matten_agg_linear_block_chunks() != AGG_BLOCK or lib.matten_agg_linear_max_mt() != AGG_MAX_MT
            or lib.matten_agg_linear_gate_sets() != AGG_GATE_SETS):
        raise _lib.MattenHipError("plan.AGG_BLOCK / AGG_MAX_MT / AGG_GATE_SETS do not match the library")
    agg = _need(agg, torch.float32, "agg")
    wtab = _need(wtab, torch.float32, "A fragments")
    n_rows, ld = agg.shape
    order, seg = species_order if species_order is not None else (None, None)
    n_species = wtab.shape[0] if wtab.dim() == 2 else 1
    if add is not None:
        add = _need_rows(add, torch.float32, "add")
    if cmeta.shape != (d_out, 4):
        raise ValueError("cmeta must be [d_out, 4]")
    if bn_scale is not None:
        bn_scale, bn_shift = _need(bn_scale, torch.float32, "bn_scale"), _need(bn_shift, torch.float32, "bn_shift")
        if bn_scale.numel() != d_act or bn_shift.numel() != d_act:
            raise ValueError("bn_scale / bn_shift must have one value per activated column")
    out = torch.empty(n_rows, d_act, dtype=torch.float32, device=agg.device)
    with _timed(f"agg_linear/ld={ld}"):
        rc = lib.matten_agg_linear_gate(_ptr(agg), ld, _ptr(order), _ptr(seg), n_species, _ptr(wtab), wtab.shape[-1],
                                        _ptr(io_table), io_table.shape[0], _ptr(blocks), blocks.shape[0], _ptr(add),
                                        add.stride(0) if add is not None else d_out, d_out, n_rows, _ptr(cmeta),
                                        _ptr(act_cst), _ptr(bn_scale), _ptr(bn_shift), d_act, _ptr(out), _stream())
    _lib.check(rc, "matten_agg_linear_gate")
    return out


_SL_ROWS_LDS_BYTES = 52 * 1024  # three workgroups of matten_species_linear_rows per CU


def species_linear_route(d_in: int, w_stride: int, n_items_per_pass) -> str:
    """"rows" (matten_species_linear_rows: rows and weights resident in LDS) or "stream" (matten_species_linear) for a
    call with rows of d_in floats, w_stride packed weights per species and segment tables of n_items_per_pass items (one
    entry per pass).  Pure: the MATTEN_SL_ROWS override and species_linear's variant= argument act on top of it."""
    n_items = list(n_items_per_pass)
    fits = len(n_items) == 1 and 4 * (16 * (d_in | 1) + w_stride + 8 * n_items[0] + 4) <= _SL_ROWS_LDS_BYTES
    return "rows" if fits else "stream"


def species_linear(x, species_order, wp, w_stride: int, item_tables, d_out: int, add=None,
                   fully_covered: bool = True, variant: Optional[str] = None) -> torch.Tensor:
    """species_order: None (plain linear) or (order[N] i32, seg[S+1] i32) = nodes sorted by species.
    item_tables: list of int32 [n_items,8] tensors (passes).  out = add + sum_passes.
    variant: None = choose (row-resident kernel when rows + weights fit LDS), "rows" / "stream" force one (self-check)."""
    lib = _lib.load()
    x = _need(x, torch.float32, "x")
    from . import selfcheck
    selfcheck.check_species_linear(x.device)   # first call per device: both inline-asm MFMA kernels on exact integer cases
    wp = _need(wp, torch.float32, "packed weights")
    n_rows, d_in = x.shape
    order, seg = species_order if species_order is not None else (None, None)
    n_species = wp.shape[0] if wp.dim() == 2 else 1
    cur_add = add
    if cur_add is not None:
        cur_add = _need_rows(cur_add, torch.float32, "add")
    if fully_covered:
        out = torch.empty(n_rows, d_out, dtype=torch.float32, device=x.device)
    else:  # irreps without an input path stay zero (e3nn output_mask semantics)
        out = cur_add.clone() if cur_add is not None else torch.zeros(n_rows, d_out, dtype=torch.float32, device=x.device)
    # short rows (node features: lin1 / self-connection, first-layer lin2, read-out): rows and weights resident in LDS
    rows_fits = species_linear_route(d_in, w_stride, [t.shape[0] for t in item_tables]) == "rows"
    rows_variant = rows_fits and os.environ.get("MATTEN_SL_ROWS", "1") != "0"
    if variant is not None:
        rows_variant = rows_fits and variant == "rows"
    for items in item_tables:
        fn = lib.matten_species_linear_rows if rows_variant else lib.matten_species_linear
        _lib.check(
            fn(_ptr(x), d_in, _ptr(order), _ptr(seg), n_species, _ptr(wp), w_stride,
                                      _ptr(items), items.shape[0], d_out, _ptr(cur_add),
                                      cur_add.stride(0) if cur_add is not None else d_out, n_rows, _ptr(out), _stream()),
            "matten_species_linear",
        )
        cur_add = out
    return out


def gate_bn(x, meta, act_cst, running_mean=None, running_var=None, bn_weight=None, bn_bias=None, eps: float = 1e-5):
    lib = _lib.load()
    x = _need(x, torch.float32, "x")
    n_rows, d_in = x.shape
    d_out = meta.shape[0]
    out = torch.empty(n_rows, d_out, dtype=torch.float32, device=x.device)
    _lib.check(
        lib.matten_gate_bn(_ptr(x), d_in, _ptr(meta), d_out, _ptr(act_cst), _ptr(running_mean), _ptr(running_var),
                           _ptr(bn_weight), _ptr(bn_bias), eps, n_rows, _ptr(out), _stream()),
        "matten_gate_bn",
    )
    return out


def segment_reduce(x, ptr, mean: bool) -> torch.Tensor:
    lib = _lib.load()
    x = _need(x, torch.float32, "x")
    ptr = _need(ptr, torch.int64, "ptr")
    B = ptr.shape[0] - 1
    out = torch.empty(B, x.shape[1], dtype=torch.float32, device=x.device)
    _lib.check(lib.matten_segment_reduce(_ptr(x), x.shape[1], _ptr(ptr), B, int(mean), _ptr(out), _stream()),
               "matten_segment_reduce")
    return out


def segment_minmax(x, ptr, take_max: bool, want_arg: bool = False):
    """per crystal and column min / max -> out [B, dim] (and the source rows [B, dim] int64 when want_arg)"""
    lib = _lib.load()
    x = _need(x, torch.float32, "x")
    ptr = _need(ptr, torch.int64, "ptr")
    B = ptr.shape[0] - 1
    out = torch.empty(B, x.shape[1], dtype=torch.float32, device=x.device)
    arg = torch.empty(B, x.shape[1], dtype=torch.int64, device=x.device) if want_arg else None
    _lib.check(lib.matten_segment_minmax(_ptr(x), x.shape[1], _ptr(ptr), B, int(take_max), _ptr(out), _ptr(arg), _stream()),
               "matten_segment_minmax")
    return (out, arg) if want_arg else out


def segment_minmax_bwd(dy, arg, n_rows: int) -> torch.Tensor:
    lib = _lib.load()
    dy = _need(dy, torch.float32, "dy")
    dx = torch.zeros(n_rows, dy.shape[1], dtype=torch.float32, device=dy.device)
    _lib.check(lib.matten_segment_minmax_bwd(_ptr(dy), dy.shape[1], _ptr(arg), dy.shape[0], _ptr(dx), _stream()),
               "matten_segment_minmax_bwd")
    return dx


def dense_rows(x, q) -> torch.Tensor:
    lib = _lib.load()
    x = _need(x, torch.float32, "x")
    q = _need(q, torch.float32, "q")
    out = torch.empty(x.shape[0], q.shape[1], dtype=torch.float32, device=x.device)
    _lib.check(lib.matten_dense_rows(_ptr(x), x.shape[1], _ptr(q), q.shape[1], x.shape[0], _ptr(out), _stream()),
               "matten_dense_rows")
    return out


def elastic_props(c, layout: int):
    """c [B,81] (layout 0, Cartesian) or [B,36] (layout 1, Voigt), fp32 or fp64 -> (voigt [B,6,6], compliance [B,6,6],
    props [B,10], flags [B] int32), all fp64 (include/matten_hip.h: matten_elastic_props)"""
    lib = _lib.load()
    if not isinstance(c, torch.Tensor) or c.dtype not in (torch.float32, torch.float64):
        raise TypeError("c: expected an fp32 or fp64 tensor")
    c = _need(c, c.dtype, "c")
    if layout not in (0, 1) or c.dim() != 2 or c.shape[1] != (81, 36)[layout]:
        raise ValueError(f"c: expected [B,{(81, 36)[layout] if layout in (0, 1) else '?'}] for layout {layout}, got {tuple(c.shape)}")
    B = c.shape[0]
    voigt = torch.empty(B, 6, 6, dtype=torch.float64, device=c.device)
    compliance = torch.empty(B, 6, 6, dtype=torch.float64, device=c.device)
    props = torch.empty(B, 10, dtype=torch.float64, device=c.device)
    flags = torch.empty(B, dtype=torch.int32, device=c.device)
    _lib.check(lib.matten_elastic_props(_ptr(c), int(c.dtype == torch.float64), layout, B, _ptr(voigt), _ptr(compliance),
                                        _ptr(props), _ptr(flags), _stream()), "matten_elastic_props")
    return voigt, compliance, props, flags


def _opt_grad(g, shape, name: str):
    """an optional fp64 upstream gradient: None stays None (a null pointer for the kernel)"""
    if g is None:
        return None
    g = _need(g, torch.float64, name)
    if g.shape != shape:
        raise ValueError(f"{name}: expected {tuple(shape)}, got {tuple(g.shape)}")
    return g


def _ext_grad(g_ext, arg, B: int, n_ext: int, n_arg: int):
    """the extremes' optional upstream gradient g_ext [B,n_ext] and, with it, the forward's arg [B,n_arg] int32"""
    g_ext = _opt_grad(g_ext, (B, n_ext), "g_ext")
    if g_ext is None:
        return None, None
    if arg is None:
        raise ValueError("arg: the extremes' gradient g_ext needs the direction indices the forward returned")
    arg = _need(arg, torch.int32, "arg")
    if arg.shape != (B, n_arg):
        raise ValueError(f"arg: expected {(B, n_arg)}, got {tuple(arg.shape)}")
    return g_ext, arg


_ABSENT = object()


def _dir_set_args(matrix, name: str, flags, dirs, density=_ABSENT, cos_sin=_ABSENT):
    """the inputs the direction-set entries share, checked: ``matrix`` (``name`` = compliance or voigt) [B,6,6], flags [B],
    dirs [D>=1,3] and, for the entries that take them, density [B] and cos_sin [M>=1,2] -> those tensors (an argument the
    entry does not take stays as it is), B, D"""
    matrix = _need(matrix, torch.float64, name)
    flags = _need(flags, torch.int32, "flags")
    if density is not _ABSENT:
        density = _need(density, torch.float64, "density")
    dirs = _need(dirs, torch.float64, "dirs")
    if cos_sin is not _ABSENT:
        cos_sin = _need(cos_sin, torch.float64, "cos_sin")
    B = flags.shape[0]
    if (matrix.shape != (B, 6, 6) or (density is not _ABSENT and density.shape != (B,)) or dirs.dim() != 2
            or dirs.shape[1] != 3 or dirs.shape[0] < 1
            or (cos_sin is not _ABSENT and (cos_sin.dim() != 2 or cos_sin.shape[1] != 2 or cos_sin.shape[0] < 1))):
        took = [(f"{name} [B,6,6]", matrix), ("flags [B]", flags), ("density [B]", density), ("dirs [D>=1,3]", dirs),
                ("cos_sin [M>=1,2]", cos_sin)]
        took = [(what, t) for what, t in took if t is not _ABSENT]
        raise ValueError("expected " + ", ".join(what for what, _ in took) + "; got "
                         + ", ".join(str(tuple(t.shape)) for _, t in took))
    return matrix, flags, dirs, density, cos_sin, B, dirs.shape[0]


def elastic_props_bwd(voigt, compliance, props, flags, g_props, g_voigt, g_compliance, layout: int, dtype):
    """the adjoint of ``elastic_props``: its four outputs and the upstream gradients g_props [B,10], g_voigt [B,6,6] or
    None, g_compliance [B,6,6] or None (fp64; None = zero) -> the gradient of c, [B,81] (layout 0) or [B,36] (layout 1) in
    ``dtype`` (fp32 or fp64); rows with flag bit 0 are zero (matten_elastic_props_bwd)"""
    lib = _lib.load()
    if dtype not in (torch.float32, torch.float64):
        raise TypeError("dtype: expected fp32 or fp64")
    if layout not in (0, 1):
        raise ValueError(f"layout: expected 0 or 1, got {layout}")
    voigt = _need(voigt, torch.float64, "voigt")
    compliance = _need(compliance, torch.float64, "compliance")
    props = _need(props, torch.float64, "props")
    flags = _need(flags, torch.int32, "flags")
    g_props = _need(g_props, torch.float64, "g_props")
    B = flags.shape[0]
    if voigt.shape != (B, 6, 6) or compliance.shape != (B, 6, 6) or props.shape != (B, 10) or g_props.shape != (B, 10):
        raise ValueError(f"expected voigt / compliance [B,6,6], props / g_props [B,10], flags [B]; got {tuple(voigt.shape)}, "
                         f"{tuple(compliance.shape)}, {tuple(props.shape)}, {tuple(flags.shape)}, {tuple(g_props.shape)}")
    g_voigt = _opt_grad(g_voigt, (B, 6, 6), "g_voigt")
    g_compliance = _opt_grad(g_compliance, (B, 6, 6), "g_compliance")
    g_c = torch.empty(B, (81, 36)[layout], dtype=dtype, device=flags.device)
    _lib.check(lib.matten_elastic_props_bwd(_ptr(voigt), _ptr(compliance), _ptr(props), _ptr(flags), _ptr(g_props),
                                            _ptr(g_voigt), _ptr(g_compliance), int(dtype == torch.float64), layout, B,
                                            _ptr(g_c), _stream()), "matten_elastic_props_bwd")
    return g_c


def rank2_props(t, want_axes: bool = True):
    """t [N,9] (= [N,3,3] row-major), fp32 or fp64 -> (vals [N,3], axes [N,3,3] or None, props [N,5], flags [N] int32),
    all fp64 (include/matten_hip.h: matten_rank2_props)"""
    lib = _lib.load()
    if not isinstance(t, torch.Tensor) or t.dtype not in (torch.float32, torch.float64):
        raise TypeError("t: expected an fp32 or fp64 tensor")
    t = _need(t, t.dtype, "t")
    if t.dim() != 2 or t.shape[1] != 9:
        raise ValueError(f"t: expected [N,9], got {tuple(t.shape)}")
    N = t.shape[0]
    vals = torch.empty(N, 3, dtype=torch.float64, device=t.device)
    axes = torch.empty(N, 3, 3, dtype=torch.float64, device=t.device) if want_axes else None
    props = torch.empty(N, 5, dtype=torch.float64, device=t.device)
    flags = torch.empty(N, dtype=torch.int32, device=t.device)
    _lib.check(lib.matten_rank2_props(_ptr(t), int(t.dtype == torch.float64), N, _ptr(vals), _ptr(axes), _ptr(props),
                                      _ptr(flags), _stream()), "matten_rank2_props")
    return vals, axes, props, flags


def rank2_props_bwd(vals, axes, props, flags, g_vals, g_props, dtype):
    """the adjoint of ``rank2_props``: its four outputs and the upstream gradients g_vals [N,3] or None, g_props [N,5] or
    None (fp64; None = zero) -> the gradient of t, [N,9] in ``dtype`` (fp32 or fp64); rows with flag bit 0 are zero
    (matten_rank2_props_bwd)"""
    lib = _lib.load()
    if dtype not in (torch.float32, torch.float64):
        raise TypeError("dtype: expected fp32 or fp64")
    vals = _need(vals, torch.float64, "vals")
    axes = _need(axes, torch.float64, "axes")
    props = _need(props, torch.float64, "props")
    flags = _need(flags, torch.int32, "flags")
    N = flags.shape[0]
    if vals.shape != (N, 3) or axes.shape != (N, 3, 3) or props.shape != (N, 5):
        raise ValueError(f"expected vals [N,3], axes [N,3,3], props [N,5], flags [N]; got {tuple(vals.shape)}, "
                         f"{tuple(axes.shape)}, {tuple(props.shape)}, {tuple(flags.shape)}")
    g_vals = _opt_grad(g_vals, (N, 3), "g_vals")
    g_props = _opt_grad(g_props, (N, 5), "g_props")
    g_t = torch.empty(N, 9, dtype=dtype, device=flags.device)
    _lib.check(lib.matten_rank2_props_bwd(_ptr(vals), _ptr(axes), _ptr(props), _ptr(flags), _ptr(g_vals), _ptr(g_props),
                                          int(dtype == torch.float64), N, _ptr(g_t), _stream()), "matten_rank2_props_bwd")
    return g_t


WIGNER_STRIDE = 165      # doubles per rotation in the table of matten_wigner_d: the blocks D^0..D^4, 1 + 9 + 25 + 49 + 81
WIGNER_MAX_LAYOUT = 16   # layout rows per call of matten_irreps_rotate / matten_irreps_average


def wigner_d(R, lmax: int = 4, orth_tol: float = 1e-6, out=None):
    """R [G,3,3] (or [G,9]) fp64 -> (D [G,165] fp64, flags [G] int32): the packed blocks D^0..D^lmax of the proper part of
    every matrix; flags bit 0 non-finite, bit 1 not orthogonal to orth_tol (both: the row is NaN), bit 2 improper
    (include/matten_hip.h: matten_wigner_d).  ``out`` = (D, flags) to write into (a captured graph's buffers)."""
    lib = _lib.load()
    R = _need(R, torch.float64, "R")
    if R.dim() < 2 or R.numel() != R.shape[0] * 9:
        raise ValueError(f"R: expected [G,3,3], got {tuple(R.shape)}")
    G = R.shape[0]
    if out is None:
        D = torch.empty(G, WIGNER_STRIDE, dtype=torch.float64, device=R.device)
        flags = torch.empty(G, dtype=torch.int32, device=R.device)
    else:
        D, flags = _need(out[0], torch.float64, "D"), _need(out[1], torch.int32, "flags")
        if D.shape != (G, WIGNER_STRIDE) or flags.shape != (G,) or D is not out[0] or flags is not out[1]:
            raise ValueError("out: expected contiguous (D [G,165] fp64, flags [G] int32)")
    _lib.check(lib.matten_wigner_d(_ptr(R), G, int(lmax), float(orth_tol), _ptr(D), _ptr(flags), _stream()), "matten_wigner_d")
    return D, flags


def _irreps_rows(x, layout, D, flags):
    if not isinstance(x, torch.Tensor) or x.dtype not in (torch.float32, torch.float64):
        raise TypeError("x: expected an fp32 or fp64 tensor")
    x = _need(x, x.dtype, "x")
    if x.dim() != 2:
        raise ValueError(f"x: expected [n,dim], got {tuple(x.shape)}")
    layout = np.ascontiguousarray(layout, dtype=np.int32).reshape(-1, 4)     # host rows (offset, mul, l, parity)
    D = _need(D, torch.float64, "D")
    flags = _need(flags, torch.int32, "flags")
    if D.dim() != 2 or D.shape[1] != WIGNER_STRIDE or flags.shape != (D.shape[0],):
        raise ValueError(f"expected D [G,165] and flags [G], got {tuple(D.shape)}, {tuple(flags.shape)}")
    return x, layout, D, flags


def _irreps_out(x, out):
    if out is None:
        return torch.empty_like(x)
    if out.shape != x.shape or out.dtype != x.dtype or out.device != x.device or not out.is_contiguous():
        raise ValueError("out: expected a contiguous tensor of x's shape, dtype and device")
    return out


def irreps_rotate(x, layout, D, flags, index=None, transpose: bool = False, out=None):
    """out[r] = D(M_g) x[r] (``transpose``: D^T, the adjoint) with g = index[r], or without index g = 0 (one rotation) or
    g = r (one per row).  x [n,dim] fp32 or fp64, layout [K,4] host int32 rows (offset, mul, l, parity), (D, flags) of
    ``wigner_d`` (matten_irreps_rotate)"""
    lib = _lib.load()
    x, layout, D, flags = _irreps_rows(x, layout, D, flags)
    n, G = x.shape[0], D.shape[0]
    if index is not None:
        index = _need(index, torch.int32, "index")
        if index.shape != (n,):
            raise ValueError(f"index: expected [{n}], got {tuple(index.shape)}")
    elif n > 0 and G not in (1, n):
        raise ValueError(f"without index the {n} rows need 1 or {n} rotations, got {G}")
    out = _irreps_out(x, out)
    _lib.check(lib.matten_irreps_rotate(_ptr(x), int(x.dtype == torch.float64), n, x.shape[1], layout.ctypes.data, len(layout),
                                        _ptr(D), _ptr(flags), _ptr(index), G, int(bool(transpose)), _ptr(out), _stream()),
               "matten_irreps_rotate")
    return out


def irreps_average(x, layout, D, flags, op_ptr, op_idx, weights=None, transpose: bool = False, want_deviation: bool = True,
                   out=None):
    """out[r] = sum_j w_j D(M_op_idx[j]) x[r] / sum_j w_j over j in [op_ptr[r], op_ptr[r+1]) and deviation[r] =
    |x[r] - out[r]| / |x[r]| (fp64, or None).  op_ptr [n+1] int64 and op_idx [nnz] int32 on the device; the caller vouches
    for op_ptr (ascending, op_ptr[n] <= nnz), as for every CSR here; weights [nnz] fp64 or None (matten_irreps_average)"""
    lib = _lib.load()
    x, layout, D, flags = _irreps_rows(x, layout, D, flags)
    n = x.shape[0]
    op_ptr = _need(op_ptr, torch.int64, "op_ptr")
    op_idx = _need(op_idx, torch.int32, "op_idx")
    if op_ptr.shape != (n + 1,) or op_idx.dim() != 1:
        raise ValueError(f"expected op_ptr [{n + 1}] and op_idx [nnz], got {tuple(op_ptr.shape)}, {tuple(op_idx.shape)}")
    if weights is not None:
        weights = _need(weights, torch.float64, "weights")
        if weights.shape != op_idx.shape:
            raise ValueError(f"weights: expected {tuple(op_idx.shape)}, got {tuple(weights.shape)}")
    out = _irreps_out(x, out)
    # nnz = 0 (every list empty): an empty tensor has no address, and the library asks for one; flags stands in, unread
    idx_ptr = _ptr(op_idx) if op_idx.numel() else _ptr(flags)
    deviation = torch.empty(n, dtype=torch.float64, device=x.device) if want_deviation else None
    _lib.check(lib.matten_irreps_average(_ptr(x), int(x.dtype == torch.float64), n, x.shape[1], layout.ctypes.data, len(layout),
                                         _ptr(D), _ptr(flags), D.shape[0], _ptr(op_ptr), idx_ptr, _ptr(weights),
                                         int(bool(transpose)), _ptr(out), _ptr(deviation), _stream()), "matten_irreps_average")
    return out, deviation


SYM_MAX_OPS = 48        # operations per crystal (MATTEN_SYM_MAX_OPS): the order of the largest point group
SYM_MAX_ATOMS = 1024    # atoms per crystal that the symmetry search takes (MATTEN_SYM_MAX_ATOMS)


def _sym_out(out, specs, dev):
    """the output buffers of a symmetry entry: fresh ones, or the caller's ``out`` tuple checked against (shape, dtype)"""
    if out is None:
        return tuple(torch.empty(shape, dtype=dtype, device=dev) for shape, dtype in specs)
    if len(out) != len(specs):
        raise ValueError(f"out: expected {len(specs)} tensors")
    for t, (shape, dtype) in zip(out, specs):
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(shape) or t.dtype != dtype or t.device != dev \
                or not t.is_contiguous():
            raise ValueError(f"out: expected a contiguous {dtype} tensor of shape {tuple(shape)} on {dev}")
    return tuple(out)


def lattice_group(cell, symprec: float = 1e-3, out=None):
    """cell [B,3,3] fp64 -> (N [B,48,9] int8, n_lat [B] int32, flags [B] int32): the integer matrices that keep each
    cell's metric to ``symprec``, the identity first, then in ascending order (matten_lattice_group)"""
    lib = _lib.load()
    cell = _need(cell, torch.float64, "cell")
    if cell.dim() != 3 or cell.shape[1:] != (3, 3):
        raise ValueError(f"cell: expected [B,3,3], got {tuple(cell.shape)}")
    B = cell.shape[0]
    N, n_lat, flags = _sym_out(out, (((B, SYM_MAX_OPS, 9), torch.int8), ((B,), torch.int32), ((B,), torch.int32)), cell.device)
    if B:
        _lib.check(lib.matten_lattice_group(_ptr(cell), B, float(symprec), _ptr(N), _ptr(n_lat), _ptr(flags), _stream()),
                   "matten_lattice_group")
    return N, n_lat, flags


def crystal_symmetry(pos, cell, Z, ptr, lattice, pbc=None, symprec: float = 1e-3, max_trans: int = 64, out=None):
    """The operations of every crystal of a packed batch (pos [N,3] fp64, cell [B,3,3] fp64, Z [N] int64, ptr [B+1] int64,
    pbc [B,3] uint8 or None) among the lattice operations ``lattice`` = ``lattice_group(cell, symprec)`` ->
    (rot [B,48,9] fp64, rot_int [B,48,9] int8, trans [B,48,3] fp64, n_rot [B] int32, src [48,N] int32, n_trans [B] int32,
    ttrans [B,max_trans,3] fp64, tsrc [max_trans,N] int32, flags [B] int32) (matten_crystal_symmetry)"""
    lib = _lib.load()
    pos, cell = _need(pos, torch.float64, "pos"), _need(cell, torch.float64, "cell")
    Z, ptr = _need(Z, torch.int64, "Z"), _need(ptr, torch.int64, "ptr")
    N_in, n_lat, lat_flags = (_need(lattice[0], torch.int8, "lattice N"), _need(lattice[1], torch.int32, "lattice n_lat"),
                              _need(lattice[2], torch.int32, "lattice flags"))
    B, n = cell.shape[0], pos.shape[0]
    if pos.shape != (n, 3) or cell.shape != (B, 3, 3) or Z.shape != (n,) or ptr.shape != (B + 1,):
        raise ValueError("expected pos [N,3], cell [B,3,3], Z [N], ptr [B+1]")
    if N_in.shape != (B, SYM_MAX_OPS, 9) or n_lat.shape != (B,) or lat_flags.shape != (B,):
        raise ValueError("lattice: expected the (N [B,48,9], n_lat [B], flags [B]) of lattice_group")
    if pbc is not None:
        pbc = _need(pbc, torch.uint8, "pbc")
        if pbc.shape != (B, 3):
            raise ValueError(f"pbc: expected [{B},3], got {tuple(pbc.shape)}")
    max_trans = int(max_trans)
    if max_trans < 1:
        raise ValueError("max_trans: expected at least 1")
    f64, i32 = torch.float64, torch.int32
    specs = (((B, SYM_MAX_OPS, 9), f64), ((B, SYM_MAX_OPS, 9), torch.int8), ((B, SYM_MAX_OPS, 3), f64), ((B,), i32),
             ((SYM_MAX_OPS, n), i32), ((B,), i32), ((B, max_trans, 3), f64), ((max_trans, n), i32), ((B,), i32))
    bufs = _sym_out(out, specs, pos.device)
    if B and n:
        _lib.check(lib.matten_crystal_symmetry(_ptr(pos), _ptr(cell), _ptr(Z), _ptr(ptr), _ptr(pbc), B, n, float(symprec), max_trans,
                                               _ptr(N_in), _ptr(n_lat), _ptr(lat_flags), *[_ptr(t) for t in bufs], _stream()),
                   "matten_crystal_symmetry")
    return bufs


def irreps_average_atoms(x, layout, D, flags, n_ops, row_struct, src, out=None):
    """out[k] = (1 / n_ops[b]) sum_{g < n_ops[b]} D(R_{b,g}) x[src[g,k]], b = row_struct[k]: per-atom rows averaged over their
    crystal's operations.  x [n,dim] fp32 or fp64, (D [B*G_cap,165], flags) of ``wigner_d`` over the rotations [B,G_cap,3,3]
    or D = None for identity blocks, n_ops [B] int32, row_struct [n] int32, src [G_cap,n] int32 (matten_irreps_average_atoms)"""
    lib = _lib.load()
    if not isinstance(x, torch.Tensor) or x.dtype not in (torch.float32, torch.float64):
        raise TypeError("x: expected an fp32 or fp64 tensor")
    x = _need(x, x.dtype, "x")
    if x.dim() != 2:
        raise ValueError(f"x: expected [n,dim], got {tuple(x.shape)}")
    layout = np.ascontiguousarray(layout, dtype=np.int32).reshape(-1, 4)
    n_ops, row_struct, src = _need(n_ops, torch.int32, "n_ops"), _need(row_struct, torch.int32, "row_struct"), _need(src, torch.int32, "src")
    n, B = x.shape[0], n_ops.shape[0]
    if n_ops.dim() != 1 or row_struct.shape != (n,) or src.dim() != 2 or src.shape[1] != n or src.shape[0] < 1:
        raise ValueError("expected n_ops [B], row_struct [n] and src [G_cap,n]")
    G_cap = src.shape[0]
    if D is not None:
        D, flags = _need(D, torch.float64, "D"), _need(flags, torch.int32, "flags")
        if D.shape != (B * G_cap, WIGNER_STRIDE) or flags.shape != (B * G_cap,):
            raise ValueError(f"expected D [{B * G_cap},165] and flags [{B * G_cap}], got {tuple(D.shape)}, {tuple(flags.shape)}")
    out = _irreps_out(x, out)
    if out.data_ptr() == x.data_ptr() and n:
        raise ValueError("out: must not be x (rows are gathered from other atoms)")
    if n:
        _lib.check(lib.matten_irreps_average_atoms(_ptr(x), int(x.dtype == torch.float64), n, x.shape[1], layout.ctypes.data,
                                                   len(layout), _ptr(D), _ptr(flags) if D is not None else None, B, G_cap,
                                                   _ptr(n_ops), _ptr(row_struct), _ptr(src), _ptr(out), _stream()),
                   "matten_irreps_average_atoms")
    return out


def _kelvin_rows(voigt, flags):
    voigt = _need(voigt, torch.float64, "voigt")
    flags = _need(flags, torch.int32, "flags")
    B = flags.shape[0] if flags.dim() == 1 else -1
    if voigt.shape != (B, 6, 6):
        raise ValueError(f"expected voigt [B,6,6], flags [B]; got {tuple(voigt.shape)}, {tuple(flags.shape)}")
    return voigt, flags, B


def elastic_kelvin(voigt, flags, want_vectors: bool = True, want_dilatation: bool = True):
    """voigt [B,6,6] fp64 and flags [B] int32 as ``elastic_props`` returns them -> (moduli [B,6] ascending, vectors [B,6,6]
    or None, dilatation [B,6] or None), fp64: the Kelvin moduli of the Mandel matrix, their eigenvectors (columns) and
    (tr eps_k)^2 / 3; a row with flag bit 0 or a non-finite entry is NaN (include/matten_hip.h: matten_elastic_kelvin)"""
    lib = _lib.load()
    voigt, flags, B = _kelvin_rows(voigt, flags)
    moduli = torch.empty(B, 6, dtype=torch.float64, device=voigt.device)
    vectors = torch.empty(B, 6, 6, dtype=torch.float64, device=voigt.device) if want_vectors else None
    dilatation = torch.empty(B, 6, dtype=torch.float64, device=voigt.device) if want_dilatation else None
    _lib.check(lib.matten_elastic_kelvin(_ptr(voigt), _ptr(flags), B, _ptr(moduli), _ptr(vectors), _ptr(dilatation),
                                         _stream()), "matten_elastic_kelvin")
    return moduli, vectors, dilatation


def elastic_kelvin_bwd(vectors, flags, g_moduli) -> torch.Tensor:
    """the adjoint of ``elastic_kelvin``'s moduli: the forward's vectors [B,6,6], flags [B] and the upstream gradient
    g_moduli [B,6] (fp64) -> g_voigt [B,6,6] fp64, symmetric; rows with flag bit 0 or non-finite vectors are zero
    (matten_elastic_kelvin_bwd)"""
    lib = _lib.load()
    vectors, flags, B = _kelvin_rows(vectors, flags)
    g_moduli = _need(g_moduli, torch.float64, "g_moduli")
    if g_moduli.shape != (B, 6):
        raise ValueError(f"g_moduli: expected {(B, 6)}, got {tuple(g_moduli.shape)}")
    g_voigt = torch.empty(B, 6, 6, dtype=torch.float64, device=vectors.device)
    _lib.check(lib.matten_elastic_kelvin_bwd(_ptr(vectors), _ptr(flags), _ptr(g_moduli), B, _ptr(g_voigt), _stream()),
               "matten_elastic_kelvin_bwd")
    return g_voigt


def elastic_kelvin_clamp(voigt, moduli, vectors, floor: float = 0.0) -> torch.Tensor:
    """voigt [B,6,6] and the moduli [B,6] and vectors [B,6,6] ``elastic_kelvin`` gave for it (fp64), floor >= 0 ->
    [B,6,6] fp64: the Voigt matrix of the nearest tensor whose Kelvin moduli are all >= floor; rows that already are come
    back as they went in, bit for bit (matten_elastic_kelvin_clamp).  ``voigt`` must be the SYMMETRISED matrix, as
    ``elastic_props`` returns it: a kept row is a copy of its 36 entries, so an unsymmetric row would come back unsymmetric
    beside rebuilt rows that are symmetric."""
    lib = _lib.load()
    floor = float(floor)
    if not (np.isfinite(floor) and floor >= 0.0):
        raise ValueError(f"floor: expected a finite number >= 0, got {floor!r}")
    voigt = _need(voigt, torch.float64, "voigt")
    moduli = _need(moduli, torch.float64, "moduli")
    vectors = _need(vectors, torch.float64, "vectors")
    B = moduli.shape[0]
    if voigt.shape != (B, 6, 6) or moduli.shape != (B, 6) or vectors.shape != (B, 6, 6):
        raise ValueError(f"expected voigt / vectors [B,6,6], moduli [B,6]; got {tuple(voigt.shape)}, {tuple(vectors.shape)}, "
                         f"{tuple(moduli.shape)}")
    out = torch.empty(B, 6, 6, dtype=torch.float64, device=voigt.device)
    _lib.check(lib.matten_elastic_kelvin_clamp(_ptr(voigt), _ptr(moduli), _ptr(vectors), floor, B, _ptr(out), _stream()),
               "matten_elastic_kelvin_clamp")
    return out


def elastic_polycrystal(voigt, flags, moduli, vectors, hs_grid: int = 64, sc_tol: float = 1e-12, sc_max_iter: int = 200,
                        want_media: bool = True):
    """voigt [B,6,6] fp64 and flags [B] int32 as ``elastic_props`` returns them, moduli [B,6] and vectors [B,6,6] as
    ``elastic_kelvin`` returns them for it -> (out [B,6] = k_hs_lower, g_hs_lower, k_sc, g_sc, k_hs_upper, g_hs_upper,
    media [B,8] or None = the (K0, G0) of the four bounds, status [B,2] int32 = status, iterations): the Hashin-Shtrikman
    bounds and the self-consistent estimate (include/matten_hip.h: matten_elastic_polycrystal)"""
    lib = _lib.load()
    hs_grid, sc_tol, sc_max_iter = int(hs_grid), float(sc_tol), int(sc_max_iter)
    if not 2 <= hs_grid <= 0x7fffffff:
        raise ValueError(f"hs_grid: expected an int >= 2, got {hs_grid!r}")
    if not (np.isfinite(sc_tol) and sc_tol > 0.0):
        raise ValueError(f"sc_tol: expected a finite positive number, got {sc_tol!r}")
    if not 1 <= sc_max_iter <= 0x7fffffff:
        raise ValueError(f"sc_max_iter: expected an int >= 1, got {sc_max_iter!r}")
    voigt, flags, B = _kelvin_rows(voigt, flags)
    moduli = _need(moduli, torch.float64, "moduli")
    vectors = _need(vectors, torch.float64, "vectors")
    if moduli.shape != (B, 6) or vectors.shape != (B, 6, 6):
        raise ValueError(f"expected moduli [B,6], vectors [B,6,6]; got {tuple(moduli.shape)}, {tuple(vectors.shape)}")
    out = torch.empty(B, 6, dtype=torch.float64, device=voigt.device)
    media = torch.empty(B, 8, dtype=torch.float64, device=voigt.device) if want_media else None
    status = torch.empty(B, 2, dtype=torch.int32, device=voigt.device)
    _lib.check(lib.matten_elastic_polycrystal(_ptr(voigt), _ptr(flags), _ptr(moduli), _ptr(vectors), B, hs_grid, sc_tol,
                                              sc_max_iter, _ptr(out), _ptr(media), _ptr(status), _stream()),
               "matten_elastic_polycrystal")
    return out, media, status


def elastic_polycrystal_bwd(voigt, flags, out, status, g_sc) -> torch.Tensor:
    """the adjoint of ``elastic_polycrystal``'s self-consistent pair: voigt [B,6,6], flags [B] as the forward got them, out
    [B,6] and status [B,2] as it wrote them, the upstream gradient g_sc [B,2] of (k_sc, g_sc) (fp64) -> g_voigt [B,6,6]
    fp64, symmetric; rows with status -1 or 2 are zero (matten_elastic_polycrystal_bwd)"""
    lib = _lib.load()
    voigt, flags, B = _kelvin_rows(voigt, flags)
    out = _need(out, torch.float64, "out")
    status = _need(status, torch.int32, "status")
    g_sc = _need(g_sc, torch.float64, "g_sc")
    if out.shape != (B, 6) or status.shape != (B, 2) or g_sc.shape != (B, 2):
        raise ValueError(f"expected out [B,6], status [B,2], g_sc [B,2]; got {tuple(out.shape)}, {tuple(status.shape)}, "
                         f"{tuple(g_sc.shape)}")
    g_voigt = torch.empty(B, 6, 6, dtype=torch.float64, device=voigt.device)
    _lib.check(lib.matten_elastic_polycrystal_bwd(_ptr(voigt), _ptr(flags), _ptr(out), _ptr(status), _ptr(g_sc), B,
                                                  _ptr(g_voigt), _stream()), "matten_elastic_polycrystal_bwd")
    return g_voigt


TEXTURE_SLICE = 1024          # orientations per workgroup of matten_texture_operator
_TEXTURE_PART = 448           # doubles per (texture, slice) partial sum


def texture_operator(R, weights, tex_ptr, orth_tol: float = 1e-6, slice_len: int = TEXTURE_SLICE):
    """R [G,3,3] fp64, weights [G] fp64 or None (equal), tex_ptr [T+1] int64 (texture t owns orientations tex_ptr[t] ..
    tex_ptr[t+1]) -> (op [T,21,21] fp64, tex_flags [T] int32): the operator of every texture on the 21 upper-triangle
    entries of a Mandel matrix; a bad texture is NaN with flag bit 0.  ``slice_len`` orientations go to one workgroup, the
    slices' partial sums are added in order (include/matten_hip.h: matten_texture_operator)"""
    lib = _lib.load()
    slice_len, orth_tol = int(slice_len), float(orth_tol)
    if slice_len < 1:
        raise ValueError(f"slice_len: expected an int >= 1, got {slice_len!r}")
    if not (np.isfinite(orth_tol) and orth_tol >= 0.0):
        raise ValueError(f"orth_tol: expected a finite number >= 0, got {orth_tol!r}")
    R = _need(R, torch.float64, "R")
    tex_ptr = _need(tex_ptr, torch.int64, "tex_ptr")
    if R.dim() != 3 or R.shape[1:] != (3, 3) or tex_ptr.dim() != 1 or tex_ptr.numel() < 1:
        raise ValueError(f"expected R [G,3,3], tex_ptr [T+1]; got {tuple(R.shape)}, {tuple(tex_ptr.shape)}")
    G, T = R.shape[0], tex_ptr.numel() - 1
    if weights is not None:
        weights = _need(weights, torch.float64, "weights")
        if weights.shape != (G,):
            raise ValueError(f"weights: expected {(G,)}, got {tuple(weights.shape)}")
    op = torch.empty(T, 21, 21, dtype=torch.float64, device=R.device)
    tex_flags = torch.empty(T, dtype=torch.int32, device=R.device)
    n_ws = T * ((G + slice_len - 1) // slice_len) * _TEXTURE_PART
    ws = torch.empty(n_ws, dtype=torch.float64, device=R.device) if n_ws else None
    _lib.check(lib.matten_texture_operator(_ptr(R), _ptr(weights), _ptr(tex_ptr), G, T, orth_tol, slice_len, _ptr(ws), n_ws,
                                           _ptr(op), _ptr(tex_flags), _stream()), "matten_texture_operator")
    return op, tex_flags


def _texture_members(op, tex_flags, member_crystal, member_texture, member_fraction, agg_ptr):
    op, tex_flags = _need(op, torch.float64, "op"), _need(tex_flags, torch.int32, "tex_flags")
    member_crystal = _need(member_crystal, torch.int32, "member_crystal")
    member_texture = _need(member_texture, torch.int32, "member_texture")
    member_fraction = _need(member_fraction, torch.float64, "member_fraction")
    agg_ptr = _need(agg_ptr, torch.int64, "agg_ptr")
    T, M = tex_flags.shape[0] if tex_flags.dim() == 1 else -1, member_crystal.numel()
    if op.shape != (T, 21, 21):
        raise ValueError(f"expected op [T,21,21], tex_flags [T]; got {tuple(op.shape)}, {tuple(tex_flags.shape)}")
    if member_crystal.shape != (M,) or member_texture.shape != (M,) or member_fraction.shape != (M,) or agg_ptr.dim() != 1 \
            or agg_ptr.numel() < 1:
        raise ValueError("expected member_crystal, member_texture, member_fraction [M] and agg_ptr [A+1]")
    return op, tex_flags, member_crystal, member_texture, member_fraction, agg_ptr, T, M, agg_ptr.numel() - 1


def texture_average(voigt, flags, moduli, vectors, op, tex_flags, member_crystal, member_texture, member_fraction, agg_ptr):
    """voigt [n,6,6] fp64, flags [n] int32 as ``elastic_props`` returns them, moduli [n,6], vectors [n,6,6] as
    ``elastic_kelvin`` returns them for it; (op, tex_flags) of ``texture_operator``; the members (crystal [M] int32, texture
    [M] int32, fraction [M] fp64) of the aggregates agg_ptr [A+1] int64 -> (out [A,4,6,6] = the voigt, reuss, hill and
    geometric means as Voigt matrices, status [A] int32: 0, 2 not positive definite, -1 no value)
    (include/matten_hip.h: matten_texture_average)"""
    lib = _lib.load()
    voigt, flags, n = _kelvin_rows(voigt, flags)
    moduli, vectors = _need(moduli, torch.float64, "moduli"), _need(vectors, torch.float64, "vectors")
    if moduli.shape != (n, 6) or vectors.shape != (n, 6, 6):
        raise ValueError(f"expected moduli [n,6], vectors [n,6,6]; got {tuple(moduli.shape)}, {tuple(vectors.shape)}")
    op, tex_flags, mc, mt, mf, agg_ptr, T, M, A = _texture_members(op, tex_flags, member_crystal, member_texture,
                                                                  member_fraction, agg_ptr)
    out = torch.empty(A, 4, 6, 6, dtype=torch.float64, device=voigt.device)
    status = torch.empty(A, dtype=torch.int32, device=voigt.device)
    _lib.check(lib.matten_texture_average(_ptr(voigt), _ptr(flags), _ptr(moduli), _ptr(vectors), n, _ptr(op), _ptr(tex_flags), T,
                                          _ptr(mc), _ptr(mt), _ptr(mf), M, _ptr(agg_ptr), A, _ptr(out), _ptr(status), _stream()),
               "matten_texture_average")
    return out, status


def texture_average_bwd(moduli, vectors, op, tex_flags, member_crystal, member_texture, member_fraction, agg_ptr, out, status,
                        g_out, crystal_ptr, crystal_member) -> torch.Tensor:
    """the adjoint of ``texture_average``: its inputs, its outputs (out [A,4,6,6], status [A]), the upstream gradient g_out
    [A,4,6,6] and the inverse of member_crystal (crystal_ptr [n+1] int64, crystal_member [M] int32: the members of every
    crystal, ascending) -> g_voigt [n,6,6] fp64, symmetric; a crystal's memberships are added in member order
    (matten_texture_average_bwd)"""
    lib = _lib.load()
    moduli, vectors = _need(moduli, torch.float64, "moduli"), _need(vectors, torch.float64, "vectors")
    n = moduli.shape[0]
    if moduli.shape != (n, 6) or vectors.shape != (n, 6, 6):
        raise ValueError(f"expected moduli [n,6], vectors [n,6,6]; got {tuple(moduli.shape)}, {tuple(vectors.shape)}")
    op, tex_flags, mc, mt, mf, agg_ptr, T, M, A = _texture_members(op, tex_flags, member_crystal, member_texture,
                                                                  member_fraction, agg_ptr)
    out, g_out = _need(out, torch.float64, "out"), _need(g_out, torch.float64, "g_out")
    status = _need(status, torch.int32, "status")
    crystal_ptr, crystal_member = _need(crystal_ptr, torch.int64, "crystal_ptr"), _need(crystal_member, torch.int32, "crystal_member")
    if out.shape != (A, 4, 6, 6) or g_out.shape != (A, 4, 6, 6) or status.shape != (A,):
        raise ValueError(f"expected out, g_out [A,4,6,6], status [A]; got {tuple(out.shape)}, {tuple(g_out.shape)}, "
                         f"{tuple(status.shape)}")
    if crystal_ptr.shape != (n + 1,) or crystal_member.shape != (M,):
        raise ValueError(f"expected crystal_ptr [{n + 1}], crystal_member [{M}]; got {tuple(crystal_ptr.shape)}, "
                         f"{tuple(crystal_member.shape)}")
    g_voigt = torch.empty(n, 6, 6, dtype=torch.float64, device=moduli.device)
    n_ws = A * 64 + M * 21
    ws = torch.empty(n_ws, dtype=torch.float64, device=moduli.device) if n_ws else None
    _lib.check(lib.matten_texture_average_bwd(_ptr(moduli), _ptr(vectors), n, _ptr(op), T, _ptr(mc), _ptr(mt), _ptr(mf), M,
                                              _ptr(agg_ptr), A, _ptr(out), _ptr(status), _ptr(g_out), _ptr(crystal_ptr),
                                              _ptr(crystal_member), _ptr(ws), n_ws, _ptr(g_voigt), _stream()),
               "matten_texture_average_bwd")
    return g_voigt


def elastic_directional(compliance, flags, dirs, keep: bool = False):
    """compliance [B,6,6] fp64, flags [B] int32, unit directions dirs [D,3] fp64 -> (young [B,D] or None, beta [B,D] or
    None, ext [B,4] = E_min, E_max, beta_min, beta_max, arg [B,4] int32) (matten_elastic_directional)"""
    lib = _lib.load()
    compliance, flags, dirs, _, _, B, D = _dir_set_args(compliance, "compliance", flags, dirs)
    young = torch.empty(B, D, dtype=torch.float64, device=dirs.device) if keep else None
    beta = torch.empty(B, D, dtype=torch.float64, device=dirs.device) if keep else None
    ext = torch.empty(B, 4, dtype=torch.float64, device=dirs.device)
    arg = torch.empty(B, 4, dtype=torch.int32, device=dirs.device)
    _lib.check(lib.matten_elastic_directional(_ptr(compliance), _ptr(flags), _ptr(dirs), B, D, _ptr(young), _ptr(beta),
                                              _ptr(ext), _ptr(arg), _stream()), "matten_elastic_directional")
    return young, beta, ext, arg


def elastic_pair(compliance, flags, dirs, cos_sin, keep: bool = False):
    """compliance [B,6,6] fp64, flags [B] int32, unit directions dirs [D,3] fp64, cos_sin [M,2] fp64 -> (maps [B,D,4] or
    None, ext [B,4] = G_min, G_max, nu_min, nu_max, arg [B,4] int32 = flat pair indices d M + k) (matten_elastic_pair)"""
    lib = _lib.load()
    compliance, flags, dirs, _, cos_sin, B, D = _dir_set_args(compliance, "compliance", flags, dirs, cos_sin=cos_sin)
    M = cos_sin.shape[0]
    maps = torch.empty(B, D, 4, dtype=torch.float64, device=dirs.device) if keep else None
    ext = torch.empty(B, 4, dtype=torch.float64, device=dirs.device)
    arg = torch.empty(B, 4, dtype=torch.int32, device=dirs.device)
    _lib.check(lib.matten_elastic_pair(_ptr(compliance), _ptr(flags), _ptr(dirs), _ptr(cos_sin), B, D, M, _ptr(maps), _ptr(ext),
                                       _ptr(arg), _stream()), "matten_elastic_pair")
    return maps, ext, arg


def elastic_acoustic(voigt, flags, density, dirs, modulus_unit: float = 1e9, keep: bool = False):
    """voigt [B,6,6] fp64, flags [B] int32, density [B] fp64 (kg/m^3), unit directions dirs [D,3] fp64, modulus_unit in Pa
    per unit of voigt -> (vel [B,D,3] or None, ext [B,3] = v_slow_min, v_fast_max, sum of v^-3, arg [B,2] int32,
    n_unstable [B] int32) (matten_elastic_acoustic)"""
    lib = _lib.load()
    voigt, flags, dirs, density, _, B, D = _dir_set_args(voigt, "voigt", flags, dirs, density=density)
    vel = torch.empty(B, D, 3, dtype=torch.float64, device=dirs.device) if keep else None
    ext = torch.empty(B, 3, dtype=torch.float64, device=dirs.device)
    arg = torch.empty(B, 2, dtype=torch.int32, device=dirs.device)
    n_unstable = torch.empty(B, dtype=torch.int32, device=dirs.device)
    _lib.check(lib.matten_elastic_acoustic(_ptr(voigt), _ptr(flags), _ptr(density), _ptr(dirs), B, D, float(modulus_unit),
                                           _ptr(vel), _ptr(ext), _ptr(arg), _ptr(n_unstable), _stream()),
               "matten_elastic_acoustic")
    return vel, ext, arg, n_unstable


def elastic_waves(voigt, flags, density, dirs, modulus_unit: float = 1e9, deg_tol: float = 1e-6, keep: bool = True):
    """voigt [B,6,6] fp64, flags [B] int32, density [B] fp64 (kg/m^3), unit directions dirs [D,3] fp64, modulus_unit in Pa
    per unit of voigt, deg_tol the relative eigenvalue gap below which a mode counts as degenerate -> (pol [B,D,3,3],
    group [B,D,3,3], scal [B,D,3,5] = v, |g|, psi, character, J -- each None without ``keep`` --, ext [B,6] = psi_max per
    branch, then min |J| per branch, arg [B,6] int32, n_degenerate [B,3] int32, n_unstable [B] int32)
    (matten_elastic_waves)"""
    lib = _lib.load()
    voigt, flags, dirs, density, _, B, D = _dir_set_args(voigt, "voigt", flags, dirs, density=density)
    deg_tol = float(deg_tol)
    if not (0.0 <= deg_tol < float("inf")):
        raise ValueError(f"deg_tol: expected a finite value >= 0, got {deg_tol}")
    dev = dirs.device
    pol = torch.empty(B, D, 3, 3, dtype=torch.float64, device=dev) if keep else None
    group = torch.empty(B, D, 3, 3, dtype=torch.float64, device=dev) if keep else None
    scal = torch.empty(B, D, 3, 5, dtype=torch.float64, device=dev) if keep else None
    ext = torch.empty(B, 6, dtype=torch.float64, device=dev)
    arg = torch.empty(B, 6, dtype=torch.int32, device=dev)
    n_degenerate = torch.empty(B, 3, dtype=torch.int32, device=dev)
    n_unstable = torch.empty(B, dtype=torch.int32, device=dev)
    _lib.check(lib.matten_elastic_waves(_ptr(voigt), _ptr(flags), _ptr(density), _ptr(dirs), B, D, float(modulus_unit), deg_tol,
                                        _ptr(pol), _ptr(group), _ptr(scal), _ptr(ext), _ptr(arg), _ptr(n_degenerate),
                                        _ptr(n_unstable), _stream()),
               "matten_elastic_waves")
    return pol, group, scal, ext, arg, n_degenerate, n_unstable


def elastic_refine(compliance, flags, dirs, ext_dir, arg_dir, cos_sin=None, ext_pair=None, arg_pair=None, tol: float = 1e-9,
                   max_iter: int = 32):
    """the extremes of ``elastic_directional`` (ext_dir / arg_dir [B,4]) and, with cos_sin [M,2] and ext_pair / arg_pair
    [B,4], of ``elastic_pair`` refined off the grid -> (value [Q,B], n [Q,B,3], m [Q,B,3], status [Q,B] int32, iterations
    [Q,B] int32), Q = 4 (E_min, E_max, beta_min, beta_max) or 8 (then G_min, G_max, nu_min, nu_max)
    (matten_elastic_refine)"""
    lib = _lib.load()
    compliance, flags, dirs, _, _, B, D = _dir_set_args(compliance, "compliance", flags, dirs)
    ext_dir = _need(ext_dir, torch.float64, "ext_dir")
    arg_dir = _need(arg_dir, torch.int32, "arg_dir")
    if ext_dir.shape != (B, 4) or arg_dir.shape != (B, 4):
        raise ValueError(f"expected ext_dir / arg_dir [B,4]; got {tuple(ext_dir.shape)}, {tuple(arg_dir.shape)}")
    pair = (cos_sin is not None, ext_pair is not None, arg_pair is not None)
    if any(pair) != all(pair):
        raise ValueError("cos_sin, ext_pair and arg_pair go together: all three or none")
    M = 0
    if all(pair):
        cos_sin = _need(cos_sin, torch.float64, "cos_sin")
        ext_pair = _need(ext_pair, torch.float64, "ext_pair")
        arg_pair = _need(arg_pair, torch.int32, "arg_pair")
        if cos_sin.dim() != 2 or cos_sin.shape[1] != 2 or cos_sin.shape[0] < 1 or ext_pair.shape != (B, 4) or arg_pair.shape != (B, 4):
            raise ValueError(f"expected cos_sin [M>=1,2], ext_pair / arg_pair [B,4]; got {tuple(cos_sin.shape)}, "
                             f"{tuple(ext_pair.shape)}, {tuple(arg_pair.shape)}")
        M = cos_sin.shape[0]
    Q = 8 if M else 4
    value = torch.empty(Q, B, dtype=torch.float64, device=dirs.device)
    vec_n = torch.empty(Q, B, 3, dtype=torch.float64, device=dirs.device)
    vec_m = torch.empty(Q, B, 3, dtype=torch.float64, device=dirs.device)
    status = torch.empty(Q, B, dtype=torch.int32, device=dirs.device)
    iterations = torch.empty(Q, B, dtype=torch.int32, device=dirs.device)
    _lib.check(lib.matten_elastic_refine(_ptr(compliance), _ptr(flags), _ptr(dirs), _ptr(cos_sin), _ptr(ext_dir), _ptr(arg_dir),
                                         _ptr(ext_pair), _ptr(arg_pair), B, D, M, float(tol), int(max_iter), _ptr(value),
                                         _ptr(vec_n), _ptr(vec_m), _ptr(status), _ptr(iterations), _stream()),
               "matten_elastic_refine")
    return value, vec_n, vec_m, status, iterations


def elastic_directional_bwd(compliance, flags, dirs, g_young=None, g_beta=None, g_ext=None, arg=None) -> torch.Tensor:
    """the adjoint of ``elastic_directional``: its inputs, the upstream gradients g_young / g_beta [B,D] and g_ext [B,4] (fp64;
    None = zero) and the forward's arg [B,4] int32 (needed with g_ext) -> the gradient of compliance [B,6,6]; rows with
    flag bit 0 are zero (matten_elastic_directional_bwd)"""
    lib = _lib.load()
    compliance, flags, dirs, _, _, B, D = _dir_set_args(compliance, "compliance", flags, dirs)
    g_young = _opt_grad(g_young, (B, D), "g_young")
    g_beta = _opt_grad(g_beta, (B, D), "g_beta")
    g_ext, arg = _ext_grad(g_ext, arg, B, 4, 4)
    g_compliance = torch.empty(B, 6, 6, dtype=torch.float64, device=dirs.device)
    _lib.check(lib.matten_elastic_directional_bwd(_ptr(compliance), _ptr(flags), _ptr(dirs), B, D, _ptr(g_young), _ptr(g_beta),
                                                  _ptr(g_ext), _ptr(arg), _ptr(g_compliance), _stream()),
               "matten_elastic_directional_bwd")
    return g_compliance


def elastic_acoustic_bwd(voigt, flags, density, dirs, modulus_unit: float = 1e9, g_vel=None, g_ext=None, arg=None) -> torch.Tensor:
    """the adjoint of ``elastic_acoustic``: its inputs, the upstream gradients g_vel [B,D,3] and g_ext [B,3] (v_slow_min,
    v_fast_max, sum of v^-3; fp64; None = zero) and the forward's arg [B,2] int32 (needed with g_ext) -> the gradient of
    voigt [B,6,6]; rows with flag bit 0 or a bad density are zero, unstable directions add nothing
    (matten_elastic_acoustic_bwd)"""
    lib = _lib.load()
    voigt, flags, dirs, density, _, B, D = _dir_set_args(voigt, "voigt", flags, dirs, density=density)
    g_vel = _opt_grad(g_vel, (B, D, 3), "g_vel")
    g_ext, arg = _ext_grad(g_ext, arg, B, 3, 2)
    g_voigt = torch.empty(B, 6, 6, dtype=torch.float64, device=dirs.device)
    _lib.check(lib.matten_elastic_acoustic_bwd(_ptr(voigt), _ptr(flags), _ptr(density), _ptr(dirs), B, D, float(modulus_unit),
                                               _ptr(g_vel), _ptr(g_ext), _ptr(arg), _ptr(g_voigt), _stream()),
               "matten_elastic_acoustic_bwd")
    return g_voigt


# ---------------------------------------------------------------------------------------------------
# adjoint operators (training step)
# ---------------------------------------------------------------------------------------------------
def tp_backward(x, w_edge, sh_sorted, src_sorted, dst_sorted, col_meta, nnz_ijk, nnz_c, g_agg,
                avg_num_neighbors: float, num_neigh=None, in_groups=None):
    """-> (dx [N,d_in], dw [E,W]) for agg = tp(x, w_edge) with w_edge in the reference column order.
    in_groups: optional (in_ptr [n_in+1] i32, in_cols [W] i32) = the columns grouped by input channel (plan.bw_in_*)."""
    lib = _lib.load()
    x = _need(x, torch.float32, "x")
    w_edge = _edge_dtype(w_edge, "w_edge")
    g_agg = _need(g_agg, torch.float32, "grad agg")
    N, d_in = x.shape
    E = w_edge.shape[0]
    W = col_meta.shape[0]
    dx = torch.zeros(N, d_in, dtype=torch.float32, device=x.device)
    dw = torch.empty(E, w_edge.shape[1], dtype=w_edge.dtype, device=x.device)   # same row stride and storage as w_edge
    if num_neigh is not None:
        num_neigh = _need(num_neigh, torch.float32, "num_neigh")
    with _timed(f"tp_backward/d_mid={g_agg.shape[1]}/d_in={d_in}"):
        rc = lib.matten_tp_backward(_ptr(x), d_in, _ptr(w_edge), w_edge.shape[1], _ptr(sh_sorted), sh_sorted.shape[1],
                                    _ptr(src_sorted), _ptr(dst_sorted), _ptr(col_meta), W, _ptr(nnz_ijk), _ptr(nnz_c),
                                    _ptr(g_agg), g_agg.shape[1], float(avg_num_neighbors or 0.0), _ptr(num_neigh), E,
                                    _ptr(dx), _ptr(dw), dw.shape[1], _ptr(in_groups[0]) if in_groups else None,
                                    _ptr(in_groups[1]) if in_groups else None,
                                    in_groups[0].shape[0] - 1 if in_groups else 0,
                                    int(w_edge.dtype == torch.bfloat16), _stream())
    _lib.check(rc, "matten_tp_backward")
    return dx, dw


def split_a_tiles_dev(w2p, entries, n_tiles: int, h_scale=None):
    """-> (frag [n_tiles, 64, 16] fp16, scale_inv [n_entries]): matten_split_a_tiles on the device, no host read (the values of
    split_a_tiles; h_scale = the [s, 1/s] pair of matten_radial_h_scale folds 1/s into scale_inv)"""
    lib = _lib.load()
    w2p = _need(w2p, torch.float32, "w2p")
    entries = _need(entries, torch.int32, "entries")
    frag = torch.empty(n_tiles, 64, 16, dtype=torch.float16, device=w2p.device)
    inv = torch.empty(entries.shape[0], dtype=torch.float32, device=w2p.device)
    _lib.check(lib.matten_split_a_tiles(_ptr(w2p), w2p.shape[1], _ptr(entries), entries.shape[0], _ptr(h_scale), _ptr(frag),
                                        _ptr(inv), _stream()), "matten_split_a_tiles")
    return frag, inv


WFREE_MAX_MUL = 256   # widest input block (channels) matten_tp_backward_lit_wfree takes: one workgroup = 256 / lanes-per-edge edges


def tp_backward_lit(x, w_edge, sh_sorted, src_sorted, dst_sorted, blocks, paths, sum_lanes: int, g_agg,
                    avg_num_neighbors: float, num_neigh=None, out_csr=None, blocks_cover_input: bool = True, wfree=None,
                    dw_shape=None, lds_floats: int = 4096, max_l: int = 4, max_mul: int = 256):
    """the adjoint of tp_backward with literal-coefficient coupling code (include/matten_hip.h matten_tp_backward_lit;
    tables plan.bw_blocks / bw_paths) -> (dx [N,d_in], dw [E, ld of w_edge]).
    out_csr = (out_ptr [N+1] i32, out_perm [E] i32): sorted-edge indices grouped by SOURCE node -- dx is then summed per
    node in that fixed order (bitwise reproducible) instead of through atomics.
    wfree = (h2s [E, 2, 32] fp16, frag, w_inv) with w_edge None: the weights are re-evaluated inside the kernel on the matrix
    cores (matten_tp_backward_lit_wfree; frag / w_inv from split_a_tiles_dev over plan.bw_w_entries); dw_shape = ((E, ld), dtype);
    max_mul = plan.bw_max_mul, the widest block's channel count (the library refuses > 256: WFREE_MAX_MUL)."""
    lib = _lib.load()
    x = _need(x, torch.float32, "x")
    g_agg = _need(g_agg, torch.float32, "grad agg")
    N, d_in = x.shape
    if wfree is not None:
        if w_edge is not None or dw_shape is None:
            raise ValueError("wfree: pass w_edge=None and dw_shape=((E, ld), dtype)")
        h2s, frag, w_inv = (_need(t, dt, n) for t, dt, n in zip(wfree, (torch.float16, torch.float16, torch.float32),
                                                                ("h2s", "frag", "w_inv")))
        (E, dw_ld), dw_dtype = dw_shape
        if h2s.shape != (E, 2, 32) or w_inv.numel() != paths.shape[0]:
            raise ValueError("wfree: h2s must be [E, 2, 32] and w_inv hold one value per path")
    else:
        w_edge = _edge_dtype(w_edge, "w_edge")
        E, dw_ld, dw_dtype = w_edge.shape[0], w_edge.shape[1], w_edge.dtype
    if out_csr is not None:
        out_ptr, out_perm = (_need(t, torch.int32, n) for t, n in zip(out_csr, ("out_ptr", "out_perm")))
        dx = torch.empty(N, d_in, dtype=torch.float32, device=x.device)
        dx_edges = (torch.empty if blocks_cover_input else torch.zeros)(E, d_in, dtype=torch.float32, device=x.device)
    else:
        out_ptr = out_perm = dx_edges = None
        dx = torch.zeros(N, d_in, dtype=torch.float32, device=x.device)
    # columns no path writes (the pad up to the row stride) must not hold NaN for the MLP adjoint's masked reads: they are
    # masked by a select there, so plain empty storage is fine
    dw = torch.empty(E, dw_ld, dtype=dw_dtype, device=x.device)
    if num_neigh is not None:
        num_neigh = _need(num_neigh, torch.float32, "num_neigh")
    # the run of arguments the two entries share, from sh_sorted to dx_edges
    shared = (_ptr(sh_sorted), sh_sorted.shape[1], _ptr(src_sorted), _ptr(dst_sorted), _ptr(blocks), blocks.shape[0],
              int(sum_lanes), _ptr(paths), paths.shape[0], _ptr(g_agg), g_agg.shape[1], float(avg_num_neighbors or 0.0),
              _ptr(num_neigh), E, _ptr(dx), _ptr(dw), dw_ld, int(dw_dtype == torch.bfloat16), N, _ptr(out_ptr), _ptr(out_perm),
              _ptr(dx_edges))
    with _timed(f"tp_backward/d_mid={g_agg.shape[1]}/d_in={d_in}"):
        if wfree is not None:
            entry = "matten_tp_backward_lit_wfree"
            rc = lib.matten_tp_backward_lit_wfree(_ptr(x), d_in, _ptr(h2s), _ptr(frag), _ptr(w_inv), *shared, int(lds_floats),
                                                  int(max_l), int(max_mul), _stream())
        else:
            entry = "matten_tp_backward_lit"
            rc = lib.matten_tp_backward_lit(_ptr(x), d_in, _ptr(w_edge), dw_ld, *shared, int(max_l), _stream())
    _lib.check(rc, entry)
    return dx, dw


def tp_backward_sh(x, w_edge, src_sorted, dst_sorted, blocks, paths, max_mul: int, g_agg, avg_num_neighbors: float,
                   num_neigh=None, max_l: int = 4, sh_stride: int = SH_STRIDE) -> torch.Tensor:
    """the adjoint of the 'uvu' product w.r.t. the edge harmonics (include/matten_hip.h matten_tp_backward_sh; the tables
    of tp_backward_lit, max_mul = plan.bw_max_mul) -> dY [E, sh_stride] fp32, every column written"""
    lib = _lib.load()
    x = _need(x, torch.float32, "x")
    g_agg = _need(g_agg, torch.float32, "grad agg")
    w_edge = _edge_dtype(w_edge, "w_edge")
    E = w_edge.shape[0]
    dy = torch.empty(E, sh_stride, dtype=torch.float32, device=x.device)
    if num_neigh is not None:
        num_neigh = _need(num_neigh, torch.float32, "num_neigh")
    with _timed(f"tp_backward_sh/d_mid={g_agg.shape[1]}/d_in={x.shape[1]}"):
        rc = lib.matten_tp_backward_sh(_ptr(x), x.shape[1], _ptr(w_edge), w_edge.shape[1], _ptr(src_sorted), _ptr(dst_sorted),
                                       _ptr(blocks), blocks.shape[0], int(max_mul), _ptr(paths), paths.shape[0], _ptr(g_agg),
                                       g_agg.shape[1], float(avg_num_neighbors or 0.0), _ptr(num_neigh), E,
                                       int(w_edge.dtype == torch.bfloat16), _ptr(dy), sh_stride, int(max_l), _stream())
    _lib.check(rc, "matten_tp_backward_sh")
    return dy


def radial_mlp_bwd_len(geom_sorted, n_basis: int, r_start: float, r_end: float, w0p, w_mid, w2p, w_cols: int,
                       dw) -> torch.Tensor:
    """the adjoint of the radial MLP w.r.t. the edge length (matten_radial_mlp_bwd_len) -> dlen [E] fp32.
    w_mid: the packed middle layers, [n_mid, 32, 32] or one [32, 32] layer (any depth through the one entry)"""
    lib = _lib.load()
    geom_sorted = _need(geom_sorted, torch.float32, "geom_sorted")
    w0p, w2p = _need(w0p, torch.float32, "w0p"), _need(w2p, torch.float32, "w2p")
    w_mid, n_mid = _mid(w_mid.unsqueeze(0) if w_mid is not None and w_mid.dim() == 2 else w_mid, "w_mid")
    if dw.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError("dw must be fp32 or bf16")
    dw = _need(dw, dw.dtype, "dw")
    E = geom_sorted.shape[0]
    nb_pad, hidden = w0p.shape
    dlen = torch.empty(E, dtype=torch.float32, device=geom_sorted.device)
    with _timed(f"radial_mlp_bwd_len/w_pad={w2p.shape[1]}"):
        rc = lib.matten_radial_mlp_bwd_len(_ptr(geom_sorted), E, n_basis, r_start, r_end, _ptr(w0p), nb_pad,
                                           _ptr(w_mid) if n_mid else None, n_mid, _ptr(w2p), hidden, w2p.shape[1], int(w_cols),
                                           _ptr(dw), dw.shape[1], int(dw.dtype == torch.bfloat16), _ptr(dlen), _stream())
    _lib.check(rc, "matten_radial_mlp_bwd_len")
    return dlen


def edge_geom_bwd(geom_sorted, dy, dlen, lmax: int, n_nodes: int, rowptr, out_csr, perm=None, edge_cell_shift=None,
                  n_cells: int = 0, ptr=None):
    """the adjoint of edge_geom (matten_edge_geom_bwd) -> (dpos [N,3], dcell [n_cells,3,3] or None).
    dy [E, stride] / dlen [E]: dL/d(harmonics) and dL/d(length) summed over the conv layers, either may be None;
    out_csr = (out_ptr, out_perm) as tp_backward_lit takes it; n_cells > 0 with edge_cell_shift asks for dcell
    (ptr [n_cells+1] int64, the crystals' first atoms, when n_cells > 1)"""
    lib = _lib.load()
    geom_sorted = _need(geom_sorted, torch.float32, "geom_sorted")
    E, dev = geom_sorted.shape[0], geom_sorted.device
    dy = None if dy is None else _need(dy, torch.float32, "dy")
    dlen = None if dlen is None else _need(dlen, torch.float32, "dlen")
    rowptr = _need(rowptr, torch.int32, "rowptr")
    out_ptr, out_perm = (_need(t, torch.int32, n) for t, n in zip(out_csr, ("out_ptr", "out_perm")))
    dcell = None
    if n_cells > 0 and edge_cell_shift is not None:
        edge_cell_shift = _need(edge_cell_shift, torch.float32, "edge_cell_shift")
        perm = None if perm is None else _need(perm, torch.int32, "perm")
        if n_cells > 1:
            ptr = _need(ptr, torch.int64, "ptr")
        dcell = torch.empty(n_cells, 3, 3, dtype=torch.float32, device=dev)
    dv = torch.empty(E, 4, dtype=torch.float32, device=dev)
    dpos = torch.empty(n_nodes, 3, dtype=torch.float32, device=dev)
    with _timed("edge_geom_bwd"):
        rc = lib.matten_edge_geom_bwd(_ptr(geom_sorted), _ptr(dy), dy.shape[1] if dy is not None else 0, _ptr(dlen), int(lmax), E,
                                      n_nodes, _ptr(rowptr), _ptr(out_ptr), _ptr(out_perm), _ptr(perm), _ptr(edge_cell_shift),
                                      n_cells if dcell is not None else 0, _ptr(ptr), _ptr(dv), _ptr(dpos), _ptr(dcell), _stream())
    _lib.check(rc, "matten_edge_geom_bwd")
    return dpos, dcell


def species_linear_wgrad(x, dy, species_order, n_species: int, seg_tables, w_stride: int) -> torch.Tensor:
    lib = _lib.load()
    x = _need(x, torch.float32, "x")
    dy = _need(dy, torch.float32, "dy")
    order, seg = species_order if species_order is not None else (None, None)
    # every packed weight is written exactly once (nothing to pre-zero); large batches cut the species' rows into slices
    # (a compact list of (species, slice) items) whose partial sums the library adds in slice order
    n_scratch = lib.matten_species_linear_wgrad_scratch_floats(x.shape[0], n_species, w_stride)
    dwp = torch.empty(n_species, w_stride, dtype=torch.float32, device=x.device)
    partial = torch.empty(n_scratch, dtype=torch.float32, device=x.device) if n_scratch > 0 else None
    for segs in seg_tables:
        _lib.check(
            lib.matten_species_linear_wgrad(_ptr(x), x.shape[1], _ptr(dy), dy.shape[1], _ptr(order), _ptr(seg),
                                            n_species, x.shape[0], _ptr(segs), segs.shape[0], w_stride, _ptr(dwp),
                                            _ptr(partial), _stream()),
            "matten_species_linear_wgrad",
        )
    return dwp


def gate_bwd(x, meta, act_cst, dy) -> torch.Tensor:
    lib = _lib.load()
    x = _need(x, torch.float32, "x")
    dy = _need(dy, torch.float32, "dy")
    dx = torch.empty_like(x)   # every input column (scalars, gates, gated) is written exactly once
    _lib.check(lib.matten_gate_bwd(_ptr(x), x.shape[1], _ptr(meta), meta.shape[0], _ptr(act_cst), _ptr(dy), x.shape[0],
                                   _ptr(dx), _stream()), "matten_gate_bwd")
    return dx


def _bn_scratch(lib, x):
    """partial records of the two-stage whole-batch reductions (large batches only)"""
    n = lib.matten_bn_scratch_floats(x.shape[0], x.shape[1])
    return torch.empty(n, dtype=torch.float32, device=x.device) if n > 0 else None


def _bn_n_valid(n_valid, x):
    """the device word of the valid-rows entries: int64, on x's device, never read by the host"""
    if n_valid.dtype != torch.int64 or n_valid.device != x.device or n_valid.numel() < 1 or not n_valid.is_contiguous():
        raise ValueError(f"n_valid must be a contiguous int64 tensor on {x.device}, got {n_valid.dtype} {tuple(n_valid.shape)} "
                         f"on {n_valid.device}")
    return n_valid


def bn_train_fwd(x, col2chan, chan, weight, bias, eps: float, running_mean=None, running_var=None, momentum: float = 0.0,
                 n_valid=None):
    """batch statistics -> (y, mean, nu); running_mean / running_var (optional) are updated in place by the same launch.
    n_valid (optional, int64 on the device; its first element is read by the kernels): the statistics run over the rows
    [0, n_valid) only (a padded batch, matten_bn_train_fwd_valid)"""
    lib = _lib.load()
    x = _need(x, torch.float32, "x")
    C = chan.shape[0]
    mean = torch.empty(C, dtype=torch.float32, device=x.device)
    nu = torch.empty(C, dtype=torch.float32, device=x.device)
    y = torch.empty_like(x)
    if running_var is not None:
        running_mean = _need(running_mean, torch.float32, "running_mean")
        running_var = _need(running_var, torch.float32, "running_var")
    scratch = _bn_scratch(lib, x)
    args = [_ptr(x), x.shape[1], x.shape[0], _ptr(col2chan), _ptr(chan), C, _ptr(weight), _ptr(bias), eps, _ptr(mean), _ptr(nu),
            _ptr(y), _ptr(running_mean), _ptr(running_var), float(momentum), _ptr(scratch)]
    name = "matten_bn_train_fwd"
    if n_valid is not None:
        args.append(_ptr(_bn_n_valid(n_valid, x)))
        name += "_valid"
    _lib.check(getattr(lib, name)(*args, _stream()), name)
    if running_var is not None:
        bump_weights_epoch()   # the running statistics were updated through raw pointers (caches of the folded BatchNorm)
    return y, mean, nu


def norm_act(x, chan, act: int, epsilon: float = 1e-8, running_mean=None, running_var=None, bn_weight=None, bn_bias=None,
             bn_eps: float = 1e-5) -> torch.Tensor:
    """e3nn NormActivation (+ optional eval-mode BatchNorm), include/matten_hip.h matten_norm_act"""
    lib = _lib.load()
    x = _need(x, torch.float32, "x")
    y = torch.empty_like(x)
    _lib.check(lib.matten_norm_act(_ptr(x), x.shape[1], x.shape[0], _ptr(chan), chan.shape[0], int(act), float(epsilon),
                                   _ptr(running_mean), _ptr(running_var), _ptr(bn_weight), _ptr(bn_bias), float(bn_eps),
                                   _ptr(y), _stream()), "matten_norm_act")
    return y


def norm_act_bwd(x, dy, chan, act: int, epsilon: float = 1e-8) -> torch.Tensor:
    lib = _lib.load()
    dy = _need(dy, torch.float32, "dy")
    dx = torch.empty_like(x)
    _lib.check(lib.matten_norm_act_bwd(_ptr(x), _ptr(dy), x.shape[1], x.shape[0], _ptr(chan), chan.shape[0], int(act),
                                       float(epsilon), _ptr(dx), _stream()), "matten_norm_act_bwd")
    return dx


def _bn_eval_bwd_outputs(lib, x, n_cols: int, n_chan: int, n_bias: int, param_grads: bool):
    dx = torch.empty_like(x)   # every input column is written exactly once
    if not param_grads:
        return dx, None, None, None
    dweight = torch.empty(n_chan, dtype=torch.float32, device=x.device)
    dbias = torch.empty(n_bias, dtype=torch.float32, device=x.device)
    scratch = torch.empty(lib.matten_bn_eval_bwd_scratch_floats(x.shape[0], n_cols), dtype=torch.float32, device=x.device)
    return dx, dweight, dbias, scratch


def gate_bn_eval_bwd(x, meta, act_cst, bn_chan, running_mean, running_var, bn_weight, eps: float, dy, n_bias: int,
                     param_grads: bool = True):
    """adjoint of gate_bn WITH the running statistics (eval-mode BatchNorm) -> (dx, dweight [C], dbias [n_bias]);
    param_grads=False: (dx, None, None) from one launch (frozen affine)"""
    lib = _lib.load()
    x = _need(x, torch.float32, "x")
    dy = _need(dy, torch.float32, "dy")
    if x.shape[0] == 0:
        z = (lambda n: torch.zeros(n, dtype=torch.float32, device=x.device)) if param_grads else (lambda n: None)
        return torch.empty_like(x), z(bn_chan.shape[0]), z(n_bias)
    d_out, C = meta.shape[0], bn_chan.shape[0]
    dx, dweight, dbias, scratch = _bn_eval_bwd_outputs(lib, x, d_out, C, n_bias, param_grads)
    _lib.check(lib.matten_gate_bn_eval_bwd(_ptr(x), x.shape[1], _ptr(meta), d_out, _ptr(act_cst), _ptr(bn_chan), C,
                                           _ptr(running_mean), _ptr(running_var), _ptr(bn_weight), float(eps), _ptr(dy),
                                           x.shape[0], _ptr(dx), _ptr(dweight), _ptr(dbias), _ptr(scratch), _stream()),
               "matten_gate_bn_eval_bwd")
    return dx, dweight, dbias


def norm_act_bn_eval_bwd(x, dy, chan, act: int, epsilon: float, running_mean, running_var, bn_weight, bn_eps: float,
                         n_bias: int, param_grads: bool = True):
    """adjoint of norm_act WITH the running statistics (eval-mode BatchNorm) -> (dx, dweight [C], dbias [n_bias])"""
    lib = _lib.load()
    x = _need(x, torch.float32, "x")
    dy = _need(dy, torch.float32, "dy")
    C = chan.shape[0]
    if x.shape[0] == 0:
        z = (lambda n: torch.zeros(n, dtype=torch.float32, device=x.device)) if param_grads else (lambda n: None)
        return torch.empty_like(x), z(C), z(n_bias)
    dx, dweight, dbias, scratch = _bn_eval_bwd_outputs(lib, x, C, C, n_bias, param_grads)
    _lib.check(lib.matten_norm_act_bn_eval_bwd(_ptr(x), _ptr(dy), x.shape[1], x.shape[0], _ptr(chan), C, int(act),
                                               float(epsilon), _ptr(running_mean), _ptr(running_var), _ptr(bn_weight),
                                               float(bn_eps), _ptr(dx), _ptr(dweight), _ptr(dbias), _ptr(scratch),
                                               _stream()), "matten_norm_act_bn_eval_bwd")
    return dx, dweight, dbias


def instance_norm_fwd(x, seg_ptr, seg_of_row, col2chan, chan, weight, bias, eps: float):
    """per-crystal statistics (reference InstanceNorm, nn/utils.py:448-588) -> (y, mean [B, C], nu [B, C])"""
    lib = _lib.load()
    x = _need(x, torch.float32, "x")
    seg_ptr = _need(seg_ptr, torch.int64, "ptr")
    seg_of_row = _need(seg_of_row, torch.int64, "batch")
    C, B = chan.shape[0], seg_ptr.shape[0] - 1
    mean = torch.empty(B, C, dtype=torch.float32, device=x.device)
    nu = torch.empty(B, C, dtype=torch.float32, device=x.device)
    y = torch.empty_like(x)
    _lib.check(lib.matten_instance_norm_fwd(_ptr(x), x.shape[1], x.shape[0], _ptr(seg_ptr), _ptr(seg_of_row), B,
                                            _ptr(col2chan), _ptr(chan), C, _ptr(weight), _ptr(bias), eps, _ptr(mean),
                                            _ptr(nu), _ptr(y), _stream()), "matten_instance_norm_fwd")
    return y, mean, nu


def instance_norm_bwd(x, dy, seg_ptr, seg_of_row, col2chan, chan, mean, nu, weight, eps: float):
    lib = _lib.load()
    dy = _need(dy, torch.float32, "dy")
    B, C = mean.shape
    A = torch.empty(B, C, dtype=torch.float32, device=x.device)
    Bs = torch.empty(B, C, dtype=torch.float32, device=x.device)
    dx = torch.empty_like(x)
    _lib.check(lib.matten_instance_norm_bwd(_ptr(x), _ptr(dy), x.shape[1], x.shape[0], _ptr(seg_ptr), _ptr(seg_of_row), B,
                                            _ptr(col2chan), _ptr(chan), C, _ptr(mean), _ptr(nu), _ptr(weight), eps,
                                            _ptr(A), _ptr(Bs), _ptr(dx), _stream()), "matten_instance_norm_bwd")
    return dx, A, Bs


def bn_train_bwd(x, dy, col2chan, chan, mean, nu, weight, eps: float, n_bias: int, n_valid=None):
    """-> (dx, dweight [C], dbias [n_bias]): the parameter gradients come out of the reduction kernel itself.
    n_valid as in bn_train_fwd: the reductions over the valid rows, dx of the rows behind them exactly zero"""
    lib = _lib.load()
    dy = _need(dy, torch.float32, "dy")
    C = chan.shape[0]
    A = torch.empty(C, dtype=torch.float32, device=x.device)
    B = torch.empty(C, dtype=torch.float32, device=x.device)
    dweight = torch.empty(C, dtype=torch.float32, device=x.device)
    dbias = torch.empty(n_bias, dtype=torch.float32, device=x.device)
    dx = torch.empty_like(x)
    scratch = _bn_scratch(lib, x)
    args = [_ptr(x), _ptr(dy), x.shape[1], x.shape[0], _ptr(col2chan), _ptr(chan), C, _ptr(mean), _ptr(nu), _ptr(weight), eps,
            _ptr(A), _ptr(B), _ptr(dx), _ptr(dweight), _ptr(dbias), _ptr(scratch)]
    name = "matten_bn_train_bwd"
    if n_valid is not None:
        args.append(_ptr(_bn_n_valid(n_valid, x)))
        name += "_valid"
    _lib.check(getattr(lib, name)(*args, _stream()), name)
    return dx, dweight, dbias


def segment_reduce_bwd(dy, ptr, n_rows: int, mean: bool) -> torch.Tensor:
    lib = _lib.load()
    dy = _need(dy, torch.float32, "dy")
    ptr = _need(ptr, torch.int64, "ptr")
    dx = torch.zeros(n_rows, dy.shape[1], dtype=torch.float32, device=dy.device)
    _lib.check(lib.matten_segment_reduce_bwd(_ptr(dy), dy.shape[1], _ptr(ptr), dy.shape[0], int(mean), _ptr(dx),
                                             _stream()), "matten_segment_reduce_bwd")
    return dx


LOSS_KINDS = {"mse": 0, "l2": 0, "squared": 0, 0: 0, "mae": 1, "l1": 1, "absolute": 1, 1: 1}


def _selected_args(pred, target, selector, kind):
    if kind not in LOSS_KINDS or isinstance(kind, bool):
        raise ValueError(f"kind = {kind!r}: 0 / 'mse' (squared error) or 1 / 'mae' (absolute error)")
    pred = _need(pred, torch.float32, "pred")
    target = _need(target, torch.float32, "target")
    selector = _need(selector, torch.int32, "selector")
    if pred.dim() < 1 or selector.dim() != 1 or selector.shape[0] != pred.shape[0]:
        raise ValueError(f"selector {tuple(selector.shape)} does not hold one word per row of pred {tuple(pred.shape)}")
    if target.shape[0] != pred.shape[0] or target.numel() != pred.numel():
        raise ValueError(f"target {tuple(target.shape)} and pred {tuple(pred.shape)} differ: the dense per-atom layout keeps "
                         f"one target row per atom (zeros where the selector is 0)")
    n_rows = pred.shape[0]
    d = pred.numel() // n_rows if n_rows else max(1, int(np.prod(pred.shape[1:])))
    return pred, target, selector, n_rows, d, LOSS_KINDS[kind]


def selected_loss(pred, target, selector, kind=0):
    """mean of the per-element loss over the rows with selector != 0 (include/matten_hip.h: matten_selected_loss) ->
    (loss fp32 [], sum fp64 [], count int64 []), all on the device; trailing dimensions of pred / target are flattened"""
    lib = _lib.load()
    pred, target, selector, n_rows, d, kind = _selected_args(pred, target, selector, kind)
    dev = pred.device
    loss = torch.empty((), dtype=torch.float32, device=dev)
    total = torch.empty((), dtype=torch.float64, device=dev)
    count = torch.empty((), dtype=torch.int64, device=dev)
    nbytes = int(lib.matten_selected_loss_workspace_bytes(n_rows, d))
    ws = torch.empty(nbytes // 8, dtype=torch.int64, device=dev) if nbytes else None
    _lib.check(lib.matten_selected_loss(_ptr(pred), _ptr(target), _ptr(selector), n_rows, d, kind, _ptr(total), _ptr(count),
                                        _ptr(loss), _ptr(ws), nbytes, _stream()), "matten_selected_loss")
    return loss, total, count


def selected_loss_bwd(pred, target, selector, kind, g, count) -> torch.Tensor:
    """the adjoint of selected_loss with respect to pred; g (fp32 []) and count (int64 [], the forward's) stay on the device"""
    lib = _lib.load()
    pred, target, selector, n_rows, d, kind = _selected_args(pred, target, selector, kind)
    g = _need(g, torch.float32, "g")
    count = _need(count, torch.int64, "count")
    if g.numel() != 1 or count.numel() != 1:
        raise ValueError("g and count are one word each")
    grad = torch.empty_like(pred)
    _lib.check(lib.matten_selected_loss_bwd(_ptr(pred), _ptr(target), _ptr(selector), n_rows, d, kind, _ptr(g), _ptr(count),
                                            _ptr(grad), _stream()), "matten_selected_loss_bwd")
    return grad


def _valid_args(pred, target, n_valid, kind):
    if kind not in LOSS_KINDS or isinstance(kind, bool):
        raise ValueError(f"kind = {kind!r}: 0 / 'mse' (squared error) or 1 / 'mae' (absolute error)")
    pred = _need(pred, torch.float32, "pred")
    target = _need(target, torch.float32, "target")
    n_valid = _need(n_valid, torch.int64, "n_valid")
    if pred.dim() < 1 or n_valid.numel() != 1:
        raise ValueError(f"n_valid {tuple(n_valid.shape)} is not one int64 word (batch['_amd_n_valid'][2:3]) or pred "
                         f"{tuple(pred.shape)} has no rows")
    if target.shape[0] != pred.shape[0] or target.numel() != pred.numel():
        raise ValueError(f"target {tuple(target.shape)} and pred {tuple(pred.shape)} differ: a padded batch keeps one "
                         f"target row per crystal, padding crystals included")
    n_rows = pred.shape[0]
    d = pred.numel() // n_rows if n_rows else max(1, int(np.prod(pred.shape[1:])))
    return pred, target, n_valid, n_rows, d, LOSS_KINDS[kind]


def valid_loss(pred, target, n_valid, kind=0):
    """mean of the per-element loss over the rows [0, *n_valid) of a padded crystal batch, and the sums its metric keeps
    (include/matten_hip.h: matten_valid_loss) -> (loss fp32 [], sums fp64 [2] = (squared, absolute), count int64 []), all
    on the device; n_valid is a device word (``batch["_amd_n_valid"][2:3]``), clamped to [0, n_rows]"""
    lib = _lib.load()
    pred, target, n_valid, n_rows, d, kind = _valid_args(pred, target, n_valid, kind)
    dev = pred.device
    loss = torch.empty((), dtype=torch.float32, device=dev)
    sums = torch.empty(2, dtype=torch.float64, device=dev)
    count = torch.empty((), dtype=torch.int64, device=dev)
    nbytes = int(lib.matten_valid_loss_workspace_bytes(n_rows, d))
    ws = torch.empty(nbytes // 8, dtype=torch.int64, device=dev) if nbytes else None
    _lib.check(lib.matten_valid_loss(_ptr(pred), _ptr(target), _ptr(n_valid), n_rows, d, kind, _ptr(sums), _ptr(count),
                                     _ptr(loss), _ptr(ws), nbytes, _stream()), "matten_valid_loss")
    return loss, sums, count


def valid_loss_bwd(pred, target, n_valid, kind, g, count) -> torch.Tensor:
    """the adjoint of valid_loss with respect to pred; g (fp32 []) and count (int64 [], the forward's) stay on the device"""
    lib = _lib.load()
    pred, target, n_valid, n_rows, d, kind = _valid_args(pred, target, n_valid, kind)
    g = _need(g, torch.float32, "g")
    count = _need(count, torch.int64, "count")
    if g.numel() != 1 or count.numel() != 1:
        raise ValueError("g and count are one word each")
    grad = torch.empty_like(pred)
    _lib.check(lib.matten_valid_loss_bwd(_ptr(pred), _ptr(target), _ptr(n_valid), n_rows, d, kind, _ptr(g), _ptr(count),
                                         _ptr(grad), _stream()), "matten_valid_loss_bwd")
    return grad


def valid_loss_host(pred, target, n_valid: int, kind=0):
    """numpy fp64 restatement of valid_loss (what the tests hold the kernel to): pred / target array-likes [n_rows, ...],
    n_valid an integer -> (loss np.float32, sums np.float64 [2], count int).  Rows at or beyond n_valid are sliced away,
    whatever they hold."""
    if kind not in LOSS_KINDS or isinstance(kind, bool):
        raise ValueError(f"kind = {kind!r}: 0 / 'mse' (squared error) or 1 / 'mae' (absolute error)")
    p = np.asarray(pred, dtype=np.float64)
    t = np.asarray(target, dtype=np.float64)
    n_rows = p.shape[0]
    count = min(max(int(n_valid), 0), n_rows)
    x = p[:count] - t[:count]
    d = max(1, int(np.prod(p.shape[1:])))
    sums = np.array([np.sum(x * x), np.sum(np.abs(x))], dtype=np.float64)
    loss = np.float32(sums[LOSS_KINDS[kind]] / (count * d)) if count > 0 else np.float32(0.0)
    return loss, sums, count


def valid_loss_bwd_host(pred, target, n_valid: int, kind=0, g: float = 1.0):
    """numpy restatement of valid_loss_bwd: g * dl / (count * d) in fp64 on the valid rows, rounded once to fp32; +0.0 on
    every other row"""
    p = np.asarray(pred, dtype=np.float64)
    t = np.asarray(target, dtype=np.float64)
    n_rows = p.shape[0]
    count = min(max(int(n_valid), 0), n_rows)
    grad = np.zeros(p.shape, dtype=np.float32)
    if count > 0:
        x = p[:count] - t[:count]
        d = max(1, int(np.prod(p.shape[1:])))
        dl = 2.0 * x if LOSS_KINDS[kind] == 0 else np.sign(x)
        grad[:count] = (float(np.float32(g)) * dl / (float(count) * float(d))).astype(np.float32)
    return grad


def _need_out(t, dtype, numel: int, name: str, why: str = "") -> torch.Tensor:
    """an output tensor the caller allocated, checked: contiguous, of the size the kernel writes (rows of a larger buffer
    are fine: ``buf[:N]``)"""
    if _need(t, dtype, name) is not t or t.numel() != numel:
        raise ValueError(f"{name}: expected a contiguous {dtype} tensor of {numel} elements{why}")
    return t


def _prep_outputs(out, N: int, B: int, singular: bool, dev):
    """the outputs of graph_prep / graph_prep_pbc (+ singular): the caller's (``out=``), checked, or new ones"""
    names = ("frac", "bound", "batch", "pos32", "cell32") + (("singular",) if singular else ())
    want = ((torch.float64, (N, 3)), (torch.float64, (B, 3)), (torch.int64, (N,)), (torch.float32, (N, 3)),
            (torch.float32, (3 * B, 3)), (torch.int32, (B,)))[:len(names)]
    if out is None:
        return tuple(torch.empty(shape, dtype=dtype, device=dev) for dtype, shape in want)
    if len(out) != len(names):
        raise ValueError(f"out: expected the {len(names)} tensors {names}")
    return tuple(_need_out(t, dtype, int(np.prod(shape)), name) for t, name, (dtype, shape) in zip(out, names, want))


def _search_inputs(pos64, cell64, ptr, frac, bound, index, index_name: str):
    """what every route of the neighbour search takes, checked -> the six tensors in the order given (index: pair_ptr on
    the pair route, batch on the others) + (B, N, device)"""
    pos64 = _need(pos64, torch.float64, "pos")
    return (pos64, _need(cell64, torch.float64, "cell"), _need(ptr, torch.int64, "ptr"), _need(frac, torch.float64, "frac"),
            _need(bound, torch.float64, "bound"), _need(index, torch.int64, index_name), ptr.shape[0] - 1, pos64.shape[0],
            pos64.device)


def _edge_outputs(offsets, run_ptr, B: int, N: int, summary, search: bool = True):
    """The second half of every eager route, between its counting and its fill pass.  offsets: the scanned counts; run_ptr
    [B+1]: where each crystal's run starts in them; summary: an int64 tensor of two or more elements; search = False:
    nothing was counted, nothing is read back.  -> (E, min_edges, host, edge_index [2,E], shifts [E,3], num_neigh [N])
    through the one host sync of graph construction: the edge count sizes the outputs; the smallest edge count of a
    crystal (0: the caller has to find and report the edgeless ones) and whatever else ``summary`` holds ride on the same
    read-back, ``host``."""
    host = [0] * summary.numel()
    if search:
        _lib.check(_lib.load().matten_neighbor_summary(_ptr(offsets), _ptr(run_ptr), B, _ptr(summary), _stream()),
                   "matten_neighbor_summary")
        host = summary.tolist()
    E, min_edges, dev = host[0], int(host[1]), offsets.device
    edge_index = torch.empty(2, E, dtype=torch.int64, device=dev)
    shifts = torch.empty(E, 3, dtype=torch.float32, device=dev)
    num_neigh = torch.empty(N, dtype=torch.float32, device=dev)
    return E, min_edges, host, edge_index, shifts, num_neigh


def _edge_outputs_by_atom(counts, ptr, summary):
    """_edge_outputs for the routes that count per centre atom (rows, cells): crystals are runs of atoms, as they are runs
    of pairs on the pair route, so ptr takes pair_ptr's place.  -> offsets [N+1] i64 + _edge_outputs' results"""
    N, dev = counts.shape[0], counts.device
    offsets = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    torch.cumsum(counts, 0, dtype=torch.int64, out=offsets[1:])
    if summary is None:
        summary = torch.zeros(3, dtype=torch.int64, device=dev)
    return (offsets,) + _edge_outputs(offsets, ptr, ptr.shape[0] - 1, N, summary, search=N > 0)


def graph_prep(pos64, cell64, ptr, r_cut: float, out=None):
    """per-crystal prologue of the device graph builder (include/matten_hip.h matten_graph_prep)
    -> (frac [N,3] f64, bound [B,3] f64, batch [N] i64, pos [N,3] f32, cell [3B,3] f32); ``out``: these five, allocated by
    the caller, are written in place (a loop that rebuilds the same atoms: data.rebuild.GeometryBatch)"""
    lib = _lib.load()
    pos64 = _need(pos64, torch.float64, "pos")
    cell64 = _need(cell64, torch.float64, "cell")
    ptr = _need(ptr, torch.int64, "ptr")
    B = ptr.shape[0] - 1
    frac, bound, batch, pos32, cell32 = outs = _prep_outputs(out, pos64.shape[0], B, False, pos64.device)
    _lib.check(lib.matten_graph_prep(_ptr(pos64), _ptr(cell64), _ptr(ptr), B, float(r_cut), _ptr(frac), _ptr(bound),
                                     _ptr(batch), _ptr(pos32), _ptr(cell32), _stream()), "matten_graph_prep")
    return outs


def neighbor_list(pos64, cell64, ptr, frac, bound, pair_ptr, r_cut: float, max_atoms: int, n_pairs: int, want_csr: bool = True):
    """see neighbor_list_flagged, which this is without the prologue's flags: -> its first six results"""
    return neighbor_list_flagged(pos64, cell64, ptr, frac, bound, pair_ptr, r_cut, max_atoms, n_pairs, want_csr)[:6]


def neighbor_list_flagged(pos64, cell64, ptr, frac, bound, pair_ptr, r_cut: float, max_atoms: int, n_pairs: int,
                          want_csr: bool = True, summary: torch.Tensor = None):
    """Periodic neighbour list of a batch of crystals, canonical (i, j, Sx, Sy, Sz) order.
    frac / bound: ops.graph_prep; pair_ptr[B+1] = running sum of n_b^2 (ordered pairs numbered crystal by crystal,
    i-major), n_pairs = pair_ptr[B].
    -> (edge_index [2,E] i64 (global ids), edge_cell_shift [E,3] f32, num_neigh [N] f32 (edges per centre atom),
        pair_offsets [n_pairs+1] i64, smallest edge count of a crystal: an int, read back together with the edge count,
        csr = (perm [E] i32, rowptr [N+1] i32, src_sorted [E] i32) -- the destination-sorted view ops.csr_build would derive
        from edge_index, bit for bit -- or None)
    summary (optional): an int64 tensor of more than two elements whose first two receive the read-back; the others
    (flags of the prologue, e.g. graph_prep_pbc's n_singular) cross in the same copy.  The read-back as a host list is
    the seventh result, always (as in neighbor_list_rows)."""
    lib = _lib.load()
    pos64, cell64, ptr, frac, bound, pair_ptr, B, N, dev = _search_inputs(pos64, cell64, ptr, frac, bound, pair_ptr, "pair_ptr")
    # i-major counts in the first half, the same counts numbered j-major in the second: ONE scan serves both orders
    counts = torch.empty((2 if want_csr else 1) * n_pairs, dtype=torch.int32, device=dev)
    with _timed("neighbor_count"):
        _lib.check(
            lib.matten_neighbor_count(_ptr(pos64), _ptr(cell64), _ptr(ptr), _ptr(frac), _ptr(bound), _ptr(pair_ptr),
                                      float(r_cut), B, int(max_atoms), _ptr(counts),
                                      counts.data_ptr() + 4 * n_pairs if (want_csr and n_pairs) else None, _stream()),
            "matten_neighbor_count",
        )
    scan = torch.zeros(counts.numel() + 1, dtype=torch.int64, device=dev)
    torch.cumsum(counts, 0, dtype=torch.int64, out=scan[1:])
    offsets = scan[: n_pairs + 1]
    if summary is None:
        summary = torch.empty(2, dtype=torch.int64, device=dev)
    E, min_edges, host, edge_index, shifts, num_neigh = _edge_outputs(offsets, pair_ptr, B, N, summary, search=n_pairs > 0)
    csr = offsets_t = None
    if want_csr and n_pairs and E < 2 ** 31:
        offsets_t = scan[n_pairs:]               # the j-major half of the scan (starts at E: the kernel subtracts it)
        csr = (torch.empty(E, dtype=torch.int32, device=dev), torch.empty(N + 1, dtype=torch.int32, device=dev),
               torch.empty(E, dtype=torch.int32, device=dev))
    with _timed("neighbor_fill"):
        _lib.check(
            lib.matten_neighbor_fill(_ptr(pos64), _ptr(cell64), _ptr(ptr), _ptr(frac), _ptr(bound), _ptr(pair_ptr),
                                     float(r_cut), B, int(max_atoms), _ptr(offsets), E, _ptr(edge_index), _ptr(shifts),
                                     _ptr(num_neigh), _ptr(offsets_t), N, _ptr(csr[1]) if csr else None,
                                     _ptr(csr[2]) if csr else None, _ptr(csr[0]) if csr else None, _stream()),
            "matten_neighbor_fill",
        )
    return edge_index, shifts, num_neigh, offsets, min_edges, csr, host


def neighbor_list_capped(pos64, cell64, ptr, frac, bound, pair_ptr, r_cut: float, max_atoms: int, n_pairs: int, capacity,
                         edge_index, edge_cell_shift, num_neigh, perm, rowptr, src_sorted, n_valid, flags,
                         counts=None, scan=None, singular=None):
    """neighbor_list_flagged into the caller's buffers of fixed ``capacity`` = (N_b, E_b, B_b), with the edge count left on
    the device (include/matten_hip.h matten_neighbor_fill_capped): nothing is read back and nothing is sized by device
    data, so the call captures into a hipGraph.  Outputs (all written in place, the padded layout of
    ``GraphStoreHost.padded_reference``): edge_index [2,E_b] i64, edge_cell_shift [E_b,3] f32, num_neigh [N_b] f32,
    perm [E_b] / rowptr [N_b+1] / src_sorted [E_b] i32, n_valid [3] i64 = (N, E, B); flags: an int32 element the
    MATTEN_CAPPED_* bits are OR-ed into (1: E > E_b and NOTHING else was written, 2: a crystal without any edge,
    4: a singular periodic cell, from ``singular`` = graph_prep_pbc's output).  counts [2 n_pairs] i32 / scan
    [2 n_pairs + 1] i64: scratch the caller may keep between calls.  -> scan (scan[n_pairs] is E, scan[pair_ptr] the
    first edge of each crystal)."""
    lib = _lib.load()
    pos64, cell64, ptr, frac, bound, pair_ptr, B, N, dev = _search_inputs(pos64, cell64, ptr, frac, bound, pair_ptr, "pair_ptr")
    n_b, e_b, b_b = (int(v) for v in capacity)
    for name, t, dtype, numel in (("edge_index", edge_index, torch.int64, 2 * e_b),
                                  ("edge_cell_shift", edge_cell_shift, torch.float32, 3 * e_b),
                                  ("num_neigh", num_neigh, torch.float32, n_b), ("perm", perm, torch.int32, e_b),
                                  ("rowptr", rowptr, torch.int32, n_b + 1), ("src_sorted", src_sorted, torch.int32, e_b),
                                  ("n_valid", n_valid, torch.int64, 3), ("flags", flags, torch.int32, 1)):
        _need_out(t, dtype, numel, name, f" for capacity {(n_b, e_b, b_b)}")
    if counts is None:
        counts = torch.empty(2 * n_pairs, dtype=torch.int32, device=dev)
    if scan is None:
        scan = torch.empty(2 * n_pairs + 1, dtype=torch.int64, device=dev)
    counts, scan = _need(counts, torch.int32, "counts"), _need(scan, torch.int64, "scan")
    if counts.numel() != 2 * n_pairs or scan.numel() != 2 * n_pairs + 1 or n_pairs <= 0:
        raise ValueError(f"counts / scan: expected {2 * n_pairs} and {2 * n_pairs + 1} elements for {n_pairs} > 0 pairs")
    if singular is not None:
        singular = _need(singular, torch.int32, "singular")
    stream = _stream()
    _lib.check(lib.matten_neighbor_count(_ptr(pos64), _ptr(cell64), _ptr(ptr), _ptr(frac), _ptr(bound), _ptr(pair_ptr),
                                         float(r_cut), B, int(max_atoms), _ptr(counts), counts.data_ptr() + 4 * n_pairs,
                                         stream), "matten_neighbor_count")
    _lib.check(lib.matten_neighbor_scan(_ptr(counts), 2 * n_pairs, _ptr(scan), stream), "matten_neighbor_scan")
    _lib.check(lib.matten_neighbor_fill_capped(
        _ptr(pos64), _ptr(cell64), _ptr(ptr), _ptr(frac), _ptr(bound), _ptr(pair_ptr), float(r_cut), B, int(max_atoms),
        _ptr(scan), scan.data_ptr() + 8 * n_pairs, N, _ptr(singular), n_b, e_b, b_b, _ptr(edge_index), _ptr(edge_cell_shift),
        _ptr(num_neigh), _ptr(rowptr), _ptr(src_sorted), _ptr(perm), _ptr(n_valid), _ptr(flags), stream),
        "matten_neighbor_fill_capped")
    return scan


def graph_prep_pbc(pos64, cell64, ptr, pbc, r_cut: float, n_singular: torch.Tensor, out=None):
    """graph_prep for open / partly periodic crystals (include/matten_hip.h matten_graph_prep_pbc): pbc [B,3] uint8.
    -> graph_prep's five outputs + singular [B] i32 (1: the periodic vectors of that crystal are linearly dependent).
    n_singular: a zeroed int64 element that receives the number of such crystals (the caller reads it back with the
    edge count: see neighbor_list_flagged(summary=)).  ``out``: the six outputs, allocated by the caller (see graph_prep)."""
    lib = _lib.load()
    pos64 = _need(pos64, torch.float64, "pos")
    cell64 = _need(cell64, torch.float64, "cell")
    ptr = _need(ptr, torch.int64, "ptr")
    pbc = _need(pbc, torch.uint8, "pbc")
    B = ptr.shape[0] - 1
    if pbc.numel() != 3 * B or n_singular.dtype != torch.int64 or n_singular.numel() != 1:
        raise ValueError("pbc must hold [B,3] flags, n_singular one int64")
    frac, bound, batch, pos32, cell32, singular = outs = _prep_outputs(out, pos64.shape[0], B, True, pos64.device)
    _lib.check(lib.matten_graph_prep_pbc(_ptr(pos64), _ptr(cell64), _ptr(ptr), _ptr(pbc), B, float(r_cut), _ptr(frac),
                                         _ptr(bound), _ptr(batch), _ptr(pos32), _ptr(cell32), _ptr(singular),
                                         n_singular.data_ptr(), _stream()), "matten_graph_prep_pbc")
    return outs


def neighbor_list_rows(pos64, cell64, ptr, batch, frac, bound, r_cut: float, summary: torch.Tensor = None):
    """The same list as neighbor_list without per-pair bookkeeping (matten_neighbor_rows_count / _fill: one wave per
    centre atom, O(N) scratch): for large structures.  batch / frac / bound: ops.graph_prep.
    -> (edge_index [2,E] i64, edge_cell_shift [E,3] f32, num_neigh [N] f32, offsets [N+1] i64 (first edge of each centre
        atom), smallest edge count of a crystal, summary [3] i64 on the host).  No CSR on this route (ops.csr_build)."""
    lib = _lib.load()
    pos64, cell64, ptr, frac, bound, batch, B, N, dev = _search_inputs(pos64, cell64, ptr, frac, bound, batch, "batch")
    search = (_ptr(pos64), _ptr(cell64), _ptr(ptr), _ptr(batch), _ptr(frac), _ptr(bound), float(r_cut), N)
    counts = torch.empty(N, dtype=torch.int32, device=dev)
    with _timed("neighbor_rows_count"):
        _lib.check(lib.matten_neighbor_rows_count(*search, _ptr(counts), _stream()), "matten_neighbor_rows_count")
    offsets, E, min_edges, host, edge_index, shifts, num_neigh = _edge_outputs_by_atom(counts, ptr, summary)
    with _timed("neighbor_rows_fill"):
        _lib.check(lib.matten_neighbor_rows_fill(*search, _ptr(offsets), E, _ptr(edge_index), _ptr(shifts), _ptr(num_neigh),
                                                 _stream()), "matten_neighbor_rows_fill")
    return edge_index, shifts, num_neigh, offsets, min_edges, host


def neighbor_cells_row_capacity() -> int:
    """neighbouring atoms of a centre atom that the cells route's fill pass ranks in LDS; a longer row is walked as on the
    rows route (matten_neighbor_cells_row_capacity)"""
    return int(_lib.load().matten_neighbor_cells_row_capacity())


def neighbor_list_cells(pos64, cell64, ptr, batch, frac, bound, r_cut: float, summary: torch.Tensor = None, pbc=None,
                        singular=None):
    """neighbor_list_rows with a cell list in front (matten_neighbor_cells_grid / _bin / _scatter / _count / _fill): a
    centre atom tests the atoms of at most 27 bins instead of its whole structure, which makes the search linear in the
    number of atoms.  The same arguments, the same results bit for bit and the same one read-back as neighbor_list_rows;
    pbc [B,3] uint8 and singular [B] i32 are ops.graph_prep_pbc's (None: every axis periodic).  Scratch is O(N): about
    65 bytes per atom."""
    lib = _lib.load()
    pos64, cell64, ptr, frac, bound, batch, B, N, dev = _search_inputs(pos64, cell64, ptr, frac, bound, batch, "batch")
    if pbc is not None:
        pbc = _need(pbc, torch.uint8, "pbc")
    if singular is not None:
        singular = _need(singular, torch.int32, "singular")
    if (pbc is not None and pbc.numel() != 3 * B) or (singular is not None and singular.numel() != B):
        raise ValueError("pbc must hold [B,3] flags, singular [B]")
    grid = torch.empty(B, 8, dtype=torch.int32, device=dev)
    grid_f = torch.empty(B, 16, dtype=torch.float64, device=dev)
    bin_base = torch.zeros(B + 1, dtype=torch.int64, device=dev)
    n_bins = torch.empty(B, dtype=torch.int64, device=dev)
    with _timed("neighbor_cells_bin"):
        _lib.check(lib.matten_neighbor_cells_grid(_ptr(pos64), _ptr(cell64), _ptr(ptr), _ptr(bound), _ptr(pbc), _ptr(singular),
                                                  B, float(r_cut), _ptr(grid), _ptr(grid_f), _ptr(n_bins), _stream()),
                   "matten_neighbor_cells_grid")
        torch.cumsum(n_bins, 0, out=bin_base[1:])
        # a structure has at most as many bins as atoms (one when it is empty): N + B bounds their number without a read-back
        bin_count = torch.zeros(N + B, dtype=torch.int32, device=dev)
        bin_start = torch.zeros(N + B + 1, dtype=torch.int32, device=dev)
        bin_of = torch.empty(N, dtype=torch.int32, device=dev)
        slot_atom = torch.empty(N, dtype=torch.int32, device=dev)
        _lib.check(lib.matten_neighbor_cells_bin(_ptr(pos64), _ptr(frac), _ptr(batch), _ptr(grid), _ptr(grid_f), _ptr(bin_base),
                                                 N, _ptr(bin_of), _ptr(bin_count), _stream()), "matten_neighbor_cells_bin")
        torch.cumsum(bin_count, 0, dtype=torch.int32, out=bin_start[1:])
        _lib.check(lib.matten_neighbor_cells_scatter(_ptr(batch), _ptr(bin_base), _ptr(bin_of), _ptr(bin_start), N,
                                                     _ptr(bin_count), _ptr(slot_atom), _stream()),
                   "matten_neighbor_cells_scatter")
    del bin_count, n_bins, grid_f
    search = (_ptr(pos64), _ptr(cell64), _ptr(ptr), _ptr(batch), _ptr(frac), _ptr(bound), _ptr(grid), _ptr(bin_base),
              _ptr(bin_of), _ptr(bin_start), _ptr(slot_atom), float(r_cut), N)
    counts = torch.empty(N, dtype=torch.int32, device=dev)
    with _timed("neighbor_cells_count"):
        _lib.check(lib.matten_neighbor_cells_count(*search, _ptr(counts), _stream()), "matten_neighbor_cells_count")
    offsets, E, min_edges, host, edge_index, shifts, num_neigh = _edge_outputs_by_atom(counts, ptr, summary)
    with _timed("neighbor_cells_fill"):
        _lib.check(lib.matten_neighbor_cells_fill(*search, _ptr(offsets), E, _ptr(edge_index), _ptr(shifts), _ptr(num_neigh),
                                                  _stream()), "matten_neighbor_cells_fill")
    return edge_index, shifts, num_neigh, offsets, min_edges, host
