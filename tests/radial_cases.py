"""Cases, inputs and references for the radial-MLP kernels (csrc/radial_mlp.hip: radial_mlp_kernel; csrc/tp_fused.hip:
radial_hidden_kernel, radial_hidden_multi_kernel; csrc/radial_mlp_bwd.hip: radial_mlp_bwd_edges + radial_mlp_bwd_w2,
radial_mlp_bwd_fused and the operand packers), planned with no GPU and shared by test_radial_kernels_host.py (the plan,
the references and the constants) and test_gpu_radial_kernels.py (the kernels).

Reference (one function of dtype, `reference`): the oracle's soft_one_hot_linspace(len, r_start, r_end, nb, "bessel", True)
* sqrt(nb), silu layers with normalize2mom_const("silu") on the raw weights / sqrt(fan_in) -- the arithmetic of
test_gpu_radial_depth.py.  fp64 autograd of it is what the kernels are compared with; the same function in fp32 is the
baseline of the bounds: for each quantity CONSTANTS holds the worst, over the cases of this file, of
    |fp32 reference - fp64 reference|.max() / |fp64 reference|.max()     over the block compared
(the rows of a length band for the forward quantities, the whole matrix for a weight gradient) and a kernel may be
FACTOR = 4 times that far from fp64 (another summation order, FMA contraction -- not other arithmetic).

Length bands by t = (len - r_start) / (r_end - r_start): near_start 0 < t < 0.05, mid 0.05 <= t < 0.9, near_end
0.9 <= t < 1.  Rows with t <= 0 or t >= 1 are outside the support: the reference is exactly zero there and so must the
kernels' outputs be.  A row of length exactly r_start (0/0 in the reference) is left out of every comparison; it is planted
once in every case of 16 edges or more and nothing else is ever left out.

`python tests/radial_cases.py` recomputes and prints the constants; the figures printed for the committed cases:
    w/near_start 7.559e-07   w/mid 7.272e-07   w/near_end 3.170e-06   w/all 7.559e-07
    h/near_start 5.780e-07   h/mid 1.365e-06   h/near_end 6.820e-06
    dW0 1.507e-06   dWmid0 1.950e-06   dWmid1 1.186e-06   dWmid2 7.745e-07   dW2 1.372e-06
(CONSTANTS holds them rounded up by about 1.3; the host test keeps every committed value within [1, 2] x the recomputed
figure.  The near-end figures are the largest because the reference features are about 20 times smaller there while the
fp32 argument of sin(pi (k+1) t) is rounded at the size of (k+1) pi.)
"""
import functools
import os
import sys
import zlib
from dataclasses import dataclass
from typing import Dict

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FACTOR = 4.0
HID = 32
NB_CYCLE = (3, 8, 12, 16)                 # nb_pad 4, 8, 12, 16: KS0 = 1, 2, 3, 4
R_CYCLE = ((0.0, 5.0), (0.5, 4.0))
BANDS = (("near_start", 0.0, 0.05), ("mid", 0.05, 0.9), ("near_end", 0.9, 1.0))
TWO_KERNEL = 0                            # form: 0 = radial_mlp_bwd_edges + radial_mlp_bwd_w2, else the fused kernel's chunks

# ---- the weight adjoint's dispatch, spelled out -------------------------------------------------------------------------
# radial_mlp_bwd.hip: bw_fused(w_pad, n_mid) = 128 <= w_pad <= 64 * fu_maxch(n_mid), fu_maxch = {0: 6, 1: 8, 2: 4, 3: 0};
# launch_bwd_fused takes the smallest of 4 / 6 / 8 chunks per wave with w_pad <= 64 * chunks.
GRID_W = {112: 100, 128: 128, 256: 256, 272: 260, 384: 377, 400: 390, 512: 500, 528: 520}     # w_pad -> W
EXPECTED_FORM = {
    # w_pad: (n_mid = 0, 1, 2, 3)
    112: (0, 0, 0, 0),
    128: (4, 4, 4, 0),
    256: (4, 4, 4, 0),
    272: (6, 6, 0, 0),
    384: (6, 6, 0, 0),
    400: (0, 8, 0, 0),
    512: (0, 8, 0, 0),
    528: (0, 0, 0, 0),
    # the widths of the edge-count cases
    48: (0, 0, 0, 0),
    224: (4, 4, 4, 0),
    336: (6, 6, 0, 0),
}


def dispatch_rule(w_pad: int, n_mid: int) -> int:
    """the rule of bw_fused / launch_bwd_fused restated (the host test holds EXPECTED_FORM against it)"""
    maxch = {0: 6, 1: 8, 2: 4, 3: 0}[n_mid]
    if not 128 <= w_pad <= 64 * maxch:
        return TWO_KERNEL
    return next(ch for ch in (4, 6, 8) if ch <= maxch and w_pad <= 64 * ch)


def bw_tiles(E: int) -> int:
    """16-edge tiles (rounds) per wave of the weight adjoint"""
    return min(8, max(1, E // (16 * 2048)))


def small_slices(E: int) -> int:
    return -(-(-(-E // (16 * bw_tiles(E)))) // 4) * 4


@dataclass(frozen=True)
class Case:
    name: str
    group: str
    E: int
    W: int
    n_mid: int
    nb: int
    r_start: float
    r_end: float
    weight_gain: float = 1.0          # multiplies the hidden layers' raw weights (h_scale < 1 at 1e3)
    adjoint: bool = True
    storage: bool = False             # also run with bf16 dw and with dw_ld = w_pad + 16

    @property
    def w_pad(self) -> int:
        return (self.W + 15) // 16 * 16

    @property
    def nb_pad(self) -> int:
        return (self.nb + 3) // 4 * 4

    @property
    def form(self) -> int:
        return EXPECTED_FORM[self.w_pad][self.n_mid]

    @property
    def seed(self) -> int:
        return zlib.crc32(self.name.encode()) & 0x7fffffff


def build_cases() -> Dict[str, Case]:
    c: Dict[str, Case] = {}

    def add(case):
        assert case.name not in c
        c[case.name] = case

    # 1. dispatch grid at 67 edges (four full tiles + three edges: a full workgroup, then one whose waves 1..3 are idle);
    #    nb and the radial range cycle along the diagonals of the grid so that neither is tied to a width or a depth
    storage_grid = {(128, 2), (400, 1), (112, 0), (528, 3)}       # two per form
    for iw, (w_pad, W) in enumerate(GRID_W.items()):
        for n_mid in range(4):
            nb = NB_CYCLE[(iw + n_mid) % 4]
            r_start, r_end = R_CYCLE[(iw // 2 + n_mid) % 2]
            add(Case(f"grid/w{w_pad}/m{n_mid}", "grid", 67, W, n_mid, nb, r_start, r_end,
                     storage=(w_pad, n_mid) in storage_grid))
    # 2. edge counts
    i = 0
    for W in (43, 216):
        for E in (1, 15, 16, 17, 64, 65):
            add(Case(f"edges/E{E}/w{(W + 15) // 16 * 16}", "edges", E, W, 1, NB_CYCLE[i % 4], *R_CYCLE[(i // 2) % 2]))
            i += 1
    add(Case("edges/E65535/w48", "edges", 65535, 48, 1, 8, 0.0, 5.0))
    add(Case("edges/E65536/w48", "edges", 65536, 48, 1, 12, 0.5, 4.0))
    add(Case("rounds/m2/w224", "rounds", 70001, 216, 2, 12, 0.5, 4.0, storage=True))
    add(Case("rounds/m0/w336", "rounds", 70001, 330, 0, 3, 0.0, 5.0, storage=True))
    add(Case("rounds/m1/w400", "rounds", 70001, 390, 1, 16, 0.5, 4.0, storage=True))
    # 5. hidden layers x 1e3: h_scale < 1, the lo-flush of the split in units of 1 / h_scale (forward only)
    add(Case("gain1e3/m1", "gain", 67, 100, 1, 8, 0.5, 4.0, weight_gain=1e3, adjoint=False))
    add(Case("gain1e3/m2", "gain", 67, 100, 2, 12, 0.0, 5.0, weight_gain=1e3, adjoint=False))
    return c


CASES = build_cases()
ADJOINT_CASES = tuple(n for n, c in CASES.items() if c.adjoint)
STORAGE_CASES = tuple(n for n, c in CASES.items() if c.storage)
STORAGE_FORMS = (("bf16", 0), ("fp32", 16), ("bf16", 16))            # (dw dtype, dw_ld - w_pad) beyond the plain (fp32, 0) run
# radial_hidden_multi_deep with 1, 4 and 8 MLPs: every depth, every KS0, both NT-independent tails, one large case
MULTI_CASES = ("grid/w112/m0", "grid/w128/m1", "grid/w256/m2", "grid/w272/m3", "edges/E17/w48", "edges/E65536/w48",
               "gain1e3/m1")
MULTI_COUNTS = (1, 4, 8)
NAN_EMPTY_CASES = ("grid/w400/m1", "grid/w112/m0")        # one per form
NON_DEEP_CASE = "grid/w272/m1"


def multi_h_scale(j: int) -> float:
    """the (power of two) output scale MLP j of a multi launch is given: distinct per MLP"""
    return 2.0 ** -j


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def planted_lengths(case: Case):
    """-> list of (name, fp32 value) planted in a case of 16 edges or more: the issue's six (five at r_start = 0), the
    excluded length r_start itself, and two fillers per band so that each band has three rows whatever the seed"""
    rs, re = case.r_start, case.r_end
    c = re - rs
    p = [("at_end", re), ("far", re + 1.5), ("start+1e-3", rs + 1e-3), ("start+0.01", rs + 0.01), ("end-1e-3", re - 1e-3)]
    if rs > 0:
        p.append(("below_start", rs - 0.2))
    p.append(("at_start", rs))
    p += [("fill/near_start", rs + 0.03 * c), ("fill/near_end0", re - 0.03 * c), ("fill/near_end1", re - 0.07 * c),
          ("fill/mid0", rs + 0.3 * c), ("fill/mid1", rs + 0.55 * c), ("fill/mid2", rs + 0.8 * c)]
    return p


def planted_rows(case: Case):
    """row of each planted length: spread evenly, so that on the large cases they fall in different workgroups, the last
    (ragged) one included"""
    p = planted_lengths(case)
    n, E = len(p), case.E
    rows = [min(E - 1, (j * E) // n + E // (2 * n)) for j in range(n - 1)] + [E - 1]
    assert len(set(rows)) == n
    return {name: r for (name, _), r in zip(p, rows)}


def make_lengths(case: Case) -> torch.Tensor:
    g = torch.Generator().manual_seed(case.seed)
    c = case.r_end - case.r_start
    lens = (case.r_start + torch.rand(case.E, generator=g, dtype=torch.float64) * 1.08 * c).float()
    if case.E == 1:       # a single edge in the middle of the range: one random row would set the scale of its whole band
        lens[0] = case.r_start + 0.4 * c
    if case.E >= 16:
        rows = planted_rows(case)
        for name, v in planted_lengths(case):
            lens[rows[name]] = v
    return lens


def make_weights(case: Case, mlp: int = 0):
    """raw layers (w0 [nb, 32], wm [n_mid, 32, 32], w2 [32, W]) of MLP `mlp` of the case, randn"""
    g = torch.Generator().manual_seed(case.seed + 7919 * (mlp + 1))
    w0 = torch.randn(case.nb, HID, generator=g) * case.weight_gain
    wm = torch.randn(case.n_mid, HID, HID, generator=g) * case.weight_gain
    w2 = torch.randn(HID, case.W, generator=g)
    return w0, wm, w2


def act_cst() -> float:
    from matten_amd.nn._activation import normalize2mom_const

    return normalize2mom_const("silu")


def scales(case: Case):
    """what the packers multiply the raw layers by"""
    c = act_cst()
    return (1.0 / case.nb**0.5, c / HID**0.5, c / HID**0.5)


def reference(case: Case, lens, w0, wm, w2, dtype, gouts=()):
    """-> (w [E, W], last hidden layer [E, 32] (before its activation constant, as the kernels hold it), and per gout the
    weight gradients [dW0, dWmid_0.., dW2]) in `dtype`.  `lens` are the fp32 lengths the kernels see."""
    from oracle.e3nn_lite.math import soft_one_hot_linspace

    c = act_cst()
    ws = [w.to(dtype).requires_grad_(bool(gouts)) for w in (w0, *wm.unbind(0), w2)]
    x = soft_one_hot_linspace(lens.to(dtype), case.r_start, case.r_end, case.nb, "bessel", True) * case.nb**0.5
    a = torch.nn.functional.silu(x @ (ws[0] / case.nb**0.5))
    for w in ws[1:-1]:
        a = torch.nn.functional.silu((a * c) @ (w / HID**0.5))
    out = (a * c) @ (ws[-1] / HID**0.5)
    grads = []
    for i, g in enumerate(gouts):
        grads.append([t.detach() for t in torch.autograd.grad(out, ws, grad_outputs=g.to(dtype),
                                                              retain_graph=i + 1 < len(gouts))])
    return out.detach(), a.detach(), grads


GRAD_KEYS = ("dW0", "dWmid0", "dWmid1", "dWmid2", "dW2")


def grad_names(n_mid: int):
    return ["dW0"] + [f"dWmid{i}" for i in range(n_mid)] + ["dW2"]


def _ratio(a32, a64) -> float:
    return float((a32.double() - a64).abs().max() / a64.abs().max())


class Problem:
    """inputs and references of one (case, MLP); nothing here is modified after construction"""

    def __init__(self, case: Case, mlp: int = 0):
        self.case, self.mlp = case, mlp
        self.lens = make_lengths(case)
        self.w0, self.wm, self.w2 = make_weights(case, mlp)
        t = (self.lens.double() - case.r_start) / (case.r_end - case.r_start)
        self.t = t
        self.excluded = torch.nonzero(self.lens == case.r_start).flatten()          # 0/0 in the reference
        self.outside = torch.nonzero((t <= 0) | (t >= 1)).flatten()
        self.bands = {name: torch.nonzero((t > 0) & (t >= lo) & (t < hi)).flatten() for name, lo, hi in BANDS}
        self.compared = torch.nonzero(self.lens != case.r_start).flatten()
        # the reference of an excluded row is evaluated outside the support: a zero row that adds nothing to a gradient,
        # which is what the kernels make of it (their basis is 0 where 0 < len - r_start does not hold)
        lens_ref = torch.where(self.lens == case.r_start, torch.full_like(self.lens, case.r_end + 1.0), self.lens)
        adjoint = case.adjoint and mlp == 0
        gouts = ()
        if adjoint:
            g = torch.Generator().manual_seed(case.seed + 1)
            self.gout = torch.randn(case.E, case.W, generator=g)
            gouts = (self.gout,) + ((self.gout.bfloat16().float(),) if case.storage else ())
        w64, h64, g64 = reference(case, lens_ref, self.w0, self.wm, self.w2, torch.float64, gouts)
        w32, h32, g32 = reference(case, lens_ref, self.w0, self.wm, self.w2, torch.float32, gouts)
        self.h = h64
        self.w = w64 if mlp == 0 else None                # (the further MLPs of a multi launch: hidden layers only)
        self.grads = dict(zip(("fp32", "bf16"), g64))     # by the dtype dw is stored in
        # fp32-torch distance from fp64 per quantity: what CONSTANTS is the worst of
        r: Dict[str, float] = {}
        for name, rows in self.bands.items():
            if rows.numel():
                r[f"h/{name}"] = _ratio(h32[rows], h64[rows])
                if mlp == 0:
                    r[f"w/{name}"] = _ratio(w32[rows], w64[rows])
        if mlp == 0:
            r["w/all"] = _ratio(w32, w64)
        for a, b in zip(g32, g64):
            for key, x32, x64 in zip(grad_names(case.n_mid), a, b):
                r[key] = max(r.get(key, 0.0), _ratio(x32, x64))
        self.ratios = r

    def band_scale(self, ref, name: str) -> float:
        return float(ref[self.bands[name]].abs().max())


@functools.lru_cache(maxsize=None)
def problem(name: str, mlp: int = 0) -> Problem:
    return Problem(CASES[name], mlp)


def all_problems():
    """every (case, MLP) the GPU file compares with a reference"""
    for name in CASES:
        yield problem(name)
    for name in MULTI_CASES:
        for j in range(1, max(MULTI_COUNTS)):
            yield problem(name, j)


def recompute_constants() -> Dict[str, float]:
    worst: Dict[str, float] = {}
    for p in all_problems():
        for k, v in p.ratios.items():
            worst[k] = max(worst.get(k, 0.0), v)
    return worst


# worst fp32-torch / fp64 distance per quantity over the cases above, rounded up (python tests/radial_cases.py)
CONSTANTS = {
    "w/near_start": 9.8e-7, "w/mid": 9.4e-7, "w/near_end": 4.1e-6, "w/all": 9.8e-7,
    "h/near_start": 7.5e-7, "h/mid": 1.8e-6, "h/near_end": 8.8e-6,
    "dW0": 2.0e-6, "dWmid0": 2.5e-6, "dWmid1": 1.5e-6, "dWmid2": 1.0e-6, "dW2": 1.8e-6,
}


def allowed(key: str, scale: float) -> float:
    return FACTOR * CONSTANTS[key] * scale


# ---- the split fp16 form of the hidden layer ----------------------------------------------------------------------------------
# h2s [E, 2, 32] fp16: column g * 8 + kk of either half holds feature 16 (kk >> 2) + 4 g + (kk & 3)
H2S_PERM = torch.tensor([16 * (kk >> 2) + 4 * g + (kk & 3) for g in range(4) for kk in range(8)])


def decode_h2s(h2s: torch.Tensor) -> torch.Tensor:
    """-> the 32 features in natural order, fp64 (hi + lo / 2048)"""
    v = h2s[:, 0].double() + h2s[:, 1].double() / 2048.0
    out = torch.empty_like(v)
    out[:, H2S_PERM.to(v.device)] = v
    return out


def split_format_term(v_abs: torch.Tensor) -> torch.Tensor:
    """|decode(split(v)) - v| <= 2^-22 |v| + 2^-25, from split_f16 (tp_walk.h) and the decode hi + lo / 2048:
    hi = fp16(v), 11 significant bits: |v - hi| <= 2^-11 |v| (hi = 0 below the fp16 minimum normal 2^-14: then the residual
    is v itself); lo = fp16(2^11 (v - hi)), again 11 bits: 2^-11 * 2^-11 |v| after the division by 2^11 -- or, where
    |v| < 2^-14, 2^-11 |v| < 2^-25; a lo below 2^-14 is flushed to zero: at most 2^-14 / 2^11 = 2^-25.
    v = h_scale[0] * h: in units of h the floor is 2^-25 / h_scale[0]."""
    return 2.0**-22 * v_abs + 2.0**-25


# ---- packers: a synthetic fused-column plan -----------------------------------------------------------------------------------
PACK_W, PACK_NB = 77, 12          # raw last-layer columns, basis functions
PACK_N_COLS = 59                  # fused columns: no multiple of 16 -> w_pad = 64 + 16


def pack_plan():
    """-> (cols int64 [59]: a permutation of a subset of the 77 raw columns, none repeated, seven structural zeros (-1);
    group_entries int32 [5, 32] with fields 5, 6, 7 = w_base, a_tile, n_mt: entries at bases that are no multiple of 16,
    one merged second-half record (field 0 < 0: no tiles) and a last entry whose last tile reaches past the last column)"""
    g = torch.Generator().manual_seed(5)
    cols = torch.randperm(PACK_W, generator=g)[:PACK_N_COLS].clone()
    cols[torch.tensor([0, 5, 16, 17, 31, 47, 58])] = -1
    w_pad = (PACK_N_COLS + 15) // 16 * 16 + 16
    ent = torch.zeros(5, 32, dtype=torch.int32)
    a_tile = 0
    for i, (w_base, n_mt, first) in enumerate(((0, 1, 0), (16, 2, 0), (37, 1, 0), (0, 0, -1), (48, 2, 0))):
        ent[i, 0], ent[i, 5], ent[i, 6], ent[i, 7] = first, w_base, a_tile, n_mt
        a_tile += n_mt
    assert 48 + 16 > PACK_N_COLS and 48 + 32 == w_pad      # the last tile lies wholly in the pad
    return cols, ent, a_tile, w_pad


if __name__ == "__main__":
    got = recompute_constants()
    for k in sorted(got):
        print(f"    {k:16s} {got[k]:.3e}" + (f"   committed {CONSTANTS[k]:.1e}" if k in CONSTANTS else ""))
