"""Cases for the two species-linear kernels (matten_species_linear: register-streaming, csrc/species_linear.hip;
matten_species_linear_rows: LDS-resident, csrc/species_linear_rows.hip), planned with no GPU and shared by
test_species_linear_host.py (routing and branch coverage) and test_gpu_species_linear.py (the kernels).

Per case: inputs built once and write-protected, the oracle's FullyConnectedTensorProduct(x, one_hot(species)) (or o3.Linear
for the plain-linear cases) holding the same flat weight in fp64 and fp32 -- the plan's tables are under test, so no
reference reads them -- and an INTEGER TWIN as in selfcheck._case: x in [-2, 2], weights in [-1, 1] (packed through the
plan's gather WITHOUT the path normalisation), addend in [-3, 3]; every partial sum stays below 2^24, so the fp32 result
is exact in any summation order and the expected values are int64 arithmetic over the irreps (not over the plan)."""
import functools
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from matten_amd import ops, plan as mplan

RTOL = 2e-6    # test_species_linear_shape_sweep's bound, here per (irrep block, species)


def ir(l: int) -> str:
    return f"{l}{'e' if l % 2 == 0 else 'o'}"


def steps_per_chunk(d: int, nb: int = 10) -> int:
    """16-channel steps per chunk of the streaming kernel (species_linear.hip: SL_NB = 10 loads per lane and chunk)"""
    return max(1, nb // d)


CHUNK_CHANNELS = {d: 16 * steps_per_chunk(d) for d in (1, 3, 5, 7, 9)}
assert CHUNK_CHANNELS == {1: 160, 3: 48, 5: 32, 7: 16, 9: 16}


@dataclass(frozen=True)
class Case:
    family: str
    irreps_in: str
    irreps_out: str
    S: Optional[int]                  # None: plain linear (species_order=None, reference o3.Linear)
    counts: Tuple[int, ...]           # rows per species (one entry for a plain linear)
    variants: Tuple[str, ...]         # kernels the case is run on ("rows" only where species_linear_route says "rows")
    adds: Tuple[bool, ...] = (False, True)
    reverse: bool = False             # rows of every species in descending node order
    seg_rotate: int = 0               # rotate the rows of the (single) segment table: segments of a pass are independent

    @property
    def n_rows(self) -> int:
        return int(sum(self.counts))


def _spread(n_rows: int, S: int, seed: int) -> Tuple[int, ...]:
    """ragged species groups as selfcheck._case makes them: a third of the rows in species 0, the rest at random"""
    sp = np.random.default_rng(seed).integers(0, S, n_rows)
    sp[: n_rows // 3] = 0
    return tuple(int(c) for c in np.bincount(sp, minlength=S))


OUT_MO = (1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 79, 80, 81, 144, 145)
OUT_MI = {0: 8, 1: 5, 2: 3, 3: 2, 4: 2}
BLOCK_WALK = ("3x0e+2x1o+1x2e+1x3o+1x4e", "17x0e+2x1o+1x1e+1x2e+1x3o+1x4e")   # 30 + 47 floats per row; 1x1e has no input
SPECIES_PAIR = ("8x0e+5x1o+3x2e", "17x0e+4x1o+3x2e")
GROUP_SIZES = (0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129)
W_LDS_BELOW, W_LDS_ABOVE = ("346x0e", "88x0e"), ("350x0e", "88x0e")        # w_stride 30448 / 30800 around 30464 floats
ROWS_ODD_MAX, ROWS_EVEN_MAX, ROWS_OVER = 781, 780, 782                      # d_in of "Kx0e -> 1x0e" around the 52 KB rule


def input_mis(d: int) -> Tuple[int, ...]:
    c = CHUNK_CHANNELS[d]
    return tuple(sorted({1, 15, 16, 17, c - 1, c, c + 1, 2 * c - 1, 2 * c, 2 * c + 1, 321}))


def _s70_counts() -> Tuple[int, ...]:
    """70 species (more than one wave scans): the twelve group sizes on species spread over both scan chunks, species 5
    and 69 empty (as in test_species_linear_gradients_vs_oracle_autograd), every other species one to three rows"""
    counts = [1 + (s % 3) for s in range(70)]
    for s, n in zip((0, 3, 6, 9, 17, 31, 33, 47, 63, 64, 66, 69), GROUP_SIZES[1:] + (0,)):
        counts[s] = n
    counts[5] = 0
    return tuple(counts)


def build_cases() -> Dict[str, Case]:
    c: Dict[str, Case] = {}
    both, stream = ("rows", "stream"), ("stream",)
    # -- output tiles (streaming forced): the d = 1 members with an addend are the miscompile family of species_linear.hip
    for l in range(5):
        for mo in OUT_MO:
            c[f"out/l{l}/mo{mo}"] = Case("out_tiles", f"{OUT_MI[l]}x{ir(l)}", f"{mo}x{ir(l)}", 2, _spread(37, 2, mo), stream)
    # -- input chunks (streaming forced)
    for l in range(5):
        for mi in input_mis(2 * l + 1):
            c[f"in/l{l}/mi{mi}"] = Case("in_chunks", f"{mi}x{ir(l)}", f"5x{ir(l)}", 3, _spread(50, 3, mi), stream)
    # -- block walk (streaming forced): 37 rows = one irrep block per blockIdx.y; the two large ones are filled in by
    #    block_walk_cases(threshold) because their row count comes from the library's accessor
    c["walk/n37"] = Case("block_walk", *BLOCK_WALK, 3, _spread(37, 3, 1), stream)
    c["walk/n37/empty_mid"] = Case("block_walk", *BLOCK_WALK, 3, _spread(37, 3, 1), stream, seg_rotate=3)
    # -- species and row tiles (both kernels)
    c["species/S70"] = Case("species", *SPECIES_PAIR, 70, _s70_counts(), both, reverse=True)
    for i in range(4):
        c[f"species/S3/{i}"] = Case("species", *SPECIES_PAIR, 3, GROUP_SIZES[3 * i:3 * i + 3], both, reverse=bool(i % 2))
    c["species/S1/n129"] = Case("species", *SPECIES_PAIR, 1, (129,), both, reverse=True)
    c["species/S1/n1"] = Case("species", *SPECIES_PAIR, 1, (1,), both)
    c["species/S3/n1"] = Case("species", *SPECIES_PAIR, 3, (0, 1, 0), both)
    # -- A operand in LDS against global memory (streaming)
    c["w_lds/below"] = Case("w_lds", *W_LDS_BELOW, 2, _spread(37, 2, 2), stream)
    c["w_lds/above"] = Case("w_lds", *W_LDS_ABOVE, 2, _spread(37, 2, 3), stream)
    # -- rows-kernel capacity
    for k in (ROWS_ODD_MAX, ROWS_EVEN_MAX):
        c[f"rows_cap/din{k}"] = Case("rows_cap", f"{k}x0e", "1x0e", 2, (20, 17), ("rows",))
    for k in (256, 257):
        c[f"rows_cap/din{k}"] = Case("rows_cap", f"{k}x0e", "3x0e", 2, (20, 17), ("rows",))
    c["rows_cap/w15"] = Case("rows_cap", "5x0e", "3x0e", 3, (9, 20, 8), ("rows",))        # w_stride % 4 = 3: scalar copy
    for mi in (0, 1, 4, 5, 8, 9):
        iin = "2x0e" if mi == 0 else f"2x0e+{mi}x1o"
        c[f"rows_cap/mul_in{mi}"] = Case("rows_cap", iin, "3x0e+2x1o", 2, (20, 17), ("rows",))
    for n_items in (1, 3, 4, 5):
        c[f"rows_cap/items{n_items}"] = Case("rows_cap", "4x0e", f"{16 * n_items}x0e", 2, (20, 17), ("rows",))
    # -- strided addend (both kernels): see dev_add("slice") of the GPU file
    c["strided_add"] = Case("strided_add", *SPECIES_PAIR, 3, (17, 0, 33), both, adds=(True,))
    c["strided_add/walk"] = Case("strided_add", *BLOCK_WALK, 3, _spread(37, 3, 4), both, adds=(True,))
    # -- plain linear (both kernels)
    for n in (1, 16, 129):
        c[f"plain/n{n}"] = Case("plain", *SPECIES_PAIR, None, (n,), both)
    # -- uncovered irreps: 2x2e of the output has no input path (forward); 2x2e of the input feeds no output (dx)
    c["uncovered/out"] = Case("uncovered", "4x0e+3x1o", "5x0e+2x2e+3x1o", 2, (20, 17), both)
    c["uncovered/in"] = Case("uncovered", "4x0e+2x2e+3x1o", "5x0e+3x1o", 2, (20, 17), both)
    # -- several passes: two input blocks of one irrep feed one output block (forward), two output blocks read one input
    #    block (adjoint); only the streaming kernel takes more than one segment table
    c["passes/fctp"] = Case("passes", "2x0e+1x1o+3x0e", "3x0e+2x1o+1x0e", 2, (20, 17), stream)
    c["passes/plain"] = Case("passes", "2x0e+3x0e", "3x0e", None, (37,), stream)
    return c


CASES = build_cases()
ADJOINT_CASES = ("walk/n37", "species/S70", "uncovered/in", "passes/fctp")


def walk_rows(threshold: int, S: int = 3) -> Tuple[int, int]:
    """(smallest N with cdiv(N, 64) + S >= threshold, the largest N one workgroup below)"""
    tiles = threshold - S
    return 64 * (tiles - 1) + 1, 64 * (tiles - 1)


def block_walk_cases(threshold: int) -> Dict[str, Case]:
    n_at, n_below = walk_rows(threshold)
    return {
        "walk/at": Case("block_walk", *BLOCK_WALK, 3, _spread(n_at, 3, 5), ("stream",)),
        "walk/at/empty_mid": Case("block_walk", *BLOCK_WALK, 3, _spread(n_at, 3, 5), ("stream",), seg_rotate=3),
        "walk/below": Case("block_walk", *BLOCK_WALK, 3, _spread(n_below, 3, 6), ("stream",)),
    }


# ---- planning and routing ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def plan_of(case: Case) -> "mplan.LinearPlan":
    if case.S is None:
        return mplan.plan_linear(case.irreps_in, case.irreps_out)
    return mplan.plan_fctp(case.irreps_in, case.S, case.irreps_out)


def seg_tables(case: Case, transposed: bool = False):
    """the pass tables handed to the kernel (seg_rotate applied to a single-pass table)"""
    lp = plan_of(case)
    tabs = [np.ascontiguousarray(t) for t in (lp.passes_t if transposed else lp.passes)]
    if case.seg_rotate:
        assert len(tabs) == 1 and not transposed
        tabs = [np.ascontiguousarray(np.roll(tabs[0], case.seg_rotate, axis=0))]
    return tabs


def route(case: Case, transposed: bool = False) -> str:
    lp = plan_of(case)
    tabs = lp.passes_t if transposed else lp.passes
    return ops.species_linear_route(lp.d_out if transposed else lp.d_in, lp.w_stride, [len(t) for t in tabs])


def rows_lds_bytes(case: Case) -> int:
    """what matten_species_linear_rows compares with its limit"""
    lp = plan_of(case)
    assert len(lp.passes) == 1
    return 4 * (16 * (lp.d_in | 1) + ((lp.w_stride + 3) & ~3) + 8 * len(lp.passes[0]))


def stream_blocks(case: Case) -> int:
    """matten_species_linear's workgroups along x: cdiv(N, 64) + S (no species term for a plain linear)"""
    return -(-case.n_rows // 64) + (case.S or 0)


def irrep_blocks(irreps):
    out, off = [], 0
    for i, (mul, irr) in enumerate(irreps):
        out.append((off, off + mul * irr.dim, f"{i}:{mul}x{irr}"))
        off += mul * irr.dim
    return [b for b in out if b[1] > b[0]]


def order_seg(species, S, reverse=False):
    species = np.asarray(species)
    order = np.argsort(species, kind="stable")
    seg = np.concatenate([[0], np.cumsum(np.bincount(species, minlength=S))])
    if reverse and len(order):
        order = np.concatenate([order[seg[s]:seg[s + 1]][::-1] for s in range(S)])
    return order.astype(np.int32), seg.astype(np.int32)


# ---- references ---------------------------------------------------------------------------------------------------------
def oracle_module(case: Case, w, dtype):
    from oracle.e3nn_lite import o3 as ro3

    if case.S is None:
        ref = ro3.Linear(case.irreps_in, case.irreps_out)
    else:
        ref = ro3.FullyConnectedTensorProduct(case.irreps_in, f"{case.S}x0e", case.irreps_out)
    ref = ref.to(dtype)
    with torch.no_grad():
        assert ref.weight.numel() == len(w), (case, ref.weight.numel(), len(w))
        ref.weight.copy_(torch.from_numpy(np.array(w)).to(dtype))
    return ref


def oracle_apply(case: Case, ref, x, species, dtype):
    if case.S is None:
        return ref(x)
    return ref(x, torch.nn.functional.one_hot(torch.from_numpy(np.array(species)).long(), case.S).to(dtype))


def integer_expected(case: Case, xi, wi_flat, species, addi=None):
    """int64 evaluation over the irreps: instructions in the reference's order (for i_in, for i_out, equal irrep), flat
    weight block [mul_in, S, mul_out]; no normalisation (the integer twin packs the raw weights)"""
    from matten_amd.o3 import Irreps

    ii, io = Irreps(case.irreps_in), Irreps(case.irreps_out)
    if case.S is not None:
        ii, io = ii.simplify(), io.simplify()
    S, N = case.S or 1, xi.shape[0]
    xo, oo = ii.offsets(), io.offsets()
    out = np.zeros((N, io.dim), dtype=np.int64) if addi is None else addi.astype(np.int64).copy()
    flat = 0
    for a, (mi, ia) in enumerate(ii):
        for b, (mo, ib) in enumerate(io):
            if ia != ib:
                continue
            d = ia.dim
            W = wi_flat[flat:flat + mi * S * mo].astype(np.int64).reshape(mi, S, mo)[:, species, :]   # [mi, N, mo]
            X = xi[:, xo[a]:xo[a] + mi * d].astype(np.int64).reshape(N, mi, d)
            out[:, oo[b]:oo[b] + mo * d] += np.einsum("unv,num->nvm", W, X).reshape(N, mo * d)
            flat += mi * S * mo
    assert flat == len(wi_flat)
    return out


class Problem:
    """inputs, packed weights and references of one case; nothing here is modified after construction"""

    def __init__(self, case: Case, seed: int = 0, adjoint: bool = False):
        self.case, self.plan = case, plan_of(case)
        lp, S = self.plan, case.S or 1
        rng = np.random.default_rng(seed)
        self.species = rng.permutation(np.repeat(np.arange(S), case.counts)).astype(np.int64)
        N = self.N = len(self.species)
        self.x = rng.standard_normal((N, lp.d_in)).astype(np.float32)
        self.w = rng.standard_normal(lp.weight_numel).astype(np.float32)
        self.add = rng.standard_normal((N, lp.d_out)).astype(np.float32)
        self.wp = (self.w[lp.gather] * lp.scale[None, :].astype(np.float32)).astype(np.float32)   # SpeciesLinear._pack
        self.xi = rng.integers(-2, 3, (N, lp.d_in)).astype(np.float32)
        self.wi = rng.integers(-1, 2, lp.weight_numel).astype(np.float32)
        self.addi = rng.integers(-3, 4, (N, lp.d_out)).astype(np.float32)
        self.wpi = self.wi[lp.gather].astype(np.float32)
        self.want_int = integer_expected(case, self.xi, self.wi, self.species)
        with torch.no_grad():
            self.want64, self.want32 = (
                oracle_apply(case, oracle_module(case, self.w, dt), torch.from_numpy(self.x).to(dt), self.species, dt)
                for dt in (torch.float64, torch.float32))
        if adjoint:
            self.gy = rng.standard_normal((N, lp.d_out)).astype(np.float32)
            self.grads = {}
            for dt in (torch.float64, torch.float32):
                ref = oracle_module(case, self.w, dt)
                xr = torch.from_numpy(self.x).to(dt).requires_grad_(True)
                oracle_apply(case, ref, xr, self.species, dt).backward(torch.from_numpy(self.gy).to(dt))
                self.grads[dt] = (xr.grad.detach(), ref.weight.grad.detach())
            self.gy.setflags(write=False)
        for a in (self.species, self.x, self.w, self.add, self.wp, self.xi, self.wi, self.addi, self.wpi, self.want_int):
            a.setflags(write=False)

    def refs(self, add: bool):
        """(fp64 reference, the oracle in fp32) of the forward (+ addend)"""
        if not add:
            return self.want64, self.want32
        a = torch.from_numpy(np.array(self.add))
        return self.want64 + a.double(), self.want32 + a

    def int_refs(self, add: bool) -> np.ndarray:
        return (self.want_int + (self.addi.astype(np.int64) if add else 0)).astype(np.float32)

    def order(self):
        if self.case.S is None:
            return None
        return order_seg(self.species, self.case.S, self.case.reverse)

    def weight_blocks(self):
        """per (instruction path, species): index arrays into the flat weight [mul_in, S, mul_out] of the path"""
        lp, S = self.plan, self.case.S or 1
        res = {}
        for (i_in, i_out, off, n) in lp.instr:
            mi, mo = lp.irreps_in[i_in].mul, lp.irreps_out[i_out].mul
            assert n == mi * S * mo
            idx = off + np.arange(n).reshape(mi, S, mo)
            for s in range(S):
                res[(f"{i_in}->{i_out}", s)] = idx[:, s, :].reshape(-1)
        return res


@functools.lru_cache(maxsize=None)
def problem(name: str, threshold: int = 0, adjoint: bool = False) -> Problem:
    case = CASES[name] if name in CASES else block_walk_cases(threshold)[name]
    return Problem(case, seed=len(name), adjoint=adjoint)


# ---- the error measure ----------------------------------------------------------------------------------------------------
def block_errors(got, want64, want32, species, blocks, rtol=RTOL):
    """per block and per species -> (max |got - fp64|, allowed, block maximum) with allowed = max(rtol x the block's
    maximum over the species' rows, 4 x the fp32 oracle's own distance from the fp64 one there); a block whose reference
    is identically zero allows nothing: it must be exactly zero"""
    got, want64, want32 = (np.asarray(t, dtype=np.float64) for t in (got, want64, want32))
    assert got.shape == want64.shape == want32.shape, (got.shape, want64.shape, want32.shape)
    assert blocks[-1][1] == want64.shape[1]
    res = {}
    for s in np.unique(species):
        rows = np.nonzero(np.asarray(species) == s)[0]
        for lo, hi, name in blocks:
            ref = want64[rows, lo:hi]
            scale = np.abs(ref).max()
            d32 = np.abs(want32[rows, lo:hi] - ref).max()
            allowed = max(rtol * scale, 4.0 * d32) if scale > 0 else 0.0
            res[(name, int(s))] = (np.abs(got[rows, lo:hi] - ref).max(), allowed, scale)
    return res


def vector_errors(got, want64, want32, groups, rtol=RTOL):
    """the same rule over index groups of a flat vector (the weight gradient per instruction path and species)"""
    got, want64, want32 = (np.asarray(t, dtype=np.float64).reshape(-1) for t in (got, want64, want32))
    res = {}
    for key, idx in groups.items():
        ref = want64[idx]
        scale = np.abs(ref).max()
        d32 = np.abs(want32[idx] - ref).max()
        res[key] = (np.abs(got[idx] - ref).max(), max(rtol * scale, 4.0 * d32) if scale > 0 else 0.0, scale)
    return res
