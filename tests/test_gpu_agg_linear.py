"""matten_agg_linear / matten_agg_linear_gate (csrc/agg_linear.hip) called directly, per output irrep block and per
species against the oracle in fp64: the single-layer cases, inputs and references of agg_linear_cases.py (the
component-major row holds NaN wherever no group entry writes; the buffer ops allocates for the result is NaN before
every launch of this module).

Tolerance (no new number): per block and per species the kernel may be max(2e-6 x the block's maximum, 4 x the fp32
oracle's own distance from the fp64 one) away from the fp64 reference -- 2e-6 is test_species_linear_shape_sweep's bound,
the second term the want64 rule of test_gpu_parity.close_blocks.

Worst measured |kernel - fp64| / block maximum over all blocks, species and row patterns, MI355X (fraction of the
allowed distance in brackets):
  lin2       paper_like 3.8e-7 (0.19)   wide_scalars 5.4e-7 (0.27)   mo17 2.4e-7 (0.12)   mo33 2.8e-7 (0.14)
             mo12_d3 2.6e-7 (0.13)   K_small 1.0e-7 (0.05)   K_big 8.8e-7 (0.35)   odd 1.9e-7 (0.09)   tiny 9.5e-8 (0.05)
             lds_79k 9.2e-7 (0.40)   species scans (S = 4400, 73) 5.5e-8 (0.03)
  gate (+bn) paper_like 2.3e-7 (0.11)   gates_65 2.1e-7 (0.11)   gates_33 2.1e-7 (0.10)   gates_25 1.7e-7 (0.08)
             odd_scalars 1.7e-7 (0.08)   no_scalars 1.9e-7 (0.10)   scalars_only 1.8e-7 (0.09)   tiny 1.7e-7 (0.09)
  controls   one weight off by 1e-3: 3.7e-4 (183 x allowed)   two slots swapped: 3.1e-3 (1528 x allowed)
(the fp32 oracle itself sits at up to 0.25 of the allowed distance by construction; K_big / lds_79k sum 224 to 352 terms)
"""
import functools

import numpy as np
import pytest
import torch

import agg_linear_cases as alc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _dev(a, device=DEV):
    """a (write-protected) numpy array as a tensor: a copy, so that the shared inputs stay as they were made"""
    return torch.from_numpy(np.array(a)).to(device)


ONE_ROWS = (1, 16, 129)     # the single-species entry (species_order=None)


@pytest.fixture(autouse=True)
def nan_empty(monkeypatch):
    """every float buffer torch.empty hands out on the device starts as NaN (the style of MATTEN_TEST_NAN_EMPTY, for this
    module only): an output element the kernel does not write fails the comparison instead of passing by chance"""
    _empty = torch.empty

    def empty(*a, **k):
        t = _empty(*a, **k)
        return t.fill_(float("nan")) if t.is_floating_point() and t.device.type == "cuda" else t

    monkeypatch.setattr(torch, "empty", empty)


# ---- one problem per (case, rows): inputs and the lin2 references, computed once and never modified ---------------------
class Problem:
    def __init__(self, lay, species, seed=0):
        self.lay, self.species = lay, np.asarray(species)
        self.N = len(species)
        self.agg, self.w = alc.make_inputs(lay, species, seed)
        self.row, _ = alc.scatter_rows(lay, self.agg)
        self.wtab = alc.make_wtab(lay.ap, self.w)
        self.lin64 = alc.reference_lin2(lay, self.agg, species, self.w, torch.float64)
        self.lin32 = alc.reference_lin2(lay, self.agg, species, self.w, torch.float32)
        rng = np.random.default_rng(seed + 1)
        self.add = rng.standard_normal((self.N, lay.ap.d_out)).astype(np.float32)   # the self-connection
        for a in (self.agg, self.w, self.row, self.wtab, self.add, self.species):
            a.setflags(write=False)

    def order(self, reverse=False):
        if self.lay.S == 1:
            return None
        return tuple(_dev(t) for t in alc.order_seg(self.species, self.lay.S, reverse))

    def tables(self):
        ap = self.lay.ap
        return _dev(ap.io_table), _dev(ap.blocks)

    def lin2_refs(self, add=False):
        """(fp64 reference, the oracle in fp32) of lin2 (+ addend)"""
        if not add:
            return self.lin64, self.lin32
        a = _dev(self.add, "cpu")
        return self.lin64 + a.double(), self.lin32 + a

    def gate_refs(self, bn=None):
        """the same through the oracle's Gate (+ BatchNorm), the self-connection added in front of it"""
        import copy

        lay, (x64, x32) = self.lay, self.lin2_refs(add=True)
        with torch.no_grad():
            x64, x32 = alc.oracle_gate(lay).double()(x64), alc.oracle_gate(lay)(x32)
            if bn is not None:
                x64, x32 = copy.deepcopy(bn).double()(x64), bn(x32)
        return x64, x32


@functools.lru_cache(maxsize=None)
def problem(name, pattern, gated=False) -> Problem:
    if isinstance(pattern, int):      # `one`: N rows of a single species
        return Problem(alc.layer(name, 1, gated), np.zeros(pattern, dtype=np.int64))
    counts = alc.ROW_PATTERNS[pattern]
    return Problem(alc.layer(name, len(counts), gated), alc.species_rows(counts))


def run_lin2(p: Problem, add=None, row=None, wtab=None, order="sorted"):
    from matten_amd import ops

    io, blk = p.tables()
    row = _dev(p.row if row is None else row)
    wtab = _dev(p.wtab if wtab is None else wtab)
    return ops.agg_linear(row, p.order() if order == "sorted" else order, wtab, io, blk, p.lay.ap.d_out, add=add)


def run_gate(p: Problem, add, bn=None, row=None, order="sorted"):
    from matten_amd import ops
    from matten_amd.nn._activation import act_const_table

    lay = p.lay
    io, blk = p.tables()
    scale = shift = None
    if bn is not None:
        scale, shift = (t.to(DEV) for t in alc.fold_batchnorm(lay, bn))
    return ops.agg_linear_gate(_dev(p.row if row is None else row),
                               p.order() if order == "sorted" else order, _dev(p.wtab), io, blk,
                               lay.ap.d_out, _dev(lay.cmeta), act_const_table().to(DEV),
                               lay.gate.irreps_out.dim, add=add, bn_scale=scale, bn_shift=shift)


def failures(got, want64, want32, species, irreps, what=""):
    """{(block, species)} outside the module's tolerance; prints the worst ratios (kept in the module docstring)"""
    got = got.detach().cpu()
    assert torch.isfinite(got).all(), f"{what}: {int((~torch.isfinite(got)).sum())} output elements are not finite"
    res = alc.block_errors(got.numpy(), want64.numpy(), want32.numpy(), species, alc.irrep_blocks(irreps))
    rel = max(res.items(), key=lambda kv: kv[1][0] / kv[1][2])
    frac = max(res.items(), key=lambda kv: kv[1][0] / kv[1][1])
    print(f"agg_linear ratio {what}: worst |err| / block max {rel[1][0] / rel[1][2]:.2e} at {rel[0]}, "
          f"worst fraction of the allowed distance {frac[1][0] / frac[1][1]:.2f} at {frac[0]}")
    return {k: v for k, v in res.items() if not v[0] <= v[1]}


def dev_add(p: Problem, how):
    """None / contiguous / a column slice of a wider buffer whose other columns are NaN (production: both[:, d1:])"""
    if how is None:
        return None
    a = _dev(p.add)
    if how == "contiguous":
        return a
    d = a.shape[1]
    wide = torch.full((p.N, d + 37), float("nan"), device=DEV)
    wide[:, 24:24 + d] = a
    return wide[:, 24:24 + d]


# ---- 1. per block against fp64 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", list(alc.ROW_PATTERNS))
@pytest.mark.parametrize("name", list(alc.CASES))
def test_lin2_per_block_and_species_against_fp64(name, pattern):
    p = problem(name, pattern)
    bad = failures(run_lin2(p), *p.lin2_refs(), p.species, p.lay.irreps_out, f"{name}/{pattern}")
    assert not bad, bad


@pytest.mark.parametrize("n_rows", ONE_ROWS)
@pytest.mark.parametrize("name", ["paper_like", "mo17", "tiny"])
def test_single_species_entry_against_fp64(name, n_rows):
    p = problem(name, n_rows)
    assert p.order() is None
    bad = failures(run_lin2(p), *p.lin2_refs(), p.species, p.lay.irreps_out, f"{name}/one/{n_rows}")
    assert not bad, bad


# ---- 2. the addend ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["contiguous", "slice"])
@pytest.mark.parametrize("name", ["paper_like", "mo33", "mo12_d3"])
def test_addend_contiguous_and_as_a_column_slice(name, how):
    p = problem(name, "ragged")
    add = dev_add(p, how)
    assert how != "slice" or (add.stride(0) > p.lay.ap.d_out and not add.is_contiguous())
    bad = failures(run_lin2(p, add=add), *p.lin2_refs(add=True), p.species, p.lay.irreps_out, f"{name}/add {how}")
    assert not bad, bad


# ---- 3. the Gate (+ BatchNorm) epilogue ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", list(alc.ROW_PATTERNS))
@pytest.mark.parametrize("name", list(alc.GATED))
def test_gate_epilogue_per_block_against_fp64_gate_and_batchnorm(name, pattern):
    p = problem(name, pattern, True)
    for with_bn in (False, True):
        bn = alc.oracle_batchnorm(p.lay) if with_bn else None
        got = run_gate(p, dev_add(p, "slice"), bn)
        assert got.shape == (p.N, p.lay.gate.irreps_out.dim)
        bad = failures(got, *p.gate_refs(bn), p.species, p.lay.gate.irreps_out, f"gate {name}/{pattern}/bn={with_bn}")
        assert not bad, bad


# ---- 4. row independence and reproducibility ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,gated", [("paper_like", False), ("paper_like", True), ("gates_65", True)])
def test_rows_do_not_depend_on_their_neighbours_in_the_wave(name, gated):
    """a row's result has the same bits whatever rows share its wave: the same launch twice, the rows of every species in
    reverse order, the batch cut to its first half (species kept) -- nothing leaks between the 16 rows of a wave through
    the stage, rowid or the gate registers"""
    p = problem(name, "blocks", gated)
    bn = alc.oracle_batchnorm(p.lay) if gated else None
    run = (lambda **k: run_gate(p, k.pop("add"), bn, **k)) if gated else (lambda **k: run_lin2(p, **k))
    add = dev_add(p, "contiguous")
    first = run(add=add)
    assert torch.isfinite(first).all()
    assert torch.equal(first, run(add=add))
    assert torch.equal(first, run(add=add, order=p.order(reverse=True)))
    h = p.N // 2
    order_h = tuple(_dev(t) for t in alc.order_seg(p.species[:h], p.lay.S))
    half = run(add=add[:h], row=np.ascontiguousarray(p.row[:h]), order=order_h)
    assert half.shape[0] == h and torch.equal(first[:h], half)


# ---- 5. unwritten output ---------------------------------------------------------------------------------------------------------
def test_every_output_element_is_written():
    """the result buffer really is NaN before the launch (the module's fixture reaches ops), and afterwards every element
    is finite and right: rows of a one-row species and the last, partly filled wave included"""
    from matten_amd import ops

    assert torch.isnan(torch.empty(3, 5, device=DEV)).all() and ops.torch.empty is torch.empty
    for name, gated in (("paper_like", False), ("wide_scalars", False), ("mo17", False), ("paper_like", True), ("gates_65", True)):
        p = problem(name, "ragged", gated)
        assert 1 in np.bincount(p.species).tolist() and p.N % 16 != 0
        if gated:
            got, refs, irreps = run_gate(p, dev_add(p, "contiguous")), p.gate_refs(), p.lay.gate.irreps_out
        else:
            got, refs, irreps = run_lin2(p), p.lin2_refs(), p.lay.irreps_out
        assert torch.isfinite(got).all()
        assert not failures(got, *refs, p.species, irreps, f"poisoned out {name} gated={gated}")


# ---- 6. the species scan -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,rows_of", [(4400, {0: 3, 1: 1, 4347: 2, 4348: 5, 4399: 1}), (73, {2: 130, 3: 1, 40: 128, 71: 40, 72: 1})])
def test_species_scan_paths(S, rows_of):
    """S + 1 = 4401 offsets exceed what the scan keeps in LDS (8 x (16 x 33 + 16) - 4 = 4348 ints): the global-memory
    fallback; S = 73 takes the LDS scan with most species empty"""
    counts = np.zeros(S, dtype=np.int64)
    for s, n in rows_of.items():
        counts[s] = n
    assert counts.sum() == (12 if S == 4400 else 300)
    assert (S + 1 > 8 * (16 * 33 + 16) - 4) == (S == 4400)
    p = Problem(alc.plan_case(*alc.CASES["tiny"], S, name="tiny"), alc.species_rows(counts))
    assert not failures(run_lin2(p, add=dev_add(p, "contiguous")), *p.lin2_refs(add=True), p.species, p.lay.irreps_out, f"tiny S={S}")


# ---- 7. LDS above the default ------------------------------------------------------------------------------------------------
def test_lds_above_64k_runs_and_above_80k_is_refused():
    from matten_amd import _lib

    lib = _lib.load()
    p = problem("lds_79k", "ragged")
    ap = p.lay.ap
    assert lib.matten_agg_linear_lds_bytes(ap.w_stride, len(ap.io_table), len(ap.blocks)) == alc.LDS_79K_BYTES
    assert not failures(run_lin2(p), *p.lin2_refs(), p.species, p.lay.irreps_out, "lds_79k/ragged")
    # the 93 KB layout: MATTEN_EINVAL from the C entry, before any launch (well-formed buffers; no reference needed)
    lay = alc.plan_case(*alc.LDS_OVER, 2)
    ap = lay.ap
    assert lib.matten_agg_linear_lds_bytes(ap.w_stride, len(ap.io_table), len(ap.blocks)) == alc.LDS_OVER_BYTES
    species = alc.species_rows((9, 8))
    agg, w = alc.make_inputs(lay, species)
    row = _dev(alc.scatter_rows(lay, agg)[0])
    order = tuple(_dev(t) for t in alc.order_seg(species, 2))
    from matten_amd import ops

    with pytest.raises(_lib.MattenHipError, match="MATTEN_EINVAL"):
        ops.agg_linear(row, order, _dev(alc.make_wtab(ap, w)), _dev(ap.io_table),
                       _dev(ap.blocks), ap.d_out)


# ---- 8. arguments refused without a launch -----------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_any_launch():
    """host-side argument checks only: every buffer is well formed, none of these calls reaches a kernel"""
    from matten_amd import _lib, ops
    from matten_amd.nn._activation import act_const_table

    p = problem("tiny", "ragged", True)
    lay, ap = p.lay, p.lay.ap
    io, blk = p.tables()
    row, wtab = _dev(p.row), _dev(p.wtab)
    order, seg = p.order()
    einval = pytest.raises(_lib.MattenHipError, match="MATTEN_EINVAL")
    with einval:   # ld not a multiple of 4
        ops.agg_linear(torch.zeros(p.N, ap.ld + 2, device=DEV), (order, seg), wtab, io, blk, ap.d_out)
    with einval:   # order without seg
        ops.agg_linear(row, (order, None), wtab, io, blk, ap.d_out)
    with einval:   # seg without order
        ops.agg_linear(row, (None, seg), wtab, io, blk, ap.d_out)
    with einval:   # several species without order
        ops.agg_linear(row, None, wtab, io, blk, ap.d_out)
    with einval:   # addend rows shorter than the output row
        ops.agg_linear(row, (order, seg), wtab, io, blk, ap.d_out, add=torch.zeros(p.N, ap.d_out - 1, device=DEV))
    cmeta, cst = _dev(lay.cmeta), act_const_table().to(DEV)
    d_act = lay.gate.irreps_out.dim
    with einval:
        ops.agg_linear_gate(row, (order, None), wtab, io, blk, ap.d_out, cmeta, cst, d_act)
    with pytest.raises(ValueError, match="cmeta"):
        ops.agg_linear_gate(row, (order, seg), wtab, io, blk, ap.d_out, cmeta[:-1], cst, d_act)
    with pytest.raises(ValueError, match="bn_scale"):
        ops.agg_linear_gate(row, (order, seg), wtab, io, blk, ap.d_out, cmeta, cst, d_act,
                            bn_scale=torch.ones(d_act + 1, device=DEV), bn_shift=torch.zeros(d_act + 1, device=DEV))
    empty = ops.agg_linear(row[:0], (order[:0], seg), wtab, io, blk, ap.d_out)       # no rows: an empty result
    assert empty.shape == (0, ap.d_out)
    assert ops.agg_linear_gate(row[:0], (order[:0], seg), wtab, io, blk, ap.d_out, cmeta, cst, d_act).shape == (0, d_act)


# ---- 9. the comparison can see an error ---------------------------------------------------------------------------------------
def _weak_block(p):
    """(io_table row, block) of paper_like's 2x4e: the weakest block of the row (2 channels of 32 + 16 + 16 + ...)"""
    lo, hi, name = alc.irrep_blocks(p.lay.irreps_out)[-1]
    assert name == "2x4e"
    r = [alc.unpack_io(x) for x in p.lay.ap.io_table if int(x[5]) == lo]
    assert len(r) == 1 and r[0]["mo"] == 2 and r[0]["kk"] == 9
    return r[0], name


def test_comparison_sees_one_weight_off_by_a_thousandth():
    """negative control: one A-fragment entry of ONE species, in the 2x4e block, changed by 1e-3 of its value -> exactly
    (2x4e, that species) fails; every other block and species still passes"""
    p = problem("paper_like", "ragged")
    r, name = _weak_block(p)
    s = 3
    wtab = p.wtab.copy()
    span = np.arange(r["a_off"], r["a_off"] + r["T"] * r["n_mt"] * 4 * r["cw"] * 4)
    idx = span[np.argmax(np.abs(wtab[s, span]))]
    wtab[s, idx] *= np.float32(1.001)
    bad = failures(run_lin2(p, wtab=wtab), *p.lin2_refs(), p.species, p.lay.irreps_out, "control: weight")
    assert set(bad) == {(name, s)}, bad


def test_comparison_sees_two_swapped_slots_of_one_row():
    """negative control: two adjacent channel slots of one component of the 2x4e region swapped in ONE row -> exactly
    (2x4e, that row's species) fails"""
    p = problem("paper_like", "ragged")
    r, name = _weak_block(p)
    n = int(np.nonzero(p.species == 4)[0][5])
    row = p.row.copy()
    o = 16 * (r["c0"] + 4 * r["T"]) + 2          # component k = 4, slots 2 and 3
    assert np.isfinite(row[n, o:o + 2]).all() and row[n, o] != row[n, o + 1]
    row[n, o], row[n, o + 1] = row[n, o + 1], row[n, o]
    bad = failures(run_lin2(p, row=row), *p.lin2_refs(), p.species, p.lay.irreps_out, "control: slots")
    assert set(bad) == {(name, 4)}, bad
