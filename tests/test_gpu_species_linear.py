"""matten_species_linear (register-streaming) and matten_species_linear_rows (LDS-resident) called directly through
ops.species_linear(variant=...), per output irrep block and per species against the oracle in fp64: the cases, inputs and
references of species_linear_cases.py (test_species_linear_host.py asserts which kernel and which branch every case
reaches).  The buffer ops allocates for the result is NaN before every launch of this module.

Tolerance (no new number): per block and per species the kernel may be max(2e-6 x the block's maximum, 4 x the fp32
oracle's own distance from the fp64 one) away from the fp64 reference -- 2e-6 is test_species_linear_shape_sweep's bound,
the second term the want64 rule of test_gpu_parity.close_blocks; a block whose reference is identically zero must be
exactly zero.  Every case also runs its integer twin (exact in fp32 in any summation order) bit for bit, and twice.

Worst measured |kernel - fp64| / block maximum over all blocks, species and cases of a family, MI355X (fraction of the
allowed distance in brackets); every integer twin exact, every second call bit-identical:
  streaming  out_tiles l = 0..4: 1.9e-7 (0.09)  1.6e-7 (0.08)  1.3e-7 (0.06)  9.2e-8 (0.05)  9.4e-8 (0.05)
             in_chunks l = 0..4: 1.1e-6 (0.55)  8.8e-7 (0.44)  8.6e-7 (0.43)  1.0e-6 (0.52)  1.2e-6 (0.58)   (mi up to 321)
             block walk n37 9.5e-8 (0.05)   n37 / empty segment mid-table 1.1e-7 (0.06)   one workgroup below the
             threshold (32512 rows) 1.0e-7 (0.05)   at the threshold (32513 rows) 1.2e-7 (0.06), mid-table 1.1e-7 (0.06)
             w_lds (table in LDS / in global memory) 8.8e-7 (0.44)   passes 1.3e-7 (0.07)
  both       species rows 1.8e-7 (0.09) stream 2.5e-7 (0.13)   plain 1.1e-7 (0.06) / 1.0e-7 (0.05)
             uncovered 8.2e-8 (0.04) / 8.2e-8 (0.04)   strided addend 1.4e-7 (0.07) on both, bit-identical to the copy
  rows       rows_cap 8.2e-7 (0.41)   (d_in 780 / 781: 781 terms)
  adjoints   dx: walk 1.7e-7 (0.08) rows, 1.5e-7 (0.07) stream   S70 2.1e-7 (0.10) / 1.9e-7 (0.10)   uncovered 9.1e-8 (0.05)
             passes 6.9e-8 (0.03);   dweight: walk 6.3e-7 (0.31)   S70 1.0e-6 (0.52)   uncovered 1.1e-7 (0.05)   passes 4.7e-7 (0.24)
  controls   one packed weight off by 1e-3: 500 x allowed   two species' tables swapped: >= 418361 x allowed in every block
  rows vs stream: 55 of the 123 cases that fit both kernels differ in some bit, by at most 1.8e-7 of the output maximum
The whole file takes about 5 s on MI355X (41 tests, the slowest 0.7 s).
"""
import collections

import numpy as np
import pytest
import torch

import species_linear_cases as slc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CALLS = collections.Counter()      # launches per C entry since the test began (see entry_calls)


def _dev(a, device=DEV):
    """a (write-protected) numpy array as a tensor: a copy, so that the shared inputs stay as they were made"""
    return torch.from_numpy(np.array(a)).to(device)


@pytest.fixture(autouse=True)
def nan_empty(monkeypatch):
    """every float buffer torch.empty hands out on the device starts as NaN (for this module only): an output element a
    kernel does not write fails the comparison instead of passing by chance"""
    _empty = torch.empty

    def empty(*a, **k):
        t = _empty(*a, **k)
        return t.fill_(float("nan")) if t.is_floating_point() and t.device.type == "cuda" else t

    monkeypatch.setattr(torch, "empty", empty)


@pytest.fixture(autouse=True)
def entry_calls(monkeypatch):
    """counts the launches of the two C entries, so that a test can assert which kernel it ran"""
    from matten_amd import _lib, selfcheck

    selfcheck.check_species_linear(torch.device(DEV))     # the first call's self-check, before counting starts
    lib = _lib.load()
    CALLS.clear()
    for name in ("matten_species_linear", "matten_species_linear_rows"):
        fn = getattr(lib, name)

        def counted(*a, _fn=fn, _name=name):
            CALLS[_name] += 1
            return _fn(*a)

        monkeypatch.setattr(lib, name, counted)
    yield CALLS


def _threshold():
    from matten_amd import _lib

    return _lib.load().matten_species_linear_walk_all_blocks()


def dev_add(a, how):
    """None / contiguous / a column slice at a non-zero, odd column offset of a wider row-major buffer whose other columns
    are NaN -- as conv.py forms self_connection = both[:, d1:]: add_ld != d_out and a base that is only 4-byte aligned"""
    if how is None:
        return None
    a = _dev(a)
    if how == "contiguous":
        return a
    d = a.shape[1]
    wide = torch.full((a.shape[0], d + 19), float("nan"), device=DEV)
    wide[:, 13:13 + d] = a
    view = wide[:, 13:13 + d]
    assert view.stride(0) == d + 19 and not (view.is_contiguous() and d > 0 and a.shape[0] > 1) and view.data_ptr() % 16 == 4
    return view


def run(p: slc.Problem, variant, add=None, integer=False, wp=None, x=None):
    """one call of ops.species_linear on the case's plan tables, on the kernel asked for"""
    from matten_amd import ops

    lp = p.plan
    if variant == "rows":
        assert slc.route(p.case) == "rows"        # variant="rows" on a layout that does not fit would stream
    tabs = [_dev(t) for t in slc.seg_tables(p.case)]
    order = p.order()
    order = None if order is None else tuple(_dev(t) for t in order)
    x = _dev((p.xi if integer else p.x) if x is None else x)
    wp = _dev((p.wpi if integer else p.wp) if wp is None else wp)
    before = collections.Counter(CALLS)
    out = ops.species_linear(x, order, wp, lp.w_stride, tabs, lp.d_out, add, lp.fully_covered, variant=variant)
    new = CALLS - before
    assert new == {"matten_species_linear_rows" if variant == "rows" else "matten_species_linear": len(tabs)}, new
    return out


def failures(got, want64, want32, species, blocks, what="", stats=None):
    """{(block, species)} outside the module's tolerance; stats collects (worst |err| / block max, worst err / allowed)"""
    got = got.detach().cpu()
    assert torch.isfinite(got).all(), f"{what}: {int((~torch.isfinite(got)).sum())} output elements are not finite"
    res = slc.block_errors(got.numpy(), want64.numpy(), want32.numpy(), species, blocks)
    if stats is not None:
        for err, allowed, scale in res.values():
            if scale > 0:
                stats[0] = max(stats[0], err / scale)
                stats[1] = max(stats[1], err / allowed)
    return {(what,) + k: v for k, v in res.items() if not v[0] <= v[1]}


def check_case(name, variant, stats, threshold=0):
    """gaussian inputs per block and species against fp64, the integer twin bit for bit, both twice -- without and with a
    contiguous addend as the case asks"""
    p = slc.problem(name, threshold)
    blocks = slc.irrep_blocks(p.plan.irreps_out)
    bad = {}
    for with_add in p.case.adds:
        what = f"{name}/{variant}/add={int(with_add)}"
        got = run(p, variant, dev_add(p.add, "contiguous" if with_add else None))
        bad.update(failures(got, *p.refs(with_add), p.species, blocks, what, stats))
        assert torch.equal(got, run(p, variant, dev_add(p.add, "contiguous" if with_add else None))), f"{what}: not repeatable"
        goti = run(p, variant, dev_add(p.addi, "contiguous" if with_add else None), integer=True).cpu().numpy()
        wanti = p.int_refs(with_add)
        assert goti.shape == wanti.shape
        n_bad = int((goti != wanti).sum())        # (NaN != x: an unwritten element counts)
        assert n_bad == 0, f"{what}: integer twin: {n_bad} of {goti.size} outputs wrong"
    return bad


def check_family(names, variant, label, threshold=0):
    stats, bad = [0.0, 0.0], {}
    for name in names:
        bad.update(check_case(name, variant, stats, threshold))
    print(f"species_linear ratio {label} [{variant}] ({len(names)} cases): worst |err| / block max {stats[0]:.2e}, "
          f"worst fraction of the allowed distance {stats[1]:.2f}")
    assert not bad, bad


def _names(family, variant, prefix=""):
    return [n for n, c in slc.CASES.items() if c.family == family and variant in c.variants and n.startswith(prefix)]


# ---- 1. forward, per block and species against fp64 + integer twins --------------------------------------------------------
@pytest.mark.parametrize("l", range(5))
def test_output_tiles_streaming(l):
    """mo across the 16-channel tiles (two tiles per group for d = 1, 3); d = 1 with an addend is the family in which
    species_linear.hip's accumulators once came out with a stale half"""
    names = _names("out_tiles", "stream", f"out/l{l}/")
    assert len(names) == len(slc.OUT_MO)
    check_family(names, "stream", f"out_tiles l={l}")


@pytest.mark.parametrize("l", range(5))
def test_input_chunks_streaming(l):
    names = _names("in_chunks", "stream", f"in/l{l}/")
    assert len(names) == len(slc.input_mis(2 * l + 1))
    check_family(names, "stream", f"in_chunks l={l}")


@pytest.mark.parametrize("name", ["walk/n37", "walk/n37/empty_mid", "walk/below", "walk/at", "walk/at/empty_mid"])
def test_block_walk_streaming(name):
    """one irrep block per blockIdx.y (37 rows; one workgroup below the launcher's threshold) against ONE workgroup walking
    all irrep blocks with the load cursor two chunks ahead across block boundaries (at the threshold); the table in plan
    order (empty segment last) and rotated (empty segment between two others)"""
    check_family([name], "stream", name, _threshold())


@pytest.mark.parametrize("variant", ["rows", "stream"])
@pytest.mark.parametrize("family", ["species", "plain", "uncovered"])
def test_family_on_both_kernels(family, variant):
    names = _names(family, variant)
    assert len(names) == len([c for c in slc.CASES.values() if c.family == family])
    check_family(names, variant, family)


def test_a_operand_in_lds_and_in_global_memory():
    check_family(_names("w_lds", "stream"), "stream", "w_lds")


def test_rows_kernel_capacity():
    names = _names("rows_cap", "rows")
    assert len(names) == 15
    check_family(names, "rows", "rows_cap")


def test_several_passes_streaming():
    check_family(_names("passes", "stream"), "stream", "passes")


def test_uncovered_output_block_is_zero_or_the_addend():
    """an output irrep without an input path: exactly zero, or exactly the addend, written by the kernel itself into the
    NaN buffer (the plan marks the layout fully covered: ops does not pre-fill)"""
    p = slc.problem("uncovered/out")
    assert p.plan.fully_covered and torch.isnan(torch.empty(2, 2, device=DEV)).all()
    for variant in ("rows", "stream"):
        assert (run(p, variant)[:, 5:15] == 0).all()
        add = dev_add(p.add, "contiguous")
        assert torch.equal(run(p, variant, add)[:, 5:15], add[:, 5:15])


# ---- 2. the strided addend ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["rows", "stream"])
@pytest.mark.parametrize("name", ["strided_add", "strided_add/walk"])
def test_strided_addend_equals_the_contiguous_copy(name, variant):
    p = slc.problem(name)
    for integer in (False, True):
        a = p.addi if integer else p.add
        sliced = run(p, variant, dev_add(a, "slice"), integer=integer)
        assert torch.isfinite(sliced).all()
        assert torch.equal(sliced, run(p, variant, dev_add(a, "contiguous"), integer=integer))
    stats = [0.0, 0.0]
    bad = failures(run(p, variant, dev_add(p.add, "slice")), *p.refs(True), p.species, slc.irrep_blocks(p.plan.irreps_out),
                   f"{name}/{variant}/slice", stats)
    print(f"species_linear ratio {name} slice [{variant}]: worst |err| / block max {stats[0]:.2e}, fraction {stats[1]:.2f}")
    assert not bad, bad


# ---- 3. the two kernels' summation orders -----------------------------------------------------------------------------------
def test_report_whether_the_two_kernels_agree_bit_for_bit():
    """both kernels are within the bound and exact on the integer twins (above); their fp32 sums are NOT required to agree
    in the last bit: the streaming kernel's j-th matrix instruction of a step contracts channels 16 st + 4 g + j, the rows
    kernel's channels k0 + g.  This prints how many of the cases that fit both kernels differ (the figure is quoted in
    species_linear_rows.hip's header); no equality is asserted."""
    names = [n for n, c in slc.CASES.items() if slc.route(c) == "rows" and c.family in ("species", "plain", "uncovered", "out_tiles")]
    differ, worst = [], 0.0
    for name in names:
        p = slc.problem(name)
        add = dev_add(p.add, "contiguous")
        a, b = run(p, "rows", add).cpu(), run(p, "stream", add).cpu()
        if not torch.equal(a, b):
            differ.append(name)
            worst = max(worst, float(((a - b).abs().max() / p.refs(True)[0].abs().max())))
    print(f"species_linear rows vs stream: {len(differ)} of {len(names)} cases differ in some bit, worst |rows - stream| / "
          f"output maximum {worst:.2e}; first: {differ[:6]}")
    assert len(names) > 100


# ---- 4. adjoints through SpeciesLinearFn --------------------------------------------------------------------------------------
# (the several-pass case streams in both directions: the rows kernel takes one segment table only)
ADJOINT_RUNS = [(n, r) for n in slc.ADJOINT_CASES for r in ("rows", "stream") if r == "stream" or slc.CASES[n].family != "passes"]


@pytest.mark.parametrize("name,route", ADJOINT_RUNS)
def test_adjoints_per_block_and_species_against_fp64_autograd(name, route, monkeypatch, entry_calls):
    """dx (the same kernels on the transposed tables) per input irrep block and species, dweight per instruction path and
    species, against fp64 autograd through the oracle; two evaluations bit-identical; an input irrep that feeds no output
    gets gradient rows that are exactly 0"""
    from matten_amd.nn.utils import SpeciesLinear

    p = slc.problem(name, 0, True)
    c, lp = p.case, p.plan
    assert route == "stream" or slc.route(c) == slc.route(c, transposed=True) == "rows"
    monkeypatch.setenv("MATTEN_SL_ROWS", "1" if route == "rows" else "0")
    mod = SpeciesLinear(c.irreps_in, c.S, c.irreps_out).to(DEV)
    with torch.no_grad():
        mod.weight.copy_(_dev(p.w))
    order = tuple(_dev(t) for t in p.order())
    x = _dev(p.x).requires_grad_(True)
    gy = _dev(p.gy)
    grads = []
    for _ in range(2):
        mod.weight.grad = x.grad = None
        mod(x, order).backward(gy)
        grads.append((x.grad.clone(), mod.weight.grad.clone()))
    entry = "matten_species_linear_rows" if route == "rows" else "matten_species_linear"
    assert set(entry_calls) == {entry} and entry_calls[entry] == 2 * (len(lp.passes) + len(lp.passes_t)), dict(entry_calls)
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])
    (dx64, dw64), (dx32, dw32) = p.grads[torch.float64], p.grads[torch.float32]
    stats = [0.0, 0.0]
    bad = failures(grads[0][0], dx64, dx32, p.species, slc.irrep_blocks(lp.irreps_in), f"{name}/{route}/dx", stats)
    print(f"species_linear ratio {name} dx [{route}]: worst |err| / block max {stats[0]:.2e}, fraction {stats[1]:.2f}")
    assert not bad, bad
    if name == "uncovered/in":
        assert (dx64[:, 4:14] == 0).all() and (grads[0][0][:, 4:14] == 0).all()
    dw = grads[0][1].cpu()
    assert torch.isfinite(dw).all()
    res = slc.vector_errors(dw.numpy(), dw64.numpy(), dw32.numpy(), p.weight_blocks())
    live = [v for v in res.values() if v[2] > 0]
    print(f"species_linear ratio {name} dweight [{route}]: worst |err| / block max {max(v[0] / v[2] for v in live):.2e}, "
          f"fraction {max(v[0] / v[1] for v in live):.2f}; {len(res) - len(live)} (path, species) blocks exactly zero")
    badw = {k: v for k, v in res.items() if not v[0] <= v[1]}
    assert not badw, badw


# ---- 5. the comparison can see an error -------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["rows", "stream"])
def test_comparison_sees_one_weight_off_by_a_thousandth(variant):
    """negative control: the largest packed weight of ONE species in the 1x4e -> 1x4e block changed by 1e-3 of its value ->
    exactly (1x4e, that species) fails; every other block and species still passes"""
    p = slc.problem("walk/n37")
    seg = [r for r in slc.seg_tables(p.case)[0] if r[1] == 9]
    assert len(seg) == 1 and tuple(seg[0][2:5]) == (1, int(seg[0][3]), 1)
    s = 1
    wp = p.wp.copy()
    wp[s, seg[0][3]] *= np.float32(1.001)
    blocks = slc.irrep_blocks(p.plan.irreps_out)
    bad = failures(run(p, variant, wp=wp), *p.refs(False), p.species, blocks, "control")
    assert set(bad) == {("control", blocks[-1][2], s)} and blocks[-1][2].endswith("1x4e"), bad
    err, allowed, _ = bad[("control", blocks[-1][2], s)]
    print(f"species_linear control [{variant}]: one weight off by 1e-3: {err / allowed:.0f} x allowed")
    assert err > 50 * allowed


@pytest.mark.parametrize("variant", ["rows", "stream"])
def test_comparison_sees_two_species_tables_swapped(variant):
    """negative control: the packed tables of species 0 and 1 swapped -> every covered block of those two species fails,
    species 2 passes"""
    p = slc.problem("walk/n37")
    wp = p.wp.copy()
    wp[[0, 1]] = wp[[1, 0]]
    blocks = slc.irrep_blocks(p.plan.irreps_out)
    bad = failures(run(p, variant, wp=wp), *p.refs(False), p.species, blocks, "control")
    covered = [b[2] for b in blocks if not b[2].endswith("1x1e")]
    assert set(bad) == {("control", b, s) for b in covered for s in (0, 1)}, sorted(bad)
    factor = min(v[0] / v[1] for v in bad.values())
    print(f"species_linear control [{variant}]: two species' tables swapped: at least {factor:.0f} x allowed in every block")
    assert factor > 50
