"""What tests/test_gpu_species_linear.py relies on, as far as a machine without a GPU can check it: every case of
species_linear_cases.py sits on the kernel and on the side of every launcher threshold it claims (thresholds from the
library's accessors, the route from ops.species_linear_route -- the rule ops.species_linear itself applies), every family
reaches the branches it names, the integer twins are exact in fp32, and the fp32 oracle's distance from the fp64 one is
printed per family.  A later change of a threshold or of the routing rule fails HERE instead of silently moving cases to
the other kernel."""
import os
from collections import Counter

import numpy as np
import pytest

import species_linear_cases as slc
from matten_amd import _lib, ops, plan as mplan


@pytest.fixture(scope="module")
def lib():
    return _lib.load()     # symbols only: no device needed


def _segs(case, transposed=False):
    return [tuple(int(v) for v in r) for t in slc.seg_tables(case, transposed) for r in t]


def _family(name):
    return {n: c for n, c in slc.CASES.items() if c.family == name}


# ---- the accessors and the routing rule ------------------------------------------------------------------------------------
def test_accessors_are_declared_bound_and_exported(lib):
    header = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "matten_hip.h")).read()
    for name in ("matten_species_linear_walk_all_blocks", "matten_species_linear_lds_w_floats",
                 "matten_species_linear_rows_lds_bytes"):
        assert name in _lib.SIGNATURES and name + "(void)" in header and getattr(lib, name)() > 0
    assert _lib.ABI_VERSION == 47 and lib.matten_abi_version() == 47          # entries were only added
    # the streaming kernel's table capacity leaves room for the four waves' transpose tiles; the rows kernel's limit is
    # at least what the routing rule hands it
    assert lib.matten_species_linear_lds_w_floats() % 4 == 0
    assert ops._SL_ROWS_LDS_BYTES <= lib.matten_species_linear_rows_lds_bytes()


def test_route_is_the_rule_of_ops_species_linear():
    """the pure function: the 52 KB rule on one segment table, "stream" for several passes; ops.species_linear calls it"""
    import inspect

    assert "species_linear_route(" in inspect.getsource(ops.species_linear)
    for d_in, w, n in ((30, 58, 6), (781, 781, 1), (782, 782, 1), (256, 768, 1), (1000, 10, 1), (10, 13000, 2)):
        want = "rows" if 4 * (16 * (d_in | 1) + w + 8 * n + 4) <= 52 * 1024 else "stream"
        assert ops.species_linear_route(d_in, w, [n]) == want
        assert ops.species_linear_route(d_in, w, [n, 1]) == "stream"
    assert ops.species_linear_route(781, 781, [1]) == "rows" and ops.species_linear_route(782, 782, [1]) == "stream"


def test_every_case_is_on_the_kernel_it_claims(lib):
    """the routing table: a case runs on "rows" only where the rule routes it there (variant="rows" on anything else would
    silently stream) and where the C entry accepts the layout; every forced-streaming case states whether the table is in
    LDS and whether one workgroup walks all irrep blocks"""
    walk, w_cap, rows_cap = (lib.matten_species_linear_walk_all_blocks(), lib.matten_species_linear_lds_w_floats(),
                             lib.matten_species_linear_rows_lds_bytes())
    cases = dict(slc.CASES, **slc.block_walk_cases(walk))
    table = Counter()
    for name, c in cases.items():
        lp = slc.plan_of(c)
        r = slc.route(c)
        assert set(c.variants) <= {"rows", "stream"} and c.variants, name
        if "rows" in c.variants:
            assert r == "rows" and len(lp.passes) == 1 and slc.rows_lds_bytes(c) <= rows_cap, name
        w_lds = ((lp.w_stride + 3) & ~3) <= w_cap
        one_wg = slc.stream_blocks(c) >= walk
        assert w_lds == (name != "w_lds/above"), name
        assert one_wg == name.startswith("walk/at"), name
        table[(c.family, "+".join(c.variants), f"routes to {r}", "W in LDS" if w_lds else "W in global memory",
               "one workgroup walks all blocks" if one_wg else "one block per blockIdx.y")] += 1
    print("\nspecies-linear cases: family, kernels run, natural route, A operand, walk -> cases")
    for k, n in sorted(table.items()):
        print("  " + " | ".join(k) + f" -> {n}")
    # the adjoint cases: both directions fit the rows kernel except the several-pass one
    for name in slc.ADJOINT_CASES:
        c = slc.CASES[name]
        want = "stream" if c.family == "passes" else "rows"
        assert slc.route(c) == want and slc.route(c, transposed=True) == want, name


# ---- branches per family -----------------------------------------------------------------------------------------------------
def test_output_tiles_family_crosses_every_tile_boundary():
    fam = _family("out_tiles")
    assert len(fam) == 5 * len(slc.OUT_MO) and {c.n_rows for c in fam.values()} == {37}
    assert set(slc.OUT_MO) == set(range(1, 6)) | {15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 79, 80, 81, 144, 145}
    for l in range(5):
        d = 2 * l + 1
        segs = [_segs(c) for n, c in fam.items() if n.startswith(f"out/l{l}/")]
        assert all(len(s) == 1 and s[0][1] == d and s[0][2] == slc.OUT_MI[l] for s in segs)
        n_vt = sorted({-(-s[0][4] // 16) for s in segs})
        assert n_vt == [1, 2, 3, 4, 5, 6, 9, 10]
        # d <= 3: two tiles per group -- a lone last tile (odd n_vt) and a full last pair; d >= 5: one tile per group
        assert {n % 2 for n in n_vt} == {0, 1}
        # tiles whose last lane group holds 1, 2, 3 channels (the scalar store branch) and a full 4 (the 16-byte stores)
        assert {s[0][4] % 4 for s in segs} == {0, 1, 2, 3}
        assert all(c.adds == (False, True) and c.variants == ("stream",) for c in fam.values())


def test_input_chunks_family_crosses_every_step_and_chunk_boundary():
    fam = _family("in_chunks")
    for l in range(5):
        d = 2 * l + 1
        ks, ch = slc.steps_per_chunk(d), slc.CHUNK_CHANNELS[d]
        mis = sorted(_segs(c)[0][2] for n, c in fam.items() if n.startswith(f"in/l{l}/"))
        assert mis == list(slc.input_mis(d)) and {1, 15, 16, 17, ch - 1, ch, ch + 1, 2 * ch - 1, 2 * ch, 2 * ch + 1, 321} == set(mis)
        chunks = {-(-(-(-mi // 16)) // ks) for mi in mis}
        assert {1, 2, 3} <= chunks                       # one, two, three and (mi = 321) many chunks per output tile
        assert {mi % 4 for mi in mis} >= {0, 1, 3}       # contraction tails inside one matrix instruction
    assert all(c.S == 3 and c.n_rows == 50 and c.variants == ("stream",) for c in fam.values())


def test_block_walk_family(lib):
    walk = lib.matten_species_linear_walk_all_blocks()
    n_at, n_below = slc.walk_rows(walk)
    assert -(-n_at // 64) + 3 == walk and -(-n_below // 64) + 3 == walk - 1 and n_at == n_below + 1
    for name, c in dict(_family("block_walk"), **slc.block_walk_cases(walk)).items():
        lp, segs = slc.plan_of(c), _segs(c)
        assert lp.d_in + lp.d_out == 77 and 4 * c.n_rows * 77 < 11e6                 # ~70 floats per row, <= 10 MB
        assert sorted(s[1] for s in segs if s[2]) == [1, 3, 5, 7, 9]                  # all five d
        assert any(s[0] % 2 for s in segs) and any(s[5] % 2 for s in segs)            # odd x_off / o_off
        empty = [i for i, s in enumerate(segs) if s[2] == 0]
        assert len(empty) == 1 and segs[empty[0]][1:3] == (3, 0) and segs[empty[0]][4] == 1
        # the plan appends empty segments to the table; the rotated table puts it between two others
        assert empty[0] == (2 if c.seg_rotate else len(segs) - 1), name
        assert sorted(segs) == sorted(_segs(slc.CASES["walk/n37"]))                   # the same segments in every order
    assert {c.n_rows for c in slc.block_walk_cases(walk).values()} == {n_at, n_below}


def test_species_family_group_sizes_and_order():
    fam = _family("species")
    assert {c.S for c in fam.values()} == {1, 3, 70}
    s3 = [n for c in fam.values() if c.S == 3 for n in c.counts]
    assert set(s3) >= set(slc.GROUP_SIZES)
    s70 = slc.CASES["species/S70"]
    assert set(s70.counts) >= set(slc.GROUP_SIZES) and s70.counts[5] == 0 and s70.counts[69] == 0 and s70.counts[66] == 129
    assert {c.n_rows for c in fam.values()} >= {1, 129}
    for name in ("species/S70", "species/S3/1", "species/S1/n129"):
        order, seg = slc.problem(name).order()
        assert (np.diff(order.astype(np.int64)) < 0).any(), name                       # `order` is not monotone in node id
        sp = slc.problem(name).species
        assert (np.diff(sp[order]) >= 0).all() and seg[-1] == len(sp)
    assert all(c.variants == ("rows", "stream") for c in fam.values())


def test_w_lds_family_straddles_the_capacity(lib):
    cap = lib.matten_species_linear_lds_w_floats()
    below, above = slc.plan_of(slc.CASES["w_lds/below"]), slc.plan_of(slc.CASES["w_lds/above"])
    assert cap - 88 < below.w_stride <= cap < above.w_stride <= cap + 4 * 88          # within one / four input channels
    assert _segs(slc.CASES["w_lds/below"])[0][4] == 88 == _segs(slc.CASES["w_lds/above"])[0][4]   # six tiles: three groups


def test_rows_capacity_family(lib):
    fam = _family("rows_cap")
    route_of = lambda k: slc.route(slc.Case("x", f"{k}x0e", "1x0e", 2, (1, 1), ("rows",)))
    assert slc.ROWS_ODD_MAX % 2 == 1 and slc.ROWS_EVEN_MAX % 2 == 0
    assert [route_of(k) for k in (slc.ROWS_EVEN_MAX, slc.ROWS_ODD_MAX, slc.ROWS_OVER, slc.ROWS_OVER + 1)] == \
        ["rows", "rows", "stream", "stream"]
    assert {slc.plan_of(c).d_in for c in fam.values()} >= {256, 257, 780, 781}
    w15 = slc.plan_of(fam["rows_cap/w15"])
    assert w15.w_stride % 4 == 3 and fam["rows_cap/w15"].S == 3      # species 1, 2: tables at 60 and 120 bytes
    assert [(_segs(fam[f"rows_cap/mul_in{m}"])[-1][2]) for m in (0, 1, 4, 5, 8, 9)] == [0, 1, 4, 5, 8, 9]
    assert [sum(-(-s[4] // 16) for s in _segs(fam[f"rows_cap/items{n}"])) for n in (1, 3, 4, 5)] == [1, 3, 4, 5]
    assert all(slc.rows_lds_bytes(c) <= ops._SL_ROWS_LDS_BYTES for c in fam.values())


def test_plain_uncovered_and_strided_families():
    assert [c.n_rows for c in _family("plain").values()] == [1, 16, 129] and all(c.S is None for c in _family("plain").values())
    assert slc.problem("plain/n16").order() is None
    out, inn = slc.CASES["uncovered/out"], slc.CASES["uncovered/in"]
    assert [s for s in _segs(out) if s[2] == 0] == [(0, 5, 0, 0, 2, 5, 0, 0)]            # 2x2e of the output: empty segment
    assert [s for s in _segs(inn, transposed=True) if s[2] == 0] == [(0, 5, 0, 0, 2, 4, 0, 0)]   # 2x2e of the input, in dx
    assert slc.plan_of(out).fully_covered and slc.plan_of(inn).input_covered              # the kernels fill them themselves
    p = slc.problem("uncovered/out")
    assert (p.want64[:, 5:15] == 0).all() and (p.want_int[:, 5:15] == 0).all()
    assert all(c.adds == (True,) and c.variants == ("rows", "stream") for c in _family("strided_add").values())


def test_some_irreps_need_several_passes():
    """plan_fctp merges only ADJACENT equal irreps and plan_linear merges nothing, so two input blocks of one irrep give
    a second forward pass and two output blocks of one irrep a second adjoint pass; the rows kernel takes one table only,
    so such calls always stream"""
    fctp, plain = slc.plan_of(slc.CASES["passes/fctp"]), slc.plan_of(slc.CASES["passes/plain"])
    assert (len(fctp.passes), len(fctp.passes_t)) == (2, 2) and (len(plain.passes), len(plain.passes_t)) == (2, 1)
    assert slc.route(slc.CASES["passes/fctp"]) == slc.route(slc.CASES["passes/plain"]) == "stream"
    # the shipped layouts (sorted, simplified irreps) have one pass each way
    lp = mplan.plan_fctp("32x0e+16x1o+4x2e", 4, "32x0e+16x1o+16x1e+4x2e")
    assert len(lp.passes) == len(lp.passes_t) == 1


# ---- the references ----------------------------------------------------------------------------------------------------------
def test_integer_twins_are_exact_in_fp32_and_agree_with_the_oracle():
    """every partial sum of a twin is an integer below 2^24, and int64 arithmetic over the irreps gives what the oracle
    (fp64, raw weights: its path normalisation divided out per output block) gives"""
    import torch

    for name in ("out/l0/mo17", "in/l1/mi321", "walk/n37", "species/S70", "plain/n16", "uncovered/out", "passes/fctp",
                 "passes/plain", "rows_cap/din781"):
        p = slc.problem(name)
        lp = p.plan
        bound = 2 * max(int(s[2]) for t in lp.passes for s in t) * len(lp.passes) + 3
        assert np.abs(p.int_refs(True)).max() <= bound < 2 ** 24
        ref = slc.oracle_module(p.case, p.wi, torch.float64)
        with torch.no_grad():
            got = slc.oracle_apply(p.case, ref, torch.from_numpy(np.array(p.xi)).double(), p.species, torch.float64).numpy()
        S = p.case.S or 1
        fan = {}
        for i_in, i_out, _, _ in lp.instr:
            fan[i_out] = fan.get(i_out, 0) + lp.irreps_in[i_in].mul * S
        offs = lp.irreps_out.offsets()
        for i_out, (mul, irr) in enumerate(lp.irreps_out):
            lo, hi = offs[i_out], offs[i_out] + mul * irr.dim
            np.testing.assert_allclose(got[:, lo:hi] * fan.get(i_out, 1) ** 0.5, p.want_int[:, lo:hi], rtol=0, atol=1e-9)


def test_fp32_oracle_distance_per_family():
    """printed for the record: the fp32 oracle's own distance from the fp64 one, as a fraction of 2e-6 x the block maximum
    (per irrep block and species).  Where it exceeds 0.25 the second term of the bound (4 x that distance) is the larger."""
    worst = {}
    for name, c in slc.CASES.items():
        p = slc.problem(name)
        res = slc.block_errors(p.want32.numpy(), p.want64.numpy(), p.want32.numpy(), p.species,
                               slc.irrep_blocks(p.plan.irreps_out))
        for (blk, s), (err, allowed, scale) in res.items():
            if scale > 0:
                assert err <= allowed / 4 + 1e-300 or allowed == 4 * err
                worst[c.family] = max(worst.get(c.family, 0.0), err / (slc.RTOL * scale))
    print("\nfp32 oracle distance / (2e-6 x block maximum), worst per family:")
    for k, v in sorted(worst.items()):
        print(f"  {k}: {v:.2f}")
    assert set(worst) == {c.family for c in slc.CASES.values()}


def test_inputs_are_write_protected():
    p = slc.problem("walk/n37")
    for a in (p.x, p.w, p.wp, p.add, p.xi, p.wpi, p.species):
        with pytest.raises(ValueError):
            a[...] = 0


# ---- the existing sweep ------------------------------------------------------------------------------------------------------
def test_shape_sweep_routing_is_what_its_docstring_records():
    """test_gpu_parity.test_species_linear_shape_sweep's families under today's rule: the docstring there quotes these
    counts"""
    def r(iin, iout, S):
        lp = mplan.plan_fctp(iin, S, iout)
        return ops.species_linear_route(lp.d_in, lp.w_stride, [len(t) for t in lp.passes])

    mo = Counter(r(f"{mi}x{slc.ir(l)}", f"{m}x{slc.ir(l)}", 2)
                 for m in list(range(1, 40)) + [63, 64, 65, 70, 78, 79, 80, 81, 96, 97, 127, 128, 129, 161]
                 for l, mi in ((0, 8), (1, 5), (2, 3)))
    mi_stream = sorted((m, l) for m in list(range(1, 36, 2)) + [159, 160, 161, 170, 321] for l in range(5)
                       if r(f"{m}x{slc.ir(l)}+3x0e", f"5x{slc.ir(l)}+2x0e", 3) == "stream")
    assert mo == {"rows": 159}
    assert len(mi_stream) == 16 and all((m >= 159 and l >= 2) or (m == 321 and l >= 1) for m, l in mi_stream)
    assert r("400x0e+20x1o", "90x0e+7x1o", 3) == r("330x1o", "100x1o", 2) == "stream"
