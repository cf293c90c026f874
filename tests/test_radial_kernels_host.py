"""The cases, references and constants of tests/test_gpu_radial_kernels.py (radial_cases.py), as far as a machine without
a GPU can check them: every committed fp32-torch constant is at least the recomputed figure and at most twice it, the
planted lengths exist in the intended numbers, every band of every case of 16 edges or more has rows and a non-zero
reference, rows outside the support have exactly-zero references, the expected-form table is the dispatch rule and covers
every form and every KS0, the split fp16 form's representation term holds, and nothing but the planted len == r_start row
is ever left out of a comparison."""
import numpy as np
import pytest
import torch

import radial_cases as rc


def test_constants_are_the_recomputed_figures_rounded_up():
    got = rc.recompute_constants()
    assert set(got) == set(rc.CONSTANTS), set(got) ^ set(rc.CONSTANTS)
    for k, v in got.items():
        assert v <= rc.CONSTANTS[k] <= 2.0 * v, f"{k}: committed {rc.CONSTANTS[k]:.3e}, recomputed {v:.3e}"
    assert rc.FACTOR == 4.0


def test_case_tables_are_the_ones_planned():
    c = rc.CASES
    grid = [x for x in c.values() if x.group == "grid"]
    assert len(grid) == 32 and {x.E for x in grid} == {67}
    assert {(x.w_pad, x.n_mid) for x in grid} == {(w, m) for w in (112, 128, 256, 272, 384, 400, 512, 528) for m in range(4)}
    assert {x.w_pad for x in grid if x.W == x.w_pad} == {128, 256} and all(x.W == rc.GRID_W[x.w_pad] for x in grid)
    edges = [x for x in c.values() if x.group == "edges"]
    assert {(x.E, x.w_pad) for x in edges} == {(E, w) for E in (1, 15, 16, 17, 64, 65) for w in (48, 224)} | \
        {(65535, 48), (65536, 48)}
    assert all(x.n_mid == 1 for x in edges)
    assert {x.W for x in edges if x.E > 65} == {48}
    assert rc.bw_tiles(65535) == 1 and rc.bw_tiles(65536) == 2       # (and the forward's NT = 1 | 4 switch: 64 * 1024)
    rounds = {(x.n_mid, x.w_pad, x.form) for x in c.values() if x.group == "rounds"}
    assert rounds == {(2, 224, 4), (0, 336, 6), (1, 400, 8)}
    assert all(x.E == 70001 and x.storage for x in c.values() if x.group == "rounds")
    # two rounds per wave, 547 workgroups of 128 edges, the last one with 113
    assert rc.bw_tiles(70001) == 2 and rc.small_slices(70001) == 4 * 547 and 70001 - 546 * 128 == 113
    assert rc.small_slices(67) == 8 and rc.small_slices(64) == 4 and rc.small_slices(65) == 8
    gain = [x for x in c.values() if x.group == "gain"]
    assert gain and all(x.weight_gain == 1e3 and not x.adjoint for x in gain)
    assert set(rc.MULTI_CASES) <= set(c) and rc.MULTI_COUNTS == (1, 4, 8)
    assert {c[n].n_mid for n in rc.MULTI_CASES} == {0, 1, 2, 3} and {c[n].nb_pad for n in rc.MULTI_CASES} == {4, 8, 12, 16}
    assert len({rc.multi_h_scale(j) for j in range(8)}) == 8
    assert {c[n].form != rc.TWO_KERNEL for n in rc.NAN_EMPTY_CASES} == {True, False}
    assert c[rc.NON_DEEP_CASE].n_mid == 1
    # nb and the radial range are tied neither to a width nor to a depth
    for key in (lambda x: x.w_pad, lambda x: x.n_mid):
        for v in {key(x) for x in grid}:
            sub = [x for x in grid if key(x) == v]
            assert len({x.nb for x in sub}) >= 2 and len({x.r_start for x in sub}) == 2, (v,)


def test_expected_form_table_is_the_dispatch_rule_and_covers_every_form():
    for w_pad, row in rc.EXPECTED_FORM.items():
        assert row == tuple(rc.dispatch_rule(w_pad, m) for m in range(4)), w_pad
    adj = [rc.CASES[n] for n in rc.ADJOINT_CASES]
    for form in (rc.TWO_KERNEL, 4, 6, 8):
        assert sum(x.form == form for x in adj if x.group == "grid") >= 2, form
    # both sides of every break of every depth: 112|128, 256|272 (4|6 or the end of n_mid = 2), 384|400, 512|528
    for lo, hi in ((112, 128), (256, 272), (384, 400), (512, 528)):
        assert any(rc.dispatch_rule(lo, m) != rc.dispatch_rule(hi, m) for m in range(4)), (lo, hi)
        assert lo + 16 == hi
    for fused in (False, True):
        assert {x.nb_pad // 4 for x in adj if (x.form != rc.TWO_KERNEL) == fused} == {1, 2, 3, 4}, fused
        assert {x.r_start for x in adj if (x.form != rc.TWO_KERNEL) == fused} == {0.0, 0.5}, fused
    assert {x.nb for x in adj} == {3, 8, 12, 16}
    sto = [rc.CASES[n] for n in rc.STORAGE_CASES]
    assert sum(x.group == "grid" and x.form == rc.TWO_KERNEL for x in sto) == 2
    assert sum(x.group == "grid" and x.form != rc.TWO_KERNEL for x in sto) == 2
    assert {x.form for x in sto if x.group == "rounds"} == {4, 6, 8}
    assert set(rc.STORAGE_FORMS) == {("bf16", 0), ("fp32", 16), ("bf16", 16)}


@pytest.mark.parametrize("name", list(rc.CASES))
def test_lengths_bands_and_rows_left_out(name):
    p = rc.problem(name)
    case, lens, E = p.case, p.lens, p.case.E
    assert lens.dtype == torch.float32 and lens.shape == (E,)
    c = case.r_end - case.r_start
    n_start = int((lens == case.r_start).sum())
    if E >= 16:
        rows = rc.planted_rows(case)
        want = dict(rc.planted_lengths(case))
        assert len(want) == (13 if case.r_start > 0 else 12) and ("below_start" in want) == (case.r_start > 0)
        for k, v in want.items():
            assert lens[rows[k]] == torch.tensor(v, dtype=torch.float32), k
        f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))
        assert int((lens == case.r_end).sum()) == 1 and int((lens == case.r_end + 1.5).sum()) == 1
        assert int((lens == f32(case.r_start + 1e-3)).sum()) == 1 and int((lens == f32(case.r_start + 0.01)).sum()) == 1
        assert int((lens == f32(case.r_end - 1e-3)).sum()) == 1 and f32(case.r_end - 1e-3) < case.r_end
        assert int((lens < case.r_start).sum()) == (1 if case.r_start > 0 else 0)
        assert n_start == 1
        for band, idx in p.bands.items():
            assert idx.numel() >= 3, (band, idx.numel())
            assert p.band_scale(p.h, band) > 0 and p.band_scale(p.w, band) > 0
        assert p.outside.numel() >= 3 + (1 if case.r_start > 0 else 0)       # r_start, r_end, r_end + 1.5, r_start - 0.2
    else:
        assert n_start == 0
    assert float(lens.min()) >= case.r_start - 0.2 - 1e-6 and float(lens.max()) <= max(case.r_end + 1.5, case.r_end + 0.08 * c)
    # rows left out of any comparison: the planted len == r_start row and nothing else
    assert p.excluded.numel() == n_start and p.compared.numel() == E - n_start
    assert torch.equal(torch.sort(torch.cat([p.compared, p.excluded])).values, torch.arange(E))
    # every row is in exactly one band or outside the support (the excluded row counts as outside: its output must be 0)
    parts = torch.cat([*p.bands.values(), p.outside])
    assert torch.equal(torch.sort(parts).values, torch.arange(E))
    assert all(bool((p.t[i] > 0).all() & (p.t[i] < 1).all()) for i in p.bands.values())
    assert set(p.excluded.tolist()) <= set(p.outside.tolist())
    # outside the support the references are exactly zero (silu(0) = 0, no biases)
    assert (p.w[p.outside] == 0).all() and (p.h[p.outside] == 0).all()
    assert torch.isfinite(p.w).all() and torch.isfinite(p.h).all()
    if case.adjoint:
        assert p.gout.shape == (E, case.W) and set(p.grads) == ({"fp32", "bf16"} if case.storage else {"fp32"})
        for g in p.grads.values():
            assert [tuple(x.shape) for x in g] == [(case.nb, 32)] + [(32, 32)] * case.n_mid + [(32, case.W)]
            assert all(torch.isfinite(x).all() and x.abs().max() > 0 for x in g)
    else:
        assert not p.grads


def test_near_end_features_are_much_smaller_than_mid_band_ones():
    """what a whole-tensor scale hides: measured here on the fp64 reference"""
    ratios = [p.band_scale(p.h, "mid") / p.band_scale(p.h, "near_end")
              for p in map(rc.problem, rc.CASES) if p.case.E >= 16 and p.case.weight_gain == 1]
    assert np.median(ratios) > 3.0, np.median(ratios)


@pytest.mark.parametrize("name", ["grid/w128/m1", "grid/w400/m1", "edges/E65536/w48", "gain1e3/m1", "gain1e3/m2"])
def test_split_format_term_holds_for_the_reference(name):
    """ops.split_hidden (the torch statement of split_f16) of the scaled fp64 reference, rounded to the fp32 value a kernel
    would split, decodes to within the representation term: the term is pinned by the format, not by a kernel"""
    from matten_amd import ops

    p = rc.problem(name)
    top = float(p.h.abs().max())
    s0 = min(1.0, 2.0 ** np.floor(np.log2(16384.0 / top)))
    for s in (s0, s0 * 2.0**-7, s0 * 2.0**-20):
        v = (p.h * s).float()
        assert float(v.abs().max()) < 2.0**15
        h2s = ops.split_hidden(v[:, rc.H2S_PERM])
        assert h2s.shape == (p.case.E, 2, 32) and h2s.dtype == torch.float16
        dec = rc.decode_h2s(h2s)
        err = (dec - v.double()).abs()
        assert (err <= rc.split_format_term(v.double().abs())).all(), (name, s, float(err.max()))
        assert (h2s[p.outside] == 0).all()
    # the term is not slack: the relative part is reached within a factor of four, and the floor within a factor of two
    v = (p.h * s0).float()
    err = (rc.decode_h2s(ops.split_hidden(v[:, rc.H2S_PERM])) - v.double()).abs()
    big = v.double().abs() > 2.0**-3
    if big.any():
        assert float((err[big] / v.double().abs()[big]).max()) > 2.0**-24


def test_pack_plan():
    cols, ent, n_tiles, w_pad = rc.pack_plan()
    live = cols[cols >= 0]
    assert cols.dtype == torch.int64 and cols.numel() == rc.PACK_N_COLS and rc.PACK_N_COLS % 16 != 0
    assert int((cols == -1).sum()) == 7 and live.numel() == len(set(live.tolist())) and int(live.max()) < rc.PACK_W
    assert not torch.equal(live, torch.sort(live).values)
    assert w_pad == (rc.PACK_N_COLS + 15) // 16 * 16 + 16
    assert ent.dtype == torch.int32 and ent.shape[1] == 32
    used = ent[ent[:, 7] > 0]
    assert n_tiles == int(used[:, 7].sum()) and torch.equal(used[:, 6], torch.cumsum(used[:, 7], 0) - used[:, 7])
    assert int((used[:, 5] + 16 * used[:, 7]).max()) == w_pad > rc.PACK_N_COLS + 16 - 1
    assert int((ent[:, 7] == 0).sum()) == 1 and rc.PACK_NB % 4 == 0 and rc.PACK_NB // 4 == 3
