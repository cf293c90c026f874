"""The inputs, references and constants of tests/test_gpu_edge_geom.py and tests/test_gpu_node_kernels.py, as far as a machine
without a GPU can check them: the planted rows exist in the intended numbers, every committed fp32-torch constant is at
least the recomputed figure and at most twice it (a stale or hand-loosened constant fails here), rows are left out of a
comparison and reference blocks vanish only where the GPU files say so."""
import torch

import test_gpu_edge_geom as eg
import test_gpu_node_kernels as nk
from test_gpu_eval_grad import LAYOUTS, _blocks


def _within(committed, recomputed, what):
    assert recomputed <= committed <= 2.0 * recomputed, f"{what}: committed {committed:.3e}, recomputed {recomputed:.3e}"


# ---- edge geometry ------------------------------------------------------------------------------------------------------
def test_edge_cases_cover_every_axis_and_every_pair():
    cases = eg.CASES
    assert {c[0] for c in cases} == set(range(5)) and {c[1] for c in cases} == set(eg.CELLS)
    assert {c[3] for c in cases} == set(eg.ES) and {c[4] for c in cases} == set(eg.RBF)
    for lmax in (4, 2):
        assert {(c[3], c[2]) for c in cases if c[0] == lmax} == {(E, p) for E in eg.ES for p in (False, True)}
    assert {(c[1], c[4]) for c in cases} == {(a, b) for a in eg.CELLS for b in eg.RBF}
    assert len(set(cases)) == len(cases) <= 30


def test_edge_cases_hold_the_planted_edges():
    for case in eg.CASES:
        d = eg._edge_inputs(case)
        lmax, cells, permuted, E, (nb, r_start, r_end) = case
        ref = eg._edge_reference(d, torch.float64)
        r, v = ref["edge_lengths"], ref["edge_vectors"]
        src, dst = d["edge_index"]
        assert d["edge_index"].shape == (2, E) and d["shift"].shape == (E, 3)
        assert not ((src == eg.LONE_ATOM) | (dst == eg.LONE_ATOM)).any(), "one atom without an edge"
        assert (d["batch"][src] == d["batch"][dst]).all(), "edges stay inside their crystal"
        assert d["shift"].abs().max() <= 2 and (d["shift"] == d["shift"].round()).all()
        assert (d["perm"] is not None) == permuted
        if permuted:
            assert d["perm"].dtype == torch.int32 and torch.equal(d["perm"].long().sort().values, torch.arange(E))
        if E == 1:
            assert d["n_planted"] == 1 and 5e-5 < r[0] < 2e-4
            assert int(eg._excluded_rows(ref).sum()) == 0
            continue
        p = d["planted"]
        assert d["n_planted"] == (19 if cells != "none" else 16) and sum(t.numel() for t in p.values()) == d["n_planted"]
        # along +-x, +-y, +-z: two of the three components exactly 0, both signs of every axis
        assert p["axis"].numel() == 6 and ((v[p["axis"]] == 0).sum(1) == 2).all()
        assert {tuple(torch.sign(v[e]).long().tolist()) for e in p["axis"]} == \
            {(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)}
        assert p["tiny"].numel() == 2 and ((r[p["tiny"]] > 5e-5) & (r[p["tiny"]] < 2e-4)).all()
        # the cutoff, in the fp32 values the kernel sees
        r32 = r.float()
        assert p["below"].numel() == p["at"].numel() == p["above"].numel() == p["far"].numel() == 1
        assert r32[p["below"]] < r_end and r_end - r[p["below"]] < 2e-6
        assert r32[p["at"]] == r_end and r[p["at"]] == r_end
        assert r32[p["above"]] > r_end and r[p["above"]] - r_end < 1e-6
        assert r[p["far"]] == r_end + 1.5
        assert p["half"].numel() == 1 and r[p["half"]] == eg.R_START_PLANTED
        # zero-length edges: a self edge without a shift, two coincident atoms
        z = p["zero"]
        assert z.numel() == 3 and (r[z] == 0).all() and (d["shift"][z] == 0).all()
        assert int((src[z] == dst[z]).sum()) == 1 and int((r == 0).sum()) == 3
        if cells != "none":   # self images
            im = p["image"]
            assert im.numel() == 3 and (src[im] == dst[im]).all() and (d["shift"][im].abs().sum(1) > 0).all() and (r[im] > 0).all()
        # the rows left out of the embedding comparison are the planted ones of length r_start and nothing else
        placed = p["zero"] if r_start == 0.0 else p["half"]
        assert torch.equal(eg._excluded_rows(ref).nonzero()[:, 0], placed)
        assert int((r == r_start).sum()) == placed.numel()
        # no random edge sits within rounding of either end of the basis (the planted ones are exact)
        rand = torch.ones(E, dtype=torch.bool)
        rand[torch.cat(list(p.values()))] = False
        assert ((r[rand] - r_end).abs() > 1e-5).all() and ((r[rand] - r_start).abs() > 1e-5).all()
        assert int(((r > r_start) & (r < r_end)).sum()) >= 20, "enough edges inside the basis' support"


def test_edge_reference_blocks_vanish_only_where_listed():
    """l = 0 is the constant 1; every other degree block and every basis function has a non-zero scale, except the
    embedding of the single-edge cases' r_start = 0.5 basis (none among the cases) -- so no bound is 0 by accident"""
    for case in eg.CASES:
        d = eg._edge_inputs(case)
        ref = eg._edge_reference(d, torch.float64)
        assert (ref["edge_attrs"][:, 0] == 1).all()
        e = eg._edge_errors({k: v.float() for k, v in ref.items()}, ref, d)
        assert e["vec"][1] > 0 and e["len"][1] > 0
        assert all(scale > 0 for _, scale in e["sh"]) and all(scale > 0 for _, scale in e["emb"]), eg._case_id(case)
        z = d["planted"].get("zero")
        if z is not None:   # the oracle's row of a zero-length edge
            assert (ref["edge_attrs"][z][:, 1:] == 0).all()


def test_edge_constants_are_the_fp32_torch_errors():
    w = eg.fp32_torch_errors()
    c = eg.FP32_TORCH
    _within(c["vec"], w["vec"], "vectors")
    _within(c["len"], w["len"], "lengths")
    assert c["sh"][0] == 0.0 and w["sh"][0] == 0.0, "the l = 0 block is exact"
    for l in range(1, 5):
        _within(c["sh"][l], w["sh"][l], f"harmonics l={l}")
    for rbf in eg.RBF:
        _within(c["emb"][rbf], w["emb"][rbf], f"embedding {rbf}")
    assert eg.VEC_RTOL == 4 * c["vec"] and eg.LEN_RTOL == 4 * c["len"]
    assert eg.SH_RTOL == tuple(4 * v for v in c["sh"]) and eg.EMB_RTOL == {k: 4 * v for k, v in c["emb"].items()}


# ---- node kernels -------------------------------------------------------------------------------------------------------
def test_gate_cases_reach_every_activation_and_hold_the_planted_values():
    from matten_amd.nn.utils import ActivationLayer

    codes = set()
    for case in nk.GATE_CASES:
        layout, acts, n = case
        d = nk._gate_inputs(case)
        meta = ActivationLayer(*nk.GATE_LAYOUTS[layout], activation_type="gate", **nk._act_kwargs(acts)).plan.meta
        codes |= {int(r[2]) & 0xff for r in meta if r[1] < 0} | {(int(r[2]) >> 8) & 0xff for r in meta if r[1] >= 0}
        x = d["x"]
        assert x.shape[0] == n and sorted(d["scal"] + d["gates"]) == sorted(set(d["scal"]) | set(d["gates"]))
        assert bool(d["abs_gates"]) == (layout == "odd_gates" and acts == "layer")
        if n >= 37 and d["abs_gates"]:
            assert d["planted"]["abs_zero_rows"] == [2] and (x[2, d["abs_gates"]] == 0).all()
        else:
            assert d["planted"]["abs_zero_rows"] == []
        if n >= 1030:
            assert d["planted"]["big_rows"] == [3, 4, 5, 6]
            for r, v in zip((3, 4, 5, 6), nk.BIG):
                assert (x[r, d["scal"]] == v).all() and (x[r, d["gates"]] == -v).all()
            assert int((x.abs() >= 25).any(1).sum()) == 4
        else:
            assert d["planted"]["big_rows"] == [] and x.abs().max() < 20
        if n == 1:
            assert x.abs().min() >= nk.ONE_ROW_MIN
    assert set(LAYOUTS) < set(nk.GATE_LAYOUTS) and {c[2] for c in nk.GATE_CASES} == {1, 37, 1030}
    assert codes == {1, 2, 3, 4, 5}, codes


def test_norm_cases_hold_the_clamped_rows():
    for case in nk.NORM_CASES:
        layout, act, n = case
        d = nk._norm_inputs(case)
        x = d["x"].double()
        norms = torch.stack([x[:, off:off + dim].norm(dim=1) for off, dim in d["chans"]], 1)
        assert sum(dim for _, dim in d["chans"]) == x.shape[1]
        clamped = (norms < nk.NORM_EPS).all(1)
        assert ((norms < nk.NORM_EPS).any(1) == clamped).all(), "a row is clamped in every channel or in none"
        if n < 37:
            assert int(clamped.sum()) == 0 and d["compared"].all()
        elif act == "silu":
            assert d["rows"] == dict(zero=[1], above=[2], below=[3]) and clamped.nonzero()[:, 0].tolist() == [1, 3]
            assert (norms[1] == 0).all() and torch.allclose(norms[2], torch.full_like(norms[2], 3e-8), rtol=1e-5)
            assert torch.allclose(norms[3], torch.full_like(norms[3], 1e-9), rtol=1e-5)
            assert d["compared"].all(), "every silu row is compared"
        else:
            assert d["rows"] == dict(zero=[1], above=[], below=[]) and clamped.nonzero()[:, 0].tolist() == [1]
            assert (~d["compared"]).nonzero()[:, 0].tolist() == [1], "only the all-zero ssp row is left out"
        if act == "ssp":
            live = torch.ones(n, dtype=torch.bool)
            live[d["rows"]["zero"]] = False
            assert norms[live].min() >= 1e-2


def test_instance_norm_and_pooling_inputs():
    d = nk._inorm_inputs()
    sizes = nk.IN_SIZES
    assert sizes == [1, 2, 0, 7, 1000, 64, 1] and d["ptr"].tolist() == [0, 1, 3, 3, 10, 1010, 1074, 1075]
    assert torch.equal(torch.bincount(d["batch"], minlength=len(sizes)), torch.tensor(sizes))
    assert sizes.count(0) == 1 and sizes[0] == sizes[-1] == 1 and d["lone_rows"] == [0, 1074] and max(sizes) > 768
    assert (d["x"][:, :8].mean(0) - 5.0).abs().max() < 0.2 and d["x"][:, 8:].mean(0).abs().max() < 0.2
    assert ((d["weight"] >= 0.5) & (d["weight"] <= 1.5)).all() and d["bias"].numel() == nk.IN_SCALAR_COLS
    y, dx, dw, db = nk._inorm_reference(d, torch.float64)
    for r in d["lone_rows"]:
        assert (dx[r, :nk.IN_SCALAR_COLS] == 0).all() and torch.equal(y[r, :nk.IN_SCALAR_COLS], d["bias"].double())
    blocks, chans, scalars = nk._inorm_blocks(d["irreps"])
    for t, bl in ((y, blocks), (dx, blocks), (dw, chans), (db, scalars)):
        assert bl[-1][1] == t.shape[-1] and all(t[..., lo:hi].abs().max() > 0 for lo, hi, _ in bl), "no block vanishes"
    # pooling: the eight-row loop and its tail on both sides, one empty segment; the ties sit where the test says
    assert nk.POOL_SEGMENTS == [0, 1, 7, 8, 9, 64, 1000]
    for width in nk.POOL_WIDTHS:
        m = nk._minmax_inputs(width)
        x, ptr = m["x"], m["ptr"]
        for take_max in (False, True):
            vals, arg = nk._minmax_reference(m, take_max)
            assert (arg[0] == -1).all() and (vals[0] == 0).all() and (arg[1:] >= 0).all()
            for b in range(1, len(nk.POOL_SEGMENTS)):
                seg = x[int(ptr[b]):int(ptr[b + 1]), 0]
                n_ext = int((seg == (seg.max() if take_max else seg.min())).sum())
                assert n_ext == (2 if (b, take_max) in m["ties"] else 1)
                if (b, take_max) in m["ties"]:
                    assert int(arg[b, 0]) == m["ties"][(b, take_max)]
        assert len(m["ties"]) == 4
        s8, s9 = int(ptr[3]), int(ptr[4])
        signs = torch.signbit(torch.stack([x[s8 + 1, 0], x[s8 + 4, 0], x[s9 + 2, 0], x[s9 + 5, 0]])).tolist()
        assert signs == [True, False, False, True], "-0.0 against 0.0, either order"


def test_gather_scale_cases():
    ns = {(c[0], c[3]) for c in nk.GS_CASES}
    assert ns == {(n, q) for n in (1, 255, 257, 4 * nk.GS_PERIOD) for q in (False, True)}
    assert {c[2] for c in nk.GS_CASES} == {False, True}
    assert all(n % p == 0 for n, p, _, q in nk.GS_CASES if q)
    assert (4 * nk.GS_PERIOD, nk.GS_PERIOD, True, True) in nk.GS_CASES


def test_node_constants_are_the_fp32_torch_errors():
    w = nk.fp32_torch_errors()
    assert set(w) == set(nk.CONSTANTS)
    for k, v in nk.CONSTANTS.items():
        _within(v, w[k], k)
        assert nk.RTOL[k] == 4 * v
    # every compared block of the gate / norm references has a scale of its own
    for case in nk.GATE_CASES:
        d = nk._gate_inputs(case)
        y, dx = nk._module_reference(d["ref"], d["x"], d["dy"], torch.float64)
        assert all(y[:, lo:hi].abs().max() > 0 for lo, hi, _ in _blocks(d["ref"].irreps_out))
        assert all(dx[:, lo:hi].abs().max() > 0 for lo, hi, _ in _blocks(d["ref"].irreps_in))
