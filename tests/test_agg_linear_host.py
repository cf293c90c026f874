"""The streaming lin2's plan (plan.plan_agg_linear / plan_agg_gate) walked on the host: agg_linear_cases.emulate does in
numpy what matten_agg_linear does with the tables -- block list, K mask, A-fragment indexing, stage and flush -- for every
single-layer case of agg_linear_cases against the oracle in fp64.  No GPU; test_gpu_agg_linear.py runs the same cases on
the kernel."""
import numpy as np
import pytest
import torch

import agg_linear_cases as alc
from matten_amd import plan as mplan

S = 3
HOST_RTOL = 1e-6   # per block: the bound test_agg_linear_plan_reproduces_lin2_on_the_host uses (fp64 sums, fp32 table)


def _check_blocks(out, want, blocks, what):
    for lo, hi, name in blocks:
        scale = np.abs(want[:, lo:hi]).max()
        err = np.abs(out[:, lo:hi] - want[:, lo:hi]).max()
        assert scale > 0 and err <= HOST_RTOL * scale, f"{what} block {name}: {err:.2e} vs block max {scale:.2e}"


def _emulated_lin2(lay, N=7, add=False):
    species = np.random.default_rng(1).integers(0, S, N)
    agg, w = alc.make_inputs(lay, species)
    row, written = alc.scatter_rows(lay, agg)
    ap = lay.ap
    # the entries are a bijection onto the written slots; nothing else is finite
    assert written.max() == 1 and written.sum() == lay.uvu.d_mid
    assert (np.isfinite(row[0]) == (written == 1)).all() and not written[16 * ap.n_chunks:].any()
    assert ap.ld % 32 == 0 and 16 * ap.n_chunks <= ap.ld
    addend = np.random.default_rng(2).standard_normal((N, ap.d_out)).astype(np.float32) if add else None
    out, stores = alc.emulate(ap, row, alc.make_wtab(ap, w), species, add=addend)   # (asserts that no read slot is NaN)
    assert (stores == 1).all()                                                     # every output column leaves once
    return species, agg, w, addend, out


@pytest.mark.parametrize("name", list(alc.CASES))
def test_emulated_walk_matches_fp64_lin2(name):
    lay = alc.layer(name, S)
    species, agg, w, _, out = _emulated_lin2(lay)
    want = alc.reference_lin2(lay, agg, species, w).numpy()
    _check_blocks(out, want, alc.irrep_blocks(lay.irreps_out), name)


@pytest.mark.parametrize("name", list(alc.GATED))
def test_emulated_gate_epilogue_matches_fp64_gate_and_batchnorm(name):
    """lin2 for the Gate's input irreps, then the epilogue as cmeta describes it (activated scalars, gates parked per
    register set and lane, gated components, BatchNorm folded into scale / shift) against the oracle's Gate + BatchNorm"""
    lay = alc.layer(name, S, gated=True)
    species, agg, w, addend, conv = _emulated_lin2(lay, add=True)
    want_conv = alc.reference_lin2(lay, agg, species, w).numpy() + addend
    _check_blocks(conv, want_conv, alc.irrep_blocks(lay.irreps_out), name + " lin2")
    cm = lay.cmeta
    assert cm.shape == (lay.ap.d_out, 4) and set((cm[:, 0] & 255).tolist()) <= {1, 2, 3}
    n_gates = int(((cm[:, 0] & 255) == 2).sum())
    assert n_gates == lay.gate.irreps_gates.dim
    blocks = alc.irrep_blocks(lay.gate.irreps_out)
    got = alc.emulate_gate(lay, conv)
    _check_blocks(got, alc.reference_gated(lay, agg, species, w, add=addend).numpy(), blocks, name + " gate")
    bn = alc.oracle_batchnorm(lay)
    scale, shift = alc.fold_batchnorm(lay, bn)
    got = alc.emulate_gate(lay, conv, scale.double().numpy(), shift.double().numpy())
    _check_blocks(got, alc.reference_gated(lay, agg, species, w, add=addend, bn=bn).numpy(), blocks, name + " gate + bn")


@pytest.mark.parametrize("name", list(alc.GATED))
def test_production_batchnorm_folding_matches_the_written_out_one(name):
    """PointConvWithActivation._fold_bn (what production hands the kernel) against agg_linear_cases.fold_batchnorm (what
    the kernel tests hand it); no_scalars has no 0e channel: empty running_mean / bias, which _fold_bn once indexed"""
    from types import SimpleNamespace

    from matten_amd.nn.conv import PointConvWithActivation

    lay = alc.layer(name, S, gated=True)
    bn = alc.oracle_batchnorm(lay)
    stub = SimpleNamespace(act=SimpleNamespace(plan=lay.gate), norm=SimpleNamespace(n=bn))
    scale, shift = PointConvWithActivation._fold_bn(stub, bn.running_mean, bn.running_var, bn.weight.detach(), bn.bias.detach())
    want_scale, want_shift = alc.fold_batchnorm(lay, bn)
    assert torch.equal(scale, want_scale) and torch.equal(shift, want_shift)
    assert scale.shape == (lay.gate.irreps_out.dim,) and bool(shift.any()) == (bn.bias.numel() > 0)


def test_gate_sets_reached_by_the_gated_cases():
    """what the case table promises: gates_65 fills all three register sets, gates_25 has a set holding one gate,
    no_scalars no activated scalar, scalars_only no gate"""
    def sets(name):
        cm = alc.layer(name, S, gated=True).cmeta
        g = cm[(cm[:, 0] & 255) == 2]
        return np.bincount(g[:, 3], minlength=mplan.AGG_GATE_SETS).tolist() if len(g) else []

    assert sum(sets("paper_like")) == 46 and sets("paper_like")[2] == 0 and min(sets("paper_like")[:2]) > 0
    assert sum(sets("gates_65")) == 65 and min(sets("gates_65")) > 0
    assert sets("gates_33") == [24, 9, 0] and sets("gates_25") == [24, 1, 0]
    assert sets("scalars_only") == [] and sum(sets("tiny")) == 1
    assert not ((alc.layer("no_scalars", S, gated=True).cmeta[:, 0] & 255) == 1).any()
    assert "0o" in str(alc.layer("odd_scalars", S, gated=True).gate.irreps_scalars)


def test_table_shapes_reached_by_the_cases():
    """the branches the case table names are really in the plans (a planner change that moves them must move the cases)"""
    def rows(name):
        return [alc.unpack_io(r) for r in alc.layer(name, S).ap.io_table]

    assert {r["T"] for r in rows("paper_like")} >= {2, 4, 5} and {r["n_mt"] for r in rows("paper_like")} == {1, 2}
    assert [r["mo"] for r in rows("wide_scalars")][:3] == [32, 32, 16]
    assert len({r["c0"] for r in rows("wide_scalars")[:3]}) == 1                     # ... that re-read the same chunks
    assert any(r["mo"] == 17 and r["kk"] == 1 for r in rows("mo17")) and any(r["cw"] == 5 for r in rows("mo17"))
    assert [r["mo"] for r in rows("mo33")][:2] == [32, 1]
    assert {r["cw"] for r in rows("mo12_d3")} == {12, 7, 3} and {r["K"] for r in rows("mo12_d3")} >= {14, 20, 22}
    assert {r["K"] for r in rows("K_small")} == {2}
    assert min(r["T"] for r in rows("K_big")) > 3 * mplan.AGG_BLOCK and alc.layer("K_big", S).ap.ld == 7488
    assert alc.layer("tiny", S).ap.w_stride == 32 and {r["K"] for r in rows("tiny")} == {1}


def test_layouts_the_planners_refuse():
    in1, target, sh = alc.REFUSED_GATE
    lay = alc.plan_case(in1, target, sh, S, gated=True)
    assert lay.ap is not None and lay.gate.irreps_gates.dim == 97 and lay.cmeta is None   # 97 gates exceed 3 sets of 32
    in1, out, sh = alc.REFUSED_AGG
    assert alc.plan_case(in1, out, sh, S).ap is None                                      # alignment holes


def test_lds_sizes_of_the_large_layouts():
    """lds_79k sits between the 64 KB default and the kernel's 80 KB cap (the launcher raises the attribute), the
    48x0e variant above the cap (refused): hand-computed from the plan, and equal to the library's count where it loads"""
    def by_hand(ap):   # A fragments + io rows (8 ints) + blocks (4 ints) + 8 waves x (16 x 33 stage + 16 row ids)
        return 4 * ap.w_stride + 32 * len(ap.io_table) + 16 * len(ap.blocks) + 4 * 8 * (16 * 33 + 16)

    a79 = alc.layer("lds_79k", 2).ap
    over = alc.plan_case(*alc.LDS_OVER, 2).ap
    assert by_hand(a79) == alc.LDS_79K_BYTES and 64 * 1024 < alc.LDS_79K_BYTES <= 80 * 1024
    assert by_hand(over) == alc.LDS_OVER_BYTES and alc.LDS_OVER_BYTES > 80 * 1024
    assert by_hand(alc.layer("lds_79k", S).ap) == alc.LDS_79K_BYTES      # (the species count does not enter)
    try:
        from matten_amd import _lib

        lib = _lib.load()
    except Exception:  # noqa: BLE001  (no library on this machine: the hand count stands alone)
        return
    for ap, want in ((a79, alc.LDS_79K_BYTES), (over, alc.LDS_OVER_BYTES)):
        assert lib.matten_agg_linear_lds_bytes(ap.w_stride, len(ap.io_table), len(ap.blocks)) == want
    assert lib.matten_agg_linear_max_lds_bytes() == 80 * 1024
