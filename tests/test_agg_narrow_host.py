"""The narrowed neighbour-sum row (plan.plan_agg_narrow) walked on the host, in the style of test_agg_linear_host.py: the writer
(matten_tp_fused_narrow's epilogue: a narrowed coupling leaves as sum_u Wn[species][u][v] * sum[u][k], mo floats per component)
and the unchanged reader (agg_linear_cases.emulate = matten_agg_linear's walk of the tables) in fp64 numpy against the oracle's
FullyConnectedTensorProduct of the mul_ir sums.  No GPU; test_gpu_agg_narrow.py runs the kernels.

Also held here: plan_agg_linear itself returns what it returned before the narrowed planner was added (digests of its arrays
for every case of agg_linear_cases, recorded from the parent commit in tests/golden/agg_linear_plan_digests.json), the Gate
assignment does not depend on the layout, and the row length equals a count made from the instruction list alone.

For the operator-level GPU file test_gpu_tp_narrow.py: its case table (agg_narrow_cases.py) reaches exactly the 54 template
instances the planner can emit, its cases pass the host walk, and a record that does not fit the bit fields of the packed
entry words gives no plan instead of wrapped words."""
import hashlib
import json
import os

import numpy as np
import pytest

import agg_linear_cases as alc
import agg_narrow_cases as anc
from common import LMAX2, PAPER
from matten_amd import plan as mplan

HOST_RTOL = 1e-6   # per block, as test_agg_linear_host.py (fp64 sums of fp32 tables)
SH2 = "0e+1o+2e"
# the inference view of the paper model's last conv layer: the output irreps the head (16x0e+2x2e+4e) reads, at the layer's
# own multiplicities (model_factory.eliminate_dead_outputs)
_HEAD = {str(ir) for _, ir in mplan.Irreps(PAPER["conv_to_output_hidden_irreps_out"])}
VIEW = "+".join(f"{m}x{ir}" for m, ir in mplan.Irreps(PAPER["conv_layer_irreps"]) if str(ir) in _HEAD)
assert VIEW == "32x0e+4x2e+2x4e", VIEW

# id -> (irreps_in1, target, harmonics, gated, species)
LAYERS = {
    "paper_gated_S3": (PAPER["conv_layer_irreps"], PAPER["conv_layer_irreps"], alc.SH4, True, 3),
    "paper_gated_S1": (PAPER["conv_layer_irreps"], PAPER["conv_layer_irreps"], alc.SH4, True, 1),
    "lmax2_gated_S3": (LMAX2["conv_layer_irreps"], LMAX2["conv_layer_irreps"], SH2, True, 3),
    "paper_view_S3": (PAPER["conv_layer_irreps"], VIEW, alc.SH4, False, 3),
    "paper_like_S3": (*alc.CASES["paper_like"], False, 3),
}
# the operator-level cases of test_gpu_tp_narrow.py: 8-lane scalar entries, 16-lane vector entries, mo = 1, every D3
LAYERS.update({name: (in1, target, anc.SH4, False, 3) for name, (in1, target, _) in anc.CASES.items()})


def _layer(name):
    """(Layer with the plain plan, Layer with the narrowed plan)"""
    in1, target, sh, gated, S = LAYERS[name]
    lay = alc.plan_case(in1, target, sh, S, gated, name)
    assert lay.ap is not None
    apn = mplan.plan_agg_narrow(lay.uvu, S, lay.irreps_out)
    assert apn is not None and apn.narrow is not None, name
    cm = mplan.plan_agg_gate(apn, lay.gate) if gated else None
    return lay, alc.Layer(name, S, lay.uvu, apn, lay.irreps_out, lay.gate, cm)


_narrow_weights, _wtab = anc.narrow_weights, anc.wtab      # (shared with test_gpu_tp_narrow.py)


def _write_rows(lay, agg, species, w):
    """the writer: agg_linear_cases.scatter_rows, but a narrowed coupling's cu lanes leave partial[v][k] at out_off + v + k t_off"""
    uvu, ap = lay.uvu, lay.ap
    row = np.full((agg.shape[0], ap.ld), np.nan)
    written = np.zeros(ap.ld, dtype=np.int64)
    # read the way the kernel reads: everything from the entry record inside the one buffer of plan.narrow_blob
    blob = mplan.narrow_blob(ap, _narrow_weights(ap, w))
    n = len(ap.entries)
    assert blob.dtype == np.int32 and blob.size == 32 * n + ap.narrow_gather.size
    ent = blob[: 32 * n].reshape(-1, 32)
    assert np.array_equal(ent, ap.entries)
    for e in range(n):
        mul = int(uvu.group_entry_mul[e])
        u = np.arange(mul)
        for c, pi in uvu.group_entry_paths[e].items():
            pth = uvu.paths[pi]
            d3 = 2 * pth.l3 + 1
            ks, o, mo, rel = mplan.narrow_unpack(ent[e][8 + c], ent[e][20 + c])
            src = agg[:, pth.out_off + (uvu.group_entry_u0[e] + u)[:, None] * d3 + np.arange(d3)[None, :]].astype(np.float64)  # [N, u, k]
            nw = int(ap.narrow[e][c])
            assert (nw & 255) == mo and (mo == 0 or 32 * e + rel == 32 * n + (nw >> 8))     # the host-side table says the same
            if mo == 0:
                for k in range(d3):
                    row[:, o + u + k * ks] = src[:, :, k]
                    np.add.at(written, o + u + k * ks, 1)
                continue
            assert int(ent[e][0]) & mplan.TP_KIND_NARROW and int(ent[e][0]) & mplan.TP_KIND_WREG
            assert (1 << int(ent[e][3])) == mul == int(ent[e][2]) and mul in (8, 16) and mo in (1, 2, 4)
            assert rel % 4 == 0 and o % mo == 0 and ks % 16 == 0     # 16-byte loads of the weights, one aligned piece per (node, k)
            base = 32 * e + rel
            blk = blob[base: base + lay.S * mul * mo].view(np.float32).astype(np.float64).reshape(lay.S, mul, mo)[species]   # [N, u, v]
            part = np.einsum("nuv,nuk->nvk", blk, src)
            for k in range(d3):
                row[:, o + np.arange(mo) + k * ks] = part[:, :, k]
                np.add.at(written, o + np.arange(mo) + k * ks, 1)
    return row, written


def _check_blocks(out, want, blocks, what):
    for lo, hi, name in blocks:
        scale = np.abs(want[:, lo:hi]).max()
        err = np.abs(out[:, lo:hi] - want[:, lo:hi]).max()
        assert scale > 0 and err <= HOST_RTOL * scale, f"{what} block {name}: {err:.2e} vs block max {scale:.2e}"


@pytest.mark.parametrize("name", list(LAYERS))
def test_narrowed_writer_and_unchanged_reader_match_fp64_lin2(name):
    _, lay = _layer(name)
    _walk_writer_and_reader(lay, name, 9)


def _walk_writer_and_reader(lay, name, N):
    ap = lay.ap
    species = np.random.default_rng(1).integers(0, lay.S, N)
    agg, w = alc.make_inputs(lay, species)
    row, written = _write_rows(lay, agg, species, w)
    # every slot below a region's K is written exactly once, nothing else is
    want_written = np.zeros(ap.ld, dtype=np.int64)
    for c0, T, K, d3 in {(int(r[0]), int(r[1]), int(r[2]), int(r[3]) & 255) for r in ap.io_table}:
        for k in range(d3):
            want_written[16 * (c0 + k * T): 16 * (c0 + k * T) + K] = 1
    assert (written == want_written).all() and not written[16 * ap.n_chunks:].any()
    assert (np.isfinite(row[0]) == (written == 1)).all()
    assert ap.ld % 32 == 0 and 16 * ap.n_chunks <= ap.ld
    out, stores = alc.emulate(ap, row.astype(np.float64), _wtab(ap, w), species)   # (asserts that no read slot is NaN)
    assert (stores == 1).all()
    want = alc.reference_lin2(lay, agg, species, w).numpy()
    _check_blocks(out, want, alc.irrep_blocks(lay.irreps_out), name)


@pytest.mark.parametrize("name", [n for n in LAYERS if LAYERS[n][3]])
def test_gate_assignment_does_not_depend_on_the_layout(name):
    plain, narrow = _layer(name)
    assert plain.cmeta is not None and narrow.cmeta is not None
    assert np.array_equal(plain.cmeta, narrow.cmeta)


def _count_from_instructions(uvu, irreps_out):
    """floats of data per row and the row stride, from the paths and the entries' channel counts alone: a coupling of a full
    8- or 16-lane entry of a scalar or vector input block whose output irrep has mo in {1, 2, 4} < mul channels takes mo slots
    per component, every other one its channels"""
    out = mplan.Irreps(irreps_out).simplify()
    K, _ = _slots_per_irrep(uvu, out)
    data = sum(K[io] * out[io].ir.dim for io in K)
    chunks = sum(-(-K[io] // 16) * out[io].ir.dim for io in K)
    return data, -(-(16 * chunks) // 32) * 32


def _slots_per_irrep(uvu, out):
    """({output irrep: channel slots per component}, {output irrep: it has a narrowed piece}) by the rule above"""
    K, narrowed = {}, {}
    for e, paths in enumerate(uvu.group_entry_paths):
        mul, lanes = int(uvu.group_entry_mul[e]), 1 << int(uvu.group_entries[e][3])
        for c, pi in paths.items():
            p = uvu.paths[pi]
            (io, mo), = [(i, int(m)) for i, (m, ir) in enumerate(out) if (ir.l, ir.p) == (p.l3, p.p3)]
            narrow = p.l1 <= 1 and mul == lanes and mul in (8, 16) and mo < mul and mo in (1, 2, 4)
            K[io] = K.get(io, 0) + (mo if narrow else mul)
            narrowed[io] = narrowed.get(io, False) or narrow
    return K, narrowed


def test_row_length_equals_the_count_from_the_instruction_list():
    plain, narrow = _layer("paper_gated_S3")
    data, ld = _count_from_instructions(plain.uvu, plain.irreps_out)
    assert data == 2326 and ld == narrow.ap.ld == 2560          # layers 1 and 2 of the paper model: 4170 floats before
    assert sum(int(r[2]) * (int(r[3]) & 255) for r in {int(r[0]): r for r in narrow.ap.io_table}.values()) == data
    assert sum(int(r[2]) * (int(r[3]) & 255) for r in {int(r[0]): r for r in plain.ap.io_table}.values()) == 4170
    assert plain.ap.ld == 4352
    for name in ("lmax2_gated_S3", "paper_view_S3"):
        plain, narrow = _layer(name)
        assert _count_from_instructions(plain.uvu, plain.irreps_out)[1] == narrow.ap.ld < plain.ap.ld


def test_layers_nothing_narrows_in_keep_the_plain_plan():
    lay = alc.layer("wide_scalars", 3)          # 80x0e + 16x1o outputs: no output irrep narrower than its inputs' entries
    assert mplan.plan_agg_narrow(lay.uvu, 3, lay.irreps_out) is None
    assert mplan.plan_agg_narrow(alc.plan_case(*alc.REFUSED_AGG, 3).uvu, 3, mplan.Irreps(alc.REFUSED_AGG[1]).simplify()) is None


def _digest(ap):
    h = hashlib.sha256()
    for name in ("entries", "io_table", "blocks", "gather", "scale"):
        a = np.ascontiguousarray(getattr(ap, name))
        h.update(f"{name}:{a.dtype}:{a.shape}".encode())
        h.update(a.tobytes())
    h.update(repr((ap.ld, ap.n_chunks, ap.w_stride, ap.d_out, ap.max_mt)).encode())
    return h.hexdigest()


def test_plan_agg_linear_returns_what_it_returned_before(golden_dir):
    """entries, io_table, blocks, gather, scale and the scalars of every case of agg_linear_cases, one and three species"""
    with open(os.path.join(golden_dir, "agg_linear_plan_digests.json")) as f:
        want = json.load(f)
    got = {}
    for S in (1, 3):
        for name in alc.CASES:
            got[f"{name}/S{S}"] = _digest(alc.layer(name, S).ap)
        for name in alc.GATED:
            got[f"gated:{name}/S{S}"] = _digest(alc.layer(name, S, gated=True).ap)
    assert got == want
    ap = alc.layer("paper_like", 3).ap
    assert ap.narrow is None and ap.narrow_gather is None and not (ap.entries[:, 0] & mplan.TP_KIND_NARROW).any()
    assert ap.gather.min() == -1                  # (no sentinel in a plain plan)


# ---- the operator-level case table -------------------------------------------------------------------------------------------
def test_case_table_reaches_every_instance_the_planner_emits():
    """the mirror of test_gpu_tp_narrow.py's coverage assertion: the (input l1, lanes per node, D3, mo) of the narrowed
    couplings of agg_narrow_cases.CASES are exactly the 54 instances; a case dropped there shows here, without a GPU"""
    anc.assert_every_instance_has_a_case()
    assert anc.instances("s8_1") >= {(0, 8, d3, 1) for d3 in (1, 3, 5, 7, 9)}                  # 8-lane scalar entries, mo = 1
    assert anc.instances("even_4") >= {(1, 16, d3, 4) for d3 in (1, 5, 9)}                     # 16-lane vector entries
    assert {mo for _, _, _, mo in anc.instances("head2")} == {1, 2}                            # mixed mo in one plan
    assert all(S == 3 for n, S in anc.PARAMS if n != "full_2") and {S for n, S in anc.PARAMS if n == "full_2"} == {1, 3, 5}
    # view: narrowed and un-narrowed couplings side by side in one entry
    uvu, ap = anc.uvu_plan("view"), anc.narrow_plan("view", 3)
    per_entry = {}
    for e, _, _, _, _, mo in anc.couplings(uvu, ap):
        per_entry.setdefault(e, set()).add(bool(mo))
    assert any(v == {True, False} for v in per_entry.values())
    for name, S in anc.PARAMS:                                        # far from the packed words' limits
        uvu, ap = anc.uvu_plan(name), anc.narrow_plan(name, S)
        _assert_words_round_trip(uvu, ap, S)
        assert max(o for *_, o, mo in anc.couplings(uvu, ap) if mo) <= 2606


# ---- the packed words ---------------------------------------------------------------------------------------------------------
def _assert_words_round_trip(uvu, ap, S):
    """the two words of every coupling unpack to what the host-side table says, every field inside its bits, the weight block
    inside the buffer of plan.narrow_blob; nothing reaches the sign bit"""
    n = len(ap.entries)
    for e, c, _, ks, o, mo in anc.couplings(uvu, ap):
        nw, t, ow = int(ap.narrow[e][c]), int(ap.entries[e][8 + c]), int(ap.entries[e][20 + c])
        assert t >= 0 and ow >= 0
        if not nw:
            assert mo == 0 and t < 1 << 20        # (a plain word must not read as a narrowed one)
            continue
        rel = mplan.narrow_unpack(t, ow)[3]
        assert mo == nw & 255 and 32 * e + rel == 32 * n + (nw >> 8)
        assert rel // 4 < 1 << 15 and o < 1 << 16 and ks < 1 << 20 and o + (mo - 1) < ap.ld
        assert 32 * e + rel + S * int(uvu.group_entry_mul[e]) * mo <= 32 * n + ap.narrow_gather.size


def test_weight_distance_past_its_field_gives_no_plan():
    """a narrowed coupling's weight block lies rel floats behind its entry, rel / 4 in 15 bits: full_4's 2816 S floats of
    writer weights pass 2^17 between S = 46 and 47.  Below: a plan whose words round-trip; from there on None, never a
    wrapped distance (the caller keeps the plain plan)"""
    uvu, target = anc.uvu_plan("full_4"), anc.CASES["full_4"][1]
    ap3 = anc.narrow_plan("full_4", 3)
    n = len(ap3.entries)
    first = [(e, c, int(ap3.narrow[e][c]) >> 8) for e in range(n) for c in range(ap3.narrow.shape[1]) if ap3.narrow[e][c]]
    assert all(w % 3 == 0 for _, _, w in first)        # blocks [species][u][v]: every offset is a multiple of S

    def need(S):
        return max(32 * (n - e) + w // 3 * S for e, _, w in first)

    assert need(46) < 1 << 17 <= need(47)
    for S in (40, 45, 46, 47, 48, 64, 200):
        ap = mplan.plan_agg_narrow(uvu, S, target)
        if need(S) >= 1 << 17:
            assert ap is None, S
            continue
        assert ap is not None, S
        _assert_words_round_trip(uvu, ap, S)
        assert max(mplan.narrow_unpack(ap.entries[e][8 + c], ap.entries[e][20 + c])[3] for e, c, _ in first) == need(S)


WIDE_TARGET = "32x0e+32x0o+16x1o+16x1e+16x2e+16x2o+16x3o+16x3e+1x4e+1x4o"    # only 4e and 4o narrow: the END of the row


def _wide(mul):
    in1 = f"{mul}x0e+{mul}x0o+{mul // 2}x1o+{mul // 2}x1e"
    lay = alc.plan_case(in1, WIDE_TARGET, alc.SH4, 1, False, f"wide_{mul}")
    out = lay.irreps_out
    K, narrowed = _slots_per_irrep(lay.uvu, out)
    start, starts = 0, {}
    for io, (_, ir) in enumerate(out):                  # regions in the order of lin2's output irreps, [component][Kpad]
        starts[io] = start
        start += 16 * -(-K[io] // 16) * ir.dim
    return lay, max(starts[io] for io in K if narrowed[io])


def test_row_offset_past_its_field_gives_no_plan():
    """a narrowed piece's first float has 16 bits.  A synthetic layer (816 / 832 scalar channels per parity, a wide target
    whose only narrow irreps are the last two) puts the narrowed regions just below / above float 2^16 of the row: below, a
    plan whose words round-trip and whose writer and reader walk to the fp64 lin2; above, None.  (The third field, floats
    between components < 2^20, needs a region of a million channel slots: no irreps within the planner's other limits reach
    it; _assert_words_round_trip pins it for every plan seen here.)"""
    lay, start = _wide(816)
    assert (1 << 16) - 1024 <= start < 1 << 16
    ap = mplan.plan_agg_narrow(lay.uvu, 1, lay.irreps_out)
    assert ap is not None and ap.ld > 1 << 16
    _assert_words_round_trip(lay.uvu, ap, 1)
    assert start <= max(o for *_, o, mo in anc.couplings(lay.uvu, ap) if mo) < 1 << 16
    _walk_writer_and_reader(alc.Layer(lay.name, 1, lay.uvu, ap, lay.irreps_out, None, None), lay.name, 2)
    lay, start = _wide(832)
    assert start >= 1 << 16 and lay.ap is not None
    assert mplan.plan_agg_narrow(lay.uvu, 1, lay.irreps_out) is None
