"""
The narrowed neighbour sums (matten_tp_fused_narrow: narrow_sum, narrow_coupling, store_narrow of csrc/tp_fused.hip) at the
operator level, per narrowed piece against fp64, and matten_agg_linear reading the rows the kernel wrote.

    row[n][out_off + v + k * t_off] = sum_u Wn[species(n)][u][v] * agg[n][path][u0 + u][k],   v < mo, k < D3

for every (entry, coupling) the plan narrows (lin2 applied by the entry's 8 or 16 channel lanes before the sums leave); every
other coupling leaves its channels as plan_agg_linear's component-major row.  agg: test_gpu_tp_forward's operator.

Cases (agg_narrow_cases.CASES): together they reach all 54 (input l1, lanes per node, D3, mo) instances the planner can emit
at sh lmax 4 -- asserted by the `built` fixture and, without a GPU, by test_agg_narrow_host.py.  Graph: the 70 nodes of
test_gpu_agg_narrow (one 64-node tile and a partial one, in-degrees 0, 1, 5, 19, 40, 910 shuffled edges), species drawn at
random per node (every wave of 4 nodes holds at least two), both normalisations (num_neigh = 0 where nothing arrives).
Operands: test_gpu_tp_forward._operands (NaN pad columns of the harmonics, NaN rows of x that nothing reads, h2_eff rebuilt
from the kernel's own fp16 halves), a flat lin2 weight of fp32 normals, packed as PointConv packs it.

Reference: the oracle's tensor product in fp64 + scatter + normalisation (test_gpu_tp_forward._reference), then for a narrowed
piece the output-irrep block of the oracle's lin2 (agg_linear_cases.reference_lin2) on a copy of the sums in which every
column but that path's channels u0 .. u0 + mul is zero.  narrow_gather, narrow_scale and the weights behind the entries are
not used for the values; the entry words only say where the piece sits (plan.narrow_unpack).  The same in fp32 gives r32: the
largest distance of the fp32 from the fp64 reference over the pieces, relative to the piece's maximum.

Every narrowed piece, and every path's un-narrowed slots, are compared with THEIR OWN largest |reference| over the nodes
with in-edges; allowed: min(2e-5, 8 r32) of it (FWD_RTOL, R32_FACTOR of test_gpu_tp_forward: both references apply the same
extra product and additions, so no new factor).  Slots no entry writes are still NaN, written ones finite, rows of nodes
nothing arrives at exactly 0, two launches the same bits, the entry-major walk the same bits in the scalar-input entries'
slots and inside the same bound everywhere.  Nothing here is derived from the kernel's own error.

The reader: the kernel-written row through ops.agg_linear with PointConv._pack_agg_weights' table (sentinel -> 1.0), per
output irrep block and species against reference_lin2 of the fp64 sums, with test_gpu_agg_linear's rule
(agg_linear_cases.block_errors: 2e-6 of the block's maximum or 4 x the fp32 oracle's distance).

r32 (it does not depend on the kernel): 2.3e-7 .. 5.1e-7 over the cases, i.e. 1.9e-6 .. 4.1e-6 of a piece's maximum allowed.

Worst error / allowed, measured on MI355X: every checked group / the narrowed pieces alone (the worst group of a case with
l1 >= 2 entries is an un-narrowed block of the heaviest kind, path 4,4,4 or 4,4,2, as in test_gpu_tp_forward):
                 avg              node             r32 avg / node
    full_1-S3    0.26 / 0.13      0.18 / 0.14      3.6e-7 / 3.5e-7
    full_2-S3    0.18 / 0.093     0.19 / 0.13      5.1e-7 / 3.3e-7
    full_2-S1    0.27 / 0.17      0.22 / 0.14      3.4e-7 / 2.9e-7
    full_2-S5    0.24 / 0.13      0.18 / 0.12      3.9e-7 / 3.7e-7
    full_4-S3    0.26 / 0.14      0.16 / 0.099     3.6e-7 / 4.0e-7
    even_1-S3    0.36 / 0.14      0.30 / 0.11      2.6e-7 / 2.6e-7
    even_2-S3    0.30 / 0.12      0.33 / 0.14      3.1e-7 / 2.3e-7
    even_4-S3    0.34 / 0.11      0.16 / 0.064     2.8e-7 / 4.9e-7
    s8_1-S3      0.15 / 0.15      0.096 / 0.096    3.2e-7 / 4.7e-7     (every coupling of these plans is narrowed)
    s8_2-S3      0.25 / 0.25      0.16 / 0.16      3.8e-7 / 3.2e-7
    s8_4-S3      0.18 / 0.18      0.12 / 0.12      3.7e-7 / 3.4e-7
    view-S3      0.26 / 0.10      0.22 / 0.084     3.6e-7 / 3.5e-7
    head2-S3     0.33 / 0.13      0.32 / 0.15      2.9e-7 / 2.4e-7
The entry-major walk gives the same worst figures but for s8 (0.20, 0.17, 0.18 with avg; 0.096, 0.16, 0.12 per node: its vector
entries sum edge pairs in another association).  No case came near the bound and no kernel or planner change was needed.
The reader on the kernel-written rows, worst fraction of the allowed distance avg / node (worst |error| / block maximum):
    full_1 0.22 / 0.16 (4.4e-7)   full_4 0.27 / 0.21 (5.4e-7)   view 0.20 / 0.16 (4.1e-7)   head2 0.15 / 0.14 (2.9e-7)

Controls (test_controls_are_seen: in-bounds mutations of the operands handed to the unchanged kernel, full_2-S3; the
unmutated launch passes at 0.18 / 0.19): worst piece in units of the allowed distance, pieces outside of 116 checked groups
    species of two nodes of one wave swapped          2.6e5    68   (every narrowed piece; the un-narrowed blocks do not move)
    one writer weight x (1 + 1e-3)                    141       1   (entry 0, coupling 4: path 0,4,4, channels 0..15)
    weight blocks of two species of one coupling      3.6e5     1   (entry 4, coupling 3: path 1,1,2, channels 0..7)
    num_neigh exchanged between neighbouring nodes    4.6e5   116
    out_off low halves of two couplings swapped       3.1e5     2   (path 0,0,0, channels 0..15 and 16..31)
"""
import dataclasses

import numpy as np
import pytest
import torch

import agg_linear_cases as alc
import agg_narrow_cases as anc
from test_gpu_agg_narrow import DEGREES, N_NODES, _graph as _graph_70
from test_gpu_tp_forward import (AVG, DEV, FWD_RTOL, R32_FACTOR, Case, _nan_prefill, _operands, _oracle_tp_of, _ratio,
                                 _reference)

pytestmark = pytest.mark.gpu

NORMS = ("avg", "node")
LMAX = 4
PIECE_BATCH = 12          # narrowed pieces per call of the oracle's lin2 (rows = pieces x nodes)
SPECIES_SEED = {1: 0, 3: 1, 5: 0}      # per species count: the first draw in which every wave of 4 nodes holds two species (asserted)
READER = ("full_1", "full_4", "view", "head2")
CASES = [(name, S, norm) for name, S in anc.PARAMS for norm in NORMS]


def _ids(cases):
    return [f"{c[0]}-S{c[1]}" + "".join(f"-{x}" for x in c[2:]) for c in cases]


def _species(S):
    sp = np.random.default_rng(SPECIES_SEED[S]).integers(0, S, N_NODES)
    if S > 1:
        # the 16-lane entries run 4 nodes per wave, the 8-lane ones 8: no wave of the full tile reads one species only
        assert all(len(set(sp[n: n + 4].tolist())) >= 2 for n in range(0, 64, 4)), "a wave of 4 nodes holds one species"
        assert sp.tolist() != [n % S for n in range(N_NODES)]
    return sp


class Piece:
    """one narrowed (entry, coupling): where it sits in the row and which columns of the reference row feed it"""


class State:
    pass


def _tp_key(name):
    p = anc.uvu_plan(name)
    return (anc.CASES[name][0], str(p.irreps_out))


def _tp_state(name, built):
    """operands and un-normalised neighbour sums (fp64, fp32) of a case's tensor product, shared by every case that runs the
    same one (full_1 / full_2 / full_4 differ in lin2 only)"""
    from matten_amd.nn._tables import DeviceTables

    key = _tp_key(name)
    if key not in built["tp"]:
        irreps_in, target, _ = anc.CASES[name]
        p = anc.uvu_plan(name)
        tp64, tp32 = _oracle_tp_of(irreps_in, LMAX, target)
        assert tp64.weight_numel == p.weight_numel and p.d_in == tp64.irreps_in1.dim
        op = Case()
        op.p = p
        op.t = DeviceTables(gentries=p.group_entries, gumap=p.fused_unit_map)
        edge_index = built["edge_index"]
        gen = torch.Generator().manual_seed(4000 + len(built["tp"]))
        x, Y, w64, w32 = _operands(op, LMAX, edge_index, N_NODES, gen)
        assert sorted(set(op.in_deg.tolist())) == sorted(DEGREES) and op.E == 910
        one = torch.ones(N_NODES, dtype=torch.float64)
        op.raw64 = _reference(tp64, x.double(), Y.double(), w64, edge_index, N_NODES, one)
        op.raw32 = _reference(tp32, x, Y, w32, edge_index, N_NODES, one.float())
        assert op.raw64.shape == (N_NODES, p.d_mid) and op.raw32.dtype == torch.float32
        nn = op.in_deg.float()                                # 0 where nothing arrives, as in production
        op.nn = nn.to(DEV)
        op.nrm = {"avg": torch.full((N_NODES,), AVG ** -0.5, dtype=torch.float64),
                  "node": torch.where(op.rows_in, nn.double().clamp(min=1) ** -0.5, torch.zeros((), dtype=torch.float64))}
        built["tp"][key] = op
    op = built["tp"][key]
    p = anc.uvu_plan(name)
    assert np.array_equal(np.asarray(p.group_entries), np.asarray(op.p.group_entries)) and p.d_mid == op.p.d_mid
    assert np.array_equal(np.asarray(p.fused_cols), np.asarray(op.p.fused_cols))
    return op


def sums(op, norm, dtype):
    """the normalised neighbour sums, as _reference leaves them (the un-normalised sums x the norm, in the sums' dtype)"""
    raw, nrm = (op.raw64, op.nrm[norm]) if dtype == torch.float64 else (op.raw32, op.nrm[norm].float())
    return raw * nrm[:, None]


def layout(name, S):
    """-> (Layer, narrowed pieces, [(path label, slots, reference columns)] of the un-narrowed couplings per path,
    written-slot mask, mask of the scalar-input entries' slots) from the plans alone: no GPU"""
    p, ap = anc.uvu_plan(name), anc.narrow_plan(name, S)
    lay = alc.Layer(name, S, p, ap, anc.mplan.Irreps(anc.CASES[name][1]).simplify(), None, None)
    out_blocks = {(ir.l, ir.p): (lo, hi, int(mul)) for (mul, ir), (lo, hi, _) in zip(lay.irreps_out, alc.irrep_blocks(lay.irreps_out))}
    pieces, plain = [], {}
    written, l0 = torch.zeros(ap.ld, dtype=torch.bool), torch.zeros(ap.ld, dtype=torch.bool)
    for e, c, q, ks, o, mo in anc.couplings(p, ap):
        d3, mul, u0 = 2 * q.l3 + 1, int(p.group_entry_mul[e]), int(p.group_entry_u0[e])
        u, k = np.arange(mul), np.arange(d3)
        cols = (q.out_off + (u0 + u)[:, None] * d3 + k[None, :]).reshape(-1)          # [u][k] of the mul_ir row
        if mo:
            lo, hi, mo_out = out_blocks[(q.l3, q.p3)]
            assert mo == mo_out and hi - lo == mo * d3
            pc = Piece()
            pc.e, pc.c, pc.mo, pc.d3, pc.lo, pc.hi, pc.l1, pc.path = e, c, mo, d3, lo, hi, q.l1, (q.l1, q.l2, q.l3)
            pc.label = f"entry {e} coupling {c} (path {q.l1},{q.l2},{q.l3}, channels {u0}..{u0 + mul - 1}, mo {mo})"
            pc.cols = torch.as_tensor(cols)
            pc.slots = torch.as_tensor((o + np.arange(mo)[:, None] + k[None, :] * ks).reshape(-1))   # [v][k], as lin2's block
            pieces.append(pc)
            slots = pc.slots
        else:
            slots = torch.as_tensor((o + u[:, None] + k[None, :] * ks).reshape(-1))
            label = f"path {q.l1},{q.l2},{q.l3} (un-narrowed slots)"
            plain.setdefault(label, []).append((slots, torch.as_tensor(cols)))
        assert 0 <= int(slots.min()) and int(slots.max()) < ap.ld and not written[slots].any()    # every slot written once
        written[slots] = True
        if q.l1 == 0:
            l0[slots] = True
    plain = [(label, torch.cat([s for s, _ in v]), torch.cat([c_ for _, c_ in v])) for label, v in plain.items()]
    return lay, pieces, plain, written, l0


def expected_rows(lay, pieces, plain, species, w, agg):
    """the row the kernel should write (NaN where no entry writes), in the dtype of the sums `agg` [N, d_mid]: an
    un-narrowed slot is its column of agg; a narrowed piece is its output-irrep block of the oracle's lin2 on a copy of agg
    that is zero but for the piece's own channels (lin2 is linear: PIECE_BATCH pieces per call, stacked as rows)"""
    N, dtype = agg.shape[0], agg.dtype
    want = torch.full((N, lay.ap.ld), float("nan"), dtype=dtype)
    for _, slots, cols in plain:
        want[:, slots] = agg[:, cols]
    for b0 in range(0, len(pieces), PIECE_BATCH):
        batch = pieces[b0: b0 + PIECE_BATCH]
        z = torch.zeros(len(batch), N, agg.shape[1], dtype=dtype)
        for i, pc in enumerate(batch):
            z[i][:, pc.cols] = agg[:, pc.cols]
        out = alc.reference_lin2(lay, z.reshape(len(batch) * N, -1), np.tile(species, len(batch)), w, dtype)
        out = out.reshape(len(batch), N, -1)
        for i, pc in enumerate(batch):
            want[:, pc.slots] = out[i][:, pc.lo: pc.hi]
    return want


def _state(name, S, built):
    from matten_amd import plan as mplan

    if (name, S) not in built["state"]:
        st = State()
        st.name, st.S = f"{name}-S{S}", S
        st.op = op = _tp_state(name, built)
        st.lay, st.pieces, st.plain, st.written, st.l0 = layout(name, S)
        st.ap = ap = st.lay.ap
        st.species = built["species"][S]
        rng = np.random.default_rng(100 + len(built["state"]))
        st.w = rng.standard_normal(alc.weight_numel(st.lay)).astype(np.float32)
        st.wn = anc.narrow_weights(ap, st.w)
        st.blob = torch.from_numpy(mplan.narrow_blob(ap, st.wn)).to(DEV)
        st.species_dev = torch.from_numpy(st.species.astype(np.int32)).to(DEV)
        assert set(st.species[op.rows_in.numpy()].tolist()) == set(range(S))       # every species has nodes with in-edges
        st.want, st.rtol, st.r32, st.results = {}, {}, {}, {}
        rows = op.rows_in
        for norm in NORMS:
            w64 = expected_rows(st.lay, st.pieces, st.plain, st.species, st.w, sums(op, norm, torch.float64))
            w32 = expected_rows(st.lay, st.pieces, st.plain, st.species, st.w, sums(op, norm, torch.float32)).double()
            assert torch.isfinite(w64[:, st.written]).all() and torch.isnan(w64[:, ~st.written]).all()
            st.want[norm] = w64
            st.r32[norm] = max(_ratio((w32[rows][:, pc.slots] - w64[rows][:, pc.slots]).abs().max().item(),
                                      w64[rows][:, pc.slots].abs().max().item()) for pc in st.pieces)
            assert 0 < st.r32[norm] < 1e-5, st.r32[norm]          # an fp32 evaluation of a few hundred terms per output
            st.rtol[norm] = min(FWD_RTOL, R32_FACTOR * st.r32[norm])
        built["state"][(name, S)] = st
    return built["state"][(name, S)]


@pytest.fixture(scope="module")
def built():
    """what the cases share, built on first use: the graph, the species draws, one set of operands and un-normalised sums
    per tensor product, one State per (case, species count)"""
    anc.assert_every_instance_has_a_case()
    g = _graph_70()
    cache = {"edge_index": g["edge_index"], "species": {S: _species(S) for S in SPECIES_SEED}, "tp": {}, "state": {}}
    yield cache
    cache.clear()
    torch.cuda.synchronize()


@pytest.fixture(scope="module", params=CASES, ids=_ids(CASES))
def case(request, built):
    name, S, norm = request.param
    return _state(name, S, built), norm


def _launch(st, norm, umap=None, species=None, blob=None, nn=None):
    """ops.tp_fused(..., narrow=...) on the case's operands: the production launch unless an argument replaces an operand"""
    from matten_amd import ops

    op = st.op
    umap = op.t.get("gumap", DEV) if umap is None else umap
    _nan_prefill(op.N, st.ap.ld)
    return ops.tp_fused(op.x, op.h2p, op.w2f, op.Y, op.rowptr, op.src, st.blob if blob is None else blob, umap, umap.numel(),
                        op.p.fused_lds_floats_per_wave, st.ap.ld, AVG if norm == "avg" else 0.0,
                        None if norm == "avg" else (op.nn if nn is None else nn), a_split=op.a_split,
                        narrow=(st.species_dev if species is None else species, len(st.ap.entries)))


def _production(st, norm):
    if norm not in st.results:
        st.results[norm] = _launch(st, norm)
    return st.results[norm]


def check_structure(st, row, what):
    """slots no entry writes are still NaN, written ones finite, the rows of nodes nothing arrives at exactly 0"""
    assert row.shape == (st.op.N, st.ap.ld) and row.dtype == torch.float32, (what, row.shape, row.dtype)
    got = row.detach().cpu()
    assert torch.isnan(got[:, ~st.written]).all(), f"{what}: a slot no entry writes was written"
    bad = int((~torch.isfinite(got[:, st.written])).sum())
    assert bad == 0, f"{what}: non-finite output ({bad} values)"
    assert (got[~st.op.rows_in][:, st.written] == 0).all(), f"{what}: a row without in-edges is not exactly 0"


def piece_errors(st, row, norm):
    """every narrowed piece and every path's un-narrowed slots against their own largest |fp64 reference| over the rows
    with in-edges -> [(error / allowed, label)], worst first"""
    rows = st.op.rows_in
    got, want = row.detach().cpu().double()[rows], st.want[norm][rows]
    groups = [(pc.label, pc.slots) for pc in st.pieces] + [(label, slots) for label, slots, _ in st.plain]
    res = []
    for label, slots in groups:
        scale = want[:, slots].abs().max().item()
        res.append((_ratio((got[:, slots] - want[:, slots]).abs().max().item(), st.rtol[norm] * scale), label))
    return sorted(res, reverse=True)


def _assert_within(st, row, norm, what):
    res = piece_errors(st, row, norm)
    bad = [(f"{r:.3g}", label) for r, label in res if not r <= 1.0]
    assert not bad, (f"{what}: error / allowed (allowed {st.rtol[norm]:.3g} of the piece's maximum, r32 {st.r32[norm]:.3g}): "
                     f"{bad[:8]} ({len(bad)} of {len(res)} pieces)")
    return res[0]


def test_narrowed_pieces_match_fp64(case):
    st, norm = case
    row = _production(st, norm)
    check_structure(st, row, f"{st.name}-{norm}")
    res = piece_errors(st, row, norm)
    worst_narrow = max(r_ for r_, l_ in res if l_.startswith("entry"))
    r, label = _assert_within(st, row, norm, f"{st.name}-{norm} tp_fused_narrow")
    print(f"\nTP_NARROW_RATIO {st.name}-{norm} {r:.3g} {label}   (narrowed pieces alone {worst_narrow:.3g}; r32 {st.r32[norm]:.3g}, "
          f"allowed {st.rtol[norm]:.3g} of a piece's maximum)")


def test_two_launches_give_identical_bits(case):
    st, norm = case
    a, b = _production(st, norm), _launch(st, norm)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_entry_major_walk(case):
    """the plain walk (entry-major unit map: every wave fetches its own rows): the same bits in every slot of the
    scalar-input entries, the narrowed ones included, and every slot inside the same fp64 bound (the vector blocks' shared walk
    sums edge pairs in another association by design)"""
    from matten_amd import plan as mplan

    st, norm = case
    p = st.op.p
    um = torch.from_numpy(mplan.fused_unit_map(p.group_entries, "entry")).to(DEV)
    plain = _launch(st, norm, umap=um)
    check_structure(st, plain, f"{st.name}-{norm} entry-major")
    shared = _production(st, norm)
    assert st.l0.any() and any(pc.l1 == 0 for pc in st.pieces)
    l0 = st.l0.to(DEV)
    assert torch.equal(shared[:, l0], plain[:, l0]), "scalar-input entries: the walk form changed the bits"
    r, label = _assert_within(st, plain, norm, f"{st.name}-{norm} entry-major walk")
    print(f"\nTP_NARROW_RATIO {st.name}-{norm}-entry-major {r:.3g} {label}")


# ---- the reader on the rows the kernel wrote ---------------------------------------------------------------------------------
READER_CASES = [(name, 3, norm) for name in READER for norm in NORMS]


@pytest.mark.parametrize("case", READER_CASES, indirect=True, ids=_ids(READER_CASES))
def test_reader_on_kernel_written_rows(case):
    from matten_amd import ops

    st, norm = case
    ap, lay = st.ap, st.lay
    assert (ap.gather == anc.mplan.AGG_GATHER_ONE).any()
    wtab = torch.from_numpy(anc.wtab(ap, st.w)).to(DEV)
    assert (wtab == 1.0).sum() >= sum(pc.mo for pc in st.pieces)
    order = tuple(torch.from_numpy(t).to(DEV) for t in alc.order_seg(st.species, st.S))
    _nan_prefill(st.op.N, ap.d_out)
    out = ops.agg_linear(_production(st, norm), order, wtab, torch.from_numpy(ap.io_table).to(DEV),
                         torch.from_numpy(ap.blocks).to(DEV), ap.d_out).cpu()
    assert out.shape == (st.op.N, ap.d_out) and torch.isfinite(out).all()
    lin64 = alc.reference_lin2(lay, sums(st.op, norm, torch.float64), st.species, st.w, torch.float64)
    lin32 = alc.reference_lin2(lay, sums(st.op, norm, torch.float32), st.species, st.w, torch.float32)
    res = alc.block_errors(out.numpy(), lin64.numpy(), lin32.numpy(), st.species, alc.irrep_blocks(lay.irreps_out))
    frac = max(res.items(), key=lambda kv: kv[1][0] / kv[1][1])
    rel = max(res.items(), key=lambda kv: kv[1][0] / kv[1][2])
    print(f"\nTP_NARROW_READER {st.name}-{norm}: worst |err| / block max {rel[1][0] / rel[1][2]:.2e} at {rel[0]}, "
          f"worst fraction of the allowed distance {frac[1][0] / frac[1][1]:.2f} at {frac[0]}")
    bad = {k: v for k, v in res.items() if not v[0] <= v[1]}
    assert not bad, bad


# ---- controls: the piece check sees in-bounds mutations of the operands handed to the unchanged kernel ------------------------
def _mut_species_swapped(st):
    """(a) the species of two nodes of one wave (4 nodes), both with in-edges, swapped"""
    sp, rows = st.species.copy(), st.op.rows_in.numpy()
    a, b = next((a, b) for n in range(0, 64, 4) for a in range(n, n + 4) for b in range(a + 1, n + 4)
                if sp[a] != sp[b] and rows[a] and rows[b])
    sp[a], sp[b] = sp[b], sp[a]
    assert sorted(sp.tolist()) == sorted(st.species.tolist())
    return "avg", dict(species=torch.from_numpy(sp.astype(np.int32)).to(DEV))


def _weight_block(st, pc):
    """(first float, [S, mul, mo] shape) of a narrowed piece's block in the writer's weights"""
    nw = int(st.ap.narrow[pc.e][pc.c])
    mul = int(st.op.p.group_entry_mul[pc.e])
    assert nw & 255 == pc.mo
    return nw >> 8, (st.S, mul, pc.mo)


def _blob_with(st, wn=None, entries=None):
    from matten_amd import plan as mplan

    ap = st.ap if entries is None else dataclasses.replace(st.ap, entries=entries)
    blob = mplan.narrow_blob(ap, st.wn if wn is None else wn)
    assert blob.shape == (st.blob.numel(),)
    return torch.from_numpy(blob).to(DEV)


def _mut_one_weight(st):
    """(b) the largest weight of one species in one D3 = 9 block times 1 + 1e-3"""
    pc = next(pc for pc in st.pieces if pc.d3 == 9 and pc.l1 == 0)
    off, shape = _weight_block(st, pc)
    wn = st.wn.copy()
    blk = wn[off: off + int(np.prod(shape))].reshape(shape)          # a view of wn
    s = 1
    i = np.unravel_index(np.argmax(np.abs(blk[s])), blk[s].shape)
    blk[s][i] *= np.float32(1.001)
    assert (wn != st.wn).sum() == 1
    return "avg", dict(blob=_blob_with(st, wn=wn))


def _mut_species_blocks(st):
    """(c) the weight blocks of species 0 and 2 of one coupling swapped"""
    pc = next(pc for pc in st.pieces if pc.l1 == 1 and pc.d3 == 5)
    off, shape = _weight_block(st, pc)
    wn = st.wn.copy()
    blk = wn[off: off + int(np.prod(shape))].reshape(shape)
    blk[[0, 2]] = blk[[2, 0]]
    assert sorted(wn.tolist()) == sorted(st.wn.tolist()) and (wn != st.wn).any()
    return "avg", dict(blob=_blob_with(st, wn=wn))


def _mut_num_neigh(st):
    """(d) num_neigh exchanged between neighbouring nodes of in-degrees 1 <-> 5 and 19 <-> 40 (per-node normalisation);
    the nodes nothing arrives at keep their 0"""
    nn = st.op.in_deg.float()
    for n in range(0, 60, 5):
        nn[[n + 1, n + 2]] = nn[[n + 2, n + 1]]
        nn[[n + 3, n + 4]] = nn[[n + 4, n + 3]]
    assert sorted(nn.tolist()) == sorted(st.op.in_deg.tolist()) and ((nn == 0) == ~st.op.rows_in).all()
    return "node", dict(nn=nn.to(DEV))


def _mut_out_off(st):
    """(e) the first-float halves of the out_off words of two narrowed couplings of the same path (two 16-channel entries
    of one input block: the same output irrep, region, mo and D3) swapped"""
    by_path = {}
    for pc in st.pieces:
        by_path.setdefault(pc.path, []).append(pc)
    a, b = next(v[:2] for v in by_path.values() if len(v) >= 2)
    assert (a.mo, a.d3, a.lo) == (b.mo, b.d3, b.lo) and a.e != b.e
    ent = st.ap.entries.copy()
    wa, wb = int(ent[a.e][20 + a.c]), int(ent[b.e][20 + b.c])
    ent[a.e][20 + a.c] = (wa & ~0xFFFF) | (wb & 0xFFFF)
    ent[b.e][20 + b.c] = (wb & ~0xFFFF) | (wa & 0xFFFF)
    assert (ent != st.ap.entries).sum() == 2
    return "avg", dict(blob=_blob_with(st, entries=ent))


CONTROLS = {"species_swapped": _mut_species_swapped, "one_weight": _mut_one_weight, "species_blocks": _mut_species_blocks,
            "num_neigh": _mut_num_neigh, "out_off": _mut_out_off}


@pytest.mark.parametrize("control", list(CONTROLS))
def test_controls_are_seen(control, built):
    """every mutation stays inside its buffer: species indices < S, weights and entry words of the same blob, num_neigh a
    permutation, swapped offsets those of another piece of the same shape and region"""
    st = _state("full_2", 3, built)
    norm, mutated = CONTROLS[control](st)
    check_structure(st, _production(st, norm), "unmutated")
    assert _assert_within(st, _production(st, norm), norm, "unmutated")[0] <= 1.0
    row = _launch(st, norm, **mutated)
    check_structure(st, row, control)
    res = piece_errors(st, row, norm)
    bad = [x for x in res if not x[0] <= 1.0]
    print(f"\nTP_NARROW_CONTROL {control}: {len(bad)} of {len(res)} pieces outside, worst {res[0][0]:.3g} x allowed at {res[0][1]}")
    assert bad, f"control {control}: the piece check sees nothing"
