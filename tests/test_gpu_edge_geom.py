"""
matten_edge_geom forward (csrc/edge.hip, csrc/sh.h) against fp64: edge vectors, lengths, real spherical harmonics per degree
block, the Bessel embedding per basis function, and the layout of the sorted outputs.

Graphs are built by hand (no fcc, no neighbour search): three triclinic cells of different size, random edges inside each
crystal, integer shifts in [-2, 2] (half of the random edges keep a zero shift so that enough of them lie inside the
cutoff), self images, one atom without an edge, and planted edges: along +-x, +-y, +-z, length ~1e-4, lengths just below /
at / just above / far beyond r_end, length 0.5 (== r_start of the third basis), and zero-length edges (a self edge with a
zero shift, two coincident atoms).  The fp64 reference -- the oracle's with_edge_vectors, o3.spherical_harmonics and
soft_one_hot_linspace(bessel, cutoff) * sqrt(nb) -- receives the same fp32 values cast up.

Bounds.  Each is 4 x the worst error of an fp32 torch evaluation of the same reference expression against its fp64
evaluation on this file's inputs (worst over the cases, relative to the largest |reference| of the block compared: the
whole of edge_vectors / edge_lengths, a degree block l of the harmonics, one basis function k of the embedding); the factor
covers another summation order and FMA contraction, not other arithmetic.  `python tests/test_gpu_edge_geom.py` prints the
fp32-torch errors (CPU only); they differ a little between ATen's CPU code paths (ATEN_CPU_CAPABILITY = default / avx2 /
avx512: the vectorised sqrt, sin and sums), the constants below are the largest figure over them, rounded up.
    fp32 torch vs fp64, worst:  vectors 8.88e-8   lengths 1.11e-7   harmonics l = 0..4: 0, 1.43e-7, 2.93e-7, 2.94e-7, 4.17e-7
                                embedding (nb, r_start, r_end) = (8, 0, 5): 1.84e-7   (16, 0, 5): 1.94e-7   (3, 0.5, 4): 2.08e-7
Worst error / allowed of the kernel, measured on MI355X:
    vectors 0.25   lengths 0.23   harmonics l = 1..4: 0.27, 0.23, 0.27, 0.55 (l = 0 exact)
    embedding 0.25 for each of the three bases
(l = 4 is the least-conditioned block: sh.h evaluates degree-4 polynomials with |n| = 1 used up, the oracle a recursion.)
Exact: the l = 0 block (the constant 1), geom_sorted / sh_sorted against the original-order outputs gathered by perm, the
padding columns of sh_sorted, embedding rows at or beyond r_end and at r_start, zero-length rows ([1, 0, ..., 0], len 0,
no gradient from matten_edge_geom_bwd), a second call, and a call whose torch.empty buffers start as NaN.
"""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from test_gpu_geom_grad import _ratio  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SH_STRIDE = 32
N_ATOMS = 20
LONE_ATOM = 5                  # no edge touches it
PLANT_ONLY = (15,)             # only the planted edges touch it (one of the coincident pair)
CUTOFF_ATOMS = (7, 12)         # first and last of the atoms that carry the planted lengths around r_end and at r_start
CELLS = ("three", "one", "none")
RBF = ((8, 0.0, 5.0), (16, 0.0, 5.0), (3, 0.5, 4.0))
R_START_PLANTED = 0.5
ES = (1, 63, 64, 65, 257, 1000)

# 4 x the fp32-torch error of the reference expression (module docstring)
FP32_TORCH = {"vec": 8.88e-8, "len": 1.11e-7, "sh": (0.0, 1.43e-7, 2.93e-7, 2.94e-7, 4.17e-7),
              "emb": {RBF[0]: 1.84e-7, RBF[1]: 1.94e-7, RBF[2]: 2.08e-7}}
VEC_RTOL = 4 * FP32_TORCH["vec"]
LEN_RTOL = 4 * FP32_TORCH["len"]
SH_RTOL = tuple(4 * v for v in FP32_TORCH["sh"])
EMB_RTOL = {k: 4 * v for k, v in FP32_TORCH["emb"].items()}


def _cases():
    """every (E, perm) pair at lmax 4 and at lmax 2, the cells and the bases cycling through all nine combinations; then
    lmax 0, 1, 3"""
    out, i = [], 0
    for lmax in (4, 2):
        for E in ES:
            for permuted in (False, True):
                out.append((lmax, CELLS[i % 3], permuted, E, RBF[(i // 3) % 3]))
                i += 1
    out += [(0, "three", True, 65, RBF[0]), (1, "one", False, 257, RBF[1]), (3, "none", True, 64, RBF[2])]
    return out


CASES = _cases()


def _case_id(case):
    lmax, cells, permuted, E, (nb, r0, r1) = case
    return f"lmax{lmax}-{cells}-{'perm' if permuted else 'ident'}-E{E}-nb{nb}_{r0:g}_{r1:g}"


def _edge_inputs(case):
    """host operands of one case (fp32) and where the planted edges ended up: d["planted"][name] -> edge ids"""
    lmax, cells, permuted, E, (nb, r_start, r_end) = case
    gen = torch.Generator().manual_seed(7000 + CASES.index(case))
    sizes = [7, 6, 7] if cells == "three" else [N_ATOMS]
    B = len(sizes)
    batch = torch.cat([torch.full((n,), b, dtype=torch.int64) for b, n in enumerate(sizes)])
    cell = (torch.eye(3) * 4.0 + 0.5 * torch.randn(B, 3, 3, generator=gen)) * (1.0 + 0.3 * torch.arange(B)[:, None, None])
    pos = 4.0 * torch.rand(N_ATOMS, 3, generator=gen)
    # planted geometry: coordinates that fp32 holds exactly, so that the differences are exact too
    p0 = torch.tensor([1.0, 0.5, 0.25])
    pos[0] = p0
    pos[1] = p0 + torch.tensor([2.0, 0.0, 0.0])
    pos[2] = p0 + torch.tensor([0.0, 1.5, 0.0])
    pos[3] = p0 + torch.tensor([0.0, 0.0, 3.0])
    pos[4] = p0 + torch.tensor([6e-5, 3e-5, 8e-5])
    q0 = torch.tensor([0.5, 0.25, 0.0])
    pos[7] = q0
    for a, z in zip((8, 9, 10, 11), (r_end - 1e-6, r_end, r_end + 5e-7, r_end + 1.5)):
        pos[a] = q0 + torch.tensor([0.0, 0.0, z])
    pos[12] = q0 + torch.tensor([0.0, R_START_PLANTED, 0.0])
    pos[15] = pos[14]
    zero = (0.0, 0.0, 0.0)
    planted = [(0, 1, zero, "axis"), (1, 0, zero, "axis"), (0, 2, zero, "axis"), (2, 0, zero, "axis"), (0, 3, zero, "axis"),
               (3, 0, zero, "axis"), (0, 4, zero, "tiny"), (4, 0, zero, "tiny"), (7, 8, zero, "below"), (7, 9, zero, "at"),
               (7, 10, zero, "above"), (7, 11, zero, "far"), (7, 12, zero, "half"), (13, 13, zero, "zero"),
               (14, 15, zero, "zero"), (15, 14, zero, "zero")]
    if cells != "none":
        planted += [(16, 16, (1.0, 0.0, 0.0), "image"), (16, 16, (0.0, -1.0, 1.0), "image"), (19, 19, (2.0, -2.0, 1.0), "image")]
    if E < len(planted):   # a single edge: the short one, where every basis function is near its maximum (one row is all
        planted = [(0, 4, zero, "tiny")]   # a column has, and a value near a zero of the sine would be its own scale)
    n_rand = E - len(planted)
    # random edges inside each crystal, between different atoms
    free = []
    first = 0
    for n in sizes:
        free.append(torch.tensor([a for a in range(first, first + n) if a != LONE_ATOM and a not in PLANT_ONLY]))
        first += n
    k = 4 * n_rand + 32
    crystal = torch.randint(B, (k,), generator=gen)
    u, v = torch.rand(k, generator=gen), torch.rand(k, generator=gen)
    n_free = torch.tensor([len(f) for f in free])[crystal]
    start = torch.tensor([0] + [len(f) for f in free]).cumsum(0)[:-1][crystal]
    flat = torch.cat(free)
    s = flat[start + (u * n_free).long().clamp(max=n_free - 1)]
    t = flat[start + (v * n_free).long().clamp(max=n_free - 1)]
    sh = torch.randint(-2, 3, (k, 3), generator=gen).float() * (torch.rand(k, generator=gen) < 0.5)[:, None]
    if cells == "none":
        sh.zero_()
    # (no unshifted edge between two atoms of the planted cutoff lengths: it would add rows at those lengths)
    planted_pair = (s >= CUTOFF_ATOMS[0]) & (s <= CUTOFF_ATOMS[1]) & (t >= CUTOFF_ATOMS[0]) & (t <= CUTOFF_ATOMS[1])
    keep = ((s != t) & ~(planted_pair & (sh == 0).all(1))).nonzero()[:n_rand, 0]
    assert keep.numel() == n_rand
    src = torch.cat([torch.tensor([p[0] for p in planted], dtype=torch.int64), s[keep]])
    dst = torch.cat([torch.tensor([p[1] for p in planted], dtype=torch.int64), t[keep]])
    shift = torch.cat([torch.tensor([p[2] for p in planted], dtype=torch.float32).reshape(-1, 3), sh[keep]])
    order = torch.randperm(E, generator=gen)
    where = torch.empty(E, dtype=torch.int64)
    where[order] = torch.arange(E)             # edge i of the list above sits at where[i]
    names = sorted({p[3] for p in planted})
    marks = {n: torch.tensor(sorted(int(where[i]) for i, p in enumerate(planted) if p[3] == n), dtype=torch.int64) for n in names}
    perm = torch.randperm(E, generator=gen).to(torch.int32) if permuted else None
    return dict(lmax=lmax, cells=cells, E=E, B=B, nb=nb, r_start=r_start, r_end=r_end, batch=batch,
                cell=None if cells == "none" else cell, pos=pos, edge_index=torch.stack([src, dst])[:, order].contiguous(),
                shift=shift[order].contiguous(), perm=perm, planted=marks, n_planted=len(planted))


def _edge_reference(d, dtype):
    """the oracle's edge vectors, lengths, harmonics and embedding (original edge order) evaluated in `dtype`"""
    from oracle.e3nn_lite.math import soft_one_hot_linspace
    from oracle.e3nn_lite.o3 import spherical_harmonics
    from oracle.matten_ref.nn import DataKey, with_edge_vectors

    data = {DataKey.POSITIONS: d["pos"].to(dtype), DataKey.EDGE_INDEX: d["edge_index"]}
    if d["cell"] is not None:
        data[DataKey.CELL] = d["cell"].to(dtype)
        data[DataKey.EDGE_CELL_SHIFT] = d["shift"].to(dtype)
        if d["B"] > 1:
            data[DataKey.BATCH] = d["batch"]
    data = with_edge_vectors(data)
    v, r = data[DataKey.EDGE_VECTORS], data[DataKey.EDGE_LENGTH]
    Y = spherical_harmonics(list(range(d["lmax"] + 1)), v, True, "component")
    emb = soft_one_hot_linspace(r, d["r_start"], d["r_end"], d["nb"], basis="bessel", cutoff=True) * d["nb"] ** 0.5
    return dict(edge_vectors=v, edge_lengths=r, edge_attrs=Y, edge_embedding=emb)


def _excluded_rows(ref):
    """edges whose length is exactly r_start: the reference's embedding is 0 / 0 there"""
    return torch.isnan(ref["edge_embedding"]).any(1)


def _edge_errors(got, ref, d):
    """-> {"vec": (err, scale), "len": (err, scale), "sh": [(err, scale)] per l, "emb": [(err, scale)] per k}; the rows
    of _excluded_rows(ref) are left out of the embedding"""
    def es(a, b):
        return (a.double() - b).abs().max().item(), b.abs().max().item()

    out = {"vec": es(got["edge_vectors"], ref["edge_vectors"]), "len": es(got["edge_lengths"], ref["edge_lengths"])}
    out["sh"] = [es(got["edge_attrs"][:, l * l:(l + 1) ** 2], ref["edge_attrs"][:, l * l:(l + 1) ** 2])
                 for l in range(d["lmax"] + 1)]
    ok = ~_excluded_rows(ref)
    out["emb"] = [es(got["edge_embedding"][ok, k], ref["edge_embedding"][ok, k]) if ok.any() else (0.0, 0.0)
                  for k in range(d["nb"])]
    return out


def fp32_torch_errors():
    """worst fp32-torch error / block scale over the cases, in the shape of the committed constants (without the 4)"""
    worst = {"vec": 0.0, "len": 0.0, "sh": [0.0] * 5, "emb": {r: 0.0 for r in RBF}}
    rel = lambda e: e[0] / e[1] if e[1] else (0.0 if e[0] == 0 else math.inf)
    for case in CASES:
        d = _edge_inputs(case)
        ref = _edge_reference(d, torch.float64)
        e = _edge_errors(_edge_reference(d, torch.float32), ref, d)
        worst["vec"], worst["len"] = max(worst["vec"], rel(e["vec"])), max(worst["len"], rel(e["len"]))
        for l, x in enumerate(e["sh"]):
            worst["sh"][l] = max(worst["sh"][l], rel(x))
        worst["emb"][case[4]] = max([worst["emb"][case[4]]] + [rel(x) for x in e["emb"]])
    return worst


def nan_filled_empty(monkeypatch):
    """torch.empty / torch.empty_like hand out NaN-filled float buffers on the device (what MATTEN_TEST_NAN_EMPTY does for
    a whole session): a kernel that leaves a part of its output unwritten, or reads what nobody wrote, shows"""
    _empty, _empty_like = torch.empty, torch.empty_like

    def nan_empty(*a, **k):
        t = _empty(*a, **k)
        return t.fill_(float("nan")) if t.is_floating_point() and t.device.type == "cuda" else t

    def nan_empty_like(*a, **k):
        t = _empty_like(*a, **k)
        return t.fill_(float("nan")) if t.is_floating_point() and t.device.type == "cuda" else t

    monkeypatch.setattr(torch, "empty", nan_empty)
    monkeypatch.setattr(torch, "empty_like", nan_empty_like)


OUTPUTS = ("geom_sorted", "sh_sorted", "edge_vectors", "edge_lengths", "edge_attrs", "edge_embedding")


@pytest.fixture(scope="module", params=CASES, ids=[_case_id(c) for c in CASES])
def edge_case(request):
    d = _edge_inputs(request.param)
    d["name"] = _case_id(request.param)
    d["ref"] = _edge_reference(d, torch.float64)
    d["dev"] = dict(pos=d["pos"].to(DEV), edge_index=d["edge_index"].to(DEV), shift=d["shift"].to(DEV),
                    cell=None if d["cell"] is None else d["cell"].to(DEV), batch=d["batch"].to(DEV) if d["B"] > 1 else None,
                    perm=None if d["perm"] is None else d["perm"].to(DEV))
    yield d
    torch.cuda.synchronize()


def _run(d):
    from matten_amd import ops

    t = d["dev"]
    torch.full((d["E"], SH_STRIDE), float("nan"), device=DEV)   # what the allocator hands out next must not pass as zeros
    return ops.edge_geom(t["pos"], t["edge_index"], t["shift"], t["cell"], t["batch"], t["perm"], d["lmax"], d["nb"],
                         d["r_start"], d["r_end"], want_vectors=True, want_lengths=True, want_attrs=True, want_embedding=True)


def test_edge_geom_matches_fp64_per_block(edge_case):
    d = edge_case
    E, lmax, nb, ref = d["E"], d["lmax"], d["nb"], d["ref"]
    sh_dim = (lmax + 1) ** 2
    out = _run(d)
    got = {k: out[k].cpu() for k in OUTPUTS}
    assert got["geom_sorted"].shape == (E, 4) and got["sh_sorted"].shape == (E, SH_STRIDE)
    assert got["edge_vectors"].shape == (E, 3) and got["edge_lengths"].shape == (E,)
    assert got["edge_attrs"].shape == (E, sh_dim) and got["edge_embedding"].shape == (E, nb)
    assert all(torch.isfinite(got[k]).all() for k in OUTPUTS)

    e = _edge_errors(got, ref, d)
    ratios = {"vec": _ratio(e["vec"][0], VEC_RTOL * e["vec"][1]), "len": _ratio(e["len"][0], LEN_RTOL * e["len"][1]),
              "sh": [_ratio(err, SH_RTOL[l] * scale) for l, (err, scale) in enumerate(e["sh"])],
              "emb": [_ratio(err, EMB_RTOL[(nb, d["r_start"], d["r_end"])] * scale) for err, scale in e["emb"]]}
    print(f"\nEDGE_GEOM {d['name']} vec {ratios['vec']:.3g} len {ratios['len']:.3g} sh "
          + " ".join(f"{r:.3g}" for r in ratios["sh"]) + " emb " + " ".join(f"{r:.3g}" for r in ratios["emb"]))
    assert ratios["vec"] <= 1.0 and ratios["len"] <= 1.0, f"{d['name']}: vectors / lengths error / allowed {ratios}"
    for l, r in enumerate(ratios["sh"]):
        assert r <= 1.0, f"{d['name']}: harmonics l={l} error / allowed = {r:.3g} (err {e['sh'][l][0]:.3e}, scale {e['sh'][l][1]:.3e})"
    for k, r in enumerate(ratios["emb"]):
        assert r <= 1.0, f"{d['name']}: embedding k={k} error / allowed = {r:.3g} (err {e['emb'][k][0]:.3e}, scale {e['emb'][k][1]:.3e})"

    # the sorted outputs are the original-order ones gathered by perm, bit for bit; the padding columns are zeros
    pl = torch.arange(E) if d["perm"] is None else d["perm"].long()
    assert torch.equal(got["geom_sorted"][:, :3], got["edge_vectors"][pl])
    assert torch.equal(got["geom_sorted"][:, 3], got["edge_lengths"][pl])
    assert torch.equal(got["sh_sorted"][:, :sh_dim], got["edge_attrs"][pl])
    assert (got["sh_sorted"][:, sh_dim:] == 0).all(), "padding columns of every row, the last partial wave included"

    # embedding: exact zeros at or beyond r_end and at r_start
    beyond = ref["edge_lengths"] >= d["r_end"]
    assert (got["edge_embedding"][beyond] == 0).all()
    excluded = _excluded_rows(ref)
    placed = d["planted"].get("zero" if d["r_start"] == 0.0 else "half", torch.zeros(0, dtype=torch.int64))
    assert int(excluded.sum()) == placed.numel() and torch.equal(excluded.nonzero()[:, 0], placed)
    assert (got["edge_embedding"][excluded] == 0).all()
    if "zero" in d["planted"]:
        assert bool(beyond[d["planted"]["at"]].all() and beyond[d["planted"]["above"]].all() and beyond[d["planted"]["far"]].all())
        assert not bool(beyond[d["planted"]["below"]].any())
        if d["r_start"] < 1e-4:
            assert (got["edge_embedding"][d["planted"]["tiny"]] != 0).all()
        # zero-length edges: the oracle's row [1, 0, ..., 0], length exactly 0
        z = d["planted"]["zero"]
        assert z.numel() == 3 and (got["edge_lengths"][z] == 0).all() and (got["edge_vectors"][z] == 0).all()
        assert torch.equal(got["edge_attrs"][z], ref["edge_attrs"][z].float())
        assert (got["edge_attrs"][z][:, 0] == 1).all() and (got["edge_attrs"][z][:, 1:] == 0).all()

    again = _run(d)
    assert all(torch.equal(again[k], out[k]) for k in OUTPUTS), "a second call returns the same bits"


def test_edge_geom_leaves_no_uninitialised_output(edge_case, monkeypatch):
    d = edge_case
    want = _run(d)
    with monkeypatch.context() as m:
        nan_filled_empty(m)
        assert torch.isnan(torch.empty(4, device=DEV)).all()
        got = _run(d)
        torch.cuda.synchronize()
    for k in OUTPUTS:
        assert not torch.isnan(got[k]).any(), f"{d['name']}: NaN left in {k}"
        assert torch.equal(got[k], want[k]), k


@pytest.mark.parametrize("lmax", range(5))
def test_zero_length_edges_forward_and_adjoint(lmax):
    """a self edge with a zero shift and two coincident atoms: harmonics [1, 0, ..., 0] as the oracle's (which normalises
    the vector to 0), length exactly 0, and matten_edge_geom_bwd sends nothing back through them"""
    from matten_amd import ops
    from oracle.e3nn_lite.o3 import spherical_harmonics

    gen = torch.Generator().manual_seed(7100 + lmax)
    pos = torch.tensor([[0.3, 1.7, 2.9], [1.1, 0.2, 0.6], [1.1, 0.2, 0.6], [2.0, 2.5, 0.5], [3.1, 0.4, 1.2]])
    edge_index = torch.tensor([[0, 1, 2, 3, 4], [0, 2, 1, 4, 3]])
    N, E = 5, 5
    cell = (torch.eye(3) * 4.0 + 0.5 * torch.randn(1, 3, 3, generator=gen))
    shift = torch.zeros(E, 3)
    ei = edge_index.to(DEV)
    perm, rowptr, src_sorted, err = ops.csr_build(ei, N)
    assert int(err.item()) == 0
    out_perm, out_ptr, _, _ = ops.csr_build(torch.stack([src_sorted.long(), src_sorted.long()]), N)
    fwd = ops.edge_geom(pos.to(DEV), ei, shift.to(DEV), cell.to(DEV), None, perm, lmax, want_lengths=True, want_attrs=True)
    sh_dim = (lmax + 1) ** 2
    want = spherical_harmonics(list(range(lmax + 1)), torch.zeros(1, 3, dtype=torch.float64), True, "component")
    assert want[0, 0] == 1 and (want[0, 1:] == 0).all()
    attrs, lens = fwd["edge_attrs"].cpu(), fwd["edge_lengths"].cpu()
    assert (lens[:3] == 0).all() and (lens[3:] > 0).all()
    for e in range(3):
        assert torch.equal(attrs[e], want[0].float()), (e, attrs[e])
    pl = perm.long().cpu()
    assert torch.equal(fwd["sh_sorted"].cpu()[:, :sh_dim], attrs[pl]) and (fwd["sh_sorted"][:, sh_dim:] == 0).all()
    dy = torch.full((E, SH_STRIDE), float("nan"))
    dy[:, :sh_dim] = torch.randn(E, sh_dim, generator=gen)
    dlen = torch.randn(E, generator=gen)
    torch.full((N, 3), float("nan"), device=DEV)
    dpos, dcell = ops.edge_geom_bwd(fwd["geom_sorted"], dy[pl].to(DEV), dlen[pl].to(DEV), lmax, N, rowptr, (out_ptr, out_perm),
                                    perm, shift.to(DEV), 1, None)
    dpos = dpos.cpu()
    assert (dpos[:3] == 0).all(), "no gradient through a zero-length edge"
    assert torch.isfinite(dpos).all() and (dpos[3:].abs().amax(1) > 0).all()
    assert (dcell == 0).all(), "every shift is zero"


if __name__ == "__main__":   # the fp32-torch errors behind the bounds (CPU only)
    w = fp32_torch_errors()
    print(f"vectors {w['vec']:.2e}  lengths {w['len']:.2e}")
    print("harmonics l = 0..4: " + "  ".join(f"{x:.2e}" for x in w["sh"]))
    for r in RBF:
        print(f"embedding (nb, r_start, r_end) = {r}: {w['emb'][r]:.2e}")
