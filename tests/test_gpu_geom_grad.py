"""
Gradients with respect to atomic positions and cells: the three operator adjoints against fp64 autograd, then the whole
chain structure -> tensor -> modulus against the CPU oracle's autograd.

    matten_tp_backward_sh       dY[e] = dL/d(harmonics of edge e): fp64 autograd through the oracle's TensorProduct
    matten_radial_mlp_bwd_len   dlen[e] = dL/d(length of edge e): fp64 autograd through the oracle's Bessel basis and a plain MLP
    matten_edge_geom_bwd        dpos, dcell: fp64 autograd through normalise + the oracle's harmonics + the length

Operator bounds.  Each is 4 x the error of an fp32 torch evaluation of the same reference expression against its fp64
evaluation on this file's inputs (worst case over the cases, relative to the largest |reference| of the block compared:
a degree block l2 of dY, the whole of dlen, dpos, dcell): the factor covers another summation order, not other arithmetic.
`PYTHONPATH=.:tests python tests/test_gpu_geom_grad.py` prints the fp32-torch errors the constants were taken from (CPU only).
    fp32 torch vs fp64, worst:  dY 6.87e-7   dlen 1.43e-5   dpos 4.71e-7   dcell 3.65e-7
Worst error / allowed of the kernels, measured on MI355X:
    dY   fp32 0.080     bf16 w (the reference sees the rounded w) 0.070
    dlen 0.16
    dpos 0.18   dcell 0.21
(dY sums up to a few thousand terms per edge -- 200 channels x 5 paths in "wide200" -- and stays at 2.2e-7 of the block
maximum: a lane adds its channels in sequence, the lanes meet in a tree.)
End to end the bound is the project's gradient tolerance, 3e-3 of the largest reference entry
(test_training_step_matches_oracle_autograd); measured worst error / allowed: 1.1e-3 (lmax2 train() pos.grad; eval() cases
2e-4 .. 3e-4); sum of pos.grad per crystal 8e-8 .. 3e-7 of its largest entry (allowed 1e-5); strain asymmetry 5e-8
(allowed 1e-4).
"""
import copy
import math
import os

import pytest
import torch

from common import ATOMIC, LMAX2, PAPER, build_pair
from test_gpu_tp_adjoint import IRREPS, _graph, _oracle_tp, _sh_irreps

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
AVG = 18.0
SH_STRIDE = 32
# 4 x the fp32-torch error of the reference expression (module docstring)
DY_RTOL = 4 * 6.87e-7
DLEN_RTOL = 4 * 1.43e-5
DPOS_RTOL = 4 * 4.71e-7
DCELL_RTOL = 4 * 3.65e-7
E2E_RTOL = 3e-3
R_START, R_END, NB = 0.5, 5.0, 8

DY_IRREPS = ("lmax2", "paper", "ragged", "wide200")
DY_GRAPHS = ("tiny", "empty", "hubs", "e65")
DY_CASES = ([(i, g, n, "fp32") for i in DY_IRREPS for g in DY_GRAPHS for n in ("avg", "node")]
            + [("lmax2", "hubs", "avg", "bf16")])
DLEN_CASES = [(E, W, depth) for E in (1, 17, 300) for W in (16, 842) for depth in (1, 2, 4)]
GEOM_CASES = [(lmax, cells) for lmax in range(5) for cells in ("three", "one", "none")]


def _ratio(err, allowed):
    if allowed > 0:
        return err / allowed
    return 0.0 if err == 0 else math.inf


# ---------------------------------------------------------------------------------------------------------------------
# dY
# ---------------------------------------------------------------------------------------------------------------------
def _dy_graph(kind, gen):
    if kind == "e65":   # one edge past a wave
        return torch.randint(9, (2, 65), generator=gen), 9
    return _graph(kind, gen)


def _dy_inputs(case):
    """host operands of one dY case (fp32 values) and the oracle's tensor product"""
    from matten_amd import plan as mplan
    from oracle.e3nn_lite.o3 import spherical_harmonics

    irreps_name, graph, norm, storage = case
    irreps_in, lmax, target = IRREPS[irreps_name]
    gen = torch.Generator().manual_seed(3000 + DY_CASES.index(case))
    p = mplan.plan_uvu(irreps_in, _sh_irreps(lmax), target or irreps_in)
    tp = _oracle_tp(irreps_in, lmax, target)
    edge_index, N = _dy_graph(graph, gen)
    E, W = edge_index.shape[1], p.weight_numel
    x = torch.randn(N, p.d_in, generator=gen)
    g = torch.randn(N, p.d_mid, generator=gen)
    vec = torch.randn(E, 3, generator=gen, dtype=torch.float64)
    Y = spherical_harmonics(list(range(lmax + 1)), vec, True, "component").float()
    w = torch.randn(E, W, generator=gen)
    if storage == "bf16":
        w = w.bfloat16().float()
    in_deg = torch.bincount(edge_index[1], minlength=N)
    nrm = torch.full((N,), AVG ** -0.5, dtype=torch.float64) if norm == "avg" else \
        torch.where(in_deg > 0, in_deg.double().clamp(min=1) ** -0.5, torch.zeros((), dtype=torch.float64))
    return dict(p=p, tp=tp, lmax=lmax, edge_index=edge_index, N=N, E=E, W=W, x=x, g=g, Y=Y, w=w, nrm=nrm, in_deg=in_deg,
                norm=norm, bf16=storage == "bf16")


def _dy_reference(d, dtype):
    """dL/dY [E, sh_dim] (original edge order) of L = sum_e nrm[dst] <g[dst], tp(x[src], Y_e, w_e)> by autograd in `dtype`"""
    src, dst = d["edge_index"]
    tp = copy.deepcopy(d["tp"]).to(dtype)
    Y = d["Y"].to(dtype).clone().requires_grad_(True)
    if d["E"] == 0:
        return torch.zeros_like(Y)
    out = tp(d["x"].to(dtype)[src], Y, d["w"].to(dtype))
    L = (out * d["g"].to(dtype)[dst] * d["nrm"].to(dtype)[dst][:, None]).sum()
    return torch.autograd.grad(L, Y)[0].detach()


def _dy_errors(got, ref, lmax):
    """per degree block l2: max |got - ref| / max |ref| -> list"""
    out = []
    for l2 in range(lmax + 1):
        sl = slice(l2 * l2, (l2 + 1) ** 2)
        scale = ref[:, sl].abs().max().item() if ref.numel() else 0.0
        err = (got[:, sl].double() - ref[:, sl]).abs().max().item() if ref.numel() else 0.0
        out.append((err, scale))
    return out


@pytest.fixture(scope="module", params=DY_CASES, ids=["-".join(c) for c in DY_CASES])
def dy_case(request):
    from matten_amd import ops
    from matten_amd.nn._tables import DeviceTables

    d = _dy_inputs(request.param)
    d["name"] = "-".join(request.param)
    p, N, E, W = d["p"], d["N"], d["E"], d["W"]
    d["t"] = DeviceTables(bw_blocks=p.bw_blocks, bw_paths=p.bw_paths)
    ei = d["edge_index"].to(DEV)
    perm, rowptr, src_sorted, err = ops.csr_build(ei, N)
    assert int(err.item()) == 0
    d["perm"] = perm.long().cpu()
    d["src"] = src_sorted
    d["dst"] = ei[1][perm.long()].to(torch.int32).contiguous()
    nan = float("nan")
    out_deg = torch.bincount(d["edge_index"][0], minlength=N)
    xd, gd = d["x"].clone(), d["g"].clone()
    xd[out_deg == 0] = nan          # never read: no edge leaves these nodes
    gd[d["in_deg"] == 0] = nan      # never read: no edge arrives
    d["xd"], d["gd"] = xd.to(DEV), gd.to(DEV)
    w_pad = (W + 16) // 16 * 16
    wd = torch.full((E, w_pad), nan)   # the pad columns of the weight rows hold NaN
    wd[:, :W] = d["w"]
    d["wd"] = wd[d["perm"]].to(DEV, torch.bfloat16 if d["bf16"] else torch.float32)
    d["nn"] = d["in_deg"].float().to(DEV) if d["norm"] == "node" else None
    d["ref"] = _dy_reference(d, torch.float64)[d["perm"]]
    yield d
    torch.cuda.synchronize()


def _run_dy(d):
    from matten_amd import ops

    p, t = d["p"], d["t"]
    torch.full((d["E"], SH_STRIDE), float("nan"), device=DEV)   # what the allocator hands out next must not pass as zeros
    return ops.tp_backward_sh(d["xd"], d["wd"], d["src"], d["dst"], t.get("bw_blocks", DEV), t.get("bw_paths", DEV),
                              p.bw_max_mul, d["gd"], AVG if d["norm"] == "avg" else 0.0, d["nn"], max_l=p.bw_max_l,
                              sh_stride=SH_STRIDE)


def test_dy_matches_fp64_per_degree(dy_case):
    d = dy_case
    dy = _run_dy(d)
    assert dy.shape == (d["E"], SH_STRIDE) and dy.dtype == torch.float32
    sh_dim = (d["lmax"] + 1) ** 2
    assert (dy[:, sh_dim:] == 0).all(), "columns past (lmax+1)^2 are exact zeros"
    got = dy.cpu()
    assert torch.isfinite(got).all()
    worst = 0.0
    for l2, (err, scale) in enumerate(_dy_errors(got, d["ref"], d["lmax"])):
        r = _ratio(err, DY_RTOL * scale)
        print(f"\nGEOM_GRAD dY {d['name']} l2={l2} err {err:.3e} scale {scale:.3e} ratio {r:.3g}")
        worst = max(worst, r)
    assert worst <= 1.0, f"{d['name']}: dY error / allowed = {worst:.3g}"
    again = _run_dy(d)
    assert torch.equal(again, dy), "a second call returns the same bits"


# ---------------------------------------------------------------------------------------------------------------------
# dlen
# ---------------------------------------------------------------------------------------------------------------------
def _dlen_inputs(case):
    E, W, depth = case
    gen = torch.Generator().manual_seed(4000 + DLEN_CASES.index(case))
    n_mid = depth - 1
    w_pad = (W + 15) // 16 * 16
    nb_pad = (NB + 3) // 4 * 4
    w0p = torch.zeros(nb_pad, 32)
    w0p[:NB] = torch.randn(NB, 32, generator=gen) / NB ** 0.5
    w_mid = torch.randn(n_mid, 32, 32, generator=gen) * (1.679 / 32 ** 0.5)
    w2p = torch.zeros(32, w_pad)
    w2p[:, :W] = torch.randn(32, W, generator=gen) * (1.679 / 32 ** 0.5)
    r = R_START + 0.2 + (R_END - R_START - 0.4) * torch.rand(E, generator=gen)
    if E >= 4:
        r[0] = R_START - 0.2     # below r_start: exact zero expected
        r[1] = R_END + 0.5       # beyond r_end: exact zero expected
        r[2] = R_START + 0.01    # near r_start
        r[3] = R_END - 0.01
    dw = torch.randn(E, w_pad, generator=gen)
    return dict(E=E, W=W, n_mid=n_mid, w_pad=w_pad, w0p=w0p, w_mid=w_mid, w2p=w2p, r=r, dw=dw)


def _dlen_reference(d, dtype):
    """dL/dr of L = <dw, MLP(bessel(r))> by autograd in `dtype`: the oracle's basis (times sqrt(nb)), silu layers, the
    packed matrices as the kernels read them"""
    from oracle.e3nn_lite.math import soft_one_hot_linspace

    r = d["r"].to(dtype).clone().requires_grad_(True)
    emb = soft_one_hot_linspace(r, R_START, R_END, NB, basis="bessel", cutoff=True) * NB ** 0.5
    h = torch.nn.functional.silu(emb @ d["w0p"][:NB].to(dtype))
    for m in range(d["n_mid"]):
        h = torch.nn.functional.silu(h @ d["w_mid"][m].to(dtype))
    w = h @ d["w2p"][:, : d["W"]].to(dtype)
    return torch.autograd.grad((w * d["dw"][:, : d["W"]].to(dtype)).sum(), r)[0].detach()


@pytest.mark.parametrize("case", DLEN_CASES, ids=[f"E{e}-W{w}-L{dp}" for e, w, dp in DLEN_CASES])
def test_dlen_matches_fp64(case):
    from matten_amd import ops

    d = _dlen_inputs(case)
    ref = _dlen_reference(d, torch.float64)
    geom = torch.full((d["E"], 4), float("nan"))
    geom[:, 3] = d["r"]
    dw = d["dw"].clone()
    dw[:, d["W"]:] = float("nan")     # pad columns of dw are never read as data
    args = (geom.to(DEV), NB, R_START, R_END, d["w0p"].to(DEV), d["w_mid"].to(DEV), d["w2p"].to(DEV), d["W"], dw.to(DEV))
    got = ops.radial_mlp_bwd_len(*args)
    assert got.shape == (d["E"],) and got.dtype == torch.float32
    again = ops.radial_mlp_bwd_len(*args)
    assert torch.equal(got, again)
    got = got.cpu()
    if d["E"] >= 4:
        assert got[0] == 0 and got[1] == 0 and ref[0] == 0 and ref[1] == 0, "outside the basis' support: exact zeros"
    err, scale = (got.double() - ref).abs().max().item(), ref.abs().max().item()
    r = _ratio(err, DLEN_RTOL * scale)
    print(f"\nGEOM_GRAD dlen {case} err {err:.3e} scale {scale:.3e} ratio {r:.3g}")
    assert r <= 1.0, f"dlen {case}: error / allowed = {r:.3g}"
    if d["n_mid"] == 1:   # the shipped depth: one [32, 32] middle layer is taken as well
        assert torch.equal(ops.radial_mlp_bwd_len(*args[:5], d["w_mid"][0].to(DEV), *args[6:]).cpu(), got)


# ---------------------------------------------------------------------------------------------------------------------
# edge_geom_bwd
# ---------------------------------------------------------------------------------------------------------------------
def _geom_inputs(case):
    """three small crystals with different cells; self-image edges (src == dst, non-zero shift); atom 5 has no edge"""
    lmax, cells = case
    gen = torch.Generator().manual_seed(5000 + GEOM_CASES.index(case))
    sizes = [7, 6, 7] if cells == "three" else [20]
    N = sum(sizes)
    batch = torch.cat([torch.full((n,), b, dtype=torch.int64) for b, n in enumerate(sizes)])
    B = len(sizes)
    cell = (torch.eye(3) * 4.0 + 0.5 * torch.randn(B, 3, 3, generator=gen)) * (1.0 + 0.3 * torch.arange(B)[:, None, None])
    pos = 4.0 * torch.rand(N, 3, generator=gen)
    src, dst, shift = [], [], []
    first = 0
    for n in sizes:
        k = 7 * n
        s = first + torch.randint(n, (k,), generator=gen)
        t = first + torch.randint(n, (k,), generator=gen)
        sh = torch.randint(-1, 2, (k, 3), generator=gen).float()
        if cells == "none":
            sh.zero_()
        keep = (s != t) & (s != 5) & (t != 5)
        src.append(s[keep]), dst.append(t[keep]), shift.append(sh[keep])
        if cells != "none":   # self images
            for a in (first, first + 2, first + n - 1):
                if a != 5:
                    src.append(torch.tensor([a, a])), dst.append(torch.tensor([a, a]))
                    shift.append(torch.tensor([[1.0, 0.0, 0.0], [0.0, -1.0, 1.0]]))
        first += n
    edge_index = torch.stack([torch.cat(src), torch.cat(dst)])
    shift = torch.cat(shift)
    order = torch.randperm(edge_index.shape[1], generator=gen)
    edge_index, shift = edge_index[:, order], shift[order]
    E = edge_index.shape[1]
    dy = torch.randn(E, (lmax + 1) ** 2, generator=gen)
    dlen = torch.randn(E, generator=gen)
    return dict(lmax=lmax, cells=cells, N=N, B=B, E=E, batch=batch, cell=None if cells == "none" else cell, pos=pos,
                edge_index=edge_index, shift=shift, dy=dy, dlen=dlen)


def _geom_reference(d, dtype):
    """(dpos, dcell) of L = <dy, Y(n)> + <dlen, r> by autograd in `dtype` (original edge order throughout)"""
    from oracle.e3nn_lite.o3 import spherical_harmonics

    pos = d["pos"].to(dtype).clone().requires_grad_(True)
    src, dst = d["edge_index"]
    v = pos[dst] - pos[src]
    cell = None
    if d["cell"] is not None:
        cell = d["cell"].to(dtype).clone().requires_grad_(True)
        v = v + torch.einsum("ni,nij->nj", d["shift"].to(dtype), cell[d["batch"][src]])
    r = v.norm(dim=1)
    n = torch.nn.functional.normalize(v, dim=1)
    Y = spherical_harmonics(list(range(d["lmax"] + 1)), n, False, "component")
    L = (Y * d["dy"].to(dtype)).sum() + (r * d["dlen"].to(dtype)).sum()
    grads = torch.autograd.grad(L, (pos,) if cell is None else (pos, cell))
    return grads[0].detach(), (None if cell is None else grads[1].detach())


@pytest.mark.parametrize("case", GEOM_CASES, ids=[f"lmax{l}-{c}" for l, c in GEOM_CASES])
def test_edge_geom_bwd_matches_fp64(case):
    from matten_amd import ops

    d = _geom_inputs(case)
    ref_pos, ref_cell = _geom_reference(d, torch.float64)
    N, E, B = d["N"], d["E"], d["B"]
    ei = d["edge_index"].to(DEV)
    perm, rowptr, src_sorted, err = ops.csr_build(ei, N)
    assert int(err.item()) == 0
    pairs = torch.stack([src_sorted.long(), src_sorted.long()])
    out_perm, out_ptr, _, _ = ops.csr_build(pairs, N)
    cell = None if d["cell"] is None else d["cell"].to(DEV)
    shift = d["shift"].to(DEV)
    batch = d["batch"].to(DEV)
    fwd = ops.edge_geom(d["pos"].to(DEV), ei, shift, cell, batch if B > 1 else None, perm, d["lmax"])
    pl = perm.long().cpu()
    dy = torch.full((E, SH_STRIDE), float("nan"))
    dy[:, : (d["lmax"] + 1) ** 2] = d["dy"]
    dy, dlen = dy[pl].to(DEV), d["dlen"][pl].to(DEV)
    ptr = torch.searchsorted(batch, torch.arange(B + 1, device=DEV)) if B > 1 else None

    def run():
        torch.full((N, 3), float("nan"), device=DEV)
        return ops.edge_geom_bwd(fwd["geom_sorted"], dy, dlen, d["lmax"], N, rowptr, (out_ptr, out_perm), perm,
                                 shift if cell is not None else None, B if cell is not None else 0, ptr)

    dpos, dcell = run()
    dpos2, dcell2 = run()
    assert torch.equal(dpos, dpos2) and (dcell is None or torch.equal(dcell, dcell2)), "bitwise repeatable"
    assert dpos.shape == (N, 3) and (dpos[5] == 0).all(), "an atom without edges gets exact zeros"
    err, scale = (dpos.double().cpu() - ref_pos).abs().max().item(), ref_pos.abs().max().item()
    r_pos = _ratio(err, DPOS_RTOL * scale)
    print(f"\nGEOM_GRAD dpos {case} err {err:.3e} scale {scale:.3e} ratio {r_pos:.3g}")
    assert r_pos <= 1.0, f"dpos {case}: error / allowed = {r_pos:.3g}"
    if cell is None:
        assert dcell is None
    else:
        assert dcell.shape == (B, 3, 3)
        err, scale = (dcell.double().cpu() - ref_cell).abs().max().item(), ref_cell.abs().max().item()
        r_cell = _ratio(err, DCELL_RTOL * scale)
        print(f"\nGEOM_GRAD dcell {case} err {err:.3e} scale {scale:.3e} ratio {r_cell:.3g}")
        assert r_cell <= 1.0, f"dcell {case}: error / allowed = {r_cell:.3g}"
        assert (ref_cell.abs().amax(dim=(1, 2)) > 0).all()
    # parts: dY alone, dlen alone, neither (zeros), and the empty batch
    only_y = ops.edge_geom_bwd(fwd["geom_sorted"], dy, None, d["lmax"], N, rowptr, (out_ptr, out_perm))[0]
    only_l = ops.edge_geom_bwd(fwd["geom_sorted"], None, dlen, d["lmax"], N, rowptr, (out_ptr, out_perm))[0]
    assert (only_y.double() + only_l.double() - dpos.double()).abs().max().item() <= DPOS_RTOL * ref_pos.abs().max().item()
    none = ops.edge_geom_bwd(fwd["geom_sorted"], None, None, d["lmax"], N, rowptr, (out_ptr, out_perm))[0]
    assert (none == 0).all()


def test_edge_geom_bwd_empty_batch_zeroes_the_outputs():
    from matten_amd import ops

    N, B = 4, 2
    z32 = torch.zeros(N + 1, dtype=torch.int32, device=DEV)
    e32 = torch.zeros(0, dtype=torch.int32, device=DEV)
    torch.full((N, 3), float("nan"), device=DEV)
    dpos, dcell = ops.edge_geom_bwd(torch.zeros(0, 4, device=DEV), None, None, 2, N, z32, (z32, e32), e32,
                                    torch.zeros(0, 3, device=DEV), B, torch.tensor([0, 2, 4], device=DEV))
    assert (dpos == 0).all() and dpos.shape == (N, 3) and (dcell == 0).all() and dcell.shape == (B, 3, 3)


# ---------------------------------------------------------------------------------------------------------------------
# end to end: structure -> tensor -> scalar, against the oracle's autograd
# ---------------------------------------------------------------------------------------------------------------------
HPS = {"lmax2": LMAX2, "paper": PAPER}
_CACHE = {}


def _rattled(golden_dir):
    """the first 3 crystals of the n100 sample, positions rattled by a seeded N(0, 0.05 A): ONE graph for both sides
    (unrattled, crystal 0's position gradient is identically zero by symmetry)"""
    if "graphs" not in _CACHE:
        import numpy as np

        from matten_amd.data.graph import average_num_neighbors, crystal_graph
        from oracle.matten_ref.data import structures_from_json

        structs = structures_from_json(os.path.join(golden_dir, "example_crystal_elasticity_tensor_n100.json"))[:3]
        rng = np.random.default_rng(11)
        graphs = [crystal_graph(np.asarray(s["cart_coords"]) + rng.normal(0.0, 0.05, np.asarray(s["cart_coords"]).shape),
                                s["lattice"], s["atomic_numbers"], 5.0) for s in structs]
        species = sorted({int(z) for s in structs for z in s["atomic_numbers"]})
        _CACHE["graphs"] = (graphs, {"allowed_species": species, "average_num_neighbors": average_num_neighbors(graphs)})
    return _CACHE["graphs"]


def _pair(golden_dir, name):
    if name not in _CACHE:
        graphs, ds = _rattled(golden_dir)
        hp, atomic = (ATOMIC, True) if name == "atomic" else (HPS[name], False)
        _CACHE[name] = build_pair(dict(hp), ds, randomize_bn=True, atomic=atomic)
    return _CACHE[name]


def _oracle_grads(ref, graphs, cot):
    """(pos.grad, cell.grad) of <cot, ref.decode(batch)> by the oracle's autograd"""
    from matten_amd.data.graph import collate

    b = collate(graphs)
    b["pos"].requires_grad_(True)
    b["cell"].requires_grad_(True)
    out = ref.decode(b)
    (out * cot).sum().backward()
    return b["pos"].grad, b["cell"].grad, b


def _device_grads(model, graphs, cot, flags=("pos", "cell"), **kw):
    from matten_amd.data.graph import collate

    b = collate(graphs, device=DEV)
    for k in flags:
        b[k].requires_grad_(True)
    preds, _ = model(b, **kw)
    out = preds[kw.get("task_name", "elastic_tensor_full")]
    (out * cot.to(DEV)).sum().backward()
    return b


def _close(got, want, rtol, what):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    scale = max(1e-12, want.abs().max().item())
    err = (got - want).abs().max().item()
    print(f"\nGEOM_GRAD e2e {what}: err {err:.3e} scale {scale:.3e} ratio {err / (rtol * scale):.3g}")
    assert err <= rtol * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e}"


def _bn_state(*mods):
    return [copy.deepcopy({k: v.clone() for k, v in m.named_buffers()}) for m in mods]


def _restore(mods, states):
    for m, st in zip(mods, states):
        for k, v in m.named_buffers():
            v.copy_(st[k])


@pytest.mark.parametrize("mode", ["eval", "train"])
@pytest.mark.parametrize("hp_name", ["lmax2", "paper"])
def test_position_and_cell_gradients_match_the_oracle(golden_dir, hp_name, mode):
    graphs, _ = _rattled(golden_dir)
    ref, model = _pair(golden_dir, hp_name)
    cot = torch.randn(len(graphs), 21, generator=torch.Generator().manual_seed(7))
    saved = _bn_state(ref, model)
    try:
        ref.train(mode == "train"), model.train(mode == "train")
        pos_r, cell_r, _ = _oracle_grads(ref, graphs, cot)
        b = _device_grads(model, graphs, cot)
    finally:
        ref.eval(), model.eval()
        with torch.no_grad():
            _restore((ref, model), saved)
        model.zero_grad(), ref.zero_grad()
    assert pos_r.abs().max() > 0 and cell_r.abs().max() > 0
    _close(b["pos"].grad, pos_r, E2E_RTOL, f"{hp_name} {mode} pos.grad")
    _close(b["cell"].grad, cell_r, E2E_RTOL, f"{hp_name} {mode} cell.grad")
    # translation invariance: a crystal's position gradients add up to nothing
    g = b["pos"].grad.double().cpu()
    sums = torch.zeros(len(graphs), 3, dtype=torch.float64).index_add_(0, b["batch"].cpu(), g)
    print(f"\nGEOM_GRAD e2e {hp_name} {mode} sum of pos.grad per crystal / largest entry {sums.abs().max().item() / g.abs().max().item():.3e}")
    assert sums.abs().max().item() <= 1e-5 * g.abs().max().item()


def test_saliency_with_everything_frozen_in_eval(golden_dir):
    """pure saliency: every parameter frozen, eval(), only the geometry requires grad"""
    graphs, _ = _rattled(golden_dir)
    ref, model = _pair(golden_dir, "lmax2")
    cot = torch.randn(len(graphs), 21, generator=torch.Generator().manual_seed(7))
    pos_r, cell_r, _ = _oracle_grads(ref, graphs, cot)
    ref.zero_grad()
    params = list(model.parameters())
    try:
        for p in params:
            p.requires_grad_(False)
        only_pos = _device_grads(model, graphs, cot, flags=("pos",))
        both = _device_grads(model, graphs, cot)
    finally:
        for p in params:
            p.requires_grad_(True)
    assert only_pos["cell"].grad is None and all(p.grad is None for p in params)
    _close(only_pos["pos"].grad, pos_r, E2E_RTOL, "frozen, pos only: pos.grad")
    _close(both["pos"].grad, pos_r, E2E_RTOL, "frozen: pos.grad")
    _close(both["cell"].grad, cell_r, E2E_RTOL, "frozen: cell.grad")
    assert torch.equal(both["pos"].grad, only_pos["pos"].grad)


def test_saliency_on_the_large_batch_inference_route(golden_dir, monkeypatch):
    """from AGG_KM_MIN_ROWS atoms on, an inference forward streams lin2 (and Gate + BatchNorm) from component-major
    neighbour sums; with the geometry requiring grad the layers must leave that route although no parameter and no
    node feature asks for it.  The threshold is lowered to this batch instead of building 8192 atoms."""
    from matten_amd.nn import conv

    graphs, _ = _rattled(golden_dir)
    ref, model = _pair(golden_dir, "lmax2")
    cot = torch.randn(len(graphs), 21, generator=torch.Generator().manual_seed(7))
    pos_r, cell_r, _ = _oracle_grads(ref, graphs, cot)
    ref.zero_grad()
    monkeypatch.setattr(conv, "AGG_KM_MIN_ROWS", 1)
    params = list(model.parameters())
    try:
        for p in params:
            p.requires_grad_(False)
        b = _device_grads(model, graphs, cot)
    finally:
        for p in params:
            p.requires_grad_(True)
    _close(b["pos"].grad, pos_r, E2E_RTOL, "frozen, streaming-lin2 threshold at 1: pos.grad")
    _close(b["cell"].grad, cell_r, E2E_RTOL, "frozen, streaming-lin2 threshold at 1: cell.grad")


def test_parameter_gradients_do_not_depend_on_the_geometry_flags(golden_dir, monkeypatch):
    """a training step's parameter gradients are bit for bit the same whether pos requires grad or not (paths route)"""
    monkeypatch.setenv("MATTEN_TRAIN_TP", "paths")
    graphs, _ = _rattled(golden_dir)
    ref, model = _pair(golden_dir, "lmax2")
    cot = torch.randn(len(graphs), 21, generator=torch.Generator().manual_seed(7))
    saved = _bn_state(model)
    runs = []
    try:
        model.train()
        for flags in ((), ("pos", "cell")):
            with torch.no_grad():
                _restore((model,), saved)
            model.zero_grad()
            _device_grads(model, graphs, cot, flags=flags)
            runs.append({k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None})
    finally:
        model.eval()
        with torch.no_grad():
            _restore((model,), saved)
        model.zero_grad()
    assert runs[0] and set(runs[0]) == set(runs[1])
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k


def test_table_adjoint_with_geometry_gradients_names_the_switch(golden_dir, monkeypatch):
    monkeypatch.setenv("MATTEN_TP_BWD", "table")
    graphs, _ = _rattled(golden_dir)
    _, model = _pair(golden_dir, "lmax2")
    cot = torch.randn(len(graphs), 21)
    with pytest.raises(NotImplementedError, match="MATTEN_TP_BWD"):
        _device_grads(model, graphs, cot)
    model.zero_grad()


def test_strain_gradient_of_the_bulk_modulus_and_geometry_gradients(golden_dir):
    """loss = k_vrh.sum() through elastic_moduli_from_irreps: the strain gradient is symmetric (k_vrh is rotation
    invariant), and geometry_gradients agrees with the oracle fed the device's own dL/dpreds as cotangent"""
    from matten_amd.data.graph import collate
    from matten_amd.elastic import elastic_moduli_from_irreps
    from matten_amd.geometry import geometry_gradients

    graphs, _ = _rattled(golden_dir)
    ref, model = _pair(golden_dir, "lmax2")
    seen = {}

    def loss(p):
        t = p["elastic_tensor_full"]
        t.register_hook(lambda g: seen.__setitem__("cot", g.detach().clone()))
        return elastic_moduli_from_irreps(t).k_vrh.sum()

    batch = collate(graphs, device=DEV)
    out = geometry_gradients(model, batch, loss)
    model.zero_grad()
    assert batch["pos"].grad is None and not batch["pos"].requires_grad, "the caller's tensors are left alone"
    s = out["strain"].double().cpu()
    assert s.shape == (len(graphs), 3, 3)
    asym = (s - s.transpose(1, 2)).abs().max().item()
    print(f"\nGEOM_GRAD e2e strain asymmetry / largest entry {asym / s.abs().max().item():.3e}")
    assert asym <= 1e-4 * s.abs().max().item()
    pos_r, cell_r, b = _oracle_grads(ref, graphs, seen["cot"].cpu().to(torch.float32))
    ref.zero_grad()
    _close(out["pos"], pos_r, E2E_RTOL, "geometry_gradients pos")
    _close(out["cell"], cell_r, E2E_RTOL, "geometry_gradients cell")
    want = torch.zeros(len(graphs), 3, 3).index_add_(0, b["batch"], b["pos"].detach().unsqueeze(2) * pos_r.unsqueeze(1)) \
        + b["cell"].detach().reshape(-1, 3, 3).transpose(1, 2) @ cell_r.reshape(-1, 3, 3)
    _close(out["strain"], want, E2E_RTOL, "geometry_gradients strain")


def test_without_a_flag_no_new_code_runs(golden_dir, monkeypatch):
    """an inference forward and a training step of a batch whose geometry does not require grad never reach the new
    operators, and the batch dict carries the keys it always did"""
    from matten_amd import autograd as ag, ops
    from matten_amd.data.graph import collate

    graphs, _ = _rattled(golden_dir)
    _, model = _pair(golden_dir, "lmax2")
    with torch.no_grad():
        want = model(collate(graphs, device=DEV))[0]["elastic_tensor_full"]
        keys = set(model(collate(graphs, device=DEV), mode="backbone")[0])

    def boom(*a, **k):
        raise AssertionError("geometry-gradient code ran without a geometry tensor that requires grad")

    for name in ("tp_backward_sh", "radial_mlp_bwd_len", "edge_geom_bwd"):
        monkeypatch.setattr(ops, name, boom)
    monkeypatch.setattr(ag.EdgeGeomFn, "apply", boom)
    with torch.no_grad():
        b = collate(graphs, device=DEV)
        got = model(b)[0]["elastic_tensor_full"]
        data = model(collate(graphs, device=DEV), mode="backbone")[0]
    assert torch.equal(got, want) and set(data) == keys
    assert not any(isinstance(v, torch.Tensor) and v.requires_grad for v in data.values())
    direct = ops.edge_geom(b["pos"], b["edge_index"], b["edge_cell_shift"], b["cell"], b["batch"], data["_amd_perm"], 2)
    assert torch.equal(data["_amd_geom_sorted"], direct["geom_sorted"]) and torch.equal(data["_amd_sh_sorted"], direct["sh_sorted"])
    assert {str(k) for k in keys} == INFERENCE_KEYS, sorted({str(k) for k in keys} ^ INFERENCE_KEYS)
    saved = _bn_state(model)
    try:
        model.train()
        _device_grads(model, graphs, torch.randn(len(graphs), 21), flags=())
    finally:
        model.eval()
        with torch.no_grad():
            _restore((model,), saved)
        model.zero_grad()


# the batch dict after an inference forward of the backbone, as before this file's feature existed
INFERENCE_KEYS = {
    "('_amd_csr_split', 8, True)", "_amd_csr_err", "_amd_geom_sorted", "_amd_h2s", "_amd_kept_irreps_only", "_amd_lmax", "_amd_perm",
    "_amd_rbf_params", "_amd_rowptr", "_amd_sh_sorted", "_amd_species_i32", "_amd_species_order", "_amd_src_sorted",
    "atomic_numbers", "batch", "cell", "edge_cell_shift", "edge_index", "my_model_output", "node_features", "num_neigh", "pos",
    "ptr", "species_index",
}


def test_atomic_tensor_model_position_gradients(golden_dir):
    graphs, _ = _rattled(golden_dir)
    ref, model = _pair(golden_dir, "atomic")
    n = sum(int(g["pos"].shape[0]) for g in graphs)
    cot = torch.randn(n, 6, generator=torch.Generator().manual_seed(9))
    pos_r, cell_r, _ = _oracle_grads(ref, graphs, cot)
    ref.zero_grad()
    b = _device_grads(model, graphs, cot, task_name="nmr_tensor")
    model.zero_grad()
    _close(b["pos"].grad, pos_r, E2E_RTOL, "atomic pos.grad")
    _close(b["cell"].grad, cell_r, E2E_RTOL, "atomic cell.grad")


if __name__ == "__main__":   # the fp32-torch errors behind the operator bounds (CPU only)
    worst = {"dY": 0.0, "dlen": 0.0, "dpos": 0.0, "dcell": 0.0}
    for case in DY_CASES:
        d = _dy_inputs(case)
        for err, scale in _dy_errors(_dy_reference(d, torch.float32), _dy_reference(d, torch.float64), d["lmax"]):
            worst["dY"] = max(worst["dY"], err / scale if scale else 0.0)
    for case in DLEN_CASES:
        d = _dlen_inputs(case)
        r64 = _dlen_reference(d, torch.float64)
        worst["dlen"] = max(worst["dlen"], ((_dlen_reference(d, torch.float32).double() - r64).abs().max() / r64.abs().max()).item())
    for case in GEOM_CASES:
        d = _geom_inputs(case)
        (p32, c32), (p64, c64) = _geom_reference(d, torch.float32), _geom_reference(d, torch.float64)
        worst["dpos"] = max(worst["dpos"], ((p32.double() - p64).abs().max() / p64.abs().max()).item())
        if c64 is not None:
            worst["dcell"] = max(worst["dcell"], ((c32.double() - c64).abs().max() / c64.abs().max()).item())
    print({k: f"{v:.2e}" for k, v in worst.items()})
