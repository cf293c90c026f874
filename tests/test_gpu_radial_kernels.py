"""The radial-MLP kernels per layer, adjoint form and length band against fp64 autograd of the plain formula: the
materialising forward (radial_mlp_kernel), the production forward's hidden layers (radial_hidden_kernel,
radial_hidden_multi_kernel: hardware sin / exp2 / rcp, split fp16 output), the weight adjoint in its two-kernel form
(radial_mlp_bwd_edges + radial_mlp_bwd_w2) and its one-kernel form (radial_mlp_bwd_fused at 4, 6 and 8 column chunks per
wave, one and two rounds per wave), and the operand packers (radial_pack_cols*, radial_h_scale*, split_a_tiles), exactly.

Cases, references and bounds: radial_cases.py (no tolerance here is chosen by hand: every allowed error is FACTOR x the
fp32-torch reference's own distance from fp64 on the block compared; the decoded split form adds the representation
error of its two fp16 halves, radial_cases.split_format_term).  Every run is made twice and compared bit for bit.

Every test prints its worst error / allowed ratio (lines starting with RADIAL).

measured on MI355X (worst error / allowed over the cases, per quantity and form; the whole file takes about 11 s):
    quantity        two-kernel   one-kernel/4   one-kernel/6   one-kernel/8
    dW0             0.188        0.139          0.0416         0.0758
    dWmid0          0.123        0.137          0.0325         0.0415
    dWmid1          0.184        0.146          -              -
    dWmid2          0.192        -              -              -
    dW2             0.0596       0.163          0.0429         0.0606
    quantity        near_start   mid            near_end       all
    w  (radial_mlp_deep)            0.174   0.194   0.191   0.174
    h  (radial_hidden_deep)         0.492   0.173   0.0901
    h  (radial_hidden_multi_deep)   0.400   0.135   0.411
The hardware sin / rcp / exp2 path of radial_hidden* stays inside every band's bound, the near-start band at
r_start = 0.5 and the near-end band included: no kernel was changed for these tests.

That the tests bite (each edit changes values only, run once on a scratch build, never committed):
    radial_mlp_bwd_fused without its `q + s < w_cols` select     test_weight_adjoint (every one-kernel case with pad
                                                                  columns), test_weight_adjoint_storage,
                                                                  test_same_bits_with_nan_filled_scratch[grid/w400/m1]
    radial_hidden_kernel with inv_xr = rcp(len)                  test_forward_per_band (every case with r_start = 0.5),
                                                                  test_hidden_multi_every_output (single launch differs)
    store_small with s0 and s1 swapped                           test_weight_adjoint, test_weight_adjoint_storage (every
                                                                  case of both)
"""
import functools

import pytest
import torch

import radial_cases as rc
from test_gpu_edge_geom import nan_filled_empty
from test_gpu_radial_depth import _h2s_features

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
WORST = {}      # (quantity, form) -> worst ratio seen in this session (printed by the last test)


def _form_name(form: int) -> str:
    return "two-kernel" if form == rc.TWO_KERNEL else f"one-kernel/{form}"


class _Checks:
    """prints every figure, keeps the failures, asserts at the end: a failing case shows all of its numbers"""

    def __init__(self, tag: str, form: str):
        self.tag, self.form, self.failed = tag, form, []

    def record(self, what: str, key: str, err: float, allowed: float):
        ratio = err / allowed if allowed > 0 else (0.0 if err == 0 else float("inf"))
        print(f"\nRADIAL {self.tag} {what}: err {err:.3e} allowed {allowed:.3e} ratio {ratio:.3g}", end="")
        k = (key, self.form)
        WORST[k] = max(WORST.get(k, 0.0), ratio)
        if not ratio <= 1.0:
            self.failed.append(f"{what}: err {err:.3e} > allowed {allowed:.3e} (ratio {ratio:.3g})")

    def block(self, what: str, key: str, got, ref, rows=None):
        """max |got - fp64| over the block against FACTOR x CONSTANTS[key] x the block's own largest reference value"""
        got = got.detach().cpu().double()
        assert got.shape == ref.shape, (what, got.shape, ref.shape)
        if rows is not None:
            if rows.numel() == 0:
                return
            got, ref = got[rows], ref[rows]
        scale = float(ref.abs().max())
        assert scale > 0, what
        self.record(what, key, float((got - ref).abs().max()), rc.allowed(key, scale))

    def require(self, ok: bool, what: str):
        if not ok:
            print(f"\nRADIAL {self.tag} FAILED: {what}", end="")
            self.failed.append(what)

    def done(self):
        print()
        assert not self.failed, f"{self.tag}: " + "; ".join(self.failed)


def _same_bits(a, b) -> bool:
    """bit for bit, NaN included (pad columns of dW2 in the two-kernel form are not numbers)"""
    if a.dtype in (torch.float32,):
        return torch.equal(a.view(torch.int32), b.view(torch.int32))
    if a.dtype in (torch.float16, torch.bfloat16):
        return torch.equal(a.view(torch.int16), b.view(torch.int16))
    return torch.equal(a, b)


@functools.lru_cache(maxsize=None)
def _inputs(name: str, mlp: int = 0):
    """device inputs of (case, MLP): geom with NaN in the three columns no radial kernel may read, raw and packed layers"""
    from matten_amd import ops

    p = rc.problem(name, mlp)
    case = p.case
    geom = torch.full((case.E, 4), NAN, device=DEV)
    geom[:, 3] = p.lens.to(DEV)
    raw = tuple(w.to(DEV) for w in (p.w0, p.wm, p.w2))
    packed = ops.radial_pack_deep(*raw, rc.scales(case))
    hs = ops.radial_h_scale_deep(raw[0], raw[1], case.r_start, case.r_end, rc.act_cst())
    return dict(geom=geom, raw=raw, packed=packed, hs=hs, args=(geom, case.nb, case.r_start, case.r_end))


def _check_hidden(ck: _Checks, what: str, p, h2s, s: float):
    """the split fp16 form decoded and divided by its scale s, per band; exact zeros outside the support"""
    h2s = h2s.cpu()
    assert h2s.shape == (p.case.E, 2, 32) and h2s.dtype == torch.float16
    dec = rc.decode_h2s(h2s)
    ck.require(torch.equal(_h2s_features(h2s), dec.float()), f"{what}: decode differs from _h2s_features")
    ck.require(bool(torch.isfinite(dec).all()), f"{what}: not finite")
    ck.require(bool((h2s[p.outside] == 0).all()), f"{what}: rows outside the support are not exactly zero in both halves")
    for band, rows in p.bands.items():
        if rows.numel() == 0:
            continue
        ref = p.h[rows]
        base = rc.allowed(f"h/{band}", float(ref.abs().max()))
        tot = base + rc.split_format_term((ref.abs() + base) * s) / s      # elementwise
        err = (dec[rows] / s - ref).abs()
        i = int(torch.argmax(err / tot))
        ck.record(f"{what} {band}", f"h/{band}", float(err.flatten()[i]), float(tot.flatten()[i]))


@pytest.mark.parametrize("name", list(rc.CASES))
def test_forward_per_band(name):
    """radial_mlp_deep (fp32 and bf16) and radial_hidden_deep on the same inputs"""
    from matten_amd import ops

    p, d = rc.problem(name), _inputs(name)
    case = p.case
    w0p, wmp, w2p = d["packed"]

    def run():
        return dict(w=ops.radial_mlp_deep(*d["args"], w0p, wmp, w2p),
                    wb=ops.radial_mlp_deep(*d["args"], w0p, wmp, w2p, out_dtype=torch.bfloat16),
                    h2s=ops.radial_hidden_deep(*d["args"], w0p, wmp, d["hs"]))

    a, b = run(), run()
    torch.cuda.synchronize()
    ck = _Checks(name, "forward")
    for k in a:
        ck.require(_same_bits(a[k], b[k]), f"{k} differs between two runs")
    w = a["w"].cpu()
    assert w.shape == (case.E, case.w_pad)
    ck.require(bool(torch.isfinite(w).all()), "w: not finite")
    ck.require(bool((w[:, case.W:] == 0).all()), "w: pad columns are not exactly zero")
    ck.require(bool((w[p.outside] == 0).all()), "w: rows outside the support are not exactly zero")
    ck.require(torch.equal(a["wb"].cpu(), w.bfloat16()), "bf16 output is not the round-to-nearest-even of the fp32 output")
    for band, rows in p.bands.items():
        ck.block(f"w {band}", f"w/{band}", w[:, :case.W], p.w, rows)
    ck.block("w all", "w/all", w[:, :case.W], p.w, p.compared)
    s = float(d["hs"][0])
    ck.require(0.0 < s <= 1.0 and float(d["hs"][1]) == 1.0 / s, f"h_scale {d['hs'].tolist()}")
    if case.weight_gain > 1:
        ck.require(s < 1.0, f"weights x {case.weight_gain:g} should need h_scale < 1, got {s}")
    _check_hidden(ck, "h2s", p, a["h2s"], s)
    ck.done()


@pytest.mark.parametrize("n_mlps", rc.MULTI_COUNTS)
@pytest.mark.parametrize("name", rc.MULTI_CASES)
def test_hidden_multi_every_output(name, n_mlps):
    """radial_hidden_multi_deep with 1, 4 and 8 MLPs of distinct weights and distinct output scales: every output"""
    from matten_amd import ops

    ds = [_inputs(name, j) for j in range(n_mlps)]
    # MLP j's own bound-derived scale times 2^-j: distinct per MLP, |s h| stays below the fp16 range
    hss = [torch.stack([d["hs"][0] * rc.multi_h_scale(j), d["hs"][1] / rc.multi_h_scale(j)]) for j, d in enumerate(ds)]
    run = lambda: ops.radial_hidden_multi_deep(*ds[0]["args"], [d["packed"][0] for d in ds], [d["packed"][1] for d in ds], hss)
    a, b = run(), run()
    torch.cuda.synchronize()
    ck = _Checks(f"{name} x{n_mlps}", "multi")
    assert len(a) == n_mlps
    for j in range(n_mlps):
        ck.require(_same_bits(a[j], b[j]), f"MLP {j} differs between two runs")
        _check_hidden(ck, f"MLP {j}", rc.problem(name, j), a[j], float(hss[j][0]))
    alone = ops.radial_hidden_deep(*ds[-1]["args"], ds[-1]["packed"][0], ds[-1]["packed"][1], hss[-1])
    ck.require(_same_bits(alone, a[-1]), "the last MLP differs from its single launch")
    ck.done()


def _device_dw(p, dtype: str, ld_extra: int):
    """dL/dw as the adjoint gets it: [E, dw_ld] fp32 or bf16, every column from W to dw_ld NaN"""
    case = p.case
    dt = torch.bfloat16 if dtype == "bf16" else torch.float32
    dw = torch.full((case.E, case.w_pad + ld_extra), NAN, dtype=dt, device=DEV)
    dw[:, :case.W] = p.gout.to(DEV).to(dt)
    return dw


def _run_adjoint(name: str, dtype: str = "fp32", ld_extra: int = 0):
    from matten_amd import ops

    p, d = rc.problem(name), _inputs(name)
    dw = _device_dw(p, dtype, ld_extra)
    return ops.radial_mlp_bwd_deep(*d["args"], *d["packed"], p.case.W, dw, scales=rc.scales(p.case))


def _check_adjoint(ck: _Checks, p, out, dtype: str):
    """d2[:, W:] is not asserted on: autograd._radial_mlp_bwd never uses it (the two-kernel form leaves what it read from
    dw's pad columns there, the one-kernel form zeros)"""
    case = p.case
    d0, dm, d2 = (t.cpu() for t in out)
    assert d0.shape == (case.nb_pad, 32) and dm.shape == (case.n_mid, 32, 32) and d2.shape == (32, case.w_pad)
    ck.require(not bool(torch.isnan(d0).any() | torch.isnan(dm).any() | torch.isnan(d2[:, :case.W]).any()),
               "NaN in dW0, dWmid or dW2[:, :W]")
    ck.require(bool((d0[case.nb:] == 0).all()), "rows nb..nb_pad of dW0 are not exactly zero")
    got = [d0[:case.nb], *dm.unbind(0), d2[:, :case.W]]
    for key, g, ref in zip(rc.grad_names(case.n_mid), got, p.grads[dtype]):
        ck.block(f"{key} (dw {dtype})", key, g, ref)


def _assert_form(case):
    """the partial-sum count is small_slices / 4 exactly when the one-kernel form runs (at 67 edges: 2 against 1 range)"""
    from matten_amd import _lib

    lib = _lib.load()
    for E in {67, case.E} - set(range(65)):             # (64 edges or fewer: one partial sum in either form)
        slices = lib.matten_radial_mlp_bwd_small_slices(E)
        assert slices == rc.small_slices(E), (E, slices)
        ranges = lib.matten_radial_mlp_bwd_w2_ranges_deep(E, case.w_pad, case.n_mid)
        assert (ranges == slices // 4) == (case.form != rc.TWO_KERNEL), \
            f"{case.name}: expected {_form_name(case.form)}, the library says {ranges} partial sums of {slices // 4} workgroups"


@pytest.mark.parametrize("name", rc.ADJOINT_CASES)
def test_weight_adjoint(name):
    p = rc.problem(name)
    _assert_form(p.case)
    a, b = _run_adjoint(name), _run_adjoint(name)
    torch.cuda.synchronize()
    ck = _Checks(name, _form_name(p.case.form))
    ck.require(all(_same_bits(x, y) for x, y in zip(a, b)), "gradients differ between two runs")
    _check_adjoint(ck, p, a, "fp32")
    ck.done()


@pytest.mark.parametrize("dtype,ld_extra", rc.STORAGE_FORMS)
@pytest.mark.parametrize("name", rc.STORAGE_CASES)
def test_weight_adjoint_storage(name, dtype, ld_extra):
    """bf16 dw (reference on the bf16-rounded values: the kernels compute in fp32, the fp32 bounds apply) and a strided dw"""
    p = rc.problem(name)
    a, b = _run_adjoint(name, dtype, ld_extra), _run_adjoint(name, dtype, ld_extra)
    torch.cuda.synchronize()
    ck = _Checks(f"{name} dw {dtype} ld+{ld_extra}", _form_name(p.case.form))
    ck.require(all(_same_bits(x, y) for x, y in zip(a, b)), "gradients differ between two runs")
    _check_adjoint(ck, p, a, dtype)
    if ld_extra:    # the row stride is an address, not a value
        plain = _run_adjoint(name, dtype, 0)
        W = p.case.W
        ck.require(_same_bits(plain[0], a[0]) and _same_bits(plain[1], a[1]) and
                   _same_bits(plain[2][:, :W].contiguous(), a[2][:, :W].contiguous()), "a strided dw changes the gradients")
    ck.done()


@pytest.mark.parametrize("name", rc.NAN_EMPTY_CASES)
def test_same_bits_with_nan_filled_scratch(name):
    """every scratch and output buffer starts as NaN: nothing unwritten is read or returned"""
    from matten_amd import ops

    p, d = rc.problem(name), _inputs(name)

    def run():
        w0p, wmp, w2p = ops.radial_pack_deep(*d["raw"], rc.scales(p.case))
        hs = ops.radial_h_scale_deep(d["raw"][0], d["raw"][1], p.case.r_start, p.case.r_end, rc.act_cst())
        out = [w0p, wmp, w2p, hs, ops.radial_mlp_deep(*d["args"], w0p, wmp, w2p),
               ops.radial_hidden_deep(*d["args"], w0p, wmp, hs),
               *ops.radial_hidden_multi_deep(*d["args"], [w0p, w0p], [wmp, wmp], [hs, hs])]
        d0, dm, d2 = ops.radial_mlp_bwd_deep(*d["args"], w0p, wmp, w2p, p.case.W, _device_dw(p, "fp32", 0),
                                             scales=rc.scales(p.case))
        torch.cuda.synchronize()
        return out + [d0, dm, d2[:, :p.case.W].contiguous()]

    want = run()
    with pytest.MonkeyPatch.context() as m:
        nan_filled_empty(m)
        assert torch.isnan(torch.empty(4, device=DEV)).all()
        got = run()
    for i, (x, y) in enumerate(zip(got, want)):
        assert not torch.isnan(x.float()).any(), f"{name}: NaN left in output {i}"
        assert _same_bits(x, y), f"{name}: output {i} changes with NaN-filled buffers"


def test_non_deep_entries_are_the_deep_ones_at_one_middle_layer():
    from matten_amd import ops

    name = rc.NON_DEEP_CASE
    p, d = rc.problem(name), _inputs(name)
    case = p.case
    assert case.n_mid == 1
    sc = rc.scales(case)
    w0p, wmp, w2p = d["packed"]
    q0, q1, q2 = ops.radial_pack(d["raw"][0], d["raw"][1][0], d["raw"][2], sc)
    assert torch.equal(q0, w0p) and torch.equal(q1, wmp[0]) and torch.equal(q2, w2p)
    for dt in (torch.float32, torch.bfloat16):
        assert _same_bits(ops.radial_mlp(*d["args"], q0, q1, q2, out_dtype=dt),
                          ops.radial_mlp_deep(*d["args"], w0p, wmp, w2p, out_dtype=dt))
    assert _same_bits(ops.radial_hidden(*d["args"], q0, q1, d["hs"]), ops.radial_hidden_deep(*d["args"], w0p, wmp, d["hs"]))
    m1 = ops.radial_hidden_multi(*d["args"], [q0, q0 * 0.5], [q1, q1], [d["hs"], d["hs"]])
    m2 = ops.radial_hidden_multi_deep(*d["args"], [w0p, w0p * 0.5], [wmp, wmp], [d["hs"], d["hs"]])
    assert all(_same_bits(x, y) for x, y in zip(m1, m2))
    dw = _device_dw(p, "fp32", 0)
    o = ops.radial_mlp_bwd(*d["args"], q0, q1, q2, case.W, dw, scales=sc)
    o2 = ops.radial_mlp_bwd_deep(*d["args"], w0p, wmp, w2p, case.W, dw, scales=sc)
    assert _same_bits(o[0], o2[0]) and _same_bits(o[1], o2[1][0]) and _same_bits(o[2], o2[2])


@pytest.mark.parametrize("n_mid", [0, 1, 2, 3])
def test_fused_operand_packers_exact(n_mid):
    """ops.fused_operands(_deep): the column gather with -1 structural zeros, h_scale and the A fragments, bit for bit"""
    from matten_amd import ops

    cols, ent, n_tiles, w_pad = rc.pack_plan()
    nb, W, n_cols = rc.PACK_NB, rc.PACK_W, rc.PACK_N_COLS
    nb_pad = (nb + 3) // 4 * 4
    g = torch.Generator().manual_seed(600 + n_mid)
    gain = 1e3 if n_mid == 2 else 1.0       # (one depth with h_scale < 1: 1 / s folded into the fragments' scales)
    w0 = (torch.randn(nb, 32, generator=g) * gain).to(DEV)
    wm = (torch.randn(n_mid, 32, 32, generator=g) * gain).to(DEV)
    w2 = torch.randn(32, W, generator=g).to(DEV)
    c = rc.act_cst()
    sc = (1.0 / nb**0.5, c / 32**0.5, c / 32**0.5)
    r_start, r_end = 0.5, 4.0
    run = lambda: ops.fused_operands_deep(w0, wm, w2, sc, cols.to(DEV), ent.to(DEV), n_tiles, r_start, r_end, c)
    a, b = run(), run()
    torch.cuda.synchronize()
    assert all(_same_bits(x, y) for x, y in zip(a, b)), "a second call differs"
    w0p, wmp, w2p, hs, frag, inv = a
    s0, s1, s2 = (torch.tensor(s, dtype=torch.float32, device=DEV) for s in sc)
    want0 = torch.zeros(nb_pad, 32, device=DEV)
    want0[:nb] = w0 * s0
    want2 = torch.zeros(32, w_pad, device=DEV)
    live = torch.nonzero(cols >= 0).flatten().to(DEV)
    want2[:, live] = w2[:, cols.to(DEV)[live]] * s2
    assert w0p.shape == want0.shape and torch.equal(w0p, want0)
    assert wmp.shape == (n_mid, 32, 32) and torch.equal(wmp, wm * s1)
    assert w2p.shape == want2.shape and torch.equal(w2p, want2)
    assert (w2p[:, n_cols:] == 0).all() and (w2p[:, torch.nonzero(cols < 0).flatten().to(DEV)] == 0).all()
    want_hs = ops.radial_h_scale_deep(w0, wm, r_start, r_end, c)
    assert torch.equal(hs, want_hs) and 0.0 < float(hs[0]) <= 1.0 and float(hs[1]) == 1.0 / float(hs[0])
    assert gain == 1 or float(hs[0]) < 1.0
    want_frag, want_inv = ops.split_a_tiles(w2p, ent.numpy())
    assert frag.shape == want_frag.shape == (n_tiles, 64, 16) and _same_bits(frag, want_frag)
    assert _same_bits(inv, want_inv * hs[1])
    if n_mid == 1:
        o = ops.fused_operands(w0, wm[0], w2, sc, cols.to(DEV), ent.to(DEV), n_tiles, r_start, r_end, c)
        assert _same_bits(o[1], wmp[0]) and all(_same_bits(x, y) for x, y in zip(o[:1] + o[2:], a[:1] + a[2:]))


def test_zz_worst_ratios():
    """the figures of the module docstring: worst error / allowed per quantity and form over this session's tests"""
    print()
    for (key, form), r in sorted(WORST.items()):
        print(f"RADIAL worst {key:14s} {form:14s} {r:.3g}")
