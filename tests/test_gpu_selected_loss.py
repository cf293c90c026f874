"""The selected-loss kernels (matten_selected_loss / matten_selected_loss_bwd, csrc/loss.hip) against the fp64 restatement
of tests/test_atom_targets_host.py: every shape at which the forward takes another path (one workgroup, several, the
strided loop above the workgroup cap), both kinds, four selector densities; junk in unselected rows, NaN in a selected
one, an empty selection, determinism, the upstream gradient, and a captured forward + backward replayed on new contents."""
import pytest
import torch

from test_atom_targets_host import selected_loss_bwd_ref, selected_loss_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS32 = 2.0 ** -23
MAX_ELEMS = 200_000      # keeps n * 2^-53 below the 1e-10 bound on `sum`
ROWS = ("1", "63", "64", "65", "wg-1", "wg", "wg+1", "many", "strided")
DENSITIES = ("sparse", "all", "one", "none")


def _n_rows(label, d):
    """row counts from the kernel's own constants: `wg` = the rows one workgroup takes in a round, `many` = more than 64
    workgroups with a ragged tail, `strided` = more elements than the workgroup cap covers in one round"""
    from matten_amd import _lib

    lib = _lib.load()
    tile, cap = lib.matten_selected_loss_tile_elems(), lib.matten_selected_loss_max_blocks()
    assert cap > 65
    n = {"wg-1": tile // d - 1, "wg": tile // d, "wg+1": tile // d + 1, "many": (65 * tile) // d + 3,
         "strided": (cap * tile) // d + 5}.get(label)
    n = int(label) if n is None else n
    if label == "many":
        assert 65 * tile < n * d <= cap * tile and (n * d) % tile != 0
    if label == "strided":
        assert n * d > cap * tile and (n * d) % tile != 0
    assert 1 <= n and n * d <= MAX_ELEMS
    return n


def _selector(n, density, gen):
    if density == "sparse":          # about 15 %, as in the NMR set
        return (torch.rand(n, generator=gen) < 0.15).to(torch.int32) * 7     # any nonzero value selects
    if density == "all":
        return torch.ones(n, dtype=torch.int32)
    sel = torch.zeros(n, dtype=torch.int32)
    if density == "one":
        sel[int(torch.randint(n, (1,), generator=gen))] = -1
    return sel


def _inputs(n, d, density, seed):
    gen = torch.Generator().manual_seed(seed)
    pred = torch.randn(n, d, generator=gen)
    target = torch.randn(n, d, generator=gen)
    if n > 3:
        target[:3, 0] = pred[:3, 0]  # exact zeros of the difference: sign(0) = 0
    return pred, target, _selector(n, density, gen)


def _is_plus_zero(t):
    return bool((t.contiguous().view(torch.int32) == 0).all())


def _check(pred, target, sel, kind, g=None):
    from matten_amd import ops

    p, t, s = pred.to(DEV), target.to(DEV), sel.to(DEV)
    loss, total, count = ops.selected_loss(p, t, s, kind)
    assert loss.dtype == torch.float32 and total.dtype == torch.float64 and count.dtype == torch.int64
    assert loss.shape == total.shape == count.shape == ()
    up = torch.ones((), device=DEV) if g is None else torch.tensor(float(g), device=DEV)
    grad = ops.selected_loss_bwd(p, t, s, kind, up, count)
    assert grad.shape == pred.shape and grad.dtype == torch.float32
    want_loss, want_total, want_count = selected_loss_ref(pred, target, sel, kind)
    want_grad = selected_loss_bwd_ref(pred, target, sel, kind, 1.0 if g is None else g)
    assert int(count) == want_count
    assert abs(float(total) - float(want_total)) <= 1e-10 * abs(float(want_total))
    assert abs(float(loss.double()) - float(want_loss)) <= EPS32 * abs(float(want_loss))
    got = grad.cpu().double()
    assert bool(((got - want_grad).abs() <= EPS32 * want_grad.abs()).all())
    assert _is_plus_zero(grad[s == 0])
    return loss, total, count, grad


@pytest.mark.parametrize("d", [1, 6, 9, 21])
@pytest.mark.parametrize("rows", ROWS)
def test_loss_and_adjoint_against_fp64(rows, d):
    n = _n_rows(rows, d)
    for kind in (0, 1):
        for i, density in enumerate(DENSITIES):
            pred, target, sel = _inputs(n, d, density, seed=1000 * d + 10 * i + kind)
            loss, total, count, grad = _check(pred, target, sel, kind)
            if density == "none":
                assert float(loss) == 0.0 and float(total) == 0.0 and int(count) == 0 and _is_plus_zero(grad)
            if density == "all":
                assert int(count) == n and float(loss) > 0.0


@pytest.mark.parametrize("kind", [0, 1])
def test_junk_in_unselected_rows_changes_no_bit(kind):
    from matten_amd import ops

    n, d = _n_rows("many", 6), 6
    pred, target, sel = _inputs(n, d, "sparse", seed=5)
    off = torch.nonzero(sel == 0).flatten()
    junk_p, junk_t = pred.clone(), target.clone()
    junk_p[off[0::3]] = float("nan")
    junk_p[off[1::3]] = float("inf")
    junk_t[off[1::3]] = float("inf")            # inf - inf
    junk_t[off[2::3]] = float("-inf")
    junk_t[off[0::5]] = float("nan")
    clean = _check(pred, target, sel, kind)
    s = sel.to(DEV)
    loss, total, count = ops.selected_loss(junk_p.to(DEV), junk_t.to(DEV), s, kind)
    grad = ops.selected_loss_bwd(junk_p.to(DEV), junk_t.to(DEV), s, kind, torch.ones((), device=DEV), count)
    for got, want in zip((loss, total, count, grad), clean):
        assert torch.equal(got, want)
    assert _is_plus_zero(grad[s == 0])


@pytest.mark.parametrize("kind", [0, 1])
def test_nan_in_a_selected_row_reaches_the_loss(kind):
    from matten_amd import ops

    n, d = _n_rows("wg+1", 6), 6
    pred, target, sel = _inputs(n, d, "sparse", seed=6)
    row = int(torch.nonzero(sel).flatten()[-1])
    pred[row, 2] = float("nan")
    loss, total, count = ops.selected_loss(pred.to(DEV), target.to(DEV), sel.to(DEV), kind)
    assert torch.isnan(loss) and torch.isnan(total) and int(count) == int((sel != 0).sum())


def test_empty_row_set_and_empty_selection():
    from matten_amd import ops

    loss, total, count = ops.selected_loss(torch.empty(0, 6, device=DEV), torch.empty(0, 6, device=DEV),
                                           torch.empty(0, dtype=torch.int32, device=DEV), 0)
    assert float(loss) == 0.0 and float(total) == 0.0 and int(count) == 0
    pred = torch.full((70, 6), float("nan"), device=DEV)
    sel = torch.zeros(70, dtype=torch.int32, device=DEV)
    loss, total, count = ops.selected_loss(pred, pred, sel, 1)
    grad = ops.selected_loss_bwd(pred, pred, sel, 1, torch.ones((), device=DEV), count)
    assert float(loss) == 0.0 and _is_plus_zero(loss) and float(total) == 0.0 and int(count) == 0 and _is_plus_zero(grad)


@pytest.mark.parametrize("rows", ["65", "many", "strided"])
def test_two_calls_give_the_same_bits(rows):
    from matten_amd import ops

    n, d = _n_rows(rows, 9), 9
    pred, target, sel = (x.to(DEV) for x in _inputs(n, d, "sparse", seed=8))
    a = ops.selected_loss(pred, target, sel, 0)
    junk = torch.randn(1 << 16, device=DEV)      # other work in between: the partials' slots are reused or not
    b = ops.selected_loss(pred, target, sel, 0)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and junk.numel() > 0
    one = torch.ones((), device=DEV)
    assert torch.equal(ops.selected_loss_bwd(pred, target, sel, 0, one, a[2]), ops.selected_loss_bwd(pred, target, sel, 0, one, b[2]))


@pytest.mark.parametrize("kind", [0, 1])
def test_adjoint_follows_the_upstream_gradient(kind):
    pred, target, sel = _inputs(130, 6, "sparse", seed=9)
    _check(pred, target, sel, kind, g=0.5)
    *_, grad = _check(pred, target, sel, kind, g=0.0)
    assert bool((grad == 0).all())


def test_autograd_function_flattens_and_differentiates_pred_only():
    from matten_amd.autograd import SelectedLossFn

    gen = torch.Generator().manual_seed(10)
    wide = torch.randn(90, 3, 6, generator=gen)
    pred_cpu = wide[:, :, :3]                                      # [90, 3, 3], not contiguous
    target_cpu, sel = torch.randn(90, 3, 3, generator=gen), _selector(90, "sparse", gen)
    pred = wide.to(DEV)[:, :, :3].requires_grad_(True)
    target = target_cpu.to(DEV).requires_grad_(True)
    assert not pred.is_contiguous()
    loss, count, total = SelectedLossFn.apply(pred, target, sel.to(DEV), 0)
    assert loss.requires_grad and not count.requires_grad and not total.requires_grad
    (0.5 * loss).backward()
    assert target.grad is None and pred.grad.shape == (90, 3, 3)
    want = selected_loss_bwd_ref(pred_cpu, target_cpu, sel, 0, 0.5)
    assert bool(((pred.grad.cpu().double() - want).abs() <= EPS32 * want.abs()).all())
    want_loss, want_total, want_count = selected_loss_ref(pred_cpu, target_cpu, sel, 0)
    assert int(count) == want_count and abs(float(loss.detach()) - float(want_loss)) <= EPS32 * float(want_loss)


@pytest.mark.parametrize("rows", ["wg", "many"])
def test_captured_forward_and_backward_follow_the_buffers(rows):
    """captured once, replayed after selector and pred were overwritten: the bits of the eager call on the new contents"""
    from matten_amd.autograd import SelectedLossFn

    n, d = _n_rows(rows, 6), 6
    pred0, target, sel0 = (x.to(DEV) for x in _inputs(n, d, "sparse", seed=11))
    pred1, _, sel1 = (x.to(DEV) for x in _inputs(n, d, "sparse", seed=12))
    assert not torch.equal(sel0, sel1)
    pred_buf, sel_buf = pred0.clone().requires_grad_(True), sel0.clone()

    def run(p, s):
        loss, count, total = SelectedLossFn.apply(p, target, s, 0)
        (grad,) = torch.autograd.grad(loss, p)
        return loss, count, total, grad

    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        run(pred_buf, sel_buf)
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize(DEV)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = run(pred_buf, sel_buf)
    for p_new, s_new in ((pred0, sel0), (pred1, sel1), (pred1, torch.zeros_like(sel1))):
        with torch.no_grad():
            pred_buf.copy_(p_new)
            sel_buf.copy_(s_new)
        graph.replay()
        torch.cuda.synchronize(DEV)
        eager = run(p_new.clone().requires_grad_(True), s_new)
        for got, want in zip(captured, eager):
            assert torch.equal(got, want)
    assert int(captured[1]) == 0 and float(captured[0]) == 0.0
