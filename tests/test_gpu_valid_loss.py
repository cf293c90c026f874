"""The valid-loss kernels (matten_valid_loss / matten_valid_loss_bwd, csrc/loss.hip) against the numpy fp64 restatement
``ops.valid_loss_host`` and, bit for bit, against the selected-loss entry with selector[row] = (row < n_valid).

Tolerances: every term is an fp32 difference (exact in fp64), squared or taken absolute in fp64; fewer than 2^19 additions at
unit roundoff 2^-53 bound the relative error of a sum by about 6e-11, so 1e-10.  ``count`` is exact.  ``loss`` and every
gradient element are one fp64 expression rounded once to fp32: within one fp32 ulp of the host's."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _lib_sizes():
    from matten_amd import _lib

    lib = _lib.load()
    return lib.matten_selected_loss_tile_elems(), lib.matten_selected_loss_max_blocks()


def _shapes():
    tile, cap = _lib_sizes()
    return [(1, 1), (1, 21), (33, 21), (34, 6),                     # edge cases
            (tile - 1, 1), (tile, 1), (tile + 1, 1),                # one workgroup / the second one and the combine kernel
            (2 * tile * cap + 17, 1)]                               # several strided rounds and a ragged last one


def _n_valids(n_rows):
    return [0, 1, n_rows - 1, n_rows, n_rows + 5, -3]              # the last two are clamped


@functools.lru_cache(maxsize=None)
def _inputs(n_rows, d):
    """(pred, target) on the host and on the device, built once per shape and never written"""
    g = torch.Generator().manual_seed(1000 * d + n_rows % 997)
    pred = torch.randn(n_rows, d, generator=g)
    target = torch.randn(n_rows, d, generator=g)
    pred[0, 0] = target[0, 0]                                       # one zero difference: sign(0) = 0
    return pred, target, pred.to(DEV), target.to(DEV)


def _word(k):
    """the crystal word of a padded batch's count words, as the model slices it"""
    return torch.tensor([7, 11, k], dtype=torch.int64, device=DEV)[2:3]


def _one_ulp(got, want, what):
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    assert (err <= np.spacing(np.abs(want)).astype(np.float64)).all(), (what, float(err.max()))


def test_the_shapes_cover_the_paths():
    from matten_amd import _lib

    tile, cap = _lib_sizes()
    q = _lib.load().matten_valid_loss_workspace_bytes
    assert q(tile, 1) == 0 and q(tile + 1, 1) == 2 * 24 and q(2 * tile * cap + 17, 1) == cap * 24
    assert 2 * tile * cap + 17 < 2 ** 19                            # the additions the tolerance counts on


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("shape", range(8))
def test_valid_loss_against_the_host_and_the_selected_entry(shape, kind):
    from matten_amd import ops

    n_rows, d = _shapes()[shape]
    pred, target, p, t = _inputs(n_rows, d)
    g = torch.tensor(0.75, device=DEV)
    rows = torch.arange(n_rows, device=DEV)
    for n_valid in _n_valids(n_rows):
        k = min(max(n_valid, 0), n_rows)
        word = _word(n_valid)
        loss, sums, count = ops.valid_loss(p, t, word, kind)
        grad = ops.valid_loss_bwd(p, t, word, kind, g, count)
        assert loss.dtype == torch.float32 and sums.dtype == torch.float64 and count.dtype == torch.int64
        assert loss.shape == () and sums.shape == (2,) and count.shape == () and grad.shape == p.shape
        want_loss, want_sums, want_count = ops.valid_loss_host(pred.numpy(), target.numpy(), n_valid, kind)
        want_grad = ops.valid_loss_bwd_host(pred.numpy(), target.numpy(), n_valid, kind, g=0.75)
        rel = np.abs(sums.cpu().numpy() - want_sums) / np.maximum(np.abs(want_sums), 1e-300)
        print(f"[{n_rows},{d}] kind {kind} n_valid {n_valid}: sums rel err {rel}, loss {float(loss)} (host {float(want_loss)})")
        assert int(count) == want_count == k
        assert (rel <= 1e-10).all() if k else not sums.any()
        _one_ulp(loss.cpu().numpy(), want_loss, "loss")
        _one_ulp(grad.cpu().numpy(), want_grad, "grad")
        assert (grad[k:].view(torch.int32) == 0).all()              # +0.0, by the sign bit
        if k == 0:
            assert float(loss) == 0.0 and (grad.view(torch.int32) == 0).all()
        elif kind == 1 and d * n_rows > 1:
            assert float(grad[0, 0]) == 0.0                         # sign(0) = 0
        # reproducible
        again = ops.valid_loss(p, t, word, kind)
        assert all(torch.equal(a, b) for a, b in zip(again, (loss, sums, count)))
        assert torch.equal(ops.valid_loss_bwd(p, t, word, kind, g, count), grad)
        # what the padding rows hold changes no bit
        junk_p, junk_t = p.clone(), t.clone()
        junk_p[k:] = float("nan")
        junk_t[k:] = float("inf")
        j_loss, j_sums, j_count = ops.valid_loss(junk_p, junk_t, word, kind)
        assert torch.equal(j_loss, loss) and torch.equal(j_sums, sums) and torch.equal(j_count, count)
        assert torch.equal(ops.valid_loss_bwd(junk_p, junk_t, word, kind, g, count).view(torch.int32), grad.view(torch.int32))
        # the selector route with selector[row] = (row < k): the same bits, for both kinds
        selector = (rows < k).to(torch.int32)
        for kd in (0, 1):
            s_loss, s_sum, s_count = ops.selected_loss(p, t, selector, kd)
            v_loss, v_sums, v_count = (loss, sums, count) if kd == kind else ops.valid_loss(p, t, word, kd)
            assert torch.equal(v_sums, sums)                        # both sums whatever the kind
            assert torch.equal(s_sum, v_sums[kd]) and torch.equal(s_count, v_count) and torch.equal(s_loss, v_loss), kd
        assert torch.equal(ops.selected_loss_bwd(p, t, selector, kind, g, count), grad)


def test_no_rows_and_no_valid_rows():
    from matten_amd import ops

    empty = torch.empty(0, 6, device=DEV)
    for kind in (0, 1):
        loss, sums, count = ops.valid_loss(empty, empty, _word(3), kind)
        assert float(loss) == 0.0 and sums.tolist() == [0.0, 0.0] and int(count) == 0
        assert ops.valid_loss_bwd(empty, empty, _word(3), kind, torch.ones((), device=DEV), count).shape == (0, 6)
    pred = torch.randn(9, 6, device=DEV)
    loss, sums, count = ops.valid_loss(pred, pred + 1.0, _word(0), 0)
    assert float(loss) == 0.0 and sums.tolist() == [0.0, 0.0] and int(count) == 0


def test_autograd_function_and_valid_mean_loss():
    from matten_amd import ops
    from matten_amd.autograd import ValidLossFn
    from matten_amd.graphs import valid_mean_loss

    pred_cpu, target_cpu, _, t = _inputs(34, 6)
    pred = pred_cpu.to(DEV).requires_grad_(True)
    loss, sums, count = ValidLossFn.apply(pred, t, _word(20), 0)
    assert not sums.requires_grad and not count.requires_grad
    (0.5 * loss).backward()
    _one_ulp(pred.grad.cpu().numpy(), ops.valid_loss_bwd_host(pred_cpu.numpy(), target_cpu.numpy(), 20, 0, g=0.5), "grad")
    batch = {"_amd_n_valid": torch.tensor([0, 0, 20], dtype=torch.int64, device=DEV)}
    for kind in ("mse", "mae"):
        fn = valid_mean_loss(kind, key="y")
        got = fn({"y": pred}, t, batch)
        assert torch.equal(got, ops.valid_loss(pred.detach(), t, _word(20), kind)[0])
    # the trailing dimensions are flattened
    a = ops.valid_loss(pred.detach().reshape(34, 2, 3), t.reshape(34, 2, 3), _word(20), 1)
    assert all(torch.equal(x, y) for x, y in zip(a, ops.valid_loss(pred.detach(), t, _word(20), 1)))


def test_captured_loss_follows_the_refreshed_word():
    """forward and backward in one hipGraph; the replay reads the count word and the rows of the moment"""
    from matten_amd import ops
    from matten_amd.autograd import ValidLossFn

    tile, _ = _lib_sizes()
    pred_cpu, target_cpu, p, t = _inputs(tile + 1, 1)
    words = torch.tensor([0, 0, 5], dtype=torch.int64, device=DEV)
    pred = p.clone().requires_grad_(True)
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        ValidLossFn.apply(pred, t, words[2:3], 0)[0].backward()
    torch.cuda.current_stream(DEV).wait_stream(side)
    torch.cuda.synchronize()
    pred.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss, sums, count = ValidLossFn.apply(pred, t, words[2:3], 0)
        loss.backward()
    for k in (tile + 1, 7, 0):
        words[2] = k
        graph.replay()
        want = ops.valid_loss(p, t, _word(k), 0)
        assert torch.equal(loss, want[0]) and torch.equal(sums, want[1]) and int(count) == k
        assert torch.equal(pred.grad, ops.valid_loss_bwd(p, t, _word(k), 0, torch.ones((), device=DEV), want[2]))
