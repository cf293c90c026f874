"""
The polycrystal moduli on the GPU (matten_amd/elastic.py over csrc/polycrystal.hip) against the numpy statement of the
algorithm, ``polycrystal_host`` / ``polycrystal_bwd_host`` (tested in tests/test_polycrystal_host.py), on the one batch of 257
rows of tests/polycrystal_cases.py: more than one workgroup, not a multiple of the wave; the isotropic tensor, both cubic
cases, a hexagonal tensor, 250 seeded triclinic tensors, a near-singular row, a row that is not positive definite, a NaN row.

Tolerances.  The reference is the host function, never the kernel; the bound is ten times the largest relative distance
the host function itself moves on this batch (floor 1e-12)
  * between sc_tol = 1e-12 and 1e-15:            k_sc / g_sc 1.6e-12
  * between hs_grid = 64 and a 20 001-point scan: the four bounds 1.8e-11
so TOL = 1.8e-10, relative, for every forward quantity.  The adjoint, same rule: ``polycrystal_bwd_host`` moves by 1.3e-12 of
a row's largest entry between sc_tol = 1e-12 and 1e-15, so TOL_BWD = 1.3e-11 of the row's largest entry.  (Measured with
numpy on the CPU; the kernel evaluates F from the Kelvin decomposition, the host by its definition with a 6x6 inverse.)
"""
import warnings

import numpy as np
import pytest
import torch

import polycrystal_cases as pc
from common import LMAX2

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = 1.8e-10
TOL_BWD = 1.3e-11
NAMES6 = ("k_hs_lower", "g_hs_lower", "k_sc", "g_sc", "k_hs_upper", "g_hs_upper")
BAD = [pc.ROW_NOT_PD, pc.ROW_NAN]


def _np(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def batch():
    """the batch through ``elastic_properties(polycrystal=True)`` once, the kernel's own inputs and outputs through ``ops``,
    and the host statement of what the kernel was given (its ``voigt`` and ``flags``): shared, never written to"""
    from matten_amd import elastic, ops

    C = pc.batch()
    props = elastic.elastic_properties(C, polycrystal=True)
    voigt, flags = props.voigt, props.flags
    moduli, vectors, _ = ops.elastic_kelvin(voigt, flags, want_dilatation=False)
    out, media, status = ops.elastic_polycrystal(voigt, flags, moduli, vectors)
    ref = elastic.polycrystal_host(_np(voigt), flags=_np(flags))
    good = np.ones(pc.N_BATCH, dtype=bool)
    good[BAD] = False
    return dict(C=C, props=props, voigt=voigt, flags=flags, moduli=moduli, vectors=vectors, out=out, media=media,
                status=status, ref=ref, good=good)


def test_forward_against_polycrystal_host(batch):
    """Every forward field within TOL of the host statement on the good rows, NaN and the documented statuses on the bad
    ones.  Measured on one MI355X: k_hs_lower 5.5e-11, g_hs_lower 4.4e-11, k_sc 3.6e-15, g_sc 1.3e-15, k_hs_upper 6.7e-15,
    g_hs_upper 1.8e-15, y_sc 2.7e-15, poisson_sc 6.3e-13."""
    from matten_amd import elastic

    p, ref, good = batch["props"], batch["ref"], batch["good"]
    assert list(ref["sc_status"][BAD]) == [2, -1] and (ref["sc_status"][good] == 0).all()
    worst = {}
    for name in NAMES6 + ("y_sc", "poisson_sc"):
        got = _np(getattr(p, name))
        assert got.shape == (pc.N_BATCH,) and got.dtype == np.float64
        worst[name] = np.abs(got[good] / ref[name][good] - 1.0).max()
        assert np.isnan(got[BAD]).all(), name
    print("device against host, largest relative distance: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    for name, w in worst.items():
        assert w <= TOL, (name, w)
    assert np.array_equal(_np(p.sc_status), ref["sc_status"]) and _np(p.sc_status).dtype == np.int32
    it = _np(p.sc_iterations)
    assert (np.abs(it - ref["sc_iterations"]) <= 1).all() and (it[BAD] == 0).all() and (it[good] >= 1).all()
    # the fields are the kernel's columns, and the Kelvin fields do not appear unasked
    assert np.array_equal(_np(p.k_sc), _np(batch["out"])[:, 2], equal_nan=True)
    assert np.array_equal(_np(p.g_hs_upper), _np(batch["out"])[:, 5], equal_nan=True)
    assert np.array_equal(_np(p.hs_media).reshape(-1, 8), _np(batch["media"]), equal_nan=True)
    assert not hasattr(p, "kelvin_moduli")
    # the media: feasible, and F there (by the host's definition) is the bound that was reported -- where the frontier is
    # flat the medium itself is not unique, so it is not compared
    media = _np(p.hs_media)
    assert media.shape == (pc.N_BATCH, 4, 2) and np.isnan(media[BAD]).all() and (media[good] > 0).all()
    Ch = elastic.MANDEL_WEIGHT * _np(batch["voigt"])[good]
    lam = np.linalg.eigvalsh(Ch)
    for q, (name, sign) in enumerate((("k_hs_lower", 1.0), ("g_hs_lower", 1.0), ("k_hs_upper", -1.0), ("g_hs_upper", -1.0))):
        K0, G0 = media[good, q, 0], media[good, q, 1]
        gap = np.linalg.eigvalsh(sign * (Ch - elastic.iso_mandel(K0, G0)))[:, 0]
        assert (gap >= -1e-9 * lam[:, 5]).all(), name
        f = elastic.polycrystal_F(Ch, K0, G0)[q % 2]
        assert np.abs(f / _np(getattr(p, name))[good] - 1.0).max() <= TOL, name
    # the closed forms
    K, m1, m2, g1, g2, g_sc = pc.cubic_closed_forms(*pc.COPPER)
    assert abs(_np(p.g_sc)[pc.ROW_CUBIC] / g_sc - 1.0) <= 1e-10 and abs(_np(p.g_hs_lower)[pc.ROW_CUBIC] / g1 - 1.0) <= 1e-10
    for name in NAMES6:
        assert abs(_np(getattr(p, name))[pc.ROW_ISOTROPIC] / (160.0 if name[0] == "k" else 80.0) - 1.0) <= 1e-12, name
    # the ordering chain
    slack = 1.0 + 1e-12
    for lo, hsl, sc, hsu, hi in ((p.k_reuss, p.k_hs_lower, p.k_sc, p.k_hs_upper, p.k_voigt),
                                 (p.g_reuss, p.g_hs_lower, p.g_sc, p.g_hs_upper, p.g_voigt)):
        lo, hsl, sc, hsu, hi = (_np(t)[good] for t in (lo, hsl, sc, hsu, hi))
        assert (lo <= hsl * slack).all() and (hsl <= sc * slack).all() and (sc <= hsu * slack).all() and (hsu <= hi * slack).all()


def test_iteration_cap_and_grid_size(batch):
    from matten_amd import elastic, ops

    args = (batch["voigt"], batch["flags"], batch["moduli"], batch["vectors"])
    out, _, status = ops.elastic_polycrystal(*args, hs_grid=2, sc_max_iter=2)
    st = _np(status)
    assert list(st[BAD, 0]) == [2, -1] and (st[batch["good"], 1] <= 2).all() and (st[batch["good"], 0] == 1).sum() > 200
    ref = elastic.polycrystal_host(_np(batch["voigt"]), hs_grid=2, sc_max_iter=2, flags=_np(batch["flags"]))
    assert np.array_equal(st[:, 0], ref["sc_status"])
    for q, name in enumerate(NAMES6):
        assert np.abs(_np(out)[batch["good"], q] / ref[name][batch["good"]] - 1.0).max() <= TOL, name
    # a coarse grid is still a bound, only a looser one
    full = _np(batch["out"])[batch["good"]]
    coarse = _np(out)[batch["good"]]
    assert (coarse[:, :2] <= full[:, :2] * (1.0 + 1e-12)).all() and (coarse[:, 4:] >= full[:, 4:] * (1.0 - 1e-12)).all()


def test_empty_and_single_row(batch):
    from matten_amd import elastic, ops

    e64 = torch.empty(0, 6, 6, dtype=torch.float64, device=DEV)
    out, media, status = ops.elastic_polycrystal(e64, torch.empty(0, dtype=torch.int32, device=DEV),
                                                 torch.empty(0, 6, dtype=torch.float64, device=DEV), e64)
    assert out.shape == (0, 6) and media.shape == (0, 8) and status.shape == (0, 2)
    g = ops.elastic_polycrystal_bwd(e64, torch.empty(0, dtype=torch.int32, device=DEV), out, status,
                                    torch.empty(0, 2, dtype=torch.float64, device=DEV))
    assert g.shape == (0, 6, 6)
    one = elastic.elastic_properties(batch["C"][pc.ROW_HEXAGONAL], polycrystal=True)
    assert one.k_sc.shape == () and one.hs_media.shape == (4, 2) and one.sc_status.shape == ()
    for name in elastic.POLYCRYSTAL_FIELDS:
        assert torch.equal(getattr(one, name), getattr(batch["props"], name)[pc.ROW_HEXAGONAL]), name


def test_bits_repeat_and_do_not_depend_on_the_batch(batch):
    from matten_amd import ops

    args = (batch["voigt"], batch["flags"], batch["moduli"], batch["vectors"])
    again = ops.elastic_polycrystal(*args)
    for a, b in zip(again, (batch["out"], batch["media"], batch["status"])):
        assert np.array_equal(_np(a), _np(b), equal_nan=True)
    perm = torch.from_numpy(np.random.default_rng(0).permutation(pc.N_BATCH)).to(DEV)
    shuffled = ops.elastic_polycrystal(*(t[perm].contiguous() for t in args))
    for a, b in zip(shuffled, (batch["out"], batch["media"], batch["status"])):
        assert np.array_equal(_np(a), _np(b[perm]), equal_nan=True)
    lean, none, status = ops.elastic_polycrystal(*args, want_media=False)
    assert none is None and np.array_equal(_np(lean), _np(batch["out"]), equal_nan=True)
    assert torch.equal(status, batch["status"])


def test_adjoint_against_polycrystal_bwd_host(batch):
    """within TOL_BWD of a row's largest entry; measured on one MI355X: 4.2e-15"""
    from matten_amd import elastic, ops

    good = batch["good"]
    g = np.random.default_rng(4).standard_normal((pc.N_BATCH, 2))
    got = ops.elastic_polycrystal_bwd(batch["voigt"], batch["flags"], batch["out"], batch["status"], torch.from_numpy(g).to(DEV))
    again = ops.elastic_polycrystal_bwd(batch["voigt"], batch["flags"], batch["out"], batch["status"], torch.from_numpy(g).to(DEV))
    assert torch.equal(got, again)
    got = _np(got)
    want = elastic.polycrystal_bwd_host(_np(batch["voigt"]), g, flags=_np(batch["flags"]))
    assert got.shape == (pc.N_BATCH, 6, 6) and np.array_equal(got, got.transpose(0, 2, 1))
    assert (got[BAD] == 0.0).all() and (want[BAD] == 0.0).all()
    err = np.abs(got - want).max(axis=(1, 2))[good] / np.abs(want).max(axis=(1, 2))[good]
    print(f"adjoint against host: {err.max():.2e} of the row's largest entry (row {int(np.nonzero(good)[0][err.argmax()])})")
    assert (err <= TOL_BWD).all()
    # a NaN gradient into a row without a value still leaves exact zeros
    g_nan = torch.full((pc.N_BATCH, 2), float("nan"), dtype=torch.float64, device=DEV)
    z = _np(ops.elastic_polycrystal_bwd(batch["voigt"], batch["flags"], batch["out"], batch["status"], g_nan))
    assert (z[BAD] == 0.0).all()


def _irreps_rows():
    """x [8,21] fp32 whose tensors are the first eight rows of the batch (isotropic, cubic x 2, hexagonal, 4 triclinic)"""
    from matten_amd import elastic

    V = elastic.voigt_basis()
    return torch.from_numpy(pc.batch()[:8].reshape(8, 36) @ np.linalg.pinv(V)).float()


def test_moduli_loss_backward_to_the_irreps_rows():
    """``elastic_moduli_from_irreps(x, polycrystal=True)`` -> ``ModuliLoss(("k_sc", "g_sc"))`` -> backward to x [8,21], against
    fp64 central differences of the host path (``polycrystal_host``'s fixed point on x @ voigt_basis, sc_tol = 1e-15) on the
    widened x.  The targets sit 10 % off the values, away from the kink of the L1 loss.  The device differs from that by
    the fp32 rounding of the two dense_rows products (forward [8,36], adjoint [8,21]): 21- and 36-term sums at 2^-24 per
    term, carried through a fixed point whose sensitivity is bounded by the tensors' condition numbers (< 100 on these
    rows): 36 * 2^-24 * 100 = 2e-4 of the largest gradient entry is the bound; the central differences (step 1e-6 max|x|)
    are good to 1e-8.  Measured on one MI355X: the gradient 3.1e-7, the loss 2.3e-8."""
    from matten_amd import elastic

    x = _irreps_rows()
    V32 = torch.from_numpy(elastic.voigt_basis().copy()).float().double().numpy()
    x64 = x.double().numpy()
    rows0 = elastic._polycrystal_rows((x64 @ V32).reshape(8, 6, 6), None)
    K0, G0, _, _ = elastic._sc_iterate(rows0[0], rows0[1], rows0[2], 1e-15, 2000)
    targets = {"k_sc": torch.from_numpy(0.9 * K0), "g_sc": torch.from_numpy(1.1 * G0)}

    def host_loss(xv):
        rows = elastic._polycrystal_rows((xv @ V32).reshape(8, 6, 6), None)
        K, G, _, _ = elastic._sc_iterate(rows[0], rows[1], rows[2], 1e-15, 2000)
        return (np.abs(K - 0.9 * K0).sum() + np.abs(G - 1.1 * G0).sum()) / 16.0

    h = 1e-6 * np.abs(x64).max()
    want = np.zeros((8, 21))
    for b in range(8):
        for c in range(21):
            xp, xm = x64.copy(), x64.copy()
            xp[b, c] += h
            xm[b, c] -= h
            want[b, c] = (host_loss(xp) - host_loss(xm)) / (2.0 * h)

    xd = x.to(DEV).requires_grad_()
    props = elastic.elastic_moduli_from_irreps(xd, polycrystal=True)
    loss = elastic.ModuliLoss(("k_sc", "g_sc"))(props, {k: v.to(DEV) for k, v in targets.items()})
    loss.backward()
    assert props.k_sc.requires_grad and props.g_sc.requires_grad and props.y_sc.requires_grad and props.poisson_sc.requires_grad
    for name in ("k_hs_lower", "g_hs_lower", "k_hs_upper", "g_hs_upper", "hs_media", "sc_status", "sc_iterations"):
        assert not getattr(props, name).requires_grad, name
    assert xd.grad.dtype == torch.float32 and (props.sc_status == 0).all()
    err = np.abs(_np(xd.grad).astype(np.float64) - want).max() / np.abs(want).max()
    print(f"loss {loss.item():.12e} against {host_loss(x64):.12e}; gradient off by {err:.2e} of its largest entry")
    assert abs(loss.item() / host_loss(x64) - 1.0) <= 2e-4 and err <= 2e-4
    # y_sc and poisson_sc train too, and the same bits come out of the route without gradient
    x2 = x.to(DEV).requires_grad_()
    p2 = elastic.elastic_moduli_from_irreps(x2, polycrystal=True, kelvin=True)
    elastic.ModuliLoss(("y_sc", "poisson_sc"))(p2, {"y_sc": torch.zeros(8), "poisson_sc": torch.zeros(8)}).backward()
    assert torch.isfinite(x2.grad).all() and x2.grad.abs().max() > 0 and p2.kelvin_moduli.requires_grad
    plain = elastic.elastic_properties_from_irreps(x.to(DEV), polycrystal=True)
    for name in elastic.POLYCRYSTAL_FIELDS:
        assert torch.equal(getattr(plain, name), getattr(props, name).detach()), name
        assert torch.equal(getattr(plain, name), getattr(p2, name).detach()), name
    with pytest.raises(ValueError, match="polycrystal=True"):
        elastic.ModuliLoss(("k_sc",))(elastic.elastic_moduli_from_irreps(x.to(DEV)), {"k_sc": torch.zeros(8)})


def test_forward_and_backward_replay_as_a_graph():
    from matten_amd import elastic

    x = _irreps_rows().to(DEV)
    targets = {"k_sc": torch.full((8,), 100.0, device=DEV), "g_sc": torch.full((8,), 50.0, device=DEV)}
    loss_fn = elastic.ModuliLoss(("k_sc", "g_sc"), kind="mse")

    def step(xs):
        props = elastic.elastic_moduli_from_irreps(xs, polycrystal=True)
        loss = loss_fn(props, targets)
        (grad,) = torch.autograd.grad(loss, xs)
        return loss, grad, props.k_hs_lower, props.sc_status

    sx = x.clone().requires_grad_()
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(sx)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step(sx)
    for scale in (1.0, 0.5, 2.0):
        with torch.no_grad():
            sx.copy_(x * scale)
        graph.replay()
        torch.cuda.synchronize()
        eager = step((x * scale).requires_grad_())
        assert torch.isfinite(eager[0]) and eager[1].abs().max() > 0
        for c, e in zip(captured, eager):
            assert torch.equal(c, e)


def test_predict_with_polycrystal_moduli():
    from matten_amd import elastic
    from matten_amd import predict as P
    from matten_amd.data import synthetic
    from matten_amd.model_factory.tfn_scalar_tensor import ScalarTensorModel

    structs = synthetic.fcc64_structures(3)
    structs = [{k: s[k] for k in ("lattice", "cart_coords", "atomic_numbers")} for s in structs]
    ds = {"allowed_species": list(synthetic.FCC_METALS), "average_num_neighbors": 18.0}
    torch.manual_seed(35)
    model = ScalarTensorModel(backbone_hparams=dict(LMAX2), dataset_hparams=ds).to(DEV).eval()
    cfg = {"data": {"r_cut": 5.0, "tensor_target_name": "elastic_tensor_full", "tensor_target_formula": "ijkl=jikl=klij"}}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, without = P.predict(structs, model=model, config=cfg, properties=True)
        tensors, props = P.predict(structs, model=model, config=cfg, properties=True, polycrystal=True)
        with pytest.raises(ValueError, match="properties=True"):
            P.predict(structs, model=model, config=cfg, polycrystal=True)
        with pytest.raises(ValueError, match="hs_grid"):
            P.predict(structs, model=model, config=cfg, properties=True, polycrystal=True, hs_grid=1)
    got, base = props.to_dict(), without.to_dict()
    assert len(tensors) == 3 and list(got) == list(base) + list(elastic.POLYCRYSTAL_FIELDS)
    for k, v in base.items():                      # the existing fields: bit-equal to a call without the flag
        assert np.array_equal(v, got[k], equal_nan=True), k
    status = got["sc_status"]
    assert status.shape == (3,) and set(status.tolist()) <= {0, 1, 2}      # (a random-init model: any signature)
    for b in range(3):
        values = [got[n][b] for n in NAMES6]
        if status[b] == 2:
            assert np.isnan(values).all() and got["sc_iterations"][b] == 0
        else:
            assert np.isfinite(values).all() and np.isfinite(got["hs_media"][b]).all()
            slack = 1.0 + 1e-12
            for lo, hsl, sc, hsu, hi in (("k_reuss", "k_hs_lower", "k_sc", "k_hs_upper", "k_voigt"),
                                         ("g_reuss", "g_hs_lower", "g_sc", "g_hs_upper", "g_voigt")):
                chain = [got[n][b] for n in (lo, hsl, sc, hsu, hi)]
                assert all(a <= c * slack for a, c in zip(chain, chain[1:])), (b, chain)
