"""
The Kelvin decomposition on the GPU (matten_amd/elastic.py over csrc/kelvin.hip, csrc/sym6.h) against the numpy restatement
``kelvin_host`` / ``kelvin_bwd_host`` / ``nearest_stable_host`` (LAPACK; tested in tests/test_kelvin_host.py, whose
generators and pool of 257 rows this file shares), the differentiable route from the model's irreps rows against torch's
``eigvalsh`` in fp64 on the CPU, the clamp, and the penalty on a padded batch.

Bounds.  Cyclic Jacobi and LAPACK's eigh are both backward stable: each returns the exact decomposition of a matrix within
a few eps max|C^| of C^, so eigenvalues agree to that and the residuals C^ U - U L and U^T U - 1 are of that size.  1e-13
(450 eps) is the bound tests/test_gpu_rank2.py uses for the same rotation on 3 x 3 matrices; a numpy run of the 6 x 6
rotation reaches 4.3e-15.  The pool holds nearly degenerate clusters too (test_kelvin_host.NEARLY), six of them rows on
which seven sweeps of the rotation leave a residual of 1e-10 to 9e-9 max|C^|: the sweep count of csrc/sym6.h is held to the
bound where it is hardest to meet.
"""
import numpy as np
import pytest
import torch

from test_kelvin_host import (GAP, INF_ROW, NAN_ROW, PREFIXES, ZERO_ROW, cubic, gap_ok, isotropic, kelvin_pool,
                              mandel_weight)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def pool():
    """the pool through ``elastic_properties(kelvin=True)`` once, and the host restatement of what the kernel was given (its
    ``voigt`` and ``flags``): shared by the tests below, never written to"""
    from matten_amd import elastic

    C, kinds = kelvin_pool()
    props = elastic.elastic_properties(C, kelvin=True)
    voigt, flags = props.voigt, props.flags
    ref = elastic.kelvin_host(voigt.cpu().numpy(), flags.cpu().numpy())
    bad = np.isnan(ref["kelvin_moduli"]).any(axis=1)
    with np.errstate(invalid="ignore"):
        big = np.abs(ref["mandel"]).max(axis=(1, 2))
    return dict(C=C, kinds=kinds, props=props, voigt=voigt, flags=flags, ref=ref, bad=bad, ok=~bad, big=big)


def _np(t):
    return t.detach().cpu().numpy()


# ----------------------------------------------------------------------------------------------------------------------
# forward
# ----------------------------------------------------------------------------------------------------------------------
def test_forward_against_kelvin_host(pool):
    """Per row, in units of max|C^|: moduli and margin within 1e-13; C^ U = U L within 1e-13 max|C^| and U^T U = 1 within
    1e-13; the dilatation within 1e-12 absolute on the rows that pass the gap test (GAP = 0.02 max|C^|), in [0, 1]
    everywhere.  Measured on one MI355X over the 257 rows: moduli and margin 1.6e-15, residual 1.2e-15 of max|C^|,
    orthogonality 1.1e-15, dilatation 7.3e-15 (77 rows)."""
    p, ref, ok, big = pool["props"], pool["ref"], pool["ok"], pool["big"][pool["ok"]]
    lam, U, dil = _np(p.kelvin_moduli), _np(p.kelvin_vectors), _np(p.kelvin_dilatation)
    assert lam.shape == (257, 6) and U.shape == (257, 6, 6) and dil.shape == (257, 6) and lam.dtype == np.float64
    err = np.abs(lam[ok] - ref["kelvin_moduli"][ok]).max(axis=1) / big
    merr = np.abs(_np(p.stability_margin)[ok] - ref["stability_margin"][ok]) / big
    Ch = ref["mandel"][ok]
    resid = np.abs(Ch @ U[ok] - U[ok] * lam[ok][:, None, :]).max(axis=(1, 2)) / big
    ortho = np.abs(U[ok].transpose(0, 2, 1) @ U[ok] - np.eye(6)).max(axis=(1, 2))
    keep = gap_ok(_np(pool["voigt"]))
    assert keep.sum() >= 64 and not keep[pool["bad"]].any()
    derr = np.abs(dil[keep] - ref["kelvin_dilatation"][keep]).max()
    print(f"moduli {err.max():.2e}, margin {merr.max():.2e}, residual {resid.max():.2e} of max|C^|; orthogonality "
          f"{ortho.max():.2e}; dilatation {derr:.2e} on {keep.sum()} rows")
    assert (err <= 1e-13).all(), (err.max(), int(err.argmax()))
    assert (merr <= 1e-13).all()
    assert (resid <= 1e-13).all() and (ortho <= 1e-13).all()
    assert derr <= 1e-12
    assert (np.diff(lam[ok], axis=1) >= 0).all()
    assert ((dil[ok] >= 0) & (dil[ok] <= 1 + 1e-12)).all() and np.abs(dil[ok].sum(axis=1) - 1.0).max() <= 1e-12
    assert np.array_equal(_np(p.stability_margin), lam[:, 0], equal_nan=True)
    cond = _np(p.kelvin_condition)
    stable = ok & (np.nan_to_num(lam[:, 0]) > 0)
    assert np.array_equal(cond[stable], lam[stable, 5] / lam[stable, 0]) and np.isnan(cond[~stable]).all()
    # the known answers
    from matten_amd import elastic

    known = elastic.elastic_properties(np.stack([isotropic(100.0, 40.0), cubic(250.0, 120.0, 80.0)]), kelvin=True)
    want = np.array([[80.0, 80.0, 80.0, 80.0, 80.0, 300.0], [130.0, 130.0, 160.0, 160.0, 160.0, 490.0]])
    assert np.abs(_np(known.kelvin_moduli) - want).max() <= 1e-12
    assert np.abs(_np(known.kelvin_dilatation) - [0, 0, 0, 0, 0, 1]).max() <= 1e-12
    eps = _np(elastic.eigenstrains(known))
    assert eps.shape == (2, 6, 3, 3) and np.abs((eps ** 2).sum(axis=(2, 3)) - 1.0).max() <= 1e-13


def test_flagged_rows_are_nan(pool):
    p, flags = pool["props"], _np(pool["flags"])
    assert flags[NAN_ROW] & 1 and flags[INF_ROW] & 1 and NAN_ROW < 63 and INF_ROW < 63
    bad = (flags & 1) != 0
    assert np.array_equal(bad, pool["bad"])          # every NaN row of the restatement is a flagged row here
    for name in ("kelvin_moduli", "kelvin_vectors", "kelvin_dilatation", "stability_margin", "kelvin_condition"):
        v = _np(getattr(p, name))
        assert np.isnan(v[bad]).all() and (name == "kelvin_condition" or np.isfinite(v[~bad]).all()), name
    # a non-finite entry under a clear flag is caught by the kernel itself, overflow of the Mandel factor included
    from matten_amd import ops

    C = torch.tensor(np.stack([isotropic(100.0, 40.0)] * 4), device=DEV)
    C[1, 3, 4] = float("nan")
    C[2, 5, 5] = 1e308                               # 2 * 1e308 overflows
    C[3, 0, 1] = float("-inf")
    lam, U, dil = ops.elastic_kelvin(C, torch.zeros(4, dtype=torch.int32, device=DEV))
    assert torch.isfinite(lam[0]).all() and torch.isfinite(U[0]).all() and torch.isfinite(dil[0]).all()
    assert torch.isnan(lam[1:]).all() and torch.isnan(U[1:]).all() and torch.isnan(dil[1:]).all()


def test_positive_definiteness_agrees_with_the_flag(pool):
    """(smallest modulus > 0) == (flag bit 1 clear) on every finite row whose smallest modulus is further than
    1e-10 max|C^| from zero: all but the one deliberate zero-modulus row"""
    lam, flags, ok = _np(pool["props"].kelvin_moduli), _np(pool["flags"]), pool["ok"]
    decided = ok & (np.abs(np.nan_to_num(lam[:, 0])) > 1e-10 * np.nan_to_num(pool["big"], nan=1.0))
    exempt = np.nonzero(ok & ~decided)[0]
    assert exempt.tolist() == [ZERO_ROW]
    assert np.array_equal(lam[decided, 0] > 0, (flags[decided] & 2) == 0)
    assert (lam[decided, 0] > 0).sum() >= 100 and (lam[decided, 0] < 0).sum() >= 40


def test_bits_repeat_and_do_not_depend_on_the_batch(pool):
    from matten_amd import ops

    voigt, flags = pool["voigt"], pool["flags"]
    lam, U, dil = ops.elastic_kelvin(voigt, flags)
    for t, name in ((lam, "kelvin_moduli"), (U, "kelvin_vectors"), (dil, "kelvin_dilatation")):
        assert np.array_equal(_np(t), _np(getattr(pool["props"], name)), equal_nan=True), name
    for n in PREFIXES:
        a = ops.elastic_kelvin(voigt[:n].clone(), flags[:n].clone())
        for got, want in zip(a, (lam, U, dil)):
            assert got.shape[0] == n and np.array_equal(_np(got), _np(want[:n]), equal_nan=True), n
    tail = ops.elastic_kelvin(voigt[200:].clone(), flags[200:].clone())
    assert np.array_equal(_np(tail[0]), _np(lam[200:]))
    # the moduli are the same bits whichever of the other outputs are asked for
    for want_vectors, want_dilatation in ((False, False), (True, False), (False, True)):
        l2, U2, d2 = ops.elastic_kelvin(voigt, flags, want_vectors=want_vectors, want_dilatation=want_dilatation)
        assert np.array_equal(_np(l2), _np(lam), equal_nan=True), (want_vectors, want_dilatation)
        assert (U2 is None) == (not want_vectors) and (d2 is None) == (not want_dilatation)
        assert U2 is None or np.array_equal(_np(U2), _np(U), equal_nan=True)
        assert d2 is None or np.array_equal(_np(d2), _np(dil), equal_nan=True)
    empty = ops.elastic_kelvin(voigt[:0], flags[:0])
    assert empty[0].shape == (0, 6) and empty[1].shape == (0, 6, 6)


# ----------------------------------------------------------------------------------------------------------------------
# adjoint
# ----------------------------------------------------------------------------------------------------------------------
def test_adjoint_against_kelvin_bwd_host(pool):
    """g_voigt = D (U diag(g) U^T) D with the forward's U on both sides, so the two differ by the rounding of 6-term sums:
    within 1e-13 max|g| per row.  Flagged rows get exact +0.0 whatever arrives.  Measured on one MI355X: 3.6e-16 of max|g|."""
    from matten_amd import elastic, ops

    voigt, flags, U = pool["voigt"], pool["flags"], pool["props"].kelvin_vectors
    rng = np.random.default_rng(5)
    g = rng.standard_normal((257, 6))
    g[pool["bad"]] = np.nan
    g[3] = [1.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    got = _np(ops.elastic_kelvin_bwd(U, flags, torch.tensor(g, device=DEV)))
    want = elastic.kelvin_bwd_host(_np(voigt), g, _np(flags), vectors=_np(U))
    ok = pool["ok"]
    scale = np.abs(g[ok]).max(axis=1)
    err = np.abs(got[ok] - want[ok]).max(axis=(1, 2)) / scale
    print(f"adjoint against kelvin_bwd_host: {err.max():.2e} of max|g| per row")
    assert (err <= 1e-13).all()
    assert np.array_equal(got, got.transpose(0, 2, 1))
    assert (got[~ok] == 0).all() and not np.signbit(got[~ok]).any()
    # with LAPACK's own vectors the per-modulus gradients agree where the moduli are separated
    keep = gap_ok(_np(voigt))
    lapack = elastic.kelvin_bwd_host(_np(voigt), g, _np(flags))
    rel = np.abs(got[keep] - lapack[keep]).max(axis=(1, 2)) / np.abs(g[keep]).max(axis=1)
    # (eigenvectors within 8e-15 / GAP of each other; six terms of two factors each, the Mandel factor at most 2)
    assert (rel <= 2.0 * 6 * 2 * 8e-15 / GAP).all()
    # the trace's gradient is D^2 on the diagonal, whatever the basis (U^T U = 1 to 1e-13: the forward's bound)
    ones = _np(ops.elastic_kelvin_bwd(U, flags, torch.ones(257, 6, dtype=torch.float64, device=DEV)))
    assert np.abs(ones[ok] - np.diag(np.diag(mandel_weight()))).max() <= 2e-13
    # prefixes: a row's bits do not depend on its batch
    gd = torch.tensor(g, device=DEV)
    for n in PREFIXES:
        part = _np(ops.elastic_kelvin_bwd(U[:n].clone(), flags[:n].clone(), gd[:n].clone()))
        assert np.array_equal(part, got[:n]), n


def test_autograd_from_irreps_rows_against_eigvalsh():
    """x [65,21] fp32 (seeded normal: tensors of any signature), the squared ``StabilityPenalty`` at margin 0.5 (active and
    inactive modes in every batch of this size, asserted) on ``elastic_moduli_from_irreps(x, kelvin=True)``.  Reference: the
    same function with torch.linalg.eigvalsh in fp64 on the CPU, on the widened x and the fp64 basis.  The tolerance is the
    one of the rank-2 irreps route (tests/test_gpu_rank2.py::test_autograd_from_irreps_rows_against_eigvalsh), K_IRREPS = 8
    in units of 2^-23 max|grad|: the device differs from the reference by the fp32 rounding of the two dense_rows products
    (forward [65,36], adjoint [65,21]), whose emulation on the CPU is asserted to stay below 2; the value is held to its
    first-order sensitivity to the forward product's rounding.  Measured on one MI355X: k = 0.70 (the CPU emulation: 0.70), value off by 9.7e-9 against a bound of 4.1e-6."""
    from matten_amd import elastic

    K_IRREPS = 8.0
    gen = torch.Generator().manual_seed(2)
    x = torch.randn(65, 21, generator=gen)
    V64 = torch.from_numpy(elastic.voigt_basis().copy())
    V32 = V64.float()
    W = torch.from_numpy(mandel_weight())
    margin = 0.5

    def penalty(rows):
        C = rows.reshape(-1, 6, 6)
        lam = torch.linalg.eigvalsh(W * (0.5 * (C + C.transpose(1, 2))))
        return lam, (torch.relu(margin - lam) ** 2).mean()

    x64 = x.double().requires_grad_()
    lam_ref, want = penalty(x64 @ V64)
    assert (lam_ref < margin).any() and (lam_ref > margin).any()
    want.backward()
    unit = 2.0 ** -23 * x64.grad.abs().max().item()
    rows = (x @ V32).double().requires_grad_()
    penalty(rows)[1].backward()
    k_cpu = ((rows.grad.float() @ V32.T).double() - x64.grad).abs().max().item() / unit
    print(f"CPU emulation of the two fp32 products: k = {k_cpu:.2f}")
    assert k_cpu <= 2.0

    xd = x.to(DEV).requires_grad_()
    props = elastic.elastic_moduli_from_irreps(xd, kelvin=True)
    got = elastic.StabilityPenalty(margin, "squared")(props)
    got.backward()
    assert (props.flags & 1).sum() == 0 and xd.grad.dtype == torch.float32 and got.dtype == torch.float64
    assert props.kelvin_moduli.requires_grad and props.stability_margin.requires_grad
    assert not props.kelvin_vectors.requires_grad and not props.kelvin_dilatation.requires_grad
    assert not props.kelvin_condition.requires_grad
    k_dev = (xd.grad.cpu().double() - x64.grad).abs().max().item() / unit
    first_order = 4.0 * 2.0 ** -23 * (rows.grad.abs() * (x.abs().double() @ V64.abs())).sum().item()
    print(f"device: k = {k_dev:.2f}; penalty {got.item():.12e} against {want.item():.12e} (bound {first_order:.2e})")
    assert k_dev <= K_IRREPS
    assert abs(got.item() - want.item()) <= first_order
    # the same bits as the route without gradient, and the other fields untouched by the keyword
    plain = elastic.elastic_properties_from_irreps(x.to(DEV), kelvin=True)
    assert torch.equal(plain.kelvin_moduli, props.kelvin_moduli.detach()) and torch.equal(plain.voigt, props.voigt.detach())
    # the moduli alone (what stability_penalized asks for): no dilatation is written, the same bits, the same gradient
    xl = x.to(DEV).requires_grad_()
    lean = elastic.elastic_moduli_from_irreps(xl, kelvin=True, kelvin_dilatation=False)
    assert lean.kelvin_dilatation is None and torch.equal(lean.kelvin_moduli, props.kelvin_moduli)
    assert torch.equal(lean.kelvin_vectors, props.kelvin_vectors) and lean.to_dict()["kelvin_dilatation"] is None
    elastic.StabilityPenalty(margin, "squared")(lean).backward()
    assert torch.equal(xl.grad, xd.grad)
    without = elastic.elastic_moduli_from_irreps(x.to(DEV))
    assert not hasattr(without, "kelvin_moduli") and torch.equal(without.k_vrh, props.k_vrh.detach())
    assert torch.equal(without.flags, props.flags)


# ----------------------------------------------------------------------------------------------------------------------
# the nearest stable tensor
# ----------------------------------------------------------------------------------------------------------------------
def test_clamp(pool):
    """``nearest_stable`` against ``nearest_stable_host`` within 1e-13 max|C^| per row at floors 0 and 1e-6 max|C^| of each
    row's own scale (one floor per call: rows are grouped by their floor); rows already >= floor come back unchanged, bit
    for bit; the repaired tensors have flag bit 1 clear.  Measured on one MI355X: 2.8e-15 (floor 0) and 2.9e-15 of max|C^|."""
    from matten_amd import elastic, ops

    C, ok, big, ref = pool["C"], pool["ok"], pool["big"], pool["ref"]
    sym = _np(pool["voigt"])
    V, cart, changed = elastic.nearest_stable(C, 0.0)
    assert V.shape == (257, 6, 6) and cart.shape == (257, 3, 3, 3, 3) and changed.shape == (257,) and changed.dtype == torch.bool
    V, cart, changed = _np(V), _np(cart), _np(changed)
    want, want_cart, want_changed = elastic.nearest_stable_host(sym, 0.0, _np(pool["flags"]))
    lam = _np(pool["props"].kelvin_moduli)
    decided = ok & (np.abs(np.nan_to_num(lam[:, 0])) > 1e-10 * np.nan_to_num(big, nan=1.0))
    assert np.array_equal(changed[decided], want_changed[decided]) and not changed[~ok].any()
    assert np.isnan(V[~ok]).all() and np.isnan(cart[~ok]).all()
    err = np.abs(V[ok] - want[ok]).max(axis=(1, 2)) / big[ok]
    print(f"clamp at floor 0 against the host restatement: {err.max():.2e} of max|C^|")
    assert (err <= 1e-13).all()
    assert np.array_equal(cart, elastic.voigt_to_cartesian(V), equal_nan=True) and np.array_equal(V, V.transpose(0, 2, 1), equal_nan=True)
    keep = ok & ~changed
    assert keep.sum() >= 100 and np.array_equal(V[keep], sym[keep])          # changed == False: the input, bit for bit
    assert (np.abs(V[keep] - sym[keep]).max(axis=(1, 2)) <= 1e-13 * big[keep]).all()
    # floor = 1e-6 max|C^| per row: every finite row comes back positive definite
    rows = np.nonzero(ok)[0]
    floors = 1e-6 * big[rows]
    moduli, vectors = pool["props"].kelvin_moduli, pool["props"].kelvin_vectors
    repaired = torch.empty(len(rows), 6, 6, dtype=torch.float64, device=DEV)
    for f in np.unique(floors):
        sel = torch.tensor(rows[floors == f], device=DEV)
        at = torch.tensor(np.nonzero(floors == f)[0], device=DEV)
        repaired[at] = ops.elastic_kelvin_clamp(pool["voigt"][sel], moduli[sel], vectors[sel], float(f))
    host = np.stack([elastic.nearest_stable_host(sym[r], f)[0] for r, f in zip(rows, floors)])
    err = np.abs(_np(repaired) - host).max(axis=(1, 2)) / big[rows]
    print(f"clamp at floor 1e-6 max|C^| against the host restatement: {err.max():.2e} of max|C^|")
    assert (err <= 1e-13).all()
    again = elastic.elastic_properties(repaired, kelvin=True)
    assert ((again.flags & 3) == 0).all()                                     # finite, and flag bit 1 cleared on every row
    assert (_np(again.stability_margin) >= floors - 1e-13 * big[rows]).all()
    lifted = lam[rows, 0] < floors
    assert lifted.sum() >= 40 and (np.abs(_np(again.kelvin_moduli)[lifted, 0] - floors[lifted]) <= 1e-13 * big[rows][lifted]).all()
    # unbatched, Cartesian input, a list
    one = elastic.nearest_stable(C[ZERO_ROW + 1], 0.0)
    assert one[0].shape == (6, 6) and one[1].shape == (3, 3, 3, 3) and one[2].shape == () and bool(one[2])
    assert np.array_equal(_np(one[0]), V[ZERO_ROW + 1])
    c4 = elastic.voigt_to_cartesian(C[ZERO_ROW + 1:ZERO_ROW + 4])
    from_cart = elastic.nearest_stable(c4, 0.0)
    assert np.array_equal(_np(from_cart[0]), V[ZERO_ROW + 1:ZERO_ROW + 4])
    assert not any(t.requires_grad for t in from_cart)


# ----------------------------------------------------------------------------------------------------------------------
# the penalty on a padded batch
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["squared", "hinge"])
def test_penalty_on_a_padded_batch(kind):
    """x [40,21] fp32, the first 29 rows real (``n_valid`` a device word): the padding rows holding zeros, other numbers or
    NaN change no bit of the value or of the gradient, the padding rows' gradient is exactly zero, the value is the mean
    over the 29 x 6 real modes (within fp32 rounding of the fp64 mean), and a margin below every modulus gives exactly 0
    with an all-zero gradient."""
    from matten_amd import elastic

    gen = torch.Generator().manual_seed(4)
    x = torch.randn(40, 21, generator=gen)
    n_valid = torch.tensor([29], dtype=torch.int64, device=DEV)
    pen = elastic.StabilityPenalty(0.5, kind)

    def run(fill, penalty=pen):
        xp = x.clone()
        xp[29:] = fill
        xd = xp.to(DEV).requires_grad_()
        props = elastic.elastic_moduli_from_irreps(xd, kelvin=True)
        value = penalty(props, n_valid)
        value.backward()
        return value.detach(), xd.grad, props

    v0, g0, props = run(0.0)
    lam = _np(props.kelvin_moduli)[:29]
    assert (lam < 0.5).any() and (lam > 0.5).any() and v0.dtype == torch.float32 and float(v0) > 0
    short = np.maximum(0.5 - lam, 0.0)
    want = (short ** 2 if kind == "squared" else short).mean()
    assert abs(float(v0) - want) <= 4 * 2.0 ** -24 * want
    assert g0[:29].abs().max() > 0 and not g0[29:].any()
    for fill in (7.5, float("nan"), float("inf")):
        v, g, p = run(fill)
        assert torch.equal(v, v0) and torch.equal(g, g0), fill
        assert fill == 7.5 or bool((p.flags[29:] & 1).all())
    # all rows valid: the torch mean in fp64 and the kernel's agree
    full = elastic.elastic_moduli_from_irreps(x.to(DEV), kelvin=True)
    a, b = pen(full), pen(full, torch.tensor([40], dtype=torch.int64, device=DEV))
    assert a.dtype == torch.float64 and abs(float(a) - float(b)) <= 4 * 2.0 ** -24 * float(a)
    # a margin below every modulus
    low = float(_np(full.kelvin_moduli).min()) - 1.0
    for nv in (None, n_valid):
        xd = x.to(DEV).requires_grad_()
        value = elastic.StabilityPenalty(low, kind)(elastic.elastic_moduli_from_irreps(xd, kelvin=True), nv)
        value.backward()
        assert float(value.detach()) == 0.0 and not xd.grad.any()
