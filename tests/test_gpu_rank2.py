"""Per-atom shielding parameters on the GPU (csrc/rank2.hip through matten_amd/rank2.py): ``matten_rank2_props`` and its
adjoint against the numpy restatement ``rank2_host`` / ``rank2_bwd_host`` (LAPACK, never the kernel itself), the autograd
route from the model's irreps rows against torch's ``eigvalsh`` in fp64 on the CPU, and a captured forward + backward
with ``Rank2Loss``.  One pool of 257 rows serves every test: row counts 1, 63, 64, 65 and 257 are its prefixes (wave and
workgroup edges), and the reference of the pool is computed once."""
import numpy as np
import pytest
import torch

from test_rank2_host import fixture_tensors, gap_ok, random_tensors

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
COUNTS = (1, 63, 64, 65, 257)
NAN_ROW, INF_ROW, IDENTITY_ROW = 6, 9, 7


def _pool() -> np.ndarray:
    """[257,3,3] fp64: the 20 fixture tensors, 55 random general tensors at each entry scale 1e-4, 1e-2, 1, 30 around
    isotropic parts in +-500, a diagonal tensor, c I, axially symmetric tensors (diagonal and rotated, both signs), a NaN
    row and an Inf row between good rows; the special rows sit inside the first 63"""
    fx = fixture_tensors()
    rnd = np.concatenate([random_tensors(55, s, 100 + q) for q, s in enumerate((1e-4, 1e-2, 1.0, 30.0))])
    rng = np.random.default_rng(9)
    R, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    bad, inf = rnd[0].copy(), rnd[60].copy()
    bad[1, 2], inf[2, 0] = np.nan, -np.inf
    special = [np.diag([4.0, 1.0, 2.0]), bad, -212.25 * np.eye(3), rnd[1], inf, np.diag([1.0, 1.0, 5.0]),
               R @ np.diag([310.0, 310.0, 290.0]) @ R.T, np.diag([-7.0, 2.0, 2.0])]
    rng.shuffle(rnd)      # the scales interleave: every prefix holds all four
    pool = np.concatenate([fx[:5], np.stack(special), fx[5:], rnd, random_tensors(9, 1.0, 200)])
    assert pool.shape == (257, 3, 3) and np.isnan(pool[NAN_ROW]).any() and np.isinf(pool[INF_ROW]).any()
    assert np.array_equal(pool[IDENTITY_ROW], -212.25 * np.eye(3))
    return pool


@pytest.fixture(scope="module")
def pool():
    from matten_amd.rank2 import rank2_host

    T = _pool()
    T.setflags(write=False)
    ref = rank2_host(T)
    for v in ref.values():
        v.setflags(write=False)
    return T, ref


def _run(T, dtype=torch.float64):
    from matten_amd import ops

    t = torch.as_tensor(np.array(T)).to(dtype).reshape(-1, 9).to(DEV)
    return ops.rank2_props(t)


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


# ----------------------------------------------------------------------------------------------------------------------
# forward
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", COUNTS)
def test_forward_matches_the_restatement(pool, n):
    """Per row, in units of max|A| (A the symmetrised input): principal values, iso, span and zeta within 1e-13, skew and
    eta within 1e-13 / span; A U = U diag(l) within 1e-13 max|A| and U^T U = 1 within 1e-13.  Measured on one MI355X over
    the 257 rows: values 6.9e-16, iso 2.1e-16, span 1.0e-15, zeta 3.4e-16 of max|A|; skew 1.9e-15 and eta 1.4e-15 of
    max|A| / span; residual 3.4e-16 max|A|, orthonormality 4.4e-16."""
    T, ref = pool
    T, ref = T[:n], {k: v[:n] for k, v in ref.items()}
    vals, axes, props, flags = (t.cpu().numpy() for t in _run(T))
    assert vals.shape == (n, 3) and axes.shape == (n, 3, 3) and props.shape == (n, 5) and flags.shape == (n,)
    assert np.array_equal(flags, ref["flags"])
    ok = ref["flags"] & 1 == 0
    A = 0.5 * (T + T.transpose(0, 2, 1))[ok]
    m = np.abs(A).max(axis=(1, 2))
    assert (np.diff(vals[ok], axis=1) >= 0).all()
    worst = {}

    def check(name, got, want, unit):
        err = np.abs(got - want) / unit
        worst[name] = err.max()
        assert (err <= 1e-13).all(), (name, err.max(), int(err.argmax()))

    check("principal_values", vals[ok], ref["principal_values"][ok], m[:, None])
    for q, name in enumerate(("iso", "span", "skew", "zeta", "eta")):
        got, want = props[ok, q], ref[name][ok]
        if name in ("skew", "eta", "zeta"):
            flat = ref["is_isotropic"][ok]
            # where |skew| < 1e-6 the Haeberlen branch may legitimately differ: such rows would be left out of zeta and
            # eta -- the pool has none
            near = ~flat & (np.abs(ref["skew"][ok]) < 1e-6)
            assert not near.any()
        if name in ("skew", "eta"):
            with np.errstate(divide="ignore"):
                unit = np.where(flat, 1.0, m / np.where(flat, 1.0, ref["span"][ok]))
            check(name, got, want, unit)
        else:
            check(name, got, want, m)
    assert ((props[ok, 4] >= 0) & (props[ok, 4] <= 1 + 1e-12)).all() and (props[ok, 1] >= 0).all()
    U, lam = axes[ok], vals[ok]
    resid = np.abs(A @ U - U * lam[:, None, :]).max(axis=(1, 2)) / m
    ortho = np.abs(U.transpose(0, 2, 1) @ U - np.eye(3)).max(axis=(1, 2))
    worst["residual"], worst["orthonormality"] = resid.max(), ortho.max()
    print(f"n = {n}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert (resid <= 1e-13).all() and (ortho <= 1e-13).all()
    # flagged rows are NaN, c I carries bit 1 with exact zeros
    for i in np.nonzero(~ok)[0]:
        assert flags[i] == 1 and np.isnan(vals[i]).all() and np.isnan(axes[i]).all() and np.isnan(props[i]).all()
    if n > IDENTITY_ROW:
        i = IDENTITY_ROW
        assert flags[i] == 2 and props[i, 2] == 0.0 and props[i, 4] == 0.0 and props[i, 1] == 0.0
        assert not np.signbit(props[i, [2, 4]]).any() and props[i, 0] == -212.25 and (vals[i] == -212.25).all()
        assert (n > INF_ROW) and flags[NAN_ROW] == 1 and flags[INF_ROW] == 1 and (flags == 1).sum() == 2


def test_rows_do_not_depend_on_their_batch_and_calls_repeat(pool):
    T, _ = pool
    whole = _run(T[:65])
    again = _run(T[:65])
    for a, b in zip(whole, again):
        assert torch.equal(_bits(a), _bits(b))
    for i in range(65):      # NaN rows included: the bits are compared
        alone = _run(T[i : i + 1])
        for a, b in zip(whole, alone):
            assert torch.equal(_bits(a[i : i + 1]), _bits(b)), i
    big = _run(T)
    for a, b in zip(whole, big):
        assert torch.equal(_bits(a), _bits(b[:65]))
    # without the axes: the same values
    from matten_amd import ops

    t = torch.as_tensor(np.array(T)).reshape(-1, 9).to(DEV)
    vals, axes, props, flags = ops.rank2_props(t, want_axes=False)
    assert axes is None and torch.equal(_bits(vals), _bits(big[0])) and torch.equal(_bits(props), _bits(big[2]))
    assert torch.equal(flags, big[3])
    empty = ops.rank2_props(t[:0])
    assert empty[0].shape == (0, 3) and empty[3].shape == (0,)


def test_fp32_input_is_the_fp64_call_on_the_widened_values(pool):
    T, _ = pool
    narrow = T.astype(np.float32)
    a, b = _run(narrow, torch.float32), _run(narrow.astype(np.float64))
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and torch.equal(_bits(x), _bits(y))


def test_public_entries_take_every_input_form(pool):
    from matten_amd.rank2 import Rank2Properties, rank2_invariants, rank2_properties

    T, ref = pool
    T = T[:65]
    want = rank2_properties(torch.as_tensor(T.copy()).to(DEV))
    assert isinstance(want, Rank2Properties) and want.iso.is_cuda and want.principal_axes.shape == (65, 3, 3)
    assert torch.equal(want.anisotropy[want.flags == 0], 1.5 * want.zeta[want.flags == 0])
    assert want.is_isotropic.tolist() == ref["is_isotropic"][:65].tolist()
    for form in (T.copy(), torch.as_tensor(T.copy()), [t for t in T], [torch.as_tensor(t.copy()) for t in T]):
        got = rank2_properties(form)
        for k in ("principal_values", "principal_axes", "iso", "span", "skew", "zeta", "anisotropy", "eta", "flags"):
            assert torch.equal(_bits(getattr(got, k)), _bits(getattr(want, k))), k
    one = rank2_properties(T[0])
    assert one.iso.shape == () and one.principal_values.shape == (3,) and one.principal_axes.shape == (3, 3)
    assert torch.equal(one.iso, want.iso[0])
    d = want.cpu().to_dict()
    assert set(d) == {"principal_values", "principal_axes", "iso", "span", "skew", "zeta", "anisotropy", "eta", "flags",
                      "is_isotropic"} and isinstance(d["iso"], np.ndarray)
    # the differentiable twin: the same kernel, the same bits
    twin = rank2_invariants(torch.as_tensor(T.copy()).to(DEV).requires_grad_())
    assert twin.iso.requires_grad and not twin.principal_axes.requires_grad and not twin.flags.requires_grad
    for k in ("principal_values", "iso", "span", "skew", "zeta", "eta"):
        assert torch.equal(_bits(getattr(twin, k).detach()), _bits(getattr(want, k))), k


# ----------------------------------------------------------------------------------------------------------------------
# adjoint
# ----------------------------------------------------------------------------------------------------------------------
def _upstream(n, seed=4):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, 3)), rng.standard_normal((n, 5))


def _bwd(out, g_vals, g_props, dtype=torch.float64):
    from matten_amd import ops

    dev = lambda g: None if g is None else torch.as_tensor(np.ascontiguousarray(g)).to(DEV)
    return ops.rank2_props_bwd(*out, dev(g_vals), dev(g_props), dtype).cpu().numpy().reshape(-1, 3, 3)


def test_adjoint_matches_the_restatement(pool):
    """On the rows of the pool whose relative gaps and |skew| are >= 0.05 (the condition of tests/test_rank2_host.py's
    gradient check; the pool keeps >= 80 % of its finite rows): within 1e-12 max|g_T| per row of ``rank2_bwd_host``.
    Measured on one MI355X: 4.8e-15 at worst (227 of the 255 finite rows meet the condition)."""
    from matten_amd.rank2 import rank2_bwd_host

    T, ref = pool
    keep = gap_ok(T)
    finite = ref["flags"] & 1 == 0
    print(f"gap-conditioned rows: {keep.sum()} of {finite.sum()} finite rows")
    assert keep.sum() >= 0.8 * finite.sum()
    g_vals, g_props = _upstream(len(T))
    out = _run(T)
    got = _bwd(out, g_vals, g_props)
    want = rank2_bwd_host(T, g_vals, g_props)
    assert np.array_equal(got, got.transpose(0, 2, 1)) and np.isfinite(got).all()
    scale = np.abs(want[keep]).max(axis=(1, 2))
    err = np.abs(got[keep] - want[keep]).max(axis=(1, 2)) / scale
    print(f"adjoint against rank2_bwd_host: {err.max():.2e} of max|g_T| per row at worst (row {np.nonzero(keep)[0][err.argmax()]})")
    assert (err <= 1e-12).all()
    # NULL upstream gradients are zeros
    for gv, gp in ((g_vals, None), (None, g_props)):
        part = _bwd(out, gv, gp)
        zeros = _bwd(out, np.zeros_like(g_vals) if gv is None else gv, np.zeros_like(g_props) if gp is None else gp)
        assert np.array_equal(part, zeros)
    assert not _bwd(out, None, None).any()
    # fp32 output: the fp64 one rounded
    assert np.array_equal(_bwd(out, g_vals, g_props, torch.float32), got.astype(np.float32))
    # a prefix gives the same rows
    n = 65
    assert np.array_equal(_bwd(tuple(t[:n] for t in out), g_vals[:n], g_props[:n]), got[:n])


def test_adjoint_of_excluded_rows(pool):
    T, ref = pool
    T = T[:64]
    out = _run(T)
    g_vals, g_props = _upstream(64)
    base = _bwd(out, g_vals, g_props)
    # a row with bit 0 returns exact +0.0 even with NaN upstream
    nasty_v, nasty_p = g_vals.copy(), g_props.copy()
    nasty_v[[NAN_ROW, INF_ROW]], nasty_p[[NAN_ROW, INF_ROW]] = np.nan, np.inf
    # a row with bit 1 ignores the upstream gradients of skew and eta, NaN included
    nasty_p[IDENTITY_ROW, 2], nasty_p[IDENTITY_ROW, 4] = np.nan, -3e300
    got = _bwd(out, nasty_v, nasty_p)
    for i in (NAN_ROW, INF_ROW):
        assert (got[i] == 0).all() and not np.signbit(got[i]).any() and (base[i] == 0).all()
    assert np.array_equal(got, base) and np.isfinite(got).all()
    # on c I the gradient of iso is the identity over three whatever basis Jacobi left
    only_iso = np.zeros((64, 5))
    only_iso[:, 0] = 1.0
    g = _bwd(out, None, only_iso)
    ok = ref["flags"][:64] & 1 == 0
    assert np.abs(g[ok] - np.eye(3) / 3.0).max() <= 1e-13          # (U^T U = 1 to 1e-13: the forward's bound)


# ----------------------------------------------------------------------------------------------------------------------
# autograd end to end, from the irreps rows
# ----------------------------------------------------------------------------------------------------------------------
def _functional_torch(rows, c_vals, c_props):
    """the linear functional of all outputs with torch.linalg.eigvalsh (fp64, wherever rows lives)"""
    T = rows.reshape(-1, 3, 3)
    lam = torch.linalg.eigvalsh(0.5 * (T + T.transpose(1, 2)))
    iso = lam.sum(1) / 3.0
    span = lam[:, 2] - lam[:, 0]
    skew = 3.0 * (lam[:, 1] - iso) / span
    z_hi = skew <= 0
    zeta = torch.where(z_hi, lam[:, 2], lam[:, 0]) - iso
    eta = (lam[:, 1] - torch.where(z_hi, lam[:, 0], lam[:, 2])) / zeta
    props = torch.stack([iso, span, skew, zeta, eta, 1.5 * zeta], dim=1)
    return (lam * c_vals).sum() + (props * c_props).sum()


def test_autograd_from_irreps_rows_against_eigvalsh():
    """x [65,6] fp32 (seeded normal), a random linear functional of the three values, the five scalars and the anisotropy.
    Reference: the same function with torch.linalg.eigvalsh in fp64 on the CPU, on the widened x and the fp64 basis.  The
    device differs from it by the fp32 rounding of the two dense_rows products (forward [65,9], adjoint [65,6]); the same
    two roundings emulated on the CPU (fp32 matmuls around the fp64 function) measure k = 0.7 to 1.0 in units of
    2^-23 max|grad| (two machines; the order of the CPU's sums differs).  The bound is k = 8: that emulation's figure
    with an eightfold margin for the order of the sums; the emulation itself is asserted to stay below 2.  The value of the
    functional is held to its first-order sensitivity to the forward product's rounding, 4 * 2^-23 sum |dL/drows| (|x| |B|).
    Measured on one MI355X: gradient k = 1.03, functional off by 1.7e-6 against a bound of 2.2e-4."""
    from matten_amd.rank2 import rank2_basis, rank2_invariants_from_irreps

    g = torch.Generator().manual_seed(1)
    x = torch.randn(65, 6, generator=g)
    c_vals = torch.randn(65, 3, generator=g, dtype=torch.float64)
    c_props = torch.randn(65, 6, generator=g, dtype=torch.float64)
    B64 = torch.from_numpy(rank2_basis().copy())
    B32 = B64.float()
    x64 = x.double().requires_grad_()
    want = _functional_torch(x64 @ B64, c_vals, c_props)
    want.backward()
    unit = 2.0 ** -23 * x64.grad.abs().max().item()
    # the CPU's measure of the two fp32 products
    rows = (x @ B32).double().requires_grad_()
    _functional_torch(rows, c_vals, c_props).backward()
    k_cpu = ((rows.grad.float() @ B32.T).double() - x64.grad).abs().max().item() / unit
    print(f"CPU emulation of the two fp32 products: k = {k_cpu:.2f}")
    assert k_cpu <= 2.0

    xd = x.to(DEV).requires_grad_()
    p = rank2_invariants_from_irreps(xd)
    cv, cp = c_vals.to(DEV), c_props.to(DEV)
    outs = torch.stack([p.iso, p.span, p.skew, p.zeta, p.eta, p.anisotropy], dim=1)
    got = (p.principal_values * cv).sum() + (outs * cp).sum()
    got.backward()
    assert (p.flags == 0).all() and xd.grad.dtype == torch.float32
    k_dev = (xd.grad.cpu().double() - x64.grad).abs().max().item() / unit
    first_order = 4.0 * 2.0 ** -23 * (rows.grad.abs() * (x.abs().double() @ B64.abs())).sum().item()
    print(f"device: k = {k_dev:.2f}; functional {got.item():.12e} against {want.item():.12e} (bound {first_order:.2e})")
    assert k_dev <= 8.0
    assert abs(got.item() - want.item()) <= first_order


# ----------------------------------------------------------------------------------------------------------------------
# capture
# ----------------------------------------------------------------------------------------------------------------------
def test_captured_forward_and_backward_replay_on_new_contents():
    from matten_amd.rank2 import Rank2Loss, rank2_invariants_from_irreps

    n = 65
    loss_fn = Rank2Loss(("iso", "span"), weights=[1.0, 0.25], kind="mse")
    g = torch.Generator().manual_seed(7)

    def contents(k):
        x = 3.0 * torch.randn(n, 6, generator=g)
        sel = (torch.rand(n, generator=g) < 0.4).to(torch.int32)
        sel[k] = 1
        targets = torch.randn(n, 2, generator=g)
        if k:
            targets[k, 1] = float("nan")      # a selected row without a usable target: dropped on the device
        return x.to(DEV), sel.to(DEV), targets.to(DEV)

    def step(x, sel, targets):
        x = x.detach().requires_grad_()
        loss = loss_fn(rank2_invariants_from_irreps(x), {"iso": targets[:, 0], "span": targets[:, 1:2]}, sel)
        (grad,) = torch.autograd.grad(loss, x)
        return loss, grad

    sx, ssel, st = (t.clone() for t in contents(0))
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(sx, ssel, st)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss_c, grad_c = step(sx, ssel, st)
    for k in (0, 5, 11):
        x, sel, targets = contents(k)
        sx.copy_(x), ssel.copy_(sel), st.copy_(targets)
        graph.replay()
        torch.cuda.synchronize()
        loss_e, grad_e = step(x, sel, targets)
        assert torch.isfinite(loss_e) and torch.isfinite(grad_e).all() and grad_e.abs().max() > 0
        assert torch.equal(_bits(loss_c), _bits(loss_e)) and torch.equal(_bits(grad_c), _bits(grad_e)), k
        if k:
            assert not grad_e[k].any()                 # the row with the NaN target got no gradient
            # ... and the loss is the mean over the remaining selected rows, in fp64 on the host
            from matten_amd.rank2 import rank2_host, rank2_basis

            h = rank2_host((x.cpu().double() @ torch.from_numpy(rank2_basis().copy())).reshape(n, 3, 3).numpy())
            use = sel.cpu().numpy() != 0
            use[k] = False
            t = targets.cpu().double().numpy()
            want = (((h["iso"] - t[:, 0]) ** 2)[use].sum() + 0.25 * ((h["span"] - t[:, 1]) ** 2)[use].sum()) / (2 * use.sum())
            assert abs(loss_e.item() - want) <= 1e-5 * abs(want)
