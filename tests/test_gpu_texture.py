"""
The textured-polycrystal means on the GPU (matten_amd/texture.py over csrc/texture.hip) against the numpy statements
``texture_operator_host`` / ``texture_average_host`` / ``texture_average_bwd_host`` (tested in tests/test_texture_host.py), on
the 257 rows of tests/polycrystal_cases.py -- more than one workgroup, not a multiple of the wave; isotropic, cubic,
hexagonal, 250 seeded triclinic tensors, a near-singular row, a row that is not positive definite, a NaN row -- under the
eight packed textures of tests/texture_cases.py (1, 5, 60, 37 weighted and 10 007 orientations; a sheared matrix, a zero
weight sum, an empty segment) in the full 257 x 8 cross product and in six explicit multi-phase aggregates.

Tolerances.  The reference is the host function, never the kernel.
  * The operator: the reference adds the orientations in ``numpy.longdouble``; the bound is ten times the largest distance
    between that and the same sum in fp64, floor 1e-14, absolute (entries are bounded by 2).  Computed in the fixture:
    2.3e-15 on the 10 007 orientations, so the bound is 2.3e-14.
  * The four means: the distance is relative to the largest entry of the result.  The host's two formulations (w_g N_g X
    N_g^T orientation by orientation, and the 36 x 36 matrix sum_g w_g N_g (x) N_g) differ on this cross product by at
    most voigt 5.8e-14, reuss 1.7e-13, hill 5.7e-14, geometric 1.1e-12 on the ordinary rows (numpy, on the CPU; a minute
    of einsums, so the figure is written here and not computed again).  Ten times the largest, floor 1e-12: TOL = 1.1e-11.
    The near-singular row (condition 1e6) gets TOL times its condition number over 1e3 = 1.1e-8: the device inverts
    through Jacobi eigenvalues good to ~3e-15 max|C^| (csrc/sym6.h), 3e-9 of that row's softest modulus.  (The host's own
    movement on that row: reuss 2.6e-11, hill 8.5e-12.)
  * The adjoint, same rule, relative to the row's largest gradient entry: the host's two formulations differ by at most
    HOST_BWD = 1.7e-12 on the ordinary rows of the cross product (cubic 4.4e-14, isotropic 2.2e-13, near-singular 4.7e-9;
    two minutes of einsums on the CPU), so TOL_BWD = 1.7e-11; the near-singular row times 1e3.
  * End to end against central differences of the host chain: 1e-6 relative, the finite-difference error at h = 1e-5 (not
    a device tolerance).
Measured on one MI355X: see the docstrings of the tests.
"""
import numpy as np
import pytest
import torch

import polycrystal_cases as pc
import texture_cases as tc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SCHEMES = ("voigt", "reuss", "hill", "geometric")
TOL = 1.1e-11
HOST_BWD = 1.7e-12
TOL_BWD = max(10.0 * HOST_BWD, 1e-12)
NEAR_SINGULAR_FACTOR = 1e6 / 1e3
T = tc.N_TEXTURES
GOOD_T, BAD_T = list(tc.GOOD_TEXTURES), list(tc.BAD_TEXTURES)


def _np(t):
    return t.detach().cpu().numpy()


def _up(a, dtype=None):
    return torch.tensor(np.asarray(a if dtype is None else a.astype(dtype)), device=DEV)


@pytest.fixture(scope="module")
def batch():
    """the kernels' own inputs and outputs through ``ops`` on the cross product and on the six aggregates, and the host
    statement of what the kernels were given: computed once, shared, never written to"""
    from matten_amd import elastic, ops
    from matten_amd import texture as tx

    C = pc.batch()
    tex = tc.textures()
    props = elastic.elastic_properties(C)
    voigt, flags = props.voigt, props.flags
    moduli, vectors, _ = ops.elastic_kelvin(voigt, flags, want_dilatation=False)
    op, tex_flags = tex.operator(DEV)
    cross = tx._device_members(pc.N_BATCH, T, None, DEV)
    aggs = tx._device_members(pc.N_BATCH, T, tc.phases(), DEV)
    out_x, st_x = ops.texture_average(voigt, flags, moduli, vectors, op, tex_flags, *cross[1:4], cross[0])
    out_a, st_a = ops.texture_average(voigt, flags, moduli, vectors, op, tex_flags, *aggs[1:4], aggs[0])
    hv, hf = _np(voigt), _np(flags)
    ref_x = tx.texture_average_host(hv, tex, flags=hf, method="kronecker")
    ref_a = tx.texture_average_host(hv, tex, phases=tc.phases(), flags=hf, method="kronecker")
    return dict(C=C, tex=tex, voigt=voigt, flags=flags, moduli=moduli, vectors=vectors, op=op, tex_flags=tex_flags, cross=cross,
                aggs=aggs, out_x=out_x, st_x=st_x, out_a=out_a, st_a=st_a, ref_x=ref_x, ref_a=ref_a, hv=hv, hf=hf)


def _relative(got, want):
    """per matrix: the largest distance over the largest entry of the reference"""
    return np.abs(got - want).max(axis=(-2, -1)) / np.abs(want).max(axis=(-2, -1))


def test_operator_against_texture_operator_host(batch):
    """Within ten times the distance between the host's longdouble and fp64 sums (floor 1e-14, absolute), with the default
    slice and with slices of 500 (21 slices for the large texture, the last of 7 orientations); flags and NaN operators of
    the three bad textures.  Measured on one MI355X: default slice 1.7e-16, slices of 500 1.4e-16."""
    from matten_amd import ops
    from matten_amd import texture as tx

    tex = batch["tex"]
    ref, ref_flags = tx.texture_operator_host(tex, dtype=np.longdouble)
    f64, _ = tx.texture_operator_host(tex)
    bound = max(10.0 * float(np.abs(ref[GOOD_T] - f64[GOOD_T]).max()), 1e-14)
    print(f"operator: host longdouble against host fp64 {float(np.abs(ref[GOOD_T] - f64[GOOD_T]).max()):.1e}, bound {bound:.1e}")
    R, w, ptr = _up(tex.rotations), _up(tex.weights), _up(tex.ptr)
    small, small_flags = ops.texture_operator(R, w, ptr, slice_len=tc.SMALL_SLICE)
    for name, (op, flags) in (("default slice", (batch["op"], batch["tex_flags"])), (f"slices of {tc.SMALL_SLICE}", (small, small_flags))):
        op, flags = _np(op), _np(flags)
        assert op.shape == (T, 21, 21) and op.dtype == np.float64 and flags.dtype == np.int32
        assert list(flags) == list(ref_flags) == [0, 0, 0, 0, 0, 1, 1, 1]
        assert np.isnan(op[BAD_T]).all() and np.isfinite(op[GOOD_T]).all()
        worst = float(np.abs(op[GOOD_T] - ref[GOOD_T]).max())
        print(f"operator, {name}: {worst:.1e} from the longdouble sum")
        assert worst <= bound, (name, worst)
    # a texture in one slice does not depend on the slice length; the large one moves only within the bound
    assert np.array_equal(_np(small)[GOOD_T[:4]], _np(batch["op"])[GOOD_T[:4]])
    # equal weights through a null pointer: the same bits as explicit ones
    u = tx.Texture.uniform()
    ones = ops.texture_operator(_up(u.rotations), torch.ones(60, dtype=torch.float64, device=DEV), _up(u.ptr))[0]
    assert torch.equal(ops.texture_operator(_up(u.rotations), None, _up(u.ptr))[0], ones)
    assert torch.equal(ones[0], batch["op"][tc.T_UNIFORM])
    # nothing to do
    none = ops.texture_operator(torch.zeros(0, 3, 3, dtype=torch.float64, device=DEV), None, torch.zeros(1, dtype=torch.int64, device=DEV))
    assert none[0].shape == (0, 21, 21) and none[1].shape == (0,)
    empty = ops.texture_operator(torch.zeros(0, 3, 3, dtype=torch.float64, device=DEV), None, torch.zeros(3, dtype=torch.int64, device=DEV))
    assert torch.isnan(empty[0]).all() and empty[1].tolist() == [1, 1]


def test_means_against_texture_average_host(batch):
    """The four means of the cross product and of the six aggregates within TOL of the host (the near-singular row within
    TOL * 1e3), statuses and NaN patterns.  Measured on one MI355X, ordinary rows: voigt 2.8e-15, reuss 7.8e-14,
    hill 3.8e-14, geometric 2.5e-12; the near-singular row: voigt 1.6e-15, reuss 9.4e-11, hill 4.7e-11, geometric 1.6e-12;
    the aggregates: voigt 1.1e-15, reuss 4.0e-15, hill 6.6e-16, geometric 4.6e-15."""
    good_rows = np.ones(pc.N_BATCH, dtype=bool)
    good_rows[[pc.ROW_NOT_PD, pc.ROW_NAN]] = False
    ordinary = good_rows.copy()
    ordinary[pc.ROW_NEAR_SINGULAR] = False
    for got, st, ref, shape in ((batch["out_x"], batch["st_x"], batch["ref_x"], (pc.N_BATCH, T)),
                                (batch["out_a"], batch["st_a"], batch["ref_a"], (6,))):
        got, st = _np(got).reshape(*shape, 4, 6, 6), _np(st).reshape(shape)
        want_st = ref["status"].reshape(shape)
        assert st.dtype == np.int32 and np.array_equal(st, want_st)
        assert np.array_equal(got, np.swapaxes(got, -1, -2), equal_nan=True)          # symmetric, every element written
        for k, name in enumerate(SCHEMES):
            want = ref[name].reshape(*shape, 6, 6)
            has = (st == 0) | ((st == 2) & (k == 0))
            assert np.isfinite(got[..., k, :, :][has]).all() and np.isnan(got[..., k, :, :][~has]).all(), name
            if len(shape) == 2:
                d = _relative(got[..., k, :, :][:, GOOD_T], want[:, GOOD_T])
                ns = float(d[pc.ROW_NEAR_SINGULAR].max())
                rest = float(np.nanmax(d[ordinary]))
                print(f"cross product, {name}: ordinary rows {rest:.1e}, near-singular row {ns:.1e}")
                assert rest <= TOL and ns <= TOL * NEAR_SINGULAR_FACTOR, (name, rest, ns)
                if k == 0:          # voigt of the row that is not positive definite has a value
                    assert float(d[pc.ROW_NOT_PD].max()) <= TOL
            else:
                d = _relative(got[has, k], want[has])
                print(f"aggregates, {name}: {float(d.max()):.1e}")
                assert (d <= TOL).all(), (name, d)
    st = _np(batch["st_x"]).reshape(pc.N_BATCH, T)
    assert (st[:, BAD_T] == -1).all() and (st[pc.ROW_NAN] == -1).all() and (st[pc.ROW_NOT_PD, GOOD_T] == 2).all()
    assert (st[good_rows][:, GOOD_T] == 0).all()
    assert tuple(_np(batch["st_a"])) == tc.AGGREGATE_STATUS


def test_closed_forms_fibre_invariance_and_the_single_orientation(batch):
    """On device output: copper under the icosahedral group is isotropic with the closed-form moduli (1e-12); the fibre
    means do not move under a turn about the fibre axis (1e-13 of the largest entry); one orientation gives the rotated
    tensor in all four means (TOL)."""
    from matten_amd import texture as tx

    out = _np(batch["out_x"]).reshape(pc.N_BATCH, T, 4, 6, 6)
    K, gv, gr, gh, gg = tc.uniform_closed_forms(*pc.COPPER)
    for k, G in enumerate((gv, gr, gh, gg)):
        want = pc.isotropic(K, G)
        assert np.abs(out[pc.ROW_CUBIC, tc.T_UNIFORM, k] - want).max() <= 1e-12 * np.abs(want).max(), SCHEMES[k]
        for t in GOOD_T:          # an isotropic tensor is every texture's fixed point
            iso = batch["C"][pc.ROW_ISOTROPIC]
            assert np.abs(out[pc.ROW_ISOTROPIC, t, k] - iso).max() <= 1e-12 * np.abs(iso).max(), (SCHEMES[k], t)
    Q = pc.rotation_voigt(tx.axis_angle(tc.FIBRE_SAMPLE, 0.7319))
    for b in (pc.ROW_CUBIC, pc.ROW_HEXAGONAL, pc.ROW_TRICLINIC):
        for k in range(4):
            m = out[b, tc.T_FIBRE, k]
            assert np.abs(Q @ m @ Q.T - m).max() <= 1e-13 * np.abs(m).max(), (b, SCHEMES[k])
    Q = pc.rotation_voigt(tc.single_rotation())
    for b in (pc.ROW_CUBIC, pc.ROW_HEXAGONAL, pc.ROW_TRICLINIC, pc.ROW_TRICLINIC + 7):
        want = Q @ batch["hv"][b] @ Q.T
        for k in range(4):
            assert np.abs(out[b, tc.T_SINGLE, k] - want).max() <= TOL * np.abs(want).max(), (b, SCHEMES[k])


def test_voigt_mean_agrees_with_average_irreps(batch):
    """the Voigt mean against the project's other route to it: ``symmetry.average_irreps`` (fp64 rows, one Wigner-D product
    per row and orientation) of the same tensors under the weighted 37 orientations, within TOL.  Measured on one MI355X: 1.3e-15."""
    from matten_amd import elastic, symmetry

    rows = np.r_[0:40, pc.ROW_NEAR_SINGULAR]
    V = elastic.voigt_basis()
    x = batch["hv"][rows].reshape(-1, 36) @ np.linalg.pinv(V)
    assert np.abs(x @ V - batch["hv"][rows].reshape(-1, 36)).max() <= 1e-12 * 300.0          # elasticity tensors: in the span
    R37, w37 = tc.weighted_37()
    avg, _ = symmetry.average_irreps(_up(x), "ijkl=jikl=klij", _up(R37), weights=_up(w37))
    want = (_np(avg) @ V).reshape(-1, 6, 6)
    got = _np(batch["out_x"]).reshape(pc.N_BATCH, T, 4, 6, 6)[rows, tc.T_WEIGHTED, 0]
    d = _relative(got, want)
    print(f"voigt mean against average_irreps: {float(d.max()):.1e}")
    assert (d <= TOL).all()


def test_adjoint_against_texture_average_bwd_host(batch):
    """seeded g_out on the cross product and on the aggregates; within TOL_BWD of the row's largest gradient entry (the
    near-singular row: times 1e3), with asserts of their own for the cubic, isotropic and near-singular rows; parts without
    a value are exact zeros, also when NaN arrives for them; a crystal in several aggregates collects all of them.
    Measured on one MI355X: ordinary rows 9.6e-12, cubic 3.4e-15, isotropic 2.7e-15, near-singular 3.8e-10;
    aggregates 1.0e-14."""
    from matten_amd import ops
    from matten_amd import texture as tx

    rng = np.random.default_rng(8)
    common = (batch["moduli"], batch["vectors"], batch["op"], batch["tex_flags"])
    for name, members, out, st, phases, A in (("cross product", batch["cross"], batch["out_x"], batch["st_x"], None, pc.N_BATCH * T),
                                              ("aggregates", batch["aggs"], batch["out_a"], batch["st_a"], tc.phases(), 6)):
        agg_ptr, mc, mt, mf, crystal_ptr, crystal_member = members
        g = rng.standard_normal((A, 4, 6, 6))
        args = (*common, mc, mt, mf, agg_ptr, out, st)
        got = ops.texture_average_bwd(*args, _up(g), crystal_ptr, crystal_member)
        assert torch.equal(got, ops.texture_average_bwd(*args, _up(g), crystal_ptr, crystal_member))
        got = _np(got)
        want = tx.texture_average_bwd_host(batch["hv"], batch["tex"], g, phases=phases, flags=batch["hf"])
        assert got.shape == (pc.N_BATCH, 6, 6) and np.array_equal(got, got.transpose(0, 2, 1))
        assert (got[pc.ROW_NAN] == 0.0).all() and (want[pc.ROW_NAN] == 0.0).all()
        touched = np.abs(want).max(axis=(1, 2)) > 0
        assert (got[~touched] == 0.0).all()          # every element written, also of crystals without a member
        d = np.abs(got - want).max(axis=(1, 2))[touched] / np.abs(want).max(axis=(1, 2))[touched]
        d_of = dict(zip(np.nonzero(touched)[0], d))
        rest = max(v for r, v in d_of.items() if r != pc.ROW_NEAR_SINGULAR)
        print(f"adjoint, {name}: ordinary rows {rest:.1e}" + "".join(
            f", {label} {d_of[r]:.1e}" for label, r in (("cubic", pc.ROW_CUBIC), ("isotropic", pc.ROW_ISOTROPIC),
                                                       ("near-singular", pc.ROW_NEAR_SINGULAR)) if r in d_of))
        assert rest <= TOL_BWD
        assert d_of[pc.ROW_CUBIC] <= TOL_BWD and d_of[pc.ROW_ISOTROPIC] <= TOL_BWD          # degenerate moduli: 1, 2, 3 and 1, 5
        if phases is None:
            assert d_of[pc.ROW_NEAR_SINGULAR] <= TOL_BWD * NEAR_SINGULAR_FACTOR
            assert pc.ROW_NOT_PD in d_of          # its voigt parts flow
        else:
            # the cubic row is a member of five of the six aggregates, of which two have a value: both arrive
            one = np.zeros_like(g)
            one[0] = g[0]
            only0 = _np(ops.texture_average_bwd(*args, _up(one), crystal_ptr, crystal_member))
            one = np.zeros_like(g)
            one[1] = g[1]
            only1 = _np(ops.texture_average_bwd(*args, _up(one), crystal_ptr, crystal_member))
            assert np.abs(only0[pc.ROW_CUBIC]).max() > 0 and np.abs(only1[pc.ROW_CUBIC]).max() > 0
            assert np.abs(only0[pc.ROW_CUBIC] + only1[pc.ROW_CUBIC] - got[pc.ROW_CUBIC]).max() <= 1e-14 * np.abs(got[pc.ROW_CUBIC]).max()
            # status 2: only the voigt part flows; status -1: nothing, whatever arrives
            poison = np.zeros_like(g)
            poison[2, 1:] = np.nan
            poison[3:] = np.nan
            z = _np(ops.texture_average_bwd(*args, _up(poison), crystal_ptr, crystal_member))
            assert (z == 0.0).all()
            poison[2, 0] = 1.0
            z = _np(ops.texture_average_bwd(*args, _up(poison), crystal_ptr, crystal_member))
            assert np.isfinite(z).all() and np.abs(z[pc.ROW_NOT_PD]).max() > 0 and np.abs(z[pc.ROW_ISOTROPIC]).max() > 0
            assert (z[pc.ROW_CUBIC] == 0.0).all() and (z[pc.ROW_HEXAGONAL] == 0.0).all()


def _host_y_mod(C):
    """Young's modulus of the Hill average of a Voigt matrix [..,6,6]: 9 K G / (3 K + G) of the Voigt-Reuss-Hill pair"""
    S = np.linalg.inv(C)
    tr = lambda A, idx: sum(A[..., i, i] for i in idx)      # noqa: E731
    off = lambda A: A[..., 0, 1] + A[..., 0, 2] + A[..., 1, 2]      # noqa: E731
    kv, kr = C[..., :3, :3].sum(axis=(-2, -1)) / 9.0, 1.0 / S[..., :3, :3].sum(axis=(-2, -1))
    gv = (tr(C, (0, 1, 2)) - off(C) + 3.0 * tr(C, (3, 4, 5))) / 15.0
    gr = 15.0 / (4.0 * tr(S, (0, 1, 2)) - 4.0 * off(S) + 3.0 * tr(S, (3, 4, 5)))
    K, G = 0.5 * (kv + kr), 0.5 * (gv + gr)
    return 9.0 * K * G / (3.0 * K + G)


def test_end_to_end_gradient_against_central_differences(batch):
    """``elastic_moduli(texture_average(C).hill).y_mod.sum().backward()`` to the leaf C [5,6,6] (isotropic, cubic x 2,
    hexagonal, one triclinic; fibre and weighted textures) against central differences of the host chain at h = 1e-5 max|C|:
    1e-6 of the largest gradient entry, the finite-difference error.  Measured on one MI355X: 2.4e-9; the value 2.2e-16."""
    from matten_amd import elastic
    from matten_amd import texture as tx

    C = batch["C"][:5].copy()
    R37, w37 = tc.weighted_37()
    tex = tx.Texture.stack([tx.Texture.fibre(tc.FIBRE_CRYSTAL, tc.FIBRE_SAMPLE, 5), tx.Texture(R37, w37)])

    def value(Cx):
        return _host_y_mod(tx.texture_average_host(Cx, tex, method="kronecker")["hill"]).sum()

    want = np.zeros_like(C)
    for b in range(len(C)):
        h = 1e-5 * np.abs(C[b]).max()
        for i in range(6):
            for j in range(i, 6):
                E = np.zeros_like(C)
                E[b, i, j] = E[b, j, i] = h
                want[b, i, j] = want[b, j, i] = (value(C + E) - value(C - E)) / (2.0 * h) / (1.0 if i == j else 2.0)
    leaf = _up(C).requires_grad_()
    avg = tx.texture_average(leaf, tex)
    assert avg.hill.shape == (5, 2, 6, 6) and avg.hill.requires_grad and not avg.status.requires_grad
    y = elastic.elastic_moduli(avg.hill.reshape(-1, 6, 6)).y_mod.sum()
    y.backward()
    got = _np(leaf.grad)
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"end to end: value off by {abs(y.item() / value(C) - 1.0):.1e}, gradient off by {err:.1e} of its largest entry")
    assert abs(y.item() / value(C) - 1.0) <= 1e-12 and err <= 1e-6
    # the same through ModuliLoss, and the irreps front end trains too
    loss = elastic.ModuliLoss(("y_mod",))(elastic.elastic_moduli(tx.texture_average(leaf, tex).hill.reshape(-1, 6, 6)),
                                         {"y_mod": torch.zeros(10, device=DEV)})
    assert abs(loss.item() / (value(C) / 10.0) - 1.0) <= 1e-12


def test_public_interface(batch):
    """``texture_average`` on arrays, lists with holes, single tensors, Cartesian input and explicit phases gives the kernels'
    bits; ``texture_average_from_irreps`` the bits of ``texture_average`` on the Voigt matrices ``dense_rows`` makes"""
    from matten_amd import elastic, ops
    from matten_amd import texture as tx

    tex = batch["tex"]
    full = tx.texture_average(batch["C"], tex)
    out = batch["out_x"].reshape(pc.N_BATCH, T, 4, 6, 6)
    for k, name in enumerate(SCHEMES):
        assert getattr(full, name).shape == (pc.N_BATCH, T, 6, 6)
        assert np.array_equal(_np(getattr(full, name)), _np(out[:, :, k]), equal_nan=True), name
        assert full.tensor(name) is getattr(full, name)
    assert torch.equal(full.status, batch["st_x"].reshape(pc.N_BATCH, T)) and full.status.dtype == torch.int32
    assert full.cartesian("reuss").shape == (pc.N_BATCH, T, 3, 3, 3, 3)
    assert torch.equal(full.cartesian("voigt")[3, 1, 0, 1, 0, 1], full.voigt[3, 1, 5, 5])
    aggs = tx.texture_average(batch["C"], tex, phases=tc.phases())
    assert aggs.hill.shape == (6, 6, 6) and np.array_equal(_np(aggs.hill), _np(batch["out_a"][:, 2]), equal_nan=True)
    assert tuple(aggs.status.tolist()) == tc.AGGREGATE_STATUS
    one = tx.texture_average(batch["C"][pc.ROW_HEXAGONAL], tex)
    assert one.geometric.shape == (T, 6, 6) and one.status.shape == (T,)
    assert np.array_equal(_np(one.geometric), _np(full.geometric[pc.ROW_HEXAGONAL]), equal_nan=True)
    cart = elastic.voigt_to_cartesian(batch["C"][:4])
    assert np.array_equal(_np(tx.texture_average(cart, tex).hill), _np(full.hill[:4]), equal_nan=True)
    holes = tx.texture_average([batch["C"][1], None, batch["C"][3]], tex)          # what predict returns for a failed structure
    assert (holes.status[1] == -1).all() and torch.isnan(holes.voigt[1]).all()
    assert np.array_equal(_np(holes.hill[[0, 2]]), _np(full.hill[[1, 3]]), equal_nan=True)
    # directional Young's modulus of a sheet in one call
    sheet = tx.texture_average(batch["C"][pc.ROW_CUBIC], tx.Texture.fibre(tc.FIBRE_CRYSTAL, tc.FIBRE_SAMPLE)).properties(
        "hill", directions=np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]), keep_directional=True)
    young = _np(sheet.young)[0]
    assert abs(young[0] / young[1] - 1.0) <= 1e-12 and young[2] > young[0] * 1.05          # <111> fibre: stiff along the axis
    # the irreps front end
    V = elastic.voigt_basis()
    x = torch.from_numpy(batch["C"][:8].reshape(8, 36) @ np.linalg.pinv(V)).float().to(DEV)
    rows = ops.dense_rows(x, torch.tensor(V, dtype=torch.float32, device=DEV)).reshape(8, 6, 6)
    a, b = tx.texture_average_from_irreps(x, tex), tx.texture_average(rows, tex)
    for name in SCHEMES:
        assert np.array_equal(_np(getattr(a, name)), _np(getattr(b, name)), equal_nan=True), name
    assert torch.equal(a.status, b.status)
    xg = x.clone().requires_grad_()
    tx.texture_average_from_irreps(xg, tex).hill[:, GOOD_T].sum().backward()
    assert xg.grad.shape == (8, 21) and xg.grad.dtype == torch.float32 and torch.isfinite(xg.grad).all() and xg.grad.abs().max() > 0
    with pytest.raises(ValueError, match="Texture"):
        tx.texture_average(batch["C"], (tex.rotations, None, tex.ptr))


def test_bits_repeat_and_empty_inputs(batch):
    """two runs of every kernel give the same bits; A = 0, M = 0 and n = 0 are no-ops"""
    from matten_amd import ops

    tex = batch["tex"]
    again = ops.texture_operator(_up(tex.rotations), _up(tex.weights), _up(tex.ptr))
    assert np.array_equal(_np(again[0]), _np(batch["op"]), equal_nan=True) and torch.equal(again[1], batch["tex_flags"])
    common = (batch["voigt"], batch["flags"], batch["moduli"], batch["vectors"], batch["op"], batch["tex_flags"])
    for members, out, st in ((batch["cross"], batch["out_x"], batch["st_x"]), (batch["aggs"], batch["out_a"], batch["st_a"])):
        o2, s2 = ops.texture_average(*common, *members[1:4], members[0])
        assert np.array_equal(_np(o2), _np(out), equal_nan=True) and torch.equal(s2, st)
    i32, i64, f64 = (lambda n, dt=dt: torch.zeros(n, dtype=dt, device=DEV) for dt in (torch.int32, torch.int64, torch.float64))
    out, st = ops.texture_average(*common, i32(0), i32(0), f64(0), i64(1))
    assert out.shape == (0, 4, 6, 6) and st.shape == (0,)
    out, st = ops.texture_average(*common, i32(0), i32(0), f64(0), i64(3))          # two empty aggregates
    assert st.tolist() == [-1, -1] and torch.isnan(out).all()
    g = ops.texture_average_bwd(*common[2:], i32(0), i32(0), f64(0), i64(3), out, st, torch.ones_like(out), i64(pc.N_BATCH + 1), i32(0))
    assert g.shape == (pc.N_BATCH, 6, 6) and (g == 0.0).all()
    e = torch.zeros(0, 6, 6, dtype=torch.float64, device=DEV)
    g = ops.texture_average_bwd(f64(0).reshape(0, 6), e, batch["op"], batch["tex_flags"], i32(0), i32(0), f64(0), i64(1),
                                torch.zeros(0, 4, 6, 6, dtype=torch.float64, device=DEV), i32(0),
                                torch.zeros(0, 4, 6, 6, dtype=torch.float64, device=DEV), i64(1), i32(0))
    assert g.shape == (0, 6, 6)
