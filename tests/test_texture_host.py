"""
CPU tests of the textured-polycrystal means (matten_amd/texture.py over csrc/texture.hip): the numpy statements
``texture_operator_host`` / ``texture_average_host`` / ``texture_average_bwd_host`` against closed forms, invariances, the
Loewner order and central differences; the ``Texture`` constructors and their validation; the library's three entries
(declared, bound, exported, bad arguments refused without a device).  The GPU tests (tests/test_gpu_texture.py) hold the
kernels to the statements tested here; both share tests/texture_cases.py.

The adjoint against central differences.  Step FD_STEP = 1e-6 max|C| on one symmetric pair of entries.  The means go
through an inverse and a logarithm, whose third derivative against the first grows as 1 / l_min^2: truncation is
(step / l_min)^2 = (1e-6 * condition)^2, rounding eps * condition / 1e-6.  The rows used have condition numbers up to ~200:
4e-8 and 2e-8.  FD_TOL = 2e-7 of the largest entry of the row's gradient; measured on this file's rows: 5.9e-9.
"""
import os
import re

import numpy as np
import pytest

import polycrystal_cases as pc
import texture_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FD_STEP, FD_TOL = 1e-6, 2e-7
SCHEMES = ("voigt", "reuss", "hill", "geometric")


def mandel(C):
    from matten_amd import elastic

    return elastic.MANDEL_WEIGHT * C


def unmandel(X):
    from matten_amd import elastic

    return elastic.MANDEL_UNWEIGHT * X


def rotated(C, R):
    Q = pc.rotation_voigt(R)
    return Q @ C @ Q.T


# ----------------------------------------------------------------------------------------------------------------------
# closed forms and invariances
# ----------------------------------------------------------------------------------------------------------------------
def test_uniform_texture_gives_the_isotropic_closed_forms():
    """copper under the 60 icosahedral rotations: K in all four means, the closed-form shear moduli, isotropic: 1e-12"""
    from matten_amd import texture as tx

    u = tx.Texture.uniform()
    assert len(u) == 1 and u.rotations.shape == (60, 3, 3) and np.allclose(u.rotations[0], np.eye(3))
    assert np.abs(np.linalg.det(u.rotations) - 1.0).max() < 1e-12
    K, gv, gr, gh, gg = tc.uniform_closed_forms(*pc.COPPER)
    for method in ("congruence", "kronecker"):
        r = tx.texture_average_host(pc.cubic(*pc.COPPER), u, method=method)
        assert list(r["status"]) == [0]
        for name, G in zip(SCHEMES, (gv, gr, gh, gg)):
            want = pc.isotropic(K, G)
            assert np.abs(r[name][0] - want).max() <= 1e-12 * np.abs(want).max(), (method, name)


def test_fibre_is_exact_from_five_turns():
    """fibre(n=5): every mean is invariant under an arbitrary turn about the fibre axis, to 1e-13 of the largest entry;
    four turns are not enough (and are refused)"""
    from matten_amd import texture as tx

    C = np.stack([pc.cubic(*pc.COPPER), pc.batch()[pc.ROW_TRICLINIC]])
    turn = tx.axis_angle(tc.FIBRE_SAMPLE, 0.7319)
    for n in (5, 12):
        f = tx.Texture.fibre(tc.FIBRE_CRYSTAL, tc.FIBRE_SAMPLE, n)
        assert f.rotations.shape == (n, 3, 3)
        axis = f.rotations @ (np.ones(3) / np.sqrt(3.0))
        assert np.abs(axis - np.array(tc.FIBRE_SAMPLE)).max() < 1e-14          # [111] of every grain along the sample axis
        r = tx.texture_average_host(C, f)
        for name in SCHEMES:
            for b in range(2):
                assert np.abs(rotated(r[name][b], turn) - r[name][b]).max() <= 1e-13 * np.abs(r[name][b]).max(), (n, name, b)
    four = tx.Texture(tx.axis_angle(tc.FIBRE_SAMPLE, 2.0 * np.pi * np.arange(4) / 4) @ tx.rotation_between(tc.FIBRE_CRYSTAL,
                                                                                                          tc.FIBRE_SAMPLE))
    v = tx.texture_average_host(C[1], four)["voigt"][0]          # (the triclinic row: a cubic crystal's own triad would help)
    assert np.abs(rotated(v, turn) - v).max() > 1e-3 * np.abs(v).max()
    with pytest.raises(ValueError, match="n"):
        tx.Texture.fibre(tc.FIBRE_CRYSTAL, tc.FIBRE_SAMPLE, 4)


def test_single_orientation_rotates_and_identity_returns_the_input():
    """one orientation: all four means are the rotated tensor (also for an improper matrix, which acts like its negative);
    the identity returns the input.  1e-12 of the largest entry (an inverse and a logarithm taken and undone at condition
    numbers of a few hundred)."""
    from matten_amd import texture as tx

    C = pc.batch()[[pc.ROW_CUBIC, pc.ROW_HEXAGONAL, pc.ROW_TRICLINIC, pc.ROW_TRICLINIC + 1]]
    R = tc.single_rotation()
    for M, acts_as in ((R, R), (-R, R), (np.eye(3), np.eye(3))):
        r = tx.texture_average_host(C, tx.Texture.single(M))
        for name in SCHEMES:
            assert r[name].shape == (4, 6, 6)
            for b in range(len(C)):
                want = rotated(C[b], acts_as)
                assert np.abs(r[name][b] - want).max() <= 1e-12 * np.abs(want).max(), (name, b)


def test_geometric_mean_of_the_compliance_is_the_inverse():
    """Matthies & Humbert: geometric(C)^-1 == geometric(S), here on Mandel matrices; 1e-11 relative (eps x condition x 10)"""
    from matten_amd import texture as tx

    C = pc.batch()[pc.ROW_CUBIC:pc.ROW_TRICLINIC + 6]
    R37, w37 = tc.weighted_37()
    t = tx.Texture(R37, w37)
    S_as_voigt = unmandel(np.linalg.inv(mandel(C)))
    gC = mandel(tx.texture_average_host(C, t)["geometric"])
    gS = mandel(tx.texture_average_host(S_as_voigt, t)["geometric"])
    for b in range(len(C)):
        assert np.abs(gC[b] @ gS[b] - np.eye(6)).max() <= 1e-11, b


def test_loewner_order_reuss_geometric_voigt():
    """reuss <= geometric <= voigt (and reuss <= hill <= voigt) in the Loewner order on the 250 seeded triclinic tensors under
    the weighted 37-orientation texture: the smallest eigenvalue of each difference is >= -1e-12 of the largest modulus"""
    from matten_amd import texture as tx

    C = pc.batch()[pc.ROW_TRICLINIC:pc.ROW_NEAR_SINGULAR]
    assert len(C) == 250
    R37, w37 = tc.weighted_37()
    r = tx.texture_average_host(C, tx.Texture(R37, w37), method="kronecker")
    assert (r["status"] == 0).all()
    top = np.linalg.eigvalsh(mandel(r["voigt"]))[:, 5]
    strict = 0
    for lo, hi in (("reuss", "geometric"), ("geometric", "voigt"), ("reuss", "hill"), ("hill", "voigt")):
        gap = np.linalg.eigvalsh(mandel(r[hi]) - mandel(r[lo]))
        assert (gap[:, 0] >= -1e-12 * top).all(), (lo, hi)
        strict += int((gap[:, 5] > 1e-6 * top).all())
    assert strict == 4          # and they are different tensors


def test_operator_is_the_average_on_the_upper_triangle():
    from matten_amd import texture as tx

    R, w, ptr = tc.packed()
    op, flags = tx.texture_operator_host((R, w, ptr))
    assert op.shape == (8, 21, 21) and list(flags) == [0, 0, 0, 0, 0, 1, 1, 1]
    assert np.isnan(op[list(tc.BAD_TEXTURES)]).all() and np.isfinite(op[list(tc.GOOD_TEXTURES)]).all()
    X = mandel(pc.batch()[pc.ROW_TRICLINIC])
    tri = np.array([X[i, j] for i in range(6) for j in range(i, 6)])
    for t in tc.GOOD_TEXTURES[:4]:
        N = tx.rotation_mandel(R[ptr[t]:ptr[t + 1]])
        assert np.abs(N @ N.transpose(0, 2, 1) - np.eye(6)).max() <= 1e-14          # N is orthogonal
        wt = w[ptr[t]:ptr[t + 1]] / w[ptr[t]:ptr[t + 1]].sum()
        want = np.einsum("g,gik,kl,gjl->ij", wt, N, X, N)
        got = op[t] @ tri
        assert np.abs(got - np.array([want[i, j] for i in range(6) for j in range(i, 6)])).max() <= 1e-13 * np.abs(X).max(), t
    # Bond's matrix: N = D Q D^-1 with the Q of the polycrystal cases
    d = np.array([1.0, 1.0, 1.0] + [np.sqrt(2.0)] * 3)
    assert np.abs(tx.rotation_mandel(R[1])[0] - d[:, None] * pc.rotation_voigt(R[1]) / d[None, :]).max() <= 1e-15
    lo, _ = tx.texture_operator_host((R[:100], None, np.array([0, 100])), dtype=np.longdouble)
    assert lo.dtype == np.longdouble


def test_statuses_and_nan_patterns():
    from matten_amd import texture as tx

    r = tx.texture_average_host(pc.batch(), tc.textures(), phases=tc.phases())
    assert tuple(r["status"]) == tc.AGGREGATE_STATUS
    for a, st in enumerate(tc.AGGREGATE_STATUS):
        assert np.isfinite(r["voigt"][a]).all() == (st != -1), a
        for name in SCHEMES[1:]:
            assert np.isfinite(r[name][a]).all() == (st == 0) and (st == 0 or np.isnan(r[name][a]).all()), (a, name)
    # fractions are normalised per aggregate, a zero-fraction member changes nothing
    two = tx.texture_average_host(pc.batch(), tc.textures(), phases=(np.array([0, 2]), np.array([pc.ROW_CUBIC, pc.ROW_TRICLINIC]),
                                                                     np.array([tc.T_UNIFORM, tc.T_SINGLE]), np.array([4.0, 2.0])))
    for name in SCHEMES:
        assert np.abs(two[name][0] - r[name][1]).max() <= 1e-12 * np.abs(two[name][0]).max(), name
    # flags: bit 0 gives -1, bit 1 gives 2
    fl = np.zeros(pc.N_BATCH, dtype=np.int32)
    fl[pc.ROW_CUBIC], fl[pc.ROW_HEXAGONAL] = 1, 2
    cross = tx.texture_average_host(pc.batch()[:5], tc.textures(), flags=fl[:5])
    st = cross["status"].reshape(5, 8)
    assert (st[:, list(tc.BAD_TEXTURES)] == -1).all() and (st[pc.ROW_CUBIC] == -1).all()
    assert (st[pc.ROW_HEXAGONAL, list(tc.GOOD_TEXTURES)] == 2).all() and (st[pc.ROW_ISOTROPIC, list(tc.GOOD_TEXTURES)] == 0).all()
    with pytest.raises(ValueError, match="phases"):
        tx.texture_average_host(pc.batch()[:5], tc.textures(), phases=(np.array([0, 3]), np.zeros(2), np.zeros(2), np.ones(2)))


# ----------------------------------------------------------------------------------------------------------------------
# the adjoint
# ----------------------------------------------------------------------------------------------------------------------
def test_adjoint_against_central_differences():
    """four rows -- triclinic, cubic (moduli of multiplicity 1, 2, 3), isotropic (1, 5), hexagonal -- under two textures, in
    the cross product and in a two-phase aggregate that shares a crystal with it"""
    from matten_amd import texture as tx

    C = pc.batch()[[pc.ROW_TRICLINIC, pc.ROW_CUBIC, pc.ROW_ISOTROPIC, pc.ROW_HEXAGONAL]]
    R37, w37 = tc.weighted_37()
    tex = tx.Texture.stack([tx.Texture(R37[:9], w37[:9]), tx.Texture.fibre(tc.FIBRE_CRYSTAL, tc.FIBRE_SAMPLE, 5)])
    rng = np.random.default_rng(3)
    worst = 0.0
    for phases in (None, (np.array([0, 2, 3]), np.array([1, 0, 1]), np.array([0, 1, 1]), np.array([0.3, 0.9, 1.0]))):
        A = 8 if phases is None else 2
        g = rng.standard_normal((A, 4, 6, 6))
        got = tx.texture_average_bwd_host(C, tex, g, phases=phases)
        assert got.shape == (4, 6, 6) and np.array_equal(got, got.transpose(0, 2, 1))

        def value(Cx):
            r = tx.texture_average_host(Cx, tex, phases=phases)
            return sum((g[:, k] * r[name]).sum() for k, name in enumerate(SCHEMES))

        rows = range(4) if phases is None else (0, 1)
        if phases is not None:
            assert (got[2:] == 0.0).all()
        for b in rows:
            h = FD_STEP * np.abs(C[b]).max()
            for i in range(6):
                for j in range(i, 6):
                    E = np.zeros_like(C)
                    E[b, i, j] = E[b, j, i] = h
                    fd = (value(C + E) - value(C - E)) / (2.0 * h)
                    an = got[b, i, j] * (1.0 if i == j else 2.0)
                    worst = max(worst, abs(fd - an) / np.abs(got[b]).max())
    print(f"adjoint vs central differences: {worst:.2e} of the row's largest entry")
    assert worst <= FD_TOL


def test_adjoint_parts_without_a_value_are_zero():
    from matten_amd import texture as tx

    C = pc.batch()
    g = np.ones((6, 4, 6, 6))
    got = tx.texture_average_bwd_host(C, tc.textures(), g, phases=tc.phases())
    assert np.abs(got[pc.ROW_CUBIC]).max() > 0 and np.abs(got[pc.ROW_TRICLINIC]).max() > 0
    assert (got[pc.ROW_NAN] == 0.0).all()
    # the status-2 aggregate: only its voigt part flows, to both members
    only_voigt = np.zeros((6, 4, 6, 6))
    only_voigt[2, 0] = 1.0
    a = tx.texture_average_bwd_host(C, tc.textures(), only_voigt, phases=tc.phases())
    others = np.zeros((6, 4, 6, 6))
    others[2, 1:] = 1.0
    b = tx.texture_average_bwd_host(C, tc.textures(), others, phases=tc.phases())
    assert np.abs(a[pc.ROW_NOT_PD]).max() > 0 and np.abs(a[pc.ROW_ISOTROPIC]).max() > 0 and (b == 0.0).all()


# ----------------------------------------------------------------------------------------------------------------------
# Texture: constructors and validation
# ----------------------------------------------------------------------------------------------------------------------
def test_bunge_convention_on_a_hand_worked_orientation():
    """phi1 = 90 degrees, Phi = phi2 = 0: Bunge's g (sample -> crystal) is [[0,1,0],[-1,0,0],[0,0,1]]; the crystal is turned
    by +90 degrees about z, its x axis lies along the sample's y: R = g^T"""
    from matten_amd import texture as tx

    t = tx.Texture.from_bunge(90.0, 0.0, 0.0)
    want = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    assert np.abs(t.rotations[0] - want).max() <= 1e-15
    assert np.abs(t.rotations[0] @ np.array([1.0, 0.0, 0.0]) - np.array([0.0, 1.0, 0.0])).max() <= 1e-15
    # Phi about the turned x axis: (phi1, Phi, phi2) = (0, 90, 0) takes crystal z to sample -y
    t = tx.Texture.from_bunge([0.0], [np.pi / 2], [0.0], degrees=False)
    assert np.abs(t.rotations[0] @ np.array([0.0, 0.0, 1.0]) - np.array([0.0, -1.0, 0.0])).max() <= 1e-15
    many = tx.Texture.from_bunge([10.0, 20.0, 30.0], [40.0, 50.0, 60.0], [70.0, 80.0, 90.0], weights=[1.0, 2.0, 3.0])
    assert many.rotations.shape == (3, 3, 3) and np.abs(np.linalg.det(many.rotations) - 1.0).max() < 1e-14


def test_constructors():
    from matten_amd import texture as tx

    a = tx.Texture.scatter(np.eye(3), 10.0, 50, seed=4)
    b = tx.Texture.scatter(np.eye(3), 10.0, 50, seed=4)
    assert np.array_equal(a.rotations, b.rotations) and a.rotations.shape == (50, 3, 3)
    angle = np.degrees(np.arccos(np.clip((np.trace(a.rotations, axis1=1, axis2=2) - 1.0) / 2.0, -1.0, 1.0)))
    assert 5.0 < angle.mean() < 30.0 and np.abs(a.rotations @ a.rotations.transpose(0, 2, 1) - np.eye(3)).max() < 1e-14
    assert np.array_equal(tx.Texture.scatter(np.eye(3), 0.0, 3, seed=1).rotations, np.stack([np.eye(3)] * 3))
    f = tx.Texture.fibre((0, 0, 1), (0, 0, -1), 6)          # antiparallel axes
    assert np.abs(f.rotations @ np.array([0.0, 0.0, 1.0]) - np.array([0.0, 0.0, -1.0])).max() < 1e-14
    mixed = tx.Texture.mix([tx.Texture.uniform(), tx.Texture.single(np.eye(3))], [3.0, 1.0])
    assert len(mixed) == 1 and mixed.rotations.shape == (61, 3, 3)
    assert abs(mixed.weights[:60].sum() - 3.0) < 1e-14 and mixed.weights[60] == 1.0
    C = pc.cubic(*pc.COPPER)
    v = tx.texture_average_host(C, mixed)["voigt"][0]
    K, gv, *_ = tc.uniform_closed_forms(*pc.COPPER)
    assert np.abs(v - (0.75 * pc.isotropic(K, gv) + 0.25 * C)).max() <= 1e-12 * np.abs(C).max()
    stacked = tx.Texture.stack([tx.Texture.uniform(), a, mixed])
    assert len(stacked) == 3 and list(stacked.sizes) == [60, 50, 61] and stacked.weights.shape == (171,)
    assert len(tx.Texture.stack([a, b])) == 2 and tx.Texture.stack([a, b]).weights is None
    with pytest.raises(ValueError):
        stacked.rotations[0, 0, 0] = 2.0          # read-only: the operator is cached


def test_constructor_validation():
    from matten_amd import texture as tx

    R = tc.random_rotations(4, 2)
    sheared = R.copy()
    sheared[2, 0, 1] += 1e-3
    nan = R.copy()
    nan[1, 1, 1] = np.nan
    for args, match in (((sheared,), "orthogonal"), ((nan,), "finite"), ((R, [1.0, 1.0, 1.0]), "weights"),
                        ((R, [1.0, -1.0, 1.0, 1.0]), "weights"), ((R, [1.0, np.inf, 1.0, 1.0]), "weights"),
                        ((R, [0.0, 0.0, 1.0, 1.0], [0, 2, 4]), "weight sum"), ((R, None, [0, 2, 2, 4]), "empty"),
                        ((R, None, [0, 2, 3]), "ptr"), ((R, None, [1, 4]), "ptr"), ((R, None, [0, 3, 2, 4]), "ptr"),
                        ((np.zeros((4, 2, 3)),), "rotations"), ((np.zeros((0, 3, 3)),), "empty")):
        with pytest.raises(ValueError, match=match):
            tx.Texture(*args)
    assert len(tx.Texture(sheared, validate=False)) == 1          # left to the device's flags
    with pytest.raises(ValueError, match="R"):
        tx.Texture.single(R)
    for n in (4, 0, 5.0, True):
        with pytest.raises(ValueError, match="n"):
            tx.Texture.fibre((1, 0, 0), (0, 0, 1), n)
    with pytest.raises(ValueError, match="crystal_axis"):
        tx.Texture.fibre((0, 0, 0), (0, 0, 1))
    with pytest.raises(ValueError, match="sigma_deg"):
        tx.Texture.scatter(np.eye(3), -1.0, 5, seed=0)
    with pytest.raises(ValueError, match="n"):
        tx.Texture.scatter(np.eye(3), 1.0, 0, seed=0)
    with pytest.raises(ValueError, match="one length"):
        tx.Texture.from_bunge([0.0, 1.0], [0.0], [0.0])
    with pytest.raises(ValueError, match="fractions"):
        tx.Texture.mix([tx.Texture.uniform()], [0.0])
    with pytest.raises(ValueError, match="mix"):
        tx.Texture.mix([tx.Texture.stack([tx.Texture.uniform(), tx.Texture.uniform()])], [1.0])
    with pytest.raises(ValueError, match="scheme"):
        tx.TextureAverage(None, None, None, None, None).tensor("kroener")
    with pytest.raises(ValueError, match="Texture"):          # before anything touches a device
        tx._average_rows(None, 1, False, None, (R, None, [0, 4]), None, False)


# ----------------------------------------------------------------------------------------------------------------------
# the library
# ----------------------------------------------------------------------------------------------------------------------
ENTRIES = ("matten_texture_operator", "matten_texture_average", "matten_texture_average_bwd")


def test_library_declares_binds_and_exports_the_entries():
    from matten_amd import _lib, autograd, ops

    header = open(os.path.join(ROOT, "include", "matten_hip.h")).read()
    declared = set(re.findall(r"\b(matten_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for name in ENTRIES:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.matten_abi_version() == _lib.ABI_VERSION == 47          # entries were only added
    assert [len(_lib.SIGNATURES[n][1]) for n in ENTRIES] == [12, 17, 20]
    makefile = open(os.path.join(ROOT, "matten_amd", "csrc", "Makefile")).read()
    assert "texture.hip" in makefile
    source = open(os.path.join(ROOT, "matten_amd", "csrc", "texture.hip")).read()
    assert '#include "sym6.h"' in source and "atomic" not in source.replace("no atomics", "")
    for name in ("texture_operator", "texture_average", "texture_average_bwd"):
        assert callable(getattr(ops, name))
    assert hasattr(autograd, "TextureAverageFn")


def test_bad_arguments_come_back_without_a_device():
    from matten_amd import _lib

    lib = _lib.load()
    operator, fwd, bwd = (getattr(lib, n) for n in ENTRIES)
    p = 4096      # never dereferenced: every call below returns from the checks
    too_many = (2 ** 31 - 1) * 64 + 1
    # no-ops
    assert operator(None, None, None, 0, 0, 1e-6, 1024, None, 0, None, None, None) == 0
    assert fwd(None, None, None, None, 0, None, None, 0, None, None, None, 0, None, 0, None, None, None) == 0
    assert bwd(None, None, 0, None, 0, None, None, None, 0, None, 0, None, None, None, None, None, None, 0, None, None) == 0
    good = [p, p, p, 100, 2, 1e-6, 64, p, 2 * 2 * 448, p, p, None]
    for k, value in ((3, -1), (4, -1), (4, 2 ** 31), (5, -1e-6), (5, float("nan")), (5, float("inf")), (6, 0), (6, -5),
                     (0, None), (2, None), (9, None), (10, None)):
        args = list(good)
        args[k] = value
        assert operator(*args) == -1, (k, value)
    for k, value in ((7, None), (8, 2 * 2 * 448 - 1)):          # the workspace: MATTEN_ENOMEM
        args = list(good)
        args[k] = value
        assert operator(*args) == -3, (k, value)
    good = [p, p, p, p, 5, p, p, 2, p, p, p, 10, p, 10, p, p, None]
    for k, value in ((4, -1), (4, too_many), (7, -1), (7, 2 ** 31), (11, -1), (11, too_many), (13, -1), (13, too_many),
                     (0, None), (1, None), (2, None), (3, None), (5, None), (6, None), (8, None), (9, None), (10, None),
                     (12, None), (14, None), (15, None)):
        args = list(good)
        args[k] = value
        assert fwd(*args) == -1, (k, value)
    good = [p, p, 5, p, 2, p, p, p, 10, p, 10, p, p, p, p, p, p, 10 * 64 + 10 * 21, p, None]
    for k, value in ((2, -1), (2, too_many), (4, -1), (8, -1), (8, too_many), (10, -1), (10, too_many), (0, None), (1, None),
                     (3, None), (5, None), (6, None), (7, None), (9, None), (11, None), (12, None), (13, None), (14, None),
                     (15, None), (18, None)):
        args = list(good)
        args[k] = value
        assert bwd(*args) == -1, (k, value)
    for k, value in ((16, None), (17, 10 * 64 + 10 * 21 - 1)):
        args = list(good)
        args[k] = value
        assert bwd(*args) == -3, (k, value)
