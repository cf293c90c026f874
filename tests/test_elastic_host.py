"""
CPU tests of the derived-elastic-properties module (matten_amd/elastic.py): the irreps -> Voigt basis, the direction sets
and their validation, and the two C entries' declarations and bindings.  No kernel is launched.
"""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# pymatgen's Voigt order: xx, yy, zz, yz, xz, xy
PAIRS = ((0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1))


def voigt_picks(c4):
    return np.array([[c4[i, j, k, l] for (k, l) in PAIRS] for (i, j) in PAIRS])


def test_voigt_basis_is_the_cartesian_basis_at_the_voigt_picks():
    from matten_amd import elastic, o3

    V = elastic.voigt_basis()
    assert V.shape == (21, 36) and V.dtype == np.float64
    _, Q = o3.cartesian_tensor_basis("ijkl=jikl=klij")
    x = np.random.default_rng(5).standard_normal(21)
    cart = np.einsum("qijkl,q->ijkl", Q, x)
    want = voigt_picks(cart)
    got = (x @ V).reshape(6, 6)
    assert np.abs(got - want).max() <= 1e-13 * max(1.0, np.abs(want).max())
    # a symmetric rank-4 tensor: the Voigt matrix is symmetric and nothing of the tensor is lost
    assert np.abs(got - got.T).max() <= 1e-13
    assert np.linalg.matrix_rank(V) == 21
    with pytest.raises(ValueError):
        elastic.voigt_basis("ij=ji")


def test_the_alias_package_reaches_the_module():
    import matten.elastic
    from matten_amd import elastic

    assert matten.elastic is elastic


@pytest.mark.parametrize("D", [1, 2, 63, 64, 257, 1024])
def test_fibonacci_hemisphere(D):
    from matten_amd import elastic

    n = elastic.fibonacci_hemisphere(D)
    assert n.shape == (D, 3) and n.dtype == np.float64
    assert np.abs(np.linalg.norm(n, axis=1) - 1.0).max() <= 4e-16
    assert (n[:, 2] >= 0.0).all()
    assert np.array_equal(n, elastic.fibonacci_hemisphere(D))                 # deterministic
    assert np.array_equal(n, elastic.check_directions(D))                     # an int means this set
    if D > 1:
        assert len(np.unique(np.round(n, 12), axis=0)) == D                   # no direction twice
    with pytest.raises(ValueError):
        elastic.fibonacci_hemisphere(0)


def test_direction_validation():
    from matten_amd import elastic

    good = np.array([[2.0, 0.0, 0.0], [1.0, 1.0, 1.0], [0.0, -3e-200, 4e-200], [1e200, 0.0, 1e200]])
    n = elastic.check_directions(good)
    assert np.abs(np.linalg.norm(n, axis=1) - 1.0).max() <= 4e-16
    assert np.allclose(n[0], [1, 0, 0]) and np.allclose(n[1], np.ones(3) / np.sqrt(3))
    assert np.allclose(n[2], [0, -0.6, 0.8]) and np.allclose(n[3], [np.sqrt(0.5), 0, np.sqrt(0.5)])
    assert elastic.check_directions([0.0, 0.0, 5.0]).shape == (1, 3)
    with pytest.raises(ValueError, match="zero vector at index 1"):
        elastic.check_directions(np.array([[1.0, 0.0, 0.0], [0.0, 0.0, 0.0]]))
    with pytest.raises(ValueError, match="non-finite"):
        elastic.check_directions(np.array([[1.0, 0.0, 0.0], [0.0, np.nan, 1.0]]))
    with pytest.raises(ValueError, match="non-finite"):
        elastic.check_directions(np.array([[np.inf, 0.0, 0.0]]))
    with pytest.raises(ValueError):
        elastic.check_directions(np.zeros((0, 3)))
    with pytest.raises(ValueError):
        elastic.check_directions(np.ones((4, 2)))
    # validation happens before any upload: elastic_properties refuses the set without touching a device
    with pytest.raises(ValueError, match="zero vector"):
        elastic.elastic_properties(np.eye(6), directions=np.zeros((2, 3)))
    with pytest.raises(ValueError, match="non-finite"):
        elastic.elastic_properties(np.eye(6), directions=np.full((1, 3), np.nan))


def test_input_shapes_are_checked_on_the_host():
    from matten_amd import elastic

    for bad in (np.zeros((2, 3, 3)), np.zeros((2, 6, 5)), np.zeros((1, 2, 3, 3, 3, 3)), np.zeros(36)):
        with pytest.raises(ValueError):
            elastic.elastic_properties(bad)
    with pytest.raises(ValueError):
        elastic.elastic_properties([])
    with pytest.raises(ValueError):
        elastic.elastic_properties([None, None])


def test_library_declares_and_binds_the_elastic_entries():
    from matten_amd import _lib, ops

    header = open(os.path.join(ROOT, "include", "matten_hip.h")).read()
    declared = set(re.findall(r"\b(matten_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for name in ("matten_elastic_props", "matten_elastic_directional"):
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name)
    assert header.count("predict.py:217-218") >= 1
    assert _lib.ABI_VERSION == 47 and lib.matten_abi_version() == 47
    assert callable(ops.elastic_props) and callable(ops.elastic_directional)
    # host-detectable argument errors, no GPU touched
    assert lib.matten_elastic_props(None, 0, 0, 3, None, None, None, None, None) == -1
    assert lib.matten_elastic_props(None, 0, 2, 0, None, None, None, None, None) == -1
    assert lib.matten_elastic_props(None, 1, 1, 0, None, None, None, None, None) == 0
    assert lib.matten_elastic_directional(None, None, None, 2, 0, None, None, None, None, None) == -1    # D >= 1
    assert lib.matten_elastic_directional(None, None, None, 2, 5, None, None, None, None, None) == -1
    assert lib.matten_elastic_directional(None, None, None, 0, 5, None, None, None, None, None) == 0


def test_predict_refuses_properties_of_per_atom_tensors():
    from matten_amd import predict as P

    with pytest.raises(ValueError, match="is_atomic_tensor"):
        P.predict([], model=object(), config={"data": {"r_cut": 5.0}}, is_atomic_tensor=True, properties=True)
