"""
CPU tests of the pair (shear modulus, Poisson's ratio) and acoustic (sound velocities, Debye temperature) properties of
matten_amd/elastic.py: the two C entries' declarations and bindings, the angle table, the split of the flat pair index and
every argument error that is raised before anything reaches a device.  No kernel is launched.
"""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = {"data": {"r_cut": 5.0, "tensor_target_name": "elastic_tensor_full", "tensor_target_formula": "ijkl=jikl=klij"}}


def test_library_declares_and_binds_the_pair_and_acoustic_entries():
    from matten_amd import _lib, ops

    header = open(os.path.join(ROOT, "include", "matten_hip.h")).read()
    declared = set(re.findall(r"\b(matten_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for name in ("matten_elastic_pair", "matten_elastic_acoustic"):
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name)
    assert header.count("predict.py:217-218") >= 3                      # each new entry names the call site it stands in for
    assert _lib.ABI_VERSION == 47 and lib.matten_abi_version() == 47    # entries were only added
    assert callable(ops.elastic_pair) and callable(ops.elastic_acoustic)
    # host-detectable argument errors, no GPU touched: (n, n_dirs, n_angles)
    pair = lambda n, D, M: lib.matten_elastic_pair(None, None, None, None, n, D, M, None, None, None, None)
    assert pair(0, 5, 3) == 0                                           # n == 0 is fine
    assert pair(2, 5, 3) == -1                                          # null pointers
    assert pair(0, 0, 3) == -1 and pair(0, 5, 0) == -1 and pair(-1, 5, 3) == -1
    assert pair(0, 1 << 20, 1 << 11) == -1 and pair(0, 1 << 20, (1 << 11) - 1) == 0      # D M <= 2^31 - 1
    assert pair(0, 1, 0x7fffffff) == 0 and pair(0, 1, 0x80000000) == -1
    ac = lambda n, D: lib.matten_elastic_acoustic(None, None, None, None, n, D, 1e9, None, None, None, None, None)
    assert ac(0, 5) == 0 and ac(2, 5) == -1 and ac(0, 0) == -1 and ac(-1, 5) == -1


@pytest.mark.parametrize("M", [1, 2, 7, 180])
def test_angle_table(M):
    from matten_amd import elastic

    t = elastic.angle_table(M)
    chi = np.pi * np.arange(M) / M
    assert t.shape == (M, 2) and t.dtype == np.float64
    assert np.array_equal(t[:, 0], np.cos(chi)) and np.array_equal(t[:, 1], np.sin(chi))
    assert t[0, 0] == 1.0 and t[0, 1] == 0.0 and (t[:, 1] >= 0.0).all()            # half a turn: m and -m count once
    for bad in (0, -3, 2.5, True, None):
        with pytest.raises(ValueError, match="angles"):
            elastic.angle_table(bad)


def test_flat_pair_index_splits_into_direction_and_angle():
    from matten_amd import elastic

    M = 7
    d, k = np.meshgrid(np.arange(5), np.arange(M), indexing="ij")
    flat = np.concatenate([(d * M + k).ravel(), [-1]]).astype(np.int32)
    want_d, want_k = np.concatenate([d.ravel(), [-1]]), np.concatenate([k.ravel(), [-1]])
    got_d, got_k = elastic.split_pair_index(flat, M)
    assert np.array_equal(got_d, want_d) and np.array_equal(got_k, want_k)
    got_d, got_k = elastic.split_pair_index(torch.from_numpy(flat), M)
    assert got_d.dtype == torch.int32 and np.array_equal(got_d.numpy(), want_d) and np.array_equal(got_k.numpy(), want_k)
    big = np.array([0x7fffffff], dtype=np.int32)                        # the largest index the kernel can report
    for f in (big, torch.from_numpy(big)):
        got_d, got_k = elastic.split_pair_index(f, 180)
        assert int(got_d[0]) == 0x7fffffff // 180 and int(got_k[0]) == 0x7fffffff % 180
    got_d, got_k = elastic.split_pair_index(np.array([0, 1, 2, -1]), 1)  # M = 1: the flat index is the direction
    assert list(got_d) == [0, 1, 2, -1] and list(got_k) == [0, 0, 0, -1]


def test_argument_errors_are_raised_on_the_host():
    from matten_amd import elastic

    C = np.stack([np.eye(6), 2 * np.eye(6), 3 * np.eye(6)])
    x = torch.zeros(3, 21)
    for call in (lambda **kw: elastic.elastic_properties(C, **kw), lambda **kw: elastic.elastic_properties_from_irreps(x, **kw)):
        with pytest.raises(ValueError, match="angles.*directions"):
            call(angles=4)
        for bad in (0, -1, 2.5, True):
            with pytest.raises(ValueError, match="angles"):
                call(angles=bad, directions=5)
        with pytest.raises(ValueError, match="density.*directions"):
            call(density=[1000.0, 2000.0, 3000.0])
        with pytest.raises(ValueError, match="number_density.*density"):
            call(directions=5, number_density=[5e28] * 3)
        with pytest.raises(ValueError, match="density: expected 3"):
            call(directions=5, density=[1000.0, 2000.0])
        with pytest.raises(ValueError, match="density: expected 3"):
            call(directions=5, density=1000.0)                          # a scalar serves an unbatched input only
        with pytest.raises(ValueError, match="density.*at index 1"):
            call(directions=5, density=[1000.0, 0.0, -5.0])
        with pytest.raises(ValueError, match="density.*at index 2"):
            call(directions=5, density=np.array([1000.0, 2000.0, np.nan]))
        with pytest.raises(ValueError, match="density.*at index 0"):
            call(directions=5, density=torch.tensor([np.inf, 2000.0, 1.0]))
        with pytest.raises(ValueError, match="number_density: expected 3"):
            call(directions=5, density=[1000.0] * 3, number_density=[5e28])
        with pytest.raises(ValueError, match="number_density.*at index 2"):
            call(directions=5, density=[1000.0] * 3, number_density=[5e28, 5e28, -1.0])
    with pytest.raises(ValueError, match="density.*at index 0"):
        elastic.elastic_properties(np.eye(6), directions=5, density=-2.0)


def test_predict_checks_its_arguments_before_any_forward():
    from matten_amd import predict as P

    s = {"lattice": 3.0 * np.eye(3), "cart_coords": np.zeros((1, 3)), "atomic_numbers": np.array([13])}
    structs = [dict(s), dict(s, density=2700.0), dict(s)]
    for kw in (dict(angles=4), dict(density=[1.0, 2.0, 3.0]), dict(number_density=[5e28] * 3), dict(density="structure")):
        with pytest.raises(ValueError, match="properties=True"):
            P.predict(structs, model=object(), config=CFG, **kw)
    run = lambda **kw: P.predict(structs, model=object(), config=CFG, properties=True, **kw)   # (object(): no forward can run)
    with pytest.raises(ValueError, match="angles.*directions"):
        run(angles=4)
    with pytest.raises(ValueError, match="density.*directions"):
        run(density=[1000.0] * 3)
    with pytest.raises(ValueError, match="number_density.*density"):
        run(directions=5, number_density=[5e28] * 3)
    with pytest.raises(ValueError, match="density: expected 3"):
        run(directions=5, density=[1000.0] * 4)
    with pytest.raises(ValueError, match="density.*at index 1"):
        run(directions=5, density=[1000.0, np.nan, 1.0])
    with pytest.raises(ValueError, match=r"structures \[0, 2\]"):
        run(directions=5, density="structure")
    with pytest.raises(ValueError, match="density"):
        run(directions=5, density="pymatgen")


def test_structure_densities_are_read_in_si():
    from matten_amd import predict as P

    class WithDensity:              # what a pymatgen Structure offers: g/cm^3
        density = 2.7

    class Without:
        pass

    got = P._structure_densities([{"density": 2330.0}, WithDensity(), {"density": 1.0, "lattice": None}])
    assert np.array_equal(got, [2330.0, 1000.0 * 2.7, 1.0])
    with pytest.raises(ValueError, match=r"structures \[1, 3\]"):
        P._structure_densities([{"density": 1.0}, {}, WithDensity(), Without()])
