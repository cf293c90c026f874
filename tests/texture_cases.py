"""
What the texture tests share (tests/test_texture_host.py, tests/test_gpu_texture.py): the eight packed textures and the six
explicit aggregates the device is compared on, over the 257 rows of tests/polycrystal_cases.py.  numpy only.
"""
import numpy as np

import polycrystal_cases as pc

FIBRE_CRYSTAL, FIBRE_SAMPLE = (1.0, 1.0, 1.0), (0.0, 0.0, 1.0)
T_SINGLE, T_FIBRE, T_UNIFORM, T_WEIGHTED, T_LARGE, T_NOT_ORTHOGONAL, T_ZERO_WEIGHT, T_EMPTY = range(8)
N_TEXTURES = 8
GOOD_TEXTURES = (T_SINGLE, T_FIBRE, T_UNIFORM, T_WEIGHTED, T_LARGE)
BAD_TEXTURES = (T_NOT_ORTHOGONAL, T_ZERO_WEIGHT, T_EMPTY)
SIZES = (1, 5, 60, 37, 10007, 3, 4, 0)
SMALL_SLICE = 500          # 10 007 orientations: 21 slices, the last one of 7


def random_rotations(n: int, seed: int) -> np.ndarray:
    """n proper rotations, seeded (QR of a normal matrix, signs fixed)"""
    rng = np.random.default_rng(seed)
    Q, R = np.linalg.qr(rng.standard_normal((n, 3, 3)))
    Q = Q * np.sign(np.diagonal(R, axis1=1, axis2=2))[:, None, :]
    return Q * np.linalg.det(Q)[:, None, None]


def single_rotation() -> np.ndarray:
    return random_rotations(1, 11)[0]


def weighted_37():
    """37 seeded orientations, one of them improper, with seeded positive weights that do not sum to 1"""
    R = random_rotations(37, 12)
    R[5] = -R[5]
    return R, np.random.default_rng(13).uniform(0.1, 2.0, size=37)


def packed():
    """(R [10117,3,3], weights [10117], ptr [9]) of the eight textures, as plain arrays: the last three are bad on
    purpose (a sheared matrix, weights that sum to zero, no orientations), which a validating ``Texture`` would refuse"""
    from matten_amd.texture import Texture

    R37, w37 = weighted_37()
    sheared = random_rotations(3, 14)
    sheared[1, 0, 1] += 1e-3
    parts = [(single_rotation()[None], None), (Texture.fibre(FIBRE_CRYSTAL, FIBRE_SAMPLE, 5).rotations, None),
             (Texture.uniform().rotations, None), (R37, w37), (random_rotations(10007, 15), None), (sheared, None),
             (random_rotations(4, 16), np.zeros(4)), (np.zeros((0, 3, 3)), None)]
    assert tuple(len(r) for r, _ in parts) == SIZES
    R = np.concatenate([r for r, _ in parts])
    w = np.concatenate([np.ones(len(r)) if wt is None else wt for r, wt in parts])
    ptr = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    return R, w, ptr


def textures():
    """the eight textures as one ``Texture`` (not validated on the host: the device flags the bad ones)"""
    from matten_amd.texture import Texture

    return Texture(*packed(), validate=False)


# six explicit aggregates of 2 to 3 members: (crystal, texture, fraction) lists
AGGREGATES = (
    ((pc.ROW_CUBIC, T_FIBRE, 0.7), (pc.ROW_HEXAGONAL, T_WEIGHTED, 0.3)),                                # two phases: status 0
    ((pc.ROW_CUBIC, T_UNIFORM, 2.0), (pc.ROW_TRICLINIC, T_SINGLE, 1.0), (pc.ROW_CUBIC, T_SINGLE, 0.0)),  # fractions not normalised
    ((pc.ROW_ISOTROPIC, T_LARGE, 0.5), (pc.ROW_NOT_PD, T_FIBRE, 0.5)),                                   # status 2, voigt finite
    ((pc.ROW_CUBIC, T_FIBRE, 0.5), (pc.ROW_NAN, T_FIBRE, 0.5)),                                          # status -1
    ((pc.ROW_CUBIC, T_FIBRE, 0.5), (pc.ROW_HEXAGONAL, T_ZERO_WEIGHT, 0.5)),                              # a bad texture: -1
    ((pc.ROW_CUBIC, T_FIBRE, 0.0), (pc.ROW_HEXAGONAL, T_UNIFORM, 0.0)),                                  # zero fraction sum: -1
)
AGGREGATE_STATUS = (0, 0, 2, -1, -1, -1)


def phases():
    """(agg_ptr [7], crystal [13], texture [13], fraction [13]) of AGGREGATES"""
    sizes = [len(a) for a in AGGREGATES]
    flat = [m for a in AGGREGATES for m in a]
    return (np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), np.array([m[0] for m in flat], dtype=np.int32),
            np.array([m[1] for m in flat], dtype=np.int32), np.array([m[2] for m in flat], dtype=np.float64))


def uniform_closed_forms(c11, c12, c44):
    """-> (K, G_voigt, G_reuss, G_hill, G_geometric) of an untextured aggregate of cubic crystals"""
    K, m1, m2 = (c11 + 2.0 * c12) / 3.0, 0.5 * (c11 - c12), c44
    gv, gr = (2.0 * m1 + 3.0 * m2) / 5.0, 5.0 / (2.0 / m1 + 3.0 / m2)
    return K, gv, gr, 0.5 * (gv + gr), m1 ** 0.4 * m2 ** 0.6
