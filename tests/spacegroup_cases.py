"""
Crystals with known symmetry for the tests of the symmetry search (test_spacegroup_host.py, test_gpu_spacegroup.py): each
as (cell [3,3] rows = lattice vectors, fractional coordinates [n,3], Z [n]), the expected point-group order and number of
pure translations, a seeded noise helper and the packing into the arrays ``find_symmetry`` takes.  None of the cases sits
near the tolerance: symprec = 1e-3, noise amplitude 1e-4.
"""
import numpy as np

SYMPREC = 1e-3
NOISE = 1e-4            # symprec / 10, uniform, on every cell entry and every Cartesian coordinate

_FCC = np.array([[0, 0, 0], [0, .5, .5], [.5, 0, .5], [.5, .5, 0]])
_DIAMOND = np.concatenate([_FCC, _FCC + 0.25])


def _hex(a, c):
    return np.array([[a, 0, 0], [-a / 2, a * np.sqrt(3) / 2, 0], [0, 0, c]])


def _lattice(a, b, c, alpha, beta, gamma):
    al, be, ga = np.radians([alpha, beta, gamma])
    cx = c * np.cos(be)
    cy = c * (np.cos(al) - np.cos(be) * np.cos(ga)) / np.sin(ga)
    return np.array([[a, 0, 0], [b * np.cos(ga), b * np.sin(ga), 0], [cx, cy, np.sqrt(c * c - cx * cx - cy * cy)]])


def supercell(cell, frac, Z, reps):
    """(cell, frac, Z) repeated reps = (n0, n1, n2) times along the lattice vectors"""
    reps = np.asarray(reps)
    shifts = np.array([(i, j, k) for i in range(reps[0]) for j in range(reps[1]) for k in range(reps[2])], dtype=np.float64)
    f = ((np.asarray(frac)[None] + shifts[:, None]) / reps).reshape(-1, 3)
    return np.asarray(cell) * reps[:, None], f, np.tile(np.asarray(Z), len(shifts))


def _origin(z=13):
    return np.zeros((1, 3)), [z]


_RNG = np.random.default_rng(2024)
_TRICLINIC = _lattice(4.1, 5.2, 6.3, 77.0, 83.0, 98.0)
_RANDOM5 = _RNG.uniform(0.05, 0.95, (5, 3))
_PAIR = np.array([[0.5, 0.5, 0.5], [0.137, 0.291, 0.413], [0.863, 0.709, 0.587]])   # a centre atom and a pair related by inversion
_X = 0.305    # rutile
_U = 0.375    # wurtzite
_A = 4.0

# name -> (cell, frac, Z, point-group order, pure translations)
CASES = {
    "simple_cubic": (np.eye(3) * 3.0, *_origin(), 48, 1),
    "fcc_primitive": (0.5 * _A * np.array([[0., 1, 1], [1, 0, 1], [1, 1, 0]]), *_origin(), 48, 1),
    "fcc_conventional": (np.eye(3) * _A, _FCC, [13] * 4, 48, 4),
    "bcc_conventional": (np.eye(3) * 3.3, np.array([[0, 0, 0], [.5, .5, .5]]), [26] * 2, 48, 2),
    "diamond": (np.eye(3) * 5.43, _DIAMOND, [14] * 8, 48, 4),
    "rocksalt": (np.eye(3) * 5.64, np.concatenate([_FCC, (_FCC + [.5, 0, 0]) % 1.0]), [11] * 4 + [17] * 4, 48, 4),
    "fcc_2x2x2": (*supercell(np.eye(3) * _A, _FCC, [13] * 4, (2, 2, 2)), 48, 32),
    "cubic_skew": (3.0 * np.array([[1., 0, 0], [1, 1, 0], [0, 0, 1]]), *_origin(), 48, 1),          # (a, a+b, c): m = (2,1,1)
    "zincblende": (np.eye(3) * 5.41, _DIAMOND, [30] * 4 + [16] * 4, 24, 4),
    "hcp": (_hex(3.2, 3.2 * np.sqrt(8 / 3)), np.array([[1 / 3, 2 / 3, .25], [2 / 3, 1 / 3, .75]]), [12] * 2, 24, 1),
    "wurtzite": (_hex(3.82, 6.26), np.array([[1 / 3, 2 / 3, 0], [2 / 3, 1 / 3, .5], [1 / 3, 2 / 3, _U], [2 / 3, 1 / 3, .5 + _U]]),
                 [30, 30, 16, 16], 12, 1),
    "rutile": (np.diag([4.59, 4.59, 2.96]),
               np.array([[0, 0, 0], [.5, .5, .5], [_X, _X, 0], [1 - _X, 1 - _X, 0], [.5 + _X, .5 - _X, .5], [.5 - _X, .5 + _X, .5]]),
               [22, 22, 8, 8, 8, 8], 16, 1),
    "tetragonal": (np.diag([3.0, 3.0, 4.1]), *_origin(), 16, 1),
    "orthorhombic": (np.diag([3.0, 3.7, 4.4]), *_origin(), 8, 1),
    "monoclinic": (_lattice(3.0, 3.7, 4.4, 90.0, 100.0, 90.0), *_origin(), 4, 1),
    "triclinic": (_TRICLINIC, *_origin(), 2, 1),
    "triclinic_random5": (_TRICLINIC, _RANDOM5, [8, 8, 14, 14, 14], 1, 1),
    "triclinic_inversion": (_TRICLINIC, _PAIR, [20, 8, 8], 2, 1),
}
NAMES = list(CASES)
RANGE_CELL = 3.0 * np.array([[1., 0, 0], [2, 1, 0], [1, 0, 1]])       # (a, 2a+b, a+c): m = (5,2,2)


def crystal(name, noisy=False):
    """(cell, Cartesian positions, Z) of a case; ``noisy``: with seeded uniform noise of amplitude NOISE on both"""
    cell, frac, Z = CASES[name][:3]
    cell, pos = np.array(cell, dtype=np.float64), np.asarray(frac, dtype=np.float64) @ np.asarray(cell, dtype=np.float64)
    if noisy:
        rng = np.random.default_rng(NAMES.index(name) + 1)
        cell = cell + rng.uniform(-NOISE, NOISE, (3, 3))
        pos = pos + rng.uniform(-NOISE, NOISE, pos.shape)
    return cell, pos, np.asarray(Z, dtype=np.int64)


def expected(name):
    return CASES[name][3], CASES[name][4]


def pack(crystals):
    """[(cell, pos, Z), ...] -> dict(pos, cell, Z, ptr) as ``find_symmetry`` takes them"""
    ptr = np.concatenate([[0], np.cumsum([len(c[1]) for c in crystals])]).astype(np.int64)
    return dict(pos=np.concatenate([np.asarray(c[1], dtype=np.float64).reshape(-1, 3) for c in crystals]),
                cell=np.stack([np.asarray(c[0], dtype=np.float64) for c in crystals]),
                Z=np.concatenate([np.asarray(c[2], dtype=np.int64) for c in crystals]), ptr=ptr)


def fcc_primitive_4x4x4():
    """64 atoms, 64 pure translations"""
    cell, frac, Z = supercell(CASES["fcc_primitive"][0], np.zeros((1, 3)), [13], (4, 4, 4))
    return cell, frac @ cell, np.asarray(Z, dtype=np.int64)


def interstitial_65():
    """the 64-atom supercell plus one atom of another species at a general position: the pivot species has one atom"""
    cell, pos, Z = fcc_primitive_4x4x4()
    extra = np.array([[0.137, 0.291, 0.413]]) @ cell
    return cell, np.concatenate([pos, extra]), np.concatenate([Z, [1]])


def random_triclinic(n, seed, species=(8, 14)):
    """n atoms at random in a triclinic cell of 5 atoms' density; every eighth atom is of the first (the pivot) species"""
    rng = np.random.default_rng(seed)
    cell = _TRICLINIC * (n / 5.0) ** (1.0 / 3.0)
    Z = np.where(np.arange(n) % 8 == 3, species[0], species[1]).astype(np.int64)
    return cell, rng.uniform(0, 1, (n, 3)) @ cell, Z


def displaced_diamond(amount):
    """diamond with atom 5 moved by ``amount`` along a general direction"""
    cell, pos, Z = crystal("diamond")
    d = np.array([0.36, -0.48, 0.8])
    pos = pos.copy()
    pos[5] += amount * d / np.linalg.norm(d)
    return cell, pos, Z


def maps_onto_itself(cell, pos, Z, R, t, src, symprec=SYMPREC):
    """the direct check of one operation, independent of the search: atom src[k] (local index) imaged by r' = R r + t L lands
    within symprec of atom k under the minimum image, and is of its species -> the largest distance"""
    image = pos[src] @ R.T + t @ cell
    d = (image - pos) @ np.linalg.inv(cell)
    d -= np.round(d)
    dist = np.linalg.norm(d @ cell, axis=1)
    assert (Z[src] == Z).all()
    return dist.max()
