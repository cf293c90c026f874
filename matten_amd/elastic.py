"""
Derived elastic properties of (predicted) elasticity tensors, on the device.

The reference ends ``predict`` with ``predictions = [ElasticTensor(t) for t in predictions]`` (predict.py:217-218) and its
users read bulk and shear moduli, Young's modulus, Poisson's ratio, the anisotropy index, the compliance tensor and
directional moduli off that pymatgen object, one Python object per crystal.  Here two kernels
(``matten_elastic_props`` / ``matten_elastic_directional``, csrc/elastic.hip) compute them for a whole batch in fp64.
``elastic_properties`` detaches its input; ``elastic_moduli`` / ``elastic_moduli_from_irreps`` give the Voigt matrix, the
compliance and the ten scalars attached to the autograd graph (``matten_elastic_props_bwd``), and ``ModuliLoss`` is the loss
to fine-tune a tensor model against scalar moduli.  With ``directions`` / ``density`` / ``number_density`` they attach the
directional Young's modulus and compressibility, the Christoffel velocities, their extremes, the Debye average and the
Debye temperature as well (``matten_elastic_directional_bwd`` / ``matten_elastic_acoustic_bwd``), and ``ModuliLoss`` takes
those names: training on ultrasonic, calorimetric and indentation data.  The pair quantities (shear modulus and Poisson's
ratio over direction pairs) carry no gradient, neither do directions and densities, there is no Lightning ``Task`` around
the loss, and a host tensor is not differentiated.
Two more serve what depends on two directions or on the mass density: ``matten_elastic_pair`` (shear modulus and Poisson's
ratio over pairs of perpendicular directions) and ``matten_elastic_acoustic`` (the Christoffel phase velocities per
direction, their Debye average and, with a number density, the Debye temperature).

Conventions ("Derived elastic properties"): Voigt order xx, yy, zz, yz, xz, xy as in pymatgen;
``C_IJ = C_ijkl`` without factors and ``compliance = inv(C_IJ)``, the engineering convention (the factors 2 and 4 live in
the compliance); the input is symmetrised, never trusted.  Every value is in the units of the input tensor -- pymatgen's
``y_mod`` alone is multiplied by 1e9 (GPa -> Pa); this module does not copy that.  The velocities (m/s) and the Debye
temperature (K) alone are SI: ``density`` is kg/m^3, ``number_density`` atoms/m^3, ``modulus_unit`` Pa per unit of the input.
"""
import numpy as np
import torch

from . import o3, ops

PROP_NAMES = ("k_voigt", "g_voigt", "k_reuss", "g_reuss", "k_vrh", "g_vrh", "y_mod", "homogeneous_poisson",
              "universal_anisotropy", "pugh_ratio")
# the [B] directional and acoustic quantities that ``elastic_moduli`` attaches to the graph and ``ModuliLoss`` accepts, with
# the argument of ``elastic_moduli`` that produces each
DIRECTIONAL_NAMES = {"young_min": "directions", "young_max": "directions", "compressibility_min": "directions",
                     "compressibility_max": "directions", "v_slow_min": "density", "v_fast_max": "density",
                     "v_mean": "density", "debye_temperature": "number_density"}
FLAG_SINGULAR, FLAG_NOT_POSITIVE_DEFINITE, FLAG_FAILED_STRUCTURE = 1, 2, 4

# Voigt index -> Cartesian pair, pymatgen's order
VOIGT_PAIRS = ((0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1))

# exact SI constants (2019 redefinition): hbar = h / 2 pi [J s], k_B [J/K]
HBAR = 6.62607015e-34 / (2.0 * np.pi)
K_B = 1.380649e-23

class ElasticProperties:
    """Batch of derived properties: ``voigt`` / ``compliance`` [B,6,6], one [B] tensor per name of ``PROP_NAMES``,
    ``flags`` [B] int32 (bit 0 singular or non-finite input: the row is NaN; bit 1 not positive definite; bit 2 the
    structure failed in ``predict``), ``is_stable`` / ``is_singular`` [B] bool.  With directions also ``directions`` [D,3],
    ``young_min`` / ``young_max`` / ``compressibility_min`` / ``compressibility_max`` [B] with their ``*_argmin`` /
    ``*_argmax`` direction indices (-1 on singular rows), and ``young`` / ``compressibility`` [B,D] when they were kept
    (else None).  With ``angles`` = M also ``angles`` [M] (chi_k = pi k / M), ``shear_min`` / ``shear_max`` / ``poisson_min`` /
    ``poisson_max`` [B] over all pairs (direction d, angle k), each with a ``*_direction`` and a ``*_angle`` index (-1 on
    singular rows), and the per-direction extremes over chi ``shear_dir_min`` / ``shear_dir_max`` / ``poisson_dir_min`` /
    ``poisson_dir_max`` [B,D] when kept.  With ``density`` also ``v_slow_min`` / ``v_fast_max`` [B] (m/s) with their
    ``*_direction``, ``sum_inv_v3``, ``v_mean`` = (sum_inv_v3 / 3D)^(-1/3), ``acoustic_unstable_directions`` [B] int32 and
    ``velocities`` [B,D,3] (ascending) when kept; with ``number_density`` also ``debye_temperature`` [B] (K).
    An unbatched input ([3,3,3,3] or [6,6]) gives the same without the leading dimension."""

    def __init__(self, **fields):
        self._names = tuple(fields)
        for k, v in fields.items():
            setattr(self, k, v)

    @property
    def has_directions(self) -> bool:
        return "directions" in self._names

    def _map(self, fn) -> "ElasticProperties":
        return ElasticProperties(**{k: (None if getattr(self, k) is None else fn(getattr(self, k))) for k in self._names})

    def cpu(self) -> "ElasticProperties":
        return self._map(lambda t: t.cpu())

    def to_dict(self) -> dict:
        """name -> numpy array on the host (None for directional maps that were not kept)"""
        return {k: (None if getattr(self, k) is None else getattr(self, k).detach().cpu().numpy()) for k in self._names}

    def __repr__(self):
        shape = tuple(self.flags.shape)
        return f"ElasticProperties(batch={shape}, directions={self.directions.shape[0] if self.has_directions else None})"


def fibonacci_hemisphere(D: int) -> np.ndarray:
    """D unit vectors [D,3] (fp64) spread evenly over the hemisphere z >= 0 by the golden-angle spiral: E(n) = E(-n), so
    the other half adds nothing.  Deterministic."""
    D = int(D)
    if D < 1:
        raise ValueError(f"directions: at least one direction is needed, got {D}")
    k = np.arange(D, dtype=np.float64)
    z = 1.0 - (k + 0.5) / D                         # equal-area rings, z in (0, 1)
    phi = k * (np.pi * (3.0 - np.sqrt(5.0)))
    r = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    n = np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)
    return n / np.linalg.norm(n, axis=1, keepdims=True)


def check_directions(directions) -> np.ndarray:
    """int D -> ``fibonacci_hemisphere(D)``; an array [D,3] is validated on the host (finite, non-zero: else ValueError)
    and normalised there -> [D,3] fp64 unit vectors"""
    if isinstance(directions, (int, np.integer)) and not isinstance(directions, bool):
        return fibonacci_hemisphere(int(directions))
    if isinstance(directions, torch.Tensor):
        directions = directions.detach().cpu().numpy()
    n = np.array(directions, dtype=np.float64)
    if n.ndim == 1 and n.shape[0] == 3:
        n = n[None]
    if n.ndim != 2 or n.shape[1] != 3 or n.shape[0] < 1:
        raise ValueError(f"directions: expected an int or an array [D,3] with D >= 1, got shape {n.shape}")
    if not np.isfinite(n).all():
        raise ValueError("directions: non-finite component")
    # (scaled by the largest component first: the norm of a tiny or huge but valid vector neither under- nor overflows)
    big = np.abs(n).max(axis=1, keepdims=True)
    if (big == 0.0).any():
        raise ValueError(f"directions: zero vector at index {int(np.nonzero(big[:, 0] == 0.0)[0][0])}")
    n = n / big
    return n / np.linalg.norm(n, axis=1, keepdims=True)


def angle_table(M: int) -> np.ndarray:
    """[M,2] fp64 = (cos chi_k, sin chi_k), chi_k = pi k / M for k = 0..M-1: half a turn, m and -m count once.  Made with
    numpy on the host and uploaded, so the kernel and a host reference use the same bits."""
    if isinstance(M, bool) or not isinstance(M, (int, np.integer)) or M < 1:
        raise ValueError(f"angles: expected an int M >= 1, got {M!r}")
    chi = np.pi * np.arange(int(M), dtype=np.float64) / int(M)
    return np.stack([np.cos(chi), np.sin(chi)], axis=1)


def split_pair_index(flat, M: int):
    """flat pair index d M + k (a torch tensor or numpy array; -1 = none) -> (direction index d, angle index k), -1 kept"""
    if isinstance(flat, torch.Tensor):
        none = flat < 0
        d = torch.div(flat, M, rounding_mode="floor")
        return torch.where(none, flat, d), torch.where(none, flat, flat - d * M)
    flat = np.asarray(flat)
    return np.where(flat < 0, flat, flat // M), np.where(flat < 0, flat, flat % M)


def _check_per_row(name: str, values, B: int, single: bool):
    """``density`` / ``number_density``: a device tensor is taken as it is (the kernel answers a bad entry with NaN); a
    host input is checked here, before anything is uploaded -> a tensor [B] (device input) or a numpy array [B] fp64"""
    if isinstance(values, torch.Tensor) and values.is_cuda:
        t = values.detach().reshape(-1).to(torch.float64)
        if t.shape[0] != B:
            raise ValueError(f"{name}: expected {B} value(s), one per tensor, got {t.shape[0]}")
        return t
    a = np.asarray(values.detach().numpy() if isinstance(values, torch.Tensor) else values, dtype=np.float64)
    if a.ndim == 0 and (single or B == 1):
        a = a.reshape(1)
    if a.ndim != 1 or a.shape[0] != B:
        raise ValueError(f"{name}: expected {B} value(s), one per tensor, got shape {a.shape}")
    bad = ~(np.isfinite(a) & (a > 0.0))
    if bad.any():
        i = int(np.nonzero(bad)[0][0])
        raise ValueError(f"{name}: expected finite positive values, got {a[i]} at index {i}")
    return a


def _check_extras(directions, angles, density, number_density):
    """the argument combinations of the pair and acoustic properties (ValueError before anything else happens)"""
    if angles is not None:
        if isinstance(angles, bool) or not isinstance(angles, (int, np.integer)) or angles < 1:
            raise ValueError(f"angles: expected an int M >= 1, got {angles!r}")
        if directions is None:
            raise ValueError("angles: the pairs (n, m) need a direction set, pass directions")
    if density is not None and directions is None:
        raise ValueError("density: the acoustic velocities need a direction set, pass directions")
    if number_density is not None and density is None:
        raise ValueError("number_density: the Debye temperature needs the sound velocities, pass density")


_VOIGT_BASIS = {}


def voigt_basis(formula: str = "ijkl=jikl=klij") -> np.ndarray:
    """[21,36] fp64: the model's irreps components of a rank-4 elasticity tensor straight to the row-major Voigt matrix,
    ``voigt.reshape(36) = x @ voigt_basis()`` -- the 36 Voigt columns of ``o3.cartesian_tensor_basis``'s [21,81]"""
    if formula not in _VOIGT_BASIS:
        _, Q = o3.cartesian_tensor_basis(formula)
        if Q.ndim != 5:
            raise ValueError(f"voigt_basis: {formula!r} is not a rank-4 tensor")
        cols = [Q[:, i, j, k, l] for (i, j) in VOIGT_PAIRS for (k, l) in VOIGT_PAIRS]
        V = np.ascontiguousarray(np.stack(cols, axis=1), dtype=np.float64)
        V.setflags(write=False)
        _VOIGT_BASIS[formula] = V
    return _VOIGT_BASIS[formula]


def _default_device() -> torch.device:
    return torch.device("cuda", torch.cuda.current_device())


def _as_rows(tensors):
    """-> (rows [B,81] or [B,36] where the input is -- ``_upload`` makes the one copy of a host input once every host
    check has passed --, layout, unbatched?, failed [B] bool on the host or None)"""
    failed = None
    if isinstance(tensors, (list, tuple)):
        if not tensors:
            raise ValueError("tensors: empty list")
        missing = [t is None for t in tensors]
        if all(missing):
            raise ValueError("tensors: every entry is None")
        if any(missing):      # what predict() returns for structures it could not use: NaN rows, flag bit 2
            first = next(t for t in tensors if t is not None)
            if isinstance(first, torch.Tensor):
                hole = torch.full_like(first, float("nan"))
            else:
                first = np.asarray(first)
                hole = np.full(first.shape, np.nan, dtype=first.dtype if first.dtype.kind == "f" else np.float64)
            tensors = [hole if t is None else t for t in tensors]
            failed = np.array(missing)
        if isinstance(tensors[0], torch.Tensor):
            tensors = torch.stack(list(tensors))
        else:
            tensors = np.stack([np.asarray(t) for t in tensors])
    if not isinstance(tensors, torch.Tensor):
        a = np.asarray(tensors)
        if a.dtype not in (np.float32, np.float64):
            a = a.astype(np.float64)
        tensors = torch.from_numpy(np.ascontiguousarray(a))
    if tensors.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"tensors: expected fp32 or fp64, got {tensors.dtype}")
    shape = tuple(tensors.shape)
    if shape[-4:] == (3, 3, 3, 3) and len(shape) in (4, 5):
        layout, single, width = 0, len(shape) == 4, 81
    elif shape[-2:] == (6, 6) and len(shape) in (2, 3):
        layout, single, width = 1, len(shape) == 2, 36
    else:
        raise ValueError(f"tensors: expected [B,3,3,3,3], [B,6,6], [3,3,3,3] or [6,6], got {shape}")
    rows = tensors.detach().reshape(-1, width)
    return rows, layout, single, failed


def _upload(rows):
    if not rows.is_cuda:
        rows = rows.to(_default_device())          # the one copy of a host input
    return rows.contiguous()


def _directional_fields(young, beta, ext, arg, dirs) -> dict:
    """the outputs of the directional kernel under their field names"""
    return dict(young=young, compressibility=beta,
                young_min=ext[:, 0], young_max=ext[:, 1], young_argmin=arg[:, 0], young_argmax=arg[:, 1],
                compressibility_min=ext[:, 2], compressibility_max=ext[:, 3],
                compressibility_argmin=arg[:, 2], compressibility_argmax=arg[:, 3], directions=dirs)


def _acoustic_fields(vel, ext, arg, n_unstable, n_dirs: int, number_density) -> dict:
    """the outputs of the acoustic kernel under their field names, with the Debye average and temperature (torch
    expressions on the sum of v^-3)"""
    fields = dict(velocities=vel, v_slow_min=ext[:, 0], v_fast_max=ext[:, 1], v_slow_min_direction=arg[:, 0],
                  v_fast_max_direction=arg[:, 1], sum_inv_v3=ext[:, 2],
                  v_mean=(ext[:, 2] / (3.0 * n_dirs)) ** (-1.0 / 3.0), acoustic_unstable_directions=n_unstable)
    if number_density is not None:
        n_at = torch.as_tensor(number_density, dtype=torch.float64).to(ext.device)
        fields["debye_temperature"] = (HBAR / K_B) * (6.0 * np.pi ** 2 * n_at) ** (1.0 / 3.0) * fields["v_mean"]
    return fields


def _from_rows(rows, layout, dirs=None, keep_directional=False, single=False, failed=None, angles=None, density=None,
               number_density=None, modulus_unit: float = 1e9) -> ElasticProperties:
    """rows on the device -> ElasticProperties; ``dirs``: unit vectors out of ``check_directions`` (host) or None;
    ``density`` / ``number_density``: out of ``_check_per_row`` or None"""
    voigt, compliance, props, flags = ops.elastic_props(rows, layout)
    if failed is not None and failed.any():
        flags |= torch.as_tensor(failed.astype(np.int32) * FLAG_FAILED_STRUCTURE, device=flags.device)
    fields = {"voigt": voigt, "compliance": compliance}
    for q, name in enumerate(PROP_NAMES):
        fields[name] = props[:, q]
    fields["flags"] = flags
    fields["is_stable"] = flags == 0
    fields["is_singular"] = (flags & FLAG_SINGULAR) != 0
    if dirs is not None:
        dirs = torch.from_numpy(np.ascontiguousarray(dirs)).to(rows.device)
        fields.update(_directional_fields(*ops.elastic_directional(compliance, flags, dirs, keep=keep_directional), dirs))
    if angles is not None:
        M = int(angles)
        table = angle_table(M)
        maps, ext, arg = ops.elastic_pair(compliance, flags, dirs, torch.from_numpy(table).to(rows.device),
                                          keep=keep_directional)
        fields["angles"] = torch.from_numpy(np.pi * np.arange(M, dtype=np.float64) / M).to(rows.device)
        for q, name in enumerate(("shear_min", "shear_max", "poisson_min", "poisson_max")):
            fields[name] = ext[:, q]
            fields[name + "_direction"], fields[name + "_angle"] = split_pair_index(arg[:, q], M)
        for q, name in enumerate(("shear_dir_min", "shear_dir_max", "poisson_dir_min", "poisson_dir_max")):
            fields[name] = None if maps is None else maps[:, :, q]
    if density is not None:
        rho = torch.as_tensor(density, dtype=torch.float64).to(rows.device)
        fields.update(_acoustic_fields(*ops.elastic_acoustic(voigt, flags, rho, dirs, modulus_unit, keep=keep_directional),
                                       dirs.shape[0], number_density))
    if single:
        fields = {k: (v if v is None or k in ("directions", "angles") else v[0]) for k, v in fields.items()}
    return ElasticProperties(**fields)


def elastic_properties(tensors, directions=None, keep_directional: bool = False, angles=None, density=None,
                       number_density=None, modulus_unit: float = 1e9) -> ElasticProperties:
    """``tensors``: a torch tensor or numpy array [B,3,3,3,3], [B,6,6], [3,3,3,3] or [6,6], fp32 or fp64, on the device or
    on the host (copied once), or a list of such tensors as ``predict`` returns (stacked; a ``None`` entry becomes a NaN
    row with flag bit 2).  ``directions``: an int D (``fibonacci_hemisphere(D)``) or an array [D,3] (validated and
    normalised on the host); with them the extremes of Young's modulus and of the linear compressibility over the
    directions are returned, and the full [B,D] maps when ``keep_directional``.  ``angles``: an int M >= 1 (needs
    ``directions``): shear modulus G(n,m) and Poisson's ratio nu(n,m) over the D x M pairs of a direction n and the
    perpendicular m at angle chi_k = pi k / M in n's frame, their extremes with a direction and an angle index each.
    ``density``: [B] (a scalar for an unbatched input) in kg/m^3 (needs ``directions``): the three acoustic phase
    velocities per direction in m/s, their extremes and the Debye average ``v_mean``; ``modulus_unit`` is Pa per unit of
    the input (1e9: GPa).  ``number_density``: [B] atoms/m^3 (needs ``density``): ``debye_temperature`` in K.  A host
    ``density`` / ``number_density`` is checked before anything is uploaded (ValueError naming the first bad index).
    The results stay on the device."""
    _check_extras(directions, angles, density, number_density)
    dirs = None if directions is None else check_directions(directions)      # (before anything is uploaded)
    rows, layout, single, failed = _as_rows(tensors)
    if density is not None:
        density = _check_per_row("density", density, rows.shape[0], single)
    if number_density is not None:
        number_density = _check_per_row("number_density", number_density, rows.shape[0], single)
    return _from_rows(_upload(rows), layout, dirs, keep_directional, single, failed, angles, density, number_density,
                      modulus_unit)


_VOIGT_Q = {}


def elastic_properties_from_irreps(x, directions=None, keep_directional: bool = False,
                                   formula: str = "ijkl=jikl=klij", angles=None, density=None, number_density=None,
                                   modulus_unit: float = 1e9) -> ElasticProperties:
    """The same from the model's irreps rows ``x`` [B,21] (fp32, on the device): one ``dense_rows`` with ``voigt_basis``
    gives the Voigt matrices [B,36] directly -- no [B,81] Cartesian intermediate."""
    if not isinstance(x, torch.Tensor) or x.dim() not in (1, 2):
        raise ValueError("x: expected a tensor [B,21] or [21]")
    _check_extras(directions, angles, density, number_density)
    dirs = None if directions is None else check_directions(directions)
    single = x.dim() == 1
    x = x.detach().reshape(-1, x.shape[-1])
    if density is not None:
        density = _check_per_row("density", density, x.shape[0], single)
    if number_density is not None:
        number_density = _check_per_row("number_density", number_density, x.shape[0], single)
    V = voigt_basis(formula)
    if x.shape[1] != V.shape[0]:
        raise ValueError(f"x: expected {V.shape[0]} irreps components per row, got {x.shape[1]}")
    if not x.is_cuda:
        x = x.to(_default_device())
    key = (formula, x.device)
    if key not in _VOIGT_Q:
        _VOIGT_Q[key] = torch.tensor(V, dtype=torch.float32, device=x.device)
    rows = ops.dense_rows(x.to(torch.float32), _VOIGT_Q[key])
    return _from_rows(rows, 1, dirs, keep_directional, single, None, angles, density, number_density, modulus_unit)


# ---------------------------------------------------------------------------------------------------
# differentiable: training on moduli
# ---------------------------------------------------------------------------------------------------
def _moduli_fields(rows, layout, single, dirs=None, keep_directional=False, density=None, number_density=None,
                   modulus_unit: float = 1e9) -> ElasticProperties:
    """``_from_rows`` attached to the autograd graph (no pair quantities): the same kernels, so the same bits"""
    from .autograd import ElasticAcousticFn, ElasticDirectionalFn, ElasticPropsFn

    voigt, compliance, props, flags = ElasticPropsFn.apply(rows, layout)
    fields = {"voigt": voigt, "compliance": compliance}
    for q, name in enumerate(PROP_NAMES):
        fields[name] = props[:, q]
    fields["flags"] = flags
    fields["is_stable"] = flags == 0
    fields["is_singular"] = (flags & FLAG_SINGULAR) != 0
    if dirs is not None:
        dirs = torch.from_numpy(np.ascontiguousarray(dirs)).to(rows.device)
        fields.update(_directional_fields(*ElasticDirectionalFn.apply(compliance, flags, dirs, bool(keep_directional)), dirs))
    if density is not None:
        rho = torch.as_tensor(density, dtype=torch.float64).to(rows.device)
        fields.update(_acoustic_fields(*ElasticAcousticFn.apply(voigt, flags, rho, dirs, float(modulus_unit),
                                                                bool(keep_directional)), dirs.shape[0], number_density))
    if single:
        fields = {k: (v if v is None or k == "directions" else v[0]) for k, v in fields.items()}
    return ElasticProperties(**fields)


def _check_moduli_extras(directions, angles, density, number_density, B: int, single: bool):
    """the directional arguments of ``elastic_moduli*``, validated as ``elastic_properties`` does, before anything touches
    the device -> (dirs, density, number_density)"""
    if angles is not None:
        raise ValueError("angles: the pair quantities carry no gradient (shear modulus and Poisson's ratio over direction "
                         "pairs); use elastic_properties for them")
    _check_extras(directions, None, density, number_density)
    dirs = None if directions is None else check_directions(directions)
    if density is not None:
        density = _check_per_row("density", density, B, single)
    if number_density is not None:
        number_density = _check_per_row("number_density", number_density, B, single)
    return dirs, density, number_density


def elastic_moduli(tensors, directions=None, keep_directional: bool = False, density=None, number_density=None,
                   modulus_unit: float = 1e9, angles=None) -> ElasticProperties:
    """The differentiable ``elastic_properties``: ``tensors`` is a device tensor [B,3,3,3,3], [B,6,6], [3,3,3,3] or [6,6],
    fp32 or fp64; ``voigt``, ``compliance`` and the ten scalars of ``PROP_NAMES`` come back attached to its autograd graph
    (``flags``, ``is_stable``, ``is_singular`` as in ``elastic_properties``).  A row with flag bit 0 is NaN and sends a zero
    gradient back; an indefinite row is differentiated like any other.  ``directions``, ``keep_directional``, ``density``,
    ``number_density`` and ``modulus_unit`` are those of ``elastic_properties`` (same validation, same values bit for
    bit); with them ``young_min`` / ``young_max``, ``compressibility_min`` / ``compressibility_max``, ``v_slow_min``,
    ``v_fast_max``, ``sum_inv_v3``, ``v_mean``, ``debye_temperature`` and, when kept, the maps ``young`` / ``compressibility``
    / ``velocities`` are attached too (``DIRECTIONAL_NAMES``); an extreme's gradient is that of the direction where it was
    found, an acoustically unstable direction contributes nothing.  The directions and densities receive no gradient.
    ``angles`` is refused: the pair quantities carry no gradient."""
    if not isinstance(tensors, torch.Tensor):
        raise ValueError("tensors: elastic_moduli differentiates device tensors only; for arrays, lists and host tensors "
                         "use elastic_properties (no gradient)")
    if tensors.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"tensors: expected fp32 or fp64, got {tensors.dtype}")
    shape = tuple(tensors.shape)
    if shape[-4:] == (3, 3, 3, 3) and len(shape) in (4, 5):
        layout, single, width = 0, len(shape) == 4, 81
    elif shape[-2:] == (6, 6) and len(shape) in (2, 3):
        layout, single, width = 1, len(shape) == 2, 36
    else:
        raise ValueError(f"tensors: expected [B,3,3,3,3], [B,6,6], [3,3,3,3] or [6,6], got {shape}")
    B = 1 if single else shape[0]
    dirs, density, number_density = _check_moduli_extras(directions, angles, density, number_density, B, single)
    if not tensors.is_cuda:
        raise ValueError("tensors: elastic_moduli differentiates device tensors only; a host tensor goes through "
                         "elastic_properties (no gradient)")
    return _moduli_fields(tensors.reshape(-1, width), layout, single, dirs, keep_directional, density, number_density,
                          modulus_unit)


_VOIGT_QT = {}


def elastic_moduli_from_irreps(x, formula: str = "ijkl=jikl=klij", directions=None, keep_directional: bool = False,
                               density=None, number_density=None, modulus_unit: float = 1e9, angles=None) -> ElasticProperties:
    """The differentiable ``elastic_properties_from_irreps``: ``x`` [B,21] (or [21]) fp32 on the device, usually the model's
    output with its ``grad_fn``.  The forward is the same ``dense_rows`` with ``voigt_basis``; its adjoint is ``dense_rows``
    with the transposed basis [36,21].  The directional arguments are those of ``elastic_moduli``."""
    from .autograd import DenseRowsFn

    if not isinstance(x, torch.Tensor) or x.dim() not in (1, 2):
        raise ValueError("x: expected a tensor [B,21] or [21]")
    V = voigt_basis(formula)
    if x.shape[-1] != V.shape[0]:
        raise ValueError(f"x: expected {V.shape[0]} irreps components per row, got {x.shape[-1]}")
    single = x.dim() == 1
    dirs, density, number_density = _check_moduli_extras(directions, angles, density, number_density,
                                                         1 if single else x.shape[0], single)
    if not x.is_cuda or x.dtype != torch.float32:
        raise ValueError("x: elastic_moduli_from_irreps differentiates fp32 device tensors only; a host tensor goes through "
                         "elastic_properties_from_irreps (no gradient)")
    key = (formula, x.device)
    if key not in _VOIGT_Q:
        _VOIGT_Q[key] = torch.tensor(V, dtype=torch.float32, device=x.device)
    if key not in _VOIGT_QT:
        _VOIGT_QT[key] = _VOIGT_Q[key].t().contiguous()
    rows = DenseRowsFn.apply(x.reshape(-1, x.shape[-1]), _VOIGT_Q[key], _VOIGT_QT[key])
    return _moduli_fields(rows, 1, single, dirs, keep_directional, density, number_density, modulus_unit)


class ModuliLoss(torch.nn.Module):
    """Loss on scalar moduli: ``forward(props, targets)`` with ``props`` an ``ElasticProperties`` (of ``elastic_moduli`` or
    ``elastic_moduli_from_irreps``) and ``targets`` a dict name -> [B]; the mean of |difference| (``kind="l1"``) or of its
    square (``"mse"``), weighted per name, over the entries whose row has flag bit 0 clear and whose target is finite.
    ``names`` come from ``PROP_NAMES`` and ``DIRECTIONAL_NAMES`` (directional extremes, sound velocities, the Debye
    temperature: ``props`` must have been made with the directional arguments); an entry of the latter whose value is not
    finite (a row with acoustically unstable directions, say) is excluded as well.
    Excluded entries are replaced with ``torch.where``, never multiplied away, so their NaN reaches neither the value nor
    the gradient; a batch without a single entry gives a zero that is still attached to the graph."""

    def __init__(self, names=("k_vrh", "g_vrh"), weights=None, kind: str = "l1"):
        super().__init__()
        names = (names,) if isinstance(names, str) else tuple(names)
        if not names:
            raise ValueError("names: at least one property is needed")
        unknown = [n for n in names if n not in PROP_NAMES and n not in DIRECTIONAL_NAMES]
        if unknown:
            raise ValueError(f"names: {unknown} not in {PROP_NAMES + tuple(DIRECTIONAL_NAMES)}")
        if len(set(names)) != len(names):
            raise ValueError(f"names: repeated entry in {names}")
        if kind not in ("l1", "mse"):
            raise ValueError(f"kind: expected 'l1' or 'mse', got {kind!r}")
        if weights is None:
            weights = {n: 1.0 for n in names}
        elif isinstance(weights, dict):
            if set(weights) != set(names):
                raise ValueError(f"weights: expected one weight for each of {names}, got {sorted(weights)}")
        else:
            weights = list(weights)
            if len(weights) != len(names):
                raise ValueError(f"weights: expected {len(names)} weights, got {len(weights)}")
            weights = dict(zip(names, weights))
        weights = {n: float(weights[n]) for n in names}
        if not all(np.isfinite(w) and w >= 0.0 for w in weights.values()):
            raise ValueError(f"weights: expected finite non-negative values, got {weights}")
        self.names, self.weights, self.kind = names, weights, kind

    def forward(self, props: ElasticProperties, targets: dict) -> torch.Tensor:
        missing = [n for n in self.names if n not in targets]
        if missing:
            raise ValueError(f"targets: no entry for {missing}")
        row_ok = (props.flags & FLAG_SINGULAR) == 0
        total, count = None, None
        for name in self.names:
            value = getattr(props, name, None)
            if value is None:
                raise ValueError(f"props: no {name!r}; pass {DIRECTIONAL_NAMES[name]} to elastic_moduli / "
                                 f"elastic_moduli_from_irreps")
            target = torch.as_tensor(targets[name], dtype=value.dtype, device=value.device)
            if target.shape != value.shape:
                raise ValueError(f"targets[{name!r}]: expected shape {tuple(value.shape)}, got {tuple(target.shape)}")
            use = row_ok & torch.isfinite(target)
            if name in DIRECTIONAL_NAMES:      # e.g. a row with acoustically unstable directions, a bad density
                use = use & torch.isfinite(value.detach())
            zero = torch.zeros_like(value)
            diff = torch.where(use, value, zero) - torch.where(use, target, zero)
            term = (diff.abs() if self.kind == "l1" else diff * diff).sum() * self.weights[name]
            total = term if total is None else total + term
            count = use.sum() if count is None else count + use.sum()
        return total / count.clamp(min=1).to(total.dtype)
