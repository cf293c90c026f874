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

``refine=True`` polishes the grid's directional extremes off the grid (``matten_elastic_refine``: a damped Newton iteration
over rotations of the pair (n, m) from each grid winner, the compressibility by a 3x3 eigen-decomposition);
``refine_extremes_host`` states the algorithm in numpy.  ``elastic_moduli*`` do not take it: the refined extremes carry no
gradient.

``kelvin=True`` adds the Kelvin (eigen-stiffness) decomposition, the eigen-decomposition of the 6x6 Mandel matrix
(``matten_elastic_kelvin``, csrc/kelvin.hip): the six Kelvin moduli, their eigenstrains (``eigenstrains``) and dilatations, a
signed stability margin and a condition number -- how far an unstable prediction is from stable, and in which mode.
``nearest_stable`` repairs a tensor (``matten_elastic_kelvin_clamp``), ``StabilityPenalty`` trains against instability on the
moduli that ``elastic_moduli*`` attach to the graph (``matten_elastic_kelvin_bwd``); ``kelvin_host`` / ``kelvin_bwd_host`` /
``nearest_stable_host`` restate them in numpy.  Conventions: INTEGRATION.md, "Kelvin moduli and mechanical stability".

``polycrystal=True`` adds the polycrystal moduli beyond Voigt, Reuss and Hill (``matten_elastic_polycrystal``,
csrc/polycrystal.hip): the Hashin-Shtrikman bounds and the self-consistent estimate of the bulk and shear modulus, for any
crystal symmetry, from the Kelvin decomposition.  ``elastic_moduli*`` attach ``k_sc`` / ``g_sc`` / ``y_sc`` / ``poisson_sc`` to the
graph (``matten_elastic_polycrystal_bwd``) and ``ModuliLoss`` takes those names: training on measured polycrystal moduli.  The
bounds carry no gradient.  ``polycrystal_host`` / ``polycrystal_bwd_host`` state the algorithm in numpy.  Conventions:
INTEGRATION.md, "Polycrystal bounds and the self-consistent estimate".
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
    With ``refine`` also, for every X of ``young_min`` / ``young_max`` / ``compressibility_min`` / ``compressibility_max`` and
    (with ``angles``) ``shear_min`` / ``shear_max`` / ``poisson_min`` / ``poisson_max``: ``X_refined`` [B], the extreme off the
    grid, ``X_refined_n`` [B,3] and (pair quantities) ``X_refined_m`` [B,3] where it is taken, ``X_refined_status`` [B] int32
    (0 converged, 1 iteration cap, 2 not refined, -1 singular row) and ``X_refined_iterations`` [B] int32.
    With ``kelvin`` also ``kelvin_moduli`` [B,6] (ascending), ``kelvin_vectors`` [B,6,6] (columns), ``kelvin_dilatation``
    [B,6], ``stability_margin`` [B] and ``kelvin_condition`` [B] (NaN where the margin is <= 0).
    With ``polycrystal`` also ``k_hs_lower`` / ``g_hs_lower`` / ``k_hs_upper`` / ``g_hs_upper`` [B] (Hashin-Shtrikman bounds),
    ``hs_media`` [B,4,2] (their comparison media (K0, G0), in that order), ``k_sc`` / ``g_sc`` / ``y_sc`` / ``poisson_sc`` [B] (the
    self-consistent estimate), ``sc_status`` [B] int32 (0 converged, 1 iteration cap, 2 not positive definite, -1 singular
    row) and ``sc_iterations`` [B] int32.
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


# ---------------------------------------------------------------------------------------------------
# refinement of the directional extremes off the grid (``refine=True``; matten_elastic_refine, csrc/elastic.hip)
# ---------------------------------------------------------------------------------------------------
# the refined extremes, in the order of the kernel's items (item = q B + b): the four of the directional kernel's ``ext``,
# then the four of the pair kernel's
REFINE_NAMES = ("young_min", "young_max", "compressibility_min", "compressibility_max", "shear_min", "shear_max",
                "poisson_min", "poisson_max")
REFINE_CONVERGED, REFINE_ITERATION_CAP, REFINE_NOT_REFINED, REFINE_SINGULAR = 0, 1, 2, -1
# constants of the iteration, the same in the kernel: the rotation angle of the central differences that give the Hessian
# from the analytic gradient (truncation h^2 ~ 4e-9, rounding eps / h ~ 4e-12 of the Hessian: Newton stays superlinear), the
# step cap in rad, the eigenvalue clamp relative to the largest magnitude, the damped retries of one step, and the
# gradient below which a step that can no longer improve the value counts as converged (an improvement g^2 / 2H under
# eps |f| cannot be seen in fp64, which is |g| <~ sqrt(2 eps) |f| ~ 2e-8 |f|; 1e-7 leaves a factor 5)
REFINE_FD_STEP = 2.0 ** -14
REFINE_MAX_STEP = 0.3
REFINE_CLAMP = 1e-3
REFINE_DAMP_TRIES = 30
REFINE_STALL_TOL = 1e-7


def _check_refine(refine, directions, refine_tol, refine_max_iter):
    """the arguments of the refinement (ValueError before anything else happens)"""
    if not refine:
        return
    if directions is None:
        raise ValueError("refine: the refinement starts at the winners of a direction set, pass directions")
    if not (isinstance(refine_tol, (float, int, np.floating, np.integer)) and not isinstance(refine_tol, bool)
            and np.isfinite(refine_tol) and refine_tol > 0.0):
        raise ValueError(f"refine_tol: expected a finite positive number, got {refine_tol!r}")
    if (isinstance(refine_max_iter, bool) or not isinstance(refine_max_iter, (int, np.integer)) or refine_max_iter < 0
            or refine_max_iter > 0x7fffffff):
        raise ValueError(f"refine_max_iter: expected an int >= 0, got {refine_max_iter!r}")


def _v6(n):
    return np.array([n[0] * n[0], n[1] * n[1], n[2] * n[2], n[1] * n[2], n[0] * n[2], n[0] * n[1]])


def _w6(n, m):
    return np.array([2.0 * n[0] * m[0], 2.0 * n[1] * m[1], 2.0 * n[2] * m[2], n[1] * m[2] + n[2] * m[1],
                     n[0] * m[2] + n[2] * m[0], n[0] * m[1] + n[1] * m[0]])


def _a3(a, x):
    """A(a) x with the symmetric A(a) = [[2 a0, a5, a4], [a5, 2 a1, a3], [a4, a3, 2 a2]]: a . v(n) = n^T A(a) n / 2 and
    a . w(n,m) = n^T A(a) m, so A(a) x is the derivative of either"""
    return np.array([2.0 * a[0] * x[0] + a[5] * x[1] + a[4] * x[2], a[5] * x[0] + 2.0 * a[1] * x[1] + a[3] * x[2],
                     a[4] * x[0] + a[3] * x[1] + 2.0 * a[2] * x[2]])


def pair_frame(n):
    """the branch-free orthonormal frame (e1, e2) of a unit vector n, as in the pair kernel"""
    sg = 1.0 if n[2] >= 0.0 else -1.0
    fa = -1.0 / (sg + n[2])
    fb = n[0] * n[1] * fa
    return (np.array([1.0 + sg * n[0] * n[0] * fa, sg * fb, -sg * n[0]]), np.array([fb, sg + n[1] * n[1] * fa, -n[1]]))


def _refine_eval(kind: int, S, n, m):
    """kind 0: E(n), 1: G(n,m), 2: nu(n,m) -> (f, df/dn, df/dm), n and m taken as independent vectors"""
    if kind == 1:
        w = _w6(n, m)
        Sw = S @ w
        f = 1.0 / (w @ Sw)
        c = -2.0 * f * f
        return f, c * _a3(Sw, m), c * _a3(Sw, n)
    v = _v6(n)
    Sv = S @ v
    q = v @ Sv
    if kind == 0:
        f = 1.0 / q
        return f, (-2.0 * f * f) * _a3(Sv, n), np.zeros(3)
    vm = _v6(m)
    p = Sv @ vm
    return -p / q, -_a3(S @ vm, n) / q + (2.0 * p / (q * q)) * _a3(Sv, n), -_a3(Sv, m) / q


def _rotate(w, x):
    """R(w) x, the rotation by |w| about w (Rodrigues)"""
    t2 = w @ w
    if t2 < 1e-16:
        a, b = 1.0, 0.5
    else:
        t = np.sqrt(t2)
        sh = np.sin(0.5 * t)
        a, b = np.sin(t) / t, 2.0 * sh * sh / t2
    wx = np.cross(w, x)
    return x + a * wx + b * np.cross(w, wx)


def _orthonormal(n, m):
    n = n / np.sqrt(n @ n)
    m = m - (m @ n) * n
    return n, m / np.sqrt(m @ m)


def _refine_one(kind: int, sign: float, S, n, m, tol: float, max_iter: int):
    """one extreme of E, G or nu (``sign`` +1: maximum, -1: minimum) from the start pair (n, m) -> (value, n, m, status,
    accepted steps).  F(w) = sign f(R(w) n, R(w) m) is maximised: the gradient at w = 0 is n x dF/dn + m x dF/dm; the
    Hessian is the symmetric part of that gradient's central differences over rotations by +-h about the three axes (the
    antisymmetric part is the chart's, not the function's); its eigenvalues are clamped to the ascent side, min(lambda,
    -1e-3 max|lambda|), the step is capped at 0.3 rad and taken only if the value strictly improves, else damped and tried
    again.  A step that no damping can make improve ends the iteration: the value is then stationary to fp64."""
    def grad(n_, m_):
        f, dn, dm = _refine_eval(kind, S, n_, m_)
        return sign * f, sign * (np.cross(n_, dn) + np.cross(m_, dm))

    h = REFINE_FD_STEP
    it = 0
    while True:
        F0, g = grad(n, m)
        if not np.isfinite(F0):
            return sign * F0, n, m, REFINE_NOT_REFINED, it
        scale = max(abs(F0), 1.0) if kind == 2 else abs(F0)
        gnorm = np.sqrt(g @ g)
        if gnorm <= tol * scale:
            return sign * F0, n, m, REFINE_CONVERGED, it
        if it >= max_iter:
            return sign * F0, n, m, REFINE_ITERATION_CAP, it
        D = np.empty((3, 3))
        for j in range(3):
            e = np.zeros(3)
            e[j] = h
            D[:, j] = (grad(_rotate(e, n), _rotate(e, m))[1] - grad(_rotate(-e, n), _rotate(-e, m))[1]) / (2.0 * h)
        ev, U = np.linalg.eigh(0.5 * (D + D.T))
        dl = REFINE_CLAMP * np.abs(ev).max() + 1e-300
        ug = U.T @ g
        damp, moved = 0.0, False
        for _ in range(REFINE_DAMP_TRIES):
            step = U @ (-ug / (np.minimum(ev, -dl) - damp))
            length = np.sqrt(step @ step)
            if length > REFINE_MAX_STEP:
                step = step * (REFINE_MAX_STEP / length)
            n1, m1 = _orthonormal(_rotate(step, n), _rotate(step, m))
            F1 = sign * _refine_eval(kind, S, n1, m1)[0]
            if F1 > F0:
                n, m, moved = n1, m1, True
                break
            damp = max(2.0 * damp, dl)
        if not moved:
            ok = gnorm <= max(tol, REFINE_STALL_TOL) * scale
            return sign * F0, n, m, REFINE_CONVERGED if ok else REFINE_ITERATION_CAP, it
        it += 1


def compressibility_matrix(S):
    """B_ij = sum_k S_ijkk as a symmetric 3x3 matrix from the 6x6 compliance: beta(n) = n^T B n"""
    r = S[:, 0] + S[:, 1] + S[:, 2]
    return np.array([[r[0], 0.5 * r[5], 0.5 * r[4]], [0.5 * r[5], r[1], 0.5 * r[3]], [0.5 * r[4], 0.5 * r[3], r[2]]])


def _grid_winners(S, dirs, table):
    """the grid pass of the directional and the pair kernel in numpy: name -> (value, direction index, angle index); equal
    values go to the lowest (flat) index, NaN is never taken, (nan, -1, -1) if nothing compares"""
    V = np.stack([dirs[:, 0] ** 2, dirs[:, 1] ** 2, dirs[:, 2] ** 2, dirs[:, 1] * dirs[:, 2], dirs[:, 0] * dirs[:, 2],
                  dirs[:, 0] * dirs[:, 1]], axis=1)
    SV = V @ S
    q = np.einsum("di,di->d", V, SV)
    with np.errstate(all="ignore"):
        maps = {"young": (1.0 / q)[:, None], "compressibility": (V @ (S[:, 0] + S[:, 1] + S[:, 2]))[:, None]}
        if table is not None:
            E12 = [pair_frame(n) for n in dirs]
            e1, e2 = np.array([e[0] for e in E12]), np.array([e[1] for e in E12])
            m = table[None, :, 0, None] * e1[:, None, :] + table[None, :, 1, None] * e2[:, None, :]      # [D,M,3]
            n = dirs[:, None, :]
            W = np.stack([2.0 * n[..., 0] * m[..., 0], 2.0 * n[..., 1] * m[..., 1], 2.0 * n[..., 2] * m[..., 2],
                          n[..., 1] * m[..., 2] + n[..., 2] * m[..., 1], n[..., 0] * m[..., 2] + n[..., 2] * m[..., 0],
                          n[..., 0] * m[..., 1] + n[..., 1] * m[..., 0]], axis=-1)
            VM = np.stack([m[..., 0] ** 2, m[..., 1] ** 2, m[..., 2] ** 2, m[..., 1] * m[..., 2], m[..., 0] * m[..., 2],
                           m[..., 0] * m[..., 1]], axis=-1)
            maps["shear"] = 1.0 / np.einsum("dki,ij,dkj->dk", W, S, W)
            maps["poisson"] = -np.einsum("di,dki->dk", SV, VM) / q[:, None]
    out = {}
    for name, f in maps.items():
        for side, fill, pick in (("min", np.inf, np.argmin), ("max", -np.inf, np.argmax)):
            flat = f.reshape(-1)
            if np.isnan(flat).all():
                out[f"{name}_{side}"] = (np.nan, -1, -1)
                continue
            i = int(pick(np.where(np.isnan(flat), fill, flat)))
            out[f"{name}_{side}"] = (flat[i], i // f.shape[1], i % f.shape[1])
    return out


def refine_extremes_host(compliance, directions, angles=None, tol: float = 1e-9, max_iter: int = 32, flags=None) -> dict:
    """The refinement of ``refine=True`` restated in numpy fp64 -- the documented algorithm, which the kernel follows step
    for step.  ``compliance`` [B,6,6] or [6,6] (engineering convention, the mean of its two triangles is used),
    ``directions`` / ``angles`` as in ``elastic_properties``, ``flags`` [B] as ``matten_elastic_props`` sets them (None: bit
    0 for a non-finite row, bit 1 for one that is not positive definite).  -> name -> dict(value [B], n [B,3], m [B,3],
    status [B], iterations [B], grid_value [B], grid_direction [B], grid_angle [B]) for the names of ``REFINE_NAMES`` (the
    first four without ``angles``).

    Per extreme: the grid pass picks the winner (d, k) as the kernels do, the start pair is n = directions[d],
    m = cos(chi_k) e1 + sin(chi_k) e2 in ``pair_frame(n)``, and ``_refine_one`` polishes it; the result is the stationary
    point of the basin the winner lies in.  The compressibility's extremes are the extreme eigenvalues of
    ``compressibility_matrix`` with their eigenvectors, no iteration.  A result that rounding left behind the grid value
    gives way to the grid's value and pair.  Status: 0 converged, 1 iteration cap reached (the value is still no worse
    than the grid's), 2 not refined (flag bit 1: grid value and pair copied), -1 flag bit 0 (NaN)."""
    S_all = np.asarray(compliance, dtype=np.float64)
    single = S_all.ndim == 2
    S_all = S_all.reshape(-1, 6, 6)
    S_all = 0.5 * (S_all + S_all.transpose(0, 2, 1))
    B = S_all.shape[0]
    dirs = check_directions(directions)
    table = None if angles is None else angle_table(angles)
    if flags is None:
        flags = np.zeros(B, dtype=np.int32)
        for b in range(B):
            if not np.isfinite(S_all[b]).all():
                flags[b] = FLAG_SINGULAR | FLAG_NOT_POSITIVE_DEFINITE
            elif not (np.linalg.eigvalsh(S_all[b]) > 0.0).all():
                flags[b] = FLAG_NOT_POSITIVE_DEFINITE
    flags = np.asarray(flags).reshape(-1)
    names = REFINE_NAMES if table is not None else REFINE_NAMES[:4]
    out = {name: dict(value=np.full(B, np.nan), n=np.full((B, 3), np.nan), m=np.full((B, 3), np.nan),
                      status=np.full(B, REFINE_SINGULAR, dtype=np.int32), iterations=np.zeros(B, dtype=np.int32),
                      grid_value=np.full(B, np.nan), grid_direction=np.full(B, -1, dtype=np.int64),
                      grid_angle=np.full(B, -1, dtype=np.int64)) for name in names}
    for b in range(B):
        if flags[b] & FLAG_SINGULAR:
            continue
        S = S_all[b]
        winners = _grid_winners(S, dirs, table)
        for name in names:
            o = out[name]
            grid, d, k = winners[name]
            o["grid_value"][b], o["grid_direction"][b], o["grid_angle"][b] = grid, d, k
            if d < 0:
                continue
            n0 = dirs[d]
            e1, e2 = pair_frame(n0)
            m0 = e1 if table is None or name.startswith(("young", "compressibility")) else table[k, 0] * e1 + table[k, 1] * e2
            sign = 1.0 if name.endswith("_max") else -1.0
            if flags[b] & FLAG_NOT_POSITIVE_DEFINITE:
                value, n, m, status, it = grid, n0, m0, REFINE_NOT_REFINED, 0
            elif name.startswith("compressibility"):
                ev, U = np.linalg.eigh(compressibility_matrix(S))
                i = 2 if sign > 0 else 0
                value, n, m, status, it = ev[i], U[:, i], U[:, 1], REFINE_CONVERGED, 0
            else:
                kind = 0 if name.startswith("young") else 1 if name.startswith("shear") else 2
                value, n, m, status, it = _refine_one(kind, sign, S, n0, m0, float(tol), int(max_iter))
                if status == REFINE_NOT_REFINED:
                    value = grid
            if not sign * value >= sign * grid:       # (rounding alone can leave it behind; also a NaN)
                value, n, m = grid, n0, m0
            o["value"][b], o["n"][b], o["m"][b], o["status"][b], o["iterations"][b] = value, n, m, status, it
    if single:
        out = {name: {k: v[0] for k, v in o.items()} for name, o in out.items()}
    return out


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


# ---------------------------------------------------------------------------------------------------
# Kelvin (eigen-stiffness) decomposition (``kelvin=True``; matten_elastic_kelvin, csrc/kelvin.hip)
# ---------------------------------------------------------------------------------------------------
KELVIN_NAMES = ("kelvin_moduli", "kelvin_vectors", "kelvin_dilatation", "stability_margin", "kelvin_condition")
# the Mandel factors d_I d_J of C^ = D C D, D = diag(1,1,1,sqrt2,sqrt2,sqrt2): 1, sqrt2 and exactly 2 (not sqrt2 * sqrt2),
# as in the kernel
_MANDEL_D = np.array([1.0, 1.0, 1.0, np.sqrt(2.0), np.sqrt(2.0), np.sqrt(2.0)])
MANDEL_WEIGHT = np.where(np.arange(6)[:, None] < 3, np.where(np.arange(6)[None, :] < 3, 1.0, np.sqrt(2.0)),
                         np.where(np.arange(6)[None, :] < 3, np.sqrt(2.0), 2.0))
MANDEL_UNWEIGHT = np.where(MANDEL_WEIGHT == 1.0, 1.0, np.where(MANDEL_WEIGHT == 2.0, 0.5, 0.70710678118654757))
# Voigt index of a Cartesian pair: C_ijkl = C_IJ with I = _VOIGT_OF[i, j], J = _VOIGT_OF[k, l]
_VOIGT_OF = np.array([[0, 5, 4], [5, 1, 3], [4, 3, 2]])


def _check_kelvin(kelvin):
    if not isinstance(kelvin, (bool, np.bool_)):
        raise ValueError(f"kelvin: expected True or False, got {kelvin!r}")


def _check_number(value, name: str, lowest=None) -> float:
    """a finite real number, python or numpy (not a bool, not a string), at least `lowest` -> float; else ValueError: the
    one check of ``floor``, ``margin`` and ``weight``"""
    if (isinstance(value, (bool, np.bool_)) or not isinstance(value, (float, int, np.floating, np.integer))
            or not np.isfinite(value) or (lowest is not None and value < lowest)):
        raise ValueError(f"{name}: expected a finite number{'' if lowest is None else f' >= {lowest:g}'}, got {value!r}")
    return float(value)


def _check_floor(floor, name: str = "floor") -> float:
    return _check_number(floor, name, 0.0)


def _host_voigt(voigt):
    """-> ([B,6,6] fp64 numpy, unbatched?)"""
    if isinstance(voigt, torch.Tensor):
        voigt = voigt.detach().cpu().numpy()
    C = np.asarray(voigt, dtype=np.float64)
    if C.shape[-2:] != (6, 6) or C.ndim not in (2, 3):
        raise ValueError(f"voigt: expected [B,6,6] or [6,6], got {C.shape}")
    return C.reshape(-1, 6, 6), C.ndim == 2


def _host_flags(flags, C):
    """the rows the kernel writes as NaN: flag bit 0 (``flags`` None: none set), or a non-finite entry of C^"""
    with np.errstate(all="ignore"):
        Ch = MANDEL_WEIGHT * (0.5 * (C + C.transpose(0, 2, 1)))
    bad = ~np.isfinite(Ch).all(axis=(1, 2))
    if flags is not None:
        flags = np.asarray(flags.detach().cpu().numpy() if isinstance(flags, torch.Tensor) else flags).reshape(-1)
        if flags.shape[0] != C.shape[0]:
            raise ValueError(f"flags: expected {C.shape[0]} word(s), got {flags.shape[0]}")
        bad = bad | ((flags & FLAG_SINGULAR) != 0)
    return Ch, bad


def kelvin_host(voigt, flags=None) -> dict:
    """The Kelvin decomposition in numpy fp64 (``numpy.linalg.eigh``), what the tests hold ``matten_elastic_kelvin`` to.
    ``voigt`` [B,6,6] or [6,6]: the symmetrised Voigt matrix C_IJ (pymatgen order, no factors; the mean of the two
    triangles is used), ``flags`` [B] as ``matten_elastic_props`` sets them, or None.  With C^ = D C D,
    D = diag(1,1,1,sqrt2,sqrt2,sqrt2) -> dict of ``kelvin_moduli`` [B,6] (eigenvalues of C^, ascending), ``kelvin_vectors``
    [B,6,6] (orthonormal eigenvectors in the columns), ``kelvin_dilatation`` [B,6] = (tr eps_k)^2 / 3, ``stability_margin``
    [B] = the smallest modulus, ``kelvin_condition`` [B] = largest / smallest (NaN where the smallest is <= 0), and
    ``mandel`` [B,6,6] = C^.  A row with flag bit 0 or a non-finite entry is NaN."""
    C, single = _host_voigt(voigt)
    Ch, bad = _host_flags(flags, C)
    lam, U = np.linalg.eigh(np.where(bad[:, None, None], np.eye(6), Ch))
    tr = (U[:, 0, :] + U[:, 1, :]) + U[:, 2, :]
    with np.errstate(all="ignore"):
        cond = np.where(lam[:, 0] > 0.0, lam[:, 5] / np.where(lam[:, 0] > 0.0, lam[:, 0], 1.0), np.nan)
    nan = np.nan
    out = dict(kelvin_moduli=np.where(bad[:, None], nan, lam), kelvin_vectors=np.where(bad[:, None, None], nan, U),
               kelvin_dilatation=np.where(bad[:, None], nan, tr * tr / 3.0), stability_margin=np.where(bad, nan, lam[:, 0]),
               kelvin_condition=np.where(bad, nan, cond), mandel=np.where(bad[:, None, None], nan, Ch))
    return {k: v[0] for k, v in out.items()} if single else out


def kelvin_bwd_host(voigt, g_moduli, flags=None, vectors=None) -> np.ndarray:
    """The adjoint of the Kelvin moduli in numpy fp64: ``g_moduli`` [B,6] -> g_voigt [B,6,6] = D (U diag(g_moduli) U^T) D,
    symmetric, with U of ``kelvin_host(voigt)`` or, when given, ``vectors`` [B,6,6] (the kernel's: at degenerate moduli a
    per-modulus gradient depends on the basis).  Rows with flag bit 0, a non-finite entry or non-finite vectors are zero."""
    C, single = _host_voigt(voigt)
    _, bad = _host_flags(flags, C)
    if vectors is None:
        U = kelvin_host(C, flags)["kelvin_vectors"]
    else:
        U = _host_voigt(vectors)[0]
    bad = bad | ~np.isfinite(U).all(axis=(1, 2))
    U = np.where(bad[:, None, None], 0.0, U)
    g = np.asarray(g_moduli.detach().cpu().numpy() if isinstance(g_moduli, torch.Tensor) else g_moduli, dtype=np.float64)
    g = np.where(bad[:, None], 0.0, g.reshape(-1, 6))
    out = MANDEL_WEIGHT * np.einsum("bik,bk,bjk->bij", U, g, U)
    out = np.where(bad[:, None, None], 0.0, 0.5 * (out + out.transpose(0, 2, 1)))
    return out[0] if single else out


def voigt_to_cartesian(voigt):
    """[...,6,6] -> [...,3,3,3,3], C_ijkl = C_IJ (a torch tensor or a numpy array; a gather, no arithmetic)"""
    if isinstance(voigt, torch.Tensor):
        idx = torch.as_tensor(_VOIGT_OF, device=voigt.device)
        return voigt[..., idx[:, :, None, None], idx[None, None, :, :]]
    return np.asarray(voigt)[..., _VOIGT_OF[:, :, None, None], _VOIGT_OF[None, None, :, :]]


def nearest_stable_host(voigt, floor: float = 0.0, flags=None):
    """``nearest_stable`` in numpy fp64 for Voigt matrices [B,6,6] or [6,6]: C+ = D^-1 U diag(max(l_k, floor)) U^T D^-1
    with (l, U) of ``kelvin_host`` -> (voigt [B,6,6], cartesian [B,3,3,3,3], changed [B] bool).  A row whose moduli are
    all >= floor is returned as it came; a NaN row stays NaN."""
    floor = _check_floor(floor)
    C, single = _host_voigt(voigt)
    h = kelvin_host(C, flags)
    lam, U = h["kelvin_moduli"], h["kelvin_vectors"]
    with np.errstate(invalid="ignore"):
        changed = (lam < floor).any(axis=1)
        keep = (lam >= floor).all(axis=1)
        w = np.where(lam < floor, floor, lam)
    rebuilt = MANDEL_UNWEIGHT * np.einsum("bik,bk,bjk->bij", U, w, U)
    rebuilt = 0.5 * (rebuilt + rebuilt.transpose(0, 2, 1))
    out = np.where(keep[:, None, None], C, rebuilt)
    cart = voigt_to_cartesian(out)
    return (out[0], cart[0], changed[0]) if single else (out, cart, changed)


def _kelvin_fields(moduli, vectors, dilatation) -> dict:
    """the outputs of the Kelvin kernel under their field names, with the margin and the condition number (torch
    expressions on the moduli)"""
    lo, hi = moduli[:, 0], moduli[:, 5]
    stable = lo.detach() > 0.0
    cond = torch.where(stable, hi.detach() / torch.where(stable, lo.detach(), torch.ones_like(lo)),
                       torch.full((), float("nan"), dtype=moduli.dtype, device=moduli.device))
    return dict(kelvin_moduli=moduli, kelvin_vectors=vectors, kelvin_dilatation=dilatation, stability_margin=lo,
                kelvin_condition=cond)


def eigenstrains(props):
    """The eigenstrains of the Kelvin modes as symmetric 3 x 3 tensors: ``props`` an ``ElasticProperties`` made with
    ``kelvin=True`` (or its ``kelvin_vectors``, [B,6,6] or [6,6], torch or numpy) -> [B,6,3,3] (or [6,3,3]), mode k at index
    k.  The Mandel shear components are divided by sqrt2, so every tensor has unit Frobenius norm.  No gradient."""
    U = getattr(props, "kelvin_vectors", props)
    if U is None or isinstance(U, ElasticProperties):
        raise ValueError("props: no kelvin_vectors; pass kelvin=True to elastic_properties / elastic_moduli / predict")
    if isinstance(U, torch.Tensor):
        U = U.detach()
        comp = (U * torch.as_tensor(1.0 / _MANDEL_D, dtype=U.dtype, device=U.device)[:, None]).transpose(-1, -2)   # [..., k, I]
        idx = torch.as_tensor(_VOIGT_OF, device=U.device)
        return comp[..., idx]
    U = np.asarray(U, dtype=np.float64)
    if U.shape[-2:] != (6, 6):
        raise ValueError(f"kelvin_vectors: expected [B,6,6] or [6,6], got {U.shape}")
    return np.swapaxes(U / _MANDEL_D[:, None], -1, -2)[..., _VOIGT_OF]


def nearest_stable(tensors, floor: float = 0.0):
    """The tensor nearest to each input, in the Frobenius norm of the rank-4 tensor, among those whose Kelvin moduli are all
    >= ``floor`` (finite, >= 0: else ValueError): C^+ = U diag(max(l_k, floor)) U^T on the Mandel matrix
    (``matten_elastic_kelvin_clamp``).  ``tensors`` as for ``elastic_properties`` -> (voigt [B,6,6], cartesian
    [B,3,3,3,3], changed [B] bool) on the device, fp64; an unbatched input gives an unbatched result.  A row with
    ``changed`` False is the symmetrised input, bit for bit; a row ``elastic_properties`` answers with NaN (flag bit 0)
    stays NaN and unchanged.  ``floor=0`` leaves a semi-definite tensor (flag bit 1 may stay set); a small positive floor
    gives a positive definite one.  No gradient."""
    floor = _check_floor(floor)
    rows, layout, single, _ = _as_rows(tensors)
    voigt, _, _, flags = ops.elastic_props(_upload(rows), layout)
    moduli, vectors, _ = ops.elastic_kelvin(voigt, flags, want_dilatation=False)
    out = ops.elastic_kelvin_clamp(voigt, moduli, vectors, floor)
    changed = (moduli < floor).any(dim=1)
    cart = voigt_to_cartesian(out)
    return (out[0], cart[0], changed[0]) if single else (out, cart, changed)


# ---------------------------------------------------------------------------------------------------
# polycrystal moduli: Hashin-Shtrikman bounds and the self-consistent estimate (``polycrystal=True``;
# matten_elastic_polycrystal, csrc/polycrystal.hip)
# ---------------------------------------------------------------------------------------------------
# the [B] quantities that ``elastic_moduli(polycrystal=True)`` attaches to the graph and ``ModuliLoss`` accepts, with the
# argument that produces each
POLYCRYSTAL_NAMES = {"k_sc": "polycrystal", "g_sc": "polycrystal", "y_sc": "polycrystal", "poisson_sc": "polycrystal"}
POLYCRYSTAL_FIELDS = ("k_hs_lower", "g_hs_lower", "k_hs_upper", "g_hs_upper", "k_sc", "g_sc", "y_sc", "poisson_sc",
                      "sc_status", "sc_iterations", "hs_media")
SC_CONVERGED, SC_ITERATION_CAP, SC_NOT_POSITIVE_DEFINITE, SC_SINGULAR = 0, 1, 2, -1
# constants of the search, the same in the kernel: the relative distance the frontier grids keep from lambda_min / 2 and
# lambda_max / 2, the factor the upper grid spans, the golden-section steps after the grid and the golden ratio's inverse
HS_EDGE = 1e-12
HS_UPPER_SPAN = 4.0
HS_GOLDEN_STEPS = 60
HS_GOLDEN = 0.6180339887498949
_U6 = np.array([1.0, 1.0, 1.0, 0.0, 0.0, 0.0]) / np.sqrt(3.0)
_J6 = np.outer(_U6, _U6)
_K6 = np.eye(6) - _J6


def _check_polycrystal(polycrystal, hs_grid=64, sc_tol=1e-12, sc_max_iter=200):
    """the arguments of the polycrystal moduli (ValueError before anything else happens)"""
    if not isinstance(polycrystal, (bool, np.bool_)):
        raise ValueError(f"polycrystal: expected True or False, got {polycrystal!r}")
    if not polycrystal:
        return
    if isinstance(hs_grid, (bool, np.bool_)) or not isinstance(hs_grid, (int, np.integer)) or not 2 <= hs_grid <= 0x7fffffff:
        raise ValueError(f"hs_grid: expected an int >= 2, got {hs_grid!r}")
    if (isinstance(sc_tol, (bool, np.bool_)) or not isinstance(sc_tol, (float, int, np.floating, np.integer))
            or not np.isfinite(sc_tol) or not sc_tol > 0.0):
        raise ValueError(f"sc_tol: expected a finite positive number, got {sc_tol!r}")
    if (isinstance(sc_max_iter, (bool, np.bool_)) or not isinstance(sc_max_iter, (int, np.integer))
            or not 1 <= sc_max_iter <= 0x7fffffff):
        raise ValueError(f"sc_max_iter: expected an int >= 1, got {sc_max_iter!r}")


def iso_mandel(K, G):
    """iso(K, G) = 3K J + 2G K_d as Mandel matrices [...,6,6]"""
    K, G = np.asarray(K, dtype=np.float64), np.asarray(G, dtype=np.float64)
    return 3.0 * K[..., None, None] * _J6 + 2.0 * G[..., None, None] * _K6


def polarisation_mandel(K0, G0):
    """Hill's polarisation tensor of a sphere in the isotropic medium (K0, G0), as Mandel matrices [...,6,6]"""
    K0, G0 = np.asarray(K0, dtype=np.float64), np.asarray(G0, dtype=np.float64)
    pj = 1.0 / (3.0 * K0 + 4.0 * G0)
    pk = 3.0 * (K0 + 2.0 * G0) / (5.0 * G0 * (3.0 * K0 + 4.0 * G0))
    return pj[..., None, None] * _J6 + pk[..., None, None] * _K6


def _c_jk(T):
    """the isotropic projections (c_J, c_K) of Mandel matrices [...,6,6]: the orientation average is c_J J + c_K K_d"""
    cj = np.einsum("i,...ij,j->...", _U6, T, _U6)
    return cj, (np.trace(T, axis1=-2, axis2=-1) - cj) / 5.0


def polycrystal_F(mandel, K0, G0):
    """F(C^; K0, G0) -> (F_K, F_G) as documented, by the definition: R = C^ - iso(K0, G0), A = (1 + P R)^-1,
    F_K = c_J(C^ A) / 3 c_J(A), F_G = c_K(C^ A) / 2 c_K(A).  ``mandel`` [...,6,6], K0 / G0 [...] (broadcast)."""
    Ch = np.asarray(mandel, dtype=np.float64)
    K0, G0 = np.broadcast_arrays(np.asarray(K0, dtype=np.float64), np.asarray(G0, dtype=np.float64))
    A = np.linalg.inv(np.eye(6) + polarisation_mandel(K0, G0) @ (Ch - iso_mandel(K0, G0)))
    aj, ak = _c_jk(A)
    cj, ck = _c_jk(Ch @ A)
    return cj / (3.0 * aj), ck / (2.0 * ak)


def _hs_frontier_k0(lam, w, G0, upper: bool):
    """K0 of the frontier medium at G0: the largest (lower frontier) or smallest (upper) K0 with C^ - iso(K0, G0) still
    positive (negative) semi-definite; lam [B,6] ascending, w [B,6] = (U_k . u)^2, G0 [B]"""
    if upper:
        return (2.0 * G0 - 1.0 / (w / (2.0 * G0[:, None] - lam)).sum(axis=1)) / 3.0
    return (2.0 * G0 + 1.0 / (w / (lam - 2.0 * G0[:, None])).sum(axis=1)) / 3.0


def _hs_grid_g0(lam, i, M: int, upper: bool):
    """the grid point i of the frontier (lower: i = 1..M, i = 0 is G0 = 0 and never evaluated; upper: i = 0..M-1)"""
    if upper:
        return (0.5 * lam[:, 5] * (1.0 + HS_EDGE)) * np.exp2(np.log2(HS_UPPER_SPAN) * i / (M - 1))
    return (0.5 * lam[:, 0] * (1.0 - HS_EDGE)) * (i / M)


def _hs_search(Ch, lam, w, M: int, upper: bool):
    """the two searches along one frontier, for all rows at once -> (value [B,2], medium [B,2,2]): index 0 the bound on
    K, 1 the bound on G; medium[:, q] = (K0, G0) where it was found.  The grid, then ``HS_GOLDEN_STEPS`` golden-section
    steps in the bracket of the grid winner's two neighbours; the best point visited is kept (strictly better only: the
    first wins a tie, a NaN never wins)."""
    B = lam.shape[0]
    sign = -1.0 if upper else 1.0

    def evaluate(G0):
        K0 = _hs_frontier_k0(lam, w, G0, upper)
        FK, FG = polycrystal_F(Ch, K0, G0)
        return K0, (FK, FG)

    first, last = (0, M - 1) if upper else (1, M)
    best = np.full((B, 2), -np.inf)          # of sign * F
    medium = np.full((B, 2, 2), np.nan)
    winner = np.full((B, 2), first, dtype=np.int64)

    def keep(q, f, K0, G0):
        take = sign * f > best[:, q]
        best[:, q] = np.where(take, sign * f, best[:, q])
        medium[:, q, 0] = np.where(take, K0, medium[:, q, 0])
        medium[:, q, 1] = np.where(take, G0, medium[:, q, 1])
        return take

    for i in range(first, last + 1):
        G0 = _hs_grid_g0(lam, np.full(B, float(i)), M, upper)
        K0, F = evaluate(G0)
        for q in (0, 1):
            winner[:, q] = np.where(keep(q, F[q], K0, G0), i, winner[:, q])
    for q in (0, 1):
        a = _hs_grid_g0(lam, np.maximum(winner[:, q] - 1, 0).astype(np.float64), M, upper)
        b = _hs_grid_g0(lam, np.minimum(winner[:, q] + 1, last).astype(np.float64), M, upper)
        x1, x2 = b - HS_GOLDEN * (b - a), a + HS_GOLDEN * (b - a)
        K1, F1 = evaluate(x1)
        K2, F2 = evaluate(x2)
        f1, f2 = sign * F1[q], sign * F2[q]
        keep(q, F1[q], K1, x1)
        keep(q, F2[q], K2, x2)
        for _ in range(HS_GOLDEN_STEPS):
            left = f1 > f2                       # the maximum is in [a, x2]
            b = np.where(left, x2, b)
            a = np.where(left, a, x1)
            xn = np.where(left, b - HS_GOLDEN * (b - a), a + HS_GOLDEN * (b - a))
            Kn, Fn = evaluate(xn)
            fn = sign * Fn[q]
            keep(q, Fn[q], Kn, xn)
            x1, x2, f1, f2 = (np.where(left, xn, x2), np.where(left, x1, xn), np.where(left, fn, f2),
                              np.where(left, f1, fn))
    return sign * best, medium


def _polycrystal_rows(voigt, flags):
    """-> (C^ [B,6,6] with bad rows replaced by the identity, lam [B,6], w [B,6], singular [B], not_pd [B], unbatched?)"""
    C, single = _host_voigt(voigt)
    Ch, singular = _host_flags(flags, C)
    not_pd = np.zeros(C.shape[0], dtype=bool)
    if flags is not None:
        f = np.asarray(flags.detach().cpu().numpy() if isinstance(flags, torch.Tensor) else flags).reshape(-1)
        not_pd = (f & FLAG_NOT_POSITIVE_DEFINITE) != 0
    Ch = np.where(singular[:, None, None], np.eye(6), Ch)
    lam, U = np.linalg.eigh(Ch)
    not_pd = (not_pd | ~(lam[:, 0] > 0.0)) & ~singular
    Ch = np.where(not_pd[:, None, None], np.eye(6), Ch)
    lam, U = np.where(not_pd[:, None], 1.0, lam), np.where(not_pd[:, None, None], np.eye(6), U)
    w = ((U[:, 0, :] + U[:, 1, :]) + U[:, 2, :]) ** 2 / 3.0
    return Ch, lam, w, singular, not_pd, single


def _sc_iterate(Ch, lam, w, sc_tol: float, sc_max_iter: int):
    """the fixed point (K, G) = F(C^; K, G) from the Voigt pair, all rows at once -> (K [B], G [B], status [B],
    iterations [B])"""
    B = lam.shape[0]
    wl = (w * lam).sum(axis=1)
    K, G = wl / 3.0, (lam.sum(axis=1) - wl) / 10.0
    active = np.ones(B, dtype=bool)
    status = np.full(B, SC_ITERATION_CAP, dtype=np.int32)
    iterations = np.zeros(B, dtype=np.int32)
    for _ in range(int(sc_max_iter)):
        Kn, Gn = polycrystal_F(Ch, K, G)
        iterations[active] += 1
        done = active & (np.abs(Kn - K) + np.abs(Gn - G) <= sc_tol * (Kn + Gn))
        K, G = np.where(active, Kn, K), np.where(active, Gn, G)
        status[done] = SC_CONVERGED
        active = active & ~done
        if not active.any():
            break
    return K, G, status, iterations


def polycrystal_host(voigt, hs_grid: int = 64, sc_tol: float = 1e-12, sc_max_iter: int = 200, flags=None) -> dict:
    """The polycrystal moduli in numpy fp64 -- the documented algorithm ("Polycrystal bounds and the
    self-consistent estimate"), what the tests hold ``matten_elastic_polycrystal`` to.  ``voigt`` [B,6,6] or [6,6]: the Voigt
    matrix C_IJ (the mean of its two triangles is used), ``flags`` [B] as ``matten_elastic_props`` sets them, or None.
    F is evaluated by its definition (``polycrystal_F``: one 6x6 inverse per point); the frontiers come from
    ``numpy.linalg.eigh`` of the Mandel matrix.  -> dict of ``k_hs_lower``, ``g_hs_lower``, ``k_sc``, ``g_sc``, ``k_hs_upper``,
    ``g_hs_upper``, ``y_sc`` = 9KG / (3K + G), ``poisson_sc`` = (3K - 2G) / (6K + 2G) [B], ``sc_status`` [B] int32 (0 converged,
    1 iteration cap: the last iterate, 2 not positive definite: NaN, -1 flag bit 0 or a non-finite entry: NaN),
    ``sc_iterations`` [B] int32 and ``hs_media`` [B,4,2]: the comparison medium (K0, G0) of ``k_hs_lower``, ``g_hs_lower``,
    ``k_hs_upper``, ``g_hs_upper``.  A row counts as not positive definite with flag bit 1 or a smallest Kelvin modulus
    that is not > 0."""
    _check_polycrystal(True, hs_grid, sc_tol, sc_max_iter)
    Ch, lam, w, singular, not_pd, single = _polycrystal_rows(voigt, flags)
    bad = singular | not_pd
    with np.errstate(all="ignore"):
        K, G, status, iterations = _sc_iterate(Ch, lam, w, float(sc_tol), int(sc_max_iter))
        lower, media_lo = _hs_search(Ch, lam, w, int(hs_grid), False)
        upper, media_up = _hs_search(Ch, lam, w, int(hs_grid), True)
        nan = np.nan
        K, G = np.where(bad, nan, K), np.where(bad, nan, G)
        out = dict(k_hs_lower=np.where(bad, nan, lower[:, 0]), g_hs_lower=np.where(bad, nan, lower[:, 1]), k_sc=K, g_sc=G,
                   k_hs_upper=np.where(bad, nan, upper[:, 0]), g_hs_upper=np.where(bad, nan, upper[:, 1]),
                   y_sc=9.0 * K * G / (3.0 * K + G), poisson_sc=(3.0 * K - 2.0 * G) / (6.0 * K + 2.0 * G),
                   sc_status=np.where(singular, SC_SINGULAR, np.where(not_pd, SC_NOT_POSITIVE_DEFINITE, status)).astype(np.int32),
                   sc_iterations=np.where(bad, 0, iterations).astype(np.int32),
                   hs_media=np.where(bad[:, None, None], nan, np.concatenate([media_lo, media_up], axis=1)))
    return {k: v[0] for k, v in out.items()} if single else out


def polycrystal_bwd_host(voigt, g_sc, flags=None, sc=None, sc_tol: float = 1e-12, sc_max_iter: int = 200) -> np.ndarray:
    """The adjoint of the self-consistent pair in numpy fp64: ``g_sc`` [B,2] (the upstream gradients of k_sc and g_sc) ->
    g_voigt [B,6,6], symmetric.  ``sc``: (k_sc [B], g_sc [B], sc_status [B]) as a forward returned them (None: those of
    ``polycrystal_host``).  With x = (K, G) the fixed point of F and M = (C^ + C*)^-1, C* = 4G J + b K_d,
    b = G (9K + 8G) / 3 (K + 2G), v = M u, m_J = u . v, m_K = (tr M - m_J) / 5:
    dF_K/dC^ = v v^T / 3 m_J^2, dF_G/dC^ = (M^2 - v v^T) / 10 m_K^2; dF/dx is analytic as well (through C*: dM =
    -M dC* M); (1 - dF/dx)^T l = g is a 2x2 solve, g_C^ = l_K dF_K/dC^ + l_G dF_G/dC^ and g_voigt = D g_C^ D.  Rows with
    status -1 or 2 are zero."""
    C, single = _host_voigt(voigt)
    Ch, _ = _host_flags(flags, C)
    g = np.asarray(g_sc.detach().cpu().numpy() if isinstance(g_sc, torch.Tensor) else g_sc, dtype=np.float64).reshape(-1, 2)
    if sc is None:
        rows = _polycrystal_rows(C, flags)
        K, G, status, _ = _sc_iterate(rows[0], rows[1], rows[2], float(sc_tol), int(sc_max_iter))
        status = np.where(rows[3], SC_SINGULAR, np.where(rows[4], SC_NOT_POSITIVE_DEFINITE, status))
    else:
        K, G, status = (np.asarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t).reshape(-1) for t in sc)
    status = np.asarray(status)
    bad = ((status != SC_CONVERGED) & (status != SC_ITERATION_CAP)) | ~np.isfinite(K) | ~np.isfinite(G)
    K, G = np.where(bad, 1.0, K).astype(np.float64), np.where(bad, 1.0, G).astype(np.float64)
    Ch = np.where(bad[:, None, None], np.eye(6), Ch)
    a = 4.0 * G
    b = G * (9.0 * K + 8.0 * G) / (3.0 * (K + 2.0 * G))
    M = np.linalg.inv(Ch + a[:, None, None] * _J6 + b[:, None, None] * _K6)
    v = M @ _U6
    mj = v @ _U6
    q = (v * v).sum(axis=1)
    t2 = (M * M).sum(axis=(1, 2))
    mk = (np.trace(M, axis1=1, axis2=2) - mj) / 5.0
    fk_b = (q - mj * mj) / (3.0 * mj * mj)
    fg_a = (q - mj * mj) / (10.0 * mk * mk)
    fg_b = (t2 - 2.0 * q + mj * mj) / (10.0 * mk * mk) - 0.5
    den = 3.0 * (K + 2.0 * G) ** 2
    b_k, b_g = 10.0 * G * G / den, (9.0 * K * K + 16.0 * K * G + 16.0 * G * G) / den
    j11, j12, j21, j22 = fk_b * b_k, fk_b * b_g, fg_b * b_k, 4.0 * fg_a + fg_b * b_g
    det = (1.0 - j11) * (1.0 - j22) - j12 * j21
    lk = (g[:, 0] * (1.0 - j22) + j21 * g[:, 1]) / det
    lg = ((1.0 - j11) * g[:, 1] + j12 * g[:, 0]) / det
    vv = v[:, :, None] * v[:, None, :]
    gc = (lk / (3.0 * mj * mj))[:, None, None] * vv + (lg / (10.0 * mk * mk))[:, None, None] * (M @ M - vv)
    out = MANDEL_WEIGHT * (0.5 * (gc + gc.transpose(0, 2, 1)))
    out = np.where(bad[:, None, None], 0.0, out)
    return out[0] if single else out


def _polycrystal_fields(out, media, status) -> dict:
    """the outputs of the polycrystal kernel under their field names, with Young's modulus and Poisson's ratio of the
    self-consistent pair (torch expressions on it); the Hashin-Shtrikman fields carry no gradient"""
    hs = out.detach()
    K, G = out[:, 2], out[:, 3]
    return dict(k_hs_lower=hs[:, 0], g_hs_lower=hs[:, 1], k_hs_upper=hs[:, 4], g_hs_upper=hs[:, 5], k_sc=K, g_sc=G,
                y_sc=9.0 * K * G / (3.0 * K + G), poisson_sc=(3.0 * K - 2.0 * G) / (6.0 * K + 2.0 * G),
                sc_status=status[:, 0], sc_iterations=status[:, 1], hs_media=media.reshape(-1, 4, 2))


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
               number_density=None, modulus_unit: float = 1e9, refine: bool = False, refine_tol: float = 1e-9,
               refine_max_iter: int = 32, kelvin: bool = False, polycrystal: bool = False, hs_grid: int = 64,
               sc_tol: float = 1e-12, sc_max_iter: int = 200) -> ElasticProperties:
    """rows on the device -> ElasticProperties; ``dirs``: unit vectors out of ``check_directions`` (host) or None;
    ``density`` / ``number_density``: out of ``_check_per_row`` or None; ``refine*``: checked by ``_check_refine``;
    ``kelvin``: checked by ``_check_kelvin``; ``polycrystal``, ``hs_grid``, ``sc_*``: checked by ``_check_polycrystal``"""
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
        young, beta, ext_dir, arg_dir = ops.elastic_directional(compliance, flags, dirs, keep=keep_directional)
        fields.update(_directional_fields(young, beta, ext_dir, arg_dir, dirs))
    table = ext = arg = None
    if angles is not None:
        M = int(angles)
        table = torch.from_numpy(angle_table(M)).to(rows.device)
        maps, ext, arg = ops.elastic_pair(compliance, flags, dirs, table, keep=keep_directional)
        fields["angles"] = torch.from_numpy(np.pi * np.arange(M, dtype=np.float64) / M).to(rows.device)
        for q, name in enumerate(("shear_min", "shear_max", "poisson_min", "poisson_max")):
            fields[name] = ext[:, q]
            fields[name + "_direction"], fields[name + "_angle"] = split_pair_index(arg[:, q], M)
        for q, name in enumerate(("shear_dir_min", "shear_dir_max", "poisson_dir_min", "poisson_dir_max")):
            fields[name] = None if maps is None else maps[:, :, q]
    if refine:      # (one launch on the winners just written; nothing comes back to the host)
        value, vec_n, vec_m, status, iterations = ops.elastic_refine(compliance, flags, dirs, ext_dir, arg_dir, table, ext, arg,
                                                                     refine_tol, refine_max_iter)
        for q in range(value.shape[0]):
            name = REFINE_NAMES[q] + "_refined"
            fields[name], fields[name + "_n"] = value[q], vec_n[q]
            if q >= 4:
                fields[name + "_m"] = vec_m[q]
            fields[name + "_status"], fields[name + "_iterations"] = status[q], iterations[q]
    if density is not None:
        rho = torch.as_tensor(density, dtype=torch.float64).to(rows.device)
        fields.update(_acoustic_fields(*ops.elastic_acoustic(voigt, flags, rho, dirs, modulus_unit, keep=keep_directional),
                                       dirs.shape[0], number_density))
    if kelvin:      # (after the failed-structure bit went into the flags: the kernel reads bit 0 only)
        moduli, vectors, dilatation = ops.elastic_kelvin(voigt, flags)
        fields.update(_kelvin_fields(moduli, vectors, dilatation))
    if polycrystal:      # (works from the Kelvin decomposition, whose fields appear only with ``kelvin``)
        if not kelvin:
            moduli, vectors, _ = ops.elastic_kelvin(voigt, flags, want_dilatation=False)
        fields.update(_polycrystal_fields(*ops.elastic_polycrystal(voigt, flags, moduli, vectors, hs_grid, sc_tol, sc_max_iter)))
    if single:
        fields = {k: (v if v is None or k in ("directions", "angles") else v[0]) for k, v in fields.items()}
    return ElasticProperties(**fields)


def elastic_properties(tensors, directions=None, keep_directional: bool = False, angles=None, density=None,
                       number_density=None, modulus_unit: float = 1e9, refine: bool = False, refine_tol: float = 1e-9,
                       refine_max_iter: int = 32, kelvin: bool = False, polycrystal: bool = False, hs_grid: int = 64,
                       sc_tol: float = 1e-12, sc_max_iter: int = 200) -> ElasticProperties:
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
    ``refine`` (needs ``directions``): every grid winner -- ``young_*``, ``compressibility_*`` and, with ``angles``,
    ``shear_*`` / ``poisson_*`` -- is polished off the grid on the device (``refine_extremes_host`` is the algorithm): for each
    such name X the fields ``X_refined`` [B], ``X_refined_n`` [B,3] (unit), ``X_refined_m`` [B,3] (pair quantities only; unit,
    perpendicular to n), ``X_refined_status`` [B] int32 (0 converged, 1 iteration cap, 2 not refined: the row is not positive
    definite and keeps the grid's value and pair, -1 singular row: NaN) and ``X_refined_iterations`` [B] int32 come beside
    the grid fields, which stay as they are.  ``refine_tol`` is the relative gradient residual at which the iteration stops,
    ``refine_max_iter`` its cap.  The refined extreme is the stationary point of the basin the grid winner lies in: on a
    coarse grid that need not be the global extreme.  The sign of n and of m is unspecified (all four functions are even).
    ``kelvin=True`` adds the Kelvin decomposition (``matten_elastic_kelvin``; INTEGRATION.md, "Kelvin moduli and mechanical
    stability"): ``kelvin_moduli`` [B,6] ascending, ``kelvin_vectors`` [B,6,6] (columns), ``kelvin_dilatation`` [B,6],
    ``stability_margin`` [B] (the smallest modulus, signed) and ``kelvin_condition`` [B] (NaN where the margin is <= 0);
    ``eigenstrains(props)`` gives the 3 x 3 eigenstrains.  Every other field and flag bit is the same with and without it.
    ``polycrystal=True`` adds the polycrystal moduli beyond Voigt, Reuss and Hill (``matten_elastic_polycrystal``;
    INTEGRATION.md, "Polycrystal bounds and the self-consistent estimate"): the Hashin-Shtrikman bounds ``k_hs_lower`` /
    ``g_hs_lower`` / ``k_hs_upper`` / ``g_hs_upper`` [B] with their comparison media ``hs_media`` [B,4,2] (K0, G0 in that order
    of bounds), the self-consistent estimate ``k_sc`` / ``g_sc`` with ``y_sc`` = 9KG / (3K + G) and ``poisson_sc`` =
    (3K - 2G) / (6K + 2G), ``sc_status`` [B] int32 (0 converged, 1 iteration cap: the last iterate, 2 not positive
    definite: NaN, -1 singular row: NaN) and ``sc_iterations`` [B] int32.  ``hs_grid`` (>= 2) is the number of grid points
    per frontier before the golden-section polish -- every point visited is a feasible medium, so the bounds are valid
    whatever the search does, it decides only how tight they are --, ``sc_tol`` the relative change at which the fixed-point
    iteration stops, ``sc_max_iter`` its cap.  The Kelvin kernel runs for it; its fields appear only with ``kelvin=True``.
    The results stay on the device."""
    _check_kelvin(kelvin)
    _check_polycrystal(polycrystal, hs_grid, sc_tol, sc_max_iter)
    _check_extras(directions, angles, density, number_density)
    _check_refine(refine, directions, refine_tol, refine_max_iter)
    dirs = None if directions is None else check_directions(directions)      # (before anything is uploaded)
    rows, layout, single, failed = _as_rows(tensors)
    if density is not None:
        density = _check_per_row("density", density, rows.shape[0], single)
    if number_density is not None:
        number_density = _check_per_row("number_density", number_density, rows.shape[0], single)
    return _from_rows(_upload(rows), layout, dirs, keep_directional, single, failed, angles, density, number_density,
                      modulus_unit, refine, refine_tol, refine_max_iter, kelvin, polycrystal, hs_grid, sc_tol, sc_max_iter)


_VOIGT_Q = {}


def elastic_properties_from_irreps(x, directions=None, keep_directional: bool = False,
                                   formula: str = "ijkl=jikl=klij", angles=None, density=None, number_density=None,
                                   modulus_unit: float = 1e9, refine: bool = False, refine_tol: float = 1e-9,
                                   refine_max_iter: int = 32, kelvin: bool = False, polycrystal: bool = False,
                                   hs_grid: int = 64, sc_tol: float = 1e-12, sc_max_iter: int = 200) -> ElasticProperties:
    """The same from the model's irreps rows ``x`` [B,21] (fp32, on the device): one ``dense_rows`` with ``voigt_basis``
    gives the Voigt matrices [B,36] directly -- no [B,81] Cartesian intermediate."""
    if not isinstance(x, torch.Tensor) or x.dim() not in (1, 2):
        raise ValueError("x: expected a tensor [B,21] or [21]")
    _check_kelvin(kelvin)
    _check_polycrystal(polycrystal, hs_grid, sc_tol, sc_max_iter)
    _check_extras(directions, angles, density, number_density)
    _check_refine(refine, directions, refine_tol, refine_max_iter)
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
    return _from_rows(rows, 1, dirs, keep_directional, single, None, angles, density, number_density, modulus_unit, refine,
                      refine_tol, refine_max_iter, kelvin, polycrystal, hs_grid, sc_tol, sc_max_iter)


# ---------------------------------------------------------------------------------------------------
# differentiable: training on moduli
# ---------------------------------------------------------------------------------------------------
def _moduli_fields(rows, layout, single, dirs=None, keep_directional=False, density=None, number_density=None,
                   modulus_unit: float = 1e9, kelvin: bool = False, kelvin_dilatation: bool = True, polycrystal: bool = False,
                   hs_grid: int = 64, sc_tol: float = 1e-12, sc_max_iter: int = 200) -> ElasticProperties:
    """``_from_rows`` attached to the autograd graph (no pair quantities): the same kernels, so the same bits"""
    from .autograd import ElasticAcousticFn, ElasticDirectionalFn, ElasticKelvinFn, ElasticPolycrystalFn, ElasticPropsFn

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
    if kelvin:
        moduli, vectors, dilatation = ElasticKelvinFn.apply(voigt, flags, bool(kelvin_dilatation))
        fields.update(_kelvin_fields(moduli, vectors, dilatation))
    if polycrystal:      # (the gradient goes to voigt directly: the decomposition enters detached)
        if kelvin:
            moduli = moduli.detach()
        else:
            moduli, vectors, _ = ops.elastic_kelvin(voigt.detach(), flags, want_dilatation=False)
        fields.update(_polycrystal_fields(*ElasticPolycrystalFn.apply(voigt, flags, moduli, vectors, int(hs_grid),
                                                                      float(sc_tol), int(sc_max_iter))))
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
                   modulus_unit: float = 1e9, angles=None, kelvin: bool = False,
                   kelvin_dilatation: bool = True, polycrystal: bool = False, hs_grid: int = 64, sc_tol: float = 1e-12,
                   sc_max_iter: int = 200) -> ElasticProperties:
    """The differentiable ``elastic_properties``: ``tensors`` is a device tensor [B,3,3,3,3], [B,6,6], [3,3,3,3] or [6,6],
    fp32 or fp64; ``voigt``, ``compliance`` and the ten scalars of ``PROP_NAMES`` come back attached to its autograd graph
    (``flags``, ``is_stable``, ``is_singular`` as in ``elastic_properties``).  A row with flag bit 0 is NaN and sends a zero
    gradient back; an indefinite row is differentiated like any other.  ``directions``, ``keep_directional``, ``density``,
    ``number_density`` and ``modulus_unit`` are those of ``elastic_properties`` (same validation, same values bit for
    bit); with them ``young_min`` / ``young_max``, ``compressibility_min`` / ``compressibility_max``, ``v_slow_min``,
    ``v_fast_max``, ``sum_inv_v3``, ``v_mean``, ``debye_temperature`` and, when kept, the maps ``young`` / ``compressibility``
    / ``velocities`` are attached too (``DIRECTIONAL_NAMES``); an extreme's gradient is that of the direction where it was
    found, an acoustically unstable direction contributes nothing.  The directions and densities receive no gradient.
    ``angles`` is refused: the pair quantities carry no gradient.  ``kelvin=True`` adds the Kelvin fields of
    ``elastic_properties``: ``kelvin_moduli`` and ``stability_margin`` are attached to the graph
    (``matten_elastic_kelvin_bwd``; what ``StabilityPenalty`` trains on), the vectors, the dilatation and
    ``kelvin_condition`` carry no gradient.  ``kelvin_dilatation=False`` leaves the dilatation out (the field is None, the
    kernel gets a null pointer for it): for a loss that reads the moduli alone, as ``graphs.stability_penalized`` does.
    ``polycrystal=True`` (with ``hs_grid``, ``sc_tol``, ``sc_max_iter``) adds the polycrystal fields of ``elastic_properties``:
    ``k_sc``, ``g_sc``, ``y_sc`` and ``poisson_sc`` are attached to the graph (``matten_elastic_polycrystal_bwd``, the
    implicit-function theorem at the fixed point; ``POLYCRYSTAL_NAMES``, what ``ModuliLoss`` accepts); the Hashin-Shtrikman
    bounds and their media are detached -- the optimal medium sits on a constraint that moves with the tensor, as the
    refined extremes do.  A row with ``sc_status`` -1 or 2 is NaN and sends a zero gradient back."""
    _check_kelvin(kelvin)
    _check_polycrystal(polycrystal, hs_grid, sc_tol, sc_max_iter)
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
                          modulus_unit, kelvin, kelvin_dilatation, polycrystal, hs_grid, sc_tol, sc_max_iter)


_VOIGT_QT = {}


def elastic_moduli_from_irreps(x, formula: str = "ijkl=jikl=klij", directions=None, keep_directional: bool = False,
                               density=None, number_density=None, modulus_unit: float = 1e9, angles=None,
                               kelvin: bool = False, kelvin_dilatation: bool = True, polycrystal: bool = False,
                               hs_grid: int = 64, sc_tol: float = 1e-12, sc_max_iter: int = 200) -> ElasticProperties:
    """The differentiable ``elastic_properties_from_irreps``: ``x`` [B,21] (or [21]) fp32 on the device, usually the model's
    output with its ``grad_fn``.  The forward is the same ``dense_rows`` with ``voigt_basis``; its adjoint is ``dense_rows``
    with the transposed basis [36,21].  The directional arguments, ``kelvin`` and ``polycrystal`` are those of
    ``elastic_moduli``."""
    from .autograd import DenseRowsFn

    _check_kelvin(kelvin)
    _check_polycrystal(polycrystal, hs_grid, sc_tol, sc_max_iter)
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
    return _moduli_fields(rows, 1, single, dirs, keep_directional, density, number_density, modulus_unit, kelvin,
                          kelvin_dilatation, polycrystal, hs_grid, sc_tol, sc_max_iter)


class ModuliLoss(torch.nn.Module):
    """Loss on scalar moduli: ``forward(props, targets)`` with ``props`` an ``ElasticProperties`` (of ``elastic_moduli`` or
    ``elastic_moduli_from_irreps``) and ``targets`` a dict name -> [B]; the mean of |difference| (``kind="l1"``) or of its
    square (``"mse"``), weighted per name, over the entries whose row has flag bit 0 clear and whose target is finite.
    ``names`` come from ``PROP_NAMES`` and ``DIRECTIONAL_NAMES`` (directional extremes, sound velocities, the Debye
    temperature: ``props`` must have been made with the directional arguments); an entry of the latter whose value is not
    finite (a row with acoustically unstable directions, say) is excluded as well.  So are the names of
    ``POLYCRYSTAL_NAMES`` (the self-consistent ``k_sc``, ``g_sc``, ``y_sc``, ``poisson_sc``: ``props`` must have been made with
    ``polycrystal=True``; a row that is not positive definite has none and is excluded).
    Excluded entries are replaced with ``torch.where``, never multiplied away, so their NaN reaches neither the value nor
    the gradient; a batch without a single entry gives a zero that is still attached to the graph."""

    def __init__(self, names=("k_vrh", "g_vrh"), weights=None, kind: str = "l1"):
        super().__init__()
        names = (names,) if isinstance(names, str) else tuple(names)
        if not names:
            raise ValueError("names: at least one property is needed")
        unknown = [n for n in names if n not in PROP_NAMES and n not in DIRECTIONAL_NAMES and n not in POLYCRYSTAL_NAMES]
        if unknown:
            raise ValueError(f"names: {unknown} not in {PROP_NAMES + tuple(DIRECTIONAL_NAMES) + tuple(POLYCRYSTAL_NAMES)}")
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
                needs = f"{POLYCRYSTAL_NAMES[name]}=True" if name in POLYCRYSTAL_NAMES else DIRECTIONAL_NAMES[name]
                raise ValueError(f"props: no {name!r}; pass {needs} to elastic_moduli / elastic_moduli_from_irreps")
            target = torch.as_tensor(targets[name], dtype=value.dtype, device=value.device)
            if target.shape != value.shape:
                raise ValueError(f"targets[{name!r}]: expected shape {tuple(value.shape)}, got {tuple(target.shape)}")
            use = row_ok & torch.isfinite(target)
            # (e.g. a row with acoustically unstable directions, a bad density, a row that is not positive definite)
            if name in DIRECTIONAL_NAMES or name in POLYCRYSTAL_NAMES:
                use = use & torch.isfinite(value.detach())
            zero = torch.zeros_like(value)
            diff = torch.where(use, value, zero) - torch.where(use, target, zero)
            term = (diff.abs() if self.kind == "l1" else diff * diff).sum() * self.weights[name]
            total = term if total is None else total + term
            count = use.sum() if count is None else count + use.sum()
        return total / count.clamp(min=1).to(total.dtype)


class StabilityPenalty(torch.nn.Module):
    """Penalty on mechanically unstable predictions: ``forward(props, n_valid=None)`` with ``props`` an ``ElasticProperties``
    made with ``kelvin=True`` (of ``elastic_moduli`` or ``elastic_moduli_from_irreps`` to train on it) returns the mean over
    the crystals and their six Kelvin modes of h(margin - l_k), h(x) = max(x, 0) for ``kind="hinge"`` and max(x, 0)^2 for
    ``"squared"``: zero exactly where every modulus is at least ``margin`` (units of the tensor).  A spectral function, so
    its gradient U diag(-h') U^T does not depend on the basis Jacobi left at degenerate moduli.  A row with flag bit 0 (or
    NaN moduli) is replaced with ``torch.where``, never multiplied away: it adds nothing to the value and gets a zero
    gradient.  ``n_valid``: the device word of a padded batch (``batch["_amd_n_valid"][2:3]``, int64 [1]); the mean then runs
    over the first ``n_valid`` crystals only, in the valid-loss kernel (``autograd.ValidLossFn`` against zeros, fp32 result),
    with no host read, so it captures; without it the mean is a torch expression in fp64."""

    def __init__(self, margin: float = 0.0, kind: str = "squared"):
        super().__init__()
        margin = _check_number(margin, "margin")
        if kind not in ("hinge", "squared"):
            raise ValueError(f"kind: expected 'hinge' or 'squared', got {kind!r}")
        self.margin, self.kind = margin, kind

    def forward(self, props: ElasticProperties, n_valid=None) -> torch.Tensor:
        lam = getattr(props, "kelvin_moduli", None)
        if lam is None:
            raise ValueError("props: no kelvin_moduli; pass kelvin=True to elastic_moduli / elastic_moduli_from_irreps")
        lam = lam.reshape(-1, 6)
        bad = ((props.flags.reshape(-1) & FLAG_SINGULAR) != 0)[:, None] | ~torch.isfinite(lam.detach())
        short = torch.relu(torch.where(bad, torch.zeros((), dtype=lam.dtype, device=lam.device), self.margin - lam))
        if n_valid is None:
            return (short if self.kind == "hinge" else short * short).mean()
        from .autograd import ValidLossFn

        short = short.to(torch.float32)
        return ValidLossFn.apply(short, torch.zeros_like(short), n_valid,
                                 ops.LOSS_KINDS["mae" if self.kind == "hinge" else "mse"])[0]
