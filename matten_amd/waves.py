"""
Group velocities, polarisations and phonon focusing of (predicted) elasticity tensors, on the device.

``elastic_properties(..., density=...)`` solves the Christoffel equation per direction and keeps the three phase velocities.
This module keeps the eigenvectors as well (``matten_elastic_waves``, csrc/waves.hip): how each acoustic mode is polarised,
where its energy goes (the group velocity and the power-flow angle between it and the wave normal -- what an ultrasonic
time-of-flight measurement sees off a symmetry axis) and how strongly the crystal focuses phonons (the enhancement factor of
phonon imaging and ballistic heat-pulse experiments).  ``acoustic_waves`` takes tensors, ``acoustic_waves_from_irreps`` the
model's irreps rows, ``predict(..., properties=True, waves=True)`` the structures; ``acoustic_waves_host`` states the
definitions in numpy.  Nothing here carries a gradient: eigenvector derivatives are singular at acoustic axes.

Definitions ("Group velocities, polarisations and phonon focusing"; all fp64; Voigt order and symmetrisation
as ``elastic_properties``).  With s = modulus_unit / density and a unit direction n:

* Gamma_ik = C_ijkl n_j n_l, eigenpairs (lambda_k, u_k) with lambda ascending, k = 0, 1, 2; phase velocity v_k = sqrt(lambda_k s).
* Unstable direction -- an eigenvalue that is not positive and finite: every output of the direction is NaN, the direction
  is counted in ``n_unstable``.
* Degenerate mode -- gap_k = min_{m != k} |lambda_k - lambda_m| / lambda_2 < ``deg_tol``: the phase velocity is still given;
  polarisation, group velocity, power-flow angle, character and Jacobian are NaN (undefined: conical refraction), the mode
  is counted in ``n_degenerate[:, k]``.
* Polarisation: the unit vector u_k with u.n >= 0; where |u.n| <= 1e-9, u.e1 >= 0; where that is <= 1e-9 too, u.e2 >= 0.
  (e1, e2) = ``elastic.pair_frame(n)``, e1 x e2 = n.  Longitudinal character (u_k.n)^2.
* Group velocity g_k = (s / v_k) P, P_j = C_ijml u_i u_m n_l (m/s); g_k.n = v_k.  Power-flow angle
  psi_k = acos(min(1, v_k / |g_k|)).
* Focusing Jacobian J_k = g^ . (d_e1 g^ x d_e2 g^), g^ = g_k / |g_k|: the signed Jacobian of n -> g^ between unit spheres.
  1 / |J_k| is the phonon-focusing enhancement factor (infinite on a caustic); J < 0 marks a folded sheet.
"""
import numpy as np
import torch

from . import ops
from .elastic import (FLAG_FAILED_STRUCTURE, FLAG_SINGULAR, _as_rows, _check_number, _check_per_row, _host_voigt, _upload,
                      check_directions, pair_frame, voigt_to_cartesian)

SIGN_EPS = 1e-9      # below this |u.n| (then |u.e1|) does not decide the sign of a polarisation
SCAL_NAMES = ("phase_velocity", "group_speed", "power_flow_angle", "longitudinal_character", "focusing_jacobian")


class AcousticWaves:
    """Batch of acoustic-wave properties over B crystals, D directions and the three branches (ascending phase velocity):
    ``phase_velocity``, ``group_speed``, ``power_flow_angle`` (rad), ``longitudinal_character``, ``focusing_jacobian``,
    ``enhancement`` (= 1 / |J|, inf on a caustic) [B,D,3]; ``polarisation`` and ``group_velocity`` [B,D,3,3] (branch,
    component) -- all None when the directional maps were not kept; ``power_flow_angle_max`` [B,3] with
    ``power_flow_angle_max_index`` (the direction where it is taken; -1 where no mode of the branch is defined),
    ``focusing_min_jacobian`` [B,3] (the smallest |J|: the strongest focusing on the grid) with
    ``focusing_min_jacobian_index``; ``n_degenerate`` [B,3] and ``n_unstable`` [B] int32; ``flags`` [B] int32 as in
    ``ElasticProperties``; ``directions`` [D,3].  A row with flag bit 0 or a density that is not positive and finite is NaN
    with -1 in every integer field.  An unbatched input gives the same without the leading dimension."""

    def __init__(self, **fields):
        self._names = tuple(fields)
        for k, v in fields.items():
            setattr(self, k, v)

    def _map(self, fn) -> "AcousticWaves":
        return AcousticWaves(**{k: (None if getattr(self, k) is None else fn(getattr(self, k))) for k in self._names})

    def cpu(self) -> "AcousticWaves":
        return self._map(lambda t: t.cpu())

    def to_dict(self) -> dict:
        """name -> numpy array on the host (None for directional maps that were not kept)"""
        return {k: (None if getattr(self, k) is None else getattr(self, k).detach().cpu().numpy()) for k in self._names}

    def __repr__(self):
        return f"AcousticWaves(batch={tuple(self.flags.shape)}, directions={self.directions.shape[0]})"


def check_deg_tol(deg_tol) -> float:
    return _check_number(deg_tol, "deg_tol", 0.0)


def _fields(pol, group, scal, ext, arg, n_degenerate, n_unstable, flags, dirs, single: bool) -> AcousticWaves:
    fields = {}
    for q, name in enumerate(SCAL_NAMES):
        fields[name] = None if scal is None else scal[..., q]
    fields["enhancement"] = None if scal is None else 1.0 / scal[..., 4].abs()
    fields["polarisation"], fields["group_velocity"] = pol, group
    fields["power_flow_angle_max"], fields["power_flow_angle_max_index"] = ext[:, 0:3], arg[:, 0:3]
    fields["focusing_min_jacobian"], fields["focusing_min_jacobian_index"] = ext[:, 3:6], arg[:, 3:6]
    fields["n_degenerate"], fields["n_unstable"], fields["flags"] = n_degenerate, n_unstable, flags
    if single:
        fields = {k: (None if v is None else v[0]) for k, v in fields.items()}
    fields["directions"] = dirs
    return AcousticWaves(**fields)


def waves_from_voigt(voigt, flags, density, dirs, modulus_unit: float = 1e9, deg_tol: float = 1e-6,
                     keep_directional: bool = True, single: bool = False) -> AcousticWaves:
    """``voigt`` [B,6,6] / ``flags`` [B] as ``matten_elastic_props`` wrote them (device), ``density`` out of
    ``_check_per_row``, ``dirs`` [D,3] unit vectors (host array out of ``check_directions``, or already on the device)"""
    if not isinstance(dirs, torch.Tensor):
        dirs = torch.from_numpy(np.ascontiguousarray(dirs)).to(voigt.device)
    rho = torch.as_tensor(density, dtype=torch.float64).to(voigt.device)
    out = ops.elastic_waves(voigt, flags, rho, dirs, modulus_unit, deg_tol, keep=keep_directional)
    return _fields(*out, flags, dirs, single)


def acoustic_waves(tensors, density, directions, modulus_unit: float = 1e9, deg_tol: float = 1e-6,
                   keep_directional: bool = True) -> AcousticWaves:
    """``tensors``: as ``elastic.elastic_properties`` takes them ([B,3,3,3,3], [B,6,6], unbatched, or a list as ``predict``
    returns; fp32 or fp64; device or host, copied once).  ``density``: [B] (a scalar for an unbatched input) in kg/m^3;
    ``directions``: an int D (``fibonacci_hemisphere(D)``) or an array [D,3]; ``modulus_unit``: Pa per unit of the input
    (1e9: GPa); ``deg_tol``: the relative eigenvalue gap below which a mode counts as degenerate (finite, >= 0).  Host
    arguments are checked before anything is uploaded.  ``keep_directional=False`` returns the extremes and the counts
    only (the per-direction fields are None).  The results stay on the device."""
    deg_tol = check_deg_tol(deg_tol)
    dirs = check_directions(directions)
    rows, layout, single, failed = _as_rows(tensors)
    density = _check_per_row("density", density, rows.shape[0], single)
    voigt, _, _, flags = ops.elastic_props(_upload(rows), layout)
    if failed is not None and failed.any():
        flags |= torch.as_tensor(failed.astype(np.int32) * FLAG_FAILED_STRUCTURE, device=flags.device)
    return waves_from_voigt(voigt, flags, density, dirs, modulus_unit, deg_tol, keep_directional, single)


def acoustic_waves_from_irreps(x, density, directions, formula: str = "ijkl=jikl=klij", modulus_unit: float = 1e9,
                               deg_tol: float = 1e-6, keep_directional: bool = True) -> AcousticWaves:
    """The same from the model's irreps rows ``x`` [B,21] (fp32, on the device): one ``dense_rows`` with
    ``elastic.voigt_basis`` gives the Voigt matrices directly, as in ``elastic_properties_from_irreps``."""
    from .elastic import _VOIGT_Q, _default_device, voigt_basis

    if not isinstance(x, torch.Tensor) or x.dim() not in (1, 2):
        raise ValueError("x: expected a tensor [B,21] or [21]")
    deg_tol = check_deg_tol(deg_tol)
    dirs = check_directions(directions)
    single = x.dim() == 1
    x = x.detach().reshape(-1, x.shape[-1])
    density = _check_per_row("density", density, x.shape[0], single)
    V = voigt_basis(formula)
    if x.shape[1] != V.shape[0]:
        raise ValueError(f"x: expected {V.shape[0]} irreps components per row, got {x.shape[1]}")
    if not x.is_cuda:
        x = x.to(_default_device())
    key = (formula, x.device)
    if key not in _VOIGT_Q:
        _VOIGT_Q[key] = torch.tensor(V, dtype=torch.float32, device=x.device)
    voigt, _, _, flags = ops.elastic_props(ops.dense_rows(x.to(torch.float32), _VOIGT_Q[key]), 1)
    return waves_from_voigt(voigt, flags, density, dirs, modulus_unit, deg_tol, keep_directional, single)


# ---------------------------------------------------------------------------------------------------
# the definitions in numpy
# ---------------------------------------------------------------------------------------------------

def sign_rule(u, n):
    """u or -u by the sign rule of the module docstring"""
    e1, e2 = pair_frame(n)
    for axis in (n, e1):
        p = float(u @ axis)
        if abs(p) > SIGN_EPS:
            return -u if p < 0.0 else u
    return -u if float(u @ e2) < 0.0 else u


def christoffel_host(C4, n):
    """Gamma_ik = C_ijkl n_j n_l"""
    return np.einsum("ijkl,j,l->ik", C4, n, n)


def _mode_host(C4, n, frame, lam, U, k: int, s: float):
    """polarisation (sign rule applied), group velocity, |g|, psi, character and J of the non-degenerate branch k"""
    u, v = U[:, k], np.sqrt(lam[k] * s)
    P = np.einsum("ijml,i,m,l->j", C4, u, u, n)
    g = (s / v) * P
    g_abs = np.linalg.norm(g)
    gh = g / g_abs
    dgh = []
    for e in frame:
        dG = np.einsum("ijkl,j,l->ik", C4, e, n) + np.einsum("ijkl,j,l->ik", C4, n, e)
        du = sum(U[:, m] * (U[:, m] @ dG @ u) / (lam[k] - lam[m]) for m in range(3) if m != k)
        dv = s * (u @ dG @ u) / (2.0 * v)
        dP = (np.einsum("ijml,i,m,l->j", C4, du, u, n) + np.einsum("ijml,i,m,l->j", C4, u, du, n)
              + np.einsum("ijml,i,m,l->j", C4, u, u, e))
        dg = s * dP / v - g * dv / v
        dgh.append((dg - gh * (gh @ dg)) / g_abs)
    J = float(gh @ np.cross(dgh[0], dgh[1]))
    return sign_rule(u, n), g, g_abs, float(np.arccos(min(1.0, v / g_abs))), float(u @ n) ** 2, J


def _best(values, largest: bool):
    """(extreme, index) over axis 0 ignoring NaN, equal values to the lowest index; (NaN, -1) if none is finite"""
    ok = ~np.isnan(values)
    if not ok.any():
        return np.nan, -1
    filled = np.where(ok, values, -np.inf if largest else np.inf)
    i = int(np.argmax(filled) if largest else np.argmin(filled))
    return float(values[i]), i


def acoustic_waves_host(voigt, density, directions, modulus_unit: float = 1e9, deg_tol: float = 1e-6, flags=None) -> dict:
    """The definitions of the module docstring in numpy fp64 (``numpy.linalg.eigh`` per direction), what the tests hold
    ``matten_elastic_waves`` to.  ``voigt`` [B,6,6] or [6,6] (the mean of the two triangles is used), ``density`` [B] or a
    scalar, ``directions`` as ``acoustic_waves`` takes them, ``flags`` [B] as ``matten_elastic_props`` sets them, or None.
    -> dict of the fields of ``AcousticWaves`` (``flags`` left out), and ``relative_gap`` [B,D,3] = gap_k.  A row with flag
    bit 0, a non-finite entry or a density that is not positive and finite is NaN with -1 in the integer fields."""
    deg_tol = check_deg_tol(deg_tol)
    dirs = check_directions(directions)
    C, single = _host_voigt(voigt)
    B, D = C.shape[0], dirs.shape[0]
    with np.errstate(all="ignore"):
        C = 0.5 * (C + C.transpose(0, 2, 1))
    rho = np.asarray(density.detach().cpu().numpy() if isinstance(density, torch.Tensor) else density, dtype=np.float64)
    rho = np.full(B, float(rho)) if rho.ndim == 0 else rho.reshape(-1)
    if rho.shape[0] != B:
        raise ValueError(f"density: expected {B} value(s), one per tensor, got {rho.shape[0]}")
    bad = ~np.isfinite(C).all(axis=(1, 2)) | ~(np.isfinite(rho) & (rho > 0.0))
    if flags is not None:
        flags = np.asarray(flags.detach().cpu().numpy() if isinstance(flags, torch.Tensor) else flags).reshape(-1)
        if flags.shape[0] != B:
            raise ValueError(f"flags: expected {B} word(s), got {flags.shape[0]}")
        bad = bad | ((flags & FLAG_SINGULAR) != 0)

    scal = np.full((B, D, 3, 5), np.nan)
    pol, group, gap = np.full((B, D, 3, 3), np.nan), np.full((B, D, 3, 3), np.nan), np.full((B, D, 3), np.nan)
    ext, arg = np.full((B, 6), np.nan), np.full((B, 6), -1, dtype=np.int32)
    n_degenerate, n_unstable = np.full((B, 3), -1, dtype=np.int32), np.full(B, -1, dtype=np.int32)
    frames = [pair_frame(n) for n in dirs]
    for b in np.nonzero(~bad)[0]:
        C4, s = voigt_to_cartesian(C[b]), modulus_unit / rho[b]
        n_degenerate[b], n_unstable[b] = 0, 0
        for d, n in enumerate(dirs):
            lam, U = np.linalg.eigh(christoffel_host(C4, n))
            if not (np.isfinite(lam).all() and (lam > 0.0).all()):
                n_unstable[b] += 1
                continue
            scal[b, d, :, 0] = np.sqrt(lam * s)
            for k in range(3):
                gap[b, d, k] = min(abs(lam[k] - lam[m]) for m in range(3) if m != k) / lam[2]
                if gap[b, d, k] < deg_tol:
                    n_degenerate[b, k] += 1
                    continue
                pol[b, d, k], group[b, d, k], *scal[b, d, k, 1:] = _mode_host(C4, n, frames[d], lam, U, k, s)
        for k in range(3):
            ext[b, k], arg[b, k] = _best(scal[b, :, k, 2], True)
            ext[b, 3 + k], arg[b, 3 + k] = _best(np.abs(scal[b, :, k, 4]), False)
    out = {name: scal[..., q] for q, name in enumerate(SCAL_NAMES)}
    with np.errstate(divide="ignore"):
        out["enhancement"] = 1.0 / np.abs(scal[..., 4])
    out.update(polarisation=pol, group_velocity=group, power_flow_angle_max=ext[:, 0:3], power_flow_angle_max_index=arg[:, 0:3],
               focusing_min_jacobian=ext[:, 3:6], focusing_min_jacobian_index=arg[:, 3:6], n_degenerate=n_degenerate,
               n_unstable=n_unstable, relative_gap=gap)
    if single:
        out = {k: v[0] for k, v in out.items()}
    out["directions"] = dirs
    return out
