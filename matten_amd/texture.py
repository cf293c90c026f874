"""
Textured polycrystals: the effective anisotropic elasticity tensor of an aggregate under an orientation distribution.

``elastic_properties`` gives the Voigt / Reuss / Hill scalars, the Hashin-Shtrikman bounds and the self-consistent estimate
of an UNTEXTURED polycrystal: two isotropic numbers.  Rolled sheet, drawn wire and fibre-textured films are textured; what
is asked of them is a tensor -- Young's modulus of the sheet along the rolling and the transverse direction.  This module
computes the Voigt, Reuss, Hill and geometric (Matthies & Humbert) means of single-crystal tensors over a ``Texture`` on the
device (csrc/texture.hip), for single- and multi-phase aggregates, differentiable in the tensors.

Conventions ("Textured polycrystals").  A rotation R maps crystal-frame to sample-frame components,
C'_ijkl = R_ia R_jb R_kc R_ld C_abcd; an improper R acts like -R.  Mandel form C^ = D C D, D = diag(1,1,1,sqrt2,sqrt2,sqrt2);
N(R) = D Q(R) D^-1 with Bond's matrix Q is orthogonal and C'^ = N C^ N^T.  A texture is G orientations with weights
normalised to sum 1, its operator <X> = sum_g w_g N_g X N_g^T.  An aggregate is a list of members (crystal, texture, volume
fraction), the fractions normalised per aggregate.  With S^ = (C^)^-1 and L^ = log C^:

    voigt = sum_m f_m <C^_m>      reuss = (sum_m f_m <S^_m>)^-1      hill = (voigt + reuss) / 2
    geometric = exp(sum_m f_m <L^_m>)

each returned as a Voigt stiffness matrix (pymatgen order, no factors): the convention of ``ElasticProperties.voigt``, so a
result goes straight into ``elastic_properties`` / ``elastic_moduli``.  The G orientations of a texture are reduced once
per device to a 21 x 21 operator (``Texture.operator``): the cost per crystal does not depend on G.

``texture_operator_host`` / ``texture_average_host`` / ``texture_average_bwd_host`` restate the definitions in numpy (Bond
matrices, ``numpy.linalg.inv``, ``eigh`` for log and exp): the tests hold the kernels to them.

Not here: grain shape (every mean is shape-blind), a self-consistent textured estimate, gradients with respect to
orientations, weights or fractions.
"""
from __future__ import annotations

import numpy as np
import torch

from . import elastic, ops

STATUS_OK, STATUS_NOT_POSITIVE_DEFINITE, STATUS_NO_VALUE = 0, 2, -1
SCHEMES = ("voigt", "reuss", "hill", "geometric")
ORTH_TOL = 1e-6
_PAIRS = elastic.VOIGT_PAIRS
_TRI = tuple((i, j) for i in range(6) for j in range(i, 6))


# ---------------------------------------------------------------------------------------------------
# rotations (host numpy)
# ---------------------------------------------------------------------------------------------------
def _unit(v, name: str) -> np.ndarray:
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    if v.shape != (3,) or not np.isfinite(v).all() or not np.linalg.norm(v) > 0:
        raise ValueError(f"{name}: expected a finite non-zero vector of 3, got {v!r}")
    return v / np.linalg.norm(v)


def axis_angle(axis, angle) -> np.ndarray:
    """Rodrigues: the rotation(s) by ``angle`` (radians; a scalar or [n]) about ``axis`` -> [3,3] or [n,3,3]"""
    a = _unit(axis, "axis")
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    t = np.asarray(angle, dtype=np.float64)
    return np.eye(3) + np.sin(t)[..., None, None] * K + (1.0 - np.cos(t))[..., None, None] * (K @ K)


def rotation_between(a, b) -> np.ndarray:
    """the rotation by the smallest angle with R a = b (unit vectors are made of both)"""
    a, b = _unit(a, "crystal_axis"), _unit(b, "sample_axis")
    v, c = np.cross(a, b), float(a @ b)
    if np.linalg.norm(v) < 1e-12:
        if c > 0:
            return np.eye(3)
        p = np.cross(a, np.eye(3)[np.argmin(np.abs(a))])      # antiparallel: half a turn about any perpendicular
        return axis_angle(p, np.pi)
    return axis_angle(v, np.arctan2(np.linalg.norm(v), c))


def _exp_so3(w) -> np.ndarray:
    """exp([w]_x) for w [n,3]"""
    w = np.asarray(w, dtype=np.float64).reshape(-1, 3)
    t = np.linalg.norm(w, axis=1)
    K = np.zeros((len(w), 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -w[:, 2], w[:, 1], w[:, 2], -w[:, 0], -w[:, 1], w[:, 0]
    small = t < 1e-8
    ts = np.where(small, 1.0, t)
    a = np.where(small, 1.0 - t * t / 6.0, np.sin(ts) / ts)
    b = np.where(small, 0.5 - t * t / 24.0, (1.0 - np.cos(ts)) / (ts * ts))
    return np.eye(3) + a[:, None, None] * K + b[:, None, None] * (K @ K)


def rotation_mandel(R, dtype=np.float64) -> np.ndarray:
    """N(R) = D Q(R) D^-1 for every matrix of R ([G,3,3] or [3,3]) -> [G,6,6]: the orthogonal matrix with C'^ = N C^ N^T.
    Q is Bond's matrix, Q[(ij),(kl)] = R_ik R_jl (k == l) or R_ik R_jl + R_il R_jk."""
    R = np.asarray(R, dtype=dtype).reshape(-1, 3, 3)
    d = np.array([1, 1, 1, 2, 2, 2], dtype=dtype)
    d[3:] = np.sqrt(d[3:])
    N = np.empty((len(R), 6, 6), dtype=dtype)
    for I, (i, j) in enumerate(_PAIRS):
        for J, (k, l) in enumerate(_PAIRS):
            q = R[:, i, k] * R[:, j, l] if k == l else R[:, i, k] * R[:, j, l] + R[:, i, l] * R[:, j, k]
            N[:, I, J] = q * (d[I] / d[J])
    return N


# ---------------------------------------------------------------------------------------------------
# Texture
# ---------------------------------------------------------------------------------------------------
class Texture:
    """``T`` orientation distributions, packed: ``rotations`` [G,3,3] (crystal -> sample), ``weights`` [G] or None (equal),
    ``ptr`` [T+1] or None (one texture of all G).  Validated on the host (ValueError): finite orthogonal matrices (to 1e-6;
    improper ones are accepted and act like their negative), finite non-negative weights, every texture non-empty with
    a positive weight sum.  ``validate=False`` skips that and leaves a bad texture to the device, which flags it (every
    aggregate that uses it gets status -1).  The 21 x 21 operators are computed once per device and kept."""

    def __init__(self, rotations, weights=None, ptr=None, validate: bool = True):
        if isinstance(rotations, torch.Tensor):
            rotations = rotations.detach().cpu().numpy()
        R = np.asarray(rotations, dtype=np.float64)
        if R.size == 0:
            R = R.reshape(0, 3, 3)
        if R.shape[-2:] != (3, 3) or R.ndim not in (2, 3):
            raise ValueError(f"rotations: expected [G,3,3] or [3,3], got {R.shape}")
        R = np.ascontiguousarray(R.reshape(-1, 3, 3))
        G = len(R)
        if weights is not None:
            weights = np.ascontiguousarray(np.asarray(weights, dtype=np.float64).reshape(-1))
            if weights.shape != (G,):
                raise ValueError(f"weights: expected {G} (one per rotation), got {weights.shape[0]}")
        if ptr is None:
            ptr = np.array([0, G], dtype=np.int64)
        else:
            ptr = np.ascontiguousarray(np.asarray(ptr).reshape(-1)).astype(np.int64)
            if len(ptr) < 2 or ptr[0] != 0 or ptr[-1] != G or (np.diff(ptr) < 0).any():
                raise ValueError(f"ptr: expected [T+1] ascending offsets from 0 to {G}")
        if validate:
            if not np.isfinite(R).all():
                raise ValueError("rotations: a matrix is not finite")
            skew = np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max(axis=(1, 2)) if G else np.zeros(0)
            if (skew > ORTH_TOL).any():
                raise ValueError(f"rotations: matrix {int(np.argmax(skew > ORTH_TOL))} is not orthogonal (max|R R^T - 1| = "
                                 f"{skew.max():.2e})")
            if weights is not None and not (np.isfinite(weights).all() and (weights >= 0).all()):
                raise ValueError("weights: expected finite numbers >= 0")
            for t in range(len(ptr) - 1):
                if ptr[t + 1] == ptr[t]:
                    raise ValueError(f"texture {t} is empty")
                if weights is not None and not weights[ptr[t]:ptr[t + 1]].sum() > 0:
                    raise ValueError(f"texture {t}: the weight sum is not positive")
        self.rotations, self.weights, self.ptr = R, weights, ptr
        for a in (self.rotations, self.ptr) + (() if weights is None else (weights,)):
            a.setflags(write=False)
        self._operators = {}

    def __len__(self) -> int:
        return len(self.ptr) - 1

    @property
    def sizes(self) -> np.ndarray:
        return np.diff(self.ptr)

    def operator(self, device=None, slice_len: int = ops.TEXTURE_SLICE):
        """(op [T,21,21] fp64, flags [T] int32) on ``device``, computed on first use (matten_texture_operator)"""
        device = torch.device(elastic._default_device() if device is None else device)
        key = (device, int(slice_len))
        if key not in self._operators:
            R = torch.tensor(self.rotations, device=device)
            w = None if self.weights is None else torch.tensor(self.weights, device=device)
            self._operators[key] = ops.texture_operator(R, w, torch.tensor(self.ptr, device=device), ORTH_TOL, slice_len)
        return self._operators[key]

    # ---- constructors: host numpy, deterministic
    @classmethod
    def single(cls, R) -> "Texture":
        """one orientation: every mean is the rotated tensor"""
        R = np.asarray(R, dtype=np.float64)
        if R.shape != (3, 3):
            raise ValueError(f"R: expected [3,3], got {R.shape}")
        return cls(R[None])

    @classmethod
    def uniform(cls) -> "Texture":
        """No texture: the 60 rotations of the icosahedral group (generators: a 5-fold turn about (0,1,phi), a 3-fold about
        (1,1,1)).  The group has no invariants for 1 <= l <= 5, so its mean of a rank-4 tensor is the full orientation
        average, exactly."""
        from .symmetry import group_closure

        phi = 0.5 * (1.0 + np.sqrt(5.0))
        gens = np.stack([axis_angle((0.0, 1.0, phi), 2.0 * np.pi / 5.0), axis_angle((1.0, 1.0, 1.0), 2.0 * np.pi / 3.0)])
        R = group_closure(gens, tol=1e-9, max_order=60)
        if len(R) != 60:
            raise RuntimeError(f"icosahedral group: {len(R)} elements")
        return cls(R)

    @classmethod
    def fibre(cls, crystal_axis, sample_axis, n: int = 12) -> "Texture":
        """A fibre texture: ``crystal_axis`` of every grain along ``sample_axis``, uniformly turned about it.  The rotation
        taking the one axis to the other, composed with ``n`` equally spaced turns about ``sample_axis``: exact for a
        rank-4 tensor from n = 5 (n = 4 is not), so n < 5 is refused."""
        if isinstance(n, (bool, np.bool_)) or not isinstance(n, (int, np.integer)) or n < 5:
            raise ValueError(f"n: expected an int >= 5 (a rank-4 tensor needs five turns), got {n!r}")
        R0 = rotation_between(crystal_axis, sample_axis)
        turns = axis_angle(sample_axis, 2.0 * np.pi * np.arange(n) / n)
        return cls(turns @ R0)

    @classmethod
    def from_bunge(cls, phi1, Phi, phi2, weights=None, degrees: bool = True) -> "Texture":
        """Bunge Euler angles (Z-X-Z; arrays [G] or scalars).  Bunge's g = Z(phi2) X(Phi) Z(phi1) maps SAMPLE to CRYSTAL
        components, so the rotation used here (crystal -> sample) is its transpose: R = g^T."""
        p1, P, p2 = (np.atleast_1d(np.asarray(a, dtype=np.float64)) for a in (phi1, Phi, phi2))
        if not (p1.ndim == P.ndim == p2.ndim == 1 and len(p1) == len(P) == len(p2)):
            raise ValueError("phi1, Phi, phi2: expected three arrays of one length")
        if degrees:
            p1, P, p2 = np.deg2rad(p1), np.deg2rad(P), np.deg2rad(p2)
        c1, s1, c, s, c2, s2 = np.cos(p1), np.sin(p1), np.cos(P), np.sin(P), np.cos(p2), np.sin(p2)
        g = np.empty((len(p1), 3, 3))
        g[:, 0, 0], g[:, 0, 1], g[:, 0, 2] = c1 * c2 - s1 * s2 * c, s1 * c2 + c1 * s2 * c, s2 * s
        g[:, 1, 0], g[:, 1, 1], g[:, 1, 2] = -c1 * s2 - s1 * c2 * c, -s1 * s2 + c1 * c2 * c, c2 * s
        g[:, 2, 0], g[:, 2, 1], g[:, 2, 2] = s1 * s, -c1 * s, c
        return cls(g.transpose(0, 2, 1), weights)

    @classmethod
    def scatter(cls, R0, sigma_deg: float, n: int, seed: int) -> "Texture":
        """``n`` orientations scattered about ``R0``: R0 exp([w]_x) with w ~ N(0, sigma^2 1_3) (radians), seeded"""
        R0 = np.asarray(R0, dtype=np.float64)
        if R0.shape != (3, 3):
            raise ValueError(f"R0: expected [3,3], got {R0.shape}")
        sigma = elastic._check_number(sigma_deg, "sigma_deg", 0.0)
        if isinstance(n, (bool, np.bool_)) or not isinstance(n, (int, np.integer)) or n < 1:
            raise ValueError(f"n: expected an int >= 1, got {n!r}")
        w = np.random.default_rng(seed).standard_normal((n, 3)) * np.deg2rad(sigma)
        return cls(R0 @ _exp_so3(w))

    @classmethod
    def mix(cls, textures, fractions) -> "Texture":
        """one texture out of components (each a single texture): component i carries ``fractions[i]`` of the weight"""
        textures = list(textures)
        f = np.asarray(fractions, dtype=np.float64).reshape(-1)
        if not textures or len(f) != len(textures) or any(len(t) != 1 for t in textures):
            raise ValueError("mix: expected single textures and one fraction each")
        if not (np.isfinite(f).all() and (f >= 0).all() and f.sum() > 0):
            raise ValueError("fractions: expected finite numbers >= 0 with a positive sum")
        ws = []
        for t, fi in zip(textures, f):
            w = np.ones(len(t.rotations)) if t.weights is None else t.weights
            ws.append(fi * w / w.sum())
        return cls(np.concatenate([t.rotations for t in textures]), np.concatenate(ws))

    @classmethod
    def stack(cls, textures, validate: bool = True) -> "Texture":
        """the textures of all arguments side by side"""
        textures = list(textures)
        if not textures:
            raise ValueError("stack: no textures")
        weighted = any(t.weights is not None for t in textures)
        w = np.concatenate([np.ones(len(t.rotations)) if t.weights is None else t.weights for t in textures]) if weighted else None
        sizes = np.concatenate([t.sizes for t in textures])
        return cls(np.concatenate([t.rotations for t in textures]), w, np.concatenate([[0], np.cumsum(sizes)]), validate=validate)


def _texture_arrays(texture):
    if isinstance(texture, Texture):
        return texture.rotations, texture.weights, texture.ptr
    R, w, ptr = texture
    R = np.asarray(R, dtype=np.float64).reshape(-1, 3, 3)
    return R, None if w is None else np.asarray(w, dtype=np.float64).reshape(-1), np.asarray(ptr, dtype=np.int64).reshape(-1)


# ---------------------------------------------------------------------------------------------------
# the definitions in numpy
# ---------------------------------------------------------------------------------------------------
def _texture_state(R, w, ptr, orth_tol):
    """per texture: (bad?, normalised weights or None)"""
    out = []
    for t in range(len(ptr) - 1):
        lo, hi = int(ptr[t]), int(ptr[t + 1])
        Rt = R[lo:hi]
        wt = np.ones(hi - lo) if w is None else w[lo:hi]
        with np.errstate(invalid="ignore"):
            skew = np.abs(Rt @ Rt.transpose(0, 2, 1) - np.eye(3)).max(axis=(1, 2)) if hi > lo else np.zeros(0)
            bad = hi <= lo or not np.isfinite(Rt).all() or not np.isfinite(wt).all() or bool((wt < 0).any()) \
                or not wt.sum() > 0 or bool((skew > orth_tol).any())
        out.append((bad, None if bad else wt / wt.sum()))
    return out


def texture_operator_host(texture, orth_tol: float = ORTH_TOL, dtype=np.float64):
    """The operators by their definition -> (op [T,21,21], flags [T] int32): op[(I,J),(K,L)] = sum_g w_g (N_IK N_JL +
    [K != L] N_IL N_JK) on the 21 upper-triangle entries in row-major order, the orientations added one after the other in
    ``dtype`` (``numpy.longdouble`` for a reference sum).  ``texture``: a ``Texture`` or (R [G,3,3], weights [G] or None,
    ptr [T+1]).  A bad texture (``Texture``) is NaN with flag 1."""
    R, w, ptr = _texture_arrays(texture)
    T = len(ptr) - 1
    op, flags = np.full((T, 21, 21), np.nan, dtype=dtype), np.zeros(T, dtype=np.int32)
    I, J = np.array([p[0] for p in _TRI]), np.array([p[1] for p in _TRI])
    cross = (I != J).astype(dtype)
    for t, (bad, wt) in enumerate(_texture_state(R, w, ptr, orth_tol)):
        if bad:
            flags[t] = 1
            continue
        N = rotation_mandel(R[ptr[t]:ptr[t + 1]], dtype)
        wt = wt.astype(dtype)
        acc = np.zeros((21, 21), dtype=dtype)
        for g in range(len(N)):
            n = N[g]
            acc += wt[g] * (n[I[:, None], I[None, :]] * n[J[:, None], J[None, :]]
                            + cross[None, :] * (n[I[:, None], J[None, :]] * n[J[:, None], I[None, :]]))
        op[t] = acc
    return op, flags


def _kron_operators(R, w, ptr, orth_tol):
    """per texture the 36 x 36 matrix K with vec(<X>) = K vec(X), or None for a bad texture"""
    out = []
    for t, (bad, wt) in enumerate(_texture_state(R, w, ptr, orth_tol)):
        if bad:
            out.append(None)
            continue
        N = rotation_mandel(R[ptr[t]:ptr[t + 1]])
        out.append(np.einsum("g,gik,gjl->ijkl", wt, N, N).reshape(36, 36))
    return out


def _members(n, T, phases):
    """-> (agg_ptr [A+1], crystal [M], texture [M], fraction [M]) as int64 / fp64 host arrays"""
    if phases is None:
        A = n * T
        return np.arange(A + 1, dtype=np.int64), np.repeat(np.arange(n), T), np.tile(np.arange(T), n), np.ones(A)
    if len(phases) != 4:
        raise ValueError("phases: expected (agg_ptr, crystal, texture, fraction)")
    ptr, c, t, f = (np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a).reshape(-1) for a in phases)
    ptr, c, t, f = ptr.astype(np.int64), c.astype(np.int64), t.astype(np.int64), f.astype(np.float64)
    M = len(c)
    if len(t) != M or len(f) != M:
        raise ValueError(f"phases: crystal, texture and fraction differ in length ({M}, {len(t)}, {len(f)})")
    if len(ptr) < 1 or ptr[0] != 0 or ptr[-1] != M or (np.diff(ptr) < 0).any():
        raise ValueError(f"phases: agg_ptr: expected [A+1] ascending offsets from 0 to {M}")
    if (np.abs(c) > 0x7fffffff).any() or (np.abs(t) > 0x7fffffff).any():
        raise ValueError("phases: an index does not fit 32 bits")
    return ptr, c, t, f


def _spectral(Ch, fn):
    lam, U = np.linalg.eigh(Ch)
    return (U * fn(lam)) @ U.T


def texture_average_host(voigt, texture, phases=None, flags=None, method: str = "congruence", orth_tol: float = ORTH_TOL) -> dict:
    """The four means by their definitions in numpy fp64 -> dict of ``voigt``, ``reuss``, ``hill``, ``geometric`` [A,6,6]
    (Voigt matrices) and ``status`` [A] int32; without ``phases`` A = B * T, aggregate b * T + t.  ``voigt`` [B,6,6] or
    [6,6] (the mean of the two triangles is used), ``flags`` [B] as ``matten_elastic_props`` sets them, or None.
    ``method``: "congruence" adds w_g N_g X N_g^T orientation by orientation, "kronecker" applies the 36 x 36 matrix
    sum_g w_g N_g (x) N_g -- two routes to the same numbers, whose distance is the measure of the host's own rounding."""
    if method not in ("congruence", "kronecker"):
        raise ValueError(f"method: expected 'congruence' or 'kronecker', got {method!r}")
    C, _ = elastic._host_voigt(voigt)
    Ch, singular = elastic._host_flags(flags, C)
    fl = np.zeros(len(C), dtype=np.int64) if flags is None else np.asarray(
        flags.detach().cpu().numpy() if isinstance(flags, torch.Tensor) else flags).reshape(-1)
    R, w, ptr = _texture_arrays(texture)
    n, T = len(C), len(ptr) - 1
    agg_ptr, mc, mt, mf = _members(n, T, phases)
    states = _texture_state(R, w, ptr, orth_tol)
    Ns = [None if bad else rotation_mandel(R[ptr[t]:ptr[t + 1]]) for t, (bad, _) in enumerate(states)]
    Ks = _kron_operators(R, w, ptr, orth_tol) if method == "kronecker" else None
    lam_min = np.full(n, np.nan)
    lam_min[~singular] = np.linalg.eigvalsh(Ch[~singular])[:, 0] if (~singular).any() else []

    def mean(X, t):
        if Ks is not None:
            return (Ks[t] @ X.reshape(36)).reshape(6, 6)
        return np.einsum("g,gik,kl,gjl->ij", states[t][1], Ns[t], X, Ns[t])

    A = len(agg_ptr) - 1
    out = {k: np.full((A, 6, 6), np.nan) for k in SCHEMES}
    status = np.zeros(A, dtype=np.int32)
    inv_log = {}
    for a in range(A):
        ms = range(int(agg_ptr[a]), int(agg_ptr[a + 1]))
        f = mf[list(ms)]
        ok = len(ms) > 0 and np.isfinite(f).all() and (f >= 0).all() and f.sum() > 0
        pd = True
        for m in ms:
            c, t = mc[m], mt[m]
            if not (0 <= c < n and 0 <= t < T) or singular[c] or states[t][0]:
                ok = False
                continue
            pd = pd and (fl[c] & 2) == 0 and lam_min[c] > 0
        if not ok:
            status[a] = STATUS_NO_VALUE
            continue
        f = f / f.sum()
        out["voigt"][a] = elastic.MANDEL_UNWEIGHT * sum(fi * mean(Ch[mc[m]], mt[m]) for fi, m in zip(f, ms))
        if not pd:
            status[a] = STATUS_NOT_POSITIVE_DEFINITE
            continue
        for m in ms:
            if mc[m] not in inv_log:
                inv_log[mc[m]] = (np.linalg.inv(Ch[mc[m]]), _spectral(Ch[mc[m]], np.log))
        Sbar = sum(fi * mean(inv_log[mc[m]][0], mt[m]) for fi, m in zip(f, ms))
        Lbar = sum(fi * mean(inv_log[mc[m]][1], mt[m]) for fi, m in zip(f, ms))
        out["reuss"][a] = elastic.MANDEL_UNWEIGHT * np.linalg.inv(0.5 * (Sbar + Sbar.T))
        out["geometric"][a] = elastic.MANDEL_UNWEIGHT * _spectral(0.5 * (Lbar + Lbar.T), np.exp)
        out["hill"][a] = 0.5 * (out["voigt"][a] + out["reuss"][a])
    for k in SCHEMES:
        out[k] = 0.5 * (out[k] + out[k].transpose(0, 2, 1))
    out["status"] = status
    return out


def _dd(fn_name: str, lam: np.ndarray) -> np.ndarray:
    """divided differences (f(a_i) - f(a_j)) / (a_i - a_j) of log or exp, finite where a_i == a_j"""
    a, b = lam[:, None], lam[None, :]
    with np.errstate(all="ignore"):
        if fn_name == "log":
            t = (a - b) / b
            tt = np.where(np.abs(t) < 1e-6, 1.0, t)
            return np.where(np.abs(t) < 1e-6, (1.0 - t / 2.0 + t * t / 3.0) / b, np.log1p(tt) / (tt * b))
        d = a - b
        dd = np.where(np.abs(d) < 1e-6, 1.0, d)
        return np.exp(b) * np.where(np.abs(d) < 1e-6, 1.0 + d / 2.0 + d * d / 6.0, np.expm1(dd) / dd)


def _dk(Ch, fn_name: str, G):
    """Daleckii-Krein: the adjoint of the spectral function at the symmetric Ch applied to the symmetric G"""
    lam, U = np.linalg.eigh(Ch)
    return U @ (_dd(fn_name, lam) * (U.T @ G @ U)) @ U.T


def texture_average_bwd_host(voigt, texture, g_out, phases=None, flags=None, method: str = "kronecker",
                             orth_tol: float = ORTH_TOL) -> np.ndarray:
    """The adjoint of ``texture_average_host`` in numpy fp64: ``g_out`` [A,4,6,6] (voigt, reuss, hill, geometric) -> g_voigt
    [B,6,6], symmetric.  voigt: the transposed operator; reuss: g_S = -C_R g C_R, the transposed operator, g_C = -S g_S S;
    hill: half of each; geometric: Daleckii-Krein at exp and at log.  Parts without a value (status -1: all; status 2:
    all but voigt) contribute zeros.  ``method`` as in ``texture_average_host``: the transposed 36 x 36 matrix, or
    sum_g w_g N_g^T G N_g orientation by orientation."""
    C, single = elastic._host_voigt(voigt)
    Ch, _ = elastic._host_flags(flags, C)
    R, w, ptr = _texture_arrays(texture)
    n, T = len(C), len(ptr) - 1
    agg_ptr, mc, mt, mf = _members(n, T, phases)
    fwd = texture_average_host(C, (R, w, ptr), phases, flags, method=method, orth_tol=orth_tol)
    states = _texture_state(R, w, ptr, orth_tol)
    if method == "kronecker":
        Ks = _kron_operators(R, w, ptr, orth_tol)
    else:
        Ns = [None if bad else rotation_mandel(R[ptr[t]:ptr[t + 1]]) for t, (bad, _) in enumerate(states)]
    g_out = np.asarray(g_out.detach().cpu().numpy() if isinstance(g_out, torch.Tensor) else g_out, dtype=np.float64)
    g_out = g_out.reshape(-1, 4, 6, 6)
    g_out = elastic.MANDEL_UNWEIGHT * (0.5 * (g_out + g_out.transpose(0, 1, 3, 2)))      # with respect to the Mandel matrices

    def adjoint(Gm, t):      # sum_g w_g N_g^T G N_g: the transpose of the 36 x 36 matrix of the average
        if method == "kronecker":
            return (Ks[t].T @ Gm.reshape(36)).reshape(6, 6)
        return np.einsum("g,gki,kl,glj->ij", states[t][1], Ns[t], Gm, Ns[t])

    out = np.zeros((n, 6, 6))
    for a in range(len(agg_ptr) - 1):
        st = fwd["status"][a]
        if st == STATUS_NO_VALUE:
            continue
        ms = list(range(int(agg_ptr[a]), int(agg_ptr[a + 1])))
        f = mf[ms] / mf[ms].sum()
        full = st == STATUS_OK
        GV = g_out[a, 0] + (0.5 * g_out[a, 2] if full else 0.0)
        if full:
            CR = elastic.MANDEL_WEIGHT * fwd["reuss"][a]
            GS = -CR @ (g_out[a, 1] + 0.5 * g_out[a, 2]) @ CR
            Lbar = _spectral(elastic.MANDEL_WEIGHT * fwd["geometric"][a], np.log)
            GL = _dk(Lbar, "exp", g_out[a, 3])
        for fi, m in zip(f, ms):
            c, t = mc[m], mt[m]
            g = fi * adjoint(GV, t)
            if full:
                S = np.linalg.inv(Ch[c])
                g = g - S @ (fi * adjoint(GS, t)) @ S + _dk(Ch[c], "log", fi * adjoint(GL, t))
            out[c] += elastic.MANDEL_WEIGHT * g
    out = 0.5 * (out + out.transpose(0, 2, 1))
    return out[0] if single else out


# ---------------------------------------------------------------------------------------------------
# the device
# ---------------------------------------------------------------------------------------------------
class TextureAverage:
    """The result of ``texture_average``: ``voigt``, ``reuss``, ``hill``, ``geometric`` ([B,T,6,6] without phases, [A,6,6]
    with; Voigt stiffness matrices on the device, attached to the graph when the input required a gradient) and ``status``
    ([B,T] or [A] int32: 0; 2 a member is not positive definite, only ``voigt`` has a value; -1 no value)."""

    def __init__(self, voigt, reuss, hill, geometric, status):
        self.voigt, self.reuss, self.hill, self.geometric, self.status = voigt, reuss, hill, geometric, status

    def tensor(self, scheme: str = "hill") -> torch.Tensor:
        if scheme not in SCHEMES:
            raise ValueError(f"scheme: expected one of {SCHEMES}, got {scheme!r}")
        return getattr(self, scheme)

    def cartesian(self, scheme: str = "hill") -> torch.Tensor:
        """[...,3,3,3,3] (``elastic.voigt_to_cartesian``)"""
        return elastic.voigt_to_cartesian(self.tensor(scheme))

    def properties(self, scheme: str = "hill", **kw) -> elastic.ElasticProperties:
        """``elastic_properties`` of the aggregate tensors (rows in the order of ``tensor(scheme).reshape(-1, 6, 6)``):
        with ``directions`` the directional Young's modulus of a sheet is one call"""
        return elastic.elastic_properties(self.tensor(scheme).detach().reshape(-1, 6, 6), **kw)


def _device_members(n, T, phases, device):
    """the member lists and the inverse of member_crystal on the device"""
    if phases is None:      # every crystal under every texture: nothing to sort, nothing uploaded
        A = n * T
        ar = torch.arange(A, dtype=torch.int32, device=device)
        return (torch.arange(A + 1, dtype=torch.int64, device=device), ar // max(T, 1), ar % max(T, 1),
                torch.ones(A, dtype=torch.float64, device=device), torch.arange(n + 1, dtype=torch.int64, device=device) * T, ar)
    agg_ptr, c, t, f = _members(n, T, phases)
    inside = (c >= 0) & (c < n)
    order = np.argsort(np.where(inside, c, n), kind="stable")
    counts = np.bincount(c[inside], minlength=n) if n else np.zeros(0, dtype=np.int64)
    crystal_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    crystal_member = np.full(len(c), -1, dtype=np.int32)
    crystal_member[:int(inside.sum())] = order[:int(inside.sum())]
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a.astype(dt))).to(device)      # noqa: E731
    return (up(agg_ptr, np.int64), up(c, np.int32), up(t, np.int32), up(f, np.float64), up(crystal_ptr, np.int64),
            up(crystal_member, np.int32))


def _average_rows(rows, layout, single, failed, texture, phases, grad):
    from .autograd import ElasticPropsFn, TextureAverageFn

    if not isinstance(texture, Texture):
        raise ValueError("texture: expected a Texture")
    if grad:
        voigt, _, _, flags = ElasticPropsFn.apply(rows, layout)
    else:
        voigt, _, _, flags = ops.elastic_props(rows, layout)
    if failed is not None and failed.any():
        flags |= torch.as_tensor(failed.astype(np.int32) * (elastic.FLAG_FAILED_STRUCTURE | elastic.FLAG_SINGULAR),
                                 device=flags.device)
    moduli, vectors, _ = ops.elastic_kelvin(voigt.detach(), flags, want_dilatation=False)
    op, tex_flags = texture.operator(rows.device)
    n, T = rows.shape[0], len(texture)
    agg_ptr, mc, mt, mf, crystal_ptr, crystal_member = _device_members(n, T, phases, rows.device)
    if grad:
        out, status = TextureAverageFn.apply(voigt, flags, moduli, vectors, op, tex_flags, mc, mt, mf, agg_ptr, crystal_ptr,
                                             crystal_member)
    else:
        out, status = ops.texture_average(voigt, flags, moduli, vectors, op, tex_flags, mc, mt, mf, agg_ptr)
    if phases is None:
        shape = (T,) if single else (n, T)
        out, status = out.reshape(*shape, 4, 6, 6), status.reshape(shape)
    return TextureAverage(out[..., 0, :, :], out[..., 1, :, :], out[..., 2, :, :], out[..., 3, :, :], status)


def texture_average(tensors, texture: Texture, phases=None) -> TextureAverage:
    """The Voigt, Reuss, Hill and geometric means of ``tensors`` under ``texture``.  ``tensors`` as ``elastic_properties``
    takes them ([B,3,3,3,3], [B,6,6], [3,3,3,3], [6,6], torch or numpy, or the list ``predict`` returns: a ``None`` entry
    gives status -1).  Without ``phases`` every crystal is averaged under every texture: fields [B,T,6,6] ([T,6,6] for an
    unbatched input), ``status`` [B,T].  ``phases = (agg_ptr [A+1], crystal [M], texture [M], fraction [M])`` lists explicit
    multi-phase aggregates: aggregate a consists of the members agg_ptr[a] .. agg_ptr[a+1], each a crystal under a texture
    with a volume fraction (normalised per aggregate); fields [A,6,6].  A device tensor that requires a gradient gets one
    (``matten_texture_average_bwd``): the results can go on into ``elastic_moduli`` and ``ModuliLoss``, so a single-crystal
    model can be fine-tuned on measured sheet moduli.  Textures, weights and fractions receive no gradient."""
    grad = isinstance(tensors, torch.Tensor) and tensors.requires_grad and torch.is_grad_enabled()
    rows, layout, single, failed = elastic._as_rows(tensors)
    if grad:
        if not tensors.is_cuda:
            raise ValueError("tensors: only device tensors are differentiated; detach a host tensor")
        rows = tensors.reshape(-1, rows.shape[1])
    else:
        rows = elastic._upload(rows)
    return _average_rows(rows, layout, single, failed, texture, phases, grad)


def texture_average_from_irreps(x, texture: Texture, formula: str = "ijkl=jikl=klij", phases=None) -> TextureAverage:
    """The same from the model's irreps rows ``x`` [B,21] (or [21]; fp32): one ``dense_rows`` with ``elastic.voigt_basis``
    gives the Voigt matrices, as in ``elastic_properties_from_irreps``; differentiable in ``x`` when it requires a gradient."""
    from .autograd import DenseRowsFn

    if not isinstance(x, torch.Tensor) or x.dim() not in (1, 2):
        raise ValueError("x: expected a tensor [B,21] or [21]")
    V = elastic.voigt_basis(formula)
    if x.shape[-1] != V.shape[0]:
        raise ValueError(f"x: expected {V.shape[0]} irreps components per row, got {x.shape[-1]}")
    single = x.dim() == 1
    grad = x.requires_grad and torch.is_grad_enabled()
    if not x.is_cuda:
        if grad:
            raise ValueError("x: only device tensors are differentiated; detach a host tensor")
        x = x.to(elastic._default_device())
    key = (formula, x.device)
    if key not in elastic._VOIGT_Q:
        elastic._VOIGT_Q[key] = torch.tensor(V, dtype=torch.float32, device=x.device)
    if key not in elastic._VOIGT_QT:
        elastic._VOIGT_QT[key] = elastic._VOIGT_Q[key].t().contiguous()
    x2 = x.reshape(-1, x.shape[-1]).to(torch.float32)
    if grad:
        rows = DenseRowsFn.apply(x2, elastic._VOIGT_Q[key], elastic._VOIGT_QT[key])
    else:
        rows = ops.dense_rows(x2.detach(), elastic._VOIGT_Q[key])
    return _average_rows(rows, 1, single, None, texture, phases, grad)
