"""
Rotations and symmetry averages of irreps tensors, on the device.

The model computes in the irreps basis end to end; this module applies a rotation (proper or improper) to rows of
irreps, or averages them over a list of operations, without leaving the device or the basis: ``wigner_D``,
``rotate_irreps``, ``average_irreps`` / ``symmetrize_irreps`` / ``symmetry_deviation`` (three kernels, csrc/rotate.hip),
``group_closure`` to turn generators into a group on the host, and ``symmetrize_graphs`` to clean crystal-level targets
before a training set is built.  The reference rotates Cartesian tensors on the host with an einsum
(tests/model/test_tfn_tensor.py:98-139 after utils.py:110-133).

Conventions ("Rotations and symmetry of irreps tensors").  For a formula f with
``irreps, Q = o3.cartesian_tensor_basis(f)`` and Qf = Q flattened to [dim, 3^rank] (orthonormal rows), any orthogonal M acts by

    D_f(M) = Qf (M x ... x M) Qf^T                      (rank Kronecker factors),

which is block diagonal over the irreps, the block of irrep (l, p) being

    D_{l,p}(M) = p^[det M < 0] D^l(det(M) M),           Y_l(R v) = D^l(R) Y_l(v)

with the model's own harmonics Y_l: one convention for the harmonics, the Cartesian bases and parity.  A rotation acts
on a Cartesian tensor as T' = M ... M T, i.e. on positions as r' = M r (row vectors: ``pos @ M.T``).
Flags of a rotation: bit 0 a non-finite entry, bit 1 max|M^T M - I| above ``orth_tol``, bit 2 improper; rows rotated by a
matrix with bit 0 or 1 are NaN.  ``wigner_D_host`` / ``rotate_irreps_host`` / ``average_irreps_host`` restate the
definitions in numpy from the Kronecker form above (not the kernels' method): the tests hold the kernels to them.

Not here: finding a crystal's operations, symmetrising per-atom tensors across equivalent atoms (needs the atom
permutation), gradients with respect to rotations, Reuss / Hill texture averages, Euler-angle and quaternion front ends,
l > 4.
"""
import functools
import re

import numpy as np
import torch

from . import o3
from . import ops as _ops
from .autograd import IrrepsAverageFn, IrrepsRotateFn

FLAG_NOT_FINITE, FLAG_NOT_ORTHOGONAL, FLAG_IMPROPER = 1, 2, 4
LMAX = 4
# a fully symmetric tensor of rank l holds irrep (l, (-1)^l) once: its rows of the Cartesian basis define D^l
_SYMMETRIC_FORMULA = {1: "i", 2: "ij=ji", 3: "ijk=jik=ikj", 4: "ijkl=jikl=ikjl=ijlk"}
_FORMULA = re.compile(r"^[-a-z=]+$")


# ---------------------------------------------------------------------------------------------------
# irreps, layouts
# ---------------------------------------------------------------------------------------------------
def irreps_of(irreps_or_formula) -> o3.Irreps:
    """an ``Irreps``, an irreps string (``"2x0e+2x2e+4e"``) or a Cartesian formula (``"ijkl=jikl=klij"``) -> Irreps"""
    if isinstance(irreps_or_formula, str) and _FORMULA.match(irreps_or_formula.strip()):
        return o3.cartesian_tensor_basis(irreps_or_formula.strip())[0]
    return o3.Irreps(irreps_or_formula)


def irreps_layout(irreps_or_formula) -> np.ndarray:
    """the kernels' layout rows [K,4] int32 (offset, mul, l, parity), one per ``mul x (l, p)`` entry of the irreps"""
    irreps = irreps_of(irreps_or_formula)
    rows = [(off, b.mul, b.ir.l, b.ir.p) for off, b in zip(irreps.offsets(), irreps)]
    if any(l > LMAX for _, _, l, _ in rows):
        raise ValueError(f"irreps {irreps}: l > {LMAX} is not supported")
    if len(rows) > _ops.WIGNER_MAX_LAYOUT:
        raise ValueError(f"irreps {irreps}: more than {_ops.WIGNER_MAX_LAYOUT} entries (simplify() merges neighbours)")
    return np.asarray(rows, dtype=np.int32).reshape(-1, 4)


# ---------------------------------------------------------------------------------------------------
# the definitions in numpy (fp64), from the Kronecker form
# ---------------------------------------------------------------------------------------------------
def _matrices(R) -> np.ndarray:
    if isinstance(R, torch.Tensor):
        R = R.detach().cpu().numpy()
    R = np.asarray(R, dtype=np.float64)
    if R.size == 0:
        return np.zeros((0, 3, 3))
    if R.shape[-2:] != (3, 3) or R.ndim not in (2, 3):
        raise ValueError(f"R: expected [G,3,3] or [3,3], got {R.shape}")
    return R.reshape(-1, 3, 3)


def _kron_power(M: np.ndarray, rank: int) -> np.ndarray:
    K = np.ones((1, 1))
    for _ in range(rank):
        K = np.kron(K, M)
    return K


@functools.lru_cache(maxsize=None)
def _flat_basis(formula: str):
    irreps, Q = o3.cartesian_tensor_basis(formula)
    return irreps, Q.reshape(Q.shape[0], -1), Q.ndim - 1


def formula_D_host(formula: str, R) -> np.ndarray:
    """D_f(M) = Qf (M x ... x M) Qf^T for every matrix of R -> [G, dim, dim] fp64: the definition, for any M"""
    _, Qf, rank = _flat_basis(formula)
    return np.stack([Qf @ _kron_power(M, rank) @ Qf.T for M in _matrices(R)])


def wigner_D_host(l: int, R, parity=None) -> np.ndarray:
    """[G, 2l+1, 2l+1] fp64: D^l of the proper part det(M) M of every matrix, or with ``parity`` (+1 / -1) the block
    D_{l,p}(M) = p^[det M < 0] D^l(det(M) M).  Built from the fully symmetric rank-l Cartesian basis."""
    if not 0 <= int(l) <= LMAX:
        raise ValueError(f"l = {l}: expected 0..{LMAX}")
    if parity not in (None, 1, -1):
        raise ValueError("parity: expected None, 1 or -1")
    M = _matrices(R)
    improper = np.linalg.det(M) < 0
    proper = np.where(improper[:, None, None], -M, M)
    if l == 0:
        D = np.ones((len(M), 1, 1))
    else:
        irreps, Qf, rank = _flat_basis(_SYMMETRIC_FORMULA[l])
        lo = irreps.offsets()[[b.ir.l for b in irreps].index(l)]
        Ql = Qf[lo:lo + 2 * l + 1]
        D = np.stack([Ql @ _kron_power(P, rank) @ Ql.T for P in proper])
    if parity == -1:
        D = np.where(improper[:, None, None], -D, D)
    return D


def irreps_D_host(irreps_or_formula, R) -> np.ndarray:
    """the block-diagonal matrix of every M on rows of these irreps -> [G, dim, dim] fp64"""
    irreps = irreps_of(irreps_or_formula)
    M = _matrices(R)
    out = np.zeros((len(M), irreps.dim, irreps.dim))
    for off, b in zip(irreps.offsets(), irreps):
        D = wigner_D_host(b.ir.l, M, b.ir.p)
        for u in range(b.mul):
            lo = off + u * b.ir.dim
            out[:, lo:lo + b.ir.dim, lo:lo + b.ir.dim] = D
    return out


def _host_D(irreps_or_formula, R) -> np.ndarray:
    if isinstance(irreps_or_formula, str) and _FORMULA.match(irreps_or_formula.strip()):
        return formula_D_host(irreps_or_formula.strip(), R)       # the Kronecker definition itself
    return irreps_D_host(irreps_or_formula, R)


def _host_x(x) -> np.ndarray:
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.atleast_2d(np.asarray(x, dtype=np.float64))


def rotate_irreps_host(x, irreps_or_formula, R, index=None) -> np.ndarray:
    """numpy fp64 restatement of ``rotate_irreps``: x [N,dim] -> [N,dim]"""
    x = _host_x(x)
    D = _host_D(irreps_or_formula, R)
    if index is None:
        if len(D) not in (1, len(x)):
            raise ValueError(f"without index the {len(x)} rows need 1 or {len(x)} rotations, got {len(D)}")
        index = np.zeros(len(x), dtype=np.int64) if len(D) == 1 else np.arange(len(x))
    index = np.asarray(index.detach().cpu().numpy() if isinstance(index, torch.Tensor) else index, dtype=np.int64)
    return np.einsum("nij,nj->ni", D[index], x)


def average_irreps_host(x, irreps_or_formula, R, op_ptr=None, op_idx=None, weights=None, orth_tol: float = 1e-6):
    """numpy fp64 restatement of ``average_irreps`` -> (avg [N,dim], deviation [N]); without op_ptr / op_idx every row
    takes all of R (weights [G] then)"""
    x = _host_x(x)
    M = _matrices(R)
    D = _host_D(irreps_or_formula, M) if len(M) else np.zeros((0, x.shape[1], x.shape[1]))
    n, G = len(x), len(M)
    if op_ptr is None:
        op_ptr, op_idx = np.arange(n + 1) * G, np.tile(np.arange(G), n)
        weights = None if weights is None else np.tile(np.asarray(weights, dtype=np.float64), n)
    op_ptr, op_idx = np.asarray(op_ptr, dtype=np.int64), np.asarray(op_idx, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        skew = np.abs(np.einsum("gki,gkj->gij", M, M) - np.eye(3)).max(axis=(1, 2)) if G else np.zeros(0)
    ok = np.isfinite(M).all(axis=(1, 2)) & (skew <= orth_tol) if G else np.zeros(0, dtype=bool)
    out, dev = np.empty_like(x), np.empty(n)
    with np.errstate(invalid="ignore", divide="ignore"):
        for r in range(n):
            js = np.arange(op_ptr[r], op_ptr[r + 1])
            if len(js) == 0:
                out[r], dev[r] = x[r], 0.0
                continue
            w = np.ones(len(js)) if weights is None else np.asarray(weights, dtype=np.float64)[js]
            wsum = w.sum()
            g = op_idx[js]
            inside = bool(((g >= 0) & (g < G)).all())              # an operation outside R: the row is NaN, like a flagged one
            if not (inside and np.isfinite(w).all() and wsum > 0 and ok[g].all()):
                out[r], dev[r] = np.nan, np.nan
                continue
            acc = np.zeros(x.shape[1])
            for j, wj in zip(js, w):
                acc += wj * (D[op_idx[j]] @ x[r])
            out[r] = acc / wsum
            nx = np.linalg.norm(x[r])
            dev[r] = 0.0 if nx == 0 else np.linalg.norm(x[r] - out[r]) / nx
    return out, dev


def group_closure(generators, tol: float = 1e-6, max_order: int = 192, orthonormalize: bool = True) -> np.ndarray:
    """Close a set of orthogonal 3x3 matrices under multiplication (host numpy) -> [order,3,3] fp64, the identity first.
    Two products are the same element when they agree to ``tol`` entrywise.  ``orthonormalize`` replaces each element
    by its polar factor (the nearest orthogonal matrix), so operations read from a file at 1e-6 become orthogonal to
    rounding and products do not drift.  Raises ValueError when the set has not closed at ``max_order`` elements."""
    def polish(M):
        if not orthonormalize:
            return M
        U, _, Vt = np.linalg.svd(M)
        P = U @ Vt
        return P @ (1.5 * np.eye(3) - 0.5 * (P.T @ P))       # one Newton-Schulz step: the product's own rounding goes too

    gens = [polish(M) for M in _matrices(generators)]
    for M in gens:
        if not np.isfinite(M).all() or np.abs(M.T @ M - np.eye(3)).max() > max(tol, 1e-12) * 10:
            raise ValueError("group_closure: a generator is not orthogonal")
    elements = [np.eye(3)]

    def known(M):
        return any(np.abs(M - E).max() <= tol for E in elements)

    frontier = [np.eye(3)]
    while frontier:
        new = []
        for E in frontier:
            for Gm in gens:
                M = polish(Gm @ E)
                if not known(M):
                    if len(elements) >= max_order:
                        raise ValueError(f"group_closure: no closure within max_order = {max_order} elements")
                    elements.append(M)
                    new.append(M)
        frontier = new
    return np.stack(elements)


# ---------------------------------------------------------------------------------------------------
# the device
# ---------------------------------------------------------------------------------------------------
def _device_R(R, device=None) -> torch.Tensor:
    if not isinstance(R, torch.Tensor):
        if device is None:
            raise ValueError("R: a host array needs tensors on a device to go with")
        R = torch.as_tensor(np.asarray(R, dtype=np.float64), device=device)
    if R.shape[-2:] != (3, 3) or R.dim() not in (2, 3):
        raise ValueError(f"R: expected [G,3,3] or [3,3], got {tuple(R.shape)}")
    if device is not None and R.device != torch.device(device):
        R = R.to(device)             # (a handful of matrices; rows on the host are refused by the kernels' wrappers)
    return R.detach().to(torch.float64).reshape(-1, 3, 3)


def wigner_D(l: int, R, parity=None, orth_tol: float = 1e-6) -> torch.Tensor:
    """[G, 2l+1, 2l+1] fp64 on R's device: D^l of the proper part of every matrix of R ([G,3,3] or [3,3]), or with
    ``parity`` the block D_{l,p}(M).  A matrix that is not finite or not orthogonal to ``orth_tol`` gives NaN."""
    if not 0 <= int(l) <= LMAX:
        raise ValueError(f"l = {l}: expected 0..{LMAX}")
    if parity not in (None, 1, -1):
        raise ValueError("parity: expected None, 1 or -1")
    D, flags = _ops.wigner_d(_device_R(R), int(l), orth_tol)
    lo = l * (4 * l * l - 1) // 3
    block = D[:, lo:lo + (2 * l + 1) ** 2].reshape(-1, 2 * l + 1, 2 * l + 1)
    if parity == -1:
        block = torch.where((flags & FLAG_IMPROPER).bool()[:, None, None], -block, block)
    return block.contiguous()


def _rows(x):
    if not isinstance(x, torch.Tensor):
        raise TypeError("x: expected a tensor on the device")
    if x.dim() not in (1, 2):
        raise ValueError(f"x: expected [N,dim] or [dim], got {tuple(x.shape)}")
    return (x.unsqueeze(0), True) if x.dim() == 1 else (x, False)


def _table(irreps_or_formula, x, R, orth_tol):
    irreps = irreps_of(irreps_or_formula)
    if x.shape[1] != irreps.dim:
        raise ValueError(f"x: {x.shape[1]} columns, the irreps {irreps} have {irreps.dim}")
    layout = irreps_layout(irreps)
    R = _device_R(R, x.device)
    D, flags = _ops.wigner_d(R, irreps.lmax if len(irreps) else 0, orth_tol)
    return layout, D, flags


def rotate_irreps(x, irreps_or_formula, R, index=None, orth_tol: float = 1e-6) -> torch.Tensor:
    """D(M) x per row.  x [N,dim] or [dim], fp32 or fp64, on the device; R [3,3] (one rotation for all rows), [N,3,3]
    (one per row) or [G,3,3] with ``index`` [N] mapping rows to rotations -- pass ``batch["batch"]`` to rotate per-atom
    predictions by their structure's rotation.  Proper and improper M.  Differentiable in x (the backward applies D^T);
    R carries no gradient.  Rows of a flagged rotation, or of an index outside R, are NaN."""
    x, squeeze = _rows(x)
    layout, D, flags = _table(irreps_or_formula, x, R, orth_tol)
    if index is not None:
        index = torch.as_tensor(index, device=x.device).to(torch.int32)
    out = IrrepsRotateFn.apply(x, layout, D, flags, index)
    return out[0] if squeeze else out


def _csr(x, R, op_ptr, op_idx, weights):
    """(R [G,3,3] host or device, op_ptr, op_idx, weights) as the kernel takes them, from the three input forms"""
    n, dev = x.shape[0], x.device
    if isinstance(R, (list, tuple)) and op_ptr is None:                    # one array of operations per row
        if len(R) != n:
            raise ValueError(f"R: {len(R)} lists of operations for {n} rows")
        mats = [_matrices(r) for r in R]
        counts = np.asarray([len(m) for m in mats], dtype=np.int64)
        ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        R = np.concatenate(mats) if ptr[-1] else np.zeros((0, 3, 3))
        idx = np.arange(ptr[-1], dtype=np.int32)
        if isinstance(weights, (list, tuple)):
            weights = np.concatenate([np.asarray(w, dtype=np.float64).reshape(-1) for w in weights]) if ptr[-1] else np.zeros(0)
    elif op_ptr is None:                                                  # the same list for every row
        G = int(_matrices(R).shape[0]) if not isinstance(R, torch.Tensor) else int(R.reshape(-1, 3, 3).shape[0])
        ptr = torch.arange(n + 1, dtype=torch.int64, device=dev) * G
        idx = torch.arange(G, dtype=torch.int32, device=dev).repeat(n)
        if weights is not None:
            weights = torch.as_tensor(weights, dtype=torch.float64, device=dev).reshape(-1)
            if weights.numel() == G:
                weights = weights.repeat(n)
    else:
        if op_idx is None:
            raise ValueError("op_ptr needs op_idx")
        ptr = torch.as_tensor(op_ptr).to(torch.int64).reshape(-1)
        idx = torch.as_tensor(op_idx).to(torch.int32).reshape(-1)
        # one look at the lists before a kernel walks them (a read-back when they live on the device)
        if ptr.numel() != n + 1 or int(ptr[0]) != 0 or bool((ptr[1:] < ptr[:-1]).any()) or int(ptr[-1]) > idx.numel():
            raise ValueError("op_ptr: expected [N+1] ascending offsets from 0 into op_idx")
    ptr = torch.as_tensor(ptr, device=dev)
    idx = torch.as_tensor(idx, device=dev)
    if weights is not None:
        weights = torch.as_tensor(weights, dtype=torch.float64, device=dev).reshape(-1)
        if weights.numel() != idx.numel():
            raise ValueError(f"weights: expected one per operation ({idx.numel()}), got {weights.numel()}")
    return R, ptr.contiguous(), idx.contiguous(), weights


def average_irreps(x, irreps_or_formula, R, op_ptr=None, op_idx=None, weights=None, orth_tol: float = 1e-6):
    """(avg, deviation): avg[r] = sum_j w_j D(M_j) x[r] / sum_j w_j over the operations of row r and deviation[r] =
    |x[r] - avg[r]| / |x[r]| (fp64; 0 for a zero row).  x [N,dim] or [dim] on the device.  The operations come as
      * R [G,3,3] alone: the same list for every row (``weights`` [G]);
      * R a list of N arrays [g_r,3,3]: a list per row (``weights`` a list alike), the CSR is built on the host;
      * R [G,3,3] with op_ptr [N+1] and op_idx [nnz]: rows share rotations (``weights`` [nnz]), e.g. all cubic crystals
        of a batch pointing at the same 48.
    An empty list is the trivial group (avg = x).  A flagged operation, a non-finite weight or a weight sum that is not
    positive gives a NaN row.  With weights this is the Voigt (orientation) average of a texture.  Differentiable in x."""
    x, squeeze = _rows(x)
    R, ptr, idx, weights = _csr(x, R, op_ptr, op_idx, weights)
    if isinstance(R, np.ndarray) and len(R) == 0:
        R = torch.zeros(0, 3, 3, dtype=torch.float64, device=x.device)
    layout, D, flags = _table(irreps_or_formula, x, R, orth_tol)
    avg, deviation = IrrepsAverageFn.apply(x, layout, D, flags, ptr, idx, weights)
    return (avg[0], deviation[0]) if squeeze else (avg, deviation)


def symmetrize_irreps(x, irreps_or_formula, R, op_ptr=None, op_idx=None) -> torch.Tensor:
    """the unweighted average over the operations: the projection onto the tensors invariant under the group"""
    return average_irreps(x, irreps_or_formula, R, op_ptr, op_idx)[0]


def symmetry_deviation(x, irreps_or_formula, R, op_ptr=None, op_idx=None) -> torch.Tensor:
    """how far each row is from its symmetrised self, |x - P x| / |x| (fp64)"""
    return average_irreps(x, irreps_or_formula, R, op_ptr, op_idx)[1]


def symmetrize_graphs(graphs, key: str, formula: str, ops, device="cuda") -> np.ndarray:
    """Project the crystal-level target ``key`` (irreps rows of ``formula``) of un-collated host graphs onto the symmetry
    of their crystals, in place, in one device call; returns the per-crystal deviation [len(graphs)] (how far each
    label was from its point group).  ``ops``: [G,3,3] for all crystals, or one array per crystal (an empty one leaves
    the label as it is).  Data cleaning, done before a ``DeviceGraphStore`` or a data module is built from the graphs."""
    if not graphs:
        return np.zeros(0)
    rows = [torch.as_tensor(g[key]) for g in graphs]
    dim = irreps_of(formula).dim
    if any(r.numel() != dim for r in rows):
        raise ValueError(f"{key}: expected one row of {dim} irreps components per graph ({formula})")
    x = torch.stack([r.reshape(dim) for r in rows]).to(device)
    if not x.is_floating_point():
        raise TypeError(f"{key}: expected floating-point labels")
    per_crystal = False
    if isinstance(ops, (list, tuple)):          # [G,3,3] as nested lists is one group for all; anything else a list per crystal
        try:
            per_crystal = np.asarray(ops, dtype=np.float64).ndim != 3
        except (ValueError, TypeError):
            per_crystal = True
    with torch.no_grad():
        avg, deviation = average_irreps(x, formula, list(ops) if per_crystal else ops)
    avg = avg.cpu()
    for g, r, a in zip(graphs, rows, avg):
        g[key] = a.reshape(r.shape).to(r.dtype)
    return deviation.cpu().numpy()
