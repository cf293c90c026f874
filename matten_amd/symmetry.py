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

Finding the operations: ``find_symmetry`` searches every crystal of a batch on the device (csrc/spacegroup.hip; rotations,
translations and atom permutations in a ``CrystalSymmetry``), ``symmetrize_atoms`` averages per-atom rows over it and
``symmetrize_graphs(..., ops="find")`` cleans crystal-level labels with it; ``find_symmetry_host`` /
``symmetrize_atoms_host`` restate both in numpy ("Finding a crystal's symmetry").

Not here: cell reduction (a cell outside the search range is flagged), crystals above 1024 atoms, refinement of
positions, space-group symbols, gradients through ``symmetrize_atoms`` or with respect to rotations, Euler-angle and
quaternion front ends, l > 4.  The Reuss, Hill and geometric texture averages are in ``matten_amd/texture.py``.
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


def symmetrize_graphs(graphs, key: str, formula: str, ops, device="cuda", symprec: float = 1e-3, pos_key: str = "pos",
                      cell_key: str = "cell", z_key: str = "atomic_numbers") -> np.ndarray:
    """Project the crystal-level target ``key`` (irreps rows of ``formula``) of un-collated host graphs onto the symmetry
    of their crystals, in place, in one device call; returns the per-crystal deviation [len(graphs)] (how far each
    label was from its point group).  ``ops``: [G,3,3] for all crystals, one array per crystal (an empty one leaves
    the label as it is), or ``"find"``: each crystal's point group is found on the device (``find_symmetry`` at
    ``symprec``, from the graphs' ``pos_key``, ``cell_key`` and ``z_key`` entries; a crystal the search flags keeps its
    label).  Data cleaning, done before a ``DeviceGraphStore`` or a data module is built from the graphs."""
    if not graphs:
        return np.zeros(0)
    rows = [torch.as_tensor(g[key]) for g in graphs]
    dim = irreps_of(formula).dim
    if any(r.numel() != dim for r in rows):
        raise ValueError(f"{key}: expected one row of {dim} irreps components per graph ({formula})")
    x = torch.stack([r.reshape(dim) for r in rows]).to(device)
    if not x.is_floating_point():
        raise TypeError(f"{key}: expected floating-point labels")
    if isinstance(ops, str):
        if ops != "find":
            raise ValueError(f"ops: expected matrices or 'find', got {ops!r}")
        pos = [np.asarray(torch.as_tensor(g[pos_key]).cpu().numpy(), dtype=np.float64).reshape(-1, 3) for g in graphs]
        ptr = np.concatenate([[0], np.cumsum([len(p) for p in pos])]).astype(np.int64)
        cell = np.stack([np.asarray(torch.as_tensor(g[cell_key]).cpu().numpy(), dtype=np.float64).reshape(3, 3) for g in graphs])
        Z = np.concatenate([np.asarray(torch.as_tensor(g[z_key]).cpu().numpy(), dtype=np.int64).reshape(-1) for g in graphs])
        sym = find_symmetry(pos=np.concatenate(pos), cell=cell, Z=Z, ptr=ptr, symprec=symprec, device=device)
        with torch.no_grad():
            avg, deviation = sym.average_crystal_rows(x, formula)
        avg = avg.cpu()
        for g, r, a in zip(graphs, rows, avg):
            g[key] = a.reshape(r.shape).to(r.dtype)
        return deviation.cpu().numpy()
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


# ---------------------------------------------------------------------------------------------------
# finding a crystal's symmetry ("Finding a crystal's symmetry"; csrc/spacegroup.hip)
# ---------------------------------------------------------------------------------------------------
SYM_NOT_FINITE, SYM_RANGE, SYM_TOO_LARGE, SYM_AMBIGUOUS, SYM_TRUNC, SYM_NOT_PERIODIC = 1, 2, 4, 8, 16, 32
SYM_IDENTITY_ONLY = SYM_NOT_FINITE | SYM_RANGE | SYM_TOO_LARGE | SYM_AMBIGUOUS | SYM_NOT_PERIODIC
SYM_FLAG_NAMES = {SYM_NOT_FINITE: "non-finite input or singular cell", SYM_RANGE: "cell outside the search range (reduce it)",
                  SYM_TOO_LARGE: f"more than {_ops.SYM_MAX_ATOMS} atoms", SYM_AMBIGUOUS: "ambiguous (symprec too large)",
                  SYM_TRUNC: "more pure translations than max_trans", SYM_NOT_PERIODIC: "not periodic along all three axes"}
MAX_OPS = _ops.SYM_MAX_OPS
_SINGULAR = 1e-12
_MAX_M = 4


def _equivalent_atoms(src, tsrc, where, big):
    """label[i] = min_g c[src[g,i]] with c = min_tau tsrc (absent rows, -1, count as ``big``); numpy or torch by ``where``"""
    c = where(tsrc < 0, big, tsrc).min(0)
    c = c[0] if isinstance(c, tuple) else c
    lab = where(src < 0, big, c[src.clip(0)]).min(0)
    return lab[0] if isinstance(lab, tuple) else lab


class HostSymmetry:
    """The fields of ``CrystalSymmetry`` as numpy arrays (padded alike), from ``find_symmetry_host`` or
    ``CrystalSymmetry.host()``; ``crystals`` trims the per-crystal lists to n_rot / n_trans."""
    FIELDS = ("rotations", "rotations_int", "translations", "n_rot", "src", "n_trans", "pure_translations", "tsrc", "flags", "ptr",
              "row_struct")

    def __init__(self, **fields):
        for k in self.FIELDS:
            setattr(self, k, fields[k])

    @property
    def crystals(self):
        out = []
        for b in range(len(self.n_rot)):
            lo, hi, g = int(self.ptr[b]), int(self.ptr[b + 1]), int(self.n_rot[b])
            t = min(int(self.n_trans[b]), self.tsrc.shape[0])
            out.append({"rotations": self.rotations[b, :g], "rotations_int": self.rotations_int[b, :g],
                        "translations": self.translations[b, :g], "src": self.src[:g, lo:hi],
                        "pure_translations": self.pure_translations[b, :t], "tsrc": self.tsrc[:t, lo:hi],
                        "n_trans": int(self.n_trans[b]), "flags": int(self.flags[b])})
        return out

    def equivalent_atoms(self) -> np.ndarray:
        return _equivalent_atoms(self.src, self.tsrc, np.where, len(self.row_struct)).astype(np.int64)


class CrystalSymmetry:
    """The symmetry of a packed batch of crystals, on the device (``find_symmetry``).  Per crystal b, 48 slots of which the
    first n_rot[b] are its point group in lattice order (identity first): ``rotations`` [B,48,3,3] fp64 (Cartesian M,
    r' = M r + t L), ``rotations_int`` [B,48,3,3] int8 (N, f' = f N + t), ``translations`` [B,48,3] (fractional t of each
    representative), ``src`` [48,N] int32 (src[g,k] = the atom whose image under operation g lands on atom k, global
    indices, -1 in absent slots); the pure translations ``pure_translations`` [B,max_trans,3], ``tsrc`` [max_trans,N] with
    their number ``n_trans`` [B]; ``flags`` [B] (SYM_*), ``ptr`` [B+1] int64, ``row_struct`` [N] int32."""

    def __init__(self, **fields):
        for k in HostSymmetry.FIELDS:
            setattr(self, k, fields[k])

    def op_csr(self):
        """(R [B*48,3,3], op_ptr [B+1] int64, op_idx [B*48] int32) for ``average_irreps`` of one row per crystal; device
        arithmetic only (op_idx has the capacity B*48: entries past op_ptr[B] are not read)"""
        B = self.n_rot.shape[0]
        dev = self.n_rot.device
        op_ptr = torch.zeros(B + 1, dtype=torch.int64, device=dev)
        torch.cumsum(self.n_rot, 0, out=op_ptr[1:])
        j = torch.arange(B * MAX_OPS, dtype=torch.int64, device=dev)
        b = torch.searchsorted(op_ptr[1:].contiguous(), j, right=True).clamp_(max=max(B - 1, 0))
        op_idx = (b * MAX_OPS + (j - op_ptr[b]).clamp_(0, MAX_OPS - 1)).to(torch.int32)
        return self.rotations.reshape(-1, 3, 3), op_ptr, op_idx

    def average_crystal_rows(self, x, irreps_or_formula, orth_tol: float = 1e-6):
        """(avg, deviation) of one irreps row per crystal over its point group: ``average_irreps`` with ``op_csr`` and
        without its look at the lists (nothing is read back)"""
        x, squeeze = _rows(x)
        R, op_ptr, op_idx = self.op_csr()
        layout, D, flags = _table(irreps_or_formula, x, R, orth_tol)
        if x.shape[0] != self.n_rot.shape[0]:
            raise ValueError(f"x: {x.shape[0]} rows for {self.n_rot.shape[0]} crystals")
        avg, deviation = _ops.irreps_average(x, layout, D, flags, op_ptr, op_idx)
        return (avg[0], deviation[0]) if squeeze else (avg, deviation)

    def equivalent_atoms(self) -> torch.Tensor:
        """[N] int64: the smallest atom index of each atom's orbit under the full group (plain torch)"""
        n = self.row_struct.shape[0]
        return _equivalent_atoms(self.src.long(), self.tsrc.long(), torch.where, torch.full((), n, dtype=torch.int64, device=self.src.device))

    def host(self) -> HostSymmetry:
        return HostSymmetry(**{k: getattr(self, k).cpu().numpy() for k in HostSymmetry.FIELDS})

    def raise_for_flags(self, ignore: int = 0):
        """the one read-back: ValueError naming every flagged crystal (``ignore``: bits to let pass, e.g. SYM_TRUNC)"""
        flags = self.flags.cpu().numpy() & ~int(ignore)
        bad = np.nonzero(flags)[0]
        if len(bad):
            def names(f):
                return ", ".join(v for k, v in SYM_FLAG_NAMES.items() if f & k)
            raise ValueError("find_symmetry: " + "; ".join(f"crystal {b}: {names(int(flags[b]))}" for b in bad[:8])
                             + (f"; and {len(bad) - 8} more" if len(bad) > 8 else ""))
        return self


def _packed(structures, pos, cell, Z, ptr, pbc):
    """-> (pos [N,3] f64, cell [B,3,3] f64, Z [N] i64, ptr [B+1] i64, pbc [B,3] bool or None) as numpy or torch, as given"""
    if structures is not None:
        from .predict import pack_structures

        structures = list(structures) if isinstance(structures, (list, tuple)) else [structures]
        pos, cell, Z, ptr, _, failed, flags = pack_structures(structures, with_pbc=True, pbc=pbc)
        if failed:
            raise ValueError(f"find_symmetry: structures {failed} cannot be used (malformed, non-finite or singular)")
        return pos, cell, Z, ptr, flags
    if pos is None or cell is None or Z is None or ptr is None:
        raise ValueError("find_symmetry: give structures, or pos, cell, Z and ptr")
    return pos, cell, Z, ptr, pbc


def _host_packed(structures, pos, cell, Z, ptr, pbc):
    pos, cell, Z, ptr, pbc = _packed(structures, pos, cell, Z, ptr, pbc)
    def arr(a, dt):
        return np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=dt)
    pos, cell, Z, ptr = arr(pos, np.float64).reshape(-1, 3), arr(cell, np.float64).reshape(-1, 3, 3), arr(Z, np.int64).reshape(-1), \
        arr(ptr, np.int64).reshape(-1)
    B = len(cell)
    if pbc is not None:
        pbc = arr(pbc, bool)
        pbc = np.broadcast_to(pbc.reshape(-1, 3), (B, 3)).copy()
    if len(ptr) != B + 1 or ptr[0] != 0 or ptr[-1] != len(pos) or len(Z) != len(pos) or (np.diff(ptr) < 0).any():
        raise ValueError("find_symmetry: expected pos [N,3], cell [B,3,3], Z [N] and ptr [B+1] ascending from 0 to N")
    return pos, cell, Z, ptr, pbc


def find_symmetry(structures=None, *, pos=None, cell=None, Z=None, ptr=None, pbc=None, symprec: float = 1e-3, max_trans: int = 64,
                  device="cuda") -> CrystalSymmetry:
    """The symmetry of every crystal of a batch, found on the device: what ``predict.pack_structures`` accepts, or the packed
    arrays (pos [N,3], cell [B,3,3], Z [N], ptr [B+1], pbc None / three bools / [B,3]).  Two entries of the library
    (``ops.lattice_group``, ``ops.crystal_symmetry``); nothing is read back -- ``flags`` says per crystal what went wrong
    (``raise_for_flags`` reads it).  ``symprec`` is a length in the units of the positions."""
    if not (float(symprec) > 0.0 and np.isfinite(float(symprec))):
        raise ValueError("symprec: expected a positive finite length")
    on_device = structures is None and all(isinstance(a, torch.Tensor) and a.is_cuda for a in (pos, cell, Z, ptr))
    if on_device:
        pos, cell = pos.detach().to(torch.float64).reshape(-1, 3), cell.detach().to(torch.float64).reshape(-1, 3, 3)
        Z, ptr = Z.to(torch.int64).reshape(-1), ptr.to(torch.int64).reshape(-1)
        B = cell.shape[0]
        if ptr.shape[0] != B + 1 or Z.shape[0] != pos.shape[0]:
            raise ValueError("find_symmetry: expected pos [N,3], cell [B,3,3], Z [N] and ptr [B+1]")
        if pbc is not None:
            pbc = torch.as_tensor(pbc, device=pos.device).to(torch.bool).reshape(-1, 3).expand(B, 3)
    else:
        pos, cell, Z, ptr, pbc = _host_packed(structures, pos, cell, Z, ptr, pbc)
        pos, cell, Z, ptr = (torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in (pos, cell, Z, ptr))
        if pbc is not None:
            pbc = torch.from_numpy(pbc).to(device)
    pbc8 = None if pbc is None else pbc.to(torch.uint8).contiguous()
    B, n = cell.shape[0], pos.shape[0]
    lattice = _ops.lattice_group(cell, symprec)
    rot, rot_int, trans, n_rot, src, n_trans, ttrans, tsrc, flags = _ops.crystal_symmetry(pos, cell, Z, ptr, lattice, pbc8, symprec,
                                                                                          max_trans)
    row_struct = torch.searchsorted(ptr[1:].contiguous(), torch.arange(n, dtype=torch.int64, device=pos.device), right=True).to(torch.int32)
    return CrystalSymmetry(rotations=rot.view(B, MAX_OPS, 3, 3), rotations_int=rot_int.view(B, MAX_OPS, 3, 3), translations=trans,
                           n_rot=n_rot, src=src, n_trans=n_trans, pure_translations=ttrans, tsrc=tsrc, flags=flags, ptr=ptr,
                           row_struct=row_struct)


def lattice_group_host(cell, symprec: float = 1e-3):
    """numpy restatement of the lattice step -> (N [B,48,9] int8, n_lat [B], flags [B]): EVERY integer matrix with row
    entries in [-m_j, m_j] is held to |(N G N^T)_ij - G_ij| <= 2 symprec a_max (no candidate rows: not the kernel's method)"""
    cell = np.asarray(cell, dtype=np.float64).reshape(-1, 3, 3)
    B = len(cell)
    N_out, n_lat, flags = np.zeros((B, MAX_OPS, 9), dtype=np.int8), np.ones(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
    N_out[:, 0] = np.eye(3, dtype=np.int8).reshape(9)
    for b, L in enumerate(cell):
        with np.errstate(all="ignore"):
            if not np.isfinite(L).all() or not abs(np.linalg.det(L)) > _SINGULAR:
                flags[b] = SYM_NOT_FINITE
                continue
            G = L @ L.T
            a_max = np.sqrt(np.diag(G).max())
            m = np.floor((a_max + symprec) * np.linalg.norm(np.linalg.inv(L), axis=0))
        if not (m <= _MAX_M).all():
            flags[b] = SYM_RANGE
            continue
        m = m.astype(int)
        rows = np.array([(i, j, k) for i in range(-m[0], m[0] + 1) for j in range(-m[1], m[1] + 1) for k in range(-m[2], m[2] + 1)])
        tol = 2.0 * symprec * a_max
        Q = rows @ G @ rows.T                                # Q[a,b] = r_a G r_b^T
        d = np.diag(Q)
        found = []
        for a in range(len(rows)):                           # first row a, every (second, third) pair at once
            ok = (np.abs(d[a] - G[0, 0]) <= tol) & (np.abs(d - G[1, 1]) <= tol)[:, None] & (np.abs(d - G[2, 2]) <= tol)[None, :] \
                & (np.abs(Q[a] - G[0, 1]) <= tol)[:, None] & (np.abs(Q[a] - G[0, 2]) <= tol)[None, :] & (np.abs(Q - G[1, 2]) <= tol)
            for bb, cc in zip(*np.nonzero(ok)):
                found.append(np.concatenate([rows[a], rows[bb], rows[cc]]))
        eye = np.eye(3, dtype=int).reshape(9)
        found = [eye] + [f for f in found if not np.array_equal(f, eye)]
        if len(found) > MAX_OPS:
            flags[b] = SYM_AMBIGUOUS
            continue
        n_lat[b] = len(found)
        N_out[b, :len(found)] = np.asarray(found, dtype=np.int8)
    return N_out, n_lat, flags


def _polar(M):
    U, _, Vt = np.linalg.svd(M)
    return U @ Vt


def find_symmetry_host(structures=None, *, pos=None, cell=None, Z=None, ptr=None, pbc=None, symprec: float = 1e-3,
                       max_trans: int = 64) -> HostSymmetry:
    """numpy fp64 restatement of ``find_symmetry`` from the definitions (every lattice matrix enumerated, every (N, j)
    pair tested in full: no early exits): the tests hold the kernels to it"""
    pos, cell, Z, ptr, pbc = _host_packed(structures, pos, cell, Z, ptr, pbc)
    B, n_all = len(cell), len(pos)
    N_lat, n_lat, lat_flags = lattice_group_host(cell, symprec)
    rot, rot_int = np.zeros((B, MAX_OPS, 3, 3)), np.zeros((B, MAX_OPS, 3, 3), dtype=np.int8)
    trans, n_rot = np.zeros((B, MAX_OPS, 3)), np.ones(B, dtype=np.int32)
    src, tsrc = np.full((MAX_OPS, n_all), -1, dtype=np.int32), np.full((max_trans, n_all), -1, dtype=np.int32)
    n_trans, ttrans, flags = np.ones(B, dtype=np.int32), np.zeros((B, max_trans, 3)), lat_flags.copy()
    for b in range(B):
        lo, hi = int(ptr[b]), int(ptr[b + 1])
        n, L, z = hi - lo, cell[b], Z[lo:hi]
        if n < 1 or not np.isfinite(pos[lo:hi]).all():
            flags[b] |= SYM_NOT_FINITE
        if n > _ops.SYM_MAX_ATOMS:
            flags[b] |= SYM_TOO_LARGE
        if pbc is not None and not pbc[b].all():
            flags[b] |= SYM_NOT_PERIODIC
        ops_found, pure, ambiguous = [], [], False
        if not flags[b]:
            f = pos[lo:hi] @ np.linalg.inv(L)
            species, counts = np.unique(z, return_counts=True)
            zp = species[np.lexsort((species, counts))[0]]           # the fewest atoms, ties to the smallest Z
            pivots = np.nonzero(z == zp)[0]
            p = pivots[0]
            same = z[:, None] == z[None, :]
            step = max(1, 2_000_000 // (n * n))
            for g in range(n_lat[b]):
                N = N_lat[b, g].reshape(3, 3).astype(np.float64)
                fN = f @ N
                first = None
                for c0 in range(0, len(pivots), step):
                    js = pivots[c0:c0 + step]
                    t = f[js] - fN[p]                                     # [J,3]
                    d = fN[None, :, None, :] + t[:, None, None, :] - f[None, None, :, :]
                    d -= np.round(d)
                    cart = d @ L
                    match = ((cart * cart).sum(-1) <= symprec * symprec) & same[None]
                    accepted = match.any(axis=2).all(axis=1)
                    for q in np.nonzero(accepted)[0]:
                        many = bool((match[q].sum(axis=1) > 1).any())
                        image = match[q].argmax(axis=1)                   # atom i lands on atom image[i]
                        many = many or len(np.unique(image)) < n
                        entry = (N, t[q], image, many)
                        if first is None:
                            first = entry
                        if g == 0:
                            pure.append(entry)
                if first is not None:
                    ops_found.append(first)
            ambiguous = any(e[3] for e in ops_found + pure)
            if ambiguous:
                flags[b] |= SYM_AMBIGUOUS
        if flags[b] & SYM_IDENTITY_ONLY:
            rot[b, 0], rot_int[b, 0] = np.eye(3), np.eye(3, dtype=np.int8)
            src[0, lo:hi] = tsrc[0, lo:hi] = np.arange(lo, hi)
            continue
        n_rot[b], n_trans[b] = len(ops_found), len(pure)
        Li = np.linalg.inv(L)
        for g, (N, t, image, _) in enumerate(ops_found):
            rot_int[b, g] = N.astype(np.int8)
            rot[b, g] = _polar((Li @ N @ L).T)
            trans[b, g] = t - np.round(t)
            src[g, lo + image] = lo + np.arange(n)
        for tau, (_, t, image, _) in enumerate(pure[:max_trans]):
            ttrans[b, tau] = t - np.round(t)
            tsrc[tau, lo + image] = lo + np.arange(n)
        if len(pure) > max_trans:
            flags[b] |= SYM_TRUNC
    row_struct = np.repeat(np.arange(B, dtype=np.int32), np.diff(ptr))
    return HostSymmetry(rotations=rot, rotations_int=rot_int, translations=trans, n_rot=n_rot, src=src, n_trans=n_trans,
                        pure_translations=ttrans, tsrc=tsrc, flags=flags, ptr=ptr, row_struct=row_struct)


def _atom_deviation(x, out):
    xd, od = x.double(), out.double()
    num, den = (xd - od).norm(dim=1), xd.norm(dim=1)
    return torch.where((den == 0) & ~torch.isnan(num), torch.zeros_like(num), num / den)


def symmetrize_atoms(x, irreps_or_formula, sym: CrystalSymmetry, translations: bool = True, orth_tol: float = 1e-6):
    """(out, deviation [N]): per-atom irreps rows x [N,dim] (fp32 or fp64, on the device) averaged over their crystal's
    symmetry: out[k] = (1/n_rot) sum_g D(M_g) x[src[g,k]] over the point-group representatives, then with ``translations``
    the mean over the pure translations, out[k] <- (1/n_trans) sum_tau out[tsrc[tau,k]].  Every operation of the space group
    (modulo lattice translations) is one pure translation times one representative, so the two steps together are the
    average over the full group: the projection onto the tensors that the symmetry allows, equal on equivalent atoms up
    to their rotation.  A crystal whose translation list was truncated (SYM_TRUNC) gives NaN rows with ``translations``.
    deviation = |x - out| / |x| per atom (fp64, 0 for a zero row).  No gradient."""
    if not isinstance(x, torch.Tensor) or x.dim() != 2:
        raise ValueError("x: expected [N,dim] on the device")
    x = x.detach()
    irreps = irreps_of(irreps_or_formula)
    if x.shape[1] != irreps.dim or x.shape[0] != sym.row_struct.shape[0]:
        raise ValueError(f"x: expected [{sym.row_struct.shape[0]},{irreps.dim}], got {tuple(x.shape)}")
    layout = irreps_layout(irreps)
    D, flags = _ops.wigner_d(sym.rotations.reshape(-1, 3, 3), irreps.lmax if len(irreps) else 0, orth_tol)
    out = _ops.irreps_average_atoms(x, layout, D, flags, sym.n_rot, sym.row_struct, sym.src)
    if translations:
        n_ops = torch.where((sym.flags & SYM_TRUNC) != 0, torch.zeros_like(sym.n_trans), sym.n_trans)
        out = _ops.irreps_average_atoms(out, layout, None, None, n_ops, sym.row_struct, sym.tsrc)
    return out, _atom_deviation(x, out)


def symmetrize_atoms_host(x, irreps_or_formula, sym: HostSymmetry, translations: bool = True):
    """numpy fp64 restatement of ``symmetrize_atoms`` -> (out [N,dim], deviation [N])"""
    x = _host_x(x)
    out = np.full_like(x, np.nan)
    for b, c in enumerate(sym.crystals):
        lo, hi = int(sym.ptr[b]), int(sym.ptr[b + 1])
        D = _host_D(irreps_or_formula, c["rotations"])
        y = np.zeros((hi - lo, x.shape[1]))
        for g in range(len(D)):
            y += x[c["src"][g]] @ D[g].T
        y /= len(D)
        if translations:
            if c["flags"] & SYM_TRUNC:
                continue
            y = sum(y[c["tsrc"][tau] - lo] for tau in range(len(c["tsrc"]))) / len(c["tsrc"])
        out[lo:hi] = y
    with np.errstate(invalid="ignore", divide="ignore"):
        num, den = np.linalg.norm(x - out, axis=1), np.linalg.norm(x, axis=1)
        dev = np.where((den == 0) & ~np.isnan(num), 0.0, num / den)
    return out, dev
