"""
Derived quantities of (predicted) per-atom rank-2 tensors, on the device: what NMR users read off a shielding tensor.

The reference's per-atom workflow ends at the raw 3 x 3 tensors (predict.py:117-148: one array per atom).  Two kernels
(``matten_rank2_props`` / ``matten_rank2_props_bwd``, csrc/rank2.hip) turn a batch of them into principal values and axes,
the isotropic value, span and skew, and the Haeberlen reduced anisotropy and asymmetry, in fp64, with the adjoint.
``rank2_properties`` / ``rank2_properties_from_irreps`` detach their input; ``rank2_invariants`` /
``rank2_invariants_from_irreps`` give the same bits attached to the autograd graph, and ``Rank2Loss`` is the loss to
fine-tune a per-atom tensor model against such scalars (isotropic shifts are plentiful where full tensors are rare) on the
dense selector layout.  ``rank2_host`` / ``rank2_bwd_host`` restate the definitions in numpy (LAPACK): the tests hold the
kernels to them.

Conventions ("Derived quantities of per-atom tensors"): the input is symmetrised, A = (T + T^T)/2, never
trusted; eigenvalues ascending l1 <= l2 <= l3, eigenvectors the columns of ``principal_axes`` in the same order (the sign
of a column is unspecified but deterministic).  iso = (l1 + l2 + l3)/3, span = l3 - l1, skew = 3 (l2 - iso)/span OF THE
TENSOR AS GIVEN -- for a shielding tensor the Herzfeld-Berger kappa is its negative --, zeta = l_z - iso with z the
principal value furthest from iso (l3 when skew <= 0, ties included, else l1), eta = (l_y - l_x)/zeta in [0, 1] with y = 2
and x the other extreme, anisotropy = 1.5 zeta.  Flags: bit 0 a non-finite input (the row is NaN, its gradient zero),
bit 1 span == 0 exactly (skew = eta = 0 by definition).  Values are in the units of the input.  The antisymmetric part,
gradients to the axes, second derivatives, Euler angles between tensors, EFG quantities and chemical-shift referencing
are not here.
"""
import numpy as np
import torch

from . import o3, ops

RANK2_NAMES = ("iso", "span", "skew", "zeta", "eta")      # the columns of the kernel's props [N,5], in order
FLAG_NOT_FINITE, FLAG_ISOTROPIC = 1, 2


class Rank2Properties:
    """Batch of derived quantities: ``principal_values`` [N,3] ascending, ``principal_axes`` [N,3,3] (columns),
    ``iso`` / ``span`` / ``skew`` / ``zeta`` / ``anisotropy`` (= 1.5 zeta) / ``eta`` [N], ``flags`` [N] int32 (bit 0
    non-finite input: the row is NaN; bit 1 a multiple of the identity), ``is_isotropic`` [N] bool; out of ``predict`` also
    ``ptr`` [S+1] int64: the atoms of structure s are the rows ptr[s]:ptr[s+1].  An unbatched input ([3,3]) gives the same
    without the leading dimension."""

    def __init__(self, **fields):
        self._names = tuple(fields)
        for k, v in fields.items():
            setattr(self, k, v)

    def _map(self, fn) -> "Rank2Properties":
        return Rank2Properties(**{k: fn(getattr(self, k)) for k in self._names})

    def cpu(self) -> "Rank2Properties":
        return self._map(lambda t: t.cpu())

    def to_dict(self) -> dict:
        """name -> numpy array on the host"""
        return {k: getattr(self, k).detach().cpu().numpy() for k in self._names}

    def __repr__(self):
        return f"Rank2Properties(atoms={tuple(self.flags.shape)})"


# ---------------------------------------------------------------------------------------------------
# the definitions in numpy (fp64, LAPACK)
# ---------------------------------------------------------------------------------------------------
def _host_rows(tensors) -> np.ndarray:
    if isinstance(tensors, torch.Tensor):
        tensors = tensors.detach().cpu().numpy()
    elif isinstance(tensors, (list, tuple)):
        tensors = np.stack([t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t) for t in tensors])
    T = np.asarray(tensors, dtype=np.float64)
    if T.shape[-2:] != (3, 3) or T.ndim not in (2, 3):
        raise ValueError(f"tensors: expected [N,3,3] or [3,3], got {T.shape}")
    return T.reshape(-1, 3, 3)


def rank2_host(tensors) -> dict:
    """The definitions of this module in numpy fp64 (``numpy.linalg.eigh``): ``tensors`` [N,3,3] or [3,3] (array, torch
    tensor or list) -> dict of [N]-leading arrays ``principal_values``, ``principal_axes``, ``iso``, ``span``, ``skew``,
    ``zeta``, ``anisotropy``, ``eta``, ``flags`` (int32), ``is_isotropic``."""
    T = _host_rows(tensors)
    ok = np.isfinite(T).all(axis=(1, 2))
    A = 0.5 * (T + T.transpose(0, 2, 1))
    A = np.where(ok[:, None, None], A, np.eye(3))
    # the isotropic part comes off first (t = tr(A)/3 as rounded): the axes are those of the deviator, and on it they are
    # resolved to eps span / gap instead of eps |A| / gap; the scalars are formed from the deviator's values d_k, l_k = t + d_k
    t0 = ((A[:, 0, 0] + A[:, 1, 1]) + A[:, 2, 2]) / 3.0
    lam, U = np.linalg.eigh(A - t0[:, None, None] * np.eye(3))
    dev = ((lam[:, 0] + lam[:, 1]) + lam[:, 2]) / 3.0
    iso = t0 + dev
    span = lam[:, 2] - lam[:, 0]
    flat = ok & (span == 0.0)
    safe = np.where(span == 0.0, 1.0, span)
    skew = np.where(flat, 0.0, 3.0 * (lam[:, 1] - dev) / safe)
    z_hi = skew <= 0.0
    lz, lx = np.where(z_hi, lam[:, 2], lam[:, 0]), np.where(z_hi, lam[:, 0], lam[:, 2])
    zeta = lz - dev
    eta = np.where(flat, 0.0, (lam[:, 1] - lx) / np.where(zeta == 0.0, 1.0, zeta))
    lam = lam + t0[:, None]
    nan = np.nan
    out = dict(principal_values=np.where(ok[:, None], lam, nan), principal_axes=np.where(ok[:, None, None], U, nan))
    for name, v in (("iso", iso), ("span", span), ("skew", skew), ("zeta", zeta), ("anisotropy", 1.5 * zeta), ("eta", eta)):
        out[name] = np.where(ok, v, nan)
    out["flags"] = (np.where(ok, 0, FLAG_NOT_FINITE) | np.where(flat, FLAG_ISOTROPIC, 0)).astype(np.int32)
    out["is_isotropic"] = flat
    return out


def rank2_bwd_host(tensors, g_vals=None, g_props=None) -> np.ndarray:
    """The adjoint in numpy fp64: ``tensors`` [N,3,3], the upstream gradients ``g_vals`` [N,3] and ``g_props`` [N,5] (order
    ``RANK2_NAMES``; None = zero) -> g_T [N,3,3] = U diag(w) U^T with w = g_vals + sum_q g_props[q] dq/dl.  Rows with flag
    bit 0 are zero whatever arrives; rows with bit 1 ignore the gradients of skew and eta."""
    T = _host_rows(tensors)
    n = T.shape[0]
    h = rank2_host(T)
    bad, flat = (h["flags"] & FLAG_NOT_FINITE) != 0, (h["flags"] & FLAG_ISOTROPIC) != 0
    U = np.where(bad[:, None, None], 0.0, h["principal_axes"])
    w = np.zeros((n, 3)) if g_vals is None else np.array(g_vals, dtype=np.float64).reshape(n, 3)
    if g_props is not None:
        g = np.asarray(g_props, dtype=np.float64).reshape(n, 5)
        span, skew, zeta, eta = (np.where(bad, 1.0, h[k]) for k in ("span", "skew", "zeta", "eta"))
        z_hi = skew <= 0.0
        third = 1.0 / 3.0
        one, zero = np.ones(n), np.zeros(n)
        dz = np.stack([np.where(z_hi, 0.0, 1.0) - third, -third * one, np.where(z_hi, 1.0, 0.0) - third], axis=1)
        dyx = np.stack([np.where(z_hi, -1.0, 0.0), one, np.where(z_hi, 0.0, -1.0)], axis=1)
        s = np.where(flat, 1.0, span)[:, None]
        z = np.where(flat, 1.0, zeta)[:, None]
        dskew = np.stack([skew - 1.0, 2.0 * one, -skew - 1.0], axis=1) / s
        deta = dyx / z - (eta[:, None] / z) * dz
        dspan = np.stack([-one, zero, one], axis=1)
        w = w + g[:, 0:1] * third + g[:, 1:2] * dspan + g[:, 3:4] * dz
        w = w + np.where(flat[:, None], 0.0, g[:, 2:3] * dskew + g[:, 4:5] * deta)
    g_t = np.einsum("nik,nk,njk->nij", U, np.where(bad[:, None], 0.0, w), U)
    g_t = 0.5 * (g_t + g_t.transpose(0, 2, 1))      # (the transpose of the symmetrisation)
    return np.where(bad[:, None, None], 0.0, g_t)


# ---------------------------------------------------------------------------------------------------
# on the device
# ---------------------------------------------------------------------------------------------------
def _default_device() -> torch.device:
    return torch.device("cuda", torch.cuda.current_device())


def _as_rows(tensors):
    """-> (rows [N,9] where the input is, unbatched?)"""
    if isinstance(tensors, (list, tuple)):
        if not tensors:
            raise ValueError("tensors: empty list")
        if isinstance(tensors[0], torch.Tensor):
            tensors = torch.stack(list(tensors))
        else:
            tensors = np.stack([np.asarray(t) for t in tensors])
    if not isinstance(tensors, torch.Tensor):
        a = np.asarray(tensors)
        if a.dtype not in (np.float32, np.float64):
            a = a.astype(np.float64)
        a = np.ascontiguousarray(a)
        tensors = torch.from_numpy(a if a.flags.writeable else a.copy())
    if tensors.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"tensors: expected fp32 or fp64, got {tensors.dtype}")
    shape = tuple(tensors.shape)
    if shape[-2:] != (3, 3) or len(shape) not in (2, 3):
        raise ValueError(f"tensors: expected [N,3,3] or [3,3], got {shape}")
    return tensors.reshape(-1, 9), len(shape) == 2


def _fields(vals, axes, props, flags, single: bool, ptr=None) -> Rank2Properties:
    fields = {"principal_values": vals, "principal_axes": axes}
    for q, name in enumerate(RANK2_NAMES):
        fields[name] = props[:, q]
        if name == "zeta":
            fields["anisotropy"] = 1.5 * props[:, q]
    fields["flags"] = flags
    fields["is_isotropic"] = (flags & FLAG_ISOTROPIC) != 0
    if single:
        fields = {k: v[0] for k, v in fields.items()}
    if ptr is not None:
        fields["ptr"] = ptr
    return Rank2Properties(**fields)


def rank2_properties(tensors, ptr=None) -> Rank2Properties:
    """``tensors``: a torch tensor or numpy array [N,3,3] or [3,3], fp32 or fp64, on the device or on the host (copied
    once), or a list of 3 x 3 arrays as ``predict(is_atomic_tensor=True)`` returns -> ``Rank2Properties`` on the device,
    without gradient."""
    rows, single = _as_rows(tensors)
    rows = rows.detach()
    if not rows.is_cuda:
        rows = rows.to(_default_device())
    return _fields(*ops.rank2_props(rows.contiguous()), single, ptr)


_BASIS = {}       # formula -> [n_irreps, 9] fp64 on the host
_Q, _QT = {}, {}  # (formula, device) -> fp32 [n_irreps, 9] / [9, n_irreps]


def rank2_basis(formula: str = "ij=ji") -> np.ndarray:
    """[6,9] fp64: the model's irreps components of a symmetric rank-2 tensor to the row-major 3 x 3 tensor,
    ``t.reshape(9) = x @ rank2_basis()`` (``o3.cartesian_tensor_basis`` flattened).  ValueError for a formula that is not
    a symmetric rank 2."""
    if formula not in _BASIS:
        try:
            _, Q = o3.cartesian_tensor_basis(formula)
        except Exception as e:
            raise ValueError(f"formula {formula!r}: not a Cartesian tensor formula ({e})") from e
        if Q.ndim != 3 or not np.allclose(Q, Q.transpose(0, 2, 1), atol=1e-12):
            raise ValueError(f"formula {formula!r} is not a symmetric rank-2 tensor (ij=ji)")
        B = np.ascontiguousarray(Q.reshape(Q.shape[0], 9), dtype=np.float64)
        B.setflags(write=False)
        _BASIS[formula] = B
    return _BASIS[formula]


def _device_basis(formula: str, device):
    key = (formula, torch.device(device))
    if key not in _Q:
        _Q[key] = torch.tensor(rank2_basis(formula), dtype=torch.float32, device=device)
        _QT[key] = _Q[key].t().contiguous()
    return _Q[key], _QT[key]


def _check_irreps(x, formula: str):
    B = rank2_basis(formula)
    if not isinstance(x, torch.Tensor) or x.dim() not in (1, 2):
        raise ValueError(f"x: expected a tensor [N,{B.shape[0]}] or [{B.shape[0]}]")
    if x.shape[-1] != B.shape[0]:
        raise ValueError(f"x: expected {B.shape[0]} irreps components per row for {formula!r}, got {x.shape[-1]}")
    return x.dim() == 1


def rank2_properties_from_irreps(x, formula: str = "ij=ji", ptr=None) -> Rank2Properties:
    """The same from the model's irreps rows ``x`` [N,6] (fp32): one ``dense_rows`` with ``rank2_basis`` gives the tensors."""
    single = _check_irreps(x, formula)
    x = x.detach().reshape(-1, x.shape[-1])
    if not x.is_cuda:
        x = x.to(_default_device())
    q, _ = _device_basis(formula, x.device)
    rows = ops.dense_rows(x.to(torch.float32), q)
    return _fields(*ops.rank2_props(rows), single, ptr)


# ---------------------------------------------------------------------------------------------------
# differentiable: training on the derived scalars
# ---------------------------------------------------------------------------------------------------
def rank2_invariants(tensors) -> Rank2Properties:
    """The differentiable ``rank2_properties``: ``tensors`` is a device tensor [N,3,3] or [3,3], fp32 or fp64; the principal
    values and the five scalars (and ``anisotropy``) come back attached to its autograd graph (same kernel forward, so the
    same bits; ``matten_rank2_props_bwd`` backward).  The axes, ``flags`` and ``is_isotropic`` carry no gradient; a row with
    flag bit 0 is NaN and sends a zero gradient back."""
    from .autograd import Rank2PropsFn

    if not isinstance(tensors, torch.Tensor) or not tensors.is_cuda:
        raise ValueError("tensors: rank2_invariants differentiates device tensors only; for arrays, lists and host "
                         "tensors use rank2_properties (no gradient)")
    if tensors.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"tensors: expected fp32 or fp64, got {tensors.dtype}")
    shape = tuple(tensors.shape)
    if shape[-2:] != (3, 3) or len(shape) not in (2, 3):
        raise ValueError(f"tensors: expected [N,3,3] or [3,3], got {shape}")
    return _fields(*Rank2PropsFn.apply(tensors.reshape(-1, 9)), len(shape) == 2)


def rank2_invariants_from_irreps(x, formula: str = "ij=ji") -> Rank2Properties:
    """The differentiable ``rank2_properties_from_irreps``: ``x`` [N,6] (or [6]) fp32 on the device, usually the model's
    output with its ``grad_fn``.  The forward is the same ``dense_rows``; its adjoint is ``dense_rows`` with the transposed
    basis [9,6]."""
    from .autograd import DenseRowsFn, Rank2PropsFn

    single = _check_irreps(x, formula)
    if not x.is_cuda or x.dtype != torch.float32:
        raise ValueError("x: rank2_invariants_from_irreps differentiates fp32 device tensors only; a host tensor goes "
                         "through rank2_properties_from_irreps (no gradient)")
    q, qt = _device_basis(formula, x.device)
    rows = DenseRowsFn.apply(x.reshape(-1, x.shape[-1]), q, qt)
    return _fields(*Rank2PropsFn.apply(rows), single)


class Rank2Loss(torch.nn.Module):
    """Loss on the derived scalars of per-atom tensors: ``forward(props, targets, selector)`` with ``props`` a
    ``Rank2Properties`` (of ``rank2_invariants`` or ``rank2_invariants_from_irreps``), ``targets`` a dict name -> [N] or
    [N,1] (one row per atom, the dense label layout) and ``selector`` the dense int32 [N].  The mean of the squared
    (``kind="mse"``) or absolute (``"l1"``) difference, weighted per name, over the selected atoms and the chosen names, by
    the selected-loss kernel (``autograd.SelectedLossFn``).  An atom whose tensor was not finite (flag bit 0) or whose target
    is not finite is taken out of the selector with ``torch.where``; nothing is read back, so it captures.
    ``names`` come from ``RANK2_NAMES``."""

    def __init__(self, names=("iso",), weights=None, kind: str = "mse"):
        super().__init__()
        names = (names,) if isinstance(names, str) else tuple(names)
        if not names:
            raise ValueError("names: at least one quantity is needed")
        unknown = [n for n in names if n not in RANK2_NAMES]
        if unknown:
            raise ValueError(f"names: {unknown} not in {RANK2_NAMES}")
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
        # a weight on a column's loss is a scale on the column's prediction and target: w |d| = |w d|, w d^2 = (sqrt(w) d)^2
        self._scales = {n: (w if kind == "l1" else float(np.sqrt(w))) for n, w in weights.items()}

    def forward(self, props: Rank2Properties, targets: dict, selector: torch.Tensor) -> torch.Tensor:
        from .autograd import SelectedLossFn

        missing = [n for n in self.names if n not in targets]
        if missing:
            raise ValueError(f"targets: no entry for {missing}")
        if selector.dtype == torch.bool or selector.is_floating_point():
            raise TypeError(f"selector is {selector.dtype}: the dense layout takes an integer selector")
        n_rows = props.flags.shape[0]
        if selector.shape != (n_rows,):
            raise ValueError(f"selector: expected [{n_rows}], got {tuple(selector.shape)}")
        pred_cols, target_cols = [], []
        for name in self.names:
            value = getattr(props, name)
            target = torch.as_tensor(targets[name], device=value.device)
            if target.shape not in ((n_rows,), (n_rows, 1)):
                raise ValueError(f"targets[{name!r}]: expected [{n_rows}] or [{n_rows},1], got {tuple(target.shape)}")
            target = target.reshape(n_rows).to(torch.float32)
            value = value.to(torch.float32)
            s = self._scales[name]
            if s != 1.0:
                value, target = value * s, target * s
            pred_cols.append(value)
            target_cols.append(target)
        pred, target = torch.stack(pred_cols, dim=1), torch.stack(target_cols, dim=1)
        use = ((props.flags & FLAG_NOT_FINITE) == 0) & torch.isfinite(target).all(dim=1)
        selector = torch.where(use, selector.to(torch.int32), torch.zeros((), dtype=torch.int32, device=selector.device))
        return SelectedLossFn.apply(pred, target, selector, ops.LOSS_KINDS[self.kind])[0]
