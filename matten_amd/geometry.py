"""
Gradients of a prediction with respect to the structure: atomic positions, cells and homogeneous strain.

The reference gets these from plain autograd through e3nn (its ``with_edge_vectors`` and spherical harmonics are torch
code, nn/_nequip.py:130-268).  Here the per-edge geometry is a kernel with a hand-written adjoint
(``autograd.EdgeGeomFn`` / ``matten_edge_geom_bwd``), the radial MLP returns dL/d(length)
(``matten_radial_mlp_bwd_len``) and the tensor product dL/d(harmonics) (``matten_tp_backward_sh``); a forward whose
``pos`` or ``cell`` requires grad chains them.  The edge list is fixed: an edge that crosses the cutoff contributes a
kink, as in the reference.  First derivatives only.  (A loop that moves the atoms rebuilds the list on the device with
``data.rebuild.GeometryBatch``; ``graphs.GraphedGeometryStep`` replays rebuild, forward and these gradients as one hipGraph.)

    out = geometry_gradients(model, batch, lambda p: elastic_moduli_from_irreps(p["elastic_tensor_full"]).k_vrh.sum())
    out["pos"]     # [N,3]    d k_vrh / d position: which atom moves the bulk modulus
    out["strain"]  # [B,3,3]  d k_vrh / d strain of each crystal
"""
from typing import Callable, Dict

import torch

from .data.irreps import DataKey

# entries of a batch dict that were computed from the positions / cells of an earlier forward
_DERIVED = (DataKey.AMD_GEOM, DataKey.AMD_SH, DataKey.EDGE_VECTORS, DataKey.EDGE_LENGTH, DataKey.EDGE_ATTRS,
            DataKey.EDGE_EMBEDDING, "_amd_h2s")


def strain_gradient(batch: Dict[str, torch.Tensor]) -> torch.Tensor:
    """dL/d(strain) [B,3,3] from the gradients a backward left on ``batch["pos"]`` and ``batch["cell"]``:

        dL/deps[b] = pos_b^T pos_b.grad + cell_b^T cell_b.grad

    the response to the homogeneous deformation x -> x (1 + eps) of a crystal's positions and lattice vectors together
    (rows of ``cell`` are the lattice vectors).  Symmetric for any rotation-invariant scalar L.  Without a cell (open
    structures) the second term is absent; without ``batch["batch"]`` all atoms belong to one crystal."""
    pos = batch[DataKey.POSITIONS]
    if pos.grad is None:
        raise ValueError("strain_gradient: batch['pos'].grad is None -- run a backward with pos.requires_grad first")
    cell = batch.get(DataKey.CELL)
    index = batch.get(DataKey.BATCH)
    n_crystals = 1
    if cell is not None:
        n_crystals = cell.numel() // 9
    elif index is not None and index.numel():
        n_crystals = int(index.max()) + 1
    outer = pos.detach().unsqueeze(2) * pos.grad.unsqueeze(1)          # [N,3,3]: x_i g_j per atom
    out = outer.new_zeros(n_crystals, 3, 3)
    if index is None:
        out[0] = outer.sum(0)
    else:
        out.index_add_(0, index, outer)
    if cell is not None and cell.grad is not None:
        out = out + cell.detach().reshape(-1, 3, 3).transpose(1, 2) @ cell.grad.reshape(-1, 3, 3)
    return out


def geometry_gradients(model, batch: Dict[str, torch.Tensor], fn: Callable, **forward_kwargs) -> Dict[str, torch.Tensor]:
    """Gradients of the scalar ``fn(preds)`` w.r.t. the structure: {"pos": [N,3], "cell": like batch["cell"] or None,
    "strain": [B,3,3]}.  ``batch`` is a dict as ``data.graph.collate`` builds it, on the model's device; its ``pos`` /
    ``cell`` are replaced by leaves that require grad (the caller's tensors are left alone), the forward runs with
    autograd on, ``fn(preds).backward()`` follows.  Parameters may be frozen and the model in eval(): the layers take
    their differentiable route whenever the geometry requires grad.  ``forward_kwargs`` go to the model's forward
    (``task_name="nmr_tensor"`` for the per-atom model)."""
    batch = dict(batch)
    for key in _DERIVED:
        batch.pop(key, None)
    dev = getattr(model, "device", None)
    for key in (DataKey.POSITIONS, DataKey.CELL):
        t = batch.get(key)
        if t is not None:
            t = t.detach()
            if dev is not None and t.device != dev:
                t = t.to(dev)
            batch[key] = t.clone().requires_grad_(True)
    with torch.enable_grad():
        preds, _ = model(batch, **forward_kwargs)
        fn(preds).backward()
    cell = batch.get(DataKey.CELL)
    return {"pos": batch[DataKey.POSITIONS].grad, "cell": None if cell is None else cell.grad, "strain": strain_gradient(batch)}
