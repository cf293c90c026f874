"""
The edge list of the SAME atoms rebuilt on the device for new positions and cells, without a host read.

``geometry.py`` differentiates a prediction with respect to positions, cells and strain on a FIXED edge list.  Whoever
then moves the atoms -- a strain or volume sweep, the frames of a trajectory, a structure optimisation, a
finite-difference check -- needs the list of the new geometry.  ``batch_graphs_gpu_soa`` builds it, but re-uploads from
numpy and reads the edge count back to size its outputs (``ops.neighbor_list_flagged``): a host sync per geometry, so
the loop cannot be captured.

``GeometryBatch`` keeps one padded batch of fixed capacity (N_b, E_b, B_b) -- the layout of the padded training batches,
``GraphStoreHost.padded_reference`` -- and ``update`` rewrites it in place from device tensors: prologue, counting pass,
scan, capped fill (``matten_neighbor_fill_capped``: the edge count stays on the device, the padding edges follow it in
closed form).  No allocation is sized by device data and nothing is read back, so "new positions -> edge list -> forward"
is one hipGraph replay (``graphs.GraphedGeometryStep``).  What can go wrong in an update is recorded in a flag word on the
device: more edges than the capacity (nothing is written then: the batch keeps the previous, valid list), a crystal
without any edge, a singular periodic cell.  ``check`` reads it (the one sync) and raises.

Scope: the pair search (structures below ``rows_min_atoms()`` atoms, at most 65535 crystals); atom counts and species
are fixed at construction.
"""
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _key as DataKey
from .graph import (_MAX_CRYSTALS_PER_LAUNCH, EdgelessStructures, SingularCells, batch_graphs_gpu_soa, rows_min_atoms)

FLAG_OVERFLOW, FLAG_EDGELESS, FLAG_SINGULAR = 1, 2, 4   # MATTEN_CAPPED_* (include/matten_hip.h)
EDGE_QUANTUM = 64

# the tensors an update rewrites from the edge list (an overflowing update leaves every one of them alone)
EDGE_KEYS = (DataKey.EDGE_INDEX, DataKey.EDGE_CELL_SHIFT, DataKey.NUM_NEIGH, DataKey.AMD_PERM, DataKey.AMD_ROWPTR,
             DataKey.AMD_SRC, DataKey.AMD_N_VALID)
TRAIN_KEYS = (DataKey.AMD_DST, DataKey.AMD_OUT_PTR, DataKey.AMD_OUT_PERM)


class EdgeCapacityExceeded(ValueError):
    """An update found more edges than the batch has room for; ``n_edges`` and ``capacity`` say how many.  The batch still
    holds the list of the update before (``GeometryBatch.grow`` makes room)."""

    def __init__(self, n_edges: int, capacity: int):
        super().__init__(f"the geometry has {int(n_edges)} edges inside the cutoff, the batch was built for {int(capacity)}: "
                         f"grow(edge_capacity) it (the edge list of the previous update is still in place)")
        self.n_edges, self.capacity = int(n_edges), int(capacity)


def edge_capacity_for(n_edges: int, slack: float = 1.25) -> int:
    """the default capacity for a structure of ``n_edges`` edges: 64 * ceil(slack * n_edges / 64)"""
    slack = float(slack)
    if not (slack >= 1.0 and np.isfinite(slack)):
        raise ValueError(f"slack {slack}: the capacity must hold the construction geometry (slack >= 1)")
    return EDGE_QUANTUM * int(-(-int(np.ceil(slack * int(n_edges))) // EDGE_QUANTUM))


def plan_capacity(n_atoms: int, n_crystals: int, n_edges: Optional[int], edge_capacity: Optional[int] = None,
                  slack: float = 1.25, pad_nodes: int = 1, pad_crystals: int = 1) -> Tuple[int, int, int]:
    """-> (N_b, E_b, B_b) of a ``GeometryBatch``, or a ValueError that names the limit.  ``n_edges``: the edge count of the
    construction geometry (None before it is known: then ``edge_capacity`` is checked alone).  ``pad_nodes`` padding atoms
    in ``pad_crystals`` padding crystals (each needs one)."""
    from ..graphs import _check_capturable

    pad_nodes, pad_crystals = int(pad_nodes), int(pad_crystals)
    if pad_crystals < 1:
        raise ValueError(f"pad_crystals = {pad_crystals}: a padded batch has at least one padding crystal")
    if pad_nodes < pad_crystals:
        raise ValueError(f"pad_nodes = {pad_nodes}: each of the {pad_crystals} padding crystals needs an atom")
    n_b, b_b = int(n_atoms) + pad_nodes, int(n_crystals) + pad_crystals
    if edge_capacity is None:
        if n_edges is None:
            raise ValueError("no edge count to derive a capacity from")
        e_b = edge_capacity_for(n_edges, slack)
    else:
        e_b = int(edge_capacity)
        if n_edges is not None and e_b < int(n_edges):
            raise ValueError(f"edge_capacity = {e_b} is below the {int(n_edges)} edges of the construction geometry")
        if e_b < 1:
            raise ValueError(f"edge_capacity = {e_b}: a batch holds at least one edge")
    if n_b >= 2 ** 31 or e_b >= 2 ** 31:
        raise ValueError(f"a batch of {n_b} atoms and {e_b} edges: both must stay below 2^31")
    # (shapes only: what a capture of this batch would be refused for)
    _check_capturable({"edge_index": torch.empty((2, e_b), device="meta"), "pos": torch.empty((n_b, 3), device="meta")})
    return n_b, e_b, b_b


class GeometryBatch:
    """One padded batch whose edge list follows the geometry (module docstring).

    ``pos`` [N,3], ``cell`` [B,3,3], ``Z`` [N], ``ptr`` [B+1]: the flat arrays of ``batch_graphs_gpu_soa`` (host); ``pbc``
    [B,3] bools or None.  Construction builds the graph once on the existing route (with its read-back), learns the edge
    count E0 and allocates every tensor of ``batch`` once: ``edge_capacity`` edges (default 64 * ceil(slack * E0 / 64)),
    ``pad_nodes`` padding atoms of species ``pad_species`` (default: the smallest atomic number present) in
    ``pad_crystals`` padding crystals with the cell ``pad_length`` * I.  ``training=True`` also keeps the tensors a
    backward walks (``_amd_dst_sorted``, ``_amd_out_ptr``, ``_amd_out_perm``), derived per update by ``ops.csr_build`` on the
    sorted source column.

    ValueError at construction: a structure of ``rows_min_atoms()`` atoms or more (the rows and cells searches are out of
    scope), more than 65535 crystals, a capacity below E0, a graph so dense that it could not be captured."""

    def __init__(self, pos, cell, Z, ptr, r_cut: float, device="cuda", pbc=None, edge_capacity: Optional[int] = None,
                 slack: float = 1.25, pad_nodes: int = 1, pad_crystals: int = 1, pad_species: Optional[int] = None,
                 pad_length: float = 2.0, training: bool = False):
        pos = np.ascontiguousarray(pos, dtype=np.float64).reshape(-1, 3)
        cell = np.ascontiguousarray(cell, dtype=np.float64).reshape(-1, 3, 3)
        Z = np.ascontiguousarray(Z, dtype=np.int64).reshape(-1)
        ptr = np.ascontiguousarray(ptr, dtype=np.int64).reshape(-1)
        sizes = np.diff(ptr)
        n_crystals, n_atoms = len(sizes), int(ptr[-1]) if len(ptr) else 0
        if n_crystals < 1 or ptr[0] != 0 or (sizes < 1).any() or len(pos) != n_atoms or len(Z) != n_atoms \
                or len(cell) != n_crystals:
            raise ValueError(f"pos {pos.shape}, cell {cell.shape}, Z {Z.shape}, ptr {ptr.shape}: expected [N,3], [B,3,3], [N] "
                             f"and the running sum [B+1] of at least one atom per crystal")
        if n_crystals > _MAX_CRYSTALS_PER_LAUNCH:
            raise ValueError(f"{n_crystals} crystals: one launch of the pair search takes at most {_MAX_CRYSTALS_PER_LAUNCH}")
        if int(sizes.max()) >= rows_min_atoms():
            raise ValueError(f"a structure of {int(sizes.max())} atoms: from rows_min_atoms() = {rows_min_atoms()} atoms on "
                             f"the builder searches without per-pair bookkeeping, which the capped rebuild does not cover")
        if pbc is not None:
            pbc = np.ascontiguousarray(pbc, dtype=bool).reshape(-1, 3)
            if len(pbc) != n_crystals:
                raise ValueError(f"pbc holds {len(pbc)} rows for {n_crystals} structures")
            if pbc.all():
                pbc = None
        species = np.unique(Z)
        z_pad = int(species[0]) if pad_species is None else int(pad_species)
        if z_pad not in species.tolist():
            raise ValueError(f"pad_species {z_pad} is none of the batch's species {species.tolist()}")
        length = float(pad_length)
        if not (length > 0.0 and np.isfinite(length)):
            raise ValueError(f"pad_length {pad_length}: a padding edge needs a positive length")
        if edge_capacity is not None:   # (everything that can be refused before the device is touched)
            plan_capacity(n_atoms, n_crystals, None, edge_capacity, slack, pad_nodes, pad_crystals)
        else:
            plan_capacity(n_atoms, n_crystals, 1, None, slack, pad_nodes, pad_crystals)
        self.device = torch.device(device)
        self.r_cut, self.training = float(r_cut), bool(training)
        self.n_atoms, self.n_crystals, self.max_atoms = n_atoms, n_crystals, int(sizes.max())
        # the construction geometry on the existing route: its read-back is where E0 comes from (and its exceptions are
        # those of every other batch: EdgelessStructures, SingularCells)
        first = batch_graphs_gpu_soa(pos, cell, Z, ptr, r_cut, self.device, pbc=pbc)
        self.n_edges_at_construction = int(first[DataKey.EDGE_INDEX].shape[1])
        self.n_b, self.e_b, self.b_b = plan_capacity(n_atoms, n_crystals, self.n_edges_at_construction, edge_capacity, slack,
                                                     pad_nodes, pad_crystals)
        dev = self.device
        pair_ptr = np.zeros(n_crystals + 1, dtype=np.int64)
        np.cumsum(sizes * sizes, out=pair_ptr[1:])
        self.n_pairs = int(pair_ptr[-1])
        ptrs = torch.from_numpy(np.stack([ptr, pair_ptr])).to(dev)
        self._ptr, self._pair_ptr = ptrs[0], ptrs[1]
        self.pos64 = torch.from_numpy(pos).to(dev)                    # [N,3]: what update() searches
        self.cell64 = torch.from_numpy(cell.reshape(-1, 9)).to(dev)   # [B,9]
        self._pbc = None if pbc is None else torch.from_numpy(pbc.astype(np.uint8)).to(dev)
        self._singular = None if pbc is None else torch.zeros(n_crystals, dtype=torch.int32, device=dev)
        self._n_singular = torch.zeros(1, dtype=torch.int64, device=dev)
        self._frac = torch.empty(n_atoms, 3, dtype=torch.float64, device=dev)
        self._bound = torch.empty(n_crystals, 3, dtype=torch.float64, device=dev)
        self._counts = torch.zeros(2 * self.n_pairs, dtype=torch.int32, device=dev)
        self._scan = torch.zeros(2 * self.n_pairs + 1, dtype=torch.int64, device=dev)
        self.flags = torch.zeros(1, dtype=torch.int32, device=dev)   # the sticky word check() reads and clears
        # the rows no update touches
        k = self.b_b - n_crystals
        p = self.n_b - n_atoms - (k - 1)
        pad_sizes = np.concatenate([[p], np.ones(k - 1, dtype=np.int64)])
        ptr_b = np.concatenate([ptr, n_atoms + np.cumsum(pad_sizes)])
        self._static = {
            DataKey.POSITIONS: torch.zeros(self.n_b, 3, dtype=torch.float32, device=dev),
            DataKey.CELL: (length * torch.eye(3, dtype=torch.float32)).repeat(self.b_b, 1).to(dev),
            DataKey.ATOMIC_NUMBERS: torch.from_numpy(np.concatenate([Z, np.full(self.n_b - n_atoms, z_pad, dtype=np.int64)])).to(dev),
            DataKey.BATCH: torch.from_numpy(np.repeat(np.arange(self.b_b, dtype=np.int64), np.diff(ptr_b))).to(dev),
            DataKey.PTR: torch.from_numpy(ptr_b).to(dev),
        }
        self.batch: Dict[str, torch.Tensor] = {}
        self._allocate(self.e_b)
        self.update()
        self.check()

    # ------------------------------------------------------------------------------------------------------------------
    def _allocate(self, e_b: int) -> None:
        """the tensors of ``batch`` for ``e_b`` edges, in the key order of ``padded_reference``; the static rows are shared"""
        dev, s = self.device, self._static
        i32 = dict(dtype=torch.int32, device=dev)
        self.e_b = int(e_b)
        b = {
            DataKey.POSITIONS: s[DataKey.POSITIONS],
            DataKey.EDGE_INDEX: torch.zeros(2, self.e_b, dtype=torch.int64, device=dev),
            DataKey.EDGE_CELL_SHIFT: torch.zeros(self.e_b, 3, dtype=torch.float32, device=dev),
            DataKey.CELL: s[DataKey.CELL],
            DataKey.NUM_NEIGH: torch.zeros(self.n_b, dtype=torch.float32, device=dev),
            DataKey.ATOMIC_NUMBERS: s[DataKey.ATOMIC_NUMBERS],
            DataKey.BATCH: s[DataKey.BATCH],
            DataKey.PTR: s[DataKey.PTR],
            DataKey.AMD_PERM: torch.zeros(self.e_b, **i32),
            DataKey.AMD_ROWPTR: torch.zeros(self.n_b + 1, **i32),
            DataKey.AMD_SRC: torch.zeros(self.e_b, **i32),
        }
        if self.training:
            b[DataKey.AMD_DST] = torch.zeros(self.e_b, **i32)
            b[DataKey.AMD_OUT_PTR] = torch.zeros(self.n_b + 1, **i32)
            b[DataKey.AMD_OUT_PERM] = torch.zeros(self.e_b, **i32)
        b[DataKey.AMD_N_VALID] = torch.zeros(3, dtype=torch.int64, device=dev)
        self.batch = b

    @property
    def capacity(self) -> Tuple[int, int, int]:
        """(N_b, E_b, B_b)"""
        return self.n_b, self.e_b, self.b_b

    @property
    def edge_count(self) -> torch.Tensor:
        """the edge count of the latest update as a device word (int64 [1]; it may exceed the capacity)"""
        return self._scan[self.n_pairs:self.n_pairs + 1]

    def update(self, pos=None, cell=None, flags_out=None) -> None:
        """Rewrite the batch for new positions ``pos`` [N,3] and / or cells ``cell`` [B,3,3] (device tensors; None: keep).
        No host sync and no allocation sized by device data: the call captures.  The search runs in fp64; an fp32 tensor
        is widened on the device, and the edge list is then that of the ROUNDED positions.  Rewritten: the real rows of
        ``pos`` / ``cell``, ``edge_index``, ``edge_cell_shift``, ``num_neigh``, the CSR keys and ``_amd_n_valid``.  With more
        edges than the capacity only ``pos`` / ``cell`` change: the edge list of the update before stays in place.
        ``flags_out``: an int32 device element that receives this update's flags instead of the sticky word ``check`` reads."""
        from .. import ops

        if pos is not None:
            if not isinstance(pos, torch.Tensor) or pos.device != self.device or tuple(pos.shape) != (self.n_atoms, 3) \
                    or pos.dtype not in (torch.float32, torch.float64):
                raise ValueError(f"pos: expected an fp64 (or fp32) tensor [{self.n_atoms}, 3] on {self.device}")
            self.pos64.copy_(pos)
        if cell is not None:
            if not isinstance(cell, torch.Tensor) or cell.device != self.device or cell.numel() != 9 * self.n_crystals \
                    or cell.dtype not in (torch.float32, torch.float64):
                raise ValueError(f"cell: expected an fp64 (or fp32) tensor [{self.n_crystals}, 3, 3] on {self.device}")
            self.cell64.copy_(cell.reshape(self.n_crystals, 9))
        flags = self.flags
        if flags_out is not None:
            if not isinstance(flags_out, torch.Tensor) or flags_out.dtype != torch.int32 or flags_out.numel() != 1 \
                    or flags_out.device != self.device or not flags_out.is_contiguous():
                raise ValueError("flags_out: expected one int32 element on the batch's device")
            flags = flags_out
            flags.zero_()   # (a fill kernel: the word holds this update's bits alone)
        b, n, nc = self.batch, self.n_atoms, self.n_crystals
        out = (self._frac, self._bound, b[DataKey.BATCH][:n], b[DataKey.POSITIONS][:n], b[DataKey.CELL][:3 * nc])
        if self._pbc is None:
            ops.graph_prep(self.pos64, self.cell64, self._ptr, self.r_cut, out=out)
        else:
            ops.graph_prep_pbc(self.pos64, self.cell64, self._ptr, self._pbc, self.r_cut, self._n_singular,
                               out=out + (self._singular,))
        ops.neighbor_list_capped(self.pos64, self.cell64, self._ptr, self._frac, self._bound, self._pair_ptr, self.r_cut,
                                 self.max_atoms, self.n_pairs, self.capacity, b[DataKey.EDGE_INDEX],
                                 b[DataKey.EDGE_CELL_SHIFT], b[DataKey.NUM_NEIGH], b[DataKey.AMD_PERM], b[DataKey.AMD_ROWPTR],
                                 b[DataKey.AMD_SRC], b[DataKey.AMD_N_VALID], flags, counts=self._counts, scan=self._scan,
                                 singular=self._singular)
        if self.training:
            # what nn/_nequip._training_edge_tensors derives: the padding edges have non-decreasing sources >= N, so the
            # stable grouping by source reproduces padded_reference (an overflowing update re-derives what is there)
            perm = b[DataKey.AMD_PERM].long()
            b[DataKey.AMD_DST].copy_(b[DataKey.EDGE_INDEX][1][perm])
            src = b[DataKey.AMD_SRC].long()
            out_perm, out_ptr, _, _ = ops.csr_build(torch.stack([src, src]), self.n_b)
            b[DataKey.AMD_OUT_PTR].copy_(out_ptr)
            b[DataKey.AMD_OUT_PERM].copy_(out_perm)

    def check(self) -> None:
        """Read the sticky flag word (the one host sync), clear it, and raise for what the updates since the last check
        recorded: ``SingularCells`` / ``EdgelessStructures`` with the crystal indices, ``EdgeCapacityExceeded`` with the edge
        count and the capacity -- indices and counts are those of the LATEST update."""
        word = int(self.flags.item())
        if not word:
            return
        self.flags.zero_()
        if word & FLAG_SINGULAR:
            raise SingularCells(torch.nonzero(self._singular).flatten().tolist())
        if word & FLAG_OVERFLOW:
            raise EdgeCapacityExceeded(int(self.edge_count.item()), self.e_b)
        first = self._scan[self._pair_ptr]
        raise EdgelessStructures(torch.nonzero(first[1:] == first[:-1]).flatten().tolist())

    def grow(self, edge_capacity: int) -> None:
        """New edge buffers of ``edge_capacity`` edges, filled from the current geometry.  ``batch`` holds NEW tensors
        afterwards: whatever was captured on the old ones (``GraphedGeometryStep``) must be captured again."""
        plan_capacity(self.n_atoms, self.n_crystals, None, edge_capacity, 1.0, self.n_b - self.n_atoms,
                      self.b_b - self.n_crystals)
        self._allocate(int(edge_capacity))
        self.update()
