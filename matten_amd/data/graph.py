"""
Host-side crystal graph construction and batching (the producer side of the backbone's data dict).

Contract kept from the reference (data/data.py:285-413, which delegates to ASE):
  * edges are all ordered triples (i, j, S) with |r_j + S.cell - r_i| < r_cut (strict, fp64),
    periodic in x, y, z, minus the true self edges (i == j and S == 0)
  * edge_index[0] = i (centre), edge_index[1] = j (neighbour); edge_cell_shift = S as float
  * num_neigh = bincount(i); cell rows are lattice vectors
  * ``pbc`` (a bool or one per axis, as the reference hands it to ASE): an open axis generates no image, S_k = 0 there;
    its cell row may be zero (``cell=None``: a molecule) and, when it is not, stays in ``cell`` without any effect on
    the edges.  Atoms are never wrapped.
ASE leaves the order within a centre atom unspecified; here edges come out in the canonical
lexicographic order (i, j, Sx, Sy, Sz).

``collate`` lays a list of crystals out as the flat struct-of-arrays batch that PyG's
``Batch.from_data_list`` + ``tensor_property_to_dict`` (data/data.py:146-159) would produce.
"""
from typing import Dict, List, Optional, Sequence, Tuple

import os

import numpy as np
import torch
from scipy.spatial import cKDTree


def image_reach(pos: np.ndarray, cell: np.ndarray, r_cut: float) -> np.ndarray:
    """Number of periodic images to scan along each lattice direction so that no pair within r_cut is missed:
    cutoff over the lattice-plane spacing, plus the fractional extent of the atoms (they need not be wrapped)."""
    recip = np.linalg.inv(cell).T  # rows: reciprocal vectors (without 2 pi)
    plane_dist = 1.0 / np.linalg.norm(recip, axis=1)
    frac = pos @ np.linalg.inv(cell)
    span = frac.max(0) - frac.min(0) if len(pos) else np.zeros(3)
    return np.ceil(float(r_cut) / plane_dist + span).astype(int)


SINGULAR_CELL = 1e-12   # smallest volume / area / length of the periodic sub-lattice that counts as independent vectors


def normalize_pbc(pbc) -> Tuple[bool, bool, bool]:
    """a bool or three bools -> three bools (what ASE does with the reference's ``pbc`` argument)"""
    if isinstance(pbc, (bool, np.bool_)):
        return (bool(pbc),) * 3
    flags = tuple(bool(p) for p in np.asarray(pbc).reshape(-1))
    if len(flags) != 3:
        raise ValueError(f"pbc must be a bool or three bools, got {pbc!r}")
    return flags


def complete_cell(cell: np.ndarray, pbc) -> np.ndarray:
    """The cell the image bounds are derived from: every open-axis row replaced by a unit vector orthogonal to the
    periodic rows (``ase.geometry.complete_cell`` for the rows a molecule, wire or slab leaves zero; a non-zero row on
    an open axis generates no image, so it is treated as absent too and can never make the cell singular).  It serves
    the inverse and nothing else: the column of the inverse that belongs to a periodic axis lies in the span of the
    periodic rows whatever the completion, and the open axes get no fractional coordinate or bound at all."""
    pbc = normalize_pbc(pbc)
    cell = np.array(cell, dtype=np.float64).reshape(3, 3)
    per = [k for k in range(3) if pbc[k]]
    if len(per) == 3:
        return cell
    if len(per) == 0:
        return np.eye(3)
    with np.errstate(all="ignore"):
        if len(per) == 2:
            o = 3 - per[0] - per[1]
            n = np.cross(cell[(o + 1) % 3], cell[(o + 2) % 3])
            cell[o] = n / np.linalg.norm(n)
        else:
            k = per[0]
            e = np.zeros(3)
            e[int(np.argmin(np.abs(cell[k])))] = 1.0
            u = np.cross(cell[k], e)
            u = u / np.linalg.norm(u)
            v = np.cross(cell[k], u)
            cell[(k + 1) % 3], cell[(k + 2) % 3] = u, v / np.linalg.norm(v)
    return cell


def periodic_volume(cell: np.ndarray, pbc: np.ndarray) -> np.ndarray:
    """cell [B,3,3], pbc [B,3] -> [B]: volume (three periodic axes: |det|), area (two) or length (one) spanned by the
    periodic vectors, 1 for an open structure.  > SINGULAR_CELL <=> the periodic vectors are linearly independent: the
    validity test of the packers and of the device prologue (|det| of the completed cell is this number)."""
    cell = np.asarray(cell, dtype=np.float64).reshape(-1, 3, 3)
    pbc = np.asarray(pbc, dtype=bool).reshape(-1, 3)
    n_per = pbc.sum(1)
    with np.errstate(all="ignore"):
        out = np.abs(np.linalg.det(cell))
        for b in np.nonzero(n_per < 3)[0]:
            rows = cell[b][pbc[b]]
            out[b] = (1.0 if len(rows) == 0 else np.linalg.norm(rows[0]) if len(rows) == 1
                      else np.linalg.norm(np.cross(rows[0], rows[1])))
    return out


def image_reach_pbc(pos: np.ndarray, cell: np.ndarray, r_cut: float, pbc) -> np.ndarray:
    """``image_reach`` with open axes: 0 images there; on the periodic axes the bound of the completed cell."""
    pbc = normalize_pbc(pbc)
    if all(pbc):
        return image_reach(pos, cell, r_cut)
    if not any(pbc):
        return np.zeros(3, dtype=int)
    if not periodic_volume(cell, pbc)[0] > SINGULAR_CELL:   # (also catches NaN)
        raise ValueError(f"zero or linearly dependent lattice vectors on the periodic axes (pbc={pbc})")
    reach = image_reach(pos, complete_cell(cell, pbc), r_cut)
    reach[~np.asarray(pbc)] = 0
    return reach


def neighbor_list(pos: np.ndarray, cell: np.ndarray, r_cut: float, pbc=True):
    """-> edge_index [2,E] int64, shifts [E,3] int64 (canonical order).  Host builder (scipy KD-tree); the
    production path for batches is ``batch_graphs_gpu`` below, which emits the identical list on the device.
    ``pbc``: see the module docstring; ``cell`` may be None (or hold zero rows) only where no image is generated."""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    pbc = normalize_pbc(pbc)
    cell = np.zeros((3, 3)) if cell is None else np.asarray(cell, dtype=np.float64).reshape(3, 3)
    n = pos.shape[0]
    rc = float(r_cut)
    reach = image_reach(pos, cell, rc) if all(pbc) else image_reach_pbc(pos, cell, rc, pbc)

    # candidate images: every lattice shift in the reach box; a KD-tree over the image atoms prunes
    # the pair search, the strict fp64 test below decides (same expression as the brute-force form)
    rng = [np.arange(-m, m + 1) for m in reach]
    S = np.stack(np.meshgrid(*rng, indexing="ij"), axis=-1).reshape(-1, 3)
    T = S @ cell
    img = (pos[None, :, :] + T[:, None, :]).reshape(-1, 3)  # [ns*n, 3], index = s*n + j
    tree = cKDTree(img)
    cand = tree.query_ball_point(pos, rc * (1.0 + 1e-9) + 1e-9)
    i = np.repeat(np.arange(n), [len(c) for c in cand])
    flat = np.concatenate([np.asarray(c, dtype=np.int64) for c in cand]) if len(i) else np.zeros(0, dtype=np.int64)
    sidx, j = flat // n, flat % n
    d = (pos[j] + T[sidx]) - pos[i]
    ok = np.sqrt((d * d).sum(-1)) < rc
    ok &= ~((i == j) & np.all(S[sidx] == 0, axis=1))
    i, j, s = i[ok], j[ok], S[sidx[ok]]
    if i.size == 0:
        raise ValueError("After eliminating self edges, no edges remain in this system.")
    order = np.lexsort((s[:, 2], s[:, 1], s[:, 0], j, i))
    return np.stack([i[order], j[order]]).astype(np.int64), s[order].astype(np.int64)


def crystal_graph(pos, cell, atomic_numbers, r_cut: float, y: Optional[Dict[str, torch.Tensor]] = None,
                  pbc=True, **extra) -> Dict[str, torch.Tensor]:
    """One crystal as the tensors a reference ``Crystal`` data point carries (data/data.py:134-144).  ``cell`` is
    returned as given (zeros for None), like the reference's ``Crystal.from_points``: never the completed cell."""
    pos = np.asarray(pos, dtype=np.float64)
    cell = np.zeros((3, 3)) if cell is None else np.asarray(cell, dtype=np.float64)
    edge_index, shifts = neighbor_list(pos, cell, r_cut, pbc)
    g = {
        "pos": torch.as_tensor(pos, dtype=torch.float32),
        "edge_index": torch.as_tensor(edge_index),
        "edge_cell_shift": torch.as_tensor(shifts, dtype=torch.float32),
        "cell": torch.as_tensor(cell, dtype=torch.float32),
        "num_neigh": torch.as_tensor(np.bincount(edge_index[0], minlength=len(pos)), dtype=torch.float32),
        "atomic_numbers": torch.as_tensor(np.asarray(atomic_numbers, dtype=np.int64)),
    }
    for k, v in {**(y or {}), **extra}.items():
        g[k] = torch.as_tensor(v)
    return g


def collate(graphs: Sequence[Dict[str, torch.Tensor]], device=None, pin: bool = False) -> Dict[str, torch.Tensor]:
    """Disjoint union of crystals: node offsets added to edge_index, `batch` and `ptr` appended."""
    sizes = [int(g["pos"].shape[0]) for g in graphs]
    ptr = np.zeros(len(graphs) + 1, dtype=np.int64)
    np.cumsum(sizes, out=ptr[1:])
    out: Dict[str, torch.Tensor] = {}
    keys = list(graphs[0].keys())
    for k in keys:
        if k == "edge_index":
            out[k] = torch.cat([g[k] + int(o) for g, o in zip(graphs, ptr[:-1])], dim=1)
        else:
            out[k] = torch.cat([g[k] for g in graphs], dim=0)
    out["batch"] = torch.repeat_interleave(torch.arange(len(graphs), dtype=torch.int64), torch.as_tensor(sizes))
    out["ptr"] = torch.from_numpy(ptr)
    if pin:
        out = {k: v.pin_memory() for k, v in out.items()}
    if device is not None:
        out = {k: v.to(device, non_blocking=pin) for k, v in out.items()}
    return out


def average_num_neighbors(graphs: Sequence[Dict[str, torch.Tensor]]) -> float:
    """dataset statistic the reference derives in get_to_model_info (dataset/structure_scalar_tensor.py:640-666)."""
    return float(torch.cat([g["num_neigh"] for g in graphs]).mean())


_MAX_CRYSTALS_PER_LAUNCH = 65535
EMIT_CSR = os.environ.get("MATTEN_GRAPH_EMIT_CSR", "1") != "0"   # device builder: batches carry their destination-sorted CSR


class EdgelessStructures(ValueError):
    """Some crystals of a batch have no edge inside the cutoff; ``indices`` are their positions in the batch."""

    def __init__(self, indices):
        super().__init__(f"After eliminating self edges, no edges remain in this system (structures {list(indices)}).")
        self.indices = list(indices)


class SingularCells(ValueError):
    """Some crystals of a batch have zero or linearly dependent lattice vectors on their periodic axes."""

    def __init__(self, indices):
        super().__init__(f"zero or linearly dependent lattice vectors on the periodic axes (structures {list(indices)}).")
        self.indices = list(indices)


def rows_min_atoms() -> int:
    """Size of the largest structure of a batch from which the device builder takes the pair-free search
    (matten_neighbor_rows_count / _fill) instead of the per-pair one.  The pair kernels keep 24 bytes per ordered atom
    pair and launch max_atoms^2 threads for EVERY crystal of the batch: 0.15 GB at 2000 atoms, 0.6 GB at 4000, 2.4 GB at 8000 (measured); the rows
    kernels walk every pair three times (count, recount, emit) with O(N) scratch.  Measured
    (docs/LAB_NOTES.md, tools/pbc_graph_bench.py): the rows build is level with the pair build at 1000 atoms (where the CSR
    the pair route emits still saves the forward its own build), 0.07-0.10 ms faster at 2000, 2.5x faster at 8000, and a
    batch of 200 fcc-64 crystals with ONE 2000-atom cluster builds in 0.32 instead of 1.69 ms.  Existing inputs (64 atoms
    at most) stay far below.  Read per call, so MATTEN_NEIGHBOR_ROWS_MIN_ATOMS=1 / a huge value force either route (tests, tools/pbc_graph_bench.py)."""
    return int(os.environ.get("MATTEN_NEIGHBOR_ROWS_MIN_ATOMS", "2048"))


def cells_min_atoms() -> int:
    """Size of the largest structure of a batch from which the rows search gets a cell list in front
    (matten_neighbor_cells_*: a centre atom tests the atoms of at most 27 bins instead of its whole structure).
    The default is measured (docs/LAB_NOTES.md, "Graph builder: the cell list"; tools/pbc_graph_bench.py --route, one
    structure per batch at 5 A, rows ms -> cells ms on one MI355X): the cell list costs five more launches and two scans,
    so at 2048 atoms it loses (fcc ball 0.30 -> 0.33, periodic supercell 0.22 -> 0.30); at 4096 it wins on both (0.53 ->
    0.33, 0.34 -> 0.28), by 2-3x at 8000, 7-17x at 32 000 and 27-62x at 100 000 (127 -> 2.0 ms).  4096 is the smallest
    power of two from which the cells build is not slower on either generator.  Where rows exceed the 512 records of the
    fill pass (14 A cutoff, ~500 edges per atom) the fallback makes the cells build 1.3x slower than rows at 8000 atoms
    and 1.3x faster at 32 000.
    Read per call; the route is taken when the largest structure has at least max(rows_min_atoms(), cells_min_atoms())
    atoms (``search_route``), so a huge MATTEN_NEIGHBOR_CELLS_MIN_ATOMS switches it off and
    MATTEN_NEIGHBOR_ROWS_MIN_ATOMS=1 alone still means the rows route."""
    return int(os.environ.get("MATTEN_NEIGHBOR_CELLS_MIN_ATOMS", "4096"))


def search_route(max_atoms: int) -> str:
    """The search kernels the device builder takes for a batch whose largest structure has ``max_atoms`` atoms:
    "pair" (one thread per ordered atom pair, emits the CSR), "rows" (one wave per centre atom, O(N) memory) or "cells"
    (rows behind a cell list, O(N) arithmetic too).  All three yield the same list bit for bit."""
    if max_atoms < rows_min_atoms():
        return "pair"
    return "cells" if max_atoms >= cells_min_atoms() else "rows"


CELLS_MAX_NB = 1 << 20   # bins along one axis before the cap at the atom count: matten_neighbor_cells_max_axis_bins()
                         # (tests/test_cells_host.py holds the two equal)


def cell_grid_host(pos: np.ndarray, cell: np.ndarray, pbc, r_cut: float) -> Tuple[np.ndarray, np.ndarray]:
    """-> (nb [3], bin_of_atom [n]): the grid of the cells route for one structure, restated in numpy; the bin of an atom
    is (c0 nb[1] + c1) nb[2] + c2 with c_k its index along axis k.
    Periodic axis k: nb_k = floor(1 / (bound_k (1 + 1e-6))) with bound_k = r_cut |inv[:, k]|, equal bins of
    frac - floor(frac); below three bins the axis collapses to one (with two, c - 1 and c + 1 are the same bin).
    Open axis: u = pos . inv[:, k] of the completed cell, bins r_cut |inv[:, k]| (1 + 1e-6) wide from the smallest u, no
    wrap.  |d . inv[:, k]| < r_cut |inv[:, k]| for every edge, so its two atoms lie in the same or in adjacent bins.
    The axis with the most bins is halved until the structure has no more bins than atoms."""
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    pbc = normalize_pbc(pbc)
    cell = np.zeros((3, 3)) if cell is None else np.asarray(cell, dtype=np.float64).reshape(3, 3)
    inv = np.linalg.inv(complete_cell(cell, pbc))
    n = len(pos)
    u = pos @ inv
    nb, raw, width, origin = [1] * 3, [1] * 3, [0.0] * 3, [0.0] * 3
    for k in range(3):
        b = float(r_cut) * float(np.linalg.norm(inv[:, k]))
        if pbc[k]:
            q = 1.0 / (b * (1.0 + 1e-6))
            nb[k] = raw[k] = min(int(q), CELLS_MAX_NB) if q >= 3.0 else 1
        else:
            width[k] = b * (1.0 + 1e-6)
            origin[k] = float(u[:, k].min()) if n else 0.0
            q = (float(u[:, k].max()) - origin[k]) / width[k] if n else 0.0
            nb[k] = raw[k] = (min(int(q), CELLS_MAX_NB - 2) if q >= 1.0 else 0) + 1
    while nb[0] * nb[1] * nb[2] > max(n, 1):
        k = int(np.argmax(nb))   # (the first of equals)
        nb[k] = (nb[k] + 1) // 2
        if pbc[k] and nb[k] < 3:
            nb[k] = 1
    bins = np.zeros((n, 3), dtype=np.int64)
    for k in range(3):
        if nb[k] == 1:
            continue
        if pbc[k]:
            t = (u[:, k] - np.floor(u[:, k])) * nb[k]
        else:
            t = (u[:, k] - origin[k]) / (width[k] * (raw[k] / nb[k]))
        bins[:, k] = np.clip(np.floor(t).astype(np.int64), 0, nb[k] - 1)
    return np.asarray(nb, dtype=np.int64), (bins[:, 0] * nb[1] + bins[:, 1]) * nb[2] + bins[:, 2]


def batch_graphs_gpu(structures: Sequence, r_cut: float, device="cuda", y: Optional[Dict[str, torch.Tensor]] = None,
                     ) -> Dict[str, torch.Tensor]:
    """Crystals -> collated batch, with the neighbour search on the GPU (matten_neighbor_count/_fill).

    ``structures`` is a sequence of (pos [n,3], cell [3,3], atomic_numbers [n]) triples or (pos, cell, atomic_numbers,
    pbc) items (cell may be None where no axis is periodic); they are packed into the flat struct-of-arrays form of
    ``batch_graphs_gpu_soa``, which callers that already hold their crystals as arrays should use directly (no
    per-structure Python work)."""
    sizes = np.array([len(s[0]) for s in structures], dtype=np.int64)
    ptr = np.zeros(len(structures) + 1, dtype=np.int64)
    np.cumsum(sizes, out=ptr[1:])
    pos = np.concatenate([np.asarray(s[0], dtype=np.float64).reshape(-1, 3) for s in structures])
    cell = np.stack([np.zeros((3, 3)) if s[1] is None else np.asarray(s[1], dtype=np.float64).reshape(3, 3)
                     for s in structures])
    Z = np.concatenate([np.asarray(s[2], dtype=np.int64).reshape(-1) for s in structures])
    pbc = None
    if any(len(s) > 3 for s in structures):
        pbc = np.array([normalize_pbc(s[3]) if len(s) > 3 else (True, True, True) for s in structures], dtype=bool)
    return batch_graphs_gpu_soa(pos, cell, Z, ptr, r_cut, device, y, pbc=pbc)


def batch_graphs_gpu_soa(pos: np.ndarray, cell: np.ndarray, Z: np.ndarray, ptr: np.ndarray, r_cut: float,
                         device="cuda", y: Optional[Dict[str, torch.Tensor]] = None, *, pbc=None) -> Dict[str, torch.Tensor]:
    """Flat batch (pos [N,3] fp64, cell [B,3,3] fp64, Z [N] int64, ptr [B+1] int64) ->
    collated graph batch on the device.

    The result has exactly the keys, dtypes and edge order of ``collate([crystal_graph(...) ...], device)``; only
    positions, cells and species cross PCIe (fp64 for the distance test, as in the host builder).  A crystal without
    any edge raises ``EdgelessStructures`` (a ValueError, like the reference data/data.py:398-402).

    ``pbc``: [B,3] bools (None: every axis of every crystal periodic); a crystal whose periodic vectors are linearly
    dependent raises ``SingularCells``.  A batch whose largest structure has ``rows_min_atoms()`` atoms or more is
    searched without per-pair bookkeeping (``search_route``: the rows or the cells kernels) and carries no CSR keys (the
    forward builds the CSR itself)."""
    from .. import ops

    pos = np.ascontiguousarray(pos, dtype=np.float64).reshape(-1, 3)
    cell = np.ascontiguousarray(cell, dtype=np.float64).reshape(-1, 3, 3)
    Z = np.ascontiguousarray(Z, dtype=np.int64).reshape(-1)
    ptr = np.ascontiguousarray(ptr, dtype=np.int64)
    sizes = np.diff(ptr)
    n_crystals = len(sizes)
    if pbc is not None:
        pbc = np.ascontiguousarray(pbc, dtype=bool).reshape(-1, 3)
        if len(pbc) != n_crystals:
            raise ValueError(f"pbc holds {len(pbc)} rows for {n_crystals} structures")
        if pbc.all():
            pbc = None   # fully periodic: the prologue and the kernels of every batch before pbc existed
    if n_crystals > _MAX_CRYSTALS_PER_LAUNCH:  # blockIdx.y of the neighbour kernels: build in slabs and concatenate
        parts = []
        for lo in range(0, n_crystals, _MAX_CRYSTALS_PER_LAUNCH):
            hi = min(n_crystals, lo + _MAX_CRYSTALS_PER_LAUNCH)
            a, b = ptr[lo], ptr[hi]
            try:
                parts.append(batch_graphs_gpu_soa(pos[a:b], cell[lo:hi], Z[a:b], ptr[lo : hi + 1] - a, r_cut, device,
                                                  pbc=None if pbc is None else pbc[lo:hi]))
                for k in [k for k in parts[-1] if k.startswith("_amd_")]:
                    del parts[-1][k]   # a slab's own CSR does not concatenate: the forward builds the whole batch's
            except EdgelessStructures as e:
                raise EdgelessStructures([lo + k for k in e.indices]) from None
            except SingularCells as e:
                raise SingularCells([lo + k for k in e.indices]) from None
        out, node_off, cry_off = {}, 0, 0
        for p in parts:
            p["edge_index"] = p["edge_index"] + node_off
            p["batch"] = p["batch"] + cry_off
            node_off += p["pos"].shape[0]
            cry_off += p["ptr"].shape[0] - 1
        for k in parts[0]:
            if k == "edge_index":
                out[k] = torch.cat([p[k] for p in parts], dim=1)
            elif k != "ptr":
                out[k] = torch.cat([p[k] for p in parts], dim=0)
        for k, v in (y or {}).items():
            out[k] = torch.as_tensor(v).to(out["pos"].device)
        out["ptr"] = torch.from_numpy(ptr).to(out["pos"].device)
        return out
    # Four arrays cross PCIe (positions, cells, species, the two running sums of the crystals); one kernel derives what
    # the search and the model need per crystal and per atom (ops.graph_prep), two passes find the edges, one 16-byte
    # read-back sizes the outputs.  (The first device builder did this prologue with ~45 small library launches: 0.5 ms
    # of host time per call, and bounded the image loops per crystal instead of per pair.)
    n_atoms = int(ptr[-1])
    dev = torch.device(device)
    pos_d = torch.from_numpy(pos).to(dev)
    cell_d = torch.from_numpy(cell.reshape(-1, 9)).to(dev)
    route = search_route(int(sizes.max())) if n_crystals > 0 else "pair"
    rows = route != "pair"
    if pbc is None and not rows:   # the common path: crystals of ordinary size
        pair_ptr = np.zeros(n_crystals + 1, dtype=np.int64)
        np.cumsum(sizes * sizes, out=pair_ptr[1:])
        n_pairs = int(pair_ptr[-1])
        ptrs_d = torch.from_numpy(np.stack([ptr, pair_ptr])).to(dev)
        ptr_d, pair_ptr_d = ptrs_d[0], ptrs_d[1]
        frac_d, bound_d, batch_d, pos32, cell32 = ops.graph_prep(pos_d, cell_d, ptr_d, r_cut)
        edge_index, shifts, num_neigh, pair_off, min_edges, csr = ops.neighbor_list(
            pos_d, cell_d, ptr_d, frac_d, bound_d, pair_ptr_d, r_cut, int(sizes.max()), n_pairs)
        if min_edges == 0:   # (came back with the edge count: no second sync on the common path)
            per_crystal = pair_off[pair_ptr_d[1:]] - pair_off[pair_ptr_d[:-1]]
            raise EdgelessStructures(torch.nonzero(per_crystal == 0).flatten().tolist())
    else:
        # open axes and / or large structures.  The read-back is three numbers here: the prologue's count of singular
        # cells travels with the edge count and the smallest edge count of a crystal.
        summary = torch.zeros(3, dtype=torch.int64, device=dev)
        singular = None
        if rows:
            ptr_d = torch.from_numpy(ptr).to(dev)
        else:
            pair_ptr = np.zeros(n_crystals + 1, dtype=np.int64)
            np.cumsum(sizes * sizes, out=pair_ptr[1:])
            ptrs_d = torch.from_numpy(np.stack([ptr, pair_ptr])).to(dev)
            ptr_d, pair_ptr_d = ptrs_d[0], ptrs_d[1]
        if pbc is None:
            frac_d, bound_d, batch_d, pos32, cell32 = ops.graph_prep(pos_d, cell_d, ptr_d, r_cut)
        else:
            pbc_d = torch.from_numpy(pbc.astype(np.uint8)).to(dev)
            frac_d, bound_d, batch_d, pos32, cell32, singular = ops.graph_prep_pbc(pos_d, cell_d, ptr_d, pbc_d, r_cut,
                                                                                   summary[2:])
        if rows:
            csr = None
            if route == "cells":
                edge_index, shifts, num_neigh, first, min_edges, host = ops.neighbor_list_cells(
                    pos_d, cell_d, ptr_d, batch_d, frac_d, bound_d, r_cut, summary,
                    pbc=None if pbc is None else pbc_d, singular=singular)
            else:
                edge_index, shifts, num_neigh, first, min_edges, host = ops.neighbor_list_rows(
                    pos_d, cell_d, ptr_d, batch_d, frac_d, bound_d, r_cut, summary)
            seg = ptr_d
        else:
            edge_index, shifts, num_neigh, first, min_edges, csr, host = ops.neighbor_list_flagged(
                pos_d, cell_d, ptr_d, frac_d, bound_d, pair_ptr_d, r_cut, int(sizes.max()), int(pair_ptr[-1]),
                summary=summary)
            seg = pair_ptr_d
        if host[2]:
            raise SingularCells(torch.nonzero(singular).flatten().tolist())
        if min_edges == 0:
            per_crystal = first[seg[1:]] - first[seg[:-1]]
            raise EdgelessStructures(torch.nonzero(per_crystal == 0).flatten().tolist())
    out = {
        "pos": pos32,
        "edge_index": edge_index,
        "edge_cell_shift": shifts,
        "cell": cell32,
        "num_neigh": num_neigh,
        "atomic_numbers": torch.from_numpy(Z).to(dev),
    }
    for k, v in (y or {}).items():
        out[k] = torch.as_tensor(v).to(dev)
    out["batch"] = batch_d
    out["ptr"] = ptr_d
    if csr is not None and EMIT_CSR:
        # the destination-sorted view every conv layer walks, emitted by the search itself (bit-identical to what
        # matten_csr_build derives from edge_index: tests/test_gpu_parity.py); the forward then skips that build.  Private
        # keys: whoever edits edge_index afterwards must drop them (nn/_nequip.ensure_graph trusts them when present)
        from ._key import AMD_PERM, AMD_ROWPTR, AMD_SRC

        out[AMD_PERM], out[AMD_ROWPTR], out[AMD_SRC] = csr
    return out
