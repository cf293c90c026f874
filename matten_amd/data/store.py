"""
Device-resident training set: the crystals of a data set uploaded once, batches gathered on the device.

``collate`` (data/graph.py; PyG's collate at reference data/dataset.py:150-152) concatenates the picked crystals on the
host for every batch of every epoch, and the forward then derives the destination-sorted CSR of the batch.  The graphs
never change between epochs, and a batch is a disjoint union with node and edge ranges in crystal order, so

  * every array of a batch is the concatenation of the picked crystals' rows, ``edge_index`` with the crystal's first
    node of the batch added;
  * the batch's stable destination-sorted CSR (``ops.csr_build``) is the concatenation of the crystals' own CSRs with the
    crystal's first node / first edge added, and so is the source-keyed CSR of the sorted list that
    ``ensure_training_edge_tensors`` derives: sources of a crystal lie in its node range, positions in its edge range.

``GraphStoreHost`` is the host half (running sums, key classes, ``plan``); ``DeviceGraphStore`` holds the flat arrays
and the crystal-relative CSRs on the device and assembles a batch with one small host-to-device copy (the plan's table)
and one ``matten_batch_gather`` launch.  Nothing is read back.
"""
from typing import Dict, List, Sequence, Tuple

import numpy as np
import torch

from . import _key as DataKey

NODE, EDGE, CRYSTAL = 0, 1, 2   # MATTEN_BATCH_NODE / _EDGE / _CRYSTAL (include/matten_hip.h)
OP_RAW, OP_ADD32_NODE, OP_ADD32_EDGE, OP_ADD64_NODE, OP_ROWPTR32, OP_BATCH64, OP_PTR64 = range(7)
STREAM_WORDS = 6
# matten_batch_gather_padded: two more words per stream, the fill of a RAW stream's padding rows and the fill's element
PAD_STREAM_WORDS = 8
PAD_ZERO, PAD_CONST, PAD_FIRST, PAD_DIAG3, PAD_DEGREE = range(5)

# key -> (class, dtype, shape of one crystal's tensor with n atoms / e edges written as "n" / "e")
CORE_KEYS = {
    DataKey.POSITIONS: (NODE, torch.float32, ("n", 3)),
    DataKey.EDGE_INDEX: (EDGE, torch.int64, (2, "e")),
    DataKey.EDGE_CELL_SHIFT: (EDGE, torch.float32, ("e", 3)),
    DataKey.CELL: (CRYSTAL, torch.float32, (3, 3)),
    DataKey.NUM_NEIGH: (NODE, torch.float32, ("n",)),
    DataKey.ATOMIC_NUMBERS: (NODE, torch.int64, ("n",)),
}
_RESERVED = (DataKey.BATCH, DataKey.PTR)

SLAB_EDGES = 1 << 24   # edges per csr_build call when the store derives its CSRs (whole crystals; far below its 2^31)


class GraphStoreHost:
    """Host half of a store, usable without a device: the flat arrays, the node and edge running sums, the class of
    every non-core key and the per-batch plan."""

    def __init__(self, graphs: Sequence[Dict[str, torch.Tensor]]):
        graphs = list(graphs)
        if not graphs:
            raise ValueError("a store needs at least one graph")
        self.n = len(graphs)
        self.keys: List[str] = list(graphs[0].keys())
        for k in CORE_KEYS:
            if k not in self.keys:
                raise ValueError(f"key '{k}' is missing from graph 0")
        for k in self.keys:
            if k in _RESERVED or k.startswith("_amd_"):
                raise ValueError(f"key '{k}' of graph 0 is written by the batch itself: a store takes un-collated graphs")
        n_atoms = np.empty(self.n, dtype=np.int64)
        n_edges = np.empty(self.n, dtype=np.int64)
        for i, g in enumerate(graphs):
            if list(g.keys()) != self.keys:
                raise ValueError(f"graph {i} holds keys {sorted(g.keys())}, graph 0 holds {sorted(self.keys)}")
            n_atoms[i], n_edges[i] = g[DataKey.POSITIONS].shape[0], g[DataKey.EDGE_INDEX].shape[-1]
            for k, (_, dtype, shape) in CORE_KEYS.items():
                want = tuple(n_atoms[i] if s == "n" else n_edges[i] if s == "e" else s for s in shape)
                if tuple(g[k].shape) != want or g[k].dtype != dtype:
                    raise ValueError(f"key '{k}' of graph {i} is {tuple(g[k].shape)} {g[k].dtype}, expected {want} {dtype}")
        self.node_ptr = np.zeros(self.n + 1, dtype=np.int64)
        self.edge_ptr = np.zeros(self.n + 1, dtype=np.int64)
        np.cumsum(n_atoms, out=self.node_ptr[1:])
        np.cumsum(n_edges, out=self.edge_ptr[1:])
        if self.node_ptr[-1] >= 2 ** 31 or self.edge_ptr[-1] >= 2 ** 31:
            raise ValueError("a store holds fewer than 2^31 atoms and 2^31 edges")
        self.classes: Dict[str, int] = {k: c for k, (c, _, _) in CORE_KEYS.items()}
        for k in self.keys:
            if k not in CORE_KEYS:
                self.classes[k] = self._classify(k, graphs, n_atoms, n_edges)
        # flat arrays: what collate's torch.cat yields over the whole set, edge_index with crystal-relative ids
        self.flat: Dict[str, torch.Tensor] = {}
        for k in self.keys:
            dim = 1 if k == DataKey.EDGE_INDEX else 0
            self.flat[k] = torch.cat([g[k] for g in graphs], dim=dim).contiguous()

    def _classify(self, key: str, graphs, n_atoms, n_edges) -> int:
        first = graphs[0][key]
        for i, g in enumerate(graphs):
            v = g[key]
            if not isinstance(v, torch.Tensor) or v.dim() == 0:
                raise ValueError(f"key '{key}' of graph {i} is not a tensor with a leading dimension")
            if v.dtype != first.dtype or v.shape[1:] != first.shape[1:]:
                raise ValueError(f"key '{key}' of graph {i} is {tuple(v.shape)} {v.dtype}, graph 0 has "
                                 f"{tuple(first.shape)} {first.dtype}")
        if first.element_size() not in (4, 8):
            raise ValueError(f"key '{key}' of graph 0 has {first.element_size()}-byte elements ({first.dtype}): the gather "
                             f"moves 4- and 8-byte elements")
        lead = np.array([g[key].shape[0] for g in graphs], dtype=np.int64)
        bad = {}
        for cls, want in ((NODE, n_atoms), (EDGE, n_edges), (CRYSTAL, np.ones_like(n_atoms))):
            miss = np.nonzero(lead != want)[0]
            if miss.size == 0:
                return cls
            bad[cls] = int(miss[0])
        i = max(bad.values())   # the first graph at which the last surviving class fails
        raise ValueError(f"key '{key}' of graph {i} has leading length {int(lead[i])}: neither its {int(n_atoms[i])} atoms, "
                         f"its {int(n_edges[i])} edges nor 1, like the graphs before it")

    def __len__(self) -> int:
        return self.n

    def plan(self, idx) -> Tuple[np.ndarray, int, int]:
        """-> (table int32 [5, B + 1], N_out, E_out) for the crystals ``idx`` in batch order; the table's rows are the
        destination node start, destination edge start, source node start, source edge start and source crystal, its
        closing column (N_out, E_out, 0, 0, 0): what matten_batch_gather takes."""
        idx = np.asarray(idx, dtype=np.int64).reshape(-1)
        if idx.size == 0:
            raise ValueError("an empty batch")
        if idx.min() < 0 or idx.max() >= self.n:
            raise IndexError(f"crystal ids {idx[(idx < 0) | (idx >= self.n)][:5].tolist()} outside a store of {self.n}")
        b = idx.size
        sums = np.zeros((2, b + 1), dtype=np.int64)
        np.cumsum(self.node_ptr[idx + 1] - self.node_ptr[idx], out=sums[0, 1:])
        np.cumsum(self.edge_ptr[idx + 1] - self.edge_ptr[idx], out=sums[1, 1:])
        n_out, e_out = int(sums[0, -1]), int(sums[1, -1])
        if n_out >= 2 ** 31 or e_out >= 2 ** 31:
            raise ValueError(f"a batch of {n_out} atoms and {e_out} edges: both must stay below 2^31")
        table = np.zeros((5, b + 1), dtype=np.int32)
        table[:2] = sums
        table[2, :b], table[3, :b], table[4, :b] = self.node_ptr[idx], self.edge_ptr[idx], idx
        return table, n_out, e_out

    # ---- padded batches: fixed sizes (N_b, E_b, B_b), so that a captured training step can replay them ----------------
    #
    # Behind the B picked crystals (N nodes, E edges, exactly the unpadded batch) come K = B_b - B >= 1 padding crystals.
    # Padding crystal 0 owns P = N_b - N - (K - 1) >= 1 nodes and all E_b - E padding edges; padding crystals 1 .. K-1 own
    # one node and no edge (the short last batch of an epoch).  Node j of padding crystal 0 owns the padding edges
    # [floor(j (E_b - E) / P), floor((j + 1) (E_b - E) / P)), each a self-image edge j -> j with cell shift (1, 0, 0) in the
    # cell pad_length * I: its length is pad_length > 0 (a zero-length edge is 0/0 in the harmonics), no padding crystal
    # is empty (mean pooling), and the padding edges are destination-sorted as they stand.
    def plan_padded(self, idx, pad_to) -> Tuple[np.ndarray, int, int]:
        """-> (table int32 [5, B_b + 1], N, E) for matten_batch_gather_padded: the destination running sums cover the
        padding crystals, the source rows of the padding columns are 0, the closing column is (N_b, E_b, N, E, B).
        ValueError unless B_b > B, E_b >= E and N_b >= N + (B_b - B)."""
        real, n, e = self.plan(idx)
        b = real.shape[1] - 1
        try:
            n_b, e_b, b_b = (int(v) for v in pad_to)
        except (TypeError, ValueError):
            raise ValueError(f"pad_to = {pad_to!r}: expected (nodes, edges, crystals)") from None
        k = b_b - b
        if k < 1:
            raise ValueError(f"pad_to asks for {b_b} crystals, the batch holds {b}: at least one padding crystal is needed")
        if e_b < e:
            raise ValueError(f"pad_to asks for {e_b} edges, the batch holds {e}")
        if n_b < n + k:
            raise ValueError(f"pad_to asks for {n_b} nodes, the batch holds {n} and its {k} padding crystals need one each")
        if n_b >= 2 ** 31 or e_b >= 2 ** 31:
            raise ValueError(f"a batch of {n_b} atoms and {e_b} edges: both must stay below 2^31")
        p = n_b - n - (k - 1)
        table = np.zeros((5, b_b + 1), dtype=np.int32)
        table[:, :b] = real[:, :b]
        table[0, b] = n
        table[0, b + 1:b_b] = n + p + np.arange(k - 1)
        table[1, b] = e
        table[1, b + 1:b_b] = e_b
        table[:, b_b] = (n_b, e_b, n, e, b)
        return table, n, e

    def pad_values(self, pad_species=None, pad_length: float = 2.0) -> Tuple[int, float]:
        """(species, length) of the padding atoms and edges, checked: the species must be one of the store's (default: its
        smallest atomic number), so that the model's species table holds it; the length must be positive"""
        species = np.unique(self.flat[DataKey.ATOMIC_NUMBERS].numpy())
        z = int(species[0]) if pad_species is None else int(pad_species)
        if z not in species.tolist():
            raise ValueError(f"pad_species {z} is none of the store's species {species.tolist()}")
        length = float(pad_length)
        if not (length > 0.0 and np.isfinite(length)):
            raise ValueError(f"pad_length {pad_length}: a padding edge needs a positive length")
        return z, length

    def padded_reference(self, idx, pad_to, pad_species=None, pad_length: float = 2.0,
                         training: bool = True) -> Dict[str, torch.Tensor]:
        """The padded batch restated on the host, key for key what ``DeviceGraphStore.batch(idx, pad_to=...)`` returns: the
        definition the kernel is tested against."""
        table, n, e = self.plan_padded(idx, pad_to)
        z, length = self.pad_values(pad_species, pad_length)
        b_b = table.shape[1] - 1
        n_b, e_b, b = int(table[0, -1]), int(table[1, -1]), int(table[4, -1])
        k, ep = b_b - b, e_b - e
        p = n_b - n - (k - 1)
        idx = np.asarray(idx, dtype=np.int64).reshape(-1)
        # padding node j of crystal 0 owns the edges [lo[j], lo[j + 1]) (python integers: exact)
        lo = np.array([j * ep // p for j in range(p + 1)], dtype=np.int64)
        owner = n + np.repeat(np.arange(p, dtype=np.int64), np.diff(lo))            # per padding edge
        degree = np.concatenate([np.diff(lo), np.zeros(k - 1, dtype=np.int64)])      # per padding node
        rows = {NODE: n_b - n, EDGE: ep, CRYSTAL: k}
        out: Dict[str, torch.Tensor] = {}
        for key in self.keys:
            flat, cls = self.flat[key], self.classes[key]
            ptr = self.node_ptr if cls == NODE else self.edge_ptr if cls == EDGE else np.arange(self.n + 1)
            if key == DataKey.EDGE_INDEX:
                real = torch.cat([flat[:, ptr[i]:ptr[i + 1]] + int(table[0, c]) for c, i in enumerate(idx)], dim=1)
                out[key] = torch.cat([real, torch.from_numpy(np.stack([owner, owner]))], dim=1)
                continue
            per = 3 if key == DataKey.CELL else 1   # (a crystal's cell is three rows)
            real = torch.cat([flat[per * ptr[i]:per * ptr[i + 1]] for i in idx], dim=0)
            pad = torch.zeros((per * rows[cls],) + tuple(flat.shape[1:]), dtype=flat.dtype)
            if key == DataKey.CELL:
                pad = (length * torch.eye(3, dtype=flat.dtype)).repeat(k, 1)
            elif key == DataKey.EDGE_CELL_SHIFT:
                pad[:, 0] = 1.0
            elif key == DataKey.ATOMIC_NUMBERS:
                pad[:] = z
            elif key == DataKey.NUM_NEIGH:
                pad = torch.from_numpy(degree).to(flat.dtype)
            out[key] = torch.cat([real, pad], dim=0)
        sizes = np.diff(table[0].astype(np.int64))   # nodes per crystal, the padding ones included
        out[DataKey.BATCH] = torch.from_numpy(np.repeat(np.arange(b_b, dtype=np.int64), sizes))
        out[DataKey.PTR] = torch.from_numpy(table[0].astype(np.int64))
        # the real part's CSR by a stable sort, the padding part by its closed form
        src, dst = (out[DataKey.EDGE_INDEX][r, :e].numpy() for r in (0, 1))
        perm = np.argsort(dst, kind="stable")
        src_s, dst_s = src[perm], dst[perm]
        out_perm = np.argsort(src_s, kind="stable")
        pad_ids = np.arange(e, e_b, dtype=np.int64)
        pad_ptr = np.concatenate([e + lo[:p], np.full(k, e_b, dtype=np.int64)])   # padding nodes, then the closing entry

        def rowptr(ids):
            return np.concatenate([np.searchsorted(ids, np.arange(n), side="left"), pad_ptr])

        i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a).astype(np.int32))
        out[DataKey.AMD_PERM] = i32(np.concatenate([perm, pad_ids]))
        out[DataKey.AMD_ROWPTR] = i32(rowptr(dst_s))
        out[DataKey.AMD_SRC] = i32(np.concatenate([src_s, owner]))
        if training:
            out[DataKey.AMD_DST] = i32(np.concatenate([dst_s, owner]))
            out[DataKey.AMD_OUT_PTR] = i32(rowptr(src_s[out_perm]))
            out[DataKey.AMD_OUT_PERM] = i32(np.concatenate([out_perm, pad_ids]))
        out[DataKey.AMD_N_VALID] = torch.tensor([n, e, b], dtype=torch.int64)
        return out


class DeviceGraphStore:
    """The whole set on one device.  ``batch(idx)`` returns what ``collate([graphs[i] for i in idx], device)`` returns,
    bit for bit, plus the batch's CSR keys (``_amd_perm``, ``_amd_rowptr``, ``_amd_src_sorted``: ``ops.csr_build`` of the
    batch) and, with ``training=True``, what ``ensure_training_edge_tensors`` derives (``_amd_dst_sorted`` and the
    source-keyed CSR as the two tensors ``_amd_out_ptr`` / ``_amd_out_perm``)."""

    def __init__(self, host: GraphStoreHost, device):
        from .. import _lib

        self.host = host
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.MattenHipError(f"a DeviceGraphStore lives on an MI355X, not on {self.device}")
        self._lib = _lib.load()
        self._max_streams = int(self._lib.matten_batch_gather_max_streams())
        self._dev = {k: v.to(self.device) for k, v in host.flat.items()}
        self._derive()
        # the streams of a batch in the key order of collate: (key, source tensor, dtype, row shape, class, operation)
        ei = self._dev[DataKey.EDGE_INDEX]
        self._public = []
        for k in host.keys:
            v = self._dev[k]
            if k == DataKey.EDGE_INDEX:
                self._public.append((k, ei, torch.int64, (), EDGE, OP_ADD64_NODE))
            elif k == DataKey.CELL:
                self._public.append((k, v, v.dtype, (3, 3), CRYSTAL, OP_RAW))
            else:
                self._public.append((k, v, v.dtype, tuple(v.shape[1:]), host.classes[k], OP_RAW))
        self._csr = [(DataKey.AMD_PERM, self._perm, EDGE, OP_ADD32_EDGE), (DataKey.AMD_ROWPTR, self._rowptr, NODE, OP_ROWPTR32),
                     (DataKey.AMD_SRC, self._src, EDGE, OP_ADD32_NODE)]
        self._train = [(DataKey.AMD_DST, self._dst, EDGE, OP_ADD32_NODE), (DataKey.AMD_OUT_PTR, self._out_ptr, NODE, OP_ROWPTR32),
                       (DataKey.AMD_OUT_PERM, self._out_perm, EDGE, OP_ADD32_EDGE)]

    @classmethod
    def from_graphs(cls, graphs: Sequence[Dict[str, torch.Tensor]], device) -> "DeviceGraphStore":
        return cls(GraphStoreHost(graphs), device)

    def _derive(self) -> None:
        """per-crystal CSR data, once: csr_build over slabs of whole crystals (a slab is itself a disjoint union, so its
        CSR is the concatenation of its crystals'), stored crystal-relative"""
        from .. import ops

        host, dev = self.host, self.device
        node_ptr, edge_ptr = host.node_ptr, host.edge_ptr
        n_nodes, n_edges = int(node_ptr[-1]), int(edge_ptr[-1])
        ei = self._dev[DataKey.EDGE_INDEX]
        i32 = dict(dtype=torch.int32, device=dev)
        self._perm, self._src, self._dst, self._out_perm = (torch.empty(n_edges, **i32) for _ in range(4))
        self._rowptr, self._out_ptr = (torch.empty(n_nodes, **i32) for _ in range(2))
        c0 = 0
        while c0 < host.n:
            c1 = int(np.searchsorted(edge_ptr, edge_ptr[c0] + SLAB_EDGES, side="right")) - 1
            c1 = min(max(c1, c0 + 1), host.n)
            n0, n1, e0, e1 = int(node_ptr[c0]), int(node_ptr[c1]), int(edge_ptr[c0]), int(edge_ptr[c1])
            sizes_n = torch.from_numpy(np.diff(node_ptr[c0:c1 + 1])).to(dev)
            sizes_e = torch.from_numpy(np.diff(edge_ptr[c0:c1 + 1])).to(dev)
            node_off = torch.from_numpy(node_ptr[c0:c1] - n0).to(dev)
            edge_off = torch.from_numpy(edge_ptr[c0:c1] - e0).to(dev)
            noff_e = torch.repeat_interleave(node_off, sizes_e, output_size=e1 - e0)   # per edge: its crystal's first node
            eoff_e = torch.repeat_interleave(edge_off, sizes_e, output_size=e1 - e0)
            eoff_n = torch.repeat_interleave(edge_off, sizes_n, output_size=n1 - n0)
            slab = (ei[:, e0:e1] + noff_e).contiguous()
            perm, rowptr, src, _ = ops.csr_build(slab, n1 - n0)
            dst = slab[1][perm.long()]
            srcl = src.long()
            out_perm, out_ptr, _, _ = ops.csr_build(torch.stack([srcl, srcl]), n1 - n0)
            self._perm[e0:e1] = perm - eoff_e
            self._src[e0:e1] = src - noff_e
            self._dst[e0:e1] = dst - noff_e
            self._out_perm[e0:e1] = out_perm - eoff_e
            self._rowptr[n0:n1] = rowptr[:-1] - eoff_n
            self._out_ptr[n0:n1] = out_ptr[:-1] - eoff_n
            c0 = c1

    def __len__(self) -> int:
        return self.host.n

    @property
    def nbytes(self) -> int:
        """bytes of device memory the store holds"""
        own = (self._perm, self._src, self._dst, self._out_perm, self._rowptr, self._out_ptr)
        return sum(t.numel() * t.element_size() for t in (*self._dev.values(), *own))

    def batch(self, idx, training: bool = True, pad_to=None, pad_species=None,
              pad_length: float = 2.0) -> Dict[str, torch.Tensor]:
        """pad_to = (N_b, E_b, B_b): the batch grown to exactly these sizes by padding crystals the same launch writes
        (layout: GraphStoreHost.plan_padded; the definition: GraphStoreHost.padded_reference), plus the tensor key
        ``_amd_n_valid`` = (N, E, B).  pad_to=None: the batch as it is."""
        from .. import _lib
        from ..ops import _stream

        padded = pad_to is not None
        if padded:
            table, n_real, e_real = self.host.plan_padded(idx, pad_to)
            z, length = self.host.pad_values(pad_species, pad_length)
            n_out, e_out = int(table[0, -1]), int(table[1, -1])
            # (CORE_KEYS pins these dtypes, checked per graph by GraphStoreHost: edge_cell_shift, cell and num_neigh are
            # float32, atomic_numbers int64 -- the fills below are elements of those widths)
            bits = lambda v: int(np.float32(v).view(np.int32))
            fills = {DataKey.EDGE_CELL_SHIFT: (PAD_FIRST, bits(1.0)), DataKey.CELL: (PAD_DIAG3, bits(length)),
                     DataKey.NUM_NEIGH: (PAD_DEGREE, 0), DataKey.ATOMIC_NUMBERS: (PAD_CONST, z)}
        else:
            table, n_out, e_out = self.host.plan(idx)
        b = table.shape[1] - 1
        dev = self.device
        rows = (n_out, e_out, b)
        out: Dict[str, torch.Tensor] = {}
        streams: List[Tuple[str, Tuple[int, ...]]] = []   # (key, the six words of the stream)
        for k, src, dtype, row, cls, op in self._public:
            if k == DataKey.EDGE_INDEX:
                dst = torch.empty((2, e_out), dtype=dtype, device=dev)
                stride = 8 * src.shape[1]
                streams.append((k, (src.data_ptr(), dst.data_ptr(), 8, 1, cls, op)))
                streams.append((k, (src.data_ptr() + stride, dst.data_ptr() + 8 * e_out, 8, 1, cls, op)))
            elif k == DataKey.CELL:
                dst = torch.empty((3 * b, 3), dtype=dtype, device=dev)
                streams.append((k, (src.data_ptr(), dst.data_ptr(), 4, 9, cls, op)))
            else:
                dst = torch.empty((rows[cls],) + row, dtype=dtype, device=dev)
                n_elem = 1
                for s in row:
                    n_elem *= s
                if n_elem == 0:
                    out[k] = dst
                    continue
                streams.append((k, (src.data_ptr(), dst.data_ptr(), src.element_size(), n_elem, cls, op)))
            out[k] = dst
        out[DataKey.BATCH] = torch.empty(n_out, dtype=torch.int64, device=dev)
        out[DataKey.PTR] = torch.empty(b + 1, dtype=torch.int64, device=dev)
        streams.append((DataKey.BATCH, (0, out[DataKey.BATCH].data_ptr(), 8, 1, NODE, OP_BATCH64)))
        streams.append((DataKey.PTR, (0, out[DataKey.PTR].data_ptr(), 8, 1, CRYSTAL, OP_PTR64)))
        for k, src, cls, op in (self._csr + self._train if training else self._csr):
            dst = torch.empty((n_out + 1) if op == OP_ROWPTR32 else e_out, dtype=torch.int32, device=dev)
            streams.append((k, (src.data_ptr(), dst.data_ptr(), 4, 1, cls, op)))
            out[k] = dst
        tab = torch.from_numpy(table).to(dev)   # the one host-to-device copy of a batch
        if padded:   # two more words per stream: the fill that follows its key
            desc = np.array([words + fills.get(k, (PAD_ZERO, 0)) for k, words in streams], dtype=np.int64)
            out[DataKey.AMD_N_VALID] = n_valid = torch.empty(3, dtype=torch.int64, device=dev)
            b_real = int(table[4, -1])
        else:
            desc = np.array([words for _, words in streams], dtype=np.int64)
        for lo in range(0, len(streams), self._max_streams):   # (one launch up to 32 streams: 17 extra keys)
            part = np.ascontiguousarray(desc[lo:lo + self._max_streams])
            if padded:
                _lib.check(self._lib.matten_batch_gather_padded(part.ctypes.data, part.shape[0], tab.data_ptr(), b, n_out,
                                                                e_out, b_real, n_real, e_real, n_valid.data_ptr(),
                                                                _stream()), "matten_batch_gather_padded")
            else:
                _lib.check(self._lib.matten_batch_gather(part.ctypes.data, part.shape[0], tab.data_ptr(), b, n_out, e_out,
                                                         _stream()), "matten_batch_gather")
        return out
