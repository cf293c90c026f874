"""
``TensorDataModule``: the data module the reference's training script builds (scripts/train_materials_tensor.py:35-37;
dataset/structure_scalar_tensor.py:368-666), reduced to what feeds the message-passing path: the reference's JSON files
(``structure`` column = pymatgen ``Structure.as_dict()``, target column = Cartesian tensor) -> crystal graphs with the
neighbour list of ``matten_amd.data.graph`` -> collated batch dicts whose target is the irreps vector of the tensor
(``CartesianTensor.from_cartesian``, reference :262-267).  pymatgen / pandas / PyG / Lightning are not needed.

Per-atom targets (scripts/train_atomic_tensor.py, configs/atomic_tensor.yaml of the reference): ``atom_selector`` names a
column of per-atom flags and the target column holds one tensor per flagged atom.  ``atom_target_layout`` picks how the
labels are stored: "compact" is the reference's ([M, d] targets + a ``bool`` selector, consumed by ``preds[selector]``),
"dense" keeps one target row per atom (zeros where unselected) + an ``int32`` selector, which the device store, the
padded batches and the selected-loss kernels take as ordinary per-node keys.  The selector's dtype picks the route.

Padding: ``device_resident=True`` with ``loader_kwargs["pad"] = (node_quantum, edge_quantum)`` pads every TRAINING batch to a
few bucket shapes; ``pad_eval=True`` pads the validation and test batches the same way (unshuffled as ever), so that
``matten_amd.model.trainer.Trainer(graphed=True)`` replays captured steps in all three loops.  A model that sees padded
batches must keep the padding crystals out of loss and metric: ``BaseModel.loss_over_valid_rows``.

Not carried over (outside the path; ``NotImplementedError`` when asked for): featurizers (``global_featurizer``,
``atom_featurizer``), scalar targets, on-disk caching (``reuse``); target normalisation is available through
``normalize_tensor_target`` + ``matten_amd.data.transform`` (crystal targets only).
"""
import os
from typing import Any, Dict, Iterator, List, Optional

import numpy as np
import torch

from ..data.graph import collate, crystal_graph
from ..data.io import structures_from_json
from ..utils import CartesianTensorWrapper


class _Loader:
    """the subset of torch_geometric's DataLoader the training loop uses: iteration over collated batches"""

    def __init__(self, graphs: List[Dict[str, torch.Tensor]], batch_size: int = 1, shuffle: bool = False,
                 device=None, seed: int = 0, **ignored):
        self.graphs, self.batch_size, self.shuffle, self.device = graphs, int(batch_size), bool(shuffle), device
        self._gen = torch.Generator().manual_seed(seed)

    def __len__(self) -> int:
        return -(-len(self.graphs) // self.batch_size)

    def __iter__(self) -> Iterator[Dict[str, torch.Tensor]]:
        n = len(self.graphs)
        order = torch.randperm(n, generator=self._gen).tolist() if self.shuffle else list(range(n))
        for lo in range(0, n, self.batch_size):
            yield collate([self.graphs[i] for i in order[lo:lo + self.batch_size]], device=self.device)


class _DeviceLoader:
    """``_Loader`` over a device-resident store (``matten_amd.data.store.DeviceGraphStore``): the same ``batch_size`` /
    ``shuffle`` / ``seed`` semantics -- the same generator and the same ``randperm`` per epoch, so it visits the same
    crystals in the same order, the short last batch included -- with every batch gathered on the device.

    ``pad=(node_quantum, edge_quantum)``: every batch is padded (``DeviceGraphStore.batch(pad_to=...)``) to
    ``batch_size + 1`` crystals, to the next multiple of `node_quantum` nodes that holds its atoms and one per padding
    crystal, and to the next multiple of `edge_quantum` edges, so that an epoch has a few batch shapes only
    (``matten_amd.graphs.BucketedTrainStep``).  The crystals and their order do not change.  Off by default."""

    def __init__(self, store, batch_size: int = 1, shuffle: bool = False, seed: int = 0, training: bool = True,
                 pad=None, pad_species=None, pad_length: float = 2.0, **ignored):
        self.store, self.batch_size, self.shuffle, self.training = store, int(batch_size), bool(shuffle), bool(training)
        self._gen = torch.Generator().manual_seed(seed)
        self.pad = None
        if pad is not None:
            self.pad = tuple(int(q) for q in pad)
            if len(self.pad) != 2 or min(self.pad) < 1:
                raise ValueError(f"pad = {pad!r}: expected (node_quantum, edge_quantum), both at least 1")
        self.pad_species, self.pad_length = pad_species, pad_length

    def __len__(self) -> int:
        return -(-len(self.store) // self.batch_size)

    def batch_indices(self) -> List[List[int]]:
        """the crystal ids of every batch of the NEXT epoch (draws that epoch's permutation, like one pass of iteration)"""
        n = len(self.store)
        order = torch.randperm(n, generator=self._gen).tolist() if self.shuffle else list(range(n))
        return [order[lo:lo + self.batch_size] for lo in range(0, n, self.batch_size)]

    def padded_sizes(self, idx) -> tuple:
        """(N_b, E_b, B_b) of the batch `idx` under ``pad``: B_b = batch_size + 1, N_b the next multiple of the node quantum
        from N + (B_b - B) (the atoms and one node per padding crystal), E_b the next multiple of the edge quantum from E"""
        host = getattr(self.store, "host", self.store)
        _, n, e = host.plan(idx)
        qn, qe = self.pad
        b_b = self.batch_size + 1
        need = n + (b_b - len(idx))
        return qn * -(-need // qn), qe * -(-e // qe), b_b

    def __iter__(self) -> Iterator[Dict[str, torch.Tensor]]:
        for idx in self.batch_indices():
            if self.pad is None:
                yield self.store.batch(idx, training=self.training)
            else:
                yield self.store.batch(idx, training=self.training, pad_to=self.padded_sizes(idx),
                                       pad_species=self.pad_species, pad_length=self.pad_length)


class TensorDataModule:
    def __init__(
        self,
        trainset_filename: str,
        valset_filename: str,
        testset_filename: str,
        *,
        r_cut: float,
        tensor_target_name: str,
        tensor_target_format: str = "irreps",
        tensor_target_formula: str = "ijkl=jikl=klij",
        tensor_target_scale: float = 1.0,
        normalize_tensor_target: bool = False,
        root: str = ".",
        reuse: bool = True,
        loader_kwargs: Optional[Dict[str, Any]] = None,
        device=None,
        pbc=None,
        device_resident: bool = False,
        atom_selector: Optional[str] = None,
        atom_target_layout: Optional[str] = None,
        pad_eval: bool = False,
        **unsupported,
    ):
        bad = {k: v for k, v in unsupported.items() if v not in (None, False, [], {})
               and k in ("global_featurizer", "atom_featurizer", "scalar_target_names", "tensor_target_weight")}
        if bad:
            raise NotImplementedError(f"TensorDataModule options outside the accelerated path: {sorted(bad)}")
        # per-atom targets: "compact" = the reference's layout, "dense" = one row per atom + an int32 selector
        self.atom_selector = atom_selector or None
        if atom_target_layout is None:
            atom_target_layout = "dense" if device_resident else "compact"
        if atom_target_layout not in ("compact", "dense"):
            raise ValueError(f'atom_target_layout = {atom_target_layout!r}: "compact" or "dense"')
        if self.atom_selector is not None and device_resident and atom_target_layout == "compact":
            raise ValueError('atom_target_layout="compact" with device_resident=True: the compact target holds M <= N rows '
                             'per crystal and a bool selector, and the device store gathers per-atom, per-edge and '
                             'per-crystal keys of 4- or 8-byte elements only; use "dense" (the default there)')
        self.atom_target_layout = atom_target_layout
        if normalize_tensor_target:
            raise NotImplementedError("normalize_tensor_target: standardise with matten_amd.data.transform.TensorTargetTransform")
        self.files = {"train": trainset_filename, "val": valset_filename, "test": testset_filename}
        self.root, self.r_cut = root, float(r_cut)
        self.tensor_target_name, self.tensor_target_format = tensor_target_name, tensor_target_format
        self.tensor_target_formula, self.tensor_target_scale = tensor_target_formula, float(tensor_target_scale)
        self.loader_kwargs = dict(loader_kwargs or {})
        self.device = device
        self.pbc = pbc   # a bool or one per axis, applied to every structure; None: each record's own (Molecule: open)
        # device_resident: the sets are uploaded once in setup() (one DeviceGraphStore per distinct file) and the loaders
        # gather their batches on the device; the batches are those of the default loaders, plus their CSR keys
        self.device_resident = bool(device_resident)
        if self.device_resident and device is None:
            raise ValueError("device_resident=True needs `device`: the store lives on one GPU")
        if self.loader_kwargs.get("pad") is not None and not self.device_resident:
            raise ValueError("loader_kwargs['pad'] pads batches in the device loader's gather: it needs device_resident=True "
                             "(the host loader does not pad)")
        # pad_eval: the validation and test loaders pad like the training loader (a few bucket shapes: their steps replay
        # captured graphs, Trainer(graphed=True)); the model then needs loss_over_valid_rows, which that Trainer sets
        self.pad_eval = bool(pad_eval)
        if self.pad_eval:
            missing = [what for what, ok in (("device_resident=True", self.device_resident),
                                             ("loader_kwargs['pad']", self.loader_kwargs.get("pad") is not None)) if not ok]
            if missing:
                raise ValueError(f"pad_eval=True pads the validation and test batches in the device loader's gather: it needs "
                                 f"{' and '.join(missing)}")
        self._data: Dict[str, List[Dict[str, torch.Tensor]]] = {}
        self._stores: Dict[str, Any] = {}

    # Lightning's DataModule protocol
    def prepare_data(self):
        pass

    def _load(self, filename: str) -> List[Dict[str, torch.Tensor]]:
        path = filename if os.path.isabs(filename) else os.path.join(self.root, filename)
        bool_columns = (self.atom_selector,) if self.atom_selector is not None else ()
        rows = structures_from_json(path, target_columns=(self.tensor_target_name,), bool_columns=bool_columns)
        converter = CartesianTensorWrapper(self.tensor_target_formula)
        graphs = []
        for i, r in enumerate(rows):
            y = {}
            if self.atom_selector is not None:
                y = self._atom_targets(r, i, filename, converter)
            elif self.tensor_target_name in r:
                t = torch.as_tensor(r[self.tensor_target_name], dtype=torch.float64) * self.tensor_target_scale
                if self.tensor_target_format == "irreps":   # reference dataset/structure_scalar_tensor.py:262-267
                    t = converter.from_cartesian(t)
                y[self.tensor_target_name] = t.to(torch.float32).unsqueeze(0)
            pbc = self.pbc if self.pbc is not None else r.get("pbc", "lattice" in r)
            graphs.append(crystal_graph(r["cart_coords"], r.get("lattice"), r["atomic_numbers"], self.r_cut, y=y, pbc=pbc))
        return graphs

    def _atom_targets(self, r, i: int, filename: str, converter) -> Dict[str, torch.Tensor]:
        """the labels of one crystal with per-atom targets (reference dataset/structure_scalar_tensor.py:256-312): the
        tensors of the flagged atoms, scaled and converted like a crystal's, and the selector.  The tensors are taken as
        they are -- NMR shielding tensors are not symmetric; ``from_cartesian`` projects them, like the reference."""
        n = int(r["atomic_numbers"].shape[0])
        where = f"row {i} of {filename}"
        if self.atom_selector not in r or self.tensor_target_name not in r:
            raise ValueError(f"{where}: per-atom targets need the columns '{self.atom_selector}' and "
                             f"'{self.tensor_target_name}'")
        sel = torch.as_tensor(r[self.atom_selector])
        if sel.shape[0] != n:
            raise ValueError(f"{where}: '{self.atom_selector}' holds {sel.shape[0]} flags, the structure has {n} atoms")
        t = torch.as_tensor(r[self.tensor_target_name], dtype=torch.float64)
        m = int(sel.sum())
        if t.dim() < 1 or t.shape[0] != m or (m and t.numel() == 0):
            raise ValueError(f"{where}: '{self.tensor_target_name}' holds {t.shape[0] if t.dim() else 0} tensors, "
                             f"'{self.atom_selector}' flags {m} atoms")
        t = t * self.tensor_target_scale
        if self.tensor_target_format == "irreps":
            t = converter.from_cartesian(t)
        t = t.to(torch.float32)
        if self.atom_target_layout == "compact":
            return {self.tensor_target_name: t, "atom_selector": sel}
        dense = torch.zeros((n,) + tuple(t.shape[1:]), dtype=torch.float32)
        dense[sel] = t
        return {self.tensor_target_name: dense, "atom_selector": sel.to(torch.int32)}

    def setup(self, stage: Optional[str] = None):
        cache: Dict[str, List] = {}
        for mode, fn in self.files.items():
            if fn not in cache:
                cache[fn] = self._load(fn)
            self._data[mode] = cache[fn]
        if self.device_resident:
            from ..data.store import DeviceGraphStore

            stores: Dict[str, Any] = {}
            for mode, fn in self.files.items():
                if fn not in stores:
                    stores[fn] = DeviceGraphStore.from_graphs(cache[fn], self.device)
                self._stores[mode] = stores[fn]

    @property
    def train_data(self):
        return self._data["train"]

    def train_dataloader(self):
        if self.device_resident:
            return _DeviceLoader(self._stores["train"], training=True, **self.loader_kwargs)
        return _Loader(self._data["train"], device=self.device, **self.loader_kwargs)

    def _eval_kwargs(self) -> Dict[str, Any]:
        """validation and test batches are unshuffled, and unpadded (`pad` serves the captured training step) unless
        ``pad_eval`` keeps `pad`, `pad_species` and `pad_length` for them"""
        kw = dict(self.loader_kwargs, shuffle=False)
        if not self.pad_eval:
            for k in ("pad", "pad_species", "pad_length"):
                kw.pop(k, None)
        return kw

    def val_dataloader(self):
        if self.device_resident:
            return _DeviceLoader(self._stores["val"], training=False, **self._eval_kwargs())
        return _Loader(self._data["val"], device=self.device, **dict(self.loader_kwargs, shuffle=False))

    def test_dataloader(self):
        if self.device_resident:
            return _DeviceLoader(self._stores["test"], training=False, **self._eval_kwargs())
        return _Loader(self._data["test"], device=self.device, **dict(self.loader_kwargs, shuffle=False))

    # reference dataset/structure_scalar_tensor.py:640-666
    def get_to_model_info(self) -> Dict[str, Any]:
        z = set()
        num_neigh = []
        for g in self._data["train"]:
            z.update(g["atomic_numbers"].tolist())
            num_neigh.append(g["num_neigh"])
        return {
            "allowed_species": tuple(sorted(z)),
            "average_num_neighbors": torch.mean(torch.cat(num_neigh)).item(),
            "global_feats_size": None,
            "atom_feats_size": None,
        }
