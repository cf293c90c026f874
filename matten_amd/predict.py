"""
``predict`` / ``evaluate``: the reference's public inference API (predict.py:117-245) on MI355X.

Same signature and semantics: one structure or a list in, one tensor or a list out in input order,
``None`` (plus a warning) for structures whose graph cannot be built, ``RuntimeError`` for species the
model was not trained on.  Differences, all forced by the environment: structures are duck-typed
(``.lattice.matrix`` / ``.cart_coords`` / ``.atomic_numbers``, or dicts with keys ``lattice`` /
``cart_coords`` / ``atomic_numbers``) so pymatgen is optional -- when it is importable and
``is_elasticity_tensor`` is set the result is wrapped in ``ElasticTensor`` exactly like the reference,
otherwise a ``numpy [3,3,3,3]`` array is returned -- and the checkpoint is a plain ``torch.save`` of
{"state_dict", "hyper_parameters"} or a Lightning ``.ckpt`` with the same two keys.

Boundary conditions: a dict may carry ``"pbc"`` (a bool or one per axis); a dict without ``"lattice"`` or an object
without ``.lattice`` (a pymatgen ``Molecule``: ``.cart_coords`` / ``.atomic_numbers``) is an open structure; an object
with ``.lattice`` is fully periodic whatever ``lattice.pbc`` says, which is what the reference's ``from_pymatgen`` does.
``predict(..., pbc=...)`` overrides every structure.
"""
import warnings
from pathlib import Path
from typing import Any, Dict, List, Sequence, Union

import numpy as np
import torch

from .data.graph import (SINGULAR_CELL, EdgelessStructures, SingularCells, batch_graphs_gpu, collate, crystal_graph,
                         image_reach, image_reach_pbc, normalize_pbc, periodic_volume)
from .model_factory.tfn_atomic_tensor import AtomicTensorModel
from .model_factory.tfn_scalar_tensor import ScalarTensorModel
from .parallel import sharded_apply
from .utils import CartesianTensorWrapper, yaml_load


def get_pretrained_model_dir(identifier: str) -> Path:
    p = Path(identifier)
    if p.exists() and p.is_dir():
        return p
    return Path(__file__).parent.parent / "pretrained" / identifier


def get_pretrained_config(identifier: str, config_filename: str = "config_final.yaml"):
    return yaml_load(get_pretrained_model_dir(identifier) / config_filename)


def get_pretrained_model(identifier: str, checkpoint: str = "model_final.ckpt", model_class=ScalarTensorModel,
                         device="cuda"):
    path = get_pretrained_model_dir(identifier) / checkpoint
    if not path.exists():
        raise FileNotFoundError(
            f"{path} not found. (The reference's own pretrained/20230627/model_final.ckpt is a large blob that is "
            "not shipped with the source tree; pass a directory holding model_final.ckpt + config_final.yaml.)"
        )
    from .checkpoint import filter_state_dict, load_checkpoint, plain, rebuild_tasks

    # restricted unpickler: the file's matten / e3nn / Lightning objects become inert placeholders (checkpoint.py)
    ckpt = load_checkpoint(path)
    hp = ckpt["hyper_parameters"]
    tasks = rebuild_tasks(hp.get("tasks"), path.parent)
    model = model_class(
        tasks=tasks, backbone_hparams=plain(hp["backbone_hparams"]), dataset_hparams=plain(hp["dataset_hparams"]),
        optimizer_hparams=plain(hp.get("optimizer_hparams")), lr_scheduler_hparams=plain(hp.get("lr_scheduler_hparams")),
    )
    # e3nn-internal buffers (output_mask, empty weight / bias placeholders, fx-graph Wigner-3j constants) and
    # Lightning metric state are dropped; anything else that does not match is an error
    state, missing, bad = filter_state_dict(ckpt["state_dict"], list(model.state_dict().keys()))
    if missing or bad:
        raise RuntimeError(f"checkpoint does not match the model: missing={missing} unexpected={bad}")
    model.load_state_dict(state, strict=True)
    return model.to(device).eval()


_OPEN, _PERIODIC = (False, False, False), (True, True, True)


def _raw_fields(s, pbc=None):
    """-> (cart_coords, lattice or None, atomic_numbers, pbc as three bools) of a dict or a pymatgen-like object (module
    docstring); ``pbc`` overrides the structure's own flags"""
    if isinstance(s, dict):
        lattice = s.get("lattice")
        own = s["pbc"] if "pbc" in s else (lattice is not None)
        p, z = s["cart_coords"], s["atomic_numbers"]
    else:
        lattice = getattr(s, "lattice", None)
        own = lattice is not None
        if lattice is not None:
            lattice = lattice.matrix
        p, z = s.cart_coords, s.atomic_numbers
    return p, lattice, z, normalize_pbc(own if pbc is None else pbc)


def _fields(s, pbc=None) -> Dict[str, np.ndarray]:
    p, lattice, z, flags = _raw_fields(s, pbc)
    return {"lattice": np.zeros((3, 3)) if lattice is None else np.asarray(lattice), "cart_coords": np.asarray(p),
            "atomic_numbers": np.asarray(z), "pbc": flags}


def check_species(model, structures: Sequence, Z=None, ptr=None, index=None):
    """Raise like the reference (predict.py:96-114) if a structure holds a species the model was not trained on.
    With the packed arrays of ``pack_structures`` the common all-supported case is one vectorised membership test."""
    supported = set(int(z) for z in model.hparams["dataset_hparams"]["allowed_species"])
    if Z is not None:
        bad = ~np.isin(Z, np.fromiter(supported, dtype=np.int64))
        if not bad.any():
            return
        k = int(np.searchsorted(ptr, np.nonzero(bad)[0][0], side="right") - 1)
        structures, first = [structures[index[k]]], index[k]
    else:
        first = 0
    for i, s in enumerate(structures, start=first):
        numbers = set(int(z) for z in _fields(s)["atomic_numbers"])
        if not numbers.issubset(supported):
            not_supported = ", ".join(str(z) for z in sorted(numbers - supported))
            raise RuntimeError(
                f"Cannot make predictions for structure {i}. It contains species {not_supported} not supported by "
                f"the model. The model were trained with species {supported}."
            )


def _pack_fast(structures: Sequence):
    """pack_structures for the common case -- every structure a dict whose three fields already are well-formed numpy arrays
    ([n, 3] float64 coordinates, [3, 3] float64 lattice, [n] integer species, n > 0, everything finite, cell not singular,
    every axis periodic: no "pbc" key) --
    without a per-structure Python body: three list comprehensions, three concatenations and vectorised checks (0.4 instead
    of 2.1 ms per 1000 fcc-64 structures).  Anything else -> None, and the per-structure path decides and warns."""
    try:
        ps = [s["cart_coords"] for s in structures]
        cs = [s["lattice"] for s in structures]     # (an open structure without a lattice leaves through the KeyError)
        zs = [s["atomic_numbers"] for s in structures]
        if any("pbc" in s for s in structures):
            return None
        if not ps or not all(type(p) is np.ndarray and p.ndim == 2 for p in ps):
            return None
        pos, cell, Z = np.concatenate(ps), np.concatenate(cs), np.concatenate(zs)
        sizes = np.fromiter(map(len, zs), dtype=np.int64, count=len(zs))
        n = len(ps)
        if (pos.dtype != np.float64 or cell.dtype != np.float64 or Z.dtype.kind not in "iu" or pos.ndim != 2 or pos.shape[1] != 3
                or cell.shape != (3 * n, 3) or Z.ndim != 1 or len(Z) != len(pos) or sizes.min() <= 0):
            return None
        if not np.array_equal(np.fromiter(map(len, ps), dtype=np.int64, count=n), sizes):
            return None
        cell = cell.reshape(n, 3, 3)
        if not (np.isfinite(pos).all() and np.isfinite(cell).all() and (np.abs(np.linalg.det(cell)) > 1e-12).all()):
            return None
        ptr = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(sizes, out=ptr[1:])
        return pos, cell, Z.astype(np.int64, copy=False), ptr, list(range(n)), []
    except Exception:  # noqa: BLE001  (objects instead of dicts, ragged arrays, ...: the careful path handles and reports them)
        return None


def pack_structures(structures: Sequence, first: int = 0, with_pbc: bool = False, pbc=None):
    """One pass over the structures -> flat struct-of-arrays batch (pos [N,3] f64, cell [B,3,3] f64, Z [N] i64,
    ptr [B+1]) of the usable ones, plus the indices that cannot be used (same role as the per-structure try/except of
    the reference dataset, dataset/structure_scalar_tensor.py:296-362): malformed arrays, no atoms, non-finite
    numbers, linearly dependent (or zero) lattice vectors on the periodic axes.  Everything after the attribute access
    is vectorised.

    Open and partly periodic structures (module docstring) are kept, with zeros for a missing lattice.  The result
    stays the 6-tuple (pos, cell, Z, ptr, keep, failed); ``with_pbc=True`` appends the flags of the kept structures,
    [B,3] bools or None when every axis of every one is periodic -- what ``batch_graphs_gpu_soa(pbc=)`` takes.
    ``pbc`` (a bool or three) overrides the structures' own flags."""
    override = None if pbc is None else normalize_pbc(pbc)
    fast = _pack_fast(structures) if override in (None, _PERIODIC) else None
    if fast is not None:
        return fast + (None,) if with_pbc else fast
    pos_l, cell_l, z_l, pbc_l, keep, failed = [], [], [], [], [], []
    asarray, f64, i64 = np.asarray, np.float64, np.int64
    zero_cell = np.zeros((3, 3))
    for i, s in enumerate(structures):
        try:
            p, c, z, flags = _raw_fields(s, override)
            p, c, z = asarray(p, dtype=f64), zero_cell if c is None else asarray(c, dtype=f64), asarray(z, dtype=i64)
            if p.ndim != 2 or p.shape[1] != 3:
                p = p.reshape(-1, 3)
            if c.shape != (3, 3):
                c = c.reshape(3, 3)
            if z.ndim != 1:
                z = z.reshape(-1)
            if len(p) == 0 or len(p) != len(z):
                raise ValueError("malformed structure")
        except Exception as e:  # noqa: BLE001
            warnings.warn(f"Failed converting structure {first + i}, Skip it. {e}")
            failed.append(i)
            continue
        pos_l.append(p); cell_l.append(c); z_l.append(z); pbc_l.append(flags); keep.append(i)
    if not keep:
        raise RuntimeError("Cannot successfully convert any structures.")

    def flat(pos_l, cell_l, z_l):
        sizes = np.fromiter(map(len, z_l), dtype=np.int64, count=len(z_l))
        ptr = np.zeros(len(z_l) + 1, dtype=np.int64)
        np.cumsum(sizes, out=ptr[1:])
        return np.concatenate(pos_l), np.stack(cell_l), np.concatenate(z_l), ptr

    pos, cell, Z, ptr = flat(pos_l, cell_l, z_l)
    flags = np.array(pbc_l, dtype=bool).reshape(-1, 3)
    with np.errstate(all="ignore"):
        # periodic vectors linearly independent (three periodic axes: |det| > 1e-12, the test of every earlier version)
        ok = np.isfinite(cell).all(axis=(1, 2)) & (periodic_volume(cell, flags) > SINGULAR_CELL)
        ok &= np.logical_and.reduceat(np.isfinite(pos).all(axis=1), ptr[:-1])
    if not ok.all():
        for k in np.nonzero(~ok)[0]:
            warnings.warn(f"Failed converting structure {first + keep[k]}, Skip it. singular cell or non-finite coordinates")
            failed.append(keep[k])
        sel = np.nonzero(ok)[0]
        if len(sel) == 0:
            raise RuntimeError("Cannot successfully convert any structures.")
        keep = [keep[k] for k in sel]
        pos, cell, Z, ptr = flat([pos_l[k] for k in sel], [cell_l[k] for k in sel], [z_l[k] for k in sel])
        flags = flags[sel]
    out = (pos, cell, Z, ptr, keep, sorted(failed))
    return out + (None if flags.all() else flags,) if with_pbc else out


_SIDE_STREAMS: Dict[Any, Any] = {}

# atoms one forward may hold when evaluate_soa coalesces user batches (MATTEN_PREDICT_NODE_BUDGET; ~30 KB of device buffers
# per atom at 30 neighbours: 2 GB at the default)
NODE_BUDGET = int(__import__("os").environ.get("MATTEN_PREDICT_NODE_BUDGET", "65536"))


REFERENCE_BATCH_SIZE = 200   # predict.py:155 of the reference


def effective_node_budget(batch_size: int, node_budget: int = None) -> int:
    """atoms a merged forward may hold: the caller's `node_budget` when given; otherwise NODE_BUDGET -- unless the caller
    LOWERED batch_size below the reference's default, which is how one makes a forward fit a small or shared GPU there:
    such batches are run as they are (0 = no merging)"""
    if node_budget is not None:
        return max(0, int(node_budget))
    return NODE_BUDGET if batch_size >= REFERENCE_BATCH_SIZE else 0


def coalesce_batches(ptr, batch_size: int, node_budget: int = None):
    """Crystal index ranges of the forwards evaluate_soa runs.  ``batch_size`` is the reference's knob for how many
    structures share a forward (predict.py:155, default 200); a crystal's prediction does not depend on its batch mates
    (tests: bitwise within a kernel path, ~1e-7 across the row-resident / streaming lin2 switch), so here it only bounds
    memory: consecutive user batches are merged while the atoms of the merged batch stay within ``node_budget``.  The
    reference's data set averages 4.7 atoms per crystal -- 200 of them are ~1000 atoms, a forward that is all launch
    latency (~45 launches), while 65536 atoms fill the GPU.  A single user batch larger than the budget is kept as it is."""
    node_budget = NODE_BUDGET if node_budget is None else node_budget
    B = len(ptr) - 1
    chunks, lo = [], 0
    while lo < B:
        hi = min(B, lo + batch_size)
        while hi < B and ptr[min(B, hi + batch_size)] - ptr[lo] <= node_budget:
            hi = min(B, hi + batch_size)
        chunks.append(np.arange(lo, hi))
        lo = hi
    return chunks


def _side_stream(device):
    """one persistent graph-construction stream per device (a fresh stream per call would also mean a fresh, empty
    allocator pool per call)"""
    key = torch.device(device)
    if key not in _SIDE_STREAMS:
        _SIDE_STREAMS[key] = torch.cuda.Stream(key)
    return _SIDE_STREAMS[key]


_CONVERTERS: Dict[str, CartesianTensorWrapper] = {}


def _converter(formula: str) -> CartesianTensorWrapper:
    """one converter per formula: its change-of-basis matrix stays on the device between calls (a fresh one uploads it
    behind the forward: a blocking 7 KB copy the host sits in for the whole forward)"""
    if formula not in _CONVERTERS:
        _CONVERTERS[formula] = CartesianTensorWrapper(formula)
    return _CONVERTERS[formula]


class _deferred_input_checks:
    """the per-forward range checks are read one batch late (and all of them before the results leave): the host keeps
    building the next batch instead of waiting for the flags of the one it has just enqueued"""

    def __init__(self, model):
        self.model = model

    def __enter__(self):
        self.modes = [(m, m.check_species) for m in self.model.modules() if hasattr(m, "check_species")]
        if hasattr(self.model, "set_input_checks"):
            self.model.set_input_checks("deferred")
        return self

    def __exit__(self, *exc):
        for m, mode in self.modes:
            m._pending = None
            m.check_species = mode
        return False


def evaluate_soa(model, pos, cell, Z, ptr, r_cut: float, batch_size: int = 200,
                 tensor_target_name: str = "elastic_tensor_full", tensor_target_formula: str = "ijkl=jikl=klij",
                 node_budget: int = None, *, pbc=None):
    """Batched forward straight from the flat arrays of ``pack_structures`` (``pbc``: the [B,3] flags its
    ``with_pbc=True`` appends; None: every axis periodic).  Graphs are built on the device batch
    by batch on a SECOND stream: the neighbour search of batch k+1 (and its one host sync, the edge count) overlaps
    the forward of batch k, which runs on the caller's stream.
    -> (Cartesian tensors [B, 3, ...] on the host as one array, indices of the crystals no graph could be built of: no
    edge inside the cutoff, or linearly dependent periodic vectors; their rows are NaN)."""
    model.eval()
    with _deferred_input_checks(model):
        return _soa_end(model, _soa_begin(model, pos, cell, Z, ptr, r_cut, batch_size, tensor_target_name,
                                          tensor_target_formula, node_budget, pbc))


def _soa_begin(model, pos, cell, Z, ptr, r_cut, batch_size, tensor_target_name, tensor_target_formula, node_budget=None,
               pbc=None):
    """enqueue every forward of the packed structures (inside _deferred_input_checks) -> (device tensors [B, 3, ...],
    indices of crystals without any edge); nothing here waits for the forwards"""
    from .data.graph import batch_graphs_gpu_soa

    converter = _converter(tensor_target_formula)
    device = model.device
    rank_dims = (3,) * len(tensor_target_formula.split("=")[0].replace("-", ""))
    B = len(ptr) - 1
    out = torch.full((B,) + rank_dims, float("nan"), device=device)
    edgeless = []
    main = torch.cuda.current_stream(device)
    side = _side_stream(device)

    def slice_of(ids):
        a, b = ptr[ids[0]], ptr[ids[-1] + 1]
        if np.all(np.diff(ids) == 1):
            return pos[a:b], cell[ids], Z[a:b], ptr[ids[0] : ids[-1] + 2] - a
        rows = np.concatenate([np.arange(ptr[i], ptr[i + 1]) for i in ids])  # crystals were dropped: regather
        sp = np.zeros(len(ids) + 1, dtype=np.int64)
        np.cumsum(ptr[ids + 1] - ptr[ids], out=sp[1:])
        return pos[rows], cell[ids], Z[rows], sp

    def build(ids):
        """graph batch of crystals `ids` on the side stream; crystals without edges are dropped and recorded"""
        with torch.cuda.stream(side):
            while len(ids):
                try:
                    return ids, batch_graphs_gpu_soa(*slice_of(ids), r_cut, device, pbc=None if pbc is None else pbc[ids])
                except (EdgelessStructures, SingularCells) as e:
                    # (SingularCells: a cell at the packer's threshold that the device's own arithmetic puts below it, or
                    # arrays that did not come from pack_structures: no graph either, reported the same way)
                    edgeless.extend(int(ids[k]) for k in e.indices)
                    ids = np.delete(ids, e.indices)
        return ids, None

    budget = effective_node_budget(batch_size, node_budget)
    try:
        _evaluate_soa_loop(model, coalesce_batches(ptr, batch_size, budget), build, main, side, out, edgeless, converter,
                           tensor_target_name, device)
    except torch.cuda.OutOfMemoryError:
        if budget == 0:
            raise
        # a merged forward did not fit (a shared or small GPU): start over with the caller's own batches
        torch.cuda.synchronize(device)
        torch.cuda.empty_cache()
        warnings.warn(f"a merged forward of up to {budget} atoms ran out of device memory: running batches of {batch_size} "
                      "structures unmerged (pass node_budget= to predict() to set the limit)")
        out.fill_(float("nan"))
        del edgeless[:]
        _evaluate_soa_loop(model, coalesce_batches(ptr, batch_size, 0), build, main, side, out, edgeless, converter,
                           tensor_target_name, device)
    return out, edgeless


def _soa_end(model, handle):
    out, edgeless = handle
    if hasattr(model, "finish_input_checks"):
        model.finish_input_checks()
    return out.cpu().numpy(), sorted(edgeless)


def _evaluate_soa_loop(model, chunks, build, main, side, out, edgeless, converter, tensor_target_name, device):
    with torch.no_grad():
        nxt = build(chunks[0]) if chunks else None
        for k in range(len(chunks)):
            ids, batch = nxt
            if batch is not None:
                main.wait_stream(side)
                for t in batch.values():
                    t.record_stream(main)  # allocated on the side stream, consumed on the caller's
                preds, _ = model(batch, task_name=tensor_target_name)
                p = preds[tensor_target_name]
                if p.dim() == 2:  # irreps -> Cartesian on the GPU
                    p = converter.to_cartesian(p)
                if len(ids) and ids[-1] - ids[0] + 1 == len(ids):
                    out[int(ids[0]) : int(ids[-1]) + 1] = p     # a plain range: no index upload (a blocking copy
                else:                                            # queued behind the forward would stall the host here)
                    out[torch.as_tensor(ids, device=device)] = p
            nxt = build(chunks[k + 1]) if k + 1 < len(chunks) else None  # overlaps the forward just enqueued


def build_graphs(structures: Sequence, r_cut: float, on_gpu: bool = False, pbc=None):
    """-> (graphs, failed indices): per-structure try/except like the reference dataset
    (dataset/structure_scalar_tensor.py:296-362).

    ``on_gpu``: only validate on the host and return (pos, cell, Z) triples -- (pos, cell, Z, pbc) for a structure
    with an open axis; the neighbour search then runs on the device, batch by batch, inside ``evaluate`` (crystals
    that turn out to have no edge come back as NaN rows and are reported as failed by ``predict``).
    ``pbc`` overrides the structures' own boundary conditions (module docstring)."""
    graphs, failed = [], []
    for i, s in enumerate(structures):
        try:
            f = _fields(s, pbc)
            if on_gpu:
                pos = np.asarray(f["cart_coords"], dtype=np.float64).reshape(-1, 3)
                cell = np.asarray(f["lattice"], dtype=np.float64).reshape(3, 3)
                Z = np.asarray(f["atomic_numbers"], dtype=np.int64).reshape(-1)
                if len(pos) == 0 or len(pos) != len(Z) or not np.all(np.isfinite(image_reach_pbc(pos, cell, r_cut, f["pbc"]))):
                    raise ValueError("malformed structure")
                if not all(f["pbc"]) and not (np.all(np.isfinite(pos)) and np.all(np.isfinite(cell))):
                    raise ValueError("malformed structure")   # (an open axis has no reach that would go non-finite)
                graphs.append((pos, cell, Z) if all(f["pbc"]) else (pos, cell, Z, f["pbc"]))
                continue
            graphs.append(crystal_graph(f["cart_coords"], f["lattice"], f["atomic_numbers"], r_cut, pbc=f["pbc"]))
        except Exception as e:  # noqa: BLE001
            warnings.warn(f"Failed converting structure {i}, Skip it. {e}")
            failed.append(i)
    if not graphs:
        raise RuntimeError("Cannot successfully convert any structures.")
    return graphs, failed


def evaluate(model, graphs: List, batch_size: int = 200,
             tensor_target_name: str = "elastic_tensor_full", tensor_target_formula: str = "ijkl=jikl=klij",
             distributed: bool = False, r_cut: float = None) -> List[torch.Tensor]:
    """Batched forward; returns one Cartesian tensor per graph (on the host).  With ``distributed`` the
    graphs are sharded by index over the ranks and gathered with one collective per call.

    ``graphs`` holds either host graph dicts (``crystal_graph``) or raw (pos, cell, Z) triples; triples are
    turned into a batch on the device (``batch_graphs_gpu``, needs ``r_cut``).  A triple without any edge
    yields a NaN tensor."""
    converter = _converter(tensor_target_formula)
    device = model.device
    rank_dims = (3,) * len(tensor_target_formula.split("=")[0].replace("-", ""))
    # what the model emits per crystal: the irreps row ([21] for the elasticity tensor) or, for
    # output_format == "cartesian", the tensor itself.  The rows are what crosses xGMI (north star: ONE gather of
    # [B, 21]); the change of basis to [3,3,3,3] (81 floats) runs after the gather, on every rank's full set.
    cartesian_out = getattr(model, "to_cartesian", None) is not None
    row_dims = rank_dims if cartesian_out else (converter._Q.shape[0],)

    def run(shard):
        outs = []
        with torch.no_grad():
            for lo in range(0, len(shard), batch_size):
                items = shard[lo : lo + batch_size]
                keep = list(range(len(items)))
                if isinstance(items[0], dict):
                    batch = collate(items, device=device)
                else:
                    try:
                        batch = batch_graphs_gpu(items, r_cut, device)
                    except EdgelessStructures as e:
                        keep = [i for i in keep if i not in set(e.indices)]
                        batch = batch_graphs_gpu([items[i] for i in keep], r_cut, device) if keep else None
                full = torch.full((len(items),) + row_dims, float("nan"), device=device)
                if batch is not None:
                    preds, _ = model(batch, task_name=tensor_target_name)
                    p = preds[tensor_target_name]
                    if len(keep) == len(items):
                        full = p.reshape((len(items),) + row_dims)
                    else:
                        full[torch.as_tensor(keep, device=device)] = p.reshape((len(keep),) + row_dims)
                outs.append(full)
        return torch.cat(outs, dim=0)

    model.eval()
    if distributed:
        rows = sharded_apply(run, graphs, row_dims, device)
    else:
        rows = run(graphs)
    preds = rows if cartesian_out else converter.to_cartesian(rows)   # NaN rows stay NaN tensors
    return list(preds.cpu())


def evaluate_atomic(model, graphs: List, batch_size: int = 200, tensor_target_name: str = "nmr_tensor",
                    tensor_target_formula: str = "ij=ji", r_cut: float = None, sink: list = None) -> List[torch.Tensor]:
    """Per-atom tensors of all atoms of all structures, in input order, as ONE flat list -- what the reference's
    ``evaluate`` produces for an ``AtomicTensorModel`` (predict.py:117-148: ``predictions.extend(p)``).
    ``sink`` (a list): receives each forward's device tensor [n, 3, ...] for a consumer that works on the device."""
    converter = _converter(tensor_target_formula)
    device = model.device
    outs = []
    model.eval()
    with torch.no_grad():
        for lo in range(0, len(graphs), batch_size):
            items = graphs[lo : lo + batch_size]
            batch = collate(items, device=device) if isinstance(items[0], dict) else batch_graphs_gpu(items, r_cut, device)
            preds, _ = model(batch, task_name=tensor_target_name)
            p = preds[tensor_target_name]
            if p.dim() == 2:
                p = converter.to_cartesian(p)
            outs.append(p)
            if sink is not None:
                sink.append(p)
    return list(torch.cat(outs, dim=0).cpu())


def equivariance_report(model, structures, rotations=None, n_random: int = 2, seed: int = 0, r_cut: float = None,
                        formula: str = "ijkl=jikl=klij", is_atomic_tensor: bool = False) -> Dict[str, Any]:
    """Is this model, on this build, still equivariant?  Every structure is predicted as given and with positions and cell
    rotated (r' = M r) by every rotation; the unrotated prediction is rotated on the device in the irreps basis
    (``symmetry.rotate_irreps``; per-atom tensors by their structure's rotation through the ``index`` path) and compared
    with the prediction of the rotated structure -- the reference's own check (tests/model/test_tfn_tensor.py:98-139)
    without the trip to the host and the rank-4 einsum.

    ``rotations`` [G,3,3] (orthogonal, proper or improper); by default ``n_random`` seeded random proper rotations plus
    one improper one (the negative of a further random rotation).  ``r_cut`` defaults to the model's radial cutoff
    (``radial_basis_end``).  The forwards are those of ``evaluate`` / ``evaluate_atomic`` (``collate`` of host graphs, eval
    mode, no grad); one read-back at the end.
    -> {"rotations" [G,3,3], "max_abs" [S,G] = max|D y(x) - y(M x)|, "max_rel" [S,G] = that over max|y(x)|, both in the
    irreps basis, "worst_abs", "worst_rel", "worst" = (structure, rotation) of worst_rel}."""
    from .symmetry import irreps_of, rotate_irreps

    structures = list(structures) if isinstance(structures, (list, tuple)) else [structures]
    if not structures:
        raise ValueError("equivariance_report: no structure")
    if rotations is None:
        rng = np.random.default_rng(seed)
        mats = []
        for k in range(n_random + 1):
            q, r = np.linalg.qr(rng.standard_normal((3, 3)))
            q = q * np.sign(np.diag(r))
            q = q if np.linalg.det(q) > 0 else -q
            mats.append(-q if k == n_random else q)
        rotations = np.stack(mats)
    rotations = np.asarray(rotations, dtype=np.float64).reshape(-1, 3, 3)
    G, S = len(rotations), len(structures)
    if r_cut is None:
        r_cut = float(model.hparams["backbone_hparams"]["radial_basis_end"])
    check_species(model, structures)
    device = model.device
    name = list(model.tasks.keys())[0]
    converter = _converter(formula)
    dim = irreps_of(formula).dim
    cartesian_out = getattr(model, "to_cartesian", None) is not None

    def graph(s, M):
        f = _fields(s)
        return crystal_graph(f["cart_coords"] @ M.T, f["lattice"] @ M.T, f["atomic_numbers"], r_cut, pbc=f["pbc"])

    def rows(graphs):
        batch = collate(graphs, device=device)
        preds, _ = model(batch, task_name=name)
        p = preds[name]
        if cartesian_out:
            p = converter.from_cartesian(p)
        return p.reshape(-1, dim), batch["batch"]

    model.eval()
    R = torch.as_tensor(rotations, device=device)
    max_abs = torch.empty(S, G, dtype=torch.float64, device=device)
    scale = torch.empty(S, dtype=torch.float64, device=device)
    with torch.no_grad():
        for i, s in enumerate(structures):
            # ONE forward per structure: graph 0 of the batch is the structure as given, graph 1 + g its copy under rotation g
            # (eval mode: a prediction does not depend on its batch)
            y_all, owner = rows([graph(s, np.eye(3))] + [graph(s, M) for M in rotations])
            n = y_all.shape[0] // (G + 1)                                 # rows per copy: atoms, or 1
            y, y_rot = y_all[:n], y_all[n:]
            # row r of y_rot belongs to rotation g: the per-atom path maps atoms to rotations, the crystal path is one row each
            index = owner[n:] - 1 if is_atomic_tensor else None
            want = rotate_irreps(y.repeat(G, 1), formula, R, index=index)
            diff = (want - y_rot).abs().double().reshape(G, -1).amax(dim=1)
            max_abs[i].copy_(diff)
            scale[i] = y.abs().double().amax()
    max_abs, scale = max_abs.cpu().numpy(), scale.cpu().numpy()      # the one read-back
    with np.errstate(invalid="ignore", divide="ignore"):
        max_rel = max_abs / scale[:, None]
    worst = np.unravel_index(int(np.nanargmax(max_rel)), max_rel.shape) if np.isfinite(max_rel).any() else (0, 0)
    return {"rotations": rotations, "max_abs": max_abs, "max_rel": max_rel, "worst_abs": float(np.nanmax(max_abs)),
            "worst_rel": float(np.nanmax(max_rel)), "worst": (int(worst[0]), int(worst[1]))}


def symmetry_report(model, structures, symprec: float = 1e-3, r_cut: float = None, formula: str = "ijkl=jikl=klij",
                    is_atomic_tensor: bool = False, batch_size: int = 200) -> Dict[str, Any]:
    """Does this model's prediction have the symmetry of its crystal?  Every structure is predicted (the forwards of
    ``evaluate`` / ``evaluate_atomic``: ``collate`` of host graphs, eval mode, no grad), its symmetry is found on the device
    (``symmetry.find_symmetry`` at ``symprec``) and the prediction is compared with its symmetrised self in the irreps basis:
    a crystal-level tensor with the average over the point group (``CrystalSymmetry.average_crystal_rows``), per-atom
    tensors with ``symmetry.symmetrize_atoms`` (the worst atom of each structure).  One read-back at the end.
    -> {"order" [S], "n_trans" [S], "flags" [S] (symmetry.SYM_*), "deviation" [S] = |y - P y| / |y|, "worst" = the largest
    deviation, "worst_structure", "predictions" (the device rows in the irreps basis), "symmetry" (the CrystalSymmetry)}."""
    from .symmetry import find_symmetry, irreps_of, symmetrize_atoms

    structures = list(structures) if isinstance(structures, (list, tuple)) else [structures]
    if not structures:
        raise ValueError("symmetry_report: no structure")
    if r_cut is None:
        r_cut = float(model.hparams["backbone_hparams"]["radial_basis_end"])
    check_species(model, structures)
    device = model.device
    name = list(model.tasks.keys())[0]
    converter = _converter(formula)
    dim = irreps_of(formula).dim
    cartesian_out = getattr(model, "to_cartesian", None) is not None
    fields = [_fields(s) for s in structures]
    sym = find_symmetry([dict(f) for f in fields], symprec=symprec, device=device)
    graphs = [crystal_graph(f["cart_coords"], f["lattice"], f["atomic_numbers"], r_cut, pbc=f["pbc"]) for f in fields]
    model.eval()
    rows = []
    with torch.no_grad():
        for lo in range(0, len(graphs), batch_size):
            preds, _ = model(collate(graphs[lo:lo + batch_size], device=device), task_name=name)
            p = preds[name]
            if cartesian_out:
                p = converter.from_cartesian(p)
            rows.append(p.reshape(-1, dim))
        y = torch.cat(rows).contiguous()
        if is_atomic_tensor:
            _, per_atom = symmetrize_atoms(y, formula, sym)
            deviation = torch.zeros(len(structures), dtype=torch.float64, device=device)
            deviation = deviation.scatter_reduce(0, sym.row_struct.long(), per_atom, "amax", include_self=False)
        else:
            deviation = sym.average_crystal_rows(y, formula)[1]
        table = torch.stack([sym.n_rot.double(), sym.n_trans.double(), sym.flags.double(), deviation]).cpu().numpy()   # the read-back
    dev = table[3]
    worst = int(np.nanargmax(dev)) if np.isfinite(dev).any() else 0
    return {"order": table[0].astype(np.int64), "n_trans": table[1].astype(np.int64), "flags": table[2].astype(np.int64),
            "deviation": dev, "worst": float(dev[worst]), "worst_structure": worst, "predictions": y, "symmetry": sym}


PREDICT_SLAB = int(__import__("os").environ.get("MATTEN_PREDICT_SLAB", "1024"))   # structures packed per slab
# (a small first slab with 4x growth -- device started after 0.3 ms of packing -- was measured in round 5 and dropped: every
# forward costs the host ~1 ms (graph-build read-back + ~45 launches), so three forwards instead of one gave back what the
# earlier start gained on 1000 fcc-64 structures, 8.1 ms either way, and small structures lost: 3.4 -> 5.3 ms per 1000; with the
# vectorised packer a HALF first slab for large cells only was measured again: 6.3-6.4 vs 6.3-6.6 ms per 1000 fcc-64
# structures, 5.1-5.3 either way at 4000 -- inside the run-to-run spread, not kept)


def _predict_slabs(model, structures, r_cut, batch_size, tensor_target_name, tensor_target_formula, node_budget=None,
                   pbc=None, device_rows=None):
    """-> (predictions of the usable structures in input order, sorted indices of the failed ones)
    ``device_rows`` (a list): receives one (structure indices, device tensors [len, 3, ...]) pair per slab -- the forwards'
    own output buffers, NaN rows for crystals without a graph -- for a consumer that works on the device"""
    n = len(structures)
    budget = effective_node_budget(batch_size, node_budget)

    def pack(lo, hi):
        try:
            pos, cell, Z, ptr, keep, failed, flags = pack_structures(structures[lo:hi], first=lo, with_pbc=True, pbc=pbc)
        except RuntimeError:                       # not one usable structure in this slab (each one was warned about)
            return None, list(range(lo, hi))
        keep = [lo + k for k in keep]
        check_species(model, structures, Z, ptr, keep)   # (raises like the reference, naming the structure's own index)
        return (pos, cell, Z, ptr, keep, flags), [lo + k for k in failed]

    failed, inflight = [], []
    model.eval()
    with _deferred_input_checks(model):
        lo, size = 0, PREDICT_SLAB
        nxt = pack(0, min(n, size)) if n else None
        while nxt is not None:
            cur, bad = nxt
            failed += bad
            lo = min(n, lo + size)
            if cur is not None:
                pos, cell, Z, ptr, keep, flags = cur
                inflight.append((keep, _soa_begin(model, pos, cell, Z, ptr, r_cut, batch_size, tensor_target_name,
                                                  tensor_target_formula, node_budget, flags)))
                # a slab should fill a forward: ~NODE_BUDGET atoms (1024 fcc-64 crystals, ~14 000 of the reference's
                # 4.7-atom ones), between PREDICT_SLAB and 16 PREDICT_SLAB structures
                per = max(1.0, len(pos) / max(1, len(keep)))
                size = int(min(16 * PREDICT_SLAB, max(PREDICT_SLAB, max(NODE_BUDGET, budget) / per)))
            nxt = pack(lo, min(n, lo + size)) if lo < n else None   # overlaps the forwards just enqueued
        predictions = []
        for keep, handle in inflight:
            tensors, edgeless = _soa_end(model, handle)
            if device_rows is not None:
                device_rows.append((keep, handle[0]))
            for j in edgeless:
                warnings.warn(f"Failed converting structure {keep[j]}, Skip it. After eliminating self edges, no edges "
                              "remain in this system (or its periodic lattice vectors are linearly dependent).")
            dropped = set(edgeless)
            failed += [keep[j] for j in edgeless]
            predictions += [tensors[j] for j in range(len(keep)) if j not in dropped]
    return predictions, sorted(set(failed))


def _structure_densities(structures) -> np.ndarray:
    """``density="structure"``: kg/m^3 per structure, from a ``.density`` attribute (pymatgen: g/cm^3) or a dict's
    ``"density"`` key (kg/m^3); ValueError listing the structures that carry none"""
    out, missing = np.zeros(len(structures)), []
    for i, s in enumerate(structures):
        if isinstance(s, dict):
            rho = s.get("density")
        else:
            rho = getattr(s, "density", None)
            rho = None if rho is None else 1000.0 * float(rho)
        if rho is None:
            missing.append(i)
        else:
            out[i] = float(rho)
    if missing:
        raise ValueError(f'density="structure": no density on structures {missing} (a `.density` attribute in g/cm^3 or a '
                         'dict key "density" in kg/m^3)')
    return out


def _properties_of_slabs(device_rows, n, failed, directions, single, angles=None, density=None, number_density=None,
                         modulus_unit=1e9, refine=False, refine_tol=1e-9, refine_max_iter=32, kelvin=False,
                         polycrystal=False, hs_grid=64, sc_tol=1e-12, sc_max_iter=200):
    """ElasticProperties of all n input structures from the slabs' device tensors: they never come back from the host.
    Structures without a prediction (``failed``) keep NaN rows and get flag bit 2."""
    from .elastic import _from_rows

    first = device_rows[0][1]
    rows = torch.full((n, 81), float("nan"), dtype=first.dtype, device=first.device)
    for keep, t in device_rows:
        if keep and keep[-1] - keep[0] + 1 == len(keep):
            rows[keep[0] : keep[-1] + 1] = t.reshape(len(keep), 81)
        elif keep:
            rows[torch.as_tensor(keep, device=first.device)] = t.reshape(len(keep), 81)
    mask = np.zeros(n, dtype=bool)
    mask[list(failed)] = True
    return _from_rows(rows, 0, directions, False, single, mask, angles, density, number_density, modulus_unit, refine,
                      refine_tol, refine_max_iter, kelvin, polycrystal, hs_grid, sc_tol, sc_max_iter)


def predict(
    structure,
    model_identifier="20230627",
    checkpoint: str = "model_final.ckpt",
    batch_size: int = 200,
    logger_level: str = "ERROR",
    is_elasticity_tensor: bool = True,
    is_atomic_tensor: bool = False,
    model: ScalarTensorModel = None,
    config: Dict[str, Any] = None,
    node_budget: int = None,
    pbc=None,
    properties: bool = False,
    directions=None,
    angles=None,
    density=None,
    number_density=None,
    modulus_unit: float = 1e9,
    refine: bool = False,
    refine_tol: float = 1e-9,
    refine_max_iter: int = 32,
    kelvin: bool = False,
    polycrystal: bool = False,
    hs_grid: int = 64,
    sc_tol: float = 1e-12,
    sc_max_iter: int = 200,
    waves: bool = False,
    deg_tol: float = 1e-6,
    shielding: bool = False,
):
    """See the module docstring.  ``model`` / ``config`` let a caller reuse an already loaded model.
    ``properties=True`` (elasticity tensors only: ``ValueError`` with ``is_atomic_tensor``) returns ``(tensors, props)``:
    the usual return value and an ``elastic.ElasticProperties`` with one row per input structure (bulk and shear moduli,
    Young's modulus, compliance, ...; with ``directions`` -- an int or an array [D,3] -- also the directional extremes),
    computed from the forwards' device buffers.  Rows of failed structures are NaN and carry flag bit 2.
    ``angles`` (an int M), ``density`` (kg/m^3, one value per input structure, or ``"structure"``: read from each structure's
    ``.density`` in g/cm^3 or a dict's ``"density"`` key in kg/m^3), ``number_density`` (atoms/m^3) and ``modulus_unit`` are
    those of ``elastic.elastic_properties`` (shear modulus and Poisson's ratio over direction pairs, sound velocities, Debye
    temperature); they need ``properties=True`` and are checked before any forward runs.  So are ``refine``, ``refine_tol``
    and ``refine_max_iter``: the directional extremes polished off the grid (the ``*_refined*`` fields; needs ``directions``).
    ``kelvin=True`` (needs ``properties=True``) adds the Kelvin decomposition of ``elastic.elastic_properties(kelvin=True)``:
    ``kelvin_moduli``, ``kelvin_vectors``, ``kelvin_dilatation``, ``stability_margin``, ``kelvin_condition``.
    ``polycrystal=True`` (needs ``properties=True``; with ``hs_grid``, ``sc_tol``, ``sc_max_iter``) adds the polycrystal moduli of
    ``elastic.elastic_properties(polycrystal=True)``: the Hashin-Shtrikman bounds ``k_hs_lower`` / ``g_hs_lower`` / ``k_hs_upper``
    / ``g_hs_upper`` with ``hs_media``, the self-consistent ``k_sc`` / ``g_sc`` / ``y_sc`` / ``poisson_sc``, ``sc_status`` and
    ``sc_iterations``.
    ``waves=True`` (needs ``properties=True``, ``directions`` and ``density``; with ``deg_tol``) returns ``(tensors, props, waves)``,
    ``waves`` a ``waves.AcousticWaves`` with one row per input structure: polarisations, group velocities, power-flow angles
    and phonon-focusing Jacobians per direction and branch, from the Voigt matrices ``props`` holds on the device.  Tensors
    and ``props`` are what they are without it.
    ``batch_size`` (reference predict.py:155) is the memory knob it is there: consecutive batches are merged into one forward
    only while the merged batch stays within ``node_budget`` atoms (default MATTEN_PREDICT_NODE_BUDGET = 65536, ~2 GB) and
    only when batch_size is at least the reference's default of 200; ``node_budget=0`` never merges.  A merged forward
    that runs out of device memory is retried unmerged.
    ``shielding=True`` (per-atom tensors only: needs ``is_atomic_tensor`` and a symmetric rank-2 target formula, ``ValueError``
    before any forward otherwise) returns ``(tensors, props)``: the usual flat list and a ``rank2.Rank2Properties`` over all
    atoms in the order of that list (principal values and axes, isotropic value, span, skew, Haeberlen anisotropy and
    asymmetry), computed from the forwards' device buffers, with ``ptr`` [S+1]: the atoms of structure s are rows
    ptr[s]:ptr[s+1]."""
    from .log import set_logger

    set_logger(logger_level)  # reference predict.py:194
    if is_atomic_tensor:  # reference predict.py:196-199
        is_elasticity_tensor = False
    if properties and is_atomic_tensor:
        raise ValueError("properties=True derives elastic moduli from a rank-4 elasticity tensor per structure; "
                         "per-atom tensors (is_atomic_tensor=True) have none")
    if not properties:
        for name, value in (("angles", angles), ("density", density), ("number_density", number_density)):
            if value is not None:
                raise ValueError(f"{name} belongs to the derived properties: pass properties=True")
        if refine:
            raise ValueError("refine belongs to the derived properties: pass properties=True")
        if kelvin:
            raise ValueError("kelvin belongs to the derived properties: pass properties=True")
        if polycrystal:
            raise ValueError("polycrystal belongs to the derived properties: pass properties=True")
        if waves:
            raise ValueError("waves belongs to the derived properties: pass properties=True")
    if shielding:
        from .rank2 import rank2_basis

        if not is_atomic_tensor:
            raise ValueError("shielding=True derives the shielding parameters of per-atom rank-2 tensors: pass "
                             "is_atomic_tensor=True")
        if config is None:
            config = get_pretrained_config(model_identifier)
        rank2_basis(config["data"]["tensor_target_formula"])      # (ValueError unless a symmetric rank 2)
    single = not isinstance(structure, (list, tuple))
    structures = [structure] if single else list(structure)
    if properties:
        from .elastic import _check_extras, _check_kelvin, _check_per_row, _check_polycrystal, _check_refine

        _check_kelvin(kelvin)
        _check_polycrystal(polycrystal, hs_grid, sc_tol, sc_max_iter)
        _check_extras(directions, angles, density, number_density)
        _check_refine(refine, directions, refine_tol, refine_max_iter)
        if not isinstance(waves, (bool, np.bool_)):
            raise ValueError(f"waves: expected True or False, got {waves!r}")
        if waves:
            from .waves import check_deg_tol

            if directions is None:
                raise ValueError("waves: the acoustic modes need a direction set, pass directions")
            if density is None:
                raise ValueError("waves: the velocities need the mass density, pass density")
            deg_tol = check_deg_tol(deg_tol)
        if isinstance(density, str):
            if density != "structure":
                raise ValueError(f'density: expected values in kg/m^3 or "structure", got {density!r}')
            density = _structure_densities(structures)
        if density is not None:
            density = _check_per_row("density", density, len(structures), single)
        if number_density is not None:
            number_density = _check_per_row("number_density", number_density, len(structures), single)

    if model is None:
        model = get_pretrained_model(model_identifier, checkpoint,
                                     model_class=AtomicTensorModel if is_atomic_tensor else ScalarTensorModel)
    if config is None:
        config = get_pretrained_config(model_identifier)
    r_cut = config["data"]["r_cut"]
    if is_atomic_tensor:
        check_species(model, structures)
        # one tensor per atom; the reference returns them as one flat list over all structures and never unwraps a
        # single structure (predict.py:210-242).  A structure whose graph cannot be built fails the whole call
        # here: with per-atom outputs the reference's "None at the failed index" bookkeeping has no meaning.
        graphs, failed = build_graphs(structures, r_cut=r_cut, on_gpu=True, pbc=pbc)
        if failed:
            raise RuntimeError(f"Cannot build the graph of structures {failed}.")
        sink = [] if shielding else None
        preds = evaluate_atomic(model, graphs, batch_size=batch_size,
                                tensor_target_name=config["data"]["tensor_target_name"],
                                tensor_target_formula=config["data"]["tensor_target_formula"], r_cut=r_cut, sink=sink)
        if shielding:      # (from the forwards' device buffers; the list above is their host copy)
            from .rank2 import rank2_properties

            counts = [int(g["pos"].shape[0]) if isinstance(g, dict) else len(g[0]) for g in graphs]
            ptr = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int64, device=sink[0].device)
            return [t.numpy() for t in preds], rank2_properties(torch.cat(sink, dim=0), ptr=ptr)
        return [t.numpy() for t in preds]
    # fast path: the structures are packed into flat arrays slab by slab (PREDICT_SLAB structures each); while the
    # device runs the forwards of slab k the host packs slab k + 1 (a 1000-structure slab packs in 2-3 ms, its forwards
    # take 4-5 ms: the host work of all slabs but the first disappears behind the device)
    device_rows = None
    if properties:
        from .elastic import check_directions

        if len(config["data"]["tensor_target_formula"].split("=")[0].replace("-", "")) != 4:
            raise ValueError(f"properties=True needs a rank-4 tensor target, not {config['data']['tensor_target_formula']!r}")
        if directions is not None:
            directions = check_directions(directions)      # (a bad direction set fails before any forward runs)
        device_rows = []
    predictions, failed = _predict_slabs(model, structures, r_cut, batch_size, config["data"]["tensor_target_name"],
                                         config["data"]["tensor_target_formula"], node_budget, pbc, device_rows)
    if not predictions:
        raise RuntimeError("Cannot successfully convert any structures.")
    if properties:
        props = _properties_of_slabs(device_rows, len(structures), failed, directions, single, angles, density,
                                     number_density, modulus_unit, refine, refine_tol, refine_max_iter, kelvin,
                                     polycrystal, hs_grid, sc_tol, sc_max_iter)
        if waves:      # (from the Voigt matrices and the direction set that props holds on the device)
            from .waves import waves_from_voigt

            wave_props = waves_from_voigt(props.voigt.reshape(-1, 6, 6), props.flags.reshape(-1), density, props.directions,
                                          modulus_unit, deg_tol, True, single)
    if is_elasticity_tensor:
        try:
            from pymatgen.analysis.elasticity import ElasticTensor

            predictions = [ElasticTensor(t) for t in predictions]
        except ImportError:
            pass

    if failed:
        failed_set, it = set(failed), iter(predictions)
        out = [None if i in failed_set else next(it) for i in range(len(structures))]
        warnings.warn(
            "Cannot make predictions for the following structures. Their returned "
            f"elasticity tensor set to `None`: {sorted(failed_set)}."
        )
    else:
        out = predictions
    out = out[0] if single else out
    if properties and waves:
        return out, props, wave_props
    return (out, props) if properties else out


def evaluate_frames(model, structure, pos_frames, cell_frames=None, r_cut: float = 5.0,
                    tensor_target_name: str = "elastic_tensor_full", tensor_target_formula: str = "ijkl=jikl=klij",
                    properties: bool = False, slack: float = 1.25, pbc=None):
    """The tensors of F geometries of ONE structure -- the frames of a trajectory, a strain or volume sweep -- with the
    edge list rebuilt on the device per frame and every frame one hipGraph replay (``data.rebuild.GeometryBatch``,
    ``graphs.GraphedGeometryStep``).

    ``structure`` gives the species and the boundary conditions (and the cell, when ``cell_frames`` is None: a fixed
    cell); ``pos_frames`` [F,N,3] and ``cell_frames`` [F,3,3] are arrays or tensors (fp64; the search runs in fp64).
    -> the F Cartesian tensors as a list on the host, like ``evaluate``; with ``properties=True`` ``(tensors, props)``,
    ``props`` = ``elastic.elastic_properties`` of the stacked tensors (F rows).

    The edge buffers are sized from frame 0 (64 * ceil(slack * E0 / 64) edges).  Per-frame flags are collected on the
    device and read back ONCE after the last frame: frames with more edges than that are run again after
    ``GeometryBatch.grow`` to 64 * ceil(1.25 * E / 64) for the largest such frame (E from an eager build of it); a frame
    without any edge or with a singular cell raises ``EdgelessStructures`` / ``SingularCells`` with the FRAME indices."""
    from .data.graph import batch_graphs_gpu_soa
    from .data.rebuild import FLAG_EDGELESS, FLAG_OVERFLOW, FLAG_SINGULAR, EdgeCapacityExceeded, GeometryBatch, edge_capacity_for
    from .graphs import GraphedGeometryStep

    model.eval()
    device = model.device
    p0, lattice, z, flags3 = _raw_fields(structure, pbc)
    Z = np.asarray(z, dtype=np.int64).reshape(-1)
    n = len(Z)
    as_dev = lambda a: (a.detach() if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a, dtype=np.float64))).to(
        device=device, dtype=torch.float64)
    pos_d = as_dev(pos_frames)
    if pos_d.dim() != 3 or tuple(pos_d.shape[1:]) != (n, 3) or pos_d.shape[0] < 1:
        raise ValueError(f"pos_frames is {tuple(pos_d.shape)}: expected [F, {n}, 3] for the {n} atoms of the structure")
    F = pos_d.shape[0]
    if cell_frames is None:
        if lattice is None and any(flags3):
            raise ValueError("the structure has no lattice: pass cell_frames, or pbc=False")
        cell_d = as_dev(np.zeros((3, 3)) if lattice is None else np.asarray(lattice, dtype=np.float64)).reshape(1, 3, 3)
    else:
        cell_d = as_dev(cell_frames)
        if tuple(cell_d.shape) != (F, 3, 3):
            raise ValueError(f"cell_frames is {tuple(cell_d.shape)}: expected [{F}, 3, 3]")
    check_species(model, [{"atomic_numbers": Z, "cart_coords": p0, "lattice": lattice}])
    ptr = np.array([0, n], dtype=np.int64)
    pbc_rows = None if all(flags3) else np.array([flags3], dtype=bool)
    cell_of = (lambda f: cell_d[0]) if cell_frames is None else (lambda f: cell_d[f])
    gb = GeometryBatch(pos_d[0].cpu().numpy(), cell_of(0).cpu().numpy(), Z, ptr, r_cut, device, pbc=pbc_rows, slack=slack)
    converter = _converter(tensor_target_formula)
    rows, frame_flags = None, torch.zeros(F, dtype=torch.int32, device=device)
    counts = torch.zeros(F, dtype=torch.int64, device=device)

    def run(frames):
        nonlocal rows
        step = GraphedGeometryStep(model, gb, task_name=tensor_target_name)
        for f in frames:
            out = step.step(pos=pos_d[f], cell=None if cell_frames is None else cell_d[f], flags_out=frame_flags[f:f + 1])
            counts[f:f + 1].copy_(gb.edge_count)
            if rows is None:
                rows = torch.full((F,) + tuple(out.shape[1:]), float("nan"), dtype=out.dtype, device=device)
            rows[f].copy_(out[0])
        return frame_flags.tolist()   # the one read-back of the pass

    host = run(range(F))
    for bit, exc in ((FLAG_SINGULAR, SingularCells), (FLAG_EDGELESS, EdgelessStructures)):
        bad = [f for f, w in enumerate(host) if w & bit]
        if bad:
            raise exc(bad)
    again = [f for f, w in enumerate(host) if w & FLAG_OVERFLOW]
    if again:
        worst = again[int(torch.argmax(counts[torch.as_tensor(again, device=device)]))]
        eager = batch_graphs_gpu_soa(pos_d[worst].cpu().numpy(), cell_of(worst).cpu().numpy(), Z, ptr, r_cut, device,
                                     pbc=pbc_rows)
        needed = int(eager["edge_index"].shape[1])
        gb.grow(edge_capacity_for(needed, 1.25))
        host = run(again)
        still = [f for f in again if host[f] & FLAG_OVERFLOW]
        if still:   # (the worst frame was measured: cannot happen unless the inputs changed under the call)
            raise EdgeCapacityExceeded(int(counts[still[0]]), gb.e_b)
    gb.flags.zero_()
    cartesian_out = getattr(model, "to_cartesian", None) is not None
    preds = rows if cartesian_out else converter.to_cartesian(rows)
    tensors = list(preds.cpu())
    if properties:
        from .elastic import elastic_properties

        return tensors, elastic_properties(preds)
    return tensors
