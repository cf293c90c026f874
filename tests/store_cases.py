"""Graphs shared by tests/test_store_host.py and tests/test_gpu_store.py: the 100 golden crystals plus three special ones;
the stream records both gather entries refuse."""
import functools
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N100 = "example_crystal_elasticity_tensor_n100.json"
TARGET = "elastic_tensor_full"
R_CUT = 5.0

ONE_ATOM, CLUSTER, MOLECULE = 100, 101, 102   # positions of the special graphs


def data_module(root=GOLDEN, **kw):
    from matten.dataset.structure_scalar_tensor import TensorDataModule

    return TensorDataModule(trainset_filename=N100, valset_filename=N100, testset_filename=N100, root=root, r_cut=R_CUT,
                            tensor_target_name=TARGET, tensor_target_scale=1e-2, **kw)


@functools.lru_cache(maxsize=None)
def golden_graphs():
    """the 100 golden crystals as the data module loads them (473 atoms, 14 380 edges), target [1,21] included"""
    dm = data_module()
    dm.setup()
    return tuple(dm.train_data)


@functools.lru_cache(maxsize=None)
def store_graphs():
    """golden graphs + a one-atom periodic fcc primitive cell (every edge a self-loop to an image) + fcc_cluster(300)
    (open; more atoms than a workgroup has threads) + one molecule; all with the golden graphs' keys"""
    from matten_amd.data import synthetic
    from matten_amd.data.graph import crystal_graph

    rng = np.random.default_rng(7)

    def target():
        return {TARGET: torch.as_tensor(rng.normal(size=(1, 21)), dtype=torch.float32)}

    a = 4.05
    prim = 0.5 * a * np.array([[0.0, 1, 1], [1, 0, 1], [1, 1, 0]])
    one = crystal_graph(np.zeros((1, 3)), prim, np.array([13]), R_CUT, y=target())
    c = synthetic.fcc_cluster(300)
    cluster = crystal_graph(c["cart_coords"], None, c["atomic_numbers"], R_CUT, y=target(), pbc=False)
    m = synthetic.molecules(3)[1]
    molecule = crystal_graph(m["cart_coords"], None, m["atomic_numbers"], R_CUT, y=target(), pbc=False)
    graphs = list(golden_graphs()) + [one, cluster, molecule]
    assert len(graphs) == 103 and list(one.keys()) == list(graphs[0].keys())
    assert one["pos"].shape[0] == 1 and bool((one["edge_index"] == 0).all()) and cluster["pos"].shape[0] == 300
    return tuple(graphs)


def index_lists():
    """name -> crystal ids of a batch"""
    g = torch.Generator().manual_seed(11)
    return {
        "single tiny": [ONE_ATOM],
        "cluster alone": [CLUSTER],
        "cluster between tiny": [ONE_ATOM, CLUSTER, MOLECULE],
        "shuffled 32": torch.randperm(103, generator=g)[:32].tolist(),
        "all reversed": list(range(102, -1, -1)),
        "repeated": [7, 7, 7],
    }


@functools.lru_cache(maxsize=None)
def many_key_graphs():
    """store_graphs()[88:] (15 crystals) with 18 extra keys, six per class: 4- and 8-byte elements, rows of 1, 2, 4 and 9
    elements (4, 8, 16, 36 and 72 bytes: the 4-, 8- and 16-byte copies).  With them a training batch has more streams
    than one launch of the gather takes."""
    rng = torch.Generator().manual_seed(9)
    kinds = ((1, torch.float32), (2, torch.int32), (4, torch.float32), (9, torch.float64), (1, torch.int64), (9, torch.float32))
    graphs = []
    for g in store_graphs()[88:]:
        lead = {"node": g["pos"].shape[0], "edge": g["edge_index"].shape[1], "crystal": 1}
        extra = {}
        for cls, rows in lead.items():
            for j, (width, dtype) in enumerate(kinds):
                shape = (rows,) if width == 1 else (rows, width)
                if dtype.is_floating_point:
                    extra[f"{cls}_extra{j}"] = torch.randn(shape, generator=rng, dtype=dtype)
                else:
                    extra[f"{cls}_extra{j}"] = torch.randint(1, 2 ** 30, shape, generator=rng, dtype=dtype)
        graphs.append(dict(g, **extra))
    assert len(graphs) == 15 and len(graphs[0]) == len(store_graphs()[0]) + 18
    return tuple(graphs)


def streams_needed(host, training=True):
    """streams of one batch of a store: one per key, edge_index two, batch and ptr, the CSR keys (three, six in training)"""
    return len(host.keys) + 1 + 2 + (6 if training else 3)


def refused_streams(p):
    """lists of six-word stream records that a gather entry must refuse, each for one reason; `p` is an address that
    stands in for device memory (never dereferenced before the checks fail)"""
    from matten_amd.data.store import EDGE, NODE, OP_ADD32_EDGE, OP_ADD32_NODE, OP_ADD64_NODE, OP_BATCH64, OP_PTR64, OP_RAW, OP_ROWPTR32

    ok = (p, p, 4, 3, NODE, OP_RAW)
    bad = [[(p, p, elem, 3, NODE, OP_RAW)] for elem in (1, 2, 3, 16, 0, -4)]       # element sizes
    bad += [
        [(0, p, 4, 3, NODE, OP_RAW)],                                             # no source
        [(p, 0, 4, 3, NODE, OP_RAW)],                                             # no destination
        [(0, 0, 8, 1, NODE, OP_BATCH64)],                                         # a fill needs its destination too
        [(p, p, 4, 0, NODE, OP_RAW)],                                             # empty rows
        [(p, p, 4, 3, 3, OP_RAW)], [(p, p, 4, 3, -1, OP_RAW)],                    # class
        [(p, p, 4, 3, NODE, 7)], [(p, p, 4, 3, NODE, -1)],                        # operation
        [(p, p, 8, 1, EDGE, OP_ADD32_NODE)], [(p, p, 4, 1, EDGE, OP_ADD64_NODE)],  # an operation off its element size
        [(p, p, 4, 2, EDGE, OP_ADD32_EDGE)],                                      # the offset forms take one element per row
        [(p, p, 4, 1, EDGE, OP_ROWPTR32)],                                        # row pointers are per node
        [(p, p, 8, 1, NODE, OP_PTR64)],                                           # ptr is per crystal
        [(p + 4, p, 8, 1, NODE, OP_RAW)],                                         # a pointer off its element size
        [ok, (p, p, 2, 3, NODE, OP_RAW)],                                         # any stream of several
        [ok] * 33,                                                                # more than the kernel's argument block holds
    ]
    return bad
