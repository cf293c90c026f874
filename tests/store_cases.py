"""Graphs shared by tests/test_store_host.py and tests/test_gpu_store.py: the 100 golden crystals plus three special ones."""
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
