"""Host half of the device-resident training set (matten_amd/data/store.py), the device loader's index sequence, the data
module's option and the argument checks of matten_batch_gather: everything that needs no GPU."""
import numpy as np
import pytest
import torch

from store_cases import data_module, golden_graphs, index_lists, store_graphs


@pytest.fixture(scope="module")
def host():
    from matten.data.store import GraphStoreHost

    return GraphStoreHost(store_graphs())


def _plan_restated(graphs, idx):
    """the record table from the graphs themselves: per picked crystal the first node / edge of the batch and of the set"""
    n_atoms = np.array([g["pos"].shape[0] for g in graphs], dtype=np.int64)
    n_edges = np.array([g["edge_index"].shape[1] for g in graphs], dtype=np.int64)
    table = np.zeros((5, len(idx) + 1), dtype=np.int64)
    dn = de = 0
    for b, i in enumerate(idx):
        table[:, b] = (dn, de, n_atoms[:i].sum(), n_edges[:i].sum(), i)
        dn, de = dn + n_atoms[i], de + n_edges[i]
    table[:2, -1] = (dn, de)
    return table, int(dn), int(de)


def test_running_sums(host):
    graphs = store_graphs()
    assert len(host) == 103
    assert host.node_ptr.tolist() == np.cumsum([0] + [g["pos"].shape[0] for g in graphs]).tolist()
    assert host.edge_ptr.tolist() == np.cumsum([0] + [g["edge_index"].shape[1] for g in graphs]).tolist()
    assert host.node_ptr[100] == 473 and host.edge_ptr[100] == 14380   # the golden set
    # the flat edge_index keeps crystal-relative ids
    for i in (0, 57, 101):
        e0, e1 = host.edge_ptr[i], host.edge_ptr[i + 1]
        assert torch.equal(host.flat["edge_index"][:, e0:e1], graphs[i]["edge_index"])


@pytest.mark.parametrize("name", list(index_lists()) + ["single id"])
def test_plan(host, name):
    idx = [41] if name == "single id" else index_lists()[name]
    table, n_out, e_out = host.plan(idx)
    want, n_want, e_want = _plan_restated(store_graphs(), idx)
    assert table.dtype == np.int32 and table.shape == (5, len(idx) + 1)
    assert np.array_equal(table.astype(np.int64), want) and (n_out, e_out) == (n_want, e_want)


def test_plan_errors(host):
    with pytest.raises(ValueError):
        host.plan([])
    for bad in ([103], [0, -1], [5, 1000, 2]):
        with pytest.raises(IndexError):
            host.plan(bad)


def _with(graphs, key, make):
    return [dict(g, **{key: make(g)}) for g in graphs]


def test_key_classes():
    from matten.data.store import CRYSTAL, EDGE, NODE, GraphStoreHost

    base = list(store_graphs()[95:])   # 5 golden + the three special graphs (one of them has ONE atom)
    n = lambda g: g["pos"].shape[0]
    e = lambda g: g["edge_index"].shape[1]
    graphs = _with(base, "per_node", lambda g: torch.zeros(n(g), 9))
    graphs = _with(graphs, "per_edge", lambda g: torch.zeros(e(g), dtype=torch.int64))
    graphs = _with(graphs, "per_crystal", lambda g: torch.zeros(1, 2, 3, dtype=torch.float64))
    h = GraphStoreHost(graphs)
    assert h.classes["per_node"] == NODE and h.classes["per_edge"] == EDGE and h.classes["per_crystal"] == CRYSTAL
    assert h.classes["elastic_tensor_full"] == CRYSTAL and h.classes["pos"] == NODE and h.classes["cell"] == CRYSTAL
    assert h.flat["per_node"].shape == (h.node_ptr[-1], 9) and h.flat["per_crystal"].shape == (8, 2, 3)
    # one-atom crystals only: per node and per crystal coincide, either class gathers the same rows
    ones = _with([store_graphs()[100]] * 2, "k", lambda g: torch.zeros(1, 4))
    assert GraphStoreHost(ones).classes["k"] in (NODE, CRYSTAL)

    # a key of the wrong length: the key and the first offending graph are named
    bad = _with(base, "odd", lambda g: torch.zeros(n(g), 2))
    bad[3] = dict(bad[3], odd=torch.zeros(n(bad[3]) + 1, 2))
    with pytest.raises(ValueError, match=r"'odd' of graph 3\b"):
        GraphStoreHost(bad)
    # elements below 4 bytes
    for dtype in (torch.uint8, torch.bool, torch.float16):
        with pytest.raises(ValueError, match="'flag'"):
            GraphStoreHost(_with(base, "flag", lambda g: torch.zeros(n(g), dtype=dtype)))
    # trailing shapes must agree, keys must agree
    ragged = _with(base, "r", lambda g: torch.zeros(1, n(g)))
    with pytest.raises(ValueError, match="'r'"):
        GraphStoreHost(ragged)
    missing = [dict(g) for g in base]
    del missing[2]["elastic_tensor_full"]
    with pytest.raises(ValueError, match="graph 2"):
        GraphStoreHost(missing)
    with pytest.raises(ValueError):
        GraphStoreHost([])


def test_device_loader_visits_what_the_host_loader_visits():
    """shuffle=True, seed=3, batch_size=32 over the 100 golden graphs, two epochs: the same crystals in the same order as
    _Loader (recovered from the batches' targets, which are distinct), the last batch of 4 included"""
    from matten.data.store import GraphStoreHost
    from matten.dataset.structure_scalar_tensor import _DeviceLoader, _Loader

    graphs = list(golden_graphs())
    targets = torch.cat([g["elastic_tensor_full"] for g in graphs])
    assert len(torch.unique(targets, dim=0)) == 100
    ref = _Loader(graphs, batch_size=32, shuffle=True, seed=3)
    dev = _DeviceLoader(GraphStoreHost(graphs), batch_size=32, shuffle=True, seed=3)
    assert len(dev) == len(ref) == 4
    epochs = []
    for _ in range(2):
        idx = dev.batch_indices()
        assert [len(i) for i in idx] == [32, 32, 32, 4]
        batches = list(ref)
        assert len(batches) == len(idx)
        for b, i in zip(batches, idx):
            assert torch.equal(b["elastic_tensor_full"], targets[i])
        epochs.append(idx)
    assert epochs[0] != epochs[1] and sorted(sum(epochs[0], [])) == list(range(100))
    plain = _DeviceLoader(GraphStoreHost(graphs), batch_size=32)
    assert plain.batch_indices() == [list(range(lo, min(lo + 32, 100))) for lo in range(0, 100, 32)]


def test_device_resident_needs_a_device():
    with pytest.raises(ValueError, match="device"):
        data_module(device_resident=True)
    dm = data_module()   # default off
    assert dm.device_resident is False


def test_batch_gather_argument_errors():
    """MATTEN_EINVAL for everything the host can see, before any launch"""
    from matten_amd import _lib
    from matten_amd.data import store

    lib = _lib.load()
    assert _lib.ABI_VERSION == 47 and lib.matten_abi_version() == 47
    assert lib.matten_batch_gather_max_streams() == 32 and lib.matten_batch_gather_lds_rows() >= 2
    buf = np.zeros(64, dtype=np.int64)   # stands in for device memory: never dereferenced before the checks fail
    p = buf.ctypes.data

    def call(streams, n_streams=None, table=p, b=1, n=1, e=1):
        d = np.asarray(streams, dtype=np.int64).reshape(-1, store.STREAM_WORDS)
        n_streams = len(d) if n_streams is None else n_streams
        return lib.matten_batch_gather(d.ctypes.data if d.size else None, n_streams, table, b, n, e, None)

    ok = (p, p, 4, 3, store.NODE, store.OP_RAW)
    assert call([ok], b=-1) == -1 and call([ok], n=-1) == -1 and call([ok], e=-1) == -1 and call([ok], n_streams=-1) == -1
    assert call([ok], n=2 ** 31) == -1 and call([ok], e=2 ** 31) == -1
    assert call([ok], table=None) == -1
    assert call([], n_streams=1) == -1                                        # no stream array
    assert call([ok] * 33) == -1                                              # more than the kernel's argument block holds
    for elem in (1, 2, 3, 16, 0, -4):
        assert call([(p, p, elem, 3, store.NODE, store.OP_RAW)]) == -1, elem
    assert call([(0, p, 4, 3, store.NODE, store.OP_RAW)]) == -1               # no source
    assert call([(p, 0, 4, 3, store.NODE, store.OP_RAW)]) == -1               # no destination
    assert call([(0, 0, 8, 1, store.NODE, store.OP_BATCH64)]) == -1           # a fill needs its destination too
    assert call([(p, p, 4, 0, store.NODE, store.OP_RAW)]) == -1               # empty rows
    assert call([(p, p, 4, 3, 3, store.OP_RAW)]) == -1 and call([(p, p, 4, 3, -1, store.OP_RAW)]) == -1
    assert call([(p, p, 4, 3, store.NODE, 7)]) == -1 and call([(p, p, 4, 3, store.NODE, -1)]) == -1
    assert call([(p, p, 8, 1, store.EDGE, store.OP_ADD32_NODE)]) == -1        # int32 operation on 8-byte elements
    assert call([(p, p, 4, 1, store.EDGE, store.OP_ADD64_NODE)]) == -1
    assert call([(p, p, 4, 2, store.EDGE, store.OP_ADD32_EDGE)]) == -1        # the offset forms take one element per row
    assert call([(p, p, 4, 1, store.EDGE, store.OP_ROWPTR32)]) == -1          # row pointers are per node
    assert call([(p, p, 8, 1, store.NODE, store.OP_PTR64)]) == -1             # ptr is per crystal
    assert call([(p + 4, p, 8, 1, store.NODE, store.OP_RAW)]) == -1           # a pointer off its element size
    assert call([ok, (p, p, 2, 3, store.NODE, store.OP_RAW)]) == -1           # any stream of several
