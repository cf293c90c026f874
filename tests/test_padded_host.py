"""Padded batches without a GPU: the table and the host restatement of a padded batch (GraphStoreHost.plan_padded /
padded_reference, matten_amd/data/store.py), the refusals, the quantum rule of the padded device loader, and the new
symbols of the library."""
import numpy as np
import pytest
import torch

from store_cases import golden_graphs, refused_streams

CSR_KEYS = ("_amd_perm", "_amd_rowptr", "_amd_src_sorted")
TRAIN_KEYS = ("_amd_dst_sorted", "_amd_out_ptr", "_amd_out_perm")


@pytest.fixture(scope="module")
def host():
    from matten.data.store import GraphStoreHost

    return GraphStoreHost(golden_graphs())


def _sizes(graphs, idx):
    return sum(graphs[i]["pos"].shape[0] for i in idx), sum(graphs[i]["edge_index"].shape[1] for i in idx)


def _rowptr(sorted_ids, n_nodes):
    return np.searchsorted(sorted_ids, np.arange(n_nodes + 1), side="left")


CASES = {
    # name: (crystal ids, lambda (N, E, B) -> pad_to)
    "16 crystals to (64, 1024)": (list(range(40, 56)), lambda n, e, b: (64 * -(-(n + 1) // 64), 1024 * -(-e // 1024), b + 1)),
    "no padding edges": ([3, 1, 4, 1, 5], lambda n, e, b: (n + 7, e, b + 1)),
    "one hub": ([9, 2, 6], lambda n, e, b: (n + 1, e + 300, b + 1)),
    "K = 3": ([5, 99, 0, 17], lambda n, e, b: (n + 10, e + 23, b + 3)),
    "more padding nodes than edges": ([8], lambda n, e, b: (n + 9, e + 4, b + 2)),
    "short last batch": ([70, 71, 72, 73], lambda n, e, b: (64, 2048, 33)),
}


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("training", [True, False])
def test_padded_reference(host, name, training):
    from matten_amd.data.graph import collate

    graphs = golden_graphs()
    idx, to = CASES[name]
    n, e = _sizes(graphs, idx)
    b = len(idx)
    n_b, e_b, b_b = pad_to = to(n, e, b)
    k = b_b - b
    p = n_b - n - (k - 1)
    pad_length = 1.75

    table, n_plan, e_plan = host.plan_padded(idx, pad_to)
    real, _, _ = host.plan(idx)
    assert (n_plan, e_plan) == (n, e) and table.dtype == np.int32 and table.shape == (5, b_b + 1)
    assert np.array_equal(table[:, :b], real[:, :b])
    assert table[:, -1].tolist() == [n_b, e_b, n, e, b]
    assert table[0, b:].tolist() == [n] + [n + p + i for i in range(k - 1)] + [n_b]
    assert table[1, b:].tolist() == [e] + [e_b] * k and not table[2:, b:b_b].any()

    got = host.padded_reference(idx, pad_to, pad_length=pad_length, training=training)
    want = collate([graphs[i] for i in idx])
    assert list(got.keys()) == list(want.keys()) + list(CSR_KEYS + (TRAIN_KEYS if training else ())) + ["_amd_n_valid"]
    # sizes are exactly pad_to, the real part is collate
    assert got["pos"].shape == (n_b, 3) and got["edge_index"].shape == (2, e_b) and got["cell"].shape == (3 * b_b, 3)
    assert got["batch"].shape == (n_b,) and got["ptr"].shape == (b_b + 1,) and got["elastic_tensor_full"].shape == (b_b, 21)
    for key, v in want.items():
        g = got[key]
        assert g.dtype == v.dtype, key
        if key == "edge_index":
            assert torch.equal(g[:, :e], v)
        elif key == "ptr":
            assert torch.equal(g[:b + 1], v)
        else:
            assert torch.equal(g[:v.shape[0]], v), key
    # the layout: crystal b owns P nodes, the others one; ptr / batch / n_valid follow
    sizes = [p] + [1] * (k - 1)
    assert got["ptr"][b:].tolist() == np.cumsum([n] + sizes).tolist()
    assert got["batch"][n:].tolist() == sum(([b + i] * s for i, s in enumerate(sizes)), [])
    assert got["_amd_n_valid"].dtype == torch.int64 and got["_amd_n_valid"].tolist() == [n, e, b]
    # padding rows: zeros, the smallest species of the store, the degree, the cell pad_length * I
    species = sorted({int(z) for g in graphs for z in g["atomic_numbers"].tolist()})
    assert not got["pos"][n:].any() and not got["elastic_tensor_full"][b:].any()
    assert (got["atomic_numbers"][n:] == species[0]).all()
    assert torch.equal(got["cell"][3 * b:], (pad_length * torch.eye(3)).repeat(k, 1))
    ei = got["edge_index"].numpy()
    lo = [j * (e_b - e) // p for j in range(p + 1)]
    owner = np.repeat(n + np.arange(p), np.diff(lo))
    assert np.array_equal(ei[0, e:], owner) and np.array_equal(ei[1, e:], owner)   # self-image edges, owner by owner
    degree = np.bincount(ei[1, e:] - n, minlength=n_b - n)
    assert got["num_neigh"].dtype == torch.float32 and np.array_equal(got["num_neigh"][n:].numpy(), degree.astype(np.float32))
    assert degree[p:].sum() == 0 and degree.max(initial=0) - degree[:p].min() <= 1
    # every padding edge has length pad_length: pos[dst] - pos[src] + shift @ cell of the edge's crystal
    shift, cell = got["edge_cell_shift"], got["cell"].view(b_b, 3, 3)
    crystal = got["batch"][got["edge_index"][0]]
    vec = got["pos"][got["edge_index"][1]] - got["pos"][got["edge_index"][0]] + torch.einsum("ej,ejk->ek", shift, cell[crystal])
    assert (crystal[e:] == b).all() and torch.equal(vec[e:].norm(dim=1), torch.full((e_b - e,), pad_length))
    assert torch.equal(shift[e:], torch.tensor([1.0, 0.0, 0.0]).repeat(e_b - e, 1))
    # the closed-form CSR = a stable sort of the padded edge_index by destination (and by source for the out-CSR)
    perm = np.argsort(ei[1], kind="stable")
    assert np.array_equal(got["_amd_perm"].numpy(), perm) and got["_amd_perm"].dtype == torch.int32
    assert np.array_equal(got["_amd_src_sorted"].numpy(), ei[0][perm])
    assert np.array_equal(got["_amd_rowptr"].numpy(), _rowptr(ei[1][perm], n_b))
    if training:
        src_sorted = ei[0][perm]
        out_perm = np.argsort(src_sorted, kind="stable")
        assert np.array_equal(got["_amd_dst_sorted"].numpy(), ei[1][perm])
        assert np.array_equal(got["_amd_out_perm"].numpy(), out_perm)
        assert np.array_equal(got["_amd_out_ptr"].numpy(), _rowptr(src_sorted[out_perm], n_b))


def test_pad_species(host):
    idx, pad_to = [0, 1], (40, 600, 3)
    species = sorted({int(z) for g in golden_graphs() for z in g["atomic_numbers"].tolist()})
    n, _ = _sizes(golden_graphs(), idx)
    got = host.padded_reference(idx, pad_to, pad_species=species[-1])
    assert (got["atomic_numbers"][n:] == species[-1]).all() and got["atomic_numbers"].dtype == torch.int64


def test_refusals(host):
    """each a ValueError from the host, before anything is launched"""
    idx = [10, 11, 12]
    n, e = _sizes(golden_graphs(), idx)
    species = sorted({int(z) for g in golden_graphs() for z in g["atomic_numbers"].tolist()})
    absent = next(z for z in range(1, 119) if z not in species)
    host.plan_padded(idx, (n + 2, e, 5))   # the tightest fit: K = 2, P = 1, no padding edge
    for bad in ((n + 1, e + 8, 5),          # N_b < N + K
                (n + 8, e - 1, 4),          # E_b < E
                (n + 8, e + 8, 3),          # B_b <= B
                (n + 8, e + 8, 2),
                (n + 8, e + 8)):
        with pytest.raises(ValueError):
            host.plan_padded(idx, bad)
        with pytest.raises(ValueError):
            host.padded_reference(idx, bad)
    ok = (n + 8, e + 8, 4)
    with pytest.raises(ValueError, match="pad_species"):
        host.padded_reference(idx, ok, pad_species=absent)
    for length in (0.0, -2.0, float("nan")):
        with pytest.raises(ValueError, match="pad_length"):
            host.padded_reference(idx, ok, pad_length=length)


def test_device_store_refuses_before_any_launch(host):
    """DeviceGraphStore.batch checks through the same host methods: with a library that must not be called"""
    from matten.data.store import DeviceGraphStore

    class NoLaunch:
        def __getattr__(self, name):
            raise AssertionError(f"{name} was called")

    store = DeviceGraphStore.__new__(DeviceGraphStore)
    store.host, store._lib, store.device = host, NoLaunch(), torch.device("cpu")
    idx = [10, 11, 12]
    n, e = _sizes(golden_graphs(), idx)
    for kw in (dict(pad_to=(n + 1, e + 8, 5)), dict(pad_to=(n + 8, e - 1, 4)), dict(pad_to=(n + 8, e + 8, 3)),
               dict(pad_to=(n + 8, e + 8, 4), pad_species=118), dict(pad_to=(n + 8, e + 8, 4), pad_length=0.0)):
        with pytest.raises(ValueError):
            store.batch(idx, **kw)


def test_loader_quantum_rule(host):
    """N_b = q ceil((N + K) / q), E_b = q ceil(E / q), B_b = batch_size + 1: a batch whose N + K already is a multiple of
    the quantum gets no extra block; the crystals and their order are those of the unpadded loader"""
    from matten.dataset.structure_scalar_tensor import _DeviceLoader

    graphs = golden_graphs()
    idx = list(range(20, 28))
    n, e = _sizes(graphs, idx)
    for batch_size in (8, 11):
        k = batch_size + 1 - len(idx)
        exact = _DeviceLoader(host, batch_size=batch_size, pad=(n + k, e))
        assert exact.padded_sizes(idx) == (n + k, e, batch_size + 1)
        over = _DeviceLoader(host, batch_size=batch_size, pad=(n + k - 1, e - 1))
        assert over.padded_sizes(idx) == (2 * (n + k - 1), 2 * (e - 1), batch_size + 1)
        host.plan_padded(idx, exact.padded_sizes(idx))   # accepted: P = 1
    loader = _DeviceLoader(host, batch_size=32, shuffle=True, seed=3, pad=(64, 2048))
    plain = _DeviceLoader(host, batch_size=32, shuffle=True, seed=3)
    batches = loader.batch_indices()
    assert batches == plain.batch_indices() and [len(i) for i in batches] == [32, 32, 32, 4]
    for i in batches:
        n_i, e_i = _sizes(graphs, i)
        n_b, e_b, b_b = loader.padded_sizes(i)
        assert b_b == 33 and n_b % 64 == 0 and e_b % 2048 == 0
        assert n_i + (33 - len(i)) <= n_b < n_i + (33 - len(i)) + 64 and e_i <= e_b < e_i + 2048
    assert _DeviceLoader(host, batch_size=32).pad is None   # off by default
    for bad in ((64,), (0, 8), (64, 2048, 3)):
        with pytest.raises(ValueError):
            _DeviceLoader(host, batch_size=32, pad=bad)


def test_data_module_pads_the_train_loader_only():
    from store_cases import data_module

    dm = data_module(device="cuda:0", device_resident=True, loader_kwargs={"batch_size": 32, "pad": (64, 2048)})
    assert dm._eval_kwargs() == {"batch_size": 32, "shuffle": False}
    assert dm.loader_kwargs["pad"] == (64, 2048)
    with pytest.raises(ValueError, match="device_resident"):   # the host loader does not pad: refused, not ignored
        data_module(loader_kwargs={"batch_size": 32, "pad": (64, 2048)})
    data_module(loader_kwargs={"batch_size": 32, "pad": None})


def test_padded_mean_loss_refuses_an_unpadded_batch():
    from matten_amd.graphs import padded_mean_loss

    loss = padded_mean_loss(lambda p, t: (p - t) ** 2)
    with pytest.raises(ValueError, match="_amd_n_valid"):
        loss(torch.zeros(3, 2), torch.zeros(3, 2), {"pos": torch.zeros(4, 3)})
    n_valid = torch.tensor([0, 0, 2])
    got = loss(torch.tensor([[1.0, 3.0], [2.0, 0.0], [float("nan"), 9.0]]), torch.zeros(3, 2), {"_amd_n_valid": n_valid})
    assert float(got) == (1.0 + 9.0 + 4.0 + 0.0) / 4


def test_new_symbols_and_abi():
    """entries were only added"""
    from matten_amd import _lib
    from matten_amd.data import _key, store

    lib = _lib.load()
    assert _lib.ABI_VERSION == 47 and lib.matten_abi_version() == 47
    for name in ("matten_batch_gather_padded", "matten_bn_train_fwd_valid", "matten_bn_train_bwd_valid"):
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    assert _key.AMD_N_VALID == "_amd_n_valid"
    # MATTEN_EINVAL for what the host can see, before any launch (the pointers are never dereferenced)
    buf = np.zeros(64, dtype=np.int64)
    p = buf.ctypes.data

    def call(stream, table=p, sizes=(3, 10, 10), valid=(2, 8, 8), n_valid=p):
        d = np.asarray([stream], dtype=np.int64)
        assert d.shape == (1, store.PAD_STREAM_WORDS)
        return lib.matten_batch_gather_padded(d.ctypes.data, 1, table, *sizes, *valid, n_valid, None)

    ok = (p, p, 4, 3, store.NODE, store.OP_RAW, store.PAD_ZERO, 0)
    assert call(ok, n_valid=None) == -1 and call(ok, table=None) == -1
    assert call(ok, valid=(3, 8, 8)) == -1      # no padding crystal
    assert call(ok, valid=(1, 9, 8)) == -1      # two padding crystals, one padding node
    assert call(ok, valid=(2, 8, 11)) == -1     # fewer edges than the batch holds
    assert call(ok, valid=(-1, 8, 8)) == -1 and call(ok, sizes=(3, 2 ** 31, 10)) == -1
    assert call((p, p, 4, 3, store.NODE, store.OP_RAW, 5, 0)) == -1 and call((p, p, 4, 3, store.NODE, store.OP_RAW, -1, 0)) == -1
    assert call((p, p, 4, 1, store.EDGE, store.OP_ADD32_EDGE, store.PAD_CONST, 1)) == -1   # a fill off a RAW stream
    assert call((p, p, 8, 1, store.NODE, store.OP_RAW, store.PAD_DEGREE, 0)) == -1         # the degree is one float per node
    assert call((p, p, 4, 1, store.EDGE, store.OP_RAW, store.PAD_DEGREE, 0)) == -1
    assert call((p, p, 4, 3, store.CRYSTAL, store.OP_RAW, store.PAD_DIAG3, 0)) == -1       # the diagonal of a 3 x 3 row
    assert call((p, p, 2, 3, store.NODE, store.OP_RAW, store.PAD_ZERO, 0)) == -1
    # the valid-rows BatchNorm entries refuse a NULL count before anything else happens
    f = lib.matten_bn_train_fwd_valid(p, 4, 8, p, p, 1, p, p, 1e-5, p, p, p, None, None, 0.1, None, None, None)
    b = lib.matten_bn_train_bwd_valid(p, p, 4, 8, p, p, 1, p, p, p, 1e-5, p, p, p, None, None, None, None, None)
    assert f == -1 and b == -1


def test_both_gather_entries_refuse_the_same_streams():
    """one decoder behind both entries: every six-word record matten_batch_gather refuses (the rows of
    test_store_host.py::test_batch_gather_argument_errors), extended by the fill (PAD_ZERO, 0), is refused by
    matten_batch_gather_padded too, before any launch"""
    from matten_amd import _lib
    from matten_amd.data import store

    lib = _lib.load()
    buf = np.zeros(64, dtype=np.int64)
    p = buf.ctypes.data
    bad = refused_streams(p)
    assert len(bad) >= 22

    def plain(streams):
        d = np.asarray(streams, dtype=np.int64).reshape(-1, store.STREAM_WORDS)
        return lib.matten_batch_gather(d.ctypes.data, len(d), p, 1, 1, 1, None)

    def padded(streams):   # (the sizes of test_new_symbols_and_abi: a good record passes every check with them)
        d = np.asarray([tuple(s) + (store.PAD_ZERO, 0) for s in streams], dtype=np.int64).reshape(-1, store.PAD_STREAM_WORDS)
        return lib.matten_batch_gather_padded(d.ctypes.data, len(d), p, 3, 10, 10, 2, 8, 8, p, None)

    for streams in bad:
        assert plain(streams) == -1, streams
        assert padded(streams) == -1, streams
