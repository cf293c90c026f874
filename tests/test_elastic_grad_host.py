"""
CPU tests of the differentiable derived elastic properties (matten_amd/elastic.py: elastic_moduli, ModuliLoss; the entry
matten_elastic_props_bwd): declarations and bindings, argument validation, the loss's masking, and the fp64 torch statement
of the forward that tests/test_gpu_elastic_grad.py differentiates as its reference.  No kernel is launched.

The reference (``ref_forward``) is written out here -- the 8-position mean or (C + C^T)/2, torch.linalg.inv, the textbook
formulas -- and shares no code with matten_amd.elastic; torch.autograd.gradcheck ties its autograd to finite differences.
"""
import json
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# pymatgen's Voigt order: xx, yy, zz, yz, xz, xy
PAIRS = ((0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1))
NAMES = ("k_voigt", "g_voigt", "k_reuss", "g_reuss", "k_vrh", "g_vrh", "y_mod", "homogeneous_poisson",
         "universal_anisotropy", "pugh_ratio")
_FLAT = [((i * 3 + j) * 3 + k) * 3 + l for (i, j) in PAIRS for (k, l) in PAIRS]


# ---------------------------------------------------------------------------------------------------
# the reference forward: torch fp64, differentiable
# ---------------------------------------------------------------------------------------------------
def symmetrise_cartesian(c4):
    """[B,3,3,3,3] -> the mean over ij<->ji, kl<->lk, (ij)<->(kl)"""
    s = c4 + c4.transpose(1, 2)
    s = s + s.transpose(3, 4)
    s = s + s.permute(0, 3, 4, 1, 2)
    return s / 8.0


def ref_voigt(c, layout):
    """c [B,81] (layout 0) or [B,36] (layout 1) -> the symmetrised Voigt matrices [B,6,6]"""
    if layout == 0:
        return symmetrise_cartesian(c.reshape(-1, 3, 3, 3, 3)).reshape(-1, 81)[:, _FLAT].reshape(-1, 6, 6)
    C = c.reshape(-1, 6, 6)
    return 0.5 * (C + C.transpose(1, 2))


def ref_scalars(C, S):
    """the ten scalars [B,10] of the matrices C and S = C^-1 [B,6,6], from the entries on and above the diagonal"""
    cd, co, cs = C[:, 0, 0] + C[:, 1, 1] + C[:, 2, 2], C[:, 0, 1] + C[:, 0, 2] + C[:, 1, 2], C[:, 3, 3] + C[:, 4, 4] + C[:, 5, 5]
    sd, so, ss = S[:, 0, 0] + S[:, 1, 1] + S[:, 2, 2], S[:, 0, 1] + S[:, 0, 2] + S[:, 1, 2], S[:, 3, 3] + S[:, 4, 4] + S[:, 5, 5]
    kv, gv, kr, gr = (cd + 2 * co) / 9, (cd - co + 3 * cs) / 15, 1 / (sd + 2 * so), 15 / (4 * sd - 4 * so + 3 * ss)
    K, G = (kv + kr) / 2, (gv + gr) / 2
    return torch.stack([kv, gv, kr, gr, K, G, 9 * K * G / (3 * K + G), (3 * K - 2 * G) / (2 * (3 * K + G)),
                        5 * gv / gr + kv / kr - 6, K / G], dim=1)


def ref_forward(c, layout):
    """-> (voigt [B,6,6], compliance [B,6,6], props [B,10]) in the dtype of c"""
    C = ref_voigt(c, layout)
    S = torch.linalg.inv(C)
    return C, S, ref_scalars(C, S)


def example_tensors():
    """the 100 Cartesian tensors of the example data set, fp64 [100,3,3,3,3]"""
    raw = json.load(open(os.path.join(ROOT, "tests", "golden", "example_crystal_elasticity_tensor_n100.json")))
    keys = sorted(raw["elastic_tensor_full"], key=int)
    return np.array([raw["elastic_tensor_full"][k] for k in keys], dtype=np.float64)


def fake_props(B=5, seed=0, requires_grad=True, **override):
    """a hand-built ElasticProperties of plain CPU tensors (no kernel): every scalar an independent leaf"""
    from matten_amd.elastic import ElasticProperties

    g = torch.Generator().manual_seed(seed)
    fields = {n: (50.0 + 10.0 * torch.randn(B, generator=g, dtype=torch.float64)).requires_grad_(requires_grad) for n in NAMES}
    fields["flags"] = torch.zeros(B, dtype=torch.int32)
    fields.update(override)
    return ElasticProperties(**fields)


# ---------------------------------------------------------------------------------------------------
# tests
# ---------------------------------------------------------------------------------------------------
def test_library_declares_and_binds_the_adjoint_entry():
    from matten_amd import _lib, autograd, ops

    header = open(os.path.join(ROOT, "include", "matten_hip.h")).read()
    declared = set(re.findall(r"\b(matten_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    name = "matten_elastic_props_bwd"
    assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.ABI_VERSION == 47 and lib.matten_abi_version() == 47          # entries were only added
    assert callable(ops.elastic_props_bwd) and issubclass(autograd.ElasticPropsFn, torch.autograd.Function)
    # host-detectable argument errors as in matten_elastic_props, no GPU touched
    nul = (None,) * 7
    assert lib.matten_elastic_props_bwd(*nul, 0, 0, 3, None, None) == -1       # null required pointers
    assert lib.matten_elastic_props_bwd(*nul, 0, 2, 0, None, None) == -1       # bad layout
    assert lib.matten_elastic_props_bwd(*nul, 2, 0, 0, None, None) == -1       # bad dtype switch
    assert lib.matten_elastic_props_bwd(*nul, 1, 1, -1, None, None) == -1      # negative n
    assert lib.matten_elastic_props_bwd(*nul, 1, 1, 0, None, None) == 0        # n == 0


def test_elastic_moduli_refuses_what_it_cannot_differentiate_before_touching_the_device():
    from matten_amd import elastic

    with pytest.raises(ValueError, match="elastic_properties"):
        elastic.elastic_moduli(torch.zeros(2, 6, 6))                           # a host tensor
    with pytest.raises(ValueError, match="elastic_properties"):
        elastic.elastic_moduli(np.zeros((2, 6, 6)))
    with pytest.raises(ValueError, match="elastic_properties"):
        elastic.elastic_moduli([torch.zeros(6, 6)])
    for bad in (torch.zeros(2, 3, 3), torch.zeros(2, 6, 5), torch.zeros(1, 2, 3, 3, 3, 3), torch.zeros(36)):
        with pytest.raises(ValueError):
            elastic.elastic_moduli(bad)
    with pytest.raises(TypeError):
        elastic.elastic_moduli(torch.zeros(2, 6, 6, dtype=torch.int64))
    with pytest.raises(TypeError):
        elastic.elastic_moduli(torch.zeros(2, 6, 6, dtype=torch.float16))
    with pytest.raises(ValueError):
        elastic.elastic_moduli_from_irreps(torch.zeros(2, 20))
    with pytest.raises(ValueError, match="elastic_properties_from_irreps"):
        elastic.elastic_moduli_from_irreps(torch.zeros(2, 21))                 # a host tensor
    with pytest.raises(ValueError):
        elastic.elastic_moduli_from_irreps(np.zeros((2, 21)))


def test_moduli_loss_argument_validation():
    from matten_amd.elastic import ModuliLoss

    assert ModuliLoss().names == ("k_vrh", "g_vrh") and ModuliLoss().kind == "l1"
    assert isinstance(ModuliLoss(), torch.nn.Module)
    with pytest.raises(ValueError, match="bulk"):
        ModuliLoss(names=("k_vrh", "bulk"))
    with pytest.raises(ValueError):
        ModuliLoss(names=())
    with pytest.raises(ValueError):
        ModuliLoss(names=("k_vrh", "k_vrh"))
    with pytest.raises(ValueError):
        ModuliLoss(kind="huber")
    with pytest.raises(ValueError):
        ModuliLoss(weights=(1.0,))
    with pytest.raises(ValueError):
        ModuliLoss(weights={"k_vrh": 1.0})
    with pytest.raises(ValueError):
        ModuliLoss(weights=(1.0, float("nan")))
    assert ModuliLoss(weights=(2.0, 0.5)).weights == {"k_vrh": 2.0, "g_vrh": 0.5}
    assert ModuliLoss(names="y_mod", weights={"y_mod": 3}).weights == {"y_mod": 3.0}
    p = fake_props()
    with pytest.raises(ValueError, match="g_vrh"):
        ModuliLoss()(p, {"k_vrh": torch.zeros(5)})
    with pytest.raises(ValueError, match="shape"):
        ModuliLoss()(p, {"k_vrh": torch.zeros(5), "g_vrh": torch.zeros(4)})


@pytest.mark.parametrize("kind", ["l1", "mse"])
def test_moduli_loss_value_and_masking(kind):
    from matten_amd.elastic import ModuliLoss

    B = 5
    flags = torch.tensor([0, 1, 2, 3, 0], dtype=torch.int32)         # rows 1 and 3 singular; row 2 merely indefinite
    p = fake_props(B, flags=flags)
    with torch.no_grad():
        for n in NAMES:                                              # what the kernel writes on a singular row
            getattr(p, n)[flags.bool() & (flags & 1).bool()] = float("nan")
    tk = torch.tensor([40.0, 41.0, float("nan"), 43.0, 44.0], dtype=torch.float64)
    tg = torch.tensor([float("inf"), 31.0, 32.0, 33.0, 34.0], dtype=torch.float64)
    loss = ModuliLoss(weights=(1.0, 0.25), kind=kind)(p, {"k_vrh": tk, "g_vrh": tg})
    # by hand: k_vrh uses rows 0 and 4, g_vrh rows 2 and 4 -> four entries
    f = (lambda d: d.abs()) if kind == "l1" else (lambda d: d * d)
    k, g = p.k_vrh.detach(), p.g_vrh.detach()
    want = (f(k[0] - 40.0) + f(k[4] - 44.0) + 0.25 * (f(g[2] - 32.0) + f(g[4] - 34.0))) / 4.0
    assert torch.isfinite(loss) and abs(loss.item() - want.item()) <= 1e-12 * abs(want.item())
    loss.backward()
    gk, gg = p.k_vrh.grad, p.g_vrh.grad
    assert torch.isfinite(gk).all() and torch.isfinite(gg).all()
    assert torch.equal(gk[[1, 2, 3]], torch.zeros(3, dtype=torch.float64))      # exactly zero, not NaN * 0
    assert torch.equal(gg[[0, 1, 3]], torch.zeros(3, dtype=torch.float64))
    assert (gk[[0, 4]] != 0).all() and (gg[[2, 4]] != 0).all()
    assert p.y_mod.grad is None


def test_moduli_loss_with_every_entry_excluded_is_a_zero_with_a_graph():
    from matten_amd.elastic import ModuliLoss

    p = fake_props(3, flags=torch.tensor([1, 3, 0], dtype=torch.int32))
    nan = torch.full((3,), float("nan"), dtype=torch.float64)
    loss = ModuliLoss()(p, {"k_vrh": nan, "g_vrh": torch.tensor([1.0, 2.0, float("nan")], dtype=torch.float64)})
    assert loss.item() == 0.0 and loss.grad_fn is not None
    loss.backward()
    assert torch.equal(p.k_vrh.grad, torch.zeros(3, dtype=torch.float64))
    assert torch.equal(p.g_vrh.grad, torch.zeros(3, dtype=torch.float64))
    # an unbatched ElasticProperties works the same
    q = fake_props(3)
    one = type(q)(**{n: getattr(q, n)[0] for n in NAMES + ("flags",)})
    l1 = ModuliLoss()(one, {"k_vrh": 40.0, "g_vrh": 30.0})
    assert l1.shape == () and abs(l1.item() - 0.5 * (abs(q.k_vrh[0].item() - 40.0) + abs(q.g_vrh[0].item() - 30.0))) <= 1e-12


@pytest.mark.parametrize("layout", [0, 1])
def test_reference_forward_passes_gradcheck_and_matches_numpy(layout):
    """the reference the GPU test leans on: its autograd against finite differences on three tensors of the example set
    (plus noise, so that the symmetrisation is exercised), its values against numpy"""
    full = example_tensors()
    assert full.shape == (100, 3, 3, 3, 3)
    rng = np.random.default_rng(3)
    for r in (0, 41, 99):
        c4 = full[r] + 0.5 * rng.standard_normal((3, 3, 3, 3))
        c = torch.tensor(c4.reshape(1, 81) if layout == 0 else c4.reshape(81)[_FLAT].reshape(1, 36), dtype=torch.float64)
        C, S, P = ref_forward(c, layout)
        Cn = C[0].numpy()
        assert np.array_equal(Cn, Cn.T) and np.linalg.cond(Cn) <= 100
        Sn = S[0].numpy()
        assert np.abs(Sn - np.linalg.inv(Cn)).max() <= 1e-12 * np.abs(Sn).max()
        sd, so = np.trace(Sn[:3, :3]), Sn[0, 1] + Sn[0, 2] + Sn[1, 2]
        assert abs(P[0, 2].item() - 1 / (sd + 2 * so)) <= 1e-12 * abs(P[0, 2].item())
        assert abs(P[0, 4].item() - 0.5 * (P[0, 0] + P[0, 2]).item()) <= 1e-12 * abs(P[0, 4].item())
        if layout == 0:      # the mean of the 8 positions, written as an explicit loop
            want = np.zeros((6, 6))
            for I, (i, j) in enumerate(PAIRS):
                for J, (k, l) in enumerate(PAIRS):
                    want[I, J] = (c4[i, j, k, l] + c4[j, i, k, l] + c4[i, j, l, k] + c4[j, i, l, k] + c4[k, l, i, j] + c4[k, l, j, i]
                                  + c4[l, k, i, j] + c4[l, k, j, i]) / 8.0
            assert np.abs(Cn - want).max() <= 1e-13 * np.abs(want).max()

        def fn(x):
            C, S, P = ref_forward(x, layout)
            return torch.cat([C.reshape(-1), S.reshape(-1) * 1e4, P.reshape(-1)])   # S ~ 1e-2 / GPa: lifted to O(1)

        assert torch.autograd.gradcheck(fn, (c.clone().requires_grad_(),), eps=1e-4, atol=1e-6, rtol=1e-5)
