"""Geometry gradients, the parts a machine without a GPU can check: the three entries are exported and bound, refuse bad
arguments on the host, and ``strain_gradient`` is the strain response of an invariant of the edge vectors."""
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("matten_tp_backward_sh", "matten_radial_mlp_bwd_len", "matten_edge_geom_bwd")
EINVAL = -1


def test_entries_are_declared_exported_and_bound():
    from matten_amd import _lib

    header = open(os.path.join(ROOT, "include", "matten_hip.h")).read()
    declared = set(re.findall(r"\b(matten_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for name in ENTRIES:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.matten_abi_version() == _lib.ABI_VERSION == 47   # entries were only added
    from matten_amd import autograd, ops

    assert all(hasattr(ops, n) for n in ("tp_backward_sh", "radial_mlp_bwd_len", "edge_geom_bwd"))
    assert hasattr(autograd, "EdgeGeomFn")


def test_host_detectable_argument_errors():
    from matten_amd import _lib

    lib = _lib.load()

    def sh(n_edges=0, max_l=2, sh_stride=32):
        return lib.matten_tp_backward_sh(None, 8, None, 16, None, None, None, 1, 4, None, 1, None, 8, 18.0, None, n_edges, 0, None,
                                         sh_stride, max_l, None)

    assert sh() == 0                       # an empty batch is fine and touches nothing
    assert sh(n_edges=-1) == EINVAL
    assert sh(max_l=5) == EINVAL
    assert sh(max_l=4, sh_stride=16) == EINVAL
    assert sh(n_edges=3) == EINVAL         # null operands

    def ln(n_edges=0, n_mid=1, nb_pad=8, w_pad=16):
        return lib.matten_radial_mlp_bwd_len(None, n_edges, 8, 0.0, 5.0, None, nb_pad, None, n_mid, None, 32, w_pad, 16, None, 16,
                                             0, None, None)

    assert ln() == 0
    assert ln(n_edges=-1) == EINVAL
    assert ln(n_mid=4) == EINVAL
    assert ln(nb_pad=6) == EINVAL
    assert ln(w_pad=24) == EINVAL
    assert ln(n_edges=3) == EINVAL

    def gb(n_edges=0, lmax=2, n_nodes=0):
        return lib.matten_edge_geom_bwd(None, None, 32, None, lmax, n_edges, n_nodes, None, None, None, None, None, 0, None, None,
                                        None, None, None)

    assert gb() == 0
    assert gb(n_edges=-1) == EINVAL
    assert gb(lmax=5) == EINVAL
    assert gb(n_edges=3) == EINVAL         # edges without atoms


def test_matten_geometry_resolves_through_the_alias():
    import matten.geometry
    import matten_amd.geometry

    assert matten.geometry is matten_amd.geometry
    assert callable(matten.geometry.strain_gradient) and callable(matten.geometry.geometry_gradients)


def _toy(pos, cell, edge_index, shift, batch):
    """a rotation-invariant scalar of the edge vectors"""
    src, dst = edge_index
    v = pos[dst] - pos[src] + torch.einsum("ni,nij->nj", shift, cell[batch[src]])
    r2 = (v * v).sum(1)
    same = batch[src][:-1] == batch[src][1:]     # neighbouring edges of one crystal (each crystal is strained on its own)
    return (torch.exp(-0.3 * r2) * (1.0 + r2)).sum() + (((v[:-1] * v[1:]).sum(1) ** 2) * same).sum()


def test_strain_gradient_is_the_response_to_a_homogeneous_deformation():
    from matten_amd.geometry import strain_gradient

    gen = torch.Generator().manual_seed(3)
    sizes = [4, 5]
    batch = torch.cat([torch.full((n,), b) for b, n in enumerate(sizes)])
    pos = torch.randn(9, 3, generator=gen, dtype=torch.float64)
    cell = torch.eye(3, dtype=torch.float64) * 3.0 + 0.3 * torch.randn(2, 3, 3, generator=gen, dtype=torch.float64)
    src = torch.tensor([0, 1, 2, 3, 0, 4, 5, 6, 7, 8, 4, 4])
    dst = torch.tensor([1, 2, 3, 0, 0, 5, 6, 7, 8, 4, 4, 6])
    edge_index = torch.stack([src, dst])
    shift = torch.randint(-1, 2, (12, 3), generator=gen).double()
    shift[4] = torch.tensor([1.0, 0.0, 0.0])    # self images
    shift[10] = torch.tensor([0.0, 1.0, -1.0])

    p, c = pos.clone().requires_grad_(True), cell.clone().requires_grad_(True)
    _toy(p, c, edge_index, shift, batch).backward()
    got = strain_gradient({"pos": p, "cell": c, "batch": batch})

    # the definition: positions and lattice vectors of crystal b deformed together, x -> x (1 + eps_b)
    eps = torch.zeros(2, 3, 3, dtype=torch.float64, requires_grad=True)
    F = torch.eye(3, dtype=torch.float64) + eps
    L = _toy(torch.einsum("ni,nij->nj", pos, F[batch]), cell @ F, edge_index, shift, batch)
    (want,) = torch.autograd.grad(L, eps)
    assert got.shape == (2, 3, 3)
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-12)
    assert torch.allclose(got, got.transpose(1, 2), rtol=1e-10, atol=1e-10), "symmetric for a rotation-invariant scalar"
    assert want.abs().max() > 1e-3

    # open structures: no cell, one crystal without a batch vector
    p = pos[:4].clone().requires_grad_(True)
    v = p[dst[:4]] - p[src[:4]]
    ((v * v).sum(1) ** 1.5).sum().backward()
    one = strain_gradient({"pos": p})
    assert one.shape == (1, 3, 3) and torch.allclose(one[0], p.detach().t() @ p.grad)
