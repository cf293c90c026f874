#!/usr/bin/env python3
"""Optimisation step of the lmax-2 configuration with BatchNorm in training mode against the same step with frozen
statistics (model.freeze_batchnorm), eager and replayed from a hipGraph, at the batch sizes given (default 32 2048):
step time and the number of library entries called per eager step.   python3 tools/frozen_bn_bench.py [BATCH ...]"""
import os, sys, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from common import LMAX2
from matten_amd import _lib
from matten_amd.data.graph import average_num_neighbors, collate, crystal_graph
from matten_amd.data.io import structures_from_json
from matten_amd.graphs import GraphedTrainStep
from matten_amd.model import freeze_batchnorm
from matten_amd.model_factory.tfn_scalar_tensor import ScalarTensorModel
from matten_amd.optim import FlatAdam

dev = "cuda:0"
n100 = structures_from_json(os.path.join(ROOT, "tests", "golden", "example_crystal_elasticity_tensor_n100.json"))
graphs = [crystal_graph(s["cart_coords"], s["lattice"], s["atomic_numbers"], 5.0) for s in n100]
ds = {"allowed_species": sorted({int(z) for s in n100 for z in s["atomic_numbers"]}),
      "average_num_neighbors": average_num_neighbors(graphs)}
CALLS = [0]
_check = _lib.check


def counting_check(rc, what):
    CALLS[0] += 1
    return _check(rc, what)


def loss_fn(preds, t):
    return torch.nn.functional.mse_loss(preds["elastic_tensor_full"], t)


def make(frozen):
    torch.manual_seed(3)
    m = ScalarTensorModel(backbone_hparams=dict(LMAX2), dataset_hparams=ds).to(dev).train()
    if frozen:
        freeze_batchnorm(m)
    return m, FlatAdam(m.parameters(), lr=1e-2, weight_decay=1e-5)


def timed(fn, warm, n):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


for B in [int(a) for a in sys.argv[1:]] or [32, 2048]:
    batch = collate([graphs[i % len(graphs)] for i in range(B)], device=dev)
    target = torch.randn(B, 21, device=dev)
    warm, n = (5, 30) if B <= 256 else (3, 8)
    for frozen in (False, True):
        m, opt = make(frozen)

        def step():
            loss = loss_fn(m(dict(batch))[0], target)
            opt.zero_grad()
            loss.backward()
            opt.step()

        eager = timed(step, warm, n)
        _lib.check = counting_check
        CALLS[0] = 0
        step()
        calls = CALLS[0]
        _lib.check = _check
        g = GraphedTrainStep(m, opt, loss_fn, batch, target, warmup=2)
        graphed = timed(lambda: g.step(batch, target), warm, n)
        print(f"batch {B} ({batch['pos'].shape[0]} nodes, {batch['edge_index'].shape[1]} edges) "
              f"{'frozen statistics' if frozen else 'train-mode BatchNorm'}: eager {eager:.3f} ms/step, hipGraph {graphed:.3f} ms/step, "
              f"{calls} library entries per step", flush=True)
        del g, m, opt
        torch.cuda.empty_cache()
