#!/usr/bin/env python3
"""What geometry gradients cost: the backward of the lmax-2 model on the n100 sample tiled to BATCH crystals (default
2048), materialised-w route (MATTEN_TRAIN_TP=paths), train mode, in ONE process with alternating arms:
    A   parameters require grad                      (the training step's backward, as before)
    B   parameters, pos and cell require grad        (adds matten_tp_backward_sh + matten_radial_mlp_bwd_len per conv layer
                                                      and one matten_edge_geom_bwd)
Each round times, per arm, REPS forward + backward pairs with device events around the forward and around the backward;
printed: the median over the rounds and the spread (min .. max) per arm, and B - A.
    python3 tools/geom_grad_bench.py [--batch 2048] [--rounds 7] [--reps 5] [--arms AB]
--arms A runs on a tree without the feature (the parent's number from the same script)."""
import argparse, os, statistics, sys

os.environ["MATTEN_TRAIN_TP"] = "paths"
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from common import LMAX2
from matten_amd.data.graph import average_num_neighbors, collate, crystal_graph
from matten_amd.data.io import structures_from_json
from matten_amd.model_factory.tfn_scalar_tensor import ScalarTensorModel

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=2048)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--arms", default="AB")
args = ap.parse_args()

dev = "cuda:0"
n100 = structures_from_json(os.path.join(ROOT, "tests", "golden", "example_crystal_elasticity_tensor_n100.json"))
graphs = [crystal_graph(s["cart_coords"], s["lattice"], s["atomic_numbers"], 5.0) for s in n100]
ds = {"allowed_species": sorted({int(z) for s in n100 for z in s["atomic_numbers"]}),
      "average_num_neighbors": average_num_neighbors(graphs)}
torch.manual_seed(3)
model = ScalarTensorModel(backbone_hparams=dict(LMAX2), dataset_hparams=ds).to(dev).train()
base = collate([graphs[i % len(graphs)] for i in range(args.batch)], device=dev)
target = torch.randn(args.batch, 21, device=dev)
print(f"batch {args.batch}: {base['pos'].shape[0]} nodes, {base['edge_index'].shape[1]} edges", flush=True)


def one(arm):
    """-> (forward ms, backward ms) of one pair"""
    b = dict(base)
    if arm == "B":
        b["pos"] = base["pos"].clone().requires_grad_(True)
        b["cell"] = base["cell"].clone().requires_grad_(True)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    model.zero_grad(set_to_none=True)
    ev[0].record()
    loss = torch.nn.functional.mse_loss(model(b)[0]["elastic_tensor_full"], target)
    ev[1].record()
    loss.backward()
    ev[2].record()
    torch.cuda.synchronize()
    if arm == "B":
        assert b["pos"].grad is not None and b["cell"].grad is not None
    return ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2])


for arm in args.arms:   # every shape warmed
    for _ in range(3):
        one(arm)
rounds = {arm: [] for arm in args.arms}
for r in range(args.rounds):
    for arm in (args.arms if r % 2 == 0 else args.arms[::-1]):   # alternating, order swapped every round
        ts = [one(arm) for _ in range(args.reps)]
        rounds[arm].append((statistics.median(t[0] for t in ts), statistics.median(t[1] for t in ts)))
med = {}
for arm in args.arms:
    f, bw = [x[0] for x in rounds[arm]], [x[1] for x in rounds[arm]]
    med[arm] = statistics.median(bw)
    print(f"arm {arm}: backward median {med[arm]:.3f} ms (rounds {min(bw):.3f} .. {max(bw):.3f}), "
          f"forward median {statistics.median(f):.3f} ms (rounds {min(f):.3f} .. {max(f):.3f})", flush=True)
if "A" in med and "B" in med:
    print(f"B - A: {med['B'] - med['A']:.3f} ms per backward ({100.0 * (med['B'] / med['A'] - 1.0):.1f} %)")
