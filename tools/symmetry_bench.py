#!/usr/bin/env python3
"""Rotations and symmetry averages of irreps rows: the kernels of csrc/rotate.hip against what a user can write without
them, in one process with the arms alternating

  arm K   ``ops.irreps_rotate`` / ``ops.irreps_average`` on a D table made once by ``ops.wigner_d``;
  arm T   host-built D_f matrices [G,21,21] (``symmetry.formula_D_host``) uploaded once, then a batched ``torch.matmul`` on
          the device: ``(Dbar @ x.T).T`` with the group's mean matrix for the average (one matrix: what a user would
          precompute), ``torch.bmm(full, x[:, :, None])`` over a prebuilt ``full`` [n,21,21] (one matrix per row, no gather)
          for one rotation per row.

Cases, rows of ``ijkl=jikl=klij`` (21 components) in fp32 and fp64:
  average   `--rows-average` rows (default 1e5), every row over the same 48 cubic operations (shared op_idx);
  rotate    `--rows-rotate` rows (default 1e6), one rotation each (G = n; the D table and the [n,21,21] matrices are built
            outside the timed window).
Every arm runs `--warmup` times, then `--reps` times between device events, the arms alternating rep by rep; medians and
min-max in ms, and for the kernel arm the bytes per second against the rows' compulsory traffic (x read and out written
once; for rotate also the blocks of the row's D that 2x0e+2x2e+4e needs, D^0, D^2 and D^4: 1 + 25 + 81 = 107 doubles per row).  The machine's calibration record comes first.  There is no
pass/fail threshold: the numbers are for docs/LAB_NOTES.md and INTEGRATION.md "Rotations and symmetry of irreps tensors".

    python tools/symmetry_bench.py [--rows-average 100000] [--rows-rotate 1000000] [--reps 20] [--warmup 5]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from matten_amd import ops  # noqa: E402
from matten_amd.symmetry import formula_D_host, group_closure, irreps_layout  # noqa: E402

DEV = "cuda:0"
FORMULA = "ijkl=jikl=klij"
DIM = 21


def cubic_group() -> np.ndarray:
    c, s = 0.0, 1.0
    c4 = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    c3 = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    return group_closure([c4, c3, -np.eye(3)])


def random_rotations(n: int, seed: int) -> torch.Tensor:
    """n proper rotations on the device (QR of Gaussian matrices)"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    q, r = torch.linalg.qr(torch.randn(n, 3, 3, dtype=torch.float64, device=DEV, generator=g))
    q = q * torch.sign(torch.diagonal(r, dim1=1, dim2=2))[:, None, :]
    return q * torch.linalg.det(q)[:, None, None]


def timed(arms: dict, reps: int, warmup: int) -> dict:
    for arm in arms.values():
        for _ in range(warmup):
            arm()
    torch.cuda.synchronize()
    times = {name: [] for name in arms}
    for _ in range(reps):
        for name, arm in arms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            arm()
            b.record()
            times[name].append((a, b))
    torch.cuda.synchronize()
    out = {}
    for name, evs in times.items():
        ms = sorted(a.elapsed_time(b) for a, b in evs)
        out[name] = {"median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4)}
    return out


def bench_average(n: int, dtype, reps: int, warmup: int) -> dict:
    layout = irreps_layout(FORMULA)
    group = cubic_group()
    G = len(group)
    x = torch.randn(n, DIM, dtype=dtype, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    out = torch.empty_like(x)
    D, flags = ops.wigner_d(torch.as_tensor(group, device=DEV), 4)
    op_ptr = torch.arange(n + 1, dtype=torch.int64, device=DEV) * G
    op_idx = torch.arange(G, dtype=torch.int32, device=DEV).repeat(n)
    mean = torch.as_tensor(formula_D_host(FORMULA, group).mean(axis=0), dtype=dtype, device=DEV)

    def kernel():
        ops.irreps_average(x, layout, D, flags, op_ptr, op_idx, want_deviation=False, out=out)

    def kernel_with_deviation():
        ops.irreps_average(x, layout, D, flags, op_ptr, op_idx, out=out)

    def torch_mean_matrix():
        torch.matmul(x, mean.T)

    def torch_mean_matrix_with_deviation():
        avg = torch.matmul(x, mean.T)
        (x - avg).norm(dim=1) / x.norm(dim=1)

    res = timed({"kernel": kernel, "kernel+deviation": kernel_with_deviation, "torch_matmul": torch_mean_matrix,
                 "torch_matmul+deviation": torch_mean_matrix_with_deviation}, reps, warmup)
    compulsory = 2 * n * DIM * x.element_size()
    res["kernel"]["GBps_of_compulsory"] = round(compulsory / (res["kernel"]["median_ms"] * 1e-3) / 1e9, 1)
    return {"case": "average", "rows": n, "operations": G, "dtype": str(dtype), "compulsory_bytes": compulsory, **res}


def bench_rotate(n: int, dtype, reps: int, warmup: int) -> dict:
    layout = irreps_layout(FORMULA)
    x = torch.randn(n, DIM, dtype=dtype, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    out = torch.empty_like(x)
    R = random_rotations(n, seed=3)
    D, flags = ops.wigner_d(R, 4)
    # the plain-torch arm's matrices: block diagonal [n,21,21] assembled from the table (outside the timed window, as the
    # table is for the kernel arm)
    full = torch.zeros(n, DIM, DIM, dtype=dtype, device=DEV)
    offs = {0: 0, 2: 10, 4: 84}
    for off, mul, l, _ in layout.tolist():
        m = 2 * l + 1
        block = D[:, offs[l]:offs[l] + m * m].reshape(n, m, m).to(dtype)
        for u in range(mul):
            full[:, off + u * m:off + (u + 1) * m, off + u * m:off + (u + 1) * m] = block

    def kernel():
        ops.irreps_rotate(x, layout, D, flags, out=out)

    def torch_bmm():
        torch.bmm(full, x[:, :, None])

    def table():
        ops.wigner_d(R, 4, out=(D, flags))

    res = timed({"kernel": kernel, "torch_bmm": torch_bmm, "wigner_d_table": table}, reps, warmup)
    compulsory = 2 * n * DIM * x.element_size() + n * (1 + 25 + 81) * 8      # x, out, and the blocks D^0, D^2, D^4 of the row's D
    res["kernel"]["GBps_of_compulsory"] = round(compulsory / (res["kernel"]["median_ms"] * 1e-3) / 1e9, 1)
    res["torch_bmm"]["bytes_read"] = n * DIM * DIM * x.element_size() + 2 * n * DIM * x.element_size()
    return {"case": "rotate", "rows": n, "dtype": str(dtype), "compulsory_bytes": compulsory, **res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows-average", type=int, default=100_000)
    ap.add_argument("--rows-rotate", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    from pbc_graph_bench import calibration

    print(json.dumps({"calibration": calibration()}), flush=True)
    for dtype in (torch.float32, torch.float64):
        print(json.dumps(bench_average(a.rows_average, dtype, a.reps, a.warmup)), flush=True)
        print(json.dumps(bench_rotate(a.rows_rotate, dtype, a.reps, a.warmup)), flush=True)


if __name__ == "__main__":
    main()
