"""
The outputs of the tensor-product adjoint kernels (csrc/tp_backward.hip) as .npy files, to compare two builds bit for bit, and
their device-event times.

    python tools/tp_adjoint_ab.py write <dir>            on each build, on the same machine
    python tools/tp_adjoint_ab.py compare <dir a> <dir b>

`write` saves dx and dw of the routes lit-ordered, lit-atomic and wfree-ordered and dY of the route sh (the route names of
tests/test_gpu_tp_adjoint.py) on seeded inputs over that test's `hubs` graph (300 nodes, 5000 edges, two hubs, self-loops), for
the lmax2 and paper irreps, fp32 and bf16 edge storage, the average and the per-node normalisation.  The harmonics are seeded
random numbers: the kernels take any Y.  Then it prints the median device-event time of each route, 20 timed runs after 5
warm-ups, for the two plans (fp32, average normalisation) on a seeded random graph of 293 000 edges over 20 000 nodes.
`compare` wants every array equal, except dx of lit-atomic (the order of its atomics is not fixed): each input block of it
lies within 5e-5 of the block's largest entry (the test's DX_RTOL) of the other directory's lit-ordered dx.  It prints what
differs and exits with the count.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"
AVG = 18.0
DX_RTOL = 5e-5
IRREPS = {"lmax2": ("32x0o+32x0e+16x1o+16x1e+4x2o+4x2e", 2),
          "paper": ("32x0o+32x0e + 16x1o+16x1e + 4x2o+4x2e + 2x3o+2x3e + 2x4e", 4)}
ROUTES = ("lit-ordered", "lit-atomic", "wfree-ordered", "sh")


def hubs(gen):
    """tests/test_gpu_tp_adjoint.py _graph("hubs") -> (edge_index [2, 5000], 300)"""
    import torch
    N = 300
    nodes = torch.randperm(N, generator=gen)
    src_pool, dst_pool, both = torch.cat([nodes[30:40], nodes[50:]]), nodes[40:], nodes[50:]
    pick = lambda pool, n: pool[torch.randint(len(pool), (n,), generator=gen)]
    n_rand, loops = 5000 - 600 - 900 - 40, pick(both, 40)
    src = torch.cat([pick(src_pool, 600), nodes[51].repeat(900), pick(src_pool, n_rand), loops])
    dst = torch.cat([nodes[50].repeat(600), pick(dst_pool, 900), pick(dst_pool, n_rand), loops])
    order = torch.randperm(src.numel(), generator=gen)
    return torch.stack([src[order], dst[order]]), N


class Problem:
    """one plan on one graph: the device operands of every route, seeded"""

    def __init__(self, name, edge_index, N, bf16, per_node, seed):
        import torch
        from matten_amd import ops, plan as mplan
        from matten_amd.nn._tables import DeviceTables
        from matten_amd.o3 import Irreps

        irreps, lmax = IRREPS[name]
        gen = torch.Generator().manual_seed(seed)
        self.p = p = mplan.plan_uvu(irreps, Irreps.spherical_harmonics(lmax), irreps)
        self.t = DeviceTables(bw_blocks=p.bw_blocks, bw_paths=p.bw_paths, bw_w_entries=p.bw_w_entries)
        E, W = edge_index.shape[1], p.weight_numel
        self.E, self.N, self.ld = E, N, (W + 16) // 16 * 16
        self.dtype = torch.bfloat16 if bf16 else torch.float32
        perm, _, self.src, err = ops.csr_build(edge_index.to(DEV), N)
        assert int(err.item()) == 0
        self.dst = edge_index[1].to(DEV)[perm.long()].to(torch.int32).contiguous()
        out_perm, out_ptr, _, _ = ops.csr_build(torch.stack([self.src.long(), self.src.long()]), N)
        self.out_csr = (out_ptr, out_perm)
        rnd = lambda *shape: torch.randn(*shape, generator=gen).to(DEV)
        self.x, self.g, self.Y = rnd(N, p.d_in), rnd(N, p.d_mid), rnd(E, ops.SH_STRIDE)
        self.w = rnd(E, self.ld).to(self.dtype)
        self.h2s = ops.split_hidden(rnd(E, 32))
        W2p = torch.zeros(32, self.ld)
        W2p[:, :W] = torch.randn(32, W, generator=gen) / 32 ** 0.5
        self.frag, self.inv = ops.split_a_tiles_dev(W2p.to(DEV), self.t.get("bw_w_entries", DEV), p.bw_a_tiles)
        self.avg = 0.0 if per_node else AVG
        self.nn = torch.bincount(edge_index[1], minlength=N).float().to(DEV) if per_node else None

    def run(self, route):
        """-> the route's outputs: (dx, dw), or (dY,)"""
        from matten_amd import ops
        p, t = self.p, self.t
        blocks, paths = t.get("bw_blocks", DEV), t.get("bw_paths", DEV)
        if route == "sh":
            return (ops.tp_backward_sh(self.x, self.w, self.src, self.dst, blocks, paths, p.bw_max_mul, self.g, self.avg, self.nn,
                                       max_l=p.bw_max_l),)
        kind, mode = route.split("-")
        common = dict(out_csr=self.out_csr if mode == "ordered" else None, max_l=p.bw_max_l)
        if kind == "lit":
            return ops.tp_backward_lit(self.x, self.w, self.Y, self.src, self.dst, blocks, paths, p.bw_sum_lanes, self.g, self.avg,
                                       self.nn, **common)
        return ops.tp_backward_lit(self.x, None, self.Y, self.src, self.dst, blocks, paths, p.bw_sum_lanes, self.g, self.avg,
                                   self.nn, wfree=(self.h2s, self.frag, self.inv), dw_shape=((self.E, self.ld), self.dtype),
                                   lds_floats=p.bw_wfree_lds_floats, max_mul=p.bw_max_mul, **common)


def write(out):
    import torch
    os.makedirs(out, exist_ok=True)
    seed = 20261019
    for name in IRREPS:
        for bf16 in (False, True):
            for per_node in (False, True):
                seed += 1
                pr = Problem(name, *hubs(torch.Generator().manual_seed(seed)), bf16, per_node, seed)
                key = f"{name}.{'bf16' if bf16 else 'fp32'}.{'node' if per_node else 'avg'}"
                np.save(os.path.join(out, f"{key}.blocks.npy"),
                        np.array([[x0, x0 + mul * (2 * l1 + 1)] for x0, mul, l1, _ in pr.p.bw_blocks.tolist()]))
                for route in ROUTES:
                    for what, v in zip(("dY",) if route == "sh" else ("dx", "dw"), pr.run(route)):
                        np.save(os.path.join(out, f"{key}.{route}.{what}.npy"), v.float().cpu().numpy())
    print(f"tp_adjoint_ab: {len(os.listdir(out))} arrays -> {out}")
    gen = torch.Generator().manual_seed(293)
    edge_index = torch.randint(20_000, (2, 293_000), generator=gen)
    for name in IRREPS:
        pr = Problem(name, edge_index, 20_000, False, False, 293)
        for route in ROUTES:
            for _ in range(5):
                pr.run(route)
            ms = []
            for _ in range(20):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                pr.run(route)
                b.record()
                torch.cuda.synchronize()
                ms.append(a.elapsed_time(b))
            print(f"TP_ADJOINT_MS {name} {route} {float(np.median(ms)):.4f}")
        del pr
    return 0


def compare(a, b):
    names, bad = sorted(os.listdir(a)), 0
    assert names == sorted(os.listdir(b)) and names, "the two directories do not hold the same arrays"
    for name in names:
        x, y = np.load(os.path.join(a, name)), np.load(os.path.join(b, name))
        if name.endswith("lit-atomic.dx.npy"):
            y = np.load(os.path.join(b, name.replace("lit-atomic", "lit-ordered")))
            blocks = np.load(os.path.join(a, name.split(".lit-atomic")[0] + ".blocks.npy"))
            ok = x.shape == y.shape and all(np.abs(x[:, i:j] - y[:, i:j]).max() <= DX_RTOL * np.abs(y[:, i:j]).max() for i, j in blocks)
        else:
            ok = x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x, y, equal_nan=True)
        if not ok:
            bad += 1
            diff = np.nanmax(np.abs(x.astype(np.float64) - y)) if x.shape == y.shape else "shapes differ"
            print(f"DIFFERS {name}: largest difference {diff} (largest entry {np.nanmax(np.abs(x))})")
    print(f"tp_adjoint_ab: {len(names)} arrays, {bad} differ")
    return bad


if __name__ == "__main__":
    sys.exit(write(sys.argv[2]) if sys.argv[1] == "write" else compare(sys.argv[2], sys.argv[3]))
