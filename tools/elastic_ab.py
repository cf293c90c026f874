"""
Every output of the eight `ops.elastic_*` entries as .npy files, to compare two builds of csrc/elastic.hip bit for bit.

    python tools/elastic_ab.py write <dir>            on each build, on the same machine
    python tools/elastic_ab.py compare <dir a> <dir b>

Inputs: the 100 tensors of the example data set, and a seeded synthetic set of 8 with a singular (flagged), an indefinite, a
cubic and a NaN-holding row.  Settings: fp32 and fp64 input in both layouts for the scalar moduli and their adjoint; D in
(1, 65, 300) directions, M in (1, 7) angles, keep=True, for the maps, their adjoints and the refinement with pairs.
`compare` wants every array equal, NaNs in equal places; it prints those that are not and exits with their number.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PAIRS = ((0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1))


def inputs():
    """{set name: (Cartesian [B,81], Voigt [B,36])} in fp64 holding fp32-exact values"""
    raw = json.load(open(os.path.join(ROOT, "tests", "golden", "example_crystal_elasticity_tensor_n100.json")))
    full = np.array([raw["elastic_tensor_full"][k] for k in sorted(raw["elastic_tensor_full"], key=int)], dtype=np.float32)
    rng = np.random.default_rng(20261019)
    Q = np.linalg.qr(rng.standard_normal((8, 6, 6)))[0]
    V = (Q * (10.0 * np.exp(rng.uniform(0.0, 4.0, size=(8, 1, 6))))) @ Q.transpose(0, 2, 1)
    V = 0.5 * (V + V.transpose(0, 2, 1))
    V[0, 5], V[0, :, 5], V[3, 1, 2] = 0.0, 0.0, np.nan                 # row 0 singular, row 3 holds a NaN
    V[1] -= 2.0 * np.linalg.eigvalsh(V[1])[1] * np.eye(6)              # indefinite
    V[2] = 75.0 * np.eye(6)                                            # cubic: C11 = 168, C12 = 121, C44 = 75
    V[2, :3, :3] = 121.0 + 47.0 * np.eye(3)
    V = V.astype(np.float32).astype(np.float64)
    cart = np.zeros((8, 3, 3, 3, 3))
    for I, (i, j) in enumerate(PAIRS):
        for J, (k, l) in enumerate(PAIRS):
            cart[:, i, j, k, l] = cart[:, j, i, k, l] = cart[:, i, j, l, k] = cart[:, j, i, l, k] = V[:, I, J]
    pick = np.stack([[[t[i, j, k, l] for (k, l) in PAIRS] for (i, j) in PAIRS] for t in full.astype(np.float64)])
    return {"n100": (full.reshape(100, 81).astype(np.float64), pick.reshape(100, 36)),
            "synthetic": (cart.reshape(8, 81), V.reshape(8, 36))}


def write(out):
    import torch
    from matten_amd import elastic, ops
    os.makedirs(out, exist_ok=True)
    gen = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *shape: torch.randn(*shape, generator=gen, dtype=torch.float64, device="cuda")

    def save(name, tensors):
        for i, t in enumerate(tensors):
            np.save(os.path.join(out, f"{name}.{i}.npy"), t.cpu().numpy())

    for tag, layouts in inputs().items():
        B = layouts[0].shape[0]
        for layout, c64 in enumerate(layouts):
            for dtype in (torch.float32, torch.float64):
                key = f"{tag}.layout{layout}.{str(dtype)[6:]}"
                p = ops.elastic_props(torch.from_numpy(c64).to("cuda", dtype), layout)
                save(key + ".props", p)
                save(key + ".props_bwd", [ops.elastic_props_bwd(*p, rnd(B, 10), rnd(B, 6, 6), rnd(B, 6, 6), layout, dtype),
                                          ops.elastic_props_bwd(*p, rnd(B, 10), None, None, layout, dtype)])
        voigt, compliance, _, flags = p                                # (Voigt layout, fp64)
        rho = torch.linspace(2000.0, 12000.0, B, dtype=torch.float64).cuda()
        for D in (1, 65, 300):
            dirs = torch.from_numpy(elastic.fibonacci_hemisphere(D)).cuda()
            key = f"{tag}.D{D}"
            d = ops.elastic_directional(compliance, flags, dirs, keep=True)
            a = ops.elastic_acoustic(voigt, flags, rho, dirs, keep=True)
            save(key + ".directional", d)
            save(key + ".acoustic", a)
            gd, ga = rnd(B, 4), rnd(B, 3)                              # with the maps' gradients, and the extremes' alone
            save(key + ".directional_bwd", [ops.elastic_directional_bwd(compliance, flags, dirs, *g, gd, d[3])
                                            for g in ((rnd(B, D), rnd(B, D)), (None, None))])
            save(key + ".acoustic_bwd", [ops.elastic_acoustic_bwd(voigt, flags, rho, dirs, 1e9, g, ga, a[2])
                                         for g in (rnd(B, D, 3), None)])
            for M in (1, 7):
                table = torch.from_numpy(elastic.angle_table(M)).cuda()
                pr = ops.elastic_pair(compliance, flags, dirs, table, keep=True)
                save(f"{key}.M{M}.pair", pr)
                save(f"{key}.M{M}.refine", ops.elastic_refine(compliance, flags, dirs, d[2], d[3], table, pr[1], pr[2]))
    print(f"elastic_ab: {len(os.listdir(out))} arrays -> {out}")


def compare(a, b):
    names, bad = sorted(os.listdir(a)), 0
    assert names == sorted(os.listdir(b)) and names, "the two directories do not hold the same arrays"
    for name in names:
        x, y = np.load(os.path.join(a, name)), np.load(os.path.join(b, name))
        if x.shape != y.shape or x.dtype != y.dtype or not np.array_equal(x, y, equal_nan=x.dtype.kind == "f"):
            bad += 1
            nans = x.shape == y.shape and not (np.isnan(x) ^ np.isnan(y)).any()
            diff = np.nanmax(np.abs(x.astype(np.float64) - y)) if nans else "NaNs or shapes differ"
            print(f"DIFFERS {name}: largest difference {diff} (largest entry {np.nanmax(np.abs(x))})")
    print(f"elastic_ab: {len(names)} arrays, {bad} differ")
    return bad


if __name__ == "__main__":
    sys.exit(write(sys.argv[2]) if sys.argv[1] == "write" else compare(sys.argv[2], sys.argv[3]))
