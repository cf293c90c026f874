"""
Synthetic workloads named by BASELINE.json / SURVEY.md section 8(d).

fcc-64: 4x4x4 primitive fcc cells (64 atoms), a ~ U[4.20, 4.90] A so that exactly the first two
neighbour shells fall inside the 5 A cutoff (18 neighbours/atom, 1152 edges), Gaussian jitter
sigma = 0.02 A, species i.i.d. from ten fcc metals.  Seeded with numpy default_rng(20250711).

Open and partly periodic inputs (seeded too): ``molecules`` (random clusters with a minimum distance, no lattice),
``fcc_slabs`` (periodic in x and y, open along z), ``fcc_cluster`` (a ball cut from the fcc lattice) and
``fcc_supercell`` (nx x ny x nz conventional cells, optionally sheared: the periodic counterpart) for the large cases of
the pair-free neighbour search.
"""
from typing import Dict, List

import numpy as np
import torch

from .graph import collate, crystal_graph

FCC_METALS = (13, 28, 29, 45, 46, 47, 77, 78, 79, 82)
FCC_SEED = 20250711


def fcc64_structures(n: int, seed: int = FCC_SEED, start: int = 0) -> List[Dict[str, np.ndarray]]:
    """crystals [start, start + n) of the set seeded with `seed` (one sequential random stream: a shard of a larger set
    is the same crystals the whole set would hold at those indices -- SURVEY.md 8d config 5: rank r of an 8-GPU run owns
    crystals [1000 r, 1000 r + 1000) of ONE 8000-crystal set)"""
    rng = np.random.default_rng(seed)
    prim = 0.5 * np.array([[0.0, 1.0, 1.0], [1.0, 0.0, 1.0], [1.0, 1.0, 0.0]])
    grid = np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(4), indexing="ij"), -1).reshape(-1, 3)
    out = []
    for _ in range(start + n):
        a = rng.uniform(4.20, 4.90)
        cell = 4.0 * a * prim
        pos = (grid @ (a * prim)) + rng.normal(0.0, 0.02, size=(64, 3))
        z = rng.choice(FCC_METALS, size=64)
        out.append({"lattice": cell, "cart_coords": pos, "atomic_numbers": z.astype(np.int64)})
    return out[start:]


def fcc64_graphs(n: int, seed: int = FCC_SEED, r_cut: float = 5.0, start: int = 0):
    return [crystal_graph(s["cart_coords"], s["lattice"], s["atomic_numbers"], r_cut)
            for s in fcc64_structures(n, seed, start)]


def fcc64_shard(rank: int, world: int, per_rank: int, r_cut: float = 5.0):
    """The crystals rank `rank` of `world` owns (bench.py, BASELINE configs[2] / configs[4]): one GPU runs the config-3
    set (seed FCC_SEED); N > 1 GPUs shard ONE set of N x per_rank crystals seeded FCC_SEED + 1 contiguously by batch
    index, rank r taking [r per_rank, (r + 1) per_rank)."""
    if world == 1:
        return fcc64_graphs(per_rank, FCC_SEED, r_cut)
    return fcc64_graphs(per_rank, FCC_SEED + 1, r_cut, start=rank * per_rank)


def tile_batch(unique: List[Dict[str, torch.Tensor]], n_total: int) -> List[Dict[str, torch.Tensor]]:
    """Repeat a pool of distinct crystals up to n_total graphs (graph construction is host work outside the timed path)."""
    return [unique[i % len(unique)] for i in range(n_total)]


MOLECULE_SPECIES = (1, 6, 7, 8)
OPEN_SEED = 20261017


def molecules(n: int, seed: int = OPEN_SEED, min_atoms: int = 3, max_atoms: int = 24, min_dist: float = 0.9,
              species=MOLECULE_SPECIES) -> List[Dict[str, np.ndarray]]:
    """n random clusters without a lattice: atoms are added one at a time at 1.0-1.8 A from a random earlier atom and
    kept when no atom is closer than `min_dist` (connected, so every atom has an edge at any cutoff >= 1.8 A)."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        k = int(rng.integers(min_atoms, max_atoms + 1))
        pos = [rng.normal(0.0, 3.0, size=3)]          # anywhere: molecules are not centred on the origin
        while len(pos) < k:
            d = rng.normal(size=3)
            cand = pos[int(rng.integers(len(pos)))] + rng.uniform(1.0, 1.8) * d / np.linalg.norm(d)
            if np.min(np.linalg.norm(np.asarray(pos) - cand, axis=1)) >= min_dist:
                pos.append(cand)
        out.append({"cart_coords": np.asarray(pos), "atomic_numbers": rng.choice(species, size=k).astype(np.int64),
                    "pbc": (False, False, False)})
    return out


def fcc_slabs(n: int, seed: int = OPEN_SEED + 1, layers: int = 3, vacuum_vector: bool = True) -> List[Dict[str, np.ndarray]]:
    """n fcc (001) slabs, 3 x 3 conventional cells wide and `layers` atomic layers thick: periodic in x and y, open
    along z.  The third lattice vector is a (tilted) non-zero vector when `vacuum_vector` -- it must not generate
    images -- and zero otherwise.  Atoms are jittered and not wrapped."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        a = rng.uniform(3.6, 4.2)
        base = np.array([[0.0, 0.0], [0.5, 0.5]])
        pos = []
        for lz in range(layers):
            for ix in range(3):
                for iy in range(3):
                    for k in range(2):
                        x, y = base[k] + (0.5 * (lz % 2), 0.0)
                        pos.append(((ix + x) * a, (iy + y) * a, 0.5 * a * lz))
        pos = np.asarray(pos) + rng.normal(0.0, 0.02, size=(len(pos), 3))
        cell = np.array([[3 * a, 0.0, 0.0], [0.0, 3 * a, 0.0], [0.3 * a, -0.2 * a, 2.0 * a] if vacuum_vector else [0.0] * 3])
        out.append({"lattice": cell, "cart_coords": pos, "atomic_numbers": rng.choice(FCC_METALS, size=len(pos)).astype(np.int64),
                    "pbc": (True, True, False)})
    return out


def fcc_cluster(n_atoms: int, seed: int = OPEN_SEED + 2, a: float = 4.05) -> Dict[str, np.ndarray]:
    """The n_atoms fcc sites closest to the origin (a ball), jittered by 0.02 A: one large open structure, 42 neighbours
    per inner atom (three shells) at a 5 A cutoff."""
    rng = np.random.default_rng(seed)
    m = int(np.ceil((0.75 * n_atoms / np.pi) ** (1.0 / 3.0) / 1.5874)) + 2   # conventional cells per half edge (4 atoms each)
    g = np.arange(-m, m + 1)
    corners = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 1, 3)
    basis = 0.5 * np.array([[0.0, 0, 0], [0, 1, 1], [1, 0, 1], [1, 1, 0]])
    sites = (corners + basis).reshape(-1, 3) * a
    if len(sites) < n_atoms:
        raise ValueError("fcc_cluster: lattice block too small")
    order = np.argsort((sites * sites).sum(1), kind="stable")[:n_atoms]
    pos = sites[np.sort(order)] + rng.normal(0.0, 0.02, size=(n_atoms, 3))
    return {"cart_coords": pos, "atomic_numbers": rng.choice(FCC_METALS, size=n_atoms).astype(np.int64),
            "pbc": (False, False, False)}


def fcc_supercell(nx: int, ny: int, nz: int, a: float = 4.05, seed: int = OPEN_SEED + 3, jitter: float = 0.02,
                  shear=None) -> Dict[str, np.ndarray]:
    """nx x ny x nz conventional fcc cells (4 nx ny nz atoms), jittered by `jitter` A: one periodic structure, the same
    dict as ``fcc_cluster`` plus ``lattice``.  ``shear``: a [3,3] strictly upper-triangular perturbation E of the cell,
    lattice = diag(nx, ny, nz) a (1 + E), applied to the atoms too (a triclinic cell with the same fractional sites)."""
    rng = np.random.default_rng(seed)
    corners = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 1, 3)
    basis = 0.5 * np.array([[0.0, 0, 0], [0, 1, 1], [1, 0, 1], [1, 1, 0]])
    pos = (corners + basis).reshape(-1, 3) * a
    lattice = np.diag([nx * a, ny * a, nz * a]).astype(np.float64)
    if shear is not None:
        strain = np.eye(3) + np.triu(np.asarray(shear, dtype=np.float64).reshape(3, 3), 1)
        pos, lattice = pos @ strain, lattice @ strain
    n = len(pos)
    if jitter:
        pos = pos + rng.normal(0.0, jitter, size=(n, 3))
    return {"lattice": lattice, "cart_coords": pos, "atomic_numbers": rng.choice(FCC_METALS, size=n).astype(np.int64),
            "pbc": (True, True, True)}
