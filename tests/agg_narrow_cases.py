"""Cases for the narrowed neighbour sums at the operator level (plan.plan_agg_narrow; matten_tp_fused_narrow's narrow_sum,
narrow_coupling and store_narrow), planned with no model and no GPU: shared by test_agg_narrow_host.py (which template
instances the table reaches, the host walk) and test_gpu_tp_narrow.py (the kernel per narrowed piece against fp64).

An instance is (input l1, lanes per node, D3 = components of the output irrep, mo = output channels of lin2): the kernel's
epilogue is compiled per (lanes, D3), loads and stores 4 x mo bytes, and reaches its walk forms by input l1."""
import functools

import numpy as np

from common import PAPER
from matten_amd import plan as mplan

SH4 = "0e+1o+2e+3o+4e"
PAPER_IN = PAPER["conv_layer_irreps"]
S8_IN = "8x0e+8x0o+16x1o+16x1e"          # scalar blocks of 8 channels: 8-lane scalar entries
_EVERY = ("0e", "0o", "1o", "1e", "2e", "2o", "3o", "3e", "4e", "4o")


def _full(m):
    return "+".join(f"{m}x{ir}" for ir in _EVERY)


def _even(m):
    return f"{m}x0e+{m}x2e+{m}x4e"


# name -> (input irreps, lin2 output irreps, species counts)
CASES = {}
for _m in (1, 2, 4):
    CASES[f"full_{_m}"] = (PAPER_IN, _full(_m), (3, 1, 5) if _m == 2 else (3,))   # 16-lane scalar, 8-lane vector entries; every D3
for _m in (1, 2, 4):
    CASES[f"even_{_m}"] = (PAPER_IN, _even(_m), (3,))        # 16-lane vector entries (alternative kinds); D3 = 1, 5, 9
for _m in (1, 2, 4):
    CASES[f"s8_{_m}"] = (S8_IN, _full(_m), (3,))             # 8-lane scalar entries; every D3
CASES["view"] = (PAPER_IN, "32x0e+4x2e+2x4e", (3,))          # narrowed and un-narrowed couplings in one entry
CASES["head2"] = (PAPER_IN, "2x0e+2x2e+4e", (3,))            # mo 2, 2, 1 in one plan; D3 = 1 with a production head
del _m

PARAMS = [(name, S) for name, (_, _, counts) in CASES.items() for S in counts]

# every instance the planner can emit for sh lmax 4; no irreps found that narrow a 16-lane vector entry at D3 = 3 or 7
# (the alternative kinds that run a vector block at 16 lanes couple it to even output degrees only)
INSTANCES = ({(0, lanes, d3, mo) for lanes in (8, 16) for d3 in (1, 3, 5, 7, 9) for mo in (1, 2, 4)}
             | {(1, 8, d3, mo) for d3 in (1, 3, 5, 7, 9) for mo in (1, 2, 4)}
             | {(1, 16, d3, mo) for d3 in (1, 5, 9) for mo in (1, 2, 4)})
assert len(INSTANCES) == 54


@functools.lru_cache(maxsize=None)
def uvu_plan(name):
    irreps_in, target, _ = CASES[name]
    return mplan.plan_uvu(irreps_in, mplan.Irreps(SH4), target)


@functools.lru_cache(maxsize=None)
def narrow_plan(name, S):
    ap = mplan.plan_agg_narrow(uvu_plan(name), S, CASES[name][1])
    assert ap is not None and ap.narrow is not None, (name, S)
    return ap


def couplings(uvu, ap):
    """(entry, coupling, path, floats between components, first float, mo -- 0: not narrowed) of every coupling of every
    entry: where the piece sits in the row, read from the entry's words alone (plan.narrow_unpack)"""
    out = []
    for e, paths in enumerate(uvu.group_entry_paths):
        for c, pi in sorted(paths.items()):
            ks, o, mo, _ = mplan.narrow_unpack(ap.entries[e][8 + c], ap.entries[e][20 + c])
            out.append((e, c, uvu.paths[pi], ks, o, mo))
    return out


def instances(name, S=3):
    """the (input l1, lanes per node, D3, mo) of the case's narrowed couplings"""
    uvu, ap = uvu_plan(name), narrow_plan(name, S)
    got = set()
    for e, c, pth, _, _, mo in couplings(uvu, ap):
        if mo:
            lanes = 1 << int(ap.entries[e][3])
            assert lanes == int(uvu.group_entry_mul[e]) and pth.l1 == (int(ap.entries[e][0]) & 255) // mplan.TP_KIND_STRIDE
            got.add((pth.l1, lanes, 2 * pth.l3 + 1, mo))
    return got


def assert_every_instance_has_a_case():
    got = set().union(*(instances(name) for name in CASES))
    assert got == INSTANCES, f"instances without a case: {sorted(INSTANCES - got)}; unknown instances: {sorted(got - INSTANCES)}"


def narrow_weights(ap, w):
    """PointConv._pack_narrow_weights: gathered from the flat lin2 weight, scaled in fp32"""
    return (np.asarray(w, dtype=np.float32)[ap.narrow_gather] * ap.narrow_scale).astype(np.float32)


def wtab(ap, w):
    """PointConv._pack_agg_weights with the sentinel: 1.0 where a narrowed coupling wrote lin2's output channel itself"""
    w = np.asarray(w, dtype=np.float32)
    one = (ap.gather == mplan.AGG_GATHER_ONE).astype(np.float32)
    return np.where(ap.gather >= 0, w[np.clip(ap.gather, 0, None)] * ap.scale[None, :].astype(np.float32), one).astype(np.float32)
