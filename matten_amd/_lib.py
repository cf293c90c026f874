"""
ctypes binding of libmatten_hip.so (C ABI declared in include/matten_hip.h).

There is no fallback: if the shared library is missing or a symbol is absent, importing the
compute path fails loudly.  Build it with ``python -c "import __graft_entry__ as g; g.build()"``
or ``make -C matten_amd/csrc``.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import c_float, c_int, c_int32, c_int64, c_size_t, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmatten_hip.so")

ABI_VERSION = 47

# name -> (restype, argtypes); must match include/matten_hip.h
P = c_void_p
SIGNATURES = {
    "matten_abi_version": (c_int, []),
    "matten_csr_workspace_bytes": (c_size_t, [c_int64, c_int64]),
    "matten_group_workspace_bytes": (c_size_t, [c_int64, c_int64]),
    "matten_csr_counting_max_avg_degree": (c_int, []),
    "matten_csr_build": (c_int, [P, c_int64, c_int64, P, P, P, P, c_size_t, P, P]),
    "matten_csr_split_bound": (c_int64, [c_int64, c_int64, c_int64]),
    "matten_csr_split": (c_int, [P, c_int64, c_int64, c_int64, P, P, P, P, P]),
    "matten_group_by_key": (c_int, [P, c_int64, c_int64, P, P, P, c_size_t, P, P]),
    "matten_species_embed": (c_int, [P, c_int64, P, c_int64, c_int64, c_int64, P, P, c_int64, P, P, P, P, P, P]),
    "matten_edge_geom": (c_int, [P, P, P, P, c_int64, P, P, c_int64, c_int64, c_int, c_int, c_float, c_float, P, P, c_int, P, P, P, P, P]),
    "matten_radial_mlp": (c_int, [P, c_int64, c_int, c_float, c_float, P, c_int, P, P, c_int, c_int, c_float, P, c_int, P]),
    "matten_radial_mlp_deep": (c_int, [P, c_int64, c_int, c_float, c_float, P, c_int, P, c_int, P, c_int, c_int, c_float, P, c_int,
                                       P]),
    "matten_tp_tile_nodes": (c_int, []),
    "matten_tp_paths": (c_int, [P, c_int64, P, c_int64, P, c_int64, P, P, c_int64, P, P, c_int64, c_int64, c_int64, c_float, P, P, c_int,
                                P]),
    "matten_radial_hidden_multi": (c_int, [P, c_int64, c_int, c_float, c_float, P, c_int, P, c_int, P, P, c_int, P]),
    "matten_radial_hidden_multi_deep": (c_int, [P, c_int64, c_int, c_float, c_float, P, c_int, P, c_int, c_int, P, P, c_int, P]),
    "matten_agg_linear_max_mt": (c_int, []),
    "matten_agg_linear_block_chunks": (c_int, []),
    "matten_agg_linear_lds_bytes": (c_size_t, [c_int64, c_int64, c_int64]),
    "matten_agg_linear_max_lds_bytes": (c_size_t, []),
    "matten_agg_linear": (c_int, [P, c_int64, P, P, c_int64, P, c_int64, P, c_int64, P, c_int64, P, c_int64, c_int64,
                                  c_int64, P, P]),
    "matten_agg_linear_gate": (c_int, [P, c_int64, P, P, c_int64, P, c_int64, P, c_int64, P, c_int64, P, c_int64, c_int64,
                                       c_int64, P, P, P, P, c_int64, P, P]),
    "matten_agg_linear_gate_sets": (c_int, []),
    "matten_radial_hidden": (c_int, [P, c_int64, c_int, c_float, c_float, P, c_int, P, c_int, P, P, P]),
    "matten_radial_hidden_deep": (c_int, [P, c_int64, c_int, c_float, c_float, P, c_int, P, c_int, c_int, P, P, P]),
    "matten_tp_wreg": (c_int, []),
    "matten_tp_max_cols": (c_int, []),
    "matten_tp_max_cols_l0": (c_int, []),
    "matten_tp_max_cols_l1": (c_int, []),
    "matten_tp_groups_hash": (c_int, []),
    "matten_tp_fused": (c_int, [P, c_int64, P, P, c_int64, P, c_int64, P, P, c_int64, P, P, c_int64, c_int64, c_int64, c_int64, c_float, P, P, P, P, P]),
    "matten_tp_fused_narrow": (c_int, [P, c_int64, P, P, c_int64, P, c_int64, P, P, c_int64, P, P, c_int64, c_int64, c_int64, c_int64, c_float, P, P, P, P, P, P]),
    "matten_tp_narrow_max_l1": (c_int, []),
    "matten_species_linear": (c_int, [P, c_int64, P, P, c_int64, P, c_int64, P, c_int64, c_int64, P, c_int64, c_int64, P, P]),
    "matten_species_linear_rows": (c_int, [P, c_int64, P, P, c_int64, P, c_int64, P, c_int64, c_int64, P, c_int64, c_int64, P, P]),
    "matten_radial_mlp_bwd_small_slices": (c_int64, [c_int64]),
    "matten_radial_mlp_bwd_w2_ranges": (c_int64, [c_int64, c_int64]),
    "matten_radial_mlp_bwd_w2_ranges_deep": (c_int64, [c_int64, c_int64, c_int]),
    "matten_radial_mlp_bwd": (c_int, [P, c_int64, c_int, c_float, c_float, P, c_int, P, P, c_int, c_int, c_int, P, c_int64,
                                      c_int, P, P, P, c_float, c_float, c_float, P, P, P]),
    "matten_radial_mlp_bwd_deep": (c_int, [P, c_int64, c_int, c_float, c_float, P, c_int, P, c_int, P, c_int, c_int, c_int, P,
                                           c_int64, c_int, P, P, P, c_float, c_float, c_float, P, P, P]),
    "matten_radial_pack": (c_int, [P, P, P, c_int, c_int, c_int, c_int, c_float, c_float, c_float, P, P, P, P]),
    "matten_radial_pack_deep": (c_int, [P, P, c_int, P, c_int, c_int, c_int, c_int, c_float, c_float, c_float, P, P, P, P]),
    "matten_radial_pack_cols": (c_int, [P, P, P, c_int, c_int, c_int, P, c_int, c_int, c_float, c_float, c_float, P, P, P, P]),
    "matten_radial_pack_cols_deep": (c_int, [P, P, c_int, P, c_int, c_int, c_int, P, c_int, c_int, c_float, c_float, c_float, P, P,
                                             P, P]),
    "matten_radial_h_scale": (c_int, [P, P, c_int, c_float, c_float, c_float, P, P]),
    "matten_radial_h_scale_deep": (c_int, [P, P, c_int, c_int, c_float, c_float, c_float, P, P]),
    "matten_split_a_tiles": (c_int, [P, c_int64, P, c_int64, P, P, P, P]),
    "matten_gather_scale": (c_int, [P, P, P, c_int64, c_int64, c_int, P, P, P, P]),
    "matten_species_linear_walk_all_blocks": (c_int, []),
    "matten_species_linear_lds_w_floats": (c_int64, []),
    "matten_species_linear_rows_lds_bytes": (c_int64, []),
    "matten_species_linear_wgrad_scratch_floats": (c_int64, [c_int64, c_int64, c_int64]),
    "matten_tp_backward": (c_int, [P, c_int64, P, c_int64, P, c_int64, P, P, P, c_int64, P, P, P, c_int64, c_float, P, c_int64, P, P, c_int64,
                                   P, P, c_int64, c_int, P]),
    "matten_tp_backward_lit": (c_int, [P, c_int64, P, c_int64, P, c_int64, P, P, P, c_int64, c_int64, P, c_int64, P, c_int64, c_float,
                                       P, c_int64, P, P, c_int64, c_int, c_int64, P, P, P, c_int, P]),
    "matten_tp_backward_lit_wfree": (c_int, [P, c_int64, P, P, P, P, c_int64, P, P, P, c_int64, c_int64, P, c_int64, P, c_int64, c_float,
                                             P, c_int64, P, P, c_int64, c_int, c_int64, P, P, P, c_int64, c_int, c_int, P]),
    "matten_tp_backward_sh": (c_int, [P, c_int64, P, c_int64, P, P, P, c_int64, c_int64, P, c_int64, P, c_int64, c_float, P, c_int64,
                                      c_int, P, c_int64, c_int, P]),
    "matten_radial_mlp_bwd_len": (c_int, [P, c_int64, c_int, c_float, c_float, P, c_int, P, c_int, P, c_int, c_int, c_int, P,
                                          c_int64, c_int, P, P]),
    "matten_edge_geom_bwd": (c_int, [P, P, c_int64, P, c_int, c_int64, c_int64, P, P, P, P, P, c_int64, P, P, P, P, P]),
    "matten_adam_step": (c_int, [P, P, P, P, c_int64, P, c_float, c_float, c_float, c_float, c_float, P]),
    "matten_adam_ctl_workspace_bytes": (c_size_t, [c_int64]),
    "matten_adam_step_ctl": (c_int, [P, P, P, P, P, c_int64, P, P, P, P, c_size_t, c_float, c_float, c_float, c_float, c_float,
                                     c_float, c_int, c_int, P]),
    "matten_species_linear_wgrad": (c_int, [P, c_int64, P, c_int64, P, P, c_int64, c_int64, P, c_int64, c_int64, P, P, P]),
    "matten_gate_bwd": (c_int, [P, c_int64, P, c_int64, P, P, c_int64, P, P]),
    "matten_bn_scratch_floats": (c_int64, [c_int64, c_int64]),
    "matten_bn_train_fwd": (c_int, [P, c_int64, c_int64, P, P, c_int64, P, P, c_float, P, P, P, P, P, c_float, P, P]),
    "matten_bn_train_bwd": (c_int, [P, P, c_int64, c_int64, P, P, c_int64, P, P, P, c_float, P, P, P, P, P, P, P]),
    "matten_bn_train_fwd_valid": (c_int, [P, c_int64, c_int64, P, P, c_int64, P, P, c_float, P, P, P, P, P, c_float, P, P, P]),
    "matten_bn_train_bwd_valid": (c_int, [P, P, c_int64, c_int64, P, P, c_int64, P, P, P, c_float, P, P, P, P, P, P, P, P]),
    "matten_norm_act": (c_int, [P, c_int64, c_int64, P, c_int64, c_int, c_float, P, P, P, P, c_float, P, P]),
    "matten_norm_act_bwd": (c_int, [P, P, c_int64, c_int64, P, c_int64, c_int, c_float, P, P]),
    "matten_bn_eval_bwd_scratch_floats": (c_int64, [c_int64, c_int64]),
    "matten_gate_bn_eval_bwd": (c_int, [P, c_int64, P, c_int64, P, P, c_int64, P, P, P, c_float, P, c_int64, P, P, P, P, P]),
    "matten_norm_act_bn_eval_bwd": (c_int, [P, P, c_int64, c_int64, P, c_int64, c_int, c_float, P, P, P, c_float, P, P, P, P,
                                            P]),
    "matten_instance_norm_fwd": (c_int, [P, c_int64, c_int64, P, P, c_int64, P, P, c_int64, P, P, c_float, P, P, P, P]),
    "matten_instance_norm_bwd": (c_int, [P, P, c_int64, c_int64, P, P, c_int64, P, P, c_int64, P, P, P, c_float, P, P, P, P]),
    "matten_segment_reduce_bwd": (c_int, [P, c_int64, P, c_int64, c_int, P, P]),
    "matten_graph_prep": (c_int, [P, P, P, c_int64, ctypes.c_double, P, P, P, P, P, P]),
    "matten_graph_prep_pbc": (c_int, [P, P, P, P, c_int64, ctypes.c_double, P, P, P, P, P, P, P, P]),
    "matten_neighbor_rows_count": (c_int, [P, P, P, P, P, P, ctypes.c_double, c_int64, P, P]),
    "matten_neighbor_rows_fill": (c_int, [P, P, P, P, P, P, ctypes.c_double, c_int64, P, c_int64, P, P, P, P]),
    "matten_neighbor_cells_row_capacity": (c_int, []),
    "matten_neighbor_cells_max_axis_bins": (c_int, []),
    "matten_neighbor_cells_grid": (c_int, [P, P, P, P, P, P, c_int64, ctypes.c_double, P, P, P, P]),
    "matten_neighbor_cells_bin": (c_int, [P, P, P, P, P, P, c_int64, P, P, P]),
    "matten_neighbor_cells_scatter": (c_int, [P, P, P, P, c_int64, P, P, P]),
    "matten_neighbor_cells_count": (c_int, [P, P, P, P, P, P, P, P, P, P, P, ctypes.c_double, c_int64, P, P]),
    "matten_neighbor_cells_fill": (c_int, [P, P, P, P, P, P, P, P, P, P, P, ctypes.c_double, c_int64, P, c_int64, P, P, P, P]),
    "matten_neighbor_count": (c_int, [P, P, P, P, P, P, ctypes.c_double, c_int64, c_int64, P, P, P]),
    "matten_neighbor_summary": (c_int, [P, P, c_int64, P, P]),
    "matten_neighbor_fill": (c_int, [P, P, P, P, P, P, ctypes.c_double, c_int64, c_int64, P, c_int64, P, P, P, P, c_int64,
                                     P, P, P, P]),
    "matten_neighbor_scan": (c_int, [P, c_int64, P, P]),
    "matten_neighbor_fill_capped": (c_int, [P, P, P, P, P, P, ctypes.c_double, c_int64, c_int64, P, P, c_int64, P, c_int64,
                                            c_int64, c_int64, P, P, P, P, P, P, P, P, P]),
    "matten_gate_bn": (c_int, [P, c_int64, P, c_int64, P, P, P, P, P, c_float, c_int64, P, P]),
    "matten_segment_reduce": (c_int, [P, c_int64, P, c_int64, c_int, P, P]),
    "matten_segment_minmax": (c_int, [P, c_int64, P, c_int64, c_int, P, P, P]),
    "matten_segment_minmax_bwd": (c_int, [P, c_int64, P, c_int64, P, P]),
    "matten_dense_rows": (c_int, [P, c_int64, P, c_int64, c_int64, P, P]),
    "matten_elastic_props": (c_int, [P, c_int, c_int, c_int64, P, P, P, P, P]),
    "matten_elastic_props_bwd": (c_int, [P, P, P, P, P, P, P, c_int, c_int, c_int64, P, P]),
    "matten_elastic_directional": (c_int, [P, P, P, c_int64, c_int64, P, P, P, P, P]),
    "matten_elastic_pair": (c_int, [P, P, P, P, c_int64, c_int64, c_int64, P, P, P, P]),
    "matten_elastic_acoustic": (c_int, [P, P, P, P, c_int64, c_int64, ctypes.c_double, P, P, P, P, P]),
    "matten_elastic_directional_bwd": (c_int, [P, P, P, c_int64, c_int64, P, P, P, P, P, P]),
    "matten_elastic_acoustic_bwd": (c_int, [P, P, P, P, c_int64, c_int64, ctypes.c_double, P, P, P, P, P]),
    "matten_elastic_refine": (c_int, [P, P, P, P, P, P, P, P, c_int64, c_int64, c_int64, ctypes.c_double, c_int64, P, P, P, P, P,
                                      P]),
    "matten_elastic_kelvin": (c_int, [P, P, c_int64, P, P, P, P]),
    "matten_elastic_kelvin_bwd": (c_int, [P, P, P, c_int64, P, P]),
    "matten_elastic_kelvin_clamp": (c_int, [P, P, P, ctypes.c_double, c_int64, P, P]),
    "matten_elastic_polycrystal": (c_int, [P, P, P, P, c_int64, c_int, ctypes.c_double, c_int, P, P, P, P]),
    "matten_elastic_polycrystal_bwd": (c_int, [P, P, P, P, P, c_int64, P, P]),
    "matten_texture_operator": (c_int, [P, P, P, c_int64, c_int64, ctypes.c_double, c_int64, P, c_int64, P, P, P]),
    "matten_texture_average": (c_int, [P, P, P, P, c_int64, P, P, c_int64, P, P, P, c_int64, P, c_int64, P, P, P]),
    "matten_texture_average_bwd": (c_int, [P, P, c_int64, P, c_int64, P, P, P, c_int64, P, c_int64, P, P, P, P, P, P, c_int64,
                                           P, P]),
    "matten_elastic_waves": (c_int, [P, P, P, P, c_int64, c_int64, ctypes.c_double, ctypes.c_double, P, P, P, P, P, P, P, P]),
    "matten_rank2_props": (c_int, [P, c_int, c_int64, P, P, P, P, P]),
    "matten_rank2_props_bwd": (c_int, [P, P, P, P, P, P, c_int, c_int64, P, P]),
    "matten_wigner_d": (c_int, [P, c_int64, c_int, ctypes.c_double, P, P, P]),
    "matten_irreps_rotate": (c_int, [P, c_int, c_int64, c_int64, P, c_int, P, P, P, c_int64, c_int, P, P]),
    "matten_irreps_average": (c_int, [P, c_int, c_int64, c_int64, P, c_int, P, P, c_int64, P, P, P, c_int, P, P, P]),
    "matten_lattice_group": (c_int, [P, c_int64, ctypes.c_double, P, P, P, P]),
    "matten_crystal_symmetry": (c_int, [P, P, P, P, P, c_int64, c_int64, ctypes.c_double, c_int, P, P, P, P, P, P, P, P, P, P, P,
                                        P, P]),
    "matten_irreps_average_atoms": (c_int, [P, c_int, c_int64, c_int64, P, c_int, P, P, c_int64, c_int64, P, P, P, P, P]),
    "matten_batch_gather_lds_rows": (c_int, []),
    "matten_batch_gather_max_streams": (c_int, []),
    "matten_batch_gather": (c_int, [P, c_int64, P, c_int64, c_int64, c_int64, P]),
    "matten_batch_gather_padded": (c_int, [P, c_int64, P, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64, P, P]),
    "matten_selected_loss_tile_elems": (c_int, []),
    "matten_selected_loss_max_blocks": (c_int, []),
    "matten_selected_loss_workspace_bytes": (c_size_t, [c_int64, c_int64]),
    "matten_selected_loss": (c_int, [P, P, P, c_int64, c_int64, c_int, P, P, P, P, c_size_t, P]),
    "matten_selected_loss_bwd": (c_int, [P, P, P, c_int64, c_int64, c_int, P, P, P, P]),
    "matten_valid_loss_workspace_bytes": (c_size_t, [c_int64, c_int64]),
    "matten_valid_loss": (c_int, [P, P, P, c_int64, c_int64, c_int, P, P, P, P, c_size_t, P]),
    "matten_valid_loss_bwd": (c_int, [P, P, P, c_int64, c_int64, c_int, P, P, P, P]),
}

_lib = None


class MattenHipError(RuntimeError):
    pass


def load() -> ctypes.CDLL:
    """Load (once) and return the library with argtypes set."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MattenHipError(
            f"{LIB_PATH} not found: the HIP extension is not built. matten_amd has no CPU fallback; "
            "run `make -C matten_amd/csrc` (needs hipcc, --offload-arch=gfx950)."
        )
    # One HIP runtime per process.  A torch wheel may ship its own runtime (torch/lib/libamdhip64.so) and ask for it under
    # another name than this library's DT_NEEDED entry (libamdhip64.so.N, found in the ROCm installation).  If this library
    # comes first, torch's copy is mapped as a SECOND runtime beside it, and a kernel registered with one runtime cannot be
    # launched on a stream of the other: every launch fails (MATTEN_ELAUNCH).  With torch loaded first its runtime carries
    # the SONAME this library asks for, and the loader hands it the same one.
    import torch  # noqa: F401

    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise MattenHipError(f"symbol {name} missing from {LIB_PATH}") from e
        fn.restype = res
        fn.argtypes = args
    v = lib.matten_abi_version()
    if v != ABI_VERSION:
        raise MattenHipError(f"ABI version mismatch: library {v}, python binding {ABI_VERSION}")
    _lib = lib
    return lib


_ERRORS = {-1: "MATTEN_EINVAL (bad argument)", -2: "MATTEN_ELAUNCH (HIP launch failed)", -3: "MATTEN_ENOMEM (workspace too small)"}


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise MattenHipError(f"{what} failed: {_ERRORS.get(rc, rc)}")
