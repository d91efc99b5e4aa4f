"""ctypes binding of `libgcl_hip.so` (C ABI: `include/gcl.h`).

PyTorch tensors are containers only: every wrapper hands raw device pointers, leading dimensions
and the current HIP stream to the library.  There is NO CPU fallback - if the shared library is
missing or a tensor is not on a GPU the call raises.
"""
import ctypes as C
import os
from typing import Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GCL_LIB") or os.path.join(_HERE, "libgcl_hip.so")  # GCL_LIB: A/B builds while tuning

GRAPH_GCN, GRAPH_GAT, GRAPH_MEAN = 0, 1, 2

_lib = None

_i32, _i64, _f32, _vp, _sz = C.c_int32, C.c_int64, C.c_float, C.c_void_p, C.c_size_t

# name -> (restype, argtypes); must list every symbol declared in include/gcl.h
_SIGNATURES = {
    "gcl_version": (C.c_int, []),
    "gcl_last_error": (C.c_char_p, []),
    "gcl_graph_count_edges": (C.c_int, [_vp, _i64, _i32, _i32, C.POINTER(_i64)]),
    "gcl_graph_build_host": (C.c_int, [_vp, _i64, _i32, _i32] + [_vp] * 8),
    "gcl_graph_create": (C.c_int, [_vp, _i64, _i32, _i32, C.POINTER(_vp)]),
    "gcl_graph_destroy": (None, [_vp]),
    "gcl_graph_num_nodes": (_i32, [_vp]),
    "gcl_graph_num_edges": (_i64, [_vp]),
    "gcl_graph_max_in_degree": (_i32, [_vp]),
    "gcl_graph_export_edges": (C.c_int, [_vp, _vp]),
    "gcl_graph_eperm_device": (_vp, [_vp]),
    "gcl_graph_halo_info": (C.c_int, [_vp, _i32, _i32, _vp]),
    "gcl_linear_fwd": (C.c_int, [_vp, _i64, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _i32, _vp]),
    "gcl_linear_bwd_dx": (C.c_int, [_vp, _i64, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _i64, _i32, _i32, _vp, _sz, _vp]),
    "gcl_linear_bwd_dw": (C.c_int, [_vp, _i64, _vp, _i64, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp, _sz, _vp]),
    "gcl_linear_bwd_ws_bytes": (_sz, [_i64, _i32, _i32]),
    "gcl_linear_bwd_all": (C.c_int, [_vp, _i64, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _i32, _i32,
                                     _i32, _vp, _sz, _vp]),
    "gcl_linear_bwd_all_deferred": (C.c_int, [_vp, _i64, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _i32,
                                              _i32, _i32, _vp, _sz, _vp, _vp]),
    "gcl_reduce_jobs": (C.c_int, [_vp, _i32, _vp]),
    "gcl_layernorm_bwd_deferred": (C.c_int, [_vp, _i64, _i64, _vp, _i32, _i32, _vp, _i64, _vp, _vp, _vp, _i64, _vp, _vp, _vp,
                                             _i32, _i64, _i32, _vp, _sz, _vp, _vp]),
    "gcl_colsum_deferred": (C.c_int, [_vp, _i64, _i64, _i32, _vp, _i32, _vp, _sz, _vp, _vp]),
    "gcl_colsum_split_deferred": (C.c_int, [_vp, _i64, _i64, _vp, _i64, _i64, _i32, _i32, _i32, _i32, _vp, _i32, _vp, _sz,
                                            _vp, _vp]),
    "gcl_linear_bwd_dw_deferred": (C.c_int, [_vp, _i64, _vp, _i64, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp, _sz, _vp,
                                             _vp]),
    "gcl_dense_bwd_dw_deferred": (C.c_int, [_vp, _i64, _vp, _i64, _i32, _vp, _vp, _i64, _vp, _i64, _i32, _i32, _i32, _vp,
                                            C.c_size_t, _vp, _vp]),
    "gcl_linear_bwd_all_ws_bytes": (_sz, [_i64, _i32, _i32]),
    "gcl_aggregate": (C.c_int, [_vp, _i32, _vp, _i64, _i64, _vp, _vp, _i64, _i64, _i32, _i32, _vp]),
    "gcl_aggregate_present": (C.c_int, [_vp, _i32, _vp, _i64, _i64, _vp, _vp, _vp, _i64, _i64, _i32, _i32, _vp]),
    "gcl_aggregate_compact_ok": (C.c_int, [_vp, _i32, _i64, _i64, _i64, _i64, _i32, _i32]),
    "gcl_aggregate_compact": (C.c_int, [_vp, _i32, _vp, _i64, _i64, _vp, _vp, _i64, _i64, _vp, _i64, _i64, _i32, _i32, _vp]),
    "gcl_aggregate_heavy_launches": (_i64, []),
    "gcl_aggregate_split": (C.c_int, [_vp, _i32, _vp, _i64, _i64, _vp, _i64, _i64, _i32, _vp, _vp, _i64, _i64, _i32, _i32,
                                      _vp]),
    "gcl_aggregate_head": (C.c_int, [_vp, _i32, _vp, _i64, _i64, _i32, _vp, _vp, _i64, _i64, _i32, _i32, _vp]),
    "gcl_gat_fwd": (C.c_int, [_vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _i32, _i32, _vp]),
    "gcl_gat_bwd": (C.c_int, [_vp, _vp, _i64, _i64, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64,
                              _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _sz, _vp]),
    "gcl_gat_bwd_ws_bytes": (_sz, [_i64, _i32, _i32, _i32, _i32]),
    "gcl_gat_fwd_tab": (C.c_int, [_vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _i32, _i32, _vp]),
    "gcl_gat_bwd_tab": (C.c_int, [_vp, _vp, _i64, _i64, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64,
                                  _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _sz, _vp]),
    "gcl_gat_tab_ok": (C.c_int, [_vp, _i64, _i32, _i32]),
    "gcl_gat_alpha_to_edge_order": (C.c_int, [_vp, _vp, _vp, _i32, _vp]),
    "gcl_gat_prune": (C.c_int, [_vp, _vp, _f32, _vp, C.POINTER(_i64), _vp, _sz, _vp]),
    "gcl_gat_prune_ws_bytes": (_sz, [_i64]),
    "gcl_layernorm_fwd": (C.c_int, [_vp, _i64, _vp, _vp, _f32, _vp, _i64, _vp, _i64, _i32, _vp]),
    "gcl_layernorm_bwd": (C.c_int, [_vp, _i64, _vp, _i64, _vp, _vp, _vp, _i64, _vp, _vp, _i32, _i64, _i32, _vp, _sz, _vp]),
    "gcl_layernorm_bwd_cs": (C.c_int, [_vp, _i64, _vp, _i64, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _i32, _i64, _i32, _vp, _sz, _vp]),
    "gcl_layernorm_bwd_map": (C.c_int, [_vp, _i64, _i64, _vp, _i32, _vp, _i64, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _i32, _i64,
                                        _i32, _vp, _sz, _vp]),
    "gcl_layernorm_fwd_map_skip": (C.c_int, [_vp, _i64, _vp, _vp, _f32, _vp, _i64, _i64, _vp, _i32, _vp, _i32, _vp, _i64, _i32,
                                             _vp]),
    "gcl_layernorm_bwd_map_skip": (C.c_int, [_vp, _i64, _i64, _vp, _i32, _vp, _i64, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _i32,
                                             _i64, _i32, _vp, _sz, _vp]),
    "gcl_layernorm_bwd_ws_bytes": (_sz, [_i64, _i32]),
    "gcl_graphnorm_fwd": (C.c_int, [_vp, _i64, _i64, _vp, _vp, _f32, _vp, _i64, _i64, _vp, _i32, _i32, _i32, _vp, _sz, _vp]),
    "gcl_graphnorm_bwd": (C.c_int, [_vp, _i64, _i64, _vp, _i64, _i64, _vp, _vp, _f32, _vp, _i64, _i64, _vp, _vp,
                                    _i32, _i32, _i32, _i32, _vp, _sz, _vp]),
    "gcl_graphnorm_ws_bytes": (_sz, [_i32, _i32, _i32]),
    "gcl_colsum": (C.c_int, [_vp, _i64, _i64, _i32, _vp, _i32, _vp, _sz, _vp]),
    "gcl_colsum_ws_bytes": (_sz, [_i64, _i32]),
    "gcl_colsum_split": (C.c_int, [_vp, _i64, _i64, _vp, _i64, _i64, _i32, _i32, _i32, _i32, _vp, _i32, _vp, _sz, _vp]),
    "gcl_assemble_input": (C.c_int, [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _vp]),
    "gcl_assemble_input_tail": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _vp]),
    "gcl_wmse_fwd_bwd": (C.c_int, [_vp, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _vp, _vp, _f32, _f32, _vp,
                                   _vp, _vp, _vp, _i32, _i32, _i32, _vp, _sz, _vp]),
    "gcl_wmse_fwd_bwd_ld": (C.c_int, [_vp, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _vp, _vp, _f32, _f32, _vp, _i64, _i64,
                                      _vp, _vp, _vp, _i32, _i32, _i32, _vp, _sz, _vp]),
    "gcl_ar_step_bwd": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _i32, _i32, _i32, _i32, _vp]),
    "gcl_ar_step_bwd_ld": (C.c_int, [_vp, _i64, _i64, _vp, _vp, _vp, _i32, _i32, _vp, _i64, _i64, _vp, _i32, _i32, _i32, _i32,
                                     _vp]),
    "gcl_pad_rows": (C.c_int, [_vp, _i64, _i64, _i32, _i32, _vp, _i64, _i64, _i32, _i32, _i32, _vp]),
    "gcl_zero": (C.c_int, [_vp, _sz, _vp]),
    "gcl_wmse_ws_bytes": (_sz, [_i32, _i32, _i32]),
    "gcl_adam_step": (C.c_int, [_vp, _vp, _vp, _vp, _i64, _f32, _f32, _f32, _f32, _f32, _i32, _f32, _vp]),
    "gcl_adam_step_dev": (C.c_int, [_vp, _vp, _vp, _vp, _i64, _f32, _f32, _f32, _f32, _f32, _vp, _vp, _f32, _vp]),
    "gcl_adam_step_groups": (C.c_int, [_vp, _vp, _vp, _vp, _i64, _vp, _i32, _vp, _vp, _vp, _vp, _f32, _f32, _f32, _f32,
                                       _f32, _vp]),
    "gcl_copy_rows": (C.c_int, [_vp, _i64, _i64, _vp, _i64, _i64, _i32, _i32, _i32, _vp]),
    "gcl_dense_fwd": (C.c_int, [_vp, _i64, _i32, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _i64, _i32, _i32, _vp]),
    "gcl_mlp_fwd_chain_ok": (C.c_int, [_vp, _i64, _i64, _i32, _i32, _i32] + [_vp, _i64, _i32] * 3 + [_vp, _vp, _i64, _vp]),
    "gcl_mlp_fwd_chain": (C.c_int, [_vp, _i64, _i64, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _i64, _i32]
                          + [_vp, _vp, _vp, _vp, _i64, _i32] * 2 + [_vp, _vp, _f32, _vp, _i64, _vp, _vp]),
    "gcl_dense_bwd_dx": (C.c_int, [_vp, _i64, _vp, _i64, _vp, _i64, _i32, _vp, _vp, _vp, _i64, _vp, _i64, _i64, _i32, _i32,
                                   _vp, C.c_size_t, _vp]),
    "gcl_dense_bwd_dw": (C.c_int, [_vp, _i64, _vp, _i64, _i32, _vp, _vp, _i64, _vp, _i64, _i32, _i32, _i32, _vp,
                                   C.c_size_t, _vp]),
    "gcl_gcn_layer_fwd": (C.c_int, [_vp, _vp, _i64, _i64, _i32, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _i32, _i32, _i32, _vp]),
    "gcl_gcn_layer_fwd_rows": (C.c_int, [_vp, _vp, _i64, _i64, _i32, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _i32, _i32, _i32, _i32, _vp]),
    "gcl_gcn_layer_fwd_split": (C.c_int, [_vp, _vp, _i64, _i64, _i32, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _i64, _i64, _i32, _i32, _i32,
                                          _i32, _i32, _vp]),
    "gcl_gcn_layer_fwd_split_ok": (C.c_int, [_vp, _i64, _i64, _i64, _i64, _i64, _i64, _i32, _i32, _i32, _i32, _i32]),
    "gcl_gcn_layer_fwd_present": (C.c_int, [_vp, _vp, _i64, _i64, _i32, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _i32, _i32, _i32, _i32,
                                            _vp]),
    "gcl_layernorm_fwd_map": (C.c_int, [_vp, _i64, _vp, _vp, _f32, _vp, _i64, _i64, _vp, _i32, _vp, _i64, _i32, _vp]),
    "gcl_gcn_layer_fwd_tab": (C.c_int, [_vp, _vp, _i64, _i64, _i64, _vp, _i32, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _i32, _i32, _i32, _vp]),
    "gcl_gcn_layer_fwd_tab_ok": (C.c_int, [_vp, _i64, _i64, _i64, _i32, _i32, _i32]),
    "gcl_segment_reduce": (C.c_int, [_vp, _i64, _i64, _vp, _vp, _i32, _vp, _i64, _i64, _i32, _i32, _i32, _vp]),
    "gcl_edge_combine": (C.c_int, [_vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _i32, _i64, _i32, _vp]),
    "gcl_act_fwd": (C.c_int, [_vp, _vp, _i64, _i32, _vp, _vp]),
    "gcl_act_bwd": (C.c_int, [_vp, _vp, _vp, _i64, _i32, _vp, _vp, _vp, C.c_size_t, _vp]),
    "gcl_act_bwd_ws_bytes": (C.c_size_t, []),
    "gcl_window_pack": (C.c_int, [_vp, _i64, _i32, _i32, _i32, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _i32, _vp]),
    "gcl_ar_advance": (C.c_int, [_vp, _vp, _i64, _i64, _vp, _i64, _i64, _vp, _vp, _vp, _i64, _i64, _i32, _i32, _i32, _i32,
                                 _i32, _i32, _vp]),
    "gcl_gather2_rows": (C.c_int, [_vp, _i64, _i64, _vp, _vp, _i64, _i64, _vp, _vp, _i64, _i64, _i32, _i32, _i32, _i32, _vp]),
    "gcl_roi_gather_rows": (C.c_int, [_vp, _i32, _i32] + [_vp, _i64, _i64, _i32] * 3 + [_vp, _i64, _i64, _i32, _i32, _vp]),
    "gcl_roi_compose": (C.c_int, [_vp, _i64, _i64, _vp, _i64, _i64, _vp, _vp, _i64, _i64, _i32, _i32, _i32, _vp]),
    "gcl_segment_wsum": (C.c_int, [_vp, _i64, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _i64, _i64, _i32,
                                   _i32, _i32, _i32, _vp]),
    "gcl_cross_update_fwd": (C.c_int, [_vp, _i64, _i64, _vp, _i64, _i64, _vp, _vp, _vp, _f32, _vp, _vp, _vp, _i32, _i32,
                                       _i32, _vp]),
    "gcl_nudge": (C.c_int, [_vp, _i64, _i64, _vp, _i64, _i64, _vp, _f32, _f32, _i32, _vp, _i64, _i64, _i32, _i32, _i32,
                            _vp]),
    "gcl_nudge_rows": (C.c_int, [_vp, _i64, _i64, _vp, _i64, _i64, _vp, _i32, _vp, _vp, _vp, _vp, _i64, _i64, _i32, _i32,
                                 _i32, _vp]),
    "gcl_oi_max_stations": (C.c_int, []),
    "gcl_oi_station_cov": (C.c_int, [_vp, _vp, _i32, C.c_double, C.c_double, C.c_double, _vp, _vp]),
    "gcl_oi_factor": (C.c_int, [_vp, _i32, _vp]),
    "gcl_oi_solve": (C.c_int, [_vp, _i32, _vp, _vp, _vp, _i32, _vp]),
    "gcl_oi_innovation": (C.c_int, [_vp, _i64, _i64, _vp, _i64, _i64, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp]),
    "gcl_oi_analysis": (C.c_int, [_vp, _i64, _i64, _vp, _i64, _i64, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp,
                                  _vp, _i32, _f32, _f32, _f32, _f32, _i32, _vp]),
    "gcl_oi_analysis_rows": (C.c_int, [_vp, _i64, _i64, _vp, _i64, _i64, _vp, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _vp,
                                       _vp, _vp, _i32, _vp, _vp, _f32, _f32, _i32, _vp]),
    "gcl_verify_colstats_ws_bytes": (_sz, [_i32, _i32, _i32, _i32]),
    "gcl_verify_colstats": (C.c_int, [_vp, _i64, _i64, _i32, _i32] + [_vp, _i64, _i64, _vp] * 4
                            + [_vp, _i32, _i32, _vp, _vp, _sz, _vp]),
    "gcl_verify_accumulate": (C.c_int, [_vp, _vp, _i32, _vp, _vp, _vp]),
    "gcl_regrid_blend": (C.c_int, [_vp, _i32, _i64, _i64, _i32, _vp, _vp, _i32, _i32, _vp, _i64, _i64, _vp, _vp, _i64,
                                   _i64, _vp, _i64, _i64, _i32, _vp]),
    "gcl_taper_blend": (C.c_int, [_vp, _vp, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _i32, _i32, _i32, _vp]),
    "gcl_mos_forest_eval": (C.c_int, [_vp, _vp, _i32, C.c_double, _vp, _i32, _vp, _vp]),
    "gcl_mos_forest_predict": (C.c_int, [_vp, _vp, _i32, C.c_double, _vp, _i32, _i64, _i64, _i64, _i32] + [_i32] * 5
                               + [_vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _vp]),
    "gcl_mos_idw_apply": (C.c_int, [_vp, _i32, _i64, _i64, _i64, _vp, _i64, _i64, _i64, _i32, _i32, _i32, _i32, _vp,
                                    _vp, _vp, _i32, _vp, _i32, C.c_double, C.c_double, _vp, _i32, _vp]),
    "gcl_mos_idw_sweep_ws_bytes": (_sz, [_i32, _i32, _i32, _i32]),
    "gcl_mos_idw_sweep_max_configs": (C.c_int, []),
    "gcl_mos_idw_sweep": (C.c_int, [_vp, _i32, _i64, _i64, _i64, _vp, _i64, _i64, _i64, _i32, _i32, _i32, _vp, _vp, _vp,
                                    _i32, _vp, _i32, _vp, _vp, _i32, _vp, _i32, _i32, _vp, _vp, _vp, _sz, _i32, _vp]),
    "gcl_mos_table_apply": (C.c_int, [_vp, _i32, _i64, _i64, _i64, _vp, _i64, _i64, _i64, _i32, _i32, _i32, _i32, _vp,
                                      _i32, _i32, _vp]),
    "gcl_mos_fit_ws_bytes": (_sz, [_i32, _i32, _i32, _i32, _i32]),
    "gcl_mos_fit_bin": (C.c_int, [_vp, _i32, _i32, _vp, _vp, _vp, _i64, _vp]),
    "gcl_mos_fit_gradients": (C.c_int, [_vp, _vp, _vp, _i32, _vp]),
    "gcl_mos_fit_histogram": (C.c_int, [_vp, _i64, _i32, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _sz, _vp]),
    "gcl_mos_fit_hist_subtract": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp]),
    "gcl_mos_fit_split": (C.c_int, [_vp, _vp, _i32, _vp, _i32, C.c_double, _i32, C.c_double, _vp, _vp, _vp, _sz, _vp]),
    "gcl_mos_fit_partition": (C.c_int, [_vp, _i64, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _sz, _vp]),
    "gcl_mos_fit_score": (C.c_int, [_vp, _vp, _i32, _vp, _vp, _sz, _vp]),
    "gcl_mos_fit_tree": (C.c_int, [_vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp, _vp, _i32, _i32, _i32,
                                   C.c_double, C.c_double, _i32, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "gcl_multires_window_pack": (C.c_int, [_vp, _i64, _i32, _i32, _i32, _vp, _i64, _i32, _i32, _i32, _vp, _i32, _i32, _vp,
                                           _vp, _vp, _i64, _i64, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _i32,
                                           _vp]),
    "gcl_pipeline_roi_phys": (C.c_int, [_vp, _i64, _vp, _i64, _vp, _i32, _i32, _i32, _vp, _vp, _i32, _i32, C.c_double,
                                        _i32, _vp, _vp, _vp]),
    "gcl_pipeline_lapse": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, C.c_double, _i32, _vp]),
    "gcl_pipeline_lapse_geopotential": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, C.c_double, _vp]),
    "gcl_pipeline_station_obs": (C.c_int, [_vp, _i64, _vp, _i32, _i32, _i32, _vp, _vp]),
    "gcl_pipeline_sqerr": (C.c_int, [_vp, _i64, _i64, _i32, _vp, _i64, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp]),
    "gcl_maps_colstats_ws_bytes": (_sz, [_i32, _i32, _i32]),
    "gcl_maps_colstats": (C.c_int, [_vp, _i64, _i64, _vp, _i64, _i64, _vp, _i32, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _sz,
                                    _vp]),
    "gcl_maps_accumulate": (C.c_int, [_vp, _i64, _i64, _vp, _i64, _i64, _vp, _i32, _i32, _vp, _vp, _vp, _i32, _i32, _vp,
                                      _i32, _vp, _vp, _vp]),
    "gcl_maps_finalize": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i64, _i32, _vp, _vp, _i32, _i32, _vp, _vp]),
    "gcl_maps_convert": (C.c_int, [_vp, _vp, _i64, _i32, _vp, _vp, _vp]),
    "gcl_live_max_dest": (C.c_int, []),
    "gcl_live_frame_pack": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i64, _i32, _i32, _vp]),
    "gcl_live_region_stats": (C.c_int, [_vp, _i64, _i64, _i64, _vp, _i32, _vp, _vp, _i32, _i32, _vp, _i32, _vp]),
    "gcl_dataset_ws_bytes": (_sz, [_i32]),
    "gcl_dataset_max_sources": (C.c_int, []),
    "gcl_dataset_pack": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _i64, _i32, _i64, _vp, _vp, _vp, _sz,
                                   _vp]),
    "gcl_dataset_stats": (C.c_int, [_vp, _i64, _i32, _i32, _i32, _i64, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz,
                                    _vp]),
    "gcl_dataset_welford": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _vp]),
    "gcl_dataset_widen": (C.c_int, [_vp, _i64, _i32, _i32, _i32, _vp, _i32, _vp, _vp]),
    "gcl_wrf_sample": (C.c_int, [_vp, _i32, _i64, _vp, _vp, _vp, _i32, _vp, _vp, _i32, _vp, _vp]),
    "gcl_wrf_scores_ws_bytes": (_sz, [_i32, _i32]),
    "gcl_wrf_scores": (C.c_int, [_vp, _i32, _i64, _vp, _vp, _vp, _i32, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32,
                                 _vp, _i64, _vp, _i32, _vp, _vp, _sz, _vp]),
    "gcl_wrf_box_means": (C.c_int, [_vp, _i64, _i64, _vp, _i32, _vp, _vp, _i32, _i32, _i32, _vp, _i64, _vp, _i64, _vp]),
    "gcl_downscale_coarse": (C.c_int, [_vp, _i64, _i64, _i32, _vp, _vp, _i64, _i64, _i64, _vp, _i64, _i64, _vp]),
    "gcl_downscale_pred": (C.c_int, [_vp, _i64, _i64, _vp, _i64, _i64, _vp, _vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp,
                                     _i64, _vp]),
    "gcl_downscale_batch": (C.c_int, [_vp, _vp, _i64, _i32, _i32, _i32, _vp, _i32, _i32, _vp, _vp, _vp, _i32, _vp, _vp,
                                      _vp, _f32, _vp, _vp, _vp]),
    "gcl_downscale_ws_bytes": (_sz, [_i32]),
    "gcl_downscale_pair_mse": (C.c_int, [_vp, _vp, _i64, _i64, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _sz, _vp]),
    "gcl_downscale_loss_ws_bytes": (_sz, [_i32, _i32, _i32, _i32]),
    "gcl_downscale_loss_fwd_bwd": (C.c_int, [_vp, _vp, _i64, _vp, _vp, _i32, _i32, _i32, _i32, _f32, _f32, _vp, _vp, _vp,
                                             _sz, _vp]),
    "gcl_downscale_spectral_fwd_bwd": (C.c_int, [_vp, _vp, _i64, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _f32, _i32,
                                                 _vp, _vp, _vp, _sz, _vp]),
    "gcl_downscale_metrics": (C.c_int, [_vp, _vp, _i64, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _sz, _vp]),
    "gcl_downscale_loss_scale": (C.c_int, [_vp, _vp, _i64, _vp, _vp]),
    "gcl_eval_colstats_ws_bytes": (_sz, [_i32, _i32, _i32]),
    "gcl_eval_colstats": (C.c_int, [_vp, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _vp, _vp, _i32, _vp, _i64, _i64,
                                    _vp, _i32, _i32, _i32, _vp, _sz, _vp]),
    "gcl_eval_accumulate": (C.c_int, [_vp, _vp, _vp, C.c_double, _i32, _i32, _i32, _vp, _vp]),
    "gcl_tensor_batch_pack": (C.c_int, [_vp, _i32, _i32, _vp, _i32, _i32, _i64, _i32, _i32, _i32, _vp, _i32, _vp, _i64,
                                        _i64, _vp, _i64, _i64, _vp]),
    "gcl_region_cache_record_bytes": (_sz, [_i32] * 7),
    "gcl_region_cache_store": (C.c_int, [_vp, _i64, _i64] * 5 + [_vp, _vp, _vp, _vp, _i64] + [_i32] * 10 + [_vp]),
    "gcl_region_cache_fetch": (C.c_int, [_vp, _i64, _vp] + [_i32] * 8 + [_vp, _i64] * 4 + [_vp]),
    "gcl_region_eval_pair_ws_bytes": (_sz, [_i32] * 4),
    "gcl_region_eval_pair": (C.c_int, [_i32] + [_vp, _i64, _i64, _vp, _i64, _i64, _vp, _vp, _i64, _i64] * 2
                             + [_vp, _i64, _i64, _vp, _i32, _vp, _i32, C.c_double, _vp, _i32, _i32, _i32, _i32, _vp, _sz,
                                _vp]),
    "gcl_obs_pack": (C.c_int, [_vp, _i64, _i64, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _i64, _i64, _vp]),
    "gcl_region_interp_scores_ws_bytes": (_sz, [_i32] * 4),
    "gcl_region_interp_scores": (C.c_int, [_vp, _i64, _i64, _i32, _i32, _vp, _vp, _vp, _i32, _i32, _vp, _i32, _vp, _vp,
                                           _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _sz, _vp]),
    "gcl_unet_packed_floats": (_i64, [_i32, _i32]),
    "gcl_unet_pack_weights": (C.c_int, [_vp, _i32, _i32, _vp, _vp]),
    "gcl_unet_conv3x3": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _f32, _vp, _i32, _i32, _i32, _i32, _i32, _vp]),
    "gcl_unet_conv1x1_out": (C.c_int, [_vp, _vp, _vp, _vp, _i64, _vp, _i32, _i32, _i32, _i32, _i32, _vp]),
    "gcl_unet_launches": (_i64, []),
    "gcl_cascade_pack": (C.c_int, [_vp] * 8 + [_i32] * 6 + [_vp]),
    "gcl_cascade_scores_ws_bytes": (_sz, [_i32] * 4),
    "gcl_cascade_scores": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp] + [_i32] * 6 + [_vp, _sz, _vp]),
    "gcl_unet_train_launches": (_i64, []),
    "gcl_unet_colsum_ws_bytes": (_sz, [_i64, _i64]),
    "gcl_unet_bn_stats": (C.c_int, [_vp, _i64, _i32, _f32, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "gcl_unet_bn_gelu": (C.c_int, [_vp] * 6 + [_i64, _i32, _vp]),
    "gcl_unet_bn_gelu_bwd": (C.c_int, [_vp] * 9 + [_i64, _i32, _vp, _sz, _vp]),
    "gcl_unet_wgrad_chunks": (_i32, [_i32] * 5),
    "gcl_unet_wgrad_ws_bytes": (_sz, [_i32] * 5),
    "gcl_unet_conv3x3_wgrad": (C.c_int, [_vp, _vp, _vp] + [_i32] * 5 + [_vp, _sz, _vp]),
    "gcl_unet_pack_weights_dgrad": (C.c_int, [_vp, _i32, _i32, _vp, _vp]),
    "gcl_unet_pool_bwd": (C.c_int, [_vp, _vp, _vp, _i64, _vp, _i32, _i32, _i32, _i32, _vp]),
    "gcl_unet_upsample_bwd": (C.c_int, [_vp, _i64, _i32, _vp] + [_i32] * 6 + [_vp]),
    "gcl_unet_conv1x1_out_bwd_ws_bytes": (_sz, [_i32] * 5),
    "gcl_unet_conv1x1_out_bwd": (C.c_int, [_vp] * 6 + [_i32] * 5 + [_vp, _sz, _vp]),
    "gcl_unet_v2_launches": (_i64, []),
    "gcl_unet_v2_gn_stats": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _f32, _vp, _vp, _vp]),
    "gcl_unet_v2_gn_gelu": (C.c_int, [_vp] * 6 + [_i32] * 4 + [_vp]),
    "gcl_unet_v2_conv1x1": (C.c_int, [_vp] * 5 + [_i64] + [_i32] * 5 + [_vp]),
    "gcl_unet_v2_tail_chunks": (_i32, [_i32]),
    "gcl_unet_v2_tail_ws_bytes": (_sz, [_i32] * 3),
    "gcl_unet_v2_block_tail": (C.c_int, [_vp] * 11 + [_i32] * 5 + [_vp, _sz, _vp]),
    "gcl_unet_v2_layernorm": (C.c_int, [_vp, _vp, _vp, _f32, _vp, _i64, _i32, _vp]),
    "gcl_unet_v2_attention": (C.c_int, [_vp, _vp] + [_i32] * 4 + [_vp]),
    "gcl_unet_v2_spectral_pack": (C.c_int, [_vp, _vp] + [_i32] * 6 + [_vp, _vp]),
    "gcl_unet_v2_spectral_fwd": (C.c_int, [_vp, _vp] + [_i32] * 6 + [_vp]),
    "gcl_unet_v2_spectral_mix": (C.c_int, [_vp] * 3 + [_i32] * 4 + [_vp]),
    "gcl_unet_v2_spectral_inv": (C.c_int, [_vp, _vp, _i64] + [_i32] * 6 + [_vp]),
    "gcl_unet_forecast_launches": (_i64, []),
    "gcl_grid_window_pack": (C.c_int, [_vp, _i64, _i32, _i32, _i32, _vp, _vp, _vp, _i32, _i32, _vp, _i32, _vp]),
    "gcl_grid_forecast_step_ws_bytes": (_sz, [_i32] * 4),
    "gcl_grid_forecast_step": (C.c_int, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp, _vp, _vp, _vp] + [_i32] * 4
                               + [_vp] * 5 + [_i32, _vp, _sz, _vp]),
}


def exported_symbols():
    return sorted(_SIGNATURES)


def lib():
    """The loaded shared library; raises loudly when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or `make -C graphcast-lite_amd/csrc`). The HIP path has no CPU fallback."
            )
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def _check(rc: int):
    if rc != 0:
        raise RuntimeError(f"libgcl_hip error {rc}: {lib().gcl_last_error().decode()}")


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[torch.Tensor]):
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("libgcl_hip needs GPU tensors (there is no CPU fallback)")
    if t.dtype != torch.float32:
        raise RuntimeError(f"libgcl_hip needs float32 tensors, got {t.dtype}")
    return t.data_ptr()


_ws = {}
_ws_retired = []  # outgrown buffers stay allocated: kernels inside a captured hipGraph may still point at them


def workspace(nbytes: int, device) -> torch.Tensor:
    """Grow-only per-device scratch buffer (uint8).  Grows geometrically and never frees the buffers
    it outgrows (a replayed hipGraph keeps using the one that was current at capture time)."""
    key = torch.device(device).index if torch.device(device).index is not None else torch.cuda.current_device()
    cur = _ws.get(key)
    if cur is None or cur.numel() < nbytes:
        size = max(int(nbytes), 1 << 20, 2 * cur.numel() if cur is not None else 0)
        if cur is not None:
            _ws_retired.append(cur)
        cur = torch.empty(size, dtype=torch.uint8, device=f"cuda:{key}")
        _ws[key] = cur
    return cur


def rows2d(t: torch.Tensor) -> torch.Tensor:
    """View `[..., F]` as `[rows, F]` with a single row stride; copies only if it must."""
    if t.dim() == 2 and t.stride(1) == 1:
        return t
    if not t.is_contiguous():
        t = t.contiguous()
    return t.view(-1, t.shape[-1])


class Graph:
    """Device CSR (+transpose) of a reference-layout `edge_index` (int64 `[2,E]`, CPU or GPU)."""

    def __init__(self, edge_index: torch.Tensor, num_nodes: int, kind: int):
        ei = edge_index.detach().to("cpu", torch.int64).contiguous()
        if ei.dim() != 2 or ei.shape[0] != 2:
            raise ValueError(f"edge_index must be [2, E], got {tuple(ei.shape)}")
        self.kind = kind
        self._h = _vp()
        _check(lib().gcl_graph_create(ei.data_ptr(), ei.shape[1], int(num_nodes), kind, C.byref(self._h)))
        self.n = int(num_nodes)
        self.e = int(lib().gcl_graph_num_edges(self._h))
        self.max_in_degree = int(lib().gcl_graph_max_in_degree(self._h))
        # PyG-order edge list with loops, as a tensor with a STABLE identity: when the input already
        # is that list (SparseGATConv feeds its own output back, src/models.py:846) the input tensor
        # itself is returned, so the CSR cache keeps hitting instead of rebuilding every step.
        self._exported = {}
        if ei.shape[1] == self.e and torch.equal(self.export_edges(), ei):
            self._exported[str(edge_index.device)] = edge_index

    @property
    def handle(self):
        return self._h

    def export_edges(self) -> torch.Tensor:
        out = torch.empty(2, self.e, dtype=torch.int64)
        _check(lib().gcl_graph_export_edges(self._h, out.data_ptr()))
        return out

    def halo_info(self, transpose: bool = False, T: int = 64):
        """(T, tiles, staged-source stride) of the source-tile layout, or None when it was not built."""
        out = (C.c_int32 * 4)()
        _check(lib().gcl_graph_halo_info(self._h, 1 if transpose else 0, T, out))
        return (out[0], out[1], out[2]) if out[0] else None

    def row_group_order(self, transpose: bool = False) -> bool:
        """Do the per-edge aggregation kernels of this direction walk 16-row groups in a processing order (order16)?"""
        out = (C.c_int32 * 4)()
        _check(lib().gcl_graph_halo_info(self._h, 1 if transpose else 0, 64, out))
        return bool(out[3])

    def edges_with_loops(self, device) -> torch.Tensor:
        key = str(torch.device(device))
        t = self._exported.get(key)
        if t is None:
            t = self.export_edges().to(device)
            self._exported[key] = t
        return t

    def __del__(self):
        try:
            if self._h:
                lib().gcl_graph_destroy(self._h)
                self._h = _vp()
        except Exception:
            pass


def build_csr_host(edge_index: torch.Tensor, num_nodes: int, kind: int):
    """CPU-only CSR construction (no GPU needed) - returns a dict of torch CPU tensors."""
    ei = edge_index.detach().to("cpu", torch.int64).contiguous()
    e_out = _i64(0)
    _check(lib().gcl_graph_count_edges(ei.data_ptr(), ei.shape[1], int(num_nodes), kind, C.byref(e_out)))
    Ep, n = e_out.value, int(num_nodes)
    i32 = lambda k: torch.zeros(max(k, 1), dtype=torch.int32)
    f32 = lambda k: torch.zeros(max(k, 1), dtype=torch.float32)
    out = dict(rowptr=i32(n + 1), col=i32(Ep), w=f32(Ep), eperm=i32(Ep), trowptr=i32(n + 1), tcol=i32(Ep),
               tw=f32(Ep), tslot=i32(Ep))
    _check(lib().gcl_graph_build_host(
        ei.data_ptr(), ei.shape[1], n, kind, out["rowptr"].data_ptr(), out["col"].data_ptr(), out["w"].data_ptr(),
        out["eperm"].data_ptr(), out["trowptr"].data_ptr(), out["tcol"].data_ptr(), out["tw"].data_ptr(),
        out["tslot"].data_ptr()))
    for k in ("col", "w", "eperm", "tcol", "tw", "tslot"):
        out[k] = out[k][:Ep]
    out["num_edges"] = Ep
    return out


# ------------------------------------------------------------------------------------------------
# raw wrappers (no autograd).  2-D tensors are [rows, F] with stride (ld, 1).
# ------------------------------------------------------------------------------------------------
def _ld(t: torch.Tensor) -> int:
    assert t.dim() == 2 and t.stride(1) == 1, "expected a [rows, F] view with unit channel stride"
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])


def _act_of(act, slope):
    return (ACT_PRELU if slope is not None else ACT_NONE) if act is None else int(act)


def linear_fwd(x, W, bias, in_slope, out=None, ld_out=None, act=None):
    """y = act(x) W^T + bias; act None: PReLU when in_slope is given, else identity."""
    rows, Fin = x.shape
    Fout = W.shape[0]
    if out is None:
        ld = ld_out or Fout
        out = torch.empty(rows, ld, dtype=torch.float32, device=x.device)[:, :Fout]
    if rows == 0:
        return out
    _check(lib().gcl_dense_fwd(_p(x), _ld(x), _act_of(act, in_slope), _p(in_slope), _p(W), W.stride(0), _p(bias), None, 0,
                               _p(out), _ld(out), rows, Fin, Fout, _stream()))
    return out


def mlp_fwd_chain(x, Ws, bs, slopes, in_slope=None, ln=None):
    """2 or 3 consecutive Linear layers in one launch: z_0 = act(x) W_0^T + b_0 (PReLU when in_slope is given, else
    identity), z_k = prelu(z_{k-1}; slopes[k-1]) W_k^T + b_k.  ln = (gamma, beta, eps): the node LayerNorm behind the last
    layer.  Returns ([z_0, ..], y, stats) - the tensors, bit for bit, that linear_fwd gives layer by layer and
    layernorm_fwd gives for the last of them; y and stats are None when no LayerNorm was asked for or the kernel does
    not take it with this run (the caller then launches it) - or None when the run is not one the chained kernel takes
    (gcl_mlp_fwd_chain_ok; GCL_MLP_CHAIN=0 turns it off): the caller then launches the layers one by one."""
    n = len(Ws)
    rows, Fin = x.shape
    if n < 2 or n > 3 or rows == 0 or len(slopes) != n - 1 or any(W.stride(0) != W.shape[1] or W.stride(1) != 1 for W in Ws):
        return None
    if Fin > 64 or any(W.shape[0] > 64 for W in Ws):  # no output tensors for a wide MLP, which the kernel never takes
        return None
    zs = [torch.empty(rows, W.shape[0], dtype=torch.float32, device=x.device) for W in Ws]
    act0 = ACT_PRELU if in_slope is not None else ACT_NONE
    zargs = []
    for z in zs + [None] * (3 - n):
        zargs += [_p(z), z.shape[1] if z is not None else 0, z.shape[1] if z is not None else 0]
    y = stats = None
    if ln is not None:
        y = torch.empty(rows, Ws[-1].shape[0], dtype=torch.float32, device=x.device)
        stats = torch.empty(rows, 2, dtype=torch.float32, device=x.device)
        if not lib().gcl_mlp_fwd_chain_ok(_p(x), _ld(x), rows, Fin, act0, n, *zargs, _p(ln[0]), _p(y), y.shape[1], _p(stats)):
            ln = y = stats = None
    if ln is None and not lib().gcl_mlp_fwd_chain_ok(_p(x), _ld(x), rows, Fin, act0, n, *zargs, None, None, 0, None):
        return None
    largs = [_p(Ws[0]), _p(bs[0])] + zargs[0:3]
    for k in (1, 2):
        if k < n:
            largs += [_p(Ws[k]), _p(bs[k]), _p(slopes[k - 1])] + zargs[3 * k: 3 * k + 3]
        else:
            largs += [None, None, None, None, 0, 0]
    if ln is not None:
        largs += [_p(ln[0]), _p(ln[1]), float(ln[2]), _p(y), y.shape[1], _p(stats)]
    else:
        largs += [None, None, 0.0, None, 0, None]
    _check(lib().gcl_mlp_fwd_chain(_p(x), _ld(x), rows, Fin, act0, _p(in_slope), n, *largs, _stream()))
    return zs, y, stats


def linear_bwd_dx(dy, W, x, in_slope, d_in_slope, act=None):
    a = _act_of(act, in_slope)
    return dense_bwd_dx(dy, W, x if a != ACT_NONE else None, a, in_slope, d_in_slope)


def linear_bwd_dw(dy, x, in_slope, dW, db, accumulate: bool, act=None):
    dense_bwd_dw(dy, x, dW, db, accumulate, _act_of(act, in_slope), in_slope)


ACT_NONE, ACT_PRELU, ACT_SILU = 0, 1, 2


# Optional launch probe (None in the product): measurement code (bench.py) may install an object with
# `begin(kind, **info) -> token | None` and `end(token)`; the wrappers of the roofline kernels call it around
# their launch so that HIP events can be recorded on the launch stream without any profiling state here.
PROBE = None


def _probe_begin(kind, **info):
    return PROBE.begin(kind, **info) if PROBE is not None else None


def _probe_end(tok):
    if tok is not None:
        PROBE.end(tok)


def dense_fwd(x, W, bias, act=ACT_NONE, slope=None, addend=None, out=None):
    """y = act(x) W^T + bias + addend.  x / W / addend / out may be column blocks (unit channel
    stride, any row stride) of wider tensors."""
    rows, Fin = x.shape
    Fout = W.shape[0]
    assert W.shape[1] == Fin and W.stride(1) == 1 and x.stride(1) == 1
    if out is None:
        out = torch.empty(rows, Fout, dtype=torch.float32, device=x.device)
    if rows == 0:  # an empty batch of rows: nothing to launch (empty tensors have no device pointer)
        return out
    tok = _probe_begin("dense_fwd", rows=rows, Fin=Fin, Fout=Fout)
    _check(lib().gcl_dense_fwd(_p(x), _ld(x), int(act), _p(slope), _p(W), W.stride(0), _p(bias), _p(addend),
                               _ld(addend) if addend is not None else 0, _p(out), _ld(out), rows, Fin, Fout, _stream()))
    _probe_end(tok)
    return out


def dense_bwd_dx(dy, W, z=None, act=ACT_NONE, slope=None, d_slope=None, addend=None, out=None):
    """dx = (dy W) * act'(z) + addend."""
    rows, Fout = dy.shape
    Fin = W.shape[1]
    assert W.shape[0] == Fout and W.stride(1) == 1
    if out is None:
        out = torch.empty(rows, Fin, dtype=torch.float32, device=dy.device)
    if rows == 0:
        return out
    nb = lib().gcl_linear_bwd_ws_bytes(rows, Fin, Fout)
    ws = workspace(nb, dy.device)
    _check(lib().gcl_dense_bwd_dx(_p(dy), _ld(dy), _p(W), W.stride(0), _p(z), _ld(z) if z is not None else 0, int(act),
                                  _p(slope), _p(d_slope), _p(addend), _ld(addend) if addend is not None else 0, _p(out),
                                  _ld(out), rows, Fin, Fout, ws.data_ptr(), ws.numel(), _stream()))
    return out


def dense_bwd_dw(dy, x, dW, db, accumulate: bool, act=ACT_NONE, slope=None):
    """dW (+)= dy^T act(x) (dW may be a column block of a wider gradient), db (+)= colsum(dy)."""
    rows, Fout = dy.shape
    Fin = x.shape[1]
    assert tuple(dW.shape) == (Fout, Fin) and dW.stride(1) == 1
    if rows == 0:  # the sum over no rows: zero unless accumulating
        if not accumulate:
            dW.zero_()
            if db is not None:
                db.zero_()
        return
    nb = lib().gcl_linear_bwd_ws_bytes(rows, Fin, Fout)
    if _deferred.active:
        _queue(nb, dy.device, (dW, db), 2, lambda ws, jobs: lib().gcl_dense_bwd_dw_deferred(
            _p(dy), _ld(dy), _p(x), _ld(x), int(act), _p(slope), _p(dW), dW.stride(0), _p(db), rows, Fin, Fout,
            1 if accumulate else 0, ws.data_ptr(), ws.numel(), _stream(), C.cast(jobs, C.c_void_p)))
        return
    ws = workspace(nb, dy.device)
    _check(lib().gcl_dense_bwd_dw(_p(dy), _ld(dy), _p(x), _ld(x), int(act), _p(slope), _p(dW), dW.stride(0), _p(db), rows,
                                  Fin, Fout, 1 if accumulate else 0, ws.data_ptr(), ws.numel(), _stream()))


ACC_DW, ACC_DB, ACC_COLSUM = 1, 2, 4  # GCL_ACC_* bits of gcl_linear_bwd_all


class _RedSeg(C.Structure):
    _fields_ = [("out", C.c_void_p), ("poff", C.c_int32), ("count", C.c_int32), ("pld", C.c_int32), ("cols", C.c_int32),
                ("ldo", C.c_int32), ("acc", C.c_int32)]


class ReduceJob(C.Structure):
    """Mirror of gcl_reduce_job (include/gcl.h)."""
    _fields_ = [("part", C.c_void_p), ("pstride", C.c_int64), ("seg", _RedSeg * 3), ("spart", C.c_void_p),
                ("sout", C.c_void_p), ("nparts", C.c_int32), ("ns", C.c_int32)]


class _Deferred:
    """Pending final passes of the calls that end in a sum over per-block partial records (the fused dense backward, the
    dW kernel, the LayerNorm backward, the column sums: gcl_*_deferred): a training step opens the queue before its
    backward and flushes it once afterwards - one launch per 24 calls instead of one per call.
    Every pending call owns a workspace from a pool that persists across steps (a replayed hipGraph keeps using it)."""

    def __init__(self):
        self.active = False
        self.jobs, self.dests, self.pool, self.used = [], set(), [], 0
        # the queued job only carries raw pointers: the destination (and slope-gradient) tensors are held here until
        # the flush, so a temporary one (the gradient slot of a frozen parameter) cannot be freed and its block handed
        # to another tensor before the final pass writes it
        self.keep = []

    def ws(self, nbytes, device):
        if self.used == len(self.pool):
            self.pool.append(None)
        cur = self.pool[self.used]
        if cur is None or cur.numel() < nbytes or cur.device != torch.device(device):
            if cur is not None:
                _ws_retired.append(cur)
            cur = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
            self.pool[self.used] = cur
        self.used += 1
        return cur


_deferred = _Deferred()


def defer_begin():
    """Open the deferred-reduction queue (idempotent); pair with defer_flush()."""
    _deferred.active = True


def defer_flush(close: bool = True, drop: bool = False):
    """Run the pending final passes (gcl_reduce_jobs) on the current stream.  `drop` discards them instead (the
    backward that queued them failed).  The queue is emptied whatever happens, so a failed launch cannot leave
    later, unrelated backward calls queueing into a list nobody flushes."""
    d = _deferred
    try:
        if d.jobs and not drop:
            arr = (ReduceJob * len(d.jobs))(*d.jobs)
            _check(lib().gcl_reduce_jobs(C.cast(arr, C.c_void_p), len(d.jobs), _stream()))
    finally:
        d.jobs, d.dests, d.used, d.keep = [], set(), 0, []
        if close:
            d.active = False


def _queue(nbytes, device, dests, njobs, call):
    """Make one deferred call with the queue open: `call(ws, jobs)` runs the main kernel with a workspace of the pool
    (not the shared scratch buffer, which the next call overwrites) and fills `jobs`; what it left to do is queued.
    Two pending passes must not write the same destination (a layer that runs twice in one backward, e.g. an
    autoregressive rollout): what is queued is flushed first."""
    d = _deferred
    ptrs = {t.data_ptr() for t in dests if t is not None}
    if ptrs & d.dests:
        defer_flush(close=False)
    ws = d.ws(nbytes, device)
    jobs = (ReduceJob * njobs)()
    try:
        _check(call(ws, jobs))
    except BaseException:
        d.used -= 1
        raise
    pending = [j for j in jobs if j.nparts > 0]
    if pending:
        d.jobs.extend(pending)
        d.dests |= ptrs
        d.keep.append(tuple(dests) + (ws, jobs))
    else:
        d.used -= 1  # reduced on the spot: the workspace slot is free again


def linear_bwd_all(dy, W, x, in_slope, d_in_slope, dW, db, colsum_dx, acc_dW: bool, acc_db=None, acc_colsum=None,
                   act=None):
    """dx (pre-activation gradient) + dW (+ db, slope gradient, column sums of dx) in one call.
    Each destination has its own accumulate flag (acc_db / acc_colsum default to acc_dW): dW, db and
    colsum_dx are gradients of different parameters."""
    acc_db = acc_dW if acc_db is None else acc_db
    acc_colsum = acc_dW if acc_colsum is None else acc_colsum
    a = _act_of(act, in_slope)
    if a == ACT_SILU:  # the fused kernel knows PReLU only
        if db is not None and bool(acc_db) != bool(acc_dW):
            dense_bwd_dw(dy, x, dW, None, acc_dW, a, None)
            colsum(dy, db, acc_db)
        else:
            dense_bwd_dw(dy, x, dW, db, acc_dW, a, None)
        dx = dense_bwd_dx(dy, W, x, a, None, None)
        if colsum_dx is not None:
            colsum(dx, colsum_dx, acc_colsum)
        return dx
    rows, Fout = dy.shape
    Fin = W.shape[1]
    dx = torch.empty(rows, Fin, dtype=torch.float32, device=dy.device)
    nb = lib().gcl_linear_bwd_all_ws_bytes(rows, Fin, Fout)
    acc = (ACC_DW if acc_dW else 0) | (ACC_DB if acc_db else 0) | (ACC_COLSUM if acc_colsum else 0)
    d = _deferred
    if d.active:
        # two pending passes must not write the same destination (a layer that runs twice in one backward, e.g. an
        # autoregressive rollout): flush what is queued first
        dests = {t.data_ptr() for t in (dW, db, colsum_dx) if t is not None}
        if dests & d.dests:
            defer_flush(close=False)
        ws = d.ws(nb, dy.device)
        job = ReduceJob()
        _check(lib().gcl_linear_bwd_all_deferred(
            _p(dy), _ld(dy), _p(W), _p(x), _ld(x), _p(in_slope), _p(d_in_slope), _p(dx), Fin, _p(dW), _p(db),
            _p(colsum_dx), rows, Fin, Fout, acc, ws.data_ptr(), ws.numel(), _stream(), C.byref(job)))
        if job.nparts > 0:
            d.jobs.append(job)
            d.dests |= dests
            d.keep.append((dW, db, colsum_dx, d_in_slope, ws))
        else:
            d.used -= 1  # reduced on the spot: the workspace slot is free again
        return dx
    ws = workspace(nb, dy.device)
    _check(lib().gcl_linear_bwd_all(
        _p(dy), _ld(dy), _p(W), _p(x), _ld(x), _p(in_slope), _p(d_in_slope), _p(dx), Fin, _p(dW), _p(db),
        _p(colsum_dx), rows, Fin, Fout, acc, ws.data_ptr(), ws.numel(), _stream()))
    return dx


AGG_HEAVY_INSIDE = 2  # gcl.h GCL_AGG_HEAVY_INSIDE


def _agg_flags(transpose) -> int:
    """The flag word of the aggregation entries: direction, and heavy rows inside the main launch (gcl.h)."""
    return (1 if transpose else 0) | AGG_HEAVY_INSIDE


def aggregate(graph: Graph, h3, bias, transpose=False, out=None):
    """h3: [B, n, F] with unit channel stride; returns [B, n, F]."""
    B, n, F = h3.shape
    assert n == graph.n, f"graph has {graph.n} nodes, features have {n} rows"
    assert h3.stride(2) == 1
    if out is None:
        out = torch.empty(B, n, F, dtype=torch.float32, device=h3.device)
    tok = _probe_begin("aggregate", graph=graph, transpose=bool(transpose), B=B, F=F)
    _check(lib().gcl_aggregate(graph.handle, _agg_flags(transpose), _p(h3), h3.stride(1), h3.stride(0), _p(bias),
                               _p(out), out.stride(1), out.stride(0), B, F, _stream()))
    _probe_end(tok)
    return out


def aggregate_present(graph: Graph, h3, present, bias=None, transpose=False, out=None):
    """hip.aggregate with absent source rows: present int32 [n], entry < 0 = that row of h3 counts as zeros and is never
    read (it may be uninitialised memory).  Reported to the launch probe under a kind of its own."""
    B, n, F = h3.shape
    assert n == graph.n, f"graph has {graph.n} nodes, features have {n} rows"
    assert h3.stride(2) == 1 and present.dtype == torch.int32 and present.numel() == n and present.is_contiguous()
    if out is None:
        out = torch.empty(B, n, F, dtype=torch.float32, device=h3.device)
    tok = _probe_begin("aggregate_present", graph=graph, transpose=bool(transpose), B=B, F=F)
    _check(lib().gcl_aggregate_present(graph.handle, _agg_flags(transpose), _p(h3), h3.stride(1), h3.stride(0),
                                       _pi(present), _p(bias), _p(out), out.stride(1), out.stride(0), B, F, _stream()))
    _probe_end(tok)
    return out


def aggregate_compact_ok(graph: Graph, h3, transpose=False) -> bool:
    """Can aggregate_compact take h3 [B, n, F] (output dense [B, n, F])?"""
    B, n, F = h3.shape
    return bool(lib().gcl_aggregate_compact_ok(graph.handle, 1 if transpose else 0, h3.stride(1), h3.stride(0), F, n * F, B, F))


def aggregate_compact(graph: Graph, h3, smap, outc, transpose=False, out=None):
    """hip.aggregate with a store map: int32 smap [n], entry >= 0 = that row goes to row smap[i] of outc [B, *, F] instead
    of `out` (whose rows with such an entry stay unwritten).  Reported to the launch probe under a kind of its own."""
    B, n, F = h3.shape
    assert n == graph.n and h3.stride(2) == 1 and outc.stride(2) == 1 and outc.shape[0] == B and outc.shape[2] == F
    assert smap.dtype == torch.int32 and smap.numel() == n and smap.is_contiguous()
    if out is None:
        out = torch.empty(B, n, F, dtype=torch.float32, device=h3.device)
    tok = _probe_begin("aggregate_compact", graph=graph, transpose=bool(transpose), B=B, F=F)
    _check(lib().gcl_aggregate_compact(graph.handle, 1 if transpose else 0, _p(h3), h3.stride(1), h3.stride(0), _pi(smap),
                                       _p(out), out.stride(1), out.stride(0), _p(outc), outc.stride(1), outc.stride(0), B, F,
                                       _stream()))
    _probe_end(tok)
    return out


def aggregate_heavy_launches() -> int:
    """Launches of the one-block-per-heavy-row kernel as a launch of its own, so far in this process (see gcl.h)."""
    return int(lib().gcl_aggregate_heavy_launches())


def aggregate_split(graph: Graph, a3, b3, transpose=False, out=None):
    """hip.aggregate over the rows of TWO tensors: a3 [B, head, F] are rows < head of every sample, b3 [B, n - head, F] the
    rest (any row / batch strides that keep rows whole 16-byte units).  Reported to the launch probe under a kind of its
    own."""
    B, head, F = a3.shape
    n = head + b3.shape[1]
    assert n == graph.n, f"graph has {graph.n} nodes, the two parts have {n} rows"
    assert b3.shape[0] == B and b3.shape[2] == F and a3.stride(2) == 1 and b3.stride(2) == 1
    if out is None:
        out = torch.empty(B, n, F, dtype=torch.float32, device=a3.device)
    tok = _probe_begin("aggregate_split", graph=graph, transpose=bool(transpose), B=B, F=F)
    _check(lib().gcl_aggregate_split(graph.handle, _agg_flags(transpose), _p(a3), a3.stride(1), a3.stride(0), _p(b3),
                                     b3.stride(1), b3.stride(0), head, None, _p(out), out.stride(1), out.stride(0), B, F,
                                     _stream()))
    _probe_end(tok)
    return out


def aggregate_head(graph: Graph, a3, transpose=False, out=None):
    """hip.aggregate over a source whose rows >= head are zeros that are stored nowhere: a3 [B, head, F] are rows < head of
    every sample (rows whole 16-byte units, as for aggregate_split).  Reported to the launch probe under a kind of its own."""
    B, head, F = a3.shape
    n = graph.n
    assert 0 < head <= n and a3.stride(2) == 1
    if out is None:
        out = torch.empty(B, n, F, dtype=torch.float32, device=a3.device)
    tok = _probe_begin("aggregate_head", graph=graph, transpose=bool(transpose), B=B, F=F)
    _check(lib().gcl_aggregate_head(graph.handle, _agg_flags(transpose), _p(a3), a3.stride(1), a3.stride(0), head, None,
                                    _p(out), out.stride(1), out.stride(0), B, F, _stream()))
    _probe_end(tok)
    return out


def layernorm_fwd(x, gamma, beta, eps=1e-5):
    rows, F = x.shape
    y = torch.empty(rows, F, dtype=torch.float32, device=x.device)
    stats = torch.empty(rows, 2, dtype=torch.float32, device=x.device)
    _check(lib().gcl_layernorm_fwd(_p(x), _ld(x), _p(gamma), _p(beta), float(eps), _p(y), F, _p(stats), rows, F, _stream()))
    return y, stats


def layernorm_fwd_map(x, gamma, beta, eps, out3, pos):
    """LayerNorm of x [B * n, F] with row (b, i) written to out3[b, pos[i], :F] (pos[i] >= 0) and dropped otherwise;
    returns the (mean, rstd) statistics of every row."""
    rows, F = x.shape
    n_per = pos.numel()
    assert out3.stride(2) == 1 and rows % n_per == 0 and out3.shape[0] == rows // n_per
    stats = torch.empty(rows, 2, dtype=torch.float32, device=x.device)
    _check(lib().gcl_layernorm_fwd_map(_p(x), _ld(x), _p(gamma), _p(beta), float(eps), _p(out3), out3.stride(1), out3.stride(0),
                                       _pi(pos), n_per, _p(stats), rows, F, _stream()))
    return stats


def layernorm_fwd_map_skip(x, gamma, beta, eps, out3, pos, rlist):
    """layernorm_fwd_map for a LayerNorm whose dropped rows nobody reads: rlist int32 = the rows i with pos[i] >= 0.  Only
    those rows of x are read; the statistics of the others are uninitialised (layernorm_bwd(..., skip=True) ignores them)."""
    rows, F = x.shape
    n_per = pos.numel()
    assert out3.stride(2) == 1 and rows % n_per == 0 and out3.shape[0] == rows // n_per and rlist.stride(0) == 1
    stats = torch.empty(rows, 2, dtype=torch.float32, device=x.device)
    _check(lib().gcl_layernorm_fwd_map_skip(_p(x), _ld(x), _p(gamma), _p(beta), float(eps), _p(out3), out3.stride(1),
                                            out3.stride(0), _pi(pos), n_per, _pi(rlist), rlist.numel(), _p(stats), rows, F,
                                            _stream()))
    return stats


def layernorm_bwd(dy, x, gamma, stats, dgamma, dbeta, accumulate: bool, colsum_dx=None, acc_colsum: bool = False,
                  dy_map=None, skip: bool = False):
    """dx of the node LayerNorm (+ dgamma, dbeta); `colsum_dx` also receives the column sums of dx (the bias
    gradient of the layer below) from the same pass.  dy_map = (src3 [B, m, F'], pos int32 [n]): dy is not dense -
    row (b, i) reads src3[b, pos[i], :F] (zero where pos[i] < 0); x then holds B * n rows."""
    rows, F = x.shape
    dx = torch.empty(rows, F, dtype=torch.float32, device=x.device)
    nb = lib().gcl_layernorm_bwd_ws_bytes(rows, F)
    acc = (ACC_DW if accumulate else 0) | (ACC_COLSUM if acc_colsum else 0)
    if dy_map is not None:
        src3, pos = dy_map
        assert src3.stride(2) == 1 and src3.shape[2] >= F and rows % pos.numel() == 0 and src3.shape[0] == rows // pos.numel()
    else:
        assert not skip, "skip needs the mapped gradient"
    if _deferred.active:
        if dy_map is not None:
            a = (_p(src3), src3.stride(1), src3.stride(0), _pi(pos), pos.numel(), 1 if skip else 0)
        else:
            a = (_p(dy), _ld(dy), 0, None, 0, 0)
        _queue(nb, x.device, (dgamma, dbeta, colsum_dx), 1, lambda ws, jobs: lib().gcl_layernorm_bwd_deferred(
            *a, _p(x), _ld(x), _p(gamma), _p(stats), _p(dx), F, _p(dgamma), _p(dbeta), _p(colsum_dx), acc, rows, F,
            ws.data_ptr(), ws.numel(), _stream(), C.cast(jobs, C.c_void_p)))
        return dx
    ws = workspace(nb, x.device)
    if dy_map is not None:
        # skip: rows with pos < 0 are not touched - their x / statistics are not read, their dx (zero) is not written
        fn = lib().gcl_layernorm_bwd_map_skip if skip else lib().gcl_layernorm_bwd_map
        _check(fn(_p(src3), src3.stride(1), src3.stride(0), _pi(pos), pos.numel(), _p(x), _ld(x),
                                           _p(gamma), _p(stats), _p(dx), F, _p(dgamma), _p(dbeta), _p(colsum_dx), acc, rows, F,
                                           ws.data_ptr(), ws.numel(), _stream()))
        return dx
    _check(lib().gcl_layernorm_bwd_cs(_p(dy), _ld(dy), _p(x), _ld(x), _p(gamma), _p(stats), _p(dx), F, _p(dgamma),
                                      _p(dbeta), _p(colsum_dx), acc, rows, F, ws.data_ptr(), ws.numel(), _stream()))
    return dx


def graphnorm_fwd(x3, gamma, beta, eps=1e-5):
    B, n, F = x3.shape
    y = torch.empty(B, n, F, dtype=torch.float32, device=x3.device)
    stats = torch.empty(B, 2, dtype=torch.float32, device=x3.device)
    nb = lib().gcl_graphnorm_ws_bytes(B, n, F)
    ws = workspace(nb, x3.device)
    _check(lib().gcl_graphnorm_fwd(_p(x3), x3.stride(1), x3.stride(0), _p(gamma), _p(beta), float(eps), _p(y), F, n * F,
                                   _p(stats), B, n, F, ws.data_ptr(), ws.numel(), _stream()))
    return y, stats


def graphnorm_bwd(dy3, x3, gamma, stats, dgamma, dbeta, accumulate: bool, eps=1e-5):
    B, n, F = x3.shape
    dx = torch.empty(B, n, F, dtype=torch.float32, device=x3.device)
    nb = lib().gcl_graphnorm_ws_bytes(B, n, F)
    ws = workspace(nb, x3.device)
    _check(lib().gcl_graphnorm_bwd(_p(dy3), dy3.stride(1), dy3.stride(0), _p(x3), x3.stride(1), x3.stride(0), _p(gamma),
                                   _p(stats), float(eps), _p(dx), F, n * F, _p(dgamma), _p(dbeta),
                                   1 if accumulate else 0, B, n, F, ws.data_ptr(), ws.numel(), _stream()))
    return dx


def colsum(x, out, accumulate: bool):
    rows, F = x.shape
    nb = lib().gcl_colsum_ws_bytes(rows, F)
    if _deferred.active:
        _queue(nb, x.device, (out,), 1, lambda ws, jobs: lib().gcl_colsum_deferred(
            _p(x), _ld(x), rows, F, _p(out), 1 if accumulate else 0, ws.data_ptr(), ws.numel(), _stream(),
            C.cast(jobs, C.c_void_p)))
        return out
    ws = workspace(nb, x.device)
    _check(lib().gcl_colsum(_p(x), _ld(x), rows, F, _p(out), 1 if accumulate else 0, ws.data_ptr(), ws.numel(), _stream()))
    return out


def colsum_split(a3, b3, out, accumulate: bool):
    """hip.colsum over the B * n rows of a two-part source (see aggregate_split)."""
    B, head, F = a3.shape
    n = head + b3.shape[1]
    assert b3.shape[0] == B and b3.shape[2] == F and a3.stride(2) == 1 and b3.stride(2) == 1
    nb = lib().gcl_colsum_ws_bytes(B * n, F)
    args = (_p(a3), a3.stride(1), a3.stride(0), _p(b3), b3.stride(1), b3.stride(0), head, n, B, F, _p(out),
            1 if accumulate else 0)
    if _deferred.active:
        _queue(nb, a3.device, (out,), 1, lambda ws, jobs: lib().gcl_colsum_split_deferred(
            *args, ws.data_ptr(), ws.numel(), _stream(), C.cast(jobs, C.c_void_p)))
        return out
    ws = workspace(nb, a3.device)
    _check(lib().gcl_colsum_split(*args, ws.data_ptr(), ws.numel(), _stream()))
    return out


def gat_tab_ok(graph: Graph, H: int, Cc: int) -> bool:
    """True when gat_fwd / gat_bwd can read the rows of h through a row table (one head, source-tile graph)."""
    return bool(lib().gcl_gat_tab_ok(graph.handle, H * Cc, int(H), int(Cc)))


def gat_fwd(graph: Graph, h3, att_src, att_dst, bias, H, Cc, need_alpha=True, tab=None):
    """tab (int32 [graph.n]): h3 is [B, rows, H*C] and mesh row i of sample b is h3[b, tab[i]] or the flat row ~tab[i]."""
    B, n, HC = h3.shape
    if tab is not None:
        n = graph.n
        assert h3.is_contiguous()
    dev = h3.device
    a_s = torch.empty(B, n, H, dtype=torch.float32, device=dev)
    a_d = torch.empty(B, n, H, dtype=torch.float32, device=dev)
    alpha = torch.empty(B, graph.e, H, dtype=torch.float32, device=dev) if need_alpha else None
    y = torch.empty(B, n, Cc, dtype=torch.float32, device=dev)
    tok = _probe_begin("gat_fwd", graph=graph, B=B, H=H, C=Cc, alpha=need_alpha)
    if tab is not None:
        _check(lib().gcl_gat_fwd_tab(graph.handle, _p(h3), h3.stride(1), h3.stride(0), _pi(tab), _p(att_src), _p(att_dst),
                                     _p(bias), _p(a_s), _p(a_d), _p(alpha), _p(y), Cc, n * Cc, B, H, Cc, _stream()))
    else:
        _check(lib().gcl_gat_fwd(graph.handle, _p(h3), h3.stride(1), h3.stride(0), _p(att_src), _p(att_dst), _p(bias),
                                 _p(a_s), _p(a_d), _p(alpha), _p(y), Cc, n * Cc, B, H, Cc, _stream()))
    _probe_end(tok)
    return y, a_s, a_d, alpha


def gat_bwd(graph: Graph, dy3, h3, att_src, att_dst, a_s, a_d, alpha, d_att_src, d_att_dst, d_bias, accumulate, H, Cc, tab=None):
    B, n, HC = h3.shape
    if tab is not None:
        n = graph.n  # dh is dense [B, n, HC]: the gradient of the table-read rows
    dy3 = dy3.contiguous()
    dh = torch.empty(B, n, HC, dtype=torch.float32, device=h3.device)
    nb = lib().gcl_gat_bwd_ws_bytes(graph.e, n, B, H, Cc)
    ws = workspace(nb, h3.device)
    tok = _probe_begin("gat_bwd", graph=graph, B=B, H=H, C=Cc)
    if tab is not None:
        _check(lib().gcl_gat_bwd_tab(graph.handle, _p(dy3), Cc, n * Cc, _p(h3), h3.stride(1), h3.stride(0), _pi(tab), _p(att_src),
                                     _p(att_dst), _p(a_s), _p(a_d), _p(alpha), _p(dh), HC, n * HC, _p(d_att_src),
                                     _p(d_att_dst), _p(d_bias), 1 if accumulate else 0, B, H, Cc, ws.data_ptr(), ws.numel(),
                                     _stream()))
    else:
        _check(lib().gcl_gat_bwd(graph.handle, _p(dy3), Cc, n * Cc, _p(h3), h3.stride(1), h3.stride(0), _p(att_src),
                                 _p(att_dst), _p(a_s), _p(a_d), _p(alpha), _p(dh), HC, n * HC, _p(d_att_src), _p(d_att_dst),
                                 _p(d_bias), 1 if accumulate else 0, B, H, Cc, ws.data_ptr(), ws.numel(), _stream()))
    _probe_end(tok)
    return dh


def gat_alpha_edge_order(graph: Graph, alpha_slots_1sample, H):
    out = torch.empty(graph.e, H, dtype=torch.float32, device=alpha_slots_1sample.device)
    _check(lib().gcl_gat_alpha_to_edge_order(graph.handle, _p(alpha_slots_1sample.contiguous()), _p(out), H, _stream()))
    return out


def gat_prune(graph: Graph, alpha_edges, threshold: float) -> torch.Tensor:
    """Surviving PyG-order edge list (CPU int64 `[2, kept]`)."""
    buf = torch.empty(2 * graph.e, dtype=torch.int64)
    kept = _i64(0)
    nb = lib().gcl_gat_prune_ws_bytes(graph.e)
    ws = workspace(nb, alpha_edges.device)
    _check(lib().gcl_gat_prune(graph.handle, _p(alpha_edges.contiguous()), float(threshold), buf.data_ptr(),
                               C.byref(kept), ws.data_ptr(), ws.numel(), _stream()))
    k = kept.value
    return buf[: 2 * k].view(2, k).clone()


def assemble_input(x3, grid_static, mesh_static, tail3=None):
    """[B, G + M, Cdyn + Cs] = grid rows [x | grid_static], mesh rows [0 | mesh_static]; `tail3` [B, r, C] (optional)
    overwrites the last r mesh rows of every sample (per-sample rows: the folded batch-invariant mesh rows)."""
    B, G, Cdyn = x3.shape
    M, Cs = mesh_static.shape
    x3 = x3.contiguous()
    out = torch.empty(B, G + M, Cdyn + Cs, dtype=torch.float32, device=x3.device)
    if tail3 is not None and tail3.is_contiguous() and tail3.shape[2] == Cdyn + Cs:
        _check(lib().gcl_assemble_input_tail(_p(x3), _p(grid_static), _p(mesh_static), _p(tail3), tail3.shape[1], _p(out),
                                             Cdyn + Cs, B, G, M, Cdyn, Cs, _stream()))
        return out
    _check(lib().gcl_assemble_input(_p(x3), _p(grid_static), _p(mesh_static), _p(out), Cdyn + Cs, B, G, M, Cdyn, Cs, _stream()))
    if tail3 is not None:
        copy_rows(tail3, out[:, G + M - tail3.shape[1]:, :])
    return out


def wmse_fwd_bwd(delta3, x_last3, y3, node_w, chan_w, inv_wsum, grad_scale, want_grad=True, want_state=False,
                 loss_prev=None, ldd_out=None):
    """delta3 [B,G,C] contiguous; x_last3 / y3 may be strided views (unit channel stride).  ldd_out (>= C): the gradient
    is the [..., :C] view of a contiguous [B, G, ldd_out] tensor whose other columns are written as zeros
    (gcl_wmse_fwd_bwd_ld); the loss and the values are the same."""
    B, G, Cc = delta3.shape
    dev = delta3.device
    if delta3.stride(2) != 1:
        delta3 = delta3.contiguous()  # (a row-strided view - e.g. the grid rows of a padded output - is read in place)
    dd = None
    if want_grad:
        dd = torch.empty(B, G, ldd_out if ldd_out else Cc, dtype=torch.float32, device=dev)
    st = torch.empty(B, G, Cc, dtype=torch.float32, device=dev) if want_state else None
    loss = torch.empty((), dtype=torch.float32, device=dev)
    nb = lib().gcl_wmse_ws_bytes(B, G, Cc)
    ws = workspace(nb, dev)
    xl = x_last3
    head = (_p(delta3), delta3.stride(1), delta3.stride(0), _p(xl), xl.stride(1) if xl is not None else 0,
            xl.stride(0) if xl is not None else 0, _p(y3), y3.stride(1), y3.stride(0), _p(node_w), _p(chan_w), float(inv_wsum),
            float(grad_scale), _p(dd))
    tail = (_p(st), _p(loss_prev), _p(loss), B, G, Cc, ws.data_ptr(), ws.numel(), _stream())
    if ldd_out:
        assert ldd_out >= Cc
        _check(lib().gcl_wmse_fwd_bwd_ld(*head, int(ldd_out), G * int(ldd_out), *tail))
        return loss, (dd[..., :Cc] if dd is not None else None), st
    _check(lib().gcl_wmse_fwd_bwd(*head, *tail))
    return loss, dd, st


def adam_step(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0):
    _check(lib().gcl_adam_step(_p(p), _p(g), _p(m), _p(v), p.numel(), lr, beta1, beta2, eps, weight_decay, int(step),
                               float(grad_scale), _stream()))


def adam_step_dev(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step_dev, bc_dev, grad_scale=1.0):
    assert step_dev.dtype == torch.int32 and step_dev.is_cuda
    _check(lib().gcl_adam_step_dev(_p(p), _p(g), _p(m), _p(v), p.numel(), lr, beta1, beta2, eps, weight_decay,
                                   step_dev.data_ptr(), _p(bc_dev), float(grad_scale), _stream()))


def adam_step_groups(p, g, m, v, chunk_param, active, lr, step, bc, beta1, beta2, eps, weight_decay, grad_scale=1.0):
    """Grouped Adam over a flat bucket (see gcl.h): per-parameter `active` / `step` (int32), `lr` (float32) and `bc`
    (float32 [P, 2] scratch) and the chunk -> parameter map `chunk_param` (int32 [p.numel() / 64]), all on the device."""
    P = step.numel()
    assert p.is_cuda and p.numel() % 64 == 0 and chunk_param.numel() == p.numel() // 64
    assert step.dtype == active.dtype == chunk_param.dtype == torch.int32 and lr.dtype == bc.dtype == torch.float32
    assert active.numel() == lr.numel() == P and bc.numel() == 2 * P
    _check(lib().gcl_adam_step_groups(_p(p), _p(g), _p(m), _p(v), p.numel(), _pi(chunk_param), P, _pi(active),
                                      _p(lr), _pi(step), _p(bc), beta1, beta2, eps, weight_decay, float(grad_scale),
                                      _stream()))


def copy_rows(src3, dst3):
    B, rows, F = src3.shape
    _check(lib().gcl_copy_rows(_p(src3), src3.stride(1), src3.stride(0), _p(dst3), dst3.stride(1), dst3.stride(0), B, rows, F, _stream()))
    return dst3


def _pi(t):
    if t is None:
        return None
    assert t.is_cuda and t.dtype == torch.int32 and t.is_contiguous()
    return t.data_ptr()


def gather2_rows(a3, map_a, b3, map_b, nd: int, B: int, sum_batch: bool = False, out=None, deal: int = 0):
    """dst[b,i] = a3[b, map_a[i]] | b3[b or 0, map_b[i]] | 0   (see gcl_gather2_rows).
    a3 / b3: [Ba, na, F] with unit channel stride; Ba == 1 broadcasts over B.  `out`: a (possibly row-strided)
    [B | 1, nd, F] destination, e.g. a row range of a larger buffer.  sum_batch with deal = R > 1: the nd batch-summed
    rows are stored R to a destination sample, out [nd / R, R, F] (possibly strided)."""
    F = a3.shape[-1]
    if sum_batch and deal > 1:
        assert out is not None and nd % deal == 0 and out.shape == (nd // deal, deal, F) and out.stride(2) == 1
        flag = deal
    else:
        if out is None:
            out = torch.empty(1 if sum_batch else B, nd, F, dtype=torch.float32, device=a3.device)
        assert out.shape == (1 if sum_batch else B, nd, F) and out.stride(2) == 1
        flag = 1 if sum_batch else 0
    bsa = a3.stride(0) if (a3.shape[0] > 1 or sum_batch) else 0
    bsb = 0 if b3 is None else (b3.stride(0) if b3.shape[0] > 1 else 0)
    _check(lib().gcl_gather2_rows(_p(a3), a3.stride(1), bsa, _pi(map_a), _p(b3), 0 if b3 is None else b3.stride(1),
                                  bsb, _pi(map_b), _p(out), out.stride(1), out.stride(0), B, nd, F, flag, _stream()))
    return out


def roi_gather_rows(rows, rows_src: int, srcs, Fp: int, B: int, out=None):
    """out[b, i] = [s0[b, rows[i]] | s1[b, rows[i]] | s2[b, rows[i]] | 0] (see gcl_roi_gather_rows).  `srcs`: up to three
    [B | 1, rows_src, w] tensors with unit channel stride and any row / batch stride (batch 1 broadcasts); `rows`: int32
    device indices (None = identity over the first `out.shape[1]` rows).  Returns [B, n, Fp] (or writes `out`)."""
    n = rows.numel() if rows is not None else out.shape[1]
    if out is None:
        out = torch.empty(B, n, Fp, dtype=torch.float32, device=srcs[0].device)
    assert out.shape == (B, n, Fp) and out.stride(2) == 1 and len(srcs) <= 3
    args = []
    for k in range(3):
        t = srcs[k] if k < len(srcs) else None
        if t is None or t.shape[-1] == 0:
            args += [None, 0, 0, 0]
            continue
        assert t.dim() == 3 and t.stride(2) == 1 and t.shape[1] == rows_src and t.shape[0] in (1, B)
        args += [_p(t), t.stride(1), t.stride(0) if t.shape[0] > 1 else 0, t.shape[2]]
    _check(lib().gcl_roi_gather_rows(_pi(rows), n, rows_src, *args, _p(out), out.stride(1), out.stride(0), Fp, B,
                                     _stream()))
    return out


def roi_compose(pred3, corr3, pos, out=None):
    """out[b, g] = pred3[b, g] + corr3[b, pos[g]] where pos[g] >= 0, else pred3[b, g] (see gcl_roi_compose)."""
    B, G, Cc = pred3.shape
    assert corr3.dim() == 3 and corr3.shape[0] == B and corr3.shape[2] >= Cc and pos.numel() == G
    assert pred3.stride(2) == 1 and corr3.stride(2) == 1
    if out is None:
        out = torch.empty(B, G, Cc, dtype=torch.float32, device=pred3.device)
    _check(lib().gcl_roi_compose(_p(pred3), pred3.stride(1), pred3.stride(0), _p(corr3), corr3.stride(1), corr3.stride(0),
                                 _pi(pos), _p(out), out.stride(1), out.stride(0), B, G, Cc, _stream()))
    return out


def segment_wsum(src3, idx, w, rowptr, out3=None, addend3=None, act=ACT_NONE, accumulate: bool = False):
    """out3[b, i] (+)= addend3[b, i] + sum_k w[k] act(src3[b, idx[k]]) over k in [rowptr[i], rowptr[i+1]) (see
    gcl_segment_wsum).  src3 [B | 1, n_src, >= D] (batch 1 broadcasts), out3 / addend3 [B, n, D]: unit channel stride,
    any row / batch stride (out3 may be a column block).  idx / rowptr int32, w float32 (None: idx = k, w = 1)."""
    n = rowptr.numel() - 1
    if out3 is None:
        B = src3.shape[0] if addend3 is None else addend3.shape[0]
        D = src3.shape[2] if addend3 is None else addend3.shape[2]
        out3 = torch.empty(B, n, D, dtype=torch.float32, device=src3.device)
    B, _, D = out3.shape
    assert out3.shape[1] == n and src3.stride(2) == 1 and out3.stride(2) == 1 and src3.shape[2] >= D
    assert src3.shape[0] in (1, B) and (addend3 is None or (addend3.shape == out3.shape and addend3.stride(2) == 1))
    assert w is None or (w.is_cuda and w.dtype == torch.float32 and w.is_contiguous())
    _check(lib().gcl_segment_wsum(_p(src3), src3.stride(1), src3.stride(0) if src3.shape[0] > 1 else 0, src3.shape[1],
                                  int(act), _pi(idx), w.data_ptr() if w is not None else None, _pi(rowptr), _p(addend3),
                                  addend3.stride(1) if addend3 is not None else 0,
                                  addend3.stride(0) if addend3 is not None else 0, _p(out3), out3.stride(1),
                                  out3.stride(0), 1 if accumulate else 0, B, n, D, _stream()))
    return out3


def cross_update_fwd(h3, msg3, rowptr, gamma, beta, eps=1e-5):
    """(pre [B, n, D], y [B, n, D], stats [B * n, 2]): pre = h + per-receiver mean of msg rows (receiver-sorted, CSR
    rowptr), y = node LayerNorm of pre (see gcl_cross_update_fwd)."""
    B, n, D = h3.shape
    assert h3.stride(2) == 1 and msg3.stride(2) == 1 and msg3.shape[0] == B and msg3.shape[2] == D
    assert rowptr.numel() == n + 1
    pre = torch.empty(B, n, D, dtype=torch.float32, device=h3.device)
    y = torch.empty(B, n, D, dtype=torch.float32, device=h3.device)
    stats = torch.empty(B * n, 2, dtype=torch.float32, device=h3.device)
    _check(lib().gcl_cross_update_fwd(_p(h3), h3.stride(1), h3.stride(0), _p(msg3), msg3.stride(1), msg3.stride(0),
                                      _pi(rowptr), _p(gamma), _p(beta), float(eps), _p(pre), _p(y), _p(stats), B, n, D,
                                      _stream()))
    return pre, y, stats


def ar_advance(state4, delta3, y_step3, chan_kind, out3, out_off: int, residual: bool):
    """state4 [B,G,obs,C] contiguous -> new state (same shape); appends the step to out3 [B,G,steps*C]."""
    B, G, obs, Cc = state4.shape
    assert state4.is_contiguous() and delta3.stride(2) == 1
    new_state = torch.empty_like(state4)
    _check(lib().gcl_ar_advance(
        _p(state4), _p(delta3), delta3.stride(1), delta3.stride(0), _p(y_step3), y_step3.stride(1) if y_step3 is not None else 0,
        y_step3.stride(0) if y_step3 is not None else 0, _pi(chan_kind), _p(new_state), _p(out3),
        out3.stride(1) if out3 is not None else 0, out3.stride(0) if out3 is not None else 0, int(out_off), B, G, obs, Cc,
        1 if residual else 0, _stream()))
    return new_state


def ar_step_bwd(dd3, g_loss, g_new4, chan_kind, has_y: bool, residual: bool, obs: int, want_state: bool, ldd_out=None):
    """Backward of one autoregressive training step (see gcl_ar_step_bwd): (d_delta [B,G,C], d_state [B,G,obs,C] | None).
    ldd_out: d_delta is the [..., :C] view of a contiguous [B, G, ldd_out] tensor with zero padding columns, and dd3 may be
    such a view itself (gcl_ar_step_bwd_ld)."""
    B, G, Cc = dd3.shape
    d_state = torch.empty(B, G, obs, Cc, dtype=torch.float32, device=dd3.device) if want_state else None
    if g_new4 is not None and not g_new4.is_contiguous():
        g_new4 = g_new4.contiguous()
    if ldd_out or not dd3.is_contiguous():
        assert dd3.stride(2) == 1
        ldo = int(ldd_out) if ldd_out else Cc
        d_delta = torch.empty(B, G, ldo, dtype=torch.float32, device=dd3.device)
        _check(lib().gcl_ar_step_bwd_ld(_p(dd3), dd3.stride(1), dd3.stride(0), _p(g_loss), _p(g_new4), _pi(chan_kind),
                                        1 if has_y else 0, 1 if residual else 0, _p(d_delta), ldo, G * ldo, _p(d_state), B, G,
                                        obs, Cc, _stream()))
        return d_delta[..., :Cc], d_state
    d_delta = torch.empty_like(dd3)
    _check(lib().gcl_ar_step_bwd(_p(dd3), _p(g_loss), _p(g_new4), _pi(chan_kind), 1 if has_y else 0, 1 if residual else 0,
                                 _p(d_delta), _p(d_state), B, G, obs, Cc, _stream()))
    return d_delta, d_state


def pad_rows(src3, rows_dst: int, F_dst: int):
    """[B, r, F] (unit channel stride) -> zero-padded contiguous [B, rows_dst, F_dst] in one pass."""
    B, r, F = src3.shape
    assert src3.stride(2) == 1
    dst = torch.empty(B, rows_dst, F_dst, dtype=torch.float32, device=src3.device)
    _check(lib().gcl_pad_rows(_p(src3), src3.stride(1), src3.stride(0), r, F, _p(dst), F_dst, rows_dst * F_dst, rows_dst, F_dst,
                              B, _stream()))
    return dst


def zero_(t: torch.Tensor):
    """t.zero_() as a stream memset through the C ABI (no torch fill kernel on the step)."""
    assert t.is_contiguous() and t.is_cuda
    _check(lib().gcl_zero(t.data_ptr(), t.numel() * t.element_size(), _stream()))
    return t


def segment_reduce(src3, perm, rowptr, mean: bool, out3=None):
    """src3 [B, E, D] (unit channel stride) -> out3 [B, n, D]: per-segment sum / mean of rows
    perm[rowptr[i]:rowptr[i+1]] (perm None: the rows themselves)."""
    B, _, D = src3.shape
    n = rowptr.numel() - 1
    if out3 is None:
        out3 = torch.empty(B, n, D, dtype=torch.float32, device=src3.device)
    assert src3.stride(2) == 1 and out3.stride(2) == 1 and tuple(out3.shape) == (B, n, D)
    _check(lib().gcl_segment_reduce(_p(src3), src3.stride(1), src3.stride(0), _pi(perm), _pi(rowptr), 1 if mean else 0,
                                    _p(out3), out3.stride(1), out3.stride(0), B, n, D, _stream()))
    return out3


def edge_combine(base3, extra3, A3, ia, sa, C3, ic, out3=None):
    """out[b,e] = base[b,e] + extra[b,e] + A[b, ia[e]] * sa[ia[e]] + C[b, ic[e]]  (operands optional)."""
    ref = base3 if base3 is not None else extra3
    if ref is not None:
        B, E, D = ref.shape
    else:
        B, E, D = (A3 if A3 is not None else C3).shape[0], ia.numel() if ia is not None else ic.numel(), \
            (A3 if A3 is not None else C3).shape[2]
    for t in (base3, extra3):
        assert t is None or t.is_contiguous()
    if out3 is None:
        out3 = torch.empty(B, E, D, dtype=torch.float32, device=(A3 if ref is None else ref).device)
    _check(lib().gcl_edge_combine(
        _p(base3), _p(extra3), _p(A3), A3.stride(1) if A3 is not None else 0, A3.stride(0) if A3 is not None else 0,
        _pi(ia), _p(sa), _p(C3), C3.stride(1) if C3 is not None else 0, C3.stride(0) if C3 is not None else 0, _pi(ic),
        _p(out3), B, E, D, _stream()))
    return out3


def act_fwd(x, act, slope=None):
    y = torch.empty_like(x)
    assert x.is_contiguous()
    _check(lib().gcl_act_fwd(_p(x), _p(y), x.numel(), int(act), _p(slope), _stream()))
    return y


def act_bwd(x, dy, act, slope=None, d_slope=None):
    assert x.is_contiguous() and dy.is_contiguous()
    dx = torch.empty_like(x)
    ws = workspace(lib().gcl_act_bwd_ws_bytes(), x.device)
    _check(lib().gcl_act_bwd(_p(x), _p(dy), _p(dx), x.numel(), int(act), _p(slope), _p(d_slope), ws.data_ptr(), ws.numel(),
                             _stream()))
    return dx


def window_pack(series, t0, mean, std, C: int, obs: int, pred: int, out=None):
    """series: fp16 [T, n_lon, n_lat, Ct] (or flat [T, N, Ct]) on the GPU; t0: int64 [B] window starts on
    the GPU.  Returns X [B, G, obs*C] and Y [B, G, pred*C] (None when pred == 0).  out = (X, Y): contiguous fp32
    buffers of those shapes to fill in place (e.g. TrainStep.input_buffers())."""
    assert series.is_cuda and series.dtype == torch.float16 and series.is_contiguous()
    assert t0.is_cuda and t0.dtype == torch.int64 and t0.is_contiguous()
    if series.dim() == 3:
        T, n_lon, Ct = series.shape
        n_lat = 1
    else:
        T, n_lon, n_lat, Ct = series.shape
    B, G = t0.numel(), n_lon * n_lat
    if out is not None:
        X, Y = out
        assert X.is_contiguous() and X.shape == (B, G, obs * C) and X.dtype == torch.float32 and X.device == series.device
        assert pred == 0 or (Y.is_contiguous() and Y.shape == (B, G, pred * C) and Y.dtype == torch.float32)
    else:
        X = torch.empty(B, G, obs * C, dtype=torch.float32, device=series.device)
        Y = torch.empty(B, G, pred * C, dtype=torch.float32, device=series.device) if pred > 0 else None
    _check(lib().gcl_window_pack(series.data_ptr(), T, n_lon, n_lat, Ct, t0.data_ptr(), _p(mean), _p(std), C, obs, pred,
                                 _p(X), _p(Y), B, _stream()))
    return X, Y


def gcn_layer_fusable(graph: Graph, x3, Fin: int, Fout: int) -> bool:
    """Does this GCNConv layer fit the one-kernel path (csrc/gcn_layer.hip)?  GCL_FUSED_GCN=0 forces the
    two-kernel path (linear + aggregate) for A/B measurements."""
    import os
    if os.environ.get("GCL_FUSED_GCN", "1") in ("0",):
        return False
    return (Fin % 4 == 0 and 4 <= Fin <= 64 and 1 <= Fout <= 64 and graph.max_in_degree <= 64 and graph.kind in (GRAPH_GCN, GRAPH_MEAN)
            and x3.stride(2) == 1 and x3.stride(1) % 4 == 0 and x3.stride(0) % 4 == 0 and x3.data_ptr() % 16 == 0)


def gcn_layer_fwd(graph: Graph, x3, act, slope, W, bias, out=None, rows_out=None, present=None):
    """y = (A_hat act(x)) W^T + bias for x3 [B, n, Fin] -> [B, n, Fout] (one kernel).  The result is a view of
    a [B, n, roundup(Fout, 4)] buffer whose padding columns are zero.  rows_out: only the first rows_out rows of every
    sample are computed (the others stay unwritten).  present int32 [n]: rows with a negative entry may stay unwritten
    too (gcl_gcn_layer_fwd_present; reported to the launch probe under a kind of its own)."""
    B, n, Fin = x3.shape
    assert n == graph.n
    Fout = W.shape[0]
    Fst = (Fout + 3) // 4 * 4
    if out is None:
        out = torch.empty(B, n, Fst, dtype=torch.float32, device=x3.device)
    assert out.shape[2] >= Fst or out.stride(1) >= Fst
    if present is not None:
        assert not rows_out and present.numel() == n
        tok = _probe_begin("gcn_layer_fwd_present", graph=graph, B=B, Fin=Fin, Fout=Fout)
        _check(lib().gcl_gcn_layer_fwd_present(graph.handle, _p(x3), x3.stride(1), x3.stride(0), int(act), _p(slope),
                                               _p(W.contiguous()), _p(bias), _p(out), out.stride(1), out.stride(0),
                                               _pi(present), B, Fin, Fout, Fst, _stream()))
        _probe_end(tok)
        return out[..., :Fout]
    tok = _probe_begin("gcn_layer_fwd", graph=graph, B=B, Fin=Fin, Fout=Fout)
    _check(lib().gcl_gcn_layer_fwd_rows(graph.handle, _p(x3), x3.stride(1), x3.stride(0), int(act), _p(slope),
                                        _p(W.contiguous()), _p(bias), _p(out), out.stride(1), out.stride(0), B, Fin, Fout,
                                        Fst, int(rows_out) if rows_out else n, _stream()))
    _probe_end(tok)
    return out[..., :Fout]


def gcn_layer_split_ok(graph: Graph, x3, Fout: int, ya, yb=None) -> bool:
    """True when gcn_layer_fwd_split would store the layer's rows < ya.shape[1] in ya and the others in yb (None: a
    contiguous [B, n - head, roundup(Fout, 4)] tensor that the caller has yet to make)."""
    B, n, Fin = x3.shape
    head, Fst = ya.shape[1], (int(Fout) + 3) // 4 * 4
    if not (gcn_layer_fusable(graph, x3, Fin, Fout) and n == graph.n and ya.stride(2) == 1 and ya.data_ptr() % 16 == 0):
        return False
    if yb is not None and not (yb.stride(2) == 1 and yb.data_ptr() % 16 == 0 and head + yb.shape[1] == n):
        return False
    ldb, bsb = (yb.stride(1), yb.stride(0)) if yb is not None else (Fst, (n - head) * Fst)
    return bool(lib().gcl_gcn_layer_fwd_split_ok(graph.handle, x3.stride(1), x3.stride(0), ya.stride(1), ya.stride(0), ldb, bsb,
                                                 head, B, Fin, int(Fout), Fst))


def gcn_layer_fwd_split(graph: Graph, x3, act, slope, W, bias, ya, yb):
    """gcn_layer_fwd with a two-part destination (gcl_gcn_layer_fwd_split): rows < head = ya.shape[1] of every sample go to
    ya [B, head, >= Fout], the others to yb [B, n - head, >= Fout]; both may be row ranges of larger buffers.  Reported to the
    launch probe under a kind of its own."""
    B, n, Fin = x3.shape
    head = ya.shape[1]
    assert n == graph.n and head + yb.shape[1] == n and ya.shape[0] == B and yb.shape[0] == B
    assert ya.stride(2) == 1 and yb.stride(2) == 1
    Fout = W.shape[0]
    Fst = (Fout + 3) // 4 * 4
    tok = _probe_begin("gcn_layer_fwd_split", graph=graph, B=B, Fin=Fin, Fout=Fout)
    _check(lib().gcl_gcn_layer_fwd_split(graph.handle, _p(x3), x3.stride(1), x3.stride(0), int(act), _p(slope), _p(W.contiguous()),
                                         _p(bias), _p(ya), ya.stride(1), ya.stride(0), _p(yb), yb.stride(1), yb.stride(0), head, B,
                                         Fin, Fout, Fst, _stream()))
    _probe_end(tok)


def gcn_layer_tab_ok(graph: Graph, x3, Fout: int) -> bool:
    """True when gcn_layer_fwd_tab would run on x3 [B, rows, Fin] (source-tile graph, 48 / 64-wide rows, 32-bit offsets)."""
    B, nx, Fin = x3.shape
    return bool(lib().gcl_gcn_layer_fwd_tab_ok(graph.handle, x3.stride(1), x3.stride(0), B * nx, B, Fin, int(Fout)))


def gcn_layer_fwd_tab(graph: Graph, x3, tab, act, slope, W, bias):
    """The one-kernel GCNConv layer whose input row i of sample b is x3[b, tab[i]] (tab[i] >= 0) or the batch-invariant
    row ~tab[i] of x3 viewed as [B * rows, Fin] (tab[i] < 0): the mesh latents of the compact pipeline are never
    materialised (see gcl_gcn_layer_fwd_tab).  x3 [B, rows, Fin] contiguous, tab int32 [graph.n]."""
    B, nx, Fin = x3.shape
    assert x3.is_contiguous() and tab.dtype == torch.int32 and tab.numel() == graph.n
    Fout = W.shape[0]
    Fst = (Fout + 3) // 4 * 4
    out = torch.empty(B, graph.n, Fst, dtype=torch.float32, device=x3.device)
    tok = _probe_begin("gcn_layer_fwd", graph=graph, B=B, Fin=Fin, Fout=Fout)
    _check(lib().gcl_gcn_layer_fwd_tab(graph.handle, _p(x3), x3.stride(1), x3.stride(0), B * nx, _pi(tab), int(act), _p(slope),
                                       _p(W.contiguous()), _p(bias), _p(out), out.stride(1), out.stride(0), B, Fin, Fout, Fst,
                                       _stream()))
    _probe_end(tok)
    return out[..., :Fout]


# ------------------------------------------------------------------------------------------------------------------
# Data assimilation (csrc/assim.hip)
# ------------------------------------------------------------------------------------------------------------------
def _pd(t: torch.Tensor):
    assert t.is_cuda and t.dtype == torch.float64 and t.is_contiguous()
    return t.data_ptr()


def nudge(f3, o3, out3, c0: float, c1: float, form: int, chan_mask=None):
    """out3 = nudged f3 (see gcl_nudge).  f3, o3, out3: [B, G, C] views with unit channel stride; chan_mask: uint8 [C]
    device tensor or None.  out3 may be f3."""
    B, G, Cc = f3.shape
    assert o3.shape == f3.shape and out3.shape == f3.shape
    assert f3.stride(2) == 1 and o3.stride(2) == 1 and out3.stride(2) == 1
    if chan_mask is not None:
        assert chan_mask.is_cuda and chan_mask.dtype == torch.uint8 and chan_mask.numel() == Cc
    if f3.numel() == 0:  # no element to nudge (an empty view has a null data_ptr(), which the C entry point refuses)
        return out3
    _check(lib().gcl_nudge(_p(f3), f3.stride(1), f3.stride(0), _p(o3), o3.stride(1), o3.stride(0),
                           chan_mask.data_ptr() if chan_mask is not None else None, float(c0), float(c1), int(form),
                           _p(out3), out3.stride(1), out3.stride(0), B, G, Cc, _stream()))
    return out3


def nudge_rows(f3, o3, out3, station_mask, net_of_row, alpha, chan_mask=None):
    """out3 = f3 nudged row by row (see gcl_nudge_rows): row b with alpha[b] (float32 [B]) at the stations of network
    net_of_row[b] (int32 [B], -1: not nudged) of station_mask (uint8 [n_net, G]).  o3 is [B, G, C] or [1, G, C] (one
    truth for every row).  out3 may be f3."""
    B, G, Cc = f3.shape
    assert out3.shape == f3.shape and o3.shape[1:] == f3.shape[1:] and o3.shape[0] in (1, B)
    assert f3.stride(2) == 1 and o3.stride(2) == 1 and out3.stride(2) == 1
    assert station_mask.is_cuda and station_mask.dtype == torch.uint8 and station_mask.is_contiguous()
    assert station_mask.dim() == 2 and station_mask.shape[1] == G
    assert net_of_row.dtype == torch.int32 and net_of_row.numel() == B and alpha.numel() == B
    if chan_mask is not None:
        assert chan_mask.is_cuda and chan_mask.dtype == torch.uint8 and chan_mask.numel() == Cc
    if f3.numel() == 0:  # as in `nudge`
        return out3
    _check(lib().gcl_nudge_rows(_p(f3), f3.stride(1), f3.stride(0), _p(o3), o3.stride(1),
                                o3.stride(0) if o3.shape[0] == B and B > 1 else 0, station_mask.data_ptr(),
                                station_mask.shape[0], _pi(net_of_row), _p(alpha),
                                chan_mask.data_ptr() if chan_mask is not None else None, _p(out3), out3.stride(1),
                                out3.stride(0), B, G, Cc, _stream()))
    return out3


def oi_max_stations() -> int:
    return int(lib().gcl_oi_max_stations())


def oi_factor(lat, lon, sb2: float, rl2: float, diag: float):
    """float64 [m, m] factor of the station covariance of stations (lat, lon) (float64 radians, device)."""
    m = lat.numel()
    M = torch.empty(m, m, dtype=torch.float64, device=lat.device)
    _check(lib().gcl_oi_station_cov(_pd(lat), _pd(lon), m, float(sb2), float(rl2), float(diag), M.data_ptr(), _stream()))
    _check(lib().gcl_oi_factor(M.data_ptr(), m, _stream()))
    return M


def oi_solve(M, rhs, tmp, W):
    """W [n, m] float32 = S^-1 rhs for rhs [n, m] float64 (tmp: float64 workspace of the same shape)."""
    m = M.shape[0]
    n = rhs.shape[0]
    assert rhs.shape == (n, m) and tmp.shape == (n, m) and W.shape == (n, m) and W.is_contiguous()
    _check(lib().gcl_oi_solve(_pd(M), m, _pd(rhs), _pd(tmp), _p(W), n, _stream()))
    return W


def oi_innovation(obs3, xb3, obs_row, node_row, chans, rhs):
    """rhs[b * nch + q, k] = obs3[b, obs_row[k], chans[q]] - xb3[b, node_row[k], chans[q]] (float64)."""
    B = xb3.shape[0]
    m, nch = obs_row.numel(), chans.numel()
    assert obs3.shape[0] == B and obs3.stride(2) == 1 and xb3.stride(2) == 1 and rhs.shape == (B * nch, m)
    _check(lib().gcl_oi_innovation(_p(obs3), obs3.stride(1), obs3.stride(0), _p(xb3), xb3.stride(1), xb3.stride(0),
                                   _pi(obs_row), _pi(node_row), _pi(chans), m, nch, B, _pd(rhs), _stream()))
    return rhs


def oi_analysis(xb3, xa3, chans, node_row, nodes, stations, W, sb2: float, rl2: float, th_cut: float, a_cut: float):
    """xa3[b, node_row[i], chans[q]] = xb3[...] + sum_k sb2 K(i, k) W[b * nch + q, k] (see gcl_oi_analysis).
    nodes / stations: (lat f64, lon f64, cos(lat) f32) device triples."""
    B = xb3.shape[0]
    nlat, nlon, ncos = nodes
    slat, slon, scos = stations
    m, nch = slat.numel(), chans.numel()
    assert xb3.stride(2) == 1 and xa3.stride(2) == 1 and W.shape == (B * nch, m) and W.is_contiguous()
    _check(lib().gcl_oi_analysis(_p(xb3), xb3.stride(1), xb3.stride(0), _p(xa3), xa3.stride(1), xa3.stride(0),
                                 _pi(chans), nch, _pi(node_row), _pd(nlat), _pd(nlon), _p(ncos), nlat.numel(),
                                 _pd(slat), _pd(slon), _p(scos), _p(W), m, float(sb2), float(rl2), float(th_cut),
                                 float(a_cut), B, _stream()))
    return xa3


def oi_analysis_rows(xb3, xa3, chans, node_row, nodes, stations, W, sb2_row, rl2_row, th_cut: float, a_cut: float):
    """`oi_analysis` with one (sb2, rl2) per sample: float32 device tables [B] (see gcl_oi_analysis_rows); th_cut /
    a_cut those of the longest correlation length."""
    B = xb3.shape[0]
    nlat, nlon, ncos = nodes
    slat, slon, scos = stations
    m, nch = slat.numel(), chans.numel()
    assert xb3.stride(2) == 1 and xa3.stride(2) == 1 and W.shape == (B * nch, m) and W.is_contiguous()
    assert sb2_row.numel() == B and rl2_row.numel() == B
    _check(lib().gcl_oi_analysis_rows(_p(xb3), xb3.stride(1), xb3.stride(0), _p(xa3), xa3.stride(1), xa3.stride(0),
                                      _pi(chans), nch, _pi(node_row), _pd(nlat), _pd(nlon), _p(ncos), nlat.numel(),
                                      _pd(slat), _pd(slon), _p(scos), _p(W), m, _p(sb2_row), _p(rl2_row),
                                      float(th_cut), float(a_cut), B, _stream()))
    return xa3


# ------------------------------------------------------------------------------------------------------------------
# Forecast scoring and regional blending (csrc/verify.hip)
# ------------------------------------------------------------------------------------------------------------------
def _rows_view(t: torch.Tensor) -> torch.Tensor:
    """A [B, rows, K] float32 view with unit column stride (copies only when the columns are strided)."""
    if t.dtype != torch.float32:
        t = t.float()
    if t.stride(-1) != 1:
        t = t.contiguous()
    return t


def verify_colstats(truth3, preds, rows, stats):
    """Column statistics (see gcl_verify_colstats).  truth3 [B, G, >= K] float32 with unit column stride; preds: up to
    four (tensor [B, G, W] with unit column stride, int32 column map [K] on the device or None); rows int32 [n] or None;
    stats float64 [B, len(preds), K, 3].  K = stats.shape[2]."""
    B, G, _ = truth3.shape
    npred, K = stats.shape[1], stats.shape[2]
    assert 1 <= npred <= 4 and len(preds) == npred and stats.shape == (B, npred, K, 3) and stats.is_contiguous()
    n = rows.numel() if rows is not None else G
    args = []
    for q in range(4):
        if q < npred:
            p, m = preds[q]
            assert p.shape[0] == B and p.stride(2) == 1 and (m is not None or p.shape[2] >= K)
            assert m is None or (m.dtype == torch.int32 and m.numel() == K)
            args += [_p(p), p.stride(1), p.stride(0), _pi(m)]
        else:
            args += [None, 0, 0, None]
    nbytes = int(lib().gcl_verify_colstats_ws_bytes(n, K, npred, B))
    ws = workspace(nbytes, truth3.device)
    _check(lib().gcl_verify_colstats(_p(truth3), truth3.stride(1), truth3.stride(0), K, npred, *args, _pi(rows), n, B,
                                     _pd(stats), ws.data_ptr(), ws.numel(), _stream()))
    return stats


def verify_accumulate(stats, jobs, state, masks=None):
    """Add column statistics into metrics states (see gcl_verify_accumulate).  jobs int64 [njobs, 8] on the device."""
    assert jobs.is_cuda and jobs.dtype == torch.int64 and jobs.is_contiguous() and jobs.shape[1] == 8
    assert masks is None or (masks.is_cuda and masks.dtype == torch.uint8)
    _check(lib().gcl_verify_accumulate(_pd(stats), jobs.data_ptr(), jobs.shape[0], _pd(state),
                                       masks.data_ptr() if masks is not None else None, _stream()))


def regrid_blend(src3, nlat: int, cell, w, K: int, g3=None, mask=None, r3=None, out3=None):
    """g3[b, i, :K] = bilinear regrid of src3 [B, G_src, >= K] (float32 or float64) through the tables cell int32
    [nt, 2] / w float64 [nt, 4]; with out3 also out3 = mask r3 + (1 - mask) g (see gcl_regrid_blend)."""
    B = src3.shape[0]
    nt = cell.shape[0]
    assert src3.stride(2) == 1 and src3.dtype in (torch.float32, torch.float64) and src3.is_cuda
    assert cell.dtype == torch.int32 and cell.is_contiguous() and w.shape == (nt, 4)
    f64 = src3.dtype == torch.float64
    for t in (g3, r3, out3):
        assert t is None or (t.shape[0] == B and t.shape[1] == nt and t.shape[2] >= K and t.stride(2) == 1)
    if out3 is not None:
        assert mask is not None and r3 is not None and mask.numel() == nt and mask.is_contiguous()
    assert g3 is not None or out3 is not None
    if nt == 0:  # no target row: the empty views have null data_ptr()s, which the C entry point takes for absent
        return

    def lb(t):
        return (t.stride(1), t.stride(0)) if t is not None else (0, 0)
    _check(lib().gcl_regrid_blend(src3.data_ptr(), int(f64), src3.stride(1), src3.stride(0), int(nlat), _pi(cell),
                                  _pd(w), nt, int(K), _p(g3), *lb(g3), _p(mask), _p(r3), *lb(r3), _p(out3), *lb(out3),
                                  B, _stream()))


def taper_blend(mask, r3, g3, out3):
    """out3 = mask r3 + (1 - mask) g3 (float32, see gcl_taper_blend); mask [nt] per row."""
    B, nt, K = out3.shape
    assert r3.shape == out3.shape and g3.shape == out3.shape and mask.numel() == nt and mask.is_contiguous()
    assert r3.stride(2) == 1 and g3.stride(2) == 1 and out3.stride(2) == 1
    if out3.numel() == 0:  # as in `regrid_blend`
        return out3
    _check(lib().gcl_taper_blend(_p(mask), _p(r3), r3.stride(1), r3.stride(0), _p(g3), g3.stride(1), g3.stride(0),
                                 _p(out3), out3.stride(1), out3.stride(0), nt, K, B, _stream()))
    return out3


def multires_window_pack(gseries, rseries, rank, n_kept: int, n_reg: int, corner, w, t0, off_g: int, off_r: int, mean,
                         std, C: int, obs: int, pred: int, quantize: bool = True, out=None, out_f16: bool = False):
    """Windows of the flat multires node set (see gcl_multires_window_pack).  gseries fp16 [Tg, n_lon, n_lat, Ct];
    rseries fp16 [Tr, rn_lon, rn_lat, Ct] (merge mode) or None (interpolate mode: corner int32 [n_reg, 4], w float64
    [n_reg, 4]); rank int32 [n_lat * n_lon]; t0 int64 [B] on the GPU; mean / std float32 [>= C] or both None.  Returns
    X [B, N, obs*C] and Y [B, N, pred*C] (None when pred == 0), float32 or (out_f16) float16; out = (X, Y) fills
    contiguous buffers of those shapes in place."""
    for s in (gseries, rseries):
        assert s is None or (s.is_cuda and s.dtype == torch.float16 and s.is_contiguous() and s.dim() == 4)
    assert t0.is_cuda and t0.dtype == torch.int64 and t0.is_contiguous()
    Tg, n_lon, n_lat, Ctg = gseries.shape
    Tr, rn_lon, rn_lat, Ctr = rseries.shape if rseries is not None else (0, 0, 0, 0)
    assert rank.numel() == n_lon * n_lat
    if rseries is None and n_reg:
        assert corner.shape == (n_reg, 4) and w.shape == (n_reg, 4)
    B, N = t0.numel(), n_kept + n_reg
    dt = torch.float16 if out_f16 else torch.float32
    if out is not None:
        X, Y = out
        assert X.is_contiguous() and X.shape == (B, N, obs * C) and X.dtype == dt and X.device == gseries.device
        assert pred == 0 or (Y.is_contiguous() and Y.shape == (B, N, pred * C) and Y.dtype == dt and Y.device == X.device)
    else:
        X = torch.empty(B, N, obs * C, dtype=dt, device=gseries.device)
        Y = torch.empty(B, N, pred * C, dtype=dt, device=gseries.device) if pred > 0 else None
    _check(lib().gcl_multires_window_pack(
        gseries.data_ptr(), Tg, n_lon, n_lat, Ctg, rseries.data_ptr() if rseries is not None else None, Tr, rn_lon,
        rn_lat, Ctr, _pi(rank), int(n_kept), int(n_reg), _pi(corner), _pd(w) if w is not None else None, t0.data_ptr(),
        int(off_g), int(off_r), _p(mean), _p(std), int(C), int(obs), int(pred), int(bool(quantize)), int(out_f16),
        X.data_ptr(), Y.data_ptr() if pred > 0 else None, B, _stream()))
    return X, Y


def pipeline_roi_phys(pred2, x_last2, rows, row0: int, G: int, mean, std, t_idx: int, z_idx: int, elev: float,
                      lapse_f64: bool, raw, lapse=None):
    """raw / lapse [G, C] from the model output pred2 [N, >= C] (see gcl_pipeline_roi_phys)."""
    C = raw.shape[1]
    assert pred2.dim() == 2 and pred2.stride(1) == 1 and pred2.shape[1] >= C and raw.shape == (G, C) and raw.is_contiguous()
    assert x_last2 is None or (x_last2.dim() == 2 and x_last2.stride(1) == 1 and x_last2.shape[0] == pred2.shape[0])
    assert lapse is None or (lapse.shape == raw.shape and lapse.is_contiguous())
    assert (rows.numel() == G) if rows is not None else (0 <= row0 and row0 + G <= pred2.shape[0])
    _check(lib().gcl_pipeline_roi_phys(_p(pred2), pred2.stride(0), _p(x_last2), x_last2.stride(0) if x_last2 is not None
                                       else 0, _pi(rows), int(row0), int(G), C, _p(mean), _p(std), int(t_idx), int(z_idx),
                                       float(elev), int(bool(lapse_f64)), _p(raw), _p(lapse), _stream()))
    return raw, lapse


def pipeline_lapse(x3, t_idx: int, z_idx: int, elev: float, lapse_f64: bool):
    """The lapse-corrected copy of contiguous x3 [G, S, C] (see gcl_pipeline_lapse)."""
    assert x3.dim() == 3 and x3.is_contiguous()
    G, S, C = x3.shape
    out = torch.empty_like(x3)
    _check(lib().gcl_pipeline_lapse(_p(x3), _p(out), G, S, C, int(t_idx), int(z_idx), float(elev), int(bool(lapse_f64)),
                                    _stream()))
    return out


def pipeline_lapse_geopotential(x3, t_idx: int, z_idx: int, elev: float, out=None):
    """The copy of contiguous x3 [G, S, C] corrected by the lapse formula of scripts/mos_idw_sweep_v2.py (see
    gcl_pipeline_lapse_geopotential)."""
    assert x3.dim() == 3 and x3.is_contiguous()
    G, S, C = x3.shape
    if out is None:
        out = torch.empty_like(x3)
    assert out.shape == x3.shape and out.is_contiguous()
    _check(lib().gcl_pipeline_lapse_geopotential(_p(x3), _p(out), G, S, C, int(t_idx), int(z_idx), float(elev),
                                                 _stream()))
    return out


def pipeline_station_obs(truth2, stn, out=None):
    """NaN field [G, C] with the rows stn (int32, device) of truth2 [G, C] (see gcl_pipeline_station_obs)."""
    G, C = truth2.shape
    assert truth2.stride(1) == 1
    if out is None:
        out = torch.empty(G, C, dtype=torch.float32, device=truth2.device)
    assert out.shape == (G, C) and out.is_contiguous()
    _check(lib().gcl_pipeline_station_obs(_p(truth2), truth2.stride(0), _pi(stn), stn.numel(), G, C, _p(out), _stream()))
    return out


def pipeline_sqerr(preds3, truth2, stn, h: int, acc_grid, acc_stn=None):
    """acc_grid[v, h, :] += column sums of (preds3[v] - truth2)^2, acc_stn the same over the rows stn (see
    gcl_pipeline_sqerr).  preds3 [V, G, C] with unit column stride, accumulators float64 [V, H, C]."""
    V, G, C = preds3.shape
    assert preds3.stride(2) == 1 and truth2.shape == (G, C) and truth2.stride(1) == 1
    assert acc_grid.shape[0] == V and acc_grid.shape[2] == C and (acc_stn is None or acc_stn.shape == acc_grid.shape)
    _check(lib().gcl_pipeline_sqerr(_p(preds3), preds3.stride(0), preds3.stride(1), V, _p(truth2), truth2.stride(0),
                                    _pi(stn), stn.numel() if stn is not None else 0, G, C, acc_grid.shape[1], int(h),
                                    _pd(acc_grid), _pd(acc_stn) if acc_stn is not None else None, _stream()))


def mos_idw_sweep_max_configs() -> int:
    """The most (power, radius) settings one gcl_mos_idw_sweep call takes."""
    return int(lib().gcl_mos_idw_sweep_max_configs())


def mos_idw_sweep(pred4, truth3, t2m: int, node_lat, node_lon, pt_idx, bias, idw: bool, power, radius, acc, h0: int = 0,
                  fields_out=None, n_out=None, ws=None):
    """acc[p, h0 + s] += sum over b, g of (y_p[b, g, s] - truth3[b, g, s])^2 for the P settings (power[p], radius[p]),
    y_p the t2m that gcl_mos_idw_apply writes for setting p (see gcl_mos_idw_sweep).  pred4 [B, G, steps, C] float32 or
    float64 with unit channel stride; truth3 [B, G, steps] of the same dtype, any strides; bias float64 [B, K, steps];
    power / radius float64 device tensors [P]; acc float64 [P, H].  fields_out [P, B, G, steps] (pred4's dtype) and
    n_out int32 [P, B] (zeroed by the caller) are optional.  ws: a uint8 workspace (default: the shared one)."""
    B, G, S, _ = pred4.shape
    P, K = power.numel(), pt_idx.numel()
    assert pred4.is_cuda and pred4.dtype in (torch.float32, torch.float64) and pred4.stride(3) == 1
    assert truth3.is_cuda and truth3.dtype == pred4.dtype and truth3.shape == (B, G, S)
    assert bias.shape == (B, K, S) and radius.numel() == P and acc.dim() == 2 and acc.shape[0] == P
    assert fields_out is None or (fields_out.shape == (P, B, G, S) and fields_out.dtype == pred4.dtype
                                  and fields_out.is_cuda and fields_out.is_contiguous())
    assert n_out is None or n_out.shape == (P, B)
    need = int(lib().gcl_mos_idw_sweep_ws_bytes(G, P, S, B))
    if ws is None:
        ws = workspace(need, pred4.device)
    _check(lib().gcl_mos_idw_sweep(
        pred4.data_ptr(), int(pred4.dtype == torch.float64), pred4.stride(0), pred4.stride(1), pred4.stride(2),
        truth3.data_ptr(), truth3.stride(0), truth3.stride(1), truth3.stride(2), G, S, int(t2m),
        _pd(node_lat) if node_lat is not None else None, _pd(node_lon) if node_lon is not None else None, _pi(pt_idx),
        K, _pd(bias), int(bool(idw)), _pd(power), _pd(radius), P, _pd(acc), acc.shape[1], int(h0),
        fields_out.data_ptr() if fields_out is not None else None, _pi(n_out), ws.data_ptr(), ws.numel(), B, _stream()))
    return acc


# ------------------------------------------------------------------------------------------------------------------
# Per-grid-point error maps (csrc/maps.hip)
# ------------------------------------------------------------------------------------------------------------------
MAPS_SUM_E, MAPS_SUM_SQ, MAPS_SUM_ABS, MAPS_SUM_PT = 1, 2, 4, 8
MAPS_RMSE, MAPS_MAE, MAPS_BIAS, MAPS_ACC, MAPS_SKILL = 0, 1, 2, 3, 4


def _maps_layout(truth3, pred3, pmap, rows, conv, flags, K: int):
    B, G, W = truth3.shape
    assert truth3.is_cuda and truth3.stride(2) == 1 and W >= K
    assert pred3.shape[0] == B and pred3.shape[1] == G and pred3.stride(2) == 1 and (pmap is not None or pred3.shape[2] >= K)
    assert pmap is None or pmap.numel() == K
    assert (conv is None) == (flags is None)
    assert conv is None or (conv.shape == (K, 4) and conv.is_contiguous() and flags.numel() == K)
    return B, (rows.numel() if rows is not None else G)


def maps_colstats(truth3, pred3, pmap, rows, conv, flags, cs):
    """Per-sample field mean and unbiased std of the converted prediction and truth (see gcl_maps_colstats).  truth3
    [B, G, >= K] and pred3 [B, G, W] float32 with unit column stride; pmap int32 [K] or None; rows int32 [n] or None;
    conv float32 [K, 4] with flags int32 [K], or both None; cs float64 [B, K, 4]."""
    K = cs.shape[1]
    B, n = _maps_layout(truth3, pred3, pmap, rows, conv, flags, K)
    assert cs.shape == (B, K, 4)
    ws = workspace(int(lib().gcl_maps_colstats_ws_bytes(n, K, B)), truth3.device)
    _check(lib().gcl_maps_colstats(_p(truth3), truth3.stride(1), truth3.stride(0), _p(pred3), pred3.stride(1),
                                   pred3.stride(0), _pi(pmap), K, _p(conv), _pi(flags), _pi(rows), n, B, _pd(cs),
                                   ws.data_ptr(), ws.numel(), _stream()))
    return cs


def maps_accumulate(truth3, pred3, pmap, rows, conv, flags, cs, sums: int, C: int, state, count):
    """Add a batch into the float64 map state [leads, nsums, n * C] and B into count (int64 [1], on the device); see
    gcl_maps_accumulate.  cs: the result of `maps_colstats` (None without the ACC sum)."""
    leads, nsums, nE = state.shape
    assert nsums == bin(sums).count("1") and count.is_cuda and count.dtype == torch.int64 and count.numel() == 1
    B, n = _maps_layout(truth3, pred3, pmap, rows, conv, flags, leads * C)
    assert nE == n * C
    _check(lib().gcl_maps_accumulate(_p(truth3), truth3.stride(1), truth3.stride(0), _p(pred3), pred3.stride(1),
                                     pred3.stride(0), _pi(pmap), leads, C, _p(conv), _pi(flags), _pi(rows), n, B,
                                     _pd(cs) if cs is not None else None, int(sums), _pd(state), count.data_ptr(),
                                     _stream()))


def maps_finalize(state, count, plane: int, kind: int, out, ref_state=None, ref_count=None, ref_plane: int = 0):
    """out float32 [leads, n * C] = the map of `kind` from sum `plane` of the state (see gcl_maps_finalize)."""
    leads, nsums, nE = state.shape
    assert out.is_contiguous() and out.numel() == leads * nE
    assert ref_state is None or (ref_state.shape[0] == leads and ref_state.shape[2] == nE)
    _check(lib().gcl_maps_finalize(_pd(state), count.data_ptr(), int(plane), nsums, leads, nE, int(kind),
                                   _pd(ref_state) if ref_state is not None else None,
                                   ref_count.data_ptr() if ref_count is not None else None, int(ref_plane),
                                   ref_state.shape[1] if ref_state is not None else 0, _p(out), _stream()))
    return out


def maps_convert(x, conv, flags):
    """A new tensor: x [..., K] float32 converted column by column (see gcl_maps_convert)."""
    K = conv.shape[0]
    assert conv.shape == (K, 4) and conv.is_contiguous() and flags.numel() == K and x.shape[-1] == K
    x = x.contiguous()
    out = torch.empty_like(x)
    _check(lib().gcl_maps_convert(_p(x), _p(out), x.numel(), K, _p(conv), _pi(flags), _stream()))
    return out


def _room(t: torch.Tensor) -> int:
    """Elements of t's storage from its first element on."""
    return t.untyped_storage().nbytes() // t.element_size() - t.storage_offset()


def live_max_dest() -> int:
    """The most window slots one gcl_live_frame_pack call fills."""
    return int(lib().gcl_live_max_dest())


def live_frame_pack(arena, statics, chan, chan_div, pos, w, mean, std, out, dests, ldo: int, G: int, C: int):
    """One analysis cycle into the window slots `out + dests[d] + g * ldo + c` (see gcl_live_frame_pack).  arena float32
    [n] or None; statics float32 [n_static, G] or None; chan int64 [C, 3]; chan_div float32 [C]; pos int32 / w float64
    [n_tab, G, 4] or None; mean / std float32 [>= C]; dests: element offsets from out's first element (host ints).
    Every destination is checked against out's storage here; the positions are the table builder's to validate."""
    assert chan.is_cuda and chan.dtype == torch.int64 and chan.shape == (C, 3) and chan.is_contiguous()
    assert chan_div.shape == (C,) and chan_div.is_contiguous() and mean.numel() >= C and std.numel() >= C
    assert out.is_cuda and out.dtype == torch.float32
    if pos is not None:
        assert arena is not None and arena.is_contiguous() and arena.dim() == 1
        assert pos.dim() == 3 and pos.shape[1:] == (G, 4) and w.shape == pos.shape and pos.is_contiguous() and w.is_contiguous()
    if statics is not None:
        assert statics.dim() == 2 and statics.shape[1] == G and statics.is_contiguous()
    dests = [int(d) for d in dests]
    if not 1 <= len(dests) <= live_max_dest():
        raise ValueError(f"live_frame_pack: {len(dests)} destinations (1 .. {live_max_dest()})")
    if ldo < C or min(dests) < 0 or max(dests) + (G - 1) * int(ldo) + C > _room(out):
        raise ValueError(f"live_frame_pack: destinations {dests} with row stride {ldo} leave the output buffer")
    offs = (_i64 * len(dests))(*dests)
    _check(lib().gcl_live_frame_pack(_p(arena), _p(statics), chan.data_ptr(), _p(chan_div), _pi(pos),
                                     _pd(w) if w is not None else None, _p(mean), _p(std), out.data_ptr(), offs,
                                     len(dests), int(ldo), int(G), int(C), _stream()))
    return out


def live_region_stats(pred4, rows, chans, offs, out=None, validated: bool = False):
    """float64 [B, S, nc, 3] = mean, min, max over the rows `rows` (int32, device) of pred4[b, rows, s, chans[k]]
    (+ offs[k]) (see gcl_live_region_stats).  pred4 float32 [B, G, S, C], unit channel stride; chans int32 [nc], offs
    float32 [nc] on the device.  An empty row list raises.  rows and chans are checked against G and C here, which
    reads them back (one synchronise); a caller that built them from host data it has checked passes validated=True."""
    assert pred4.dim() == 4 and pred4.stride(3) == 1
    B, G, S, Cc = pred4.shape
    n, nc = rows.numel(), chans.numel()
    if n == 0:
        raise ValueError("live_region_stats: empty row list (the reference writes no city block then)")
    if nc == 0:
        raise ValueError("live_region_stats: no channels listed")
    if not validated:
        r, c = rows.cpu(), chans.cpu()
        if int(r.min()) < 0 or int(r.max()) >= G:
            raise ValueError(f"live_region_stats: a row index lies outside the {G} nodes")
        if int(c.min()) < 0 or int(c.max()) >= Cc:
            raise ValueError(f"live_region_stats: a channel index lies outside the {Cc} channels")
    assert offs.numel() == nc and rows.is_contiguous() and chans.is_contiguous() and offs.is_contiguous()
    if out is None:
        out = torch.empty(B, S, nc, 3, dtype=torch.float64, device=pred4.device)
    assert out.shape == (B, S, nc, 3) and out.dtype == torch.float64 and out.is_contiguous() and out.is_cuda
    _check(lib().gcl_live_region_stats(_p(pred4), pred4.stride(0), pred4.stride(1), pred4.stride(2), _pi(rows), n,
                                       _pi(chans), _p(offs), nc, S, out.data_ptr(), B, _stream()))
    return out


DATASET_NAN_TO_ZERO, DATASET_INF_TO_ZERO = 1, 2  # flag bits of gcl_dataset_stats


def dataset_max_sources() -> int:
    """The most source planes one gcl_dataset_pack call takes."""
    return int(lib().gcl_dataset_max_sources())


def _series_shape(series):
    """(T, n_lon, n_lat, Ct) of a contiguous fp16 series [T, lon, lat, Ct] or flat [T, N, Ct] on the GPU."""
    assert series.is_cuda and series.dtype == torch.float16 and series.is_contiguous() and series.dim() in (3, 4)
    if series.dim() == 3:
        return series.shape[0], series.shape[1], 1, series.shape[2]
    return tuple(series.shape)


def _dataset_ws(C: int, device):
    ws = workspace(lib().gcl_dataset_ws_bytes(int(C)), device)
    return ws.data_ptr(), ws.numel()


def dataset_pack(sources, chans, scales, nt: int, series, t0: int, sums, sumsq, grid=None):
    """One time block of float32 planes into rows [t0, t0 + nt) of `series`, with the block's sums (see
    gcl_dataset_pack).  sources: contiguous float32 GPU tensors, [nt, lon, lat] / [nt, P] or, time-invariant, [lon, lat]
    / [P]; chans / scales: their destination channels and float32 factors (host).  sums / sumsq: float64 [Ct] on the
    GPU, written at the listed channels.  series None: the sums alone, on the grid = (n_lon, n_lat, Ct) given."""
    if series is not None:
        T, n_lon, n_lat, Ct = _series_shape(series)
    else:
        (n_lon, n_lat, Ct), T, t0 = grid, int(nt), 0
    P, n = n_lon * n_lat, len(sources)
    if not (1 <= n <= dataset_max_sources() and len(chans) == n and len(scales) == n):
        raise ValueError(f"dataset_pack: {n} sources (1 .. {dataset_max_sources()}), {len(chans)} channels, "
                         f"{len(scales)} factors")
    strides = []
    for x in sources:
        assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous(), "dataset_pack: float32 contiguous GPU planes"
        if x.numel() == nt * P:
            strides.append(P)
        elif x.numel() == P:
            strides.append(0)
        else:
            raise ValueError(f"dataset_pack: a source of {tuple(x.shape)} is neither [{nt}, {P}] nor [{P}]")
    for t in (sums, sumsq):
        assert t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and t.numel() == Ct
    dev = sources[0].device
    ws, ws_bytes = _dataset_ws(Ct, dev)
    _check(lib().gcl_dataset_pack((_vp * n)(*[x.data_ptr() for x in sources]), (_i64 * n)(*strides),
                                  (_i32 * n)(*[int(c) for c in chans]), (_f32 * n)(*[float(s) for s in scales]), n,
                                  int(nt), n_lon, n_lat, series.data_ptr() if series is not None else None, T, Ct,
                                  int(t0), sums.data_ptr(), sumsq.data_ptr(), ws, ws_bytes, _stream()))


def dataset_stats(series, t_s: int, t_e: int, flags: int = 0, out=None):
    """(sum f64, sumsq f64, min f32, max f32, n_nan i64, n_inf i64), each [Ct] on the GPU, of rows [t_s, t_e) of the
    fp16 series (see gcl_dataset_stats).  out: such a tuple to fill."""
    T, n_lon, n_lat, Ct = _series_shape(series)
    if out is None:
        mk = lambda dt: torch.empty(Ct, dtype=dt, device=series.device)  # noqa: E731
        out = (mk(torch.float64), mk(torch.float64), mk(torch.float32), mk(torch.float32), mk(torch.int64),
               mk(torch.int64))
    for t, dt in zip(out, (torch.float64, torch.float64, torch.float32, torch.float32, torch.int64, torch.int64)):
        assert t.is_cuda and t.dtype == dt and t.is_contiguous() and t.numel() == Ct
    ws, ws_bytes = _dataset_ws(Ct, series.device)
    _check(lib().gcl_dataset_stats(series.data_ptr(), T, n_lon, n_lat, Ct, int(t_s), int(t_e), int(flags),
                                   *[t.data_ptr() for t in out], ws, ws_bytes, _stream()))
    return out


def dataset_welford(mean, m2, n, block_sum, block_sumsq, block_n: int):
    """The reference's welford_update on device state: mean / m2 float64 [C], n int64 [1] (see gcl_dataset_welford)."""
    Cn = mean.numel()
    for t in (mean, m2, block_sum, block_sumsq):
        assert t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and t.numel() == Cn
    assert n.is_cuda and n.dtype == torch.int64 and n.numel() == 1
    _check(lib().gcl_dataset_welford(mean.data_ptr(), m2.data_ptr(), n.data_ptr(), block_sum.data_ptr(),
                                     block_sumsq.data_ptr(), int(block_n), Cn, _stream()))


def dataset_widen(src, extra, out=None):
    """[T, ..., Ct + K] fp16 from src [T, ..., Ct] and extra [T, K] fp16 (see gcl_dataset_widen)."""
    T, n_lon, n_lat, Ct = _series_shape(src)
    assert extra.is_cuda and extra.dtype == torch.float16 and extra.is_contiguous() and extra.dim() == 2
    assert extra.shape[0] == T and extra.shape[1] >= 1
    Cn = Ct + extra.shape[1]
    if out is None:
        out = torch.empty(*src.shape[:-1], Cn, dtype=torch.float16, device=src.device)
    assert out.is_cuda and out.dtype == torch.float16 and out.is_contiguous() and out.shape == (*src.shape[:-1], Cn)
    _check(lib().gcl_dataset_widen(src.data_ptr(), T, n_lon, n_lat, Ct, extra.data_ptr(), Cn, out.data_ptr(), _stream()))
    return out


WRF_POINT, WRF_SRC0, WRF_SRC1, WRF_POINT64, WRF_CONVERT = 0, 1, 2, 3, 4  # side kinds of a gcl_wrf_scores job


class WrfSource:
    """A source of grid fields for gcl_wrf_sample / gcl_wrf_scores: `values` a float32 or fp16 GPU tensor read in place,
    `node_stride` the elements between two nodes of a field, `n_nodes` the nodes of a field, pos int32 / w float64
    [P, 4] its point table on the GPU (from wrf.wrf_point_tables: every position below n_nodes, negative = outside)."""

    def __init__(self, values, node_stride: int, n_nodes: int, pos, w):
        if not values.is_cuda or values.dtype not in (torch.float32, torch.float16):
            raise RuntimeError("libgcl_hip needs float32 or fp16 GPU tensors as WRF sources (there is no CPU fallback)")
        if pos.dim() != 2 or pos.shape[1] != 4 or w.shape != pos.shape:
            raise ValueError(f"WrfSource: point table of shapes {tuple(pos.shape)} / {tuple(w.shape)}, expected [P, 4]")
        if node_stride < 1 or n_nodes < 1:
            raise ValueError(f"WrfSource: node stride {node_stride}, {n_nodes} nodes")
        self.values, self.node_stride, self.n_nodes, self.pos, self.w = values, int(node_stride), int(n_nodes), pos, w
        self.half = int(values.dtype == torch.float16)
        self.P = int(pos.shape[0])

    def check_offsets(self, offs, what: str):
        """Every field at the element offsets `offs` (host ints) lies inside the storage of `values`."""
        if len(offs) and (min(offs) < 0 or max(offs) + (self.n_nodes - 1) * self.node_stride >= _room(self.values)):
            raise ValueError(f"{what}: a field offset in [{min(offs)}, {max(offs)}] with node stride {self.node_stride} "
                             f"and {self.n_nodes} nodes leaves the source buffer")

    def args(self):
        return (self.values.data_ptr(), self.half, self.node_stride, _pi(self.pos), _pd(self.w))


def wrf_sample(source: WrfSource, field_off, field_off_dev=None, mul=None, add=None, out=None):
    """float64 [nf, P]: the fields of `source` at the element offsets field_off (host ints) on its point table, NaN
    outside the source axes (see gcl_wrf_sample).  mul / add: float32 [nf] GPU tensors (both or neither), the
    conversion applied to every source value first.  field_off_dev: the same offsets as an int64 GPU tensor, for a
    caller that keeps them there."""
    offs = [int(o) for o in field_off]
    nf = len(offs)
    if nf == 0:
        raise ValueError("wrf_sample: no fields listed")
    source.check_offsets(offs, "wrf_sample")
    if (mul is None) != (add is None):
        raise ValueError("wrf_sample: mul and add go together")
    dev = source.values.device
    if field_off_dev is None:
        field_off_dev = torch.tensor(offs, dtype=torch.int64, device=dev)
    assert field_off_dev.is_cuda and field_off_dev.dtype == torch.int64 and field_off_dev.numel() == nf
    if mul is not None:
        assert mul.numel() == nf and add.numel() == nf and mul.is_contiguous() and add.is_contiguous()
    if out is None:
        out = torch.empty(nf, source.P, dtype=torch.float64, device=dev)
    assert out.shape == (nf, source.P) and out.is_contiguous()
    _check(lib().gcl_wrf_sample(*source.args()[:3], field_off_dev.data_ptr(), _p(mul), _p(add), nf, *source.args()[3:],
                                source.P, _pd(out), _stream()))
    return out


def wrf_scores(P: int, jobs, conv, jobs_dev=None, conv_dev=None, src0=None, src1=None, pts=None, pts64=None, slots=None,
               offsets=None, target: int = 0, filled=None, accumulate: bool = False, out=None, validated: bool = False):
    """float64 [S, 6] = n, sum d, sum d^2, sum |d|, sum a, sum b of the NaN-masked pairs of every job (see
    gcl_wrf_scores).  pts float32 / pts64 float64: the arenas of the point fields.  jobs: host rows (kind a, offset a,
    kind b, offset b, gated, delta), conv: host rows (mul a, add a, mul b, add b); every offset is checked here against the side's buffer.  jobs_dev / conv_dev: the same tables on the
    GPU (int64 [J, 6] / float32 [J, 4]) for a caller that keeps them there.  slots: S (default J: one slot per job);
    offsets int64 [J / S] and filled int32 [S] on the GPU serve the gated jobs.  validated: the caller has checked this
    job table against these buffers already (a table it reuses every step)."""
    J = len(jobs)
    if J == 0 or len(conv) != J:
        raise ValueError(f"wrf_scores: {J} jobs, {len(conv)} conversion rows")
    S = J if slots is None else int(slots)
    if S < 1 or J % S:
        raise ValueError(f"wrf_scores: {J} jobs do not fill {S} slots evenly")
    srcs = (src0, src1)
    by_side = {0: [], 1: [], 2: [], 3: []}
    gated = validated and offsets is not None
    for row in ([] if validated else jobs):
        if len(row) != 6:
            raise ValueError("wrf_scores: a job is (kind a, offset a, kind b, offset b, gated, delta)")
        for kind, off in ((row[0], row[1]), (row[2], row[3])):
            if not 0 <= int(kind) < 8:
                raise ValueError(f"wrf_scores: unknown side kind {kind}")
            by_side[int(kind) & 3].append(int(off))
        gated = gated or bool(row[4])
    for k in (1, 2):
        if by_side[k]:
            if srcs[k - 1] is None:
                raise ValueError(f"wrf_scores: a job reads source {k - 1}, which is not given")
            if srcs[k - 1].P != P:
                raise ValueError(f"wrf_scores: source {k - 1} has a table of {srcs[k - 1].P} points, the jobs {P}")
            srcs[k - 1].check_offsets(by_side[k], f"wrf_scores source {k - 1}")
    if by_side[0]:
        if pts is None:
            raise ValueError("wrf_scores: a job reads a point field, and pts is not given")
        assert pts.is_contiguous()
        if min(by_side[0]) < 0 or max(by_side[0]) + P > pts.numel():
            raise ValueError(f"wrf_scores: a point field of {P} values leaves pts ({pts.numel()} values)")
    if by_side[3]:
        if pts64 is None:
            raise ValueError("wrf_scores: a job reads a float64 point field, and pts64 is not given")
        if min(by_side[3]) < 0 or max(by_side[3]) + P > pts64.numel():
            raise ValueError(f"wrf_scores: a point field of {P} values leaves pts64 ({pts64.numel()} values)")
    if gated:
        if offsets is None or filled is None:
            raise ValueError("wrf_scores: gated jobs need offsets and filled")
        assert offsets.is_cuda and offsets.dtype == torch.int64 and offsets.is_contiguous() and offsets.numel() == J // S
        assert filled.is_cuda and filled.dtype == torch.int32 and filled.is_contiguous() and filled.numel() == S
    dev = next(t for t in (pts, pts64, src0 and src0.values, src1 and src1.values) if t is not None).device
    if jobs_dev is None:
        jobs_dev = torch.tensor([[int(v) for v in r] for r in jobs], dtype=torch.int64, device=dev)
        conv_dev = torch.tensor([[float(v) for v in r] for r in conv], dtype=torch.float32, device=dev)
    assert jobs_dev.is_cuda and jobs_dev.dtype == torch.int64 and jobs_dev.shape == (J, 6) and jobs_dev.is_contiguous()
    assert conv_dev.is_cuda and conv_dev.dtype == torch.float32 and conv_dev.shape == (J, 4) and conv_dev.is_contiguous()
    if out is None:
        if accumulate:
            raise ValueError("wrf_scores: accumulate needs the state to add to")
        out = torch.empty(S, 6, dtype=torch.float64, device=dev)
    assert out.numel() == S * 6 and out.is_contiguous()
    nbytes = int(lib().gcl_wrf_scores_ws_bytes(J, int(P)))
    ws = workspace(nbytes, dev)
    none = (None, 0, 0, None, None)
    _check(lib().gcl_wrf_scores(*(src0.args() if src0 is not None else none),
                                *(src1.args() if src1 is not None else none), _p(pts),
                                _pd(pts64) if pts64 is not None else None, jobs_dev.data_ptr(),
                                _p(conv_dev), J, S, int(P), offsets.data_ptr() if gated else None, int(target),
                                _pi(filled) if gated else None, int(bool(accumulate)), _pd(out), ws.data_ptr(),
                                ws.numel(), _stream()))
    return out


def wrf_box_means(x3, rows, n_rows_total: int, std, mean, out=None, count=None, validated: bool = False):
    """float32 [B, K]: the mean over the listed rows of x3[s, rows[r], k] * std[k % C] + mean[k % C] in numpy's float32
    order (see gcl_wrf_box_means).  x3 float32 [B, G, K] with unit column stride; rows int32 on the GPU; std / mean
    float32 [C] on the GPU, K a multiple of C.  With `count` (int64 [1] on the GPU) the rows go to out[count + s] of an
    out [cap, K]; rows past cap are dropped.  rows are checked against G here, which reads them back (one
    synchronise); a caller that built them from host data it has checked passes validated=True."""
    assert x3.dim() == 3 and x3.stride(2) == 1
    B, G, K = x3.shape
    R, Cc = rows.numel(), std.numel()
    if R == 0:
        raise ValueError("wrf_box_means: empty row list (the mean of no rows is undefined)")
    if Cc == 0 or K % Cc or mean.numel() != Cc:
        raise ValueError(f"wrf_box_means: {K} columns and scalers of {Cc} / {mean.numel()} channels")
    if G != n_rows_total:
        raise ValueError(f"wrf_box_means: the batch has {G} rows, the row list was made for {n_rows_total}")
    if not validated:
        r = rows.cpu()
        if int(r.min()) < 0 or int(r.max()) >= G:
            raise ValueError(f"wrf_box_means: a row index lies outside the {G} nodes")
    assert std.is_contiguous() and mean.is_contiguous()
    if out is None:
        if count is not None:
            raise ValueError("wrf_box_means: count needs the state to write to")
        out = torch.empty(B, K, dtype=torch.float32, device=x3.device)
    assert out.dim() == 2 and out.shape[1] == K and out.stride(1) == 1 and out.dtype == torch.float32 and out.is_cuda
    if count is None and out.shape[0] < B:
        raise ValueError(f"wrf_box_means: out has {out.shape[0]} rows for {B} samples")
    if count is not None:
        assert count.is_cuda and count.dtype == torch.int64 and count.numel() == 1
    _check(lib().gcl_wrf_box_means(_p(x3), x3.stride(0), x3.stride(1), _pi(rows), R, _p(std), _p(mean), Cc, K, B,
                                   out.data_ptr(), out.stride(0), count.data_ptr() if count is not None else None,
                                   out.shape[0], _stream()))
    return out


def _ph(t):
    assert t.is_cuda and t.dtype == torch.float16 and t.is_contiguous()
    return t.data_ptr()


def _pl(t):
    assert t.is_cuda and t.dtype == torch.int64 and t.is_contiguous()
    return t.data_ptr()


def _point_table(pos, w, who: str):
    """P of a device point table pos int32 [P, 4] / w float64 [P, 4]."""
    if pos.dim() != 2 or pos.shape[1] != 4 or tuple(w.shape) != tuple(pos.shape) or pos.shape[0] == 0:
        raise ValueError(f"{who}: a point table is pos int32 [P, 4] and w float64 [P, 4] with P > 0")
    _pi(pos), _pd(w)
    return pos.shape[0]


def downscale_coarse(series, pos, w, t0: int, nt: int, out, to0: int):
    """Frames [t0, t0 + nt) of the fp16 `series` [T, N, C] (or [T, lon, lat, C]) through the point table onto frames
    [to0, to0 + nt) of the fp16 archive `out` [T_out, P, C] (or [T_out, lon, lat, C]); pos / w None: the frames are
    copied (see gcl_downscale_coarse).  The table's positions must lie below N (the caller's tables are checked on the
    host, where they are built)."""
    _ph(series), _ph(out)
    T, Cc = series.shape[0], series.shape[-1]
    N = series.numel() // (T * Cc) if T * Cc else 0
    T_out = out.shape[0]
    P = out.numel() // (T_out * Cc) if T_out * Cc else 0
    if out.shape[-1] != Cc:
        raise ValueError(f"downscale_coarse: {Cc} channels in, {out.shape[-1]} out")
    if (pos is None) != (w is None):
        raise ValueError("downscale_coarse: the positions and the weights of a point table go together")
    if pos is not None and _point_table(pos, w, "downscale_coarse") != P:
        raise ValueError(f"downscale_coarse: a table of {pos.shape[0]} points for frames of {P}")
    _check(lib().gcl_downscale_coarse(series.data_ptr(), T, N, Cc, None if pos is None else pos.data_ptr(),
                                      None if w is None else w.data_ptr(), P, int(t0), int(nt), out.data_ptr(), T_out,
                                      int(to0), _stream()))
    return out


def downscale_pred(pred3, pos, w, std, mean, dest, out, last3=None):
    """The float32 predictions pred3 [B, G, >= C] (unit channel stride; last3 alike: the residual base) through the
    point table, denormalised, into the frames dest (int64 [B] on the GPU) of the fp16 archive out [T_out, P, C] (see
    gcl_downscale_pred).  The table's positions must lie below G."""
    _ph(out)
    B, G, Cc = pred3.shape[0], pred3.shape[1], out.shape[-1]
    T_out = out.shape[0]
    P = _point_table(pos, w, "downscale_pred")
    if out.numel() != T_out * P * Cc:
        raise ValueError(f"downscale_pred: an archive of shape {tuple(out.shape)} for a table of {P} points")
    for x in (pred3,) + ((last3,) if last3 is not None else ()):
        if x.dim() != 3 or x.stride(2) != 1 or x.shape[2] < Cc or x.shape[:2] != (B, G):
            raise ValueError(f"downscale_pred: a [B, G, >= {Cc}] tensor with unit channel stride, got {tuple(x.shape)}")
    if std.numel() != Cc or mean.numel() != Cc or dest.numel() != B:
        raise ValueError(f"downscale_pred: scalers of {std.numel()} / {mean.numel()} channels for {Cc}, {dest.numel()} "
                         f"destinations for {B} samples")
    _check(lib().gcl_downscale_pred(_p(pred3), pred3.stride(0), pred3.stride(1), _p(last3),
                                    last3.stride(0) if last3 is not None else 0,
                                    last3.stride(1) if last3 is not None else 0, pos.data_ptr(), w.data_ptr(), P, Cc, B,
                                    _p(std), _p(mean), _pl(dest), out.data_ptr(), T_out, _stream()))
    return out


def downscale_batch(coarse, fine, t, obs: int, mean, std, static=None, flip=None, neg=None, noise=None,
                    sigma: float = 0.0, out=None):
    """(X [B, obs * C + Ns, H, W], Y [B, C, H, W]) float32 of the samples t (int64 [B] on the GPU) from the fp16
    archives coarse / fine [T, W, H, C] (see gcl_downscale_batch).  static float32 [W, H, Ns]; flip int32 [B]; neg int32
    [C]; noise float32 [B, obs * C, H, W] with its factor sigma.  out: (X, Y) to fill."""
    _ph(coarse), _ph(fine)
    if coarse.dim() != 4 or coarse.shape != fine.shape:
        raise ValueError(f"downscale_batch: archives of {tuple(coarse.shape)} and {tuple(fine.shape)}")
    T, W, Hh, Cc = coarse.shape
    B, Ns = t.numel(), 0 if static is None else static.shape[-1]
    if static is not None and (tuple(static.shape[:2]) != (W, Hh) or not static.is_contiguous()):
        raise ValueError(f"downscale_batch: static fields of {tuple(static.shape)} on a grid of {W} x {Hh}")
    if mean.numel() != Cc or std.numel() != Cc:
        raise ValueError(f"downscale_batch: scalers of {mean.numel()} / {std.numel()} channels for {Cc}")
    if flip is not None and flip.numel() != B or neg is not None and neg.numel() != Cc:
        raise ValueError("downscale_batch: flip is one int32 per sample, neg one per channel")
    if noise is not None and (tuple(noise.shape) != (B, obs * Cc, Hh, W) or not noise.is_contiguous()):
        raise ValueError(f"downscale_batch: noise of {tuple(noise.shape)} for {(B, obs * Cc, Hh, W)}")
    if out is None:
        out = (torch.empty(B, obs * Cc + Ns, Hh, W, dtype=torch.float32, device=coarse.device),
               torch.empty(B, Cc, Hh, W, dtype=torch.float32, device=coarse.device))
    X, Y = out
    assert X.is_contiguous() and Y.is_contiguous() and tuple(X.shape) == (B, obs * Cc + Ns, Hh, W)
    assert tuple(Y.shape) == (B, Cc, Hh, W)
    _check(lib().gcl_downscale_batch(coarse.data_ptr(), fine.data_ptr(), T, W, Hh, Cc, _pl(t), B, int(obs), _p(mean),
                                     _p(std), _p(static), Ns, _pi(flip), _pi(neg), _p(noise), float(sigma), _p(X), _p(Y),
                                     _stream()))
    return X, Y


def downscale_pair_mse(a, b, t, mean, std, out=None):
    """float64 [C, 2] = per channel {elements, sum of d^2} of the normalised difference of the fp16 archives a and b
    [T, ..., C] over the frames t (int64 on the GPU; see gcl_downscale_pair_mse)."""
    _ph(a), _ph(b)
    if a.shape != b.shape or a.dim() < 2:
        raise ValueError(f"downscale_pair_mse: archives of {tuple(a.shape)} and {tuple(b.shape)}")
    T, Cc = a.shape[0], a.shape[-1]
    P = a.numel() // (T * Cc) if T * Cc else 0
    if mean.numel() != Cc or std.numel() != Cc or t.numel() == 0:
        raise ValueError(f"downscale_pair_mse: scalers of {mean.numel()} / {std.numel()} channels for {Cc}, "
                         f"{t.numel()} frames")
    if out is None:
        out = torch.empty(Cc, 2, dtype=torch.float64, device=a.device)
    ws = workspace(lib().gcl_downscale_ws_bytes(Cc), a.device)
    _check(lib().gcl_downscale_pair_mse(a.data_ptr(), b.data_ptr(), T, P, Cc, _pl(t), t.numel(), _p(mean), _p(std),
                                        _pd(out), ws.data_ptr(), ws.numel(), _stream()))
    return out


# ---- the downscaler's objective and scores (csrc/downscale_loss.hip) ---------------------------------------------------
DOWNSCALE_LOSS_MAX_DIM, DOWNSCALE_LOSS_MAX_C = 256, 64
_twiddles = {}


def _twiddle_tables(H: int, W: int, device):
    """(tw_h float64 [H, 2], tw_w float64 [W, 2]) = (cos, sin)(2 pi k / n) on the device, built once in double."""
    import numpy as np

    out = []
    for n in (H, W):
        key = (n, str(torch.device(device)))
        t = _twiddles.get(key)
        if t is None:
            a = 2.0 * np.pi * np.arange(n, dtype=np.float64) / n
            t = torch.from_numpy(np.stack([np.cos(a), np.sin(a)], axis=1)).to(device)
            _twiddles[key] = t
        out.append(t)
    return out


def downscale_loss_check(out, Y, x_last=None, mask=None, who: str = "downscale_loss"):
    """(B, C, H, W) of the operands of the downscaler losses, or an error: everything here is decided from shapes,
    dtypes and devices, before any GPU work."""
    if out.dim() != 4 or out.shape != Y.shape:
        raise ValueError(f"{who}: out and target are [B, C, H, W] of one shape, got {tuple(out.shape)} and {tuple(Y.shape)}")
    B, Cc, Hh, W = (int(v) for v in out.shape)
    if B < 1 or not (2 <= Hh <= DOWNSCALE_LOSS_MAX_DIM and 2 <= W <= DOWNSCALE_LOSS_MAX_DIM):
        raise ValueError(f"{who}: a grid of {Hh} x {W} for {B} samples; H and W lie in 2 .. {DOWNSCALE_LOSS_MAX_DIM}")
    if not 1 <= Cc <= DOWNSCALE_LOSS_MAX_C:
        raise ValueError(f"{who}: {Cc} channels; at most {DOWNSCALE_LOSS_MAX_C} (the limit of gcl_downscale_batch)")
    if mask is not None and (mask.dim() != 1 or mask.numel() != Cc):
        raise ValueError(f"{who}: a channel mask of shape {tuple(mask.shape)} for {Cc} channels")
    if x_last is not None and (tuple(x_last.shape) != (B, Cc, Hh, W)
                               or x_last.stride()[1:] != (Hh * W, W, 1) or x_last.stride(0) < Cc * Hh * W):
        raise ValueError(f"{who}: x_last is a channel slice [B, {Cc}, {Hh}, {W}] of a contiguous X, got shape "
                         f"{tuple(x_last.shape)} with strides {x_last.stride()}")
    for t in (out, Y, x_last, mask):
        _p(t)
    if not (out.is_contiguous() and Y.is_contiguous()):
        raise ValueError(f"{who}: out and target must be contiguous")
    return B, Cc, Hh, W


def downscale_loss_fwd_bwd(out, Y, rec, x_last=None, mask=None, mse_weight: float = 1.0, gradient_weight: float = 0.0,
                           dout=None):
    """rec[0] = mse and rec[1] = grad (float64 [3] on the GPU; a term whose weight is not > 0 is skipped), and
    d(mse_weight * mse + gradient_weight * grad) / d out into dout (see gcl_downscale_loss_fwd_bwd)."""
    B, Cc, Hh, W = downscale_loss_check(out, Y, x_last, mask, "downscale_loss_fwd_bwd")
    assert dout is None or (dout.is_contiguous() and dout.shape == out.shape)
    ws = workspace(lib().gcl_downscale_loss_ws_bytes(0, 0, 0, 0), out.device)
    _check(lib().gcl_downscale_loss_fwd_bwd(_p(out), _p(x_last), x_last.stride(0) if x_last is not None else 0, _p(Y),
                                            _p(mask), B, Cc, Hh, W, float(mse_weight), float(gradient_weight), _pd(rec),
                                            _p(dout), ws.data_ptr(), ws.numel(), _stream()))
    return rec


def downscale_spectral_fwd_bwd(out, Y, rec, x_last=None, mask=None, spectral_weight: float = 1.0, dout=None,
                               accumulate: bool = False):
    """rec[2] = spec, and spectral_weight * d spec / d out added to (accumulate) or stored in dout (see
    gcl_downscale_spectral_fwd_bwd)."""
    B, Cc, Hh, W = downscale_loss_check(out, Y, x_last, mask, "downscale_spectral_fwd_bwd")
    assert dout is None or (dout.is_contiguous() and dout.shape == out.shape)
    tw_h, tw_w = _twiddle_tables(Hh, W, out.device)
    ws = workspace(lib().gcl_downscale_loss_ws_bytes(B, Cc, Hh, W), out.device)
    _check(lib().gcl_downscale_spectral_fwd_bwd(_p(out), _p(x_last), x_last.stride(0) if x_last is not None else 0, _p(Y),
                                                _p(mask), _pd(tw_h), _pd(tw_w), B, Cc, Hh, W, float(spectral_weight),
                                                1 if accumulate else 0, _pd(rec), _p(dout), ws.data_ptr(), ws.numel(),
                                                _stream()))
    return rec


def downscale_metrics(out, x_last, Y, residual: bool, state, count):
    """One batch of compute_metrics: state float64 [C, 2] += the per-batch means of (o - Y)^2 and (x_last - Y)^2, count
    (int64 [1] on the GPU) += 1 (see gcl_downscale_metrics)."""
    if out.dim() != 4 or out.shape != Y.shape or x_last.shape != out.shape:
        raise ValueError(f"downscale_metrics: out, x_last and Y are [B, C, H, W] of one shape, got {tuple(out.shape)}, "
                         f"{tuple(x_last.shape)} and {tuple(Y.shape)}")
    B, Cc, Hh, W = (int(v) for v in out.shape)
    if not 1 <= Cc <= DOWNSCALE_LOSS_MAX_C or B < 1:
        raise ValueError(f"downscale_metrics: {Cc} channels for {B} samples; at most {DOWNSCALE_LOSS_MAX_C} channels")
    if x_last.stride()[1:] != (Hh * W, W, 1) or x_last.stride(0) < Cc * Hh * W:
        raise ValueError(f"downscale_metrics: x_last is a channel slice of a contiguous X, got strides {x_last.stride()}")
    if tuple(state.shape) != (Cc, 2) or count.numel() != 1 or not (out.is_contiguous() and Y.is_contiguous()):
        raise ValueError("downscale_metrics: state is float64 [C, 2], count int64 [1], out and Y contiguous")
    ws = workspace(lib().gcl_downscale_loss_ws_bytes(0, 0, 0, 0), out.device)
    _check(lib().gcl_downscale_metrics(_p(out), _p(x_last), x_last.stride(0), _p(Y), 1 if residual else 0, B, Cc, Hh, W,
                                       _pd(state), _pl(count), ws.data_ptr(), ws.numel(), _stream()))
    return state


def downscale_loss_scale(dout, g, out=None):
    """dout * g[0] with g a float32 scalar on the GPU (see gcl_downscale_loss_scale)."""
    assert dout.is_contiguous() and g.numel() == 1
    if out is None:
        out = torch.empty_like(dout)
    _check(lib().gcl_downscale_loss_scale(_p(dout), _p(g), dout.numel(), _p(out), _stream()))
    return out


EVAL_NS = 7  # sums per (sample, channel) of gcl_eval_colstats


def _bgc(t, who: str):
    if t.dim() != 3 or t.stride(2) != 1:
        raise ValueError(f"{who}: expected a [B, G, C] view with unit channel stride, got {tuple(t.shape)} / {t.stride()}")
    return t.stride(1), t.stride(0)


def eval_colstats(delta3, x_last3, y3, node_w, chan_kind, residual: bool, stats, out3=None):
    """The seven float64 sums per (sample, channel) behind the scores of one validation batch, into stats [B, C, 7]
    (see gcl_eval_colstats).  delta3 / x_last3 / y3 / out3: [B, G, C] views with unit channel stride (x_last3 the last
    slot of the window, y3 step 0 of the targets); node_w float32 [G] or None; chan_kind int32 [C] or None.  With out3
    the one-step prediction is stored as well, bit-equal to `ar_advance`'s."""
    B, G, Cc = delta3.shape
    if tuple(x_last3.shape) != (B, G, Cc) or tuple(y3.shape) != (B, G, Cc) or (out3 is not None and tuple(out3.shape) != (B, G, Cc)):
        raise ValueError(f"eval_colstats: delta {tuple(delta3.shape)}, x_last {tuple(x_last3.shape)}, y {tuple(y3.shape)}"
                         + (f", out {tuple(out3.shape)}" if out3 is not None else "") + " must be one [B, G, C]")
    if tuple(stats.shape) != (B, Cc, EVAL_NS):
        raise ValueError(f"eval_colstats: stats is float64 [{B}, {Cc}, {EVAL_NS}], got {tuple(stats.shape)}")
    if node_w is not None and (node_w.numel() != G or not node_w.is_contiguous()):
        raise ValueError(f"eval_colstats: node_w holds {node_w.numel()} weights for {G} nodes")
    if chan_kind is not None and chan_kind.numel() != Cc:
        raise ValueError(f"eval_colstats: chan_kind holds {chan_kind.numel()} entries for {Cc} channels")
    ldd, bsd = _bgc(delta3, "eval_colstats")
    ldx, bsx = _bgc(x_last3, "eval_colstats")
    ldy, bsy = _bgc(y3, "eval_colstats")
    ldo, bso = _bgc(out3, "eval_colstats") if out3 is not None else (0, 0)
    ws = workspace(lib().gcl_eval_colstats_ws_bytes(B, G, Cc), delta3.device)
    _check(lib().gcl_eval_colstats(_p(delta3), ldd, bsd, _p(x_last3), ldx, bsx, _p(y3), ldy, bsy, _p(node_w), _pi(chan_kind),
                                   1 if residual else 0, _p(out3), ldo, bso, _pd(stats), B, G, Cc, ws.data_ptr(),
                                   ws.numel(), _stream()))
    return stats


def eval_accumulate(stats, chan_w, chan_kind, inv_wsum: float, G: int, state):
    """state (float64 [4] on the GPU) += {loss, acc, raw_mse, 1} of the batch whose sums stats [B, C, 7] holds (see
    gcl_eval_accumulate)."""
    B, Cc, ns = stats.shape
    if ns != EVAL_NS or state.numel() != 4:
        raise ValueError(f"eval_accumulate: stats is [B, C, {EVAL_NS}] and state float64 [4], got {tuple(stats.shape)} and "
                         f"{tuple(state.shape)}")
    if chan_w is not None and (chan_w.numel() != Cc or not chan_w.is_contiguous()):
        raise ValueError(f"eval_accumulate: chan_w holds {chan_w.numel()} weights for {Cc} channels")
    _check(lib().gcl_eval_accumulate(_pd(stats), _p(chan_w), _pi(chan_kind), float(inv_wsum), B, int(G), Cc, _pd(state),
                                     _stream()))
    return state


def tensor_batch_pack(X4, Y4, idx, Wxu: int, Wyu: int, Fu: int, out=None):
    """Batches from the stored legacy tensors X4 [N, G, Wx, F] / Y4 [N, G, Wy, F] (float32, contiguous, on the GPU; Y4
    may be None): samples idx (int64 [B] on the GPU), the last Wxu / Wyu steps, the first Fu features -> (X [B, G,
    Wxu * Fu], Y [B, G, Wyu * Fu] or None), one launch (see gcl_tensor_batch_pack).  out = (X, Y): [B, G, .] views with
    unit channel stride to fill in place."""
    if X4.dim() != 4 or not X4.is_contiguous() or (Y4 is not None and (Y4.dim() != 4 or not Y4.is_contiguous()
                                                                       or Y4.shape[:2] != X4.shape[:2] or Y4.shape[3] != X4.shape[3])):
        raise ValueError("tensor_batch_pack: X4 and Y4 are contiguous [N, G, W, F] tensors over the same samples, nodes and "
                         "features")
    N, G, Wx, F = (int(v) for v in X4.shape)
    Wy = int(Y4.shape[2]) if Y4 is not None else 0
    B = idx.numel()
    X, Y = out if out is not None else (None, None)
    if X is None:
        X = torch.empty(B, G, Wxu * Fu, dtype=torch.float32, device=X4.device)
    if Y is None and Y4 is not None:
        Y = torch.empty(B, G, Wyu * Fu, dtype=torch.float32, device=X4.device)
    if tuple(X.shape) != (B, G, Wxu * Fu) or (Y4 is not None and tuple(Y.shape) != (B, G, Wyu * Fu)):
        raise ValueError(f"tensor_batch_pack: out buffers {tuple(X.shape)} / {tuple(Y.shape) if Y is not None else None} do "
                         f"not hold [{B}, {G}, {Wxu * Fu}] / [{B}, {G}, {Wyu * Fu}]")
    ldx, bsx = _bgc(X, "tensor_batch_pack")
    ldy, bsy = _bgc(Y, "tensor_batch_pack") if Y4 is not None else (0, 0)
    _check(lib().gcl_tensor_batch_pack(_p(X4), Wx, int(Wxu), _p(Y4), Wy, int(Wyu), N, G, F, int(Fu), _pl(idx), B, _p(X), ldx,
                                       bsx, _p(Y) if Y4 is not None else None, ldy, bsy, _stream()))
    return X, (Y if Y4 is not None else None)


# ------------------------------------------------------------------------------------------------------------------
# Training and scoring the regional heads (csrc/region_train.hip)
# ------------------------------------------------------------------------------------------------------------------
class RegionRecord:
    """Shape of one cache record (see gcl_region_cache_record_bytes): the used widths, the padded row widths and the
    float offsets of the four parts.  Pure arithmetic (`nbytes` asks the library, which refuses unsupported shapes)."""

    def __init__(self, n_roi: int, half_E: int, XF: int, D: int, Dm: int, C: int, P: int = 1):
        self.n_roi, self.half_E, self.XF, self.D, self.Dm, self.C, self.P = (int(v) for v in (n_roi, half_E, XF, D, Dm, C, P))
        up4 = lambda v: (v + 3) // 4 * 4
        self.Sp, self.Dgp, self.Cp, self.Yp = up4(self.XF + self.D), up4(self.Dm), up4(self.C), up4(self.P * self.C)
        self.sizes = (self.n_roi * self.Sp, self.half_E * self.Dgp, self.n_roi * self.Cp, self.n_roi * self.Yp)
        self.offsets = (0, self.sizes[0], self.sizes[0] + self.sizes[1], self.sizes[0] + self.sizes[1] + self.sizes[2])
        self.floats = sum(self.sizes)

    @property
    def dims(self):
        return self.n_roi, self.half_E, self.XF, self.D, self.Dm, self.C, self.P

    @property
    def nbytes(self) -> int:
        nb = lib().gcl_region_cache_record_bytes(*self.dims)
        if nb != 4 * self.floats:
            raise ValueError(f"region cache record {self.dims}: the library reports {nb} bytes, the layout {4 * self.floats}")
        return nb

    def parts(self, B: int, device):
        """Fresh contiguous (roi3 [B, n_roi, Sp], send [B, half_E, Dgp], pred [B, n_roi, Cp], y [B, n_roi, Yp])."""
        e = lambda r, w: torch.empty(B, r, w, dtype=torch.float32, device=device)
        return e(self.n_roi, self.Sp), e(self.half_E, self.Dgp), e(self.n_roi, self.Cp), e(self.n_roi, self.Yp)


def _cache_of(rec: RegionRecord, cache, who: str) -> int:
    if cache.dim() != 2 or cache.shape[1] != rec.floats or not cache.is_contiguous() or cache.shape[0] == 0:
        raise ValueError(f"{who}: the cache is a contiguous float32 [n_slots, {rec.floats}] tensor, got {tuple(cache.shape)}")
    return cache.shape[0]


def region_cache_store(rec: RegionRecord, cache, slots, pred3, lat3, mesh3, X3, y3, rows, snd):
    """Records slots[b] (device int64 [B], distinct) of cache [n_slots, rec.floats] from one batch of global outputs (see
    gcl_region_cache_store).  pred3 [B,G,C], lat3 [B,G,D], mesh3 [B,M,Dm], X3 [B,G,XF], y3 [B,G,P*C]: unit channel stride,
    any row / batch stride.  rows int32 [n_roi], snd int32 [half_E]."""
    n_slots = _cache_of(rec, cache, "region_cache_store")
    B, G = X3.shape[0], X3.shape[1]
    M = mesh3.shape[1]
    want = {"pred": (pred3, (B, G, rec.C)), "lat": (lat3, (B, G, rec.D)), "mesh": (mesh3, (B, M, rec.Dm)),
            "X": (X3, (B, G, rec.XF)), "y": (y3, (B, G, rec.P * rec.C))}
    args = []
    for name, (t, shape) in want.items():
        if tuple(t.shape) != shape or t.stride(2) != 1:
            raise ValueError(f"region_cache_store: {name} is a {shape} view with unit channel stride, got {tuple(t.shape)} / "
                             f"{t.stride()}")
        args += [_p(t), t.stride(1), t.stride(0)]
    if rows.numel() != rec.n_roi or snd.numel() != rec.half_E or slots.numel() != B:
        raise ValueError(f"region_cache_store: {rows.numel()} rows / {snd.numel()} senders / {slots.numel()} slots for a "
                         f"record of {rec.n_roi} / {rec.half_E} and a batch of {B}")
    _check(lib().gcl_region_cache_store(*args, _pi(rows), _pi(snd), _pl(slots), _p(cache), n_slots, B, G, M, *rec.dims,
                                        _stream()))
    return cache


def region_cache_fetch(rec: RegionRecord, cache, slots, out=None):
    """(roi3, send, pred, y) of the records slots (device int64 [B]; repeats allowed, a slot outside the cache gives zero
    rows), one launch (see gcl_region_cache_fetch).  out: the four destination buffers (`rec.parts`), any of them None."""
    n_slots = _cache_of(rec, cache, "region_cache_fetch")
    B = slots.numel()
    if out is None:
        out = rec.parts(B, cache.device)
    rows = (rec.n_roi, rec.half_E, rec.n_roi, rec.n_roi)
    widths = (rec.Sp, rec.Dgp, rec.Cp, rec.Yp)
    args = []
    for t, r, w in zip(out, rows, widths):
        if t is None:
            args += [None, 0]
            continue
        if tuple(t.shape) != (B, r, w) or t.stride(2) != 1 or (r > 1 and t.stride(1) != w):
            raise ValueError(f"region_cache_fetch: a destination is a [{B}, {r}, {w}] buffer with dense rows, got "
                             f"{tuple(t.shape)} / {t.stride()}")
        args += [_p(t), t.stride(0)]
    _check(lib().gcl_region_cache_fetch(_p(cache), n_slots, _pl(slots), B, *rec.dims, *args, _stream()))
    return tuple(out)


def region_eval_pair(preds, y_step3, chan_kind, residual: bool, rows, weight: float, acc, obs: int, n=None):
    """One lock-step AR step of one or two predictions and their ROI losses (see gcl_region_eval_pair).  preds: a list of
    one or two (delta3 [B,G,C], win3 [B,G,obs*C], new_win4 [B,G,obs,C] contiguous | None, out3 [B,G,C] | None); y_step3
    [B,G,C]; views with unit channel stride.  rows: int32 device rows the loss runs over (None: the first `n` rows, all G
    by default).  acc: device float64 [len(preds)], acc[q] += weight * mean((step_out_q - y)^2 over the rows)."""
    nq = len(preds)
    B, G, Cc = preds[0][0].shape
    n = rows.numel() if rows is not None else (G if n is None else int(n))
    if nq not in (1, 2) or acc.numel() != nq:
        raise ValueError(f"region_eval_pair: one or two predictions and a float64 [{nq}] accumulator, got {nq} and "
                         f"{tuple(acc.shape)}")
    if tuple(y_step3.shape) != (B, G, Cc):
        raise ValueError(f"region_eval_pair: y_step {tuple(y_step3.shape)} is not [{B}, {G}, {Cc}]")
    ldy, bsy = _bgc(y_step3, "region_eval_pair")
    args = []
    for delta3, win3, new4, out3 in preds:
        if tuple(delta3.shape) != (B, G, Cc) or tuple(win3.shape[:2]) != (B, G) or win3.shape[2] < obs * Cc:
            raise ValueError(f"region_eval_pair: delta {tuple(delta3.shape)} / window {tuple(win3.shape)} do not hold "
                             f"[{B}, {G}, {Cc}] / [{B}, {G}, {obs * Cc}]")
        if new4 is not None and (tuple(new4.shape) != (B, G, obs, Cc) or not new4.is_contiguous()):
            raise ValueError(f"region_eval_pair: the new window is a contiguous [{B}, {G}, {obs}, {Cc}] tensor")
        if out3 is not None and tuple(out3.shape) != (B, G, Cc):
            raise ValueError(f"region_eval_pair: out {tuple(out3.shape)} is not [{B}, {G}, {Cc}]")
        ldd, bsd = _bgc(delta3, "region_eval_pair")
        ldw, bsw = _bgc(win3, "region_eval_pair")
        ldo, bso = _bgc(out3, "region_eval_pair") if out3 is not None else (0, 0)
        args += [_p(delta3), ldd, bsd, _p(win3), ldw, bsw, _p(new4), _p(out3), ldo, bso]
    if nq == 1:
        args += [None, 0, 0, None, 0, 0, None, None, 0, 0]
    if chan_kind is not None and chan_kind.numel() != Cc:
        raise ValueError(f"region_eval_pair: chan_kind holds {chan_kind.numel()} entries for {Cc} channels")
    ws = workspace(lib().gcl_region_eval_pair_ws_bytes(nq, B, n, Cc), y_step3.device)
    _check(lib().gcl_region_eval_pair(nq, *args, _p(y_step3), ldy, bsy, _pi(chan_kind), 1 if residual else 0, _pi(rows), n,
                                      float(weight), _pd(acc), B, G, int(obs), Cc, ws.data_ptr(), ws.numel(), _stream()))
    return acc


# ------------------------------------------------------------------------------------------------------------------
# Station observations and regional scoring of a saved forecast (csrc/predict.hip)
# ------------------------------------------------------------------------------------------------------------------
def _pu8(t, n: int, who: str):
    if not (t.is_cuda and t.dtype == torch.uint8 and t.is_contiguous() and t.numel() == n):
        raise ValueError(f"{who}: expected a contiguous uint8 device tensor of {n} entries")
    return t.data_ptr()


def obs_pack(y3, keep_row, keep_chan, out3=None):
    """out3[b, g, k] = y3[b, g, k] where keep_row[g] and keep_chan[k % C] (uint8 device masks [G] / [C]), NaN elsewhere;
    one launch (see gcl_obs_pack).  y3 / out3: [B, G, K] views with unit channel stride; out3 may be y3."""
    B, G, K = y3.shape
    if out3 is None:
        out3 = torch.empty(B, G, K, dtype=torch.float32, device=y3.device)
    if tuple(out3.shape) != (B, G, K):
        raise ValueError(f"obs_pack: out {tuple(out3.shape)} is not [{B}, {G}, {K}]")
    Cc = keep_chan.numel()
    if Cc == 0 or K % Cc:
        raise ValueError(f"obs_pack: {K} columns are not whole steps of {Cc} channels")
    ldy, bsy = _bgc(y3, "obs_pack")
    ldo, bso = _bgc(out3, "obs_pack")
    if B * G == 0:
        return out3
    _check(lib().gcl_obs_pack(_p(y3), ldy, bsy, _pu8(keep_row, G, "obs_pack"), _pu8(keep_chan, Cc, "obs_pack"), B, G, K, Cc,
                              _p(out3), ldo, bso, _stream()))
    return out3


REGION_NS = 11  # per (horizon, channel): se, ae, base se, count, St, Stt, Sv, Svv, Stv, pivot t, pivot v


def region_interp_scores(pred3, nlat: int, cell, w, series, t0, first: int, mean, std, P: int, Cc: int, sums, vout=None,
                         tout=None):
    """The float64 sums [P, C, REGION_NS] behind the regional scores of a saved global forecast (see
    gcl_region_interp_scores).  pred3 [N, Gg, >= P * C] float32 with unit column stride; cell int32 [nr, 2] / w float64
    [nr, 4]; series fp16 [n_time, nr, n_feat] contiguous; t0 int32 [N] on the device (-1: skip); first: the first sample
    that is not skipped; mean / std float64 [C].  vout / tout: contiguous float32 [N, P, nr, C] or None."""
    N, Gg = pred3.shape[0], pred3.shape[1]
    nr = cell.shape[0]
    if pred3.dim() != 3 or pred3.stride(2) != 1 or pred3.shape[2] < P * Cc:
        raise ValueError(f"region_interp_scores: the forecast is a [N, G, >= {P * Cc}] view with unit column stride")
    if series.dim() != 3 or series.shape[1] != nr or series.shape[2] < Cc or tuple(w.shape) != (nr, 4):
        raise ValueError(f"region_interp_scores: series {tuple(series.shape)} / weights {tuple(w.shape)} for {nr} nodes")
    if t0.numel() != N or mean.numel() != Cc or std.numel() != Cc or tuple(sums.shape) != (P, Cc, REGION_NS):
        raise ValueError("region_interp_scores: t0 [N], mean / std [C] and sums [P, C, 11] expected")
    for t in (vout, tout):
        if t is not None and (tuple(t.shape) != (N, P, nr, Cc) or not t.is_contiguous()):
            raise ValueError(f"region_interp_scores: a stored field is a contiguous [{N}, {P}, {nr}, {Cc}] tensor")
    ws = workspace(int(lib().gcl_region_interp_scores_ws_bytes(N, P, nr, Cc)), pred3.device)
    _check(lib().gcl_region_interp_scores(_p(pred3), pred3.stride(1), pred3.stride(0), Gg, int(nlat), _pi(cell), _pd(w),
                                          _ph(series), series.shape[2], series.shape[0], _pi(t0), int(first), _pd(mean),
                                          _pd(std), N, int(P), nr, int(Cc), _pd(sums), _p(vout), _p(tout), ws.data_ptr(),
                                          ws.numel(), _stream()))
    return sums


# ======================================================================================================================
# WeatherUNet inference and the cascade scores (csrc/unet.hip)
# ======================================================================================================================
UNET_PLANAR, UNET_ROWS, UNET_POOL, UNET_UPCAT = 0, 1, 2, 3


class UnetSrc(C.Structure):
    """gcl_unet_src_t: how a 3x3 convolution reads its input (see include/gcl.h)."""
    _fields_ = [("a", _vp), ("b", _vp), ("kind", _i32), ("C1", _i32), ("C2", _i32), ("Hs", _i32), ("Ws", _i32)]


def unet_src(kind: int, a, b=None):
    """The source descriptor of `a` (and, for UNET_UPCAT, the low tensor `b`): contiguous float32 device tensors, planar
    [B, C, H, W] for UNET_PLANAR and channels-last [B, H, W, C] otherwise."""
    for t in (a, b):
        if t is not None and not t.is_contiguous():
            raise ValueError("unet_src: contiguous tensors expected")
    s = UnetSrc(_p(a), _p(b), int(kind), 0, 0, 0, 0)
    if kind == UNET_POOL:
        s.Hs, s.Ws = a.shape[1], a.shape[2]
    elif kind == UNET_UPCAT:
        s.C1, s.C2, s.Hs, s.Ws = a.shape[3], b.shape[3], b.shape[1], b.shape[2]
    return s


def unet_launches() -> int:
    """Kernels launched by the entry points of csrc/unet.hip in this process."""
    return int(lib().gcl_unet_launches())


def _out(out, shape, like, who, name="out", exact=False):
    """`out`, or when None a new float32 tensor of `shape` on like's device.  A given one is contiguous and holds shape's
    elements (exact: has that shape)."""
    if out is None:
        return torch.empty(*shape, dtype=torch.float32, device=like.device)
    if not out.is_contiguous() or (tuple(out.shape) != tuple(shape) if exact else out.numel() != torch.Size(shape).numel()):
        raise ValueError(f"{who}: {name} is a contiguous {list(shape)} tensor, got {tuple(out.shape)}")
    return out


def _pack3x3(w, out, dgrad: bool):
    who = "unet_pack_weights_dgrad" if dgrad else "unet_pack_weights"
    if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3) or not w.is_contiguous():
        raise ValueError(f"{who}: a contiguous [Cout, Cin, 3, 3] weight expected, got {tuple(w.shape)}")
    Cout, Cin = w.shape[0], w.shape[1]
    # the data gradient is the transposed convolution: Cin' = Cout, Cout' = Cin
    n = int(lib().gcl_unet_packed_floats(Cout, Cin) if dgrad else lib().gcl_unet_packed_floats(Cin, Cout))
    out = _out(out, (n,), w, who)
    _check(getattr(lib(), "gcl_" + who)(_p(w), Cin, Cout, _p(out), _stream()))
    return out


def unet_pack_weights(w, out=None):
    """torch's [Cout, Cin, 3, 3] convolution weight in the order gcl_unet_conv3x3 streams."""
    return _pack3x3(w, out, False)


def unet_conv3x3(src: UnetSrc, packed, norm, eps: float, y, Cin: int):
    """y [B, H, W, Cout] = the 3x3 convolution of the source with BatchNorm (norm = (gamma, beta, mean, var)) and GELU
    behind it; norm None: the bare convolution (see gcl_unet_conv3x3)."""
    if y.dim() != 4 or not y.is_contiguous():
        raise ValueError("unet_conv3x3: y is a contiguous [B, H, W, Cout] tensor")
    B, H, W, Cout = y.shape
    g, bt, m, v = norm if norm is not None else (None, None, None, None)
    _check(lib().gcl_unet_conv3x3(C.byref(src), _p(packed), _p(g), _p(bt), _p(m), _p(v), float(eps), _p(y), B, H, W,
                                  int(Cin), Cout, _stream()))
    return y


def unet_conv1x1_out(x, w, bias, y, residual=None, res_bs: int = 0):
    """y [B, Cout, H, W] (planar) = x [B, H, W, F] times w [Cout, F] plus bias, plus channel co of the planar `residual`
    view (sample stride res_bs floats) when given (see gcl_unet_conv1x1_out)."""
    B, H, W, F = x.shape
    Cout = w.shape[0]
    if tuple(y.shape) != (B, Cout, H, W) or not (x.is_contiguous() and y.is_contiguous() and w.is_contiguous()):
        raise ValueError(f"unet_conv1x1_out: contiguous x [B, H, W, F], w [Cout, F] and y [{B}, {Cout}, {H}, {W}] expected")
    _check(lib().gcl_unet_conv1x1_out(_p(x), _p(w), _p(bias), _p(residual), int(res_bs), _p(y), B, H, W, F, Cout,
                                      _stream()))
    return y


def cascade_pack(coarse, gnn_mean, gnn_std, ds_mean, ds_std, static_fine, obs: int, coarse_phys=None, X=None):
    """(coarse_phys [B, H, W, C], X [B, obs * C + Ns, H, W]) of coarse [B, H, W, C] (see gcl_cascade_pack).  The four
    vectors: float32 [C]; static_fine: float32 [W, H, Ns] or None."""
    B, H, W, Cc = coarse.shape
    Ns = 0 if static_fine is None else static_fine.shape[2]
    if static_fine is not None and (tuple(static_fine.shape[:2]) != (W, H) or not static_fine.is_contiguous()):
        raise ValueError(f"cascade_pack: static_fine is a contiguous [{W}, {H}, Ns] tensor")
    if not coarse.is_contiguous() or any(v.numel() != Cc for v in (gnn_mean, gnn_std, ds_mean, ds_std)):
        raise ValueError("cascade_pack: a contiguous coarse [B, H, W, C] and four vectors of C values expected")
    if coarse_phys is None:
        coarse_phys = torch.empty_like(coarse)
    if X is None:
        X = torch.empty(B, obs * Cc + Ns, H, W, dtype=torch.float32, device=coarse.device)
    if tuple(X.shape) != (B, obs * Cc + Ns, H, W) or not X.is_contiguous() or not coarse_phys.is_contiguous():
        raise ValueError(f"cascade_pack: X is a contiguous [{B}, {obs * Cc + Ns}, {H}, {W}] tensor")
    _check(lib().gcl_cascade_pack(_p(coarse), _p(gnn_mean), _p(gnn_std), _p(ds_mean), _p(ds_std), _p(static_fine),
                                  _p(coarse_phys), _p(X), B, H, W, Cc, int(obs), Ns, _stream()))
    return coarse_phys, X


def cascade_scores(out, coarse_phys, fine, t_fine, t_persist, ds_mean, ds_std, state, count, step: int, ws=None):
    """state [AR, C, 3] float64 / count [AR] int64 += the scores of one step (see gcl_cascade_scores).  out [B, C, H, W];
    coarse_phys [B, H, W, C]; fine fp16 [T, W, H, n_feat]; t_fine / t_persist int64 [B] on the device."""
    B, Cc, H, W = out.shape
    if tuple(coarse_phys.shape) != (B, H, W, Cc) or fine.dim() != 4 or tuple(fine.shape[1:3]) != (W, H):
        raise ValueError(f"cascade_scores: coarse_phys [{B}, {H}, {W}, {Cc}] and fine [T, {W}, {H}, >= {Cc}] expected")
    if not (out.is_contiguous() and coarse_phys.is_contiguous()) or t_fine.numel() != B or t_persist.numel() != B:
        raise ValueError("cascade_scores: contiguous fields and t_fine / t_persist of B values expected")
    if state.dim() != 3 or tuple(state.shape[1:]) != (Cc, 3) or count.numel() != state.shape[0]:
        raise ValueError(f"cascade_scores: state [AR, {Cc}, 3] and count [AR] expected")
    need = int(lib().gcl_cascade_scores_ws_bytes(B, H, W, Cc))
    if ws is None:
        ws = workspace(need, out.device)
    _check(lib().gcl_cascade_scores(_p(out), _p(coarse_phys), _ph(fine), fine.shape[0], fine.shape[3], _pl(t_fine),
                                    _pl(t_persist), _p(ds_mean), _p(ds_std), _pd(state), _pl(count), int(step),
                                    state.shape[0], B, H, W, Cc, ws.data_ptr(), ws.numel() * ws.element_size(), _stream()))
    return state


# ======================================================================================================================
# WeatherUNet training (csrc/unet_train.hip)
# ======================================================================================================================
def unet_train_launches() -> int:
    """Kernels launched by the entry points of csrc/unet_train.hip in this process."""
    return int(lib().gcl_unet_train_launches())


def _ws_for(need: int, ws, device):
    """(pointer, bytes) of the caller's scratch tensor, or of the shared workspace when None."""
    if ws is None:
        ws = workspace(need, device)
    return ws.data_ptr(), ws.numel() * ws.element_size()


def _rows(t, who, name="the input", dims=None):
    """(rows, C) of the contiguous [..., C] tensor t, which has `dims` dimensions when given."""
    if t.dim() < 2 or (dims is not None and t.dim() != dims) or not t.is_contiguous():
        raise ValueError(f"{who}: {name} is a contiguous {'[B, H, W, C]' if dims == 4 else '[..., C]'} tensor, got "
                         f"{tuple(t.shape)}")
    return t.numel() // t.shape[-1], t.shape[-1]


def unet_bn_stats(z, eps: float, momentum: float, mean, invstd, running_mean=None, running_var=None,
                  num_batches=None, ws=None):
    """(mean, invstd) float32 [C] of the rows of z [..., C]; the running buffers and the int64 counter are updated in
    place when given (see gcl_unet_bn_stats)."""
    n, Cc = _rows(z, "unet_bn_stats")
    if any(t is not None and (t.numel() != Cc or not t.is_contiguous()) for t in (mean, invstd, running_mean, running_var)):
        raise ValueError(f"unet_bn_stats: vectors of {Cc} values expected")
    if n < 2:
        raise ValueError(f"unet_bn_stats: expected more than 1 value per channel when training, got {n}")
    if num_batches is not None and (num_batches.dtype != torch.int64 or num_batches.numel() != 1 or not num_batches.is_cuda):
        raise ValueError("unet_bn_stats: num_batches is one int64 on the device")
    wp, wb = _ws_for(int(lib().gcl_unet_colsum_ws_bytes(n, 2 * Cc)), ws, z.device)
    _check(lib().gcl_unet_bn_stats(_p(z), n, Cc, float(eps), float(momentum), _p(mean), _p(invstd), _p(running_mean),
                                   _p(running_var), None if num_batches is None else num_batches.data_ptr(), wp, wb,
                                   _stream()))
    return mean, invstd


def unet_bn_gelu(z, gamma, beta, mean, invstd, out):
    """out = gelu(gamma * (z - mean) * invstd + beta) over the rows of z [..., C] (see gcl_unet_bn_gelu)."""
    n, Cc = _rows(z, "unet_bn_gelu")
    if out.shape != z.shape or not out.is_contiguous():
        raise ValueError("unet_bn_gelu: out has z's shape")
    _check(lib().gcl_unet_bn_gelu(_p(z), _p(gamma), _p(beta), _p(mean), _p(invstd), _p(out), n, Cc, _stream()))
    return out


def unet_bn_gelu_bwd(z, dA, gamma, beta, mean, invstd, dZ, dgamma, dbeta, ws=None):
    """(dZ, dgamma, dbeta) of gelu(batch_norm(z)) given dA; dZ may be dA (see gcl_unet_bn_gelu_bwd)."""
    n, Cc = _rows(z, "unet_bn_gelu_bwd")
    if dA.shape != z.shape or dZ.shape != z.shape or not (dA.is_contiguous() and dZ.is_contiguous()):
        raise ValueError("unet_bn_gelu_bwd: dA and dZ have z's shape")
    if dgamma.numel() != Cc or dbeta.numel() != Cc:
        raise ValueError(f"unet_bn_gelu_bwd: dgamma and dbeta of {Cc} values expected")
    wp, wb = _ws_for(int(lib().gcl_unet_colsum_ws_bytes(n, 2 * Cc)), ws, z.device)
    _check(lib().gcl_unet_bn_gelu_bwd(_p(z), _p(dA), _p(gamma), _p(beta), _p(mean), _p(invstd), _p(dZ), _p(dgamma),
                                      _p(dbeta), n, Cc, wp, wb, _stream()))
    return dZ, dgamma, dbeta


def unet_wgrad_chunks(B: int, H: int, W: int, Cin: int, Cout: int) -> int:
    """The pixel chunks gcl_unet_conv3x3_wgrad splits this shape into."""
    return int(lib().gcl_unet_wgrad_chunks(B, H, W, Cin, Cout))


def unet_wgrad_ws_bytes(B: int, H: int, W: int, Cin: int, Cout: int) -> int:
    return int(lib().gcl_unet_wgrad_ws_bytes(B, H, W, Cin, Cout))


def unet_conv3x3_wgrad(src: UnetSrc, dZ, Cin: int, dW=None, ws=None):
    """dW [Cout, Cin, 3, 3] of the 3x3 convolution that read `src`, from dZ [B, H, W, Cout] (see
    gcl_unet_conv3x3_wgrad)."""
    if dZ.dim() != 4 or not dZ.is_contiguous():
        raise ValueError("unet_conv3x3_wgrad: dZ is a contiguous [B, H, W, Cout] tensor")
    B, H, W, Cout = dZ.shape
    dW = _out(dW, (Cout, int(Cin), 3, 3), dZ, "unet_conv3x3_wgrad", "dW", exact=True)
    wp, wb = _ws_for(unet_wgrad_ws_bytes(B, H, W, int(Cin), Cout), ws, dZ.device)
    _check(lib().gcl_unet_conv3x3_wgrad(C.byref(src), _p(dZ), _p(dW), B, H, W, int(Cin), Cout, wp, wb, _stream()))
    return dW


def unet_pack_weights_dgrad(w, out=None):
    """torch's [Cout, Cin, 3, 3] weight transposed and tap-flipped, in the order gcl_unet_conv3x3 streams: the data
    gradient is unet_conv3x3(unet_src(UNET_ROWS, dZ), packed, None, eps, dX [B, H, W, Cin], Cout)."""
    return _pack3x3(w, out, True)


def unet_pool_bwd(act, dpooled, dA, skip=None):
    """dA [B, Hs, Ws, C] = skip + the max-pool backward of dpooled [B, Hs // 2, Ws // 2, C] through the argmax of act;
    skip: a [B, Hs, Ws, C] view of wider contiguous rows (a channel slice from 0), or None (see gcl_unet_pool_bwd)."""
    B, Hs, Ws, Cc = act.shape
    if tuple(dpooled.shape) != (B, Hs // 2, Ws // 2, Cc) or tuple(dA.shape) != (B, Hs, Ws, Cc) or not (
            act.is_contiguous() and dpooled.is_contiguous() and dA.is_contiguous()):
        raise ValueError(f"unet_pool_bwd: contiguous act / dA [{B}, {Hs}, {Ws}, {Cc}] and dpooled at half the size expected")
    ld = 0
    if skip is not None:
        ld = skip.stride(2)
        if tuple(skip.shape) != (B, Hs, Ws, Cc) or skip.stride(3) != 1 or skip.stride(1) != Ws * ld or skip.stride(0) != Hs * Ws * ld:
            raise ValueError("unet_pool_bwd: skip is a leading channel slice of contiguous [B, Hs, Ws, ld] rows")
    _check(lib().gcl_unet_pool_bwd(_p(act), _p(dpooled), _p(skip), int(ld), _p(dA), B, Hs, Ws, Cc, _stream()))
    return dA


def unet_upsample_bwd(d, c_off: int, dlow):
    """dlow [B, Hs, Ws, C2] = the adjoint of upsample-and-pad applied to channels c_off .. c_off + C2 of the contiguous
    d [B, H, W, ld] (see gcl_unet_upsample_bwd)."""
    B, H, W, ld = d.shape
    if dlow.dim() != 4 or dlow.shape[0] != B or not (d.is_contiguous() and dlow.is_contiguous()):
        raise ValueError("unet_upsample_bwd: contiguous d [B, H, W, ld] and dlow [B, Hs, Ws, C2] expected")
    _check(lib().gcl_unet_upsample_bwd(_p(d), ld, int(c_off), _p(dlow), B, H, W, dlow.shape[1], dlow.shape[2],
                                       dlow.shape[3], _stream()))
    return dlow


def unet_conv1x1_out_bwd(dY, a, w, dA, dW=None, db=None, ws=None):
    """(dA [B, H, W, F], dW [Cout, F], db [Cout]) of unet_conv1x1_out from the planar dY [B, Cout, H, W] (see
    gcl_unet_conv1x1_out_bwd)."""
    B, H, W, F = a.shape
    Cout = w.shape[0]
    if tuple(dY.shape) != (B, Cout, H, W) or tuple(dA.shape) != (B, H, W, F) or tuple(w.shape) != (Cout, F) or not (
            dY.is_contiguous() and a.is_contiguous() and w.is_contiguous() and dA.is_contiguous()):
        raise ValueError(f"unet_conv1x1_out_bwd: contiguous dY [{B}, {Cout}, {H}, {W}], a / dA [B, H, W, F], w [Cout, F] expected")
    dW = _out(dW, (Cout, F), a, "unet_conv1x1_out_bwd", "dW")
    db = _out(db, (Cout,), a, "unet_conv1x1_out_bwd", "db")
    wp, wb = _ws_for(int(lib().gcl_unet_conv1x1_out_bwd_ws_bytes(B, H, W, F, Cout)), ws, a.device)
    _check(lib().gcl_unet_conv1x1_out_bwd(_p(dY), _p(a), _p(w), _p(dA), _p(dW), _p(db), B, H, W, F, Cout, wp, wb, _stream()))
    return dA, dW, db


# ======================================================================================================================
# WeatherUNetV2 inference (csrc/unet_v2.hip)
# ======================================================================================================================
def unet_v2_launches() -> int:
    """Kernels launched by the entry points of csrc/unet_v2.hip in this process."""
    return int(lib().gcl_unet_v2_launches())


def _v2_slice(out, shape, who):
    """ldo of `out`: a [B, H, W, C] channel slice of contiguous [B, H, W, ld] rows."""
    B, H, W, Cc = shape
    ld = out.stride(2)
    if tuple(out.shape) != tuple(shape) or ld < Cc or out.stride() != (H * W * ld, W * ld, ld, 1):
        raise ValueError(f"{who}: out is a [{B}, {H}, {W}, {Cc}] channel slice of contiguous rows, got shape "
                         f"{tuple(out.shape)} strides {out.stride()}")
    return ld


def unet_v2_gn_stats(z, G: int, eps: float, mean=None, invstd=None):
    """(mean, invstd) float32 [B, G] of the GroupNorm of z [B, H, W, C] (see gcl_unet_v2_gn_stats)."""
    n, Cc = _rows(z, "unet_v2_gn_stats", "z", 4)
    B, HW = z.shape[0], n // z.shape[0]
    if G < 1 or Cc % G:
        raise ValueError(f"unet_v2_gn_stats: G = {G} must divide C = {Cc}")
    mean = _out(mean, (B, G), z, "unet_v2_gn_stats", "mean", exact=True)
    invstd = _out(invstd, (B, G), z, "unet_v2_gn_stats", "invstd", exact=True)
    _check(lib().gcl_unet_v2_gn_stats(_p(z), B, HW, Cc, int(G), float(eps), _p(mean), _p(invstd), _stream()))
    return mean, invstd


def unet_v2_gn_gelu(z, gamma, beta, mean, invstd, out=None):
    """out = gelu(GroupNorm(z)) from the statistics [B, G] (see gcl_unet_v2_gn_gelu)."""
    n, Cc = _rows(z, "unet_v2_gn_gelu", "z", 4)
    B, HW = z.shape[0], n // z.shape[0]
    if out is None:
        out = torch.empty_like(z)
    G = mean.shape[-1]
    if (tuple(out.shape) != tuple(z.shape) or not out.is_contiguous() or out.data_ptr() == z.data_ptr()
            or tuple(mean.shape) != (B, G) or tuple(invstd.shape) != (B, G) or Cc % G or gamma.numel() != Cc
            or beta.numel() != Cc or not all(t.is_contiguous() for t in (mean, invstd, gamma, beta))):
        raise ValueError(f"unet_v2_gn_gelu: out of z's shape (not z itself), statistics [{B}, G] and affine vectors of "
                         f"{Cc} values expected")
    _check(lib().gcl_unet_v2_gn_gelu(_p(z), _p(gamma), _p(beta), _p(mean), _p(invstd), _p(out), B, HW, Cc, G, _stream()))
    return out


def unet_v2_conv1x1(src: UnetSrc, w, out, Cin: int, bias=None, res=None):
    """out [B, H, W, Cout] (a channel slice of contiguous rows is allowed) = the 1x1 convolution of the source with
    w [Cout, Cin], + bias, + res [B, H, W, Cout]; w None: the identity (see gcl_unet_v2_conv1x1)."""
    if out.dim() != 4:
        raise ValueError("unet_v2_conv1x1: out is a [B, H, W, Cout] tensor")
    B, H, W, Cout = out.shape
    ld = _v2_slice(out, out.shape, "unet_v2_conv1x1")
    if w is not None and (tuple(w.shape) != (Cout, int(Cin)) or not w.is_contiguous()):
        raise ValueError(f"unet_v2_conv1x1: w is a contiguous [{Cout}, {Cin}] tensor, got {tuple(w.shape)}")
    if bias is not None and (bias.numel() != Cout or not bias.is_contiguous()):
        raise ValueError(f"unet_v2_conv1x1: bias holds {Cout} values")
    if res is not None and (tuple(res.shape) != (B, H, W, Cout) or not res.is_contiguous()):
        raise ValueError(f"unet_v2_conv1x1: res is a contiguous [{B}, {H}, {W}, {Cout}] tensor")
    _check(lib().gcl_unet_v2_conv1x1(C.byref(src), _p(w), _p(bias), _p(res), _p(out), ld, B, H, W, int(Cin), Cout,
                                     _stream()))
    return out


def unet_v2_tail_ws_bytes(B: int, HW: int, Cc: int) -> int:
    return int(lib().gcl_unet_v2_tail_ws_bytes(B, HW, Cc))


def unet_v2_block_tail(z, gamma, beta, mean, invstd, skip, w1, b1, w2, b2, out=None, ws=None):
    """out = u * sigmoid(w2 gelu(w1 mean_hw(u) + b1) + b2), u = gelu(GroupNorm(z)) + skip (see gcl_unet_v2_block_tail).
    ws: a float64 tensor of unet_v2_tail_ws_bytes(B, H * W, C) bytes, or None for the shared workspace."""
    n, Cc = _rows(z, "unet_v2_block_tail", "z", 4)
    B, HW = z.shape[0], n // z.shape[0]
    if out is None:
        out = torch.empty_like(z)
    G, hid = mean.shape[-1], w1.shape[0]
    if (tuple(skip.shape) != tuple(z.shape) or tuple(out.shape) != tuple(z.shape) or not (skip.is_contiguous() and out.is_contiguous())
            or tuple(mean.shape) != (B, G) or tuple(invstd.shape) != (B, G) or Cc % G or gamma.numel() != Cc or beta.numel() != Cc
            or tuple(w1.shape) != (hid, Cc) or tuple(w2.shape) != (Cc, hid) or b1.numel() != hid or b2.numel() != Cc
            or not all(t.is_contiguous() for t in (mean, invstd, gamma, beta, w1, b1, w2, b2))):
        raise ValueError(f"unet_v2_block_tail: skip / out of z's shape {tuple(z.shape)}, statistics [{B}, G], affine vectors of "
                         f"{Cc}, w1 [hidden, {Cc}], b1 [hidden], w2 [{Cc}, hidden], b2 [{Cc}] expected")
    wp, wb = _ws_for(unet_v2_tail_ws_bytes(B, HW, Cc), ws, z.device)
    _check(lib().gcl_unet_v2_block_tail(_p(z), _p(gamma), _p(beta), _p(mean), _p(invstd), _p(skip), _p(w1), _p(b1), _p(w2),
                                        _p(b2), _p(out), B, HW, Cc, G, hid, wp, wb, _stream()))
    return out


def unet_v2_layernorm(x, gamma, beta, eps: float, out=None):
    """nn.LayerNorm over the last dimension of the contiguous x [..., C] (see gcl_unet_v2_layernorm)."""
    n, Cc = _rows(x, "unet_v2_layernorm")
    out = _out(out, x.shape, x, "unet_v2_layernorm", exact=True)
    if gamma.numel() != Cc or beta.numel() != Cc or not (gamma.is_contiguous() and beta.is_contiguous()):
        raise ValueError(f"unet_v2_layernorm: affine vectors of {Cc} values expected")
    _check(lib().gcl_unet_v2_layernorm(_p(x), _p(gamma), _p(beta), float(eps), _p(out), n, Cc, _stream()))
    return out


def unet_v2_attention(qkv, heads: int, out=None):
    """qkv [B, N, 3 * C] (split as [3, heads, C / heads]) -> out [B, N, C] (see gcl_unet_v2_attention)."""
    if qkv.dim() != 3 or not qkv.is_contiguous() or heads < 1 or qkv.shape[2] % (3 * heads):
        raise ValueError(f"unet_v2_attention: a contiguous qkv [B, N, 3 * heads * head_dim] expected, got {tuple(qkv.shape)}")
    B, N, C3 = qkv.shape
    if N > 4096:
        raise ValueError(f"unet_v2_attention: at most 4096 tokens, got {N}")
    Cc = C3 // 3
    out = _out(out, (B, N, Cc), qkv, "unet_v2_attention")
    _check(lib().gcl_unet_v2_attention(_p(qkv), _p(out), B, N, int(heads), Cc // heads, _stream()))
    return out


def spectral_modes(Hb: int, Wb: int, modes_h: int, modes_w: int):
    """(mh, mw) of model_v2.py:111-112: the kept modes on an Hb x Wb grid."""
    return min(int(modes_h), Hb), min(int(modes_w), Wb // 2 + 1)


def unet_v2_spectral_pack(w_re, w_im, mh: int, mw: int, out=None):
    """weights_re / weights_im [Cin, Cout, modes_h, modes_w] -> [mh * mw, Cin, Cout, 2] (see gcl_unet_v2_spectral_pack)."""
    if w_re.dim() != 4 or tuple(w_im.shape) != tuple(w_re.shape) or not (w_re.is_contiguous() and w_im.is_contiguous()):
        raise ValueError("unet_v2_spectral_pack: two contiguous [Cin, Cout, modes_h, modes_w] tensors expected")
    Cin, Cout, MH, MW = w_re.shape
    if not (1 <= mh <= MH and 1 <= mw <= MW):
        raise ValueError(f"unet_v2_spectral_pack: {mh} x {mw} modes of {MH} x {MW}")
    out = _out(out, (mh * mw, Cin, Cout, 2), w_re, "unet_v2_spectral_pack")
    _check(lib().gcl_unet_v2_spectral_pack(_p(w_re), _p(w_im), Cin, Cout, MH, MW, int(mh), int(mw), _p(out), _stream()))
    return out


def unet_v2_spectral_fwd(x, mh: int, mw: int, out=None):
    """x [B, Hb, Wb, C] -> X [B, mh * mw, C, 2] (see gcl_unet_v2_spectral_fwd)."""
    if x.dim() != 4 or not x.is_contiguous():
        raise ValueError("unet_v2_spectral_fwd: x is a contiguous [B, Hb, Wb, C] tensor")
    B, Hb, Wb, Cc = x.shape
    out = _out(out, (B, mh * mw, Cc, 2), x, "unet_v2_spectral_fwd")
    _check(lib().gcl_unet_v2_spectral_fwd(_p(x), _p(out), B, Hb, Wb, Cc, int(mh), int(mw), _stream()))
    return out


def unet_v2_spectral_mix(X, packed, out=None):
    """X [B, modes, Cin, 2] times packed [modes, Cin, Cout, 2] -> O [B, modes, Cout, 2] (see gcl_unet_v2_spectral_mix)."""
    if X.dim() != 4 or packed.dim() != 4 or X.shape[3] != 2 or packed.shape[3] != 2 or X.shape[1] != packed.shape[0] \
            or X.shape[2] != packed.shape[1] or not (X.is_contiguous() and packed.is_contiguous()):
        raise ValueError(f"unet_v2_spectral_mix: contiguous X [B, modes, Cin, 2] and packed [modes, Cin, Cout, 2] expected, got "
                         f"{tuple(X.shape)} and {tuple(packed.shape)}")
    B, nm, Cin, _ = X.shape
    Cout = packed.shape[2]
    out = _out(out, (B, nm, Cout, 2), X, "unet_v2_spectral_mix")
    _check(lib().gcl_unet_v2_spectral_mix(_p(X), _p(packed), _p(out), B, nm, Cin, Cout, _stream()))
    return out


def unet_v2_spectral_inv(O, out, mh: int, mw: int):
    """O [B, mh * mw, C, 2] -> out [B, Hb, Wb, C] (a channel slice of contiguous rows is allowed; see
    gcl_unet_v2_spectral_inv)."""
    if out.dim() != 4:
        raise ValueError("unet_v2_spectral_inv: out is a [B, Hb, Wb, C] tensor")
    B, Hb, Wb, Cc = out.shape
    ld = _v2_slice(out, out.shape, "unet_v2_spectral_inv")
    if tuple(O.shape) != (B, mh * mw, Cc, 2) or not O.is_contiguous():
        raise ValueError(f"unet_v2_spectral_inv: O is a contiguous [{B}, {mh * mw}, {Cc}, 2] tensor, got {tuple(O.shape)}")
    _check(lib().gcl_unet_v2_spectral_inv(_p(O), _p(out), ld, B, Hb, Wb, Cc, int(mh), int(mw), _stream()))
    return out


# ======================================================================================================================
# The regional U-Net forecaster's loop around its network (csrc/unet_forecast.hip)
# ======================================================================================================================
def unet_forecast_launches() -> int:
    """Kernels launched by the entry points of csrc/unet_forecast.hip in this process."""
    return int(lib().gcl_unet_forecast_launches())


def _grid_series(series, t0, who):
    if series.dim() != 4 or not series.is_cuda or series.dtype != torch.float16 or not series.is_contiguous():
        raise ValueError(f"{who}: series is a contiguous float16 [T, n_lon, n_lat, Ct] GPU tensor")
    if t0.dim() != 1 or t0.numel() < 1:
        raise ValueError(f"{who}: t0 holds one window start per sample")
    return series.shape


def grid_window_pack(series, t0, mean, std, obs: int, out=None):
    """X [B, obs * C, H = n_lat, W = n_lon] of the windows starting at t0 (int64 [B] on the device) of the fp16 series
    [T, n_lon, n_lat, Ct], C = mean.numel() <= Ct (see gcl_grid_window_pack).  out: the tensor to fill."""
    T, n_lon, n_lat, Ct = _grid_series(series, t0, "grid_window_pack")
    Cc, B = mean.numel(), t0.numel()
    if std.numel() != Cc or not 1 <= Cc <= Ct or obs < 1:
        raise ValueError(f"grid_window_pack: mean and std of C <= {Ct} values and obs >= 1 expected")
    X = _out(out, (B, obs * Cc, n_lat, n_lon), series, "grid_window_pack", exact=True)
    _check(lib().gcl_grid_window_pack(_ph(series), T, n_lon, n_lat, Ct, _pl(t0), _p(mean), _p(std), Cc, int(obs), _p(X), B,
                                      _stream()))
    return X


def grid_forecast_step(out, X, series, t0, chan_kind, mean, std, step: int, X_next, state, acc_count, count, pred=None,
                       ws=None):
    """One autoregressive step around the network (see gcl_grid_forecast_step): out [B, C, H, W] (residual applied) and the
    window X [B, obs * C, H, W] -> X_next (not X), pred (optional) and the scores of `step` added to state float64
    [AR, C, 5], acc_count int64 [AR, C] and count int64 [AR].  chan_kind: uint8 [C] on the device (0 dynamic, 1 static,
    2 forcing); t0: int64 [B] on the device, a negative entry skips its sample."""
    T, n_lon, n_lat, Ct = _grid_series(series, t0, "grid_forecast_step")
    if out.dim() != 4 or X.dim() != 4:
        raise ValueError("grid_forecast_step: out [B, C, H, W] and X [B, obs * C, H, W] expected")
    B, Cc, H, W = out.shape
    if (H, W) != (n_lat, n_lon) or X.shape[0] != B or tuple(X.shape[2:]) != (H, W) or X.shape[1] % Cc or X.shape[1] < Cc:
        raise ValueError(f"grid_forecast_step: out [B, C, {n_lat}, {n_lon}] and X [B, obs * C, {n_lat}, {n_lon}] expected, got "
                         f"{tuple(out.shape)} and {tuple(X.shape)}")
    obs = X.shape[1] // Cc
    if tuple(X_next.shape) != tuple(X.shape) or (pred is not None and tuple(pred.shape) != tuple(out.shape)):
        raise ValueError("grid_forecast_step: X_next has X's shape and pred has out's")
    if not all(t.is_contiguous() for t in (out, X, X_next) + ((pred,) if pred is not None else ())) or t0.numel() != B:
        raise ValueError("grid_forecast_step: contiguous fields and t0 of B values expected")
    if chan_kind.dtype != torch.uint8 or chan_kind.numel() != Cc or not chan_kind.is_cuda or mean.numel() != Cc \
            or std.numel() != Cc:
        raise ValueError(f"grid_forecast_step: chan_kind uint8 [{Cc}] on the device and mean / std of {Cc} values expected")
    if state.dim() != 3 or tuple(state.shape[1:]) != (Cc, 5) or tuple(acc_count.shape) != tuple(state.shape[:2]) \
            or count.numel() != state.shape[0]:
        raise ValueError(f"grid_forecast_step: state [AR, {Cc}, 5], acc_count [AR, {Cc}] and count [AR] expected")
    ws_ptr, ws_bytes = _ws_for(int(lib().gcl_grid_forecast_step_ws_bytes(B, H, W, Cc)), ws, out.device)
    _check(lib().gcl_grid_forecast_step(_p(out), _p(X), _ph(series), T, n_lon, n_lat, Ct, _pl(t0), chan_kind.data_ptr(),
                                        _p(mean), _p(std), Cc, obs, int(step), state.shape[0], _p(X_next), _p(pred),
                                        _pd(state), _pl(acc_count), _pl(count), B, ws_ptr, ws_bytes, _stream()))
    return X_next
