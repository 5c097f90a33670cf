"""ctypes binding of libodx.so (C ABI: include/odx.h).

The product path has no CPU fallback: if the shared library is missing, or no MI355X is
visible, every entry point raises ``OdxUnavailable`` loudly.  Device memory, streams and
collectives come from PyTorch-ROCm; the arithmetic is the hand-written gfx950 HIP in
``online-detection_amd/csrc``.
"""
import ctypes
import os

_LIB = None
# (ODX_LIB_PATH: a development knob — another build of the library)
_LIB_PATH = os.environ.get("ODX_LIB_PATH") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libodx.so")

ODX_OK = 0
KNM_F32, KNM_U24, KNM_BF16 = 0, 1, 2
KNM_CODE = {"f32": KNM_F32, "u24": KNM_U24, "bf16": KNM_BF16}      # Knm.fmt -> the ODX_KNM_* code of include/odx.h
KERNEL_GAUSS, KERNEL_MATERN32, KERNEL_MATERN52 = 0, 1, 2          # ODX_KERNEL_*: the radial kernels of the odx_radial_* entries
STREAM_MAX_VECTORS = 16     # ODX_STREAM_MAX_VECTORS: vectors one odx_gauss_ktk_stream_h2n call serves from one build of K
GRID_MAX_SIGMAS = 4         # ODX_GRID_MAX_SIGMAS: kernel widths one odx_gauss_knm_h2_store_sigmas call builds from one contraction
GEMM_LOWER_ONLY, GEMM_A_UPPER, GEMM_B_UPPER, GEMM_A_LOWER, GEMM_B_LOWER, GEMM_STORE_T = 1, 2, 4, 8, 16, 32


class OdxUnavailable(RuntimeError):
    pass


class OdxError(RuntimeError):
    pass


_vp, _i64, _i32, _f64, _f32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_double, ctypes.c_float

# name -> (restype, argtypes): exactly the declarations of include/odx.h
SIGNATURES = {
    "odx_last_error_string": (ctypes.c_char_p, []),
    "odx_knm_pass_kernel_name": (ctypes.c_char_p, [_i64, _i32, _i32]),
    "odx_version": (_i32, []),
    "odx_device_cus": (_i32, []),
    "odx_set_option": (_i32, [ctypes.c_char_p, _i32]),
    "odx_get_option": (_i32, [ctypes.c_char_p, _vp]),
    "odx_option_default": (_i32, [ctypes.c_char_p, _vp]),
    "odx_release_helper_streams": (_i32, []),
    "odx_set_helper_streams": (_i32, [_vp, _vp]),
    "odx_stream_create_cu_mask": (_i32, [_vp, _i32, _vp]),
    "odx_stream_destroy": (_i32, [_vp]),
    "odx_set_pass_cus": (_i32, [_i32]),
    "odx_set_side_stream_cu_mask": (_i32, [_vp, _i32]),
    "odx_debug_placement": (_i32, [_vp, _i32, _i32, _vp]),
    "odx_row_sqnorm_f32": (_i32, [_vp, _i64, _i64, _i32, _vp, _vp]),
    "odx_row_sqnorm_absmax_f32": (_i32, [_vp, _i64, _i64, _i32, _vp, _vp, _vp]),
    "odx_split_f16_premax": (_i32, [_vp, _i64, _i64, _i32, _vp, _i64, _vp, _vp]),
    "odx_gauss_knm_f32": (_i32, [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _i32, _f64, _vp, _i64, _vp]),
    "odx_gauss_knm_direct_f32": (_i32, [_vp, _i64, _i64, _vp, _i64, _i64, _i32, _f64, _vp, _i64, _vp]),
    "odx_gauss_mmv_f32": (_i32, [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _i32, _f64, _vp, _i64, _vp, _i32, _vp, _i64, _vp]),
    "odx_split_f16": (_i32, [_vp, _i64, _i64, _i32, _vp, _i64, _vp, _vp]),
    "odx_gauss_h2_tile": (_i32, [_i64, _i64]),
    "odx_set_h2_tile": (_i32, [_i32]),
    "odx_gauss_knm_h2": (_i32, [_vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _i32, _f64, _vp, _i64, _vp]),
    "odx_gauss_knm_h2_rhs_workspace_bytes": (_i64, [_i64, _i64]),
    "odx_gauss_knm_h2_rhs": (_i32, [_vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _i32, _f64, _vp, _i64, _vp, _vp, _vp, _i64,
                                    _vp]),
    "odx_gauss_mmv_h2_workspace_bytes": (_i64, [_i64, _i64, _i32]),
    "odx_gauss_mmv_h2": (_i32, [_vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _i32, _f64, _vp, _i64, _vp, _i32, _vp, _i64,
                                _vp, _i64, _vp]),
    "odx_gauss_mmvn_h2_workspace_bytes": (_i64, [_i64, _i64, _i32]),
    "odx_gauss_mmvn_h2": (_i32, [_vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _i32, _f64, _vp, _i64, _i32, _vp, _i64,
                                 _vp, _i64, _vp]),
    "odx_gauss_mmvn_h2_sigmas_workspace_bytes": (_i64, [_i64, _i64, _i32]),
    "odx_gauss_mmvn_h2_sigmas": (_i32, [_vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _i32, _vp, _vp, _i64, _i32, _vp, _i64,
                                        _vp, _i64, _vp]),
    "odx_radial_knm_h2_store": (_i32, [_vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _i32, _f64, _i32, _i32, _vp, _i64, _vp, _i64,
                                       _vp, _vp, _vp, _i64, _vp]),
    "odx_radial_mmv_h2": (_i32, [_vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _i32, _f64, _i32, _vp, _i64, _vp, _i32, _vp, _i64,
                                 _vp, _i64, _vp]),
    "odx_radial_mmvn_h2": (_i32, [_vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _i32, _f64, _i32, _vp, _i64, _i32, _vp, _i64,
                                  _vp, _i64, _vp]),
    "odx_falkon_precond_radial_f64": (_i32, [_vp, _i64, _i64, _i32, _f64, _i32, _f64, _f64, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _i64, _vp]),
    "odx_falkon_precond_path_radial_f64": (_i32, [_vp, _i64, _i64, _i32, _f64, _i32, _vp, _i32, _f64, _vp, _vp, _vp, _i64, _vp, _vp, _i64,
                                                  _vp]),
    "odx_row_sqnorm_b16": (_i32, [_vp, _i64, _i64, _i32, _i32, _vp, _vp]),
    "odx_gauss_knm_b16_store_workspace_bytes": (_i64, [_i64, _i64]),
    "odx_gauss_knm_b16_store": (_i32, [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _i32, _i32, _f64, _i32, _vp, _i64, _vp, _i64, _vp, _vp,
                                       _vp, _i64, _vp]),
    "odx_gauss_mmv_b16_workspace_bytes": (_i64, [_i64, _i64, _i32]),
    "odx_gauss_mmv_b16": (_i32, [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _i32, _i32, _f64, _vp, _i64, _vp, _i32, _vp, _i64, _vp, _i64,
                                 _vp]),
    "odx_gauss_mmvn_b16_workspace_bytes": (_i64, [_i64, _i64, _i32]),
    "odx_gauss_mmvn_b16": (_i32, [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _i32, _i32, _f64, _vp, _i64, _i32, _vp, _i64, _vp, _i64,
                                  _vp]),
    "odx_gauss_knm_h2_store_sigmas_workspace_bytes": (_i64, [_i64, _i64, _i32]),
    "odx_gauss_knm_h2_store_sigmas": (_i32, [_vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _i32, _vp, _i32, _i32, _vp, _i64, _vp,
                                             _i64, _vp, _vp, _i64, _vp, _i64, _vp]),
    "odx_falkon_cg_workspace_bytes": (_i64, [_i64, _i64]),
    "odx_falkon_cg_f64": (_i32, [_vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _i64, _vp, _f64, _f64, _i32, _i32, _f64, _f64, _vp, _vp,
                                 _i64, _vp]),
    "odx_falkon_cg_batched_workspace_bytes": (_i64, [_i32, _vp, _vp]),
    "odx_falkon_cg_batched_f64": (_i32, [_i32, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _vp, _i64, _vp, _f64, _i32, _i32, _f64, _f64,
                                         _vp, _vp, _i64, _vp]),
    "odx_falkon_cg_batched_q_workspace_bytes": (_i64, [_i32, _vp, _vp, _i32]),
    "odx_falkon_cg_batched_q_f64": (_i32, [_i32, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _i64, _i64, _i64, _vp, _i64, _vp, _f64, _i32, _i32,
                                           _f64, _f64, _vp, _vp, _i64, _vp]),
    "odx_knm_fwd_bwd_workspace_bytes": (_i64, [_i64, _i64]),
    "odx_set_pass_reserved_cus": (_i32, [_i32]),
    "odx_knm_fwd_bwd": (_i32, [_vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _i64, _vp]),
    "odx_knm_fwd_bwd2_workspace_bytes": (_i64, [_i64, _i64]),
    "odx_knm_fwd_bwd2": (_i32, [_vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "odx_knm_ld": (_i64, [_i64, _i32]),
    "odx_knm_bytes": (_i64, [_i64, _i64, _i32]),
    "odx_gauss_knm_h2_store": (_i32, [_vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _i32, _f64, _i32, _vp, _i64, _vp, _i64,
                                      _vp, _vp, _vp, _i64, _vp]),
    "odx_knm_fwd_bwd_t": (_i32, [_vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "odx_knm_fwd_bwd2_t": (_i32, [_vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "odx_knm_fwd_bwd_q_t": (_i32, [_vp, _i64, _vp, _i64, _i32, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "odx_knm_fwd_bwd2_q_t": (_i32, [_vp, _i64, _vp, _i64, _i32, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "odx_knm_fwd_bwd_q_cols_t": (_i32, [_vp, _i64, _vp, _i64, _i32, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp]),
    "odx_knm_fwd_bwd2_q_cols_t": (_i32, [_vp, _i64, _vp, _i64, _i32, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp,
                                         _vp]),
    "odx_knm_fwd_bwd_q_rows_t": (_i32, [_vp, _i64, _vp, _i64, _i32, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "odx_knm_fwd_bwd_q_rows_cols_t": (_i32, [_vp, _i64, _vp, _i64, _i32, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp,
                                             _vp, _vp]),
    "odx_cols_fold_f64": (_i32, [_vp, _i64, _vp, _vp, _i64, _vp, _vp]),
    "odx_cols_expand_f64": (_i32, [_vp, _i64, _vp, _i64, _vp, _vp]),
    "odx_cg_scores_axpy_f64": (_i32, [_vp, _vp, _vp, _i64, _vp]),
    "odx_cg_scores_store_f32": (_i32, [_vp, _i64, _vp, _i64, _vp]),
    "odx_knm_fwd_bwd_q_workspace_bytes": (_i64, [_i64, _i64, _i32]),
    "odx_knm_fwd_bwd_q": (_i32, [_vp, _i64, _vp, _i64, _i32, _i64, _i64, _vp, _vp, _vp, _vp, _i64, _vp]),
    "odx_knm_fwd_bwd2_q_workspace_bytes": (_i64, [_i64, _i64, _i32]),
    "odx_knm_fwd_bwd2_q": (_i32, [_vp, _i64, _vp, _i64, _i32, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "odx_knm_fwd_bwdn_q_workspace_bytes": (_i64, [_i64, _i64, _i32, _i32]),
    "odx_knm_fwd_bwdn_q": (_i32, [_vp, _i64, _vp, _i64, _i32, _i64, _i64, _i32, _vp, _i64, _vp, _i64, _vp, _i64, _vp]),
    "odx_knm_fwd_bwdn_q_rw_workspace_bytes": (_i64, [_i64, _i64, _i32, _i32]),
    "odx_knm_fwd_bwdn_q_rw": (_i32, [_vp, _i64, _vp, _i64, _i32, _i64, _i64, _i32, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _vp, _i64,
                                     _vp, _i64, _vp]),
    "odx_knm_bwdn_q_workspace_bytes": (_i64, [_i64, _i64, _i32, _i32]),
    "odx_knm_bwdn_q": (_i32, [_vp, _i64, _vp, _i64, _i32, _i64, _i64, _i32, _vp, _i64, _vp, _i64, _vp, _i64, _vp]),
    "odx_knm_fwdn_q_workspace_bytes": (_i64, [_i64, _i64, _i32, _i32]),
    "odx_knm_fwdn_q": (_i32, [_vp, _i64, _vp, _i64, _i32, _i64, _i64, _i32, _vp, _i64, _vp, _i64, _vp, _i64, _vp]),
    "odx_knm_mv": (_i32, [_vp, _i64, _vp, _i64, _i32, _i64, _i64, _vp, _vp, _i64, _vp]),
    "odx_gauss_ktk_stream_h2_rows": (_i64, [_i64, _i32]),
    "odx_gauss_ktk_stream_h2_workspace_bytes": (_i64, [_i64, _i64, _i32]),
    "odx_gauss_ktk_stream_h2": (_i32, [_vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _i32, _f64, _vp, _vp, _vp, _vp, _vp, _vp,
                                       _i64, _vp]),
    "odx_gauss_ktk_stream_h2n_rows": (_i64, [_i64, _i32]),
    "odx_gauss_ktk_stream_h2n_workspace_bytes": (_i64, [_i64, _i64, _i32, _i32]),
    "odx_gauss_ktk_stream_h2n": (_i32, [_vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _i32, _f64, _i32, _vp, _i64, _vp, _i64,
                                        _vp, _i64, _vp]),
    "odx_split_f8": (_i32, [_vp, _i64, _i64, _i32, _vp, _i64, _vp, _vp, _vp]),
    "odx_gauss_knm_f8_store": (_i32, [_vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _i32, _f64, _i32, _vp, _i64, _vp, _i64,
                                      _vp, _vp, _vp, _i64, _vp]),
    "odx_gauss_mmv_f8": (_i32, [_vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _i32, _f64, _vp, _i64, _vp, _i32, _vp, _i64,
                                _vp, _i64, _vp]),
    "odx_cg_residual": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "odx_falkon_precond_workspace_bytes": (_i64, [_i64, _i32]),
    "odx_falkon_precond_f64": (_i32, [_vp, _i64, _i64, _i32, _f64, _f64, _f64, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _i64, _vp]),
    "odx_falkon_precond_path_workspace_bytes": (_i64, [_i64, _i32, _i32]),
    "odx_falkon_precond_path_f64": (_i32, [_vp, _i64, _i64, _i32, _f64, _vp, _i32, _f64, _vp, _vp, _vp, _i64, _vp, _vp, _i64, _vp]),
    "odx_falkon_precond_batched_workspace_bytes": (_i64, [_i64, _i32, _i32]),
    "odx_falkon_precond_batched_f64": (_i32, [_vp, _vp, _vp, _i32, _i64, _i32, _f64, _f64, _f64, _vp, _i64, _i64, _vp, _vp, _i64, _vp]),
    "odx_falkon_precond_batched_partial_f64": (_i32, [_vp, _vp, _vp, _i32, _i64, _i32, _f64, _f64, _f64, _i64, _vp, _i64, _i64, _vp, _vp, _i64, _vp]),
    "odx_tri_blocked_mv_workspace_bytes": (_i64, [_i64]),
    "odx_tri_blocked_mv_f64": (_i32, [_vp, _i64, _i64, _i32, _vp, _i32, _vp, _f64, _f64, _vp, _vp, _vp, _i64, _vp]),
    "odx_trmv_f64": (_i32, [_vp, _i64, _i64, _i32, _vp, _f64, _f64, _vp, _vp, _vp]),
    "odx_trmvn_f64": (_i32, [_vp, _i64, _i64, _i32, _i32, _vp, _i64, _f64, _f64, _vp, _i64, _vp, _i64, _vp]),
    "odx_cg_init": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "odx_cg_step": (_i32, [_vp, _vp, _vp, _vp, _vp, _f64, _i32, _i64, _vp]),
    "odx_cg_finish": (_i32, [_vp, _vp, _vp, _f64, _f64, _i64, _vp]),
    "odx_axpby_f64": (_i32, [_f64, _vp, _f64, _vp, _i64, _vp]),
    "odx_gemm_nt_f64": (_i32, [_vp, _i64, _vp, _i64, _vp, _i64, _i64, _i64, _i64, _f64, _f64, _i32, _vp]),
    "odx_gemm_nt_f32": (_i32, [_vp, _i64, _vp, _i64, _vp, _i64, _i64, _i64, _i64, _f32, _f32, _i32, _vp]),
    "odx_potrf_workspace_bytes": (_i64, [_i64]),
    "odx_potrf_f64": (_i32, [_vp, _i64, _i64, _vp, _vp, _i64, _vp]),
    "odx_trtri_workspace_bytes": (_i64, [_i64]),
    "odx_trtri_f64": (_i32, [_vp, _i64, _i64, _vp, _vp, _i64, _vp, _i64, _vp]),
    "odx_trtri_partial_f64": (_i32, [_vp, _i64, _i64, _i64, _vp, _vp, _i64, _vp, _i64, _vp]),
    "odx_convert_f32_f64": (_i32, [_vp, _i64, _vp, _i64, _i64, _i64, _vp]),
    "odx_convert_f64_f32": (_i32, [_vp, _i64, _vp, _i64, _i64, _i64, _vp]),
    "odx_knm_rowquad_f64": (_i32, [_vp, _i64, _i64, _i64, _vp, _i64, _vp, _vp]),
    "odx_radial_kmm_f64": (_i32, [_vp, _i64, _i64, _i32, _f64, _i32, _vp, _f64, _vp, _i64, _vp, _vp]),
    "odx_knm_gram_f64": (_i32, [_vp, _i64, _i64, _i64, _vp, _vp, _f64, _vp, _i64, _vp, _vp]),
    "odx_knm_gram_rhsn_f64": (_i32, [_vp, _i64, _i64, _i64, _vp, _vp, _i64, _i32, _f64, _vp, _i64, _vp, _i64, _vp]),
    "odx_symvn_f64": (_i32, [_vp, _i64, _i64, _i32, _vp, _i64, _f64, _vp, _i64, _vp]),
    "odx_knm_fwd_bwd_rw": (_i32, [_vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "odx_logistic_rows_f64": (_i32, [_vp, _vp, _i64, _f64, _vp, _vp, _vp, _vp]),
    "odx_knm_fwd_bwd_q_rw": (_i32, [_vp, _i64, _vp, _i64, _i32, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "odx_rls_gram_workspace_bytes": (_i64, [_i64, _i32]),
    "odx_rls_gram_f64": (_i32, [_vp, _i64, _i32, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp]),
    "odx_rls_solve_workspace_bytes": (_i64, [_i32]),
    "odx_rls_solve_f64": (_i32, [_vp, _i64, _i32, _f64, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _vp]),
    "odx_rls_gram_batched_workspace_bytes": (_i64, [_i64, _i32]),
    "odx_rls_gram_batched_f64": (_i32, [_vp, _i64, _i32, _vp, _i64, _vp, _vp, _i32, _vp, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _vp]),
    "odx_rls_pad_index": (_i32, [_vp, _i64, _vp, _vp, _i32, _i64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "odx_rls_gram_raw_batched_f64": (_i32, [_vp, _i64, _i32, _vp, _i64, _vp, _vp, _i32, _vp, _i64, _vp, _i64, _i64, _vp, _i64, _vp]),
    "odx_rls_fold_whitened_f64": (_i32, [_vp, _i64, _i32, _i32, _vp, _vp, _vp, _i64, _i64, _vp, _i64, _i64, _vp]),
    "odx_rls_xty_batched_f64": (_i32, [_vp, _i64, _i32, _vp, _i64, _vp, _vp, _i32, _vp, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _vp]),
    "odx_rls_rows_form": (_i32, [_vp, _i64, _i32]),
    "odx_rls_solve_batched_workspace_bytes": (_i64, [_i32, _i32]),
    "odx_rls_solve_batched_f64": (_i32, [_vp, _i64, _i64, _i32, _i32, _f64, _vp, _i64, _i64, _vp, _i64, _i64, _vp, _vp, _i64, _vp]),
    "odx_rls_predict_rows_f64": (_i32, [_vp, _i64, _i32, _vp, _i64, _vp, _i64, _vp, _i64, _vp]),
    "odx_rls_predict_rows_batched_f64": (_i32, [_vp, _i64, _i32, _vp, _vp, _i32, _i64, _vp, _i64, _i64, _vp, _i64, _vp]),
    "odx_roi_align_fwd_f32": (_i32, [_vp, _i32, _i32, _i32, _i32, _vp, _i32, _f32, _i32, _i32, _i32, _vp, _vp]),
    "odx_split_f16_taps3x3": (_i32, [_vp, _i64, _i64, _i32, _i32, _i32, _vp, _i64, _vp, _vp]),
    "odx_gemm_b16": (_i32, [_vp, _i64, _i64, _vp, _i64, _i64, _i32, _i32, _vp, _vp, _i64, _i32, _vp, _i64, _i32, _vp]),
    "odx_taps3x3_16": (_i32, [_vp, _i64, _i64, _i32, _i32, _i32, _vp, _i64, _vp]),
    "odx_gemm_h2_f32": (_i32, [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _i32, _vp, _vp, _i64, _i32, _vp, _i64, _vp]),
    "odx_roi_align_rows_f32": (_i32, [_vp, _i32, _i32, _i32, _i32, _vp, _i32, _f32, _i32, _i32, _i32, _i32, _vp, _vp]),
    "odx_roi_align_rows_nhwc_f32": (_i32, [_vp, _i64, _i32, _i32, _i32, _i32, _vp, _i32, _f32, _i32, _i32, _i32, _i32, _vp, _vp]),
    "odx_gemm_h2_max_f32": (_i32, [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _i32, _vp, _vp, _i64, _i32, _vp, _i64, _vp, _vp]),
    "odx_split_f16_taps3x3_premax": (_i32, [_vp, _i64, _i64, _i32, _i32, _i32, _vp, _i64, _vp, _vp]),
    "odx_gemm_h2_taps_supported": (_i32, [_i64, _i64, _i32, _i64]),
    "odx_gemm_h2_taps_f32": (_i32, [_vp, _i64, _vp, _i64, _i32, _i32, _i32, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _i32, _vp, _i64, _vp,
                                    _vp, _i64, _f32, _f32, _vp, _vp]),
    "odx_gemm_h2_chain_f32": (_i32, [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _i32, _vp, _vp, _i64, _i32, _vp, _i64, _vp,
                                     _vp, _i64, _f32, _f32, _vp, _vp]),
    "odx_taps3x3_packed": (_i32, [_vp, _i64, _i64, _i32, _i32, _i32, _vp, _i64, _vp]),
    "odx_rpn_label_f32": (_i32, [_vp, _i32, _vp, _vp, _i32, _i32, _f32, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "odx_det_label_f32": (_i32, [_vp, _vp, _i32, _vp, _i32, _i32, _f32, _f32, _f32, _f32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "odx_box_targets_f32": (_i32, [_vp, _vp, _i64, _vp, _vp]),
    "odx_debug_gemm_h2_mf32": (_i32, [_vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _i32, _vp, _i64, _vp]),
    "odx_gemm_b16_taps_supported": (_i32, [_i64, _i64, _i32, _i64]),
    "odx_gemm_b16_taps": (_i32, [_vp, _i64, _i64, _i32, _i32, _i32, _vp, _i64, _i64, _i32, _vp, _vp, _i64, _i32, _vp, _i64, _i32, _vp]),
    "odx_roi_align_fpn_f32": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp]),
    "odx_roi_align_fpn_nhwc_f32": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp]),
    "odx_stem_pool_rows_f32": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _vp, _i64, _vp, _vp]),
    "odx_stem_pool_rows_16": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _i64, _vp]),
    "odx_upsample_add_rows_f32": (_i32, [_vp, _i64, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp]),
    "odx_upsample_add_rows_16": (_i32, [_vp, _i64, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "odx_roi_align_fpn_nhwc_16": (_i32, [_vp, _i32, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp]),
    "odx_nms_workspace_bytes": (_i64, [_i32]),
    "odx_nms_f32": (_i32, [_vp, _i32, _f32, _vp, _vp, _i64, _vp]),
    "odx_nms_first_f32": (_i32, [_vp, _i32, _f32, _i32, _vp, _vp, _i64, _vp]),
    "odx_nms_batched_workspace_bytes": (_i64, [_i32, _i32]),
    "odx_nms_batched_f32": (_i32, [_vp, _vp, _i32, _i32, _f32, _vp, _vp, _i64, _vp]),
    "odx_rpn_topk_decode_f32": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _f32, _f32, _f32, _vp, _vp, _vp, _vp]),
    "odx_nms_compact_f32": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp]),
    "odx_nms_batched_first_f32": (_i32, [_vp, _vp, _i32, _i32, _f32, _i32, _vp, _vp, _i64, _vp]),
    "odx_paste_masks_u8": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _f32, _i32, _vp, _vp]),
    "odx_bias_act_nchw_f32": (_i32, [_vp, _vp, _vp, _i64, _i32, _i64, _i32, _vp]),
    "odx_bias_act_nchw_16": (_i32, [_vp, _vp, _vp, _i32, _i64, _i32, _i64, _i32, _vp]),
}


def radial_of(sigma):
    """(sigma, ODX_KERNEL_* kind) of the `sigma` argument of a backend wrapper that knows the radial kernels: a number is
    the Gaussian's width, a kernel object (odx.MaternKernel) carries .sigma and .kind.  Wrappers that were not taught the
    kind do float(sigma) on the object and fail there (it defines no __float__): nothing computes a Gaussian silently."""
    kind = getattr(sigma, "kind", None)
    if kind is None:
        return float(sigma), KERNEL_GAUSS
    return float(sigma.sigma), int(kind)


def lib_path():
    return _LIB_PATH


def load():
    """dlopen libodx.so and bind every symbol of include/odx.h (no GPU needed for this)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(_LIB_PATH):
        raise OdxUnavailable(
            "libodx.so not found at %s — build it with `make -C online-detection_amd/csrc` "
            "(or __graft_entry__.build()); there is no CPU fallback." % _LIB_PATH)
    lib = ctypes.CDLL(_LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError here = header / library mismatch
        fn.restype = res
        fn.argtypes = args
    _LIB = lib
    return lib


def check(rc, what=""):
    if rc != ODX_OK:
        msg = load().odx_last_error_string().decode("utf-8", "replace")
        raise OdxError("%s failed (code %d): %s" % (what or "libodx call", rc, msg))


def require_gpu():
    import torch
    if not torch.cuda.is_available():
        raise OdxUnavailable("no HIP device visible: the odx hot path runs on MI355X only (no CPU fallback)")
    return load()
