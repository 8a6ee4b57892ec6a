"""ctypes binding of libgphip.so (include/gphip.h).  No torch, no CPU fallback.

The product path fails loudly when the HIP library is missing or no GPU is
visible: ``load()`` raises ``RuntimeError``; nothing here (or anywhere in this
package) imports ``oracle/``.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libgphip.so")

c_double_p = ctypes.POINTER(ctypes.c_double)
c_int64_p = ctypes.POINTER(ctypes.c_int64)
c_int_p = ctypes.POINTER(ctypes.c_int)

GP_KERNEL_RBF, GP_KERNEL_MATERN52 = 0, 1
GP_KERNEL_MATERN32, GP_KERNEL_EXPONENTIAL = 2, 3
GP_ACQ_EI, GP_ACQ_LCB, GP_ACQ_MPI = 0, 1, 2
GP_ACQ_PER_COST = 0x100      # or-ed into a scoring call's type: the scores are divided by the resident cost surface
GP_ACQ_POF = 3               # the rule whose value is 1: valid only with GP_ACQ_TIMES_FEAS (the probability of feasibility alone)
GP_ACQ_MES = 4               # max-value entropy search over the handle's resident samples of the minimum's value (gp_mes_set)
GP_PATHS_MAX_S, GP_PATHS_MAX_F, GP_PATHS_MAX_ROWS = 64, 4096, 8   # posterior paths: paths, features, locations per rows call
GP_QEI_MAX_S, GP_QEI_MAX_Q = 4096, 8   # joint expected improvement: base samples resident, locations of a batch
GP_KG_MAX_A = 256                      # knowledge gradient: discretisation points resident
GP_NEI_MAX_S = 64                      # noisy EI: fantasies resident
GP_NEI_MAX_ROWS = 8                    # ... and locations of a fused gp_nei_rows call
GP_MES_MAX_K, GP_MES_MAX_G = 64, 64   # samples of the minimum's value; trial values per gp_mes_logsurv call
GP_ACQ_TIMES_FEAS = 0x200    # or-ed into a table scoring call's type: the scores are multiplied by the cached probability of feasibility
GP_FEAS_MAX = 8
GP_EHVI_MAX_OBJ, GP_EHVI_MAX_LEVELS, GP_EHVI_MAX_CELLS = 3, 256, 32768   # expected hypervolume improvement: objectives, levels per objective, cells
GP_ERR_ARG, GP_ERR_HIP, GP_ERR_STATE, GP_ERR_RCCL, GP_ERR_NOT_PD_DIAG = -1, -2, -3, -4, -5
GP_LAPLACE_NOT_CONVERGED = 1 << 30     # gp_laplace_fit: the Newton iteration reached its cap
LAPLACE_MAX_ITER = 40                  # ... the cap the Python layer asks for

# every symbol include/gphip.h declares: (name, restype, argtypes)
_vp = ctypes.c_void_p
SIGNATURES = [
    ("gp_last_error", ctypes.c_char_p, []),
    ("gp_version", ctypes.c_char_p, []),
    ("gp_device_count", ctypes.c_int, [c_int_p]),
    ("gp_device_info", ctypes.c_int, [ctypes.c_int, ctypes.c_char_p, ctypes.c_int, c_int_p, c_int64_p]),
    ("gp_create", ctypes.c_int, [ctypes.POINTER(_vp), ctypes.c_int]),
    ("gp_destroy", ctypes.c_int, [_vp]),
    ("gp_shutdown", ctypes.c_int, []),
    ("gp_get_fit_state", ctypes.c_int, [_vp, c_double_p, c_double_p, c_double_p]),
    ("gp_get_dl_dk", ctypes.c_int, [_vp, c_double_p]),
    ("gp_lml_grad_lds", ctypes.c_int, [_vp, c_int64_p, c_int64_p]),
    ("gp_posterior_samples", ctypes.c_int, [_vp, ctypes.c_int, c_double_p, ctypes.c_int, ctypes.c_int, c_double_p,
                                            c_double_p, c_double_p]),
    ("gp_acq_topk", ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                   ctypes.c_double, ctypes.c_int, ctypes.c_int, c_int64_p, c_double_p]),
    ("gp_comm_allgather_topk", ctypes.c_int, [_vp, ctypes.c_int, c_double_p, c_int64_p, c_double_p, c_int64_p]),
    ("gp_set_data", ctypes.c_int, [_vp, c_double_p, c_double_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int]),
    ("gp_set_params", ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_double, c_double_p, ctypes.c_double]),
    ("gp_set_gower", ctypes.c_int, [_vp, ctypes.c_int, c_int_p, c_double_p]),
    ("gp_fit", ctypes.c_int, [_vp, ctypes.c_int, c_double_p, c_double_p, c_double_p]),
    ("gp_fit_predict", ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, c_double_p, c_double_p, c_double_p, c_double_p,
                                      c_double_p]),
    ("gp_get_alpha", ctypes.c_int, [_vp, c_double_p]),
    ("gp_get_chol", ctypes.c_int, [_vp, c_double_p]),
    ("gp_get_woodbury_inv", ctypes.c_int, [_vp, c_double_p]),
    ("gp_kernel_matrix", ctypes.c_int, [_vp, c_double_p]),
    ("gp_cross_kernel_matrix", ctypes.c_int, [_vp, c_double_p, ctypes.c_int64, c_double_p]),
    ("gp_lml_grad", ctypes.c_int, [_vp, c_double_p, c_double_p, c_double_p]),
    ("gp_fit_grad", ctypes.c_int, [_vp, ctypes.c_int, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p,
                                   c_double_p]),
    ("gp_lml_grad_x", ctypes.c_int, [_vp, c_double_p]),
    ("gp_fit_grad_x", ctypes.c_int, [_vp, ctypes.c_int, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p,
                                     c_double_p, c_double_p]),
    ("gp_fit_grad_batch", ctypes.c_int, [_vp, ctypes.c_int, c_double_p, c_double_p, c_double_p, ctypes.c_int, c_double_p,
                                         c_double_p, c_double_p, c_double_p, c_double_p, c_double_p, c_int_p]),
    ("gp_fit_grad_x_batch", ctypes.c_int, [_vp, ctypes.c_int, c_double_p, c_double_p, c_double_p, c_double_p, ctypes.c_int,
                                           c_double_p, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p,
                                           c_int_p]),
    ("gp_fit_grad_warp_batch", ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, c_double_p, c_double_p, c_double_p, c_double_p,
                                              c_double_p, ctypes.c_int, c_double_p, c_double_p, c_double_p, c_double_p,
                                              c_double_p, c_double_p, c_double_p, c_double_p, c_double_p, c_int_p]),
    ("gp_set_candidates",ctypes.c_int, [_vp, c_double_p, ctypes.c_int64]),
    ("gp_set_candidates_kumar", ctypes.c_int, [_vp, c_double_p, ctypes.c_int64, c_int_p, c_double_p, c_double_p, c_double_p,
                                               c_double_p, c_double_p]),
    ("gp_predict", ctypes.c_int, [_vp, ctypes.c_int, c_double_p, c_double_p]),
    ("gp_set_output_warp", ctypes.c_int, [_vp, ctypes.c_int, c_double_p, ctypes.c_double, c_double_p]),
    ("gp_get_targets", ctypes.c_int, [_vp, c_double_p]),
    ("gp_warp_grad", ctypes.c_int, [_vp, c_double_p, c_double_p]),
    ("gp_fit_grad_warp", ctypes.c_int, [_vp, ctypes.c_int, c_double_p, ctypes.c_double, ctypes.c_int, c_double_p, c_double_p,
                                        c_double_p, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p]),
    ("gp_predict_warped", ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_int, c_double_p,
                                         c_double_p, ctypes.c_int, c_double_p, c_double_p, c_double_p, c_double_p]),
    ("gp_warp_moments", ctypes.c_int, [_vp, c_double_p, c_double_p, ctypes.c_int64, ctypes.c_double, ctypes.c_double,
                                       ctypes.c_int, c_double_p, c_double_p, ctypes.c_int, c_double_p, c_double_p, c_double_p,
                                       c_double_p]),
    ("gp_warp_inverse", ctypes.c_int, [_vp, c_double_p, ctypes.c_int64, c_double_p]),
    ("gp_sparse_set_inducing", ctypes.c_int, [_vp, c_double_p, ctypes.c_int64]),
    ("gp_sparse_fit", ctypes.c_int, [_vp, ctypes.c_int, c_double_p, c_double_p, c_double_p]),
    ("gp_sparse_fit_grad", ctypes.c_int, [_vp, ctypes.c_int, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p]),
    ("gp_sparse_fit_grad_batch", ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int64, c_double_p, c_double_p, c_double_p, c_double_p,
                                                ctypes.c_int, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p,
                                                c_double_p, c_int_p]),
    ("gp_sparse_batch_bytes", ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]),
    ("gp_sparse_posterior", ctypes.c_int, [_vp, c_double_p, c_double_p]),
    ("gp_sparse_predict", ctypes.c_int, [_vp, c_double_p, ctypes.c_int64, ctypes.c_int, c_double_p, c_double_p, c_double_p,
                                         c_double_p]),
    ("gp_sparse_fmin", ctypes.c_int, [_vp, c_double_p]),
    ("gp_sparse_set_candidates", ctypes.c_int, [_vp, c_double_p, ctypes.c_int64]),
    ("gp_sparse_acq", ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                     ctypes.c_int, ctypes.c_int, c_double_p, ctypes.c_int, c_double_p, c_double_p, c_double_p,
                                     c_double_p]),
    ("gp_sparse_acq_argbest", ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                             ctypes.c_double, ctypes.c_int, ctypes.c_int, c_double_p, ctypes.c_int, c_double_p,
                                             c_double_p, ctypes.c_int, c_int64_p, ctypes.c_int, c_int64_p, c_double_p]),
    ("gp_sparse_acq_topk", ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                          ctypes.c_double, ctypes.c_int, ctypes.c_int, c_int64_p, c_double_p]),
    # (void* for the pointers of the two rows entries, as for gp_predict_rows / gp_acq_rows below)
    ("gp_sparse_predict_rows", ctypes.c_int, [_vp, _vp, ctypes.c_int64, ctypes.c_int, _vp, _vp, _vp, _vp]),
    ("gp_sparse_acq_rows", ctypes.c_int, [_vp, _vp, ctypes.c_int64, ctypes.c_int, ctypes.c_double, ctypes.c_double,
                                          ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_int, _vp, ctypes.c_int,
                                          _vp, _vp, _vp, _vp]),
    ("gp_sparse_rows_stats", ctypes.c_int, [_vp, c_int64_p, c_int64_p]),
    ("gp_sparse_predict_full_cov", ctypes.c_int, [_vp, c_double_p, ctypes.c_int64, ctypes.c_int, c_double_p, c_double_p]),
    ("gp_sparse_posterior_samples", ctypes.c_int, [_vp, c_double_p, ctypes.c_int64, ctypes.c_int, c_double_p, ctypes.c_int,
                                                   ctypes.c_int, c_double_p, c_double_p, c_double_p]),
    ("gp_sparse_cov_set_points", ctypes.c_int, [_vp, c_double_p, ctypes.c_int64]),
    # (void* for the pointers of the per-candidate entry, as for the rows entries above)
    ("gp_sparse_cov_between", ctypes.c_int, [_vp, _vp, ctypes.c_int64, _vp]),
    ("gp_ens_fit", ctypes.c_int, [_vp, ctypes.c_int, c_double_p, c_double_p, c_double_p, ctypes.c_int, c_double_p, c_double_p,
                                  c_double_p, c_double_p]),
    ("gp_ens_info", ctypes.c_int, [_vp, c_int_p]),
    # (void* for the pointers of the two rows entries, as for gp_predict_rows / gp_acq_rows below)
    ("gp_ens_predict_rows", ctypes.c_int, [_vp, _vp, ctypes.c_int64, ctypes.c_int, _vp, _vp, _vp, _vp]),
    ("gp_ens_acq_rows", ctypes.c_int, [_vp, _vp, ctypes.c_int64, ctypes.c_int, ctypes.c_double, _vp, _vp]),
    ("gp_ens_acq", ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_double, c_double_p]),
    ("gp_ens_acq_argbest", ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_double, ctypes.c_int, c_int64_p, c_double_p]),
    ("gp_es_set_representers", ctypes.c_int, [_vp, c_double_p, ctypes.c_int, ctypes.c_double, ctypes.c_double, c_double_p,
                                              c_double_p]),
    ("gp_es_pmin", ctypes.c_int, [_vp, c_double_p, c_double_p, ctypes.c_int, ctypes.c_int, ctypes.c_double, c_double_p,
                                  c_double_p, c_double_p, c_int_p, c_int_p]),
    ("gp_es_set_belief", ctypes.c_int, [_vp, c_double_p, c_double_p, c_double_p, c_double_p, ctypes.c_int, c_double_p,
                                        ctypes.c_int]),
    ("gp_es_acq", ctypes.c_int, [_vp, ctypes.c_double, c_double_p]),
    ("gp_es_acq_argbest", ctypes.c_int, [_vp, ctypes.c_double, ctypes.c_int, c_int64_p, c_double_p]),
    ("gp_es_acq_rows", ctypes.c_int, [_vp, _vp, ctypes.c_int64, ctypes.c_double, _vp]),
    ("gp_predict_full_cov", ctypes.c_int, [_vp, ctypes.c_int, c_double_p, c_double_p]),
    ("gp_predict_grad", ctypes.c_int, [_vp, c_double_p, c_double_p]),
    ("gp_fmin", ctypes.c_int, [_vp, c_double_p]),
    ("gp_acq", ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                              ctypes.c_double, c_double_p]),
    ("gp_acq_argbest", ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                      ctypes.c_double, ctypes.c_int, c_int64_p, c_double_p]),
    ("gp_acq_grad", ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                   ctypes.c_double, c_double_p, c_double_p]),
    ("gp_acq_lp", ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                 ctypes.c_int, c_double_p, ctypes.c_int, c_double_p, c_double_p, c_double_p]),
    ("gp_acq_lp_argbest", ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                         ctypes.c_double, ctypes.c_int, c_double_p, ctypes.c_int, c_double_p, c_double_p,
                                         ctypes.c_int, c_int64_p, ctypes.c_int, c_int64_p, c_double_p]),
    ("gp_acq_lp_grad", ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                      ctypes.c_int, c_double_p, ctypes.c_int, c_double_p, c_double_p, c_double_p, c_double_p]),
    # (the double* arguments of these two are declared void*: the caller passes ndarray.ctypes.data, an integer -- building a
    # typed ctypes pointer costs ~4 us apiece, a tenth of the whole call)
    ("gp_predict_rows", ctypes.c_int, [_vp, _vp, ctypes.c_int64, ctypes.c_int, _vp, _vp, _vp, _vp]),
    ("gp_acq_rows", ctypes.c_int, [_vp, _vp, ctypes.c_int64, ctypes.c_int, ctypes.c_double, ctypes.c_double,
                                   ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_int, _vp, ctypes.c_int,
                                   _vp, _vp, _vp, _vp]),
    ("gp_rows_stats", ctypes.c_int, [_vp, c_int64_p, c_int64_p]),
    ("gp_rows_pass_stats", ctypes.c_int, [_vp, c_int64_p, c_int64_p]),
    ("gp_append", ctypes.c_int, [_vp, c_double_p, ctypes.c_int64, c_double_p, c_double_p, c_double_p]),
    ("gp_append_stats", ctypes.c_int, [_vp, c_int64_p, c_int64_p, c_int64_p]),
    ("gp_comm_unique_id", ctypes.c_int, [ctypes.c_char_p]),
    ("gp_comm_init", ctypes.c_int, [_vp, ctypes.c_char_p, ctypes.c_int, ctypes.c_int]),
    ("gp_comm_destroy", ctypes.c_int, [_vp]),
    ("gp_comm_info", ctypes.c_int, [_vp, c_int_p, c_int_p]),
    ("gp_comm_allgather_best", ctypes.c_int, [_vp, ctypes.c_double, ctypes.c_int64, c_double_p, c_int64_p]),
    ("gp_comm_bcast_fit", ctypes.c_int, [_vp, ctypes.c_int]),
    ("gp_comm_version", ctypes.c_int, [c_int_p]),
    ("gp_comm_selftest_fit_record", ctypes.c_int, [c_double_p, c_double_p, c_int_p]),
    ("gp_group_create", ctypes.c_int, [ctypes.POINTER(_vp), ctypes.c_int, c_int_p]),
    ("gp_group_destroy", ctypes.c_int, [_vp]),
    ("gp_group_info", ctypes.c_int, [_vp, c_int_p, c_int_p, ctypes.c_char_p, ctypes.c_int]),
    ("gp_group_member", ctypes.c_int, [_vp, ctypes.c_int, ctypes.POINTER(_vp)]),
    ("gp_group_set_data", ctypes.c_int, [_vp, c_double_p, c_double_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int]),
    ("gp_group_set_params", ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_double, c_double_p, ctypes.c_double]),
    ("gp_group_set_gower", ctypes.c_int, [_vp, ctypes.c_int, c_int_p, c_double_p]),
    ("gp_group_set_option", ctypes.c_int, [_vp, ctypes.c_char_p, ctypes.c_int64]),
    ("gp_group_fit", ctypes.c_int, [_vp, ctypes.c_int, c_double_p, c_double_p, c_double_p]),
    ("gp_group_fmin", ctypes.c_int, [_vp, c_double_p]),
    ("gp_group_set_candidates", ctypes.c_int, [_vp, c_double_p, ctypes.c_int64]),
    ("gp_group_acq_argbest", ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                            ctypes.c_double, ctypes.c_int, c_int64_p, c_double_p]),
    ("gp_group_acq_lp_argbest", ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                               ctypes.c_double, ctypes.c_int, c_double_p, ctypes.c_int, c_double_p, c_double_p,
                                               ctypes.c_int, c_int64_p, ctypes.c_int, c_int64_p, c_double_p]),
    ("gp_group_acq_topk", ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                         ctypes.c_double, ctypes.c_int, ctypes.c_int, c_int64_p, c_double_p]),
    ("gp_merge_best", ctypes.c_int, [ctypes.c_int, c_double_p, c_int64_p, ctypes.c_int, c_int64_p, c_double_p]),
    ("gp_merge_topk", ctypes.c_int, [ctypes.c_int, c_double_p, c_int64_p, ctypes.c_int, ctypes.c_int, c_int64_p, c_double_p]),
    ("gp_last_phases", ctypes.c_int, [_vp, ctypes.c_int, ctypes.POINTER(ctypes.c_char_p), c_double_p, c_double_p,
                                      c_double_p]),
    ("gp_profile", ctypes.c_int, [_vp, ctypes.c_int]),
    ("gp_gemm_stats", ctypes.c_int, [_vp, c_int64_p, c_double_p, c_double_p]),
    ("gp_rns_stats", ctypes.c_int, [_vp, c_int64_p, c_double_p, c_double_p]),
    ("gp_gemm_busy", ctypes.c_int, [_vp, c_double_p]),
    ("gp_gemm_trace", ctypes.c_int, [_vp, ctypes.c_int, c_int64_p, c_int_p, c_double_p]),
    ("gp_synchronize", ctypes.c_int, [_vp]),
    ("gp_debug_gemm", ctypes.c_int, [_vp, ctypes.c_int, c_double_p, c_double_p, c_double_p, ctypes.c_int64, ctypes.c_int,
                                     ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    ("gp_set_option", ctypes.c_int, [_vp, ctypes.c_char_p, ctypes.c_int64]),
    ("gp_cost_set", ctypes.c_int, [_vp, c_double_p, ctypes.c_int64, c_double_p, ctypes.c_int, ctypes.c_int, ctypes.c_double,
                                   c_double_p, ctypes.c_double, ctypes.c_double]),
    ("gp_cost_info", ctypes.c_int, [_vp, c_int64_p]),
    ("gp_cost_rows", ctypes.c_int, [_vp, _vp, ctypes.c_int64, _vp, _vp]),
    ("gp_feas_table", ctypes.c_int, [_vp, ctypes.POINTER(_vp), ctypes.c_int, c_double_p, c_double_p, c_double_p]),
    ("gp_feas_info", ctypes.c_int, [_vp, c_int_p, c_int64_p]),
    ("gp_feas_get_table", ctypes.c_int, [_vp, c_double_p]),
    ("gp_feas_rows", ctypes.c_int, [ctypes.POINTER(_vp), ctypes.c_int, c_double_p, c_double_p, c_double_p, _vp, ctypes.c_int64,
                                    _vp, _vp]),
    ("gp_acq_rows_feas", ctypes.c_int, [_vp, ctypes.POINTER(_vp), ctypes.c_int, c_double_p, c_double_p, c_double_p, _vp,
                                        ctypes.c_int64, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                        ctypes.c_double, _vp, _vp]),
    ("gp_fmin_rows", ctypes.c_int, [_vp, c_int64_p, ctypes.c_int64, c_double_p]),
    ("gp_mean_set", ctypes.c_int, [_vp, c_double_p, c_double_p]),
    ("gp_mean_info", ctypes.c_int, [_vp, c_int_p, c_int_p]),
    ("gp_mean_grad", ctypes.c_int, [_vp, c_double_p, c_double_p]),
    ("gp_mes_set", ctypes.c_int, [_vp, c_double_p, ctypes.c_int]),
    ("gp_mes_info", ctypes.c_int, [_vp, c_int_p]),
    ("gp_mes_logsurv", ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_double, ctypes.c_double, c_double_p, ctypes.c_int, c_double_p]),
    ("gp_mes_bracket", ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double, c_double_p, c_double_p]),
    ("gp_paths_set", ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, c_double_p, c_double_p, c_double_p, c_double_p]),
    ("gp_paths_info", ctypes.c_int, [_vp, c_int_p, c_int_p]),
    ("gp_paths_table", ctypes.c_int, [_vp, ctypes.c_double, ctypes.c_double, c_double_p]),
    ("gp_paths_argbest", ctypes.c_int, [_vp, ctypes.c_double, ctypes.c_double, ctypes.c_int, c_int64_p, c_double_p]),
    ("gp_paths_rows", ctypes.c_int, [_vp, _vp, ctypes.c_int, _vp, ctypes.c_double, ctypes.c_double, _vp, _vp]),
    ("gp_kg_set_points", ctypes.c_int, [_vp, c_double_p, ctypes.c_int, ctypes.c_double, ctypes.c_double, _vp]),
    ("gp_kg_info", ctypes.c_int, [_vp, c_int_p]),
    ("gp_kg_acq", ctypes.c_int, [_vp, ctypes.c_double, c_double_p]),
    ("gp_kg_acq_argbest", ctypes.c_int, [_vp, ctypes.c_double, ctypes.c_int, c_int64_p, c_double_p]),
    ("gp_kg_acq_topk", ctypes.c_int, [_vp, ctypes.c_double, ctypes.c_int, ctypes.c_int, c_int64_p, c_double_p]),
    ("gp_kg_rows", ctypes.c_int, [_vp, _vp, ctypes.c_int64, ctypes.c_double, _vp, _vp]),
    ("gp_nei_set", ctypes.c_int, [_vp, _vp, ctypes.c_int, _vp, _vp]),
    ("gp_nei_info", ctypes.c_int, [_vp, c_int_p, c_double_p, c_double_p]),
    ("gp_nei_get", ctypes.c_int, [_vp, _vp, _vp]),
    ("gp_nei_stats", ctypes.c_int, [_vp, c_int64_p, c_int_p, c_int_p]),
    ("gp_nei_table", ctypes.c_int, [_vp, ctypes.c_double, ctypes.c_double, ctypes.c_double, c_double_p]),
    ("gp_nei_argbest", ctypes.c_int, [_vp, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_int, c_int64_p, c_double_p]),
    ("gp_nei_topk", ctypes.c_int, [_vp, ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_int, c_int64_p,
                                   c_double_p]),
    ("gp_nei_rows", ctypes.c_int, [_vp, _vp, ctypes.c_int64, ctypes.c_double, ctypes.c_double, ctypes.c_double, _vp, _vp]),
    ("gp_laplace_fit", ctypes.c_int, [_vp, c_double_p, ctypes.c_int, c_double_p, c_double_p, c_int_p, c_int_p, c_int_p]),
    ("gp_laplace_fit_grad", ctypes.c_int, [_vp, c_double_p, ctypes.c_int, c_double_p, c_double_p, c_int_p, c_int_p, c_int_p,
                                           c_double_p]),
    ("gp_laplace_info", ctypes.c_int, [_vp, c_int_p, c_int_p, c_double_p, c_double_p]),
    ("gp_laplace_get_mode", ctypes.c_int, [_vp, c_double_p, c_double_p]),
    ("gp_qei_set", ctypes.c_int, [_vp, c_double_p, ctypes.c_int, ctypes.c_int]),
    ("gp_qei_info", ctypes.c_int, [_vp, c_int_p, c_int_p]),
    ("gp_qei_stats", ctypes.c_int, [_vp, c_int64_p, c_int64_p]),
    ("gp_qei_rows", ctypes.c_int, [_vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                   ctypes.c_double, _vp, _vp, _vp, _vp]),
    ("gp_ehvi_set", ctypes.c_int, [_vp, ctypes.c_int, c_double_p, c_int_p, c_int_p, c_int_p, ctypes.c_int]),
    ("gp_ehvi_info", ctypes.c_int, [_vp, c_int_p, c_int_p]),
    ("gp_ehvi_table", ctypes.c_int, [_vp, ctypes.POINTER(_vp), ctypes.c_int, c_double_p, c_double_p, _vp]),
    ("gp_ehvi_argbest", ctypes.c_int, [_vp, ctypes.POINTER(_vp), ctypes.c_int, c_double_p, c_double_p, ctypes.c_int, c_int64_p,
                                       ctypes.c_int, c_int64_p, c_double_p]),
    ("gp_ehvi_topk", ctypes.c_int, [_vp, ctypes.POINTER(_vp), ctypes.c_int, c_double_p, c_double_p, ctypes.c_int, ctypes.c_int,
                                    c_int64_p, c_double_p]),
    ("gp_ehvi_rows", ctypes.c_int, [_vp, ctypes.POINTER(_vp), ctypes.c_int, c_double_p, c_double_p, _vp, ctypes.c_int64, _vp, _vp]),
]

_lib = None


def load_library():
    """dlopen libgphip.so and bind every declared symbol (no GPU needed for this step)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "libgphip.so is missing at %s: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback." % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for name, restype, argtypes in SIGNATURES:
        fn = getattr(lib, name)  # AttributeError here means header and library disagree
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = lib
    return lib


def load():
    """Library handle, insisting on a visible GPU."""
    lib = load_library()
    n = ctypes.c_int(0)
    rc = lib.gp_device_count(ctypes.byref(n))
    if rc != 0 or n.value < 1:
        raise RuntimeError("gphip: no HIP device visible (%s). The GP path runs on MI355X only; "
                           "there is no CPU fallback." % lib.gp_last_error().decode())
    return lib


def dptr(a):
    return a.ctypes.data_as(c_double_p)


def as_f64(a, ndim=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if ndim is not None and a.ndim != ndim:
        raise ValueError("expected a %d-D array, got shape %s" % (ndim, a.shape))
    return a


def check(lib, rc, what):
    """Map C return codes to the exceptions the reference raises (linalg.py:62-75, bo.py:134-137)."""
    if rc == 0:
        return
    msg = lib.gp_last_error().decode()
    if rc > 0:
        raise np.linalg.LinAlgError("not positive definite, even with jitter.")
    if rc == GP_ERR_NOT_PD_DIAG:
        raise np.linalg.LinAlgError("not pd: non-positive diagonal elements")
    if rc == GP_ERR_ARG:
        raise ValueError("%s: %s" % (what, msg))
    raise RuntimeError("%s failed (%d): %s" % (what, rc, msg))


def _fit_scalars():
    """The (lml, logdet, jitter) out-parameters of the fit entry points."""
    return ctypes.c_double(), ctypes.c_double(), ctypes.c_double()


def _lp_pack(lp, ptr=dptr):
    """THE packer of the penaliser: ``lp`` = None or (transform, Xb, r_x0, s_x0) -> (on, transform, arrays kept alive, nb,
    pointers to Xb, r_x0, s_x0 as ``ptr`` makes them); no batch is nb = 0 and null pointers."""
    if lp is None:
        return 0, 0, None, 0, None, None, None
    if lp[1] is None:
        return 1, int(lp[0]), None, 0, None, None, None
    keep = (as_f64(np.atleast_2d(lp[1]), 2), as_f64(np.atleast_1d(lp[2]), 1), as_f64(np.atleast_1d(lp[3]), 1))
    return 1, int(lp[0]), keep, keep[0].shape[0], ptr(keep[0]), ptr(keep[1]), ptr(keep[2])


def _lp_args(Xb, r_x0, s_x0):
    """The batch alone, for the entries that take the transform by itself: (arrays kept alive, nb, pointers)."""
    return _lp_pack((0, Xb, r_x0, s_x0))[2:]


def _address(a):
    """An array's address as a plain integer, for the rows entries declared with ``void *``: a typed pointer costs ~4 us apiece."""
    return a.ctypes.data


def _acq_rows_entry(symbol, doc):
    """``Handle.acq_rows`` / ``Handle.sparse_acq_rows``: one body around the C symbol each names.  The L-BFGS inner loop lives here
    (~40 us a call, host-bound), so nothing is delegated: addresses instead of typed pointers, no helper for the common cases."""
    def rows(self, Xs, type_, par, fmin, y_mean=0.0, y_std=1.0, grad=False, lp=None):
        Xs = np.ascontiguousarray(Xs, dtype=np.float64)
        if Xs.ndim != 2:
            raise ValueError("expected a 2-D array, got shape %s" % (Xs.shape,))
        M = Xs.shape[0]
        dout = np.empty((M, self.D)) if grad else None
        if lp is None:
            out = np.empty((M, 1))
            on = tr = nb = 0
            pX = pr = ps = None
        else:
            out = np.empty(M)
            on, tr, keep, nb, pX, pr, ps = _lp_pack(lp, _address)
        rc = getattr(self.lib, symbol)(self.h, Xs.ctypes.data, M, int(type_), par, fmin, y_mean, y_std, on, tr, pX, nb, pr, ps,
                                       out.ctypes.data, dout.ctypes.data if grad else None)
        if rc:
            check(self.lib, rc, symbol)
        return (out, dout) if grad else out
    rows.__doc__ = doc
    return rows


class FeasPack(object):
    """The constraint side of a feasibility call, packed once per refit: K handles with their bounds and output normalisers as the
    C entries take them (``gp_feas_*``, ``gp_acq_rows_feas``).  Holds the Handle objects, so none is collected under a call."""

    def __init__(self, handles, bounds, c_mean, c_std):
        self.handles = list(handles)
        self.K = len(self.handles)
        if not 1 <= self.K <= GP_FEAS_MAX:
            raise ValueError("between 1 and %d constraints, got %d" % (GP_FEAS_MAX, self.K))
        self.bounds = as_f64(np.ravel(bounds), 1)
        self.c_mean = as_f64(np.ravel(c_mean), 1)
        self.c_std = as_f64(np.ravel(c_std), 1)
        if not (self.bounds.size == self.c_mean.size == self.c_std.size == self.K):
            raise ValueError("bounds, c_mean and c_std take one entry per constraint")
        self.D = self.handles[0].D
        self.lib = self.handles[0].lib
        self.cons = (_vp * self.K)(*[h.h for h in self.handles])
        self.args = (self.cons, self.K, dptr(self.bounds), dptr(self.c_mean), dptr(self.c_std))

    def rows(self, Xs, grad=False):
        """log prod_k Phi [M] at the rows of ``Xs`` and, with ``grad``, its x-gradient [M, D] (gp_feas_rows)."""
        Xs = as_f64(Xs, 2)
        if Xs.shape[1] != self.D:
            raise ValueError("locations have %d columns, the constraint models have %d" % (Xs.shape[1], self.D))
        M = Xs.shape[0]
        logF = np.empty(M)
        dlogF = np.empty((M, self.D)) if grad else None
        rc = self.lib.gp_feas_rows(*(self.args + (Xs.ctypes.data, M, logF.ctypes.data, dlogF.ctypes.data if grad else None)))
        if rc:
            check(self.lib, rc, "gp_feas_rows")
        return (logF, dlogF) if grad else logF


class EhviPack(object):
    """The objective side of an expected-hypervolume-improvement call (``gp_ehvi_*``): K = 2 or 3 handles, the first of which is
    scored and owns the cell decomposition, with their output normalisers.  Holds the Handle objects, so none is collected under a
    call."""

    def __init__(self, handles, y_mean, y_std):
        self.handles = list(handles)
        self.K = len(self.handles)
        if not 2 <= self.K <= GP_EHVI_MAX_OBJ:
            raise ValueError("between 2 and %d objectives, got %d" % (GP_EHVI_MAX_OBJ, self.K))
        self.y_mean = as_f64(np.ravel(y_mean), 1)
        self.y_std = as_f64(np.ravel(y_std), 1)
        if not (self.y_mean.size == self.y_std.size == self.K):
            raise ValueError("y_mean and y_std take one entry per objective")
        self.scored = self.handles[0]
        self.D = self.scored.D
        self.lib = self.scored.lib
        self.others = (_vp * (self.K - 1))(*[h.h for h in self.handles[1:]])
        self.args = (self.scored.h, self.others, self.K, dptr(self.y_mean), dptr(self.y_std))

    def set_cells(self, levels, cell_lo, cell_hi):
        """Make the decomposition resident on the scored handle (gp_ehvi_set): ``levels`` a list of K arrays (entry 0 of each
        stands for -inf), ``cell_lo`` / ``cell_hi`` [C, K] indices into them."""
        levels = [as_f64(np.ravel(l), 1) for l in levels]
        nlev = np.array([l.size for l in levels], dtype=np.intc)
        flat = as_f64(np.concatenate(levels), 1)
        lo = np.ascontiguousarray(np.atleast_2d(cell_lo), dtype=np.intc)
        hi = np.ascontiguousarray(np.atleast_2d(cell_hi), dtype=np.intc)
        if len(levels) != self.K or lo.shape != hi.shape or lo.ndim != 2 or lo.shape[1] != self.K:
            raise ValueError("expected %d level arrays and cells [C, %d], got %d and %s, %s"
                             % (self.K, self.K, len(levels), lo.shape, hi.shape))
        check(self.lib, self.lib.gp_ehvi_set(self.scored.h, self.K, dptr(flat), nlev.ctypes.data_as(c_int_p),
                                             lo.ctypes.data_as(c_int_p), hi.ctypes.data_as(c_int_p), lo.shape[0]), "gp_ehvi_set")

    def clear(self):
        check(self.lib, self.lib.gp_ehvi_set(self.scored.h, 0, None, None, None, None, 0), "gp_ehvi_set")

    def info(self):
        K, C = ctypes.c_int(0), ctypes.c_int(0)
        check(self.lib, self.lib.gp_ehvi_info(self.scored.h, ctypes.byref(K), ctypes.byref(C)), "gp_ehvi_info")
        return K.value, C.value

    def _tables_moved(self):
        for h in self.handles[1:]:   # their resident tables are the scored handle's now
            h.M = self.scored.M
            h.feas_key = None

    def table(self):
        """-EHVI [M, 1] over the scored handle's resident candidates (gp_ehvi_table)."""
        out = np.empty((self.scored.M, 1))
        check(self.lib, self.lib.gp_ehvi_table(*(self.args + (out.ctypes.data,))), "gp_ehvi_table")
        self._tables_moved()
        return out

    def argbest(self, sense, exclude=()):
        ex = np.asarray(list(exclude), dtype=np.int64)
        idx, val = ctypes.c_int64(), ctypes.c_double()
        check(self.lib, self.lib.gp_ehvi_argbest(*(self.args + (int(sense), ex.ctypes.data_as(c_int64_p), int(ex.size),
                                                                ctypes.byref(idx), ctypes.byref(val)))), "gp_ehvi_argbest")
        self._tables_moved()
        return idx.value, val.value

    def topk(self, sense, k):
        idx = np.empty(k, dtype=np.int64)
        val = np.empty(k)
        check(self.lib, self.lib.gp_ehvi_topk(*(self.args + (int(sense), int(k), idx.ctypes.data_as(c_int64_p), dptr(val)))),
              "gp_ehvi_topk")
        self._tables_moved()
        return idx, val

    def rows(self, Xs, grad=False):
        """-EHVI [M, 1] at the rows of ``Xs`` and, with ``grad``, its x-gradient [M, D]: every handle's fused pass, the fold and
        one drain in ONE call (gp_ehvi_rows)."""
        Xs = np.ascontiguousarray(Xs, dtype=np.float64)
        if Xs.ndim != 2 or Xs.shape[1] != self.D:
            raise ValueError("expected locations [M, %d], got shape %s" % (self.D, Xs.shape))
        M = Xs.shape[0]
        out = np.empty((M, 1))
        dout = np.empty((M, self.D)) if grad else None
        rc = self.lib.gp_ehvi_rows(*(self.args + (Xs.ctypes.data, M, out.ctypes.data, dout.ctypes.data if grad else None)))
        if rc:
            check(self.lib, rc, "gp_ehvi_rows")
        return (out, dout) if grad else out


class KgEntries(object):
    """The knowledge gradient's entries of a handle (include/gphip.h, gp_kg_*): discrete KG over resident discretisation points.
    ``handle.kg`` makes one; it holds nothing but the handle."""

    def __init__(self, handle):
        self.handle = handle

    def set_points(self, Xa, y_mean=0.0, y_std=1.0, key=None):
        """Make ``Xa`` [A, D] the resident discretisation points; returns their posterior means [A], un-normalised.  ``key`` is
        remembered as the handle's ``kg_key``."""
        h = self.handle
        Xa = as_f64(Xa, 2)
        if Xa.shape[1] != h.D:
            raise ValueError("expected points of shape [A, %d], got %s" % (h.D, Xa.shape))
        A = Xa.shape[0]
        mu = np.empty(max(A, 1))
        h.kg_key = None
        check(h.lib, h.lib.gp_kg_set_points(h.h, dptr(Xa), A, float(y_mean), float(y_std), mu.ctypes.data), "gp_kg_set_points")
        h.kg_key = key
        return mu[:A]

    def info(self):
        """How many discretisation points are resident (0: none, or a new fit dropped them)."""
        h = self.handle
        A = ctypes.c_int(0)
        check(h.lib, h.lib.gp_kg_info(h.h, ctypes.byref(A)), "gp_kg_info")
        return A.value

    def acq(self, y_std=1.0):
        """+KG of the resident candidates, [M, 1]."""
        h = self.handle
        out = np.empty((h.M, 1))
        check(h.lib, h.lib.gp_kg_acq(h.h, float(y_std), dptr(out)), "gp_kg_acq")
        return out

    def acq_argbest(self, sense, y_std=1.0):
        h = self.handle
        idx, val = ctypes.c_int64(), ctypes.c_double()
        check(h.lib, h.lib.gp_kg_acq_argbest(h.h, float(y_std), int(sense), ctypes.byref(idx), ctypes.byref(val)), "gp_kg_acq_argbest")
        return idx.value, val.value

    def acq_topk(self, sense, k, y_std=1.0):
        h = self.handle
        idx = np.empty(k, dtype=np.int64)
        val = np.empty(k)
        check(h.lib, h.lib.gp_kg_acq_topk(h.h, float(y_std), int(sense), int(k), idx.ctypes.data_as(c_int64_p), dptr(val)),
              "gp_kg_acq_topk")
        return idx, val

    def rows(self, Xs, y_std=1.0, grad=False):
        """-KG at the locations ``Xs`` [M, D] given by value, [M, 1]; with ``grad`` its gradient [M, D] as well (up to eight
        locations: the fused rows path)."""
        h = self.handle
        Xs = np.ascontiguousarray(Xs, dtype=np.float64)
        if Xs.ndim != 2 or Xs.shape[1] != h.D:
            raise ValueError("expected locations of shape [M, %d], got %s" % (h.D, Xs.shape))
        out = np.empty((Xs.shape[0], 1))
        dout = np.empty((Xs.shape[0], h.D)) if grad else None
        rc = h.lib.gp_kg_rows(h.h, Xs.ctypes.data, Xs.shape[0], float(y_std), out.ctypes.data, dout.ctypes.data if grad else None)
        if rc:
            check(h.lib, rc, "gp_kg_rows")
        return (out, dout) if grad else out


class NeiEntries(object):
    """Noisy expected improvement's entries of a handle (include/gphip.h, gp_nei_*).  The handle is the TWIN: a near-noiseless fit
    of the model's kernel over the model's inputs, on which the fantasies become resident.  ``handle.nei`` makes one; it holds
    nothing but the handle."""

    def __init__(self, handle):
        self.handle = handle

    def set(self, model, Z, E):
        """Draw S fantasies of the noiseless training values from the standard normals ``Z``, ``E`` [S, N] through the factor of
        ``model`` (a fitted Handle over the same inputs and kernel) and this handle's.  Nothing is factored."""
        h = self.handle
        Z = as_f64(Z, 2)
        E = as_f64(E, 2)
        if Z.shape != E.shape or Z.shape[1] != h.N:
            raise ValueError("expected Z and E of one shape [S, %d], got %s and %s" % (h.N, Z.shape, E.shape))
        check(h.lib, h.lib.gp_nei_set(h.h, model.h, Z.shape[0], Z.ctypes.data, E.ctypes.data), "gp_nei_set")

    def clear(self):
        h = self.handle
        check(h.lib, h.lib.gp_nei_set(h.h, None, 0, None, None), "gp_nei_set")

    def info(self):
        """(S, d_model, d_twin): the fantasies resident (0: none, or a new fit dropped them) and the two factors' diagonals."""
        h = self.handle
        S, d, d0 = ctypes.c_int(0), ctypes.c_double(0.0), ctypes.c_double(0.0)
        check(h.lib, h.lib.gp_nei_info(h.h, ctypes.byref(S), ctypes.byref(d), ctypes.byref(d0)), "gp_nei_info")
        return S.value, d.value, d0.value

    def get(self):
        """(F [S, N], fstar [S]): the fantasies and their minima, normalised."""
        h = self.handle
        S = self.info()[0]
        F = np.empty((max(S, 1), h.N))
        fstar = np.empty(max(S, 1))
        check(h.lib, h.lib.gp_nei_get(h.h, F.ctypes.data, fstar.ctypes.data), "gp_nei_get")
        return F[:S], fstar[:S]

    def stats(self):
        """Route checks: how often the handle's inverse factor was built, and of the last pass of the last ``rows`` call the kernels
        launched and how many of them read the inverse factor (0, 0: the table route)."""
        h = self.handle
        b, n, r = ctypes.c_int64(0), ctypes.c_int(0), ctypes.c_int(0)
        check(h.lib, h.lib.gp_nei_stats(h.h, ctypes.byref(b), ctypes.byref(n), ctypes.byref(r)), "gp_nei_stats")
        return dict(linv_builds=b.value, launches=n.value, reads=r.value)

    def table(self, par=0.0, y_mean=0.0, y_std=1.0):
        """+NEI of the resident candidates, [M, 1]."""
        h = self.handle
        out = np.empty((h.M, 1))
        check(h.lib, h.lib.gp_nei_table(h.h, float(par), float(y_mean), float(y_std), dptr(out)), "gp_nei_table")
        return out

    def argbest(self, sense, par=0.0, y_mean=0.0, y_std=1.0):
        h = self.handle
        idx, val = ctypes.c_int64(), ctypes.c_double()
        check(h.lib, h.lib.gp_nei_argbest(h.h, float(par), float(y_mean), float(y_std), int(sense), ctypes.byref(idx), ctypes.byref(val)),
              "gp_nei_argbest")
        return idx.value, val.value

    def topk(self, sense, k, par=0.0, y_mean=0.0, y_std=1.0):
        h = self.handle
        idx = np.empty(k, dtype=np.int64)
        val = np.empty(k)
        check(h.lib, h.lib.gp_nei_topk(h.h, float(par), float(y_mean), float(y_std), int(sense), int(k), idx.ctypes.data_as(c_int64_p),
                                       dptr(val)), "gp_nei_topk")
        return idx, val

    def rows(self, Xs, par=0.0, y_mean=0.0, y_std=1.0, grad=False):
        """-NEI at the locations ``Xs`` [M, D] given by value, [M, 1]; with ``grad`` its gradient [M, D] as well (up to eight
        locations: the fused rows path)."""
        h = self.handle
        Xs = np.ascontiguousarray(Xs, dtype=np.float64)
        if Xs.ndim != 2 or Xs.shape[1] != h.D:
            raise ValueError("expected locations of shape [M, %d], got %s" % (h.D, Xs.shape))
        out = np.empty((Xs.shape[0], 1))
        dout = np.empty((Xs.shape[0], h.D)) if grad else None
        rc = h.lib.gp_nei_rows(h.h, Xs.ctypes.data, Xs.shape[0], float(par), float(y_mean), float(y_std), out.ctypes.data,
                               dout.ctypes.data if grad else None)
        if rc:
            check(h.lib, rc, "gp_nei_rows")
        return (out, dout) if grad else out


class Handle(object):
    """Owns one gp_t (one device)."""

    def __init__(self, device=0):
        self.lib = load()
        h = _vp()
        check(self.lib, self.lib.gp_create(ctypes.byref(h), int(device)), "gp_create")
        self.h = h
        self.device = int(device)
        self.sparse_M = 0      # rows of the sparse model's candidate table (sparse_set_candidates); 0: the library refuses to score
        self.sparse_R = 0      # rows of the sparse model's second point set (sparse_cov_set_points); 0: sparse_cov_between is refused
        self.cost_key = None   # whose cost surface the handle holds: set by the caller of cost_set, dropped with the surface
        self.mes_key = None    # whose samples of the minimum's value the handle holds: set by the caller of mes_set
        self.feas_key = None   # whose probability of feasibility the handle caches over its candidates: set by the caller of feas_table
        self.paths_key = None  # whose posterior paths the handle holds: set by the caller of paths_set

    def close(self):
        if getattr(self, "h", None):
            self.lib.gp_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- thin typed wrappers -------------------------------------------------
    def set_data(self, X, Y):
        X = as_f64(X, 2)
        Y = as_f64(Y, 2)
        if X.shape[0] != Y.shape[0]:
            raise ValueError("X and Y row counts differ")
        check(self.lib, self.lib.gp_set_data(self.h, dptr(X), dptr(Y), X.shape[0], X.shape[1], Y.shape[1]),
              "gp_set_data")
        if getattr(self, "D", X.shape[1]) != X.shape[1]:
            self.cost_key = None       # the library drops a cost surface of another width
            self.feas_key = None       # ... and a probability of feasibility cached over candidates of another width
        self.N, self.D, self.P = X.shape[0], X.shape[1], Y.shape[1]

    def set_params(self, kernel, ard, variance, lengthscale, noise):
        ls = as_f64(np.atleast_1d(lengthscale), 1)
        if ls.size != (self.D if ard else 1):
            raise ValueError("lengthscale has %d entries, expected %d" % (ls.size, self.D if ard else 1))
        check(self.lib, self.lib.gp_set_params(self.h, int(kernel), int(bool(ard)), float(variance), dptr(ls),
                                               float(noise)), "gp_set_params")
        self.n_ls = ls.size

    def append(self, Xnew, Yall):
        """gp_append: ``Xnew`` [k, D] joins the data of the valid fit, ``Yall`` [N + k, P] replaces all targets; the factor grows by
        k rows instead of being rebuilt.  Returns (lml, logdet).  A border that is not positive definite raises
        ``numpy.linalg.LinAlgError`` and leaves the handle as it was: the caller refits (``set_data`` + ``fit``)."""
        Xnew = as_f64(Xnew, 2)
        Yall = as_f64(Yall, 2)
        N = getattr(self, "N", None)
        if N is None:
            raise ValueError("append extends a fit: set_data, set_params and fit come first")
        if Xnew.shape[1] != self.D:
            raise ValueError("Xnew has %d columns, the model %d" % (Xnew.shape[1], self.D))
        if Yall.shape != (N + Xnew.shape[0], self.P):
            raise ValueError("Yall must hold ALL targets, shape %s; got %s" % ((N + Xnew.shape[0], self.P), Yall.shape))
        lml, logdet = ctypes.c_double(), ctypes.c_double()
        rc = self.lib.gp_append(self.h, dptr(Xnew), Xnew.shape[0], dptr(Yall), ctypes.byref(lml), ctypes.byref(logdet))
        if rc > 0:
            raise np.linalg.LinAlgError("gp_append: the border is not positive definite (row %d of the grown matrix)" % rc)
        check(self.lib, rc, "gp_append")
        self.N = N + Xnew.shape[0]
        return lml.value, logdet.value

    def append_stats(self):
        """(borders written inside the last tile, borders that opened a new tile, calls refused) since the handle was created."""
        a, b, c = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        check(self.lib, self.lib.gp_append_stats(self.h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)), "gp_append_stats")
        return a.value, b.value, c.value

    def _grad_ls(self, nls):
        """The lengthscale-gradient buffer for gp_lml_grad / gp_fit_grad: the library writes one entry per lengthscale of the
        LAST gp_set_params (1, or D with ard) whatever the caller expects, so a wrong count is refused here."""
        want = getattr(self, "n_ls", None)
        if want is None:
            raise ValueError("set_params has not been called on this handle")
        if int(nls) != want:
            raise ValueError("the model has %d lengthscale(s), the caller asked for %d gradient entries" % (want, int(nls)))
        return np.empty(want)

    def set_gower(self, is_discrete=None, ranges=None):
        """Enable (or, with no arguments, disable) the fork's Gower product kernel."""
        if is_discrete is None:
            check(self.lib, self.lib.gp_set_gower(self.h, 0, None, None), "gp_set_gower")
            return
        disc = np.ascontiguousarray(is_discrete, dtype=np.int32)
        rng = as_f64(ranges, 1)
        if disc.size != self.D or rng.size != self.D:
            raise ValueError("is_discrete / ranges need one entry per input dimension")
        check(self.lib, self.lib.gp_set_gower(self.h, 1, disc.ctypes.data_as(c_int_p), dptr(rng)), "gp_set_gower")

    def fit(self, maxtries=5):
        lml, logdet, jit = _fit_scalars()
        rc = self.lib.gp_fit(self.h, int(maxtries), ctypes.byref(lml), ctypes.byref(logdet), ctypes.byref(jit))
        check(self.lib, rc, "gp_fit")
        return lml.value, logdet.value, jit.value

    # -- GP classification (gp_laplace_*) ----------------------------------------
    def _laplace_labels(self, y):
        y = as_f64(np.ravel(y), 1)
        if y.size != getattr(self, "N", -1):
            raise ValueError("one label per training row: got %d, the data has %s" % (y.size, getattr(self, "N", None)))
        return y

    def _laplace_check(self, rc, what):
        if rc == GP_LAPLACE_NOT_CONVERGED:
            raise RuntimeError("%s: %s" % (what, self.lib.gp_last_error().decode()))
        if rc > 0:
            raise np.linalg.LinAlgError("%s: B = I + W^1/2 K W^1/2 is not positive definite (pivot %d)" % (what, rc))
        check(self.lib, rc, what)

    def laplace_fit(self, y, cap=LAPLACE_MAX_ITER):
        """gp_laplace_fit: the probit Laplace fit of the labels ``y`` [N] in {-1, +1} under the handle's data and kernel, at most
        ``cap`` Newton steps.  Returns
        (log Z, log|B|, Newton steps, halvings); the handle is then Laplace-fitted (the latent posterior through ``predict*``).
        Raises RuntimeError when ``cap`` steps did not converge, numpy.linalg.LinAlgError on a failed pivot."""
        y = self._laplace_labels(y)
        lz, ld = ctypes.c_double(), ctypes.c_double()
        it, hv, cv = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        rc = self.lib.gp_laplace_fit(self.h, dptr(y), int(cap), ctypes.byref(lz), ctypes.byref(ld), ctypes.byref(it),
                                     ctypes.byref(hv), ctypes.byref(cv))
        self._laplace_check(rc, "gp_laplace_fit")
        return lz.value, ld.value, it.value, hv.value

    def laplace_fit_grad(self, y, nls, cap=LAPLACE_MAX_ITER):
        """gp_laplace_fit_grad: the fit and d log Z / d (variance, lengthscale(s)).  Returns ((log Z, log|B|, steps, halvings),
        (dvariance, dlengthscale [nls]))."""
        y = self._laplace_labels(y)
        grad = np.empty(1 + self._grad_ls(nls).size)
        lz, ld = ctypes.c_double(), ctypes.c_double()
        it, hv, cv = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        rc = self.lib.gp_laplace_fit_grad(self.h, dptr(y), int(cap), ctypes.byref(lz), ctypes.byref(ld), ctypes.byref(it),
                                          ctypes.byref(hv), ctypes.byref(cv), dptr(grad))
        self._laplace_check(rc, "gp_laplace_fit_grad")
        return (lz.value, ld.value, it.value, hv.value), (grad[0], grad[1:].copy())

    def laplace_info(self):
        """(Newton steps, halvings, min W, max W) of the last Laplace fit (gp_laplace_info)."""
        it, hv = ctypes.c_int(), ctypes.c_int()
        lo, hi = ctypes.c_double(), ctypes.c_double()
        check(self.lib, self.lib.gp_laplace_info(self.h, ctypes.byref(it), ctypes.byref(hv), ctypes.byref(lo), ctypes.byref(hi)),
              "gp_laplace_info")
        return it.value, hv.value, lo.value, hi.value

    def laplace_mode(self):
        """(f [N] at the mode, W [N]) of the Laplace-fitted handle (gp_laplace_get_mode)."""
        f, W = np.empty(self.N), np.empty(self.N)
        check(self.lib, self.lib.gp_laplace_get_mode(self.h, dptr(f), dptr(W)), "gp_laplace_get_mode")
        return f, W

    def fit_predict(self, include_noise=True, maxtries=5):
        """gp_fit + gp_predict on the resident candidates as one pipelined pass."""
        lml, logdet, jit = _fit_scalars()
        mean = np.empty((self.M, self.P))
        var = np.empty((self.M, 1))
        rc = self.lib.gp_fit_predict(self.h, int(maxtries), int(bool(include_noise)), ctypes.byref(lml),
                                     ctypes.byref(logdet), ctypes.byref(jit), dptr(mean), dptr(var))
        check(self.lib, rc, "gp_fit_predict")
        return (lml.value, logdet.value, jit.value), mean, var

    def fit_grad(self, nls, maxtries=5):
        """gp_fit + gp_lml_grad as one call: ((lml, logdet, jitter), (dvariance, dlengthscale[nls], dnoise))."""
        lml, logdet, jit = _fit_scalars()
        dv, dn = ctypes.c_double(), ctypes.c_double()
        dl = self._grad_ls(nls)
        rc = self.lib.gp_fit_grad(self.h, int(maxtries), ctypes.byref(lml), ctypes.byref(logdet), ctypes.byref(jit),
                                  ctypes.byref(dv), dptr(dl), ctypes.byref(dn))
        check(self.lib, rc, "gp_fit_grad")
        return (lml.value, logdet.value, jit.value), (dv.value, dl, dn.value)

    def lml_grad_lds(self):
        """(bytes of LDS a workgroup of the gradient pass needs for this data and Gower setting, bytes the device gives one): the
        gradient entries raise ValueError while the first exceeds the second."""
        need, avail = ctypes.c_int64(), ctypes.c_int64()
        check(self.lib, self.lib.gp_lml_grad_lds(self.h, ctypes.byref(need), ctypes.byref(avail)), "gp_lml_grad_lds")
        return need.value, avail.value

    def lml_grad_x(self):
        """dL/dX [N, D] of the training inputs at the current fit (gp_lml_grad_x)."""
        out = np.empty((self.N, self.D))
        check(self.lib, self.lib.gp_lml_grad_x(self.h, dptr(out)), "gp_lml_grad_x")
        return out

    def fit_grad_x(self, nls, maxtries=5):
        """gp_fit_grad + gp_lml_grad_x as one call: ((lml, logdet, jitter), (dvariance, dlengthscale[nls], dnoise), dL_dX [N, D])."""
        lml, logdet, jit = _fit_scalars()
        dv, dn = ctypes.c_double(), ctypes.c_double()
        dl = self._grad_ls(nls)
        dX = np.empty((self.N, self.D))
        rc = self.lib.gp_fit_grad_x(self.h, int(maxtries), ctypes.byref(lml), ctypes.byref(logdet), ctypes.byref(jit),
                                    ctypes.byref(dv), dptr(dl), ctypes.byref(dn), dptr(dX))
        check(self.lib, rc, "gp_fit_grad_x")
        return (lml.value, logdet.value, jit.value), (dv.value, dl, dn.value), dX

    def fit_grad_batch(self, variances, lengthscales, noises, maxtries=5):
        """gp_fit_grad for R parameter vectors in one call (the resident fit is untouched).  ``lengthscales`` is [R, nls] with nls
        the last set_params' lengthscale count.  Returns ((lml, logdet, jitter) [R] each, (dvariance [R], dlengthscale [R, nls],
        dnoise [R]), status [R]); status[r] != 0 is what gp_fit_grad returns for member r, whose numbers are then NaN."""
        var = as_f64(np.atleast_1d(variances), 1)
        noi = as_f64(np.atleast_1d(noises), 1)
        R = var.size
        want = getattr(self, "n_ls", None)
        if want is None:
            raise ValueError("set_params has not been called on this handle")
        ls = np.asarray(lengthscales, dtype=float)
        if ls.ndim != 2 or ls.shape != (R, want):
            raise ValueError("lengthscales has shape %s, expected (%d, %d): one row per member, one entry per lengthscale of "
                             "the model" % (ls.shape, R, want))
        if noi.size != R:
            raise ValueError("variances and noises differ in length (%d, %d)" % (R, noi.size))
        ls = np.ascontiguousarray(ls)
        lml, logdet, jit = np.empty(R), np.empty(R), np.empty(R)
        dv, dl, dn = np.empty(R), np.empty((R, want)), np.empty(R)
        status = np.zeros(R, dtype=np.int32)
        rc = self.lib.gp_fit_grad_batch(self.h, int(R), dptr(var), dptr(ls), dptr(noi), int(maxtries), dptr(lml), dptr(logdet),
                                        dptr(jit), dptr(dv), dptr(dl), dptr(dn), status.ctypes.data_as(c_int_p))
        check(self.lib, rc, "gp_fit_grad_batch")
        return (lml, logdet, jit), (dv, dl, dn), status

    def _batch_params(self, variances, lengthscales, noises):
        """(R, variance [R], lengthscale [R, nls], noise [R]) of a batch call, checked against the last set_params."""
        var = as_f64(np.atleast_1d(variances), 1)
        noi = as_f64(np.atleast_1d(noises), 1)
        R = var.size
        want = getattr(self, "n_ls", None)
        if want is None:
            raise ValueError("set_params has not been called on this handle")
        ls = np.asarray(lengthscales, dtype=float)
        if ls.ndim != 2 or ls.shape != (R, want):
            raise ValueError("lengthscales has shape %s, expected (%d, %d): one row per member, one entry per lengthscale of "
                             "the model" % (ls.shape, R, want))
        if noi.size != R:
            raise ValueError("variances and noises differ in length (%d, %d)" % (R, noi.size))
        return R, var, np.ascontiguousarray(ls), noi

    def fit_grad_x_batch(self, Xw, variances, lengthscales, noises, maxtries=5):
        """gp_fit_grad_x for R members in one call, member r over the inputs ``Xw[r]`` ([R, N, D], already warped) and the
        resident targets; the resident fit and data are untouched.  Returns ((lml, logdet, jitter) [R] each, (dvariance [R],
        dlengthscale [R, nls], dnoise [R]), dL_dX [R, N, D], status [R]); a member with status[r] != 0 has NaN outputs."""
        R, var, ls, noi = self._batch_params(variances, lengthscales, noises)
        Xw = as_f64(Xw, 3)
        if Xw.shape != (R, self.N, self.D):
            raise ValueError("Xw has shape %s, expected (%d, %d, %d): the training inputs of every member"
                             % (Xw.shape, R, self.N, self.D))
        lml, logdet, jit = np.empty(R), np.empty(R), np.empty(R)
        dv, dl, dn = np.empty(R), np.empty((R, ls.shape[1])), np.empty(R)
        dX = np.empty((R, self.N, self.D))
        status = np.zeros(R, dtype=np.int32)
        rc = self.lib.gp_fit_grad_x_batch(self.h, int(R), dptr(Xw), dptr(var), dptr(ls), dptr(noi), int(maxtries), dptr(lml),
                                          dptr(logdet), dptr(jit), dptr(dv), dptr(dl), dptr(dn), dptr(dX),
                                          status.ctypes.data_as(c_int_p))
        check(self.lib, rc, "gp_fit_grad_x_batch")
        return (lml, logdet, jit), (dv, dl, dn), dX, status

    def fit_grad_warp_batch(self, psis, ds, variances, lengthscales, noises, maxtries=5):
        """gp_fit_grad_warp for R members in one call, member r with the tanh warp (``psis[r]`` [n_terms, 3], ``ds[r]``) of the
        resident RAW targets; the resident fit, targets and warp are untouched.  Returns ((lml, logdet, jitter) [R] each,
        (dvariance [R], dlengthscale [R, nls], dnoise [R]), log_jacobian [R], (dpsi [R, n_terms, 3], dd [R]), status [R]); a
        member with status[r] != 0 has NaN outputs."""
        R, var, ls, noi = self._batch_params(variances, lengthscales, noises)
        psis = as_f64(psis, 3)
        ds = as_f64(np.atleast_1d(ds), 1)
        if psis.shape[0] != R or psis.shape[2] != 3 or ds.size != R:
            raise ValueError("psis needs shape (%d, n_terms, 3) and ds %d entries, got %s and %d" % (R, R, psis.shape, ds.size))
        lml, logdet, jit = np.empty(R), np.empty(R), np.empty(R)
        dv, dl, dn = np.empty(R), np.empty((R, ls.shape[1])), np.empty(R)
        lj, dpsi, dd = np.empty(R), np.empty_like(psis), np.empty(R)
        status = np.zeros(R, dtype=np.int32)
        rc = self.lib.gp_fit_grad_warp_batch(self.h, int(R), int(psis.shape[1]), dptr(psis), dptr(ds), dptr(var), dptr(ls),
                                             dptr(noi), int(maxtries), dptr(lml), dptr(logdet), dptr(jit), dptr(dv), dptr(dl),
                                             dptr(dn), dptr(lj), dptr(dpsi), dptr(dd), status.ctypes.data_as(c_int_p))
        check(self.lib, rc, "gp_fit_grad_warp_batch")
        return (lml, logdet, jit), (dv, dl, dn), lj, (dpsi, dd), status

    def fit_state(self):
        lml, logdet, jit = _fit_scalars()
        check(self.lib, self.lib.gp_get_fit_state(self.h, ctypes.byref(lml), ctypes.byref(logdet), ctypes.byref(jit)),
              "gp_get_fit_state")
        return lml.value, logdet.value, jit.value

    def dL_dK(self):
        out = np.empty((self.N, self.N))
        check(self.lib, self.lib.gp_get_dl_dk(self.h, dptr(out)), "gp_get_dl_dk")
        return out

    def posterior_samples(self, Z, include_noise=False, maxtries=5):
        """Z[S, M] standard normals -> (mean[M, P], dev[S, M], jitter): draw s of output d = mean[:, d] + dev[s]."""
        Z = as_f64(Z, 2)
        if Z.shape[1] != self.M:
            raise ValueError("Z needs one column per resident candidate")
        mean = np.empty((self.M, self.P))
        dev = np.empty((Z.shape[0], self.M))
        jit = ctypes.c_double()
        rc = self.lib.gp_posterior_samples(self.h, int(bool(include_noise)), dptr(Z), Z.shape[0], int(maxtries),
                                           dptr(mean), dptr(dev), ctypes.byref(jit))
        check(self.lib, rc, "gp_posterior_samples")
        return mean, dev, jit.value

    def acq_topk(self, type_, par, fmin, sense, k, y_mean=0.0, y_std=1.0):
        idx = np.empty(k, dtype=np.int64)
        val = np.empty(k)
        check(self.lib, self.lib.gp_acq_topk(self.h, int(type_), float(par), float(fmin), float(y_mean), float(y_std),
                                             int(sense), int(k), idx.ctypes.data_as(c_int64_p), dptr(val)),
              "gp_acq_topk")
        return idx, val

    def alpha(self):
        out = np.empty((self.N, self.P))
        check(self.lib, self.lib.gp_get_alpha(self.h, dptr(out)), "gp_get_alpha")
        return out

    def chol(self):
        out = np.empty((self.N, self.N))
        check(self.lib, self.lib.gp_get_chol(self.h, dptr(out)), "gp_get_chol")
        return out

    def woodbury_inv(self):
        out = np.empty((self.N, self.N))
        check(self.lib, self.lib.gp_get_woodbury_inv(self.h, dptr(out)), "gp_get_woodbury_inv")
        return out

    def kernel_matrix(self):
        out = np.empty((self.N, self.N))
        check(self.lib, self.lib.gp_kernel_matrix(self.h, dptr(out)), "gp_kernel_matrix")
        return out

    def cross_kernel_matrix(self, X2):
        """kern.K(X, X2): [N, M2] (stationary.py:107-140 with X2 given)."""
        X2 = as_f64(X2, 2)
        if X2.shape[1] != self.D:
            raise ValueError("X2 has %d columns, model has %d" % (X2.shape[1], self.D))
        out = np.empty((self.N, X2.shape[0]))
        check(self.lib, self.lib.gp_cross_kernel_matrix(self.h, dptr(X2), X2.shape[0], dptr(out)),
              "gp_cross_kernel_matrix")
        return out

    def lml_grad(self, nls):
        dv, dn = ctypes.c_double(), ctypes.c_double()
        dl = self._grad_ls(nls)
        check(self.lib, self.lib.gp_lml_grad(self.h, ctypes.byref(dv), dptr(dl), ctypes.byref(dn)), "gp_lml_grad")
        return dv.value, dl, dn.value

    def set_candidates(self, Xs):
        Xs = as_f64(Xs, 2)
        if Xs.shape[1] != self.D:
            raise ValueError("candidates have %d columns, model has %d" % (Xs.shape[1], self.D))
        check(self.lib, self.lib.gp_set_candidates(self.h, dptr(Xs), Xs.shape[0]), "gp_set_candidates")
        self.M = Xs.shape[0]
        self.feas_key = None   # the library drops the probability of feasibility cached over the old table

    def set_candidates_kumar(self, Xs, warp, a, b, xmin, xmax, want_warped=False):
        """gp_set_candidates of the Kumaraswamy-warped table, warped on the device: ``warp`` [D] 0 / 1, ``a``, ``b``, ``xmin``,
        ``xmax`` [D] (read where ``warp`` is set; the bounds already widened by epsilon).  Returns the warped table with
        ``want_warped``."""
        Xs = as_f64(Xs, 2)
        if Xs.shape[1] != self.D:
            raise ValueError("candidates have %d columns, model has %d" % (Xs.shape[1], self.D))
        warp = np.ascontiguousarray(warp, dtype=np.int32).reshape(-1)
        vecs = [as_f64(np.atleast_1d(v), 1) for v in (a, b, xmin, xmax)]
        if warp.size != self.D or any(v.size != self.D for v in vecs):
            raise ValueError("warp, a, b, xmin and xmax need one entry per input dimension")
        out = np.empty_like(Xs) if want_warped else None
        rc = self.lib.gp_set_candidates_kumar(self.h, dptr(Xs), Xs.shape[0], warp.ctypes.data_as(c_int_p), dptr(vecs[0]),
                                              dptr(vecs[1]), dptr(vecs[2]), dptr(vecs[3]), dptr(out) if want_warped else None)
        check(self.lib, rc, "gp_set_candidates_kumar")
        self.M = Xs.shape[0]
        return out

    # -- output warp (include/gphip.h, "output-warped GP") --------------------------
    @staticmethod
    def _psi(psi):
        psi = as_f64(np.atleast_2d(psi), 2)
        if psi.shape[1] != 3:
            raise ValueError("psi needs one (a, b, c) row per term, got shape %s" % (psi.shape,))
        return psi

    def set_output_warp(self, psi=None, d=1.0):
        """Warp the resident targets with f(y) = d y + sum a tanh(b (y + c)), ``psi`` [n_terms, 3]; returns sum log f'(y).
        ``psi`` None (or empty) switches the warp off."""
        lj = ctypes.c_double()
        if psi is None or np.size(psi) == 0:
            check(self.lib, self.lib.gp_set_output_warp(self.h, 0, None, 1.0, ctypes.byref(lj)), "gp_set_output_warp")
            return 0.0
        psi = self._psi(psi)
        check(self.lib, self.lib.gp_set_output_warp(self.h, psi.shape[0], dptr(psi), float(d), ctypes.byref(lj)),
              "gp_set_output_warp")
        return lj.value

    def targets(self):
        """The resident targets [N, P] as the fit sees them (f of the raw ones under a warp)."""
        out = np.empty((self.N, self.P))
        check(self.lib, self.lib.gp_get_targets(self.h, dptr(out)), "gp_get_targets")
        return out

    def warp_grad(self, n_terms):
        """(dpsi [n_terms, 3], dd): natural gradients of LML + log-Jacobian at the current fit."""
        dpsi, dd = np.empty((int(n_terms), 3)), ctypes.c_double()
        check(self.lib, self.lib.gp_warp_grad(self.h, dptr(dpsi), ctypes.byref(dd)), "gp_warp_grad")
        return dpsi, dd.value

    def fit_grad_warp(self, psi, d, nls, maxtries=5):
        """set_output_warp + fit_grad + warp_grad as one call: ((lml, logdet, jitter), (dvariance, dlengthscale[nls], dnoise),
        log_jacobian, (dpsi [n_terms, 3], dd))."""
        psi = self._psi(psi)
        lml, logdet, jit = _fit_scalars()
        dv, dn, lj, dd = ctypes.c_double(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        dl = self._grad_ls(nls)
        dpsi = np.empty_like(psi)
        rc = self.lib.gp_fit_grad_warp(self.h, psi.shape[0], dptr(psi), float(d), int(maxtries), ctypes.byref(lml),
                                       ctypes.byref(logdet), ctypes.byref(jit), ctypes.byref(dv), dptr(dl), ctypes.byref(dn),
                                       ctypes.byref(lj), dptr(dpsi), ctypes.byref(dd))
        check(self.lib, rc, "gp_fit_grad_warp")
        return (lml.value, logdet.value, jit.value), (dv.value, dl, dn.value), lj.value, (dpsi, dd.value)

    @staticmethod
    def _gauss_hermite(deg):
        t, w = np.polynomial.hermite.hermgauss(int(deg))
        return as_f64(t, 1), as_f64(w, 1)

    def _moments(self, call, M, deg, median, partials):
        t, w = self._gauss_hermite(deg)
        mean, var = np.empty((M, 1)), np.empty((M, 1))
        med = np.empty((M, 1)) if median else None
        part = np.empty((M, 4)) if partials else None
        call(t.size, dptr(t), dptr(w), 1 if median else 0, dptr(mean), dptr(var), dptr(med) if median else None,
             dptr(part) if partials else None)
        return mean, var, med, part

    def predict_warped(self, include_noise=True, y_mean=0.0, y_std=1.0, deg=20, median=False, partials=False):
        """Warped (mean [M, 1], var [M, 1], median [M, 1] or None, partials [M, 4] or None) of the resident candidates."""
        def call(n, t, w, wm, mean, var, med, part):
            check(self.lib, self.lib.gp_predict_warped(self.h, int(bool(include_noise)), float(y_mean), float(y_std), n, t, w,
                                                       wm, mean, var, med, part), "gp_predict_warped")
        return self._moments(call, self.M, deg, median, partials)

    def warp_moments(self, mean, var, y_mean=0.0, y_std=1.0, deg=20, median=False, partials=False):
        """The same for a latent posterior given by value (``mean``, ``var`` of M entries each)."""
        mi, vi = as_f64(np.ravel(mean), 1), as_f64(np.ravel(var), 1)
        if mi.size != vi.size or mi.size < 1:
            raise ValueError("mean and var need the same, positive number of entries")

        def call(n, t, w, wm, mo, vo, med, part):
            check(self.lib, self.lib.gp_warp_moments(self.h, dptr(mi), dptr(vi), mi.size, float(y_mean), float(y_std), n, t, w,
                                                     wm, mo, vo, med, part), "gp_warp_moments")
        return self._moments(call, mi.size, deg, median, partials)

    def warp_inverse(self, z):
        """f^-1 of every entry of ``z`` with the warp in force, in the shape of ``z``."""
        z = as_f64(z)
        out = np.empty_like(z)
        if z.size:
            check(self.lib, self.lib.gp_warp_inverse(self.h, dptr(z.reshape(-1)), z.size, dptr(out.reshape(-1))), "gp_warp_inverse")
        return out

    # -- sparse GP (include/gphip.h, "sparse GP") --------------------------------------
    def sparse_set_inducing(self, Z):
        Z = as_f64(Z, 2)
        if Z.shape[1] != self.D:
            raise ValueError("inducing inputs have %d columns, model has %d" % (Z.shape[1], self.D))
        check(self.lib, self.lib.gp_sparse_set_inducing(self.h, dptr(Z), Z.shape[0]), "gp_sparse_set_inducing")
        self.Mz = Z.shape[0]

    def sparse_fit(self, maxtries=5):
        """(lml, jitter of Kmm's ladder, jitter of B's ladder)."""
        lml, jk, jb = _fit_scalars()
        check(self.lib, self.lib.gp_sparse_fit(self.h, int(maxtries), ctypes.byref(lml), ctypes.byref(jk), ctypes.byref(jb)),
              "gp_sparse_fit")
        return lml.value, jk.value, jb.value

    def sparse_fit_grad(self, nls, maxtries=5):
        """gp_sparse_fit and its gradients as one call: (lml, (dvariance, dlengthscale[nls], dnoise, dZ [Mz, D]))."""
        lml, dv, dn = _fit_scalars()
        dl = self._grad_ls(nls)
        dZ = np.empty((self.Mz, self.D))
        rc = self.lib.gp_sparse_fit_grad(self.h, int(maxtries), ctypes.byref(lml), ctypes.byref(dv), dptr(dl), ctypes.byref(dn),
                                         dptr(dZ))
        check(self.lib, rc, "gp_sparse_fit_grad")
        return lml.value, (dv.value, dl, dn.value, dZ)

    def sparse_fit_grad_batch(self, Z, variances, lengthscales, noises, maxtries=5):
        """gp_sparse_fit_grad for R members in one call, member r over the inducing inputs ``Z[r]`` ([R, Mz, D]) and its own
        parameters; the resident inducing inputs, sparse fit and everything else on the handle are untouched.  Returns
        ((lml, jitter_kmm, jitter_b) [R] each, (dvariance [R], dlengthscale [R, nls], dnoise [R], dZ [R, Mz, D]), status [R]);
        a member with status[r] != 0 has NaN outputs."""
        R, var, ls, noi = self._batch_params(variances, lengthscales, noises)
        Z = as_f64(Z, 3)
        if Z.shape[0] != R or Z.shape[2] != self.D:
            raise ValueError("Z has shape %s, expected (%d, Mz, %d): the inducing inputs of every member" % (Z.shape, R, self.D))
        Mz = Z.shape[1]
        lml, jk, jb = np.empty(R), np.empty(R), np.empty(R)
        dv, dl, dn = np.empty(R), np.empty((R, ls.shape[1])), np.empty(R)
        dZ = np.empty((R, Mz, self.D))
        status = np.zeros(R, dtype=np.int32)
        rc = self.lib.gp_sparse_fit_grad_batch(self.h, int(R), int(Mz), dptr(Z), dptr(var), dptr(ls), dptr(noi), int(maxtries),
                                               dptr(lml), dptr(jk), dptr(jb), dptr(dv), dptr(dl), dptr(dn), dptr(dZ),
                                               status.ctypes.data_as(c_int_p))
        check(self.lib, rc, "gp_sparse_fit_grad_batch")
        return (lml, jk, jb), (dv, dl, dn, dZ), status

    def sparse_batch_bytes(self, R, Mz):
        """Bytes of device buffers sparse_fit_grad_batch would hold for R members of Mz inducing inputs over the resident data."""
        out = ctypes.c_int64(0)
        check(self.lib, self.lib.gp_sparse_batch_bytes(self.h, int(R), int(Mz), ctypes.byref(out)), "gp_sparse_batch_bytes")
        return int(out.value)

    def sparse_posterior(self):
        """(woodbury_vector [Mz, P], woodbury_inv [Mz, Mz]) of the sparse fit."""
        wv, wi = np.empty((self.Mz, self.P)), np.empty((self.Mz, self.Mz))
        check(self.lib, self.lib.gp_sparse_posterior(self.h, dptr(wv), dptr(wi)), "gp_sparse_posterior")
        return wv, wi

    def sparse_predict(self, Xs, include_noise=True, grad=False):
        """(mean [M, P], var [M, 1]) at ``Xs`` and, with ``grad``, (dmdx [M, D, P], dvdx [M, D]) as well."""
        Xs = as_f64(Xs, 2)
        if Xs.shape[1] != self.D:
            raise ValueError("candidates have %d columns, model has %d" % (Xs.shape[1], self.D))
        M = Xs.shape[0]
        mean, var = np.empty((M, self.P)), np.empty((M, 1))
        dm = np.empty((M, self.D, self.P)) if grad else None
        dv = np.empty((M, self.D)) if grad else None
        rc = self.lib.gp_sparse_predict(self.h, dptr(Xs), M, int(bool(include_noise)), dptr(mean), dptr(var),
                                        dptr(dm) if grad else None, dptr(dv) if grad else None)
        check(self.lib, rc, "gp_sparse_predict")
        return (mean, var, dm, dv) if grad else (mean, var)

    def sparse_fmin(self):
        v = ctypes.c_double()
        check(self.lib, self.lib.gp_sparse_fmin(self.h, ctypes.byref(v)), "gp_sparse_fmin")
        return v.value

    # -- acquisitions over the sparse posterior (include/gphip.h): a table of the sparse model's own, and rows by value
    def sparse_set_candidates(self, Xs):
        Xs = as_f64(Xs, 2)
        if Xs.shape[1] != self.D:
            raise ValueError("candidates have %d columns, model has %d" % (Xs.shape[1], self.D))
        check(self.lib, self.lib.gp_sparse_set_candidates(self.h, dptr(Xs), Xs.shape[0]), "gp_sparse_set_candidates")
        self.sparse_M = Xs.shape[0]

    def sparse_acq(self, type_, par, fmin, y_mean=0.0, y_std=1.0, grad=False, lp=None):
        """Negated acquisition of the sparse table, [M, 1] (1-D with ``lp``, as AcquisitionLP returns it), and with ``grad`` its
        gradient [M, D]: the return shapes of ``acq`` / ``acq_grad`` / ``acq_lp`` / ``acq_lp_grad``."""
        on, tr, keep, nb, pX, pr, ps = _lp_pack(lp)
        M = self.sparse_M
        out = np.empty(M) if on else np.empty((M, 1))
        dout = np.empty((M, self.D)) if grad else None
        check(self.lib, self.lib.gp_sparse_acq(self.h, int(type_), float(par), float(fmin), float(y_mean), float(y_std), on, tr,
                                               pX, nb, pr, ps, dptr(out), dptr(dout) if grad else None), "gp_sparse_acq")
        return (out, dout) if grad else out

    def sparse_acq_argbest(self, type_, par, fmin, sense, y_mean=0.0, y_std=1.0, lp=None, exclude=()):
        on, tr, keep, nb, pX, pr, ps = _lp_pack(lp)
        ex = np.asarray(list(exclude), dtype=np.int64)
        idx, val = ctypes.c_int64(), ctypes.c_double()
        check(self.lib, self.lib.gp_sparse_acq_argbest(self.h, int(type_), float(par), float(fmin), float(y_mean), float(y_std),
                                                       on, tr, pX, nb, pr, ps, int(sense), ex.ctypes.data_as(c_int64_p),
                                                       int(ex.size), ctypes.byref(idx), ctypes.byref(val)),
              "gp_sparse_acq_argbest")
        return idx.value, val.value

    def sparse_acq_topk(self, type_, par, fmin, sense, k, y_mean=0.0, y_std=1.0):
        idx = np.empty(k, dtype=np.int64)
        val = np.empty(k)
        check(self.lib, self.lib.gp_sparse_acq_topk(self.h, int(type_), float(par), float(fmin), float(y_mean), float(y_std),
                                                    int(sense), int(k), idx.ctypes.data_as(c_int64_p), dptr(val)),
              "gp_sparse_acq_topk")
        return idx, val

    def sparse_predict_rows(self, Xs, include_noise=True, grad=False):
        """(mean [M, 1], var [M, 1]) and, with ``grad``, (dmdx [M, D, 1], dvdx [M, D]) as well: ``predict_rows`` on the sparse model."""
        Xs = as_f64(Xs, 2)
        M = Xs.shape[0]
        mean, var = np.empty((M, 1)), np.empty((M, 1))
        dm = np.empty((M, self.D, 1)) if grad else None
        dv = np.empty((M, self.D)) if grad else None
        rc = self.lib.gp_sparse_predict_rows(self.h, Xs.ctypes.data, M, 1 if include_noise else 0, mean.ctypes.data,
                                             var.ctypes.data, dm.ctypes.data if grad else None, dv.ctypes.data if grad else None)
        if rc:
            check(self.lib, rc, "gp_sparse_predict_rows")
        return (mean, var, dm, dv) if grad else (mean, var)

    def sparse_mean_grad_rows(self, Xs):
        """d mean / dx [M, D, 1] of a handful of locations, alone (the woodbury vector only)."""
        Xs = as_f64(Xs, 2)
        M = Xs.shape[0]
        dm = np.empty((M, self.D, 1))
        rc = self.lib.gp_sparse_predict_rows(self.h, Xs.ctypes.data, M, 0, None, None, dm.ctypes.data, None)
        if rc:
            check(self.lib, rc, "gp_sparse_predict_rows")
        return dm

    sparse_acq_rows = _acq_rows_entry("gp_sparse_acq_rows", """``acq_rows`` on the sparse model: negated acquisition [M, 1] (1-D with
        ``lp``) and, with ``grad``, its gradient [M, D].""")

    def sparse_rows_stats(self):
        a, b = ctypes.c_int64(), ctypes.c_int64()
        check(self.lib, self.lib.gp_sparse_rows_stats(self.h, ctypes.byref(a), ctypes.byref(b)), "gp_sparse_rows_stats")
        return dict(fused=a.value, fallback=b.value)

    # -- the joint posterior of the sparse model (include/gphip.h, csrc/api_sparse_cov.hip)
    def _sparse_rows_of(self, Xs, what):
        Xs = as_f64(Xs, 2)
        if Xs.shape[1] != self.D:
            raise ValueError("%s have %d columns, model has %d" % (what, Xs.shape[1], self.D))
        return Xs

    def sparse_predict_full_cov(self, Xs, include_noise=True):
        """(mean [M, P], cov [M, M]) of the sparse posterior at ``Xs``; cov is bitwise symmetric."""
        Xs = self._sparse_rows_of(Xs, "candidates")
        M = Xs.shape[0]
        mean, cov = np.empty((M, self.P)), np.empty((M, M))
        rc = self.lib.gp_sparse_predict_full_cov(self.h, dptr(Xs), M, int(bool(include_noise)), dptr(mean), dptr(cov))
        check(self.lib, rc, "gp_sparse_predict_full_cov")
        return mean, cov

    def sparse_posterior_samples(self, Xs, Z, include_noise=False, maxtries=5):
        """Z[S, M] standard normals -> (mean[M, P], dev[S, M], jitter) over the sparse posterior at ``Xs``: draw s of output d =
        mean[:, d] + dev[s]."""
        Xs = self._sparse_rows_of(Xs, "candidates")
        Z = as_f64(Z, 2)
        M = Xs.shape[0]
        if Z.shape[1] != M:
            raise ValueError("Z needs one column per row of Xs")
        mean, dev = np.empty((M, self.P)), np.empty((Z.shape[0], M))
        jit = ctypes.c_double()
        rc = self.lib.gp_sparse_posterior_samples(self.h, dptr(Xs), M, int(bool(include_noise)), dptr(Z), Z.shape[0], int(maxtries),
                                                  dptr(mean), dptr(dev), ctypes.byref(jit))
        check(self.lib, rc, "gp_sparse_posterior_samples")
        return mean, dev, jit.value

    def sparse_cov_set_points(self, X2):
        """Make ``X2`` [R, D] the resident second point set of ``sparse_cov_between``."""
        X2 = self._sparse_rows_of(X2, "the points")
        check(self.lib, self.lib.gp_sparse_cov_set_points(self.h, dptr(X2), X2.shape[0]), "gp_sparse_cov_set_points")
        self.sparse_R = X2.shape[0]

    def sparse_cov_between(self, X1):
        """cov [M1, R]: the sparse posterior covariance between the rows of ``X1`` and the resident points."""
        X1 = self._sparse_rows_of(X1, "locations")
        cov = np.empty((X1.shape[0], self.sparse_R))
        rc = self.lib.gp_sparse_cov_between(self.h, X1.ctypes.data, X1.shape[0], cov.ctypes.data)
        if rc:
            check(self.lib, rc, "gp_sparse_cov_between")
        return cov

    # -- the ensemble (include/gphip.h, gp_ens_*): S hyper-parameter members with resident posteriors --------------------------
    def ens_fit(self, variances, lengthscales, noises, maxtries=5):
        """Factor and keep S members ([S], [S, nls], [S]); returns (lml, logdet, jitter, fmin), [S] each."""
        var = as_f64(np.atleast_1d(variances), 1)
        noi = as_f64(np.atleast_1d(noises), 1)
        S = var.size
        want = getattr(self, "n_ls", None)
        if want is None:
            raise ValueError("set_params has not been called on this handle")
        ls = np.ascontiguousarray(np.asarray(lengthscales, dtype=float))
        if ls.ndim != 2 or ls.shape != (S, want) or noi.size != S:
            raise ValueError("expected variances [S], lengthscales [S, %d] and noises [S]; got %s, %s, %s"
                             % (want, var.shape, ls.shape, noi.shape))
        lml, logdet, jit, fmin = np.empty(S), np.empty(S), np.empty(S), np.empty(S)
        check(self.lib, self.lib.gp_ens_fit(self.h, int(S), dptr(var), dptr(ls), dptr(noi), int(maxtries), dptr(lml),
                                            dptr(logdet), dptr(jit), dptr(fmin)), "gp_ens_fit")
        self.ens_S = S
        return lml, logdet, jit, fmin

    def ens_info(self):
        n = ctypes.c_int(0)
        check(self.lib, self.lib.gp_ens_info(self.h, ctypes.byref(n)), "gp_ens_info")
        return n.value

    def ens_predict_rows(self, Xs, include_noise=True, grad=False):
        """Every member's posterior at M <= 8 locations: (mean [S, M], var [S, M]) and, with ``grad``, (dmdx, dvdx) [S, M, D]."""
        Xs = as_f64(Xs, 2)
        M, S = Xs.shape[0], self.ens_info()
        mean, var = np.empty((S, M)), np.empty((S, M))
        dm = np.empty((S, M, self.D)) if grad else None
        dv = np.empty((S, M, self.D)) if grad else None
        rc = self.lib.gp_ens_predict_rows(self.h, Xs.ctypes.data, M, 1 if include_noise else 0, mean.ctypes.data,
                                          var.ctypes.data, dm.ctypes.data if grad else None, dv.ctypes.data if grad else None)
        if rc:
            check(self.lib, rc, "gp_ens_predict_rows")
        return (mean, var, dm, dv) if grad else (mean, var)

    def ens_acq_rows(self, Xs, type_, par, grad=False):
        """The integrated acquisition, negated, [M, 1] (and its gradient [M, D]) at M <= 8 locations."""
        Xs = as_f64(Xs, 2)
        M = Xs.shape[0]
        out = np.empty((M, 1))
        dout = np.empty((M, self.D)) if grad else None
        rc = self.lib.gp_ens_acq_rows(self.h, Xs.ctypes.data, M, int(type_), par, out.ctypes.data,
                                      dout.ctypes.data if grad else None)
        if rc:
            check(self.lib, rc, "gp_ens_acq_rows")
        return (out, dout) if grad else out

    def ens_acq(self, type_, par):
        """The same value over the resident candidate table (set_candidates), [M, 1]."""
        out = np.empty((self.M, 1))
        check(self.lib, self.lib.gp_ens_acq(self.h, int(type_), float(par), dptr(out)), "gp_ens_acq")
        return out

    def ens_acq_argbest(self, type_, par, sense):
        idx, val = ctypes.c_int64(), ctypes.c_double()
        check(self.lib, self.lib.gp_ens_acq_argbest(self.h, int(type_), float(par), int(sense), ctypes.byref(idx),
                                                    ctypes.byref(val)), "gp_ens_acq_argbest")
        return idx.value, val.value

    # -- entropy search (include/gphip.h, gp_es_*) -------------------------------------------------------------------------
    def es_set_representers(self, Xr, y_mean=0.0, y_std=1.0):
        """Make ``Xr`` [R, D] the resident representers; (mu [R], cov [R, R]): their posterior with noise, un-normalised."""
        Xr = as_f64(Xr, 2)
        R = Xr.shape[0]
        mu, cov = np.empty(max(R, 1)), np.empty((max(R, 1), max(R, 1)))
        check(self.lib, self.lib.gp_es_set_representers(self.h, dptr(Xr), R, float(y_mean), float(y_std), dptr(mu), dptr(cov)),
              "gp_es_set_representers")
        return mu, cov

    def es_pmin(self, mu, cov, max_sweeps=50, tol=1e-3):
        """The EP sweeps of the R chains over the Gaussian (mu, cov): (P, MP, logS [R, R - 1], status [R], sweeps [R])."""
        mu, cov = as_f64(mu, 1), as_f64(cov, 2)
        R = mu.shape[0]
        if cov.shape != (R, R):
            raise ValueError("cov must be [R, R]")
        P, MP, logS = (np.zeros((R, max(R - 1, 0))) for _ in range(3))
        status, sweeps = np.zeros(max(R, 1), dtype=np.int32), np.zeros(max(R, 1), dtype=np.int32)
        check(self.lib, self.lib.gp_es_pmin(self.h, dptr(mu), dptr(cov), R, int(max_sweeps), float(tol), dptr(P), dptr(MP),
                                            dptr(logS), status.ctypes.data_as(c_int_p), sweeps.ctypes.data_as(c_int_p)),
              "gp_es_pmin")
        return P, MP, logS, status[:R], sweeps[:R]

    def es_set_belief(self, logP, u, G, Q, W):
        logP, u, G, Q, W = as_f64(np.ravel(logP), 1), as_f64(np.ravel(u), 1), as_f64(G, 2), as_f64(Q, 3), as_f64(np.ravel(W), 1)
        R = logP.shape[0]
        if u.shape != (R,) or G.shape != (R, R) or Q.shape != (R, R, R):
            raise ValueError("belief arrays disagree about R")
        check(self.lib, self.lib.gp_es_set_belief(self.h, dptr(logP), dptr(u), dptr(G), dptr(Q), R, dptr(W), W.shape[0]),
              "gp_es_set_belief")

    def es_acq(self, y_std=1.0):
        """The negated information gain of the resident candidates, [M, 1]."""
        out = np.empty((self.M, 1))
        check(self.lib, self.lib.gp_es_acq(self.h, float(y_std), dptr(out)), "gp_es_acq")
        return out

    def es_acq_rows(self, Xs, y_std=1.0):
        """The same value at the locations ``Xs`` [M, D] given by value, [M, 1]: up to eight take the fused rows path."""
        Xs = as_f64(Xs, 2)
        out = np.empty((Xs.shape[0], 1))
        rc = self.lib.gp_es_acq_rows(self.h, Xs.ctypes.data, Xs.shape[0], float(y_std), out.ctypes.data)
        if rc:
            check(self.lib, rc, "gp_es_acq_rows")
        return out

    def es_acq_argbest(self, sense, y_std=1.0):
        idx, val = ctypes.c_int64(), ctypes.c_double()
        check(self.lib, self.lib.gp_es_acq_argbest(self.h, float(y_std), int(sense), ctypes.byref(idx), ctypes.byref(val)),
              "gp_es_acq_argbest")
        return idx.value, val.value

    def predict(self, include_noise=True):
        mean = np.empty((self.M, self.P))
        var = np.empty((self.M, 1))
        check(self.lib, self.lib.gp_predict(self.h, int(bool(include_noise)), dptr(mean), dptr(var)), "gp_predict")
        return mean, var

    def predict_full_cov(self, include_noise=True):
        mean = np.empty((self.M, self.P))
        cov = np.empty((self.M, self.M))
        check(self.lib, self.lib.gp_predict_full_cov(self.h, int(bool(include_noise)), dptr(mean), dptr(cov)),
              "gp_predict_full_cov")
        return mean, cov

    def predict_grad(self, mean_only=False):
        dm = np.empty((self.M, self.D, self.P))
        if mean_only:      # the mean's gradients alone: no Ky^-1, no K* Ky^-1 (include/gphip.h)
            check(self.lib, self.lib.gp_predict_grad(self.h, dptr(dm), None), "gp_predict_grad")
            return dm
        dv = np.empty((self.M, self.D))
        check(self.lib, self.lib.gp_predict_grad(self.h, dptr(dm), dptr(dv)), "gp_predict_grad")
        return dm, dv

    def fmin(self):
        v = ctypes.c_double()
        check(self.lib, self.lib.gp_fmin(self.h, ctypes.byref(v)), "gp_fmin")
        return v.value

    def acq(self, type_, par, fmin, y_mean=0.0, y_std=1.0):
        out = np.empty((self.M, 1))
        check(self.lib, self.lib.gp_acq(self.h, int(type_), float(par), float(fmin), float(y_mean), float(y_std),
                                        dptr(out)), "gp_acq")
        return out

    def acq_grad(self, type_, par, fmin, y_mean=0.0, y_std=1.0):
        out = np.empty((self.M, 1))
        dout = np.empty((self.M, self.D))
        check(self.lib, self.lib.gp_acq_grad(self.h, int(type_), float(par), float(fmin), float(y_mean),
                                             float(y_std), dptr(out), dptr(dout)), "gp_acq_grad")
        return out, dout

    def acq_argbest(self, type_, par, fmin, sense, y_mean=0.0, y_std=1.0):
        idx, val = ctypes.c_int64(), ctypes.c_double()
        check(self.lib, self.lib.gp_acq_argbest(self.h, int(type_), float(par), float(fmin), float(y_mean),
                                                float(y_std), int(sense), ctypes.byref(idx), ctypes.byref(val)),
              "gp_acq_argbest")
        return idx.value, val.value

    # -- a handful of locations per call (include/gphip.h, gp_*_rows): set_candidates + the batched call in ONE entry point
    def predict_rows(self, Xs, include_noise=True, grad=False):
        """(mean [M, P], var [M, 1]) and, with ``grad``, (dmdx [M, D, P], dvdx [M, D]) as well."""
        Xs = as_f64(Xs, 2)
        M = Xs.shape[0]
        mean, var = np.empty((M, self.P)), np.empty((M, 1))
        if grad:
            dm, dv = np.empty((M, self.D, self.P)), np.empty((M, self.D))
            rc = self.lib.gp_predict_rows(self.h, Xs.ctypes.data, M, 1 if include_noise else 0, mean.ctypes.data,
                                          var.ctypes.data, dm.ctypes.data, dv.ctypes.data)
        else:
            rc = self.lib.gp_predict_rows(self.h, Xs.ctypes.data, M, 1 if include_noise else 0, mean.ctypes.data,
                                          var.ctypes.data, None, None)
        if rc:
            check(self.lib, rc, "gp_predict_rows")
        return (mean, var, dm, dv) if grad else (mean, var)

    def mean_grad_rows(self, Xs):
        """d mean / dx [M, D, P] of a handful of locations, alone: one pass over the training points (include/gphip.h)."""
        Xs = as_f64(Xs, 2)
        M = Xs.shape[0]
        dm = np.empty((M, self.D, self.P))
        rc = self.lib.gp_predict_rows(self.h, Xs.ctypes.data, M, 0, None, None, dm.ctypes.data, None)
        if rc:
            check(self.lib, rc, "gp_predict_rows")
        return dm

    acq_rows = _acq_rows_entry("gp_acq_rows", """Negated acquisition [M, 1] (and its gradient [M, D]); ``lp`` = (transform, Xb, r_x0,
        s_x0) adds the local penalisation, in which case the value comes back 1-D as AcquisitionLP returns it.""")

    # -- black-box constraints (include/gphip.h, gp_feas_*): the probability of feasibility behind EI / MPI ----------------------
    def feas_table(self, pack, key=None):
        """Cache log prod_k Phi of ``pack`` (a FeasPack) over the resident candidates; ``pack=None`` clears it.  The constraint
        handles' resident tables are this handle's afterwards.  ``key`` is remembered as ``feas_key`` (the staleness check)."""
        self.feas_key = None
        if pack is None:
            check(self.lib, self.lib.gp_feas_table(self.h, None, 0, None, None, None), "gp_feas_table")
            return
        check(self.lib, self.lib.gp_feas_table(self.h, *pack.args), "gp_feas_table")
        for h in pack.handles:
            h.M = self.M
            h.feas_key = None
        self.feas_key = key

    def feas_info(self):
        K, M = ctypes.c_int(0), ctypes.c_int64(0)
        check(self.lib, self.lib.gp_feas_info(self.h, ctypes.byref(K), ctypes.byref(M)), "gp_feas_info")
        return K.value, M.value

    def feas_get_table(self):
        K, M = self.feas_info()
        logF = np.empty(M)
        check(self.lib, self.lib.gp_feas_get_table(self.h, dptr(logF)), "gp_feas_get_table")
        return logF

    def acq_rows_feas(self, pack, Xs, type_, par, fmin, y_mean=0.0, y_std=1.0, grad=False):
        """Negated acquisition times the probability of feasibility [M, 1] (and its gradient [M, D]) at the rows of ``Xs``: this
        handle's and the constraint handles' fused passes, the fold and one drain in ONE call (gp_acq_rows_feas)."""
        Xs = np.ascontiguousarray(Xs, dtype=np.float64)
        if Xs.ndim != 2 or Xs.shape[1] != self.D:
            raise ValueError("expected locations [M, %d], got shape %s" % (self.D, Xs.shape))
        M = Xs.shape[0]
        out = np.empty((M, 1))
        dout = np.empty((M, self.D)) if grad else None
        rc = self.lib.gp_acq_rows_feas(self.h, pack.cons, pack.K, pack.args[2], pack.args[3], pack.args[4], Xs.ctypes.data, M,
                                       int(type_), par, fmin, y_mean, y_std, out.ctypes.data, dout.ctypes.data if grad else None)
        if rc:
            check(self.lib, rc, "gp_acq_rows_feas")
        return (out, dout) if grad else out

    def fmin_rows(self, rows):
        """``fmin`` over the listed training rows alone (gp_fmin_rows): the incumbent among the feasible observations."""
        rows = np.ascontiguousarray(np.ravel(rows), dtype=np.int64)
        v = ctypes.c_double()
        check(self.lib, self.lib.gp_fmin_rows(self.h, rows.ctypes.data_as(c_int64_p), rows.size, ctypes.byref(v)), "gp_fmin_rows")
        return v.value

    # -- the cost surface of cost-aware EI / MPI (include/gphip.h, gp_cost_*) ---------------------------------------------
    def cost_set(self, Xc, alpha, kernel, ard, variance, lengthscale, shift=0.0, scale=1.0, key=None):
        """Make (Xc [Nc, D], alpha [Nc], kernel parameters, normaliser) the handle's cost surface -- a copy: nothing of the
        cost GP is kept; ``Xc=None`` clears it.  ``key`` is remembered as ``cost_key`` (the routes' staleness check)."""
        if Xc is None:
            check(self.lib, self.lib.gp_cost_set(self.h, None, 0, None, 0, 0, 1.0, None, 0.0, 1.0), "gp_cost_set")
            self.cost_key = None
            return
        Xc = as_f64(Xc, 2)
        alpha = as_f64(np.ravel(alpha), 1)
        ls = as_f64(np.atleast_1d(lengthscale), 1)
        D = getattr(self, "D", None)
        if D is None:
            raise RuntimeError("gp_cost_set: set_data first (the surface has the handle's D columns)")
        if Xc.shape[1] != D:
            raise ValueError("gp_cost_set: the surface has %d columns, the handle has %d" % (Xc.shape[1], D))
        if alpha.size != Xc.shape[0] or ls.size != (D if ard else 1):
            raise ValueError("gp_cost_set: expected alpha [%d] and lengthscale [%d]; got %s, %s"
                             % (Xc.shape[0], D if ard else 1, alpha.shape, ls.shape))
        self.cost_key = None
        check(self.lib, self.lib.gp_cost_set(self.h, dptr(Xc), Xc.shape[0], dptr(alpha), int(kernel), int(bool(ard)),
                                             float(variance), dptr(ls), float(shift), float(scale)), "gp_cost_set")
        self.cost_key = key

    def cost_info(self):
        n = ctypes.c_int64(0)
        check(self.lib, self.lib.gp_cost_info(self.h, ctypes.byref(n)), "gp_cost_info")
        return n.value

    def cost_rows(self, Xs, grad=False):
        """log cost [M] of the resident surface at the rows of ``Xs`` and, with ``grad``, its x-gradient [M, D]."""
        Xs = as_f64(Xs, 2)
        if Xs.shape[1] != self.D:
            raise ValueError("locations have %d columns, the handle has %d" % (Xs.shape[1], self.D))
        M = Xs.shape[0]
        logc = np.empty(M)
        dlogc = np.empty((M, self.D)) if grad else None
        rc = self.lib.gp_cost_rows(self.h, Xs.ctypes.data, M, logc.ctypes.data, dlogc.ctypes.data if grad else None)
        if rc:
            check(self.lib, rc, "gp_cost_rows")
        return (logc, dlogc) if grad else logc

    # -- max-value entropy search (include/gphip.h, gp_mes_*): the samples behind GP_ACQ_MES and the sampler's reductions ---------
    def mes_set(self, ystar, key=None):
        """Make ``ystar`` [K] the handle's samples of the minimum's value (un-normalised) -- a copy; ``None`` or an empty array
        clears them.  ``key`` is remembered as ``mes_key`` (the routes' staleness check)."""
        self.mes_key = None
        if ystar is None or np.size(ystar) == 0:
            check(self.lib, self.lib.gp_mes_set(self.h, None, 0), "gp_mes_set")
            return
        ystar = as_f64(np.ravel(ystar), 1)
        check(self.lib, self.lib.gp_mes_set(self.h, dptr(ystar), ystar.size), "gp_mes_set")
        self.mes_key = key

    def mes_info(self):
        K = ctypes.c_int(0)
        check(self.lib, self.lib.gp_mes_info(self.h, ctypes.byref(K)), "gp_mes_info")
        return K.value

    def mes_logsurv(self, y, include_noise=False, y_mean=0.0, y_std=1.0):
        """sum_i log Phi((m_i - y_g) / s_i) [G] over the resident candidates' table posterior at the trial values ``y`` [G]."""
        y = as_f64(np.ravel(y), 1)
        out = np.empty(y.size)
        check(self.lib, self.lib.gp_mes_logsurv(self.h, int(bool(include_noise)), float(y_mean), float(y_std), dptr(y), y.size,
                                                dptr(out)), "gp_mes_logsurv")
        return out

    def mes_bracket(self, nsig=8.0, include_noise=False, y_mean=0.0, y_std=1.0):
        """(min_i (m_i - nsig s_i), min_i (m_i + nsig s_i)) over the resident candidates' table posterior."""
        lo, hi = ctypes.c_double(), ctypes.c_double()
        check(self.lib, self.lib.gp_mes_bracket(self.h, int(bool(include_noise)), float(y_mean), float(y_std), float(nsig),
                                                ctypes.byref(lo), ctypes.byref(hi)), "gp_mes_bracket")
        return lo.value, hi.value

    # -- posterior paths (include/gphip.h, gp_paths_*): function samples by pathwise conditioning on the resident factor ----------
    def paths_set(self, omega_unit, phase, w, z_eps, key=None):
        """Make S = ``w.shape[0]`` paths of F = ``w.shape[1]`` features resident from draws that do not depend on the
        hyper-parameters: ``omega_unit`` [F, D], ``phase`` [F], ``w`` [S, F], ``z_eps`` [S, N].  ``w`` None clears.  ``key`` is
        remembered as ``paths_key`` (the routes' staleness check); the library itself drops the paths with the factor."""
        self.paths_key = None
        if w is None or np.size(w) == 0:
            check(self.lib, self.lib.gp_paths_set(self.h, 0, 0, None, None, None, None), "gp_paths_set")
            return
        omega_unit, phase, w, z_eps = as_f64(omega_unit, 2), as_f64(np.ravel(phase), 1), as_f64(w, 2), as_f64(z_eps, 2)
        S, F = w.shape
        if omega_unit.shape != (F, self.D) or phase.size != F or z_eps.shape != (S, self.N):
            raise ValueError("paths_set: omega_unit [F, D], phase [F], w [S, F], z_eps [S, N] with F = %d, S = %d, D = %d, N = %d; got "
                             "%s, %s, %s, %s" % (F, S, self.D, self.N, omega_unit.shape, phase.shape, w.shape, z_eps.shape))
        check(self.lib, self.lib.gp_paths_set(self.h, S, F, dptr(omega_unit), dptr(phase), dptr(w), dptr(z_eps)), "gp_paths_set")
        self.paths_key = key

    def paths_info(self):
        """(S, F) of the resident paths, (0, 0) when none belong to the current fit."""
        S, F = ctypes.c_int(0), ctypes.c_int(0)
        check(self.lib, self.lib.gp_paths_info(self.h, ctypes.byref(S), ctypes.byref(F)), "gp_paths_info")
        return S.value, F.value

    def paths_table(self, y_mean=0.0, y_std=1.0):
        """Every resident path over the resident candidates: [S, M], de-normalised."""
        S = self.paths_info()[0]
        out = np.empty((max(S, 1), self.M))
        check(self.lib, self.lib.gp_paths_table(self.h, float(y_mean), float(y_std), dptr(out)), "gp_paths_table")
        return out[:S]

    def paths_argbest(self, sense=-1, y_mean=0.0, y_std=1.0):
        """Per path the best row of that table (lowest index among ties) and its value: (idx [S], val [S])."""
        idx = np.empty(GP_PATHS_MAX_S, dtype=np.int64)
        val = np.empty(GP_PATHS_MAX_S)
        check(self.lib, self.lib.gp_paths_argbest(self.h, float(y_mean), float(y_std), int(sense), idx.ctypes.data_as(c_int64_p),
                                                  dptr(val)), "gp_paths_argbest")
        S = self.paths_info()[0]
        return idx[:S].copy(), val[:S].copy()

    def paths_rows(self, Xs, path, y_mean=0.0, y_std=1.0, grad=False):
        """Up to GP_PATHS_MAX_ROWS locations by value, row i on path ``path[i]``: values [M] and, with ``grad``, gradients [M, D]."""
        Xs = np.ascontiguousarray(Xs, dtype=np.float64)
        if Xs.ndim != 2 or Xs.shape[1] != self.D:
            raise ValueError("expected locations of shape [M, %d], got %s" % (self.D, Xs.shape))
        M = Xs.shape[0]
        path = np.ascontiguousarray(np.broadcast_to(np.asarray(path, dtype=np.int32).ravel(), (M,)) if np.size(path) == 1
                                    else np.asarray(path, dtype=np.int32).ravel())
        if path.size != M:
            raise ValueError("one path index per location: %d locations, %d indices" % (M, path.size))
        out = np.empty(M)
        dout = np.empty((M, self.D)) if grad else None
        rc = self.lib.gp_paths_rows(self.h, Xs.ctypes.data, M, path.ctypes.data, y_mean, y_std, out.ctypes.data,
                                    dout.ctypes.data if grad else None)
        if rc:
            check(self.lib, rc, "gp_paths_rows")
        return (out, dout) if grad else out

    # -- joint expected improvement (include/gphip.h, gp_qei_*): a batch of q locations scored as a whole ---------------------------
    qei_key = None      # whose base samples are resident (AcquisitionQEI's staleness check)

    def qei_set(self, Z, key=None):
        """Make the base samples ``Z`` [S, q] (standard normals) resident -- a copy; they survive every fit of the handle.
        ``key`` is remembered as ``qei_key``."""
        Z = as_f64(Z, 2)
        self.qei_key = None
        check(self.lib, self.lib.gp_qei_set(self.h, dptr(Z), Z.shape[0], Z.shape[1]), "gp_qei_set")
        self.qei_key = key

    def qei_info(self):
        """(S, q) of the resident base samples, (0, 0) without."""
        S, q = ctypes.c_int(0), ctypes.c_int(0)
        check(self.lib, self.lib.gp_qei_info(self.h, ctypes.byref(S), ctypes.byref(q)), "gp_qei_info")
        return S.value, q.value

    def qei_stats(self):
        """(calls, calls with a gradient) gp_qei_rows has answered on this handle."""
        a, b = ctypes.c_int64(0), ctypes.c_int64(0)
        check(self.lib, self.lib.gp_qei_stats(self.h, ctypes.byref(a), ctypes.byref(b)), "gp_qei_stats")
        return a.value, b.value

    def qei_rows(self, Xq, par=0.0, fmin=0.0, y_mean=0.0, y_std=1.0, include_noise=True, grad=False, posterior=False):
        """The NEGATED joint expected improvement of the batch ``Xq`` [q, D] over the resident base samples (their leading q
        columns); with ``grad`` its negated gradient [q, D] as well; with ``posterior`` also the joint mean [q] and covariance
        [q, q] that were factored (de-normalised).  Returns the value, or a tuple (value[, gradient][, mean, cov]).  A pivot of the
        covariance that is not positive raises ``np.linalg.LinAlgError`` (``.args[1]``: its 1-based row)."""
        Xq = np.ascontiguousarray(Xq, dtype=np.float64)
        if Xq.ndim != 2 or Xq.shape[1] != self.D:
            raise ValueError("expected locations of shape [q, %d], got %s" % (self.D, Xq.shape))
        q = Xq.shape[0]
        out = np.empty(1)
        dout = np.empty((q, self.D)) if grad else None
        mean = np.empty(q) if posterior else None
        cov = np.empty((q, q)) if posterior else None
        rc = self.lib.gp_qei_rows(self.h, Xq.ctypes.data, q, int(bool(include_noise)), float(par), float(fmin), float(y_mean),
                                  float(y_std), out.ctypes.data, dout.ctypes.data if grad else None,
                                  mean.ctypes.data if posterior else None, cov.ctypes.data if posterior else None)
        if rc > 0:
            raise np.linalg.LinAlgError("gp_qei_rows: the batch's joint covariance is not positive definite at row %d" % rc, rc)
        if rc:
            check(self.lib, rc, "gp_qei_rows")
        res = (out[0],) + ((dout,) if grad else ()) + ((mean, cov) if posterior else ())
        return res if len(res) > 1 else res[0]

    # -- knowledge gradient (include/gphip.h, gp_kg_*): the entries are ``KgEntries``' methods, reached as ``handle.kg.<entry>`` ---------
    kg_key = None       # whose discretisation points are resident (AcquisitionKG's staleness check; the library drops the points
                        # with the fit, which kg.info() tells)

    @property
    def kg(self):
        return KgEntries(self)

    # -- noisy expected improvement (include/gphip.h, gp_nei_*): ``NeiEntries``' methods on the TWIN, reached as ``handle.nei.<entry>``
    @property
    def nei(self):
        return NeiEntries(self)

    # -- the mean function m(x) = x^T A + b of the exact GP (include/gphip.h, gp_mean_*) -----------------------------------
    def mean_set(self, A=None, b=None):
        """Make ``A`` [D, P] and ``b`` [P] the handle's mean function -- a copy; either may be None (that part is not there),
        both None clears it.  Drops the fit, as ``set_params`` does."""
        D, P = getattr(self, "D", None), getattr(self, "P", None)
        if D is None:
            raise RuntimeError("gp_mean_set: set_data first (A is [D, P] and b [P] of the data)")
        if A is not None:
            A = as_f64(A, 2)
            if A.shape != (D, P):
                raise ValueError("gp_mean_set: A has shape %s, the data wants (%d, %d)" % (A.shape, D, P))
        if b is not None:
            b = as_f64(np.ravel(b), 1)
            if b.size != P:
                raise ValueError("gp_mean_set: b has %d entries, the data wants %d" % (b.size, P))
        check(self.lib, self.lib.gp_mean_set(self.h, None if A is None else dptr(A), None if b is None else dptr(b)),
              "gp_mean_set")

    def mean_info(self):
        """(has_A, has_b) of the resident mean function; (False, False): none."""
        a, b = ctypes.c_int(0), ctypes.c_int(0)
        check(self.lib, self.lib.gp_mean_info(self.h, ctypes.byref(a), ctypes.byref(b)), "gp_mean_info")
        return bool(a.value), bool(b.value)

    def mean_grad(self):
        """dL/dA = X^T alpha [D, P] and dL/db = 1^T alpha [P] of the current fit."""
        dA, db = np.empty((self.D, self.P)), np.empty(self.P)
        check(self.lib, self.lib.gp_mean_grad(self.h, dptr(dA), dptr(db)), "gp_mean_grad")
        return dA, db

    def rows_stats(self):
        a, b = ctypes.c_int64(), ctypes.c_int64()
        check(self.lib, self.lib.gp_rows_stats(self.h, ctypes.byref(a), ctypes.byref(b)), "gp_rows_stats")
        return dict(fused=a.value, fallback=b.value)

    def rows_pass_stats(self):
        """Passes of the fused path so far: of at most four locations (``narrow``) and of 5 .. 8 (``wide``)."""
        a, b = ctypes.c_int64(), ctypes.c_int64()
        check(self.lib, self.lib.gp_rows_pass_stats(self.h, ctypes.byref(a), ctypes.byref(b)), "gp_rows_pass_stats")
        return dict(narrow=a.value, wide=b.value)

    def acq_lp(self, type_, par, fmin, transform, Xb=None, r_x0=None, s_x0=None, y_mean=0.0, y_std=1.0):
        keep, nb, pX, pr, ps = _lp_args(Xb, r_x0, s_x0)
        out = np.empty(self.M)
        check(self.lib, self.lib.gp_acq_lp(self.h, int(type_), float(par), float(fmin), float(y_mean), float(y_std),
                                           int(transform), pX, nb, pr, ps, dptr(out)), "gp_acq_lp")
        return out

    def acq_lp_grad(self, type_, par, fmin, transform, Xb=None, r_x0=None, s_x0=None, y_mean=0.0, y_std=1.0):
        """Penalised acquisition and its gradient at the resident candidates: (value[M], gradient[M, D])."""
        keep, nb, pX, pr, ps = _lp_args(Xb, r_x0, s_x0)
        out = np.empty(self.M)
        dout = np.empty((self.M, self.D))
        check(self.lib, self.lib.gp_acq_lp_grad(self.h, int(type_), float(par), float(fmin), float(y_mean), float(y_std),
                                                int(transform), pX, nb, pr, ps, dptr(out), dptr(dout)), "gp_acq_lp_grad")
        return out, dout

    def acq_lp_argbest(self, type_, par, fmin, transform, sense, Xb=None, r_x0=None, s_x0=None, exclude=(),
                       y_mean=0.0, y_std=1.0):
        keep, nb, pX, pr, ps = _lp_args(Xb, r_x0, s_x0)
        ex = np.asarray(list(exclude), dtype=np.int64)
        idx, val = ctypes.c_int64(), ctypes.c_double()
        check(self.lib, self.lib.gp_acq_lp_argbest(self.h, int(type_), float(par), float(fmin), float(y_mean),
                                                   float(y_std), int(transform), pX, nb, pr, ps, int(sense),
                                                   ex.ctypes.data_as(c_int64_p), int(ex.size), ctypes.byref(idx),
                                                   ctypes.byref(val)), "gp_acq_lp_argbest")
        return idx.value, val.value

    def phases(self):
        cap = 16
        names = (ctypes.c_char_p * cap)()
        ms = (ctypes.c_double * cap)()
        fl = (ctypes.c_double * cap)()
        by = (ctypes.c_double * cap)()
        n = self.lib.gp_last_phases(self.h, cap, names, ms, fl, by)
        return [dict(name=names[i].decode(), ms=ms[i], flops=fl[i], bytes=by[i]) for i in range(max(n, 0))]

    def profile(self, on=True):
        """on: False/0 off, True/1 events around every launch of the dominant GEMM symbol (8 waves, 128-tiles), 2 around
        every launch of the 64 x 64 work-unit symbol instead (stalls the latency chain: for an un-timed pass only)."""
        check(self.lib, self.lib.gp_profile(self.h, int(on)), "gp_profile")

    def gemm_stats(self):
        n, ms, fl = ctypes.c_int64(), ctypes.c_double(), ctypes.c_double()
        check(self.lib, self.lib.gp_gemm_stats(self.h, ctypes.byref(n), ctypes.byref(ms), ctypes.byref(fl)),
              "gp_gemm_stats")
        return dict(launches=n.value, ms=ms.value, flops=fl.value)

    def rns_stats(self):
        n, ms, ops = ctypes.c_int64(), ctypes.c_double(), ctypes.c_double()
        check(self.lib, self.lib.gp_rns_stats(self.h, ctypes.byref(n), ctypes.byref(ms), ctypes.byref(ops)), "gp_rns_stats")
        return dict(launches=n.value, ms=ms.value, ops=ops.value)

    def gemm_busy(self):
        b = ctypes.c_double()
        check(self.lib, self.lib.gp_gemm_busy(self.h, ctypes.byref(b)), "gp_gemm_busy")
        return b.value

    def gemm_trace(self, cap=100000):
        tiles = np.empty(cap, dtype=np.int64)
        K = np.empty(cap, dtype=np.int32)
        ms = np.empty(cap)
        n = self.lib.gp_gemm_trace(self.h, cap, tiles.ctypes.data_as(c_int64_p), K.ctypes.data_as(c_int_p), dptr(ms))
        return tiles[:n], K[:n], ms[:n]

    def synchronize(self):
        check(self.lib, self.lib.gp_synchronize(self.h), "gp_synchronize")

    def set_option(self, name, value):
        check(self.lib, self.lib.gp_set_option(self.h, name.encode(), int(value)), "gp_set_option")

    def debug_gemm(self, mode, C, A, B, K, r0, r1, c0, c1, tri=False):
        """Test hook: one GEMM launch on host operands (gp_debug_gemm); returns the new C, the arguments stay as they are."""
        A, B = as_f64(A, 2), as_f64(B, 2)
        out = np.array(C, dtype=np.float64, order="C")
        ld = out.shape[1]
        if A.shape != (r1 * 128, ld) or B.shape != (c1 * 128, ld) or out.shape[0] != r1 * 128:
            raise ValueError("C, A [r1 * 128, ld] and B [c1 * 128, ld] share one pitch")
        check(self.lib, self.lib.gp_debug_gemm(self.h, int(mode), dptr(out), dptr(A), dptr(B), ld, int(K), int(r0), int(r1),
                                               int(c0), int(c1), int(bool(tri))), "gp_debug_gemm")
        return out

    # -- RCCL ------------------------------------------------------------------
    def comm_unique_id(self):
        buf = ctypes.create_string_buffer(128)
        check(self.lib, self.lib.gp_comm_unique_id(buf), "gp_comm_unique_id")
        return buf.raw

    def comm_version(self):
        v = ctypes.c_int()
        check(self.lib, self.lib.gp_comm_version(ctypes.byref(v)), "gp_comm_version")
        return v.value

    def comm_init(self, uid, rank, nranks):
        check(self.lib, self.lib.gp_comm_init(self.h, uid, int(rank), int(nranks)), "gp_comm_init")

    def comm_info(self):
        r, n = ctypes.c_int(), ctypes.c_int()
        check(self.lib, self.lib.gp_comm_info(self.h, ctypes.byref(r), ctypes.byref(n)), "gp_comm_info")
        return r.value, n.value

    def comm_allgather_best(self, val, idx, nranks):
        vals = np.empty(nranks)
        idxs = np.empty(nranks, dtype=np.int64)
        check(self.lib, self.lib.gp_comm_allgather_best(self.h, float(val), int(idx), dptr(vals),
                                                        idxs.ctypes.data_as(c_int64_p)), "gp_comm_allgather_best")
        return vals, idxs

    def comm_allgather_topk(self, vals, idxs, nranks):
        vals = as_f64(vals, 1)
        idxs = np.ascontiguousarray(idxs, dtype=np.int64)
        k = vals.size
        av = np.empty(nranks * k)
        ai = np.empty(nranks * k, dtype=np.int64)
        check(self.lib, self.lib.gp_comm_allgather_topk(self.h, k, dptr(vals), idxs.ctypes.data_as(c_int64_p), dptr(av),
                                                        ai.ctypes.data_as(c_int64_p)), "gp_comm_allgather_topk")
        return av, ai

    def comm_bcast_fit(self, root=0):
        check(self.lib, self.lib.gp_comm_bcast_fit(self.h, int(root)), "gp_comm_bcast_fit")


class Group(object):
    """Owns one gp_group_t: the model replicated on ``devices`` (a device may appear more than once), one candidate table
    split over them, winners merged with NumPy's lowest-index rule (include/gphip.h, gp_group_*)."""

    def __init__(self, devices):
        self.lib = load()
        devs = np.ascontiguousarray(list(devices), dtype=np.int32)
        if devs.ndim != 1 or devs.size < 1:
            raise ValueError("devices must be a non-empty list of HIP device ordinals")
        h = _vp()
        check(self.lib, self.lib.gp_group_create(ctypes.byref(h), int(devs.size), devs.ctypes.data_as(c_int_p)),
              "gp_group_create")
        self.h = h
        self.devices = tuple(int(d) for d in devs)

    def close(self):
        if getattr(self, "h", None):
            self.lib.gp_group_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        n, r = ctypes.c_int(), ctypes.c_int()
        buf = ctypes.create_string_buffer(256)
        check(self.lib, self.lib.gp_group_info(self.h, ctypes.byref(n), ctypes.byref(r), buf, 256), "gp_group_info")
        return dict(ndev=n.value, rccl=bool(r.value), note=buf.value.decode())

    def set_data(self, X, Y):
        X, Y = as_f64(X, 2), as_f64(Y, 2)
        if X.shape[0] != Y.shape[0]:
            raise ValueError("X and Y row counts differ")
        check(self.lib, self.lib.gp_group_set_data(self.h, dptr(X), dptr(Y), X.shape[0], X.shape[1], Y.shape[1]),
              "gp_group_set_data")
        self.N, self.D, self.P = X.shape[0], X.shape[1], Y.shape[1]

    def set_params(self, kernel, ard, variance, lengthscale, noise):
        ls = as_f64(np.atleast_1d(lengthscale), 1)
        if ls.size != (self.D if ard else 1):
            raise ValueError("lengthscale has %d entries, expected %d" % (ls.size, self.D if ard else 1))
        check(self.lib, self.lib.gp_group_set_params(self.h, int(kernel), int(bool(ard)), float(variance), dptr(ls),
                                                     float(noise)), "gp_group_set_params")

    def set_gower(self, is_discrete=None, ranges=None):
        if is_discrete is None:
            check(self.lib, self.lib.gp_group_set_gower(self.h, 0, None, None), "gp_group_set_gower")
            return
        disc = np.ascontiguousarray(is_discrete, dtype=np.int32)
        rng = as_f64(ranges, 1)
        check(self.lib, self.lib.gp_group_set_gower(self.h, 1, disc.ctypes.data_as(c_int_p), dptr(rng)), "gp_group_set_gower")

    def set_option(self, name, value):
        check(self.lib, self.lib.gp_group_set_option(self.h, name.encode(), int(value)), "gp_group_set_option")

    def fit(self, maxtries=5):
        lml, logdet, jit = _fit_scalars()
        check(self.lib, self.lib.gp_group_fit(self.h, int(maxtries), ctypes.byref(lml), ctypes.byref(logdet),
                                              ctypes.byref(jit)), "gp_group_fit")
        return lml.value, logdet.value, jit.value

    def fmin(self):
        v = ctypes.c_double()
        check(self.lib, self.lib.gp_group_fmin(self.h, ctypes.byref(v)), "gp_group_fmin")
        return v.value

    def set_candidates(self, Xs):
        Xs = as_f64(Xs, 2)
        if Xs.shape[1] != self.D:
            raise ValueError("candidates have %d columns, model has %d" % (Xs.shape[1], self.D))
        check(self.lib, self.lib.gp_group_set_candidates(self.h, dptr(Xs), Xs.shape[0]), "gp_group_set_candidates")
        self.M = Xs.shape[0]

    def acq_argbest(self, type_, par, fmin, sense, y_mean=0.0, y_std=1.0):
        idx, val = ctypes.c_int64(), ctypes.c_double()
        check(self.lib, self.lib.gp_group_acq_argbest(self.h, int(type_), float(par), float(fmin), float(y_mean),
                                                      float(y_std), int(sense), ctypes.byref(idx), ctypes.byref(val)),
              "gp_group_acq_argbest")
        return idx.value, val.value

    def acq_lp_argbest(self, type_, par, fmin, transform, sense, Xb=None, r_x0=None, s_x0=None, exclude=(), y_mean=0.0,
                       y_std=1.0):
        keep, nb, pX, pr, ps = _lp_args(Xb, r_x0, s_x0)
        ex = np.asarray(list(exclude), dtype=np.int64)
        idx, val = ctypes.c_int64(), ctypes.c_double()
        check(self.lib, self.lib.gp_group_acq_lp_argbest(self.h, int(type_), float(par), float(fmin), float(y_mean),
                                                         float(y_std), int(transform), pX, nb, pr, ps, int(sense),
                                                         ex.ctypes.data_as(c_int64_p), int(ex.size), ctypes.byref(idx),
                                                         ctypes.byref(val)), "gp_group_acq_lp_argbest")
        return idx.value, val.value

    def acq_topk(self, type_, par, fmin, sense, k, y_mean=0.0, y_std=1.0):
        idx = np.empty(k, dtype=np.int64)
        val = np.empty(k)
        check(self.lib, self.lib.gp_group_acq_topk(self.h, int(type_), float(par), float(fmin), float(y_mean), float(y_std),
                                                   int(sense), int(k), idx.ctypes.data_as(c_int64_p), dptr(val)),
              "gp_group_acq_topk")
        return idx, val
