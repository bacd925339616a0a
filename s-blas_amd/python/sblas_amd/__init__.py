"""ctypes binding of libsblas_hip.so (the C ABI in include/sblas_hip.h).

Plumbing only: torch supplies device memory and streams, every compute call goes through the
shared library.  There is no CPU or torch fallback here -- if the HIP library is missing, or a
tensor is not on the GPU, the call raises.
"""
import ctypes as C
import os

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.normpath(os.path.join(_PKG, "..", ".."))
# SBLAS_LIB_PATH: A/B runs of two builds of the library (experiments only)
LIB_PATH = os.environ.get("SBLAS_LIB_PATH") or os.path.join(_ROOT, "lib", "libsblas_hip.so")

# every symbol include/sblas_hip.h declares (tests check that the .so exports all of them)
EXPORTS = [
    "sblas_hip_version", "sblas_hip_error_string", "sblas_hip_device_count",
    "sblas_hip_spmm_csr_f64_i32_workspace", "sblas_hip_spmm_csr_f64_i32", "sblas_hip_spmm_ldbt",
    "sblas_hip_dense_to_rowmajor_f64", "sblas_hip_spmm_csr_rowmajorB_f64_i32",
    "sblas_hip_debug_spmm_panel_stats", "sblas_hip_debug_reload_env",
    "sblas_hip_debug_spmm_kernel_events", "sblas_hip_debug_spmm_last_kernel_ms", "sblas_hip_spmv_csr_f64_i32", "sblas_hip_axpby_f64",
    "sblas_hip_comm_get", "sblas_hip_comm_release_all", "sblas_hip_allreduce_sum_f64",
    "sblas_hip_merge_rowblocks_f64", "sblas_hip_merge_rowblocks_local_f64",
    "sblas_find_row_of_nnz", "sblas_partition_nnz", "sblas_partition_dense",
    "sblas_mm_read_info", "sblas_mm_read_csr", "sblas_host_fill_rand0to1",
    "sblas_hip_spmm_csr_workspace", "sblas_hip_spmm_csr", "sblas_hip_spmv_csr", "sblas_hip_axpby",
    "sblas_hip_allreduce_sum", "sblas_hip_merge_rowblocks", "sblas_partition_nnz_i64",
    "sblas_hip_debug_validate_csr_i32",
    "sblas_hip_spmm_plan_create", "sblas_hip_spmm_plan_destroy", "sblas_hip_spmm_plan_info", "sblas_hip_spmm_csr_f64_i32_planned",
    "sblas_hip_spmv_plan_create", "sblas_hip_spmv_plan_destroy", "sblas_hip_spmv_plan_info", "sblas_hip_spmv_csr_f64_i32_planned",
    "sblas_spmv_plan_classify",
    "sblas_hip_spmm_csr_ordered", "sblas_hip_spmm_csr_ordered_f64_i32_planned", "sblas_hip_merge_rowblocks_ordered",
    "sblas_hip_spmm_plan_create_split", "sblas_hip_spmm_plan_split_info", "sblas_spmm_split_classify",
    "sblas_spmm_rule_describe",
    "sblas_hip_csr_transpose_workspace", "sblas_hip_csr_transpose_f64_i32", "sblas_hip_gather_f64",
    "sblas_hip_transpose_plan_create", "sblas_hip_transpose_plan_update_values", "sblas_hip_transpose_plan_info",
    "sblas_hip_transpose_plan_csc", "sblas_hip_transpose_plan_destroy", "sblas_hip_spmv_csr_t_f64_i32_planned",
    "sblas_hip_spmm_csr_t_f64_i32_planned",
    "sblas_hip_coo_to_csr_workspace", "sblas_hip_coo_to_csr_f64_i32", "sblas_hip_coo_plan_create", "sblas_hip_coo_plan_info",
    "sblas_hip_coo_plan_csr", "sblas_hip_coo_plan_assemble", "sblas_hip_coo_plan_destroy",
    "sblas_hip_sddmm_csr_workspace", "sblas_hip_sddmm_csr_f64_i32",
    "sblas_hip_csr_softmax_workspace", "sblas_hip_csr_softmax_f64_i32", "sblas_hip_csr_softmax_backward_f64_i32",
    "sblas_hip_csr_attention_workspace", "sblas_hip_csr_attention_f64_i32", "sblas_hip_csr_attention_backward_f64_i32",
    "sblas_hip_spgemm_limits", "sblas_hip_spgemm_classify", "sblas_hip_spgemm_group_width", "sblas_hip_spgemm_check_nnz",
    "sblas_hip_spgemm_plan_create", "sblas_hip_spgemm_plan_info", "sblas_hip_spgemm_plan_csr", "sblas_hip_spgemm_plan_numeric",
    "sblas_hip_spgemm_plan_destroy",
    "sblas_hip_sptrsv_limits", "sblas_sptrsv_levels", "sblas_sptrsv_schedule", "sblas_sptrsv_pack",
    "sblas_hip_sptrsv_plan_create", "sblas_hip_sptrsv_plan_info", "sblas_hip_sptrsv_plan_order", "sblas_hip_sptrsv_plan_destroy",
    "sblas_hip_sptrsv_f64_i32_planned", "sblas_hip_sptrsm_f64_i32_planned",
    "sblas_hip_ilu0_limits", "sblas_ilu0_check", "sblas_hip_ilu0_plan_create", "sblas_hip_ilu0_plan_info",
    "sblas_hip_ilu0_plan_diag", "sblas_hip_ilu0_plan_destroy", "sblas_hip_ilu0_f64_i32_planned",
    "sblas_hip_color_limits", "sblas_csr_color", "sblas_hip_color_plan_create", "sblas_hip_color_plan_info",
    "sblas_hip_color_plan_order", "sblas_hip_color_plan_destroy",
    "sblas_hip_permute_plan_create", "sblas_hip_permute_plan_info", "sblas_hip_permute_plan_csr", "sblas_hip_permute_plan_inverse",
    "sblas_hip_permute_plan_values", "sblas_hip_permute_plan_destroy",
    "sblas_hip_spmv_plan_speaks_for", "sblas_hip_sptrsv_plan_speaks_for",
    "sblas_krylov_limits", "sblas_krylov_dot_ref", "sblas_krylov_launches", "sblas_hip_krylov_dot_workspace", "sblas_hip_krylov_dot_f64",
    "sblas_hip_krylov_update_f64", "sblas_hip_krylov_plan_create", "sblas_hip_krylov_plan_info", "sblas_hip_krylov_plan_destroy",
    "sblas_hip_krylov_start", "sblas_hip_krylov_iterate", "sblas_hip_krylov_status",
    "sblas_gmres_limits", "sblas_gmres_step_ref", "sblas_gmres_solve_ref", "sblas_gmres_launches", "sblas_hip_gmres_dots_workspace",
    "sblas_hip_gmres_dots_f64", "sblas_hip_gmres_project_f64", "sblas_hip_gmres_combine_f64", "sblas_hip_gmres_plan_create",
    "sblas_hip_gmres_plan_info", "sblas_hip_gmres_plan_destroy", "sblas_hip_gmres_start", "sblas_hip_gmres_iterate",
    "sblas_hip_gmres_status",
    "sblas_amg_limits", "sblas_amg_aggregate", "sblas_amg_launches", "sblas_amg_wd_ref", "sblas_amg_cycle_ref",
    "sblas_hip_amg_plan_create", "sblas_hip_amg_plan_info", "sblas_hip_amg_plan_level", "sblas_hip_amg_plan_setup",
    "sblas_hip_amg_plan_apply", "sblas_hip_amg_plan_check", "sblas_hip_amg_plan_speaks_for", "sblas_hip_amg_plan_destroy",
    "sblas_hip_amg_sweep_f64", "sblas_hip_amg_restrict_f64", "sblas_hip_amg_prolong_f64",
]
# what include/sblas_hip_amg_sa.h declares (smoothed aggregation); kept apart from EXPORTS, which names sblas_hip.h's own
EXPORTS_AMG_SA = [
    "sblas_amg_keep_level", "sblas_amg_prolongator_ref", "sblas_amg_transfer_ref", "sblas_amg_cycle_sa_ref",
    "sblas_hip_amg_plan_create_ex", "sblas_hip_amg_plan_transfer", "sblas_hip_amg_plan_options", "sblas_hip_amg_pvalues_f64",
]
# what include/sblas_hip_amg_dev.h declares (aggregation on the device)
EXPORTS_AMG_DEV = [
    "sblas_amg_roots_rounds_ref", "sblas_hip_amg_aggregate_workspace", "sblas_hip_amg_aggregate_i32", "sblas_hip_amg_plan_create_dev",
]
# what include/sblas_hip_cheby.h declares (Chebyshev smoothing on a device eigenvalue estimate)
EXPORTS_CHEBY = [
    "sblas_cheby_limits", "sblas_cheby_start_ref", "sblas_cheby_lanczos_ref", "sblas_cheby_ritz_ref", "sblas_cheby_rowbound_ref",
    "sblas_cheby_lambda_ref", "sblas_cheby_coef_ref", "sblas_cheby_apply_ref",
    "sblas_hip_cheby_plan_create", "sblas_hip_cheby_plan_setup", "sblas_hip_cheby_plan_apply", "sblas_hip_cheby_plan_smooth",
    "sblas_hip_cheby_plan_check", "sblas_hip_cheby_plan_scalars", "sblas_hip_cheby_plan_info", "sblas_hip_cheby_plan_speaks_for",
    "sblas_hip_cheby_plan_destroy",
    "sblas_hip_amg_plan_setup_ex", "sblas_hip_amg_plan_eig", "sblas_amg_launches_cheb", "sblas_amg_cycle_cheb_ref", "sblas_amg_cycle_cheb_sa_ref",
]
# what include/sblas_hip_krylov_multi.h declares (PCG and BiCGStab for several right-hand sides on one SpMM per product)
EXPORTS_KRYLOV_MULTI = [
    "sblas_krylov_multi_limits", "sblas_krylov_multi_precond_ok", "sblas_krylov_multi_launches", "sblas_krylov_multi_grid",
    "sblas_krylov_scalar_step_ref",
    "sblas_hip_krylov_multi_dot_workspace", "sblas_hip_krylov_multi_dot_f64", "sblas_hip_krylov_multi_update_f64",
    "sblas_hip_krylov_multi_plan_create", "sblas_hip_krylov_multi_plan_info", "sblas_hip_krylov_multi_plan_destroy",
    "sblas_hip_krylov_multi_start", "sblas_hip_krylov_multi_iterate", "sblas_hip_krylov_multi_status",
]
# what include/sblas_hip_amg_multi.h declares (the AMG cycle on a block of columns and its seat under the solvers above)
EXPORTS_AMG_MULTI = [
    "sblas_amg_multi_limits", "sblas_amg_multi_grid", "sblas_krylov_multi_precond_plan_ok", "sblas_krylov_multi_launches_ex",
    "sblas_hip_amg_plan_reserve_multi", "sblas_hip_amg_plan_multi_info", "sblas_hip_amg_plan_apply_multi",
    "sblas_hip_amg_sweep_multi_f64", "sblas_hip_amg_restrict_multi_f64", "sblas_hip_amg_prolong_multi_f64",
    "sblas_hip_krylov_multi_plan_create_ex",
]
# what include/sblas_hip_sptrsm_tile.h declares (the triangular solve on a block of columns with the single solve's bits, and
# ILU(0)'s seat under the multi-right-hand-side solvers)
EXPORTS_SPTRSM_TILE = [
    "sblas_sptrsm_tile_limits", "sblas_sptrsm_tile_grid", "sblas_krylov_multi_precond_pair_ok", "sblas_krylov_multi_launches_pair",
    "sblas_hip_sptrsm_tiled_f64_i32_planned", "sblas_hip_krylov_multi_plan_create_pair",
]
# what include/sblas_hip_gmres_multi.h declares (restarted GMRES for several right-hand sides on one SpMM per Arnoldi step)
EXPORTS_GMRES_MULTI = [
    "sblas_gmres_multi_limits", "sblas_gmres_multi_grid", "sblas_gmres_multi_launches", "sblas_gmres_multi_precond_ok",
    "sblas_gmres_multi_precond_plan_ok", "sblas_gmres_multi_precond_pair_ok",
    "sblas_hip_gmres_multi_dots_workspace", "sblas_hip_gmres_multi_dots_f64", "sblas_hip_gmres_multi_project_f64",
    "sblas_hip_gmres_multi_combine_f64",
    "sblas_hip_gmres_multi_plan_create", "sblas_hip_gmres_multi_plan_info", "sblas_hip_gmres_multi_plan_block",
    "sblas_hip_gmres_multi_plan_destroy", "sblas_hip_gmres_multi_start", "sblas_hip_gmres_multi_iterate", "sblas_hip_gmres_multi_status",
]
# what include/sblas_hip_geam.h declares (CSR addition C = alpha * A + beta * B on a plan that re-adds)
EXPORTS_GEAM = [
    "sblas_geam_check_nnz", "sblas_geam_ref",
    "sblas_hip_geam_plan_create", "sblas_hip_geam_plan_info", "sblas_hip_geam_plan_csr", "sblas_hip_geam_plan_maps",
    "sblas_hip_geam_plan_numeric", "sblas_hip_geam_plan_destroy",
]
# what include/sblas_hip_mspgemm.h declares (masked SpGEMM out = M o (X Y^T) on a CSR pattern, on a plan that re-multiplies)
EXPORTS_MSPGEMM = [
    "sblas_mspgemm_limits", "sblas_mspgemm_ref",
    "sblas_hip_mspgemm_plan_create", "sblas_hip_mspgemm_plan_info", "sblas_hip_mspgemm_plan_numeric", "sblas_hip_mspgemm_plan_destroy",
]
# what include/sblas_hip_sddmm_narrow.h declares (SDDMM at k <= 8 on a part of a CSR pattern: the values gradient of the solves)
EXPORTS_SDDMM_NARROW = [
    "sblas_sddmm_narrow_limits", "sblas_sddmm_narrow_ref", "sblas_hip_sddmm_narrow_f64_i32",
]
# what include/sblas_hip_fsai.h declares (FSAI: a factorised sparse approximate inverse on a device plan)
EXPORTS_FSAI = [
    "sblas_fsai_limits", "sblas_fsai_pattern", "sblas_fsai_ref",
    "sblas_hip_fsai_plan_create", "sblas_hip_fsai_plan_setup", "sblas_hip_fsai_plan_apply", "sblas_hip_fsai_plan_check",
    "sblas_hip_fsai_plan_csr", "sblas_hip_fsai_plan_info", "sblas_hip_fsai_plan_speaks_for", "sblas_hip_fsai_plan_destroy",
]


# what include/sblas_hip_eigsh.h declares (thick-restart Lanczos eigenpairs on a device plan)
EXPORTS_EIGSH = [
    "sblas_eigsh_limits", "sblas_eigsh_sizes", "sblas_eigsh_launches", "sblas_eigsh_jacobi_ref", "sblas_eigsh_ritz_ref", "sblas_eigsh_step_ref",
    "sblas_eigsh_rotate_ref", "sblas_hip_eigsh_rotate_f64", "sblas_hip_eigsh_ritz_f64", "sblas_hip_eigsh_plan_create", "sblas_hip_eigsh_start",
    "sblas_hip_eigsh_iterate", "sblas_hip_eigsh_status", "sblas_hip_eigsh_values", "sblas_hip_eigsh_vectors", "sblas_hip_eigsh_info",
    "sblas_hip_eigsh_destroy",
]


class SblasError(RuntimeError):
    pass


_lib = None


def lib():
    """Load (once) and return the ctypes handle.  Raises if the library was not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SblasError("libsblas_hip.so not built (%s): run __graft_entry__.build() / make -C s-blas_amd" % LIB_PATH)
    # torch wheels bundle their own libamdhip64.so.7 / libhsa-runtime64.so.1 / librccl.so.1.  Load torch FIRST so
    # that our DT_NEEDED entries (and the dlopen of RCCL) resolve by SONAME to the copies already in the process:
    # two HIP runtimes in one process do not share a device context.
    import torch  # noqa: F401
    L = C.CDLL(LIB_PATH)
    i64, i32, f64, vp, sz = C.c_int64, C.c_int32, C.c_double, C.c_void_p, C.c_size_t
    L.sblas_hip_version.restype = C.c_int
    L.sblas_hip_error_string.restype = C.c_char_p
    L.sblas_hip_error_string.argtypes = [C.c_int]
    L.sblas_hip_device_count.restype = C.c_int
    L.sblas_hip_spmm_ldbt.restype = i64
    L.sblas_hip_spmm_ldbt.argtypes = [i64]
    L.sblas_hip_spmm_csr_f64_i32_workspace.restype = sz
    L.sblas_hip_spmm_csr_f64_i32_workspace.argtypes = [i64, i64, i64, i64]
    L.sblas_hip_spmm_csr_f64_i32.restype = C.c_int
    L.sblas_hip_spmm_csr_f64_i32.argtypes = [C.c_int, vp, i64, i64, i64, vp, vp, vp, vp, i64, i64, f64, f64, vp, i64, vp, sz]
    L.sblas_hip_debug_validate_csr_i32.restype = C.c_int
    L.sblas_hip_debug_validate_csr_i32.argtypes = [C.c_int, vp, i64, i64, i64, vp, vp]
    L.sblas_hip_spmm_plan_create.restype = C.c_int
    L.sblas_hip_spmm_plan_create.argtypes = [C.c_int, vp, i64, i64, i64, vp, vp, i64, C.POINTER(vp)]
    L.sblas_hip_spmm_plan_create_split.restype = C.c_int
    L.sblas_hip_spmm_plan_create_split.argtypes = [C.c_int, vp, i64, i64, i64, vp, vp, i64, i64, i64, C.POINTER(vp)]
    L.sblas_hip_spmm_plan_split_info.restype = C.c_int
    L.sblas_hip_spmm_plan_split_info.argtypes = [vp, C.POINTER(i64)]
    L.sblas_spmm_split_classify.restype = i64
    L.sblas_spmm_split_classify.argtypes = [vp, i64, i64, i64, i64, vp, i64, vp, i64]
    L.sblas_spmm_rule_describe.restype = i64
    L.sblas_spmm_rule_describe.argtypes = [i64, i64, i64, i64, i64, i64, C.c_int, vp, vp, i64]
    L.sblas_hip_spmm_plan_destroy.restype = C.c_int
    L.sblas_hip_spmm_plan_destroy.argtypes = [vp]
    L.sblas_hip_spmm_plan_info.restype = C.c_int
    L.sblas_hip_spmm_plan_info.argtypes = [vp, C.POINTER(i64)]
    L.sblas_hip_spmm_csr_f64_i32_planned.restype = C.c_int
    L.sblas_hip_spmm_csr_f64_i32_planned.argtypes = [vp, C.c_int, vp, i64, i64, i64, vp, vp, vp, vp, i64, i64, f64, f64, vp, i64, vp, sz]
    L.sblas_hip_spmv_plan_create.restype = C.c_int
    L.sblas_hip_spmv_plan_create.argtypes = [C.c_int, vp, i64, i64, i64, vp, vp, C.POINTER(vp)]
    L.sblas_hip_spmv_plan_destroy.restype = C.c_int
    L.sblas_hip_spmv_plan_destroy.argtypes = [vp]
    L.sblas_hip_spmv_plan_info.restype = C.c_int
    L.sblas_hip_spmv_plan_info.argtypes = [vp, C.POINTER(i64)]
    L.sblas_hip_spmv_csr_f64_i32_planned.restype = C.c_int
    L.sblas_hip_spmv_csr_f64_i32_planned.argtypes = [vp, C.c_int, vp, i64, i64, i64, vp, vp, vp, vp, f64, f64, vp]
    L.sblas_spmv_plan_classify.restype = i64
    L.sblas_spmv_plan_classify.argtypes = [vp, i64, i64, i64, i64, vp, i64]
    L.sblas_hip_dense_to_rowmajor_f64.restype = C.c_int
    L.sblas_hip_dense_to_rowmajor_f64.argtypes = [C.c_int, vp, i64, i64, vp, i64, vp, i64]
    L.sblas_hip_spmm_csr_rowmajorB_f64_i32.restype = C.c_int
    L.sblas_hip_spmm_csr_rowmajorB_f64_i32.argtypes = [C.c_int, vp, i64, i64, i64, vp, vp, vp, vp, i64, i64, f64, f64, vp, i64]
    L.sblas_hip_debug_reload_env.restype = C.c_int
    L.sblas_hip_debug_reload_env.argtypes = []
    L.sblas_hip_debug_spmm_panel_stats.restype = C.c_int
    L.sblas_hip_debug_spmm_panel_stats.argtypes = [C.POINTER(C.c_uint64), C.c_int]
    L.sblas_hip_debug_spmm_kernel_events.restype = C.c_int
    L.sblas_hip_debug_spmm_kernel_events.argtypes = [C.c_int]
    L.sblas_hip_debug_spmm_last_kernel_ms.restype = C.c_int
    L.sblas_hip_debug_spmm_last_kernel_ms.argtypes = [C.POINTER(C.c_float)]
    L.sblas_hip_spmv_csr_f64_i32.restype = C.c_int
    L.sblas_hip_spmv_csr_f64_i32.argtypes = [C.c_int, vp, i64, i64, i64, vp, vp, vp, vp, f64, f64, vp]
    L.sblas_hip_axpby_f64.restype = C.c_int
    L.sblas_hip_axpby_f64.argtypes = [C.c_int, vp, i64, f64, vp, f64, vp]
    L.sblas_hip_comm_get.restype = C.c_int
    L.sblas_hip_comm_get.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(vp)]
    L.sblas_hip_comm_release_all.restype = None
    L.sblas_hip_allreduce_sum_f64.restype = C.c_int
    L.sblas_hip_allreduce_sum_f64.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), i64]
    L.sblas_hip_merge_rowblocks_f64.restype = C.c_int
    L.sblas_hip_merge_rowblocks_f64.argtypes = [vp, i64, i64, C.POINTER(i64), C.POINTER(i64), C.POINTER(vp), C.POINTER(vp),
                                                f64, f64, C.POINTER(vp), i64, C.POINTER(vp)]
    L.sblas_hip_merge_rowblocks_local_f64.restype = C.c_int
    L.sblas_hip_merge_rowblocks_local_f64.argtypes = [C.c_int, vp, i64, i64, C.c_int, C.POINTER(i64), C.POINTER(i64),
                                                      C.POINTER(vp), f64, f64, vp, i64]
    L.sblas_find_row_of_nnz.restype = i32
    L.sblas_find_row_of_nnz.argtypes = [vp, i32, i32]
    L.sblas_partition_nnz.restype = i64
    L.sblas_partition_nnz.argtypes = [vp, i32, i32, C.c_int, C.c_int, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(i64), vp]
    L.sblas_partition_dense.restype = C.c_int
    L.sblas_partition_dense.argtypes = [i64, C.c_int, C.c_int, C.POINTER(i64), C.POINTER(i64)]
    L.sblas_mm_read_info.restype = C.c_int
    L.sblas_mm_read_info.argtypes = [C.c_char_p] + [C.POINTER(i32)] * 4
    L.sblas_mm_read_csr.restype = C.c_int
    L.sblas_mm_read_csr.argtypes = [C.c_char_p, vp, vp, vp]
    L.sblas_host_fill_rand0to1.restype = C.c_int
    L.sblas_host_fill_rand0to1.argtypes = [vp, i64, C.c_uint]
    L.sblas_hip_spmm_csr_workspace.restype = sz
    L.sblas_hip_spmm_csr_workspace.argtypes = [C.c_int, C.c_int, i64, i64, i64, i64]
    L.sblas_hip_spmm_csr.restype = C.c_int
    L.sblas_hip_spmm_csr.argtypes = [C.c_int, vp, C.c_int, C.c_int, i64, i64, i64, vp, vp, vp, vp, i64, i64, f64, f64, vp, i64, vp, sz]
    L.sblas_hip_spmv_csr.restype = C.c_int
    L.sblas_hip_spmv_csr.argtypes = [C.c_int, vp, C.c_int, C.c_int, i64, i64, i64, vp, vp, vp, vp, f64, f64, vp]
    L.sblas_hip_axpby.restype = C.c_int
    L.sblas_hip_axpby.argtypes = [C.c_int, vp, C.c_int, i64, f64, vp, f64, vp]
    L.sblas_hip_allreduce_sum.restype = C.c_int
    L.sblas_hip_allreduce_sum.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(vp), i64]
    L.sblas_hip_merge_rowblocks.restype = C.c_int
    L.sblas_hip_merge_rowblocks.argtypes = [vp, C.c_int, i64, i64, C.POINTER(i64), C.POINTER(i64), C.POINTER(vp), C.POINTER(vp),
                                            f64, f64, C.POINTER(vp), i64, C.POINTER(vp)]
    L.sblas_hip_spmm_csr_ordered.restype = C.c_int
    L.sblas_hip_spmm_csr_ordered.argtypes = [C.c_int, vp, C.c_int, C.c_int, i64, i64, i64, vp, vp, vp, vp, i64, C.c_int, i64,
                                             f64, f64, vp, i64, C.c_int, vp, sz]
    L.sblas_hip_spmm_csr_ordered_f64_i32_planned.restype = C.c_int
    L.sblas_hip_spmm_csr_ordered_f64_i32_planned.argtypes = [vp, C.c_int, vp, i64, i64, i64, vp, vp, vp, vp, i64, C.c_int, i64,
                                                             f64, f64, vp, i64, C.c_int, vp, sz]
    L.sblas_hip_merge_rowblocks_ordered.restype = C.c_int
    L.sblas_hip_merge_rowblocks_ordered.argtypes = [vp, C.c_int, C.c_int, i64, i64, C.POINTER(i64), C.POINTER(i64), C.POINTER(vp),
                                                    C.POINTER(vp), f64, f64, C.POINTER(vp), i64, C.POINTER(vp)]
    L.sblas_hip_csr_transpose_workspace.restype = sz
    L.sblas_hip_csr_transpose_workspace.argtypes = [i64, i64, i64]
    L.sblas_hip_csr_transpose_f64_i32.restype = C.c_int
    L.sblas_hip_csr_transpose_f64_i32.argtypes = [C.c_int, vp, i64, i64, i64, vp, vp, vp, vp, vp, vp, vp, vp, sz]
    L.sblas_hip_gather_f64.restype = C.c_int
    L.sblas_hip_gather_f64.argtypes = [C.c_int, vp, i64, vp, vp, vp]
    L.sblas_hip_transpose_plan_create.restype = C.c_int
    L.sblas_hip_transpose_plan_create.argtypes = [C.c_int, vp, i64, i64, i64, vp, vp, vp, i64, C.c_int, C.POINTER(vp)]
    L.sblas_hip_transpose_plan_update_values.restype = C.c_int
    L.sblas_hip_transpose_plan_update_values.argtypes = [vp, vp, vp]
    L.sblas_hip_transpose_plan_info.restype = C.c_int
    L.sblas_hip_transpose_plan_info.argtypes = [vp, C.POINTER(i64)]
    L.sblas_hip_transpose_plan_csc.restype = C.c_int
    L.sblas_hip_transpose_plan_csc.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    L.sblas_hip_transpose_plan_destroy.restype = C.c_int
    L.sblas_hip_transpose_plan_destroy.argtypes = [vp]
    L.sblas_hip_coo_to_csr_workspace.restype = sz
    L.sblas_hip_coo_to_csr_workspace.argtypes = [i64, i64, i64]
    L.sblas_hip_coo_to_csr_f64_i32.restype = C.c_int
    L.sblas_hip_coo_to_csr_f64_i32.argtypes = [C.c_int, vp, i64, i64, i64, vp, vp, vp, C.c_int, vp, vp, vp, vp, vp, vp, sz]
    L.sblas_hip_coo_plan_create.restype = C.c_int
    L.sblas_hip_coo_plan_create.argtypes = [C.c_int, vp, i64, i64, i64, vp, vp, C.c_int, C.POINTER(vp)]
    L.sblas_hip_coo_plan_info.restype = C.c_int
    L.sblas_hip_coo_plan_info.argtypes = [vp, C.POINTER(i64)]
    L.sblas_hip_coo_plan_csr.restype = C.c_int
    L.sblas_hip_coo_plan_csr.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    L.sblas_hip_coo_plan_assemble.restype = C.c_int
    L.sblas_hip_coo_plan_assemble.argtypes = [vp, vp, vp, vp]
    L.sblas_hip_coo_plan_destroy.restype = C.c_int
    L.sblas_hip_coo_plan_destroy.argtypes = [vp]
    L.sblas_hip_spmv_csr_t_f64_i32_planned.restype = C.c_int
    L.sblas_hip_spmv_csr_t_f64_i32_planned.argtypes = [vp, C.c_int, vp, vp, f64, f64, vp]
    L.sblas_hip_spmm_csr_t_f64_i32_planned.restype = C.c_int
    L.sblas_hip_spmm_csr_t_f64_i32_planned.argtypes = [vp, C.c_int, vp, vp, i64, C.c_int, i64, f64, f64, vp, i64, C.c_int, vp, sz]
    L.sblas_partition_nnz_i64.restype = i64
    L.sblas_partition_nnz_i64.argtypes = [vp, i64, i64, C.c_int, C.c_int] + [C.POINTER(i64)] * 4 + [vp]
    L.sblas_hip_sddmm_csr_workspace.restype = sz
    L.sblas_hip_sddmm_csr_workspace.argtypes = [i64, i64, i64, i64, C.c_int, C.c_int]
    L.sblas_hip_sddmm_csr_f64_i32.restype = C.c_int
    L.sblas_hip_sddmm_csr_f64_i32.argtypes = [C.c_int, vp, i64, i64, i64, vp, vp, vp, i64, C.c_int, vp, i64, C.c_int, i64, f64, f64,
                                              vp, vp, sz]
    L.sblas_hip_csr_softmax_workspace.restype = sz
    L.sblas_hip_csr_softmax_workspace.argtypes = [i64, i64]
    L.sblas_hip_csr_softmax_f64_i32.restype = C.c_int
    L.sblas_hip_csr_softmax_f64_i32.argtypes = [C.c_int, vp, i64, i64, vp, vp, f64, vp, vp, sz]
    L.sblas_hip_csr_softmax_backward_f64_i32.restype = C.c_int
    L.sblas_hip_csr_softmax_backward_f64_i32.argtypes = [C.c_int, vp, i64, i64, vp, vp, vp, f64, vp, vp, sz]
    L.sblas_hip_csr_attention_workspace.restype = sz
    L.sblas_hip_csr_attention_workspace.argtypes = [i64, i64, i64, i64]
    L.sblas_hip_csr_attention_f64_i32.restype = C.c_int
    L.sblas_hip_csr_attention_f64_i32.argtypes = [C.c_int, vp, i64, i64, i64, vp, vp, vp, i64, vp, i64, vp, i64, i64, i64, f64,
                                                  vp, i64, vp, vp, vp, sz]
    L.sblas_hip_csr_attention_backward_f64_i32.restype = C.c_int
    L.sblas_hip_csr_attention_backward_f64_i32.argtypes = [C.c_int, vp, i64, i64, i64, vp, vp, vp, i64, vp, i64, vp, i64, i64, i64,
                                                           f64, vp, i64, vp, vp, vp, i64, vp, vp, vp, sz]
    L.sblas_hip_spgemm_limits.restype = C.c_int
    L.sblas_hip_spgemm_limits.argtypes = [C.POINTER(i64)]
    L.sblas_hip_spgemm_classify.restype = C.c_int
    L.sblas_hip_spgemm_classify.argtypes = [i64, vp, vp, C.c_int, C.c_int, i64, vp, vp, C.POINTER(i64)]
    L.sblas_hip_spgemm_group_width.restype = C.c_int
    L.sblas_hip_spgemm_group_width.argtypes = [i64, i64, i64]
    L.sblas_hip_spgemm_check_nnz.restype = C.c_int
    L.sblas_hip_spgemm_check_nnz.argtypes = [i64]
    L.sblas_hip_spgemm_plan_create.restype = C.c_int
    L.sblas_hip_spgemm_plan_create.argtypes = [C.c_int, vp, i64, i64, i64, vp, vp, vp, vp, C.c_int, i64, C.POINTER(vp)]
    L.sblas_hip_spgemm_plan_info.restype = C.c_int
    L.sblas_hip_spgemm_plan_info.argtypes = [vp, C.POINTER(i64)]
    L.sblas_hip_spgemm_plan_csr.restype = C.c_int
    L.sblas_hip_spgemm_plan_csr.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
    L.sblas_hip_spgemm_plan_numeric.restype = C.c_int
    L.sblas_hip_spgemm_plan_numeric.argtypes = [vp, vp, vp, vp, vp]
    L.sblas_hip_spgemm_plan_destroy.restype = C.c_int
    L.sblas_hip_spgemm_plan_destroy.argtypes = [vp]
    L.sblas_hip_sptrsv_limits.restype = C.c_int
    L.sblas_hip_sptrsv_limits.argtypes = [C.POINTER(i64)]
    L.sblas_sptrsv_levels.restype = C.c_int
    L.sblas_sptrsv_levels.argtypes = [i64, vp, vp, C.c_int, C.c_int, vp, C.POINTER(i64), C.POINTER(i64)]
    L.sblas_sptrsv_schedule.restype = C.c_int
    L.sblas_sptrsv_schedule.argtypes = [i64, vp, C.c_int, i64, vp, vp, C.POINTER(i64)]
    L.sblas_sptrsv_pack.restype = C.c_int
    L.sblas_sptrsv_pack.argtypes = [i64, vp, vp, i64, vp, vp, vp, vp, vp, C.POINTER(i64)]
    L.sblas_hip_sptrsv_plan_create.restype = C.c_int
    L.sblas_hip_sptrsv_plan_create.argtypes = [C.c_int, vp, i64, i64, vp, vp, C.c_int, C.c_int, C.c_int, i64, C.POINTER(vp), C.POINTER(i64)]
    L.sblas_hip_sptrsv_plan_info.restype = C.c_int
    L.sblas_hip_sptrsv_plan_info.argtypes = [vp, C.POINTER(i64)]
    L.sblas_hip_sptrsv_plan_order.restype = C.c_int
    L.sblas_hip_sptrsv_plan_order.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
    L.sblas_hip_sptrsv_plan_destroy.restype = C.c_int
    L.sblas_hip_sptrsv_plan_destroy.argtypes = [vp]
    L.sblas_hip_sptrsv_f64_i32_planned.restype = C.c_int
    L.sblas_hip_sptrsv_f64_i32_planned.argtypes = [vp, vp, vp, vp, vp, f64, vp, vp]
    L.sblas_hip_sptrsm_f64_i32_planned.restype = C.c_int
    L.sblas_hip_sptrsm_f64_i32_planned.argtypes = [vp, vp, vp, vp, vp, i64, f64, vp, i64, vp, i64]
    L.sblas_hip_ilu0_limits.restype = C.c_int
    L.sblas_hip_ilu0_limits.argtypes = [C.POINTER(i64)]
    L.sblas_ilu0_check.restype = C.c_int
    L.sblas_ilu0_check.argtypes = [i64, vp, vp, vp, C.POINTER(i64)]
    L.sblas_hip_ilu0_plan_create.restype = C.c_int
    L.sblas_hip_ilu0_plan_create.argtypes = [C.c_int, vp, i64, i64, vp, vp, C.c_int, i64, C.POINTER(vp), C.POINTER(i64)]
    L.sblas_hip_ilu0_plan_info.restype = C.c_int
    L.sblas_hip_ilu0_plan_info.argtypes = [vp, C.POINTER(i64)]
    L.sblas_hip_ilu0_plan_diag.restype = C.c_int
    L.sblas_hip_ilu0_plan_diag.argtypes = [vp, C.POINTER(vp)]
    L.sblas_hip_ilu0_plan_destroy.restype = C.c_int
    L.sblas_hip_ilu0_plan_destroy.argtypes = [vp]
    L.sblas_hip_ilu0_f64_i32_planned.restype = C.c_int
    L.sblas_hip_ilu0_f64_i32_planned.argtypes = [vp, vp, vp, vp, vp, vp]
    L.sblas_hip_color_limits.restype = C.c_int
    L.sblas_hip_color_limits.argtypes = [C.POINTER(i64)]
    L.sblas_csr_color.restype = C.c_int
    L.sblas_csr_color.argtypes = [i64, vp, vp, C.c_uint32, vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)]
    L.sblas_hip_color_plan_create.restype = C.c_int
    L.sblas_hip_color_plan_create.argtypes = [C.c_int, vp, i64, i64, vp, vp, C.c_uint32, C.POINTER(vp), C.POINTER(i64)]
    L.sblas_hip_color_plan_info.restype = C.c_int
    L.sblas_hip_color_plan_info.argtypes = [vp, C.POINTER(i64)]
    L.sblas_hip_color_plan_order.restype = C.c_int
    L.sblas_hip_color_plan_order.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    L.sblas_hip_color_plan_destroy.restype = C.c_int
    L.sblas_hip_color_plan_destroy.argtypes = [vp]
    L.sblas_hip_permute_plan_create.restype = C.c_int
    L.sblas_hip_permute_plan_create.argtypes = [C.c_int, vp, i64, i64, vp, vp, vp, C.POINTER(vp), C.POINTER(i64)]
    L.sblas_hip_permute_plan_info.restype = C.c_int
    L.sblas_hip_permute_plan_info.argtypes = [vp, C.POINTER(i64)]
    L.sblas_hip_permute_plan_csr.restype = C.c_int
    L.sblas_hip_permute_plan_csr.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    L.sblas_hip_permute_plan_inverse.restype = C.c_int
    L.sblas_hip_permute_plan_inverse.argtypes = [vp, C.POINTER(vp)]
    L.sblas_hip_permute_plan_values.restype = C.c_int
    L.sblas_hip_permute_plan_values.argtypes = [vp, vp, vp, vp]
    L.sblas_hip_permute_plan_destroy.restype = C.c_int
    L.sblas_hip_permute_plan_destroy.argtypes = [vp]
    L.sblas_hip_spmv_plan_speaks_for.restype = C.c_int
    L.sblas_hip_spmv_plan_speaks_for.argtypes = [vp, C.c_int, i64, i64, i64, vp, vp]
    L.sblas_hip_sptrsv_plan_speaks_for.restype = C.c_int
    L.sblas_hip_sptrsv_plan_speaks_for.argtypes = [vp, C.c_int, vp, vp]
    L.sblas_krylov_limits.restype = C.c_int
    L.sblas_krylov_limits.argtypes = [C.POINTER(i64)]
    L.sblas_krylov_dot_ref.restype = f64
    L.sblas_krylov_dot_ref.argtypes = [i64, vp, vp]
    L.sblas_krylov_launches.restype = i64
    L.sblas_krylov_launches.argtypes = [C.c_int, C.c_int, C.POINTER(i64), C.POINTER(i64)]
    L.sblas_hip_krylov_dot_workspace.restype = sz
    L.sblas_hip_krylov_dot_workspace.argtypes = [i64, C.c_int]
    L.sblas_hip_krylov_dot_f64.restype = C.c_int
    L.sblas_hip_krylov_dot_f64.argtypes = [C.c_int, vp, i64, C.c_int, C.POINTER(vp), C.POINTER(vp), vp, vp, sz]
    L.sblas_hip_krylov_update_f64.restype = C.c_int
    L.sblas_hip_krylov_update_f64.argtypes = [C.c_int, vp, C.c_int, C.c_int, i64, vp, C.POINTER(vp), C.c_int, vp]
    L.sblas_hip_krylov_plan_create.restype = C.c_int
    L.sblas_hip_krylov_plan_create.argtypes = [C.c_int, vp, C.c_int, i64, i64, vp, vp, vp, C.c_int, vp, vp, C.POINTER(vp)]
    L.sblas_hip_krylov_plan_info.restype = C.c_int
    L.sblas_hip_krylov_plan_info.argtypes = [vp, C.POINTER(i64)]
    L.sblas_hip_krylov_plan_destroy.restype = C.c_int
    L.sblas_hip_krylov_plan_destroy.argtypes = [vp]
    L.sblas_hip_krylov_start.restype = C.c_int
    L.sblas_hip_krylov_start.argtypes = [vp, vp, vp, vp, vp, vp, f64, f64, i64]
    L.sblas_hip_krylov_iterate.restype = C.c_int
    L.sblas_hip_krylov_iterate.argtypes = [vp, vp, i64]
    L.sblas_hip_krylov_status.restype = C.c_int
    L.sblas_hip_krylov_status.argtypes = [vp, vp, C.POINTER(f64)]
    L.sblas_gmres_limits.restype = C.c_int
    L.sblas_gmres_limits.argtypes = [C.POINTER(i64)]
    L.sblas_gmres_step_ref.restype = C.c_int
    L.sblas_gmres_step_ref.argtypes = [C.c_int, vp, f64, vp, vp, vp, vp, f64, i64, C.POINTER(i64), C.POINTER(f64), C.POINTER(i64)]
    L.sblas_gmres_solve_ref.restype = C.c_int
    L.sblas_gmres_solve_ref.argtypes = [C.c_int, vp, C.c_int, vp, vp]
    L.sblas_gmres_launches.restype = i64
    L.sblas_gmres_launches.argtypes = [C.c_int, C.c_int, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)]
    L.sblas_hip_gmres_dots_workspace.restype = sz
    L.sblas_hip_gmres_dots_workspace.argtypes = [i64, C.c_int]
    L.sblas_hip_gmres_dots_f64.restype = C.c_int
    L.sblas_hip_gmres_dots_f64.argtypes = [C.c_int, vp, i64, C.c_int, vp, i64, vp, vp, vp, sz]
    L.sblas_hip_gmres_project_f64.restype = C.c_int
    L.sblas_hip_gmres_project_f64.argtypes = [C.c_int, vp, i64, C.c_int, vp, i64, vp, vp, vp]
    L.sblas_hip_gmres_combine_f64.restype = C.c_int
    L.sblas_hip_gmres_combine_f64.argtypes = [C.c_int, vp, i64, C.c_int, vp, i64, vp, vp]
    L.sblas_hip_gmres_plan_create.restype = C.c_int
    L.sblas_hip_gmres_plan_create.argtypes = [C.c_int, vp, i64, i64, vp, vp, C.c_int, vp, C.c_int, vp, vp, C.POINTER(vp)]
    L.sblas_hip_gmres_plan_info.restype = C.c_int
    L.sblas_hip_gmres_plan_info.argtypes = [vp, C.POINTER(i64)]
    L.sblas_hip_gmres_plan_destroy.restype = C.c_int
    L.sblas_hip_gmres_plan_destroy.argtypes = [vp]
    L.sblas_hip_gmres_start.restype = C.c_int
    L.sblas_hip_gmres_start.argtypes = [vp, vp, vp, vp, vp, vp, f64, f64, i64]
    L.sblas_hip_gmres_iterate.restype = C.c_int
    L.sblas_hip_gmres_iterate.argtypes = [vp, vp, i64]
    L.sblas_hip_gmres_status.restype = C.c_int
    L.sblas_hip_gmres_status.argtypes = [vp, vp, C.POINTER(f64)]
    L.sblas_amg_limits.restype = C.c_int
    L.sblas_amg_limits.argtypes = [C.POINTER(i64)]
    L.sblas_amg_aggregate.restype = C.c_int
    L.sblas_amg_aggregate.argtypes = [i64, vp, vp, vp, f64, C.c_uint32, C.c_uint32, vp, vp, vp, C.POINTER(i64), C.POINTER(i64)]
    L.sblas_amg_launches.restype = i64
    L.sblas_amg_launches.argtypes = [C.c_int, C.c_int, C.c_int]
    L.sblas_amg_wd_ref.restype = C.c_int
    L.sblas_amg_wd_ref.argtypes = [i64, vp, vp, vp, C.c_int, f64, vp, C.POINTER(i64)]
    L.sblas_amg_cycle_ref.restype = C.c_int
    L.sblas_amg_cycle_ref.argtypes = [C.c_int, C.POINTER(i64)] + [C.POINTER(vp)] * 7 + [C.c_int, C.c_int, f64, vp, vp]
    L.sblas_hip_amg_plan_create.restype = C.c_int
    L.sblas_hip_amg_plan_create.argtypes = [C.c_int, vp, i64, i64, vp, vp, vp, f64, i64, C.c_int, C.c_uint32, C.POINTER(vp), C.POINTER(i64)]
    L.sblas_hip_amg_plan_info.restype = C.c_int
    L.sblas_hip_amg_plan_info.argtypes = [vp, C.POINTER(i64)]
    L.sblas_hip_amg_plan_level.restype = C.c_int
    L.sblas_hip_amg_plan_level.argtypes = [vp, C.c_int, C.POINTER(i64), C.POINTER(vp)]
    L.sblas_hip_amg_plan_setup.restype = C.c_int
    L.sblas_hip_amg_plan_setup.argtypes = [vp, vp, vp, C.c_int, f64, C.c_int, C.c_int, f64]
    L.sblas_hip_amg_plan_apply.restype = C.c_int
    L.sblas_hip_amg_plan_apply.argtypes = [vp, vp, vp, vp]
    L.sblas_hip_amg_plan_check.restype = C.c_int
    L.sblas_hip_amg_plan_check.argtypes = [vp, vp, C.POINTER(i64)]
    L.sblas_hip_amg_plan_speaks_for.restype = C.c_int
    L.sblas_hip_amg_plan_speaks_for.argtypes = [vp, C.c_int, i64, i64, vp, vp]
    L.sblas_hip_amg_plan_destroy.restype = C.c_int
    L.sblas_hip_amg_plan_destroy.argtypes = [vp]
    L.sblas_hip_amg_sweep_f64.restype = C.c_int
    L.sblas_hip_amg_sweep_f64.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, vp]
    L.sblas_hip_amg_restrict_f64.restype = C.c_int
    L.sblas_hip_amg_restrict_f64.argtypes = [vp, vp, C.c_int, vp, vp]
    L.sblas_hip_amg_prolong_f64.restype = C.c_int
    L.sblas_hip_amg_prolong_f64.argtypes = [vp, vp, C.c_int, f64, vp, vp]
    L.sblas_amg_keep_level.restype = C.c_int
    L.sblas_amg_keep_level.argtypes = [i64, i64, f64]
    L.sblas_amg_prolongator_ref.restype = C.c_int
    L.sblas_amg_prolongator_ref.argtypes = [i64, vp, vp, vp, vp, i64, f64, vp, vp, vp, C.POINTER(i64), C.POINTER(i64)]
    L.sblas_amg_transfer_ref.restype = C.c_int
    L.sblas_amg_transfer_ref.argtypes = [C.c_int, i64, vp, vp, vp, f64, vp, vp]
    L.sblas_amg_cycle_sa_ref.restype = C.c_int
    L.sblas_amg_cycle_sa_ref.argtypes = [C.c_int, C.POINTER(i64)] + [C.POINTER(vp)] * 10 + [C.c_int, C.c_int, f64, vp, vp]
    L.sblas_hip_amg_plan_create_ex.restype = C.c_int
    L.sblas_hip_amg_plan_create_ex.argtypes = [C.c_int, vp, i64, i64, vp, vp, vp, f64, i64, C.c_int, C.c_uint32, C.c_int, f64, f64,
                                               C.POINTER(vp), C.POINTER(i64)]
    L.sblas_hip_amg_plan_transfer.restype = C.c_int
    L.sblas_hip_amg_plan_transfer.argtypes = [vp, C.c_int, C.POINTER(i64), C.POINTER(vp)]
    L.sblas_hip_amg_plan_options.restype = C.c_int
    L.sblas_hip_amg_plan_options.argtypes = [vp, C.POINTER(f64)]
    L.sblas_hip_amg_pvalues_f64.restype = C.c_int
    L.sblas_hip_amg_pvalues_f64.argtypes = [vp, vp, C.c_int, vp, vp]
    L.sblas_amg_roots_rounds_ref.restype = C.c_int
    L.sblas_amg_roots_rounds_ref.argtypes = [i64, vp, vp, vp, f64, C.c_uint32, C.c_uint32, vp, C.POINTER(i64), C.POINTER(i64)]
    L.sblas_hip_amg_aggregate_workspace.restype = sz
    L.sblas_hip_amg_aggregate_workspace.argtypes = [i64, i64]
    L.sblas_hip_amg_aggregate_i32.restype = C.c_int
    L.sblas_hip_amg_aggregate_i32.argtypes = [C.c_int, vp, i64, i64, vp, vp, vp, f64, C.c_uint32, C.c_uint32, vp, vp, vp, vp, sz,
                                              C.POINTER(i64), C.POINTER(i64)]
    L.sblas_hip_amg_plan_create_dev.restype = C.c_int
    L.sblas_hip_amg_plan_create_dev.argtypes = [C.c_int, vp, i64, i64, vp, vp, vp, f64, i64, C.c_int, C.c_uint32, C.c_int, f64, f64, C.c_int,
                                                C.POINTER(vp), C.POINTER(i64)]
    u32 = C.c_uint32
    L.sblas_cheby_limits.restype = C.c_int
    L.sblas_cheby_limits.argtypes = [C.POINTER(i64)]
    L.sblas_cheby_start_ref.restype = C.c_int
    L.sblas_cheby_start_ref.argtypes = [i64, u32, u32, vp]
    L.sblas_cheby_lanczos_ref.restype = C.c_int
    L.sblas_cheby_lanczos_ref.argtypes = [i64, vp, vp, vp, u32, u32, C.c_int, vp, vp, C.POINTER(i64), C.POINTER(i64)]
    L.sblas_cheby_ritz_ref.restype = C.c_int
    L.sblas_cheby_ritz_ref.argtypes = [C.c_int, vp, vp, vp, vp, C.POINTER(f64)]
    L.sblas_cheby_rowbound_ref.restype = C.c_int
    L.sblas_cheby_rowbound_ref.argtypes = [i64, vp, vp, vp, C.POINTER(f64), C.POINTER(i64)]
    L.sblas_cheby_lambda_ref.restype = f64
    L.sblas_cheby_lambda_ref.argtypes = [i64, f64, f64, f64]
    L.sblas_cheby_coef_ref.restype = C.c_int
    L.sblas_cheby_coef_ref.argtypes = [f64, f64, C.c_int, vp, C.POINTER(f64)]
    L.sblas_cheby_apply_ref.restype = C.c_int
    L.sblas_cheby_apply_ref.argtypes = [i64, vp, vp, vp, vp, C.c_int, vp, vp, vp, C.POINTER(i64)]
    L.sblas_hip_cheby_plan_create.restype = C.c_int
    L.sblas_hip_cheby_plan_create.argtypes = [C.c_int, vp, i64, i64, vp, vp, C.c_int, C.c_int, f64, f64, u32, C.POINTER(vp), C.POINTER(i64)]
    L.sblas_hip_cheby_plan_setup.restype = C.c_int
    L.sblas_hip_cheby_plan_setup.argtypes = [vp, vp, vp, f64]
    L.sblas_hip_cheby_plan_apply.restype = C.c_int
    L.sblas_hip_cheby_plan_apply.argtypes = [vp, vp, vp, vp]
    L.sblas_hip_cheby_plan_smooth.restype = C.c_int
    L.sblas_hip_cheby_plan_smooth.argtypes = [vp, vp, vp, vp, vp]
    L.sblas_hip_cheby_plan_check.restype = C.c_int
    L.sblas_hip_cheby_plan_check.argtypes = [vp, vp, C.POINTER(f64)]
    L.sblas_hip_cheby_plan_scalars.restype = C.c_int
    L.sblas_hip_cheby_plan_scalars.argtypes = [vp, vp, vp, vp, vp]
    L.sblas_hip_cheby_plan_info.restype = C.c_int
    L.sblas_hip_cheby_plan_info.argtypes = [vp, C.POINTER(i64)]
    L.sblas_hip_cheby_plan_speaks_for.restype = C.c_int
    L.sblas_hip_cheby_plan_speaks_for.argtypes = [vp, C.c_int, i64, i64, vp, vp]
    L.sblas_hip_cheby_plan_destroy.restype = C.c_int
    L.sblas_hip_cheby_plan_destroy.argtypes = [vp]
    L.sblas_hip_amg_plan_setup_ex.restype = C.c_int
    L.sblas_hip_amg_plan_setup_ex.argtypes = [vp, vp, vp, C.c_int, f64, C.c_int, C.c_int, f64, C.c_int, C.c_int, f64, f64]
    L.sblas_hip_amg_plan_eig.restype = C.c_int
    L.sblas_hip_amg_plan_eig.argtypes = [vp, vp, C.c_int, C.POINTER(f64), vp, C.POINTER(C.c_int)]
    L.sblas_amg_launches_cheb.restype = i64
    L.sblas_amg_launches_cheb.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
    L.sblas_amg_cycle_cheb_ref.restype = C.c_int
    L.sblas_amg_cycle_cheb_ref.argtypes = [C.c_int, C.POINTER(i64)] + [C.POINTER(vp)] * 8 + [C.c_int, C.c_int, C.c_int, f64, vp, vp]
    L.sblas_amg_cycle_cheb_sa_ref.restype = C.c_int
    L.sblas_amg_cycle_cheb_sa_ref.argtypes = [C.c_int, C.POINTER(i64)] + [C.POINTER(vp)] * 11 + [C.c_int, C.c_int, C.c_int, f64, vp, vp]
    L.sblas_krylov_multi_limits.restype = C.c_int
    L.sblas_krylov_multi_limits.argtypes = [C.POINTER(i64)]
    L.sblas_krylov_multi_precond_ok.restype = C.c_int
    L.sblas_krylov_multi_precond_ok.argtypes = [C.c_int]
    L.sblas_krylov_multi_launches.restype = i64
    L.sblas_krylov_multi_launches.argtypes = [C.c_int, C.c_int, i64]
    L.sblas_krylov_multi_grid.restype = C.c_int
    L.sblas_krylov_multi_grid.argtypes = [i64, C.c_int, C.POINTER(i64)]
    L.sblas_krylov_scalar_step_ref.restype = C.c_int
    L.sblas_krylov_scalar_step_ref.argtypes = [C.c_int, C.c_int, C.c_int, vp, vp, f64, f64, i64]
    L.sblas_hip_krylov_multi_dot_workspace.restype = sz
    L.sblas_hip_krylov_multi_dot_workspace.argtypes = [i64, C.c_int, C.c_int]
    L.sblas_hip_krylov_multi_dot_f64.restype = C.c_int
    L.sblas_hip_krylov_multi_dot_f64.argtypes = [C.c_int, vp, i64, C.c_int, C.c_int, C.POINTER(vp), C.POINTER(i64), C.POINTER(vp), C.POINTER(i64),
                                                 vp, vp, sz]
    L.sblas_hip_krylov_multi_update_f64.restype = C.c_int
    L.sblas_hip_krylov_multi_update_f64.argtypes = [C.c_int, vp, C.c_int, C.c_int, i64, C.c_int, vp, C.POINTER(vp), C.POINTER(i64), C.c_int, vp]
    L.sblas_hip_krylov_multi_plan_create.restype = C.c_int
    L.sblas_hip_krylov_multi_plan_create.argtypes = [C.c_int, vp, C.c_int, i64, i64, vp, vp, C.c_int, C.c_int, C.POINTER(vp)]
    L.sblas_hip_krylov_multi_plan_info.restype = C.c_int
    L.sblas_hip_krylov_multi_plan_info.argtypes = [vp, C.POINTER(i64)]
    L.sblas_hip_krylov_multi_plan_destroy.restype = C.c_int
    L.sblas_hip_krylov_multi_plan_destroy.argtypes = [vp]
    L.sblas_hip_krylov_multi_start.restype = C.c_int
    L.sblas_hip_krylov_multi_start.argtypes = [vp, vp, vp, vp, vp, i64, vp, i64, f64, f64, i64]
    L.sblas_hip_krylov_multi_iterate.restype = C.c_int
    L.sblas_hip_krylov_multi_iterate.argtypes = [vp, vp, i64]
    L.sblas_hip_krylov_multi_status.restype = C.c_int
    L.sblas_hip_krylov_multi_status.argtypes = [vp, vp, C.POINTER(f64)]
    L.sblas_amg_multi_limits.restype = C.c_int
    L.sblas_amg_multi_limits.argtypes = [C.POINTER(i64)]
    L.sblas_amg_multi_grid.restype = C.c_int
    L.sblas_amg_multi_grid.argtypes = [i64, C.c_int, C.POINTER(i64)]
    L.sblas_krylov_multi_precond_plan_ok.restype = C.c_int
    L.sblas_krylov_multi_precond_plan_ok.argtypes = [C.c_int]
    L.sblas_krylov_multi_launches_ex.restype = i64
    L.sblas_krylov_multi_launches_ex.argtypes = [C.c_int, C.c_int, i64, i64]
    L.sblas_hip_amg_plan_reserve_multi.restype = C.c_int
    L.sblas_hip_amg_plan_reserve_multi.argtypes = [vp, vp, C.c_int]
    L.sblas_hip_amg_plan_multi_info.restype = C.c_int
    L.sblas_hip_amg_plan_multi_info.argtypes = [vp, C.POINTER(i64)]
    L.sblas_hip_amg_plan_apply_multi.restype = C.c_int
    L.sblas_hip_amg_plan_apply_multi.argtypes = [vp, vp, C.c_int, vp, i64, vp, i64]
    L.sblas_hip_amg_sweep_multi_f64.restype = C.c_int
    L.sblas_hip_amg_sweep_multi_f64.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, i64, vp, i64, vp, i64]
    L.sblas_hip_amg_restrict_multi_f64.restype = C.c_int
    L.sblas_hip_amg_restrict_multi_f64.argtypes = [vp, vp, C.c_int, C.c_int, vp, i64, vp, i64]
    L.sblas_hip_amg_prolong_multi_f64.restype = C.c_int
    L.sblas_hip_amg_prolong_multi_f64.argtypes = [vp, vp, C.c_int, f64, C.c_int, vp, i64, vp, i64]
    L.sblas_hip_krylov_multi_plan_create_ex.restype = C.c_int
    L.sblas_hip_krylov_multi_plan_create_ex.argtypes = [C.c_int, vp, C.c_int, i64, i64, vp, vp, C.c_int, C.c_int, vp, C.POINTER(vp)]
    L.sblas_sptrsm_tile_limits.restype = C.c_int
    L.sblas_sptrsm_tile_limits.argtypes = [C.POINTER(i64)]
    L.sblas_sptrsm_tile_grid.restype = C.c_int
    L.sblas_sptrsm_tile_grid.argtypes = [i64, i64, C.POINTER(i64)]
    L.sblas_krylov_multi_precond_pair_ok.restype = C.c_int
    L.sblas_krylov_multi_precond_pair_ok.argtypes = [C.c_int]
    L.sblas_krylov_multi_launches_pair.restype = i64
    L.sblas_krylov_multi_launches_pair.argtypes = [C.c_int, C.c_int, i64, i64, i64]
    L.sblas_hip_sptrsm_tiled_f64_i32_planned.restype = C.c_int
    L.sblas_hip_sptrsm_tiled_f64_i32_planned.argtypes = [vp, vp, vp, vp, vp, i64, f64, vp, i64, vp, i64]
    L.sblas_hip_krylov_multi_plan_create_pair.restype = C.c_int
    L.sblas_hip_krylov_multi_plan_create_pair.argtypes = [C.c_int, vp, C.c_int, i64, i64, vp, vp, C.c_int, vp, vp, C.POINTER(vp)]
    L.sblas_gmres_multi_limits.restype = C.c_int
    L.sblas_gmres_multi_limits.argtypes = [C.POINTER(i64)]
    L.sblas_gmres_multi_grid.restype = C.c_int
    L.sblas_gmres_multi_grid.argtypes = [i64, C.c_int, C.POINTER(i64)]
    L.sblas_gmres_multi_launches.restype = i64
    L.sblas_gmres_multi_launches.argtypes = [C.c_int, C.c_int, i64, i64, i64, C.POINTER(i64)]
    for name in ("sblas_gmres_multi_precond_ok", "sblas_gmres_multi_precond_plan_ok", "sblas_gmres_multi_precond_pair_ok"):
        getattr(L, name).restype = C.c_int
        getattr(L, name).argtypes = [C.c_int]
    L.sblas_hip_gmres_multi_dots_workspace.restype = sz
    L.sblas_hip_gmres_multi_dots_workspace.argtypes = [i64, C.c_int, C.c_int]
    L.sblas_hip_gmres_multi_dots_f64.restype = C.c_int
    L.sblas_hip_gmres_multi_dots_f64.argtypes = [C.c_int, vp, i64, C.c_int, C.c_int, vp, i64, i64, vp, i64, vp, vp, vp, sz]
    L.sblas_hip_gmres_multi_project_f64.restype = C.c_int
    L.sblas_hip_gmres_multi_project_f64.argtypes = [C.c_int, vp, i64, C.c_int, C.c_int, vp, i64, i64, vp, i64, vp, i64, vp, vp]
    L.sblas_hip_gmres_multi_combine_f64.restype = C.c_int
    L.sblas_hip_gmres_multi_combine_f64.argtypes = [C.c_int, vp, i64, C.c_int, C.c_int, vp, i64, i64, vp, i64, vp, i64, vp]
    L.sblas_hip_gmres_multi_plan_create.restype = C.c_int
    L.sblas_hip_gmres_multi_plan_create.argtypes = [C.c_int, vp, i64, i64, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, C.POINTER(vp)]
    L.sblas_hip_gmres_multi_plan_info.restype = C.c_int
    L.sblas_hip_gmres_multi_plan_info.argtypes = [vp, C.POINTER(i64)]
    L.sblas_hip_gmres_multi_plan_block.restype = C.c_int
    L.sblas_hip_gmres_multi_plan_block.argtypes = [vp, vp, C.c_int, vp]
    L.sblas_hip_gmres_multi_plan_destroy.restype = C.c_int
    L.sblas_hip_gmres_multi_plan_destroy.argtypes = [vp]
    L.sblas_hip_gmres_multi_start.restype = C.c_int
    L.sblas_hip_gmres_multi_start.argtypes = [vp, vp, vp, vp, vp, i64, vp, i64, f64, f64, i64]
    L.sblas_hip_gmres_multi_iterate.restype = C.c_int
    L.sblas_hip_gmres_multi_iterate.argtypes = [vp, vp, i64]
    L.sblas_hip_gmres_multi_status.restype = C.c_int
    L.sblas_hip_gmres_multi_status.argtypes = [vp, vp, C.POINTER(f64)]
    L.sblas_geam_check_nnz.restype = C.c_int
    L.sblas_geam_check_nnz.argtypes = [i64]
    L.sblas_geam_ref.restype = C.c_int
    L.sblas_geam_ref.argtypes = [i64, i64, vp, vp, vp, vp, vp, vp, f64, f64, vp, vp, vp, vp, vp, C.POINTER(i64)]
    L.sblas_hip_geam_plan_create.restype = C.c_int
    L.sblas_hip_geam_plan_create.argtypes = [C.c_int, vp, i64, i64, vp, vp, vp, vp, C.c_int, C.POINTER(vp)]
    L.sblas_hip_geam_plan_info.restype = C.c_int
    L.sblas_hip_geam_plan_info.argtypes = [vp, C.POINTER(i64)]
    L.sblas_hip_geam_plan_csr.restype = C.c_int
    L.sblas_hip_geam_plan_csr.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
    L.sblas_hip_geam_plan_maps.restype = C.c_int
    L.sblas_hip_geam_plan_maps.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
    L.sblas_hip_geam_plan_numeric.restype = C.c_int
    L.sblas_hip_geam_plan_numeric.argtypes = [vp, vp, vp, vp, f64, f64, vp]
    L.sblas_hip_geam_plan_destroy.restype = C.c_int
    L.sblas_hip_geam_plan_destroy.argtypes = [vp]
    L.sblas_mspgemm_limits.restype = C.c_int
    L.sblas_mspgemm_limits.argtypes = [C.POINTER(i64)]
    L.sblas_mspgemm_ref.restype = C.c_int
    L.sblas_mspgemm_ref.argtypes = [i64, i64, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.sblas_hip_mspgemm_plan_create.restype = C.c_int
    L.sblas_hip_mspgemm_plan_create.argtypes = [C.c_int, vp, i64, i64, i64, vp, vp, vp, vp, vp, vp, C.c_int, C.POINTER(vp)]
    L.sblas_hip_mspgemm_plan_info.restype = C.c_int
    L.sblas_hip_mspgemm_plan_info.argtypes = [vp, C.POINTER(i64)]
    L.sblas_hip_mspgemm_plan_numeric.restype = C.c_int
    L.sblas_hip_mspgemm_plan_numeric.argtypes = [vp, vp, vp, vp, vp]
    L.sblas_hip_mspgemm_plan_destroy.restype = C.c_int
    L.sblas_hip_mspgemm_plan_destroy.argtypes = [vp]
    L.sblas_sddmm_narrow_limits.restype = C.c_int
    L.sblas_sddmm_narrow_limits.argtypes = [C.POINTER(i64)]
    for fn in (L.sblas_sddmm_narrow_ref, L.sblas_hip_sddmm_narrow_f64_i32):
        fn.restype = C.c_int
        fn.argtypes = [C.c_int, vp, i64, i64, i64, vp, vp, vp, i64, vp, i64, C.c_int, f64, f64, C.c_int, vp]
    L.sblas_fsai_limits.restype = C.c_int
    L.sblas_fsai_limits.argtypes = [C.POINTER(i64)]
    L.sblas_fsai_pattern.restype = C.c_int
    L.sblas_fsai_pattern.argtypes = [i64, vp, vp, i64, vp, vp, C.c_int, vp, vp, C.POINTER(i64)]
    L.sblas_fsai_ref.restype = C.c_int
    L.sblas_fsai_ref.argtypes = [i64, vp, vp, vp, vp, vp, vp, C.POINTER(i64)]
    L.sblas_hip_fsai_plan_create.restype = C.c_int
    L.sblas_hip_fsai_plan_create.argtypes = [C.c_int, vp, i64, i64, vp, vp, i64, vp, vp, C.c_int, C.POINTER(vp), C.POINTER(i64)]
    L.sblas_hip_fsai_plan_setup.restype = C.c_int
    L.sblas_hip_fsai_plan_setup.argtypes = [vp, vp, vp]
    L.sblas_hip_fsai_plan_apply.restype = C.c_int
    L.sblas_hip_fsai_plan_apply.argtypes = [vp, vp, vp, vp]
    L.sblas_hip_fsai_plan_check.restype = C.c_int
    L.sblas_hip_fsai_plan_check.argtypes = [vp, vp, C.POINTER(i64)]
    L.sblas_hip_fsai_plan_csr.restype = C.c_int
    L.sblas_hip_fsai_plan_csr.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    L.sblas_hip_fsai_plan_info.restype = C.c_int
    L.sblas_hip_fsai_plan_info.argtypes = [vp, C.POINTER(i64)]
    L.sblas_hip_fsai_plan_speaks_for.restype = C.c_int
    L.sblas_hip_fsai_plan_speaks_for.argtypes = [vp, C.c_int, i64, i64, vp, vp]
    L.sblas_hip_fsai_plan_destroy.restype = C.c_int
    L.sblas_hip_fsai_plan_destroy.argtypes = [vp]
    L.sblas_eigsh_limits.restype = C.c_int
    L.sblas_eigsh_limits.argtypes = [C.POINTER(i64)]
    L.sblas_eigsh_sizes.restype = C.c_int
    L.sblas_eigsh_sizes.argtypes = [i64, C.c_int, C.c_int, C.c_int, C.POINTER(i64)]
    L.sblas_eigsh_launches.restype = i64
    L.sblas_eigsh_launches.argtypes = [C.c_int, C.c_int, C.POINTER(i64)]
    L.sblas_eigsh_jacobi_ref.restype = C.c_int
    L.sblas_eigsh_jacobi_ref.argtypes = [C.c_int, vp, C.c_int, vp, vp, C.c_int, C.POINTER(C.c_int)]
    L.sblas_eigsh_ritz_ref.restype = C.c_int
    L.sblas_eigsh_ritz_ref.argtypes = [C.c_int, C.c_int, C.c_int, vp, vp]
    L.sblas_eigsh_step_ref.restype = C.c_int
    L.sblas_eigsh_step_ref.argtypes = [C.c_int, vp, f64, vp, vp]
    L.sblas_eigsh_rotate_ref.restype = C.c_int
    L.sblas_eigsh_rotate_ref.argtypes = [i64, C.c_int, C.c_int, vp, i64, vp, C.c_int]
    L.sblas_hip_eigsh_rotate_f64.restype = C.c_int
    L.sblas_hip_eigsh_rotate_f64.argtypes = [C.c_int, vp, i64, C.c_int, C.c_int, vp, i64, vp, C.c_int]
    L.sblas_hip_eigsh_ritz_f64.restype = C.c_int
    L.sblas_hip_eigsh_ritz_f64.argtypes = [C.c_int, vp, C.c_int, C.c_int, C.c_int, vp, vp]
    L.sblas_hip_eigsh_plan_create.restype = C.c_int
    L.sblas_hip_eigsh_plan_create.argtypes = [C.c_int, vp, i64, i64, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, u32, C.POINTER(vp)]
    L.sblas_hip_eigsh_start.restype = C.c_int
    L.sblas_hip_eigsh_start.argtypes = [vp, vp, vp, vp, f64, f64, i64]
    L.sblas_hip_eigsh_iterate.restype = C.c_int
    L.sblas_hip_eigsh_iterate.argtypes = [vp, vp, i64]
    L.sblas_hip_eigsh_status.restype = C.c_int
    L.sblas_hip_eigsh_status.argtypes = [vp, vp, C.POINTER(f64), vp, vp]
    L.sblas_hip_eigsh_values.restype = C.c_int
    L.sblas_hip_eigsh_values.argtypes = [vp, vp, vp]
    L.sblas_hip_eigsh_vectors.restype = C.c_int
    L.sblas_hip_eigsh_vectors.argtypes = [vp, C.POINTER(vp), C.POINTER(i64)]
    L.sblas_hip_eigsh_info.restype = C.c_int
    L.sblas_hip_eigsh_info.argtypes = [vp, C.POINTER(i64)]
    L.sblas_hip_eigsh_destroy.restype = C.c_int
    L.sblas_hip_eigsh_destroy.argtypes = [vp]
    _lib = L
    return L


def check(rc, what):
    if rc != 0:
        raise SblasError("%s failed: %s (code %d)" % (what, lib().sblas_hip_error_string(rc).decode(), rc))


# ------------------------------------------------------------------------------------------
# host-side pure functions
# ------------------------------------------------------------------------------------------
def read_mtx(path):
    """MatrixMarket -> (rows, cols, nnz, symmetric, rowptr[int32], colidx[int32], val[float64])."""
    L = lib()
    r, c, z, s = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
    check(L.sblas_mm_read_info(os.fsencode(path), C.byref(r), C.byref(c), C.byref(z), C.byref(s)), "sblas_mm_read_info")
    rowptr = np.zeros(r.value + 1, np.int32)
    colidx = np.zeros(max(z.value, 1), np.int32)
    val = np.zeros(max(z.value, 1), np.float64)
    check(L.sblas_mm_read_csr(os.fsencode(path), rowptr.ctypes.data, colidx.ctypes.data, val.ctypes.data), "sblas_mm_read_csr")
    return r.value, c.value, z.value, s.value, rowptr, colidx[:z.value], val[:z.value]


def rand0to1(count, seed=211):
    """The reference's dense initialiser (DenseMatrix ctor, matrix.h:519-528): srand(seed), rand() / RAND_MAX."""
    out = np.empty(int(count), np.float64)
    check(lib().sblas_host_fill_rand0to1(out.ctypes.data, int(count), seed), "sblas_host_fill_rand0to1")
    return out


def find_row_of_nnz(rowptr, nnz_idx):
    rowptr = np.ascontiguousarray(rowptr, np.int32)
    return int(lib().sblas_find_row_of_nnz(rowptr.ctypes.data, len(rowptr) - 1, int(nnz_idx)))


def partition_nnz(rowptr, n_gpu, i_gpu):
    """-> dict(start_row, stop_row, nnz, first_nnz, rowptr) of GPU i's nnz-balanced row block."""
    rowptr = np.ascontiguousarray(rowptr, np.int32)
    rows = len(rowptr) - 1
    nnz = int(rowptr[-1])
    s, e, k, f = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int64()
    buf = np.zeros(rows + 2, np.int32)
    num = lib().sblas_partition_nnz(rowptr.ctypes.data, rows, nnz, n_gpu, i_gpu, C.byref(s), C.byref(e),
                                    C.byref(k), C.byref(f), buf.ctypes.data)
    if num < 0:
        raise SblasError("sblas_partition_nnz failed (%d)" % num)
    return dict(start_row=s.value, stop_row=e.value, nnz=k.value, first_nnz=f.value, rowptr=buf[:num].copy())


# kinds of the SpMV plan's work items (SBLAS_SPMV_ITEM_* in sblas_hip.h) and its default split parameters
SPMV_ITEM_LPR, SPMV_ITEM_STREAM4096, SPMV_ITEM_STREAM6144, SPMV_ITEM_SEG = 0, 1, 2, 3
SPMV_ITEM_LDS_S2, SPMV_ITEM_LDS_S3, SPMV_ITEM_LDS_S4, SPMV_ITEM_LDS_S7, SPMV_ITEM_SPLIT = 4, 5, 6, 7, 8
SPMV_SPLIT_MIN, SPMV_SPLIT_PIECE = 12288, 4096


def spmv_plan_classify(rowptr, nnz=None, split_min=0, piece=0):
    """The SpMV plan's work items (sblas_spmv_plan_classify) as an (n, 4) int32 array of
    (first row, row count, kind, pieces); nnz defaults to rowptr[-1]."""
    rowptr = np.ascontiguousarray(rowptr, np.int32)
    rows = len(rowptr) - 1
    nnz = int(rowptr[-1]) if nnz is None else int(nnz)
    L = lib()
    n = L.sblas_spmv_plan_classify(rowptr.ctypes.data, rows, nnz, split_min, piece, None, 0)
    if n < 0:
        raise SblasError("sblas_spmv_plan_classify refused the row pointers")
    out = np.zeros((max(n, 1), 4), np.int32)
    if L.sblas_spmv_plan_classify(rowptr.ctypes.data, rows, nnz, split_min, piece, out.ctypes.data, n) != n:
        raise SblasError("sblas_spmv_plan_classify changed its answer")
    return out[:n]


# the split SpMM plan's default parameters (SBLAS_SPMM_SPLIT_* in sblas_hip.h)
SPMM_SPLIT_MIN, SPMM_SPLIT_PIECE = 16384, 4096


def spmm_split_classify(rowptr, nnz=None, split_min=0, piece=0, direct_mask=None, panel_rows=0):
    """The split SpMM plan's classifier (sblas_spmm_split_classify): (pieces, split_rows), int32 arrays of shape (P, 4)
    {row, first nonzero, end, partial slot} and (S, 4) {row, first slot, pieces, -1}.  direct_mask: one flag per panel
    of panel_rows rows (None: every panel); nnz defaults to rowptr[-1]."""
    rowptr = np.ascontiguousarray(rowptr, np.int32)
    rows = len(rowptr) - 1
    nnz = int(rowptr[-1]) if nnz is None else int(nnz)
    mask = None if direct_mask is None else np.ascontiguousarray(np.asarray(direct_mask) != 0, np.uint8).ravel()
    if mask is not None and (panel_rows <= 0 or len(mask) < (rows + panel_rows - 1) // panel_rows):
        raise SblasError("direct_mask needs one entry per panel of panel_rows rows (%d rows)" % rows)
    mptr = mask.ctypes.data if mask is not None else None
    L = lib()
    n = L.sblas_spmm_split_classify(rowptr.ctypes.data, rows, nnz, split_min, piece, mptr, panel_rows, None, 0)
    if n < 0:
        raise SblasError("sblas_spmm_split_classify refused its arguments")
    out = np.zeros((max(n, 1), 4), np.int32)
    if L.sblas_spmm_split_classify(rowptr.ctypes.data, rows, nnz, split_min, piece, mptr, panel_rows, out.ctypes.data, n) != n:
        raise SblasError("sblas_spmm_split_classify changed its answer")
    out = out[:n]
    n_pieces = int(np.count_nonzero(out[:, 3] >= 0))
    return out[:n_pieces], out[n_pieces:]


# the fields of sblas_spmm_rule_describe, in the order of the SBLAS_SPMM_RULE_* / SBLAS_SPMM_RULE_PLAN_* enums of sblas_hip.h
SPMM_RULE_FIELDS = (
    "staging", "verdicts", "panel_rows", "groups", "panels", "plannable",
    "tiled", "tiled_g", "w6_nh", "w6_grid_y", "lanes_nc", "lanes_cp", "lanes_lpe",
    "mfma", "mfma_batch", "mfma_lds_floor",
    "four_rows", "four_rows_waves", "four_rows_voted", "merge", "dpp_groups", "dpp_pad", "dpp_long", "narrow", "rows8",
    "interleave", "skip", "split_groups")
SPMM_RULE_PLAN_FIELDS = ("n_window", "n_direct", "n_mfma_w", "n_mfma_d", "merge", "four_rows", "n_split", "panel_rows", "groups")


def spmm_rule(rows, cols, nnz, ldbt, n=None, ncu=256, caller_staged=False, plan=None):
    """The SpMM kernel rule (sblas_spmm_rule_describe; no GPU): what one column chunk of these sizes stages, classifies
    and launches, as a dict over SPMM_RULE_FIELDS.  n defaults to ldbt; plan: None for an unplanned call, else a dict over
    SPMM_RULE_PLAN_FIELDS (missing counts are 0)."""
    n = ldbt if n is None else n
    pl = None
    if plan is not None:
        unknown = set(plan) - set(SPMM_RULE_PLAN_FIELDS)
        if unknown:
            raise SblasError("spmm_rule: unknown plan fields %s" % sorted(unknown))
        pl = np.array([int(plan.get(k, 0)) for k in SPMM_RULE_PLAN_FIELDS], np.int64)
    out = np.zeros(len(SPMM_RULE_FIELDS), np.int64)
    got = lib().sblas_spmm_rule_describe(rows, cols, nnz, ldbt, n, ncu, int(bool(caller_staged)),
                                         None if pl is None else pl.ctypes.data, out.ctypes.data, len(out))
    if got != len(out):
        raise SblasError("sblas_spmm_rule_describe refused its arguments" if got < 0 else
                         "sblas_spmm_rule_describe has %d fields, SPMM_RULE_FIELDS %d" % (got, len(out)))
    return dict(zip(SPMM_RULE_FIELDS, out.tolist()))


# SpGEMM: plan flags and the host rule's row paths (SBLAS_SPGEMM_* in sblas_hip.h)
SPGEMM_AUTO, SPGEMM_GENERAL = 0, 1
SPGEMM_PATH_EMPTY, SPGEMM_PATH_ROW, SPGEMM_PATH_GENERAL = 0, 1, 2


def spgemm_limits():
    """The SpGEMM plan's limits (sblas_hip_spgemm_limits): dict(s_max, acc_cap, chunk_cap)."""
    out = (C.c_int64 * 4)()
    check(lib().sblas_hip_spgemm_limits(out), "sblas_hip_spgemm_limits")
    return dict(s_max=int(out[0]), acc_cap=int(out[1]), chunk_cap=int(out[2]))


def spgemm_classify(products, span, b_ascending=True, general=False, chunk_cap=0):
    """The SpGEMM plan's host rule (sblas_hip_spgemm_classify) -> (path, chunk_first): path[i] is SPGEMM_PATH_EMPTY, _ROW
    or _GENERAL for row i; chunk c holds the general rows, numbered in row order, chunk_first[c] .. chunk_first[c + 1] - 1.
    products and span are per-row int64 counts."""
    products = np.ascontiguousarray(products, np.int64)
    span = np.ascontiguousarray(span, np.int64)
    m = len(products)
    if len(span) != m:
        raise SblasError("span has %d entries, products %d" % (len(span), m))
    path = np.zeros(max(m, 1), np.uint8)
    chunk_first = np.zeros(m + 1, np.int64)
    n = C.c_int64()
    rc = lib().sblas_hip_spgemm_classify(m, products.ctypes.data, span.ctypes.data, 1 if b_ascending else 0,
                                         SPGEMM_GENERAL if general else SPGEMM_AUTO, int(chunk_cap), path.ctypes.data,
                                         chunk_first.ctypes.data, C.byref(n))
    check(rc, "sblas_hip_spgemm_classify")
    return path[:m], chunk_first[:n.value + 1].copy()


def spgemm_group_width(products, a_len, span):
    """Lanes that own a row-path row (sblas_hip_spgemm_group_width): 16 or 64."""
    return int(lib().sblas_hip_spgemm_group_width(int(products), int(a_len), int(span)))


def spgemm_check_nnz(nnz_c):
    """The return code of the plan's check on the counted nnz(C) (0: it fits an int32 index)."""
    return int(lib().sblas_hip_spgemm_check_nnz(int(nnz_c)))


GEAM_AUTO, GEAM_GENERAL, GEAM_SCATTER = 0, 1, 2
GEAM_PATH_SORTED, GEAM_PATH_GENERAL = 0, 1


def geam_check_nnz(nnz_c):
    """0 when nnz_c fits an int32 index, else the library's invalid-argument code (sblas_geam_check_nnz)."""
    return int(lib().sblas_geam_check_nnz(int(nnz_c)))


def geam_ref(rows, cols, rowptr_a, colidx_a, val_a, rowptr_b, colidx_b, val_b, alpha=1.0, beta=1.0):
    """The GEAM contract as the library's scalar loop over numpy arrays (sblas_geam_ref; no GPU) -> (rowptr_c, colidx_c,
    val_c, dest_a, dest_b): C = alpha * A + beta * B with A's terms of a row before B's, and the entry of C where each
    input entry lands."""
    rpa, rpb = np.ascontiguousarray(rowptr_a, np.int32), np.ascontiguousarray(rowptr_b, np.int32)
    cia, cib = np.ascontiguousarray(colidx_a, np.int32), np.ascontiguousarray(colidx_b, np.int32)
    va, vb = np.ascontiguousarray(val_a, np.float64), np.ascontiguousarray(val_b, np.float64)
    if len(rpa) != rows + 1 or len(rpb) != rows + 1:
        raise SblasError("rowptr_a and rowptr_b need rows + 1 = %d entries" % (rows + 1))
    if len(va) != len(cia) or len(vb) != len(cib):
        raise SblasError("val_a / val_b have %d / %d entries, colidx_a / colidx_b %d / %d" % (len(va), len(vb), len(cia), len(cib)))
    if (rows and (int(rpa[-1]) > len(cia) or int(rpb[-1]) > len(cib))):
        raise SblasError("a rowptr ends beyond its colidx")
    total = len(cia) + len(cib)
    rowptr_c = np.zeros(rows + 1, np.int32)
    colidx_c, val_c = np.zeros(total, np.int32), np.zeros(total, np.float64)
    dest_a, dest_b = np.zeros(len(cia), np.int32), np.zeros(len(cib), np.int32)
    nnz_c = C.c_int64(0)
    ptr = lambda a: a.ctypes.data if a.size else None
    check(lib().sblas_geam_ref(rows, cols, rpa.ctypes.data, ptr(cia), ptr(va), rpb.ctypes.data, ptr(cib), ptr(vb), float(alpha), float(beta),
                               rowptr_c.ctypes.data, ptr(colidx_c), ptr(val_c), ptr(dest_a), ptr(dest_b), C.byref(nnz_c)), "sblas_geam_ref")
    n = int(nnz_c.value)
    return rowptr_c, colidx_c[:n].copy(), val_c[:n].copy(), dest_a, dest_b


MSPGEMM_AUTO, MSPGEMM_GENERAL = 0, 1
MSPGEMM_PATH_SORTED, MSPGEMM_PATH_GENERAL = 0, 1


def mspgemm_limits():
    """The sizes the masked SpGEMM's kernels are built on (sblas_mspgemm_limits): the longest X row a wave stages in LDS
    and the mask entries one workgroup takes."""
    out = (C.c_int64 * 4)()
    check(lib().sblas_mspgemm_limits(out), "sblas_mspgemm_limits")
    return dict(lds_row=int(out[0]), threads=int(out[1]))


def mspgemm_ref(m, n, k, rowptr_m, colidx_m, rowptr_x, colidx_x, val_x, rowptr_y, colidx_y, val_y):
    """The masked SpGEMM contract as the library's scalar loop over numpy arrays (sblas_mspgemm_ref; no GPU) -> out, one
    double per stored mask entry: out = M o (X Y^T) with X m x k, Y n x k and the mask m x n."""
    rpm, rpx, rpy = (np.ascontiguousarray(a, np.int32) for a in (rowptr_m, rowptr_x, rowptr_y))
    cim, cix, ciy = (np.ascontiguousarray(a, np.int32) for a in (colidx_m, colidx_x, colidx_y))
    vx, vy = np.ascontiguousarray(val_x, np.float64), np.ascontiguousarray(val_y, np.float64)
    if len(rpm) != m + 1 or len(rpx) != m + 1 or len(rpy) != n + 1:
        raise SblasError("rowptr_m and rowptr_x need m + 1 = %d entries and rowptr_y n + 1 = %d" % (m + 1, n + 1))
    if len(vx) != len(cix) or len(vy) != len(ciy):
        raise SblasError("val_x / val_y have %d / %d entries, colidx_x / colidx_y %d / %d" % (len(vx), len(vy), len(cix), len(ciy)))
    if int(rpm[-1]) > len(cim) or int(rpx[-1]) > len(cix) or int(rpy[-1]) > len(ciy):
        raise SblasError("a rowptr ends beyond its colidx")
    out = np.zeros(len(cim), np.float64)
    ptr = lambda a: a.ctypes.data if a.size else None
    check(lib().sblas_mspgemm_ref(m, n, k, rpm.ctypes.data, ptr(cim), rpx.ctypes.data, ptr(cix), ptr(vx), rpy.ctypes.data, ptr(ciy), ptr(vy),
                                  ptr(out)), "sblas_mspgemm_ref")
    return out


# the parts of a pattern the narrow SDDMM fills (SBLAS_PART_* in sblas_hip_sddmm_narrow.h)
PART_ALL, PART_LOWER, PART_UPPER, PART_STRICT_LOWER, PART_STRICT_UPPER = 0, 1, 2, 3, 4
_PARTS = {"all": PART_ALL, "lower": PART_LOWER, "upper": PART_UPPER, "strict_lower": PART_STRICT_LOWER, "strict_upper": PART_STRICT_UPPER}


def _part(part):
    if part in _PARTS:
        return _PARTS[part]
    if isinstance(part, int) and not isinstance(part, bool):
        return part                                # the library refuses a number it does not know
    raise SblasError("part must be one of %s, not %r" % (", ".join(repr(p) for p in _PARTS), part))


def sddmm_narrow_limits():
    """The sizes the narrow SDDMM's kernel is built on (sblas_sddmm_narrow_limits): the widest k, the stored entries one
    workgroup takes (a run), the threads of a workgroup and the consecutive entries one lane owns."""
    out = (C.c_int64 * 4)()
    check(lib().sblas_sddmm_narrow_limits(out), "sblas_sddmm_narrow_limits")
    return dict(max_k=int(out[0]), chunk=int(out[1]), threads=int(out[2]), entries_per_lane=int(out[3]))


def sddmm_narrow_ref(rows, cols, rowptr, colidx, X, Y, out=None, alpha=1.0, beta=0.0, part="all"):
    """The narrow SDDMM's contract as the library's scalar loop over numpy arrays (sblas_sddmm_narrow_ref; no GPU) -> out,
    one double per stored entry: alpha * <X[row(e), :k], Y[col(e), :k]> + beta * out[e] inside `part`, +0.0 or beta *
    out[e] outside.  X (rows x k) and Y (cols x k) are read in place when their last axis is contiguous (any row stride
    of at least k), so a slice of a wider array keeps its leading dimension; a 1-D X or Y is k = 1.  beta != 0 needs
    `out`, which is not modified: the result is a new array."""
    rp, ci = np.ascontiguousarray(rowptr, np.int32), np.ascontiguousarray(colidx, np.int32)

    def dense(t, n, what):
        t = np.asarray(t, np.float64)
        if t.ndim == 1:
            t = t.reshape(-1, 1)
        if t.ndim != 2 or t.shape[0] != n:
            raise SblasError("%s must have %d rows, got shape %s" % (what, n, t.shape))
        if t.size and (t.strides[1] != 8 or t.strides[0] % 8 or t.strides[0] < 8 * t.shape[1]) and not (t.shape[0] <= 1 and t.strides[1] == 8):
            t = np.ascontiguousarray(t)
        ld = t.strides[0] // 8 if t.size and t.shape[0] > 1 else max(int(t.shape[1]), 1)
        return t, int(ld)
    X, ldx = dense(X, rows, "X")
    Y, ldy = dense(Y, cols, "Y")
    if X.shape[1] != Y.shape[1]:
        raise SblasError("X and Y must have the same number of columns, got %d and %d" % (X.shape[1], Y.shape[1]))
    if len(rp) != rows + 1 or int(rp[-1]) != len(ci):
        raise SblasError("rowptr needs rows + 1 = %d entries and must end at nnz = %d" % (rows + 1, len(ci)))
    if beta != 0.0 and out is None:
        raise SblasError("beta != 0 needs out")
    res = np.zeros(len(ci), np.float64) if out is None else np.array(out, np.float64).reshape(-1)
    if len(res) != len(ci):
        raise SblasError("out must hold one value per stored entry (%d), got %d" % (len(ci), len(res)))
    ptr = lambda a: a.ctypes.data if a.size else None
    check(lib().sblas_sddmm_narrow_ref(-1, None, rows, cols, len(ci), rp.ctypes.data, ptr(ci), ptr(X), max(ldx, 1), ptr(Y), max(ldy, 1),
                                       int(X.shape[1]), float(alpha), float(beta), _part(part), ptr(res)), "sblas_sddmm_narrow_ref")
    return res


# triangular solves: fill, diagonal, plan modes and launch kinds (SBLAS_FILL_*, SBLAS_DIAG_*, SBLAS_SPTRSV_* in sblas_hip.h)
FILL_LOWER, FILL_UPPER = 0, 1
DIAG_NON_UNIT, DIAG_UNIT = 0, 1
SPTRSV_AUTO, SPTRSV_PER_LEVEL, SPTRSV_CHAIN_ONLY = 0, 1, 2
SPTRSV_LAUNCH_WIDE, SPTRSV_LAUNCH_CHAIN = 0, 1
_SPTRSV_MODE = {"auto": SPTRSV_AUTO, "per_level": SPTRSV_PER_LEVEL, "chain": SPTRSV_CHAIN_ONLY}


def _sptrsv_mode(mode):
    if mode not in _SPTRSV_MODE:
        raise SblasError("mode must be 'auto', 'per_level' or 'chain', not %r" % (mode,))
    return _SPTRSV_MODE[mode]


def _bad_structure(what, rc, bad_row):
    """the SblasError of a refused triangular structure; it names the first bad row and carries it as .bad_row"""
    where = ": row %d" % bad_row if bad_row >= 0 else ""
    err = SblasError("%s failed: %s (code %d)%s" % (what, lib().sblas_hip_error_string(rc).decode(), rc, where))
    err.bad_row = bad_row
    return err


def sptrsv_limits():
    """The triangular solve's limits (sblas_hip_sptrsv_limits): dict(chain_rows, chain_threads, g4_max, g16_max) -- the
    default chain_rows, the chain workgroup's threads, and the longest stored rows that 4 and 16 lanes take."""
    out = (C.c_int64 * 4)()
    check(lib().sblas_hip_sptrsv_limits(out), "sblas_hip_sptrsv_limits")
    return dict(chain_rows=int(out[0]), chain_threads=int(out[1]), g4_max=int(out[2]), g16_max=int(out[3]))


def sptrsv_levels(n, rowptr, colidx, lower=True, unit_diag=False):
    """The level of every row (sblas_sptrsv_levels, host arrays) -> (level, n_levels).  A refused structure raises an
    SblasError whose .bad_row is the first bad row."""
    rowptr = np.ascontiguousarray(rowptr, np.int32)
    colidx = np.ascontiguousarray(colidx, np.int32)
    if len(rowptr) != n + 1:
        raise SblasError("rowptr has %d entries for %d rows" % (len(rowptr), n))
    level = np.zeros(max(n, 1), np.int32)
    n_levels, bad = C.c_int64(), C.c_int64(-1)
    rc = lib().sblas_sptrsv_levels(n, rowptr.ctypes.data, colidx.ctypes.data if len(colidx) else None,
                                   FILL_LOWER if lower else FILL_UPPER, DIAG_UNIT if unit_diag else DIAG_NON_UNIT,
                                   level.ctypes.data, C.byref(n_levels), C.byref(bad))
    if rc != 0:
        raise _bad_structure("sblas_sptrsv_levels", rc, bad.value)
    return level[:n], int(n_levels.value)


def sptrsv_schedule(widths, mode="auto", chain_rows=0):
    """The launches of a solve over levels of the given widths (sblas_sptrsv_schedule) -> (kind, launch_first): launch q
    is SPTRSV_LAUNCH_WIDE or _CHAIN and covers the levels launch_first[q] .. launch_first[q + 1] - 1."""
    widths = np.ascontiguousarray(widths, np.int64)
    L = len(widths)
    kind = np.zeros(max(L, 1), np.uint8)
    first = np.zeros(L + 1, np.int64)
    n = C.c_int64()
    check(lib().sblas_sptrsv_schedule(L, widths.ctypes.data, _sptrsv_mode(mode), int(chain_rows), kind.ctypes.data,
                                      first.ctypes.data, C.byref(n)), "sblas_sptrsv_schedule")
    return kind[:n.value].copy(), first[:n.value + 1].copy()


def sptrsv_pack(n, rowptr, level, n_levels):
    """The lanes of a level plan (sblas_sptrsv_pack, host arrays) -> (perm, level_ptr, level_unit_ptr, unit_row, unit_q):
    the rows by (level, row), where each level's rows and four-lane units begin, and for every unit its row (-1: a pad) and
    its number within the row."""
    rowptr = np.ascontiguousarray(rowptr, np.int32)
    level = np.ascontiguousarray(level, np.int32)
    if len(rowptr) != n + 1 or len(level) != n:
        raise SblasError("rowptr has %d entries and level %d for %d rows" % (len(rowptr), len(level), n))
    args = (n, rowptr.ctypes.data, level.ctypes.data if n else None, n_levels)
    units = C.c_int64()
    check(lib().sblas_sptrsv_pack(*args, None, None, None, None, None, C.byref(units)), "sblas_sptrsv_pack")
    perm, level_ptr, level_unit_ptr = np.zeros(n, np.int32), np.zeros(n_levels + 1, np.int32), np.zeros(n_levels + 1, np.int64)
    unit_row, unit_q = np.zeros(units.value, np.int32), np.zeros(units.value, np.int32)
    check(lib().sblas_sptrsv_pack(*args, *[a.ctypes.data if len(a) else None for a in (perm, level_ptr, level_unit_ptr, unit_row, unit_q)],
                                  C.byref(units)), "sblas_sptrsv_pack")
    return perm, level_ptr, level_unit_ptr, unit_row, unit_q


def ilu0_limits():
    """ILU(0)'s limits (sblas_hip_ilu0_limits): dict(chain_rows, chain_threads, g4_max, g16_max, lds_max, wide_threads) --
    the default chain_rows, the chain workgroup's threads, the longest stored rows that 4 and 16 lanes take, the longest
    row whose working copy lives in LDS, and a wide workgroup's threads."""
    out = (C.c_int64 * 6)()
    check(lib().sblas_hip_ilu0_limits(out), "sblas_hip_ilu0_limits")
    return dict(chain_rows=int(out[0]), chain_threads=int(out[1]), g4_max=int(out[2]), g16_max=int(out[3]), lds_max=int(out[4]),
                wide_threads=int(out[5]))


def ilu0_check(n, rowptr, colidx):
    """ILU(0)'s structure check (sblas_ilu0_check, host arrays) -> the position of every row's diagonal.  Rows must be
    strictly ascending in column and store their diagonal; a refused structure raises an SblasError whose .bad_row is the
    first bad row."""
    rowptr = np.ascontiguousarray(rowptr, np.int32)
    colidx = np.ascontiguousarray(colidx, np.int32)
    if len(rowptr) != n + 1:
        raise SblasError("rowptr has %d entries for %d rows" % (len(rowptr), n))
    diag = np.zeros(max(n, 1), np.int32)
    bad = C.c_int64(-1)
    rc = lib().sblas_ilu0_check(n, rowptr.ctypes.data, colidx.ctypes.data if len(colidx) else None, diag.ctypes.data, C.byref(bad))
    if rc != 0:
        raise _bad_structure("sblas_ilu0_check", rc, bad.value)
    return diag[:n]


def color_limits():
    """The colouring's limits (sblas_hip_color_limits): dict(g4_max, g16_max, window, threads) -- the greatest p (stored
    entries of row v of A plus those of row v of A^T) that 4 and 16 lanes take, the colours one pass of the round kernel
    sees, and a round workgroup's threads."""
    out = (C.c_int64 * 4)()
    check(lib().sblas_hip_color_limits(out), "sblas_hip_color_limits")
    return dict(g4_max=int(out[0]), g16_max=int(out[1]), window=int(out[2]), threads=int(out[3]))


def color_ref(n, rowptr, colidx, seed=0):
    """The colouring rule on host arrays (sblas_csr_color) -> (color, n_colors, sync_rounds): first fit in descending
    h(v) = fmix32(v + 0x9E3779B9 * (seed + 1)), and the rounds of the parallel form when every round sees only the colours
    of the rounds before it.  A refused structure raises an SblasError whose .bad_row is the first bad row."""
    rowptr = np.ascontiguousarray(rowptr, np.int32)
    colidx = np.ascontiguousarray(colidx, np.int32)
    if len(rowptr) != n + 1:
        raise SblasError("rowptr has %d entries for %d rows" % (len(rowptr), n))
    color = np.zeros(max(n, 1), np.int32)
    n_colors, rounds, bad = C.c_int64(), C.c_int64(), C.c_int64(-1)
    rc = lib().sblas_csr_color(n, rowptr.ctypes.data, colidx.ctypes.data if len(colidx) else None, int(seed) & 0xffffffff,
                               color.ctypes.data, C.byref(n_colors), C.byref(rounds), C.byref(bad))
    if rc != 0:
        raise _bad_structure("sblas_csr_color", rc, bad.value)
    return color[:n], int(n_colors.value), int(rounds.value)


# Krylov solvers: methods, preconditioners, status words and the denominators a breakdown names (SBLAS_KRYLOV_*, SBLAS_PRECOND_*)
KRYLOV_PCG, KRYLOV_BICGSTAB = 0, 1
PRECOND_NONE, PRECOND_JACOBI, PRECOND_ILU0, PRECOND_AMG, PRECOND_CHEBYSHEV = 0, 1, 2, 3, 4
PRECOND_FSAI = 6                                                            # SBLAS_PRECOND_FSAI; 5 is no kind
KRYLOV_RUNNING, KRYLOV_CONVERGED, KRYLOV_BREAKDOWN, KRYLOV_LIMIT = 0, 1, 2, 3
KRYLOV_STATUS = {KRYLOV_RUNNING: "running", KRYLOV_CONVERGED: "converged", KRYLOV_BREAKDOWN: "breakdown", KRYLOV_LIMIT: "limit"}
KRYLOV_DENOM = {0: None, 1: "(p, q)", 2: "rho", 3: "(r^, v)", 4: "(t, t)", 5: "omega"}
KRYLOV_UPDATES = {"pcg_xr": 0, "pcg_p": 1, "bicg_p": 2, "bicg_s": 3, "bicg_xr": 4}
_KRYLOV_METHOD = {"pcg": KRYLOV_PCG, "bicgstab": KRYLOV_BICGSTAB}
_PRECOND_NAME = (None, "jacobi", "ilu0", "amg", "chebyshev", None, "fsai")  # a kind's name, at its code PRECOND_*; 5 is a hole
_PRECOND_CODE = {name: code for code, name in enumerate(_PRECOND_NAME) if code != 5}


def krylov_limits():
    """The Krylov solvers' limits (sblas_krylov_limits): dict(cell, width, pcg_vectors, bicgstab_vectors, max_dots) -- the
    elements of a dot product's cell, the lanes of its second stage, the work vectors each method owns (ILU(0) adds the
    solves' temporary) and the dots one pass over memory can carry."""
    out = (C.c_int64 * 5)()
    check(lib().sblas_krylov_limits(out), "sblas_krylov_limits")
    return dict(cell=int(out[0]), width=int(out[1]), pcg_vectors=int(out[2]), bicgstab_vectors=int(out[3]), max_dots=int(out[4]))


def krylov_dot_ref(x, y):
    """The pinned dot product restated on the host (sblas_krylov_dot_ref), on numpy arrays -> float"""
    x = np.ascontiguousarray(x, np.float64).ravel()
    y = np.ascontiguousarray(y, np.float64).ravel()
    if len(x) != len(y):
        raise SblasError("x has %d entries, y %d" % (len(x), len(y)))
    return float(lib().sblas_krylov_dot_ref(len(x), x.ctypes.data, y.ctypes.data))


def krylov_launches(method="pcg", precond=None, lower_launches=0, upper_launches=0):
    """Launches of one iteration (sblas_krylov_launches).  precond: None, "jacobi" or "ilu0"; lower_launches /
    upper_launches: SptrsvPlan.info()["launches"] of the two solves, read with "ilu0" only; with "amg" lower_launches is
    AmgPlan.info()["launches"], one cycle's; with "chebyshev" it is the polynomial's degree; with "fsai" FsaiPlan.info()["launches"], 2."""
    if method not in _KRYLOV_METHOD:
        raise SblasError("method must be 'pcg' or 'bicgstab', not %r" % (method,))
    lo, up = (C.c_int64 * 12)(), (C.c_int64 * 12)()
    lo[5], up[5] = int(lower_launches), int(upper_launches)
    n = int(lib().sblas_krylov_launches(_KRYLOV_METHOD[method], _PRECOND_CODE.get(precond, -1), lo, up))
    if n < 0:
        raise SblasError("sblas_krylov_launches refused its arguments")
    return n


# Restarted GMRES: the denominators a breakdown names continue the Krylov solvers' (SBLAS_GMRES_DENOM_*)
GMRES_DENOM = dict(KRYLOV_DENOM)
GMRES_DENOM.update({6: "givens", 7: "beta"})


def gmres_limits():
    """GMRES's limits (sblas_gmres_limits): dict(max_restart, default_restart, max_dots, vectors_per_restart,
    vectors_fixed, scalar_bytes, matrix_bytes, dot_group).  A plan of restart m owns vectors_per_restart * m +
    vectors_fixed work vectors (ILU(0) adds the solves' temporary)."""
    out = (C.c_int64 * 8)()
    check(lib().sblas_gmres_limits(out), "sblas_gmres_limits")
    keys = ("max_restart", "default_restart", "max_dots", "vectors_per_restart", "vectors_fixed", "scalar_bytes", "matrix_bytes", "dot_group")
    return dict(zip(keys, (int(v) for v in out)))


def gmres_step_ref(j, h, eta, c, s, g, tol, iterations=0, max_iter=1000):
    """The scalar step of Arnoldi step j restated on the host (sblas_gmres_step_ref).  h: the j + 1 entries of the new
    Hessenberg column; c, s: the rotations so far (at least j entries); g: at least j + 1 entries.  Nothing given is
    changed -> dict(status, code, h, c, s, g, rcol, iterations, rnorm, breakdown) with c, s of j + 1 and g of j + 2
    entries; rnorm is None and c, s, g are the given ones after a breakdown."""
    j = int(j)
    if not 0 <= j < gmres_limits()["max_restart"]:
        raise SblasError("j must be in [0, %d), not %d" % (gmres_limits()["max_restart"], j))
    pad = lambda a, k: np.concatenate([np.asarray(a, np.float64).ravel()[:k], np.zeros(max(k - len(np.ravel(a)), 0))])
    if len(np.ravel(h)) != j + 1 or len(np.ravel(c)) < j or len(np.ravel(s)) < j or len(np.ravel(g)) < j + 1:
        raise SblasError("h needs j + 1 entries, c and s at least j, g at least j + 1")
    h, c, s, g, rcol = pad(h, j + 1), pad(c, j + 1), pad(s, j + 1), pad(g, j + 2), np.zeros(j + 1)
    it, rnorm, which = C.c_int64(int(iterations)), C.c_double(float("nan")), C.c_int64(0)
    code = lib().sblas_gmres_step_ref(j, h.ctypes.data, float(eta), c.ctypes.data, s.ctypes.data, g.ctypes.data, rcol.ctypes.data,
                                      float(tol), int(max_iter), C.byref(it), C.byref(rnorm), C.byref(which))
    if code < 0:
        raise SblasError("sblas_gmres_step_ref refused its arguments")
    broke = code == KRYLOV_BREAKDOWN
    return dict(status=KRYLOV_STATUS[code], code=code, h=h, c=c[:j] if broke else c, s=s[:j] if broke else s, g=g[:j + 1] if broke else g,
                rcol=None if broke else rcol, iterations=int(it.value), rnorm=None if broke else float(rnorm.value),
                breakdown=GMRES_DENOM[int(which.value)])


def gmres_solve_ref(R, g):
    """The back substitution restated on the host (sblas_gmres_solve_ref): y with R y = g over k = R.shape[0] columns; R
    is the k x k upper triangle as a numpy matrix (R[i, l]), g has at least k entries."""
    R = np.asarray(R, np.float64)
    k = R.shape[0] if R.ndim == 2 else -1
    if R.ndim != 2 or R.shape[1] != k or len(np.ravel(g)) < k:
        raise SblasError("R must be k x k and g have at least k entries")
    cols = np.ascontiguousarray(R.T)                                         # by columns: entry (i, l) at l * k + i
    g = np.ascontiguousarray(np.ravel(g)[:k], np.float64)
    y = np.zeros(k)
    check(lib().sblas_gmres_solve_ref(k, cols.ctypes.data, max(k, 1), g.ctypes.data, y.ctypes.data), "sblas_gmres_solve_ref")
    return y


def gmres_launches(restart=30, precond=None, lower_launches=0, upper_launches=0):
    """Launches of GMRES (sblas_gmres_launches) -> dict(step, close, restart, start, cycle); a step's do not depend on j.
    precond: None, "jacobi" or "ilu0"; lower_launches / upper_launches: SptrsvPlan.info()["launches"], read with "ilu0" only;
    with "amg" lower_launches is one cycle's, with "chebyshev" the polynomial's degree, with "fsai" 2."""
    lo, up, out = (C.c_int64 * 12)(), (C.c_int64 * 12)(), (C.c_int64 * 4)()
    lo[5], up[5] = int(lower_launches), int(upper_launches)
    cycle = int(lib().sblas_gmres_launches(int(restart), _PRECOND_CODE.get(precond, -1), lo, up, out))
    if cycle < 0:
        raise SblasError("sblas_gmres_launches refused its arguments")
    return dict(step=int(out[0]), close=int(out[1]), restart=int(out[2]), start=int(out[3]), cycle=cycle)


# Aggregation AMG: smoothers and sweep modes (SBLAS_AMG_*)
AMG_SMOOTHERS = {"jacobi": 0, "l1": 1}
AMG_CHEBYSHEV = 2                                                           # SBLAS_AMG_CHEBYSHEV: AmgPlan.setup(smoother="chebyshev")
AMG_SWEEP_MODES = {"sweep": 0, "residual": 1, "first": 2}


def amg_limits():
    """The AMG plan's limits (sblas_amg_limits): dict(g4_max, g16_max, threads, coarse_max, max_levels, nu, coarse_sweeps,
    level_cap) -- the longest stored rows that 4 and 16 lanes sum, a workgroup's threads, the defaults, and the largest
    max_levels."""
    out = (C.c_int64 * 8)()
    check(lib().sblas_amg_limits(out), "sblas_amg_limits")
    keys = ("g4_max", "g16_max", "threads", "coarse_max", "max_levels", "nu", "coarse_sweeps", "level_cap")
    return dict(zip(keys, (int(v) for v in out)))


def amg_aggregate(n, rowptr, colidx, val=None, theta=0.0, seed=0, level=0):
    """One level's pinned aggregation on host arrays (sblas_amg_aggregate) -> (agg, aggptr, members): every vertex's
    aggregate, and the vertices by (aggregate, vertex) with aggptr of n_agg + 1 entries.  Roots are the greedy maximal
    independent set over the strong neighbours in descending fmix32(v + 0x9E3779B9 * (seed + level + 1)).  A refused
    structure raises an SblasError whose .bad_row is the first bad row."""
    rowptr = np.ascontiguousarray(rowptr, np.int32)
    colidx = np.ascontiguousarray(colidx, np.int32)
    if len(rowptr) != n + 1:
        raise SblasError("rowptr has %d entries for %d rows" % (len(rowptr), n))
    if val is not None:
        val = np.ascontiguousarray(val, np.float64)
        if len(val) != len(colidx):
            raise SblasError("val has %d entries, colidx %d" % (len(val), len(colidx)))
    agg, aggptr, members = np.zeros(max(n, 1), np.int32), np.zeros(n + 1, np.int32), np.zeros(max(n, 1), np.int32)
    n_agg, bad = C.c_int64(), C.c_int64(-1)
    rc = lib().sblas_amg_aggregate(n, rowptr.ctypes.data, colidx.ctypes.data if len(colidx) else None,
                                   val.ctypes.data if val is not None else None, float(theta), int(seed) & 0xffffffff,
                                   int(level) & 0xffffffff, agg.ctypes.data, aggptr.ctypes.data, members.ctypes.data, C.byref(n_agg),
                                   C.byref(bad))
    if rc != 0:
        raise _bad_structure("sblas_amg_aggregate", rc, bad.value)
    return agg[:n], aggptr[:n_agg.value + 1].copy(), members[:n]


AMG_AGGREGATIONS = {"host": 0, "device": 1}                                # SBLAS_AMG_AGG_*


def amg_roots_rounds_ref(n, rowptr, colidx, val=None, theta=0.0, seed=0, level=0):
    """The aggregation rule in synchronous rounds on host arrays (sblas_amg_roots_rounds_ref) -> (root, rounds): root[v]
    is True for the roots of amg_aggregate, rounds counts the rounds that decided a vertex -- the upper bound of
    amg_aggregate_device's.  The arguments and refusals of amg_aggregate."""
    rowptr = np.ascontiguousarray(rowptr, np.int32)
    colidx = np.ascontiguousarray(colidx, np.int32)
    if len(rowptr) != n + 1:
        raise SblasError("rowptr has %d entries for %d rows" % (len(rowptr), n))
    if val is not None:
        val = np.ascontiguousarray(val, np.float64)
        if len(val) != len(colidx):
            raise SblasError("val has %d entries, colidx %d" % (len(val), len(colidx)))
    root = np.zeros(max(n, 1), np.uint8)
    rounds, bad = C.c_int64(), C.c_int64(-1)
    rc = lib().sblas_amg_roots_rounds_ref(n, rowptr.ctypes.data, colidx.ctypes.data if len(colidx) else None,
                                          val.ctypes.data if val is not None else None, float(theta), int(seed) & 0xffffffff,
                                          int(level) & 0xffffffff, root.ctypes.data, C.byref(rounds), C.byref(bad))
    if rc != 0:
        raise _bad_structure("sblas_amg_roots_rounds_ref", rc, bad.value)
    return root[:n].astype(bool), int(rounds.value)


def amg_aggregate_device(n, rowptr, colidx, val=None, theta=0.0, seed=0, level=0, stream=None):
    """One level's aggregation on the device (sblas_hip_amg_aggregate_i32) -> (agg, aggptr, members, rounds): torch int32
    tensors equal to amg_aggregate's, and the Jones-Plassmann rounds taken (at most amg_roots_rounds_ref's).  rowptr,
    colidx (int32) and val (float64, needed when theta > 0) are GPU tensors.  The entry point trusts the structure, so
    it is checked here on the host first (sblas_ilu0_check): a refused one raises an SblasError with .bad_row and
    nothing is launched.  Synchronises."""
    import torch
    nnz = _structure(n, rowptr, colidx)
    theta = float(theta)
    if not 0.0 <= theta <= 1.0:
        raise SblasError("theta must be in [0, 1], not %r" % (theta,))
    if theta > 0.0 and val is None:
        raise SblasError("theta > 0 needs val, the values the strength test reads")
    device = rowptr.device
    if colidx.device != device or not rowptr.is_contiguous() or not colidx.is_contiguous():
        raise SblasError("rowptr and colidx must be contiguous tensors on one device")
    if val is not None:
        _krylov_vector("val", val, nnz, device)
    h_rp, h_ci = rowptr.cpu().numpy(), colidx.cpu().numpy()
    bad = C.c_int64(-1)
    if n > 0 and int(h_rp[n]) != nnz:
        raise _bad_structure("sblas_hip_amg_aggregate_i32", 1, n - 1)
    rc = lib().sblas_ilu0_check(n, h_rp.ctypes.data, h_ci.ctypes.data if nnz else None, None, C.byref(bad))
    if rc != 0:
        raise _bad_structure("sblas_hip_amg_aggregate_i32", rc, bad.value)
    agg = torch.empty(n, dtype=torch.int32, device=device)
    aggptr = torch.empty(n + 1, dtype=torch.int32, device=device)
    members = torch.empty(n, dtype=torch.int32, device=device)
    bytes_ = int(lib().sblas_hip_amg_aggregate_workspace(n, nnz))
    ws = torch.empty(max(bytes_, 16), dtype=torch.uint8, device=device)
    n_agg, rounds = C.c_int64(), C.c_int64()
    with torch.cuda.device(device):
        rc = lib().sblas_hip_amg_aggregate_i32(-1, _stream(stream), n, nnz, rowptr.data_ptr() if n else None, colidx.data_ptr() if nnz else None,
                                               val.data_ptr() if val is not None and theta > 0.0 and nnz else None, theta,
                                               int(seed) & 0xffffffff, int(level) & 0xffffffff, agg.data_ptr() if n else None,
                                               aggptr.data_ptr(), members.data_ptr() if n else None, ws.data_ptr(), bytes_, C.byref(n_agg),
                                               C.byref(rounds))
    check(rc, "sblas_hip_amg_aggregate_i32")
    return agg, aggptr[:n_agg.value + 1], members, int(rounds.value)


def amg_launches(levels, nu=1, coarse_sweeps=8, degree=0):
    """Launches of one AmgPlan.apply (sblas_amg_launches): (2 nu + 3) a level above the coarsest, coarse_sweeps on it; with
    the Chebyshev smoother of `degree` >= 1 (sblas_amg_launches_cheb) (2 nu degree + 3) a level."""
    if degree:
        k = int(lib().sblas_amg_launches_cheb(int(levels), int(nu), int(coarse_sweeps), int(degree)))
    else:
        k = int(lib().sblas_amg_launches(int(levels), int(nu), int(coarse_sweeps)))
    if k < 0:
        raise SblasError("sblas_amg_launches refused its arguments")
    return k


def amg_wd_ref(n, rowptr, colidx, val, smoother="jacobi", omega=None):
    """setup's wd on host arrays (sblas_amg_wd_ref) -> (wd, bad_row): omega / a_ii, or omega / sum |a_ie| for "l1";
    bad_row is the first row whose diagonal is not finite and > 0, or -1."""
    if smoother not in AMG_SMOOTHERS:
        raise SblasError("smoother must be 'jacobi' or 'l1', not %r" % (smoother,))
    if omega is None:
        omega = 1.0 if smoother == "l1" else 2.0 / 3.0
    rowptr, colidx = np.ascontiguousarray(rowptr, np.int32), np.ascontiguousarray(colidx, np.int32)
    val = np.ascontiguousarray(val, np.float64)
    wd, bad = np.zeros(max(n, 1)), C.c_int64(-1)
    rc = lib().sblas_amg_wd_ref(n, rowptr.ctypes.data, colidx.ctypes.data, val.ctypes.data, AMG_SMOOTHERS[smoother], float(omega),
                                wd.ctypes.data, C.byref(bad))
    if rc != 0:
        raise _bad_structure("sblas_amg_wd_ref", rc, bad.value)
    return wd[:n], int(bad.value)


def amg_cycle_ref(levels, r, nu=1, coarse_sweeps=8, coarse_scale=1.0, degree=0):
    """The whole V-cycle in plain C++ on host arrays (sblas_amg_cycle_ref) -> z.  levels: a list of dicts with n, rowptr,
    colidx, val, wd and, on all but the last, agg, aggptr, members (numpy arrays).  degree >= 1: the Chebyshev smoother
    (sblas_amg_cycle_cheb_ref): wd holds 1 / a_ii and every level has table, its (c1_k, c2_k) rows."""
    k = len(levels)
    if k == 0:
        return np.zeros(0)
    keep = []

    def column(name, dtype, upto):
        arr = (C.c_void_p * k)()
        for l in range(upto):
            a = np.ascontiguousarray(levels[l][name], dtype)
            keep.append(a)
            arr[l] = a.ctypes.data if a.size else None
        return arr
    ns = (C.c_int64 * k)(*[int(L["n"]) for L in levels])
    r = np.ascontiguousarray(r, np.float64)
    if len(r) != ns[0]:
        raise SblasError("r has %d entries for %d rows" % (len(r), ns[0]))
    z = np.zeros(max(len(r), 1))
    if degree:
        check(lib().sblas_amg_cycle_cheb_ref(k, ns, column("rowptr", np.int32, k), column("colidx", np.int32, k), column("val", np.float64, k),
                                             column("wd", np.float64, k), column("table", np.float64, k), column("agg", np.int32, k - 1),
                                             column("aggptr", np.int32, k - 1), column("members", np.int32, k - 1), int(nu), int(degree),
                                             int(coarse_sweeps), float(coarse_scale), r.ctypes.data if len(r) else None, z.ctypes.data),
              "sblas_amg_cycle_cheb_ref")
        return z[:len(r)]
    check(lib().sblas_amg_cycle_ref(k, ns, column("rowptr", np.int32, k), column("colidx", np.int32, k), column("val", np.float64, k),
                                    column("wd", np.float64, k), column("agg", np.int32, k - 1), column("aggptr", np.int32, k - 1),
                                    column("members", np.int32, k - 1), int(nu), int(coarse_sweeps), float(coarse_scale),
                                    r.ctypes.data if len(r) else None, z.ctypes.data), "sblas_amg_cycle_ref")
    return z[:len(r)]


# Smoothed aggregation: the prolongators and the modes of the transfer row product (SBLAS_AMG_*)
AMG_PROLONGATORS = {"plain": 0, "smoothed": 1}
AMG_TRANSFER_MODES = {"restrict": 0, "prolong": 1}
AMG_PROLONG_OMEGA = 2.0 / 3.0
AMG_SMOOTHED_MIN_REDUCTION = 0.2


def amg_keep_level(n, n_next, min_reduction=0.0):
    """The coarsening guard (sblas_amg_keep_level): a level of n rows whose aggregation leaves n_next is kept when
    n_next < n and float(n_next) <= (1.0 - min_reduction) * float(n), the product rounded once."""
    rc = lib().sblas_amg_keep_level(int(n), int(n_next), float(min_reduction))
    if rc < 0:
        raise SblasError("sblas_amg_keep_level refused its arguments: sizes >= 0, min_reduction in [0, 1)")
    return bool(rc)


def amg_prolongator_ref(n, rowptr, colidx, val, agg, n_agg, prolong_omega=AMG_PROLONG_OMEGA):
    """The smoothed prolongator on host arrays in the pinned order (sblas_amg_prolongator_ref) -> (p_rowptr, p_colidx,
    p_val): n rows by n_agg columns, the COO sum of the triplets (row(e), agg[col(e)], t_e)."""
    rowptr, colidx = np.ascontiguousarray(rowptr, np.int32), np.ascontiguousarray(colidx, np.int32)
    val, agg = np.ascontiguousarray(val, np.float64), np.ascontiguousarray(agg, np.int32)
    n = int(n)
    if len(rowptr) != n + 1 or len(agg) != n or len(colidx) != len(val) or (n and rowptr[n] != len(colidx)):
        raise SblasError("rowptr must have n + 1 entries, agg n, colidx and val rowptr[n]")
    nnz = len(colidx)
    prp, pci, pv = np.zeros(n + 1, np.int32), np.zeros(max(nnz, 1), np.int32), np.zeros(max(nnz, 1), np.float64)
    count, bad = C.c_int64(0), C.c_int64(-1)
    rc = lib().sblas_amg_prolongator_ref(n, rowptr.ctypes.data, colidx.ctypes.data if nnz else None, val.ctypes.data if nnz else None,
                                         agg.ctypes.data if n else None, int(n_agg), float(prolong_omega), prp.ctypes.data, pci.ctypes.data,
                                         pv.ctypes.data, C.byref(count), C.byref(bad))
    if rc != 0:
        raise _bad_structure("sblas_amg_prolongator_ref", rc, bad.value)
    return prp, pci[:count.value].copy(), pv[:count.value].copy()


def amg_transfer_ref(mode, rowptr, colidx, val, x, out=None, scale=1.0):
    """The transfers' row product in lane order on host arrays (sblas_amg_transfer_ref).  mode "restrict": -> s, the row
    sums of the CSR (rowptr, colidx, val) on x; "prolong": -> out + scale * s (out is not changed)."""
    if mode not in AMG_TRANSFER_MODES:
        raise SblasError("mode must be 'restrict' or 'prolong', not %r" % (mode,))
    rowptr, colidx = np.ascontiguousarray(rowptr, np.int32), np.ascontiguousarray(colidx, np.int32)
    val, x = np.ascontiguousarray(val, np.float64), np.ascontiguousarray(x, np.float64)
    rows = len(rowptr) - 1
    if rows < 0 or len(colidx) != len(val) or (rows and rowptr[rows] != len(colidx)) or (len(colidx) and int(colidx.max()) >= len(x)):
        raise SblasError("a CSR of len(rowptr) - 1 rows whose columns name entries of x")
    if mode == "prolong":
        if out is None or len(out) != rows:
            raise SblasError("prolong needs out, one entry a row")
        y = np.array(out, np.float64)
    else:
        y = np.zeros(rows)
    buf = y if rows else np.zeros(1)
    check(lib().sblas_amg_transfer_ref(AMG_TRANSFER_MODES[mode], rows, rowptr.ctypes.data, colidx.ctypes.data if len(colidx) else None,
                                       val.ctypes.data if len(val) else None, float(scale), x.ctypes.data if len(x) else None,
                                       buf.ctypes.data), "sblas_amg_transfer_ref")
    return y


def amg_cycle_sa_ref(levels, r, nu=1, coarse_sweeps=8, coarse_scale=1.0, degree=0):
    """The V-cycle with general transfer operators in plain C++ on host arrays (sblas_amg_cycle_sa_ref) -> z.  levels: a
    list of dicts with n, rowptr, colidx, val, wd and, on all but the last, p_rowptr, p_colidx, p_val, r_rowptr, r_colidx,
    r_val (numpy arrays).  degree >= 1: the Chebyshev smoother (sblas_amg_cycle_cheb_sa_ref), as amg_cycle_ref's."""
    k = len(levels)
    if k == 0:
        return np.zeros(0)
    keep = []

    def column(name, dtype, upto):
        arr = (C.c_void_p * k)()
        for l in range(upto):
            a = np.ascontiguousarray(levels[l][name], dtype)
            keep.append(a)
            arr[l] = a.ctypes.data if a.size else None
        return arr
    ns = (C.c_int64 * k)(*[int(L["n"]) for L in levels])
    r = np.ascontiguousarray(r, np.float64)
    if len(r) != ns[0]:
        raise SblasError("r has %d entries for %d rows" % (len(r), ns[0]))
    z = np.zeros(max(len(r), 1))
    if degree:
        check(lib().sblas_amg_cycle_cheb_sa_ref(k, ns, column("rowptr", np.int32, k), column("colidx", np.int32, k), column("val", np.float64, k),
                                                column("wd", np.float64, k), column("table", np.float64, k), column("p_rowptr", np.int32, k - 1),
                                                column("p_colidx", np.int32, k - 1), column("p_val", np.float64, k - 1),
                                                column("r_rowptr", np.int32, k - 1), column("r_colidx", np.int32, k - 1),
                                                column("r_val", np.float64, k - 1), int(nu), int(degree), int(coarse_sweeps), float(coarse_scale),
                                                r.ctypes.data if len(r) else None, z.ctypes.data), "sblas_amg_cycle_cheb_sa_ref")
        return z[:len(r)]
    check(lib().sblas_amg_cycle_sa_ref(k, ns, column("rowptr", np.int32, k), column("colidx", np.int32, k), column("val", np.float64, k),
                                       column("wd", np.float64, k), column("p_rowptr", np.int32, k - 1), column("p_colidx", np.int32, k - 1),
                                       column("p_val", np.float64, k - 1), column("r_rowptr", np.int32, k - 1),
                                       column("r_colidx", np.int32, k - 1), column("r_val", np.float64, k - 1), int(nu), int(coarse_sweeps),
                                       float(coarse_scale), r.ctypes.data if len(r) else None, z.ctypes.data), "sblas_amg_cycle_sa_ref")
    return z[:len(r)]


def partition_dense(first_order, n_gpu, i_gpu):
    o, d = C.c_int64(), C.c_int64()
    check(lib().sblas_partition_dense(first_order, n_gpu, i_gpu, C.byref(o), C.byref(d)), "sblas_partition_dense")
    return o.value, d.value


# ------------------------------------------------------------------------------------------
# device calls (torch tensors carry the device pointers)
# ------------------------------------------------------------------------------------------
def _dev_ptr(t, dtype, what):
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise SblasError("%s must be a GPU tensor (no CPU path exists)" % what)
    if t.dtype != dtype or not t.is_contiguous():
        raise SblasError("%s must be a contiguous %s tensor" % (what, dtype))
    return t.data_ptr()


def _stream(stream=None):
    import torch
    s = stream if stream is not None else torch.cuda.current_stream()
    return C.c_void_p(s.cuda_stream)


def spmm_workspace_bytes(rows, cols, nnz, n):
    return int(lib().sblas_hip_spmm_csr_f64_i32_workspace(rows, cols, nnz, n))


def spmm(rows, cols, rowptr, colidx, val, B, ldb, n, alpha, beta, Cmat, ldc, workspace, stream=None, c_offset=0):
    """C = alpha*A*B + beta*C through sblas_hip_spmm_csr_f64_i32.  B, C column-major flat tensors.
    c_offset: element offset into Cmat (method 2 points C at Ccopy + start_row)."""
    import torch
    nnz = int(colidx.numel())
    rc = lib().sblas_hip_spmm_csr_f64_i32(
        -1, _stream(stream), rows, cols, nnz,
        _dev_ptr(rowptr, torch.int32, "rowptr"), _dev_ptr(colidx, torch.int32, "colidx") if nnz else None,
        _dev_ptr(val, torch.float64, "val") if nnz else None,
        _dev_ptr(B, torch.float64, "B") if cols else None, ldb, n, alpha, beta,
        _dev_ptr(Cmat, torch.float64, "C") + 8 * c_offset, ldc,
        _dev_ptr(workspace, torch.float64, "workspace") if workspace is not None and workspace.numel() else None,
        workspace.numel() * 8 if workspace is not None else 0)
    check(rc, "sblas_hip_spmm_csr_f64_i32")


class SpmmPlan:
    """A per-matrix plan (sblas_hip_spmm_plan_create): the panel verdicts of one structure (rowptr, colidx) at one
    width n, taken once.  Keeps the structure tensors alive; destroy() / garbage collection frees the device buffer.
    split=True makes a split plan (sblas_hip_spmm_plan_create_split): rows of split_min+ nonzeros in the direct kernels'
    panels are summed in pieces of at most `piece` nonzeros on workgroups of their own (0: the library's defaults)."""

    def __init__(self, rows, cols, rowptr, colidx, n, stream=None, split=False, split_min=0, piece=0):
        import torch
        self.rows, self.cols, self.n, self.rowptr, self.colidx = rows, cols, n, rowptr, colidx
        self.nnz = int(colidx.numel())
        h = C.c_void_p()
        args = (-1, _stream(stream), rows, cols, self.nnz, _dev_ptr(rowptr, torch.int32, "rowptr"),
                _dev_ptr(colidx, torch.int32, "colidx") if self.nnz else None, n)
        if split:
            check(lib().sblas_hip_spmm_plan_create_split(*args, split_min, piece, C.byref(h)), "sblas_hip_spmm_plan_create_split")
        else:
            check(lib().sblas_hip_spmm_plan_create(*args, C.byref(h)), "sblas_hip_spmm_plan_create")
        self.handle = h

    def split_info(self):
        out = (C.c_int64 * 4)()
        check(lib().sblas_hip_spmm_plan_split_info(self.handle, out), "sblas_hip_spmm_plan_split_info")
        return dict(split_rows=int(out[0]), pieces=int(out[1]), split_nnz=int(out[2]), partial_bytes=int(out[3]))

    def info(self):
        out = (C.c_int64 * 8)()
        check(lib().sblas_hip_spmm_plan_info(self.handle, out), "sblas_hip_spmm_plan_info")
        return dict(active=bool(out[0]), windowed=int(out[1]), direct=int(out[2]), mfma=int(out[3]), merge=out[4] == 1,
                    four_rows=out[4] == 2,
                    stage_range=bool(out[5]), ldbt=int(out[6]), panel_rows=int(out[7]))

    def spmm(self, val, B, ldb, n, alpha, beta, Cmat, ldc, workspace, stream=None, c_offset=0):
        """The planned form of spmm(): same arguments, same results, only the kernels that have panels are launched."""
        import torch
        rc = lib().sblas_hip_spmm_csr_f64_i32_planned(
            self.handle, -1, _stream(stream), self.rows, self.cols, self.nnz,
            _dev_ptr(self.rowptr, torch.int32, "rowptr"), _dev_ptr(self.colidx, torch.int32, "colidx") if self.nnz else None,
            _dev_ptr(val, torch.float64, "val") if self.nnz else None,
            _dev_ptr(B, torch.float64, "B") if self.cols else None, ldb, n, alpha, beta,
            _dev_ptr(Cmat, torch.float64, "C") + 8 * c_offset, ldc,
            _dev_ptr(workspace, torch.float64, "workspace") if workspace is not None and workspace.numel() else None,
            workspace.numel() * 8 if workspace is not None else 0)
        check(rc, "sblas_hip_spmm_csr_f64_i32_planned")

    def spmm_ordered(self, val, B, ldb, order_b, n, alpha, beta, Cmat, ldc, order_c, workspace, stream=None, c_offset=0):
        """The planned form of spmm_ordered() (float64 values, int32 indices): one plan serves every order pair."""
        import torch
        rc = lib().sblas_hip_spmm_csr_ordered_f64_i32_planned(
            self.handle, -1, _stream(stream), self.rows, self.cols, self.nnz,
            _dev_ptr(self.rowptr, torch.int32, "rowptr"), _dev_ptr(self.colidx, torch.int32, "colidx") if self.nnz else None,
            _dev_ptr(val, torch.float64, "val") if self.nnz else None,
            _dev_ptr(B, torch.float64, "B") if self.cols else None, ldb, order_b, n, alpha, beta,
            _dev_ptr(Cmat, torch.float64, "C") + 8 * c_offset, ldc, order_c,
            _dev_ptr(workspace, workspace.dtype, "workspace") if workspace is not None and workspace.numel() else None,
            workspace.numel() * workspace.element_size() if workspace is not None else 0)
        check(rc, "sblas_hip_spmm_csr_ordered_f64_i32_planned")

    def destroy(self):
        if self.handle:
            lib().sblas_hip_spmm_plan_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def dense_to_rowmajor(cols, n, B, ldb, Bt, stream=None):
    import torch
    ldbt = int(lib().sblas_hip_spmm_ldbt(n))
    check(lib().sblas_hip_dense_to_rowmajor_f64(-1, _stream(stream), cols, n, _dev_ptr(B, torch.float64, "B"), ldb,
                                                _dev_ptr(Bt, torch.float64, "Bt"), ldbt), "sblas_hip_dense_to_rowmajor_f64")
    return ldbt


def spmm_rowmajorB(rows, cols, rowptr, colidx, val, Bt, n, alpha, beta, Cmat, ldc, stream=None, c_offset=0):
    import torch
    nnz = int(colidx.numel())
    ldbt = int(lib().sblas_hip_spmm_ldbt(n))
    rc = lib().sblas_hip_spmm_csr_rowmajorB_f64_i32(
        -1, _stream(stream), rows, cols, nnz,
        _dev_ptr(rowptr, torch.int32, "rowptr"), _dev_ptr(colidx, torch.int32, "colidx") if nnz else None,
        _dev_ptr(val, torch.float64, "val") if nnz else None,
        _dev_ptr(Bt, torch.float64, "Bt") if Bt is not None else None, ldbt, n, alpha, beta,
        _dev_ptr(Cmat, torch.float64, "C") + 8 * c_offset, ldc)
    check(rc, "sblas_hip_spmm_csr_rowmajorB_f64_i32")


def validate_csr(rows, cols, rowptr, colidx, stream=None):
    """True when the CSR structure on the device is well formed (sblas_hip_debug_validate_csr_i32; synchronises)."""
    import torch
    nnz = int(colidx.numel())
    rc = lib().sblas_hip_debug_validate_csr_i32(-1, _stream(stream), rows, cols, nnz, _dev_ptr(rowptr, torch.int32, "rowptr"),
                                                _dev_ptr(colidx, torch.int32, "colidx") if nnz else None)
    if rc not in (0, 1):
        check(rc, "sblas_hip_debug_validate_csr_i32")
    return rc == 0


def panel_stats(reset=True):
    """(windowed, direct, fallback) panel counts of the SpMM launches since the last reset."""
    out = (C.c_uint64 * 4)()
    check(lib().sblas_hip_debug_spmm_panel_stats(out, 1 if reset else 0), "sblas_hip_debug_spmm_panel_stats")
    return int(out[0]), int(out[1]), int(out[2])


def kernel_events(enable):
    check(lib().sblas_hip_debug_spmm_kernel_events(1 if enable else 0), "sblas_hip_debug_spmm_kernel_events")


def last_kernel_ms():
    """Duration of the dominant stage-2 kernel of the most recent SpMM launch (waits for it); needs kernel_events(True)."""
    ms = C.c_float()
    check(lib().sblas_hip_debug_spmm_last_kernel_ms(C.byref(ms)), "sblas_hip_debug_spmm_last_kernel_ms")
    return float(ms.value)


def reload_env():
    """Have the library re-read its SBLAS_* experiment switches (it reads the environment only once)."""
    check(lib().sblas_hip_debug_reload_env(), "sblas_hip_debug_reload_env")


def spmv(rows, cols, rowptr, colidx, val, x, alpha, beta, y, stream=None, y_offset=0):
    import torch
    nnz = int(colidx.numel())
    rc = lib().sblas_hip_spmv_csr_f64_i32(
        -1, _stream(stream), rows, cols, nnz,
        _dev_ptr(rowptr, torch.int32, "rowptr"), _dev_ptr(colidx, torch.int32, "colidx") if nnz else None,
        _dev_ptr(val, torch.float64, "val") if nnz else None,
        _dev_ptr(x, torch.float64, "x"), alpha, beta, _dev_ptr(y, torch.float64, "y") + 8 * y_offset)
    check(rc, "sblas_hip_spmv_csr_f64_i32")


class SpmvPlan:
    """A per-matrix SpMV plan (sblas_hip_spmv_plan_create): the work items of one structure (rowptr, colidx), taken once.
    Keeps the structure tensors alive; destroy() / garbage collection frees the device buffer."""

    def __init__(self, rows, cols, rowptr, colidx, stream=None):
        import torch
        self.rows, self.cols, self.rowptr, self.colidx = rows, cols, rowptr, colidx
        self.nnz = int(colidx.numel())
        self.handle = None
        h = C.c_void_p()
        check(lib().sblas_hip_spmv_plan_create(-1, _stream(stream), rows, cols, self.nnz, _dev_ptr(rowptr, torch.int32, "rowptr"),
                                               _dev_ptr(colidx, torch.int32, "colidx") if self.nnz else None, C.byref(h)),
              "sblas_hip_spmv_plan_create")
        self.handle = h

    def info(self):
        out = (C.c_int64 * 8)()
        check(lib().sblas_hip_spmv_plan_info(self.handle, out), "sblas_hip_spmv_plan_info")
        return dict(active=bool(out[0]), lanes=int(out[1]), stream4096=int(out[2]), stream6144=int(out[3]), segmented=int(out[4]),
                    lds=int(out[5]), split_rows=int(out[6]), split_pieces=int(out[7]))

    def spmv(self, val, x, alpha, beta, y, stream=None, y_offset=0, rows=None, nnz=None):
        """The planned form of spmv(): y = alpha*A*x + beta*y.  rows / nnz override the plan's own (tests of the refusal)."""
        import torch
        rc = lib().sblas_hip_spmv_csr_f64_i32_planned(
            self.handle, -1, _stream(stream), self.rows if rows is None else rows, self.cols,
            self.nnz if nnz is None else nnz,
            _dev_ptr(self.rowptr, torch.int32, "rowptr"), _dev_ptr(self.colidx, torch.int32, "colidx") if self.nnz else None,
            _dev_ptr(val, torch.float64, "val") if self.nnz else None,
            _dev_ptr(x, torch.float64, "x"), alpha, beta, _dev_ptr(y, torch.float64, "y") + 8 * y_offset)
        return rc

    def __call__(self, val, x, alpha, beta, y, stream=None, y_offset=0):
        check(self.spmv(val, x, alpha, beta, y, stream, y_offset), "sblas_hip_spmv_csr_f64_i32_planned")

    def destroy(self):
        if self.handle:
            lib().sblas_hip_spmv_plan_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def merge_rowblocks_local(M, N, starts, nrows, blocks, alpha, beta, Cmat, ldc=None, stream=None):
    """C = beta*C + alpha * (packed row blocks scattered into place), sblas_hip_merge_rowblocks_local_f64.
    blocks[q]: flat float64 device tensor holding an nrows[q] x N column-major block (leading dimension nrows[q])."""
    import torch
    g = len(blocks)
    st = (C.c_int64 * g)(*[int(v) for v in starts])
    nr = (C.c_int64 * g)(*[int(v) for v in nrows])
    for q in range(g):
        if blocks[q] is not None and blocks[q].numel() < int(nrows[q]) * N:
            raise SblasError("block %d is smaller than nrows x N" % q)
    ptrs = (C.c_void_p * g)(*[_dev_ptr(b, torch.float64, "block") if b is not None and b.numel() else None for b in blocks])
    pc = _dev_ptr(Cmat, torch.float64, "C")
    check(lib().sblas_hip_merge_rowblocks_local_f64(-1, _stream(stream), M, N, g, st, nr, ptrs, alpha, beta, pc,
                                                    M if ldc is None else ldc), "sblas_hip_merge_rowblocks_local_f64")


def axpby(n, alpha, x, beta, y, stream=None):
    """y = beta*y + alpha*x (kernel.h:27-38 semantics)."""
    import torch
    px, py = _dev_ptr(x, torch.float64, "x"), _dev_ptr(y, torch.float64, "y")
    check(lib().sblas_hip_axpby_f64(-1, _stream(stream), n, alpha, px, beta, py), "sblas_hip_axpby_f64")


# ------------------------------------------------------------------------------------------
# one process driving several GPUs (the reference's process model): comm.hip through the C ABI
# ------------------------------------------------------------------------------------------
def comm_get(devs):
    """Persistent communicator set over the device list `devs` (sblas_hip_comm_get).  All equal = ranks folded onto one
    device (on-device sum / no copies); all distinct = RCCL over xGMI."""
    arr = (C.c_int * len(devs))(*[int(d) for d in devs])
    out = C.c_void_p()
    check(lib().sblas_hip_comm_get(len(devs), arr, C.byref(out)), "sblas_hip_comm_get")
    return out


def _ptr_array(tensors, what, allow_none=False):
    import torch
    vals = []
    for t in tensors:
        if t is None or (allow_none and t.numel() == 0):
            vals.append(None)
        else:
            vals.append(_dev_ptr(t, torch.float64, what))
    return (C.c_void_p * len(vals))(*vals)


def _stream_array(streams):
    return (C.c_void_p * len(streams))(*[s.cuda_stream for s in streams])


def allreduce_sum(comm, bufs, streams, count):
    """In-place sum of bufs[r] (rank r's buffer on rank r's device / stream): sblas_hip_allreduce_sum_f64."""
    check(lib().sblas_hip_allreduce_sum_f64(comm, _ptr_array(bufs, "buf"), _stream_array(streams), count),
          "sblas_hip_allreduce_sum_f64")


def merge_rowblocks(comm, M, N, starts, nrows, partial, gather, alpha, beta, Cs, ldc, streams):
    """Method-2 / SpMV merge over the ranks of `comm`: exchange the packed row blocks (RCCL send/recv; folded ranks
    skip the copies) and scatter + alpha/beta on every rank (sblas_hip_merge_rowblocks_f64)."""
    g = len(partial)
    st = (C.c_int64 * g)(*[int(v) for v in starts])
    nr = (C.c_int64 * g)(*[int(v) for v in nrows])
    ga = _ptr_array(gather, "gather", allow_none=True) if gather is not None else None
    check(lib().sblas_hip_merge_rowblocks_f64(comm, M, N, st, nr, _ptr_array(partial, "partial", allow_none=True), ga,
                                              alpha, beta, _ptr_array(Cs, "C"), ldc, _stream_array(streams)),
          "sblas_hip_merge_rowblocks_f64")


def panel_census(reset=True):
    """dict(windowed, direct, fallback, mfma): row panels per stage-2 kernel since the last reset."""
    out = (C.c_uint64 * 4)()
    check(lib().sblas_hip_debug_spmm_panel_stats(out, 1 if reset else 0), "sblas_hip_debug_spmm_panel_stats")
    return dict(windowed=int(out[0]), direct=int(out[1]), fallback=int(out[2]), mfma=int(out[3]))


# ------------------------------------------------------------------------------------------
# the other value / index types of the reference's templates (typed entry points; tags from the tensors' dtypes)
# ------------------------------------------------------------------------------------------
F64, F32, I32, I64 = 0, 1, 0, 1


def _tags(val_dtype, idx_dtype):
    import torch
    vt = {torch.float64: F64, torch.float32: F32}.get(val_dtype)
    it = {torch.int32: I32, torch.int64: I64}.get(idx_dtype)
    if vt is None or it is None:
        raise SblasError("values must be float32 / float64 and indices int32 / int64 tensors")
    return vt, it


def spmm_typed_workspace_bytes(val_dtype, idx_dtype, rows, cols, nnz, n):
    vt, it = _tags(val_dtype, idx_dtype)
    return int(lib().sblas_hip_spmm_csr_workspace(vt, it, rows, cols, nnz, n))


def spmm_typed(rows, cols, rowptr, colidx, val, B, ldb, n, alpha, beta, Cmat, ldc, workspace, stream=None, c_offset=0):
    """sblas_hip_spmm_csr: C = alpha*A*B + beta*C in the tensors' own value / index types (workspace: a uint8 tensor)."""
    import torch
    vt, it = _tags(val.dtype, rowptr.dtype)
    nnz = int(colidx.numel())
    rc = lib().sblas_hip_spmm_csr(
        -1, _stream(stream), vt, it, rows, cols, nnz, _dev_ptr(rowptr, rowptr.dtype, "rowptr"),
        _dev_ptr(colidx, rowptr.dtype, "colidx") if nnz else None, _dev_ptr(val, val.dtype, "val") if nnz else None,
        _dev_ptr(B, val.dtype, "B") if cols else None, ldb, n, alpha, beta,
        _dev_ptr(Cmat, val.dtype, "C") + Cmat.element_size() * c_offset, ldc,
        _dev_ptr(workspace, torch.uint8, "workspace") if workspace is not None and workspace.numel() else None,
        workspace.numel() if workspace is not None else 0)
    check(rc, "sblas_hip_spmm_csr")


def spmv_typed(rows, cols, rowptr, colidx, val, x, alpha, beta, y, stream=None, y_offset=0):
    vt, it = _tags(val.dtype, rowptr.dtype)
    nnz = int(colidx.numel())
    rc = lib().sblas_hip_spmv_csr(
        -1, _stream(stream), vt, it, rows, cols, nnz, _dev_ptr(rowptr, rowptr.dtype, "rowptr"),
        _dev_ptr(colidx, rowptr.dtype, "colidx") if nnz else None, _dev_ptr(val, val.dtype, "val") if nnz else None,
        _dev_ptr(x, val.dtype, "x"), alpha, beta, _dev_ptr(y, val.dtype, "y") + y.element_size() * y_offset)
    check(rc, "sblas_hip_spmv_csr")


def axpby_typed(n, alpha, x, beta, y, stream=None):
    vt, _ = _tags(x.dtype, __import__("torch").int32)
    check(lib().sblas_hip_axpby(-1, _stream(stream), vt, n, alpha, _dev_ptr(x, x.dtype, "x"), beta, _dev_ptr(y, x.dtype, "y")),
          "sblas_hip_axpby")


def _typed_ptr_array(tensors, dtype, what, allow_none=False):
    vals = []
    for t in tensors:
        vals.append(None if t is None or (allow_none and t.numel() == 0) else _dev_ptr(t, dtype, what))
    return (C.c_void_p * len(vals))(*vals)


def allreduce_sum_typed(comm, bufs, streams, count):
    vt, _ = _tags(bufs[0].dtype, __import__("torch").int32)
    check(lib().sblas_hip_allreduce_sum(comm, vt, _typed_ptr_array(bufs, bufs[0].dtype, "buf"), _stream_array(streams), count),
          "sblas_hip_allreduce_sum")


def merge_rowblocks_typed(comm, M, N, starts, nrows, partial, gather, alpha, beta, Cs, ldc, streams):
    dt = Cs[0].dtype
    vt, _ = _tags(dt, __import__("torch").int32)
    g = len(partial)
    st = (C.c_int64 * g)(*[int(v) for v in starts])
    nr = (C.c_int64 * g)(*[int(v) for v in nrows])
    ga = _typed_ptr_array(gather, dt, "gather", allow_none=True) if gather is not None else None
    check(lib().sblas_hip_merge_rowblocks(comm, vt, M, N, st, nr, _typed_ptr_array(partial, dt, "partial", allow_none=True), ga,
                                          alpha, beta, _typed_ptr_array(Cs, dt, "C"), ldc, _stream_array(streams)),
          "sblas_hip_merge_rowblocks")


def partition_nnz_i64(rowptr, n_gpu, i_gpu):
    """sblas_partition_nnz for 64-bit row pointers."""
    rowptr = np.ascontiguousarray(rowptr, np.int64)
    rows = len(rowptr) - 1
    s, e, k, f = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
    buf = np.zeros(rows + 2, np.int64)
    num = lib().sblas_partition_nnz_i64(rowptr.ctypes.data, rows, int(rowptr[-1]), n_gpu, i_gpu, C.byref(s), C.byref(e),
                                        C.byref(k), C.byref(f), buf.ctypes.data)
    if num < 0:
        raise SblasError("sblas_partition_nnz_i64 failed (%d)" % num)
    return dict(start_row=s.value, stop_row=e.value, nnz=k.value, first_nnz=f.value, rowptr=buf[:num].copy())


# ------------------------------------------------------------------------------------------
# row-major dense operands (sblas_hip_spmm_csr_ordered & co.)
# ------------------------------------------------------------------------------------------
COL_MAJOR, ROW_MAJOR = 0, 1


def spmm_ordered(rows, cols, rowptr, colidx, val, B, ldb, order_b, n, alpha, beta, Cmat, ldc, order_c, workspace,
                 stream=None, c_offset=0):
    """sblas_hip_spmm_csr_ordered: C = alpha*A*B + beta*C with B and C each COL_MAJOR or ROW_MAJOR, in the tensors' own
    value / index types (float64 / int32 runs the tuned kernels).  B, C: flat device tensors; c_offset: element offset
    into Cmat.  workspace: any device tensor of at least spmm_typed_workspace_bytes(...) bytes (the same for every
    order pair)."""
    vt, it = _tags(val.dtype, rowptr.dtype)
    nnz = int(colidx.numel())
    rc = lib().sblas_hip_spmm_csr_ordered(
        -1, _stream(stream), vt, it, rows, cols, nnz, _dev_ptr(rowptr, rowptr.dtype, "rowptr"),
        _dev_ptr(colidx, rowptr.dtype, "colidx") if nnz else None, _dev_ptr(val, val.dtype, "val") if nnz else None,
        _dev_ptr(B, val.dtype, "B") if cols else None, ldb, order_b, n, alpha, beta,
        _dev_ptr(Cmat, val.dtype, "C") + Cmat.element_size() * c_offset, ldc, order_c,
        _dev_ptr(workspace, workspace.dtype, "workspace") if workspace is not None and workspace.numel() else None,
        workspace.numel() * workspace.element_size() if workspace is not None else 0)
    check(rc, "sblas_hip_spmm_csr_ordered")


def merge_rowblocks_ordered(comm, order, M, N, starts, nrows, partial, gather, alpha, beta, Cs, ldc, streams):
    """merge_rowblocks_typed with C in either order (sblas_hip_merge_rowblocks_ordered).  ROW_MAJOR: C is row-major and
    partial[q] holds an nrows[q] x N row-major block at leading dimension N."""
    dt = Cs[0].dtype
    vt, _ = _tags(dt, __import__("torch").int32)
    g = len(partial)
    st = (C.c_int64 * g)(*[int(v) for v in starts])
    nr = (C.c_int64 * g)(*[int(v) for v in nrows])
    ga = _typed_ptr_array(gather, dt, "gather", allow_none=True) if gather is not None else None
    check(lib().sblas_hip_merge_rowblocks_ordered(comm, vt, order, M, N, st, nr,
                                                  _typed_ptr_array(partial, dt, "partial", allow_none=True), ga, alpha, beta,
                                                  _typed_ptr_array(Cs, dt, "C"), ldc, _stream_array(streams)),
          "sblas_hip_merge_rowblocks_ordered")


def _layout(t, rows, cols, what):
    """(order, leading dimension) of a 2-D tensor view: strides (ld, 1) are row-major, (1, ld) column-major."""
    if t.dim() != 2 or tuple(t.shape) != (rows, cols):
        raise SblasError("%s must be a %d x %d tensor, got shape %s" % (what, rows, cols, tuple(t.shape)))
    s0, s1 = t.stride()
    if rows == 0 or cols == 0:                    # no element: whatever strides the tensor carries (numpy's are (0, 0)) say nothing
        return ROW_MAJOR, max(cols, 1)
    if s1 == 1 and s0 >= max(cols, 1):
        return ROW_MAJOR, s0
    if s0 == 1 and s1 >= max(rows, 1):
        return COL_MAJOR, s1
    if rows <= 1 and s1 == 1:
        return ROW_MAJOR, max(cols, 1)
    if cols <= 1 and s0 == 1:
        return COL_MAJOR, max(rows, 1)
    raise SblasError("%s has strides %s: only (ld, 1) (row-major) or (1, ld) (column-major) views are supported" %
                     (what, (s0, s1)))


def _view_ptr(t, what):
    import torch
    if t.dtype != torch.float64:
        raise SblasError("%s must be float64 (spmm_tensor handles float64 / int32 only; use spmm_ordered)" % what)
    if not t.is_cuda:
        raise SblasError("%s must be a GPU tensor (no CPU path exists)" % what)
    return t.data_ptr()


def spmm_tensor(A, B, C_, alpha, beta, workspace=None, plan=None, stream=None):
    """C = alpha*A*B + beta*C on 2-D torch tensors, without a copy: each dense operand's order and leading dimension
    come from its strides ((ld, 1) row-major, (1, ld) column-major), so contiguous tensors, .t() views and column slices
    work as they are.  A = (rows, cols, rowptr, colidx, val); float64 values and int32 indices only.  workspace: None
    (allocated here) or a device tensor of at least spmm_workspace_bytes(rows, cols, nnz, n) bytes; plan: an SpmmPlan
    of A."""
    import torch
    rows, cols, rowptr, colidx, val = A
    if val.dtype != torch.float64 or rowptr.dtype != torch.int32 or colidx.dtype != torch.int32:
        raise SblasError("spmm_tensor handles float64 values and int32 indices only; use spmm_ordered for other types")
    if B.dim() != 2 or C_.dim() != 2:
        raise SblasError("B and C must be 2-D tensors")
    n = int(C_.shape[1])
    order_b, ldb = _layout(B, cols, n, "B")
    order_c, ldc = _layout(C_, rows, n, "C")
    pb, pc = _view_ptr(B, "B"), _view_ptr(C_, "C")
    nnz = int(colidx.numel())
    if workspace is None:
        workspace = torch.empty((spmm_workspace_bytes(rows, cols, nnz, n) + 7) // 8, dtype=torch.float64, device=C_.device)
    if not workspace.is_contiguous():
        raise SblasError("workspace must be contiguous")
    wptr = workspace.data_ptr() if workspace.numel() else None
    wbytes = workspace.numel() * workspace.element_size()
    L = lib()
    ap = (_dev_ptr(rowptr, torch.int32, "rowptr"), _dev_ptr(colidx, torch.int32, "colidx") if nnz else None,
          _dev_ptr(val, torch.float64, "val") if nnz else None)
    if plan is not None:
        if plan.rowptr.data_ptr() != rowptr.data_ptr() or plan.colidx.data_ptr() != colidx.data_ptr():
            raise SblasError("the plan was made for another structure")
        rc = L.sblas_hip_spmm_csr_ordered_f64_i32_planned(plan.handle, -1, _stream(stream), rows, cols, nnz, *ap,
                                                          pb if cols else None, ldb, order_b, n, alpha, beta, pc, ldc, order_c,
                                                          wptr, wbytes)
        check(rc, "sblas_hip_spmm_csr_ordered_f64_i32_planned")
    else:
        rc = L.sblas_hip_spmm_csr_ordered(-1, _stream(stream), F64, I32, rows, cols, nnz, *ap, pb if cols else None, ldb,
                                          order_b, n, alpha, beta, pc, ldc, order_c, wptr, wbytes)
        check(rc, "sblas_hip_spmm_csr_ordered")


# ------------------------------------------------------------------------------------------
# transposed products (sblas_hip_csr_transpose_f64_i32, sblas_hip_transpose_plan_* & co.)
# ------------------------------------------------------------------------------------------
TRANSPOSE_SPLIT = 1


def _typed(what, t, dtype):
    """dtype and contiguity first (these wrappers say which is wrong even for a CPU tensor), then _dev_ptr's GPU check"""
    if t.dtype != dtype or not t.is_contiguous():
        raise SblasError("%s must be a contiguous %s tensor" % (what, dtype))


def transpose_workspace_bytes(rows, cols, nnz):
    return int(lib().sblas_hip_csr_transpose_workspace(rows, cols, nnz))


def csr_transpose(rows, cols, rowptr, colidx, val=None, stream=None, with_perm=True):
    """A (rows x cols CSR, int32 indices) as CSC on the device: (colptr, rowidx, valT, perm) torch tensors.  Column c lists
    its entries in CSR order (a stable sort of colidx).  val=None: structure only (valT is None); with_perm=False: perm is
    None.  Allocates its own workspace; stream-ordered, does not synchronise."""
    import torch
    nnz = int(colidx.numel())
    _typed("rowptr", rowptr, torch.int32), _typed("colidx", colidx, torch.int32)
    if val is not None:
        _typed("val", val, torch.float64)
    pr = _dev_ptr(rowptr, torch.int32, "rowptr")
    pc = _dev_ptr(colidx, torch.int32, "colidx") if nnz else None
    pv = _dev_ptr(val, torch.float64, "val") if val is not None and nnz else None
    dev = rowptr.device
    colptr = torch.empty(cols + 1, dtype=torch.int32, device=dev)
    rowidx = torch.empty(nnz, dtype=torch.int32, device=dev)
    valT = torch.empty(nnz, dtype=torch.float64, device=dev) if val is not None else None
    perm = torch.empty(nnz, dtype=torch.int32, device=dev) if with_perm else None
    wsb = transpose_workspace_bytes(rows, cols, nnz)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev) if wsb else None
    rc = lib().sblas_hip_csr_transpose_f64_i32(
        -1, _stream(stream), rows, cols, nnz, pr, pc, pv, colptr.data_ptr(), rowidx.data_ptr() if nnz else None,
        valT.data_ptr() if valT is not None and nnz else None, perm.data_ptr() if perm is not None and nnz else None,
        ws.data_ptr() if ws is not None else None, wsb)
    check(rc, "sblas_hip_csr_transpose_f64_i32")
    return colptr, rowidx, valT, perm


def gather(idx, src, dst, stream=None):
    """dst[i] = src[idx[i]] (sblas_hip_gather_f64)."""
    import torch
    n = int(idx.numel())
    _typed("idx", idx, torch.int32), _typed("src", src, torch.float64), _typed("dst", dst, torch.float64)
    if dst.numel() < n:
        raise SblasError("dst is shorter than idx")
    check(lib().sblas_hip_gather_f64(-1, _stream(stream), n, _dev_ptr(idx, torch.int32, "idx") if n else None,
                                     _dev_ptr(src, torch.float64, "src") if n else None,
                                     _dev_ptr(dst, torch.float64, "dst") if n else None), "sblas_hip_gather_f64")


class _DeviceArray:
    """A view of n elements of a library-owned device array (torch.as_tensor reads __cuda_array_interface__)."""

    def __init__(self, ptr, n, typestr):
        self.__cuda_array_interface__ = dict(shape=(n,), typestr=typestr, data=(ptr, False), version=2, strides=None)


class TransposePlan:
    """A^T of one CSR matrix (sblas_hip_transpose_plan_create): the CSC arrays in the plan's own buffers, an SpMV plan over
    them and, for n > 0, an SpMM plan of width n (split=True: a split SpMM plan).  The plan keeps its own values: after
    val changes, call update_values(val).  destroy() / garbage collection frees the device buffers."""

    def __init__(self, rows, cols, rowptr, colidx, val, n=0, split=False, stream=None):
        import torch
        self.rows, self.cols, self.n = rows, cols, n
        self.nnz = int(colidx.numel())
        self.handle = None
        self.device = rowptr.device
        _typed("rowptr", rowptr, torch.int32), _typed("colidx", colidx, torch.int32), _typed("val", val, torch.float64)
        if val.numel() != self.nnz:
            raise SblasError("val has %d entries, colidx %d" % (val.numel(), self.nnz))
        h = C.c_void_p()
        check(lib().sblas_hip_transpose_plan_create(
            -1, _stream(stream), rows, cols, self.nnz, _dev_ptr(rowptr, torch.int32, "rowptr"),
            _dev_ptr(colidx, torch.int32, "colidx") if self.nnz else None,
            _dev_ptr(val, torch.float64, "val") if self.nnz else None, n, TRANSPOSE_SPLIT if split else 0, C.byref(h)),
            "sblas_hip_transpose_plan_create")
        self.handle = h

    def info(self):
        out = (C.c_int64 * 8)()
        check(lib().sblas_hip_transpose_plan_info(self.handle, out), "sblas_hip_transpose_plan_info")
        return dict(active=bool(out[0]), nnz=int(out[1]), bytes=int(out[2]), spmm_plan=bool(out[3]), n=int(out[4]),
                    spmv_split_rows=int(out[5]), spmm_split_rows=int(out[6]))

    def csc(self):
        """(colptr, rowidx, valT): torch copies of the plan's device arrays."""
        import torch
        cp, ri, vt = C.c_void_p(), C.c_void_p(), C.c_void_p()
        check(lib().sblas_hip_transpose_plan_csc(self.handle, C.byref(cp), C.byref(ri), C.byref(vt)), "sblas_hip_transpose_plan_csc")
        def one(p, n, typestr, dtype):
            if n == 0:
                return torch.empty(0, dtype=dtype, device=self.device)
            if not p.value:          # a matrix without columns: the plan holds nothing, colptr = [0]
                return torch.zeros(n, dtype=dtype, device=self.device)
            return torch.as_tensor(_DeviceArray(p.value, n, typestr), device=self.device).clone()
        out = (one(cp, self.cols + 1, "<i4", torch.int32), one(ri, self.nnz, "<i4", torch.int32),
               one(vt, self.nnz, "<f8", torch.float64))
        return tuple(out)

    def update_values(self, val, stream=None):
        import torch
        _typed("val", val, torch.float64)
        if val.numel() != self.nnz:
            raise SblasError("val has %d entries, the plan %d" % (val.numel(), self.nnz))
        check(lib().sblas_hip_transpose_plan_update_values(self.handle, _stream(stream),
                                                           _dev_ptr(val, torch.float64, "val") if self.nnz else None),
              "sblas_hip_transpose_plan_update_values")

    def spmv(self, x, alpha, beta, y, stream=None):
        """y (cols) = alpha * A^T x (x: rows) + beta * y."""
        import torch
        if x.numel() < self.rows or y.numel() < self.cols:
            raise SblasError("A^T x needs x of %d and y of %d entries" % (self.rows, self.cols))
        check(lib().sblas_hip_spmv_csr_t_f64_i32_planned(self.handle, -1, _stream(stream), _dev_ptr(x, torch.float64, "x"),
                                                         alpha, beta, _dev_ptr(y, torch.float64, "y")),
              "sblas_hip_spmv_csr_t_f64_i32_planned")

    def spmm_ordered(self, B, ldb, order_b, n, alpha, beta, Cmat, ldc, order_c, workspace, stream=None):
        """C (cols x n) = alpha * A^T B (B: rows x n) + beta * C, flat tensors in either order; workspace of at least
        spmm_workspace_bytes(cols, rows, nnz, n) bytes (A^T's shape)."""
        import torch
        rc = lib().sblas_hip_spmm_csr_t_f64_i32_planned(
            self.handle, -1, _stream(stream), _dev_ptr(B, torch.float64, "B") if self.rows else None, ldb, order_b, n, alpha,
            beta, _dev_ptr(Cmat, torch.float64, "C"), ldc, order_c,
            _dev_ptr(workspace, workspace.dtype, "workspace") if workspace is not None and workspace.numel() else None,
            workspace.numel() * workspace.element_size() if workspace is not None else 0)
        check(rc, "sblas_hip_spmm_csr_t_f64_i32_planned")

    def spmm_tensor(self, B, C_, alpha, beta, workspace=None, stream=None):
        """C = alpha * A^T B + beta * C on 2-D tensors; each operand's order and leading dimension come from its strides
        (as spmm_tensor)."""
        import torch
        if B.dim() != 2 or C_.dim() != 2:
            raise SblasError("B and C must be 2-D tensors")
        n = int(C_.shape[1])
        order_b, ldb = _layout(B, self.rows, n, "B")
        order_c, ldc = _layout(C_, self.cols, n, "C")
        pb, pc = _view_ptr(B, "B"), _view_ptr(C_, "C")
        if workspace is None:
            workspace = torch.empty((spmm_workspace_bytes(self.cols, self.rows, self.nnz, n) + 7) // 8, dtype=torch.float64,
                                    device=C_.device)
        if not workspace.is_contiguous():
            raise SblasError("workspace must be contiguous")
        rc = lib().sblas_hip_spmm_csr_t_f64_i32_planned(
            self.handle, -1, _stream(stream), pb if self.rows else None, ldb, order_b, n, alpha, beta, pc, ldc, order_c,
            workspace.data_ptr() if workspace.numel() else None, workspace.numel() * workspace.element_size())
        check(rc, "sblas_hip_spmm_csr_t_f64_i32_planned")

    def destroy(self):
        if self.handle:
            lib().sblas_hip_transpose_plan_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


# ------------------------------------------------------------------------------------------
# CSR from COO triplets (sblas_hip_coo_to_csr_f64_i32, sblas_hip_coo_plan_*)
# ------------------------------------------------------------------------------------------
COO_KEEP, COO_SUM = 0, 1
_DUP = {"keep": COO_KEEP, "sum": COO_SUM}


def _dup(dup):
    if dup not in _DUP:
        raise SblasError("dup must be 'keep' or 'sum', not %r" % (dup,))
    return _DUP[dup]


def _triplets(row, col, val):
    """dtype, contiguity and lengths of a set of triplets (val may be None) -> nnz"""
    import torch
    _typed("row", row, torch.int32), _typed("col", col, torch.int32)
    nnz = int(row.numel())
    if int(col.numel()) != nnz:
        raise SblasError("col has %d entries, row %d" % (col.numel(), nnz))
    if val is not None:
        _typed("val", val, torch.float64)
        if int(val.numel()) != nnz:
            raise SblasError("val has %d entries, row %d" % (val.numel(), nnz))
    return nnz


def coo_workspace_bytes(rows, cols, nnz):
    return int(lib().sblas_hip_coo_to_csr_workspace(rows, cols, nnz))


def coo_to_csr(rows, cols, row, col, val=None, dup="keep", stream=None):
    """CSR of the triplets (row[k], col[k], val[k]) -- any order, duplicates allowed -- as (rowptr, colidx, val, perm,
    runptr) torch tensors on the triplets' device.  Entries are sorted by (row, col), equal pairs in input order
    (numpy.lexsort((col, row))); perm[i] is the input position of sorted position i.  dup="keep": one entry per triplet;
    dup="sum": one entry per distinct (row, col), its run added left to right in input order, runptr[e] the sorted
    position where entry e's run starts.  val=None: structure only (the returned val is None).  Allocates its own
    workspace; stream-ordered.  "sum" trims colidx, val and runptr to the entry count, which it reads back from
    rowptr[rows]: the one place that waits for the device."""
    import torch
    mode = _dup(dup)
    nnz = _triplets(row, col, val)
    pr = _dev_ptr(row, torch.int32, "row") if nnz else None
    pc = _dev_ptr(col, torch.int32, "col") if nnz else None
    pv = _dev_ptr(val, torch.float64, "val") if val is not None and nnz else None
    if not row.is_cuda:
        raise SblasError("row must be a GPU tensor (no CPU path exists)")
    dev = row.device
    with torch.cuda.device(dev):
        rowptr = torch.empty(rows + 1, dtype=torch.int32, device=dev)
        colidx = torch.empty(nnz, dtype=torch.int32, device=dev)
        out = torch.empty(nnz, dtype=torch.float64, device=dev) if val is not None else None
        perm = torch.empty(nnz, dtype=torch.int32, device=dev)
        runptr = torch.empty(nnz + 1, dtype=torch.int32, device=dev)
        wsb = coo_workspace_bytes(rows, cols, nnz)
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev) if wsb else None
        rc = lib().sblas_hip_coo_to_csr_f64_i32(
            -1, _stream(stream), rows, cols, nnz, pr, pc, pv, mode, rowptr.data_ptr(), colidx.data_ptr() if nnz else None,
            out.data_ptr() if out is not None and nnz else None, perm.data_ptr() if nnz else None, runptr.data_ptr(),
            ws.data_ptr() if ws is not None else None, wsb)
        check(rc, "sblas_hip_coo_to_csr_f64_i32")
        if mode == COO_SUM and nnz:
            if stream is not None:
                stream.synchronize()
            count = int(rowptr[rows].item())
            colidx, runptr = colidx[:count], runptr[:count + 1]
            out = out[:count] if out is not None else None
    return rowptr, colidx, out, perm, runptr


def coo_from_torch(t):
    """(rows, cols, row, col, val) of a 2-D fp64 torch.sparse_coo_tensor, coalesced or not: int32 index tensors and the
    values as stored, on the tensor's own device.  Nothing is sorted or summed here: that is coo_to_csr's / CooPlan's
    work (they refuse a CPU tensor)."""
    import torch
    if not isinstance(t, torch.Tensor) or t.layout != torch.sparse_coo:
        raise SblasError("expected a torch.sparse_coo_tensor")
    if t.dim() != 2 or t.sparse_dim() != 2:
        raise SblasError("expected a 2-D sparse tensor with two sparse dimensions")
    if t.dtype != torch.float64:
        raise SblasError("expected float64 values, got %s" % t.dtype)
    rows, cols = int(t.shape[0]), int(t.shape[1])
    idx, val = t._indices(), t._values()
    nnz = int(val.numel())
    if rows >= 1 << 31 or cols >= 1 << 31 or nnz >= 1 << 31:
        raise SblasError("rows, cols and nnz must be below 2^31 (int32 indices)")
    return rows, cols, idx[0].to(torch.int32).contiguous(), idx[1].to(torch.int32).contiguous(), val.contiguous()


class CooPlan:
    """The sorted structure of one set of (row, col) triplets (sblas_hip_coo_plan_create): rowptr, colidx, perm and runptr
    in the plan's own buffers.  assemble(val) turns new triplet values into CSR values with one launch.  Creation checks
    the index ranges on the device and refuses a triplet outside the matrix.  destroy() / garbage collection frees the
    device buffers."""

    def __init__(self, rows, cols, row, col, dup="keep", stream=None):
        import torch
        self.rows, self.cols, self.dup = rows, cols, dup
        self.handle = None
        mode = _dup(dup)
        self.nnz = _triplets(row, col, None)
        self.device = row.device
        h = C.c_void_p()
        pr = _dev_ptr(row, torch.int32, "row") if self.nnz else None
        pc = _dev_ptr(col, torch.int32, "col") if self.nnz else None
        if not row.is_cuda:
            raise SblasError("row must be a GPU tensor (no CPU path exists)")
        with torch.cuda.device(self.device):
            check(lib().sblas_hip_coo_plan_create(-1, _stream(stream), rows, cols, self.nnz, pr, pc, mode, C.byref(h)),
                  "sblas_hip_coo_plan_create")
        self.handle = h
        self.csr_nnz = self.info()["csr_nnz"]

    def info(self):
        out = (C.c_int64 * 8)()
        check(lib().sblas_hip_coo_plan_info(self.handle, out), "sblas_hip_coo_plan_info")
        return dict(rows=int(out[0]), cols=int(out[1]), nnz=int(out[2]), csr_nnz=int(out[3]), longest_run=int(out[4]),
                    passes=int(out[5]), bytes=int(out[6]), dup="sum" if out[7] == COO_SUM else "keep")

    def csr(self):
        """(rowptr, colidx, perm, runptr): torch views of the plan's device arrays; they live as long as the plan."""
        import torch
        ptrs = [C.c_void_p() for _ in range(4)]
        check(lib().sblas_hip_coo_plan_csr(self.handle, *[C.byref(p) for p in ptrs]), "sblas_hip_coo_plan_csr")
        def one(p, n):
            if n == 0:
                return torch.empty(0, dtype=torch.int32, device=self.device)
            return torch.as_tensor(_DeviceArray(p.value, n, "<i4"), device=self.device)
        return tuple(one(p, n) for p, n in zip(ptrs, (self.rows + 1, self.csr_nnz, self.nnz, self.csr_nnz + 1)))

    def assemble(self, val, out=None, stream=None):
        """The CSR values of the triplet values `val` (csr_nnz of them), written to `out` when given.  One launch."""
        import torch
        _typed("val", val, torch.float64)
        if val.numel() != self.nnz:
            raise SblasError("val has %d entries, the plan %d" % (val.numel(), self.nnz))
        if out is None:
            out = torch.empty(self.csr_nnz, dtype=torch.float64, device=val.device)
        _typed("out", out, torch.float64)
        if out.numel() < self.csr_nnz:
            raise SblasError("out has %d entries, the CSR %d" % (out.numel(), self.csr_nnz))
        pv = _dev_ptr(val, torch.float64, "val") if self.nnz else None
        po = _dev_ptr(out, torch.float64, "out") if self.nnz else None
        check(lib().sblas_hip_coo_plan_assemble(self.handle, _stream(stream), pv, po), "sblas_hip_coo_plan_assemble")
        return out

    def destroy(self):
        if self.handle:
            lib().sblas_hip_coo_plan_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


# ------------------------------------------------------------------------------------------
# SpGEMM: C = A * B for two CSR matrices (sblas_hip_spgemm_plan_*)
# ------------------------------------------------------------------------------------------
class SpgemmPlan:
    """The structure of C = A * B (sblas_hip_spgemm_plan_create): A is m x k, B is k x n, both CSR with int32 indices;
    rows may be unsorted and hold duplicates.  Creation checks both structures on the device (a bad one raises), copies
    them, and builds C's rowptr and colidx, which the plan owns.  multiply(val_a, val_b) fills C's values; it allocates
    nothing inside the library and is graph-capturable.  general=True sends every row through the expand / sort / sum
    path; chunk_cap bounds the products of one of its chunks (0: the default).  destroy() / garbage collection frees the
    device buffers."""

    def __init__(self, m, k, n, rowptr_a, colidx_a, rowptr_b, colidx_b, general=False, chunk_cap=0, stream=None):
        import torch
        self.m, self.k, self.n = m, k, n
        self.handle = None
        for name, t in (("rowptr_a", rowptr_a), ("colidx_a", colidx_a), ("rowptr_b", rowptr_b), ("colidx_b", colidx_b)):
            _typed(name, t, torch.int32)
            if not t.is_cuda:
                raise SblasError("%s must be a GPU tensor (no CPU path exists)" % name)
        if rowptr_a.numel() != m + 1 or rowptr_b.numel() != k + 1:
            raise SblasError("rowptr_a needs m + 1 = %d entries and rowptr_b k + 1 = %d" % (m + 1, k + 1))
        self.device = rowptr_a.device
        self.nnz_a, self.nnz_b = int(colidx_a.numel()), int(colidx_b.numel())
        h = C.c_void_p()
        ptr = lambda t: t.data_ptr() if t.numel() else None
        with torch.cuda.device(self.device):
            check(lib().sblas_hip_spgemm_plan_create(-1, _stream(stream), m, k, n, ptr(rowptr_a), ptr(colidx_a), ptr(rowptr_b),
                                                     ptr(colidx_b), SPGEMM_GENERAL if general else SPGEMM_AUTO, int(chunk_cap),
                                                     C.byref(h)), "sblas_hip_spgemm_plan_create")
        self.handle = h
        self.nnz_c = self.info()["nnz_c"]

    def info(self):
        out = (C.c_int64 * 12)()
        check(lib().sblas_hip_spgemm_plan_info(self.handle, out), "sblas_hip_spgemm_plan_info")
        return dict(m=int(out[0]), k=int(out[1]), n=int(out[2]), nnz_c=int(out[3]), products=int(out[4]), rows_row=int(out[5]),
                    rows_general=int(out[6]), chunks=int(out[7]), max_row_products=int(out[8]), b_ascending=bool(out[9]),
                    bytes=int(out[10]), general=out[11] == SPGEMM_GENERAL)

    def csr(self):
        """(rowptr_c, colidx_c): torch views of the plan's device arrays; they live as long as the plan."""
        import torch
        ptrs = [C.c_void_p() for _ in range(2)]
        check(lib().sblas_hip_spgemm_plan_csr(self.handle, *[C.byref(p) for p in ptrs]), "sblas_hip_spgemm_plan_csr")
        def one(p, n):
            if n == 0:
                return torch.empty(0, dtype=torch.int32, device=self.device)
            return torch.as_tensor(_DeviceArray(p.value, n, "<i4"), device=self.device)
        return tuple(one(p, n) for p, n in zip(ptrs, (self.m + 1, self.nnz_c)))

    def multiply(self, val_a, val_b, out=None, stream=None):
        """C's values (nnz_c of them) for the values val_a and val_b in A's and B's stored order, written to `out` when
        given."""
        import torch
        _typed("val_a", val_a, torch.float64), _typed("val_b", val_b, torch.float64)
        if val_a.numel() != self.nnz_a or val_b.numel() != self.nnz_b:
            raise SblasError("val_a / val_b have %d / %d entries, the plan %d / %d" % (val_a.numel(), val_b.numel(), self.nnz_a, self.nnz_b))
        if out is None:
            out = torch.empty(self.nnz_c, dtype=torch.float64, device=self.device)
        _typed("out", out, torch.float64)
        if out.numel() < self.nnz_c:
            raise SblasError("out has %d entries, C %d" % (out.numel(), self.nnz_c))
        if self.nnz_c:
            pa, pb, po = _dev_ptr(val_a, torch.float64, "val_a"), _dev_ptr(val_b, torch.float64, "val_b"), _dev_ptr(out, torch.float64, "out")
        else:
            pa = pb = po = None
        check(lib().sblas_hip_spgemm_plan_numeric(self.handle, _stream(stream), pa, pb, po), "sblas_hip_spgemm_plan_numeric")
        return out

    def destroy(self):
        if self.handle:
            lib().sblas_hip_spgemm_plan_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def spgemm(A, B, stream=None):
    """C = A * B, one shot: A = (m, k, rowptr, colidx, val) and B = (k, n, rowptr, colidx, val) as GPU tensors -> (rowptr_c,
    colidx_c, val_c), tensors of their own (the plan made here is destroyed before returning)."""
    m, k, rowptr_a, colidx_a, val_a = A
    kb, n, rowptr_b, colidx_b, val_b = B
    if k != kb:
        raise SblasError("A is %d x %d, B is %d x %d" % (m, k, kb, n))
    plan = SpgemmPlan(m, k, n, rowptr_a, colidx_a, rowptr_b, colidx_b, stream=stream)
    try:
        rowptr_c, colidx_c = plan.csr()
        val_c = plan.multiply(val_a, val_b, stream=stream)
        rowptr_c, colidx_c = rowptr_c.clone(), colidx_c.clone()
        if stream is not None:
            stream.synchronize()
        else:
            import torch
            torch.cuda.current_stream().synchronize()
    finally:
        plan.destroy()
    return rowptr_c, colidx_c, val_c


# ------------------------------------------------------------------------------------------
# GEAM: C = alpha * A + beta * B for two CSR matrices (sblas_hip_geam_plan_*)
# ------------------------------------------------------------------------------------------
class GeamPlan:
    """The structure of C = alpha * A + beta * B (sblas_hip_geam_plan_create): A and B are rows x cols CSR with int32
    indices; rows may be unsorted and hold duplicates.  Creation checks both structures on the device (a bad one raises)
    and builds C's rowptr and colidx and the maps dest_a / dest_b, which the plan owns; it keeps neither A's nor B's
    structure.  add(val_a, val_b, alpha, beta) fills C's values; it allocates nothing inside the library and is
    graph-capturable.  When every row of both operands is strictly ascending the plan takes the sorted path (one launch
    over C's entries; scatter=True keeps the two-launch ordered scatter over the maps instead, the same bits, slower where
    entries match: DESIGN.md 3.34); otherwise, or with general=True, it owns a CooPlan-like sort of the concatenated triplets.
    destroy() / garbage collection frees the device buffers.

    A time step on two assembled matrices, M + dt K with new values every step:
        m, k = CooPlan(n, n, mrow, mcol, dup="sum"), CooPlan(n, n, krow, kcol, dup="sum")
        plan = GeamPlan(n, n, m.csr()[0], m.csr()[1], k.csr()[0], k.csr()[1])
        rowptr, colidx = plan.csr()                          # what Ilu0Plan / AmgPlan / KrylovPlan are built on
        val = plan.add(m.assemble(mval), k.assemble(kval), 1.0, dt)
    A shift A + sigma I:
        eye = torch.arange(n + 1, dtype=torch.int32, device=dev)
        plan = GeamPlan(n, n, rowptr, colidx, eye, eye[:n])
        val = plan.add(val_a, torch.ones(n, dtype=torch.float64, device=dev), 1.0, sigma)
    Symmetrising, A + A^T on the transpose plan's arrays:
        t = TransposePlan(n, n, rowptr, colidx, val_a)
        colptr, rowidx, val_t = t.csc()
        plan = GeamPlan(n, n, rowptr, colidx, colptr, rowidx)
        val = plan.add(val_a, val_t)"""

    def __init__(self, rows, cols, rowptr_a, colidx_a, rowptr_b, colidx_b, general=False, stream=None, scatter=False):
        import torch
        self.rows, self.cols = rows, cols
        if general and scatter:
            raise SblasError("scatter is a form of the sorted path: general and scatter exclude each other")
        self.handle = None
        for name, t in (("rowptr_a", rowptr_a), ("colidx_a", colidx_a), ("rowptr_b", rowptr_b), ("colidx_b", colidx_b)):
            if not isinstance(t, torch.Tensor):
                raise SblasError("%s must be a GPU tensor (no CPU path exists)" % name)
            _typed(name, t, torch.int32)
        if rowptr_a.numel() != rows + 1 or rowptr_b.numel() != rows + 1:
            raise SblasError("rowptr_a and rowptr_b need rows + 1 = %d entries, not %d and %d" % (rows + 1, rowptr_a.numel(), rowptr_b.numel()))
        for name, t in (("rowptr_a", rowptr_a), ("colidx_a", colidx_a), ("rowptr_b", rowptr_b), ("colidx_b", colidx_b)):
            if not t.is_cuda:
                raise SblasError("%s must be a GPU tensor (no CPU path exists)" % name)
            if t.device != rowptr_a.device:
                raise SblasError("%s is on %s, rowptr_a on %s" % (name, t.device, rowptr_a.device))
        self.device = rowptr_a.device
        self.nnz_a, self.nnz_b = int(colidx_a.numel()), int(colidx_b.numel())
        h = C.c_void_p()
        ptr = lambda t: t.data_ptr() if t.numel() else None
        with torch.cuda.device(self.device):
            with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
                ends = (int(rowptr_a[rows].item()), int(rowptr_b[rows].item()))   # the library reads colidx as far as rowptr says
            if ends != (self.nnz_a, self.nnz_b):
                raise SblasError("colidx_a / colidx_b have %d / %d entries, the row pointers end at %d / %d" % ((self.nnz_a, self.nnz_b) + ends))
            check(lib().sblas_hip_geam_plan_create(-1, _stream(stream), rows, cols, ptr(rowptr_a), ptr(colidx_a), ptr(rowptr_b), ptr(colidx_b),
                                                   GEAM_GENERAL if general else GEAM_SCATTER if scatter else GEAM_AUTO, C.byref(h)),
                  "sblas_hip_geam_plan_create")
        self.handle = h
        self.nnz_c = self.info()["nnz_c"]

    def info(self):
        out = (C.c_int64 * 12)()
        check(lib().sblas_hip_geam_plan_info(self.handle, out), "sblas_hip_geam_plan_info")
        return dict(rows=int(out[0]), cols=int(out[1]), nnz_a=int(out[2]), nnz_b=int(out[3]), nnz_c=int(out[4]), matched=int(out[5]),
                    path="sorted" if out[6] == GEAM_PATH_SORTED else "general", a_ascending=bool(out[7]), b_ascending=bool(out[8]),
                    launches=int(out[9]), bytes=int(out[10]), general=out[11] == GEAM_GENERAL,
                    scatter=out[11] == GEAM_SCATTER)

    def _views(self, call, what, sizes):
        import torch
        ptrs = [C.c_void_p() for _ in sizes]
        check(call(self.handle, *[C.byref(p) for p in ptrs]), what)
        def one(p, n):
            if n == 0:
                return torch.empty(0, dtype=torch.int32, device=self.device)
            return torch.as_tensor(_DeviceArray(p.value, n, "<i4"), device=self.device)
        return tuple(one(p, n) for p, n in zip(ptrs, sizes))

    def csr(self):
        """(rowptr_c, colidx_c): torch views of the plan's device arrays; they live as long as the plan."""
        return self._views(lib().sblas_hip_geam_plan_csr, "sblas_hip_geam_plan_csr", (self.rows + 1, self.nnz_c))

    def maps(self):
        """(dest_a, dest_b): the entry of C where each entry of A and of B lands; torch views that live as long as the plan."""
        return self._views(lib().sblas_hip_geam_plan_maps, "sblas_hip_geam_plan_maps", (self.nnz_a, self.nnz_b))

    def add(self, val_a, val_b, alpha=1.0, beta=1.0, out=None, stream=None):
        """C's values (nnz_c of them) for the values val_a and val_b in A's and B's stored order, written to `out` when
        given; `out` may not overlap val_a or val_b."""
        import torch
        _typed("val_a", val_a, torch.float64), _typed("val_b", val_b, torch.float64)
        if val_a.numel() != self.nnz_a or val_b.numel() != self.nnz_b:
            raise SblasError("val_a / val_b have %d / %d entries, the plan %d / %d" % (val_a.numel(), val_b.numel(), self.nnz_a, self.nnz_b))
        if out is None:
            out = torch.empty(self.nnz_c, dtype=torch.float64, device=self.device)
        _typed("out", out, torch.float64)
        if out.numel() < self.nnz_c:
            raise SblasError("out has %d entries, C %d" % (out.numel(), self.nnz_c))
        pa = _dev_ptr(val_a, torch.float64, "val_a") if self.nnz_a else None
        pb = _dev_ptr(val_b, torch.float64, "val_b") if self.nnz_b else None
        po = _dev_ptr(out, torch.float64, "out") if self.nnz_c else None
        check(lib().sblas_hip_geam_plan_numeric(self.handle, _stream(stream), pa, pb, float(alpha), float(beta), po),
              "sblas_hip_geam_plan_numeric")
        return out

    def destroy(self):
        if self.handle:
            lib().sblas_hip_geam_plan_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def csr_add(A, B, alpha=1.0, beta=1.0, stream=None):
    """C = alpha * A + beta * B, one shot: A = (rows, cols, rowptr, colidx, val) and B likewise as GPU tensors -> (rowptr_c,
    colidx_c, val_c), tensors of their own (the plan made here is destroyed before returning)."""
    rows, cols, rowptr_a, colidx_a, val_a = A
    rows_b, cols_b, rowptr_b, colidx_b, val_b = B
    if rows != rows_b or cols != cols_b:
        raise SblasError("A is %d x %d, B is %d x %d" % (rows, cols, rows_b, cols_b))
    import torch
    plan = GeamPlan(rows, cols, rowptr_a, colidx_a, rowptr_b, colidx_b, stream=stream)
    try:
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(plan.device)):
            rowptr_c, colidx_c = plan.csr()                  # val_c is allocated, and the copies are made, on the stream that adds
            val_c = plan.add(val_a, val_b, alpha, beta, stream=torch.cuda.current_stream())
            rowptr_c, colidx_c = rowptr_c.clone(), colidx_c.clone()
            torch.cuda.current_stream().synchronize()
    finally:
        plan.destroy()
    return rowptr_c, colidx_c, val_c


# ------------------------------------------------------------------------------------------
# Masked SpGEMM: out = M o (X Y^T) on a CSR pattern (sblas_hip_mspgemm_plan_*)
# ------------------------------------------------------------------------------------------
class MaskedSpgemmPlan:
    """out = M o (X Y^T) (sblas_hip_mspgemm_plan_create): the product of two sparse matrices evaluated only on a pattern.
    X is m x k and Y n x k, both CSR with int32 indices; the mask is an m x n CSR pattern; rows of all three may be unsorted
    and hold duplicates.  Creation checks the three structures on the device (a bad one raises) and copies them, so the
    plan keeps none of the caller's arrays.  multiply(val_x, val_y) fills one double per stored mask entry, in the mask's
    stored order: the products x * y over the columns X's row i and Y's row j share, added left to right in X's stored
    order (include/sblas_hip_mspgemm.h has the contract); it allocates nothing inside the library and is graph-capturable.
    When every row of X and of Y is strictly ascending the plan takes the sorted path (a lane per mask entry walks the
    shorter row and binary-searches the longer); otherwise, or with general=True, the general path, which is quadratic in
    the row lengths: the slow path.  destroy() / garbage collection frees the device buffers.

    SpGEMM's values on its own pattern, bit for bit (the contract's order is SpGEMM's):
        c = SpgemmPlan(m, k, n, rowptr_a, colidx_a, rowptr_b, colidx_b)
        colptr, rowidx, val_t = TransposePlan(k, n, rowptr_b, colidx_b, val_b).csc()
        plan = MaskedSpgemmPlan(m, n, k, *c.csr(), rowptr_a, colidx_a, colptr, rowidx)
        val_c = plan.multiply(val_a, val_t)
    The gradient of C = A B with respect to A's values, dA = (dC B^T) on A's pattern:
        plan = MaskedSpgemmPlan(m, k, n, rowptr_a, colidx_a, *c.csr(), rowptr_b, colidx_b)
        d_val_a = plan.multiply(d_val_c, val_b)"""

    def __init__(self, m, n, k, rowptr_m, colidx_m, rowptr_x, colidx_x, rowptr_y, colidx_y, general=False, stream=None):
        import torch
        self.m, self.n, self.k = m, n, k
        self.handle = None
        named = (("rowptr_m", rowptr_m), ("colidx_m", colidx_m), ("rowptr_x", rowptr_x), ("colidx_x", colidx_x), ("rowptr_y", rowptr_y),
                 ("colidx_y", colidx_y))
        for name, t in named:
            if not isinstance(t, torch.Tensor):
                raise SblasError("%s must be a GPU tensor (no CPU path exists)" % name)
            _typed(name, t, torch.int32)
        if rowptr_m.numel() != m + 1 or rowptr_x.numel() != m + 1 or rowptr_y.numel() != n + 1:
            raise SblasError("rowptr_m and rowptr_x need m + 1 = %d entries and rowptr_y n + 1 = %d, not %d, %d and %d"
                             % (m + 1, n + 1, rowptr_m.numel(), rowptr_x.numel(), rowptr_y.numel()))
        for name, t in named:
            if not t.is_cuda:
                raise SblasError("%s must be a GPU tensor (no CPU path exists)" % name)
            if t.device != rowptr_m.device:
                raise SblasError("%s is on %s, rowptr_m on %s" % (name, t.device, rowptr_m.device))
        self.device = rowptr_m.device
        self.nnz_m, self.nnz_x, self.nnz_y = int(colidx_m.numel()), int(colidx_x.numel()), int(colidx_y.numel())
        h = C.c_void_p()
        ptr = lambda t: t.data_ptr() if t.numel() else None
        with torch.cuda.device(self.device):
            with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
                ends = tuple(int(v) for v in torch.stack((rowptr_m[m], rowptr_x[m], rowptr_y[n])).tolist())   # the library reads colidx as far as rowptr says
            if ends != (self.nnz_m, self.nnz_x, self.nnz_y):
                raise SblasError("colidx_m / colidx_x / colidx_y have %d / %d / %d entries, the row pointers end at %d / %d / %d"
                                 % ((self.nnz_m, self.nnz_x, self.nnz_y) + ends))
            check(lib().sblas_hip_mspgemm_plan_create(-1, _stream(stream), m, n, k, ptr(rowptr_m), ptr(colidx_m), ptr(rowptr_x), ptr(colidx_x),
                                                      ptr(rowptr_y), ptr(colidx_y), MSPGEMM_GENERAL if general else MSPGEMM_AUTO, C.byref(h)),
                  "sblas_hip_mspgemm_plan_create")
        self.handle = h

    def info(self):
        out = (C.c_int64 * 12)()
        check(lib().sblas_hip_mspgemm_plan_info(self.handle, out), "sblas_hip_mspgemm_plan_info")
        return dict(m=int(out[0]), n=int(out[1]), k=int(out[2]), nnz_m=int(out[3]), nnz_x=int(out[4]), nnz_y=int(out[5]),
                    path="sorted" if out[6] == MSPGEMM_PATH_SORTED else "general", x_ascending=bool(out[7]), y_ascending=bool(out[8]),
                    launches=int(out[9]), bytes=int(out[10]), general=out[11] == MSPGEMM_GENERAL)

    def multiply(self, val_x, val_y, out=None, stream=None):
        """The masked product's values (nnz_m of them, in the mask's stored order) for the values val_x and val_y in X's
        and Y's stored order, written to `out` when given; `out` may not overlap val_x or val_y."""
        import torch
        for name, t in (("val_x", val_x), ("val_y", val_y)):
            if not isinstance(t, torch.Tensor):
                raise SblasError("%s must be a GPU tensor (no CPU path exists)" % name)
            _typed(name, t, torch.float64)
        if val_x.numel() != self.nnz_x or val_y.numel() != self.nnz_y:
            raise SblasError("val_x / val_y have %d / %d entries, the plan %d / %d" % (val_x.numel(), val_y.numel(), self.nnz_x, self.nnz_y))
        if out is None:
            out = torch.empty(self.nnz_m, dtype=torch.float64, device=self.device)
        _typed("out", out, torch.float64)
        if out.numel() < self.nnz_m:
            raise SblasError("out has %d entries, the mask %d" % (out.numel(), self.nnz_m))
        for name, t in (("val_x", val_x), ("val_y", val_y), ("out", out)):
            if t.is_cuda and t.device != self.device:
                raise SblasError("%s is on %s, the plan on %s" % (name, t.device, self.device))
        px = _dev_ptr(val_x, torch.float64, "val_x") if self.nnz_x else None
        py = _dev_ptr(val_y, torch.float64, "val_y") if self.nnz_y else None
        po = _dev_ptr(out, torch.float64, "out") if self.nnz_m else None
        check(lib().sblas_hip_mspgemm_plan_numeric(self.handle, _stream(stream), px, py, po), "sblas_hip_mspgemm_plan_numeric")
        return out

    def destroy(self):
        if self.handle:
            lib().sblas_hip_mspgemm_plan_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def masked_spgemm(mask, X, Y, stream=None):
    """out = M o (X Y^T), one shot: mask = (m, n, rowptr, colidx), X = (m, k, rowptr, colidx, val) and Y = (n, k, rowptr,
    colidx, val) as GPU tensors -> one double per stored mask entry (the plan made here is destroyed before returning)."""
    m, n, rowptr_m, colidx_m = mask
    mx, k, rowptr_x, colidx_x, val_x = X
    ny, ky, rowptr_y, colidx_y, val_y = Y
    if mx != m or ny != n or ky != k:
        raise SblasError("the mask is %d x %d, X is %d x %d and Y %d x %d: X Y^T is %d x %d" % (m, n, mx, k, ny, ky, mx, ny))
    import torch
    plan = MaskedSpgemmPlan(m, n, k, rowptr_m, colidx_m, rowptr_x, colidx_x, rowptr_y, colidx_y, stream=stream)
    try:
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(plan.device)):
            out = plan.multiply(val_x, val_y, stream=torch.cuda.current_stream())     # out is allocated on the stream that multiplies
            torch.cuda.current_stream().synchronize()
    finally:
        plan.destroy()
    return out


def _structure(n, rowptr, colidx):
    """the checks every structure plan makes on (rowptr, colidx) before the library sees them -> nnz"""
    import torch
    for name, t in (("rowptr", rowptr), ("colidx", colidx)):
        if not isinstance(t, torch.Tensor):
            raise SblasError("%s must be a torch tensor" % name)
        _typed(name, t, torch.int32)
        if not t.is_cuda:
            raise SblasError("%s must be a GPU tensor (no CPU path exists)" % name)
    if rowptr.numel() != n + 1:
        raise SblasError("rowptr has %d entries for %d rows" % (rowptr.numel(), n))
    return int(colidx.numel())


# ------------------------------------------------------------------------------------------
# Sparse triangular solves: T x = alpha b, T X = alpha B (sblas_hip_sptrsv_plan_*)
# ------------------------------------------------------------------------------------------
class SptrsvPlan:
    """The level schedule of one triangle of a square CSR matrix (sblas_hip_sptrsv_plan_create): the lower (lower=True) or
    upper triangle of the n x n matrix (rowptr, colidx), int32 indices; rows may be unsorted, off-diagonal duplicates add,
    and stored entries in the other triangle are ignored.  unit_diag=True ignores stored diagonals and uses 1; otherwise
    every row needs exactly one.  A bad structure raises an SblasError that names the first bad row (.bad_row).  The plan
    keeps rowptr and colidx alive and solves on them as they are: do not change them.  mode: "auto" (a level above
    chain_rows rows is one launch, a run of narrower levels one single-workgroup launch), "per_level" or "chain";
    chain_rows=0 takes the default.  solve() allocates nothing inside the library and is graph-capturable.
    solve_multi() is the tiled solve of an (n, nrhs) block (include/sblas_hip_sptrsm_tile.h): column j has exactly the bits
    of solve() on column j, in solve()'s launches whatever nrhs is; solve()'s own 2-D path keeps its older kernels.  The
    transposed solve: a plan with the opposite `lower` on TransposePlan.csc()'s (colptr, rowidx), solved with its valT."""

    def __init__(self, n, rowptr, colidx, lower=True, unit_diag=False, mode="auto", chain_rows=0, stream=None):
        import torch
        self.n, self.lower, self.unit_diag, self.mode = n, bool(lower), bool(unit_diag), mode
        self.handle = None
        flags = _sptrsv_mode(mode)
        self.nnz = _structure(n, rowptr, colidx)
        self.rowptr, self.colidx = rowptr, colidx
        self.device = rowptr.device
        h, bad = C.c_void_p(), C.c_int64(-1)
        with torch.cuda.device(self.device):
            rc = lib().sblas_hip_sptrsv_plan_create(-1, _stream(stream), n, self.nnz, rowptr.data_ptr(),
                                                    colidx.data_ptr() if self.nnz else None,
                                                    FILL_LOWER if lower else FILL_UPPER, DIAG_UNIT if unit_diag else DIAG_NON_UNIT,
                                                    flags, int(chain_rows), C.byref(h), C.byref(bad))
        if rc != 0:
            raise _bad_structure("sblas_hip_sptrsv_plan_create", rc, bad.value)
        self.handle = h

    def info(self):
        out = (C.c_int64 * 12)()
        check(lib().sblas_hip_sptrsv_plan_info(self.handle, out), "sblas_hip_sptrsv_plan_info")
        return dict(n=int(out[0]), nnz=int(out[1]), lower=out[2] == FILL_LOWER, unit_diag=out[3] == DIAG_UNIT, levels=int(out[4]),
                    launches=int(out[5]), wide_launches=int(out[6]), chain_launches=int(out[7]), widest_level=int(out[8]),
                    longest_row=int(out[9]), bytes=int(out[10]), mode=[k for k, v in _SPTRSV_MODE.items() if v == out[11]][0])

    def levels(self):
        """(perm, level_ptr): torch views of the plan's device arrays -- the rows ordered by (level, row), and level l as
        perm[level_ptr[l] : level_ptr[l + 1]]; they live as long as the plan."""
        import torch
        ptrs = [C.c_void_p() for _ in range(2)]
        check(lib().sblas_hip_sptrsv_plan_order(self.handle, *[C.byref(p) for p in ptrs]), "sblas_hip_sptrsv_plan_order")
        if self.n == 0:
            return torch.empty(0, dtype=torch.int32, device=self.device), torch.zeros(1, dtype=torch.int32, device=self.device)
        lv = self.info()["levels"]
        return tuple(torch.as_tensor(_DeviceArray(p.value, k, "<i4"), device=self.device) for p, k in zip(ptrs, (self.n, lv + 1)))

    def solve(self, val, b, x=None, alpha=1.0, stream=None):
        """x with T x = alpha * b for the values val (in stored order).  A 1-D b of n entries is one right-hand side
        (SpSV); a 2-D n x nrhs b with strides (ld, 1) is nrhs of them (SpSM), read by its stride.  x: like b (x is b: in
        place); made here when None.  Returns x."""
        import torch
        for name, t in (("val", val), ("b", b)) + ((("x", x),) if x is not None else ()):
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise SblasError("%s must be a GPU tensor (no CPU path exists)" % name)
            if t.dtype != torch.float64:
                raise SblasError("%s must be float64, got %s" % (name, t.dtype))
        if not val.is_contiguous() or val.numel() != self.nnz:
            raise SblasError("val must be contiguous with one value per stored entry (%d), got %d" % (self.nnz, val.numel()))
        if b.dim() not in (1, 2) or b.shape[0] != self.n:
            raise SblasError("b must hold %d entries or be %d x nrhs, got shape %s" % (self.n, self.n, tuple(b.shape)))
        if x is None:
            x = torch.empty(tuple(b.shape), dtype=torch.float64, device=self.device)
        if tuple(x.shape) != tuple(b.shape):
            raise SblasError("x has shape %s, b %s" % (tuple(x.shape), tuple(b.shape)))
        pr, pc = self.rowptr.data_ptr(), (self.colidx.data_ptr() if self.nnz else None)
        pv = val.data_ptr() if self.nnz else None
        if b.dim() == 1:
            for name, t in (("b", b), ("x", x)):
                if self.n > 1 and t.stride(0) != 1:
                    raise SblasError("%s must be contiguous" % name)
            check(lib().sblas_hip_sptrsv_f64_i32_planned(self.handle, _stream(stream), pr, pc, pv, float(alpha),
                                                         b.data_ptr() if self.n else None, x.data_ptr() if self.n else None),
                  "sblas_hip_sptrsv_f64_i32_planned")
            return x
        nrhs = int(b.shape[1])
        ld = []
        for name, t in (("b", b), ("x", x)):
            if self.n > 0 and nrhs > 1 and t.stride(1) != 1:               # without rows there are no strides to read
                raise SblasError("%s must be row-major (strides (ld, 1)), got strides %s" % (name, tuple(t.stride())))
            l = int(t.stride(0)) if self.n > 1 else max(nrhs, 1)
            if l < nrhs:
                raise SblasError("%s has a leading dimension of %d for %d columns" % (name, l, nrhs))
            ld.append(max(l, 1))
        live = self.n > 0 and nrhs > 0
        check(lib().sblas_hip_sptrsm_f64_i32_planned(self.handle, _stream(stream), pr, pc, pv, nrhs, float(alpha),
                                                     b.data_ptr() if live else None, ld[0], x.data_ptr() if live else None, ld[1]),
              "sblas_hip_sptrsm_f64_i32_planned")
        return x

    def solve_multi(self, val, B, X=None, alpha=1.0, stream=None):
        """X with T X = alpha * B by the tiled solve (sblas_hip_sptrsm_tiled_f64_i32_planned): B an (n, nrhs) float64
        tensor with strides (ld, 1), and X[:, j] has EXACTLY the bits solve(val, B[:, j]) gives, for every nrhs, leading
        dimension, alignment and mode.  The 2-D checks and refusals of solve().  X: like B, made here when None; X is B
        solves in place.  The launches are solve()'s on one right-hand side, whatever nrhs is.  Returns X."""
        import torch
        for name, t in (("val", val), ("B", B)) + ((("X", X),) if X is not None else ()):
            if not isinstance(t, torch.Tensor) or not t.is_cuda:
                raise SblasError("%s must be a GPU tensor (no CPU path exists)" % name)
            if t.dtype != torch.float64:
                raise SblasError("%s must be float64, got %s" % (name, t.dtype))
            if t.device != self.device:
                raise SblasError("%s is on %s, the plan on %s" % (name, t.device, self.device))
        if not val.is_contiguous() or val.numel() != self.nnz:
            raise SblasError("val must be contiguous with one value per stored entry (%d), got %d" % (self.nnz, val.numel()))
        if B.dim() != 2 or B.shape[0] != self.n:
            raise SblasError("B must be %d x nrhs, got shape %s" % (self.n, tuple(B.shape)))
        if X is None:
            X = torch.empty(tuple(B.shape), dtype=torch.float64, device=self.device)
        if tuple(X.shape) != tuple(B.shape):
            raise SblasError("X has shape %s, B %s" % (tuple(X.shape), tuple(B.shape)))
        nrhs = int(B.shape[1])
        ld = []
        for name, t in (("B", B), ("X", X)):
            if self.n > 0 and nrhs > 1 and t.stride(1) != 1:               # without rows there are no strides to read
                raise SblasError("%s must be row-major (strides (ld, 1)), got strides %s" % (name, tuple(t.stride())))
            l = int(t.stride(0)) if self.n > 1 else max(nrhs, 1)
            if l < nrhs:
                raise SblasError("%s has a leading dimension of %d for %d columns" % (name, l, nrhs))
            ld.append(max(l, 1))
        live = self.n > 0 and nrhs > 0
        if live and X is not B and X.data_ptr() == B.data_ptr() and ld[0] != ld[1]:
            raise SblasError("in place needs equal leading dimensions, got %d and %d" % (ld[0], ld[1]))
        with torch.cuda.device(self.device):
            check(lib().sblas_hip_sptrsm_tiled_f64_i32_planned(self.handle, _stream(stream), self.rowptr.data_ptr(),
                                                               self.colidx.data_ptr() if self.nnz else None,
                                                               val.data_ptr() if self.nnz else None, nrhs, float(alpha),
                                                               B.data_ptr() if live else None, ld[0], X.data_ptr() if live else None, ld[1]),
                  "sblas_hip_sptrsm_tiled_f64_i32_planned")
        return X

    def destroy(self):
        if self.handle:
            lib().sblas_hip_sptrsv_plan_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def sptrsm_tile_limits():
    """The tiled SpSM's sizes (sblas_sptrsm_tile_limits): dict(tile, wide_threads, chain_threads, max_grid)."""
    out = (C.c_int64 * 4)()
    check(lib().sblas_sptrsm_tile_limits(out), "sblas_sptrsm_tile_limits")
    return dict(tile=int(out[0]), wide_threads=int(out[1]), chain_threads=int(out[2]), max_grid=int(out[3]))


def sptrsm_tile_grid(units, nrhs):
    """Workgroups of one wide launch of the tiled SpSM (sblas_sptrsm_tile_grid): dict(unit_blocks, tiles, grid, last_tile);
    a chain launch is `tiles` workgroups."""
    out = (C.c_int64 * 4)()
    check(lib().sblas_sptrsm_tile_grid(int(units), int(nrhs), out), "sblas_sptrsm_tile_grid")
    return dict(unit_blocks=int(out[0]), tiles=int(out[1]), grid=int(out[2]), last_tile=int(out[3]))


def sptrsv(A, b, lower=True, unit_diag=False, alpha=1.0, stream=None):
    """x with T x = alpha * b, one shot: A = (n, rowptr, colidx, val) as GPU tensors, T its lower or upper triangle; b 1-D,
    or 2-D for several right-hand sides.  The plan made here is destroyed before returning."""
    n, rowptr, colidx, val = A
    plan = SptrsvPlan(n, rowptr, colidx, lower=lower, unit_diag=unit_diag, stream=stream)
    try:
        x = plan.solve(val, b, alpha=alpha, stream=stream)
        if stream is not None:
            stream.synchronize()
        else:
            import torch
            torch.cuda.current_stream().synchronize()
    finally:
        plan.destroy()
    return x


# ------------------------------------------------------------------------------------------
# ILU(0) on the device: lu = ILU0(A) on A's own pattern (sblas_hip_ilu0_plan_*)
# ------------------------------------------------------------------------------------------
class Ilu0Plan:
    """The level schedule of ILU(0) of the square n x n CSR matrix (rowptr, colidx), int32 indices
    (sblas_hip_ilu0_plan_create).  Every row must be strictly ascending in column and store its diagonal; a bad
    structure raises an SblasError that names the first bad row (.bad_row).  The plan keeps rowptr and colidx alive and
    factors on them as they are: do not change them.  mode and chain_rows as for SptrsvPlan.  factor() allocates nothing
    inside the library and is graph-capturable; its bits are a function of val and the pattern alone."""

    def __init__(self, n, rowptr, colidx, mode="auto", chain_rows=0, stream=None):
        import torch
        self.n, self.mode = n, mode
        self.handle = None
        self._solvers = None
        flags = _sptrsv_mode(mode)
        self.nnz = _structure(n, rowptr, colidx)
        self.rowptr, self.colidx = rowptr, colidx
        self.device = rowptr.device
        h, bad = C.c_void_p(), C.c_int64(-1)
        with torch.cuda.device(self.device):
            rc = lib().sblas_hip_ilu0_plan_create(-1, _stream(stream), n, self.nnz, rowptr.data_ptr(),
                                                  colidx.data_ptr() if self.nnz else None, flags, int(chain_rows),
                                                  C.byref(h), C.byref(bad))
        if rc != 0:
            raise _bad_structure("sblas_hip_ilu0_plan_create", rc, bad.value)
        self.handle = h

    def info(self):
        out = (C.c_int64 * 12)()
        check(lib().sblas_hip_ilu0_plan_info(self.handle, out), "sblas_hip_ilu0_plan_info")
        return dict(n=int(out[0]), nnz=int(out[1]), levels=int(out[2]), launches=int(out[3]), wide_launches=int(out[4]),
                    chain_launches=int(out[5]), widest_level=int(out[6]), longest_row=int(out[7]), long_rows=int(out[8]),
                    bytes=int(out[9]), mode=[k for k, v in _SPTRSV_MODE.items() if v == out[10]][0], chain_rows=int(out[11]))

    def diag(self):
        """The position of each row's diagonal in val and lu: a torch view (int32, n) of the plan's device array; it
        lives as long as the plan."""
        import torch
        if self.n == 0:
            return torch.empty(0, dtype=torch.int32, device=self.device)
        p = C.c_void_p()
        check(lib().sblas_hip_ilu0_plan_diag(self.handle, C.byref(p)), "sblas_hip_ilu0_plan_diag")
        return torch.as_tensor(_DeviceArray(p.value, self.n, "<i4"), device=self.device)

    def _values(self, name, t):
        import torch
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise SblasError("%s must be a GPU tensor (no CPU path exists)" % name)
        if t.dtype != torch.float64:
            raise SblasError("%s must be float64, got %s" % (name, t.dtype))
        if t.dim() != 1 or not t.is_contiguous() or t.numel() != self.nnz:
            raise SblasError("%s must be contiguous with one value per stored entry (%d), got %d" % (name, self.nnz, t.numel()))

    def factor(self, val, out=None, stream=None):
        """lu = ILU0(A) for the values val (in stored order): L's strictly-lower entries and U's diagonal and upper
        entries on A's pattern.  out: made here when None; out is val factors in place.  Returns out."""
        import torch
        self._values("val", val)
        if out is None:
            out = torch.empty(self.nnz, dtype=torch.float64, device=self.device)
        self._values("out", out)
        check(lib().sblas_hip_ilu0_f64_i32_planned(self.handle, _stream(stream), self.rowptr.data_ptr(),
                                                   self.colidx.data_ptr() if self.nnz else None,
                                                   val.data_ptr() if self.nnz else None, out.data_ptr() if self.nnz else None),
              "sblas_hip_ilu0_f64_i32_planned")
        return out

    def pivots(self, lu, out=None, stream=None):
        """U's diagonal, lu[diag()], by one gather; a zero, Inf or NaN in it is what factor() does not report."""
        import torch
        self._values("lu", lu)
        if out is None:
            out = torch.empty(self.n, dtype=torch.float64, device=self.device)
        if self.n:
            gather(self.diag(), lu, out, stream=stream)
        return out

    def solvers(self):
        """(lower, upper): the two SptrsvPlans on the plan's own arrays that consume a factor -- L with its unit diagonal
        implied, U with its stored one.  Made at the first call and kept until destroy()."""
        if self._solvers is None:
            lower = SptrsvPlan(self.n, self.rowptr, self.colidx, lower=True, unit_diag=True)
            try:
                upper = SptrsvPlan(self.n, self.rowptr, self.colidx, lower=False, unit_diag=False)
            except Exception:
                lower.destroy()
                raise
            self._solvers = (lower, upper)
        return self._solvers

    def apply(self, lu, r, out=None, tmp=None, stream=None):
        """out = U^-1 (L^-1 r), the preconditioner's action; r: n entries, or n x nrhs row-major.  tmp holds L^-1 r (made
        here when None; with tmp and out given, and solvers() called before, nothing is allocated)."""
        lower, upper = self.solvers()
        tmp = lower.solve(lu, r, x=tmp, stream=stream)
        return upper.solve(lu, tmp, x=out, stream=stream)

    def apply_multi(self, lu, R, out=None, stream=None):
        """out = U^-1 (L^-1 R) on an (n, s) row-major block by the tiled solves (SptrsvPlan.solve_multi), the second one
        in place: out[:, j] has exactly the bits apply(lu, R[:, j]) gives, and no temporary is needed (out is R: both
        solves in place).  With out given, and solvers() called before, nothing is allocated."""
        lower, upper = self.solvers()
        out = lower.solve_multi(lu, R, X=out, stream=stream)
        return upper.solve_multi(lu, out, X=out, stream=stream)

    def destroy(self):
        if self._solvers is not None:
            for plan in self._solvers:
                plan.destroy()
            self._solvers = None
        if self.handle:
            lib().sblas_hip_ilu0_plan_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def ilu0(A, stream=None):
    """lu = ILU0(A), one shot: A = (n, rowptr, colidx, val) as GPU tensors.  The plan made here is destroyed before
    returning."""
    n, rowptr, colidx, val = A
    plan = Ilu0Plan(n, rowptr, colidx, stream=stream)
    try:
        lu = plan.factor(val, stream=stream)
        if stream is not None:
            stream.synchronize()
        else:
            import torch
            torch.cuda.current_stream().synchronize()
    finally:
        plan.destroy()
    return lu


# ------------------------------------------------------------------------------------------
# Multicolour reordering: a device graph colouring and P A P^T on a plan (sblas_hip_color_plan_*, sblas_hip_permute_plan_*)
# ------------------------------------------------------------------------------------------
class ColorPlan:
    """A colouring of the n x n CSR pattern (rowptr, colidx), int32 indices (sblas_hip_color_plan_create): no stored
    off-diagonal entry joins two vertices of one colour.  The pattern need not be symmetric; rows may be unsorted, hold
    duplicates and lack a diagonal.  The colours are those of color_ref(): a function of the pattern and seed alone.  A
    bad structure raises an SblasError that names the first bad row (.bad_row).  The plan owns its arrays and keeps
    neither rowptr nor colidx.  Numbering the rows colour by colour (permute()) bounds the levels of both triangles by
    the number of colours."""

    def __init__(self, n, rowptr, colidx, seed=0, stream=None):
        import torch
        self.n, self.seed = n, int(seed) & 0xffffffff
        self.handle = None
        self.nnz = _structure(n, rowptr, colidx)
        self.device = rowptr.device
        h, bad = C.c_void_p(), C.c_int64(-1)
        with torch.cuda.device(self.device):
            rc = lib().sblas_hip_color_plan_create(-1, _stream(stream), n, self.nnz, rowptr.data_ptr(),
                                                   colidx.data_ptr() if self.nnz else None, self.seed, C.byref(h), C.byref(bad))
        if rc != 0:
            raise _bad_structure("sblas_hip_color_plan_create", rc, bad.value)
        self.handle = h

    def info(self):
        out = (C.c_int64 * 8)()
        check(lib().sblas_hip_color_plan_info(self.handle, out), "sblas_hip_color_plan_info")
        return dict(n=int(out[0]), nnz=int(out[1]), colors=int(out[2]), rounds=int(out[3]), largest_class=int(out[4]),
                    smallest_class=int(out[5]), largest_degree=int(out[6]), bytes=int(out[7]))

    def order(self):
        """(color, perm, inv, color_ptr): torch views of the plan's device arrays -- the colour of every vertex, the
        vertices by (colour, vertex), the inverse of that, and class c as perm[color_ptr[c] : color_ptr[c + 1]]; they
        live as long as the plan."""
        import torch
        if self.n == 0:
            empty = lambda: torch.empty(0, dtype=torch.int32, device=self.device)
            return empty(), empty(), empty(), torch.zeros(1, dtype=torch.int32, device=self.device)
        ptrs = [C.c_void_p() for _ in range(4)]
        check(lib().sblas_hip_color_plan_order(self.handle, *[C.byref(p) for p in ptrs]), "sblas_hip_color_plan_order")
        sizes = (self.n, self.n, self.n, self.info()["colors"] + 1)
        return tuple(torch.as_tensor(_DeviceArray(p.value, k, "<i4"), device=self.device) for p, k in zip(ptrs, sizes))

    def permute(self, rowptr, colidx, stream=None):
        """The PermutePlan of (rowptr, colidx) -- this pattern, or another of the same size -- under the plan's perm."""
        return PermutePlan(self.n, rowptr, colidx, self.order()[1], stream=stream)

    def destroy(self):
        if self.handle:
            lib().sblas_hip_color_plan_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class PermutePlan:
    """B = P A P^T of the n x n CSR matrix (rowptr, colidx) for a permutation perm (int32, on the GPU; row r of B is row
    perm[r] of A) (sblas_hip_permute_plan_create).  B's rows come out sorted by column whatever A's order, equal columns
    in A's stored order.  A perm with an entry outside [0, n) or a repeated one raises an SblasError whose .bad_index (and,
    as elsewhere, .bad_row) is the first such index.  The plan owns B's structure and keeps none of the caller's arrays (perm is copied)."""

    def __init__(self, n, rowptr, colidx, perm, stream=None):
        import torch
        self.n = n
        self.handle = None
        self.nnz = _structure(n, rowptr, colidx)
        if not isinstance(perm, torch.Tensor):
            raise SblasError("perm must be a torch tensor")
        _typed("perm", perm, torch.int32)
        if not perm.is_cuda:
            raise SblasError("perm must be a GPU tensor (no CPU path exists)")
        if perm.numel() != n:
            raise SblasError("perm has %d entries for %d rows" % (perm.numel(), n))
        self.device = rowptr.device
        self.perm = perm.clone()                                                # to_permuted() gathers through it
        h, bad = C.c_void_p(), C.c_int64(-1)
        with torch.cuda.device(self.device):
            rc = lib().sblas_hip_permute_plan_create(-1, _stream(stream), n, self.nnz, rowptr.data_ptr(),
                                                     colidx.data_ptr() if self.nnz else None,
                                                     self.perm.data_ptr() if n else None, C.byref(h), C.byref(bad))
        if rc != 0:
            where = ": perm[%d] is out of range or repeated" % bad.value if bad.value >= 0 else ""
            err = SblasError("sblas_hip_permute_plan_create failed: %s (code %d)%s" % (lib().sblas_hip_error_string(rc).decode(), rc, where))
            err.bad_index = err.bad_row = bad.value
            raise err
        self.handle = h

    def info(self):
        out = (C.c_int64 * 4)()
        check(lib().sblas_hip_permute_plan_info(self.handle, out), "sblas_hip_permute_plan_info")
        return dict(n=int(out[0]), nnz=int(out[1]), passes=int(out[2]), bytes=int(out[3]))

    def _view(self, p, k):
        import torch
        if k == 0:
            return torch.empty(0, dtype=torch.int32, device=self.device)
        return torch.as_tensor(_DeviceArray(p.value, k, "<i4"), device=self.device)

    def csr(self):
        """(rowptr_b, colidx_b, src): torch views of the plan's device arrays; B's entry e is A's entry src[e].  They live
        as long as the plan."""
        ptrs = [C.c_void_p() for _ in range(3)]
        check(lib().sblas_hip_permute_plan_csr(self.handle, *[C.byref(p) for p in ptrs]), "sblas_hip_permute_plan_csr")
        return tuple(self._view(p, k) for p, k in zip(ptrs, (self.n + 1, self.nnz, self.nnz)))

    def inverse(self):
        """inv (int32, n): a torch view of the plan's device array, inv[perm[r]] = r"""
        p = C.c_void_p()
        check(lib().sblas_hip_permute_plan_inverse(self.handle, C.byref(p)), "sblas_hip_permute_plan_inverse")
        return self._view(p, self.n)

    def _vector(self, name, t, k):
        import torch
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise SblasError("%s must be a GPU tensor (no CPU path exists)" % name)
        if t.dtype != torch.float64:
            raise SblasError("%s must be float64, got %s" % (name, t.dtype))
        if t.dim() != 1 or not t.is_contiguous() or t.numel() != k:
            raise SblasError("%s must be contiguous with %d entries, got %d" % (name, k, t.numel()))

    def _out(self, x, out, k):
        import torch
        if out is None:
            out = torch.empty(k, dtype=torch.float64, device=self.device)
        self._vector("out", out, k)
        if k and out.data_ptr() == x.data_ptr():
            raise SblasError("out must not be the input: a gather in place is not defined")
        return out

    def values(self, val, out=None, stream=None):
        """B's values for A's values val (in A's stored order): out[e] = val[src[e]].  One launch; with out given nothing
        is allocated, and the call is graph-capturable.  Returns out."""
        self._vector("val", val, self.nnz)
        out = self._out(val, out, self.nnz)
        check(lib().sblas_hip_permute_plan_values(self.handle, _stream(stream), val.data_ptr() if self.nnz else None,
                                                  out.data_ptr() if self.nnz else None), "sblas_hip_permute_plan_values")
        return out

    def to_permuted(self, x, out=None, stream=None):
        """x_B = x_A[perm]: a vector of A's numbering in B's"""
        self._vector("x", x, self.n)
        out = self._out(x, out, self.n)
        if self.n:
            gather(self.perm, x, out, stream=stream)
        return out

    def from_permuted(self, x, out=None, stream=None):
        """x_A = x_B[inv]: a vector of B's numbering in A's"""
        self._vector("x", x, self.n)
        out = self._out(x, out, self.n)
        if self.n:
            gather(self.inverse(), x, out, stream=stream)
        return out

    def destroy(self):
        if self.handle:
            lib().sblas_hip_permute_plan_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def csr_color(A, seed=0, stream=None):
    """(color, perm, color_ptr) of the pattern A = (n, rowptr, colidx) as GPU tensors, one shot: tensors of their own.
    The plan made here is destroyed before returning."""
    n, rowptr, colidx = A[:3]
    plan = ColorPlan(n, rowptr, colidx, seed=seed, stream=stream)
    try:
        color, perm, _, color_ptr = (t.clone() for t in plan.order())
    finally:
        plan.destroy()
    return color, perm, color_ptr


def _krylov_vector(name, t, n, device=None):
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise SblasError("%s must be a GPU tensor (no CPU path exists)" % name)
    if t.dtype != torch.float64:
        raise SblasError("%s must be float64, got %s" % (name, t.dtype))
    if t.dim() != 1 or not t.is_contiguous() or t.numel() != n:
        raise SblasError("%s must be contiguous with %d entries, got shape %s" % (name, n, tuple(t.shape)))
    if device is not None and t.device != device:
        raise SblasError("%s is on %s, the plan on %s" % (name, t.device, device))


# ------------------------------------------------------------------------------------------
# Aggregation AMG: a V-cycle preconditioner on a device plan (sblas_hip_amg_plan_*)
# ------------------------------------------------------------------------------------------
class AmgPlan:
    """Plain aggregation AMG of the square n x n CSR matrix (rowptr, colidx), int32 indices (sblas_hip_amg_plan_create):
    apply() is z = M^-1 r by one V(nu, nu) cycle from a zero guess.  Every row must be strictly ascending in column and
    store its diagonal; a bad structure raises an SblasError that names the first bad row (.bad_row).  theta > 0 keeps
    only the strong entries |a_ij| >= theta * max_k |a_ik| in the aggregation and needs val; the hierarchy is then fixed.
    The plan keeps rowptr and colidx alive and sweeps level 0 on them: do not change them.  setup(val) forms every
    level's values and the smoother on the device and is repeatable; setup and apply allocate nothing inside the library,
    never synchronise and are graph-capturable; check() is the one call that synchronises.  Every bit is pinned
    (include/sblas_hip.h; amg_cycle_ref restates a cycle on the host).  KrylovPlan and GmresPlan take the plan as precond.
    prolongator="smoothed" (sblas_hip_amg_plan_create_ex, include/sblas_hip_amg_sa.h) smooths the prolongator: P = (I -
    prolong_omega D^-1 A) T over the same aggregates, R = P^T, the coarse matrix R (A P) by two SpGEMM plans, the
    transfers of a cycle one row-product kernel; transfer(l) shows P and R and amg_cycle_sa_ref restates the cycle.
    min_reduction in [0, 1) is the coarsening guard (amg_keep_level): a level is kept only when it removes at least that
    share of the rows; None means 0 (any reduction, as before) for a plain plan and 0.2 for a smoothed one.
    aggregation="device" (sblas_hip_amg_plan_create_dev, include/sblas_hip_amg_dev.h) aggregates every level on the device
    in Jones-Plassmann rounds and builds the same plan, array for array; "host" (the default) is create as it was.
    setup(val, smoother="chebyshev", degree=2, ...) (include/sblas_hip_cheby.h) smooths with a Chebyshev polynomial in
    D^-1 A on every level's own device estimate of lambda_max; eig() shows the estimates.
    apply_multi(R) (include/sblas_hip_amg_multi.h) is the cycle on an (n, s) row-major block, s <= 64: column j has exactly
    the bits of apply(R[:, j]).  reserve(s) makes its level vectors (the one call that allocates); a KrylovMultiPlan takes
    the plan as precond.  Not with the Chebyshev smoother."""

    def __init__(self, n, rowptr, colidx, val=None, theta=0.0, coarse_max=64, max_levels=20, seed=0, stream=None, prolongator="plain",
                 prolong_omega=AMG_PROLONG_OMEGA, min_reduction=None, aggregation="host"):
        import torch
        if prolongator not in AMG_PROLONGATORS:
            raise SblasError("prolongator must be 'plain' or 'smoothed', not %r" % (prolongator,))
        if aggregation not in AMG_AGGREGATIONS:
            raise SblasError("aggregation must be 'host' or 'device', not %r" % (aggregation,))
        if min_reduction is None:                                          # plain: today's rule, any reduction keeps a level
            min_reduction = AMG_SMOOTHED_MIN_REDUCTION if prolongator == "smoothed" else 0.0
        if not 0.0 <= float(min_reduction) < 1.0:
            raise SblasError("min_reduction must be in [0, 1), not %r" % (min_reduction,))
        if prolongator == "smoothed" and not 0.0 < float(prolong_omega) < float("inf"):
            raise SblasError("prolong_omega must be positive and finite, not %r" % (prolong_omega,))
        self.n, self.handle, self._val, self._cheb_ready = n, None, None, False
        self.nnz = _structure(n, rowptr, colidx)
        self.rowptr, self.colidx, self.device = rowptr, colidx, rowptr.device
        theta = float(theta)
        if not 0.0 <= theta <= 1.0:
            raise SblasError("theta must be in [0, 1], not %r" % (theta,))
        if theta > 0.0 and val is None:
            raise SblasError("theta > 0 needs val, the values the strength test reads")
        if val is not None:
            _krylov_vector("val", val, self.nnz, self.device)
        if int(coarse_max) < 1 or not 1 <= int(max_levels) <= amg_limits()["level_cap"]:
            raise SblasError("coarse_max must be at least 1 and max_levels in [1, %d]" % amg_limits()["level_cap"])
        h, bad = C.c_void_p(), C.c_int64(-1)
        with torch.cuda.device(self.device):
            args = (-1, _stream(stream), n, self.nnz, rowptr.data_ptr() if n else None, colidx.data_ptr() if self.nnz else None,
                    val.data_ptr() if val is not None and theta > 0.0 and self.nnz else None, theta, int(coarse_max), int(max_levels),
                    int(seed) & 0xffffffff)
            if aggregation != "host":
                name = "sblas_hip_amg_plan_create_dev"
                rc = lib().sblas_hip_amg_plan_create_dev(*args, AMG_PROLONGATORS[prolongator], float(prolong_omega), float(min_reduction),
                                                         AMG_AGGREGATIONS[aggregation], C.byref(h), C.byref(bad))
            elif prolongator == "plain" and float(min_reduction) == 0.0:   # the entry point as it was
                name = "sblas_hip_amg_plan_create"
                rc = lib().sblas_hip_amg_plan_create(*args, C.byref(h), C.byref(bad))
            else:
                name = "sblas_hip_amg_plan_create_ex"
                rc = lib().sblas_hip_amg_plan_create_ex(*args, AMG_PROLONGATORS[prolongator], float(prolong_omega), float(min_reduction),
                                                        C.byref(h), C.byref(bad))
        if rc != 0:
            raise _bad_structure(name, rc, bad.value)
        self.handle = h

    def info(self):
        out = (C.c_int64 * 12)()
        check(lib().sblas_hip_amg_plan_info(self.handle, out), "sblas_hip_amg_plan_info")
        opt = (C.c_double * 4)()
        check(lib().sblas_hip_amg_plan_options(self.handle, opt), "sblas_hip_amg_plan_options")
        return dict(n=int(out[0]), nnz=int(out[1]), levels=int(out[2]), nu=int(out[3]), coarse_sweeps=int(out[4]), launches=int(out[5]),
                    rows=int(out[6]), entries=int(out[7]), bytes=int(out[8]), smoother=("jacobi", "l1", "chebyshev")[out[9]], ready=bool(out[10]),
                    coarsest=int(out[11]), operator_complexity=(out[7] / out[1] if out[1] else 1.0),
                    prolongator=("plain", "smoothed")[int(opt[0])], prolong_omega=float(opt[1]), min_reduction=float(opt[2]),
                    aggregation=("host", "device")[int(opt[3])])

    def transfer(self, l):
        """A smoothed plan's transfer operators between level l and l + 1 as torch views that live as long as the plan
        (sblas_hip_amg_plan_transfer): dict(n, n_coarse, nnz, p_rowptr, p_colidx, p_val, r_rowptr, r_colidx, r_val); P is
        n x n_coarse, R = P^T; the values are there after setup().  Refused on a plain plan and on the coarsest level."""
        import torch
        sizes, ptrs = (C.c_int64 * 3)(), (C.c_void_p * 6)()
        check(lib().sblas_hip_amg_plan_transfer(self.handle, int(l), sizes, ptrs), "sblas_hip_amg_plan_transfer")
        n, nc, nnz = int(sizes[0]), int(sizes[1]), int(sizes[2])
        view = lambda p, k, t: torch.as_tensor(_DeviceArray(p, k, t), device=self.device) if p and k else None
        return dict(n=n, n_coarse=nc, nnz=nnz, p_rowptr=view(ptrs[0], n + 1, "<i4"), p_colidx=view(ptrs[1], nnz, "<i4"),
                    p_val=view(ptrs[2], nnz, "<f8"), r_rowptr=view(ptrs[3], nc + 1, "<i4"), r_colidx=view(ptrs[4], nnz, "<i4"),
                    r_val=view(ptrs[5], nnz, "<f8"))

    def level(self, l):
        """Level l's device arrays as torch views that live as long as the plan: dict(n, nnz, n_coarse, units, rowptr,
        colidx, val, wd, agg, aggptr, members); agg, aggptr and members are None on the coarsest level, val (and wd's
        content) is there after setup()."""
        import torch
        sizes, ptrs = (C.c_int64 * 4)(), (C.c_void_p * 7)()
        check(lib().sblas_hip_amg_plan_level(self.handle, int(l), sizes, ptrs), "sblas_hip_amg_plan_level")
        n, nnz, nc = int(sizes[0]), int(sizes[1]), int(sizes[2])
        view = lambda p, k, t: torch.as_tensor(_DeviceArray(p, k, t), device=self.device) if p and k else None
        return dict(n=n, nnz=nnz, n_coarse=nc, units=int(sizes[3]), rowptr=view(ptrs[0], n + 1, "<i4"), colidx=view(ptrs[1], nnz, "<i4"),
                    val=view(ptrs[2], nnz, "<f8"), wd=view(ptrs[3], n, "<f8"), agg=view(ptrs[4], n if nc else 0, "<i4"),
                    aggptr=view(ptrs[5], nc + 1 if nc else 0, "<i4"), members=view(ptrs[6], n if nc else 0, "<i4"))

    def levels(self):
        """[(n, nnz)] of every level, the finest first"""
        out = []
        for l in range(self.info()["levels"]):
            sizes, ptrs = (C.c_int64 * 4)(), (C.c_void_p * 7)()
            check(lib().sblas_hip_amg_plan_level(self.handle, l, sizes, ptrs), "sblas_hip_amg_plan_level")
            out.append((int(sizes[0]), int(sizes[1])))
        return out

    def setup(self, val, smoother="jacobi", omega=None, nu=1, coarse_sweeps=8, coarse_scale=1.0, stream=None, degree=2, eig_steps=10,
              eig_boost=1.1, eig_ratio=30.0):
        """Every level's values (the Galerkin sums of the aggregates) and the smoother's omega / d from val, on the
        device.  smoother: "jacobi" (omega defaults to 2/3) or "l1" (1).  The plan keeps val alive and sweeps level 0 on
        it: do not change it before the next setup.  Every refusal comes before any launch.
        smoother="chebyshev" (sblas_hip_amg_plan_setup_ex, include/sblas_hip_cheby.h): every smoothing is one Chebyshev
        polynomial of `degree` in D^-1 A on the level's own estimate of lambda_max (eig_steps, eig_boost, eig_ratio as
        ChebyshevPlan's), the coarsest level one polynomial of degree coarse_sweeps (at most 64); omega must be left unset.
        A plan's first such setup allocates the levels' extra vectors and is refused while a stream capture is under way;
        eig() shows every level's estimate."""
        import torch
        if smoother == "chebyshev":
            return self._setup_chebyshev(val, omega, nu, coarse_sweeps, coarse_scale, stream, degree, eig_steps, eig_boost, eig_ratio)
        if smoother not in AMG_SMOOTHERS:
            raise SblasError("smoother must be 'jacobi', 'l1' or 'chebyshev', not %r" % (smoother,))
        _krylov_vector("val", val, self.nnz, self.device)
        if omega is None:
            omega = 0.0
        elif not (float(omega) > 0.0 and float(omega) < float("inf")):
            raise SblasError("omega must be positive and finite, not %r" % (omega,))
        if int(nu) < 1 or int(coarse_sweeps) < 1:
            raise SblasError("nu and coarse_sweeps must be at least 1")
        with torch.cuda.device(self.device):
            rc = lib().sblas_hip_amg_plan_setup(self.handle, _stream(stream), val.data_ptr() if self.nnz else None,
                                                AMG_SMOOTHERS[smoother], float(omega), int(nu), int(coarse_sweeps), float(coarse_scale))
        check(rc, "sblas_hip_amg_plan_setup")
        self._val = val

    def _setup_chebyshev(self, val, omega, nu, coarse_sweeps, coarse_scale, stream, degree, eig_steps, eig_boost, eig_ratio):
        import torch
        _krylov_vector("val", val, self.nnz, self.device)
        if omega is not None:
            raise SblasError("omega must be left unset with the Chebyshev smoother")
        _cheby_options(degree, eig_steps, eig_boost, eig_ratio)
        if int(nu) < 1 or not 1 <= int(coarse_sweeps) <= cheby_limits()["max_degree"]:
            raise SblasError("nu must be at least 1 and coarse_sweeps in [1, %d] with the Chebyshev smoother" % cheby_limits()["max_degree"])
        with torch.cuda.device(self.device):
            if not self._cheb_ready and torch.cuda.is_current_stream_capturing():
                raise SblasError("the plan's first Chebyshev setup allocates its vectors: run it once before capturing a graph")
            rc = lib().sblas_hip_amg_plan_setup_ex(self.handle, _stream(stream), val.data_ptr() if self.nnz else None, AMG_CHEBYSHEV, 0.0,
                                                   int(nu), int(coarse_sweeps), float(coarse_scale), degree, eig_steps, float(eig_boost),
                                                   float(eig_ratio))
        if rc != 0 and not self._cheb_ready:
            raise SblasError("sblas_hip_amg_plan_setup_ex refused (code %d): the plan's first Chebyshev setup allocates its vectors and "
                             "cannot run while a stream capture is under way" % rc)
        check(rc, "sblas_hip_amg_plan_setup_ex")
        self._val, self._cheb_ready = val, True

    def eig(self, stream=None):
        """Every level's estimate after a Chebyshev setup (sblas_hip_amg_plan_eig): a list of dict(m, ritz, g, lambda_max,
        table), table the level's (c1_k, c2_k) rows.  Synchronises."""
        import torch
        levels = []
        for l in range(self.info()["levels"]):
            out, table, count = (C.c_double * 4)(), np.zeros((64, 2)), C.c_int(0)
            with torch.cuda.device(self.device):
                check(lib().sblas_hip_amg_plan_eig(self.handle, _stream(stream), l, out, table.ctypes.data, C.byref(count)), "sblas_hip_amg_plan_eig")
            levels.append(dict(m=int(out[0]), ritz=float(out[1]), g=float(out[2]), lambda_max=float(out[3]), table=table[:count.value].copy()))
        return levels

    def apply(self, r, out=None, stream=None):
        """out = M^-1 r: one V-cycle from a zero guess.  out: made here when None; it must not be r.  Returns out."""
        import torch
        _krylov_vector("r", r, self.n, self.device)
        if out is None:
            out = torch.empty(self.n, dtype=torch.float64, device=self.device)
        _krylov_vector("out", out, self.n, self.device)
        with torch.cuda.device(self.device):
            rc = lib().sblas_hip_amg_plan_apply(self.handle, _stream(stream), r.data_ptr() if self.n else None,
                                                out.data_ptr() if self.n else None)
        check(rc, "sblas_hip_amg_plan_apply")
        return out

    def reserve(self, nrhs, stream=None):
        """The block cycle's level vectors for nrhs columns (sblas_hip_amg_plan_reserve_multi): only grows -- a smaller
        request changes nothing.  Allocates, so it is refused while a stream capture is under way.  Returns the width
        reserved."""
        import torch
        nrhs = _amg_multi_width(nrhs)
        with torch.cuda.device(self.device):
            if nrhs > self.multi_info()["width"] and torch.cuda.is_current_stream_capturing():
                raise SblasError("reserve allocates the block cycle's level vectors: call it before capturing a graph")
            check(lib().sblas_hip_amg_plan_reserve_multi(self.handle, _stream(stream), nrhs), "sblas_hip_amg_plan_reserve_multi")
        return self.multi_info()["width"]

    def multi_info(self):
        """dict(width, bytes, launches) of the block cycle (sblas_hip_amg_plan_multi_info): the reserved columns, the
        bytes of the level vectors, the launches of one block cycle (one cycle's: a walk call is one launch)."""
        out = (C.c_int64 * 4)()
        check(lib().sblas_hip_amg_plan_multi_info(self.handle, out), "sblas_hip_amg_plan_multi_info")
        return dict(width=int(out[0]), bytes=int(out[1]), launches=int(out[2]))

    def apply_multi(self, R, out=None, stream=None):
        """out = M^-1 R on an (n, s) row-major block, one block cycle (sblas_hip_amg_plan_apply_multi): out[:, j] has
        exactly the bits of apply(R[:, j]).  R and out may be column slices of wider tensors; out is made here when None
        and must not overlap R.  Reserves on demand when no capture is under way.  Every refusal comes before any launch."""
        import torch
        if not isinstance(R, torch.Tensor) or R.dim() != 2:
            raise SblasError("R must be an (n, nrhs) GPU tensor")
        s = _amg_multi_width(R.shape[1])
        ldr = _krylov_block("R", R, self.n, s, self.device)
        if out is None:
            out = torch.empty((self.n, s), dtype=torch.float64, device=self.device)
        ldz = _krylov_block("out", out, self.n, s, self.device)
        info = self.info()
        if not info["ready"]:
            raise SblasError("apply_multi needs setup() first")
        if info["smoother"] == "chebyshev":
            raise SblasError("the Chebyshev smoother has no block cycle: apply_multi takes a plan set up with 'jacobi' or 'l1'")
        if self.n and _blocks_overlap(R, ldr, out, ldz, self.n, s):
            raise SblasError("out must not overlap R")
        with torch.cuda.device(self.device):
            if s > self.multi_info()["width"]:
                if torch.cuda.is_current_stream_capturing():
                    raise SblasError("the block cycle's level vectors are reserved for %d columns, not %d: call reserve(%d) before "
                                     "capturing a graph" % (self.multi_info()["width"], s, s))
                self.reserve(s, stream=stream)
            rc = lib().sblas_hip_amg_plan_apply_multi(self.handle, _stream(stream), s, R.data_ptr() if self.n else None, ldr,
                                                      out.data_ptr() if self.n else None, ldz)
        check(rc, "sblas_hip_amg_plan_apply_multi")
        return out

    def check(self, stream=None):
        """None, or (level, row) of the least diagonal the last setup() found not finite and > 0.  Synchronises."""
        import torch
        out = (C.c_int64 * 2)()
        with torch.cuda.device(self.device):
            check(lib().sblas_hip_amg_plan_check(self.handle, _stream(stream), out), "sblas_hip_amg_plan_check")
        return None if out[0] < 0 else (int(out[0]), int(out[1]))

    def destroy(self):
        if self.handle:
            lib().sblas_hip_amg_plan_destroy(self.handle)
            self.handle = None
        self._val = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def _amg_level_vector(name, t, n, plan):
    _krylov_vector(name, t, n, plan.device)
    return t.data_ptr() if n else None


def _amg_level_sizes(plan, level):
    sizes, ptrs = (C.c_int64 * 4)(), (C.c_void_p * 7)()
    check(lib().sblas_hip_amg_plan_level(plan.handle, int(level), sizes, ptrs), "sblas_hip_amg_plan_level")
    return int(sizes[0]), int(sizes[2])


def amg_sweep(plan, level, b, x, y, mode="sweep", stream=None):
    """One launch of the row sweep on level `level` of an AmgPlan after setup() (sblas_hip_amg_sweep_f64): mode "sweep"
    y = x + wd o (b - A x), "residual" y = b - A x, "first" y = wd o b (x may be None).  y must be neither x nor b."""
    import torch
    if mode not in AMG_SWEEP_MODES:
        raise SblasError("mode must be 'sweep', 'residual' or 'first', not %r" % (mode,))
    n, _ = _amg_level_sizes(plan, level)
    pb, py = _amg_level_vector("b", b, n, plan), _amg_level_vector("y", y, n, plan)
    px = _amg_level_vector("x", x, n, plan) if (mode != "first" or x is not None) else None
    with torch.cuda.device(plan.device):
        check(lib().sblas_hip_amg_sweep_f64(plan.handle, _stream(stream), int(level), AMG_SWEEP_MODES[mode], pb, px, py),
              "sblas_hip_amg_sweep_f64")
    return y


def amg_pvalues(plan, level, val, t, stream=None):
    """t for every stored entry of level `level` of a smoothed AmgPlan from the level's values val
    (sblas_hip_amg_pvalues_f64): -(q_i a_ie) off the diagonal, 1 - q_i a_ii on it, q_i = prolong_omega / a_ii."""
    import torch
    sizes, ptrs = (C.c_int64 * 4)(), (C.c_void_p * 7)()
    check(lib().sblas_hip_amg_plan_level(plan.handle, int(level), sizes, ptrs), "sblas_hip_amg_plan_level")
    nnz = int(sizes[1])
    pv, pt = _amg_level_vector("val", val, nnz, plan), _amg_level_vector("t", t, nnz, plan)
    with torch.cuda.device(plan.device):
        check(lib().sblas_hip_amg_pvalues_f64(plan.handle, _stream(stream), int(level), pv, pt), "sblas_hip_amg_pvalues_f64")
    return t


def amg_restrict(plan, level, res, bc, stream=None):
    """bc[I] = the sum of res over aggregate I of level `level`, ascending; on a smoothed plan after setup(), row I of
    R times res in the sweep's order (sblas_hip_amg_restrict_f64)"""
    import torch
    n, nc = _amg_level_sizes(plan, level)
    pr, pc = _amg_level_vector("res", res, n, plan), _amg_level_vector("bc", bc, nc, plan)
    with torch.cuda.device(plan.device):
        check(lib().sblas_hip_amg_restrict_f64(plan.handle, _stream(stream), int(level), pr, pc), "sblas_hip_amg_restrict_f64")
    return bc


def amg_prolong(plan, level, e, x, scale=1.0, stream=None):
    """x_i = x_i + scale * e[agg[i]] on level `level`; on a smoothed plan after setup(), x_i + scale * (row i of P times
    e) (sblas_hip_amg_prolong_f64)"""
    import torch
    n, nc = _amg_level_sizes(plan, level)
    pe, px = _amg_level_vector("e", e, nc, plan), _amg_level_vector("x", x, n, plan)
    with torch.cuda.device(plan.device):
        check(lib().sblas_hip_amg_prolong_f64(plan.handle, _stream(stream), int(level), float(scale), pe, px), "sblas_hip_amg_prolong_f64")
    return x


# ------------------------------------------------------------------------------------------
# The AMG cycle on a block of columns (sblas_amg_multi_*, sblas_hip_amg_*_multi*; include/sblas_hip_amg_multi.h)
# ------------------------------------------------------------------------------------------
def amg_multi_limits():
    """The block cycle's limits (sblas_amg_multi_limits): dict(max_rhs, tile, threads)."""
    out = (C.c_int64 * 4)()
    check(lib().sblas_amg_multi_limits(out), "sblas_amg_multi_limits")
    return dict(max_rhs=int(out[0]), tile=int(out[1]), threads=int(out[2]))


def amg_multi_grid(units, nrhs):
    """Workgroups of one multi-column row kernel over `units` four-lane units (sblas_amg_multi_grid): dict(unit_blocks,
    tiles, grid, last_tile)."""
    out = (C.c_int64 * 4)()
    check(lib().sblas_amg_multi_grid(int(units), int(nrhs), out), "sblas_amg_multi_grid")
    return dict(unit_blocks=int(out[0]), tiles=int(out[1]), grid=int(out[2]), last_tile=int(out[3]))


def _amg_multi_width(s):
    if not 1 <= int(s) <= amg_multi_limits()["max_rhs"]:
        raise SblasError("between 1 and %d columns, not %d" % (amg_multi_limits()["max_rhs"], s))
    return int(s)


def _amg_level_block(name, t, n, s, plan):
    ld = _krylov_block(name, t, n, s, plan.device)
    return (t.data_ptr() if n else None), ld


def _amg_block_width(t):
    import torch
    if not isinstance(t, torch.Tensor) or t.dim() != 2:
        raise SblasError("a block must be a 2-D GPU tensor")
    return _amg_multi_width(t.shape[1])


def amg_sweep_multi(plan, level, B, X, Y, mode="sweep", stream=None):
    """amg_sweep on (n_level, s) row-major blocks, one launch (sblas_hip_amg_sweep_multi_f64): column j of Y has the bits
    amg_sweep gives on column j.  Y must overlap neither B nor X; X may be None with mode "first"."""
    import torch
    if mode not in AMG_SWEEP_MODES:
        raise SblasError("mode must be 'sweep', 'residual' or 'first', not %r" % (mode,))
    s = _amg_block_width(B)
    n, _ = _amg_level_sizes(plan, level)
    pb, ldb = _amg_level_block("B", B, n, s, plan)
    py, ldy = _amg_level_block("Y", Y, n, s, plan)
    px, ldx = _amg_level_block("X", X, n, s, plan) if (mode != "first" or X is not None) else (None, s)
    with torch.cuda.device(plan.device):
        check(lib().sblas_hip_amg_sweep_multi_f64(plan.handle, _stream(stream), int(level), AMG_SWEEP_MODES[mode], s, pb, ldb, px, ldx, py, ldy),
              "sblas_hip_amg_sweep_multi_f64")
    return Y


def amg_restrict_multi(plan, level, RES, BC, stream=None):
    """amg_restrict on row-major blocks: RES (n_level, s) -> BC (n_coarse, s) (sblas_hip_amg_restrict_multi_f64)"""
    import torch
    s = _amg_block_width(RES)
    n, nc = _amg_level_sizes(plan, level)
    pr, ldr = _amg_level_block("RES", RES, n, s, plan)
    pc, ldc = _amg_level_block("BC", BC, nc, s, plan)
    with torch.cuda.device(plan.device):
        check(lib().sblas_hip_amg_restrict_multi_f64(plan.handle, _stream(stream), int(level), s, pr, ldr, pc, ldc),
              "sblas_hip_amg_restrict_multi_f64")
    return BC


def amg_prolong_multi(plan, level, E, X, scale=1.0, stream=None):
    """amg_prolong on row-major blocks: X (n_level, s) += scale * P E, E (n_coarse, s) (sblas_hip_amg_prolong_multi_f64)"""
    import torch
    s = _amg_block_width(X)
    n, nc = _amg_level_sizes(plan, level)
    pe, lde = _amg_level_block("E", E, nc, s, plan)
    px, ldx = _amg_level_block("X", X, n, s, plan)
    with torch.cuda.device(plan.device):
        check(lib().sblas_hip_amg_prolong_multi_f64(plan.handle, _stream(stream), int(level), float(scale), s, pe, lde, px, ldx),
              "sblas_hip_amg_prolong_multi_f64")
    return X


# ------------------------------------------------------------------------------------------
# Chebyshev smoothing on a device eigenvalue estimate (sblas_cheby_*, sblas_hip_cheby_plan_*; include/sblas_hip_cheby.h)
# ------------------------------------------------------------------------------------------
def cheby_limits():
    """The Chebyshev plan's limits (sblas_cheby_limits): dict(threads, max_degree, max_steps, degree, eig_steps, bisections,
    block_slots)."""
    out = (C.c_int64 * 8)()
    check(lib().sblas_cheby_limits(out), "sblas_cheby_limits")
    return dict(zip(("threads", "max_degree", "max_steps", "degree", "eig_steps", "bisections", "block_slots"), (int(v) for v in out)))


def _cheby_csr(n, rowptr, colidx, val):
    rowptr = np.ascontiguousarray(rowptr, np.int32)
    colidx = np.ascontiguousarray(colidx, np.int32)
    val = np.ascontiguousarray(val, np.float64)
    if len(rowptr) != int(n) + 1 or len(colidx) != len(val) or (n and int(rowptr[-1]) != len(colidx)):
        raise SblasError("rowptr needs n + 1 entries that end at len(colidx) == len(val)")
    return rowptr, colidx, val


def _cheby_options(degree=None, eig_steps=None, eig_boost=None, eig_ratio=None):
    """every refusal of the options, before any launch (a NaN fails every comparison)"""
    lim = cheby_limits()
    if degree is not None and (isinstance(degree, bool) or not isinstance(degree, int) or not 1 <= degree <= lim["max_degree"]):
        raise SblasError("degree must be an integer in [1, %d], not %r" % (lim["max_degree"], degree))
    if eig_steps is not None and (isinstance(eig_steps, bool) or not isinstance(eig_steps, int) or not 1 <= eig_steps <= lim["max_steps"]):
        raise SblasError("eig_steps must be an integer in [1, %d], not %r" % (lim["max_steps"], eig_steps))
    if eig_boost is not None and not 1.0 <= float(eig_boost) < float("inf"):
        raise SblasError("eig_boost must be finite and at least 1, not %r" % (eig_boost,))
    if eig_ratio is not None and not 1.0 < float(eig_ratio) < float("inf"):
        raise SblasError("eig_ratio must be finite and greater than 1, not %r" % (eig_ratio,))


def cheby_start_ref(n, seed=0, level=0):
    """The estimate's start vector b0 (sblas_cheby_start_ref): (2 h(i) + 1) 2^-32 - 1 with h the colouring's priority hash
    of salt seed + level -> numpy float64."""
    b0 = np.zeros(int(n))
    check(lib().sblas_cheby_start_ref(int(n), int(seed) & 0xffffffff, int(level) & 0xffffffff, b0.ctypes.data), "sblas_cheby_start_ref")
    return b0


def cheby_lanczos_ref(n, rowptr, colidx, val, eig_steps=10, seed=0, level=0):
    """The estimate's recurrence on the host (sblas_cheby_lanczos_ref) -> dict(alpha, beta, m, bad_row): alpha has m
    entries, beta max(m - 1, 0); bad_row is the least row whose diagonal is not finite and > 0, or None."""
    _cheby_options(eig_steps=eig_steps)
    rowptr, colidx, val = _cheby_csr(n, rowptr, colidx, val)
    alpha, beta, m, bad = np.zeros(eig_steps), np.zeros(eig_steps), C.c_int64(0), C.c_int64(-1)
    rc = lib().sblas_cheby_lanczos_ref(int(n), rowptr.ctypes.data, colidx.ctypes.data, val.ctypes.data, int(seed) & 0xffffffff,
                                       int(level) & 0xffffffff, eig_steps, alpha.ctypes.data, beta.ctypes.data, C.byref(m), C.byref(bad))
    if rc != 0:
        raise _bad_structure("sblas_cheby_lanczos_ref", rc, bad.value)
    k = int(m.value)
    return dict(alpha=alpha[:k], beta=beta[:max(k - 1, 0)], m=k, bad_row=None if bad.value < 0 else int(bad.value))


def cheby_ritz_ref(alpha, beta):
    """The tridiagonal of m = len(alpha) >= 1 finished steps and its largest eigenvalue by Sturm bisection
    (sblas_cheby_ritz_ref) -> dict(t, e2, ritz)."""
    alpha, beta = np.ascontiguousarray(alpha, np.float64).ravel(), np.ascontiguousarray(beta, np.float64).ravel()
    m = len(alpha)
    if not 1 <= m <= cheby_limits()["max_steps"] or len(beta) < m - 1:
        raise SblasError("alpha needs 1 to %d entries and beta at least one fewer" % cheby_limits()["max_steps"])
    t, e2, ritz = np.zeros(m), np.zeros(m), C.c_double(0.0)
    check(lib().sblas_cheby_ritz_ref(m, alpha.ctypes.data, beta.ctypes.data, t.ctypes.data, e2.ctypes.data, C.byref(ritz)), "sblas_cheby_ritz_ref")
    return dict(t=t, e2=e2[:m - 1], ritz=float(ritz.value))


def cheby_rowbound_ref(n, rowptr, colidx, val):
    """g = max_i (sum_e |a_ie| / a_ii) in the pinned order (sblas_cheby_rowbound_ref) -> float"""
    rowptr, colidx, val = _cheby_csr(n, rowptr, colidx, val)
    g, bad = C.c_double(0.0), C.c_int64(-1)
    rc = lib().sblas_cheby_rowbound_ref(int(n), rowptr.ctypes.data, colidx.ctypes.data, val.ctypes.data, C.byref(g), C.byref(bad))
    if rc != 0:
        raise _bad_structure("sblas_cheby_rowbound_ref", rc, bad.value)
    return float(g.value)


def cheby_lambda_ref(m, ritz, g, eig_boost=1.1):
    """lambda_max = min(eig_boost * ritz, g) after m >= 1 steps, g after none (sblas_cheby_lambda_ref)"""
    _cheby_options(eig_boost=eig_boost)
    return float(lib().sblas_cheby_lambda_ref(int(m), float(ritz), float(g), float(eig_boost)))


def cheby_coef_ref(lambda_max, degree=4, eig_ratio=30.0):
    """The coefficient table on [lambda_max / eig_ratio, lambda_max] (sblas_cheby_coef_ref) -> dict(table, lambda_min):
    table is degree x 2, the rows (c1_k, c2_k)."""
    _cheby_options(degree=degree, eig_ratio=eig_ratio)
    if float(lambda_max) != float(lambda_max):
        raise SblasError("lambda_max must not be a NaN")
    table, low = np.zeros((degree, 2)), C.c_double(0.0)
    check(lib().sblas_cheby_coef_ref(float(lambda_max), float(eig_ratio), degree, table.ctypes.data, C.byref(low)), "sblas_cheby_coef_ref")
    return dict(table=table, lambda_min=float(low.value))


def cheby_apply_ref(n, rowptr, colidx, val, table, b, x=None):
    """The polynomial of degree len(table) applied to b on the host (sblas_cheby_apply_ref): from zero, or from the guess
    x -> numpy float64."""
    rowptr, colidx, val = _cheby_csr(n, rowptr, colidx, val)
    table = np.ascontiguousarray(table, np.float64)
    if table.ndim != 2 or table.shape[1] != 2:
        raise SblasError("table must be degree x 2")
    _cheby_options(degree=int(table.shape[0]))
    b = np.ascontiguousarray(b, np.float64).ravel()
    if x is not None:
        x = np.ascontiguousarray(x, np.float64).ravel()
    if len(b) != n or (x is not None and len(x) != n):
        raise SblasError("b and x need n = %d entries" % n)
    y, bad = np.zeros(int(n)), C.c_int64(-1)
    rc = lib().sblas_cheby_apply_ref(int(n), rowptr.ctypes.data, colidx.ctypes.data, val.ctypes.data, table.ctypes.data, int(table.shape[0]),
                                     b.ctypes.data, x.ctypes.data if x is not None else None, y.ctypes.data, C.byref(bad))
    if rc != 0:
        raise _bad_structure("sblas_cheby_apply_ref", rc, bad.value)
    return y


class ChebyshevPlan:
    """z = p(D^-1 A) D^-1 r for the square n x n CSR matrix (rowptr, colidx), int32 indices (sblas_hip_cheby_plan_create):
    p is the Chebyshev polynomial of `degree` on [lambda_max / eig_ratio, lambda_max], and lambda_max(D^-1 A) is estimated
    on the device by eig_steps steps of Jacobi-preconditioned CG from a hashed start vector, boosted by eig_boost and
    capped by the row bound max_i sum_e |a_ie| / a_ii.  Every row must be strictly ascending in column and store its
    diagonal; a bad structure raises an SblasError that names the first bad row (.bad_row).  The plan keeps rowptr and
    colidx alive and sweeps on them: do not change them.  setup(val) is device work only, repeatable and graph-capturable;
    apply() and smooth() are `degree` launches of one row kernel, allocate nothing inside the library and never
    synchronise; check() is the one call that synchronises.  Every bit is pinned (include/sblas_hip_cheby.h; the
    cheby_*_ref functions restate it on the host).  KrylovPlan and GmresPlan take the plan as precond."""

    def __init__(self, n, rowptr, colidx, degree=4, eig_steps=10, eig_boost=1.1, eig_ratio=30.0, seed=0, stream=None):
        import torch
        self.n, self.handle, self._val = n, None, None
        _cheby_options(degree, eig_steps, eig_boost, eig_ratio)
        self.nnz = _structure(n, rowptr, colidx)
        self.rowptr, self.colidx, self.device = rowptr, colidx, rowptr.device
        self.degree = degree
        h, bad = C.c_void_p(), C.c_int64(-1)
        with torch.cuda.device(self.device):
            rc = lib().sblas_hip_cheby_plan_create(-1, _stream(stream), n, self.nnz, rowptr.data_ptr() if n else None,
                                                   colidx.data_ptr() if self.nnz else None, degree, eig_steps, float(eig_boost),
                                                   float(eig_ratio), int(seed) & 0xffffffff, C.byref(h), C.byref(bad))
        if rc != 0:
            raise _bad_structure("sblas_hip_cheby_plan_create", rc, bad.value)
        self.handle = h

    def info(self):
        out = (C.c_int64 * 12)()
        check(lib().sblas_hip_cheby_plan_info(self.handle, out), "sblas_hip_cheby_plan_info")
        return dict(n=int(out[0]), nnz=int(out[1]), degree=int(out[2]), eig_steps=int(out[3]), units=int(out[4]), launches=int(out[5]),
                    bytes=int(out[6]), ready=bool(out[7]), setup_launches=int(out[8]), seed=int(out[9]))

    def setup(self, val, lambda_max=None, stream=None):
        """dinv, the row bound and the coefficient table from val, on the device; lambda_max None runs the estimate, a
        finite positive lambda_max takes its place (through the same scalar kernel).  The plan keeps val alive and sweeps
        on it: do not change it before the next setup.  Every refusal comes before any launch."""
        import torch
        _krylov_vector("val", val, self.nnz, self.device)
        if lambda_max is None:
            lambda_max = float("nan")
        elif not 0.0 < float(lambda_max) < float("inf"):
            raise SblasError("lambda_max must be positive and finite (or None for the estimate), not %r" % (lambda_max,))
        with torch.cuda.device(self.device):
            rc = lib().sblas_hip_cheby_plan_setup(self.handle, _stream(stream), val.data_ptr() if self.nnz else None, float(lambda_max))
        check(rc, "sblas_hip_cheby_plan_setup")
        self._val = val

    def apply(self, r, out=None, stream=None):
        """out = p(D^-1 A) D^-1 r from a zero guess.  out: made here when None; it must not be r.  Returns out."""
        import torch
        _krylov_vector("r", r, self.n, self.device)
        if out is None:
            out = torch.empty(self.n, dtype=torch.float64, device=self.device)
        _krylov_vector("out", out, self.n, self.device)
        with torch.cuda.device(self.device):
            rc = lib().sblas_hip_cheby_plan_apply(self.handle, _stream(stream), r.data_ptr() if self.n else None,
                                                  out.data_ptr() if self.n else None)
        check(rc, "sblas_hip_cheby_plan_apply")
        return out

    def smooth(self, b, x, out=None, stream=None):
        """out = x + p(D^-1 A) D^-1 (b - A x): the polynomial from the guess x.  out must be neither b nor x."""
        import torch
        _krylov_vector("b", b, self.n, self.device), _krylov_vector("x", x, self.n, self.device)
        if out is None:
            out = torch.empty(self.n, dtype=torch.float64, device=self.device)
        _krylov_vector("out", out, self.n, self.device)
        with torch.cuda.device(self.device):
            rc = lib().sblas_hip_cheby_plan_smooth(self.handle, _stream(stream), b.data_ptr() if self.n else None,
                                                   x.data_ptr() if self.n else None, out.data_ptr() if self.n else None)
        check(rc, "sblas_hip_cheby_plan_smooth")
        return out

    def check(self, stream=None):
        """What the last setup() found -> dict(bad_row, m, ritz, g, lambda_max, lambda_min): bad_row is the least row whose
        diagonal is not finite and > 0, or None; m the finished steps of the estimate.  Synchronises."""
        import torch
        out = (C.c_double * 6)()
        with torch.cuda.device(self.device):
            check(lib().sblas_hip_cheby_plan_check(self.handle, _stream(stream), out), "sblas_hip_cheby_plan_check")
        return dict(bad_row=None if out[0] < 0 else int(out[0]), m=int(out[1]), ritz=float(out[2]), g=float(out[3]), lambda_max=float(out[4]),
                    lambda_min=float(out[5]))

    def scalars(self, stream=None):
        """The estimate's alpha (m entries) and beta (m - 1) and the coefficient table (degree x 2) of the last setup(), as
        numpy arrays (sblas_hip_cheby_plan_scalars).  Synchronises."""
        import torch
        m = self.check(stream)["m"]
        alpha, beta, table = np.zeros(cheby_limits()["max_steps"]), np.zeros(cheby_limits()["max_steps"]), np.zeros((self.degree, 2))
        with torch.cuda.device(self.device):
            check(lib().sblas_hip_cheby_plan_scalars(self.handle, _stream(stream), alpha.ctypes.data, beta.ctypes.data, table.ctypes.data),
                  "sblas_hip_cheby_plan_scalars")
        return dict(alpha=alpha[:m], beta=beta[:max(m - 1, 0)], table=table)

    def destroy(self):
        if self.handle:
            lib().sblas_hip_cheby_plan_destroy(self.handle)
            self.handle = None
        self._val = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


# ------------------------------------------------------------------------------------------
# FSAI: a factorised sparse approximate inverse on a device plan (sblas_fsai_*, sblas_hip_fsai_plan_*; include/sblas_hip_fsai.h)
# ------------------------------------------------------------------------------------------
def fsai_limits():
    """The FSAI plan's limits (sblas_fsai_limits): dict(threads, row_max, g4_max, g16_max, tri_per_lane, vec_per_lane,
    lds_bytes) -- the setup kernel's workgroup, the longest row of G, the longest rows that 4 and 16 lanes take, and the
    LDS a lane and a workgroup own."""
    out = (C.c_int64 * 8)()
    check(lib().sblas_fsai_limits(out), "sblas_fsai_limits")
    return dict(zip(("threads", "row_max", "g4_max", "g16_max", "tri_per_lane", "vec_per_lane", "lds_bytes"), (int(v) for v in out)))


def _fsai_max_row(max_row):
    """max_row as the library takes it: None is 0 (a row above row_max entries is refused)"""
    if max_row is None:
        return 0
    if isinstance(max_row, bool) or not isinstance(max_row, int) or not 1 <= max_row <= fsai_limits()["row_max"]:
        raise SblasError("max_row must be None or an integer in [1, %d], not %r" % (fsai_limits()["row_max"], max_row))
    return max_row


def _fsai_structure(n, rowptr, colidx, what):
    rowptr = np.ascontiguousarray(rowptr, np.int32)
    colidx = np.ascontiguousarray(colidx, np.int32)
    if len(rowptr) != int(n) + 1 or (n and int(rowptr[-1]) != len(colidx)):
        raise SblasError("%s: rowptr needs n + 1 entries that end at len(colidx)" % what)
    return rowptr, colidx


def fsai_pattern(n, rowptr, colidx, pattern=None, max_row=None):
    """G's pattern on the host (sblas_fsai_pattern, numpy arrays) -> (rowptr_g, colidx_g): row i holds the stored entries
    of A's row i with column <= i, or those of pattern = (rowptr_p, colidx_p); max_row = k keeps of every longer row its
    diagonal and the k - 1 entries of largest column below it.  A refused structure raises an SblasError whose .bad_row
    is the first bad row: a row of A out of order or without its diagonal, a pattern row that does not ascend or lacks
    its diagonal, a row of G above row_max entries without max_row."""
    k = _fsai_max_row(max_row)
    rowptr, colidx = _fsai_structure(n, rowptr, colidx, "A")
    if pattern is not None:
        rp, cp = _fsai_structure(n, pattern[0], pattern[1], "pattern")
    out_rp = np.zeros(int(n) + 1, np.int32)
    out_ci = np.zeros(max(len(cp) if pattern is not None else len(colidx), 1), np.int32)
    bad = C.c_int64(-1)
    rc = lib().sblas_fsai_pattern(int(n), rowptr.ctypes.data, colidx.ctypes.data, len(cp) if pattern is not None else 0,
                                  rp.ctypes.data if pattern is not None else None, cp.ctypes.data if pattern is not None else None, k,
                                  out_rp.ctypes.data, out_ci.ctypes.data, C.byref(bad))
    if rc != 0:
        raise _bad_structure("sblas_fsai_pattern", rc, bad.value)
    return out_rp, out_ci[:int(out_rp[-1])].copy()


def fsai_ref(n, rowptr, colidx, val, rowptr_g, colidx_g):
    """G's values by the scalar loop that is the contract (sblas_fsai_ref, numpy arrays), on a pattern fsai_pattern gave
    -> (val_g, bad_row): bad_row is the least row whose dense system failed (written as its diagonal alone), or None."""
    rowptr, colidx, val = _cheby_csr(n, rowptr, colidx, val)
    rowptr_g, colidx_g = _fsai_structure(n, rowptr_g, colidx_g, "G")
    val_g = np.zeros(max(len(colidx_g), 1))
    bad = C.c_int64(-1)
    rc = lib().sblas_fsai_ref(int(n), rowptr.ctypes.data, colidx.ctypes.data, val.ctypes.data, rowptr_g.ctypes.data, colidx_g.ctypes.data,
                              val_g.ctypes.data, C.byref(bad))
    if rc != 0:
        raise _bad_structure("sblas_fsai_ref", rc, bad.value)
    return val_g[:len(colidx_g)].copy(), None if bad.value < 0 else int(bad.value)


class FsaiPlan:
    """The factorised sparse approximate inverse of Kolotilina and Yeremin for the symmetric positive definite n x n CSR
    matrix (rowptr, colidx), int32 indices (sblas_hip_fsai_plan_create): a sparse lower-triangular G with G A G^T ~ I,
    applied as z = G^T (G r) by two planned SpMVs.  Every row must be strictly ascending in column and store its diagonal;
    only entries with column <= row are ever read.  pattern None: row i of G holds the stored entries of A's row i with
    column <= i; pattern = (rowptr_g, colidx_g), GPU int32 tensors: the caller's (ascending rows; entries above the
    diagonal are ignored; positions A does not store count as zero).  A row of G above 64 entries is refused unless
    max_row = k (1 <= k <= 64): every longer row then keeps its diagonal and the k - 1 entries of largest column below
    it -- a structural and crude thinning that knows no value (on A^2 of a grid it drops the far neighbours first and
    costs more iterations than A's own pattern).  A bad structure raises an SblasError that names the first bad row
    (.bad_row).  The plan keeps rowptr and colidx alive and gathers from them: do not change them.  setup(val) is one
    launch of the gather-and-Cholesky kernel and the transpose's value update: device work only, repeatable and
    graph-capturable; apply() allocates nothing inside the library and never synchronises; check() is the one call that
    synchronises.  Every bit is pinned (include/sblas_hip_fsai.h; fsai_pattern and fsai_ref restate it on the host).
    KrylovPlan and GmresPlan take the plan as precond.

    The lower triangle of A^2 as the pattern, through SpgemmPlan and a lower-triangle filter:

        sq = SpgemmPlan(n, n, n, rowptr, colidx, rowptr, colidx)
        rp2, ci2 = sq.csr()                                  # rows ascend when A's do
        rows = torch.repeat_interleave(torch.arange(n, device=ci2.device), (rp2[1:] - rp2[:-1]).long())
        keep = ci2.long() <= rows
        counts = torch.zeros(n, dtype=torch.long, device=ci2.device).index_add_(0, rows[keep], torch.ones_like(rows[keep]))
        rpl = torch.cat([counts.new_zeros(1), counts.cumsum(0)]).int()
        plan = FsaiPlan(n, rowptr, colidx, pattern=(rpl, ci2[keep].contiguous()))
    """

    def __init__(self, n, rowptr, colidx, pattern=None, max_row=None, stream=None):
        import torch
        self.n, self.handle, self._val = n, None, None
        k = _fsai_max_row(max_row)
        self.nnz = _structure(n, rowptr, colidx)
        self.rowptr, self.colidx, self.device = rowptr, colidx, rowptr.device
        self.pattern = None
        nnz_p, rp_p, ci_p = 0, None, None
        if pattern is not None:
            if not isinstance(pattern, (tuple, list)) or len(pattern) != 2:
                raise SblasError("pattern must be None or a pair (rowptr_g, colidx_g)")
            nnz_p = _structure(n, pattern[0], pattern[1])
            if pattern[0].device != self.device or pattern[1].device != self.device:
                raise SblasError("pattern is on %s, the matrix on %s" % (pattern[0].device, self.device))
            self.pattern = (pattern[0], pattern[1])
            rp_p = pattern[0].data_ptr()
            ci_p = pattern[1].data_ptr() if nnz_p else None
        if colidx.device != self.device:
            raise SblasError("colidx is on %s, rowptr on %s" % (colidx.device, self.device))
        h, bad = C.c_void_p(), C.c_int64(-1)
        with torch.cuda.device(self.device):
            rc = lib().sblas_hip_fsai_plan_create(-1, _stream(stream), n, self.nnz, rowptr.data_ptr() if n else None,
                                                  colidx.data_ptr() if self.nnz else None, nnz_p, rp_p, ci_p, k, C.byref(h), C.byref(bad))
        if rc != 0:
            raise _bad_structure("sblas_hip_fsai_plan_create", rc, bad.value)
        self.handle = h
        self.nnz_g = self.info()["nnz_g"]

    def info(self):
        out = (C.c_int64 * 12)()
        check(lib().sblas_hip_fsai_plan_info(self.handle, out), "sblas_hip_fsai_plan_info")
        return dict(n=int(out[0]), nnz=int(out[1]), nnz_g=int(out[2]), longest=int(out[3]), units=int(out[4]), launches=int(out[5]),
                    bytes=int(out[6]), ready=bool(out[7]), rows_g4=int(out[8]), rows_g16=int(out[9]), rows_g64=int(out[10]))

    def csr(self):
        """(rowptr_g, colidx_g, val_g): torch views of the plan's device arrays; they live as long as the plan, and val_g
        holds what the last setup() wrote."""
        import torch
        ptrs = [C.c_void_p() for _ in range(3)]
        check(lib().sblas_hip_fsai_plan_csr(self.handle, *[C.byref(p) for p in ptrs]), "sblas_hip_fsai_plan_csr")
        def one(p, n, typestr, dtype):
            if n == 0 or not p.value:
                return torch.zeros(n, dtype=dtype, device=self.device)
            return torch.as_tensor(_DeviceArray(p.value, n, typestr), device=self.device)
        return (one(ptrs[0], self.n + 1, "<i4", torch.int32), one(ptrs[1], self.nnz_g, "<i4", torch.int32),
                one(ptrs[2], self.nnz_g, "<f8", torch.float64))

    def setup(self, val, stream=None):
        """G's values from val, on the device.  Every refusal comes before any launch."""
        import torch
        _krylov_vector("val", val, self.nnz, self.device)
        with torch.cuda.device(self.device):
            rc = lib().sblas_hip_fsai_plan_setup(self.handle, _stream(stream), val.data_ptr() if self.nnz else None)
        check(rc, "sblas_hip_fsai_plan_setup")
        self._val = val

    def apply(self, r, out=None, stream=None):
        """out = G^T (G r).  out: made here when None; it must not overlap r.  Returns out."""
        import torch
        _krylov_vector("r", r, self.n, self.device)
        if out is None:
            out = torch.empty(self.n, dtype=torch.float64, device=self.device)
        _krylov_vector("out", out, self.n, self.device)
        with torch.cuda.device(self.device):
            rc = lib().sblas_hip_fsai_plan_apply(self.handle, _stream(stream), r.data_ptr() if self.n else None,
                                                 out.data_ptr() if self.n else None)
        check(rc, "sblas_hip_fsai_plan_apply")
        return out

    def check(self, stream=None):
        """The least row whose dense system the last setup() failed (it was written as its diagonal alone), or None.
        Synchronises."""
        import torch
        bad = C.c_int64(-1)
        with torch.cuda.device(self.device):
            check(lib().sblas_hip_fsai_plan_check(self.handle, _stream(stream), C.byref(bad)), "sblas_hip_fsai_plan_check")
        return None if bad.value < 0 else int(bad.value)

    def destroy(self):
        if self.handle:
            lib().sblas_hip_fsai_plan_destroy(self.handle)
            self.handle = None
        self._val = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


# ------------------------------------------------------------------------------------------
# Krylov solvers on a plan, resident on the device: PCG and BiCGStab (sblas_hip_krylov_*)
# ------------------------------------------------------------------------------------------
def krylov_dots(pairs, out=None, workspace=None, stream=None):
    """The pinned dot products (x, y) of up to three pairs in ONE pass over memory (sblas_hip_krylov_dot_f64): a device
    tensor of len(pairs) doubles, each with exactly the bits krylov_dot gives alone.  No synchronisation; with out and
    workspace (a float64 tensor of at least len(pairs) * ceil(n / cell) entries) given, nothing is allocated."""
    import torch
    k = len(pairs)
    if not 1 <= k <= 3:
        raise SblasError("one to three pairs, not %d" % k)
    n = pairs[0][0].numel() if isinstance(pairs[0][0], torch.Tensor) else -1
    for q, (x, y) in enumerate(pairs):
        _krylov_vector("x[%d]" % q, x, n), _krylov_vector("y[%d]" % q, y, n, x.device)
    device = pairs[0][0].device
    if out is None:
        out = torch.empty(k, dtype=torch.float64, device=device)
    _krylov_vector("out", out, k, device)
    need = int(lib().sblas_hip_krylov_dot_workspace(n, k))
    if workspace is None:
        workspace = torch.empty(need // 8, dtype=torch.float64, device=device)
    if not isinstance(workspace, torch.Tensor) or not workspace.is_cuda or workspace.dtype != torch.float64 or not workspace.is_contiguous():
        raise SblasError("workspace must be a contiguous float64 GPU tensor")
    xs = (C.c_void_p * k)(*[x.data_ptr() if n else None for x, _ in pairs])
    ys = (C.c_void_p * k)(*[y.data_ptr() if n else None for _, y in pairs])
    with torch.cuda.device(device):
        check(lib().sblas_hip_krylov_dot_f64(-1, _stream(stream), n, k, xs, ys, out.data_ptr(), workspace.data_ptr(),
                                             workspace.numel() * 8), "sblas_hip_krylov_dot_f64")
    return out


def krylov_dot(x, y, out=None, workspace=None, stream=None):
    """The pinned dot product (x, y): a one-element device tensor, no synchronisation.  Its bits are krylov_dot_ref's: a
    function of n and the two vectors alone."""
    return krylov_dots([(x, y)], out=out, workspace=workspace, stream=stream)


def krylov_update(op, scalars, vectors, partial=None, jacobi=False, stream=None):
    """One fused update of the solvers on its own (sblas_hip_krylov_update_f64).  op: a key of KRYLOV_UPDATES; scalars: a
    device block of 16 eight-byte slots ([0] status as int64 -- anything but 0 and the call writes nothing -- [4] alpha,
    [5] beta, [6] omega); vectors: the op's vectors in the header's order, n entries each; partial: float64, at least
    2 * ceil(n / cell) entries, for the ops that are also a dot's first stage."""
    import torch
    if op not in KRYLOV_UPDATES:
        raise SblasError("op must be one of %s, not %r" % (sorted(KRYLOV_UPDATES), op))
    n = vectors[0].numel() if len(vectors) and isinstance(vectors[0], torch.Tensor) else -1
    for q, t in enumerate(vectors):
        _krylov_vector("vectors[%d]" % q, t, n)
    _krylov_vector("scalars", scalars, 16)
    if partial is not None:
        _krylov_vector("partial", partial, partial.numel() if isinstance(partial, torch.Tensor) else -1)
        if partial.numel() < 2 * -(-n // krylov_limits()["cell"]):
            raise SblasError("partial is too short")
    v = (C.c_void_p * len(vectors))(*[t.data_ptr() if n else None for t in vectors])
    with torch.cuda.device(scalars.device):
        check(lib().sblas_hip_krylov_update_f64(-1, _stream(stream), KRYLOV_UPDATES[op], 1 if jacobi else 0, n, scalars.data_ptr(), v,
                                                len(vectors), partial.data_ptr() if partial is not None and partial.numel() else None),
              "sblas_hip_krylov_update_f64")


def _precond_seat(precond):
    """precond as a solver plan takes it -> (kind, lower, upper): the code PRECOND_* and the plans whose handles go with it.
    An AmgPlan's, a ChebyshevPlan's or an FsaiPlan's handle travels in the lower plan's place, with no upper one."""
    if precond is None:
        return PRECOND_NONE, None, None
    if isinstance(precond, str) and precond == "jacobi":
        return PRECOND_JACOBI, None, None
    if isinstance(precond, Ilu0Plan):
        return (PRECOND_ILU0,) + tuple(precond.solvers())
    if isinstance(precond, (tuple, list)) and len(precond) == 2 and all(isinstance(q, SptrsvPlan) for q in precond):
        return PRECOND_ILU0, precond[0], precond[1]
    if isinstance(precond, AmgPlan):
        return PRECOND_AMG, precond, None
    if isinstance(precond, ChebyshevPlan):
        return PRECOND_CHEBYSHEV, precond, None
    if isinstance(precond, FsaiPlan):
        return PRECOND_FSAI, precond, None
    raise SblasError("precond must be None, 'jacobi', an Ilu0Plan, a pair of SptrsvPlans, an AmgPlan, a ChebyshevPlan or an FsaiPlan, not %r"
                     % (precond,))


class _SolverPlan:
    """What KrylovPlan and GmresPlan share: the seat of the preconditioner, start / iterate / solve and the handle's end.
    A subclass names its C functions in _c (sblas_hip_<_c>_start, ...), checks its own arguments, creates the handle and
    gives info() and status()."""

    def _seat(self, spmv_plan, precond):
        """refuses precond, then spmv_plan -> what plan_create takes after the structure: (spmv, kind, lower, upper)"""
        self.spmv_plan, self.precond = spmv_plan, precond
        self.precond_kind, lower, upper = _precond_seat(precond)
        if spmv_plan is not None and not isinstance(spmv_plan, SpmvPlan):
            raise SblasError("spmv_plan must be an SpmvPlan or None")
        self._solvers = (lower, upper)
        self._keep = None
        return (spmv_plan.handle if spmv_plan is not None else None, self.precond_kind,
                lower.handle if lower is not None else None, upper.handle if upper is not None else None)

    def _bind(self, n, rowptr, colidx):
        self.n, self.nnz = n, _structure(n, rowptr, colidx)
        self.rowptr, self.colidx, self.device = rowptr, colidx, rowptr.device

    def _call(self, name):
        return getattr(lib(), "sblas_hip_%s_%s" % (self._c, name))

    def _values(self, lu, dinv):
        """start's lu / dinv, by the seated kind -> the tensor that travels as lu_or_dinv, or None"""
        if self.precond_kind == PRECOND_ILU0:
            if lu is None:
                raise SblasError("an ILU(0) preconditioner needs lu, its factor")
            _krylov_vector("lu", lu, self.nnz, self.device)
            return lu
        if self.precond_kind == PRECOND_JACOBI:
            if dinv is None:
                raise SblasError("the Jacobi preconditioner needs dinv, the inverse diagonal")
            _krylov_vector("dinv", dinv, self.n, self.device)
            return dinv
        return None

    def start(self, val, b, x, lu=None, dinv=None, rtol=1e-8, atol=0.0, max_iter=1000, stream=None):
        """Begins a solve: x on entry is the initial guess and is updated in place by iterate().  lu: the ILU(0) factor
        (precond an Ilu0Plan); dinv: the inverse diagonal (precond "jacobi").  Every refusal comes before any launch."""
        import torch
        _krylov_vector("val", val, self.nnz, self.device), _krylov_vector("b", b, self.n, self.device)
        _krylov_vector("x", x, self.n, self.device)
        pre = self._values(lu, dinv)
        if self.n and x.data_ptr() == b.data_ptr():
            raise SblasError("x must not be b")
        if not (rtol >= 0.0 and atol >= 0.0) or int(max_iter) < 0:
            raise SblasError("rtol and atol must be >= 0 and max_iter >= 0")
        with torch.cuda.device(self.device):
            rc = self._call("start")(self.handle, _stream(stream), val.data_ptr() if self.nnz else None,
                                     pre.data_ptr() if pre is not None and pre.numel() else None,
                                     b.data_ptr() if self.n else None, x.data_ptr() if self.n else None,
                                     float(rtol), float(atol), int(max_iter))
        check(rc, "sblas_hip_%s_start" % self._c)
        self._keep = (val, b, x, pre)

    def iterate(self, k, stream=None):
        """Enqueues k iterations (GMRES: Arnoldi steps, and the closes and restarts that belong with them): allocates
        nothing, never synchronises, graph-capturable as a chain."""
        import torch
        with torch.cuda.device(self.device):
            check(self._call("iterate")(self.handle, _stream(stream), int(k)), "sblas_hip_%s_iterate" % self._c)

    def solve(self, val, b, x=None, lu=None, dinv=None, rtol=1e-8, atol=0.0, max_iter=1000, check_every=8, stream=None):
        """start(), then iterate(check_every) / status() until the status is not "running" -> (x, status dict).  x: the
        initial guess, updated in place (zeros made here when None).  The result does not depend on check_every."""
        import torch
        if int(check_every) < 1:
            raise SblasError("check_every must be at least 1")
        if x is None:
            _krylov_vector("b", b, self.n, self.device)
            x = torch.zeros(self.n, dtype=torch.float64, device=self.device)
        self.start(val, b, x, lu=lu, dinv=dinv, rtol=rtol, atol=atol, max_iter=max_iter, stream=stream)
        while True:
            self.iterate(int(check_every), stream=stream)
            st = self.status(stream=stream)
            if st["code"] != KRYLOV_RUNNING:
                return x, st

    def destroy(self):
        if self.handle:
            self._call("plan_destroy")(self.handle)
            self.handle = None
        self._keep = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class KrylovPlan(_SolverPlan):
    """A Krylov solver for A x = b on the n x n CSR structure (rowptr, colidx), int32 indices, resident on the device
    (sblas_hip_krylov_plan_create).  method: "pcg" (A symmetric positive definite) or "bicgstab".  spmv_plan: an SpmvPlan on
    the same tensors, or None.  precond: None, "jacobi" (start / solve take dinv, the inverse diagonal) or an Ilu0Plan on
    the same tensors (they take lu, its factor; a pair (lower, upper) of SptrsvPlans serves too).  The plan owns the work
    vectors, the partial sums and the scalar block, and keeps the tensors and plans it was given alive.

    start() forms r = b - A x and the first direction; iterate(k) enqueues k iterations without allocating or
    synchronising (graph-capturable); status() is the one call that synchronises.  Once the stopping test
    |r| <= max(rtol |b|, atol) is met on the device, the iterations already enqueued change nothing: x, the count and
    |r| are those of the iteration that met it, whatever check_every is.  Every bit is pinned (include/sblas_hip.h).

    A system in the multicolour order is the caller's composition:
        color = ColorPlan(n, rowptr, colidx); perm = color.permute(rowptr, colidx); rp, ci, _ = perm.csr()
        ilu = Ilu0Plan(n, rp, ci); val_b = perm.values(val); lu = ilu.factor(val_b)
        x_b, st = KrylovPlan(n, rp, ci, precond=ilu).solve(val_b, perm.to_permuted(b), lu=lu)
        x = perm.from_permuted(x_b)"""

    _c = "krylov"

    def __init__(self, n, rowptr, colidx, method="pcg", spmv_plan=None, precond=None, stream=None):
        import torch
        self.handle = None
        if method not in _KRYLOV_METHOD:
            raise SblasError("method must be 'pcg' or 'bicgstab', not %r" % (method,))
        self.method = method
        self._bind(n, rowptr, colidx)
        seat = self._seat(spmv_plan, precond)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            rc = lib().sblas_hip_krylov_plan_create(-1, _stream(stream), _KRYLOV_METHOD[method], n, self.nnz, rowptr.data_ptr(),
                                                    colidx.data_ptr() if self.nnz else None, *seat, C.byref(h))
        check(rc, "sblas_hip_krylov_plan_create")
        self.handle = h

    def info(self):
        out = (C.c_int64 * 10)()
        check(lib().sblas_hip_krylov_plan_info(self.handle, out), "sblas_hip_krylov_plan_info")
        return dict(n=int(out[0]), nnz=int(out[1]), method=[k for k, v in _KRYLOV_METHOD.items() if v == out[2]][0],
                    precond=_PRECOND_NAME[out[3]], vectors=int(out[4]), vector_bytes=int(out[5]), partial_bytes=int(out[6]),
                    scalar_bytes=int(out[7]), bytes=int(out[8]), launches=int(out[9]))

    def status(self, stream=None):
        """Copies the scalar block back and synchronises the stream -> dict(status, code, iterations, rnorm, bnorm, alpha,
        beta, omega, breakdown): status is "running", "converged", "breakdown" or "limit"; breakdown names the zero or
        non-finite denominator (a value of KRYLOV_DENOM) or is None."""
        import torch
        out = (C.c_double * 8)()
        with torch.cuda.device(self.device):
            check(lib().sblas_hip_krylov_status(self.handle, _stream(stream), out), "sblas_hip_krylov_status")
        return dict(status=KRYLOV_STATUS[int(out[0])], code=int(out[0]), iterations=int(out[1]), rnorm=float(out[2]), bnorm=float(out[3]),
                    alpha=float(out[4]), beta=float(out[5]), omega=float(out[6]), breakdown=KRYLOV_DENOM[int(out[7])])


def _krylov_one_shot(method, A, b, precond, x, kw, make=None):
    import torch
    n, rowptr, colidx, val = A
    if precond not in (None, "jacobi", "ilu0", "amg", "amg_smoothed", "chebyshev", "fsai"):
        raise SblasError("precond must be None, 'jacobi', 'ilu0', 'amg', 'amg_smoothed', 'chebyshev' or 'fsai', not %r" % (precond,))
    ilu = plan = amg = None
    lu = dinv = None
    try:
        if precond in ("amg", "amg_smoothed"):                            # the defaults: V(1, 1), Jacobi 2/3, structure only
            amg = AmgPlan(n, rowptr, colidx, prolongator="smoothed" if precond == "amg_smoothed" else "plain")
            amg.setup(val)
        elif precond == "chebyshev":                                        # the defaults: degree 4 on the device's estimate
            amg = ChebyshevPlan(n, rowptr, colidx)
            amg.setup(val)
        elif precond == "fsai":                                             # the default: G on A's lower pattern
            amg = FsaiPlan(n, rowptr, colidx)
            amg.setup(val)
        elif precond is not None:                                           # both read the diagonal's places off the ILU(0) plan
            ilu = Ilu0Plan(n, rowptr, colidx)
            if precond == "ilu0":
                lu = ilu.factor(val)
            else:
                dinv = ilu.pivots(val).reciprocal_()
        pre = ilu if precond == "ilu0" else amg if amg is not None else precond
        plan = make(n, rowptr, colidx, pre) if make is not None else KrylovPlan(n, rowptr, colidx, method=method, precond=pre)
        return plan.solve(val, b, x=x, lu=lu, dinv=dinv, **kw)
    finally:
        if plan is not None:
            plan.destroy()
        if ilu is not None:
            ilu.destroy()
        if amg is not None:
            amg.destroy()


def pcg(A, b, precond=None, x=None, rtol=1e-8, atol=0.0, max_iter=1000, check_every=8):
    """x with A x = b by preconditioned CG, one shot: A = (n, rowptr, colidx, val) as GPU tensors, symmetric positive
    definite; precond None, "jacobi" or "ilu0" (rows sorted with a stored diagonal for the last two).  -> (x, status
    dict).  The plans made here are destroyed before returning."""
    return _krylov_one_shot("pcg", A, b, precond, x, dict(rtol=rtol, atol=atol, max_iter=max_iter, check_every=check_every))


def bicgstab(A, b, precond=None, x=None, rtol=1e-8, atol=0.0, max_iter=1000, check_every=8):
    """x with A x = b by preconditioned BiCGStab, one shot, as pcg(); A need not be symmetric."""
    return _krylov_one_shot("bicgstab", A, b, precond, x, dict(rtol=rtol, atol=atol, max_iter=max_iter, check_every=check_every))


# ------------------------------------------------------------------------------------------
# PCG and BiCGStab for several right-hand sides on one SpMM per product (sblas_hip_krylov_multi_*)
# ------------------------------------------------------------------------------------------
def krylov_multi_limits():
    """The multi-right-hand-side solvers' limits (sblas_krylov_multi_limits): dict(max_rhs, tile, cell, width, pcg_blocks,
    bicgstab_blocks, max_dots, block_slots)."""
    out = (C.c_int64 * 8)()
    check(lib().sblas_krylov_multi_limits(out), "sblas_krylov_multi_limits")
    return dict(max_rhs=int(out[0]), tile=int(out[1]), cell=int(out[2]), width=int(out[3]), pcg_blocks=int(out[4]),
                bicgstab_blocks=int(out[5]), max_dots=int(out[6]), block_slots=int(out[7]))


def _solver_pair(precond):
    return isinstance(precond, (tuple, list)) and len(precond) == 2 and all(isinstance(q, SptrsvPlan) for q in precond)


def _multi_precond(precond):
    """precond of a multi-right-hand-side plan -> its code; the kinds without a multi-column apply are refused by name.
    An AmgPlan INSTANCE is taken (its block cycle); the name "amg" carries no plan and stays refused.  ILU(0) comes in as
    the PAIR of SptrsvPlans ilu.solvers() (the tiled solves); an Ilu0Plan instance and the name "ilu0" stay refused."""
    if isinstance(precond, AmgPlan) and lib().sblas_krylov_multi_precond_plan_ok(PRECOND_AMG) == 0:
        return PRECOND_AMG
    if _solver_pair(precond) and lib().sblas_krylov_multi_precond_pair_ok(PRECOND_ILU0) == 0:
        return PRECOND_ILU0
    kind = _precond_seat(precond)[0] if not isinstance(precond, str) or precond == "jacobi" else _PRECOND_CODE.get(precond, -1)
    if kind < 0:
        raise SblasError("precond must be None or 'jacobi', not %r" % (precond,))
    if lib().sblas_krylov_multi_precond_ok(kind) != 0:
        raise SblasError("the %s preconditioner has no multi-column apply: several right-hand sides take None or 'jacobi'%s"
                         % (_PRECOND_NAME[kind], ", or ILU(0) as the pair precond=ilu.solvers()" if kind == PRECOND_ILU0 else ""))
    return kind


def krylov_multi_launches(method="pcg", precond=None, spmm_launches=0):
    """Launches of one lockstep iteration (sblas_krylov_multi_launches): the solver's own kernels and spmm_launches for
    each product (PCG one, BiCGStab two).  precond an AmgPlan: its block cycles, the dots and the fold that go with them
    are counted too (sblas_krylov_multi_launches_ex with the plan's cycle); a pair of SptrsvPlans (ilu.solvers()): the two
    solves' launches in the cycle's place (sblas_krylov_multi_launches_pair)."""
    if method not in _KRYLOV_METHOD:
        raise SblasError("method must be 'pcg' or 'bicgstab', not %r" % (method,))
    kind = _multi_precond(precond)
    if isinstance(precond, AmgPlan):
        n = int(lib().sblas_krylov_multi_launches_ex(_KRYLOV_METHOD[method], kind, int(spmm_launches), precond.multi_info()["launches"]))
    elif _solver_pair(precond):
        n = int(lib().sblas_krylov_multi_launches_pair(_KRYLOV_METHOD[method], kind, int(spmm_launches), precond[0].info()["launches"],
                                                       precond[1].info()["launches"]))
    else:
        n = int(lib().sblas_krylov_multi_launches(_KRYLOV_METHOD[method], kind, int(spmm_launches)))
    if n < 0:
        raise SblasError("sblas_krylov_multi_launches refused its arguments")
    return n


def krylov_multi_grid(n, nrhs):
    """Workgroups of one multi-column pass (sblas_krylov_multi_grid): dict(cells, tiles, grid, last_tile)."""
    out = (C.c_int64 * 4)()
    check(lib().sblas_krylov_multi_grid(int(n), int(nrhs), out), "sblas_krylov_multi_grid")
    return dict(cells=int(out[0]), tiles=int(out[1]), grid=int(out[2]), last_tile=int(out[3]))


KRYLOV_STEPS = {"start_b": 1, "start_r": 2, "rho0": 3, "pcg_alpha": 4, "pcg_res": 5, "pcg_beta": 6, "bicg_alpha": 7, "bicg_omega": 8,
                "bicg_res": 9}                                              # SBLAS_KRYLOV_STEP_*


def krylov_scalar_step_ref(op, d, block, flag=0, rtol=0.0, atol=0.0, max_iter=0):
    """The solvers' scalar step on a host block (sblas_krylov_scalar_step_ref): the text the device folds run.  block: 16
    float64 slots (the status, the count, max_iter, which and zero_x slots hold int64 bits), updated in place."""
    if op not in KRYLOV_STEPS:
        raise SblasError("op must be one of %s, not %r" % (sorted(KRYLOV_STEPS), op))
    d = np.ascontiguousarray(d, np.float64)
    if not isinstance(block, np.ndarray) or block.dtype != np.float64 or block.shape != (16,) or not block.flags.c_contiguous:
        raise SblasError("block must be a contiguous float64 array of 16 slots")
    check(lib().sblas_krylov_scalar_step_ref(KRYLOV_STEPS[op], len(d), int(flag), d.ctypes.data, block.ctypes.data, float(rtol), float(atol),
                                             int(max_iter)), "sblas_krylov_scalar_step_ref")
    return block


def _krylov_block(name, t, n, s, device=None):
    """an n x s row-major block: a 2-D float64 GPU tensor with unit stride along a row and a row stride >= s -> its ld"""
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise SblasError("%s must be a GPU tensor (no CPU path exists)" % name)
    if t.dtype != torch.float64:
        raise SblasError("%s must be float64, got %s" % (name, t.dtype))
    if t.dim() != 2 or tuple(t.shape) != (n, s):
        raise SblasError("%s must be a (%d, %d) tensor, got shape %s" % (name, n, s, tuple(t.shape)))
    if device is not None and t.device != device:
        raise SblasError("%s is on %s, the plan on %s" % (name, t.device, device))
    if n == 0:                                                             # without rows there are no strides to read (an empty
        return max(int(s), 1)                                              # tensor that came from numpy has strides (0, 0))
    ld = t.stride(0) if n > 1 else max(t.stride(0), s)
    if (s > 1 and t.stride(1) != 1) or ld < s:
        raise SblasError("%s must be row-major with a leading dimension of at least %d, got strides %s" % (name, s, tuple(t.stride())))
    return int(ld)


def _multi_width(s):
    if not 1 <= int(s) <= krylov_multi_limits()["max_rhs"]:
        raise SblasError("between 1 and %d right-hand sides, not %d" % (krylov_multi_limits()["max_rhs"], s))
    return int(s)


def _blocks_overlap(a, lda, b, ldb, n, s):
    span = lambda ld: ((n - 1) * ld + s) * 8 if n else 0
    return a.data_ptr() < b.data_ptr() + span(ldb) and b.data_ptr() < a.data_ptr() + span(lda)


def krylov_multi_dots(pairs, out=None, workspace=None, stream=None):
    """The pinned dot of every column of up to three pairs of (n, s) row-major blocks in ONE pass over memory
    (sblas_hip_krylov_multi_dot_f64): a (len(pairs), s) device tensor, entry [k, j] with exactly the bits krylov_dot
    gives on column j of pair k.  A block may be a column slice of a wider tensor.  No synchronisation; with out and
    workspace (float64, at least len(pairs) * s * ceil(n / cell) entries) given, nothing is allocated."""
    import torch
    k = len(pairs)
    if not 1 <= k <= 3:
        raise SblasError("one to three pairs, not %d" % k)
    first = pairs[0][0]
    if not isinstance(first, torch.Tensor) or first.dim() != 2:
        raise SblasError("x[0] must be a 2-D GPU tensor")
    n, s = int(first.shape[0]), _multi_width(first.shape[1])
    device = first.device
    lds = [(_krylov_block("x[%d]" % q, x, n, s, device), _krylov_block("y[%d]" % q, y, n, s, device)) for q, (x, y) in enumerate(pairs)]
    if out is None:
        out = torch.empty((k, s), dtype=torch.float64, device=device)
    if not isinstance(out, torch.Tensor) or not out.is_cuda or out.dtype != torch.float64 or not out.is_contiguous() or out.numel() != k * s:
        raise SblasError("out must be a contiguous float64 GPU tensor of %d entries" % (k * s))
    need = int(lib().sblas_hip_krylov_multi_dot_workspace(n, s, k))
    if workspace is None:
        workspace = torch.empty(need // 8, dtype=torch.float64, device=device)
    if not isinstance(workspace, torch.Tensor) or not workspace.is_cuda or workspace.dtype != torch.float64 or not workspace.is_contiguous():
        raise SblasError("workspace must be a contiguous float64 GPU tensor")
    xs = (C.c_void_p * k)(*[x.data_ptr() if n else None for x, _ in pairs])
    ys = (C.c_void_p * k)(*[y.data_ptr() if n else None for _, y in pairs])
    ldx, ldy = (C.c_int64 * k)(*[a for a, _ in lds]), (C.c_int64 * k)(*[b for _, b in lds])
    with torch.cuda.device(device):
        check(lib().sblas_hip_krylov_multi_dot_f64(-1, _stream(stream), n, s, k, xs, ldx, ys, ldy, out.data_ptr(), workspace.data_ptr(),
                                                   workspace.numel() * 8), "sblas_hip_krylov_multi_dot_f64")
    return out


_KRYLOV_MULTI_DINV = {"pcg_xr": 4, "bicg_p": 3, "bicg_s": 3}                # the place of dinv among an update's operands


def krylov_multi_update(op, scalars, blocks, partial=None, jacobi=False, stream=None):
    """One fused multi-column update on its own (sblas_hip_krylov_multi_update_f64).  op: a key of KRYLOV_UPDATES;
    scalars: an (s, 16) device tensor of eight-byte slots, row j column j's block ([0] status as int64 -- anything but 0
    and column j is neither read nor written -- [4] alpha, [5] beta, [6] omega); blocks: the op's operands in the
    header's order, (n, s) row-major blocks, with jacobi the dinv vector of n entries at its place; partial: float64, at
    least 2 * s * ceil(n / cell) entries, for the ops that are also a dot's first stage."""
    import torch
    if op not in KRYLOV_UPDATES:
        raise SblasError("op must be one of %s, not %r" % (sorted(KRYLOV_UPDATES), op))
    first = blocks[0] if len(blocks) else None
    if not isinstance(first, torch.Tensor) or first.dim() != 2:
        raise SblasError("blocks[0] must be a 2-D GPU tensor")
    n, s = int(first.shape[0]), _multi_width(first.shape[1])
    device = first.device
    dp = _KRYLOV_MULTI_DINV.get(op, -1) if jacobi else -1
    lds = []
    for q, t in enumerate(blocks):
        if q == dp:
            _krylov_vector("dinv", t, n, device)
            lds.append(0)
        else:
            lds.append(_krylov_block("blocks[%d]" % q, t, n, s, device))
    if not isinstance(scalars, torch.Tensor) or not scalars.is_cuda or scalars.dtype != torch.float64 or not scalars.is_contiguous() \
            or scalars.numel() != 16 * s or scalars.device != device:
        raise SblasError("scalars must be a contiguous float64 GPU tensor of %d x 16 slots" % s)
    if partial is not None:
        _krylov_vector("partial", partial, partial.numel() if isinstance(partial, torch.Tensor) else -1, device)
        if partial.numel() < 2 * s * -(-n // krylov_limits()["cell"]):
            raise SblasError("partial is too short")
    v = (C.c_void_p * len(blocks))(*[t.data_ptr() if n else None for t in blocks])
    ld = (C.c_int64 * len(blocks))(*lds)
    with torch.cuda.device(device):
        check(lib().sblas_hip_krylov_multi_update_f64(-1, _stream(stream), KRYLOV_UPDATES[op], 1 if jacobi else 0, n, s, scalars.data_ptr(), v,
                                                      ld, len(blocks), partial.data_ptr() if partial is not None and partial.numel() else None),
              "sblas_hip_krylov_multi_update_f64")


class _MultiSolverPlan(_SolverPlan):
    """What KrylovMultiPlan and GmresMultiPlan share beside _SolverPlan's iterate and handle's end: the seat of a
    multi-column preconditioner, start / solve on (n, nrhs) blocks and the common columns of status().  A subclass names
    its C functions in _c, checks its own arguments, creates the handle, gives info() and names the three status
    columns of its own in _columns, as (name, is an integer), and the names of its breakdowns in _denom."""

    def _seat_multi(self, n, rowptr, colidx, precond, stream):
        """refuses precond, then the structure, then a plan made for another one -> (lower, upper), the handles that
        travel with the kind; an AmgPlan's level vectors are reserved for nrhs columns.  self.precond keeps the plans alive."""
        import torch
        self.precond, self.precond_kind = precond, _multi_precond(precond)
        self._bind(n, rowptr, colidx)
        self._keep = None
        same = lambda q: q.n == n and q.rowptr.data_ptr() == rowptr.data_ptr() and q.colidx.data_ptr() == colidx.data_ptr()
        if isinstance(precond, AmgPlan):
            if not same(precond):
                raise SblasError("the AmgPlan was made for another structure than this solver's (rowptr, colidx)")
            with torch.cuda.device(self.device):
                precond.reserve(self.nrhs, stream=stream)
            return precond.handle, None
        if self.precond_kind == PRECOND_ILU0:
            if not all(same(q) for q in precond):
                raise SblasError("the SptrsvPlans were made for another structure than this solver's (rowptr, colidx)")
            if not (precond[0].lower and precond[0].unit_diag and not precond[1].lower and not precond[1].unit_diag):
                raise SblasError("the pair must be (lower with a unit diagonal, upper with a stored one), as Ilu0Plan.solvers() gives it")
            return precond[0].handle, precond[1].handle
        return None, None

    def start(self, val, B, X, lu=None, dinv=None, rtol=1e-8, atol=0.0, max_iter=1000, stream=None):
        """Begins a solve: X on entry holds the initial guesses and is updated in place by iterate().  lu: the ILU(0)
        factor (precond a pair of SptrsvPlans); dinv: the inverse diagonal (precond "jacobi").  Every refusal comes
        before any launch."""
        import torch
        _krylov_vector("val", val, self.nnz, self.device)
        ldb = _krylov_block("B", B, self.n, self.nrhs, self.device)
        ldx = _krylov_block("X", X, self.n, self.nrhs, self.device)
        pre = self._values(lu, dinv)
        if self.precond_kind == PRECOND_AMG:
            info = self.precond.info()
            if not info["ready"]:
                raise SblasError("the AmgPlan needs setup() before a solve")
            if info["smoother"] == "chebyshev":
                raise SblasError("the Chebyshev smoother has no block cycle: set the AmgPlan up with 'jacobi' or 'l1'")
        if self.n and _blocks_overlap(X, ldx, B, ldb, self.n, self.nrhs):
            raise SblasError("X must not overlap B")
        if not (rtol >= 0.0 and atol >= 0.0) or int(max_iter) < 0:
            raise SblasError("rtol and atol must be >= 0 and max_iter >= 0")
        with torch.cuda.device(self.device):
            rc = self._call("start")(self.handle, _stream(stream), val.data_ptr() if self.nnz else None,
                                     pre.data_ptr() if pre is not None and pre.numel() else None,
                                     B.data_ptr() if self.n else None, ldb, X.data_ptr() if self.n else None, ldx,
                                     float(rtol), float(atol), int(max_iter))
        check(rc, "sblas_hip_%s_start" % self._c)
        self._keep = (val, B, X, pre)

    def status(self, stream=None):
        """Copies the scalar blocks back and synchronises the stream -> dict of per-column numpy arrays (code, iterations,
        rnorm, bnorm, the plan's own three, which), lists status and breakdown (the names, as the single solver's status
        gives them) and running, the count of columns still running."""
        import torch
        out = (C.c_double * (8 * self.nrhs))()
        with torch.cuda.device(self.device):
            check(self._call("status")(self.handle, _stream(stream), out), "sblas_hip_%s_status" % self._c)
        a = np.array(out, np.float64).reshape(self.nrhs, 8)
        code, which = a[:, 0].astype(np.int64), a[:, 7].astype(np.int64)
        st = dict(code=code, iterations=a[:, 1].astype(np.int64), rnorm=a[:, 2].copy(), bnorm=a[:, 3].copy())
        for k, (name, integer) in enumerate(self._columns, 4):
            st[name] = a[:, k].astype(np.int64) if integer else a[:, k].copy()
        st.update(which=which, status=[KRYLOV_STATUS[int(c)] for c in code], breakdown=[self._denom[int(w)] for w in which],
                  running=int((code == KRYLOV_RUNNING).sum()))
        return st

    def solve(self, val, B, X=None, lu=None, dinv=None, rtol=1e-8, atol=0.0, max_iter=1000, check_every=8, stream=None):
        """start(), then iterate(check_every) / status() until no column is running -> (X, status dict).  X: the initial
        guesses, updated in place (zeros made here when None).  No column's result depends on check_every."""
        import torch
        if int(check_every) < 1:
            raise SblasError("check_every must be at least 1")
        if X is None:
            _krylov_block("B", B, self.n, self.nrhs, self.device)
            X = torch.zeros((self.n, self.nrhs), dtype=torch.float64, device=self.device)
        self.start(val, B, X, lu=lu, dinv=dinv, rtol=rtol, atol=atol, max_iter=max_iter, stream=stream)
        while True:
            self.iterate(int(check_every), stream=stream)
            st = self.status(stream=stream)
            if st["running"] == 0:
                return X, st


class KrylovMultiPlan(_MultiSolverPlan):
    """PCG or BiCGStab for A X = B with nrhs right-hand sides at once on the n x n CSR structure (rowptr, colidx), int32
    indices (sblas_hip_krylov_multi_plan_create): nrhs independent recurrences that share A and run in lockstep, one SpMM
    per product instead of nrhs SpMVs.  method: "pcg" (A symmetric positive definite) or "bicgstab"; precond: None or
    "jacobi" (start / solve take dinv, one inverse diagonal for all columns), or an AmgPlan on the same tensors after its
    setup() with "jacobi" or "l1" (sblas_hip_krylov_multi_plan_create_ex): its block cycle runs on all columns where the
    single solver applies the cycle, column j with exactly AmgPlan.apply's bits; the solver reserves the plan's level
    vectors for nrhs columns, keeps the plan alive and takes no dinv.  Two solvers seated on one AmgPlan share its level
    vectors, as two single solvers do: do not run them at the same time.  ILU(0) is seated as the PAIR of SptrsvPlans
    (lower, upper) that ilu.solvers() returns, the form KrylovPlan already accepts (sblas_hip_krylov_multi_plan_create_pair):
    M^-1 is the two tiled solves (SptrsvPlan.solve_multi, the second in place), column j with exactly Ilu0Plan.apply's
    bits; start / solve then take lu, the factor, and the solver keeps the two plans alive.  This door is the pair because
    the older refusals are pinned: an Ilu0Plan INSTANCE, a ChebyshevPlan, and the NAMES "ilu0", "amg" and "chebyshev",
    which carry no plan, stay refused as having no multi-column apply.  B and X are (n, nrhs) float64 GPU tensors, row-major: contiguous, or a column
    slice of a wider tensor.  The plan owns an SpMM plan for this width, its workspace, the work blocks, the partial sums
    and one scalar block a column, and keeps the structure tensors alive.

    start() forms every r_j = b_j - A x_j and first direction; iterate(k) enqueues k lockstep iterations without
    allocating or synchronising (graph-capturable); status() is the one call that synchronises.  Every column has its own
    scalars and stopping test: once column j's test is met (or it breaks down) nothing reads or writes column j again,
    while the others go on, so every column's x, count and |r| are those of its own stopping iteration, whatever
    check_every is.  A solve equals the lockstep loop composed of the SpMM, the pinned dot per column and numpy updates
    bit for bit; it is NOT promised to equal a KrylovPlan solve of one column, or a batch of another width.

    start / solve take (val, B, X, lu=None, dinv=None, rtol, atol, max_iter[, check_every], stream), the order of every
    other solver plan; they once had dinv ahead of rtol and lu last.  Pass what follows X by keyword: a dinv passed by
    position now arrives as lu, and the Jacobi plan refuses the call for its missing dinv."""

    _c = "krylov_multi"
    _columns = (("alpha", False), ("beta", False), ("omega", False))
    _denom = KRYLOV_DENOM

    def __init__(self, n, rowptr, colidx, nrhs, method="pcg", precond=None, stream=None):
        import torch
        self.handle = None
        if method not in _KRYLOV_METHOD:
            raise SblasError("method must be 'pcg' or 'bicgstab', not %r" % (method,))
        self.method, self.nrhs = method, _multi_width(nrhs)
        lower, upper = self._seat_multi(n, rowptr, colidx, precond, stream)
        # one create a door: the plan of an applied kind (AMG), the pair of solve plans (ILU(0)), or neither
        if upper is not None:
            door, plans = "_pair", (lower, upper)
        elif lower is not None:
            door, plans = "_ex", (self.precond_kind, lower)
        else:
            door, plans = "", (self.precond_kind,)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            rc = self._call("plan_create" + door)(-1, _stream(stream), _KRYLOV_METHOD[method], n, self.nnz, rowptr.data_ptr(),
                                                  colidx.data_ptr() if self.nnz else None, self.nrhs, *plans, C.byref(h))
        check(rc, "sblas_hip_krylov_multi_plan_create" + door)
        self.handle = h

    def info(self):
        out = (C.c_int64 * 12)()
        check(lib().sblas_hip_krylov_multi_plan_info(self.handle, out), "sblas_hip_krylov_multi_plan_info")
        return dict(n=int(out[0]), nnz=int(out[1]), method=[k for k, v in _KRYLOV_METHOD.items() if v == out[2]][0],
                    precond=_PRECOND_NAME[out[3]], nrhs=int(out[4]), blocks=int(out[5]), block_bytes=int(out[6]), partial_bytes=int(out[7]),
                    scalar_bytes=int(out[8]), workspace_bytes=int(out[9]), bytes=int(out[10]), launches=int(out[11]))


def _krylov_multi_one_shot(method, A, B, precond, X, kw, make=None):
    import torch
    n, rowptr, colidx, val = A
    one_shot_amg = isinstance(precond, str) and precond in ("amg", "amg_smoothed")
    if _solver_pair(precond):                                               # a pair needs its factor at start: the plan's door
        raise SblasError("the one-shots take no pair of solve plans: use %s(..., precond=ilu.solvers()).solve(..., lu=lu)"
                         % ("KrylovMultiPlan" if make is None else "GmresMultiPlan"))
    kind =PRECOND_AMG if one_shot_amg else _multi_precond(precond)
    if not isinstance(B, torch.Tensor) or B.dim() != 2:
        raise SblasError("B must be an (n, nrhs) GPU tensor")
    ilu = plan = dinv = amg = None
    try:
        if one_shot_amg:                                                    # the defaults, as pcg(): V(1, 1), Jacobi 2/3, structure only
            amg = precond = AmgPlan(n, rowptr, colidx, prolongator="smoothed" if precond == "amg_smoothed" else "plain")
            amg.setup(val)
        if kind == PRECOND_JACOBI:                                          # the diagonal's places, read off the ILU(0) plan
            ilu = Ilu0Plan(n, rowptr, colidx)
            dinv = ilu.pivots(val).reciprocal_()
        if make is not None:                                                # another plan with the same doors (gmres_multi)
            plan = make(n, rowptr, colidx, B.shape[1], precond)
        else:
            plan = KrylovMultiPlan(n, rowptr, colidx, B.shape[1], method=method, precond=precond)
        return plan.solve(val, B, X=X, dinv=dinv, **kw)
    finally:
        if plan is not None:
            plan.destroy()
        if ilu is not None:
            ilu.destroy()
        if amg is not None:
            amg.destroy()


def pcg_multi(A, B, precond=None, X=None, rtol=1e-8, atol=0.0, max_iter=1000, check_every=8):
    """X with A X = B by preconditioned CG on all columns of B at once, one shot: A = (n, rowptr, colidx, val) as GPU
    tensors, symmetric positive definite; B an (n, nrhs) row-major tensor; precond None, "jacobi", "amg" or
    "amg_smoothed" (rows sorted with a stored diagonal; the last two build an AmgPlan with pcg()'s defaults and set it up).  -> (X, status dict of per-column arrays).  The plans made here are destroyed before returning."""
    return _krylov_multi_one_shot("pcg", A, B, precond, X, dict(rtol=rtol, atol=atol, max_iter=max_iter, check_every=check_every))


def bicgstab_multi(A, B, precond=None, X=None, rtol=1e-8, atol=0.0, max_iter=1000, check_every=8):
    """X with A X = B by preconditioned BiCGStab on all columns of B at once, one shot, as pcg_multi(); A need not be
    symmetric."""
    return _krylov_multi_one_shot("bicgstab", A, B, precond, X, dict(rtol=rtol, atol=atol, max_iter=max_iter, check_every=check_every))


# ------------------------------------------------------------------------------------------
# Restarted GMRES(m) on a plan of its own (sblas_hip_gmres_*)
# ------------------------------------------------------------------------------------------
def _gmres_columns(V, k_max):
    """V: k columns of n entries as a (k, n) float64 GPU tensor with unit stride along a column and one stride between
    columns (a view with a larger stride serves) -> (k, n, ldv)"""
    import torch
    if not isinstance(V, torch.Tensor) or not V.is_cuda:
        raise SblasError("V must be a GPU tensor (no CPU path exists)")
    if V.dtype != torch.float64 or V.dim() != 2:
        raise SblasError("V must be a float64 tensor of shape (columns, n)")
    k, n = V.shape
    if not 1 <= k <= k_max:
        raise SblasError("one to %d columns, not %d" % (k_max, k))
    if n > 1 and V.stride(1) != 1:
        raise SblasError("a column of V must be contiguous")
    ldv = V.stride(0) if k > 1 else max(n, 1)
    if k > 1 and ldv < n:
        raise SblasError("the column stride %d is below n = %d" % (ldv, n))
    return k, n, ldv


def gmres_dots(V, w, out=None, workspace=None, stream=None):
    """out[i] = (V[i], w) for up to 65 columns in ONE pass over memory (sblas_hip_gmres_dots_f64), each with exactly the bits
    krylov_dot(V[i], w) gives.  V: (k, n), see _gmres_columns.  No synchronisation; with out and workspace (float64, at
    least k * ceil(n / cell) entries) given, nothing is allocated."""
    import torch
    k, n, ldv = _gmres_columns(V, gmres_limits()["max_dots"])
    _krylov_vector("w", w, n, V.device)
    if out is None:
        out = torch.empty(k, dtype=torch.float64, device=V.device)
    _krylov_vector("out", out, k, V.device)
    need = int(lib().sblas_hip_gmres_dots_workspace(n, k))
    if workspace is None:
        workspace = torch.empty(need // 8, dtype=torch.float64, device=V.device)
    if not isinstance(workspace, torch.Tensor) or not workspace.is_cuda or workspace.dtype != torch.float64 or not workspace.is_contiguous():
        raise SblasError("workspace must be a contiguous float64 GPU tensor")
    with torch.cuda.device(V.device):
        check(lib().sblas_hip_gmres_dots_f64(-1, _stream(stream), n, k, V.data_ptr() if n else None, ldv, w.data_ptr() if n else None,
                                             out.data_ptr(), workspace.data_ptr(), workspace.numel() * 8), "sblas_hip_gmres_dots_f64")
    return out


def gmres_project(V, h, w, partial=None, stream=None):
    """w = w - h[0] V[0] - h[1] V[1] - ... in place, ascending, each product and each difference rounded
    (sblas_hip_gmres_project_f64); h: k doubles on the device.  partial: None, or a float64 tensor of at least
    ceil(n / cell) entries that receives the first stage of (w, w) over the new w."""
    import torch
    k, n, ldv = _gmres_columns(V, gmres_limits()["max_dots"])
    _krylov_vector("w", w, n, V.device), _krylov_vector("h", h, k, V.device)
    if partial is not None:
        _krylov_vector("partial", partial, partial.numel() if isinstance(partial, torch.Tensor) else -1, V.device)
        if partial.numel() < -(-n // krylov_limits()["cell"]):
            raise SblasError("partial is too short")
    with torch.cuda.device(V.device):
        check(lib().sblas_hip_gmres_project_f64(-1, _stream(stream), n, k, V.data_ptr() if n else None, ldv, h.data_ptr(),
                                                w.data_ptr() if n else None,
                                                partial.data_ptr() if partial is not None and partial.numel() else None),
              "sblas_hip_gmres_project_f64")
    return w


def gmres_combine(V, y, out=None, stream=None):
    """u = y[0] V[0], then u = u + y[l] V[l] ascending, rounded product and rounded sum (sblas_hip_gmres_combine_f64) ->
    u (out when given; it must not be part of V)."""
    import torch
    k, n, ldv = _gmres_columns(V, gmres_limits()["max_dots"])
    _krylov_vector("y", y, k, V.device)
    if out is None:
        out = torch.empty(n, dtype=torch.float64, device=V.device)
    _krylov_vector("out", out, n, V.device)
    with torch.cuda.device(V.device):
        check(lib().sblas_hip_gmres_combine_f64(-1, _stream(stream), n, k, V.data_ptr() if n else None, ldv, y.data_ptr(),
                                                out.data_ptr() if n else None), "sblas_hip_gmres_combine_f64")
    return out


class GmresPlan(_SolverPlan):
    """Right-preconditioned restarted GMRES(restart) for A x = b on the n x n CSR structure (rowptr, colidx), int32
    indices, resident on the device (sblas_hip_gmres_plan_create).  A need not be symmetric.  spmv_plan and precond: as
    KrylovPlan's.  A plan of its own rather than a method of KrylovPlan: it owns restart + 1 basis vectors and the small
    triangular system beside the work vectors, and one iteration is one Arnoldi step (one SpMV, one M^-1).

    start() forms r = b - A x and v_0; iterate(k) enqueues k steps -- with a close (x = x + M^-1 V y) and a restart
    behind every restart-th step, and a close at its end -- without allocating or synchronising (graph-capturable);
    status() is the one call that synchronises.  Once the test |g_{j+1}| <= max(rtol |b|, atol) is met on the device,
    what is already enqueued only forms x from the finished columns: x, the count, |r| and the restart count do not
    depend on check_every.  Every bit is pinned (include/sblas_hip.h)."""

    _c = "gmres"

    def __init__(self, n, rowptr, colidx, restart=30, spmv_plan=None, precond=None, stream=None):
        import torch
        self.handle = None
        if isinstance(restart, bool) or not isinstance(restart, int) or not 1 <= restart <= gmres_limits()["max_restart"]:
            raise SblasError("restart must be an integer in [1, %d], not %r" % (gmres_limits()["max_restart"], restart))
        self.restart = restart
        seat = self._seat(spmv_plan, precond)
        self._bind(n, rowptr, colidx)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            rc = lib().sblas_hip_gmres_plan_create(-1, _stream(stream), n, self.nnz, rowptr.data_ptr(),
                                                   colidx.data_ptr() if self.nnz else None, restart, *seat, C.byref(h))
        check(rc, "sblas_hip_gmres_plan_create")
        self.handle = h

    def info(self):
        out = (C.c_int64 * 14)()
        check(lib().sblas_hip_gmres_plan_info(self.handle, out), "sblas_hip_gmres_plan_info")
        return dict(n=int(out[0]), nnz=int(out[1]), restart=int(out[2]), precond=_PRECOND_NAME[out[3]], vectors=int(out[4]),
                    vector_bytes=int(out[5]), partial_bytes=int(out[6]), scalar_bytes=int(out[7]), matrix_bytes=int(out[8]),
                    bytes=int(out[9]), step_launches=int(out[10]), close_launches=int(out[11]), restart_launches=int(out[12]),
                    cycle_launches=int(out[13]))

    def start(self, val, b, x, lu=None, dinv=None, rtol=1e-8, atol=0.0, max_iter=1000, stream=None):
        """As KrylovPlan.start(); x is updated in place as cycles close.  x is b is refused before anything is looked at."""
        if x is b:
            raise SblasError("x must not be b")
        super().start(val, b, x, lu=lu, dinv=dinv, rtol=rtol, atol=atol, max_iter=max_iter, stream=stream)

    def status(self, stream=None):
        """Copies the scalar block back and synchronises the stream -> dict(status, code, iterations, rnorm, bnorm,
        restarts, columns, eta, breakdown): columns are the finished ones of the open cycle, breakdown a value of
        GMRES_DENOM or None."""
        import torch
        out = (C.c_double * 8)()
        with torch.cuda.device(self.device):
            check(lib().sblas_hip_gmres_status(self.handle, _stream(stream), out), "sblas_hip_gmres_status")
        return dict(status=KRYLOV_STATUS[int(out[0])], code=int(out[0]), iterations=int(out[1]), rnorm=float(out[2]), bnorm=float(out[3]),
                    restarts=int(out[4]), columns=int(out[5]), eta=float(out[6]), breakdown=GMRES_DENOM[int(out[7])])


def gmres(A, b, precond=None, restart=30, x=None, rtol=1e-8, atol=0.0, max_iter=1000, check_every=8):
    """x with A x = b by right-preconditioned restarted GMRES(restart), one shot, as pcg(); A need not be symmetric and
    max_iter counts Arnoldi steps."""
    return _krylov_one_shot(None, A, b, precond, x, dict(rtol=rtol, atol=atol, max_iter=max_iter, check_every=check_every),
                            make=lambda n, rowptr, colidx, pre: GmresPlan(n, rowptr, colidx, restart=restart, precond=pre))


# ------------------------------------------------------------------------------------------
# Restarted GMRES(m) for several right-hand sides on one SpMM per Arnoldi step (sblas_hip_gmres_multi_*)
# ------------------------------------------------------------------------------------------
def gmres_multi_limits():
    """The multi-right-hand-side GMRES's limits (sblas_gmres_multi_limits): dict(max_rhs, tile, cell, width, max_restart,
    fixed_blocks, block_slots, matrix_doubles).  A plan of restart m owns m + 1 + fixed_blocks blocks (AMG adds one)."""
    out = (C.c_int64 * 8)()
    check(lib().sblas_gmres_multi_limits(out), "sblas_gmres_multi_limits")
    keys = ("max_rhs", "tile", "cell", "width", "max_restart", "fixed_blocks", "block_slots", "matrix_doubles")
    return dict(zip(keys, (int(v) for v in out)))


def gmres_multi_grid(n, nrhs):
    """Workgroups of one multi-column pass (sblas_gmres_multi_grid): dict(cells, tiles, grid, last_tile)."""
    out = (C.c_int64 * 4)()
    check(lib().sblas_gmres_multi_grid(int(n), int(nrhs), out), "sblas_gmres_multi_grid")
    return dict(cells=int(out[0]), tiles=int(out[1]), grid=int(out[2]), last_tile=int(out[3]))


def gmres_multi_launches(restart=30, precond=None, spmm_launches=0):
    """Launches of the multi-right-hand-side GMRES (sblas_gmres_multi_launches) -> dict(step, close, restart, start, cycle):
    the single solver's with spmm_launches in the SpMV's place.  precond: None, "jacobi", an AmgPlan (its block cycle's
    launches are counted) or a pair of SptrsvPlans (the two tiled solves')."""
    kind = _multi_precond(precond)
    first = second = 0
    if isinstance(precond, AmgPlan):
        first = precond.multi_info()["launches"]
    elif _solver_pair(precond):
        first, second = precond[0].info()["launches"], precond[1].info()["launches"]
    out = (C.c_int64 * 4)()
    cycle = int(lib().sblas_gmres_multi_launches(int(restart), kind, int(spmm_launches), first, second, out))
    if cycle < 0:
        raise SblasError("sblas_gmres_multi_launches refused its arguments")
    return dict(step=int(out[0]), close=int(out[1]), restart=int(out[2]), start=int(out[3]), cycle=cycle)


def _gmres_multi_blocks(V, W, name):
    """V: k basis blocks as a (k, n, s) float64 GPU tensor with unit stride along a row (a view with a larger row or block
    stride serves); W: an (n, s) row-major block -> (k, n, s, ldv, block_stride, ldw)"""
    import torch
    if not isinstance(V, torch.Tensor) or not V.is_cuda:
        raise SblasError("V must be a GPU tensor (no CPU path exists)")
    if V.dtype != torch.float64 or V.dim() != 3:
        raise SblasError("V must be a float64 tensor of shape (blocks, n, nrhs)")
    k, n, s = (int(v) for v in V.shape)
    _multi_width(s)
    if not 1 <= k <= gmres_limits()["max_dots"]:
        raise SblasError("one to %d basis blocks, not %d" % (gmres_limits()["max_dots"], k))
    if s > 1 and V.stride(2) != 1:
        raise SblasError("a row of V must be contiguous")
    ldv = V.stride(1) if n > 1 else max(V.stride(1), s)
    if ldv < s:
        raise SblasError("the leading dimension %d of V is below nrhs = %d" % (ldv, s))
    stride = V.stride(0) if k > 1 else n * ldv
    if k > 1 and stride < n * ldv:
        raise SblasError("the block stride %d is below n * ld = %d" % (stride, n * ldv))
    return k, n, s, int(ldv), int(stride), _krylov_block(name, W, n, s, V.device)


def _gmres_multi_scalars(scalars, s, device):
    import torch
    if scalars is None:
        return None
    if not isinstance(scalars, torch.Tensor) or not scalars.is_cuda or scalars.dtype != torch.float64 or not scalars.is_contiguous() \
            or scalars.numel() != 16 * s or scalars.device != device:
        raise SblasError("scalars must be a contiguous float64 GPU tensor of %d x 16 slots" % s)
    return scalars.data_ptr()


def _gmres_multi_coef(name, H, s, k, device):
    """column c's k coefficients at H[c, :k]: an (s, >= k) float64 GPU tensor with unit stride along a row -> its row stride"""
    import torch
    if not isinstance(H, torch.Tensor) or not H.is_cuda or H.dtype != torch.float64 or H.dim() != 2 or H.device != device:
        raise SblasError("%s must be a 2-D float64 GPU tensor on the operands' device" % name)
    if H.shape[0] != s or H.shape[1] < k or (H.shape[1] > 1 and H.stride(1) != 1):
        raise SblasError("%s must hold %d rows of at least %d contiguous coefficients, got shape %s" % (name, s, k, tuple(H.shape)))
    return int(H.stride(0)) if s > 1 else max(int(H.stride(0)), k)


def gmres_multi_dots(V, W, scalars=None, out=None, workspace=None, stream=None):
    """out[i, c] = (V[i][:, c], W[:, c]) for up to 65 basis blocks in ONE pass over memory (sblas_hip_gmres_multi_dots_f64),
    each with exactly the bits krylov_dot gives on the two columns.  V: (k, n, s), see _gmres_multi_blocks; W: (n, s)
    row-major.  scalars: None, or an (s, 16) tensor of eight-byte slots whose slot 0 is a status as int64: a column
    that is not running is neither read nor written (its out entries keep what they held; zeros when made here).  No
    synchronisation; with out and workspace (float64, at least k * s * ceil(n / cell) entries) given, nothing is allocated."""
    import torch
    k, n, s, ldv, stride, ldw = _gmres_multi_blocks(V, W, "W")
    if out is None:
        out = torch.zeros((k, s), dtype=torch.float64, device=V.device)
    if not isinstance(out, torch.Tensor) or not out.is_cuda or out.dtype != torch.float64 or not out.is_contiguous() or out.numel() != k * s:
        raise SblasError("out must be a contiguous float64 GPU tensor of %d entries" % (k * s))
    need = int(lib().sblas_hip_gmres_multi_dots_workspace(n, s, k))
    if workspace is None:
        workspace = torch.empty(need // 8, dtype=torch.float64, device=V.device)
    if not isinstance(workspace, torch.Tensor) or not workspace.is_cuda or workspace.dtype != torch.float64 or not workspace.is_contiguous():
        raise SblasError("workspace must be a contiguous float64 GPU tensor")
    with torch.cuda.device(V.device):
        check(lib().sblas_hip_gmres_multi_dots_f64(-1, _stream(stream), n, s, k, V.data_ptr() if n else None, ldv, stride,
                                                   W.data_ptr() if n else None, ldw, _gmres_multi_scalars(scalars, s, V.device), out.data_ptr(),
                                                   workspace.data_ptr(), workspace.numel() * 8), "sblas_hip_gmres_multi_dots_f64")
    return out


def gmres_multi_project(V, H, W, partial=None, scalars=None, stream=None):
    """W[:, c] = W[:, c] - H[c, 0] V[0][:, c] - H[c, 1] V[1][:, c] - ... in place, ascending, each product and each
    difference rounded (sblas_hip_gmres_multi_project_f64).  partial: None, or a float64 tensor of at least s * ceil(n /
    cell) entries that receives the first stage of (w, w) over the new W, column c's cells at partial[c * cells:]."""
    import torch
    k, n, s, ldv, stride, ldw = _gmres_multi_blocks(V, W, "W")
    ldh = _gmres_multi_coef("H", H, s, k, V.device)
    if partial is not None:
        _krylov_vector("partial", partial, partial.numel() if isinstance(partial, torch.Tensor) else -1, V.device)
        if partial.numel() < s * -(-n // krylov_limits()["cell"]):
            raise SblasError("partial is too short")
    with torch.cuda.device(V.device):
        check(lib().sblas_hip_gmres_multi_project_f64(-1, _stream(stream), n, s, k, V.data_ptr() if n else None, ldv, stride, H.data_ptr(), ldh,
                                                      W.data_ptr() if n else None, ldw, _gmres_multi_scalars(scalars, s, V.device),
                                                      partial.data_ptr() if partial is not None and partial.numel() else None),
              "sblas_hip_gmres_multi_project_f64")
    return W


def gmres_multi_combine(V, Y, out=None, scalars=None, stream=None):
    """U[:, c] = Y[c, 0] V[0][:, c], then U[:, c] = U[:, c] + Y[c, l] V[l][:, c] ascending, rounded product and rounded sum
    (sblas_hip_gmres_multi_combine_f64) -> U (out when given, an (n, s) row-major block that is no part of V)."""
    import torch
    if out is None:
        if not isinstance(V, torch.Tensor) or V.dim() != 3:
            raise SblasError("V must be a float64 tensor of shape (blocks, n, nrhs)")
        out = torch.zeros(tuple(V.shape[1:]), dtype=torch.float64, device=V.device)
    k, n, s, ldv, stride, ldu = _gmres_multi_blocks(V, out, "out")
    ldy = _gmres_multi_coef("Y", Y, s, k, V.device)
    with torch.cuda.device(V.device):
        check(lib().sblas_hip_gmres_multi_combine_f64(-1, _stream(stream), n, s, k, V.data_ptr() if n else None, ldv, stride, Y.data_ptr(), ldy,
                                                      out.data_ptr() if n else None, ldu, _gmres_multi_scalars(scalars, s, V.device)),
              "sblas_hip_gmres_multi_combine_f64")
    return out


class GmresMultiPlan(_MultiSolverPlan):
    """Right-preconditioned restarted GMRES(restart) for A X = B with nrhs right-hand sides at once on the n x n CSR
    structure (rowptr, colidx), int32 indices (sblas_hip_gmres_multi_plan_create): nrhs independent GMRES(m) recurrences
    that share A and run in lockstep, one SpMM per Arnoldi step instead of nrhs SpMVs.  A need not be symmetric.  precond:
    as KrylovMultiPlan's -- None, "jacobi" (start / solve take dinv), an AmgPlan after its setup() with "jacobi" or "l1"
    (its block cycle), or the pair of SptrsvPlans ilu.solvers() returns (the two tiled solves; start / solve take lu).  B
    and X are (n, nrhs) float64 GPU tensors, row-major: contiguous, or a column slice of a wider tensor.  The plan owns an
    SpMM plan for this width, restart + 1 basis blocks, the work blocks, and one scalar and one small-matrix block a column.

    start() forms every r_c = b_c - A x_c and v_0; iterate(k) enqueues k lockstep steps -- a close and a restart behind
    every restart-th, a close at its end -- without allocating or synchronising (graph-capturable); status() is the one
    call that synchronises.  Every column has its own Hessenberg column, rotations and stopping test: once column c's
    test is met (or it breaks down) nothing reads or writes column c again but the close that applies its pending
    columns, so every column's x, count, |r| and restart count do not depend on check_every.  A solve equals the lockstep
    loop composed of the SpMM, the pinned dot per column, numpy updates and the scalar step bit for bit; it is NOT
    promised to equal a GmresPlan solve of one column, or a batch of another width."""

    _c = "gmres_multi"
    _columns = (("restarts", True), ("columns", True), ("eta", False))
    _denom = GMRES_DENOM

    def __init__(self, n, rowptr, colidx, nrhs, restart=30, precond=None, stream=None):
        import torch
        self.handle = None
        self.nrhs = _multi_width(nrhs)
        if isinstance(restart, bool) or not isinstance(restart, int) or not 1 <= restart <= gmres_multi_limits()["max_restart"]:
            raise SblasError("restart must be an integer in [1, %d], not %r" % (gmres_multi_limits()["max_restart"], restart))
        self.restart = restart
        lower, upper = self._seat_multi(n, rowptr, colidx, precond, stream)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            rc = lib().sblas_hip_gmres_multi_plan_create(-1, _stream(stream), n, self.nnz, rowptr.data_ptr(),
                                                         colidx.data_ptr() if self.nnz else None, self.nrhs, restart, self.precond_kind,
                                                         lower, upper, C.byref(h))
        check(rc, "sblas_hip_gmres_multi_plan_create")
        self.handle = h

    def info(self):
        out = (C.c_int64 * 16)()
        check(lib().sblas_hip_gmres_multi_plan_info(self.handle, out), "sblas_hip_gmres_multi_plan_info")
        return dict(n=int(out[0]), nnz=int(out[1]), restart=int(out[2]), precond=_PRECOND_NAME[out[3]], nrhs=int(out[4]), blocks=int(out[5]),
                    block_bytes=int(out[6]), partial_bytes=int(out[7]), scalar_bytes=int(out[8]), matrix_bytes=int(out[9]),
                    workspace_bytes=int(out[10]), bytes=int(out[11]), step_launches=int(out[12]), close_launches=int(out[13]),
                    restart_launches=int(out[14]), cycle_launches=int(out[15]))

    def block(self, k, stream=None):
        """A copy of block k of the plan as an (n, nrhs) tensor (sblas_hip_gmres_multi_plan_block): 0 .. restart are the
        basis blocks V_k, then W, U, Z.  Stream-ordered; allocates its result."""
        import torch
        out = torch.empty((self.n, self.nrhs), dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            check(lib().sblas_hip_gmres_multi_plan_block(self.handle, _stream(stream), int(k), out.data_ptr() if self.n else None),
                  "sblas_hip_gmres_multi_plan_block")
        return out


def gmres_multi(A, B, precond=None, restart=30, X=None, rtol=1e-8, atol=0.0, max_iter=1000, check_every=8):
    """X with A X = B by right-preconditioned restarted GMRES(restart) on all columns of B at once, one shot, as
    pcg_multi(): precond None, "jacobi", "amg" or "amg_smoothed"; A need not be symmetric and max_iter counts Arnoldi
    steps.  -> (X, status dict of per-column arrays).  The plans made here are destroyed before returning."""
    return _krylov_multi_one_shot(None, A, B, precond, X, dict(rtol=rtol, atol=atol, max_iter=max_iter, check_every=check_every),
                                  make=lambda n, rowptr, colidx, nrhs, pre: GmresMultiPlan(n, rowptr, colidx, nrhs, restart=restart, precond=pre))


# ------------------------------------------------------------------------------------------
# Eigenpairs of a symmetric matrix: thick-restart Lanczos on a plan (sblas_hip_eigsh_*)
# ------------------------------------------------------------------------------------------
EIGSH_WHICH = {"LA": 0, "SA": 1, "LM": 2}
EIGSH_DENOM = {0: None, 1: "v0", 2: "beta", 3: "t", 4: "invariant"}


def eigsh_limits():
    """The eigenvalue plan's limits (sblas_eigsh_limits): dict(max_ncv, default_ncv, ld, max_sweeps, block_slots,
    matrix_doubles, the offsets t, y, theta, rho, q, h, c in the small-matrix block, rotate_rows, ritz_threads)."""
    out = (C.c_int64 * 16)()
    check(lib().sblas_eigsh_limits(out), "sblas_eigsh_limits")
    names = ("max_ncv", "default_ncv", "ld", "max_sweeps", "block_slots", "matrix_doubles", "t", "y", "theta", "rho", "q", "h", "c",
             "rotate_rows", "ritz_threads")
    return {name: int(out[i]) for i, name in enumerate(names)}


def _eigsh_sizes(n, k, ncv, keep, which):
    """the refusals of k, ncv, keep and which, in the Krylov plans' style -> (ncv, keep) with the defaults put in"""
    lim = eigsh_limits()
    if which not in EIGSH_WHICH:
        raise SblasError("which must be 'LA', 'SA' or 'LM', not %r" % (which,))
    for name, v in (("n", n), ("k", k), ("ncv", ncv), ("keep", keep)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) and not (v is None and name in ("ncv", "keep")):
            raise SblasError("%s must be an integer, not %r" % (name, v))
    if k < 1:
        raise SblasError("k must be at least 1, not %d" % k)
    if ncv is None:
        ncv = min(max(2 * k + 1, lim["default_ncv"]), lim["max_ncv"], n - 1)
    if ncv > lim["max_ncv"]:
        raise SblasError("ncv must be at most %d, not %d" % (lim["max_ncv"], ncv))
    if ncv >= n:
        raise SblasError("ncv must be below n = %d, not %d" % (n, ncv))
    if k >= ncv:
        raise SblasError("k must be below ncv = %d, not %d" % (ncv, k))
    if keep is None:
        keep = k + (ncv - k) // 2
    if not k <= keep <= ncv - 1:
        raise SblasError("keep must be in [k, ncv - 1] = [%d, %d], not %d" % (k, ncv - 1, keep))
    return int(ncv), int(keep)


def eigsh_launches(ncv=20, keep=12):
    """Launches of the eigenvalue plan (sblas_eigsh_launches) -> dict(step, start, cycle, tail): a step's do not depend
    on its column; tail is the cycle's Ritz kernel and rotation."""
    out = (C.c_int64 * 4)()
    if int(lib().sblas_eigsh_launches(int(ncv), int(keep), out)) < 0:
        raise SblasError("sblas_eigsh_launches refused its arguments")
    return dict(step=int(out[0]), start=int(out[1]), cycle=int(out[2]), tail=int(out[3]))


def eigsh_jacobi_ref(T):
    """The cyclic Jacobi loop restated on the host (sblas_eigsh_jacobi_ref): T symmetric (mm, mm), finite -> dict(theta,
    Y, sweeps): the diagonal the loop ends with (unordered), the eigenvectors by columns, the sweeps that rotated."""
    T = np.asarray(T, dtype=np.float64)
    if T.ndim != 2 or T.shape[0] != T.shape[1] or not 1 <= T.shape[0] <= eigsh_limits()["max_ncv"]:
        raise SblasError("T must be square with 1 to %d rows, got shape %s" % (eigsh_limits()["max_ncv"], T.shape))
    mm = T.shape[0]
    cols = np.ascontiguousarray(T.T)
    theta, Y, sweeps = np.zeros(mm), np.zeros((mm, mm)), C.c_int(0)
    check(lib().sblas_eigsh_jacobi_ref(mm, cols.ctypes.data, mm, theta.ctypes.data, Y.ctypes.data, mm, C.byref(sweeps)), "sblas_eigsh_jacobi_ref")
    return dict(theta=theta, Y=np.ascontiguousarray(Y.T), sweeps=int(sweeps.value))


def eigsh_step_ref(j, h, beta, T=None, matvecs=0):
    """The scalar part of step j's last fold restated on the host (sblas_eigsh_step_ref): h, the j + 1 coefficients,
    becomes column j and row j of T ((ncv, ncv), updated in a copy; zeros when None), the matvec is counted and beta
    decides -> dict(T, columns, matvecs, beta, forms (v_{j+1} = w / beta is formed), invariant, status, breakdown)."""
    lim = eigsh_limits()
    h = np.ascontiguousarray(h, dtype=np.float64)
    if not 0 <= int(j) < lim["max_ncv"] or h.shape != (int(j) + 1,):
        raise SblasError("0 <= j < %d and h of j + 1 entries, not j = %r and h of shape %s" % (lim["max_ncv"], j, h.shape))
    T = np.zeros((j + 1, j + 1)) if T is None else np.array(T, dtype=np.float64)
    if T.ndim != 2 or T.shape[0] != T.shape[1] or not j < T.shape[0] <= lim["max_ncv"]:
        raise SblasError("T must be square with j + 1 to %d rows, got shape %s" % (lim["max_ncv"], T.shape))
    blk, mat = _eigsh_blocks(T, 0.0, 0.0, 0.0, 0, 0, False, 0)
    blk[2], blk[3] = int(matvecs), int(j)
    forms = int(lib().sblas_eigsh_step_ref(int(j), h.ctypes.data, float(beta), blk.ctypes.data, mat.ctypes.data))
    if forms < 0:
        raise SblasError("sblas_eigsh_step_ref refused its arguments")
    ld, m = lim["ld"], T.shape[0]
    return dict(T=mat[lim["t"]:lim["t"] + ld * ld].reshape(ld, ld).T[:m, :m].copy(), columns=int(blk[3]), matvecs=int(blk[2]),
                beta=float(blk.view(np.float64)[4]), forms=bool(forms), invariant=bool(blk[12]), status=KRYLOV_STATUS[int(blk[0])],
                breakdown=EIGSH_DENOM[int(blk[5])])


def _eigsh_blocks(T, beta, rtol, atol, restarts, max_restarts, invariant, status):
    """the two blocks of a Ritz step over T's mm columns as host arrays: (blk as int64 with a float64 view, mat)"""
    lim = eigsh_limits()
    T = np.asarray(T, dtype=np.float64)
    if T.ndim != 2 or T.shape[0] != T.shape[1] or not 1 <= T.shape[0] <= lim["max_ncv"]:
        raise SblasError("T must be square with 1 to %d rows, got shape %s" % (lim["max_ncv"], T.shape))
    mm, ld = T.shape[0], lim["ld"]
    blk = np.zeros(lim["block_slots"], dtype=np.int64)
    fb = blk.view(np.float64)
    blk[0], blk[1], blk[3], blk[10], blk[12] = int(status), int(restarts), mm, int(max_restarts), 1 if invariant else 0
    fb[4], fb[8], fb[9] = float(beta), float(rtol), float(atol)
    mat = np.zeros(lim["matrix_doubles"])
    mat[lim["t"]:lim["t"] + ld * ld].reshape(ld, ld)[:mm, :mm] = T.T
    return blk, mat


def _eigsh_ritz_result(blk, mat, mm):
    lim = eigsh_limits()
    ld, fb = lim["ld"], blk.view(np.float64)
    square = lambda key: mat[lim[key]:lim[key] + ld * ld].reshape(ld, ld).T.copy()
    kk = int(blk[14])
    return dict(status=KRYLOV_STATUS[int(blk[0])], code=int(blk[0]), restarts=int(blk[1]), converged=int(blk[11]), columns=int(blk[3]),
                breakdown=EIGSH_DENOM[int(blk[5])], act=int(blk[6]), mm=int(blk[13]), kk=kk, beta=float(fb[4]),
                theta=mat[lim["theta"]:lim["theta"] + mm].copy(), residuals=mat[lim["rho"]:lim["rho"] + mm].copy(),
                T=square("t"), Y=square("y"), Q=square("q")[:mm, :kk].copy(), blk=blk.copy(), mat=mat.copy())


def _eigsh_ritz_args(k, keep, which):
    if which not in EIGSH_WHICH:
        raise SblasError("which must be 'LA', 'SA' or 'LM', not %r" % (which,))
    if not 1 <= int(k) <= int(keep) <= eigsh_limits()["max_ncv"] - 1:
        raise SblasError("1 <= k <= keep <= %d, not k = %r, keep = %r" % (eigsh_limits()["max_ncv"] - 1, k, keep))
    return int(k), int(keep), EIGSH_WHICH[which]


def eigsh_ritz_ref(T, beta, k, keep, which="LA", rtol=1e-8, atol=0.0, restarts=0, max_restarts=300, invariant=False, status=0):
    """The whole Ritz step restated on the host (sblas_eigsh_ritz_ref) over the mm = T.shape[0] finished columns ->
    dict(status, code, restarts, converged, columns, breakdown, act, mm, kk, beta, theta, residuals (mm each, in the
    order of which), T, Y (64 x 64, as rows and columns), Q (mm x kk), blk, mat (the raw blocks))."""
    k, keep, w = _eigsh_ritz_args(k, keep, which)
    blk, mat = _eigsh_blocks(T, beta, rtol, atol, restarts, max_restarts, invariant, status)
    check(lib().sblas_eigsh_ritz_ref(k, keep, w, blk.ctypes.data, mat.ctypes.data), "sblas_eigsh_ritz_ref")
    return _eigsh_ritz_result(blk, mat, np.asarray(T).shape[0])


def eigsh_ritz(T, beta, k, keep, which="LA", rtol=1e-8, atol=0.0, restarts=0, max_restarts=300, invariant=False, status=0,
               device=None, stream=None):
    """The Ritz kernel alone (sblas_hip_eigsh_ritz_f64): the host arrays of eigsh_ritz_ref go to the device, one workgroup
    runs, and everything comes back -> the same dict.  Synchronises (a test and measurement door, not a solver's)."""
    import torch
    k, keep, w = _eigsh_ritz_args(k, keep, which)
    blk, mat = _eigsh_blocks(T, beta, rtol, atol, restarts, max_restarts, invariant, status)
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    dblk, dmat = torch.from_numpy(blk).to(device), torch.from_numpy(mat).to(device)
    with torch.cuda.device(device):
        check(lib().sblas_hip_eigsh_ritz_f64(-1, _stream(stream), k, keep, w, dblk.data_ptr(), dmat.data_ptr()), "sblas_hip_eigsh_ritz_f64")
    return _eigsh_ritz_result(dblk.cpu().numpy(), dmat.cpu().numpy(), np.asarray(T).shape[0])


def eigsh_rotate_ref(V, Q):
    """The basis rotation restated on the host (sblas_eigsh_rotate_ref).  V: (mm + 1, n) rows as columns of the basis; Q:
    (mm, keep).  -> a new (mm + 1, n) array: rows 0 .. keep - 1 are sum_l Q[l][i] V[l] in gmres_combine's order, row keep
    is row mm, the others are unchanged."""
    V = np.array(V, dtype=np.float64, order="C")
    Q = np.asarray(Q, dtype=np.float64)
    if V.ndim != 2 or Q.ndim != 2 or V.shape[0] != Q.shape[0] + 1 or not 1 <= Q.shape[1] <= Q.shape[0] <= eigsh_limits()["max_ncv"]:
        raise SblasError("V must be (mm + 1, n) and Q (mm, keep) with 1 <= keep <= mm <= %d, got %s and %s"
                         % (eigsh_limits()["max_ncv"], V.shape, Q.shape))
    mm, keep = Q.shape
    n = V.shape[1]
    cols = np.ascontiguousarray(Q.T)
    check(lib().sblas_eigsh_rotate_ref(n, mm, keep, V.ctypes.data, max(n, 1), cols.ctypes.data, mm), "sblas_eigsh_rotate_ref")
    return V


def eigsh_rotate(V, Q, stream=None):
    """V[i] <- sum_l Q[l][i] V[l] for i < keep over l < mm, in place and in ONE pass over V, and V[keep] <- V[mm]
    (sblas_hip_eigsh_rotate_f64): row i has exactly the bits of gmres_combine(V[:mm], Q[:, i]).  V: (mm + 1, n) float64 on
    the GPU, each row contiguous, rows a constant stride >= n apart (see _gmres_columns); Q: (mm, keep) float64 on the
    same device.  No synchronisation.  -> V."""
    import torch
    k1, n, ldv = _gmres_columns(V, eigsh_limits()["max_ncv"] + 1)
    if not isinstance(Q, torch.Tensor) or Q.dtype != torch.float64 or Q.device != V.device or Q.dim() != 2:
        raise SblasError("Q must be a float64 (mm, keep) tensor on V's device")
    mm, keep = int(Q.shape[0]), int(Q.shape[1])
    if k1 != mm + 1 or not 1 <= keep <= mm:
        raise SblasError("V must have mm + 1 = %d rows and 1 <= keep <= mm, got %d rows and keep = %d" % (mm + 1, k1, keep))
    cols = Q.t().contiguous()
    with torch.cuda.device(V.device):
        check(lib().sblas_hip_eigsh_rotate_f64(-1, _stream(stream), n, mm, keep, V.data_ptr() if n else None, ldv, cols.data_ptr(), mm),
              "sblas_hip_eigsh_rotate_f64")
    return V


class _DeviceColumns:
    """k columns of n doubles a column stride apart in a plan's device memory, as the array interface torch reads: what
    lets EigshPlan.vectors() be a view.  Holds the plan, so the plan object outlives every view."""

    def __init__(self, owner, ptr, k, n, ld):
        self.owner = owner
        self.__cuda_array_interface__ = dict(shape=(k, n), typestr="<f8", data=(ptr, False), version=2, strides=(ld * 8, 8))


class EigshPlan:
    """k eigenpairs at one end of the spectrum of a SYMMETRIC n x n CSR matrix (rowptr, colidx), int32 indices, fp64
    values, by thick-restart Lanczos with full reorthogonalisation, resident on the device (sblas_hip_eigsh_plan_create).
    Symmetry is the caller's promise, as with PCG: it is not checked, and a matrix that is not symmetric gives numbers
    that mean nothing.  which: "LA" (largest), "SA" (smallest) or "LM" (largest magnitude).  1 <= k < ncv <= min(64, n -
    1), default ncv = min(max(2 k + 1, 20), 64, n - 1); k <= keep <= ncv - 1 Ritz vectors survive a restart, default k +
    (ncv - k) // 2.  spmv_plan: an SpmvPlan on the same tensors, or None.  seed: of the default start vector.

    A single-vector Lanczos method finds ONE copy of a multiple eigenvalue.  On a matrix whose wanted eigenvalues are not
    simple (the square-grid Laplacian is one) the k values returned can all have small residuals and still not be the k
    extremal eigenvalues counted with multiplicity; that needs a block method.

    start() normalises v0 and enqueues the first `keep` steps; iterate(cycles) enqueues restart cycles without allocating
    or synchronising (graph-capturable, always the same chain); status() is the one call that synchronises.  Once the
    status is not "running", cycles already enqueued change nothing.  Every bit is pinned (include/sblas_hip_eigsh.h)."""

    def __init__(self, n, rowptr, colidx, k, ncv=None, which="LA", keep=None, spmv_plan=None, seed=0, stream=None):
        import torch
        self.handle = None
        self.ncv, self.keep = _eigsh_sizes(n, k, ncv, keep, which)
        self.k, self.which, self.seed = int(k), which, int(seed) & 0xffffffff
        self.n, self.nnz = n, _structure(n, rowptr, colidx)
        self.rowptr, self.colidx, self.device, self.spmv_plan = rowptr, colidx, rowptr.device, spmv_plan
        if spmv_plan is not None and not isinstance(spmv_plan, SpmvPlan):
            raise SblasError("spmv_plan must be an SpmvPlan or None")
        self._keep = None
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            rc = lib().sblas_hip_eigsh_plan_create(-1, _stream(stream), n, self.nnz, rowptr.data_ptr(), colidx.data_ptr() if self.nnz else None,
                                                   self.k, self.ncv, self.keep, EIGSH_WHICH[which],
                                                   spmv_plan.handle if spmv_plan is not None else None, self.seed, C.byref(h))
        check(rc, "sblas_hip_eigsh_plan_create")
        self.handle = h

    def info(self):
        out = (C.c_int64 * 14)()
        check(lib().sblas_hip_eigsh_info(self.handle, out), "sblas_hip_eigsh_info")
        return dict(n=int(out[0]), nnz=int(out[1]), k=int(out[2]), ncv=int(out[3]), keep=int(out[4]),
                    which=[w for w, v in EIGSH_WHICH.items() if v == out[5]][0], vectors=int(out[3]) + 2, vector_bytes=int(out[6]),
                    partial_bytes=int(out[7]), scalar_bytes=int(out[8]), matrix_bytes=int(out[9]), bytes=int(out[10]),
                    step_launches=int(out[11]), start_launches=int(out[12]), cycle_launches=int(out[13]))

    def start(self, val, v0=None, rtol=1e-8, atol=0.0, max_restarts=300, stream=None):
        """Begins a solve on the values val: v0 (n doubles, or None: cheby_start_ref's hashed vector with the plan's seed)
        is normalised and the first `keep` steps are enqueued.  Every refusal comes before any launch."""
        import torch
        _krylov_vector("val", val, self.nnz, self.device)
        if v0 is not None:
            _krylov_vector("v0", v0, self.n, self.device)
        if not (rtol >= 0.0 and atol >= 0.0) or int(max_restarts) < 0:
            raise SblasError("rtol and atol must be >= 0 and max_restarts >= 0")
        with torch.cuda.device(self.device):
            rc = lib().sblas_hip_eigsh_start(self.handle, _stream(stream), val.data_ptr() if self.nnz else None,
                                             v0.data_ptr() if v0 is not None else None, float(rtol), float(atol), int(max_restarts))
        check(rc, "sblas_hip_eigsh_start")
        self._keep = (val, v0)

    def iterate(self, cycles, stream=None):
        """Enqueues `cycles` restart cycles (steps keep .. ncv - 1, the Ritz kernel, the rotation): allocates nothing,
        never synchronises, graph-capturable as a chain."""
        import torch
        with torch.cuda.device(self.device):
            check(lib().sblas_hip_eigsh_iterate(self.handle, _stream(stream), int(cycles)), "sblas_hip_eigsh_iterate")

    def status(self, stream=None):
        """Copies the scalar block and the first k Ritz values and estimates back and synchronises the stream ->
        dict(status, code, restarts, matvecs, converged, theta, residuals, breakdown, columns, beta): converged counts the
        first k estimates that met the test; breakdown is a value of EIGSH_DENOM ("invariant": the Krylov space ended at
        `columns` < k columns)."""
        import torch
        out, theta, res = (C.c_double * 8)(), np.zeros(self.k), np.zeros(self.k)
        with torch.cuda.device(self.device):
            check(lib().sblas_hip_eigsh_status(self.handle, _stream(stream), out, theta.ctypes.data, res.ctypes.data), "sblas_hip_eigsh_status")
        return dict(status=KRYLOV_STATUS[int(out[0])], code=int(out[0]), restarts=int(out[1]), matvecs=int(out[2]), converged=int(out[3]),
                    theta=theta, residuals=res, breakdown=EIGSH_DENOM[int(out[5])], columns=int(out[6]), beta=float(out[4]))

    def values(self, stream=None):
        """The k Ritz values in the order of which, as a device tensor.  No synchronisation."""
        import torch
        out = torch.empty(self.k, dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            check(lib().sblas_hip_eigsh_values(self.handle, _stream(stream), out.data_ptr()), "sblas_hip_eigsh_values")
        return out

    def vectors(self, copy=False):
        """The first k columns of V as a (k, n) device tensor, row i the Ritz vector of values()[i] once the solve has
        ended: a VIEW of the plan's memory (rows a column stride apart), which the next start overwrites and destroy()
        frees; the view keeps the plan object alive but cannot keep it from being destroyed.  copy=True gives a tensor of
        its own.  No launch, no synchronisation: work already enqueued on the stream writes into what the view shows."""
        import torch
        ptr, ldv = C.c_void_p(), C.c_int64()
        check(lib().sblas_hip_eigsh_vectors(self.handle, C.byref(ptr), C.byref(ldv)), "sblas_hip_eigsh_vectors")
        view = torch.as_tensor(_DeviceColumns(self, ptr.value, self.k, self.n, ldv.value), device=self.device)
        return view.clone() if copy else view

    def solve(self, val, v0=None, rtol=1e-8, atol=0.0, max_restarts=300, check_every=1, stream=None):
        """start(), then iterate(check_every) / status() until the status is not "running" -> (values, vectors, status
        dict); vectors is vectors()'s view.  The result does not depend on check_every."""
        if int(check_every) < 1:
            raise SblasError("check_every must be at least 1")
        self.start(val, v0=v0, rtol=rtol, atol=atol, max_restarts=max_restarts, stream=stream)
        while True:
            self.iterate(int(check_every), stream=stream)
            st = self.status(stream=stream)
            if st["code"] != KRYLOV_RUNNING:
                return self.values(stream=stream), self.vectors(), st

    def destroy(self):
        if self.handle:
            lib().sblas_hip_eigsh_destroy(self.handle)
            self.handle = None
        self._keep = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


def eigsh(A, k, which="LA", ncv=None, keep=None, v0=None, rtol=1e-8, atol=0.0, max_restarts=300, check_every=1, seed=0):
    """k eigenpairs of the symmetric A = (n, rowptr, colidx, val) (GPU tensors), one shot, as pcg() is -> (values (k),
    vectors (k, n), status dict).  See EigshPlan for the limits, and for what a multiple eigenvalue does to the answer.
    The plan made here is destroyed before returning."""
    n, rowptr, colidx, val = A
    plan = EigshPlan(n, rowptr, colidx, k, ncv=ncv, which=which, keep=keep, seed=seed)
    try:
        values, vectors, st = plan.solve(val, v0=v0, rtol=rtol, atol=atol, max_restarts=max_restarts, check_every=check_every)
        return values, vectors.clone(), st                                   # the plan's memory ends with the plan
    finally:
        plan.destroy()


# ------------------------------------------------------------------------------------------
# SDDMM on a CSR pattern (sblas_hip_sddmm_csr_f64_i32)
# ------------------------------------------------------------------------------------------
def sddmm_workspace_bytes(rows, cols, nnz, k, order_x=ROW_MAJOR, order_y=ROW_MAJOR):
    """Bytes of workspace of an SDDMM call: 0 when both operands are ROW_MAJOR, a row-major copy per COL_MAJOR operand."""
    return int(lib().sblas_hip_sddmm_csr_workspace(rows, cols, nnz, k, order_x, order_y))


def _sddmm_call(rows, cols, nnz, prow, pcol, px, ldx, order_x, py, ldy, order_y, k, alpha, beta, pout, workspace, stream):
    if workspace is not None and not workspace.is_contiguous():
        raise SblasError("workspace must be contiguous")
    wptr = workspace.data_ptr() if workspace is not None and workspace.numel() else None
    wbytes = workspace.numel() * workspace.element_size() if workspace is not None else 0
    check(lib().sblas_hip_sddmm_csr_f64_i32(-1, _stream(stream), rows, cols, nnz, prow, pcol, px, ldx, order_x, py, ldy, order_y,
                                            k, alpha, beta, pout, wptr, wbytes), "sblas_hip_sddmm_csr_f64_i32")


def sddmm(rows, cols, rowptr, colidx, X, ldx, order_x, Y, ldy, order_y, k, alpha, beta, out, workspace=None, stream=None,
          x_offset=0, nnz=None):
    """out[e] = alpha * <X[row(e), :], Y[col(e), :]> + beta * out[e] over the pattern (rowptr, colidx).  X (rows x k), Y
    (cols x k): flat device tensors, each COL_MAJOR or ROW_MAJOR; x_offset: element offset into X (a re-based row block
    points X at its first row).  out: nnz values in CSR order.  workspace: a device tensor of at least
    sddmm_workspace_bytes(...) bytes, needed only for COL_MAJOR operands."""
    import torch
    nnz = int(colidx.numel()) if nnz is None else int(nnz)
    px = _dev_ptr(X, torch.float64, "X") + 8 * x_offset if k and nnz else None
    py = _dev_ptr(Y, torch.float64, "Y") if k and nnz else None
    _sddmm_call(rows, cols, nnz, _dev_ptr(rowptr, torch.int32, "rowptr"), _dev_ptr(colidx, torch.int32, "colidx") if nnz else None,
                px, ldx, order_x, py, ldy, order_y, k, alpha, beta, _dev_ptr(out, torch.float64, "out") if nnz else None,
                workspace, stream)


def sddmm_tensor(A, X, Y, out, alpha=1.0, beta=0.0, workspace=None, stream=None):
    """SDDMM on 2-D torch tensors without a copy: A = (rows, cols, rowptr, colidx), X rows x k and Y cols x k with order and
    leading dimension taken from their strides (as spmm_tensor), out a contiguous float64 tensor of nnz entries.
    workspace: None (allocated here when a column-major operand needs one) or a device tensor of at least
    sddmm_workspace_bytes(...) bytes."""
    import torch
    rows, cols, rowptr, colidx = A
    if rowptr.dtype != torch.int32 or colidx.dtype != torch.int32:
        raise SblasError("sddmm_tensor handles float64 values and int32 indices only")
    if not isinstance(X, torch.Tensor) or not isinstance(Y, torch.Tensor) or X.dim() != 2 or Y.dim() != 2:
        raise SblasError("X and Y must be 2-D tensors")
    if X.dtype != torch.float64 or Y.dtype != torch.float64:
        raise SblasError("X and Y must be float64 (sddmm_tensor handles float64 values and int32 indices only)")
    k = int(X.shape[1])
    order_x, ldx = _layout(X, rows, k, "X")      # shapes and strides first: they are wrong on any device
    order_y, ldy = _layout(Y, cols, k, "Y")
    px, py = _view_ptr(X, "X"), _view_ptr(Y, "Y")
    nnz = int(colidx.numel())
    if rowptr.numel() != rows + 1:
        raise SblasError("rowptr has %d entries for %d rows" % (rowptr.numel(), rows))
    if out.dim() != 1 or out.numel() != nnz:
        raise SblasError("out must hold one value per stored entry (%d), got shape %s" % (nnz, tuple(out.shape)))
    pout = _dev_ptr(out, torch.float64, "out")
    need = sddmm_workspace_bytes(rows, cols, nnz, k, order_x, order_y)
    if workspace is None and need:
        workspace = torch.empty((need + 7) // 8, dtype=torch.float64, device=out.device)
    _sddmm_call(rows, cols, nnz, _dev_ptr(rowptr, torch.int32, "rowptr"), _dev_ptr(colidx, torch.int32, "colidx") if nnz else None,
                px if k and nnz else None, ldx, order_x, py if k and nnz else None, ldy, order_y, k, alpha, beta,
                pout if nnz else None, workspace, stream)


def _narrow_operand(t, n, what):
    """(pointer, leading dimension, k) of a row-major operand of the narrow SDDMM: n x k with strides (ld, 1), or 1-D (k = 1,
    any positive stride)"""
    import torch
    if not isinstance(t, torch.Tensor) or t.dim() not in (1, 2) or t.shape[0] != n:
        raise SblasError("%s must be a tensor of %d rows with 1 or 2 dimensions" % (what, n))
    if t.dtype != torch.float64:
        raise SblasError("%s must be float64 (sddmm_narrow handles float64 values and int32 indices only)" % what)
    if not t.is_cuda:
        raise SblasError("%s must be a GPU tensor (no CPU path exists)" % what)
    if t.dim() == 1:
        ld = int(t.stride(0)) if n > 1 else 1
        if ld < 1:
            raise SblasError("%s has stride %d: a 1-D operand needs a positive stride" % (what, ld))
        return t.data_ptr(), ld, 1
    k = int(t.shape[1])
    order, ld = _layout(t, n, k, what)
    if order != ROW_MAJOR and k > 1 and n > 1:
        raise SblasError("%s must be row-major (strides (ld, 1)): the narrow SDDMM stages nothing" % what)
    if order != ROW_MAJOR:                         # one row or one column: the strides name no order
        ld = int(t.stride(0)) if k == 1 and n > 1 else max(k, 1)
    return t.data_ptr(), int(ld), k


def sddmm_narrow(A, X, Y, out, alpha=1.0, beta=0.0, part="all", stream=None):
    """The narrow SDDMM (sblas_hip_sddmm_narrow_f64_i32): out[e] = alpha * <X[row(e), :k], Y[col(e), :k]> + beta * out[e]
    for the stored entries of A = (rows, cols, rowptr, colidx) that lie in `part` ("all", "lower": col <= row, "upper",
    "strict_lower", "strict_upper"); an entry outside gets +0.0 (beta == 0) or beta * out[e], and its rows of X and Y are
    never read.  X rows x k and Y cols x k are row-major views (strides (ld, 1)) with 1 <= k <= 8; a 1-D X or Y is k = 1.
    out: a contiguous float64 tensor of nnz entries.  For part="all" the bits are sddmm_tensor's; one launch, no
    workspace, graph-capturable."""
    import torch
    rows, cols, rowptr, colidx = A
    if not isinstance(rowptr, torch.Tensor) or not isinstance(colidx, torch.Tensor) or rowptr.dtype != torch.int32 or colidx.dtype != torch.int32:
        raise SblasError("sddmm_narrow handles float64 values and int32 indices only")
    px, ldx, kx = _narrow_operand(X, rows, "X")
    py, ldy, ky = _narrow_operand(Y, cols, "Y")
    if kx != ky:
        raise SblasError("X and Y must have the same number of columns, got %d and %d" % (kx, ky))
    nnz = int(colidx.numel())
    if rowptr.numel() != rows + 1:
        raise SblasError("rowptr has %d entries for %d rows" % (rowptr.numel(), rows))
    if not isinstance(out, torch.Tensor) or out.dim() != 1 or out.numel() != nnz:
        raise SblasError("out must hold one value per stored entry (%d)" % nnz)
    pout = _dev_ptr(out, torch.float64, "out")
    prow, pcol = _dev_ptr(rowptr, torch.int32, "rowptr"), _dev_ptr(colidx, torch.int32, "colidx")
    for name, t in (("colidx", colidx), ("X", X), ("Y", Y), ("out", out)):
        if t.device != rowptr.device:
            raise SblasError("%s is on %s, the pattern on %s" % (name, t.device, rowptr.device))
    if nnz:                                        # the kernel reads X and Y while it writes out: the extents must be apart
        for name, p, ld, n in (("X", px, ldx, rows), ("Y", py, ldy, cols)):
            if n and pout < p + 8 * ((n - 1) * ld + kx) and p < pout + 8 * nnz:
                raise SblasError("out must not overlap %s" % name)
    with torch.cuda.device(rowptr.device):
        check(lib().sblas_hip_sddmm_narrow_f64_i32(-1, _stream(stream), rows, cols, nnz, prow, pcol if nnz else None, px if nnz else None,
                                                   ldx, py if nnz else None, ldy, kx, float(alpha), float(beta), _part(part),
                                                   pout if nnz else None), "sblas_hip_sddmm_narrow_f64_i32")
    return out


# ------------------------------------------------------------------------------------------
# Row-wise softmax on a CSR pattern (sblas_hip_csr_softmax_f64_i32 and its backward)
# ------------------------------------------------------------------------------------------
def csr_softmax_workspace_bytes(rows, nnz):
    """Bytes of workspace of a softmax call or its backward: a function of rows and nnz alone, 0 while no row can be
    longer than 4096 entries."""
    return int(lib().sblas_hip_csr_softmax_workspace(rows, nnz))


def _softmax_args(rowptr, tensors, workspace):
    """(rows, nnz, row pointer, value pointers, workspace pointer, workspace bytes, workspace) of a softmax call on 1-D
    float64 GPU tensors of equal length; the checks come before anything touches the device"""
    import torch
    if not isinstance(rowptr, torch.Tensor) or rowptr.dim() != 1 or rowptr.numel() < 1:
        raise SblasError("rowptr must be a 1-D tensor of rows + 1 entries")
    if rowptr.dtype != torch.int32:
        raise SblasError("csr_softmax handles float64 values and int32 row pointers only")
    rows = int(rowptr.numel()) - 1
    for what, t in tensors:                          # dtypes and shapes first: they are wrong on any device
        if not isinstance(t, torch.Tensor):
            raise SblasError("%s must be a GPU tensor (no CPU path exists)" % what)
        if t.dtype != torch.float64:
            raise SblasError("%s must be float64, got %s" % (what, t.dtype))
        if t.dim() != 1 or t.numel() != tensors[0][1].numel():
            raise SblasError("%s must hold one value per stored entry (%d), got shape %s" % (what, tensors[0][1].numel(),
                                                                                            tuple(t.shape)))
    nnz = int(tensors[0][1].numel())
    for what, t in tensors:
        if not t.is_cuda:
            raise SblasError("%s must be a GPU tensor (no CPU path exists)" % what)
    prow = _dev_ptr(rowptr, torch.int32, "rowptr")
    ptrs = [_dev_ptr(t, torch.float64, what) if nnz else None for what, t in tensors]
    need = csr_softmax_workspace_bytes(rows, nnz)
    if workspace is None and need:
        workspace = torch.empty((need + 7) // 8, dtype=torch.float64, device=tensors[0][1].device)
    if workspace is not None and not workspace.is_contiguous():
        raise SblasError("workspace must be contiguous")
    wptr = workspace.data_ptr() if workspace is not None and workspace.numel() else None
    wbytes = workspace.numel() * workspace.element_size() if workspace is not None else 0
    return rows, nnz, prow, ptrs, wptr, wbytes, workspace


def csr_softmax(rowptr, x, out=None, scale=1.0, workspace=None, stream=None):
    """out[e] = exp(scale * x[e] - m) / s over the stored entries of each row of the pattern `rowptr` (int32, rows + 1
    entries, relative to x).  x: nnz float64 values on the GPU; out: the same (None: a new tensor; x itself: in place).
    Precondition: x holds exactly rowptr[-1] values.  nnz is taken from x, and this call has no colidx to check it
    against (sddmm_tensor and CsrOperator do): with a shorter x the kernels read and write past its end.  SBLAS_VALIDATE=1
    refuses a rowptr that is not monotone or does not end at nnz, at the price of a synchronisation.
    workspace: None (allocated here when rows may exceed 4096 entries) or a device tensor of at least
    csr_softmax_workspace_bytes(rows, nnz) bytes.  Returns out."""
    import torch
    if out is None and isinstance(x, torch.Tensor):
        out = torch.empty_like(x)
    rows, nnz, prow, (px, pout), wptr, wbytes, _keep = _softmax_args(rowptr, [("x", x), ("out", out)], workspace)
    check(lib().sblas_hip_csr_softmax_f64_i32(-1, _stream(stream), rows, nnz, prow, px, float(scale), pout, wptr, wbytes),
          "sblas_hip_csr_softmax_f64_i32")
    return out


def csr_softmax_backward(rowptr, p, dp, dx=None, scale=1.0, workspace=None, stream=None):
    """dx[e] = scale * p[e] * (dp[e] - sum over the row of p * dp): the gradient of csr_softmax with respect to x, from
    its output p and the gradient dp of that output.  dx: None (a new tensor), or a tensor of nnz entries (dp itself: in
    place).  The precondition of csr_softmax holds here too: p, dp and dx hold exactly rowptr[-1] values.  Returns dx."""
    import torch
    if dx is None and isinstance(dp, torch.Tensor):
        dx = torch.empty_like(dp)
    rows, nnz, prow, (pp, pdp, pdx), wptr, wbytes, _keep = _softmax_args(rowptr, [("p", p), ("dp", dp), ("dx", dx)], workspace)
    check(lib().sblas_hip_csr_softmax_backward_f64_i32(-1, _stream(stream), rows, nnz, prow, pp, pdp, float(scale), pdx, wptr,
                                                       wbytes), "sblas_hip_csr_softmax_backward_f64_i32")
    return dx


# ------------------------------------------------------------------------------------------
# Fused attention on a CSR pattern (sblas_hip_csr_attention_f64_i32 and its backward)
# ------------------------------------------------------------------------------------------
ATTENTION_MAX_WIDTH = 128      # widest Q / K / V row the fused kernels take


def csr_attention_workspace_bytes(rows, nnz, d, dv):
    """Bytes of workspace of a fused attention call or its backward: a function of (rows, nnz, d, dv) alone, 0 while no
    row can be longer than 4096 entries; about nnz / 4096 rows of max(d, dv) doubles otherwise, never nnz itself."""
    return int(lib().sblas_hip_csr_attention_workspace(rows, nnz, d, dv))


def _attention_dense(t, rows, width, what):
    """leading dimension of a row-major 2-D float64 tensor of `rows` rows (and `width` columns when given)"""
    import torch
    if not isinstance(t, torch.Tensor):
        raise SblasError("%s must be a GPU tensor (no CPU path exists)" % what)
    if t.dtype != torch.float64:
        raise SblasError("%s must be float64, got %s" % (what, t.dtype))
    if t.dim() != 2 or t.shape[0] != rows or (width is not None and t.shape[1] != width):
        raise SblasError("%s must be a %d x %s tensor, got shape %s" % (what, rows, "k" if width is None else width, tuple(t.shape)))
    w = int(t.shape[1])
    if not 1 <= w <= ATTENTION_MAX_WIDTH:
        raise SblasError("%s has %d columns: the fused attention kernels take 1 .. %d" % (what, w, ATTENTION_MAX_WIDTH))
    order, ld = _layout(t, rows, w, what)
    if order != ROW_MAJOR and rows > 1 and w > 1:
        raise SblasError("%s must be row-major (strides (ld, 1)) for the fused attention kernels, got strides %s" %
                         (what, tuple(t.stride())))
    return ld if order == ROW_MAJOR else w


def _attention_args(A, Q, K, V, others, workspace):
    """the checks csr_attention and csr_attention_backward share, shapes and dtypes before devices; `others`: (name,
    tensor, rows, width) of the further dense operands.  Returns the sizes, pointers and leading dimensions."""
    import torch
    rows, cols, rowptr, colidx = A
    if not isinstance(rowptr, torch.Tensor) or not isinstance(colidx, torch.Tensor):
        raise SblasError("rowptr and colidx must be GPU tensors (no CPU path exists)")
    if rowptr.dtype != torch.int32 or colidx.dtype != torch.int32:
        raise SblasError("csr_attention handles float64 values and int32 indices only")
    if rowptr.dim() != 1 or rowptr.numel() != rows + 1 or colidx.dim() != 1:
        raise SblasError("rowptr has %d entries for %d rows" % (rowptr.numel(), rows))
    ldq = _attention_dense(Q, rows, None, "Q")
    d = int(Q.shape[1])
    ldk = _attention_dense(K, cols, d, "K")
    ldv = _attention_dense(V, cols, None, "V")
    dv = int(V.shape[1])
    lds = [_attention_dense(t, r, d if w == "d" else dv, what) for what, t, r, w in others]
    for what, t in [("rowptr", rowptr), ("colidx", colidx), ("Q", Q), ("K", K), ("V", V)] + [(o[0], o[1]) for o in others]:
        if not t.is_cuda:
            raise SblasError("%s must be a GPU tensor (no CPU path exists)" % what)
    nnz = int(colidx.numel())
    need = csr_attention_workspace_bytes(rows, nnz, d, dv)
    if workspace is None and need:
        workspace = torch.empty((need + 7) // 8, dtype=torch.float64, device=Q.device)
    if workspace is not None and not workspace.is_contiguous():
        raise SblasError("workspace must be contiguous")
    wptr = workspace.data_ptr() if workspace is not None and workspace.numel() else None
    wbytes = workspace.numel() * workspace.element_size() if workspace is not None else 0
    prow = _dev_ptr(rowptr, torch.int32, "rowptr")
    pcol = _dev_ptr(colidx, torch.int32, "colidx") if nnz else None
    return rows, cols, nnz, d, dv, prow, pcol, ldq, ldk, ldv, lds, wptr, wbytes, workspace


def _row_vector(t, rows, what):
    import torch
    if not isinstance(t, torch.Tensor):
        raise SblasError("%s must be a GPU tensor (no CPU path exists)" % what)
    if t.dim() != 1 or t.numel() != rows:
        raise SblasError("%s must hold one value per row (%d), got shape %s" % (what, rows, tuple(t.shape)))
    return _dev_ptr(t, torch.float64, what)


def csr_attention(A, Q, K, V, scale=1.0, out=None, row_max=None, row_sum=None, workspace=None, stream=None):
    """O = softmax(scale * Q K^T restricted to A's pattern) V in one pass, with no nnz-sized array: A = (rows, cols, rowptr,
    colidx) (int32, on the GPU), Q rows x d, K cols x d, V cols x dv, float64, row-major with any leading dimension
    (column slices work as they are), 1 <= d, dv <= 128.  out: rows x dv, row-major (None: a new tensor).  row_max,
    row_sum: both or neither, one float64 per row: the row's max of scale * s and its sum of exp(t - max), all the
    backward needs.  An empty row gives a +0 row, -Inf and +0.  workspace: None (allocated here when a row may exceed 4096
    entries) or a device tensor of at least csr_attention_workspace_bytes(rows, nnz, d, dv) bytes.  Returns out."""
    import torch
    rows = A[0]
    if out is None and isinstance(Q, torch.Tensor) and isinstance(V, torch.Tensor) and V.dim() == 2:
        out = torch.empty(rows, int(V.shape[1]), dtype=torch.float64, device=Q.device)
    if (row_max is None) != (row_sum is None):
        raise SblasError("row_max and row_sum come together: both or neither")
    (rows, cols, nnz, d, dv, prow, pcol, ldq, ldk, ldv, (ldo,), wptr, wbytes,
     _keep) = _attention_args(A, Q, K, V, [("out", out, rows, "dv")], workspace)
    pmax = _row_vector(row_max, rows, "row_max") if row_max is not None else None
    psum = _row_vector(row_sum, rows, "row_sum") if row_sum is not None else None
    check(lib().sblas_hip_csr_attention_f64_i32(-1, _stream(stream), rows, cols, nnz, prow, pcol, _view_ptr(Q, "Q"), ldq,
                                                _view_ptr(K, "K"), ldk, _view_ptr(V, "V"), ldv, d, dv, float(scale),
                                                _view_ptr(out, "out"), ldo, pmax, psum, wptr, wbytes),
          "sblas_hip_csr_attention_f64_i32")
    return out


def csr_attention_backward(A, Q, K, V, dO, row_max, row_sum, scale=1.0, dQ=None, P=None, dS=None, workspace=None, stream=None):
    """The backward of csr_attention from its inputs, the gradient dO (rows x dv) of its output and the row_max / row_sum it
    wrote.  Each of dQ (rows x d, row-major), P and dS (nnz float64 each) is written when given and costs nothing when
    None: P alone forms no <dO, V>.  P[e] is the attention probability of entry e, dS[e] the gradient of the score
    <Q[i], K[c(e)]>; the caller forms dV = A(P)^T dO and dK = A(dS)^T Q with a TransposePlan.  P and dS are, bit for bit,
    csr_softmax(sddmm(Q, K), scale) and csr_softmax_backward(P, sddmm(dO, V), scale).  Returns (dQ, P, dS)."""
    import torch
    rows = A[0]
    if isinstance(A[3], torch.Tensor):                   # shapes first: they are wrong on any device
        for what, t in (("P", P), ("dS", dS)):
            if t is not None and (not isinstance(t, torch.Tensor) or t.dim() != 1 or t.numel() != A[3].numel()):
                raise SblasError("%s must hold one value per stored entry (%d)" % (what, A[3].numel()))
    others = []
    if dQ is not None or dS is not None:
        others.append(("dO", dO, rows, "dv"))
    if dQ is not None:
        others.append(("dQ", dQ, rows, "d"))
    (rows, cols, nnz, d, dv, prow, pcol, ldq, ldk, ldv, lds, wptr, wbytes,
     _keep) = _attention_args(A, Q, K, V, others, workspace)
    lddo = lds[0] if others else dv
    lddq = lds[-1] if dQ is not None else d
    pp = _dev_ptr(P, torch.float64, "P") if P is not None and nnz else None
    pds = _dev_ptr(dS, torch.float64, "dS") if dS is not None and nnz else None
    check(lib().sblas_hip_csr_attention_backward_f64_i32(
        -1, _stream(stream), rows, cols, nnz, prow, pcol, _view_ptr(Q, "Q"), ldq, _view_ptr(K, "K"), ldk, _view_ptr(V, "V"), ldv,
        d, dv, float(scale), _view_ptr(dO, "dO") if others else None, lddo, _row_vector(row_max, rows, "row_max"),
        _row_vector(row_sum, rows, "row_sum"), _view_ptr(dQ, "dQ") if dQ is not None else None, lddq, pp, pds, wptr, wbytes),
        "sblas_hip_csr_attention_backward_f64_i32")
    return dQ, P, dS
