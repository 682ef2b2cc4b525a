"""Host-side mirror of the reference interface over the C ABI of libchebhip.so.

The product is the C-ABI shared library (include/chebhip.h); this module is the
thin ctypes binding the tests and bench.py use, shaped after the reference's
operator interface:

  ChebPlan(dims, tr).mult(x, y)        <-> MatCreateCheb / ChebMult / ChebDestroy
                                           (chebyshev.h:31-34, chebyshev.c:89-235)
  EllipticOp(dims).mult(U, V)          <-> MatCreate_Elliptic / MatMult_Elliptic
                                           (elliptic.C:250-339)
  EllipticOp.function(U, b, rhs, ...)  <-> FormFunction (elliptic.C:481-533)

Device vectors are torch.float64 CUDA(HIP) tensors; torch is used only for
device memory and streams.  There is no CPU fallback: if libchebhip.so is
missing or no GPU is usable, construction raises.

The directory name carries a hyphen, so import it with `load()` from
__graft_entry__.py (importlib by path) rather than `import`.
"""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
# CHEBHIP_LIB_PATH: a diagnostic build of the same library (`make -C csrc diag`, or the parent commit's build for an A/B); production uses the in-tree one
LIB_PATH = os.environ.get("CHEBHIP_LIB_PATH") or os.path.join(_HERE, "libchebhip.so")
INCLUDE_DIR = os.path.join(os.path.dirname(_HERE), "include")

# every symbol include/chebhip.h declares (checked by tests/test_abi.py)
ABI_SYMBOLS = [
    "chebhip_last_error", "chebhip_version", "chebhip_arch", "chebhip_launch_count", "chebhip_vec_launch_count",
    "chebhip_set_option", "chebhip_get_option", "chebhip_option_name",
    "cheb_plan_create", "cheb_apply", "cheb_apply_host", "cheb_plan_destroy", "cheb_plan_size",
    "cheb_plan_create_trimmed", "cheb_apply_lap1d", "cheb_slab_pack", "cheb_slab_unpack_add",
    "ell_op_create", "ell_op_destroy", "ell_op_local_size", "ell_op_global_size",
    "ell_op_dirichlet_size", "ell_op_mult", "ell_op_mult_host", "ell_op_function",
    "ell_op_function_host", "ell_op_set_dirichlet", "ell_op_get_state", "ell_op_set_state",
    "ell_op_create_slab", "ell_op_pencil_sweep",
    "stokes_op_create", "stokes_op_destroy", "stokes_op_size", "stokes_op_set_rheology",
    "stokes_op_set_dirichlet", "stokes_op_set_force", "stokes_op_mult", "stokes_op_mult_vv",
    "stokes_op_mult_pv", "stokes_op_mult_vp", "stokes_op_mult_vv_cm", "stokes_op_mult_pv_cm", "stokes_op_mult_vp_cm", "stokes_op_mult_schur_cm", "stokes_op_function", "stokes_op_get_state",
    "stokes_op_set_state", "stokes_op_create_slab", "stokes_op_pencil_sweep", "stokes_op_pencil_pressure", "stokes_op_pencil_sweep_pressure", "stokes_op_mult_schur", "stokes_op_set_inner_solver", "stokes_op_inner_iterations", "stokes_op_set_inner_reduce",
    "chebhip_fgmres_create", "chebhip_fgmres_destroy", "chebhip_fgmres_set_tolerances", "chebhip_fgmres_solve",
    "chebhip_fgmres_iterations", "chebhip_fgmres_residual", "chebhip_fgmres_reason", "chebhip_fgmres_set_reduce",
    "ell_pc_create", "stokes_pc_create", "chebhip_fdpc_destroy", "chebhip_fdpc_update", "chebhip_fdpc_set_sweeps",
    "chebhip_fdpc_mult", "chebhip_fdpc_apply", "chebhip_fdpc_apply_cm",
    "chebhip_fdpc_step", "chebhip_fdpc_step_route", "chebhip_fdpc_line_host", "cheb_helmholtz_fdpc",
    "stokes_saddle_create", "stokes_saddle_destroy", "stokes_saddle_set_type", "stokes_saddle_set_inner",
    "stokes_saddle_setup", "stokes_saddle_apply", "stokes_saddle_iterations", "stokes_saddle_set_pc_sweeps", "stokes_saddle_set_schur_jacobi",
    "chebhip_timers_enable", "chebhip_timers_reset", "chebhip_timers_read", "chebhip_stage_name",
    "stokes_op_viscosity_range", "stokes_op_write_vtk",
    "chebhip_dist_create", "chebhip_dist_destroy", "chebhip_dist_local_size", "chebhip_dist_slab_offset",
    "chebhip_dist_use_rccl", "chebhip_dist_set_exchange", "chebhip_dist_mult", "chebhip_dist_mult_batch",
    "chebhip_rccl_unique_id", "chebhip_rccl_comm_create", "chebhip_rccl_comm_destroy", "chebhip_rccl_reduce",
    "chebhip_comm_create_rccl", "chebhip_local_group_create", "chebhip_local_group_destroy", "chebhip_local_group_abort",
    "chebhip_comm_create_local", "chebhip_comm_create_callback", "chebhip_comm_create_null", "chebhip_comm_null_set_shadow", "chebhip_comm_destroy", "chebhip_comm_size", "chebhip_comm_rank",
    "chebhip_ipc_group_open", "chebhip_ipc_group_close", "chebhip_ipc_group_abort", "chebhip_comm_create_ipc",
    "chebhip_comm_reduce", "chebhip_dist_use_comm",
    "chebhip_dist_stokes_create", "chebhip_dist_stokes_destroy", "chebhip_dist_stokes_op", "chebhip_dist_stokes_ranges",
    "chebhip_dist_ell_create", "chebhip_dist_ell_destroy", "chebhip_dist_ell_op", "chebhip_dist_ell_ranges",
    "stokes_pc_create_slab", "ell_pc_create_slab", "chebhip_fdpc_pencil_transform", "chebhip_dist_stokes_pc", "chebhip_dist_ell_pc",
    "stokes_saddle_create_slab",
    "cheb_resample_create", "cheb_resample_apply", "cheb_resample_destroy", "cheb_resample_size", "cheb_resample_matrix_host",
    "cheb_helmholtz_create", "cheb_helmholtz_solve", "cheb_helmholtz_apply", "cheb_helmholtz_destroy", "cheb_helmholtz_size",
    "cheb_helmholtz_line_host", "ell_pc_create_spectral",
    "cheb_helmholtz_create_bc", "cheb_helmholtz_solve_bc", "cheb_helmholtz_full_size", "cheb_helmholtz_boundary_size",
    "cheb_helmholtz_singular", "cheb_helmholtz_line_bc_host",
    "cheb_modal_create", "cheb_modal_destroy", "cheb_modal_size", "cheb_modal_spectrum_size", "cheb_modal_forward", "cheb_modal_backward",
    "cheb_modal_set_filter", "cheb_modal_filter", "cheb_modal_spectrum", "cheb_modal_integrate",
    "cheb_modal_matrix_host", "cheb_modal_weights_host", "cheb_modal_filter_matrix_host",
    "cheb_points_create", "cheb_points_destroy", "cheb_points_chunk", "cheb_points_rows", "cheb_points_eval",
    "cheb_points_spread", "cheb_points_spread_pass",
    "cheb_points_grid_reserve", "cheb_points_eval_grid", "cheb_nodes_host", "cheb_points_matrix_host",
    "cheb_points_drows", "cheb_points_dmatrix_host", "cheb_points_eval_deriv", "cheb_points_spread_deriv",
    "cheb_points_eval_grid_deriv", "cheb_points_eval_grad",
    "cheb_dealias_fine_size", "cheb_dealias_matrix_host", "cheb_dealias_create", "cheb_dealias_destroy", "cheb_dealias_fine_dims",
    "cheb_dealias_size", "cheb_dealias_work_bytes", "cheb_dealias_multiply", "cheb_dealias_reserve_advect", "cheb_dealias_advect",
    "cheb_reduce_weights_host", "cheb_reduce_create", "cheb_reduce_destroy", "cheb_reduce_set_weights", "cheb_reduce_size",
    "cheb_reduce_slices", "cheb_reduce_apply",
    "cheb_stats_spacing_host", "cheb_stats_rate_host", "cheb_stats_check", "cheb_stats_create", "cheb_stats_destroy",
    "cheb_stats_set_weights", "cheb_stats_size", "cheb_stats_summary", "cheb_stats_histogram", "cheb_stats_cfl",
    "cheb_grad_create", "cheb_grad_destroy", "cheb_grad_size", "cheb_grad_work_size", "cheb_grad_grad", "cheb_grad_tensor",
    "cheb_grad_div", "cheb_grad_curl", "cheb_grad_strain", "cheb_grad_laplacian", "cheb_grad_invariants",
    "cheb_layout_create", "cheb_layout_destroy", "cheb_layout_size", "cheb_layout_map_host", "cheb_layout_unpack", "cheb_layout_pack",
    "cheb_helmholtz_create_box", "cheb_helmholtz_line_box_host",
    "cheb_fourier_nodes_host", "cheb_fourier_diff_matrix_host", "cheb_fourier_modes_host", "cheb_fourier_modal_matrix_host",
    "cheb_fourier_line_host", "cheb_grad_create_basis", "cheb_modal_create_basis", "cheb_helmholtz_create_basis",
    "cheb_project_create", "cheb_project_destroy", "cheb_project_size", "cheb_project_singular", "cheb_project_faces_host",
    "cheb_project_apply",
    "cheb_opfun_create", "cheb_opfun_destroy", "cheb_opfun_set_terms", "cheb_opfun_apply", "cheb_opfun_apply_full", "cheb_opfun_size",
    "cheb_opfun_singular", "cheb_opfun_check_terms", "cheb_opfun_weight_host", "cheb_opfun_weights_host", "cheb_opfun_eval",
    "cheb_dealias_create_basis", "cheb_dealias_fine_size_basis", "cheb_dealias_matrix_basis_host",
    "cheb_project_create_basis", "cheb_project_faces_basis_host", "cheb_opfun_create_basis",
    "cheb_points_create_basis", "cheb_points_fourier_matrix_host",
    "cheb_varhelm_create", "cheb_varhelm_destroy", "cheb_varhelm_size", "cheb_varhelm_full_size", "cheb_varhelm_boundary_size",
    "cheb_varhelm_work_bytes", "cheb_varhelm_set_coefficients", "cheb_varhelm_sigma", "cheb_varhelm_singular", "cheb_varhelm_mult",
    "cheb_varhelm_apply", "cheb_varhelm_residual", "cheb_varhelm_precond", "cheb_varhelm_solve", "cheb_varhelm_iterations",
    "cheb_varhelm_last_residual", "cheb_varhelm_reason",
    "cheb_varhelm_solve_deflated", "cheb_varhelm_null_count", "cheb_varhelm_defect", "cheb_varhelm_null_signs_host",
    "cheb_varhelm_remove_null", "cheb_varhelm_apply_deflated", "cheb_varhelm_precond_deflated",
    "cheb_varhelm_set_tensor", "cheb_varhelm_mode",
    "cheb_project_create_variable", "cheb_project_set_inverse_density", "cheb_project_apply_variable", "cheb_project_varhelm",
]


class OpFunTerm(C.Structure):
    """cheb_opfun_term"""
    _fields_ = [("out", C.c_int), ("inp", C.c_int), ("kind", C.c_int), ("coef", C.c_double), ("tau", C.c_double), ("par", C.c_double)]


class ChebhipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("chebhip error %d: %s" % (code, msg))
        self.code = code


def build(force=False):
    """Compile libchebhip.so for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    src = os.path.join(_HERE, "csrc")
    if force:
        subprocess.check_call(["make", "-C", src, "-s", "clean"])
    subprocess.check_call(["make", "-C", src, "-s"])
    return LIB_PATH


_lib = None


def lib():
    """Load the C-ABI library; fails loudly if the HIP extension has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ChebhipError(-1, "libchebhip.so not built (run __graft_entry__.build()); there is no CPU fallback")
        L = C.CDLL(LIB_PATH)
        dp, ip, vp = C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_void_p
        L.chebhip_last_error.restype = C.c_char_p
        L.chebhip_arch.restype = C.c_char_p
        L.chebhip_launch_count.restype = C.c_long
        L.chebhip_vec_launch_count.restype = C.c_long
        L.chebhip_set_option.argtypes = [C.c_char_p, C.c_int]
        L.chebhip_get_option.argtypes = [C.c_char_p, C.POINTER(C.c_int)]
        L.chebhip_option_name.argtypes = [C.c_int]
        L.chebhip_option_name.restype = C.c_char_p
        L.cheb_plan_create.argtypes = [C.c_int, C.c_int, ip, C.POINTER(vp)]
        L.cheb_apply.argtypes = [vp, vp, vp, vp]
        L.cheb_plan_create_trimmed.argtypes = [C.c_int, C.c_int, ip, C.POINTER(vp)]
        L.cheb_apply_lap1d.argtypes = [vp, vp, vp, C.c_double, vp, vp]
        lp = C.POINTER(C.c_long)
        L.cheb_slab_pack.argtypes = [C.c_long, C.c_long, C.c_long, C.c_int, lp, vp, vp, vp]
        L.cheb_slab_unpack_add.argtypes = [C.c_long, C.c_long, C.c_long, C.c_int, lp, vp, vp, C.c_double, vp, vp]
        L.cheb_apply_host.argtypes = [vp, dp, dp]
        L.cheb_plan_destroy.argtypes = [vp]
        L.cheb_plan_size.argtypes = [vp]
        L.cheb_plan_size.restype = C.c_long
        L.ell_op_create.argtypes = [C.c_int, ip, C.POINTER(vp)]
        L.ell_op_destroy.argtypes = [vp]
        L.ell_op_create_slab.argtypes = [C.c_int, ip, C.c_int, C.c_int, vp, vp, C.POINTER(vp)]
        L.ell_op_pencil_sweep.argtypes = [vp, C.c_long, vp, vp, vp]
        for f in (L.ell_op_local_size, L.ell_op_global_size, L.ell_op_dirichlet_size):
            f.argtypes = [vp]
            f.restype = C.c_long
        L.ell_op_mult.argtypes = [vp, vp, vp, vp]
        L.ell_op_mult_host.argtypes = [vp, dp, dp]
        L.ell_op_function.argtypes = [vp, C.c_double, C.c_double, vp, vp, vp, vp]
        L.ell_op_function_host.argtypes = [vp, C.c_double, C.c_double, dp, dp, dp]
        L.ell_op_set_dirichlet.argtypes = [vp, dp]
        L.ell_op_get_state.argtypes = [vp, C.c_int, dp]
        L.ell_op_set_state.argtypes = [vp, C.c_int, dp]
        L.stokes_op_create.argtypes = [C.c_int, ip, C.POINTER(vp)]
        L.stokes_op_destroy.argtypes = [vp]
        L.stokes_op_size.argtypes = [vp, C.c_int]
        L.stokes_op_size.restype = C.c_long
        L.stokes_op_set_rheology.argtypes = [vp, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double]
        L.stokes_op_set_dirichlet.argtypes = [vp, dp]
        L.stokes_op_set_force.argtypes = [vp, dp]
        for f in (L.stokes_op_mult, L.stokes_op_mult_vv, L.stokes_op_mult_pv, L.stokes_op_mult_vp, L.stokes_op_function,
                  L.stokes_op_mult_vv_cm, L.stokes_op_mult_pv_cm, L.stokes_op_mult_vp_cm):
            f.argtypes = [vp, vp, vp, vp]
        L.stokes_op_mult_schur_cm.argtypes = [vp, vp, vp, vp, vp, vp]
        L.stokes_op_get_state.argtypes = [vp, C.c_int, dp]
        L.stokes_op_set_state.argtypes = [vp, C.c_int, dp]
        L.stokes_op_create_slab.argtypes = [C.c_int, ip, C.c_int, C.c_int, vp, vp, C.POINTER(vp)]
        L.stokes_op_pencil_sweep.argtypes = [vp, C.c_int, C.c_long, vp, vp, vp]
        L.stokes_op_pencil_pressure.argtypes = [vp, C.c_long, vp, vp, vp]
        L.stokes_op_mult_schur.argtypes = [vp, vp, vp, vp, vp, vp]
        L.stokes_op_set_inner_solver.argtypes = [vp, C.c_int, C.c_double, C.c_double, C.c_int]
        L.stokes_op_inner_iterations.argtypes = [vp]
        L.stokes_op_set_inner_reduce.argtypes = [vp, vp, vp]
        L.chebhip_fgmres_create.argtypes = [C.c_long, C.c_int, C.POINTER(vp)]
        L.chebhip_fgmres_destroy.argtypes = [vp]
        L.chebhip_fgmres_set_tolerances.argtypes = [vp, C.c_double, C.c_double, C.c_int]
        L.chebhip_fgmres_solve.argtypes = [vp, vp, vp, vp, vp, vp, vp, C.c_int, vp]
        L.chebhip_fgmres_iterations.argtypes = [vp]
        L.chebhip_fgmres_residual.argtypes = [vp]
        L.chebhip_fgmres_residual.restype = C.c_double
        L.chebhip_fgmres_reason.argtypes = [vp]
        L.chebhip_fgmres_set_reduce.argtypes = [vp, vp, vp]
        L.ell_pc_create.argtypes = [vp, C.POINTER(vp)]
        L.stokes_pc_create.argtypes = [vp, C.POINTER(vp)]
        L.chebhip_fdpc_destroy.argtypes = [vp]
        L.chebhip_fdpc_update.argtypes = [vp, vp]
        L.chebhip_fdpc_set_sweeps.argtypes = [vp, C.c_int]
        L.chebhip_fdpc_mult.argtypes = [vp, vp, vp, vp]
        L.chebhip_fdpc_apply.argtypes = [vp, vp, vp, vp]
        L.chebhip_fdpc_apply_cm.argtypes = [vp, vp, vp, vp]
        L.stokes_saddle_create.argtypes = [vp, C.POINTER(vp)]
        L.stokes_saddle_destroy.argtypes = [vp]
        L.stokes_saddle_set_type.argtypes = [vp, C.c_int]
        L.stokes_saddle_set_inner.argtypes = [vp, C.c_int, C.c_int, C.c_double]
        L.stokes_saddle_setup.argtypes = [vp, vp]
        L.stokes_saddle_apply.argtypes = [vp, vp, vp, vp]
        L.stokes_saddle_iterations.argtypes = [vp, C.c_int]
        L.stokes_saddle_set_pc_sweeps.argtypes = [vp, C.c_int]
        L.stokes_saddle_set_schur_jacobi.argtypes = [vp, C.c_int]
        L.chebhip_timers_enable.argtypes = [C.c_int]
        L.chebhip_timers_read.argtypes = [C.c_int, dp, C.POINTER(C.c_long)]
        L.chebhip_stage_name.argtypes = [C.c_int]
        L.chebhip_stage_name.restype = C.c_char_p
        L.stokes_op_viscosity_range.argtypes = [vp, dp, dp, vp]
        L.stokes_op_write_vtk.argtypes = [vp, vp, C.c_char_p]
        L.chebhip_dist_create.argtypes = [C.c_int, ip, C.c_int, C.c_int, C.POINTER(vp)]
        L.chebhip_dist_destroy.argtypes = [vp]
        for f in (L.chebhip_dist_local_size, L.chebhip_dist_slab_offset):
            f.argtypes = [vp]
            f.restype = C.c_long
        L.chebhip_dist_use_rccl.argtypes = [vp, vp]
        L.chebhip_dist_set_exchange.argtypes = [vp, vp, vp]
        L.chebhip_dist_mult.argtypes = [vp, vp, vp, vp]
        L.chebhip_dist_mult_batch.argtypes = [vp, C.c_int, vp, vp, vp]
        L.chebhip_rccl_unique_id.argtypes = [vp]
        L.chebhip_rccl_comm_create.argtypes = [C.c_int, C.c_int, vp, C.POINTER(vp)]
        L.chebhip_rccl_comm_destroy.argtypes = [vp]
        L.chebhip_rccl_reduce.argtypes = [vp, vp, C.c_int, vp]
        L.chebhip_comm_create_rccl.argtypes = [vp, C.c_int, C.c_int, C.POINTER(vp)]
        L.chebhip_local_group_create.argtypes = [C.c_int, C.POINTER(vp)]
        L.chebhip_local_group_destroy.argtypes = [vp]
        L.chebhip_local_group_abort.argtypes = [vp]
        L.chebhip_comm_create_local.argtypes = [vp, C.c_int, C.POINTER(vp)]
        L.chebhip_comm_create_callback.argtypes = [C.c_int, C.c_int, vp, vp, vp, C.POINTER(vp)]
        L.chebhip_comm_destroy.argtypes = [vp]
        L.chebhip_comm_create_null.argtypes = [C.c_int, C.c_int, C.POINTER(vp)]
        L.chebhip_comm_null_set_shadow.argtypes = [vp, C.c_int, C.POINTER(vp)]
        L.chebhip_ipc_group_open.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(vp)]
        L.chebhip_ipc_group_close.argtypes = [vp]
        L.chebhip_ipc_group_abort.argtypes = [vp]
        L.chebhip_comm_create_ipc.argtypes = [vp, vp, C.POINTER(vp)]
        L.chebhip_comm_size.argtypes = [vp]
        L.chebhip_comm_rank.argtypes = [vp]
        L.chebhip_comm_reduce.argtypes = [vp, vp, C.c_int, vp]
        L.chebhip_dist_use_comm.argtypes = [vp, vp]
        for nm in ("stokes", "ell"):
            getattr(L, "chebhip_dist_%s_create" % nm).argtypes = [C.c_int, ip, vp, C.POINTER(vp)]
            getattr(L, "chebhip_dist_%s_destroy" % nm).argtypes = [vp]
            getattr(L, "chebhip_dist_%s_op" % nm).argtypes = [vp]
            getattr(L, "chebhip_dist_%s_op" % nm).restype = vp
            getattr(L, "chebhip_dist_%s_ranges" % nm).argtypes = [vp, lp]
            getattr(L, "chebhip_dist_%s_pc" % nm).argtypes = [vp, C.POINTER(vp)]
            getattr(L, "%s_pc_create_slab" % nm).argtypes = [vp, C.c_long, vp, vp, C.POINTER(vp)]
        L.chebhip_fdpc_pencil_transform.argtypes = [vp, C.c_int, C.c_int, C.c_long, vp, vp, vp]
        L.stokes_saddle_create_slab.argtypes = [vp, vp, vp, vp, C.POINTER(vp)]
        L.cheb_resample_create.argtypes = [C.c_int, ip, C.c_int, ip, C.c_int, C.c_int, C.POINTER(vp)]
        L.cheb_resample_apply.argtypes = [vp, vp, vp, vp]
        L.cheb_resample_destroy.argtypes = [vp]
        L.cheb_resample_size.argtypes = [vp, C.c_int]
        L.cheb_resample_size.restype = C.c_long
        L.cheb_resample_matrix_host.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, dp]
        L.cheb_helmholtz_create.argtypes = [C.c_int, ip, C.c_double, C.c_int, C.POINTER(vp)]
        for f in (L.cheb_helmholtz_solve, L.cheb_helmholtz_apply):
            f.argtypes = [vp, vp, vp, vp]
        L.cheb_helmholtz_destroy.argtypes = [vp]
        L.cheb_helmholtz_size.argtypes = [vp]
        L.cheb_helmholtz_size.restype = C.c_long
        L.cheb_helmholtz_line_host.argtypes = [C.c_int, dp, dp, dp]
        L.chebhip_fdpc_line_host.argtypes = [C.c_int, dp, dp, dp]
        L.chebhip_fdpc_step.argtypes = [vp, C.c_int, C.c_int, vp, vp, vp]
        L.chebhip_fdpc_step_route.argtypes = [vp, C.c_int, C.c_int]
        L.cheb_helmholtz_fdpc.argtypes = [vp]
        L.cheb_helmholtz_fdpc.restype = vp
        L.ell_pc_create_spectral.argtypes = [vp, C.c_double, C.POINTER(vp)]
        L.cheb_helmholtz_create_bc.argtypes = [C.c_int, ip, dp, C.c_double, C.c_int, C.POINTER(vp)]
        L.cheb_helmholtz_solve_bc.argtypes = [vp, vp, vp, vp, vp]
        for f in (L.cheb_helmholtz_full_size, L.cheb_helmholtz_boundary_size):
            f.argtypes = [vp]
            f.restype = C.c_long
        L.cheb_helmholtz_singular.argtypes = [vp]
        L.cheb_helmholtz_line_bc_host.argtypes = [C.c_int, dp, dp, dp, dp, dp, dp, dp]
        L.cheb_modal_create.argtypes = [C.c_int, ip, C.c_int, C.POINTER(vp)]
        L.cheb_modal_destroy.argtypes = [vp]
        for f in (L.cheb_modal_size, L.cheb_modal_spectrum_size):
            f.argtypes = [vp]
            f.restype = C.c_long
        for f in (L.cheb_modal_forward, L.cheb_modal_backward, L.cheb_modal_filter, L.cheb_modal_spectrum):
            f.argtypes = [vp, vp, vp, vp]
        L.cheb_modal_set_filter.argtypes = [vp, C.c_int, dp]
        L.cheb_modal_integrate.argtypes = [vp, vp, vp, vp, vp]
        L.cheb_modal_matrix_host.argtypes = [C.c_int, C.c_int, dp]
        L.cheb_modal_weights_host.argtypes = [C.c_int, dp]
        L.cheb_modal_filter_matrix_host.argtypes = [C.c_int, dp, dp]
        L.cheb_points_create.argtypes = [C.c_int, ip, C.c_int, C.POINTER(vp)]
        L.cheb_points_destroy.argtypes = [vp]
        L.cheb_points_chunk.argtypes = [vp]
        L.cheb_points_chunk.restype = C.c_long
        L.cheb_points_rows.argtypes = [vp, C.c_int, vp, C.c_long, vp, vp]
        L.cheb_points_eval.argtypes = [vp, vp, vp, C.c_long, vp, vp]
        L.cheb_points_spread.argtypes = [vp, vp, vp, C.c_long, vp, C.c_int, vp]
        L.cheb_points_spread_pass.argtypes = [vp]
        L.cheb_points_spread_pass.restype = C.c_long
        L.cheb_points_grid_reserve.argtypes = [vp, ip]
        L.cheb_points_eval_grid.argtypes = [vp, vp, vp, ip, vp, vp]
        L.cheb_nodes_host.argtypes = [C.c_int, dp]
        L.cheb_points_matrix_host.argtypes = [C.c_int, C.c_int, dp, dp]
        L.cheb_points_drows.argtypes = [vp, C.c_int, vp, C.c_long, vp, vp]
        L.cheb_points_dmatrix_host.argtypes = [C.c_int, C.c_int, dp, dp]
        L.cheb_points_eval_deriv.argtypes = [vp, vp, vp, C.c_long, ip, vp, vp]
        L.cheb_points_spread_deriv.argtypes = [vp, vp, vp, C.c_long, ip, vp, C.c_int, vp]
        L.cheb_points_eval_grid_deriv.argtypes = [vp, vp, vp, ip, ip, vp, vp]
        L.cheb_points_eval_grad.argtypes = [vp, vp, vp, C.c_long, dp, C.c_int, vp, vp]
        L.cheb_dealias_fine_size.argtypes = [C.c_int]
        L.cheb_dealias_matrix_host.argtypes = [C.c_int, C.c_int, C.c_int, dp]
        L.cheb_dealias_create.argtypes = [C.c_int, ip, ip, C.c_int, C.POINTER(vp)]
        L.cheb_dealias_destroy.argtypes = [vp]
        L.cheb_dealias_fine_dims.argtypes = [vp, ip]
        for f in (L.cheb_dealias_size, L.cheb_dealias_work_bytes):
            f.argtypes = [vp]
            f.restype = C.c_long
        L.cheb_dealias_reserve_advect.argtypes = [vp]
        for f in (L.cheb_dealias_multiply, L.cheb_dealias_advect):
            f.argtypes = [vp, vp, vp, vp, vp]
        L.cheb_reduce_weights_host.argtypes = [C.c_int, C.c_int, C.c_double, dp]
        L.cheb_reduce_create.argtypes = [C.c_int, ip, C.c_int, ip, C.POINTER(vp)]
        L.cheb_reduce_destroy.argtypes = [vp]
        L.cheb_reduce_set_weights.argtypes = [vp, C.c_int, dp]
        L.cheb_reduce_size.argtypes = [vp, C.c_int]
        L.cheb_reduce_size.restype = C.c_long
        L.cheb_reduce_slices.argtypes = [vp]
        L.cheb_reduce_apply.argtypes = [vp, vp, vp, vp, vp]
        L.cheb_stats_spacing_host.argtypes = [C.c_int, dp]
        L.cheb_stats_rate_host.argtypes = [C.c_int, C.c_double, dp]
        L.cheb_stats_check.argtypes = [C.c_int, ip, C.c_int, C.c_int, C.c_int]
        L.cheb_stats_create.argtypes = [C.c_int, ip, C.c_int, C.c_int, C.POINTER(vp)]
        L.cheb_stats_destroy.argtypes = [vp]
        L.cheb_stats_set_weights.argtypes = [vp, C.c_int, dp]
        L.cheb_stats_size.argtypes = [vp, C.c_int]
        L.cheb_stats_size.restype = C.c_long
        L.cheb_stats_summary.argtypes = [vp, vp, vp, vp, vp]
        L.cheb_stats_histogram.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, vp, vp]
        L.cheb_stats_cfl.argtypes = [vp, vp, dp, vp, vp]
        L.cheb_grad_create.argtypes = [C.c_int, ip, dp, C.POINTER(vp)]
        L.cheb_grad_destroy.argtypes = [vp]
        L.cheb_grad_size.argtypes = [vp]
        L.cheb_grad_size.restype = C.c_long
        L.cheb_grad_work_size.argtypes = [vp, C.c_int]
        L.cheb_grad_work_size.restype = C.c_long
        for f in (L.cheb_grad_grad, L.cheb_grad_tensor, L.cheb_grad_div, L.cheb_grad_curl, L.cheb_grad_strain):
            f.argtypes = [vp, C.c_int, vp, vp, vp]
        L.cheb_grad_laplacian.argtypes = [vp, C.c_int, vp, vp, vp, vp]
        L.cheb_grad_invariants.argtypes = [vp, C.c_int, vp, C.c_uint, vp, vp]
        L.cheb_layout_create.argtypes = [C.c_int, ip, C.POINTER(vp)]
        L.cheb_layout_destroy.argtypes = [vp]
        L.cheb_layout_size.argtypes = [vp, C.c_int]
        L.cheb_layout_size.restype = C.c_long
        L.cheb_layout_map_host.argtypes = [C.c_int, ip, ip]
        L.cheb_layout_unpack.argtypes = [vp, C.c_int, vp, C.c_long, C.c_long, vp, C.c_long, C.c_long, vp, vp]
        L.cheb_layout_pack.argtypes = [vp, C.c_int, vp, vp, C.c_long, C.c_long, vp, C.c_long, C.c_long, vp]
        L.cheb_helmholtz_create_box.argtypes = [C.c_int, ip, dp, dp, C.c_double, C.c_int, C.POINTER(vp)]
        L.cheb_helmholtz_line_box_host.argtypes = [C.c_int, dp, C.c_double, dp, dp, dp, dp, dp, dp]
        L.cheb_fourier_nodes_host.argtypes = [C.c_int, dp]
        L.cheb_fourier_diff_matrix_host.argtypes = [C.c_int, C.c_int, dp]
        L.cheb_fourier_modes_host.argtypes = [C.c_int, ip, ip]
        L.cheb_fourier_modal_matrix_host.argtypes = [C.c_int, C.c_int, dp]
        L.cheb_fourier_line_host.argtypes = [C.c_int, C.c_double, dp, dp, dp]
        L.cheb_grad_create_basis.argtypes = [C.c_int, ip, dp, ip, C.POINTER(vp)]
        L.cheb_modal_create_basis.argtypes = [C.c_int, ip, C.c_int, ip, C.POINTER(vp)]
        L.cheb_helmholtz_create_basis.argtypes = [C.c_int, ip, ip, dp, dp, C.c_double, C.c_int, C.POINTER(vp)]
        L.cheb_project_create.argtypes = [C.c_int, ip, ip, dp, C.c_int, C.POINTER(vp)]
        L.cheb_project_destroy.argtypes = [vp]
        L.cheb_project_size.argtypes = [vp, C.c_int]
        L.cheb_project_size.restype = C.c_long
        L.cheb_project_singular.argtypes = [vp]
        L.cheb_project_faces_host.argtypes = [C.c_int, ip, ip]
        L.cheb_project_apply.argtypes = [vp, vp, vp, vp, vp, vp]
        L.cheb_opfun_create.argtypes = [C.c_int, ip, dp, dp, C.c_double, C.c_int, C.c_int, C.POINTER(vp)]
        L.cheb_opfun_destroy.argtypes = [vp]
        L.cheb_opfun_set_terms.argtypes = [vp, C.c_int, C.POINTER(OpFunTerm)]
        L.cheb_opfun_check_terms.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(OpFunTerm)]
        L.cheb_opfun_apply.argtypes = [vp, vp, vp, vp]
        L.cheb_opfun_apply_full.argtypes = [vp, vp, vp, vp]
        L.cheb_opfun_size.argtypes = [vp, C.c_int]
        L.cheb_opfun_size.restype = C.c_long
        L.cheb_opfun_singular.argtypes = [vp]
        L.cheb_opfun_weight_host.argtypes = [C.c_int, C.c_double, C.c_double, C.c_double, dp]
        L.cheb_opfun_weights_host.argtypes = [C.c_int, C.c_double, C.c_double, C.c_long, dp, dp]
        L.cheb_opfun_eval.argtypes = [C.c_int, C.c_double, C.c_double, vp, C.c_long, vp, vp]
        L.cheb_dealias_create_basis.argtypes = [C.c_int, ip, ip, ip, C.c_int, C.POINTER(vp)]
        L.cheb_dealias_fine_size_basis.argtypes = [C.c_int, C.c_int]
        L.cheb_dealias_matrix_basis_host.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, dp]
        L.cheb_project_create_basis.argtypes = [C.c_int, ip, ip, ip, dp, C.c_int, C.POINTER(vp)]
        L.cheb_project_faces_basis_host.argtypes = [C.c_int, ip, ip, ip]
        L.cheb_opfun_create_basis.argtypes = [C.c_int, ip, ip, dp, dp, C.c_double, C.c_int, C.c_int, C.POINTER(vp)]
        L.cheb_points_create_basis.argtypes = [C.c_int, ip, C.c_int, ip, C.POINTER(vp)]
        L.cheb_points_fourier_matrix_host.argtypes = [C.c_int, C.c_int, dp, C.c_int, dp]
        L.cheb_varhelm_create.argtypes = [C.c_int, ip, ip, dp, dp, C.c_int, C.POINTER(vp)]
        L.cheb_varhelm_destroy.argtypes = [vp]
        for f in (L.cheb_varhelm_size, L.cheb_varhelm_full_size, L.cheb_varhelm_boundary_size, L.cheb_varhelm_work_bytes):
            f.argtypes = [vp]
            f.restype = C.c_long
        L.cheb_varhelm_set_coefficients.argtypes = [vp, vp, vp, C.c_double, vp]
        L.cheb_varhelm_set_tensor.argtypes = [vp, vp, vp, vp, C.c_double, vp]
        L.cheb_varhelm_mode.argtypes = [vp]
        L.cheb_varhelm_sigma.argtypes = [vp]
        L.cheb_varhelm_sigma.restype = C.c_double
        L.cheb_varhelm_singular.argtypes = [vp]
        L.cheb_varhelm_mult.argtypes = [vp, vp, vp, vp]
        L.cheb_varhelm_apply.argtypes = [vp, vp, vp, vp]
        L.cheb_varhelm_residual.argtypes = [vp, vp, vp, vp, vp, vp]
        L.cheb_varhelm_precond.argtypes = [vp, vp, vp, vp]
        L.cheb_varhelm_solve.argtypes = [vp, vp, vp, vp, C.c_int, vp, C.c_double, C.c_double, C.c_int, C.c_int, vp]
        L.cheb_varhelm_iterations.argtypes = [vp]
        L.cheb_varhelm_last_residual.argtypes = [vp]
        L.cheb_varhelm_last_residual.restype = C.c_double
        L.cheb_varhelm_reason.argtypes = [vp]
        L.cheb_varhelm_solve_deflated.argtypes = L.cheb_varhelm_solve.argtypes
        L.cheb_varhelm_null_count.argtypes = [vp]
        L.cheb_varhelm_defect.argtypes = [vp, dp]
        L.cheb_varhelm_null_signs_host.argtypes = [C.c_int, ip, ip, ip]
        L.cheb_varhelm_remove_null.argtypes = [vp, vp, vp, vp]
        L.cheb_varhelm_apply_deflated.argtypes = [vp, vp, vp, vp]
        L.cheb_varhelm_precond_deflated.argtypes = [vp, vp, vp, vp]
        L.cheb_project_create_variable.argtypes = [C.c_int, ip, ip, ip, dp, C.c_int, C.POINTER(vp)]
        L.cheb_project_set_inverse_density.argtypes = [vp, vp, vp]
        L.cheb_project_apply_variable.argtypes = [vp, vp, vp, vp, vp, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, vp]
        L.cheb_project_varhelm.argtypes = [vp]
        L.cheb_project_varhelm.restype = vp
        _lib = L
    return _lib


def set_option(name, value):
    """chebhip_set_option: the library's run-time switches (include/chebhip.h lists them); the environment is never read."""
    _chk(lib().chebhip_set_option(name.encode(), int(value)))


def get_option(name):
    v = C.c_int()
    _chk(lib().chebhip_get_option(name.encode(), C.byref(v)))
    return v.value


def options():
    out, i = {}, 0
    while True:
        n = lib().chebhip_option_name(i).decode()
        if not n:
            return out
        out[n] = get_option(n)
        i += 1


def _chk(rc):
    if rc != 0:
        raise ChebhipError(rc, lib().chebhip_last_error().decode())


def _ints(v):
    return (C.c_int * len(v))(*[int(x) for x in v])


def _np_dp(a):
    import numpy as np
    assert isinstance(a, np.ndarray) and a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _dev_ptr(t, n):
    import torch
    assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64 and t.is_contiguous()
    assert t.numel() == n, "expected %d elements, got %d" % (n, t.numel())
    return t.data_ptr()


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def device_view(ptr, n):
    """A float64 tensor over n doubles of device memory owned by someone else (no copy)."""
    import torch

    if not ptr or int(n) == 0:          # an empty vector (a slab that owns only boundary planes): the library may hand over NULL
        return torch.empty(0, dtype=torch.float64, device=torch.device("cuda", torch.cuda.current_device()))

    class _Arr:
        pass
    a = _Arr()
    a.__cuda_array_interface__ = {"shape": (int(n),), "typestr": "<f8", "data": (int(ptr), False), "version": 2, "strides": None}
    return torch.as_tensor(a, device=torch.device("cuda", torch.cuda.current_device()))


REDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p)


def allreduce_trampoline(group=None):
    """A chebhip_reduce_fn that sums device doubles over the ranks of `group` with torch.distributed."""
    import torch.distributed as dist

    def red(ctx, ptr, count, stream):
        try:
            t = device_view(ptr, count)
            if dist.get_backend(group) == "gloo":          # rehearsal on one GPU: stage through the host
                h = t.cpu(); dist.all_reduce(h, group=group); t.copy_(h)
            else:
                dist.all_reduce(t, group=group)
            return 0
        except Exception:
            import traceback
            traceback.print_exc()
            return 5
    return REDUCE_FN(red)


class _Handle:
    """Owner of one library handle `_h`; a subclass names its destroy entry point in `_destroy`.  destroy() may be called any number
    of times, also after a constructor that raised before `_h` was set; a borrowed handle (`_owned` false) is dropped, not destroyed."""
    _destroy = None
    _owned = True

    def destroy(self):
        if getattr(self, "_h", None):
            if self._owned:
                getattr(lib(), self._destroy)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class ChebPlan(_Handle):
    """y = d/dx_tr x on a row-major tensor of shape dims (MatCreateCheb, chebyshev.c:89-138)."""
    _destroy = "cheb_plan_destroy"

    def __init__(self, dims, tr):
        self.dims = tuple(int(d) for d in dims)
        self.tr = int(tr)
        h = C.c_void_p()
        _chk(lib().cheb_plan_create(len(self.dims), self.tr, _ints(self.dims), C.byref(h)))
        self._h = h
        self.size = lib().cheb_plan_size(h)

    def mult(self, x, y):
        """ChebMult (chebyshev.c:142-199) on device tensors, asynchronous on torch's current stream."""
        _chk(lib().cheb_apply(self._h, _dev_ptr(x, self.size), _dev_ptr(y, self.size), _stream()))
        return y

    def mult_host(self, x):
        import numpy as np
        x = np.ascontiguousarray(x, dtype=np.float64)
        assert x.size == self.size
        y = np.empty_like(x)
        _chk(lib().cheb_apply_host(self._h, _np_dp(x), _np_dp(y)))
        return y


NODES = {"all": 0, "interior": 1}


def _nodes(v):
    if v in NODES.values():
        return int(v)
    if v not in NODES:
        raise ValueError("node set %r: expected one of %s" % (v, sorted(NODES)))
    return NODES[v]


def resample_matrix(n_in, n_out, nodes_in="all", nodes_out="all"):
    """The interpolation matrix of one direction (cheb_resample_matrix_host) as a numpy array of shape
    (stored output nodes, stored input nodes); needs no device."""
    import numpy as np
    ni, no = _nodes(nodes_in), _nodes(nodes_out)
    R = np.empty((max(int(n_out) - 2 * no, 0), max(int(n_in) - 2 * ni, 0)))
    _chk(lib().cheb_resample_matrix_host(int(n_in), ni, int(n_out), no, R.ctypes.data_as(C.POINTER(C.c_double)) if R.size else None))
    return R


class Resample(_Handle):
    """y = (R_0 x ... x R_{d-1}) x: a field on the CGL grid dims_in (node set nodes_in: "all" or "interior") interpolated to the
    grid dims_out (cheb_resample_*); ncomp components innermost.  Sizes: size(0) input values, size(1) output values."""
    _destroy = "cheb_resample_destroy"

    def __init__(self, dims_in, dims_out, nodes_in="all", nodes_out="all", ncomp=1):
        self.dims_in = tuple(int(d) for d in dims_in)
        self.dims_out = tuple(int(d) for d in dims_out)
        if len(self.dims_in) != len(self.dims_out):
            raise ValueError("dims_in and dims_out have different lengths")
        h = C.c_void_p()
        _chk(lib().cheb_resample_create(len(self.dims_in), _ints(self.dims_in), _nodes(nodes_in), _ints(self.dims_out),
                                        _nodes(nodes_out), int(ncomp), C.byref(h)))
        self._h = h
        self.ncomp = int(ncomp)

    def size(self, which):
        return lib().cheb_resample_size(self._h, int(which))

    def apply(self, x, y):
        """Asynchronous on torch's current stream."""
        _chk(lib().cheb_resample_apply(self._h, _dev_ptr(x, self.size(0)), _dev_ptr(y, self.size(1)), _stream()))
        return y


MODAL = {"forward": 0, "backward": 1}


def modal_matrix(n, which):
    """One direction's Chebyshev transform matrix (cheb_modal_matrix_host) as an (n, n) numpy array: "forward" T (values ->
    coefficients, T[k][j] = 2 / (N c_k c_j) cos(pi j k / N)) or "backward" B (B[j][k] = T_k(x_j)); needs no device."""
    import numpy as np
    if which not in MODAL:
        raise ValueError("transform %r: expected one of %s" % (which, sorted(MODAL)))
    M = np.empty((max(int(n), 0),) * 2)
    _chk(lib().cheb_modal_matrix_host(int(n), MODAL[which], M.ctypes.data_as(C.POINTER(C.c_double)) if M.size else None))
    return M


def cc_weights(n):
    """The Clenshaw-Curtis weights of the n CGL nodes (cheb_modal_weights_host): exact up to degree n - 1, sum 2; needs no device."""
    import numpy as np
    w = np.empty(max(int(n), 0))
    _chk(lib().cheb_modal_weights_host(int(n), w.ctypes.data_as(C.POINTER(C.c_double)) if w.size else None))
    return w


def _sigma(n, sigma):
    import numpy as np
    s = np.ascontiguousarray(sigma, dtype=np.float64)
    if s.shape != (int(n),):
        raise ValueError("sigma: expected %d values, got shape %r" % (int(n), s.shape))
    return s


def filter_matrix(n, sigma):
    """F = B diag(sigma) T of one direction (cheb_modal_filter_matrix_host); sigma all ones gives exactly the identity."""
    import numpy as np
    s = _sigma(n, sigma)
    F = np.empty((int(n), int(n)))
    _chk(lib().cheb_modal_filter_matrix_host(int(n), _np_dp(s), _np_dp(F)))
    return F


def exp_filter(n, order=16, alpha=36.0, cutoff=0):
    """sigma_k = 1 for k < cutoff and exp(-alpha ((k - cutoff) / (N - cutoff))^order) from there on, N = n - 1."""
    import numpy as np
    N, kc = int(n) - 1, int(cutoff)
    if not 0 <= kc < N:
        raise ValueError("cutoff %d outside 0..%d" % (kc, N - 1))
    k = np.arange(N + 1, dtype=np.float64)
    return np.where(k < kc, 1.0, np.exp(-float(alpha) * (np.maximum(k - kc, 0.0) / (N - kc)) ** order))


def sharp_filter(n, keep):
    """sigma_k = 1 for k < keep and 0 otherwise."""
    import numpy as np
    return (np.arange(int(n)) < int(keep)).astype(np.float64)


class ChebModal(_Handle):
    """The modal side of `nfields` stacked full-grid fields on the CGL grid `dims` (cheb_modal_*): values <-> Chebyshev
    coefficients, modal filters, per-direction spectra and Clenshaw-Curtis integrals.  Fields are field-major, row-major over all
    nodes; size() values per array.  Everything is asynchronous on torch's current stream.  periodic (None: no direction): one
    flag per direction; a flagged direction (2 <= dims[k] <= 256) transforms with fourier_modal_matrix, its coefficients laid out
    as fourier_modes(dims[k]) says, integrates with the weight 2 / dims[k], and takes its filter's sigma per coefficient position
    (fourier_filter expands a function of the wavenumber); spectrum sums squares per position, the caller folds cos / sin pairs."""
    _destroy = "cheb_modal_destroy"

    def __init__(self, dims, nfields=1, periodic=None):
        self.dims = tuple(int(d) for d in dims)
        self.nfields = int(nfields)
        self.periodic = _periodic_flags(periodic, len(self.dims))
        h = C.c_void_p()
        if periodic is None:
            _chk(lib().cheb_modal_create(len(self.dims), _ints(self.dims), self.nfields, C.byref(h)))
        else:
            _chk(lib().cheb_modal_create_basis(len(self.dims), _ints(self.dims), self.nfields, _ints([int(p) for p in self.periodic]),
                                               C.byref(h)))
        self._h = h

    def size(self):
        return lib().cheb_modal_size(self._h)

    def spectrum_size(self):
        return lib().cheb_modal_spectrum_size(self._h)

    def forward(self, u, a):
        """a = coefficients of the values u."""
        _chk(lib().cheb_modal_forward(self._h, _dev_ptr(u, self.size()), _dev_ptr(a, self.size()), _stream()))
        return a

    def backward(self, a, u):
        """u = values of the coefficients a."""
        _chk(lib().cheb_modal_backward(self._h, _dev_ptr(a, self.size()), _dev_ptr(u, self.size()), _stream()))
        return u

    def set_filter(self, k, sigma):
        """sigma of direction k (dims[k] host values, e.g. exp_filter / sharp_filter); None clears."""
        if sigma is None:
            _chk(lib().cheb_modal_set_filter(self._h, int(k), None))
        else:
            if not 0 <= int(k) < len(self.dims):
                raise ChebhipError(2, "direction %d out of range 0..%d" % (int(k), len(self.dims) - 1))
            _chk(lib().cheb_modal_set_filter(self._h, int(k), _np_dp(_sigma(self.dims[int(k)], sigma))))

    def filter(self, u, v):
        """v = (F_0 x ... x F_{d-1}) u over the directions with a filter set."""
        _chk(lib().cheb_modal_filter(self._h, _dev_ptr(u, self.size()), _dev_ptr(v, self.size()), _stream()))
        return v

    def spectrum(self, a, E=None):
        """E[f][k][m] = sum of a^2 with direction k's index held at m: a device tensor of spectrum_size() values, field by field,
        direction by direction."""
        import torch
        if E is None:
            E = torch.empty(self.spectrum_size(), dtype=torch.float64, device=a.device)
        _chk(lib().cheb_modal_spectrum(self._h, _dev_ptr(a, self.size()), _dev_ptr(E, self.spectrum_size()), _stream()))
        return E

    def integrate(self, u, v=None, out=None):
        """The integrals of u (of u v) over the domain, one per field, as a device tensor of nfields values; does not synchronise."""
        import torch
        if out is None:
            out = torch.empty(self.nfields, dtype=torch.float64, device=u.device)
        _chk(lib().cheb_modal_integrate(self._h, _dev_ptr(u, self.size()), None if v is None else _dev_ptr(v, self.size()),
                                        _dev_ptr(out, self.nfields), _stream()))
        return out


def _periodic_flags(periodic, d):
    if periodic is None:
        return (False,) * d
    flags = tuple(bool(p) for p in periodic)
    if len(flags) != d:
        raise ValueError("periodic: expected %d flags, got %d" % (d, len(flags)))
    return flags


def fourier_nodes(n):
    """The n nodes x_j = -1 + 2 j / n of a periodic direction (cheb_fourier_nodes_host): period 2, no duplicated end point;
    2 <= n <= 256.  Needs no device."""
    import numpy as np
    x = np.empty(max(int(n), 0))
    _chk(lib().cheb_fourier_nodes_host(int(n), _np_dp(x) if x.size else None))
    return x


def fourier_diff_matrix(n, order=1):
    """D_F (order 1) or D_F D_F (order 2) of a periodic direction of n nodes as an (n, n) numpy array (cheb_fourier_diff_matrix_host):
    D_F = pi D_theta with D_theta[i][j] = 1/2 (-1)^(i-j) cot(pi (i-j) / n) for even n and 1/2 (-1)^(i-j) / sin(pi (i-j) / n) for
    odd n, zero diagonal.  The second derivative is the product, formed in long double and rounded once -- not the textbook
    second-derivative matrix, from which it differs at the Nyquist vector of an even n.  Needs no device."""
    import numpy as np
    D = np.empty((max(int(n), 0),) * 2)
    _chk(lib().cheb_fourier_diff_matrix_host(int(n), int(order), _np_dp(D) if D.size else None))
    return D


FOURIER_KINDS = ("cos", "sin", "nyquist")        # CHEB_FOURIER_*


def fourier_modes(n):
    """The coefficient layout of a periodic direction of n nodes (cheb_fourier_modes_host): a list of (k, kind) per position, kind
    one of FOURIER_KINDS.  With c = -1 / n, the point the flip j -> n-1-j reflects about: position 0 is the constant (0, "cos"),
    position k <= floor((n-1)/2) is cos(pi k (x - c)); from the far end, position n-1 is the Nyquist vector (n/2, "nyquist") for
    even n, followed downwards by sin(pi k (x - c)), k = 1, 2, ...; for odd n the sines start at n-1.  Needs no device."""
    n = int(n)
    k, kind = (C.c_int * max(n, 1))(), (C.c_int * max(n, 1))()
    _chk(lib().cheb_fourier_modes_host(n, k, kind))
    return [(k[p], FOURIER_KINDS[kind[p]]) for p in range(n)]


def fourier_modal_matrix(n, which):
    """The transform matrix of a periodic direction (cheb_fourier_modal_matrix_host) as an (n, n) numpy array: "backward" B, whose
    column p is mode p of fourier_modes(n) with amplitude 1 (the constant's coefficient is the mean, a cos / sin coefficient the
    amplitude), or "forward" T = B^-1.  Needs no device."""
    import numpy as np
    if which not in MODAL:
        raise ValueError("transform %r: expected one of %s" % (which, sorted(MODAL)))
    M = np.empty((max(int(n), 0),) * 2)
    _chk(lib().cheb_fourier_modal_matrix_host(int(n), MODAL[which], _np_dp(M) if M.size else None))
    return M


def fourier_line(n, scale=1.0):
    """(S, Sinv, lam) of the line operator -scale^2 D_F D_F on all n nodes of a periodic direction (cheb_fourier_line_host), in
    closed form: S = fourier_modal_matrix(n, "backward"), Sinv its inverse, lam = (pi k scale)^2 in the layout of fourier_modes(n),
    exactly 0 for the constant and the Nyquist vector.  Needs no device."""
    import numpy as np
    n = int(n)
    S, Si, lam = np.empty((max(n, 0),) * 2), np.empty((max(n, 0),) * 2), np.empty(max(n, 0))
    ptr = lambda a: _np_dp(a) if a.size else None
    _chk(lib().cheb_fourier_line_host(n, float(scale), ptr(S), ptr(Si), ptr(lam)))
    return S, Si, lam


def fourier_filter(n, sigma_of_k):
    """sigma per coefficient position of a periodic direction from a function of the wavenumber k = 0 .. n // 2 (what
    ChebModal.set_filter takes there): a cos / sin pair gets one value."""
    import numpy as np
    return np.array([float(sigma_of_k(k)) for k, _ in fourier_modes(n)], dtype=np.float64)


def cgl_nodes(n):
    """The n Chebyshev-Gauss-Lobatto nodes x_j = cos(pi j / (n - 1)) (cheb_nodes_host), x_0 = +1: long double, rounded once; the
    table the device interpolates on.  Needs no device."""
    import numpy as np
    x = np.empty(max(int(n), 0))
    _chk(lib().cheb_nodes_host(int(n), x.ctypes.data_as(C.POINTER(C.c_double)) if x.size else None))
    return x


def interp_matrix(n, x, periodic=False):
    """The barycentric rows l_j(x_i) of the coordinates x on the n CGL nodes (cheb_points_matrix_host) as an (len(x), n) numpy
    array: long double on the double node table, rounded once.  A coordinate on a node gives the exact unit row, a NaN or infinite
    one a row of NaN, |x| > 1 extrapolates.  Needs no device.
    periodic: the rows r_j(x_i) of the trigonometric interpolant on fourier_nodes(n) (cheb_points_fourier_matrix_host), by its cosine
    sums in long double, rounded once; x is wrapped into the period, never extrapolated."""
    import numpy as np
    xs = np.ascontiguousarray(x, dtype=np.float64).ravel()
    R = np.empty((xs.size, max(int(n), 0)))
    if periodic:
        _chk(lib().cheb_points_fourier_matrix_host(int(n), int(xs.size), _np_dp(xs), 0, _np_dp(R)))
    else:
        _chk(lib().cheb_points_matrix_host(int(n), int(xs.size), _np_dp(xs), _np_dp(R)))
    return R


def deriv_matrix(n, x, periodic=False):
    """The rows l'_j(x_i) of the derivative of the barycentric interpolant on the n CGL nodes (cheb_points_dmatrix_host) as an
    (len(x), n) numpy array: long double on the double node table, rounded once.  A coordinate on a node gives that node's row of
    the differentiation matrix, a NaN or infinite one a row of NaN, |x| > 1 extrapolates.  Needs no device.
    periodic: the rows r_j'(x_i) of the trigonometric interpolant's derivative (cheb_points_fourier_matrix_host, deriv = 1); at a
    node, that node's row of fourier_diff_matrix(n)."""
    import numpy as np
    xs = np.ascontiguousarray(x, dtype=np.float64).ravel()
    R = np.empty((xs.size, max(int(n), 0)))
    if periodic:
        _chk(lib().cheb_points_fourier_matrix_host(int(n), int(xs.size), _np_dp(xs), 1, _np_dp(R)))
    else:
        _chk(lib().cheb_points_dmatrix_host(int(n), int(xs.size), _np_dp(xs), _np_dp(R)))
    return R


class ChebPoints(_Handle):
    """Values of `nfields` stacked full-grid fields on the CGL grid `dims` (field-major, row-major over all nodes, as ChebModal) at
    arbitrary points of [-1, 1]^d (cheb_points_*): scattered points (eval) and tensor grids of arbitrary coordinates (eval_grid:
    plane and line cuts, plotting grids), and the transpose of the scattered evaluation (spread: point forces and sources on the
    grid).  Coordinates are device tensors; |x| > 1 extrapolates, a NaN coordinate gives NaN at that
    point only, a point on a node returns the field's bits.  Everything but reserve_grid is asynchronous on torch's current stream.
    First derivatives with respect to the reference coordinates: deriv=(0 or 1 per direction) on eval, spread and eval_grid takes
    the flagged directions' derivative rows (drows) in place of their value rows; eval_grad gives every first derivative of every
    field in one call.

    periodic (None: no direction): one flag per direction (cheb_points_create_basis).  A flagged direction holds a
    periodic function on fourier_nodes(dims[k]), 2 <= dims[k] <= 256, and is evaluated by its trigonometric interpolant.  There a
    coordinate is WRAPPED into the period, whatever its size -- it is never extrapolated, unlike a CGL direction; a coordinate that
    is a node modulo the period returns the field's bits, NaN or +-Inf poison their point only.  Derivatives are with respect to the
    reference coordinate (period 2).  spread(delta=True) divides by the weight 2 / n of a periodic direction's nodes, so that
    ChebModal(dims, periodic=...).integrate(out, phi) is sum_p s_p phi(x_p) for every phi the grid holds."""
    _destroy = "cheb_points_destroy"

    def __init__(self, dims, nfields=1, periodic=None):
        self.dims = tuple(int(d) for d in dims)
        self.nfields = int(nfields)
        self.periodic = _periodic_flags(periodic, len(self.dims))
        h = C.c_void_p()
        if periodic is None:
            _chk(lib().cheb_points_create(len(self.dims), _ints(self.dims), self.nfields, C.byref(h)))
        else:
            _chk(lib().cheb_points_create_basis(len(self.dims), _ints(self.dims), self.nfields, _ints([int(p) for p in self.periodic]),
                                                C.byref(h)))
        self._h = h
        self._reserved = None

    def size(self):
        n = self.nfields
        for d in self.dims:
            n *= d
        return n

    @property
    def chunk(self):
        """Points per chunk of eval: the rows and direction 0's output of one chunk are the handle's work memory."""
        return lib().cheb_points_chunk(self._h)

    def _rows(self, entry, k, x, out):
        """rows and drows: the C entry's (len(x), dims[k]) device tensor of direction k's rows for the device coordinates x."""
        import torch
        if not 0 <= int(k) < len(self.dims):
            raise ChebhipError(2, "direction %d out of range 0..%d" % (int(k), len(self.dims) - 1))
        m, n = x.numel(), self.dims[int(k)]
        if out is None:
            out = torch.empty((m, n), dtype=torch.float64, device=x.device)
        if m:
            _chk(entry(self._h, int(k), _dev_ptr(x, m), m, _dev_ptr(out, m * n), _stream()))
        return out

    def rows(self, k, x, out=None):
        """The rows l_j(x_i) of direction k for the device coordinates x: a (len(x), dims[k]) device tensor."""
        return self._rows(lib().cheb_points_rows, k, x, out)

    def _deriv(self, deriv):
        """deriv as the C array of d ints (None: NULL, the plain call); values other than 0 and 1 are refused by the library."""
        if deriv is None:
            return None
        deriv = tuple(int(v) for v in deriv)
        if len(deriv) != len(self.dims):
            raise ValueError("deriv: expected %d flags, got %d" % (len(self.dims), len(deriv)))
        return _ints(deriv)

    def drows(self, k, x, out=None):
        """The rows l'_j(x_i) of the interpolant's derivative in direction k for the device coordinates x (cheb_points_drows): a
        (len(x), dims[k]) device tensor."""
        return self._rows(lib().cheb_points_drows, k, x, out)

    def eval_grad(self, u, pts, out=None, value=False, scale=None):
        """out[f][c][p] = scale[c] d u_f / d x_c at pts[p], c < d, in one call (cheb_points_eval_grad): an (nfields, d, npts) device
        tensor; value=True appends the value as component d: (nfields, d + 1, npts).  scale: d finite factors 2 / L_k, None = ones."""
        import numpy as np
        import torch
        d = len(self.dims)
        if pts.dim() != 2 or pts.shape[1] != d:
            raise ValueError("pts: expected shape (npts, %d), got %r" % (d, tuple(pts.shape)))
        npts, nc = pts.shape[0], d + (1 if value else 0)
        if out is None:
            out = torch.empty((self.nfields, nc, npts), dtype=torch.float64, device=u.device)
        sc = None
        if scale is not None:
            sc = np.ascontiguousarray(scale, dtype=np.float64).ravel()
            if sc.size != d:
                raise ValueError("scale: expected %d factors, got %d" % (d, sc.size))
        _chk(lib().cheb_points_eval_grad(self._h, _dev_ptr(u, self.size()) if npts else None, _dev_ptr(pts, npts * d) if npts else None,
                                         npts, None if sc is None else _np_dp(sc), 1 if value else 0,   # CHEB_POINTS_GRAD_VALUE
                                         _dev_ptr(out, self.nfields * nc * npts) if npts else None, _stream()))
        return out

    def eval(self, u, pts, out=None, deriv=None):
        """out[f][p] = the value of field f at the point pts[p]: pts is an (npts, d) device tensor, out (nfields, npts).  deriv: d
        flags, 0 or 1: the derivative along the flagged directions instead (cheb_points_eval_deriv); None is the plain call."""
        import torch
        d = len(self.dims)
        if pts.dim() != 2 or pts.shape[1] != d:
            raise ValueError("pts: expected shape (npts, %d), got %r" % (d, tuple(pts.shape)))
        npts = pts.shape[0]
        if out is None:
            out = torch.empty((self.nfields, npts), dtype=torch.float64, device=u.device)
        dv = self._deriv(deriv)
        if npts or dv is not None:                         # (no points and no flags to refuse: nothing to call)
            _chk(lib().cheb_points_eval_deriv(self._h, _dev_ptr(u, self.size()) if npts else None, _dev_ptr(pts, npts * d) if npts else None,
                                              npts, dv, _dev_ptr(out, self.nfields * npts) if npts else None, _stream()))
        return out

    def spread(self, s, pts, out=None, accumulate=False, delta=False, deriv=None):
        """The transpose of eval: out[f][i] = sum_p s[f][p] prod_k l_{i_k}(pts[p][k]) on the full grid (cheb_points_spread).  s is an
        (nfields, npts) device tensor (npts values for one field), pts (npts, d), out size() values: nfields stacked fields, written,
        or added to with accumulate=True.  delta=True divides by the Clenshaw-Curtis weights of the nodes, so that
        ChebModal.integrate(out, phi) is sum_p s_p phi(x_p): a point source of strength s.  Results repeat bit for bit; a NaN
        coordinate makes every field NaN, a NaN strength its own field only.  deriv: d flags, 0 or 1: the flagged directions take
        their derivative rows, the transpose of eval(deriv=...) (cheb_points_spread_deriv) -- a force dipole; None is the plain call."""
        import torch
        d = len(self.dims)
        if pts.dim() != 2 or pts.shape[1] != d:
            raise ValueError("pts: expected shape (npts, %d), got %r" % (d, tuple(pts.shape)))
        npts = pts.shape[0]
        if s.numel() != self.nfields * npts:
            raise ValueError("s: expected %d x %d values, got %d" % (self.nfields, npts, s.numel()))
        if out is None:
            if accumulate:
                raise ValueError("accumulate=True needs the array to add to (out)")
            out = torch.empty(self.size(), dtype=torch.float64, device=pts.device)
        flags = (1 if accumulate else 0) | (2 if delta else 0)                     # CHEB_SPREAD_ACCUMULATE, CHEB_SPREAD_DELTA
        dv = self._deriv(deriv)
        sp_, xp_ = (_dev_ptr(s, self.nfields * npts), _dev_ptr(pts, npts * d)) if npts else (None, None)
        _chk(lib().cheb_points_spread_deriv(self._h, sp_, xp_, npts, dv, _dev_ptr(out, self.size()), flags, _stream()))
        return out

    def spread_pass(self):
        """Points per pass of spread (cheb_points_spread_pass; the option points_spread_pass lowers it)."""
        return lib().cheb_points_spread_pass(self._h)

    def reserve_grid(self, m_max):
        """Allocates eval_grid's buffers for every grid of at most m_max[k] coordinates in direction k (synchronous)."""
        m_max = tuple(int(v) for v in m_max)
        if len(m_max) != len(self.dims):
            raise ValueError("m_max: expected %d counts" % len(self.dims))
        _chk(lib().cheb_points_grid_reserve(self._h, _ints(m_max)))
        self._reserved = m_max

    def eval_grid(self, u, coords, out=None, deriv=None):
        """The fields on the tensor grid coords[0] x .. x coords[d-1] (one 1-d device tensor of coordinates per direction): a device
        tensor of shape (nfields, len(coords[0]), .., len(coords[d-1])).  Without an earlier reserve_grid the buffers are
        reserved for this grid's size; a grid larger than the reserved one is refused.  deriv: d flags, 0 or 1: the derivative along
        the flagged directions instead (cheb_points_eval_grid_deriv); None is the plain call."""
        import torch
        if len(coords) != len(self.dims):
            raise ValueError("coords: expected %d coordinate arrays" % len(self.dims))
        m = tuple(int(c.numel()) for c in coords)
        if self._reserved is None:
            self.reserve_grid(tuple(max(v, 1) for v in m))
        nout = self.nfields
        for v in m:
            nout *= v
        if out is None:
            out = torch.empty((self.nfields,) + m, dtype=torch.float64, device=u.device)
        xs = torch.cat([c.reshape(-1) for c in coords]) if len(coords) > 1 else coords[0].reshape(-1).contiguous()
        dv = self._deriv(deriv)
        args = (self._h, _dev_ptr(u, self.size()), _dev_ptr(xs, sum(m)) if sum(m) else None, _ints(m))
        _chk(lib().cheb_points_eval_grid_deriv(*args, dv, _dev_ptr(out, nout) if nout else None, _stream()))
        return out


DEALIAS = {"R": 0, "P": 1, "G": 2}


def dealias_size(n, periodic=False):
    """The 3/2 rule's fine size of a direction of n points: ceil(3n/2) on a CGL direction (cheb_dealias_fine_size),
    3 floor(n/2) + 1 on a periodic one (cheb_dealias_fine_size_basis): a product reaches wavenumber 2K, K = floor(n/2), which must not
    fold onto |k| <= K."""
    m = lib().cheb_dealias_fine_size_basis(int(n), 1) if periodic else lib().cheb_dealias_fine_size(int(n))
    if m < 0:
        raise ChebhipError(4, lib().chebhip_last_error().decode())
    return m


def dealias_matrix(n, which, m=None, periodic=False):
    """One direction's dealiasing matrix (cheb_dealias_matrix_host) for n coarse and m fine points (default dealias_size(n)):
    "R" (m, n) interpolation to the fine nodes, "P" (n, m) = B_n T_m[0:n, :] back to the coarse nodes keeping n modes, "G" (m, n)
    = R D; needs no device.  periodic (cheb_dealias_matrix_basis_host): the nodes are fourier_nodes(n) and fourier_nodes(m), R is
    the trigonometric interpolant, G = R D_F, and P cuts the fine grid's Fourier series at |k| <= floor(n/2) (for even n the Nyquist
    wavenumber stays, as the coarse grid sees it: the square of (-1)^j comes back as 1/2)."""
    import numpy as np
    if which not in DEALIAS:
        raise ValueError("matrix %r: expected one of %s" % (which, sorted(DEALIAS)))
    n = int(n)
    m = dealias_size(n, periodic) if m is None else int(m)
    A = np.empty((max(n, 0), max(m, 0)) if which == "P" else (max(m, 0), max(n, 0)))
    ptr = A.ctypes.data_as(C.POINTER(C.c_double)) if A.size else None
    if periodic:
        _chk(lib().cheb_dealias_matrix_basis_host(n, m, DEALIAS[which], 1, ptr))
    else:
        _chk(lib().cheb_dealias_matrix_host(n, m, DEALIAS[which], ptr))
    return A


class ChebDealias(_Handle):
    """Dealiased products of `nfields` stacked full-grid fields on the CGL grid `dims` (cheb_dealias_*; field-major, row-major over
    all nodes, as ChebModal): multiply(u, v) = the truncation to degree dims[k] - 1 per direction of the polynomial product u v,
    advect(vel, c) = that of sum_k vel[k] d_k c.  `fine` is the padded grid (default: the 3/2 rule, dealias_size per direction;
    fine[k] == dims[k] leaves direction k unpadded).  Asynchronous on torch's current stream; advect reserves its work memory on
    first use (synchronous).

    periodic (None: no direction): one flag per direction (cheb_dealias_create_basis).  A flagged direction holds a
    periodic function on fourier_nodes(dims[k]), 2 <= dims[k] <= 256; the product is cut at the wavenumbers |k| <= floor(n/2) the
    grid holds (dealias_matrix(..., periodic=True)), the derivative of advect is D_F, and the default fine size is
    3 floor(n/2) + 1.  advect differentiates in reference coordinates (period 2), as it does on a CGL direction: it has no scale."""
    _destroy = "cheb_dealias_destroy"

    def __init__(self, dims, nfields=1, fine=None, periodic=None):
        self.dims = tuple(int(d) for d in dims)
        self.nfields = int(nfields)
        self.periodic = _periodic_flags(periodic, len(self.dims))
        if fine is not None and len(fine) != len(self.dims):
            raise ValueError("fine: expected %d sizes" % len(self.dims))
        h = C.c_void_p()
        if periodic is None:
            _chk(lib().cheb_dealias_create(len(self.dims), _ints(self.dims), None if fine is None else _ints(fine), self.nfields, C.byref(h)))
        else:
            _chk(lib().cheb_dealias_create_basis(len(self.dims), _ints(self.dims), None if fine is None else _ints(fine),
                                                 _ints([int(p) for p in self.periodic]), self.nfields, C.byref(h)))
        self._h = h
        m = (C.c_int * len(self.dims))()
        _chk(lib().cheb_dealias_fine_dims(self._h, m))
        self.fine = tuple(m)
        self._advect = False

    def size(self):
        return lib().cheb_dealias_size(self._h)

    def work_bytes(self):
        """Device bytes the handle owns (matrices included); grows once, at the first advect."""
        return lib().cheb_dealias_work_bytes(self._h)

    def multiply(self, u, v, out=None):
        """out[f] = the dealiased product u[f] v[f]; `u is v` gives squares."""
        import torch
        if out is None:
            out = torch.empty_like(u)
        _chk(lib().cheb_dealias_multiply(self._h, _dev_ptr(u, self.size()), _dev_ptr(v, self.size()), _dev_ptr(out, self.size()), _stream()))
        return out

    def reserve_advect(self):
        _chk(lib().cheb_dealias_reserve_advect(self._h))
        self._advect = True

    def advect(self, vel, c, out=None):
        """out[f] = the dealiased sum_k vel[k] d_k c[f]; vel holds len(dims) fields."""
        import torch
        if not self._advect:
            self.reserve_advect()
        if out is None:
            out = torch.empty_like(c)
        nv = self.size() // self.nfields * len(self.dims)
        _chk(lib().cheb_dealias_advect(self._h, _dev_ptr(vel, nv), _dev_ptr(c, self.size()), _dev_ptr(out, self.size()), _stream()))
        return out


def _set_direction_weights(h, setter, k, w, named=None):
    """set_weights of ChebReduce and ChebStats: dims[k] host values into direction k through `setter`, None for the default;
    `named(n, w)` turns what is no array (a kind of reduce_weights) into one, or returns w."""
    import numpy as np
    k = int(k)
    if not 0 <= k < len(h.dims):
        raise ChebhipError(2, "direction %d out of range 0..%d" % (k, len(h.dims) - 1))
    if w is None:
        _chk(setter(h._h, k, None))
        return
    if named is not None:
        w = named(h.dims[k], w)
    w = np.ascontiguousarray(w, dtype=np.float64)
    if w.shape != (h.dims[k],):
        raise ValueError("weights of direction %d: expected %d values, got shape %r" % (k, h.dims[k], w.shape))
    _chk(setter(h._h, k, _np_dp(w)))


REDUCE_W = {"integral": 0, "mean": 1, "node": 2, "dnode": 3, "point": 4, "dpoint": 5}


def reduce_weights(n, kind, arg=None):
    """The n weights one contracted direction of n points is summed against (cheb_reduce_weights_host), long double rounded once:
    "integral" (the Clenshaw-Curtis weights), "mean" (half of them), ("node", j) the unit vector e_j (the value on the grid plane
    i = j; j = 0 is x = +1), ("dnode", j) row j of D (d/dx on that plane; the outward derivative is + at j = 0, - at j = n - 1),
    ("point", x) the barycentric row of x, ("dpoint", x) r(x)^T D.  A kind with an argument is a pair, or `arg` carries it.
    Needs no device."""
    import numpy as np
    if isinstance(kind, (tuple, list)):
        if len(kind) != 2 or arg is not None:
            raise ValueError("weights %r: expected a name or a (name, argument) pair" % (kind,))
        kind, arg = kind
    if kind not in REDUCE_W:
        raise ValueError("weights %r: expected one of %s" % (kind, sorted(REDUCE_W)))
    if (arg is None) != (REDUCE_W[kind] < 2):
        raise ValueError("weights %r take %s argument" % (kind, "no" if REDUCE_W[kind] < 2 else "one"))
    w = np.empty(max(int(n), 0))
    _chk(lib().cheb_reduce_weights_host(int(n), REDUCE_W[kind], 0.0 if arg is None else float(arg),
                                        w.ctypes.data_as(C.POINTER(C.c_double)) if w.size else None))
    return w


class ChebReduce(_Handle):
    """Partial contractions of `nfields` stacked full-grid fields on the CGL grid `dims` (cheb_reduce_*; field-major, row-major over
    all nodes, as ChebModal): the directions listed in `over` are summed against one weight vector each, the others are kept --
    out[f][kept indices] = sum prod_k w_k[i_k] u[f][i] (v[f][i]).  Every contracted direction starts with the Clenshaw-Curtis
    weights (a partial integral); `weights` maps a direction to what set_weights takes.  apply is asynchronous on torch's current
    stream, adds in a fixed order (the same input gives the same bits) and uses no vendor GEMM."""
    _destroy = "cheb_reduce_destroy"

    def __init__(self, dims, nfields=1, over=(), weights=None):
        self.dims = tuple(int(d) for d in dims)
        self.nfields = int(nfields)
        over = (over,) if isinstance(over, int) else tuple(int(k) for k in over)
        for k in over:
            if not 0 <= k < len(self.dims):
                raise ChebhipError(2, "direction %d out of range 0..%d" % (k, len(self.dims) - 1))
        self.over = tuple(sorted(set(over)))
        self.out_dims = tuple(n for k, n in enumerate(self.dims) if k not in self.over)
        h = C.c_void_p()
        _chk(lib().cheb_reduce_create(len(self.dims), _ints(self.dims), self.nfields,
                                      _ints([int(k in self.over) for k in range(len(self.dims))]), C.byref(h)))
        self._h = h
        for k, w in (weights or {}).items():
            self.set_weights(k, w)

    def size(self, which=0):
        """Values of the input (which = 0) or of the output (1)."""
        return lib().cheb_reduce_size(self._h, int(which))

    @property
    def slices(self):
        """Partial sums per output value: 1 = the kernel stores the outputs itself, more = one fold launch adds them."""
        return lib().cheb_reduce_slices(self._h)

    def set_weights(self, k, w):
        """The weights of the contracted direction k: dims[k] host values, or what reduce_weights takes as `kind` ("mean",
        ("dnode", 0), ..); None restores the default.  Synchronous."""
        def named(n, w):
            kind = isinstance(w, str) or (isinstance(w, (tuple, list)) and len(w) == 2 and isinstance(w[0], str))
            return reduce_weights(n, w) if kind else w
        _set_direction_weights(self, lib().cheb_reduce_set_weights, k, w, named)

    def apply(self, u, v=None, out=None):
        """The contraction of u (of u v; `v is u` gives squares) as a device tensor of shape (nfields,) + out_dims; does not
        synchronise.  `out` must not overlap the inputs."""
        import torch
        if out is None:
            out = torch.empty((self.nfields,) + self.out_dims, dtype=torch.float64, device=u.device)
        _chk(lib().cheb_reduce_apply(self._h, _dev_ptr(u, self.size(0)), None if v is None else _dev_ptr(v, self.size(0)),
                                     _dev_ptr(out, self.size(1)), _stream()))
        return out


def stats_spacing(n):
    """h[j] = the smaller of the distances from node j of n CGL nodes to its neighbours, one-sided at the two ends
    (cheb_stats_spacing_host): long double, rounded once.  Needs no device."""
    import numpy as np
    h = np.empty(max(int(n), 0))
    _chk(lib().cheb_stats_spacing_host(int(n), h.ctypes.data_as(C.POINTER(C.c_double)) if h.size else None))
    return h


def stats_rate(n, s=1.0):
    """r[j] = s / h[j] (cheb_stats_rate_host), the quotient in long double rounded once: what ChebStats.cfl multiplies the
    speeds along a direction of n points with.  Needs no device."""
    import numpy as np
    r = np.empty(max(int(n), 0))
    _chk(lib().cheb_stats_rate_host(int(n), float(s), r.ctypes.data_as(C.POINTER(C.c_double)) if r.size else None))
    return r


def _stack2(a, b):
    import torch
    return torch.stack((a, b), dim=1).contiguous()


def stats_edges(edges, nfields, bins):
    """The host edge array of ChebStats.histogram as an (nfields, bins + 1) array: one row is repeated for every field.  Edges
    that are NaN or decrease are a ChebhipError of code CHEBHIP_ERR_ARG.  Needs no device."""
    import numpy as np
    e = np.asarray(edges, dtype=np.float64)
    if e.ndim == 1:
        e = np.broadcast_to(e, (int(nfields), e.shape[0]))
    if e.shape != (int(nfields), int(bins) + 1):
        raise ChebhipError(4, "edges: expected %d + 1 values (per field), got shape %r" % (int(bins), np.shape(edges)))
    if np.isnan(e).any() or (e[:, 1:] < e[:, :-1]).any():
        raise ChebhipError(4, "edges: the values must not decrease")
    return np.ascontiguousarray(e)


class ChebStats(_Handle):
    """Statistics of `nfields` stacked full-grid fields on the CGL grid `dims` (cheb_stats_*; field-major, row-major over all
    nodes, as ChebModal): summary (min, max, where, NaN count, weighted moments), histogram (volume-weighted, optionally of a
    second field per bin) and cfl.  The weight of a node is prod_k w_k[i_k], Clenshaw-Curtis unless `weights` maps a direction to
    dims[k] values.  Everything is asynchronous on torch's current stream, adds in a fixed order (the same input gives the same
    bits) and uses no atomics."""
    _destroy = "cheb_stats_destroy"
    SUMMARY = ("min", "max", "argmin", "argmax", "nan", "m1", "m2", "m3", "m4")

    def __init__(self, dims, nfields=1, max_bins=256, weights=None):
        self.dims = tuple(int(d) for d in dims)
        self.nfields = int(nfields)
        self.max_bins = int(max_bins)
        h = C.c_void_p()
        _chk(lib().cheb_stats_create(len(self.dims), _ints(self.dims), self.nfields, self.max_bins, C.byref(h)))
        self._h = h
        for k, w in (weights or {}).items():
            self.set_weights(k, w)

    def size(self, which=0):
        """0: values of the input, 1: of a summary, 2: max_bins, 3 / 4: workgroups per field of summary, cfl / of histogram."""
        return lib().cheb_stats_size(self._h, int(which))

    def set_weights(self, k, w):
        """The weights of direction k: dims[k] host values; None restores the Clenshaw-Curtis weights.  Synchronous."""
        _set_direction_weights(self, lib().cheb_stats_set_weights, k, w)

    def summary(self, u, center=None, out=None):
        """A device tensor (nfields, 9): the columns of ChebStats.SUMMARY.  `center`: a device tensor of nfields values the
        moments are taken about (e.g. a mean from an earlier summary, without a sync), or None for 0."""
        import torch
        if out is None:
            out = torch.empty((self.nfields, 9), dtype=torch.float64, device=u.device)
        _chk(lib().cheb_stats_summary(self._h, _dev_ptr(u, self.size(0)), None if center is None else _dev_ptr(center, self.nfields),
                                      _dev_ptr(out, 9 * self.nfields), _stream()))
        return out

    @staticmethod
    def auto_range(summary):
        """(lo, hi) per field from a summary, on the device: lo = min and hi = max + 2^-40 (max - min + |max| + |min|), so that
        the maximum falls into the last bin, not into overflow (t < bins by a margin far above the roundings of t).  A field
        that is zero everywhere, or has no value that is not NaN, gets hi <= lo: everything in overflow."""
        lo, hi = summary[:, 0], summary[:, 1]
        return _stack2(lo, hi + 2.0 ** -40 * ((hi - lo) + hi.abs() + lo.abs()))

    def histogram(self, u, bins, range=None, edges=None, cond=None, out=None):
        """A device tensor (nfields, 2, bins + 3): row 0 the mass of a slot (with `cond`: the sum of W cond over it), row 1 its
        number of values; slot 0 underflow, 1..bins the bins, bins + 1 overflow, bins + 2 NaN.  `edges` (bins + 1 values, or
        that per field; host values or a device tensor) selects the bins by comparisons; otherwise the bins are uniform over
        `range`: (lo, hi), an (nfields, 2) array or device tensor, or None for auto_range of a summary of u (taken on the
        device, no sync)."""
        import numpy as np
        import torch
        bins = int(bins)
        if edges is not None:
            if range is not None:
                raise ValueError("histogram: give range or edges, not both")
            mode = 1
            spec = edges if isinstance(edges, torch.Tensor) else torch.from_numpy(stats_edges(edges, self.nfields, bins)).to(u.device)
            nspec = self.nfields * (bins + 1)
        else:
            mode = 0
            nspec = 2 * self.nfields
            if range is None:
                spec = self.auto_range(self.summary(u))
            elif isinstance(range, torch.Tensor):
                spec = range
            else:
                r = np.asarray(range, dtype=np.float64)
                if r.shape not in ((2,), (self.nfields, 2)):
                    raise ValueError("range: expected (lo, hi) or that per field, got shape %r" % (r.shape,))
                spec = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(r, (self.nfields, 2)))).to(u.device)
        if out is None:
            out = torch.empty((self.nfields, 2, bins + 3), dtype=torch.float64, device=u.device)
        _chk(lib().cheb_stats_histogram(self._h, _dev_ptr(u, self.size(0)), None if cond is None else _dev_ptr(cond, self.size(0)),
                                        mode, bins, _dev_ptr(spec, nspec), _dev_ptr(out, self.nfields * 2 * (bins + 3)), _stream()))
        return out

    def cfl(self, vel, scale=None, out=None):
        """A device tensor (2,): max_i sum_k |vel_k(i)| s_k / h_k(i_k) of the len(dims) fields of vel (whatever nfields is), and
        the flat index of the first node that attains it; NaN and the first such node if a component is NaN anywhere.
        scale: len(dims) values 2 / L_k, or None for ones."""
        import numpy as np
        import torch
        d = len(self.dims)
        if out is None:
            out = torch.empty(2, dtype=torch.float64, device=vel.device)
        sc = None
        if scale is not None:
            sc = np.ascontiguousarray(scale, dtype=np.float64)
            if sc.shape != (d,):
                raise ValueError("scale: expected %d values, got shape %r" % (d, sc.shape))
        _chk(lib().cheb_stats_cfl(self._h, _dev_ptr(vel, d * (self.size(0) // self.nfields)), None if sc is None else _np_dp(sc),
                                  _dev_ptr(out, 2), _stream()))
        return out


INVARIANTS = {"div": 1, "vort2": 2, "strain2": 4, "gamma": 8, "q": 16, "norm2": 32}


def _inv_mask(which):
    """(mask, number of fields) of a tuple of names of INVARIANTS (one name is taken as a tuple of one)."""
    which = (which,) if isinstance(which, str) else tuple(which)
    mask = 0
    for w in which:
        if w not in INVARIANTS:
            raise ValueError("invariant %r: expected one of %s" % (w, sorted(INVARIANTS)))
        mask |= INVARIANTS[w]
    if not mask:
        raise ValueError("no invariant selected")
    return mask, bin(mask).count("1")


class ChebGrad(_Handle):
    """Vector calculus of stacked full-grid fields on the CGL grid `dims` (cheb_grad_*; field-major, row-major over all nodes, as
    ChebModal): grad, tensor, div, curl, strain, laplacian as signed derivative sweeps added in a fixed order, and the pointwise
    invariants of a gradient tensor.  scale[k] multiplies the derivative along direction k (2 / L_k for a box of length L_k).  A
    vector field is d consecutive fields; the number of fields (vectors) of a call is taken from numel() // N.  out=None allocates
    the output.  The outputs come back with the layouts of include/chebhip.h, shaped (fields, *dims).  Asynchronous on torch's
    current stream; the same input gives the same bits.  periodic (None: no direction): one flag per direction; a flagged
    direction lives on fourier_nodes(dims[k]) (2 <= dims[k] <= 256, period 2 / scale[k]) and is differentiated with
    fourier_diff_matrix, by the same sweeps (cheb_grad_create_basis)."""
    _destroy = "cheb_grad_destroy"

    def __init__(self, dims, scale=None, periodic=None):
        import numpy as np
        self.dims = tuple(int(d) for d in dims)
        self.d = len(self.dims)
        self.periodic = _periodic_flags(periodic, self.d)
        sc = None
        if scale is not None:
            sc = np.ascontiguousarray(scale, dtype=np.float64)
            if sc.shape != (self.d,):
                raise ValueError("scale: expected %d values, got shape %r" % (self.d, sc.shape))
        self.scale = None if sc is None else tuple(float(v) for v in sc)
        h = C.c_void_p()
        if periodic is None:
            _chk(lib().cheb_grad_create(self.d, _ints(self.dims), None if sc is None else _np_dp(sc), C.byref(h)))
        else:
            _chk(lib().cheb_grad_create_basis(self.d, _ints(self.dims), None if sc is None else _np_dp(sc),
                                              _ints([int(p) for p in self.periodic]), C.byref(h)))
        self._h = h
        self.N = lib().cheb_grad_size(h)

    def _count(self, t, per, what):
        n = t.numel()
        if n == 0 or n % (self.N * per):
            raise ValueError("%s: %d values are no multiple of %d" % (what, n, self.N * per))
        return n // (self.N * per)

    def _run(self, fn, x, per_in, per_out, out, what):
        import torch
        n = self._count(x, per_in, what)
        if out is None:
            out = torch.empty((n * per_out,) + self.dims, dtype=torch.float64, device=x.device)
        _chk(fn(self._h, n, _dev_ptr(x, n * per_in * self.N), _dev_ptr(out, n * per_out * self.N), _stream()))
        return out

    def grad(self, s, out=None):
        """out[f * d + k] = scale_k d_k s[f]."""
        return self._run(lib().cheb_grad_grad, s, 1, self.d, out, "grad")

    def tensor(self, u, out=None):
        """G[v][c][k] = scale_k d_k u[v][c]: the gradient of a vector field, d * d fields per vector."""
        return self._run(lib().cheb_grad_tensor, u, self.d, self.d * self.d, out, "tensor")

    def div(self, u, out=None):
        return self._run(lib().cheb_grad_div, u, self.d, 1, out, "div")

    def curl(self, u, out=None):
        """d = 3: three fields per vector; d = 2: the one field d_0 u_1 - d_1 u_0."""
        return self._run(lib().cheb_grad_curl, u, self.d, 3 if self.d == 3 else 1, out, "curl")

    def strain(self, u, out=None):
        """Per vector the d (d + 1) / 2 fields (0,0), (0,1), .., (d-1,d-1) of the symmetrised gradient."""
        return self._run(lib().cheb_grad_strain, u, self.d, self.d * (self.d + 1) // 2, out, "strain")

    def work_size(self, nfields):
        """Doubles laplacian's `work` must hold for nfields fields (0: none needed)."""
        return lib().cheb_grad_work_size(self._h, int(nfields))

    def laplacian(self, s, out=None, work=None):
        """out[f] = sum_k scale_k^2 d_k^2 s[f]; `work` (work_size(nfields) doubles) is allocated if needed and not given."""
        import torch
        n = self._count(s, 1, "laplacian")
        if out is None:
            out = torch.empty((n,) + self.dims, dtype=torch.float64, device=s.device)
        ws = self.work_size(n) if n <= 16 else 0
        if ws and work is None:
            work = torch.empty(ws, dtype=torch.float64, device=s.device)
        _chk(lib().cheb_grad_laplacian(self._h, n, _dev_ptr(s, n * self.N), None if not ws else _dev_ptr(work, ws),
                                       _dev_ptr(out, n * self.N), _stream()))
        return out

    def invariants_from(self, G, which, out=None):
        """The invariants named in `which` (names of INVARIANTS) of the tensor G[v][c][k], per vector in the order of INVARIANTS'
        bits: a device tensor of shape (vectors * len(which), *dims)."""
        import torch
        mask, nsel = _inv_mask(which)
        nv = self._count(G, self.d * self.d, "invariants")
        if out is None:
            out = torch.empty((nv * nsel,) + self.dims, dtype=torch.float64, device=G.device)
        _chk(lib().cheb_grad_invariants(self._h, nv, _dev_ptr(G, nv * self.d * self.d * self.N), mask,
                                        _dev_ptr(out, nv * nsel * self.N), _stream()))
        return out

    def invariants(self, u, which, out=None):
        """invariants_from(tensor(u), which): G is a torch allocation of this call."""
        return self.invariants_from(self.tensor(u), which, out)


def layout_map(dims):
    """ChebLayout's node table on the host (cheb_layout_map_host): per row-major node its number among the interior nodes, or
    -1 - (its number among the boundary nodes); an int32 numpy array of shape dims.  Needs no device."""
    import numpy as np
    dims = tuple(int(d) for d in dims)
    m = np.empty(dims if all(n > 0 for n in dims) else (0,), dtype=np.int32)
    _chk(lib().cheb_layout_map_host(len(dims), _ints(dims), m.ctypes.data_as(C.POINTER(C.c_int)) if m.size else None))
    return m


class ChebLayout(_Handle):
    """Between the operators' vectors (interior nodes, node-major, components interleaved; Dirichlet values in a compact array of
    the boundary nodes) and full-grid, field-major fields (cheb_layout_*).  unpack / pack take the interior array with its stride
    and offset (xi, si, oi) and the boundary array likewise (xb, sb, ob); either may be None.  Values are moved, never computed.
    Asynchronous on torch's current stream."""
    _destroy = "cheb_layout_destroy"

    def __init__(self, dims):
        self.dims = tuple(int(d) for d in dims)
        h = C.c_void_p()
        _chk(lib().cheb_layout_create(len(self.dims), _ints(self.dims), C.byref(h)))
        self._h = h
        self.N, self.I, self.B = (lib().cheb_layout_size(h, w) for w in range(3))

    def unpack(self, ncomp, xi=None, si=1, oi=0, xb=None, sb=1, ob=0, out=None):
        """out[c] = component c as a full-grid field, shape (ncomp, *dims); a missing source gives 0 at its nodes."""
        import torch
        ncomp = int(ncomp)
        if out is None:
            dev = xi.device if xi is not None else xb.device if xb is not None else torch.device("cuda", torch.cuda.current_device())
            out = torch.empty((max(ncomp, 0),) + self.dims, dtype=torch.float64, device=dev)
        _chk(lib().cheb_layout_unpack(self._h, ncomp, None if xi is None else _dev_ptr(xi, self.I * int(si)), int(si), int(oi),
                                      None if xb is None else _dev_ptr(xb, self.B * int(sb)), int(sb), int(ob),
                                      _dev_ptr(out, ncomp * self.N) if ncomp > 0 else out.data_ptr(), _stream()))
        return out

    def pack(self, ncomp, fields, xi=None, si=1, oi=0, xb=None, sb=1, ob=0):
        """The inverse of unpack: writes the addressed entries of xi and xb, leaves every other entry alone."""
        ncomp = int(ncomp)
        _chk(lib().cheb_layout_pack(self._h, ncomp, _dev_ptr(fields, ncomp * self.N) if ncomp > 0 else fields.data_ptr(),
                                    None if xi is None else _dev_ptr(xi, self.I * int(si)), int(si), int(oi),
                                    None if xb is None else _dev_ptr(xb, self.B * int(sb)), int(sb), int(ob), _stream()))


def helmholtz_line(P):
    """(S, Sinv, lam) of the spectral line operator A_1 = -(D D)[1..n-1, 1..n-1] of a line of P points (cheb_helmholtz_line_host):
    A_1 = S diag(lam) S^-1, M = P - 2; modes by parity (even ones first, odd ones from the end).  Needs no device."""
    import numpy as np
    M = max(int(P) - 2, 0)
    S, Si, lam = np.empty((M, M)), np.empty((M, M)), np.empty(M)
    ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double)) if a.size else None
    _chk(lib().cheb_helmholtz_line_host(int(P), ptr(S), ptr(Si), ptr(lam)))
    return S, Si, lam


def fdpc_line(P):
    """(S, Sinv, lam) of the three-point line operator of the finite-difference preconditioner for a line of P points
    (chebhip_fdpc_line_host): T = S diag(lam) S^-1, M = P - 2, the layout and mode order of helmholtz_line.  Needs no device."""
    import numpy as np
    M = max(int(P) - 2, 0)
    S, Si, lam = np.empty((M, M)), np.empty((M, M)), np.empty(M)
    ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double)) if a.size else None
    _chk(lib().chebhip_fdpc_line_host(int(P), ptr(S), ptr(Si), ptr(lam)))
    return S, Si, lam


# the steps of the fast-diagonalisation solve (CHEBHIP_FDPC_STEP_*) and what runs for them (CHEBHIP_FDPC_ROUTE_*)
FDPC_STEPS = {"forward": 0, "forward_over_eta": 1, "forward_scaled": 2, "zsolve": 3, "scale": 4, "backward": 5}
FDPC_ROUTES = {"raw": 1, "two_launch": 2, "general": 4, "fused_mul": 8, "eta_pass": 16, "zsolve": 32, "scale3": 64, "scale_general": 128, "dense": 256}


class _FdmSteps:
    """step / step_route of the handles whose solve is the fast diagonalisation (chebhip_fdpc_step): one step of the solve along
    direction k on the handle's stacked interior fields (component-major on a Stokes handle), by the very function the solve is made
    of.  A mode the solve does not take on this handle raises ChebhipError (code 4)."""

    def _fdpc(self):
        return self._h

    def _nstep(self):
        return self.n

    def step(self, k, mode, x, y):
        n = self._nstep()
        _chk(lib().chebhip_fdpc_step(self._fdpc(), int(k), FDPC_STEPS[mode], _dev_ptr(x, n), _dev_ptr(y, n), _stream()))
        return y

    def step_route(self, k, mode):
        """The set of FDPC_ROUTES names of what that step runs between the handle's own buffers; None where step would refuse."""
        r = lib().chebhip_fdpc_step_route(self._fdpc(), int(k), FDPC_STEPS[mode])
        return None if r < 0 else frozenset(name for name, bit in FDPC_ROUTES.items() if r & bit)


def _bc_spec(spec):
    """(alpha, beta) of one end: "dirichlet", "neumann" or a pair of numbers."""
    if isinstance(spec, str):
        if spec.lower() == "dirichlet":
            return (1.0, 0.0)
        if spec.lower() == "neumann":
            return (0.0, 1.0)
        raise ValueError("unknown boundary condition %r: 'dirichlet', 'neumann' or (alpha, beta)" % spec)
    try:
        a, b = spec
        return (float(a), float(b))
    except (TypeError, ValueError):
        raise ValueError("a boundary condition is 'dirichlet', 'neumann' or (alpha, beta), got %r" % (spec,))


def _bc_ends(entry):
    """(alpha_first, beta_first, alpha_last, beta_last) of one direction: one spec for both ends or a pair (index 0, index n)."""
    if isinstance(entry, str):
        return _bc_spec(entry) * 2
    entry = tuple(entry)
    if len(entry) == 2 and all(isinstance(e, (int, float)) for e in entry):
        return _bc_spec(entry) * 2
    if len(entry) == 2:
        return _bc_spec(entry[0]) + _bc_spec(entry[1])
    raise ValueError("a direction's boundary condition is one spec or a pair of specs, got %r" % (entry,))


def _bc_periodic(entry):
    """True for the entry "periodic", which covers the whole direction; a pair with one periodic end is refused."""
    if isinstance(entry, str):
        return entry.lower() == "periodic"
    try:
        ends = tuple(entry)
    except TypeError:
        return False
    if any(isinstance(e, str) and e.lower() == "periodic" for e in ends):
        raise ChebhipError(4, "bc %r: a direction is periodic as a whole, not at one end" % (entry,))
    return False


def bc_split(bc, d):
    """(periodic, b, ends) of HelmholtzSolver's `bc`: the flag per direction, the 4 d doubles of the create calls (Dirichlet
    placeholders on a periodic direction, whose entries are not read) and, per direction, the four end values or None where it is
    periodic.  The one place that parses "periodic": a pair with one periodic end is refused here."""
    if isinstance(bc, str) or len(bc) != d:
        raise ValueError("bc needs one entry per direction (%d)" % d)
    periodic = tuple(_bc_periodic(entry) for entry in bc)
    b = bc_array(["dirichlet" if p else entry for p, entry in zip(periodic, bc)], d)
    return periodic, b, tuple(None if periodic[k] else tuple(b[4 * k:4 * k + 4]) for k in range(d))


def bc_array(bc, d):
    """The 4 d doubles of cheb_helmholtz_create_bc from a length-d sequence of per-direction entries (HelmholtzSolver's `bc`)."""
    if isinstance(bc, str) or len(bc) != d:
        raise ValueError("bc needs one entry per direction (%d)" % d)
    return [v for entry in bc for v in _bc_ends(entry)]


def helmholtz_line_bc(P, bc):
    """(S, Sinv, lam, Q, L, Binv) of the line operator with the ends eliminated by `bc` (one spec or a pair, as an entry of
    HelmholtzSolver's bc; cheb_helmholtz_line_bc_host): A~ = -(DD)_II - (DD)_IB Q = S diag(lam) S^-1, the end values
    u_B = Q u_I + Binv g, the lift L = (DD)_IB Binv.  Needs no device."""
    import numpy as np
    M = max(int(P) - 2, 0)
    b4 = np.array(_bc_ends(bc), dtype=np.float64)
    S, Si, lam, Q, L, Bi = np.empty((M, M)), np.empty((M, M)), np.empty(M), np.empty((2, M)), np.empty((M, 2)), np.empty((2, 2))
    ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double)) if a.size else None
    _chk(lib().cheb_helmholtz_line_bc_host(int(P), ptr(b4), ptr(S), ptr(Si), ptr(lam), ptr(Q), ptr(L), ptr(Bi)))
    return S, Si, lam, Q, L, Bi


def helmholtz_line_box(P, bc, s):
    """helmholtz_line_bc for a direction of scale s = 2 / length (cheb_helmholtz_line_box_host): the line of the ends
    (alpha, beta s) with lam and L times s^2, so that A~ = -s^2 ((DD)_II + (DD)_IB Q) and the ends carry
    alpha u + beta s du/dnu = g.  s = 1 gives helmholtz_line_bc's bits.  Needs no device."""
    import numpy as np
    M = max(int(P) - 2, 0)
    b4 = np.array(_bc_ends(bc), dtype=np.float64)
    S, Si, lam, Q, L, Bi = np.empty((M, M)), np.empty((M, M)), np.empty(M), np.empty((2, M)), np.empty((M, 2)), np.empty((2, 2))
    ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double)) if a.size else None
    _chk(lib().cheb_helmholtz_line_box_host(int(P), ptr(b4), float(s), ptr(S), ptr(Si), ptr(lam), ptr(Q), ptr(L), ptr(Bi)))
    return S, Si, lam, Q, L, Bi


def _scale_array(scale, d):
    """(numpy array or None, tuple or None) of a per-direction scale."""
    import numpy as np
    if scale is None:
        return None, None
    sc = np.ascontiguousarray(scale, dtype=np.float64)
    if sc.shape != (d,):
        raise ValueError("scale: expected %d values, got shape %r" % (d, sc.shape))
    return sc, tuple(float(v) for v in sc)


class HelmholtzSolver(_FdmSteps, _Handle):
    """u = (sigma I + A)^-1 f with A the EllipticOp operator at eta == 1 (zero Dirichlet values) by fast diagonalisation
    (cheb_helmholtz_*): `nfields` stacked interior fields of the grid `dims` per call; `size` values.  Usable as the M of
    Fgmres.solve.

    bc (None: Dirichlet on every face, today's solver): one entry per direction, either one spec for both ends or a pair
    (spec at index 0, spec at index n-1); a spec is "dirichlet", "neumann" or (alpha, beta) for alpha u + beta du/dnu = g,
    du/dnu outward.  Such a solver also has solve_full (full-grid output from interior f and boundary data g), full_size,
    boundary_size and singular (sigma = 0 with Neumann everywhere: the constant-like zero mode is dropped).

    scale (needs bc; None: the cube, today's handle): scale[k] = 2 / L_k of a box; the solver inverts sigma - sum_k scale_k^2 d_k^2
    and beta multiplies the physical normal derivative, alpha u + beta scale_k du/dnu = g (cheb_helmholtz_create_box).

    A bc entry "periodic" makes the whole direction periodic (cheb_helmholtz_create_basis): dims[k] unknowns on the
    nodes fourier_nodes(dims[k]), 2 <= dims[k] <= 256, period 2 / scale[k], no faces and no entries in g.  The arrays of solve are
    then row-major over dims[k] (periodic) or dims[k] - 2 (wall) unknowns per direction; `periodic` holds the flags.  singular is
    true for sigma = 0 with every direction periodic or Neumann / Neumann: every product of the directions' zero-eigenvalue modes is
    dropped -- the constants and, on a periodic direction of even extent, the Nyquist vector (-1)^j.  With every direction periodic
    boundary_size is 0 and g must be None."""
    _destroy = "cheb_helmholtz_destroy"

    def __init__(self, dims, sigma=0.0, nfields=1, bc=None, scale=None):
        self.dims = tuple(int(d) for d in dims)
        self.sigma = float(sigma)
        self.nfields = int(nfields)
        self.bc = None
        self.periodic = (False,) * len(self.dims)
        if scale is not None and bc is None:
            raise ValueError("scale needs bc: the box solve is a boundary-condition handle")
        sc, self.scale = _scale_array(scale, len(self.dims))
        h = C.c_void_p()
        if bc is None:
            _chk(lib().cheb_helmholtz_create(len(self.dims), _ints(self.dims), self.sigma, self.nfields, C.byref(h)))
        else:
            d = len(self.dims)
            self.periodic, b, self.bc = bc_split(bc, d)
            # (no periodic direction and no scale: cheb_helmholtz_create_bc's handle; no periodic direction: cheb_helmholtz_create_box's)
            _chk(lib().cheb_helmholtz_create_basis(d, _ints(self.dims), _ints([int(p) for p in self.periodic]), (C.c_double * len(b))(*b),
                                                   None if sc is None else _np_dp(sc), self.sigma, self.nfields, C.byref(h)))
            self.full_size = lib().cheb_helmholtz_full_size(h)
            self.boundary_size = lib().cheb_helmholtz_boundary_size(h)
            self.singular = bool(lib().cheb_helmholtz_singular(h))
        self._h = h
        self.size = lib().cheb_helmholtz_size(h)

    def _fdpc(self):
        return lib().cheb_helmholtz_fdpc(self._h)

    def _nstep(self):
        return self.size

    def solve(self, f, u):
        """Asynchronous on torch's current stream; u may be f.  With bc: the interior problem with zero boundary data."""
        _chk(lib().cheb_helmholtz_solve(self._h, _dev_ptr(f, self.size), _dev_ptr(u, self.size), _stream()))
        return u

    def solve_full(self, f, g, u):
        """With bc: f (size interior values), g (boundary_size compact boundary values in row-major node order, or None: zero
        data) -> u (full_size full-grid values, boundary included).  u may not alias f or g.  Asynchronous on torch's current
        stream."""
        import torch
        if self.bc is None:
            raise ValueError("solve_full needs a solver made with bc")
        for name, t, n in (("f", f, self.size), ("g", g, self.boundary_size), ("u", u, self.full_size)):
            if t is None and name == "g":
                continue
            if name == "g" and n == 0:
                raise ChebhipError(4, "g given, but every direction is periodic: there is no boundary data to lift")
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float64 or not t.is_contiguous():
                raise ValueError("%s must be a contiguous float64 device tensor" % name)
            if t.numel() != n:
                raise ValueError("%s has %d elements, expected %d" % (name, t.numel(), n))
        _chk(lib().cheb_helmholtz_solve_bc(self._h, f.data_ptr(), None if g is None else g.data_ptr(), u.data_ptr(), _stream()))
        return u


class VarHelmholtz(_Handle):
    """y = c x - sum_k scale_k^2 d_k( kappa d_k W ) at the unknown nodes, W the full-grid extension of the unknowns x by the faces'
    conditions (cheb_varhelm_*), and the solve of c u - div(kappa grad u) = f by FGMRES with the direct solve
    H(sigma_p)^-1 (r / kappa) as its right preconditioner.  dims, nfields (1..16), bc ("periodic" entries included) and scale are
    HelmholtzSolver's, as are the unknown layout (interior nodes of a wall direction, all nodes of a periodic one, row-major, fields
    stacked), the compact boundary layout of g and `size`, `full_size`, `boundary_size`.

    The faces carry alpha u + beta scale_k du/dnu = g WITHOUT kappa: for Neumann data of the flux kappa du/dnu divide g by kappa at
    the face first.  kappa is one full-grid field (finite, > 0, read at face nodes too) shared by the stacked fields; c a scalar >= 0
    or one full-grid field >= 0.  Usable as the A (entry "mult") and the M (m_entry="precond") of Fgmres.solve."""
    _destroy = "cheb_varhelm_destroy"

    def __init__(self, dims, nfields=1, bc=None, scale=None):
        self.dims = tuple(int(d) for d in dims)
        self.nfields = int(nfields)
        d = len(self.dims)
        self.periodic, b, self.bc = bc_split(["dirichlet"] * d if bc is None else bc, d)
        sc, self.scale = _scale_array(scale, d)
        h = C.c_void_p()
        _chk(lib().cheb_varhelm_create(d, _ints(self.dims), _ints([int(p) for p in self.periodic]), (C.c_double * len(b))(*b),
                                       None if sc is None else _np_dp(sc), self.nfields, C.byref(h)))
        self._h = h
        self.size = lib().cheb_varhelm_size(h)
        self.full_size = lib().cheb_varhelm_full_size(h)
        self.boundary_size = lib().cheb_varhelm_boundary_size(h)
        self.nodes = self.full_size // self.nfields
        self.iterations, self.residual_norm, self.reason = 0, 0.0, 0

    def _vec(self, name, t, n, optional=False):
        import torch
        if t is None and optional:
            return None
        if name == "g" and n == 0:
            raise ChebhipError(4, "g given, but every direction is periodic: there is no boundary data to lift")
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float64 or not t.is_contiguous():
            raise ValueError("%s must be a contiguous float64 device tensor" % name)
        if t.numel() != n:
            raise ValueError("%s has %d elements, expected %d" % (name, t.numel(), n))
        return t.data_ptr()

    def set_coefficients(self, kappa, c=0.0):
        """Copies kappa (a full-grid field) and c (a scalar or a full-grid field) into the handle; synchronises.  Raises ChebhipError
        (code 4) where kappa is not finite and > 0 or c is negative or not finite; the handle then keeps what it had."""
        import torch
        cf = isinstance(c, torch.Tensor)
        _chk(lib().cheb_varhelm_set_coefficients(self._h, self._vec("kappa", kappa, self.nodes), self._vec("c", c, self.nodes) if cf else None,
                                                 0.0 if cf else float(c), _stream()))

    def set_tensor(self, K, c=0.0, vel=None):
        """The tensor mode (cheb_varhelm_set_tensor; 2-D and 3-D): the operator becomes
        c u + vel . grad u - div(K grad u).  K: the d (d + 1) / 2 full-grid fields of a symmetric positive definite tensor, stacked
        in the order tensor_order(d) (diagonal first, then the upper triangle row-major); vel: d stacked full-grid fields or None;
        c as in set_coefficients.  Synchronises.  Raises ChebhipError (code 4) for another d, where K is not finite and positive
        definite at some node, vel is not finite or c is negative or not finite; the handle then keeps what it had.  precond
        becomes H(sigma_p)^-1 (r / kbar) with kbar = trace(K) / d; set_coefficients returns the handle to the scalar mode."""
        import torch
        d = len(self.dims)
        cf = isinstance(c, torch.Tensor)
        _chk(lib().cheb_varhelm_set_tensor(self._h, self._vec("K", K, len(tensor_order(d)) * self.nodes),
                                           self._vec("vel", vel, d * self.nodes, True), self._vec("c", c, self.nodes) if cf else None,
                                           0.0 if cf else float(c), _stream()))

    mode = property(lambda self: lib().cheb_varhelm_mode(self._h), doc="0: no coefficients yet, 1: scalar (set_coefficients), 2: tensor (set_tensor)")
    sigma = property(lambda self: lib().cheb_varhelm_sigma(self._h))
    singular = property(lambda self: bool(lib().cheb_varhelm_singular(self._h) == 1))

    def work_bytes(self):
        return lib().cheb_varhelm_work_bytes(self._h)

    def mult(self, x, out):
        """out = the linear operator (zero boundary data) of x.  Asynchronous on torch's current stream; out may not overlap x."""
        _chk(lib().cheb_varhelm_mult(self._h, self._vec("x", x, self.size), self._vec("out", out, self.size), _stream()))
        return out

    def residual(self, x, f, g, out):
        """out = f - (the operator with boundary data g)(x); g None: zero data.  This is what solve lifts the data with."""
        _chk(lib().cheb_varhelm_residual(self._h, self._vec("x", x, self.size), self._vec("f", f, self.size),
                                         self._vec("g", g, self.boundary_size, True), self._vec("out", out, self.size), _stream()))
        return out

    def precond(self, r, z):
        """z = H(sigma_p)^-1 (r / kappa): the solve's right preconditioner."""
        _chk(lib().cheb_varhelm_precond(self._h, self._vec("r", r, self.size), self._vec("z", z, self.size), _stream()))
        return z

    def solve(self, f, g=None, u_full=None, x0=None, rtol=1e-8, atol=0.0, max_it=200, restart=30):
        """The unknowns x of (operator at g) x = f, by one library call; u_full (full_size values) receives the full grid.  x0: the
        initial guess (it is not overwritten).  Afterwards iterations, residual_norm (Fgmres's `residual`; the name is the method's
        here) and reason as on Fgmres.  A singular problem (c == 0
        and every direction periodic or Neumann / Neumann) raises ChebhipError (code 4)."""
        return self._solve(lib().cheb_varhelm_solve, f, g, u_full, x0, rtol, atol, max_it, restart)

    def _solve(self, entry, f, g, u_full, x0, rtol, atol, max_it, restart):
        import torch
        fp = self._vec("f", f, self.size)
        x = torch.zeros_like(f) if x0 is None else None
        if x is None:
            self._vec("x0", x0, self.size)
            x = x0.clone()
        try:
            _chk(entry(self._h, fp, self._vec("g", g, self.boundary_size, True), x.data_ptr(), 0 if x0 is None else 1,
                       self._vec("u_full", u_full, self.full_size, True), float(rtol), float(atol), int(max_it), int(restart), _stream()))
        finally:
            self.iterations = lib().cheb_varhelm_iterations(self._h)
            self.residual_norm = lib().cheb_varhelm_last_residual(self._h)
            self.reason = lib().cheb_varhelm_reason(self._h)
        return x

    def solve_deflated(self, f, g=None, u_full=None, x0=None, rtol=1e-8, atol=0.0, max_it=200, restart=30):
        """solve for a singular problem: the x with N^T x = 0 and Pi (b - A x) = 0, N the `null_count` null vectors of
        +-1 (`null_space()`), Pi = I - N N^T / G per field, b = residual(0, f, g).  What is left of b - A x is N lambda: `defect`.
        iterations, residual_norm and reason are those of the projected system, |Pi (b - A x)| against rtol |Pi b|.  On a
        nonsingular handle this is solve, bit for bit.  More than three even periodic directions raise ChebhipError (code 4)."""
        return self._solve(lib().cheb_varhelm_solve_deflated, f, g, u_full, x0, rtol, atol, max_it, restart)

    null_count = property(lambda self: lib().cheb_varhelm_null_count(self._h))

    @property
    def defect(self):
        """lambda = N^T (b - A x) / G of the last solve_deflated of a singular problem: a (nfields, q) NumPy array.  Synchronises."""
        import numpy as np
        q = self.null_count
        out = np.zeros((self.nfields, max(q, 0)))
        if q > 0:
            _chk(lib().cheb_varhelm_defect(self._h, _np_dp(out)))
        return out

    def null_space(self):
        """The null vectors of the geometry with every wall Neumann / Neumann and c == 0: a host array (q, *unknown dims) of +-1."""
        return null_space(self.dims, self.periodic)

    def remove_null(self, x, out=None):
        """out = Pi x (out None: in place); the identity on a nonsingular handle."""
        out = x if out is None else out
        _chk(lib().cheb_varhelm_remove_null(self._h, self._vec("x", x, self.size), self._vec("out", out, self.size), _stream()))
        return out

    def mult_deflated(self, x, out):
        """out = Pi mult(x): the operator of solve_deflated (a_entry="mult_deflated" of Fgmres.solve)."""
        _chk(lib().cheb_varhelm_apply_deflated(self._h, self._vec("x", x, self.size), self._vec("out", out, self.size), _stream()))
        return out

    def precond_deflated(self, r, z):
        """z = Pi precond(r): the right preconditioner of solve_deflated (m_entry="precond_deflated")."""
        _chk(lib().cheb_varhelm_precond_deflated(self._h, self._vec("r", r, self.size), self._vec("z", z, self.size), _stream()))
        return z


def tensor_order(d):
    """The index pairs (j, k) of the fields VarHelmholtz.set_tensor takes, in its order: the diagonal, then the upper triangle
    row-major -- d = 3: 00 11 22 01 02 12."""
    d = int(d)
    return [(j, j) for j in range(d)] + [(j, k) for j in range(d) for k in range(j + 1, d)]


def null_signs(dims, periodic):
    """cheb_varhelm_null_signs_host: per null vector the bit mask of the directions in which it alternates (host only)."""
    d = len(dims)
    flags = (C.c_int * 8)()
    q = lib().cheb_varhelm_null_signs_host(d, _ints([int(p) for p in dims]), _ints([int(bool(p)) for p in periodic]), flags)
    if q < 0:
        _chk(-q)
    return [int(flags[j]) for j in range(q)]


def null_space(dims, periodic):
    """The null vectors of c == 0, every direction periodic or Neumann / Neumann: (q, *unknown dims) of +-1, from null_signs."""
    import numpy as np
    M = [int(p) if per else int(p) - 2 for p, per in zip(dims, periodic)]
    out = []
    for mask in null_signs(dims, periodic):
        z = np.ones(M)
        for k, m in enumerate(M):
            if mask >> k & 1:
                z = z * ((-1.0) ** np.arange(m)).reshape([-1 if a == k else 1 for a in range(len(M))])
        out.append(z)
    return np.stack(out)


OPFUN_KINDS = {"one": 0, "inv": 1, "res": 2, "exp": 3, "phi1": 4, "phi2": 5, "phi3": 6, "pow": 7}           # CHEB_OPFUN_*


def _opfun_kind(kind):
    if isinstance(kind, str):
        if kind.lower() not in OPFUN_KINDS:
            raise ValueError("unknown kind %r: one of %s" % (kind, ", ".join(OPFUN_KINDS)))
        return OPFUN_KINDS[kind.lower()]
    return int(kind)


def _opfun_terms(terms):
    """(tuples, ctypes array) of a list of (out, in, kind, coef, tau, par)."""
    terms = [tuple(t) for t in terms]
    if any(len(t) != 6 for t in terms):
        raise ValueError("a term is (out, in, kind, coef, tau, par)")
    arr = (OpFunTerm * max(len(terms), 1))()
    for e, (o, i, kind, c, ta, pa) in zip(arr, terms):
        e.out, e.inp, e.kind, e.coef, e.tau, e.par = int(o), int(i), _opfun_kind(kind), float(c), float(ta), float(pa)
    return terms, arr


def opfun_check_terms(nin, nout, terms):
    """ChebOpFun.set_terms' checks for a handle of nin inputs and nout outputs, without one (cheb_opfun_check_terms): raises
    ChebhipError as set_terms would.  Needs no device."""
    terms, arr = _opfun_terms(terms)
    _chk(lib().cheb_opfun_check_terms(int(nin), int(nout), len(terms), arr))


def opfun_weight(kind, tau, par, s):
    """f(s) of one kind of ChebOpFun for host values (cheb_opfun_weights_host): z = -tau s and f in long double, rounded once.
    s: a number or a numpy array; the result has its shape.  Needs no device."""
    import numpy as np
    a = np.ascontiguousarray(s, dtype=np.float64)
    w = np.empty_like(a)
    ptr = lambda v: v.ctypes.data_as(C.POINTER(C.c_double)) if v.size else None
    _chk(lib().cheb_opfun_weights_host(_opfun_kind(kind), float(tau), float(par), a.size, ptr(a), ptr(w)))
    return w if np.ndim(s) else float(w.reshape(-1)[0])


def opfun_eval(kind, tau, par, s_dev, out=None):
    """The same on the device, by the device functions ChebOpFun's kernel runs (cheb_opfun_eval): s_dev a contiguous float64 device
    tensor; returns a tensor of its shape.  Asynchronous on torch's current stream."""
    import torch
    if out is None:
        out = torch.empty_like(s_dev)
    n = s_dev.numel()
    _chk(lib().cheb_opfun_eval(_opfun_kind(kind), float(tau), float(par), _dev_ptr(s_dev, n) if n else None, n,
                               _dev_ptr(out, n) if n else None, _stream()))
    return out


class ChebOpFun(_Handle):
    """Functions of the Helmholtz operator B = sigma - sum_k scale_k^2 d_k^2 of HelmholtzSolver (same dims, bc, scale, sigma;
    cheb_opfun_*): one call maps `nin` stacked interior fields to `nout`,
        y_o = sum_{terms (o, i, kind, coef, tau, par)} coef f_kind(B) x_i,
    by the solver's line transforms around ONE pointwise kernel in mode space, whatever the number of terms (at most 32).  Kinds,
    with s an eigenvalue of B: "one" 1, "inv" 1/s, "res" 1/(par + tau s), "exp" e^(-tau s), "phi1".."phi3" phi_k(-tau s) (the
    functions of exponential integrators), "pow" s^par.  A mode with s == 0 (`singular`: sigma = 0, Neumann everywhere) gets 0 from
    inv and pow, 1/k! from phi_k, 1 from exp.  Terms of an output are added in table order; the same input gives the same bits.

    A bc entry "periodic" makes the whole direction periodic, as for HelmholtzSolver (cheb_opfun_create_basis): the
    fields are then in the solver's unknown layout, dims[k] (periodic) or dims[k] - 2 (wall) values per direction; `periodic` holds
    the flags.  The rule for s == 0 is the one above, unchanged: `singular` is sigma = 0 with every direction periodic or Neumann /
    Neumann, and EVERY product of the directions' zero-eigenvalue modes -- the constants and, on a periodic direction of even
    extent, the Nyquist vector (-1)^j -- has s == 0 exactly.  apply_full works on every handle made with bc; with every direction
    periodic the unknown layout is the full grid and it equals apply."""
    _destroy = "cheb_opfun_destroy"

    def __init__(self, dims, nin=1, nout=None, sigma=0.0, bc=None, scale=None):
        self.dims = tuple(int(d) for d in dims)
        self.nin = int(nin)
        self.nout = self.nin if nout is None else int(nout)
        self.sigma = float(sigma)
        d = len(self.dims)
        if scale is not None and bc is None:
            raise ValueError("scale needs bc: the box is a boundary-condition handle")
        sc, self.scale = _scale_array(scale, d)
        self.periodic, b, ends = (False,) * d, None, None
        if bc is not None:
            self.periodic, b, ends = bc_split(bc, d)
        self.bc = ends                           # per direction the four end values, None where it is periodic
        h = C.c_void_p()
        if any(self.periodic):
            _chk(lib().cheb_opfun_create_basis(d, _ints(self.dims), _ints([int(p) for p in self.periodic]), (C.c_double * len(b))(*b),
                                               None if sc is None else _np_dp(sc), self.sigma, self.nin, self.nout, C.byref(h)))
        else:
            _chk(lib().cheb_opfun_create(d, _ints(self.dims), None if b is None else (C.c_double * len(b))(*b),
                                         None if sc is None else _np_dp(sc), self.sigma, self.nin, self.nout, C.byref(h)))
        self._h = h
        self.size, self.out_size, self.full_size = (lib().cheb_opfun_size(h, w) for w in range(3))
        self.singular = bool(lib().cheb_opfun_singular(h))
        self.terms = ()

    def set_terms(self, terms, tau=0.0, par=0.0, coef=1.0):
        """terms: tuples (out, in, kind, coef, tau, par), or one kind name: that function on every field (nin == nout) with the
        keyword tau / par / coef.  Host work only; an apply queued earlier keeps the table it was issued with."""
        if isinstance(terms, str):
            if self.nin != self.nout:
                raise ValueError("the shorthand needs nin == nout")
            terms = [(f, f, terms, coef, tau, par) for f in range(self.nin)]
        terms, arr = _opfun_terms(terms)
        _chk(lib().cheb_opfun_set_terms(self._h, len(terms), arr))
        self.terms = tuple(terms)

    def _check(self, name, t, n):
        import torch
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float64 or not t.is_contiguous():
            raise ValueError("%s must be a contiguous float64 device tensor" % name)
        if t.numel() != n:
            raise ValueError("%s has %d elements, expected %d" % (name, t.numel(), n))

    def apply(self, x, out=None):
        """x: `size` = nin * G values; out (allocated if None): `out_size` = nout * G values, may be x when nin == nout.
        Asynchronous on torch's current stream."""
        import torch
        self._check("x", x, self.size)
        if out is None:
            out = torch.empty(self.out_size, dtype=torch.float64, device=x.device)
        self._check("out", out, self.out_size)
        _chk(lib().cheb_opfun_apply(self._h, x.data_ptr(), out.data_ptr(), _stream()))
        return out

    def apply_full(self, x, out=None):
        """With bc: the same, each output as a full-grid field (`full_size` = nout * N values) whose boundary values are those of
        the homogeneous conditions (u_B = Q u_I)."""
        import torch
        if self.bc is None:
            raise ValueError("apply_full needs a handle made with bc")
        self._check("x", x, self.size)
        if out is None:
            out = torch.empty(self.full_size, dtype=torch.float64, device=x.device)
        self._check("out", out, self.full_size)
        _chk(lib().cheb_opfun_apply_full(self._h, x.data_ptr(), out.data_ptr(), _stream()))
        return out


FACES = {"wall": 0, "open": 1}           # CHEB_FACE_*


def _face_codes(bc, d):
    """The 2 d ints of cheb_project_create from one entry per direction: "wall", "open" or a pair (index 0, index n - 1).  A
    direction that is "periodic" (_bc_periodic: as a whole) has no faces; its two codes are "wall" placeholders that are not read."""
    if bc is None:
        return None
    if isinstance(bc, str) or len(bc) != d:
        raise ValueError("bc needs one entry per direction (%d)" % d)
    out = []
    for entry in bc:
        if _bc_periodic(entry):
            out += [FACES["wall"]] * 2
            continue
        pair = (entry, entry) if isinstance(entry, str) else tuple(entry) if isinstance(entry, (tuple, list)) else ()
        if len(pair) != 2 or any(not isinstance(e, str) or e.lower() not in FACES for e in pair):
            raise ValueError("a direction's faces are 'wall', 'open' or a pair of them, got %r" % (entry,))
        out += [FACES[e.lower()] for e in pair]
    return out


def project_faces(dims, periodic=None):
    """Per compact boundary node (row-major boundary order) 2 k + end of the face whose condition the node takes: the highest
    direction k in which it is an end node, end 0 = index 0 (cheb_project_faces_host).  An int32 numpy array; needs no device.
    periodic (one flag per direction, cheb_project_faces_basis_host): a flagged direction has no end nodes; the boundary nodes are
    the end nodes of the other directions and the highest of those names the face."""
    import numpy as np
    dims = tuple(int(d) for d in dims)
    per = _periodic_flags(periodic, len(dims))
    ok = all(n >= (2 if p else 3) for n, p in zip(dims, per))
    nb = int(np.prod(dims)) - int(np.prod([n if p else n - 2 for n, p in zip(dims, per)])) if ok else 0
    f = np.empty(max(nb, 0), dtype=np.int32)
    ptr = f.ctypes.data_as(C.POINTER(C.c_int)) if f.size else None
    if periodic is None:
        _chk(lib().cheb_project_faces_host(len(dims), _ints(dims), ptr))
    else:
        _chk(lib().cheb_project_faces_basis_host(len(dims), _ints(dims), _ints([int(p) for p in per]), ptr))
    return f


class ChebProject(_Handle):
    """Projection of velocity fields onto discretely divergence-free ones on the box of `dims` and `scale` (scale[k] = 2 / L_k;
    cheb_project_*): out_k = u_k - scale_k d_k phi, phi from one direct solve.  bc: per direction "wall" (the normal
    velocity of the result is `flux`, default 0), "open" (phi = 0, an outflow face) or a pair for the two ends; None: walls.  A
    velocity is d stacked full-grid fields (ChebGrad.div's layout), `nvec` of them per call, nvec * d <= 16.

    With an open face div(out) = 0 at the interior nodes to rounding.  With walls only (`singular`) the solver drops the
    constant-like mode and div(out) is one constant c(u) there: small for resolved fields, O(1) for noise.  An edge or corner node
    meets the wall condition of its highest end direction only.  Asynchronous on torch's current stream; the same input gives the
    same bits.

    A bc entry "periodic" covers a whole direction (cheb_project_create_basis): 2 <= dims[k] <= 256 nodes
    fourier_nodes(dims[k]), period 2 / scale[k], no faces; `periodic` holds the flags.  The unknowns of phi's problem are then the
    nodes that are interior in every WALL direction (interior_size) and boundary_size counts the end nodes of the wall directions
    (project_faces(dims, periodic)).  The divergence of the result, ChebGrad(dims, scale, periodic).div(out):
      every direction periodic -- zero to rounding at EVERY node, although the handle is `singular`: the range of D_F holds neither
        the constant nor the Nyquist vector, so div u has no component along any dropped mode.  boundary_size is 0 and flux must
        be None;
      an open face -- zero to rounding at the unknown nodes;
      walls in the wall directions, the rest periodic (a channel) -- `singular`: at the unknown nodes it is free along the dropped
        modes, which are constant along the wall directions and, per periodic direction, the constant or -- for an EVEN extent --
        the Nyquist vector (-1)^j: one constant as above when the periodic extents are odd, 2^e coefficients with e even ones
        (the wall-normal velocity may carry a Nyquist component no potential removes; small for resolved fields).

    variable=True (cheb_project_create_variable): out_k = u_k - kappa scale_k d_k phi with kappa = 1 / rho > 0 one
    full-grid field shared by the vectors (set_inverse_density, before the first project), phi from
    sum_k scale_k^2 d_k(kappa d_k phi) = div u by VarHelmholtz.solve_deflated (FGMRES: project's warm, rtol, atol, max_it and
    restart; afterwards iterations, residual_norm, reason and defect).  The normal velocity of the result at a wall node is
    `flux` as above.  At the unknown nodes div(out) is the negative of the solve's residual: with an open face it is at the
    solve's TOLERANCE, not at rounding; with walls and periodic directions only it lies, up to that tolerance, in the span of the
    null vectors (null_count of them, coefficients -defect)."""
    _destroy = "cheb_project_destroy"

    def __init__(self, dims, nvec=1, bc=None, scale=None, variable=False):
        self.dims = tuple(int(d) for d in dims)
        self.d = len(self.dims)
        self.nvec = int(nvec)
        faces = _face_codes(bc, self.d)
        self.faces = None if faces is None else tuple(faces)
        self.periodic = (False,) * self.d if faces is None else tuple(_bc_periodic(entry) for entry in bc)
        sc, self.scale = _scale_array(scale, self.d)
        h = C.c_void_p()
        self.variable = bool(variable)
        self.iterations, self.residual_norm, self.reason = 0, 0.0, 0
        if self.variable:
            _chk(lib().cheb_project_create_variable(self.d, _ints(self.dims), _ints([int(p) for p in self.periodic]) if any(self.periodic) else None,
                                                    None if faces is None else _ints(faces), None if sc is None else _np_dp(sc), self.nvec, C.byref(h)))
        elif any(self.periodic):
            _chk(lib().cheb_project_create_basis(self.d, _ints(self.dims), _ints([int(p) for p in self.periodic]), _ints(faces),
                                                 None if sc is None else _np_dp(sc), self.nvec, C.byref(h)))
        else:
            _chk(lib().cheb_project_create(self.d, _ints(self.dims), None if faces is None else _ints(faces),
                                           None if sc is None else _np_dp(sc), self.nvec, C.byref(h)))
        self._h = h
        self.size, self.interior_size, self.boundary_size = (lib().cheb_project_size(h, w) for w in range(3))
        self.singular = bool(lib().cheb_project_singular(h))

    def set_inverse_density(self, kappa):
        """kappa = 1 / rho at every node (a device tensor of `size` values, finite and > 0), for a variable=True handle; synchronises.
        Refusals as VarHelmholtz.set_coefficients: the handle then keeps what it had."""
        _chk(lib().cheb_project_set_inverse_density(self._h, _dev_ptr(kappa, self.size), _stream()))

    def _varhelm(self):
        return lib().cheb_project_varhelm(self._h)

    null_count = property(lambda self: lib().cheb_varhelm_null_count(self._varhelm()) if self.variable else 0)

    @property
    def defect(self):
        """VarHelmholtz.defect of the last project of a variable=True handle without an open face: (nvec, null_count)."""
        import numpy as np
        q = self.null_count
        out = np.zeros((self.nvec, max(q, 0)))
        if q > 0:
            _chk(lib().cheb_varhelm_defect(self._varhelm(), _np_dp(out)))
        return out

    def project(self, u, out=None, phi=None, flux=None, warm=False, rtol=1e-8, atol=0.0, max_it=200, restart=30):
        """u: (nvec * d, *dims); flux: nvec * boundary_size prescribed outward normal velocities at the boundary nodes (compact,
        row-major) or None; phi: nvec * size values, receives the potential (allocated if None); out (allocated if None) may be u.
        Returns out.  warm .. restart: a variable=True handle's solve (warm: from the unknowns of the call before)."""
        import torch
        nu = self.nvec * self.d * self.size
        if flux is not None and self.boundary_size == 0:
            raise ChebhipError(4, "flux given, but every direction is periodic: there is no wall to prescribe it on")
        if out is None:
            out = torch.empty((self.nvec * self.d,) + self.dims, dtype=torch.float64, device=u.device)
        if phi is None:
            phi = torch.empty((self.nvec,) + self.dims, dtype=torch.float64, device=u.device)
        if self.variable:
            try:
                _chk(lib().cheb_project_apply_variable(self._h, _dev_ptr(u, nu), None if flux is None else _dev_ptr(flux, self.nvec * self.boundary_size),
                                                       _dev_ptr(phi, self.nvec * self.size), _dev_ptr(out, nu), int(bool(warm)), float(rtol), float(atol),
                                                       int(max_it), int(restart), _stream()))
            finally:
                vh = self._varhelm()
                self.iterations, self.reason = lib().cheb_varhelm_iterations(vh), lib().cheb_varhelm_reason(vh)
                self.residual_norm = lib().cheb_varhelm_last_residual(vh)
            return out
        _chk(lib().cheb_project_apply(self._h, _dev_ptr(u, nu), None if flux is None else _dev_ptr(flux, self.nvec * self.boundary_size),
                                      _dev_ptr(phi, self.nvec * self.size), _dev_ptr(out, nu), _stream()))
        return out


class Lap1dPlan(_Handle):
    """y = acc + alpha * D_tr D_tr x on an interior-layout tensor (cheb_plan_create_trimmed /
    cheb_apply_lap1d): one direction of the linear MatMult_Elliptic, usable on slabs and pencils."""
    _destroy = "cheb_plan_destroy"

    def __init__(self, dims, tr):
        self.dims = tuple(int(d) for d in dims)
        self.tr = int(tr)
        h = C.c_void_p()
        _chk(lib().cheb_plan_create_trimmed(len(self.dims), self.tr, _ints(self.dims), C.byref(h)))
        self._h = h
        self.size = lib().cheb_plan_size(h)

    def apply(self, x, y, acc=None, alpha=1.0):
        ap = _dev_ptr(acc, self.size) if acc is not None else None
        _chk(lib().cheb_apply_lap1d(self._h, _dev_ptr(x, self.size), ap, alpha, _dev_ptr(y, self.size), _stream()))
        return y


def slab_pack(slab, buf, m0, M1, R, c1):
    """buf <- slab (m0, M1, R) reordered into per-peer column blocks (cheb_slab_pack)."""
    n = int(m0) * int(M1) * int(R)
    cs = (C.c_long * len(c1))(*[int(v) for v in c1])
    _chk(lib().cheb_slab_pack(m0, M1, R, len(c1) - 1, cs, _dev_ptr(slab, n), _dev_ptr(buf, n), _stream()))
    return buf


def slab_unpack_add(buf, acc, out, m0, M1, R, c1, alpha=1.0):
    """out = acc + alpha * slab-ordered(buf) (cheb_slab_unpack_add); acc may be None."""
    n = int(m0) * int(M1) * int(R)
    cs = (C.c_long * len(c1))(*[int(v) for v in c1])
    ap = _dev_ptr(acc, n) if acc is not None else None
    _chk(lib().cheb_slab_unpack_add(m0, M1, R, len(c1) - 1, cs, _dev_ptr(buf, n), ap, alpha, _dev_ptr(out, n), _stream()))
    return out


DIM0_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p)


def _dim0_trampoline(dim0):
    def tramp(ctx, kind, nf, inp, acc, alpha, out, stream):
        try:
            return int(dim0(kind, nf, inp, acc, alpha, out, stream) or 0)
        except Exception:                      # never unwind through the C frames
            import traceback
            traceback.print_exc()
            return 5
    return DIM0_FN(tramp)


class EllipticOp(_Handle):
    """The scalar elliptic MatShell (MatCreate_Elliptic, elliptic.C:250-293)."""
    _destroy = "ell_op_destroy"

    def __init__(self, dims, slab=None, dim0=None, handle=None):
        """slab = (lo, hi): the planes [lo, hi) of grid dimension 0 (ell_op_create_slab); dim0 is then the Python
        callable (kind, nfields, in_ptr, acc_ptr_or_None, alpha, out_ptr, stream) -> int doing the sweeps along dim 0.
        handle: wrap an ell_op owned by someone else (chebhip_dist_ell_op)."""
        self.dims = tuple(int(d) for d in dims)
        h = C.c_void_p()
        self._owned = handle is None
        if handle is not None:
            h = C.c_void_p(handle)
        elif slab is None:
            _chk(lib().ell_op_create(len(self.dims), _ints(self.dims), C.byref(h)))
        else:
            self._cb = _dim0_trampoline(dim0)           # keep the trampoline alive as long as the handle
            _chk(lib().ell_op_create_slab(len(self.dims), _ints(self.dims), int(slab[0]), int(slab[1]),
                                          C.cast(self._cb, C.c_void_p), None, C.byref(h)))
        self._h = h
        self.local_size = lib().ell_op_local_size(h)
        self.global_size = lib().ell_op_global_size(h)
        self.dirichlet_size = lib().ell_op_dirichlet_size(h)

    def mult(self, U, V):
        """MatMult_Elliptic (elliptic.C:297-339) on device tensors of global_size."""
        _chk(lib().ell_op_mult(self._h, _dev_ptr(U, self.global_size), _dev_ptr(V, self.global_size), _stream()))
        return V

    def pencil_sweep(self, ncol, inp, out):
        _chk(lib().ell_op_pencil_sweep(self._h, ncol, inp.data_ptr(), out.data_ptr(), _stream()))
        return out

    def mult_host(self, U):
        import numpy as np
        U = np.ascontiguousarray(U, dtype=np.float64)
        assert U.size == self.global_size
        V = np.empty_like(U)
        _chk(lib().ell_op_mult_host(self._h, _np_dp(U), _np_dp(V)))
        return V

    def function(self, U, b, rhs, gamma=0.0, exponent=2.0):
        """FormFunction (elliptic.C:481-533) on device tensors; b may be None."""
        bp = _dev_ptr(b, self.global_size) if b is not None else None
        _chk(lib().ell_op_function(self._h, gamma, exponent, _dev_ptr(U, self.global_size), bp,
                                   _dev_ptr(rhs, self.global_size), _stream()))
        return rhs

    def function_host(self, U, b=None, gamma=0.0, exponent=2.0):
        import numpy as np
        U = np.ascontiguousarray(U, dtype=np.float64)
        rhs = np.empty_like(U)
        bp = None
        if b is not None:
            b = np.ascontiguousarray(b, dtype=np.float64)
            bp = _np_dp(b)
        _chk(lib().ell_op_function_host(self._h, gamma, exponent, _np_dp(U), bp, _np_dp(rhs)))
        return rhs

    def set_dirichlet(self, values):
        import numpy as np
        values = np.ascontiguousarray(values, dtype=np.float64)
        assert values.size == self.dirichlet_size
        _chk(lib().ell_op_set_dirichlet(self._h, _np_dp(values)))

    def get_state(self, which):
        import numpy as np
        out = np.empty(self.local_size)
        _chk(lib().ell_op_get_state(self._h, which, _np_dp(out)))
        return out

    def set_state(self, which, values):
        import numpy as np
        values = np.ascontiguousarray(values, dtype=np.float64)
        assert values.size == self.local_size
        _chk(lib().ell_op_set_state(self._h, which, _np_dp(values)))


class StokesOp(_Handle):
    """The Stokes MatShells (StokesCreate, stokes.C:257-344) with -boundary 0.

    mult <-> StokesMatMult (stokes.C:499-519); mult_vv / mult_pv / mult_vp <-> MatVV / MatPV / MatVP
    (:623-676, :557-566, :599-619); function <-> StokesFunction (:680-758)."""
    _destroy = "stokes_op_destroy"

    def __init__(self, dims, slab=None, dim0=None, handle=None):
        """slab = (lo, hi): the planes [lo, hi) of grid dimension 0 (stokes_op_create_slab); dim0 is then the Python
        callable (kind, nfields, in_ptr, acc_ptr_or_None, alpha, out_ptr, stream) -> int doing the work along dim 0.
        handle: wrap a stokes_op owned by someone else (chebhip_dist_stokes_op)."""
        self.dims = tuple(int(d) for d in dims)
        self.d = len(self.dims)
        h = C.c_void_p()
        self._owned = handle is None
        if handle is not None:
            h = C.c_void_p(handle)
        elif slab is None:
            _chk(lib().stokes_op_create(self.d, _ints(self.dims), C.byref(h)))
        else:
            self._cb = _dim0_trampoline(dim0)           # keep the trampoline alive as long as the handle
            _chk(lib().stokes_op_create_slab(self.d, _ints(self.dims), int(slab[0]), int(slab[1]),
                                             C.cast(self._cb, C.c_void_p), None, C.byref(h)))
        self._h = h
        sz = [lib().stokes_op_size(h, w) for w in range(6)]
        self.local_nodes, self.interior_nodes, self.velocity_size, self.pressure_size, self.global_size, self.dirichlet_size = sz

    def set_rheology(self, kind, hardness=1.0, exponent=1.0, regularization=1.0, gamma0=1.0):
        _chk(lib().stokes_op_set_rheology(self._h, kind, hardness, exponent, regularization, gamma0))

    def set_dirichlet(self, values):
        import numpy as np
        values = np.ascontiguousarray(values, dtype=np.float64)
        assert values.size == self.dirichlet_size
        _chk(lib().stokes_op_set_dirichlet(self._h, _np_dp(values)))

    def set_force(self, force):
        import numpy as np
        force = np.ascontiguousarray(force, dtype=np.float64)
        assert force.size == self.global_size
        _chk(lib().stokes_op_set_force(self._h, _np_dp(force)))

    def _call(self, fn, x, nx, y, ny):
        _chk(fn(self._h, _dev_ptr(x, nx), _dev_ptr(y, ny), _stream()))
        return y

    def mult(self, x, y):
        return self._call(lib().stokes_op_mult, x, self.global_size, y, self.global_size)

    def mult_vv(self, v, out):
        return self._call(lib().stokes_op_mult_vv, v, self.velocity_size, out, self.velocity_size)

    def mult_pv(self, v, pout):
        return self._call(lib().stokes_op_mult_pv, v, self.velocity_size, pout, self.pressure_size)

    def mult_vp(self, p, vout):
        return self._call(lib().stokes_op_mult_vp, p, self.pressure_size, vout, self.velocity_size)

    # the same on component-major velocity vectors (component c of interior node n at c * I + n): the layout of the block
    # preconditioners' inner solves
    def mult_vv_cm(self, v, out):
        return self._call(lib().stokes_op_mult_vv_cm, v, self.velocity_size, out, self.velocity_size)

    def mult_pv_cm(self, v, pout):
        return self._call(lib().stokes_op_mult_pv_cm, v, self.velocity_size, pout, self.pressure_size)

    def mult_vp_cm(self, p, vout):
        return self._call(lib().stokes_op_mult_vp_cm, p, self.pressure_size, vout, self.velocity_size)

    def pencil_sweep(self, nfields, ncol, inp, out):
        _chk(lib().stokes_op_pencil_sweep(self._h, nfields, ncol, inp.data_ptr(), out.data_ptr(), _stream()))
        return out

    def pencil_pressure(self, ncol, p_pencil, gp0_pencil):
        _chk(lib().stokes_op_pencil_pressure(self._h, ncol, p_pencil.data_ptr(), gp0_pencil.data_ptr(), _stream()))
        return gp0_pencil

    def mult_schur(self, p, pout, restart=None, rtol=None, atol=1e-50, max_it=10000, inner=None):
        """StokesMatMultSchur (stokes.C:523-535) with the built-in inner GMRES on MatVV (KSP defaults unless given), or with
        `inner`: a callable (b, x) on device velocity tensors that solves VV x = b -- the user's KSPSchurVelocity (stokes.C:531),
        handed to the C entry point as its inner_solve callback exactly as the PETSc adapter does."""
        if restart is not None or rtol is not None:
            _chk(lib().stokes_op_set_inner_solver(self._h, 30 if restart is None else restart, 1e-5 if rtol is None else rtol, atol, max_it))
        cb = None
        if inner is not None:
            n = self.velocity_size

            def tramp(ctx, bp, xp, stream):
                try:
                    inner(device_view(bp, n), device_view(xp, n))
                    return 0
                except Exception:
                    import traceback
                    traceback.print_exc()
                    return 5
            cb = Fgmres.APPLY_FN(tramp)
        _chk(lib().stokes_op_mult_schur(self._h, _dev_ptr(p, self.pressure_size), _dev_ptr(pout, self.pressure_size),
                                        C.cast(cb, C.c_void_p) if cb else None, None, _stream()))
        return pout

    def set_inner_reduce(self, group=None):
        """Slab mode: the built-in inner solve of mult_schur works on distributed velocity vectors."""
        self._red = allreduce_trampoline(group)
        _chk(lib().stokes_op_set_inner_reduce(self._h, C.cast(self._red, C.c_void_p), None))

    @property
    def inner_iterations(self):
        return lib().stokes_op_inner_iterations(self._h)

    def viscosity_range(self):
        """(min, max) of eta after the last `function`: what StokesFunction prints (stokes.C:731-734)."""
        lo, hi = C.c_double(), C.c_double()
        _chk(lib().stokes_op_viscosity_range(self._h, C.byref(lo), C.byref(hi), _stream()))
        return lo.value, hi.value

    def write_vtk(self, state, path):
        """StokesStateView (stokes.C:1821-1894): the -output_vtk dump of a state vector (device tensor)."""
        _chk(lib().stokes_op_write_vtk(self._h, _dev_ptr(state, self.global_size), str(path).encode()))

    def function(self, x, y):
        return self._call(lib().stokes_op_function, x, self.global_size, y, self.global_size)

    def get_state(self, which):
        import numpy as np
        n = self.local_nodes if which < 2 else self.local_nodes * self.d
        out = np.empty(n)
        _chk(lib().stokes_op_get_state(self._h, which, _np_dp(out)))
        return out

    def set_state(self, which, values):
        import numpy as np
        values = np.ascontiguousarray(values, dtype=np.float64)
        n = self.local_nodes if which < 2 else self.local_nodes * self.d
        assert values.size == n
        _chk(lib().stokes_op_set_state(self._h, which, _np_dp(values)))


def timers(enable=None, reset=False):
    """Per-stage device timers of the library (chebhip_timers_*): timers(True) switches them on, timers() returns
    {stage name: (total ms, calls)} for every stage that ran, timers(reset=True) clears the counters."""
    L = lib()
    if enable is not None:
        _chk(L.chebhip_timers_enable(1 if enable else 0))
    if reset:
        _chk(L.chebhip_timers_reset())
    out = {}
    i = 0
    while True:
        name = L.chebhip_stage_name(i).decode()
        if not name:
            break
        ms, calls = C.c_double(), C.c_long()
        _chk(L.chebhip_timers_read(i, C.byref(ms), C.byref(calls)))
        if calls.value:
            out[name] = (ms.value, calls.value)
        i += 1
    return out


class FdPc(_FdmSteps, _Handle):
    """The finite-difference preconditioner of the reference on the device: FormJacobian's matrix P
    (elliptic.C:537-590) for an EllipticOp, MatVVPC (stokes.C:1160-1241) on velocity vectors for a StokesOp.
    `apply` is an approximate solve with P (fast diagonalisation + `sweeps` defect corrections); pass the object as
    the `M` of Fgmres.solve."""
    _destroy = "chebhip_fdpc_destroy"

    def __init__(self, op, sweeps=1, handle=None):
        """handle: a slab-mode handle owned by a slab driver (dist.py: DistStokesC.pc / DistEllipticC.pc) -- borrowed."""
        kind = type(op).__name__
        self._owned = handle is None
        if handle is None:
            h = C.c_void_p()
            _chk((lib().ell_pc_create if kind == "EllipticOp" else lib().stokes_pc_create)(op._h, C.byref(h)))
        else:
            h = handle
        self._h = h
        self._op = op                     # the handle reads the operator's state: keep it alive
        self.n = op.global_size if kind == "EllipticOp" else op.velocity_size
        _chk(lib().chebhip_fdpc_set_sweeps(h, sweeps))

    def update(self):
        """FormJacobian / StokesPCSetUp0: re-assemble from the operator's current eta, deta (gradu)."""
        _chk(lib().chebhip_fdpc_update(self._h, _stream()))

    def mult(self, x, y):
        _chk(lib().chebhip_fdpc_mult(self._h, _dev_ptr(x, self.n), _dev_ptr(y, self.n), _stream()))
        return y

    def apply(self, r, z):
        _chk(lib().chebhip_fdpc_apply(self._h, _dev_ptr(r, self.n), _dev_ptr(z, self.n), _stream()))
        return z

    def apply_cm(self, r, z):
        """MatVVPC solve on component-major velocity vectors (StokesOp.mult_vv_cm), sweeps = 0."""
        _chk(lib().chebhip_fdpc_apply_cm(self._h, _dev_ptr(r, self.n), _dev_ptr(z, self.n), _stream()))
        return z


class SpectralPc(_FdmSteps, _Handle):
    """z = (sigma I + A)^-1 (r / eta) for an EllipticOp (ell_pc_create_spectral): the direct solve of the constant-coefficient
    operator after division by the viscosity.  `update` refreshes eta from the operator's last FormFunction; pass the object as
    the `M` of Fgmres.solve."""
    _destroy = "chebhip_fdpc_destroy"

    def __init__(self, op, sigma=0.0):
        h = C.c_void_p()
        _chk(lib().ell_pc_create_spectral(op._h, float(sigma), C.byref(h)))
        self._h = h
        self._op = op                     # the handle reads the operator's state: keep it alive
        self.n = op.global_size
        self.sigma = float(sigma)

    def update(self):
        _chk(lib().chebhip_fdpc_update(self._h, _stream()))

    def apply(self, r, z):
        _chk(lib().chebhip_fdpc_apply(self._h, _dev_ptr(r, self.n), _dev_ptr(z, self.n), _stream()))
        return z


class StokesSaddlePc(_Handle):
    """StokesPCApply0..3 (stokes.C:1714-1817) on the device: block LU / upper / diagonal / lower preconditioners of the
    saddle-point system, with the inner solves KSPVelocity, KSPSchur, KSPSchurVelocity (stokes.C:328-341).
    Pass the object as the `M` of Fgmres.solve around StokesOp.mult."""
    _destroy = "stokes_saddle_destroy"

    def __init__(self, op, saddle_type=0, vel=(4, 1e-5), schur=(3, 1e-5), svel=(0, 1e-5), pc_sweeps=0, schur_jacobi=True, slab=None):
        """schur_jacobi: KSPSchur's PCJACOBI with 1/eta on the diagonal (stokes.C:330-331, 538-553); False = -schur_pc_type none.
        slab = (slab-mode FdPc, reduce_fn, reduce_ctx): `op` is the slab-mode operator of a slab driver (dist.py); the inner solves
        and the pressure mean complete their sums over the ranks, and apply() is collective."""
        h = C.c_void_p()
        if slab is None:
            _chk(lib().stokes_saddle_create(op._h, C.byref(h)))
        else:
            pc, rfn, rctx = slab
            self._slab_pc = pc
            _chk(lib().stokes_saddle_create_slab(op._h, pc._h, rfn, rctx, C.byref(h)))
        self._h = h
        self._op = op
        self.n = op.global_size
        _chk(lib().stokes_saddle_set_type(h, saddle_type))
        _chk(lib().stokes_saddle_set_pc_sweeps(h, pc_sweeps))
        _chk(lib().stokes_saddle_set_schur_jacobi(h, 1 if schur_jacobi else 0))
        for which, (m, rtol) in enumerate((vel, schur, svel)):
            _chk(lib().stokes_saddle_set_inner(h, which, m, rtol))

    def setup(self):
        """StokesPCSetUp0: call after StokesOp.function has changed the viscosity."""
        _chk(lib().stokes_saddle_setup(self._h, _stream()))

    def apply(self, x, y):
        _chk(lib().stokes_saddle_apply(self._h, _dev_ptr(x, self.n), _dev_ptr(y, self.n), _stream()))
        return y

    inner_iterations = property(lambda self: (lib().stokes_saddle_iterations(self._h, 0), lib().stokes_saddle_iterations(self._h, 1)))


class Fgmres(_Handle):
    """Restarted flexible GMRES on device vectors (KSPFGMRES's role, elliptic.C:181-185).

    `A` and the optional right preconditioner `M` are operator objects of this module (EllipticOp,
    StokesOp): their C entry points are handed to the solver directly, no Python in the loop.
    """
    _destroy = "chebhip_fgmres_destroy"

    def __init__(self, n, restart=30, rtol=1e-5, atol=1e-50, max_it=10000):
        self.n = int(n)
        h = C.c_void_p()
        _chk(lib().chebhip_fgmres_create(self.n, restart, C.byref(h)))
        self._h = h
        _chk(lib().chebhip_fgmres_set_tolerances(h, rtol, atol, max_it))

    APPLY_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p)
    REDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p)

    def _fn(self, op, entry):
        """C entry point + handle of an operator object, or a trampoline around a Python callable (x, y) on
        device tensors (used by the multi-rank drivers of dist.py, whose matvec includes the exchanges)."""
        if op is None:
            return None, None
        kind = type(op).__name__
        if kind in ("FdPc", "SpectralPc"):
            return C.cast(lib().chebhip_fdpc_apply, C.c_void_p), op._h
        if kind == "HelmholtzSolver":
            return C.cast(lib().cheb_helmholtz_apply, C.c_void_p), op._h
        if kind == "StokesSaddlePc":
            return C.cast(lib().stokes_saddle_apply, C.c_void_p), op._h
        if kind == "VarHelmholtz":                       # entry "mult": the operator; "precond": its preconditioner; "*_deflated": Pi of them
            name = {"precond": "cheb_varhelm_precond", "mult_deflated": "cheb_varhelm_apply_deflated",
                    "precond_deflated": "cheb_varhelm_precond_deflated"}.get(entry, "cheb_varhelm_apply")
            return C.cast(getattr(lib(), name), C.c_void_p), op._h
        if kind in ("EllipticOp", "StokesOp"):
            name = {"EllipticOp": "ell_op_", "StokesOp": "stokes_op_"}[kind] + entry
            return C.cast(getattr(lib(), name), C.c_void_p), op._h
        n = self.n

        def tramp(ctx, xp, yp, stream):
            try:
                op(device_view(xp, n), device_view(yp, n))
                return 0
            except Exception:
                import traceback
                traceback.print_exc()
                return 5
        cb = Fgmres.APPLY_FN(tramp)
        self._keep.append(cb)
        return C.cast(cb, C.c_void_p), None

    def set_reduce_raw(self, fn, ctx):
        """The same with a chebhip_reduce_fn given as (function pointer, context): Comm.reduce_fn() of dist.py."""
        _chk(lib().chebhip_fgmres_set_reduce(self._h, fn, ctx))

    def set_reduce(self, group=None):
        """Vectors are distributed over the ranks of `group`: complete every inner product with an all-reduce."""
        self._red = allreduce_trampoline(group)
        _chk(lib().chebhip_fgmres_set_reduce(self._h, C.cast(self._red, C.c_void_p), None))

    def solve(self, A, b, x, M=None, x_nonzero=False, a_entry="mult", m_entry="mult"):
        self._keep = []
        fa, ca = self._fn(A, a_entry)
        fm, cm = self._fn(M, m_entry)
        _chk(lib().chebhip_fgmres_solve(self._h, fa, ca, fm, cm, _dev_ptr(b, self.n), _dev_ptr(x, self.n),
                                        1 if x_nonzero else 0, _stream()))
        return x

    iterations = property(lambda self: lib().chebhip_fgmres_iterations(self._h))
    residual = property(lambda self: lib().chebhip_fgmres_residual(self._h))
    reason = property(lambda self: lib().chebhip_fgmres_reason(self._h))
