"""ctypes binding of libwavehip.so (the C ABI of include/wavehip.h)."""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_int, c_int32, c_int64, c_size_t, c_void_p

HERE = os.path.dirname(os.path.abspath(__file__))
# WAVEHIP_LIB selects another build of the same library (the diagnostic builds of tools/diag_build.sh
# and tools/dense_trace.sh); there is still no fallback if the file is missing.
LIB_PATH = os.environ.get("WAVEHIP_LIB") or os.path.join(HERE, "libwavehip.so")


class WavehipError(RuntimeError):
    """Mirrors the std::runtime_error the reference throws on device failures
    (common/cuda/array.hpp:15-17, mass.hpp:91-92, utils.hpp:30-34)."""


class Tuning(ctypes.Structure):
    """wf_tuning: explicit kernel selection / tuning (all zero = the library's choice)."""
    _fields_ = [("kernel", c_int), ("variant", c_int), ("lz", c_int), ("lz0", c_int),
                ("bx", c_int), ("by", c_int), ("bz", c_int), ("keep_cell_order", c_int), ("orient", c_int),
                ("geometry", c_int), ("metric", c_int), ("update", c_int)]


class OpDesc(ctypes.Structure):
    _fields_ = [
        ("kind", c_int), ("degree", c_int), ("ncells", c_int), ("ndofs", c_int),
        ("h_dofmap", POINTER(c_int32)), ("h_perm", POINTER(c_int32)),
        ("h_G", POINTER(c_double)), ("h_detJ", POINTER(c_double)),
        ("nverts", c_int), ("h_xverts", POINTER(c_double)), ("h_geom_dofmap", POINTER(c_int32)),
        ("c0", c_double), ("flags", c_int),
        ("nq1", c_int), ("h_phi1", POINTER(c_double)),
        ("h_qpts1", POINTER(c_double)), ("h_qwts1", POINTER(c_double)),
        ("tuning", POINTER(Tuning)),
        ("h_cell_coeff", POINTER(c_double)),
    ]


class DenseDesc(ctypes.Structure):
    _fields_ = [
        ("nd", c_int), ("nq", c_int), ("ncells", c_int), ("ndofs", c_int),
        ("h_dofmap", POINTER(c_int32)), ("h_dphi", POINTER(c_double)), ("h_weights", POINTER(c_double)),
        ("nverts", c_int), ("h_xverts", POINTER(c_double)), ("h_geom_dofmap", POINTER(c_int32)),
        ("c0", c_double), ("flags", c_int),
        ("h_cell_coeff", POINTER(c_double)),
    ]


class DenseMassDesc(ctypes.Structure):
    _fields_ = [
        ("nd", c_int), ("nq", c_int), ("ncells", c_int), ("ndofs", c_int),
        ("h_dofmap", POINTER(c_int32)), ("h_phi", POINTER(c_double)), ("h_weights", POINTER(c_double)),
        ("nverts", c_int), ("h_xverts", POINTER(c_double)), ("h_geom_dofmap", POINTER(c_int32)),
        ("flags", c_int),
        ("h_cell_coeff", POINTER(c_double)),
    ]


class OpInfo(ctypes.Structure):
    _fields_ = [
        ("kind", c_int), ("degree", c_int), ("num_cells", c_int), ("num_dofs_cell", c_int),
        ("num_quads", c_int), ("ndofs", c_int), ("structured", c_int),
        ("flops", c_double), ("alg_bytes", c_double), ("device_bytes", c_size_t),
        ("items_interior", c_int), ("items_interface", c_int),
        ("kernel", c_int), ("plan_items", c_int), ("plan_patterns", c_int), ("plan_lz", c_int),
        ("plan_reoriented", c_int), ("plan_fill", c_double), ("geometry", c_int), ("metric", c_int),
        ("update", c_int), ("cell_coeff", c_int),
    ]


class CellFormInfo(ctypes.Structure):
    """wf_cell_form_info_t"""
    _fields_ = [
        ("kind", c_int), ("degree", c_int), ("num_cells", c_int), ("ndofs", c_int), ("geometry", c_int),
        ("cell_coeff", c_int), ("alg_bytes", c_double), ("device_bytes", c_size_t),
    ]


class UpdaterDesc(ctypes.Structure):
    _fields_ = [
        ("ndofs", c_int),
        ("num_send_neighbors", c_int), ("send_neighbors", POINTER(c_int)),
        ("send_offsets", POINTER(c_int32)), ("send_indices", POINTER(c_int32)),
        ("num_recv_neighbors", c_int), ("recv_neighbors", POINTER(c_int)),
        ("recv_offsets", POINTER(c_int32)), ("ghost_positions", POINTER(c_int32)),
        ("flags", c_int),
    ]


class BoxPartitionInfo(ctypes.Structure):
    """wf_box_partition_info"""
    _fields_ = [
        ("procs", c_int * 3), ("coords", c_int * 3), ("owned_lo", c_int * 3), ("lattice", c_int * 3),
        ("size_global", c_int64), ("num_owned", c_int64),
        ("num_send_neighbors", c_int), ("num_recv_neighbors", c_int),
        ("num_send_indices", c_int32), ("num_recv_indices", c_int32),
        ("face_tag", c_int * 6),
    ]


class Wavelet(ctypes.Structure):
    """wf_wavelet"""
    _fields_ = [("kind", c_int), ("amplitude", c_double), ("frequency", c_double), ("delay", c_double),
                ("nsamples", c_int), ("h_samples", POINTER(c_double)), ("t_start", c_double), ("dt", c_double)]


MATVEC_FN = ctypes.CFUNCTYPE(c_int, c_void_p, c_void_p, c_void_p, c_void_p)


class CGDesc(ctypes.Structure):
    _fields_ = [
        ("n", c_int64), ("op", c_void_p), ("matvec", MATVEC_FN), ("user", c_void_p),
        ("updater", c_void_p), ("comm", c_void_p), ("kmax", c_int), ("rtol", c_double),
    ]


class WaveSource(ctypes.Structure):
    """wf_wave_source"""
    _fields_ = [("c0", c_double), ("c0_squared", c_double), ("p0", c_double), ("w0", c_double), ("freq0", c_double),
                ("alpha", c_double), ("period", c_double), ("medium", c_int)]


WAVE_RHS_FN = ctypes.CFUNCTYPE(c_int, c_void_p, c_void_p, c_void_p, c_void_p)
WAVE_STEP_FN = ctypes.CFUNCTYPE(c_int, c_void_p, c_int64, c_double, c_void_p, c_void_p, c_void_p, c_void_p)


class WaveDesc(ctypes.Structure):
    """wf_wave_desc"""
    _fields_ = [
        ("n", c_int64), ("d_m", c_void_p), ("d_b", c_void_p), ("bc", c_void_p), ("source", WaveSource),
        ("fold_boundary", c_int), ("op", c_void_p), ("updater", c_void_p), ("overlapped", c_int),
        ("rhs", WAVE_RHS_FN), ("rhs_user", c_void_p), ("sources", c_void_p), ("receivers", c_void_p),
        ("d_traces", c_void_p), ("h_times", POINTER(c_double)), ("trace_rows", c_int64), ("d_work", POINTER(c_void_p)),
    ]


WF_WAVE_RK4_FUSED, WF_WAVE_LEAPFROG, WF_WAVE_LEAPFROG4 = 0, 1, 2
WF_QUAD_GLL, WF_QUAD_GAUSS_JACOBI = 0, 1
WF_VARIANT_GLL_WARPED, WF_VARIANT_EQUISPACED = 0, 1
WF_MAX_QUAD_POINTS = 16
WF_COMM_ID_BYTES = 128
WF_SUM, WF_MAX = 0, 1
WF_UPDATER_DEFAULT, WF_UPDATER_INLINE = 0, 1
(WF_KERNEL_NONE, WF_KERNEL_MARCH_BOX, WF_KERNEL_MARCH_IDX, WF_KERNEL_BATCH_UNIQUE, WF_KERNEL_BOX_BLOCK, WF_KERNEL_DIAGONAL,
 WF_KERNEL_MASS_DENSE_ANY, WF_KERNEL_DENSE_SIMPLEX, WF_KERNEL_ELEMENTWISE, WF_KERNEL_CELLS_ORDERED,
 WF_KERNEL_DENSE_SIMPLEX_MASS) = range(11)
(WF_KERNEL_AUTO, WF_KERNEL_FORCE_BATCH, WF_KERNEL_FORCE_BOX_BLOCK, WF_KERNEL_FORCE_MASS_ANY, WF_KERNEL_FORCE_ELEMENTWISE,
 WF_KERNEL_FORCE_MARCH, WF_KERNEL_FORCE_MASS_MARCH) = range(7)
WF_OP_STIFFNESS, WF_OP_MASS_LUMPED, WF_OP_MASS_DENSE = 0, 1, 2
WF_FLAG_NONE, WF_FLAG_NO_FABS, WF_FLAG_NO_CLAMP, WF_FLAG_MASS_ELEMENTWISE, WF_FLAG_TENSOR_X_SLOWEST = 0, 1, 2, 4, 8
WF_FLAG_ORDERED = 16   # order-fixed accumulation: bitwise reproducible y on any mesh (include/wavehip.h)
WF_UPDATE_NONE, WF_UPDATE_ATOMIC, WF_UPDATE_OWNER, WF_UPDATE_ORDERED = 0, 1, 2, 3   # ORDERED: wf_op_info_t.update only
WF_WAVELET_RICKER, WF_WAVELET_SAMPLED = 0, 1
WF_PART_ALL, WF_PART_INTERIOR, WF_PART_INTERFACE, WF_PART_INTERIOR_A, WF_PART_INTERIOR_B = 0, 1, 2, 3, 4

# every symbol include/wavehip.h declares: name -> (restype, argtypes)
_DP, _IP, _VP = POINTER(c_double), POINTER(c_int32), c_void_p
SIGNATURES = {
    "wf_last_error": (c_char_p, []),
    "wf_version": (c_char_p, []),
    "wf_device_count": (c_int, [POINTER(c_int)]),
    "wf_set_device": (c_int, [c_int]),
    "wf_device_info": (c_int, [c_int, c_char_p, c_size_t, POINTER(c_size_t), POINTER(c_int)]),
    "wf_malloc": (c_int, [POINTER(c_void_p), c_size_t]),
    "wf_free": (c_int, [c_void_p]),
    "wf_memcpy_h2d": (c_int, [c_void_p, c_void_p, c_size_t]),
    "wf_memcpy_d2h": (c_int, [c_void_p, c_void_p, c_size_t]),
    "wf_memset": (c_int, [c_void_p, c_int, c_size_t, c_void_p]),
    "wf_sync": (c_int, [c_void_p]),
    "wf_tabulate_gll": (c_int, [c_int, _DP, _DP, _DP]),
    "wf_tabulate_dense": (c_int, [c_int, _DP]),
    "wf_quadrature_1d": (c_int, [c_int, c_int, POINTER(c_int), _DP, _DP]),
    "wf_tabulate_1d": (c_int, [c_int, c_int, c_int, _DP, c_int, _DP]),
    "wf_geometry_hex_rule": (c_int, [c_int, c_int, _DP, _IP, c_int, _DP, _DP, c_int, c_int, _DP, _DP]),
    "wf_geometry_hex_cell": (c_int, [c_int, c_int64, c_int64, _DP, _IP, c_int, c_int, _DP, POINTER(c_int64), POINTER(c_int)]),
    "wf_reorder_dofmap": (c_int, [c_int, c_int, _IP, _IP, _IP]),
    "wf_lattice_numbering": (c_int, [c_int, ctypes.c_int64, ctypes.c_int32, _IP, _IP]),
    "wf_geometry_hex": (c_int, [c_int, c_int, c_int, _DP, _IP, c_int, c_int, _DP, _DP]),
    "wf_op_create": (c_int, [POINTER(OpDesc), POINTER(c_void_p)]),
    "wf_op_create_box": (c_int, [c_int, c_int, c_int, c_int, c_int, _DP, c_double, c_int, POINTER(c_void_p)]),
    "wf_op_create_box_tuned": (c_int, [c_int, c_int, c_int, c_int, c_int, _DP, c_double, c_int, POINTER(Tuning),
                                       POINTER(c_void_p)]),
    "wf_op_create_box_coeff": (c_int, [c_int, c_int, c_int, c_int, c_int, _DP, c_double, _DP, c_int, POINTER(Tuning),
                                       POINTER(c_void_p)]),
    "wf_op_set_ghost_dofs": (c_int, [c_void_p, _IP, c_int32]),
    "wf_op_create_dense_simplex": (c_int, [POINTER(DenseDesc), POINTER(c_void_p)]),
    "wf_op_create_dense_simplex_mass": (c_int, [POINTER(DenseMassDesc), POINTER(c_void_p)]),
    "wf_op_apply": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "wf_op_set_ghost_faces": (c_int, [c_void_p, c_int, c_int, c_int]),
    "wf_op_apply_part": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "wf_op_info": (c_int, [c_void_p, POINTER(OpInfo)]),
    "wf_box_run_plan": (c_int, [c_int, c_int, c_int, c_int, c_double, c_int, POINTER(c_int32), c_int32, POINTER(c_int32),
                                POINTER(c_double), POINTER(c_double), POINTER(c_int32)]),
    "wf_op_replan_runs": (c_int, [c_void_p, c_int]),
    "wf_op_set_runs": (c_int, [c_void_p, POINTER(c_int32), c_int32]),
    "wf_op_get_runs": (c_int, [c_void_p, POINTER(c_int32), c_int32, POINTER(c_int32)]),
    "wf_op_destroy": (c_int, [c_void_p]),
    "wf_gather": (c_int, [c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "wf_scatter_add": (c_int, [c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "wf_scatter_set": (c_int, [c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "wf_transform1": (c_int, [c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "wf_ordered_slots": (c_int, [c_int64, c_int, c_int32, _IP, _IP, _IP]),
    "wf_segment_sum_add": (c_int, [c_int32, c_void_p, c_void_p, c_void_p, c_void_p]),
    "wf_tsmm": (c_int, [c_int, c_int64, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "wf_copy": (c_int, [c_int64, c_void_p, c_void_p, c_void_p]),
    "wf_fill": (c_int, [c_int64, c_double, c_void_p, c_void_p]),
    "wf_axpy": (c_int, [c_int64, c_double, c_void_p, c_void_p, c_void_p, c_void_p]),
    "wf_scale": (c_int, [c_int64, c_double, c_void_p, c_void_p]),
    "wf_pointwise_div": (c_int, [c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "wf_pointwise_mult_add": (c_int, [c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "wf_dot": (c_int, [c_int64, c_void_p, c_void_p, c_void_p, c_void_p]),
    "wf_rk4_stage": (c_int, [c_int64, c_double, c_double, c_int] + [c_void_p] * 12),
    "wf_boundary_create": (c_int, [c_int64, c_int32, _IP, _DP, c_int32, _IP, _DP, POINTER(c_void_p)]),
    "wf_boundary_destroy": (c_int, [c_void_p]),
    "wf_boundary_apply_plan": (c_int, [c_void_p, c_double, c_double, c_void_p, c_void_p, c_void_p]),
    "wf_rk4_stage_bc": (c_int, [c_int64, c_double, c_double, c_int] + [c_void_p] * 11 + [c_void_p, c_double, c_double, c_void_p]),
    "wf_leapfrog_step": (c_int, [c_int64, c_double] + [c_void_p] * 7),
    "wf_leapfrog_step_bc": (c_int, [c_int64, c_double] + [c_void_p] * 6 + [c_void_p, c_double, c_double, c_void_p]),
    "wf_leapfrog4_predict": (c_int, [c_int64, c_double] + [c_void_p] * 6 + [c_void_p, c_double, c_double, c_void_p]),
    "wf_leapfrog4_correct": (c_int, [c_int64, c_double] + [c_void_p] * 6 + [c_void_p, c_double, c_double, c_void_p]),
    "wf_comm_unique_id": (c_int, [c_char_p]),
    "wf_comm_create": (c_int, [c_char_p, c_int, c_int, POINTER(c_void_p)]),
    "wf_comm_rendezvous_file": (c_int, [c_char_p, c_int, c_double, c_char_p]),
    "wf_comm_create_from_file": (c_int, [c_char_p, c_int, c_int, c_double, POINTER(c_void_p)]),
    "wf_comm_info": (c_int, [c_void_p, POINTER(c_int), POINTER(c_int), POINTER(c_int)]),
    "wf_comm_allreduce": (c_int, [c_void_p, c_int, c_int64, c_void_p, c_void_p, c_void_p]),
    "wf_comm_barrier": (c_int, [c_void_p, c_void_p]),
    "wf_comm_destroy": (c_int, [c_void_p]),
    "wf_updater_create": (c_int, [c_void_p, POINTER(UpdaterDesc), POINTER(c_void_p)]),
    "wf_updater_fwd_begin": (c_int, [c_void_p, c_void_p, c_void_p]),
    "wf_updater_fwd_end": (c_int, [c_void_p, c_void_p, c_void_p]),
    "wf_updater_fwd": (c_int, [c_void_p, c_void_p, c_void_p]),
    "wf_updater_rev_begin": (c_int, [c_void_p, c_void_p, c_void_p]),
    "wf_updater_rev_end": (c_int, [c_void_p, c_void_p, c_void_p]),
    "wf_updater_rev": (c_int, [c_void_p, c_void_p, c_void_p]),
    "wf_updater_info": (c_int, [c_void_p, POINTER(c_int), POINTER(c_int), POINTER(c_int), POINTER(c_int)]),
    "wf_updater_destroy": (c_int, [c_void_p]),
    "wf_op_apply_overlapped": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "wf_mesh_open": (c_int, [c_char_p, c_char_p, POINTER(c_void_p)]),
    "wf_mesh_sizes": (c_int, [c_void_p, POINTER(c_int64), POINTER(c_int64)]),
    "wf_mesh_read": (c_int, [c_void_p, _DP, _IP]),
    "wf_mesh_tags_size": (c_int, [c_void_p, c_char_p, POINTER(c_int64)]),
    "wf_mesh_read_tags": (c_int, [c_void_p, c_char_p, _IP, _IP]),
    "wf_mesh_close": (c_int, [c_void_p]),
    "wf_mesh_write": (c_int, [c_char_p, c_char_p, c_int64, _DP, c_int64, _IP, c_char_p, c_int64, _IP, _IP]),
    "wf_markers_enable": (c_int, [c_int]),
    "wf_marker_push": (c_int, [c_char_p]),
    "wf_marker_pop": (c_int, []),
    "wf_marker_mark": (c_int, [c_char_p]),
    "wf_fs_build": (c_int, [c_int, c_int64, _DP, c_int64, _IP, POINTER(c_int64), _IP, _DP, c_int64]),
    "wf_fs_locate_facets": (c_int, [c_int64, _IP, c_int64, _IP, _IP, _IP, _IP]),
    "wf_fs_facet_mass": (c_int, [c_int, c_int64, _DP, c_int64, _IP, _IP, c_int64, _IP, _IP, _IP, POINTER(c_int64), _IP, _DP]),
    "wf_fs_facet_mass_weighted": (c_int, [c_int, c_int64, _DP, c_int64, _IP, _IP, c_int64, _IP, _IP, _IP, _DP, POINTER(c_int64),
                                          _IP, _DP]),
    "wf_fs_min_cell_diameter": (c_int, [c_int64, _DP, c_int64, _IP, POINTER(c_double)]),
    "wf_box_mesh": (c_int, [POINTER(c_int), _DP, _DP, _DP, _IP]),
    "wf_box_dofmap": (c_int, [c_int, POINTER(c_int), _IP]),
    "wf_box_facet_mass": (c_int, [c_int, POINTER(c_int), _DP, POINTER(c_int), c_int, _DP, POINTER(c_int64), _IP, _DP]),
    "wf_decompose3d": (c_int, [c_int, POINTER(c_int)]),
    "wf_box_partition": (c_int, [POINTER(c_int), c_int, c_int, c_int, POINTER(c_int), POINTER(BoxPartitionInfo),
                                 POINTER(c_int), _IP, _IP, POINTER(c_int), _IP, _IP]),
    "wf_cg": (c_int, [POINTER(CGDesc), c_void_p, c_void_p, POINTER(c_int), POINTER(c_double), c_void_p]),
    "wf_boundary_apply": (c_int, [c_int32, c_void_p, c_void_p, c_double, c_int32, c_void_p, c_void_p, c_double,
                                  c_void_p, c_void_p, c_void_p]),
    "wf_points_locate": (c_int, [c_int64, _DP, c_int64, _IP, c_int64, _DP, c_double, _IP, _DP]),
    "wf_points_weights": (c_int, [c_int, c_int64, _DP, _DP]),
    "wf_sources_merge": (c_int, [c_int, c_int, _IP, _DP, _IP, _IP, _IP, _IP, _IP, _DP]),
    "wf_points_create": (c_int, [c_int, c_int64, c_int, _IP, _DP, POINTER(c_void_p)]),
    "wf_points_destroy": (c_int, [c_void_p]),
    "wf_points_info": (c_int, [c_void_p, POINTER(c_int), POINTER(c_int), POINTER(c_int)]),
    "wf_points_sample": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "wf_sources_create": (c_int, [c_void_p, c_int, _IP, POINTER(Wavelet), POINTER(c_void_p)]),
    "wf_sources_destroy": (c_int, [c_void_p]),
    "wf_sources_info": (c_int, [c_void_p, POINTER(c_int), POINTER(c_int), POINTER(c_int)]),
    "wf_sources_add": (c_int, [c_void_p, c_double, c_void_p, c_void_p]),
    "wf_sources_add_stencil": (c_int, [c_void_p, c_int, _DP, _DP, c_void_p, c_void_p]),
    "wf_leapfrog_correlate": (c_int, [c_int64] + [c_void_p] * 6),
    "wf_leapfrog4_correlate": (c_int, [c_int64] + [c_void_p] * 9),
    "wf_sources_add_values": (c_int, [c_void_p, c_void_p, c_double, c_void_p, c_void_p]),
    "wf_cell_form_create": (c_int, [POINTER(OpDesc), POINTER(c_void_p)]),
    "wf_cell_form_create_box": (c_int, [c_int, c_int, c_int, c_int, c_int, _DP, c_double, _DP, c_int, POINTER(Tuning),
                                        POINTER(c_void_p)]),
    "wf_cell_form_eval": (c_int, [c_void_p, c_void_p, c_void_p, c_double, c_int, c_void_p, c_void_p]),
    "wf_cell_form_info": (c_int, [c_void_p, POINTER(CellFormInfo)]),
    "wf_cell_form_destroy": (c_int, [c_void_p]),
    "wf_wave_window": (c_double, [POINTER(WaveSource), c_double]),
    "wf_wave_g": (c_double, [POINTER(WaveSource), c_double]),
    "wf_wave_s1": (c_double, [POINTER(WaveSource), c_double]),
    "wf_wave_s1_left_to_right": (c_double, [POINTER(WaveSource), c_double]),
    "wf_wave_s2": (c_double, [POINTER(WaveSource)]),
    "wf_wave_work_vectors": (c_int, [c_int]),
    "wf_wave_step_count": (c_int64, [c_int, c_double, c_double, c_double, c_int64]),
    "wf_wave_rk4_fused": (c_int, [POINTER(WaveDesc), c_double, c_double, c_double, c_int64, c_void_p, c_void_p,
                                  POINTER(c_double), POINTER(c_int64), c_void_p]),
    "wf_wave_leapfrog": (c_int, [POINTER(WaveDesc), c_double, c_double, c_double, c_int64, c_void_p, c_void_p, WAVE_STEP_FN,
                                 c_void_p, POINTER(c_double), POINTER(c_int64), c_void_p]),
    "wf_wave_leapfrog4": (c_int, [POINTER(WaveDesc), c_double, c_double, c_double, c_int64, c_void_p, c_void_p, WAVE_STEP_FN,
                                  c_void_p, POINTER(c_void_p), POINTER(c_double), POINTER(c_int64), c_void_p]),
}

_LIB = None


def lib():
    """Load libwavehip.so.  Raises (never falls back) when it is missing."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise WavehipError(
                f"{LIB_PATH} not found: build it with `python -m wave_fenics_amd.build` "
                "(there is no CPU fallback for the operator path)")
        # PyTorch-ROCm bundles its own HIP runtime; if libwavehip pulled in the system
        # libamdhip64 first, torch would later start a second runtime in the same
        # process and see no GPU.  Load torch's runtime first whenever torch is there
        # (libwavehip then binds to the already-loaded libamdhip64 by SONAME).
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)          # AttributeError if the library lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        _LIB = L
    return _LIB


def _dp(a):
    """a float64 numpy array (or None) as the const double* of a C ABI call"""
    return None if a is None else a.ctypes.data_as(_DP)


def _ip(a):
    """an int32 numpy array (or None) as the const int32_t* of a C ABI call"""
    return None if a is None else a.ctypes.data_as(_IP)


class Handle:
    """Owner of one library handle, self._h (a c_void_p), freed by the wf_*_destroy function a subclass names: close()
    once or many times, or the garbage collector.  A closed object holds the null handle, which every entry point
    refuses."""
    _destroy: str = ""

    def close(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            getattr(lib(), self._destroy)(h)
        self._h = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def check(rc: int):
    if rc != 0:
        msg = lib().wf_last_error().decode(errors="replace")
        err = WavehipError(f"libwavehip error {rc}: {msg}")
        err.status = rc   # the wf_status value
        raise err
