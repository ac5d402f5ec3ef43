"""ctypes binding of the device library (include/nsx.h -> csrc/libnsx.so).

Plumbing for tests and bench.py only.  There is no CPU fallback: without a HIP device `Nsx(...)` raises,
and without the built library the import of the symbols raises.
"""
import ctypes as C

import numpy as np

from ._lib import DEV_SO, load

_i32p = C.POINTER(C.c_int32)
_f64p = C.POINTER(C.c_double)

TEMAM, DOUBLE_CONVECTION = 1, 2
YOSIDA, SIMPLE, AYOSIDA, ASIMPLE = 0, 1, 2, 3

# every symbol include/nsx.h declares (tests check that the library exports all of them)
API = [
    "nsx_create", "nsx_destroy", "nsx_last_error", "nsx_version", "nsx_set_tables", "nsx_set_mesh", "nsx_set_ranks",
    "nsx_set_schur_blocks", "nsx_set_solution", "nsx_get_solution", "nsx_get_solution_ghosted", "nsx_get_rhs",
    "nsx_set_rhs", "nsx_assemble", "nsx_assemble_time_step", "nsx_add_rhs", "nsx_apply_boundary_values",
    "nsx_solve_time_step", "nsx_prec_initialize", "nsx_prec_vmult", "nsx_system_vmult", "nsx_ilu_apply",
    "nsx_export_block", "nsx_schur_nnz", "nsx_schur_get", "nsx_scalar_graph_nnz", "nsx_scalar_graph", "nsx_ilu_get",
    "nsx_profile_enable", "nsx_profile_reset", "nsx_profile_count", "nsx_profile_get", "nsx_persistent_state", "nsx_path_info", "nsx_ilu_path_info", "nsx_ilu_invert_staged", "nsx_schur_plan_info", "nsx_comm_self_halo_test", "nsx_comm_unique_id",
    "nsx_comm_init", "nsx_comm_init_callbacks", "nsx_comm_counters", "nsx_set_mesh_distributed", "nsx_set_force_faces", "nsx_compute_forces",
    "nsx_set_internal_layout", "nsx_layout_info", "nsx_layout_get", "nsx_gram_schmidt_cycle", "nsx_set_inner_precision",
    "nsx_gram_schmidt_sweeps", "nsx_compute_diagnostics", "nsx_get_cell_diagnostic", "nsx_schur_cg", "nsx_blas1_run", "nsx_gmres",
    "nsx_set_probes", "nsx_get_probe_cells", "nsx_eval_probes", "nsx_set_tracers", "nsx_advect_tracers", "nsx_get_tracers",
    "nsx_sparse_product", "nsx_prec_get_vector", "nsx_compute_nodal_fields", "nsx_nodal_field_components", "nsx_get_nodal_field",
    "nsx_extract_isosurface", "nsx_get_isosurface",
    "nsx_set_lattice", "nsx_get_lattice_cells", "nsx_eval_lattice", "nsx_get_lattice",
    "nsx_stats_begin", "nsx_stats_accumulate", "nsx_stats_info", "nsx_stats_components", "nsx_stats_get",
    "nsx_set_surface", "nsx_surface_info", "nsx_get_surface_layout", "nsx_compute_surface", "nsx_surface_field_components", "nsx_get_surface_field",
]
# declared in include/nsx.h as well, but with a capital letter in its name, which the header scan of tests/test_abi.py (lower case only)
# does not see: kept beside the list that scan is compared with; build() checks both
API_EXTRA = ["nsx_inner_F_vmult"]
FIRST_TOUCH, COLOUR, COLOUR_ALL = 0, 1, 2  # node order of nsx_set_internal_layout
INNER_FP64, INNER_FP32 = 0, 1  # nsx_set_inner_precision: how F and the ILU(0) entries of F are stored for the inner solves
# planes of nsx_get_cell_diagnostic (NSX_DIAG_*)
DIAG_ENERGY, DIAG_DIV2, DIAG_GRAD2, DIAG_ENSTROPHY, DIAG_CHANGE2, DIAG_VOLUME, DIAG_CFL, DIAG_SPEED, DIAG_COUNT = range(9)
# ops of nsx_sparse_product (NSX_PROD_*)
PROD_F, PROD_F_INNER, PROD_F_RESID, PROD_MASS, PROD_B, PROD_B_MINUS_R, PROD_R_MINUS_B, PROD_G, PROD_G_ACC, PROD_S, PROD_SADDLE, PROD_COUNT = range(12)
# vectors of nsx_prec_get_vector (NSX_PREC_VEC_*)
PREC_VEC_D, PREC_VEC_D_INV, PREC_VEC_NEG_D_INV, PREC_VEC_LUMP_M, PREC_VEC_SCHUR_W, PREC_VEC_DIRMASK, PREC_VEC_COUNT = range(7)
TRACER_EULER, TRACER_RK2, TRACER_RK4 = 1, 2, 4                                   # NSX_TRACER_*: scheme
TRACER_FROZEN, TRACER_LINEAR = 0, 1                                              # field
TRACER_NOT_FOUND, TRACER_ACTIVE, TRACER_EXITED, TRACER_LOST = 0, 1, 2, 3         # status
# fields of nsx_get_nodal_field (NSX_FIELD_*)
FIELD_GRADIENT, FIELD_VORTICITY, FIELD_Q, FIELD_STRAIN, FIELD_DIVERGENCE, FIELD_COUNT = range(6)
# source kinds of nsx_extract_isosurface (NSX_ISO_*)
ISO_VELOCITY, ISO_PRESSURE, ISO_NODAL, ISO_PLANE = range(4)
# quantities of nsx_eval_lattice / nsx_get_lattice (NSX_LATTICE_*): bits
LATTICE_VELOCITY, LATTICE_PRESSURE, LATTICE_GRADIENT, LATTICE_NODAL = 1, 2, 4, 8
# parts of nsx_stats_begin (NSX_STATS_*: bits) and quantities of nsx_stats_get
STATS_VELOCITY, STATS_PRESSURE = 1, 2
(STATS_MEAN_U, STATS_COMOMENT_U, STATS_STRESS_U, STATS_RMS_U, STATS_TKE, STATS_MEAN_P, STATS_COMOMENT_P, STATS_VAR_P, STATS_RMS_P,
 STATS_QUANTITY_COUNT) = range(10)
# nsx_set_surface: form of the viscous stress; nsx_get_surface_field: where, and which field (NSX_SURFACE_*)
SURFACE_SYMMETRIC, SURFACE_GRADIENT = 0, 1
SURFACE_AT_FACES, SURFACE_AT_NODES = 0, 1
(SURFACE_PRESSURE, SURFACE_TRACTION, SURFACE_SHEAR, SURFACE_SHEAR_MAGNITUDE, SURFACE_NORMAL, SURFACE_YPLUS,
 SURFACE_FIELD_COUNT) = range(7)

ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, _f64p, C.c_int)
EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(_f64p), C.POINTER(C.c_int),
                          C.POINTER(_f64p), C.POINTER(C.c_int))


class Params(C.Structure):
    _fields_ = [("dim", C.c_int), ("device", C.c_int), ("nu", C.c_double), ("deltat", C.c_double)]


class Stats(C.Structure):
    _fields_ = [("outer_iterations", C.c_int), ("inner_F_iterations", C.c_int), ("inner_S_iterations", C.c_int),
                ("n_F_solves", C.c_int), ("n_S_solves", C.c_int), ("final_residual", C.c_double),
                ("t_prec", C.c_double), ("t_solve", C.c_double), ("status", C.c_int), ("persistent_fallbacks", C.c_int)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class FlowDiag(C.Structure):
    """nsx_flow_diag"""
    _fields_ = [("kinetic_energy", C.c_double), ("div_l2", C.c_double), ("grad_l2_sq", C.c_double), ("enstrophy", C.c_double),
                ("change_l2", C.c_double), ("volume", C.c_double), ("cfl_max", C.c_double), ("speed_max", C.c_double),
                ("n_cells", C.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class SurfaceTotals(C.Structure):
    """nsx_surface_totals"""
    _fields_ = [("area", C.c_double), ("force_pressure", C.c_double * 3), ("force_viscous", C.c_double * 3), ("torque", C.c_double * 3),
                ("flux", C.c_double), ("pressure_integral", C.c_double), ("n_faces", C.c_int64)]

    def as_dict(self):
        return {k: (np.array(getattr(self, k)) if k in ("force_pressure", "force_viscous", "torque") else getattr(self, k)) for k, _ in self._fields_}


BLAS1_KINDS = ("dot", "add_and_dot", "add", "add_dev", "sadd", "scale", "scale_dev_inv", "scale_vec", "axpy_multi", "axpy_multi_into",
               "cg_update", "cg_direction", "reciprocal", "finalize", "read", "write_scalar")   # NSX_BLAS1_*, in the header's order
BLAS1_MAX_K = 40
GMRES_F, GMRES_S = 0, 1                                                                           # NSX_GMRES_*: system
GMRES_PLAIN, GMRES_FUSED_GUESS, GMRES_FUSED_FROM_X0, GMRES_ZERO, GMRES_FUSED_ZERO_NEG = range(5)  # mode
GMRES_ABS_TOL = 256


class Blas1Op(C.Structure):
    """nsx_blas1_op"""
    _fields_ = [("kind", C.c_int32), ("d", C.c_int32), ("v", C.c_int32), ("w", C.c_int32), ("x", C.c_int32), ("slot", C.c_int32),
                ("num", C.c_int32), ("den", C.c_int32), ("count", C.c_int32), ("read", C.c_int32), ("n", C.c_int32), ("k", C.c_int32),
                ("vs", C.c_int32 * BLAS1_MAX_K), ("a", C.c_double), ("s", C.c_double), ("coef", C.c_double * BLAS1_MAX_K)]


class IsoSource(C.Structure):
    """nsx_iso_source"""
    _fields_ = [("kind", C.c_int), ("which", C.c_int), ("component", C.c_int), ("normal", C.c_double * 3)]


def iso_source(kind, which=0, component=0, normal=None):
    """an nsx_iso_source: ISO_VELOCITY (component 0 .. dim-1, -1: magnitude), ISO_PRESSURE, ISO_NODAL (which = FIELD_*, component),
    ISO_PLANE (normal)"""
    n = list(normal) if normal is not None else []
    return IsoSource(int(kind), int(which), int(component), (C.c_double * 3)(*(n + [0.0] * (3 - len(n)))))


class NsxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("nsx error %d: %s" % (code, msg))
        self.code = code
        self.diag = None  # Nsx.diagnostics(): the values of a call that found some of them not finite


def lib():
    L = load(DEV_SO)
    if getattr(L, "_nsx_ready", False):
        return L
    vp = C.c_void_p
    L.nsx_create.argtypes = [C.POINTER(Params), C.POINTER(vp)]
    L.nsx_destroy.argtypes = [vp]
    L.nsx_last_error.restype = C.c_char_p
    L.nsx_last_error.argtypes = [vp]
    L.nsx_version.restype = C.c_char_p
    L.nsx_set_tables.argtypes = [vp, C.c_int, C.c_int, C.c_int, _f64p, _f64p, _f64p, _f64p]
    L.nsx_set_mesh.argtypes = [vp, C.c_int, C.c_int, _i32p, _f64p, C.c_int, C.c_int]
    L.nsx_set_ranks.argtypes = [vp, C.c_int, _i32p, _i32p]
    L.nsx_set_schur_blocks.argtypes = [vp, C.c_int, _i32p]
    L.nsx_set_internal_layout.argtypes = [vp, C.c_int, C.c_int, C.c_int]
    L.nsx_layout_info.argtypes = [vp, C.POINTER(C.c_int)]
    L.nsx_layout_get.argtypes = [vp, _i32p, _i32p, _i32p, _i32p, _i32p]
    L.nsx_gram_schmidt_cycle.argtypes = [vp, C.c_int, C.c_int, _f64p, C.c_double, _f64p, _f64p]
    L.nsx_gram_schmidt_sweeps.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, _f64p, C.c_double, C.c_int, _f64p, _f64p, _f64p, _i32p]
    for f in ("nsx_set_solution", "nsx_get_solution", "nsx_get_solution_ghosted", "nsx_get_rhs", "nsx_set_rhs"):
        getattr(L, f).argtypes = [vp, _f64p]
    L.nsx_assemble.argtypes = [vp, C.c_int]
    L.nsx_assemble_time_step.argtypes = [vp, C.c_int]
    L.nsx_add_rhs.argtypes = [vp, C.c_int, _i32p, _f64p]
    L.nsx_apply_boundary_values.argtypes = [vp, C.c_int, _i32p, _f64p]
    L.nsx_solve_time_step.argtypes = [vp, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.POINTER(Stats)]
    L.nsx_prec_initialize.argtypes = [vp, C.c_int]
    L.nsx_prec_vmult.argtypes = [vp, C.c_int, C.c_double, C.c_int, _f64p, _f64p, C.POINTER(Stats)]
    L.nsx_system_vmult.argtypes = [vp, _f64p, _f64p]
    L.nsx_ilu_apply.argtypes = [vp, C.c_int, _f64p, _f64p]
    L.nsx_export_block.argtypes = [vp, C.c_int, C.c_int, C.c_int, _i32p, _i32p, _f64p]
    L.nsx_schur_nnz.argtypes = [vp, C.POINTER(C.c_int64)]
    L.nsx_schur_get.argtypes = [vp, _i32p, _i32p, _f64p]
    L.nsx_scalar_graph_nnz.argtypes = [vp, C.c_int, C.POINTER(C.c_int64)]
    L.nsx_scalar_graph.argtypes = [vp, C.c_int, _i32p, _i32p]
    L.nsx_ilu_get.argtypes = [vp, C.c_int, _f64p]
    L.nsx_profile_enable.argtypes = [vp, C.c_int]
    L.nsx_profile_reset.argtypes = [vp]
    L.nsx_profile_count.argtypes = [vp]
    L.nsx_profile_get.argtypes = [vp, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int64), _f64p, _f64p]
    L.nsx_persistent_state.argtypes = [vp, C.POINTER(C.c_int)]
    L.nsx_ilu_path_info.argtypes = [vp, C.c_int, C.POINTER(C.c_int)]
    L.nsx_ilu_invert_staged.argtypes = [vp, C.c_int, C.POINTER(C.c_int)]
    L.nsx_schur_plan_info.argtypes = [vp, C.POINTER(C.c_longlong)]
    L.nsx_comm_unique_id.argtypes = [C.POINTER(C.c_uint8)]
    L.nsx_comm_init.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_uint8)]
    L.nsx_comm_init_callbacks.argtypes = [vp, C.c_int, C.c_int, ALLREDUCE_FN, EXCHANGE_FN, C.c_void_p]
    L.nsx_comm_counters.argtypes = [vp, C.POINTER(C.c_longlong)]
    L.nsx_set_mesh_distributed.argtypes = [vp, C.c_int, C.c_int, C.c_int, _i32p, _f64p, C.c_int, C.c_int, C.c_int, C.c_int,
                                           _i32p, _i32p, C.c_int, _i32p, _i32p, _i32p, _i32p, _i32p]
    L.nsx_set_force_faces.argtypes = [vp, C.c_int, _i32p, _i32p, C.c_int, _f64p, _f64p, _f64p, _f64p]
    L.nsx_compute_forces.argtypes = [vp, _f64p, _f64p]
    L.nsx_compute_diagnostics.argtypes = [vp, C.POINTER(FlowDiag)]
    L.nsx_get_cell_diagnostic.argtypes = [vp, C.c_int, _f64p]
    L.nsx_set_probes.argtypes = [vp, C.c_int, _f64p, C.c_double]
    L.nsx_get_probe_cells.argtypes = [vp, _i32p, _i32p, _f64p]
    L.nsx_eval_probes.argtypes = [vp, _f64p, _f64p, _f64p, _i32p]
    L.nsx_set_tracers.argtypes = [vp, C.c_int, _f64p, C.c_double]
    L.nsx_advect_tracers.argtypes = [vp, C.c_double, C.c_int, C.c_int, C.c_int]
    L.nsx_get_tracers.argtypes = [vp, _f64p, _i32p, _i32p, _i32p, _f64p]
    L.nsx_compute_nodal_fields.argtypes = [vp]
    L.nsx_nodal_field_components.argtypes = [vp, C.c_int, C.POINTER(C.c_int)]
    L.nsx_get_nodal_field.argtypes = [vp, C.c_int, _f64p]
    L.nsx_extract_isosurface.argtypes = [vp, C.POINTER(IsoSource), C.c_double, C.POINTER(IsoSource), C.POINTER(C.c_int64)]
    L.nsx_get_isosurface.argtypes = [vp, _f64p, _f64p, _i32p]
    L.nsx_set_lattice.argtypes = [vp, _f64p, _f64p, _i32p, C.c_double, C.POINTER(C.c_int64)]
    L.nsx_get_lattice_cells.argtypes = [vp, _i32p]
    L.nsx_eval_lattice.argtypes = [vp, C.c_int]
    L.nsx_get_lattice.argtypes = [vp, C.c_int, C.c_int, _f64p]
    L.nsx_stats_begin.argtypes = [vp, C.c_int, C.c_int]
    L.nsx_stats_accumulate.argtypes = [vp, C.c_int, C.c_double]
    L.nsx_stats_info.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int64), _f64p]
    L.nsx_stats_components.argtypes = [vp, C.c_int, C.POINTER(C.c_int)]
    L.nsx_stats_get.argtypes = [vp, C.c_int, C.c_int, _f64p]
    L.nsx_set_surface.argtypes = [vp, C.c_int, _i32p, _i32p, _i32p, C.c_int, C.c_int, _f64p]
    L.nsx_surface_info.argtypes = [vp, C.POINTER(C.c_int)]
    L.nsx_get_surface_layout.argtypes = [vp, _i32p, _i32p, _i32p, _f64p]
    L.nsx_compute_surface.argtypes = [vp, C.POINTER(SurfaceTotals)]
    L.nsx_surface_field_components.argtypes = [vp, C.c_int, C.POINTER(C.c_int)]
    L.nsx_get_surface_field.argtypes = [vp, C.c_int, C.c_int, _f64p]
    L.nsx_set_inner_precision.argtypes = [vp, C.c_int]
    L.nsx_inner_F_vmult.argtypes = [vp, _f64p, _f64p]
    L.nsx_schur_cg.argtypes = [vp, C.c_double, C.c_int, _f64p, _f64p, C.POINTER(C.c_int), _f64p, C.POINTER(C.c_int)]
    L.nsx_sparse_product.argtypes = [vp, C.c_int, _f64p, _f64p, _f64p]
    L.nsx_prec_get_vector.argtypes = [vp, C.c_int, _f64p]
    L.nsx_gmres.argtypes = [vp, C.c_int, C.c_int, C.c_double, C.c_int, _f64p, _f64p, _f64p, C.POINTER(C.c_int), _f64p]
    L.nsx_blas1_run.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, _f64p, C.c_int, C.POINTER(Blas1Op), _f64p, _f64p, C.c_int]
    L._nsx_ready = True
    return L


def _i(a):
    return a.ctypes.data_as(_i32p)


def _d(a):
    return a.ctypes.data_as(_f64p)


def _ci(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _cd(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def gloo_callbacks():
    """Host-buffer communicator callbacks on torch.distributed (any backend with CPU tensors, e.g. gloo)."""
    import torch
    import torch.distributed as dist

    def allreduce(ctx, buf, count):
        t = torch.from_numpy(np.ctypeslib.as_array(buf, shape=(count,)))
        dist.all_reduce(t)
        return 0

    def exchange(ctx, n, ranks, send, scount, recv, rcount):
        reqs, keep = [], []
        for k in range(n):
            if rcount[k]:
                t = torch.from_numpy(np.ctypeslib.as_array(recv[k], shape=(rcount[k],)))
                keep.append(t)
                reqs.append(dist.irecv(t, src=int(ranks[k])))
            if scount[k]:
                t = torch.from_numpy(np.ctypeslib.as_array(send[k], shape=(scount[k],)).copy())
                keep.append(t)
                reqs.append(dist.isend(t, dst=int(ranks[k])))
        for q in reqs:
            q.wait()
        return 0

    return ALLREDUCE_FN(allreduce), EXCHANGE_FN(exchange)


class Nsx:
    """One device-side `NavierStokes` problem (a handle of libnsx)."""

    def __init__(self, dofs, tables, nu, deltat, device=0, rank=0, world=1, comm="rccl", layout=None, inner_precision=None):
        """world == 1: the whole problem on one GPU.  world > 1: this process holds rank `rank` of a run with one
        process per GPU (mesh partitioned with Mesh.partition(world, n_sub)); `comm` = "rccl" (needs an initialised
        torch.distributed group to broadcast the unique id) or "callbacks" (host buffers over torch.distributed).
        layout = (n_virtual_ranks, order, schur_max_rows): nsx_set_internal_layout, requested before the mesh is handed over.
        inner_precision = INNER_FP64 / INNER_FP32 (nsx_set_inner_precision); None leaves the library's initial value (the environment's
        NSX_INNER_PRECISION, else FP64)."""
        L = lib()
        self.L = L
        self._h = C.c_void_p()
        prm = Params(dofs.dim, device, float(nu), float(deltat))
        rc = L.nsx_create(C.byref(prm), C.byref(self._h))
        if rc:
            raise NsxError(rc, (L.nsx_last_error(None) or b"").decode())
        self.dim, self.n_u, self.n_p = dofs.dim, dofs.n_u, dofs.n_p
        self.n = self.n_u + self.n_p
        self.dofs = dofs
        self.rank, self.world = rank, world
        N2, dN2, N1, w = _cd(tables.N2), _cd(tables.dN2), _cd(tables.N1), _cd(tables.weights)
        self._ck(L.nsx_set_tables(self._h, tables.n_q, tables.n_p2, tables.n_p1, _d(N2), _d(dN2), _d(N1), _d(w)))
        if inner_precision is not None:
            self.set_inner_precision(inner_precision)
        if layout:
            self.set_internal_layout(*layout)
        if world == 1:
            cd, cc = _ci(dofs.cell_dofs), _cd(dofs.cell_coords)
            self._ck(L.nsx_set_mesh(self._h, dofs.n_cells, dofs.dofs_per_cell, _i(cd), _d(cc), dofs.n_u, dofs.n_p))
            if dofs.n_subdomains > 1:
                self.set_ranks(dofs.owned_u_ptr, dofs.owned_p_ptr)
            return
        v = dofs.rank_view(rank, world)
        self.view = v
        cd, cc = _ci(v["cell_dofs"]), _cd(v["cell_coords"])
        arrs = [_ci(v[k]) for k in ("gpu_u_ptr", "gpu_p_ptr", "neighbors", "send_u_ptr", "send_u_nodes", "send_p_ptr", "send_p_nodes")]
        self._ck(L.nsx_set_mesh_distributed(self._h, v["n_cells"], v["n_cells_layer1"], dofs.dofs_per_cell, _i(cd), _d(cc),
                                            dofs.n_u, dofs.n_p, world, rank, _i(arrs[0]), _i(arrs[1]), len(arrs[2]), _i(arrs[2]),
                                            _i(arrs[3]), _i(arrs[4]), _i(arrs[5]), _i(arrs[6])))
        if len(v["rank_u_ptr"]) > 2:  # one rank of the caller per GPU is the handle's default table
            self.set_ranks(v["rank_u_ptr"], v["rank_p_ptr"])
        if comm == "callbacks":
            self._cb = gloo_callbacks()           # keep the CFUNCTYPE objects alive
            self._ck(L.nsx_comm_init_callbacks(self._h, rank, world, self._cb[0], self._cb[1], None))
        else:
            import torch.distributed as dist
            ident = (C.c_uint8 * 128)()
            if rank == 0:
                self._ck(L.nsx_comm_unique_id(ident))
            box = [bytes(ident)]
            dist.broadcast_object_list(box, src=0)
            ident = (C.c_uint8 * 128).from_buffer_copy(box[0])
            self._ck(L.nsx_comm_init(self._h, rank, world, ident))

    def persistent_state(self):
        """dict: sweep / cg on their single-launch path, time-outs so far, non-empty mailbox words (nsx_persistent_state)"""
        st = (C.c_int * 4)()
        self._ck(self.L.nsx_persistent_state(self._h, st))
        return {"sweep_persistent": bool(st[0]), "cg_persistent": bool(st[1]), "fallbacks": int(st[2]), "dirty_mailbox_words": int(st[3])}

    PATH_KEYS = ("spmv_lds_staged", "spmv_chunks", "spmv_chunks_behind_halo", "sweep_entries_per_thread", "sweep_grid", "sweep_collective_inside",
                 "sweep_entries_per_thread_max", "cus_reserved", "schur_cg_path", "schur_blocks", "neighbours", "nodes_sent_per_exchange", "ghost_nodes",
                 "schur_dense_inverses", "sweep_off", "fallbacks", "rccl_sweep_velocity_plain", "rccl_sweep_velocity_masked", "rccl_sweep_block_plain",
                 "rccl_sweep_block_masked", "schur_blocks_per_partial", "sweep_velocity_one_gpu", "owned_p2_nodes", "owned_p1_nodes", "sweep_with_ilu_inside", "fused_launches",
                 "inner_F_fp32", "ilu_F_fp32", "schur_cg_rows_per_lane_group", "schur_cg_operator_in_lds",
                 "spmv_max_chunk_rows", "spmv_max_staged_columns")

    def path_info(self):
        """dict: which code paths the handle's products and solves take (nsx_path_info; schur_cg_path: 1 launch per operation,
        2 persistent, 3 two launches per iteration)"""
        v = (C.c_int * 32)()
        self._ck(self.L.nsx_path_info(self._h, v))
        return {k: int(v[i]) for i, k in enumerate(self.PATH_KEYS)}

    ILU_PATH_KEYS = ("factor", "invert", "solve", "entries_per_tick", "slabs_per_set", "ncomp", "float_stream", "waves", "blocks", "max_block_rows",
                     "max_block_nnz", "max_wave_rows", "levelled", "lane_stream", "dense_inverses", "factor_lds_bytes")
    ILU_FACTOR = {0: None, 1: "level", 2: "lds", 3: "dense_row", 4: "general"}
    ILU_INVERT = {0: None, 1: "lds", 2: "global"}
    ILU_SOLVE = {0: None, 1: "levelled", 2: "dense", 3: "lanes", 4: "block_lds", 5: "block_global"}

    def ilu_path_info(self, which):
        """dict: the kernels the ILU(0) of F (which = 0) / of the Schur matrix (1) ran (nsx_ilu_path_info): the factorisation and
        inversion kernels of the last initialisation and the kernel of the last triangular solve by name, the stream's parameters and
        the schedule's sizes"""
        v = (C.c_int * 16)()
        self._ck(self.L.nsx_ilu_path_info(self._h, int(which), v))
        d = {k: int(v[i]) for i, k in enumerate(self.ILU_PATH_KEYS)}
        d["factor"], d["invert"], d["solve"] = self.ILU_FACTOR[d["factor"]], self.ILU_INVERT[d["invert"]], self.ILU_SOLVE[d["solve"]]
        return d

    def ilu_invert_staged(self, which):
        """whether the last inversion in LDS on that schedule read the factor from its LDS copy (nsx_ilu_invert_staged)"""
        v = C.c_int(0)
        self._ck(self.L.nsx_ilu_invert_staged(self._h, int(which), C.byref(v)))
        return bool(v.value)

    SCHUR_PLAN_KEYS = ("planned", "used", "entries", "matches", "words", "bytes", "max_row", "build_us")

    def schur_plan_info(self):
        """dict: the plan of the Schur product and whether the last product ran the planned kernel (nsx_schur_plan_info)"""
        v = (C.c_longlong * 8)()
        self._ck(self.L.nsx_schur_plan_info(self._h, v))
        return {k: int(v[i]) for i, k in enumerate(self.SCHUR_PLAN_KEYS)}

    def comm_counters(self):
        """(all-reduces, ghost exchanges) issued since the communicator was set"""
        c = (C.c_longlong * 2)()
        self._ck(self.L.nsx_comm_counters(self._h, c))
        return int(c[0]), int(c[1])

    def comm_self_halo_test(self, n_own, n_ghost, ncomp):
        """largest error of a self-addressed RCCL ghost exchange (nsx_comm_self_halo_test; needs comm_init_single)"""
        e = C.c_double(0.0)
        self._ck(self.L.nsx_comm_self_halo_test(self._h, int(n_own), int(n_ghost), int(ncomp), C.byref(e)))
        return float(e.value)

    def comm_init_single(self):
        """1-rank RCCL communicator on this handle: every dot product then goes through ncclAllReduce (API self-test)."""
        ident = (C.c_uint8 * 128)()
        self._ck(self.L.nsx_comm_unique_id(ident))
        self._ck(self.L.nsx_comm_init(self._h, 0, 1, ident))

    def gather_solution(self):
        """Global solution vector on every rank (owned parts summed over the process group)."""
        x = np.zeros(self.n)
        self._ck(self.L.nsx_get_solution(self._h, _d(x)))
        if self.world > 1:
            import torch
            import torch.distributed as dist
            t = torch.from_numpy(x)
            if dist.get_backend() == "nccl":
                t = t.cuda()
            dist.all_reduce(t)
            x = t.cpu().numpy()
        return x

    def _ck(self, rc):
        if rc:
            raise NsxError(rc, (self.L.nsx_last_error(self._h) or b"").decode())

    def close(self):
        if self._h:
            self.L.nsx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- setup ---------------------------------------------------------------------------------
    def set_ranks(self, u_ptr, p_ptr):
        u_ptr, p_ptr = _ci(u_ptr), _ci(p_ptr)
        self._ck(self.L.nsx_set_ranks(self._h, len(u_ptr) - 1, _i(u_ptr), _i(p_ptr)))

    def set_internal_layout(self, n_virtual_ranks, order=COLOUR, schur_max_rows=0):
        self._ck(self.L.nsx_set_internal_layout(self._h, int(n_virtual_ranks), int(order), int(schur_max_rows)))

    def set_inner_precision(self, precision):
        """INNER_FP64 / INNER_FP32 (nsx_set_inner_precision); takes effect with the next prec_initialize / solve_time_step"""
        self._ck(self.L.nsx_set_inner_precision(self._h, int(precision)))

    def layout_info(self):
        info = (C.c_int * 5)()
        self._ck(self.L.nsx_layout_info(self._h, info))
        return {"on": bool(info[0]), "ranks": int(info[1]), "schur_blocks": int(info[2]), "colours": int(info[3]), "colours_p": int(info[4])}

    def layout(self):
        """node_perm / pnode_perm (owned caller node -> internal node, global ids), u_ptr / p_ptr / schur_ptr (nsx_layout_get)"""
        info = self.layout_info()
        if self.world == 1:
            n2, n1 = self.n_u // self.dim, self.n_p
        else:
            n2 = int(self.view["gpu_u_ptr"][self.rank + 1] - self.view["gpu_u_ptr"][self.rank])
            n1 = int(self.view["gpu_p_ptr"][self.rank + 1] - self.view["gpu_p_ptr"][self.rank])
        out = {"node_perm": np.empty(n2, np.int32), "pnode_perm": np.empty(n1, np.int32), "u_ptr": np.empty(info["ranks"] + 1, np.int32),
               "p_ptr": np.empty(info["ranks"] + 1, np.int32), "schur_ptr": np.empty(info["schur_blocks"] + 1, np.int32)}
        self._ck(self.L.nsx_layout_get(self._h, *[_i(out[k]) for k in ("node_perm", "pnode_perm", "u_ptr", "p_ptr", "schur_ptr")]))
        out.update(info)
        return out

    def set_schur_blocks(self, p_ptr):
        p_ptr = _ci(p_ptr)
        self._ck(self.L.nsx_set_schur_blocks(self._h, len(p_ptr) - 1, _i(p_ptr)))

    # -- state ---------------------------------------------------------------------------------
    def set_solution(self, v):
        v = _cd(v)
        assert v.shape == (self.n,)
        self._ck(self.L.nsx_set_solution(self._h, _d(v)))

    def _get(self, fn):
        v = np.zeros(self.n)
        self._ck(fn(self._h, _d(v)))
        return v

    @property
    def solution_owned(self):
        return self._get(self.L.nsx_get_solution)

    @property
    def solution(self):
        return self._get(self.L.nsx_get_solution_ghosted)

    @property
    def rhs(self):
        return self._get(self.L.nsx_get_rhs)

    def set_rhs(self, v):
        v = _cd(v)
        self._ck(self.L.nsx_set_rhs(self._h, _d(v)))

    # -- hot path ------------------------------------------------------------------------------
    def assemble(self, flags=0):
        self._ck(self.L.nsx_assemble(self._h, flags))

    def assemble_time_step(self, flags=0):
        self._ck(self.L.nsx_assemble_time_step(self._h, flags))

    def add_rhs(self, dofs, vals):
        dofs, vals = _ci(dofs), _cd(vals)
        self._ck(self.L.nsx_add_rhs(self._h, len(dofs), _i(dofs), _d(vals)))

    def apply_boundary_values(self, dofs, vals):
        dofs, vals = _ci(dofs), _cd(vals)
        self._ck(self.L.nsx_apply_boundary_values(self._h, len(dofs), _i(dofs), _d(vals)))

    def solve_time_step(self, prec=YOSIDA, tol_abs=1e-4, inner_rtol=1e-2, maxiter=100000, inner_maxiter=100000,
                        check=True):
        st = Stats()
        rc = self.L.nsx_solve_time_step(self._h, prec, tol_abs, inner_rtol, maxiter, inner_maxiter, C.byref(st))
        if rc and (check or rc != -4):
            self._ck(rc)
        return st.as_dict()

    def prec_initialize(self, prec):
        self._ck(self.L.nsx_prec_initialize(self._h, prec))

    def prec_vmult(self, prec, src, inner_rtol=1e-2, inner_maxiter=100000, dst0=None):
        src = _cd(src)
        dst = np.zeros_like(src) if dst0 is None else _cd(dst0).copy()
        st = Stats()
        self._ck(self.L.nsx_prec_vmult(self._h, prec, inner_rtol, inner_maxiter, _d(dst), _d(src), C.byref(st)))
        return dst, st.as_dict()

    def system_vmult(self, src):
        src = _cd(src)
        dst = np.zeros_like(src)
        self._ck(self.L.nsx_system_vmult(self._h, _d(dst), _d(src)))
        return dst

    def inner_F_vmult(self, src):
        """F src exactly as the inner GMRES computes it, in the handle's inner precision (nsx_inner_F_vmult; after prec_initialize)"""
        src = _cd(src)
        dst = np.empty_like(src)
        self._ck(self.L.nsx_inner_F_vmult(self._h, _d(dst), _d(src)))
        return dst

    def sparse_product(self, op, x, aux=None):
        """nsx_sparse_product: one sparse product of the solver (PROD_*) on block vectors of length n_u + n_p, by the function the solver
        calls; the entries the op does not produce are 0.  In a multi-process run the vectors are globally indexed, every rank calls, and
        the entries this rank does not own come back as 0 (sum over the ranks for the whole vector)."""
        x = _cd(x)
        aux = None if aux is None else _cd(aux)
        assert x.shape == (self.n,) and (aux is None or aux.shape == (self.n,))
        dst = np.zeros_like(x)
        self._ck(self.L.nsx_sparse_product(self._h, int(op), _d(dst), _d(x), None if aux is None else _d(aux)))
        return dst

    def prec_vector(self, which):
        """nsx_prec_get_vector: one vector of the preconditioner set-up (PREC_VEC_*) as the last prec_initialize left it, length n_u in the
        caller's numbering.  Distributed handles: global-sized, the entries this rank owns filled, the rest 0."""
        v = np.zeros(self.n_u)
        self._ck(self.L.nsx_prec_get_vector(self._h, int(which), _d(v)))
        return v

    def ilu_apply(self, which, src):
        src = _cd(src)
        dst = np.empty_like(src)
        self._ck(self.L.nsx_ilu_apply(self._h, which, _d(dst), _d(src)))
        return dst

    def schur_cg(self, b, x0=None, rtol=1e-2, maxiter=100000):
        """nsx_schur_cg: one CG solve of negative_S_tilde x = b from the guess x0 (default 0) with tolerance rtol * |b|, by the function
        the preconditioners call (after prec_initialize).  Returns (x, steps, last_residual, status); status 0 converged, 1 not.
        Vectors of length n_p in the caller's numbering; in a multi-process run globally indexed, every rank calls, and the entries of x
        this rank does not own come back as 0 (sum over the ranks for the whole vector)."""
        b = _cd(b)
        x = np.zeros_like(b) if x0 is None else _cd(x0).copy()
        assert b.shape == (self.n_p,) and x.shape == (self.n_p,)
        steps, status, last = C.c_int(), C.c_int(), C.c_double()
        self._ck(self.L.nsx_schur_cg(self._h, float(rtol), int(maxiter), _d(x), _d(b), C.byref(steps), C.byref(last), C.byref(status)))
        if self.world > 1:
            lo, hi = int(self.view["gpu_p_ptr"][self.rank]), int(self.view["gpu_p_ptr"][self.rank + 1])
            x[:lo] = 0.0
            x[hi:] = 0.0
        return x, steps.value, last.value, status.value

    def gram_schmidt_cycle(self, vectors, norm_guard=-1.0):
        """nsx_gram_schmidt_cycle: (orthonormalised vectors, coefficients [m][m], |w|^2 after each sweep)"""
        v = np.ascontiguousarray(vectors, dtype=np.float64).copy()
        m, n = v.shape
        coeffs, norms2 = np.zeros((m, m)), np.zeros(m)
        self._ck(self.L.nsx_gram_schmidt_cycle(self._h, n, m, _d(v), float(norm_guard), _d(coeffs), _d(norms2)))
        return v, coeffs, norms2

    SWEEP_CONSIDER, SWEEP_NO_NORMALIZE = 1, 2  # flags of nsx_gram_schmidt_sweeps

    def gram_schmidt_sweeps(self, vectors, split=None, gap=0, norm_guard=-1.0, flags=0):
        """nsx_gram_schmidt_sweeps on vectors[m][n + gap] in the device layout of a Span(n, split, gap): (vectors after the cycle
        in the same layout, coefficients [m][m], |w|^2 after each sweep, |w|^2 before it (flags & SWEEP_CONSIDER), whether the
        sweep normalised the vector itself)"""
        v = np.ascontiguousarray(vectors, dtype=np.float64).copy()
        m, n = v.shape[0], v.shape[1] - int(gap)
        split = n if split is None else int(split)
        coeffs, norms2, before, normalized = np.zeros((m, m)), np.zeros(m), np.zeros(m), np.zeros(m, dtype=np.int32)
        self._ck(self.L.nsx_gram_schmidt_sweeps(self._h, n, split, int(gap), m, _d(v), float(norm_guard), int(flags), _d(coeffs), _d(norms2),
                                                _d(before), _i(normalized)))
        return v, coeffs, norms2, before, normalized

    def gmres(self, system, mode, b, x0=None, tol=1e-2, maxiter=100000, neg_out=None, abs_tol=False):
        """nsx_gmres: one GMRES solve of an inner system (GMRES_F / GMRES_S) by the call site `mode` names, from the guess x0 (default 0).
        Returns a dict: x, neg_out (None unless given), steps, status, x_written, neg_done, last_residual."""
        b = _cd(b)
        x = np.zeros_like(b) if x0 is None else _cd(x0).copy()
        y = None if neg_out is None else _cd(neg_out).copy()
        n = self.n_u if system == GMRES_F else self.n_p
        assert b.shape == (n,) and x.shape == (n,) and (y is None or y.shape == (n,))
        info, last = (C.c_int * 4)(), C.c_double()
        self._ck(self.L.nsx_gmres(self._h, int(system), int(mode) | (GMRES_ABS_TOL if abs_tol else 0), float(tol), int(maxiter), _d(x), _d(b),
                                  None if y is None else _d(y), info, C.byref(last)))
        return {"x": x, "neg_out": y, "steps": int(info[0]), "status": int(info[1]), "x_written": int(info[2]), "neg_done": int(info[3]),
                "last_residual": last.value}

    def blas1_run(self, vectors, ops, split=None, gap=0):
        """nsx_blas1_run: a program of BLAS-1 operations on vectors[m][n + gap] in the device layout of a Span(n, split, gap).  ops: a list
        of dicts -- "kind" (a name of BLAS1_KINDS) and the fields of nsx_blas1_op that op uses (vector indices d, v, w, x and slots num,
        den default to -1, everything else to 0; vs / coef: sequences of k entries).  Returns (vectors afterwards in the same layout,
        out[len(ops)], the values every "read" op published, in order)."""
        v = np.ascontiguousarray(vectors, dtype=np.float64).copy()
        m, n = v.shape[0], v.shape[1] - int(gap)
        split = n if split is None else int(split)
        recs = (Blas1Op * max(1, len(ops)))()
        n_read = 0
        for r, op in zip(recs, ops):
            op = dict(op)
            r.kind = BLAS1_KINDS.index(op.pop("kind"))
            r.d = r.v = r.w = r.x = r.num = r.den = -1
            vs, coef = list(op.pop("vs", ())), list(op.pop("coef", ()))
            assert len(vs) == len(coef) <= BLAS1_MAX_K
            r.k = op.pop("k", len(vs))
            for j, (i, c) in enumerate(zip(vs, coef)):
                r.vs[j], r.coef[j] = int(i), float(c)
            for key, val in op.items():
                if key not in ("d", "v", "w", "x", "slot", "num", "den", "count", "read", "n", "a", "s"):
                    raise KeyError(key)
                setattr(r, key, float(val) if key in ("a", "s") else int(val))
            if BLAS1_KINDS[r.kind] == "read":
                n_read += max(0, r.count)
        out, scalars = np.zeros(max(1, len(ops))), np.zeros(max(1, n_read))
        self._ck(self.L.nsx_blas1_run(self._h, n, split, int(gap), m, _d(v), len(ops), recs, _d(out), _d(scalars), n_read))
        return v, out[:len(ops)], scalars[:n_read]

    # -- forces --------------------------------------------------------------------------------
    def set_force_faces(self, cells, lfaces, ftab):
        """obstacle faces as (global cell id, local face); in a multi-process run only the faces of owned cells are kept."""
        cells, lfaces = np.asarray(cells), np.asarray(lfaces)
        if self.world > 1:
            n_sub = self.dofs.n_subdomains // self.world
            mine = (self.dofs.mesh.subdomain[cells] // n_sub) == self.rank
            pos = {int(c): i for i, c in enumerate(self.view["cell_ids"])}
            cells = np.array([pos[int(c)] for c in cells[mine]], dtype=np.int32)
            lfaces = lfaces[mine]
        cells, lfaces = _ci(cells), _ci(lfaces)
        N2, dN2, N1, w = _cd(ftab.N2), _cd(ftab.dN2), _cd(ftab.N1), _cd(ftab.weights[:ftab.n_qf])
        self._ck(self.L.nsx_set_force_faces(self._h, len(cells), _i(cells), _i(lfaces), ftab.n_qf, _d(N2), _d(dN2), _d(N1), _d(w)))

    def compute_forces(self):
        d, l = C.c_double(), C.c_double()
        self._ck(self.L.nsx_compute_forces(self._h, C.byref(d), C.byref(l)))
        return d.value, l.value

    # -- flow diagnostics ----------------------------------------------------------------------
    def diagnostics(self):
        """nsx_compute_diagnostics as a dict (the fields of nsx_flow_diag).  Values that are not finite raise NsxError (code -5) with
        that dict attached as `.diag`."""
        d = FlowDiag()
        rc = self.L.nsx_compute_diagnostics(self._h, C.byref(d))
        if rc == -5:
            err = NsxError(rc, (self.L.nsx_last_error(self._h) or b"").decode())
            err.diag = d.as_dict()
            raise err
        self._ck(rc)
        return d.as_dict()

    def cell_diagnostic(self, which):
        """per-cell values (DIAG_*) of the last diagnostics(), in the order of the cells handed to the handle (nsx_get_cell_diagnostic)"""
        n = self.dofs.n_cells if self.world == 1 else int(self.view["n_cells"])
        v = np.empty(n)
        self._ck(self.L.nsx_get_cell_diagnostic(self._h, int(which), _d(v)))
        return v

    # -- point probes --------------------------------------------------------------------------
    def set_probes(self, points, tol=-1.0):
        """nsx_set_probes: locate points [n][dim] once and keep them as the handle's probe set (an empty list clears it); returns the
        located `cells` (position in the cell list handed to the handle, -1: in no cell, or another rank evaluates the probe).  In a
        multi-process run every rank passes the same points, unchanged."""
        pts = _cd(points).reshape(-1, self.dim)
        self._ck(self.L.nsx_set_probes(self._h, len(pts), _d(pts), float(tol)))
        self._n_probes = len(pts)               # a refused call leaves the earlier set (and its size) in place
        return self.probe_cells()[0] if len(pts) else np.empty(0, np.int32)

    def probe_cells(self):
        """(cells [n], owners [n], lambda [n][dim+1]) of the probe set (nsx_get_probe_cells)"""
        n = getattr(self, "_n_probes", 0)
        cells, owners, lam = np.empty(n, np.int32), np.empty(n, np.int32), np.empty((n, self.dim + 1))
        self._ck(self.L.nsx_get_probe_cells(self._h, _i(cells), _i(owners), _d(lam)))
        return cells, owners, lam

    def eval_probes(self, gradient=False):
        """nsx_eval_probes on the ghosted solution: {"velocity" [n][dim], "pressure" [n], "found" [n] (bool)} and, when asked,
        "gradient" [n][dim][dim] (d_j u_i)"""
        n = getattr(self, "_n_probes", 0)
        out = {"velocity": np.empty((n, self.dim)), "pressure": np.empty(n)}
        found = np.empty(n, np.int32)
        grad = np.empty((n, self.dim, self.dim)) if gradient else None
        self._ck(self.L.nsx_eval_probes(self._h, _d(out["velocity"]), _d(out["pressure"]), _d(grad) if gradient else None, _i(found)))
        out["found"] = found.astype(bool)
        if gradient:
            out["gradient"] = grad
        return out

    # -- tracer particles ----------------------------------------------------------------------
    def set_tracers(self, points, tol=-1.0):
        """nsx_set_tracers: locate the seeds [n][dim] and make them the handle's tracer set (an empty list clears it); returns the
        statuses (TRACER_ACTIVE, or TRACER_NOT_FOUND for a seed in no cell)"""
        pts = _cd(points).reshape(-1, self.dim)
        self._ck(self.L.nsx_set_tracers(self._h, len(pts), _d(pts), float(tol)))
        self._n_tracers = len(pts)              # a refused call leaves the earlier set (and its size) in place
        return self.get_tracers()["status"] if len(pts) else np.empty(0, np.int32)

    def advect_tracers(self, dt, n_substeps=1, scheme=TRACER_RK4, field=TRACER_FROZEN):
        """nsx_advect_tracers: n_substeps steps of size dt / n_substeps through u_h of the state the handle holds (TRACER_LINEAR: from
        previous_solution to solution across the call); dt < 0 traces backwards"""
        self._ck(self.L.nsx_advect_tracers(self._h, float(dt), int(n_substeps), int(scheme), int(field)))

    def get_tracers(self):
        """{"positions" [n][dim], "cells" [n], "status" [n], "exit_faces" [n], "age" [n]} of the tracer set (nsx_get_tracers)"""
        n = getattr(self, "_n_tracers", 0)
        out = {"positions": np.empty((n, self.dim)), "cells": np.empty(n, np.int32), "status": np.empty(n, np.int32),
               "exit_faces": np.empty(n, np.int32), "age": np.empty(n)}
        self._ck(self.L.nsx_get_tracers(self._h, _d(out["positions"]), _i(out["cells"]), _i(out["status"]), _i(out["exit_faces"]), _d(out["age"])))
        return out

    # -- nodal fields --------------------------------------------------------------------------
    def compute_nodal_fields(self):
        """nsx_compute_nodal_fields: the recovered gradient and the fields derived from it at every owned P2 node, from the state the
        handle holds; nodal_field() hands them out"""
        self._ck(self.L.nsx_compute_nodal_fields(self._h))

    def nodal_field(self, which):
        """[n_nodes][n_components] of field `which` (FIELD_*) as the last compute_nodal_fields() left it, nodes in the caller's numbering
        (nsx_get_nodal_field).  Distributed handles: global-sized, the entries this rank owns filled, the rest 0."""
        nc = C.c_int(0)
        self._ck(self.L.nsx_nodal_field_components(self._h, int(which), C.byref(nc)))
        out = np.zeros((self.n_u // self.dim, nc.value))
        self._ck(self.L.nsx_get_nodal_field(self._h, int(which), _d(out)))
        return out

    # -- isosurfaces and slices ----------------------------------------------------------------
    def extract_isosurface(self, field, isovalue, colour=None):
        """nsx_extract_isosurface + nsx_get_isosurface: the primitives of { field = isovalue } (segments in 2D, triangles in 3D) as
        (points [n][dim][dim], colour [n][dim] or None, cells [n]); field / colour: iso_source(...).  Distributed handles: this rank's
        primitives, cells in the rank's own cell list."""
        n = C.c_int64(0)
        self._ck(self.L.nsx_extract_isosurface(self._h, C.byref(field), float(isovalue), C.byref(colour) if colour is not None else None, C.byref(n)))
        pts, cells = np.empty((n.value, self.dim, self.dim)), np.empty(n.value, np.int32)
        col = np.empty((n.value, self.dim)) if colour is not None else None
        self._ck(self.L.nsx_get_isosurface(self._h, _d(pts), _d(col) if col is not None else None, _i(cells)))
        return pts, col, cells

    # -- lattice sampling ----------------------------------------------------------------------
    def set_lattice(self, origin, spacing, counts, tol=-1.0):
        """nsx_set_lattice: the lattice x_d = origin_d + i_d * spacing_d, i_d < counts_d (x fastest), every point located once; returns
        n_found, the points that lie in a cell.  origin = spacing = counts = None clears the lattice."""
        n = C.c_int64(0)
        if origin is None and spacing is None and counts is None:
            self._ck(self.L.nsx_set_lattice(self._h, None, None, None, float(tol), C.byref(n)))
            self._lattice_counts = None
            return 0
        o, s, c = _cd(origin), _cd(spacing), _ci(counts)
        if not (o.shape == s.shape == c.shape == (self.dim,)):
            raise ValueError("origin, spacing and counts have dim = %d entries each" % self.dim)
        self._ck(self.L.nsx_set_lattice(self._h, _d(o), _d(s), _i(c), float(tol), C.byref(n)))
        self._lattice_counts = tuple(int(k) for k in c)      # a refused call leaves the earlier lattice (and its shape) in place
        return int(n.value)

    def _lattice_shape(self):
        counts = getattr(self, "_lattice_counts", None)
        return counts[::-1] if counts else (0,)

    def lattice_cells(self):
        """owning cell of every lattice point, shaped counts[::-1] (x fastest), -1: in no cell (nsx_get_lattice_cells)"""
        cells = np.empty(self._lattice_shape(), np.int32)
        self._ck(self.L.nsx_get_lattice_cells(self._h, _i(cells)))
        return cells

    def eval_lattice(self, what):
        """nsx_eval_lattice: sample `what` (an OR of LATTICE_*) from the state the handle holds; get_lattice() hands the planes out"""
        self._ck(self.L.nsx_eval_lattice(self._h, int(what)))

    def get_lattice(self, quantity, which=0):
        """[n_components, *counts[::-1]] of one quantity (LATTICE_*; which = FIELD_* for LATTICE_NODAL) as the last eval_lattice() left it:
        dim velocity components, 1 pressure, dim^2 gradient entries (row-major d_j u_i), the components of the nodal field"""
        dim = self.dim
        nc = {LATTICE_VELOCITY: dim, LATTICE_PRESSURE: 1, LATTICE_GRADIENT: dim * dim,
              LATTICE_NODAL: {FIELD_GRADIENT: dim * dim, FIELD_VORTICITY: 3 if dim == 3 else 1}.get(which, 1)}.get(quantity, 1)
        out = np.empty((nc,) + self._lattice_shape())
        self._ck(self.L.nsx_get_lattice(self._h, int(quantity), int(which), _d(out)))
        return out

    # -- running statistics --------------------------------------------------------------------
    def stats_begin(self, what=STATS_VELOCITY | STATS_PRESSURE, n_bins=1):
        """nsx_stats_begin: open an accumulation of `what` (an OR of STATS_VELOCITY, STATS_PRESSURE) with n_bins zeroed phase bins;
        what = n_bins = 0 closes it and frees its memory"""
        self._ck(self.L.nsx_stats_begin(self._h, int(what), int(n_bins)))

    def stats_accumulate(self, bin=0, weight=1.0):
        """nsx_stats_accumulate: the state the handle holds as one sample of weight `weight` into bin `bin`"""
        self._ck(self.L.nsx_stats_accumulate(self._h, int(bin), float(weight)))

    def stats_info(self):
        """{"what", "n_bins", "samples" [n_bins], "weights" [n_bins]} of the open accumulation (nsx_stats_info)"""
        what, n_bins = C.c_int(0), C.c_int(0)
        self._ck(self.L.nsx_stats_info(self._h, C.byref(what), C.byref(n_bins), None, None))
        samples, weights = np.zeros(n_bins.value, np.int64), np.zeros(n_bins.value)
        self._ck(self.L.nsx_stats_info(self._h, None, None, samples.ctypes.data_as(C.POINTER(C.c_int64)), _d(weights)))
        return {"what": what.value, "n_bins": n_bins.value, "samples": samples, "weights": weights}

    def stats_get(self, quantity, bin=-1):
        """[n_nodes][n_components] of one quantity (STATS_*) of bin `bin`, or of all non-empty bins pooled (bin = -1), nodes in the
        caller's numbering: P2 nodes for the velocity quantities, P1 nodes for the pressure's (nsx_stats_get).  Distributed handles:
        global-sized, the entries this rank owns filled, the rest 0."""
        nc = C.c_int(0)
        self._ck(self.L.nsx_stats_components(self._h, int(quantity), C.byref(nc)))
        out = np.zeros((self.n_u // self.dim if quantity < STATS_MEAN_P else self.n_p, nc.value))
        self._ck(self.L.nsx_stats_get(self._h, int(quantity), int(bin), _d(out)))
        return out

    # -- surface loads -------------------------------------------------------------------------
    def set_surface(self, cells, local_faces, groups=None, n_groups=None, form=SURFACE_SYMMETRIC, centre=None):
        """nsx_set_surface: boundary faces (position in the cell list, deal.II local face number) in groups (None: all 0; n_groups None:
        largest group + 1), the form of the viscous stress and the centre of the torque (None: origin).  No faces: clears the set.
        problem.boundary_faces() gives the three arrays.  In a multi-process run `cells` are global cell ids in ascending face order and the
        faces of the cells this rank's view holds are kept (self.surface_faces: their positions in the list handed in)."""
        cells, lf = np.asarray(cells), np.asarray(local_faces)
        gr = None if groups is None else _ci(groups)
        if n_groups is None:
            n_groups = 1 if gr is None or len(gr) == 0 else int(gr.max()) + 1
        if self.world > 1:
            pos = {int(c): i for i, c in enumerate(self.view["cell_ids"])}
            keep = np.array([k for k, c in enumerate(cells) if int(c) in pos], dtype=np.int64)
            self.surface_faces = keep
            cells, lf = np.array([pos[int(c)] for c in cells[keep]], dtype=np.int32), lf[keep]
            gr = None if gr is None else _ci(gr[keep])
        cells, lf = _ci(cells), _ci(lf)
        cen = None if centre is None else _cd(centre)
        self._ck(self.L.nsx_set_surface(self._h, len(cells), _i(cells), _i(lf), None if gr is None else _i(gr), int(n_groups), int(form),
                                        None if cen is None else _d(cen)))

    def surface_info(self):
        """dict: n_faces, n_groups, n_nodes (surface nodes), nodes_per_face (nsx_surface_info)"""
        v = (C.c_int * 4)()
        self._ck(self.L.nsx_surface_info(self._h, v))
        return {"n_faces": int(v[0]), "n_groups": int(v[1]), "n_nodes": int(v[2]), "nodes_per_face": int(v[3])}

    def surface_layout(self):
        """dict: nodes [n_nodes] (P2 node of every surface node, caller's numbering), node_groups [n_nodes], face_nodes
        [n_faces][nodes_per_face] (surface node of every face node), areas [n_faces] (nsx_get_surface_layout)"""
        i = self.surface_info()
        nodes, groups = np.zeros(i["n_nodes"], dtype=np.int32), np.zeros(i["n_nodes"], dtype=np.int32)
        fn, areas = np.zeros((i["n_faces"], i["nodes_per_face"]), dtype=np.int32), np.zeros(i["n_faces"])
        self._ck(self.L.nsx_get_surface_layout(self._h, _i(nodes), _i(groups), _i(fn), _d(areas)))
        return {"nodes": nodes, "node_groups": groups, "face_nodes": fn, "areas": areas}

    def compute_surface(self, totals=True):
        """nsx_compute_surface: evaluates every face node and surface node of the set from the state the handle holds; returns the totals
        of every group as a list of dicts (area, force_pressure [3], force_viscous [3], torque [3], flux, pressure_integral, n_faces), or
        None with totals=False (a distributed handle then issues no collective)."""
        if not totals:
            self._ck(self.L.nsx_compute_surface(self._h, None))
            return None
        t = (SurfaceTotals * self.surface_info()["n_groups"])()
        self._ck(self.L.nsx_compute_surface(self._h, t))
        return [g.as_dict() for g in t]

    def surface_field(self, which, at=SURFACE_AT_NODES):
        """one field (SURFACE_*) of the last compute_surface(): [n_faces][nodes_per_face][n_components] at = SURFACE_AT_FACES (faces in
        the caller's order), [n_nodes][n_components] at = SURFACE_AT_NODES (nsx_get_surface_field).  Distributed handles: the surface nodes
        whose P2 node the rank owns are filled, the rest 0."""
        nc = C.c_int(0)
        self._ck(self.L.nsx_surface_field_components(self._h, int(which), C.byref(nc)))
        i = self.surface_info()
        out = np.zeros((i["n_faces"], i["nodes_per_face"], nc.value) if at == SURFACE_AT_FACES else (i["n_nodes"], nc.value))
        self._ck(self.L.nsx_get_surface_field(self._h, int(which), int(at), _d(out)))
        return out

    # -- export --------------------------------------------------------------------------------
    def export_block(self, which, block, graph=None):
        """values of matrix `which` in the reference's padded block-CSR graph (default: the front-end's)."""
        rowptr, colind = graph if graph is not None else self.dofs.reference_sparsity(3 if which == 4 else block)
        rowptr, colind = _ci(rowptr), _ci(colind)
        vals = np.empty(len(colind))
        self._ck(self.L.nsx_export_block(self._h, which, block, len(rowptr) - 1, _i(rowptr), _i(colind), _d(vals)))
        return vals

    def scalar_graph(self, which):
        nnz = C.c_int64()
        self._ck(self.L.nsx_scalar_graph_nnz(self._h, which, C.byref(nnz)))
        n = (self.n_u // self.dim) if which == 0 else self.n_p
        rp, ci = np.empty(n + 1, np.int32), np.empty(nnz.value, np.int32)
        self._ck(self.L.nsx_scalar_graph(self._h, which, _i(rp), _i(ci)))
        return rp, ci

    def schur(self):
        import scipy.sparse as sp
        rp, ci = self.scalar_graph(1)
        v = np.empty(len(ci))
        self._ck(self.L.nsx_schur_get(self._h, _i(rp), _i(ci), _d(v)))
        return sp.csr_matrix((v, ci, rp), shape=(self.n_p, self.n_p))

    def ilu(self, which):
        rp, ci = self.scalar_graph(which)
        v = np.empty(len(ci))
        self._ck(self.L.nsx_ilu_get(self._h, which, _d(v)))
        return rp, ci, v

    # -- measurement ---------------------------------------------------------------------------
    def profile(self, on=True):
        self._ck(self.L.nsx_profile_enable(self._h, int(on)))

    def profile_reset(self):
        self._ck(self.L.nsx_profile_reset(self._h))

    def profile_table(self):
        out = {}
        for i in range(self.L.nsx_profile_count(self._h)):
            name, n, ms, b = C.c_char_p(), C.c_int64(), C.c_double(), C.c_double()
            self.L.nsx_profile_get(self._h, i, C.byref(name), C.byref(n), C.byref(ms), C.byref(b))
            out[name.value.decode()] = {"launches": n.value, "total_ms": ms.value, "bytes_per_launch": b.value}
        return out
