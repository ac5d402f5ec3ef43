/* nsx.h — C-ABI of libnsx.so, the MI355X (gfx950) implementation of the per-time-step hot path of
 * lelecaruso/NavierStokes_Project_NM4PDE:
 *
 *     NavierStokes::assemble(time)            reference Navier-Stokes/src/NavierStokes3D.cpp:163-356
 *     NavierStokes::assemble_time_step(time)  reference Navier-Stokes/src/NavierStokes3D.cpp:361-544
 *     NavierStokes::solve_time_step()         reference Navier-Stokes/src/NavierStokes3D.cpp:546-640
 *     Precondition{Yosida,SIMPLE,aYosida,aSIMPLE}::initialize / ::vmult
 *                                              reference Navier-Stokes/include/Preconditioners.hpp:118-534
 * (2D: src/NavierStokes2D.cpp:164-639; convergence study: src/Convergence3D.cpp:187-680.)
 *
 * The reference has no plugin / FFI layer: the seams a replacement binds to are those member functions
 * (SURVEY.md section 8b).  Every entry point below names the member (file:line) whose work it performs;
 * INTEGRATION.md shows the deal.II-side adaptor that forwards the three members to these calls.
 *
 * Conventions: extern "C"; opaque handle, one per GPU / rank; every call returns 0 (NSX_OK) or a negative
 * nsx_status, with a message available from nsx_last_error(); no exception crosses the boundary; host
 * arrays are borrowed for the duration of the call only; device memory is owned by the handle; calls on
 * one handle are not thread-safe.  Indices are int32 (as Epetra's), values are FP64.
 *
 * Numbering contract (what deal.II's DoFHandler provides after DoFRenumbering::component_wise by block,
 * reference NavierStokes3D.cpp:62-69): velocity dofs first, [0, n_u), the `dim` components of one P2 node
 * consecutive (dof = dim * node + c); pressure dofs after them, dof = n_u + p1_node.  Local dof order on a
 * cell is FESystem's: per vertex the dim velocity components then the pressure, then per line the dim
 * velocity components (34 dofs on a tetrahedron, 15 on a triangle).
 */
#ifndef NSX_H
#define NSX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nsx_handle nsx_handle;

typedef enum {
  NSX_OK = 0,
  NSX_ERR_ARG = -1,          /* bad argument / call order */
  NSX_ERR_HIP = -2,          /* HIP runtime error (message has the HIP error string) */
  NSX_ERR_UNSUPPORTED = -3,  /* valid input this build has no kernel for (e.g. quadrature size) */
  NSX_ERR_NOCONV = -4,       /* a Krylov solver hit its iteration limit: deal.II would throw SolverControl::NoConvergence */
  NSX_ERR_NUMERIC = -5,      /* NaN / zero pivot */
  NSX_ERR_COMM = -6          /* RCCL error */
} nsx_status;

/* preconditioner_type of NavierStokes::solve_time_step (reference NavierStokes3D.cpp:562-634) */
typedef enum { NSX_PREC_YOSIDA = 0, NSX_PREC_SIMPLE = 1, NSX_PREC_AYOSIDA = 2, NSX_PREC_ASIMPLE = 3 } nsx_prec;

/* assembly variants: which terms the reference's three executables put into the convection matrix */
enum {
  NSX_TEMAM = 1,             /* 0.5 (div u_n) (phi_i . phi_j): NS3D first step only (:255); NS2D / Conv every step (NS2D:446, Conv:490) */
  NSX_DOUBLE_CONVECTION = 2  /* Convergence3D.cpp:277 + :284 add the convective term twice in the first assembly */
};

typedef struct {
  int dim;          /* 2 or 3 */
  int device;       /* HIP device ordinal */
  double nu;        /* kinematic viscosity (reference NavierStokes3D.hpp:162) */
  double deltat;    /* time step (reference NavierStokes3D.hpp:191) */
} nsx_params;

typedef struct {
  int outer_iterations;    /* solver_control.last_step()  (reference NavierStokes3D.cpp:636) */
  int inner_F_iterations;  /* sum over all inner GMRES(F) solves of the step */
  int inner_S_iterations;  /* sum over all inner CG / GMRES(S) solves of the step */
  int n_F_solves, n_S_solves;
  double final_residual;   /* last preconditioned residual norm seen by the outer GMRES */
  double t_prec;           /* seconds, preconditioner initialize (reference NavierStokes3D.cpp:558-572, time_prec) */
  double t_solve;          /* seconds, outer solve               (reference NavierStokes3D.cpp:573-577, time_solve) */
  int status;              /* 0 ok, 1 outer GMRES not converged, 2 an inner solve not converged */
  int persistent_fallbacks; /* persistent kernels (Gram-Schmidt sweep, Schur CG) that timed out on this handle SO FAR because their grid was
                            * not co-resident; the handle then stays on the launch-per-operation path.  0 in a healthy run. */
} nsx_solve_stats;

/* ---- life cycle ---- */
int nsx_create(const nsx_params *params, nsx_handle **out);
int nsx_destroy(nsx_handle *h);
const char *nsx_last_error(const nsx_handle *h); /* h may be NULL: error of the last failed nsx_create */
const char *nsx_version(void);

/* ---- setup: the outputs of NavierStokes::setup() (reference NavierStokes3D.cpp:2-157) ---- */

/* FEValues tables on the reference cell, as data (reference NavierStokes3D.cpp:31-50, 172-175):
 * scalar P2 values N2[n_q][n_p2], reference gradients dN2[n_q][n_p2][dim], scalar P1 values N1[n_q][n_p1],
 * quadrature weights w[n_q] (sum = volume of the reference simplex).  n_p2 = 6/10, n_p1 = 3/4. */
int nsx_set_tables(nsx_handle *h, int n_q, int n_p2, int n_p1, const double *N2, const double *dN2,
                   const double *N1, const double *weights);

/* Mesh + DoF tables: cell->get_dof_indices for every locally owned cell (reference NavierStokes3D.cpp:304,494)
 * and the cell's vertex coordinates (affine map).  Builds the sparsity graphs of the three blocks
 * (reference NavierStokes3D.cpp:109-124) internally.  cell_dofs[n_cells][dofs_per_cell], cell_coords[n_cells][dim+1][dim]. */
int nsx_set_mesh(nsx_handle *h, int n_cells, int dofs_per_cell, const int32_t *cell_dofs, const double *cell_coords,
                 int n_u, int n_p);

/* MPI-rank structure of the run being reproduced: velocity P2-node ranges u_ptr[n_ranks+1] and P1-node
 * ranges p_ptr[n_ranks+1] owned by each rank.  They define (a) the blocks of the per-rank Ifpack ILU(0)
 * (TrilinosWrappers::PreconditionILU, overlap 0: reference Preconditioners.hpp:215-216 and SURVEY D4) and
 * (b) the per-rank diagonal scan of MatrixTools::apply_boundary_values.  Default: one rank.
 * On one GPU this lets the ILU run as n_ranks independent triangular solves, exactly what `mpirun -n n_ranks`
 * of the reference computes. */
int nsx_set_ranks(nsx_handle *h, int n_ranks, const int32_t *u_ptr, const int32_t *p_ptr);
/* Optional: coarser blocks for the Schur-complement ILU (unions of consecutive ranks); default = the ranks. */
int nsx_set_schur_blocks(nsx_handle *h, int n_blocks, const int32_t *p_ptr);

/* The numbering libnsx works in BEHIND this boundary.  The reference numbers its DoFs with distribute_dofs +
 * DoFRenumbering::component_wise on a METIS partition into mpi_size parts (reference NavierStokes3D.cpp:16-19,58-69) and a caller
 * hands exactly that over (nsx_set_mesh, nsx_set_ranks).  The triangular solves of the per-rank ILU(0) want thousands of small,
 * spatially compact rank blocks with a shallow dependency graph inside each; with this call libnsx builds them itself:
 * inside the node range of EVERY rank of the caller the cells are bisected (coordinates of their centroids) into virtual ranks --
 * n_virtual_ranks over the whole handle, dealt to the caller's ranks in proportion to their nodes --, a node belongs to the lowest
 * virtual rank touching it (deal.II's rule), nodes are numbered virtual rank by virtual rank in first-touch order (cell by cell,
 * vertices then lines) and, for NSX_ORDER_COLOUR, sorted by a greedy colouring of the rank's P2 graph (NSX_ORDER_COLOUR_ALL: the
 * pressure nodes as well, on the graph of the Schur complement).  schur_max_rows > 0 merges consecutive virtual ranks into Schur
 * ILU blocks of at most that many pressure rows (on one handle a block may span two ranks of the caller; nothing spans handles);
 * 0: one block per virtual rank.
 * What the library then computes is what the reference computes on n_virtual_ranks MPI ranks with that numbering (per-rank ILU(0),
 * per-rank diagonal of apply_boundary_values).  NOTHING changes at the boundary: every vector, dof list, graph and value array that
 * crosses it stays in the caller's numbering (permuted on the device on the way in and out).
 * Call order: any time before nsx_assemble -- before nsx_set_mesh (one set-up pass) or after it and after nsx_set_ranks (the set-up
 * products are rebuilt; state vectors are reset).  nsx_set_ranks afterwards lays the nodes out again inside the new ranges;
 * nsx_set_schur_blocks is refused while a layout is in force.  n_virtual_ranks = 0 switches the layout off. */
enum { NSX_ORDER_FIRST_TOUCH = 0, NSX_ORDER_COLOUR = 1, NSX_ORDER_COLOUR_ALL = 2 };
int nsx_set_internal_layout(nsx_handle *h, int n_virtual_ranks, int order, int schur_max_rows);
/* info = {layout in force (0/1), ranks the ILU(0) of system(0,0) runs on, Schur ILU blocks, colours of the P2 nodes, colours of the P1 nodes} */
int nsx_layout_info(nsx_handle *h, int info[5]);
/* The layout itself, for tests and tools (any pointer may be NULL): node_perm[i] / pnode_perm[i] = internal (global) number of the
 * i-th P2 / P1 node this handle owns, u_ptr / p_ptr [info[1] + 1] the internal node ranges of the ranks, schur_ptr [info[2] + 1]. */
int nsx_layout_get(nsx_handle *h, int32_t *node_perm, int32_t *pnode_perm, int32_t *u_ptr, int32_t *p_ptr, int32_t *schur_ptr);

/* ---- state ---- */
/* `solution` (ghosted) and `solution_owned` (reference NavierStokes3D.hpp:245-248), length n_u + n_p. */
int nsx_set_solution(nsx_handle *h, const double *solution_owned);  /* also does solution = solution_owned (NavierStokes3D.cpp:696-697) */
int nsx_get_solution(nsx_handle *h, double *solution_owned);
int nsx_get_solution_ghosted(nsx_handle *h, double *solution);
int nsx_get_rhs(nsx_handle *h, double *system_rhs);
int nsx_set_rhs(nsx_handle *h, const double *system_rhs);

/* ---- the hot path ---- */

/* NavierStokes::assemble(time) without its Dirichlet block (reference NavierStokes3D.cpp:163-324):
 * mass/deltat, nu*stiffness, convection(u_n) (+Temam), -B^T / B, pressure mass; system = blocks + M + C + K; rhs.
 * As the run's set-up step it also builds the ILU schedules for the current rank / Schur block tables (host work, once). */
int nsx_assemble(nsx_handle *h, int flags);
/* NavierStokes::assemble_time_step(time) without its Dirichlet block (reference NavierStokes3D.cpp:361-512):
 * new convection(u_n) and rhs; system = system - C_old + C_new. */
int nsx_assemble_time_step(nsx_handle *h, int flags);
/* system_rhs.add(dof_indices, cell_rhs) for terms integrated by the caller (Neumann face term, Convergence3D.cpp:309-331). */
int nsx_add_rhs(nsx_handle *h, int n, const int32_t *dofs, const double *values);
/* MatrixTools::apply_boundary_values(boundary_values, system_matrix, solution, system_rhs, false)
 * (reference NavierStokes3D.cpp:353,541).  (dofs[k], values[k]) is the std::map, sorted by dof; every component
 * of a constrained P2 node must be present (the reference's ComponentMask always selects all of them). */
int nsx_apply_boundary_values(nsx_handle *h, int n, const int32_t *dofs, const double *values);
/* NavierStokes::solve_time_step() (reference NavierStokes3D.cpp:546-640): previous_solution = solution;
 * preconditioner.initialize(...); SolverGMRES(solver_control(maxiter, tol_abs)).solve(system_matrix,
 * solution_owned, system_rhs, preconditioner); solution = solution_owned.
 * Reference values: tol_abs = 1e-4, inner_rtol = 1e-2, maxiter = 100000, inner_maxiter = 100000 (10000 for (a)SIMPLE). */
int nsx_solve_time_step(nsx_handle *h, int prec_type, double tol_abs, double inner_rtol, int maxiter,
                        int inner_maxiter, nsx_solve_stats *stats);

/* Pieces of solve_time_step, exposed for parity tests and for callers that drive deal.II's own SolverGMRES
 * through the preconditioner concept (initialize / vmult, reference Preconditioners.hpp:122-126,152-153). */
int nsx_prec_initialize(nsx_handle *h, int prec_type);
int nsx_prec_vmult(nsx_handle *h, int prec_type, double inner_rtol, int inner_maxiter, double *dst, const double *src,
                   nsx_solve_stats *stats);
int nsx_system_vmult(nsx_handle *h, double *dst, const double *src); /* BlockSparseMatrix::vmult, host vectors n_u+n_p */
/* One PreconditionILU::vmult with the factors of the last initialize: which = 0 (F, length n_u; read in the handle's inner precision)
 * or 1 (S, length n_p). */
int nsx_ilu_apply(nsx_handle *h, int which, double *dst, const double *src);

/* ---- inner precision (opt-in) ---- */
/* How the two value streams of the INNER solves on the velocity block are stored.  NSX_INNER_FP64 (default): as doubles.  NSX_INNER_FP32:
 * (1) the scalar velocity operator F as read by every F->vmult inside a preconditioner's vmult (the operator of the inner GMRES,
 * reference Preconditioners.hpp:173,273,382,405, and aYosida's F->vmult(yu,yu), :507) and (2) the off-diagonal entries of ILU(0)(F) in the
 * stream of the triangular solves (-L and -U/d) are stored and read as float; the inverse pivots 1/d stay double.  Everything is still
 * COMPUTED in double, and everything else stays double: system_matrix.vmult of the outer GMRES, the right-hand side, the factorisation
 * itself (factorised in double, rounded when the stream is written), the Schur complement, its factors and its CG, block(0,1) /
 * block(1,0), all vectors, the Krylov bases, every reduction.  The linear system that is solved is unchanged; only the preconditioner
 * differs, by the rounding of its data: NSX_INNER_FP32 computes what NSX_INNER_FP64 computes on (double)(float)value.
 * The float copy of F and the float stream are written by nsx_prec_initialize from the F of that moment (the factors have always been
 * those of the last initialisation; in NSX_INNER_FP32 the F of the inner products is, too: a later assembly or nsx_apply_boundary_values
 * reaches them with the next initialisation, which every nsx_solve_time_step performs).
 * Allowed any time after nsx_create; the preconditioner has to be initialised again afterwards (nsx_solve_time_step does; a
 * nsx_prec_vmult before the next nsx_prec_initialize is the usual call-order error).  Unknown value: NSX_ERR_ARG.  A value of F or of its
 * factors that is not finite as a float fails the initialisation with NSX_ERR_NUMERIC.
 * Environment: NSX_INNER_PRECISION = fp32 | fp64 is read once by nsx_create as the handle's initial value (anything else: nsx_create fails
 * with NSX_ERR_ARG).
 * Paths without a float twin read the double values and say so (nsx_path_info [26], [27]): the plain velocity SpMV (no LDS-staged
 * chunks), the level-per-launch and the workgroup-per-block triangular solves; the fused kernel of NSX_ILU_MGS=1 is not used. */
enum { NSX_INNER_FP64 = 0, NSX_INNER_FP32 = 1 };
int nsx_set_inner_precision(nsx_handle *h, int precision);
/* Test hook: dst = F src exactly as the inner GMRES computes it (Preconditioners.hpp:382), in the handle's current inner precision; host
 * vectors of length n_u in the caller's numbering, single-process handles, after nsx_prec_initialize. */
int nsx_inner_F_vmult(nsx_handle *h, double *dst, const double *src);
/* Test hook: ONE SolverCG<Vector>(SolverControl(maxiter, rtol * |b|)).solve(negative_S_tilde, x, b, preconditioner_S) on the caller's
 * vectors (Preconditioners.hpp:179-182,388-390,500-502), by the very function the preconditioners' vmult calls: the persistent kernel
 * where the layout allows it, else two launches per iteration, else one launch per operation (nsx_path_info [8], [28], [29] say which).
 * x: initial guess in, iterate out; steps / last_residual / status (0 converged, 1 not converged) as SolverControl leaves them.
 * Single-process handles (with or without a 1-rank communicator): x and b have length n_p, in the caller's numbering.  Distributed
 * handles: length n_p of the whole mesh, globally indexed as for nsx_system_vmult; every rank calls, only the owned entries of b and x
 * are read and only the owned entries of x are written.  After nsx_prec_initialize (otherwise the usual call-order NSX_ERR_ARG). */
int nsx_schur_cg(nsx_handle *h, double rtol, int maxiter, double *x, const double *b, int *steps, double *last_residual, int *status);
/* Test hook: ONE SolverGMRES solve of an inner system on the caller's vectors, by the very call sites the preconditioners' vmult uses
 * (gmres() in csrc/nsx_solve.hip: Arnoldi with the Gram-Schmidt sweep, SolverGMRES' re-orthogonalisation test on every fifth iteration,
 * Givens rotations, restart after 28 iterations, and the seams of NSX_STEP_FUSED).
 *   system  NSX_GMRES_F   F in the handle's inner precision with the velocity ILU(0), vectors of length n_u   (Preconditioners.hpp:173,273,382,405)
 *           NSX_GMRES_S   negative_S_tilde with its ILU(0), vectors of length n_p (aSIMPLE, :287-289); modes PLAIN and FUSED_GUESS only
 *   mode    NSX_GMRES_PLAIN           x = the guess; tolerance tol * |b|, |b| through a reduction and a host round trip of its own
 *           NSX_GMRES_FUSED_GUESS     the same solve with |b|^2 collected together with the first residual norm and the residual of a cycle
 *                                     from the product's own launch
 *           NSX_GMRES_FUSED_FROM_X0   x = the guess, handed to the solver in a vector of its own: x itself is only written (by the first
 *                                     update, x = x0 + sum; if the guess converges as it stands, by a copy: info[2] = 0)
 *           NSX_GMRES_ZERO            x is zeroed and the solver told so (the first residual is b)
 *           NSX_GMRES_FUSED_ZERO_NEG  the solver told that x is zero WITHOUT x being zeroed; if the solve ends in its first cycle, the update
 *                                     is neg_out = -neg_out + x without x ever being stored (info[3] = 1, x comes back as it went in);
 *                                     else x holds the solution (info[2] = 1, neg_out untouched)
 *           | NSX_GMRES_ABS_TOL       (PLAIN, ZERO) tol is the tolerance itself: tol = 0 with maxiter = k pins iterate k (the fused modes take
 *                                     tol * |b| on the device; tol = 0 pins there too)
 * info[0] steps, [1] status (0 converged, 1 not), [2] x_written, [3] neg_done; last_residual as SolverControl leaves it: the estimate
 * |gamma| inside a cycle, the true preconditioned residual at a restart.  Single-process handles (with or without a 1-rank communicator), in
 * the caller's numbering; distributed handles are not supported (NSX_ERR_UNSUPPORTED).  After nsx_prec_initialize. */
enum { NSX_GMRES_F = 0, NSX_GMRES_S = 1 };
enum { NSX_GMRES_PLAIN = 0, NSX_GMRES_FUSED_GUESS, NSX_GMRES_FUSED_FROM_X0, NSX_GMRES_ZERO, NSX_GMRES_FUSED_ZERO_NEG, NSX_GMRES_ABS_TOL = 256 };
int nsx_gmres(nsx_handle *h, int system, int mode, double tol, int maxiter, double *x, const double *b, double *neg_out, int info[4],
              double *last_residual);
/* Test hook: ONE sparse product of the solver on the caller's vectors, by the very function the solver calls (csrc/nsx_sparse.hip), so
 * that each product kernel can be compared with a reference on its own (tests/test_gpu_sparse.py).  dst, src and aux are host vectors of
 * length n_u + n_p of the whole mesh, globally indexed exactly as for nsx_system_vmult; x_u / x_p are the velocity / pressure part of src.
 * Works on single-process and on distributed handles (every rank calls; the ghosts travel through the halo exchange of the product); a
 * distributed handle writes only its owned entries of dst.  The entries `op` does not produce come back 0.  aux may be NULL where unused.
 *   NSX_PROD_F          y_u = F x_u                          spmv_F on F as assembled (system_matrix.vmult's velocity block)
 *   NSX_PROD_F_INNER    y_u = F x_u                          spmv_F_inner: F in the handle's inner precision (as nsx_inner_F_vmult)
 *   NSX_PROD_F_RESID    y_u = aux_u - F x_u                  spmv_F_inner_resid: the residual of an inner solve's cycle
 *   NSX_PROD_MASS       y_u = (M / deltat) x_u               spmv_F on the mass values: the product that forms every right-hand side
 *   NSX_PROD_B          y_p = B x_u                          spmv_B
 *   NSX_PROD_B_MINUS_R  y_p = B x_u - aux_p                  spmv_B(.., aux, +1)
 *   NSX_PROD_R_MINUS_B  y_p = aux_p - B x_u                  spmv_B(.., aux, -1)
 *   NSX_PROD_G          y_u = G x_p                          spmv_G, overwriting       (G = block(0,1), B = block(1,0))
 *   NSX_PROD_G_ACC      y_u = aux_u + G x_p                  spmv_G accumulating onto a y preloaded with aux_u
 *   NSX_PROD_S          y_p = S x_p                          spmv_S: negative_S_tilde of the last initialisation
 *   NSX_PROD_SADDLE     as nsx_system_vmult                  spmv_saddle
 * Documented bitwise identities (the fused epilogues act on the finished row sum): F_RESID == aux - F_INNER, B_MINUS_R == B - aux,
 * R_MINUS_B == aux - B, G_ACC == aux + G, and where the LDS-staged kernel runs (nsx_path_info [0]) the velocity part of SADDLE == F + G.
 * NSX_ERR_ARG: null dst / src, nothing assembled, F_INNER / F_RESID / S before nsx_prec_initialize, aux missing, unknown op.
 * nsx_path_info [26] afterwards says whether this call streamed float values. */
enum { NSX_PROD_F = 0, NSX_PROD_F_INNER, NSX_PROD_F_RESID, NSX_PROD_MASS, NSX_PROD_B, NSX_PROD_B_MINUS_R, NSX_PROD_R_MINUS_B, NSX_PROD_G,
       NSX_PROD_G_ACC, NSX_PROD_S, NSX_PROD_SADDLE, NSX_PROD_COUNT };
int nsx_sparse_product(nsx_handle *h, int op, double *dst, const double *src, const double *aux);
/* Test hook: one vector of the per-step preconditioner set-up as the last nsx_prec_initialize left it on the device, so that the diagonal,
 * its reciprocals, the lumped mass, the Schur weights and the Dirichlet mask can be compared with a reference on their own
 * (tests/test_gpu_prec_setup.py).  values: a host vector of length n_u of the whole mesh in the caller's numbering, laid out as the velocity
 * part of nsx_get_rhs; a distributed handle writes only its owned entries.  Read-only: a copy, no kernel beyond the one that undoes an
 * internal layout.
 *   NSX_PREC_VEC_D          D: diag(mass_matrix) (Yosida) or diag(F) (SIMPLE, aSIMPLE, aYosida), replicated on the dim components
 *   NSX_PREC_VEC_D_INV      1 / D
 *   NSX_PREC_VEC_NEG_D_INV  -1 / D
 *   NSX_PREC_VEC_LUMP_M     -1 / sum_j |M_ij|: written by an aYosida initialisation only, otherwise what the last one left (0 at first)
 *   NSX_PREC_VEC_SCHUR_W    the weights of the Schur product, w = -V * mask, V = -1 / D (aYosida: lump_M)
 *   NSX_PREC_VEC_DIRMASK    1 = free, 0 = row constrained by nsx_apply_boundary_values since the last nsx_assemble
 * NSX_ERR_ARG: null values, unknown `which`, before nsx_prec_initialize (DIRMASK: before the first assembly). */
enum { NSX_PREC_VEC_D = 0, NSX_PREC_VEC_D_INV, NSX_PREC_VEC_NEG_D_INV, NSX_PREC_VEC_LUMP_M, NSX_PREC_VEC_SCHUR_W, NSX_PREC_VEC_DIRMASK,
       NSX_PREC_VEC_COUNT };
int nsx_prec_get_vector(nsx_handle *h, int which, double *values);

/* ---- export in the reference's own layout (Trilinos block CSR with all velocity couplings stored) ---- */
/* which: 0 system_matrix, 1 mass_matrix, 2 convection_matrix, 3 stiffness_matrix, 4 pressure_mass
 * block: 0=(0,0) n_u x n_u, 1=(0,1) n_u x n_p, 2=(1,0) n_p x n_u, 3=(1,1) (pressure_mass only).
 * The caller passes the CSR graph it wants filled (e.g. Epetra's ExtractCrsDataPointers); entries that are
 * structural zeros in the reference (cross-component couplings) are written as 0. */
int nsx_export_block(nsx_handle *h, int which, int block, int n_rows, const int32_t *rowptr, const int32_t *colind,
                     double *values);
/* negative_S_tilde of the last initialize (reference Preconditioners.hpp:144,248,358,468): query nnz, then fetch. */
int nsx_schur_nnz(nsx_handle *h, int64_t *nnz);
int nsx_schur_get(nsx_handle *h, int32_t *rowptr, int32_t *colind, double *values);
/* ILU(0) factors of the last initialize in the compact layout of the scalar velocity graph / the Schur graph
 * (strict lower = L, diagonal = 1/d, strict upper = U/d as Ifpack stores them); graph via nsx_scalar_graph.  Always the double factors,
 * whatever the inner precision. */
int nsx_scalar_graph_nnz(nsx_handle *h, int which, int64_t *nnz); /* which: 0 velocity scalar P2 graph, 1 Schur graph */
int nsx_scalar_graph(nsx_handle *h, int which, int32_t *rowptr, int32_t *colind);
int nsx_ilu_get(nsx_handle *h, int which, double *values);

/* ---- forces on the obstacle ---- */
/* NavierStokes::compute_forces (reference NavierStokes3D.cpp:744-846, NavierStokes2D.cpp:752-859): drag and lift by
 * face quadrature over the faces with boundary id 3.  cells[f] = position of the face's cell in the cell list given to
 * nsx_set_mesh(_distributed), local_faces[f] = deal.II face number inside that cell.  Face tables: for every face of the
 * reference cell the shape values / reference gradients at its n_qf quadrature points, N2f[(face*n_qf+q)][n_p2] etc.,
 * weights wf[n_qf] summing to 1 (QGaussSimplex<dim-1>(3) in 3D, QGauss<1>(3) in 2D).  Returns the raw forces; the
 * coefficients 2F/(rho U^2 D H) (3D) and 2F/(U^2 D) (2D) are host arithmetic (NavierStokes3D.cpp:835-842).
 * In a multi-process run each rank passes the faces of the cells it owns and the sum is all-reduced. */
int nsx_set_force_faces(nsx_handle *h, int n_faces, const int32_t *cells, const int32_t *local_faces, int n_qf, const double *N2f,
                        const double *dN2f, const double *N1f, const double *wf);
int nsx_compute_forces(nsx_handle *h, double *drag, double *lift);

/* ---- flow diagnostics ---- */
/* How the flow is doing, from the state the handle holds -- the reference prints nothing of the kind; a deal.II application would call
 * VectorTools::integrate_difference, which imports the ghosted vector and loops over the cells on the host.  u is the velocity part of
 * `solution` (the ghosted vector: current after nsx_set_solution and after nsx_solve_time_step), previous_solution is what the handle
 * holds (reference NavierStokes3D.cpp:555; zero until the first solve).  The integrals use the quadrature rule of nsx_set_tables, the one
 * of the assembly.  lambda_k are the barycentric coordinates of a cell: grad lambda_k = row k of J^-1 for k = 1..dim, grad lambda_0 = minus
 * their sum, so u_q . grad lambda_k is a component of the reference-cell velocity J^-1 u_q; cfl_max >= 1 means: in one time step the flow
 * crosses a cell's height towards one of its faces.
 * nsx_compute_diagnostics reads state only: no vector, matrix or solver state of the handle changes and a following solve computes what
 * it would have computed without the call.  In a multi-process run a cell that several ranks hold is counted by the rank that owns its
 * lowest global P2 node, every rank gets the same totals, and the two all-reduces of a call do count in nsx_comm_counters; all ranks
 * must call it together.  The sums are folded in the caller's cell order in a fixed tree: the results are bitwise reproducible and do not
 * depend on nsx_set_ranks / nsx_set_internal_layout.
 * Returns NSX_ERR_ARG before nsx_set_tables / nsx_set_mesh(_distributed), NSX_ERR_UNSUPPORTED for a (dim, n_p2, n_q) the cell kernels are
 * not instantiated for (the set nsx_assemble accepts), and NSX_ERR_NUMERIC when any per-cell value (of any rank) is not finite -- *out is
 * then still filled, the values that are not finite propagated (the maxima do not drop a NaN). */
typedef struct {
  double kinetic_energy;  /* 1/2 int |u|^2 */
  double div_l2;          /* ( int (div u)^2 )^(1/2) */
  double grad_l2_sq;      /* int grad u : grad u   (nu * this = viscous dissipation) */
  double enstrophy;       /* 1/2 int |curl u|^2   (2D: the scalar curl) */
  double change_l2;       /* ( int |u - previous_solution|^2 )^(1/2) */
  double volume;          /* sum of |cell| over the cells counted */
  double cfl_max;         /* deltat * max over cells, quadrature points q, k = 0..dim of |u_q . grad lambda_k| */
  double speed_max;       /* max over cells and quadrature points of |u_q| */
  int64_t n_cells;        /* cells counted (all ranks) */
} nsx_flow_diag;
enum { NSX_DIAG_ENERGY = 0, NSX_DIAG_DIV2, NSX_DIAG_GRAD2, NSX_DIAG_ENSTROPHY, NSX_DIAG_CHANGE2, NSX_DIAG_VOLUME, NSX_DIAG_CFL, NSX_DIAG_SPEED,
       NSX_DIAG_COUNT };
int nsx_compute_diagnostics(nsx_handle *h, nsx_flow_diag *out);
/* The per-cell values of the last nsx_compute_diagnostics, values[n_cells of nsx_set_mesh(_distributed)] in the caller's cell order.  Sums: the
 * cell's share of the integral (NSX_DIAG_DIV2: int_cell (div u)^2, no root; NSX_DIAG_CHANGE2 likewise; energy and enstrophy with their 1/2);
 * maxima: the cell's own maximum, NSX_DIAG_CFL already multiplied by deltat.  A cell another rank counts has 0 everywhere.
 * NSX_ERR_ARG before any nsx_compute_diagnostics on the current mesh and for a `which` outside [0, NSX_DIAG_COUNT). */
int nsx_get_cell_diagnostic(nsx_handle *h, int which, double *values);

/* ---- point probes ---- */
/* The finite-element solution at given points: NavierStokes::compute_pressure_difference (reference NavierStokes3D.cpp:849-923) is
 * VectorTools::point_value on every rank -- a search of the mesh per call -- followed by a reduce.  Here the search is set-up and the per-step
 * call gathers on the device; nothing is downloaded but the values.
 * Containment: a point lies in a cell when all dim+1 barycentric coordinates are >= -tol, the coordinates being defined by x = X0 + J lambda
 * with lambda_0 = 1 - sum_k lambda_k.  tol < 0: the library's own value, 1e-12 (the one nsxh_pressure_difference uses); 0 <= tol < 1 is taken
 * as given.
 * Ties: a point on a face, an edge or a vertex lies in several cells; the probe takes the one with the lowest position in the caller's cell
 * list (the first hit in cell order, as nsxh_pressure_difference).  The choice depends on the mesh and the point only, not on
 * nsx_set_ranks / nsx_set_internal_layout or on how the search is scheduled (an integer minimum: csrc/nsx_probe.hip).
 * Not found: found = 0, cells = owners = -1 and all values exactly 0.0 -- the reference's rank that does not hold the point contributes 0.
 * Lifetime: the set survives nsx_set_ranks and nsx_set_internal_layout (cells stay in the caller's order, the geometry is the same); a new
 * nsx_set_mesh(_distributed) drops it; n_points = 0 clears it.
 * Errors: NSX_ERR_ARG for a probe call before the mesh is set, a get / eval call without a probe set, n_points < 0, null points with
 * n_points > 0, tol >= 1 and any coordinate that is not finite; NSX_ERR_UNSUPPORTED for n_points > 65536 and for a (dim, n_p2) other than
 * (2, 6) / (3, 10).
 * Distributed handles: all ranks call together, with the same points.  A rank searches only the cells it counts for the flow diagnostics, so a
 * point inside a cell has exactly one finder; a point on a face shared by cells of two ranks goes to the lowest rank that found it.  Every rank
 * receives the same owners and found, and BITWISE the same values: the owner's travel through the SUM collective with exact zeros from
 * everybody else.  nsx_set_probes costs exactly one all-reduce, nsx_eval_probes exactly one, neither a ghost exchange (nsx_comm_counters). */

/* Locate n_points points (points[n][dim]) in the mesh of nsx_set_mesh(_distributed) and keep them as the handle's probe set: the search
 * VectorTools::point_value repeats at every call (reference NavierStokes3D.cpp:862-881), done once. */
int nsx_set_probes(nsx_handle *h, int n_points, const double *points, double tol);
/* cells[n]: position of the probe's cell in the caller's cell list (-1: not found, or another rank owns the probe).
 * owners[n]: rank that evaluates it (-1: in no cell).  lambda[n][dim+1]: barycentric coordinates in that cell (0 where cells is -1).
 * Any pointer may be NULL.  (The cell and the point on the reference cell that point_value works out inside: reference NavierStokes3D.cpp:864-865, 875-876.) */
int nsx_get_probe_cells(nsx_handle *h, int32_t *cells, int32_t *owners, double *lambda);
/* velocity[n][dim], pressure[n], gradient[n][dim][dim] (d_j u_i; may be NULL), found[n] (0/1) of the ghosted `solution` (current after
 * nsx_set_solution and after nsx_solve_time_step): the point values and the reduce of reference NavierStokes3D.cpp:862-899.
 * u_h = sum_a N_a(lambda) U_a with the P2 shape functions in barycentric form (vertices lambda (2 lambda - 1), lines 4 lambda_i lambda_j in the
 * local line order {0,1},{1,2},{2,0}[,{0,3},{1,3},{2,3}]), p_h = sum_v lambda_v P_v, gradient = (sum_a U_a (x) grad_lambda N_a) J^-1 taken in
 * the probe's own cell.  Velocity and pressure are continuous across cells; the gradient is NOT: on a face it is the value from the side of the
 * cell the tie rule chose.  Any output pointer may be NULL.  A state value that is not finite propagates into the outputs of the probes whose
 * cell holds it; the call still returns NSX_OK.
 * Reads state only, like nsx_compute_diagnostics: no vector, matrix or solver state changes, a following solve computes what it would have
 * computed without the call, and two calls give bitwise equal results. */
int nsx_eval_probes(nsx_handle *h, double *velocity, double *pressure, double *gradient, int32_t *found);

/* ---- tracer particles ---- */
/* Massless particles carried by the finite-element velocity u_h: pathlines, streaklines and residence times need the velocity of EVERY time
 * step, which the output files (one VTU every 20 steps) do not hold.  No counterpart in the reference.  The particles live on the device:
 * nsx_set_tracers locates the seeds once (the probes' search), nsx_advect_tracers moves them through u_h of the state the handle holds, walking
 * from cell to cell through a face-neighbour table, and nsx_get_tracers downloads positions, cells, statuses, exit faces and ages.
 * The tracer set and the probe set are independent of each other.
 * Containment and ties: as for the point probes -- all dim+1 barycentric coordinates >= -tol, tol < 0: the library's own 1e-12, 0 <= tol < 1
 * as given; a seed on a face, an edge or a vertex starts in the lowest containing cell of the caller's cell list.  The walk uses the same tol.
 * Face neighbours: nbr[k][cell] is the cell across the face opposite local vertex k, -1 on the boundary; built from the connectivity as
 * handed over by the first nsx_set_tracers on a mesh (host/adjacency.hpp: sorted face keys), so the mesh set-up itself costs what it did.
 * Status: NSX_TRACER_NOT_FOUND the seed is in no cell; the particle never moves (position = seed, cell = -1, exit face = -1, age = 0).
 *         NSX_TRACER_ACTIVE    moves with every nsx_advect_tracers.
 *         NSX_TRACER_EXITED    a stage point or the new position of a substep left the mesh through a boundary face; the particle stays at
 *                              its position from the start of that substep, cells holds the cell of that face and exit_faces the deal.II
 *                              local number of the face: 3 - k in 3D, (k + 1) % 3 in 2D for the face opposite local vertex k (the
 *                              face -> vertex tables {0,1,2},{1,0,3},{0,2,3},{2,1,3} and {0,1},{1,2},{2,0}).  Final.
 *         NSX_TRACER_LOST      a position that is not finite (a state value that is not finite makes the particles that meet it LOST), or
 *                              more than 1024 cell-to-cell steps for one point; the particle stays at its position and in its cell from the
 *                              start of that substep, exit face -1.  Final.  The walk is bounded: the call always returns.
 * Lifetime: the set and its state (positions, ages) survive nsx_set_ranks and nsx_set_internal_layout; a new nsx_set_mesh(_distributed) drops
 * the set and the neighbour table; n = 0 clears the set.
 * Errors: NSX_ERR_ARG for a tracer call before the mesh is set, advect / get without a set, n < 0, null points with n > 0, tol >= 1, a seed
 * coordinate or a dt that is not finite, n_substeps < 1, an unknown scheme or field, and a mesh in which a face belongs to more than two
 * cells; NSX_ERR_UNSUPPORTED for n > 1048576, for a (dim, n_p2) other than (2, 6) / (3, 10), and for distributed handles with more than one
 * process (particles that cross rank boundaries are out of scope; a 1-rank communicator works).  No call issues a collective or a ghost
 * exchange (nsx_comm_counters does not move). */
enum { NSX_TRACER_EULER = 1, NSX_TRACER_RK2 = 2, NSX_TRACER_RK4 = 4 };   /* scheme: explicit Euler, explicit midpoint, classical RK4 */
enum { NSX_TRACER_FROZEN = 0, NSX_TRACER_LINEAR = 1 };                   /* field */
enum { NSX_TRACER_NOT_FOUND = 0, NSX_TRACER_ACTIVE = 1, NSX_TRACER_EXITED = 2, NSX_TRACER_LOST = 3 };

/* Locate n seeds (points[n][dim]) and make them the handle's tracer set, replacing any earlier one; ages start at 0. */
int nsx_set_tracers(nsx_handle *h, int n, const double *points /*[n][dim]*/, double tol);
/* Advance every ACTIVE particle by n_substeps steps of size h = dt / n_substeps (dt < 0: backward tracing), all inside one kernel launch.
 * field NSX_TRACER_FROZEN: the velocity is u_h of the ghosted `solution`; previous_solution is not read.
 * field NSX_TRACER_LINEAR: the velocity at stage node c (0, 1/2 or 1) of substep s is u_prev(x) + theta (u(x) - u_prev(x)) with
 *   theta = (s + c) / n_substeps for dt > 0 and theta = 1 - (s + c) / n_substeps for dt < 0, u_prev being u_h of previous_solution: one call
 *   with dt = the time step spans the step solved last.  previous_solution is zero before the first nsx_solve_time_step.
 * u_h(x) is evaluated as nsx_eval_probes does (P2 shape functions in barycentric form).  Walk rule, for every stage point and for the new
 * position: the first stage point starts from the particle's cell, each later point from the cell in which the previous point of that substep
 * was accepted; with lambda of the point in the current cell, the cell is accepted when every lambda_k >= -tol, otherwise the walk steps to
 * nbr[k], k the index of the smallest lambda (ties: the lowest k); nbr[k] = -1 ends it (EXITED).  age grows by h per completed substep.
 * Reads state only: a following solve computes bitwise what it would have computed without the call.  Particles are independent of each
 * other, so the results are bitwise reproducible and do not depend on the number of particles, nsx_set_ranks or nsx_set_internal_layout. */
int nsx_advect_tracers(nsx_handle *h, double dt, int n_substeps, int scheme, int field);
/* positions[n][dim], cells[n] (position in the caller's cell list), status[n] (NSX_TRACER_*), exit_faces[n] (-1 unless EXITED), age[n].
 * Any pointer may be NULL. */
int nsx_get_tracers(nsx_handle *h, double *positions /*[n][dim]*/, int32_t *cells, int32_t *status, int32_t *exit_faces, double *age);

/* ---- nodal fields ---- */
/* Gradient-derived fields at the P2 nodes, on the device: vorticity, Q-criterion, strain rate -- what a contour plot or an isosurface needs.
 * The per-cell values of nsx_get_cell_diagnostic are constants per cell and the gradient of nsx_eval_probes is taken in one cell only (it
 * jumps across faces); this is the continuous nodal field between the two.  No counterpart in the reference (its output() writes velocity and
 * pressure; DataPostprocessors would loop over the cells on the host).
 * Recovered gradient.  For every P2 node n the handle owns
 *     Gbar(n) = ( sum_c |c| grad u_h|_c(x_n) ) / ( sum_c |c| )
 * c runs over the cells of the mesh that hold n (all cells round the vertex, or round the edge for a mid-edge node) IN ASCENDING POSITION OF
 * THE CALLER'S CELL LIST, both sums folded left to right in double; |c| = |det J| / 2 (triangles), |det J| / 6 (tetrahedra);
 * grad u_h|_c(x_n) is evaluated exactly as nsx_eval_probes evaluates its gradient -- the P2 shape functions in barycentric form, local line order
 * {0,1},{1,2},{2,0}[,{0,3},{1,3},{2,3}], G_ij = d_j u_i = ((sum_a U_a (x) grad_lambda N_a) J^-1)_ij -- at the barycentric position of the node in
 * c: the unit vector e_k for local vertex k, (e_i + e_j) / 2 for the line {i, j}.  u is the velocity part of the ghosted `solution` (current
 * after nsx_set_solution and after nsx_solve_time_step).  An owned node that no cell holds gets exact zeros.
 * Derived fields, all computed from Gbar (not averaged separately), S = (Gbar + Gbar^T) / 2, W = (Gbar - Gbar^T) / 2:
 *     NSX_FIELD_GRADIENT    dim^2 components   Gbar_ij, row-major
 *     NSX_FIELD_VORTICITY   3 in 3D, 1 in 2D   3D: (Gbar_21 - Gbar_12, Gbar_02 - Gbar_20, Gbar_10 - Gbar_01); 2D: Gbar_10 - Gbar_01
 *     NSX_FIELD_Q           1                  (|W|_F^2 - |S|_F^2) / 2, evaluated as the algebraically equal -(sum_ij Gbar_ij Gbar_ji) / 2
 *                                              (no difference of two large norms in a shear layer)
 *     NSX_FIELD_STRAIN      1                  sqrt(2 S : S)
 *     NSX_FIELD_DIVERGENCE  1                  tr Gbar
 * Layout of values: values[n_nodes][n_components], node = P2 node in the CALLER's numbering (node i carries the velocity DoFs dim i ...
 * dim i + dim - 1 of the velocity block); n_nodes = n_u / dim on one handle.  Distributed handles are indexed globally (n_u_glob / dim nodes)
 * and fill only the entries this rank owns, like nsx_get_solution; the other entries are not touched.
 * nsx_compute_nodal_fields reads state only: no vector, matrix or solver state changes, a following solve computes bitwise what it would have
 * computed without the call, and two calls give bitwise equal results.  The results do not depend on nsx_set_ranks / nsx_set_internal_layout:
 * the fold order is the caller's cell order and the output is in the caller's numbering.  nsx_get_nodal_field returns the values of the LAST
 * nsx_compute_nodal_fields; it does not recompute after a later solve (like nsx_get_cell_diagnostic).  A state value that is not finite
 * propagates to the nodes whose patch holds it; the call still returns NSX_OK, as nsx_eval_probes does.
 * Patch table: the node -> (cell, local node) lists are built by the first nsx_compute_nodal_fields on a mesh, from the connectivity as handed
 * over (host/nodal_patch.hpp: a counting sort over the cells in their order), so the mesh set-up itself costs what it did.  The table survives
 * nsx_set_ranks and nsx_set_internal_layout; a new nsx_set_mesh(_distributed) drops the table and the results.
 * Distributed handles: every owned node has its complete patch among the handle's layer-1 cells (that is how nsx_set_mesh_distributed defines
 * them) and the ghost values are in the ghosted `solution`, so no collective and no ghost exchange is issued (nsx_comm_counters does not
 * move) and the ranks need not call together.  The values of a node equal BITWISE those of the single-process handle on the same mesh and
 * numbering, provided the rank's cell list keeps the cells that hold owned nodes in ascending global order (nsxh_rank_view_* does: layer-1
 * cells ascending, then layer-2 cells ascending, and no layer-2 cell holds an owned node).
 * Errors: NSX_ERR_ARG for a compute call before tables or mesh are set, a get / components call before any compute on the current mesh, a
 * `which` outside [0, NSX_FIELD_COUNT), null values, null n_components and a null handle; NSX_ERR_UNSUPPORTED for a (dim, n_p2) other than
 * (2, 6) / (3, 10).  A refused call leaves the results of an earlier compute readable. */
enum { NSX_FIELD_GRADIENT = 0, NSX_FIELD_VORTICITY = 1, NSX_FIELD_Q = 2, NSX_FIELD_STRAIN = 3, NSX_FIELD_DIVERGENCE = 4, NSX_FIELD_COUNT = 5 };
/* Gbar and the derived fields of the state the handle holds, at every owned P2 node, in one kernel launch (csrc/nsx_nodal.hip). */
int nsx_compute_nodal_fields(nsx_handle *h);
/* *n_components = components per node of field `which` (the table above). */
int nsx_nodal_field_components(nsx_handle *h, int which, int *n_components);
/* values[n_nodes][n_components] of field `which` as the last nsx_compute_nodal_fields left it. */
int nsx_get_nodal_field(nsx_handle *h, int which, double *values /*[n_nodes][n_components]*/);

/* ---- isosurfaces and slices ---- */
/* The isosurface { s = isovalue } of a nodal scalar s, extracted on the device by marching sub-simplices: what travels to the host is the
 * surface, O(N^(2/3)) cells of the mesh, instead of one value per P2 node (nsx_get_nodal_field) that the host then has to contour.  No
 * counterpart in the reference (its output() writes the whole volume as a VTU).
 * Output: an unindexed soup of primitives -- triangles in 3D (3 vertices), segments in 2D (2 vertices): dim vertices of dim coordinates each.
 * points[n][dim][dim] (primitive, vertex, coordinate), colour[n][dim] (the second scalar interpolated to every vertex), cells[n] (position of
 * the primitive's cell in the caller's cell list).  Any pointer of nsx_get_isosurface may be NULL; a colour pointer needs an extract with one.
 * Nodal scalar s at every P2 node of a cell, by source (nsx_iso_source; `which` and `component` are read where the table names them):
 *     NSX_ISO_VELOCITY   component 0 .. dim-1: the velocity DoF of the node, an exact copy; component -1: sqrt(sum_i u_i^2), summed left to right
 *     NSX_ISO_PRESSURE   the P1 value at a vertex; 0.5 (p_i + p_j) at the mid-edge node of line {i, j} -- exact for P1, so the extraction from
 *                        the pressure is the exact level set of p_h
 *     NSX_ISO_NODAL      component `component` of field `which` (NSX_FIELD_*) as the last nsx_compute_nodal_fields left it
 *     NSX_ISO_PLANE      normal . x_node (left to right), x_node the vertex or 0.5 (X_i + X_j) for a mid-edge node: slices, with any other
 *                        source as colour
 * u and p are the ghosted `solution` (current after nsx_set_solution and after nsx_solve_time_step).
 * Subdivision.  Every P2 cell is cut into linear sub-simplices on its own nodes (local line order {0,1},{1,2},{2,0}[,{0,3},{1,3},{2,3}]):
 *     2D: the triangles (0,3,5) (3,1,4) (5,4,2) (3,4,5)
 *     3D: the corner tetrahedra (0,4,6,7) (4,1,5,8) (6,5,2,9) (7,8,9,3) and the inner octahedron split along its diagonal 4-9 into
 *         (4,9,5,6) (4,9,6,7) (4,9,7,8) (4,9,8,5)
 * The diagonal is interior to the cell and every face is split into the canonical 4 triangles whatever the neighbour does: the surface is
 * watertight across cells.  The surface is the level set of the piecewise LINEAR interpolant on the sub-simplices (second order, not the
 * curved P2 level set).
 * Classification and vertices.  A node is inside when s >= isovalue.  On an edge with a inside and b outside the vertex is
 *     t = (s_a - iso) / (s_a - s_b),   x = x_a + t (x_b - x_a),   c = c_a + t (c_b - c_a)
 * always from the inside end to the outside end, never by node number, without contraction into fused multiply-adds: two cells that share
 * the edge compute BITWISE the same vertex, under every internal layout.  A sub-simplex with a nodal s that is not finite emits nothing (the
 * call still returns NSX_OK).  Zero-area primitives (s == iso exactly at nodes) are emitted as they come.
 * Cases, by the set of inside vertices of the sub-simplex (v0,v1,v2[,v3]); a-b is the crossing from inside vertex a to outside vertex b.
 * Orientation: the normal (p1 - p0) x (p2 - p0) points from inside to outside; in 2D the inside lies to the left of p0 -> p1.  The table is
 * the vertex order in a cell with det J > 0; a cell with det J < 0 swaps the last two vertices of every primitive.  A tetrahedron with two
 * inside {i < j} and two outside {k < l} gives the quad i-k i-l j-l j-k, split along its first and third corner.
 *     tetrahedron                                          triangle
 *     {0}      (0-1 0-2 0-3)                               {0}    (0-1 0-2)
 *     {1}      (1-0 1-3 1-2)                               {1}    (1-2 1-0)
 *     {0,1}    (0-2 0-3 1-3)  (0-2 1-3 1-2)                {0,1}  (1-2 0-2)
 *     {2}      (2-0 2-1 2-3)                               {2}    (2-0 2-1)
 *     {0,2}    (0-1 2-3 0-3)  (0-1 2-1 2-3)                {0,2}  (0-1 2-1)
 *     {1,2}    (1-0 1-3 2-3)  (1-0 2-3 2-0)                {1,2}  (2-0 1-0)
 *     {0,1,2}  (0-3 1-3 2-3)
 *     {3}      (3-0 3-2 3-1)
 *     {0,3}    (0-1 0-2 3-2)  (0-1 3-2 3-1)
 *     {1,3}    (1-0 3-2 1-2)  (1-0 3-0 3-2)
 *     {0,1,3}  (0-2 3-2 1-2)
 *     {2,3}    (2-0 2-1 3-1)  (2-0 3-1 3-0)
 *     {0,2,3}  (0-1 2-1 3-1)
 *     {1,2,3}  (1-0 3-0 2-0)
 * (host/iso_tables.hpp holds the tables.)
 * Order: ascending position in the caller's cell list, then the sub-simplex order above, then the table order.  The positions come from an
 * exclusive prefix sum of the per-cell counts (count, scan, emit: csrc/nsx_iso.hip), not from an atomic cursor, so the result does not depend on
 * the scheduling, nsx_set_ranks or nsx_set_internal_layout, and two calls agree bitwise.  nsx_extract_isosurface reads state only: no vector,
 * matrix or solver state changes and a following solve computes bitwise what it would have computed without the call.  The result survives
 * until the next extract or a new nsx_set_mesh(_distributed); nsx_get_isosurface does not recompute after a later solve.
 * The vertex coordinates of the cells and the node maps the kernels need are uploaded by the first extract on a mesh (the mesh set-up itself costs
 * what it did).  The workgroup width of the count / scan / emit kernels is read per call from NSX_ISO_WG (64 / 128 / 256, default 256), as
 * NSX_SPMV_R is.
 * Distributed handles: a rank extracts from the cells it counts for the flow diagnostics (nsx_compute_diagnostics: the owner of the cell's
 * lowest global P2 node), so every cell has one extractor and the union over the ranks is the single-process surface, primitive by
 * primitive bitwise.  No collective and no ghost exchange is issued (nsx_comm_counters does not move) and the ranks need not call together;
 * *n_primitives is the rank's own count and cells index the rank's own cell list.  NSX_ISO_NODAL, as field or colour, returns
 * NSX_ERR_UNSUPPORTED with more than one process (ghost nodes have no nodal results); a 1-rank communicator works.
 * Errors: NSX_ERR_ARG for a null handle, field or n_primitives, a call before tables, mesh or state, an unknown kind, `which` or `component`,
 * an isovalue that is not finite, a plane normal that is not finite or all zero, NSX_ISO_NODAL without valid nodal results on the current
 * mesh, and a get before any extract on the current mesh; NSX_ERR_UNSUPPORTED for a (dim, n_p2) other than (2, 6) / (3, 10) and for more than
 * 2^31 - 1 primitives.  A refused call leaves an earlier result readable. */
enum { NSX_ISO_VELOCITY = 0, NSX_ISO_PRESSURE = 1, NSX_ISO_NODAL = 2, NSX_ISO_PLANE = 3 };
typedef struct {
  int kind;         /* NSX_ISO_* */
  int which;        /* NSX_ISO_NODAL: the field, NSX_FIELD_* */
  int component;    /* NSX_ISO_VELOCITY: 0 .. dim-1, or -1 for the magnitude; NSX_ISO_NODAL: component of the field */
  double normal[3]; /* NSX_ISO_PLANE: s = normal . x (the first dim entries) */
} nsx_iso_source;
/* Extracts { field = isovalue } from the state the handle holds; *n_primitives = primitives this handle found. */
int nsx_extract_isosurface(nsx_handle *h, const nsx_iso_source *field, double isovalue, const nsx_iso_source *colour /* NULL: none */,
                           int64_t *n_primitives);
/* The primitives of the last nsx_extract_isosurface. */
int nsx_get_isosurface(nsx_handle *h, double *points /*[n][dim][dim]*/, double *colour /*[n][dim]*/, int32_t *cells /*[n]*/);

/* ---- lattice sampling ---- */
/* u_h, p_h, grad u_h and the nodal fields on a regular axis-aligned lattice, sampled on the device: an image of a 2D flow, a volume for
 * rendering, a plane image at constant z, uniform data for spectra.  No counterpart in the reference.  The point probes search every cell for
 * every point and take at most 65536 points; here every cell visits the lattice points its bounding box can hold (a rasterisation,
 * csrc/nsx_lattice.hip), and nothing is stored per point but the owning cell.
 * Lattice: point (i_0, ..., i_{dim-1}) has the coordinates x_d = origin_d + (double)i_d * spacing_d, formed with one rounded multiply and one
 * rounded add, never a fused multiply-add: origin + i * spacing in IEEE double arithmetic on the host gives the same bits.  Linear index
 * i_0 + counts_0 (i_1 + counts_1 i_2), x fastest: a plane is an image as it stands.  n_total = prod counts_d; counts_d = 1 is allowed (a plane
 * image of a 3D flow).  origin = spacing = counts = NULL clears the lattice.
 * Ownership: containment, tolerance and ties are those of the point probes -- a point lies in a cell when all dim+1 barycentric coordinates
 * are >= -tol (tol < 0: the library's 1e-12; 0 <= tol < 1 as given), and among several cells the one with the lowest position in the
 * caller's cell list owns the point (an integer minimum: exact and order-free).  The owner table depends on the mesh and the lattice alone,
 * not on the scheduling, nsx_set_ranks or nsx_set_internal_layout.  A point in no cell has cells = -1 and every sampled value exactly 0.0;
 * *n_found is the number of owned points.
 * Values: of the ghosted `solution` (current after nsx_set_solution and after nsx_solve_time_step), as nsx_eval_probes defines them --
 * u_h = sum_a N_a(lambda) U_a, p_h = sum_v lambda_v P_v, gradient = (sum_a U_a (x) grad_lambda N_a) J^-1 taken in the owner cell (d_j u_i,
 * discontinuous across faces as the probes').  NSX_LATTICE_NODAL samples the P2 interpolant sum_a N_a(lambda) V_a of every plane the last
 * nsx_compute_nodal_fields left at the cell's nodes: continuous images of the recovered gradient, vorticity, Q, strain rate and divergence.
 * A state value that is not finite propagates into the points whose cell holds it; the call still returns NSX_OK.
 * `what` of nsx_eval_lattice is an OR of the NSX_LATTICE_* bits; only what is asked for is computed and stored (8 bytes per point and
 * component).  nsx_get_lattice hands out one quantity (one of the bits; `which` an NSX_FIELD_* for NSX_LATTICE_NODAL, ignored otherwise) as
 * planes values[n_components][n_total]: dim for the velocity, 1 for the pressure, dim^2 (row-major d_j u_i) for the gradient, the field's
 * components for a nodal field.  It returns what the last nsx_eval_lattice computed and does not recompute after a later solve.
 * The three calls read state only: no vector, matrix or solver state changes, a following solve computes bitwise what it would have computed
 * without them, and two calls agree bitwise.  The lattice and its results survive nsx_set_ranks and nsx_set_internal_layout; a new
 * nsx_set_mesh(_distributed) or a new nsx_set_lattice drops them.  A refused call leaves an earlier lattice and its results readable.  No call
 * issues a collective or a ghost exchange (nsx_comm_counters does not move).
 * Errors: NSX_ERR_ARG for a null handle or output pointer, a call before tables or mesh, an eval / get call without a lattice, some but not
 * all of origin / spacing / counts null, a count < 1, a spacing that is not finite or not > 0, an origin that is not finite, tol >= 1 or not
 * finite, a lattice whose neighbouring coordinates are not distinct finite doubles at either end of an axis, `what` = 0 or with unknown bits,
 * an unknown `quantity` or `which`, a quantity the last nsx_eval_lattice did not compute, NSX_LATTICE_NODAL without valid nodal results on
 * the current mesh and an eval before the handle holds a state.  NSX_ERR_UNSUPPORTED for a (dim, n_p2) other than (2, 6) / (3, 10), for
 * n_total > 2^26 (checked before anything is allocated) and for a handle with more than one process (merging the ranks' lattices is out of
 * scope; a 1-rank communicator works, as for the tracers). */
enum { NSX_LATTICE_VELOCITY = 1, NSX_LATTICE_PRESSURE = 2, NSX_LATTICE_GRADIENT = 4, NSX_LATTICE_NODAL = 8 };
/* Installs the lattice and finds the owner of every point; *n_found (may be NULL) = points that lie in a cell. */
int nsx_set_lattice(nsx_handle *h, const double *origin /*[dim]*/, const double *spacing /*[dim]*/, const int32_t *counts /*[dim]*/, double tol,
                    int64_t *n_found);
/* cells[n_total]: position of the point's cell in the caller's cell list, -1: in no cell. */
int nsx_get_lattice_cells(nsx_handle *h, int32_t *cells /*[n_total]*/);
/* Samples what `what` names from the state the handle holds. */
int nsx_eval_lattice(nsx_handle *h, int what);
/* One quantity of the last nsx_eval_lattice. */
int nsx_get_lattice(nsx_handle *h, int quantity, int which, double *values /*[n_components][n_total]*/);

/* ---- running statistics ---- */
/* The time-averaged flow and its fluctuations, accumulated on the device one sample per call from the state the handle holds: weighted mean of
 * velocity and pressure, the co-moments sum w u'_i u'_j (Reynolds stresses, rms, turbulent kinetic energy) and the pressure variance, in up to
 * 64 phase bins (the caller decides which bin a time step belongs to: a phase-averaged flow of a periodic shedding), each bin on its own or all
 * pooled.  No counterpart in the reference (its output() writes snapshots only).  csrc/nsx_stats.hip.
 * Accumulators: per bin a weight sum W and a sample count on the host; on the device, per P2 node this handle owns, the mean m_c (dim planes)
 * and the upper triangle of the co-moment C_ij (3 or 6 planes), and per owned P1 node m and C (2 planes).  Symmetric component order:
 * xx, yy, [zz,] xy[, xz, yz].  The planes are kept in the CALLER's node numbering, so an accumulation survives nsx_set_ranks and
 * nsx_set_internal_layout untouched (hand the state over again after a new layout, as always); a new nsx_set_mesh(_distributed) drops it.
 * The recurrence (a contract: the results are reproducible to the bit from it).  For a sample x of weight w > 0 into a bin with weight W (0 when
 * empty) the host forms three doubles, one rounded operation each,
 *     W' = W + w,   r = w / W',   q = W * r,
 * and the device does per DoF and per pair i <= j, every operation an IEEE double operation rounded on its own, never a fused multiply-add,
 *     d_i  = x_i - m_i
 *     m_i  = m_i + r * d_i                 (product, then sum)
 *     C_ij = C_ij + (q * d_i) * d_j        (left to right; d from before the mean moved)
 * With q >= 0 the diagonal increments are q times a square: C_ii never decreases and no variance is negative.  The first sample of a bin has
 * r = 1, q = 0: m = x and C = 0 exactly.
 * Quantities (nsx_stats_get; computed on the device from the raw planes, the host passes invW = 1 / W): NSX_STATS_MEAN_U [dim] and
 * NSX_STATS_COMOMENT_U [3 | 6] are the raw planes; NSX_STATS_STRESS_U [3 | 6] = C_ij * invW; NSX_STATS_RMS_U [dim] = sqrt(C_ii * invW);
 * NSX_STATS_TKE [1] = 0.5 * (R_00 + R_11 [+ R_22]) with R = the stresses, summed left to right, then halved; NSX_STATS_MEAN_P,
 * NSX_STATS_COMOMENT_P, NSX_STATS_VAR_P = C * invW and NSX_STATS_RMS_P = sqrt(C * invW) [1 each].
 * Pooled (bin = -1): the non-empty bins are folded in ascending order with the pairwise merge (a, b) -> a; the host forms W = W_a + W_b,
 * s = W_b / W, t = W_a * s, the device per node, in registers, delta_i = m_b,i - m_a,i, C_ij = (C_a,ij + C_b,ij) + (t * delta_i) * delta_j,
 * m_i = m_a,i + s * delta_i (C first: delta and m_a from before the mean moved), then the quantity with invW = 1 / W of the fold.  The
 * accumulators themselves are not modified.
 * nsx_stats_accumulate reads state only (the ghosted `solution`, current after nsx_set_solution and nsx_solve_time_step): no vector, matrix
 * or solver state changes and a following solve computes bitwise what it would have computed without the call.  A state value that is not
 * finite sticks in the accumulators of its own DoF only; the call returns NSX_OK.  The values do not depend on the scheduling, the rank
 * tables or the internal layout.  Distributed handles accumulate the nodes they own and issue no collective and no ghost exchange
 * (nsx_comm_counters does not move); the ranks need not call together.  nsx_stats_get is indexed globally and fills only the entries this
 * rank owns, as nsx_get_nodal_field does; they are bitwise those of a single-process handle.
 * Errors: NSX_ERR_ARG for a null handle or output pointer (nsx_stats_info: any pointer may be NULL), a call before tables, mesh or (accumulate)
 * a state, accumulate / info / get without an open accumulation, `what` with unknown bits, exactly one of what / n_bins zero, n_bins outside
 * 1..64, a bin out of range, a weight that is not finite or <= 0, an unknown quantity, a get of a quantity whose part (`what`) is not
 * accumulated, a get from an empty bin or pooled with all bins empty; NSX_ERR_UNSUPPORTED for a (dim, n_p2) other than (2, 6) / (3, 10).  A
 * refused call leaves the accumulation as it was. */
enum { NSX_STATS_VELOCITY = 1, NSX_STATS_PRESSURE = 2 };
/* Opens (or, with what = 0 and n_bins = 0, closes and frees) an accumulation: zeroed accumulators for n_bins phase bins, 1 <= n_bins <= 64. */
int nsx_stats_begin(nsx_handle *h, int what, int n_bins);
/* Adds the state the handle holds as one sample of weight `weight` to bin `bin`.  One kernel launch. */
int nsx_stats_accumulate(nsx_handle *h, int bin, double weight);
/* what, n_bins, samples[n_bins], weights[n_bins] (the running W of each bin); any pointer may be NULL. */
int nsx_stats_info(nsx_handle *h, int *what, int *n_bins, int64_t *samples, double *weights);
enum { NSX_STATS_MEAN_U = 0, NSX_STATS_COMOMENT_U, NSX_STATS_STRESS_U, NSX_STATS_RMS_U, NSX_STATS_TKE,
       NSX_STATS_MEAN_P, NSX_STATS_COMOMENT_P, NSX_STATS_VAR_P, NSX_STATS_RMS_P, NSX_STATS_QUANTITY_COUNT };
/* Components per node of a quantity (needs a mesh, not an open accumulation). */
int nsx_stats_components(nsx_handle *h, int quantity, int *n_components);
/* values[n_nodes][n_components] (P2 nodes for the velocity quantities, P1 nodes for the pressure's); bin >= 0: that bin; bin = -1: all
 * non-empty bins pooled. */
int nsx_stats_get(nsx_handle *h, int quantity, int bin, double *values);

/* ---- surface loads ---- */
/* What the flow does to a boundary, from the state the handle holds: wall pressure, traction, wall shear stress and y+ at every node of a set
 * of boundary faces, and per group of faces (typically a boundary id) area, pressure force, viscous force, torque, flow rate and pressure
 * integral.  nsx_compute_forces (above, unchanged) returns drag and lift of one face set by a caller-supplied face quadrature and sums on
 * the host; here no table is needed: every surface integrand of a P2/P1 state is a polynomial of degree <= 2 on a face, which the P2 nodal
 * rule of the face integrates exactly.  csrc/nsx_surface.hip.  Forces are kinematic (density 1), as the project's.
 * Faces: cells[f] and local_faces[f] as for nsx_set_force_faces (position in the caller's cell list, deal.II local face number);
 * groups[f] in [0, n_groups), 1 <= n_groups <= 64.  The face opposite local vertex k has the deal.II number 3 - k in 3D and (k + 1) % 3 in 2D
 * (the tables of the tracer section).
 * Geometry of the face opposite local vertex k: grad lambda_k is row k of J^-1 for k >= 1 (rows counted from 1) and minus the sum of the rows
 * (added in their order) for k = 0; the outward unit normal of the fluid domain n = -grad lambda_k / |grad lambda_k| (the direction of
 * fe_face_values.normal_vector; up to rounding the J^-T nref of nsx_compute_forces); the height of the cell over the face d = 1 / |grad lambda_k|;
 * the measure |f| = |det J| |grad lambda_k| m with m = 1 in 2D and 1/2 in 3D.
 * Face nodes: the face's vertices in the order of the face -> vertex tables {0,1},{1,2},{2,0} and {0,1,2},{1,0,3},{0,2,3},{2,1,3}, then in 3D
 * the mid-edge nodes of the face lines (v0 v1, v1 v2, v2 v0), in 2D the one mid-point: 3 nodes per face in 2D, 6 in 3D.
 * Values at a face node, taken in the face's own cell (the one-sided wall gradient) and evaluated as nsx_eval_probes evaluates (P2 in
 * barycentric form, reference derivatives first, J^-1 last): p the P1 value, G_ij = d_j u_i, tau = nu (G + G^T) (NSX_SURFACE_SYMMETRIC) or
 * nu G (NSX_SURFACE_GRADIENT); the traction the fluid exerts on the boundary t = p n - tau n; the wall shear stress
 * s = -(tau n - (n . tau n) n); the shear magnitude |s|; y+ = sqrt(|s|) d / nu (all zeros when nu <= 0; at faces only).
 * Surface nodes: a distinct (group, P2 node) pair among the face nodes -- a node on the seam of two groups is two surface nodes, one per
 * group -- numbered by ascending group, then ascending P2 node id in the caller's numbering.  nsx_get_surface_layout: nodes[s] the P2 node
 * (caller's numbering; global on a distributed handle), node_groups[s], face_nodes[f][j] the surface node of face node j of face f,
 * areas[f] = |f|; any pointer may be NULL.
 * Recovery at a surface node: Vbar(s) = sum_f |f| V_f(x_s) / sum_f |f| over the faces of that group that hold the node, in ascending position
 * in the caller's face list, both sums folded left to right in double: pressure, traction and shear.  The shear magnitude at a node is that of
 * the averaged shear, the normal is sum_f |f| n_f normalised.
 * Totals per group by the P2 nodal rule of the face: weights |f| (1/6, 1/6, 4/6) in 2D (vertices, mid-point); |f| / 3 on the three mid-edge
 * nodes and 0 on the vertices in 3D.  A face's weighted terms are added in the order of its nodes; the faces of a group are folded in a
 * fixed tree over the caller's order whose shape depends on the face counts alone.  No atomics: bitwise reproducible, independent of
 * nsx_set_ranks and nsx_set_internal_layout.
 * Fields (nsx_get_surface_field): NSX_SURFACE_PRESSURE [1], _TRACTION [dim], _SHEAR [dim], _SHEAR_MAGNITUDE [1], _NORMAL [dim], _YPLUS [1].
 * at = NSX_SURFACE_AT_FACES: values[n_faces][nodes per face][n_components], faces in the caller's order (the normal is the face's at each of
 * its nodes); at = NSX_SURFACE_AT_NODES: values[n_surface_nodes][n_components].
 * The calls read state only (the ghosted `solution`, current after nsx_set_solution and nsx_solve_time_step): a following solve computes
 * bitwise what it would have computed without them.  nsx_get_surface_field returns the values of the last nsx_compute_surface and does not
 * recompute after a later solve.  A state value that is not finite propagates to exactly the face nodes whose cell holds it and to the
 * surface nodes and group totals built from them; the call still returns NSX_OK.  The set survives nsx_set_ranks and
 * nsx_set_internal_layout; a new nsx_set_mesh(_distributed) drops it; n_faces = 0 clears it.
 * Distributed handles: the caller passes the boundary faces of the rank's cell list in ascending global face order, at least those of its
 * layer-1 cells.  A face enters the totals on the rank that counts its cell (the rule of the flow diagnostics).  nsx_compute_surface with
 * totals costs exactly one all-reduce (every rank gets the sums of all ranks), with totals = NULL none; no call issues a ghost exchange.
 * Values at nodes are filled for the surface nodes whose P2 node the rank owns (the rest 0) and are bitwise those of a single-process
 * handle; values at faces are filled for every face passed.
 * Errors: NSX_ERR_ARG for a null handle, a call before tables or mesh, a get / info / compute call without a set, a get before a compute,
 * a compute before the handle holds a state, a bad cell, local face, group, n_groups, form, `which` or `at`, NSX_SURFACE_YPLUS at nodes, a
 * centre that is not finite, a null output where one is required, a (cell, face) pair given twice; NSX_ERR_UNSUPPORTED for a (dim, n_p2)
 * other than (2, 6) / (3, 10).  A refused call writes nothing and leaves an earlier set and its results readable. */
enum { NSX_SURFACE_SYMMETRIC = 0, NSX_SURFACE_GRADIENT = 1 };       /* viscous stress tau = nu (G + G^T) | nu G,  G_ij = d_j u_i */
enum { NSX_SURFACE_AT_FACES = 0, NSX_SURFACE_AT_NODES = 1 };
enum { NSX_SURFACE_PRESSURE = 0, NSX_SURFACE_TRACTION, NSX_SURFACE_SHEAR, NSX_SURFACE_SHEAR_MAGNITUDE, NSX_SURFACE_NORMAL, NSX_SURFACE_YPLUS,
       NSX_SURFACE_FIELD_COUNT };
typedef struct {
  double area;                 /* sum |f| */
  double force_pressure[3];    /* int p n               (entries >= dim are 0) */
  double force_viscous[3];     /* -int tau n */
  double torque[3];            /* int (x - centre) x t ; 2D: torque[2] only */
  double flux;                 /* int u . n */
  double pressure_integral;    /* int p */
  int64_t n_faces;             /* faces counted (all ranks) */
} nsx_surface_totals;

/* Installs the face set (n_faces = 0: clears it). */
int nsx_set_surface(nsx_handle *h, int n_faces, const int32_t *cells, const int32_t *local_faces, const int32_t *groups /* NULL: all 0 */,
                    int n_groups, int form, const double *centre /*[dim]; NULL: origin*/);
int nsx_surface_info(nsx_handle *h, int info[4]);   /* n_faces, n_groups, n_surface_nodes, nodes per face (3 | 6) */
int nsx_get_surface_layout(nsx_handle *h, int32_t *nodes, int32_t *node_groups, int32_t *face_nodes, double *areas);
/* Evaluates every face node and surface node of the set from the state the handle holds; the totals of every group if asked for. */
int nsx_compute_surface(nsx_handle *h, nsx_surface_totals *totals /*[n_groups]; may be NULL*/);
int nsx_surface_field_components(nsx_handle *h, int which, int *n_components);
int nsx_get_surface_field(nsx_handle *h, int which, int at, double *values);

/* ---- measurement ---- */
/* Per-kernel HIP-event timing of the hot path (bench.py roofline): enable, run, then read name/count/total-ms. */
int nsx_profile_enable(nsx_handle *h, int on);
int nsx_profile_reset(nsx_handle *h);
int nsx_profile_count(nsx_handle *h);
int nsx_profile_get(nsx_handle *h, int i, const char **name, int64_t *launches, double *total_ms, double *bytes_per_launch);

/* State of the two persistent (single-launch, grid-wide-exchange) kernels of this handle, for tests and bench.py:
 * state[0] / state[1] = 1 while the Gram-Schmidt sweep / the Schur-complement CG run as ONE launch (0: never used yet, switched
 * off, or fallen back), state[2] = time-outs so far (= nsx_solve_stats::persistent_fallbacks), state[3] = mailbox words that are
 * not empty in the region the next launch would use (0 on a healthy handle and after a recovered time-out). */
int nsx_persistent_state(nsx_handle *h, int state[4]);

/* Which code paths this handle's products and solves take -- for tests, and for the log a multi-GPU rehearsal writes per rank:
 * info[0] 1 = every F->vmult (reference Preconditioners.hpp:382,405; NavierStokes3D.cpp:574) goes through the LDS-staged SpMV,
 * [1] its chunks, [2] those of them that stage a ghost column (launched behind the ghost exchange; 0 on one GPU),
 * [3] entries per thread of the LAST Gram-Schmidt sweep that ran as one persistent launch (8 / 10 / 12; 0: none yet, or two passes),
 * [4] workgroups of its grid, [5] 1 = with the collective inside, [6] the largest instantiation any sweep has used so far,
 * [7] CUs the compute stream leaves to the communication stream (0 or 8), [8] the last Schur-complement CG: 1 one launch per
 * operation, 2 one persistent launch, 3 two launches per iteration, [9] Schur ILU blocks, [10] neighbours of the ghost exchange,
 * [11] owned P2 nodes sent per exchange, [12] ghost P2 nodes, [13] 1 = explicit inverses of the Schur ILU blocks,
 * [14] 1 = the persistent sweep is switched off or has fallen back, [15] persistent kernels that timed out so far,
 * [16] / [17] entries per thread of the sweep instantiation an RCCL run WOULD use for the velocity vector on plain / on CU-masked
 * streams (0: the resident grid does not hold it: two passes), [18] / [19] the same for the block vector, [20] Schur blocks per
 * entry of a partial-sum array of the two-launch CG (1: no fold launch), [21] the velocity sweep's instantiation on one GPU without a
 * communicator, [22] / [23] P2 / P1 nodes this handle owns, [24] 1 = the last persistent sweep had the triangular solves of the velocity
 * ILU(0) inside its launch (k_ilu_mgs: PreconditionILU::vmult + the orthogonalisation of one inner GMRES iteration, reference
 * Preconditioners.hpp:382,405, as ONE kernel), [25] such launches so far, [26] 1 = the inner F products of the last solve streamed float
 * values (NSX_INNER_FP32 through the LDS-staged SpMV), [27] 1 = its velocity triangular solves did (the lane-owner stream) -- "solve":
 * the last nsx_solve_time_step / nsx_prec_vmult, or the last call of the test hooks nsx_inner_F_vmult / nsx_sparse_product ([26]) /
 * nsx_ilu_apply(0) ([27]);
 * [28] rows per lane group of the register-resident block inverses in the last Schur-complement CG (6: blocks of up to 96 rows, 8: up to
 * 128; 0: the inverses were streamed, or the persistent kernel did not run), [29] 1 = that kernel held the operator's rows in LDS;
 * [30] rows of the largest chunk of the LDS-staged SpMV, [31] staged columns of the chunk that stages most (the kernel serves chunks of
 * up to 448 rows whose staged x entries fit 64 KiB of LDS; [0] says whether it is used).
 * The switches of the velocity product are read once by nsx_create, like NSX_INNER_PRECISION: NSX_SPMV_W (lanes per row of the plain
 * kernel: 8 / 32, anything else 16), NSX_SPMV_BLOCKED=0 (never the LDS-staged kernel), NSX_SPMV_ORDER=0 (its chunks in row order instead of
 * largest first).  NSX_SPMV_R (target rows per chunk, 16..448, default 130) is read whenever the chunk table is rebuilt. */
int nsx_path_info(nsx_handle *h, int info[32]);

/* Which kernels the block-Jacobi ILU(0) of F (which = 0) or of the Schur matrix (which = 1) ran -- a test hook:
 * info[0] the factorisation kernel of the last nsx_prec_initialize / solve (NSX_ILU_FACTOR_*: one launch per level, the block staged
 * in LDS, a dense row per wave, the general one; 0: none yet), [1] the kernel that built the explicit block inverses (NSX_ILU_INVERT_*),
 * [2] the kernel of the LAST triangular solve on that schedule (NSX_ILU_SOLVE_*: one launch per level, the dense inverses, the
 * lane-owner stream, a workgroup per block with its part of x in LDS / in global memory; 0: none since the schedule was built),
 * [3] entries per lane and tick of the stream (NSX_ILU_EPT; 0: no stream), [4] slabs per register set of that solve (NSX_PF: 4 / 8; 0: not
 * the stream), [5] its interleaved right-hand sides, [6] 1 = it read the float stream, [7] waves of the stream, [8] blocks,
 * [9] rows of the largest block, [10] in-block entries of the largest block, [11] rows of the largest wave, [12] 1 = the schedule is
 * levelled, [13] 1 = it has a usable lane-owner stream, [14] 1 = it has explicit inverses, [15] bytes of dynamic LDS the factorisation
 * asked for (the LDS-staged kernel; else 0).
 * The solves inside a fused sweep launch (k_ilu_mgs) are not recorded. */
#define NSX_ILU_FACTOR_LEVEL 1
#define NSX_ILU_FACTOR_LDS 2
#define NSX_ILU_FACTOR_DENSE_ROW 3
#define NSX_ILU_FACTOR_GENERAL 4
#define NSX_ILU_INVERT_NONE 0
#define NSX_ILU_INVERT_LDS 1
#define NSX_ILU_INVERT_GLOBAL 2
#define NSX_ILU_SOLVE_LEVELLED 1
#define NSX_ILU_SOLVE_DENSE 2
#define NSX_ILU_SOLVE_LANES 3
#define NSX_ILU_SOLVE_BLOCK_LDS 4
#define NSX_ILU_SOLVE_BLOCK_GLOBAL 5
int nsx_ilu_path_info(nsx_handle *h, int which, int info[16]);
/* 1 = the last inversion on that schedule (nsx_ilu_path_info [1] == NSX_ILU_INVERT_LDS) read the factor from LDS: the in-block entries of
 * every block fitted beside its matrix under the device's opt-in limit of dynamic LDS, and NSX_ILU_INVERT_STAGE (read per call,
 * default 1) was not 0; 0 = it read the factor from global memory, or no inversion in LDS has run.  A test hook. */
int nsx_ilu_invert_staged(nsx_handle *h, int which, int *staged);
/* The plan of the Schur product S = B diag(w) B^T (host/schur_plan.hpp) -- a test hook: info[0] 1 = the handle's Schur graph is
 * planned (0: not built yet, a row of block(1,0) of 65535 entries or more, or a distributed handle), [1] 1 = the last product ran the
 * planned kernel (NSX_SCHUR_PLAN, read per call, default 1; handles with a communicator or a distributed mesh always run the merge
 * kernel), [2] entries of S, [3] terms over all entries, [4] 32-bit words of the plan, [5] its bytes on the device, [6] longest row of
 * block(1,0), [7] host time of the plan in microseconds. */
int nsx_schur_plan_info(nsx_handle *h, long long info[8]);

/* SolverGMRES' orthogonalisation (deal.II's modified Gram-Schmidt add_and_dot chain inside every solver.solve of the path: reference
 * NavierStokes3D.cpp:574, Preconditioners.hpp:173,273,288,382,405) on the caller's vectors, through the very sweep kernel the solvers
 * use: vectors[m][n] (row k = vector k) -- vector 0 is normalised, vector k is orthogonalised against vectors 0..k-1 and normalised,
 * in place.  coeffs[k * m + i] = h(i) of sweep k, norms2[k] = |w|^2 after sweep k (norms2[0]: |vector 0|^2 as it came).
 * norm_guard: the sweep takes |w'|^2 from the basis' Gram matrix (|w|^2 - 2 h.r + h^T G h) while more than that fraction of |w|^2
 * is left and sums it explicitly otherwise; 0 = always the formula, 1e300 = always the explicit sum, < 0 = the library's own (1e-2).
 * A test hook for that formula; m <= 30. */
int nsx_gram_schmidt_cycle(nsx_handle *h, int n, int m, double *vectors, double norm_guard, double *coeffs, double *norms2);
/* The same cycle with the arguments of the sweep that nsx_gram_schmidt_cycle fixes, ONE sweep per vector (SolverGMRES' second,
 * re-orthogonalising sweep is not imitated).  vectors[m][n + gap] is in the device layout of a distributed block vector: logical
 * entry i of a vector lives at i + (i >= split ? gap : 0) (0 <= split <= n; split == n needs gap == 0); the gap entries are uploaded
 * and downloaded as they are and no sweep may touch them.  flags bit 0: the sweep also returns |w|^2 BEFORE it (norms2_before[k];
 * 0 without the bit, [0] = norms2[0]) and decides itself, by SolverGMRES' test |w'| <= 10 |w| sqrt(eps), whether a second sweep
 * would follow -- it then leaves w unnormalised; flags bit 1: the sweep does not normalise at all (the first sweep of a
 * re-orthogonalising iteration).  normalized[k] = 1 where the sweep normalised vector k itself, 0 where the hook scaled it with
 * 1 / sqrt(norms2[k]) afterwards ([0] = 0: vector 0 is always scaled by the hook).  coeffs, norms2, norm_guard, m <= 30: as above. */
int nsx_gram_schmidt_sweeps(nsx_handle *h, int n, int split, int gap, int m, double *vectors, double norm_guard, int flags, double *coeffs,
                            double *norms2, double *norms2_before, int *normalized);

/* Test hook: a short PROGRAM of the Krylov drivers' BLAS-1 operations (csrc/nsx_blas.hip, v_reciprocal of csrc/nsx_solve.hip) on the
 * caller's vectors, every op by the very host function the solvers call -- so that a reduction followed by a consumer that sums its
 * partial sums, with or without a finalisation in between, can be compared with a reference on its own (tests/test_gpu_blas1.py).
 * vectors[m][n + gap] is in the device layout of a block vector as for nsx_gram_schmidt_sweeps (logical entry i at
 * i + (i >= split ? gap : 0); 0 <= split <= n; split == n needs gap == 0); the gap entries are uploaded and downloaded as they are.
 * The ops run in order on the handle's stream; out[i] is the value of op i's result slot if its `read` flag is set (read through
 * read_scalars: the slot is final afterwards), else 0.  NSX_BLAS1_READ publishes `count` slots from `slot` on; its values are appended
 * to scalars_out (capacity scalars_cap doubles; more is NSX_ERR_ARG) and out[i] is the first of them.
 * Vector indices address rows of `vectors` (-1 = none, only where the table says so); slots are the solvers' scalar slots 0 .. 126; `num`
 * / `den` = -1 where the op takes none.  The ops with a plain length (no span) need gap == 0 or a length `n` of their own: an op with
 * n > 0 runs on the first n <= split entries of its vectors alone (a short reduction into a slot a long one has left its partial sums in).
 *   kind                      host function            fields
 *   NSX_BLAS1_DOT             v_dot                    slot = d . w
 *   NSX_BLAS1_ADD_AND_DOT     v_add_and_dot            d += a value(num) v ; slot = d . w   (w == d: the kernel's self branch)
 *   NSX_BLAS1_ADD             v_add                    d += a v
 *   NSX_BLAS1_ADD_DEV         v_add_dev                d += a value(num) v
 *   NSX_BLAS1_SADD            v_sadd                   d = s d + a v
 *   NSX_BLAS1_SCALE           v_scale                  d *= a
 *   NSX_BLAS1_SCALE_DEV_INV   v_scale_dev_inv          d *= 1 / value(den)
 *   NSX_BLAS1_SCALE_VEC       v_scale_vec              d[i] *= v[i]                          (plain length)
 *   NSX_BLAS1_AXPY_MULTI      v_axpy_multi             d += sum_j coef[j] vectors[vs[j]], j < k <= 40 (above 32: two launches)
 *   NSX_BLAS1_AXPY_MULTI_INTO v_axpy_multi_into        d = (v >= 0 ? v : 0) + sum_j ..., then d = -w + d if w >= 0 (w may be d).
 *                                                      k > 32, or v >= 0 together with w >= 0: the library's own NSX_ERR_ARG
 *   NSX_BLAS1_CG_UPDATE       cg_update                d += alpha v ; w += alpha x ; slot = w . w, alpha = value(num) / value(den)   (plain length)
 *   NSX_BLAS1_CG_DIRECTION    cg_direction             d = (value(num) / value(den)) d - v   (plain length)
 *   NSX_BLAS1_RECIPROCAL      v_reciprocal             d[i] = a / v[i]                        (plain length)
 *   NSX_BLAS1_FINALIZE        finalize_slots           slots slot .. slot + count - 1 become final (count > 64: NSX_ERR_ARG)
 *   NSX_BLAS1_READ            read_scalars             as above (count > 64: the library's own NSX_ERR_ARG)
 *   NSX_BLAS1_WRITE_SCALAR    write_scalar             slot = a
 * A coefficient a value(num) / value(den) is evaluated on the device from the slots as they are: still spread over the partial sums of the
 * reduction that wrote them, or final.  The hook leaves nothing behind: every slot counts as final again when it returns (also after an
 * error), so a program never sees the state of an earlier one.  Single-process handles, with or without a 1-rank communicator (which
 * forces the fixed grid of 256 partial sums per reduction; a distributed handle: NSX_ERR_UNSUPPORTED, as nsx_gmres); any time after
 * nsx_set_mesh. */
enum {
  NSX_BLAS1_DOT = 0, NSX_BLAS1_ADD_AND_DOT, NSX_BLAS1_ADD, NSX_BLAS1_ADD_DEV, NSX_BLAS1_SADD, NSX_BLAS1_SCALE, NSX_BLAS1_SCALE_DEV_INV,
  NSX_BLAS1_SCALE_VEC, NSX_BLAS1_AXPY_MULTI, NSX_BLAS1_AXPY_MULTI_INTO, NSX_BLAS1_CG_UPDATE, NSX_BLAS1_CG_DIRECTION, NSX_BLAS1_RECIPROCAL,
  NSX_BLAS1_FINALIZE, NSX_BLAS1_READ, NSX_BLAS1_WRITE_SCALAR, NSX_BLAS1_KIND_COUNT
};
#define NSX_BLAS1_MAX_K 40
typedef struct nsx_blas1_op {
  int32_t kind;                 /* NSX_BLAS1_* */
  int32_t d, v, w, x;           /* vector indices */
  int32_t slot, num, den;       /* result slot; slots of the coefficient's numerator and denominator */
  int32_t count;                /* FINALIZE, READ: length of the slot range */
  int32_t read;                 /* != 0: read the result slot now (out[i]) */
  int32_t n;                    /* 0: the op runs on the program's span; > 0: on the first n entries alone, a plain length (n <= split) */
  int32_t k;                    /* multi-axpy: number of terms */
  int32_t vs[NSX_BLAS1_MAX_K];  /* ... their vectors */
  double a, s;                  /* host coefficients */
  double coef[NSX_BLAS1_MAX_K]; /* multi-axpy: coefficients */
} nsx_blas1_op;
int nsx_blas1_run(nsx_handle *h, int n, int split, int gap, int m, double *vectors, int n_ops, const nsx_blas1_op *ops, double *out,
                  double *scalars_out, int scalars_cap);

/* ---- multi-GPU (one process per GPU, RCCL over xGMI) ---- */
/* Replaces the MPI communicator inside Epetra (reference NavierStokes3D.hpp:93-94,102): MPI_Allreduce behind every
 * dot / norm, Epetra_Import behind every vmult and behind `solution = solution_owned` (NavierStokes3D.cpp:638). */
int nsx_comm_unique_id(uint8_t id[128]);                       /* rank 0: ncclGetUniqueId */
int nsx_comm_init(nsx_handle *h, int rank, int world, const uint8_t id[128]);   /* RCCL over xGMI */
/* Bring-your-own communicator (the reference's MPI, gloo in the tests): host-buffer callbacks, return 0 on success.
 * allreduce: in-place sum of `count` doubles over all ranks.  exchange: for each of n neighbours send send[k]
 * (send_count[k] doubles) to rank ranks[k] and receive recv_count[k] doubles from it into recv[k]. */
typedef int (*nsx_allreduce_fn)(void *ctx, double *buf, int count);
typedef int (*nsx_exchange_fn)(void *ctx, int n, const int *ranks, const double *const *send, const int *send_count,
                               double *const *recv, const int *recv_count);
int nsx_comm_init_callbacks(nsx_handle *h, int rank, int world, nsx_allreduce_fn allreduce, nsx_exchange_fn exchange, void *ctx);
/* Collectives issued by this handle since the communicator was set: counts[0] all-reduces (the MPI_Allreduce behind Epetra's
 * Dot / Norm2, reference Preconditioners.hpp:157,179,371,388,403 and every SolverGMRES / SolverCG iteration), counts[1] ghost
 * exchanges (the Epetra_Import of every vmult).  The orthogonalisation of a Krylov vector costs ONE all-reduce (csrc/nsx_mgs.hip,
 * mgs_lowsync; a second one only when the sweep removes more than 99 % of the vector's norm) where the reference pays one per link
 * of the add_and_dot chain. */
int nsx_comm_counters(const nsx_handle *h, long long counts[2]);
/* Test hook: the RCCL branch of the ghost exchange (pack kernel, grouped ncclSend / ncclRecv straight into the ghost region -- the
 * Epetra_Import of every vmult --, event, wait of the compute stream) on a 1-rank communicator whose only neighbour is the rank
 * itself: ghost node k of a vector of n_own + n_ghost nodes must receive the ncomp values of owned node (7 k + 3) % n_own.
 * max_err = largest deviation after three exchanges in a row.  (RCCL refuses two ranks on one device: a one-GPU box has no other way
 * to execute that branch.) */
int nsx_comm_self_halo_test(nsx_handle *h, int n_own, int n_ghost, int ncomp, double *max_err);
/* Distributed mesh, replaces nsx_set_mesh for world > 1.  cell_dofs keep the GLOBAL deal.II numbering; gpu_u_ptr /
 * gpu_p_ptr [world+1] are the P2 / P1 node ranges owned by each rank (locally_owned_dofs per block, reference
 * NavierStokes3D.cpp:71-87).  Cells: first the n_cells_layer1 cells that touch an owned P2 node (every owned row is
 * assembled locally, no compress(VectorOperation::add), NavierStokes3D.cpp:314-319), then the cells touching a node
 * of those (rows of block(1,0) for the ghost pressure nodes the Schur product reaches).  Halo plan: for each
 * neighbour (ascending ranks) the global ids of the owned nodes it needs, ascending (include/nsx_host.h:
 * nsxh_rank_view_*).  Afterwards nsx_set_ranks takes GLOBAL node ranges of this rank's sub-blocks; state vectors
 * (nsx_set_solution, nsx_get_*, nsx_apply_boundary_values, nsx_system_vmult) are indexed GLOBALLY, get_* fill only the
 * entries this rank owns. */
int nsx_set_mesh_distributed(nsx_handle *h, int n_cells, int n_cells_layer1, int dofs_per_cell, const int32_t *cell_dofs,
                             const double *cell_coords, int n_u_global, int n_p_global, int world, int rank,
                             const int32_t *gpu_u_ptr, const int32_t *gpu_p_ptr, int n_neighbors, const int32_t *neighbors,
                             const int32_t *send_u_ptr, const int32_t *send_u_nodes, const int32_t *send_p_ptr,
                             const int32_t *send_p_nodes);

#ifdef __cplusplus
}
#endif
#endif
