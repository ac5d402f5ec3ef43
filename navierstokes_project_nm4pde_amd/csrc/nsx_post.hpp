// nsx_post.hpp — what the post-processing files share (nsx_diag, nsx_probe, nsx_tracer, nsx_nodal, nsx_iso, nsx_lattice, nsx_stats, nsx_surface): the affine cell map, the P2
// shape functions in barycentric form, the push-forward of a reference gradient, the space check and the layout of the nodal results.
// Their state lives in nsx_internal.hpp (DiagState ... SurfaceState), and so does the guard of their C entries (NSX_TRY / NSX_CATCH).
#pragma once
#include "nsx_internal.hpp"

namespace nsx {

// ------------------------------------------------------------------ device: cell map
// J^-1 (rows of geo) and vertex 0 of a cell: x = X0 + J lambda[1..]
template <int DIM>
__device__ __forceinline__ void load_cell_map(int n_cells, int cell, const double *__restrict__ geo, const double *__restrict__ x0, double (&Ji)[DIM][DIM],
                                              double (&X0)[DIM]) {
#pragma unroll
  for (int k = 0; k < DIM; ++k) {
    X0[k] = x0[(size_t)k * n_cells + cell];
#pragma unroll
    for (int d = 0; d < DIM; ++d) Ji[k][d] = geo[(size_t)(k * DIM + d) * n_cells + cell];
  }
}

// lambda[0..DIM] of x in the cell (X0, J^-1): x = X0 + J lambda[1..], lambda[0] = 1 - sum.  A coordinate that is not finite is in no cell.
template <int DIM>
__device__ __forceinline__ bool probe_lambda(const double (&Ji)[DIM][DIM], const double (&X0)[DIM], const double *x, double tol, double (&lam)[DIM + 1]) {
  double l0 = 1.0;
  bool in = true;
#pragma unroll
  for (int k = 0; k < DIM; ++k) {
    double s = 0.0;
#pragma unroll
    for (int d = 0; d < DIM; ++d) s += Ji[k][d] * (x[d] - X0[d]);
    lam[k + 1] = s;
    l0 -= s;
    in = in && s >= -tol;
  }
  lam[0] = l0;
  return in && l0 >= -tol;
}

// ------------------------------------------------------------------ device and host: P2 on a simplex
// FESystem's local order: the DIM + 1 vertices, then the lines {P2_LI[l], P2_LJ[l]} in the front-end's order {0,1},{1,2},{2,0}[,{0,3},{1,3},{2,3}]
constexpr int P2_LI[6] = {0, 1, 2, 0, 1, 2}, P2_LJ[6] = {1, 2, 0, 3, 3, 3};

// Shape function a in barycentric form: vertices lambda_a (2 lambda_a - 1), lines 4 lambda_i lambda_j.  VALUE: n = N_a(lam); GRAD: g[m] =
// dN_a / d lambda_m.  The reference coordinates are xi_k = lambda_k (k = 1..DIM) with lambda_0 = 1 - sum xi, so dN_a / d xi_k = g[k] - g[0].
// Called with a the counter of an unrolled loop: lam and g are indexed statically and stay in registers; no table is read at run time, so
// nothing is hoisted into SGPRs (the trap described above k_cell_diag does not arise).
template <int DIM, bool VALUE, bool GRAD>
__device__ __forceinline__ void p2_shape(int a, const double (&lam)[DIM + 1], double &n, double (&g)[DIM + 1]) {
  constexpr int NV = DIM + 1;
  if (GRAD) {
#pragma unroll
    for (int m = 0; m < NV; ++m) g[m] = 0.0;
  }
  if (a < NV) {
    if (VALUE) n = lam[a] * (2.0 * lam[a] - 1.0);
    if (GRAD) g[a] = 4.0 * lam[a] - 1.0;
  } else {
    const int i = P2_LI[a - NV], j = P2_LJ[a - NV];
    if (VALUE) n = 4.0 * lam[i] * lam[j];
    if (GRAD) {
      g[i] = 4.0 * lam[j];
      g[j] = 4.0 * lam[i];
    }
  }
}

// Column j of grad u = H J^-1 in a cell (H[i][k] = d u_i / d xi_k, geo holds J^-1 row-major): sink(i, d_j u_i) for i = 0..DIM-1, in that
// order, each value handed over as soon as it is formed (the callers store or fold it at once, as their own loops did)
template <int DIM, class Sink>
__device__ __forceinline__ void push_forward_col(int n_cells, int cell, const double *__restrict__ geo, const double (&H)[DIM][DIM], int j, Sink &&sink) {
  double Jc[DIM];  // column j of J^-1
#pragma unroll
  for (int k = 0; k < DIM; ++k) Jc[k] = geo[(size_t)(k * DIM + j) * n_cells + cell];
#pragma unroll
  for (int i = 0; i < DIM; ++i) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < DIM; ++k) s += H[i][k] * Jc[k];
    sink(i, s);
  }
}

// ------------------------------------------------------------------ host
// "a mesh is set and the element is P2/P1 on simplices": the first test of every entry of the family; `who` is the entry's name
inline void post_check_space(const nsx_handle *h, const char *who) {
  if (!h->have_mesh) NSX_THROW(NSX_ERR_ARG, "%s: nsx_set_tables and nsx_set_mesh first", who);
  if (!((h->dim == 2 && h->np2 == 6) || (h->dim == 3 && h->np2 == 10)))
    NSX_THROW(NSX_ERR_UNSUPPORTED, "%s: no kernel instantiated for dim=%d n_p2=%d (P2/P1 on simplices only)", who, h->dim, h->np2);
}

constexpr double PROBE_TOL = 1e-12;  // the tolerance of nsxh_pressure_difference
// the search of nsx_set_probes on n device points [n][dim]: best [n] (INT32_MAX on entry) -> cells [n] (-1: in no cell), lam SoA [dim+1][n]
void probe_locate(nsx_handle *h, int n, const double *points, double tol, int32_t *best, int32_t *cells, double *lam);

// planes of nodal.out: the dim^2 entries of Gbar (row-major), then vorticity (3 / 1), Q, strain rate, divergence
constexpr int nodal_planes(int dim) { return dim * dim + (dim == 3 ? 3 : 1) + 3; }
inline int nodal_components(int dim, int which) { return which == NSX_FIELD_GRADIENT ? dim * dim : which == NSX_FIELD_VORTICITY ? (dim == 3 ? 3 : 1) : 1; }
inline int nodal_first_plane(int dim, int which) {
  int p = 0;
  for (int f = 0; f < which; ++f) p += nodal_components(dim, f);
  return p;
}

// what nsx_iso.hip keeps on the device for itself and for nsx_lattice.hip: the vertex coordinates of every cell (iso.cellx, uploaded by the
// first caller on a mesh) and the map internal P2 node -> slot of nodal.out (iso.slot, rebuilt when the layout has moved)
void iso_ensure_coords(nsx_handle *h);
void iso_ensure_slots(nsx_handle *h);

}  // namespace nsx
