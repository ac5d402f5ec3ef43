// nsx_tracer.hip — tracer particles: massless particles carried by u_h (include/nsx.h, section "tracer particles").  No counterpart in the
// reference, whose output (one VTU every 20 steps, NavierStokes3D.cpp:643-683) cannot give pathlines.
// A probe is located once and never moves; a tracer walks from cell to cell several times per step.  Everything it needs sits on the device:
// the ghosted `solution` and `previous_solution`, cell_n2, geo (J^-1), probe.cell_x0 and the probes' containment arithmetic (probe_lambda); the one
// table that was missing, the face neighbours tracer.cell_nbr[k][cell], is built by the first nsx_set_tracers on a mesh (host/adjacency.hpp).
//
//   k_tracer_advect  one PARTICLE PER LANE, 64-lane workgroups, ALL n_substeps inside one launch.  Position, cell, stage velocities and the
//                    cell map stay in registers; everything is unrolled with static indexing, as k_probe_eval.  Per stage point: the walk
//                    (lambda in the current cell by probe_lambda; accept, or step through the face of the smallest lambda) and NP2 * DIM
//                    gathered doubles (twice that for the LINEAR field).  The kernel is bound by the latency of those dependent gathers, not
//                    by bytes: no LDS, no atomics, registers kept low for occupancy.  Particles do not interact, so a particle's result
//                    depends on its own state, the mesh and the field alone -- not on the launch geometry, the number of particles,
//                    nsx_set_ranks or nsx_set_internal_layout (cells stay in the caller's order, cell_n2 names the internal nodes).
//                    The walk cannot spin: at most TRACER_MAX_HOPS cell-to-cell steps per point, then the particle is LOST.
//                    Particle state is SoA: coalesced loads and stores.
#include <algorithm>
#include <cmath>

#include "../host/adjacency.hpp"
#include "nsx_post.hpp"

namespace nsx {

constexpr int TRACER_MAX = 1048576;
constexpr int TRACER_MAX_HOPS = 1024;  // cell-to-cell steps for one point (the CPU prototype of the walk never needed more than 7)

// walk: from cell `cur` to the cell that holds x.  0: accepted (cur, lam of x in it), otherwise NSX_TRACER_EXITED (cur: the cell of the
// boundary face, kexit: its opposite local vertex) or NSX_TRACER_LOST.  Every nbr entry is -1 or a cell (checked on the host).
template <int DIM>
__device__ __forceinline__ int tracer_walk(int n_cells, const int32_t *__restrict__ nbr, const double *__restrict__ geo, const double *__restrict__ x0,
                                           const double (&x)[DIM], double tol, int &cur, double (&lam)[DIM + 1], int &kexit) {
  bool finite = true;
#pragma unroll
  for (int d = 0; d < DIM; ++d) finite = finite && fabs(x[d]) <= 1.79769313486231570815e308;  // false for NaN and inf
  if (!finite) return NSX_TRACER_LOST;
  for (int hop = 0; hop <= TRACER_MAX_HOPS; ++hop) {
    double Ji[DIM][DIM], X0[DIM];
    load_cell_map<DIM>(n_cells, cur, geo, x0, Ji, X0);
    if (probe_lambda<DIM>(Ji, X0, x, tol, lam)) return 0;
    int k = 0;
    double lmin = lam[0];
#pragma unroll
    for (int m = 1; m <= DIM; ++m)
      if (lam[m] < lmin) {  // strict: ties go to the lowest k
        lmin = lam[m];
        k = m;
      }
    const int next = nbr[(size_t)k * n_cells + cur];
    if (next < 0) {
      kexit = k;
      return NSX_TRACER_EXITED;
    }
    cur = next;
  }
  return NSX_TRACER_LOST;
}

// u_h at lam in `cell` (p2_shape, nsx_post.hpp).  LINEAR: u_prev + theta (u - u_prev), both sums node by node.
template <int DIM, int NP2, bool LINEAR>
__device__ __forceinline__ void tracer_velocity(int n_cells, int cell, const int32_t *__restrict__ cell_n2, const double *__restrict__ sol,
                                                const double *__restrict__ prev, const double (&lam)[DIM + 1], double theta, double (&u)[DIM]) {
  double up[DIM];
#pragma unroll
  for (int i = 0; i < DIM; ++i) u[i] = up[i] = 0.0;
#pragma unroll
  for (int a = 0; a < NP2; ++a) {
    double n, g[DIM + 1];  // g: not computed
    p2_shape<DIM, true, false>(a, lam, n, g);
    const int node = cell_n2[(size_t)a * n_cells + cell];
#pragma unroll
    for (int i = 0; i < DIM; ++i) {
      u[i] += n * sol[(size_t)node * DIM + i];
      if (LINEAR) up[i] += n * prev[(size_t)node * DIM + i];
    }
  }
  if (LINEAR) {
#pragma unroll
    for (int i = 0; i < DIM; ++i) u[i] = up[i] + theta * (u[i] - up[i]);
  }
}

// SCHEME: NSX_TRACER_EULER / RK2 (explicit midpoint) / RK4.  h = dt / n_substeps (signed); forward = dt > 0.
template <int DIM, int NP2, int SCHEME, bool LINEAR>
__global__ __launch_bounds__(64) void k_tracer_advect(int n, double *__restrict__ px, int32_t *__restrict__ pcell, int32_t *__restrict__ pstatus,
                                                      int32_t *__restrict__ pface, double *__restrict__ page, int n_cells,
                                                      const int32_t *__restrict__ nbr, const int32_t *__restrict__ cell_n2,
                                                      const double *__restrict__ geo, const double *__restrict__ x0, const double *__restrict__ sol,
                                                      const double *__restrict__ prev, double h, int n_substeps, int forward, double tol) {
  constexpr int NSTAGE = SCHEME == NSX_TRACER_RK4 ? 4 : SCHEME == NSX_TRACER_RK2 ? 2 : 1;
  const int p = blockIdx.x * 64 + threadIdx.x;
  if (p >= n) return;
  if (pstatus[p] != NSX_TRACER_ACTIVE) return;
  double x[DIM], age = page[p];
#pragma unroll
  for (int d = 0; d < DIM; ++d) x[d] = px[(size_t)d * n + p];
  int cell = pcell[p], status = NSX_TRACER_ACTIVE, face = -1;
  if (cell < 0 || cell >= n_cells) return;  // never the case for an ACTIVE particle
  const double inv_n = 1.0 / (double)n_substeps;
  for (int s = 0; s < n_substeps && status == NSX_TRACER_ACTIVE; ++s) {
    int cur = cell, kexit = -1, r = 0;
    double y[DIM], acc[DIM], k[DIM], lam[DIM + 1];
#pragma unroll
    for (int d = 0; d < DIM; ++d) {
      y[d] = x[d];
      acc[d] = 0.0;
    }
#pragma unroll
    for (int st = 0; st < NSTAGE; ++st) {
      // stage node c and the weight of this stage in the update
      const double c = NSTAGE == 4 ? (st == 0 ? 0.0 : st == 3 ? 1.0 : 0.5) : NSTAGE == 2 ? (st == 0 ? 0.0 : 0.5) : 0.0;
      if (r == 0) {
        r = tracer_walk<DIM>(n_cells, nbr, geo, x0, y, tol, cur, lam, kexit);
        if (r == 0) {
          double theta = ((double)s + c) * inv_n;
          if (!forward) theta = 1.0 - theta;
          tracer_velocity<DIM, NP2, LINEAR>(n_cells, cur, cell_n2, sol, prev, lam, theta, k);
#pragma unroll
          for (int d = 0; d < DIM; ++d) {
            if (NSTAGE == 4) {
              acc[d] += (st == 0 || st == 3 ? 1.0 : 2.0) * k[d];
              y[d] = x[d] + (st == 2 ? h : 0.5 * h) * k[d];  // the next stage point (unused behind the last stage)
            } else if (NSTAGE == 2) {
              acc[d] = k[d];
              y[d] = x[d] + 0.5 * h * k[d];
            } else {
              acc[d] = k[d];
            }
          }
        }
      }
    }
    if (r == 0) {  // the new position
#pragma unroll
      for (int d = 0; d < DIM; ++d) y[d] = x[d] + (NSTAGE == 4 ? h / 6.0 : h) * acc[d];
      r = tracer_walk<DIM>(n_cells, nbr, geo, x0, y, tol, cur, lam, kexit);
    }
    if (r == 0) {
#pragma unroll
      for (int d = 0; d < DIM; ++d) x[d] = y[d];
      cell = cur;
      age += h;
    } else {  // frozen at the position from the start of this substep
      status = r;
      if (r == NSX_TRACER_EXITED) {
        cell = cur;
        face = DIM == 3 ? 3 - kexit : (kexit + 1) % 3;
      }
    }
  }
#pragma unroll
  for (int d = 0; d < DIM; ++d) px[(size_t)d * n + p] = x[d];
  pcell[p] = cell;
  pstatus[p] = status;
  pface[p] = face;
  page[p] = age;
}

// ------------------------------------------------------------------ host drivers
static void tracer_check_space(nsx_handle *h, const char *who) {
  post_check_space(h, who);
  if (h->world > 1) NSX_THROW(NSX_ERR_UNSUPPORTED, "tracer particles on %d processes: particles that cross rank boundaries are not supported", h->world);
}

static void ensure_neighbours(nsx_handle *h) {
  if (h->tracer.have_nbr) return;
  const int nv = h->dim + 1;
  if (h->np1 != nv || h->cell_n1_in.size() != (size_t)h->n_cells * nv) NSX_THROW(NSX_ERR_ARG, "the connectivity does not name dim + 1 vertices per cell");
  std::vector<int32_t> nbr;
  const int64_t rc = build_face_neighbours(h->n_cells, nv, h->cell_n1_in.data(), nbr);
  if (rc > 0) NSX_THROW(NSX_ERR_ARG, "cell %lld: a face of it belongs to more than two cells", (long long)(rc - 1));
  if (rc < 0 || nbr.size() != (size_t)h->n_cells * nv) NSX_THROW(NSX_ERR_ARG, "the face-neighbour table could not be built");
  for (int32_t c : nbr)
    if (c < -1 || c >= h->n_cells) NSX_THROW(NSX_ERR_ARG, "the face-neighbour table names cell %d", c);
  h->tracer.cell_nbr.upload(nbr, h->stream);
  h->tracer.have_nbr = true;
}

static void set_tracers(nsx_handle *h, int n, const double *points, double tol) {
  tracer_check_space(h, "nsx_set_tracers");
  if (n < 0) NSX_THROW(NSX_ERR_ARG, "n = %d", n);
  if (n > TRACER_MAX) NSX_THROW(NSX_ERR_UNSUPPORTED, "%d tracer particles: at most %d per handle", n, TRACER_MAX);
  if (n > 0 && !points) NSX_THROW(NSX_ERR_ARG, "null points");
  if (!(tol < 1.0)) NSX_THROW(NSX_ERR_ARG, "tol = %g: a value below 1 (negative: the library's own, %g)", tol, PROBE_TOL);
  const int dim = h->dim;
  for (size_t i = 0; i < (size_t)n * dim; ++i)
    if (!std::isfinite(points[i])) NSX_THROW(NSX_ERR_ARG, "tracer %zu: coordinate %zu is not finite", i / dim, i % dim);
  if (n == 0) {
    h->tracer.n = 0;
    return;
  }
  if (tol < 0.0) tol = PROBE_TOL;
  HIP_CHECK(hipSetDevice(h->prm.device));
  ensure_neighbours(h);
  h->tracer.n = 0;  // a failure below leaves no set
  DevBuf<double> pts, lam;
  DevBuf<int32_t> best;
  pts.upload(points, (size_t)n * dim, h->stream);
  best.upload(std::vector<int32_t>((size_t)n, INT32_MAX), h->stream);
  lam.alloc((size_t)(dim + 1) * n);
  h->tracer.cell.alloc(n);
  probe_locate(h, n, pts.p, tol, best.p, h->tracer.cell.p, lam.p);
  std::vector<int32_t> cells((size_t)n), status((size_t)n);
  h->tracer.cell.download(cells.data(), cells.size(), h->stream);
  for (int p = 0; p < n; ++p) status[p] = cells[p] >= 0 ? NSX_TRACER_ACTIVE : NSX_TRACER_NOT_FOUND;
  std::vector<double> x((size_t)dim * n);
  for (int p = 0; p < n; ++p)
    for (int d = 0; d < dim; ++d) x[(size_t)d * n + p] = points[(size_t)p * dim + d];
  h->tracer.x.upload(x, h->stream);
  h->tracer.status.upload(status, h->stream);
  h->tracer.face.upload(std::vector<int32_t>((size_t)n, -1), h->stream);
  h->tracer.age.upload(std::vector<double>((size_t)n, 0.0), h->stream);
  h->tracer.tol = tol;
  h->tracer.n = n;
}

template <int DIM, int NP2, int SCHEME, bool LINEAR>
static void launch_advect(nsx_handle *h, double dt, int n_substeps) {
  constexpr int NSTAGE = SCHEME == NSX_TRACER_RK4 ? 4 : SCHEME == NSX_TRACER_RK2 ? 2 : 1;
  const int n = h->tracer.n;
  // algorithmic bytes: the particle state in and out, and per substep NSTAGE + 1 cell maps and NSTAGE gathers (node ids + values) without a hop
  const double per_stage = 4.0 * NP2 + 8.0 * NP2 * DIM * (LINEAR ? 2 : 1), per_map = 8.0 * (DIM * DIM + DIM);
  const double bytes = (double)n * (2.0 * (8.0 * (DIM + 1) + 12.0) + (double)n_substeps * (NSTAGE * per_stage + (NSTAGE + 1) * per_map));
  LaunchScope ls(h, "tracer_advect", bytes);
  hipLaunchKernelGGL((k_tracer_advect<DIM, NP2, SCHEME, LINEAR>), dim3(cdiv(n, 64)), dim3(64), 0, h->stream, n, h->tracer.x.p, h->tracer.cell.p,
                     h->tracer.status.p, h->tracer.face.p, h->tracer.age.p, h->n_cells, h->tracer.cell_nbr.p, h->cell_n2.p, h->geo.p, h->probe.cell_x0.p, h->sol.p,
                     h->prev_sol.p, dt / n_substeps, n_substeps, dt > 0.0 ? 1 : 0, h->tracer.tol);
}

template <int DIM, int NP2>
static void dispatch_advect(nsx_handle *h, double dt, int n_substeps, int scheme, int field) {
  const bool lin = field == NSX_TRACER_LINEAR;
  if (scheme == NSX_TRACER_EULER) lin ? launch_advect<DIM, NP2, NSX_TRACER_EULER, true>(h, dt, n_substeps) : launch_advect<DIM, NP2, NSX_TRACER_EULER, false>(h, dt, n_substeps);
  else if (scheme == NSX_TRACER_RK2) lin ? launch_advect<DIM, NP2, NSX_TRACER_RK2, true>(h, dt, n_substeps) : launch_advect<DIM, NP2, NSX_TRACER_RK2, false>(h, dt, n_substeps);
  else lin ? launch_advect<DIM, NP2, NSX_TRACER_RK4, true>(h, dt, n_substeps) : launch_advect<DIM, NP2, NSX_TRACER_RK4, false>(h, dt, n_substeps);
}

static void advect_tracers(nsx_handle *h, double dt, int n_substeps, int scheme, int field) {
  tracer_check_space(h, "nsx_advect_tracers");
  if (h->tracer.n == 0 || !h->tracer.have_nbr) NSX_THROW(NSX_ERR_ARG, "nsx_set_tracers first");
  if (!std::isfinite(dt)) NSX_THROW(NSX_ERR_ARG, "dt is not finite");
  if (n_substeps < 1) NSX_THROW(NSX_ERR_ARG, "n_substeps = %d", n_substeps);
  if (scheme != NSX_TRACER_EULER && scheme != NSX_TRACER_RK2 && scheme != NSX_TRACER_RK4) NSX_THROW(NSX_ERR_ARG, "scheme = %d (NSX_TRACER_EULER / RK2 / RK4)", scheme);
  if (field != NSX_TRACER_FROZEN && field != NSX_TRACER_LINEAR) NSX_THROW(NSX_ERR_ARG, "field = %d (NSX_TRACER_FROZEN / LINEAR)", field);
  if (!h->sol.p || !h->prev_sol.p || h->sol.n < (size_t)h->len_blk || h->prev_sol.n < (size_t)h->len_blk) NSX_THROW(NSX_ERR_ARG, "the handle holds no state yet");
  HIP_CHECK(hipSetDevice(h->prm.device));
  if (h->dim == 2) dispatch_advect<2, 6>(h, dt, n_substeps, scheme, field);
  else dispatch_advect<3, 10>(h, dt, n_substeps, scheme, field);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(h->stream));
}

static void get_tracers(nsx_handle *h, double *positions, int32_t *cells, int32_t *status, int32_t *exit_faces, double *age) {
  tracer_check_space(h, "nsx_get_tracers");
  if (h->tracer.n == 0) NSX_THROW(NSX_ERR_ARG, "nsx_set_tracers first");
  HIP_CHECK(hipSetDevice(h->prm.device));
  const int dim = h->dim, n = h->tracer.n;
  if (positions) {
    std::vector<double> x((size_t)dim * n);
    h->tracer.x.download(x.data(), x.size(), h->stream);
    for (int p = 0; p < n; ++p)
      for (int d = 0; d < dim; ++d) positions[(size_t)p * dim + d] = x[(size_t)d * n + p];
  }
  if (cells) h->tracer.cell.download(cells, n, h->stream);
  if (status) h->tracer.status.download(status, n, h->stream);
  if (exit_faces) h->tracer.face.download(exit_faces, n, h->stream);
  if (age) h->tracer.age.download(age, n, h->stream);
}

}  // namespace nsx

extern "C" {

int nsx_set_tracers(nsx_handle *h, int n, const double *points, double tol) {
  NSX_TRY(h)
  nsx::set_tracers(h, n, points, tol);
  NSX_CATCH(h)
}

int nsx_advect_tracers(nsx_handle *h, double dt, int n_substeps, int scheme, int field) {
  NSX_TRY(h)
  nsx::advect_tracers(h, dt, n_substeps, scheme, field);
  NSX_CATCH(h)
}

int nsx_get_tracers(nsx_handle *h, double *positions, int32_t *cells, int32_t *status, int32_t *exit_faces, double *age) {
  NSX_TRY(h)
  nsx::get_tracers(h, positions, cells, status, exit_faces, age);
  NSX_CATCH(h)
}

}  // extern "C"
