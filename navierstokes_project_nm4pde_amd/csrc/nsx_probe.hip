// nsx_probe.hip — point probes: the finite-element solution at given points (include/nsx.h, section "point probes").
//
//   NavierStokes::compute_pressure_difference   reference Navier-Stokes/src/NavierStokes3D.cpp:849-923 (VectorTools::point_value on every
//                                               rank, then a reduce); the host restatement is nsxh_pressure_difference (host/frontend.cpp)
// The reference searches the mesh at every call.  Here the search is set-up (nsx_set_probes) and the per-step call (nsx_eval_probes) only
// gathers: everything it needs already sits on the device -- cell_n2, cell_n1, geo (J^-1) and the ghosted `solution`; the mesh set-up adds
// vertex 0 of every cell (probe.cell_x0).
//
//   k_probe_locate  one CELL PER LANE, one wave per workgroup, as the cell kernels: a lane loads X0 and J^-1 of its cell once and walks ALL
//                   points, staged in LDS in tiles of PROBE_TILE, so one pass over the cells serves every point.  A point lies in a cell
//                   when lambda = (1 - sum, J^-1 (x - X0)) >= -tol in every component.  Per point the wave's lowest containing cell comes
//                   from one ballot (cells ascend with the lanes), and that lane issues one atomicMin on the point's int32: an integer
//                   minimum is exact and order-free, so the result depends on the mesh and the point alone -- not on the scheduling, the
//                   launch geometry, nsx_set_ranks or nsx_set_internal_layout (cells stay in the caller's order).
//                   Set-up cost.  Algorithmic bytes per launch 8 (dim^2 + dim) n_cells, n_cells * n_points containment tests.
//   k_probe_finish  one probe per lane: lambda in the chosen cell, by the arithmetic of the search (probe_lambda), stored for the evaluations.
//   k_probe_eval    one PROBE PER LANE: gathers the NP2 dim + dim + 1 values of its cell, u = sum N_a(lambda) U_a, p = sum lambda_v P_v,
//                   grad u = (sum U_a (x) grad_ref N_a) J^-1, and leaves dim + 1 + dim^2 values per probe as SoA planes [.][n_points] of ONE
//                   buffer (coalesced stores) -- all-reduced in a distributed run, copied out in one copy.  A probe this handle does not
//                   evaluate writes exact zeros.  The call reads state only.
#include <algorithm>
#include <cmath>

#include "nsx_post.hpp"

namespace nsx {

constexpr int PROBE_TILE = 64;        // points staged in LDS at a time
constexpr int PROBE_MAX = 65536;
constexpr int PROBE_RANK_BITS = 48;   // ranks per double of the owner collective

// best[p] starts at INT32_MAX.  counted: the cells this handle searches (all of them on one process; diag.counted in a distributed run).
template <int DIM>
__global__ __launch_bounds__(64) void k_probe_locate(int n_cells, const uint8_t *__restrict__ counted, const double *__restrict__ geo,
                                                     const double *__restrict__ x0, int n_points, const double *__restrict__ points, double tol,
                                                     int32_t *__restrict__ best) {
  __shared__ double sp[PROBE_TILE * DIM];
  const int cell = blockIdx.x * 64 + threadIdx.x;
  const int c = min(cell, n_cells - 1);  // lanes behind the last cell load that cell's map and never match
  const bool live = cell < n_cells && counted[c];
  double Ji[DIM][DIM], X0[DIM];
  load_cell_map<DIM>(n_cells, c, geo, x0, Ji, X0);
  for (int p0 = 0; p0 < n_points; p0 += PROBE_TILE) {
    const int nt = min(PROBE_TILE, n_points - p0);
    __syncthreads();  // the previous tile has been read
    for (int i = threadIdx.x; i < nt * DIM; i += 64) sp[i] = points[(size_t)p0 * DIM + i];
    __syncthreads();
    for (int j = 0; j < nt; ++j) {
      double lam[DIM + 1];
      const bool in = live && probe_lambda<DIM>(Ji, X0, sp + j * DIM, tol, lam);
      const unsigned long long hits = __ballot(in);
      if (hits != 0 && (int)threadIdx.x == __ffsll(hits) - 1) atomicMin(best + p0 + j, cell);
    }
  }
}

// cells[p] = best[p] or -1; lam[k][p] = lambda_k of point p in that cell (0 where there is none)
template <int DIM>
__global__ __launch_bounds__(64) void k_probe_finish(int n_cells, const double *__restrict__ geo, const double *__restrict__ x0, int n_points,
                                                     const double *__restrict__ points, const int32_t *__restrict__ best, int32_t *__restrict__ cells,
                                                     double *__restrict__ lam_out) {
  const int p = blockIdx.x * 64 + threadIdx.x;
  if (p >= n_points) return;
  const int32_t b = best[p];
  const bool found = b >= 0 && b < n_cells;
  cells[p] = found ? b : -1;
  double lam[DIM + 1];
#pragma unroll
  for (int k = 0; k <= DIM; ++k) lam[k] = 0.0;
  if (found) {
    double Ji[DIM][DIM], X0[DIM], x[DIM];
    load_cell_map<DIM>(n_cells, b, geo, x0, Ji, X0);
#pragma unroll
    for (int d = 0; d < DIM; ++d) x[d] = points[(size_t)p * DIM + d];
    (void)probe_lambda<DIM>(Ji, X0, x, 0.0, lam);
  }
#pragma unroll
  for (int k = 0; k <= DIM; ++k) lam_out[(size_t)k * n_points + p] = lam[k];
}

// The shape functions and the push-forward are p2_shape / push_forward_col (nsx_post.hpp).  Everything is unrolled: lam, g, u and H are
// indexed statically and stay in registers.
// out planes: [0, DIM) velocity, [DIM] pressure, [DIM + 1 + i * DIM + j] d_j u_i.
template <int DIM, int NP2>
__global__ __launch_bounds__(64) void k_probe_eval(int n_points, const int32_t *__restrict__ cells, const double *__restrict__ lam_in, int n_cells,
                                                   const int32_t *__restrict__ cell_n2, const int32_t *__restrict__ cell_n1,
                                                   const double *__restrict__ geo, const double *__restrict__ sol, int off_p,
                                                   double *__restrict__ out) {
  constexpr int NV = DIM + 1, NOUT = DIM + 1 + DIM * DIM;
  const int p = blockIdx.x * 64 + threadIdx.x;
  if (p >= n_points) return;
  const int cell = cells[p];
  if (cell < 0) {  // in no cell, or another rank evaluates it
#pragma unroll
    for (int k = 0; k < NOUT; ++k) out[(size_t)k * n_points + p] = 0.0;
    return;
  }
  double lam[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) lam[k] = lam_in[(size_t)k * n_points + p];
  double u[DIM], H[DIM][DIM], pr = 0.0;
#pragma unroll
  for (int i = 0; i < DIM; ++i) {
    u[i] = 0.0;
#pragma unroll
    for (int k = 0; k < DIM; ++k) H[i][k] = 0.0;
  }
#pragma unroll
  for (int v = 0; v < NV; ++v) pr += lam[v] * sol[(size_t)off_p + cell_n1[(size_t)v * n_cells + cell]];
#pragma unroll
  for (int a = 0; a < NP2; ++a) {
    double g[NV], n;
    p2_shape<DIM, true, true>(a, lam, n, g);
    const int node = cell_n2[(size_t)a * n_cells + cell];
#pragma unroll
    for (int i = 0; i < DIM; ++i) {
      const double U = sol[(size_t)node * DIM + i];
      u[i] += n * U;
#pragma unroll
      for (int k = 0; k < DIM; ++k) H[i][k] += U * (g[k + 1] - g[0]);
    }
  }
  double *o = out + p;
#pragma unroll
  for (int i = 0; i < DIM; ++i) o[(size_t)i * n_points] = u[i];
  o[(size_t)DIM * n_points] = pr;
#pragma unroll
  for (int j = 0; j < DIM; ++j)
    push_forward_col<DIM>(n_cells, cell, geo, H, j, [&](int i, double s) { o[(size_t)(DIM + 1 + i * DIM + j) * n_points] = s; });
}

// ------------------------------------------------------------------ host drivers
void probe_mesh_setup(nsx_handle *h, const double *cell_coords) {
  const int dim = h->dim, nv = dim + 1, n_cells = h->n_cells;
  std::vector<double> x0((size_t)dim * n_cells);
  for (int c = 0; c < n_cells; ++c)
    for (int d = 0; d < dim; ++d) x0[(size_t)d * n_cells + c] = cell_coords[(size_t)c * nv * dim + d];
  h->probe.cell_x0.upload(x0, h->stream);
}

template <int DIM>
static void launch_locate(nsx_handle *h, int n, const double *points, double tol, int32_t *best, int32_t *cells, double *lam) {
  {
    LaunchScope ls(h, "probe_locate", 8.0 * (DIM * DIM + DIM) * h->n_cells);
    hipLaunchKernelGGL((k_probe_locate<DIM>), dim3(cdiv(h->n_cells, 64)), dim3(64), 0, h->stream, h->n_cells, h->diag.counted.p, h->geo.p, h->probe.cell_x0.p, n,
                       points, tol, best);
  }
  hipLaunchKernelGGL((k_probe_finish<DIM>), dim3(cdiv(n, 64)), dim3(64), 0, h->stream, h->n_cells, h->geo.p, h->probe.cell_x0.p, n, points, best, cells, lam);
  HIP_CHECK(hipGetLastError());
}

void probe_locate(nsx_handle *h, int n, const double *points, double tol, int32_t *best, int32_t *cells, double *lam) {
  if (h->dim == 2) launch_locate<2>(h, n, points, tol, best, cells, lam);
  else launch_locate<3>(h, n, points, tol, best, cells, lam);
}

static void set_probes(nsx_handle *h, int n, const double *points, double tol) {
  post_check_space(h, "nsx_set_probes");
  if (n < 0) NSX_THROW(NSX_ERR_ARG, "n_points = %d", n);
  if (n > PROBE_MAX) NSX_THROW(NSX_ERR_UNSUPPORTED, "%d probes: at most %d per handle", n, PROBE_MAX);
  if (n > 0 && !points) NSX_THROW(NSX_ERR_ARG, "null points");
  if (!(tol < 1.0)) NSX_THROW(NSX_ERR_ARG, "tol = %g: a value below 1 (negative: the library's own, %g)", tol, PROBE_TOL);
  const int dim = h->dim, nl = dim + 1;
  for (size_t i = 0; i < (size_t)n * dim; ++i)
    if (!std::isfinite(points[i])) NSX_THROW(NSX_ERR_ARG, "probe %zu: coordinate %zu is not finite", i / dim, i % dim);
  h->probe.mesh_changed();  // the earlier set is given up, as by a new mesh
  if (n == 0) return;
  if (tol < 0.0) tol = PROBE_TOL;
  HIP_CHECK(hipSetDevice(h->prm.device));
  DevBuf<double> pts;
  DevBuf<int32_t> best;
  pts.upload(points, (size_t)n * dim, h->stream);
  best.upload(std::vector<int32_t>((size_t)n, INT32_MAX), h->stream);
  h->probe.cell.alloc(n);
  h->probe.lambda.alloc((size_t)nl * n);
  h->probe.out.alloc((size_t)(dim + 1 + dim * dim) * n);
  probe_locate(h, n, pts.p, tol, best.p, h->probe.cell.p, h->probe.lambda.p);
  std::vector<int32_t> cells((size_t)n), owner((size_t)n);
  std::vector<double> lam_soa((size_t)nl * n);
  h->probe.cell.download(cells.data(), cells.size(), h->stream);
  h->probe.lambda.download(lam_soa.data(), lam_soa.size(), h->stream);
  for (int p = 0; p < n; ++p) owner[p] = cells[p] >= 0 ? h->rank : -1;
  if (h->comm && h->world > 1) {
    // who found what, through the SUM collective: rank r adds bit r % 48 of double r / 48 of every point it found -- distinct powers of two below
    // 2^48 add up exactly in any order, and the lowest bit set is the lowest rank that found the point.  Every rank issues this ONE collective.
    const int chunks = cdiv(h->world, PROBE_RANK_BITS);
    std::vector<double> flags((size_t)n * chunks, 0.0);
    for (int p = 0; p < n; ++p)
      if (cells[p] >= 0) flags[(size_t)p * chunks + h->rank / PROBE_RANK_BITS] = std::ldexp(1.0, h->rank % PROBE_RANK_BITS);
    DevBuf<double> dflags;
    dflags.upload(flags, h->stream);
    comm_allreduce_partials(h, dflags.p, (int)flags.size());
    dflags.download(flags.data(), flags.size(), h->stream);
    bool changed = false;
    for (int p = 0; p < n; ++p) {
      owner[p] = -1;
      for (int c = 0; c < chunks && owner[p] < 0; ++c) {
        const unsigned long long bits = (unsigned long long)flags[(size_t)p * chunks + c];
        if (bits) owner[p] = c * PROBE_RANK_BITS + __builtin_ctzll(bits);
      }
      if (cells[p] >= 0 && owner[p] != h->rank) {  // a lower rank holds the point on a shared face: it evaluates
        cells[p] = -1;
        for (int k = 0; k < nl; ++k) lam_soa[(size_t)k * n + p] = 0.0;
        changed = true;
      }
    }
    if (changed) h->probe.cell.upload(cells, h->stream);
  }
  h->probe.lambda_h.resize((size_t)n * nl);
  for (int p = 0; p < n; ++p)
    for (int k = 0; k < nl; ++k) h->probe.lambda_h[(size_t)p * nl + k] = lam_soa[(size_t)k * n + p];
  h->probe.cells_h = std::move(cells);
  h->probe.owner_h = std::move(owner);
  h->probe.n = n;
}

template <int DIM, int NP2>
static void launch_eval(nsx_handle *h) {
  int mine = 0;
  for (int32_t c : h->probe.cells_h) mine += c >= 0;
  constexpr int NOUT = DIM + 1 + DIM * DIM;
  const double bytes = 4.0 * h->probe.n + (double)mine * (8.0 * (DIM + 1) + 4.0 * (NP2 + DIM + 1) + 8.0 * (NP2 * DIM + DIM + 1) + 8.0 * DIM * DIM) + 8.0 * NOUT * h->probe.n;
  LaunchScope ls(h, "probe_eval", bytes);
  hipLaunchKernelGGL((k_probe_eval<DIM, NP2>), dim3(cdiv(h->probe.n, 64)), dim3(64), 0, h->stream, h->probe.n, h->probe.cell.p, h->probe.lambda.p, h->n_cells,
                     h->cell_n2.p, h->cell_n1.p, h->geo.p, h->sol.p, h->off_p, h->probe.out.p);
}

static void eval_probes(nsx_handle *h, double *velocity, double *pressure, double *gradient, int32_t *found) {
  post_check_space(h, "nsx_eval_probes");
  if (h->probe.n == 0) NSX_THROW(NSX_ERR_ARG, "nsx_set_probes first");
  HIP_CHECK(hipSetDevice(h->prm.device));
  const int dim = h->dim, n = h->probe.n, nout = dim + 1 + dim * dim;
  if (dim == 2) launch_eval<2, 6>(h);
  else launch_eval<3, 10>(h);
  HIP_CHECK(hipGetLastError());
  // the owner's values and exact zeros from everybody else (x + 0 is exact, NaN and inf survive): every rank gets the same bits
  if (h->comm && h->world > 1) comm_allreduce_partials(h, h->probe.out.p, nout * n);
  std::vector<double> v((size_t)nout * n);
  h->probe.out.download(v.data(), v.size(), h->stream);
  for (int p = 0; p < n; ++p) {
    if (velocity)
      for (int i = 0; i < dim; ++i) velocity[(size_t)p * dim + i] = v[(size_t)i * n + p];
    if (pressure) pressure[p] = v[(size_t)dim * n + p];
    if (gradient)
      for (int k = 0; k < dim * dim; ++k) gradient[(size_t)p * dim * dim + k] = v[(size_t)(dim + 1 + k) * n + p];
    if (found) found[p] = h->probe.owner_h[p] >= 0;
  }
}

}  // namespace nsx

extern "C" {

int nsx_set_probes(nsx_handle *h, int n_points, const double *points, double tol) {
  NSX_TRY(h)
  nsx::set_probes(h, n_points, points, tol);
  NSX_CATCH(h)
}

int nsx_get_probe_cells(nsx_handle *h, int32_t *cells, int32_t *owners, double *lambda) {
  NSX_TRY(h)
  nsx::post_check_space(h, "nsx_get_probe_cells");
  if (h->probe.n == 0) NSX_THROW(NSX_ERR_ARG, "nsx_set_probes first");
  if (cells) std::copy(h->probe.cells_h.begin(), h->probe.cells_h.end(), cells);
  if (owners) std::copy(h->probe.owner_h.begin(), h->probe.owner_h.end(), owners);
  if (lambda) std::copy(h->probe.lambda_h.begin(), h->probe.lambda_h.end(), lambda);
  NSX_CATCH(h)
}

int nsx_eval_probes(nsx_handle *h, double *velocity, double *pressure, double *gradient, int32_t *found) {
  NSX_TRY(h)
  nsx::eval_probes(h, velocity, pressure, gradient, found);
  NSX_CATCH(h)
}

}  // extern "C"
