// nsx_lattice.hip — lattice sampling: u_h, p_h, grad u_h and the nodal fields on a regular axis-aligned grid (include/nsx.h, section
// "lattice sampling").  No counterpart in the reference (its output() writes the unstructured volume as a VTU).
//
// The point probes search every cell for every point (k_probe_locate: n_cells * n_points tests).  For a lattice the work is reversed: a cell
// knows which lattice points its bounding box can hold (host/lattice_box.hpp), so locating is a rasterisation, O(points covered).
//
//   k_lattice_locate  one CELL PER LANE, one wave per workgroup, as the cell kernels: a lane loads the vertices, X0 and J^-1 of its cell and
//                     forms the cell's index box.  The wave then works through its non-empty boxes one after the other (a ballot picks the
//                     next, its data is broadcast through LDS); the 64 lanes stride over the box's points, x fastest, each computing x by the
//                     pinned formula (lattice_coord) and lambda by probe_lambda, and issuing atomicMin(owner + index, cell) on a hit.  A
//                     lattice coarser than the mesh leaves most boxes empty (one ballot); a lattice finer than the mesh has boxes of
//                     thousands of points, which the wave shares instead of serialising one lane.  The integer minimum is exact and
//                     order-free: the owner depends on the mesh and the lattice alone.
//   k_lattice_finish  INT32_MAX -> -1, and the owned points counted: per workgroup in a fixed order, the workgroups' counts added by the host.
//   k_lattice_eval    one LATTICE POINT PER LANE, x fastest: the lane reads its owner, recomputes x and lambda in the owner cell (no lambda is
//                     stored per point: at 256^3 that would be 0.5 GB) and gathers the cell's values; neighbouring lanes mostly share a cell,
//                     so the gathers hit in cache.  `WHAT` is a template parameter: an image of the velocity alone does not carry the
//                     gradient's registers.  SoA planes, coalesced stores, exact zeros where there is no owner.  Everything is unrolled and
//                     statically indexed, as k_probe_eval; no table is read at run time (see the note above p2_shape).
// The three entries read state only.
#include <algorithm>
#include <cmath>

#include "../host/lattice_box.hpp"
#include "../host/nodal_patch.hpp"
#include "nsx_post.hpp"

namespace nsx {

constexpr int64_t LATTICE_MAX = (int64_t)1 << 26;  // points per lattice
constexpr int LATTICE_WG = 256;                    // k_lattice_finish, k_lattice_eval
constexpr int LATTICE_FINISH_WGS = 1024;           // workgroups of k_lattice_finish at most (grid-stride)
constexpr int LATTICE_ALL = NSX_LATTICE_VELOCITY | NSX_LATTICE_PRESSURE | NSX_LATTICE_GRADIENT | NSX_LATTICE_NODAL;

template <int DIM>
struct LatticeGrid {
  double origin[DIM], spacing[DIM];
  int32_t counts[DIM];
};

// owner[p] starts at INT32_MAX.  cellx: SoA [(dim+1) dim][n_cells] vertex coordinates (iso.cellx).
template <int DIM>
__global__ __launch_bounds__(64) void k_lattice_locate(int n_cells, const uint8_t *__restrict__ counted, const double *__restrict__ geo,
                                                       const double *__restrict__ x0, const double *__restrict__ cellx, LatticeGrid<DIM> g, double tol,
                                                       int32_t *__restrict__ owner) {
  __shared__ double s_map[64][DIM * DIM + DIM];
  __shared__ int32_t s_box[64][2 * DIM];
  const int lane = threadIdx.x;
  const int cell = blockIdx.x * 64 + lane;
  const int c = min(cell, n_cells - 1);  // lanes behind the last cell load that cell and have no box
  {
    double Ji[DIM][DIM], X0[DIM], X[DIM + 1][DIM];
    load_cell_map<DIM>(n_cells, c, geo, x0, Ji, X0);
#pragma unroll
    for (int v = 0; v <= DIM; ++v)
#pragma unroll
      for (int d = 0; d < DIM; ++d) X[v][d] = cellx[(size_t)(v * DIM + d) * n_cells + c];
    int32_t lo[DIM], hi[DIM];
    const bool any = lattice_box<DIM>(X, tol, g.origin, g.spacing, g.counts, lo, hi) && cell < n_cells && counted[c];
#pragma unroll
    for (int k = 0; k < DIM; ++k) {
      s_map[lane][DIM * DIM + k] = X0[k];
#pragma unroll
      for (int d = 0; d < DIM; ++d) s_map[lane][k * DIM + d] = Ji[k][d];
      s_box[lane][2 * k] = any ? lo[k] : 0;
      s_box[lane][2 * k + 1] = any ? hi[k] : -1;
    }
  }
  __syncthreads();
  unsigned long long todo = __ballot(s_box[lane][0] <= s_box[lane][1]);
  while (todo != 0) {  // wave-uniform
    const int src = __ffsll(todo) - 1;
    todo &= todo - 1;
    double Ji[DIM][DIM], X0[DIM];
    int32_t lo[DIM];
    uint32_t ext[DIM];
#pragma unroll
    for (int k = 0; k < DIM; ++k) {
      X0[k] = s_map[src][DIM * DIM + k];
#pragma unroll
      for (int d = 0; d < DIM; ++d) Ji[k][d] = s_map[src][k * DIM + d];
      lo[k] = s_box[src][2 * k];
      ext[k] = (uint32_t)(s_box[src][2 * k + 1] - lo[k] + 1);
    }
    // a box holds at most n_total <= 2^26 points: the position inside the box is decomposed in 32 bits, the lattice index is 64-bit
    uint32_t n_box = 1;
#pragma unroll
    for (int k = 0; k < DIM; ++k) n_box *= ext[k];
    const int32_t src_cell = blockIdx.x * 64 + src;
    for (uint32_t t = lane; t < n_box; t += 64) {
      uint32_t r = t;
      int32_t i[DIM];
#pragma unroll
      for (int k = 0; k < DIM - 1; ++k) {
        const uint32_t q = r / ext[k];
        i[k] = lo[k] + (int32_t)(r - q * ext[k]);
        r = q;
      }
      i[DIM - 1] = lo[DIM - 1] + (int32_t)r;
      double x[DIM], lam[DIM + 1];
      int64_t idx = 0;
#pragma unroll
      for (int k = DIM - 1; k >= 0; --k) {
        x[k] = lattice_coord(g.origin[k], g.spacing[k], i[k]);
        idx = idx * (int64_t)g.counts[k] + (int64_t)i[k];
      }
      if (probe_lambda<DIM>(Ji, X0, x, tol, lam)) atomicMin(owner + idx, src_cell);
    }
  }
}

// owner: INT32_MAX -> -1; part[workgroup] = owned points of the workgroup's share, summed in a fixed order
__global__ __launch_bounds__(LATTICE_WG) void k_lattice_finish(long long n_total, int n_cells, int32_t *__restrict__ owner, long long *__restrict__ part) {
  __shared__ long long s_sum[LATTICE_WG];
  long long mine = 0;
  for (long long p = (long long)blockIdx.x * LATTICE_WG + threadIdx.x; p < n_total; p += (long long)gridDim.x * LATTICE_WG) {
    const int32_t o = owner[p];
    const bool found = o >= 0 && o < n_cells;
    if (!found) owner[p] = -1;
    mine += found;
  }
  s_sum[threadIdx.x] = mine;
  __syncthreads();
  for (int w = LATTICE_WG / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) s_sum[threadIdx.x] += s_sum[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = s_sum[0];
}

// The arithmetic of k_probe_eval (p2_shape, push_forward_col), lambda by probe_lambda in the owner cell.  NP: planes of nodal_out sampled
// (nodal_planes(DIM) with NSX_LATTICE_NODAL, else 0); slot: internal P2 node -> slot of nodal_out.
template <int DIM, int NP2, int WHAT>
__global__ __launch_bounds__(LATTICE_WG) void k_lattice_eval(long long n_total, LatticeGrid<DIM> g, const int32_t *__restrict__ owner, int n_cells,
                                                             const int32_t *__restrict__ cell_n2, const int32_t *__restrict__ cell_n1,
                                                             const double *__restrict__ geo, const double *__restrict__ x0,
                                                             const double *__restrict__ sol, int off_p, const int32_t *__restrict__ slot,
                                                             const double *__restrict__ nodal_out, size_t n_slots, double *__restrict__ vel,
                                                             double *__restrict__ pres, double *__restrict__ grad, double *__restrict__ nodal) {
  constexpr int NV = DIM + 1;
  constexpr bool VEL = (WHAT & NSX_LATTICE_VELOCITY) != 0, PRES = (WHAT & NSX_LATTICE_PRESSURE) != 0, GRAD = (WHAT & NSX_LATTICE_GRADIENT) != 0,
                 NODAL = (WHAT & NSX_LATTICE_NODAL) != 0;
  constexpr int NP = NODAL ? nodal_planes(DIM) : 1;
  const long long p = (long long)blockIdx.x * LATTICE_WG + threadIdx.x;
  if (p >= n_total) return;
  const size_t n = (size_t)n_total;
  const int cell = owner[p];
  if (cell < 0) {  // in no cell
    if (VEL) {
#pragma unroll
      for (int i = 0; i < DIM; ++i) vel[(size_t)i * n + p] = 0.0;
    }
    if (PRES) pres[p] = 0.0;
    if (GRAD) {
#pragma unroll
      for (int k = 0; k < DIM * DIM; ++k) grad[(size_t)k * n + p] = 0.0;
    }
    if (NODAL) {
#pragma unroll
      for (int k = 0; k < NP; ++k) nodal[(size_t)k * n + p] = 0.0;
    }
    return;
  }
  double lam[NV];
  {
    double Ji[DIM][DIM], X0[DIM], x[DIM];
    load_cell_map<DIM>(n_cells, cell, geo, x0, Ji, X0);
    uint32_t r = (uint32_t)p;  // p < n_total <= 2^26: the position is decomposed in 32 bits, the plane offsets are 64-bit
#pragma unroll
    for (int k = 0; k < DIM; ++k) {
      const uint32_t q = k + 1 < DIM ? r / (uint32_t)g.counts[k] : 0u;
      x[k] = lattice_coord(g.origin[k], g.spacing[k], (int32_t)(r - q * (uint32_t)g.counts[k]));
      r = q;
    }
    (void)probe_lambda<DIM>(Ji, X0, x, 0.0, lam);
  }
  double u[DIM], H[DIM][DIM], V[NP];
#pragma unroll
  for (int i = 0; i < DIM; ++i) {
    u[i] = 0.0;
#pragma unroll
    for (int k = 0; k < DIM; ++k) H[i][k] = 0.0;
  }
#pragma unroll
  for (int k = 0; k < NP; ++k) V[k] = 0.0;
  if (PRES) {
    double pr = 0.0;
#pragma unroll
    for (int v = 0; v < NV; ++v) pr += lam[v] * sol[(size_t)off_p + cell_n1[(size_t)v * n_cells + cell]];
    pres[p] = pr;
  }
#pragma unroll
  for (int a = 0; a < NP2; ++a) {
    double gl[NV], na = 0.0;
    p2_shape<DIM, VEL || NODAL, GRAD>(a, lam, na, gl);
    const int node = cell_n2[(size_t)a * n_cells + cell];
    if (VEL || GRAD) {
#pragma unroll
      for (int i = 0; i < DIM; ++i) {
        const double U = sol[(size_t)node * DIM + i];
        if (VEL) u[i] += na * U;
        if (GRAD) {
#pragma unroll
          for (int k = 0; k < DIM; ++k) H[i][k] += U * (gl[k + 1] - gl[0]);
        }
      }
    }
    if (NODAL) {
      const size_t s = (size_t)slot[node];
#pragma unroll
      for (int k = 0; k < NP; ++k) V[k] += na * nodal_out[(size_t)k * n_slots + s];
    }
  }
  if (VEL) {
#pragma unroll
    for (int i = 0; i < DIM; ++i) vel[(size_t)i * n + p] = u[i];
  }
  if (GRAD) {
#pragma unroll
    for (int j = 0; j < DIM; ++j) push_forward_col<DIM>(n_cells, cell, geo, H, j, [&](int i, double s) { grad[(size_t)(i * DIM + j) * n + p] = s; });
  }
  if (NODAL) {
#pragma unroll
    for (int k = 0; k < NP; ++k) nodal[(size_t)k * n + p] = V[k];
  }
}

// ------------------------------------------------------------------ host drivers
static void lattice_check_space(nsx_handle *h, const char *who) {
  post_check_space(h, who);
  if (h->world > 1) NSX_THROW(NSX_ERR_UNSUPPORTED, "%s: lattice sampling on %d processes: merging the ranks' lattices is not supported", who, h->world);
}

static void lattice_need(nsx_handle *h, const char *who) {
  lattice_check_space(h, who);
  if (!h->lattice.set) NSX_THROW(NSX_ERR_ARG, "%s: nsx_set_lattice first", who);
}

template <int DIM>
static LatticeGrid<DIM> lattice_grid(const LatticeState &s) {
  LatticeGrid<DIM> g;
  for (int d = 0; d < DIM; ++d) {
    g.origin[d] = s.origin[d];
    g.spacing[d] = s.spacing[d];
    g.counts[d] = s.counts[d];
  }
  return g;
}

template <int DIM>
static void launch_lattice_locate(nsx_handle *h, const LatticeState &s, int32_t *owner, long long *part, int n_part) {
  {
    LaunchScope ls(h, "lattice_locate", 8.0 * (2 * DIM * DIM + 2 * DIM) * h->n_cells + 4.0 * (double)s.n_total);
    hipLaunchKernelGGL((k_lattice_locate<DIM>), dim3(cdiv(h->n_cells, 64)), dim3(64), 0, h->stream, h->n_cells, h->diag.counted.p, h->geo.p, h->probe.cell_x0.p,
                       h->iso.cellx.p, lattice_grid<DIM>(s), s.tol, owner);
  }
  LaunchScope ls(h, "lattice_finish", 8.0 * (double)s.n_total);
  hipLaunchKernelGGL(k_lattice_finish, dim3(n_part), dim3(LATTICE_WG), 0, h->stream, (long long)s.n_total, h->n_cells, owner, part);
}

static void set_lattice(nsx_handle *h, const double *origin, const double *spacing, const int32_t *counts, double tol, int64_t *n_found) {
  lattice_check_space(h, "nsx_set_lattice");
  const int dim = h->dim;
  if (!origin && !spacing && !counts) {  // clears the lattice
    h->lattice.clear();
    if (n_found) *n_found = 0;
    return;
  }
  if (!origin || !spacing || !counts) NSX_THROW(NSX_ERR_ARG, "nsx_set_lattice: origin, spacing and counts are all null (clears the lattice) or none of them is");
  if (!(tol < 1.0) || !std::isfinite(tol)) NSX_THROW(NSX_ERR_ARG, "nsx_set_lattice: tol = %g: a finite value below 1 (negative: the library's own, %g)", tol, PROBE_TOL);
  LatticeState s;
  s.tol = tol < 0.0 ? PROBE_TOL : tol;
  for (int d = 0; d < dim; ++d) {
    if (counts[d] < 1) NSX_THROW(NSX_ERR_ARG, "nsx_set_lattice: counts[%d] = %d", d, counts[d]);
    if (!std::isfinite(spacing[d]) || !(spacing[d] > 0.0)) NSX_THROW(NSX_ERR_ARG, "nsx_set_lattice: spacing[%d] = %g: a finite value above 0", d, spacing[d]);
    if (!std::isfinite(origin[d])) NSX_THROW(NSX_ERR_ARG, "nsx_set_lattice: origin[%d] is not finite", d);
    // neighbouring coordinates are distinct finite doubles at either end of the axis
    const int32_t n = counts[d];
    const double first = lattice_coord(origin[d], spacing[d], 0), last = lattice_coord(origin[d], spacing[d], n - 1);
    bool ok = std::isfinite(first) && std::isfinite(last);
    if (n > 1) ok = ok && first < lattice_coord(origin[d], spacing[d], 1) && lattice_coord(origin[d], spacing[d], n - 2) < last;
    if (!ok) NSX_THROW(NSX_ERR_ARG, "nsx_set_lattice: axis %d: origin %g, spacing %g, %d points: neighbouring coordinates are not distinct finite doubles", d, origin[d], spacing[d], n);
    s.origin[d] = origin[d];
    s.spacing[d] = spacing[d];
    s.counts[d] = n;
  }
  int64_t n_total = 1;  // at most 2^26 * 2^31 before the test
  for (int d = 0; d < dim; ++d) {
    n_total *= counts[d];
    if (n_total > LATTICE_MAX) NSX_THROW(NSX_ERR_UNSUPPORTED, "nsx_set_lattice: more than 2^26 = %lld lattice points", (long long)LATTICE_MAX);
  }
  s.n_total = n_total;
  HIP_CHECK(hipSetDevice(h->prm.device));
  iso_ensure_coords(h);
  const int n_part = std::min<int64_t>(LATTICE_FINISH_WGS, cdiv(n_total, LATTICE_WG));
  DevBuf<long long> dpart;
  s.owner.alloc((size_t)n_total);
  dpart.alloc((size_t)n_part);
  HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)s.owner.p, INT32_MAX, (size_t)n_total, h->stream));
  if (dim == 2) launch_lattice_locate<2>(h, s, s.owner.p, dpart.p, n_part);
  else launch_lattice_locate<3>(h, s, s.owner.p, dpart.p, n_part);
  HIP_CHECK(hipGetLastError());
  std::vector<long long> part((size_t)n_part);
  dpart.download(part.data(), part.size(), h->stream);
  for (long long c : part) s.n_found += c;
  if (s.n_found < 0 || s.n_found > n_total) NSX_THROW(NSX_ERR_NUMERIC, "nsx_set_lattice: %lld of %lld points counted as owned", (long long)s.n_found, (long long)n_total);
  // from here on the earlier lattice and its results are given up (the result buffers stay for the next nsx_eval_lattice to reuse)
  h->lattice.what = 0;
  std::swap(h->lattice.owner.p, s.owner.p);
  std::swap(h->lattice.owner.n, s.owner.n);
  for (int d = 0; d < 3; ++d) {
    h->lattice.origin[d] = s.origin[d];
    h->lattice.spacing[d] = s.spacing[d];
    h->lattice.counts[d] = s.counts[d];
  }
  h->lattice.tol = s.tol;
  h->lattice.n_total = n_total;
  h->lattice.n_found = s.n_found;
  h->lattice.set = true;
  if (n_found) *n_found = s.n_found;
}

template <int DIM, int NP2, int WHAT>
static void launch_lattice_eval(nsx_handle *h) {
  LatticeState &s = h->lattice;
  constexpr int NPL = ((WHAT & NSX_LATTICE_VELOCITY) ? DIM : 0) + ((WHAT & NSX_LATTICE_PRESSURE) ? 1 : 0) + ((WHAT & NSX_LATTICE_GRADIENT) ? DIM * DIM : 0) +
                      ((WHAT & NSX_LATTICE_NODAL) ? nodal_planes(DIM) : 0);
  // per owned point: the cell map and the connectivity; the nodal values themselves are shared by the points of a cell
  const double bytes = (4.0 + 8.0 * NPL) * (double)s.n_total + (double)s.n_found * (8.0 * (DIM * DIM + DIM) + 4.0 * (NP2 + DIM + 1));
  LaunchScope ls(h, "lattice_eval", bytes);
  hipLaunchKernelGGL((k_lattice_eval<DIM, NP2, WHAT>), dim3(cdiv(s.n_total, LATTICE_WG)), dim3(LATTICE_WG), 0, h->stream, (long long)s.n_total, lattice_grid<DIM>(s),
                     s.owner.p, h->n_cells, h->cell_n2.p, h->cell_n1.p, h->geo.p, h->probe.cell_x0.p, h->sol.p, h->off_p, h->iso.slot.p, h->nodal.out.p,
                     (size_t)h->nodal.tiles * NODAL_TILE, s.vel.p, s.pres.p, s.grad.p, s.nodal.p);
}

template <int DIM, int NP2, int WHAT = LATTICE_ALL>
static void dispatch_lattice_eval(nsx_handle *h, int what) {
  if constexpr (WHAT == 0) {
    (void)what;
  } else {
    if (what == WHAT) launch_lattice_eval<DIM, NP2, WHAT>(h);
    else dispatch_lattice_eval<DIM, NP2, WHAT - 1>(h, what);
  }
}

static void eval_lattice(nsx_handle *h, int what) {
  lattice_need(h, "nsx_eval_lattice");
  if (what == 0 || (what & ~LATTICE_ALL) != 0) NSX_THROW(NSX_ERR_ARG, "nsx_eval_lattice: what = %d: an OR of NSX_LATTICE_VELOCITY ... NSX_LATTICE_NODAL", what);
  if (!h->sol.p || h->sol.n < (size_t)h->len_blk) NSX_THROW(NSX_ERR_ARG, "nsx_eval_lattice: the handle holds no state yet");
  if ((what & NSX_LATTICE_NODAL) && (!h->nodal.have_patches || !h->nodal.valid))
    NSX_THROW(NSX_ERR_ARG, "nsx_eval_lattice: NSX_LATTICE_NODAL needs nsx_compute_nodal_fields first");
  if ((what & NSX_LATTICE_NODAL) && h->N2_loc != h->N2) NSX_THROW(NSX_ERR_UNSUPPORTED, "nsx_eval_lattice: NSX_LATTICE_NODAL with ghost nodes (they have no nodal results)");
  HIP_CHECK(hipSetDevice(h->prm.device));
  LatticeState &s = h->lattice;
  const int dim = h->dim;
  const size_t n = (size_t)s.n_total;
  if (what & NSX_LATTICE_NODAL) iso_ensure_slots(h);
  if (what & NSX_LATTICE_VELOCITY) s.vel.alloc((size_t)dim * n);
  if (what & NSX_LATTICE_PRESSURE) s.pres.alloc(n);
  if (what & NSX_LATTICE_GRADIENT) s.grad.alloc((size_t)dim * dim * n);
  if (what & NSX_LATTICE_NODAL) s.nodal.alloc((size_t)nodal_planes(dim) * n);
  s.what = 0;  // a failure below leaves no results
  if (dim == 2) dispatch_lattice_eval<2, 6>(h, what);
  else dispatch_lattice_eval<3, 10>(h, what);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipStreamSynchronize(h->stream));
  s.what = what;
}

static void get_lattice(nsx_handle *h, int quantity, int which, double *values) {
  lattice_need(h, "nsx_get_lattice");
  if (!values) NSX_THROW(NSX_ERR_ARG, "nsx_get_lattice: null values");
  const LatticeState &s = h->lattice;
  const int dim = h->dim;
  const size_t n = (size_t)s.n_total;
  const double *src = nullptr;
  int nc = 0;
  switch (quantity) {
    case NSX_LATTICE_VELOCITY: src = s.vel.p, nc = dim; break;
    case NSX_LATTICE_PRESSURE: src = s.pres.p, nc = 1; break;
    case NSX_LATTICE_GRADIENT: src = s.grad.p, nc = dim * dim; break;
    case NSX_LATTICE_NODAL:
      if (which < 0 || which >= NSX_FIELD_COUNT) NSX_THROW(NSX_ERR_ARG, "nsx_get_lattice: nodal field %d (NSX_FIELD_GRADIENT ... NSX_FIELD_DIVERGENCE)", which);
      src = s.nodal.p + (size_t)nodal_first_plane(dim, which) * n, nc = nodal_components(dim, which);
      break;
    default: NSX_THROW(NSX_ERR_ARG, "nsx_get_lattice: quantity %d: one of NSX_LATTICE_VELOCITY ... NSX_LATTICE_NODAL", quantity);
  }
  if (!(s.what & quantity)) NSX_THROW(NSX_ERR_ARG, "nsx_get_lattice: the last nsx_eval_lattice did not compute quantity %d", quantity);
  HIP_CHECK(hipSetDevice(h->prm.device));
  HIP_CHECK(hipMemcpyAsync(values, src, (size_t)nc * n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIP_CHECK(hipStreamSynchronize(h->stream));
}

}  // namespace nsx

extern "C" {

int nsx_set_lattice(nsx_handle *h, const double *origin, const double *spacing, const int32_t *counts, double tol, int64_t *n_found) {
  NSX_TRY(h)
  nsx::set_lattice(h, origin, spacing, counts, tol, n_found);
  NSX_CATCH(h)
}

int nsx_get_lattice_cells(nsx_handle *h, int32_t *cells) {
  NSX_TRY(h)
  nsx::lattice_need(h, "nsx_get_lattice_cells");
  if (!cells) NSX_THROW(NSX_ERR_ARG, "nsx_get_lattice_cells: null cells");
  HIP_CHECK(hipSetDevice(h->prm.device));
  h->lattice.owner.download(cells, (size_t)h->lattice.n_total, h->stream);
  NSX_CATCH(h)
}

int nsx_eval_lattice(nsx_handle *h, int what) {
  NSX_TRY(h)
  nsx::eval_lattice(h, what);
  NSX_CATCH(h)
}

int nsx_get_lattice(nsx_handle *h, int quantity, int which, double *values) {
  NSX_TRY(h)
  nsx::get_lattice(h, quantity, which, values);
  NSX_CATCH(h)
}

}  // extern "C"
