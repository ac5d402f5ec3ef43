// nsx_diag.hip — flow diagnostics of the state the handle holds (include/nsx.h, section "flow diagnostics").
//
// The reference prints none of these; a deal.II application would get them from VectorTools::integrate_difference calls, each of
// which imports the ghosted vector and loops over the cells on the host.  Everything needed already sits on the device: geo,
// cell_n2, the quadrature tables of the assembly, `solution` and `previous_solution` (reference NavierStokes3D.cpp:555).
//
//   k_cell_diag    one CELL PER LANE as k_cell_convection (nsx_assemble.hip): gathers U_a and Uprev_a once and leaves the eight
//                  per-cell values as SoA planes [NSX_DIAG_COUNT][n_cells] (coalesced stores) -- the "store pass";
//   k_diag_reduce  the "sum pass": folds FOLD_CELLS consecutive entries of every plane per workgroup, launched level by level until
//                  one entry is left.  Which entry a thread takes and the tree it is combined in depend on n_cells alone and the
//                  cells are in the caller's order: no atomics, bitwise reproducible, the same for every internal layout.
// The call reads state only.  Roofline: HBM.  Algorithmic bytes per cell: 4*NP2 ids + 8*(DIM^2+1) geometry + 2*8*DIM*NP2 gathers +
// 8*NSX_DIAG_COUNT stores.
#include <algorithm>
#include <cmath>

#include "nsx_post.hpp"

namespace nsx {

// the larger of two values where a NaN on either side wins (fmax would drop it: a blown-up run has to show in the maxima)
__host__ __device__ __forceinline__ double nan_max(double a, double b) { return (b > a || b != b) ? b : a; }

// ------------------------------------------------------------------ per-cell values
// Per quadrature point: u_q = sum_a N_a U_a, d_q = sum_a N_a (U_a - Uprev_a), H[i][k] = sum_a U_a,i d_k N_a (reference gradient),
// G = H J^-1 (G[i][j] = d_j u_i) and ut = J^-1 u_q, whose component k-1 is u_q . grad lambda_k (k = 1..DIM; lambda_0 takes minus their sum).
// J^-1 u_q is formed from u_q (DIM^2 multiplications per point) rather than from Ut_a = J^-1 U_a as k_cell_convection does: the kernel
// already keeps U_a and U_a - Uprev_a in registers (4*DIM*NP2 VGPRs) and a third copy would halve the occupancy for nothing.
// The q loop stays rolled (#pragma unroll 1): fully unrolled, hipcc would hoist every table value into SGPRs and spill them into VGPRs
// (the trap k_cell_convection's comment describes).  Every table read depends on q, so a rolled loop leaves nothing to hoist and no
// opaque pointer is needed -- with k_cell_convection's asm barrier on them the table pointers lose their address space and the tables
// come through 80 VGPRs of flat loads instead of scalar loads (3D: 256 VGPRs, 1 wave per SIMD).  a and the components are unrolled,
// so U and D are indexed statically and stay in registers: no scratch (resource usage per instantiation: DESIGN.md section 4).
template <int DIM, int NP2, int NQ>
__global__ __launch_bounds__(64) void k_cell_diag(int n_cells, const uint8_t *__restrict__ counted, const int32_t *__restrict__ cell_n2,
                                                  const double *__restrict__ geo, const double *__restrict__ tN,
                                                  const double *__restrict__ tdN, const double *__restrict__ tw,
                                                  const double *__restrict__ sol, const double *__restrict__ prev, double deltat,
                                                  double *__restrict__ planes) {
  const int cell = blockIdx.x * 64 + threadIdx.x;
  if (cell >= n_cells) return;
  double *out = planes + cell;
  if (!counted[cell]) {  // a neighbour rank counts this cell
#pragma unroll
    for (int p = 0; p < NSX_DIAG_COUNT; ++p) out[(size_t)p * n_cells] = 0.0;
    return;
  }
  double Ji[DIM][DIM];
#pragma unroll
  for (int k = 0; k < DIM; ++k)
#pragma unroll
    for (int d = 0; d < DIM; ++d) Ji[k][d] = geo[(size_t)(k * DIM + d) * n_cells + cell];
  const double adet = geo[(size_t)(DIM * DIM) * n_cells + cell];
  double U[NP2][DIM], D[NP2][DIM];
#pragma unroll
  for (int a = 0; a < NP2; ++a) {
    const int node = cell_n2[(size_t)a * n_cells + cell];
#pragma unroll
    for (int c = 0; c < DIM; ++c) {
      U[a][c] = sol[(size_t)node * DIM + c];
      D[a][c] = U[a][c] - prev[(size_t)node * DIM + c];
    }
  }
  double e2 = 0.0, div2 = 0.0, grad2 = 0.0, curl2 = 0.0, chg2 = 0.0, vol = 0.0, cfl = 0.0, speed2 = 0.0;
#pragma unroll 1
  for (int q = 0; q < NQ; ++q) {
    const double *pN = tN + q * NP2, *pdN = tdN + q * NP2 * DIM;
    const double jxw = adet * tw[q];
    double u[DIM], d[DIM], H[DIM][DIM];
#pragma unroll
    for (int i = 0; i < DIM; ++i) {
      u[i] = 0.0;
      d[i] = 0.0;
#pragma unroll
      for (int k = 0; k < DIM; ++k) H[i][k] = 0.0;
    }
#pragma unroll
    for (int a = 0; a < NP2; ++a) {
      const double n = pN[a];
#pragma unroll
      for (int i = 0; i < DIM; ++i) {
        u[i] += n * U[a][i];
        d[i] += n * D[a][i];
#pragma unroll
        for (int k = 0; k < DIM; ++k) H[i][k] += U[a][i] * pdN[a * DIM + k];
      }
    }
    double G[DIM][DIM];
#pragma unroll
    for (int i = 0; i < DIM; ++i)
#pragma unroll
      for (int j = 0; j < DIM; ++j) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < DIM; ++k) s += H[i][k] * Ji[k][j];
        G[i][j] = s;
      }
    double uu = 0.0, dd = 0.0, div = 0.0, gg = 0.0, ut0 = 0.0;
#pragma unroll
    for (int i = 0; i < DIM; ++i) {
      uu += u[i] * u[i];
      dd += d[i] * d[i];
      div += G[i][i];
#pragma unroll
      for (int j = 0; j < DIM; ++j) gg += G[i][j] * G[i][j];
    }
#pragma unroll
    for (int k = 0; k < DIM; ++k) {
      double s = 0.0;
#pragma unroll
      for (int i = 0; i < DIM; ++i) s += Ji[k][i] * u[i];
      ut0 -= s;
      cfl = nan_max(cfl, fabs(s));
    }
    cfl = nan_max(cfl, fabs(ut0));
    double ww;
    if (DIM == 2) {
      const double w = G[1][0] - G[0][1];
      ww = w * w;
    } else {
      const double w0 = G[DIM - 1][1] - G[1][DIM - 1], w1 = G[0][DIM - 1] - G[DIM - 1][0], w2 = G[1][0] - G[0][1];
      ww = w0 * w0 + w1 * w1 + w2 * w2;
    }
    e2 += uu * jxw;
    div2 += div * div * jxw;
    grad2 += gg * jxw;
    curl2 += ww * jxw;
    chg2 += dd * jxw;
    vol += jxw;
    speed2 = nan_max(speed2, uu);
  }
  out[(size_t)NSX_DIAG_ENERGY * n_cells] = 0.5 * e2;
  out[(size_t)NSX_DIAG_DIV2 * n_cells] = div2;
  out[(size_t)NSX_DIAG_GRAD2 * n_cells] = grad2;
  out[(size_t)NSX_DIAG_ENSTROPHY * n_cells] = 0.5 * curl2;
  out[(size_t)NSX_DIAG_CHANGE2 * n_cells] = chg2;
  out[(size_t)NSX_DIAG_VOLUME * n_cells] = vol;
  out[(size_t)NSX_DIAG_CFL * n_cells] = deltat * cfl;
  out[(size_t)NSX_DIAG_SPEED * n_cells] = sqrt(speed2);
}

// ------------------------------------------------------------------ deterministic fold
// Workgroup b folds entries [b * FOLD_CELLS, (b + 1) * FOLD_CELLS) of every plane of in[.][stride_in] into entry b of out[.][gridDim.x]:
// thread t takes entries t, t + 256, ... in that order, then the fixed tree of block_fold.  Planes NSX_DIAG_CFL and NSX_DIAG_SPEED are
// folded with nan_max, the others by addition; plane NSX_DIAG_COUNT of `out` counts the values that are not finite (FIRST: found in
// the eight planes of k_cell_diag; later levels add the counts up).
constexpr int FOLD_CELLS = 2048;
constexpr int FOLD_PLANES = NSX_DIAG_COUNT + 1;

template <bool MAX>
__device__ __forceinline__ double block_fold(double v, double *sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double w = __shfl_down(v, o, 64);
    v = MAX ? nan_max(v, w) : v + w;
  }
  __syncthreads();  // sh is reused plane after plane
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = sh[0];
  for (int k = 1; k < 4; ++k) t = MAX ? nan_max(t, sh[k]) : t + sh[k];
  return t;  // the same value in every thread
}

template <bool FIRST>
__global__ __launch_bounds__(256) void k_diag_reduce(int n, int stride_in, const double *__restrict__ in, double *__restrict__ out) {
  __shared__ double sh[4];
  const int i0 = blockIdx.x * FOLD_CELLS + threadIdx.x, i1 = (int)min((int64_t)n, ((int64_t)blockIdx.x + 1) * FOLD_CELLS);
  double bad = 0.0;
  for (int p = 0; p < (FIRST ? NSX_DIAG_COUNT : FOLD_PLANES); ++p) {
    const bool is_max = p == NSX_DIAG_CFL || p == NSX_DIAG_SPEED;
    const double *src = in + (size_t)p * stride_in;
    double acc = 0.0;  // every value is >= 0 (or not finite)
    for (int i = i0; i < i1; i += 256) {
      const double v = src[i];
      if (FIRST && !isfinite(v)) bad += 1.0;
      acc = is_max ? nan_max(acc, v) : acc + v;
    }
    if (!FIRST && p == NSX_DIAG_COUNT) {
      bad = acc;
      break;
    }
    const double t = is_max ? block_fold<true>(acc, sh) : block_fold<false>(acc, sh);
    if (threadIdx.x == 0) out[(size_t)p * gridDim.x + blockIdx.x] = t;
  }
  const double t = block_fold<false>(bad, sh);
  if (threadIdx.x == 0) out[(size_t)NSX_DIAG_COUNT * gridDim.x + blockIdx.x] = t;
}

// ------------------------------------------------------------------ host drivers
template <int DIM, int NP2, int NQ>
static void launch_diag(nsx_handle *h) {
  const double bytes = (double)h->diag.n_counted * (4.0 * NP2 + 8.0 * (DIM * DIM + 1) + 2.0 * 8.0 * DIM * NP2) + 8.0 * NSX_DIAG_COUNT * h->n_cells;
  LaunchScope ls(h, "diag_cells", bytes);
  hipLaunchKernelGGL((k_cell_diag<DIM, NP2, NQ>), dim3(cdiv(h->n_cells, 64)), dim3(64), 0, h->stream, h->n_cells, h->diag.counted.p,
                     h->cell_n2.p, h->geo.p, h->tab_N2.p, h->tab_dN2.p, h->tab_w.p, h->sol.p, h->prev_sol.p, h->prm.deltat, h->diag.planes.p);
}

// the instantiation set of k_cell_convection (dispatch_conv, nsx_assemble.hip); false: none for this (dim, n_p2, n_q)
static bool dispatch_diag(nsx_handle *h, bool launch) {
#define NSX_DIAG_CASE(D_, P_, Q_) \
  case Q_:                        \
    if (launch) launch_diag<D_, P_, Q_>(h); \
    return true;
  if (h->dim == 2 && h->np2 == 6) {
    switch (h->n_q) {
      NSX_DIAG_CASE(2, 6, 3)
      NSX_DIAG_CASE(2, 6, 4)
      NSX_DIAG_CASE(2, 6, 6)
      NSX_DIAG_CASE(2, 6, 7)
      NSX_DIAG_CASE(2, 6, 12)
    }
  } else if (h->dim == 3 && h->np2 == 10) {
    switch (h->n_q) {
      NSX_DIAG_CASE(3, 10, 4)
      NSX_DIAG_CASE(3, 10, 10)
      NSX_DIAG_CASE(3, 10, 11)
      NSX_DIAG_CASE(3, 10, 14)
      NSX_DIAG_CASE(3, 10, 15)
      NSX_DIAG_CASE(3, 10, 24)
    }
  }
#undef NSX_DIAG_CASE
  return false;
}

// Which cells this handle counts: all of them on a one-process handle; in a distributed run neighbours share the cells along their
// border, and the rank that owns the cell's lowest GLOBAL P2 node counts it (that rank holds the cell among its layer-1 cells, and
// every rank can decide it from its own tables).  cell_n2_in holds caller-local ids: owned nodes first, then the ghosts in the
// order of ghost_u.  Called at the end of every mesh set-up.
void diag_mesh_setup(nsx_handle *h) {
  const int np2 = h->np2, n_cells = h->n_cells;
  std::vector<uint8_t> counted((size_t)n_cells, 1);
  h->diag.n_counted = n_cells;
  if (h->dist) {
    h->diag.n_counted = 0;
    for (int c = 0; c < n_cells; ++c) {
      int32_t lowest = INT32_MAX;
      for (int a = 0; a < np2; ++a) {
        const int32_t l = h->cell_n2_in[(size_t)c * np2 + a];
        lowest = std::min(lowest, l < h->N2 ? h->goff_u + l : h->ghost_u[l - h->N2]);
      }
      counted[c] = lowest >= h->goff_u && lowest < h->goff_u + h->N2;
      h->diag.n_counted += counted[c];
    }
  }
  h->diag.counted.upload(counted, h->stream);
  h->diag.valid = false;
}

static void fold_planes(nsx_handle *h, double totals[FOLD_PLANES]) {
  // level sizes n_cells -> cdiv(., FOLD_CELLS) -> ... -> 1, one region of diag_fold per level
  std::vector<int> sizes;
  size_t total = 0;
  for (int n = h->n_cells; sizes.empty() || sizes.back() > 1; n = sizes.back()) {
    sizes.push_back(cdiv(n, FOLD_CELLS));
    total += (size_t)FOLD_PLANES * sizes.back();
  }
  h->diag.fold.alloc(total);
  LaunchScope ls(h, "diag_reduce", 8.0 * NSX_DIAG_COUNT * h->n_cells);
  const double *in = h->diag.planes.p;
  double *out = h->diag.fold.p;
  int n = h->n_cells;
  for (size_t l = 0; l < sizes.size(); ++l) {
    if (l == 0)
      hipLaunchKernelGGL((k_diag_reduce<true>), dim3(sizes[l]), dim3(256), 0, h->stream, n, n, in, out);
    else
      hipLaunchKernelGGL((k_diag_reduce<false>), dim3(sizes[l]), dim3(256), 0, h->stream, n, n, in, out);
    in = out;
    n = sizes[l];
    out += (size_t)FOLD_PLANES * n;
  }
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpyAsync(totals, in, FOLD_PLANES * sizeof(double), hipMemcpyDeviceToHost, h->stream));
}

// returns the number of per-cell values (of all ranks) that are not finite
static double run_diagnostics(nsx_handle *h, nsx_flow_diag *out) {
  post_check_space(h, "nsx_compute_diagnostics");
  if (!dispatch_diag(h, false))
    NSX_THROW(NSX_ERR_UNSUPPORTED, "no diagnostics kernel instantiated for dim=%d n_p2=%d n_q=%d (see dispatch_diag in nsx_diag.hip)", h->dim, h->np2, h->n_q);
  HIP_CHECK(hipSetDevice(h->prm.device));
  h->diag.planes.alloc((size_t)NSX_DIAG_COUNT * h->n_cells);
  h->diag.valid = false;
  dispatch_diag(h, true);
  double t[FOLD_PLANES];
  fold_planes(h, t);
  HIP_CHECK(hipStreamSynchronize(h->stream));
  h->diag.valid = true;
  // [0..4] the five sums, [5] volume, [6] cells counted, [7] values that are not finite
  double s[8] = {t[NSX_DIAG_ENERGY], t[NSX_DIAG_DIV2], t[NSX_DIAG_GRAD2], t[NSX_DIAG_ENSTROPHY], t[NSX_DIAG_CHANGE2], t[NSX_DIAG_VOLUME],
                 (double)h->diag.n_counted, t[NSX_DIAG_COUNT]};
  double cfl = t[NSX_DIAG_CFL], speed = t[NSX_DIAG_SPEED];
  if (h->comm) {
    // every rank issues the same two collectives, whatever it found: an error is reported behind them, never instead of them
    // the slots of S_POST are per-solve scratch of the Krylov drivers (written before they are read in every solve, nothing is carried
    // from one call to the next), as nsx_compute_forces uses the first two
    static_assert(sizeof(s) / sizeof(s[0]) == S_POST_LEN, "the slot table has the length");
    for (int i = 0; i < S_POST_LEN; ++i) {
      h->scal_host[S_POST + i] = s[i];
      h->slot_nb[S_POST + i] = 0;
    }
    HIP_CHECK(hipMemcpyAsync(h->scal.p + S_POST, h->scal_host + S_POST, S_POST_LEN * sizeof(double), hipMemcpyHostToDevice, h->stream));
    comm_allreduce_scalars(h, S_POST, S_POST_LEN);
    read_scalars(h, S_POST, S_POST_LEN, s);
    // the maxima through the same SUM collective: every rank fills its own slot of a zeroed vector (x + 0 is exact, NaN and inf survive)
    const int w = h->world;
    std::vector<double> m((size_t)2 * w, 0.0);
    m[h->rank] = cfl;
    m[w + h->rank] = speed;
    h->diag.max.alloc(m.size());
    HIP_CHECK(hipMemcpyAsync(h->diag.max.p, m.data(), m.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_CHECK(hipStreamSynchronize(h->stream));
    comm_allreduce_partials(h, h->diag.max.p, 2 * w);
    h->diag.max.download(m.data(), m.size(), h->stream);
    cfl = speed = 0.0;
    for (int r = 0; r < w; ++r) {
      cfl = nan_max(cfl, m[r]);
      speed = nan_max(speed, m[w + r]);
    }
  }
  out->kinetic_energy = s[0];
  out->div_l2 = std::sqrt(s[1]);
  out->grad_l2_sq = s[2];
  out->enstrophy = s[3];
  out->change_l2 = std::sqrt(s[4]);
  out->volume = s[5];
  out->cfl_max = cfl;
  out->speed_max = speed;
  out->n_cells = (int64_t)s[6];
  return s[7];
}

}  // namespace nsx

extern "C" {

int nsx_compute_diagnostics(nsx_handle *h, nsx_flow_diag *out) {
  NSX_TRY(h)
  if (!out) NSX_THROW(NSX_ERR_ARG, "null output");
  const double bad = nsx::run_diagnostics(h, out);
  if (!(bad == 0.0)) NSX_THROW(NSX_ERR_NUMERIC, "flow diagnostics: %.0f per-cell values are not finite (speed_max = %g)", bad, out->speed_max);
  NSX_CATCH(h)
}

int nsx_get_cell_diagnostic(nsx_handle *h, int which, double *values) {
  NSX_TRY(h)
  if (!values || which < 0 || which >= NSX_DIAG_COUNT) NSX_THROW(NSX_ERR_ARG, "bad diagnostic %d / null output", which);
  if (!h->have_mesh || !h->diag.valid) NSX_THROW(NSX_ERR_ARG, "nsx_compute_diagnostics first");
  HIP_CHECK(hipSetDevice(h->prm.device));
  HIP_CHECK(hipMemcpyAsync(values, h->diag.planes.p + (size_t)which * h->n_cells, (size_t)h->n_cells * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIP_CHECK(hipStreamSynchronize(h->stream));
  NSX_CATCH(h)
}

}  // extern "C"
