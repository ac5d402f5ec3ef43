// nsx_stats.hip — running statistics: weighted mean and co-moments of velocity and pressure over the time steps, per phase bin, at every node
// this handle owns; include/nsx.h, section "running statistics" (the recurrence there is a contract).  No counterpart in the reference.
//
//   k_stats_update  ONE launch per sample for velocity and pressure together: the leading workgroups take the P2 nodes, the rest the P1 nodes
//                   (a workgroup-uniform branch).  A pure stream: a lane takes TWO neighbouring nodes of the caller's numbering, so every
//                   accumulator plane is read and written as 16 bytes per lane, coalesced; the planes' stride is a multiple of 64 entries,
//                   so the pair of the last node of an odd count stays inside its plane (its second half accumulates x = 0 and stays 0).  The
//                   state is read where the node lives inside libnsx: through perm2_d / perm1_d with a layout in force (a gather of dim
//                   consecutive doubles per node), directly -- 16 bytes per lane again for the velocity -- without one.
//                   Algorithmic bytes per launch: per P2 node 8 dim (state) + 16 (dim + dim (dim + 1) / 2) (planes in and out), 3D: 24 + 144;
//                   per P1 node 8 + 32; 4 per node for the permutation when a layout is in force.
//                   Cache policy: plain loads and stores.  A plane written by one call is next read one time step later, behind a solve that
//                   streams gigabytes, so nothing written here can still be in the 256-MiB Infinity Cache then; and non-temporal stores leave
//                   the line in the L2 exactly as plain ones do and move the same bytes out of it, so they have nothing to save either.
//   k_stats_finish  one node per lane: folds the bins a get names (one bin, or all non-empty ones in ascending order: the pairwise merge of
//                   the header) in registers, derives the quantity and writes [n_nodes][n_components].  The accumulators are only read.
//
// Both kernels are elementwise in the caller's numbering and every operation is an IEEE operation rounded on its own (no contraction, below):
// the results depend on the samples and their order alone, not on the scheduling, the rank tables, the layout or the partition into processes.
#include <cmath>

#include "nsx_post.hpp"

#pragma clang fp contract(off)

namespace nsx {

constexpr int STATS_WG = 256;       // lanes per workgroup of both kernels
constexpr int STATS_MAX_BINS = 64;
constexpr int STATS_ALL = NSX_STATS_VELOCITY | NSX_STATS_PRESSURE;
__host__ __device__ constexpr int stats_nsym(int nc) { return nc * (nc + 1) / 2; }
// plane of the pair (i, j), i <= j, among the co-moment planes: xx, yy, [zz,] xy[, xz, yz]
__host__ __device__ constexpr int stats_sym(int nc, int i, int j) { return i == j ? i : nc + i + j - 1; }

// The recurrence for the nodes n0, n0 + 1 (n0 even) of one space: planes [NC + NSYM][stride] of the bin, x[k][c] the sample at node n0 + k.
template <int NC>
__device__ __forceinline__ void stats_fold_pair(double *__restrict__ planes, size_t stride, size_t n0, const double (&x)[2][NC], double r, double q) {
  constexpr int NSYM = stats_nsym(NC);
  double2 *p = reinterpret_cast<double2 *>(planes + n0);  // stride and n0 are even: 16-byte aligned in every plane
  const size_t s2 = stride / 2;
  double2 m[NC], C[NSYM];
#pragma unroll
  for (int c = 0; c < NC; ++c) m[c] = p[(size_t)c * s2];
#pragma unroll
  for (int k = 0; k < NSYM; ++k) C[k] = p[(size_t)(NC + k) * s2];
  double d[2][NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    d[0][c] = x[0][c] - m[c].x;
    d[1][c] = x[1][c] - m[c].y;
    m[c].x = m[c].x + r * d[0][c];
    m[c].y = m[c].y + r * d[1][c];
  }
#pragma unroll
  for (int i = 0; i < NC; ++i)
#pragma unroll
    for (int j = i; j < NC; ++j) {
      const int k = stats_sym(NC, i, j);
      C[k].x = C[k].x + (q * d[0][i]) * d[0][j];
      C[k].y = C[k].y + (q * d[1][i]) * d[1][j];
    }
#pragma unroll
  for (int c = 0; c < NC; ++c) p[(size_t)c * s2] = m[c];
#pragma unroll
  for (int k = 0; k < NSYM; ++k) p[(size_t)(NC + k) * s2] = C[k];
}

// nb2 workgroups for the N2 owned P2 nodes (0: velocity is not accumulated), the others for the NP owned P1 nodes.  vel / pres: the bin's
// planes.  sol: the ghosted block vector, velocity of internal node n at sol[n DIM + c], pressure at sol[off_p + n]; PERM: caller-local owned
// node -> internal node through perm2 / perm1 (both map owned nodes to owned nodes).
template <int DIM, bool PERM>
__global__ __launch_bounds__(STATS_WG) void k_stats_update(int N2, int NP, int nb2, const int32_t *__restrict__ perm2, const int32_t *__restrict__ perm1,
                                                           const double *__restrict__ sol, int off_p, double *__restrict__ vel, size_t stride2,
                                                           double *__restrict__ pres, size_t stride1, double r, double q) {
  if ((int)blockIdx.x < nb2) {
    const size_t n0 = 2 * ((size_t)blockIdx.x * STATS_WG + threadIdx.x);
    if (n0 >= (size_t)N2) return;
    double x[2][DIM];
    if (!PERM && n0 + 1 < (size_t)N2) {  // 2 DIM consecutive doubles from a 16-byte boundary (n0 is even)
      const double2 *s = reinterpret_cast<const double2 *>(sol + n0 * DIM);
      double f[2 * DIM];
#pragma unroll
      for (int c = 0; c < DIM; ++c) {
        const double2 v = s[c];
        f[2 * c] = v.x;
        f[2 * c + 1] = v.y;
      }
#pragma unroll
      for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int c = 0; c < DIM; ++c) x[k][c] = f[k * DIM + c];
    } else {
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const bool have = n0 + k < (size_t)N2;
        const size_t src = !have ? 0 : PERM ? (size_t)perm2[n0 + k] : n0 + k;
#pragma unroll
        for (int c = 0; c < DIM; ++c) x[k][c] = have ? sol[src * DIM + c] : 0.0;
      }
    }
    stats_fold_pair<DIM>(vel, stride2, n0, x, r, q);
  } else {
    const size_t n0 = 2 * ((size_t)(blockIdx.x - nb2) * STATS_WG + threadIdx.x);
    if (n0 >= (size_t)NP) return;
    double x[2][1];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const bool have = n0 + k < (size_t)NP;
      const size_t src = !have ? 0 : PERM ? (size_t)perm1[n0 + k] : n0 + k;
      x[k][0] = have ? sol[(size_t)off_p + src] : 0.0;
    }
    stats_fold_pair<1>(pres, stride1, n0, x, r, q);
  }
}

// what a get folds: the planes of bin[0], then the merges with bin[1 .. n) (coefficients s, t of the header; entry 0 unused), and 1 / W of the result
struct StatsFold {
  int n;
  int bin[STATS_MAX_BINS];
  double s[STATS_MAX_BINS], t[STATS_MAX_BINS];
  double invW;
};
enum { STATS_K_MEAN = 0, STATS_K_COMOMENT, STATS_K_STRESS, STATS_K_RMS, STATS_K_TKE };

// planes [n_bins][NC + NSYM][stride]; out [n_nodes][components of the kind]
template <int NC>
__global__ __launch_bounds__(STATS_WG) void k_stats_finish(int n_nodes, const double *__restrict__ planes, size_t stride, StatsFold f, int kind,
                                                           double *__restrict__ out) {
  constexpr int NSYM = stats_nsym(NC);
  const size_t node = (size_t)blockIdx.x * STATS_WG + threadIdx.x;
  if (node >= (size_t)n_nodes) return;
  const size_t bin_stride = (size_t)(NC + NSYM) * stride;
  double m[NC], C[NSYM];
  {
    const double *a = planes + (size_t)f.bin[0] * bin_stride + node;
#pragma unroll
    for (int c = 0; c < NC; ++c) m[c] = a[(size_t)c * stride];
#pragma unroll
    for (int k = 0; k < NSYM; ++k) C[k] = a[(size_t)(NC + k) * stride];
  }
  for (int b = 1; b < f.n; ++b) {
    const double *pb = planes + (size_t)f.bin[b] * bin_stride + node;
    const double s = f.s[b], t = f.t[b];
    double del[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) del[c] = pb[(size_t)c * stride] - m[c];
#pragma unroll
    for (int i = 0; i < NC; ++i)
#pragma unroll
      for (int j = i; j < NC; ++j) {
        const int k = stats_sym(NC, i, j);
        C[k] = (C[k] + pb[(size_t)(NC + k) * stride]) + (t * del[i]) * del[j];
      }
#pragma unroll
    for (int c = 0; c < NC; ++c) m[c] = m[c] + s * del[c];
  }
  switch (kind) {
    case STATS_K_MEAN:
#pragma unroll
      for (int c = 0; c < NC; ++c) out[node * NC + c] = m[c];
      break;
    case STATS_K_COMOMENT:
#pragma unroll
      for (int k = 0; k < NSYM; ++k) out[node * NSYM + k] = C[k];
      break;
    case STATS_K_STRESS:
#pragma unroll
      for (int k = 0; k < NSYM; ++k) out[node * NSYM + k] = C[k] * f.invW;
      break;
    case STATS_K_RMS:
#pragma unroll
      for (int c = 0; c < NC; ++c) out[node * NC + c] = sqrt(C[c] * f.invW);
      break;
    default: {  // STATS_K_TKE
      double e = C[0] * f.invW;
#pragma unroll
      for (int c = 1; c < NC; ++c) e = e + C[c] * f.invW;
      out[node] = 0.5 * e;
    }
  }
}

// ------------------------------------------------------------------ host drivers
// a quantity of nsx_stats_get: which part it belongs to, what the finish kernel derives, components per node
struct StatsQuantity {
  int part, kind, nc;
};
static StatsQuantity stats_quantity(int dim, int quantity, const char *who) {
  switch (quantity) {
    case NSX_STATS_MEAN_U: return {NSX_STATS_VELOCITY, STATS_K_MEAN, dim};
    case NSX_STATS_COMOMENT_U: return {NSX_STATS_VELOCITY, STATS_K_COMOMENT, stats_nsym(dim)};
    case NSX_STATS_STRESS_U: return {NSX_STATS_VELOCITY, STATS_K_STRESS, stats_nsym(dim)};
    case NSX_STATS_RMS_U: return {NSX_STATS_VELOCITY, STATS_K_RMS, dim};
    case NSX_STATS_TKE: return {NSX_STATS_VELOCITY, STATS_K_TKE, 1};
    case NSX_STATS_MEAN_P: return {NSX_STATS_PRESSURE, STATS_K_MEAN, 1};
    case NSX_STATS_COMOMENT_P: return {NSX_STATS_PRESSURE, STATS_K_COMOMENT, 1};
    case NSX_STATS_VAR_P: return {NSX_STATS_PRESSURE, STATS_K_STRESS, 1};
    case NSX_STATS_RMS_P: return {NSX_STATS_PRESSURE, STATS_K_RMS, 1};
    default: NSX_THROW(NSX_ERR_ARG, "%s: quantity %d (NSX_STATS_MEAN_U ... NSX_STATS_RMS_P)", who, quantity);
  }
}

static void stats_need(nsx_handle *h, const char *who) {
  post_check_space(h, who);
  if (h->stats.n_bins == 0) NSX_THROW(NSX_ERR_ARG, "%s: nsx_stats_begin first", who);
}

static void stats_begin(nsx_handle *h, int what, int n_bins) {
  post_check_space(h, "nsx_stats_begin");
  if ((what & ~STATS_ALL) != 0) NSX_THROW(NSX_ERR_ARG, "nsx_stats_begin: what = %d: an OR of NSX_STATS_VELOCITY and NSX_STATS_PRESSURE", what);
  if (what == 0 && n_bins == 0) {  // closes the accumulation
    h->stats.clear();
    return;
  }
  if (what == 0 || n_bins == 0) NSX_THROW(NSX_ERR_ARG, "nsx_stats_begin: what = %d, n_bins = %d: both zero (closes the accumulation) or neither", what, n_bins);
  if (n_bins < 1 || n_bins > STATS_MAX_BINS) NSX_THROW(NSX_ERR_ARG, "nsx_stats_begin: n_bins = %d: 1 .. %d", n_bins, STATS_MAX_BINS);
  HIP_CHECK(hipSetDevice(h->prm.device));
  const int dim = h->dim;
  const size_t stride2 = ((size_t)h->N2 + 63) / 64 * 64, stride1 = ((size_t)h->NP + 63) / 64 * 64;
  DevBuf<double> vel, pres;  // the earlier accumulation stays until both are there
  if (what & NSX_STATS_VELOCITY) {
    vel.alloc((size_t)n_bins * (dim + stats_nsym(dim)) * stride2);
    vel.zero(h->stream);
  }
  if (what & NSX_STATS_PRESSURE) {
    pres.alloc((size_t)n_bins * 2 * stride1);
    pres.zero(h->stream);
  }
  StatsState &s = h->stats;
  s.clear();
  std::swap(s.vel.p, vel.p);
  std::swap(s.vel.n, vel.n);
  std::swap(s.pres.p, pres.p);
  std::swap(s.pres.n, pres.n);
  s.what = what;
  s.n_bins = n_bins;
  s.stride2 = stride2;
  s.stride1 = stride1;
  s.W.assign((size_t)n_bins, 0.0);
  s.samples.assign((size_t)n_bins, 0);
}

template <int DIM, bool PERM>
static void launch_stats_update(nsx_handle *h, int bin, double r, double q) {
  StatsState &s = h->stats;
  constexpr int NPL = DIM + stats_nsym(DIM);
  const int N2 = (s.what & NSX_STATS_VELOCITY) ? h->N2 : 0, NP = (s.what & NSX_STATS_PRESSURE) ? h->NP : 0;
  const int nb2 = cdiv(cdiv(N2, 2), STATS_WG), nb1 = cdiv(cdiv(NP, 2), STATS_WG);
  if (nb2 + nb1 == 0) return;
  const double bytes = (double)N2 * (8.0 * DIM + 16.0 * NPL + (PERM ? 4.0 : 0.0)) + (double)NP * (8.0 + 32.0 + (PERM ? 4.0 : 0.0));
  LaunchScope ls(h, "stats_update", bytes);
  hipLaunchKernelGGL((k_stats_update<DIM, PERM>), dim3(nb2 + nb1), dim3(STATS_WG), 0, h->stream, N2, NP, nb2, h->perm2_d.p, h->perm1_d.p, h->sol.p, h->off_p,
                     s.vel.p + (size_t)bin * NPL * s.stride2, s.stride2, s.pres.p + (size_t)bin * 2 * s.stride1, s.stride1, r, q);
}

static void stats_accumulate(nsx_handle *h, int bin, double weight) {
  stats_need(h, "nsx_stats_accumulate");
  StatsState &s = h->stats;
  if (bin < 0 || bin >= s.n_bins) NSX_THROW(NSX_ERR_ARG, "nsx_stats_accumulate: bin %d of %d", bin, s.n_bins);
  if (!std::isfinite(weight) || !(weight > 0.0)) NSX_THROW(NSX_ERR_ARG, "nsx_stats_accumulate: weight = %g: a finite value above 0", weight);
  if (!h->sol.p || h->sol.n < (size_t)h->len_blk) NSX_THROW(NSX_ERR_ARG, "nsx_stats_accumulate: the handle holds no state yet");
  HIP_CHECK(hipSetDevice(h->prm.device));
  // the three coefficients of the contract, one rounded operation each (volatile: no reassociation, no excess precision)
  const volatile double W = s.W[(size_t)bin], W1 = W + weight, r = weight / W1, q = W * r;
  if (h->dim == 2) h->layout_on ? launch_stats_update<2, true>(h, bin, r, q) : launch_stats_update<2, false>(h, bin, r, q);
  else h->layout_on ? launch_stats_update<3, true>(h, bin, r, q) : launch_stats_update<3, false>(h, bin, r, q);
  HIP_CHECK(hipGetLastError());
  s.W[(size_t)bin] = W1;
  s.samples[(size_t)bin]++;
}

template <int NC>
static void launch_stats_finish(nsx_handle *h, int n_nodes, const double *planes, size_t stride, const StatsFold &f, const StatsQuantity &qy) {
  StatsState &s = h->stats;
  s.out.alloc((size_t)n_nodes * qy.nc);
  if (n_nodes == 0) return;
  LaunchScope ls(h, "stats_finish", 8.0 * n_nodes * ((double)f.n * (NC + stats_nsym(NC)) + qy.nc));
  hipLaunchKernelGGL((k_stats_finish<NC>), dim3(cdiv(n_nodes, STATS_WG)), dim3(STATS_WG), 0, h->stream, n_nodes, planes, stride, f, qy.kind, s.out.p);
}

static void stats_get(nsx_handle *h, int quantity, int bin, double *values) {
  stats_need(h, "nsx_stats_get");
  StatsState &s = h->stats;
  const StatsQuantity qy = stats_quantity(h->dim, quantity, "nsx_stats_get");
  if (!(s.what & qy.part)) NSX_THROW(NSX_ERR_ARG, "nsx_stats_get: quantity %d: the open accumulation holds no %s", quantity, qy.part == NSX_STATS_VELOCITY ? "velocity" : "pressure");
  if (bin < -1 || bin >= s.n_bins) NSX_THROW(NSX_ERR_ARG, "nsx_stats_get: bin %d of %d (-1: pooled)", bin, s.n_bins);
  if (!values) NSX_THROW(NSX_ERR_ARG, "nsx_stats_get: null values");
  StatsFold f{};
  volatile double W = 0.0;
  if (bin >= 0) {
    if (s.samples[(size_t)bin] == 0) NSX_THROW(NSX_ERR_ARG, "nsx_stats_get: bin %d is empty", bin);
    f.bin[f.n++] = bin;
    W = s.W[(size_t)bin];
  } else {
    for (int b = 0; b < s.n_bins; ++b) {
      if (s.samples[(size_t)b] == 0) continue;
      if (f.n > 0) {  // W = W_a + W_b, s = W_b / W, t = W_a s: one rounded operation each
        const volatile double Wa = W, Wb = s.W[(size_t)b], Wn = Wa + Wb, sc = Wb / Wn, tc = Wa * sc;
        f.s[f.n] = sc;
        f.t[f.n] = tc;
        W = Wn;
      } else {
        W = s.W[(size_t)b];
      }
      f.bin[f.n++] = b;
    }
    if (f.n == 0) NSX_THROW(NSX_ERR_ARG, "nsx_stats_get: every bin is empty");
  }
  f.invW = 1.0 / W;
  HIP_CHECK(hipSetDevice(h->prm.device));
  const bool vel = qy.part == NSX_STATS_VELOCITY;
  const int n_nodes = vel ? h->N2 : h->NP;
  if (!vel) launch_stats_finish<1>(h, n_nodes, s.pres.p, s.stride1, f, qy);
  else if (h->dim == 2) launch_stats_finish<2>(h, n_nodes, s.vel.p, s.stride2, f, qy);
  else launch_stats_finish<3>(h, n_nodes, s.vel.p, s.stride2, f, qy);
  HIP_CHECK(hipGetLastError());
  // caller-local node i = global node goff + i: only the owned entries are written
  double *dst = values + (size_t)(vel ? h->goff_u : h->goff_p) * qy.nc;
  if (n_nodes > 0) HIP_CHECK(hipMemcpyAsync(dst, s.out.p, (size_t)n_nodes * qy.nc * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIP_CHECK(hipStreamSynchronize(h->stream));
}

}  // namespace nsx

extern "C" {

int nsx_stats_begin(nsx_handle *h, int what, int n_bins) {
  NSX_TRY(h)
  nsx::stats_begin(h, what, n_bins);
  NSX_CATCH(h)
}

int nsx_stats_accumulate(nsx_handle *h, int bin, double weight) {
  NSX_TRY(h)
  nsx::stats_accumulate(h, bin, weight);
  NSX_CATCH(h)
}

int nsx_stats_info(nsx_handle *h, int *what, int *n_bins, int64_t *samples, double *weights) {
  NSX_TRY(h)
  nsx::stats_need(h, "nsx_stats_info");
  const nsx::StatsState &s = h->stats;
  if (what) *what = s.what;
  if (n_bins) *n_bins = s.n_bins;
  for (int b = 0; b < s.n_bins; ++b) {
    if (samples) samples[b] = s.samples[(size_t)b];
    if (weights) weights[b] = s.W[(size_t)b];
  }
  NSX_CATCH(h)
}

int nsx_stats_components(nsx_handle *h, int quantity, int *n_components) {
  NSX_TRY(h)
  nsx::post_check_space(h, "nsx_stats_components");
  const nsx::StatsQuantity qy = nsx::stats_quantity(h->dim, quantity, "nsx_stats_components");
  if (!n_components) NSX_THROW(NSX_ERR_ARG, "nsx_stats_components: null n_components");
  *n_components = qy.nc;
  NSX_CATCH(h)
}

int nsx_stats_get(nsx_handle *h, int quantity, int bin, double *values) {
  NSX_TRY(h)
  nsx::stats_get(h, quantity, bin, values);
  NSX_CATCH(h)
}

}  // extern "C"
