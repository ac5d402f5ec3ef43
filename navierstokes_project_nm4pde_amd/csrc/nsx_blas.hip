// nsx_blas.hip — fused BLAS-1 for the Krylov drivers (the Epetra_Vector operations behind deal.II's
// SolverGMRES / SolverCG and the sadd/add/scale calls of reference Preconditioners.hpp:176,195,202-203,281,294-309,386,406,492-515).
//
// Scalars never visit the host inside an orthogonalisation sweep.  A reduction leaves per-block partial sums in
// h->red_partial[slot][0..nb); the CONSUMER kernel (the next add_and_dot / axpy / CG update) sums them itself in a fixed
// order while it starts up, so a dot product costs one launch, not two (a separate 1-block finalise kernel measured
// 4.6 us x 13 000 launches per step, profiles/r01).  Coefficients are SRef = c * value(num) / value(den) evaluated on the
// device.  Everything is deterministic: fixed grids, fixed-order sums, no atomics.
// Multi-GPU: every rank leaves the same number of partial sums, they are all-reduced element-wise over RCCL
// (comm_allreduce_partials) and consumed exactly as on one GPU.
#include "nsx_grid.hpp"
#include "nsx_ilu_lanes.hpp"

namespace nsx {

constexpr int RED_BLOCKS = 512;
constexpr int RED_STRIDE = 1024;  // partial slots reserved per scalar

struct SRef {
  double c;
  int num, den;        // slots, -1 = none
  int num_nb, den_nb;  // number of valid partials (0 = scal[slot] is final)
};

__device__ __forceinline__ double wave_sum_all(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// value of one slot, cooperatively by the block (blockDim.x >= 64); sh: one double of LDS
__device__ __forceinline__ double slot_value(const double *__restrict__ scal, const double *__restrict__ partial, int slot, int nb,
                                             double *sh) {
  if (nb == 0) return scal[slot];
  if (threadIdx.x < 64) {
    // nb <= RED_BLOCKS = 512: eight independent loads per lane, one L2 round trip
    const double *p = partial + (size_t)slot * RED_STRIDE;
    double t[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int i = threadIdx.x + 64 * k;
      t[k] = i < nb ? p[i] : 0.0;
    }
    double a = ((t[0] + t[1]) + (t[2] + t[3])) + ((t[4] + t[5]) + (t[6] + t[7]));
    a = wave_sum_all(a);
    if (threadIdx.x == 0) *sh = a;
  }
  __syncthreads();
  const double v = *sh;
  __syncthreads();
  return v;
}
__device__ __forceinline__ double sval(const double *__restrict__ scal, const double *__restrict__ partial, SRef r, double *sh) {
  double v = r.c;
  if (r.num >= 0) v *= slot_value(scal, partial, r.num, r.num_nb, sh);
  if (r.den >= 0) v /= slot_value(scal, partial, r.den, r.den_nb, sh);
  return v;
}

// d (+)= alpha v ; partial[b] = sum_i d_i * w_i over the block's fixed slice
enum { OP_DOT = 0, OP_ADD_AND_DOT = 1 };
template <int OP>
__global__ __launch_bounds__(256) void k_reduce(int n, int split, int gap, double *__restrict__ d, SRef a, const double *__restrict__ v,
                                                const double *__restrict__ w, const double *__restrict__ scal,
                                                const double *__restrict__ partial_in, double *__restrict__ partial) {
  __shared__ double sh[5];
  constexpr int U = 4;
  const bool self = (w == d);
  const int stride = gridDim.x * 256;
  // first batch of loads is issued BEFORE the coefficient is known: the partial-sum prologue (an L2 round trip, a wave
  // reduction and two barriers) then overlaps with the HBM latency of the stream instead of preceding it
  double dv[U], vv[U], wv[U];
  int idx[U];
#pragma unroll
  for (int k = 0; k < U; ++k) {
    const int i0 = blockIdx.x * 256 + threadIdx.x + k * stride;
    const bool ok = i0 < n;
    const int i = ok ? i0 + (i0 >= split ? gap : 0) : 0;
    idx[k] = ok ? i : -1;
    dv[k] = ok ? d[i] : 0.0;
    vv[k] = (ok && OP == OP_ADD_AND_DOT) ? v[i] : 0.0;
    wv[k] = (ok && !self) ? w[i] : 0.0;
  }
  const double alpha = OP == OP_ADD_AND_DOT ? sval(scal, partial_in, a, sh + 4) : 0.0;
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < U; ++k) {
    double di = dv[k];
    if (OP == OP_ADD_AND_DOT) {
      di += alpha * vv[k];
      if (idx[k] >= 0) d[idx[k]] = di;
    }
    acc += di * (self ? di : wv[k]);
  }
#pragma unroll 4
  for (int i0 = blockIdx.x * 256 + threadIdx.x + U * stride; i0 < n; i0 += stride) {
    const int i = i0 + (i0 >= split ? gap : 0);
    double di = d[i];
    if (OP == OP_ADD_AND_DOT) {
      di += alpha * v[i];
      d[i] = di;
    }
    acc += di * (self ? di : w[i]);
  }
  const double t = block_sum_256(acc, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

struct NbArgs {
  int nb[64];
};
__global__ __launch_bounds__(256) void k_finalize(int slot0, NbArgs nbs, const double *__restrict__ partial, double *__restrict__ scal) {
  __shared__ double sh;
  const int slot = slot0 + blockIdx.x;
  const int nb = nbs.nb[blockIdx.x];
  if (nb == 0) return;
  const double v = slot_value(scal, partial, slot, nb, &sh);
  if (threadIdx.x == 0) scal[slot] = v;
}

// finalise a range of slots AND publish them to mapped host memory; the block that finishes last raises the flag
__global__ __launch_bounds__(256) void k_publish(int slot0, int count, NbArgs nbs, const double *__restrict__ partial,
                                                 double *__restrict__ scal, double *pub_vals, unsigned long long *pub_flag,
                                                 unsigned long long seq, unsigned int *counter) {
  __shared__ double sh;
  const int slot = slot0 + blockIdx.x;
  const int nb = nbs.nb[blockIdx.x];
  const double v = slot_value(scal, partial, slot, nb, &sh);
  if (threadIdx.x == 0) {
    if (nb) scal[slot] = v;
    __hip_atomic_store(pub_vals + slot, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __threadfence_system();
    const unsigned int ticket = atomicAdd(counter, 1u);
    if (ticket == (unsigned int)count - 1) {
      *counter = 0;
      __threadfence_system();
      __hip_atomic_store(pub_flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

// Number of per-block partial sums of a reduction over n entries.  With a communicator every rank must use the SAME count
// (the partial sums are all-reduced element by element, see after_reduction), whatever its local size: a fixed grid.
constexpr int DIST_RED_BLOCKS = 256;
int red_blocks(nsx_handle *h, int n) { return h->comm ? DIST_RED_BLOCKS : std::max(1, std::min(RED_BLOCKS, cdiv(n, 1024))); }

static SRef sref(nsx_handle *h, double c, int num, int den) {
  return SRef{c, num, den, num >= 0 ? h->slot_nb[num] : 0, den >= 0 ? h->slot_nb[den] : 0};
}

// make scal[slot0 .. slot0+count) final (one launch for the whole range)
void finalize_slots(nsx_handle *h, int slot0, int count) {
  if (count > 64) NSX_THROW(NSX_ERR_ARG, "internal: finalize_slots range too long");
  bool any = false;
  for (int i = 0; i < count; ++i) any = any || h->slot_nb[slot0 + i] > 0;
  if (!any) return;
  NbArgs args;
  for (int i = 0; i < count; ++i) args.nb[i] = h->slot_nb[slot0 + i];
  hipLaunchKernelGGL(k_finalize, dim3(count), dim3(256), 0, h->stream, slot0, args, h->red_partial.p, h->scal.p);
  for (int i = 0; i < count; ++i) h->slot_nb[slot0 + i] = 0;
}

// Hold back / release the all-reduces of finished reductions (distributed runs).  On release, slots whose partial-sum regions
// are adjacent go out as one collective.
void defer_reductions(nsx_handle *h, bool on) {
  h->defer_red = on;
  if (on || h->pending_red.empty()) return;
  std::sort(h->pending_red.begin(), h->pending_red.end());
  size_t k = 0;
  while (k < h->pending_red.size()) {
    size_t e = k + 1;
    while (e < h->pending_red.size() && h->pending_red[e] == h->pending_red[e - 1] + 1) ++e;
    const int first = h->pending_red[k], count = (int)(e - k);
    comm_allreduce_partials(h, h->red_partial.p + (size_t)first * RED_STRIDE, (count - 1) * RED_STRIDE + DIST_RED_BLOCKS);
    k = e;
  }
  h->pending_red.clear();
}

void after_reduction(nsx_handle *h, int slot, int nb) {
  h->slot_nb[slot] = nb > 1 ? nb : 0;
  if (!h->comm) return;
  if (h->defer_red && nb == DIST_RED_BLOCKS) {
    h->pending_red.push_back(slot);
    return;
  }
  // global sum needed before anybody consumes the value
  if (nb == DIST_RED_BLOCKS) {
    // all-reduce the partial sums themselves (2 KB instead of 8 B costs the same latency) and let the consumer add
    // them up as on one GPU: no finalising launch in front of the collective
    comm_allreduce_partials(h, h->red_partial.p + (size_t)slot * RED_STRIDE, nb);
  } else {
    finalize_slots(h, slot, 1);
    comm_allreduce_scalars(h, slot, 1);
  }
}
double *red_out(nsx_handle *h, int slot, int nb) {
  return nb > 1 ? h->red_partial.p + (size_t)slot * RED_STRIDE : h->scal.p + slot;
}

void v_dot(nsx_handle *h, Span sp, const double *a, const double *b, int slot) {
  const int n = sp.n;
  LaunchScope ls(h, "dot", (a == b ? 8.0 : 16.0) * n);
  const int nb = red_blocks(h, n);
  hipLaunchKernelGGL((k_reduce<OP_DOT>), dim3(nb), dim3(256), 0, h->stream, n, sp.split, sp.gap, const_cast<double *>(a), SRef{0, -1, -1, 0, 0}, nullptr, b,
                     h->scal.p, h->red_partial.p, red_out(h, slot, nb));
  after_reduction(h, slot, nb);
}

void v_add_and_dot(nsx_handle *h, Span sp, double *d, double a, int aslot, const double *v, const double *w, int slot) {
  const int n = sp.n;
  LaunchScope ls(h, "add_and_dot", (w == d ? 24.0 : 32.0) * n);
  const int nb = red_blocks(h, n);
  hipLaunchKernelGGL((k_reduce<OP_ADD_AND_DOT>), dim3(nb), dim3(256), 0, h->stream, n, sp.split, sp.gap, d, sref(h, a, aslot, -1), v, w, h->scal.p,
                     h->red_partial.p, red_out(h, slot, nb));
  after_reduction(h, slot, nb);
}

void wait_published(nsx_handle *h, unsigned long long seq) {
  volatile unsigned long long *flag_host = pub_word_host<unsigned long long>(h, PUB_FLAG);
  unsigned long long spins = 0;
  // sequence numbers only grow: a later publication that has already landed also proves this one did
  while (__atomic_load_n(flag_host, __ATOMIC_ACQUIRE) < seq) {
    if (++spins > 200000000ull) {  // bounded: fall back to a stream synchronisation, which also surfaces launch errors
      HIP_CHECK(hipStreamSynchronize(h->stream));
      if (__atomic_load_n(flag_host, __ATOMIC_ACQUIRE) < seq) NSX_THROW(NSX_ERR_HIP, "scalar publication never arrived");
      break;
    }
  }
}

// ---- element-wise
__global__ __launch_bounds__(256) void k_axpby(int n, int split, int gap, double *__restrict__ d, SRef s, SRef a, const double *__restrict__ v,
                                               const double *__restrict__ scal, const double *__restrict__ partial, int mode) {
  // mode 0: d = s d + a v ; mode 1: d = a v ; mode 2: d = s d
  __shared__ double sh;
  const double sv = mode == 1 ? 0.0 : sval(scal, partial, s, &sh), av = mode == 2 ? 0.0 : sval(scal, partial, a, &sh);
#pragma unroll 4
  for (int i0 = blockIdx.x * 256 + threadIdx.x; i0 < n; i0 += gridDim.x * 256) {
    const int i = i0 + (i0 >= split ? gap : 0);
    if (mode == 0) d[i] = sv * d[i] + av * v[i];
    else if (mode == 1) d[i] = av * v[i];
    else d[i] = sv * d[i];
  }
}
__global__ void k_scale_vec(int n, double *__restrict__ d, const double *__restrict__ f) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) d[i] *= f[i];
}
constexpr int MULTI_MAX = 32;  // vectors of one launch
static_assert(MULTI_MAX >= KRYLOV_N_TMP + 2, "a GMRES cycle's update is one launch");
struct MultiArgs {
  const double *v[MULTI_MAX];
  double c[MULTI_MAX];
  int k;
};
// START: where the sum starts from.  AX_SELF: x itself.  AX_FROM: x0 (x is only written).  AX_ZERO: 0.0 -- what reading a zeroed x gives,
// with the same chain of fused multiply-adds behind it.  y (AX_ZERO only, may alias x): x = -y + s, the caller's sadd(-1, s) applied to
// the double s the plain kernel would have stored.
enum { AX_SELF = 0, AX_FROM = 1, AX_ZERO = 2 };
template <int START>
__device__ __forceinline__ void axpy_multi_entries(int n, int split, int gap, double *x, const double *x0, const double *y, const MultiArgs &m) {
  for (int i0 = blockIdx.x * 256 + threadIdx.x; i0 < n; i0 += gridDim.x * 256) {
    const int i = i0 + (i0 >= split ? gap : 0);
    double s = START == AX_ZERO ? 0.0 : START == AX_FROM ? x0[i] : x[i];
    for (int j = 0; j < m.k; ++j) s += m.c[j] * m.v[j][i];  // same order as the reference's x.add(h(i), tmp_vectors[i]) loop
    x[i] = (START == AX_ZERO && y) ? -y[i] + s : s;
  }
}
__global__ void k_axpy_multi(int n, int split, int gap, double *__restrict__ x, MultiArgs m) {
  axpy_multi_entries<AX_SELF>(n, split, gap, x, nullptr, nullptr, m);
}
__global__ void k_axpy_multi_from(int n, int split, int gap, double *__restrict__ x, const double *__restrict__ x0, MultiArgs m) {
  axpy_multi_entries<AX_FROM>(n, split, gap, x, x0, nullptr, m);
}
__global__ void k_axpy_multi_zero(int n, int split, int gap, double *x, const double *y, MultiArgs m) {
  axpy_multi_entries<AX_ZERO>(n, split, gap, x, nullptr, y, m);
}
// CG update (SolverCG): x += alpha d ; g += alpha h ; partial(g.g), alpha = value(gh) / value(dh)
__global__ __launch_bounds__(256) void k_cg_update(int n, double *__restrict__ x, const double *__restrict__ dvec, double *__restrict__ g,
                                                   const double *__restrict__ hvec, SRef a, const double *__restrict__ scal,
                                                   const double *__restrict__ partial_in, double *__restrict__ partial) {
  __shared__ double sh[5];
  const double alpha = sval(scal, partial_in, a, sh + 4);
  double acc = 0.0;
#pragma unroll 2
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    x[i] += alpha * dvec[i];
    const double gi = g[i] + alpha * hvec[i];
    g[i] = gi;
    acc += gi * gi;
  }
  const double t = block_sum_256(acc, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

static int ew_blocks(int n) { return std::max(1, std::min(2048, cdiv(n, 512))); }

static void axpby(nsx_handle *h, Span sp, double *d, SRef s, SRef a, const double *v, int mode, double bytes_per) {
  const int n = sp.n;
  LaunchScope ls(h, "axpby", bytes_per * n);
  hipLaunchKernelGGL(k_axpby, dim3(ew_blocks(n)), dim3(256), 0, h->stream, n, sp.split, sp.gap, d, s, a, v, h->scal.p, h->red_partial.p, mode);
}

void v_copy(nsx_handle *h, int n, double *d, const double *s) {
  if (d != s && n) HIP_CHECK(hipMemcpyAsync(d, s, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
}
void v_zero(nsx_handle *h, int n, double *d) {
  if (n) HIP_CHECK(hipMemsetAsync(d, 0, (size_t)n * sizeof(double), h->stream));
}
void v_add(nsx_handle *h, Span n, double *d, double a, const double *v) { axpby(h, n, d, SRef{1, -1, -1, 0, 0}, SRef{a, -1, -1, 0, 0}, v, 0, 24); }
void v_add_dev(nsx_handle *h, Span n, double *d, double a, int slot, const double *v) {
  axpby(h, n, d, SRef{1, -1, -1, 0, 0}, sref(h, a, slot, -1), v, 0, 24);
}
void v_sadd(nsx_handle *h, Span n, double *d, double s, double a, const double *v) {
  axpby(h, n, d, SRef{s, -1, -1, 0, 0}, SRef{a, -1, -1, 0, 0}, v, 0, 24);
}
void v_scale(nsx_handle *h, Span n, double *d, double a) { axpby(h, n, d, SRef{a, -1, -1, 0, 0}, SRef{0, -1, -1, 0, 0}, nullptr, 2, 16); }
void v_scale_dev_inv(nsx_handle *h, Span n, double *d, int slot) { axpby(h, n, d, sref(h, 1, -1, slot), SRef{0, -1, -1, 0, 0}, nullptr, 2, 16); }
void v_scale_vec(nsx_handle *h, int n, double *d, const double *f) {
  LaunchScope ls(h, "scale_vec", 24.0 * n);
  hipLaunchKernelGGL(k_scale_vec, dim3(ew_blocks(n)), dim3(256), 0, h->stream, n, d, f);
}
void v_axpy_multi(nsx_handle *h, Span sp, double *x, int k, double *const *vs, const double *coef) {
  const int n = sp.n;
  for (int j0 = 0; j0 < k; j0 += MULTI_MAX) {
    MultiArgs m;
    m.k = std::min(MULTI_MAX, k - j0);
    for (int j = 0; j < m.k; ++j) {
      m.v[j] = vs[j0 + j];
      m.c[j] = coef[j0 + j];
    }
    LaunchScope ls(h, "axpy_multi", 8.0 * n * (2 + m.k));
    hipLaunchKernelGGL(k_axpy_multi, dim3(ew_blocks(n)), dim3(256), 0, h->stream, n, sp.split, sp.gap, x, m);
  }
}

// The same update when x does not hold its starting value yet (k <= MULTI_MAX): x = x0 + sum (x0 != nullptr), or x = sum (x0 == nullptr: the
// starting value is zero), the latter optionally followed by x = -y + x (y may be x itself).  One launch; x is only written.
void v_axpy_multi_into(nsx_handle *h, Span sp, double *x, const double *x0, const double *y, int k, double *const *vs, const double *coef) {
  if (k > MULTI_MAX || (x0 && y)) NSX_THROW(NSX_ERR_ARG, "internal: v_axpy_multi_into takes one launch's worth of vectors, and y only with a zero start");
  const int n = sp.n;
  MultiArgs m;
  m.k = k;
  for (int j = 0; j < k; ++j) {
    m.v[j] = vs[j];
    m.c[j] = coef[j];
  }
  LaunchScope ls(h, "axpy_multi", 8.0 * n * (1 + (x0 ? 1 : 0) + (y ? 1 : 0) + k));
  if (x0) hipLaunchKernelGGL(k_axpy_multi_from, dim3(ew_blocks(n)), dim3(256), 0, h->stream, n, sp.split, sp.gap, x, x0, m);
  else hipLaunchKernelGGL(k_axpy_multi_zero, dim3(ew_blocks(n)), dim3(256), 0, h->stream, n, sp.split, sp.gap, x, y, m);
}

// SolverCG helpers
void cg_update(nsx_handle *h, int n, double *x, const double *d, double *g, const double *hv, int gh_slot, int dh_slot, int res_slot) {
  LaunchScope ls(h, "cg_update", 48.0 * n);
  const int nb = red_blocks(h, n);
  hipLaunchKernelGGL(k_cg_update, dim3(nb), dim3(256), 0, h->stream, n, x, d, g, hv, sref(h, 1, gh_slot, dh_slot), h->scal.p,
                     h->red_partial.p, red_out(h, res_slot, nb));
  after_reduction(h, res_slot, nb);
}
// d = (value(num)/value(den)) d - h
void cg_direction(nsx_handle *h, int n, double *d, const double *hv, int num_slot, int den_slot) {
  axpby(h, n, d, sref(h, 1, num_slot, den_slot), SRef{-1, -1, -1, 0, 0}, hv, 0, 24);
}

double read_scalar(nsx_handle *h, int slot) {
  double v;
  read_scalars(h, slot, 1, &v);
  return v;
}
// Enqueue the publication of scal[slot0 .. slot0+count) and return its sequence number; the host may enqueue more work
// before it waits for the values (collect_published).  No other publication may be enqueued in between.
unsigned long long publish_scalars(nsx_handle *h, int slot0, int count) {
  if (count > 64) NSX_THROW(NSX_ERR_ARG, "internal: read_scalars range too long");
  NbArgs args;
  for (int i = 0; i < count; ++i) {
    args.nb[i] = h->slot_nb[slot0 + i];
    h->slot_nb[slot0 + i] = 0;
  }
  const unsigned long long seq = ++h->pub_seq;
  unsigned long long *flag_dev = pub_word_dev<unsigned long long>(h, PUB_FLAG);
  hipLaunchKernelGGL(k_publish, dim3(count), dim3(256), 0, h->stream, slot0, count, args, h->red_partial.p, h->scal.p, h->pub_dev, flag_dev, seq,
                     h->pub_counter.p);
  return seq;
}
void collect_published(nsx_handle *h, unsigned long long seq, int slot0, int count, double *out) {
  wait_published(h, seq);
  for (int i = 0; i < count; ++i) out[i] = h->pub_host[slot0 + i];
}
void read_scalars(nsx_handle *h, int slot0, int count, double *out) { collect_published(h, publish_scalars(h, slot0, count), slot0, count, out); }
void write_scalar(nsx_handle *h, int slot, double v) {
  HIP_CHECK(hipStreamSynchronize(h->stream));
  h->scal_host[slot] = v;
  h->slot_nb[slot] = 0;
  HIP_CHECK(hipMemcpyAsync(h->scal.p + slot, h->scal_host + slot, sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIP_CHECK(hipStreamSynchronize(h->stream));
}

void v_reciprocal(nsx_handle *h, int n, double *d, const double *s, double num);  // nsx_solve.hip

// One op of nsx_blas1_run (include/nsx.h): the arguments are checked as far as they index the caller's arrays and the slot table; what the
// host functions refuse themselves (a launch's worth of vectors, a publication's range) is left to them.
static void blas1_op(nsx_handle *h, Span whole, int m, const std::vector<DevBuf<double>> &vec, const nsx_blas1_op &op, double *out,
                     double *scalars_out, int scalars_cap, int &n_scalars) {
  if (op.n < 0 || op.n > whole.split) NSX_THROW(NSX_ERR_ARG, "nsx_blas1_run: an op's own length %d (split %d)", op.n, whole.split);
  const Span sp = op.n > 0 ? Span(op.n) : whole;
  auto V = [&](int i, bool optional = false) -> double * {
    if (i < 0 && optional) return nullptr;
    if (i < 0 || i >= m) NSX_THROW(NSX_ERR_ARG, "nsx_blas1_run: vector index %d of %d", i, m);
    return vec[i].p;
  };
  auto S = [&](int s, bool optional = false, int count = 1) {
    if (s < 0 && optional) return -1;
    if (s < 0 || count < 1 || s + count > S_AGREE) NSX_THROW(NSX_ERR_ARG, "nsx_blas1_run: slots %d .. %d + %d", s, s, count);
    return s;
  };
  auto plain = [&]() {
    if (sp.gap != 0) NSX_THROW(NSX_ERR_ARG, "nsx_blas1_run: op %d takes a plain length", op.kind);
    return sp.n;
  };
  bool has_result = false;
  switch (op.kind) {
    case NSX_BLAS1_DOT:
      v_dot(h, sp, V(op.d), V(op.w), S(op.slot));
      has_result = true;
      break;
    case NSX_BLAS1_ADD_AND_DOT:
      v_add_and_dot(h, sp, V(op.d), op.a, S(op.num, true), V(op.v), V(op.w), S(op.slot));
      has_result = true;
      break;
    case NSX_BLAS1_ADD: v_add(h, sp, V(op.d), op.a, V(op.v)); break;
    case NSX_BLAS1_ADD_DEV: v_add_dev(h, sp, V(op.d), op.a, S(op.num), V(op.v)); break;
    case NSX_BLAS1_SADD: v_sadd(h, sp, V(op.d), op.s, op.a, V(op.v)); break;
    case NSX_BLAS1_SCALE: v_scale(h, sp, V(op.d), op.a); break;
    case NSX_BLAS1_SCALE_DEV_INV: v_scale_dev_inv(h, sp, V(op.d), S(op.den)); break;
    case NSX_BLAS1_SCALE_VEC: v_scale_vec(h, plain(), V(op.d), V(op.v)); break;
    case NSX_BLAS1_AXPY_MULTI:
    case NSX_BLAS1_AXPY_MULTI_INTO: {
      if (op.k < 0 || op.k > NSX_BLAS1_MAX_K) NSX_THROW(NSX_ERR_ARG, "nsx_blas1_run: %d terms", op.k);
      double *vs[NSX_BLAS1_MAX_K];
      for (int j = 0; j < op.k; ++j) vs[j] = V(op.vs[j]);
      if (op.kind == NSX_BLAS1_AXPY_MULTI) v_axpy_multi(h, sp, V(op.d), op.k, vs, op.coef);
      else v_axpy_multi_into(h, sp, V(op.d), V(op.v, true), V(op.w, true), op.k, vs, op.coef);
      break;
    }
    case NSX_BLAS1_CG_UPDATE:
      cg_update(h, plain(), V(op.d), V(op.v), V(op.w), V(op.x), S(op.num), S(op.den), S(op.slot));
      has_result = true;
      break;
    case NSX_BLAS1_CG_DIRECTION: cg_direction(h, plain(), V(op.d), V(op.v), S(op.num), S(op.den)); break;
    case NSX_BLAS1_RECIPROCAL: v_reciprocal(h, plain(), V(op.d), V(op.v), op.a); break;
    case NSX_BLAS1_FINALIZE: finalize_slots(h, S(op.slot, false, op.count), op.count); break;
    case NSX_BLAS1_READ: {
      S(op.slot, false, op.count);
      if (n_scalars + op.count > scalars_cap || !scalars_out) NSX_THROW(NSX_ERR_ARG, "nsx_blas1_run: scalars_out holds %d values", scalars_cap);
      std::vector<double> vals(op.count);
      read_scalars(h, op.slot, op.count, vals.data());
      for (int i = 0; i < op.count; ++i) scalars_out[n_scalars++] = vals[i];
      *out = vals[0];
      return;
    }
    case NSX_BLAS1_WRITE_SCALAR:
      write_scalar(h, S(op.slot), op.a);
      has_result = true;
      break;
    default: NSX_THROW(NSX_ERR_ARG, "nsx_blas1_run: kind %d", op.kind);
  }
  *out = 0.0;
  if (op.read) {
    if (!has_result) NSX_THROW(NSX_ERR_ARG, "nsx_blas1_run: op %d has no result slot to read", op.kind);
    read_scalars(h, op.slot, 1, out);
  }
}

}  // namespace nsx

// A program of BLAS-1 operations on the caller's vectors: see include/nsx.h.  For tests/test_gpu_blas1.py.
extern "C" int nsx_blas1_run(nsx_handle *h, int n, int split, int gap, int m, double *vectors, int n_ops, const nsx_blas1_op *ops, double *out,
                             double *scalars_out, int scalars_cap) {
  if (!h || !vectors || n < 1 || m < 1 || split < 0 || split > n || gap < 0 || (split == n && gap != 0) || n_ops < 0 || (n_ops && (!ops || !out)) ||
      scalars_cap < 0)
    return NSX_ERR_ARG;
  NSX_TRY(h)
  if (!h->have_mesh) NSX_THROW(NSX_ERR_ARG, "nsx_blas1_run needs a mesh: call nsx_set_mesh first");
  if (h->dist) NSX_THROW(NSX_ERR_UNSUPPORTED, "nsx_blas1_run works on a single-process handle only");
  HIP_CHECK(hipSetDevice(h->prm.device));
  const size_t len = (size_t)n + gap;
  std::vector<nsx::DevBuf<double>> v(m);
  for (int k = 0; k < m; ++k) v[k].upload(vectors + (size_t)k * len, len, h->stream);
  auto forget = [&]() {
    for (int s = 0; s < nsx::N_SLOTS; ++s) h->slot_nb[s] = 0;
  };
  forget();
  try {
    const nsx::Span sp(n, split, gap);
    int n_scalars = 0;
    for (int i = 0; i < n_ops; ++i) nsx::blas1_op(h, sp, m, v, ops[i], out + i, scalars_out, scalars_cap, n_scalars);
    HIP_CHECK(hipStreamSynchronize(h->stream));
  } catch (...) {
    (void)hipStreamSynchronize(h->stream);  // the vectors are released on the way out
    forget();
    throw;
  }
  forget();
  for (int k = 0; k < m; ++k) v[k].download(vectors + (size_t)k * len, len, h->stream);
  NSX_CATCH(h)
}

extern "C" int nsx_persistent_state(nsx_handle *h, int state[4]) {
  if (!h || !state) return NSX_ERR_ARG;
  NSX_TRY(h)
  HIP_CHECK(hipSetDevice(h->prm.device));
  state[0] = h->mgs.box.allocated() && !h->mgs.disabled && h->mgs.max_wg > 0;
  state[1] = h->cg.box.allocated() && !h->cg.disabled && h->cg.max_wg > 0;
  state[2] = h->n_persistent_fallbacks;
  state[3] = nsx::mgs_dirty_words(h) + nsx::cg_dirty_words(h);
  NSX_CATCH(h)
}

// Which code paths this handle's products and solves take (tests, bench.py's rehearsal log): see include/nsx.h
extern "C" int nsx_path_info(nsx_handle *h, int info[32]) {
  if (!h || !info) return NSX_ERR_ARG;
  for (int k = 0; k < 32; ++k) info[k] = 0;
  if (!h->have_mesh) return NSX_OK;
  NSX_TRY(h)
  HIP_CHECK(hipSetDevice(h->prm.device));
  const nsx::SpmvBlocked &b = h->blkA;
  info[0] = nsx::blocked_usable(h) ? 1 : 0;
  info[1] = b.n_chunks;
  info[2] = b.n_chunks_if;
  info[3] = h->mgs.last_e;
  info[4] = h->mgs.last_nwg;
  info[5] = h->mgs.last_dist;
  info[6] = h->mgs.max_e_seen;
  info[7] = h->cu_reserved;
  info[8] = h->cg.last_path;
  info[9] = h->schedS.n_blocks;
  info[10] = (int)h->haloU.nbr.size();
  info[11] = h->haloU.nbr.empty() ? 0 : h->haloU.send_ptr[h->haloU.nbr.size()];
  info[12] = h->N2_loc - h->N2;
  info[13] = h->schedS.dense ? 1 : 0;
  info[14] = h->mgs.disabled ? 1 : 0;
  info[15] = h->n_persistent_fallbacks;
  // what the distributed sweep WOULD run with an RCCL communicator (a rehearsal over host callbacks runs the two-pass sweep): the
  // instantiation for the velocity and the block vector on plain streams (only the 8-entry grid leaves RCCL's kernel room) and on
  // masked ones; 0 = the resident grid does not hold the vector
  if (!h->mgs.disabled) {
    nsx::mgs_setup(h);
    auto fit = [&](int n, const int *caps, int n_inst) {
      const nsx::MgsPick p = nsx::mgs_pick(n, caps, n_inst, nsx::MGS_ENTRIES);
      return p.fits() ? p.e : 0;
    };
    info[16] = fit(h->n_u, h->mgs.max_wg_dist, 1);
    info[17] = fit(h->n_u, h->mgs.dist_cap_reserved, 3);
    info[18] = fit(h->n_u + h->n_p, h->mgs.max_wg_dist, 1);
    info[19] = fit(h->n_u + h->n_p, h->mgs.dist_cap_reserved, 3);
    info[21] = fit(h->n_u, h->mgs.max_wg_e, 3);  // one GPU, no communicator
  }
  info[20] = nsx::cdiv(std::max(1, h->schedS.n_blocks), 1024);  // Schur blocks per entry of a partial-sum array of the two-launch CG (1: no fold launch)
  info[22] = h->N2;
  info[23] = h->NP;
  info[24] = h->mgs.last_fused;
  info[25] = h->mgs.fused_launches;
  info[26] = h->inner_F_fp32_used;
  info[27] = h->ilu_F_fp32_used;
  info[28] = h->cg.last_rpg;
  info[29] = h->cg.last_lres;
  info[30] = b.max_rows;
  info[31] = b.max_ucols;
  NSX_CATCH(h)
}

// Which ILU(0) kernels ran on the schedule of F (0) / of the Schur matrix (1): see include/nsx.h
extern "C" int nsx_ilu_path_info(nsx_handle *h, int which, int info[16]) {
  if (!h || !info || which < 0 || which > 1) return NSX_ERR_ARG;
  for (int k = 0; k < 16; ++k) info[k] = 0;
  if (!h->have_mesh) return NSX_OK;
  const nsx::IluSchedule &s = which == 0 ? h->schedF : h->schedS;
  const bool stream = s.stream_ncomp > 0 && !s.levelled;
  info[0] = s.path.factor;
  info[1] = s.path.invert;
  info[2] = s.path.solve;
  info[3] = stream ? s.stream_epl : 0;
  info[4] = s.path.solve_pf;
  info[5] = s.path.solve_ncomp;
  info[6] = s.path.solve_f32;
  info[7] = stream ? s.n_waves : 0;
  info[8] = s.n_blocks;
  info[9] = s.max_rows;
  info[10] = s.max_block_nnz;
  info[11] = stream ? s.max_wave_rows : 0;
  info[12] = s.levelled ? 1 : 0;
  info[13] = s.packed_ok ? 1 : 0;
  info[14] = s.dense ? 1 : 0;
  info[15] = s.path.factor_lds_bytes;
  return NSX_OK;
}

extern "C" int nsx_ilu_invert_staged(nsx_handle *h, int which, int *staged) {
  if (!h || !staged || which < 0 || which > 1) return NSX_ERR_ARG;
  *staged = h->have_mesh && (which == 0 ? h->schedF : h->schedS).path.invert_staged ? 1 : 0;
  return NSX_OK;
}

extern "C" int nsx_schur_plan_info(nsx_handle *h, long long info[8]) {
  if (!h || !info) return NSX_ERR_ARG;
  const nsx::SchurPlanDev &p = h->schur_plan;
  const bool have = h->have_mesh && p.current;
  const long long v[8] = {have && p.ok, have && p.used_last, p.entries, p.matches, p.slots, p.bytes, p.max_row, (long long)(1e6 * p.build_s)};
  for (int k = 0; k < 8; ++k) info[k] = have ? v[k] : 0;
  return NSX_OK;
}
