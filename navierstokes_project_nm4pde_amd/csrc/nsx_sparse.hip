// nsx_sparse.hip — sparse products of the saddle-point solve on gfx950.
//
//   block SpMV            system_matrix.vmult inside SolverGMRES    reference NavierStokes3D.cpp:574
//   F / B / B_T vmult     Preconditioners.hpp:175,201,280,304,385,398,496,507,510
//   S = B diag(v) B_T     B->mmult(negative_S, *B_T, v)              Preconditioners.hpp:144,248,358,468
// (the block-Jacobi ILU(0) these products are preconditioned with: nsx_ilu.hip)
//
// Layout exploited: F(0,0) = delta_cd (x) A with a scalar P2 x P2 operator A, so one 12-byte CSR entry serves the
// dim interleaved velocity components (the reference streams dim^2 entries, 2/3 of them explicit zeros, SURVEY A-struct).
// All kernels are HBM/L2-bandwidth bound; reductions inside a row use wavefront shuffles (64-wide waves, sub-groups of
// 8/16/32/64 lanes per row chosen from the average row length: lane_group_sum, nsx_internal.hpp).
#include "nsx_internal.hpp"
#include "../host/schur_plan.hpp"

namespace nsx {

// ------------------------------------------------------------------ SpMV
// y[i][c] = sum_j A[i,j] x[j][c]  (+ sum_k G[i,k][c] xp[k]);  W lanes per row.
// RESID (the residual of a Krylov cycle): y = b - (A x), the subtraction applied to the finished row sum -- the double the plain kernel
// stores, so the result is bit for bit that of the product followed by sadd(-1, 1, b).
template <int DIM, int W, bool WITH_G, bool RESID>
__device__ __forceinline__ void spmv_vel_rows(int n_rows, const int32_t *__restrict__ rp, const int32_t *__restrict__ ci,
                                              const double *__restrict__ av, const double *__restrict__ x,
                                              const int32_t *__restrict__ grp, const int32_t *__restrict__ gci,
                                              const double *__restrict__ gv, const double *__restrict__ xp,
                                              double *__restrict__ y, const int32_t *__restrict__ rows, const double *__restrict__ b) {
  // rows: optional list of the rows to compute (n_rows of them): interior / interface split of a distributed product
  // XCD-aware mapping: workgroups are dealt round-robin over the 8 XCDs, so give XCD k the k-th contiguous eighth of the
  // rows: the x entries a row gathers are then shared inside one 4-MiB L2 instead of being fetched into all eight
  // (grid is a multiple of 8; speed only, any placement is correct).
  const int bid = (blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3);
  const int slot = (bid * 256 + threadIdx.x) / W, lane = threadIdx.x % W;
  if (slot >= n_rows) return;  // whole groups exit together
  const int row = rows ? rows[slot] : slot;
  double acc[DIM];
#pragma unroll
  for (int c = 0; c < DIM; ++c) acc[c] = 0.0;
  const int e = rp[row + 1];
  for (int p = rp[row] + lane; p < e; p += W) {
    const double a = av[p];
    const double *xj = x + (size_t)ci[p] * DIM;
#pragma unroll
    for (int c = 0; c < DIM; ++c) acc[c] += a * xj[c];
  }
  if (WITH_G) {
    const int ge = grp[row + 1];
    for (int p = grp[row] + lane; p < ge; p += W) {
      const double xk = xp[gci[p]];
#pragma unroll
      for (int c = 0; c < DIM; ++c) acc[c] += gv[(size_t)p * DIM + c] * xk;
    }
  }
#pragma unroll
  for (int c = 0; c < DIM; ++c) acc[c] = lane_group_sum<W>(acc[c]);
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < DIM; ++c) y[(size_t)row * DIM + c] = RESID ? b[(size_t)row * DIM + c] - acc[c] : acc[c];
  }
}
template <int DIM, int W, bool WITH_G>
__global__ __launch_bounds__(256) void k_spmv_vel(int n_rows, const int32_t *__restrict__ rp, const int32_t *__restrict__ ci,
                                                  const double *__restrict__ av, const double *__restrict__ x,
                                                  const int32_t *__restrict__ grp, const int32_t *__restrict__ gci,
                                                  const double *__restrict__ gv, const double *__restrict__ xp,
                                                  double *__restrict__ y, const int32_t *__restrict__ rows) {
  spmv_vel_rows<DIM, W, WITH_G, false>(n_rows, rp, ci, av, x, grp, gci, gv, xp, y, rows, nullptr);
}
template <int DIM, int W>
__global__ __launch_bounds__(256) void k_spmv_vel_resid(int n_rows, const int32_t *__restrict__ rp, const int32_t *__restrict__ ci,
                                                        const double *__restrict__ av, const double *__restrict__ x, double *__restrict__ y,
                                                        const int32_t *__restrict__ rows, const double *__restrict__ b) {
  spmv_vel_rows<DIM, W, false, true>(n_rows, rp, ci, av, x, nullptr, nullptr, nullptr, nullptr, y, rows, b);
}

// y_u[i][c] (+)= sum_k G[i,k][c] xp[k]
template <int DIM, int W>
__global__ __launch_bounds__(256) void k_spmv_G(int n_rows, const int32_t *__restrict__ rp, const int32_t *__restrict__ ci,
                                                const double *__restrict__ gv, const double *__restrict__ xp,
                                                double *__restrict__ y, int accumulate, const int32_t *__restrict__ rows) {
  const int slot = (blockIdx.x * 256 + threadIdx.x) / W, lane = threadIdx.x % W;
  if (slot >= n_rows) return;
  const int row = rows ? rows[slot] : slot;
  double acc[DIM];
#pragma unroll
  for (int c = 0; c < DIM; ++c) acc[c] = 0.0;
  const int e = rp[row + 1];
  for (int p = rp[row] + lane; p < e; p += W) {
    const double xk = xp[ci[p]];
#pragma unroll
    for (int c = 0; c < DIM; ++c) acc[c] += gv[(size_t)p * DIM + c] * xk;
  }
#pragma unroll
  for (int c = 0; c < DIM; ++c) acc[c] = lane_group_sum<W>(acc[c]);
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < DIM; ++c) {
      double *o = y + (size_t)row * DIM + c;
      *o = accumulate ? *o + acc[c] : acc[c];
    }
  }
}

// y_p[i] = sum_j sum_c B[i,j][c] xu[j][c]
// SUB: 0 the product; 1: y = (B xu) - r; -1: y = r - (B xu) -- add(-1, r) / sadd(-1, 1, r) applied to the finished row sum
template <int DIM, int W, int SUB>
__device__ __forceinline__ void spmv_B_rows(int n_rows, const int32_t *__restrict__ rp, const int32_t *__restrict__ ci,
                                            const double *__restrict__ bv, const double *__restrict__ xu,
                                            double *__restrict__ y, const int32_t *__restrict__ rows, const double *__restrict__ r) {
  const int slot = (blockIdx.x * 256 + threadIdx.x) / W, lane = threadIdx.x % W;
  if (slot >= n_rows) return;
  const int row = rows ? rows[slot] : slot;
  double acc = 0.0;
  const int e = rp[row + 1];
  for (int p = rp[row] + lane; p < e; p += W) {
    const double *xj = xu + (size_t)ci[p] * DIM;
#pragma unroll
    for (int c = 0; c < DIM; ++c) acc += bv[(size_t)p * DIM + c] * xj[c];
  }
  acc = lane_group_sum<W>(acc);
  if (lane == 0) y[row] = SUB > 0 ? acc - r[row] : SUB < 0 ? r[row] - acc : acc;
}
template <int DIM, int W>
__global__ __launch_bounds__(256) void k_spmv_B(int n_rows, const int32_t *__restrict__ rp, const int32_t *__restrict__ ci,
                                                const double *__restrict__ bv, const double *__restrict__ xu,
                                                double *__restrict__ y, const int32_t *__restrict__ rows) {
  spmv_B_rows<DIM, W, 0>(n_rows, rp, ci, bv, xu, y, rows, nullptr);
}
template <int DIM, int W, int SUB>
__global__ __launch_bounds__(256) void k_spmv_B_sub(int n_rows, const int32_t *__restrict__ rp, const int32_t *__restrict__ ci,
                                                    const double *__restrict__ bv, const double *__restrict__ xu,
                                                    double *__restrict__ y, const int32_t *__restrict__ rows, const double *__restrict__ r) {
  spmv_B_rows<DIM, W, SUB>(n_rows, rp, ci, bv, xu, y, rows, r);
}

template <int W>
__global__ __launch_bounds__(256) void k_spmv_csr(int n_rows, const int32_t *__restrict__ rp, const int32_t *__restrict__ ci,
                                                  const double *__restrict__ v, const double *__restrict__ x,
                                                  double *__restrict__ y, const int32_t *__restrict__ rows) {
  const int slot = (blockIdx.x * 256 + threadIdx.x) / W, lane = threadIdx.x % W;
  if (slot >= n_rows) return;
  const int row = rows ? rows[slot] : slot;
  double acc = 0.0;
  const int e = rp[row + 1];
  for (int p = rp[row] + lane; p < e; p += W) acc += v[p] * x[ci[p]];
  acc = lane_group_sum<W>(acc);
  if (lane == 0) y[row] = acc;
}

#ifdef NSX_SPMV_TRACE  // development only (tools/spmv_trace.sh): wall-clock stamps of every workgroup of ONE launch of the LDS-staged SpMV
__device__ unsigned long long *g_spmv_trace = nullptr;
__device__ int g_spmv_dbg = 0;  // what the traced launch leaves out: 1 the x gathers, 2 gathers from consecutive addresses, 3 the matrix stream, 4 all of the staging
#define SPMV_DBG (g_spmv_trace ? g_spmv_dbg : 0)
#define SPMV_STAMP(k)                                                                              \
  do {                                                                                             \
    if (g_spmv_trace && threadIdx.x == 0) g_spmv_trace[(size_t)blockIdx.x * 4 + (k)] = wall_clock64(); \
  } while (0)
#else
#define SPMV_DBG 0
#define SPMV_STAMP(k) \
  do {                \
  } while (0)
#endif

// LDS-staged SpMV: y[i][c] = sum_j A[i,j] x[j][c] with the chunk's x entries gathered ONCE into LDS (SpmvBlocked).
// The per-non-zero stream is 8 B value + 2 B local column; the 24-B gathers of the plain kernel (10 M per product,
// bound by the per-CU address rate, not by bytes) become ~1.5 M staged gathers + LDS reads.
// VT: the type the matrix stream stores its values in.  double: F as assembled.  float (NSX_INNER_FP32, k_spmv_blocked_f32): the float
// copy of F the inner solves read -- 4 B value + 2 B local column per non-zero; a value is widened to double in the register it arrives
// in, so lanes, trips, row order and the grouping of every row's sum are those of the double kernel: the result is the double kernel's on
// (double)(float)F up to nothing (same operations on the same operands in the same order).
// RESID (k_spmv_blocked_resid, the residual of a Krylov cycle): y = b - (A x), the subtraction applied to the finished row sum.
template <int DIM, int W, class VT, bool RESID = false>
__device__ __forceinline__ void spmv_blocked_rows(int n_rows, const int32_t *__restrict__ desc, const int32_t *__restrict__ rp,
                                                  const uint16_t *__restrict__ lidx, const VT *__restrict__ av, const int32_t *__restrict__ ucols,
                                                  const double *__restrict__ x, double *__restrict__ y, const double *__restrict__ b = nullptr) {
  extern __shared__ double xs[];
  __shared__ int rps[449];
  // launch order (SpmvBlocked::desc): workgroups are dealt round-robin over the 8 XCDs and XCD k takes a contiguous range of chunks, so
  // the x entries its chunks stage (neighbouring chunks share most of them) stay in ONE 4-MiB L2 instead of being fetched into all
  // eight (x is 8 MB at 1 M DoF); inside an XCD the chunks with the most non-zeros start first.  Speed only.
  const int4 d = reinterpret_cast<const int4 *>(desc)[blockIdx.x];
  const int c0 = d.x, nu = d.y, r0 = d.z, r1 = d.w;
  if (r1 <= r0) return;
  SPMV_STAMP(0);
  [[maybe_unused]] const int dbg = SPMV_DBG;
  for (int t = threadIdx.x; t <= r1 - r0; t += 256) rps[t] = rp[r0 + t];
  for (int t = threadIdx.x; t < nu && dbg != 4; t += 256) {
    const int u = dbg == 2 ? (c0 + t) % n_rows : ucols[c0 + t];
    const double *xj = x + (size_t)u * DIM;
#pragma unroll
    for (int c = 0; c < DIM; ++c) xs[t * DIM + c] = dbg == 1 ? (double)u : xj[c];
  }
  __syncthreads();
  SPMV_STAMP(1);
  static_assert(W == 8 || W == 16 || W == 32, "lanes per row");
  constexpr int G = 256 / W, U = 64 / W;  // rows in flight per pass, loads per lane kept in flight (W = 16: 4; a register set holds 64 entries of a row)
  const int grp = threadIdx.x / W, lane = threadIdx.x % W;
  // software pipeline over the rows of this lane group: the loads of the next row are issued before the current row is
  // reduced, so a wave always has 2*U value loads + 2*U index loads outstanding instead of one dependent chain per row
  double a[U], na[U];
  int l[U], nl[U];
  int row = r0 + grp;
  auto fetch = [&](int rw, double (&va)[U], int (&vl)[U]) {
    const bool live = rw < r1;
    const int p0 = live ? rps[rw - r0] + lane : 0, e = live ? rps[rw - r0 + 1] : 0;
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const int q = p0 + k * W;
      const bool ok = q < e;
      va[k] = ok ? (double)ld_stream<2>(av + q) : 0.0;
      vl[k] = ok ? (int)ld_stream<2>(lidx + q) : 0;
    }
  };
  auto consume = [&](int rw, const double (&va)[U], const int (&vl)[U]) {
    if (rw >= r1) return;
    double acc[DIM];
#pragma unroll
    for (int c = 0; c < DIM; ++c) acc[c] = 0.0;
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const double *xj = xs + vl[k] * DIM;
#pragma unroll
      for (int c = 0; c < DIM; ++c) acc[c] += va[k] * xj[c];
    }
    const int e = rps[rw - r0 + 1];
    for (int p = rps[rw - r0] + lane + U * W; p < e; p += W) {  // rows longer than U*W entries (rare)
      const double av_ = (double)av[p];
      const double *xj = xs + (int)lidx[p] * DIM;
#pragma unroll
      for (int c = 0; c < DIM; ++c) acc[c] += av_ * xj[c];
    }
#pragma unroll
    for (int c = 0; c < DIM; ++c) acc[c] = lane_group_sum<W>(acc[c]);
    if (lane == 0) {
#pragma unroll
      for (int c = 0; c < DIM; ++c) y[(size_t)rw * DIM + c] = RESID ? b[(size_t)rw * DIM + c] - acc[c] : acc[c];
    }
  };
  // two register sets, no moves: while one row is reduced the loads of the next two are in flight
  if (SPMV_DBG == 3) row = r1;
  fetch(row, a, l);
  fetch(row + G, na, nl);
  for (; row < r1; row += 2 * G) {
    consume(row, a, l);
    fetch(row + 2 * G, a, l);
    consume(row + G, na, nl);
    fetch(row + 3 * G, na, nl);
  }
#ifdef NSX_SPMV_TRACE
  __syncthreads();
  SPMV_STAMP(2);
  if (g_spmv_trace && threadIdx.x == 0) {
    unsigned xcc, id;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(id));
    g_spmv_trace[(size_t)blockIdx.x * 4 + 3] = ((unsigned long long)xcc << 32) | id;
  }
#endif
}

template <int DIM, int W>
__global__ __launch_bounds__(256) void k_spmv_blocked(int n_rows, const int32_t *__restrict__ desc, const int32_t *__restrict__ rp, const uint16_t *__restrict__ lidx,
                                                      const double *__restrict__ av, const int32_t *__restrict__ ucols, const double *__restrict__ x,
                                                      double *__restrict__ y) {
  spmv_blocked_rows<DIM, W, double>(n_rows, desc, rp, lidx, av, ucols, x, y);
}
template <int DIM, int W>
__global__ __launch_bounds__(256) void k_spmv_blocked_resid(int n_rows, const int32_t *__restrict__ desc, const int32_t *__restrict__ rp, const uint16_t *__restrict__ lidx,
                                                            const double *__restrict__ av, const int32_t *__restrict__ ucols, const double *__restrict__ x,
                                                            double *__restrict__ y, const double *__restrict__ b) {
  spmv_blocked_rows<DIM, W, double, true>(n_rows, desc, rp, lidx, av, ucols, x, y, b);
}
#ifndef NSX_SPMV_F32_W
#define NSX_SPMV_F32_W 16  // lanes per row of the float kernel (compile time; 16 = the double kernel's, the only value with its grouping of the sums)
#endif
// the same product with the float copy of the values (NSX_INNER_FP32: the operator of the inner GMRES on F and aYosida's F->vmult)
template <int DIM, int W>
__global__ __launch_bounds__(256) void k_spmv_blocked_f32(int n_rows, const int32_t *__restrict__ desc, const int32_t *__restrict__ rp, const uint16_t *__restrict__ lidx,
                                                          const float *__restrict__ av, const int32_t *__restrict__ ucols, const double *__restrict__ x,
                                                          double *__restrict__ y) {
  spmv_blocked_rows<DIM, W, float>(n_rows, desc, rp, lidx, av, ucols, x, y);
}

// float copy of a value array (F for the inner products of a handle in NSX_INNER_FP32); a value beyond float's range raises the word
// ilu_check() reads (code 4) instead of leaving an inf in the stream
__global__ __launch_bounds__(256) void k_to_f32(int64_t n, const double *__restrict__ v, float *__restrict__ out, int *__restrict__ err) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double d = v[i];
  const float f = (float)d;
  out[i] = f;
  if (!(fabsf(f) <= 3.402823466e+38f)) __hip_atomic_store(err, 4, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);  // inf or NaN
}

static double bytes_vel(nsx_handle *h, bool with_g, bool f32 = false) {
  double b = (f32 ? 8.0 : 12.0) * h->gA.nnz() + (double)h->N2 * (4 + 8.0 * h->dim * 2);  // per non-zero: value (8 B, float copy: 4 B) + column
  if (with_g) b += (4.0 + 8.0 * h->dim) * h->gG.nnz() + 4.0 * h->N2 + 8.0 * h->NP;
  return b;
}

// ---- launches (rows == nullptr: all n rows)
// b (products without block(0,1) only): y = b - A x (k_spmv_vel_resid)
static void launch_vel(nsx_handle *h, bool with_g, const double *vals, const double *x, const double *xp, double *y, const int32_t *rows, int n,
                       const double *b = nullptr) {
  if (n <= 0) return;
  const int w = with_g && !b ? 16 : h->spmv_w == 8 || h->spmv_w == 32 ? h->spmv_w : 16;  // the product with block(0,1) has the 16-lane kernel only
  with_int<2, 3>(h->dim, [&](auto D) {
    with_int<8, 16, 32>(w, [&](auto W_) {
      constexpr int DIM = decltype(D)::value, W = decltype(W_)::value;
      const dim3 grid((cdiv((int64_t)n * W, 256) + 7) & ~7);
      auto vel = [&](auto G) {
        hipLaunchKernelGGL((k_spmv_vel<DIM, W, decltype(G)::value>), grid, dim3(256), 0, h->stream, n, h->gA.rowptr.p, h->gA.colind.p, vals, x, h->gG.rowptr.p,
                           h->gG.colind.p, h->vG.p, xp, y, rows);
      };
      if (b) hipLaunchKernelGGL((k_spmv_vel_resid<DIM, W>), grid, dim3(256), 0, h->stream, n, h->gA.rowptr.p, h->gA.colind.p, vals, x, y, rows, b);
      else if (!with_g) vel(std::false_type{});
      else if constexpr (W == 16) vel(std::true_type{});
    });
  });
}
// r, sub = +-1: yp = B xu - r / r - B xu (k_spmv_B_sub)
static void launch_B(nsx_handle *h, const double *xu, double *yp, const int32_t *rows, int n, const double *r = nullptr, int sub = 0) {
  if (n <= 0) return;
  with_int<2, 3>(h->dim, [&](auto D) {
    constexpr int DIM = decltype(D)::value, W = DIM == 2 ? 32 : 64;
    const dim3 grid(cdiv((int64_t)n * W, 256));
    if (!r) hipLaunchKernelGGL((k_spmv_B<DIM, W>), grid, dim3(256), 0, h->stream, n, h->gB.rowptr.p, h->gB.colind.p, h->vB.p, xu, yp, rows);
    else
      with_int<1, -1>(sub > 0 ? 1 : -1, [&](auto S) {
        hipLaunchKernelGGL((k_spmv_B_sub<DIM, W, decltype(S)::value>), grid, dim3(256), 0, h->stream, n, h->gB.rowptr.p, h->gB.colind.p, h->vB.p, xu, yp, rows, r);
      });
  });
}
static void launch_G(nsx_handle *h, const double *xp, double *yu, bool accumulate, const int32_t *rows, int n) {
  if (n <= 0) return;
  constexpr int W = 8;
  with_int<2, 3>(h->dim, [&](auto D) {
    hipLaunchKernelGGL((k_spmv_G<decltype(D)::value, W>), dim3(cdiv((int64_t)n * W, 256)), dim3(256), 0, h->stream, n, h->gG.rowptr.p, h->gG.colind.p, h->vG.p, xp, yu,
                       (int)accumulate, rows);
  });
}
static void launch_S(nsx_handle *h, const double *x, double *y, const int32_t *rows, int n) {
  if (n <= 0) return;
  const int W = 32;
  hipLaunchKernelGGL((k_spmv_csr<W>), dim3(cdiv((int64_t)n * W, 256)), dim3(256), 0, h->stream, n, h->gS.rowptr.p, h->gS.colind.p, h->vSchur.p, x, y, rows);
}

// y_u = A x_u through the LDS-staged kernel; false if the handle has no chunk table for it
bool blocked_usable(const nsx_handle *h) {
  const SpmvBlocked &b = h->blkA;
  return h->spmv_blocked && b.n_chunks > 0 && b.max_rows <= 448 && (size_t)b.max_ucols * h->dim * sizeof(double) <= 64 * 1024;
}
// part 0: the table of a one-GPU handle / the chunks of a distributed handle whose staged columns are all owned; part 1: the chunks that
// stage a ghost column (distributed handles only; an empty table launches nothing)
// rb (double values only): y = rb - A x (k_spmv_blocked_resid)
static bool launch_blocked(nsx_handle *h, const double *vals, const double *x, double *y, int part = 0, const float *vals32 = nullptr, const double *rb = nullptr) {
  const SpmvBlocked &b = h->blkA;
  if (!blocked_usable(h)) return false;
  const size_t shm = (size_t)b.max_ucols * h->dim * sizeof(double);
  const int grid = part ? b.grid_if : b.grid;
  const int32_t *desc = part ? b.desc_if.p : b.desc.p;
  if (grid == 0) return true;
  // one launch of a kernel instantiated for the handle's dim, on the value stream v; more: the right-hand side of the residual twin
  auto go = [&](auto kernel, const auto *v, auto... more) {
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), shm, h->stream, h->N2, desc, h->gA.rowptr.p, b.lidx.p, v, b.ucols.p, x, y, more...);
  };
  if (rb) {
    with_int<2, 3>(h->dim, [&](auto D) { go(k_spmv_blocked_resid<decltype(D)::value, 16>, vals, rb); });
    return true;
  }
  if (vals32) {  // the float stream: same chunks, same launch tables
    // NSX_SPMV_F32_W = 16 lanes per row as in the double kernel: the same lanes take the same entries, so every row's sum is grouped as
    // there.  -DNSX_SPMV_F32_W=32 / 8 (compile time, measurements only: another grouping of the sums) lets a lane group read 128 / 32
    // contiguous bytes of values per trip instead of 64; both are slower (profiles/inner_fp32_spmv_width.json)
    with_int<2, 3>(h->dim, [&](auto D) { go(k_spmv_blocked_f32<decltype(D)::value, NSX_SPMV_F32_W>, vals32); });
    return true;
  }
  const auto plain = [&] { with_int<2, 3>(h->dim, [&](auto D) { go(k_spmv_blocked<decltype(D)::value, 16>, vals); }); };
#ifdef NSX_SPMV_TRACE
  static int n_call = 0;
  const bool traced = getenv("NSX_SPMV_TRACE_OUT") && ++n_call == (getenv("NSX_SPMV_TRACE_CALL") ? atoi(getenv("NSX_SPMV_TRACE_CALL")) : 5000);
  for (int mode = 0; traced && part == 0 && mode <= 4; ++mode) {  // every variant once, traced; the untraced launch below leaves the right y behind
    unsigned long long *tr = nullptr;
    (void)hipStreamSynchronize(h->stream);
    (void)hipMalloc(&tr, (size_t)grid * 4 * sizeof(unsigned long long));
    (void)hipMemset(tr, 0, (size_t)grid * 4 * sizeof(unsigned long long));
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_spmv_trace), &tr, sizeof(tr));
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_spmv_dbg), &mode, sizeof(mode));
    plain();
    (void)hipStreamSynchronize(h->stream);
    std::vector<unsigned long long> host((size_t)grid * 4);
    (void)hipMemcpy(host.data(), tr, host.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    unsigned long long *none = nullptr;
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_spmv_trace), &none, sizeof(none));
    (void)hipFree(tr);
    const std::string path = std::string(getenv("NSX_SPMV_TRACE_OUT")) + "_mode" + std::to_string(mode) + ".txt";
    if (FILE *f = fopen(path.c_str(), "w")) {
      fprintf(f, "# block chunk rows ucols t_start t_staged t_end xcc hw_id   (wall_clock64 ticks of 10 ns)\n");
      std::vector<int32_t> ds((size_t)grid * 4);
      (void)hipMemcpy(ds.data(), b.desc.p, ds.size() * 4, hipMemcpyDeviceToHost);
      for (int blk = 0; blk < grid; ++blk) {
        if (b.order[blk] < 0) continue;
        fprintf(f, "%d %d %d %d %llu %llu %llu %llu %llu\n", blk, b.order[blk], ds[4 * (size_t)blk + 3] - ds[4 * (size_t)blk + 2], ds[4 * (size_t)blk + 1],
                host[4 * (size_t)blk], host[4 * (size_t)blk + 1], host[4 * (size_t)blk + 2], host[4 * (size_t)blk + 3] >> 32, host[4 * (size_t)blk + 3] & 0xffffffffull);
      }
      fclose(f);
    }
  }
#endif
  plain();
  return true;
}

// algorithmic bytes of a ghost exchange as LaunchScope counts them (pack read + buffer write, both directions)
static double bytes_halo(const HaloPlan &p, int ncomp) {
  const int nn = (int)p.nbr.size();
  return nn ? 16.0 * (p.send_ptr[nn] + p.recv_ptr[nn]) * ncomp : 0.0;
}

// vals32: the float copy of vals (the inner products of a handle in NSX_INNER_FP32).  Only the LDS-staged kernel has a float twin: where
// it cannot be used the plain kernel reads the double values, and the handle does not report a float product (nsx_path_info [26]).
// rb: y = rb - A x in the same launches (double values only: the caller checks spmv_F_resid_fused)
void spmv_F(nsx_handle *h, const double *vals, const double *x, double *y, const float *vals32, const double *rb) {
  if (vals32 && !blocked_usable(h)) vals32 = nullptr;
  if (rb && vals32) NSX_THROW(NSX_ERR_ARG, "internal: the residual product has no float twin");
  const bool f32 = vals32 != nullptr;
  if (f32) h->inner_F_fp32_used = 1;
  if (h->dist) {
    // Scopes: "spmv_F" = the rows that need no ghost (they run while the exchange is in flight), "spmv_F_if" = the rows behind it,
    // "halo_u_wait" = what the compute stream waits for the exchange once the first launch is through (its exposed part).
    // (Round 5 tried the second launch on a SECOND compute stream behind the exchange's event, beside the first launch -- a launch of a few
    // hundred chunks costs a 12 - 18 us floor whatever it holds -- and measured it without an exchange in between, one rank's share alone
    // on the card: 1.09 M DoF / 8: +15 us per product (26 - 28 against 23 - 26 ms for a solve of 128 products), / 2: no difference.  The
    // two extra cross-stream event hops cost more than the floor they hide.  Removed.)
    double *xx = const_cast<double *>(x);
    const bool blk = blocked_usable(h);
    const double frac_if = blk ? h->blkA.frac_if : (double)h->splitA.n_interface / std::max(1, h->N2);
    comm_halo_begin(h, h->haloU, xx, h->dim);
    {
      LaunchScope ls(h, "spmv_F", bytes_vel(h, false, f32) * (1.0 - frac_if));
      if (blk) launch_blocked(h, vals, x, y, 0, vals32, rb);
      else launch_vel(h, false, vals, x, nullptr, y, h->splitA.interior.p, h->splitA.n_interior, rb);
    }
    {
      LaunchScope ls(h, "halo_u_wait", bytes_halo(h->haloU, h->dim));
      comm_halo_finish(h, h->haloU, xx, h->dim);
    }
    {
      LaunchScope ls(h, "spmv_F_if", bytes_vel(h, false, f32) * frac_if);
      if (blk) launch_blocked(h, vals, x, y, 1, vals32, rb);
      else launch_vel(h, false, vals, x, nullptr, y, h->splitA.interface.p, h->splitA.n_interface, rb);
    }
    return;
  }
  LaunchScope ls(h, "spmv_F", bytes_vel(h, false, f32));
  if (!launch_blocked(h, vals, x, y, 0, vals32, rb)) launch_vel(h, false, vals, x, nullptr, y, nullptr, h->N2, rb);
}

// F->vmult inside a preconditioner's vmult (the operator of the inner GMRES, Preconditioners.hpp:173,273,382,405; aYosida's :507)
void spmv_F_inner(nsx_handle *h, const double *x, double *y) {
  spmv_F(h, h->vF.p, x, y, h->inner_precision == NSX_INNER_FP32 ? h->vF32.p : nullptr);
}
// y = b - F x, the residual of an inner solve's cycle, in the launches of the product.  Where the product streams the float copy of F
// (no residual twin of that kernel) it is the product followed by the subtraction, as the solver does it on its own.
void spmv_F_inner_resid(nsx_handle *h, const double *x, const double *b, double *y) {
  if (h->inner_precision == NSX_INNER_FP32 && blocked_usable(h)) {
    spmv_F_inner(h, x, y);
    v_sadd(h, Span(h->n_u), y, -1., 1., b);
    return;
  }
  spmv_F(h, h->vF.p, x, y, nullptr, b);
}

// Distributed products: the rows whose columns are all owned are computed while the ghosts of the input are still on
// their way (second stream, comm_halo_begin / finish); the rows on the partition interface follow once they have arrived.
// This is the Epetra_Import + local multiply of every vmult with the import hidden behind the interior rows.
// spmv_overlapped is that protocol for one operator and one exchanged vector (ncomp components, plan): begin the exchange, launch the rows of
// the split that need no ghost, finish the exchange, launch the rows behind it; a one-GPU handle makes the single launch over all n_rows rows.
// launch(rows, n): n rows listed in rows, or all of them (rows == nullptr).  spmv_F above and spmv_saddle below spell the protocol out
// themselves: the first times its three parts in scopes of their own and has a chunk-table variant, the second begins two exchanges.
template <class Launch>
static void spmv_overlapped(nsx_handle *h, HaloPlan &plan, const double *x, int ncomp, const RowSplit &sp, int n_rows, Launch launch) {
  if (!h->dist) {
    launch(nullptr, n_rows);
    return;
  }
  double *xx = const_cast<double *>(x);
  comm_halo_begin(h, plan, xx, ncomp);
  launch(sp.interior.p, sp.n_interior);
  comm_halo_finish(h, plan, xx, ncomp);
  launch(sp.interface.p, sp.n_interface);
}

static double bytes_B(nsx_handle *h) { return (4.0 + 8.0 * h->dim) * h->gB.nnz() + 12.0 * h->NP + 8.0 * h->dim * h->N2; }
void spmv_B(nsx_handle *h, const double *xu, double *yp, const double *r, int sub) {
  LaunchScope ls(h, "spmv_B", bytes_B(h) + (r ? 8.0 * h->NP : 0.0));
  spmv_overlapped(h, h->haloU, xu, h->dim, h->splitB, h->NP, [&](const int32_t *rows, int n) { launch_B(h, xu, yp, rows, n, r, sub); });
}

void spmv_G(nsx_handle *h, const double *xp, double *yu, bool accumulate) {
  LaunchScope ls(h, "spmv_G", (4.0 + 8.0 * h->dim) * h->gG.nnz() + (double)h->N2 * (4 + 8.0 * h->dim) + 8.0 * h->NP);
  spmv_overlapped(h, h->haloP, xp, 1, h->splitG, h->N2, [&](const int32_t *rows, int n) { launch_G(h, xp, yu, accumulate, rows, n); });
}

// BlockSparseMatrix::vmult: y_u = F x_u + block(0,1) x_p ; y_p = block(1,0) x_u  (block (1,1) has an empty pattern)
void spmv_saddle(nsx_handle *h, const double *x, double *y) {
  double *xx = const_cast<double *>(x);
  if (h->dist) {
    comm_halo_begin(h, h->haloU, xx, h->dim);
    comm_halo_begin(h, h->haloP, xx + h->off_p, 1);
  }
  const bool blk_dist = h->dist && blocked_usable(h);
  {
    LaunchScope ls(h, "spmv_saddle_u", bytes_vel(h, true));
    if (blk_dist) launch_blocked(h, h->vF.p, x, y, 0);  // F x_u on the chunks without a ghost column; the rest and += block(0,1) x_p behind the exchange
    else if (h->dist) launch_vel(h, true, h->vF.p, x, x + h->off_p, y, h->splitVel.interior.p, h->splitVel.n_interior);
    else if (launch_blocked(h, h->vF.p, x, y)) launch_G(h, x + h->off_p, y, true, nullptr, h->N2);  // F x_u staged through LDS, then += block(0,1) x_p
    else launch_vel(h, true, h->vF.p, x, x + h->off_p, y, nullptr, h->N2);
  }
  {
    LaunchScope ls(h, "spmv_B", bytes_B(h));
    if (h->dist) launch_B(h, x, y + h->off_p, h->splitB.interior.p, h->splitB.n_interior);
    else launch_B(h, x, y + h->off_p, nullptr, h->NP);
  }
  if (h->dist) {
    {
      LaunchScope ls(h, "halo_up_wait", bytes_halo(h->haloU, h->dim) + bytes_halo(h->haloP, 1));
      comm_halo_finish(h, h->haloU, xx, h->dim);
      comm_halo_finish(h, h->haloP, xx + h->off_p, 1);
    }
    LaunchScope ls(h, "spmv_saddle_if", 0);
    if (blk_dist) {
      launch_blocked(h, h->vF.p, x, y, 1);
      launch_G(h, x + h->off_p, y, true, nullptr, h->N2);
    } else {
      launch_vel(h, true, h->vF.p, x, x + h->off_p, y, h->splitVel.interface.p, h->splitVel.n_interface);
    }
    launch_B(h, x, y + h->off_p, h->splitB.interface.p, h->splitB.n_interface);
  }
}

void spmv_S(nsx_handle *h, const double *x, double *y) {
  LaunchScope ls(h, "spmv_S", 12.0 * h->gS.nnz() + 20.0 * h->NP);
  spmv_overlapped(h, h->haloP, x, 1, h->splitS, h->NP, [&](const int32_t *rows, int n) { launch_S(h, x, y, rows, n); });
}

// interior / interface rows of the distributed operators (owned rows; a column >= the owned count is a ghost)
static void split_rows(nsx_handle *h, RowSplit &sp, int n_rows, const Csr &a, int own_a, const Csr *b, int own_b) {
  std::vector<int32_t> in, out;
  for (int i = 0; i < n_rows; ++i) {
    bool ghost = false;
    for (int k = a.rowptr[i]; k < a.rowptr[i + 1] && !ghost; ++k) ghost = a.colind[k] >= own_a;
    if (b)
      for (int k = b->rowptr[i]; k < b->rowptr[i + 1] && !ghost; ++k) ghost = b->colind[k] >= own_b;
    (ghost ? out : in).push_back(i);
  }
  sp.n_interior = (int)in.size();
  sp.n_interface = (int)out.size();
  sp.interior.upload(in, h->stream);
  sp.interface.upload(out, h->stream);
}
void build_row_splits(nsx_handle *h) {
  if (!h->dist) return;
  split_rows(h, h->splitA, h->N2, h->gA.host, h->N2, nullptr, 0);
  split_rows(h, h->splitVel, h->N2, h->gA.host, h->N2, &h->gG.host, h->NP);
  split_rows(h, h->splitG, h->N2, h->gG.host, h->NP, nullptr, 0);
  split_rows(h, h->splitB, h->NP, h->gB.host, h->N2, nullptr, 0);
  split_rows(h, h->splitS, h->NP, h->gS.host, h->NP, nullptr, 0);
  if (nsx_debug())
    fprintf(stderr, "[nsx] rank %d: interface rows F %d / %d, block(1,0) %d / %d, S %d / %d\n", h->rank, h->splitA.n_interface, h->N2, h->splitB.n_interface,
            h->NP, h->splitS.n_interface, h->NP);
}

// the float copy of F for the inner products (NSX_INNER_FP32), rebuilt by every nsx_prec_initialize: F changes with every assembly and
// every apply_boundary_values, and each of them is followed by an initialisation before the next inner solve
void convert_F_f32(nsx_handle *h) {
  const int64_t n = h->gA.nnz();
  h->vF32.alloc((size_t)n);
  LaunchScope ls(h, "F_to_f32", 12.0 * (double)n);
  if (n > 0) hipLaunchKernelGGL(k_to_f32, dim3(cdiv(n, 256)), dim3(256), 0, h->stream, n, h->vF.p, h->vF32.p, pub_word_dev(h, PUB_ILU_ERR));
}

// ------------------------------------------------------------------ diagonals
__global__ void k_extract_diag(int n_nodes, int dim, const int32_t *__restrict__ diag, const double *__restrict__ v, double *__restrict__ d) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_nodes * dim) return;
  d[i] = v[diag[i / dim]];
}
__global__ void k_abs_rowsum(int n_nodes, int dim, const int32_t *__restrict__ rp, const double *__restrict__ v, double *__restrict__ d) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_nodes) return;
  double s = 0.0;
  for (int p = rp[i]; p < rp[i + 1]; ++p) s += fabs(v[p]);
  for (int c = 0; c < dim; ++c) d[(size_t)i * dim + c] = s;
}
// F->diag_element(i) for every velocity dof (Prec.hpp:137,241,353,449): the scalar diagonal replicated on dim components
void extract_diag(nsx_handle *h, const DevCsr &g, const double *vals, double *d) {
  LaunchScope ls(h, "extract_diag", 0);
  hipLaunchKernelGGL(k_extract_diag, dim3(cdiv(h->n_u, 256)), dim3(256), 0, h->stream, g.n_rows(), h->dim, g.diag.p, vals, d);
}
// sum_j |M_ij| over the row (Prec.hpp:456-465); cross-component slots of the reference's row are zero
void abs_rowsum(nsx_handle *h, const DevCsr &g, const double *vals, double *d) {
  LaunchScope ls(h, "abs_rowsum", 0);
  hipLaunchKernelGGL(k_abs_rowsum, dim3(cdiv(g.n_rows(), 256)), dim3(256), 0, h->stream, g.n_rows(), h->dim, g.rowptr.p, vals, d);
}

// ------------------------------------------------------------------ S = B diag(v) B_T  (numeric phase on the static pattern)
// block(0,1) = -block(1,0)^T with the Dirichlet rows cleared (NS3D.cpp:258,261 + apply_boundary_values), so
//   S_ij = sum_{k in row_i(B) ^ row_j(B)} sum_c B[i,k][c] * w[k][c] * B[j,k][c],   w = -v * dirichlet_mask.
// One wave per row i: row i (columns + dim weighted values) is staged in LDS, each lane takes one S entry (i,j),
// walks row j of B and merges its (sorted) columns with the LDS copy.
// THE arithmetic of one term, for the merge kernel and the planned one alike: one statement, so the two cannot be contracted differently
template <int DIM>
__device__ __forceinline__ double schur_term(double acc, const double *rv, const double *__restrict__ bv) {
#pragma unroll
  for (int c = 0; c < DIM; ++c) acc += rv[c] * bv[c];
  return acc;
}

template <int DIM>
__global__ __launch_bounds__(64) void k_schur(int n_rows, const int32_t *__restrict__ srp, const int32_t *__restrict__ sci,
                                              const int32_t *__restrict__ brp, const int32_t *__restrict__ bci,
                                              const double *__restrict__ bv, const double *__restrict__ w, int max_row,
                                              double *__restrict__ sv) {
  extern __shared__ double smem[];
  double *rv = smem;                                  // [max_row][DIM]
  int32_t *rc = (int32_t *)(smem + (size_t)max_row * DIM);  // [max_row]
  const int i = blockIdx.x;
  if (i >= n_rows) return;
  const int b0 = brp[i], nb = brp[i + 1] - b0;
  for (int t = threadIdx.x; t < nb; t += 64) {
    const int k = bci[b0 + t];
    rc[t] = k;
#pragma unroll
    for (int c = 0; c < DIM; ++c) rv[t * DIM + c] = bv[(size_t)(b0 + t) * DIM + c] * w[(size_t)k * DIM + c];
  }
  __syncthreads();
  for (int e = srp[i] + threadIdx.x; e < srp[i + 1]; e += 64) {
    const int j = sci[e];
    double acc = 0.0;
    // both rows are sorted by column: one pass over row j with a cursor into row i's LDS copy (round 5; a binary search per entry of
    // row j before: 1.24 ms per step, now 0.93).  The products enter the sum in row j's order as before: bit-identical.  What bounds it
    // now is the gather rate: every lane walks another row j, so a load instruction touches 64 different sectors (430 M lane-loads per
    // product); fetching eight entries per trip changed nothing (1.02 ms).  A wave per (i, j) pair would read row j coalesced, but
    // its sum would need the lanes' products in row order -- another rounding, another iteration history.
    int q = 0;
    for (int p = brp[j]; p < brp[j + 1]; ++p) {
      const int k = bci[p];
      while (q < nb && rc[q] < k) ++q;
      if (q < nb && rc[q] == k) acc = schur_term<DIM>(acc, rv + q * DIM, bv + (size_t)p * DIM);
    }
    sv[e] = acc;
  }
}

// The same product from the plan (host/schur_plan.hpp): which columns rows i and j share, and in which order they enter the sum, is a
// constant of the mesh, so the merge above is done once on the host.  One wave per row i as before; a lane reads its packed terms
// (position q in row i | offset in row j), 256 contiguous bytes per wave and step, and gathers only the entries of row j that
// contribute.  Same operands in the same order through the same schur_term: sv comes out bit for bit, the exact 0.0 of an entry whose
// terms are all masked included.  A lane without a term in a step (or without an entry) computes on (rv[0], bv[0]) and drops the result.
template <int DIM>
__global__ __launch_bounds__(64) void k_schur_planned(int n_rows, const int32_t *__restrict__ srp, const int32_t *__restrict__ sci,
                                                      const int32_t *__restrict__ brp, const int32_t *__restrict__ bci,
                                                      const double *__restrict__ bv, const double *__restrict__ w,
                                                      const int32_t *__restrict__ row_grp, const int64_t *__restrict__ grp_off,
                                                      const uint32_t *__restrict__ words, double *__restrict__ sv) {
  extern __shared__ double smem[];
  double *rv = smem;  // [max_row][DIM]
  const int i = blockIdx.x;
  if (i >= n_rows) return;
  const int b0 = brp[i], nb = brp[i + 1] - b0;
  for (int t = threadIdx.x; t < nb; t += 64) {
    const int k = bci[b0 + t];
#pragma unroll
    for (int c = 0; c < DIM; ++c) rv[t * DIM + c] = bv[(size_t)(b0 + t) * DIM + c] * w[(size_t)k * DIM + c];
  }
  __syncthreads();
  const int e1 = srp[i + 1], g1 = row_grp[i + 1];
  int e = srp[i] + threadIdx.x;
  for (int g = row_grp[i]; g < g1; ++g, e += 64) {
    const int64_t o1 = grp_off[g + 1];
    const bool live = e < e1;
    const size_t pj = live ? (size_t)brp[sci[e]] : 0;
    double acc = 0.0;
#pragma unroll 4
    for (int64_t o = grp_off[g] + threadIdx.x; o < o1; o += 64) {
      const uint32_t word = __builtin_nontemporal_load(words + o);  // read once per product: the gathered rows of B are what should stay in cache
      const bool term = word != SCHUR_NO_TERM;
      const int q = term ? (int)(word >> 16) : 0;
      const size_t p = term ? pj + (word & 0xffffu) : 0;
      const double with = schur_term<DIM>(acc, rv + q * DIM, bv + p * DIM);
      acc = term ? with : acc;
    }
    if (live) sv[e] = acc;
  }
}

void schur_numeric(nsx_handle *h, const double *w) {
  comm_halo_u(h, w);  // weights of ghost velocity dofs
  ensure_schur_plan(h);  // (current since the first assembly: here it only hands over the longest row)
  SchurPlanDev &pl = h->schur_plan;
  const int max_row = pl.max_row;
  // NSX_SCHUR_PLAN is read per call like its neighbours.  Handles of a distributed mesh or with a communicator stay on the merge kernel.
  const bool planned = env_on("NSX_SCHUR_PLAN") && pl.ok && !h->dist && !h->comm;
  const size_t shm = (size_t)max_row * (h->dim * 8 + (planned ? 0 : 4)) + 8;
  if (shm > 160 * 1024) NSX_THROW(NSX_ERR_UNSUPPORTED, "row of block(1,0) too long for the Schur kernel (%d)", max_row);
  pl.used_last = planned;
  LaunchScope ls(h, "schur_numeric", 0);
  with_int<2, 3>(h->dim, [&](auto D) {
    if (planned)
      hipLaunchKernelGGL((k_schur_planned<decltype(D)::value>), dim3(h->NP), dim3(64), shm, h->stream, h->NP, h->gS.rowptr.p, h->gS.colind.p, h->gB.rowptr.p,
                         h->gB.colind.p, h->vB.p, w, pl.row_grp.p, pl.grp_off.p, pl.words.p, h->vSchur.p);
    else
      hipLaunchKernelGGL((k_schur<decltype(D)::value>), dim3(h->NP), dim3(64), shm, h->stream, h->NP, h->gS.rowptr.p, h->gS.colind.p, h->gB.rowptr.p,
                         h->gB.colind.p, h->vB.p, w, max_row, h->vSchur.p);
  });
}

}  // namespace nsx
