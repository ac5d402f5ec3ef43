// nsx_ilu.hip — block-Jacobi ILU(0) of the saddle-point solve on gfx950: factorisation, explicit block inverses, triangular solves.
//
//   ILU(0) factor/solve   TrilinosWrappers::PreconditionILU          Preconditioners.hpp:147-148,215-216 (Ifpack, overlap 0)
//
// The lane-owner solve stream's device side is nsx_ilu_lanes.hpp (shared with tools/ilu_lanes_bench.hip and nsx_mgs.hip), its schedule
// host/ilu_stream.hpp; the sparse products these factors precondition are nsx_sparse.hip.
#include <atomic>

#include "nsx_internal.hpp"
#include "nsx_ilu_lanes.hpp"

namespace nsx {

// ------------------------------------------------------------------ block-Jacobi ILU(0)
// One workgroup per rank block, rows visited level by level (levels precomputed on the static pattern, exact:
// the arithmetic of every row is that of the sequential IKJ sweep).  Storage = Ifpack_ILU's: strict lower = L,
// diagonal = 1/d, strict upper = U/d.  Entries whose column lies outside the block are dropped (Ifpack_LocalFilter).
constexpr int ILU_WAVES = 4;
constexpr int ILU_MAXROW = 1024;

// one off-diagonal entry of the factor into the packed solve stream: the double stream, or -- pk_val32 != null, a handle in
// NSX_INNER_FP32 -- the float stream INSTEAD (factorised in double, rounded on the way out; a value beyond float's range is reported
// through the word ilu_check() reads, code 5)
__device__ __forceinline__ void pk_store(double *__restrict__ pk_val, float *__restrict__ pk_val32, int sl, double v, int *err) {
  if (pk_val32) {
    const float f = (float)v;
    pk_val32[sl] = f;
    if (!(fabsf(f) <= 3.402823466e+38f)) __hip_atomic_store(err, 5, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  } else {
    pk_val[sl] = v;
  }
}

__global__ __launch_bounds__(ILU_WAVES * 64) void k_ilu_factor(const int32_t *__restrict__ bptr, const int32_t *__restrict__ lvl_off,
                                                              const int32_t *__restrict__ lvl_ptr, const int32_t *__restrict__ lvl_rows,
                                                              const int32_t *__restrict__ rp, const int32_t *__restrict__ ci,
                                                              const int32_t *__restrict__ diag, const double *__restrict__ a,
                                                              double *__restrict__ lu, const int32_t *__restrict__ slot_of,
                                                              double *__restrict__ pk_val, double *__restrict__ pk_dinv,
                                                              int *__restrict__ err, const int32_t *__restrict__ dinv_slot,
                                                              float *__restrict__ pk_val32) {
  __shared__ double wv[ILU_WAVES][ILU_MAXROW];
  const int blk = blockIdx.x, wave = threadIdx.x / 64, lane = threadIdx.x % 64;
  const int r0 = bptr[blk], r1 = bptr[blk + 1];
  volatile double *w = wv[wave];  // volatile: lanes of the wave exchange values through this row buffer
  for (int lv = lvl_off[blk]; lv < lvl_off[blk + 1]; ++lv) {
    const int l0 = lvl_ptr[lv], cnt = lvl_ptr[lv + 1] - l0;
    for (int r = wave; r < cnt; r += ILU_WAVES) {
      const int i = lvl_rows[l0 + r];
      const int p0 = rp[i], n = rp[i + 1] - p0, dpos = diag[i] - p0;
      if (n > ILU_MAXROW) {
        if (lane == 0) __hip_atomic_store(err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        continue;
      }
      for (int t = lane; t < n; t += 64) {
        const int j = ci[p0 + t];
        w[t] = (j >= r0 && j < r1) ? a[p0 + t] : 0.0;
      }
      __builtin_amdgcn_wave_barrier();
      for (int t = 0; t < dpos; ++t) {  // L part, ascending columns (wave-uniform loop)
        const int j = ci[p0 + t];
        if (j < r0) continue;
        const int dj = diag[j];
        const double mult = w[t];
        __builtin_amdgcn_wave_barrier();
        if (lane == 0) w[t] = mult * lu[dj];  // InV[jj] *= DV[j]
        const int ue = rp[j + 1];
        for (int q = dj + 1 + lane; q < ue; q += 64) {  // scaled U row of j
          const int c = ci[q];
          if (c >= r1) break;
          int lo = t + 1, hi = n - 1;  // columns of row i are sorted; c > j
          while (lo <= hi) {
            const int mid = (lo + hi) >> 1, cm = ci[p0 + mid];
            if (cm < c) lo = mid + 1; else if (cm > c) hi = mid - 1; else { w[mid] -= mult * lu[q]; break; }
          }
        }
        __builtin_amdgcn_wave_barrier();
      }
      const double d = w[dpos];
      const double dinv = 1.0 / d;
      if (lane == 0 && !(fabs(d) > 0.0)) __hip_atomic_store(err, 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      for (int t = lane; t < n; t += 64) {
        const int j = ci[p0 + t];
        double v = w[t];
        if (t == dpos) v = dinv;
        else if (t > dpos) v = (j < r1) ? v * dinv : 0.0;
        lu[p0 + t] = v;
        if (slot_of) {
          const int sl = slot_of[p0 + t];
          if (sl >= 0) pk_store(pk_val, pk_val32, sl, -v, err);  // the stream adds value * x[col]: it stores -L and -U/d
          if (t == dpos) pk_dinv[dinv_slot[i]] = dinv;
        }
      }
      __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();  // rows of the next level read the U rows written here (same CU: L1 is coherent for the workgroup)
  }
}

// ---- explicit block inverses -----------------------------------------------------------------------------------------
// P_b = U^-1 D^-1 L^-1 of one block (Ifpack storage: strict lower = L, diagonal = 1/d, strict upper = U/d), dense row-major.
// Thread j owns column j: forward sweep Y e_j = L^-1 e_j row by row, then the backward sweep in place.  Columns are
// independent, so there is no synchronisation; for a fixed row all threads read the same factor entries (broadcast)
// and consecutive entries of a row of P (coalesced).
// The same with the block's matrix in LDS while it is built (round 5): a thread owns a column and walks the rows; every row reads
// entries of its column that the same thread wrote a few rows earlier -- through global memory that is a store -> load round trip
// through L2 per row (0.76 ms per step for 511 blocks of <= 96 rows), through LDS a few hundred cycles.  Same operations on the same
// operands in the same order: bit-identical (tests/test_gpu_errors.py).
// STAGE: all threads of the workgroup walk the same (column, value) sequence of every row, so the block's IN-BLOCK factor entries --
// per row the strict-lower ones from column r0 on, the diagonal, the strict-upper ones below column r0 + n, in CSR order: exactly the
// entries the sweeps below do not skip -- are copied once into LDS behind Ps (value + 16-bit local column, compact row starts from the
// schedule's in_cptr / in_cpos as k_ilu_factor_lds stages them) and the sweeps read nothing from global memory.  Same operations,
// operands and order.  ilu_invert_stage_bytes says what that takes; where it does not fit the device, STAGE = false reads the factor
// from global memory as before.
__host__ __device__ inline size_t ilu_invert_stage_bytes(int max_rows, int max_nz) {
  return (size_t)max_rows * max_rows * sizeof(double) + (size_t)max_nz * sizeof(double) + (((size_t)max_nz * sizeof(uint16_t) + 7) & ~(size_t)7);
}
constexpr size_t ILU_INVERT_STATIC_LDS = (113 + 112) * sizeof(int);  // s_rp, s_dg below: the tables

// acc - value * P[k][j]: the statement of both sweeps, the expression `acc -= lu[p] * Ps[k * n + j]` of the unstaged loops (one
// fused multiply-add either way: tests/test_gpu_ilu_invert_stage.py compares the two bit for bit)
__device__ __forceinline__ double ilu_invert_term(double acc, double value, double p) { return acc - value * p; }

// acc minus the entries [c0, c1) of the staged factor times their rows of column j (Pcol = Ps + j), in order.  Eight entries per trip:
// none of their loads depends on acc (only the sums chain), so the compiler overlaps them; a trip's slots beyond c1 fetch entry c and
// are dropped.  Measured at 1.09 M DoF: 0.333 ms per step against 0.372 ms entry by entry; sixteen per trip with the three stages held
// apart by scheduling barriers and branches instead of selects: 0.382 ms.
__device__ __forceinline__ double ilu_invert_row(double acc, const double *sval, const uint16_t *scol, const double *Pcol, int n, int c0, int c1) {
  constexpr int U = 8;
  for (int c = c0; c < c1; c += U) {
    double v[U], p[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int cc = c + u < c1 ? c + u : c;
      v[u] = sval[cc];
      p[u] = Pcol[scol[cc] * n];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) acc = c + u < c1 ? ilu_invert_term(acc, v[u], p[u]) : acc;
  }
  return acc;
}

template <bool STAGE>
__global__ __launch_bounds__(128) void k_ilu_invert_lds(const int32_t *__restrict__ bptr, const int64_t *__restrict__ off,
                                                        const int32_t *__restrict__ rp, const int32_t *__restrict__ ci,
                                                        const int32_t *__restrict__ diag, const double *__restrict__ lu, double *__restrict__ P,
                                                        const int32_t *__restrict__ in_lo, const int32_t *__restrict__ in_cptr,
                                                        const int32_t *__restrict__ in_cpos) {
  extern __shared__ double Ps[];  // [n][n] row-major: column j of all rows by thread j, consecutive threads on consecutive banks
  __shared__ int s_rp[113], s_dg[112];  // the rows' entry ranges and diagonal positions: one trip for the block instead of one per row
  const int blk = blockIdx.x, r0 = bptr[blk], n = bptr[blk + 1] - r0;
  const int j = threadIdx.x;
  if constexpr (STAGE) {
    const int c0 = in_cptr[r0], nz = in_cptr[r0 + n] - c0;
    double *sval = Ps + n * n;                    // [nz] the in-block entries in compact order
    uint16_t *scol = (uint16_t *)(sval + nz);     // [nz] their columns, local to the block
    for (int t = threadIdx.x; t <= n; t += 128) s_rp[t] = in_cptr[r0 + t] - c0;
    for (int t = threadIdx.x; t < n; t += 128) s_dg[t] = in_cptr[r0 + t] - c0 + (diag[r0 + t] - in_lo[r0 + t]);
    for (int c = threadIdx.x; c < nz; c += 128) {
      const int p = in_cpos[c0 + c];
      sval[c] = lu[p];
      scol[c] = (uint16_t)(ci[p] - r0);
    }
    __syncthreads();
    if (j < n) {
      // the row bounds are the same in every lane: as scalars, so that the entry loops are not loops under a lane mask
      for (int i = 0; i < n; ++i) {  // Y = L^-1 (unit lower)
        const int c0 = __builtin_amdgcn_readfirstlane(s_rp[i]), pe = __builtin_amdgcn_readfirstlane(s_dg[i]);
        Ps[i * n + j] = ilu_invert_row(i == j ? 1.0 : 0.0, sval, scol, Ps + j, n, c0, pe);
      }
      for (int i = n - 1; i >= 0; --i) {  // P = U^-1 (D^-1 Y), in place from the last row up
        const int pd = __builtin_amdgcn_readfirstlane(s_dg[i]), pe = __builtin_amdgcn_readfirstlane(s_rp[i + 1]);
        Ps[i * n + j] = ilu_invert_row(sval[pd] * Ps[i * n + j], sval, scol, Ps + j, n, pd + 1, pe);
      }
    }
    __syncthreads();
    double *Pb = P + off[blk];
    for (int q = threadIdx.x; q < n * n; q += 128) Pb[q] = Ps[q];
    return;
  }
  for (int t = threadIdx.x; t <= n; t += 128) s_rp[t] = rp[r0 + t];
  for (int t = threadIdx.x; t < n; t += 128) s_dg[t] = diag[r0 + t];
  __syncthreads();
  if (j < n) {
    for (int i = 0; i < n; ++i) {  // Y = L^-1 (unit lower)
      const int pe = s_dg[i];
      double acc = i == j ? 1.0 : 0.0;
      for (int p = s_rp[i]; p < pe; ++p) {
        const int k = ci[p] - r0;
        if (k >= 0) acc -= lu[p] * Ps[k * n + j];
      }
      Ps[i * n + j] = acc;
    }
    for (int i = n - 1; i >= 0; --i) {  // P = U^-1 (D^-1 Y), in place from the last row up
      const int pd = s_dg[i], pe = s_rp[i + 1];
      double acc = lu[pd] * Ps[i * n + j];
      for (int p = pd + 1; p < pe; ++p) {
        const int k = ci[p] - r0;
        if (k < n) acc -= lu[p] * Ps[k * n + j];
      }
      Ps[i * n + j] = acc;
    }
  }
  __syncthreads();
  double *Pb = P + off[blk];
  for (int q = threadIdx.x; q < n * n; q += 128) Pb[q] = Ps[q];
}

__global__ __launch_bounds__(256) void k_ilu_invert(const int32_t *__restrict__ bptr, const int64_t *__restrict__ off,
                                                    const int32_t *__restrict__ rp, const int32_t *__restrict__ ci,
                                                    const int32_t *__restrict__ diag, const double *__restrict__ lu, double *P) {
  const int blk = blockIdx.x, r0 = bptr[blk], n = bptr[blk + 1] - r0;
  double *Pb = P + off[blk];
  for (int j = threadIdx.x; j < n; j += 256) {
    for (int i = 0; i < n; ++i) {  // Y = L^-1 (unit lower)
      const int row = r0 + i, pe = diag[row];
      double acc = i == j ? 1.0 : 0.0;
      for (int p = rp[row]; p < pe; ++p) {
        const int k = ci[p] - r0;
        if (k >= 0) acc -= lu[p] * Pb[(size_t)k * n + j];
      }
      Pb[(size_t)i * n + j] = acc;
    }
    for (int i = n - 1; i >= 0; --i) {  // P = U^-1 (D^-1 Y), in place from the last row up
      const int row = r0 + i, pd = diag[row], pe = rp[row + 1];
      double acc = lu[pd] * Pb[(size_t)i * n + j];
      for (int p = pd + 1; p < pe; ++p) {
        const int k = ci[p] - r0;
        if (k < n) acc -= lu[p] * Pb[(size_t)k * n + j];
      }
      Pb[(size_t)i * n + j] = acc;
    }
  }
}

// x_b = P_b b_b: 16 lanes per row, 64 row groups per workgroup (a ~100-row block is done in two rounds: the kernel is
// bound by load latency, not bytes, so the block gets as many loads in flight as the CU allows); optional b . x partial
constexpr int DENSE_THREADS = 1024;
__global__ __launch_bounds__(DENSE_THREADS) void k_ilu_apply_dense(const int32_t *__restrict__ bptr, const int64_t *__restrict__ off,
                                                                   const double *__restrict__ P, const double *b, double *x,
                                                                   double *__restrict__ dot_partial) {
  extern __shared__ double bs[];
  __shared__ double sh[DENSE_THREADS / 64];
  const int blk = blockIdx.x, r0 = bptr[blk], n = bptr[blk + 1] - r0;
  const double *Pb = P + off[blk];
  for (int t = threadIdx.x; t < n; t += DENSE_THREADS) bs[t] = b[r0 + t];
  __syncthreads();
  const int grp = threadIdx.x >> 4, lane = threadIdx.x & 15;
  double dot = 0.0;
  for (int i = grp; i < n; i += DENSE_THREADS / 16) {
    const double *row = Pb + (size_t)i * n;
    double a0 = 0.0, a1 = 0.0;
    int j = lane;
    for (; j + 16 < n; j += 32) {  // two independent chains, loads issued back to back
      a0 += row[j] * bs[j];
      a1 += row[j + 16] * bs[j + 16];
    }
    if (j < n) a0 += row[j] * bs[j];
    const double acc = lane_group_sum<16>(a0 + a1);
    if (lane == 0) {
      x[r0 + i] = acc;
      dot += bs[i] * acc;
    }
  }
  if (dot_partial) {
    dot = lane_group_sum<64>(dot);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = dot;
    __syncthreads();
    if (threadIdx.x == 0) {
      double t = 0.0;
#pragma unroll
      for (int k = 0; k < DENSE_THREADS / 64; ++k) t += sh[k];
      dot_partial[blk] = t;
    }
  }
}

// Same factorisation for blocks of at most ILU_DENSE_ROWS rows: every wave keeps its row as a DENSE vector over the block's
// columns in LDS (pos[c] = entry index of column c in the row, -1 outside the pattern), so an update is one LDS lookup
// instead of a binary search through global memory.  Same operations on the same entries in the same order.
constexpr int ILU_DENSE_ROWS = 512;
__global__ __launch_bounds__(ILU_WAVES * 64) void k_ilu_factor_small(const int32_t *__restrict__ bptr, const int32_t *__restrict__ lvl_off,
                                                                    const int32_t *__restrict__ lvl_ptr, const int32_t *__restrict__ lvl_rows,
                                                                    const int32_t *__restrict__ rp, const int32_t *__restrict__ ci,
                                                                    const int32_t *__restrict__ diag, const double *__restrict__ a,
                                                                    double *__restrict__ lu, const int32_t *__restrict__ slot_of,
                                                                    double *__restrict__ pk_val, double *__restrict__ pk_dinv,
                                                                    int *__restrict__ err, const int32_t *__restrict__ dinv_slot,
                                                                    float *__restrict__ pk_val32) {
  __shared__ double wv[ILU_WAVES][ILU_DENSE_ROWS];
  __shared__ short posv[ILU_WAVES][ILU_DENSE_ROWS];
  const int blk = blockIdx.x, wave = threadIdx.x / 64, lane = threadIdx.x % 64;
  const int r0 = bptr[blk], r1 = bptr[blk + 1], nb = r1 - r0;
  volatile double *w = wv[wave];  // indexed by block-local column
  volatile short *pos = posv[wave];
  for (int lv = lvl_off[blk]; lv < lvl_off[blk + 1]; ++lv) {
    const int l0 = lvl_ptr[lv], cnt = lvl_ptr[lv + 1] - l0;
    for (int r = wave; r < cnt; r += ILU_WAVES) {
      const int i = lvl_rows[l0 + r];
      const int p0 = rp[i], n = rp[i + 1] - p0, dpos = diag[i] - p0;
      for (int t = lane; t < nb; t += 64) pos[t] = -1;
      __builtin_amdgcn_wave_barrier();
      for (int t = lane; t < n; t += 64) {
        const int c = ci[p0 + t] - r0;
        if (c >= 0 && c < nb) {
          pos[c] = (short)t;
          w[c] = a[p0 + t];
        }
      }
      __builtin_amdgcn_wave_barrier();
      for (int t = 0; t < dpos; ++t) {  // L part, ascending columns (wave-uniform loop)
        const int j = ci[p0 + t];
        if (j < r0) continue;
        const int dj = diag[j];
        const double mult = w[j - r0];
        __builtin_amdgcn_wave_barrier();
        if (lane == 0) w[j - r0] = mult * lu[dj];  // InV[jj] *= DV[j]
        const int ue = rp[j + 1];
        for (int q = dj + 1 + lane; q < ue; q += 64) {  // scaled U row of j
          const int c = ci[q] - r0;
          if (c >= nb) break;
          if (pos[c] >= 0) w[c] -= mult * lu[q];
        }
        __builtin_amdgcn_wave_barrier();
      }
      const double d = w[i - r0];
      const double dinv = 1.0 / d;
      if (lane == 0 && !(fabs(d) > 0.0)) __hip_atomic_store(err, 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      for (int t = lane; t < n; t += 64) {
        const int j = ci[p0 + t], c = j - r0;
        const bool in = c >= 0 && c < nb;
        double v = in ? w[c] : 0.0;
        if (t == dpos) v = dinv;
        else if (t > dpos) v = in ? v * dinv : 0.0;
        lu[p0 + t] = v;
        if (slot_of) {
          const int sl = slot_of[p0 + t];
          if (sl >= 0) pk_store(pk_val, pk_val32, sl, -v, err);  // the stream adds value * x[col]: it stores -L and -U/d
          if (t == dpos) pk_dinv[dinv_slot[i]] = dinv;
        }
      }
      __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();  // rows of the next level read the U rows written here (same CU: L1 is coherent for the workgroup)
  }
}

// Same factorisation with the in-block part of the whole block staged in LDS (values + 16-bit local columns in the compact
// numbering of IluSchedule::in_cptr, row starts, diagonal positions, the level lists): the elimination of a row then makes no
// trip through global memory at all -- k_ilu_factor_small chases ci -> diag -> lu -> ci/lu of the pivot row through L2 for every
// L entry.  Same operations on the same entries in the same order; rows of a level are dealt to the waves, a barrier per level.
// Dynamic LDS: ilu_factor_lds_bytes(max_rows, max_block_nnz).
constexpr uint16_t ILU_NOPOS = 0xffffu;
__host__ __device__ inline size_t ilu_factor_lds_bytes(int max_rows, int max_nz) {
  const size_t nz = ((size_t)max_nz + 3) & ~(size_t)3;
  return nz * 10 + (size_t)(max_rows + 4) * 2 * (4 + ILU_WAVES);
}
__global__ __launch_bounds__(ILU_WAVES * 64) void k_ilu_factor_lds(const int32_t *__restrict__ order, const int32_t *__restrict__ bptr, const int32_t *__restrict__ lvl_off,
                                                                  const int32_t *__restrict__ lvl_ptr, const int32_t *__restrict__ lvl_rows,
                                                                  const int32_t *__restrict__ rp, const int32_t *__restrict__ ci,
                                                                  const int32_t *__restrict__ diag, const int32_t *__restrict__ in_lo,
                                                                  const int32_t *__restrict__ cptr, const int32_t *__restrict__ cpos,
                                                                  const double *__restrict__ a, double *__restrict__ lu,
                                                                  const int32_t *__restrict__ slot_of, double *__restrict__ pk_val,
                                                                  double *__restrict__ pk_dinv, int *__restrict__ err,
                                                                  const int32_t *__restrict__ dinv_slot, int max_rows, int max_nz,
                                                                  float *__restrict__ pk_val32) {
  extern __shared__ double lds_f[];
  const int nzp = (max_nz + 3) & ~3, mr = max_rows + 4;
  volatile double *lv = lds_f;                       // [nzp] the block's in-block entries, compact numbering
  volatile uint16_t *lc = (uint16_t *)(lds_f + nzp);  // [nzp] block-local column
  uint16_t *lrp = (uint16_t *)lc + nzp;              // [mr] compact row starts
  uint16_t *ldg = lrp + mr;                          // [mr] compact position of the diagonal
  uint16_t *llv = ldg + mr;                          // [mr] block-local rows in level order
  uint16_t *lvp = llv + mr;                          // [mr] level starts inside llv
  volatile uint16_t *posv = lvp + mr;                // [ILU_WAVES][mr] column -> compact position in the wave's current row
  const int blk = order[blockIdx.x], tid = threadIdx.x, wave = tid / 64, lane = tid % 64;
  const int r0 = bptr[blk], nb = bptr[blk + 1] - r0;
  if (nb == 0) return;
  const int c0 = cptr[r0];
  const int L0 = lvl_off[blk], nlev = lvl_off[blk + 1] - L0, q0 = lvl_ptr[L0];
  for (int q = tid; q <= nb; q += ILU_WAVES * 64) lrp[q] = (uint16_t)(cptr[r0 + q] - c0);
  for (int q = tid; q < nb; q += ILU_WAVES * 64) {
    ldg[q] = (uint16_t)(cptr[r0 + q] - c0 + diag[r0 + q] - in_lo[r0 + q]);
    llv[q] = (uint16_t)(lvl_rows[q0 + q] - r0);  // the level lists of a block are contiguous and hold every row once
  }
  for (int q = tid; q <= nlev; q += ILU_WAVES * 64) lvp[q] = (uint16_t)(lvl_ptr[L0 + q] - q0);
  for (int q = tid; q < ILU_WAVES * mr; q += ILU_WAVES * 64) posv[q] = ILU_NOPOS;
  // staging and write-back run flat over the block's entries (compact number -> CSR position through cpos): every load address
  // depends on the loop counter or on one earlier load, so the requests of several passes are in flight together
  const int nzb = cptr[r0 + nb] - c0;
  {
    double *lvn = lds_f;
    uint16_t *lcn = (uint16_t *)(lds_f + nzp);
    const int P1 = rp[r0 + nb];
    for (int p = rp[r0] + tid; p < P1; p += ILU_WAVES * 64) {  // entries outside the block are not part of the rank's factor
      const int c = ci[p] - r0;
      if (c < 0 || c >= nb) lu[p] = 0.0;
    }
#pragma unroll 4
    for (int e = tid; e < nzb; e += ILU_WAVES * 64) {
      const int p = cpos[c0 + e];
      lvn[e] = a[p];
      lcn[e] = (uint16_t)(ci[p] - r0);
    }
  }
  __syncthreads();
  volatile uint16_t *pos = posv + wave * mr;
  for (int l = 0; l < nlev; ++l) {
    const int a1 = lvp[l + 1];
    for (int r = lvp[l] + wave; r < a1; r += ILU_WAVES) {
      const int i = llv[r];
      const int s0 = lrp[i], s1 = lrp[i + 1], dg = ldg[i];
      for (int e = s0 + lane; e < s1; e += 64) pos[lc[e]] = (uint16_t)e;
      __builtin_amdgcn_wave_barrier();
      // L part, ascending columns (wave-uniform loop).  Everything an entry needs except its own multiplier is a constant of the
      // pattern or belongs to a finished row -- pivot, its diagonal, this lane's entry of its scaled U row and where that lands in
      // row i -- and is requested one entry ahead: the dependent chain per L entry is multiplier -> update, two LDS trips.
      struct Ahead {
        int ue, q;
        uint16_t pc;
        double uq, dinvk;
      };
      auto ahead = [&](int e) {
        Ahead n;
        const int k = lc[e], dk = ldg[k];
        n.ue = lrp[k + 1];
        n.q = dk + 1 + lane;
        const bool has = n.q < n.ue;
        n.pc = has ? pos[lc[has ? n.q : dk]] : ILU_NOPOS;
        n.uq = lv[has ? n.q : dk];
        n.dinvk = lv[dk];
        return n;
      };
      Ahead cur = ahead(s0 < dg ? s0 : dg);
      for (int e = s0; e < dg; ++e) {
        const Ahead nxt = ahead(e + 1 < dg ? e + 1 : dg);  // (a dummy request behind the last entry: row i's own diagonal)
        const double mult = lv[e];
        if (lane == 0) lv[e] = mult * cur.dinvk;  // InV[jj] *= DV[j]
        if (cur.pc != ILU_NOPOS) lv[cur.pc] -= mult * cur.uq;
        for (int q = cur.q + 64; q < cur.ue; q += 64) {  // scaled U rows of more than 64 entries
          const uint16_t pc = pos[lc[q]];
          if (pc != ILU_NOPOS) lv[pc] -= mult * lv[q];
        }
        cur = nxt;
      }
      __builtin_amdgcn_wave_barrier();
      const double d = lv[dg];
      const double dinv = 1.0 / d;
      if (lane == 0 && !(fabs(d) > 0.0)) __hip_atomic_store(err, 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __builtin_amdgcn_wave_barrier();
      for (int e = dg + lane; e < s1; e += 64) lv[e] = e == dg ? dinv : lv[e] * dinv;
      for (int e = s0 + lane; e < s1; e += 64) pos[lc[e]] = ILU_NOPOS;
      __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
  }
  {
    const double *lvn = lds_f;
#pragma unroll 4
    for (int e = tid; e < nzb; e += ILU_WAVES * 64) {
      const int p = cpos[c0 + e];
      const double v = lvn[e];
      lu[p] = v;
      if (slot_of) {
        const int sl = slot_of[p];
        if (sl >= 0) pk_store(pk_val, pk_val32, sl, -v, err);  // the stream adds value * x[col]: it stores -L and -U/d
      }
    }
    if (slot_of)
      for (int q = tid; q < nb; q += ILU_WAVES * 64) pk_dinv[dinv_slot[r0 + q]] = lvn[ldg[q]];
  }
}

// ---- levelled path (IluSchedule::levelled): blocks of any size, one launch per dependency level ------------------------
// Factorisation: one wave per row of the level, same row arithmetic as k_ilu_factor (sorted-column binary search in global
// memory); rows of earlier levels are complete because the previous launch has finished.
__global__ __launch_bounds__(ILU_WAVES * 64) void k_ilu_factor_level(int n_lvl_rows, const int32_t *__restrict__ rows,
                                                                    const int32_t *__restrict__ in_lo, const int32_t *__restrict__ in_hi,
                                                                    const int32_t *__restrict__ rp, const int32_t *__restrict__ ci,
                                                                    const int32_t *__restrict__ diag, const double *__restrict__ a,
                                                                    double *lu, int *__restrict__ err) {
  __shared__ double wv[ILU_WAVES][ILU_MAXROW];
  const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
  const int r = blockIdx.x * ILU_WAVES + wave;
  if (r >= n_lvl_rows) return;  // whole waves exit; no workgroup barrier below
  const int i = rows[r];
  volatile double *w = wv[wave];
  const int p0 = rp[i], n = rp[i + 1] - p0, dpos = diag[i] - p0, lo = in_lo[i] - p0, hi = in_hi[i] - p0;
  if (n > ILU_MAXROW) {
    if (lane == 0) __hip_atomic_store(err, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    return;
  }
  for (int t = lane; t < n; t += 64) w[t] = (t >= lo && t < hi) ? a[p0 + t] : 0.0;
  __builtin_amdgcn_wave_barrier();
  for (int t = lo; t < dpos; ++t) {  // L part, ascending columns (wave-uniform loop)
    const int j = ci[p0 + t];
    const int dj = diag[j];
    const double mult = w[t];
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) w[t] = mult * lu[dj];  // InV[jj] *= DV[j]
    const int ue = in_hi[j];
    for (int q = dj + 1 + lane; q < ue; q += 64) {  // scaled U row of j
      const int c = ci[q];
      int l2 = t + 1, h2 = hi - 1;  // columns of row i are sorted; c > j
      while (l2 <= h2) {
        const int mid = (l2 + h2) >> 1, cm = ci[p0 + mid];
        if (cm < c) l2 = mid + 1; else if (cm > c) h2 = mid - 1; else { w[mid] -= mult * lu[q]; break; }
      }
    }
    __builtin_amdgcn_wave_barrier();
  }
  const double d = w[dpos];
  const double dinv = 1.0 / d;
  if (lane == 0 && !(fabs(d) > 0.0)) __hip_atomic_store(err, 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  for (int t = lane; t < n; t += 64) {
    double v = w[t];
    if (t == dpos) v = dinv;
    else if (t > dpos) v = t < hi ? v * dinv : 0.0;
    lu[p0 + t] = v;
  }
}

// Solve: LW lanes per row of the level, x in global memory (in place: x holds b on entry of the forward sweep).
// forward:  x_i -= sum_{j<i in block} L_ij x_j ;  backward: x_i = x_i / d_i - sum_{j>i in block} (U_ij/d_i) x_j
// (the D^-1 scaling of Ifpack's ApplyInverse is folded into the backward visit of each row: its x_j are final by then)
template <int NCOMP, int LW, bool FWD>
__global__ __launch_bounds__(256) void k_ilu_solve_level(int n_lvl_rows, const int4 *__restrict__ rec, const int32_t *__restrict__ ci,
                                                         const double *__restrict__ lu, double *x) {
  const int r = (blockIdx.x * 256 + threadIdx.x) / LW, lane = threadIdx.x % LW;
  if (r >= n_lvl_rows) return;
  const int4 q = rec[r];  // row, first entry, end of entries, diagonal: one trip (the records of a level are contiguous)
  const int i = q.x, pb = q.y, pe = q.z;
  // requested with the entries, not behind the reduction: the row's own value and (backward) its 1 / d
  double xi0[NCOMP];
  double *xi = x + (size_t)i * NCOMP;
  double dinv = 1.0;
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < NCOMP; ++c) xi0[c] = xi[c];
    if (!FWD) dinv = lu[q.w];
  }
  double acc[NCOMP];
#pragma unroll
  for (int c = 0; c < NCOMP; ++c) acc[c] = 0.0;
  for (int p = pb + lane; p < pe; p += LW) {
    const double l = lu[p];
    const double *xj = x + (size_t)ci[p] * NCOMP;
#pragma unroll
    for (int c = 0; c < NCOMP; ++c) acc[c] += l * xj[c];
  }
#pragma unroll
  for (int c = 0; c < NCOMP; ++c) acc[c] = lane_group_sum<LW>(acc[c]);
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < NCOMP; ++c) xi[c] = FWD ? xi0[c] - acc[c] : xi0[c] * dinv - acc[c];
  }
}

template <int NCOMP>
static void ilu_solve_levelled(nsx_handle *h, const DevCsr &g, const IluSchedule &s, const double *lu, const double *b, double *x) {
  constexpr int LW = 8;
  v_copy(h, g.n_rows() * NCOMP, x, b);
  const int nf = (int)s.gl_f_ptr_h.size() - 1, nbk = (int)s.gl_b_ptr_h.size() - 1;
  for (int l = 1; l < nf; ++l) {  // level 0 of the forward sweep has no in-block L entries: y = b there
    const int n = s.gl_f_ptr_h[l + 1] - s.gl_f_ptr_h[l];
    if (n > 0)
      hipLaunchKernelGGL((k_ilu_solve_level<NCOMP, LW, true>), dim3(cdiv((int64_t)n * LW, 256)), dim3(256), 0, h->stream, n,
                         reinterpret_cast<const int4 *>(s.gl_f_rec.p) + s.gl_f_ptr_h[l], g.colind.p, lu, x);
  }
  for (int l = 0; l < nbk; ++l) {
    const int n = s.gl_b_ptr_h[l + 1] - s.gl_b_ptr_h[l];
    if (n > 0)
      hipLaunchKernelGGL((k_ilu_solve_level<NCOMP, LW, false>), dim3(cdiv((int64_t)n * LW, 256)), dim3(256), 0, h->stream, n,
                         reinterpret_cast<const int4 *>(s.gl_b_rec.p) + s.gl_b_ptr_h[l], g.colind.p, lu, x);
  }
}

// The factorisation kernels report a failure (row too long, zero pivot) through a word in mapped host memory, written only
// when something is wrong; ilu_check() looks at it after the caller's next synchronisation (no stream sync, no copy here).
void ilu_check(nsx_handle *h) {
  volatile int *err = pub_word_host(h, PUB_ILU_ERR);
  const int herr = *err;
  if (!herr) return;
  *err = 0;
  if (herr == 1) NSX_THROW(NSX_ERR_UNSUPPORTED, "ILU: a row has more than %d entries", ILU_MAXROW);
  if (herr == 3) NSX_THROW(NSX_ERR_HIP, "ILU: the lane-owner triangular solve found its LDS array away from address 0 and did not run (internal: a static __shared__ object in k_ilu_solve_lanes?)");
  if (herr == 4) NSX_THROW(NSX_ERR_NUMERIC, "inner precision FP32: an entry of F is not finite as a float (beyond 3.4e38, or NaN)");
  if (herr == 5) NSX_THROW(NSX_ERR_NUMERIC, "inner precision FP32: an entry of the ILU(0) factors of F is not finite as a float (beyond 3.4e38, or NaN)");
  NSX_THROW(NSX_ERR_NUMERIC, "ILU: zero pivot");
}

// f32: write the off-diagonal entries into the FLOAT solve stream (pk_val32) instead of the double one -- only where the solve will
// read the lane-owner stream (ilu_lanes_stream, the predicate ilu_solve uses); lu itself always holds the double factors
void ilu_factor(nsx_handle *h, const DevCsr &g, IluSchedule &s, const double *vals, double *lu, const char *name, bool f32) {
  int *err = pub_word_dev(h, PUB_ILU_ERR);
  float *pk32 = nullptr;
  if (f32 && ilu_lanes_stream(s, s.stream_ncomp)) {
    if (s.pk_val32.n != s.pk_val.n || !s.pk_val32.p) {  // (released whenever the schedule is rebuilt: unused slots must read 0)
      s.pk_val32.alloc(s.pk_val.n);
      s.pk_val32.zero(h->stream);
    }
    pk32 = s.pk_val32.p;
  }
  s.stream_f32 = pk32 != nullptr;
  {
    LaunchScope ls(h, name, 20.0 * g.nnz() + 12.0 * g.n_rows());
    const bool small_ok = env_on("NSX_ILU_SMALL");  // read per call, like its neighbours
    const bool lds_ok = env_on("NSX_ILU_FACTOR_LDS");  // read per call: the tests switch it
    s.path.factor_lds_bytes = 0;
    if (s.levelled) {
      s.path.factor = NSX_ILU_FACTOR_LEVEL;
      for (size_t l = 0; l + 1 < s.gl_f_ptr_h.size(); ++l) {
        const int n = s.gl_f_ptr_h[l + 1] - s.gl_f_ptr_h[l];
        if (n > 0)
          hipLaunchKernelGGL(k_ilu_factor_level, dim3(cdiv(n, ILU_WAVES)), dim3(ILU_WAVES * 64), 0, h->stream, n, s.gl_f_rows.p + s.gl_f_ptr_h[l],
                             s.in_lo.p, s.in_hi.p, g.rowptr.p, g.colind.p, g.diag.p, vals, lu, err);
      }
    } else if (lds_ok && s.max_rows <= 4096 && s.max_block_nnz < 65535 && ilu_factor_lds_bytes(s.max_rows, s.max_block_nnz) <= 80 * 1024) {
      // the whole block in LDS: at most 80 KB, so that at least two workgroups share a CU
      const size_t lds = ilu_factor_lds_bytes(s.max_rows, s.max_block_nnz);
      s.path.factor = NSX_ILU_FACTOR_LDS;
      s.path.factor_lds_bytes = (int)lds;
      static std::atomic<size_t> lds_allowed{64 * 1024};  // per process: the attribute belongs to the function, not to a handle
      if (lds > lds_allowed.load()) {
        HIP_CHECK(hipFuncSetAttribute((const void *)k_ilu_factor_lds, hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024));
        lds_allowed.store(80 * 1024);
      }
      hipLaunchKernelGGL(k_ilu_factor_lds, dim3(s.n_blocks), dim3(ILU_WAVES * 64), lds, h->stream, s.fac_order.p, s.block_ptr.p, s.blk_lvl_off.p, s.fwd_lvl_ptr.p,
                         s.fwd_rows.p, g.rowptr.p, g.colind.p, g.diag.p, s.in_lo.p, s.in_cptr.p, s.in_cpos.p, vals, lu,
                         s.packed_ok ? s.pk_slot_of.p : nullptr, s.pk_val.p, s.pk_dinv.p, err, s.pk_dinv_slot.p, s.max_rows, (int)s.max_block_nnz, pk32);
    } else if (small_ok && s.max_rows <= ILU_DENSE_ROWS) {
      s.path.factor = NSX_ILU_FACTOR_DENSE_ROW;
      hipLaunchKernelGGL(k_ilu_factor_small, dim3(s.n_blocks), dim3(ILU_WAVES * 64), 0, h->stream, s.block_ptr.p, s.blk_lvl_off.p,
                         s.fwd_lvl_ptr.p, s.fwd_rows.p, g.rowptr.p, g.colind.p, g.diag.p, vals, lu, s.packed_ok ? s.pk_slot_of.p : nullptr,
                         s.pk_val.p, s.pk_dinv.p, err, s.pk_dinv_slot.p, pk32);
    } else {
      s.path.factor = NSX_ILU_FACTOR_GENERAL;
      hipLaunchKernelGGL(k_ilu_factor, dim3(s.n_blocks), dim3(ILU_WAVES * 64), 0, h->stream, s.block_ptr.p, s.blk_lvl_off.p, s.fwd_lvl_ptr.p,
                         s.fwd_rows.p, g.rowptr.p, g.colind.p, g.diag.p, vals, lu, s.packed_ok ? s.pk_slot_of.p : nullptr, s.pk_val.p,
                         s.pk_dinv.p, err, s.pk_dinv_slot.p, pk32);
    }
  }
  s.path.invert = NSX_ILU_INVERT_NONE;
  if (s.dense) {
    LaunchScope ls(h, "ilu_invert", 8.0 * (double)s.dn_entries + 12.0 * g.nnz());
    // blocks of up to 112 rows (98 KB of LDS: one workgroup per CU and half) keep the n x n matrix in LDS while it is built
    const bool inv_lds = env_on("NSX_ILU_INVERT_LDS");  // read per call: the tests switch it inside one process
    const size_t shm = (size_t)s.max_rows * s.max_rows * sizeof(double);
    s.path.invert_staged = false;
    if (inv_lds && s.max_rows <= 112) {
      // the factor's in-block entries beside the matrix (NSX_ILU_INVERT_STAGE, read per call) where both fit the device's opt-in limit: a
      // dense 112-row block does not (98 KB + 125 KB), the flagship's 96-row blocks of the Schur graph do
      // (NSX_LDS_OPTIN, read per call: a lower limit than the device's, so that the tests reach the fallback on the graphs of real meshes)
      const size_t staged = ilu_invert_stage_bytes(s.max_rows, s.max_block_nnz);
      const size_t limit = (size_t)std::max<int64_t>(0, std::min<int64_t>(h->lds_optin, env_i64("NSX_LDS_OPTIN", h->lds_optin)));
      const bool stage = env_on("NSX_ILU_INVERT_STAGE") && s.max_block_nnz < 65535 && staged + ILU_INVERT_STATIC_LDS <= limit;
      const size_t lds = stage ? staged : shm;
      const void *fn = stage ? (const void *)k_ilu_invert_lds<true> : (const void *)k_ilu_invert_lds<false>;
      // the attribute belongs to the function on the current device: set whenever the launch needs it (a repeated call costs microseconds)
      if (lds > 64 * 1024) HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)std::max(lds, (size_t)112 * 112 * sizeof(double))));
      s.path.invert = NSX_ILU_INVERT_LDS;
      s.path.invert_staged = stage;
      if (stage)
        hipLaunchKernelGGL(k_ilu_invert_lds<true>, dim3(s.n_blocks), dim3(128), lds, h->stream, s.block_ptr.p, s.dn_off.p, g.rowptr.p, g.colind.p, g.diag.p, lu,
                           s.dn_P.p, s.in_lo.p, s.in_cptr.p, s.in_cpos.p);
      else
        hipLaunchKernelGGL(k_ilu_invert_lds<false>, dim3(s.n_blocks), dim3(128), lds, h->stream, s.block_ptr.p, s.dn_off.p, g.rowptr.p, g.colind.p, g.diag.p, lu,
                           s.dn_P.p, s.in_lo.p, s.in_cptr.p, s.in_cpos.p);
    } else {
      s.path.invert = NSX_ILU_INVERT_GLOBAL;
      hipLaunchKernelGGL(k_ilu_invert, dim3(s.n_blocks), dim3(256), 0, h->stream, s.block_ptr.p, s.dn_off.p, g.rowptr.p, g.colind.p, g.diag.p, lu,
                         s.dn_P.p);
    }
  }
}

// x = U^{-1} D^{-1} L^{-1} b per block (Ifpack_ILU::ApplyInverse), NCOMP right-hand sides interleaved.
// LW lanes cooperate on one row; the block's part of x lives in LDS when it fits (USE_LDS), else in x itself.
template <int NCOMP, int LW, bool USE_LDS>
__global__ __launch_bounds__(256) void k_ilu_solve(const int32_t *__restrict__ bptr, const int32_t *__restrict__ offF,
                                                   const int32_t *__restrict__ ptrF, const int32_t *__restrict__ rowsF,
                                                   const int32_t *__restrict__ offB, const int32_t *__restrict__ ptrB,
                                                   const int32_t *__restrict__ rowsB, const int32_t *__restrict__ rp,
                                                   const int32_t *__restrict__ ci, const int32_t *__restrict__ diag,
                                                   const double *__restrict__ lu, const double *__restrict__ b, double *__restrict__ x) {
  extern __shared__ double xs_[];
  const int blk = blockIdx.x;
  const int r0 = bptr[blk], r1 = bptr[blk + 1], nloc = r1 - r0;
  double *xs = USE_LDS ? xs_ : x + (size_t)r0 * NCOMP;
  for (int t = threadIdx.x; t < nloc * NCOMP; t += 256) xs[t] = b[(size_t)r0 * NCOMP + t];
  __syncthreads();
  const int grp = threadIdx.x / LW, lane = threadIdx.x % LW, ngrp = 256 / LW;
  for (int lv = offF[blk]; lv < offF[blk + 1]; ++lv) {  // forward: y_i = b_i - sum_{j<i} L_ij y_j
    const int l0 = ptrF[lv], cnt = ptrF[lv + 1] - l0;
    for (int r = grp; r < cnt; r += ngrp) {
      const int i = rowsF[l0 + r];
      double acc[NCOMP];
#pragma unroll
      for (int c = 0; c < NCOMP; ++c) acc[c] = 0.0;
      const int e = diag[i];
      for (int p = rp[i] + lane; p < e; p += LW) {
        const int j = ci[p];
        if (j >= r0) {
          const double l = lu[p];
#pragma unroll
          for (int c = 0; c < NCOMP; ++c) acc[c] += l * xs[(j - r0) * NCOMP + c];
        }
      }
#pragma unroll
      for (int c = 0; c < NCOMP; ++c) acc[c] = lane_group_sum<LW>(acc[c]);
      if (lane == 0) {
#pragma unroll
        for (int c = 0; c < NCOMP; ++c) xs[(i - r0) * NCOMP + c] -= acc[c];
      }
    }
    __syncthreads();
  }
  for (int t = threadIdx.x; t < nloc; t += 256) {  // y *= D^{-1}
    const double dinv = lu[diag[r0 + t]];
#pragma unroll
    for (int c = 0; c < NCOMP; ++c) xs[t * NCOMP + c] *= dinv;
  }
  __syncthreads();
  for (int lv = offB[blk]; lv < offB[blk + 1]; ++lv) {  // backward: x_i = y_i - sum_{j>i} U_ij x_j
    const int l0 = ptrB[lv], cnt = ptrB[lv + 1] - l0;
    for (int r = grp; r < cnt; r += ngrp) {
      const int i = rowsB[l0 + r];
      double acc[NCOMP];
#pragma unroll
      for (int c = 0; c < NCOMP; ++c) acc[c] = 0.0;
      const int e = rp[i + 1];
      for (int p = diag[i] + 1 + lane; p < e; p += LW) {
        const int j = ci[p];
        if (j < r1) {
          const double u = lu[p];
#pragma unroll
          for (int c = 0; c < NCOMP; ++c) acc[c] += u * xs[(j - r0) * NCOMP + c];
        }
      }
#pragma unroll
      for (int c = 0; c < NCOMP; ++c) acc[c] = lane_group_sum<LW>(acc[c]);
      if (lane == 0) {
#pragma unroll
        for (int c = 0; c < NCOMP; ++c) xs[(i - r0) * NCOMP + c] -= acc[c];
      }
    }
    __syncthreads();
  }
  if (USE_LDS)
    for (int t = threadIdx.x; t < nloc * NCOMP; t += 256) x[(size_t)r0 * NCOMP + t] = xs[t];
}

// ---- lane-owner stream: device side in nsx_ilu_lanes.hpp (shared with tools/ilu_lanes_bench.hip), schedule in host/ilu_stream.hpp
constexpr int LANES_K = 12;  // rows per lane and memory trip in the load / scale / store passes of k_ilu_solve_lanes (768 rows: one trip for a wave of 8 blocks)

// VT: the type the stream stores its off-diagonal values in (double: k_ilu_solve_lanes; float: k_ilu_solve_lanes_f32, a handle in
// NSX_INNER_FP32 -- same slots, same meta words, same ticks, half the value bytes; the inverse pivots stay double)
template <int NCOMP, int E, int PF, class VT>
__device__ __forceinline__ void ilu_solve_lanes_wave(const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ rows,
                                                     const int32_t *__restrict__ slab_ptr, const uint32_t *__restrict__ meta,
                                                     const VT *__restrict__ val, const double *__restrict__ dinv, const double *b, double *x,
                                                     double *__restrict__ dot_partial, int *err_host, int force_guard) {
  extern __shared__ double xs[];  // the only LDS of this kernel: the stream's addresses are absolute (nsx_ilu_lanes.hpp)
  // The stream's 16-bit fields are absolute LDS byte addresses: the dynamic array must start at address 0, i.e. the kernel (and
  // every helper inlined into it) must own no static __shared__ object.  Should that ever change, x is NOT written -- so the word
  // ilu_check() reads is raised (code 3) and the API call that ran this solve fails instead of handing back stale memory
  // (force_guard: NSX_ILU_LDS_GUARD_TEST, tests/test_gpu_errors.py).
  if ((uint32_t)(uintptr_t)(lds_f64 *)xs != 0u || force_guard) {
    if (threadIdx.x == 0) __hip_atomic_store(err_host, 3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    return;
  }
  const int w = blockIdx.x;
  const unsigned lane = threadIdx.x;
  const int s0 = slab_ptr[2 * w], s1 = slab_ptr[2 * w + 1], s2 = slab_ptr[2 * w + 2];
  const int rb = row_ptr[w], nr = row_ptr[w + 1] - rb;
  // The wave is alone on its SIMD: nothing hides a trip to memory but the wave's own other requests.  So everything whose address
  // is known at once is requested at once, in front of everything else: the first slabs of the forward sweep, the row ids and the
  // inverse pivots of the wave's first 64 * LANES_K rows (both kept in registers to the end: the scaling between the sweeps and
  // the store at the end then need no further trip); then the right-hand side (one dependent trip).  Waves with more rows go
  // through the same three passes chunk by chunk for the rest.
  constexpr int K = LANES_K;
  LaneSlot<E, VT> A[PF];
  lane_load<E, PF, VT>(A, s0, meta, val, lane);
  int idx0[K];
  double d0[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int t = 64 * k + (int)lane;
    idx0[k] = t < nr ? rows[rb + t] : -1;
    d0[k] = t < nr ? dinv[rb + t] : 0.0;
  }
  {
    double v[K][NCOMP];
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
      for (int c = 0; c < NCOMP; ++c) v[k][c] = idx0[k] >= 0 ? b[(size_t)idx0[k] * NCOMP + c] : 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k)
      if (idx0[k] >= 0) {
#pragma unroll
        for (int c = 0; c < NCOMP; ++c) xs[(64 * k + (int)lane) * NCOMP + c] = v[k][c];
      }
  }
  for (int base = 64 * K; base < nr; base += 64 * K) {
    int idx[K];
    double v[K][NCOMP];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int t = base + 64 * k + (int)lane;
      idx[k] = t < nr ? rows[rb + t] : -1;
    }
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
      for (int c = 0; c < NCOMP; ++c) v[k][c] = idx[k] >= 0 ? b[(size_t)idx[k] * NCOMP + c] : 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k)
      if (idx[k] >= 0) {
#pragma unroll
        for (int c = 0; c < NCOMP; ++c) xs[(base + 64 * k + (int)lane) * NCOMP + c] = v[k][c];
      }
  }
#pragma unroll
  for (int c = 0; c < NCOMP; ++c) xs[(nr + lane) * NCOMP + c] = 0.0;  // the scratch rows of the idle slots
  const uint32_t scratch = (uint32_t)(nr + lane) * (8u * NCOMP);
  __builtin_amdgcn_wave_barrier();
  lane_sweep<NCOMP, E, PF, VT>(A, s0, s1, meta, val, lane, scratch);  // y = L^{-1} b
  lane_load<E, PF, VT>(A, s1, meta, val, lane);                       // (the backward sweep's first slabs fly during the scaling)
#pragma unroll
  for (int k = 0; k < K; ++k) {                                   // y *= D^{-1} (inverse pivots stored in the wave's row order)
    const int t = 64 * k + (int)lane;
    if (t < nr) {
#pragma unroll
      for (int c = 0; c < NCOMP; ++c) xs[t * NCOMP + c] *= d0[k];
    }
  }
  for (int base = 64 * K; base < nr; base += 64 * K) {
    double d[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int t = base + 64 * k + (int)lane;
      d[k] = t < nr ? dinv[rb + t] : 0.0;
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int t = base + 64 * k + (int)lane;
      if (t < nr) {
#pragma unroll
        for (int c = 0; c < NCOMP; ++c) xs[t * NCOMP + c] *= d[k];
      }
    }
  }
  __builtin_amdgcn_wave_barrier();
  lane_sweep<NCOMP, E, PF, VT>(A, s1, s2, meta, val, lane, scratch);  // x = U^{-1} y
  double dot = 0.0;  // b . x over this wave's rows (CG's g.h right after the preconditioner, Prec.hpp:388 / SolverCG)
  for (int base = 0; base < nr; base += 64 * K) {
    int idx[K];
    double bv[K][NCOMP];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int t = base + 64 * k + (int)lane;
      idx[k] = base == 0 ? idx0[k] : (t < nr ? rows[rb + t] : -1);
    }
    if (dot_partial) {
#pragma unroll
      for (int k = 0; k < K; ++k)
#pragma unroll
        for (int c = 0; c < NCOMP; ++c) bv[k][c] = idx[k] >= 0 ? b[(size_t)idx[k] * NCOMP + c] : 0.0;
    }
#pragma unroll
    for (int k = 0; k < K; ++k)
      if (idx[k] >= 0) {
#pragma unroll
        for (int c = 0; c < NCOMP; ++c) {
          const double xv = xs[(base + 64 * k + (int)lane) * NCOMP + c];
          if (dot_partial) dot += bv[k][c] * xv;
          x[(size_t)idx[k] * NCOMP + c] = xv;
        }
      }
  }
  if (dot_partial) {
    dot = lane_group_sum<64>(dot);
    if (lane == 0) dot_partial[w] = dot;
  }
}

template <int NCOMP, int E, int PF>
__global__ __launch_bounds__(64) void k_ilu_solve_lanes(const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ rows,
                                                        const int32_t *__restrict__ slab_ptr, const uint32_t *__restrict__ meta,
                                                        const double *__restrict__ val, const double *__restrict__ dinv, const double *b, double *x,
                                                        double *__restrict__ dot_partial, int *err_host, int force_guard) {
  ilu_solve_lanes_wave<NCOMP, E, PF, double>(row_ptr, rows, slab_ptr, meta, val, dinv, b, x, dot_partial, err_host, force_guard);
}
template <int NCOMP, int E, int PF>
__global__ __launch_bounds__(64) void k_ilu_solve_lanes_f32(const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ rows,
                                                            const int32_t *__restrict__ slab_ptr, const uint32_t *__restrict__ meta,
                                                            const float *__restrict__ val, const double *__restrict__ dinv, const double *b, double *x,
                                                            double *__restrict__ dot_partial, int *err_host, int force_guard) {
  ilu_solve_lanes_wave<NCOMP, E, PF, float>(row_ptr, rows, slab_ptr, meta, val, dinv, b, x, dot_partial, err_host, force_guard);
}

// the interleaved right-hand sides of a solve as a compile-time constant: 1 (the Schur complement) or dim (the velocity block)
template <class F>
static void with_ncomp(int ncomp, F &&f) {
  if (!with_int<1, 2, 3>(ncomp, f)) NSX_THROW(NSX_ERR_ARG, "internal: %d interleaved right-hand sides", ncomp);
}

template <int NCOMP>
static void launch_lanes(nsx_handle *h, const IluSchedule &s, const double *b, double *x, double *dot_partial, bool f32) {
  const size_t shm = (size_t)(s.max_wave_rows + 64) * NCOMP * sizeof(double);
  const int pf = ilu_lanes_pf();  // read per launch, like NSX_ILU_LDS_GUARD_TEST below (the fused launch of nsx_mgs.hip asks the same function)
  s.path.solve_pf = pf;
  int *err = pub_word_dev(h, PUB_ILU_ERR);  // the mapped word ilu_check() reads
  const int force_guard = env_int("NSX_ILU_LDS_GUARD_TEST", 0);  // fault injection (tests), read per launch
  const bool known = with_int<1, 2, 3, 4>(s.stream_epl, [&](auto E_) {
    with_int<4, 8>(pf, [&](auto PF_) {
      constexpr int E = decltype(E_)::value, PF = decltype(PF_)::value;
      auto go = [&](auto kernel, const auto *val) {
        hipLaunchKernelGGL(kernel, dim3(s.n_waves), dim3(64), shm, h->stream, s.pk_row_ptr.p, s.pk_rows.p, s.pk_slab_ptr.p,
                           reinterpret_cast<const uint32_t *>(s.pk_meta.p), val, s.pk_dinv.p, b, x, dot_partial, err, force_guard);
      };
      if (f32) go(k_ilu_solve_lanes_f32<NCOMP, E, PF>, s.pk_val32.p);
      else go(k_ilu_solve_lanes<NCOMP, E, PF>, s.pk_val.p);
    });
  });
  if (!known) NSX_THROW(NSX_ERR_ARG, "internal: %d entries per tick", s.stream_epl);
}

template <int NCOMP>
static void launch_ilu_solve(nsx_handle *h, const DevCsr &g, const IluSchedule &s, const double *lu, const double *b, double *x) {
  const size_t shm = (size_t)s.max_rows * NCOMP * sizeof(double);
  constexpr int LW = 8;
  const bool lds = shm <= 64 * 1024;
  s.path.solve = lds ? NSX_ILU_SOLVE_BLOCK_LDS : NSX_ILU_SOLVE_BLOCK_GLOBAL;
  auto go = [&](auto kernel, size_t dyn) {
    hipLaunchKernelGGL(kernel, dim3(s.n_blocks), dim3(256), dyn, h->stream, s.block_ptr.p, s.blk_lvl_off.p, s.fwd_lvl_ptr.p, s.fwd_rows.p, s.blk_lvl_off_b.p,
                       s.bwd_lvl_ptr.p, s.bwd_rows.p, g.rowptr.p, g.colind.p, g.diag.p, lu, b, x);
  };
  if (lds) go(k_ilu_solve<NCOMP, LW, true>, shm);
  else go(k_ilu_solve<NCOMP, LW, false>, 0);
}

// f32: read the float solve stream where the last factorisation wrote one (IluSchedule::stream_f32); every other path reads the double
// factors and *used_f32 (optional) says which it was
bool ilu_solve(nsx_handle *h, const DevCsr &g, const IluSchedule &s, const double *lu, const double *b, double *x, int ncomp,
               const char *name, int dot_slot, bool f32, int *used_f32) {
  if (used_f32) *used_f32 = 0;
  s.path.solve_ncomp = ncomp;
  s.path.solve_pf = s.path.solve_f32 = 0;
  if (s.levelled) {
    s.path.solve = NSX_ILU_SOLVE_LEVELLED;
    LaunchScope ls(h, name, 12.0 * (double)s.in_block_nnz + (double)g.n_rows() * (4 + 16.0 * ncomp));
    with_ncomp(ncomp, [&](auto N) { ilu_solve_levelled<decltype(N)::value>(h, g, s, lu, b, x); });
    return false;
  }
  const bool packed = ilu_lanes_stream(s, ncomp);  // (the schedule already checked that a wave's rows fit 64 KiB of LDS)
  if (s.dense && ncomp == 1 && (size_t)s.max_rows * sizeof(double) <= 48 * 1024) {
    LaunchScope ls(h, name, 8.0 * (double)s.dn_entries + 16.0 * g.n_rows());
    s.path.solve = NSX_ILU_SOLVE_DENSE;
    const bool with_dot = dot_slot >= 0 && !h->comm && s.n_blocks >= 2 && s.n_blocks <= 512;  // a communicator needs equal counts on all ranks
    hipLaunchKernelGGL(k_ilu_apply_dense, dim3(s.n_blocks), dim3(DENSE_THREADS), (size_t)s.max_rows * sizeof(double), h->stream, s.block_ptr.p, s.dn_off.p,
                       s.dn_P.p, b, x, with_dot ? red_out(h, dot_slot, s.n_blocks) : nullptr);
    if (with_dot) after_reduction(h, dot_slot, s.n_blocks);
    return with_dot;
  }
  // algorithmic bytes (nnz(L+U) * 12 + n * (4 + 8 + 8) per component set): what ONE application of a per-rank ILU(0)
  // has to read -- the IN-BLOCK entries of the factor (diagonal included; couplings between ranks are dropped by Ifpack's
  // local filter and are never touched) + right-hand side and solution.  The packed stream itself moves 768 B per slab.
  const bool lanes32 = packed && f32 && s.stream_f32;
  if (packed && s.stream_f32 && !lanes32) NSX_THROW(NSX_ERR_ARG, "internal: the double solve stream is stale (the last factorisation wrote the float stream)");
  // (float stream: the off-diagonal entries cost 4 + 4 bytes, the inverse pivots stay 8 + 4)
  LaunchScope ls(h, name, 12.0 * (double)s.in_block_nnz - (lanes32 ? 4.0 * (double)(s.in_block_nnz - g.n_rows()) : 0.0) + (double)g.n_rows() * (4 + 16.0 * ncomp));
  if (packed) {
    if (used_f32) *used_f32 = lanes32 ? 1 : 0;
    s.path.solve = NSX_ILU_SOLVE_LANES;
    s.path.solve_f32 = lanes32 ? 1 : 0;
    const bool with_dot = dot_slot >= 0 && !h->comm && s.n_waves >= 2 && s.n_waves <= 512;  // one partial sum per wave
    double *dp = with_dot ? red_out(h, dot_slot, s.n_waves) : nullptr;
    with_ncomp(ncomp, [&](auto N) { launch_lanes<decltype(N)::value>(h, s, b, x, dp, lanes32); });
    if (with_dot) after_reduction(h, dot_slot, s.n_waves);
    return with_dot;
  }
  with_ncomp(ncomp, [&](auto N) { launch_ilu_solve<decltype(N)::value>(h, g, s, lu, b, x); });
  return false;
}

}  // namespace nsx
