// nsx_mgs.hip — the modified Gram-Schmidt sweep of the GMRES drivers (deal.II's SolverGMRES orthogonalisation of the new Krylov
// vector against the basis): the persistent kernels (k_mgs_one, k_ilu_mgs), the two-pass distributed sweep
// (k_ls_*, mgs_lowsync), their set-up, their recovery after a time-out, and the host driver v_mgs that chooses among them.
// The launch-per-link chain it falls back to is made of the BLAS-1 reductions of nsx_blas.hip.
#include "nsx_grid.hpp"
#include "nsx_ilu_lanes.hpp"

namespace nsx {

// ---- modified Gram-Schmidt sweep in ONE persistent launch -----------------------------------------------------------
// deal.II's SolverGMRES orthogonalises the new Krylov vector w with the chain  h(0) = w.v_0 ;
// h(i+1) = w.add_and_dot(-h(i), v_i, v_{i+1}) ; |w|^2 = w.add_and_dot(-h(dim-1), v_{dim-1}, w): dim+1 dependent global
// reductions.  As separate launches every link streams w (read + write) and two basis vectors, 32 B per entry; here the
// grid is co-resident, every thread keeps its entries of w and of the newest basis vectors in registers for the whole sweep,
// every basis vector is read once (8 B per entry; the oldest ones twice when the block does not fit), and ALL links share one
// grid-wide exchange of partial sums (nsx_grid.hpp: mailboxes, no atomics on shared counters; the algebra is at k_mgs_one).
// The arithmetic of each entry is that of the chain (w += (-h) v_i), sums are fixed-order, so results do not depend on
// timing.  Every wait is bounded by a wall-clock timeout: a grid that is not co-resident (another stream or process holds
// compute units) ends without touching w, and the host falls back to the launch-per-link chain (v_mgs).
constexpr int MGS_MAX_WG = 512;
constexpr int MGS_STEPS = 32;     // basis pointers of one sweep; a sweep against dim vectors is taken for dim + 2 <= MGS_STEPS
static_assert(MGS_STEPS >= KRYLOV_N_TMP + 2, "a sweep against dim vectors needs dim + 2 rows");
// Mailbox region of one sweep (h->mgs.box holds two, used in turn): the single exchange carries r_j and g_j (j < MGS_STEPS - 2),
// |w|^2 before the sweep and, in the second exchange, |w|^2 after it.  Value v of workgroup wg sits at box[v * nwg + wg]
// (nwg <= MGS_MAX_WG), the grid totals behind all mailboxes at box[MGS_ONE_VALS * MGS_MAX_WG + v].
constexpr int MGS_ONE_VALS = 2 * (MGS_STEPS - 2) + 2;  // r_j, g_j (j < 30), |w|^2 before, |w|^2 after (second exchange)
// words per region: the mailboxes, then the totals, rounded up to 512 bytes so that the second region and the commit words behind it start on
// a cache line as the first one does (31 806 words would put them 48 bytes into one; bench.py, three runs each: 14.75 - 14.83 time steps per
// second unrounded, 14.86 - 15.00 rounded, against 14.86 - 14.98 for the 57 408-word regions this one replaced, also a multiple of 512 bytes)
constexpr size_t MGS_BOX_REGION = ((size_t)MGS_ONE_VALS * MGS_MAX_WG + MGS_ONE_VALS + 63) / 64 * 64;
static_assert(2 * (MGS_STEPS - 2) + 1 < MGS_ONE_VALS, "the largest value index of a sweep (2 dim + 1, dim = MGS_STEPS - 2) needs a mailbox row and a total");
static_assert((size_t)MGS_ONE_VALS * MGS_MAX_WG + MGS_ONE_VALS <= MGS_BOX_REGION,
              "k_mgs_one and k_ilu_mgs put their MGS_ONE_VALS totals behind MGS_ONE_VALS rows of MGS_MAX_WG mailboxes: all of it lies inside a region");
// after the two mailbox regions: one word per workgroup = sequence number of the last sweep whose part of w it wrote back
// (distinct addresses: a shared counter would serialise 512 atomics at the end of every sweep)
constexpr size_t MGS_TAIL = MGS_MAX_WG;

struct MgsArgs {
  const double *v[MGS_STEPS];
};

// ---- pieces both persistent sweep kernels have
// SolverGMRES' re-orthogonalisation test: a second sweep is asked for when the first one left |vv| <= 10 |vv_start| sqrt(eps), sqrt(eps) = 2^-26.
// The kernels normalise w only if it does not; the host (v_mgs, gmres) takes the same decision from the same two numbers: mgs_wants_second_sweep
// (nsx_internal.hpp).
// (The prologue -- idx[k] = the thread's k-th entry of the span, wv[k] = w there -- and the commit at the end -- tail[wg] = seq, then w written
// back -- stay pasted in the kernels: as an inlined helper the prologue costs k_mgs_one<8, 10, true> eight more spilled SGPRs, and the commit as
// a call changes the instruction streams of the 10- and 12-entry instantiations.)
// the end of a sweep that gave up (a bounded wait ran out): w stays as it was.  Tell the host (mapped word) and, from workgroup 0, wake it up
__device__ __forceinline__ void mgs_give_up(int *err_host, unsigned long long *pub_flag, unsigned long long seq, int wg) {
  if (threadIdx.x == 0) {
    __hip_atomic_store(err_host, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if (wg == 0) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __hip_atomic_store(pub_flag, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

#ifdef NSX_MGS_TRACE  // development only (tools/mgs_bench.hip): wall-clock stamps of workgroup 0 and of the last workgroup
__device__ unsigned long long *g_mgs_trace = nullptr;
#define MGS_STAMP()                                                                                         \
  do {                                                                                                      \
    if (g_mgs_trace && threadIdx.x == 0 && (wg == 0 || wg == nwg - 1) && n_stamp < 64)                       \
      g_mgs_trace[(wg == 0 ? 0 : 64) + n_stamp++] = wall_clock64();                                          \
  } while (0)
#else
#define MGS_STAMP() \
  do {              \
  } while (0)
#endif

// ---- the whole sweep in ONE grid-wide exchange ---------------------------------------------------------------------------
// The chain's coefficients are h_j = v_j . w_j with w_{j+1} = w_j - h_j v_j and w_0 = w, the vector as it ENTERS the sweep.  By
// linearity of the dot product (no orthogonality of the basis is assumed)
//     h_j = v_j . (w - sum_{i<j} h_i v_i) = r_j - sum_{i<j} G_ji h_i ,   r_j = v_j . w ,   G_ji = v_j . v_i  (the basis' Gram matrix):
// a unit-lower-triangular system whose data are sums over vectors that do not change during the sweep.  G is kept
// on the device per GMRES nesting level: the sweep that meets v_{dim-1} for the first time computes its row g_i = v_{dim-1} . v_i
// beside the r_j (the same registers), all older rows were computed by the earlier sweeps of the cycle.  So ONE exchange carries
// r_0..r_{dim-1}, g_0..g_{dim-1} and |w|^2; every workgroup then solves the same unit-lower-triangular system from the same
// totals, applies  w += (-h_j) v_j  for j ascending (the chain's operations on every entry, in the chain's order; the coefficients
// differ from the chain's by the rounding of the dot products only) from the
// basis vectors it still holds in registers, and gets |w|^2 AFTER the sweep without another exchange from
//     |w - sum_j h_j v_j|^2 = |w|^2 - 2 h.r + h^T G h
// (a difference of numbers of size |w|^2: taken when the sweep leaves more than 1 % of the norm, i.e. its rounding error stays
// below 1e-12 |w'|^2; otherwise a second exchange sums |w'|^2 itself).  A sweep of `dim` links costs one exchange (two when
// the formula is refused) instead of the chain's dim + 1, and every basis vector is still read exactly once as long as the thread can
// keep the block (dim <= DMAX); beyond, the oldest dim - DMAX vectors are streamed twice (dots, then update).
// The exchange is two hops: value v is summed over the workgroups' mailboxes by workgroup v % nwg (the 2 dim + 1
// sums are spread over the grid instead of queueing in workgroup 0), the totals are picked up by everybody.  (Letting every workgroup
// read all mailboxes itself -- one hop -- measured slower, the polling traffic gets in its own way.)
// Mailboxes: box[v * nwg + wg], totals behind them at box[MGS_ONE_VALS * MGS_MAX_WG + v].
// Basis vectors beyond the block kept in registers are read TWICE by a sweep (dot pass, update pass).  The register-resident ones
// are streamed with non-temporal loads (-DNSX_NT & 1: they must not evict F and the ILU factors from the 256-MiB Infinity Cache,
// profiles/r02_cache_policy_and_links.txt); the older ones take the default policy, so that the update pass finds in that cache what
// the dot pass brought in.

// ---- the same sweep in a DISTRIBUTED run (DIST): the single exchange also crosses the ranks -------------------------------------
// The reducers leave the LOCAL totals in ext.vals (one word each) and count themselves in at ext.arrive.  On the communication
// stream the host has enqueued, right behind this launch:  k_ext_wait (spins until the count is complete)  ->  ncclAllReduce of
// ext.vals over the ranks  ->  k_ext_release (stores this sweep's sequence number in ext.flag).  Every workgroup waits for that
// flag instead of for the grid totals and goes on with the GLOBAL sums: the ten newest basis vectors stay in registers across
// the collective, where the two-pass sweep (k_ls_dots / k_ls_update) reads the basis twice and pays two more launches.
// Failure is agreed on by all ranks: a reducer whose mailbox wait timed out (or k_ext_wait, if the count never completes) raises
// (All hand-offs are RELAXED agent-scope atomics behind an explicit s_waitcnt, like the mailboxes of nsx_grid.hpp: an acquire or a
// release at agent scope makes the compiler invalidate / write back the XCD's whole L2 around the access -- polled by 448 workgroups
// that doubled the time of the sweep's first phase: profiles/r04_ext_collective_timeline.txt.)
// ext.vals[MGS_EXT_FAIL], the collective SUMS that word, and a non-zero sum makes every rank's grid end without touching w; the
// hosts then all redo the sweep with the two-pass path.  The wait for the flag is bounded ABOVE the other time-outs (mailboxes 2 s,
// k_ext_wait 4 s: a rank that fails locally needs both before its collective goes out): 8 s.  A flag wait that still times out is a
// verdict of ONE rank -- its peers' grids may have gone on with the global sums -- so it must not change this rank's collective
// sequence: the host waits for the (late) collective, finishes the sweep from the global sums it delivered (v_mgs: same coefficients,
// same updates, no further collective) and raises ext.vals[MGS_EXT_LEAVE] in its NEXT sweep; that word is summed like the failure
// word, and a non-zero sum takes every rank to the two-pass sweep together.  When the Gram formula for |w'|^2 is refused (the sweep
// removed > 99 % of the norm: decided from the global sums, i.e. alike on every rank) the grid leaves the LOCAL sum of |w'|^2 in
// ext.norm_out, does not normalise and reports "norm pending": the host all-reduces that word (the second collective).
constexpr int MGS_EXT_VALS = 64, MGS_EXT_FAIL = 63, MGS_EXT_LEAVE = 62;
constexpr unsigned long long GX_EXT_TIMEOUT_TICKS = 800000000ull;  // 8 s at 100 MHz: above the mailbox wait (2 s) + k_ext_wait (4 s) a failing peer needs before its collective goes out
static_assert(GX_EXT_TIMEOUT_TICKS > 3 * GX_TIMEOUT_TICKS, "the flag wait must outlast a peer's mailbox wait + k_ext_wait");
struct MgsExt {
  double *vals;              // [MGS_EXT_VALS] this sweep's buffer: local totals, then (after the collective) the global ones
  double *vals_other;        // the other buffer: its failure word is cleared for the next sweep
  unsigned int *arrive;      // reducers that have delivered, cumulative over all sweeps
  unsigned long long *flag;  // sequence number of the last sweep whose collective is complete
  unsigned long long *abort_seq;  // sequence number of the last sweep a workgroup gave up on: the verdict of the WHOLE grid (see the wait)
  double *norm_out;          // local |w'|^2 when the formula is refused
  int leave;                 // 1: this rank asks all ranks to leave the persistent sweep (an earlier flag wait of its own timed out)
};
__device__ __forceinline__ double ext_ld(const double *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void ext_st(double *p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

template <int E, int DMAX, bool DIST>
__global__ __launch_bounds__(256) void k_mgs_one(int n, int split, int gap, double *__restrict__ w, MgsArgs V, int dim, double *__restrict__ gram,
                                                 unsigned long long *box, unsigned long long *box_next, int reset_words, double *__restrict__ scal_out,
                                                 int *err_host, unsigned long long *tail, int normalize, int consider, double *pub_vals,
                                                 unsigned long long *pub_flag, unsigned long long seq, int drop_wg, double norm_guard, MgsExt ext) {
  __shared__ double sh[4][MGS_ONE_VALS];   // per-wave sums of every value
  __shared__ double tot[MGS_ONE_VALS];     // grid totals
  __shared__ double G[MGS_STEPS][MGS_STEPS + 1], hc[MGS_STEPS];
  __shared__ double s_norm2;
  __shared__ int s_err;
  const int nwg = gridDim.x, wg = blockIdx.x, T = nwg * 256, t = wg * 256 + threadIdx.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (threadIdx.x == 0) s_err = 0;
  [[maybe_unused]] int n_stamp = 0;  // development only (tools/mgs_bench.hip): the stamps are empty without NSX_MGS_TRACE
  MGS_STAMP();  // start
  unsigned long long *total = box + (size_t)MGS_ONE_VALS * MGS_MAX_WG, *total_next = box_next + (size_t)MGS_ONE_VALS * MGS_MAX_WG;
  for (int q = t; q < reset_words; q += T) box_next[q] = GX_EMPTY;
  if (wg == 0 && threadIdx.x < MGS_ONE_VALS) total_next[threadIdx.x] = GX_EMPTY;
  if constexpr (DIST) {
    if (wg == 0 && threadIdx.x < MGS_EXT_VALS) ext_st(ext.vals_other + threadIdx.x, 0.0);  // the next sweep's buffer (its failure word in particular)
  }
  const int nvals = 2 * dim + 1;  // r_j at j, g_j at dim + j, |w|^2 at 2 dim
  // the older rows of the Gram matrix (written by the earlier sweeps of this cycle) are requested first and parked in registers:
  // read behind the exchange they were a trip through memory on the critical path of every workgroup
  // (only where the registers are there: the E = 10 instantiation would lose its second wave per SIMD, and with it the resident grid)
  constexpr bool PRE = E <= 8;
  constexpr int GPRE = PRE ? (MGS_STEPS * MGS_STEPS + 255) / 256 : 1;
  double gpre[GPRE];
  if constexpr (PRE) {
#pragma unroll
    for (int k = 0; k < GPRE; ++k) {
      const int q = threadIdx.x + 256 * k, r_ = q / MGS_STEPS, c_ = q % MGS_STEPS;
      gpre[k] = (r_ < dim - 1 && c_ <= r_) ? gram[r_ * 32 + c_] : 0.0;
    }
  }
  double wv[E], vb[DMAX][E];
  int idx[E];
#pragma unroll
  for (int k = 0; k < E; ++k) {
    const int i0 = t + k * T;
    idx[k] = i0 < n ? i0 + (i0 >= split ? gap : 0) : -1;
    wv[k] = idx[k] >= 0 ? w[idx[k]] : 0.0;
  }
  // the block the thread keeps: the LAST min(dim, DMAX) basis vectors (the newest one, whose Gram row is due, is among them)
  const int j_keep = dim > DMAX ? dim - DMAX : 0;
#pragma unroll
  for (int i = 0; i < DMAX; ++i) {
    const double *__restrict__ vp = j_keep + i < dim ? V.v[j_keep + i] : nullptr;
#pragma unroll
    for (int k = 0; k < E; ++k) vb[i][k] = (vp && idx[k] >= 0) ? ld_stream<1>(vp + idx[k]) : 0.0;
  }
  // v_{dim-1} in registers of its own (static index): the second operand of the Gram row
  double vl[E];
#pragma unroll
  for (int k = 0; k < E; ++k) vl[k] = 0.0;
#pragma unroll
  for (int i = 0; i < DMAX; ++i)
    if (j_keep + i == dim - 1) {
#pragma unroll
      for (int k = 0; k < E; ++k) vl[k] = vb[i][k];
    }
  auto wave_post = [&](int v, double a) {  // this wave's sum of value v
    const double s_ = gx_wave_sum(a);
    if (lane == 0) sh[wave][v] = s_;
  };
  {
    double a = 0.0;
#pragma unroll
    for (int k = 0; k < E; ++k) a += wv[k] * wv[k];
    wave_post(2 * dim, a);
  }
  for (int j = 0; j < j_keep; ++j) {  // older vectors: streamed, not kept (dim > DMAX only)
    const double *__restrict__ vp = V.v[j];
    double ar = 0.0, ag = 0.0;
#pragma unroll
    for (int k = 0; k < E; ++k) {
      const double x_ = idx[k] >= 0 ? vp[idx[k]] : 0.0;
      ar += wv[k] * x_;
      ag += vl[k] * x_;
    }
    wave_post(j, ar);
    wave_post(dim + j, ag);
  }
#pragma unroll
  for (int i = 0; i < DMAX; ++i)
    if (j_keep + i < dim) {
      double ar = 0.0, ag = 0.0;
#pragma unroll
      for (int k = 0; k < E; ++k) {
        ar += wv[k] * vb[i][k];
        ag += vl[k] * vb[i][k];
      }
      wave_post(j_keep + i, ar);
      wave_post(dim + j_keep + i, ag);
    }
  if constexpr (PRE) {
#pragma unroll
    for (int k = 0; k < GPRE; ++k) {
      const int q = threadIdx.x + 256 * k, r_ = q / MGS_STEPS, c_ = q % MGS_STEPS;
      if (r_ < dim - 1 && c_ <= r_) G[r_][c_] = gpre[k];
    }
  }
  __syncthreads();
  MGS_STAMP();  // loads arrived, local sums done
  // ---- hop 1: mailboxes; value v is summed by workgroup v % nwg
  int lerr = 0;
  for (int v = threadIdx.x; v < nvals; v += 256)
    if (wg != drop_wg) gx_post(box + (size_t)v * nwg + wg, (sh[0][v] + sh[1][v]) + (sh[2][v] + sh[3][v]));  // drop_wg >= 0: fault injection (NSX_GX_DROP_WG), a workgroup that never arrives
  for (int v = wg; v < nvals; v += nwg) {
    double a = 0.0;
    for (int q = threadIdx.x; q < nwg; q += 256) a += gx_wait_value(box + (size_t)v * nwg + q, &lerr);
    if (lerr) s_err = 1;
    __syncthreads();  // sh is reused by the block sum below (and s_err must be seen)
    const double s_ = gx_wave_sum(a);
    if (lane == 0) sh[wave][0] = s_;
    __syncthreads();
    if constexpr (DIST) {
      if (threadIdx.x == 0) {
        if (!s_err) ext_st(ext.vals + v, (sh[0][0] + sh[1][0]) + (sh[2][0] + sh[3][0]));
        else ext_st(ext.vals + MGS_EXT_FAIL, 1.0);  // summed over the ranks: everybody learns of it
        if (v == 0 && ext.leave) ext_st(ext.vals + MGS_EXT_LEAVE, 1.0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_fetch_add(ext.arrive, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // counted in either way: the collective must go out
      }
    } else {
      if (threadIdx.x == 0 && !s_err) gx_post(total + v, (sh[0][0] + sh[1][0]) + (sh[2][0] + sh[3][0]));  // a total built on a timed-out mailbox never goes out
    }
    __syncthreads();
  }
  MGS_STAMP();  // posted, and (reducers) totals out
  // ---- hop 2: everybody picks up the totals
  if constexpr (DIST) {
    if (threadIdx.x == 0) {  // the collective of this sweep is complete once the flag carries its sequence number
      // A grid that gives up must give up as a whole.  The likely reason for a collective that does not come is that its kernel finds
      // no place on the device WHILE this grid holds it (RCCL's generic kernel: 256 threads x 264 VGPRs; measured with a self-addressed
      // send / receive, NSX_EXT_SELF_P2P): then the first workgroup that leaves makes room, the collective runs, and the workgroups
      // still waiting would see the flag and go on to write w.  So the first one to time out records the sweep in abort_seq BEFORE it
      // leaves, and a workgroup that sees the flag looks there before it believes it.
      unsigned long long t0 = 0;
      for (unsigned int spin = 1; __hip_atomic_load(ext.flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < seq; ++spin) {
        __builtin_amdgcn_s_sleep(1);
        if ((spin & 255u) == 0) {
          if (__hip_atomic_load(ext.abort_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == seq) {
            s_err = 1;
            break;
          }
          const unsigned long long now = wall_clock64();
          if (t0 == 0) t0 = now;
          else if (now - t0 > GX_EXT_TIMEOUT_TICKS) {
            __hip_atomic_store(ext.abort_seq, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            s_err = 1;
            break;
          }
        }
      }
      if (!s_err && __hip_atomic_load(ext.abort_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == seq) s_err = 1;
    }
    __syncthreads();
    for (int v = threadIdx.x; v < nvals; v += 256) tot[v] = ext_ld(ext.vals + v);
    if (threadIdx.x == 0 && (ext_ld(ext.vals + MGS_EXT_FAIL) != 0.0 || ext_ld(ext.vals + MGS_EXT_LEAVE) != 0.0)) s_err = 1;  // some rank's grid was not complete, or a rank asks everybody to leave
  } else {
    for (int v = threadIdx.x; v < nvals; v += 256) {
      tot[v] = gx_wait_value(total + v, &lerr);
      if (lerr) s_err = 1;
    }
  }
  __syncthreads();
  MGS_STAMP();  // totals picked up
  bool dead = s_err != 0;
  double xo[E];  // entries of the next streamed (older) vector of the update below
#pragma unroll
  for (int k = 0; k < E; ++k) xo[k] = (!dead && j_keep > 0 && idx[k] >= 0) ? V.v[0][idx[k]] : 0.0;
  if (!dead) {
    // Gram matrix of the basis: older rows parked in G before the exchange, the new row from this exchange; then h by forward substitution and the
    // norm after the sweep, one wave, lane j = link j
    if constexpr (!PRE) {
      for (int q = threadIdx.x; q < (dim - 1) * MGS_STEPS; q += 256) {
        const int r_ = q / MGS_STEPS, c_ = q % MGS_STEPS;
        if (c_ <= r_) G[r_][c_] = gram[r_ * 32 + c_];
      }
    }
    if ((int)threadIdx.x < dim) G[dim - 1][threadIdx.x] = tot[dim + threadIdx.x];
    __syncthreads();
    if (wave == 0) {
      double hj = 0.0;
      const int col = lane < dim ? lane : 0;
      double g_cur = G[0][col], t_cur = tot[0];  // the LDS operands of link j + 1 are requested while link j is summed
      for (int j = 0; j < dim; ++j) {
        const int jn = j + 1 < dim ? j + 1 : j;
        const double g_next = G[jn][col], t_next = tot[jn];
        // s = sum_{i<j} G_ji h_i over the lanes i < j
        double part = (lane < j) ? g_cur * hj : 0.0;
        part = gx_wave_sum(part);
        if (lane == j) hj = t_cur - part;
        g_cur = g_next;
        t_cur = t_next;
      }
      if (lane < dim) hc[lane] = hj;
      // |w'|^2 = |w|^2 - 2 h.r + h^T G h   (G symmetric: row lane against all columns)
      double quad = 0.0;
      if (lane < dim) {
        double row = 0.0;
        for (int i = 0; i < dim; ++i) row += (i <= lane ? G[lane][i] : G[i][lane]) * __shfl(hj, i, 64);
        quad = hj * (row - 2.0 * tot[lane]);
      } else {
        for (int i = 0; i < dim; ++i) (void)__shfl(hj, i, 64);
      }
      quad = gx_wave_sum(quad);
      if (lane == 0) s_norm2 = tot[2 * dim] + quad;
    }
    __syncthreads();
    MGS_STAMP();  // coefficients solved
    // w += (-h_j) v_j, j ascending: the streamed (older) vectors first, then the kept block.  The entries of vector j + 1 are
    // requested before those of vector j are used (one vector ahead; the first one in front of the coefficient solve): taken one
    // after the other every older vector cost a full trip through memory, 4 us each at dim 14 (profiles/r03_mgs_one_timeline.txt).
    // Same operations on the same operands in the same order.
    for (int j = 0; j < j_keep; ++j) {
      double xn[E];
#pragma unroll
      for (int k = 0; k < E; ++k) xn[k] = (j + 1 < j_keep && idx[k] >= 0) ? V.v[j + 1][idx[k]] : 0.0;
      const double alpha = -1.0 * hc[j];
#pragma unroll
      for (int k = 0; k < E; ++k)
        if (idx[k] >= 0) wv[k] += alpha * xo[k];
#pragma unroll
      for (int k = 0; k < E; ++k) xo[k] = xn[k];
    }
#pragma unroll
    for (int i = 0; i < DMAX; ++i)
      if (j_keep + i < dim) {
        const double alpha = -1.0 * hc[j_keep + i];
#pragma unroll
        for (int k = 0; k < E; ++k) wv[k] += alpha * vb[i][k];
      }
    // the formula is a difference of numbers of size |w|^2: refuse it when less than 1 % of the norm is left
    double norm2 = s_norm2;
    const double w2 = tot[2 * dim];
    bool norm_pending = false;
    if (!(norm2 > norm_guard * w2)) {  // uniform over the grid (same totals everywhere): a second exchange sums |w'|^2 itself
      double a = 0.0;
#pragma unroll
      for (int k = 0; k < E; ++k) a += wv[k] * wv[k];
      const double s_ = gx_wave_sum(a);
      __syncthreads();
      if (lane == 0) sh[wave][0] = s_;
      __syncthreads();
      const int v = 2 * dim + 1;
      if (threadIdx.x == 0 && wg != drop_wg) gx_post(box + (size_t)v * nwg + wg, (sh[0][0] + sh[1][0]) + (sh[2][0] + sh[3][0]));
      if (wg == v % nwg) {
        double b = 0.0;
        for (int q = threadIdx.x; q < nwg; q += 256) b += gx_wait_value(box + (size_t)v * nwg + q, &lerr);
        if (lerr) s_err = 1;
        __syncthreads();
        const double sb = gx_wave_sum(b);
        if (lane == 0) sh[wave][1] = sb;
        __syncthreads();
        if constexpr (DIST) {
          // the local sum for the host's collective; a timed-out mailbox makes it NaN, which the host turns into the two-pass redo
          if (threadIdx.x == 0) *ext.norm_out = s_err ? __longlong_as_double(0x7ff8000000000000ll) : (sh[0][1] + sh[1][1]) + (sh[2][1] + sh[3][1]);
        } else {
          if (threadIdx.x == 0 && !s_err) gx_post(total + v, (sh[0][1] + sh[1][1]) + (sh[2][1] + sh[3][1]));
        }
      }
      if constexpr (DIST) {
        norm_pending = true;  // nobody waits: the sum travels through the host's all-reduce behind this launch
      } else {
        if (threadIdx.x == 0) {
          const double x_ = gx_wait_value(total + v, &lerr);
          if (lerr) s_err = 1;
          s_norm2 = x_;
        }
        __syncthreads();
        dead = s_err != 0;
        norm2 = s_norm2;
      }
    }
    if (!dead && normalize && !norm_pending) {  // vv *= 1. / s with s = sqrt(|vv|^2), skipped for s == 0 (SolverGMRES)
      const double nrm = sqrt(norm2);
      const bool second_sweep = consider && mgs_wants_second_sweep(nrm, w2);
      if (nrm != 0.0 && !second_sweep) {
        const double inv = 1. / nrm;
#pragma unroll
        for (int k = 0; k < E; ++k) wv[k] = inv * wv[k];
      }
    }
  }
  if (dead) {
    mgs_give_up(err_host, pub_flag, seq, wg);
    return;
  }
  if (wg == 0) {
    // the new Gram row for the later sweeps of this cycle, the coefficients for the device and the host
    if ((int)threadIdx.x < dim) {
      gram[(dim - 1) * 32 + threadIdx.x] = tot[dim + threadIdx.x];
      scal_out[threadIdx.x] = hc[threadIdx.x];
      __hip_atomic_store(pub_vals + threadIdx.x, hc[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    if (threadIdx.x == 0) {
      scal_out[dim] = s_norm2;
      scal_out[dim + 1] = tot[2 * dim];
      __hip_atomic_store(pub_vals + dim, s_norm2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __hip_atomic_store(pub_vals + dim + 1, tot[2 * dim], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      if constexpr (DIST) {  // 1: |w'|^2 is still rank-local (ext.norm_out) and w is not normalised
        const double norm2_ = s_norm2, w2_ = tot[2 * dim];
        __hip_atomic_store(pub_vals + dim + 2, !(norm2_ > norm_guard * w2_) ? 1.0 : 0.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(pub_flag, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  if (threadIdx.x == 0) tail[wg] = seq;  // this workgroup commits its part of w, then writes it back (pasted in both kernels, see "pieces" above)
  MGS_STAMP();  // update done
#pragma unroll
  for (int k = 0; k < E; ++k)
    if (idx[k] >= 0) w[idx[k]] = wv[k];
  MGS_STAMP();  // stores issued
}

// ---- the triangular solves of the preconditioner AND the sweep in ONE launch (round 5) ------------------------------------------
// An inner GMRES iteration on F is  p = F v_k (SpMV)  ->  z = (LU)^-1 p (k_ilu_solve_lanes: one wave per ~8 rank blocks, their rows
// in LDS)  ->  sweep of z against the basis (k_mgs_one).  The last two hand z to each other through HBM, and while the sweeping wave
// of the solve works through its ~120 ticks the device moves nothing, while the sweep then spends its first 11-17 us loading basis
// vectors with every wave stalled.  Here workgroup b of the persistent grid IS wave b of the solve's schedule (same stream, same ticks,
// same arithmetic: z is bit for bit the separate kernel's): its four waves load the right-hand side rows into LDS, wave 0 runs the two
// sweeps while waves 1-3 request their entries of the basis vectors, and after a barrier every thread takes its entries of z from
// LDS -- z never travels through memory -- and the kernel goes on as k_mgs_one: one grid exchange, the coefficients from the Gram
// matrix, update, norm, normalisation.  Entry -> thread: entry e of the workgroup's rows (LDS order) belongs to thread e % 256, so a
// workgroup needs at most 256 * E / NCOMP rows (853 with E = 10; the bench layout's largest wave has 747).  Sums are fixed-order but
// taken in another grouping than k_mgs_one's (entries are dealt by rank block, not striped over the vector): same history class, other
// last bits.  No static __shared__ object: the solve's stream holds absolute LDS addresses (nsx_ilu_lanes.hpp), its rows sit at address 0.
struct IluMgsArgs {
  const int32_t *row_ptr, *rows, *slab_ptr;
  const uint32_t *meta;
  const double *val, *dinv, *rhs;
  int ilu_doubles;  // LDS doubles reserved for the solve's rows (+ 64 scratch rows), the sweep's arrays follow
  unsigned long long *trace;  // development (NSX_ILU_MGS_TRACE): 16 wall-clock stamps per wave, or null
};
#define IM_STAMP(k)                                                                                                   \
  do {                                                                                                                \
    if (I.trace && lane == 0) I.trace[((size_t)wg * 4 + wave) * 16 + (k)] = wall_clock64();                             \
  } while (0)
template <int NCOMP, int EI, int PF, int E, int DMAX>
__global__ __launch_bounds__(256) void k_ilu_mgs(int n, double *__restrict__ w, MgsArgs V, int dim, double *__restrict__ gram, unsigned long long *box,
                                                 unsigned long long *box_next, int reset_words, double *__restrict__ scal_out, int *err_host, unsigned long long *tail,
                                                 int normalize, int consider, double *pub_vals, unsigned long long *pub_flag, unsigned long long seq, int drop_wg,
                                                 double norm_guard, IluMgsArgs I) {
  extern __shared__ double xs[];
  double *sh = xs + I.ilu_doubles;                 // [4][MGS_ONE_VALS]
  double *tot = sh + 4 * MGS_ONE_VALS;             // [MGS_ONE_VALS]
  double *G = tot + MGS_ONE_VALS;                  // [MGS_STEPS][MGS_STEPS + 1]
  double *hc = G + MGS_STEPS * (MGS_STEPS + 1);    // [MGS_STEPS]
  double *s_norm2 = hc + MGS_STEPS;
  int *s_err = (int *)(s_norm2 + 1);
  double *stage = s_norm2 + 2;                     // [DMAX][E][64]: the sweeping wave's entries of the basis
  const int nwg = gridDim.x, wg = blockIdx.x, T = nwg * 256, t = wg * 256 + threadIdx.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const bool lds_ok = (uint32_t)(uintptr_t)(lds_f64 *)xs == 0u;  // uniform over the grid: everybody leaves, nobody waits
  if (!lds_ok) {
    mgs_give_up(err_host, pub_flag, seq, wg);
    return;
  }
  if (threadIdx.x == 0) *s_err = 0;
  IM_STAMP(0);  // start
  unsigned long long *total = box + (size_t)MGS_ONE_VALS * MGS_MAX_WG, *total_next = box_next + (size_t)MGS_ONE_VALS * MGS_MAX_WG;
  for (int q = t; q < reset_words; q += T) box_next[q] = GX_EMPTY;
  if (wg == 0 && threadIdx.x < MGS_ONE_VALS) total_next[threadIdx.x] = GX_EMPTY;
  const int nvals = 2 * dim + 1;
  // ---- the workgroup's rows: wave `wg` of the solve's schedule
  const int rb = I.row_ptr[wg], nr = I.row_ptr[wg + 1] - rb, ne = nr * NCOMP;
  const int s0 = I.slab_ptr[2 * wg], s1 = I.slab_ptr[2 * wg + 1], s2 = I.slab_ptr[2 * wg + 2];
  int idx[E];
#pragma unroll
  for (int k = 0; k < E; ++k) {
    const int e = (int)threadIdx.x + 256 * k;
    const int r_ = e < ne ? I.rows[rb + e / NCOMP] : -1;
    idx[k] = r_ >= 0 ? r_ * NCOMP + e % NCOMP : -1;
  }
  {
    double y[E];
#pragma unroll
    for (int k = 0; k < E; ++k) y[k] = idx[k] >= 0 ? I.rhs[idx[k]] : 0.0;
#pragma unroll
    for (int k = 0; k < E; ++k)
      if (idx[k] >= 0) xs[(int)threadIdx.x + 256 * k] = y[k];
  }
  if (wave == 0) {
#pragma unroll
    for (int c = 0; c < NCOMP; ++c) xs[(nr + lane) * NCOMP + c] = 0.0;  // the scratch rows of the idle slots
  }
  __syncthreads();
  IM_STAMP(1);  // right-hand side rows in LDS
  // which wave sweeps.  (Giving the two workgroups of a CU different sweeping waves -- different SIMDs -- measured nothing; neither did
  // delaying the other waves' basis requests by 4 - 12 us or pacing them one vector per 0.5 - 1 us: 45.9 - 46.8 us per launch throughout.)
  constexpr int iw = 0;
  if (wave == iw) {  // the two sweeps of the triangular solve, exactly k_ilu_solve_lanes'
    const uint32_t scratch = (uint32_t)(nr + lane) * (8u * NCOMP);
    LaneSlot<EI> A[PF];
    lane_load<EI, PF>(A, s0, I.meta, I.val, (unsigned)lane);
    lane_sweep<NCOMP, EI, PF>(A, s0, s1, I.meta, I.val, (unsigned)lane, scratch);  // y = L^{-1} b
    IM_STAMP(2);  // forward sweep done
    lane_load<EI, PF>(A, s1, I.meta, I.val, (unsigned)lane);
    for (int base = 0; base < nr; base += 64 * 4) {  // y *= D^{-1}
      double d[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int q = base + 64 * k + lane;
        d[k] = q < nr ? I.dinv[rb + q] : 0.0;
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int q = base + 64 * k + lane;
        if (q < nr) {
#pragma unroll
          for (int c = 0; c < NCOMP; ++c) xs[q * NCOMP + c] *= d[k];
        }
      }
    }
    __builtin_amdgcn_wave_barrier();
    lane_sweep<NCOMP, EI, PF>(A, s1, s2, I.meta, I.val, (unsigned)lane, scratch);  // x = U^{-1} y
    IM_STAMP(3);  // backward sweep done
  }
  // ---- the basis.  The three waves that do not sweep get here at once: their requests fly while the fourth sweeps.  The sweeping
  // wave's OWN entries of the basis would be requested behind its sweeps and arrive 6 - 7 us later with the whole workgroup waiting at
  // the barrier (profiles/r05_ilu_mgs_timeline.txt): the other three fetch them as well, into LDS (`stage`, [vector][k][lane]).
  double wv[E], vb[DMAX][E];
  const int j_keep = dim > DMAX ? dim - DMAX : 0;
  if (wave != iw) {
#pragma unroll
    for (int i = 0; i < DMAX; ++i) {
      const double *__restrict__ vp = j_keep + i < dim ? V.v[j_keep + i] : nullptr;
#pragma unroll
      for (int k = 0; k < E; ++k) vb[i][k] = (vp && idx[k] >= 0) ? ld_stream<1>(vp + idx[k]) : 0.0;
    }
    constexpr int HB = (64 * E + 191) / 192;
    const int hid = (wave < iw ? wave : wave - 1) * 64 + lane;  // 0 .. 191
    int gi[HB];
#pragma unroll
    for (int m = 0; m < HB; ++m) {
      const int q = hid + 192 * m, e = 64 * iw + (q & 63) + 256 * (q >> 6);
      const int r_ = (q < 64 * E && e < ne) ? I.rows[rb + e / NCOMP] : -1;
      gi[m] = r_ >= 0 ? r_ * NCOMP + e % NCOMP : -1;
    }
#pragma unroll
    for (int i = 0; i < DMAX; ++i) {
      const double *__restrict__ vp = j_keep + i < dim ? V.v[j_keep + i] : nullptr;
      double tmp[HB];
#pragma unroll
      for (int m = 0; m < HB; ++m) tmp[m] = (vp && gi[m] >= 0) ? ld_stream<1>(vp + gi[m]) : 0.0;
#pragma unroll
      for (int m = 0; m < HB; ++m)
        if (hid + 192 * m < 64 * E) stage[i * (64 * E) + hid + 192 * m] = tmp[m];
    }
  }
  if (I.trace) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    IM_STAMP(4);  // this wave's requests have arrived
  }
  __syncthreads();  // z is complete in LDS, and so is the sweeping wave's part of the basis
  IM_STAMP(5);
  if (wave == iw) {
#pragma unroll
    for (int i = 0; i < DMAX; ++i)
#pragma unroll
      for (int k = 0; k < E; ++k) vb[i][k] = stage[(i * E + k) * 64 + lane];
  }
#pragma unroll
  for (int k = 0; k < E; ++k) wv[k] = idx[k] >= 0 ? xs[(int)threadIdx.x + 256 * k] : 0.0;
  double vl[E];
#pragma unroll
  for (int k = 0; k < E; ++k) vl[k] = 0.0;
#pragma unroll
  for (int i = 0; i < DMAX; ++i)
    if (j_keep + i == dim - 1) {
#pragma unroll
      for (int k = 0; k < E; ++k) vl[k] = vb[i][k];
    }
  auto wave_post = [&](int v, double a) {
    const double s_ = gx_wave_sum(a);
    if (lane == 0) sh[wave * MGS_ONE_VALS + v] = s_;
  };
  {
    double a = 0.0;
#pragma unroll
    for (int k = 0; k < E; ++k) a += wv[k] * wv[k];
    wave_post(2 * dim, a);
  }
  for (int j = 0; j < j_keep; ++j) {  // older vectors: streamed, not kept (dim > DMAX only)
    const double *__restrict__ vp = V.v[j];
    double ar = 0.0, ag = 0.0;
#pragma unroll
    for (int k = 0; k < E; ++k) {
      const double x_ = idx[k] >= 0 ? vp[idx[k]] : 0.0;
      ar += wv[k] * x_;
      ag += vl[k] * x_;
    }
    wave_post(j, ar);
    wave_post(dim + j, ag);
  }
#pragma unroll
  for (int i = 0; i < DMAX; ++i)
    if (j_keep + i < dim) {
      double ar = 0.0, ag = 0.0;
#pragma unroll
      for (int k = 0; k < E; ++k) {
        ar += wv[k] * vb[i][k];
        ag += vl[k] * vb[i][k];
      }
      wave_post(j_keep + i, ar);
      wave_post(dim + j_keep + i, ag);
    }
  __syncthreads();
  IM_STAMP(6);  // local sums done
  // ---- hop 1: mailboxes; value v is summed by workgroup v % nwg
  int lerr = 0;
  for (int v = threadIdx.x; v < nvals; v += 256)
    if (wg != drop_wg) gx_post(box + (size_t)v * nwg + wg, (sh[v] + sh[MGS_ONE_VALS + v]) + (sh[2 * MGS_ONE_VALS + v] + sh[3 * MGS_ONE_VALS + v]));
  for (int v = wg; v < nvals; v += nwg) {
    double a = 0.0;
    for (int q = threadIdx.x; q < nwg; q += 256) a += gx_wait_value(box + (size_t)v * nwg + q, &lerr);
    if (lerr) *s_err = 1;
    __syncthreads();
    const double s_ = gx_wave_sum(a);
    if (lane == 0) sh[wave * MGS_ONE_VALS] = s_;
    __syncthreads();
    if (threadIdx.x == 0 && !*s_err) gx_post(total + v, (sh[0] + sh[MGS_ONE_VALS]) + (sh[2 * MGS_ONE_VALS] + sh[3 * MGS_ONE_VALS]));
    __syncthreads();
  }
  // ---- hop 2: everybody picks up the totals
  for (int v = threadIdx.x; v < nvals; v += 256) {
    tot[v] = gx_wait_value(total + v, &lerr);
    if (lerr) *s_err = 1;
  }
  __syncthreads();
  IM_STAMP(7);  // totals picked up
  bool dead = *s_err != 0;
  double xo[E];
#pragma unroll
  for (int k = 0; k < E; ++k) xo[k] = (!dead && j_keep > 0 && idx[k] >= 0) ? V.v[0][idx[k]] : 0.0;
  if (!dead) {
    for (int q = threadIdx.x; q < (dim - 1) * MGS_STEPS; q += 256) {
      const int r_ = q / MGS_STEPS, c_ = q % MGS_STEPS;
      if (c_ <= r_) G[r_ * (MGS_STEPS + 1) + c_] = gram[r_ * 32 + c_];
    }
    if ((int)threadIdx.x < dim) G[(dim - 1) * (MGS_STEPS + 1) + threadIdx.x] = tot[dim + threadIdx.x];
    __syncthreads();
    if (wave == 0) {
      double hj = 0.0;
      const int col = lane < dim ? lane : 0;
      double g_cur = G[col], t_cur = tot[0];
      for (int j = 0; j < dim; ++j) {
        const int jn = j + 1 < dim ? j + 1 : j;
        const double g_next = G[jn * (MGS_STEPS + 1) + col], t_next = tot[jn];
        double part = (lane < j) ? g_cur * hj : 0.0;
        part = gx_wave_sum(part);
        if (lane == j) hj = t_cur - part;
        g_cur = g_next;
        t_cur = t_next;
      }
      if (lane < dim) hc[lane] = hj;
      double quad = 0.0;
      if (lane < dim) {
        double row = 0.0;
        for (int i = 0; i < dim; ++i) row += (i <= lane ? G[lane * (MGS_STEPS + 1) + i] : G[i * (MGS_STEPS + 1) + lane]) * __shfl(hj, i, 64);
        quad = hj * (row - 2.0 * tot[lane]);
      } else {
        for (int i = 0; i < dim; ++i) (void)__shfl(hj, i, 64);
      }
      quad = gx_wave_sum(quad);
      if (lane == 0) *s_norm2 = tot[2 * dim] + quad;
    }
    __syncthreads();
    for (int j = 0; j < j_keep; ++j) {
      double xn[E];
#pragma unroll
      for (int k = 0; k < E; ++k) xn[k] = (j + 1 < j_keep && idx[k] >= 0) ? V.v[j + 1][idx[k]] : 0.0;
      const double alpha = -1.0 * hc[j];
#pragma unroll
      for (int k = 0; k < E; ++k)
        if (idx[k] >= 0) wv[k] += alpha * xo[k];
#pragma unroll
      for (int k = 0; k < E; ++k) xo[k] = xn[k];
    }
#pragma unroll
    for (int i = 0; i < DMAX; ++i)
      if (j_keep + i < dim) {
        const double alpha = -1.0 * hc[j_keep + i];
#pragma unroll
        for (int k = 0; k < E; ++k) wv[k] += alpha * vb[i][k];
      }
    double norm2 = *s_norm2;
    const double w2 = tot[2 * dim];
    if (!(norm2 > norm_guard * w2)) {  // uniform over the grid: a second exchange sums |w'|^2 itself
      double a = 0.0;
#pragma unroll
      for (int k = 0; k < E; ++k) a += wv[k] * wv[k];
      const double s_ = gx_wave_sum(a);
      __syncthreads();
      if (lane == 0) sh[wave * MGS_ONE_VALS] = s_;
      __syncthreads();
      const int v = 2 * dim + 1;
      if (threadIdx.x == 0 && wg != drop_wg) gx_post(box + (size_t)v * nwg + wg, (sh[0] + sh[MGS_ONE_VALS]) + (sh[2 * MGS_ONE_VALS] + sh[3 * MGS_ONE_VALS]));
      if (wg == v % nwg) {
        double b = 0.0;
        for (int q = threadIdx.x; q < nwg; q += 256) b += gx_wait_value(box + (size_t)v * nwg + q, &lerr);
        if (lerr) *s_err = 1;
        __syncthreads();
        const double sb = gx_wave_sum(b);
        if (lane == 0) sh[wave * MGS_ONE_VALS + 1] = sb;
        __syncthreads();
        if (threadIdx.x == 0 && !*s_err) gx_post(total + v, (sh[1] + sh[MGS_ONE_VALS + 1]) + (sh[2 * MGS_ONE_VALS + 1] + sh[3 * MGS_ONE_VALS + 1]));
      }
      if (threadIdx.x == 0) {
        const double x_ = gx_wait_value(total + v, &lerr);
        if (lerr) *s_err = 1;
        *s_norm2 = x_;
      }
      __syncthreads();
      dead = *s_err != 0;
      norm2 = *s_norm2;
    }
    if (!dead && normalize) {
      const double nrm = sqrt(norm2);
      const bool second_sweep = consider && mgs_wants_second_sweep(nrm, w2);
      if (nrm != 0.0 && !second_sweep) {
        const double inv = 1. / nrm;
#pragma unroll
        for (int k = 0; k < E; ++k) wv[k] = inv * wv[k];
      }
    }
  }
  if (dead) {
    mgs_give_up(err_host, pub_flag, seq, wg);
    return;
  }
  if (wg == 0) {
    if ((int)threadIdx.x < dim) {
      gram[(dim - 1) * 32 + threadIdx.x] = tot[dim + threadIdx.x];
      scal_out[threadIdx.x] = hc[threadIdx.x];
      __hip_atomic_store(pub_vals + threadIdx.x, hc[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    if (threadIdx.x == 0) {
      scal_out[dim] = *s_norm2;
      scal_out[dim + 1] = tot[2 * dim];
      __hip_atomic_store(pub_vals + dim, *s_norm2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      __hip_atomic_store(pub_vals + dim + 1, tot[2 * dim], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(pub_flag, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
  IM_STAMP(8);  // coefficients, update, norm done
  if (threadIdx.x == 0) tail[wg] = seq;  // commit, then write back: pasted as in k_mgs_one
#pragma unroll
  for (int k = 0; k < E; ++k)
    if (idx[k] >= 0) w[idx[k]] = wv[k];
}
// LDS of the fused kernel: the solve's rows + scratch rows, then sh, tot, G, hc, |w'|^2, the error word
static size_t ilu_mgs_lds_doubles(int ilu_doubles, int e) {
  const int dmax = e <= 8 ? 10 : e == 9 ? 9 : 8;
  return (size_t)ilu_doubles + 4 * MGS_ONE_VALS + MGS_ONE_VALS + MGS_STEPS * (MGS_STEPS + 1) + MGS_STEPS + 2 + (size_t)dmax * e * 64;
}

// entries per thread x basis vectors kept in registers: 8 x 10, 10 x 8, 12 x 6 (round 4: 1.28 M velocity dofs per GPU -- the 10.6 M-DoF mesh
// on 8 GPUs -- need 11.1 entries per thread of the 448-workgroup grid a distributed sweep may use; one GPU: vectors up to 1.57 M entries)
static const void *mgs_one_fn(int e, bool dist = false) {
  constexpr int E0 = MGS_ENTRIES[0], E1 = MGS_ENTRIES[1], E2 = MGS_ENTRIES[2];
  if (dist) return e <= E0 ? (const void *)k_mgs_one<E0, 10, true> : e <= E1 ? (const void *)k_mgs_one<E1, 8, true> : (const void *)k_mgs_one<E2, 6, true>;
  return e <= E0 ? (const void *)k_mgs_one<E0, 10, false> : e <= E1 ? (const void *)k_mgs_one<E1, 8, false> : (const void *)k_mgs_one<E2, 6, false>;
}

// The error word clear, nothing remembered about what the regions hold: what goes with emptied mailboxes
static void mgs_boxes_cleared(nsx_handle *h) {
  MgsState &m = h->mgs;
  *pub_word_host(h, PUB_MGS_ERR) = 0;
  m.used_words[0] = m.used_words[1] = 0;
}
// Both mailbox regions empty, the commit words behind them zero, and the above: a new handle's state
static void mgs_clear_boxes(nsx_handle *h) {
  h->mgs.box.clear(h->stream);
  mgs_boxes_cleared(h);
}
// workgroups that had written their part of w back in sweep `seq` (the streams are idle)
static unsigned int mgs_committed(nsx_handle *h, unsigned long long seq) {
  std::vector<unsigned long long> tail(MGS_TAIL, 0);
  HIP_CHECK(hipMemcpy(tail.data(), h->mgs.box.tail(), MGS_TAIL * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  unsigned int committed = 0;
  for (unsigned long long v : tail) committed += v == seq;
  return committed;
}

void mgs_setup(nsx_handle *h) {
  if (h->mgs.box.allocated() || h->mgs.disabled) return;
  h->mgs.max_wg = 0;
  if (!env_on("NSX_MGS")) {
    h->mgs.disabled = true;
    return;
  }
  h->mgs.box.alloc(MGS_BOX_REGION, MGS_TAIL);
  mgs_clear_boxes(h);
  // NSX_MGS_MAXWG caps every grid limit (tests: a small mesh then needs the instantiations a large one does)
  auto capped = [](int limit) { return env_set("NSX_MGS_MAXWG") ? std::max(1, mgs_maxwg_cap(limit)) : limit; };
  for (int k = 0; k < 3; ++k) {
    const ResidentGrid g = resident_grid(h, mgs_one_fn(MGS_ENTRIES[k]), 256);
    h->mgs.max_wg_e[k] = capped(std::min(MGS_MAX_WG, g.slots()));
    if (nsx_debug()) fprintf(stderr, "[nsx] mgs sweep (%d entries per thread): %d CUs x %d resident workgroups\n", MGS_ENTRIES[k], g.cus, g.per_cu);
  }
  h->mgs.max_wg = h->mgs.max_wg_e[1];
  // distributed instantiations: the collective's own kernels (RCCL's all-reduce, the two one-thread kernels around it) must find a
  // place on the device WHILE the grid is resident and waiting for them: an eighth of the slots (at least 32) stays free
  for (int k = 0; k < 3; ++k) {
    const ResidentGrid g = resident_grid(h, mgs_one_fn(MGS_ENTRIES[k], true), 256);
    const int slots = g.slots();
    h->mgs.max_wg_dist[k] = capped(std::max(0, std::min(MGS_MAX_WG, slots - std::max(32, slots / 8))));
    // on a compute stream that leaves one CU per XCD to the collective's kernel: every shader engine counts as the one that lost a CU
    h->mgs.dist_cap_reserved[k] = capped(std::max(0, std::min(MGS_MAX_WG, g.per_cu * (g.cus - 32))));
  }
  h->mgs.ext_vals.alloc(2 * MGS_EXT_VALS);
  h->mgs.ext_vals.zero(h->stream);
  h->mgs.ext_words.alloc(3);
  h->mgs.ext_words.zero(h->stream);
  h->mgs.ext_expected = 0;
}

// A persistent sweep ended on a timeout (its grid was not co-resident).  Put the handle back into a usable state: wait for the
// stragglers, empty the mailboxes, clear the error words and use the launch-per-link chain from now on.  Returns how many
// workgroups had already written their part of w (0: w is untouched and the sweep can simply be redone by the chain).
static unsigned int mgs_recover(nsx_handle *h, unsigned long long failed_seq) {
  MgsState &m = h->mgs;
  unsigned int committed = 0;
  grid_gave_up(h, m.box, true, "Gram-Schmidt sweep", "link", [&] {
    if (m.ext_vals.p) {
      m.ext_vals.zero(h->stream);
      m.ext_words.zero(h->stream);
      m.ext_expected = 0;
    }
    m.max_wg_dist[0] = m.max_wg_dist[1] = m.max_wg_dist[2] = 0;
    m.dist_fit.clear();
    committed = mgs_committed(h, failed_seq);
    mgs_boxes_cleared(h);
    m.max_wg = m.max_wg_e[0] = m.max_wg_e[1] = m.max_wg_e[2] = 0;
    m.disabled = true;
  });
  return committed;
}

static void mgs_chain(nsx_handle *h, Span sp, double *w, int dim, double *const *vs, int slot0, double *out, bool consider) {
  if (consider) v_dot(h, sp, w, w, slot0 + dim + 1);
  v_dot(h, sp, w, vs[0], slot0);
  for (int i = 1; i < dim; ++i) v_add_and_dot(h, sp, w, -1.0, slot0 + i - 1, vs[i - 1], vs[i], slot0 + i);
  v_add_and_dot(h, sp, w, -1.0, slot0 + dim - 1, vs[dim - 1], w, slot0 + dim);
  read_scalars(h, slot0, dim + 1 + (consider ? 1 : 0), out);
}

// ---- the sweep with TWO collectives (distributed runs) ------------------------------------------------------------------
// With a communicator every link of the chain is a launch plus an all-reduce (dim + 1 collectives per sweep, the reference
// pays one MPI_Allreduce per link as well).  By the linearity that k_mgs_one rests on (derived there), with w the vector as it enters,
//     h_j = v_j . w - sum_{i < j} (v_i . v_j) h_i ,
// so one pass computes r_j = v_j . w for every j and the new row of the basis' Gram matrix (v_{dim-1} . v_i, i < dim - 1; the
// older rows were computed by the earlier sweeps of this GMRES cycle and are kept on the device), ONE all-reduce sums them over
// the ranks, every rank solves the same unit lower-triangular system, and a second pass applies w += (-h_j) v_j for j ascending
// (the chain's operations on every entry, in the chain's order) and leaves the partial sums of |w|^2 for the second all-reduce.
// No orthogonality of the basis is assumed: in exact arithmetic the coefficients ARE the chain's.
constexpr int LS_C = 8;       // basis vectors per pass of the dot kernel
constexpr int LS_VALS = 64;   // r_j at j, Gram row at 32 + i, |w|^2 before the sweep at 63
constexpr int LS_BLOCKS = 2048;  // most workgroups of the dot kernel (partial sums per value)
constexpr int N_TMP_MAX = KRYLOV_N_TMP + 2;

__global__ __launch_bounds__(256) void k_ls_dots(int n, int split, int gap, const double *__restrict__ w, MgsArgs V, int dim, double *__restrict__ partial) {
  __shared__ double sh[4][2 * LS_C + 1];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const double *__restrict__ vl = V.v[dim - 1];
  for (int c0 = 0; c0 < dim; c0 += LS_C) {
    double ar[LS_C], ag[LS_C], aw = 0.0;
#pragma unroll
    for (int k = 0; k < LS_C; ++k) ar[k] = ag[k] = 0.0;
    // (two entries per thread and pass, 2 x (LS_C + 2) loads in flight, measured SLOWER at 10.2 M entries: 228 against 214 us)
    for (int i0 = blockIdx.x * 256 + threadIdx.x; i0 < n; i0 += gridDim.x * 256) {
      const int i = i0 + (i0 >= split ? gap : 0);
      const double wi = w[i], li = vl[i];
#pragma unroll
      for (int k = 0; k < LS_C; ++k)
        if (c0 + k < dim) {
          const double vk = V.v[c0 + k][i];
          ar[k] += wi * vk;
          ag[k] += li * vk;
        }
      aw += wi * wi;
    }
#pragma unroll
    for (int k = 0; k < LS_C; ++k) {
      const double a = gx_wave_sum(ar[k]), b = gx_wave_sum(ag[k]);
      if (lane == 0) sh[wave][k] = a, sh[wave][LS_C + k] = b;
    }
    {
      const double a = gx_wave_sum(aw);
      if (lane == 0) sh[wave][2 * LS_C] = a;
    }
    __syncthreads();
    if (threadIdx.x < 2 * LS_C + 1) {
      const int q = threadIdx.x;
      const double tot = (sh[0][q] + sh[1][q]) + (sh[2][q] + sh[3][q]);
      const int j = c0 + (q < LS_C ? q : q - LS_C);
      if (q < LS_C) {
        if (j < dim) partial[(size_t)j * LS_BLOCKS + blockIdx.x] = tot;
      } else if (q < 2 * LS_C) {
        if (j < dim) partial[(size_t)(32 + j) * LS_BLOCKS + blockIdx.x] = tot;  // j = dim - 1: the diagonal |v_{dim-1}|^2
      } else if (c0 == 0) {
        partial[(size_t)63 * LS_BLOCKS + blockIdx.x] = tot;
      }
    }
    __syncthreads();
  }
}
// vals[v] = fixed-order sum of the LS_BLOCKS partial sums of value v (one workgroup per value; unused values become 0)
__global__ __launch_bounds__(256) void k_ls_finalize(int dim, int nblk, const double *__restrict__ partial, double *__restrict__ vals) {
  __shared__ double sh[4];
  const int v = blockIdx.x;
  const bool used = v < dim || (v >= 32 && v < 32 + dim) || v == 63;
  double a = 0.0;
  if (used)
    for (int q = threadIdx.x; q < nblk; q += 256) a += partial[(size_t)v * LS_BLOCKS + q];
  const double t = gx_block_sum(a, sh);
  if (threadIdx.x == 0) vals[v] = t;
}
// every rank, from the same all-reduced numbers: the new Gram row (diagonal included), then h = (I + L)^-1 r by forward
// substitution, and |w|^2 AFTER the sweep without touching the vectors again:
//     |w - sum_j h_j v_j|^2 = |w|^2 - 2 sum_j h_j r_j + sum_ij h_i G_ij h_j        (G = full Gram matrix of the basis, r_j = v_j . w)
// -- exact algebra, no orthogonality assumed; in floating point a difference of numbers of size |w|^2, so its relative error is
// eps |w|^2 / |w_after|^2: the host takes it when the sweep left more than 1 % of the norm and otherwise pays the second collective
// (scal_out[dim] = |w_after|^2 by the formula, scal_out[dim + 1] = |w|^2 before the sweep).
__global__ __launch_bounds__(64) void k_ls_solve(int dim, const double *__restrict__ vals, double *__restrict__ gram, double *__restrict__ scal_out) {
  __shared__ double G[32][33], hc[32];
  const int t = threadIdx.x;
  for (int i = t; i < dim; i += 64) gram[(dim - 1) * 32 + i] = vals[32 + i];
  __syncthreads();
  for (int q = t; q < dim * 32; q += 64) G[q >> 5][q & 31] = (q & 31) <= (q >> 5) ? gram[q] : 0.0;
  __syncthreads();
  if (t == 0) {
    for (int j = 0; j < dim; ++j) {
      double s = vals[j];
      for (int i = 0; i < j; ++i) s -= G[j][i] * hc[i];
      hc[j] = s;
      scal_out[j] = s;
    }
    double cross = 0.0, quad = 0.0;
    for (int j = 0; j < dim; ++j) {
      cross += hc[j] * vals[j];
      double row = 0.5 * G[j][j] * hc[j];
      for (int i = 0; i < j; ++i) row += G[j][i] * hc[i];
      quad += hc[j] * row;  // half of the symmetric form
    }
    scal_out[dim] = vals[63] - 2.0 * cross + 2.0 * quad;
    scal_out[dim + 1] = vals[63];
  }
}
// w += (-h_j) v_j, j ascending; partial sums of |w|^2
__global__ __launch_bounds__(256) void k_ls_update(int n, int split, int gap, double *__restrict__ w, MgsArgs V, int dim, const double *__restrict__ coef,
                                                   double *__restrict__ partial) {
  __shared__ double hs[32], sh[5];
  if ((int)threadIdx.x < dim) hs[threadIdx.x] = -1.0 * coef[threadIdx.x];
  __syncthreads();
  double acc = 0.0;
  // four entries per thread and pass: the grid is at most 512 workgroups (one partial sum each), so at 10 M entries a thread walks ~80
  // of them, and taken one by one every basis vector was a dependent trip with a single load in flight (262 us per sweep at 10.2 M
  // entries, 3.1 TB/s).  Same operations on every entry in the same order, same order of the squares in the thread's sum: bit-identical.
  constexpr int U = 4;
  const int stride = gridDim.x * 256;
  int i0 = blockIdx.x * 256 + threadIdx.x;
  for (; i0 + (U - 1) * stride < n; i0 += U * stride) {
    int ii[U];
    double wi[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int q = i0 + u * stride;
      ii[u] = q + (q >= split ? gap : 0);
      wi[u] = w[ii[u]];
    }
#pragma unroll 2
    for (int j = 0; j < dim; ++j) {
      const double *__restrict__ vj = V.v[j];
      double x[U];
#pragma unroll
      for (int u = 0; u < U; ++u) x[u] = vj[ii[u]];
#pragma unroll
      for (int u = 0; u < U; ++u) wi[u] += hs[j] * x[u];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      w[ii[u]] = wi[u];
      acc += wi[u] * wi[u];
    }
  }
  for (; i0 < n; i0 += stride) {
    const int i = i0 + (i0 >= split ? gap : 0);
    double wi = w[i];
    for (int j = 0; j < dim; ++j) wi += hs[j] * V.v[j][i];
    w[i] = wi;
    acc += wi * wi;
  }
  const double t = block_sum_256(acc, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

// |w'|^2 = |w|^2 - 2 h.r + h^T G h is a difference of numbers of size |w|^2: its relative error is about eps * dim * |w|^2 / |w'|^2.
// It is accepted when |w'|^2 > guard * |w|^2 (default 1e-2: the norm of the new basis vector is then good to ~1e-13, two orders
// below the tightest tolerance the parity tests solve to); otherwise |w'|^2 is summed over the vector (one more exchange / collective).
static double mgs_norm_guard(const nsx_handle *h) {
  static const double g = env_double("NSX_MGS_NORM_GUARD", 1e-2);
  return h->mgs.guard_override >= 0.0 ? h->mgs.guard_override : g;  // the override: nsx_gram_schmidt_cycle / nsx_gram_schmidt_sweeps (tests)
}

static void mgs_ls_buffers(nsx_handle *h) {
  if (h->mgs.ls_partial.p) return;
  h->mgs.ls_partial.alloc((size_t)LS_VALS * LS_BLOCKS);
  h->mgs.ls_vals.alloc(LS_VALS);
}

static void mgs_lowsync(nsx_handle *h, Span sp, double *w, int dim, double *const *vs, int slot0, double *out, bool consider, double *gram) {
  mgs_ls_buffers(h);
  MgsArgs V;
  for (int i = 0; i < MGS_STEPS; ++i) V.v[i] = i < dim ? vs[i] : nullptr;
  const int n = sp.n;
  {
    LaunchScope ls(h, "mgs_dots", 8.0 * n * (dim + 2.0 * cdiv(dim, LS_C)));
    const int nblk = std::max(1, std::min(LS_BLOCKS, cdiv(n, 1024)));  // depends on the local size only: the values are final before they travel
    hipLaunchKernelGGL(k_ls_dots, dim3(nblk), dim3(256), 0, h->stream, n, sp.split, sp.gap, w, V, dim, h->mgs.ls_partial.p);
    hipLaunchKernelGGL(k_ls_finalize, dim3(LS_VALS), dim3(256), 0, h->stream, dim, nblk, h->mgs.ls_partial.p, h->mgs.ls_vals.p);
  }
  comm_allreduce_partials(h, h->mgs.ls_vals.p, LS_VALS);  // THE collective of the sweep: every r_j, the Gram row and |w|^2 before the sweep
  hipLaunchKernelGGL(k_ls_solve, dim3(1), dim3(64), 0, h->stream, dim, h->mgs.ls_vals.p, gram, h->scal.p + slot0);
  for (int i = 0; i <= dim + 1; ++i) h->slot_nb[slot0 + i] = 0;
  const int nb = red_blocks(h, n);
  {
    LaunchScope ls(h, "mgs_update", 8.0 * n * (dim + 2));
    // the update also leaves the partial sums of |w|^2 (slot S_LS_NORM), in case the formula cannot be trusted
    hipLaunchKernelGGL(k_ls_update, dim3(nb), dim3(256), 0, h->stream, n, sp.split, sp.gap, w, V, dim, h->scal.p + slot0, red_out(h, S_LS_NORM, nb));
  }
  double tmp[N_TMP_MAX + 2];
  read_scalars(h, slot0, dim + 2, tmp);
  // one collective: |w_after|^2 from the Gram algebra, unless the sweep removed more than 99 % of the norm (cancellation)
  const bool by_formula = h->mgs.ls_mode >= 2 && tmp[dim] > mgs_norm_guard(h) * tmp[dim + 1];
  if (!by_formula) {
    after_reduction(h, S_LS_NORM, nb);  // collective 2: |w|^2 summed over the vector
    tmp[dim] = read_scalar(h, S_LS_NORM);
  }
  for (int i = 0; i <= dim; ++i) out[i] = tmp[i];
  if (consider) out[dim + 1] = tmp[dim + 1];
}

// the all-reduced sums of a persistent sweep (r_j at j, Gram row at dim + j, |w|^2 at 2 dim) in the layout of k_ls_solve
__global__ void k_ext_to_ls(int dim, const double *__restrict__ ext_vals, double *__restrict__ ls_vals) {
  const int t = threadIdx.x;  // 64 threads
  double v = 0.0;
  if (t < dim) v = ext_vals[t];
  else if (t >= 32 && t < 32 + dim) v = ext_vals[dim + (t - 32)];
  else if (t == 63) v = ext_vals[2 * dim];
  ls_vals[t] = v;
}

// which vector of the solve a sweep works on: the same answer on every rank, whatever its local sizes (0 velocity, 1 pressure,
// 2 block vector, 3 anything else) -- the key under which choices made by all ranks together are remembered
static int mgs_role(const nsx_handle *h, Span sp) { return sp.split < sp.n ? 2 : sp.n == h->n_u ? 0 : sp.n == h->n_p ? 1 : 3; }

// fused kernel table: NCOMP x (E, DMAX)
static const void *ilu_mgs_fn(int ncomp, int e) {
  if (ncomp == 3) return e <= 8 ? (const void *)k_ilu_mgs<3, 2, 8, 8, 10> : e == 9 ? (const void *)k_ilu_mgs<3, 2, 8, 9, 9> : (const void *)k_ilu_mgs<3, 2, 8, 10, 8>;
  return e <= 8 ? (const void *)k_ilu_mgs<2, 2, 8, 8, 10> : e == 9 ? (const void *)k_ilu_mgs<2, 2, 8, 9, 9> : (const void *)k_ilu_mgs<2, 2, 8, 10, 8>;
}
// May the triangular solves of the velocity ILU(0) and the sweep behind them run as ONE launch (k_ilu_mgs)?  One GPU, the one-exchange
// sweep, the lane-owner stream with two entries per tick, a wave's rows within 256 x 8 or 256 x 10 entries, the grid resident.
// Returns the entries per thread (8 / 10) or 0.
static int ilu_mgs_entries(nsx_handle *h, Span sp, int dim, const double *gram) {
  // Opt-in (NSX_ILU_MGS=1; read per call: the tests switch it inside one process).  Measured at the bench size: 45.7 us per launch
  // against 26.7 + 25.7 for the two separate kernels, 3.05 against 3.18 ms per outer iteration (-4 %) -- and a re-rolled iteration
  // history (the sweep's sums are grouped by rank block): both sampled windows of the chaotic GMRES(28) sequence came out with MORE
  // restart steps (driver window 25.4 against 21.9 outer iterations per step, 325 steps 30.4 against 28.0), i.e. slower per time step.
  // The default therefore stays with the separate kernels and rounds 3-4's history.
  const bool wanted = ilu_mgs_wanted();
  const IluSchedule &s = h->schedF;
  if (!wanted || h->comm || h->mgs.disabled || !h->mgs.box.allocated() || !gram || dim + 2 > MGS_STEPS) return 0;
  if (sp.n != h->n_u || sp.split != sp.n || sp.gap != 0 || (h->dim != 2 && h->dim != 3)) return 0;
  if (!s.packed_ok || s.levelled || s.stream_ncomp != h->dim || s.stream_epl != 2 || s.n_waves < 1 || s.n_waves > MGS_MAX_WG) return 0;
  if (ilu_lanes_pf() != 8) return 0;  // (the fused kernel keeps 8 slabs in flight)
  // entries per thread x basis vectors kept in registers: 8 x 10, 9 x 9 (the bench layout: 747 rows in its largest wave), 10 x 8
  const int entries = s.max_wave_rows * h->dim, e = entries <= 256 * 8 ? 8 : entries <= 256 * 9 ? 9 : entries <= 256 * 10 ? 10 : 0;
  if (!e) return 0;
  const int k = e - 8;
  if (h->mgs.ilu_cap[k] < 0 || h->mgs.ilu_cap_rows != s.max_wave_rows) {  // resident-grid limit with this schedule's LDS request
    if (h->mgs.ilu_cap_rows != s.max_wave_rows) h->mgs.ilu_cap[0] = h->mgs.ilu_cap[1] = h->mgs.ilu_cap[2] = -1;
    h->mgs.ilu_cap_rows = s.max_wave_rows;
    const size_t shm = ilu_mgs_lds_doubles((s.max_wave_rows + 64) * h->dim, e) * sizeof(double);
    if (shm > 80 * 1024) h->mgs.ilu_cap[k] = 0;
    else {
      if (shm > 64 * 1024) HIP_CHECK(hipFuncSetAttribute(ilu_mgs_fn(h->dim, e), hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm));  // (160 KB per CU on gfx950; the runtime's default limit per workgroup is 64 KB)
      h->mgs.ilu_cap[k] = mgs_maxwg_cap(std::min(MGS_MAX_WG, resident_grid(h, ilu_mgs_fn(h->dim, e), 256, shm).slots()));
    }
    if (nsx_debug())
      fprintf(stderr, "[nsx] triangular solves + sweep in one launch (%d entries per thread, %zu B of LDS): %d resident workgroups for %d waves of the solve\n", e, shm,
              h->mgs.ilu_cap[k], s.n_waves);
  }
  return s.n_waves <= h->mgs.ilu_cap[k] ? e : 0;
}

MgsPick mgs_pick(int n, const int *caps, int n_inst, const int *es) {
  MgsPick p;
  for (int k = 0; k < n_inst; ++k) {
    if (caps[k] <= 0) continue;
    p.nwg = std::max(1, std::min(caps[k], cdiv(n, 256 * 4)));
    p.per_thread = cdiv(n, (int64_t)p.nwg * 256);
    p.e = es[k];
    if (p.per_thread <= es[k]) break;
  }
  return p;
}

// What one call of v_mgs runs: decided (distributed: together with the other ranks) before anything of the sweep is launched
struct MgsPlan {
  int fused_e = 0;          // > 0: k_ilu_mgs with that many entries per thread (the velocity triangular solves inside the sweep's launch)
  bool dist = false;        // k_mgs_one<.., true>: the ranks' collective inside the persistent grid
  MgsPick pick;             // instantiation and grid of the persistent sweep
  bool persistent = false;  // false: no persistent sweep for this vector ...
  bool two_pass = false;    // ... then the two-pass sweep is wanted (mgs_fallback)
};

// Every agreement below is ONE collective that all ranks enter in the same order (comm_streams_concurrent, comm_agree_all,
// comm_reserve_cus): each condition in front of one is an answer the ranks gave together, or the same on all of them by construction.
static MgsPlan mgs_plan(nsx_handle *h, Span sp, int dim, const double *gram, int fused_e) {
  MgsState &m = h->mgs;
  const int n = sp.n;
  MgsPlan p;
  p.fused_e = fused_e;
  // distributed run: the persistent sweep with the collective inside its exchange (k_mgs_one<.., true>) needs stream collectives
  // (RCCL), the Gram cache and room on the device; NSX_MGS_DIST=0 keeps the two-pass sweep (mgs_lowsync)
  if (h->comm && m.dist_state < 0) {  // decided once per handle, by all ranks together (comm_streams_concurrent)
    const bool wanted = env_on("NSX_MGS_DIST");
    m.dist_state = (wanted && comm_on_stream(h) && comm_streams_concurrent(h)) ? 1 : 0;
  }
  bool dist = h->comm && m.dist_state == 1 && !m.disabled && gram;
  if (!h->comm || dist) mgs_setup(h);
  dist = dist && 2 * dim + 1 < MGS_EXT_LEAVE;
  // entries per thread: the smallest instantiation (MGS_ENTRIES: 8, 10, 12) whose resident grid covers the vector.
  // With the collective inside the grid only the 8-entry instantiation: it holds 246 VGPRs (248 allocated), so a CU that carries
  // ONE of its workgroups keeps 264 registers per SIMD lane free -- exactly what a wave of RCCL's generic kernel needs (264; 256
  // threads, 19.7 KB of LDS) -- and the grid limit leaves such CUs (mgs_setup).  The 10- and 12-entry instantiations allocate 256:
  // RCCL's kernel finds no place beside them and the sweep times out (measured with a self-addressed send / receive in front of the
  // collective, tools/r04_self_p2p.sh: level 5, 8 entries: 23.0 -> 30.9 us per sweep, no fallback; level 7, 10 entries: time-out)
  // ... unless the compute stream leaves one CU per XCD to the communication stream (comm_reserve_cus, below): then any instantiation
  const bool only8 = dist && !h->cu_reserved;
  p.pick = mgs_pick(n, dist ? (h->cu_reserved ? m.dist_cap_reserved : m.max_wg_dist) : m.max_wg_e, m.max_wg ? (only8 ? 1 : 3) : 0, MGS_ENTRIES);
  int per_thread_max = MGS_ENTRIES[only8 ? 0 : 2];
  const int role = mgs_role(h, sp);
  if (only8 && !h->cu_reserve_failed && m.dist_fit.find(role) == m.dist_fit.end()) {
    // too long for the 8-entry grid somewhere, but not for the larger instantiations on a masked compute stream?  NSX_COMM_CU_RESERVE:
    // 0 never, 1 (default) when that is what keeps the collective inside the grid, 2 always.  Every condition below is an answer all
    // ranks gave together, so every rank takes the same steps -- including the outcome of the reservation itself: if it fails anywhere
    // (no masked stream, the probe) every rank goes back to its plain streams and nobody asks again on this communicator.
    static const int reserve = env_int("NSX_COMM_CU_RESERVE", 1);
    const bool fits8 = p.pick.e != 0 && p.pick.per_thread <= 8;
    const bool fits_reserved = mgs_pick(n, m.dist_cap_reserved, 3, MGS_ENTRIES).fits();
    const bool all8 = reserve > 0 ? comm_agree_all(h, fits8) : true;
    if (reserve > 0 && (reserve > 1 || !all8) && comm_agree_all(h, fits_reserved)) {
      const bool mine = comm_reserve_cus(h);
      if (!comm_agree_all(h, mine)) {
        if (mine) comm_release_cus(h);
        h->cu_reserve_failed = true;
      }
      if (h->cu_reserved) {  // choose the instantiation again, with the masked stream's limits
        per_thread_max = MGS_ENTRIES[2];
        p.pick = mgs_pick(n, m.dist_cap_reserved, 3, MGS_ENTRIES);
      }
    }
  }
  if (dist) {
    // does the resident grid hold the vector -- on EVERY rank?  (local lengths differ; a rank on the two-pass sweep and a rank on the
    // persistent one would all-reduce differently laid-out buffers.)  Agreed once per role of the vector in the solve.
    auto it = m.dist_fit.find(role);
    if (it == m.dist_fit.end()) it = m.dist_fit.emplace(role, comm_agree_all(h, p.pick.e != 0 && p.pick.per_thread <= per_thread_max) ? 1 : 0).first;
    if (!it->second || dim + 2 > MGS_STEPS) dist = false;
  }
  p.dist = dist;
  // no persistent sweep: a distributed solve off the in-grid collective, no resident grid, too many vectors for the mailbox rows, a vector
  // too long for the largest instantiation, or no Gram cache for the one-exchange sweep
  p.persistent = fused_e || !((h->comm && !dist) || m.max_wg == 0 || dim + 2 > MGS_STEPS || p.pick.per_thread > per_thread_max || !gram);
  // (one GPU, vector too long for the persistent sweep: the same two passes read the basis twice instead of four times)
  p.two_pass = h->comm || (!m.disabled && p.pick.per_thread > per_thread_max);
  if (fused_e) p.pick.nwg = h->schedF.n_waves, p.pick.e = p.pick.per_thread = fused_e;
  return p;
}

// The sweep without a persistent grid.  two_pass: two collectives per sweep (mgs_lowsync) instead of one per link; NSX_MGS_LOWSYNC=0:
// one launch + all-reduce per link, as the reference's MPI run does.  Without a Gram cache (or too many vectors for it) the chain as well.
static void mgs_fallback(nsx_handle *h, Span sp, double *w, int dim, double *const *vs, int slot0, double *out, bool consider, double *gram, bool two_pass) {
  if (h->mgs.ls_mode < 0) h->mgs.ls_mode = env_int("NSX_MGS_LOWSYNC", 2);  // read once per handle: 0 chain, 1 two collectives, 2 one
  if (two_pass && h->mgs.ls_mode && gram && dim <= KRYLOV_N_TMP + 1) mgs_lowsync(h, sp, w, dim, vs, slot0, out, consider, gram);
  else mgs_chain(h, sp, w, dim, vs, slot0, out, consider);
}

// development (tools/r05_ilu_mgs_trace.sh): the wall-clock stamps every wave of ONE k_ilu_mgs launch left in `buf`, as a text file
static void ilu_mgs_trace_dump(nsx_handle *h, const DevBuf<unsigned long long> &buf, const char *path, int dim, int nwg, int e) {
  std::vector<unsigned long long> tr((size_t)nwg * 4 * 16);
  buf.download(tr.data(), tr.size(), h->stream);
  FILE *f = fopen(path, "w");
  if (!f) return;
  fprintf(f, "# k_ilu_mgs launch %d: dim %d, %d workgroups, %d entries per thread; per wave: workgroup wave rows, then stamps 0..8 in ticks of 10 ns relative to the grid's first stamp\n"
             "# 0 start, 1 rhs rows in LDS, 2 forward sweep done, 3 backward sweep done (sweeping wave only), 4 basis entries arrived, 5 z complete (barrier), 6 local sums, 7 totals picked up, 8 update done\n",
          h->mgs.fused_launches, dim, nwg, e);
  unsigned long long t0 = ~0ull;
  for (size_t q = 0; q < tr.size(); q += 16)
    if (tr[q]) t0 = std::min(t0, tr[q]);
  std::vector<int32_t> rp((size_t)nwg + 1);
  h->schedF.pk_row_ptr.download(rp.data(), rp.size(), h->stream);
  for (int b = 0; b < nwg; ++b)
    for (int wv_ = 0; wv_ < 4; ++wv_) {
      fprintf(f, "%d %d %d", b, wv_, rp[b + 1] - rp[b]);
      for (int k = 0; k < 9; ++k) {
        const unsigned long long v = tr[((size_t)b * 4 + wv_) * 16 + k];
        fprintf(f, " %lld", v ? (long long)(v - t0) : -1ll);
      }
      fprintf(f, "\n");
    }
  fclose(f);
}

// Launch the planned persistent sweep `seq` (distributed: and enqueue its collective).  Returns the buffer that collective works on, else null.
// Co-residency: the grid never exceeds what the device holds at once (mgs_setup), the stream is in-order and normally nothing
// else runs on the device, so a plain launch places every workgroup at once.  (hipLaunchCooperativeKernel was an option until
// round 3: it adds a launch-time size check and ~20 us of cross-queue synchronisation per launch but no residency guarantee
// beyond that and was removed.)  What makes the sweep safe is the bounded wait: should a workgroup be missing (another stream or
// process holds compute units), the kernel ends without writing w and the sweep is redone without a persistent grid (v_mgs).
static double *mgs_launch(nsx_handle *h, const MgsPlan &p, Span sp, double *w, int dim, double *const *vs, int slot0, bool normalize, bool consider, double *gram,
                          const double *ilu_rhs, unsigned long long seq) {
  MgsState &m = h->mgs;
  const int n = sp.n, nwg = p.pick.nwg, fused_e = p.fused_e;
  m.last_e = p.pick.e;
  m.last_fused = fused_e ? 1 : 0;
  m.fused_launches += fused_e ? 1 : 0;
  m.last_nwg = nwg;
  m.last_dist = p.dist ? 1 : 0;
  m.max_e_seen = std::max(m.max_e_seen, p.pick.e);
  LaunchScope ls(h, fused_e ? "ilu_mgs" : "mgs_sweep",
                 8.0 * n * (dim + 2) + (fused_e ? 12.0 * (double)h->schedF.in_block_nnz + (double)h->N2 * (4 + 8.0 * h->dim) - 8.0 * n : 0.0));
  MgsArgs V;
  for (int i = 0; i < MGS_STEPS; ++i) V.v[i] = i < dim ? vs[i] : nullptr;
  int n_ = n, split = sp.split, gap = sp.gap, dim_ = dim, norm_ = normalize ? 1 : 0, consider_ = consider ? 1 : 0;
  const int parity = m.box.parity;
  unsigned long long *box = m.box.cur(), *box_next = m.box.other();
  double *sout = h->scal.p + slot0, *pub_vals = h->pub_dev + slot0;
  unsigned long long *pub_flag = pub_word_dev<unsigned long long>(h, PUB_FLAG), seq_ = seq;
  int *err = pub_word_dev(h, PUB_MGS_ERR);  // mapped host word
  unsigned long long *tail = m.box.tail();
  int reset_words = m.used_words[1 - parity];  // what the other region's last user filled: this launch empties it for the next one
  int drop_wg = h->gx_drop_wg;
  double *gram_ = gram, guard_ = mgs_norm_guard(h);
  double *ext_vals_this = nullptr;
  const void *fn = fused_e ? ilu_mgs_fn(h->dim, fused_e) : mgs_one_fn(p.pick.e, p.dist);
  if (fused_e) {
    const IluSchedule &s_ = h->schedF;
    IluMgsArgs I{s_.pk_row_ptr.p, s_.pk_rows.p, s_.pk_slab_ptr.p, reinterpret_cast<const uint32_t *>(s_.pk_meta.p), s_.pk_val.p, s_.pk_dinv.p, ilu_rhs,
                 (s_.max_wave_rows + 64) * h->dim, nullptr};
    // development: wall-clock stamps of every wave of ONE launch (the NSX_ILU_MGS_TRACE_CALL-th, default 3000)
    DevBuf<unsigned long long> trace_buf;
    const char *trace_path = getenv("NSX_ILU_MGS_TRACE");
    const bool traced = trace_path && m.fused_launches == env_int("NSX_ILU_MGS_TRACE_CALL", 3000);
    if (traced) {
      trace_buf.alloc((size_t)nwg * 4 * 16);
      trace_buf.zero(h->stream);
      I.trace = trace_buf.p;
    }
    const size_t shm = ilu_mgs_lds_doubles(I.ilu_doubles, fused_e) * sizeof(double);
    void *args[] = {&n_, &w, &V, &dim_, &gram_, &box, &box_next, &reset_words, &sout, &err, &tail, &norm_, &consider_, &pub_vals, &pub_flag, &seq_, &drop_wg, &guard_, &I};
    HIP_CHECK(hipLaunchKernel(fn, dim3(nwg), dim3(256), args, shm, h->stream));
    if (traced) ilu_mgs_trace_dump(h, trace_buf, trace_path, dim, nwg, fused_e);
  } else {
    MgsExt ext{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0};
    if (p.dist) {
      ext.leave = m.leave_req ? 1 : 0;
      ext.vals = m.ext_vals.p + (size_t)m.ext_parity * MGS_EXT_VALS;
      ext.vals_other = m.ext_vals.p + (size_t)(1 - m.ext_parity) * MGS_EXT_VALS;
      ext.flag = m.ext_words.p;
      ext.arrive = (unsigned int *)(m.ext_words.p + 1);
      ext.abort_seq = m.ext_words.p + 2;
      ext.norm_out = h->scal.p + S_LS_NORM;
      ext_vals_this = ext.vals;
    }
    void *args[] = {&n_, &split, &gap, &w, &V, &dim_, &gram_, &box, &box_next, &reset_words, &sout, &err, &tail, &norm_, &consider_, &pub_vals, &pub_flag, &seq_, &drop_wg, &guard_, &ext};
    HIP_CHECK(hipLaunchKernel(fn, dim3(nwg), dim3(256), args, 0, h->stream));
    if (p.dist) {
      // the collective of this sweep, on the communication stream: it starts when the grid's 2 dim + 1 reducers have delivered
      m.ext_expected += (unsigned int)(2 * dim + 1);
      comm_ext_allreduce(h, ext.vals, MGS_EXT_VALS, MGS_EXT_FAIL, ext.arrive, m.ext_expected, ext.flag, seq);
      m.ext_parity ^= 1;
      h->slot_nb[S_LS_NORM] = 0;
    }
  }
  // this launch fills the mailboxes box[v * nwg + wg] of the 2 dim + 1 values of the single exchange (+ 1 for the explicit norm); the other region is empty now
  m.used_words[parity] = (2 * dim + 2) * nwg;
  m.used_words[1 - parity] = 0;
  m.box.flip();
  for (int i = 0; i <= dim + 1; ++i) h->slot_nb[slot0 + i] = 0;
  return ext_vals_this;
}

// A distributed persistent sweep raised the error word.  Whose verdict was it?  Wait for the collective (the grid is gone, so its kernels
// find room whatever kept them) and look at the words it summed: a failure or a leave request is known to every rank alike -- all redo the
// sweep in two passes (returns false: nothing done here).  Neither: only THIS rank's grid gave up on the flag; its peers may be past this
// sweep already, so this rank must not change its collective sequence: the sweep is finished here from the global sums the (late)
// collective delivered, and the next sweep asks all ranks to leave the persistent path (returns true: out[] is filled, w not normalised).
static bool mgs_finish_late(nsx_handle *h, Span sp, double *w, int dim, double *const *vs, int slot0, double *out, bool consider, double *gram,
                            const double *ext_vals, unsigned long long seq) {
  MgsState &m = h->mgs;
  HIP_CHECK(hipStreamSynchronize(h->stream));
  HIP_CHECK(hipStreamSynchronize(h->comm_stream));
  double words[2] = {0.0, 0.0};
  HIP_CHECK(hipMemcpy(words, ext_vals + MGS_EXT_LEAVE, 2 * sizeof(double), hipMemcpyDeviceToHost));
  if (words[0] != 0.0 || words[1] != 0.0) return false;
  const unsigned int committed = mgs_committed(h, seq);
  if (committed != 0) NSX_THROW(NSX_ERR_HIP, "Gram-Schmidt sweep: %u workgroups had written w when another one gave up on the collective", committed);
  if (++m.local_timeouts > 2)
    NSX_THROW(NSX_ERR_COMM, "Gram-Schmidt sweep: the collective inside the persistent grid did not arrive within %.0f s for the third time on rank %d", 1e-8 * (double)GX_EXT_TIMEOUT_TICKS, h->rank);
  fprintf(stderr, "[nsx] warning: rank %d: the collective inside the Gram-Schmidt sweep came too late for its grid (%.0f s): this sweep is finished from the sums it delivered, "
                  "and all ranks are asked to use the two-pass sweep from the next one on\n", h->rank, 1e-8 * (double)GX_EXT_TIMEOUT_TICKS);
  // mailboxes and error word as a new handle's; the words of the collective protocol (arrival count, flag, abort word) stay: they are cumulative
  mgs_clear_boxes(h);
  h->n_persistent_fallbacks++;
  m.leave_req = true;
  // the sweep itself, from the global sums: coefficients and |w'|^2 as every grid computed them (k_ls_solve evaluates the same formula
  // in another grouping: a decision on its threshold's knife edge could differ from the peers' in the last bit), then the updates
  mgs_ls_buffers(h);
  MgsArgs V;
  for (int i = 0; i < MGS_STEPS; ++i) V.v[i] = i < dim ? vs[i] : nullptr;
  const int n = sp.n;
  hipLaunchKernelGGL(k_ext_to_ls, dim3(1), dim3(64), 0, h->stream, dim, ext_vals, m.ls_vals.p);
  hipLaunchKernelGGL(k_ls_solve, dim3(1), dim3(64), 0, h->stream, dim, m.ls_vals.p, gram, h->scal.p + slot0);
  for (int i = 0; i <= dim + 1; ++i) h->slot_nb[slot0 + i] = 0;
  const int nb = red_blocks(h, n);
  hipLaunchKernelGGL(k_ls_update, dim3(nb), dim3(256), 0, h->stream, n, sp.split, sp.gap, w, V, dim, h->scal.p + slot0, red_out(h, S_LS_NORM, nb));
  h->slot_nb[S_LS_NORM] = nb > 1 ? nb : 0;
  double tmp[N_TMP_MAX + 2];
  read_scalars(h, slot0, dim + 2, tmp);
  if (!(tmp[dim] > mgs_norm_guard(h) * tmp[dim + 1])) {  // the peers' grids refused the formula as well: the sweep's second collective
    finalize_slots(h, S_LS_NORM, 1);
    comm_allreduce_scalars(h, S_LS_NORM, 1);
    tmp[dim] = read_scalar(h, S_LS_NORM);
  }
  h->slot_nb[S_LS_NORM] = 0;
  for (int i = 0; i <= dim; ++i) out[i] = tmp[i];
  if (consider) out[dim + 1] = tmp[dim + 1];
  return true;
}

// out[0..dim) = h(i), out[dim] = |w|^2 after the sweep.  normalized: w was also normalised (only if asked to).
MgsResult v_mgs(nsx_handle *h, Span sp, double *w, int dim, double *const *vs, int slot0, bool normalize, double *out,
                const std::function<void()> *after_launch, bool consider, double *gram, const double *ilu_rhs) {
  MgsState &m = h->mgs;
  // ilu_rhs: w = (LU)^-1 ilu_rhs (the velocity ILU(0) of the last initialisation) comes FIRST -- inside the sweep's launch when
  // that is possible (k_ilu_mgs), as the separate kernel otherwise
  int fused_e = 0;
  if (ilu_rhs) {
    if (!h->comm) mgs_setup(h);
    fused_e = ilu_mgs_entries(h, sp, dim, gram);
    if (!fused_e) ilu_solve(h, h->gA, h->schedF, h->luF.p, ilu_rhs, w, h->dim, "ilu_solve_F");
  }
  const MgsPlan p = mgs_plan(h, sp, dim, gram, fused_e);
  if (!p.persistent) {
    mgs_fallback(h, sp, w, dim, vs, slot0, out, consider, gram, p.two_pass);
    return {false, false};
  }
  const unsigned long long seq = ++h->pub_seq;
  const double *ext_vals = mgs_launch(h, p, sp, w, dim, vs, slot0, normalize, consider, gram, ilu_rhs, seq);
  // w is final (and normalised) once the kernel has run: work that only depends on it may be enqueued before the host
  // has the coefficients
  const bool ran_ahead = normalize && !consider && after_launch;
  if (ran_ahead) (*after_launch)();
  wait_published(h, seq);
  if (*pub_word_host(h, PUB_MGS_ERR)) {  // the grid gave up (a bounded wait ran out) and left w as it was
    if (!(p.dist && mgs_finish_late(h, sp, w, dim, vs, slot0, out, consider, gram, ext_vals, seq))) {
      const unsigned int committed = mgs_recover(h, seq);
      if (committed != 0) NSX_THROW(NSX_ERR_HIP, "Gram-Schmidt sweep: %u workgroups had written w when another one timed out", committed);
      if (p.dist) {  // the failure word travelled through the collective, so every rank is here and redoes the sweep in two passes
        m.leave_req = false;
        mgs_fallback(h, sp, w, dim, vs, slot0, out, consider, gram, true);
      } else {
        if (fused_e) ilu_solve(h, h->gA, h->schedF, h->luF.p, ilu_rhs, w, h->dim, "ilu_solve_F");  // the fused launch ended without writing w: z first, then the chain
        mgs_chain(h, sp, w, dim, vs, slot0, out, consider);
      }
    }
    // what after_launch enqueued (the next operator application) used the unfinished w: its result is a temporary that the
    // caller recomputes when told so
    return {false, ran_ahead};
  }
  for (int i = 0; i <= dim + 1; ++i) out[i] = h->pub_host[slot0 + i];
  if (p.dist && h->pub_host[slot0 + dim + 2] != 0.0) {
    // the Gram formula for |w'|^2 was refused (alike on every rank): the grid left its local sum in the scalar slot and did not
    // normalise; the second collective of the sweep sums it over the ranks.  (A NaN -- a mailbox of that sum timed out somewhere --
    // is replaced by a plain dot product: w itself is complete.)
    comm_allreduce_scalars(h, S_LS_NORM, 1);
    double nrm2 = read_scalar(h, S_LS_NORM);
    if (nrm2 != nrm2) {
      v_dot(h, sp, w, w, S_LS_NORM);
      nrm2 = read_scalar(h, S_LS_NORM);
    }
    out[dim] = nrm2;
    return {false, ran_ahead};  // what was enqueued behind the launch used the unnormalised w
  }
  if (!normalize) return {false, false};
  // the kernel's own decision, recomputed from the same two numbers
  return {!consider || !mgs_wants_second_sweep(std::sqrt(out[dim]), out[dim + 1]), false};
}

// The Gram matrices of the GMRES bases, one 32 x 32 block per nesting level (depth < 4), zeroed when first asked for
double *mgs_gram(nsx_handle *h, int depth) {
  if (!h->mgs.ls_gram.p) {
    h->mgs.ls_gram.alloc(4 * 1024);
    h->mgs.ls_gram.zero(h->stream);
  }
  return h->mgs.ls_gram.p + (size_t)depth * 1024;
}

// diagnostics (nsx_persistent_state): words of the region the next sweep would use that are not empty.  A healthy handle keeps
// that region empty (every launch clears the other region for its successor); after a time-out mgs_recover clears both.
int mgs_dirty_words(nsx_handle *h) { return h->mgs.box.dirty_words(h); }

}  // namespace nsx

// One GMRES cycle's worth of orthogonalisation on the caller's vectors, through the very sweep the solvers use (v_mgs with the
// basis' Gram matrix kept on the device): vectors[0] is normalised, vectors[k] is swept against the k vectors in front of it and
// normalised.  norm_guard >= 0 replaces the threshold below which the Gram formula for |w'|^2 is refused (0: always the formula,
// 1e300: always the explicitly summed norm); < 0 keeps the handle's.  For the tests of that formula (tests/test_gpu_errors.py).
extern "C" int nsx_gram_schmidt_cycle(nsx_handle *h, int n, int m, double *vectors, double norm_guard, double *coeffs, double *norms2) {
  if (m < 1 || m > nsx::KRYLOV_N_TMP) return NSX_ERR_ARG;
  double before[nsx::KRYLOV_N_TMP + 2];
  int normalized[nsx::KRYLOV_N_TMP + 2];
  return nsx_gram_schmidt_sweeps(h, n, n, 0, m, vectors, norm_guard, 0, coeffs, norms2, before, normalized);  // Span(n), consider = false, normalize = true
}

// The cycle itself, with the arguments of v_mgs that nsx_gram_schmidt_cycle fixes: the vectors live in the device layout of a
// Span(n, split, gap) (the distributed block vector's: logical entry i at i + (i >= split ? gap : 0); the gap entries travel up
// and down untouched by the hook), flags bit 0 = consider (|w|^2 before the sweep in out[dim + 1], and the sweep's own decision
// whether it may normalise), flags bit 1 = do not normalise inside the sweep.  ONE sweep per vector: where v_mgs reports that it
// did not normalise, the vector is scaled here with the norm the sweep returned, so the basis stays orthonormal for the later
// sweeps.  For tests/test_gpu_mgs_sweep.py.
extern "C" int nsx_gram_schmidt_sweeps(nsx_handle *h, int n, int split, int gap, int m, double *vectors, double norm_guard, int flags, double *coeffs,
                                       double *norms2, double *norms2_before, int *normalized) {
  if (!h || !vectors || !coeffs || !norms2 || !norms2_before || !normalized || n < 1 || m < 1 || m > nsx::KRYLOV_N_TMP || split < 0 || split > n || gap < 0 ||
      (flags & ~3) != 0 || (split == n && gap != 0))
    return NSX_ERR_ARG;
  NSX_TRY(h)
  HIP_CHECK(hipSetDevice(h->prm.device));
  const size_t len = (size_t)n + gap;
  std::vector<nsx::DevBuf<double>> v(m);
  for (int k = 0; k < m; ++k) v[k].upload(vectors + (size_t)k * len, len, h->stream);
  double *gram = nsx::mgs_gram(h, 0);
  const bool consider = (flags & 1) != 0, normalize = (flags & 2) == 0;
  const double keep = h->mgs.guard_override;
  h->mgs.guard_override = norm_guard;
  try {
    const nsx::Span sp(n, split, gap);
    nsx::v_dot(h, sp, v[0].p, v[0].p, nsx::S_NRM);
    norms2[0] = norms2_before[0] = nsx::read_scalar(h, nsx::S_NRM);
    normalized[0] = 0;
    nsx::v_scale(h, sp, v[0].p, 1.0 / std::sqrt(norms2[0]));
    for (int k = 1; k < m; ++k) {
      double *vs[nsx::KRYLOV_N_TMP + 2], out[nsx::KRYLOV_N_TMP + 4];
      for (int i = 0; i < k; ++i) vs[i] = v[i].p;
      const bool done = nsx::v_mgs(h, sp, v[k].p, k, vs, nsx::S_H, normalize, out, nullptr, consider, gram).normalized;
      for (int i = 0; i < k; ++i) coeffs[(size_t)k * m + i] = out[i];
      norms2[k] = out[k];
      norms2_before[k] = consider ? out[k + 1] : 0.0;
      normalized[k] = done ? 1 : 0;
      if (!done && out[k] > 0.0) nsx::v_scale(h, sp, v[k].p, 1.0 / std::sqrt(out[k]));
    }
  } catch (...) {
    h->mgs.guard_override = keep;
    throw;
  }
  h->mgs.guard_override = keep;
  for (int k = 0; k < m; ++k) v[k].download(vectors + (size_t)k * len, len, h->stream);
  NSX_CATCH(h)
}
