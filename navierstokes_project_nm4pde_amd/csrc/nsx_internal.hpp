// nsx_internal.hpp — private state of a libnsx handle (C-ABI: include/nsx.h).
//
// HBM layout (all FP64 values, int32 indices; N2 = scalar P2 nodes, NP = P1 nodes, dim components interleaved):
//   vectors        [n_u + n_p] = [N2][dim] velocity (node-major, components consecutive) then [NP] pressure
//   A-graph        scalar P2 x P2 CSR (rowptr/colind/diag position); value arrays on it:
//                  S0 = M/dt + nu K (static), Mass = M/dt, Stiff = nu K, Conv = C(u_n), F = system(0,0), LU_F
//                  -> the reference stores dim^2 x as many entries (all component couplings, NS3D.cpp:109-119);
//                     every velocity-velocity term is delta_cd (x) scalar, so one scalar operator serves dim components.
//   G-graph        P2 x P1 CSR, dim values per entry: block (0,1) = -int psi_k d_c phi_i   (NS3D.cpp:258)
//   B-graph        P1 x P2 CSR, dim values per entry: block (1,0) = +int psi_k d_c phi_j   (NS3D.cpp:261)
//   S-graph        P1 x P1 CSR = structural product B*G: negative_S_tilde and its ILU(0)   (Prec.hpp:144,358)
//   cell tables    SoA: cell_n2[a][cell], cell_n1[v][cell], geo[k][cell] (J^-1 row-major, then |det J|)
//                  probe.cell_x0[d][cell] (vertex 0: x = X0 + J lambda, the point probes' search; ProbeState)
//                  tracer.cell_nbr[k][cell] (cell across the face opposite local vertex k, -1: boundary; the tracers' walk, built on demand; TracerState)
//   patch table    per owned P2 node the (cell, local node) pairs that hold it, ascending cell, in tiles of 64 nodes of (nearly) one
//                  patch size (the nodal fields' gather, built on demand: host/nodal_patch.hpp; NodalState)
//   iso tables     iso.cellx[(v dim + d)][cell] vertex coordinates, node maps in the internal numbering (P2 node -> P1 nodes, position, slot of
//                  the nodal results), built on demand (the isosurface extraction: nsx_iso.hip; IsoState)
//   stats planes   per phase bin and owned node, in the caller's numbering: mean and co-moment of velocity and pressure (the running statistics:
//                  nsx_stats.hip; StatsState)
//   surface tables per boundary face of the installed set, sorted by group: cell, local face, normal, height, measure, node positions; the patch
//                  lists of the surface nodes in tiles of 64; planes of the last results (the surface loads: nsx_surface.hip; SurfaceState)
//   gather maps    per CSR entry the list of (local entry, cell) contributions -> deterministic assembly, no atomics
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <map>
#include <string>
#include <functional>
#include <type_traits>
#include <vector>

#include "../../include/nsx.h"
#include "../host/graph.hpp"

// Cache policy (compile time, -DNSX_NT=mask): non-temporal loads for 1 = the Krylov basis in the Gram-Schmidt sweep,
// 2 = the matrix stream of the LDS-staged SpMV, 4 = the factor stream of the packed triangular solve.  An inner GMRES
// iteration on F streams F (126 MB), the ILU factors (130 MB) and the basis (17 - 125 MB) once each: more than the 256-MiB
// Infinity Cache holds, so with default-policy loads every stream evicts the next one's lines.  Measured per mask
// (tools/nt_sweep.sh, us per launch SpMV / triangular solve / sweep): 0: 34.2 / 34.4 / 35.2; 1: 30.6 / 32.8 / 35.7;
// 4: 30.7 / 35.1 / 32.8; 2: 39.5 / 33.4 / 33.0 (the 2-byte index stream does not like nt); 6, 7: worse.
#ifndef NSX_NT
#define NSX_NT 1
#endif
template <int BIT, class T>
__device__ __forceinline__ T ld_stream(const T *p) {
  if constexpr ((NSX_NT & BIT) != 0) return __builtin_nontemporal_load(p);
  else return *p;
}

namespace nsx {

struct Error {
  int code;
  std::string msg;
};

#define NSX_THROW(code_, ...)                              \
  do {                                                     \
    char buf_[512];                                        \
    snprintf(buf_, sizeof(buf_), __VA_ARGS__);             \
    throw ::nsx::Error{(code_), std::string(buf_)};        \
  } while (0)

// THE guard of every extern "C" entry that takes a handle: NSX_TRY(h) <body> NSX_CATCH(h).  A null handle is NSX_ERR_ARG; nsx::Error becomes
// its code, any other std::exception (bad_alloc / length_error of a vector sized by the caller) NSX_ERR_ARG with what() as the message;
// nothing unwinds through the C frame.  NSX_CATCH_TO is the same pair of handlers for an entry that has no handle yet (nsx_create) or has
// work to do behind them: the message goes to err_, the optional statements run before the return.
#define NSX_TRY(h_)              \
  if (!(h_)) return NSX_ERR_ARG; \
  try {
#define NSX_CATCH_TO(err_, ...)       \
  }                                   \
  catch (const nsx::Error &e) {       \
    err_ = e.msg;                     \
    __VA_ARGS__;                      \
    return e.code;                    \
  }                                   \
  catch (const std::exception &e) {   \
    err_ = e.what();                  \
    __VA_ARGS__;                      \
    return NSX_ERR_ARG;               \
  }
#define NSX_CATCH(h_) NSX_CATCH_TO((h_)->err) return NSX_OK;

#define HIP_CHECK(expr)                                                                                   \
  do {                                                                                                    \
    hipError_t e_ = (expr);                                                                               \
    if (e_ != hipSuccess) NSX_THROW(NSX_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

template <class T>
struct DevBuf {
  T *p = nullptr;
  size_t n = 0;
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  ~DevBuf() { release(); }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
  void alloc(size_t count) {
    if (count == n && p) return;
    release();
    n = count;
    HIP_CHECK(hipMalloc((void **)&p, (count ? count : 1) * sizeof(T)));
  }
  void zero(hipStream_t s) {
    if (n) HIP_CHECK(hipMemsetAsync(p, 0, n * sizeof(T), s));
  }
  void upload(const T *src, size_t count, hipStream_t s) {
    alloc(count);
    if (count) HIP_CHECK(hipMemcpyAsync(p, src, count * sizeof(T), hipMemcpyHostToDevice, s));
    HIP_CHECK(hipStreamSynchronize(s));
  }
  void upload(const std::vector<T> &v, hipStream_t s) { upload(v.data(), v.size(), s); }
  void download(T *dst, size_t count, hipStream_t s) const {
    if (count) HIP_CHECK(hipMemcpyAsync(dst, p, count * sizeof(T), hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
  }
};

// CSR graph resident on the device (+ host copy kept for exports / setup products)
struct DevCsr {
  Csr host;
  DevBuf<int32_t> rowptr, colind, diag;  // diag: position of (i,i) (square graphs only)
  int32_t n_rows() const { return host.n_rows; }
  int64_t nnz() const { return host.nnz(); }
};

// Deterministic gather map: out entry e sums src[ptr[e] .. ptr[e+1]) (buffer offsets, ascending cell order).
struct GatherMap {
  DevBuf<int32_t> ptr, src;
  int64_t n_out = 0, n_src = 0;
};

// Block-Jacobi ILU(0) schedule on a square graph: per block the rows sorted by dependency level.
struct IluSchedule {
  int n_blocks = 0, max_rows = 0;
  std::vector<int32_t> block_ptr_h;
  DevBuf<int32_t> block_ptr;             // [n_blocks+1] row ranges
  DevBuf<int32_t> fwd_lvl_ptr, fwd_rows; // per block: levels of the L solve / factorisation (global arrays with offsets)
  DevBuf<int32_t> bwd_lvl_ptr, bwd_rows; // per block: levels of the U solve
  DevBuf<int32_t> blk_lvl_off;           // [n_blocks+1] offsets into fwd_lvl_ptr (levels per block), same for bwd
  DevBuf<int32_t> blk_lvl_off_b;
  int max_levels = 0;
  // packed solve stream (host/ilu_stream.hpp, k_ilu_solve_lanes): one wave per group of blocks, a lane owns a row for as many ticks
  // as the row has in-block entries; slab t = tick t of the wave
  DevBuf<int32_t> in_cptr;      // [n_rows+1] running count of in-block entries (compact numbering of a block's factor)
  DevBuf<int32_t> in_cpos;      // [in-block entries] compact number -> CSR position
  DevBuf<int32_t> fac_order;    // [n_blocks] blocks by descending in-block entries (dispatch order of k_ilu_factor_lds)
  int32_t max_block_nnz = 0;    // in-block entries of the largest block
  int64_t in_block_nnz = 0;     // in-block entries of the factor, diagonal included: what one application has to read (algorithmic bytes)
  int stream_ncomp = 0;         // the stream holds LDS byte addresses: it is built for one number of interleaved right-hand sides
  int stream_epl = 1;           // entries of its row a lane takes per tick (NSX_ILU_EPT)
  int64_t n_slabs = 0;
  int blocks_per_wave = 1, n_waves = 0, max_wave_rows = 0;
  bool packed_ok = false;       // false: a wave's rows do not fit 16-bit LDS addresses (few large blocks): workgroup-per-block kernel instead
  DevBuf<int32_t> pk_row_ptr, pk_rows;  // the rows of every wave in LDS order ([n_waves+1] offsets, global row ids)
  DevBuf<int32_t> pk_dinv_slot;         // position of row i's inverse pivot in pk_dinv (wave order)
  DevBuf<int32_t> pk_slab_ptr;  // [2*n_waves+1]: forward slabs, then backward slabs, per wave
  DevBuf<int32_t> pk_meta;      // [(n_slabs + pad) * 64 * meta words]
  DevBuf<int32_t> pk_slot_of;   // [nnz]: position of every in-block off-diagonal CSR entry in pk_val, -1 otherwise
  DevBuf<double> pk_val;        // [(n_slabs + pad) * 64 * stream_epl]: -L and -U/d in stream order (unused slots stay 0)
  DevBuf<double> pk_dinv;       // [n_rows] inverse pivots in wave order
  DevBuf<float> pk_val32;       // the same slots as pk_val, stored as float: written INSTEAD of pk_val by a factorisation in NSX_INNER_FP32
  bool stream_f32 = false;      // which of the two the last factorisation wrote (the other one is stale)
  // explicit inverses (k_ilu_invert / k_ilu_apply_dense): P_b = (L D U)^-1 of every block as a dense row-major n_b x n_b
  // matrix; the triangular solves become one dependency-free dense product per block
  bool dense = false;
  DevBuf<int64_t> dn_off;       // [n_blocks+1] offsets of the blocks' matrices in dn_P
  DevBuf<double> dn_P;
  int64_t dn_entries = 0;
  // levelled path for blocks too large for one wave / one workgroup (few real MPI ranks: R = 1 is the serial reference,
  // R = 8 one rank per GPU): the dependency levels of ALL blocks merged (blocks are independent, so level l of the
  // schedule is the union of the blocks' level-l rows), one launch per level over all its rows.  in_lo/in_hi: CSR
  // positions bounding the in-block entries of every row (columns are sorted, so they are one contiguous range).
  bool levelled = false;
  std::vector<int32_t> gl_f_ptr_h, gl_b_ptr_h;  // [levels+1] offsets into gl_f_rows / gl_b_rows
  DevBuf<int32_t> gl_f_rows, gl_b_rows, in_lo, in_hi;
  DevBuf<int32_t> gl_f_rec, gl_b_rec;  // [4 * rows] per row in level order: row, first entry, end of entries, diagonal (k_ilu_solve_level)
  // ---- which kernels the last factorisation / the last solve on this schedule launched (nsx_ilu_path_info; include/nsx.h has the
  //      codes).  Written by ilu_factor / ilu_solve, cleared when the schedule is rebuilt.
  struct Path {
    int factor = 0, invert = 0, factor_lds_bytes = 0;
    bool invert_staged = false;  // k_ilu_invert_lds read the factor from its LDS copy (nsx_ilu_invert_staged)
    int solve = 0, solve_pf = 0, solve_ncomp = 0, solve_f32 = 0;
  };
  mutable Path path;
};

// The ONE test for "this schedule's triangular solves with ncomp right-hand sides run the lane-owner stream": the solve reads the stream
// under it, and a factorisation in NSX_INNER_FP32 writes the float stream under it (with the stream's own ncomp), nowhere else
inline bool ilu_lanes_stream(const IluSchedule &s, int ncomp) { return s.packed_ok && !s.levelled && !s.dense && s.stream_ncomp == ncomp; }

// Ghost exchange plan of one scalar space (the Epetra_Import of every vmult): neighbours in ascending rank order,
// what to pack for each, and where each neighbour's values land in the ghost part of a vector.
struct HaloPlan {
  std::vector<int> nbr;
  std::vector<int32_t> send_ptr, recv_ptr;  // [n_nbr+1], node units
  std::vector<int32_t> send_idx_in;         // owned nodes to pack, caller-local ids (the internal layout maps them)
  DevBuf<int32_t> send_idx;                 // local (owned) node ids to pack, internal numbering
  DevBuf<double> sendbuf;
  std::vector<double> h_send, h_recv;       // host staging for the callback backend
  int n_own = 0;                            // ghosts start at node n_own
  hipEvent_t ev_done = nullptr;             // recorded on the communication stream when the ghosts of the last exchange are in place
  bool in_flight = false;                   // callback backend: packed and copied out, the host exchange itself still to do
  bool self_test = false;                   // nsx_comm_self_halo_test: a 1-rank communicator whose only neighbour is the rank itself
};

// Rows of a distributed operator that can be computed before the halo of its input arrives (all their columns are owned)
// and those that cannot (at least one ghost column): the interior rows run while the exchange is in flight.
struct RowSplit {
  DevBuf<int32_t> interior, interface;
  int n_interior = 0, n_interface = 0;
};

// LDS-staged ("blocked") SpMV schedule on a CSR graph: rows are cut into chunks of consecutive rows; per chunk the
// sorted unique column list and, per entry, the 16-bit position of its column in that list.  A workgroup stages the
// chunk's x entries in LDS once (each x entry is gathered once per chunk instead of once per non-zero).
struct SpmvBlocked {
  int n_chunks = 0, max_ucols = 0, max_rows = 0;
  DevBuf<int32_t> crow;  // [n_chunks+1] row range of every chunk (unions of consecutive rank blocks, or a fixed row count)
  DevBuf<int32_t> cptr, ucols;
  DevBuf<uint16_t> lidx;
  double ucols_total = 0;
  // launch order: desc[4 * block] = {first staged column, staged columns, first row, end row} of the chunk workgroup `block` takes
  // (grid = 8 * blocks per XCD; {0, 0, 0, 0} pads).  Workgroup b runs on XCD b % 8: every XCD gets a CONTIGUOUS range of chunks (their
  // x entries meet in one L2) holding an eighth of the non-zeros, and takes them largest first, so the last workgroups to start are the short ones
  DevBuf<int32_t> desc;
  int grid = 0;
  std::vector<int32_t> order;  // host copy: chunk of every block, -1 = padding
  // distributed handles: `desc` holds the chunks whose staged columns are all owned (launched while the ghost exchange is in flight),
  // `desc_if` those that stage a ghost column (launched behind it); frac_if = their share of the non-zeros
  DevBuf<int32_t> desc_if;
  int grid_if = 0, n_chunks_if = 0;
  double frac_if = 0;
};

// The planned Schur product (host/schur_plan.hpp, k_schur_planned): per group of 64 entries of a row of S a slab [step][lane] of packed
// term positions.  Built with the ILU schedules (ensure_schedules), stale whenever the Schur graph is rebuilt (build_schur_graph).
struct SchurPlanDev {
  bool current = false, ok = false;  // current: built for the handle's Schur graph; ok: the graph could be planned
  bool used_last = false;            // the last schur_numeric ran the planned kernel (nsx_schur_plan_info)
  int max_row = 0;                   // longest row of block(1,0): the LDS both Schur kernels ask for
  int64_t entries = 0, matches = 0, slots = 0, bytes = 0;
  double build_s = 0;                // host time of the plan
  DevBuf<int32_t> row_grp;
  DevBuf<int64_t> grp_off;
  DevBuf<uint32_t> words;
};

// Mailboxes of a persistent grid: two regions used alternately by successive launches (a launch empties the other region for its
// successor), then tail words that start as 0 (commit / error words).  The host half of nsx_grid.hpp works on it.
struct GridBox {
  DevBuf<unsigned long long> buf;
  size_t region = 0, n_tail = 0;
  int parity = 0;  // region of the next launch
  bool allocated() const { return buf.p != nullptr; }
  void alloc(size_t region_words, size_t tail_words) { buf.alloc(2 * (region = region_words) + (n_tail = tail_words)); }
  void clear(hipStream_t s) {  // both regions empty (GX_EMPTY is all ones), the tail zero: a new handle's state
    HIP_CHECK(hipMemsetAsync(buf.p, 0xff, 2 * region * sizeof(unsigned long long), s));
    HIP_CHECK(hipMemsetAsync(tail(), 0, n_tail * sizeof(unsigned long long), s));
  }
  unsigned long long *cur() const { return buf.p + (size_t)parity * region; }
  unsigned long long *other() const { return buf.p + (size_t)(1 - parity) * region; }
  unsigned long long *tail() const { return buf.p + 2 * region; }
  void flip() { parity ^= 1; }
  int dirty_words(nsx_handle *h) const;  // diagnostics (nsx_grid.hpp): the stream synchronised, words of cur() that are not empty
};

// Persistent Schur-complement CG (nsx_cg.hip): negative_S_tilde as slabs of 256 slots per Schur ILU block, 16-bit columns
// into the block's unique-column list.
struct CgPlan {
  bool ok = false, values_current = false;
  int64_t n_slots = 0;
  DevBuf<int32_t> u_ptr, u_cols, s_ptr, s_info, s_src;
  DevBuf<uint16_t> s_lidx;
  DevBuf<double> s_val;
  DevBuf<uint16_t> a_lidx;   // local column of every entry in CSR order (the LDS-resident operator of k_cg_schur<.., true>)
  int32_t max_block_nnz = 0;
};

// State of the Schur-complement CG (nsx_cg.hip: k_cg_schur in one persistent launch, k_cgd_* in two launches per iteration), grouped by lifetime.
struct CgState {
  // ---- per handle: allocated / read from the environment once (cg_setup), given up after a time-out (cg_schur_persistent)
  GridBox box;                         // mailbox regions, then the error word
  int max_wg = 0;                      // resident-grid limit of k_cg_schur<0, false>; 0: the persistent launch is not used
  int max_wg_res[2] = {0, 0};          // ... of the variants that keep the block inverses in registers (96 / 128 rows)
  int max_wg_lres[2] = {0, 0};         // ... and of the variants that keep the operator's rows in LDS as well
  bool disabled = false;
  DevBuf<double> vec;                  // work vectors of the persistent launch: d (double-buffered), h
  DevBuf<double> d_vec, d_parts;       // two launches per iteration (cg_schur_fused): g, h, S d, d (double-buffered, with ghosts); partial sums
  DevBuf<double> d_raw;                // ... per-block partial sums of a rank with more Schur blocks than entries of a partial-sum array (k_cgd_fold)
  // ---- per schedule set: rebuilt with the ILU schedules (ensure_schedules), and what the ranks agreed for them
  CgPlan plan;
  int d_agreed = -1;                   // two-launch Schur CG: -1 not decided for the current schedules and communicator, 0 / 1 the ranks' common answer
  // ---- last solve: diagnostics for nsx_path_info
  int last_path = 0;                   // 0 none yet, 1 one launch per operation, 2 one persistent launch, 3 two launches per iteration
  int last_rpg = 0, last_lres = 0;     // its persistent kernel's rows per lane group (0, 6, 8) and whether the operator sat in LDS ([28], [29]); 0 when it did not run
  bool resident = false, lds_resident = false, variant_said = false;  // the variant NSX_DEBUG reported last (block inverses in registers, operator in LDS), and whether it has
};

struct ProfEntry {
  int64_t launches = 0;
  double bytes = 0;  // algorithmic bytes summed over the launches (a scope's size may vary: Gram-Schmidt sweeps)
  double ms = 0;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
};

// State of the modified Gram-Schmidt sweep (nsx_mgs.hip), grouped by lifetime.
struct MgsState {
  // ---- per handle: allocated / read from the environment once (mgs_setup, mgs_lowsync), given up by mgs_recover after a time-out
  GridBox box;                         // persistent sweep: mailbox regions, then one commit word per workgroup
  int max_wg = 0;                      // 0: the launch-per-link chain is used
  int used_words[2] = {0, 0};          // mailbox words the last launch on each region filled (the sweep's own clearing protocol)
  int max_wg_e[3] = {0, 0, 0};         // resident-grid limits of k_mgs_one's instantiations, MGS_ENTRIES[k] entries per thread
  int max_wg_dist[3] = {0, 0, 0};      // resident-grid limits of the distributed instantiations (8 / 10 / 12 entries per thread), room left for the collective
  int dist_cap_reserved[3] = {0, 0, 0};  // grid limits of the distributed sweep's instantiations on the masked compute stream
  bool disabled = false;
  double guard_override = -1.0;        // >= 0: threshold of the Gram formula for |w'|^2 for the duration of nsx_gram_schmidt_cycle
  // distributed sweep with two collectives (mgs_lowsync): partial sums / all-reduced values / one 32 x 32 Gram matrix per GMRES nesting level
  DevBuf<double> ls_partial, ls_vals, ls_gram;
  int ls_mode = -1;                    // NSX_MGS_LOWSYNC, read once: 0 chain, 1 two collectives, 2 one
  // the persistent sweep of a distributed run (k_mgs_one<.., true>): two value buffers used alternately, arrival counter, release flag
  DevBuf<double> ext_vals;
  DevBuf<unsigned long long> ext_words;  // [0] release flag, [1] arrival counter (32 bits used), [2] the sweep the grid gave up on
  unsigned int ext_expected = 0;
  int ext_parity = 0;
  // ---- per communicator: what the ranks chose together (krylov_new_communicator / krylov_communicator_gone; dist_fit also krylov_new_schedules)
  int dist_state = -1;                 // -1 not decided yet, 0 two-pass sweep (mgs_lowsync), 1 the collective inside the persistent grid
  std::map<int, int> dist_fit;         // role of the vector in the solve (mgs_role) -> do ALL ranks' resident grids hold their vector of that role (agreed once per role; asked again when the sizes change)
  bool leave_req = false;              // a flag wait of this rank's grid timed out on its own: the next sweep asks all ranks to leave the persistent path
  int local_timeouts = 0;
  // ---- per schedule: the fused kernel's resident-grid limits hold for one LDS request (the velocity ILU schedule's largest wave)
  int ilu_cap[3] = {-1, -1, -1}, ilu_cap_rows = -1;
  // ---- last launch: diagnostics for nsx_path_info
  int last_e = 0, last_nwg = 0, last_dist = 0, max_e_seen = 0;  // the last persistent sweep: entries per thread, grid, collective inside
  int last_fused = 0, fused_launches = 0;  // the last persistent sweep had the velocity triangular solves inside (k_ilu_mgs)
};

// ---- State of the post-processing features, one block per feature.  Each block says what a new mesh drops (mesh_changed, called by
//      post_mesh_changed below); whatever it does not reset there survives a new internal layout / rank table as well, because the cells
//      and the caller's node numbering do not move with them.  What is kept in the INTERNAL node numbering follows nsx_handle::layout_epoch.

// Force evaluation (nsx_forces.hip): obstacle faces + face-quadrature tables.  Replaced as a whole by nsx_set_force_faces.
struct ForceState {
  int n = 0, nq = 0;
  DevBuf<int32_t> cells, lf;
  DevBuf<double> N2, dN2, N1, w, out;
};

// Flow diagnostics (nsx_diag.hip).  diag_mesh_setup refills counted / n_counted and drops the results with EVERY mesh installation
// (a new mesh, a new layout, new rank tables of a handle with a layout).
struct DiagState {
  DevBuf<uint8_t> counted;  // [n_cells] 1 = this handle counts the cell (distributed: the owner of its lowest global P2 node does)
  int n_counted = 0;
  DevBuf<double> planes;    // [NSX_DIAG_COUNT][n_cells] per-cell values of the last nsx_compute_diagnostics (allocated by the first one)
  DevBuf<double> fold;      // the levels of their fold
  DevBuf<double> max;       // [2 * world] the ranks' maxima on their way through the SUM collective
  bool valid = false;       // planes holds the values of a finished call on the current mesh
};

// Point probes (nsx_probe.hip).  The set outlives a new layout / rank table, not a new mesh.
struct ProbeState {
  DevBuf<double> cell_x0;   // SoA [dim][n_cells]: vertex 0 of every cell, beside geo (x = X0 + J lambda); probe_mesh_setup, with every mesh installation
  int n = 0;                // probes of the current set (0: none)
  DevBuf<int32_t> cell;     // [n] the cell this handle evaluates the probe in (caller's cell order), -1: in no cell / another rank's
  DevBuf<double> lambda;    // SoA [dim+1][n] barycentric coordinates in that cell, stored by nsx_set_probes
  DevBuf<double> out;       // SoA [dim + 1 + dim^2][n] values of the last nsx_eval_probes
  std::vector<int32_t> cells_h, owner_h;  // what nsx_get_probe_cells hands out
  std::vector<double> lambda_h;           // [n][dim+1]
  void mesh_changed() {     // a new mesh drops the probe set
    n = 0;
    cells_h.clear();
    owner_h.clear();
    lambda_h.clear();
  }
};

// Tracer particles (nsx_tracer.hip).  The set outlives a new layout / rank table, not a new mesh.
struct TracerState {
  DevBuf<int32_t> cell_nbr;  // SoA [dim+1][n_cells]: cell across the face opposite local vertex k, -1: boundary; built by the first nsx_set_tracers on a mesh
  bool have_nbr = false;
  int n = 0;                 // particles of the current set (0: none)
  double tol = 0.0;          // containment tolerance of the set (nsx_set_tracers), used by every walk
  DevBuf<double> x;          // SoA [dim][n] positions
  DevBuf<double> age;        // [n]
  DevBuf<int32_t> cell, status, face;  // [n] each
  void mesh_changed() {      // a new mesh drops the tracer set and the face-neighbour table
    n = 0;
    have_nbr = false;
  }
};

// Nodal fields (nsx_nodal.hip).  The patch table is in the caller's node and cell numbering: it outlives a new layout / rank table, not a new mesh.
struct NodalState {
  bool have_patches = false;        // the node -> (cell, local node) patch table of the current mesh is on the device; built by the first nsx_compute_nodal_fields on a mesh
  DevBuf<int32_t> tile_ptr, ent;    // host/nodal_patch.hpp: [tiles + 1] first step of every tile of 64 slots, [steps][64] cell << 4 | local node (-1: padding)
  std::vector<int32_t> slot_of;     // [N2] caller-local owned node -> slot
  int tiles = 0;
  int64_t entries = 0;              // entries of ent, padding included
  DevBuf<double> out;               // SoA [dim^2 + (3 | 1) + 3][64 tiles] in slot order: Gbar, vorticity, Q, strain rate, divergence of the last nsx_compute_nodal_fields
  bool valid = false;               // out holds the values of a finished call on the current mesh
  void mesh_changed() {             // a new mesh drops the patch table and the results
    have_patches = false;
    valid = false;
    slot_of.clear();
  }
};

// Isosurfaces and slices (nsx_iso.hip).  Coordinates and orientation are per cell and survive a new layout / rank table; the node maps are
// in the INTERNAL numbering and are rebuilt when nsx_handle::layout_epoch has moved past the epoch they were built in.
struct IsoState {
  bool have_coords = false;         // cellx / flip hold the current mesh; uploaded by the first nsx_extract_isosurface on a mesh
  DevBuf<double> cellx;             // SoA [(dim+1) dim][n_cells]: the vertex coordinates of every cell
  DevBuf<uint8_t> flip;             // [n_cells] 1 = det J < 0: the primitives of the cell swap their last two vertices
  int map_epoch = -1, slot_epoch = -1;  // the layout_epoch the node maps below were built in
  DevBuf<int32_t> pmap;             // [2][N2_loc] internal P2 node -> its P1 node (second entry -1), or the two P1 nodes of its line
  DevBuf<double> nodex;             // SoA [dim][N2_loc] position of every internal P2 node
  DevBuf<int32_t> slot;             // [N2_loc] internal P2 node -> slot of nodal.out (-1: a ghost)
  DevBuf<double> s;                 // [2][N2_loc] nodal scalars of the last call: field plane, colour plane
  DevBuf<int32_t> pack;             // [n_cells] prefix inside the workgroup << 5 | primitives of the cell
  DevBuf<int32_t> wg_tot;           // [workgroups] primitives per workgroup of k_iso_count
  DevBuf<long long> wg_off;         // [workgroups + 1] their exclusive prefix sum; the last entry is the total
  DevBuf<double> pts, col;          // SoA [dim dim][cap], [dim][cap]: the primitives of the last extract
  DevBuf<int32_t> cells;            // [cap]
  int64_t cap = 0, n = 0;           // capacity (never shrinks), primitives of the last extract
  bool valid = false, has_colour = false;  // the buffers hold a finished extract on the current mesh; it had a colour source
  void mesh_changed() {             // a new mesh drops the coordinates, the node maps and the result
    have_coords = false;
    valid = false;
    n = 0;
    map_epoch = slot_epoch = -1;
  }
};

// Lattice sampling (nsx_lattice.hip).  The owner table is in the caller's cell order: lattice and results outlive a new layout / rank table,
// not a new mesh.  Nothing is stored per point but the owning cell.
struct LatticeState {
  bool set = false;                 // a lattice is installed
  double origin[3] = {0, 0, 0}, spacing[3] = {1, 1, 1}, tol = 0.0;  // tol: the containment tolerance the owners were found with
  int32_t counts[3] = {1, 1, 1};
  int64_t n_total = 0, n_found = 0; // points of the lattice, points that lie in a cell
  DevBuf<int32_t> owner;            // [n_total] position of the owning cell in the caller's cell list, -1: in no cell
  DevBuf<double> vel, pres, grad, nodal;  // SoA planes [dim | 1 | dim^2 | nodal_planes(dim)][n_total] of the last nsx_eval_lattice; allocated by the
                                          // first one that asks for them and kept by a new lattice (what = 0) for the next evaluation to reuse
  int what = 0;                     // the NSX_LATTICE_* bits the last nsx_eval_lattice computed (0: no results)
  void clear() {                    // gives the lattice, its results and their memory up
    set = false;
    what = 0;
    n_total = n_found = 0;
    owner.release();
    vel.release();
    pres.release();
    grad.release();
    nodal.release();
  }
  void mesh_changed() { clear(); }  // a new mesh drops the lattice and its results
};

// Running statistics (nsx_stats.hip).  The accumulator planes are in the CALLER's node numbering: an accumulation outlives a new layout / rank
// table, not a new mesh.
struct StatsState {
  int what = 0, n_bins = 0;         // NSX_STATS_* bits and phase bins of the open accumulation (0, 0: none)
  size_t stride2 = 0, stride1 = 0;  // entries per plane: the owned P2 / P1 nodes rounded up to a multiple of 64 (the kernels take two nodes per lane)
  DevBuf<double> vel;               // SoA [n_bins][dim + dim (dim + 1) / 2][stride2]: mean, then co-moment xx, yy, [zz,] xy[, xz, yz]
  DevBuf<double> pres;              // SoA [n_bins][2][stride1]: mean, co-moment
  DevBuf<double> out;               // [n_nodes][n_components] of the last nsx_stats_get on its way to the host
  std::vector<double> W;            // [n_bins] weight sums
  std::vector<int64_t> samples;     // [n_bins]
  void clear() {                    // gives the accumulation and its memory up
    what = n_bins = 0;
    stride2 = stride1 = 0;
    vel.release();
    pres.release();
    out.release();
    W.clear();
    samples.clear();
  }
  void mesh_changed() { clear(); }  // a new mesh drops the accumulation
};

// Surface loads (nsx_surface.hip).  Faces and surface nodes are in the caller's cell and node numbering: the set and its results outlive a
// new layout / rank table, not a new mesh.  "sorted": the faces stable-sorted by group (host/surface_patch.hpp).
struct SurfaceState {
  bool set = false, valid = false;  // a set is installed; the planes hold the values of a finished nsx_compute_surface on it
  int n_faces = 0, n_groups = 0, n_nodes = 0, npf = 0, form = 0, tiles = 0;
  int64_t entries = 0;              // entries of ent, padding included
  double centre[3] = {0, 0, 0};
  std::vector<int32_t> order, face_nodes, node_group, slot_of;  // sorted position -> caller's face, [n_faces][npf] surface node, [n_nodes] each
  std::vector<int32_t> nodes;       // [n_nodes] P2 node in the caller's (global) numbering
  std::vector<uint8_t> owned;       // [n_nodes] 1 = this handle owns the P2 node
  std::vector<double> areas;        // [n_faces] caller's order
  std::vector<std::vector<int32_t>> fold_blocks;  // per level of the fold {first, last + 1, group} of every block
  DevBuf<int32_t> cells, lf;        // [n_faces] sorted: cell (caller's cell list), local vertex the face lies opposite of
  DevBuf<double> fgeo;              // SoA [dim + 2][n_faces] sorted: outward unit normal, height of the cell over the face, measure
  DevBuf<double> fx;                // SoA [dim][npf][n_faces] sorted: position of every face node
  DevBuf<int32_t> tile_ptr, ent, fold_tab;  // patch lists in tiles of 64 surface nodes; the block tables of the fold, level after level
  DevBuf<double> fvals;             // SoA [surface_face_planes(dim)][npf][n_faces] sorted: the values at the face nodes
  DevBuf<double> nvals;             // SoA [surface_node_planes(dim)][64 tiles] in slot order: the values at the surface nodes
  DevBuf<double> contrib, fold;     // SoA [surface_total_planes(dim)][n_faces] per-face contributions to the totals; the levels of their fold
  void clear() {
    set = valid = false;
    n_faces = n_groups = n_nodes = npf = form = tiles = 0;
    entries = 0;
    centre[0] = centre[1] = centre[2] = 0.0;
    for (auto *v : {&order, &face_nodes, &node_group, &slot_of, &nodes}) v->clear();
    owned.clear();
    areas.clear();
    fold_blocks.clear();
    for (auto *b : {&cells, &lf, &tile_ptr, &ent, &fold_tab}) b->release();
    for (auto *b : {&fgeo, &fx, &fvals, &nvals, &contrib, &fold}) b->release();
  }
  void mesh_changed() { clear(); }  // a new mesh drops the set and its results
};

struct Comm;  // RCCL state (nsx_comm.hip)

// ---- THE table of device scalar slots (h->scal, mirrored in h->scal_host and the first N_SLOTS doubles of h->pub_host), of the mapped
//      words behind them and of the basis sizes that give the ranges their lengths.  A slot that is not listed here is free.
enum { N_SLOTS = 128 };                     // device scalar slots (reduction results)
constexpr int KRYLOV_N_TMP = 30;            // SolverGMRES::AdditionalData::max_n_tmp_vectors: a cycle sweeps against dim <= KRYLOV_N_TMP - 2 vectors
constexpr int SWEEP_SLOTS = KRYLOV_N_TMP + 1;  // a sweep writes slot0 .. slot0 + dim + 2: h(i), |w|^2 after, |w|^2 before, "the norm was summed explicitly"
enum Slot {
  S_POST = 0,              // [S_POST_LEN] BETWEEN solves: the collectives of the post-processing (nsx_diag.hip, nsx_forces.hip) borrow the solvers' per-solve
                           // scratch below S_H (written before it is read in every solve: nothing is carried from one call to the next)
  S_DH = 2,                // SolverCG: d.h
  S_GH = 3, S_GH2 = 5,     // ... g.h of the current / the next iteration (ping-pong)
  S_RES = 4,               // ... |g|^2: between the two g.h slots, so whichever is current, the pair that travels in one all-reduce is adjacent
  S_LS_NORM = 7,           // the explicitly summed |w|^2 of the distributed sweep (nsx_mgs.hip)
  S_H = 8,                 // [SWEEP_SLOTS] SolverGMRES: the sweep's coefficients
  S_T = 39,                // |b|^2 of a relative tolerance / the scratch of norm2: next to S_NRM, the two travel to the host in one publication (Seams::rtol)
  S_NRM = 40,              // SolverGMRES: |v|^2 of a cycle's first vector
  S_H2 = 41,               // [SWEEP_SLOTS] ... the coefficients of a re-orthogonalisation sweep
  S_CGP = 100,             // [S_CGP_LEN] the Schur CG's publication: steps, last residual, status, tolerance (nsx_cg.hip)
  S_AGREE = N_SLOTS - 1,   // comm_agree_all: the sum of the ranks' objections
};
constexpr int S_CGP_LEN = 4, S_POST_LEN = 8;
static_assert(S_POST + S_POST_LEN <= S_H, "the post-processing borrows scratch slots only");
// (the test hook nsx_gram_schmidt_sweeps sweeps against up to KRYLOV_N_TMP - 1 vectors from S_H: its longest sweep ends ON S_T, which
// holds nothing while the hook runs)
constexpr int SLOT_RANGES[][2] = {{S_DH, 1}, {S_GH, 1}, {S_RES, 1}, {S_GH2, 1}, {S_LS_NORM, 1}, {S_H, SWEEP_SLOTS}, {S_T, 1}, {S_NRM, 1}, {S_H2, SWEEP_SLOTS},
                                  {S_CGP, S_CGP_LEN}, {S_AGREE, 1}};
constexpr bool slot_ranges_ok() {  // listed in ascending order, each ending where the next begins at the latest: pairwise disjoint and below N_SLOTS
  int end = 0;
  for (const auto &r : SLOT_RANGES) {
    if (r[0] < end || r[1] < 1) return false;
    end = r[0] + r[1];
  }
  return end <= N_SLOTS;
}
static_assert(slot_ranges_ok(), "scalar slot ranges overlap or leave the table");
static_assert(S_NRM == S_T + 1, "|b|^2 and the first residual norm are one publication");
static_assert(S_GH < S_RES && S_RES < S_GH2 && S_GH2 - S_GH == 2, "S_RES sits between the two g.h slots");
// Mapped host words behind the slots (h->pub_host / h->pub_dev + N_SLOTS, 8 bytes each): written by kernels, read by the host without a copy
enum PubWord {
  PUB_FLAG = 0,        // sequence number of the last publication (wait_published)
  PUB_MGS_ERR = 2,     // raised by a Gram-Schmidt grid that gives up
  PUB_ILU_ERR = 3,     // raised by an ILU(0) kernel / the float conversion of F (ilu_check)
  PUB_SCHUR_SAME = 4,  // raised when the Schur product's weights differ from the last initialisation's
  PUB_WORDS = 8
};

}  // namespace nsx

struct nsx_handle {
  nsx_params prm{};
  std::string err;
  hipStream_t stream = nullptr;
  // ---- discretisation
  int dim = 0, n_q = 0, np2 = 0, np1 = 0, dpc = 0;
  int n_cells = 0, N2 = 0, NP = 0, n_u = 0, n_p = 0;  // local sizes (rows owned by this handle)
  int N2_loc = 0, NP_loc = 0;                          // owned + ghost (== N2, NP on one GPU)
  // vector layout [u_owned (n_u) | u_ghost (g_u) | p_owned (n_p) | p_ghost (g_p)]; off_p = n_u + g_u
  int n_cells1 = 0;                                    // layer-1 cells (touch an owned node): the per-step cell loop
  int g_u = 0, g_p = 0, off_p = 0, len_blk = 0, len_u = 0, len_p = 0;
  bool dist = false;
  int rank = 0, world = 1, goff_u = 0, goff_p = 0, n_u_glob = 0, n_p_glob = 0;  // global numbering of this rank's range
  std::vector<int32_t> ghost_u, ghost_p;               // global ids of the ghost nodes (sorted)
  nsx::HaloPlan haloU, haloP;
  nsx::RowSplit splitA, splitVel, splitB, splitG, splitS;  // F alone, F + block(0,1) (the saddle product), block(1,0), block(0,1), S
  hipStream_t comm_stream = nullptr;                       // halo pack / send / receive run here, beside the compute stream
  hipEvent_t ev_ready = nullptr;                           // "the input vector is complete" (compute stream -> communication stream)
  bool have_tables = false, have_mesh = false, assembled = false, prec_ready = false;
  std::vector<double> N2_h, dN2_h, N1_h, w_h;
  nsx::DevBuf<double> tab_N2, tab_dN2, tab_N1, tab_w, tab_N2T, tab_dN2T;  // T: [a][q] / [b][q][k]
  nsx::DevBuf<int32_t> cell_n2, cell_n1;  // SoA [a][cell]
  nsx::DevBuf<double> geo;                // SoA [(dim*dim+1)][cell]
  std::vector<int32_t> cell_n2_h, cell_n1_h;  // scalar connectivity in the INTERNAL numbering (what every product below is built from)
  // ---- internal layout (nsx_set_internal_layout): the caller keeps its own numbering and rank count, libnsx renumbers the owned
  //      nodes behind the boundary (virtual ranks + colour order, host/layout.hpp); perm: caller-local owned node -> internal node
  std::vector<int32_t> cell_n2_in, cell_n1_in;   // connectivity as handed over (caller-local ids: owned < N2 <= ghosts)
  std::vector<double> cell_coords_in;            // [n_cells][dim+1][dim]: a new layout reruns the set-up products
  std::vector<int32_t> in_rank_u_h, in_rank_p_h, in_sblk_h;  // the caller's rank / Schur block tables (local node ids)
  int layout_req_ranks = 0, layout_req_order = 0, layout_req_schur = 0;  // the request (0 ranks: none; may precede nsx_set_mesh)
  bool layout_on = false;
  int layout_colours = 0, layout_colours_p = 0;
  std::vector<int32_t> perm2_h, perm1_h, iperm2_h, iperm1_h;
  nsx::DevBuf<int32_t> perm2_d, perm1_d;
  nsx::DevBuf<double> io_stage;                  // block vector in the caller's order on its way in / out
  nsx::Csr caller_graph[2];                      // scalar velocity / Schur graph in the caller's numbering (exports), built on demand
  std::vector<int32_t> caller_pos[2];            // ... and for each of its entries the position in the internal CSR
  // ---- graphs and values
  nsx::DevCsr gA, gG, gB, gS, gPM;
  nsx::SpmvBlocked blkA;
  // the switches of the velocity product, read once by nsx_create: NSX_SPMV_W lanes per row of the plain kernel (8 / 16 / 32), NSX_SPMV_BLOCKED=0
  // never the LDS-staged kernel, NSX_SPMV_ORDER=0 its chunks in row order instead of largest first
  int spmv_w = 16;
  bool spmv_blocked = true, spmv_largest_first = true;
  nsx::DevBuf<double> vS0, vMass, vStiff, vConv, vF, vG, vB, vPM, vSchur, luF, luS;
  // ---- inner precision (nsx_set_inner_precision): how F and the off-diagonal ILU(0) entries of F are STORED for the inner solves
  int inner_precision = NSX_INNER_FP64;
  nsx::DevBuf<float> vF32;                 // float copy of vF, current behind every nsx_prec_initialize in NSX_INNER_FP32
  int inner_F_fp32_used = 0, ilu_F_fp32_used = 0;  // the last solve's inner F products / velocity triangular solves streamed float values (nsx_path_info [26], [27])
  nsx::DevBuf<int32_t> bt_of_g;            // for every G entry (i,k): position of (k,i) in the B graph
  nsx::GatherMap gmA, gmG, gmB, gmPM;
  nsx::DevBuf<double> cellbuf;             // per-cell local matrices, SoA [(entry)][cell]
  // ---- vectors (n_u + n_p)
  nsx::DevBuf<double> sol, sol_owned, prev_sol, rhs;
  // ---- ranks / ILU
  std::vector<int32_t> rank_u_h, rank_p_h, sblk_h;
  nsx::DevBuf<int32_t> rank_u;             // node units
  nsx::IluSchedule schedF, schedS;
  nsx::SchurPlanDev schur_plan;
  int lds_optin = 0;                       // the device's opt-in limit of dynamic LDS per workgroup, queried once (nsx_create)
  nsx::DevBuf<double> dbar;                // per-rank Dirichlet diagonal
  nsx::DevBuf<int32_t> bc_dofs;
  nsx::DevBuf<double> bc_vals;
  nsx::DevBuf<double> dirmask;             // [n_u] 1 = free, 0 = constrained row of block (0,1)
  std::vector<int32_t> bc_cache;
  // ---- preconditioner vectors
  nsx::DevBuf<double> diag_D, diag_D_inv, neg_diag_D_inv, lump_M, schur_w;
  nsx::DevBuf<double> schur_w_prev;        // weights the current Schur product / its factors were computed from
  bool schur_valid = false, schur_pending = false;  // pending: rebuilt in this initialisation, not yet confirmed (prec_confirm)
  int schur_type = -1;
  // ---- Krylov workspace
  std::vector<nsx::DevBuf<double> *> pool;  // temporary vectors handed out by size
  nsx::DevBuf<double> red_partial;          // reduction partials
  nsx::DevBuf<double> scal;                 // device scalars
  int slot_nb[nsx::N_SLOTS] = {0};          // >0: the slot's value is still spread over that many partial sums
  double *scal_host = nullptr;              // pinned mirror
  // host-visible publication of scalars without a memcpy + stream sync: the publishing kernel writes the values and then
  // a sequence number into fine-grained mapped host memory, the host polls the sequence number
  double *pub_host = nullptr, *pub_dev = nullptr;  // [N_SLOTS] values, then the PUB_WORDS mapped words (pub_word_host / pub_word_dev)
  unsigned long long pub_seq = 0;
  nsx::DevBuf<unsigned int> pub_counter;
  nsx::MgsState mgs;        // the modified Gram-Schmidt sweep of the GMRES drivers (nsx_mgs.hip)
  bool sched_dirty = true;  // the ILU schedules do not match the current rank tables yet
  int gx_drop_wg = -1;                 // NSX_GX_DROP_WG (fault injection, tests): this workgroup of a persistent grid never posts its sums
  int n_persistent_fallbacks = 0;      // persistent kernels that timed out on this handle (nsx_solve_stats::persistent_fallbacks)
  int gmres_depth = 0;                 // GMRES nesting level of the running solve (one Gram matrix of mgs.ls_gram per level)
  bool cu_reserve_failed = false;    // the ranks tried to mask their streams and one of them could not: all are back on plain streams, nobody asks again
  nsx::DevBuf<double> ext_self;           // development (NSX_EXT_SELF_P2P): operands of the self-addressed send / receive in front of the sweep's collective
  hipStream_t stream_plain = nullptr;  // the compute stream of the handle's creation once `stream` has been replaced by one with a CU mask (comm_reserve_cus)
  std::vector<hipStream_t> retired_streams;  // streams RCCL has launched on and the handle no longer uses: destroyed behind ncclCommDestroy (comm_destroy)
  int cu_reserved = 0;               // CUs (one per XCD) the compute stream leaves to the communication stream's kernels
  int comm_probe_local = -1;         // -1 not probed, 0 / 1: kernels of the communication stream run beside a waiting kernel of the compute stream (comm_prepare_streams)
  long long n_allreduce = 0, n_halo = 0;  // collectives issued (nsx_comm_counters)
  int self_p2p = 0;                       // development (NSX_EXT_SELF_P2P, read by nsx_comm_init): self-addressed send / receive pairs in front of collectives
  int n_ext_collectives = 0;              // collectives inside a persistent grid so far (fault injection: NSX_EXT_LATE_RELEASE)
  nsx::CgState cg;          // the CG on the Schur complement (nsx_cg.hip)
  // ---- post-processing: one state block per feature (above)
  int layout_epoch = 0;     // counts the installations of a mesh / an internal layout: what is kept in the INTERNAL node numbering is rebuilt when it moves
  nsx::ForceState ff;       // nsx_forces.hip
  nsx::DiagState diag;      // nsx_diag.hip
  nsx::ProbeState probe;    // nsx_probe.hip
  nsx::TracerState tracer;  // nsx_tracer.hip
  nsx::NodalState nodal;    // nsx_nodal.hip
  nsx::IsoState iso;        // nsx_iso.hip
  nsx::LatticeState lattice;  // nsx_lattice.hip
  nsx::StatsState stats;    // nsx_stats.hip
  nsx::SurfaceState surface;  // nsx_surface.hip
  // ---- profiling
  bool prof_on = false;
  std::map<std::string, nsx::ProfEntry> prof;
  std::vector<std::string> prof_names;
  // ---- comm
  nsx::Comm *comm = nullptr;
  bool defer_red = false;             // distributed runs: all-reduces of finished reductions are held back ...
  std::vector<int> pending_red;       // ... for these slots, and merged when released (defer_reductions)
};

namespace nsx {

// RAII launch timer used by every kernel launch site.
struct LaunchScope {
  nsx_handle *h;
  ProfEntry *e = nullptr;
  hipEvent_t a = nullptr, b = nullptr;
  LaunchScope(nsx_handle *h_, const char *name, double bytes) : h(h_) {
    if (!h->prof_on) return;
    e = &h->prof[name];
    e->bytes += bytes;
    (void)hipEventCreate(&a);
    (void)hipEventCreate(&b);
    (void)hipEventRecord(a, h->stream);
  }
  ~LaunchScope() {
    if (!e) return;
    (void)hipEventRecord(b, h->stream);
    e->launches++;
    e->pending.emplace_back(a, b);
  }
};

inline int cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

// The mapped word W (PubWord) as the host reads it and as a kernel writes it
template <class T = int>
inline volatile T *pub_word_host(nsx_handle *h, int W) { return (volatile T *)(h->pub_host + N_SLOTS + W); }
template <class T = int>
inline T *pub_word_dev(nsx_handle *h, int W) { return (T *)(h->pub_dev + N_SLOTS + W); }

// ---- one reset per lifetime of what the Krylov drivers' state blocks (MgsState, CgState) keep beyond a solve.  Each resets what its call
//      sites always reset, no more: a wider reset makes a later solve ask the ranks again, i.e. changes the collectives it issues.
// comm_destroy (also in front of every new communicator).  dist_state / dist_fit / d_agreed are NOT touched here: a handle whose communicator
// went keeps them until the next one arrives (below).  What a timed-out sweep gave up (mgs_recover: mgs.disabled, the grid limits) stays given
// up for the handle, whatever communicator follows.
inline void krylov_communicator_gone(nsx_handle *h) {
  h->cu_reserve_failed = h->mgs.leave_req = false;
  h->mgs.local_timeouts = 0;
}
// nsx_comm_init, nsx_comm_init_callbacks (behind comm_destroy): the paths the ranks choose together are chosen again
inline void krylov_new_communicator(nsx_handle *h) {
  h->mgs.dist_state = h->cg.d_agreed = -1;
  h->mgs.dist_fit.clear();
}
// refresh_rank_products: sizes may have changed, what the ranks agreed on for the old ones is asked again (every rank gets here alike).
// The Schur CG's answer follows the schedules, which are rebuilt later (ensure_schedules, with the next initialisation): two functions.
inline void krylov_new_rank_tables(nsx_handle *h) { h->mgs.dist_fit.clear(); }
inline void krylov_new_schedules(nsx_handle *h) { h->cg.d_agreed = -1; }

struct SolveResult {
  int status, steps;  // status: 0 success, 1 failure
  double last;
};
inline int sc_check(int step, double value, double tol, int maxsteps) {  // SolverControl::check: 0 iterate, 1 success, 2 failure
  return value <= tol ? 1 : (step >= maxsteps || std::isnan(value)) ? 2 : 0;
}

// ---- environment knobs (NSX_*): THE readers.  A reader reads when it is called, so the call site decides how long a value holds: per
//      call (what the tests switch inside one process: the ILU, Schur CG and step variants, NSX_PF, NSX_SCHUR_CACHE), once per process (the
//      initialiser of a function's `static`) or once per handle (nsx_create, mgs_setup, the schedule builders).  DESIGN.md section 4 has the list.
inline int env_int(const char *name, int dflt) {
  const char *e = getenv(name);
  return e ? atoi(e) : dflt;
}
inline int64_t env_i64(const char *name, int64_t dflt) {
  const char *e = getenv(name);
  return e ? atoll(e) : dflt;
}
inline double env_double(const char *name, double dflt) {
  const char *e = getenv(name);
  return e ? atof(e) : dflt;
}
inline bool env_set(const char *name) { return getenv(name) != nullptr; }
inline bool env_on(const char *name) { return env_int(name, 1) != 0; }      // on unless set to 0
inline bool env_opt_in(const char *name) { return env_int(name, 0) == 1; }  // off unless set to 1
inline bool nsx_debug() { return env_set("NSX_DEBUG"); }
// knobs more than one file reads
inline bool ilu_mgs_wanted() { return env_opt_in("NSX_ILU_MGS"); }          // the velocity triangular solves inside the sweep's launch (k_ilu_mgs)
inline int ilu_lanes_pf() { return env_int("NSX_PF", 8) == 4 ? 4 : 8; }     // slabs a lane-owner solve keeps in flight: 4, anything else 8
inline int mgs_maxwg_cap(int limit) { return env_set("NSX_MGS_MAXWG") ? std::min(limit, env_int("NSX_MGS_MAXWG", 0)) : limit; }  // tests: small grids

// A run-time integer as a compile-time constant: f(std::integral_constant<int, V>) for the V among Vs... that equals v; false if none does.
//   with_int<2, 3>(h->dim, [&](auto D) { launch<decltype(D)::value>(...); });
template <int... Vs, class F>
inline bool with_int(int v, F &&f) {
  return ((v == Vs ? (f(std::integral_constant<int, Vs>{}), true) : false) || ...);
}

// ---- kernels / steps implemented across the .hip files
void setup_ilu_schedule(nsx_handle *h, const Csr &g, const std::vector<int32_t> &block_ptr, IluSchedule &s, int blocks_per_wave, bool allow_dense = false,
                        int ncomp = 1);
void build_schur_graph(nsx_handle *h);
// host vectors of the C-ABI are in the CALLER's numbering (global [n_u_glob | n_p_glob]); device block vectors in the internal one
void vec_from_caller(nsx_handle *h, double *dev, const double *host, bool with_ghosts);  // owned (+ ghost) entries of a block vector
void vec_to_caller(nsx_handle *h, const double *dev, double *host);                      // owned entries only
void part_from_caller(nsx_handle *h, int which, double *dev, const double *host);        // one space, single-process handles: 0 velocity [n_u], 1 pressure [n_p]
void part_to_caller(nsx_handle *h, int which, const double *dev, double *host);
void pressure_from_caller(nsx_handle *h, double *dev, const double *host);  // one pressure vector, distributed handles too (globally indexed host, owned entries)
void pressure_to_caller(nsx_handle *h, const double *dev, double *host);
void velocity_to_caller(nsx_handle *h, const double *dev, double *host);  // one velocity vector [len_u], distributed handles too: the velocity part of vec_to_caller
inline int32_t node_to_internal(const nsx_handle *h, int32_t local_node) { return h->layout_on ? h->perm2_h[local_node] : local_node; }
inline int32_t pnode_to_internal(const nsx_handle *h, int32_t local_node) { return h->layout_on ? h->perm1_h[local_node] : local_node; }
void ensure_schedules(nsx_handle *h);  // (re)build the ILU schedules if the rank / Schur block tables changed
void ensure_schur_plan(nsx_handle *h);  // (re)build the plan of the Schur product if the Schur graph changed

// assembly (nsx_assemble.hip)
void run_assemble(nsx_handle *h, bool first, int flags);
void run_dirichlet(nsx_handle *h, int n, const int32_t *dofs, const double *vals);

// post-processing (nsx_diag.hip, nsx_probe.hip; everything else of the family: nsx_post.hpp)
void diag_mesh_setup(nsx_handle *h);                              // with every mesh set-up: which cells this handle counts
void probe_mesh_setup(nsx_handle *h, const double *cell_coords);  // with every mesh set-up: vertex 0 of every cell
// a new mesh (nsx_set_mesh / nsx_set_mesh_distributed, not a new layout or rank table): every feature drops what its state block says
inline void post_mesh_changed(nsx_handle *h) {
  h->probe.mesh_changed();
  h->tracer.mesh_changed();
  h->nodal.mesh_changed();
  h->iso.mesh_changed();
  h->lattice.mesh_changed();
  h->stats.mesh_changed();
  h->surface.mesh_changed();
}

// sparse (nsx_sparse.hip)
bool blocked_usable(const nsx_handle *h);                                                   // F->vmult goes through the LDS-staged SpMV
void spmv_F(nsx_handle *h, const double *vals, const double *x, double *y, const float *vals32 = nullptr, const double *rb = nullptr);  // y_u = A x_u   (dim comps); rb: y_u = rb - A x_u
void spmv_F_inner(nsx_handle *h, const double *x, double *y);  // F->vmult inside a preconditioner's vmult: F in the handle's inner precision
void spmv_F_inner_resid(nsx_handle *h, const double *x, const double *b, double *y);  // y = b - F x: the product with the subtraction as each row's epilogue
void convert_F_f32(nsx_handle *h);                             // vF32 = (float)vF
void spmv_saddle(nsx_handle *h, const double *x, double *y);                                // full block vmult
void spmv_G(nsx_handle *h, const double *xp, double *yu, bool accumulate);                  // y_u (+)= block(0,1) x_p
void spmv_B(nsx_handle *h, const double *xu, double *yp, const double *r = nullptr, int sub = 0);  // y_p = block(1,0) x_u; r: y_p = (block(1,0) x_u) - r (sub = 1) or r - (block(1,0) x_u) (sub = -1)
void spmv_S(nsx_handle *h, const double *x, double *y);                                     // y = negative_S x
void schur_numeric(nsx_handle *h, const double *w);                                         // S = B diag(w) G
void extract_diag(nsx_handle *h, const DevCsr &g, const double *vals, double *d);           // scalar diag
void abs_rowsum(nsx_handle *h, const DevCsr &g, const double *vals, double *d);

// block-Jacobi ILU(0) (nsx_ilu.hip)
void ilu_factor(nsx_handle *h, const DevCsr &g, IluSchedule &s, const double *vals, double *lu, const char *name, bool f32 = false);
void ilu_check(nsx_handle *h);  // after a synchronisation: throws if a factorisation kernel reported a failure
// dot_slot >= 0: also leave b.x in that scalar slot when the packed kernel can do it; returns whether it did
bool ilu_solve(nsx_handle *h, const DevCsr &g, const IluSchedule &s, const double *lu, const double *b, double *x, int ncomp,
               const char *name, int dot_slot = -1, bool f32 = false, int *used_f32 = nullptr);

// Index span of a BLAS-1 operation: n owned entries; entries at i >= split sit `gap` further (the ghost velocity block
// between the owned velocity and the owned pressure part of a distributed block vector).  Plain vectors: Span(n).
struct Span {
  int n, split, gap;
  Span(int n_) : n(n_), split(n_), gap(0) {}
  Span(int n_, int split_, int gap_) : n(n_), split(split_), gap(gap_) {}
};
inline Span blk_span(const nsx_handle *h) { return Span(h->n_u + h->n_p, h->n_u, h->g_u); }

// DPP lane permutation of a double (two 32-bit moves, pure VALU); CTRL as in the ISA: 0xB1/0x4E quad_perm,
// 0x141 row_half_mirror, 0x140 row_mirror, 0x120+n row_ror:n
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xf, 0xf, true);
  hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xf, 0xf, true);
  return __hiloint2double(hi, lo);
}
// sum over the LW lanes of a row group, result in every lane: DPP (pure VALU) up to 16 lanes, then cross-row shuffles
template <int LW>
__device__ __forceinline__ double lane_group_sum(double v) {
  if (LW >= 2) v += dpp_f64<0xB1>(v);    // quad_perm [1,0,3,2]
  if (LW >= 4) v += dpp_f64<0x4E>(v);    // quad_perm [2,3,0,1]
  if (LW >= 8) v += dpp_f64<0x141>(v);   // row_half_mirror
  if (LW >= 16) v += dpp_f64<0x140>(v);  // row_mirror
  if (LW >= 32) v += __shfl_xor(v, 16, 64);
  if (LW >= 64) v += __shfl_xor(v, 32, 64);
  return v;
}
// same, but only the rows of 16 lanes selected by ROW_MASK receive a value; the other rows get 0 (used with the row
// broadcasts 0x142 row_bcast:15 and 0x143 row_bcast:31, which hand the last lane of a row / of the lower half to the rows above)
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_f64_rows(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, ROW_MASK, 0xf, false);
  hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, ROW_MASK, 0xf, false);
  return __hiloint2double(hi, lo);
}

// BLAS-1 (nsx_blas.hip): scalars live in h->scal[slot]
void v_copy(nsx_handle *h, int n, double *d, const double *s);  // raw copy of n contiguous entries
void v_zero(nsx_handle *h, int n, double *d);
void v_add(nsx_handle *h, Span n, double *d, double a, const double *v);                     // d += a v
void v_add_dev(nsx_handle *h, Span n, double *d, double a, int slot, const double *v);       // d += a*scal[slot]*v
void v_sadd(nsx_handle *h, Span n, double *d, double s, double a, const double *v);          // d = s d + a v
void v_scale(nsx_handle *h, Span n, double *d, double a);
void v_scale_dev_inv(nsx_handle *h, Span n, double *d, int slot);                            // d *= 1/scal[slot]
void v_scale_vec(nsx_handle *h, int n, double *d, const double *f);
void v_dot(nsx_handle *h, Span n, const double *a, const double *b, int slot);               // scal[slot] = a.b
void v_add_and_dot(nsx_handle *h, Span n, double *d, double a, int aslot, const double *v, const double *w, int slot);
                                                                                            // d += a*scal[aslot]*v ; scal[slot] = d.w
// modified Gram-Schmidt sweep of SolverGMRES (w against v_0..v_{dim-1}): out[i] = h(i), out[dim] = |w|^2 afterwards (host
// values; scal[slot0+i] holds them too).  normalize: also w *= 1/|w| if the sweep runs as one launch; `normalized` says whether it did.
// after_launch (optional) runs between the launch and the wait for the coefficients, only when the sweep is one launch
// AND normalises w: the caller may enqueue work that depends on the finished w alone.  ahead_stale: after_launch ran, but w was not
// final then after all (the sweep was redone without the persistent grid, or its norm came later): what it enqueued must be redone.
struct MgsResult {
  bool normalized = false, ahead_stale = false;
};
MgsResult v_mgs(nsx_handle *h, Span n, double *w, int dim, double *const *vs, int slot0, bool normalize, double *out,
                const std::function<void()> *after_launch = nullptr, bool consider = false, double *gram = nullptr, const double *ilu_rhs = nullptr);
// SolverGMRES' re-orthogonalisation test: a second sweep is asked for when the first one left |vv| <= 10 |vv_start| sqrt(eps), sqrt(eps) = 2^-26
// exactly.  nrm = |vv| after the sweep, norm0_sq = |vv_start|^2.  ONE expression for the sweep kernels, v_mgs and gmres(): they must agree to the bit.
__host__ __device__ inline bool mgs_wants_second_sweep(double nrm, double norm0_sq) { return !(nrm > 10. * sqrt(norm0_sq) * 1.4901161193847656e-08); }
double *mgs_gram(nsx_handle *h, int depth);  // the Gram matrix (32 x 32) of the basis of the GMRES solve at nesting level depth < 4; allocated and zeroed by the first call
// ilu_rhs: the sweep's input is w = (LU_F)^-1 ilu_rhs, computed first (inside the sweep's own launch where possible: k_ilu_mgs)
// consider: also out[dim+1] = |w|^2 BEFORE the sweep (SolverGMRES' re-orthogonalisation test); a single-launch sweep then
// normalises w only if the test does not ask for a second sweep.
void v_axpy_multi(nsx_handle *h, Span n, double *x, int k, double *const *vs, const double *coef_host);
// x = x0 + sum (x0 == nullptr: x = sum, then optionally x = -y + x) in one launch that only writes x; k <= one launch's worth (MultiArgs: KRYLOV_N_TMP + 2)
void v_axpy_multi_into(nsx_handle *h, Span n, double *x, const double *x0, const double *y, int k, double *const *vs, const double *coef_host);
void finalize_slots(nsx_handle *h, int slot0, int count);
// for kernels that leave nb <= 512 per-workgroup partial sums of a scalar themselves: where to put them, and the
// bookkeeping (and the all-reduce of a distributed run) once the kernel is launched
double *red_out(nsx_handle *h, int slot, int nb);
void after_reduction(nsx_handle *h, int slot, int nb);
int red_blocks(nsx_handle *h, int n);  // per-block partial sums of a reduction over n entries (with a communicator: the same count on every rank)
// fixed-order sum over the block's waves (blockDim.x <= 256), valid in thread 0; sh: 4 doubles
__device__ __forceinline__ double block_sum_256(double v, double *sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
  if (l == 0) sh[w] = v;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0) {
    for (int k = 0; k < (int)(blockDim.x >> 6); ++k) t += sh[k];
  }
  return t;  // valid in thread 0
}
void defer_reductions(nsx_handle *h, bool on);  // hold back / release (merged) the all-reduces of a distributed run
double read_scalar(nsx_handle *h, int slot);
void read_scalars(nsx_handle *h, int slot0, int count, double *out);
unsigned long long publish_scalars(nsx_handle *h, int slot0, int count);  // asynchronous half of read_scalars
void collect_published(nsx_handle *h, unsigned long long seq, int slot0, int count, double *out);
void wait_published(nsx_handle *h, unsigned long long seq);  // host waits for the sequence number of a publication
// Gram-Schmidt sweep (nsx_mgs.hip): what the BLAS file's diagnostics use of it
void mgs_setup(nsx_handle *h);        // mailboxes and resident-grid limits of the persistent sweep, once per handle
int mgs_dirty_words(nsx_handle *h);   // diagnostics: non-empty words of the mailbox region the next sweep would use
// THE choice of a persistent sweep's instantiation: the first of n_inst instantiations (es[k] entries per thread, at most caps[k] resident
// workgroups; caps[k] <= 0: not available) whose grid covers n entries, else the last available one (then per_thread > e)
struct MgsPick {
  int e = 0, nwg = 1, per_thread = 1 << 30;  // entries per thread of the instantiation (0: none available), grid, entries a thread has to take
  bool fits() const { return e != 0 && per_thread <= e; }
};
constexpr int MGS_ENTRIES[3] = {8, 10, 12};  // entries per thread of k_mgs_one's instantiations (mgs_one_fn)
MgsPick mgs_pick(int n, const int *caps, int n_inst, const int *es);
// persistent CG on the Schur complement (nsx_cg.hip); false: not applicable here, use the launch-per-operation solver
void build_cg_plan(nsx_handle *h);   // with the ILU schedules
void cg_pack_values(nsx_handle *h);  // after every schur_numeric
// the bool: this path ran and filled res
bool cg_schur_persistent(nsx_handle *h, double *x, const double *b, double rtol, int maxiter, SolveResult &res);
bool cg_schur_fused(nsx_handle *h, double *x, const double *b, double rtol, int maxiter, SolveResult &res);  // distributed runs: two launches per iteration
int cg_dirty_words(nsx_handle *h);   // diagnostics: non-empty words of the mailbox region the next persistent solve would use
void write_scalar(nsx_handle *h, int slot, double v);

// solver (nsx_solve.hip)
void prec_initialize(nsx_handle *h, int type);
void prec_confirm(nsx_handle *h);  // after the synchronisation behind prec_initialize: ilu_check + the Schur values become reusable
void prec_vmult(nsx_handle *h, int type, double inner_rtol, int inner_maxiter, double *dst, const double *src,
                nsx_solve_stats *st, bool fused);  // fused: NSX_STEP_FUSED as the calling entry of the API read it
void solve_time_step(nsx_handle *h, int type, double tol, double inner_rtol, int maxiter, int inner_maxiter,
                     nsx_solve_stats *st);

// comm (nsx_comm.hip)
void comm_allreduce_scalars(nsx_handle *h, int slot0, int count);
void comm_allreduce_partials(nsx_handle *h, double *partials, int count);  // in place, same count on every rank
bool comm_agree_all(nsx_handle *h, bool mine);  // true iff `mine` is true on every rank (one collective): path choices that change the collective sequence
void comm_release_cus(nsx_handle *h);  // back to the plain compute stream and an unmasked communication stream
bool comm_reserve_cus(nsx_handle *h);  // replace the compute stream by one whose CU mask leaves one CU per XCD free (RCCL's kernel beside a persistent grid)
bool comm_streams_concurrent(nsx_handle *h);  // probe + agreement of all ranks (one collective): may a compute kernel wait for the communication stream?
bool comm_on_stream(const nsx_handle *h);  // RCCL backend: collectives are stream operations (the callback backend runs them on the host)
// the collective inside a persistent grid's exchange: on the communication stream wait for `arrive` to reach `expected`, all-reduce
// vals[0..count), store `seq` in `flag` (nsx_comm.hip)
void comm_ext_allreduce(nsx_handle *h, double *vals, int count, int fail_word, unsigned int *arrive, unsigned int expected, unsigned long long *flag,
                        unsigned long long seq);
void comm_halo(nsx_handle *h, HaloPlan &plan, double *x, int ncomp);
// the same exchange in two halves: begin enqueues pack + send/receive on the communication stream (after everything the
// compute stream holds so far), finish makes the compute stream wait for the ghosts; kernels launched in between overlap it
// packer (optional): fills the send buffer itself on the given stream (values that exist nowhere as a vector yet: the CG direction)
void comm_halo_begin(nsx_handle *h, HaloPlan &plan, double *x, int ncomp,
                     const std::function<void(hipStream_t, double *sendbuf, const int32_t *send_idx, int n_send)> *packer = nullptr);
void comm_halo_finish(nsx_handle *h, HaloPlan &plan, double *x, int ncomp);
void build_row_splits(nsx_handle *h);
inline void comm_halo_u(nsx_handle *h, const double *x) { if (h->dist) comm_halo(h, h->haloU, const_cast<double *>(x), h->dim); }
inline void comm_halo_p(nsx_handle *h, const double *x) { if (h->dist) comm_halo(h, h->haloP, const_cast<double *>(x), 1); }
void comm_destroy(nsx_handle *h);

}  // namespace nsx
