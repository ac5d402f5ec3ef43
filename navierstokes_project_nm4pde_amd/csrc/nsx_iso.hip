// nsx_iso.hip — isosurfaces and slices by marching sub-simplices: every P2 cell is cut into linear sub-simplices on its own nodes and each of
// them is contoured by the case tables of host/iso_tables.hpp; include/nsx.h, section "isosurfaces and slices".  No counterpart in the reference.
//
// The output size depends on the data, so one extraction is count, scan, emit -- without atomics: the position of every primitive is the
// exclusive prefix sum of the counts in the caller's cell order, which makes the output a function of the mesh and the state alone.
//
//   k_iso_scalar  one lane per LOCAL NODE (owned and ghost, internal numbering), one coalesced pass: the nodal scalar of the field and of
//                 the colour source go to two planes, so that the cell kernels gather 6 / 10 scalars through cell_n2 instead of re-deriving
//                 them, and so that two cells that share a node classify it from one and the same double.
//                 Algorithmic bytes: per node 16 (two planes written) + the source's reads: velocity 8 (component) / 8 dim (magnitude),
//                 pressure 8 + 16 (map, two values), nodal 4 + 8 (slot, value), plane 8 dim (position).
//   k_iso_count   one CELL PER LANE: gathers the NP2 scalars, classifies the sub-simplices from them alone (no coordinate is read) and writes
//                 the cell's primitive count (0..4 / 0..16) packed with its exclusive prefix inside the workgroup (prefix << 5 | count: one
//                 load tells k_iso_emit everything about an empty cell), and the workgroup total.  The counts are small integers, so the
//                 wave-level prefix is five __ballot masks (one per bit of the count) and popcounts of the lanes below; the waves of a
//                 workgroup meet in LDS.  Cells the handle does not count (diag.counted == 0: another rank's) count 0.
//                 Algorithmic bytes: n_cells (1 + 4) + counted cells (4 NP2 + 8 NP2) + 4 workgroups.
//   k_iso_scan    exclusive prefix sum of the workgroup totals into 64-bit offsets; ONE workgroup that loops over the totals (the bench mesh
//                 has 963 of them at 256 lanes), shuffle scan inside a wave, LDS across the waves, a 64-bit carry from pass to pass.  Integer
//                 sums are exact: the grouping is free.  Algorithmic bytes: 4 workgroups + 8 (workgroups + 1).
//   k_iso_emit    one CELL PER LANE again: an empty cell returns after one load; the others classify again, and every crossing reads its two
//                 nodes' scalars, colours and positions where it needs them (the active cells are O(N^(2/3)) of the mesh: no staging).
//                 Primitives go to offset + k in SoA planes (coalesced in the primitive index); nsx_get_isosurface interleaves them.
//                 Algorithmic bytes: 4 n_cells (packed counts) + 8 workgroups + active cells (4 NP2 + 16 NP2 + 8 (dim+1) dim + 1) + primitives
//                 (8 dim^2 + 8 dim + 4); the host knows the primitives, not the active cells, and states min(counted cells, primitives).
//
// A crossing is computed from the INSIDE node a to the OUTSIDE node b, t = (s_a - iso) / (s_a - s_b), x = x_a + t (x_b - x_a), never by node
// number, and floating-point contraction is off in this file: two cells that share the edge evaluate the same expression on the same
// doubles, so the surface is watertight bit by bit.  A mid-edge position is 0.5 (X_i + X_j), commutative in its operands.
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "../host/iso_tables.hpp"
#include "../host/nodal_patch.hpp"
#include "nsx_post.hpp"

#pragma clang fp contract(off)

namespace nsx {

// one nodal scalar source as the kernels see it; kind < 0: none (the colour of a call without one)
struct IsoSrc {
  int kind, component, plane;  // plane: NSX_ISO_NODAL: first plane of the field in nodal.out + component
  double normal[3];
};

template <int DIM>
__device__ __forceinline__ double iso_node_scalar(const IsoSrc &q, int n, int n_loc, const double *__restrict__ sol, int off_p,
                                                  const int32_t *__restrict__ pmap, const double *__restrict__ nodex,
                                                  const int32_t *__restrict__ slot, const double *__restrict__ nodal_out, size_t n_slots) {
  if (q.kind == NSX_ISO_VELOCITY) {
    if (q.component >= 0) return sol[(size_t)n * DIM + q.component];
    double ss = 0.0;
#pragma unroll
    for (int i = 0; i < DIM; ++i) {
      const double u = sol[(size_t)n * DIM + i];
      ss = ss + u * u;
    }
    return sqrt(ss);
  }
  if (q.kind == NSX_ISO_PRESSURE) {
    const int32_t a = pmap[n], b = pmap[(size_t)n_loc + n];
    const double pa = sol[(size_t)off_p + a];
    return b < 0 ? pa : 0.5 * (pa + sol[(size_t)off_p + b]);
  }
  if (q.kind == NSX_ISO_NODAL) {
    const int32_t s = slot[n];
    return s < 0 ? 0.0 : nodal_out[(size_t)q.plane * n_slots + s];
  }
  double s = 0.0;  // NSX_ISO_PLANE
#pragma unroll
  for (int d = 0; d < DIM; ++d) s = s + q.normal[d] * nodex[(size_t)d * n_loc + n];
  return s;
}

template <int DIM>
__global__ __launch_bounds__(256) void k_iso_scalar(int n_loc, IsoSrc field, IsoSrc colour, const double *__restrict__ sol, int off_p,
                                                    const int32_t *__restrict__ pmap, const double *__restrict__ nodex,
                                                    const int32_t *__restrict__ slot, const double *__restrict__ nodal_out, size_t n_slots,
                                                    double *__restrict__ s) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= n_loc) return;
  s[n] = iso_node_scalar<DIM>(field, n, n_loc, sol, off_p, pmap, nodex, slot, nodal_out, n_slots);
  if (colour.kind >= 0) s[(size_t)n_loc + n] = iso_node_scalar<DIM>(colour, n, n_loc, sol, off_p, pmap, nodex, slot, nodal_out, n_slots);
}

// bit a of `in`: local node a is inside (s >= iso); bit a of `fin`: its scalar is finite
template <int NP2>
__device__ __forceinline__ void iso_classify(int n_cells, int cell, const int32_t *__restrict__ cell_n2, const double *__restrict__ s, double iso,
                                             unsigned &in, unsigned &fin) {
  in = fin = 0u;
#pragma unroll
  for (int a = 0; a < NP2; ++a) {
    const double v = s[cell_n2[(size_t)a * n_cells + cell]];
    in |= (unsigned)(v >= iso) << a;
    fin |= (unsigned)(isfinite(v) ? 1 : 0) << a;
  }
}

// case index of sub-simplex `sub` (bit v: its vertex v is inside), -1 when one of its scalars is not finite
template <int DIM>
__device__ __forceinline__ int iso_case(int sub, unsigned in, unsigned fin) {
  int m = 0;
  bool ok = true;
#pragma unroll
  for (int v = 0; v <= DIM; ++v) {
    const int a = DIM == 3 ? ISO_SUB_TET[sub][v] : ISO_SUB_TRI[sub][v];
    m |= (int)((in >> a) & 1u) << v;
    ok = ok && ((fin >> a) & 1u);
  }
  return ok ? m : -1;
}

// pack[cell] = exclusive prefix of the counts inside the workgroup << 5 | count; wg_tot[workgroup] = sum of its counts.  blockDim.x = 64 / 128 / 256.
template <int DIM, int NP2>
__global__ __launch_bounds__(256) void k_iso_count(int n_cells, const uint8_t *__restrict__ counted, const int32_t *__restrict__ cell_n2,
                                                   const double *__restrict__ s, double iso, int32_t *__restrict__ pack, int32_t *__restrict__ wg_tot) {
  __shared__ int wsum[4];
  const int cell = blockIdx.x * blockDim.x + threadIdx.x;
  int cnt = 0;
  if (cell < n_cells && counted[cell]) {
    unsigned in, fin;
    iso_classify<NP2>(n_cells, cell, cell_n2, s, iso, in, fin);
#pragma unroll
    for (int sub = 0; sub < (DIM == 3 ? ISO_SUB3 : ISO_SUB2); ++sub) {
      const int m = iso_case<DIM>(sub, in, fin);
      if (m >= 0) {
        const int pop = __popc((unsigned)m);  // the counts of ISO_TET_N / ISO_TRI_N by arithmetic: no table is indexed by a lane's value
        cnt += DIM == 3 ? (pop == 2 ? 2 : (pop == 1 || pop == 3) ? 1 : 0) : ((pop == 1 || pop == 2) ? 1 : 0);
      }
    }
  }
  // counts are 0..16: the wave's exclusive prefix from one ballot per bit
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  int pre = 0, tot = 0;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const unsigned long long m = __ballot((cnt >> k) & 1);
    pre += __popcll(m & below) << k;
    tot += __popcll(m) << k;
  }
  if (lane == 0) wsum[w] = tot;
  __syncthreads();
  int base = 0, all = 0;
  for (int k = 0; k < (int)(blockDim.x >> 6); ++k) {
    if (k < w) base += wsum[k];
    all += wsum[k];
  }
  if (cell < n_cells) pack[cell] = ((base + pre) << 5) | cnt;
  if (threadIdx.x == 0) wg_tot[blockIdx.x] = all;
}

// off[i] = tot[0] + ... + tot[i - 1] (i = 0..n), one workgroup of 64 / 128 / 256 lanes looping over the totals
__global__ __launch_bounds__(256) void k_iso_scan(int n, const int32_t *__restrict__ tot, long long *__restrict__ off) {
  __shared__ long long wsum[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  long long carry = 0;
  for (int first = 0; first < n; first += (int)blockDim.x) {
    const int i = first + (int)threadIdx.x;
    const long long v = i < n ? (long long)tot[i] : 0ll;
    long long x = v;  // inclusive scan inside the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const long long y = __shfl_up(x, o, 64);
      if (lane >= o) x += y;
    }
    if (lane == 63) wsum[w] = x;
    __syncthreads();
    long long base = 0, all = 0;
    for (int k = 0; k < (int)(blockDim.x >> 6); ++k) {
      if (k < w) base += wsum[k];
      all += wsum[k];
    }
    if (i < n) off[i] = carry + base + x - v;
    carry += all;
    __syncthreads();  // wsum is written again by the next pass
  }
  if (threadIdx.x == 0) off[n] = carry;
}

// coordinate d of local node a of the cell: the vertex, or 0.5 (X_i + X_j) of the line a - (DIM + 1) = {i, j} (i and j by arithmetic)
template <int DIM>
__device__ __forceinline__ double iso_node_x(int n_cells, int cell, const double *__restrict__ cellx, int a, int d) {
  constexpr int NV = DIM + 1;
  if (a < NV) return cellx[(size_t)(a * DIM + d) * n_cells + cell];
  const int l = a - NV, i = l < 3 ? l : l - 3, j = l < 3 ? (l == 2 ? 0 : l + 1) : 3;
  return 0.5 * (cellx[(size_t)(i * DIM + d) * n_cells + cell] + cellx[(size_t)(j * DIM + d) * n_cells + cell]);
}

// s: the field plane; sc: the colour plane or null.  pts [DIM * DIM][cap] (plane = vertex * DIM + coordinate), col [DIM][cap], cells [cap].
template <int DIM, int NP2>
__global__ __launch_bounds__(256) void k_iso_emit(int n_cells, const int32_t *__restrict__ cell_n2, const double *__restrict__ s,
                                                  const double *__restrict__ sc, double iso, const int32_t *__restrict__ pack,
                                                  const long long *__restrict__ wg_off, const double *__restrict__ cellx,
                                                  const uint8_t *__restrict__ flip, long long cap, double *__restrict__ pts, double *__restrict__ col,
                                                  int32_t *__restrict__ cells) {
  const int cell = blockIdx.x * blockDim.x + threadIdx.x;
  if (cell >= n_cells) return;
  const int32_t p = pack[cell];
  const int cnt = p & 31;
  if (cnt == 0) return;
  const long long first = wg_off[blockIdx.x] + (long long)(p >> 5);
  if (first < 0 || first + cnt > cap) return;  // never past the buffers, whatever the tables hold
  const bool swap = flip[cell] != 0;
  unsigned in, fin;
  iso_classify<NP2>(n_cells, cell, cell_n2, s, iso, in, fin);
  int k = 0;
#pragma unroll
  for (int sub = 0; sub < (DIM == 3 ? ISO_SUB3 : ISO_SUB2); ++sub) {
    const int m = iso_case<DIM>(sub, in, fin);
    if (m < 0) continue;
    const int n_prim = DIM == 3 ? ISO_TET_N[m] : ISO_TRI_N[m];
    for (int t = 0; t < n_prim && k < cnt; ++t, ++k) {
      const long long o = first + k;
      cells[o] = cell;
#pragma unroll
      for (int v = 0; v < DIM; ++v) {
        const int code = DIM == 3 ? ISO_TET_V[m][3 * t + v] : ISO_TRI_V[m][v];
        const int a = DIM == 3 ? ISO_SUB_TET[sub][code >> 2] : ISO_SUB_TRI[sub][code >> 2];  // inside
        const int b = DIM == 3 ? ISO_SUB_TET[sub][code & 3] : ISO_SUB_TRI[sub][code & 3];    // outside
        const int na = cell_n2[(size_t)a * n_cells + cell], nb = cell_n2[(size_t)b * n_cells + cell];
        const double sa = s[na], sb = s[nb];
        const double tt = (sa - iso) / (sa - sb);
        // the last two vertices change places in a cell of negative orientation
        const int vo = !swap ? v : (DIM == 3 ? (v == 0 ? 0 : 3 - v) : 1 - v);
#pragma unroll
        for (int d = 0; d < DIM; ++d) {
          const double xa = iso_node_x<DIM>(n_cells, cell, cellx, a, d), xb = iso_node_x<DIM>(n_cells, cell, cellx, b, d);
          pts[(size_t)(vo * DIM + d) * cap + o] = xa + tt * (xb - xa);
        }
        if (sc) {
          const double ca = sc[na], cb = sc[nb];
          col[(size_t)vo * cap + o] = ca + tt * (cb - ca);
        }
      }
    }
  }
}

// ------------------------------------------------------------------ host drivers
// validates one source and translates it for the kernels
static IsoSrc iso_source(nsx_handle *h, const nsx_iso_source *q, const char *role) {
  IsoSrc r{};
  r.kind = q->kind;
  r.component = q->component;
  const int dim = h->dim;
  switch (q->kind) {
    case NSX_ISO_VELOCITY:
      if (q->component < -1 || q->component >= dim)
        NSX_THROW(NSX_ERR_ARG, "nsx_extract_isosurface: %s: velocity component %d (-1: magnitude, 0 .. %d)", role, q->component, dim - 1);
      break;
    case NSX_ISO_PRESSURE:
      break;
    case NSX_ISO_NODAL:
      if (h->dist) NSX_THROW(NSX_ERR_UNSUPPORTED, "nsx_extract_isosurface: %s: NSX_ISO_NODAL with more than one process (ghost nodes have no nodal results)", role);
      if (q->which < 0 || q->which >= NSX_FIELD_COUNT)
        NSX_THROW(NSX_ERR_ARG, "nsx_extract_isosurface: %s: nodal field %d (NSX_FIELD_GRADIENT ... NSX_FIELD_DIVERGENCE)", role, q->which);
      if (q->component < 0 || q->component >= nodal_components(dim, q->which))
        NSX_THROW(NSX_ERR_ARG, "nsx_extract_isosurface: %s: component %d of a nodal field with %d", role, q->component, nodal_components(dim, q->which));
      if (!h->nodal.have_patches || !h->nodal.valid) NSX_THROW(NSX_ERR_ARG, "nsx_extract_isosurface: %s: NSX_ISO_NODAL needs nsx_compute_nodal_fields first", role);
      r.plane = nodal_first_plane(dim, q->which) + q->component;
      break;
    case NSX_ISO_PLANE: {
      bool finite = true, zero = true;
      for (int d = 0; d < dim; ++d) {
        finite = finite && std::isfinite(q->normal[d]);
        zero = zero && q->normal[d] == 0.0;
        r.normal[d] = q->normal[d];
      }
      if (!finite || zero) NSX_THROW(NSX_ERR_ARG, "nsx_extract_isosurface: %s: the plane normal is not finite or all zero", role);
      break;
    }
    default:
      NSX_THROW(NSX_ERR_ARG, "nsx_extract_isosurface: %s: kind %d (NSX_ISO_VELOCITY ... NSX_ISO_PLANE)", role, q->kind);
  }
  return r;
}

static double iso_source_bytes(const IsoSrc &q, int dim) {
  switch (q.kind) {
    case NSX_ISO_VELOCITY: return q.component >= 0 ? 8.0 : 8.0 * dim;
    case NSX_ISO_PRESSURE: return 8.0 + 16.0;
    case NSX_ISO_NODAL: return 4.0 + 8.0;
    case NSX_ISO_PLANE: return 8.0 * dim;
  }
  return 0.0;
}

// vertex coordinates of the cells, SoA, and the orientation of every cell: by the first extract on a mesh (cells are never renumbered)
void iso_ensure_coords(nsx_handle *h) {
  if (h->iso.have_coords) return;
  const int dim = h->dim, nv = dim + 1, nc = h->n_cells;
  if (h->cell_coords_in.size() != (size_t)nc * nv * dim) NSX_THROW(NSX_ERR_ARG, "nsx_extract_isosurface: the handle holds no cell coordinates");
  std::vector<double> x((size_t)nv * dim * nc);
  std::vector<uint8_t> flip((size_t)nc);
  for (int c = 0; c < nc; ++c) {
    const double *X = h->cell_coords_in.data() + (size_t)c * nv * dim;
    for (int v = 0; v < nv; ++v)
      for (int d = 0; d < dim; ++d) x[(size_t)(v * dim + d) * nc + c] = X[v * dim + d];
    double J[3][3] = {{0}}, det;
    for (int d = 0; d < dim; ++d)
      for (int k = 0; k < dim; ++k) J[d][k] = X[(k + 1) * dim + d] - X[d];
    if (dim == 2)
      det = J[0][0] * J[1][1] - J[0][1] * J[1][0];
    else
      det = J[0][0] * (J[1][1] * J[2][2] - J[1][2] * J[2][1]) - J[0][1] * (J[1][0] * J[2][2] - J[1][2] * J[2][0]) +
            J[0][2] * (J[1][0] * J[2][1] - J[1][1] * J[2][0]);  // the expression of setup_mesh
    flip[c] = det < 0.0;
  }
  h->iso.cellx.upload(x, h->stream);
  h->iso.flip.upload(flip, h->stream);
  h->iso.have_coords = true;
}

// the maps over the LOCAL nodes in the INTERNAL numbering (cell_n2_h / cell_n1_h): rebuilt when a layout moves the nodes
static void iso_ensure_maps(nsx_handle *h) {
  if (h->iso.map_epoch == h->layout_epoch) return;
  const int dim = h->dim, nv = dim + 1, np2 = h->np2, np1 = h->np1, nc = h->n_cells, n_loc = h->N2_loc;
  std::vector<int32_t> pmap((size_t)2 * n_loc, 0);
  std::vector<double> nx((size_t)dim * n_loc, 0.0);
  for (int n = 0; n < n_loc; ++n) pmap[(size_t)n_loc + n] = -1;
  for (int c = 0; c < nc; ++c) {
    const int32_t *c2 = h->cell_n2_h.data() + (size_t)c * np2, *c1 = h->cell_n1_h.data() + (size_t)c * np1;
    const double *X = h->cell_coords_in.data() + (size_t)c * nv * dim;
    for (int a = 0; a < np2; ++a) {
      const int32_t n = c2[a];
      if (n < 0 || n >= n_loc) NSX_THROW(NSX_ERR_ARG, "nsx_extract_isosurface: cell %d names node %d", c, n);
      if (a < nv) {
        pmap[n] = c1[a];
        pmap[(size_t)n_loc + n] = -1;
        for (int d = 0; d < dim; ++d) nx[(size_t)d * n_loc + n] = X[a * dim + d];
      } else {
        const int i = P2_LI[a - nv], j = P2_LJ[a - nv];
        pmap[n] = c1[i];
        pmap[(size_t)n_loc + n] = c1[j];
        for (int d = 0; d < dim; ++d) nx[(size_t)d * n_loc + n] = 0.5 * (X[i * dim + d] + X[j * dim + d]);
      }
    }
  }
  for (size_t k = 0; k < pmap.size(); ++k)
    if (pmap[k] < -1 || pmap[k] >= h->NP_loc) NSX_THROW(NSX_ERR_ARG, "nsx_extract_isosurface: the node map names pressure node %d", pmap[k]);
  h->iso.pmap.upload(pmap, h->stream);
  h->iso.nodex.upload(nx, h->stream);
  h->iso.map_epoch = h->layout_epoch;
}

// internal node -> slot of nodal.out, from the layout's node permutation and nodal.slot_of (caller-local owned node -> slot)
void iso_ensure_slots(nsx_handle *h) {
  if (h->iso.slot_epoch == h->layout_epoch) return;
  const size_t n_slots = (size_t)h->nodal.tiles * NODAL_TILE;
  std::vector<int32_t> slot((size_t)h->N2_loc, -1);
  for (int n = 0; n < h->N2; ++n) {
    const int32_t caller = h->layout_on ? h->iperm2_h[n] : n;
    const int32_t s = h->nodal.slot_of[caller];
    if (s < 0 || (size_t)s >= n_slots) NSX_THROW(NSX_ERR_ARG, "nsx_extract_isosurface: node %d has slot %d of the nodal results", caller, s);
    slot[n] = s;
  }
  h->iso.slot.upload(slot, h->stream);
  h->iso.slot_epoch = h->layout_epoch;
}

static int iso_wg_width() {
  const int w = env_int("NSX_ISO_WG", 256);
  return (w == 64 || w == 128) ? w : 256;
}

template <int DIM, int NP2>
static void launch_iso_front(nsx_handle *h, const IsoSrc &f, const IsoSrc &c, double iso, int wg, int n_wg) {
  const int n_loc = h->N2_loc, nc = h->n_cells;
  const size_t n_slots = (size_t)h->nodal.tiles * NODAL_TILE;
  {
    LaunchScope ls(h, "iso_scalar", (double)n_loc * (16.0 + iso_source_bytes(f, DIM) + iso_source_bytes(c, DIM)));
    hipLaunchKernelGGL((k_iso_scalar<DIM>), dim3(cdiv(n_loc, 256)), dim3(256), 0, h->stream, n_loc, f, c, h->sol.p, h->off_p, h->iso.pmap.p, h->iso.nodex.p,
                       h->iso.slot.p, h->nodal.out.p, n_slots, h->iso.s.p);
  }
  {
    LaunchScope ls(h, "iso_count", 5.0 * nc + (double)h->diag.n_counted * 12.0 * NP2 + 4.0 * n_wg);
    hipLaunchKernelGGL((k_iso_count<DIM, NP2>), dim3(n_wg), dim3(wg), 0, h->stream, nc, h->diag.counted.p, h->cell_n2.p, h->iso.s.p, iso, h->iso.pack.p,
                       h->iso.wg_tot.p);
  }
  {
    LaunchScope ls(h, "iso_scan", 4.0 * n_wg + 8.0 * (n_wg + 1));
    hipLaunchKernelGGL(k_iso_scan, dim3(1), dim3(wg), 0, h->stream, n_wg, h->iso.wg_tot.p, h->iso.wg_off.p);
  }
}

template <int DIM, int NP2>
static void launch_iso_emit(nsx_handle *h, bool colour, double iso, int wg, int n_wg, int64_t n) {
  const int nc = h->n_cells;
  const double active = (double)std::min<int64_t>(h->diag.n_counted, n);
  LaunchScope ls(h, "iso_emit", 4.0 * nc + 8.0 * n_wg + active * (20.0 * NP2 + 8.0 * (DIM + 1) * DIM + 1.0) + (double)n * (8.0 * DIM * DIM + 8.0 * DIM + 4.0));
  hipLaunchKernelGGL((k_iso_emit<DIM, NP2>), dim3(n_wg), dim3(wg), 0, h->stream, nc, h->cell_n2.p, h->iso.s.p, colour ? h->iso.s.p + h->N2_loc : nullptr, iso,
                     h->iso.pack.p, h->iso.wg_off.p, h->iso.cellx.p, h->iso.flip.p, (long long)h->iso.cap, h->iso.pts.p, h->iso.col.p, h->iso.cells.p);
}

static void extract_isosurface(nsx_handle *h, const nsx_iso_source *field, double isovalue, const nsx_iso_source *colour, int64_t *n_primitives) {
  post_check_space(h, "nsx_extract_isosurface");
  if (!field || !n_primitives) NSX_THROW(NSX_ERR_ARG, "nsx_extract_isosurface: null field / n_primitives");
  if (!h->sol.p || h->sol.n < (size_t)h->len_blk) NSX_THROW(NSX_ERR_ARG, "nsx_extract_isosurface: the handle holds no state yet");
  if (!std::isfinite(isovalue)) NSX_THROW(NSX_ERR_ARG, "nsx_extract_isosurface: the isovalue is not finite");
  const IsoSrc f = iso_source(h, field, "field");
  IsoSrc c{};
  c.kind = -1;
  if (colour) c = iso_source(h, colour, "colour");
  HIP_CHECK(hipSetDevice(h->prm.device));
  const int dim = h->dim, nc = h->n_cells, wg = iso_wg_width(), n_wg = cdiv(nc, wg);
  iso_ensure_coords(h);
  iso_ensure_maps(h);
  if (f.kind == NSX_ISO_NODAL || c.kind == NSX_ISO_NODAL) iso_ensure_slots(h);
  if (h->iso.s.n < (size_t)2 * h->N2_loc) h->iso.s.alloc((size_t)2 * h->N2_loc);
  if (h->iso.pack.n < (size_t)nc) h->iso.pack.alloc(nc);
  if (h->iso.wg_tot.n < (size_t)n_wg) h->iso.wg_tot.alloc(n_wg);
  if (h->iso.wg_off.n < (size_t)n_wg + 1) h->iso.wg_off.alloc((size_t)n_wg + 1);
  if (dim == 2) launch_iso_front<2, 6>(h, f, c, isovalue, wg, n_wg);
  else launch_iso_front<3, 10>(h, f, c, isovalue, wg, n_wg);
  HIP_CHECK(hipGetLastError());
  long long total = 0;
  HIP_CHECK(hipMemcpyAsync(&total, h->iso.wg_off.p + n_wg, sizeof(total), hipMemcpyDeviceToHost, h->stream));
  HIP_CHECK(hipStreamSynchronize(h->stream));
  if (total < 0 || total > (long long)nc * (dim == 3 ? ISO_MAX_PRIMS_3D : ISO_MAX_PRIMS_2D))
    NSX_THROW(NSX_ERR_NUMERIC, "nsx_extract_isosurface: the scan returned %lld primitives for %d cells", total, nc);
  if (total > (long long)INT32_MAX) NSX_THROW(NSX_ERR_UNSUPPORTED, "nsx_extract_isosurface: %lld primitives (more than 2^31 - 1)", total);
  // from here on the earlier result is given up
  h->iso.valid = false;
  if (total > h->iso.cap || !h->iso.pts.p) {  // grow, never shrink
    const int64_t cap = std::max<int64_t>(total, 1);
    h->iso.pts.alloc((size_t)dim * dim * cap);
    h->iso.col.alloc((size_t)dim * cap);
    h->iso.cells.alloc((size_t)cap);
    h->iso.cap = cap;
  }
  if (total > 0) {
    if (dim == 2) launch_iso_emit<2, 6>(h, c.kind >= 0, isovalue, wg, n_wg, total);
    else launch_iso_emit<3, 10>(h, c.kind >= 0, isovalue, wg, n_wg, total);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipStreamSynchronize(h->stream));
  }
  h->iso.n = total;
  h->iso.has_colour = c.kind >= 0;
  h->iso.valid = true;
  *n_primitives = total;
}

static void get_isosurface(nsx_handle *h, double *points, double *colour, int32_t *cells) {
  post_check_space(h, "nsx_get_isosurface");
  if (!h->iso.valid) NSX_THROW(NSX_ERR_ARG, "nsx_get_isosurface: nsx_extract_isosurface first");
  if (colour && !h->iso.has_colour) NSX_THROW(NSX_ERR_ARG, "nsx_get_isosurface: the last nsx_extract_isosurface had no colour source");
  const int dim = h->dim;
  const size_t n = (size_t)h->iso.n, cap = (size_t)h->iso.cap;
  if (n == 0) return;
  HIP_CHECK(hipSetDevice(h->prm.device));
  const int np = (points ? dim * dim : 0), ncol = (colour ? dim : 0);
  std::vector<double> v((size_t)(np + ncol) * n);
  for (int p = 0; p < np; ++p) HIP_CHECK(hipMemcpyAsync(v.data() + (size_t)p * n, h->iso.pts.p + (size_t)p * cap, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  for (int p = 0; p < ncol; ++p)
    HIP_CHECK(hipMemcpyAsync(v.data() + (size_t)(np + p) * n, h->iso.col.p + (size_t)p * cap, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  if (cells) HIP_CHECK(hipMemcpyAsync(cells, h->iso.cells.p, n * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  HIP_CHECK(hipStreamSynchronize(h->stream));
  for (size_t i = 0; i < n; ++i) {
    for (int p = 0; p < np; ++p) points[i * np + p] = v[(size_t)p * n + i];
    for (int p = 0; p < ncol; ++p) colour[i * ncol + p] = v[(size_t)(np + p) * n + i];
  }
}

}  // namespace nsx

extern "C" {

int nsx_extract_isosurface(nsx_handle *h, const nsx_iso_source *field, double isovalue, const nsx_iso_source *colour, int64_t *n_primitives) {
  NSX_TRY(h)
  nsx::extract_isosurface(h, field, isovalue, colour, n_primitives);
  NSX_CATCH(h)
}

int nsx_get_isosurface(nsx_handle *h, double *points, double *colour, int32_t *cells) {
  NSX_TRY(h)
  nsx::get_isosurface(h, points, colour, cells);
  NSX_CATCH(h)
}

}  // extern "C"
