// nsx_surface.hip — surface loads: wall pressure, traction, wall shear stress and y+ at the nodes of a set of boundary faces, and per group
// of faces area, pressure force, viscous force, torque, flow rate and pressure integral; include/nsx.h, section "surface loads".  The
// reference has compute_forces alone (nsx_forces.hip); a deal.II application would loop over the boundary faces with FEFaceValues on the host.
//
// Set-up (nsx_set_surface, host, once per set): validation, the faces stable-sorted by group, the surface-node table and the node -> (face,
// face node) patch lists in tiles of 64 (host/surface_patch.hpp), the block tables of the fold, and the static geometry of every face --
// normal, height, measure from the rows of J^-1 the device holds (geo, downloaded once), the positions of the face nodes from the vertices.
//
//   k_surface_faces  one FACE PER LANE, faces in sorted order.  The lane gathers the cell's NP2 dim velocities and dim + 1 pressures once,
//                    keeps them in registers and walks the 3 | 6 nodes of its face: p, u and grad u at the node's barycentric position with
//                    p2_shape and push_forward_col (nsx_post.hpp; the arithmetic of k_probe_eval), then traction, shear, |shear| and y+.
//                    The values go to SoA planes [plane][face node][face] (coalesced stores); the face's weighted contributions to the
//                    totals (P2 nodal rule) are left as planes [plane][face] -- the "store pass", as k_cell_diag's.
//                    Why a lane per face and not per (face, face node): a wall of 10^4 faces gives 157 waves either for 256 CUs or six
//                    times as many; in both mappings a lane waits for the same chain of three dependent loads (face -> cell -> node ids
//                    -> state) and issues all its gathers back to back behind it, so the launch lasts about one such chain plus the
//                    arithmetic, and a lane per (face, face node) would gather U six times (from L2), add a cross-lane sum for the
//                    totals, and shorten only the arithmetic, which is a few hundred FMAs.  At 10^5 faces there are 1563 waves, more than
//                    one per SIMD.  This is reasoning from the access pattern: the other mapping was not built, so no comparison has been
//                    measured; the launch times of this one are in DESIGN.md section 5.
//                    The loop over the face nodes stays rolled (#pragma unroll 1): which local node a face node is depends on the lane's
//                    face, so the barycentric position is formed by arithmetic from it (no table indexed by a lane's value, as in
//                    k_nodal_fields) and nothing per-node is left to hoist into SGPRs (the trap described above k_cell_diag); a and the
//                    components are unrolled, U is indexed statically and stays in registers: no scratch.
//   k_surface_nodes  one SURFACE NODE PER LANE, one wave per tile of 64 slots sorted by patch length, as k_nodal_fields: walks the patch
//                    list in ascending face position and folds |f| V and |f| left to right in registers.  Results in slot order.
//   k_surface_fold   the "sum pass": a segmented fixed tree per group.  One wave folds 64 consecutive entries of one group of every plane
//                    (lane i takes entry i, then the shuffle tree 32, 16, ..., 1), launched level by level until every group holds one
//                    entry; the block tables depend on the face counts alone.  No atomics: bitwise reproducible, the same for every
//                    internal layout and rank table.  One download of the groups' totals follows (distributed: one all-reduce first).
// The calls read state only.  Algorithmic bytes: the drivers below.
#include <algorithm>
#include <cmath>

#include "../host/surface_patch.hpp"
#include "nsx_post.hpp"

namespace nsx {

constexpr int SURFACE_FOLD = 64;  // entries a wave of k_surface_fold folds
// planes of surface.fvals per face node: p, t [dim], s [dim], |s|, y+;  of surface.nvals: p, t, s, |s|, n [dim];  of surface.contrib: |f|,
// pressure force [dim], viscous force [dim], torque [3 | 1], flux, pressure integral, faces counted
constexpr int surface_face_planes(int dim) { return 2 * dim + 3; }
constexpr int surface_node_planes(int dim) { return 3 * dim + 2; }
constexpr int surface_total_planes(int dim) { return 2 * dim + (dim == 3 ? 3 : 1) + 4; }
inline int surface_components(int dim, int which) { return which == NSX_SURFACE_TRACTION || which == NSX_SURFACE_SHEAR || which == NSX_SURFACE_NORMAL ? dim : 1; }
// first plane of a field in fvals (the normal is not stored per face node: fgeo) / nvals (no y+)
inline int surface_first_plane(int dim, int which) {
  switch (which) {
    case NSX_SURFACE_PRESSURE: return 0;
    case NSX_SURFACE_TRACTION: return 1;
    case NSX_SURFACE_SHEAR: return 1 + dim;
    case NSX_SURFACE_SHEAR_MAGNITUDE: return 1 + 2 * dim;
    default: return 2 + 2 * dim;  // y+ at faces, the normal at nodes
  }
}

struct SurfaceCentre {
  double x[3];
};

// local P2 node of face node j of deal.II face lf: the face's vertices in the order of the face -> vertex tables, then the lines v0 v1, v1 v2,
// v2 v0 (2D: the one line).  By arithmetic: lf is a lane's value.  The host's set-up uses the same function.
template <int DIM>
__host__ __device__ __forceinline__ int surface_local_node(int lf, int j) {
  if constexpr (DIM == 2) {
    return j < 2 ? (lf + j) % 3 : 3 + lf;  // face lf = {lf, lf + 1}; the front-end's line lf is that edge
  } else {
    constexpr unsigned long long FV = 0x312320301210ULL;  // {0,1,2},{1,0,3},{0,2,3},{2,1,3}, a nibble each
    const int m0 = j < 3 ? j : j - 3, m1 = m0 == 2 ? 0 : m0 + 1;
    const int v0 = (int)((FV >> (4 * (lf * 3 + m0))) & 15), v1 = (int)((FV >> (4 * (lf * 3 + m1))) & 15);
    if (j < 3) return v0;
    const int lo = v0 < v1 ? v0 : v1, hi = v0 < v1 ? v1 : v0;  // lines {0,1},{1,2},{2,0},{0,3},{1,3},{2,3}
    return 4 + (hi == 3 ? 3 + lo : (lo == 0 && hi == 2 ? 2 : lo));
  }
}

// cells / lfs [n_faces] sorted; fgeo [DIM + 2][n_faces] (n, d, |f|); fx [DIM][NFN][n_faces]; fvals [surface_face_planes][NFN][n_faces];
// contrib [surface_total_planes][n_faces]
template <int DIM, int NP2>
__global__ __launch_bounds__(64) void k_surface_faces(int n_faces, const int32_t *__restrict__ cells, const int32_t *__restrict__ lfs,
                                                      const uint8_t *__restrict__ counted, int n_cells, const int32_t *__restrict__ cell_n2,
                                                      const int32_t *__restrict__ cell_n1, const double *__restrict__ geo,
                                                      const double *__restrict__ sol, int off_p, double nu, int form, SurfaceCentre centre,
                                                      const double *__restrict__ fgeo, const double *__restrict__ fx,
                                                      double *__restrict__ fvals, double *__restrict__ contrib) {
  constexpr int NV = DIM + 1, NFN = DIM == 3 ? 6 : 3, NTQ = DIM == 3 ? 3 : 1;
  const int f = blockIdx.x * 64 + threadIdx.x;
  if (f >= n_faces) return;
  const int cell = cells[f], lf = lfs[f];
  double n[DIM];
#pragma unroll
  for (int d = 0; d < DIM; ++d) n[d] = fgeo[(size_t)d * n_faces + f];
  const double dwall = fgeo[(size_t)DIM * n_faces + f], area = fgeo[(size_t)(DIM + 1) * n_faces + f];
  double U[NP2][DIM], P[NV];
#pragma unroll
  for (int a = 0; a < NP2; ++a) {
    const int node = cell_n2[(size_t)a * n_cells + cell];
#pragma unroll
    for (int c = 0; c < DIM; ++c) U[a][c] = sol[(size_t)node * DIM + c];
  }
#pragma unroll
  for (int v = 0; v < NV; ++v) P[v] = sol[(size_t)off_p + cell_n1[(size_t)v * n_cells + cell]];
  double fp[DIM], fv[DIM], tq[NTQ], flux = 0.0, pint = 0.0;
#pragma unroll
  for (int i = 0; i < DIM; ++i) fp[i] = fv[i] = 0.0;
#pragma unroll
  for (int i = 0; i < NTQ; ++i) tq[i] = 0.0;
#pragma unroll 1
  for (int j = 0; j < NFN; ++j) {
    // barycentric position of the face node: e_a0, or (e_i + e_j) / 2 for the line a0 - NV (as k_nodal_fields forms it)
    const int a0 = surface_local_node<DIM>(lf, j);
    const int l = a0 - NV, li = l < 3 ? l : l - 3, lj = l < 3 ? (l == 2 ? 0 : l + 1) : 3;
    double lam[NV];
#pragma unroll
    for (int m = 0; m < NV; ++m) lam[m] = a0 < NV ? (m == a0 ? 1.0 : 0.0) : ((m == li || m == lj) ? 0.5 : 0.0);
    double u[DIM], H[DIM][DIM], p = 0.0;
#pragma unroll
    for (int i = 0; i < DIM; ++i) {
      u[i] = 0.0;
#pragma unroll
      for (int k = 0; k < DIM; ++k) H[i][k] = 0.0;
    }
#pragma unroll
    for (int v = 0; v < NV; ++v) p += lam[v] * P[v];
#pragma unroll
    for (int a = 0; a < NP2; ++a) {
      double g[NV], N;
      p2_shape<DIM, true, true>(a, lam, N, g);
#pragma unroll
      for (int i = 0; i < DIM; ++i) {
        u[i] += N * U[a][i];
#pragma unroll
        for (int k = 0; k < DIM; ++k) H[i][k] += U[a][i] * (g[k + 1] - g[0]);
      }
    }
    double G[DIM][DIM];
#pragma unroll
    for (int c = 0; c < DIM; ++c) push_forward_col<DIM>(n_cells, cell, geo, H, c, [&](int i, double s) { G[i][c] = s; });
    double tn[DIM], tnn = 0.0, t[DIM], s[DIM], s2 = 0.0, un = 0.0;
#pragma unroll
    for (int i = 0; i < DIM; ++i) {
      double acc = 0.0;
#pragma unroll
      for (int c = 0; c < DIM; ++c) acc += (form == NSX_SURFACE_SYMMETRIC ? nu * (G[i][c] + G[c][i]) : nu * G[i][c]) * n[c];
      tn[i] = acc;
      tnn += n[i] * acc;
      un += u[i] * n[i];
    }
#pragma unroll
    for (int i = 0; i < DIM; ++i) {
      t[i] = p * n[i] - tn[i];
      s[i] = -(tn[i] - tnn * n[i]);
      s2 += s[i] * s[i];
    }
    const double sm = sqrt(s2);
    double *o = fvals + (size_t)j * n_faces + f;
    const size_t plane = (size_t)NFN * n_faces;
    o[0] = p;
#pragma unroll
    for (int i = 0; i < DIM; ++i) {
      o[(size_t)(1 + i) * plane] = t[i];
      o[(size_t)(1 + DIM + i) * plane] = s[i];
    }
    o[(size_t)(1 + 2 * DIM) * plane] = sm;
    o[(size_t)(2 + 2 * DIM) * plane] = nu > 0.0 ? sqrt(sm) * dwall / nu : 0.0;
    // the P2 nodal rule: 2D |f| (1/6, 1/6, 4/6); 3D |f| / 3 on the mid-edge nodes, the vertices do not enter
    if (DIM == 3 && j < 3) continue;
    const double w = area * (DIM == 3 ? 1.0 / 3.0 : (j < 2 ? 1.0 / 6.0 : 4.0 / 6.0));
    double r[DIM];
#pragma unroll
    for (int d = 0; d < DIM; ++d) r[d] = fx[((size_t)d * NFN + j) * n_faces + f] - centre.x[d];
#pragma unroll
    for (int i = 0; i < DIM; ++i) {
      fp[i] += w * (p * n[i]);
      fv[i] += w * -tn[i];
    }
    if constexpr (DIM == 3) {
      tq[0] += w * (r[1] * t[DIM - 1] - r[DIM - 1] * t[1]);
      tq[1] += w * (r[DIM - 1] * t[0] - r[0] * t[DIM - 1]);
      tq[2] += w * (r[0] * t[1] - r[1] * t[0]);
    } else {
      tq[0] += w * (r[0] * t[1] - r[1] * t[0]);
    }
    flux += w * un;
    pint += w * p;
  }
  const bool mine = counted[cell] != 0;  // a neighbour rank counts the others: they add exact zeros
  double *c = contrib + f;
  int q = 0;
  c[(size_t)(q++) * n_faces] = mine ? area : 0.0;
#pragma unroll
  for (int i = 0; i < DIM; ++i) c[(size_t)(q++) * n_faces] = mine ? fp[i] : 0.0;
#pragma unroll
  for (int i = 0; i < DIM; ++i) c[(size_t)(q++) * n_faces] = mine ? fv[i] : 0.0;
#pragma unroll
  for (int i = 0; i < NTQ; ++i) c[(size_t)(q++) * n_faces] = mine ? tq[i] : 0.0;
  c[(size_t)(q++) * n_faces] = mine ? flux : 0.0;
  c[(size_t)(q++) * n_faces] = mine ? pint : 0.0;
  c[(size_t)(q++) * n_faces] = mine ? 1.0 : 0.0;
}

// tile_ptr [n_tiles + 1], ent [tile_ptr[n_tiles] * 64] (host/surface_patch.hpp); out [surface_node_planes(DIM)][n_slots], n_slots = 64 * gridDim.x.
// A slot without a surface node has an empty list: its planes are exact zeros.
template <int DIM>
__global__ __launch_bounds__(64) void k_surface_nodes(const int32_t *__restrict__ tile_ptr, const int32_t *__restrict__ ent, int n_faces,
                                                      const double *__restrict__ fgeo, const double *__restrict__ fvals, double *__restrict__ out) {
  constexpr int NFN = DIM == 3 ? 6 : 3, NV = 1 + 2 * DIM;  // p, t, s
  const int lane = threadIdx.x;
  const size_t n_slots = (size_t)gridDim.x * 64, slot = (size_t)blockIdx.x * 64 + lane, plane = (size_t)NFN * n_faces;
  const int k0 = tile_ptr[blockIdx.x], k1 = tile_ptr[blockIdx.x + 1];
  double num[NV], nn[DIM], den = 0.0;
#pragma unroll
  for (int v = 0; v < NV; ++v) num[v] = 0.0;
#pragma unroll
  for (int d = 0; d < DIM; ++d) nn[d] = 0.0;
  for (int k = k0; k < k1; ++k) {
    const int32_t e = ent[(size_t)k * 64 + lane];
    if (e < 0) continue;  // this lane's list has ended
    const int f = e >> SURFACE_LOCAL_BITS, j = e & ((1 << SURFACE_LOCAL_BITS) - 1);
    const double a = fgeo[(size_t)(DIM + 1) * n_faces + f];
    const double *src = fvals + (size_t)j * n_faces + f;
#pragma unroll
    for (int v = 0; v < NV; ++v) num[v] += a * src[(size_t)v * plane];
#pragma unroll
    for (int d = 0; d < DIM; ++d) nn[d] += a * fgeo[(size_t)d * n_faces + f];
    den += a;
  }
  double *o = out + slot;
  double s2 = 0.0, n2 = 0.0;
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const double val = den > 0.0 ? num[v] / den : 0.0;
    o[(size_t)v * n_slots] = val;
    if (v > DIM) s2 += val * val;
  }
  o[(size_t)NV * n_slots] = sqrt(s2);
#pragma unroll
  for (int d = 0; d < DIM; ++d) n2 += nn[d] * nn[d];
  const double len = sqrt(n2);
#pragma unroll
  for (int d = 0; d < DIM; ++d) o[(size_t)(NV + 1 + d) * n_slots] = len > 0.0 ? nn[d] / len : 0.0;
}

// Block b folds entries [tab[3 b], tab[3 b + 1]) of every plane of in[.][stride_in] into entry b of out[.][gridDim.x]: lane i takes entry
// tab[3 b] + i (0 behind the end), then the tree 32, 16, ..., 1.
__global__ __launch_bounds__(64) void k_surface_fold(const int32_t *__restrict__ tab, int n_planes, int stride_in, const double *__restrict__ in,
                                                     double *__restrict__ out) {
  const int i = tab[3 * blockIdx.x] + threadIdx.x, i1 = tab[3 * blockIdx.x + 1];
  for (int p = 0; p < n_planes; ++p) {
    double v = i < i1 ? in[(size_t)p * stride_in + i] : 0.0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if (threadIdx.x == 0) out[(size_t)p * gridDim.x + blockIdx.x] = v;
  }
}

// ------------------------------------------------------------------ host drivers
static void surface_check_set(nsx_handle *h, const char *who) {
  post_check_space(h, who);
  if (!h->surface.set) NSX_THROW(NSX_ERR_ARG, "%s: nsx_set_surface first", who);
}

static void set_surface(nsx_handle *h, int n_faces, const int32_t *cells, const int32_t *local_faces, const int32_t *groups, int n_groups, int form,
                        const double *centre) {
  const char *who = "nsx_set_surface";
  post_check_space(h, who);
  if (n_faces < 0) NSX_THROW(NSX_ERR_ARG, "%s: n_faces = %d", who, n_faces);
  if (n_faces == 0) {
    h->surface.clear();
    return;
  }
  const int dim = h->dim, nv = dim + 1, np2 = h->np2, npf = dim == 3 ? 6 : 3, n_cells = h->n_cells;
  if (!cells || !local_faces) NSX_THROW(NSX_ERR_ARG, "%s: null cells / local_faces", who);
  if (n_groups < 1 || n_groups > SURFACE_MAX_GROUPS) NSX_THROW(NSX_ERR_ARG, "%s: n_groups = %d (1 .. %d)", who, n_groups, SURFACE_MAX_GROUPS);
  if (form != NSX_SURFACE_SYMMETRIC && form != NSX_SURFACE_GRADIENT) NSX_THROW(NSX_ERR_ARG, "%s: form %d (NSX_SURFACE_SYMMETRIC | NSX_SURFACE_GRADIENT)", who, form);
  double cen[3] = {0, 0, 0};
  for (int d = 0; centre && d < dim; ++d) {
    if (!std::isfinite(centre[d])) NSX_THROW(NSX_ERR_ARG, "%s: the centre is not finite", who);
    cen[d] = centre[d];
  }
  if (h->cell_n2_in.size() != (size_t)n_cells * np2 || h->cell_coords_in.size() != (size_t)n_cells * nv * dim)
    NSX_THROW(NSX_ERR_ARG, "%s: the handle holds no connectivity", who);
  std::vector<int64_t> pairs((size_t)n_faces);
  for (int f = 0; f < n_faces; ++f) {
    if (cells[f] < 0 || cells[f] >= n_cells || local_faces[f] < 0 || local_faces[f] >= nv) NSX_THROW(NSX_ERR_ARG, "%s: face %d: bad cell / local face", who, f);
    if (groups && (groups[f] < 0 || groups[f] >= n_groups)) NSX_THROW(NSX_ERR_ARG, "%s: face %d: group %d (0 .. %d)", who, f, groups[f], n_groups - 1);
    pairs[f] = (int64_t)cells[f] * 4 + local_faces[f];
  }
  std::sort(pairs.begin(), pairs.end());
  if (std::adjacent_find(pairs.begin(), pairs.end()) != pairs.end()) NSX_THROW(NSX_ERR_ARG, "%s: a (cell, face) pair is given twice", who);
  auto local_node = [&](int lf, int j) { return dim == 2 ? surface_local_node<2>(lf, j) : surface_local_node<3>(lf, j); };
  std::vector<int64_t> node_of((size_t)n_faces * npf);
  for (int f = 0; f < n_faces; ++f)
    for (int j = 0; j < npf; ++j) {
      const int32_t l = h->cell_n2_in[(size_t)cells[f] * np2 + local_node(local_faces[f], j)];  // caller-local: owned < N2 <= ghosts
      node_of[(size_t)f * npf + j] = l < h->N2 ? h->goff_u + l : h->ghost_u[l - h->N2];
    }
  SurfacePatches t;
  if (build_surface_patches(n_faces, npf, node_of.data(), groups, n_groups, t) != 0)
    NSX_THROW(NSX_ERR_ARG, "%s: the surface-node table could not be built (%d faces, %d groups)", who, n_faces, n_groups);
  const std::vector<std::vector<int32_t>> fold = build_surface_fold(t.group_ptr, SURFACE_FOLD);
  // static geometry of every face, in sorted order, from the J^-1 the kernels use
  HIP_CHECK(hipSetDevice(h->prm.device));
  std::vector<double> geo((size_t)(dim * dim + 1) * n_cells);
  h->geo.download(geo.data(), geo.size(), h->stream);
  std::vector<int32_t> scells((size_t)n_faces), slf((size_t)n_faces);
  std::vector<double> fgeo((size_t)(dim + 2) * n_faces), fx((size_t)dim * npf * n_faces), areas((size_t)n_faces);
  for (int p = 0; p < n_faces; ++p) {
    const int f = t.order[p], c = cells[f], lf = local_faces[f], k = dim == 3 ? 3 - lf : (lf + 2) % 3;  // the face lies opposite local vertex k
    scells[p] = c;
    slf[p] = lf;
    double gl[3] = {0, 0, 0}, len2 = 0.0;
    for (int d = 0; d < dim; ++d) {
      if (k > 0) gl[d] = geo[(size_t)((k - 1) * dim + d) * n_cells + c];
      else {
        double s = geo[(size_t)d * n_cells + c];
        for (int r = 1; r < dim; ++r) s += geo[(size_t)(r * dim + d) * n_cells + c];
        gl[d] = -s;
      }
      len2 += gl[d] * gl[d];
    }
    const double len = std::sqrt(len2);
    for (int d = 0; d < dim; ++d) fgeo[(size_t)d * n_faces + p] = -gl[d] / len;
    fgeo[(size_t)dim * n_faces + p] = 1.0 / len;
    areas[f] = fgeo[(size_t)(dim + 1) * n_faces + p] = geo[(size_t)(dim * dim) * n_cells + c] * len * (dim == 3 ? 0.5 : 1.0);
    const double *X = h->cell_coords_in.data() + (size_t)c * nv * dim;
    for (int j = 0; j < npf; ++j) {
      const int a = local_node(lf, j);
      for (int d = 0; d < dim; ++d)
        fx[((size_t)d * npf + j) * n_faces + p] = a < nv ? X[a * dim + d] : 0.5 * (X[P2_LI[a - nv] * dim + d] + X[P2_LJ[a - nv] * dim + d]);
    }
  }
  // everything is checked and built: replace the set
  SurfaceState &s = h->surface;
  s.clear();
  s.n_faces = n_faces;
  s.n_groups = n_groups;
  s.n_nodes = t.n_nodes;
  s.npf = npf;
  s.form = form;
  s.tiles = t.n_tiles;
  s.entries = (int64_t)t.ent.size();
  std::copy(cen, cen + 3, s.centre);
  s.nodes.resize((size_t)t.n_nodes);
  s.owned.resize((size_t)t.n_nodes);
  for (int i = 0; i < t.n_nodes; ++i) {
    s.nodes[i] = (int32_t)t.node_id[i];
    s.owned[i] = t.node_id[i] >= h->goff_u && t.node_id[i] < (int64_t)h->goff_u + h->N2;
  }
  s.areas = std::move(areas);
  s.cells.upload(scells, h->stream);
  s.lf.upload(slf, h->stream);
  s.fgeo.upload(fgeo, h->stream);
  s.fx.upload(fx, h->stream);
  s.tile_ptr.upload(t.tile_ptr, h->stream);
  s.ent.upload(t.ent, h->stream);
  std::vector<int32_t> tab;
  size_t fold_entries = 0;
  for (const auto &lvl : fold) {
    tab.insert(tab.end(), lvl.begin(), lvl.end());
    fold_entries += lvl.size() / 3;
  }
  s.fold_tab.upload(tab, h->stream);
  s.fold_blocks = fold;
  s.fvals.alloc((size_t)surface_face_planes(dim) * npf * n_faces);
  s.nvals.alloc((size_t)surface_node_planes(dim) * t.n_tiles * SURFACE_TILE);
  s.contrib.alloc((size_t)surface_total_planes(dim) * n_faces);
  s.fold.alloc((size_t)surface_total_planes(dim) * fold_entries);
  s.order = std::move(t.order);
  s.face_nodes = std::move(t.face_nodes);
  s.node_group = std::move(t.node_group);
  s.slot_of = std::move(t.slot_of);
  s.set = true;
}

template <int DIM, int NP2>
static void launch_surface(nsx_handle *h) {
  SurfaceState &s = h->surface;
  constexpr int NFN = DIM == 3 ? 6 : 3;
  const double nf = s.n_faces;
  {  // per face: 2 ints, the face geometry and node positions, the cell's ids, J^-1 and gathers, the stores
    const double bytes = nf * (8.0 + 8.0 * (DIM + 2) + 8.0 * DIM * NFN + 1.0 + 4.0 * (NP2 + DIM + 1) + 8.0 * DIM * DIM + 8.0 * (DIM * NP2 + DIM + 1) +
                               8.0 * surface_face_planes(DIM) * NFN + 8.0 * surface_total_planes(DIM));
    LaunchScope ls(h, "surface_faces", bytes);
    SurfaceCentre c{{s.centre[0], s.centre[1], s.centre[2]}};
    hipLaunchKernelGGL((k_surface_faces<DIM, NP2>), dim3(cdiv(s.n_faces, 64)), dim3(64), 0, h->stream, s.n_faces, s.cells.p, s.lf.p, h->diag.counted.p,
                       h->n_cells, h->cell_n2.p, h->cell_n1.p, h->geo.p, h->sol.p, h->off_p, h->prm.nu, s.form, c, s.fgeo.p, s.fx.p, s.fvals.p, s.contrib.p);
  }
  if (s.tiles > 0) {  // every patch entry reads 1 + 3 DIM values and the face's measure and normal
    const double bytes = 4.0 * (double)s.entries + 4.0 * (s.tiles + 1) + 8.0 * (double)s.n_faces * NFN * (2.0 * DIM + 1) + 8.0 * nf * (DIM + 1) +
                         8.0 * surface_node_planes(DIM) * (double)s.tiles * SURFACE_TILE;
    LaunchScope ls(h, "surface_nodes", bytes);
    hipLaunchKernelGGL((k_surface_nodes<DIM>), dim3(s.tiles), dim3(64), 0, h->stream, s.tile_ptr.p, s.ent.p, s.n_faces, s.fgeo.p, s.fvals.p, s.nvals.p);
  }
  HIP_CHECK(hipGetLastError());
}

// the groups' totals [surface_total_planes][n_groups] on the device, behind the last level of the fold
static double *fold_surface(nsx_handle *h) {
  SurfaceState &s = h->surface;
  const int np = surface_total_planes(h->dim);
  LaunchScope ls(h, "surface_fold", 8.0 * np * ((double)s.n_faces + s.n_groups));
  const double *in = s.contrib.p;
  double *out = s.fold.p;
  const int32_t *tab = s.fold_tab.p;
  int stride = s.n_faces;
  for (const auto &lvl : s.fold_blocks) {
    const int nb = (int)(lvl.size() / 3);
    hipLaunchKernelGGL(k_surface_fold, dim3(nb), dim3(64), 0, h->stream, tab, np, stride, in, out);
    in = out;
    stride = nb;
    tab += lvl.size();
    out += (size_t)np * nb;
  }
  HIP_CHECK(hipGetLastError());
  return const_cast<double *>(in);
}

static void compute_surface(nsx_handle *h, nsx_surface_totals *totals) {
  surface_check_set(h, "nsx_compute_surface");
  if (!h->sol.p || h->sol.n < (size_t)h->len_blk) NSX_THROW(NSX_ERR_ARG, "nsx_compute_surface: the handle holds no state yet");
  HIP_CHECK(hipSetDevice(h->prm.device));
  SurfaceState &s = h->surface;
  s.valid = false;  // a failure below leaves no results
  if (h->dim == 2) launch_surface<2, 6>(h);
  else launch_surface<3, 10>(h);
  if (totals) {
    const int dim = h->dim, np = surface_total_planes(dim), ng = s.n_groups, ntq = dim == 3 ? 3 : 1;
    double *dev = fold_surface(h);
    HIP_CHECK(hipStreamSynchronize(h->stream));
    if (h->comm) comm_allreduce_partials(h, dev, np * ng);  // every rank issues it, whatever it holds
    std::vector<double> t((size_t)np * ng);
    HIP_CHECK(hipMemcpyAsync(t.data(), dev, t.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_CHECK(hipStreamSynchronize(h->stream));
    for (int g = 0; g < ng; ++g) {
      nsx_surface_totals o{};
      int q = 0;
      o.area = t[(size_t)(q++) * ng + g];
      for (int i = 0; i < dim; ++i) o.force_pressure[i] = t[(size_t)(q++) * ng + g];
      for (int i = 0; i < dim; ++i) o.force_viscous[i] = t[(size_t)(q++) * ng + g];
      for (int i = 0; i < ntq; ++i) o.torque[dim == 3 ? i : 2] = t[(size_t)(q++) * ng + g];
      o.flux = t[(size_t)(q++) * ng + g];
      o.pressure_integral = t[(size_t)(q++) * ng + g];
      o.n_faces = (int64_t)t[(size_t)(q++) * ng + g];
      totals[g] = o;
    }
  }
  HIP_CHECK(hipStreamSynchronize(h->stream));
  s.valid = true;
}

static void surface_check_get(nsx_handle *h, const char *who, int which) {
  surface_check_set(h, who);
  if (!h->surface.valid) NSX_THROW(NSX_ERR_ARG, "%s: nsx_compute_surface first", who);
  if (which < 0 || which >= NSX_SURFACE_FIELD_COUNT) NSX_THROW(NSX_ERR_ARG, "%s: field %d (NSX_SURFACE_PRESSURE ... NSX_SURFACE_YPLUS)", who, which);
}

static void get_surface_field(nsx_handle *h, int which, int at, double *values) {
  const char *who = "nsx_get_surface_field";
  surface_check_get(h, who, which);
  if (at != NSX_SURFACE_AT_FACES && at != NSX_SURFACE_AT_NODES) NSX_THROW(NSX_ERR_ARG, "%s: at = %d (NSX_SURFACE_AT_FACES | NSX_SURFACE_AT_NODES)", who, at);
  if (which == NSX_SURFACE_YPLUS && at == NSX_SURFACE_AT_NODES) NSX_THROW(NSX_ERR_ARG, "%s: NSX_SURFACE_YPLUS exists at faces only", who);
  if (!values) NSX_THROW(NSX_ERR_ARG, "%s: null values", who);
  HIP_CHECK(hipSetDevice(h->prm.device));
  const SurfaceState &s = h->surface;
  const int dim = h->dim, nc = surface_components(dim, which), npf = s.npf;
  const size_t nf = (size_t)s.n_faces;
  if (at == NSX_SURFACE_AT_FACES) {
    const bool normal = which == NSX_SURFACE_NORMAL;  // the face's own, at each of its nodes
    std::vector<double> v(normal ? (size_t)dim * nf : (size_t)nc * npf * nf);
    const double *src = normal ? s.fgeo.p : s.fvals.p + (size_t)surface_first_plane(dim, which) * npf * nf;
    HIP_CHECK(hipMemcpyAsync(v.data(), src, v.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_CHECK(hipStreamSynchronize(h->stream));
    for (size_t p = 0; p < nf; ++p)
      for (int j = 0; j < npf; ++j)
        for (int k = 0; k < nc; ++k) values[((size_t)s.order[p] * npf + j) * nc + k] = normal ? v[(size_t)k * nf + p] : v[((size_t)k * npf + j) * nf + p];
  } else {
    const size_t n_slots = (size_t)s.tiles * SURFACE_TILE;
    std::vector<double> v((size_t)nc * n_slots);
    HIP_CHECK(hipMemcpyAsync(v.data(), s.nvals.p + (size_t)surface_first_plane(dim, which) * n_slots, v.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_CHECK(hipStreamSynchronize(h->stream));
    for (int i = 0; i < s.n_nodes; ++i)
      for (int k = 0; k < nc; ++k) values[(size_t)i * nc + k] = s.owned[i] ? v[(size_t)k * n_slots + s.slot_of[i]] : 0.0;
  }
}

}  // namespace nsx

extern "C" {

int nsx_set_surface(nsx_handle *h, int n_faces, const int32_t *cells, const int32_t *local_faces, const int32_t *groups, int n_groups, int form,
                    const double *centre) {
  NSX_TRY(h)
  nsx::set_surface(h, n_faces, cells, local_faces, groups, n_groups, form, centre);
  NSX_CATCH(h)
}

int nsx_surface_info(nsx_handle *h, int info[4]) {
  NSX_TRY(h)
  nsx::surface_check_set(h, "nsx_surface_info");
  if (!info) NSX_THROW(NSX_ERR_ARG, "nsx_surface_info: null info");
  info[0] = h->surface.n_faces;
  info[1] = h->surface.n_groups;
  info[2] = h->surface.n_nodes;
  info[3] = h->surface.npf;
  NSX_CATCH(h)
}

int nsx_get_surface_layout(nsx_handle *h, int32_t *nodes, int32_t *node_groups, int32_t *face_nodes, double *areas) {
  NSX_TRY(h)
  nsx::surface_check_set(h, "nsx_get_surface_layout");
  const nsx::SurfaceState &s = h->surface;
  if (nodes) std::copy(s.nodes.begin(), s.nodes.end(), nodes);
  if (node_groups) std::copy(s.node_group.begin(), s.node_group.end(), node_groups);
  if (face_nodes) std::copy(s.face_nodes.begin(), s.face_nodes.end(), face_nodes);
  if (areas) std::copy(s.areas.begin(), s.areas.end(), areas);
  NSX_CATCH(h)
}

int nsx_compute_surface(nsx_handle *h, nsx_surface_totals *totals) {
  NSX_TRY(h)
  nsx::compute_surface(h, totals);
  NSX_CATCH(h)
}

int nsx_surface_field_components(nsx_handle *h, int which, int *n_components) {
  NSX_TRY(h)
  nsx::surface_check_get(h, "nsx_surface_field_components", which);
  if (!n_components) NSX_THROW(NSX_ERR_ARG, "nsx_surface_field_components: null n_components");
  *n_components = nsx::surface_components(h->dim, which);
  NSX_CATCH(h)
}

int nsx_get_surface_field(nsx_handle *h, int which, int at, double *values) {
  NSX_TRY(h)
  nsx::get_surface_field(h, which, at, values);
  NSX_CATCH(h)
}

}  // extern "C"
