// nsx_nodal.hip — nodal derived fields: the recovered velocity gradient at every P2 node this handle owns and what follows from it
// (vorticity, Q, strain rate, divergence); include/nsx.h, section "nodal fields".  No counterpart in the reference.
//
//   Gbar(n) = ( sum_c |c| grad u_h|_c(x_n) ) / ( sum_c |c| ),   c over the cells that hold n, in ascending position of the caller's cell list
//
// Everything the kernel needs already sits on the device -- cell_n2, geo (J^-1, |det J|) and the ghosted `solution`; the first call on a
// mesh adds the node -> (cell, local node) patch table, built on the host from the connectivity as handed over (host/nodal_patch.hpp).
//
//   k_nodal_fields  NODE-CENTRIC GATHER, one NODE PER LANE, one wave per workgroup = one tile of 64 slots of the patch table.  A lane walks
//                   the list of its node: per entry (cell, a) it gathers the cell's NP2 node ids and NP2 dim velocities and J^-1, evaluates
//                   grad u_h at the barycentric position of local node a (e_a for a vertex, (e_i + e_j) / 2 for the line {i, j}) with the
//                   arithmetic of k_probe_eval, and folds |c| grad u_h and |c| into registers, left to right.  One launch, no intermediate
//                   buffer, no atomics: the order of every sum is the order of the list, so the result depends on the mesh and the state
//                   alone -- not on the scheduling, nsx_set_ranks or nsx_set_internal_layout (the table is in the caller's node and cell
//                   numbering; cell_n2 translates to the internal one).
//                   Imbalance: patches hold 1 to about 30 cells.  The table deals the nodes to the slots by descending patch size, so the
//                   64 lanes of a wave walk lists of (nearly) one length -- a wave runs as many steps as ITS longest list, not the mesh's
//                   -- and stores every step of a tile as one row of 64 entries (a coalesced load).  The long tiles come first in the grid.
//                   Results go to SoA planes [nodal_planes(dim)][n_slots] in SLOT order (coalesced stores); nsx_get_nodal_field undoes the
//                   slot order on the host while it interleaves the components.
//                   Algorithmic bytes per launch (every operand once): 8 dim N2_loc (state) + n_cells (4 NP2 + 8 (dim^2 + 1)) (cell tables)
//                   + 4 table entries + 4 (n_tiles + 1) + 8 nodal_planes(dim) n_slots (results).  The gathers re-read the cell tables and the
//                   state once per (cell, local node) pair, NP2 times per cell; those re-reads are served by the caches.
#include <algorithm>
#include <cmath>

#include "../host/nodal_patch.hpp"
#include "nsx_post.hpp"

namespace nsx {

// tile_ptr [n_tiles + 1], ent [tile_ptr[n_tiles] * 64] (host/nodal_patch.hpp); out [nodal_planes(DIM)][n_slots], n_slots = 64 * gridDim.x.
// A slot without a node, and a node in no cell, has an empty list: its planes are exact zeros.
template <int DIM, int NP2>
__global__ __launch_bounds__(64) void k_nodal_fields(const int32_t *__restrict__ tile_ptr, const int32_t *__restrict__ ent, int n_cells,
                                                     const int32_t *__restrict__ cell_n2, const double *__restrict__ geo,
                                                     const double *__restrict__ sol, double *__restrict__ out) {
  constexpr int NV = DIM + 1;
  constexpr double REF_VOL = DIM == 3 ? 1.0 / 6.0 : 0.5;
  const int lane = threadIdx.x;
  const size_t n_slots = (size_t)gridDim.x * 64, slot = (size_t)blockIdx.x * 64 + lane;
  const int k0 = tile_ptr[blockIdx.x], k1 = tile_ptr[blockIdx.x + 1];
  double num[DIM][DIM], den = 0.0;
#pragma unroll
  for (int i = 0; i < DIM; ++i)
#pragma unroll
    for (int j = 0; j < DIM; ++j) num[i][j] = 0.0;
  for (int k = k0; k < k1; ++k) {
    const int32_t e = ent[(size_t)k * 64 + lane];
    if (e < 0) continue;  // this lane's list has ended (the lists of a tile are padded to the longest)
    const int cell = e >> NODAL_LOCAL_BITS, a0 = e & ((1 << NODAL_LOCAL_BITS) - 1);
    // barycentric position of local node a0: e_a0, or (e_i + e_j) / 2 for the line a0 - NV = {i, j} in the front-end's line order
    // {0,1},{1,2},{2,0}[,{0,3},{1,3},{2,3}]; i and j by arithmetic, so that no table is indexed by a lane's value
    const int l = a0 - NV, li = l < 3 ? l : l - 3, lj = l < 3 ? (l == 2 ? 0 : l + 1) : 3;
    double lam[NV];
#pragma unroll
    for (int m = 0; m < NV; ++m) lam[m] = a0 < NV ? (m == a0 ? 1.0 : 0.0) : ((m == li || m == lj) ? 0.5 : 0.0);
    double H[DIM][DIM];
#pragma unroll
    for (int i = 0; i < DIM; ++i)
#pragma unroll
      for (int q = 0; q < DIM; ++q) H[i][q] = 0.0;
    // g[m] = dN_a / d lambda_m (p2_shape, nsx_post.hpp), dN_a / d xi_q = g[q + 1] - g[0], H = sum_a U_a (x) grad_ref N_a
#pragma unroll
    for (int a = 0; a < NP2; ++a) {
      double g[NV], n;  // n: not computed
      p2_shape<DIM, false, true>(a, lam, n, g);
      const int node = cell_n2[(size_t)a * n_cells + cell];
#pragma unroll
      for (int i = 0; i < DIM; ++i) {
        const double U = sol[(size_t)node * DIM + i];
#pragma unroll
        for (int q = 0; q < DIM; ++q) H[i][q] += U * (g[q + 1] - g[0]);
      }
    }
    const double vol = geo[(size_t)(DIM * DIM) * n_cells + cell] * REF_VOL;
#pragma unroll
    for (int j = 0; j < DIM; ++j)
      push_forward_col<DIM>(n_cells, cell, geo, H, j, [&](int i, double s) { num[i][j] += vol * s; });
    den += vol;
  }
  double G[DIM][DIM];
#pragma unroll
  for (int i = 0; i < DIM; ++i)
#pragma unroll
    for (int j = 0; j < DIM; ++j) G[i][j] = den > 0.0 ? num[i][j] / den : 0.0;
  // S = (G + G^T) / 2, W = (G - G^T) / 2: |S|^2 = sum_i G_ii^2 + 2 sum_{i<j} S_ij^2.  Q = (|W|^2 - |S|^2) / 2 is evaluated in the algebraically
  // equal form -(sum_ij G_ij G_ji) / 2: in a shear layer |W|^2 and |S|^2 are both about |G|^2 / 2 and their difference would carry the
  // rounding of terms of that size into a Q that is orders of magnitude smaller; the products G_ij G_ji are the terms Q is made of.
  double ss = 0.0, q = 0.0, div = 0.0;
#pragma unroll
  for (int i = 0; i < DIM; ++i) {
    ss += G[i][i] * G[i][i];
    q -= 0.5 * (G[i][i] * G[i][i]);
    div += G[i][i];
#pragma unroll
    for (int j = i + 1; j < DIM; ++j) {
      const double s = 0.5 * (G[i][j] + G[j][i]);
      ss += 2.0 * s * s;
      q -= G[i][j] * G[j][i];
    }
  }
  double *o = out + slot;
  int p = 0;
#pragma unroll
  for (int i = 0; i < DIM; ++i)
#pragma unroll
    for (int j = 0; j < DIM; ++j) o[(size_t)(p++) * n_slots] = G[i][j];
  if constexpr (DIM == 3) {
    o[(size_t)(p++) * n_slots] = G[2][1] - G[1][2];
    o[(size_t)(p++) * n_slots] = G[0][2] - G[2][0];
  }
  o[(size_t)(p++) * n_slots] = G[1][0] - G[0][1];
  o[(size_t)(p++) * n_slots] = q;
  o[(size_t)(p++) * n_slots] = sqrt(2.0 * ss);
  o[(size_t)(p++) * n_slots] = div;
}

// ------------------------------------------------------------------ host drivers
// the patch table of the current mesh, from the connectivity in the CALLER's node and cell numbering: it outlives a new layout / rank table
static void ensure_patches(nsx_handle *h) {
  if (h->nodal.have_patches) return;
  if (h->cell_n2_in.size() != (size_t)h->n_cells * h->np2) NSX_THROW(NSX_ERR_ARG, "nsx_compute_nodal_fields: the handle holds no connectivity");
  NodalPatches t;
  if (build_nodal_patches(h->n_cells, h->np2, h->cell_n2_in.data(), h->N2, t) != 0 || t.n_tiles != cdiv(h->N2, NODAL_TILE))
    NSX_THROW(NSX_ERR_ARG, "nsx_compute_nodal_fields: the node patch table could not be built (%d cells, %d nodes)", h->n_cells, h->N2);
  for (int32_t e : t.ent)
    if (e < -1 || (e >> NODAL_LOCAL_BITS) >= h->n_cells || (e >= 0 && (e & ((1 << NODAL_LOCAL_BITS) - 1)) >= h->np2))
      NSX_THROW(NSX_ERR_ARG, "nsx_compute_nodal_fields: the node patch table names entry %d", e);
  h->nodal.tile_ptr.upload(t.tile_ptr, h->stream);
  h->nodal.ent.upload(t.ent, h->stream);
  h->nodal.out.alloc((size_t)nodal_planes(h->dim) * t.n_tiles * NODAL_TILE);
  h->nodal.slot_of = std::move(t.slot_of);
  h->nodal.tiles = t.n_tiles;
  h->nodal.entries = (int64_t)t.ent.size();
  h->nodal.have_patches = true;
}

template <int DIM, int NP2>
static void launch_nodal(nsx_handle *h) {
  const double n_slots = (double)h->nodal.tiles * NODAL_TILE;
  const double bytes = 8.0 * DIM * h->N2_loc + (double)h->n_cells * (4.0 * NP2 + 8.0 * (DIM * DIM + 1)) + 4.0 * (double)h->nodal.entries +
                       4.0 * (h->nodal.tiles + 1) + 8.0 * nodal_planes(DIM) * n_slots;
  LaunchScope ls(h, "nodal_fields", bytes);
  hipLaunchKernelGGL((k_nodal_fields<DIM, NP2>), dim3(h->nodal.tiles), dim3(64), 0, h->stream, h->nodal.tile_ptr.p, h->nodal.ent.p, h->n_cells, h->cell_n2.p,
                     h->geo.p, h->sol.p, h->nodal.out.p);
}

static void compute_nodal_fields(nsx_handle *h) {
  post_check_space(h, "nsx_compute_nodal_fields");
  if (!h->sol.p || h->sol.n < (size_t)h->len_blk) NSX_THROW(NSX_ERR_ARG, "nsx_compute_nodal_fields: the handle holds no state yet");
  HIP_CHECK(hipSetDevice(h->prm.device));
  ensure_patches(h);
  h->nodal.valid = false;  // a failure below leaves no results
  if (h->nodal.tiles > 0) {
    if (h->dim == 2) launch_nodal<2, 6>(h);
    else launch_nodal<3, 10>(h);
    HIP_CHECK(hipGetLastError());
  }
  HIP_CHECK(hipStreamSynchronize(h->stream));
  h->nodal.valid = true;
}

static void nodal_check_get(nsx_handle *h, const char *who, int which) {
  post_check_space(h, who);
  if (!h->nodal.have_patches || !h->nodal.valid) NSX_THROW(NSX_ERR_ARG, "%s: nsx_compute_nodal_fields first", who);
  if (which < 0 || which >= NSX_FIELD_COUNT) NSX_THROW(NSX_ERR_ARG, "%s: field %d (NSX_FIELD_GRADIENT ... NSX_FIELD_DIVERGENCE)", who, which);
}

static void get_nodal_field(nsx_handle *h, int which, double *values) {
  nodal_check_get(h, "nsx_get_nodal_field", which);
  if (!values) NSX_THROW(NSX_ERR_ARG, "nsx_get_nodal_field: null values");
  HIP_CHECK(hipSetDevice(h->prm.device));
  const int nc = nodal_components(h->dim, which);
  const size_t n_slots = (size_t)h->nodal.tiles * NODAL_TILE;
  std::vector<double> v((size_t)nc * n_slots);
  if (!v.empty()) HIP_CHECK(hipMemcpyAsync(v.data(), h->nodal.out.p + (size_t)nodal_first_plane(h->dim, which) * n_slots, v.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIP_CHECK(hipStreamSynchronize(h->stream));
  for (int i = 0; i < h->N2; ++i) {  // caller-local node i = global node goff_u + i
    const size_t s = (size_t)h->nodal.slot_of[i];
    for (int k = 0; k < nc; ++k) values[((size_t)h->goff_u + i) * nc + k] = v[(size_t)k * n_slots + s];
  }
}

}  // namespace nsx

extern "C" {

int nsx_compute_nodal_fields(nsx_handle *h) {
  NSX_TRY(h)
  nsx::compute_nodal_fields(h);
  NSX_CATCH(h)
}

int nsx_nodal_field_components(nsx_handle *h, int which, int *n_components) {
  NSX_TRY(h)
  nsx::nodal_check_get(h, "nsx_nodal_field_components", which);
  if (!n_components) NSX_THROW(NSX_ERR_ARG, "nsx_nodal_field_components: null n_components");
  *n_components = nsx::nodal_components(h->dim, which);
  NSX_CATCH(h)
}

int nsx_get_nodal_field(nsx_handle *h, int which, double *values) {
  NSX_TRY(h)
  nsx::get_nodal_field(h, which, values);
  NSX_CATCH(h)
}

}  // extern "C"
