// nodal_patch.hpp — node -> (cell, local node) patch table of a P2 mesh, from the cell -> node connectivity alone.  Used by the device
// library's nodal fields (csrc/nsx_nodal.hip: the recovered gradient of a node is a volume-weighted mean over the cells that hold it).
//   patch of node n   every (cell, a) with cell_nodes[cell][a] == n, IN ASCENDING CELL ORDER: a counting sort over the cells in their
//                     order, no hashing, so the lists (and with them the order of every sum folded over them) depend on the connectivity only
// Patch sizes are very uneven (about 24 cells round an interior vertex of a structured tetrahedral mesh, 4 - 6 round an edge, 1 on a
// corner), and the kernel gives one lane to a node.  So the nodes are dealt to the lanes BY DESCENDING PATCH SIZE (stable: equal sizes in
// ascending node order): slot s = tile * 64 + lane holds node `order[s]`, the 64 lanes of a tile walk lists of (nearly) one length, and the
// lists of a tile are stored step-major, ent[(tile_ptr[t] + k) * 64 + lane] = entry k of the lane's list, so that every step is one
// coalesced load.  Lists shorter than their tile's longest are padded with -1; so are the slots behind the last node.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace nsx {

constexpr int NODAL_TILE = 64;       // slots per tile = lanes of a wave
constexpr int NODAL_LOCAL_BITS = 4;  // entry = cell << 4 | local node (n_p2 <= 16)

struct NodalPatches {
  int32_t n_nodes = 0, n_tiles = 0, max_size = 0;
  int64_t n_pairs = 0;            // (cell, local node) pairs of the owned nodes = entries that are not padding
  std::vector<int32_t> size;      // [n_nodes] patch size of every node
  std::vector<int32_t> order;     // [n_tiles * 64] slot -> node, -1: no node
  std::vector<int32_t> slot_of;   // [n_nodes] node -> slot
  std::vector<int32_t> tile_ptr;  // [n_tiles + 1] first step of every tile (units of 64 entries)
  std::vector<int32_t> ent;       // [tile_ptr[n_tiles] * 64] cell << 4 | local node, -1: padding
};

// cell_nodes[n_cells][np2] holds node ids; ids in [0, n_nodes) get a patch, larger ones (the ghosts of a distributed handle) are skipped.
// Returns 0, or -1 for arguments that cannot be tabulated (np2 > 16, a negative id, more cells than 2^27 - 1, more steps than an int32 holds).
inline int build_nodal_patches(int32_t n_cells, int np2, const int32_t *cell_nodes, int32_t n_nodes, NodalPatches &out) {
  out = NodalPatches();
  if (n_cells < 0 || n_nodes < 0 || np2 < 1 || np2 > (1 << NODAL_LOCAL_BITS) || (n_cells > 0 && !cell_nodes)) return -1;
  if (n_cells >= (1 << (31 - NODAL_LOCAL_BITS))) return -1;
  std::vector<int32_t> &size = out.size;
  size.assign((size_t)n_nodes, 0);
  for (size_t i = 0; i < (size_t)n_cells * np2; ++i) {
    if (cell_nodes[i] < 0) return -1;
    if (cell_nodes[i] < n_nodes) ++size[cell_nodes[i]];
  }
  std::vector<int64_t> ptr((size_t)n_nodes + 1, 0);
  for (int32_t n = 0; n < n_nodes; ++n) {
    ptr[(size_t)n + 1] = ptr[n] + size[n];
    out.max_size = std::max(out.max_size, size[n]);
  }
  out.n_pairs = ptr[n_nodes];
  std::vector<int32_t> list((size_t)out.n_pairs);  // node-major lists, ascending cell inside each: the cells are visited in their order
  {
    std::vector<int64_t> fill(ptr.begin(), ptr.end() - 1);
    for (int32_t c = 0; c < n_cells; ++c)
      for (int a = 0; a < np2; ++a) {
        const int32_t n = cell_nodes[(size_t)c * np2 + a];
        if (n < n_nodes) list[(size_t)fill[n]++] = (int32_t)(((uint32_t)c << NODAL_LOCAL_BITS) | (uint32_t)a);
      }
  }
  // slots: descending size, ascending node inside one size (counting sort by size)
  std::vector<int64_t> first((size_t)out.max_size + 2, 0);
  for (int32_t n = 0; n < n_nodes; ++n) ++first[(size_t)(out.max_size - size[n]) + 1];
  for (size_t s = 1; s < first.size(); ++s) first[s] += first[s - 1];
  out.n_tiles = (int32_t)(((int64_t)n_nodes + NODAL_TILE - 1) / NODAL_TILE);
  out.order.assign((size_t)out.n_tiles * NODAL_TILE, -1);
  out.slot_of.assign((size_t)n_nodes, -1);
  for (int32_t n = 0; n < n_nodes; ++n) {
    const int64_t s = first[(size_t)(out.max_size - size[n])]++;
    out.order[(size_t)s] = n;
    out.slot_of[n] = (int32_t)s;
  }
  out.tile_ptr.assign((size_t)out.n_tiles + 1, 0);
  int64_t steps = 0;
  for (int32_t t = 0; t < out.n_tiles; ++t) {
    steps += size[out.order[(size_t)t * NODAL_TILE]];  // the first slot of a tile holds its longest list
    if (steps * NODAL_TILE > INT32_MAX) return -1;
    out.tile_ptr[(size_t)t + 1] = (int32_t)steps;
  }
  out.ent.assign((size_t)steps * NODAL_TILE, -1);
  for (int32_t t = 0; t < out.n_tiles; ++t)
    for (int l = 0; l < NODAL_TILE; ++l) {
      const int32_t n = out.order[(size_t)t * NODAL_TILE + l];
      if (n < 0) continue;
      for (int32_t k = 0; k < size[n]; ++k) out.ent[((size_t)out.tile_ptr[t] + k) * NODAL_TILE + l] = list[(size_t)ptr[n] + k];
    }
  return 0;
}

}  // namespace nsx
