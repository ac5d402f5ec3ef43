// surface_patch.hpp — surface-node table and node -> (face, face node) patch lists of a set of boundary faces in groups, from the P2 node of
// every face node alone.  Used by the device library's surface loads (csrc/nsx_surface.hip: the value at a surface node is an area-weighted
// mean over the faces of its group that hold it).  No HIP in here: tests/surface_patch_check.cpp builds it on its own.
//   sorted faces      the faces stable-sorted by group: order[p] = caller's face at sorted position p, group g at [group_ptr[g], group_ptr[g+1])
//   surface node      a distinct (group, P2 node) pair among the face nodes, numbered by ascending group, then ascending node id: a node on
//                     the seam of two groups is two surface nodes
//   patch of s        every (sorted position p, face node j) with face_nodes[order[p]][j] == s, IN ASCENDING p -- inside one group that is
//                     the ascending position in the caller's face list, the order every sum over the patch is folded in
// As in nodal_patch.hpp the surface nodes are dealt to the lanes by DESCENDING patch size (stable: equal sizes in ascending surface node):
// slot = tile * 64 + lane, the lists of a tile stored step-major, ent[(tile_ptr[t] + k) * 64 + lane] = entry k of the lane's list, padded
// with -1 to the tile's longest.
#pragma once
#include <algorithm>
#include <cstdint>
#include <utility>
#include <vector>

namespace nsx {

constexpr int SURFACE_TILE = 64;       // slots per tile = lanes of a wave
constexpr int SURFACE_LOCAL_BITS = 3;  // entry = sorted face position << 3 | face node (at most 6 nodes per face)
constexpr int SURFACE_MAX_GROUPS = 64;

struct SurfacePatches {
  int32_t n_faces = 0, npf = 0, n_groups = 0, n_nodes = 0, n_tiles = 0, max_size = 0;
  std::vector<int32_t> order;       // [n_faces] sorted position -> caller's face
  std::vector<int32_t> group_ptr;   // [n_groups + 1] sorted positions of every group
  std::vector<int64_t> node_id;     // [n_nodes] P2 node of every surface node
  std::vector<int32_t> node_group;  // [n_nodes]
  std::vector<int32_t> face_nodes;  // [n_faces][npf] caller's face, face node -> surface node
  std::vector<int32_t> size;        // [n_nodes] patch size
  std::vector<int32_t> slot_of;     // [n_nodes] surface node -> slot
  std::vector<int32_t> tile_ptr;    // [n_tiles + 1] first step of every tile (units of 64 entries)
  std::vector<int32_t> ent;         // [tile_ptr[n_tiles] * 64] sorted position << 3 | face node, -1: padding
};

// node_of[n_faces][npf]: the P2 node of every face node (any non-negative id that names a node uniquely); groups[n_faces] (nullptr: all 0).
// Returns 0, or -1 for arguments that cannot be tabulated (npf outside 1..6, n_groups outside 1..64, a group out of range, a negative id,
// 2^28 faces or more, more steps than an int32 holds).
inline int build_surface_patches(int32_t n_faces, int npf, const int64_t *node_of, const int32_t *groups, int n_groups, SurfacePatches &out) {
  out = SurfacePatches();
  if (n_faces < 0 || npf < 1 || npf > 6 || n_groups < 1 || n_groups > SURFACE_MAX_GROUPS || (n_faces > 0 && !node_of)) return -1;
  if (n_faces >= (1 << (31 - SURFACE_LOCAL_BITS))) return -1;
  out.n_faces = n_faces;
  out.npf = npf;
  out.n_groups = n_groups;
  out.group_ptr.assign((size_t)n_groups + 1, 0);
  for (int32_t f = 0; f < n_faces; ++f) {
    const int32_t g = groups ? groups[f] : 0;
    if (g < 0 || g >= n_groups) return -1;
    ++out.group_ptr[(size_t)g + 1];
  }
  for (int g = 0; g < n_groups; ++g) out.group_ptr[(size_t)g + 1] += out.group_ptr[g];
  out.order.assign((size_t)n_faces, 0);
  {  // counting sort by group: stable
    std::vector<int32_t> fill(out.group_ptr.begin(), out.group_ptr.end() - 1);
    for (int32_t f = 0; f < n_faces; ++f) out.order[(size_t)fill[groups ? groups[f] : 0]++] = f;
  }
  // the surface nodes: the distinct (group, node) pairs in ascending order
  std::vector<std::pair<int32_t, int64_t>> keys((size_t)n_faces * npf);
  for (int32_t f = 0; f < n_faces; ++f)
    for (int j = 0; j < npf; ++j) {
      const int64_t id = node_of[(size_t)f * npf + j];
      if (id < 0) return -1;
      keys[(size_t)f * npf + j] = {groups ? groups[f] : 0, id};
    }
  std::vector<std::pair<int32_t, int64_t>> uniq(keys);
  std::sort(uniq.begin(), uniq.end());
  uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
  out.n_nodes = (int32_t)uniq.size();
  out.node_id.resize(uniq.size());
  out.node_group.resize(uniq.size());
  for (size_t s = 0; s < uniq.size(); ++s) {
    out.node_group[s] = uniq[s].first;
    out.node_id[s] = uniq[s].second;
  }
  out.face_nodes.resize(keys.size());
  std::vector<int32_t> &size = out.size;
  size.assign((size_t)out.n_nodes, 0);
  for (size_t i = 0; i < keys.size(); ++i) {
    const int32_t s = (int32_t)(std::lower_bound(uniq.begin(), uniq.end(), keys[i]) - uniq.begin());
    out.face_nodes[i] = s;
    ++size[s];
  }
  std::vector<int64_t> ptr((size_t)out.n_nodes + 1, 0);
  for (int32_t s = 0; s < out.n_nodes; ++s) {
    ptr[(size_t)s + 1] = ptr[s] + size[s];
    out.max_size = std::max(out.max_size, size[s]);
  }
  std::vector<int32_t> list((size_t)ptr[out.n_nodes]);  // node-major lists, ascending sorted position inside each
  {
    std::vector<int64_t> fill(ptr.begin(), ptr.end() - 1);
    for (int32_t p = 0; p < n_faces; ++p)
      for (int j = 0; j < npf; ++j) {
        const int32_t s = out.face_nodes[(size_t)out.order[p] * npf + j];
        list[(size_t)fill[s]++] = (int32_t)(((uint32_t)p << SURFACE_LOCAL_BITS) | (uint32_t)j);
      }
  }
  // slots: descending size, ascending surface node inside one size (counting sort by size)
  std::vector<int64_t> first((size_t)out.max_size + 2, 0);
  for (int32_t s = 0; s < out.n_nodes; ++s) ++first[(size_t)(out.max_size - size[s]) + 1];
  for (size_t k = 1; k < first.size(); ++k) first[k] += first[k - 1];
  out.n_tiles = (int32_t)(((int64_t)out.n_nodes + SURFACE_TILE - 1) / SURFACE_TILE);
  std::vector<int32_t> node_at((size_t)out.n_tiles * SURFACE_TILE, -1);
  out.slot_of.assign((size_t)out.n_nodes, -1);
  for (int32_t s = 0; s < out.n_nodes; ++s) {
    const int64_t slot = first[(size_t)(out.max_size - size[s])]++;
    node_at[(size_t)slot] = s;
    out.slot_of[s] = (int32_t)slot;
  }
  out.tile_ptr.assign((size_t)out.n_tiles + 1, 0);
  int64_t steps = 0;
  for (int32_t t = 0; t < out.n_tiles; ++t) {
    steps += size[node_at[(size_t)t * SURFACE_TILE]];  // the first slot of a tile holds its longest list
    if (steps * SURFACE_TILE > INT32_MAX) return -1;
    out.tile_ptr[(size_t)t + 1] = (int32_t)steps;
  }
  out.ent.assign((size_t)steps * SURFACE_TILE, -1);
  for (int32_t t = 0; t < out.n_tiles; ++t)
    for (int l = 0; l < SURFACE_TILE; ++l) {
      const int32_t s = node_at[(size_t)t * SURFACE_TILE + l];
      if (s < 0) continue;
      for (int32_t k = 0; k < size[s]; ++k) out.ent[((size_t)out.tile_ptr[t] + k) * SURFACE_TILE + l] = list[(size_t)ptr[s] + k];
    }
  return 0;
}

// The level sizes of the segmented fold of the totals: every group's entries are folded in blocks of `width` consecutive entries, level by
// level, until every group holds one entry (a group without a face holds one entry from the first level on: an empty block, which is 0).
// Entry l of the result lists for level l, per block, {first input entry, one past the last, group}; the outputs of a level are its blocks in order.
// The shape depends on the face counts alone.
inline std::vector<std::vector<int32_t>> build_surface_fold(const std::vector<int32_t> &group_ptr, int width) {
  std::vector<std::vector<int32_t>> out;  // [levels][3 * n_blocks]
  std::vector<int32_t> ptr(group_ptr);
  const size_t ng = ptr.size() - 1;
  for (;;) {
    std::vector<int32_t> lvl, next(ng + 1, 0);
    for (size_t g = 0; g < ng; ++g) {
      const int32_t a = ptr[g], b = ptr[g + 1];
      const int32_t nb = std::max(1, (b - a + width - 1) / width);
      for (int32_t k = 0; k < nb; ++k) {
        lvl.push_back(a + k * width);
        lvl.push_back(std::min(b, a + (k + 1) * width));
        lvl.push_back((int32_t)g);
      }
      next[g + 1] = next[g] + nb;
    }
    out.push_back(std::move(lvl));
    ptr = next;
    if ((size_t)ptr[ng] == ng) return out;
  }
}

}  // namespace nsx
