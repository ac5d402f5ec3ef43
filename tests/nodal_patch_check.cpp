// Stand-alone driver of host/nodal_patch.hpp for tests/test_nodal_patch.py (built there with -fsanitize=address,undefined):
//   nodal_patch_check FILE      FILE: "n_cells np2 n_nodes" followed by n_cells * np2 node ids
// prints "ok n_tiles max_size n_pairs" and four lines -- size [n_nodes], order [n_tiles * 64], tile_ptr [n_tiles + 1], ent [steps * 64] --
// or "bad".
#include <cstdio>
#include <vector>

#include "../navierstokes_project_nm4pde_amd/host/nodal_patch.hpp"

static void line(const std::vector<int32_t> &v) {
  for (int32_t x : v) std::printf("%d ", x);
  std::printf("\n");
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = std::fopen(argv[1], "r");
  if (!f) return 2;
  int n_cells = 0, np2 = 0, n_nodes = 0;
  if (std::fscanf(f, "%d %d %d", &n_cells, &np2, &n_nodes) != 3 || n_cells < 0 || np2 < 1 || np2 > 64) return 2;
  std::vector<int32_t> cells((size_t)n_cells * np2);
  for (auto &v : cells)
    if (std::fscanf(f, "%d", &v) != 1) return 2;
  std::fclose(f);
  nsx::NodalPatches t;
  if (nsx::build_nodal_patches(n_cells, np2, cells.data(), n_nodes, t) != 0) {
    std::printf("bad\n");
    return 0;
  }
  if (t.order.size() != (size_t)t.n_tiles * nsx::NODAL_TILE || t.tile_ptr.size() != (size_t)t.n_tiles + 1 || t.slot_of.size() != (size_t)n_nodes ||
      t.ent.size() != (size_t)t.tile_ptr.back() * nsx::NODAL_TILE)
    return 3;
  for (int n = 0; n < n_nodes; ++n)
    if (t.slot_of[n] < 0 || t.order[t.slot_of[n]] != n) return 3;
  std::printf("ok %d %d %lld\n", t.n_tiles, t.max_size, (long long)t.n_pairs);
  line(t.size);
  line(t.order);
  line(t.tile_ptr);
  line(t.ent);
  return 0;
}
