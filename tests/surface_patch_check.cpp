// surface_patch_check.cpp — stand-alone driver of host/surface_patch.hpp for tests/test_surface_patch.py (built there with
// -fsanitize=address,undefined).  Input file: "n_faces npf n_groups", then per face "group node_0 ... node_{npf-1}".
// Output: "ok n_nodes n_tiles max_size" or "bad", then one line each: order, group_ptr, node_id, node_group, face_nodes, size, slot_of,
// tile_ptr, ent, and per level of the fold its block table.
#include <cstdio>
#include <vector>

#include "../navierstokes_project_nm4pde_amd/host/surface_patch.hpp"

template <class V>
static void line(const V &v) {
  for (auto x : v) printf("%lld ", (long long)x);
  printf("\n");
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  FILE *f = fopen(argv[1], "r");
  if (!f) return 2;
  int n_faces, npf, n_groups;
  if (fscanf(f, "%d %d %d", &n_faces, &npf, &n_groups) != 3 || n_faces < 0 || npf < 0 || npf > 64) return 2;
  std::vector<int64_t> node_of((size_t)n_faces * npf);
  std::vector<int32_t> groups((size_t)n_faces);
  for (int i = 0; i < n_faces; ++i) {
    if (fscanf(f, "%d", &groups[i]) != 1) return 2;
    for (int j = 0; j < npf; ++j) {
      long long v;
      if (fscanf(f, "%lld", &v) != 1) return 2;
      node_of[(size_t)i * npf + j] = v;
    }
  }
  fclose(f);
  nsx::SurfacePatches t;
  if (nsx::build_surface_patches(n_faces, npf, node_of.data(), groups.data(), n_groups, t) != 0) {
    printf("bad\n");
    return 0;
  }
  printf("ok %d %d %d\n", t.n_nodes, t.n_tiles, t.max_size);
  line(t.order);
  line(t.group_ptr);
  line(t.node_id);
  line(t.node_group);
  line(t.face_nodes);
  line(t.size);
  line(t.slot_of);
  line(t.tile_ptr);
  line(t.ent);
  const auto fold = nsx::build_surface_fold(t.group_ptr, 64);
  printf("%d\n", (int)fold.size());
  for (const auto &lvl : fold) line(lvl);
  return 0;
}
