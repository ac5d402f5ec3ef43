// Stand-alone driver of host/adjacency.hpp for tests/test_adjacency.py (built there with -fsanitize=address,undefined):
//   adjacency_check FILE      FILE: "n_cells nv" followed by n_cells * nv vertex ids
// prints "ok" and the table nbr[k][cell] (nv rows of n_cells entries), or "refused C" (C: the cell build_face_neighbours names), or "bad".
#include <cstdio>
#include <vector>

#include "../navierstokes_project_nm4pde_amd/host/adjacency.hpp"

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = std::fopen(argv[1], "r");
  if (!f) return 2;
  int n_cells = 0, nv = 0;
  if (std::fscanf(f, "%d %d", &n_cells, &nv) != 2 || n_cells < 0 || nv < 1 || nv > 8) return 2;
  std::vector<int32_t> cells((size_t)n_cells * nv);
  for (auto &v : cells)
    if (std::fscanf(f, "%d", &v) != 1) return 2;
  std::fclose(f);
  std::vector<int32_t> nbr;
  const int64_t rc = nsx::build_face_neighbours(n_cells, nv, cells.data(), nbr);
  if (rc > 0) {
    std::printf("refused %lld\n", (long long)(rc - 1));
    return nbr.empty() ? 0 : 3;
  }
  if (rc < 0) {
    std::printf("bad\n");
    return nbr.empty() ? 0 : 3;
  }
  if (nbr.size() != (size_t)n_cells * nv) return 3;
  std::printf("ok\n");
  for (int k = 0; k < nv; ++k) {
    for (int c = 0; c < n_cells; ++c) std::printf("%d ", nbr[(size_t)k * n_cells + c]);
    std::printf("\n");
  }
  return 0;
}
