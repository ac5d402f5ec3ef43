// adjacency.hpp — face-neighbour table of a simplicial mesh, from the cell -> vertex connectivity alone.  Used by the device library's
// tracer particles (csrc/nsx_tracer.hip: a particle that leaves its cell through the face opposite local vertex k steps to nbr[k][cell]).
//   nbr[k][cell]   the cell across the face opposite local vertex k of `cell`, -1 on the boundary; SoA, in the caller's cell order
// The faces are matched by SORTING their keys (the face's vertex ids in ascending order, then the cell): the result does not depend on any
// hash order, and a face with more than two cells shows up as a run longer than two.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace nsx {

struct FaceKey {
  int32_t v[3];  // vertex ids of the face, ascending (v[2] = -1 in 2D)
  int32_t cell, k;
  bool same_face(const FaceKey &o) const { return v[0] == o.v[0] && v[1] == o.v[1] && v[2] == o.v[2]; }
  bool operator<(const FaceKey &o) const {
    for (int i = 0; i < 3; ++i)
      if (v[i] != o.v[i]) return v[i] < o.v[i];
    return cell != o.cell ? cell < o.cell : k < o.k;
  }
};

// cell_vert[n_cells][nv], nv = 3 (triangles) or 4 (tetrahedra).  Returns 0 and fills nbr [nv][n_cells]; returns 1 + c, c the lowest cell
// of the offending face, when a face belongs to more than two cells or twice to one cell (a cell with a repeated vertex): nbr is then
// left empty.  Anything else (nv, a negative id) returns -1.
inline int64_t build_face_neighbours(int32_t n_cells, int nv, const int32_t *cell_vert, std::vector<int32_t> &nbr) {
  nbr.clear();
  if (n_cells < 0 || (nv != 3 && nv != 4) || (n_cells > 0 && !cell_vert)) return -1;
  std::vector<FaceKey> keys((size_t)n_cells * nv);
  for (int32_t c = 0; c < n_cells; ++c)
    for (int k = 0; k < nv; ++k) {
      FaceKey &f = keys[(size_t)c * nv + k];
      f.v[2] = -1;
      int m = 0;
      for (int a = 0; a < nv; ++a)
        if (a != k) {
          if (cell_vert[(size_t)c * nv + a] < 0) return -1;
          f.v[m++] = cell_vert[(size_t)c * nv + a];
        }
      std::sort(f.v, f.v + m);
      f.cell = c;
      f.k = k;
    }
  std::sort(keys.begin(), keys.end());
  std::vector<int32_t> out((size_t)n_cells * nv, -1);
  for (size_t i = 0; i < keys.size();) {
    size_t j = i + 1;
    while (j < keys.size() && keys[j].same_face(keys[i])) ++j;
    if (j - i > 2 || (j - i == 2 && keys[i].cell == keys[i + 1].cell)) return 1 + (int64_t)keys[i].cell;
    if (j - i == 2) {
      out[(size_t)keys[i].k * n_cells + keys[i].cell] = keys[i + 1].cell;
      out[(size_t)keys[i + 1].k * n_cells + keys[i + 1].cell] = keys[i].cell;
    }
    i = j;
  }
  nbr = std::move(out);
  return 0;
}

}  // namespace nsx
