// gather_map.hpp — the deterministic gather map of one matrix block: for every CSR entry the cell-buffer offsets that sum into it, in
// ascending cell order (the summation order of the reference's cell loop).  Host only, no device types; nsx_setup.hip uploads the lists.
#pragma once
#include <cstdint>
#include <vector>

#include "graph.hpp"

namespace nsx {

enum GatherStatus { GATHER_OK = 0, GATHER_PAIR_NOT_IN_GRAPH, GATHER_OFFSET_OVERFLOW };

struct GatherLists {
  GatherStatus status = GATHER_OK;  // anything else: ptr and src are not to be used
  std::vector<int32_t> ptr, src;    // entry e sums src[ptr[e] .. ptr[e+1])
};

// contributions of every cell-local pair (a,b) to CSR entry (cell_r[a], cell_c[b]); src = plane * plane_stride * n_cells + cell with
// plane = a * per_c + b, or b * per_r + a when plane_rc_swapped.  Rows >= g.n_rows are ghost rows: assembled by their owner.
inline GatherLists build_gather_map(const Csr &g, int n_cells, int per_r, const int32_t *cell_r, int per_c, const int32_t *cell_c, int plane_stride,
                                    bool plane_rc_swapped) {
  const int64_t nnz = g.nnz();
  GatherLists gm;
  gm.ptr.assign((size_t)nnz + 1, 0);
  std::vector<int32_t> epos((size_t)n_cells * per_r * per_c);
  for (int c = 0; c < n_cells; ++c)
    for (int a = 0; a < per_r; ++a)
      for (int b = 0; b < per_c; ++b) {
        int32_t &e = epos[((size_t)c * per_r + a) * per_c + b];
        const int32_t row = cell_r[(size_t)c * per_r + a];
        if (row >= g.n_rows) {
          e = -1;
          continue;
        }
        e = find_in_row(g, row, cell_c[(size_t)c * per_c + b]);
        if (e < 0) {
          gm.status = GATHER_PAIR_NOT_IN_GRAPH;
          return gm;
        }
        gm.ptr[e + 1]++;
      }
  for (int64_t e = 0; e < nnz; ++e) gm.ptr[e + 1] += gm.ptr[e];
  gm.src.resize(gm.ptr[nnz]);
  std::vector<int32_t> fill(gm.ptr.begin(), gm.ptr.end() - 1);
  for (int c = 0; c < n_cells; ++c)
    for (int a = 0; a < per_r; ++a)
      for (int b = 0; b < per_c; ++b) {
        const int32_t e = epos[((size_t)c * per_r + a) * per_c + b];
        if (e < 0) continue;
        const int64_t plane = plane_rc_swapped ? ((int64_t)b * per_r + a) : ((int64_t)a * per_c + b);
        const int64_t off = plane * plane_stride * n_cells + c;
        if (off > INT32_MAX) {
          gm.status = GATHER_OFFSET_OVERFLOW;
          return gm;
        }
        gm.src[fill[e]++] = (int32_t)off;
      }
  return gm;
}

}  // namespace nsx
