// graph.hpp — small CSR graph helpers shared by the host front-end and the device library's
// host-side setup.  Builds "row entity -> column entity" couplings induced by a cell loop, i.e.
// what DoFTools::make_sparsity_pattern does for one pair of scalar spaces
// (reference Navier-Stokes/src/NavierStokes3D.cpp:109-124).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace nsx {

struct Csr {
  int32_t n_rows = 0, n_cols = 0;
  std::vector<int32_t> rowptr;  // n_rows + 1
  std::vector<int32_t> colind;  // sorted ascending inside a row
  int64_t nnz() const { return rowptr.empty() ? 0 : rowptr.back(); }
};

// entity -> cells incidence (CSR), cells listed in ascending order.
inline void build_incidence(int32_t n_cells, int32_t per_cell, const int32_t *cell_ent, int32_t n_ent,
                            std::vector<int32_t> &ptr, std::vector<int32_t> &cells) {
  ptr.assign(n_ent + 1, 0);
  for (int64_t k = 0; k < (int64_t)n_cells * per_cell; ++k) ptr[cell_ent[k] + 1]++;
  for (int32_t i = 0; i < n_ent; ++i) ptr[i + 1] += ptr[i];
  cells.resize(ptr[n_ent]);
  std::vector<int32_t> fill(ptr.begin(), ptr.end() - 1);
  for (int32_t c = 0; c < n_cells; ++c)
    for (int32_t a = 0; a < per_cell; ++a) cells[fill[cell_ent[(int64_t)c * per_cell + a]]++] = c;
}

// rows = entities of kind R (per_r per cell), cols = entities of kind C (per_c per cell).
inline Csr build_graph(int32_t n_cells, int32_t per_r, const int32_t *cell_r, int32_t n_r, int32_t per_c,
                       const int32_t *cell_c, int32_t n_c) {
  std::vector<int32_t> ptr, cells;
  build_incidence(n_cells, per_r, cell_r, n_r, ptr, cells);
  Csr g;
  g.n_rows = n_r;
  g.n_cols = n_c;
  g.rowptr.assign(n_r + 1, 0);
  std::vector<int32_t> tmp;
  // pass 1: count
  for (int32_t i = 0; i < n_r; ++i) {
    tmp.clear();
    for (int32_t k = ptr[i]; k < ptr[i + 1]; ++k) {
      const int32_t *cc = cell_c + (int64_t)cells[k] * per_c;
      tmp.insert(tmp.end(), cc, cc + per_c);
    }
    std::sort(tmp.begin(), tmp.end());
    g.rowptr[i + 1] = (int32_t)(std::unique(tmp.begin(), tmp.end()) - tmp.begin());
  }
  for (int32_t i = 0; i < n_r; ++i) g.rowptr[i + 1] += g.rowptr[i];
  g.colind.resize(g.rowptr[n_r]);
  for (int32_t i = 0; i < n_r; ++i) {
    tmp.clear();
    for (int32_t k = ptr[i]; k < ptr[i + 1]; ++k) {
      const int32_t *cc = cell_c + (int64_t)cells[k] * per_c;
      tmp.insert(tmp.end(), cc, cc + per_c);
    }
    std::sort(tmp.begin(), tmp.end());
    auto e = std::unique(tmp.begin(), tmp.end());
    std::copy(tmp.begin(), e, g.colind.begin() + g.rowptr[i]);
  }
  return g;
}

// position of column j in row i (binary search); -1 if absent.
inline int32_t find_in_row(const Csr &g, int32_t i, int32_t j) {
  const int32_t *b = g.colind.data() + g.rowptr[i], *e = g.colind.data() + g.rowptr[i + 1];
  const int32_t *p = std::lower_bound(b, e, j);
  return (p != e && *p == j) ? (int32_t)(p - g.colind.data()) : -1;
}

// pattern of B^T: row k (a column of B, n_cols of them) lists the rows of B that hold k, ascending
inline Csr transpose_pattern(const Csr &B, int32_t n_cols) {
  Csr t;
  t.n_rows = n_cols;
  t.n_cols = B.n_rows;
  t.rowptr.assign((size_t)n_cols + 1, 0);
  t.colind.resize(B.nnz());
  for (int64_t k = 0; k < B.nnz(); ++k) t.rowptr[B.colind[k] + 1]++;
  for (int32_t i = 0; i < n_cols; ++i) t.rowptr[i + 1] += t.rowptr[i];
  std::vector<int32_t> fill(t.rowptr.begin(), t.rowptr.end() - 1);
  for (int32_t j = 0; j < B.n_rows; ++j)
    for (int32_t k = B.rowptr[j]; k < B.rowptr[j + 1]; ++k) t.colind[fill[B.colind[k]]++] = j;
  return t;
}

// Pattern of B * B^T (EpetraExt::MatrixMatrix::Multiply, structural): rows [0, n_rows) of B against all its n_cols >= n_rows rows,
// columns sorted.  B may hold more rows than the product (ghost rows behind the owned ones).
inline Csr structural_product(const Csr &B, int32_t n_rows, int32_t n_cols) {
  const Csr t = transpose_pattern(B, B.n_cols);
  Csr S;
  S.n_rows = n_rows;
  S.n_cols = n_cols;
  S.rowptr.assign((size_t)n_rows + 1, 0);
  std::vector<int32_t> mark(n_cols, -1), cols;
  for (int32_t i = 0; i < n_rows; ++i) {
    cols.clear();
    for (int32_t kb = B.rowptr[i]; kb < B.rowptr[i + 1]; ++kb)
      for (int32_t q = t.rowptr[B.colind[kb]]; q < t.rowptr[B.colind[kb] + 1]; ++q) {
        const int32_t j = t.colind[q];
        if (mark[j] != i) {
          mark[j] = i;
          cols.push_back(j);
        }
      }
    std::sort(cols.begin(), cols.end());
    S.colind.insert(S.colind.end(), cols.begin(), cols.end());
    S.rowptr[i + 1] = (int32_t)S.colind.size();
  }
  return S;
}

}  // namespace nsx
