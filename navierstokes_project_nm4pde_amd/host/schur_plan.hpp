// schur_plan.hpp -- which terms enter every entry of S = B diag(w) B^T, planned once per Schur graph (plain C++, no HIP).
//
// S_ij sums over the columns that rows i and j of B share.  The patterns of S and B are fixed after the first assembly, so the list of
// terms of every entry, and their order, is a constant of the mesh: the numeric kernel (k_schur_planned, csrc/nsx_sparse.hip) reads it
// instead of merging the two rows again in every step.
//
// Layout.  The entries of row i of S are taken 64 at a time (a "group": the lanes of the one wave that computes the row).  A group owns
// a slab [step t][lane] of 32-bit words; word t of lane e is the t-th shared column of row j = S.colind[e] IN ROW j'S ASCENDING ORDER --
// the order in which the merge of k_schur adds the terms -- packed as
//     (position q of the column in row i) << 16  |  (position of the column in row j, counted from the row's start)
// and SCHUR_NO_TERM (all ones) where the lane has no t-th term or no entry.  A group has as many steps as its longest lane.  Both
// positions must stay below 65535, so a graph with a row of B of 65535 entries or more is not planned (ok = false): the merge kernel runs.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "graph.hpp"

namespace nsx {

constexpr uint32_t SCHUR_NO_TERM = 0xffffffffu;
constexpr int32_t SCHUR_PLAN_MAX_ROW = 65535;  // rows of B of this length or longer are not planned

struct SchurPlan {
  bool ok = false;
  int32_t max_row = 0;            // longest row of B (set whether or not the graph is planned)
  std::vector<int32_t> row_grp;   // [S.n_rows + 1] first group of every row
  std::vector<int64_t> grp_off;   // [groups + 1] first word of every group's slab (multiples of 64)
  std::vector<uint32_t> words;
  int64_t entries = 0, matches = 0;  // entries of S, terms over all of them
  int64_t slots() const { return (int64_t)words.size(); }
  double fill() const { return words.empty() ? 0.0 : (double)matches / (double)words.size(); }
  int64_t bytes() const { return 4 * (int64_t)words.size() + 8 * (int64_t)grp_off.size() + 4 * (int64_t)row_grp.size(); }
};

// S: the Schur graph (rows [0, S.n_rows) of B against the rows [0, S.n_cols) of B), B: the graph of block(1,0), columns sorted.
// max_words: a plan that would take more words than this is given up (ok = false).
inline SchurPlan build_schur_plan(const Csr &S, const Csr &B, int64_t max_words = (int64_t)1 << 62) {
  SchurPlan pl;
  for (int32_t j = 0; j < B.n_rows; ++j) pl.max_row = std::max(pl.max_row, B.rowptr[j + 1] - B.rowptr[j]);
  if (pl.max_row >= SCHUR_PLAN_MAX_ROW) return pl;
  // B^T with, beside every row j that holds column k, the position of k in row j: walking row i's columns in ascending order then
  // meets the shared columns of every row j in ascending order too, which is row j's own order
  int32_t n_cols = B.n_cols;
  for (int32_t k : B.colind) n_cols = std::max(n_cols, k + 1);
  std::vector<int64_t> tptr((size_t)n_cols + 1, 0);
  for (int32_t k : B.colind) tptr[(size_t)k + 1]++;
  for (int32_t k = 0; k < n_cols; ++k) tptr[(size_t)k + 1] += tptr[k];
  std::vector<int32_t> trow(B.colind.size());
  std::vector<uint16_t> toff(B.colind.size());
  {
    std::vector<int64_t> fill(tptr.begin(), tptr.end() - 1);
    for (int32_t j = 0; j < B.n_rows; ++j)
      for (int32_t p = B.rowptr[j]; p < B.rowptr[j + 1]; ++p) {
        const int64_t at = fill[B.colind[p]]++;
        trow[at] = j;
        toff[at] = (uint16_t)(p - B.rowptr[j]);
      }
  }
  pl.entries = S.nnz();
  pl.row_grp.assign((size_t)S.n_rows + 1, 0);
  for (int32_t i = 0; i < S.n_rows; ++i) pl.row_grp[(size_t)i + 1] = pl.row_grp[i] + (S.rowptr[i + 1] - S.rowptr[i] + 63) / 64;
  std::vector<int32_t> local((size_t)std::max(S.n_cols, B.n_rows), -1);  // column j of S -> its entry in the current row
  // f(entry of row i, position q in row i, place t in B^T) for every term of row i, the terms of an entry in ascending column order
  auto terms_of_row = [&](int32_t i, auto &&f) {
    const int32_t e0 = S.rowptr[i], ne = S.rowptr[i + 1] - e0;
    const int32_t b0 = i < B.n_rows ? B.rowptr[i] : 0, nb = i < B.n_rows ? B.rowptr[i + 1] - b0 : 0;
    for (int32_t e = 0; e < ne; ++e) local[S.colind[e0 + e]] = e;
    for (int32_t q = 0; q < nb; ++q) {
      const int32_t k = B.colind[b0 + q];
      for (int64_t t = tptr[k]; t < tptr[(size_t)k + 1]; ++t)
        if (local[trow[t]] >= 0) f(local[trow[t]], q, t);
    }
    for (int32_t e = 0; e < ne; ++e) local[S.colind[e0 + e]] = -1;
  };
  // first pass: the terms of every entry, so that the slabs are allocated once (they are mostly "no term": 0.7 GB at 1 M DoF)
  std::vector<int32_t> count;
  pl.grp_off.assign((size_t)pl.row_grp.back() + 1, 0);
  for (int32_t i = 0; i < S.n_rows; ++i) {
    const int32_t ne = S.rowptr[i + 1] - S.rowptr[i];
    count.assign(ne, 0);
    terms_of_row(i, [&](int32_t e, int32_t, int64_t) { count[e]++; });
    for (int32_t e = 0; e < ne; ++e) {
      int64_t &steps = pl.grp_off[(size_t)pl.row_grp[i] + e / 64 + 1];
      steps = std::max<int64_t>(steps, count[e]);
    }
  }
  for (size_t g = 1; g < pl.grp_off.size(); ++g) pl.grp_off[g] = pl.grp_off[g - 1] + 64 * pl.grp_off[g];
  if (pl.grp_off.back() > max_words) {
    pl.row_grp.clear();
    pl.grp_off.clear();
    return pl;
  }
  pl.words.assign((size_t)pl.grp_off.back(), SCHUR_NO_TERM);
  for (int32_t i = 0; i < S.n_rows; ++i) {
    count.assign(S.rowptr[i + 1] - S.rowptr[i], 0);  // terms placed so far
    terms_of_row(i, [&](int32_t e, int32_t q, int64_t t) {
      pl.words[(size_t)(pl.grp_off[(size_t)pl.row_grp[i] + e / 64] + 64 * (int64_t)count[e]++ + e % 64)] = (uint32_t)q << 16 | toff[t];
      pl.matches++;
    });
  }
  pl.ok = true;
  return pl;
}

}  // namespace nsx
