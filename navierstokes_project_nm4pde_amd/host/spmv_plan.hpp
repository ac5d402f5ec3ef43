// spmv_plan.hpp — the host side of the LDS-staged SpMV: where the chunks of rows begin and end, which columns every chunk stages and
// under which 16-bit local number, and the XCD-aware launch tables.  Host only, no device types; nsx_setup.hip uploads what these
// functions return.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "graph.hpp"

namespace nsx {

constexpr int SPMV_MAX_CHUNK_ROWS = 448;  // the kernel's row-pointer buffer
constexpr int SPMV_N_XCD = 8;

// Chunk boundaries.  With a rank table the chunks are unions of consecutive rank blocks: a rank's rows are the nodes of one
// subdomain, so a chunk that ends where a subdomain ends stages fewer columns than one that straddles three subdomains (6.3 instead
// of 5.5 non-zeros per staged entry at one ~85-row rank per chunk).  Small chunks win: two or three ranks per chunk stage even less
// (7.9) but measured slower (38 and 43 against 34 us: fewer, longer workgroups).  Without a rank table, or with ranks too large for
// a chunk: a fixed row count.
inline std::vector<int32_t> chunk_bounds(int n_rows, const std::vector<int32_t> &rank_ptr, int target, bool by_rank_allowed) {
  const int n = n_rows;
  const std::vector<int32_t> &rk = rank_ptr;
  std::vector<int32_t> bounds{0};
  const double rows_per_rank = rk.size() > 2 ? (double)n / (double)(rk.size() - 1) : 0.0;
  const bool by_rank = by_rank_allowed && rk.size() > 2 && rows_per_rank <= target;
  // ranks larger than a chunk (fewer, larger virtual ranks: --ranks 2048 has ~170 rows per block) are cut into equal parts of at most
  // `target` rows: a chunk still ends where a subdomain ends
  const bool split_ranks = !by_rank && by_rank_allowed && rk.size() > 2 && rows_per_rank <= 4.0 * target;
  if (by_rank) {
    int start = 0;
    for (size_t r = 1; r < rk.size(); ++r) {
      // close the chunk in front of a rank that would take it past the target (a single oversized rank is cut below)
      if (rk[r] - start > target && rk[r - 1] > start) {
        bounds.push_back(rk[r - 1]);
        start = rk[r - 1];
      }
    }
    bounds.push_back(n);
  } else if (split_ranks) {
    for (size_t r = 0; r + 1 < rk.size(); ++r) {
      const int rows = rk[r + 1] - rk[r];
      if (rows <= 0) continue;
      const int parts = (rows + target - 1) / target;
      for (int q = 1; q <= parts; ++q) bounds.push_back(rk[r] + (int)((int64_t)rows * q / parts));
    }
    if (bounds.back() != n) bounds.push_back(n);
  } else {
    for (int r = 128; r < n; r += 128) bounds.push_back(r);
    bounds.push_back(n);
  }
  std::vector<int32_t> out{0};
  for (size_t c = 1; c < bounds.size(); ++c) {
    while (bounds[c] - out.back() > SPMV_MAX_CHUNK_ROWS) out.push_back(out.back() + SPMV_MAX_CHUNK_ROWS / 2);
    if (bounds[c] > out.back()) out.push_back(bounds[c]);
  }
  return out;
}

// chunk c = rows [bounds[c], bounds[c+1]); it stages the columns ucols[cptr[c] .. cptr[c+1]) (ascending), and non-zero p of one of its
// rows reads staged entry lidx[p]
struct ChunkTable {
  bool ok = true;  // false: a chunk touches more than 65535 columns, no 16-bit local number for them; nothing else is filled in
  int n_chunks = 0, max_ucols = 0, max_rows = 0;
  std::vector<int32_t> cptr, ucols;
  std::vector<uint16_t> lidx;
  // launch tables ({first staged column, staged columns, first row, end row} per workgroup): `desc` for the chunks whose staged columns
  // are all owned, `desc_if` for those that stage a ghost column; order = chunk of every workgroup of `desc`, -1 = padding
  std::vector<int32_t> desc, order, desc_if;
  int grid = 0, grid_if = 0, n_chunks_if = 0;
  double frac_if = 0;  // share of the non-zeros in the chunks of desc_if
};

// Launch table of the chunks `chunks`: workgroup b runs on XCD b % 8, so workgroup 8 * j + k takes the j-th chunk of XCD k's range.
// XCD k takes the chunks [cut[k], cut[k+1]) of the list -- boundaries where the running non-zero count passes k / 8 of the total -- and,
// with largest_first, takes them by descending non-zeros (ties in list order).  {0, 0, 0, 0} pads.
inline void xcd_launch_table(const Csr &g, const std::vector<int32_t> &bounds, const std::vector<int32_t> &cptr, const std::vector<int32_t> &chunks,
                             bool largest_first, std::vector<int32_t> &desc, int &grid, std::vector<int32_t> *order) {
  const int nc = (int)chunks.size();
  auto cnnz = [&](int c) { return (int64_t)(g.rowptr[bounds[c + 1]] - g.rowptr[bounds[c]]); };
  int64_t total = 0;
  for (int c : chunks) total += cnnz(c);
  int cut[SPMV_N_XCD + 1];
  cut[0] = 0;
  int64_t run = 0;
  for (int k = 1, j = 0; k <= SPMV_N_XCD; ++k) {
    while (j < nc && (run + cnnz(chunks[j])) * SPMV_N_XCD <= total * k) run += cnnz(chunks[j++]);
    cut[k] = k == SPMV_N_XCD ? nc : j;
  }
  int per_xcd = 0;
  for (int k = 0; k < SPMV_N_XCD; ++k) per_xcd = std::max(per_xcd, cut[k + 1] - cut[k]);
  grid = SPMV_N_XCD * per_xcd;
  if (order) order->assign((size_t)grid, -1);
  desc.assign((size_t)grid * 4, 0);
  std::vector<int32_t> list;
  for (int k = 0; k < SPMV_N_XCD; ++k) {
    list.assign(chunks.begin() + cut[k], chunks.begin() + cut[k + 1]);
    if (largest_first) std::stable_sort(list.begin(), list.end(), [&](int32_t a, int32_t c) { return cnnz(a) > cnnz(c); });
    for (size_t j = 0; j < list.size(); ++j) {
      const int blk = (int)j * SPMV_N_XCD + k, c = list[j];
      if (order) (*order)[blk] = c;
      desc[4 * (size_t)blk + 0] = cptr[c];
      desc[4 * (size_t)blk + 1] = cptr[c + 1] - cptr[c];
      desc[4 * (size_t)blk + 2] = bounds[c];
      desc[4 * (size_t)blk + 3] = bounds[c + 1];
    }
  }
}

// n_own: columns below it are owned (one GPU: all of them).  The chunks whose staged columns are all owned go into the first launch
// table -- launched while the ghost exchange is in flight -- and the chunks that stage a ghost column into the second one, launched
// behind it (the Epetra_Import + local multiply of every vmult, Preconditioners.hpp:382,405).
inline ChunkTable build_chunk_table(const Csr &g, const std::vector<int32_t> &bounds, int n_own, bool largest_first) {
  ChunkTable t;
  t.n_chunks = (int)bounds.size() - 1;
  t.cptr.assign((size_t)t.n_chunks + 1, 0);
  t.lidx.resize(g.nnz());
  std::vector<int32_t> tmp;
  for (int c = 0; c < t.n_chunks; ++c) {
    const int r0 = bounds[c], r1 = bounds[c + 1];
    t.max_rows = std::max(t.max_rows, r1 - r0);
    tmp.assign(g.colind.begin() + g.rowptr[r0], g.colind.begin() + g.rowptr[r1]);
    std::sort(tmp.begin(), tmp.end());
    tmp.erase(std::unique(tmp.begin(), tmp.end()), tmp.end());
    if (tmp.size() > 65535) {
      t.ok = false;
      return t;
    }
    for (int p = g.rowptr[r0]; p < g.rowptr[r1]; ++p) t.lidx[p] = (uint16_t)(std::lower_bound(tmp.begin(), tmp.end(), g.colind[p]) - tmp.begin());
    t.ucols.insert(t.ucols.end(), tmp.begin(), tmp.end());
    t.cptr[c + 1] = (int32_t)t.ucols.size();
    t.max_ucols = std::max<int>(t.max_ucols, (int)tmp.size());
  }
  std::vector<int32_t> first, second;
  int64_t nnz_second = 0;
  for (int c = 0; c < t.n_chunks; ++c) {
    const bool ghost = t.cptr[c + 1] > t.cptr[c] && t.ucols[(size_t)t.cptr[c + 1] - 1] >= n_own;  // the list is sorted: its last entry is the largest column
    (ghost ? second : first).push_back(c);
    if (ghost) nnz_second += g.rowptr[bounds[c + 1]] - g.rowptr[bounds[c]];
  }
  xcd_launch_table(g, bounds, t.cptr, first, largest_first, t.desc, t.grid, &t.order);
  t.n_chunks_if = (int)second.size();
  t.frac_if = g.nnz() ? (double)nnz_second / (double)g.nnz() : 0.0;
  if (!second.empty()) xcd_launch_table(g, bounds, t.cptr, second, largest_first, t.desc_if, t.grid_if, nullptr);
  return t;
}

}  // namespace nsx
