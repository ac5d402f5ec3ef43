// ilu_levels.hpp — the level schedule of a block-Jacobi ILU(0) on a square graph (Ifpack overlap-0 semantics): per
// block the rows sorted by dependency level, for the forward (L) and the backward (U) sweep, the in-block entry range and compact
// numbering of every row, the dispatch order of the factorisation, and -- for blocks too large for one workgroup -- the levels of all
// blocks merged.  Host only, no device types; nsx_setup.hip uploads what these functions return.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "graph.hpp"

namespace nsx {

// The levels of one sweep direction, the blocks one after the other: block b has the levels [blk_off[b], blk_off[b+1]), level l the
// rows rows[lvl_ptr[l] .. lvl_ptr[l+1]), ascending.
struct LevelLists {
  std::vector<int32_t> lvl_ptr{0}, rows, blk_off;
};

struct IluLevels {
  LevelLists fwd, bwd;
  int max_rows = 0, max_levels = 0;         // over the blocks (levels: over both directions)
  std::vector<int32_t> in_lo, in_hi;        // [n_rows] CSR positions bounding the in-block entries of a row (sorted columns: one range)
  std::vector<int32_t> in_cptr, in_cpos;    // running count of in-block entries; compact number -> CSR position
  std::vector<int32_t> fac_order;           // blocks by descending in-block entries, ties in block order
  int32_t max_block_nnz = 0;
  int64_t in_block_nnz = 0;
};

// level[i] = 1 + max level[j] over the in-block columns j in front of i (forward) or behind it (backward)
inline void sweep_levels(const Csr &g, const std::vector<int32_t> &block_ptr, const IluLevels &lv, bool backward, LevelLists &out, int &max_levels) {
  const int nb = (int)block_ptr.size() - 1, step = backward ? -1 : 1;
  std::vector<int32_t> lev(g.n_rows, 0);
  std::vector<std::vector<int32_t>> buckets;
  out.blk_off.assign((size_t)nb + 1, 0);
  out.rows.reserve(g.n_rows);
  for (int b = 0; b < nb; ++b) {
    const int r0 = block_ptr[b], r1 = block_ptr[b + 1];
    int nl = 0;
    for (int i = backward ? r1 - 1 : r0; i >= r0 && i < r1; i += step) {
      int l = 0;
      for (int p = backward ? lv.in_hi[i] - 1 : lv.in_lo[i]; p >= lv.in_lo[i] && p < lv.in_hi[i] && (g.colind[p] - i) * step < 0; p += step)
        l = std::max(l, lev[g.colind[p]] + 1);
      lev[i] = l;
      nl = std::max(nl, l + 1);
    }
    buckets.assign(nl, {});
    for (int i = r0; i < r1; ++i) buckets[lev[i]].push_back(i);
    for (int l = 0; l < nl; ++l) {
      out.rows.insert(out.rows.end(), buckets[l].begin(), buckets[l].end());
      out.lvl_ptr.push_back((int32_t)out.rows.size());
    }
    out.blk_off[b + 1] = (int32_t)out.lvl_ptr.size() - 1;
    max_levels = std::max(max_levels, nl);
  }
}

// block b = rows [block_ptr[b], block_ptr[b+1]); the blocks cover the rows of g
inline IluLevels build_ilu_levels(const Csr &g, const std::vector<int32_t> &block_ptr) {
  const int nb = (int)block_ptr.size() - 1;
  IluLevels lv;
  lv.in_lo.assign(g.n_rows, 0);
  lv.in_hi.assign(g.n_rows, 0);
  lv.in_cptr.assign((size_t)g.n_rows + 1, 0);
  for (int b = 0; b < nb; ++b) {
    const int r0 = block_ptr[b], r1 = block_ptr[b + 1];
    lv.max_rows = std::max(lv.max_rows, r1 - r0);
    for (int i = r0; i < r1; ++i) {
      const int32_t *cb = g.colind.data() + g.rowptr[i], *ce = g.colind.data() + g.rowptr[i + 1];
      lv.in_lo[i] = (int32_t)(std::lower_bound(cb, ce, r0) - g.colind.data());
      lv.in_hi[i] = (int32_t)(std::lower_bound(cb, ce, r1) - g.colind.data());
      lv.in_cptr[i + 1] = lv.in_cptr[i] + (lv.in_hi[i] - lv.in_lo[i]);
    }
    lv.max_block_nnz = std::max(lv.max_block_nnz, lv.in_cptr[r1] - lv.in_cptr[r0]);
  }
  lv.in_block_nnz = lv.in_cptr[g.n_rows];
  lv.in_cpos.resize((size_t)lv.in_cptr[g.n_rows]);
  for (int i = 0; i < g.n_rows; ++i)
    for (int p = lv.in_lo[i]; p < lv.in_hi[i]; ++p) lv.in_cpos[lv.in_cptr[i] + (p - lv.in_lo[i])] = p;
  auto block_nnz = [&](int b) { return lv.in_cptr[block_ptr[b + 1]] - lv.in_cptr[block_ptr[b]]; };
  lv.fac_order.resize(nb);
  for (int b = 0; b < nb; ++b) lv.fac_order[b] = b;
  std::stable_sort(lv.fac_order.begin(), lv.fac_order.end(), [&](int x, int y) { return block_nnz(x) > block_nnz(y); });
  sweep_levels(g, block_ptr, lv, false, lv.fwd, lv.max_levels);
  sweep_levels(g, block_ptr, lv, true, lv.bwd, lv.max_levels);
  return lv;
}

// The levelled path: blocks are independent, so level l of the whole schedule is the union, in block order, of the blocks' level-l
// rows.  One record per row in that order -- {row, first entry, end of entries, diagonal} of the sweep's triangle -- so that a level
// kernel learns everything about its row in ONE coalesced load.
struct MergedLevels {
  std::vector<int32_t> ptr, rows, rec;  // [max_levels + 1], [n_rows], [4 * n_rows]
};

inline MergedLevels merge_levels(const Csr &g, const IluLevels &lv, bool backward) {
  const LevelLists &s = backward ? lv.bwd : lv.fwd;
  const int nb = (int)s.blk_off.size() - 1;
  MergedLevels m;
  m.ptr.assign((size_t)lv.max_levels + 1, 0);
  m.rows.resize(s.rows.size());
  for (int b = 0; b < nb; ++b)
    for (int l = s.blk_off[b]; l < s.blk_off[b + 1]; ++l) m.ptr[l - s.blk_off[b] + 1] += s.lvl_ptr[l + 1] - s.lvl_ptr[l];
  for (int l = 0; l < lv.max_levels; ++l) m.ptr[l + 1] += m.ptr[l];
  std::vector<int32_t> fill(m.ptr.begin(), m.ptr.end() - 1);
  for (int b = 0; b < nb; ++b)
    for (int l = s.blk_off[b]; l < s.blk_off[b + 1]; ++l)
      for (int q = s.lvl_ptr[l]; q < s.lvl_ptr[l + 1]; ++q) m.rows[fill[l - s.blk_off[b]]++] = s.rows[q];
  m.rec.resize(4 * m.rows.size());
  for (size_t r = 0; r < m.rows.size(); ++r) {
    const int i = m.rows[r], d = find_in_row(g, i, i);
    m.rec[4 * r + 0] = i;
    m.rec[4 * r + 1] = backward ? d + 1 : lv.in_lo[i];
    m.rec[4 * r + 2] = backward ? lv.in_hi[i] : d;
    m.rec[4 * r + 3] = d;
  }
  return m;
}

}  // namespace nsx
