// Stand-alone driver of the set-up planners (host/ilu_levels.hpp, host/spmv_plan.hpp, host/gather_map.hpp and the structural product of
// host/graph.hpp) for tests/test_setup_plan.py (built there with -fsanitize=address,undefined):
//   setup_plan_check COMMAND FILE      FILE: whitespace-separated integers, a graph being "rowptr [n_rows + 1], colind [nnz]"
//   levels   n_rows n_blocks, graph, block_ptr [n_blocks + 1]
//            -> "ok max_rows max_levels in_block_nnz max_block_nnz", then a line each for: forward lvl_ptr, rows, blk_off; backward lvl_ptr,
//               rows, blk_off; in_lo, in_hi, in_cptr, in_cpos, fac_order; merged forward ptr, rows, rec; merged backward ptr, rows, rec
//   bounds   n_rows target by_rank_allowed n_rank_ptr, rank_ptr -> "ok", the chunk bounds
//   chunks   n_rows n_own largest_first n_bounds, graph, bounds
//            -> "ok n_chunks max_ucols max_rows grid grid_if n_chunks_if frac_if", then cptr, ucols, lidx, desc, order, desc_if; or "toomany"
//   gather   n_rows n_cells per_r per_c plane_stride plane_rc_swapped, graph, cell_r [n_cells * per_r], cell_c [n_cells * per_c]
//            -> "ok", then ptr, src; or "missing" / "overflow"
//   schur    b_rows b_cols n_rows n_cols, graph of B -> "ok", then rowptr, colind
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../navierstokes_project_nm4pde_amd/host/gather_map.hpp"
#include "../navierstokes_project_nm4pde_amd/host/ilu_levels.hpp"
#include "../navierstokes_project_nm4pde_amd/host/spmv_plan.hpp"

static FILE *in;

static int num() {
  int v = 0;
  if (std::fscanf(in, "%d", &v) != 1) std::exit(2);
  return v;
}
static std::vector<int32_t> nums(size_t n) {
  std::vector<int32_t> v(n);
  for (auto &x : v) x = num();
  return v;
}
static nsx::Csr graph(int n_rows, int n_cols) {
  nsx::Csr g;
  g.n_rows = n_rows;
  g.n_cols = n_cols;
  g.rowptr = nums((size_t)n_rows + 1);
  g.colind = nums((size_t)g.rowptr.back());
  return g;
}
template <class T>
static void line(const std::vector<T> &v) {
  for (T x : v) std::printf("%d ", (int)x);
  std::printf("\n");
}

static void levels() {
  const int n = num(), nb = num();
  const nsx::Csr g = graph(n, n);
  const std::vector<int32_t> bptr = nums((size_t)nb + 1);
  const nsx::IluLevels lv = nsx::build_ilu_levels(g, bptr);
  std::printf("ok %d %d %lld %d\n", lv.max_rows, lv.max_levels, (long long)lv.in_block_nnz, lv.max_block_nnz);
  for (const nsx::LevelLists *s : {&lv.fwd, &lv.bwd}) {
    line(s->lvl_ptr);
    line(s->rows);
    line(s->blk_off);
  }
  line(lv.in_lo);
  line(lv.in_hi);
  line(lv.in_cptr);
  line(lv.in_cpos);
  line(lv.fac_order);
  for (int backward = 0; backward < 2; ++backward) {
    const nsx::MergedLevels m = nsx::merge_levels(g, lv, backward == 1);
    line(m.ptr);
    line(m.rows);
    line(m.rec);
  }
}

static void bounds() {
  const int n = num(), target = num(), allowed = num(), nrk = num();
  const std::vector<int32_t> rk = nums(nrk);
  std::printf("ok\n");
  line(nsx::chunk_bounds(n, rk, target, allowed != 0));
}

static void chunks() {
  const int n = num(), n_own = num(), largest_first = num(), n_bounds = num();
  const nsx::Csr g = graph(n, 0);
  const std::vector<int32_t> bd = nums(n_bounds);
  const nsx::ChunkTable t = nsx::build_chunk_table(g, bd, n_own, largest_first != 0);
  if (!t.ok) {
    std::printf("toomany\n");
    return;
  }
  std::printf("ok %d %d %d %d %d %d %.17g\n", t.n_chunks, t.max_ucols, t.max_rows, t.grid, t.grid_if, t.n_chunks_if, t.frac_if);
  line(t.cptr);
  line(t.ucols);
  line(t.lidx);
  line(t.desc);
  line(t.order);
  line(t.desc_if);
}

static void gather() {
  const int n = num(), n_cells = num(), per_r = num(), per_c = num(), stride = num(), swapped = num();
  const nsx::Csr g = graph(n, 0);
  const std::vector<int32_t> cr = nums((size_t)n_cells * per_r), cc = nums((size_t)n_cells * per_c);
  const nsx::GatherLists l = nsx::build_gather_map(g, n_cells, per_r, cr.data(), per_c, cc.data(), stride, swapped != 0);
  if (l.status != nsx::GATHER_OK) {
    std::printf(l.status == nsx::GATHER_PAIR_NOT_IN_GRAPH ? "missing\n" : "overflow\n");
    return;
  }
  std::printf("ok\n");
  line(l.ptr);
  line(l.src);
}

static void schur() {
  const int b_rows = num(), b_cols = num(), n_rows = num(), n_cols = num();
  const nsx::Csr B = graph(b_rows, b_cols);
  const nsx::Csr S = nsx::structural_product(B, n_rows, n_cols);
  if (S.n_rows != n_rows || S.n_cols != n_cols) std::exit(3);
  std::printf("ok\n");
  line(S.rowptr);
  line(S.colind);
}

int main(int argc, char **argv) {
  if (argc != 3 || !(in = std::fopen(argv[2], "r"))) return 2;
  const struct {
    const char *name;
    void (*run)();
  } commands[] = {{"levels", levels}, {"bounds", bounds}, {"chunks", chunks}, {"gather", gather}, {"schur", schur}};
  for (const auto &c : commands)
    if (!std::strcmp(argv[1], c.name)) {
      c.run();
      std::fclose(in);
      return 0;
    }
  return 2;
}
