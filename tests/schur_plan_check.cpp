// Stand-alone driver of the Schur product's planner (host/schur_plan.hpp) for tests/test_schur_plan.py (built there with
// -fsanitize=address,undefined):
//   schur_plan_check COMMAND FILE      FILE: whitespace-separated integers, a graph being "rowptr [n_rows + 1], colind [nnz]"
//   plan     s_rows s_cols b_rows b_cols max_words (0: no limit), graph of S, graph of B
//            -> "ok max_row entries matches slots", then a line each for row_grp, grp_off, words; or "refused max_row"
//   replay   s_rows s_cols b_rows b_cols dim seed, graph of S, graph of B
//            -> values of B and weights from the seed (every fifth weight node 0.0: masked terms), S once by the merge of k_schur and once
//               from the plan, both through ONE term function: "same entries exact_zeros" if they agree bit for bit, else "differ entry"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../navierstokes_project_nm4pde_amd/host/schur_plan.hpp"

static FILE *in;

static int num() {
  int v = 0;
  if (std::fscanf(in, "%d", &v) != 1) std::exit(2);
  return v;
}
static nsx::Csr graph(int n_rows, int n_cols) {
  nsx::Csr g;
  g.n_rows = n_rows;
  g.n_cols = n_cols;
  g.rowptr.resize((size_t)n_rows + 1);
  for (auto &x : g.rowptr) x = num();
  g.colind.resize((size_t)g.rowptr.back());
  for (auto &x : g.colind) x = num();
  return g;
}
template <class T>
static void line(const std::vector<T> &v) {
  for (T x : v) std::printf("%lld ", (long long)x);
  std::printf("\n");
}

static void plan() {
  const int s_rows = num(), s_cols = num(), b_rows = num(), b_cols = num(), max_words = num();
  const nsx::Csr S = graph(s_rows, s_cols), B = graph(b_rows, b_cols);
  const nsx::SchurPlan pl = max_words > 0 ? nsx::build_schur_plan(S, B, max_words) : nsx::build_schur_plan(S, B);
  if (!pl.ok) {
    std::printf("refused %d\n", pl.max_row);
    return;
  }
  std::printf("ok %d %lld %lld %lld\n", pl.max_row, (long long)pl.entries, (long long)pl.matches, (long long)pl.slots());
  line(pl.row_grp);
  line(pl.grp_off);
  line(pl.words);
}

// the statement of k_schur / k_schur_planned (csrc/nsx_sparse.hip), one function for both replays
static double term(double acc, const double *rv, const double *bv, int dim) {
  for (int c = 0; c < dim; ++c) acc += rv[c] * bv[c];
  return acc;
}

static void replay() {
  const int s_rows = num(), s_cols = num(), b_rows = num(), b_cols = num(), dim = num();
  unsigned long long state = (unsigned long long)num() * 2654435761ull + 12345;
  auto uniform = [&]() {  // in (-1, 1)
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(long long)(state >> 11) / (double)(1ll << 52) - 1.0;
  };
  const nsx::Csr S = graph(s_rows, s_cols), B = graph(b_rows, b_cols);
  std::vector<double> bv((size_t)B.nnz() * dim), w((size_t)b_cols * dim);
  for (auto &x : bv) x = uniform();
  for (int k = 0; k < b_cols; ++k)
    for (int c = 0; c < dim; ++c) w[(size_t)k * dim + c] = k % 5 == 0 ? 0.0 : 1.0 + 0.5 * uniform();
  const nsx::SchurPlan pl = nsx::build_schur_plan(S, B);
  if (!pl.ok) std::exit(3);
  std::vector<double> merged((size_t)S.nnz()), planned((size_t)S.nnz(), -1.0), rv;
  long long zeros = 0;
  for (int i = 0; i < s_rows; ++i) {
    const int b0 = B.rowptr[i], nb = B.rowptr[i + 1] - b0;
    rv.assign((size_t)nb * dim + 1, 0.0);
    for (int t = 0; t < nb; ++t)
      for (int c = 0; c < dim; ++c) rv[(size_t)t * dim + c] = bv[(size_t)(b0 + t) * dim + c] * w[(size_t)B.colind[b0 + t] * dim + c];
    for (int e = S.rowptr[i]; e < S.rowptr[i + 1]; ++e) {  // the merge: row j's entries in order, a cursor into row i
      const int j = S.colind[e];
      double acc = 0.0;
      int q = 0;
      for (int p = B.rowptr[j]; p < B.rowptr[j + 1]; ++p) {
        const int k = B.colind[p];
        while (q < nb && B.colind[b0 + q] < k) ++q;
        if (q < nb && B.colind[b0 + q] == k) acc = term(acc, &rv[(size_t)q * dim], &bv[(size_t)p * dim], dim);
      }
      merged[e] = acc;
    }
    for (int g = pl.row_grp[i]; g < pl.row_grp[i + 1]; ++g)  // the plan: group by group, lane by lane, step by step
      for (int lane = 0; lane < 64; ++lane) {
        const int e = S.rowptr[i] + 64 * (g - pl.row_grp[i]) + lane;
        double acc = 0.0;
        for (long long o = pl.grp_off[g] + lane; o < pl.grp_off[g + 1]; o += 64) {
          const uint32_t word = pl.words[(size_t)o];
          if (word == nsx::SCHUR_NO_TERM) continue;
          if (e >= S.rowptr[i + 1]) std::exit(4);  // a term on a lane without an entry
          acc = term(acc, &rv[(size_t)(word >> 16) * dim], &bv[((size_t)B.rowptr[S.colind[e]] + (word & 0xffffu)) * dim], dim);
        }
        if (e < S.rowptr[i + 1]) planned[e] = acc;
      }
  }
  for (long long e = 0; e < S.nnz(); ++e) {
    if (std::memcmp(&merged[e], &planned[e], sizeof(double)) != 0) {
      std::printf("differ %lld\n", e);
      return;
    }
    zeros += merged[e] == 0.0;
  }
  std::printf("same %lld %lld\n", (long long)S.nnz(), zeros);
}

int main(int argc, char **argv) {
  if (argc != 3 || !(in = std::fopen(argv[2], "r"))) return 2;
  int rc = 2;
  if (!std::strcmp(argv[1], "plan")) {
    plan();
    rc = 0;
  } else if (!std::strcmp(argv[1], "replay")) {
    replay();
    rc = 0;
  }
  std::fclose(in);
  return rc;
}
