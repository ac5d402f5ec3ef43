// lattice_box.hpp — the lattice of nsx_set_lattice (include/nsx.h, section "lattice sampling"; csrc/nsx_lattice.hip): the coordinate of a
// lattice point and the index box of a cell, i.e. the lattice points the rasterisation of k_lattice_locate visits for the cell.  Compiled
// by the kernels, by the host and by tests/lattice_box_check.cpp.
//
// Coordinate: x_d = origin_d + (double)i_d * spacing_d with ONE rounded multiply and ONE rounded add, never a fused multiply-add, so that
// numpy's origin + i * spacing gives the same bits.
//
// Box.  A point the containment test accepts for a cell is x = sum_k lambda_k X_k with sum_k lambda_k = 1 and lambda_k >= -tol.  Write
// lambda_k = mu_k - tol: mu_k >= 0, sum_k mu_k = 1 + (dim + 1) tol, and on axis d
//     x_d = sum_k mu_k X_k,d - tol sum_k X_k,d <= (1 + (dim + 1) tol) max_d - tol sum_k X_k,d = max_d + tol sum_k (max_d - X_k,d).
// One vertex attains the maximum and every other one is at most ext_d = max_d - min_d below it, so x_d <= max_d + dim tol ext_d, and in
// the same way x_d >= min_d - tol sum_k (X_k,d - min_d) >= min_d - dim tol ext_d.  The box takes the sums themselves (they are attained,
// at the vertices of the dilated simplex; dim ext_d is up to dim times as much for a cell that is thin on the axis).
// The box is the floor / ceil of these bounds in lattice units, widened by one index on each
// side -- for the rounding of the bound, of the division, of the coordinate formula and of the lambda the kernel works out in double
// precision (all far below one index while neighbouring lattice coordinates are distinct doubles, which nsx_set_lattice requires) -- and
// clamped to [0, counts_d - 1].  A box that clamps to empty on any axis is empty.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define NSX_LATTICE_HD __host__ __device__
#else
#define NSX_LATTICE_HD
#endif

namespace nsx {

NSX_LATTICE_HD inline double lattice_coord(double origin, double spacing, int32_t i) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __dadd_rn(origin, __dmul_rn((double)i, spacing));
#else
  volatile double m = (double)i * spacing;  // the product is rounded before the sum sees it
  return origin + m;
#endif
}

// Indices [lo, hi] on one axis for accepted points with xmin <= x_d <= xmax: floor / ceil in lattice units, one index more on each side,
// clamped to [0, count - 1]; false (and lo > hi): no lattice point.
NSX_LATTICE_HD inline bool lattice_axis_range(double xmin, double xmax, double origin, double spacing, int32_t count, int32_t &lo, int32_t &hi) {
  double a = floor((xmin - origin) / spacing) - 1.0;
  double b = ceil((xmax - origin) / spacing) + 1.0;
  const double last = (double)(count - 1);
  lo = 0;
  hi = -1;
  if (a > last || b < 0.0) return false;
  if (!(a > 0.0)) a = 0.0;    // a bound that is not a number keeps the whole axis
  if (!(b < last)) b = last;
  lo = (int32_t)a;
  hi = (int32_t)b;
  return lo <= hi;
}

// The index box of the cell with vertices X[dim + 1][dim]; false: empty (then lo > hi on every axis).
template <int DIM>
NSX_LATTICE_HD inline bool lattice_box(const double (&X)[DIM + 1][DIM], double tol, const double *origin, const double *spacing, const int32_t *counts,
                                       int32_t (&lo)[DIM], int32_t (&hi)[DIM]) {
  bool any = true;
  for (int d = 0; d < DIM; ++d) {
    double vmin = X[0][d], vmax = X[0][d];
    for (int v = 1; v <= DIM; ++v) {
      vmin = X[v][d] < vmin ? X[v][d] : vmin;
      vmax = X[v][d] > vmax ? X[v][d] : vmax;
    }
    double below = 0.0, above = 0.0;  // sum_k (X_k,d - min_d), sum_k (max_d - X_k,d): differences first, so the error scales with the cell
    for (int v = 0; v <= DIM; ++v) {
      below += X[v][d] - vmin;
      above += vmax - X[v][d];
    }
    any = lattice_axis_range(vmin - tol * below, vmax + tol * above, origin[d], spacing[d], counts[d], lo[d], hi[d]) && any;
  }
  if (!any)
    for (int d = 0; d < DIM; ++d) {
      lo[d] = 0;
      hi[d] = -1;
    }
  return any;
}

}  // namespace nsx
