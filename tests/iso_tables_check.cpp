// Stand-alone driver of tests/test_iso_tables.py: prints the tables of host/iso_tables.hpp, one line each.
//   sub2 / sub3   the local nodes of every sub-simplex
//   tri  m n a-b ...   case m of a sub-triangle: n segments, then their crossings (inside vertex a, outside vertex b)
//   tet  m n a-b ...   case m of a sub-tetrahedron: n triangles, then their crossings
#include <cstdio>

#include "../navierstokes_project_nm4pde_amd/host/iso_tables.hpp"

int main() {
  using namespace nsx;
  printf("max %d %d\n", ISO_MAX_PRIMS_2D, ISO_MAX_PRIMS_3D);
  for (int s = 0; s < ISO_SUB2; ++s) printf("sub2 %d %d %d\n", ISO_SUB_TRI[s][0], ISO_SUB_TRI[s][1], ISO_SUB_TRI[s][2]);
  for (int s = 0; s < ISO_SUB3; ++s) printf("sub3 %d %d %d %d\n", ISO_SUB_TET[s][0], ISO_SUB_TET[s][1], ISO_SUB_TET[s][2], ISO_SUB_TET[s][3]);
  for (int m = 0; m < 8; ++m) {
    printf("tri %d %d", m, ISO_TRI_N[m]);
    for (int k = 0; k < 2 * ISO_TRI_N[m]; ++k) printf(" %d-%d", ISO_TRI_V[m][k] >> 2, ISO_TRI_V[m][k] & 3);
    printf("\n");
  }
  for (int m = 0; m < 16; ++m) {
    printf("tet %d %d", m, ISO_TET_N[m]);
    for (int k = 0; k < 3 * ISO_TET_N[m]; ++k) printf(" %d-%d", ISO_TET_V[m][k] >> 2, ISO_TET_V[m][k] & 3);
    printf("\n");
  }
  return 0;
}
