// iso_tables.hpp — the tables of the marching sub-simplices behind nsx_extract_isosurface (include/nsx.h, section "isosurfaces and slices";
// csrc/nsx_iso.hip): how a P2 cell is cut into linear sub-simplices on its own nodes, and which crossings make the primitives of a
// sub-simplex.  Plain constexpr arrays, read by the kernels, by the host and by tests/iso_tables_check.cpp.
//
// Local P2 nodes: the vertices 0..dim, then the lines {0,1},{1,2},{2,0}[,{0,3},{1,3},{2,3}] (the front-end's order).
// Every sub-simplex below has the orientation of its cell (in reference coordinates its volume is +1/4 of the triangle's, +1/8 of the
// tetrahedron's), so one case table serves all of them.
//
// Case index: bit v is set when vertex v of the sub-simplex is inside (s >= isovalue).  A crossing is the byte 4 a + b: the edge from the
// INSIDE vertex a to the OUTSIDE vertex b of the sub-simplex; its point is x_a + t (x_b - x_a), t = (s_a - iso) / (s_a - s_b).  The vertex
// order is the one of a cell with det J > 0: the normal (p1 - p0) x (p2 - p0) points from inside to outside, in 2D the inside lies to
// the left of p0 -> p1.  A cell with det J < 0 swaps the last two vertices of every primitive.
#pragma once
#include <cstdint>

namespace nsx {

constexpr int ISO_SUB2 = 4, ISO_SUB3 = 8;  // sub-simplices per cell
constexpr int ISO_MAX_PRIMS_2D = 4, ISO_MAX_PRIMS_3D = 16;  // primitives per cell at most: 1 per sub-triangle, 2 per sub-tetrahedron

// the 4 sub-triangles: three corners, then the inner one
constexpr uint8_t ISO_SUB_TRI[ISO_SUB2][3] = {{0, 3, 5}, {3, 1, 4}, {5, 4, 2}, {3, 4, 5}};
// the 4 corner tetrahedra, then the inner octahedron split along its diagonal 4-9
constexpr uint8_t ISO_SUB_TET[ISO_SUB3][4] = {{0, 4, 6, 7}, {4, 1, 5, 8}, {6, 5, 2, 9}, {7, 8, 9, 3}, {4, 9, 5, 6}, {4, 9, 6, 7}, {4, 9, 7, 8}, {4, 9, 8, 5}};

// segments of a sub-triangle per case (0 or 1), and their 2 crossings
constexpr uint8_t ISO_TRI_N[8] = {0, 1, 1, 1, 1, 1, 1, 0};
constexpr uint8_t ISO_TRI_V[8][2] = {
    {0, 0},  // none inside
    {1, 2},  // {0}
    {6, 4},  // {1}
    {6, 2},  // {0,1}
    {8, 9},  // {2}
    {1, 9},  // {0,2}
    {8, 4},  // {1,2}
    {0, 0},  // all inside
};

// triangles of a sub-tetrahedron per case (0, 1 or 2), and their 3 crossings each.  Two inside {i < j}, two outside {k < l}: the quad
// (i,k) (i,l) (j,l) (j,k), split along its first and third corner.
constexpr uint8_t ISO_TET_N[16] = {0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0};
constexpr uint8_t ISO_TET_V[16][6] = {
    {0, 0, 0, 0, 0, 0},       // none inside
    {1, 2, 3, 0, 0, 0},       // {0}
    {4, 7, 6, 0, 0, 0},       // {1}
    {2, 3, 7, 2, 7, 6},       // {0,1}
    {8, 9, 11, 0, 0, 0},      // {2}
    {1, 11, 3, 1, 9, 11},     // {0,2}
    {4, 7, 11, 4, 11, 8},     // {1,2}
    {3, 7, 11, 0, 0, 0},      // {0,1,2}
    {12, 14, 13, 0, 0, 0},    // {3}
    {1, 2, 14, 1, 14, 13},    // {0,3}
    {4, 14, 6, 4, 12, 14},    // {1,3}
    {2, 14, 6, 0, 0, 0},      // {0,1,3}
    {8, 9, 13, 8, 13, 12},    // {2,3}
    {1, 9, 13, 0, 0, 0},      // {0,2,3}
    {4, 12, 8, 0, 0, 0},      // {1,2,3}
    {0, 0, 0, 0, 0, 0},       // all inside
};

}  // namespace nsx
