/*
 * vggsfm_amd -- a surface from the depth maps of a reconstruction: the maps integrated into a truncated signed distance
 * (TSDF) volume and the zero level set of that volume extracted as an indexed triangle mesh by marching tetrahedra on the
 * Kuhn (Freudenthal) split of each cell (libvggsfm_amd_tsdf.so, a library of its own: the entries of the other libraries
 * and the headers under include/ are closed, counted sets).
 *
 * Conventions of include/vggsfm_amd.h hold: device pointers, `stream` a hipStream_t as void*, asynchronous (no entry
 * synchronises with the host), no allocation, VGG_OK (0) or a negative VGG_ERR_* code.  The names carry the prefix vggv_;
 * their rows stand in vggsfm_amd/_lib_tsdf.py.  One argument is a HOST array: the `out` of vggv_case_table.
 *
 * Maps are row-major; a point (x, y) with integer coordinates is the centre of pixel [y][x].  depth (S, H, W) float32,
 * 0 = no depth.  poses (S, 3, 4) doubles [R|t], camera from world; cams (S, 4) doubles f, cx, cy, k (k = 0:
 * SIMPLE_PINHOLE, else SIMPLE_RADIAL).
 *
 * All arithmetic is float64 from the float32 inputs, without floating-point contraction; a + b + c means (a + b) + c.
 * Every sum is taken in a fixed order; no atomic decides a value or an order: two runs give the same bits.
 *
 * The grid: origin (ox, oy, oz), voxel h > 0, dims (nx, ny, nz), each >= 2.  Node (i, j, k) has the world position
 * X = (ox + h i, oy + h j, oz + h k) and the index n = (k ny + j) nx + i; N = nx ny nz nodes.  A grid with 7 N > 2^31 - 1
 * is refused (VGG_ERR_UNSUPPORTED), a grid with a dim < 0 or = 1 is refused (VGG_ERR_INVALID_ARGUMENT); a grid with a dim
 * = 0, and for vggv_integrate a frame of 0 pixels, is a no-op that returns VGG_OK (after the other refusals; nothing is
 * written).  Volumes: tsdf_sum (N), weight_sum (N) doubles, rgb_sum (N, 3) doubles or NULL.
 *
 * Shared with the stereo (one copy, csrc/mvs/mvs_geometry.hpp):
 *   transfer of P:              X[i] = R[i][0] P[0] + R[i][1] P[1] + R[i][2] P[2] + t[i];
 *   projection of X (X[2] > 0): iz = 1 / X[2], a = X[0] iz, b = X[1] iz, d = 1 + k (a a + b b),
 *                               x = f (a d) + cx, y = f (b d) + cy.
 */
#ifndef VGGSFM_AMD_TSDF_H
#define VGGSFM_AMD_TSDF_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VGGV_GROUP 256        /* nodes per group of the two-level count */
#define VGGV_MAX_VIEWS 256    /* views per launch of the integration */

const char* vggv_build_arch(void);

/* The 16-case table of the extraction as the kernel holds it: out is a HOST array (2, 16, 7) int32, [0] for tetrahedra with
 * sigma = +1 and [1] for sigma = -1; bit c of the case number set = corner c inside.  A row is the number of triangles (0, 1
 * or 2) and then, per triangle, its three vertices as the number of the tetrahedron's edge that carries each, with the edges
 * numbered (0,1) (0,2) (0,3) (1,2) (1,3) (2,3) = 0 .. 5; unused entries are -1.  Refused: out NULL. */
int vggv_case_table(int32_t* out);

/* Integrates the views 0 .. num_frames - 1, in that order, onto the current contents of the volumes (the caller zeroes them
 * before the first call; two calls over the views [0, a) and [a, S) give the bits of one call over [0, S)).  weights
 * (S, H, W) float32 or NULL: every weight 1.  frames (S, 3, H, W) float32 planar colours or NULL; rgb_sum is touched only
 * when both frames and rgb_sum are given.  Views go 256 to a launch.  Refused: trunc or voxel not > 0 (a NaN is refused),
 * num_frames < 1, height or width < 0, the grids named above.
 *
 * One lane per node, for s = 0 .. S - 1:  Xc = transfer of X under poses[s], projected with cams[s] to (x, y); skip unless
 * Xc[2] > 0.  xi = floor(x + 0.5), yi = floor(y + 0.5) (the nearest pixel, halves up); skip unless 0 <= xi <= W - 1 and
 * 0 <= yi <= H - 1.  z = depth[s][yi][xi]; skip unless z > 0.  w = weights[s][yi][xi] (or 1); skip unless w > 0.
 * sdf = z - Xc[2]; skip unless sdf >= -trunc.  d = min(1, sdf / trunc);  tsdf_sum += w d,  weight_sum += w,
 * rgb_sum[c] += w frames[s][c][yi][xi].  A NaN fails every test and is skipped.  No load is made at a coordinate that is not
 * used. */
int vggv_integrate(const float* depth, const float* weights, const float* frames, const double* poses, const double* cams,
                   int num_frames, int height, int width, double origin_x, double origin_y, double origin_z, double voxel,
                   int nx, int ny, int nz, double trunc, double* tsdf_sum, double* weight_sum, double* rgb_sum, void* stream);

/* The level set.  A node is valid when weight_sum >= min_weight (min_weight > 0; a NaN is refused); its value is
 * s = tsdf_sum / weight_sum; it is inside when it is valid and s < 0 (zero and NaN count as outside).  Node n owns seven
 * edges, numbered 0 .. 6, to the nodes at + (1,0,0), (0,1,0), (0,0,1), (1,1,0), (1,0,1), (0,1,1), (1,1,1) where those
 * exist; an edge carries a vertex when both ends are valid and exactly one end is inside.  Vertices are ordered by owner n,
 * then by edge number.
 *
 * Cell (i, j, k), i < nx - 1, j < ny - 1, k < nz - 1, is numbered by its node and split into six tetrahedra, one per
 * permutation pi of the axes (0, 1, 2) in lexicographic order, numbered 0 .. 5: corners p0 = the cell's node,
 * p_{m+1} = p_m + e_pi(m).  A tetrahedron emits only when its four corners are valid.  sigma = sign(pi); sgn(.) is the sign
 * of a sequence of corner numbers read as a permutation; v(x, y) is the vertex on the edge between p_x and p_y (owned by
 * the lower of the two corners).
 *   One corner a differs from the other three o0 < o1 < o2: the triangle (v(a, o0), v(a, o1), v(a, o2)), its last two
 *   vertices swapped when sgn(a, o0, o1, o2) sigma (+1 if a is the inside corner, -1 if it is the outside one) < 0.
 *   Two inside corners a < b, two outside corners c < d: the quad q = (v(a, c), v(a, d), v(b, d), v(b, c)), taken in the
 *   reverse order (q3, q2, q1, q0) when sgn(a, b, c, d) sigma < 0, emitted as the triangles (q0, q1, q2), (q0, q2, q3).
 * Every triangle's geometric normal then points to growing s.  Faces are ordered by cell, then by tetrahedron, then as
 * written.
 *
 * vggv_mesh_count writes, with group g = the nodes [256 g, 256 g + 256) and G = ceil(N / 256) groups:
 *   edge_mask (N) uint8:       bit e set = edge e of the node carries a vertex;
 *   vertex_offset (N) int32:   the number of vertices owned by the nodes of n's group before n;
 *   face_offset (N) int32:     the number of faces of the cells of n's group before n (a node that is no cell has none);
 *   group_counts (G, 2) int32: the vertices and the faces of each group;
 *   group_offsets (G, 2) int64: the vertices and the faces of the groups before g;
 *   counts (2) int64:          V and F, the numbers of vertices and faces of the mesh.
 * The order comes from counting: a wavefront's prefix sums, the wavefronts' counts per workgroup, then an exclusive scan of
 * the groups' counts by one workgroup in chunks of 1024 groups with a running carry -- integer sums, no cursor.
 * Refused: min_weight not > 0 (a NaN is refused), the grids named above. */
int vggv_mesh_count(const double* tsdf_sum, const double* weight_sum, int nx, int ny, int nz, double min_weight,
                    uint8_t* edge_mask, int32_t* vertex_offset, int32_t* face_offset, int32_t* group_counts,
                    int64_t* group_offsets, int64_t* counts, void* stream);

/* Writes the mesh that vggv_mesh_count counted on the same volumes with the same min_weight.  Row r of the vertex of edge e
 * of node n is  group_offsets[n / 256][0] + vertex_offset[n] + (the number of set bits of edge_mask[n] below bit e)  -- the
 * same look-up names the vertices of a face; the faces of cell n start at row group_offsets[n / 256][1] + face_offset[n].
 * A vertex row >= vertex_capacity and a face row >= face_capacity is not written.
 *
 * The vertex of an edge from its owner a to the other end b:  t = s_a / (s_a - s_b);  position X_a[c] + t (X_b[c] - X_a[c])
 * per component, out_vertices (capacity, 3) doubles.  Colour c_a + t (c_b - c_a) per channel with c = rgb_sum / weight_sum,
 * rounded once to float32, out_rgb (capacity, 3); rgb_sum NULL: out_rgb is not written.  The gradient of s at a node, per
 * axis, with the node's neighbours n+ and n- along the axis: (s(n+) - s(n-)) / (2 h) when both exist and are valid, else
 * (s(n+) - s) / h when n+ is, else (s - s(n-)) / h when n- is, else the gradient is missing.  g = g_a + t (g_b - g_a) per
 * component, len = sqrt(g[0] g[0] + g[1] g[1] + g[2] g[2]); the normal is g[c] / len rounded once to float32, or (0, 0, 0)
 * when either gradient is missing or len is not > 0; out_normals (capacity, 3) float32.  (The gradient points to growing s:
 * outside, towards the cameras.)  out_faces (capacity, 3) int32 vertex rows.
 * Refused: voxel or min_weight not > 0 (a NaN is refused), a negative capacity, the grids named above. */
int vggv_mesh_emit(const double* tsdf_sum, const double* weight_sum, const double* rgb_sum, double origin_x, double origin_y,
                   double origin_z, double voxel, int nx, int ny, int nz, double min_weight, const uint8_t* edge_mask,
                   const int32_t* vertex_offset, const int32_t* face_offset, const int64_t* group_offsets,
                   long vertex_capacity, long face_capacity, double* out_vertices, float* out_normals, float* out_rgb,
                   int32_t* out_faces, void* stream);

#ifdef __cplusplus
}
#endif
#endif
