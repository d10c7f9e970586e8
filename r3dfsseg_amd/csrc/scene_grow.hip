// Segments grown on the device: the device side of scene_grow.py.
// build_segments ("Building segments", G1-G7): the partition that pool_segments takes, grown from the scan
// itself.  Points fall into voxels, occupied voxels that touch (and, with a tolerance, whose mean colours agree; with
// normal_tol, whose normals agree) are joined, the connected components are the segments.
//   bounds      (scene_sort.hip) valid points, their xyz extent                -> words 0 .. 6 of the record (read 1)
//   sort        voxel keys, the stable radix sort of scene_sort.hip on (key, scan index), voxel heads as flags, their scan
//                                                                                 -> V (read 2)
//   voxels      the voxel table in ascending key order, the voxel of every point, the mean colour of a voxel (the sums of
//               the segment pool: tiles of 256 ranks, one addition at a time, tiles in order, one division)
//   centroids   with normal_tol: the mean offset of a voxel's points inside the voxel, by the loop of the mean colours
//   normals     with normal_tol: per voxel the second moments of the centroids of the occupied voxels among the 27 around
//               it, (t I - B)^256 by eight squarings, the row of the largest diagonal entry; the support
//   union       one thread per voxel and the forward half of its neighbourhood; a neighbour is found by its coordinates
//               and a binary search of its key; joined pairs are united in parent[] by lock-free hooking; with normal_tol
//               (r3d_scene_grow_union_normals) the same kernel with the test on the squared cosine of two normals
//   components  root[v] = find(v) in a launch of its own, points per root, kept roots as flags, their scan
//                                                                                 -> components, S (read 3)
//   absorb      with absorb > 0: the voxels of dropped components taken ring by ring into the kept component most of
//               their neighbours belong to, one launch per ring over two owner tables; their points join its count
//   ids         the kept components numbered in ascending root order, spread to the points   -> the counts (read 4)
// The union-find holds integers only and the component of a voxel depends on the graph alone: whichever thread hooks
// first, the root of a component ends as its smallest row.  Floats are added by __fadd_rn in the stated order.
// scene_objects.hip grows the units of a labelled scan the same way: the heads, table, init, components and ids launches
// below are gr_launch_* (scene_components.h), called here by the entry points and there by r3d_scene_obj_*.  The walks over
// a voxel's neighbours (gr_around, gr_ahead), the per-key loop of a wave (gr_per_key), the cell key and the argument checks
// are defined there too, once.
#include "scene_components.h"

extern "C" long r3d_scene_grow_ws_words(long M) { return M > 0 && M <= R3D_SCENE_MAX_POINTS ? gr_make_layout(M).total : -1; }

// what every entry point after the bounds has: the scan's size, the grid and the workspace
static int gr_check(const char* name, long M, int nx, int ny, int nz, const int32_t* ws, long ws_words) {
  SC_TRY(gr_check_grid(name, M, nx, ny, nz, "voxels", ws));
  return sc_check_ws(name, ws_words, r3d_scene_grow_ws_words(M));
}

// ---- bounds: the launcher of r3d_scene_bounds with z, into words 0 .. 6 of the record; the other words start at 0
extern "C" int r3d_scene_grow_bounds(const float* scan, int ld, long M, int32_t* ws, long ws_words, void* stream) {
  R3D_REQUIRE(scan, "r3d_scene_grow_bounds: null pointer (scan)");
  SC_TRY(sc_check_ld("r3d_scene_grow_bounds", ld));
  SC_TRY(gr_check("r3d_scene_grow_bounds", M, 1, 1, 1, ws, ws_words));
  const gr_layout L = gr_make_layout(M);
  sc_bounds(scan, ld, M, 3, (float*)(ws + L.bpart), (float*)(ws + L.rec), (hipStream_t)stream);
  R3D_LAUNCH_CHECK("r3d_scene_grow_bounds");
  return R3D_OK;
}

// ---- sort: keys (G2), the sort, the voxel heads and their scan
__global__ __launch_bounds__(SC_THREADS) void r3d_scene_grow_keys_kernel(const float* __restrict__ scan, int ld, int M, gr_grid g,
                                                                         int* __restrict__ key, int* __restrict__ idx) {
  const int i = blockIdx.x * SC_THREADS + threadIdx.x;
  if (i >= M) return;
  const float* p = scan + (long)i * ld;
  const float x = p[0], y = p[1], z = p[2];
  int k = g.nx * g.ny * g.nz;  // invalid points sort behind every voxel
  if (sc_finite3(x, y, z)) k = gr_cell_key(g, x, y, z);
  key[i] = k;
  idx[i] = i;
}

// sorted position i: heads[i] = it opens a voxel; word M is 0, so that the exclusive scan leaves V there
__global__ __launch_bounds__(SC_THREADS) void r3d_scene_grow_heads_kernel(const int* __restrict__ skey, int M, int n_cells,
                                                                          int* __restrict__ heads) {
  const int i = blockIdx.x * SC_THREADS + threadIdx.x;
  if (i > M) return;
  int h = 0;
  if (i < M) {
    const int k = skey[i];
    h = k >= 0 && k < n_cells && (i == 0 || skey[i - 1] != k);
  }
  heads[i] = h;
}

__global__ void r3d_scene_grow_word_kernel(const int* __restrict__ src, int* __restrict__ dst) { *dst = *src; }

void gr_launch_heads(const int* skey, long M, int key_limit, int* heads, int32_t* ws, const gr_layout& L, hipStream_t st) {
  hipLaunchKernelGGL(r3d_scene_grow_heads_kernel, dim3(sc_grid_of(M + 1)), dim3(SC_THREADS), 0, st, skey, (int)M, key_limit, heads);
  sc_excl_scan(heads, M + 1, ws + L.sort.part, st);
  hipLaunchKernelGGL(r3d_scene_grow_word_kernel, dim3(1), dim3(1), 0, st, heads + M, ws + L.rec + R3D_GROW_R_V);
}

extern "C" int r3d_scene_grow_sort(const float* scan, int ld, long M, float x0, float y0, float z0, float voxel, int nx, int ny,
                                   int nz, int32_t* ws, long ws_words, void* stream) {
  R3D_REQUIRE(scan, "r3d_scene_grow_sort: null pointer (scan)");
  SC_TRY(sc_check_ld("r3d_scene_grow_sort", ld));
  SC_TRY(gr_check("r3d_scene_grow_sort", M, nx, ny, nz, ws, ws_words));
  SC_TRY(gr_check_origin("r3d_scene_grow_sort", x0, y0, z0, voxel));
  const hipStream_t st = (hipStream_t)stream;
  const gr_layout L = gr_make_layout(M);
  const int n_cells = nx * ny * nz;
  const gr_grid g = {x0, y0, z0, voxel, nx, ny, nz};
  hipLaunchKernelGGL(r3d_scene_grow_keys_kernel, dim3(sc_grid_of(M)), dim3(SC_THREADS), 0, st, scan, ld, (int)M, g,
                     ws + L.sort.key[0], ws + L.sort.idx[0]);
  const int sorted = sc_sort_pairs(ws, L.sort, M, sc_passes(n_cells), st);  // keys run 0 .. n_cells (n_cells: invalid point)
  gr_launch_heads(ws + L.sort.key[sorted], M, n_cells, ws + L.sort.key[sorted ^ 1], ws, L, st);
  R3D_LAUNCH_CHECK("r3d_scene_grow_sort");
  return R3D_OK;
}

// ---- voxels: the table (G3)
// After the scan: heads[i] = rows opened in front of sorted position i, heads[M] = V (r3d_scene_obj_sort has no host read
// between the scan and this launch, so V is read here).  A row is written by the thread of its first sorted position, row
// V of vstart by the thread of position M: the points that lie in a row are the first n_in of the sorted order.
__global__ __launch_bounds__(SC_THREADS) void r3d_scene_grow_table_kernel(const int* __restrict__ skey, const int* __restrict__ order,
                                                                          int M, int key_limit, int n_in,
                                                                          const int* __restrict__ heads, int* __restrict__ vkey,
                                                                          int* __restrict__ vstart, int* __restrict__ index) {
  const int i = blockIdx.x * SC_THREADS + threadIdx.x;
  if (i > M) return;
  const int V = sc_clamp(heads[M], 0, M);
  if (i == M) {
    vstart[V] = n_in;
    return;
  }
  const int k = skey[i], v = heads[i + 1] - 1;
  const bool in = k >= 0 && k < key_limit && v >= 0 && v < V;
  const int p = sc_clamp(order[i], 0, M - 1);
  index[p] = in ? v : -1;
  if (in && heads[i + 1] != heads[i]) {
    vkey[v] = k;
    vstart[v] = i;
  }
}

void gr_launch_table(const int* skey, const int* order, long M, int key_limit, long n_in, const int* heads, int32_t* index,
                     int32_t* ws, const gr_layout& L, hipStream_t st) {
  hipLaunchKernelGGL(r3d_scene_grow_table_kernel, dim3(sc_grid_of(M + 1)), dim3(SC_THREADS), 0, st, skey, order, (int)M, key_limit,
                     (int)n_in, heads, ws + L.vkey, ws + L.vstart, index);
}

// One thread per voxel: its points in sorted order (ascending scan index: the sort is stable), three values per point
// (row(p, c): those of scan row p) summed as the segment pool sums a segment whose rows all have one vote.
template <class Row>
static __device__ __forceinline__ void gr_voxel_mean(int v, int M, const int* __restrict__ order, const int* __restrict__ vstart,
                                                     float* __restrict__ mean, Row row) {
  const int a = sc_clamp(vstart[v], 0, M), b = sc_clamp(vstart[v + 1], a, M);
  float tot[3] = {0.0f, 0.0f, 0.0f};
  for (int t0 = a; t0 < b; t0 += R3D_SCENE_SEG_TILE) {
    const int t1 = t0 + R3D_SCENE_SEG_TILE < b ? t0 + R3D_SCENE_SEG_TILE : b;
    float part[3] = {0.0f, 0.0f, 0.0f};
    for (int i = t0; i < t1; ++i) {
      float c[3];
      row(sc_clamp(order[i], 0, M - 1), c);
#pragma unroll
      for (int j = 0; j < 3; ++j) part[j] = i == t0 ? c[j] : __fadd_rn(part[j], c[j]);
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) tot[j] = t0 == a ? part[j] : __fadd_rn(tot[j], part[j]);
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) mean[3L * v + j] = b > a ? __fdiv_rn(tot[j], (float)(b - a)) : 0.0f;
}

// the mean colour of a voxel (G3): columns 3 .. 5
__global__ __launch_bounds__(SC_THREADS) void r3d_scene_grow_mean_kernel(const float* __restrict__ scan, int ld, int M, int V,
                                                                         const int* __restrict__ order, const int* __restrict__ vstart,
                                                                         float* __restrict__ mean) {
  const int v = blockIdx.x * SC_THREADS + threadIdx.x;
  if (v >= V) return;
  gr_voxel_mean(v, M, order, vstart, mean, [&](int p, float* c) {
    const float* r = scan + (long)p * ld + 3;
#pragma unroll
    for (int j = 0; j < 3; ++j) c[j] = r[j];
  });
}

extern "C" int r3d_scene_grow_voxels(const float* scan, int ld, long M, int nx, int ny, int nz, long n_valid, long n_voxels,
                                     int32_t* voxel_index, float* voxel_mean, int32_t* ws, long ws_words, void* stream) {
  R3D_REQUIRE(scan && voxel_index, "r3d_scene_grow_voxels: null pointer (scan %p, voxel_index %p)", (const void*)scan,
              (void*)voxel_index);
  const bool colour = voxel_mean != nullptr;
  SC_TRY(sc_check_ld("r3d_scene_grow_voxels", ld));
  SC_TRY(gr_check("r3d_scene_grow_voxels", M, nx, ny, nz, ws, ws_words));
  R3D_REQUIRE(n_valid >= 0 && n_valid <= M && n_voxels >= 0 && n_voxels <= n_valid,
              "r3d_scene_grow_voxels: %ld voxels of %ld valid points among %ld", n_voxels, n_valid, M);
  R3D_REQUIRE(!colour || ld >= 6, "r3d_scene_grow_voxels: a scan row of %d floats has no colour", ld);
  const hipStream_t st = (hipStream_t)stream;
  const gr_view v = gr_make_view(M, (long)nx * ny * nz, ws);
  gr_launch_table(v.skey, v.order, M, nx * ny * nz, n_valid, v.heads, voxel_index, ws, v.L, st);  // heads[M] is n_voxels
  if (colour && n_voxels > 0)
    hipLaunchKernelGGL(r3d_scene_grow_mean_kernel, dim3(sc_grid_of(n_voxels)), dim3(SC_THREADS), 0, st,
                       scan, ld, (int)M, (int)n_voxels, v.order, ws + v.L.vstart, voxel_mean);
  R3D_LAUNCH_CHECK("r3d_scene_grow_voxels");
  return R3D_OK;
}

// ---- centroids (G3c) and normals (G3n): only with normal_tol
// The centroid of a voxel: the mean of its points' offsets INSIDE the voxel, (v - v0) - (float)i * voxel with i decoded from
// the voxel's key, summed as the mean colours are.
__global__ __launch_bounds__(SC_THREADS) void r3d_scene_grow_centroid_kernel(const float* __restrict__ scan, int ld, int M, int V,
                                                                             gr_grid g, const int* __restrict__ order,
                                                                             const int* __restrict__ vstart,
                                                                             const int* __restrict__ vkey, float* __restrict__ centroid) {
  const int v = blockIdx.x * SC_THREADS + threadIdx.x;
  if (v >= V) return;
  const int key = vkey[v];
  const float v0[3] = {g.x0, g.y0, g.z0};
  const float off[3] = {__fmul_rn((float)(key % g.nx), g.s), __fmul_rn((float)((key / g.nx) % g.ny), g.s),
                        __fmul_rn((float)(key / (g.nx * g.ny)), g.s)};
  gr_voxel_mean(v, M, order, vstart, centroid, [&](int p, float* c) {
    const float* r = scan + (long)p * ld;
#pragma unroll
    for (int j = 0; j < 3; ++j) c[j] = __fsub_rn(__fsub_rn(r[j], v0[j]), off[j]);
  });
}

extern "C" int r3d_scene_grow_centroids(const float* scan, int ld, long M, float x0, float y0, float z0, float voxel, int nx,
                                        int ny, int nz, long n_voxels, float* voxel_centroid, const int32_t* ws, long ws_words,
                                        void* stream) {
  R3D_REQUIRE(scan && voxel_centroid, "r3d_scene_grow_centroids: null pointer (scan %p, voxel_centroid %p)", (const void*)scan,
              (void*)voxel_centroid);
  SC_TRY(sc_check_ld("r3d_scene_grow_centroids", ld));
  SC_TRY(gr_check("r3d_scene_grow_centroids", M, nx, ny, nz, ws, ws_words));
  SC_TRY(gr_check_origin("r3d_scene_grow_centroids", x0, y0, z0, voxel));
  SC_TRY(gr_check_rows("r3d_scene_grow_centroids", M, n_voxels, "voxels"));
  const gr_view v = gr_make_view(M, (long)nx * ny * nz, ws);
  const gr_grid g = {x0, y0, z0, voxel, nx, ny, nz};
  hipLaunchKernelGGL(r3d_scene_grow_centroid_kernel, dim3(sc_grid_of(n_voxels)), dim3(SC_THREADS), 0,
                     (hipStream_t)stream, scan, ld, (int)M, (int)n_voxels, g, v.order, ws + v.L.vstart, ws + v.L.vkey,
                     voxel_centroid);
  R3D_LAUNCH_CHECK("r3d_scene_grow_centroids");
  return R3D_OK;
}

#define GR_MIN_SUPPORT 4  // occupied voxels of the 27 below which a voxel has no normal
#define GR_SQUARINGS 8    // (t I - B)^(2^8)

// q of the neighbour at offset o (dx = o % 3 - 1, dy = (o / 3) % 3 - 1, dz = o / 9 - 1), whose centroid is c
static __device__ __forceinline__ void gr_q(int o, float s, const float* __restrict__ c, float* q) {
  q[0] = __fadd_rn(__fmul_rn((float)(o % 3 - 1), s), c[0]);
  q[1] = __fadd_rn(__fmul_rn((float)((o / 3) % 3 - 1), s), c[1]);
  q[2] = __fadd_rn(__fmul_rn((float)(o / 9 - 1), s), c[2]);
}

// One thread per voxel.  The rows of the occupied voxels among the 27 around it come from gr_around and stay in registers
// (every loop over them is unrolled, no index is a run-time value); the centroids are gathered once for the mean and once
// more for the second moments.
__global__ __launch_bounds__(SC_THREADS) void r3d_scene_grow_normals_kernel(int V, int nx, int ny, int nz, float s,
                                                                            const int* __restrict__ vkey,
                                                                            const float* __restrict__ centroid,
                                                                            float* __restrict__ normal, int* __restrict__ support) {
  const int v = blockIdx.x * SC_THREADS + threadIdx.x;
  if (v >= V) return;
  int nb[27];
  int k = 0;
#pragma unroll
  for (int o = 0; o < 27; ++o) nb[o] = -1;
  gr_around(v, V, nx, ny, nz, vkey, [](int, int) { return false; }, [&](int r, int d, int row) {
    nb[3 * r + d] = row;
    ++k;
  });
  float m[3] = {0.0f, 0.0f, 0.0f};
  bool first = true;
#pragma unroll
  for (int o = 0; o < 27; ++o) {
    float q[3];
    gr_q(o, s, centroid + 3L * (nb[o] < 0 ? v : nb[o]), q);
    if (nb[o] >= 0) {
#pragma unroll
      for (int a = 0; a < 3; ++a) m[a] = first ? q[a] : __fadd_rn(m[a], q[a]);
      first = false;
    }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) m[a] = __fdiv_rn(m[a], (float)k);
  float C[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};  // 00 01 02 11 12 22
  first = true;
#pragma unroll
  for (int o = 0; o < 27; ++o) {
    float q[3];
    gr_q(o, s, centroid + 3L * (nb[o] < 0 ? v : nb[o]), q);
    if (nb[o] >= 0) {
      const float e0 = __fsub_rn(q[0], m[0]), e1 = __fsub_rn(q[1], m[1]), e2 = __fsub_rn(q[2], m[2]);
      const float p[6] = {__fmul_rn(e0, e0), __fmul_rn(e0, e1), __fmul_rn(e0, e2), __fmul_rn(e1, e1), __fmul_rn(e1, e2),
                          __fmul_rn(e2, e2)};
#pragma unroll
      for (int j = 0; j < 6; ++j) C[j] = first ? p[j] : __fadd_rn(C[j], p[j]);
      first = false;
    }
  }
  support[v] = k;
  bool finite = true;
#pragma unroll
  for (int j = 0; j < 6; ++j) finite = finite && fabsf(C[j]) < INFINITY;
  const float top = fmaxf(fmaxf(C[0], C[3]), C[5]);
  float* out = normal + 3L * v;
  if (k < GR_MIN_SUPPORT || !finite || !(top > 0.0f)) {
    out[0] = out[1] = out[2] = __int_as_float(0x7fc00000);
    return;
  }
  float A[6];
#pragma unroll
  for (int j = 0; j < 6; ++j) A[j] = __fdiv_rn(C[j], top);  // B
  const float t = __fadd_rn(__fadd_rn(A[0], A[3]), A[5]);
  A[0] = __fsub_rn(t, A[0]);
  A[1] = -A[1];
  A[2] = -A[2];
  A[3] = __fsub_rn(t, A[3]);
  A[4] = -A[4];
  A[5] = __fsub_rn(t, A[5]);
#define GR_DOT3(x0, y0, x1, y1, x2, y2) __fadd_rn(__fadd_rn(__fmul_rn(x0, y0), __fmul_rn(x1, y1)), __fmul_rn(x2, y2))
  for (int it = 0; it < GR_SQUARINGS; ++it) {
    const float N[6] = {GR_DOT3(A[0], A[0], A[1], A[1], A[2], A[2]), GR_DOT3(A[0], A[1], A[1], A[3], A[2], A[4]),
                        GR_DOT3(A[0], A[2], A[1], A[4], A[2], A[5]), GR_DOT3(A[1], A[1], A[3], A[3], A[4], A[4]),
                        GR_DOT3(A[1], A[2], A[3], A[4], A[4], A[5]), GR_DOT3(A[2], A[2], A[4], A[4], A[5], A[5])};
    const float mx = fmaxf(fmaxf(N[0], N[3]), N[5]);
#pragma unroll
    for (int j = 0; j < 6; ++j) A[j] = __fdiv_rn(N[j], mx);
  }
  // the row of the largest diagonal entry, the lowest on a tie
  const int j = A[3] > A[0] ? (A[5] > A[3] ? 2 : 1) : (A[5] > A[0] ? 2 : 0);
  out[0] = j == 0 ? A[0] : (j == 1 ? A[1] : A[2]);
  out[1] = j == 0 ? A[1] : (j == 1 ? A[3] : A[4]);
  out[2] = j == 0 ? A[2] : (j == 1 ? A[4] : A[5]);
}

extern "C" int r3d_scene_grow_normals(long M, int nx, int ny, int nz, long n_voxels, float voxel, const float* voxel_centroid,
                                      float* voxel_normal, int32_t* voxel_support, const int32_t* ws, long ws_words,
                                      void* stream) {
  R3D_REQUIRE(voxel_centroid && voxel_normal && voxel_support,
              "r3d_scene_grow_normals: null pointer (voxel_centroid %p, voxel_normal %p, voxel_support %p)",
              (const void*)voxel_centroid, (void*)voxel_normal, (void*)voxel_support);
  SC_TRY(gr_check("r3d_scene_grow_normals", M, nx, ny, nz, ws, ws_words));
  R3D_REQUIRE(voxel > 0.0f && voxel < INFINITY, "r3d_scene_grow_normals: voxel size %g", (double)voxel);
  SC_TRY(gr_check_rows("r3d_scene_grow_normals", M, n_voxels, "voxels"));
  const gr_layout L = gr_make_layout(M);
  hipLaunchKernelGGL(r3d_scene_grow_normals_kernel, dim3(sc_grid_of(n_voxels)), dim3(SC_THREADS), 0,
                     (hipStream_t)stream, (int)n_voxels, nx, ny, nz, voxel, ws + L.vkey, voxel_centroid, voxel_normal,
                     voxel_support);
  R3D_LAUNCH_CHECK("r3d_scene_grow_normals");
  return R3D_OK;
}

// ---- union (G4, G5)
// The union-find itself (gr_load, gr_find, gr_unite: parent[] touched by agent-scope atomics only, no thread waits) is in
// scene_components.h.
__global__ __launch_bounds__(SC_THREADS) void r3d_scene_grow_init_kernel(int V, int* __restrict__ parent) {
  const int v = blockIdx.x * SC_THREADS + threadIdx.x;
  if (v < V) parent[v] = v;
}

void gr_launch_init(int V, int32_t* ws, const gr_layout& L, hipStream_t st) {
  hipLaunchKernelGGL(r3d_scene_grow_init_kernel, dim3(sc_grid_of(V)), dim3(SC_THREADS), 0, st, V, ws + L.parent);
}

// One thread per voxel a and the occupied voxels of the forward half of its neighbourhood (gr_ahead).  NORMALS
// (r3d_scene_grow_union_normals): a pair is joined only when dot^2 >= (cos2 la) lb as well, la and lb the squared lengths of
// the two normal rows; a NaN in either row makes the comparison false.
static __device__ __forceinline__ float gr_dot3(const float* x, const float* y) {
  return __fadd_rn(__fadd_rn(__fmul_rn(x[0], y[0]), __fmul_rn(x[1], y[1])), __fmul_rn(x[2], y[2]));
}

template <bool NORMALS>
__global__ __launch_bounds__(SC_THREADS) void r3d_scene_grow_union_kernel(int V, int nx, int ny, int nz, int conn,
                                                                          const int* __restrict__ vkey, int use_colour, float tol,
                                                                          const float* __restrict__ mean,
                                                                          const float* __restrict__ normal, float cos2,
                                                                          int* __restrict__ parent, int* __restrict__ err) {
  const int a = blockIdx.x * SC_THREADS + threadIdx.x;
  if (a >= V) return;
  float na[3] = {0.0f, 0.0f, 0.0f}, la = 0.0f;
  if (NORMALS) {
#pragma unroll
    for (int j = 0; j < 3; ++j) na[j] = normal[3L * a + j];
    la = __fmul_rn(cos2, gr_dot3(na, na));
  }
  const int key = vkey[a];
  const int ix = key % nx, iy = (key / nx) % ny, iz = key / (nx * ny);
  float ma[3] = {0.0f, 0.0f, 0.0f};
  if (use_colour) {
#pragma unroll
    for (int j = 0; j < 3; ++j) ma[j] = mean[3L * a + j];
  }
  gr_ahead(a, V, nx, ny, nz, conn, ix, iy, iz, 0, vkey, [&](int b) {
    if (use_colour) {
      bool alike = true;
#pragma unroll
      for (int j = 0; j < 3; ++j) alike = alike && fabsf(__fsub_rn(ma[j], mean[3L * b + j])) <= tol;  // a NaN joins nothing
      if (!alike) return;
    }
    if (NORMALS) {
      const float nb[3] = {normal[3L * b], normal[3L * b + 1], normal[3L * b + 2]};
      const float dot = gr_dot3(na, nb);
      if (!(__fmul_rn(dot, dot) >= __fmul_rn(la, gr_dot3(nb, nb)))) return;
    }
    gr_unite(parent, a, b, V, err);
  });
}

static int gr_union(const char* name, long M, int nx, int ny, int nz, long n_voxels, int connectivity, const float* voxel_mean,
                    float colour_tol, const float* voxel_normal, float cos2, int32_t* ws, long ws_words, void* stream) {
  const bool colour = voxel_mean != nullptr;
  SC_TRY(gr_check(name, M, nx, ny, nz, ws, ws_words));
  SC_TRY(gr_check_rows(name, M, n_voxels, "voxels"));
  SC_TRY(gr_check_connectivity(name, connectivity));
  R3D_REQUIRE(!colour || (colour_tol >= 0.0f && colour_tol < INFINITY), "%s: colour_tol %g (finite, >= 0)", name,
              (double)colour_tol);
  const hipStream_t st = (hipStream_t)stream;
  const gr_layout L = gr_make_layout(M);
  const int V = (int)n_voxels, gv = sc_grid_of(V);
  gr_launch_init(V, ws, L, st);
  if (voxel_normal)
    hipLaunchKernelGGL(r3d_scene_grow_union_kernel<true>, dim3(gv), dim3(SC_THREADS), 0, st, V, nx, ny, nz, connectivity,
                       ws + L.vkey, colour ? 1 : 0, colour_tol, voxel_mean, voxel_normal, cos2, ws + L.parent,
                       ws + L.rec + R3D_GROW_R_ERROR);
  else
    hipLaunchKernelGGL(r3d_scene_grow_union_kernel<false>, dim3(gv), dim3(SC_THREADS), 0, st, V, nx, ny, nz, connectivity,
                       ws + L.vkey, colour ? 1 : 0, colour_tol, voxel_mean, voxel_normal, cos2, ws + L.parent,
                       ws + L.rec + R3D_GROW_R_ERROR);
  R3D_LAUNCH_CHECK(name);
  return R3D_OK;
}

extern "C" int r3d_scene_grow_union(long M, int nx, int ny, int nz, long n_voxels, int connectivity, const float* voxel_mean,
                                    float colour_tol, int32_t* ws, long ws_words, void* stream) {
  return gr_union("r3d_scene_grow_union", M, nx, ny, nz, n_voxels, connectivity, voxel_mean, colour_tol, nullptr, 0.0f, ws,
                  ws_words, stream);
}

extern "C" int r3d_scene_grow_union_normals(long M, int nx, int ny, int nz, long n_voxels, int connectivity,
                                            const float* voxel_mean, float colour_tol, const float* voxel_normal, float cos2,
                                            int32_t* ws, long ws_words, void* stream) {
  R3D_REQUIRE(voxel_normal, "r3d_scene_grow_union_normals: null pointer (voxel_normal)");
  R3D_REQUIRE(cos2 >= 0.0f && cos2 <= 1.0f, "r3d_scene_grow_union_normals: cos2 %g (0 .. 1)", (double)cos2);
  return gr_union("r3d_scene_grow_union_normals", M, nx, ny, nz, n_voxels, connectivity, voxel_mean, colour_tol, voxel_normal,
                  cos2, ws, ws_words, stream);
}

// ---- components (G5, G6): root[v] = find(v) in a launch of its own, into another array.  No hook happens here, so the
// roots are final; the finds still halve the paths they walk, with the atomics of the union.
__global__ __launch_bounds__(SC_THREADS) void r3d_scene_grow_flatten_kernel(int V, int* __restrict__ parent, int* __restrict__ root,
                                                                            int* __restrict__ err) {
  const int v = blockIdx.x * SC_THREADS + threadIdx.x;
  if (v >= V) return;
  const int r = gr_find(parent, v, V, err);
  root[v] = r < 0 ? v : r;  // (an overrun: an index inside the tables; the host raises on the error word)
}

// cnt[r] += n over the live lanes: integer atomics, order-independent.  The lanes of a wave that share r add their n first
// and send one atomic (gr_per_key: every lane of the wave calls this).
static __device__ __forceinline__ void gr_add_points(bool live, int r, int n, int* __restrict__ cnt) {
  gr_per_key(live, r, [&](int r0, bool mine, bool is_leader) {
    int sum = mine ? n : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    if (is_leader) atomicAdd(cnt + r0, sum);
  });
}

// points per root
__global__ __launch_bounds__(SC_THREADS) void r3d_scene_grow_count_kernel(int V, int M, const int* __restrict__ root,
                                                                          const int* __restrict__ vstart, int* __restrict__ cnt) {
  const int v = blockIdx.x * SC_THREADS + threadIdx.x;
  const bool live = v < V;
  int r = -1, n = 0;
  if (live) {
    const int a = sc_clamp(vstart[v], 0, M), b = sc_clamp(vstart[v + 1], a, M);
    r = sc_clamp(root[v], 0, V - 1);
    n = b - a;
  }
  gr_add_points(live, r, n, cnt);
}

// row v: kept[v] = it is the root of a component with at least min_points points; word V is 0 for the scan's total
__global__ __launch_bounds__(SC_THREADS) void r3d_scene_grow_kept_kernel(int V, int min_points, const int* __restrict__ root,
                                                                         const int* __restrict__ cnt, int* __restrict__ kept,
                                                                         int* __restrict__ rec) {
  __shared__ int red[SC_WAVES];
  const int v = blockIdx.x * SC_THREADS + threadIdx.x;
  const bool is_root = v < V && root[v] == v;
  if (v <= V) kept[v] = is_root && cnt[v] >= min_points;
  const int n = sc_block_count(is_root ? 1 : 0, red);
  if (threadIdx.x == 0 && n > 0) atomicAdd(rec + R3D_GROW_R_NCOMP, n);
}

void gr_launch_components(long M, int V, int min_points, int32_t* ws, const gr_layout& L, hipStream_t st) {
  const int gv = sc_grid_of(V), gv1 = sc_grid_of(V + 1);
  int* rec = ws + L.rec;
  r3d_zero_words(rec + R3D_GROW_R_NCOMP, 2, st);
  r3d_zero_words(ws + L.cnt, V, st);
  hipLaunchKernelGGL(r3d_scene_grow_flatten_kernel, dim3(gv), dim3(SC_THREADS), 0, st, V, ws + L.parent, ws + L.root,
                     rec + R3D_GROW_R_ERROR);
  hipLaunchKernelGGL(r3d_scene_grow_count_kernel, dim3(gv), dim3(SC_THREADS), 0, st, V, (int)M, ws + L.root, ws + L.vstart,
                     ws + L.cnt);
  hipLaunchKernelGGL(r3d_scene_grow_kept_kernel, dim3(gv1), dim3(SC_THREADS), 0, st, V, min_points, ws + L.root, ws + L.cnt,
                     ws + L.kept, rec);
  sc_excl_scan(ws + L.kept, V + 1L, ws + L.sort.part, st);
  hipLaunchKernelGGL(r3d_scene_grow_word_kernel, dim3(1), dim3(1), 0, st, ws + L.kept + V, rec + R3D_GROW_R_S);
}

extern "C" int r3d_scene_grow_components(long M, long n_voxels, int min_points, int32_t* ws, long ws_words, void* stream) {
  SC_TRY(gr_check("r3d_scene_grow_components", M, 1, 1, 1, ws, ws_words));
  SC_TRY(gr_check_rows("r3d_scene_grow_components", M, n_voxels, "voxels"));
  R3D_REQUIRE(min_points >= 1, "r3d_scene_grow_components: min_points %d (at least 1)", min_points);
  gr_launch_components(M, (int)n_voxels, min_points, ws, gr_make_layout(M), (hipStream_t)stream);
  R3D_LAUNCH_CHECK("r3d_scene_grow_components");
  return R3D_OK;
}

// ---- absorb (G6a): the voxels of dropped components taken into the kept component most of their neighbours belong to,
// ring by ring.  owner[v]: the root of the kept component v belongs to, -1 while v is free.  Two owner tables, one read
// and one written per round (a Jacobi round): a voxel taken in round r is seen by its neighbours from round r + 1 on.  One
// lies in the index array of the pair the sort leaves free, the other in parent[], which nothing reads after the flatten
// launch.  Rounds are launches of their own, so what a round reads was written by an earlier launch: plain loads and
// stores, no atomics on the owner tables.  No thread waits for another; a round's loops are the 27 offsets and the depth
// of a binary search.
__global__ __launch_bounds__(SC_THREADS) void r3d_scene_grow_absorb_start_kernel(int V, const int* __restrict__ root,
                                                                                 const int* __restrict__ kept,
                                                                                 int* __restrict__ owner, int* __restrict__ ring) {
  const int v = blockIdx.x * SC_THREADS + threadIdx.x;
  if (v >= V) return;
  const int r = sc_clamp(root[v], 0, V - 1);
  const bool in = kept[r + 1] != kept[r];  // after the scan: r is a kept root
  owner[v] = in ? r : -1;
  ring[v] = in ? 0 : -1;
}

// One thread per voxel.  A voxel that has an owner copies it.  A free one looks its neighbours up as the normals kernel
// does (gr_around; with connectivity 6 the (dz, dy) rows of the grid that hold no face neighbour are not searched), keeps
// the owners of those the connectivity allows in registers (every loop over them is unrolled), and takes the owner most of
// them have, the smallest on a tie.  Its own row is free, so it never counts.  The unrolled 27 x 27 tally takes 206 VGPRs;
// rolled over candidates picked by selects it takes 44 and the absorb span was 5 to 15 % longer
// (profiles/r25_scene_grow_absorb.md): a ring is bound by the free lanes' latency.
__global__ __launch_bounds__(SC_THREADS) void r3d_scene_grow_absorb_round_kernel(int V, int nx, int ny, int nz, int conn, int round,
                                                                                 const int* __restrict__ vkey,
                                                                                 const int* __restrict__ src, int* __restrict__ dst,
                                                                                 int* __restrict__ ring) {
  const int v = blockIdx.x * SC_THREADS + threadIdx.x;
  if (v >= V) return;
  const int mine = src[v];
  if (mine >= 0) {
    dst[v] = mine;
    return;
  }
  int own[27];
#pragma unroll
  for (int o = 0; o < 27; ++o) own[o] = -1;
  gr_around(v, V, nx, ny, nz, vkey, [&](int dy, int dz) { return conn == 6 && dy != 0 && dz != 0; }, [&](int r, int d, int row) {
    if (conn != 6 || (d != 1) + (r % 3 != 1) + (r / 3 != 1) == 1) own[3 * r + d] = sc_clamp(src[row], -1, V - 1);
  });
  int best = -1, best_n = 0;
#pragma unroll
  for (int i = 0; i < 27; ++i) {
    int n = 0;
#pragma unroll
    for (int j = 0; j < 27; ++j) n += own[j] == own[i];
    if (own[i] >= 0 && (n > best_n || (n == best_n && own[i] < best))) {
      best = own[i];
      best_n = n;
    }
  }
  dst[v] = best;
  if (best >= 0) ring[v] = round;
}

// The absorbed voxels (ring > 0) get their owner as their root and add their points to the owner's count: as in the count
// kernel, the lanes of a wave that share an owner add first.  Words 12 and 13 of the record: absorbed voxels and points.
__global__ __launch_bounds__(SC_THREADS) void r3d_scene_grow_absorb_end_kernel(int V, int M, const int* __restrict__ owner,
                                                                               const int* __restrict__ ring,
                                                                               const int* __restrict__ vstart, int* __restrict__ root,
                                                                               int* __restrict__ cnt, int* __restrict__ rec) {
  __shared__ int red[SC_WAVES];
  const int v = blockIdx.x * SC_THREADS + threadIdx.x;
  int r = -1, n = 0;
  if (v < V && ring[v] > 0) r = sc_clamp(owner[v], -1, V - 1);
  const bool live = r >= 0;
  if (live) {
    const int a = sc_clamp(vstart[v], 0, M), b = sc_clamp(vstart[v + 1], a, M);
    n = b - a;
    root[v] = r;
  }
  gr_add_points(live, r, n, cnt);
  const int voxels = sc_block_count(live ? 1 : 0, red), points = sc_block_count(n, red);
  if (threadIdx.x == 0 && voxels > 0) {
    atomicAdd(rec + R3D_GROW_R_ABSORBED_VOXELS, voxels);  // integer counts: order-independent
    atomicAdd(rec + R3D_GROW_R_ABSORBED_POINTS, points);
  }
}

extern "C" int r3d_scene_grow_absorb(long M, int nx, int ny, int nz, long n_voxels, int connectivity, int rings,
                                     int32_t* voxel_ring, int32_t* ws, long ws_words, void* stream) {
  R3D_REQUIRE(voxel_ring, "r3d_scene_grow_absorb: null pointer (voxel_ring)");
  SC_TRY(gr_check("r3d_scene_grow_absorb", M, nx, ny, nz, ws, ws_words));
  SC_TRY(gr_check_rows("r3d_scene_grow_absorb", M, n_voxels, "voxels"));
  SC_TRY(gr_check_connectivity("r3d_scene_grow_absorb", connectivity));
  R3D_REQUIRE(rings >= 1 && rings <= R3D_SCENE_GROW_RINGS, "r3d_scene_grow_absorb: %d rings (1 .. %d)", rings, R3D_SCENE_GROW_RINGS);
  const hipStream_t st = (hipStream_t)stream;
  const gr_layout L = gr_make_layout(M);
  const int sorted = sc_passes((long)nx * ny * nz) & 1;
  const int V = (int)n_voxels, gv = sc_grid_of(V);
  int* owner[2] = {ws + L.sort.idx[sorted ^ 1], ws + L.parent};  // M + 1 and V words: both hold V
  int* rec = ws + L.rec;
  r3d_zero_words(rec + R3D_GROW_R_ABSORBED_VOXELS, 2, st);
  hipLaunchKernelGGL(r3d_scene_grow_absorb_start_kernel, dim3(gv), dim3(SC_THREADS), 0, st, V, ws + L.root, ws + L.kept, owner[0],
                     voxel_ring);
  for (int r = 1; r <= rings; ++r)
    hipLaunchKernelGGL(r3d_scene_grow_absorb_round_kernel, dim3(gv), dim3(SC_THREADS), 0, st, V, nx, ny, nz, connectivity, r,
                       ws + L.vkey, owner[(r - 1) & 1], owner[r & 1], voxel_ring);
  hipLaunchKernelGGL(r3d_scene_grow_absorb_end_kernel, dim3(gv), dim3(SC_THREADS), 0, st, V, (int)M, owner[rings & 1], voxel_ring,
                     ws + L.vstart, ws + L.root, ws + L.cnt, rec);
  R3D_LAUNCH_CHECK("r3d_scene_grow_absorb");
  return R3D_OK;
}

// ---- ids (G7): after the scan kept[v] = kept roots in front of row v, the id of a kept root
__global__ __launch_bounds__(SC_THREADS) void r3d_scene_grow_sizes_kernel(int V, int S, const int* __restrict__ kept,
                                                                          const int* __restrict__ cnt, int* __restrict__ segment_points) {
  const int v = blockIdx.x * SC_THREADS + threadIdx.x;
  if (v >= V) return;
  const int s = kept[v];
  if (kept[v + 1] != s && s >= 0 && s < S) segment_points[s] = cnt[v];
}

__global__ __launch_bounds__(SC_THREADS) void r3d_scene_grow_spread_kernel(int M, int V, const int* __restrict__ voxel_index,
                                                                           const int* __restrict__ root, const int* __restrict__ kept,
                                                                           int* __restrict__ segments, int* __restrict__ rec) {
  __shared__ int red[SC_WAVES];
  int n_drop = 0;
  for (long p = (long)blockIdx.x * SC_THREADS + threadIdx.x; p < M; p += (long)gridDim.x * SC_THREADS) {
    const int v = voxel_index[p];
    int s = -1;
    if (v >= 0 && v < V) {
      const int r = sc_clamp(root[v], 0, V - 1);
      if (kept[r + 1] != kept[r]) s = kept[r];
      n_drop += s < 0;
    }
    segments[p] = s;
  }
  n_drop = sc_block_count(n_drop, red);
  if (threadIdx.x == 0 && n_drop > 0) atomicAdd(rec + R3D_GROW_R_NDROPPED, n_drop);  // an integer count: order-independent
}

void gr_launch_ids(long M, int V, int S, const int32_t* voxel_index, int32_t* segments, int32_t* segment_points, int32_t* ws,
                   const gr_layout& L, hipStream_t st) {
  r3d_zero_words(ws + L.rec + R3D_GROW_R_NDROPPED, 1, st);
  if (S > 0 && segment_points)
    hipLaunchKernelGGL(r3d_scene_grow_sizes_kernel, dim3(sc_grid_of(V)), dim3(SC_THREADS), 0, st, V, S, ws + L.kept, ws + L.cnt,
                       segment_points);
  hipLaunchKernelGGL(r3d_scene_grow_spread_kernel, dim3(sc_count_grid(M)), dim3(SC_THREADS), 0, st, (int)M, V, voxel_index,
                     ws + L.root, ws + L.kept, segments, ws + L.rec);
}

extern "C" int r3d_scene_grow_ids(long M, long n_voxels, long n_segments, const int32_t* voxel_index, int32_t* segments,
                                  int32_t* segment_points, int32_t* ws, long ws_words, void* stream) {
  SC_TRY(gr_check("r3d_scene_grow_ids", M, 1, 1, 1, ws, ws_words));
  R3D_REQUIRE(voxel_index && segments, "r3d_scene_grow_ids: null pointer (voxel_index %p, segments %p)", (const void*)voxel_index,
              (void*)segments);
  R3D_REQUIRE(n_voxels >= 1 && n_voxels <= M && n_segments >= 0 && n_segments <= n_voxels,
              "r3d_scene_grow_ids: %ld segments of %ld voxels of %ld points", n_segments, n_voxels, M);
  R3D_REQUIRE(n_segments == 0 || segment_points, "r3d_scene_grow_ids: null pointer (segment_points)");
  gr_launch_ids(M, (int)n_voxels, (int)n_segments, voxel_index, segments, segment_points, ws, gr_make_layout(M),
                (hipStream_t)stream);
  R3D_LAUNCH_CHECK("r3d_scene_grow_ids");
  return R3D_OK;
}
