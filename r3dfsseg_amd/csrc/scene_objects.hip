// Objects from a labelled scan: the device side of scene_objects.py.
// extract_objects ("Objects from a labelled scan", O1-O8): the connected components of a scan's points of
// one class, with a box and a centroid each.  A UNIT is the set of participating points of one class in one cell of the
// grid of build_segments; units of one class in neighbouring cells are joined by the union-find of the growers
// (scene_components.h), the components are the objects.
//   bounds      the bounds of scene_sort.hip over the finite points, then the labels of those points: the largest
//               participating label, the points left out by their label, labels that fit no key     -> the record (read 1)
//   sort        keys label * n_cells + cell, the stable radix sort of scene_sort.hip on (key, scan index), unit heads as
//               flags, their scan, the unit table and the unit of every point (the heads and table launches of
//               build_segments)                                                                      -> U (read 2)
//   union       one thread per unit and the forward half of its neighbourhood (gr_ahead, the walk of build_segments, with
//               the class base of the unit's key): the neighbour's cell is checked against the grid, its key (same class)
//               found by binary search; joined pairs united by gr_unite
//   components  the launches of build_segments: roots, points per root, kept roots, their scan       -> components, S (read 3)
//   stats       per unit the minima, maxima and sub-voxel sums of its points; the units of a wave that share an object are
//               combined by shuffles and sent as one set of integer atomics per wave and object; then per object the box
//               from the integer images and the centroid in float64
//   ids         the kept components numbered in ascending root order, spread to the points           -> the counts (read 4)
// No float goes through an atomic: minima and maxima act on the order-preserving integer image of the float bits, the
// centroid's sums are 64-bit integers.  The same scan and labels give the same bits.
#include "scene_components.h"

#define OB_SUB 256                  // sub-voxel steps per cell (O8)
// the record: the words of build_segments (R3D_GROW_R_*), the two of absorb reused (R3D_OBJ_R_*, r3d.h)
static_assert(R3D_OBJ_R_NPOINTS < R3D_SCENE_GROW_REC, "a word beyond the record");

extern "C" long r3d_scene_obj_ws_words(long M) { return M > 0 && M <= R3D_SCENE_MAX_POINTS ? gr_make_layout(M).total : -1; }

static int ob_check(const char* name, long M, int nx, int ny, int nz, long n_labels, const int32_t* ws, long ws_words) {
  SC_TRY(gr_check_grid(name, M, nx, ny, nz, "cells", ws));
  R3D_REQUIRE(n_labels >= 1 && n_labels * ((long)nx * ny * nz) <= R3D_SCENE_OBJ_KEY, "%s: %ld labels times %ld cells (at most 2^31 - 1)",
              name, n_labels, (long)nx * ny * nz);
  return sc_check_ws(name, ws_words, r3d_scene_obj_ws_words(M));
}

static int ob_check_labels(const char* name, const void* labels, int labels64, const int64_t* ignore, int n_ignore) {
  R3D_REQUIRE(labels, "%s: null pointer (labels)", name);
  R3D_REQUIRE(labels64 == 0 || labels64 == 1, "%s: labels64 %d (0: int32, 1: int64)", name, labels64);
  R3D_REQUIRE(n_ignore >= 0 && n_ignore <= R3D_SCENE_OBJ_IGNORE && (n_ignore == 0 || ignore), "%s: %d ignored classes at %p (0 .. %d)",
              name, n_ignore, (const void*)ignore, R3D_SCENE_OBJ_IGNORE);
  return R3D_OK;
}

// The class of point i (O1): its label when that is >= 0 and not in the ignore table; -1: left out by its label; -2: a
// label that fits no key.
template <class T>
static __device__ __forceinline__ int ob_class(const T* __restrict__ labels, int i, const long long* __restrict__ ignore,
                                               int n_ignore) {
  const long long l = (long long)labels[i];
  if (l < 0) return -1;
  for (int j = 0; j < n_ignore; ++j)
    if (ignore[j] == l) return -1;
  return l > R3D_SCENE_OBJ_LABEL ? -2 : (int)l;
}

// ---- bounds: r3d_scene_grow_bounds' launches, then the labels of the finite points into words 12 .. 15
template <class T>
__global__ __launch_bounds__(SC_THREADS) void r3d_scene_obj_labels_kernel(const float* __restrict__ scan, int ld, int M,
                                                                         const T* __restrict__ labels,
                                                                         const long long* __restrict__ ignore, int n_ignore,
                                                                         int* __restrict__ rec) {
  __shared__ int red[SC_WAVES];
  int top = 0, n_out = 0, n_over = 0, n_in = 0;
  for (long i = (long)blockIdx.x * SC_THREADS + threadIdx.x; i < M; i += (long)gridDim.x * SC_THREADS) {
    const float* p = scan + i * ld;
    if (!sc_finite3(p[0], p[1], p[2])) continue;
    const int c = ob_class(labels, (int)i, ignore, n_ignore);
    n_out += c == -1;
    n_over += c == -2;
    n_in += c >= 0;
    top = c + 1 > top ? c + 1 : top;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int t = __shfl_xor(top, o);
    top = t > top ? t : top;
  }
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = top;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < SC_WAVES; ++w) top = red[w] > top ? red[w] : top;
    if (top > 0) atomicMax(rec + R3D_OBJ_R_NLABELS, top);  // integer maxima and counts: order-independent
  }
  n_out = sc_block_count(n_out, red);
  n_over = sc_block_count(n_over, red);
  n_in = sc_block_count(n_in, red);
  if (threadIdx.x == 0) {
    if (n_out > 0) atomicAdd(rec + R3D_OBJ_R_NUNLABELLED, n_out);
    if (n_over > 0) atomicAdd(rec + R3D_OBJ_R_NOVER, n_over);
    if (n_in > 0) atomicAdd(rec + R3D_OBJ_R_NPOINTS, n_in);
  }
}

extern "C" int r3d_scene_obj_bounds(const float* scan, int ld, long M, const void* labels, int labels64, const int64_t* ignore,
                                    int n_ignore, int32_t* ws, long ws_words, void* stream) {
  R3D_REQUIRE(scan, "r3d_scene_obj_bounds: null pointer (scan)");
  SC_TRY(sc_check_ld("r3d_scene_obj_bounds", ld));
  SC_TRY(ob_check_labels("r3d_scene_obj_bounds", labels, labels64, ignore, n_ignore));
  SC_TRY(ob_check("r3d_scene_obj_bounds", M, 1, 1, 1, 1, ws, ws_words));
  const hipStream_t st = (hipStream_t)stream;
  const gr_layout L = gr_make_layout(M);
  sc_bounds(scan, ld, M, 3, (float*)(ws + L.bpart), (float*)(ws + L.rec), st);  // words 0 .. 6, zeros in 7 .. 15
  const dim3 grid(sc_count_grid(M)), block(SC_THREADS);
  if (labels64)
    hipLaunchKernelGGL(r3d_scene_obj_labels_kernel<long long>, grid, block, 0, st, scan, ld, (int)M, (const long long*)labels,
                       (const long long*)ignore, n_ignore, ws + L.rec);
  else
    hipLaunchKernelGGL(r3d_scene_obj_labels_kernel<int>, grid, block, 0, st, scan, ld, (int)M, (const int*)labels,
                       (const long long*)ignore, n_ignore, ws + L.rec);
  R3D_LAUNCH_CHECK("r3d_scene_obj_bounds");
  return R3D_OK;
}

// ---- sort: keys (O3), the sort, the unit heads, their scan, the unit table
template <class T>
__global__ __launch_bounds__(SC_THREADS) void r3d_scene_obj_keys_kernel(const float* __restrict__ scan, int ld, int M, gr_grid g,
                                                                       int n_labels, const T* __restrict__ labels,
                                                                       const long long* __restrict__ ignore, int n_ignore,
                                                                       int* __restrict__ key, int* __restrict__ idx) {
  const int i = blockIdx.x * SC_THREADS + threadIdx.x;
  if (i >= M) return;
  const float* p = scan + (long)i * ld;
  const float x = p[0], y = p[1], z = p[2];
  const int n_cells = g.nx * g.ny * g.nz;
  int k = n_labels * n_cells;  // a point that takes no part sorts behind every unit
  if (sc_finite3(x, y, z)) {
    const int c = ob_class(labels, i, ignore, n_ignore);
    if (c >= 0 && c < n_labels) k = c * n_cells + gr_cell_key(g, x, y, z);
  }
  key[i] = k;
  idx[i] = i;
}

extern "C" int r3d_scene_obj_sort(const float* scan, int ld, long M, const void* labels, int labels64, const int64_t* ignore,
                                  int n_ignore, float x0, float y0, float z0, float voxel, int nx, int ny, int nz, int n_labels,
                                  long n_points, int32_t* unit_index, int32_t* ws, long ws_words, void* stream) {
  R3D_REQUIRE(scan && unit_index, "r3d_scene_obj_sort: null pointer (scan %p, unit_index %p)", (const void*)scan, (void*)unit_index);
  SC_TRY(sc_check_ld("r3d_scene_obj_sort", ld));
  SC_TRY(ob_check_labels("r3d_scene_obj_sort", labels, labels64, ignore, n_ignore));
  SC_TRY(ob_check("r3d_scene_obj_sort", M, nx, ny, nz, n_labels, ws, ws_words));
  SC_TRY(gr_check_origin("r3d_scene_obj_sort", x0, y0, z0, voxel));
  R3D_REQUIRE(n_points >= 1 && n_points <= M, "r3d_scene_obj_sort: %ld participating points of %ld", n_points, M);
  const hipStream_t st = (hipStream_t)stream;
  const gr_layout L = gr_make_layout(M);
  const int key_limit = n_labels * (nx * ny * nz);
  const gr_grid g = {x0, y0, z0, voxel, nx, ny, nz};
  const dim3 grid(sc_grid_of(M)), block(SC_THREADS);
  if (labels64)
    hipLaunchKernelGGL(r3d_scene_obj_keys_kernel<long long>, grid, block, 0, st, scan, ld, (int)M, g, n_labels,
                       (const long long*)labels, (const long long*)ignore, n_ignore, ws + L.sort.key[0], ws + L.sort.idx[0]);
  else
    hipLaunchKernelGGL(r3d_scene_obj_keys_kernel<int>, grid, block, 0, st, scan, ld, (int)M, g, n_labels, (const int*)labels,
                       (const long long*)ignore, n_ignore, ws + L.sort.key[0], ws + L.sort.idx[0]);
  const int sorted = sc_sort_pairs(ws, L.sort, M, sc_passes(key_limit), st);  // keys run 0 .. key_limit (key_limit: no part)
  int* heads = ws + L.sort.key[sorted ^ 1];
  gr_launch_heads(ws + L.sort.key[sorted], M, key_limit, heads, ws, L, st);
  gr_launch_table(ws + L.sort.key[sorted], ws + L.sort.idx[sorted], M, key_limit, n_points, heads, unit_index, ws, L, st);
  R3D_LAUNCH_CHECK("r3d_scene_obj_sort");
  return R3D_OK;
}

// ---- union (O4, O5)
// One thread per unit a and the units of its class in the forward half of its neighbourhood (gr_ahead with the class base
// of a's key: the last cell of one class and the first of the next are never neighbours).  parent[] only through gr_unite
// (agent-scope atomics, scene_components.h).
__global__ __launch_bounds__(SC_THREADS) void r3d_scene_obj_union_kernel(int U, int nx, int ny, int nz, int conn,
                                                                        const int* __restrict__ ukey, int* __restrict__ parent,
                                                                        int* __restrict__ err) {
  const int a = blockIdx.x * SC_THREADS + threadIdx.x;
  if (a >= U) return;
  const int n_cells = nx * ny * nz;
  const int key = ukey[a];
  const int base = (key / n_cells) * n_cells, cell = key % n_cells;
  const int ix = cell % nx, iy = (cell / nx) % ny, iz = cell / (nx * ny);
  gr_ahead(a, U, nx, ny, nz, conn, ix, iy, iz, base, ukey, [&](int b) { gr_unite(parent, a, b, U, err); });
}

static int ob_check_units(const char* name, long M, long n_units) { return gr_check_rows(name, M, n_units, "units"); }

extern "C" int r3d_scene_obj_union(long M, int nx, int ny, int nz, int n_labels, long n_units, int connectivity, int32_t* ws,
                                   long ws_words, void* stream) {
  SC_TRY(ob_check("r3d_scene_obj_union", M, nx, ny, nz, n_labels, ws, ws_words));
  SC_TRY(ob_check_units("r3d_scene_obj_union", M, n_units));
  SC_TRY(gr_check_connectivity("r3d_scene_obj_union", connectivity));
  const hipStream_t st = (hipStream_t)stream;
  const gr_layout L = gr_make_layout(M);
  const int U = (int)n_units;
  gr_launch_init(U, ws, L, st);
  hipLaunchKernelGGL(r3d_scene_obj_union_kernel, dim3(sc_grid_of(U)), dim3(SC_THREADS), 0, st, U, nx, ny, nz, connectivity,
                     ws + L.vkey, ws + L.parent, ws + L.rec + R3D_GROW_R_ERROR);
  R3D_LAUNCH_CHECK("r3d_scene_obj_union");
  return R3D_OK;
}

// ---- components (O5, O6): the launches of r3d_scene_grow_components
extern "C" int r3d_scene_obj_components(long M, long n_units, int min_points, int32_t* ws, long ws_words, void* stream) {
  SC_TRY(ob_check("r3d_scene_obj_components", M, 1, 1, 1, 1, ws, ws_words));
  SC_TRY(ob_check_units("r3d_scene_obj_components", M, n_units));
  R3D_REQUIRE(min_points >= 1, "r3d_scene_obj_components: min_points %d (at least 1)", min_points);
  gr_launch_components(M, (int)n_units, min_points, ws, gr_make_layout(M), (hipStream_t)stream);
  R3D_LAUNCH_CHECK("r3d_scene_obj_components");
  return R3D_OK;
}

// ---- stats (O7, O8)
// The order-preserving integer image of a float's bits: a < b as floats (and -0.0 < +0.0) exactly when image(a) < image(b) as
// ints.  Its own inverse.
static __device__ __forceinline__ int ob_image(int bits) { return bits >= 0 ? bits : bits ^ 0x7fffffff; }

__global__ __launch_bounds__(SC_THREADS) void r3d_scene_obj_fill_kernel(int S, int* __restrict__ lo, int* __restrict__ hi,
                                                                       long long* __restrict__ sums, int* __restrict__ units) {
  const int s = blockIdx.x * SC_THREADS + threadIdx.x;
  if (s >= S) return;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    lo[3L * s + a] = 0x7fffffff;
    hi[3L * s + a] = (int)0x80000000;
    sums[3L * s + a] = 0;
  }
  units[s] = 0;
}

// One thread per unit: the minima and maxima of its points' coordinates as integer images and the sums of their sub-voxel
// coordinates u = (int)floorf(((v - v0) / voxel) * 256.0f), each operation rounded on its own, clamped to 0 .. 256 n - 1.
// Then one round per distinct object of the wave (neighbouring rows mostly share one): its lanes combine their values by
// shuffles and the first of them sends 6 atomic min / max, 3 64-bit atomic adds and 1 atomic add -- not one set per unit,
// let alone per point (profiles/r22_scene_grow.md: 7.5 ms for one atomic per voxel onto the root of a component that holds
// most of the scan).  Integers only, so the order does not matter.  The root's thread writes the object's class and points.
__global__ __launch_bounds__(SC_THREADS) void r3d_scene_obj_stats_kernel(const float* __restrict__ scan, int ld, int M, int U, int S,
                                                                        gr_grid g, const int* __restrict__ order,
                                                                        const int* __restrict__ ustart, const int* __restrict__ ukey,
                                                                        const int* __restrict__ root, const int* __restrict__ kept,
                                                                        const int* __restrict__ cnt, long long* __restrict__ labels,
                                                                        int* __restrict__ points, int* __restrict__ units,
                                                                        int* __restrict__ lo, int* __restrict__ hi,
                                                                        long long* __restrict__ sums) {
  const int v = blockIdx.x * SC_THREADS + threadIdx.x;
  int s = -1;
  int mn[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, mx[3] = {(int)0x80000000, (int)0x80000000, (int)0x80000000};
  unsigned long long sm[3] = {0ull, 0ull, 0ull};
  if (v < U) {
    const int r = sc_clamp(root[v], 0, U - 1);
    if (kept[r + 1] != kept[r]) s = sc_clamp(kept[r], 0, S - 1);  // after the scan: r is a kept root, kept[r] its number
    if (s >= 0 && r == v) {
      labels[s] = ukey[v] / (g.nx * g.ny * g.nz);
      points[s] = cnt[v];
    }
  }
  const bool live = s >= 0;
  if (live) {
    const int a = sc_clamp(ustart[v], 0, M), b = sc_clamp(ustart[v + 1], a, M);
    const float v0[3] = {g.x0, g.y0, g.z0};
    const int top[3] = {OB_SUB * g.nx - 1, OB_SUB * g.ny - 1, OB_SUB * g.nz - 1};
    for (int i = a; i < b; ++i) {
      const float* p = scan + (long)sc_clamp(order[i], 0, M - 1) * ld;
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const float c = p[j];
        const int im = ob_image(__float_as_int(c));
        mn[j] = im < mn[j] ? im : mn[j];
        mx[j] = im > mx[j] ? im : mx[j];
        const int u = (int)floorf(__fmul_rn(__fdiv_rn(__fsub_rn(c, v0[j]), g.s), (float)OB_SUB));
        sm[j] += (unsigned long long)sc_clamp(u, 0, top[j]);
      }
    }
  }
  gr_per_key(live, s, [&](int s0, bool mine, bool is_leader) {  // one round per distinct object of the wave
    int rmn[3], rmx[3], n = mine ? 1 : 0;
    unsigned long long rsm[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      rmn[j] = mine ? mn[j] : 0x7fffffff;
      rmx[j] = mine ? mx[j] : (int)0x80000000;
      rsm[j] = mine ? sm[j] : 0ull;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const int a = __shfl_xor(rmn[j], o), b = __shfl_xor(rmx[j], o);
        rmn[j] = a < rmn[j] ? a : rmn[j];
        rmx[j] = b > rmx[j] ? b : rmx[j];
        rsm[j] += sc_shfl_xor_u64(rsm[j], o);
      }
      n += __shfl_xor(n, o);
    }
    if (is_leader) {
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        atomicMin(lo + 3L * s0 + j, rmn[j]);
        atomicMax(hi + 3L * s0 + j, rmx[j]);
        atomicAdd((unsigned long long*)(sums + 3L * s0 + j), rsm[j]);
      }
      atomicAdd(units + s0, n);
    }
  });
}

// One thread per object: the box back from its images, in place, and the centroid (O8) in float64, v0 + voxel * ((sum / n) +
// 0.5) / 256 in that order, every operation rounded on its own, rounded once to fp32.
__global__ __launch_bounds__(SC_THREADS) void r3d_scene_obj_finish_kernel(int S, gr_grid g, const int* __restrict__ points,
                                                                         const long long* __restrict__ sums, int* __restrict__ lo,
                                                                         int* __restrict__ hi, float* __restrict__ centroid) {
  const int s = blockIdx.x * SC_THREADS + threadIdx.x;
  if (s >= S) return;
  const double v0[3] = {(double)g.x0, (double)g.y0, (double)g.z0};
  const double n = (double)(points[s] > 0 ? points[s] : 1);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    lo[3L * s + a] = ob_image(lo[3L * s + a]);
    hi[3L * s + a] = ob_image(hi[3L * s + a]);
    const double mean = (double)sums[3L * s + a] / n;
    centroid[3L * s + a] = (float)(v0[a] + ((double)g.s * (mean + 0.5)) / (double)OB_SUB);
  }
}

extern "C" int r3d_scene_obj_stats(const float* scan, int ld, long M, float x0, float y0, float z0, float voxel, int nx, int ny,
                                   int nz, int n_labels, long n_units, long n_objects, int64_t* object_labels,
                                   int32_t* object_points, int32_t* object_units, float* object_lo, float* object_hi,
                                   float* object_centroid, int64_t* object_sums, const int32_t* ws, long ws_words, void* stream) {
  R3D_REQUIRE(scan && object_labels && object_points && object_units && object_lo && object_hi && object_centroid && object_sums,
              "r3d_scene_obj_stats: null pointer (scan %p, labels %p, points %p, units %p, lo %p, hi %p, centroid %p, sums %p)",
              (const void*)scan, (void*)object_labels, (void*)object_points, (void*)object_units, (void*)object_lo,
              (void*)object_hi, (void*)object_centroid, (void*)object_sums);
  SC_TRY(sc_check_ld("r3d_scene_obj_stats", ld));
  SC_TRY(ob_check("r3d_scene_obj_stats", M, nx, ny, nz, n_labels, ws, ws_words));
  SC_TRY(gr_check_origin("r3d_scene_obj_stats", x0, y0, z0, voxel));
  SC_TRY(ob_check_units("r3d_scene_obj_stats", M, n_units));
  R3D_REQUIRE(n_objects >= 1 && n_objects <= n_units, "r3d_scene_obj_stats: %ld objects of %ld units", n_objects, n_units);
  const hipStream_t st = (hipStream_t)stream;
  const gr_view v = gr_make_view(M, (long)n_labels * ((long)nx * ny * nz), ws);
  const gr_grid g = {x0, y0, z0, voxel, nx, ny, nz};
  const int U = (int)n_units, S = (int)n_objects;
  int *lo = (int*)object_lo, *hi = (int*)object_hi;  // integer images until the last launch
  hipLaunchKernelGGL(r3d_scene_obj_fill_kernel, dim3(sc_grid_of(S)), dim3(SC_THREADS), 0, st, S, lo, hi, (long long*)object_sums,
                     object_units);
  hipLaunchKernelGGL(r3d_scene_obj_stats_kernel, dim3(sc_grid_of(U)), dim3(SC_THREADS), 0, st, scan, ld, (int)M, U, S, g, v.order,
                     ws + v.L.vstart, ws + v.L.vkey, ws + v.L.root, ws + v.L.kept, ws + v.L.cnt, (long long*)object_labels,
                     object_points, object_units, lo, hi, (long long*)object_sums);
  hipLaunchKernelGGL(r3d_scene_obj_finish_kernel, dim3(sc_grid_of(S)), dim3(SC_THREADS), 0, st, S, g, object_points,
                     (const long long*)object_sums, lo, hi, object_centroid);
  R3D_LAUNCH_CHECK("r3d_scene_obj_stats");
  return R3D_OK;
}

// ---- ids (O6): the launch of r3d_scene_grow_ids that spreads the numbers to the points
extern "C" int r3d_scene_obj_ids(long M, long n_units, long n_objects, const int32_t* unit_index, int32_t* objects, int32_t* ws,
                                 long ws_words, void* stream) {
  SC_TRY(ob_check("r3d_scene_obj_ids", M, 1, 1, 1, 1, ws, ws_words));
  R3D_REQUIRE(unit_index && objects, "r3d_scene_obj_ids: null pointer (unit_index %p, objects %p)", (const void*)unit_index,
              (void*)objects);
  SC_TRY(ob_check_units("r3d_scene_obj_ids", M, n_units));
  R3D_REQUIRE(n_objects >= 0 && n_objects <= n_units, "r3d_scene_obj_ids: %ld objects of %ld units", n_objects, n_units);
  gr_launch_ids(M, (int)n_units, (int)n_objects, unit_index, objects, nullptr, ws, gr_make_layout(M), (hipStream_t)stream);
  R3D_LAUNCH_CHECK("r3d_scene_obj_ids");
  return R3D_OK;
}
