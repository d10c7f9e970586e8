// What the growers share: scene_grow.hip (build_segments: a unit is a voxel) and scene_objects.hip (extract_objects: a unit
// is a voxel's points of one class) both sort (key, scan index) pairs, cut the sorted keys into rows of a unit table, unite
// neighbouring rows in parent[] and number the kept components.  Here: the record and the workspace they agree on, the
// argument checks, the grid and its cell key, the two walks over a row's neighbours in the table (all 27 cells, and the
// forward half), the loop that sends one set of atomics per wave and key, the union-find on integer atomics, and the
// launchers of the kernels of scene_grow.hip that scene_objects.hip needs as well (a kernel is launched only from the file
// that defines it).
#pragma once
#include "scene_common.h"

static_assert(R3D_GROW_R_MAX + 3 <= R3D_SCENE_GROW_REC && R3D_GROW_R_ABSORBED_POINTS < R3D_SCENE_GROW_REC, "a word beyond the record");

struct gr_layout {
  long rec;              // R3D_SCENE_GROW_REC words, R3D_GROW_R_* (r3d.h)
  long bpart;            // 7 * SC_BOUNDS_BLOCKS: partial bounds
  sc_sort_ws sort;       // pairs of M + 1 words; key of the pair the sort leaves free: the voxel heads, scanned
  long vkey;             // V: key of a voxel row
  long vstart;           // V + 1: first sorted position of a voxel
  long parent, root;     // V each
  long cnt;              // V: points of the component, at its root
  long kept;             // V + 1: kept roots in front of a voxel row
  long total;
};

static inline gr_layout gr_make_layout(long M) {
  gr_layout L;
  const long Ma = sc_align(M + 1);
  long o = 0;
  L.rec = o; o += R3D_SCENE_GROW_REC;
  L.bpart = o; o += sc_align(7L * SC_BOUNDS_BLOCKS);
  o = sc_sort_ws_append(L.sort, o, M, Ma, sc_sort_part_words(M, M + 1));
  L.vkey = o; o += Ma;
  L.vstart = o; o += Ma;
  L.parent = o; o += Ma;
  L.root = o; o += Ma;
  L.cnt = o; o += Ma;
  L.kept = o; o += Ma;
  L.total = o;
  return L;
}

// where the sort of keys 0 .. key_max left its result, and the pair it left free
struct gr_view {
  const int *skey, *order, *heads;
  gr_layout L;
};

static inline gr_view gr_make_view(long M, long key_max, const int32_t* ws) {
  gr_view v;
  v.L = gr_make_layout(M);
  const int sorted = sc_passes(key_max) & 1;
  v.skey = ws + v.L.sort.key[sorted];
  v.order = ws + v.L.sort.idx[sorted];
  v.heads = ws + v.L.sort.key[sorted ^ 1];
  return v;
}

// ---- the argument checks of the entry points
// the workspace pointer, the scan's size and the grid, whose cells the caller calls `noun` ("voxels", "cells")
static inline int gr_check_grid(const char* name, long M, int nx, int ny, int nz, const char* noun, const int32_t* ws) {
  R3D_REQUIRE(ws, "%s: null pointer (ws)", name);
  SC_TRY(sc_check_points(name, M));
  R3D_REQUIRE(nx >= 1 && nx <= R3D_SCENE_GROW_AXIS && ny >= 1 && ny <= R3D_SCENE_GROW_AXIS && nz >= 1 && nz <= R3D_SCENE_GROW_AXIS,
              "%s: %d x %d x %d %s (1 .. 1024 per axis)", name, nx, ny, nz, noun);
  return R3D_OK;
}

static inline int gr_check_origin(const char* name, float x0, float y0, float z0, float voxel) {
  R3D_REQUIRE(x0 == x0 && y0 == y0 && z0 == z0 && voxel > 0.0f && voxel < INFINITY, "%s: origin (%g, %g, %g), voxel size %g", name,
              (double)x0, (double)y0, (double)z0, (double)voxel);
  return R3D_OK;
}

// the rows of the unit table as read from the record: 1 .. M `noun` ("voxels", "units")
static inline int gr_check_rows(const char* name, long M, long n_rows, const char* noun) {
  R3D_REQUIRE(n_rows >= 1 && n_rows <= M, "%s: %ld %s of %ld points", name, n_rows, noun, M);
  return R3D_OK;
}

static inline int gr_check_connectivity(const char* name, int connectivity) {
  R3D_REQUIRE(connectivity == 6 || connectivity == 26, "%s: connectivity %d (6 or 26)", name, connectivity);
  return R3D_OK;
}

// ---- the grid (G2, O3) and the walks over the rows of the unit table, which is sorted by key
struct gr_grid {
  float x0, y0, z0, s;
  int nx, ny, nz;
};

// the key of the cell of a finite point: x runs fastest
static __device__ __forceinline__ int gr_cell_key(const gr_grid& g, float x, float y, float z) {
  return (sc_cell(z, g.z0, g.s, g.nz) * g.ny + sc_cell(y, g.y0, g.s, g.ny)) * g.nx + sc_cell(x, g.x0, g.s, g.nx);
}

// The rows of the occupied cells among the 27 around row v's (its own included): hit(r, d, row) for the cell at dy = r % 3 - 1,
// dz = r / 3 - 1, dx = d - 1, in ascending key order; skip(dy, dz) leaves a (dz, dy) row of the grid out.  The three
// x-neighbours of one (dz, dy) row have consecutive keys: one binary search finds the first candidate row of the table (v's
// own row of the grid needs none), the next two are checked by key, and an x outside the grid is never looked up, so a key
// that belongs to the neighbouring row of the grid is no neighbour.  Both loops are unrolled: r and d are compile-time
// constants in hit, so what it indexes by them stays in registers.
template <class Skip, class Hit>
static __device__ __forceinline__ void gr_around(int v, int V, int nx, int ny, int nz, const int* __restrict__ vkey, Skip skip,
                                                 Hit hit) {
  const int key = vkey[v];
  const int ix = key % nx, iy = (key / nx) % ny, iz = key / (nx * ny);
#pragma unroll
  for (int r = 0; r < 9; ++r) {
    const int dy = r % 3 - 1, dz = r / 3 - 1;
    const int jy = iy + dy, jz = iz + dz;
    if (jy < 0 || jy >= ny || jz < 0 || jz >= nz) continue;
    if (skip(dy, dz)) continue;
    const int base = (jz * ny + jy) * nx;
    const int first = base + (ix > 0 ? ix - 1 : 0);
    int lo = r < 4 ? 0 : v, hi = r < 4 ? v : V;  // rows in front of v hold smaller keys, rows behind it larger ones
    if (r == 4) {
      lo = v > 0 && vkey[v - 1] == first ? v - 1 : v;  // v's own row of the grid: no search
    } else {
      while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (vkey[mid] < first) lo = mid + 1; else hi = mid;
      }
    }
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const int jx = ix + d - 1;
      if (jx < 0 || jx >= nx) continue;
      if (lo < V && vkey[lo] == base + jx) {
        hit(r, d, lo);
        ++lo;
      }
    }
  }
}

// The forward half of the neighbourhood of row a, whose cell is (ix, iy, iz) and whose key is base + that cell's (the offsets
// whose cell key is larger: 3 of 6, 13 of 26): join(row) for every occupied neighbour.  The caller decodes the cell, in
// front of its other loads (decoded here, behind them, the grow union measured 2 % longer).  The neighbour's coordinates are
// checked against the grid BEFORE its key
// is formed from `base` (extract_objects: a's class times the cells; build_segments: 0), so the last cell of one class and
// the first of the next, whose keys are consecutive, are never neighbours; the key is looked up by binary search among the
// rows behind a.
template <class Join>
static __device__ __forceinline__ void gr_ahead(int a, int V, int nx, int ny, int nz, int conn, int ix, int iy, int iz, int base,
                                                const int* __restrict__ vkey, Join join) {
  for (int o = 14; o < 27; ++o) {  // (dz, dy, dx) in lexicographic order behind (0, 0, 0)
    const int dx = o % 3 - 1, dy = (o / 3) % 3 - 1, dz = o / 9 - 1;
    if (conn == 6 && (dx != 0) + (dy != 0) + (dz != 0) != 1) continue;
    const int jx = ix + dx, jy = iy + dy, jz = iz + dz;
    if (jx < 0 || jx >= nx || jy < 0 || jy >= ny || jz < 0 || jz >= nz) continue;
    const int want = base + (jz * ny + jy) * nx + jx;
    int lo = a + 1, hi = V;  // the first row in (a, V) whose key is not below `want`
    while (lo < hi) {
      const int mid = lo + ((hi - lo) >> 1);
      if (vkey[mid] < want) lo = mid + 1; else hi = mid;
    }
    if (lo < V && vkey[lo] == want) join(lo);
  }
}

// One round per distinct key among the live lanes of a wave (neighbouring rows mostly share one): body(key0, mine, is_leader)
// with mine = this lane is live and holds key0, is_leader = it is the first such lane.  The lanes that share a key combine
// their values by shuffles in the body and the leader sends one set of atomics: not one per row (profiles/r22_scene_grow.md:
// 7.5 ms at 10^6 points for one atomic per voxel onto the root of a component that holds most of the scan).  The loop and
// the body's shuffles are wave-uniform: every lane of the wave must get here, so no caller returns early in front of it.
template <class Body>
static __device__ __forceinline__ void gr_per_key(bool live, int key, Body body) {
  const int lane = threadIdx.x & 63;
  unsigned long long todo = __ballot(live);
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const int key0 = __shfl(key, leader);
    const bool mine = live && key == key0;
    body(key0, mine, lane == leader);
    todo &= ~__ballot(mine);
  }
}

// ---- the union-find (G4, G5; O5)
// parent[] is changed inside a union launch by agent-scope atomics only and read by relaxed agent-scope atomic loads: the
// L2s of the XCDs are not coherent for plain accesses within a launch.  Invariants: parent[v] <= v, and a voxel that is
// no root (parent[v] < v) never becomes one again.  A root's parent changes by one compare-and-swap (the hook); any other
// parent only by atomicMin with one of its ancestors (path halving).  So whatever a thread reads is the voxel itself or
// an ancestor of it, and the compare-and-swap decides.  No thread waits for another: every loop below counts down.
static __device__ __forceinline__ int gr_load(const int* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root of v, halving the path; a chain descends strictly, so it has at most V links.  -1: it had more (a corrupted
// table), bit 0 of the error word is set.
static __device__ __forceinline__ int gr_find(int* __restrict__ parent, int v, int V, int* __restrict__ err) {
  for (int step = 0; step <= V; ++step) {
    const int p = gr_load(parent + v);
    if (p == v) return v;
    if (p < 0 || p > v) break;
    const int gp = gr_load(parent + p);
    if (gp < 0 || gp > p) break;
    if (gp != p) atomicMin(parent + v, gp);
    v = gp;
  }
  atomicOr(err, 1);
  return -1;
}

// Unites the components of a and b.  A compare-and-swap on hi fails only when another thread gave hi a parent; hi is no
// root from then on, so no later find returns it and every failure of one unite is at another voxel: fewer than V
// failures, V + 1 attempts bound the loop.  Past that (a corrupted table): bit 1 of the error word.
static __device__ __forceinline__ void gr_unite(int* __restrict__ parent, int a, int b, int V, int* __restrict__ err) {
  for (int attempt = 0; attempt <= V; ++attempt) {
    a = gr_find(parent, a, V, err);
    b = gr_find(parent, b, V, err);
    if (a < 0 || b < 0 || a == b) return;
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    const int old = atomicCAS(parent + hi, hi, lo);
    if (old == hi) return;
    a = old;  // hi has a parent now: go on from it
    b = lo;
  }
  atomicOr(err, 2);
}

// ---- scene_grow.hip: the launches a second grower repeats.  ws and L: the workspace and its layout; every launcher only
// queues work on st.
// the sorted keys -> heads[i] = sorted position i opens a row (its key lies in 0 .. key_limit - 1 and differs from the one
// in front), their exclusive scan in place, its total (the rows) into rec[R3D_GROW_R_V]
R3D_INTERNAL void gr_launch_heads(const int* skey, long M, int key_limit, int* heads, int32_t* ws, const gr_layout& L,
                                  hipStream_t st);
// after gr_launch_heads: the unit table (vkey: the keys in ascending order, vstart: a unit's first sorted position; row
// heads[M] of vstart is n_in, the points that lie in a unit: they are sorted first) and index[p] = the row of scan point
// p's unit, -1 for a point in none
R3D_INTERNAL void gr_launch_table(const int* skey, const int* order, long M, int key_limit, long n_in, const int* heads,
                                  int32_t* index, int32_t* ws, const gr_layout& L, hipStream_t st);
// parent[v] = v
R3D_INTERNAL void gr_launch_init(int V, int32_t* ws, const gr_layout& L, hipStream_t st);
// root[], the points per root, the kept roots and their scan: words R3D_GROW_R_NCOMP, R3D_GROW_R_S (and R3D_GROW_R_ERROR) of the record
R3D_INTERNAL void gr_launch_components(long M, int V, int min_points, int32_t* ws, const gr_layout& L, hipStream_t st);
// the kept components numbered by ascending root: segment_points (S,) (skipped when null) and the id of every point from
// the row of its unit; word R3D_GROW_R_NDROPPED
R3D_INTERNAL void gr_launch_ids(long M, int V, int S, const int32_t* voxel_index, int32_t* segments, int32_t* segment_points,
                                int32_t* ws, const gr_layout& L, hipStream_t st);
