// What the growers share: scene_grow.hip (build_segments: a unit is a voxel) and scene_objects.hip (extract_objects: a unit
// is a voxel's points of one class) both sort (key, scan index) pairs, cut the sorted keys into rows of a unit table, unite
// neighbouring rows in parent[] and number the kept components.  Here: the record and the workspace they agree on, the
// union-find on integer atomics, and the launchers of the kernels of scene_grow.hip that scene_objects.hip needs as well (a
// kernel is launched only from the file that defines it).
#pragma once
#include "scene_common.h"

#define GR_AXIS_MAX 1024  // voxels per axis: keys stay below 2^30
// the record, words of ws[0 .. 16)
#define GR_R_MIN 0        // x0 y0 z0 (float bits)
#define GR_R_MAX 3        // the maxima (float bits)
#define GR_R_NVALID 6
#define GR_R_V 7          // occupied voxels (rows of the unit table)
#define GR_R_NCOMP 8      // components
#define GR_R_S 9          // kept components
#define GR_R_NDROPPED 10  // points of dropped components
#define GR_R_ERROR 11     // != 0: a bounded loop of the union-find ran out (bit 0 a find, bit 1 a unite)
#define GR_R_ABSORBED_VOXELS 12  // voxels of dropped components taken into a kept one (absorb)
#define GR_R_ABSORBED_POINTS 13  // their points

struct gr_layout {
  long rec;              // 16
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
  L.rec = o; o += 16;
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
// in front), their exclusive scan in place, its total (the rows) into rec[GR_R_V]
R3D_INTERNAL void gr_launch_heads(const int* skey, long M, int key_limit, int* heads, int32_t* ws, const gr_layout& L,
                                  hipStream_t st);
// parent[v] = v
R3D_INTERNAL void gr_launch_init(int V, int32_t* ws, const gr_layout& L, hipStream_t st);
// root[], the points per root, the kept roots and their scan: words GR_R_NCOMP, GR_R_S (and GR_R_ERROR) of the record
R3D_INTERNAL void gr_launch_components(long M, int V, int min_points, int32_t* ws, const gr_layout& L, hipStream_t st);
// the kept components numbered by ascending root: segment_points (S,) (skipped when null) and the id of every point from
// the row of its unit; word GR_R_NDROPPED
R3D_INTERNAL void gr_launch_ids(long M, int V, int S, const int32_t* voxel_index, int32_t* segments, int32_t* segment_points,
                                int32_t* ws, const gr_layout& L, hipStream_t st);
