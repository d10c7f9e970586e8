// What the scene sources share: scene.hip (labelling and support), scene_segments.hip (pool_segments), scene_grow.hip
// (build_segments) and scene_objects.hip (extract_objects; with scene_grow.hip through scene_components.h) all stand on the
// sort, the scan and the bounds of scene_sort.hip.  Here: the sizes they agree on, the
// device helpers more than one of them uses, the workspace of the sort, the argument checks they have in common and the
// host launchers of scene_sort.hip.  A kernel is launched only from the file that defines it.
#pragma once
#include "common.h"

#define SC_THREADS 256
#define SC_WAVES (SC_THREADS / R3D_WAVE)
#define SC_TILE 2048                 // points per sort tile, elements per scan block (8 per thread)
#define SC_PLAN_THREADS 1024         // the one-workgroup kernels that scan a table
#define SC_BOUNDS_BLOCKS 1024
#define SC_COUNT_BLOCKS 1024         // workgroups of the kernels that end in atomics on a record

// ------------------------------------------------------------------------------------------------ device helpers
static __device__ __forceinline__ bool sc_finite3(float x, float y, float z) {
  return isfinite(x) && isfinite(y) && isfinite(z);
}

// (int)floorf((v - v0) / s): an IEEE subtraction and an IEEE division (the build neither contracts nor uses a
// reciprocal).  The clamp never acts on a valid point when the host derived n from the same arithmetic (the
// expression is monotone in v); it keeps a key inside the cell table whatever the caller passed.
static __device__ __forceinline__ int sc_cell(float v, float v0, float s, int n) {
  const int c = (int)floorf((v - v0) / s);
  return c < 0 ? 0 : (c >= n ? n - 1 : c);
}

static __device__ __forceinline__ int sc_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

static __device__ __forceinline__ unsigned long long sc_shfl_xor_u64(unsigned long long v, int o) {
  const unsigned lo = __shfl_xor((unsigned)(v & 0xffffffffu), o), hi = __shfl_xor((unsigned)(v >> 32), o);
  return ((unsigned long long)hi << 32) | lo;
}

// One step of an arg-max (the vote, r3d_scene_merge_sets, the segment pool): class k with value v becomes the best when
// it is the first one or greater than the best so far -- the lowest class wins a tie, a NaN never replaces a value.
static __device__ __forceinline__ void sc_argmax_step(int k, float v, int& best, float& best_v) {
  if (best < 0 || v > best_v) {
    best = k;
    best_v = v;
  }
}

// the workgroup's sum of a per-thread count, valid in thread 0 (red: SC_WAVES ints)
static __device__ __forceinline__ int sc_block_count(int v, int* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();  // red may still be read from the count before
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  int t = 0;
#pragma unroll
  for (int w = 0; w < SC_WAVES; ++w) t += red[w];
  return t;
}

// ------------------------------------------------------------------------------------------------ grids, the sort's workspace
static inline long sc_align(long w) { return (w + 3) & ~3L; }  // 16-byte aligned arrays
static inline int sc_grid_of(long n) { return (int)((n + SC_THREADS - 1) / SC_THREADS); }  // one thread per element
static inline int sc_tiles_of(long n) { return (int)((n + SC_TILE - 1) / SC_TILE); }

// at most SC_COUNT_BLOCKS workgroups that stride over M points
static inline int sc_count_grid(long M) {
  const int g = sc_grid_of(M);
  return g < SC_COUNT_BLOCKS ? g : SC_COUNT_BLOCKS;
}

// radix passes of 8 bits for keys 0 .. key_max
static inline int sc_passes(long key_max) {
  return key_max < 256 ? 1 : (key_max < 65536 ? 2 : (key_max < (1L << 24) ? 3 : 4));
}

// What sc_sort_pairs works in, as word offsets into a workspace.
struct sc_sort_ws {
  long key[2], idx[2];  // ping-pong (key, scan index) pairs
  long hist;            // 256 * n_tiles digit counts, [digit][tile], scanned in place
  long part;            // one partial per SC_TILE words of hist (or of whatever else the caller scans through it)
  int n_tiles;
};

// partials for the scan of the sort's own digit counts, and for scans of up to scan_words that go through the same array
static inline long sc_sort_part_words(long M, long scan_words = 0) {
  const long n_part = sc_tiles_of(256L * sc_tiles_of(M)), n_scan = sc_tiles_of(scan_words);
  return n_part > n_scan ? n_part : n_scan;
}

// Appends the sort's arrays for M points at word o of a layout: the four arrays of the pairs, array_words each, then
// gap_words that belong to the caller (the labelling plan keeps an array of its own there), hist and part_words of
// partials.  -> the offset behind them
static inline long sc_sort_ws_append(sc_sort_ws& W, long o, long M, long array_words, long part_words, long gap_words = 0) {
  W.n_tiles = sc_tiles_of(M);
  W.key[0] = o; o += array_words;
  W.key[1] = o; o += array_words;
  W.idx[0] = o; o += array_words;
  W.idx[1] = o; o += array_words;
  o += gap_words;
  W.hist = o; o += sc_align(256L * W.n_tiles);
  W.part = o; o += sc_align(part_words);
  return o;
}

// ------------------------------------------------------------------------------------------------ argument checks
#define SC_TRY(call)        \
  do {                      \
    const int e_ = (call);  \
    if (e_) return e_;      \
  } while (0)

static inline int sc_check_ld(const char* name, int ld) {
  R3D_REQUIRE(ld >= 3 && ld <= 64, "%s: ld %d (a scan row holds x y z first: 3 .. 64 floats)", name, ld);
  return R3D_OK;
}

static inline int sc_check_points(const char* name, long M) {
  R3D_REQUIRE(M > 0 && M <= R3D_SCENE_MAX_POINTS, "%s: M %ld (1 .. 2^27 points)", name, M);
  return R3D_OK;
}

static inline int sc_check_ws(const char* name, long ws_words, long needed) {
  R3D_REQUIRE(ws_words >= needed, "%s: workspace of %ld words, %ld needed", name, ws_words, needed);
  return R3D_OK;
}

// ------------------------------------------------------------------------------------------------ scene_sort.hip
// a[0 .. n) -> its exclusive scan, in place; part: one word per SC_TILE words of a
R3D_INTERNAL void sc_excl_scan(int* a, long n, int* part, hipStream_t st);

// The M (key, scan index) pairs at W.key[0] / W.idx[0] of ws sorted by the low 8 * passes bits of the key, stable.
// -> which pair holds the result (passes & 1)
R3D_INTERNAL int sc_sort_pairs(int32_t* ws, const sc_sort_ws& W, long M, int passes, hipStream_t st);

// Valid points (x, y, z all finite), their minima and maxima over the first `axes` (2 or 3) coordinates:
// rec[0 .. axes) minima, rec[axes .. 2 axes) maxima, rec[2 axes] the count as int bits, zeros up to 8 words (axes 2) or 16
// (axes 3).  part: (2 axes + 1) * sc_bounds_blocks(M) words.
R3D_INTERNAL int sc_bounds_blocks(long M);
R3D_INTERNAL void sc_bounds(const float* scan, int ld, long M, int axes, float* part, float* rec, hipStream_t st);
