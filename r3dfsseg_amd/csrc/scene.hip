// Labelling a whole scan against a fitted support set: the device side of scene.py (definition: INTEGRATION.md,
// "Labelling a scan").  The reference only scores clouds that were cut out of a room, sampled, min-shifted and given
// their channels on the host (dataloaders/loader.py:100-119); these kernels do that cutting on the device, without a
// random number, and sum the per-chunk logits back onto the scan points:
//   bounds   valid points, their xy extent                               -> an 8-word record the host reads (read 1)
//   plan     cell keys, stable radix sort by key, cell offsets, block sizes, chunk offsets, chunk table
//                                                                        -> a record the host reads (read 2)
//   prepare  the G chunks of one predict launch as prepared clouds, gathered straight from the scan
//   vote     per scan point the sum of its chunk logits (closed-form inverted index: no atomics, a fixed order)
//   run tables (a cap on the chunks of a block: only chunks j < cap run); prepare and vote number the chunks that run
//            through them, and without a cap the plan's own chunk tables stand in for them: the cap nobody reaches
//            (the vote then skips the test against them, which no appearance would fail)
//   transfer scores and labels of the nearest voted point, among the 3 x 3 cells, to every point without a vote; or
//            (idw, when given neighbours and weights) mean logits of the three nearest, weighted by 1 / d
//   support  (fit_scene) per block and way the points of the block's chunk 0 that carry the way's class id; per way the
//            k_shot blocks with most of them; those chunks as prepared clouds with their masks
//   segments (pool_segments) the scores pooled over user-given point segments: the sort below on (id, scan index), per
//            segment the mean of its contributors' mean logits, every point of the segment takes it
//   grow     (build_segments) the segments themselves: the sort below on (voxel key, scan index), the occupied voxels
//            joined to their neighbours in a union-find on integer atomics, the components numbered and spread
// All of it is bandwidth-bound integer and min / max work; the only floating-point sums are the vote's, one running
// sum per (point, class) in a fixed order, the segment pool's, one per (tile, column) and (segment, column), and the
// voxel colours' of grow, in the pool's order.
#include "common.h"

#define SC_THREADS 256
#define SC_TILE 2048                 // points per sort tile, elements per scan block (8 per thread)
#define SC_PER_THREAD (SC_TILE / SC_THREADS)
#define SC_BOUNDS_BLOCKS 1024
#define SC_MAX_CELLS 65536
#define SC_MAX_POINTS (1L << 27)
#define SC_PLAN_THREADS 1024

// record of r3d_scene_bounds (floats, n_valid as int bits)
#define SC_B_X0 0
#define SC_B_Y0 1
#define SC_B_XMAX 2
#define SC_B_YMAX 3
#define SC_B_NVALID 4
// record of r3d_scene_plan (ints)
#define SC_P_NCHUNKS 0
#define SC_P_NBLOCKS 1
#define SC_P_NVOTED 2
// the chunks that run: r3d_scene_plan writes {n_chunks, 0, voted}, r3d_scene_run_tables the counts under its cap
#define SC_P_NRUN 4
#define SC_P_NSKIPPED 5
#define SC_P_NVOTED_RUN 6
// transfer: queries per workgroup (one thread each), candidate rows staged through LDS at a time (16 KiB)
#define SC_Q_TILE 256
#define SC_C_TILE 1024
// record of r3d_scene_transfer (ints, in the sparse workspace)
#define SC_T_NTRANSFERRED 0
#define SC_T_NTILES 1

// ------------------------------------------------------------------------------------------------ workspace layout
struct sc_layout {
  long key[2], idx[2];  // ping-pong (key, scan index) pairs of the sort, M words each
  long pos;             // M: sorted position of every scan point
  long hist;            // 256 * n_tiles digit counts, [digit][tile], scanned in place
  long part;            // one partial per SC_TILE words of hist
  long cell;            // n_cells + 2 cell offsets into the sorted order (cell n_cells: the invalid points)
  long blk_n;           // n_cells: points of a block (n_blocks <= n_cells)
  long chunk0;          // n_cells + 1: first chunk of a block (exclusive scan of the chunk counts)
  long chunk_blk;       // chunk_cap: block of a chunk
  long rec;             // 8
  long total;
  int n_tiles, n_part, passes, sorted;  // sorted: which of the two pairs holds the result
};

static long sc_align(long w) { return (w + 3) & ~3L; }  // 16-byte aligned arrays

static sc_layout sc_make_layout(long M, long n_cells, long chunk_cap) {
  sc_layout L;
  long o = 0;
  const long Ma = sc_align(M);
  L.n_tiles = (int)((M + SC_TILE - 1) / SC_TILE);
  const long n_hist = 256L * L.n_tiles;
  L.n_part = (int)((n_hist + SC_TILE - 1) / SC_TILE);
  L.passes = n_cells < 256 ? 1 : (n_cells < 65536 ? 2 : 3);  // keys run 0 .. n_cells (n_cells: invalid point)
  L.sorted = L.passes & 1;
  L.key[0] = o; o += Ma;
  L.key[1] = o; o += Ma;
  L.idx[0] = o; o += Ma;
  L.idx[1] = o; o += Ma;
  L.pos = o; o += Ma;
  L.hist = o; o += sc_align(n_hist);
  L.part = o; o += sc_align(L.n_part);
  L.cell = o; o += sc_align(n_cells + 2);
  L.blk_n = o; o += sc_align(n_cells);
  L.chunk0 = o; o += sc_align(n_cells + 1);
  L.chunk_blk = o; o += sc_align(chunk_cap);
  L.rec = o; o += 8;
  L.total = o;
  return L;
}

static bool sc_shape_ok(long M, int ncx, int ncy, int r, long chunk_cap) {
  return M > 0 && M <= SC_MAX_POINTS && ncx > 0 && ncy > 0 && (long)ncx * ncy <= SC_MAX_CELLS && r >= 1 && r <= 4 &&
         chunk_cap >= 0 && chunk_cap < (1L << 30);
}

// the second workspace: what a cap on the chunks of a block and the transfer add.  r3d_scene_ws_words and the layout above
// stay as they are, so a caller that uses neither allocates and sees what it always did.
struct sp_layout {
  long run0;     // n_cells + 1: first run chunk of a block (exclusive scan of min(nc, cap))
  long run_blk;  // chunk_cap: block of a run chunk
  long voff;     // M + 1: voted points in front of a sorted position
  long part;     // one partial per SC_TILE words of voff
  long uq;       // M: scan indices of the points without a vote, in sorted order
  long tile0;    // n_cells + 1: first query tile of a cell
  long rec;      // 8
  long cand;     // 4 * M: rows {x, y, z, scan index} of the voted points, in sorted order (16-byte aligned)
  long total;
  int n_part;
};

static sp_layout sp_make_layout(long M, long n_cells, long chunk_cap) {
  sp_layout S;
  long o = 0;
  S.n_part = (int)((M + 1 + SC_TILE - 1) / SC_TILE);
  S.run0 = o; o += sc_align(n_cells + 1);
  S.run_blk = o; o += sc_align(chunk_cap);
  S.voff = o; o += sc_align(M + 1);
  S.part = o; o += sc_align(S.n_part);
  S.uq = o; o += sc_align(M);
  S.tile0 = o; o += sc_align(n_cells + 1);
  S.rec = o; o += 8;
  S.cand = o; o += 4 * M;
  S.total = o;
  return S;
}

// ------------------------------------------------------------------------------------------------ bounds
static __device__ __forceinline__ bool sc_finite3(float x, float y, float z) {
  return isfinite(x) && isfinite(y) && isfinite(z);
}

__global__ __launch_bounds__(SC_THREADS) void r3d_scene_bounds_part_kernel(const float* __restrict__ scan, int ld, int M,
                                                                           float* __restrict__ part) {
  __shared__ float red[5][SC_THREADS / R3D_WAVE];
  float x0 = INFINITY, y0 = INFINITY, x1 = -INFINITY, y1 = -INFINITY;
  int n = 0;
  for (int i = blockIdx.x * SC_THREADS + threadIdx.x; i < M; i += gridDim.x * SC_THREADS) {
    const float* p = scan + (long)i * ld;
    const float x = p[0], y = p[1], z = p[2];
    if (sc_finite3(x, y, z)) {
      x0 = fminf(x0, x); y0 = fminf(y0, y);
      x1 = fmaxf(x1, x); y1 = fmaxf(y1, y);
      ++n;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    x0 = fminf(x0, __shfl_xor(x0, o)); y0 = fminf(y0, __shfl_xor(y0, o));
    x1 = fmaxf(x1, __shfl_xor(x1, o)); y1 = fmaxf(y1, __shfl_xor(y1, o));
    n += __shfl_xor(n, o);
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    red[0][w] = x0; red[1][w] = y0; red[2][w] = x1; red[3][w] = y1; red[4][w] = __int_as_float(n);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < SC_THREADS / R3D_WAVE; ++k) {
      x0 = fminf(x0, red[0][k]); y0 = fminf(y0, red[1][k]);
      x1 = fmaxf(x1, red[2][k]); y1 = fmaxf(y1, red[3][k]);
      n += __float_as_int(red[4][k]);
    }
    float* o = part + 5L * blockIdx.x;
    o[0] = x0; o[1] = y0; o[2] = x1; o[3] = y1; o[4] = __int_as_float(n);
  }
}

__global__ __launch_bounds__(R3D_WAVE) void r3d_scene_bounds_final_kernel(const float* __restrict__ part, int n_part,
                                                                          float* __restrict__ rec) {
  float x0 = INFINITY, y0 = INFINITY, x1 = -INFINITY, y1 = -INFINITY;
  int n = 0;
  for (int i = threadIdx.x; i < n_part; i += R3D_WAVE) {
    const float* p = part + 5L * i;
    x0 = fminf(x0, p[0]); y0 = fminf(y0, p[1]);
    x1 = fmaxf(x1, p[2]); y1 = fmaxf(y1, p[3]);
    n += __float_as_int(p[4]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    x0 = fminf(x0, __shfl_xor(x0, o)); y0 = fminf(y0, __shfl_xor(y0, o));
    x1 = fmaxf(x1, __shfl_xor(x1, o)); y1 = fmaxf(y1, __shfl_xor(y1, o));
    n += __shfl_xor(n, o);
  }
  if (threadIdx.x == 0) {
    rec[SC_B_X0] = x0; rec[SC_B_Y0] = y0; rec[SC_B_XMAX] = x1; rec[SC_B_YMAX] = y1;
    rec[SC_B_NVALID] = __int_as_float(n);
    rec[5] = 0.0f; rec[6] = 0.0f; rec[7] = 0.0f;
  }
}

static int sc_bounds_blocks(long M) {
  const long b = (M + SC_THREADS - 1) / SC_THREADS;
  return (int)(b < SC_BOUNDS_BLOCKS ? b : SC_BOUNDS_BLOCKS);
}

extern "C" long r3d_scene_bounds_ws_words(long M) { return M > 0 ? 5L * sc_bounds_blocks(M) : 0; }

extern "C" int r3d_scene_bounds(const float* scan, int ld, long M, float* rec, float* ws, long ws_words, void* stream) {
  R3D_REQUIRE(scan && rec && ws, "r3d_scene_bounds: null pointer (scan %p, rec %p, ws %p)", (const void*)scan, (void*)rec,
              (void*)ws);
  R3D_REQUIRE(M > 0 && M <= SC_MAX_POINTS, "r3d_scene_bounds: M %ld (1 .. 2^27 points)", M);
  R3D_REQUIRE(ld >= 3 && ld <= 64, "r3d_scene_bounds: ld %d (a scan row holds x y z first: 3 .. 64 floats)", ld);
  R3D_REQUIRE(ws_words >= r3d_scene_bounds_ws_words(M), "r3d_scene_bounds: workspace of %ld words, %ld needed", ws_words,
              r3d_scene_bounds_ws_words(M));
  const int nb = sc_bounds_blocks(M);
  hipLaunchKernelGGL(r3d_scene_bounds_part_kernel, dim3(nb), dim3(SC_THREADS), 0, (hipStream_t)stream, scan, ld, (int)M, ws);
  hipLaunchKernelGGL(r3d_scene_bounds_final_kernel, dim3(1), dim3(R3D_WAVE), 0, (hipStream_t)stream, ws, nb, rec);
  R3D_LAUNCH_CHECK("r3d_scene_bounds");
  return R3D_OK;
}

// ------------------------------------------------------------------------------------------------ cell keys
// (int)floorf((v - v0) / s): an IEEE subtraction and an IEEE division (the build neither contracts nor uses a
// reciprocal).  The clamp never acts on a valid point when the host derived n from the same arithmetic (the
// expression is monotone in v); it keeps a key inside the cell table whatever the caller passed.
static __device__ __forceinline__ int sc_cell(float v, float v0, float s, int n) {
  const int c = (int)floorf((v - v0) / s);
  return c < 0 ? 0 : (c >= n ? n - 1 : c);
}

__global__ __launch_bounds__(SC_THREADS) void r3d_scene_keys_kernel(const float* __restrict__ scan, int ld, int M, float x0,
                                                                    float y0, float s, int ncx, int ncy,
                                                                    int* __restrict__ key, int* __restrict__ idx) {
  const int i = blockIdx.x * SC_THREADS + threadIdx.x;
  if (i >= M) return;
  const float* p = scan + (long)i * ld;
  const float x = p[0], y = p[1], z = p[2];
  int k = ncx * ncy;  // invalid points sort behind every cell
  if (sc_finite3(x, y, z)) k = sc_cell(y, y0, s, ncy) * ncx + sc_cell(x, x0, s, ncx);
  key[i] = k;
  idx[i] = i;
}

// ------------------------------------------------------------------------------------------------ radix sort
// LSD passes of 8 bits over (key, scan index) pairs.  Pass: per-tile digit counts [digit][tile]; one exclusive scan
// over that table gives every (digit, tile) its first output position; the scatter ranks the elements of a tile
// with the same digit in index order, which keeps the sort stable.
__global__ __launch_bounds__(SC_THREADS) void r3d_scene_hist_kernel(const int* __restrict__ key, int M, int shift, int n_tiles,
                                                                    int* __restrict__ hist) {
  __shared__ int cnt[256];
  const int t = blockIdx.x;
  cnt[threadIdx.x] = 0;
  __syncthreads();
  const int base = t * SC_TILE;
#pragma unroll
  for (int k = 0; k < SC_PER_THREAD; ++k) {
    const int i = base + k * SC_THREADS + threadIdx.x;
    if (i < M) atomicAdd(&cnt[(key[i] >> shift) & 255], 1);  // integer counts in LDS: order-independent
  }
  __syncthreads();
  hist[(long)threadIdx.x * n_tiles + t] = cnt[threadIdx.x];
}

// in-place exclusive scan of a[0 .. n) in three launches: sums of SC_TILE-word blocks, scan of the sums, local scans
__global__ __launch_bounds__(SC_THREADS) void r3d_scene_scan_sum_kernel(const int* __restrict__ a, long n,
                                                                        int* __restrict__ part) {
  __shared__ int wsum[SC_THREADS / R3D_WAVE];
  const long base = (long)blockIdx.x * SC_TILE + (long)threadIdx.x * SC_PER_THREAD;
  int v = 0;
#pragma unroll
  for (int k = 0; k < SC_PER_THREAD; ++k)
    if (base + k < n) v += a[base + k];
  int total;
  r3d_block_excl_scan<SC_THREADS>(v, wsum, total);
  if (threadIdx.x == 0) part[blockIdx.x] = total;
}

__global__ __launch_bounds__(SC_PLAN_THREADS) void r3d_scene_scan_part_kernel(int* __restrict__ part, int n) {
  __shared__ int wsum[SC_PLAN_THREADS / R3D_WAVE];
  int carry = 0;
  for (int b = 0; b < n; b += SC_PLAN_THREADS) {
    const int i = b + threadIdx.x;
    const int v = i < n ? part[i] : 0;
    int total;
    const int ex = r3d_block_excl_scan<SC_PLAN_THREADS>(v, wsum, total);
    if (i < n) part[i] = carry + ex;
    carry += total;
  }
}

__global__ __launch_bounds__(SC_THREADS) void r3d_scene_scan_local_kernel(int* __restrict__ a, long n,
                                                                          const int* __restrict__ part) {
  __shared__ int wsum[SC_THREADS / R3D_WAVE];
  const long base = (long)blockIdx.x * SC_TILE + (long)threadIdx.x * SC_PER_THREAD;
  int e[SC_PER_THREAD];
  int v = 0;
#pragma unroll
  for (int k = 0; k < SC_PER_THREAD; ++k) {
    e[k] = base + k < n ? a[base + k] : 0;
    v += e[k];
  }
  int total;
  int run = part[blockIdx.x] + r3d_block_excl_scan<SC_THREADS>(v, wsum, total);
#pragma unroll
  for (int k = 0; k < SC_PER_THREAD; ++k) {
    if (base + k < n) a[base + k] = run;
    run += e[k];
  }
}

__global__ __launch_bounds__(SC_THREADS) void r3d_scene_scatter_kernel(const int* __restrict__ key_in,
                                                                       const int* __restrict__ idx_in, int M, int shift,
                                                                       int n_tiles, const int* __restrict__ offs,
                                                                       int* __restrict__ key_out, int* __restrict__ idx_out) {
  __shared__ int base[256];                           // next output position of a digit in this tile
  __shared__ int wcnt[SC_THREADS / R3D_WAVE][256];    // elements of a digit per wave in the current round
  const int t = blockIdx.x, tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  base[tid] = offs[(long)tid * n_tiles + t];
  const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  for (int k = 0; k < SC_PER_THREAD; ++k) {
    for (int j = tid; j < (SC_THREADS / R3D_WAVE) * 256; j += SC_THREADS) (&wcnt[0][0])[j] = 0;
    __syncthreads();
    const int i = t * SC_TILE + k * SC_THREADS + tid;
    const bool live = i < M;
    const int ky = live ? key_in[i] : 0, id = live ? idx_in[i] : 0;
    const int d = (ky >> shift) & 255;
    // lanes of this wave with the same digit
    unsigned long long peers = __ballot(live);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1;
      const unsigned long long m = __ballot(bit);
      peers &= bit ? m : ~m;
    }
    const int rank = __popcll(peers & below);
    if (live && rank == 0) wcnt[w][d] = __popcll(peers);  // one writer per (wave, digit)
    __syncthreads();
    if (live) {
      int o = base[d] + rank;
      for (int q = 0; q < w; ++q) o += wcnt[q][d];
      // offsets come from counts of these very keys, so o < M; the guard only matters for a corrupted table
      if (o >= 0 && o < M) {
        key_out[o] = ky;
        idx_out[o] = id;
      }
    }
    __syncthreads();
    int add = 0;
#pragma unroll
    for (int q = 0; q < SC_THREADS / R3D_WAVE; ++q) add += wcnt[q][tid];
    base[tid] += add;
    __syncthreads();
  }
}

// a[0 .. n) -> its exclusive scan, in place; part: one word per SC_TILE words of a
static void sc_excl_scan(int* a, long n, int* part, hipStream_t st) {
  const int nb = (int)((n + SC_TILE - 1) / SC_TILE);
  hipLaunchKernelGGL(r3d_scene_scan_sum_kernel, dim3(nb), dim3(SC_THREADS), 0, st, a, n, part);
  hipLaunchKernelGGL(r3d_scene_scan_part_kernel, dim3(1), dim3(SC_PLAN_THREADS), 0, st, part, nb);
  hipLaunchKernelGGL(r3d_scene_scan_local_kernel, dim3(nb), dim3(SC_THREADS), 0, st, a, n, part);
}

// The M (key, scan index) pairs at key[0] / idx[0] sorted by the low 8 * passes bits of the key; key, idx, hist and part
// are word offsets into ws (hist: 256 * n_tiles words, part: one per SC_TILE of them).  -> which pair holds the result.
static int sc_sort_pairs(int32_t* ws, const long key[2], const long idx[2], long hist, long part, long M, int n_tiles,
                         int passes, hipStream_t st) {
  for (int p = 0; p < passes; ++p) {
    const int a = p & 1, b = a ^ 1;
    hipLaunchKernelGGL(r3d_scene_hist_kernel, dim3(n_tiles), dim3(SC_THREADS), 0, st, ws + key[a], (int)M, 8 * p, n_tiles,
                       ws + hist);
    sc_excl_scan(ws + hist, 256L * n_tiles, ws + part, st);
    hipLaunchKernelGGL(r3d_scene_scatter_kernel, dim3(n_tiles), dim3(SC_THREADS), 0, st, ws + key[a], ws + idx[a], (int)M, 8 * p,
                       n_tiles, ws + hist, ws + key[b], ws + idx[b]);
  }
  return passes & 1;
}

// cell offsets from the sorted keys (every cell written by exactly one thread, empty cells included) and the sorted
// position of every scan point
__global__ __launch_bounds__(SC_THREADS) void r3d_scene_cells_kernel(const int* __restrict__ skey, const int* __restrict__ order,
                                                                     int M, int n_cells, int* __restrict__ cell,
                                                                     int* __restrict__ pos) {
  const int i = blockIdx.x * SC_THREADS + threadIdx.x;
  if (i >= M) return;
  int k = skey[i];
  k = k < 0 ? 0 : (k > n_cells ? n_cells : k);
  const int kp = i > 0 ? skey[i - 1] : -1;
  for (int c = (kp < -1 ? -1 : kp) + 1; c <= k; ++c) cell[c] = i;
  if (i == M - 1)
    for (int c = k + 1; c <= n_cells + 1; ++c) cell[c] = M;
  const int p = order[i];
  if (p >= 0 && p < M) pos[p] = i;
}

// ------------------------------------------------------------------------------------------------ blocks and chunks
struct sc_grid {
  int ncx, ncy, r, nbx, nby, M;
};

// points of block (bx, by) in front of row `row` of its cells (row = rows of the block: all of them), and the
// sorted position at which that row's run of cells starts
static __device__ __forceinline__ int sc_row_start(const int* __restrict__ cell, const sc_grid& g, int bx, int cy) {
  return cell[cy * g.ncx + bx];
}
static __device__ __forceinline__ int sc_row_end(const int* __restrict__ cell, const sc_grid& g, int bx, int cy) {
  const int ex = bx + g.r < g.ncx ? bx + g.r : g.ncx;
  return cell[cy * g.ncx + ex];
}
static __device__ __forceinline__ int sc_block_rows(const sc_grid& g, int by) {
  return (by + g.r < g.ncy ? by + g.r : g.ncy) - by;
}

// one workgroup: block sizes, chunk counts and their exclusive scan; kept blocks; valid points with a vote
__global__ __launch_bounds__(SC_PLAN_THREADS) void r3d_scene_blocks_kernel(const int* __restrict__ cell, sc_grid g, int N,
                                                                           int min_points, int* __restrict__ blk_n,
                                                                           int* __restrict__ chunk0, int* __restrict__ rec) {
  __shared__ int wsum[SC_PLAN_THREADS / R3D_WAVE];
  __shared__ int kept, voted;
  if (threadIdx.x == 0) kept = voted = 0;
  __syncthreads();
  const int nb = g.nbx * g.nby;
  int carry = 0;
  for (int b0 = 0; b0 < nb; b0 += SC_PLAN_THREADS) {
    const int b = b0 + threadIdx.x;
    int n = 0, nc = 0;
    if (b < nb) {
      const int bx = b % g.nbx, by = b / g.nbx, rows = sc_block_rows(g, by);
      for (int k = 0; k < rows; ++k) n += sc_row_end(cell, g, bx, by + k) - sc_row_start(cell, g, bx, by + k);
      if (n >= min_points) nc = (n + N - 1) / N;
      blk_n[b] = n;
      if (nc > 0) atomicAdd(&kept, 1);
    }
    int total;
    const int ex = r3d_block_excl_scan<SC_PLAN_THREADS>(nc, wsum, total);
    if (b < nb) chunk0[b] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) chunk0[nb] = carry;
  __syncthreads();  // chunk0 of every block is visible to the workgroup
  const int n_cells = g.ncx * g.ncy;
  for (int c = threadIdx.x; c < n_cells; c += SC_PLAN_THREADS) {
    const int cx = c % g.ncx, cy = c / g.ncx;
    bool any = false;
    for (int by = cy - g.r + 1 > 0 ? cy - g.r + 1 : 0; by <= cy && by < g.nby; ++by)
      for (int bx = cx - g.r + 1 > 0 ? cx - g.r + 1 : 0; bx <= cx && bx < g.nbx; ++bx) {
        const int b = by * g.nbx + bx;
        any = any || chunk0[b + 1] > chunk0[b];
      }
    if (any) atomicAdd(&voted, cell[c + 1] - cell[c]);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    rec[SC_P_NCHUNKS] = carry;
    rec[SC_P_NBLOCKS] = kept;
    rec[SC_P_NVOTED] = voted;
    rec[3] = nb;
    rec[SC_P_NRUN] = carry;  // without a cap every chunk runs
    rec[SC_P_NSKIPPED] = 0;
    rec[SC_P_NVOTED_RUN] = voted;
    rec[7] = 0;
  }
}

__global__ __launch_bounds__(SC_THREADS) void r3d_scene_chunk_table_kernel(const int* __restrict__ chunk0, int nb, int chunk_cap,
                                                                           int* __restrict__ chunk_blk) {
  const int b = blockIdx.x * SC_THREADS + threadIdx.x;
  if (b >= nb) return;
  const int c0 = chunk0[b], c1 = chunk0[b + 1];
  for (int c = c0; c < c1 && c < chunk_cap; ++c) chunk_blk[c] = b;
}

extern "C" long r3d_scene_ws_words(long M, int ncx, int ncy, long chunk_cap) {
  if (!sc_shape_ok(M, ncx, ncy, 1, chunk_cap)) return -1;
  return sc_make_layout(M, (long)ncx * ncy, chunk_cap).total;
}

extern "C" long r3d_scene_sparse_ws_words(long M, int ncx, int ncy, long chunk_cap) {
  if (!sc_shape_ok(M, ncx, ncy, 1, chunk_cap)) return -1;
  return sp_make_layout(M, (long)ncx * ncy, chunk_cap).total;
}

extern "C" int r3d_scene_sparse_ws_offsets(long M, int ncx, int ncy, long chunk_cap, long* out /* 8 HOST words */) {
  R3D_REQUIRE(out, "r3d_scene_sparse_ws_offsets: null pointer");
  R3D_REQUIRE(sc_shape_ok(M, ncx, ncy, 1, chunk_cap), "r3d_scene_sparse_ws_offsets: M %ld, cells %d x %d, chunk_cap %ld out of range",
              M, ncx, ncy, chunk_cap);
  const sp_layout S = sp_make_layout(M, (long)ncx * ncy, chunk_cap);
  out[0] = S.run0; out[1] = S.run_blk; out[2] = S.voff; out[3] = S.uq;
  out[4] = S.tile0; out[5] = S.cand; out[6] = S.rec; out[7] = S.part;
  return R3D_OK;
}

extern "C" int r3d_scene_ws_offsets(long M, int ncx, int ncy, long chunk_cap, long* out /* 8 HOST words */) {
  R3D_REQUIRE(out, "r3d_scene_ws_offsets: null pointer");
  R3D_REQUIRE(sc_shape_ok(M, ncx, ncy, 1, chunk_cap), "r3d_scene_ws_offsets: M %ld, cells %d x %d, chunk_cap %ld out of range", M,
              ncx, ncy, chunk_cap);
  const sc_layout L = sc_make_layout(M, (long)ncx * ncy, chunk_cap);
  out[0] = L.idx[L.sorted]; out[1] = L.key[L.sorted]; out[2] = L.pos; out[3] = L.cell;
  out[4] = L.blk_n; out[5] = L.chunk0; out[6] = L.chunk_blk; out[7] = L.rec;
  return R3D_OK;
}

// ------------------------------------------------------------------------------------------------ argument checks, the plan on the host
#define SC_TRY(call)        \
  do {                      \
    const int e_ = (call);  \
    if (e_) return e_;      \
  } while (0)

// what every entry point that works on a plan has: the scan's size, the cells and the workspace
static int sc_check_plan(const char* name, long M, int ncx, int ncy, long chunk_cap, long ws_words) {
  R3D_REQUIRE(M > 0 && M <= SC_MAX_POINTS, "%s: M %ld (1 .. 2^27 points)", name, M);
  R3D_REQUIRE(ncx > 0 && ncy > 0 && (long)ncx * ncy <= SC_MAX_CELLS, "%s: %d x %d cells (1 .. 65536)", name, ncx, ncy);
  R3D_REQUIRE(chunk_cap > 0 && chunk_cap < (1L << 30), "%s: chunk_cap %ld", name, chunk_cap);
  R3D_REQUIRE(ws_words >= r3d_scene_ws_words(M, ncx, ncy, chunk_cap), "%s: workspace of %ld words, %ld needed", name, ws_words,
              r3d_scene_ws_words(M, ncx, ncy, chunk_cap));
  return R3D_OK;
}

static int sc_check_ld(const char* name, int ld) {
  R3D_REQUIRE(ld >= 3 && ld <= 64, "%s: ld %d (a scan row holds x y z first: 3 .. 64 floats)", name, ld);
  return R3D_OK;
}

static int sc_check_blocks(const char* name, int r, int N) {
  R3D_REQUIRE(r >= 1 && r <= 4, "%s: r %d (block_size / stride is 1 .. 4)", name, r);
  R3D_REQUIRE(N > 0 && N <= (1 << 20), "%s: N %d points per cloud", name, N);
  return R3D_OK;
}

static int sc_check_sparse_ws(const char* name, long M, int ncx, int ncy, long chunk_cap, long sws_words) {
  R3D_REQUIRE(sc_shape_ok(M, ncx, ncy, 1, chunk_cap) && sws_words >= r3d_scene_sparse_ws_words(M, ncx, ncy, chunk_cap),
              "%s: sparse workspace of %ld words, %ld needed", name, sws_words, r3d_scene_sparse_ws_words(M, ncx, ncy, chunk_cap));
  return R3D_OK;
}

// the optional sws of prepare and vote: NULL with 0 words (no cap), or a whole sparse workspace
static int sc_check_optional_sparse_ws(const char* name, long M, int ncx, int ncy, long chunk_cap, const int32_t* sws,
                                       long sws_words) {
  R3D_REQUIRE(sws || sws_words == 0, "%s: null pointer (sws) with sws_words %ld", name, sws_words);
  return sws ? sc_check_sparse_ws(name, M, ncx, ncy, chunk_cap, sws_words) : R3D_OK;
}

// What the entry points after r3d_scene_plan read, as pointers into ws (and sws); L and S for the arrays they write.
struct sc_view {
  const int *order, *skey, *pos, *cell, *blk_n, *chunk0, *run0, *run_blk, *rec;
  sc_grid g;
  int n_cells, nb;
  sc_layout L;
  sp_layout S;
};

static sc_view sc_make_view(long M, int ncx, int ncy, int r, long chunk_cap, const int32_t* ws, const int32_t* sws) {
  sc_view v;
  v.n_cells = ncx * ncy;
  v.L = sc_make_layout(M, v.n_cells, chunk_cap);
  v.S = sp_make_layout(M, v.n_cells, chunk_cap);
  v.g.ncx = ncx; v.g.ncy = ncy; v.g.r = r; v.g.M = (int)M;
  v.g.nbx = ncx - r + 1 > 1 ? ncx - r + 1 : 1;
  v.g.nby = ncy - r + 1 > 1 ? ncy - r + 1 : 1;
  v.nb = v.g.nbx * v.g.nby;
  v.order = ws + v.L.idx[v.L.sorted];
  v.skey = ws + v.L.key[v.L.sorted];
  v.pos = ws + v.L.pos;
  v.cell = ws + v.L.cell;
  v.blk_n = ws + v.L.blk_n;
  v.chunk0 = ws + v.L.chunk0;
  v.rec = ws + v.L.rec;
  // Without sws no cap: the chunk tables under a second name (the plan record counts every chunk as a run chunk).  The
  // prepare kernel takes both names as const __restrict__ pointers and only reads through them, which is well defined.
  v.run0 = sws ? sws + v.S.run0 : v.chunk0;
  v.run_blk = sws ? sws + v.S.run_blk : ws + v.L.chunk_blk;
  return v;
}

extern "C" int r3d_scene_plan(const float* scan, int ld, long M, float x0, float y0, float s, int ncx, int ncy, int r, int N,
                              int min_points, long chunk_cap, int32_t* ws, long ws_words, void* stream) {
  R3D_REQUIRE(scan && ws, "r3d_scene_plan: null pointer (scan %p, ws %p)", (const void*)scan, (void*)ws);
  SC_TRY(sc_check_ld("r3d_scene_plan", ld));
  SC_TRY(sc_check_plan("r3d_scene_plan", M, ncx, ncy, chunk_cap, ws_words));
  SC_TRY(sc_check_blocks("r3d_scene_plan", r, N));
  R3D_REQUIRE(min_points >= 1, "r3d_scene_plan: min_points %d (at least 1)", min_points);
  R3D_REQUIRE(x0 == x0 && y0 == y0 && s > 0.0f && s < INFINITY, "r3d_scene_plan: origin (%g, %g), cell size %g", (double)x0,
              (double)y0, (double)s);
  const hipStream_t st = (hipStream_t)stream;
  const sc_view v = sc_make_view(M, ncx, ncy, r, chunk_cap, ws, nullptr);
  const sc_layout& L = v.L;
  const int gm = (int)((M + SC_THREADS - 1) / SC_THREADS);
  hipLaunchKernelGGL(r3d_scene_keys_kernel, dim3(gm), dim3(SC_THREADS), 0, st, scan, ld, (int)M, x0, y0, s, ncx, ncy,
                     ws + L.key[0], ws + L.idx[0]);
  sc_sort_pairs(ws, L.key, L.idx, L.hist, L.part, M, L.n_tiles, L.passes, st);  // into pair L.sorted: v.skey, v.order
  hipLaunchKernelGGL(r3d_scene_cells_kernel, dim3(gm), dim3(SC_THREADS), 0, st, v.skey, v.order, (int)M, v.n_cells, ws + L.cell,
                     ws + L.pos);
  hipLaunchKernelGGL(r3d_scene_blocks_kernel, dim3(1), dim3(SC_PLAN_THREADS), 0, st, v.cell, v.g, N, min_points, ws + L.blk_n,
                     ws + L.chunk0, ws + L.rec);
  hipLaunchKernelGGL(r3d_scene_chunk_table_kernel, dim3((v.nb + SC_THREADS - 1) / SC_THREADS), dim3(SC_THREADS), 0, st, v.chunk0,
                     v.nb, (int)chunk_cap, ws + L.chunk_blk);
  R3D_LAUNCH_CHECK("r3d_scene_plan");
  return R3D_OK;
}

// ------------------------------------------------------------------------------------------------ prepared clouds
// what a chunk is: block b with n points, chunk j of nc; its members are list positions j, j + nc, ...
struct sc_chunk {
  int bx, by, n, nc, j, len;
};

// list position q of block (bx, by) -> sorted position (the block's list is its rows of cells, one run each)
static __device__ __forceinline__ int sc_list_to_sorted(const int* __restrict__ cell, const sc_grid& g, int bx, int by, int q) {
  const int rows = sc_block_rows(g, by);
  int s = 0;
  for (int k = 0; k < rows; ++k) {
    const int a = sc_row_start(cell, g, bx, by + k), e = sc_row_end(cell, g, bx, by + k);
    if (q < e - a || k == rows - 1) {
      s = a + q;
      break;
    }
    q -= e - a;
  }
  return s < 0 ? 0 : (s >= g.M ? g.M - 1 : s);  // inside the sorted order whatever the tables hold
}

// one workgroup per chunk.  Pass 1: minima and maxima of xyz over the N slots; pass 2: gather again, write.
// blocks (r3d_scene_prepare_blocks): workgroup i prepares chunk 0 of block blocks[i] instead of a numbered chunk; with
// labels (element type L), cloud_class and mask: mask[i][t] = the label of slot t's point equals cloud_class[i].
template <typename L>
__global__ __launch_bounds__(SC_THREADS) void r3d_scene_prepare_kernel(
    const float* __restrict__ scan, int ld, int M, const int* __restrict__ order, const int* __restrict__ cell,
    const int* __restrict__ blk_n, const int* __restrict__ chunk0, const int* __restrict__ rec, sc_grid g, int first_chunk,
    int N, int C, int rgb_ch, int XYZ_ch, float* __restrict__ out, long o_sb, long o_sc, long o_sn,
    int* __restrict__ slot_map, const int* __restrict__ run0, const int* __restrict__ run_blk,
    const int* __restrict__ blocks, const L* __restrict__ labels, const int* __restrict__ cloud_class,
    int* __restrict__ mask) {
  __shared__ float red[6][SC_THREADS / R3D_WAVE];
  const int c = first_chunk + blockIdx.x, tid = threadIdx.x;
  // c numbers the chunks that run (run0 / run_blk; without a cap: all of them); the chunk itself is (b, j) of nc as ever
  if (!blocks && c >= rec[SC_P_NRUN]) return;  // (uniform) a launch past the plan's chunks writes nothing
  const int b = blocks ? blocks[blockIdx.x] : run_blk[c];
  if (b < 0 || b >= g.nbx * g.nby) return;
  const int bx = b % g.nbx, by = b / g.nbx;
  const int n = blk_n[b], nc = chunk0[b + 1] - chunk0[b], j = blocks ? 0 : c - run0[b];
  if (nc <= 0 || j < 0 || j >= nc || n <= j) return;
  const int len = (n - j + nc - 1) / nc;
  out += (long)blockIdx.x * o_sb;

  float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  const int members = len < N ? len : N;  // slots 0 .. members - 1 hold every member once
  for (int t = tid; t < members; t += SC_THREADS) {
    int p = order[sc_list_to_sorted(cell, g, bx, by, j + t * nc)];
    p = p < 0 ? 0 : (p >= M ? M - 1 : p);
    const float* q = scan + (long)p * ld;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      mn[a] = fminf(mn[a], q[a]);
      mx[a] = fmaxf(mx[a], q[a]);
    }
  }
  float lo[3], ext[3];
  r3d_prep_extent<SC_THREADS>(mn, mx, red, lo, ext);

  for (int t = tid; t < N; t += SC_THREADS) {
    int p = order[sc_list_to_sorted(cell, g, bx, by, j + (t % len) * nc)];
    p = p < 0 ? 0 : (p >= M ? M - 1 : p);
    const float* q = scan + (long)p * ld;
    r3d_prep_slot(q, lo, ext, rgb_ch, XYZ_ch, out + (long)t * o_sn, o_sc);
    if (slot_map) slot_map[(long)blockIdx.x * N + t] = p;
    if (mask) mask[(long)blockIdx.x * N + t] = (long long)labels[p] == (long long)cloud_class[blockIdx.x] ? 1 : 0;
  }
}

// what r3d_scene_prepare_blocks adds to the argument list: a device list of G block ids and, optionally, the labels
struct sc_block_args {
  const int32_t* blocks;
  const void* labels;
  int label_bytes;
  const int32_t* cloud_class;
  int32_t* mask;
};

// r3d_scene_prepare and r3d_scene_prepare_blocks (ba): one argument list, one launch
static int sc_prepare(const float* scan, int ld, long M, int ncx, int ncy, int r, int N, long chunk_cap, const int32_t* ws,
                      long ws_words, const int32_t* sws, int first_chunk, int G, int C, int rgb_ch, int XYZ_ch, float* out,
                      long o_sb, long o_sc, long o_sn, int32_t* slot_map, void* stream, const sc_block_args* ba = nullptr) {
  R3D_REQUIRE(scan && ws && out, "r3d_scene_prepare: null pointer (scan %p, ws %p, out %p)", (const void*)scan, (const void*)ws,
              (void*)out);
  SC_TRY(sc_check_ld("r3d_scene_prepare", ld));
  SC_TRY(sc_check_plan("r3d_scene_prepare", M, ncx, ncy, chunk_cap, ws_words));
  SC_TRY(sc_check_blocks("r3d_scene_prepare", r, N));
  R3D_REQUIRE(G > 0 && first_chunk >= 0 && (ba || (long)first_chunk + G <= chunk_cap),  // ba: G block ids, checked by the caller
              "r3d_scene_prepare: chunks %d .. %d + %d outside the chunk table of %ld", first_chunk, first_chunk, G, chunk_cap);
  R3D_REQUIRE(C == 3 || C == 6 || C == 9, "r3d_scene_prepare: C %d (3, 6 or 9 channels)", C);
  R3D_REQUIRE(rgb_ch == -1 || rgb_ch == 3, "r3d_scene_prepare: rgb_ch %d (3, or -1: none)", rgb_ch);
  R3D_REQUIRE(rgb_ch == -1 || ld >= 6, "r3d_scene_prepare: a scan row of %d floats has no colour", ld);
  R3D_REQUIRE(XYZ_ch == -1 || XYZ_ch == (rgb_ch == 3 ? 6 : 3), "r3d_scene_prepare: XYZ_ch %d (behind xyz and rgb, or -1: none)",
              XYZ_ch);
  R3D_REQUIRE(C == 3 + (rgb_ch >= 0 ? 3 : 0) + (XYZ_ch >= 0 ? 3 : 0), "r3d_scene_prepare: C %d does not hold xyz%s%s", C,
              rgb_ch >= 0 ? " rgb" : "", XYZ_ch >= 0 ? " XYZ" : "");
  R3D_REQUIRE(o_sb >= 0 && o_sc > 0 && o_sn > 0, "r3d_scene_prepare: strides must be positive (out %ld %ld %ld)", o_sb, o_sc, o_sn);
  const sc_view v = sc_make_view(M, ncx, ncy, r, chunk_cap, ws, sws);
#define SC_LAUNCH_PREPARE(T)                                                                                                  \
  hipLaunchKernelGGL(r3d_scene_prepare_kernel<T>, dim3(G), dim3(SC_THREADS), 0, (hipStream_t)stream, scan, ld, (int)M, v.order,   \
                     v.cell, v.blk_n, v.chunk0, v.rec, v.g, first_chunk, N, C, rgb_ch, XYZ_ch, out, o_sb, o_sc, o_sn, slot_map,   \
                     v.run0, v.run_blk, ba ? ba->blocks : nullptr, (const T*)(ba ? ba->labels : nullptr),                         \
                     ba ? ba->cloud_class : nullptr, ba ? ba->mask : nullptr)
  if (ba && ba->label_bytes == 8)
    SC_LAUNCH_PREPARE(long long);
  else
    SC_LAUNCH_PREPARE(int);
#undef SC_LAUNCH_PREPARE
  R3D_LAUNCH_CHECK("r3d_scene_prepare");
  return R3D_OK;
}

extern "C" int r3d_scene_prepare(const float* scan, int ld, long M, int ncx, int ncy, int r, int N, long chunk_cap,
                                 const int32_t* ws, long ws_words, const int32_t* sws, long sws_words, int first_chunk, int G,
                                 int C, int rgb_ch, int XYZ_ch, float* out, long o_sb, long o_sc, long o_sn, int32_t* slot_map,
                                 void* stream) {
  SC_TRY(sc_check_optional_sparse_ws("r3d_scene_prepare", M, ncx, ncy, chunk_cap, sws, sws_words));
  return sc_prepare(scan, ld, M, ncx, ncy, r, N, chunk_cap, ws, ws_words, sws, first_chunk, G, C, rgb_ch, XYZ_ch, out, o_sb,
                    o_sc, o_sn, slot_map, stream);
}

// ------------------------------------------------------------------------------------------------ votes
// One thread per scan point.  Its appearances follow from its cell, its rank in the cell list and the block's row
// offsets: list position q in block (bx, by) -> chunk q % nc, member q / nc, slots member, member + len, ... < N.
// Blocks by ascending id (by, then bx), slots ascending, one running fp32 sum per class: a fixed order, no atomics.

// One step of the arg-max of the vote and of the merge (r3d_scene_merge_sets): class k with value v becomes the best when
// it is the first one or greater than the best so far -- the lowest class wins a tie, a NaN never replaces a value.
static __device__ __forceinline__ void sc_argmax_step(int k, float v, int& best, float& best_v) {
  if (best < 0 || v > best_v) {
    best = k;
    best_v = v;
  }
}

__global__ __launch_bounds__(SC_THREADS) void r3d_scene_vote_kernel(
    int M, const int* __restrict__ skey, const int* __restrict__ pos, const int* __restrict__ cell,
    const int* __restrict__ blk_n, const int* __restrict__ chunk0, sc_grid g, int N, int K, const float* __restrict__ logits,
    int n_chunks, float* __restrict__ scores, long long* __restrict__ labels, int* __restrict__ votes,
    const int* __restrict__ run0) {
  const int p = blockIdx.x * SC_THREADS + threadIdx.x;
  if (p >= M) return;
  const int n_cells = g.ncx * g.ncy;
  const int sp = pos[p];
  const int key = (sp >= 0 && sp < M) ? skey[sp] : n_cells;
  int n_votes = 0, best = -1;
  float best_v = 0.0f;
  const bool valid = key >= 0 && key < n_cells;
  const int cx = valid ? key % g.ncx : 0, cy = valid ? key / g.ncx : 0;
  const int by0 = cy - g.r + 1 > 0 ? cy - g.r + 1 : 0, bx0 = cx - g.r + 1 > 0 ? cx - g.r + 1 : 0;
  for (int k = 0; k < K; ++k) {
    float acc = 0.0f;
    int cnt = 0;
    if (valid) {
      for (int by = by0; by <= cy && by < g.nby; ++by)
        for (int bx = bx0; bx <= cx && bx < g.nbx; ++bx) {
          const int b = by * g.nbx + bx;
          const int c0 = chunk0[b], nc = chunk0[b + 1] - c0;
          if (nc <= 0) continue;  // dropped block
          int q = sp - sc_row_start(cell, g, bx, cy);  // position inside its row of the block
          for (int row = by; row < cy; ++row) q += sc_row_end(cell, g, bx, row) - sc_row_start(cell, g, bx, row);
          const int n = blk_n[b], j = q % nc, m = q / nc;
          const int len = (n - j + nc - 1) / nc;
          int ch = c0 + j;
          // under a cap: the appearance counts when its chunk ran; logits are numbered by run chunk.  Reading chunk0 as
          // run0 without a cap gives the same bits, but the kernel without this (uniform) branch took 3 % longer at 10^6
          // points (profiles/r21_scene_one_entry_point.md): the vote alone is given run0 == NULL for "no cap".
          if (run0) {
            if (j >= run0[b + 1] - run0[b]) continue;
            ch = run0[b] + j;
          }
          if (q < 0 || q >= n || len <= 0 || ch >= n_chunks) continue;
          const float* z = logits + ((long)ch * K + k) * N;
          for (int t = m; t < N; t += len) {
            acc += z[t];
            ++cnt;
          }
        }
    }
    scores[(long)p * K + k] = acc;
    if (k == 0) n_votes = cnt;
    if (cnt > 0) sc_argmax_step(k, acc, best, best_v);
  }
  votes[p] = n_votes;
  labels[p] = best;
}

extern "C" int r3d_scene_vote(long M, int ncx, int ncy, int r, int N, long chunk_cap, const int32_t* ws, long ws_words,
                              const int32_t* sws, long sws_words, const float* logits, int n_chunks, int n_classes,
                              float* scores, int64_t* labels, int32_t* votes, void* stream) {
  SC_TRY(sc_check_optional_sparse_ws("r3d_scene_vote", M, ncx, ncy, chunk_cap, sws, sws_words));
  R3D_REQUIRE(ws && logits && scores && labels && votes,
              "r3d_scene_vote: null pointer (ws %p, logits %p, scores %p, labels %p, votes %p)", (const void*)ws,
              (const void*)logits, (void*)scores, (void*)labels, (void*)votes);
  SC_TRY(sc_check_plan("r3d_scene_vote", M, ncx, ncy, chunk_cap, ws_words));
  SC_TRY(sc_check_blocks("r3d_scene_vote", r, N));
  R3D_REQUIRE(n_chunks > 0 && n_chunks <= chunk_cap, "r3d_scene_vote: n_chunks %d (1 .. chunk_cap %ld)", n_chunks, chunk_cap);
  R3D_REQUIRE(n_classes >= 1 && n_classes <= 64, "r3d_scene_vote: n_classes %d (1 .. 64)", n_classes);
  const sc_view v = sc_make_view(M, ncx, ncy, r, chunk_cap, ws, sws);
  hipLaunchKernelGGL(r3d_scene_vote_kernel, dim3((int)((M + SC_THREADS - 1) / SC_THREADS)), dim3(SC_THREADS), 0,
                     (hipStream_t)stream, (int)M, v.skey, v.pos, v.cell, v.blk_n, v.chunk0, v.g, N, n_classes, logits, n_chunks,
                     scores, (long long*)labels, votes, sws ? v.run0 : nullptr);
  R3D_LAUNCH_CHECK("r3d_scene_vote");
  return R3D_OK;
}

// ------------------------------------------------------------------------------------------------ a cap on the chunks of a block
// With cap c, chunk j of a block with nc chunks runs when j < c; run chunks are numbered by block id, then j.  One
// workgroup: the exclusive scan of min(nc, c) over the blocks, and the counts for the plan record.
__global__ __launch_bounds__(SC_PLAN_THREADS) void r3d_scene_run_scan_kernel(const int* __restrict__ chunk0, int nb, int cap,
                                                                             int* __restrict__ run0, int* __restrict__ rec) {
  __shared__ int wsum[SC_PLAN_THREADS / R3D_WAVE];
  int carry = 0;
  for (int b0 = 0; b0 < nb; b0 += SC_PLAN_THREADS) {
    const int b = b0 + threadIdx.x;
    int rc = 0;
    if (b < nb) {
      const int nc = chunk0[b + 1] - chunk0[b];
      rc = nc < cap ? nc : cap;
      rc = rc < 0 ? 0 : rc;
    }
    int total;
    const int ex = r3d_block_excl_scan<SC_PLAN_THREADS>(rc, wsum, total);
    if (b < nb) run0[b] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) {
    run0[nb] = carry;
    rec[SC_P_NRUN] = carry;
    rec[SC_P_NSKIPPED] = chunk0[nb] - carry;
    rec[SC_P_NVOTED_RUN] = 0;  // counted by the next launch
  }
}

// valid points with a vote under the cap: the walk of the vote kernel without the logits.  Integer counts, one atomic
// per wave: the sum does not depend on the order.
__global__ __launch_bounds__(SC_THREADS) void r3d_scene_run_count_kernel(int M, const int* __restrict__ skey,
                                                                         const int* __restrict__ pos, const int* __restrict__ cell,
                                                                         const int* __restrict__ blk_n,
                                                                         const int* __restrict__ chunk0,
                                                                         const int* __restrict__ run0, sc_grid g,
                                                                         int* __restrict__ rec) {
  const int p = blockIdx.x * SC_THREADS + threadIdx.x;
  bool voted = false;
  if (p < M) {
    const int n_cells = g.ncx * g.ncy;
    const int sp = pos[p];
    const int key = (sp >= 0 && sp < M) ? skey[sp] : n_cells;
    if (key >= 0 && key < n_cells) {
      const int cx = key % g.ncx, cy = key / g.ncx;
      const int by0 = cy - g.r + 1 > 0 ? cy - g.r + 1 : 0, bx0 = cx - g.r + 1 > 0 ? cx - g.r + 1 : 0;
      for (int by = by0; by <= cy && by < g.nby; ++by)
        for (int bx = bx0; bx <= cx && bx < g.nbx; ++bx) {
          const int b = by * g.nbx + bx;
          const int nc = chunk0[b + 1] - chunk0[b];
          if (nc <= 0) continue;
          int q = sp - sc_row_start(cell, g, bx, cy);
          for (int row = by; row < cy; ++row) q += sc_row_end(cell, g, bx, row) - sc_row_start(cell, g, bx, row);
          if (q < 0 || q >= blk_n[b]) continue;
          voted = voted || q % nc < run0[b + 1] - run0[b];
        }
    }
  }
  const int n = __popcll(__ballot(voted));
  if ((threadIdx.x & 63) == 0 && n > 0) atomicAdd(&rec[SC_P_NVOTED_RUN], n);
}

extern "C" int r3d_scene_run_tables(long M, int ncx, int ncy, int r, int N, long chunk_cap, int32_t* ws, long ws_words,
                                    int max_chunks, int32_t* sws, long sws_words, void* stream) {
  R3D_REQUIRE(ws && sws, "r3d_scene_run_tables: null pointer (ws %p, sws %p)", (void*)ws, (void*)sws);
  SC_TRY(sc_check_plan("r3d_scene_run_tables", M, ncx, ncy, chunk_cap, ws_words));
  SC_TRY(sc_check_blocks("r3d_scene_run_tables", r, N));
  SC_TRY(sc_check_sparse_ws("r3d_scene_run_tables", M, ncx, ncy, chunk_cap, sws_words));
  R3D_REQUIRE(max_chunks >= 1, "r3d_scene_run_tables: max_chunks %d (at least 1)", max_chunks);
  const hipStream_t st = (hipStream_t)stream;
  const sc_view v = sc_make_view(M, ncx, ncy, r, chunk_cap, ws, sws);
  hipLaunchKernelGGL(r3d_scene_run_scan_kernel, dim3(1), dim3(SC_PLAN_THREADS), 0, st, v.chunk0, v.nb, max_chunks,
                     sws + v.S.run0, ws + v.L.rec);
  hipLaunchKernelGGL(r3d_scene_chunk_table_kernel, dim3((v.nb + SC_THREADS - 1) / SC_THREADS), dim3(SC_THREADS), 0, st, v.run0,
                     v.nb, (int)chunk_cap, sws + v.S.run_blk);
  hipLaunchKernelGGL(r3d_scene_run_count_kernel, dim3((int)((M + SC_THREADS - 1) / SC_THREADS)), dim3(SC_THREADS), 0, st, (int)M,
                     v.skey, v.pos, v.cell, v.blk_n, v.chunk0, v.run0, v.g, ws + v.L.rec);
  R3D_LAUNCH_CHECK("r3d_scene_run_tables");
  return R3D_OK;
}

// ------------------------------------------------------------------------------------------------ transfer
// Every valid point without a vote takes scores and label of the nearest voted point among the 3 x 3 cells around its
// own: d = (dx * dx + dy * dy) + dz * dz, every operation rounded on its own; on equal d the lowest scan index.  The
// minimum over (d, index) pairs does not depend on the order the candidates are met in.
//   flags    voff[i] = 1 when the point at sorted position i is voted; source = the point itself, or -1
//   scan     voff in place, exclusive (the three scan kernels of the sort)
//   compact  voted points -> cand rows {x, y, z, index} at voff; the others -> uq at i - voff[i]
//   tiles    per cell ceil(points without a vote / SC_Q_TILE) query tiles, their exclusive scan
//   transfer one workgroup per query tile; the candidate runs of the three cell rows go through LDS
__global__ __launch_bounds__(SC_THREADS) void r3d_scene_transfer_flags_kernel(int M, const int* __restrict__ order,
                                                                              const int* __restrict__ votes,
                                                                              int* __restrict__ voff,
                                                                              long long* __restrict__ source,
                                                                              long long* __restrict__ neighbours,
                                                                              float* __restrict__ weights) {
  const int i = blockIdx.x * SC_THREADS + threadIdx.x;
  if (i > M) return;
  int f = 0;
  if (i < M) {
    const bool voted = votes[i] > 0;
    source[i] = voted ? i : -1;
    if (neighbours) {  // (uniform) idw: a voted point is its own one neighbour, of weight 1; the receivers' rows come later
      neighbours[3L * i] = voted ? i : -1;
      neighbours[3L * i + 1] = neighbours[3L * i + 2] = -1;
      weights[3L * i] = voted ? 1.0f : 0.0f;
      weights[3L * i + 1] = weights[3L * i + 2] = 0.0f;
    }
    const int p = order[i];
    f = p >= 0 && p < M && votes[p] > 0;
  }
  voff[i] = f;
}

__global__ __launch_bounds__(SC_THREADS) void r3d_scene_transfer_compact_kernel(const float* __restrict__ scan, int ld, int M,
                                                                                const int* __restrict__ order,
                                                                                const int* __restrict__ votes,
                                                                                const int* __restrict__ voff,
                                                                                float4* __restrict__ cand,
                                                                                int* __restrict__ uq) {
  const int i = blockIdx.x * SC_THREADS + threadIdx.x;
  if (i >= M) return;
  const int p = order[i], v = voff[i];
  if (p < 0 || p >= M || v < 0 || v > i) return;  // holds for the tables of a plan; keeps both writes inside M rows
  if (votes[p] > 0) {
    const float* q = scan + (long)p * ld;
    cand[v] = make_float4(q[0], q[1], q[2], __int_as_float(p));
  } else {
    uq[i - v] = p;
  }
}

static __device__ __forceinline__ int sc_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(SC_PLAN_THREADS) void r3d_scene_transfer_tiles_kernel(const int* __restrict__ cell,
                                                                                   const int* __restrict__ voff, int n_cells,
                                                                                   int M, int* __restrict__ tile0,
                                                                                   int* __restrict__ rec) {
  __shared__ int wsum[SC_PLAN_THREADS / R3D_WAVE];
  int carry = 0;
  for (int c0 = 0; c0 < n_cells; c0 += SC_PLAN_THREADS) {
    const int c = c0 + threadIdx.x;
    int t = 0;
    if (c < n_cells) {
      const int s = sc_clamp(cell[c], 0, M), e = sc_clamp(cell[c + 1], s, M);
      const int u = (e - s) - (voff[e] - voff[s]);
      t = u > 0 ? (u + SC_Q_TILE - 1) / SC_Q_TILE : 0;
    }
    int total;
    const int ex = r3d_block_excl_scan<SC_PLAN_THREADS>(t, wsum, total);
    if (c < n_cells) tile0[c] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) {
    tile0[n_cells] = carry;
    rec[SC_T_NTRANSFERRED] = 0;
    rec[SC_T_NTILES] = carry;
    for (int k = 2; k < 8; ++k) rec[k] = 0;
  }
}

// (d, i) before (bd, bi) in lexicographic order
static __device__ __forceinline__ bool sc_closer(float d, int i, float bd, int bi) { return d < bd || (d == bd && i < bi); }

// NN = 1: the nearest voted point.  NN = 3 (idw): the three smallest (d, index) pairs, kept sorted in registers; a candidate
// meets one comparison, against the third, and the insertion (at most two shifts) sits behind that branch.  Then per class
// the means scores[q] / votes[q] of the three, weighted by w = 1 / (d + 1e-8), every operation rounded on its own.  Voted
// rows are only read and a receiver's row is written by its own thread.
template <int NN>
__global__ __launch_bounds__(SC_Q_TILE) void r3d_scene_transfer_kernel(
    const float* __restrict__ scan, int ld, int M, const int* __restrict__ cell, const int* __restrict__ voff,
    const int* __restrict__ uq, const int* __restrict__ tile0, const float4* __restrict__ cand, int ncx, int ncy, int K,
    float* __restrict__ scores, long long* __restrict__ labels, long long* __restrict__ source, int* __restrict__ rec,
    const int* __restrict__ votes, long long* __restrict__ neighbours, float* __restrict__ weights) {
  __shared__ float4 rows[SC_C_TILE];
  const int n_cells = ncx * ncy, t = blockIdx.x, tid = threadIdx.x;
  if (t >= tile0[n_cells]) return;  // (uniform) the grid is an upper bound of the tiles
  int lo = 0, hi = n_cells;         // tile0[lo] <= t < tile0[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (tile0[mid] <= t) lo = mid; else hi = mid;
  }
  const int c = lo, cx = c % ncx, cy = c / ncx;
  const int s = sc_clamp(cell[c], 0, M), e = sc_clamp(cell[c + 1], s, M);
  const int u = (s - voff[s]) + (t - tile0[c]) * SC_Q_TILE + tid;
  const bool live = u >= 0 && u < e - voff[e] && u < M;
  int p = live ? uq[u] : 0;
  p = sc_clamp(p, 0, M - 1);
  const float* pp = scan + (long)p * ld;
  const float px = pp[0], py = pp[1], pz = pp[2];
  float bd[NN];
  int bi[NN];
#pragma unroll
  for (int j = 0; j < NN; ++j) {
    bd[j] = INFINITY;
    bi[j] = 0x7fffffff;  // no candidate: every scan index comes before it
  }
  const int cx0 = cx > 0 ? cx - 1 : 0, cx1 = cx + 1 < ncx ? cx + 1 : ncx - 1;
  for (int row = cy > 0 ? cy - 1 : 0; row <= cy + 1 && row < ncy; ++row) {
    // cells (cx0 .. cx1, row) are neighbours in the sorted order: one run of candidate rows
    const int a = sc_clamp(voff[sc_clamp(cell[row * ncx + cx0], 0, M)], 0, M);
    const int b = sc_clamp(voff[sc_clamp(cell[row * ncx + cx1 + 1], 0, M)], a, M);
    for (int base = a; base < b; base += SC_C_TILE) {
      const int n = b - base < SC_C_TILE ? b - base : SC_C_TILE;
      __syncthreads();  // the previous tile has been read
      for (int k = tid; k < n; k += SC_Q_TILE) rows[k] = cand[base + k];
      __syncthreads();
      if (live) {
#pragma unroll 4
        for (int k = 0; k < n; ++k) {
          const float4 q = rows[k];  // every lane reads the same row: a broadcast
          const float dx = __fsub_rn(q.x, px), dy = __fsub_rn(q.y, py), dz = __fsub_rn(q.z, pz);
          const float d = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
          const int qi = __float_as_int(q.w);
          if (d < bd[NN - 1] || (d == bd[NN - 1] && qi < bi[NN - 1])) {
            if constexpr (NN == 3) {
              if (sc_closer(d, qi, bd[1], bi[1])) {
                bd[2] = bd[1]; bi[2] = bi[1];
                if (sc_closer(d, qi, bd[0], bi[0])) {
                  bd[1] = bd[0]; bi[1] = bi[0];
                  bd[0] = d; bi[0] = qi;
                } else {
                  bd[1] = d; bi[1] = qi;
                }
              } else {
                bd[2] = d; bi[2] = qi;
              }
            } else {
              bd[0] = d;
              bi[0] = qi;
            }
          }
        }
      }
    }
  }
  const int best_i = bi[0];
  const bool found = live && best_i >= 0 && best_i < M;
  if (found) {
    source[p] = best_i;
    if constexpr (NN == 3) {
      // the pairs are sorted, so the missing ones (fewer than three candidates) are the last
      const int nn = !(bi[1] >= 0 && bi[1] < M) ? 1 : (!(bi[2] >= 0 && bi[2] < M) ? 2 : 3);
      float w[3], cnt[3];
      int q[3];
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        q[j] = j < nn ? bi[j] : best_i;
        w[j] = j < nn ? __fdiv_rn(1.0f, __fadd_rn(bd[j], 1e-8f)) : 0.0f;  // d = +inf: w = 0
        cnt[j] = (float)votes[q[j]];
        neighbours[3L * p + j] = j < nn ? q[j] : -1;
        weights[3L * p + j] = w[j];
      }
      float wsum = w[0];
      if (nn > 1) wsum = __fadd_rn(wsum, w[1]);
      if (nn > 2) wsum = __fadd_rn(wsum, w[2]);
      int best = 0;
      float best_v = 0.0f;
      for (int k = 0; k < K; ++k) {
        const float m0 = __fdiv_rn(scores[(long)q[0] * K + k], cnt[0]);  // voted rows: nobody writes them
        float acc = __fmul_rn(w[0], m0);
        if (nn > 1) acc = __fadd_rn(acc, __fmul_rn(w[1], __fdiv_rn(scores[(long)q[1] * K + k], cnt[1])));
        if (nn > 2) acc = __fadd_rn(acc, __fmul_rn(w[2], __fdiv_rn(scores[(long)q[2] * K + k], cnt[2])));
        const float v = wsum == 0.0f ? m0 : __fdiv_rn(acc, wsum);  // every d infinite: the nearest one's means
        scores[(long)p * K + k] = v;
        if (k == 0 || v > best_v) {
          best = k;
          best_v = v;
        }
      }
      labels[p] = best;
    } else {
      labels[p] = labels[best_i];
      for (int k = 0; k < K; ++k) scores[(long)p * K + k] = scores[(long)best_i * K + k];  // a voted row: nobody writes it
    }
  }
  const int n = __popcll(__ballot(found));
  if ((tid & 63) == 0 && n > 0) atomicAdd(&rec[SC_T_NTRANSFERRED], n);  // an integer count: order-independent
}

// neighbours and weights both NULL: "nearest" (NN = 1); both given: "idw" (NN = 3).  One launch sequence.
extern "C" int r3d_scene_transfer(const float* scan, int ld, long M, int ncx, int ncy, long chunk_cap, const int32_t* ws,
                                  long ws_words, int32_t* sws, long sws_words, int n_classes, float* scores, int64_t* labels,
                                  const int32_t* votes, int64_t* source, int64_t* neighbours, float* weights, void* stream) {
  R3D_REQUIRE(scan && ws && sws && scores && labels && votes && source,
              "r3d_scene_transfer: null pointer (scan %p, ws %p, sws %p, scores %p, labels %p, votes %p, source %p)",
              (const void*)scan, (const void*)ws, (void*)sws, (void*)scores, (void*)labels, (const void*)votes, (void*)source);
  R3D_REQUIRE(!neighbours == !weights, "r3d_scene_transfer: null pointer (neighbours %p, weights %p go together)",
              (void*)neighbours, (void*)weights);
  SC_TRY(sc_check_ld("r3d_scene_transfer", ld));
  SC_TRY(sc_check_plan("r3d_scene_transfer", M, ncx, ncy, chunk_cap, ws_words));
  SC_TRY(sc_check_sparse_ws("r3d_scene_transfer", M, ncx, ncy, chunk_cap, sws_words));
  R3D_REQUIRE(n_classes >= 1 && n_classes <= 64, "r3d_scene_transfer: n_classes %d (1 .. 64)", n_classes);
  const hipStream_t st = (hipStream_t)stream;
  const sc_view v = sc_make_view(M, ncx, ncy, 1, chunk_cap, ws, sws);  // cells only: the transfer knows no blocks
  const sp_layout& S = v.S;
  float4* cand = (float4*)(sws + S.cand);
  const int gm = (int)((M + SC_THREADS - 1) / SC_THREADS), gm1 = (int)((M + 1 + SC_THREADS - 1) / SC_THREADS);
  hipLaunchKernelGGL(r3d_scene_transfer_flags_kernel, dim3(gm1), dim3(SC_THREADS), 0, st, (int)M, v.order, votes, sws + S.voff,
                     (long long*)source, (long long*)neighbours, weights);
  sc_excl_scan(sws + S.voff, M + 1, sws + S.part, st);
  hipLaunchKernelGGL(r3d_scene_transfer_compact_kernel, dim3(gm), dim3(SC_THREADS), 0, st, scan, ld, (int)M, v.order, votes,
                     sws + S.voff, cand, sws + S.uq);
  hipLaunchKernelGGL(r3d_scene_transfer_tiles_kernel, dim3(1), dim3(SC_PLAN_THREADS), 0, st, v.cell, sws + S.voff, v.n_cells,
                     (int)M, sws + S.tile0, sws + S.rec);
  // sum over the cells of ceil(u / SC_Q_TILE) <= U / SC_Q_TILE + cells that hold such a point
  const long tiles = M / SC_Q_TILE + (v.n_cells < M ? v.n_cells : M) + 1;
  const auto kernel = neighbours ? r3d_scene_transfer_kernel<3> : r3d_scene_transfer_kernel<1>;
  hipLaunchKernelGGL(kernel, dim3((int)tiles), dim3(SC_Q_TILE), 0, st, scan, ld, (int)M, v.cell, sws + S.voff, sws + S.uq,
                     sws + S.tile0, cand, ncx, ncy, n_classes, scores, (long long*)labels, (long long*)source, sws + S.rec, votes,
                     (long long*)neighbours, weights);
  R3D_LAUNCH_CHECK("r3d_scene_transfer");
  return R3D_OK;
}

// ------------------------------------------------------------------------------------------------ several support sets, one label
// predict_scene_sets, step 10 ("Labelling a scan against several support sets"): scores (M, K, C) are the
// voted (and transferred) scores of K support sets of C = n_way + 1 classes each.  One thread per scan point; a point has a
// label when it has a vote or a transfer source.  Per set the arg-max l of its C scores by sc_argmax_step; a set with
// l >= 1 claims the point with the margin m = s[l] - s[r], r the arg-max over the other classes by the same step, one fp32
// subtraction; a NaN margin does not claim.  The greatest margin wins, the lowest set on equal margins.  Nothing is summed
// and no thread reads what another writes.
__global__ __launch_bounds__(SC_THREADS) void r3d_scene_merge_sets_kernel(
    int M, int K, int C, const float* __restrict__ scores, const int* __restrict__ votes,
    const long long* __restrict__ source /* or null */, const int* __restrict__ classes, long long background,
    long long* __restrict__ set_labels, long long* __restrict__ labels, int* __restrict__ set_of, float* __restrict__ margin) {
  const int p = blockIdx.x * SC_THREADS + threadIdx.x;
  if (p >= M) return;
  const bool has = votes[p] > 0 || (source && source[p] >= 0);
  int win = -1, win_l = 0;
  float win_m = 0.0f;
  for (int k = 0; k < K; ++k) {
    if (!has) {
      set_labels[(long)p * K + k] = -1;
      continue;
    }
    const float* s = scores + ((long)p * K + k) * C;
    int l = -1, r = -1;
    float lv = 0.0f, rv = 0.0f;
    for (int j = 0; j < C; ++j) sc_argmax_step(j, s[j], l, lv);
    set_labels[(long)p * K + k] = l;
    if (l < 1) continue;  // the set says background
    for (int j = 0; j < C; ++j)
      if (j != l) sc_argmax_step(j, s[j], r, rv);
    const float m = __fsub_rn(lv, rv);
    if (m != m) continue;
    if (win < 0 || m > win_m) {
      win = k;
      win_l = l;
      win_m = m;
    }
  }
  labels[p] = !has ? -1 : (win < 0 ? background : (long long)classes[win * (C - 1) + win_l - 1]);
  set_of[p] = win;
  margin[p] = win < 0 ? 0.0f : win_m;
}

extern "C" int r3d_scene_merge_sets(long M, int n_sets, int n_classes, const float* scores, const int32_t* votes,
                                    const int64_t* source, const int32_t* classes, long background, int64_t* set_labels,
                                    int64_t* labels, int32_t* set_of, float* margin, void* stream) {
  R3D_REQUIRE(scores && votes && classes && set_labels && labels && set_of && margin,
              "r3d_scene_merge_sets: null pointer (scores %p, votes %p, classes %p, set_labels %p, labels %p, set_of %p, margin %p)",
              (const void*)scores, (const void*)votes, (const void*)classes, (void*)set_labels, (void*)labels, (void*)set_of,
              (void*)margin);
  R3D_REQUIRE(M >= 1 && M <= (1L << 27), "r3d_scene_merge_sets: M %ld (1 .. 2^27)", M);
  R3D_REQUIRE(n_sets >= 1 && n_classes >= 2 && (long)n_sets * n_classes <= 64,
              "r3d_scene_merge_sets: %d sets of %d classes (at least 2 classes, at most 64 score columns)", n_sets, n_classes);
  hipLaunchKernelGGL(r3d_scene_merge_sets_kernel, dim3((int)((M + SC_THREADS - 1) / SC_THREADS)), dim3(SC_THREADS), 0,
                     (hipStream_t)stream, (int)M, n_sets, n_classes, scores, votes, (const long long*)source, classes,
                     (long long)background, (long long*)set_labels, (long long*)labels, set_of, margin);
  R3D_LAUNCH_CHECK("r3d_scene_merge_sets");
  return R3D_OK;
}

// ------------------------------------------------------------------------------------------------ a support set from an annotated scan
// fit_scene ("Fitting from an annotated scan"): the cloud of a block is its chunk 0 -- list positions
// 0, nc, 2 nc, ..., len = ceil(n / nc) members --; fg[b][w] counts the members labelled classes[w]; way w's shots are
// its eligible blocks (fg > max((int)floorf(len * min_ratio), min_fg)) by fg descending, block id ascending.
#define SC_MAX_WAYS 7

// One workgroup per block: threads stride over the len members, per way a ballot and a population count per wave, then
// the integer sum of the waves in LDS.  Every member counts once (wrap-around slots are not visited); dropped blocks get 0.
template <typename L>
__global__ __launch_bounds__(SC_THREADS) void r3d_scene_support_counts_kernel(
    const L* __restrict__ labels, int M, const int* __restrict__ order, const int* __restrict__ cell,
    const int* __restrict__ blk_n, const int* __restrict__ chunk0, sc_grid g, const int* __restrict__ classes, int n_way,
    int* __restrict__ fg) {
  __shared__ int wcnt[SC_THREADS / R3D_WAVE][SC_MAX_WAYS + 1];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n = blk_n[b], nc = chunk0[b + 1] - chunk0[b];
  if (nc <= 0 || n <= 0) {  // (uniform) a dropped block
    if (tid < n_way) fg[(long)b * n_way + tid] = 0;
    return;
  }
  const int bx = b % g.nbx, by = b / g.nbx, len = (n + nc - 1) / nc;
  long long cls[SC_MAX_WAYS];
  int acc[SC_MAX_WAYS];
#pragma unroll
  for (int k = 0; k < SC_MAX_WAYS; ++k) {
    cls[k] = k < n_way ? (long long)classes[k] : 0;
    acc[k] = 0;
  }
  for (int t0 = 0; t0 < len; t0 += SC_THREADS) {  // a uniform trip count: every lane reaches every ballot
    const int t = t0 + tid;
    const bool live = t < len;
    long long lab = 0;
    if (live) {
      int p = order[sc_list_to_sorted(cell, g, bx, by, t * nc)];
      p = p < 0 ? 0 : (p >= M ? M - 1 : p);
      lab = (long long)labels[p];
    }
#pragma unroll
    for (int k = 0; k < SC_MAX_WAYS; ++k)
      if (k < n_way) acc[k] += __popcll(__ballot(live && lab == cls[k]));  // the wave's count, the same in every lane
  }
  if ((tid & 63) == 0) {
#pragma unroll
    for (int k = 0; k < SC_MAX_WAYS; ++k) wcnt[tid >> 6][k] = acc[k];
  }
  __syncthreads();
  if (tid < n_way) {
    int s = 0;
#pragma unroll
    for (int w = 0; w < SC_THREADS / R3D_WAVE; ++w) s += wcnt[w][tid];
    fg[(long)b * n_way + tid] = s;
  }
}

static __device__ __forceinline__ unsigned long long sc_shfl_xor_u64(unsigned long long v, int o) {
  const unsigned lo = __shfl_xor((unsigned)(v & 0xffffffffu), o), hi = __shfl_xor((unsigned)(v >> 32), o);
  return ((unsigned long long)hi << 32) | lo;
}

// One workgroup per way, k_shot rounds.  A round takes the maximum of key = (fg << 32) | (0xFFFFFFFF - b) over the eligible
// blocks whose key is below the previous round's pick: fg descending, then block id ascending, no "taken" flags.  An
// eligible block has fg >= 1, so key 0 says "none left": shot_block -1, shot_fg 0.  rec[w] = the way's eligible blocks.
__global__ __launch_bounds__(SC_THREADS) void r3d_scene_support_pick_kernel(
    const int* __restrict__ blk_n, const int* __restrict__ chunk0, int nb, const int* __restrict__ fg, int n_way, int k_shot,
    float min_ratio, int min_fg, int* __restrict__ shot_block, int* __restrict__ shot_fg, int* __restrict__ rec) {
  __shared__ unsigned long long wmax[SC_THREADS / R3D_WAVE];
  __shared__ int wcnt[SC_THREADS / R3D_WAVE];
  const int w = blockIdx.x, tid = threadIdx.x;
  unsigned long long prev = ~0ull;
  for (int round = 0; round < k_shot; ++round) {
    unsigned long long best = 0;
    int cnt = 0;
    for (int b = tid; b < nb; b += SC_THREADS) {
      const int nc = chunk0[b + 1] - chunk0[b], n = blk_n[b];
      if (nc <= 0 || n <= 0) continue;
      const int len = (n + nc - 1) / nc;
      const int ratio = (int)floorf((float)len * min_ratio);  // fp32, one IEEE multiplication (the build does not contract)
      const int thr = ratio > min_fg ? ratio : min_fg;
      const int f = fg[(long)b * n_way + w];
      if (f > thr) {
        ++cnt;
        const unsigned long long key = ((unsigned long long)(unsigned)f << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)b);
        if (key < prev && key > best) best = key;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long other = sc_shfl_xor_u64(best, o);
      best = other > best ? other : best;
      cnt += __shfl_xor(cnt, o);
    }
    if ((tid & 63) == 0) {
      wmax[tid >> 6] = best;
      wcnt[tid >> 6] = cnt;
    }
    __syncthreads();
    best = wmax[0];
    cnt = wcnt[0];
#pragma unroll
    for (int k = 1; k < SC_THREADS / R3D_WAVE; ++k) {
      best = wmax[k] > best ? wmax[k] : best;
      cnt += wcnt[k];
    }
    __syncthreads();  // wmax / wcnt are written again in the next round
    if (tid == 0) {
      shot_block[w * k_shot + round] = best ? (int)(0xFFFFFFFFu - (unsigned)(best & 0xffffffffu)) : -1;
      shot_fg[w * k_shot + round] = (int)(best >> 32);
      if (round == 0) rec[w] = cnt;
    }
    prev = best;  // 0 after the last eligible block: nothing is below it
  }
  if (w == 0 && tid >= n_way && tid < 8) rec[tid] = 0;
}

#define SC_REQUIRE_SUPPORT_ARGS(name)                                                                                     \
  R3D_REQUIRE(n_way >= 1 && n_way <= SC_MAX_WAYS, name ": n_way %d (1 .. 7)", n_way)

extern "C" int r3d_scene_support_counts(long M, int ncx, int ncy, int r, int N, long chunk_cap, const int32_t* ws,
                                        long ws_words, const void* labels, int label_bytes, const int32_t* classes, int n_way,
                                        int32_t* fg, void* stream) {
  R3D_REQUIRE(ws && labels && classes && fg, "r3d_scene_support_counts: null pointer (ws %p, labels %p, classes %p, fg %p)",
              (const void*)ws, labels, (const void*)classes, (void*)fg);
  SC_TRY(sc_check_plan("r3d_scene_support_counts", M, ncx, ncy, chunk_cap, ws_words));
  SC_TRY(sc_check_blocks("r3d_scene_support_counts", r, N));
  SC_REQUIRE_SUPPORT_ARGS("r3d_scene_support_counts");
  R3D_REQUIRE(label_bytes == 4 || label_bytes == 8, "r3d_scene_support_counts: labels of %d bytes (int32 or int64)", label_bytes);
  const sc_view v = sc_make_view(M, ncx, ncy, r, chunk_cap, ws, nullptr);
  if (label_bytes == 8)
    hipLaunchKernelGGL(r3d_scene_support_counts_kernel<long long>, dim3(v.nb), dim3(SC_THREADS), 0, (hipStream_t)stream,
                       (const long long*)labels, (int)M, v.order, v.cell, v.blk_n, v.chunk0, v.g, classes, n_way, fg);
  else
    hipLaunchKernelGGL(r3d_scene_support_counts_kernel<int>, dim3(v.nb), dim3(SC_THREADS), 0, (hipStream_t)stream,
                       (const int*)labels, (int)M, v.order, v.cell, v.blk_n, v.chunk0, v.g, classes, n_way, fg);
  R3D_LAUNCH_CHECK("r3d_scene_support_counts");
  return R3D_OK;
}

extern "C" int r3d_scene_support_pick(long M, int ncx, int ncy, int r, int N, long chunk_cap, const int32_t* ws, long ws_words,
                                      const int32_t* fg, int n_way, int k_shot, float min_ratio, int min_fg,
                                      int32_t* shot_block, int32_t* shot_fg, int32_t* rec, void* stream) {
  R3D_REQUIRE(ws && fg && shot_block && shot_fg && rec,
              "r3d_scene_support_pick: null pointer (ws %p, fg %p, shot_block %p, shot_fg %p, rec %p)", (const void*)ws,
              (const void*)fg, (void*)shot_block, (void*)shot_fg, (void*)rec);
  SC_TRY(sc_check_plan("r3d_scene_support_pick", M, ncx, ncy, chunk_cap, ws_words));
  SC_TRY(sc_check_blocks("r3d_scene_support_pick", r, N));
  SC_REQUIRE_SUPPORT_ARGS("r3d_scene_support_pick");
  R3D_REQUIRE(k_shot >= 1 && k_shot <= 64, "r3d_scene_support_pick: k_shot %d (1 .. 64)", k_shot);
  R3D_REQUIRE(min_ratio >= 0.0f && min_ratio < 1.0f, "r3d_scene_support_pick: min_ratio %g (0 <= ratio < 1)", (double)min_ratio);
  R3D_REQUIRE(min_fg >= 0, "r3d_scene_support_pick: min_fg %d (at least 0)", min_fg);
  const sc_view v = sc_make_view(M, ncx, ncy, r, chunk_cap, ws, nullptr);
  hipLaunchKernelGGL(r3d_scene_support_pick_kernel, dim3(n_way), dim3(SC_THREADS), 0, (hipStream_t)stream, v.blk_n, v.chunk0,
                     v.nb, fg, n_way, k_shot, min_ratio, min_fg, shot_block, shot_fg, rec);
  R3D_LAUNCH_CHECK("r3d_scene_support_pick");
  return R3D_OK;
}

extern "C" int r3d_scene_prepare_blocks(const float* scan, int ld, long M, int ncx, int ncy, int r, int N, long chunk_cap,
                                        const int32_t* ws, long ws_words, const int32_t* blocks, int G, int C, int rgb_ch,
                                        int XYZ_ch, float* out, long o_sb, long o_sc, long o_sn, int32_t* slot_map,
                                        const void* labels, int label_bytes, const int32_t* cloud_class, int32_t* mask,
                                        void* stream) {
  R3D_REQUIRE(blocks, "r3d_scene_prepare_blocks: null pointer (blocks)");
  R3D_REQUIRE(G > 0 && G <= SC_MAX_CELLS, "r3d_scene_prepare_blocks: G %d (1 .. 65536 block ids)", G);
  R3D_REQUIRE((labels && cloud_class && mask) || (!labels && !cloud_class && !mask),
              "r3d_scene_prepare_blocks: labels %p, cloud_class %p and mask %p go together", labels, (const void*)cloud_class,
              (void*)mask);
  R3D_REQUIRE(!labels || label_bytes == 4 || label_bytes == 8, "r3d_scene_prepare_blocks: labels of %d bytes (int32 or int64)",
              label_bytes);
  const sc_block_args ba = {blocks, labels, label_bytes, cloud_class, mask};
  return sc_prepare(scan, ld, M, ncx, ncy, r, N, chunk_cap, ws, ws_words, nullptr, 0, G, C, rgb_ch, XYZ_ch, out, o_sb, o_sc, o_sn,
                    slot_map, stream, &ba);
}

// ------------------------------------------------------------------------------------------------ one label per segment
// pool_segments ("Pooling scores over segments", P1-P5): the scan comes with a partition of its points
// (instance ids, supervoxels); per segment the mean of its contributors' mean logits, summed in a fixed order, then
// every point of a large enough segment takes its segment's row and label.
//   ids      largest legal id, negative ids, ids >= 2^31 - 1                    -> the record the host reads (read 1)
//   group    keys (a negative id: the one key above every id), the stable radix sort above on (id, scan index), heads
//            and contributors as flags, their integer scans, segment and tile tables   -> S, tiles (read 2)
//   pool     per tile of 256 contributor ranks one partial row, rows staged in LDS and added one at a time by the lane
//            that owns the column; per segment the partials added in tile order, one division, the arg-max
//   spread   per scan point its segment's row or its own                        -> the counts (read 3)
// Floats are added by __fadd_rn in the stated order and divided by __fdiv_rn; counts are integer scans and integer atomics.
#define SG_TILE 256    // contributor ranks per tile
#define SG_BATCH 32    // rows of a tile staged in LDS at a time: 32 * 64 floats per wave, 32 KiB per workgroup
#define SG_WAVES (SC_THREADS / R3D_WAVE)
#define SG_UNROLL 8    // element loads of a lane in flight while a batch is staged; partials loaded ahead of their additions
// the record, words of ws[0 .. 16)
#define SG_R_MAX1 0      // largest legal id + 1, 0 without one
#define SG_R_NNEG 1      // points with a negative id
#define SG_R_NBAD 2      // ids >= 2^31 - 1
#define SG_R_BADMAX 4    // the largest of them (two words)
#define SG_R_S 6         // segments
#define SG_R_NCONTRIB 7  // contributors
#define SG_R_NTILES 8    // tiles
#define SG_R_NPOOLED 9
#define SG_R_NFILLED 10
#define SG_R_NUNLAB 11
#define SG_ID_LIMIT 2147483647LL
#define SG_COUNT_BLOCKS 1024  // workgroups of the two kernels that end in atomics on the record

static int sg_count_grid(long M) {
  const long g = (M + SC_THREADS - 1) / SC_THREADS;
  return (int)(g < SG_COUNT_BLOCKS ? g : SG_COUNT_BLOCKS);
}

struct sg_layout {
  long rec;              // 16
  long key[2], idx[2];   // ping-pong pairs of the sort; the pair the sort leaves free holds the two scans below
  long hist, part;       // digit counts of a pass; block partials of a scan
  long tiles;            // M + 1: tile heads in front of a sorted position
  long clist;            // contributors' scan indices, segment after segment, ascending scan index inside one
  long seg_start;        // S + 1: first sorted position of a segment
  long cstart;           // S + 1: first entry of a segment in clist
  long seg_id;           // S
  long tile_seg;         // segment of a tile
  long total;
  int n_tiles, n_part, n_scan;
};

static sg_layout sg_make_layout(long M) {
  sg_layout L;
  const long Ma = sc_align(M + 1);
  long o = 0;
  L.n_tiles = (int)((M + SC_TILE - 1) / SC_TILE);
  const long n_hist = 256L * L.n_tiles;
  L.n_part = (int)((n_hist + SC_TILE - 1) / SC_TILE);
  L.n_scan = (int)((M + 1 + SC_TILE - 1) / SC_TILE);
  L.rec = o; o += 16;
  L.key[0] = o; o += Ma;
  L.key[1] = o; o += Ma;
  L.idx[0] = o; o += Ma;
  L.idx[1] = o; o += Ma;
  L.hist = o; o += sc_align(n_hist);
  L.part = o; o += sc_align(L.n_part > L.n_scan ? L.n_part : L.n_scan);
  L.tiles = o; o += Ma;
  L.clist = o; o += Ma;
  L.seg_start = o; o += Ma;
  L.cstart = o; o += Ma;
  L.seg_id = o; o += Ma;
  L.tile_seg = o; o += Ma;
  L.total = o;
  return L;
}

extern "C" long r3d_scene_seg_ws_words(long M) { return M > 0 && M <= SC_MAX_POINTS ? sg_make_layout(M).total : -1; }

// the workgroup's sum of a per-thread count, valid in thread 0 (red: SG_WAVES ints)
static __device__ __forceinline__ int sg_block_count(int v, int* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();  // red may still be read from the count before
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  int t = 0;
#pragma unroll
  for (int w = 0; w < SG_WAVES; ++w) t += red[w];
  return t;
}

// At most SG_COUNT_BLOCKS workgroups stride over the ids and each ends in one atomic per word of the record: a wave
// per atomic (15 625 of them on one cache line at 10^6 points) took longer than reading the ids.
template <typename L>
__global__ __launch_bounds__(SC_THREADS) void r3d_scene_seg_ids_kernel(const L* __restrict__ seg, int M, int* __restrict__ rec) {
  __shared__ int red[SG_WAVES];
  __shared__ unsigned long long red_max[SG_WAVES];
  int mx = 0, n_neg = 0, n_bad = 0;
  unsigned long long bmax = 0ull;
  for (long i = (long)blockIdx.x * SC_THREADS + threadIdx.x; i < M; i += (long)gridDim.x * SC_THREADS) {
    const long long g = (long long)seg[i];
    if (g < 0) {
      ++n_neg;
    } else if (g >= SG_ID_LIMIT) {
      ++n_bad;
      bmax = (unsigned long long)g > bmax ? (unsigned long long)g : bmax;
    } else {
      mx = (int)g + 1 > mx ? (int)g + 1 : mx;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int m2 = __shfl_xor(mx, o);
    mx = m2 > mx ? m2 : mx;
    const unsigned long long b2 = sc_shfl_xor_u64(bmax, o);
    bmax = b2 > bmax ? b2 : bmax;
  }
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6] = mx;
    red_max[threadIdx.x >> 6] = bmax;
  }
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 0; w < SG_WAVES; ++w) {
      mx = red[w] > mx ? red[w] : mx;
      bmax = red_max[w] > bmax ? red_max[w] : bmax;
    }
  n_neg = sg_block_count(n_neg, red);
  n_bad = sg_block_count(n_bad, red);
  if (threadIdx.x == 0) {  // integer maxima and counts: order-independent
    if (mx > 0) atomicMax(&rec[SG_R_MAX1], mx);
    if (n_neg > 0) atomicAdd(&rec[SG_R_NNEG], n_neg);
    if (n_bad > 0) {
      atomicAdd(&rec[SG_R_NBAD], n_bad);
      atomicMax((unsigned long long*)(rec + SG_R_BADMAX), bmax);
    }
  }
}

extern "C" int r3d_scene_seg_ids(const void* segments, int seg_bytes, long M, int32_t* ws, long ws_words, void* stream) {
  R3D_REQUIRE(segments && ws, "r3d_scene_seg_ids: null pointer (segments %p, ws %p)", segments, (void*)ws);
  R3D_REQUIRE(M > 0 && M <= SC_MAX_POINTS, "r3d_scene_seg_ids: M %ld (1 .. 2^27 points)", M);
  R3D_REQUIRE(seg_bytes == 4 || seg_bytes == 8, "r3d_scene_seg_ids: segments of %d bytes (int32 or int64)", seg_bytes);
  R3D_REQUIRE(ws_words >= r3d_scene_seg_ws_words(M), "r3d_scene_seg_ids: workspace of %ld words, %ld needed", ws_words,
              r3d_scene_seg_ws_words(M));
  const hipStream_t st = (hipStream_t)stream;
  const sg_layout L = sg_make_layout(M);
  const int gm = sg_count_grid(M);
  r3d_zero_words(ws + L.rec, 16, st);
  if (seg_bytes == 8)
    hipLaunchKernelGGL(r3d_scene_seg_ids_kernel<long long>, dim3(gm), dim3(SC_THREADS), 0, st, (const long long*)segments, (int)M,
                       ws + L.rec);
  else
    hipLaunchKernelGGL(r3d_scene_seg_ids_kernel<int>, dim3(gm), dim3(SC_THREADS), 0, st, (const int*)segments, (int)M,
                       ws + L.rec);
  R3D_LAUNCH_CHECK("r3d_scene_seg_ids");
  return R3D_OK;
}

template <typename L>
__global__ __launch_bounds__(SC_THREADS) void r3d_scene_seg_keys_kernel(const L* __restrict__ seg, int M, int none,
                                                                        int* __restrict__ key, int* __restrict__ idx) {
  const int i = blockIdx.x * SC_THREADS + threadIdx.x;
  if (i >= M) return;
  const long long g = (long long)seg[i];
  key[i] = (g < 0 || g >= (long long)none) ? none : (int)g;  // (the host checked: no id reaches `none`)
  idx[i] = i;
}

// sorted position i: heads[i] = it opens a segment, contrib[i] = it is a contributor (P1); word M of both is 0, so that
// the exclusive scans leave the totals there
__global__ __launch_bounds__(SC_THREADS) void r3d_scene_seg_flags_kernel(const int* __restrict__ skey, const int* __restrict__ order,
                                                                         int M, int none, const int* __restrict__ votes,
                                                                         int* __restrict__ heads, int* __restrict__ contrib) {
  const int i = blockIdx.x * SC_THREADS + threadIdx.x;
  if (i > M) return;
  int h = 0, c = 0;
  if (i < M) {
    const int k = skey[i];
    const bool in_seg = k >= 0 && k < none;
    int p = order[i];
    p = p < 0 ? 0 : (p >= M ? M - 1 : p);
    h = in_seg && (i == 0 || skey[i - 1] != k);
    c = in_seg && votes[p] > 0;
  }
  heads[i] = h;
  contrib[i] = c;
}

// after the scans: heads[i] = segments opened in front of i, contrib[i] = contributors in front of i.  Every segment's
// row of the tables is written by the thread of its first sorted position, row S by the thread of position M.
__global__ __launch_bounds__(SC_THREADS) void r3d_scene_seg_tables_kernel(
    const int* __restrict__ skey, const int* __restrict__ order, int M, int n_in_seg, const int* __restrict__ heads,
    const int* __restrict__ contrib, int* __restrict__ seg_start, int* __restrict__ cstart, int* __restrict__ seg_id,
    int* __restrict__ clist, int* __restrict__ segment_index) {
  const int i = blockIdx.x * SC_THREADS + threadIdx.x;
  if (i > M) return;
  if (i == M) {
    const int S = heads[M];
    seg_start[S] = n_in_seg;
    cstart[S] = contrib[M];
    return;
  }
  const int s = heads[i + 1] - 1, c = contrib[i];
  int p = order[i];
  p = p < 0 ? 0 : (p >= M ? M - 1 : p);
  segment_index[p] = i < n_in_seg ? s : -1;
  if (i >= n_in_seg) return;
  if (heads[i + 1] != heads[i]) {
    seg_start[s] = i;
    cstart[s] = c;
    seg_id[s] = skey[i];
  }
  if (contrib[i + 1] != c) clist[c] = p;
}

// tile heads: the contributors whose rank inside their segment is a multiple of SG_TILE
__global__ __launch_bounds__(SC_THREADS) void r3d_scene_seg_tile_flags_kernel(int M, int n_in_seg, const int* __restrict__ heads,
                                                                              const int* __restrict__ contrib,
                                                                              const int* __restrict__ cstart,
                                                                              int* __restrict__ tiles) {
  const int i = blockIdx.x * SC_THREADS + threadIdx.x;
  if (i > M) return;
  int f = 0;
  if (i < n_in_seg && contrib[i + 1] != contrib[i]) f = ((contrib[i] - cstart[heads[i + 1] - 1]) % SG_TILE) == 0;
  tiles[i] = f;
}

__global__ __launch_bounds__(SC_THREADS) void r3d_scene_seg_tile_table_kernel(int M, int n_in_seg, const int* __restrict__ heads,
                                                                              const int* __restrict__ contrib,
                                                                              const int* __restrict__ tiles,
                                                                              int* __restrict__ tile_seg, int* __restrict__ rec) {
  const int i = blockIdx.x * SC_THREADS + threadIdx.x;
  if (i > M) return;
  if (i == M) {
    rec[SG_R_S] = heads[M];
    rec[SG_R_NCONTRIB] = contrib[M];
    rec[SG_R_NTILES] = tiles[M];
    return;
  }
  if (i < n_in_seg && tiles[i + 1] != tiles[i]) tile_seg[tiles[i]] = heads[i + 1] - 1;
}

extern "C" int r3d_scene_seg_group(const void* segments, int seg_bytes, long M, const int32_t* votes, long max_id, long n_negative,
                                   int32_t* segment_index, int32_t* ws, long ws_words, void* stream) {
  R3D_REQUIRE(segments && votes && segment_index && ws, "r3d_scene_seg_group: null pointer (segments %p, votes %p, segment_index %p, ws %p)",
              segments, (const void*)votes, (void*)segment_index, (void*)ws);
  R3D_REQUIRE(M > 0 && M <= SC_MAX_POINTS, "r3d_scene_seg_group: M %ld (1 .. 2^27 points)", M);
  R3D_REQUIRE(seg_bytes == 4 || seg_bytes == 8, "r3d_scene_seg_group: segments of %d bytes (int32 or int64)", seg_bytes);
  R3D_REQUIRE(max_id >= -1 && max_id < SG_ID_LIMIT, "r3d_scene_seg_group: largest id %ld (-1: none .. 2^31 - 2)", max_id);
  R3D_REQUIRE(n_negative >= 0 && n_negative <= M, "r3d_scene_seg_group: %ld negative ids among %ld points", n_negative, M);
  R3D_REQUIRE(ws_words >= r3d_scene_seg_ws_words(M), "r3d_scene_seg_group: workspace of %ld words, %ld needed", ws_words,
              r3d_scene_seg_ws_words(M));
  const hipStream_t st = (hipStream_t)stream;
  const sg_layout L = sg_make_layout(M);
  const int none = (int)(max_id + 1);  // the key of a point without a segment: above every id
  const long key_max = n_negative > 0 ? max_id + 1 : (max_id < 0 ? 0 : max_id);
  const int passes = key_max < 256 ? 1 : (key_max < 65536 ? 2 : (key_max < (1L << 24) ? 3 : 4));
  const int gm = (int)((M + SC_THREADS - 1) / SC_THREADS), gm1 = (int)((M + 1 + SC_THREADS - 1) / SC_THREADS);
  if (seg_bytes == 8)
    hipLaunchKernelGGL(r3d_scene_seg_keys_kernel<long long>, dim3(gm), dim3(SC_THREADS), 0, st, (const long long*)segments, (int)M,
                       none, ws + L.key[0], ws + L.idx[0]);
  else
    hipLaunchKernelGGL(r3d_scene_seg_keys_kernel<int>, dim3(gm), dim3(SC_THREADS), 0, st, (const int*)segments, (int)M, none,
                       ws + L.key[0], ws + L.idx[0]);
  const int sorted = sc_sort_pairs(ws, L.key, L.idx, L.hist, L.part, M, L.n_tiles, passes, st), spare = sorted ^ 1;
  int* skey = ws + L.key[sorted];
  int* order = ws + L.idx[sorted];
  int* heads = ws + L.key[spare];
  int* contrib = ws + L.idx[spare];
  const int n_in_seg = (int)(M - n_negative);
  hipLaunchKernelGGL(r3d_scene_seg_flags_kernel, dim3(gm1), dim3(SC_THREADS), 0, st, skey, order, (int)M, none, votes, heads,
                     contrib);
  sc_excl_scan(heads, M + 1, ws + L.part, st);
  sc_excl_scan(contrib, M + 1, ws + L.part, st);
  hipLaunchKernelGGL(r3d_scene_seg_tables_kernel, dim3(gm1), dim3(SC_THREADS), 0, st, skey, order, (int)M, n_in_seg, heads, contrib,
                     ws + L.seg_start, ws + L.cstart, ws + L.seg_id, ws + L.clist, segment_index);
  hipLaunchKernelGGL(r3d_scene_seg_tile_flags_kernel, dim3(gm1), dim3(SC_THREADS), 0, st, (int)M, n_in_seg, heads, contrib,
                     ws + L.cstart, ws + L.tiles);
  sc_excl_scan(ws + L.tiles, M + 1, ws + L.part, st);
  hipLaunchKernelGGL(r3d_scene_seg_tile_table_kernel, dim3(gm1), dim3(SC_THREADS), 0, st, (int)M, n_in_seg, heads, contrib,
                     ws + L.tiles, ws + L.tile_seg, ws + L.rec);
  R3D_LAUNCH_CHECK("r3d_scene_seg_group");
  return R3D_OK;
}

// One wave per tile, four tiles per workgroup.  A batch of SG_BATCH rows is loaded with consecutive lanes on consecutive
// elements, divided by the row's votes (P1) and laid down in LDS in that order; lane j then adds column j of the batch,
// row after row (P3).  Every wave goes through every barrier: a wave without a tile, or past its tile's end, adds nothing.
__global__ __launch_bounds__(SC_THREADS) void r3d_scene_seg_pool_tiles_kernel(
    int n_tiles, int C, int M, const float* __restrict__ scores, const int* __restrict__ votes, const int* __restrict__ clist,
    const int* __restrict__ cstart, const int* __restrict__ seg_start, const int* __restrict__ tiles,
    const int* __restrict__ tile_seg, float* __restrict__ part) {
  __shared__ float stage[SG_WAVES][SG_BATCH * 64];
  __shared__ int row_p[SG_WAVES][SG_TILE];    // the tile's rows: scan index
  __shared__ float row_v[SG_WAVES][SG_TILE];  // and votes as a float
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int t = blockIdx.x * SG_WAVES + w;
  int first = 0, n = 0;
  if (t < n_tiles) {
    int s = tile_seg[t];
    s = s < 0 ? 0 : (s >= M ? M - 1 : s);
    first = cstart[s] + SG_TILE * (t - tiles[sc_clamp(seg_start[s], 0, M)]);
    n = cstart[s + 1] - first;
    n = n > SG_TILE ? SG_TILE : n;
    // the tables come from counts of these very points, so the rows lie inside clist; the guard only matters for a
    // workspace that r3d_scene_seg_group did not fill
    if (first < 0 || n < 0 || (long)first + n > M) first = n = 0;
  }
  // the tile's scan indices and votes first, four independent loads a lane: the element loads below then depend on LDS
  // only and go out eight at a time (one load per element, each waiting for its index, took ten times as long)
  int pr[SG_TILE / R3D_WAVE];
#pragma unroll
  for (int k = 0; k < SG_TILE / R3D_WAVE; ++k) {
    const int r = k * R3D_WAVE + lane;
    pr[k] = sc_clamp(clist[first + (r < n ? r : 0)], 0, M - 1);
  }
#pragma unroll
  for (int k = 0; k < SG_TILE / R3D_WAVE; ++k) {
    row_p[w][k * R3D_WAVE + lane] = pr[k];
    row_v[w][k * R3D_WAVE + lane] = (float)votes[pr[k]];
  }
  __syncthreads();
  float acc = 0.0f;
  for (int r0 = 0; r0 < SG_TILE; r0 += SG_BATCH) {
    const int nb = n - r0 < SG_BATCH ? n - r0 : SG_BATCH;  // <= 0: nothing left
    const int n_el = nb * C;
    for (int e0 = lane; e0 < n_el + lane; e0 += SG_UNROLL * R3D_WAVE) {  // (uniform trip count)
      float v[SG_UNROLL], d[SG_UNROLL];
#pragma unroll
      for (int u = 0; u < SG_UNROLL; ++u) {  // past the end: the batch's last element again, loaded and dropped
        const int e = e0 + u * R3D_WAVE < n_el ? e0 + u * R3D_WAVE : n_el - 1;
        const int row = e / C, col = e - row * C;
        v[u] = scores[(long)row_p[w][r0 + row] * C + col];
        d[u] = row_v[w][r0 + row];
      }
#pragma unroll
      for (int u = 0; u < SG_UNROLL; ++u)
        if (e0 + u * R3D_WAVE < n_el) stage[w][e0 + u * R3D_WAVE] = __fdiv_rn(v[u], d[u]);
    }
    __syncthreads();
    if (lane < C) {
#pragma unroll 8
      for (int r = 0; r < nb; ++r) {
        const float v = stage[w][r * C + lane];
        acc = (r0 + r == 0) ? v : __fadd_rn(acc, v);
      }
    }
    __syncthreads();
  }
  if (t < n_tiles && lane < C) part[(long)t * C + lane] = acc;
}

// One wave per segment: lane j adds column j of the segment's tile partials in tile order, divides by the members and
// every lane takes the arg-max over the columns (P4).
__global__ __launch_bounds__(SC_THREADS) void r3d_scene_seg_pool_final_kernel(
    int S, int C, const float* __restrict__ part, const int* __restrict__ cstart, const int* __restrict__ seg_start,
    const int* __restrict__ tiles, const int* __restrict__ seg_id, long long* __restrict__ ids, int* __restrict__ points,
    int* __restrict__ members, float* __restrict__ seg_scores, long long* __restrict__ seg_labels /* or null */, int M,
    int n_tiles) {
  const int lane = threadIdx.x & 63;
  const int s = blockIdx.x * SG_WAVES + (threadIdx.x >> 6);
  if (s >= S) return;
  const int n = cstart[s + 1] - cstart[s];
  const int t0 = sc_clamp(tiles[sc_clamp(seg_start[s], 0, M)], 0, n_tiles);
  const int t1 = sc_clamp(tiles[sc_clamp(seg_start[s + 1], 0, M)], 0, n_tiles);
  float mean = 0.0f;
  if (lane < C && n > 0 && t1 > t0) {
    float tot = part[(long)t0 * C + lane];
    for (int tb = t0 + 1; tb < t1; tb += SG_UNROLL) {  // the loads of SG_UNROLL partials go out together, the additions stay in order
      float v[SG_UNROLL];
#pragma unroll
      for (int u = 0; u < SG_UNROLL; ++u) v[u] = part[(long)(tb + u < t1 ? tb + u : t1 - 1) * C + lane];
#pragma unroll
      for (int u = 0; u < SG_UNROLL; ++u)
        if (tb + u < t1) tot = __fadd_rn(tot, v[u]);
    }
    mean = __fdiv_rn(tot, (float)n);
  }
  if (lane < C) seg_scores[(long)s * C + lane] = mean;
  int best = -1;
  float best_v = 0.0f;
  for (int j = 0; j < C; ++j) {
    const float v = __shfl(mean, j);
    if (n > 0) sc_argmax_step(j, v, best, best_v);
  }
  if (lane == 0) {
    ids[s] = (long long)seg_id[s];
    points[s] = seg_start[s + 1] - seg_start[s];
    members[s] = n;
    if (seg_labels) seg_labels[s] = best;
  }
}

extern "C" int r3d_scene_seg_pool(long M, int n_cols, const float* scores, const int32_t* votes, long n_segments, long n_tiles,
                                  const int32_t* ws, long ws_words, float* part, int64_t* seg_ids, int32_t* seg_points,
                                  int32_t* seg_members, float* seg_scores, int64_t* seg_labels, void* stream) {
  R3D_REQUIRE(scores && votes && ws, "r3d_scene_seg_pool: null pointer (scores %p, votes %p, ws %p)", (const void*)scores,
              (const void*)votes, (const void*)ws);
  R3D_REQUIRE(M > 0 && M <= SC_MAX_POINTS, "r3d_scene_seg_pool: M %ld (1 .. 2^27 points)", M);
  R3D_REQUIRE(n_cols >= 1 && n_cols <= 64, "r3d_scene_seg_pool: %d score columns (1 .. 64)", n_cols);
  R3D_REQUIRE(n_segments >= 0 && n_segments <= M && n_tiles >= 0 && n_tiles <= M,
              "r3d_scene_seg_pool: %ld segments, %ld tiles of %ld points", n_segments, n_tiles, M);
  R3D_REQUIRE(ws_words >= r3d_scene_seg_ws_words(M), "r3d_scene_seg_pool: workspace of %ld words, %ld needed", ws_words,
              r3d_scene_seg_ws_words(M));
  R3D_REQUIRE(n_segments == 0 || (seg_ids && seg_points && seg_members && seg_scores),
              "r3d_scene_seg_pool: null pointer (seg_ids %p, seg_points %p, seg_members %p, seg_scores %p)", (void*)seg_ids,
              (void*)seg_points, (void*)seg_members, (void*)seg_scores);
  R3D_REQUIRE(n_tiles == 0 || part, "r3d_scene_seg_pool: null pointer (part)");
  const hipStream_t st = (hipStream_t)stream;
  const sg_layout L = sg_make_layout(M);
  if (n_tiles > 0)
    hipLaunchKernelGGL(r3d_scene_seg_pool_tiles_kernel, dim3((int)((n_tiles + SG_WAVES - 1) / SG_WAVES)), dim3(SC_THREADS), 0, st,
                       (int)n_tiles, n_cols, (int)M, scores, votes, ws + L.clist, ws + L.cstart, ws + L.seg_start, ws + L.tiles,
                       ws + L.tile_seg, part);
  if (n_segments > 0)
    hipLaunchKernelGGL(r3d_scene_seg_pool_final_kernel, dim3((int)((n_segments + SG_WAVES - 1) / SG_WAVES)), dim3(SC_THREADS), 0,
                       st, (int)n_segments, n_cols, part, ws + L.cstart, ws + L.seg_start, ws + L.tiles, ws + L.seg_id,
                       (long long*)seg_ids, seg_points, seg_members, seg_scores, (long long*)seg_labels, (int)M, (int)n_tiles);
  R3D_LAUNCH_CHECK("r3d_scene_seg_pool");
  return R3D_OK;
}

// what a point of the scan holds, in res (in) and in the result (out); the set fields are null for a SceneResult
struct sg_point_fields {
  const float* scores;
  const long long* labels;
  const long long* set_labels;
  const int* set_of;
  const float* margin;
};

// P5, 256 scan points per round of a workgroup.  One thread per point decides: it reads its segment's row index, writes
// its label, flag and set fields and leaves the row its scores come from in LDS; then the workgroup copies the 256 rows
// with consecutive lanes on consecutive floats (one lane per row wrote 4-byte pieces 4 * C bytes apart).  At most
// SG_COUNT_BLOCKS workgroups, one integer atomic per count and workgroup.
__global__ __launch_bounds__(SC_THREADS) void r3d_scene_seg_spread_kernel(
    int M, int C, int K, int S, int min_members, const int* __restrict__ segment_index, const int* __restrict__ members,
    sg_point_fields seg, sg_point_fields in, float* __restrict__ scores, long long* __restrict__ labels,
    unsigned char* __restrict__ pooled, long long* __restrict__ set_labels, int* __restrict__ set_of, float* __restrict__ margin,
    int* __restrict__ rec) {
  __shared__ int src[SC_THREADS];  // the segment row a point's scores come from, -1: its own row of res
  __shared__ int red[SG_WAVES];
  int n_pl = 0, n_fi = 0, n_un = 0;
  for (long base = (long)blockIdx.x * SC_THREADS; base < M; base += (long)gridDim.x * SC_THREADS) {  // (uniform)
    const long p = base + threadIdx.x;
    int from = -1;
    if (p < M) {
      const int s = segment_index[p];
      const bool pl = s >= 0 && s < S && members[s] >= min_members;
      const sg_point_fields& f = pl ? seg : in;
      const long r = pl ? s : p;
      const long long lab = f.labels[r];
      labels[p] = lab;
      pooled[p] = pl ? 1 : 0;
      if (K > 0) {
        for (int k = 0; k < K; ++k) set_labels[p * K + k] = f.set_labels[r * K + k];
        set_of[p] = f.set_of[r];
        margin[p] = f.margin[r];
      }
      from = pl ? s : -1;
      n_pl += pl;
      n_fi += pl && in.labels[p] == -1;
      n_un += lab == -1;
    }
    src[threadIdx.x] = from;
    __syncthreads();
    const long left = M - base;
    const int n_el = (int)(left < SC_THREADS ? left : SC_THREADS) * C;
    for (int e = threadIdx.x; e < n_el; e += SC_THREADS) {
      const int q = e / C, j = e - q * C, s = src[q];
      scores[base * C + e] = s >= 0 ? seg.scores[(long)s * C + j] : in.scores[base * C + e];
    }
    __syncthreads();
  }
  n_pl = sg_block_count(n_pl, red);
  n_fi = sg_block_count(n_fi, red);
  n_un = sg_block_count(n_un, red);
  if (threadIdx.x == 0) {  // integer counts: order-independent
    if (n_pl > 0) atomicAdd(&rec[SG_R_NPOOLED], n_pl);
    if (n_fi > 0) atomicAdd(&rec[SG_R_NFILLED], n_fi);
    if (n_un > 0) atomicAdd(&rec[SG_R_NUNLAB], n_un);
  }
}

extern "C" int r3d_scene_seg_spread(long M, int n_cols, int n_sets, long n_segments, int min_members, const int32_t* segment_index,
                                    const int32_t* seg_members, const float* seg_scores, const int64_t* seg_labels,
                                    const int64_t* seg_set_labels, const int32_t* seg_set_of, const float* seg_margin,
                                    const float* in_scores, const int64_t* in_labels, const int64_t* in_set_labels,
                                    const int32_t* in_set_of, const float* in_margin, float* scores, int64_t* labels,
                                    uint8_t* pooled, int64_t* set_labels, int32_t* set_of, float* margin, int32_t* ws,
                                    long ws_words, void* stream) {
  R3D_REQUIRE(segment_index && in_scores && in_labels && scores && labels && pooled && ws,
              "r3d_scene_seg_spread: null pointer (segment_index %p, in_scores %p, in_labels %p, scores %p, labels %p, pooled %p, "
              "ws %p)", (const void*)segment_index, (const void*)in_scores, (const void*)in_labels, (void*)scores, (void*)labels,
              (void*)pooled, (void*)ws);
  R3D_REQUIRE(M > 0 && M <= SC_MAX_POINTS, "r3d_scene_seg_spread: M %ld (1 .. 2^27 points)", M);
  R3D_REQUIRE(n_cols >= 1 && n_cols <= 64, "r3d_scene_seg_spread: %d score columns (1 .. 64)", n_cols);
  R3D_REQUIRE(n_sets >= 0 && n_sets <= 32 && (n_sets == 0 || n_cols % n_sets == 0),
              "r3d_scene_seg_spread: %d sets over %d score columns", n_sets, n_cols);
  R3D_REQUIRE(min_members >= 1, "r3d_scene_seg_spread: min_members %d (at least 1)", min_members);
  R3D_REQUIRE(n_segments >= 0 && n_segments <= M, "r3d_scene_seg_spread: %ld segments of %ld points", n_segments, M);
  R3D_REQUIRE(n_segments == 0 || (seg_members && seg_scores && seg_labels),
              "r3d_scene_seg_spread: null pointer (seg_members %p, seg_scores %p, seg_labels %p)", (const void*)seg_members,
              (const void*)seg_scores, (const void*)seg_labels);
  R3D_REQUIRE(n_sets == 0 || (in_set_labels && in_set_of && in_margin && set_labels && set_of && margin &&
                              (n_segments == 0 || (seg_set_labels && seg_set_of && seg_margin))),
              "r3d_scene_seg_spread: with sets, set_labels, set_of and margin are needed for the segments, res and the result");
  R3D_REQUIRE(ws_words >= r3d_scene_seg_ws_words(M), "r3d_scene_seg_spread: workspace of %ld words, %ld needed", ws_words,
              r3d_scene_seg_ws_words(M));
  const sg_layout L = sg_make_layout(M);
  const sg_point_fields seg = {seg_scores, (const long long*)seg_labels, (const long long*)seg_set_labels, seg_set_of, seg_margin};
  const sg_point_fields in = {in_scores, (const long long*)in_labels, (const long long*)in_set_labels, in_set_of, in_margin};
  hipLaunchKernelGGL(r3d_scene_seg_spread_kernel, dim3(sg_count_grid(M)), dim3(SC_THREADS), 0,
                     (hipStream_t)stream, (int)M, n_cols, n_sets, (int)n_segments, min_members, segment_index, seg_members, seg, in,
                     scores, (long long*)labels, pooled, (long long*)set_labels, set_of, margin, ws + L.rec);
  R3D_LAUNCH_CHECK("r3d_scene_seg_spread");
  return R3D_OK;
}

// ------------------------------------------------------------------------------------------------ segments grown on the device
// build_segments ("Building segments", G1-G7): the partition that pool_segments takes, grown from the scan
// itself.  Points fall into voxels, occupied voxels that touch (and, with a tolerance, whose mean colours agree; with
// normal_tol, whose normals agree) are joined, the connected components are the segments.
//   bounds      valid points, their xyz extent                                    -> words 0 .. 6 of the record (read 1)
//   sort        voxel keys, the stable radix sort above on (key, scan index), voxel heads as flags, their scan
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
//   ids         the kept components numbered in ascending root order, spread to the points   -> the counts (read 4)
// The union-find holds integers only and the component of a voxel depends on the graph alone: whichever thread hooks
// first, the root of a component ends as its smallest row.  Floats are added by __fadd_rn in the stated order.
#define GR_AXIS_MAX 1024  // voxels per axis: keys stay below 2^30
// the record, words of ws[0 .. 16)
#define GR_R_MIN 0        // x0 y0 z0 (float bits)
#define GR_R_MAX 3        // the maxima (float bits)
#define GR_R_NVALID 6
#define GR_R_V 7          // occupied voxels
#define GR_R_NCOMP 8      // components
#define GR_R_S 9          // kept components
#define GR_R_NDROPPED 10  // points of dropped components
#define GR_R_ERROR 11     // != 0: a bounded loop of the union-find ran out (bit 0 a find, bit 1 a unite)

struct gr_layout {
  long rec;              // 16
  long bpart;            // 7 * SC_BOUNDS_BLOCKS: partial bounds
  long key[2], idx[2];   // ping-pong pairs of the sort; key of the pair the sort leaves free: the voxel heads, scanned
  long hist, part;
  long vkey;             // V: key of a voxel row
  long vstart;           // V + 1: first sorted position of a voxel
  long parent, root;     // V each
  long cnt;              // V: points of the component, at its root
  long kept;             // V + 1: kept roots in front of a voxel row
  long total;
  int n_tiles, n_part, n_scan;
};

static gr_layout gr_make_layout(long M) {
  gr_layout L;
  const long Ma = sc_align(M + 1);
  long o = 0;
  L.n_tiles = (int)((M + SC_TILE - 1) / SC_TILE);
  const long n_hist = 256L * L.n_tiles;
  L.n_part = (int)((n_hist + SC_TILE - 1) / SC_TILE);
  L.n_scan = (int)((M + 1 + SC_TILE - 1) / SC_TILE);
  L.rec = o; o += 16;
  L.bpart = o; o += sc_align(7L * SC_BOUNDS_BLOCKS);
  L.key[0] = o; o += Ma;
  L.key[1] = o; o += Ma;
  L.idx[0] = o; o += Ma;
  L.idx[1] = o; o += Ma;
  L.hist = o; o += sc_align(n_hist);
  L.part = o; o += sc_align(L.n_part > L.n_scan ? L.n_part : L.n_scan);
  L.vkey = o; o += Ma;
  L.vstart = o; o += Ma;
  L.parent = o; o += Ma;
  L.root = o; o += Ma;
  L.cnt = o; o += Ma;
  L.kept = o; o += Ma;
  L.total = o;
  return L;
}

extern "C" long r3d_scene_grow_ws_words(long M) { return M > 0 && M <= SC_MAX_POINTS ? gr_make_layout(M).total : -1; }

static int gr_passes(long n_cells) {  // keys run 0 .. n_cells (n_cells: invalid point)
  return n_cells < 256 ? 1 : (n_cells < 65536 ? 2 : (n_cells < (1L << 24) ? 3 : 4));
}

// what every entry point after the bounds has: the scan's size, the grid and the workspace
static int gr_check(const char* name, long M, int nx, int ny, int nz, const int32_t* ws, long ws_words) {
  R3D_REQUIRE(ws, "%s: null pointer (ws)", name);
  R3D_REQUIRE(M > 0 && M <= SC_MAX_POINTS, "%s: M %ld (1 .. 2^27 points)", name, M);
  R3D_REQUIRE(nx >= 1 && nx <= GR_AXIS_MAX && ny >= 1 && ny <= GR_AXIS_MAX && nz >= 1 && nz <= GR_AXIS_MAX,
              "%s: %d x %d x %d voxels (1 .. 1024 per axis)", name, nx, ny, nz);
  R3D_REQUIRE(ws_words >= r3d_scene_grow_ws_words(M), "%s: workspace of %ld words, %ld needed", name, ws_words,
              r3d_scene_grow_ws_words(M));
  return R3D_OK;
}

// ---- bounds: r3d_scene_bounds with z (that one's record and bits stay as they are)
__global__ __launch_bounds__(SC_THREADS) void r3d_scene_grow_bounds_part_kernel(const float* __restrict__ scan, int ld, int M,
                                                                                float* __restrict__ part) {
  __shared__ float red[7][SC_THREADS / R3D_WAVE];
  float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  int n = 0;
  for (int i = blockIdx.x * SC_THREADS + threadIdx.x; i < M; i += gridDim.x * SC_THREADS) {
    const float* p = scan + (long)i * ld;
    const float v[3] = {p[0], p[1], p[2]};
    if (sc_finite3(v[0], v[1], v[2])) {
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        mn[a] = fminf(mn[a], v[a]);
        mx[a] = fmaxf(mx[a], v[a]);
      }
      ++n;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      mn[a] = fminf(mn[a], __shfl_xor(mn[a], o));
      mx[a] = fmaxf(mx[a], __shfl_xor(mx[a], o));
    }
    n += __shfl_xor(n, o);
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      red[a][w] = mn[a];
      red[3 + a][w] = mx[a];
    }
    red[6][w] = __int_as_float(n);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < SC_THREADS / R3D_WAVE; ++k) {
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        mn[a] = fminf(mn[a], red[a][k]);
        mx[a] = fmaxf(mx[a], red[3 + a][k]);
      }
      n += __float_as_int(red[6][k]);
    }
    float* o = part + 7L * blockIdx.x;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      o[a] = mn[a];
      o[3 + a] = mx[a];
    }
    o[6] = __int_as_float(n);
  }
}

// one wave: the partials -> words 0 .. 6 of the record; the other words of the record start at 0
__global__ __launch_bounds__(R3D_WAVE) void r3d_scene_grow_bounds_final_kernel(const float* __restrict__ part, int n_part,
                                                                               float* __restrict__ rec) {
  float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  int n = 0;
  for (int i = threadIdx.x; i < n_part; i += R3D_WAVE) {
    const float* p = part + 7L * i;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      mn[a] = fminf(mn[a], p[a]);
      mx[a] = fmaxf(mx[a], p[3 + a]);
    }
    n += __float_as_int(p[6]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      mn[a] = fminf(mn[a], __shfl_xor(mn[a], o));
      mx[a] = fmaxf(mx[a], __shfl_xor(mx[a], o));
    }
    n += __shfl_xor(n, o);
  }
  if (threadIdx.x == 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      rec[GR_R_MIN + a] = mn[a];
      rec[GR_R_MAX + a] = mx[a];
    }
    rec[GR_R_NVALID] = __int_as_float(n);
    for (int k = GR_R_NVALID + 1; k < 16; ++k) rec[k] = 0.0f;
  }
}

extern "C" int r3d_scene_grow_bounds(const float* scan, int ld, long M, int32_t* ws, long ws_words, void* stream) {
  R3D_REQUIRE(scan, "r3d_scene_grow_bounds: null pointer (scan)");
  SC_TRY(sc_check_ld("r3d_scene_grow_bounds", ld));
  SC_TRY(gr_check("r3d_scene_grow_bounds", M, 1, 1, 1, ws, ws_words));
  const gr_layout L = gr_make_layout(M);
  const int nb = sc_bounds_blocks(M);
  float* part = (float*)(ws + L.bpart);
  hipLaunchKernelGGL(r3d_scene_grow_bounds_part_kernel, dim3(nb), dim3(SC_THREADS), 0, (hipStream_t)stream, scan, ld, (int)M, part);
  hipLaunchKernelGGL(r3d_scene_grow_bounds_final_kernel, dim3(1), dim3(R3D_WAVE), 0, (hipStream_t)stream, part, nb,
                     (float*)(ws + L.rec));
  R3D_LAUNCH_CHECK("r3d_scene_grow_bounds");
  return R3D_OK;
}

// ---- sort: keys (G2), the sort, the voxel heads and their scan
struct gr_grid {
  float x0, y0, z0, s;
  int nx, ny, nz;
};

__global__ __launch_bounds__(SC_THREADS) void r3d_scene_grow_keys_kernel(const float* __restrict__ scan, int ld, int M, gr_grid g,
                                                                         int* __restrict__ key, int* __restrict__ idx) {
  const int i = blockIdx.x * SC_THREADS + threadIdx.x;
  if (i >= M) return;
  const float* p = scan + (long)i * ld;
  const float x = p[0], y = p[1], z = p[2];
  int k = g.nx * g.ny * g.nz;  // invalid points sort behind every voxel
  if (sc_finite3(x, y, z)) k = (sc_cell(z, g.z0, g.s, g.nz) * g.ny + sc_cell(y, g.y0, g.s, g.ny)) * g.nx + sc_cell(x, g.x0, g.s, g.nx);
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

extern "C" int r3d_scene_grow_sort(const float* scan, int ld, long M, float x0, float y0, float z0, float voxel, int nx, int ny,
                                   int nz, int32_t* ws, long ws_words, void* stream) {
  R3D_REQUIRE(scan, "r3d_scene_grow_sort: null pointer (scan)");
  SC_TRY(sc_check_ld("r3d_scene_grow_sort", ld));
  SC_TRY(gr_check("r3d_scene_grow_sort", M, nx, ny, nz, ws, ws_words));
  R3D_REQUIRE(x0 == x0 && y0 == y0 && z0 == z0 && voxel > 0.0f && voxel < INFINITY,
              "r3d_scene_grow_sort: origin (%g, %g, %g), voxel size %g", (double)x0, (double)y0, (double)z0, (double)voxel);
  const hipStream_t st = (hipStream_t)stream;
  const gr_layout L = gr_make_layout(M);
  const int n_cells = nx * ny * nz;
  const gr_grid g = {x0, y0, z0, voxel, nx, ny, nz};
  const int gm = (int)((M + SC_THREADS - 1) / SC_THREADS), gm1 = (int)((M + 1 + SC_THREADS - 1) / SC_THREADS);
  hipLaunchKernelGGL(r3d_scene_grow_keys_kernel, dim3(gm), dim3(SC_THREADS), 0, st, scan, ld, (int)M, g, ws + L.key[0],
                     ws + L.idx[0]);
  const int sorted = sc_sort_pairs(ws, L.key, L.idx, L.hist, L.part, M, L.n_tiles, gr_passes(n_cells), st);
  int* heads = ws + L.key[sorted ^ 1];
  hipLaunchKernelGGL(r3d_scene_grow_heads_kernel, dim3(gm1), dim3(SC_THREADS), 0, st, ws + L.key[sorted], (int)M, n_cells, heads);
  sc_excl_scan(heads, M + 1, ws + L.part, st);
  hipLaunchKernelGGL(r3d_scene_grow_word_kernel, dim3(1), dim3(1), 0, st, heads + M, ws + L.rec + GR_R_V);
  R3D_LAUNCH_CHECK("r3d_scene_grow_sort");
  return R3D_OK;
}

// ---- voxels: the table (G3)
// after the scan: heads[i] = voxels opened in front of i.  A voxel's row is written by the thread of its first sorted
// position, row V of vstart by the thread of position M.
__global__ __launch_bounds__(SC_THREADS) void r3d_scene_grow_table_kernel(const int* __restrict__ skey, const int* __restrict__ order,
                                                                          int M, int n_cells, int V, int n_valid,
                                                                          const int* __restrict__ heads, int* __restrict__ vkey,
                                                                          int* __restrict__ vstart, int* __restrict__ voxel_index) {
  const int i = blockIdx.x * SC_THREADS + threadIdx.x;
  if (i > M) return;
  if (i == M) {
    vstart[V] = n_valid;
    return;
  }
  const int k = skey[i], v = heads[i + 1] - 1;
  const bool in = k >= 0 && k < n_cells && v >= 0 && v < V;
  const int p = sc_clamp(order[i], 0, M - 1);
  voxel_index[p] = in ? v : -1;
  if (in && heads[i + 1] != heads[i]) {
    vkey[v] = k;
    vstart[v] = i;
  }
}

// One thread per voxel: its points in sorted order (ascending scan index: the sort is stable), three values per point
// (row(p, c): those of scan row p) summed as the segment pool sums a segment whose rows all have one vote.
template <class Row>
static __device__ __forceinline__ void gr_voxel_mean(int v, int M, const int* __restrict__ order, const int* __restrict__ vstart,
                                                     float* __restrict__ mean, Row row) {
  const int a = sc_clamp(vstart[v], 0, M), b = sc_clamp(vstart[v + 1], a, M);
  float tot[3] = {0.0f, 0.0f, 0.0f};
  for (int t0 = a; t0 < b; t0 += SG_TILE) {
    const int t1 = t0 + SG_TILE < b ? t0 + SG_TILE : b;
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

struct gr_view {
  const int *skey, *order, *heads;
  gr_layout L;
};

static gr_view gr_make_view(long M, int nx, int ny, int nz, const int32_t* ws) {
  gr_view v;
  v.L = gr_make_layout(M);
  const int sorted = gr_passes((long)nx * ny * nz) & 1;
  v.skey = ws + v.L.key[sorted];
  v.order = ws + v.L.idx[sorted];
  v.heads = ws + v.L.key[sorted ^ 1];
  return v;
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
  const gr_view v = gr_make_view(M, nx, ny, nz, ws);
  const int gm1 = (int)((M + 1 + SC_THREADS - 1) / SC_THREADS);
  hipLaunchKernelGGL(r3d_scene_grow_table_kernel, dim3(gm1), dim3(SC_THREADS), 0, st, v.skey, v.order, (int)M, nx * ny * nz,
                     (int)n_voxels, (int)n_valid, v.heads, ws + v.L.vkey, ws + v.L.vstart, voxel_index);
  if (colour && n_voxels > 0)
    hipLaunchKernelGGL(r3d_scene_grow_mean_kernel, dim3((int)((n_voxels + SC_THREADS - 1) / SC_THREADS)), dim3(SC_THREADS), 0, st,
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
  R3D_REQUIRE(x0 == x0 && y0 == y0 && z0 == z0 && voxel > 0.0f && voxel < INFINITY,
              "r3d_scene_grow_centroids: origin (%g, %g, %g), voxel size %g", (double)x0, (double)y0, (double)z0, (double)voxel);
  R3D_REQUIRE(n_voxels >= 1 && n_voxels <= M, "r3d_scene_grow_centroids: %ld voxels of %ld points", n_voxels, M);
  const gr_view v = gr_make_view(M, nx, ny, nz, ws);
  const gr_grid g = {x0, y0, z0, voxel, nx, ny, nz};
  hipLaunchKernelGGL(r3d_scene_grow_centroid_kernel, dim3((int)((n_voxels + SC_THREADS - 1) / SC_THREADS)), dim3(SC_THREADS), 0,
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

// One thread per voxel.  The three x-neighbours of one (dz, dy) row have consecutive keys: one binary search finds the
// first candidate row of the table, the next two are checked by key, and an x outside the grid is never looked up, so a
// key that belongs to the neighbouring row of the grid is no neighbour.  The 27 rows stay in registers (every loop over
// them is unrolled, no index is a run-time value); the centroids are gathered once for the mean and once more for the
// second moments.
__global__ __launch_bounds__(SC_THREADS) void r3d_scene_grow_normals_kernel(int V, int nx, int ny, int nz, float s,
                                                                            const int* __restrict__ vkey,
                                                                            const float* __restrict__ centroid,
                                                                            float* __restrict__ normal, int* __restrict__ support) {
  const int v = blockIdx.x * SC_THREADS + threadIdx.x;
  if (v >= V) return;
  const int key = vkey[v];
  const int ix = key % nx, iy = (key / nx) % ny, iz = key / (nx * ny);
  int nb[27];
  int k = 0;
#pragma unroll
  for (int r = 0; r < 9; ++r) {
    const int jy = iy + r % 3 - 1, jz = iz + r / 3 - 1;
    nb[3 * r] = nb[3 * r + 1] = nb[3 * r + 2] = -1;
    if (jy < 0 || jy >= ny || jz < 0 || jz >= nz) continue;
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
        nb[3 * r + d] = lo;
        ++lo;
        ++k;
      }
    }
  }
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
  R3D_REQUIRE(n_voxels >= 1 && n_voxels <= M, "r3d_scene_grow_normals: %ld voxels of %ld points", n_voxels, M);
  const gr_layout L = gr_make_layout(M);
  hipLaunchKernelGGL(r3d_scene_grow_normals_kernel, dim3((int)((n_voxels + SC_THREADS - 1) / SC_THREADS)), dim3(SC_THREADS), 0,
                     (hipStream_t)stream, (int)n_voxels, nx, ny, nz, voxel, ws + L.vkey, voxel_centroid, voxel_normal,
                     voxel_support);
  R3D_LAUNCH_CHECK("r3d_scene_grow_normals");
  return R3D_OK;
}

// ---- union (G4, G5)
// parent[] is changed inside this launch by agent-scope atomics only and read by relaxed agent-scope atomic loads: the
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

__global__ __launch_bounds__(SC_THREADS) void r3d_scene_grow_init_kernel(int V, int* __restrict__ parent) {
  const int v = blockIdx.x * SC_THREADS + threadIdx.x;
  if (v < V) parent[v] = v;
}

// One thread per voxel a, the forward half of the neighbourhood (the offsets whose key is larger): 3 of 6, 13 of 26.  The
// neighbour's coordinates are checked against the grid, its key is looked up by binary search among the rows behind a.
// NORMALS (r3d_scene_grow_union_normals): a pair is joined only when dot^2 >= (cos2 la) lb as well, la and lb the squared
// lengths of the two normal rows; a NaN in either row makes the comparison false.
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
  for (int o = 14; o < 27; ++o) {  // (dz, dy, dx) in lexicographic order behind (0, 0, 0)
    const int dx = o % 3 - 1, dy = (o / 3) % 3 - 1, dz = o / 9 - 1;
    if (conn == 6 && (dx != 0) + (dy != 0) + (dz != 0) != 1) continue;
    const int jx = ix + dx, jy = iy + dy, jz = iz + dz;
    if (jx < 0 || jx >= nx || jy < 0 || jy >= ny || jz < 0 || jz >= nz) continue;
    const int want = (jz * ny + jy) * nx + jx;
    int lo = a + 1, hi = V;  // the first row in (a, V) whose key is not below `want`
    while (lo < hi) {
      const int mid = lo + ((hi - lo) >> 1);
      if (vkey[mid] < want) lo = mid + 1; else hi = mid;
    }
    if (lo >= V || vkey[lo] != want) continue;
    if (use_colour) {
      bool alike = true;
#pragma unroll
      for (int j = 0; j < 3; ++j) alike = alike && fabsf(__fsub_rn(ma[j], mean[3L * lo + j])) <= tol;  // a NaN joins nothing
      if (!alike) continue;
    }
    if (NORMALS) {
      const float nb[3] = {normal[3L * lo], normal[3L * lo + 1], normal[3L * lo + 2]};
      const float dot = gr_dot3(na, nb);
      if (!(__fmul_rn(dot, dot) >= __fmul_rn(la, gr_dot3(nb, nb)))) continue;
    }
    gr_unite(parent, a, lo, V, err);
  }
}

static int gr_union(const char* name, long M, int nx, int ny, int nz, long n_voxels, int connectivity, const float* voxel_mean,
                    float colour_tol, const float* voxel_normal, float cos2, int32_t* ws, long ws_words, void* stream) {
  const bool colour = voxel_mean != nullptr;
  SC_TRY(gr_check(name, M, nx, ny, nz, ws, ws_words));
  R3D_REQUIRE(n_voxels >= 1 && n_voxels <= M, "%s: %ld voxels of %ld points", name, n_voxels, M);
  R3D_REQUIRE(connectivity == 6 || connectivity == 26, "%s: connectivity %d (6 or 26)", name, connectivity);
  R3D_REQUIRE(!colour || (colour_tol >= 0.0f && colour_tol < INFINITY), "%s: colour_tol %g (finite, >= 0)", name,
              (double)colour_tol);
  const hipStream_t st = (hipStream_t)stream;
  const gr_layout L = gr_make_layout(M);
  const int V = (int)n_voxels, gv = (V + SC_THREADS - 1) / SC_THREADS;
  hipLaunchKernelGGL(r3d_scene_grow_init_kernel, dim3(gv), dim3(SC_THREADS), 0, st, V, ws + L.parent);
  if (voxel_normal)
    hipLaunchKernelGGL(r3d_scene_grow_union_kernel<true>, dim3(gv), dim3(SC_THREADS), 0, st, V, nx, ny, nz, connectivity,
                       ws + L.vkey, colour ? 1 : 0, colour_tol, voxel_mean, voxel_normal, cos2, ws + L.parent,
                       ws + L.rec + GR_R_ERROR);
  else
    hipLaunchKernelGGL(r3d_scene_grow_union_kernel<false>, dim3(gv), dim3(SC_THREADS), 0, st, V, nx, ny, nz, connectivity,
                       ws + L.vkey, colour ? 1 : 0, colour_tol, voxel_mean, voxel_normal, cos2, ws + L.parent,
                       ws + L.rec + GR_R_ERROR);
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

// points per root: integer atomics, order-independent.  The lanes of a wave that share a root add their counts first and
// send one atomic: neighbouring rows mostly share a root, and one atomic per voxel onto the root of a component that
// holds most of the scan took 7.5 ms at 10^6 points (profiles/r22_scene_grow.md).
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
  const int lane = threadIdx.x & 63;
  unsigned long long todo = __ballot(live);
  while (todo) {  // (uniform) one round per distinct root of the wave
    const int leader = __ffsll((long long)todo) - 1;
    const int r0 = __shfl(r, leader);
    const bool mine = live && r == r0;
    int sum = mine ? n : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    if (lane == leader) atomicAdd(cnt + r0, sum);
    todo &= ~__ballot(mine);
  }
}

// row v: kept[v] = it is the root of a component with at least min_points points; word V is 0 for the scan's total
__global__ __launch_bounds__(SC_THREADS) void r3d_scene_grow_kept_kernel(int V, int min_points, const int* __restrict__ root,
                                                                         const int* __restrict__ cnt, int* __restrict__ kept,
                                                                         int* __restrict__ rec) {
  __shared__ int red[SG_WAVES];
  const int v = blockIdx.x * SC_THREADS + threadIdx.x;
  const bool is_root = v < V && root[v] == v;
  if (v <= V) kept[v] = is_root && cnt[v] >= min_points;
  const int n = sg_block_count(is_root ? 1 : 0, red);
  if (threadIdx.x == 0 && n > 0) atomicAdd(rec + GR_R_NCOMP, n);
}

extern "C" int r3d_scene_grow_components(long M, long n_voxels, int min_points, int32_t* ws, long ws_words, void* stream) {
  SC_TRY(gr_check("r3d_scene_grow_components", M, 1, 1, 1, ws, ws_words));
  R3D_REQUIRE(n_voxels >= 1 && n_voxels <= M, "r3d_scene_grow_components: %ld voxels of %ld points", n_voxels, M);
  R3D_REQUIRE(min_points >= 1, "r3d_scene_grow_components: min_points %d (at least 1)", min_points);
  const hipStream_t st = (hipStream_t)stream;
  const gr_layout L = gr_make_layout(M);
  const int V = (int)n_voxels, gv = (V + SC_THREADS - 1) / SC_THREADS, gv1 = (V + 1 + SC_THREADS - 1) / SC_THREADS;
  int* rec = ws + L.rec;
  r3d_zero_words(rec + GR_R_NCOMP, 2, st);
  r3d_zero_words(ws + L.cnt, V, st);
  hipLaunchKernelGGL(r3d_scene_grow_flatten_kernel, dim3(gv), dim3(SC_THREADS), 0, st, V, ws + L.parent, ws + L.root,
                     rec + GR_R_ERROR);
  hipLaunchKernelGGL(r3d_scene_grow_count_kernel, dim3(gv), dim3(SC_THREADS), 0, st, V, (int)M, ws + L.root, ws + L.vstart,
                     ws + L.cnt);
  hipLaunchKernelGGL(r3d_scene_grow_kept_kernel, dim3(gv1), dim3(SC_THREADS), 0, st, V, min_points, ws + L.root, ws + L.cnt,
                     ws + L.kept, rec);
  sc_excl_scan(ws + L.kept, V + 1L, ws + L.part, st);
  hipLaunchKernelGGL(r3d_scene_grow_word_kernel, dim3(1), dim3(1), 0, st, ws + L.kept + V, rec + GR_R_S);
  R3D_LAUNCH_CHECK("r3d_scene_grow_components");
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
  __shared__ int red[SG_WAVES];
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
  n_drop = sg_block_count(n_drop, red);
  if (threadIdx.x == 0 && n_drop > 0) atomicAdd(rec + GR_R_NDROPPED, n_drop);  // an integer count: order-independent
}

extern "C" int r3d_scene_grow_ids(long M, long n_voxels, long n_segments, const int32_t* voxel_index, int32_t* segments,
                                  int32_t* segment_points, int32_t* ws, long ws_words, void* stream) {
  SC_TRY(gr_check("r3d_scene_grow_ids", M, 1, 1, 1, ws, ws_words));
  R3D_REQUIRE(voxel_index && segments, "r3d_scene_grow_ids: null pointer (voxel_index %p, segments %p)", (const void*)voxel_index,
              (void*)segments);
  R3D_REQUIRE(n_voxels >= 1 && n_voxels <= M && n_segments >= 0 && n_segments <= n_voxels,
              "r3d_scene_grow_ids: %ld segments of %ld voxels of %ld points", n_segments, n_voxels, M);
  R3D_REQUIRE(n_segments == 0 || segment_points, "r3d_scene_grow_ids: null pointer (segment_points)");
  const hipStream_t st = (hipStream_t)stream;
  const gr_layout L = gr_make_layout(M);
  const int V = (int)n_voxels;
  r3d_zero_words(ws + L.rec + GR_R_NDROPPED, 1, st);
  if (n_segments > 0)
    hipLaunchKernelGGL(r3d_scene_grow_sizes_kernel, dim3((V + SC_THREADS - 1) / SC_THREADS), dim3(SC_THREADS), 0, st, V,
                       (int)n_segments, ws + L.kept, ws + L.cnt, segment_points);
  hipLaunchKernelGGL(r3d_scene_grow_spread_kernel, dim3(sg_count_grid(M)), dim3(SC_THREADS), 0, st, (int)M, V, voxel_index,
                     ws + L.root, ws + L.kept, segments, ws + L.rec);
  R3D_LAUNCH_CHECK("r3d_scene_grow_ids");
  return R3D_OK;
}
