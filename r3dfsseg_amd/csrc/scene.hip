// Labelling a whole scan against a fitted support set: the device side of scene.py (definition: INTEGRATION.md,
// "Labelling a scan").  The reference only scores clouds that were cut out of a room, sampled, min-shifted and given
// their channels on the host (dataloaders/loader.py:100-119); these kernels do that cutting on the device, without a
// random number, and sum the per-chunk logits back onto the scan points:
//   bounds   (scene_sort.hip) valid points, their xy extent              -> an 8-word record the host reads (read 1)
//   plan     cell keys, stable radix sort by key (scene_sort.hip), cell offsets, block sizes, chunk offsets, chunk table
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
// Everything here works on an sc_view of a plan's workspace.  All of it is bandwidth-bound integer and min / max work;
// the only floating-point sums are the vote's, one running sum per (point, class) in a fixed order.
#include "scene_common.h"

// record of r3d_scene_plan (ints)
#define SC_P_NCHUNKS 0
#define SC_P_NBLOCKS 1
#define SC_P_NVOTED 2
// the chunks that run: r3d_scene_plan writes {n_chunks, 0, voted}, r3d_scene_run_tables the counts under its cap
#define SC_P_NRUN 4
#define SC_P_NSKIPPED 5
#define SC_P_NVOTED_RUN 6
// transfer: R3D_SCENE_TRANSFER_QUERY_TILE queries per workgroup (one thread each), R3D_SCENE_TRANSFER_CAND_TILE candidate
// rows staged through LDS at a time (16 KiB)
// record of r3d_scene_transfer (ints, in the sparse workspace)
#define SC_T_NTRANSFERRED 0
#define SC_T_NTILES 1

// ------------------------------------------------------------------------------------------------ workspace layout
struct sc_layout {
  sc_sort_ws sort;      // the pairs of M words each; pos lies between them and the digit counts
  long pos;             // M: sorted position of every scan point
  long cell;           // n_cells + 2 cell offsets into the sorted order (cell n_cells: the invalid points)
  long blk_n;           // n_cells: points of a block (n_blocks <= n_cells)
  long chunk0;          // n_cells + 1: first chunk of a block (exclusive scan of the chunk counts)
  long chunk_blk;       // chunk_cap: block of a chunk
  long rec;             // 8
  long total;
  int passes, sorted;   // sorted: which of the two pairs holds the result
};

static sc_layout sc_make_layout(long M, long n_cells, long chunk_cap) {
  sc_layout L;
  const long Ma = sc_align(M);
  L.passes = sc_passes(n_cells);  // keys run 0 .. n_cells (n_cells: invalid point)
  L.sorted = L.passes & 1;
  long o = sc_sort_ws_append(L.sort, 0, M, Ma, sc_sort_part_words(M), Ma);
  L.pos = L.sort.idx[1] + Ma;
  L.cell = o; o += sc_align(n_cells + 2);
  L.blk_n = o; o += sc_align(n_cells);
  L.chunk0 = o; o += sc_align(n_cells + 1);
  L.chunk_blk = o; o += sc_align(chunk_cap);
  L.rec = o; o += 8;
  L.total = o;
  return L;
}

static bool sc_shape_ok(long M, int ncx, int ncy, int r, long chunk_cap) {
  return M > 0 && M <= R3D_SCENE_MAX_POINTS && ncx > 0 && ncy > 0 && (long)ncx * ncy <= R3D_SCENE_MAX_CELLS && r >= 1 && r <= 4 &&
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
};

static sp_layout sp_make_layout(long M, long n_cells, long chunk_cap) {
  sp_layout S;
  long o = 0;
  S.run0 = o; o += sc_align(n_cells + 1);
  S.run_blk = o; o += sc_align(chunk_cap);
  S.voff = o; o += sc_align(M + 1);
  S.part = o; o += sc_align(sc_tiles_of(M + 1));
  S.uq = o; o += sc_align(M);
  S.tile0 = o; o += sc_align(n_cells + 1);
  S.rec = o; o += 8;
  S.cand = o; o += 4 * M;
  S.total = o;
  return S;
}

// ------------------------------------------------------------------------------------------------ cell keys
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
  out[0] = L.sort.idx[L.sorted]; out[1] = L.sort.key[L.sorted]; out[2] = L.pos; out[3] = L.cell;
  out[4] = L.blk_n; out[5] = L.chunk0; out[6] = L.chunk_blk; out[7] = L.rec;
  return R3D_OK;
}

// ------------------------------------------------------------------------------------------------ argument checks, the plan on the host
// what every entry point that works on a plan has: the scan's size, the cells and the workspace
static int sc_check_plan(const char* name, long M, int ncx, int ncy, long chunk_cap, long ws_words) {
  SC_TRY(sc_check_points(name, M));
  R3D_REQUIRE(ncx > 0 && ncy > 0 && (long)ncx * ncy <= R3D_SCENE_MAX_CELLS, "%s: %d x %d cells (1 .. 65536)", name, ncx, ncy);
  R3D_REQUIRE(chunk_cap > 0 && chunk_cap < (1L << 30), "%s: chunk_cap %ld", name, chunk_cap);
  return sc_check_ws(name, ws_words, r3d_scene_ws_words(M, ncx, ncy, chunk_cap));
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
  v.order = ws + v.L.sort.idx[v.L.sorted];
  v.skey = ws + v.L.sort.key[v.L.sorted];
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
  const int gm = sc_grid_of(M);
  hipLaunchKernelGGL(r3d_scene_keys_kernel, dim3(gm), dim3(SC_THREADS), 0, st, scan, ld, (int)M, x0, y0, s, ncx, ncy,
                     ws + L.sort.key[0], ws + L.sort.idx[0]);
  sc_sort_pairs(ws, L.sort, M, L.passes, st);  // into pair L.sorted: v.skey, v.order
  hipLaunchKernelGGL(r3d_scene_cells_kernel, dim3(gm), dim3(SC_THREADS), 0, st, v.skey, v.order, (int)M, v.n_cells, ws + L.cell,
                     ws + L.pos);
  hipLaunchKernelGGL(r3d_scene_blocks_kernel, dim3(1), dim3(SC_PLAN_THREADS), 0, st, v.cell, v.g, N, min_points, ws + L.blk_n,
                     ws + L.chunk0, ws + L.rec);
  hipLaunchKernelGGL(r3d_scene_chunk_table_kernel, dim3(sc_grid_of(v.nb)), dim3(SC_THREADS), 0, st, v.chunk0,
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
  hipLaunchKernelGGL(r3d_scene_vote_kernel, dim3(sc_grid_of(M)), dim3(SC_THREADS), 0,
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
  hipLaunchKernelGGL(r3d_scene_chunk_table_kernel, dim3(sc_grid_of(v.nb)), dim3(SC_THREADS), 0, st, v.run0,
                     v.nb, (int)chunk_cap, sws + v.S.run_blk);
  hipLaunchKernelGGL(r3d_scene_run_count_kernel, dim3(sc_grid_of(M)), dim3(SC_THREADS), 0, st, (int)M,
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
//   tiles    per cell ceil(points without a vote / R3D_SCENE_TRANSFER_QUERY_TILE) query tiles, their exclusive scan
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
      t = u > 0 ? (u + R3D_SCENE_TRANSFER_QUERY_TILE - 1) / R3D_SCENE_TRANSFER_QUERY_TILE : 0;
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
__global__ __launch_bounds__(R3D_SCENE_TRANSFER_QUERY_TILE) void r3d_scene_transfer_kernel(
    const float* __restrict__ scan, int ld, int M, const int* __restrict__ cell, const int* __restrict__ voff,
    const int* __restrict__ uq, const int* __restrict__ tile0, const float4* __restrict__ cand, int ncx, int ncy, int K,
    float* __restrict__ scores, long long* __restrict__ labels, long long* __restrict__ source, int* __restrict__ rec,
    const int* __restrict__ votes, long long* __restrict__ neighbours, float* __restrict__ weights) {
  __shared__ float4 rows[R3D_SCENE_TRANSFER_CAND_TILE];
  const int n_cells = ncx * ncy, t = blockIdx.x, tid = threadIdx.x;
  if (t >= tile0[n_cells]) return;  // (uniform) the grid is an upper bound of the tiles
  int lo = 0, hi = n_cells;         // tile0[lo] <= t < tile0[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (tile0[mid] <= t) lo = mid; else hi = mid;
  }
  const int c = lo, cx = c % ncx, cy = c / ncx;
  const int s = sc_clamp(cell[c], 0, M), e = sc_clamp(cell[c + 1], s, M);
  const int u = (s - voff[s]) + (t - tile0[c]) * R3D_SCENE_TRANSFER_QUERY_TILE + tid;
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
    for (int base = a; base < b; base += R3D_SCENE_TRANSFER_CAND_TILE) {
      const int n = b - base < R3D_SCENE_TRANSFER_CAND_TILE ? b - base : R3D_SCENE_TRANSFER_CAND_TILE;
      __syncthreads();  // the previous tile has been read
      for (int k = tid; k < n; k += R3D_SCENE_TRANSFER_QUERY_TILE) rows[k] = cand[base + k];
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
  const int gm = sc_grid_of(M), gm1 = sc_grid_of(M + 1);
  hipLaunchKernelGGL(r3d_scene_transfer_flags_kernel, dim3(gm1), dim3(SC_THREADS), 0, st, (int)M, v.order, votes, sws + S.voff,
                     (long long*)source, (long long*)neighbours, weights);
  sc_excl_scan(sws + S.voff, M + 1, sws + S.part, st);
  hipLaunchKernelGGL(r3d_scene_transfer_compact_kernel, dim3(gm), dim3(SC_THREADS), 0, st, scan, ld, (int)M, v.order, votes,
                     sws + S.voff, cand, sws + S.uq);
  hipLaunchKernelGGL(r3d_scene_transfer_tiles_kernel, dim3(1), dim3(SC_PLAN_THREADS), 0, st, v.cell, sws + S.voff, v.n_cells,
                     (int)M, sws + S.tile0, sws + S.rec);
  // sum over the cells of ceil(u / R3D_SCENE_TRANSFER_QUERY_TILE) <= U / R3D_SCENE_TRANSFER_QUERY_TILE + cells that hold such a point
  const long tiles = M / R3D_SCENE_TRANSFER_QUERY_TILE + (v.n_cells < M ? v.n_cells : M) + 1;
  const auto kernel = neighbours ? r3d_scene_transfer_kernel<3> : r3d_scene_transfer_kernel<1>;
  hipLaunchKernelGGL(kernel, dim3((int)tiles), dim3(R3D_SCENE_TRANSFER_QUERY_TILE), 0, st, scan, ld, (int)M, v.cell, sws + S.voff, sws + S.uq,
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
  hipLaunchKernelGGL(r3d_scene_merge_sets_kernel, dim3(sc_grid_of(M)), dim3(SC_THREADS), 0,
                     (hipStream_t)stream, (int)M, n_sets, n_classes, scores, votes, (const long long*)source, classes,
                     (long long)background, (long long*)set_labels, (long long*)labels, set_of, margin);
  R3D_LAUNCH_CHECK("r3d_scene_merge_sets");
  return R3D_OK;
}

// ------------------------------------------------------------------------------------------------ a support set from an annotated scan
// fit_scene ("Fitting from an annotated scan"): the cloud of a block is its chunk 0 -- list positions
// 0, nc, 2 nc, ..., len = ceil(n / nc) members --; fg[b][w] counts the members labelled classes[w]; way w's shots are
// its eligible blocks (fg > max((int)floorf(len * min_ratio), min_fg)) by fg descending, block id ascending.
// One workgroup per block: threads stride over the len members, per way a ballot and a population count per wave, then
// the integer sum of the waves in LDS.  Every member counts once (wrap-around slots are not visited); dropped blocks get 0.
template <typename L>
__global__ __launch_bounds__(SC_THREADS) void r3d_scene_support_counts_kernel(
    const L* __restrict__ labels, int M, const int* __restrict__ order, const int* __restrict__ cell,
    const int* __restrict__ blk_n, const int* __restrict__ chunk0, sc_grid g, const int* __restrict__ classes, int n_way,
    int* __restrict__ fg) {
  __shared__ int wcnt[SC_THREADS / R3D_WAVE][R3D_SCENE_SUPPORT_MAX_WAYS + 1];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n = blk_n[b], nc = chunk0[b + 1] - chunk0[b];
  if (nc <= 0 || n <= 0) {  // (uniform) a dropped block
    if (tid < n_way) fg[(long)b * n_way + tid] = 0;
    return;
  }
  const int bx = b % g.nbx, by = b / g.nbx, len = (n + nc - 1) / nc;
  long long cls[R3D_SCENE_SUPPORT_MAX_WAYS];
  int acc[R3D_SCENE_SUPPORT_MAX_WAYS];
#pragma unroll
  for (int k = 0; k < R3D_SCENE_SUPPORT_MAX_WAYS; ++k) {
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
    for (int k = 0; k < R3D_SCENE_SUPPORT_MAX_WAYS; ++k)
      if (k < n_way) acc[k] += __popcll(__ballot(live && lab == cls[k]));  // the wave's count, the same in every lane
  }
  if ((tid & 63) == 0) {
#pragma unroll
    for (int k = 0; k < R3D_SCENE_SUPPORT_MAX_WAYS; ++k) wcnt[tid >> 6][k] = acc[k];
  }
  __syncthreads();
  if (tid < n_way) {
    int s = 0;
#pragma unroll
    for (int w = 0; w < SC_THREADS / R3D_WAVE; ++w) s += wcnt[w][tid];
    fg[(long)b * n_way + tid] = s;
  }
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
  R3D_REQUIRE(n_way >= 1 && n_way <= R3D_SCENE_SUPPORT_MAX_WAYS, name ": n_way %d (1 .. 7)", n_way)

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
  R3D_REQUIRE(G > 0 && G <= R3D_SCENE_MAX_CELLS, "r3d_scene_prepare_blocks: G %d (1 .. 65536 block ids)", G);
  R3D_REQUIRE((labels && cloud_class && mask) || (!labels && !cloud_class && !mask),
              "r3d_scene_prepare_blocks: labels %p, cloud_class %p and mask %p go together", labels, (const void*)cloud_class,
              (void*)mask);
  R3D_REQUIRE(!labels || label_bytes == 4 || label_bytes == 8, "r3d_scene_prepare_blocks: labels of %d bytes (int32 or int64)",
              label_bytes);
  const sc_block_args ba = {blocks, labels, label_bytes, cloud_class, mask};
  return sc_prepare(scan, ld, M, ncx, ncy, r, N, chunk_cap, ws, ws_words, nullptr, 0, G, C, rgb_ch, XYZ_ch, out, o_sb, o_sc, o_sn,
                    slot_map, stream, &ba);
}
