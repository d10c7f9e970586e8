// One label per segment: the device side of scene_segments.py.
// pool_segments ("Pooling scores over segments", P1-P5): the scan comes with a partition of its points
// (instance ids, supervoxels); per segment the mean of its contributors' mean logits, summed in a fixed order, then
// every point of a large enough segment takes its segment's row and label.
//   ids      largest legal id, negative ids, ids >= 2^31 - 1                    -> the record the host reads (read 1)
//   group    keys (a negative id: the one key above every id), the stable radix sort of scene_sort.hip on (id, scan
//            index), heads and contributors as flags, their integer scans, segment and tile tables   -> S, tiles (read 2)
//   pool     per tile of 256 contributor ranks one partial row, rows staged in LDS and added one at a time by the lane
//            that owns the column; per segment the partials added in tile order, one division, the arg-max
//   spread   per scan point its segment's row or its own                        -> the counts (read 3)
// Floats are added by __fadd_rn in the stated order and divided by __fdiv_rn; counts are integer scans and integer atomics.
#include "scene_common.h"

// a tile: R3D_SCENE_SEG_TILE contributor ranks
#define SG_BATCH 32    // rows of a tile staged in LDS at a time: 32 * 64 floats per wave, 32 KiB per workgroup
#define SG_UNROLL 8    // element loads of a lane in flight while a batch is staged; partials loaded ahead of their additions
#define SG_ID_LIMIT 2147483647LL
static_assert(R3D_SEG_R_BADMAX + 2 <= R3D_SCENE_SEG_REC && R3D_SEG_R_NUNLAB < R3D_SCENE_SEG_REC, "a word beyond the record");

struct sg_layout {
  long rec;              // R3D_SCENE_SEG_REC words, R3D_SEG_R_* (r3d.h)
  sc_sort_ws sort;       // pairs of M + 1 words; the pair the sort leaves free holds the two scans, part their partials too
  long tiles;            // M + 1: tile heads in front of a sorted position
  long clist;            // contributors' scan indices, segment after segment, ascending scan index inside one
  long seg_start;        // S + 1: first sorted position of a segment
  long cstart;           // S + 1: first entry of a segment in clist
  long seg_id;           // S
  long tile_seg;         // segment of a tile
  long total;
};

static sg_layout sg_make_layout(long M) {
  sg_layout L;
  const long Ma = sc_align(M + 1);
  long o = 0;
  L.rec = o; o += R3D_SCENE_SEG_REC;
  o = sc_sort_ws_append(L.sort, o, M, Ma, sc_sort_part_words(M, M + 1));
  L.tiles = o; o += Ma;
  L.clist = o; o += Ma;
  L.seg_start = o; o += Ma;
  L.cstart = o; o += Ma;
  L.seg_id = o; o += Ma;
  L.tile_seg = o; o += Ma;
  L.total = o;
  return L;
}

extern "C" long r3d_scene_seg_ws_words(long M) { return M > 0 && M <= R3D_SCENE_MAX_POINTS ? sg_make_layout(M).total : -1; }

// what every entry point has: the scan's size and the workspace
static int sg_check(const char* name, long M, long ws_words) {
  SC_TRY(sc_check_points(name, M));
  return sc_check_ws(name, ws_words, r3d_scene_seg_ws_words(M));
}

// At most SC_COUNT_BLOCKS workgroups stride over the ids and each ends in one atomic per word of the record: a wave
// per atomic (15 625 of them on one cache line at 10^6 points) took longer than reading the ids.
template <typename L>
__global__ __launch_bounds__(SC_THREADS) void r3d_scene_seg_ids_kernel(const L* __restrict__ seg, int M, int* __restrict__ rec) {
  __shared__ int red[SC_WAVES];
  __shared__ unsigned long long red_max[SC_WAVES];
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
    for (int w = 0; w < SC_WAVES; ++w) {
      mx = red[w] > mx ? red[w] : mx;
      bmax = red_max[w] > bmax ? red_max[w] : bmax;
    }
  n_neg = sc_block_count(n_neg, red);
  n_bad = sc_block_count(n_bad, red);
  if (threadIdx.x == 0) {  // integer maxima and counts: order-independent
    if (mx > 0) atomicMax(&rec[R3D_SEG_R_MAX1], mx);
    if (n_neg > 0) atomicAdd(&rec[R3D_SEG_R_NNEG], n_neg);
    if (n_bad > 0) {
      atomicAdd(&rec[R3D_SEG_R_NBAD], n_bad);
      atomicMax((unsigned long long*)(rec + R3D_SEG_R_BADMAX), bmax);
    }
  }
}

extern "C" int r3d_scene_seg_ids(const void* segments, int seg_bytes, long M, int32_t* ws, long ws_words, void* stream) {
  R3D_REQUIRE(segments && ws, "r3d_scene_seg_ids: null pointer (segments %p, ws %p)", segments, (void*)ws);
  SC_TRY(sg_check("r3d_scene_seg_ids", M, ws_words));
  R3D_REQUIRE(seg_bytes == 4 || seg_bytes == 8, "r3d_scene_seg_ids: segments of %d bytes (int32 or int64)", seg_bytes);
  const hipStream_t st = (hipStream_t)stream;
  const sg_layout L = sg_make_layout(M);
  const int gm = sc_count_grid(M);
  r3d_zero_words(ws + L.rec, R3D_SCENE_SEG_REC, st);
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
    const int p = sc_clamp(order[i], 0, M - 1);
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
  const int p = sc_clamp(order[i], 0, M - 1);
  segment_index[p] = i < n_in_seg ? s : -1;
  if (i >= n_in_seg) return;
  if (heads[i + 1] != heads[i]) {
    seg_start[s] = i;
    cstart[s] = c;
    seg_id[s] = skey[i];
  }
  if (contrib[i + 1] != c) clist[c] = p;
}

// tile heads: the contributors whose rank inside their segment is a multiple of R3D_SCENE_SEG_TILE
__global__ __launch_bounds__(SC_THREADS) void r3d_scene_seg_tile_flags_kernel(int M, int n_in_seg, const int* __restrict__ heads,
                                                                              const int* __restrict__ contrib,
                                                                              const int* __restrict__ cstart,
                                                                              int* __restrict__ tiles) {
  const int i = blockIdx.x * SC_THREADS + threadIdx.x;
  if (i > M) return;
  int f = 0;
  if (i < n_in_seg && contrib[i + 1] != contrib[i]) f = ((contrib[i] - cstart[heads[i + 1] - 1]) % R3D_SCENE_SEG_TILE) == 0;
  tiles[i] = f;
}

__global__ __launch_bounds__(SC_THREADS) void r3d_scene_seg_tile_table_kernel(int M, int n_in_seg, const int* __restrict__ heads,
                                                                              const int* __restrict__ contrib,
                                                                              const int* __restrict__ tiles,
                                                                              int* __restrict__ tile_seg, int* __restrict__ rec) {
  const int i = blockIdx.x * SC_THREADS + threadIdx.x;
  if (i > M) return;
  if (i == M) {
    rec[R3D_SEG_R_S] = heads[M];
    rec[R3D_SEG_R_NCONTRIB] = contrib[M];
    rec[R3D_SEG_R_NTILES] = tiles[M];
    return;
  }
  if (i < n_in_seg && tiles[i + 1] != tiles[i]) tile_seg[tiles[i]] = heads[i + 1] - 1;
}

extern "C" int r3d_scene_seg_group(const void* segments, int seg_bytes, long M, const int32_t* votes, long max_id, long n_negative,
                                   int32_t* segment_index, int32_t* ws, long ws_words, void* stream) {
  R3D_REQUIRE(segments && votes && segment_index && ws, "r3d_scene_seg_group: null pointer (segments %p, votes %p, segment_index %p, ws %p)",
              segments, (const void*)votes, (void*)segment_index, (void*)ws);
  SC_TRY(sg_check("r3d_scene_seg_group", M, ws_words));
  R3D_REQUIRE(seg_bytes == 4 || seg_bytes == 8, "r3d_scene_seg_group: segments of %d bytes (int32 or int64)", seg_bytes);
  R3D_REQUIRE(max_id >= -1 && max_id < SG_ID_LIMIT, "r3d_scene_seg_group: largest id %ld (-1: none .. 2^31 - 2)", max_id);
  R3D_REQUIRE(n_negative >= 0 && n_negative <= M, "r3d_scene_seg_group: %ld negative ids among %ld points", n_negative, M);
  const hipStream_t st = (hipStream_t)stream;
  const sg_layout L = sg_make_layout(M);
  const int none = (int)(max_id + 1);  // the key of a point without a segment: above every id
  const long key_max = n_negative > 0 ? max_id + 1 : (max_id < 0 ? 0 : max_id);
  const int gm = sc_grid_of(M), gm1 = sc_grid_of(M + 1);
  if (seg_bytes == 8)
    hipLaunchKernelGGL(r3d_scene_seg_keys_kernel<long long>, dim3(gm), dim3(SC_THREADS), 0, st, (const long long*)segments, (int)M,
                       none, ws + L.sort.key[0], ws + L.sort.idx[0]);
  else
    hipLaunchKernelGGL(r3d_scene_seg_keys_kernel<int>, dim3(gm), dim3(SC_THREADS), 0, st, (const int*)segments, (int)M, none,
                       ws + L.sort.key[0], ws + L.sort.idx[0]);
  const int sorted = sc_sort_pairs(ws, L.sort, M, sc_passes(key_max), st), spare = sorted ^ 1;
  int* skey = ws + L.sort.key[sorted];
  int* order = ws + L.sort.idx[sorted];
  int* heads = ws + L.sort.key[spare];
  int* contrib = ws + L.sort.idx[spare];
  const int n_in_seg = (int)(M - n_negative);
  hipLaunchKernelGGL(r3d_scene_seg_flags_kernel, dim3(gm1), dim3(SC_THREADS), 0, st, skey, order, (int)M, none, votes, heads,
                     contrib);
  sc_excl_scan(heads, M + 1, ws + L.sort.part, st);
  sc_excl_scan(contrib, M + 1, ws + L.sort.part, st);
  hipLaunchKernelGGL(r3d_scene_seg_tables_kernel, dim3(gm1), dim3(SC_THREADS), 0, st, skey, order, (int)M, n_in_seg, heads, contrib,
                     ws + L.seg_start, ws + L.cstart, ws + L.seg_id, ws + L.clist, segment_index);
  hipLaunchKernelGGL(r3d_scene_seg_tile_flags_kernel, dim3(gm1), dim3(SC_THREADS), 0, st, (int)M, n_in_seg, heads, contrib,
                     ws + L.cstart, ws + L.tiles);
  sc_excl_scan(ws + L.tiles, M + 1, ws + L.sort.part, st);
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
  __shared__ float stage[SC_WAVES][SG_BATCH * 64];
  __shared__ int row_p[SC_WAVES][R3D_SCENE_SEG_TILE];    // the tile's rows: scan index
  __shared__ float row_v[SC_WAVES][R3D_SCENE_SEG_TILE];  // and votes as a float
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int t = blockIdx.x * SC_WAVES + w;
  int first = 0, n = 0;
  if (t < n_tiles) {
    int s = tile_seg[t];
    s = s < 0 ? 0 : (s >= M ? M - 1 : s);
    first = cstart[s] + R3D_SCENE_SEG_TILE * (t - tiles[sc_clamp(seg_start[s], 0, M)]);
    n = cstart[s + 1] - first;
    n = n > R3D_SCENE_SEG_TILE ? R3D_SCENE_SEG_TILE : n;
    // the tables come from counts of these very points, so the rows lie inside clist; the guard only matters for a
    // workspace that r3d_scene_seg_group did not fill
    if (first < 0 || n < 0 || (long)first + n > M) first = n = 0;
  }
  // the tile's scan indices and votes first, four independent loads a lane: the element loads below then depend on LDS
  // only and go out eight at a time (one load per element, each waiting for its index, took ten times as long)
  int pr[R3D_SCENE_SEG_TILE / R3D_WAVE];
#pragma unroll
  for (int k = 0; k < R3D_SCENE_SEG_TILE / R3D_WAVE; ++k) {
    const int r = k * R3D_WAVE + lane;
    pr[k] = sc_clamp(clist[first + (r < n ? r : 0)], 0, M - 1);
  }
#pragma unroll
  for (int k = 0; k < R3D_SCENE_SEG_TILE / R3D_WAVE; ++k) {
    row_p[w][k * R3D_WAVE + lane] = pr[k];
    row_v[w][k * R3D_WAVE + lane] = (float)votes[pr[k]];
  }
  __syncthreads();
  float acc = 0.0f;
  for (int r0 = 0; r0 < R3D_SCENE_SEG_TILE; r0 += SG_BATCH) {
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
  const int s = blockIdx.x * SC_WAVES + (threadIdx.x >> 6);
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
  SC_TRY(sg_check("r3d_scene_seg_pool", M, ws_words));
  R3D_REQUIRE(n_cols >= 1 && n_cols <= R3D_SCENE_SCORE_COLS_MAX, "r3d_scene_seg_pool: %d score columns (1 .. 64)", n_cols);
  R3D_REQUIRE(n_segments >= 0 && n_segments <= M && n_tiles >= 0 && n_tiles <= M,
              "r3d_scene_seg_pool: %ld segments, %ld tiles of %ld points", n_segments, n_tiles, M);
  R3D_REQUIRE(n_segments == 0 || (seg_ids && seg_points && seg_members && seg_scores),
              "r3d_scene_seg_pool: null pointer (seg_ids %p, seg_points %p, seg_members %p, seg_scores %p)", (void*)seg_ids,
              (void*)seg_points, (void*)seg_members, (void*)seg_scores);
  R3D_REQUIRE(n_tiles == 0 || part, "r3d_scene_seg_pool: null pointer (part)");
  const hipStream_t st = (hipStream_t)stream;
  const sg_layout L = sg_make_layout(M);
  if (n_tiles > 0)
    hipLaunchKernelGGL(r3d_scene_seg_pool_tiles_kernel, dim3((int)((n_tiles + SC_WAVES - 1) / SC_WAVES)), dim3(SC_THREADS), 0, st,
                       (int)n_tiles, n_cols, (int)M, scores, votes, ws + L.clist, ws + L.cstart, ws + L.seg_start, ws + L.tiles,
                       ws + L.tile_seg, part);
  if (n_segments > 0)
    hipLaunchKernelGGL(r3d_scene_seg_pool_final_kernel, dim3((int)((n_segments + SC_WAVES - 1) / SC_WAVES)), dim3(SC_THREADS), 0,
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
// SC_COUNT_BLOCKS workgroups, one integer atomic per count and workgroup.
__global__ __launch_bounds__(SC_THREADS) void r3d_scene_seg_spread_kernel(
    int M, int C, int K, int S, int min_members, const int* __restrict__ segment_index, const int* __restrict__ members,
    sg_point_fields seg, sg_point_fields in, float* __restrict__ scores, long long* __restrict__ labels,
    unsigned char* __restrict__ pooled, long long* __restrict__ set_labels, int* __restrict__ set_of, float* __restrict__ margin,
    int* __restrict__ rec) {
  __shared__ int src[SC_THREADS];  // the segment row a point's scores come from, -1: its own row of res
  __shared__ int red[SC_WAVES];
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
  n_pl = sc_block_count(n_pl, red);
  n_fi = sc_block_count(n_fi, red);
  n_un = sc_block_count(n_un, red);
  if (threadIdx.x == 0) {  // integer counts: order-independent
    if (n_pl > 0) atomicAdd(&rec[R3D_SEG_R_NPOOLED], n_pl);
    if (n_fi > 0) atomicAdd(&rec[R3D_SEG_R_NFILLED], n_fi);
    if (n_un > 0) atomicAdd(&rec[R3D_SEG_R_NUNLAB], n_un);
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
  SC_TRY(sg_check("r3d_scene_seg_spread", M, ws_words));
  R3D_REQUIRE(n_cols >= 1 && n_cols <= R3D_SCENE_SCORE_COLS_MAX, "r3d_scene_seg_spread: %d score columns (1 .. 64)", n_cols);
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
  const sg_layout L = sg_make_layout(M);
  const sg_point_fields seg = {seg_scores, (const long long*)seg_labels, (const long long*)seg_set_labels, seg_set_of, seg_margin};
  const sg_point_fields in = {in_scores, (const long long*)in_labels, (const long long*)in_set_labels, in_set_of, in_margin};
  hipLaunchKernelGGL(r3d_scene_seg_spread_kernel, dim3(sc_count_grid(M)), dim3(SC_THREADS), 0,
                     (hipStream_t)stream, (int)M, n_cols, n_sets, (int)n_segments, min_members, segment_index, seg_members, seg, in,
                     scores, (long long*)labels, pooled, (long long*)set_labels, set_of, margin, ws + L.rec);
  R3D_LAUNCH_CHECK("r3d_scene_seg_spread");
  return R3D_OK;
}
