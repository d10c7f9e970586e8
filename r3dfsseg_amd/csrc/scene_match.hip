// A scan's objects against ground-truth instances: the device side of scene_match.py.
// match_objects ("Matching objects against ground truth", M1-M8): two columns of object ids over the same
// points -> per column its rows (distinct ids, ascending), the pairs of rows that share a point with their intersection and
// IoU, every row's best partner, and the pairs that are each other's best.
//   ids     per column the largest legal id and the negatives, the points M1 takes out, ids >= 2^31 - 1   -> the record (read 1)
//   rows    per column: keys (a point without a row: the one key above every id), the stable radix sort of scene_sort.hip
//           on (id, scan index), run heads, their scan, the row tables, the row of every point, mixed rows    -> P, T (read 2)
//   pairs   the row tables as the caller keeps them; two stable sorts of 32-bit keys, by truth row, then by the pred row
//           gathered through the first order; heads where (p, t) changes, their scan, the pair tables        -> n_pairs (read 3)
//   best    IoU and the eligible flag per pair; truth_best by a 64-bit integer atomicMax per pair, pred_best by a segmented
//           maximum over the contiguous pairs of a pred row; the mutual best against the thresholds
// The IoU is two int -> fp32 conversions and one __fdiv_rn; every count and every maximum is an integer scan or an integer
// atomic, whose result does not depend on the order: no float goes through an atomic.
#include "scene_common.h"

#define MT_ID_LIMIT 2147483647LL
static_assert(R3D_MATCH_R_NPAIRS < R3D_SCENE_MATCH_REC, "a word beyond the record");

struct mt_layout {
  long rec;            // R3D_SCENE_MATCH_REC words, R3D_MATCH_R_* (r3d.h; `+ column`: 0 pred, 1 truth)
  sc_sort_ws sort;     // pairs of M + 1 words; the pair a sort leaves free holds the head scan and the mixed flags
  long row_start[2];   // R + 1: first sorted position of a row
  long row_id[2];      // R
  long row_head[2];    // R: scan index of the row's first point (the lowest: the sort is stable)
  long pair_start;     // n_pairs + 1: first sorted position of a pair
  long pair_p, pair_t; // n_pairs
  long total;
};

static mt_layout mt_make_layout(long M) {
  mt_layout L;
  const long Ma = sc_align(M + 1);
  long o = 0;
  L.rec = o; o += R3D_SCENE_MATCH_REC;
  o = sc_sort_ws_append(L.sort, o, M, Ma, sc_sort_part_words(M, M + 1));
  for (int c = 0; c < 2; ++c) {
    L.row_start[c] = o; o += Ma;
    L.row_id[c] = o; o += Ma;
    L.row_head[c] = o; o += Ma;
  }
  L.pair_start = o; o += Ma;
  L.pair_p = o; o += Ma;
  L.pair_t = o; o += Ma;
  L.total = o;
  return L;
}

extern "C" long r3d_scene_match_ws_words(long M) { return M > 0 && M <= R3D_SCENE_MAX_POINTS ? mt_make_layout(M).total : -1; }

// what every entry point has: the scan's size and the workspace
static int mt_check(const char* name, long M, long ws_words) {
  SC_TRY(sc_check_points(name, M));
  return sc_check_ws(name, ws_words, r3d_scene_match_ws_words(M));
}

static int mt_check_bytes(const char* name, const char* what, int bytes) {
  R3D_REQUIRE(bytes == 4 || bytes == 8, "%s: %s of %d bytes (int32 or int64)", name, what, bytes);
  return R3D_OK;
}

// element i of an int32 or int64 column (bytes is uniform over the launch)
static __device__ __forceinline__ long long mt_load(const void* p, int bytes, long i) {
  return bytes == 8 ? ((const long long*)p)[i] : (long long)((const int*)p)[i];
}

// What an arg-max compares: the bits of a positive fp32 order as the float does; below them the tie-break, so that the
// LOWER `tie` is the greater value.  0 is below every rank of a positive IoU.
static __device__ __forceinline__ unsigned long long mt_rank(float iou, unsigned tie) {
  return ((unsigned long long)__float_as_uint(iou) << 32) | (unsigned long long)(0xFFFFFFFFu - tie);
}

// the workgroup's maximum of a per-thread value, valid in thread 0 (red: SC_WAVES words)
static __device__ __forceinline__ unsigned long long mt_block_max(unsigned long long v, unsigned long long* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long v2 = sc_shfl_xor_u64(v, o);
    v = v2 > v ? v2 : v;
  }
  __syncthreads();  // red may still be read from the maximum before
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  unsigned long long t = 0ull;
#pragma unroll
  for (int w = 0; w < SC_WAVES; ++w) t = red[w] > t ? red[w] : t;
  return t;
}

// ------------------------------------------------------------------------------------------------ ids
// At most SC_COUNT_BLOCKS workgroups stride over both columns; one integer atomic per word of the record and workgroup.
__global__ __launch_bounds__(SC_THREADS) void r3d_scene_match_ids_kernel(const void* __restrict__ pred, int pred_bytes,
                                                                         const void* __restrict__ truth, int truth_bytes, int M,
                                                                         int ignore, int* __restrict__ rec) {
  __shared__ int red[SC_WAVES];
  __shared__ unsigned long long red_max[SC_WAVES];
  int n_neg[2] = {0, 0}, n_ign = 0, n_bad = 0;
  unsigned long long mx[2] = {0ull, 0ull}, bmax = 0ull;
  for (long i = (long)blockIdx.x * SC_THREADS + threadIdx.x; i < M; i += (long)gridDim.x * SC_THREADS) {
    const long long g[2] = {mt_load(pred, pred_bytes, i), mt_load(truth, truth_bytes, i)};
#pragma unroll
    for (int c = 0; c < 2; ++c)
      if (g[c] >= MT_ID_LIMIT) {
        ++n_bad;
        bmax = (unsigned long long)g[c] > bmax ? (unsigned long long)g[c] : bmax;
      }
    if (ignore && g[1] < 0) {  // M1
      ++n_ign;
      continue;
    }
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      if (g[c] < 0)
        ++n_neg[c];
      else if (g[c] < MT_ID_LIMIT)
        mx[c] = (unsigned long long)(g[c] + 1) > mx[c] ? (unsigned long long)(g[c] + 1) : mx[c];
    }
  }
  const unsigned long long m0 = mt_block_max(mx[0], red_max), m1 = mt_block_max(mx[1], red_max);
  bmax = mt_block_max(bmax, red_max);
  const int nn0 = sc_block_count(n_neg[0], red), nn1 = sc_block_count(n_neg[1], red);
  n_ign = sc_block_count(n_ign, red);
  n_bad = sc_block_count(n_bad, red);
  if (threadIdx.x == 0) {  // integer maxima and counts: order-independent
    if (m0 > 0) atomicMax(&rec[R3D_MATCH_R_MAX1], (int)m0);
    if (m1 > 0) atomicMax(&rec[R3D_MATCH_R_MAX1 + 1], (int)m1);
    if (nn0 > 0) atomicAdd(&rec[R3D_MATCH_R_NNEG], nn0);
    if (nn1 > 0) atomicAdd(&rec[R3D_MATCH_R_NNEG + 1], nn1);
    if (n_ign > 0) atomicAdd(&rec[R3D_MATCH_R_NIGNORED], n_ign);
    if (n_bad > 0) {
      atomicAdd(&rec[R3D_MATCH_R_NBAD], n_bad);
      atomicMax((unsigned long long*)(rec + R3D_MATCH_R_BADMAX), bmax);
    }
  }
}

extern "C" int r3d_scene_match_ids(const void* pred, int pred_bytes, const void* truth, int truth_bytes, long M,
                                   int ignore_unannotated, int32_t* ws, long ws_words, void* stream) {
  R3D_REQUIRE(pred && truth && ws, "r3d_scene_match_ids: null pointer (pred %p, truth %p, ws %p)", pred, truth, (void*)ws);
  SC_TRY(mt_check("r3d_scene_match_ids", M, ws_words));
  SC_TRY(mt_check_bytes("r3d_scene_match_ids", "pred", pred_bytes));
  SC_TRY(mt_check_bytes("r3d_scene_match_ids", "truth", truth_bytes));
  const hipStream_t st = (hipStream_t)stream;
  const mt_layout L = mt_make_layout(M);
  r3d_zero_words(ws + L.rec, R3D_SCENE_MATCH_REC, st);
  hipLaunchKernelGGL(r3d_scene_match_ids_kernel, dim3(sc_count_grid(M)), dim3(SC_THREADS), 0, st, pred, pred_bytes, truth,
                     truth_bytes, (int)M, ignore_unannotated ? 1 : 0, ws + L.rec);
  R3D_LAUNCH_CHECK("r3d_scene_match_ids");
  return R3D_OK;
}

// ------------------------------------------------------------------------------------------------ rows
// gate: the truth column when M1 is on (a point whose gate id is negative has no row), else null
__global__ __launch_bounds__(SC_THREADS) void r3d_scene_match_row_keys_kernel(const void* __restrict__ ids, int bytes,
                                                                              const void* __restrict__ gate, int gate_bytes, int M,
                                                                              int none, int* __restrict__ key, int* __restrict__ idx) {
  const int i = blockIdx.x * SC_THREADS + threadIdx.x;
  if (i >= M) return;
  const long long g = mt_load(ids, bytes, i);
  const bool out = g < 0 || g >= (long long)none || (gate && mt_load(gate, gate_bytes, i) < 0);  // (no legal id reaches `none`)
  key[i] = out ? none : (int)g;
  idx[i] = i;
}

// sorted position i: heads[i] = it opens a row; word M is 0, so that the exclusive scan leaves the total there.  The
// mixed flags of the rows start at 0.
__global__ __launch_bounds__(SC_THREADS) void r3d_scene_match_row_flags_kernel(const int* __restrict__ skey, int M, int none,
                                                                               int* __restrict__ heads, int* __restrict__ mixed) {
  const int i = blockIdx.x * SC_THREADS + threadIdx.x;
  if (i > M) return;
  int h = 0;
  if (i < M) {
    const int k = skey[i];
    h = k >= 0 && k < none && (i == 0 || skey[i - 1] != k);
  }
  heads[i] = h;
  mixed[i] = 0;
}

// after the scan: heads[i] = rows opened in front of i.  A row's entries are written by the thread of its first sorted
// position, entry R of row_start and the record's word by the thread of position M.
__global__ __launch_bounds__(SC_THREADS) void r3d_scene_match_row_tables_kernel(
    const int* __restrict__ skey, const int* __restrict__ order, int M, int n_in, const int* __restrict__ heads,
    int* __restrict__ row_start, int* __restrict__ row_id, int* __restrict__ row_head, int* __restrict__ index, int* __restrict__ rec_rows) {
  const int i = blockIdx.x * SC_THREADS + threadIdx.x;
  if (i > M) return;
  if (i == M) {
    const int R = sc_clamp(heads[M], 0, M);
    row_start[R] = n_in;
    *rec_rows = R;
    return;
  }
  const int s = heads[i + 1] - 1;
  const int p = sc_clamp(order[i], 0, M - 1);
  index[p] = i < n_in ? s : -1;
  if (i >= n_in) return;
  if (heads[i + 1] != heads[i]) {
    row_start[s] = i;
    row_id[s] = skey[i];
    row_head[s] = p;
  }
}

// M3: a point whose label differs from the label of its row's first point marks the row (every writer stores the same 1)
__global__ __launch_bounds__(SC_THREADS) void r3d_scene_match_row_mixed_kernel(const int* __restrict__ order, int M, int n_in,
                                                                               const int* __restrict__ heads,
                                                                               const int* __restrict__ row_head,
                                                                               const void* __restrict__ labels, int label_bytes,
                                                                               int* __restrict__ mixed) {
  const int i = blockIdx.x * SC_THREADS + threadIdx.x;
  if (i >= n_in || i >= M) return;
  const int s = heads[i + 1] - 1;
  if (s < 0 || s >= M) return;
  const int p = sc_clamp(order[i], 0, M - 1), hp = sc_clamp(row_head[s], 0, M - 1);
  if (mt_load(labels, label_bytes, p) != mt_load(labels, label_bytes, hp)) mixed[s] = 1;
}

__global__ __launch_bounds__(SC_THREADS) void r3d_scene_match_row_mixed_count_kernel(const int* __restrict__ heads, int M,
                                                                                     const int* __restrict__ mixed,
                                                                                     int* __restrict__ rec_mixed) {
  __shared__ int red[SC_WAVES];
  const int R = sc_clamp(heads[M], 0, M);
  int n = 0;
  for (long i = (long)blockIdx.x * SC_THREADS + threadIdx.x; i < R; i += (long)gridDim.x * SC_THREADS) n += mixed[i] != 0;
  n = sc_block_count(n, red);
  if (threadIdx.x == 0 && n > 0) atomicAdd(rec_mixed, n);  // an integer count: order-independent
}

static void mt_rows_of(int c, const void* ids, int bytes, const void* gate, int gate_bytes, const void* labels, int label_bytes,
                       long M, long max_id, long n_in, int32_t* index, int32_t* ws, const mt_layout& L, hipStream_t st) {
  const int none = (int)(max_id + 1);  // the key of a point without a row: above every id
  const long key_max = n_in < M ? max_id + 1 : max_id;
  const int gm = sc_grid_of(M), gm1 = sc_grid_of(M + 1);
  hipLaunchKernelGGL(r3d_scene_match_row_keys_kernel, dim3(gm), dim3(SC_THREADS), 0, st, ids, bytes, gate, gate_bytes, (int)M, none,
                     ws + L.sort.key[0], ws + L.sort.idx[0]);
  const int sorted = sc_sort_pairs(ws, L.sort, M, sc_passes(key_max), st), spare = sorted ^ 1;
  const int* skey = ws + L.sort.key[sorted];
  const int* order = ws + L.sort.idx[sorted];
  int* heads = ws + L.sort.key[spare];
  int* mixed = ws + L.sort.idx[spare];
  hipLaunchKernelGGL(r3d_scene_match_row_flags_kernel, dim3(gm1), dim3(SC_THREADS), 0, st, skey, (int)M, none, heads, mixed);
  sc_excl_scan(heads, M + 1, ws + L.sort.part, st);
  hipLaunchKernelGGL(r3d_scene_match_row_tables_kernel, dim3(gm1), dim3(SC_THREADS), 0, st, skey, order, (int)M, (int)n_in, heads,
                     ws + L.row_start[c], ws + L.row_id[c], ws + L.row_head[c], index, ws + L.rec + R3D_MATCH_R_ROWS + c);
  if (labels) {
    hipLaunchKernelGGL(r3d_scene_match_row_mixed_kernel, dim3(gm), dim3(SC_THREADS), 0, st, order, (int)M, (int)n_in, heads,
                       ws + L.row_head[c], labels, label_bytes, mixed);
    hipLaunchKernelGGL(r3d_scene_match_row_mixed_count_kernel, dim3(sc_count_grid(M)), dim3(SC_THREADS), 0, st, heads, (int)M, mixed,
                       ws + L.rec + R3D_MATCH_R_MIXED + c);
  }
}

extern "C" int r3d_scene_match_rows(const void* pred, int pred_bytes, const void* truth, int truth_bytes, const void* pred_labels,
                                    int pred_label_bytes, const void* truth_labels, int truth_label_bytes, long M,
                                    int ignore_unannotated, long max_pred, long max_truth, long n_pred_in, long n_truth_in,
                                    int32_t* pred_index, int32_t* truth_index, int32_t* ws, long ws_words, void* stream) {
  R3D_REQUIRE(pred && truth && pred_index && truth_index && ws,
              "r3d_scene_match_rows: null pointer (pred %p, truth %p, pred_index %p, truth_index %p, ws %p)", pred, truth,
              (void*)pred_index, (void*)truth_index, (void*)ws);
  SC_TRY(mt_check("r3d_scene_match_rows", M, ws_words));
  SC_TRY(mt_check_bytes("r3d_scene_match_rows", "pred", pred_bytes));
  SC_TRY(mt_check_bytes("r3d_scene_match_rows", "truth", truth_bytes));
  R3D_REQUIRE((pred_labels != nullptr) == (truth_labels != nullptr), "r3d_scene_match_rows: labels for one column only (pred_labels %p, "
              "truth_labels %p)", pred_labels, truth_labels);
  if (pred_labels) {
    SC_TRY(mt_check_bytes("r3d_scene_match_rows", "pred_labels", pred_label_bytes));
    SC_TRY(mt_check_bytes("r3d_scene_match_rows", "truth_labels", truth_label_bytes));
  }
  R3D_REQUIRE(max_pred >= 0 && max_pred < MT_ID_LIMIT && max_truth >= 0 && max_truth < MT_ID_LIMIT,
              "r3d_scene_match_rows: largest ids %ld and %ld (0 .. 2^31 - 2)", max_pred, max_truth);
  R3D_REQUIRE(n_pred_in >= 1 && n_pred_in <= M && n_truth_in >= 1 && n_truth_in <= M,
              "r3d_scene_match_rows: %ld and %ld points with a row among %ld", n_pred_in, n_truth_in, M);
  const hipStream_t st = (hipStream_t)stream;
  const mt_layout L = mt_make_layout(M);
  const void* gate = ignore_unannotated ? truth : nullptr;
  mt_rows_of(0, pred, pred_bytes, gate, truth_bytes, pred_labels, pred_label_bytes, M, max_pred, n_pred_in, pred_index, ws, L, st);
  mt_rows_of(1, truth, truth_bytes, nullptr, 0, truth_labels, truth_label_bytes, M, max_truth, n_truth_in, truth_index, ws, L, st);
  R3D_LAUNCH_CHECK("r3d_scene_match_rows");
  return R3D_OK;
}

// ------------------------------------------------------------------------------------------------ pairs
// the row tables as the caller keeps them (M2, M3)
__global__ __launch_bounds__(SC_THREADS) void r3d_scene_match_emit_rows_kernel(int R, int M, const int* __restrict__ row_start,
                                                                               const int* __restrict__ row_id,
                                                                               const int* __restrict__ row_head,
                                                                               const void* __restrict__ labels, int label_bytes,
                                                                               long long* __restrict__ ids, int* __restrict__ points,
                                                                               long long* __restrict__ classes) {
  const int r = blockIdx.x * SC_THREADS + threadIdx.x;
  if (r >= R) return;
  ids[r] = (long long)row_id[r];
  points[r] = row_start[r + 1] - row_start[r];
  if (labels) classes[r] = mt_load(labels, label_bytes, sc_clamp(row_head[r], 0, M - 1));
}

// first sort: by truth row; a point without both rows gets the key T and sorts last
__global__ __launch_bounds__(SC_THREADS) void r3d_scene_match_pair_keys_kernel(const int* __restrict__ pred_index,
                                                                               const int* __restrict__ truth_index, int M, int P, int T,
                                                                               int* __restrict__ key, int* __restrict__ idx) {
  const int i = blockIdx.x * SC_THREADS + threadIdx.x;
  if (i >= M) return;
  const int p = pred_index[i], t = truth_index[i];
  key[i] = (p >= 0 && p < P && t >= 0 && t < T) ? t : T;
  idx[i] = i;
}

// second sort: by the pred row gathered through the first sort's order (key P without both rows); in and out may be the
// same arrays: a thread reads and writes its own position only
__global__ __launch_bounds__(SC_THREADS) void r3d_scene_match_pair_gather_kernel(const int* key_in, const int* idx_in, int M, int P,
                                                                                 int T, const int* __restrict__ pred_index,
                                                                                 int* key_out, int* idx_out) {
  const int j = blockIdx.x * SC_THREADS + threadIdx.x;
  if (j >= M) return;
  const int q = sc_clamp(idx_in[j], 0, M - 1), t = key_in[j];
  key_out[j] = (t >= 0 && t < T) ? sc_clamp(pred_index[q], 0, P - 1) : P;
  idx_out[j] = q;
}

// sorted position i: heads[i] = (p, t) changes here; the positions with both rows are a prefix, its length goes to the record
__global__ __launch_bounds__(SC_THREADS) void r3d_scene_match_pair_flags_kernel(const int* __restrict__ skey,
                                                                                const int* __restrict__ order, int M, int P,
                                                                                const int* __restrict__ truth_index,
                                                                                int* __restrict__ heads, int* __restrict__ rec) {
  const int i = blockIdx.x * SC_THREADS + threadIdx.x;
  if (i > M) return;
  if (i == M) {
    heads[M] = 0;
    if (skey[0] < 0 || skey[0] >= P) rec[R3D_MATCH_R_NBOTH] = 0;
    return;
  }
  const int k = skey[i];
  int h = 0;
  if (k >= 0 && k < P) {
    const int t = truth_index[sc_clamp(order[i], 0, M - 1)];
    h = i == 0 || skey[i - 1] != k || truth_index[sc_clamp(order[i - 1], 0, M - 1)] != t;
    if (i == M - 1 || skey[i + 1] < 0 || skey[i + 1] >= P) rec[R3D_MATCH_R_NBOTH] = i + 1;  // one writer: the prefix's last position
  }
  heads[i] = h;
}

__global__ __launch_bounds__(SC_THREADS) void r3d_scene_match_pair_tables_kernel(const int* __restrict__ skey,
                                                                                 const int* __restrict__ order, int M,
                                                                                 const int* __restrict__ truth_index,
                                                                                 const int* __restrict__ heads,
                                                                                 int* __restrict__ pair_start, int* __restrict__ pair_p,
                                                                                 int* __restrict__ pair_t, int* __restrict__ rec) {
  const int i = blockIdx.x * SC_THREADS + threadIdx.x;
  if (i > M) return;
  if (i == M) {
    const int K = sc_clamp(heads[M], 0, M);
    pair_start[K] = rec[R3D_MATCH_R_NBOTH];  // (written by the launch before)
    rec[R3D_MATCH_R_NPAIRS] = K;
    return;
  }
  if (heads[i + 1] != heads[i]) {
    const int k = heads[i];
    pair_start[k] = i;
    pair_p[k] = skey[i];
    pair_t[k] = truth_index[sc_clamp(order[i], 0, M - 1)];
  }
}

extern "C" int r3d_scene_match_pairs(long M, long n_pred, long n_truth, const int32_t* pred_index, const int32_t* truth_index,
                                     const void* pred_labels, int pred_label_bytes, const void* truth_labels, int truth_label_bytes,
                                     int64_t* pred_ids, int32_t* pred_points, int64_t* pred_classes, int64_t* truth_ids,
                                     int32_t* truth_points, int64_t* truth_classes, int32_t* ws, long ws_words, void* stream) {
  R3D_REQUIRE(pred_index && truth_index && pred_ids && pred_points && truth_ids && truth_points && ws,
              "r3d_scene_match_pairs: null pointer (pred_index %p, truth_index %p, pred_ids %p, pred_points %p, truth_ids %p, "
              "truth_points %p, ws %p)", (const void*)pred_index, (const void*)truth_index, (void*)pred_ids, (void*)pred_points,
              (void*)truth_ids, (void*)truth_points, (void*)ws);
  SC_TRY(mt_check("r3d_scene_match_pairs", M, ws_words));
  R3D_REQUIRE(n_pred >= 1 && n_pred <= M && n_truth >= 1 && n_truth <= M, "r3d_scene_match_pairs: %ld and %ld rows of %ld points",
              n_pred, n_truth, M);
  R3D_REQUIRE((pred_labels != nullptr) == (truth_labels != nullptr) && (!pred_labels || (pred_classes && truth_classes)),
              "r3d_scene_match_pairs: labels and class tables come for both columns or for none (pred_labels %p, truth_labels %p, "
              "pred_classes %p, truth_classes %p)", pred_labels, truth_labels, (void*)pred_classes, (void*)truth_classes);
  if (pred_labels) {
    SC_TRY(mt_check_bytes("r3d_scene_match_pairs", "pred_labels", pred_label_bytes));
    SC_TRY(mt_check_bytes("r3d_scene_match_pairs", "truth_labels", truth_label_bytes));
  }
  const hipStream_t st = (hipStream_t)stream;
  const mt_layout L = mt_make_layout(M);
  const int P = (int)n_pred, T = (int)n_truth;
  const int gm = sc_grid_of(M), gm1 = sc_grid_of(M + 1);
  hipLaunchKernelGGL(r3d_scene_match_emit_rows_kernel, dim3(sc_grid_of(P)), dim3(SC_THREADS), 0, st, P, (int)M, ws + L.row_start[0],
                     ws + L.row_id[0], ws + L.row_head[0], pred_labels, pred_label_bytes, (long long*)pred_ids, pred_points,
                     (long long*)pred_classes);
  hipLaunchKernelGGL(r3d_scene_match_emit_rows_kernel, dim3(sc_grid_of(T)), dim3(SC_THREADS), 0, st, T, (int)M, ws + L.row_start[1],
                     ws + L.row_id[1], ws + L.row_head[1], truth_labels, truth_label_bytes, (long long*)truth_ids, truth_points,
                     (long long*)truth_classes);
  hipLaunchKernelGGL(r3d_scene_match_pair_keys_kernel, dim3(gm), dim3(SC_THREADS), 0, st, pred_index, truth_index, (int)M, P, T,
                     ws + L.sort.key[0], ws + L.sort.idx[0]);
  const int first = sc_sort_pairs(ws, L.sort, M, sc_passes(T), st);
  hipLaunchKernelGGL(r3d_scene_match_pair_gather_kernel, dim3(gm), dim3(SC_THREADS), 0, st, ws + L.sort.key[first],
                     ws + L.sort.idx[first], (int)M, P, T, pred_index, ws + L.sort.key[0], ws + L.sort.idx[0]);
  const int sorted = sc_sort_pairs(ws, L.sort, M, sc_passes(P), st), spare = sorted ^ 1;
  const int* skey = ws + L.sort.key[sorted];
  const int* order = ws + L.sort.idx[sorted];
  int* heads = ws + L.sort.key[spare];
  hipLaunchKernelGGL(r3d_scene_match_pair_flags_kernel, dim3(gm1), dim3(SC_THREADS), 0, st, skey, order, (int)M, P, truth_index, heads,
                     ws + L.rec);
  sc_excl_scan(heads, M + 1, ws + L.sort.part, st);
  hipLaunchKernelGGL(r3d_scene_match_pair_tables_kernel, dim3(gm1), dim3(SC_THREADS), 0, st, skey, order, (int)M, truth_index, heads,
                     ws + L.pair_start, ws + L.pair_p, ws + L.pair_t, ws + L.rec);
  R3D_LAUNCH_CHECK("r3d_scene_match_pairs");
  return R3D_OK;
}

// ------------------------------------------------------------------------------------------------ best
__global__ __launch_bounds__(SC_THREADS) void r3d_scene_match_best_fill_kernel(int P, int T, int* __restrict__ pred_best,
                                                                               int* __restrict__ truth_best,
                                                                               unsigned long long* __restrict__ pbest,
                                                                               unsigned long long* __restrict__ tbest) {
  const int i = blockIdx.x * SC_THREADS + threadIdx.x;
  if (i < P) {
    pred_best[i] = -1;
    pbest[i] = 0ull;
  }
  if (i < T) {
    truth_best[i] = -1;
    tbest[i] = 0ull;
  }
}

// M4, M5 and the first half of truth_best: one thread per pair.  eligible[] is the caller's pair_match, which the last
// launch overwrites.
__global__ __launch_bounds__(SC_THREADS) void r3d_scene_match_pair_iou_kernel(
    int K, int P, int T, const int* __restrict__ pair_start, const int* __restrict__ pair_p, const int* __restrict__ pair_t,
    const int* __restrict__ pred_points, const int* __restrict__ truth_points, const long long* __restrict__ pred_classes,
    const long long* __restrict__ truth_classes, int* __restrict__ pair_pred, int* __restrict__ pair_truth, int* __restrict__ pair_points,
    float* __restrict__ pair_iou, unsigned char* __restrict__ eligible, unsigned long long* __restrict__ tbest) {
  const int k = blockIdx.x * SC_THREADS + threadIdx.x;
  if (k >= K) return;
  // the tables come from counts of these very points, so the rows lie inside theirs; the clamps only matter for a
  // workspace that r3d_scene_match_pairs did not fill
  const int p = sc_clamp(pair_p[k], 0, P - 1), t = sc_clamp(pair_t[k], 0, T - 1);
  const int inter = pair_start[k + 1] - pair_start[k];
  const int uni = pred_points[p] + truth_points[t] - inter;
  const float iou = (inter > 0 && uni > 0) ? __fdiv_rn((float)inter, (float)uni) : 0.0f;
  const bool el = iou > 0.0f && (!pred_classes || pred_classes[p] == truth_classes[t]);
  pair_pred[k] = p;
  pair_truth[k] = t;
  pair_points[k] = inter;
  pair_iou[k] = iou;
  eligible[k] = el ? 1 : 0;
  if (el) atomicMax(&tbest[t], mt_rank(iou, (unsigned)p));  // an integer maximum: order-independent
}

// pred_best: the pairs of a pred row are contiguous.  A workgroup takes SC_THREADS pairs, runs a segmented maximum scan
// over them in LDS (log2 SC_THREADS steps: position i takes the value d positions in front when that one has its row),
// and the last position of every run inside the workgroup holds the run's maximum there.  It joins the row's word by one
// integer atomicMax per run and workgroup, so a run of any length -- longer than a wave, than a workgroup -- ends with
// its maximum whatever the order of the workgroups.
__global__ __launch_bounds__(SC_THREADS) void r3d_scene_match_pred_best_kernel(int K, int P, const int* __restrict__ pair_pred,
                                                                               const float* __restrict__ pair_iou,
                                                                               const unsigned char* __restrict__ eligible,
                                                                               unsigned long long* __restrict__ pbest) {
  __shared__ unsigned long long v_s[SC_THREADS];
  __shared__ int p_s[SC_THREADS];
  const int tid = threadIdx.x;
  const int k = blockIdx.x * SC_THREADS + tid;
  const int p = k < K ? pair_pred[k] : -2;
  unsigned long long v = (k < K && eligible[k]) ? mt_rank(pair_iou[k], (unsigned)k) : 0ull;
  p_s[tid] = p;
  v_s[tid] = v;
  __syncthreads();
#pragma unroll
  for (int d = 1; d < SC_THREADS; d <<= 1) {
    const unsigned long long o = (tid >= d && p_s[tid - d] == p) ? v_s[tid - d] : 0ull;
    __syncthreads();
    v = o > v ? o : v;
    v_s[tid] = v;
    __syncthreads();
  }
  const bool tail = tid == SC_THREADS - 1 || p_s[tid + 1] != p;
  if (tail && v != 0ull && p >= 0 && p < P) atomicMax(&pbest[p], v);
}

// the winners as pair rows: pred_best from its word; truth_best from the one eligible pair of t whose rank is the word's
__global__ __launch_bounds__(SC_THREADS) void r3d_scene_match_best_rows_kernel(int K, int P, int T, const int* __restrict__ pair_pred,
                                                                               const int* __restrict__ pair_truth,
                                                                               const float* __restrict__ pair_iou,
                                                                               const unsigned char* __restrict__ eligible,
                                                                               const unsigned long long* __restrict__ pbest,
                                                                               const unsigned long long* __restrict__ tbest,
                                                                               int* __restrict__ pred_best, int* __restrict__ truth_best) {
  const int i = blockIdx.x * SC_THREADS + threadIdx.x;
  if (i < P) {
    const unsigned long long v = pbest[i];
    if (v != 0ull) pred_best[i] = sc_clamp((int)(0xFFFFFFFFu - (unsigned)(v & 0xFFFFFFFFull)), 0, K - 1);
  }
  if (i < K && eligible[i]) {
    const int t = sc_clamp(pair_truth[i], 0, T - 1);
    if (tbest[t] == mt_rank(pair_iou[i], (unsigned)pair_pred[i])) truth_best[t] = i;  // (p, t) is unique: one writer
  }
}

struct mt_thresholds {
  float v[R3D_SCENE_MATCH_IOU];
};

// M7, written last: over eligible[]
__global__ __launch_bounds__(SC_THREADS) void r3d_scene_match_pair_match_kernel(int K, int P, int T, const int* __restrict__ pair_pred,
                                                                                const int* __restrict__ pair_truth,
                                                                                const float* __restrict__ pair_iou,
                                                                                const int* __restrict__ pred_best,
                                                                                const int* __restrict__ truth_best, int n_iou,
                                                                                mt_thresholds th, unsigned char* __restrict__ pair_match) {
  const int k = blockIdx.x * SC_THREADS + threadIdx.x;
  if (k >= K) return;
  const int p = sc_clamp(pair_pred[k], 0, P - 1), t = sc_clamp(pair_truth[k], 0, T - 1);
  int m = 0;
  if (pred_best[p] == k && truth_best[t] == k) {
    const float iou = pair_iou[k];
#pragma unroll
    for (int j = 0; j < R3D_SCENE_MATCH_IOU; ++j) m += j < n_iou && iou >= th.v[j];
  }
  pair_match[k] = (unsigned char)m;
}

extern "C" int r3d_scene_match_best(long M, long n_pred, long n_truth, long n_pairs, const int32_t* pred_points,
                                    const int32_t* truth_points, const int64_t* pred_classes, const int64_t* truth_classes,
                                    const float* thresholds, int n_iou, int32_t* pair_pred, int32_t* pair_truth, int32_t* pair_points,
                                    float* pair_iou, int32_t* pred_best, int32_t* truth_best, uint8_t* pair_match, int64_t* best_words,
                                    const int32_t* ws, long ws_words, void* stream) {
  R3D_REQUIRE(pred_points && truth_points && thresholds && pred_best && truth_best && best_words && ws,
              "r3d_scene_match_best: null pointer (pred_points %p, truth_points %p, thresholds %p, pred_best %p, truth_best %p, "
              "best_words %p, ws %p)", (const void*)pred_points, (const void*)truth_points, (const void*)thresholds, (void*)pred_best,
              (void*)truth_best, (void*)best_words, (const void*)ws);
  SC_TRY(mt_check("r3d_scene_match_best", M, ws_words));
  R3D_REQUIRE(n_pred >= 1 && n_pred <= M && n_truth >= 1 && n_truth <= M && n_pairs >= 0 && n_pairs <= M,
              "r3d_scene_match_best: %ld and %ld rows, %ld pairs of %ld points", n_pred, n_truth, n_pairs, M);
  R3D_REQUIRE(n_iou >= 1 && n_iou <= R3D_SCENE_MATCH_IOU, "r3d_scene_match_best: %d thresholds (1 .. %d)", n_iou, R3D_SCENE_MATCH_IOU);
  R3D_REQUIRE((pred_classes != nullptr) == (truth_classes != nullptr), "r3d_scene_match_best: classes for one column only "
              "(pred_classes %p, truth_classes %p)", (const void*)pred_classes, (const void*)truth_classes);
  R3D_REQUIRE(n_pairs == 0 || (pair_pred && pair_truth && pair_points && pair_iou && pair_match),
              "r3d_scene_match_best: null pointer (pair_pred %p, pair_truth %p, pair_points %p, pair_iou %p, pair_match %p)",
              (void*)pair_pred, (void*)pair_truth, (void*)pair_points, (void*)pair_iou, (void*)pair_match);
  mt_thresholds th;
  for (int j = 0; j < R3D_SCENE_MATCH_IOU; ++j) th.v[j] = j < n_iou ? thresholds[j] : 2.0f;  // thresholds: host memory
  for (int j = 0; j < n_iou; ++j)
    R3D_REQUIRE(th.v[j] > 0.0f && th.v[j] <= 1.0f && (j == 0 || th.v[j] >= th.v[j - 1]),
                "r3d_scene_match_best: threshold %d is %g (ascending, each in (0, 1])", j, (double)th.v[j]);
  const hipStream_t st = (hipStream_t)stream;
  const mt_layout L = mt_make_layout(M);
  const int P = (int)n_pred, T = (int)n_truth, K = (int)n_pairs;
  unsigned long long* pbest = (unsigned long long*)best_words;  // P words, then T: the caller's scratch
  unsigned long long* tbest = pbest + P;
  hipLaunchKernelGGL(r3d_scene_match_best_fill_kernel, dim3(sc_grid_of(P > T ? P : T)), dim3(SC_THREADS), 0, st, P, T, pred_best,
                     truth_best, pbest, tbest);
  if (K > 0) {
    const int gk = sc_grid_of(K), gkp = sc_grid_of(K > P ? K : P);
    hipLaunchKernelGGL(r3d_scene_match_pair_iou_kernel, dim3(gk), dim3(SC_THREADS), 0, st, K, P, T, ws + L.pair_start, ws + L.pair_p,
                       ws + L.pair_t, pred_points, truth_points, (const long long*)pred_classes, (const long long*)truth_classes,
                       pair_pred, pair_truth, pair_points, pair_iou, pair_match, tbest);
    hipLaunchKernelGGL(r3d_scene_match_pred_best_kernel, dim3(gk), dim3(SC_THREADS), 0, st, K, P, pair_pred, pair_iou, pair_match,
                       pbest);
    hipLaunchKernelGGL(r3d_scene_match_best_rows_kernel, dim3(gkp), dim3(SC_THREADS), 0, st, K, P, T, pair_pred, pair_truth, pair_iou,
                       pair_match, pbest, tbest, pred_best, truth_best);
    hipLaunchKernelGGL(r3d_scene_match_pair_match_kernel, dim3(gk), dim3(SC_THREADS), 0, st, K, P, T, pair_pred, pair_truth, pair_iou,
                       pred_best, truth_best, n_iou, th, pair_match);
  }
  R3D_LAUNCH_CHECK("r3d_scene_match_best");
  return R3D_OK;
}
