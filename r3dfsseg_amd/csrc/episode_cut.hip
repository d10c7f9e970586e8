// Cutting episode clouds from a block pool resident on the device (definition: INTEGRATION.md, "Cutting episodes on the
// device"; replaces the reference's per-cloud point draw and labels, dataloaders/loader.py:219-237, 258-276, 302-350).
//
// One workgroup per cloud.  A cloud is described by five int32 {block, share_class, m_A, flags, key}; with n the points of
// the block, N the points of the cloud, c = share_class, hA = r3d_stream(seed, 2 key), hB = r3d_stream(seed, 2 key + 1):
//   A   the m_A points of class c with the smallest (r3d_draw(hA, i), i), by ascending i, into slots 0 .. m_A - 1
//   B   n >= N: the N - m_A points with the smallest (r3d_draw(hB, i), i), by ascending i, into slots m_A .. N - 1
//   B'  n <  N: slot m_A + j = (uint64(r3d_draw(hB, j)) * n) >> 32
//   C   the prepared cloud over the N slots (r3d_prep_extent / r3d_prep_slot of common.h: r3d_scene_prepare's arithmetic)
//   D   support: mask = (label == c), gt = mask or zeros; query: y = 1 + position of the label in the episode's classes
// The m smallest are found without sorting the block: a radix select over the 32-bit draw (four passes of 256-bin
// histograms in LDS, most significant digit first; the draws are recomputed, never stored) gives the m-th smallest draw T
// and the number of points with draw == T to keep; those are the ones of lowest index.  A last pass in index order
// compacts the survivors by ballot and prefix count.  Integer counts only: no result depends on scheduling.
#include "common.h"

#define EC_THREADS 256
#define EC_WAVES (EC_THREADS / R3D_WAVE)
#define EC_MAX_N 8192          // slots of a cloud live in LDS (32 KiB at most)
#define EC_MAX_BLOCK (1 << 20)  // points of a block
#define EC_MAX_WAY 32

struct ec_shared {
  int cnt[256];
  int wsum[EC_WAVES];
  int pack[2][EC_WAVES];
  int digit, rem;
  float red[6][EC_WAVES];
};

// slots[0 .. m) = the m candidates with the smallest (r3d_draw(h, i), i), by ascending i.  Candidates: BY_CLASS ? the i
// with lab[i] == c : every i < n.  The caller guarantees m <= the number of candidates (counted from the same labels);
// whatever happens, only slots[0 .. m) are written, with values in [0, n).  Every thread of the workgroup calls it.
template <bool BY_CLASS>
static __device__ void ec_select(const int* __restrict__ lab, int n, int c, unsigned h, int m, int* __restrict__ slots,
                                 ec_shared& sh) {
  if (m <= 0) return;  // (uniform)
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  unsigned prefix = 0;
  int rem = m;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    sh.cnt[tid] = 0;
    if (tid == 0) {
      sh.digit = 255;
      sh.rem = 0;
    }
    __syncthreads();
    for (int i = tid; i < n; i += EC_THREADS) {
      if (BY_CLASS && lab[i] != c) continue;
      const unsigned d = r3d_draw(h, (unsigned)i);
      // the digits above this pass's must equal the prefix found so far (pass 0: there are none)
      if (pass == 0 || ((d ^ prefix) >> (shift + 8)) == 0u) atomicAdd(&sh.cnt[(d >> shift) & 255u], 1);  // integer counts
    }
    __syncthreads();
    const int v = sh.cnt[tid];
    int total;
    const int ex = r3d_block_excl_scan<EC_THREADS>(v, sh.wsum, total);
    if (ex < rem && rem <= ex + v) {  // the bin that holds the rem-th smallest: exactly one thread
      sh.digit = tid;
      sh.rem = rem - ex;
    }
    __syncthreads();
    prefix |= (unsigned)sh.digit << shift;
    rem = sh.rem;
    __syncthreads();  // digit / rem / cnt are rewritten by the next pass
  }
  // prefix = T, the m-th smallest draw; rem = how many of the candidates with draw == T are kept (lowest index first)
  int base_less = 0, base_tie = 0;
  const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  int par = 0;
  for (int i0 = 0; i0 < n; i0 += EC_THREADS, par ^= 1) {
    const int i = i0 + tid;
    const bool cand = i < n && (!BY_CLASS || lab[i] == c);
    const unsigned d = r3d_draw(h, (unsigned)i);
    const bool less = cand && d < prefix, tie = cand && d == prefix;
    const unsigned long long ml = __ballot(less), mt = __ballot(tie);
    if (lane == 0) sh.pack[par][w] = __popcll(ml) | (__popcll(mt) << 16);  // at most 64 each
    __syncthreads();  // (one barrier per round: the next round writes the other half of pack)
    int before = 0, total = 0;
#pragma unroll
    for (int k = 0; k < EC_WAVES; ++k) {
      const int s = sh.pack[par][k];
      if (k < w) before += s;
      total += s;
    }
    const int less_before = base_less + (before & 0xffff) + __popcll(ml & below);
    const int tie_before = base_tie + (before >> 16) + __popcll(mt & below);
    if (less || (tie && tie_before < rem)) {
      const int pos = less_before + (tie_before < rem ? tie_before : rem);
      if (pos < m) slots[pos] = i;
    }
    base_less += total & 0xffff;
    base_tie += total >> 16;
  }
}

// rec[0] += 1 for a cloud whose descriptor cannot be cut, rec[1] = 1 + the highest such cloud; the cloud writes nothing else
static __device__ __forceinline__ void ec_refuse(int* __restrict__ rec, int cloud) {
  if (threadIdx.x == 0) {
    atomicAdd(&rec[0], 1);
    atomicMax(&rec[1], cloud + 1);
  }
}

__global__ __launch_bounds__(EC_THREADS) void r3d_episode_cut_kernel(
    const float* __restrict__ points, const int* __restrict__ labels, const long long* __restrict__ offsets, int n_blocks,
    long long T, const int* __restrict__ desc, const int* __restrict__ classes, int n_way, int S, int Q, int N, unsigned seed,
    int rgb_ch, int XYZ_ch, float* __restrict__ out, long o_sb, long o_sc, long o_sn, int* __restrict__ mask,
    int* __restrict__ gt_mask, long long* __restrict__ query_y, long long* __restrict__ gt_query_y,
    int* __restrict__ slot_map, int* __restrict__ rec) {
  extern __shared__ int ec_slots[];  // N ints (32-bit accesses only)
  __shared__ ec_shared sh;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int e = b / (S + Q), pos = b - e * (S + Q);
  const bool query = pos >= S;  // where the cloud's labels go follows from its position; the descriptor must agree
  const int* d = desc + 5L * b;
  const int block = d[0], c = d[1], mA = d[2], flags = d[3];
  const unsigned key = (unsigned)d[4];
  // every index below is bounded here, whatever the descriptor and the offsets hold (all of it uniform)
  if (block < 0 || block >= n_blocks || mA < 0 || mA > N || (flags & ~3) != 0 || ((flags & 1) != 0) != query) {
    ec_refuse(rec, b);
    return;
  }
  const long long off0 = offsets[block], off1 = offsets[block + 1];
  if (off0 < 0 || off1 > T || off1 <= off0 || off1 - off0 > EC_MAX_BLOCK) {
    ec_refuse(rec, b);
    return;
  }
  const int n = (int)(off1 - off0);
  const int* lab = labels + off0;
  const float* pts = points + 6 * off0;

  // points of class c in the block: m_A may not exceed them
  int nv = 0;
  for (int i = tid; i < n; i += EC_THREADS) nv += lab[i] == c ? 1 : 0;
  int total;
  r3d_block_excl_scan<EC_THREADS>(nv, sh.wsum, total);
  if (mA > total) {
    ec_refuse(rec, b);
    return;
  }

  const unsigned hA = r3d_stream(seed, 2u * key), hB = r3d_stream(seed, 2u * key + 1u);
  const int mB = N - mA;
  ec_select<true>(lab, n, c, hA, mA, ec_slots, sh);
  if (n >= N) {
    ec_select<false>(lab, n, c, hB, mB, ec_slots + mA, sh);
  } else {
    for (int j = tid; j < mB; j += EC_THREADS)
      ec_slots[mA + j] = (int)(((unsigned long long)r3d_draw(hB, (unsigned)j) * (unsigned long long)n) >> 32);  // < n
  }
  __syncthreads();

  // C: the prepared cloud over the N slots
  float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int t = tid; t < N; t += EC_THREADS) {
    const float* q = pts + 6L * ec_slots[t];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      mn[a] = fminf(mn[a], q[a]);
      mx[a] = fmaxf(mx[a], q[a]);
    }
  }
  float lo[3], ext[3];
  r3d_prep_extent<EC_THREADS>(mn, mx, sh.red, lo, ext);
  out += (long)b * o_sb;
  const int* cls = classes + (long)e * n_way;
  const long sup = (long)e * S + pos, qry = (long)e * Q + (pos - S);
  for (int t = tid; t < N; t += EC_THREADS) {
    const int s = ec_slots[t];
    r3d_prep_slot(pts + 6L * s, lo, ext, rgb_ch, XYZ_ch, out + (long)t * o_sn, o_sc);
    // D: labels
    const int l = lab[s];
    if (!query) {
      const int m = l == c ? 1 : 0;
      mask[sup * N + t] = m;
      gt_mask[sup * N + t] = (flags & 2) ? 0 : m;
    } else {
      int y = 0;
      for (int k = n_way - 1; k >= 0; --k)
        if (cls[k] == l) y = k + 1;  // the first position that holds the label
      query_y[qry * N + t] = y;
      gt_query_y[qry * N + t] = y;
    }
    slot_map[(long)b * N + t] = (int)off0 + s;
  }
}

extern "C" int r3d_episode_cut(const float* points, const int32_t* labels, const int64_t* offsets, int n_blocks, long T,
                               const int32_t* desc, const int32_t* classes, int E, int n_way, int S, int Q, int N,
                               unsigned seed, int C, int rgb_ch, int XYZ_ch, float* out, long o_sb, long o_sc, long o_sn,
                               int32_t* mask, int32_t* gt_mask, int64_t* query_y, int64_t* gt_query_y, int32_t* slot_map,
                               int32_t* rec, void* stream) {
  R3D_REQUIRE(points && labels && offsets && desc && classes && out && slot_map && rec,
              "r3d_episode_cut: null pointer (points %p, labels %p, offsets %p, desc %p, classes %p, out %p, slot_map %p, rec %p)",
              (const void*)points, (const void*)labels, (const void*)offsets, (const void*)desc, (const void*)classes,
              (void*)out, (void*)slot_map, (void*)rec);
  R3D_REQUIRE(n_blocks > 0 && T > 0 && T < (1L << 31), "r3d_episode_cut: %d blocks, %ld pool rows (1 .. 2^31 - 1)", n_blocks, T);
  R3D_REQUIRE(E > 0 && S > 0 && Q >= 0 && (long)E * (S + Q) < (1L << 24), "r3d_episode_cut: E %d, S %d, Q %d", E, S, Q);
  R3D_REQUIRE(mask && gt_mask, "r3d_episode_cut: null pointer (mask %p, gt_mask %p)", (void*)mask, (void*)gt_mask);
  R3D_REQUIRE(Q == 0 || (query_y && gt_query_y), "r3d_episode_cut: null pointer (query_y %p, gt_query_y %p)", (void*)query_y,
              (void*)gt_query_y);
  R3D_REQUIRE(n_way >= 1 && n_way <= EC_MAX_WAY, "r3d_episode_cut: n_way %d (1 .. %d)", n_way, EC_MAX_WAY);
  R3D_REQUIRE(N > 0 && N <= EC_MAX_N, "r3d_episode_cut: N %d points per cloud (1 .. %d)", N, EC_MAX_N);
  R3D_REQUIRE(C == 3 || C == 6 || C == 9, "r3d_episode_cut: C %d (3, 6 or 9 channels)", C);
  R3D_REQUIRE(rgb_ch == -1 || rgb_ch == 3, "r3d_episode_cut: rgb_ch %d (3, or -1: none)", rgb_ch);
  R3D_REQUIRE(XYZ_ch == -1 || XYZ_ch == (rgb_ch == 3 ? 6 : 3), "r3d_episode_cut: XYZ_ch %d (behind xyz and rgb, or -1: none)",
              XYZ_ch);
  R3D_REQUIRE(C == 3 + (rgb_ch >= 0 ? 3 : 0) + (XYZ_ch >= 0 ? 3 : 0), "r3d_episode_cut: C %d does not hold xyz%s%s", C,
              rgb_ch >= 0 ? " rgb" : "", XYZ_ch >= 0 ? " XYZ" : "");
  R3D_REQUIRE(o_sb >= 0 && o_sc > 0 && o_sn > 0, "r3d_episode_cut: strides must be positive (out %ld %ld %ld)", o_sb, o_sc, o_sn);
  hipLaunchKernelGGL(r3d_episode_cut_kernel, dim3(E * (S + Q)), dim3(EC_THREADS), (size_t)N * sizeof(int), (hipStream_t)stream,
                     points, labels, (const long long*)offsets, n_blocks, (long long)T, desc, classes, n_way, S, Q, N, seed,
                     rgb_ch, XYZ_ch, out, o_sb, o_sc, o_sn, mask, gt_mask, (long long*)query_y, (long long*)gt_query_y, slot_map,
                     rec);
  R3D_LAUNCH_CHECK("r3d_episode_cut");
  return R3D_OK;
}
