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
//
// Partial noise (flags bit 2, steps P0-P7 of the definition; replaces loader.py:239-322: one wrong object joins a support
// mask, with probability 0.3 one right object leaves it) is the PARTIAL instantiation of the same kernel: a support cloud
// with m_A == 0 whose mask is edited per distinct OBJECT (instance id) of its N slots.  The objects are found by a
// bitonic sort of 64-bit keys (id biased to unsigned << 32 | slot) in LDS: a run of equal ids is an object, its head the
// object's lowest slot; run ids by ballot counts, the objects' flags by integer atomicOr, the r-th eligible / foreground
// object by ballot counts over the runs.  Integers only, nothing depends on scheduling, no step grows with the number of
// objects beyond the sort.  Without bit 2 a cloud takes the path of the plain kernel and gets its bits.
#include "common.h"

#define EC_THREADS 256
#define EC_WAVES (EC_THREADS / R3D_WAVE)
#define EC_MAX_N 8192          // slots of a cloud live in LDS (32 KiB at most)
#define EC_MAX_WAY 32

struct ec_shared {
  int cnt[256];
  int wsum[EC_WAVES];
  int pack[2][EC_WAVES];
  int digit, rem;
  float red[6][EC_WAVES];
  int pick[2];  // (PARTIAL) sorted positions of the heads of the flipped and of the dropped object
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

// rec[2] += 1 for a partial cloud whose final mask holds no point, rec[3] = 1 + the highest such cloud; the cloud is written
static __device__ __forceinline__ void ec_empty(int* __restrict__ rec, int cloud) {
  if (threadIdx.x == 0) {
    atomicAdd(&rec[2], 1);
    atomicMax(&rec[3], cloud + 1);
  }
}

// How many threads before this one (thread order) hold `a`, how many hold `b` (low / high half of the result), and the
// workgroup's totals packed the same way.  One barrier per call: consecutive calls alternate `par`.
static __device__ __forceinline__ int ec_count_before(bool a, bool b, int par, ec_shared& sh, int& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  const unsigned long long ma = __ballot(a), mb = __ballot(b);
  if (lane == 0) sh.pack[par][w] = __popcll(ma) | (__popcll(mb) << 16);  // at most 64 each
  __syncthreads();
  int before = 0, tot = 0;
#pragma unroll
  for (int k = 0; k < EC_WAVES; ++k) {
    const int s = sh.pack[par][k];
    if (k < w) before += s;
    tot += s;
  }
  total = tot;
  return before + (__popcll(ma & below) | (__popcll(mb & below) << 16));
}

// The smallest power of two that holds the N keys of the sort (host and device size the LDS with it)
static __host__ __device__ __forceinline__ int ec_pow2(int N) {
  int P = 1;
  while (P < N) P <<= 1;
  return P;
}

struct ec_edit {  // what P3-P5 decide for one cloud (uniform)
  int flip, drop;  // 0 / 1: the object joins / leaves the mask
  int o_flip, o_drop;
};

// P3-P5 for one partial cloud: the objects of the N slots, the flip, the drop, and the record info[0 .. 8).  keys: P
// 64-bit words, runs: N ints, both in LDS.  Every thread of the workgroup calls it; slots are complete and visible.
// Returns the points of the final mask.
static __device__ int ec_partial(const int* __restrict__ lab, const int* __restrict__ inst, int c, unsigned hA, int N,
                                 const int* __restrict__ slots, unsigned long long* __restrict__ keys, int* __restrict__ runs,
                                 ec_shared& sh, ec_edit& ed, int* __restrict__ info) {
  const int tid = threadIdx.x;
  const int P = ec_pow2(N);
  // P3: sort (id biased to unsigned, slot); the padding sorts behind every key (a slot is below 2^32 - 1)
  for (int t = tid; t < P; t += EC_THREADS)
    keys[t] = t < N ? ((unsigned long long)((unsigned)inst[slots[t]] ^ 0x80000000u) << 32) | (unsigned)t : ~0ull;
  for (int t = tid; t < N; t += EC_THREADS) runs[t] = 0;
  __syncthreads();
#ifndef EC_PROBE_NO_SORT  // probe build for timing alone (profiles/r17_episode_partial.md): wrong objects, every index in bounds
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int x = tid; x < (P >> 1); x += EC_THREADS) {
        const int i = 2 * x - (x & (j - 1)), l = i | j;  // i: bit j clear; every pair once
        const unsigned long long a = keys[i], b = keys[l];
        if ((a > b) == ((i & k) == 0)) {
          keys[i] = b;
          keys[l] = a;
        }
      }
      __syncthreads();
    }
  }
#endif
  // runs of equal ids: run r = the r-th object o_r; runs[r] = head position << 2 | fg << 1 | eligible.  The head of a run
  // is the object's lowest slot (the slot is the low word of the key).
  const int lab0 = lab[slots[0]];
  int K = 0, other = 0, par = 0;
  for (int p0 = 0; p0 < N; p0 += EC_THREADS, par ^= 1) {
    const int p = p0 + tid;
    const bool in = p < N;
    unsigned long long key = 0;
    bool head = false;
    int l = lab0;
    if (in) {
      key = keys[p];
      head = p == 0 || (unsigned)(keys[p - 1] >> 32) != (unsigned)(key >> 32);
      l = lab[slots[(int)(unsigned)key]];
    }
    int total;
    const int before = ec_count_before(head, l != lab0, par, sh, total);
    if (in) {
      const int r = K + (before & 0xffff) + (head ? 1 : 0) - 1;  // heads up to and with p, less one: 0 .. N - 1
      const int bits = (head ? (p << 2) | (l != c ? 1 : 0) : 0) | (l == c ? 2 : 0);
      if (bits) atomicOr(&runs[r], bits);  // integer or: the order does not matter
    }
    K += total & 0xffff;
    other += total >> 16;
  }
  __syncthreads();
  const bool multi = K > 1 && other > 0;
  // e eligible and f foreground objects
  int ne = 0;
  for (int r = tid; r < K; r += EC_THREADS) {
    const int v = runs[r];
    ne += (v & 1) | ((v & 2) << 15);
  }
  int tot;
  r3d_block_excl_scan<EC_THREADS>(ne, sh.wsum, tot);  // (both halves stay below 2^16: at most N = 8192 objects)
  const int e = tot & 0xffff, f = tot >> 16;
  // P4, P5: which object
  const bool flip = multi && e > 0;
  const bool drawn = r3d_draw(hA, 1u) > 0xB3333333u && f > 0;
  const int rf = flip ? (int)(((unsigned long long)r3d_draw(hA, 0u) * (unsigned long long)e) >> 32) : -1;
  const int rd = drawn ? (int)(((unsigned long long)r3d_draw(hA, 2u) * (unsigned long long)f) >> 32) : -1;
  int be = 0, bf = 0;
  if (flip || drawn) {
    for (int r0 = 0; r0 < K; r0 += EC_THREADS, par ^= 1) {
      const int r = r0 + tid;
      const int v = r < K ? runs[r] : 0;
      int total;
      const int before = ec_count_before(v & 1, v & 2, par, sh, total);
      if ((v & 1) && be + (before & 0xffff) == rf) sh.pick[0] = v >> 2;  // exactly one thread each
      if ((v & 2) && bf + (before >> 16) == rd) sh.pick[1] = v >> 2;
      be += total & 0xffff;
      bf += total >> 16;
    }
  }
  __syncthreads();
  const int o_flip = flip ? (int)((unsigned)(keys[sh.pick[0]] >> 32) ^ 0x80000000u) : 0;
  const int o_drop = drawn ? (int)((unsigned)(keys[sh.pick[1]] >> 32) ^ 0x80000000u) : 0;
  // the slots either object holds, and the points of the mask after the flip and after the drop
  int n01 = 0, n23 = 0;
  for (int t = tid; t < N; t += EC_THREADS) {
    const int s = slots[t], i = inst[s];
    const bool isf = flip && i == o_flip, isd = drawn && i == o_drop;
    const bool m1 = lab[s] == c || isf;
    n01 += (isf ? 1 : 0) | (isd ? 1 << 16 : 0);
    n23 += (m1 ? 1 : 0) | (m1 && !isd ? 1 << 16 : 0);
  }
  int t01, t23;
  r3d_block_excl_scan<EC_THREADS>(n01, sh.wsum, t01);
  r3d_block_excl_scan<EC_THREADS>(n23, sh.wsum, t23);
  const bool drop = drawn && (t23 >> 16) > 0;  // a drop that would empty the mask is not applied
  ed.flip = flip;
  ed.drop = drop;
  ed.o_flip = o_flip;
  ed.o_drop = drop ? o_drop : 0;
  if (tid == 0) {
    info[0] = K;
    info[1] = e;
    info[2] = f;
    info[3] = (flip ? 1 : 0) | (drop ? 2 : 0) | (drawn && !drop ? 4 : 0);
    info[4] = o_flip;
    info[5] = flip ? (t01 & 0xffff) : 0;
    info[6] = ed.o_drop;
    info[7] = drop ? (t01 >> 16) : 0;
  }
  return drop ? (t23 >> 16) : (t23 & 0xffff);
}

// PARTIAL = false is r3d_episode_cut; PARTIAL = true adds flags bit 2, the instance ids and the per-cloud record `info`.
template <bool PARTIAL>
__global__ __launch_bounds__(EC_THREADS) void r3d_episode_cut_kernel(
    const float* __restrict__ points, const int* __restrict__ labels, const long long* __restrict__ offsets, int n_blocks,
    long long T, const int* __restrict__ desc, const int* __restrict__ classes, int n_way, int S, int Q, int N, unsigned seed,
    int rgb_ch, int XYZ_ch, float* __restrict__ out, long o_sb, long o_sc, long o_sn, int* __restrict__ mask,
    int* __restrict__ gt_mask, long long* __restrict__ query_y, long long* __restrict__ gt_query_y,
    int* __restrict__ slot_map, int* __restrict__ rec, const int* __restrict__ instances, int* __restrict__ info) {
  // PARTIAL: P 64-bit sort keys in front (P = ec_pow2(N)) and N run words behind the slots
  extern __shared__ __attribute__((aligned(16))) int ec_dyn[];
  int* ec_slots = ec_dyn + (PARTIAL ? 2 * ec_pow2(N) : 0);  // N ints (32-bit accesses only)
  __shared__ ec_shared sh;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int e = b / (S + Q), pos = b - e * (S + Q);
  const bool query = pos >= S;  // where the cloud's labels go follows from its position; the descriptor must agree
  const int* d = desc + 5L * b;
  const int block = d[0], c = d[1], mA = d[2], flags = d[3];
  const unsigned key = (unsigned)d[4];
  constexpr int kFlags = R3D_CUT_FLAG_QUERY | R3D_CUT_FLAG_GT_ZERO | (PARTIAL ? R3D_CUT_FLAG_PARTIAL : 0);  // the legal ones
  // every index below is bounded here, whatever the descriptor and the offsets hold (all of it uniform)
  if (block < 0 || block >= n_blocks || mA < 0 || mA > N || (flags & ~kFlags) != 0 || ((flags & R3D_CUT_FLAG_QUERY) != 0) != query) {
    ec_refuse(rec, b);
    return;
  }
  const bool partial = PARTIAL && (flags & R3D_CUT_FLAG_PARTIAL) != 0;
  if (partial && (query || mA != 0 || !instances)) {  // P0
    ec_refuse(rec, b);
    return;
  }
  const long long off0 = offsets[block], off1 = offsets[block + 1];
  if (off0 < 0 || off1 > T || off1 <= off0 || off1 - off0 > R3D_CUT_MAX_BLOCK_POINTS) {
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

  ec_edit ed = {0, 0, 0, 0};
  const int* inst = nullptr;
  if (PARTIAL) {
    int* rec8 = info + 8L * b;
    if (partial) {
      inst = instances + off0;
      const int left = ec_partial(lab, inst, c, hA, N, ec_slots, (unsigned long long*)ec_dyn, ec_slots + N, sh, ed, rec8);
      if (left == 0) ec_empty(rec, b);
    } else if (tid < 8) {
      rec8[tid] = 0;
    }
  }

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
      int me = m;
      if (PARTIAL && partial) {  // P6: set, then cleared
        const int i = inst[s];
        if (ed.flip && i == ed.o_flip) me = 1;
        if (ed.drop && i == ed.o_drop) me = 0;
      }
      mask[sup * N + t] = me;
      gt_mask[sup * N + t] = (flags & R3D_CUT_FLAG_GT_ZERO) ? 0 : m;
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

// the argument checks and the launch of both entry points (name: the one that speaks in an error)
template <bool PARTIAL>
static int ec_launch(const char* name, const float* points, const int32_t* labels, const int64_t* offsets, int n_blocks, long T,
                     const int32_t* desc, const int32_t* classes, int E, int n_way, int S, int Q, int N, unsigned seed, int C,
                     int rgb_ch, int XYZ_ch, float* out, long o_sb, long o_sc, long o_sn, int32_t* mask, int32_t* gt_mask,
                     int64_t* query_y, int64_t* gt_query_y, int32_t* slot_map, int32_t* rec, const int32_t* instances,
                     int32_t* info, void* stream) {
  R3D_REQUIRE(points && labels && offsets && desc && classes && out && slot_map && rec,
              "%s: null pointer (points %p, labels %p, offsets %p, desc %p, classes %p, out %p, slot_map %p, rec %p)", name,
              (const void*)points, (const void*)labels, (const void*)offsets, (const void*)desc, (const void*)classes,
              (void*)out, (void*)slot_map, (void*)rec);
  R3D_REQUIRE(n_blocks > 0 && T > 0 && T < (1L << 31), "%s: %d blocks, %ld pool rows (1 .. 2^31 - 1)", name, n_blocks, T);
  R3D_REQUIRE(E > 0 && S > 0 && Q >= 0 && (long)E * (S + Q) < (1L << 24), "%s: E %d, S %d, Q %d", name, E, S, Q);
  R3D_REQUIRE(mask && gt_mask, "%s: null pointer (mask %p, gt_mask %p)", name, (void*)mask, (void*)gt_mask);
  R3D_REQUIRE(Q == 0 || (query_y && gt_query_y), "%s: null pointer (query_y %p, gt_query_y %p)", name, (void*)query_y,
              (void*)gt_query_y);
  R3D_REQUIRE(n_way >= 1 && n_way <= EC_MAX_WAY, "%s: n_way %d (1 .. %d)", name, n_way, EC_MAX_WAY);
  R3D_REQUIRE(N > 0 && N <= EC_MAX_N, "%s: N %d points per cloud (1 .. %d)", name, N, EC_MAX_N);
  R3D_REQUIRE(C == 3 || C == 6 || C == 9, "%s: C %d (3, 6 or 9 channels)", name, C);
  R3D_REQUIRE(rgb_ch == -1 || rgb_ch == 3, "%s: rgb_ch %d (3, or -1: none)", name, rgb_ch);
  R3D_REQUIRE(XYZ_ch == -1 || XYZ_ch == (rgb_ch == 3 ? 6 : 3), "%s: XYZ_ch %d (behind xyz and rgb, or -1: none)", name, XYZ_ch);
  R3D_REQUIRE(C == 3 + (rgb_ch >= 0 ? 3 : 0) + (XYZ_ch >= 0 ? 3 : 0), "%s: C %d does not hold xyz%s%s", name, C,
              rgb_ch >= 0 ? " rgb" : "", XYZ_ch >= 0 ? " XYZ" : "");
  R3D_REQUIRE(o_sb >= 0 && o_sc > 0 && o_sn > 0, "%s: strides must be positive (out %ld %ld %ld)", name, o_sb, o_sc, o_sn);
  R3D_REQUIRE(!PARTIAL || info, "%s: null pointer (info %p)", name, (void*)info);
  // LDS from N: the slots; PARTIAL: the sort keys in front of them, the run words behind (128 KiB at N = 8192)
  const size_t lds = (size_t)N * sizeof(int) + (PARTIAL ? (size_t)ec_pow2(N) * 8 + (size_t)N * sizeof(int) : 0);
  if (lds > 64 * 1024) {  // above the default ceiling of dynamic LDS the kernel's attribute is raised first
    const int e_ = r3d_kernel_lds((const void*)r3d_episode_cut_kernel<PARTIAL>, lds);
    if (e_ != 0) {
      r3d_set_error("%s: %zu bytes of LDS for N %d refused: %s", name, lds, N, hipGetErrorString((hipError_t)e_));
      return R3D_ERR_LAUNCH;
    }
  }
  hipLaunchKernelGGL(r3d_episode_cut_kernel<PARTIAL>, dim3(E * (S + Q)), dim3(EC_THREADS), lds, (hipStream_t)stream, points,
                     labels, (const long long*)offsets, n_blocks, (long long)T, desc, classes, n_way, S, Q, N, seed, rgb_ch,
                     XYZ_ch, out, o_sb, o_sc, o_sn, mask, gt_mask, (long long*)query_y, (long long*)gt_query_y, slot_map, rec,
                     instances, info);
  R3D_LAUNCH_CHECK(name);
  return R3D_OK;
}

extern "C" int r3d_episode_cut(const float* points, const int32_t* labels, const int64_t* offsets, int n_blocks, long T,
                               const int32_t* desc, const int32_t* classes, int E, int n_way, int S, int Q, int N,
                               unsigned seed, int C, int rgb_ch, int XYZ_ch, float* out, long o_sb, long o_sc, long o_sn,
                               int32_t* mask, int32_t* gt_mask, int64_t* query_y, int64_t* gt_query_y, int32_t* slot_map,
                               int32_t* rec, void* stream) {
  return ec_launch<false>("r3d_episode_cut", points, labels, offsets, n_blocks, T, desc, classes, E, n_way, S, Q, N, seed, C,
                          rgb_ch, XYZ_ch, out, o_sb, o_sc, o_sn, mask, gt_mask, query_y, gt_query_y, slot_map, rec, nullptr,
                          nullptr, stream);
}

extern "C" int r3d_episode_cut_partial(const float* points, const int32_t* labels, const int64_t* offsets, int n_blocks,
                                       long T, const int32_t* desc, const int32_t* classes, int E, int n_way, int S, int Q,
                                       int N, unsigned seed, int C, int rgb_ch, int XYZ_ch, float* out, long o_sb, long o_sc,
                                       long o_sn, int32_t* mask, int32_t* gt_mask, int64_t* query_y, int64_t* gt_query_y,
                                       int32_t* slot_map, int32_t* rec, const int32_t* instances, int32_t* info,
                                       void* stream) {
  return ec_launch<true>("r3d_episode_cut_partial", points, labels, offsets, n_blocks, T, desc, classes, E, n_way, S, Q, N,
                         seed, C, rgb_ch, XYZ_ch, out, o_sb, o_sc, o_sn, mask, gt_mask, query_y, gt_query_y, slot_map, rec,
                         instances, info, stream);
}
