// Small device-side heads around the main path, gfx950:
//   * clean-shot detection of eval_noise.py's eval=True path   (reference models/mpti.py:87-223, 316-371)
//   * ProtoNet head: masked average pooling + cosine / euclidean similarity (models/protonet.py:295-349)
//   * mIoU accumulator                                          (eval_noise.py:23-72)
// All are HBM / latency bound reductions over (S*N, D) point-major features.
#include "common.h"

#define AH_MAXSHOT 32   // n_way * k_shot
#define AH_MAXK 8       // shots per way in clean-shot detection (<= 4 seeds each)
#define AH_BOXES 5      // box 0: scale (1,1,1); boxes 1..4: scale (2,2,1), x outer / y inner
#define AH_DMAX 256

// ---------------------------------------------------------------------------
// clean-shot detection, step 1: per (shot, box) feature sums over the foreground points inside
// the box.  Box bounds replicate grid_sampling (mpti.py:316-371) in fp32, inclusive on both sides.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void r3d_clean_boxsum_kernel(
    const float* __restrict__ feat /* (S*N, ldf) */, long ldf, int D, const float* __restrict__ support_x /* (S, Cin, N) */,
    int Cin, const int* __restrict__ support_y /* (S, N) */, int N, float* __restrict__ box_sum /* (S, 5, 256) */,
    int* __restrict__ box_cnt /* (S, 5) */, long feat_ep_rows, long ws_stride) {
  {
    const long ep = blockIdx.z, S_ = gridDim.x;  // batch of episodes: rows / scratch of episode ep
    feat += ep * feat_ep_rows * ldf; support_x += ep * S_ * Cin * N; support_y += ep * S_ * N;
    box_sum += ep * ws_stride; box_cnt += ep * ws_stride;
  }
  __shared__ float red[4][6];
  __shared__ float bb[6];  // x_min, x_max, y_min, y_max, z_min, z_max
  __shared__ float psum[4][AH_DMAX];
  __shared__ int pcnt[4];
  const int shot = blockIdx.x, box = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int* my = support_y + (long)shot * N;
  const float* px = support_x + (long)shot * Cin * N;
  const float* py = px + N;
  const float* pz = px + 2 * N;
  // bounding box of the foreground points
  float xmin = INFINITY, xmax = -INFINITY, ymin = INFINITY, ymax = -INFINITY, zmin = INFINITY, zmax = -INFINITY;
  for (int p = tid; p < N; p += 256) {
    if (my[p] == 1) {
      const float x = px[p], y = py[p], z = pz[p];
      xmin = fminf(xmin, x); xmax = fmaxf(xmax, x);
      ymin = fminf(ymin, y); ymax = fmaxf(ymax, y);
      zmin = fminf(zmin, z); zmax = fmaxf(zmax, z);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    xmin = fminf(xmin, __shfl_xor(xmin, o)); xmax = fmaxf(xmax, __shfl_xor(xmax, o));
    ymin = fminf(ymin, __shfl_xor(ymin, o)); ymax = fmaxf(ymax, __shfl_xor(ymax, o));
    zmin = fminf(zmin, __shfl_xor(zmin, o)); zmax = fmaxf(zmax, __shfl_xor(zmax, o));
  }
  if (lane == 0) { red[w][0] = xmin; red[w][1] = xmax; red[w][2] = ymin; red[w][3] = ymax; red[w][4] = zmin; red[w][5] = zmax; }
  __syncthreads();
  if (tid < 6) {
    const float a = red[0][tid], b = red[1][tid], c = red[2][tid], d = red[3][tid];
    bb[tid] = (tid & 1) ? fmaxf(fmaxf(a, b), fmaxf(c, d)) : fminf(fminf(a, b), fminf(c, d));
  }
  __syncthreads();
  // n_z = 1 at both scales: [z_min + 0*d_z, z_min + 0*d_z + d_z] (may exclude z_max by one rounding, as the reference)
  const float dz = (bb[5] - bb[4]) / 1.f;
  const float zlo = bb[4] + 0.f * dz, zhi = zlo + dz;
  float xlo, xhi, ylo, yhi;
  if (box == 0) {  // n_x = n_y = 1: d = (max - min) / 1 ; [min + 0*d, min + 0*d + d]
    const float dx = (bb[1] - bb[0]) / 1.f, dy = (bb[3] - bb[2]) / 1.f;
    xlo = bb[0] + 0.f * dx; xhi = xlo + dx;
    ylo = bb[2] + 0.f * dy; yhi = ylo + dy;
  } else {
    const int ix = (box - 1) >> 1, iy = (box - 1) & 1;
    const float dx = (bb[1] - bb[0]) / 2.f, dy = (bb[3] - bb[2]) / 2.f;
    xlo = bb[0] + (float)ix * dx; xhi = xlo + dx;
    ylo = bb[2] + (float)iy * dy; yhi = ylo + dy;
  }
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  int cnt = 0;
  for (int base = 64 * w; base < N; base += 256) {
    const int p = base + lane;
    bool f = false;
    if (p < N && my[p] == 1) {
      const float x = px[p], y = py[p], z = pz[p];
      f = x >= xlo && x <= xhi && y >= ylo && y <= yhi && z >= zlo && z <= zhi;
    }
    unsigned long long mm = __ballot(f);
    cnt += __popcll(mm);
    while (mm) {
      const int src = __ffsll((long long)mm) - 1;
      mm &= mm - 1;
      const float* fr = feat + ((long)shot * N + base + src) * ldf;
      if (lane < D) a0 += fr[lane];
      if (lane + 64 < D) a1 += fr[lane + 64];
      if (lane + 128 < D) a2 += fr[lane + 128];
      if (lane + 192 < D) a3 += fr[lane + 192];
    }
  }
  psum[w][lane] = a0; psum[w][lane + 64] = a1; psum[w][lane + 128] = a2; psum[w][lane + 192] = a3;
  if (lane == 0) pcnt[w] = cnt;
  __syncthreads();
  box_sum[((long)shot * AH_BOXES + box) * AH_DMAX + tid] = ((psum[0][tid] + psum[1][tid]) + psum[2][tid]) + psum[3][tid];
  if (tid == 0) box_cnt[shot * AH_BOXES + box] = pcnt[0] + pcnt[1] + pcnt[2] + pcnt[3];
}

// step 2: per way: seeds (non-empty boxes, shot order, x outer / y inner) -> L2 normalise -> cosine
// map (zero diagonal; cubed at scale (1,1,1)) -> row sums > mean -> per-shot majority -> average of
// the two scales < 0.5 drops the shot; a way that loses every foreground point keeps all its shots.
__global__ __launch_bounds__(256) void r3d_clean_decide_kernel(const float* __restrict__ box_sum,
                                                               const int* __restrict__ box_cnt, int n_way, int k_shot,
                                                               int D, int* __restrict__ shot_keep /* (n_way*k_shot) */,
                                                               float* __restrict__ dbg_cos_sum /* opt (n_way, 2, 4*k_shot) */,
                                                               long ws_stride) {
  {
    const long ep = blockIdx.y;
    box_sum += ep * ws_stride; box_cnt += ep * ws_stride; shot_keep += ep * n_way * k_shot;
    if (dbg_cos_sum) dbg_cos_sum += ep * n_way * 2 * 4 * k_shot;
  }
  __shared__ float seed[4 * AH_MAXK][AH_DMAX + 1];  // <= 4 seeds per shot
  __shared__ float rowsum[4 * AH_MAXK];
  __shared__ int seed_shot[4 * AH_MAXK];
  __shared__ float flag[2][AH_MAXK];
  __shared__ int nseed_s;
  const int way = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  for (int scale = 0; scale < 2; ++scale) {
    __syncthreads();
    if (tid == 0) {
      int ns = 0;
      for (int k = 0; k < k_shot; ++k) {
        const int shot = way * k_shot + k;
        const int b0 = scale == 0 ? 0 : 1, b1 = scale == 0 ? 1 : 5;
        for (int b = b0; b < b1; ++b)
          if (box_cnt[shot * AH_BOXES + b] > 0) { seed_shot[ns] = (k << 8) | b; ++ns; }
      }
      nseed_s = ns;
    }
    __syncthreads();
    const int ns = nseed_s;
    // seed means, then F.normalize (x / max(||x||, 1e-12))
    for (int s = w; s < ns; s += 4) {
      const int k = seed_shot[s] >> 8, b = seed_shot[s] & 255;
      const int shot = way * k_shot + k;
      const float cnt = (float)box_cnt[shot * AH_BOXES + b];
      float sq = 0.f;
      for (int c = lane; c < D; c += 64) {
        const float v = box_sum[((long)shot * AH_BOXES + b) * AH_DMAX + c] / cnt;
        seed[s][c] = v;
        sq += v * v;
      }
      sq = r3d_wave_sum(sq);
      const float nrm = fmaxf(sqrtf(sq), 1e-12f);
      for (int c = lane; c < D; c += 64) seed[s][c] = seed[s][c] / nrm;
    }
    __syncthreads();
    // row sums of the (masked, optionally cubed) cosine map
    for (int i = w; i < ns; i += 4) {
      float rs = 0.f;
      for (int j = 0; j < ns; ++j) {
        float d = 0.f;
        for (int c = lane; c < D; c += 64) d += seed[i][c] * seed[j][c];
        d = r3d_wave_sum(d);
        if (j == i) d = 0.f;
        if (scale == 0) d = d * d * d;
        rs += d;
      }
      if (lane == 0) {
        rowsum[i] = rs;
        if (dbg_cos_sum) dbg_cos_sum[(way * 2 + scale) * 4 * k_shot + i] = rs;
      }
    }
    __syncthreads();
    if (tid == 0) {
      float mean = 0.f;
      for (int i = 0; i < ns; ++i) mean += rowsum[i];
      mean /= (float)ns;
      for (int k = 0; k < k_shot; ++k) {
        int tot = 0, pos = 0;
        for (int i = 0; i < ns; ++i)
          if ((seed_shot[i] >> 8) == k) { ++tot; pos += rowsum[i] > mean ? 1 : 0; }
        flag[scale][k] = (tot > 0 && ((float)pos / (float)tot) > 0.5f) ? 1.f : 0.f;
      }
    }
  }
  __syncthreads();
  if (tid == 0) {
    bool any = false;
    for (int k = 0; k < k_shot; ++k) {
      const float total = (flag[0][k] + flag[1][k]) / 2.f;
      const int keep = total < 0.5f ? 0 : 1;
      shot_keep[way * k_shot + k] = keep;
      any = any || keep;
    }
    if (!any)  // every foreground point would be dropped: reset to all ones (mpti.py:216-219)
      for (int k = 0; k < k_shot; ++k) shot_keep[way * k_shot + k] = 1;
  }
}

// ---------------------------------------------------------------------------
// ProtoNet head (models/protonet.py:295-349)
// ---------------------------------------------------------------------------
// masked sums of one support cloud: fg (mask == 1) and bg (mask == 0)
__global__ __launch_bounds__(256) void r3d_proto_pool_kernel(const float* __restrict__ feat, long ldf, int D,
                                                             const int* __restrict__ support_y, int N,
                                                             float* __restrict__ pooled /* (S, 2, 256): fg, bg */) {
  const int shot = blockIdx.x, tid = threadIdx.x;
  const int* my = support_y + (long)shot * N;
  float fg = 0.f, bg = 0.f;
  int nfg = 0;
  if (tid < D) {
    for (int p = 0; p < N; ++p) {  // rows are read coalesced across the D threads
      const float v = feat[((long)shot * N + p) * ldf + tid];
      const int m = my[p];
      fg += v * (float)m;
      bg += v * (float)(m == 0);
      nfg += m;
    }
    // getMaskedFeatures: sum(feat * mask) / (mask.sum() + 1e-5)
    pooled[((long)shot * 2 + 0) * AH_DMAX + tid] = fg / ((float)nfg + 1e-5f);
    pooled[((long)shot * 2 + 1) * AH_DMAX + tid] = bg / ((float)(N - nfg) + 1e-5f);
  }
}

// prototypes (getPrototype) + per-point similarity (calculateSimilarity) -> Z rows (n_q*N, 4).  Workgroup `blk` of `nblk`
// takes every nblk-th group of 4 query points, one wave per point: a point's arithmetic does not depend on the grid.
// keep (n_way*k_shot) or null: a way's foreground prototype is the mean of its kept shots (getPrototype(clean_flag=...),
// protonet.py:904-911), walked in shot order as without it -- all kept: the same additions, the same divisor --; the
// background prototype takes every shot either way.  keep[...] is the same word for every lane: the branch is wave-uniform.
// The two halves are device functions of their own: the fused kernels (one launch pair per head) and the fitted-support
// kernels (prototype table written out once, similarity against it later) run the SAME arithmetic.
// ah_build_protos: thread tid < D leaves channel tid of the n_way + 1 prototypes in proto[0 .. n_way][tid].
static __device__ __forceinline__ void ah_build_protos(const float* __restrict__ pooled, const int* __restrict__ keep, int n_way,
                                                       int k_shot, int D, float (*proto)[AH_DMAX]) {
  const int tid = threadIdx.x;
  if (tid < D) {
    float bgp = 0.f;
    for (int s = 0; s < n_way * k_shot; ++s) bgp += pooled[((long)s * 2 + 1) * AH_DMAX + tid];
    proto[0][tid] = bgp / (float)(n_way * k_shot);
    for (int wy = 0; wy < n_way; ++wy) {
      float f = 0.f;
      int n_kept = 0;
      for (int k = 0; k < k_shot; ++k) {
        if (keep && keep[wy * k_shot + k] == 0) continue;
        f += pooled[((long)(wy * k_shot + k) * 2 + 0) * AH_DMAX + tid];
        ++n_kept;
      }
      proto[wy + 1][tid] = f / (float)n_kept;  // (no kept shot: 0 / 0, the caller's error -- r3d.h)
    }
  }
}
// ah_sim_points: proto[0 .. n_way][0 .. D) filled by the workgroup's threads (not yet synchronised) -> the Z rows of its points
static __device__ __forceinline__ void ah_sim_points(float (*proto)[AH_DMAX], float* pnorm, int n_way,
                                                     const float* __restrict__ qfeat, long ldq, int D, int n_pts, int method,
                                                     float scaler, float4* __restrict__ Zq, float4* __restrict__ Zq2, int blk,
                                                     int nblk) {
  const int tid = threadIdx.x;
  const int n_classes = n_way + 1;
  __syncthreads();
  if (tid < D)
    for (int k = n_classes; k < 8; ++k) proto[k][tid] = 0.f;
  if (tid < 8) {
    float s = 0.f;
    if (tid < n_classes) for (int c = 0; c < D; ++c) s += proto[tid][c] * proto[tid][c];
    pnorm[tid] = sqrtf(s);
  }
  __syncthreads();
  const int lane = tid & 63, w = tid >> 6;
  for (int p = blk * 4 + w; p < n_pts; p += nblk * 4) {  // one wave per query point
    const float* q = qfeat + (long)p * ldq;
    float dot[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, qq = 0.f, dd[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int c = lane; c < D; c += 64) {
      const float v = q[c];
      qq += v * v;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        dot[k] += v * proto[k][c];
        const float df = (v - proto[k][c]) + 1e-6f;  // pairwise_distance eps (torch 1.8 semantics)
        dd[k] += df * df;
      }
    }
    qq = r3d_wave_sum(qq);
    float out[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float d = r3d_wave_sum(dot[k]);
      const float e = r3d_wave_sum(dd[k]);
      if (method == 0) out[k] = d / fmaxf(sqrtf(qq) * pnorm[k], 1e-8f) * scaler;
      else { const float dist = sqrtf(e); out[k] = -(dist * dist); }
      if (k >= n_classes) out[k] = 0.f;
    }
    if (lane == 0) Zq[p] = make_float4(out[0], out[1], out[2], out[3]);
    if (lane == 0 && Zq2) Zq2[p] = make_float4(out[4], out[5], out[6], out[7]);
  }
}
static __device__ __forceinline__ void ah_proto_sim(const float* __restrict__ pooled, const int* __restrict__ keep, int n_way,
                                                    int k_shot, const float* __restrict__ qfeat, long ldq, int D, int n_pts,
                                                    int method, float scaler, float4* __restrict__ Zq, float4* __restrict__ Zq2,
                                                    int blk, int nblk) {
  __shared__ float proto[8][AH_DMAX];
  __shared__ float pnorm[8];
  ah_build_protos(pooled, keep, n_way, k_shot, D, proto);
  ah_sim_points(proto, pnorm, n_way, qfeat, ldq, D, n_pts, method, scaler, Zq, Zq2, blk, nblk);
}

__global__ __launch_bounds__(256) void r3d_proto_sim_kernel(const float* __restrict__ pooled, int n_way, int k_shot,
                                                            const float* __restrict__ qfeat, long ldq, int D, int n_pts,
                                                            int method /*0 cosine, 1 euclidean*/, float scaler,
                                                            float4* __restrict__ Zq, float4* __restrict__ Zq2 /* classes 4..7 */) {
  ah_proto_sim(pooled, nullptr, n_way, k_shot, qfeat, ldq, D, n_pts, method, scaler, Zq, Zq2, blockIdx.x, gridDim.x);
}

// ---- the same head for a batch of episodes: grid axis y is the episode in both kernels ------------------------------------
// Pooling: r3d_proto_pool_kernel's two chains per channel, row after row in its order with its operations -- bit for bit its
// sums -- with the loads of 8 rows in flight instead of one.  grid (S, n_ep); pooled: episode e at + e * S * 2 * 256.
__global__ __launch_bounds__(256) void r3d_proto_pool_ep_kernel(const float* __restrict__ feat, long ldf, long feat_ep_rows,
                                                                int D, const int* __restrict__ support_y, int N,
                                                                float* __restrict__ pooled) {
  const int shot = blockIdx.x, S = gridDim.x, tid = threadIdx.x;
  const long ep = blockIdx.y;
  if (tid >= D) return;
  const int* my = support_y + (ep * S + shot) * N;
  const float* f = feat + (ep * feat_ep_rows + (long)shot * N) * ldf + tid;  // rows are read coalesced across the D threads
  float fg = 0.f, bg = 0.f;
  int nfg = 0;
  int p = 0;
  for (; p + 8 <= N; p += 8) {
    float v[8];
    int m[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      v[u] = f[(long)(p + u) * ldf];
      m[u] = my[p + u];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      fg += v[u] * (float)m[u];
      bg += v[u] * (float)(m[u] == 0);
      nfg += m[u];
    }
  }
  for (; p < N; ++p) {
    const float v = f[(long)p * ldf];
    const int m = my[p];
    fg += v * (float)m;
    bg += v * (float)(m == 0);
    nfg += m;
  }
  float* out = pooled + (ep * S + shot) * 2 * AH_DMAX;
  // getMaskedFeatures: sum(feat * mask) / (mask.sum() + 1e-5)
  out[tid] = fg / ((float)nfg + 1e-5f);
  out[AH_DMAX + tid] = bg / ((float)(N - nfg) + 1e-5f);
}

// grid (query tiles, n_ep); shot_keep (n_ep, n_way*k_shot) or null
__global__ __launch_bounds__(256) void r3d_proto_sim_ep_kernel(const float* __restrict__ pooled,
                                                               const int* __restrict__ shot_keep, int n_way, int k_shot,
                                                               const float* __restrict__ qfeat, long ldq, long feat_ep_rows,
                                                               int D, int n_pts, int method, float scaler,
                                                               float4* __restrict__ Zq, float4* __restrict__ Zq2) {
  const long ep = blockIdx.y;
  ah_proto_sim(pooled + ep * n_way * k_shot * 2 * AH_DMAX, shot_keep ? shot_keep + ep * n_way * k_shot : nullptr, n_way, k_shot,
               qfeat + ep * feat_ep_rows * ldq, ldq, D, n_pts, method, scaler, Zq + ep * n_pts,
               Zq2 ? Zq2 + ep * n_pts : nullptr, blockIdx.x, gridDim.x);
}

// ---- the head in two calls (a fitted support set): prototype table out, similarity against a table -------------------------
// grid (n_ep): ah_build_protos of episode e -> protos (n_ep, n_way + 1, D)
__global__ __launch_bounds__(256) void r3d_proto_table_kernel(const float* __restrict__ pooled,
                                                              const int* __restrict__ shot_keep, int n_way, int k_shot, int D,
                                                              float* __restrict__ protos) {
  __shared__ float proto[8][AH_DMAX];
  const long ep = blockIdx.x;
  const int tid = threadIdx.x;
  ah_build_protos(pooled + ep * n_way * k_shot * 2 * AH_DMAX, shot_keep ? shot_keep + ep * n_way * k_shot : nullptr, n_way,
                  k_shot, D, proto);
  if (tid < D)  // (a thread reads back the channel it wrote)
    for (int c = 0; c <= n_way; ++c) protos[(ep * (n_way + 1) + c) * D + tid] = proto[c][tid];
}
// grid (query tiles, n_sys): system g's table at protos + g * proto_stride (0: one table for all), its rows q_sys_rows
// rows after system g - 1's
__global__ __launch_bounds__(256) void r3d_proto_sim_table_kernel(const float* __restrict__ protos, long proto_stride, int n_way,
                                                                  const float* __restrict__ qfeat, long ldq, long q_sys_rows,
                                                                  int D, int n_pts, int method, float scaler,
                                                                  float4* __restrict__ Zq, float4* __restrict__ Zq2) {
  __shared__ float proto[8][AH_DMAX];
  __shared__ float pnorm[8];
  const long g = blockIdx.y;
  const int tid = threadIdx.x;
  const float* t = protos + g * proto_stride;
  if (tid < D)
    for (int c = 0; c <= n_way; ++c) proto[c][tid] = t[(long)c * D + tid];
  ah_sim_points(proto, pnorm, n_way, qfeat + g * q_sys_rows * ldq, ldq, D, n_pts, method, scaler, Zq + g * n_pts,
                Zq2 ? Zq2 + g * n_pts : nullptr, blockIdx.x, gridDim.x);
}

// ---- K prototype tables against the same query rows (predict_scene_sets) -----------------------------------------------------
// grid (query tiles, n_groups).  All K tables of a workgroup sit in LDS, R = K * (n_way + 1) <= 64 rows with an odd pitch
// (the norm pass walks a row per thread), and a query row is read ONCE: one wave per point, its D <= 256 channels in four
// registers per lane, then row after row of the tables against them.  Per (point, prototype) the operations of
// ah_sim_points in its order -- channels lane, lane + 64, ... into one chain per lane, r3d_wave_sum, the same final
// expression -- so set k's rows have the bits of r3d_proto_sim_table_kernel on table k alone.  Only the distance the
// method asks for is formed (ah_sim_points forms both and drops one).  System g * K + k: rows [(g K + k) n_pts, ...) of Z.
__global__ __launch_bounds__(256) void r3d_proto_sim_sets_kernel(const float* __restrict__ protos, long proto_stride, int K,
                                                                 int n_way, const float* __restrict__ qfeat, long ldq,
                                                                 long q_sys_rows, int D, int n_pts, int method, float scaler,
                                                                 float4* __restrict__ Zq, float4* __restrict__ Zq2) {
  extern __shared__ float ah_sets[];  // [R][pitch] prototype rows, then [R] their norms
  const int C = n_way + 1, R = K * C, pitch = D | 1;
  float* pnorm = ah_sets + R * pitch;
  const long g = blockIdx.y;
  const int tid = threadIdx.x;
  for (int i = tid; i < R * D; i += 256) {
    const int r = i / D, c = i - r * D;
    ah_sets[r * pitch + c] = protos[(long)(r / C) * proto_stride + (long)(r % C) * D + c];
  }
  __syncthreads();
  if (tid < R) {
    float s = 0.f;
    for (int c = 0; c < D; ++c) s += ah_sets[tid * pitch + c] * ah_sets[tid * pitch + c];
    pnorm[tid] = sqrtf(s);
  }
  __syncthreads();
  const int lane = tid & 63, w = tid >> 6;
  const float* qg = qfeat + g * q_sys_rows * ldq;
  for (int p = blockIdx.x * 4 + w; p < n_pts; p += gridDim.x * 4) {  // one wave per query point
    const float* q = qg + (long)p * ldq;
    float v[4], qq = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = lane + 64 * i;
      v[i] = c < D ? q[c] : 0.f;
      if (c < D) qq += v[i] * v[i];
    }
    qq = r3d_wave_sum(qq);
    for (int k = 0; k < K; ++k) {
      float out[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        out[j] = 0.f;
        if (j >= C) continue;
        const float* pr = ah_sets + (k * C + j) * pitch;
        float acc = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int c = lane + 64 * i;
          if (c >= D) continue;
          if (method == 0) {
            acc += v[i] * pr[c];
          } else {
            const float df = (v[i] - pr[c]) + 1e-6f;  // pairwise_distance eps (torch 1.8 semantics)
            acc += df * df;
          }
        }
        acc = r3d_wave_sum(acc);
        if (method == 0) out[j] = acc / fmaxf(sqrtf(qq) * pnorm[k * C + j], 1e-8f) * scaler;
        else { const float dist = sqrtf(acc); out[j] = -(dist * dist); }
      }
      const long row = (g * K + k) * n_pts + p;
      if (lane == 0) Zq[row] = make_float4(out[0], out[1], out[2], out[3]);
      if (lane == 0 && Zq2) Zq2[row] = make_float4(out[4], out[5], out[6], out[7]);
    }
  }
}

// correct[e] = #{pred == label} over the n_pts query points of episode e (integers: any order gives the same count).  grid (n_ep)
__global__ __launch_bounds__(256) void r3d_count_correct_kernel(const int* __restrict__ pred, const long long* __restrict__ labels,
                                                                long n_pts, int* __restrict__ correct) {
  __shared__ int part[4];
  const int tid = threadIdx.x;
  const int* pr = pred + (long)blockIdx.x * n_pts;
  const long long* lb = labels + (long)blockIdx.x * n_pts;
  int c = 0;
  for (long i = tid; i < n_pts; i += 256) c += (long long)pr[i] == lb[i] ? 1 : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
  if ((tid & 63) == 0) part[tid >> 6] = c;
  __syncthreads();
  if (tid == 0) correct[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

// ---------------------------------------------------------------------------
// mIoU accumulator (eval_noise.py:23-72): hist[0]=GT, hist[1]=predicted, hist[2]=true positive,
// per test class index (0 = background).  lut[l] = index of episode label l in test_classes (+1).
// ---------------------------------------------------------------------------
__global__ void r3d_miou_accumulate_kernel(const int* __restrict__ pred, const long long* __restrict__ gt, long n,
                                           const int* __restrict__ lut, int n_lut, int n_classes,
                                           unsigned long long* __restrict__ hist) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int g = (int)gt[i], p = pred[i];
  const int gi = lut[min(max(g, 0), n_lut - 1)], pi = lut[min(max(p, 0), n_lut - 1)];
  atomicAdd(&hist[gi], 1ull);
  atomicAdd(&hist[n_classes + pi], 1ull);
  if (g == p) atomicAdd(&hist[2 * n_classes + gi], 1ull);
}

// ===========================================================================
// C ABI
// ===========================================================================
// ws: 5*256*S floats + 5*S ints.  shot_keep (n_way*k_shot) int32 out.  dbg optional (n_way,2,4*k_shot).
extern "C" long r3d_clean_ws_words(int n_way, int k_shot) { return (long)n_way * k_shot * (AH_BOXES * AH_DMAX + AH_BOXES) + 64; }

// n_ep episodes at once: episode e's support features start feat_ep_rows rows after episode e - 1's, its coordinates /
// masks are entry e of (n_ep, S, Cin, N) / (n_ep, S, N) arrays, its scratch ws + e * ws_stride, its flags shot_keep + e * S
extern "C" int r3d_clean_shot_detect_batched(int n_ep, const float* feat, long ldf, long feat_ep_rows, int D,
                                             const float* support_x, int Cin, const int32_t* support_y, int n_way, int k_shot,
                                             int N, int32_t* shot_keep, float* dbg_cos_sum, int32_t* ws, long ws_stride,
                                             void* stream) {
  R3D_REQUIRE(feat && support_x && support_y && shot_keep && ws, "r3d_clean_shot_detect: null pointer");
  R3D_REQUIRE(n_way >= 1 && n_way * k_shot <= AH_MAXSHOT && k_shot <= AH_MAXK && D >= 1 && D <= AH_DMAX && Cin >= 3 && N >= 1,
              "r3d_clean_shot_detect: unsupported shape n_way=%d k_shot=%d D=%d", n_way, k_shot, D);
  R3D_REQUIRE(n_ep >= 1 && n_ep <= 65535 && (n_ep == 1 || ws_stride >= r3d_clean_ws_words(n_way, k_shot)),
              "r3d_clean_shot_detect: %d episodes, scratch stride %ld", n_ep, ws_stride);
  const int S = n_way * k_shot;
  float* box_sum = (float*)ws;
  int* box_cnt = ws + (long)S * AH_BOXES * AH_DMAX;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(r3d_clean_boxsum_kernel, dim3(S, AH_BOXES, n_ep), dim3(256), 0, st, feat, ldf, D, support_x, Cin,
                     support_y, N, box_sum, box_cnt, feat_ep_rows, ws_stride);
  hipLaunchKernelGGL(r3d_clean_decide_kernel, dim3(n_way, n_ep), dim3(256), 0, st, box_sum, box_cnt, n_way, k_shot, D,
                     shot_keep, dbg_cos_sum, ws_stride);
  R3D_LAUNCH_CHECK("r3d_clean_shot_detect");
  return R3D_OK;
}

// Z (n_q*N, 4) fp32 similarity rows (feed r3d_query_logits_ce_batched with n_proto = 0); more than 3 ways: two planes
// (2, n_q*N, 4), classes 4..7 in plane 1 (r3d_query_logits_ce_batched with z_ep_rows = n_q*N).  ws: S*2*256 floats.
extern "C" int r3d_protonet_head(const float* sfeat, long ldf, const float* qfeat, long ldq, int D,
                                 const int32_t* support_y, int n_way, int k_shot, int N, int n_query_pts, int method,
                                 float scaler, float* Z, float* ws, void* stream) {
  R3D_REQUIRE(sfeat && qfeat && support_y && Z && ws, "r3d_protonet_head: null pointer");
  R3D_REQUIRE(n_way >= 1 && n_way <= 7 && D >= 1 && D <= AH_DMAX, "r3d_protonet_head: unsupported shape");
  if (method != 0 && method != 1) {
    // the reference raises NotImplementedError for anything but cosine / euclidean (protonet.py:347)
    r3d_set_error("Error! Distance computation method (%d) is unknown!", method);
    return R3D_ERR_UNSUPPORTED;
  }
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(r3d_proto_pool_kernel, dim3(n_way * k_shot), dim3(256), 0, st, sfeat, ldf, D, support_y, N, ws);
  hipLaunchKernelGGL(r3d_proto_sim_kernel, dim3(256), dim3(256), 0, st, ws, n_way, k_shot, qfeat, ldq, D, n_query_pts,
                     method, scaler, (float4*)Z, n_way > 3 ? (float4*)Z + n_query_pts : nullptr);
  R3D_LAUNCH_CHECK("r3d_protonet_head");
  return R3D_OK;
}

// The evaluation head for n_ep episodes in ONE launch pair: per episode bit for bit what r3d_protonet_head gives for it alone
// (the pooled sums walk a shot's rows in the same order; a query point's arithmetic is the same function).  sfeat / qfeat:
// episode 0's support / query rows inside one feature matrix, episode e feat_ep_rows rows further on; support_y (n_ep, S, N);
// Z (n_ep * n_query_pts, 4) per plane, plane 1 (classes 4..7) n_ep * n_query_pts rows further on when n_way > 3.
extern "C" long r3d_protonet_head_ws_words(int n_ep, int n_way, int k_shot) {
  if (n_ep < 1 || n_ep > 65535 || n_way < 1 || n_way > 7 || k_shot < 1 || (long)n_way * k_shot > 65535) return -1;
  return (long)n_ep * n_way * k_shot * 2 * AH_DMAX;
}
// shot_keep (n_ep, n_way*k_shot) int32 on the device, 0 = the shot's foreground is left out of its way's prototype
// (r3d_clean_shot_detect_batched writes it); null: every shot is kept, which is r3d_protonet_head_batched bit for bit, as is
// a vector of ones.  The workgroups that form the prototypes read it: no launch is added and the host never reads it, so a
// way without a kept shot (which the detection never leaves) is not reported -- its prototype and similarities are NaN.
static int ah_protonet_head_ep(const char* who, int n_ep, const float* sfeat, long ldf, const float* qfeat, long ldq,
                               long feat_ep_rows, int D, const int32_t* support_y, const int32_t* shot_keep, int n_way,
                               int k_shot, int N, int n_query_pts, int method, float scaler, float* Z, float* ws,
                               long ws_words, void* stream) {
  R3D_REQUIRE(sfeat && qfeat && support_y && Z && ws, "%s: null pointer", who);
  R3D_REQUIRE(n_way >= 1 && n_way <= 7 && D >= 1 && D <= AH_DMAX && k_shot >= 1 && (long)n_way * k_shot <= 65535 && N >= 1 &&
                  n_query_pts >= 1 && ldf >= D && ldq >= D,
              "%s: unsupported shape n_way=%d k_shot=%d N=%d D=%d", who, n_way, k_shot, N, D);
  if (method != 0 && method != 1) {
    // the reference raises NotImplementedError for anything but cosine / euclidean (protonet.py:347)
    r3d_set_error("Error! Distance computation method (%d) is unknown!", method);
    return R3D_ERR_UNSUPPORTED;
  }
  const int S = n_way * k_shot;
  R3D_REQUIRE(n_ep >= 1 && n_ep <= 65535 && (n_ep == 1 || feat_ep_rows >= (long)S * N),
              "%s: %d episodes, %ld rows between them", who, n_ep, feat_ep_rows);
  const long need = r3d_protonet_head_ws_words(n_ep, n_way, k_shot);
  R3D_REQUIRE(ws_words >= need, "%s: workspace of %ld words is shorter than r3d_protonet_head_ws_words = %ld",
              who, ws_words, need);
  R3D_REQUIRE(((uintptr_t)ws & 15) == 0 && ((uintptr_t)Z & 15) == 0, "%s: ws and Z must be 16-byte aligned", who);
  R3D_REQUIRE(((uintptr_t)shot_keep & 3) == 0, "%s: shot_keep must be 4-byte aligned", who);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(r3d_proto_pool_ep_kernel, dim3(S, n_ep), dim3(256), 0, st, sfeat, ldf, feat_ep_rows, D, support_y, N, ws);
  // ~2048 workgroups over the batch (8 per CU), 256 for one episode as r3d_protonet_head: every workgroup builds the
  // prototypes of its episode again, so few episodes get many tiles and many episodes few
  const int gx = min(r3d_cdiv(n_query_pts, 4), max(32, min(256, 2048 / n_ep)));
  hipLaunchKernelGGL(r3d_proto_sim_ep_kernel, dim3(gx, n_ep), dim3(256), 0, st, ws, shot_keep, n_way, k_shot, qfeat, ldq,
                     feat_ep_rows, D, n_query_pts, method, scaler, (float4*)Z,
                     n_way > 3 ? (float4*)Z + (long)n_ep * n_query_pts : nullptr);
  R3D_LAUNCH_CHECK(who);
  return R3D_OK;
}
extern "C" int r3d_protonet_head_keep_batched(int n_ep, const float* sfeat, long ldf, const float* qfeat, long ldq,
                                              long feat_ep_rows, int D, const int32_t* support_y, const int32_t* shot_keep,
                                              int n_way, int k_shot, int N, int n_query_pts, int method, float scaler, float* Z,
                                              float* ws, long ws_words, void* stream) {
  return ah_protonet_head_ep("r3d_protonet_head_keep_batched", n_ep, sfeat, ldf, qfeat, ldq, feat_ep_rows, D, support_y,
                             shot_keep, n_way, k_shot, N, n_query_pts, method, scaler, Z, ws, ws_words, stream);
}
extern "C" int r3d_protonet_head_batched(int n_ep, const float* sfeat, long ldf, const float* qfeat, long ldq, long feat_ep_rows,
                                         int D, const int32_t* support_y, int n_way, int k_shot, int N, int n_query_pts,
                                         int method, float scaler, float* Z, float* ws, long ws_words, void* stream) {
  return ah_protonet_head_ep("r3d_protonet_head_batched", n_ep, sfeat, ldf, qfeat, ldq, feat_ep_rows, D, support_y, nullptr,
                             n_way, k_shot, N, n_query_pts, method, scaler, Z, ws, ws_words, stream);
}

// The head's halves as calls of their own (include/r3d.h): the prototype table of n_ep support sets, and the similarity
// rows of n_sys query groups against a table.  The table kernel reads pooled means only; the similarity kernel reads the
// table and the query rows it is given.
extern "C" int r3d_protonet_prototypes_batched(int n_ep, const float* sfeat, long ldf, long feat_ep_rows, int D,
                                               const int32_t* support_y, const int32_t* shot_keep, int n_way, int k_shot, int N,
                                               float* protos, float* ws, long ws_words, void* stream) {
  const char* who = "r3d_protonet_prototypes_batched";
  R3D_REQUIRE(sfeat && support_y && protos && ws, "%s: null pointer", who);
  R3D_REQUIRE(n_way >= 1 && n_way <= 7 && D >= 1 && D <= AH_DMAX && k_shot >= 1 && (long)n_way * k_shot <= 65535 && N >= 1 &&
                  ldf >= D,
              "%s: unsupported shape n_way=%d k_shot=%d N=%d D=%d", who, n_way, k_shot, N, D);
  const int S = n_way * k_shot;
  R3D_REQUIRE(n_ep >= 1 && n_ep <= 65535 && (n_ep == 1 || feat_ep_rows >= (long)S * N),
              "%s: %d episodes, %ld rows between them", who, n_ep, feat_ep_rows);
  const long need = r3d_protonet_head_ws_words(n_ep, n_way, k_shot);
  R3D_REQUIRE(ws_words >= need, "%s: workspace of %ld words is shorter than r3d_protonet_head_ws_words = %ld", who, ws_words,
              need);
  R3D_REQUIRE(((uintptr_t)ws & 15) == 0 && ((uintptr_t)shot_keep & 3) == 0, "%s: ws must be 16-byte, shot_keep 4-byte aligned",
              who);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(r3d_proto_pool_ep_kernel, dim3(S, n_ep), dim3(256), 0, st, sfeat, ldf, feat_ep_rows, D, support_y, N, ws);
  hipLaunchKernelGGL(r3d_proto_table_kernel, dim3(n_ep), dim3(256), 0, st, ws, shot_keep, n_way, k_shot, D, protos);
  R3D_LAUNCH_CHECK(who);
  return R3D_OK;
}
extern "C" int r3d_protonet_similarity_batched(int n_sys, const float* qfeat, long ldq, long q_sys_rows, int D,
                                               const float* protos, long proto_stride, int n_way, int n_query_pts, int method,
                                               float scaler, float* Z, void* stream) {
  const char* who = "r3d_protonet_similarity_batched";
  R3D_REQUIRE(qfeat && protos && Z, "%s: null pointer", who);
  R3D_REQUIRE(n_way >= 1 && n_way <= 7 && D >= 1 && D <= AH_DMAX && n_query_pts >= 1 && ldq >= D,
              "%s: unsupported shape n_way=%d n_query_pts=%d D=%d", who, n_way, n_query_pts, D);
  if (method != 0 && method != 1) {
    // the reference raises NotImplementedError for anything but cosine / euclidean (protonet.py:347)
    r3d_set_error("Error! Distance computation method (%d) is unknown!", method);
    return R3D_ERR_UNSUPPORTED;
  }
  R3D_REQUIRE(n_sys >= 1 && n_sys <= 65535 && (n_sys == 1 || q_sys_rows >= n_query_pts),
              "%s: %d systems, %ld rows between them", who, n_sys, q_sys_rows);
  R3D_REQUIRE(proto_stride == 0 || proto_stride >= (long)(n_way + 1) * D,
              "%s: prototype stride %ld (0 = one table for every system, else >= (n_way + 1) * D = %ld)", who, proto_stride,
              (long)(n_way + 1) * D);
  R3D_REQUIRE(((uintptr_t)Z & 15) == 0, "%s: Z must be 16-byte aligned", who);
  // the tiling of ah_protonet_head_ep (a point's arithmetic does not depend on the grid)
  const int gx = min(r3d_cdiv(n_query_pts, 4), max(32, min(256, 2048 / n_sys)));
  hipLaunchKernelGGL(r3d_proto_sim_table_kernel, dim3(gx, n_sys), dim3(256), 0, (hipStream_t)stream, protos, proto_stride, n_way,
                     qfeat, ldq, q_sys_rows, D, n_query_pts, method, scaler, (float4*)Z,
                     n_way > 3 ? (float4*)Z + (long)n_sys * n_query_pts : nullptr);
  R3D_LAUNCH_CHECK(who);
  return R3D_OK;
}

extern "C" int r3d_protonet_similarity_sets(int n_groups, int n_sets, const float* qfeat, long ldq, long q_sys_rows, int D,
                                            const float* protos, long proto_stride, int n_way, int n_query_pts, int method,
                                            float scaler, float* Z, void* stream) {
  const char* who = "r3d_protonet_similarity_sets";
  R3D_REQUIRE(qfeat && protos && Z, "%s: null pointer", who);
  R3D_REQUIRE(n_way >= 1 && n_way <= 7 && D >= 1 && D <= AH_DMAX && n_query_pts >= 1 && ldq >= D,
              "%s: unsupported shape n_way=%d n_query_pts=%d D=%d", who, n_way, n_query_pts, D);
  if (method != 0 && method != 1) {
    r3d_set_error("Error! Distance computation method (%d) is unknown!", method);
    return R3D_ERR_UNSUPPORTED;
  }
  R3D_REQUIRE(n_sets >= 1 && n_sets * (n_way + 1) <= 64, "%s: %d sets of %d classes (at most 64 prototype rows)", who, n_sets,
              n_way + 1);
  R3D_REQUIRE(n_groups >= 1 && n_groups <= 65535 && (n_groups == 1 || q_sys_rows >= n_query_pts) &&
                  (long)n_groups * n_sets * n_query_pts < 0x7fffffffL,
              "%s: %d groups x %d sets, %ld rows between the groups", who, n_groups, n_sets, q_sys_rows);
  R3D_REQUIRE(n_sets == 1 || proto_stride >= (long)(n_way + 1) * D, "%s: prototype stride %ld (>= (n_way + 1) * D = %ld)", who,
              proto_stride, (long)(n_way + 1) * D);
  R3D_REQUIRE(((uintptr_t)Z & 15) == 0, "%s: Z must be 16-byte aligned", who);
  const int R = n_sets * (n_way + 1);
  const size_t lds = sizeof(float) * ((size_t)R * (D | 1) + R);
  R3D_REQUIRE(r3d_kernel_lds((const void*)r3d_proto_sim_sets_kernel, lds) == 0, "%s: cannot reserve %zu B of LDS", who, lds);
  // the tiling of r3d_protonet_similarity_batched over the groups (a point's arithmetic does not depend on the grid)
  const int gx = min(r3d_cdiv(n_query_pts, 4), max(32, min(256, 2048 / n_groups)));
  const long plane = (long)n_groups * n_sets * n_query_pts;
  hipLaunchKernelGGL(r3d_proto_sim_sets_kernel, dim3(gx, n_groups), dim3(256), lds, (hipStream_t)stream, protos, proto_stride,
                     n_sets, n_way, qfeat, ldq, q_sys_rows, D, n_query_pts, method, scaler, (float4*)Z,
                     n_way > 3 ? (float4*)Z + plane : nullptr);
  R3D_LAUNCH_CHECK(who);
  return R3D_OK;
}

// correct (n_ep) int32: per episode the number of query points whose arg-max (pred (n_ep, n_pts) int32, as
// r3d_query_logits_ce_batched writes it) equals the label (n_ep, n_pts) int64
extern "C" int r3d_count_correct_batched(int n_ep, const int32_t* pred, const int64_t* labels, long n_pts, int32_t* correct,
                                         void* stream) {
  R3D_REQUIRE(pred && labels && correct, "r3d_count_correct_batched: null pointer");
  R3D_REQUIRE(n_ep >= 1 && n_pts >= 1 && n_pts < 0x7fffffffL, "r3d_count_correct_batched: %d episodes of %ld points", n_ep, n_pts);
  hipLaunchKernelGGL(r3d_count_correct_kernel, dim3(n_ep), dim3(256), 0, (hipStream_t)stream, pred, (const long long*)labels,
                     n_pts, correct);
  R3D_LAUNCH_CHECK("r3d_count_correct_batched");
  return R3D_OK;
}

extern "C" int r3d_miou_accumulate(const int32_t* pred, const int64_t* gt, long n, const int32_t* lut, int n_lut,
                                   int n_classes, uint64_t* hist, void* stream) {
  R3D_REQUIRE(pred && gt && lut && hist && n > 0 && n_lut > 0 && n_classes > 0, "r3d_miou_accumulate: bad arguments");
  hipLaunchKernelGGL(r3d_miou_accumulate_kernel, dim3(r3d_cdiv(n, 256)), dim3(256), 0, (hipStream_t)stream, pred,
                     (const long long*)gt, n, lut, n_lut, n_classes, (unsigned long long*)hist);
  R3D_LAUNCH_CHECK("r3d_miou_accumulate");
  return R3D_OK;
}
