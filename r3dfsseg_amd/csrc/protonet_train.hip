// ProtoNet head in training mode, gfx950: forward that keeps what the backward needs, and the backward of masked average
// pooling + prototype averaging + cosine / euclidean similarity (reference: autograd through models/protonet.py:295-349).
//
//   fg_s = sum_p m_sp f_sp / (n_s + 1e-5)        bg_s = sum_p (1 - m_sp) f_sp / (N - n_s + 1e-5)        s = way * k_shot + k
//   P_0 = sum_s bg_s / (n_way k_shot)            P_{w+1} = sum_k fg_{w,k} / k_shot
//   cosine:    Z_pc = scaler <q_p, P_c> / max(|q_p| |P_c|, 1e-8)
//   euclidean: Z_pc = -sum_d (q_pd - P_cd + 1e-6)^2              (torch 1.8's pairwise_distance: norm(x1 - x2 + eps))
//
// Every reduction is deterministic: per-wave register partials over a point set fixed by the launch shape, waves combined
// in wave order through LDS, workgroups combined in block order by a second stage.  No floating-point atomics; every grid
// is a function of the problem shape alone.  The evaluation head (aux_heads.hip: r3d_protonet_head) is a separate path
// and is not touched: its pooling walks a cloud's rows serially, this one splits them over workgroups, so the pooled
// sums -- and with them Z -- differ from the evaluation head's in the last bits (the per-point arithmetic is the same).
#include "common.h"

#define PT_DMAX 256
#define PT_ROWS 128                   // support rows per pooling workgroup (32 per wave)
#define PT_QPTS 32                    // query points per backward workgroup (8 per wave)
#define PT_PART (2 * PT_DMAX + 4)     // one pooling partial: fg | bg | foreground count (int) + padding
#define PT_BPART (8 * PT_DMAX + 8)    // one backward partial: sum_p alpha_pc q_p per class | sum_p beta_pc per class

// scratch of ONE episode, in 32-bit words (every offset a multiple of 4)
struct PtWs {
  long part, pooled, cnt, proto, bpart, gvec, total;
  int NB, NBq;
};
static PtWs pt_carve(int n_way, int k_shot, int N, int n_pts) {
  PtWs L;
  const long S = (long)n_way * k_shot;
  L.NB = r3d_cdiv(N, PT_ROWS);
  L.NBq = r3d_cdiv(n_pts, PT_QPTS);
  L.part = 0;                                   // (S, NB, PT_PART)
  L.pooled = L.part + S * L.NB * PT_PART;       // (S, 2, 256): fg, bg means
  L.cnt = L.pooled + S * 2 * PT_DMAX;           // (S) int: foreground points per shot
  L.proto = L.cnt + (S + 3) / 4 * 4;            // (8, 256) prototypes | (8) their norms
  L.bpart = L.proto + 8 * PT_DMAX + 8;          // (NBq, PT_BPART)
  L.gvec = L.bpart + (long)L.NBq * PT_BPART;    // (S, 2, 256): gradient of a foreground / background row of shot s
  L.total = L.gvec + S * 2 * PT_DMAX;
  return L;
}

// ---------------------------------------------------------------------------
// forward 1: masked sums of PT_ROWS rows of one support cloud.  grid (NB, S, n_ep)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void r3d_ptn_pool_partial_kernel(const float* __restrict__ feat, long ldf, long feat_ep_rows,
                                                                   int D, const int* __restrict__ support_y, int N,
                                                                   float* __restrict__ ws, long ws_stride, PtWs L) {
  __shared__ float psum[4][2][PT_DMAX];
  __shared__ int pcnt[4];
  const int blk = blockIdx.x, shot = blockIdx.y, S = gridDim.y;
  const long ep = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const float* f = feat + (ep * feat_ep_rows + (long)shot * N) * ldf;
  const int* my = support_y + (ep * S + shot) * N;
  const int r1 = min(N, (blk + 1) * PT_ROWS);
  const int c0 = min(lane, D - 1), c1 = min(lane + 64, D - 1), c2 = min(lane + 128, D - 1), c3 = min(lane + 192, D - 1);
  float fg0 = 0.f, fg1 = 0.f, fg2 = 0.f, fg3 = 0.f, bg0 = 0.f, bg1 = 0.f, bg2 = 0.f, bg3 = 0.f;
  int nfg = 0;
#pragma unroll 4
  for (int p = blk * PT_ROWS + w; p < r1; p += 4) {  // a row is read coalesced across the lanes
    const float* fr = f + (long)p * ldf;
    const int m = my[p];
    const float wf = (float)m, wb = (float)(m == 0);  // (the evaluation head's weights)
    const float v0 = fr[c0], v1 = fr[c1], v2 = fr[c2], v3 = fr[c3];
    fg0 += v0 * wf; fg1 += v1 * wf; fg2 += v2 * wf; fg3 += v3 * wf;
    bg0 += v0 * wb; bg1 += v1 * wb; bg2 += v2 * wb; bg3 += v3 * wb;
    nfg += m;
  }
  psum[w][0][lane] = fg0; psum[w][0][lane + 64] = fg1; psum[w][0][lane + 128] = fg2; psum[w][0][lane + 192] = fg3;
  psum[w][1][lane] = bg0; psum[w][1][lane + 64] = bg1; psum[w][1][lane + 128] = bg2; psum[w][1][lane + 192] = bg3;
  if (lane == 0) pcnt[w] = nfg;
  __syncthreads();
  float* out = ws + ep * ws_stride + L.part + ((long)shot * L.NB + blk) * PT_PART;
  if (tid < D) {
    out[tid] = ((psum[0][0][tid] + psum[1][0][tid]) + psum[2][0][tid]) + psum[3][0][tid];
    out[PT_DMAX + tid] = ((psum[0][1][tid] + psum[1][1][tid]) + psum[2][1][tid]) + psum[3][1][tid];
  }
  if (tid == 0) ((int*)out)[2 * PT_DMAX] = pcnt[0] + pcnt[1] + pcnt[2] + pcnt[3];
}

// forward 2: the partials of a shot in block order -> getMaskedFeatures means and the shot's count.  grid (S, n_ep)
__global__ __launch_bounds__(256) void r3d_ptn_pool_combine_kernel(int D, int N, float* __restrict__ ws, long ws_stride, PtWs L) {
  const int shot = blockIdx.x, tid = threadIdx.x;
  float* e = ws + (long)blockIdx.y * ws_stride;
  const float* part = e + L.part + (long)shot * L.NB * PT_PART;
  int nfg = 0;
  for (int b = 0; b < L.NB; ++b) nfg += ((const int*)(part + (long)b * PT_PART))[2 * PT_DMAX];
  if (tid < D) {
    float fg = 0.f, bg = 0.f;
    for (int b = 0; b < L.NB; ++b) {
      fg += part[(long)b * PT_PART + tid];
      bg += part[(long)b * PT_PART + PT_DMAX + tid];
    }
    // getMaskedFeatures: sum(feat * mask) / (mask.sum() + 1e-5)
    e[L.pooled + ((long)shot * 2 + 0) * PT_DMAX + tid] = fg / ((float)nfg + 1e-5f);
    e[L.pooled + ((long)shot * 2 + 1) * PT_DMAX + tid] = bg / ((float)(N - nfg) + 1e-5f);
  }
  if (tid == 0) ((int*)(e + L.cnt))[shot] = nfg;
}

// forward 3: prototypes (getPrototype) + per-point similarity (calculateSimilarity) -> Z rows; the arithmetic of a point is
// r3d_proto_sim_kernel's, operation for operation.  Workgroup 0 of an episode leaves prototypes and norms in the scratch.
// grid (<= 256, n_ep)
__global__ __launch_bounds__(256) void r3d_ptn_sim_kernel(float* __restrict__ ws, long ws_stride, PtWs L, int n_way, int k_shot,
                                                          const float* __restrict__ qfeat, long ldq, long feat_ep_rows, int D,
                                                          int n_pts, int method /*0 cosine, 1 euclidean*/, float scaler,
                                                          float4* __restrict__ Zq, float4* __restrict__ Zq2 /* classes 4..7 */) {
  __shared__ float proto[8][PT_DMAX];
  __shared__ float pnorm[8];
  const long ep = blockIdx.y;
  float* e = ws + ep * ws_stride;
  const float* pooled = e + L.pooled;
  qfeat += ep * feat_ep_rows * ldq;
  Zq += ep * n_pts;
  if (Zq2) Zq2 += ep * n_pts;
  const int tid = threadIdx.x;
  const int n_classes = n_way + 1;
  if (tid < D) {
    float bgp = 0.f;
    for (int s = 0; s < n_way * k_shot; ++s) bgp += pooled[((long)s * 2 + 1) * PT_DMAX + tid];
    proto[0][tid] = bgp / (float)(n_way * k_shot);
    for (int wy = 0; wy < n_way; ++wy) {
      float f = 0.f;
      for (int k = 0; k < k_shot; ++k) f += pooled[((long)(wy * k_shot + k) * 2 + 0) * PT_DMAX + tid];
      proto[wy + 1][tid] = f / (float)k_shot;
    }
    for (int k = n_classes; k < 8; ++k) proto[k][tid] = 0.f;
  } else {
    for (int k = 0; k < 8; ++k) proto[k][tid] = 0.f;
  }
  __syncthreads();
  if (tid < 8) {
    float s = 0.f;
    if (tid < n_classes) for (int c = 0; c < D; ++c) s += proto[tid][c] * proto[tid][c];
    pnorm[tid] = sqrtf(s);
  }
  __syncthreads();
  if (blockIdx.x == 0) {
    for (int k = 0; k < 8; ++k) e[L.proto + k * PT_DMAX + tid] = proto[k][tid];
    if (tid < 8) e[L.proto + 8 * PT_DMAX + tid] = pnorm[tid];
  }
  const int lane = tid & 63, w = tid >> 6;
  for (int p = blockIdx.x * 4 + w; p < n_pts; p += gridDim.x * 4) {  // one wave per query point
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
      const float ee = r3d_wave_sum(dd[k]);
      if (method == 0) out[k] = d / fmaxf(sqrtf(qq) * pnorm[k], 1e-8f) * scaler;
      else { const float dist = sqrtf(ee); out[k] = -(dist * dist); }
      if (k >= n_classes) out[k] = 0.f;
    }
    if (lane == 0) Zq[p] = make_float4(out[0], out[1], out[2], out[3]);
    if (lane == 0 && Zq2) Zq2[p] = make_float4(out[4], out[5], out[6], out[7]);
  }
}

// ---------------------------------------------------------------------------
// backward 1: one wave per query point, PT_QPTS points per workgroup.  <q, P_c> and |q|^2 are computed again (cheaper than
// 8 more floats per point through memory).  Writes the point's dq row and adds its terms of dP to register partials:
//   cosine     Z = scaler d / den, den = |q||P_c| (> 1e-8):  dZ/dq = scaler (P_c / den - d q / (|q|^2 den)),
//                                                             dZ/dP_c = scaler (q / den - d P_c / (|P_c|^2 den));
//              den <= 1e-8 (zero prototype or zero row): Z = scaler d / 1e-8, dZ/dq = scaler P_c / 1e-8, dZ/dP_c = scaler q / 1e-8
//   euclidean  dZ/dq = -2 (q - P_c + 1e-6) = -dZ/dP_c
// partial of the workgroup: A_c = sum_p alpha_pc x_p (x = q, or q - P_c + 1e-6) and B_c = sum_p beta_pc (cosine: the factor
// of -P_c).  grid (NBq, n_ep)
// ---------------------------------------------------------------------------
template <int METHOD>
__global__ __launch_bounds__(256) void r3d_ptn_bwd_query_kernel(const float* __restrict__ qfeat, long ldq, long feat_ep_rows, int D,
                                                                int n_classes, int n_pts, float scaler,
                                                                const float4* __restrict__ G, const float4* __restrict__ G2,
                                                                float* __restrict__ dq, long lddq, long dfeat_ep_rows,
                                                                float* __restrict__ ws, long ws_stride, PtWs L) {
  __shared__ float proto[8][PT_DMAX];
  __shared__ float pnorm[8];
  __shared__ float accs[4][8][PT_DMAX];
  __shared__ float bsum[4][8];
  const long ep = blockIdx.y;
  float* e = ws + ep * ws_stride;
  qfeat += ep * feat_ep_rows * ldq;
  dq += ep * dfeat_ep_rows * lddq;
  G += ep * n_pts;
  if (G2) G2 += ep * n_pts;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  for (int k = 0; k < 8; ++k) proto[k][tid] = e[L.proto + k * PT_DMAX + tid];
  if (tid < 8) pnorm[tid] = e[L.proto + 8 * PT_DMAX + tid];
  __syncthreads();
  float acc[8][4], bacc[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    bacc[k] = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[k][j] = 0.f;
  }
  const int p0 = blockIdx.x * PT_QPTS + w * (PT_QPTS / 4);
  for (int i = 0; i < PT_QPTS / 4; ++i) {
    const int p = p0 + i;
    if (p >= n_pts) break;  // uniform over the wave
    const float* q = qfeat + (long)p * ldq;
    float qv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = lane + 64 * j;
      qv[j] = r3d_keep(q[min(c, D - 1)], c < D);
    }
    const float4 ga = G[p];
    const float4 gb = G2 ? G2[p] : make_float4(0.f, 0.f, 0.f, 0.f);
    const float g[8] = {ga.x, ga.y, ga.z, ga.w, gb.x, gb.y, gb.z, gb.w};
    float dqv[4] = {0.f, 0.f, 0.f, 0.f};
    if (METHOD == 0) {
      float qq = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) qq += qv[j] * qv[j];
      qq = r3d_wave_sum(qq);
      const float qn = sqrtf(qq);
      float bq = 0.f;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        if (k < n_classes) {
          float d = 0.f;
#pragma unroll
          for (int j = 0; j < 4; ++j) d += qv[j] * proto[k][lane + 64 * j];
          d = r3d_wave_sum(d);
          const float den = qn * pnorm[k];
          const float gs = g[k] * scaler;
          float al, bk = 0.f;
          if (den > 1e-8f) {
            al = gs / den;
            bq += gs * d / (qq * den);
            bk = gs * d / (pnorm[k] * pnorm[k] * den);
          } else {
            al = gs / 1e-8f;
          }
          bacc[k] += bk;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            dqv[j] += al * proto[k][lane + 64 * j];
            acc[k][j] += al * qv[j];
          }
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) dqv[j] -= qv[j] * bq;
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        if (k < n_classes) {
          const float wk = 2.f * g[k];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float x = (qv[j] - proto[k][lane + 64 * j]) + 1e-6f;
            dqv[j] -= wk * x;
            acc[k][j] += wk * x;
          }
        }
      }
    }
    float* dr = dq + (long)p * lddq;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (lane + 64 * j < D) dr[lane + 64 * j] = dqv[j];  // coalesced across the lanes
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) {
#pragma unroll
    for (int j = 0; j < 4; ++j) accs[w][k][lane + 64 * j] = acc[k][j];
    if (lane == 0) bsum[w][k] = bacc[k];
  }
  __syncthreads();
  float* out = e + L.bpart + (long)blockIdx.x * PT_BPART;
  for (int k = 0; k < 8; ++k) out[k * PT_DMAX + tid] = ((accs[0][k][tid] + accs[1][k][tid]) + accs[2][k][tid]) + accs[3][k][tid];
  if (tid < 8) out[8 * PT_DMAX + tid] = ((bsum[0][tid] + bsum[1][tid]) + bsum[2][tid]) + bsum[3][tid];
}

// backward 2: dP_c from the workgroup partials in block order, then through the prototype average and the masked mean:
//   d f_sp = m_sp dP_{w(s)+1} / (k_shot (n_s + 1e-5)) + (1 - m_sp) dP_0 / (n_way k_shot (N - n_s + 1e-5))
// i.e. one vector per shot for its foreground rows and one for its background rows.  grid (n_classes, n_ep)
__global__ __launch_bounds__(256) void r3d_ptn_bwd_proto_kernel(int D, int N, int n_way, int k_shot, int method,
                                                                float* __restrict__ ws, long ws_stride, PtWs L) {
  __shared__ float beta_s;
  const int c = blockIdx.x, tid = threadIdx.x;
  float* e = ws + (long)blockIdx.y * ws_stride;
  const float* bp = e + L.bpart;
  if (tid < 64) {  // lane l adds blocks l, l + 64, ... in order, then the fixed butterfly of r3d_wave_sum: one order per shape
    float b = 0.f;
    if (method == 0)
      for (int i = tid; i < L.NBq; i += 64) b += bp[(long)i * PT_BPART + 8 * PT_DMAX + c];
    b = r3d_wave_sum(b);
    if (tid == 0) beta_s = b;
  }
  __syncthreads();
  if (tid >= D) return;
  // four interleaved chains over the blocks (block i in chain i & 3), combined in chain order: loads of four blocks in flight
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  const float* col = bp + c * PT_DMAX + tid;
  int i = 0;
#pragma unroll 2
  for (; i + 4 <= L.NBq; i += 4) {
    a0 += col[(long)i * PT_BPART];
    a1 += col[(long)(i + 1) * PT_BPART];
    a2 += col[(long)(i + 2) * PT_BPART];
    a3 += col[(long)(i + 3) * PT_BPART];
  }
  if (i < L.NBq) a0 += col[(long)i * PT_BPART];
  if (i + 1 < L.NBq) a1 += col[(long)(i + 1) * PT_BPART];
  if (i + 2 < L.NBq) a2 += col[(long)(i + 2) * PT_BPART];
  const float a = ((a0 + a1) + a2) + a3;
  const float dP = method == 0 ? a - e[L.proto + c * PT_DMAX + tid] * beta_s : a;
  const int* cnt = (const int*)(e + L.cnt);
  float* gvec = e + L.gvec;
  const int S = n_way * k_shot;
  if (c == 0) {
    const float dbg = dP / (float)S;
    for (int s = 0; s < S; ++s) gvec[((long)s * 2 + 1) * PT_DMAX + tid] = dbg / ((float)(N - cnt[s]) + 1e-5f);
  } else {
    const float dfg = dP / (float)k_shot;
    for (int k = 0; k < k_shot; ++k) {
      const int s = (c - 1) * k_shot + k;
      gvec[((long)s * 2 + 0) * PT_DMAX + tid] = dfg / ((float)cnt[s] + 1e-5f);
    }
  }
}

// backward 3: every support row receives its shot's foreground or background vector: a broadcast write.  VEC: 16-byte stores
// (D, the leading dimension and the base address allow it); otherwise one column per lane.  grid (cdiv(N, 64), S, n_ep)
template <bool VEC>
__global__ __launch_bounds__(256) void r3d_ptn_bwd_bcast_kernel(const int* __restrict__ support_y, int N, int D,
                                                                float* __restrict__ dsfeat, long ldds, long dfeat_ep_rows,
                                                                const float* __restrict__ ws, long ws_stride, PtWs L) {
  const int shot = blockIdx.y, S = gridDim.y;
  const long ep = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const float* gv = ws + ep * ws_stride + L.gvec + (long)shot * 2 * PT_DMAX;
  const int* my = support_y + (ep * S + shot) * N;
  float* out = dsfeat + (ep * dfeat_ep_rows + (long)shot * N) * ldds;
  const int r1 = min(N, (int)(blockIdx.x + 1) * 64);
  if (VEC) {
    const int c = 4 * lane;
    if (c >= D) return;
    const float4 gf = *reinterpret_cast<const float4*>(gv + c);
    const float4 gb = *reinterpret_cast<const float4*>(gv + PT_DMAX + c);
#pragma unroll 4
    for (int p = blockIdx.x * 64 + w; p < r1; p += 4) {
      const int m = my[p];
      const float wf = (float)m;
      const float4 v = m == 0 ? gb : make_float4(wf * gf.x, wf * gf.y, wf * gf.z, wf * gf.w);
      *reinterpret_cast<float4*>(out + (long)p * ldds + c) = v;
    }
  } else {
    float gf[4], gb[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = min(lane + 64 * j, D - 1);
      gf[j] = gv[c];
      gb[j] = gv[PT_DMAX + c];
    }
    for (int p = blockIdx.x * 64 + w; p < r1; p += 4) {
      const int m = my[p];
      const float wf = (float)m;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (lane + 64 * j < D) out[(long)p * ldds + lane + 64 * j] = m == 0 ? gb[j] : wf * gf[j];
    }
  }
}

// ===========================================================================
// C ABI
// ===========================================================================
static long pt_ep_stride(const PtWs& L) { return L.total; }

extern "C" long r3d_protonet_head_train_ws_words(int n_ep, int n_way, int k_shot, int N, int n_query_pts, int D) {
  if (n_ep < 1 || n_way < 1 || n_way > 7 || k_shot < 1 || N < 1 || n_query_pts < 1 || D < 1 || D > PT_DMAX) return -1;
  return (long)n_ep * pt_ep_stride(pt_carve(n_way, k_shot, N, n_query_pts));
}

static int pt_check(const char* who, int n_ep, long feat_ep_rows, int D, int n_way, int k_shot, int N, int n_query_pts, int method,
                    const float* ws, long ws_words) {
  R3D_REQUIRE(n_way >= 1 && n_way <= 7 && D >= 1 && D <= PT_DMAX && k_shot >= 1 && N >= 1 && n_query_pts >= 1 &&
                  (long)n_way * k_shot <= 65535,
              "%s: unsupported shape n_way=%d k_shot=%d N=%d D=%d", who, n_way, k_shot, N, D);
  if (method != 0 && method != 1) {
    // the reference raises NotImplementedError for anything but cosine / euclidean (protonet.py:347)
    r3d_set_error("Error! Distance computation method (%d) is unknown!", method);
    return R3D_ERR_UNSUPPORTED;
  }
  R3D_REQUIRE(n_ep >= 1 && n_ep <= 65535 && (n_ep == 1 || feat_ep_rows >= (long)n_way * k_shot * N),
              "%s: %d episodes, %ld rows between them", who, n_ep, feat_ep_rows);
  const long need = r3d_protonet_head_train_ws_words(n_ep, n_way, k_shot, N, n_query_pts, D);
  R3D_REQUIRE(ws_words >= need, "%s: workspace of %ld words is shorter than r3d_protonet_head_train_ws_words = %ld", who,
              ws_words, need);
  R3D_REQUIRE(((uintptr_t)ws & 15) == 0, "%s: ws must be 16-byte aligned", who);
  return R3D_OK;
}

// Z: (n_ep * n_query_pts, 4), episode after episode; more than 3 ways: two planes (2, n_ep * n_query_pts, 4), classes 4..7 in
// plane 1 -- r3d_query_logits_ce_batched / r3d_ce_grad_batched with z_ep_rows = n_cap = n_query_pts read and write that.
extern "C" int r3d_protonet_head_train_fwd(int n_ep, const float* sfeat, long ldf, const float* qfeat, long ldq, long feat_ep_rows,
                                           int D, const int32_t* support_y, int n_way, int k_shot, int N, int n_query_pts,
                                           int method, float scaler, float* Z, float* ws, long ws_words, void* stream) {
  R3D_REQUIRE(sfeat && qfeat && support_y && Z && ws, "r3d_protonet_head_train_fwd: null pointer");
  const int rc = pt_check("r3d_protonet_head_train_fwd", n_ep, feat_ep_rows, D, n_way, k_shot, N, n_query_pts, method, ws, ws_words);
  if (rc) return rc;
  R3D_REQUIRE(ldf >= D && ldq >= D && ((uintptr_t)Z & 15) == 0, "r3d_protonet_head_train_fwd: ldf, ldq >= D; Z 16-byte aligned");
  const PtWs L = pt_carve(n_way, k_shot, N, n_query_pts);
  const long stride = pt_ep_stride(L);
  const int S = n_way * k_shot;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(r3d_ptn_pool_partial_kernel, dim3(L.NB, S, n_ep), dim3(256), 0, st, sfeat, ldf, feat_ep_rows, D, support_y, N,
                     ws, stride, L);
  hipLaunchKernelGGL(r3d_ptn_pool_combine_kernel, dim3(S, n_ep), dim3(256), 0, st, D, N, ws, stride, L);
  const int gx = min(256, r3d_cdiv(n_query_pts, 4));
  hipLaunchKernelGGL(r3d_ptn_sim_kernel, dim3(gx, n_ep), dim3(256), 0, st, ws, stride, L, n_way, k_shot, qfeat, ldq, feat_ep_rows,
                     D, n_query_pts, method, scaler, (float4*)Z, n_way > 3 ? (float4*)Z + (long)n_ep * n_query_pts : nullptr);
  R3D_LAUNCH_CHECK("r3d_protonet_head_train_fwd");
  return R3D_OK;
}

// dZ in the layout of Z; ws as r3d_protonet_head_train_fwd left it (same shape arguments).  Writes -- does not accumulate --
// dsfeat (S*N rows) and dqfeat (n_query_pts rows) of every episode; episode e's rows start e * dfeat_ep_rows rows further on
// in both (the layout of one gradient matrix over [support rows | query rows] per episode).
extern "C" int r3d_protonet_head_bwd(int n_ep, const float* qfeat, long ldq, long feat_ep_rows, int D, const int32_t* support_y,
                                     int n_way, int k_shot, int N, int n_query_pts, int method, float scaler, const float* dZ,
                                     float* dsfeat, long ldds, float* dqfeat, long lddq, long dfeat_ep_rows, float* ws,
                                     long ws_words, void* stream) {
  R3D_REQUIRE(qfeat && support_y && dZ && dsfeat && dqfeat && ws, "r3d_protonet_head_bwd: null pointer");
  const int rc = pt_check("r3d_protonet_head_bwd", n_ep, feat_ep_rows, D, n_way, k_shot, N, n_query_pts, method, ws, ws_words);
  if (rc) return rc;
  R3D_REQUIRE(ldq >= D && ldds >= D && lddq >= D && ((uintptr_t)dZ & 15) == 0 &&
                  (n_ep == 1 || dfeat_ep_rows >= (long)n_way * k_shot * N),
              "r3d_protonet_head_bwd: leading dimensions >= D; dZ 16-byte aligned; dfeat_ep_rows >= S*N");
  const PtWs L = pt_carve(n_way, k_shot, N, n_query_pts);
  const long stride = pt_ep_stride(L);
  const int S = n_way * k_shot, n_classes = n_way + 1;
  hipStream_t st = (hipStream_t)stream;
  const float4* G = (const float4*)dZ;
  const float4* G2 = n_way > 3 ? G + (long)n_ep * n_query_pts : nullptr;
  if (method == 0)
    hipLaunchKernelGGL(r3d_ptn_bwd_query_kernel<0>, dim3(L.NBq, n_ep), dim3(256), 0, st, qfeat, ldq, feat_ep_rows, D, n_classes,
                       n_query_pts, scaler, G, G2, dqfeat, lddq, dfeat_ep_rows, ws, stride, L);
  else
    hipLaunchKernelGGL(r3d_ptn_bwd_query_kernel<1>, dim3(L.NBq, n_ep), dim3(256), 0, st, qfeat, ldq, feat_ep_rows, D, n_classes,
                       n_query_pts, scaler, G, G2, dqfeat, lddq, dfeat_ep_rows, ws, stride, L);
  hipLaunchKernelGGL(r3d_ptn_bwd_proto_kernel, dim3(n_classes, n_ep), dim3(256), 0, st, D, N, n_way, k_shot, method, ws, stride, L);
  const bool vec = (D & 3) == 0 && (ldds & 3) == 0 && ((uintptr_t)dsfeat & 15) == 0;
  const dim3 grid(r3d_cdiv(N, 64), S, n_ep);
  if (vec)
    hipLaunchKernelGGL(r3d_ptn_bwd_bcast_kernel<true>, grid, dim3(256), 0, st, support_y, N, D, dsfeat, ldds, dfeat_ep_rows, ws,
                       stride, L);
  else
    hipLaunchKernelGGL(r3d_ptn_bwd_bcast_kernel<false>, grid, dim3(256), 0, st, support_y, N, D, dsfeat, ldds, dfeat_ep_rows, ws,
                       stride, L);
  R3D_LAUNCH_CHECK("r3d_protonet_head_bwd");
  return R3D_OK;
}
