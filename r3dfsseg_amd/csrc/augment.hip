// Training augmentation of prepared clouds on the device (reference: dataloaders/loader.py:205-213, 354-373).
//
// A prepared cloud holds the min-shifted xyz in channels xyz_ch .. xyz_ch + 2 -- the array the reference hands to
// augment_pointcloud -- so the transform below is that function on the same input, followed by the XYZ lines after it:
//   xyz' = xyz . M^T + jitter                 M = Mirror_y . Mirror_x . Rot_z(angle) . (s I)        loader.py:356-368
//   jitter = clip(0.01 normal, -0.05, 0.05)   on the three xyz channels                              loader.py:370-372
//   XYZ' = (xyz' - min_n xyz') / max_n (xyz' - min_n xyz')   per axis, IEEE division                 loader.py:209-213
// Every other channel is copied.
//
// Randomness is stateless (the manner of attn_keep in attention.hip): everything a cloud draws is a function of
// (seed + *seed_dev, cloud_key), the jitter of (point, axis) on top of that.  Nothing is stored between the two passes of
// the kernel: pass 2 evaluates the same hash and the same arithmetic again, which is what makes out == x safe.
#include "common.h"

#define AUG_THREADS 256
#define AUG_MAX_C 9

// draw `idx` of cloud stream `h` (h = r3d_stream(seed, key)): 32 mixed bits, r3d_draw of common.h
// [0, 1) in steps of 2^-24
static __device__ __forceinline__ float aug_uniform(unsigned h, unsigned idx) { return (float)(r3d_draw(h, idx) >> 8) * 0x1p-24f; }

// draws 0..3 of a stream make the matrix, draws 8 + 2 (3 point + axis) + {0, 1} the jitter of (point, axis)
#define AUG_DRAW_SCALE 0u
#define AUG_DRAW_ANGLE 1u
#define AUG_DRAW_MIRROR_X 2u
#define AUG_DRAW_MIRROR_Y 3u
#define AUG_DRAW_JITTER 8u

// clip(0.01 z, -0.05, 0.05), z standard normal by Box-Muller from two draws (|z| <= sqrt(48 ln 2) = 5.77: the clip acts)
static __device__ __forceinline__ float aug_jitter(unsigned h, unsigned point, unsigned axis) {
  const unsigned i = AUG_DRAW_JITTER + 2u * (3u * point + axis);
  const float u1 = (float)((r3d_draw(h, i) >> 8) + 1u) * 0x1p-24f;  // (0, 1]
  const float u2 = aug_uniform(h, i + 1u);
  const float z = sqrtf(-2.0f * logf(u1)) * cosf(6.28318530717958648f * u2);
  return fminf(fmaxf(0.01f * z, -0.05f), 0.05f);
}

struct aug_xyz {
  float v[3];
};

// xyz' of one point: the ONE place the arithmetic is written, so that both passes round alike
static __device__ __forceinline__ aug_xyz aug_point(const float* x, long sc, long sn, int xyz_ch, int n, const float* M, bool jitter,
                                                    unsigned h, const float* noise_b) {
  const float* p = x + (long)n * sn + (long)xyz_ch * sc;
  const float a = p[0], b = p[sc], c = p[2 * sc];
  aug_xyz r;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    float v = a * M[3 * i] + b * M[3 * i + 1] + c * M[3 * i + 2];
    if (noise_b) v += noise_b[3L * n + i];
    else if (jitter) v += aug_jitter(h, (unsigned)n, (unsigned)i);
    r.v[i] = v;
  }
  return r;
}

// one workgroup per cloud.  x and out are NOT __restrict__: out == x is allowed.
__global__ __launch_bounds__(AUG_THREADS) void r3d_augment_kernel(
    const float* x, long x_sb, long x_sc, long x_sn, float* out, long o_sb, long o_sc, long o_sn, int C, int N, int xyz_ch,
    int XYZ_ch, float scale, int rot, float mirror_prob, int jitter, unsigned seed, const unsigned* __restrict__ seed_dev,
    unsigned first_key, const float* __restrict__ mats, const float* __restrict__ noise, float* __restrict__ mats_out) {
  __shared__ float red[6][AUG_THREADS / R3D_WAVE];
  const int b = blockIdx.x, tid = threadIdx.x;
  if (seed_dev) seed += *seed_dev;  // per-replay seed of a frozen launch sequence lives in device memory
  const unsigned h = r3d_stream(seed, first_key + (unsigned)b);
  x += (long)b * x_sb;
  out += (long)b * o_sb;
  const float* noise_b = noise ? noise + (long)b * N * 3 : nullptr;

  float M[9];
  if (mats) {
#pragma unroll
    for (int i = 0; i < 9; ++i) M[i] = mats[9L * b + i];
  } else {
    float s = 1.0f, cs = 1.0f, sn = 0.0f, mx = 1.0f, my = 1.0f;
    if (scale > 1.0f) {
      const float lo = 1.0f / scale;
      s = fminf(lo + (scale - lo) * aug_uniform(h, AUG_DRAW_SCALE), scale);
    }
    if (rot == 1) {
      const float ang = 6.28318530717958648f * aug_uniform(h, AUG_DRAW_ANGLE);
      cs = cosf(ang);
      sn = sinf(ang);
    }
    if (mirror_prob > 0.0f) {
      if (aug_uniform(h, AUG_DRAW_MIRROR_X) < 0.5f * mirror_prob) mx = -1.0f;
      if (aug_uniform(h, AUG_DRAW_MIRROR_Y) < 0.5f * mirror_prob) my = -1.0f;
    }
    const bool r = rot == 1;
    M[0] = mx * (s * cs); M[1] = r ? mx * -(s * sn) : 0.0f; M[2] = 0.0f;
    M[3] = r ? my * (s * sn) : 0.0f; M[4] = my * (s * cs); M[5] = 0.0f;
    M[6] = 0.0f; M[7] = 0.0f; M[8] = s;
  }
  if (mats_out && tid == 0) {
#pragma unroll
    for (int i = 0; i < 9; ++i) mats_out[9L * b + i] = M[i];
  }

  // pass 1: the three minima and maxima of xyz' (min / max are order-independent: the same bits run to run)
  float lo[3], ext[3];
  if (XYZ_ch >= 0) {
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mxv[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int n = tid; n < N; n += AUG_THREADS) {
      const aug_xyz p = aug_point(x, x_sc, x_sn, xyz_ch, n, M, jitter != 0, h, noise_b);
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        mn[i] = fminf(mn[i], p.v[i]);
        mxv[i] = fmaxf(mxv[i], p.v[i]);
      }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        mn[i] = fminf(mn[i], __shfl_xor(mn[i], o));
        mxv[i] = fmaxf(mxv[i], __shfl_xor(mxv[i], o));
      }
      if ((tid & 63) == 0) {
        red[i][tid >> 6] = mn[i];
        red[3 + i][tid >> 6] = mxv[i];
      }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      float a = red[i][0], c = red[3 + i][0];
#pragma unroll
      for (int w = 1; w < AUG_THREADS / R3D_WAVE; ++w) {
        a = fminf(a, red[i][w]);
        c = fmaxf(c, red[3 + i][w]);
      }
      lo[i] = a;
      ext[i] = c - a;  // == max_n (xyz' - min): the subtraction is monotone
    }
  }
  // every read of pass 1 is done before any thread writes (out may be x)
  __syncthreads();

  // pass 2: each thread reads all channels of its point, then writes them
  for (int n = tid; n < N; n += AUG_THREADS) {
    float keep[AUG_MAX_C];
#pragma unroll
    for (int c = 0; c < AUG_MAX_C; ++c)
      if (c < C) keep[c] = x[(long)n * x_sn + (long)c * x_sc];
    const aug_xyz p = aug_point(x, x_sc, x_sn, xyz_ch, n, M, jitter != 0, h, noise_b);
#pragma unroll
    for (int c = 0; c < AUG_MAX_C; ++c) {
      if (c >= C) break;
      float v = keep[c];
      const int a = c - xyz_ch, A = c - XYZ_ch;
      if (a >= 0 && a < 3) v = a == 0 ? p.v[0] : a == 1 ? p.v[1] : p.v[2];
      if (XYZ_ch >= 0 && A >= 0 && A < 3) {
        const float q = A == 0 ? p.v[0] : A == 1 ? p.v[1] : p.v[2];
        const float l = A == 0 ? lo[0] : A == 1 ? lo[1] : lo[2];
        const float e = A == 0 ? ext[0] : A == 1 ? ext[1] : ext[2];
        v = (q - l) / e;
      }
      out[(long)n * o_sn + (long)c * o_sc] = v;
    }
  }
}

extern "C" int r3d_augment_clouds(const float* x, long x_sb, long x_sc, long x_sn, float* out, long o_sb, long o_sc, long o_sn,
                                  int B, int C, int N, int xyz_ch, int XYZ_ch, float scale, int rot, float mirror_prob,
                                  int jitter, unsigned seed, const unsigned* seed_dev, unsigned first_key, const float* mats,
                                  const float* noise, float* mats_out, void* stream) {
  R3D_REQUIRE(x && out, "r3d_augment_clouds: null pointer (x %p, out %p)", (const void*)x, (void*)out);
  R3D_REQUIRE(B > 0 && N > 0, "r3d_augment_clouds: B %d, N %d (both must be positive)", B, N);
  R3D_REQUIRE(N <= (1 << 28), "r3d_augment_clouds: N %d above 2^28 points per cloud", N);
  R3D_REQUIRE(C == 3 || C == 6 || C == 9, "r3d_augment_clouds: C %d (3, 6 or 9 channels)", C);
  R3D_REQUIRE(xyz_ch >= 0 && xyz_ch + 3 <= C, "r3d_augment_clouds: xyz_ch %d outside the %d channels", xyz_ch, C);
  R3D_REQUIRE(XYZ_ch == -1 || (XYZ_ch >= 0 && XYZ_ch + 3 <= C), "r3d_augment_clouds: XYZ_ch %d outside the %d channels (-1: none)",
              XYZ_ch, C);
  R3D_REQUIRE(XYZ_ch == -1 || XYZ_ch >= xyz_ch + 3 || xyz_ch >= XYZ_ch + 3,
              "r3d_augment_clouds: the xyz channels (%d..) and the XYZ channels (%d..) overlap", xyz_ch, XYZ_ch);
  R3D_REQUIRE(x_sb >= 0 && x_sc > 0 && x_sn > 0 && o_sb >= 0 && o_sc > 0 && o_sn > 0,
              "r3d_augment_clouds: strides must be positive (x %ld %ld %ld, out %ld %ld %ld)", x_sb, x_sc, x_sn, o_sb, o_sc, o_sn);
  R3D_REQUIRE(scale == scale && mirror_prob == mirror_prob, "r3d_augment_clouds: scale / mirror_prob is NaN");
  hipLaunchKernelGGL(r3d_augment_kernel, dim3(B), dim3(AUG_THREADS), 0, (hipStream_t)stream, x, x_sb, x_sc, x_sn, out, o_sb, o_sc,
                     o_sn, C, N, xyz_ch, XYZ_ch, scale, rot, mirror_prob, jitter, seed, seed_dev, first_key, mats, noise,
                     mats_out);
  R3D_LAUNCH_CHECK("r3d_augment_clouds");
  return R3D_OK;
}
