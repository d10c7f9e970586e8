// What the scene features stand on (scene_common.h declares the launchers): the bounds of a scan, the stable radix sort of
// (key, scan index) pairs and the exclusive scan.  scene.hip sorts by cell, scene_segments.hip by segment id,
// scene_grow.hip by voxel; all of it is bandwidth-bound integer and min / max work without a floating-point sum.
#include "scene_common.h"

#define SC_PER_THREAD (SC_TILE / SC_THREADS)

// ------------------------------------------------------------------------------------------------ bounds
// Minima and maxima of the first AXES coordinates over the valid points, and their number: AXES = 2 for the labelling
// plan (r3d_scene_bounds), 3 for the voxel grid (r3d_scene_grow_bounds).  A partial is AXES minima, AXES maxima, the count.
template <int AXES>
__global__ __launch_bounds__(SC_THREADS) void r3d_scene_bounds_part_kernel(const float* __restrict__ scan, int ld, int M,
                                                                           float* __restrict__ part) {
  __shared__ float red[2 * AXES + 1][SC_THREADS / R3D_WAVE];
  float mn[AXES], mx[AXES];
#pragma unroll
  for (int a = 0; a < AXES; ++a) {
    mn[a] = INFINITY;
    mx[a] = -INFINITY;
  }
  int n = 0;
  for (int i = blockIdx.x * SC_THREADS + threadIdx.x; i < M; i += gridDim.x * SC_THREADS) {
    const float* p = scan + (long)i * ld;
    const float v[3] = {p[0], p[1], p[2]};
    if (sc_finite3(v[0], v[1], v[2])) {
#pragma unroll
      for (int a = 0; a < AXES; ++a) {
        mn[a] = fminf(mn[a], v[a]);
        mx[a] = fmaxf(mx[a], v[a]);
      }
      ++n;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int a = 0; a < AXES; ++a) {
      mn[a] = fminf(mn[a], __shfl_xor(mn[a], o));
      mx[a] = fmaxf(mx[a], __shfl_xor(mx[a], o));
    }
    n += __shfl_xor(n, o);
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int a = 0; a < AXES; ++a) {
      red[a][w] = mn[a];
      red[AXES + a][w] = mx[a];
    }
    red[2 * AXES][w] = __int_as_float(n);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < SC_THREADS / R3D_WAVE; ++k) {
#pragma unroll
      for (int a = 0; a < AXES; ++a) {
        mn[a] = fminf(mn[a], red[a][k]);
        mx[a] = fmaxf(mx[a], red[AXES + a][k]);
      }
      n += __float_as_int(red[2 * AXES][k]);
    }
    float* o = part + (2L * AXES + 1) * blockIdx.x;
#pragma unroll
    for (int a = 0; a < AXES; ++a) {
      o[a] = mn[a];
      o[AXES + a] = mx[a];
    }
    o[2 * AXES] = __int_as_float(n);
  }
}

// one wave: the partials -> words 0 .. 2 AXES of the record, in a partial's order; the other words of the record (8 for
// two axes, 16 for three) start at 0
template <int AXES>
__global__ __launch_bounds__(R3D_WAVE) void r3d_scene_bounds_final_kernel(const float* __restrict__ part, int n_part,
                                                                          float* __restrict__ rec) {
  float mn[AXES], mx[AXES];
#pragma unroll
  for (int a = 0; a < AXES; ++a) {
    mn[a] = INFINITY;
    mx[a] = -INFINITY;
  }
  int n = 0;
  for (int i = threadIdx.x; i < n_part; i += R3D_WAVE) {
    const float* p = part + (2L * AXES + 1) * i;
#pragma unroll
    for (int a = 0; a < AXES; ++a) {
      mn[a] = fminf(mn[a], p[a]);
      mx[a] = fmaxf(mx[a], p[AXES + a]);
    }
    n += __float_as_int(p[2 * AXES]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int a = 0; a < AXES; ++a) {
      mn[a] = fminf(mn[a], __shfl_xor(mn[a], o));
      mx[a] = fmaxf(mx[a], __shfl_xor(mx[a], o));
    }
    n += __shfl_xor(n, o);
  }
  if (threadIdx.x == 0) {
#pragma unroll
    for (int a = 0; a < AXES; ++a) {
      rec[a] = mn[a];
      rec[AXES + a] = mx[a];
    }
    rec[2 * AXES] = __int_as_float(n);
    for (int k = 2 * AXES + 1; k < (AXES == 2 ? 8 : 16); ++k) rec[k] = 0.0f;
  }
}

int sc_bounds_blocks(long M) {
  const int b = sc_grid_of(M);
  return b < SC_BOUNDS_BLOCKS ? b : SC_BOUNDS_BLOCKS;
}

void sc_bounds(const float* scan, int ld, long M, int axes, float* part, float* rec, hipStream_t st) {
  const int nb = sc_bounds_blocks(M);
  if (axes == 2) {
    hipLaunchKernelGGL(r3d_scene_bounds_part_kernel<2>, dim3(nb), dim3(SC_THREADS), 0, st, scan, ld, (int)M, part);
    hipLaunchKernelGGL(r3d_scene_bounds_final_kernel<2>, dim3(1), dim3(R3D_WAVE), 0, st, part, nb, rec);
  } else {
    hipLaunchKernelGGL(r3d_scene_bounds_part_kernel<3>, dim3(nb), dim3(SC_THREADS), 0, st, scan, ld, (int)M, part);
    hipLaunchKernelGGL(r3d_scene_bounds_final_kernel<3>, dim3(1), dim3(R3D_WAVE), 0, st, part, nb, rec);
  }
}

extern "C" long r3d_scene_bounds_ws_words(long M) { return M > 0 ? 5L * sc_bounds_blocks(M) : 0; }

// the record: x0, y0, xmax, ymax (floats), the valid points (int bits), three zeros
extern "C" int r3d_scene_bounds(const float* scan, int ld, long M, float* rec, float* ws, long ws_words, void* stream) {
  R3D_REQUIRE(scan && rec && ws, "r3d_scene_bounds: null pointer (scan %p, rec %p, ws %p)", (const void*)scan, (void*)rec,
              (void*)ws);
  SC_TRY(sc_check_points("r3d_scene_bounds", M));
  SC_TRY(sc_check_ld("r3d_scene_bounds", ld));
  SC_TRY(sc_check_ws("r3d_scene_bounds", ws_words, r3d_scene_bounds_ws_words(M)));
  sc_bounds(scan, ld, M, 2, ws, rec, (hipStream_t)stream);
  R3D_LAUNCH_CHECK("r3d_scene_bounds");
  return R3D_OK;
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

void sc_excl_scan(int* a, long n, int* part, hipStream_t st) {
  const int nb = sc_tiles_of(n);
  hipLaunchKernelGGL(r3d_scene_scan_sum_kernel, dim3(nb), dim3(SC_THREADS), 0, st, a, n, part);
  hipLaunchKernelGGL(r3d_scene_scan_part_kernel, dim3(1), dim3(SC_PLAN_THREADS), 0, st, part, nb);
  hipLaunchKernelGGL(r3d_scene_scan_local_kernel, dim3(nb), dim3(SC_THREADS), 0, st, a, n, part);
}

int sc_sort_pairs(int32_t* ws, const sc_sort_ws& W, long M, int passes, hipStream_t st) {
  for (int p = 0; p < passes; ++p) {
    const int a = p & 1, b = a ^ 1;
    hipLaunchKernelGGL(r3d_scene_hist_kernel, dim3(W.n_tiles), dim3(SC_THREADS), 0, st, ws + W.key[a], (int)M, 8 * p, W.n_tiles,
                       ws + W.hist);
    sc_excl_scan(ws + W.hist, 256L * W.n_tiles, ws + W.part, st);
    hipLaunchKernelGGL(r3d_scene_scatter_kernel, dim3(W.n_tiles), dim3(SC_THREADS), 0, st, ws + W.key[a], ws + W.idx[a], (int)M,
                       8 * p, W.n_tiles, ws + W.hist, ws + W.key[b], ws + W.idx[b]);
  }
  return passes & 1;
}
