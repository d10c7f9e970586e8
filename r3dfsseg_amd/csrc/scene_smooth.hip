// Scores propagated over the voxel graph: the device side of scene_smooth.py.
// smooth_scene ("Smoothing a labelled scan", S1-S7): the voted logits of a labelled scan are pooled per
// occupied voxel, swept over the voxel adjacency graph (Jacobi sweeps of label propagation, a voxel without evidence is
// filled from its neighbours ring by ring) and spread back to the points.  The grid, the sort and the voxel table are those
// of build_segments (r3d_scene_grow_bounds / _sort / _voxels and their workspace, as they are); here:
//   evidence   Y[v] = the mean of the mean logits of voxel v's contributors (valid, votes > 0), summed as the segment pool
//              sums a segment: ascending scan index, tiles of 256 contributor ranks, parts in tile order, one division;
//              members[v]; ring[v] = 0 with a member, else -1
//   graph      per voxel the rows of its occupied (and, with voxel_mean, like-coloured) neighbours among the 6 or 26 cells
//              around it, in ascending key order, packed to the front of 26 slots, -1 behind them: the binary searches of
//              gr_around are paid once, not once per sweep
//   sweep      one launch per sweep t -> t + 1, queued back to back; lanes run over (voxel, column), the column fastest
//   spread     the arg-max of every reached voxel, then per scan point its voxel's row or its own -> the counts (one read)
// Floats are added by __fadd_rn in the stated order, multiplied by __fmul_rn and divided by __fdiv_rn; none goes through an
// atomic.  Counts are integer atomics, one per workgroup and word.
#include "scene_components.h"

#define SM_CHUNK 9        // slots whose loads a lane of the sweep has in flight together
static_assert(R3D_SMOOTH_R_NUNLAB < R3D_SCENE_SMOOTH_COUNTS, "a word beyond the counts");

static int sm_check(const char* name, long M, long n_voxels, int n_cols, const int32_t* ws, long ws_words) {
  R3D_REQUIRE(ws, "%s: null pointer (ws)", name);
  SC_TRY(sc_check_points(name, M));
  SC_TRY(sc_check_ws(name, ws_words, gr_make_layout(M).total));
  SC_TRY(gr_check_rows(name, M, n_voxels, "voxels"));
  R3D_REQUIRE(n_cols >= 1 && n_cols <= R3D_SCENE_SCORE_COLS_MAX, "%s: %d score columns (1 .. 64)", name, n_cols);
  return R3D_OK;
}

// one thread per element of a (rows, C) table
static inline int sm_grid_of(long rows, int C) { return (int)((rows * C + SC_THREADS - 1) / SC_THREADS); }

// ---- evidence (S2).  One thread per (voxel, column): the C lanes of a voxel walk its points in sorted order together (the
// sort is stable: ascending scan index), so a point's row is one contiguous read and its votes one broadcast.
__global__ __launch_bounds__(SC_THREADS) void r3d_scene_smooth_evidence_kernel(int V, int C, int M, const float* __restrict__ scores,
                                                                               const int* __restrict__ votes,
                                                                               const int* __restrict__ order,
                                                                               const int* __restrict__ vstart,
                                                                               float* __restrict__ evidence, int* __restrict__ members,
                                                                               int* __restrict__ ring) {
  const long e = (long)blockIdx.x * SC_THREADS + threadIdx.x;
  if (e >= (long)V * C) return;
  const int v = (int)(e / C), j = (int)(e - (long)v * C);
  const int a = sc_clamp(vstart[v], 0, M), b = sc_clamp(vstart[v + 1], a, M);
  float tot = 0.0f, part = 0.0f;
  int n = 0;  // contributors so far: the rank of the next one
  for (int i = a; i < b; ++i) {
    const int p = sc_clamp(order[i], 0, M - 1);
    const int w = votes[p];
    if (w <= 0) continue;
    const float c = __fdiv_rn(scores[(long)p * C + j], (float)w);
    if (n % R3D_SCENE_SEG_TILE == 0) {  // a tile opens: the one before joins the total
      if (n > 0) tot = n == R3D_SCENE_SEG_TILE ? part : __fadd_rn(tot, part);
      part = c;
    } else {
      part = __fadd_rn(part, c);
    }
    ++n;
  }
  if (n > 0) tot = n <= R3D_SCENE_SEG_TILE ? part : __fadd_rn(tot, part);
  evidence[e] = n > 0 ? __fdiv_rn(tot, (float)n) : 0.0f;
  if (j == 0) {
    members[v] = n;
    ring[v] = n > 0 ? 0 : -1;
  }
}

extern "C" int r3d_scene_smooth_evidence(long M, int nx, int ny, int nz, int n_cols, const float* scores, const int32_t* votes,
                                         long n_voxels, float* voxel_evidence, int32_t* voxel_members, int32_t* voxel_ring,
                                         const int32_t* ws, long ws_words, void* stream) {
  R3D_REQUIRE(scores && votes && voxel_evidence && voxel_members && voxel_ring,
              "r3d_scene_smooth_evidence: null pointer (scores %p, votes %p, voxel_evidence %p, voxel_members %p, voxel_ring %p)",
              (const void*)scores, (const void*)votes, (void*)voxel_evidence, (void*)voxel_members, (void*)voxel_ring);
  SC_TRY(gr_check_grid("r3d_scene_smooth_evidence", M, nx, ny, nz, "voxels", ws));
  SC_TRY(sm_check("r3d_scene_smooth_evidence", M, n_voxels, n_cols, ws, ws_words));
  const gr_view w = gr_make_view(M, (long)nx * ny * nz, ws);
  hipLaunchKernelGGL(r3d_scene_smooth_evidence_kernel, dim3(sm_grid_of(n_voxels, n_cols)), dim3(SC_THREADS), 0, (hipStream_t)stream,
                     (int)n_voxels, n_cols, (int)M, scores, votes, w.order, ws + w.L.vstart, voxel_evidence, voxel_members,
                     voxel_ring);
  R3D_LAUNCH_CHECK("r3d_scene_smooth_evidence");
  return R3D_OK;
}

// ---- graph (S3).  One thread per voxel; gr_around delivers the occupied cells around it in ascending key order.  The
// table is slot-major, nbr[k * V + v], so that the lanes of a sweep, which hold consecutive voxels, read consecutive words.
__global__ __launch_bounds__(SC_THREADS) void r3d_scene_smooth_graph_kernel(int V, int nx, int ny, int nz, int conn,
                                                                            const int* __restrict__ vkey, int use_colour, float tol,
                                                                            const float* __restrict__ mean, int* __restrict__ nbr) {
  const int v = blockIdx.x * SC_THREADS + threadIdx.x;
  if (v >= V) return;
  float mv[3] = {0.0f, 0.0f, 0.0f};
  if (use_colour) {
#pragma unroll
    for (int j = 0; j < 3; ++j) mv[j] = mean[3L * v + j];
  }
  int k = 0;
  gr_around(v, V, nx, ny, nz, vkey, [&](int dy, int dz) { return conn == 6 && dy != 0 && dz != 0; }, [&](int r, int d, int row) {
    const int off = (d != 1) + (r % 3 != 1) + (r / 3 != 1);  // axes on which the cell differs from v's
    if (off == 0 || (conn == 6 && off != 1)) return;
    if (use_colour) {  // G4's test: a NaN joins nothing
      bool alike = true;
#pragma unroll
      for (int j = 0; j < 3; ++j) alike = alike && fabsf(__fsub_rn(mv[j], mean[3L * row + j])) <= tol;
      if (!alike) return;
    }
    if (k < R3D_SCENE_SMOOTH_SLOTS) nbr[(long)k * V + v] = row;
    ++k;
  });
  for (; k < R3D_SCENE_SMOOTH_SLOTS; ++k) nbr[(long)k * V + v] = -1;
}

extern "C" int r3d_scene_smooth_graph(long M, int nx, int ny, int nz, long n_voxels, int connectivity, const float* voxel_mean,
                                      float colour_tol, int32_t* voxel_neighbours, const int32_t* ws, long ws_words, void* stream) {
  R3D_REQUIRE(voxel_neighbours, "r3d_scene_smooth_graph: null pointer (voxel_neighbours)");
  SC_TRY(gr_check_grid("r3d_scene_smooth_graph", M, nx, ny, nz, "voxels", ws));
  SC_TRY(sm_check("r3d_scene_smooth_graph", M, n_voxels, 1, ws, ws_words));
  SC_TRY(gr_check_connectivity("r3d_scene_smooth_graph", connectivity));
  const bool colour = voxel_mean != nullptr;
  R3D_REQUIRE(!colour || (colour_tol >= 0.0f && colour_tol < INFINITY), "r3d_scene_smooth_graph: colour_tol %g (finite, >= 0)",
              (double)colour_tol);
  const gr_layout L = gr_make_layout(M);
  hipLaunchKernelGGL(r3d_scene_smooth_graph_kernel, dim3(sc_grid_of(n_voxels)), dim3(SC_THREADS), 0, (hipStream_t)stream,
                     (int)n_voxels, nx, ny, nz, connectivity, ws + L.vkey, colour ? 1 : 0, colour_tol, voxel_mean, voxel_neighbours);
  R3D_LAUNCH_CHECK("r3d_scene_smooth_graph");
  return R3D_OK;
}

// ---- sweep (S4).  One thread per (voxel, column) of sweep t -> t + 1: it reads sweep t's Z (zin) and writes zout, another
// array.  ring[] is ONE array, written in place by the lane of column 0 of a voxel that is filled in this sweep: the store is
// one aligned word, so a reader in the same launch sees either the -1 from before or t + 1, and the live test 0 <= ring <= t
// fails on both -- the sweep relies on that, not on a second ring table, and the result does not depend on which of the two
// a reader saw.  A voxel has a member exactly when its ring is 0 (a filled one gets t + 1 >= 1), and the lanes of a voxel
// that see its ring as -1 or as t + 1 take the same path.  A lane loads SM_CHUNK neighbour rows, then their rings, then their
// values, each set together; the additions stay in slot order.
__global__ __launch_bounds__(SC_THREADS) void r3d_scene_smooth_sweep_kernel(int V, int C, int t, float a, float b,
                                                                            const float* __restrict__ evidence,
                                                                            const int* __restrict__ nbr, const float* __restrict__ zin,
                                                                            float* __restrict__ zout, int* ring) {
  const long e = (long)blockIdx.x * SC_THREADS + threadIdx.x;
  if (e >= (long)V * C) return;
  const int v = (int)(e / C), j = (int)(e - (long)v * C);
  float s = 0.0f;
  int n = 0;
  for (int k0 = 0; k0 < R3D_SCENE_SMOOTH_SLOTS; k0 += SM_CHUNK) {
    int u[SM_CHUNK], ru[SM_CHUNK];
    float val[SM_CHUNK];
#pragma unroll
    for (int i = 0; i < SM_CHUNK; ++i) {
      const int x = k0 + i < R3D_SCENE_SMOOTH_SLOTS ? nbr[(long)(k0 + i) * V + v] : -1;
      u[i] = x < V ? x : -1;
    }
    if (u[0] < 0) break;  // the slots are packed: none behind the first empty one
#pragma unroll
    for (int i = 0; i < SM_CHUNK; ++i) ru[i] = u[i] >= 0 ? ring[u[i]] : -1;
#pragma unroll
    for (int i = 0; i < SM_CHUNK; ++i) val[i] = ru[i] >= 0 && ru[i] <= t ? zin[(long)u[i] * C + j] : 0.0f;
#pragma unroll
    for (int i = 0; i < SM_CHUNK; ++i)
      if (ru[i] >= 0 && ru[i] <= t) {  // live at t
        s = n == 0 ? val[i] : __fadd_rn(s, val[i]);
        ++n;
      }
  }
  if (n == 0) {
    zout[e] = zin[e];
    return;
  }
  const float m = __fdiv_rn(s, (float)n);
  const int rv = ring[v];
  if (rv == 0) {
    zout[e] = __fadd_rn(__fmul_rn(b, evidence[e]), __fmul_rn(a, m));
  } else {
    zout[e] = m;
    if (j == 0 && rv < 0) ring[v] = t + 1;
  }
}

extern "C" int r3d_scene_smooth_sweep(long M, long n_voxels, int n_cols, int iterations, float alpha, const float* voxel_evidence,
                                      const int32_t* voxel_neighbours, float* z0, float* z1, int32_t* voxel_ring, void* stream) {
  R3D_REQUIRE(voxel_evidence && voxel_neighbours && voxel_ring,
              "r3d_scene_smooth_sweep: null pointer (voxel_evidence %p, voxel_neighbours %p, voxel_ring %p)",
              (const void*)voxel_evidence, (const void*)voxel_neighbours, (void*)voxel_ring);
  SC_TRY(sc_check_points("r3d_scene_smooth_sweep", M));
  SC_TRY(gr_check_rows("r3d_scene_smooth_sweep", M, n_voxels, "voxels"));
  R3D_REQUIRE(n_cols >= 1 && n_cols <= R3D_SCENE_SCORE_COLS_MAX, "r3d_scene_smooth_sweep: %d score columns (1 .. 64)", n_cols);
  R3D_REQUIRE(iterations >= 0 && iterations <= R3D_SCENE_SMOOTH_SWEEPS, "r3d_scene_smooth_sweep: %d sweeps (0 .. %d)", iterations,
              R3D_SCENE_SMOOTH_SWEEPS);
  R3D_REQUIRE(alpha >= 0.0f && alpha < 1.0f, "r3d_scene_smooth_sweep: alpha %g (0 <= alpha < 1)", (double)alpha);
  R3D_REQUIRE((iterations < 1 || z0) && (iterations < 2 || z1) && (!z0 || z0 != z1),
              "r3d_scene_smooth_sweep: %d sweeps need z0 %p and, from the second on, z1 %p, two arrays", iterations, (void*)z0,
              (void*)z1);
  const float b = 1.0f - alpha;
  float* z[2] = {z0, z1};
  for (int t = 0; t < iterations; ++t)  // sweep t reads Y (t = 0) or z[(t - 1) & 1] and writes z[t & 1]
    hipLaunchKernelGGL(r3d_scene_smooth_sweep_kernel, dim3(sm_grid_of(n_voxels, n_cols)), dim3(SC_THREADS), 0, (hipStream_t)stream,
                       (int)n_voxels, n_cols, t, alpha, b, voxel_evidence, voxel_neighbours, t == 0 ? voxel_evidence : z[(t - 1) & 1],
                       z[t & 1], voxel_ring);
  R3D_LAUNCH_CHECK("r3d_scene_smooth_sweep");
  return R3D_OK;
}

// ---- spread (S5, S6)
// One thread per voxel: the arg-max of a reached voxel's row, -1 for one never reached; the voxel counts.
__global__ __launch_bounds__(SC_THREADS) void r3d_scene_smooth_labels_kernel(int V, int C, const float* __restrict__ z,
                                                                             const int* __restrict__ ring,
                                                                             long long* __restrict__ voxel_labels, int* __restrict__ counts) {
  __shared__ int red[SC_WAVES];
  const int v = blockIdx.x * SC_THREADS + threadIdx.x;
  int rv = -1;
  if (v < V) {
    rv = ring[v];
    int best = -1;
    float best_v = 0.0f;
    if (rv >= 0)
      for (int j = 0; j < C; ++j) sc_argmax_step(j, z[(long)v * C + j], best, best_v);
    voxel_labels[v] = best;
  }
  const int n_member = sc_block_count(rv == 0 ? 1 : 0, red), n_filled = sc_block_count(rv > 0 ? 1 : 0, red);
  if (threadIdx.x == 0) {  // integer counts: order-independent
    if (n_member > 0) atomicAdd(&counts[R3D_SMOOTH_R_MEMBER_VOXELS], n_member);
    if (n_filled > 0) atomicAdd(&counts[R3D_SMOOTH_R_FILLED_VOXELS], n_filled);
  }
}

// 256 scan points per round of a workgroup, as r3d_scene_seg_spread does it: one thread per point decides and leaves the voxel
// row its scores come from in LDS, then the workgroup copies the 256 rows with consecutive lanes on consecutive floats.
__global__ __launch_bounds__(SC_THREADS) void r3d_scene_smooth_spread_kernel(
    int M, int C, int V, const int* __restrict__ voxel_index, const int* __restrict__ ring, const float* __restrict__ z,
    const long long* __restrict__ voxel_labels, const float* __restrict__ in_scores, const long long* __restrict__ in_labels,
    const int* __restrict__ in_votes, float* __restrict__ scores, long long* __restrict__ labels, int* __restrict__ votes,
    unsigned char* __restrict__ smoothed, int* __restrict__ counts) {
  __shared__ int src[SC_THREADS];  // the voxel row a point's scores come from, -1: its own row of res
  __shared__ int red[SC_WAVES];
  int n_sm = 0, n_ch = 0, n_fi = 0, n_un = 0;
  for (long base = (long)blockIdx.x * SC_THREADS; base < M; base += (long)gridDim.x * SC_THREADS) {  // (uniform)
    const long p = base + threadIdx.x;
    int from = -1;
    if (p < M) {
      const int v = voxel_index[p];
      const bool sm = v >= 0 && v < V && ring[v] >= 0;
      const long long was = in_labels[p];
      const long long lab = sm ? voxel_labels[v] : was;
      labels[p] = lab;
      votes[p] = sm ? 1 : in_votes[p];
      smoothed[p] = sm ? 1 : 0;
      from = sm ? v : -1;
      n_sm += sm;
      n_ch += sm && was >= 0 && lab != was;
      n_fi += sm && was == -1;
      n_un += lab == -1;
    }
    src[threadIdx.x] = from;
    __syncthreads();
    const long left = M - base;
    const int n_el = (int)(left < SC_THREADS ? left : SC_THREADS) * C;
    for (int e = threadIdx.x; e < n_el; e += SC_THREADS) {
      const int q = e / C, j = e - q * C, v = src[q];
      scores[base * C + e] = v >= 0 ? z[(long)v * C + j] : in_scores[base * C + e];
    }
    __syncthreads();
  }
  n_sm = sc_block_count(n_sm, red);
  n_ch = sc_block_count(n_ch, red);
  n_fi = sc_block_count(n_fi, red);
  n_un = sc_block_count(n_un, red);
  if (threadIdx.x == 0) {  // integer counts: order-independent
    if (n_sm > 0) atomicAdd(&counts[R3D_SMOOTH_R_NSMOOTHED], n_sm);
    if (n_ch > 0) atomicAdd(&counts[R3D_SMOOTH_R_NCHANGED], n_ch);
    if (n_fi > 0) atomicAdd(&counts[R3D_SMOOTH_R_NFILLED], n_fi);
    if (n_un > 0) atomicAdd(&counts[R3D_SMOOTH_R_NUNLAB], n_un);
  }
}

extern "C" int r3d_scene_smooth_spread(long M, int n_cols, long n_voxels, const int32_t* voxel_index, const int32_t* voxel_ring,
                                       const float* voxel_scores, const float* in_scores, const int64_t* in_labels,
                                       const int32_t* in_votes, int64_t* voxel_labels, float* scores, int64_t* labels,
                                       int32_t* votes, uint8_t* smoothed, int32_t* counts, void* stream) {
  R3D_REQUIRE(voxel_index && voxel_ring && voxel_scores && in_scores && in_labels && in_votes && voxel_labels && scores && labels &&
                  votes && smoothed && counts,
              "r3d_scene_smooth_spread: null pointer (voxel_index %p, voxel_ring %p, voxel_scores %p, in_scores %p, in_labels %p, "
              "in_votes %p, voxel_labels %p, scores %p, labels %p, votes %p, smoothed %p, counts %p)",
              (const void*)voxel_index, (const void*)voxel_ring, (const void*)voxel_scores, (const void*)in_scores,
              (const void*)in_labels, (const void*)in_votes, (void*)voxel_labels, (void*)scores, (void*)labels, (void*)votes,
              (void*)smoothed, (void*)counts);
  SC_TRY(sc_check_points("r3d_scene_smooth_spread", M));
  SC_TRY(gr_check_rows("r3d_scene_smooth_spread", M, n_voxels, "voxels"));
  R3D_REQUIRE(n_cols >= 1 && n_cols <= R3D_SCENE_SCORE_COLS_MAX, "r3d_scene_smooth_spread: %d score columns (1 .. 64)", n_cols);
  const hipStream_t st = (hipStream_t)stream;
  r3d_zero_words(counts, R3D_SCENE_SMOOTH_COUNTS, st);
  hipLaunchKernelGGL(r3d_scene_smooth_labels_kernel, dim3(sc_grid_of(n_voxels)), dim3(SC_THREADS), 0, st, (int)n_voxels, n_cols,
                     voxel_scores, voxel_ring, (long long*)voxel_labels, counts);
  hipLaunchKernelGGL(r3d_scene_smooth_spread_kernel, dim3(sc_count_grid(M)), dim3(SC_THREADS), 0, st, (int)M, n_cols, (int)n_voxels,
                     voxel_index, voxel_ring, voxel_scores, (const long long*)voxel_labels, in_scores, (const long long*)in_labels,
                     in_votes, scores, (long long*)labels, votes, smoothed, counts);
  R3D_LAUNCH_CHECK("r3d_scene_smooth_spread");
  return R3D_OK;
}
