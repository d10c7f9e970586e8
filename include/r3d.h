/* r3d.h -- C ABI of libr3d_hip.so, the MI355X (gfx950) hot path of R3DFSSeg.
 *
 * The reference (Pixie8888/R3DFSSeg) is pure Python/PyTorch and has no FFI of its own;
 * each entry point below names the reference code it replaces (file:line under
 * /root/reference).  The binding a maintainer of the reference would add is a ctypes
 * stub, shown in INTEGRATION.md (r3dfsseg_amd/_lib.py is that stub).
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is DEVICE memory owned by the caller
 *     (PyTorch caching allocator in practice), borrowed for the duration of the call;
 *   - kernels never allocate; scratch is passed in (sizes from the *_ws_words helpers); the entry points whose scratch is
 *     carved into many arrays (prototypes, label propagation, contrastive loss, reverse neighbour list) also take its
 *     size in words and return an error for a short buffer instead of writing past it;
 *   - every function enqueues on `stream` (a hipStream_t passed as void*) and returns
 *     immediately: 0 = OK, non-zero = error, message in r3d_last_error_string();
 *   - no host synchronisation anywhere: data-dependent counts (points per class,
 *     prototypes, graph nodes) stay in a device-side descriptor;
 *   - activations are POINT-MAJOR fp32 matrices (one point per row, `ld*` = row stride in
 *     floats); the reference's channel-major (B, C, N) tensors are converted at the
 *     forward() boundary by r3d_cm_to_pm / r3d_pm_to_cm;
 *   - indices are int32;
 *   - an operation works on a BATCH OF EPISODES.  Episodes are independent units (the reference runs one per step,
 *     mpti_train_noise.py:57-98); E of them go through ONE launch sequence, and one episode is a batch of one.
 *     Encoder side, SEGMENTS: the clouds of the batch are rows of one matrix, episode after episode, [S support clouds |
 *     Q query clouds] each; BatchNorm keeps the statistics of every getFeatures call apart (models/mpti.py:434,436), so
 *     the `_seg` entry points take the two alternating segment sizes (rows_a = S N, rows_b = Q N, or in clouds) --
 *     segment 2 e + p is call p of episode e, rows_b == 0 means equal segments (rows_a = all rows: one segment) -- and
 *     address the BatchNorm vectors of segment s at (pointer + s * bn_stride).
 *     Head side: the `_batched` entry points take n_ep and the stride of every per-episode array (capacity sized);
 *     every pointer addresses episode 0.  The attention calls take seed_group, the clouds per episode.
 *     A segment's / an episode's results do not depend on the batch it runs in: reductions are partitioned by the
 *     segment's own size and summed relative to its first element.
 *   - a few operations keep a single-episode call beside the batched one (r3d_knn_topk, r3d_label_propagate,
 *     r3d_protonet_head, r3d_pointwise_conv_stats, the D = 64 attention calls): the same kernels on a batch of one.
 */
#ifndef R3D_H
#define R3D_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The NUMBERS of the contract -- the words of the records and descriptors the host reads back, their sizes, the flag and
 * enum values passed in or returned, the limits an entry point refuses beyond -- are the `#define R3D_<NAME> <value>`
 * lines of this header, each next to the entry points it belongs to, and are written nowhere else: the kernels include
 * this header, r3dfsseg_amd/_lib.py parses it (parse_constants) and r3dfsseg_amd/ops.py exports every one without its
 * prefix.  A value is an integer expression over literals and constants defined above it: decimal, hex, an L suffix,
 * + - * << |, parentheses.  No function-like macros. */
#define R3D_ABI_VERSION 6 /* what r3d_abi_version() returns; its history is beside that entry point */
/* what an entry point that returns int returns */
#define R3D_OK 0
#define R3D_ERR_ARG 1
#define R3D_ERR_LAUNCH 2
#define R3D_ERR_UNSUPPORTED 3

const char* r3d_last_error_string(void);
int r3d_abi_version(void); /* 6: r3d_scene_prepare / _vote take the optional sws, r3d_scene_transfer the optional idw outputs */
/* Arithmetic of the GEMM-shaped kernels that decide no index (self-attention forward / backward, r3d_pointwise_conv*,
 * r3d_gemm_tn): 0 = fp32 matrix core (v_mfma_f32_32x32x2_f32), 1 = every fp32 operand cut into three bf16 pieces, six
 * v_mfma_f32_32x32x16_bf16 per product block accumulated in fp32 (fp32-level accuracy at 2.67x the matrix rate;
 * csrc/common.h, csrc/gemm_bx3.hip).  kNN scores and the EdgeConv edge GEMM, which decide indices, always run on the
 * fp32 core.  Default 1.  Process-wide; call before the first launch.  The attention entry points use mode 1 only when
 * they are given a workspace (the packed operands live there); the GEMMs fall back to the fp32 kernels for shapes the
 * bf16 form does not take (K % 32 != 0, fewer than 32 output columns, operands not 16-byte aligned). */
/* test utility: fills the chip's LDS with `pattern` (no result of this library may depend on stale LDS contents) */
int r3d_debug_poison_lds(unsigned pattern, unsigned* sink /* 1 device word */, void* stream);
/* test / A-B utility: the CG's SpMV runs on its LDS-resident form when the launch holds at least min_blocks 128-row
 * workgroups (default 256; 0 = always, INT_MAX = never); both forms give the same bits.  Returns the previous value. */
int r3d_debug_set_cg_spmv_lds_min_blocks(int min_blocks);
int r3d_set_matrix_arith(int mode);
int r3d_get_matrix_arith(void);
/* A/B knob under mode 1: bit 0 the point-wise GEMM takes the bf16 form, bit 1 the weight-gradient GEMM does (default 3). */
int r3d_debug_set_gemm_bx3(int mask);

/* ---- layout conversion at the forward() boundary (models/mpti.py:433-437) -------- */
int r3d_cm_to_pm(const float* in /*(B,C,N)*/, int B, int C, int N, float* out /*(B*N,ld)*/, long ld, void* stream);
int r3d_pm_to_cm(const float* in /*(B*N,ld)*/, long ld, int B, int C, int N, float* out /*(B,C,N)*/, void* stream);
long r3d_cm_pitch(int N); /* row pitch (floats) of internal channel-major copies: avoids power-of-two channel strides */
int r3d_copy_cols(const float* src, long ld_src, float* dst, long ld_dst, long M, int C, void* stream);

/* ---- k nearest neighbours ----------------------------------------------------------
 * mode R3D_SCORE_DGCNN: models/dgcnn.py:17-23 knn(x,k): score = -xx[j] + 2<xi,xj> - xx[i], k largest.
 * mode R3D_SCORE_L2: models/mpti.py:733-735 faiss.IndexFlatL2.search: score = -max(0,|xi|^2+|xj|^2-2<xi,xj>).
 * Inner products are channel-ascending fp32 fma chains (bit-exact vs oracle/r3d_oracle.c);
 * ties resolve to the lower index; columns are sorted best first.
 * x (B*N, ldx); norm_ws (B*N) scratch; idx_out (B,N,k) int32; score_out optional (B,N,k);
 * n_valid_dev optional device int: only rows < *n_valid_dev take part. 1 <= k <= min(N,256).
 * x_cm: optional (B,C,N) channel-major copy (the reference's own tensor layout); the streamed
 * kernel (k <= 32, C <= 64) reads its operands from it and makes the copy into cm_ws (B*C*N
 * floats) when x_cm is NULL.
 * status: optional device int32.  For k > 32 a non-NULL status selects the two-pass
 * append-and-rank kernel; bit 0 set afterwards means its survivor buffer overflowed and the
 * call must be repeated with status == NULL (insertion kernel, always exact). */
#define R3D_SCORE_DGCNN 0
#define R3D_SCORE_L2 1
long r3d_knn_norm_ws_words(int B, int N);  /* floats of norm_ws: B*N norms + per-tile overflow flags */
int r3d_knn_topk(const float* x, long ldx, const float* x_cm, int B, int N, int C, int k, int mode,
                 const int32_t* n_valid_dev, float* norm_ws, float* cm_ws, int32_t* idx_out, float* score_out,
                 int32_t* status, void* stream);
/* B point sets with their own valid counts: set b has n_valid_dev[b * n_valid_stride] rows (the graph nodes of B episodes'
 * label-propagation systems, each at its capacity N).  status: ONE word for the batch.
 * ws: one scratch of r3d_knn_ws_words(B, N, C, k, flags) floats, 16-byte aligned; flags: R3D_KNN_FLAG_STATUS = status is
 * given, R3D_KNN_FLAG_X_CM = x_cm is given.  The library places in it what the path it selects needs: the squared norms, per-tile overflow flags,
 * the channel-major copy, the two partial lists per row when the large-k kernel splits its candidate axis (so few query
 * tiles that even twice as many workgroups fit the chip in one round), and the bf16 pieces of the points (C % 64 == 0,
 * needs x): the streamed kernels then run their THRESHOLD pass -- which only needs a lower bound of every score -- on the
 * bf16 matrix core, and for k <= 32 (x 16-byte aligned, ldx % 4 == 0) their second pass as a bf16 FILTER: a candidate
 * whose score's upper bound reaches the threshold is kept, and only the kept ones (~k + 10 per query) get their exact
 * score -- the fp32 fmaf chain in channel order, bit for bit the accumulation of the all-pairs fp32 pass it replaces.
 * Indices and scores are the same bits on every path. */
#define R3D_KNN_FLAG_STATUS 1
#define R3D_KNN_FLAG_X_CM 2
#define R3D_KNN_FLAG_NO_X 4          /* r3d_debug_knn_path only */
#define R3D_KNN_FLAG_FIXED_SCRATCH 8 /* r3d_debug_knn_path only */
long r3d_knn_ws_words(int B, int N, int C, int k, int flags);
int r3d_knn_topk_batched(const float* x, long ldx, const float* x_cm, int B, int N, int C, int k, int mode,
                         const int32_t* n_valid_dev, int n_valid_stride, float* ws, long ws_words, int32_t* idx_out,
                         float* score_out, int32_t* status, void* stream);
/* test / A-B utility: 0 keeps the threshold pass on the fp32 core (same results).  Returns the
 * previous setting. */
int r3d_debug_set_knn_bf16_threshold(int on);
/* the same for the second pass: <= 0 keeps it the all-pairs fp32 pass, > 0 the bf16 filter where it applies (same results) */
int r3d_debug_set_knn_bf16_filter(int on);
/* test utility: the kernel configuration r3d_knn_topk[_batched] would launch for this call, as the launcher itself decides
 * it (one host function serves both), under the two switches above as they are set.  Launches nothing, needs no device.
 * flags: R3D_KNN_FLAG_STATUS status given, _X_CM x_cm given (as r3d_knn_ws_words), _NO_X x is NULL, _FIXED_SCRATCH the call
 * is r3d_knn_topk (fixed scratch: no bf16 pieces, no split lists).  ldx: row pitch of x; x_misalign_bytes: address of x
 * modulo 16.  Returns a bit mask, or -1 for a shape the calls refuse:
 *   R3D_KNN_PATH_MASK       path: _SMALL = k <= 32 append-and-rank (overflowed tiles redone exactly), _LARGE = large-k
 *                           append-and-rank (overflow -> status bit 0), _INSERTION = sorted insertion
 *   R3D_KNN_PATH_FEW        (path _SMALL) 8 waves per query tile instead of 4
 *   R3D_KNN_PATH_SPLIT      (path _LARGE) the candidate axis dealt to two workgroups per tile, lists merged
 *   R3D_KNN_PATH_BFA        the threshold pass runs on the bf16 matrix core
 *   R3D_KNN_PATH_FILTER     (path _SMALL) pass B is the bf16 filter + exact scores of the survivors
 *   R3D_KNN_PATH_CHAN_MASK  channel configuration: R3D_KNN_CHAN_ANY = chunks of 64 with a padded tail, _LE16 = (path
 *                           _SMALL) C <= 16, _FULL = C % 64 == 0
 *   R3D_KNN_PATH_REGS_MASK  (path _INSERTION) list registers per lane: R3D_KNN_REGS_1, _2, _4 (k <= 64, <= 128, <= 256) */
#define R3D_KNN_PATH_MASK 0x3
#define R3D_KNN_PATH_SMALL 0
#define R3D_KNN_PATH_LARGE 1
#define R3D_KNN_PATH_INSERTION 2
#define R3D_KNN_PATH_FEW 0x4
#define R3D_KNN_PATH_SPLIT 0x8
#define R3D_KNN_PATH_BFA 0x10
#define R3D_KNN_PATH_FILTER 0x20
#define R3D_KNN_PATH_CHAN_SHIFT 6
#define R3D_KNN_PATH_CHAN_MASK 0xC0
#define R3D_KNN_CHAN_ANY (0 << R3D_KNN_PATH_CHAN_SHIFT)
#define R3D_KNN_CHAN_LE16 (1 << R3D_KNN_PATH_CHAN_SHIFT)
#define R3D_KNN_CHAN_FULL (2 << R3D_KNN_PATH_CHAN_SHIFT)
#define R3D_KNN_PATH_REGS_SHIFT 8
#define R3D_KNN_PATH_REGS_MASK 0x300
#define R3D_KNN_REGS_1 (1 << R3D_KNN_PATH_REGS_SHIFT)
#define R3D_KNN_REGS_2 (2 << R3D_KNN_PATH_REGS_SHIFT)
#define R3D_KNN_REGS_4 (3 << R3D_KNN_PATH_REGS_SHIFT)
int r3d_debug_knn_path(int B, int N, int C, int k, int flags, long ldx, int x_misalign_bytes);
/* 1: launches captured into a hipGraph may use their stream's packed-weight scratch of the bf16 x 3 point-wise GEMM (it
 * must exist already: run the sequence eagerly on that stream first).  The caller promises that the captured graph is the
 * only user of that stream's scratch while it replays.  Default 0: captured launches take the kernel that cuts W itself
 * (same bits).  Returns the previous setting. */
int r3d_set_wpack_in_capture(int on);

/* ---- 1x1 convolution + folded BatchNorm/bias + activation ---------------------------
 * models/dgcnn.py:64-80 conv1d, models/mpti.py:18-40 BaseLearner, models/attention.py:39-41.
 * Out[m][j] = act(scale[j] * sum_k X[m][k] W[j][k] + shift[j]); act R3D_ACT_NONE, _RELU, _LRELU = LeakyReLU(0.2).
 * scale/shift may be NULL (1 / 0). */
#define R3D_ACT_NONE 0
#define R3D_ACT_RELU 1
#define R3D_ACT_LRELU 2
int r3d_pointwise_conv(const float* X, long ldx, const float* W /*(Co,K)*/, long M, int K, int Co,
                       const float* scale, const float* shift, int act, float* Out, long ldo, void* stream);
/* test utility: the kernel r3d_pointwise_conv / _acc / _stats / _stats_seg launch for these operands, as the launcher itself
 * decides it (one host function serves both), under r3d_get_matrix_arith() and the r3d_debug_set_gemm_bx3 mask as they are
 * set: 0 = r3d_pointwise_gemm_kernel (fp32 core), 1 = r3d_pointwise_gemm_bx3_kernel (bf16 x 3, W cut per tile),
 * 2 = r3d_pointwise_gemm_bx3p_kernel (bf16 x 3, W packed once per call; mask bit 2 and M >= 256).  The bf16 forms need
 * K % 32 == 0, Co >= 32, Co % 4 == 0, M >= 64, ldx % 4 == 0, ldo % 4 == 0 and X, W, Out 16-byte aligned (*_misalign_bytes:
 * the address modulo 16).  no_scratch != 0: the stream can have no packed-W scratch (a capturing stream without
 * r3d_set_wpack_in_capture), where 1 stands in for 2 with the same bits.  Launches nothing, needs no device. */
int r3d_debug_pointwise_path(long M, int K, int Co, long ldx, long ldo, int x_misalign_bytes, int w_misalign_bytes,
                             int out_misalign_bytes, int no_scratch);

/* ---- fused EdgeConv: gather + 2-layer edge MLP + max over K --------------------------
 * models/dgcnn.py:26-61,117-118.  PQ (B*N,128) = [s1*Wa x | s1*(Wb-Wa) x + t1] per point
 * (from r3d_pointwise_conv), idx (B,N,K) local neighbour ids, W2 (64,64), s2/t2 (64) folded BN2.
 * out (B*N, ldo) 64 columns; argmax_out optional (B*N,64) winning neighbour slot.
 * Shapes: N a multiple of 4, K in {4, 8, ..., 32}; neighbour ids outside [0, N) are clamped, never dereferenced. */
int r3d_edgeconv_fwd(const float* PQ, const int32_t* idx, const float* W2, const float* s2, const float* t2,
                     float* out, long ldo, int B, int N, int K, int32_t* argmax_out, void* stream);

/* ---- point self-attention (models/attention.py:43-46), forward and flash-style backward ----
 * Head width D in {32, 64, 96, 128} (the reference's --output_dim); any other D is refused (R3D_ERR_ARG) before a launch
 * and r3d_attention_ws_words_ep_d returns -1 for it.  qkv (B*N, ld >= 3D): q / sqrt(D) | k | v at columns 0 | D | 2D;
 * out / O / dO (B*N, D columns); lse_out (B*N), saved for the backward; dqkv (B*N, ldd >= 3D).
 * Dropout on the attention weights (attention.py:45): p_drop, effective seed = seed + *seed_dev (seed_dev may be NULL; a
 * captured hipGraph bumps *seed_dev per replay).  p_drop = 0 is the inference forward.
 * Batches of episodes: clouds [e seed_group, (e + 1) seed_group) are episode e (seed_group == 0: all B clouds are one),
 * whose dropout mask is the one a call on those clouds alone draws with seed + 2 e (the one-episode schedule advances its
 * seed by 2 per episode); outputs are bit for bit those of that call.
 * ws: r3d_attention_ws_words_ep_d(B, N, seed_group, D) floats.  It holds the packed bf16 x 3 operands (without it the
 * forward runs on the fp32 core) and the partials of the key-axis split, which is chosen for ONE episode (seed_group
 * clouds) whatever the batch.  The forward may run without ws, the backward needs it.  B is a multiple of seed_group,
 * except in the forward with p_drop == 0, where seed_group only selects that split: a part of an episode's clouds (a
 * fitted support set, the query groups attached to it later) is split as the whole episode would be.
 * ws_holds_packed_qkv != 0: ws is the workspace the forward ran with on this qkv, untouched since (the bf16 x 3 kernels
 * reuse the packed q | k | v pieces it holds instead of cutting them again). */
long r3d_attention_ws_words_ep_d(int B, int N, int seed_group, int D);
int r3d_attention_fwd_train_ep_d(const float* qkv, long ld, int B, int N, float* out, long ldo, float* lse_out, float p_drop,
                                 unsigned seed, const unsigned* seed_dev, int seed_group, int D, float* ws, void* stream);
int r3d_attention_bwd_ep_d(const float* qkv, long ld, int B, int N, const float* O, long ldo, const float* dO, long lddo,
                           const float* lse, float p_drop, unsigned seed, const unsigned* seed_dev, int seed_group, int D,
                           float q_scale, float* dqkv, long ldd, float* ws, int ws_holds_packed_qkv, void* stream);
/* the D = 64 case on one episode (seed_group = 0); r3d_attention_bwd is r3d_attention_bwd_ws with ws_holds_packed_qkv = 0 */
long r3d_attention_ws_words(int B, int N);
int r3d_attention_fwd_train(const float* qkv, long ld, int B, int N, float* out, long ldo, float* lse_out, float p_drop,
                            unsigned seed, const unsigned* seed_dev, float* ws /*opt*/, void* stream);
int r3d_attention_bwd(const float* qkv, long ld, int B, int N, const float* O, long ldo, const float* dO, long lddo,
                      const float* lse, float p_drop, unsigned seed, const unsigned* seed_dev, float q_scale, float* dqkv,
                      long ldd, float* ws, void* stream);
int r3d_attention_bwd_ws(const float* qkv, long ld, int B, int N, const float* O, long ldo, const float* dO, long lddo,
                         const float* lse, float p_drop, unsigned seed, const unsigned* seed_dev, float q_scale,
                         float* dqkv, long ldd, float* ws, int ws_holds_packed_qkv, void* stream);

/* ---- multi-prototype extraction (models/mpti.py:597-715) -----------------------------
 * FPS (start index 0, ties lowest index) -> sorted unique seeds -> nearest-seed assignment ->
 * cluster means, for background + each way, then query rows appended: fills node rows
 * [0, n_proto) and [n_proto, n_proto + n_query_pts) of `nodes` and the label matrix Y.
 * desc: device int32[r3d_head_desc_words() = R3D_HD_WORDS], the words below; a segment is the background or one way.
 * Seeds per segment of n > k points: what torch_cluster.fps(feat, None, ratio = k / n) draws at the call site
 * models/mpti.py:612-613, ceil(float32(n) * float32(k / n)) = k or k + 1 (101 for 5.8 % of the n <= 20480 at k = 100),
 * so a segment can hold k + 1 prototypes: nodes / node_labels need (n_way + 1) * (k + 1) + n_query_pts rows, k < 128. */
#define R3D_HD_MAXSEG 8                         /* segments: n_way + 1 <= R3D_HD_MAXSEG */
#define R3D_HD_SEG_COUNT 0                      /* [R3D_HD_MAXSEG] points per segment */
#define R3D_HD_SEG_M R3D_HD_MAXSEG              /* [R3D_HD_MAXSEG] prototypes per segment */
#define R3D_HD_SEG_POFF (2 * R3D_HD_MAXSEG)     /* [R3D_HD_MAXSEG] first node row of the segment's prototypes */
#define R3D_HD_N_PROTO (3 * R3D_HD_MAXSEG)
#define R3D_HD_N_NODES (3 * R3D_HD_MAXSEG + 1)
#define R3D_HD_FPS_TIMEOUT (3 * R3D_HD_MAXSEG + 2) /* != 0: a workgroup of the one-launch FPS gave up waiting for its peers */
#define R3D_HD_WORDS (3 * R3D_HD_MAXSEG + 8)
int r3d_head_desc_words(void);
/* out[n], n in [0, n_max): the seeds a segment of n points gets at k (n <= k: n), as the device evaluates the count above
 * (device int32 out; for tests that hold it to the host arithmetic over every n). */
int r3d_fps_sample_count_table(int k, int n_max, int32_t* out, void* stream);
long r3d_head_proto_ws_words(int n_way, int k_shot, int N);
int r3d_head_proto_ws_offsets(int n_way, int k_shot, int N, long* out6 /* comp,mind,assign,cand,sel,seeds */);
/* flags: R3D_HEAD_FPS_ONE_LAUNCH = all FPS rounds in one persistent launch (points stay in registers; needs the
 * grid co-resident: episodes in flight x support points / 256 <= ~384 workgroups; desc word R3D_HD_FPS_TIMEOUT reports
 * a wait time-out); 0 = one launch per round. */
#define R3D_HEAD_FPS_ONE_LAUNCH 1
/* n_ep episodes in one launch sequence (every pointer addresses episode 0).  Per episode: support_y (n_way*k_shot, N),
 * shot_keep optional (n_way*k_shot), feat (S*N, ldf), qfeat (n_q*N, ldq), node_labels (n_cap, 4), assign_out (2*S*N;
 * optional for one episode), cluster_count optional (n_cap).  Strides between consecutive episodes:
 * support_y / shot_keep / desc / assign / cluster_count / ws in int32 words (ws_stride even, >= the scratch size), feat /
 * qfeat / nodes in ROWS.  fps_group: episodes whose farthest-point samplings share one persistent launch (their workgroups
 * must be co-resident: ~500 workgroup slots at D <= 192, 250 above; an episode needs ceil(S N / 256) + n_way + 1). */
int r3d_head_prototypes_batched(int n_ep, int fps_group, const int32_t* support_y, long sy_stride, const int32_t* shot_keep,
                                long keep_stride, const float* feat, long ldf, long feat_ep_rows, const float* qfeat, long ldq,
                                long qfeat_ep_rows, int n_way, int k_shot, int N, int D, int n_query_pts, int k, float* nodes,
                                long ldn, long nodes_ep_rows, float* node_labels, int32_t* desc, long desc_stride,
                                int32_t* assign_out, long assign_stride, int32_t* cluster_count, long ccount_stride,
                                int32_t* ws, long ws_words, long ws_stride, int flags, void* stream);
/* A support set fitted once, queried many times: the prototypes of models/mpti.py:488-489 depend on the support set alone,
 * the node matrix of :508 is cat(prototypes, query_feat).  ONE fitted system -- the first rows of the nodes / node_labels a
 * r3d_head_prototypes_batched call left (n_way > 3: its second label plane fit_label_rows rows behind the first), its desc
 * and, optionally, its cluster_count -- is attached to n_sys systems of query rows (system g's n_query_pts rows start
 * qfeat_sys_rows rows after system g - 1's): destination system g (node / label rows [g n_cap, (g + 1) n_cap), plane 1 of
 * the labels n_sys * n_cap rows behind plane 0) receives the n_proto prototype rows and their label rows, then its query
 * rows with zero label rows; its desc is the fitted one with n_nodes = n_proto + n_query_pts.  n_proto is read from
 * fit_desc ON THE DEVICE (no host read) and clamped to proto_cap, the prototype rows the fitted system can hold,
 * (n_way + 1) * (k + 1); proto_cap + n_query_pts > n_cap is refused with an error code.  One pass of 16-byte loads and
 * stores: D, fit_ldn, ldq, ldn multiples of 4, all row pointers 16-byte aligned.  Afterwards r3d_knn_topk_batched,
 * r3d_label_propagate_batched and r3d_query_logits_ce_batched run on the destination as after r3d_head_prototypes_batched. */
int r3d_head_attach_queries_batched(int n_sys, const float* fit_nodes, long fit_ldn, const float* fit_labels,
                                    long fit_label_rows, const int32_t* fit_desc, const int32_t* fit_cluster_count,
                                    int proto_cap, const float* qfeat, long ldq, long qfeat_sys_rows, int n_way, int D,
                                    int n_query_pts, float* nodes, long ldn, int n_cap, float* node_labels, int32_t* desc,
                                    long desc_stride, int32_t* cluster_count, long ccount_stride, void* stream);
/* r3d_head_attach_queries_sets: n_sets fitted systems against n_groups groups of query rows in one launch.  fits: a
 * DEVICE table of n_sets rows of 4 addresses {nodes, node_labels, desc, cluster_count or 0} of fitted systems that share
 * fit_ldn, fit_label_rows and proto_cap (fits of one model do); their pointers meet the alignment rules above, which only
 * the caller can check.  Destination system g * n_sets + k is what r3d_head_attach_queries_batched builds from fit k and
 * group g -- the same device function, so the same bits in its node matrix, label rows, desc and cluster counts --;
 * plane 1 of the labels lies n_groups * n_sets * n_cap rows behind plane 0.  At most 65535 systems. */
int r3d_head_attach_queries_sets(int n_groups, int n_sets, const uint64_t* fits, long fit_ldn, long fit_label_rows,
                                 int proto_cap, const float* qfeat, long ldq, long qfeat_sys_rows, int n_way, int D,
                                 int n_query_pts, float* nodes, long ldn, int n_cap, float* node_labels, int32_t* desc,
                                 long desc_stride, int32_t* cluster_count, long ccount_stride, void* stream);

/* ---- affinity + label propagation (models/mpti.py:717-776) ---------------------------
 * nbr (n_cap, kp1) from r3d_knn_topk mode 1 (column 0 is dropped as in mpti.py:736).
 * Z = (I - alpha D^-1/2 A D^-1/2)^-1 Y (all columns at once), A the symmetrised gaussian kNN affinity with zero
 * diagonal, solved by two-level conjugate gradients: coarse space = D^1/2 x indicators of 64 aggregates (nodes
 * grouped around an even subsample of the first *n_proto_dev rows, the prototypes), A-DEF2 preconditioner.
 * nodes rows are read as float4 (ldn % 4 == 0, 16-byte aligned); Y, Z (n_cap, 4) fp32, 16-byte aligned; n_cap <= 32768.
 * D: a multiple of 4, at most 256 -- anything else is refused before a launch, by r3d_label_propagate(_batched) and by
 * r3d_label_propagate_bwd_batched alike (the seed rows of the coarse space are staged as whole float4).
 * ws: r3d_lp_ws_words(n_cap, kp1) int32 words, 16-byte aligned; it keeps the graph, the coarse space and the
 * directed weights for r3d_label_propagate_bwd_batched.  stats_out optional device int32[2] = {converged, iterations}.
 * r3d_lp_ws_offsets: int32-word offsets inside ws of {row_ptr, col (uint16 entries), val, dinv, aggregate ids,
 * solver state} for tests and tools that read the system back; r3d_lp_ws_offsets_coarse: those of {M W (n_cap, 64) fp32,
 * the 16 partial matrices of E (16, 64, 64), E^-1 (64, 64) fp32, the CG residual r (n_cap, 4) fp32}. */
long r3d_lp_ws_words(int n_cap, int kp1);
int r3d_lp_ws_offsets(int n_cap, int kp1, long* out6);
int r3d_lp_ws_offsets_coarse(int n_cap, int kp1, long* out4);
int r3d_label_propagate(const float* nodes, long ldn, int D, const int32_t* nbr, int kp1, const float* Y,
                        const int32_t* n_dev, const int32_t* n_proto_dev, int n_cap, float sigma, float alpha,
                        int max_iter, float tol, float* Z, int32_t* ws, long ws_words, int32_t* stats_out, void* stream);

/* n_ep systems at once: system e = rows [e n_cap, (e + 1) n_cap) of nodes / nbr / Y / Z, counts at n_dev[e desc_stride] /
 * n_proto_dev[e desc_stride], scratch ws + e ws_stride (a multiple of 4 words, >= r3d_lp_ws_words), {converged, iterations}
 * at stats_out + e stats_stride.  Every CG launch serves all systems (two launches per iteration for the whole batch). */
int r3d_label_propagate_batched(int n_ep, const float* nodes, long ldn, int D, const int32_t* nbr, int kp1, const float* Y,
                                const int32_t* n_dev, const int32_t* n_proto_dev, long desc_stride, int n_cap, float sigma,
                                float alpha, int max_iter, float tol, float* Z, int32_t* ws, long ws_words, long ws_stride,
                                int32_t* stats_out, long stats_stride, void* stream);
/* Runtime guard for schedules with several streams in flight: recomputes the directed gaussian weights of
 * the graphs a preceding r3d_label_propagate(_batched) left in ws -- to be called with nothing else on the chip -- and adds
 * to *mismatch_out the number of entries whose bits differ from the ones the solve used.  scratch:
 * n_ep * r3d_graph_weights_verify_words(n_cap, kp1) floats. */
long r3d_graph_weights_verify_words(int n_cap, int kp1);
int r3d_graph_weights_verify(int n_ep, const float* nodes, long ldn, int D, const int32_t* n_dev, long desc_stride, int n_cap,
                             int kp1, float sigma, int32_t* ws, long ws_words, long ws_stride, float* scratch,
                             int32_t* mismatch_out, void* stream);

/* More than 3 ways (5..8 classes; models/mpti.py:49,58 take any n_way): label columns travel as float4 per node, so Y, Z
 * (and G, lambda of the backward) are TWO planes of 4 columns, (2, n_ep * n_cap, 4), plane 1 = classes 4..7, written /
 * read that way by r3d_head_prototypes_batched, r3d_query_logits_ce_batched, r3d_ce_grad_batched and
 * r3d_train_metrics_batched.  The label propagation is column-wise independent: r3d_label_propagate_batched solves plane 0
 * and leaves graph, weights and preconditioner in ws; this entry point solves further right-hand sides (plane 1) on them.
 * The backward is called once per plane (its outputs add). */
int r3d_label_propagate_solve_batched(int n_ep, const float* Y, const int32_t* n_dev, long desc_stride, int n_cap, int kp1,
                                      float alpha, int max_iter, float tol, float* Z, int32_t* ws, long ws_words,
                                      long ws_stride, int32_t* stats_out, long stats_stride, void* stream);

/* Captured episodes: enable the CG kernel nodes (three per iteration) of iterations < budget in an instantiated hipGraph holding
 * r3d_label_propagate(_batched) / r3d_label_propagate_bwd_batched launches, disable the rest (no dispatch for them).  graph: the
 * hipGraph_t the hipGraphExec_t graph_exec was instantiated from.  n_cg (optional, host): CG nodes found.
 * No reference counterpart (the reference inverts the dense matrix, models/mpti.py:758-776). */
int r3d_graph_set_lp_budget(void* graph, void* graph_exec, int budget, int* n_cg);

/* ---- query logits + cross entropy (models/mpti.py:558-559, 778-781) ------------------
 * per system of a batch: Z rows [e z_ep_rows, ...) -> logits / loss / pred number e of the batch arrays; per system
 * labels optional (n_q, N), logits (n_q, n_classes, N), loss_out optional (1), pred_out optional (n_q*N) */
int r3d_query_logits_ce_batched(int n_ep, const float* Z, long z_ep_rows, const int32_t* n_proto_dev, long desc_stride, int n_q,
                                int N, int n_classes, const int64_t* labels, float* logits, float* loss_out, int32_t* pred_out,
                                void* stream);

/* ==== training mode (BatchNorm with batch statistics, backward) =======================
 * A conv+BN+act layer: z = r3d_pointwise_conv_stats_seg (GEMM + statistics; or r3d_pointwise_conv, no affine ->
 * r3d_colstats_seg mode 0) -> r3d_bn_fold_seg -> r3d_affine_act_seg.  Backward: r3d_colstats_seg mode 1 (sum du,
 * sum du*zhat = dbeta, dgamma) -> r3d_bn_bwd_apply_seg (dz) -> r3d_pointwise_conv(_acc)(dz, W^T) for dX,
 * r3d_gemm_tn(dz, X) for dW.
 * Reference: nn.BatchNorm{1,2}d in train mode inside models/dgcnn.py:45-80, models/mpti.py:31-39. */
int r3d_pointwise_conv_acc(const float* X, long ldx, const float* W, long M, int K, int Co, const float* scale,
                           const float* shift, int act, float* Out, long ldo, void* stream);
/* z = X W^T together with its column sums (sum z, sum z^2) from the GEMM epilogue: the batch statistics of the
 * layer without a second pass over z.  ws: r3d_pointwise_conv_stats_ws_words(M, Co) floats. */
long r3d_pointwise_conv_stats_ws_words(long M, int Co);
int r3d_pointwise_conv_stats(const float* X, long ldx, const float* W, long M, int K, int Co, float* Out, long ldo,
                             float* sums_out /*[2][Co]*/, float* ws, void* stream);
/* the same with separate statistics for the alternating row segments of a batch of episodes (support and query clouds
 * are normalised separately, mpti.py:434,436; rows_a, rows_b multiples of 64): ONE GEMM launch, sums_out [seg][2][Co] */
int r3d_pointwise_conv_stats_seg(const float* X, long ldx, const float* W, long M, int K, int Co, float* Out, long ldo,
                                 long rows_a, long rows_b, float* sums_out, float* ws, void* stream);
/* Column statistics, folding and the element-wise passes over segments: sums / outputs [seg][...], BatchNorm vectors of
 * segment s at pointer + s * bn_stride, running statistics or records updated in segment order = the reference's order of
 * getFeatures calls.  r3d_colstats_seg: mode 0 (sum x, sum x^2), mode 1 (sum du, sum du*zhat; needs DY and the vectors);
 * ws: r3d_colstats_seg_ws_words floats.
 * rec (optional): instead of updating the running statistics, record (batch mean, unbiased batch variance) as 2 C floats at
 * rec + (*rec_index_dev + s) * rec_stride; r3d_bn_running_update then applies n_records such records in order, bit for bit
 * what the updates would have given one after the other (captured episodes of several streams record, the owner
 * applies them in episode order after the step). */
long r3d_colstats_seg_ws_words(long M, int C, long rows_a, long rows_b);
int r3d_colstats_seg(const float* X, long ldx, const float* DY, long lddy, long M, int C, long rows_a, long rows_b, int mode,
                     const float* scale, const float* shift, const float* mean, const float* invstd, long bn_stride, int act,
                     float* sums_out /*[seg][2][C]*/, float* ws, void* stream);
int r3d_bn_fold_seg(const float* sums /*[seg][2][C]*/, int n_seg, double count_a, double count_b, int C, const float* gamma,
                    const float* beta, float eps, float momentum, float* running_mean /*opt*/, float* running_var /*opt*/,
                    float* mean, float* invstd, float* scale, float* shift, long bn_stride, float* rec /*opt*/,
                    const int32_t* rec_index_dev /*opt*/, long rec_stride, void* stream);
int r3d_affine_act_seg(const float* Z, long ldz, long M, int C, long rows_a, long rows_b, const float* scale, const float* shift,
                       long bn_stride, int act, float* Y, long ldy, void* stream);
int r3d_bn_bwd_apply_seg(const float* Z, long ldz, const float* DY, long lddy, long M, int C, long rows_a, long rows_b,
                         const float* scale, const float* shift, const float* mean, const float* invstd, long bn_stride, int act,
                         const float* sums /*[seg][2][C]*/, double count_a, double count_b, float* DZ, long lddz, void* stream);
int r3d_bn_running_update(const float* rec, int n_records, long rec_stride, int C, float momentum,
                          const float* bias /*opt: conv bias in front of the BatchNorm*/, float* running_mean,
                          float* running_var, void* stream);
long r3d_gemm_tn_ws_words(long M, int Ca, int Cb);
int r3d_gemm_tn(const float* A, long lda, const float* B, long ldb, long M, int Ca, int Cb, float alpha, float* out,
                int accumulate, float* ws, void* stream);
/* test utility: the plan of r3d_gemm_tn for this shape, as the launcher itself decides it (one host function serves both),
 * under r3d_get_matrix_arith() and the r3d_debug_set_gemm_bx3 mask as they are set.  Returns bit 0 = bf16 x 3 (Ca >= 32 and
 * Cb >= 32), bit 1 = its 256 x 64 tiles (Cb <= 64; 128 x 128 otherwise); *rows = rows per chunk of the M axis, *chunks =
 * their number (host ints, either may be NULL).  Launches nothing, needs no device. */
int r3d_debug_gemm_tn_plan(long M, int Ca, int Cb, int* rows, int* chunks);
int r3d_add_cols(const float* src, long ld_src, float* dst, long ld_dst, long M, int C, void* stream);

/* EdgeConv with batch statistics over the edges of every segment of clouds (models/dgcnn.py:53-57 in train mode; segments
 * of clouds_a / clouds_b clouds alternating, clouds_b == 0: equal segments -- the S support and Q query clouds of every
 * episode of a batch) and its backward; PQ is the RAW point-wise GEMM [Wa x | (Wb-Wa) x].  One launch per pass over ALL
 * clouds; statistics are per segment ([seg][2][64]), BatchNorm vectors of segment s at pointer + s * bn_stride.
 * ws: r3d_edgeconv_train_ws_words(B, N) floats. */
long r3d_edgeconv_train_ws_words(int B, int N);
int r3d_edge_stats1(const float* PQ, const int32_t* idx, int B, int N, int K, int clouds_a, int clouds_b,
                    float* sums_out /*[seg][2][64]*/, float* esum /*opt (B*N,64): sum_t e1 of every point*/, float* ws,
                    void* stream);
/* one-pass training forward: z2 statistics + per point/channel max and min of z2 over the K edges; BatchNorm2 +
 * LeakyReLU is monotone per channel, so r3d_edge_select finishes the layer once the statistics are folded */
int r3d_edgeconv_train_fwd_minmax(const float* PQ, const int32_t* idx, const float* s1, const float* t1, long bn_stride,
                                  const float* W2, int B, int N, int K, int clouds_a, int clouds_b, float* zmax, float* zmin,
                                  int32_t* argmax, int32_t* argmin, float* sums_out /*[seg][2][64]*/, float* ws, void* stream);
int r3d_edge_select(float* zmax /*in: max, out: selected z*/, const float* zmin, int32_t* argmax /*in/out*/,
                    const int32_t* argmin, const float* s2, const float* t2, long bn_stride, long M, long rows_a, long rows_b,
                    float* out, long ldo, void* stream);
/* reverse neighbour list (for every point the edges that name it, ascending): rev_ws = r3d_edge_reverse_ws_words int32
 * words.  The backward gathers along it instead of scattering with float atomics: deterministic gradients. */
long r3d_edge_reverse_ws_words(int B, int N, int K);
int r3d_edge_reverse(const int32_t* idx, int B, int N, int K, int32_t* rev_ws, long ws_words, void* stream);
/* bn2_sums [seg][2][64] in; dW2 (64,64) summed over the WHOLE batch, bn1_sums [seg][2][64], dPQ (B*N,128) out.
 * zwin (B*N,64): z2 of every max-pool winner (zmax after r3d_edge_select); esum: from r3d_edge_stats1.  Both given, N % 8 == 0,
 * dout 16-byte aligned with lddo % 4 == 0 and r3d_set_matrix_arith(1): the three edge GEMMs of the backward run on the bf16
 * matrix core in three-piece arithmetic (none decides an index: the winner and its side of the LeakyReLU kink come from
 * argmax / zwin); else on the fp32 core (r3d_debug_edgeconv_bwd_path tells which). */
int r3d_edgeconv_bwd(const float* PQ, const int32_t* idx, const float* s1, const float* t1, const float* mean1,
                     const float* invstd1, const float* W2, const float* s2, const float* t2, const float* mean2,
                     const float* invstd2, long bn_stride, const float* bn2_sums, const float* dout, long lddo,
                     const int32_t* argmax, const float* zwin /*opt*/, const float* esum /*opt*/, int B, int N, int K,
                     int clouds_a, int clouds_b, float* DY1 /*(B*N*K,64) scratch*/, float* BE /*(B*N,128) scratch*/,
                     const int32_t* rev_ws /* r3d_edge_reverse of the same idx */, float* dW2, float* bn1_sums, float* dPQ,
                     float* ws, void* stream);
/* test utility: the form r3d_edgeconv_bwd takes for these operands, as the launcher itself decides it (one host function
 * serves both), under r3d_get_matrix_arith() as it is set: 1 = bf16 x 3, 0 = fp32 core.  The bf16 x 3 form needs
 * r3d_set_matrix_arith(1), zwin and esum (have_zwin_esum != 0), N % 8 == 0, lddo % 4 == 0 and a 16-byte aligned dout
 * (dout_misalign_bytes: its address modulo 16).  Launches nothing, needs no device. */
int r3d_debug_edgeconv_bwd_path(int N, long lddo, int dout_misalign_bytes, int have_zwin_esum);

/* head backward (reference: autograd through models/mpti.py:488-512,571) for n_ep episodes.  r3d_ce_grad_batched -> G =
 * dL/dZ (scaled by the device scalar *gscale_dev); r3d_label_propagate_bwd_batched: adjoint CG solve on the graph
 * r3d_label_propagate(_batched) left in ws, then gradients w.r.t. the node features; r3d_head_prototypes_bwd_batched:
 * cluster-mean / query-row backward (dsfeat must be zero-initialised by the caller).  Layouts as the forward `_batched`
 * calls; G, lam, dnodes: n_cap rows per system; *gscale_dev scales every episode alike: the step's loss is the SUM of the
 * episodes' losses. */
int r3d_ce_grad_batched(int n_ep, const float* Z, const int32_t* n_proto_dev, long desc_stride, int n_cap, int n_query_pts,
                        int n_classes, const int64_t* labels, const float* gscale_dev, float* G, void* stream);
int r3d_label_propagate_bwd_batched(int n_ep, const float* nodes, long ldn, int D, int kp1, const float* Z, const float* G,
                                    const int32_t* n_dev, long desc_stride, int n_cap, float sigma, float alpha, int max_iter,
                                    float tol, float* lam, float* dnodes, long ldd, int32_t* ws, long ws_words, long ws_stride,
                                    int32_t* stats_out, long stats_stride, void* stream);
int r3d_head_prototypes_bwd_batched(int n_ep, const float* dnodes, long ldd, long nodes_ep_rows, int n_way, int k_shot, int N,
                                    int D, int n_query_pts, const int32_t* desc, long desc_stride, const int32_t* assign,
                                    long assign_stride, const int32_t* cluster_count, long ccount_stride, const int32_t* ws,
                                    long ws_stride, float* dsfeat, long lds_, long dsfeat_ep_rows, float* dqfeat, long ldq,
                                    long dqfeat_ep_rows, void* stream);

/* per-way supervised contrastive loss, train only (models/mpti.py:226-313): per shot FPS(4) prototypes of the
 * foreground points -> proj Linear(D,128) -> L2 normalise -> SupCon(temp); mean over ways.  ws keeps what
 * r3d_contrast_bwd needs (prototype gradients, assignments, per-way parameter gradients). */
long r3d_contrast_ws_words(int n_way, int k_shot, int N);
int r3d_contrast_fwd(const float* feat, long ldf, int D, const int32_t* support_y, const int32_t* support_flag, int n_way,
                     int k_shot, int N, const float* W, const float* bias, float temp, float* loss_out, float* ws,
                     long ws_words, void* stream);
int r3d_contrast_bwd(int D, int n_way, int k_shot, int N, const float* gscale_dev, float* dfeat, long ldd, float* dW,
                     float* db, float* ws, void* stream);
/* n_ep episodes: features of episode e at feat + e feat_ep_rows ldf, masks / flags entry e of (n_ep, S, N) / (n_ep, S),
 * scratch ws + e ws_stride, loss_out[e]; the backward sums dW / db over the batch */
int r3d_contrast_fwd_batched(int n_ep, const float* feat, long ldf, long feat_ep_rows, int D, const int32_t* support_y,
                             const int32_t* support_flag, int n_way, int k_shot, int N, const float* W, const float* bias,
                             float temp, float* loss_out, float* ws, long ws_words, long ws_stride, void* stream);
int r3d_contrast_bwd_batched(int n_ep, int D, int n_way, int k_shot, int N, const float* gscale_dev, float* dfeat, long ldd,
                             long dfeat_ep_rows, float* dW, float* db, float* ws, long ws_stride, void* stream);
/* training-only debug metrics (mpti.py:515-568): out4 = query_acc_LP, query_acc_original, clean_ratio_LP_avg,
 * clean_ratio_original_avg per episode; proto_ws: the scratch r3d_head_prototypes_batched ran with */
int r3d_train_metrics_batched(int n_ep, const int32_t* pred, const int64_t* query_y, const int64_t* gt_query_y, int n_query_pts,
                              const float* Z, long z_ep_rows, const int32_t* desc, long desc_stride, const int32_t* proto_ws,
                              long pws_stride, const int32_t* assign, long assign_stride, const int32_t* gt_support_y, int n_way,
                              int k_shot, int N, float* out4 /*(n_ep,4)*/, void* stream);

/* ---- clean-shot detection, eval only (models/mpti.py:87-223, 316-371) -----------------
 * Per shot: box means of foreground features at scales (1,1,1) and (2,2,1) -> cosine map ->
 * majority vote -> shot_keep (n_way*k_shot) int32 (0 = drop the shot's foreground).
 * Per episode: feat (S*N, ldf), episode e feat_ep_rows rows further on; support_x (S, Cin, N); support_y (S, N);
 * dbg_cos_sum optional (n_way, 2, 4*k_shot); ws: r3d_clean_ws_words int32 words, episode e at ws + e * ws_stride.
 * The vote: a seed is a non-empty box (bounds in fp32, inclusive on both sides: a point on a split plane lies in two
 * boxes); per way and scale a seed votes "clean" when its row sum is ABOVE the mean of the way's row sums, a shot's flag at
 * that scale is 1 when MORE than half of its seeds do, and the shot is dropped when the mean of its two flags is below 0.5.
 * A shot WITHOUT a seed at a scale -- no foreground point, which the reference cannot run on -- takes flag 0 at that
 * scale (so it is dropped while its way keeps another shot); a way that would lose every shot, a way without any
 * foreground included, keeps all of them.  dbg_cos_sum receives the row sums of the seeds that exist, entry
 * [way][scale][i] for seed i in shot order then box order, and is left untouched beyond them.
 * Layout of ws after the call (the tests read it; S = n_way*k_shot): box_sum (S, 5, 256) fp32 -- per shot and box the sum
 * of the foreground rows inside the box, channels >= D zero; box 0 is scale (1,1,1), boxes 1..4 scale (2,2,1), x outer,
 * y inner -- then, S*5*256 words in, box_cnt (S, 5) int32, the number of those rows.  The words beyond are not written. */
long r3d_clean_ws_words(int n_way, int k_shot);
int r3d_clean_shot_detect_batched(int n_ep, const float* feat, long ldf, long feat_ep_rows, int D, const float* support_x,
                                  int Cin, const int32_t* support_y, int n_way, int k_shot, int N, int32_t* shot_keep,
                                  float* dbg_cos_sum, int32_t* ws, long ws_stride, void* stream);

/* ---- ProtoNet head (models/protonet.py:295-349): masked average pooling + similarity ----
 * method 0 cosine * scaler, 1 -euclidean^2; anything else returns non-zero like the reference's
 * NotImplementedError.  Z (n_query_pts, 4) similarity rows; ws S*2*256 floats. */
int r3d_protonet_head(const float* sfeat, long ldf, const float* qfeat, long ldq, int D, const int32_t* support_y,
                      int n_way, int k_shot, int N, int n_query_pts, int method, float scaler, float* Z, float* ws,
                      void* stream);

/* The same head for n_ep episodes in one launch pair (shots x episodes, query tiles x episodes).  Layout conventions of
 * r3d_protonet_head_train_fwd below: sfeat / qfeat point at episode 0's support / query rows inside one feature matrix,
 * episode e starts feat_ep_rows rows further on; support_y (n_ep, S, N); Z (n_ep * n_query_pts, 4) per plane, plane 1
 * (classes 4..7) n_ep * n_query_pts rows further on when n_way > 3 (r3d_query_logits_ce_batched with z_ep_rows =
 * n_query_pts).  Per episode the result is bit for bit r3d_protonet_head's on that episode alone.  1 <= n_way <= 7,
 * D <= 256, n_ep <= 65535; ws: r3d_protonet_head_ws_words(...) floats (< 0: unsupported shape), 16-byte aligned. */
long r3d_protonet_head_ws_words(int n_ep, int n_way, int k_shot);
int r3d_protonet_head_batched(int n_ep, const float* sfeat, long ldf, const float* qfeat, long ldq, long feat_ep_rows, int D,
                              const int32_t* support_y, int n_way, int k_shot, int N, int n_query_pts, int method,
                              float scaler, float* Z, float* ws, long ws_words, void* stream);
/* The batched head with clean-shot flags (reference ProtoNet_Contrast: getPrototype(clean_flag=...), protonet.py:892-915).
 * shot_keep (n_ep, n_way*k_shot) int32 in device memory, as r3d_clean_shot_detect_batched writes it: the foreground
 * prototype of a way is the sum of its KEPT shots' pooled means over the NUMBER kept; the background prototype is still the
 * sum over all n_way*k_shot shots over n_way*k_shot -- a dropped shot keeps contributing background.  The shots are walked in
 * the order of r3d_protonet_head_batched, which is this call with shot_keep = NULL: NULL or all ones give its result bit for
 * bit.  Same launches, same scratch (r3d_protonet_head_ws_words), same limits.  A way with no kept shot is the caller's
 * error (the detection resets such a way to all kept, protonet.py:529-532).  shot_keep lives on the device and is read
 * only there, by the workgroups that form the prototypes: the DEVICE DOES NOT CHECK IT and the call returns 0; that way's
 * prototype is 0 / 0 and its similarity column NaN.  A caller that holds the flags on the host checks them there
 * (ops.protonet_head_batched does, for a host tensor). */
int r3d_protonet_head_keep_batched(int n_ep, const float* sfeat, long ldf, const float* qfeat, long ldq, long feat_ep_rows,
                                   int D, const int32_t* support_y, const int32_t* shot_keep, int n_way, int k_shot, int N,
                                   int n_query_pts, int method, float scaler, float* Z, float* ws, long ws_words,
                                   void* stream);
/* The two halves of the evaluation head, for a support set that is fitted once and queried many times (the prototypes
 * depend on the support set alone: getPrototype, models/protonet.py:892-915 with clean_flag, :326-336 without).
 * r3d_protonet_prototypes_batched: masked pooling (getMaskedFeatures, protonet.py:837-842) + prototypes -> protos
 * (n_ep, n_way + 1, D) fp32, background first; sfeat / feat_ep_rows / support_y / shot_keep as in
 * r3d_protonet_head_keep_batched (foreground: kept shots, background: every shot), ws: r3d_protonet_head_ws_words floats.
 * It reads the S*N support rows of each episode and nothing else.
 * r3d_protonet_similarity_batched: calculateSimilarity (protonet.py:338-349) of n_sys systems' query rows -- system g's
 * n_query_pts rows start q_sys_rows rows after system g - 1's -- against a prototype table, system g's at protos +
 * g * proto_stride floats; proto_stride = 0 broadcasts ONE table to every system.  Z as r3d_protonet_head_batched writes
 * it (n_sys * n_query_pts rows per plane).  It never touches support memory.
 * The pair computes what r3d_protonet_head_keep_batched computes, bit for bit: the same device functions form the
 * prototypes and the similarities in both (the fused call keeps the table in LDS instead of writing it out). */
int r3d_protonet_prototypes_batched(int n_ep, const float* sfeat, long ldf, long feat_ep_rows, int D, const int32_t* support_y,
                                    const int32_t* shot_keep, int n_way, int k_shot, int N, float* protos, float* ws,
                                    long ws_words, void* stream);
int r3d_protonet_similarity_batched(int n_sys, const float* qfeat, long ldq, long q_sys_rows, int D, const float* protos,
                                    long proto_stride, int n_way, int n_query_pts, int method, float scaler, float* Z,
                                    void* stream);
/* r3d_protonet_similarity_sets: n_sets prototype tables (table k at protos + k * proto_stride floats, n_sets * (n_way + 1)
 * <= 64 rows in all) against the query rows of n_groups groups (group g's n_query_pts rows start q_sys_rows rows after
 * group g - 1's), ONE launch in which a query row is read once and scored against every table.  System g * n_sets + k
 * is rows [(g * n_sets + k) * n_query_pts, ...) of Z (per plane n_groups * n_sets * n_query_pts rows), so
 * r3d_query_logits_ce_batched with n_ep = n_groups * n_sets leaves logits (n_groups, n_sets * (n_way + 1), N) when a
 * group is one cloud.  Per (row, prototype) the operations of r3d_protonet_similarity_batched in their order: set k's
 * rows have the bits of that call on table k alone. */
int r3d_protonet_similarity_sets(int n_groups, int n_sets, const float* qfeat, long ldq, long q_sys_rows, int D,
                                 const float* protos, long proto_stride, int n_way, int n_query_pts, int method, float scaler,
                                 float* Z, void* stream);
/* correct (n_ep) int32 = per episode #{pred == label}: pred (n_ep, n_pts) int32 as r3d_query_logits_ce_batched writes it,
 * labels (n_ep, n_pts) int64.  One host read then serves the accuracy of a whole batch. */
int r3d_count_correct_batched(int n_ep, const int32_t* pred, const int64_t* labels, long n_pts, int32_t* correct,
                              void* stream);

/* ---- ProtoNet head in training mode (reference: models/protonet.py:295-349 and autograd through it; the loop
 * models/proto_learner.py:55-67 intends) ------------------------------------------------
 * n_ep episodes per call: episode e's support / query rows start e * feat_ep_rows rows behind sfeat / qfeat, its masks are
 * entry e of support_y (n_ep, S, N).  Z / dZ: (n_ep * n_query_pts, 4), episode after episode; more than 3 ways: two planes
 * (2, n_ep * n_query_pts, 4), classes 4..7 in plane 1 (r3d_query_logits_ce_batched / r3d_ce_grad_batched with z_ep_rows =
 * n_cap = n_query_pts).  The forward splits the rows of a support cloud over workgroups (its Z agrees with
 * r3d_protonet_head's to rounding, not bit for bit) and leaves pooled means, per-shot counts, prototypes and their norms
 * in ws; the backward needs ws as the forward left it and the same shape arguments.  It WRITES dsfeat (S*N rows) and
 * dqfeat (n_query_pts rows) of every episode, e * dfeat_ep_rows rows further on for episode e: both may point into one
 * gradient matrix over [support rows | query rows].  Every reduction is deterministic (no floating-point atomics).
 * 1 <= n_way <= 7, D <= 256; ws: r3d_protonet_head_train_ws_words(...) floats (-1: unsupported shape), 16-byte aligned. */
long r3d_protonet_head_train_ws_words(int n_ep, int n_way, int k_shot, int N, int n_query_pts, int D);
int r3d_protonet_head_train_fwd(int n_ep, const float* sfeat, long ldf, const float* qfeat, long ldq, long feat_ep_rows, int D,
                                const int32_t* support_y, int n_way, int k_shot, int N, int n_query_pts, int method,
                                float scaler, float* Z, float* ws, long ws_words, void* stream);
int r3d_protonet_head_bwd(int n_ep, const float* qfeat, long ldq, long feat_ep_rows, int D, const int32_t* support_y, int n_way,
                          int k_shot, int N, int n_query_pts, int method, float scaler, const float* dZ, float* dsfeat,
                          long ldds, float* dqfeat, long lddq, long dfeat_ep_rows, float* ws, long ws_words, void* stream);

/* ---- mIoU accumulator (eval_noise.py:23-72): hist (3, n_classes) uint64 = GT | predicted | TP, ADDED to what hist holds.
 * lut (n_lut) int32: test-class index of an episode label (0 = background).  A label or prediction outside [0, n_lut) is
 * CLAMPED into the table -- negative to entry 0, too large to entry n_lut - 1 -- before the look-up; a true positive is
 * gt == pred before clamping, counted under the ground truth's entry.  Every lut entry must lie in [0, n_classes). */
int r3d_miou_accumulate(const int32_t* pred, const int64_t* gt, long n, const int32_t* lut, int n_lut, int n_classes,
                        uint64_t* hist, void* stream);

/* ---- Training augmentation of prepared clouds (dataloaders/loader.py:205-213,354-373: --pc_augm) ----
 * A prepared cloud holds the min-shifted xyz in channels xyz_ch..xyz_ch+2 -- the array the reference hands to
 * augment_pointcloud -- so for each of B clouds of N points and C channels (3, 6 or 9):
 *   xyz' = xyz . M^T + jitter,  M = Mirror_y . Mirror_x . Rot_z(angle) . (s I)  (row-major 3 x 3; loader.py:356-368):
 *     s uniform in [1/scale, scale] when scale > 1, angle uniform in [0, 2 pi) when rot == 1, each mirror with
 *     probability mirror_prob / 2 when mirror_prob > 0;
 *   jitter = clip(0.01 normal, -0.05, 0.05) on the three xyz channels when jitter != 0        (loader.py:370-372);
 *   XYZ' = (xyz' - min_n xyz') / max_n (xyz' - min_n xyz') per axis, IEEE division, into channels XYZ_ch..XYZ_ch+2
 *     (XYZ_ch = -1: the cloud has none; an axis of zero extent gives NaN as the reference's division does) (loader.py:209-213);
 *   every other channel is copied.
 * x and out are addressed as p[b * sb + c * sc + n * sn] (strides in floats): contiguous channel-major (B, C, N) is
 * (C N, N, 1), point-major rows viewed as (B, C, N) are (N C, 1, C).  out == x (same strides) is allowed and gives the
 * bits of the out-of-place call; any other overlap is the caller's error.
 * Randomness is stateless: all a cloud draws is a function of (seed + *seed_dev, first_key + b), the jitter of
 * (point, axis) besides; seed_dev (may be NULL) is a device word added to seed, so that a frozen launch sequence
 * advances without re-capture (as r3d_attention_fwd_train).  The normal draws are this library's, not numpy's.
 * Optional (NULL: absent): mats (B, 9) matrices to use instead of drawing them; noise (B, N, 3) jitter to add instead of
 * generating it (used whatever `jitter` says); mats_out (B, 9) receives the matrix each cloud used.
 * One 256-thread workgroup per cloud; min / max reductions only, so results are bit-reproducible. */
int r3d_augment_clouds(const float* x, long x_sb, long x_sc, long x_sn, float* out, long o_sb, long o_sc, long o_sn, int B,
                       int C, int N, int xyz_ch, int XYZ_ch, float scale, int rot, float mirror_prob, int jitter,
                       unsigned seed, const unsigned* seed_dev, unsigned first_key, const float* mats, const float* noise,
                       float* mats_out, void* stream);

/* ---- Labelling a whole scan against a fitted support set (no reference counterpart: the reference scores clouds its
 * loader cut on the host, dataloaders/loader.py:100-119; definition in INTEGRATION.md, "Labelling a scan", steps 1-9') ----
 * scan: M rows of ld floats, x y z first (r g b behind them when ld >= 6); M <= R3D_SCENE_MAX_POINTS.  A point is VALID when x, y and z
 * are finite.  Nothing here draws a random number or sums floats in an order that depends on scheduling.
 *
 *   entry point          what it does                                                         host reads afterwards
 *   r3d_scene_bounds     rec[0..3] = min x, min y, max x, max y over the valid points (fp32),  rec (read 1 of 2)
 *                        rec[4] = their count (int32 bits); ws: r3d_scene_bounds_ws_words(M)
 *   r3d_scene_plan       cell keys cy * ncx + cx with cx = (int)floorf((x - x0) / s) (IEEE         the plan record
 *                        subtraction and division); stable 8-bit LSD radix sort of the valid points (read 2 of 2)
 *                        by key (per-tile digit counts, one scan, in-tile ranking in index order);
 *                        cell offsets; points per block; chunks per block (ceil(n / N), 0 below
 *                        min_points) and their exclusive scan; the chunk table; the plan record
 *                        {n_chunks, kept blocks, valid points with a vote, blocks, run chunks =
 *                        n_chunks, skipped chunks = 0, valid points with a vote again, 0}
 *   r3d_scene_run_tables optional, after r3d_scene_plan and before the host reads the plan record:  -
 *                        with cap c = max_chunks >= 1, chunk j of a block with nc chunks RUNS when
 *                        j < c.  Writes into sws the exclusive scan of min(nc, c) over the blocks (first
 *                        run chunk of a block) and the block of every run chunk, and into the plan
 *                        record rec[4] = run chunks, rec[5] = skipped chunks, rec[6] = valid points
 *                        with a vote under the cap.
 *   r3d_scene_prepare    run chunks first_chunk .. first_chunk + G - 1 as prepared clouds of N slots -
 *                        (slot t = member t mod len of the chunk): xyz - min over the slots,
 *                        rgb / 255.0f at rgb_ch (3 or -1), xyz' / max xyz' at XYZ_ch (behind them, or
 *                        -1; an axis of zero extent gives 0), written at out[g * o_sb + c * o_sc +
 *                        t * o_sn] (the strides of r3d_augment_clouds); slot_map (G, N) int32,
 *                        optional: the scan index of every slot.  Chunks past the record's run
 *                        chunks are left unwritten.
 *   r3d_scene_vote       per scan point the fp32 sum of logits[run chunk][class][slot] over its      -
 *                        appearances in chunks that ran, block id ascending then slot ascending, one
 *                        at a time; labels = arg-max (lowest class on ties, -1 without a vote),
 *                        votes = the appearance count.  logits: (n_chunks, n_classes, N), run-chunk
 *                        order.  The appearances are computed from the point's cell, its rank in the
 *                        cell list and the block's cell offsets: no inverted index in memory, no
 *                        atomics.
 *   r3d_scene_transfer   after a vote: every valid point p with votes[p] == 0 takes scores and     word 0 of the
 *                        label of the voted point q with the smallest d = (dx * dx + dy * dy) +     sparse record:
 *                        dz * dz (fp32, dx = x_q - x_p, every operation rounded on its own; +inf is  receivers that
 *                        a value like any other), the lowest scan index on equal d, among the voted  found a source
 *                        points of the 3 x 3 cells around p's cell (clipped at the grid).  source
 *                        (M,) int64 = q for such a point (votes[p] stays 0), p itself for a voted
 *                        point, -1 for an invalid point or one that found no candidate, which is
 *                        left as the vote left it.  Voted points go, in sorted order, into packed
 *                        rows {x, y, z, index}; the others into a list per cell, cut into tiles of
 *                        256 queries (R3D_SCENE_TRANSFER_QUERY_TILE); one workgroup per tile stages the
 *                        candidate runs of the three cell rows through LDS, 1024 rows at a time
 *                        (R3D_SCENE_TRANSFER_CAND_TILE), one thread per query keeping the
 *                        lexicographic minimum of (d, index): no float is summed across threads, the
 *                        one atomic is an integer count.
 *
 * sws of r3d_scene_prepare and r3d_scene_vote: NULL with sws_words 0 means NO CAP -- every chunk runs, run chunk c is
 * chunk c, and the plan's own chunk tables serve as the run tables --; else the sparse workspace that
 * r3d_scene_run_tables filled.  A run chunk is still chunk (b, j) of nc: same members, same len; with a cap that skips
 * nothing both give the bits of the call without sws.  NULL with sws_words != 0 is refused.
 * neighbours and weights of r3d_scene_transfer: both NULL is the transfer above ("nearest"); both given is step 9' ("idw"),
 * the same receivers, candidates, d, checks and launch sequence with another reduction per receiver: q0, q1, q2 = the
 * three smallest candidates in (d, scan index) order (fewer when there are fewer), w_i = 1.0f / (d_i + 1e-8f) (+inf gives
 * 0), m_i[k] = scores[q_i][k] / (float)votes[q_i], and per class acc = w_0 m_0; acc += w_1 m_1; acc += w_2 m_2;
 * scores[p][k] = acc / ((w_0 + w_1) + w_2), or m_0[k] when that sum is 0; every operation an IEEE one rounded on its own.
 * labels[p] = the arg-max (lowest class on ties), source[p] = q0, votes[p] stays 0.  neighbours (M, 3) int64: q0 q1 q2
 * (-1: missing) for a receiver, {p, -1, -1} for a voted point, else -1; weights (M, 3) fp32: the w_i (0: missing),
 * {1, 0, 0} for a voted point, else 0.  A receiver's scores are on the scale of mean logits, a voted point's stay sums
 * over its votes.  Each thread keeps its three pairs sorted in registers; a candidate costs one comparison against the
 * third, the insertion sits behind that branch.  One of the two without the other is refused.
 *
 * Blocks: r x r cells (1 <= r <= 4), block (bx, by) covers cells bx .. min(bx + r, ncx) - 1 by by .. min(by + r, ncy) - 1,
 * nbx = max(ncx - r + 1, 1); its point list is its cells' lists by (cy, cx), never materialised.  ncx * ncy <= R3D_SCENE_MAX_CELLS.
 * ws: ONE int32 scratch of r3d_scene_ws_words(M, ncx, ncy, chunk_cap) words (-1: shape out of range) shared by all of
 * them, which must be called with the same (M, ncx, ncy, r, N, chunk_cap); chunk_cap bounds the chunk table
 * (r * r * n_valid / N + blocks is always enough).  r3d_scene_ws_offsets fills 8 HOST words (the one host pointer of this
 * header) with the word offsets of {sorted scan indices, sorted keys, sorted position of a scan point, cell offsets
 * (ncx * ncy + 2), points per block, first chunk of a block (blocks + 1), block of a chunk, plan record (8)}.
 * sws: a SECOND int32 scratch of r3d_scene_sparse_ws_words(M, ncx, ncy, chunk_cap) words (-1: shape out of range), for
 * the same (M, ncx, ncy, chunk_cap) as ws, needed by the cap and by the transfer only; a shorter one is refused.
 * r3d_scene_sparse_ws_offsets fills 8 HOST words with the word offsets of {first run chunk of a block (blocks + 1), block
 * of a run chunk, voted points in front of a sorted position (M + 1), scan indices of the points without a vote, first
 * query tile of a cell (ncx * ncy + 1), candidate rows (4 * M), sparse record (8), scan partials}. */
#define R3D_SCENE_MAX_POINTS (1L << 27) /* rows of a scan, for every entry point that takes one */
#define R3D_SCENE_MAX_CELLS 65536
#define R3D_SCENE_TRANSFER_QUERY_TILE 256
#define R3D_SCENE_TRANSFER_CAND_TILE 1024
long r3d_scene_bounds_ws_words(long M);
int r3d_scene_bounds(const float* scan, int ld, long M, float* rec /* 8 words */, float* ws, long ws_words, void* stream);
long r3d_scene_ws_words(long M, int ncx, int ncy, long chunk_cap);
int r3d_scene_ws_offsets(long M, int ncx, int ncy, long chunk_cap, long* out);
long r3d_scene_sparse_ws_words(long M, int ncx, int ncy, long chunk_cap);
int r3d_scene_sparse_ws_offsets(long M, int ncx, int ncy, long chunk_cap, long* out);
int r3d_scene_plan(const float* scan, int ld, long M, float x0, float y0, float s, int ncx, int ncy, int r, int N,
                   int min_points, long chunk_cap, int32_t* ws, long ws_words, void* stream);
int r3d_scene_run_tables(long M, int ncx, int ncy, int r, int N, long chunk_cap, int32_t* ws, long ws_words, int max_chunks,
                         int32_t* sws, long sws_words, void* stream);
int r3d_scene_prepare(const float* scan, int ld, long M, int ncx, int ncy, int r, int N, long chunk_cap, const int32_t* ws,
                      long ws_words, const int32_t* sws, long sws_words, int first_chunk, int G, int C, int rgb_ch,
                      int XYZ_ch, float* out, long o_sb, long o_sc, long o_sn, int32_t* slot_map, void* stream);
int r3d_scene_vote(long M, int ncx, int ncy, int r, int N, long chunk_cap, const int32_t* ws, long ws_words,
                   const int32_t* sws, long sws_words, const float* logits, int n_chunks, int n_classes, float* scores,
                   int64_t* labels, int32_t* votes, void* stream);
int r3d_scene_transfer(const float* scan, int ld, long M, int ncx, int ncy, long chunk_cap, const int32_t* ws, long ws_words,
                       int32_t* sws, long sws_words, int n_classes, float* scores, int64_t* labels, const int32_t* votes,
                       int64_t* source, int64_t* neighbours, float* weights, void* stream);

/* ---- predict_scene_sets: one scan against several support sets ("Labelling a scan against several support
 * sets", step 10).
 * r3d_scene_merge_sets: scores (M, n_sets, n_classes) fp32 -- what r3d_scene_vote and r3d_scene_transfer leave for logits
 * whose columns are set after set, n_classes = n_way + 1 >= 2 each, n_sets * n_classes <= 64 --, votes (M,), source (M,)
 * of a transfer or NULL.  One thread per point, no atomics, nothing summed.  A point HAS A LABEL when votes[p] > 0 or
 * (source given) source[p] >= 0; any other point gets set_labels -1, labels -1, set_of -1, margin 0.  Per set k of a point
 * with a label: l_k = the arg-max of its n_classes scores with the comparison of r3d_scene_vote (lowest class on ties; one
 * device function serves both kernels), set_labels[p][k] = l_k; with l_k >= 1 the set CLAIMS p with the margin m_k =
 * s[l_k] - s[r], r the arg-max over the classes other than l_k by the same comparison -- one IEEE fp32 subtraction; a NaN
 * margin does not claim.  The claim with the greatest margin wins, the lowest k on equal margins: labels[p] =
 * classes[k * (n_classes - 1) + l_k - 1] (classes: n_sets * n_way int32 on the device), set_of[p] = k, margin[p] = m_k.
 * Without a claim labels[p] = background, set_of[p] = -1, margin[p] = 0.  set_labels (M, n_sets) and labels (M,) int64,
 * set_of (M,) int32, margin (M,) fp32. */
int r3d_scene_merge_sets(long M, int n_sets, int n_classes, const float* scores, const int32_t* votes, const int64_t* source,
                         const int32_t* classes, long background, int64_t* set_labels, int64_t* labels, int32_t* set_of,
                         float* margin, void* stream);

/* ---- fit_scene: the support set from an annotated scan ("Fitting from an annotated scan", S1-S5).
 * All three run after r3d_scene_plan (no cap) on its ws, with the same (M, ncx, ncy, r, N, chunk_cap).  The CLOUD of a kept
 * block of n points and nc = ceil(n / N) chunks is its chunk 0: list positions 0, nc, 2 nc, ..., len = ceil(n / nc) members,
 * slot t = member t mod len.
 * labels: M class ids, int32 (label_bytes 4) or int64 (8), read as they are; the labels of invalid points are never read.
 *
 *   entry point               what it does
 *   r3d_scene_support_counts  fg (blocks, n_way) int32: fg[b][w] = the members of block b's cloud whose label equals
 *                             classes[w] (a device array of n_way <= R3D_SCENE_SUPPORT_MAX_WAYS int32 ids), every member once; 0 for a dropped
 *                             block.  One workgroup per block, a ballot and a population count per wave and way, the
 *                             waves' integer counts summed in LDS.
 *   r3d_scene_support_pick    thr[b] = max((int)floorf((float)len * min_ratio), min_fg), one IEEE fp32 multiplication;
 *                             a kept block is ELIGIBLE for way w when fg[b][w] > thr[b].  shot_block / shot_fg (n_way,
 *                             k_shot) int32: way w's eligible blocks by fg descending, then block id ascending, the first
 *                             k_shot (a missing one: block -1, fg 0); rec (8 words): rec[w] = eligible blocks of way w.
 *                             One workgroup per way, per shot one maximum of (fg << 32) | (0xFFFFFFFF - b) below the last.
 *   r3d_scene_prepare_blocks  r3d_scene_prepare for a device list of G block ids: cloud g is chunk 0 of blocks[g], with
 *                             that entry point's bits, strides and slot_map; a block id outside the grid or a dropped
 *                             block leaves its cloud unwritten.  With labels, cloud_class (G int32 ids) and mask (G, N)
 *                             int32 -- all three or none --: mask[g][t] = (labels[slot_map[g][t]] == cloud_class[g]). */
#define R3D_SCENE_SUPPORT_MAX_WAYS 7
int r3d_scene_support_counts(long M, int ncx, int ncy, int r, int N, long chunk_cap, const int32_t* ws, long ws_words,
                             const void* labels, int label_bytes, const int32_t* classes, int n_way, int32_t* fg,
                             void* stream);
int r3d_scene_support_pick(long M, int ncx, int ncy, int r, int N, long chunk_cap, const int32_t* ws, long ws_words,
                           const int32_t* fg, int n_way, int k_shot, float min_ratio, int min_fg, int32_t* shot_block,
                           int32_t* shot_fg, int32_t* rec, void* stream);
int r3d_scene_prepare_blocks(const float* scan, int ld, long M, int ncx, int ncy, int r, int N, long chunk_cap,
                             const int32_t* ws, long ws_words, const int32_t* blocks, int G, int C, int rgb_ch, int XYZ_ch,
                             float* out, long o_sb, long o_sc, long o_sn, int32_t* slot_map, const void* labels,
                             int label_bytes, const int32_t* cloud_class, int32_t* mask, void* stream);

/* ---- pool_segments: one label per user-given segment of the scan ("Pooling scores over segments", P1-P5).
 * Replaces what a caller would write in torch as a sort plus index_add_ -- floating-point atomics, a summation order that
 * changes from run to run -- with sums in a defined order: the reference has no such step, the definition is this project's.
 * segments: M ids, int32 (seg_bytes 4) or int64 (8), read as they are; g < 0: the point is in no segment; legal ids are
 * 0 .. 2^31 - 2.  ws: ONE int32 scratch of r3d_scene_seg_ws_words(M) words (-1: M outside 1 .. R3D_SCENE_MAX_POINTS) shared
 * by the four calls of one pooling; its first R3D_SCENE_SEG_REC words are the record the host reads, R3D_SEG_R_*:
 *   MAX1 largest legal id + 1 (0: none)   NNEG negative ids   NBAD ids >= 2^31 - 1   BADMAX the largest of those (uint64, two
 *   words)   S segments   NCONTRIB contributors   NTILES tiles   NPOOLED pooled points   NFILLED pooled points whose label
 *   was -1   NUNLAB labels that are -1 in the result
 *
 *   entry point           what it does                                                                   host reads
 *   r3d_scene_seg_ids     zeroes the record, then MAX1 .. BADMAX of it (integer maxima and counts)        MAX1 .. BADMAX
 *   r3d_scene_seg_group   max_id, n_negative: MAX1 (less one) and NNEG as read.  Stable LSD radix sort of
 *                         (id, scan index), the kernels of r3d_scene_plan, 8 bits a pass up to the highest
 *                         set bit of the largest key (1 .. 4 passes); a negative id sorts under the key
 *                         max_id + 1.  CONTRIBUTOR: a point in a segment with votes > 0.  Segment rows are in
 *                         ascending id order; segment_index (M,) int32: the row of a point's segment, -1
 *                         without one.  Contributors of a segment by ascending scan index, cut into TILES
 *                         of R3D_SCENE_SEG_TILE ranks; tiles never span two segments.                    S .. NTILES
 *   r3d_scene_seg_pool    n_segments, n_tiles: S and NTILES as read; part: n_tiles * n_cols floats of
 *                         scratch.  Row of contributor p: c[j] = scores[p][j] / (float)votes[p].  Tile:
 *                         part = c of its first rank, then += the next, one fp32 addition at a time; segment:
 *                         tot = its first tile's part, then += the next; seg_scores = tot / (float)members,
 *                         zeros without a member.  seg_labels (may be NULL): the arg-max with the comparison
 *                         of r3d_scene_vote, -1 without a member.  seg_ids (S,) int64, seg_points (every
 *                         point with the id) and seg_members (contributors) (S,) int32.  One wave per tile,
 *                         rows staged in LDS, lane j adds column j; one wave per segment.  No float atomics.  -
 *   r3d_scene_seg_spread  point p with segment_index s >= 0 and seg_members[s] >= min_members is POOLED: it
 *                         takes seg_scores[s], seg_labels[s] and, with n_sets > 0 (then the set fields are
 *                         needed, else NULL), seg_set_labels / seg_set_of / seg_margin; any other point the
 *                         in_* fields of its own row.  pooled (M,) bytes 0 / 1.  One thread per point decides,
 *                         the workgroup copies the rows; one integer atomic per count and workgroup.    NPOOLED .. NUNLAB
 * n_cols <= R3D_SCENE_SCORE_COLS_MAX wherever a call takes score rows. */
#define R3D_SCENE_SEG_REC 16
#define R3D_SEG_R_MAX1 0
#define R3D_SEG_R_NNEG 1
#define R3D_SEG_R_NBAD 2
#define R3D_SEG_R_BADMAX 4
#define R3D_SEG_R_S 6
#define R3D_SEG_R_NCONTRIB 7
#define R3D_SEG_R_NTILES 8
#define R3D_SEG_R_NPOOLED 9
#define R3D_SEG_R_NFILLED 10
#define R3D_SEG_R_NUNLAB 11
#define R3D_SCENE_SEG_TILE 256
#define R3D_SCENE_SCORE_COLS_MAX 64
long r3d_scene_seg_ws_words(long M);
int r3d_scene_seg_ids(const void* segments, int seg_bytes, long M, int32_t* ws, long ws_words, void* stream);
int r3d_scene_seg_group(const void* segments, int seg_bytes, long M, const int32_t* votes, long max_id, long n_negative,
                        int32_t* segment_index, int32_t* ws, long ws_words, void* stream);
int r3d_scene_seg_pool(long M, int n_cols, const float* scores, const int32_t* votes, long n_segments, long n_tiles,
                       const int32_t* ws, long ws_words, float* part, int64_t* seg_ids, int32_t* seg_points,
                       int32_t* seg_members, float* seg_scores, int64_t* seg_labels, void* stream);
int r3d_scene_seg_spread(long M, int n_cols, int n_sets, long n_segments, int min_members, const int32_t* segment_index,
                         const int32_t* seg_members, const float* seg_scores, const int64_t* seg_labels,
                         const int64_t* seg_set_labels, const int32_t* seg_set_of, const float* seg_margin,
                         const float* in_scores, const int64_t* in_labels, const int64_t* in_set_labels,
                         const int32_t* in_set_of, const float* in_margin, float* scores, int64_t* labels, uint8_t* pooled,
                         int64_t* set_labels, int32_t* set_of, float* margin, int32_t* ws, long ws_words, void* stream);

/* ---- build_segments: the segments of r3d_scene_seg_* grown from the scan itself ("Building segments",
 * G1-G7).  Additive: no entry point above changes.  The reference reads segment ids that an offline script wrote
 * (dataloaders/loader.py:339-349); the definition is this project's.  A VALID point has finite x y z.  Voxel of a valid
 * point: i_a = (int)floorf((v_a - v0_a) / voxel) per axis, v0 the minima read from the record, key = (iz * ny + iy) * nx +
 * ix, nx, ny, nz <= R3D_SCENE_GROW_AXIS the host's counts from the same arithmetic at the maxima.  ws: ONE int32 scratch of
 * r3d_scene_grow_ws_words(M) words (-1: M outside 1 .. R3D_SCENE_MAX_POINTS) shared by the calls of one build, which pass the
 * same M and nx, ny, nz; its first R3D_SCENE_GROW_REC words are the record the host reads, R3D_GROW_R_*:
 *   MIN min x y z, MAX max x y z (three words of float bits each)   NVALID valid points   V occupied voxels   NCOMP components
 *   S kept components   NDROPPED points of dropped components   ERROR != 0: a bounded loop of the union-find ran out
 *   ABSORBED_VOXELS, ABSORBED_POINTS (r3d_scene_grow_absorb; 0 without it)
 *
 *   entry point                what it does                                                              host reads
 *   r3d_scene_grow_bounds      MIN .. NVALID of the record, zeros in the others (r3d_scene_bounds keeps no z
 *                              and stays as it is)                                                       MIN .. NVALID
 *   r3d_scene_grow_sort        keys (an invalid point: nx ny nz), the stable LSD radix sort of
 *                              r3d_scene_plan on (key, scan index), 8 bits a pass up to the highest set bit
 *                              of nx ny nz; the first sorted position of every voxel as a flag, their scan   V
 *   r3d_scene_grow_voxels      n_valid, n_voxels: NVALID and V as read.  The voxel table: rows in ascending
 *                              key order, a row's points by ascending scan index; voxel_index (M,) int32: the
 *                              row of a point's voxel, -1 for an invalid point.  voxel_mean (V, 3) fp32 or
 *                              NULL (no colour; else ld >= 6): the mean of columns 3 .. 5 per voxel, summed as
 *                              r3d_scene_seg_pool sums a segment whose points all have one vote: ranks in
 *                              tiles of 256, part = the first row, += the next, tot = the first tile's part,
 *                              += the next, tot / (float)count.                                              -
 *   r3d_scene_grow_union       parent[v] = v, then one thread per voxel a and the offsets (dx, dy, dz) with a
 *                              larger key (3 for connectivity 6, 13 for 26): the neighbour's coordinates are
 *                              checked against 0 .. n - 1 per axis, its key found by binary search among the
 *                              rows behind a; with voxel_mean (else NULL) the pair is joined only when
 *                              |mean_c(a) - mean_c(b)| <= colour_tol for c = r, g, b (fp32; a NaN joins
 *                              nothing).  A joined pair is united by lock-free hooking: both roots found
 *                              (path halving by atomicMin), the larger root compare-and-swapped onto the
 *                              smaller, a failed swap goes on from the value it returned.  parent[v] <= v throughout; only agent-scope atomics
 *                              touch parent[]; no thread waits; a find is bounded by V links and a unite by
 *                              V + 1 attempts, an overrun sets ERROR and returns.                            -
 *   r3d_scene_grow_components  root[v] = the root of v (the smallest row of its component), a launch of its
 *                              own; points per root by integer atomics (the lanes of a wave that share a root
 *                              add first); a root is KEPT when its component has at least min_points points;
 *                              the kept roots' scan.                                                     NCOMP, S, ERROR
 *   r3d_scene_grow_absorb      only with absorb > 0 (G6a), between components and ids; rings 1 .. R3D_SCENE_GROW_RINGS, voxel_ring
 *                              (V,) int32 the caller's.  owner[v] = root[v] where that root is kept, else -1 (v is
 *                              FREE); voxel_ring[v] = 0, or -1 for a free voxel.  Then `rings` launches, one thread
 *                              per voxel, each reading one owner table and writing the other (a voxel taken in
 *                              round r is seen from round r + 1 on): a voxel with an owner copies it; a free one
 *                              finds its occupied neighbours at all 6 or 26 offsets as r3d_scene_grow_normals does
 *                              (coordinates checked against 0 .. n - 1 per axis, one binary search per (dz, dy)), no
 *                              colour and no normal test, and takes the owner that most of the neighbours with an
 *                              owner have, the smallest on a tie, voxel_ring[v] = the round; none: it stays free.
 *                              A last launch sets root[v] = owner[v] for the absorbed voxels and adds their points
 *                              to the owner's count by integer atomics (the lanes of a wave that share an owner add
 *                              first).  The tables lie in the workspace (the index array of the pair the sort left
 *                              free, and parent[], dead after components); no atomics touch them, no thread waits.
 *                              S and the ids of r3d_scene_grow_ids are unchanged: only -1s become ids.        ABSORBED_*
 *   r3d_scene_grow_ids         n_segments: S as read.  Kept components are numbered 0 .. S - 1 by
 *                              ascending root; segments (M,) int32: that number, -1 for an invalid point
 *                              or a dropped component; segment_points (S,) int32 (NULL with S = 0).          NDROPPED, ABSORBED_*
 * No float atomics: the component of a voxel depends on the joined pairs alone, so the same scan gives the same bits.
 *
 * With normal_tol (G3c, G3n and the normal test of G4) two launches go between voxels and the union, and the union is
 * r3d_scene_grow_union_normals; without it none of the three is called.  Every operation below is fp32 and rounded on its
 * own (__fadd_rn, __fsub_rn, __fmul_rn, __fdiv_rn; nothing is contracted).  The three tables are the caller's, the
 * workspace and its size are as above.
 *   r3d_scene_grow_centroids   x0 y0 z0, voxel, the grid: those of the sort.  voxel_centroid (V, 3) fp32: per voxel the
 *                              mean of u_a = (v_a - v0_a) - (float)i_a * voxel over its points, i decoded from the
 *                              voxel's key (the offset inside the voxel: second moments do not cancel against the
 *                              room's extent), summed as voxel_mean: ascending scan index in tiles of 256, part = the
 *                              first, += the next, the parts in tile order, one division by (float)count.
 *   r3d_scene_grow_normals     one thread per voxel v and the offsets o = 0 .. 26 = (dz, dy, dx) in lexicographic
 *                              order over -1, 0, 1 (13: v itself), whatever the connectivity.  A neighbour is
 *                              occupied when its coordinates lie in the grid and its key is in the table: per (dz,
 *                              dy) one binary search for the first x-neighbour inside the grid, the next rows of the
 *                              table checked by key.  voxel_support (V,) int32: k, the occupied offsets, 1 .. 27.
 *                              q_o[a] = (float)d_a * voxel + centroid[b_o][a]; m = (q_first + q_next + ...) /
 *                              (float)k by ascending o; e_o = q_o - m; C = sum_o e_o e_o^T, entries 00 01 02 11 12
 *                              22, each the rounded products added by ascending o, the first starts the sum.
 *                              voxel_normal (V, 3) fp32: three NaNs when k < 4, an entry of C is not finite or s =
 *                              max(C00, C11, C22) is not > 0.  Else B = C / s, t = (B00 + B11) + B22, A = t I - B
 *                              (off-diagonal -Bij), then eight times N = A A with every entry (x y + x' y') + x'' y''
 *                              in the index order of the product, A = N / max(N00, N11, N22); the row of A with the
 *                              largest diagonal entry (the lowest on a tie): not of unit length, that entry is 1.
 *   r3d_scene_grow_union_normals  r3d_scene_grow_union (same kernel, same arguments, voxel_mean may be NULL) where a
 *                              pair a, b is joined only when also dot * dot >= (cos2 * la) * lb, dot = (na0 nb0 +
 *                              na1 nb1) + na2 nb2, la and lb the same of a row with itself; 0 <= cos2 <= 1.  No
 *                              square root, no normalisation, the sign of a row does not matter; a NaN makes the
 *                              comparison false, so a voxel without a normal joins nothing; a row of zeros reads
 *                              0 >= 0 and joins (r3d_scene_grow_normals writes none). */
#define R3D_SCENE_GROW_REC 16
#define R3D_SCENE_GROW_AXIS 1024 /* voxels per axis: keys stay below 2^30 */
#define R3D_SCENE_GROW_RINGS 64
#define R3D_GROW_R_MIN 0
#define R3D_GROW_R_MAX 3
#define R3D_GROW_R_NVALID 6
#define R3D_GROW_R_V 7
#define R3D_GROW_R_NCOMP 8
#define R3D_GROW_R_S 9
#define R3D_GROW_R_NDROPPED 10
#define R3D_GROW_R_ERROR 11 /* bit 0 a find, bit 1 a unite */
#define R3D_GROW_R_ABSORBED_VOXELS 12
#define R3D_GROW_R_ABSORBED_POINTS 13
long r3d_scene_grow_ws_words(long M);
int r3d_scene_grow_bounds(const float* scan, int ld, long M, int32_t* ws, long ws_words, void* stream);
int r3d_scene_grow_sort(const float* scan, int ld, long M, float x0, float y0, float z0, float voxel, int nx, int ny, int nz,
                        int32_t* ws, long ws_words, void* stream);
int r3d_scene_grow_voxels(const float* scan, int ld, long M, int nx, int ny, int nz, long n_valid, long n_voxels,
                          int32_t* voxel_index, float* voxel_mean, int32_t* ws, long ws_words, void* stream);
int r3d_scene_grow_union(long M, int nx, int ny, int nz, long n_voxels, int connectivity, const float* voxel_mean,
                         float colour_tol, int32_t* ws, long ws_words, void* stream);
int r3d_scene_grow_centroids(const float* scan, int ld, long M, float x0, float y0, float z0, float voxel, int nx, int ny,
                             int nz, long n_voxels, float* voxel_centroid, const int32_t* ws, long ws_words, void* stream);
int r3d_scene_grow_normals(long M, int nx, int ny, int nz, long n_voxels, float voxel, const float* voxel_centroid,
                           float* voxel_normal, int32_t* voxel_support, const int32_t* ws, long ws_words, void* stream);
int r3d_scene_grow_union_normals(long M, int nx, int ny, int nz, long n_voxels, int connectivity, const float* voxel_mean,
                                 float colour_tol, const float* voxel_normal, float cos2, int32_t* ws, long ws_words,
                                 void* stream);
int r3d_scene_grow_components(long M, long n_voxels, int min_points, int32_t* ws, long ws_words, void* stream);
int r3d_scene_grow_absorb(long M, int nx, int ny, int nz, long n_voxels, int connectivity, int rings, int32_t* voxel_ring,
                          int32_t* ws, long ws_words, void* stream);
int r3d_scene_grow_ids(long M, long n_voxels, long n_segments, const int32_t* voxel_index, int32_t* segments,
                       int32_t* segment_points, int32_t* ws, long ws_words, void* stream);

/* ---- extract_objects: object instances from a labelled scan ("Objects from a labelled scan", O1-O8).
 * Additive: no entry point above changes.  The reference has no such function; the definition is this project's.
 * labels (M,): int32 (labels64 = 0) or int64 (labels64 = 1); ignore: n_ignore <= R3D_SCENE_OBJ_IGNORE int64 class ids on the
 * device (NULL with n_ignore = 0).  A point TAKES PART when x y z are finite, its label is >= 0 and not in ignore.  The grid is
 * the one of build_segments (origin: the minima over the finite points).  A UNIT is the set of participating points of one
 * class in one cell; key = label * n_cells + cell, n_cells = nx ny nz, n_labels the largest participating label plus one (a
 * label <= R3D_SCENE_OBJ_LABEL), n_labels * n_cells <= R3D_SCENE_OBJ_KEY (the key of every other point; it sorts last).  ws:
 * ONE int32 scratch of r3d_scene_obj_ws_words(M) words (-1: M outside 1 .. R3D_SCENE_MAX_POINTS) shared by the calls of one
 * extraction, laid out as that of build_segments; its first R3D_SCENE_GROW_REC words are the record the host reads: the words
 * R3D_GROW_R_MIN .. ERROR of build_segments (NVALID finite points, V units U) and four of its own, R3D_OBJ_R_*:
 *   NLABELS n_labels   NUNLABELLED finite points left out by their label   NOVER finite points whose label is above
 *   R3D_SCENE_OBJ_LABEL and not ignored (no key holds them: the host raises)   NPOINTS participating points
 *
 *   entry point                what it does                                                              host reads
 *   r3d_scene_obj_bounds       r3d_scene_grow_bounds, then the four R3D_OBJ_R_* by integer atomics         MIN .. NVALID, OBJ_R_*
 *   r3d_scene_obj_sort         x0 y0 z0, the grid: from MIN and MAX as build_segments derives them; n_labels, n_points:
 *                              NLABELS and NPOINTS as read.  Keys, the stable LSD radix sort on (key, scan index), 8 bits a
 *                              pass up to the highest set bit of n_labels n_cells, the first sorted position of every
 *                              unit as a flag, their scan, the unit table (rows in ascending key order, a row's points by
 *                              ascending scan index); unit_index (M,) int32: the row of a point's unit, -1 for a point
 *                              that takes no part.                                                       V
 *   r3d_scene_obj_union        parent[u] = u, then one thread per unit a and the offsets (dx, dy, dz) with a larger cell
 *                              key (3 for connectivity 6, 13 for 26): the neighbour's coordinates are checked against
 *                              0 .. n - 1 per axis, then its key is formed with a's class and found by binary search among
 *                              the rows behind a; a pair found is united as r3d_scene_grow_union unites (the same device
 *                              functions; only agent-scope atomics touch parent[]; an overrun sets ERROR).     -
 *   r3d_scene_obj_components   the launches of r3d_scene_grow_components on the unit table.               NCOMP, S, ERROR
 *   r3d_scene_obj_stats        n_objects = S >= 1: S as read.  Per object s (kept components by ascending root, so by
 *                              ascending class, then smallest cell key): object_labels (S,) int64; object_points (S,)
 *                              int32; object_units (S,) int32; object_lo, object_hi (S, 3) fp32: the minima and maxima of
 *                              its points' coordinates, exact, -0.0 below +0.0; object_centroid (S, 3) fp32: per axis
 *                              v0 + voxel * ((sum / n) + 0.5) / 256 in float64 in that order, rounded once, sum the int64
 *                              sum over its points of u = (int)floorf(((v - v0) / voxel) * 256.0f) (fp32, each operation
 *                              rounded, clamped to 0 .. 256 n_axis - 1).  object_sums (S, 3) int64: the caller's scratch.
 *                              One thread per unit reduces its points; the units of a wave that share an object are
 *                              combined by shuffles; per wave and object 6 atomic min / max on the order-preserving
 *                              integer image of the float bits, 3 64-bit atomic adds and 1 atomic add.        -
 *   r3d_scene_obj_ids          objects (M,) int32: the number of the point's object, -1 for a point that takes no part
 *                              or a dropped component (r3d_scene_grow_ids' launch).                         NDROPPED, ERROR
 * No float goes through an atomic: the same scan and labels give the same bits. */
#define R3D_SCENE_OBJ_IGNORE 64
#define R3D_SCENE_OBJ_LABEL 2147483646L /* n_labels = label + 1 fits an int */
#define R3D_SCENE_OBJ_KEY 2147483647L
#define R3D_OBJ_R_NLABELS 12
#define R3D_OBJ_R_NUNLABELLED 13
#define R3D_OBJ_R_NOVER 14
#define R3D_OBJ_R_NPOINTS 15
long r3d_scene_obj_ws_words(long M);
int r3d_scene_obj_bounds(const float* scan, int ld, long M, const void* labels, int labels64, const int64_t* ignore, int n_ignore,
                         int32_t* ws, long ws_words, void* stream);
int r3d_scene_obj_sort(const float* scan, int ld, long M, const void* labels, int labels64, const int64_t* ignore, int n_ignore,
                       float x0, float y0, float z0, float voxel, int nx, int ny, int nz, int n_labels, long n_points,
                       int32_t* unit_index, int32_t* ws, long ws_words, void* stream);
int r3d_scene_obj_union(long M, int nx, int ny, int nz, int n_labels, long n_units, int connectivity, int32_t* ws, long ws_words,
                        void* stream);
int r3d_scene_obj_components(long M, long n_units, int min_points, int32_t* ws, long ws_words, void* stream);
int r3d_scene_obj_stats(const float* scan, int ld, long M, float x0, float y0, float z0, float voxel, int nx, int ny, int nz,
                        int n_labels, long n_units, long n_objects, int64_t* object_labels, int32_t* object_points,
                        int32_t* object_units, float* object_lo, float* object_hi, float* object_centroid, int64_t* object_sums,
                        const int32_t* ws, long ws_words, void* stream);
int r3d_scene_obj_ids(long M, long n_units, long n_objects, const int32_t* unit_index, int32_t* objects, int32_t* ws,
                      long ws_words, void* stream);

/* ---- match_objects: a scan's objects against ground-truth instances ("Matching objects against ground
 * truth", M1-M8).  Additive: no entry point above changes.  The reference scores points only (eval_noise.py:23-72); the
 * definition is this project's.  pred, truth: M object ids each, int32 (bytes 4) or int64 (8), read as they are; g < 0: the
 * point is in no object; legal ids are 0 .. 2^31 - 2.  With ignore_unannotated a point whose truth id is negative takes part in
 * nothing (M1).  The labels, for both columns or for none (NULL): M classes each, int32 or int64.  ws: ONE int32 scratch of
 * r3d_scene_match_ws_words(M) words (-1: M outside 1 .. R3D_SCENE_MAX_POINTS) shared by the four calls of one matching; its
 * first R3D_SCENE_MATCH_REC words are the record the host reads, R3D_MATCH_R_* (`+ column`: the word of pred, then of truth):
 *   MAX1 + column the largest legal id of a participating point + 1 (0: none)   NNEG + column the participating points with
 *   a negative id   NIGNORED points M1 took out   NBAD ids >= 2^31 - 1, both columns   BADMAX the largest of those (uint64, two
 *   words)   ROWS + column pred rows P, truth rows T   MIXED + column the rows in which some point carries another label than
 *   the row's first   NBOTH points with a row in both columns   NPAIRS pairs
 *
 *   entry point            what it does                                                                  host reads
 *   r3d_scene_match_ids    zeroes the record, then MAX1 .. BADMAX of it (integer maxima and counts, one atomic per word
 *                          and workgroup)                                                                MAX1 .. BADMAX
 *   r3d_scene_match_rows   max_pred, max_truth: the two MAX1 as read, less one (both >= 0); n_pred_in, n_truth_in: M less
 *                          NIGNORED less the column's NNEG.  Per column the stable LSD radix sort of (id, scan index), 1 .. 4 passes
 *                          by the largest key (a point without a row sorts under the largest id + 1), run heads, their
 *                          exclusive scan, the row tables in ws (rows in ascending id order, a row's points by ascending
 *                          scan index); pred_index, truth_index (M,) int32: the row of the point, -1 without one.  With
 *                          labels: every point of a run against the label of the run's head.            ROWS, MIXED
 *   r3d_scene_match_pairs  n_pred, n_truth: the two ROWS as read (both >= 1).  pred_ids (P,) int64, pred_points (P,) int32
 *                          and, with labels, pred_classes (P,) int64, the label of the row's point with the lowest scan
 *                          index; the same for truth.  Then two stable sorts of 32-bit keys: by truth row, then by the pred
 *                          row gathered through the first order (a point without both rows: the keys T and P, last); heads
 *                          where (p, t) changes, their scan, the pair tables in ws in ascending (p, t).   NBOTH, NPAIRS
 *   r3d_scene_match_best   n_pairs: NPAIRS as read.  thresholds: n_iou <= R3D_SCENE_MATCH_IOU floats in HOST memory, ascending, each in
 *                          (0, 1].  pair_pred, pair_truth, pair_points (n_pairs,) int32; pair_iou (n_pairs,) fp32 =
 *                          (float)inter / (float)(pred_points[p] + truth_points[t] - inter), one IEEE division; a pair is
 *                          ELIGIBLE without classes, or when the two classes are equal.  truth_best (T,) int32: per eligible
 *                          pair one 64-bit integer atomicMax on (iou bits << 32) | (0xFFFFFFFF - p), then the pair whose
 *                          value won; pred_best (P,) int32: a segmented maximum over the contiguous pairs of p on
 *                          (iou bits << 32) | (0xFFFFFFFF - pair row), one integer atomicMax per run and workgroup; -1
 *                          without an eligible pair.  pair_match (n_pairs,) bytes, written last: for a pair that is the
 *                          best of both its rows the number of thresholds its IoU meets, else 0.  best_words: n_pred +
 *                          n_truth int64 of the caller's scratch.                                         -
 * No float goes through an atomic: the same columns give the same bits. */
#define R3D_SCENE_MATCH_REC 32
#define R3D_SCENE_MATCH_IOU 8
#define R3D_MATCH_R_MAX1 0
#define R3D_MATCH_R_NNEG 2
#define R3D_MATCH_R_NIGNORED 4
#define R3D_MATCH_R_NBAD 5
#define R3D_MATCH_R_BADMAX 6
#define R3D_MATCH_R_ROWS 8
#define R3D_MATCH_R_MIXED 10
#define R3D_MATCH_R_NBOTH 12
#define R3D_MATCH_R_NPAIRS 13
long r3d_scene_match_ws_words(long M);
int r3d_scene_match_ids(const void* pred, int pred_bytes, const void* truth, int truth_bytes, long M, int ignore_unannotated,
                        int32_t* ws, long ws_words, void* stream);
int r3d_scene_match_rows(const void* pred, int pred_bytes, const void* truth, int truth_bytes, const void* pred_labels,
                         int pred_label_bytes, const void* truth_labels, int truth_label_bytes, long M, int ignore_unannotated,
                         long max_pred, long max_truth, long n_pred_in, long n_truth_in, int32_t* pred_index,
                         int32_t* truth_index, int32_t* ws, long ws_words, void* stream);
int r3d_scene_match_pairs(long M, long n_pred, long n_truth, const int32_t* pred_index, const int32_t* truth_index,
                          const void* pred_labels, int pred_label_bytes, const void* truth_labels, int truth_label_bytes,
                          int64_t* pred_ids, int32_t* pred_points, int64_t* pred_classes, int64_t* truth_ids,
                          int32_t* truth_points, int64_t* truth_classes, int32_t* ws, long ws_words, void* stream);
int r3d_scene_match_best(long M, long n_pred, long n_truth, long n_pairs, const int32_t* pred_points, const int32_t* truth_points,
                         const int64_t* pred_classes, const int64_t* truth_classes, const float* thresholds, int n_iou,
                         int32_t* pair_pred, int32_t* pair_truth, int32_t* pair_points, float* pair_iou, int32_t* pred_best,
                         int32_t* truth_best, uint8_t* pair_match, int64_t* best_words, const int32_t* ws, long ws_words,
                         void* stream);

/* ---- smooth_scene: the scores of a labelled scan propagated over the voxel graph ("Smoothing a labelled
 * scan", S1-S7).  Additive: no entry point above changes.  The reference has no such function; the definition is this
 * project's.  The grid, the sort and the voxel table are those of build_segments: r3d_scene_grow_bounds, _sort and _voxels
 * run first, as they are, and ws, M, nx, ny, nz below are theirs.  V = n_voxels (R3D_GROW_R_V as read), C = n_cols <= R3D_SCENE_SCORE_COLS_MAX.  Every
 * float operation is fp32 and rounded on its own (__fadd_rn, __fmul_rn, __fdiv_rn); none goes through an atomic.
 *
 *   r3d_scene_smooth_evidence  scores (M, C) fp32, votes (M,) int32: those of the result.  A CONTRIBUTOR is a valid point
 *                              with votes > 0, its row scores[p] / (float)votes[p].  voxel_evidence (V, C) fp32: per voxel
 *                              the contributors' rows by ascending scan index, summed as r3d_scene_seg_pool sums a segment
 *                              (ranks in tiles of 256, part = the first row, += the next, tot = the first tile's part, +=
 *                              the next), tot / (float)members; zeros without a member.  voxel_members (V,) int32;
 *                              voxel_ring (V,) int32: 0 with a member, else -1.
 *   r3d_scene_smooth_graph     voxel_neighbours (R3D_SCENE_SMOOTH_SLOTS, V) int32, slot-major: column v holds the rows of the occupied voxels
 *                              among the 6 or 26 cells around voxel v, found by their coordinates as r3d_scene_grow_absorb
 *                              finds them, in ascending key order, packed to the front, -1 behind them.  With voxel_mean
 *                              (V, 3) (else NULL) a neighbour must pass the colour test of r3d_scene_grow_union as well: a
 *                              NaN mean joins nothing.
 *   r3d_scene_smooth_sweep     `iterations` (0 .. R3D_SCENE_SMOOTH_SWEEPS) launches, sweep t = 0, 1, ...: sweep t reads Z_t (t = 0: voxel_evidence,
 *                              else z[(t - 1) & 1]) and writes z[t & 1]; z0, z1 (V, C) fp32, two arrays (z1 may be NULL below
 *                              two sweeps, z0 below one).  The result lies in z[(iterations - 1) & 1].  A neighbour u is LIVE
 *                              at t when 0 <= ring[u] <= t.  With n >= 1 live neighbours u_0 < u_1 < ...: s = Z_t[u_0],
 *                              s += Z_t[u_1], ..., m = s / (float)n; a voxel with a member (ring 0) gets b * Y + a * m, a =
 *                              alpha, b = 1.0f - a, two multiplications and one addition; one without gets m and, while its
 *                              ring is -1, ring = t + 1.  With n == 0 the voxel keeps Z_t and its ring.  voxel_ring is ONE
 *                              array written in place: a reader of the same launch sees -1 or t + 1, and neither is live.
 *   r3d_scene_smooth_spread    voxel_scores: the last sweep's Z (voxel_evidence without a sweep).  voxel_labels (V,) int64:
 *                              the arg-max of the row (the lowest column wins a tie, a NaN never replaces a value) where ring
 *                              >= 0, else -1.  A point whose voxel_index is a row with ring >= 0 is SMOOTHED: scores, labels
 *                              = the voxel's, votes = 1, smoothed = 1; any other point copies in_scores, in_labels, in_votes,
 *                              smoothed = 0.  counts: R3D_SCENE_SMOOTH_COUNTS int32 words, zeroed here, by integer atomics
 *                              aggregated per workgroup, R3D_SMOOTH_R_*: MEMBER_VOXELS voxels with a member  FILLED_VOXELS
 *                              filled voxels (ring > 0)  NSMOOTHED smoothed points  NCHANGED of them: in_labels >= 0 and the
 *                              label differs  NFILLED of them: in_labels == -1  NUNLAB labels that are -1 in the result. */
#define R3D_SCENE_SMOOTH_SLOTS 26
#define R3D_SCENE_SMOOTH_SWEEPS 64
#define R3D_SCENE_SMOOTH_COUNTS 8
#define R3D_SMOOTH_R_MEMBER_VOXELS 0
#define R3D_SMOOTH_R_FILLED_VOXELS 1
#define R3D_SMOOTH_R_NSMOOTHED 2
#define R3D_SMOOTH_R_NCHANGED 3
#define R3D_SMOOTH_R_NFILLED 4
#define R3D_SMOOTH_R_NUNLAB 5
int r3d_scene_smooth_evidence(long M, int nx, int ny, int nz, int n_cols, const float* scores, const int32_t* votes, long n_voxels,
                              float* voxel_evidence, int32_t* voxel_members, int32_t* voxel_ring, const int32_t* ws, long ws_words,
                              void* stream);
int r3d_scene_smooth_graph(long M, int nx, int ny, int nz, long n_voxels, int connectivity, const float* voxel_mean,
                           float colour_tol, int32_t* voxel_neighbours, const int32_t* ws, long ws_words, void* stream);
int r3d_scene_smooth_sweep(long M, long n_voxels, int n_cols, int iterations, float alpha, const float* voxel_evidence,
                           const int32_t* voxel_neighbours, float* z0, float* z1, int32_t* voxel_ring, void* stream);
int r3d_scene_smooth_spread(long M, int n_cols, long n_voxels, const int32_t* voxel_index, const int32_t* voxel_ring,
                            const float* voxel_scores, const float* in_scores, const int64_t* in_labels, const int32_t* in_votes,
                            int64_t* voxel_labels, float* scores, int64_t* labels, int32_t* votes, uint8_t* smoothed,
                            int32_t* counts, void* stream);

/* ---- Cutting episode clouds from a block pool resident on the device (dataloaders/loader.py:219-237: the per-cloud point
 * draw of sample_pointcloud_universal; :258-276: its channels; :302-350: its labels.  Definition: INTEGRATION.md, "Cutting
 * episodes on the device").  Additive: the entry points above and what they compute are as they were.
 * Pool: points (T, 6) fp32 rows x y z r g b, labels (T,) int32, offsets (n_blocks + 1,) int64: block k is rows
 * offsets[k] .. offsets[k + 1] - 1, 1 .. R3D_CUT_MAX_BLOCK_POINTS of them; T < 2^31.
 * desc: (E (S + Q), 5) int32, one row {block, share_class, m_A, flags, key} per cloud, per episode the S support clouds then
 * the Q query clouds (x_all order); flags: R3D_CUT_FLAG_QUERY 0 support / 1 query (must agree with the position),
 * R3D_CUT_FLAG_GT_ZERO the ground-truth mask is zero (R3D_CUT_FLAG_PARTIAL: r3d_episode_cut_partial below).  classes: (E, n_way) int32, the sampled classes of every episode (n_way <= 32).
 * With n the block's points, N <= 8192 the cloud's, c = share_class, mix / stream / draw the hash of r3d_augment_clouds,
 * hA = stream(seed, 2 key), hB = stream(seed, 2 key + 1):
 *   A   slots 0 .. m_A - 1: the m_A points of class c with the smallest (draw(hA, i), i), by ascending local index i;
 *   B   n >= N: slots m_A .. N - 1: the N - m_A points with the smallest (draw(hB, i), i), by ascending i;
 *   B'  n <  N: slot m_A + j = (uint64(draw(hB, j)) * n) >> 32;
 *   C   over the N slots the prepared cloud of r3d_scene_prepare (the same device function): xyz - min, rgb / 255.0f at
 *       rgb_ch, xyz' / max at XYZ_ch (a flat axis gives 0), written at out[b * o_sb + ch * o_sc + t * o_sn];
 *   D   support cloud (e, i): mask[e S + i][t] = (label of slot t == c), gt_mask = mask, or zeros under R3D_CUT_FLAG_GT_ZERO;
 *       query cloud (e, j): query_y[e Q + j][t] = gt_query_y = 1 + the first position of the label in classes[e], 0 if absent;
 *       slot_map (E (S + Q), N) int32: the pool row of every slot.
 * rec: 2 int32 words the caller zeroes.  A cloud whose descriptor cannot be cut (block outside the pool, m_A outside
 * 0 .. min(N, points of class c), unknown flag bits, a kind that disagrees with the position, offsets outside the pool)
 * writes nothing but rec[0] += 1 and rec[1] = max(rec[1], 1 + its index); every index is bounded before it is used.
 * One 256-thread workgroup per cloud; the m smallest by a radix select over the draw (four 256-bin histograms in LDS,
 * draws recomputed), ties by index, survivors compacted in index order by ballot and prefix count.  Integer counts and
 * min / max only: the same descriptors and seed give the same bits, whatever else is in the launch. */
#define R3D_CUT_MAX_BLOCK_POINTS (1 << 20)
#define R3D_CUT_FLAG_QUERY 1
#define R3D_CUT_FLAG_GT_ZERO 2
#define R3D_CUT_FLAG_PARTIAL 4
int r3d_episode_cut(const float* points, const int32_t* labels, const int64_t* offsets, int n_blocks, long T,
                    const int32_t* desc, const int32_t* classes, int E, int n_way, int S, int Q, int N, unsigned seed, int C,
                    int rgb_ch, int XYZ_ch, float* out, long o_sb, long o_sc, long o_sn, int32_t* mask, int32_t* gt_mask,
                    int64_t* query_y, int64_t* gt_query_y, int32_t* slot_map, int32_t* rec, void* stream);

/* ---- Partial noise in a cut episode (dataloaders/loader.py:239-322: one wrong object is flipped into a support mask and,
 * with probability 0.3, one right object is taken out; :741-779: the shots it is applied to.  Definition: INTEGRATION.md,
 * "Cutting episodes on the device", steps P0-P7).  Additive: r3d_episode_cut keeps its arguments and results and still
 * refuses R3D_CUT_FLAG_PARTIAL.
 * r3d_episode_cut_partial takes r3d_episode_cut's arguments, then instances (T,) int32 -- the object id of every pool row,
 * may be null -- and info (E (S + Q), 8) int32; rec has 4 words the caller zeroes.  A descriptor without R3D_CUT_FLAG_PARTIAL is cut
 * with the bits of r3d_episode_cut and gets info = 0.  The flag is legal on a support cloud with m_A == 0 when instances is
 * given; otherwise the cloud is refused as any bad descriptor (rec[0], rec[1], nothing else written, info included).
 * With the flag, over the N slots of steps B / B' (m_A = 0: a uniform sample), lab / inst read through the slot:
 *   mask0[t] = (lab[t] == c);  objects o_0 < .. < o_{K-1}: the distinct inst, ascending as signed;  first(o): the lowest
 *   slot holding o;  eligible(o) = lab[first(o)] != c;  fg(o): some slot of o has mask0;  e, f: how many are eligible, fg;
 *   multi = K > 1 and some lab[t] != lab[0];
 *   flip, if multi and e > 0: the r-th eligible object, r = (uint64(draw(hA, 0)) * e) >> 32, joins the mask;
 *   drop, if draw(hA, 1) > 0xB3333333 and f > 0: the r2-th fg object, r2 = (uint64(draw(hA, 2)) * f) >> 32, leaves it
 *   (after the flip) -- unless that leaves no point, then it is not applied;
 *   mask = the result, gt_mask = zeros under R3D_CUT_FLAG_GT_ZERO, else mask0.  A final mask without a point: rec[2] += 1,
 *   rec[3] = max(rec[3], 1 + the cloud's index); the cloud is written in full.
 *   info[cloud] = {K, e, f, did, o_flip, n_flip, o_drop, n_drop}: did bit 0 flipped, bit 1 dropped, bit 2 drop drawn but
 *   skipped; n_*: slots holding the object; ids and counts 0 where nothing happened.
 * The objects come from a bitonic sort of 64-bit keys (inst biased to unsigned << 32 | slot) in LDS, run ids and the r-th
 * object from ballot counts, the flags from integer atomicOr: integers only, nothing depends on scheduling.  LDS: 8 P + 8 N
 * bytes, P the power of two >= N (128 KiB at N = 8192). */
int r3d_episode_cut_partial(const float* points, const int32_t* labels, const int64_t* offsets, int n_blocks, long T,
                            const int32_t* desc, const int32_t* classes, int E, int n_way, int S, int Q, int N, unsigned seed,
                            int C, int rgb_ch, int XYZ_ch, float* out, long o_sb, long o_sc, long o_sn, int32_t* mask,
                            int32_t* gt_mask, int64_t* query_y, int64_t* gt_query_y, int32_t* slot_map, int32_t* rec,
                            const int32_t* instances, int32_t* info, void* stream);

#ifdef __cplusplus
}
#endif
#endif
