"""Thin torch-tensor wrappers over the C ABI (include/r3d.h).

PyTorch is plumbing here: device memory (caching allocator), the current HIP stream and
tensor views.  All compute happens in libr3d_hip.so; there is no eager fallback.
"""
import ctypes

import torch

from . import _lib

# Every number of the C ABI -- record words (GROW_R_V, HD_N_PROTO, ...), sizes, flag and enum values (ACT_LRELU, SCORE_L2,
# KNN_PATH_FEW, ...), limits (SCENE_GROW_AXIS, ...) -- is a `#define R3D_<NAME>` of include/r3d.h, declared and explained
# there next to its entry point, and is a name of this module without the prefix.  None is written here.
globals().update({name[len("R3D_"):]: value for name, value in _lib.CONSTANTS.items()})


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class SegLayout:
    """Row layout of a batch of E episodes in the encoder (include/r3d.h, "BATCHES OF EPISODES"): the clouds of the
    batch are the rows of one matrix, episode after episode, [S support clouds | Q query clouds] each.  Segment
    2 e + p is getFeatures call p of episode e (models/mpti.py:434,436: support, then query) -- the unit of the
    BatchNorm batch statistics and the order in which the running statistics see them.  Q == 0: E equal segments
    of S clouds (a plain getFeatures call is E = 1, S = B)."""

    def __init__(self, E, S, Q, N):
        self.E, self.S, self.Q, self.N = E, S, Q, N
        self.clouds = S + Q                    # clouds per episode
        self.B = E * (S + Q)                   # clouds of the batch
        self.M = self.B * N                    # rows of the batch
        self.rows_a, self.rows_b = S * N, Q * N
        self.n_seg = E * (2 if Q else 1)
        self.ep_rows = (S + Q) * N             # rows between consecutive episodes

    def counts(self, per_row=1):
        """(count_a, count_b) of the BatchNorm statistics: elements per channel in a support / query segment."""
        return float(self.rows_a * per_row), float(self.rows_b * per_row)

    def aligned(self, tile=64):
        return self.rows_a % tile == 0 and self.rows_b % tile == 0


class KernelTimer:
    """HIP-event timing of selected entry points on the stream they are launched on
    (bench.py's roofline leg).  Disabled (None) by default: zero overhead.

    repeat = 0: one event pair around every call (includes the event packets and any host launch gap).
    repeat = R > 0: after a timed region ran, its library calls are launched again R times back to back
    between ONE event pair and the region is priced at elapsed / R: device time of the launches, with the
    event and host overhead amortised (the calls are idempotent: same inputs, same outputs)."""

    def __init__(self, names, repeat=0):
        self.names = set(names)
        self.events = {n: [] for n in names}
        self.repeat = repeat
        if repeat:
            _lib.record_calls(True)

    def close(self):
        if self.repeat:
            _lib.record_calls(False)

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for n, ev in self.events.items():
            ms = [a.elapsed_time(b) / r for a, b, r in ev]
            out[n] = dict(launches=len(ms), total_ms=float(sum(ms)), avg_ms=float(sum(ms) / max(len(ms), 1)))
        return out


_TIMER = None


def set_timer(timer):
    global _TIMER
    _TIMER = timer


class _timed:
    def __init__(self, name):
        self.on = _TIMER is not None and name in _TIMER.names
        self.name = name

    def __enter__(self):
        if self.on:
            self.a = torch.cuda.Event(enable_timing=True)
            self.b = torch.cuda.Event(enable_timing=True)
            if _TIMER.repeat:
                _lib._call_log = []
            else:
                self.a.record()

    def __exit__(self, *exc):
        if self.on:
            if _TIMER.repeat:
                calls, _lib._call_log = _lib._call_log, None
                if exc[0] is None and calls:
                    self.a.record()
                    for _ in range(_TIMER.repeat):
                        for fn, args in calls:
                            fn(*args)
                    self.b.record()
                    _TIMER.events[self.name].append((self.a, self.b, _TIMER.repeat))
            else:
                self.b.record()
                _TIMER.events[self.name].append((self.a, self.b, 1))


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _rows(t):
    """(rows, ld) of a 2-D fp32 row-major view (unit column stride)."""
    assert t.dim() == 2 and t.stride(1) == 1 and t.dtype == torch.float32 and t.is_cuda, \
        "expected a 2-D fp32 CUDA tensor with unit column stride"
    return t.shape[0], t.stride(0)


def cm_to_pm(x, out=None):
    """(B, C, N) channel-major -> (B*N, C) point-major."""
    B, C, N = x.shape
    x = x.contiguous().float()
    if out is None:
        out = torch.empty(B * N, C, device=x.device, dtype=torch.float32)
    _, ld = _rows(out)
    _lib.check(_lib.load().r3d_cm_to_pm(_p(x), B, C, N, _p(out), ld, _st()))
    return out


def is_point_major_view(x):
    """x (..., C, N): a transposed VIEW of a point-major buffer (..., N, C) -- what the reference's collate hands over
    (`torch.from_numpy(raw).transpose(2, 3)`, dataloaders/loader.py:1666,1679: the on-disk layout, never materialised)."""
    if x.dtype != torch.float32 or x.dim() < 3:
        return False
    C, N = x.shape[-2], x.shape[-1]
    return x.stride(-1) == C and x.stride(-2) == 1 and x.transpose(-1, -2).is_contiguous()


def input_layouts(x):
    """x (B, C, N) as the caller hands it -> (x_pm (B*N, C), x_cm (B, C, N) contiguous or None).
    A transposed view of point-major rows is used AS IT LIES: x_pm is that buffer (no transpose kernel, no copy) and
    x_cm is None, so the first kNN builds its channel-major operand from the point-major rows itself -- the read it
    does for every later layer anyway (r3d_knn_topk_batched packs x_pm when no channel-major copy is given).  A
    contiguous channel-major tensor goes through r3d_cm_to_pm and doubles as the first kNN's operand."""
    B, C, N = x.shape
    if is_point_major_view(x):
        return x.transpose(1, 2).reshape(B * N, C), None
    x = x.contiguous().float()
    return cm_to_pm(x), x


def cat_clouds(a, b, dim=1):
    """cat((a, b), dim) of cloud tensors (..., C, N) that keeps the point-major rows of point-major views (the result is
    again such a view: one contiguous copy of rows instead of a strided gather into channel-major)."""
    if is_point_major_view(a) and is_point_major_view(b):
        return torch.cat((a.transpose(-1, -2), b.transpose(-1, -2)), dim).transpose(-1, -2)
    return torch.cat((a, b), dim)


def pm_to_cm(x_pm, B, N):
    """(B*N, C) point-major view -> (B, C, N) contiguous."""
    M, ld = _rows(x_pm)
    C = x_pm.shape[1]
    assert M == B * N
    out = torch.empty(B, C, N, device=x_pm.device, dtype=torch.float32)
    _lib.check(_lib.load().r3d_pm_to_cm(_p(x_pm), ld, B, C, N, _p(out), _st()))
    return out


def copy_cols(src, dst):
    M, lds = _rows(src)
    M2, ldd = _rows(dst)
    assert M == M2 and src.shape[1] == dst.shape[1]
    _lib.check(_lib.load().r3d_copy_cols(_p(src), lds, _p(dst), ldd, M, src.shape[1], _st()))
    return dst


def knn(x_pm, B, N, k, mode=SCORE_DGCNN, n_valid=None, return_scores=False, x_cm=None, status=None, n_valid_stride=0):
    """x_pm (B*N, C) -> idx (B, N, k) int32, best first.  x_cm: optional (B, C, N) channel-major
    copy of the same points (saves the internal transpose of the streamed k <= 32 kernel).
    n_valid (device int32) with n_valid_stride > 0: set b has n_valid[b * n_valid_stride] valid rows.
    status (device int32, k > 32): selects the large-k streamed kernel; bit 0 set afterwards = overflow, redo with None."""
    M, ld = _rows(x_pm)
    C = x_pm.shape[1]
    assert M == B * N
    if x_cm is not None:
        assert x_cm.is_contiguous() and x_cm.shape == (B, C, N) and x_cm.dtype == torch.float32
    if status is not None:
        assert status.dtype == torch.int32
    lib = _lib.load()
    dev = x_pm.device
    # one scratch; the library decides which kernels run and what they need in it
    words = lib.r3d_knn_ws_words(B, N, C, k, (status is not None) | (x_cm is not None) << 1)
    ws = torch.empty(words, device=dev, dtype=torch.float32)
    idx = torch.empty(B, N, k, device=dev, dtype=torch.int32)
    sc = torch.empty(B, N, k, device=dev, dtype=torch.float32) if return_scores else None
    with _timed("knn_topk_l2" if mode == SCORE_L2 else "knn_topk"):
        _lib.check(lib.r3d_knn_topk_batched(_p(x_pm), ld, _p(x_cm), B, N, C, k, mode, _p(n_valid), n_valid_stride, _p(ws), words,
                                            _p(idx), _p(sc), _p(status), _st()))
    return (idx, sc) if return_scores else idx


def knn_path(x_pm, B, N, k, x_cm=None, status=None):
    """The kernel configuration knn() launches for these operands under the debug switches as set: the KNN_PATH_* bit mask
    of r3d_debug_knn_path.  Launches nothing."""
    _, ld = _rows(x_pm)
    flags = (KNN_FLAG_STATUS if status is not None else 0) | (KNN_FLAG_X_CM if x_cm is not None else 0)
    return _lib.load().r3d_debug_knn_path(B, N, x_pm.shape[1], k, flags, ld, x_pm.data_ptr() % 16)


def pointwise_conv(x_pm, W, scale=None, shift=None, act=ACT_NONE, out=None):
    """act(scale * (x W^T) + shift); W (Co, K) contiguous."""
    M, ldx = _rows(x_pm)
    K = x_pm.shape[1]
    Co = W.shape[0]
    assert W.is_contiguous() and W.shape[1] == K and W.dtype == torch.float32
    if out is None:
        out = torch.empty(M, Co, device=x_pm.device, dtype=torch.float32)
    M2, ldo = _rows(out)
    assert M2 == M and out.shape[1] == Co
    with _timed("pointwise_conv"):
        _lib.check(_lib.load().r3d_pointwise_conv(_p(x_pm), ldx, _p(W), M, K, Co, _p(scale), _p(shift), act,
                                                  _p(out), ldo, _st()))
    return out


def edgeconv(PQ, idx, W2, s2, t2, out, B, N, want_argmax=False):
    K = idx.shape[-1]
    assert PQ.is_contiguous() and PQ.shape == (B * N, 128) and idx.is_contiguous() and idx.dtype == torch.int32
    assert W2.is_contiguous() and W2.shape == (64, 64)
    M, ldo = _rows(out)
    assert M == B * N and out.shape[1] == 64
    am = torch.empty(B * N, 64, device=PQ.device, dtype=torch.int32) if want_argmax else None
    with _timed("edgeconv"):
        _lib.check(_lib.load().r3d_edgeconv_fwd(_p(PQ), _p(idx), _p(W2), _p(s2), _p(t2), _p(out), ldo, B, N, K,
                                                _p(am), _st()))
    return am


def attention(qkv, B, N, out, want_lse=False, group=0):
    """Inference attention of B clouds, head width D = out.shape[1] (qkv: q | k | v, 3 D columns).  group > 0: the clouds
    are a batch of episodes of `group` clouds each; the key-axis split (and with it every output bit) is then the one of a
    single episode."""
    M, ld = _rows(qkv)
    M2, ldo = _rows(out)
    D = out.shape[1]
    assert M == B * N and M2 == M and qkv.shape[1] == 3 * D
    lib = _lib.load()
    lse = torch.empty(M, device=qkv.device, dtype=torch.float32)
    words = lib.r3d_attention_ws_words_ep_d(B, N, group, D)
    if words < 0:
        raise NotImplementedError("attention head width %d: the kernels are built for 32, 64, 96, 128" % D)
    ws = torch.empty(words, device=qkv.device, dtype=torch.float32)
    with _timed("attention"):
        _lib.check(lib.r3d_attention_fwd_train_ep_d(_p(qkv), ld, B, N, _p(out), ldo, _p(lse), 0.0, ctypes.c_uint(0), None,
                                                    group, D, _p(ws), _st()))
    return lse if want_lse else None


class HeadBuffers:
    """Device buffers of the transductive heads of E episodes (capacity sized, no host sync).  Every array has a leading
    episode axis for every E, episode e's system lives at [e] (nodes / Y / Z: rows [e n_cap, (e + 1) n_cap)); the
    single-episode head of the reference's schedule is E = 1: desc (1, HD_WORDS), stats (1, 2), ..."""

    def __init__(self, n_way, k_shot, N, n_q_pts, k_sub, k_connect, D, device, E=1):
        lib = _lib.load()
        self.E = E
        self.n_way, self.k_shot, self.N, self.n_q_pts, self.k_sub, self.kp1, self.D = \
            n_way, k_shot, N, n_q_pts, k_sub, k_connect + 1, D
        # k_sub + 1 prototype slots per class: torch_cluster's float-rounded sample count gives k or k + 1 seeds
        # (csrc/head_proto.hip::hp_fps_count, models/mpti.py:612-613)
        self.n_cap = (n_way + 1) * (k_sub + 1) + n_q_pts
        assert lib.r3d_head_desc_words() == HD_WORDS
        i32 = dict(device=device, dtype=torch.int32)
        f32 = dict(device=device, dtype=torch.float32)
        self.desc = torch.zeros(E, HD_WORDS, **i32)
        self.nodes = torch.empty(E * self.n_cap, D, **f32)
        # label columns travel as float4 per node.  More than 3 ways (5..8 classes): TWO planes of 4 columns, plane 1
        # (classes 4..7) behind the E systems of plane 0 -- the label propagation is column-wise independent and solves
        # the planes one after the other on the same graph (csrc/head_graph.hip)
        self.planes = 1 if n_way <= 3 else 2
        self.Y = torch.empty(self.planes * E * self.n_cap, 4, **f32)
        self.Z = torch.empty(self.planes * E * self.n_cap, 4, **f32)
        self.proto_words = lib.r3d_head_proto_ws_words(n_way, k_shot, N)
        self.proto_stride = (self.proto_words + 3) // 4 * 4      # even (64-bit words inside), 16-byte rows
        self.proto_ws = torch.empty(E, self.proto_stride, **i32)
        self.lp_words = lib.r3d_lp_ws_words(self.n_cap, self.kp1)
        self.lp_stride = (self.lp_words + 3) // 4 * 4             # float4 arrays inside
        self.lp_ws = torch.empty(E, self.lp_stride, **i32)
        self.assign = torch.empty(E, 2 * n_way * k_shot * N, **i32)
        self.cluster_count = torch.zeros(E, self.n_cap, **i32)
        self.stats = torch.zeros(E, 2, **i32)                # per system: {converged, CG iterations}
        self.stats2 = torch.zeros(E, 2, **i32) if self.planes == 2 else None   # ... of the second plane's solves
        self.knn_status = torch.zeros(1, **i32)                   # ONE word for the batch (bit 0: survivor overflow)
        self.stats_bwd = torch.zeros(E, 2, **i32)
        # all FPS rounds in one persistent launch: its workgroups that hold points must be co-resident (~500 slots of
        # this kernel at D <= 192, 250 above); fps_group episodes share a launch, fps_slots caps what may be resident
        # (the library clamps the group to the kernel's real occupancy as well: csrc/head_proto.hip::fps_slots_clamp)
        self.fps_one_launch = True
        self.fps_blocks = (n_way * k_shot * N + 255) // 256 + n_way + 1
        self.fps_slots = 500 if D <= 192 else 250
        off = (ctypes.c_long * 6)()
        lib.r3d_head_proto_ws_offsets(n_way, k_shot, N, off)
        self.ws_off = list(off)
        lib.r3d_lp_ws_offsets(self.n_cap, self.kp1, off)
        self.lp_off = dict(zip(("row_ptr", "col", "val", "dinv", "agg", "cg"), off))
        off4 = (ctypes.c_long * 4)()
        lib.r3d_lp_ws_offsets_coarse(self.n_cap, self.kp1, off4)
        self.lp_off.update(zip(("MW", "Epart", "Einv", "r"), off4))

    @property
    def fps_group(self):
        return max(1, self.fps_slots // self.fps_blocks)

    def n_nodes_ptr(self):
        return self.desc[0, HD_N_NODES:]   # episode e's count HD_WORDS words further on

    def n_proto_ptr(self):
        return self.desc[0, HD_N_PROTO:]

    def status(self, backward=False):
        """head_status of the last launch through these buffers (backward: of its adjoint solve as well)."""
        return head_status(self.stats, self.desc, self.knn_status, self.stats_bwd if backward else None)

    def csr(self, e=0):
        """(n, row_ptr (n+1) int64, col (nnz) int64, val (nnz) fp32) of the normalised graph S the last
        r3d_label_propagate left in episode e's workspace (synchronises; tests, tools and bench.py's byte counts)."""
        n = int(self.desc[e, HD_N_NODES].item())
        o = self.lp_off
        ws = self.lp_ws[e]
        row_ptr = ws[o["row_ptr"]:o["row_ptr"] + n + 1].to(torch.int64)
        nnz = int(row_ptr[-1].item())
        col = ws[o["col"]:o["col"] + (nnz + 1) // 2].view(torch.int16)[:nnz].to(torch.int64) & 0xffff
        val = ws[o["val"]:o["val"] + nnz].view(torch.float32)
        return n, row_ptr, col, val

    def coarse(self, e=0):
        """(agg (n,) int64, MW (n_cap, 64) fp32, Einv (64, 64) fp32, r (n_cap, 4) fp32): the coarse space of the CG's
        preconditioner and the residual the last solve left in episode e's workspace (views; synchronises; tests and
        tools)."""
        n = int(self.desc[e, HD_N_NODES].item())
        o, nc = self.lp_off, self.n_cap
        ws = self.lp_ws[e]
        agg = ws[o["agg"]:o["agg"] + n].to(torch.int64)
        MW = ws[o["MW"]:o["MW"] + nc * 64].view(torch.float32).view(nc, 64)
        Einv = ws[o["Einv"]:o["Einv"] + 64 * 64].view(torch.float32).view(64, 64)
        r = ws[o["r"]:o["r"] + nc * 4].view(torch.float32).view(nc, 4)
        return agg, MW, Einv, r


def head_status(stats, desc, knn_status, stats_bwd=None):
    """The one reading of a head launch's status words -> (4,) int32 on their device: [bad, overflow, iters_sum, iters_max].
    bad: systems whose CG did not converge (stats[e, 0] == 0), plus systems whose one-launch FPS timed out
    (desc[e, HD_FPS_TIMEOUT] != 0), plus -- stats_bwd given -- systems whose adjoint CG did not converge; overflow: 1 if
    the launch's 201-NN survivor buffer overflowed (knn_status[0] != 0); the sum and the maximum of the forward CG
    iteration counts stats[:, 1].  A launch was exact iff bad == 0 and overflow == 0.  Torch ops on (E, .) tensors
    only, no host read, no data-dependent shape: the same on CPU tensors and inside a stream capture."""
    miss = [stats[:, 0] == 0, desc[:, HD_FPS_TIMEOUT] != 0] + ([stats_bwd[:, 0] == 0] if stats_bwd is not None else [])
    bad, iters = torch.cat(miss).sum(dtype=torch.int32), stats[:, 1].to(torch.int32)
    return torch.stack((bad, knn_status[0] != 0, iters.sum(dtype=torch.int32), iters.max()))  # (the flag is promoted)


def head_prototypes(hb, support_y, shot_keep, sfeat_pm, qfeat_pm, feat_ep_rows=0):
    """Prototypes + node matrices of hb.E episodes.  sfeat_pm / qfeat_pm: the support / query rows of episode 0 inside
    the batch's feature matrix; episode e's rows start feat_ep_rows rows further on.  support_y (E, S, N) int32,
    shot_keep optional (E, S) int32."""
    S = hb.n_way * hb.k_shot
    E = hb.E
    ldf, ldq = sfeat_pm.stride(0), qfeat_pm.stride(0)
    assert sfeat_pm.dtype == torch.float32 and qfeat_pm.dtype == torch.float32 and sfeat_pm.stride(1) == 1
    assert E == 1 or feat_ep_rows >= S * hb.N
    assert support_y.dtype == torch.int32 and support_y.is_contiguous() and support_y.numel() == E * S * hb.N
    assert shot_keep is None or (shot_keep.dtype == torch.int32 and shot_keep.numel() == E * S)
    with _timed("head_prototypes"):
        _lib.check(_lib.load().r3d_head_prototypes_batched(
            E, hb.fps_group, _p(support_y), S * hb.N, _p(shot_keep), S, _p(sfeat_pm), ldf, feat_ep_rows, _p(qfeat_pm), ldq,
            feat_ep_rows, hb.n_way, hb.k_shot, hb.N, hb.D, hb.n_q_pts, hb.k_sub, _p(hb.nodes), hb.nodes.stride(0), hb.n_cap,
            _p(hb.Y), _p(hb.desc), HD_WORDS, _p(hb.assign), 2 * S * hb.N, _p(hb.cluster_count), hb.n_cap, _p(hb.proto_ws),
            hb.proto_words, hb.proto_stride, HEAD_FPS_ONE_LAUNCH if hb.fps_one_launch else 0, _st()))


def knn_nodes(hb, exact=False):
    """201-NN lists (E, n_cap, kp1) of every episode's graph nodes (mpti.py:731-736).  exact: the insertion kernel
    (always exact); otherwise the append-and-rank kernel, whose survivor-buffer overflow sets hb.knn_status."""
    nbr = knn(hb.nodes, hb.E, hb.n_cap, hb.kp1, mode=SCORE_L2, n_valid=hb.n_nodes_ptr(), n_valid_stride=HD_WORDS,
              status=None if exact else hb.knn_status)
    if exact:
        hb.knn_status.zero_()
    return nbr


def label_propagate(hb, nbr, sigma, alpha=0.99, max_iter=200, tol=1e-6):
    assert nbr.numel() == hb.E * hb.n_cap * hb.kp1 and nbr.is_contiguous()
    with _timed("label_propagate"):
        _lib.check(_lib.load().r3d_label_propagate_batched(
            hb.E, _p(hb.nodes), hb.nodes.stride(0), hb.D, _p(nbr), hb.kp1, _p(hb.Y), _p(hb.n_nodes_ptr()),
            _p(hb.n_proto_ptr()), HD_WORDS, hb.n_cap, float(sigma), float(alpha), int(max_iter), float(tol), _p(hb.Z), _p(hb.lp_ws),
            hb.lp_words, hb.lp_stride, _p(hb.stats), 2, _st()))
        if hb.planes == 2:  # label columns 4..7: the same systems, further right-hand sides
            pl = hb.E * hb.n_cap
            _lib.check(_lib.load().r3d_label_propagate_solve_batched(
                hb.E, _p(hb.Y[pl:]), _p(hb.n_nodes_ptr()), HD_WORDS, hb.n_cap, hb.kp1, float(alpha), int(max_iter), float(tol),
                _p(hb.Z[pl:]), _p(hb.lp_ws), hb.lp_words, hb.lp_stride, _p(hb.stats2), 2, _st()))
            # one {converged, iterations} pair per system for the callers: converged = both, iterations = the larger
            hb.stats[:, 0] = torch.minimum(hb.stats[:, 0], hb.stats2[:, 0])
            hb.stats[:, 1] = torch.maximum(hb.stats[:, 1], hb.stats2[:, 1])
    return hb.Z


def graph_weights_verify(hb, sigma):
    """Recompute the gaussian edge weights of the graphs the last label_propagate left in hb (call with the chip otherwise
    idle) and return the number of entries whose bits differ from the ones the solve used (device int32 tensor)."""
    lib = _lib.load()
    dev = hb.nodes.device
    scratch = torch.empty(hb.E * lib.r3d_graph_weights_verify_words(hb.n_cap, hb.kp1), device=dev, dtype=torch.float32)
    bad = torch.zeros(1, device=dev, dtype=torch.int32)
    _lib.check(lib.r3d_graph_weights_verify(hb.E, _p(hb.nodes), hb.nodes.stride(0), hb.D, _p(hb.n_nodes_ptr()), HD_WORDS, hb.n_cap,
                                            hb.kp1, float(sigma), _p(hb.lp_ws), hb.lp_words, hb.lp_stride, _p(scratch), _p(bad),
                                            _st()))
    return bad


def logits_ce(Z, z_ep_rows, n_proto_ptr, desc_stride, E, n_q, N, n_classes, labels):
    """Z rows -> logits (E, n_q, n_classes, N), loss (E,) -- each the mean over ITS episode's query points --, pred (E, n_q, N)
    int32 (the arg-max).  Z: planes of 4 class columns with z_ep_rows rows per episode, of which the first
    n_proto_ptr[e * desc_stride] are not query rows; labels (E, n_q, N) int64, or None: logits and arg-max only."""
    dev = Z.device
    logits = torch.empty(E, n_q, n_classes, N, device=dev, dtype=torch.float32)
    loss = torch.empty(E, device=dev, dtype=torch.float32)
    pred = torch.empty(E, n_q, N, device=dev, dtype=torch.int32)
    if labels is not None:
        assert labels.dtype == torch.int64 and labels.is_contiguous() and labels.numel() == E * n_q * N
    _lib.check(_lib.load().r3d_query_logits_ce_batched(E, _p(Z), z_ep_rows, _p(n_proto_ptr), desc_stride, n_q, N, n_classes,
                                                       _p(labels), _p(logits), _p(loss), _p(pred), _st()))
    return logits, loss, pred


def query_logits_ce(hb, n_q, n_classes, labels):
    """logits_ce of the label-propagation result in hb."""
    return logits_ce(hb.Z, hb.n_cap, hb.n_proto_ptr(), HD_WORDS, hb.E, n_q, hb.N, n_classes, labels)


def logits_ce_from_rows(Z, E, n_q, N, n_classes, labels):
    """logits_ce of similarity rows that are query rows only (the ProtoNet heads): Z (E * n_q*N, 4) per plane."""
    zero = torch.zeros(1, device=Z.device, dtype=torch.int32)  # (no prototype rows in front of the query rows)
    return logits_ce(Z, n_q * N, zero, 0, E, n_q, N, n_classes, labels)


def ce_grad(Z, n_proto_ptr, desc_stride, E, n_cap, n_query_pts, n_classes, labels, gscale):
    """Backward of logits_ce's loss -> G, the layout of Z (n_cap rows per episode and plane).  gscale (its first element is
    used) scales every episode alike: the step's loss is the SUM of the episodes' losses."""
    gs = gscale.reshape(-1)[:1].to(torch.float32).contiguous()
    G = torch.empty_like(Z)
    _lib.check(_lib.load().r3d_ce_grad_batched(E, _p(Z), _p(n_proto_ptr), desc_stride, n_cap, n_query_pts, n_classes, _p(labels),
                                               _p(gs), _p(G), _st()))
    return G


def clean_shot_detect(sfeat_pm, support_x, support_y, n_way, k_shot, N, want_debug=False, E=1, feat_ep_rows=0):
    """shot_keep (E, n_way*k_shot) int32 of the eval-only clean-shot detection (mpti.py:178-223).  sfeat_pm: support rows
    of episode 0 inside the batch's feature matrix, episode e feat_ep_rows rows further on; support_x (E, S, Cin, N)."""
    ldf = sfeat_pm.stride(0)
    S = n_way * k_shot
    sx = support_x.reshape(E * S, -1, N).contiguous().float()
    sy = support_y.reshape(E * S, N).to(torch.int32).contiguous()
    dev = sfeat_pm.device
    keep = torch.empty(E, S, device=dev, dtype=torch.int32)
    dbg = torch.zeros(E, n_way, 2, 4 * k_shot, device=dev, dtype=torch.float32) if want_debug else None
    words = _lib.load().r3d_clean_ws_words(n_way, k_shot)
    ws = torch.empty(E, words, device=dev, dtype=torch.int32)
    _lib.check(_lib.load().r3d_clean_shot_detect_batched(E, _p(sfeat_pm), ldf, feat_ep_rows, sfeat_pm.shape[1], _p(sx),
                                                         sx.shape[1], _p(sy), n_way, k_shot, N, _p(keep), _p(dbg), _p(ws),
                                                         words, _st()))
    if E == 1:
        keep = keep[0]
        dbg = dbg[0] if dbg is not None else None
    return (keep, dbg) if want_debug else keep


_PROTO_METHODS = {"cosine": 0, "euclidean": 1}


def _proto_method(method):
    if method not in _PROTO_METHODS:
        raise NotImplementedError('Error! Distance computation method (%s) is unknown!' % method)
    return _PROTO_METHODS[method]


def protonet_head(sfeat_pm, qfeat_pm, support_y, n_way, k_shot, N, method, scaler=10.0):
    """Similarity rows (n_q*N, 4) of the ProtoNet head; method 'cosine' | 'euclidean'.  The library's single-episode entry
    point: no model calls it (ProtoNet runs protonet_head_batched, one episode included); the tests hold the batched and
    the training head to it bit for bit."""
    M, ldf = _rows(sfeat_pm)
    Mq, ldq = _rows(qfeat_pm)
    code = _proto_method(method)
    sy = support_y.reshape(n_way * k_shot, N).to(torch.int32).contiguous()
    dev = sfeat_pm.device
    Z = torch.empty((1 if n_way <= 3 else 2) * Mq, 4, device=dev, dtype=torch.float32)  # (planes of 4 classes)
    ws = torch.empty(n_way * k_shot * 2 * 256, device=dev, dtype=torch.float32)
    _lib.check(_lib.load().r3d_protonet_head(_p(sfeat_pm), ldf, _p(qfeat_pm), ldq, sfeat_pm.shape[1], _p(sy), n_way,
                                             k_shot, N, Mq, code, float(scaler), _p(Z), _p(ws), _st()))
    return Z


def protonet_head_batched(sfeat_pm, qfeat_pm, support_y, n_way, k_shot, N, method, n_ep, feat_ep_rows, n_query_pts, scaler=10.0,
                          shot_keep=None):
    """protonet_head for n_ep episodes in one launch pair: Z (n_ep * n_query_pts, 4) per plane, episode after episode, per
    episode bit for bit protonet_head's rows.  sfeat_pm / qfeat_pm: the support / query rows of episode 0 (views into ONE
    feature matrix in which episode e's rows start feat_ep_rows rows further on).  shot_keep (n_ep, n_way*k_shot), 0 = the
    shot's foreground stays out of its way's prototype (clean_shot_detect's result; ProtoNet_Contrast): None or all ones is
    the plain head bit for bit.  A device tensor is read on the device only; a host tensor is checked here for a way without
    a kept shot."""
    _, ldf = _rows(sfeat_pm)
    _, ldq = _rows(qfeat_pm)
    code = _proto_method(method)
    sy = support_y.reshape(n_ep * n_way * k_shot, N).to(torch.int32).contiguous()
    dev = sfeat_pm.device
    lib = _lib.load()
    words = lib.r3d_protonet_head_ws_words(n_ep, n_way, k_shot)
    if words < 0:
        raise NotImplementedError("ProtoNet head: 1 <= n_way <= 7, 1 <= episodes <= 65535 (n_way=%d, episodes=%d)" % (n_way, n_ep))
    keep = None
    if shot_keep is not None:
        keep = torch.as_tensor(shot_keep)
        if keep.numel() != n_ep * n_way * k_shot:
            raise ValueError("shot_keep has %d entries for %d episodes of %d-way %d-shot" % (keep.numel(), n_ep, n_way, k_shot))
        if not keep.is_cuda and not bool((keep.reshape(n_ep, n_way, k_shot) != 0).any(-1).all()):
            raise ValueError("shot_keep drops every shot of a way: its prototype would be 0 / 0 (the detection resets such a "
                             "way to all kept, models/protonet.py:529-532)")
        keep = keep.to(device=dev, dtype=torch.int32).reshape(n_ep, n_way * k_shot).contiguous()
    ws = torch.empty(words, device=dev, dtype=torch.float32)
    Z = torch.empty((1 if n_way <= 3 else 2) * n_ep * n_query_pts, 4, device=dev, dtype=torch.float32)  # (planes of 4 classes)
    _lib.check(lib.r3d_protonet_head_keep_batched(n_ep, _p(sfeat_pm), ldf, _p(qfeat_pm), ldq, feat_ep_rows, sfeat_pm.shape[1],
                                                  _p(sy), _p(keep), n_way, k_shot, N, n_query_pts, code, float(scaler), _p(Z),
                                                  _p(ws), words, _st()))
    return Z


def protonet_prototypes(sfeat_pm, support_y, n_way, k_shot, N, n_ep=1, feat_ep_rows=0, shot_keep=None):
    """The support half of protonet_head_batched: the prototype table (n_ep, n_way + 1, D), background first, of n_ep
    support sets (sfeat_pm: the support rows of episode 0, episode e feat_ep_rows rows further on; shot_keep as there, a
    device tensor or None).  Reads support rows only."""
    _, ldf = _rows(sfeat_pm)
    D = sfeat_pm.shape[1]
    sy = support_y.reshape(n_ep * n_way * k_shot, N).to(torch.int32).contiguous()
    dev = sfeat_pm.device
    lib = _lib.load()
    words = lib.r3d_protonet_head_ws_words(n_ep, n_way, k_shot)
    if words < 0:
        raise NotImplementedError("ProtoNet head: 1 <= n_way <= 7, 1 <= episodes <= 65535 (n_way=%d, episodes=%d)" % (n_way, n_ep))
    keep = None
    if shot_keep is not None:
        if shot_keep.numel() != n_ep * n_way * k_shot:
            raise ValueError("shot_keep has %d entries for %d episodes of %d-way %d-shot" % (shot_keep.numel(), n_ep, n_way, k_shot))
        keep = shot_keep.to(device=dev, dtype=torch.int32).reshape(n_ep, n_way * k_shot).contiguous()
    ws = torch.empty(words, device=dev, dtype=torch.float32)
    protos = torch.empty(n_ep, n_way + 1, D, device=dev, dtype=torch.float32)
    with _timed("protonet_prototypes"):
        _lib.check(lib.r3d_protonet_prototypes_batched(n_ep, _p(sfeat_pm), ldf, feat_ep_rows, D, _p(sy), _p(keep), n_way, k_shot,
                                                       N, _p(protos), _p(ws), words, _st()))
    return protos


def protonet_similarity(qfeat_pm, protos, n_way, method, n_sys, n_query_pts, q_sys_rows=None, scaler=10.0):
    """The query half of protonet_head_batched: similarity rows Z (n_sys * n_query_pts, 4) per plane of n_sys systems' query
    rows (system g's start q_sys_rows rows after system g - 1's; default: back to back) against a prototype table: protos
    (n_way + 1, D) or (1, n_way + 1, D) serves every system, (n_sys, n_way + 1, D) gives each its own."""
    _, ldq = _rows(qfeat_pm)
    D = qfeat_pm.shape[1]
    code = _proto_method(method)
    assert protos.dtype == torch.float32 and protos.is_contiguous() and protos.shape[-2:] == (n_way + 1, D)
    tables = protos.numel() // ((n_way + 1) * D)
    assert tables in (1, n_sys), "one prototype table, or one per system"
    assert qfeat_pm.shape[0] >= (n_sys - 1) * (q_sys_rows or n_query_pts) + n_query_pts
    Z = torch.empty((1 if n_way <= 3 else 2) * n_sys * n_query_pts, 4, device=qfeat_pm.device, dtype=torch.float32)
    with _timed("protonet_similarity"):
        _lib.check(_lib.load().r3d_protonet_similarity_batched(
            n_sys, _p(qfeat_pm), ldq, n_query_pts if q_sys_rows is None else q_sys_rows, D, _p(protos),
            0 if tables == 1 else (n_way + 1) * D, n_way, n_query_pts, code, float(scaler), _p(Z), _st()))
    return Z


def head_attach_queries(hb, fit, qfeat_pm, q_sys_rows=None):
    """The node matrices of hb.E systems from ONE fitted system and hb.E groups of query rows (system g's hb.n_q_pts rows
    start q_sys_rows rows after system g - 1's; default: back to back).  fit: fitted.FittedHead (prototype rows, label rows,
    desc and cluster counts of a head_prototypes call on the support set alone).  Afterwards knn_nodes, label_propagate and
    query_logits_ce run on hb as after head_prototypes."""
    _, ldq = _rows(qfeat_pm)
    assert qfeat_pm.shape[1] == hb.D and fit.nodes.shape[1] == hb.D
    step = hb.n_q_pts if q_sys_rows is None else q_sys_rows
    assert qfeat_pm.shape[0] >= (hb.E - 1) * step + hb.n_q_pts
    with _timed("head_attach_queries"):
        _lib.check(_lib.load().r3d_head_attach_queries_batched(
            hb.E, _p(fit.nodes), fit.nodes.stride(0), _p(fit.Y), fit.label_rows, _p(fit.desc), _p(fit.cluster_count),
            fit.proto_cap, _p(qfeat_pm), ldq, step, hb.n_way, hb.D, hb.n_q_pts, _p(hb.nodes), hb.nodes.stride(0), hb.n_cap,
            _p(hb.Y), _p(hb.desc), HD_WORDS, _p(hb.cluster_count), hb.n_cap, _st()))


def protonet_similarity_sets(qfeat_pm, tables, n_way, method, n_groups, n_query_pts, q_sys_rows=None, scaler=10.0):
    """protonet_similarity of n_groups query groups against K prototype tables in ONE launch that reads a query row once:
    tables (K, n_way + 1, D) contiguous, K * (n_way + 1) <= 64.  -> Z (n_groups * K * n_query_pts, 4) per plane, system
    g * K + k (group g, table k) after system g * K + k - 1; per table the bits of protonet_similarity on it alone."""
    _, ldq = _rows(qfeat_pm)
    D = qfeat_pm.shape[1]
    code = _proto_method(method)
    assert tables.dtype == torch.float32 and tables.is_contiguous() and tables.dim() == 3 and tables.shape[1:] == (n_way + 1, D)
    K = tables.shape[0]
    assert K * (n_way + 1) <= 64, "at most 64 prototype rows"
    assert qfeat_pm.shape[0] >= (n_groups - 1) * (q_sys_rows or n_query_pts) + n_query_pts
    Z = torch.empty((1 if n_way <= 3 else 2) * n_groups * K * n_query_pts, 4, device=qfeat_pm.device, dtype=torch.float32)
    with _timed("protonet_similarity"):
        _lib.check(_lib.load().r3d_protonet_similarity_sets(
            n_groups, K, _p(qfeat_pm), ldq, n_query_pts if q_sys_rows is None else q_sys_rows, D, _p(tables), (n_way + 1) * D,
            n_way, n_query_pts, code, float(scaler), _p(Z), _st()))
    return Z


def head_fit_table(fits, device):
    """The device table r3d_head_attach_queries_sets reads: per fitted.FittedHead the addresses of its nodes, label rows,
    desc and cluster counts, (K, 4) int64.  The fits must share pitch, label rows and prototype capacity (fits of one
    model do) and stay alive while the table is used."""
    f0 = fits[0]
    rows = []
    for f in fits:
        assert (f.nodes.stride(0), f.nodes.shape[1], f.label_rows, f.proto_cap) == \
            (f0.nodes.stride(0), f0.nodes.shape[1], f0.label_rows, f0.proto_cap), "fits of different geometry"
        assert f.nodes.dtype == torch.float32 and f.Y.dtype == torch.float32 and f.desc.dtype == torch.int32
        assert f.nodes.data_ptr() % 16 == 0 and f.Y.data_ptr() % 16 == 0 and f.nodes.stride(0) % 4 == 0
        assert f.Y.numel() >= 4 * f.label_rows and f.desc.numel() >= HD_WORDS and f.cluster_count.numel() >= f.proto_cap
        rows.append([f.nodes.data_ptr(), f.Y.data_ptr(), f.desc.data_ptr(), f.cluster_count.data_ptr()])
    return torch.tensor(rows, dtype=torch.int64).to(device)


def head_attach_queries_sets(hb, fits, table, qfeat_pm, q_sys_rows=None):
    """head_attach_queries for K fits at once: hb.E = G * K systems, system g * K + k from fits[k] and query group g, one
    launch.  table: head_fit_table(fits).  Per system the bits head_attach_queries gives it."""
    _, ldq = _rows(qfeat_pm)
    K, f0 = len(fits), fits[0]
    assert tuple(table.shape) == (K, 4) and table.dtype == torch.int64 and table.is_cuda and table.is_contiguous()
    assert hb.E % K == 0 and qfeat_pm.shape[1] == hb.D and f0.nodes.shape[1] == hb.D
    G = hb.E // K
    step = hb.n_q_pts if q_sys_rows is None else q_sys_rows
    assert qfeat_pm.shape[0] >= (G - 1) * step + hb.n_q_pts
    with _timed("head_attach_queries"):
        _lib.check(_lib.load().r3d_head_attach_queries_sets(
            G, K, _p(table), f0.nodes.stride(0), f0.label_rows, f0.proto_cap, _p(qfeat_pm), ldq, step, hb.n_way, hb.D,
            hb.n_q_pts, _p(hb.nodes), hb.nodes.stride(0), hb.n_cap, _p(hb.Y), _p(hb.desc), HD_WORDS, _p(hb.cluster_count), hb.n_cap,
            _st()))


def protonet_head_train(sfeat_pm, qfeat_pm, support_y, n_way, k_shot, N, method, scaler=10.0, n_ep=1, feat_ep_rows=0,
                        n_query_pts=None):
    """Training forward of the ProtoNet head -> (Z, ws): the similarity rows of protonet_head (n_ep > 1: (n_ep * n_query_pts, 4)
    per plane, episode after episode) and the scratch protonet_head_bwd needs.  sfeat_pm / qfeat_pm: the support / query rows
    of episode 0 (views into ONE feature matrix in which episode e's rows start feat_ep_rows rows further on)."""
    _, ldf = _rows(sfeat_pm)
    Mq, ldq = _rows(qfeat_pm)
    n_pts = Mq if n_query_pts is None else n_query_pts
    code = _proto_method(method)
    D = sfeat_pm.shape[1]
    sy = support_y.reshape(n_ep * n_way * k_shot, N).to(torch.int32).contiguous()
    dev = sfeat_pm.device
    lib = _lib.load()
    words = lib.r3d_protonet_head_train_ws_words(n_ep, n_way, k_shot, N, n_pts, D)
    if words < 0:
        raise NotImplementedError("ProtoNet head: 1 <= n_way <= 7 and feature width <= 256 (n_way=%d, D=%d)" % (n_way, D))
    ws = torch.empty(words, device=dev, dtype=torch.float32)
    Z = torch.empty((1 if n_way <= 3 else 2) * n_ep * n_pts, 4, device=dev, dtype=torch.float32)  # (planes of 4 classes)
    _lib.check(lib.r3d_protonet_head_train_fwd(n_ep, _p(sfeat_pm), ldf, _p(qfeat_pm), ldq, feat_ep_rows, D, _p(sy), n_way, k_shot,
                                               N, n_pts, code, float(scaler), _p(Z), _p(ws), words, _st()))
    return Z, ws


def protonet_head_bwd(qfeat_pm, support_y, n_way, k_shot, N, method, dZ, ws, dsfeat, dqfeat, scaler=10.0, n_ep=1,
                      feat_ep_rows=0, dfeat_ep_rows=0, n_query_pts=None):
    """Backward of protonet_head_train: dZ (the layout of Z) -> dsfeat (S*N rows), dqfeat (n_query_pts rows), WRITTEN into the
    given 2-D views (their own leading dimensions; episode e dfeat_ep_rows rows further on in both)."""
    Mq, ldq = _rows(qfeat_pm)
    _, ldds = _rows(dsfeat)
    _, lddq = _rows(dqfeat)
    n_pts = Mq if n_query_pts is None else n_query_pts
    D = qfeat_pm.shape[1]
    assert dsfeat.shape[1] == D and dqfeat.shape[1] == D and dZ.dtype == torch.float32 and dZ.is_contiguous()
    assert dZ.numel() == (1 if n_way <= 3 else 2) * n_ep * n_pts * 4
    sy = support_y.reshape(n_ep * n_way * k_shot, N).to(torch.int32).contiguous()
    _lib.check(_lib.load().r3d_protonet_head_bwd(n_ep, _p(qfeat_pm), ldq, feat_ep_rows, D, _p(sy), n_way, k_shot, N, n_pts,
                                                 _proto_method(method), float(scaler), _p(dZ), _p(dsfeat), ldds, _p(dqfeat),
                                                 lddq, dfeat_ep_rows, _p(ws), ws.numel(), _st()))
    return dsfeat, dqfeat


def count_correct(pred, labels):
    """pred (E, ...) int32, labels (E, ...) int64 -> (E,) int32 on the device: per episode the number of points with
    pred == label (one host read then serves a whole batch's accuracies)."""
    E = pred.shape[0]
    assert pred.dtype == torch.int32 and labels.dtype == torch.int64 and pred.is_contiguous() and labels.is_contiguous()
    assert pred.numel() == labels.numel()
    correct = torch.empty(E, device=pred.device, dtype=torch.int32)
    _lib.check(_lib.load().r3d_count_correct_batched(E, _p(pred), _p(labels), pred.numel() // E, _p(correct), _st()))
    return correct


def miou_accumulate(pred, gt, lut, hist):
    """hist (3, n_classes) int64 += counts of this episode (eval_noise.py:39-62)."""
    pred = pred.to(torch.int32).contiguous()
    gt = gt.to(torch.int64).contiguous()
    _lib.check(_lib.load().r3d_miou_accumulate(_p(pred), _p(gt), pred.numel(), _p(lut), lut.numel(), hist.shape[1],
                                               _p(hist), _st()))
    return hist


def augment_clouds(x, out, scale, rot, mirror_prob, jitter, seed, first_key=0, xyz_ch=0, XYZ_ch=-1, seed_dev=None, mats=None,
                   noise=None, mats_out=None):
    """r3d_augment_clouds on x (B, C, N) fp32 -> out (B, C, N) fp32 (out may BE x): the reference's --pc_augm transform of
    prepared clouds (dataloaders/loader.py:205-213,354-373).  Either tensor is read as it lies -- contiguous channel-major
    or a transposed view of point-major rows (is_point_major_view): its three strides travel with it.  seed_dev: a device
    uint32/int32 word added to seed; mats (B, 9) / noise (B, N, 3): given matrices / jitter instead of drawn ones;
    mats_out (B, 9): receives the matrices used.  augment.augment_clouds is the surface with defaults and allocation."""
    assert x.dim() == 3 and x.shape == out.shape and x.dtype == torch.float32 and out.dtype == torch.float32 and x.is_cuda \
        and out.is_cuda, "expected two (B, C, N) fp32 CUDA tensors of one shape"
    B, C, N = x.shape
    for t, shape in ((mats, (B, 9)), (noise, (B, N, 3)), (mats_out, (B, 9))):
        assert t is None or (tuple(t.shape) == shape and t.dtype == torch.float32 and t.is_contiguous() and t.is_cuda), \
            "mats / mats_out (B, 9), noise (B, N, 3): contiguous fp32 CUDA tensors"
    assert seed_dev is None or (seed_dev.numel() == 1 and seed_dev.element_size() == 4 and seed_dev.is_cuda)
    xs, os_ = x.stride(), out.stride()
    _lib.check(_lib.load().r3d_augment_clouds(_p(x), xs[0], xs[1], xs[2], _p(out), os_[0], os_[1], os_[2], B, C, N, xyz_ch,
                                              XYZ_ch, float(scale), int(rot), float(mirror_prob), int(bool(jitter)),
                                              int(seed) & 0xffffffff, _p(seed_dev), int(first_key) & 0xffffffff, _p(mats),
                                              _p(noise), _p(mats_out), _st()))
    return out


# ---------------------------------------------------------------------------------------------- labelling a scan (scene.py)
SCENE_WS_NAMES = ("order", "sorted_key", "pos", "cell_start", "block_points", "block_chunk0", "chunk_block", "rec")


def scene_bounds(scan):
    """scan (M, ld) fp32 on the device -> the (8,) fp32 device record of r3d_scene_bounds: min x, min y, max x, max y over
    the valid points, then their count as int32 bits."""
    assert scan.dim() == 2 and scan.dtype == torch.float32 and scan.is_cuda and scan.is_contiguous()
    lib = _lib.load()
    M, ld = scan.shape
    words = lib.r3d_scene_bounds_ws_words(M)
    ws = torch.empty(max(words, 1), device=scan.device, dtype=torch.float32)
    rec = torch.empty(8, device=scan.device, dtype=torch.float32)
    _lib.check(lib.r3d_scene_bounds(_p(scan), ld, M, _p(rec), _p(ws), ws.numel(), _st()))
    return rec


def scene_workspace(M, ncx, ncy, chunk_cap, device):
    """-> (ws int32 of r3d_scene_ws_words words, {name: word offset}) for SCENE_WS_NAMES."""
    lib = _lib.load()
    words = lib.r3d_scene_ws_words(M, ncx, ncy, chunk_cap)
    if words < 0:
        raise ValueError("scene: M %d, %d x %d cells, chunk_cap %d out of range" % (M, ncx, ncy, chunk_cap))
    offs = (ctypes.c_long * 8)()
    _lib.check(lib.r3d_scene_ws_offsets(M, ncx, ncy, chunk_cap, offs))
    return torch.empty(words, device=device, dtype=torch.int32), dict(zip(SCENE_WS_NAMES, list(offs)))


def scene_plan(scan, x0, y0, s, ncx, ncy, r, N, min_points, chunk_cap, ws):
    M, ld = scan.shape
    _lib.check(_lib.load().r3d_scene_plan(_p(scan), ld, M, float(x0), float(y0), float(s), ncx, ncy, r, N, min_points,
                                          chunk_cap, _p(ws), ws.numel(), _st()))


def scene_prepare(scan, ncx, ncy, r, N, chunk_cap, ws, first_chunk, out, rgb_ch, XYZ_ch, slot_map=None, sws=None):
    """Chunks first_chunk .. first_chunk + G - 1 -> out (G, C, N) fp32, read as it lies (contiguous channel-major or a
    transposed view of point-major rows: its strides travel with it).  slot_map (G, N) int32: the scan index per slot.
    sws (the sparse workspace after scene_run_tables): first_chunk numbers the chunks that run under the cap; None: no cap."""
    assert out.dim() == 3 and out.dtype == torch.float32 and out.is_cuda
    G, C, N_ = out.shape
    assert N_ == N and (slot_map is None or (tuple(slot_map.shape) == (G, N) and slot_map.dtype == torch.int32
                                             and slot_map.is_contiguous() and slot_map.is_cuda))
    M, ld = scan.shape
    os_ = out.stride()
    _lib.check(_lib.load().r3d_scene_prepare(_p(scan), ld, M, ncx, ncy, r, N, chunk_cap, _p(ws), ws.numel(), _p(sws),
                                             0 if sws is None else sws.numel(), first_chunk, G, C, rgb_ch, XYZ_ch, _p(out),
                                             os_[0], os_[1], os_[2], _p(slot_map), _st()))
    return out


def scene_vote(M, ncx, ncy, r, N, chunk_cap, ws, logits, sws=None):
    """logits (n_chunks, n_classes, N) fp32 contiguous -> (scores (M, n_classes) fp32, labels (M,) int64, votes (M,) int32).
    sws (the sparse workspace after scene_run_tables): logits of the chunks that run; an appearance counts when its chunk ran."""
    assert logits.dim() == 3 and logits.shape[2] == N and logits.dtype == torch.float32 and logits.is_contiguous() and logits.is_cuda
    n_chunks, K = logits.shape[0], logits.shape[1]
    dev = logits.device
    scores = torch.empty(M, K, device=dev, dtype=torch.float32)
    labels = torch.empty(M, device=dev, dtype=torch.int64)
    votes = torch.empty(M, device=dev, dtype=torch.int32)
    _lib.check(_lib.load().r3d_scene_vote(M, ncx, ncy, r, N, chunk_cap, _p(ws), ws.numel(), _p(sws),
                                          0 if sws is None else sws.numel(), _p(logits), n_chunks, K, _p(scores), _p(labels),
                                          _p(votes), _st()))
    return scores, labels, votes


# ---- predict_scene on a subsample: a cap on the chunks of a block, the transfer to the points without a vote
SCENE_SPARSE_WS_NAMES = ("run_chunk0", "run_block", "voted_before", "unvoted", "tile0", "cand", "rec", "part")


def scene_sparse_workspace(M, ncx, ncy, chunk_cap, device):
    """-> (sws int32 of r3d_scene_sparse_ws_words words, {name: word offset}) for SCENE_SPARSE_WS_NAMES."""
    lib = _lib.load()
    words = lib.r3d_scene_sparse_ws_words(M, ncx, ncy, chunk_cap)
    if words < 0:
        raise ValueError("scene: M %d, %d x %d cells, chunk_cap %d out of range" % (M, ncx, ncy, chunk_cap))
    offs = (ctypes.c_long * 8)()
    _lib.check(lib.r3d_scene_sparse_ws_offsets(M, ncx, ncy, chunk_cap, offs))
    return torch.empty(words, device=device, dtype=torch.int32), dict(zip(SCENE_SPARSE_WS_NAMES, list(offs)))


def scene_run_tables(M, ncx, ncy, r, N, chunk_cap, ws, max_chunks, sws):
    """After scene_plan, before the plan record is read: the run tables of cap max_chunks into sws, the counts into the record."""
    _lib.check(_lib.load().r3d_scene_run_tables(M, ncx, ncy, r, N, chunk_cap, _p(ws), ws.numel(), int(max_chunks), _p(sws),
                                                sws.numel(), _st()))


def _scene_transfer(scan, ncx, ncy, chunk_cap, ws, sws, scores, labels, votes, idw):
    M, ld = scan.shape
    assert scan.is_contiguous() and scores.is_contiguous() and tuple(scores.shape[:1]) == (M,) and scores.dtype == torch.float32
    assert tuple(labels.shape) == (M,) and labels.dtype == torch.int64 and tuple(votes.shape) == (M,) and votes.dtype == torch.int32
    source = torch.empty(M, device=scan.device, dtype=torch.int64)
    neighbours = torch.empty(M, 3, device=scan.device, dtype=torch.int64) if idw else None
    weights = torch.empty(M, 3, device=scan.device, dtype=torch.float32) if idw else None
    _lib.check(_lib.load().r3d_scene_transfer(_p(scan), ld, M, ncx, ncy, chunk_cap, _p(ws), ws.numel(), _p(sws), sws.numel(),
                                              scores.shape[1], _p(scores), _p(labels), _p(votes), _p(source), _p(neighbours),
                                              _p(weights), _st()))
    return source, neighbours, weights


def scene_transfer(scan, ncx, ncy, chunk_cap, ws, sws, scores, labels, votes):
    """In place: scores (M, K) fp32 and labels (M,) int64 of the points with votes == 0 from their nearest voted neighbour
    in the 3 x 3 cells -> source (M,) int64; the count of receivers is word 0 of the sparse record, on the device."""
    return _scene_transfer(scan, ncx, ncy, chunk_cap, ws, sws, scores, labels, votes, False)[0]


def scene_transfer_idw(scan, ncx, ncy, chunk_cap, ws, sws, scores, labels, votes):
    """In place: scores (M, K) fp32 and labels (M,) int64 of the points with votes == 0 from the three nearest voted points
    of the 3 x 3 cells, their mean logits weighted by 1 / (d + 1e-8) -> (source (M,) int64, neighbours (M, 3) int64,
    weights (M, 3) fp32); the count of receivers is word 0 of the sparse record, on the device."""
    return _scene_transfer(scan, ncx, ncy, chunk_cap, ws, sws, scores, labels, votes, True)


# ---- predict_scene_sets: the scores of K support sets merged into one label per point
def scene_merge_sets(scores, votes, source, classes, background):
    """scores (M, K, C) fp32 contiguous (C = n_way + 1, K * C <= 64), votes (M,) int32, source (M,) int64 or None, classes
    (K, C - 1) int32 on the device, background: an int -> (set_labels (M, K) int64, labels (M,) int64, set_of (M,) int32,
    margin (M,) fp32): step 10 of predict_scene_sets (r3d_scene_merge_sets in include/r3d.h)."""
    assert scores.dim() == 3 and scores.dtype == torch.float32 and scores.is_contiguous() and scores.is_cuda
    M, K, C = scores.shape
    assert tuple(votes.shape) == (M,) and votes.dtype == torch.int32 and votes.is_contiguous()
    assert source is None or (tuple(source.shape) == (M,) and source.dtype == torch.int64 and source.is_contiguous())
    assert tuple(classes.shape) == (K, C - 1) and classes.dtype == torch.int32 and classes.is_contiguous() and classes.is_cuda
    dev = scores.device
    set_labels = torch.empty(M, K, device=dev, dtype=torch.int64)
    labels = torch.empty(M, device=dev, dtype=torch.int64)
    set_of = torch.empty(M, device=dev, dtype=torch.int32)
    margin = torch.empty(M, device=dev, dtype=torch.float32)
    _lib.check(_lib.load().r3d_scene_merge_sets(M, K, C, _p(scores), _p(votes), _p(source), _p(classes), int(background),
                                                _p(set_labels), _p(labels), _p(set_of), _p(margin), _st()))
    return set_labels, labels, set_of, margin


# ---- fit_scene: the support set from an annotated scan (scene_support.py)


def _label_bytes(labels, M):
    assert labels.is_cuda and labels.is_contiguous() and tuple(labels.shape) == (M,) and labels.dtype in (torch.int32, torch.int64)
    return labels.element_size()


def scene_support_counts(M, ncx, ncy, r, N, chunk_cap, ws, labels, classes):
    """labels (M,) int32 or int64 on the device, read as they are; classes (n_way,) int32 on the device -> fg (blocks, n_way)
    int32: per block of the plan in ws the members of its cloud (chunk 0) labelled classes[w], 0 for a dropped block."""
    assert classes.is_cuda and classes.dtype == torch.int32 and classes.is_contiguous() and classes.dim() == 1
    n_way = classes.numel()
    nb = max(ncx - r + 1, 1) * max(ncy - r + 1, 1)
    fg = torch.empty(nb, n_way, device=labels.device, dtype=torch.int32)
    _lib.check(_lib.load().r3d_scene_support_counts(M, ncx, ncy, r, N, chunk_cap, _p(ws), ws.numel(), _p(labels),
                                                    _label_bytes(labels, M), _p(classes), n_way, _p(fg), _st()))
    return fg


def scene_support_pick(M, ncx, ncy, r, N, chunk_cap, ws, fg, k_shot, min_ratio, min_fg):
    """fg (blocks, n_way) int32 -> (shot_block (n_way, k_shot) int32, shot_fg (n_way, k_shot) int32, rec (8,) int32 whose
    word w counts way w's eligible blocks): per way the eligible blocks by fg descending, then block id ascending."""
    assert fg.is_cuda and fg.dtype == torch.int32 and fg.is_contiguous() and fg.dim() == 2
    n_way = fg.shape[1]
    assert fg.shape[0] == max(ncx - r + 1, 1) * max(ncy - r + 1, 1)
    shot_block = torch.empty(n_way, k_shot, device=fg.device, dtype=torch.int32)
    shot_fg = torch.empty(n_way, k_shot, device=fg.device, dtype=torch.int32)
    rec = torch.empty(8, device=fg.device, dtype=torch.int32)
    _lib.check(_lib.load().r3d_scene_support_pick(M, ncx, ncy, r, N, chunk_cap, _p(ws), ws.numel(), _p(fg), n_way, k_shot,
                                                  float(min_ratio), int(min_fg), _p(shot_block), _p(shot_fg), _p(rec), _st()))
    return shot_block, shot_fg, rec


def scene_prepare_blocks(scan, ncx, ncy, r, N, chunk_cap, ws, blocks, out, rgb_ch, XYZ_ch, slot_map=None, labels=None,
                         cloud_class=None, mask=None):
    """Chunk 0 of every block in blocks (G,) int32 on the device -> out (G, C, N) fp32, read as it lies, with the bits of
    scene_prepare on that chunk; slot_map (G, N) int32.  labels (M,), cloud_class (G,) int32 and mask (G, N) int32, all or
    none: mask[g, t] = (labels[slot_map[g, t]] == cloud_class[g])."""
    assert out.dim() == 3 and out.dtype == torch.float32 and out.is_cuda
    G, C, N_ = out.shape
    i32 = lambda t, shape: t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and tuple(t.shape) == shape
    assert N_ == N and i32(blocks, (G,)) and (slot_map is None or i32(slot_map, (G, N)))
    M, ld = scan.shape
    nbytes = 0
    if labels is not None or cloud_class is not None or mask is not None:
        assert i32(cloud_class, (G,)) and i32(mask, (G, N))
        nbytes = _label_bytes(labels, M)
    os_ = out.stride()
    _lib.check(_lib.load().r3d_scene_prepare_blocks(_p(scan), ld, M, ncx, ncy, r, N, chunk_cap, _p(ws), ws.numel(), _p(blocks), G,
                                                    C, rgb_ch, XYZ_ch, _p(out), os_[0], os_[1], os_[2], _p(slot_map),
                                                    _p(labels), nbytes, _p(cloud_class), _p(mask), _st()))
    return out


# ---- pool_segments: scores pooled over user-given segments (scene_segments.py)


def _scene_workspace(what, name, M, device):
    """-> ws, int32 of r3d_scene_<what>_ws_words(M) words: the one scratch of a call of `name`, its record in front."""
    words = getattr(_lib.load(), "r3d_scene_%s_ws_words" % what)(M)
    if words < 0:
        raise ValueError("%s: %d points (1 .. 2^27)" % (name, M))
    return torch.empty(words, device=device, dtype=torch.int32)


def _grid_args(grid, origin=None, voxel=None):
    """-> (nx, ny, nz) as the entry points take them; with an origin, (x0, y0, z0, voxel) in front."""
    cells = tuple(int(n) for n in grid)
    return cells if origin is None else tuple(float(v) for v in origin) + (float(voxel),) + cells


def scene_seg_workspace(M, device):
    return _scene_workspace("seg", "pool_segments", M, device)


def _seg_ws_ok(ws):
    return ws.is_cuda and ws.dtype == torch.int32 and ws.is_contiguous() and ws.dim() == 1


def scene_seg_ids(segments, ws):
    """segments (M,) int32 or int64 on the device, read as they are -> words 0 .. 5 of the record in ws, on the device."""
    M = segments.numel()
    assert _seg_ws_ok(ws)
    _lib.check(_lib.load().r3d_scene_seg_ids(_p(segments), _label_bytes(segments, M), M, _p(ws), ws.numel(), _st()))


def scene_seg_group(segments, votes, max_id, n_negative, ws):
    """After scene_seg_ids and the read of its record: the sort by (id, scan index), the segment and tile tables into ws,
    words 6 .. 8 of the record -> segment_index (M,) int32."""
    M = segments.numel()
    assert _seg_ws_ok(ws)
    assert tuple(votes.shape) == (M,) and votes.dtype == torch.int32 and votes.is_contiguous() and votes.is_cuda
    segment_index = torch.empty(M, device=segments.device, dtype=torch.int32)
    _lib.check(_lib.load().r3d_scene_seg_group(_p(segments), _label_bytes(segments, M), M, _p(votes), int(max_id), int(n_negative),
                                               _p(segment_index), _p(ws), ws.numel(), _st()))
    return segment_index


def scene_seg_pool(scores, votes, n_segments, n_tiles, ws, want_labels=True):
    """scores (M, cols) fp32 contiguous, cols <= 64; n_segments, n_tiles as read from the record -> (segment_ids (S,) int64,
    segment_points (S,) int32, segment_members (S,) int32, segment_scores (S, cols) fp32, segment_labels (S,) int64 or None)."""
    assert scores.dim() == 2 and scores.dtype == torch.float32 and scores.is_contiguous() and scores.is_cuda
    M, C = scores.shape
    assert tuple(votes.shape) == (M,) and votes.dtype == torch.int32 and votes.is_contiguous() and _seg_ws_ok(ws)
    dev, S = scores.device, int(n_segments)
    part = torch.empty(int(n_tiles), C, device=dev, dtype=torch.float32)
    ids = torch.empty(S, device=dev, dtype=torch.int64)
    points = torch.empty(S, device=dev, dtype=torch.int32)
    members = torch.empty(S, device=dev, dtype=torch.int32)
    seg_scores = torch.empty(S, C, device=dev, dtype=torch.float32)
    seg_labels = torch.empty(S, device=dev, dtype=torch.int64) if want_labels else None
    nz = lambda t: _p(t) if t is not None and t.numel() else None
    _lib.check(_lib.load().r3d_scene_seg_pool(M, C, _p(scores), _p(votes), S, int(n_tiles), _p(ws), ws.numel(), nz(part), nz(ids),
                                              nz(points), nz(members), nz(seg_scores), nz(seg_labels), _st()))
    return ids, points, members, seg_scores, seg_labels


def scene_seg_spread(min_members, segment_index, seg_members, seg_fields, in_fields, ws):
    """seg_fields / in_fields: (scores (rows, cols), labels (rows,) int64, set_labels (rows, K) int64 or None, set_of (rows,)
    int32 or None, margin (rows,) fp32 or None) of the segments and of res -> the same five for the scan, freshly
    allocated, and pooled (M,) bool; words 9 .. 11 of the record."""
    sc_in, lab_in, sl_in, so_in, mg_in = in_fields
    sc_seg, lab_seg, sl_seg, so_seg, mg_seg = seg_fields
    assert sc_in.dim() == 2 and sc_in.dtype == torch.float32 and sc_in.is_contiguous() and sc_in.is_cuda
    M, C = sc_in.shape
    S = sc_seg.shape[0]
    K = 0 if sl_in is None else sl_in.shape[1]
    ok = lambda t, shape, dt: tuple(t.shape) == shape and t.dtype == dt and t.is_contiguous() and t.is_cuda
    assert ok(segment_index, (M,), torch.int32) and ok(seg_members, (S,), torch.int32) and _seg_ws_ok(ws)
    assert ok(lab_in, (M,), torch.int64) and ok(sc_seg, (S, C), torch.float32) and ok(lab_seg, (S,), torch.int64)
    if K:
        assert ok(sl_in, (M, K), torch.int64) and ok(so_in, (M,), torch.int32) and ok(mg_in, (M,), torch.float32)
        assert ok(sl_seg, (S, K), torch.int64) and ok(so_seg, (S,), torch.int32) and ok(mg_seg, (S,), torch.float32)
    else:
        assert all(t is None for t in (sl_in, so_in, mg_in, sl_seg, so_seg, mg_seg))
    dev = sc_in.device
    scores, labels = torch.empty_like(sc_in), torch.empty_like(lab_in)
    pooled = torch.empty(M, device=dev, dtype=torch.bool)
    set_labels, set_of, margin = (torch.empty_like(sl_in), torch.empty_like(so_in), torch.empty_like(mg_in)) if K else (None,) * 3
    nz = lambda t: _p(t) if t is not None and t.numel() else None
    _lib.check(_lib.load().r3d_scene_seg_spread(M, C, K, S, int(min_members), _p(segment_index), nz(seg_members), nz(sc_seg),
                                                nz(lab_seg), nz(sl_seg), nz(so_seg), nz(mg_seg), _p(sc_in), _p(lab_in), _p(sl_in),
                                                _p(so_in), _p(mg_in), _p(scores), _p(labels), _p(pooled), _p(set_labels),
                                                _p(set_of), _p(margin), _p(ws), ws.numel(), _st()))
    return scores, labels, set_labels, set_of, margin, pooled


# ---- build_segments: segments grown from the scan (scene_grow.py)


def scene_grow_workspace(M, device):
    return _scene_workspace("grow", "build_segments", M, device)


def _grow_scan_ok(scan):
    return scan.dim() == 2 and scan.dtype == torch.float32 and scan.is_cuda and scan.is_contiguous()


def scene_grow_bounds(scan, ws):
    """scan (M, ld) fp32 on the device -> words 0 .. 6 of the record in ws (zeros in the others), on the device."""
    assert _grow_scan_ok(scan) and _seg_ws_ok(ws)
    M, ld = scan.shape
    _lib.check(_lib.load().r3d_scene_grow_bounds(_p(scan), ld, M, _p(ws), ws.numel(), _st()))


def scene_grow_sort(scan, origin, voxel, grid, ws):
    """origin (x0, y0, z0) as read from the record, grid (nx, ny, nz): keys, the sort, the voxel heads -> word 7 (V)."""
    assert _grow_scan_ok(scan) and _seg_ws_ok(ws)
    M, ld = scan.shape
    _lib.check(_lib.load().r3d_scene_grow_sort(_p(scan), ld, M, *_grid_args(grid, origin, voxel), _p(ws), ws.numel(), _st()))


def scene_grow_voxels(scan, grid, n_valid, n_voxels, colour, ws):
    """After the read of V: the voxel table into ws -> (voxel_index (M,) int32, voxel_mean (V, 3) fp32 or None without
    colour)."""
    assert _grow_scan_ok(scan) and _seg_ws_ok(ws)
    M, ld = scan.shape
    voxel_index = torch.empty(M, device=scan.device, dtype=torch.int32)
    voxel_mean = torch.empty(int(n_voxels), 3, device=scan.device, dtype=torch.float32) if colour else None
    _lib.check(_lib.load().r3d_scene_grow_voxels(_p(scan), ld, M, *_grid_args(grid), int(n_valid), int(n_voxels),
                                                 _p(voxel_index), _p(voxel_mean), _p(ws), ws.numel(), _st()))
    return voxel_index, voxel_mean


def scene_grow_union(M, grid, n_voxels, connectivity, voxel_mean, colour_tol, ws):
    """The union-find over the voxel graph, in ws; voxel_mean None: adjacency alone."""
    assert _seg_ws_ok(ws)
    assert voxel_mean is None or (tuple(voxel_mean.shape) == (int(n_voxels), 3) and voxel_mean.dtype == torch.float32
                                  and voxel_mean.is_contiguous() and voxel_mean.is_cuda and colour_tol is not None)
    _lib.check(_lib.load().r3d_scene_grow_union(M, *_grid_args(grid), int(n_voxels), int(connectivity), _p(voxel_mean),
                                                0.0 if voxel_mean is None else float(colour_tol), _p(ws), ws.numel(), _st()))


def _grow_table_ok(t, n_voxels):
    return (tuple(t.shape) == (int(n_voxels), 3) and t.dtype == torch.float32 and t.is_contiguous() and t.is_cuda)


def scene_grow_centroids(scan, origin, voxel, grid, n_voxels, ws):
    """With normal_tol, after scene_grow_voxels: origin, voxel, grid as given to scene_grow_sort -> voxel_centroid (V, 3) fp32,
    the mean offset of a voxel's points inside the voxel (G3c)."""
    assert _grow_scan_ok(scan) and _seg_ws_ok(ws)
    M, ld = scan.shape
    centroid = torch.empty(int(n_voxels), 3, device=scan.device, dtype=torch.float32)
    _lib.check(_lib.load().r3d_scene_grow_centroids(_p(scan), ld, M, *_grid_args(grid, origin, voxel), int(n_voxels), _p(centroid),
                                                    _p(ws), ws.numel(), _st()))
    return centroid


def scene_grow_normals(M, grid, n_voxels, voxel, voxel_centroid, ws):
    """-> (voxel_normal (V, 3) fp32, a NaN row where a voxel has no normal, voxel_support (V,) int32: the occupied voxels among
    the 27 around it) by G3n."""
    assert _seg_ws_ok(ws) and _grow_table_ok(voxel_centroid, n_voxels)
    normal = torch.empty_like(voxel_centroid)
    support = torch.empty(int(n_voxels), device=voxel_centroid.device, dtype=torch.int32)
    _lib.check(_lib.load().r3d_scene_grow_normals(M, *_grid_args(grid), int(n_voxels), float(voxel), _p(voxel_centroid),
                                                  _p(normal), _p(support), _p(ws), ws.numel(), _st()))
    return normal, support


def scene_grow_union_normals(M, grid, n_voxels, connectivity, voxel_mean, colour_tol, voxel_normal, cos2, ws):
    """scene_grow_union with the normal test of G4 as well: voxel_normal (V, 3) fp32, cos2 the float32 squared cosine of the
    tolerance; voxel_mean None: no colour test."""
    assert _seg_ws_ok(ws) and _grow_table_ok(voxel_normal, n_voxels)
    assert voxel_mean is None or (_grow_table_ok(voxel_mean, n_voxels) and colour_tol is not None)
    _lib.check(_lib.load().r3d_scene_grow_union_normals(M, *_grid_args(grid), int(n_voxels), int(connectivity),
                                                        _p(voxel_mean), 0.0 if voxel_mean is None else float(colour_tol),
                                                        _p(voxel_normal), float(cos2), _p(ws), ws.numel(), _st()))


def scene_grow_components(M, n_voxels, min_points, ws):
    """Roots, points per root, kept roots and their scan, in ws -> words 8 (components), 9 (S) and 11 (error)."""
    assert _seg_ws_ok(ws)
    _lib.check(_lib.load().r3d_scene_grow_components(M, int(n_voxels), int(min(min_points, 2 ** 31 - 1)), _p(ws), ws.numel(), _st()))


def scene_grow_absorb(M, grid, n_voxels, connectivity, rings, ws):
    """With absorb > 0, after the read of S and before scene_grow_ids: `rings` rounds of G6a on the tables in ws -> voxel_ring
    (V,) int32: 0 for a voxel of a kept component, the round that took an absorbed one, -1 for one still free; words 12
    (absorbed voxels) and 13 (absorbed points)."""
    assert _seg_ws_ok(ws)
    ring = torch.empty(int(n_voxels), device=ws.device, dtype=torch.int32)
    _lib.check(_lib.load().r3d_scene_grow_absorb(M, *_grid_args(grid), int(n_voxels), int(connectivity), int(rings),
                                                 _p(ring), _p(ws), ws.numel(), _st()))
    return ring


def scene_grow_ids(voxel_index, n_voxels, n_segments, ws):
    """After the read of S -> (segments (M,) int32, segment_points (S,) int32); word 10 (points of dropped components)."""
    assert _seg_ws_ok(ws) and voxel_index.dtype == torch.int32 and voxel_index.is_contiguous() and voxel_index.is_cuda
    M, S = voxel_index.numel(), int(n_segments)
    segments = torch.empty(M, device=voxel_index.device, dtype=torch.int32)
    segment_points = torch.empty(S, device=voxel_index.device, dtype=torch.int32)
    _lib.check(_lib.load().r3d_scene_grow_ids(M, int(n_voxels), S, _p(voxel_index), _p(segments),
                                              _p(segment_points) if S else None, _p(ws), ws.numel(), _st()))
    return segments, segment_points


# ---- smooth_scene: scores propagated over the voxel graph (scene_smooth.py), on the workspace of build_segments


def _smooth_ok(t, shape, dtype):
    return tuple(t.shape) == tuple(shape) and t.dtype == dtype and t.is_contiguous() and t.is_cuda


def scene_smooth_evidence(scores, votes, grid, n_voxels, ws):
    """After scene_grow_voxels: scores (M, C) fp32, votes (M,) int32 of the result -> (voxel_evidence (V, C) fp32,
    voxel_members (V,) int32, voxel_ring (V,) int32: 0 with a member, else -1) by S2."""
    M, C = scores.shape
    V, dev = int(n_voxels), scores.device
    assert _smooth_ok(scores, (M, C), torch.float32) and _smooth_ok(votes, (M,), torch.int32) and _seg_ws_ok(ws)
    evidence = torch.empty(V, C, device=dev, dtype=torch.float32)
    members = torch.empty(V, device=dev, dtype=torch.int32)
    ring = torch.empty(V, device=dev, dtype=torch.int32)
    _lib.check(_lib.load().r3d_scene_smooth_evidence(M, *_grid_args(grid), C, _p(scores), _p(votes), V, _p(evidence), _p(members),
                                                     _p(ring), _p(ws), ws.numel(), _st()))
    return evidence, members, ring


def scene_smooth_graph(M, grid, n_voxels, connectivity, voxel_mean, colour_tol, ws):
    """-> voxel_neighbours (26, V) int32 by S3: per voxel the rows of its neighbours in ascending key order, -1 behind them;
    voxel_mean None: adjacency alone."""
    V = int(n_voxels)
    assert _seg_ws_ok(ws) and (voxel_mean is None or (_grow_table_ok(voxel_mean, V) and colour_tol is not None))
    nbr = torch.empty(SCENE_SMOOTH_SLOTS, V, device=ws.device, dtype=torch.int32)
    _lib.check(_lib.load().r3d_scene_smooth_graph(M, *_grid_args(grid), V, int(connectivity), _p(voxel_mean),
                                                  0.0 if voxel_mean is None else float(colour_tol), _p(nbr), _p(ws), ws.numel(), _st()))
    return nbr


def scene_smooth_sweep(M, iterations, alpha, evidence, nbr, ring):
    """`iterations` sweeps of S4, queued without a host read; ring is updated in place -> voxel_scores (V, C) fp32, a tensor
    of its own (without a sweep: a copy of evidence)."""
    V, C = evidence.shape
    n = int(iterations)
    assert _smooth_ok(evidence, (V, C), torch.float32) and _smooth_ok(nbr, (SCENE_SMOOTH_SLOTS, V), torch.int32)
    assert _smooth_ok(ring, (V,), torch.int32)
    if n == 0:
        return evidence.clone()
    z = [torch.empty_like(evidence), torch.empty_like(evidence) if n > 1 else None]
    _lib.check(_lib.load().r3d_scene_smooth_sweep(M, V, C, n, float(alpha), _p(evidence), _p(nbr), _p(z[0]), _p(z[1]), _p(ring),
                                                  _st()))
    return z[(n - 1) & 1]


def scene_smooth_spread(voxel_index, ring, voxel_scores, in_scores, in_labels, in_votes):
    """S5, S6 -> (voxel_labels (V,) int64, scores (M, C) fp32, labels (M,) int64, votes (M,) int32, smoothed (M,) bool, counts
    (8,) int32 on the device: SMOOTH_R_*)."""
    M, C = in_scores.shape
    V, dev = voxel_scores.shape[0], in_scores.device
    assert _smooth_ok(voxel_index, (M,), torch.int32) and _smooth_ok(ring, (V,), torch.int32)
    assert _smooth_ok(voxel_scores, (V, C), torch.float32) and _smooth_ok(in_scores, (M, C), torch.float32)
    assert _smooth_ok(in_labels, (M,), torch.int64) and _smooth_ok(in_votes, (M,), torch.int32)
    voxel_labels = torch.empty(V, device=dev, dtype=torch.int64)
    scores, labels, votes = torch.empty_like(in_scores), torch.empty_like(in_labels), torch.empty_like(in_votes)
    smoothed = torch.empty(M, device=dev, dtype=torch.bool)
    counts = torch.empty(SCENE_SMOOTH_COUNTS, device=dev, dtype=torch.int32)
    _lib.check(_lib.load().r3d_scene_smooth_spread(M, C, V, _p(voxel_index), _p(ring), _p(voxel_scores), _p(in_scores),
                                                   _p(in_labels), _p(in_votes), _p(voxel_labels), _p(scores), _p(labels), _p(votes),
                                                   _p(smoothed), _p(counts), _st()))
    return voxel_labels, scores, labels, votes, smoothed, counts


# ---- extract_objects: objects from a labelled scan (scene_objects.py)


def scene_obj_workspace(M, device):
    return _scene_workspace("obj", "extract_objects", M, device)


def _obj_labels_args(scan, labels, ignore):
    assert labels.dim() == 1 and labels.numel() == scan.shape[0] and labels.dtype in (torch.int32, torch.int64)
    assert labels.is_cuda and labels.is_contiguous()
    n = 0 if ignore is None else ignore.numel()
    assert n == 0 or (ignore.dtype == torch.int64 and ignore.is_cuda and ignore.is_contiguous() and n <= SCENE_OBJ_IGNORE)
    return _p(labels), int(labels.dtype == torch.int64), _p(ignore) if n else None, n


def scene_obj_bounds(scan, labels, ignore, ws):
    """scan (M, ld) fp32, labels (M,) int32 or int64, ignore (n,) int64 or None, all on the device -> words 0 .. 6 and
    12 .. 15 of the record in ws (zeros in the others), on the device."""
    assert _grow_scan_ok(scan) and _seg_ws_ok(ws)
    M, ld = scan.shape
    _lib.check(_lib.load().r3d_scene_obj_bounds(_p(scan), ld, M, *_obj_labels_args(scan, labels, ignore), _p(ws), ws.numel(),
                                                _st()))


def scene_obj_sort(scan, labels, ignore, origin, voxel, grid, n_labels, n_points, ws):
    """origin, n_labels, n_points as read from the record, grid (nx, ny, nz): keys, the sort, the unit heads, the unit table
    -> unit_index (M,) int32, the row of a point's unit or -1; word 7 (the units)."""
    assert _grow_scan_ok(scan) and _seg_ws_ok(ws)
    M, ld = scan.shape
    unit_index = torch.empty(M, device=scan.device, dtype=torch.int32)
    _lib.check(_lib.load().r3d_scene_obj_sort(_p(scan), ld, M, *_obj_labels_args(scan, labels, ignore),
                                              *_grid_args(grid, origin, voxel), int(n_labels), int(n_points), _p(unit_index), _p(ws),
                                              ws.numel(), _st()))
    return unit_index


def scene_obj_union(M, grid, n_labels, n_units, connectivity, ws):
    """The union-find over the units of one class in neighbouring cells, in ws."""
    assert _seg_ws_ok(ws)
    _lib.check(_lib.load().r3d_scene_obj_union(M, *_grid_args(grid), int(n_labels), int(n_units), int(connectivity), _p(ws),
                                               ws.numel(), _st()))


def scene_obj_components(M, n_units, min_points, ws):
    """Roots, points per root, kept roots and their scan, in ws -> words 8 (components), 9 (S) and 11 (error)."""
    assert _seg_ws_ok(ws)
    _lib.check(_lib.load().r3d_scene_obj_components(M, int(n_units), int(min(min_points, 2 ** 31 - 1)), _p(ws), ws.numel(), _st()))


def scene_obj_stats(scan, origin, voxel, grid, n_labels, n_units, n_objects, ws):
    """After the read of S >= 1: the object table -> (object_labels (S,) int64, object_points (S,) int32, object_units (S,)
    int32, object_lo, object_hi, object_centroid (S, 3) fp32)."""
    assert _grow_scan_ok(scan) and _seg_ws_ok(ws) and n_objects >= 1
    M, ld = scan.shape
    S, dev = int(n_objects), scan.device
    labels = torch.empty(S, device=dev, dtype=torch.int64)
    points, units = (torch.empty(S, device=dev, dtype=torch.int32) for _ in range(2))
    lo, hi, centroid = (torch.empty(S, 3, device=dev, dtype=torch.float32) for _ in range(3))
    sums = torch.empty(S, 3, device=dev, dtype=torch.int64)  # the kernels' scratch
    _lib.check(_lib.load().r3d_scene_obj_stats(_p(scan), ld, M, *_grid_args(grid, origin, voxel), int(n_labels), int(n_units), S,
                                               _p(labels), _p(points), _p(units), _p(lo), _p(hi), _p(centroid), _p(sums), _p(ws),
                                               ws.numel(), _st()))
    return labels, points, units, lo, hi, centroid


def scene_obj_ids(unit_index, n_units, n_objects, ws):
    """After the read of S -> objects (M,) int32; word 10 (points of dropped components)."""
    assert _seg_ws_ok(ws) and unit_index.dtype == torch.int32 and unit_index.is_contiguous() and unit_index.is_cuda
    M = unit_index.numel()
    objects = torch.empty(M, device=unit_index.device, dtype=torch.int32)
    _lib.check(_lib.load().r3d_scene_obj_ids(M, int(n_units), int(n_objects), _p(unit_index), _p(objects), _p(ws), ws.numel(),
                                             _st()))
    return objects


# ---- match_objects: a scan's objects against ground-truth instances (scene_match.py)


def scene_match_workspace(M, device):
    return _scene_workspace("match", "match_objects", M, device)


def _match_labels_args(pred_labels, truth_labels, M):
    """-> (pred_labels, bytes, truth_labels, bytes) as the entry points take them; both columns or neither."""
    assert (pred_labels is None) == (truth_labels is None)
    if pred_labels is None:
        return None, 0, None, 0
    return _p(pred_labels), _label_bytes(pred_labels, M), _p(truth_labels), _label_bytes(truth_labels, M)


def scene_match_ids(pred, truth, ignore_unannotated, ws):
    """pred, truth (M,) int32 or int64 on the device, read as they are -> words 0 .. 7 of the record in ws, on the device."""
    M = pred.numel()
    assert _seg_ws_ok(ws)
    _lib.check(_lib.load().r3d_scene_match_ids(_p(pred), _label_bytes(pred, M), _p(truth), _label_bytes(truth, M), M,
                                               int(bool(ignore_unannotated)), _p(ws), ws.numel(), _st()))


def scene_match_rows(pred, truth, pred_labels, truth_labels, ignore_unannotated, max_ids, n_in, ws):
    """After scene_match_ids and the read of its record: max_ids, n_in: per column the largest id and the points with a row.
    Per column the sort by (id, scan index) and the row tables into ws -> (pred_index, truth_index) (M,) int32; words
    8 .. 11 of the record."""
    M = pred.numel()
    assert _seg_ws_ok(ws)
    pred_index, truth_index = (torch.empty(M, device=pred.device, dtype=torch.int32) for _ in range(2))
    _lib.check(_lib.load().r3d_scene_match_rows(_p(pred), _label_bytes(pred, M), _p(truth), _label_bytes(truth, M),
                                                *_match_labels_args(pred_labels, truth_labels, M), M, int(bool(ignore_unannotated)),
                                                int(max_ids[0]), int(max_ids[1]), int(n_in[0]), int(n_in[1]), _p(pred_index),
                                                _p(truth_index), _p(ws), ws.numel(), _st()))
    return pred_index, truth_index


def scene_match_pairs(pred_index, truth_index, pred_labels, truth_labels, n_pred, n_truth, ws):
    """After the read of P and T (both >= 1): the row tables -> ((pred_ids (P,) int64, pred_points (P,) int32, pred_classes
    (P,) int64 or None), the same for truth); the two sorts and the pair tables into ws; words 12 and 13 of the record."""
    M = pred_index.numel()
    ok = lambda t: tuple(t.shape) == (M,) and t.dtype == torch.int32 and t.is_contiguous() and t.is_cuda
    assert _seg_ws_ok(ws) and ok(pred_index) and ok(truth_index) and n_pred >= 1 and n_truth >= 1
    dev = pred_index.device

    def tables(n):
        return (torch.empty(n, device=dev, dtype=torch.int64), torch.empty(n, device=dev, dtype=torch.int32),
                torch.empty(n, device=dev, dtype=torch.int64) if pred_labels is not None else None)
    pt, tt = tables(int(n_pred)), tables(int(n_truth))
    _lib.check(_lib.load().r3d_scene_match_pairs(M, int(n_pred), int(n_truth), _p(pred_index), _p(truth_index),
                                                 *_match_labels_args(pred_labels, truth_labels, M), _p(pt[0]), _p(pt[1]), _p(pt[2]),
                                                 _p(tt[0]), _p(tt[1]), _p(tt[2]), _p(ws), ws.numel(), _st()))
    return pt, tt


def scene_match_best(M, pred_tables, truth_tables, n_pairs, thresholds, ws):
    """After the read of n_pairs: pred_tables, truth_tables as scene_match_pairs returned them; thresholds: 1 .. 8 floats,
    ascending -> (pair_pred, pair_truth, pair_points (n_pairs,) int32, pair_iou (n_pairs,) fp32, pred_best (P,) int32,
    truth_best (T,) int32, pair_match (n_pairs,) uint8)."""
    (_, p_points, p_classes), (_, t_points, t_classes) = pred_tables, truth_tables
    P, T, K, dev = p_points.numel(), t_points.numel(), int(n_pairs), p_points.device
    assert _seg_ws_ok(ws) and 1 <= len(thresholds) <= SCENE_MATCH_IOU and (p_classes is None) == (t_classes is None)
    pair_pred, pair_truth, pair_points = (torch.empty(K, device=dev, dtype=torch.int32) for _ in range(3))
    pair_iou = torch.empty(K, device=dev, dtype=torch.float32)
    pair_match = torch.empty(K, device=dev, dtype=torch.uint8)
    pred_best, truth_best = torch.empty(P, device=dev, dtype=torch.int32), torch.empty(T, device=dev, dtype=torch.int32)
    words = torch.empty(P + T, device=dev, dtype=torch.int64)  # the kernels' scratch
    th = (ctypes.c_float * len(thresholds))(*[float(v) for v in thresholds])  # read on the host by the entry point
    nz = lambda t: _p(t) if t.numel() else None
    _lib.check(_lib.load().r3d_scene_match_best(M, P, T, K, _p(p_points), _p(t_points), _p(p_classes), _p(t_classes), th,
                                                len(thresholds), nz(pair_pred), nz(pair_truth), nz(pair_points), nz(pair_iou),
                                                _p(pred_best), _p(truth_best), nz(pair_match), _p(words), _p(ws), ws.numel(), _st()))
    return pair_pred, pair_truth, pair_points, pair_iou, pred_best, truth_best, pair_match


# ---------------------------------------------------------------------------------------------- cutting episodes (block_pool.py)
def _episode_cut_args(points, labels, offsets, desc, classes, S, Q, N, out, mask, gt_mask, query_y, gt_query_y, slot_map):
    E, n_way = classes.shape
    B = E * (S + Q)
    for t, shape, dt in ((points, (points.shape[0], 6), torch.float32), (labels, (points.shape[0],), torch.int32),
                         (offsets, (offsets.shape[0],), torch.int64), (desc, (B, 5), torch.int32),
                         (classes, (E, n_way), torch.int32), (mask, (E * S, N), torch.int32), (gt_mask, (E * S, N), torch.int32),
                         (query_y, (E * Q, N), torch.int64), (gt_query_y, (E * Q, N), torch.int64),
                         (slot_map, (B, N), torch.int32)):
        assert tuple(t.shape) == shape and t.dtype == dt and t.is_contiguous() and t.is_cuda, (tuple(t.shape), shape, t.dtype, dt)
    assert out.dim() == 3 and out.shape[0] == B and out.shape[2] == N and out.dtype == torch.float32 and out.is_cuda
    return E, n_way, B


def _episode_cut_refused(what, rec, B, desc, rules):
    bad, last = rec[:2]
    if bad:
        raise ValueError("%s: %d of %d descriptors could not be cut (the last of them: cloud %d, %s): block outside "
                         "the pool, m_A outside 0 .. min(N, points of the class), or flags that disagree with the position%s"
                         % (what, bad, B, last - 1, desc[last - 1].tolist(), rules))


def episode_cut(points, labels, offsets, desc, classes, S, Q, N, seed, out, rgb_ch, XYZ_ch, mask, gt_mask, query_y, gt_query_y,
                slot_map):
    """r3d_episode_cut: the E (S + Q) clouds described by desc (E (S + Q), 5) int32, cut from the pool (points (T, 6) fp32,
    labels (T,) int32, offsets (n_blocks + 1,) int64) -> out (E (S + Q), C, N) fp32, read as it lies (contiguous channel-major
    or a transposed view of point-major rows), mask / gt_mask (E S, N) int32, query_y / gt_query_y (E Q, N) int64, slot_map
    (E (S + Q), N) int32.  classes (E, n_way) int32.  Reads the kernel's record afterwards and raises ValueError when a
    descriptor could not be cut; the clouds of the other descriptors are complete then, that cloud's outputs untouched."""
    E, n_way, B = _episode_cut_args(points, labels, offsets, desc, classes, S, Q, N, out, mask, gt_mask, query_y, gt_query_y,
                                    slot_map)
    rec = torch.zeros(2, device=out.device, dtype=torch.int32)
    os_ = out.stride()
    _lib.check(_lib.load().r3d_episode_cut(_p(points), _p(labels), _p(offsets), offsets.shape[0] - 1, points.shape[0], _p(desc),
                                           _p(classes), E, n_way, S, Q, N, int(seed) & 0xffffffff, out.shape[1], rgb_ch, XYZ_ch,
                                           _p(out), os_[0], os_[1], os_[2], _p(mask), _p(gt_mask),
                                           _p(query_y) if Q else None, _p(gt_query_y) if Q else None, _p(slot_map), _p(rec),
                                           _st()))
    _episode_cut_refused("episode_cut", rec.tolist(), B, desc, "")
    return out


def episode_cut_partial(points, labels, offsets, desc, classes, S, Q, N, seed, out, rgb_ch, XYZ_ch, mask, gt_mask, query_y,
                        gt_query_y, slot_map, instances, info):
    """r3d_episode_cut_partial: episode_cut with flags bit 2 (partial noise) allowed on support
    clouds with m_A == 0.  instances (T,) int32, the object id of every pool row, or None (bit 2 is refused then); info
    (E (S + Q), 8) int32 receives {K, e, f, did, o_flip, n_flip, o_drop, n_drop} per cloud, zeros for a cloud without bit 2.
    Raises ValueError as episode_cut does for a refused descriptor, and for a partial cloud whose final mask holds no point
    (that cloud is written in full)."""
    E, n_way, B = _episode_cut_args(points, labels, offsets, desc, classes, S, Q, N, out, mask, gt_mask, query_y, gt_query_y,
                                    slot_map)
    i32 = lambda t, shape: t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and tuple(t.shape) == shape
    assert (instances is None or i32(instances, (points.shape[0],))) and i32(info, (B, 8))
    rec = torch.zeros(4, device=out.device, dtype=torch.int32)
    os_ = out.stride()
    _lib.check(_lib.load().r3d_episode_cut_partial(_p(points), _p(labels), _p(offsets), offsets.shape[0] - 1, points.shape[0],
                                                   _p(desc), _p(classes), E, n_way, S, Q, N, int(seed) & 0xffffffff,
                                                   out.shape[1], rgb_ch, XYZ_ch, _p(out), os_[0], os_[1], os_[2], _p(mask),
                                                   _p(gt_mask), _p(query_y) if Q else None, _p(gt_query_y) if Q else None,
                                                   _p(slot_map), _p(rec), _p(instances), _p(info), _st()))
    rec = rec.tolist()
    _episode_cut_refused("episode_cut_partial", rec, B, desc, ", or bit 2 on a query cloud, with m_A != 0 or without "
                         "instance ids")
    if rec[2]:
        raise ValueError("episode_cut_partial: %d of %d clouds have a support mask without any point (the last of them: "
                         "cloud %d, %s)" % (rec[2], B, rec[3] - 1, desc[rec[3] - 1].tolist()))
    return out
