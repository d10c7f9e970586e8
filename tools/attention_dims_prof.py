"""Attention forward / backward at head widths 32, 64, 96, 128 on workload S's shape (one episode of 2-way 5-shot at 2048
points: 11 clouds), in both matrix arithmetics, for a kernel trace:

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/attention_dims_prof.py

Each (width, arithmetic) runs REPS forward + backward calls after one warm-up; the trace's per-kernel statistics then give
the per-call time (kernel names carry the width: r3d_attention_*_kernel<D, ...>).  Also prints HIP-event times per call
and the algorithmic TFLOP/s (forward 4 B N^2 D, backward 10 B N^2 D: S K^T, P V and dP V^T, dS K, dS^T Q over the same
N x N products; dropout p = 0.1 as in training)."""
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from r3dfsseg_amd import _lib  # noqa: E402
from r3dfsseg_amd.ops import _p, _st  # noqa: E402

B, N, REPS, P_DROP = 11, 2048, 20, 0.1


def main():
    lib = _lib.load()
    before = lib.r3d_get_matrix_arith()
    res = []
    for mode, arith in ((1, "bf16x3"), (0, "fp32")):
        _lib.check(lib.r3d_set_matrix_arith(mode))
        for D in (32, 64, 96, 128):
            g = torch.Generator(device="cuda").manual_seed(D)
            qkv = torch.randn(B * N, 3 * D, device="cuda", generator=g)
            qkv[:, :D] *= D ** -0.5
            dO = torch.randn(B * N, D, device="cuda", generator=g)
            out = torch.empty(B * N, D, device="cuda")
            lse = torch.empty(B * N, device="cuda")
            dqkv = torch.empty(B * N, 3 * D, device="cuda")
            ws = torch.empty(lib.r3d_attention_ws_words_ep_d(B, N, 0, D), device="cuda")

            def fwd():
                _lib.check(lib.r3d_attention_fwd_train_ep_d(_p(qkv), 3 * D, B, N, _p(out), D, _p(lse), P_DROP,
                                                            ctypes.c_uint(1), None, 0, D, _p(ws), _st()))

            def bwd():
                _lib.check(lib.r3d_attention_bwd_ep_d(_p(qkv), 3 * D, B, N, _p(out), D, _p(dO), D, _p(lse), P_DROP,
                                                      ctypes.c_uint(1), None, 0, D, 1.0, _p(dqkv), 3 * D, _p(ws), 1, _st()))
            fwd(); bwd()
            torch.cuda.synchronize()
            t = {}
            for name, fn in (("fwd", fwd), ("bwd", bwd)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(REPS):
                    fwd() if name == "bwd" else None  # the backward reuses the forward's packed operands, as in training
                    fn()
                e1.record()
                torch.cuda.synchronize()
                t[name] = e0.elapsed_time(e1) / REPS
            t["bwd"] -= t["fwd"]  # the loop above ran a forward before every backward
            flops = {"fwd": 4.0 * B * N * N * D, "bwd": 10.0 * B * N * N * D}
            r = dict(arith=arith, D=D, fwd_ms=round(t["fwd"], 4), bwd_ms=round(t["bwd"], 4),
                     fwd_tflops=round(flops["fwd"] / t["fwd"] * 1e-9, 2), bwd_tflops=round(flops["bwd"] / t["bwd"] * 1e-9, 2))
            print(json.dumps(r), flush=True)
            res.append(r)
    _lib.check(lib.r3d_set_matrix_arith(before))
    return res


if __name__ == "__main__":
    main()
