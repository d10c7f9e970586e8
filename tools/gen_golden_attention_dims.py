"""Generates tests/golden/attention_d{32,96,128}.npz by IMPORTING the reference's SelfAttention (build container only).

    python tools/gen_golden_attention_dims.py /path/to/reference

models/attention.py::SelfAttention(256, D) in eval mode (dropout off) on a (2, 256, 200) input (200 points: not a
multiple of the kernels' 128-row tile, and small files), for the head widths the
attention kernels add beside 64 (the reference's --output_dim).  Each file stores the input x, the three map weights
(D, 256, 1) and the reference output y (2, D, 200); tests/test_gpu_output_dim.py reads nothing else.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
WIDTHS = (32, 96, 128)


def main(ref_root):
    sys.path.insert(0, ref_root)
    from models.attention import SelfAttention  # noqa: E402  (reference)
    torch.set_num_threads(1)
    for D in WIDTHS:
        rs = np.random.RandomState(7000 + D)
        x = (rs.randn(2, 256, 200) * 0.5).astype(np.float32)
        # the scale of synthetic.make_state_dict (gain 4 on q / k): attention weights far from uniform
        w = {m: (rs.randn(D, 256, 1) * (4.0 if m != "v" else 2.0) / np.sqrt(256)).astype(np.float32) for m in "qkv"}
        att = SelfAttention(256, D)
        att.load_state_dict({"%s_map.weight" % m: torch.from_numpy(w[m]) for m in "qkv"})
        att.eval()
        with torch.no_grad():
            y = att(torch.from_numpy(x)).numpy()
        path = os.path.join(OUT, "attention_d%d.npz" % D)
        np.savez_compressed(path, x=x, wq=w["q"], wk=w["k"], wv=w["v"], y=y)
        print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("R3D_REFERENCE", "../reference"))
