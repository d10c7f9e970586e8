"""Generates tests/golden/protonet_train.npz by RUNNING the reference's own ProtoNet in training mode (build container only).

    python tools/gen_golden_protonet_train.py

TEST INFRASTRUCTURE, not imported by the package.  The environment (the three absent third-party packages, Tensor.cuda on a
box without a GPU, torch 1.8's pairwise_distance) is the one oracle/gen_golden_head.py supplies -- see that file's header;
every line of `ProtoNet` that runs below is the reference's: model.train(), att_learner.dropout.p = 0 (the mask is a random
draw; the convention of the head_train fixtures), forward (models/protonet.py:245-275), loss.backward().

One noisy training episode at make_cfg(n_way=2, k_shot=2, pc_npts=512) with the weights make_state_dict(seed=123) minus proj.*,
both dist_methods.  Inputs and weights are regenerated from seeds by the tests; only reference OUTPUTS are stored:
  <method>/logits, <method>/loss, per parameter <method>/gnorm/ gpick/ gval/ (the head_train record format),
  <method>/dsfeat_s, dqfeat_s (the gradient at the two getFeatures results, rows ::8 of the point-major (B*N, C) matrix,
  columns ::4), <method>/buf/ BatchNorm running statistics after the step, and knnfix_where / knnfix_idx, the near-tie
  neighbour rows of the reference's GEMM-ordered kNN (call = 3 * getFeatures call + layer; the encoder does not depend on the
  method, so they are stored once).
Re-running reproduces the committed file bit for bit (one thread, fixed seeds).
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import gen_golden_head as G  # noqa: E402  (also puts the reference on sys.path)
from r3dfsseg_amd import synthetic as S  # noqa: E402

CFG = dict(n_way=2, k_shot=2, pc_npts=512)
EPISODE = dict(seed=21, noise_ratio=0.34, train=True)
METHODS = ("cosine", "euclidean")


def recording_knn(orig_knn, rows_out):
    """The reference's kNN (models/dgcnn.py:17-23) with the rows recorded where its neighbour SET differs from the oracle's
    channel-ascending chain, or its own margin is within rounding (the criterion of oracle/gen_golden_head.py::run_mpti)."""
    import r3d_oracle as O

    def knn(x, k):
        out = orig_knn(x, k)
        call = len(rows_out)
        own = O.knn(x.detach(), k)
        diff = (torch.sort(out, -1)[0] != torch.sort(own, -1)[0]).any(-1)
        with torch.no_grad():
            inner = -2 * torch.matmul(x.transpose(2, 1), x)
            xx = torch.sum(x ** 2, dim=1, keepdim=True)
            v = (-xx - inner - xx.transpose(2, 1)).topk(k + 1, dim=-1)[0]
        diff = (diff | ((v[..., k - 1] - v[..., k]) < 2e-5 * (1 + v[..., k].abs()))).nonzero()
        rows_out.append([(call, int(b), int(p), out[b, p].numpy().astype(np.int16)) for b, p in diff])
        return out
    return knn


def run(cfg, sd, data, dist_method, record):
    from models.protonet import ProtoNet  # the reference
    import models.dgcnn as ref_dgcnn
    model = ProtoNet(G.ref_args(cfg, dist_method=dist_method))
    model.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items() if not k.startswith("proj.")}, strict=True)
    model.train()
    model.att_learner.dropout.p = 0.0
    feats = []
    orig_get = model.getFeatures

    def get_features(x):
        out = orig_get(x)
        out.retain_grad()
        feats.append(out)
        return out

    model.getFeatures = get_features
    knn_rows = []
    orig_knn = ref_dgcnn.knn
    ref_dgcnn.knn = recording_knn(orig_knn, knn_rows)
    try:
        logits, loss = model(data[0], data[1], data[2], data[3])
        model.zero_grad()
        loss.backward()
    finally:
        ref_dgcnn.knn = orig_knn
    pre = dist_method + "/"
    record[pre + "logits"] = logits.detach().numpy()
    record[pre + "loss"] = np.float32(loss.item())
    rs = np.random.RandomState(77)
    n_params = 0
    for name, p in model.named_parameters():
        g = p.grad
        if g is None:
            continue
        n_params += 1
        flat = g.detach().reshape(-1).double()
        record[pre + "gnorm/" + name] = np.float64(flat.norm().item())
        pick = rs.randint(0, flat.numel(), min(256, flat.numel()))
        record[pre + "gpick/" + name] = pick.astype(np.int64)
        record[pre + "gval/" + name] = g.detach().reshape(-1)[pick].numpy()
    for name, b in model.named_buffers():
        if name.endswith("running_mean") or name.endswith("running_var"):
            record[pre + "buf/" + name] = b.detach().numpy().copy()
    assert len(feats) == 2
    for key, f in zip(("dsfeat_s", "dqfeat_s"), feats):  # (B, C, N) -> point-major rows
        gpm = f.grad.detach().permute(0, 2, 1).reshape(-1, f.shape[1])
        record[pre + key] = gpm[::8, ::4].numpy().copy()
    flat = [r for rows in knn_rows for r in rows]
    where = np.array([[c, b, p] for c, b, p, _ in flat], np.int32).reshape(-1, 3)
    idx = np.array([i for _, _, _, i in flat], np.int16).reshape(-1, cfg["dgcnn_k"])
    return where, idx, n_params, sum(1 for _ in model.parameters())


def main():
    torch.manual_seed(0)
    torch.set_num_threads(1)
    G.install_environment()
    cfg = S.make_cfg(**CFG)
    sd = S.make_state_dict(cfg, seed=123)
    data = G.to_torch(S.make_episode(cfg, **EPISODE)[0])
    rec = {}
    fixes = []
    for dm in METHODS:
        where, idx, n_grad, n_all = run(cfg, sd, data, dm, rec)
        fixes.append((where, idx))
        print("protonet_train %s: loss %.6f, %d of %d parameters with a gradient, %d near-tie kNN rows"
              % (dm, rec[dm + "/loss"], n_grad, n_all, len(where)))
    assert all(np.array_equal(fixes[0][0], f[0]) and np.array_equal(fixes[0][1], f[1]) for f in fixes)
    rec["knnfix_where"], rec["knnfix_idx"] = fixes[0]
    out = os.path.join(G.OUT, "protonet_train.npz")
    np.savez_compressed(out, **rec)
    print(out, os.path.getsize(out))


if __name__ == "__main__":
    main()
