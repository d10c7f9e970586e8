"""tests/edge_ref.py against torch autograd in float64 on the reference's own formulation of an EdgeConv layer in
training mode (models/dgcnn.py:26-61: cat(neighbour - centre, centre) through conv1, nn.BatchNorm2d in train mode applied
to every segment separately, LeakyReLU 0.2, conv2, BatchNorm, LeakyReLU, max over K), and the exclusion shares of the GPU
cases (tests/edge_cases.py) on the reference alone.  No GPU."""
import numpy as np
import pytest
import torch

import edge_cases as EC
import edge_ref as R

BAR = 1e-10


@pytest.mark.parametrize("K", [4, 20])
@pytest.mark.parametrize("lay", [(1, 1, 0, 8), (2, 3, 1, 36), (2, 1, 3, 40)])
def test_edge_ref_equals_autograd_on_the_reference_formulation(lay, K):
    C = 5
    c = EC.layer_inputs(lay, K, C, seed=31 * lay[3] + K)
    seg = c["seg"]
    B, N = seg.B, seg.N
    got = EC.layer_ref(c)
    x = c["x"].double().requires_grad_()
    W1, W2 = c["W1"].double().requires_grad_(), c["W2"].double().requires_grad_()
    bn1, bn2 = torch.nn.BatchNorm2d(64, eps=EC.EPS).double().train(), torch.nn.BatchNorm2d(64, eps=EC.EPS).double().train()
    with torch.no_grad():
        bn1.weight.copy_(c["g1"]), bn1.bias.copy_(c["b1"]), bn2.weight.copy_(c["g2"]), bn2.bias.copy_(c["b2"])
    xb = x.view(B, N, C)
    nb = torch.stack([xb[b][c["idx"][b].long()] for b in range(B)])      # (B, N, K, C)
    ctr = xb[:, :, None, :].expand(B, N, K, C)
    e1 = (torch.cat((nb - ctr, ctr), -1) @ W1.t()).permute(0, 3, 1, 2)   # (B, 64, N, K)
    lre = torch.nn.functional.leaky_relu
    outs = []
    for r0, r1 in R.seg_slices(seg):                                     # every segment its own BatchNorm batch
        s = slice(r0 // N, r1 // N)
        h1 = lre(bn1(e1[s]), 0.2)
        z2 = torch.einsum("bcnk,dc->bdnk", h1, W2)
        outs.append(lre(bn2(z2), 0.2).max(3).values.permute(0, 2, 1).reshape(-1, 64))
    out = torch.cat(outs)
    (out * c["dout"].double()).sum().backward()
    want = dict(out=out.detach(), dW1=W1.grad, dW2=W2.grad, dg1=bn1.weight.grad, db1=bn1.bias.grad, dg2=bn2.weight.grad,
                db2=bn2.bias.grad, dx=x.grad)
    for k, w in want.items():
        assert R.rel(got[k], w) <= BAR, (k, R.rel(got[k], w))


def test_fp32_restatement_follows_the_partition_and_stays_close():
    """The fp32 dtype of every function: the sums in the kernels' partition equal a plain loop over chunk, wave and
    point written here, and every result stays within fp32 distance of float64."""
    c = EC.case((2, 3, 1, 36), 20, "perm")
    seg, K = c["seg"], c["K"]
    e1 = R.gather_e1(c["PQ"], c["idx"], seg, torch.float32).numpy()
    got = R.edge_sums_f32(e1, seg, "waves").numpy()
    want = np.zeros((seg.n_seg, 64))
    cs = R.cloud_segments(seg)
    for b in range(seg.B):
        for p0 in range(0, seg.N, 32):
            waves = []
            for w in range(4):
                a = np.zeros(64, np.float32)
                for p in range(p0 + w, min(p0 + 32, seg.N), 4):
                    for t in range(K):
                        a = a + e1[b, p, t]
                waves.append(a)
            want[int(cs[b])] += (((waves[0] + waves[1]) + waves[2]) + waves[3]).astype(np.float64)
    assert np.array_equal(got, want.astype(np.float32))
    s32, s64 = R.stats1(c["PQ"], c["idx"], seg, torch.float32), c["st"]
    assert float(((s32["sums"].double() - s64["sums"]).abs() / s64["terms"]).max()) < 1e-6
    f32 = R.fwd(c["PQ"], c["idx"], c["bn1"], c["W2"], seg, bn2=c["bn2"], dtype=torch.float32, keep_edges=False)
    assert float(((f32["sums2"].double() - c["fw"]["sums2"]).abs() / c["fw"]["terms2"]).max()) < 1e-6
    assert R.rel(f32["out"], c["sel"]["out"]) < 1e-5
    b64, b32 = EC.backward(c), EC.backward(c, torch.float32)
    for k in ("dW2", "bn1_sums", "dP", "dQ"):
        assert float(((b32[k].double() - b64[k]).abs() / b64[k + "_mag"].clamp_min(1e-300)).max()) < 1e-5, k


def test_ties_take_the_lowest_edge_position_and_lists_are_what_they_claim():
    c = EC.case((2, 1, 3, 40), 12, "repeats")
    idx, fw = c["idx"].long(), c["fw"]
    B, N, K = idx.shape
    assert all(int((idx[b, i] == j).sum()) == 2 for b in range(B) for i in range(0, N, 7) for j in idx[b, i].tolist())
    am = fw["argmax"].view(B, N, 64)
    win_j = torch.gather(idx[:, :, :, None].expand(B, N, K, 64), 2, am[:, :, None, :])[:, :, 0]
    first = (idx[:, :, :, None] == win_j[:, :, None, :]).to(torch.uint8).cumsum(2).eq(1).to(torch.uint8).argmax(2)
    assert torch.equal(first, am) and int((am >= K // 2).sum()) < am.numel()  # the winner is the FIRST of its two edges
    h = EC.case((2, 1, 3, 40), 20, "hubs")["idx"]
    assert (h[:, :, 0] == 0).all() and (h[:, :, 1] == 39).all()
    assert R.n_chunks(EC.case(*EC.SMALL[0])["seg"]) == 1


@pytest.mark.parametrize("cs", EC.CASES, ids=[EC.case_id(c) for c in EC.CASES])
def test_exclusion_shares_of_the_gpu_cases_stay_below_their_caps(cs):
    """What tests/test_gpu_edge_train.py leaves out, measured on the float64 reference for the seeds it uses: pairs whose
    best two z2 are closer than 64 ULP (cap 0.5 %), dQ / dP elements with an edge within 1e-5 of LeakyReLU-1's kink and
    winners within 1e-5 of LeakyReLU-2's (cap 1 % each).  The chunk counts are the ones the layouts were chosen for."""
    c = EC.case(*cs)
    sh = c["shares"]
    print("EC| %-26s shares gap %.2e  u2 %.2e  dQ %.2e  dP %.2e" % (EC.case_id(cs), sh["gap"], sh["u2"], sh["dQ"], sh["dP"]))
    assert sh["gap"] <= EC.CAP_GAP and max(sh["u2"], sh["dQ"], sh["dP"]) <= EC.CAP_KINK, sh
    assert R.n_chunks(c["seg"]) == EC.CHUNKS[cs[0]]
    assert (c["dout"] != 0).float().mean() >= 1 - EC.CAP_KINK
