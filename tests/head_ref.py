"""Float64 references of the transductive head's training path (torch on the CPU, autograd), for
tests/test_gpu_head_backward.py; tests/test_head_ref_host.py holds them to the fp32 oracle without a GPU.

Every function takes a ``dtype``: float64 is the reference, float32 is the same dense formula in the kernels' precision
(the ``e32`` the GPU tests print beside each measured error).  INDEX decisions (neighbour lists, FPS seeds, nearest-seed
assignments) are never taken here: they come from the caller or from the oracle on the fp32 features, where they are
held bit-exact against the device elsewhere (tests/test_gpu_head.py)."""
import numpy as np
import torch

from oracle import r3d_oracle as O

EPS = float(np.finfo(float).eps)


# ------------------------------------------------------------------------------------------------------------------
# 1. affinity + label propagation (models/mpti.py:717-776), dense
# ------------------------------------------------------------------------------------------------------------------
def lp_from_nodes(xl, nbr, Y, sigma, alpha=0.99):
    """The formulas themselves, in the precision of the node matrix xl (n, D), which may carry an autograd graph of its
    own (prototype means): nbr (n, k + 1) int64 neighbour lists (column 0 dropped, whatever it holds), Y (n, C) ->
    (S (n, n), Z (n, C))."""
    dtype = xl.dtype
    Y = Y.to(dtype)
    n, d = xl.shape
    I = nbr[:, 1:]
    k = I.shape[1]
    knn_feat = xl[I.reshape(-1)].view(n, k, d)
    dist = torch.norm(xl[:, None, :] - knn_feat + 1e-6, 2, 2)  # torch-1.8 pairwise_distance: the eps inside the norm
    w = torch.exp(-0.5 * (dist / sigma) ** 2)
    A = torch.zeros(n, n, dtype=dtype).scatter(1, I, w)
    A = A + A.t()
    A = A * (1 - torch.eye(n, dtype=dtype))
    dinv = torch.sqrt(1.0 / (A.sum(1) + EPS))
    S = dinv[:, None] * A * dinv[None, :]
    Z = torch.linalg.inv(torch.eye(n, dtype=dtype) - alpha * S + EPS) @ Y
    return S, Z


def lp_dense(x, nbr, Y, sigma, alpha=0.99, dtype=torch.float64):
    """x (n, D) fp32 cast up -> (S, Z, xl): xl is the leaf the graph hangs on, xl.grad = dx after a backward() through Z."""
    xl = x.detach().to(dtype).requires_grad_()
    S, Z = lp_from_nodes(xl, nbr, Y, sigma, alpha)
    return S, Z, xl


def lp_dense_grad(x, nbr, Y, G, sigma, alpha=0.99, dtype=torch.float64):
    """-> (S, Z, lam, dx) all detached: lam = inv(I - alpha S) G, dx = d<Z, G> / dx."""
    S, Z, xl = lp_dense(x, nbr, Y, sigma, alpha, dtype)
    G = G.to(dtype)
    (Z * G).sum().backward()
    S = S.detach()
    lam = torch.linalg.inv(torch.eye(S.shape[0], dtype=dtype) - alpha * S + EPS) @ G  # (the matrix is symmetric)
    return S, Z.detach(), lam, xl.grad


# ------------------------------------------------------------------------------------------------------------------
# 2. gradient of the mean cross entropy over the query rows (models/mpti.py:778-781)
# ------------------------------------------------------------------------------------------------------------------
def ce_grad64(Z, n_proto, labels, n_classes, gscale, dtype=torch.float64):
    """Z (rows, C >= n_classes), labels (n_qpts,) int64 -> G (rows, C): gscale / n_qpts * (softmax - one-hot) over the
    first n_classes columns of rows [n_proto, n_proto + n_qpts), zero everywhere else."""
    labels = labels.reshape(-1)
    n_q = labels.numel()
    G = torch.zeros(Z.shape, dtype=dtype)
    z = Z[n_proto:n_proto + n_q, :n_classes].to(dtype)
    p = torch.softmax(z, 1)
    p[torch.arange(n_q), labels] -= 1.0
    G[n_proto:n_proto + n_q, :n_classes] = p * (float(gscale) / n_q)
    return G


# ------------------------------------------------------------------------------------------------------------------
# 3. prototypes = cluster means (models/mpti.py:597-715)
# ------------------------------------------------------------------------------------------------------------------
def cluster_means(feat32, feat, k):
    """Means of the clusters O.get_multiple_prototypes finds on feat32 (fp32: the index decisions), computed on `feat`
    (the same rows in the reference's precision, with autograd) -> (means (m, D), counts (m,) int64)."""
    _, asg, m, _ = O.get_multiple_prototypes(feat32, k)
    counts = torch.bincount(asg, minlength=m)
    sums = torch.zeros(m, feat.shape[1], dtype=feat.dtype).index_add(0, asg, feat)
    return sums / counts.to(feat.dtype)[:, None], counts


def segments(support_y):
    """support_y (n_way, k_shot, N) -> per segment (background, way 0, ...) the support rows it lists, ascending."""
    n_way, k_shot, N = support_y.shape
    segs = [torch.nonzero(support_y.reshape(-1) == 0).squeeze(1)]
    for w in range(n_way):
        segs.append(torch.nonzero(support_y[w].reshape(-1) == 1).squeeze(1) + w * k_shot * N)
    return segs


def proto_nodes(sfeat, qfeat, support_y, k_sub, dtype=torch.float64):
    """sfeat (S N, D), qfeat (Q, D) fp32, support_y (n_way, k_shot, N) -> (nodes (n_proto + Q, D), counts (n_proto,),
    seg_m [per segment], sl, ql): background prototypes, then every way's, then the query rows; sl / ql are the leaves."""
    sl = sfeat.detach().to(dtype).requires_grad_()
    ql = qfeat.detach().to(dtype).requires_grad_()
    rows, counts, seg_m = [], [], []
    for ids in segments(support_y):
        assert len(ids) > 0, "the reference cannot run an empty segment"
        p, c = cluster_means(sfeat[ids], sl[ids], k_sub)
        rows.append(p); counts.append(c); seg_m.append(p.shape[0])
    return torch.cat(rows + [ql], 0), torch.cat(counts), seg_m, sl, ql


# ------------------------------------------------------------------------------------------------------------------
# 4. per-way supervised contrastive loss (models/mpti.py:226-313; O.per_way_contrast_loss restated)
# ------------------------------------------------------------------------------------------------------------------
def supcon64(W, b, sfeat, support_y, support_flag, fps_k=4, temp=0.1, dtype=torch.float64):
    """sfeat (S N, D) fp32, support_y (n_way, k_shot, N), support_flag (n_way, k_shot), W (P, D), b (P,) ->
    (loss, sl, Wl, bl): the leaves carry dfeat, dW, db after loss.backward()."""
    n_way, k_shot, N = support_y.shape
    sl = sfeat.detach().to(dtype).requires_grad_()
    Wl, bl = W.detach().to(dtype).requires_grad_(), b.detach().to(dtype).requires_grad_()
    clean = bool(support_flag[0, 0] * k_shot == support_flag[0].sum())
    total = []
    for way in range(n_way):
        feats, labels = [], []

        def add(w, k, label):
            ids = torch.nonzero(support_y[w, k] == 1).squeeze(1) + (w * k_shot + k) * N
            p, _ = cluster_means(sfeat[ids], sl[ids], fps_k)
            feats.append(torch.nn.functional.normalize(p @ Wl.t() + bl, p=2, dim=1))
            labels.append(torch.full((p.shape[0],), float(label), dtype=dtype))

        for k in range(k_shot):
            add(way, k, float(support_flag[way, k]))
        if clean:
            other = way + 1 if way < n_way - 1 else 0
            for k in range(2):
                add(other, k, -1.0)
        f, lab = torch.cat(feats, 0), torch.cat(labels, 0)
        lm = 1.0 - torch.eye(lab.shape[0], dtype=dtype)
        gt = torch.eq(lab[:, None], lab[None, :]).to(dtype) * lm
        logits = (f @ f.t()) / temp
        log_prob = logits - torch.log((torch.exp(logits) * lm).sum(1, keepdim=True))
        total.append((-(gt * log_prob).sum(1) / gt.sum(1)).mean())
    return sum(total) / len(total), sl, Wl, bl


# ------------------------------------------------------------------------------------------------------------------
# shared by the GPU tests
# ------------------------------------------------------------------------------------------------------------------
def graph_nodes(n_proto, n_q_pts, D, seed, scale=0.06):
    """Three gaussian clusters (tests/test_gpu_head.py::_graph_nodes at any width) plus a HUB (row 5 = the mean of all
    rows: everybody's neighbour, its symmetric row far longer than k + 1) and DUPLICATES (query row n_proto + 7 = prototype
    row 3; query row n_proto + 8 = row n_proto + 9: the second pair puts a row's own index at column 1 of its list).
    -> (x (n, D) fp32, lab (n,) int64 in [0, 3))."""
    rs = np.random.RandomState(seed)
    centers = rs.randn(3, D).astype(np.float32) * scale * 2
    lab = rs.randint(0, 3, n_proto + n_q_pts)
    x = centers[lab] + rs.randn(n_proto + n_q_pts, D).astype(np.float32) * scale
    x[5] = x.mean(0)
    x[n_proto + 7] = x[3]
    x[n_proto + 8] = x[n_proto + 9]
    return torch.from_numpy(x), torch.from_numpy(lab.astype(np.int64))


def rel(got, want):
    """max |got - want| / max |want| (want: the float64 reference)."""
    return (got.double() - want.double()).abs().max().item() / max(1e-300, want.double().abs().max().item())


def block_errors(got, want, n_proto):
    """{block name: error relative to THAT block's largest reference entry}: prototype rows and query rows apart, channel
    blocks [0,64), [64,128), [128,192), [192,256) apart, so that no block hides behind a larger one."""
    out = {}
    for rname, r0, r1 in (("proto", 0, n_proto), ("query", n_proto, want.shape[0])):
        for c0 in range(0, want.shape[1], 64):
            c1 = min(c0 + 64, want.shape[1])
            out["%s[%d:%d)" % (rname, c0, c1)] = rel(got[r0:r1, c0:c1], want[r0:r1, c0:c1])
    return out
