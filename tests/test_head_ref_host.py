"""The float64 references of tests/head_ref.py against the fp32 oracle (oracle/r3d_oracle.py) and torch autograd through it,
on the CPU: each on two small inputs, values and gradients to 1e-4 of the largest entry (fp32 against float64 on such
inputs: 1e-6 ... 1e-5).  What the GPU tests of the head backward compare with is thereby the reference's own formula."""
import numpy as np
import pytest
import torch

import head_ref as R
from oracle import r3d_oracle as O

BAR = 1e-4


def _close(got, want, what):
    e = R.rel(got.detach(), want.detach())
    assert e <= BAR, (what, e)


@pytest.mark.parametrize("n_proto,n_q,D,k,sigma,seed", [(20, 100, 32, 8, 1.0, 1), (12, 60, 20, 30, 0.5, 2)])
def test_lp_dense_is_the_oracles_affinity_and_label_propagation(n_proto, n_q, D, k, sigma, seed):
    x, lab = R.graph_nodes(n_proto, n_q, D, seed)
    n = n_proto + n_q
    Y = torch.zeros(n, 3)
    Y[torch.arange(n_proto), lab[:n_proto]] = 1
    G = torch.randn(n, 3, generator=torch.Generator().manual_seed(seed))
    nbr = O.knn_l2(x, k + 1)
    assert (nbr[n_proto + 9, :2] == torch.tensor([n_proto + 8, n_proto + 9])).all()  # own index at column 1: a self-edge
    xo = x.clone().requires_grad_()
    A = O.affinity(xo, k, sigma, nbr_override=nbr)
    Zo = O.label_propagate(A, Y)
    (Zo * G).sum().backward()
    S, Z, lam, dx = R.lp_dense_grad(x, nbr, Y, G, sigma)
    assert (torch.diagonal(S) == 0).all() and torch.equal(S != 0, A.detach() != 0)
    dinv = torch.sqrt(1.0 / (A.detach().sum(1) + R.EPS))
    _close(dinv[:, None] * A.detach() * dinv[None, :], S, "S")
    _close(Zo, Z, "Z")
    _close(O.label_propagate(A.detach(), G), lam, "lam")
    _close(xo.grad, dx, "dx")
    # the same function in fp32 (what the GPU tests report as e32) is the same formula
    S32, Z32, lam32, dx32 = R.lp_dense_grad(x, nbr, Y, G, sigma, dtype=torch.float32)
    assert Z32.dtype == torch.float32 and dx32.dtype == torch.float32
    _close(Z32, Z, "Z32"); _close(dx32, dx, "dx32"); _close(lam32, lam, "lam32")


@pytest.mark.parametrize("rows,n_proto,n_q,n_classes,seed", [(40, 7, 30, 3, 1), (64, 11, 50, 8, 2)])
def test_ce_grad64_is_autograd_of_the_mean_cross_entropy(rows, n_proto, n_q, n_classes, seed):
    g = torch.Generator().manual_seed(seed)
    Z = (torch.randn(rows, 8, generator=g) * 3).requires_grad_()
    labels = torch.randint(0, n_classes, (n_q,), generator=g)
    loss = torch.nn.functional.cross_entropy(Z[n_proto:n_proto + n_q, :n_classes], labels)
    (0.37 * loss).backward()
    G = R.ce_grad64(Z.detach(), n_proto, labels, n_classes, 0.37)
    _close(Z.grad, G, "G")
    assert (G[:n_proto] == 0).all() and (G[n_proto + n_q:] == 0).all() and (G[:, n_classes:] == 0).all()


def _masks(n_way, k_shot, N, fg_counts, seed):
    """support_y (n_way, k_shot, N) with fg_counts[w][k] foreground points in shot (w, k), at random positions."""
    rs = np.random.RandomState(seed)
    y = torch.zeros(n_way, k_shot, N, dtype=torch.int64)
    for w in range(n_way):
        for k in range(k_shot):
            y[w, k, torch.from_numpy(rs.permutation(N)[:fg_counts[w][k]])] = 1
    return y


@pytest.mark.parametrize("n_way,k_shot,N,D,k_sub,fg,seed", [(2, 2, 48, 16, 10, ((3, 7), (5, 6)), 1),
                                                            (3, 1, 64, 24, 6, ((2,), (6,), (30,)), 2)])
def test_proto_nodes_are_the_oracles_prototypes(n_way, k_shot, N, D, k_sub, fg, seed):
    """Segments with n < k, n == k, n == k + 1 and n > k; values and the gradient of sum(nodes * R)."""
    g = torch.Generator().manual_seed(seed)
    y = _masks(n_way, k_shot, N, fg, seed)
    sfeat = torch.randn(n_way * k_shot * N, D, generator=g) * 0.1
    qfeat = torch.randn(N, D, generator=g) * 0.1
    so = sfeat.clone().requires_grad_()
    sf4 = so.view(n_way, k_shot, N, D).transpose(2, 3)
    fg_p, _, _, fg_m = O.get_foreground_prototypes(sf4, y, k_sub, n_way + 1)
    bg_p, _, _, bg_m = O.get_background_prototypes(sf4, torch.logical_not(y), k_sub, n_way + 1)
    want = torch.cat((bg_p, fg_p), 0)
    nodes, counts, seg_m, sl, ql = R.proto_nodes(sfeat, qfeat, y, k_sub)
    assert seg_m == [bg_m] + list(fg_m) and counts.sum().item() == n_way * k_shot * N
    n_proto = want.shape[0]
    _close(want, nodes[:n_proto], "prototypes")
    assert torch.equal(nodes[n_proto:].detach(), qfeat.double())
    Rm = torch.randn(nodes.shape, generator=g)
    (want * Rm[:n_proto]).sum().backward()
    (nodes * Rm.double()).sum().backward()
    _close(so.grad, sl.grad, "dsfeat")
    assert torch.equal(ql.grad, Rm[n_proto:].double())


@pytest.mark.parametrize("n_way,k_shot,D,flags,fg,seed", [
    (2, 2, 16, ((1, 1), (1, 1)), ((1, 4), (5, 30)), 1),                 # clean: two negative shots of the next way
    (3, 3, 24, ((1, 0, 1), (0, 0, 1), (1, 1, 0)), ((4, 5, 9), (1, 30, 5), (2, 1, 6)), 2)])  # noisy: every label twice per way
def test_supcon64_is_the_oracles_contrast_loss(n_way, k_shot, D, flags, fg, seed):
    N, P = 48, 12
    g = torch.Generator().manual_seed(seed)
    y = _masks(n_way, k_shot, N, fg, seed)
    flag = torch.tensor(flags)
    sfeat = torch.randn(n_way * k_shot * N, D, generator=g) * 0.1
    W, b = torch.randn(P, D, generator=g) * 0.3, torch.randn(P, generator=g) * 0.1
    so = sfeat.clone().requires_grad_()
    sd = {"proj.weight": W.clone().requires_grad_(), "proj.bias": b.clone().requires_grad_()}
    want = O.per_way_contrast_loss(sd, so.view(n_way, k_shot, N, D).transpose(2, 3), y, flag, 4, 0.1)
    want.backward()
    loss, sl, Wl, bl = R.supcon64(W, b, sfeat, y, flag)
    loss.backward()
    assert torch.isfinite(loss) and abs(loss.item() - want.item()) <= BAR * abs(loss.item())
    _close(so.grad, sl.grad, "dfeat")
    _close(sd["proj.weight"].grad, Wl.grad, "dW")
    _close(sd["proj.bias"].grad, bl.grad, "db")
    assert (sl.grad.view(n_way, k_shot, N, D)[y == 0] == 0).all()  # background rows carry no gradient
