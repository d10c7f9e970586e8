"""tests/edge_fwd_ref.py against oracle.r3d_oracle (get_edge_feature + conv_block + max over K) in float64, and what the
cases of tests/test_gpu_edge_fwd.py promise on the reference alone: lists drawn without replacement, a near-tie share under
its cap in every case, more than 1024 units where the grid-stride walk is claimed -- no GPU."""
import numpy as np
import pytest
import torch

import edge_fwd_ref as E
from oracle import r3d_oracle as O
from r3dfsseg_amd import synthetic as S


def _folded(sd, prefix, x):
    """The operands of r3d_edgeconv_fwd for one EdgeConv layer of the state dict, folded in float64 as dgcnn.DGCNN._fold and
    the point-wise GEMM in front of the kernel do: PQ = [s1 Wa x | s1 (Wb - Wa) x + t1]."""
    def bn(p):
        s = sd[p + ".weight"] / torch.sqrt(sd[p + ".running_var"] + 1e-5)
        return s, sd[p + ".bias"] - sd[p + ".running_mean"] * s
    W1 = sd[prefix + ".layer.0.weight"].reshape(64, -1)
    Cin = W1.shape[1] // 2
    Wa, Wb = W1[:, :Cin], W1[:, Cin:]
    s1, t1 = bn(prefix + ".layer.1")
    s2, t2 = bn(prefix + ".layer.4")
    B, _, N = x.shape
    x_pm = x.permute(0, 2, 1).reshape(B * N, Cin)
    PQ = x_pm @ torch.cat((Wa, Wb - Wa), 0).t() * torch.cat((s1, s1)) + torch.cat((torch.zeros_like(t1), t1))
    return PQ, sd[prefix + ".layer.3.weight"].reshape(64, 64), s2, t2


@pytest.mark.parametrize("B,N,K,layer", [(2, 12, 4, 1), (1, 40, 20, 1), (3, 8, 32, 2), (2, 16, 8, 0)])
def test_restatement_is_the_oracle_in_float64(B, N, K, layer):
    sd = {k: v.double() for k, v in S.make_state_dict(S.make_cfg(), 123).items() if v.is_floating_point()}
    rs = np.random.RandomState(17 * N + K)
    Cin = 9 if layer == 0 else 64
    x = torch.from_numpy(rs.randn(B, Cin, N) * 0.5)
    idx = torch.from_numpy(E.lists(B, N, K, rs))
    prefix = "encoder.edge_convs.%d" % layer
    want, want_am = O.conv_block(sd, prefix, O.get_edge_feature(x, K, idx.long()), 2, 2).max(dim=-1)  # (B, 64, N)
    PQ, W2, s2, t2 = _folded(sd, prefix, x)
    out, am, v, bound = E.reference(PQ, idx, W2, s2, t2)
    want = want.permute(0, 2, 1).reshape(B * N, 64)
    np.testing.assert_allclose(out.numpy(), want.numpy(), rtol=1e-12, atol=1e-13)
    # the winners: the oracle's value at the restatement's slot is its maximum (ties through repeated neighbours aside)
    assert torch.equal(torch.gather(v, 1, am.unsqueeze(1)).squeeze(1), out)
    assert bool((bound > 0).all()) and bound.max().item() < 1e-4 * want.abs().max().item() + 1e-4
    # fp32 on the same operands: the e32 figure is an fp32-sized one
    o32 = E.reference(PQ.float(), idx, W2.float(), s2.float(), t2.float(), dtype=torch.float32)[0]
    e32 = ((o32.double() - out).abs().max() / out.abs().max()).item()
    assert 0 < e32 < 1e-5


def test_lists_are_drawn_without_replacement():
    rs = np.random.RandomState(3)
    for B, N, K in ((3, 8, 4), (3, 8, 8), (2, 132, 32), (3, 8, 20), (1, 4, 4)):
        l = E.lists(B, N, K, rs)
        assert l.shape == (B, N, K) and l.dtype == np.int32 and l.min() >= 0 and l.max() < N
        most = max(np.bincount(row, minlength=N).max() for row in l.reshape(-1, K))
        assert most == -(-K // N)


def test_cases_cover_what_the_gpu_module_promises():
    names = [c.name for c in E.CASES]
    assert len(set(names)) == len(names)
    for shape in ((3, 8), (2, 132)):
        assert {c.K for c in E.CASES if (c.B, c.N) == shape} == set(range(4, 33, 4))
    assert any((c.B, c.N, c.K) == (1, 4, 4) for c in E.CASES)
    big = [c for c in E.CASES if c.B * c.N > 4096]
    assert {c.K for c in big} == {4, 32} and all(c.B * c.N // 4 > 1024 and c.N % 4 == 0 for c in E.CASES if c in big)
    assert all(c.N % 4 == 0 and c.K % 4 == 0 and 4 <= c.K <= 32 for c in E.CASES)


@pytest.mark.parametrize("case", E.CASES, ids=[c.name.replace(" ", "-") for c in E.CASES])
def test_near_ties_are_rare_on_the_reference_alone(case):
    """At most 1 % of the (point, channel) entries of a case have a float64 gap to the best OTHER neighbour within `bound`:
    everywhere else the winners assertion of the GPU module demands the float64 arg-max (or, where a list repeats the
    winner, one of its slots).  Some s2 are negative in every case."""
    ops = E.make(case)
    assert bool((ops["s2"] < 0).any()) and bool((ops["s2"] > 0).any())
    out, am, v, bound = E.reference(**ops)
    share = E.near_tie_share(v, ops["idx"], case.N, bound)
    print("EF| %-14s near-tie share %.5f  max bound %.2e  max |out| %.2e" % (case.name, share, bound.max().item(),
                                                                             out.abs().max().item()))
    assert share <= E.NEAR_TIE_CAP, share
    assert bool(E.winners_ok(v, am, bound).all())
    low = E.lowest_slot_of_winner(v, ops["idx"], case.N)
    assert torch.equal(low, am)  # the reference's own arg-max is the lowest slot of its winner
