"""tests/attn_ref.py, the float64 reference of the attention training kernels, held without a GPU: to torch autograd, to the
oracle and the reference's golden vectors, its keep mask to a scalar loop of the hash; and the preconditions of the
dropout-edge cases of tests/test_gpu_attention_kernels.py, whose seeds were searched on the host and are proven here."""
import os

import numpy as np
import pytest
import torch

import attn_ref as R
from golden_inputs import golden_inputs
from oracle import r3d_oracle as O
from r3dfsseg_amd import synthetic as S

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _inputs(B, N, D, seed):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B * N, 3 * D, generator=g)
    qkv[:, :D] *= 0.5 * (64.0 / D) ** 0.5
    return qkv, torch.randn(B * N, D, generator=g)


@pytest.mark.parametrize("D", [32, 64, 96, 128])
@pytest.mark.parametrize("p_drop", [0.0, 0.1])
def test_attention_against_autograd(D, p_drop):
    """Every returned quantity against float64 autograd through softmax(q k^T) * keep / (1 - p) @ v, at 1e-12."""
    B, N, q_scale = 2, 37, 0.37
    qkv, dO = _inputs(B, N, D, 5 + D)
    keep = R.keep_mask(B, N, 77, p_drop) if p_drop > 0 else None
    out, lse, rowdot, dqkv = R.attention(qkv, B, N, D, dO, keep, p_drop, q_scale)
    x = qkv.double().requires_grad_()
    q, k, v = (x[:, D * i:D * (i + 1)].view(B, N, D) for i in range(3))
    s = q @ k.transpose(1, 2)
    attn = torch.softmax(s, -1)
    if keep is not None:
        attn = attn * keep.double() / (1.0 - float(np.float32(p_drop)))
    y = (attn @ v).reshape(B * N, D)
    (y * dO.double()).sum().backward()
    want_d = x.grad.clone()
    want_d[:, :D] *= q_scale
    assert R.rel(out, y) <= 1e-12
    assert (lse - torch.logsumexp(s.detach(), -1).reshape(-1)).abs().max().item() <= 1e-12
    assert R.rel(rowdot, (y.detach() * dO.double()).sum(-1)) <= 1e-12
    for i in range(3):
        assert R.rel(dqkv[:, D * i:D * (i + 1)], want_d[:, D * i:D * (i + 1)]) <= 1e-12, "qkv"[i]
    # the fp32 column is the same formula: close to float64, and fp32
    o32 = R.attention(qkv, B, N, D, dO, keep, p_drop, q_scale, dtype=torch.float32)
    assert all(t.dtype == torch.float32 for t in o32)
    assert R.rel(o32[0], out) < 1e-5 and R.rel(o32[3], dqkv) < 1e-5


def _golden_case(name):
    """-> (x (B, 256, N), state dict of the three maps, golden y (B, D, N))."""
    if name == "attention":
        z = np.load(os.path.join(G, "attention.npz"))
        sd = S.make_state_dict(S.make_cfg(), seed=123)
        return golden_inputs()["x256"], sd, z["y"]
    z = np.load(os.path.join(G, name + ".npz"))
    sd = {"att_learner.%s_map.weight" % m: torch.from_numpy(z["w" + m]) for m in "qkv"}
    return torch.from_numpy(z["x"]), sd, z["y"]


@pytest.mark.parametrize("name", ["attention", "attention_d32", "attention_d96", "attention_d128"])
def test_attention_against_the_golden_vectors(name):
    """q | k | v of the reference's maps (q scaled by 1 / sqrt(D) as the GEMM epilogue does) through attn_ref.attention.
    The golden vectors are fp32 results of the reference, so the chain has two links: oracle.self_attention in fp32 and
    attn_ref in fp32 both meet them at the bar of tests/test_oracle_golden.py (atol 1e-6, rtol 1e-5), and attn_ref in
    float64 equals the oracle in float64 at 1e-12."""
    x, sd, gold = _golden_case(name)
    B, _, N = x.shape
    D = gold.shape[1]

    def through_ref(dtype):
        maps = [torch.nn.functional.conv1d(x.to(dtype), sd["att_learner.%s_map.weight" % m].to(dtype)) for m in "qkv"]
        maps[0] = maps[0] / D ** 0.5
        qkv = torch.cat([m.transpose(1, 2).reshape(B * N, D) for m in maps], 1)  # (B N, 3 D) point-major
        out = R.attention(qkv, B, N, D, torch.zeros(B * N, D), dtype=dtype)[0]
        return out.view(B, N, D).transpose(1, 2)

    y32 = O.self_attention(sd, x)
    np.testing.assert_allclose(y32.numpy(), gold, atol=1e-6, rtol=1e-5)
    np.testing.assert_allclose(through_ref(torch.float32).numpy(), gold, atol=1e-6, rtol=1e-5)
    sd64 = {k: v.double() for k, v in sd.items() if k.startswith("att_learner.")}
    y64 = O.self_attention(sd64, x.double())
    assert R.rel(through_ref(torch.float64), y64) <= 1e-12


def _hash_scalar(seed, row, key):
    """attn_keep's hash of one pair, one Python integer at a time."""
    m = 0xFFFFFFFF
    x = ((row * 0x9E3779B1) & m) ^ ((key * 0x85EBCA77) & m) ^ (seed & m)
    x ^= x >> 16
    x = (x * 0x7FEB352D) & m
    x ^= x >> 15
    x = (x * 0x846CA68B) & m
    x ^= x >> 16
    return x


@pytest.mark.parametrize("seed,seed_dev,group", [(4321, 0, 0), (0xFFFFFFFF, 3, 2), (0xFFFFFFF0, 0x25, 0), (7, 0, 1),
                                                 (0xFFFFFFFE, 0xFFFFFFFF, 3)])
def test_keep_mask_against_a_scalar_loop(seed, seed_dev, group):
    B, N, p = 6, 45, 0.1
    mask = R.keep_mask(B, N, seed, p, seed_dev, group)
    assert mask.shape == (B, N, N) and mask.dtype == torch.bool
    thresh = int(float(np.float32(p)) * 2 ** 32)
    assert thresh == 429496736  # float32(0.1) = 0.100000001490116..., truncated as the kernels' cast does
    rs = np.random.RandomState(1)
    pairs = [(b, int(rs.randint(N)), int(rs.randint(N))) for b in range(B) for _ in range(60)]
    pairs += [(B - 1, N - 1, N - 1), (0, 0, 0), (B - 1, 0, N - 1)]
    for b, qi, ki in pairs:
        if group > 0:
            eff, row = (seed + seed_dev + 2 * (b // group)) % 2 ** 32, (b % group) * N + qi
        else:
            eff, row = (seed + seed_dev) % 2 ** 32, b * N + qi
        assert bool(mask[b, qi, ki]) == (_hash_scalar(eff, row, ki) >= thresh), (b, qi, ki)
    assert 0.07 < 1.0 - mask.double().mean().item() < 0.13


def test_keep_mask_seed_identities():
    """What the GPU cases assert of the kernels holds of the restatement: seed and seed_dev add modulo 2^32; a batch in groups
    of g draws, for episode e, the mask of a call on its clouds alone with seed + 2 e."""
    B, N, p = 6, 33, 0.1
    a, b = 0xFFFFFFF0, 0x25
    assert torch.equal(R.keep_mask(B, N, a, p, seed_dev=b), R.keep_mask(B, N, (a + b) % 2 ** 32, p))
    g, seed = 2, 0xFFFFFFFF
    whole = R.keep_mask(B, N, seed, p, group=g)
    for e in range(B // g):
        assert torch.equal(whole[e * g:(e + 1) * g], R.keep_mask(g, N, (seed + 2 * e) % 2 ** 32, p))
    assert not torch.equal(whole[:g], whole[g:2 * g])


def test_preconditions_of_the_dropout_edge_cases():
    seed, p, B, N = R.ALL_DROPPED
    keep = R.keep_mask(B, N, seed, p)
    none = ~keep.any(-1)
    assert [tuple(r) for r in none.nonzero().tolist()] == R.ALL_DROPPED_ROWS
    assert none[1:].any() and (~none).any()  # a row past cloud 0 loses every key; other rows keep some
    seed, p, B, N = R.TILE_DROPPED
    keep = R.keep_mask(B, N, seed, p)
    b, qi = R.TILE_DROPPED_ROW
    assert not keep[b, qi, 32:64].any() and keep[b, qi, :32].any() and keep[b, qi, 64:].any()
