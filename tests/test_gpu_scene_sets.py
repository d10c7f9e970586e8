"""predict_scene_sets on the device (r3dfsseg_amd/scene.py, csrc/scene.hip, csrc/aux_heads.hip, csrc/head_proto.hip): per
support set the bits of predict_scene, one encoder pass per launch, and the merge against the numpy restatement
tests/scene_sets_ref.py.

Every comparison is torch.equal / np.array_equal: the definition ("Labelling a scan against several support
sets") fixes every operation and its order, so no tolerance is used in this file."""
import importlib
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import scene_sets_ref as R  # noqa: E402
from test_gpu_scene import CASES, _room  # noqa: E402  (its configurations and its 2 m x 1 m room)

from r3dfsseg_amd import synthetic as S  # noqa: E402

pytestmark = pytest.mark.gpu

SEEDS = (11, 12, 13)  # three support episodes, three fits
SCENE = dict(block_size=1.0, stride=0.5, min_points=100)
VARIANTS = [(None, None), (1, None), (1, "nearest"), (1, "idw")]  # (max_chunks_per_block, transfer)
_cache = {}


def _learner(name):
    """(learner of its own -- fit() replaces a learner's latest fit --, cfg, its three fits), built once per session."""
    if name not in _cache:
        path, over, noise, ev = CASES[name]
        mod, cls = path.split(".")
        cfg = S.make_cfg(**over)
        learner = getattr(importlib.import_module("r3dfsseg_amd." + mod), cls)(
            SimpleNamespace(**dict(cfg, model_checkpoint_path="synthetic")), mode="test")
        fits = [learner.fit(S.make_episode(cfg, seed=s, noise_ratio=noise)[0], eval=ev) for s in SEEDS]
        _cache[name] = (learner, cfg, fits)
    return _cache[name]


def _single(name, k, cap, transfer):
    """predict_scene against fit k alone: the reference of the per-set comparison, computed once."""
    key = (name, k, cap, transfer)
    if key not in _cache:
        learner, cfg, fits = _learner(name)
        res = learner.predict_scene(_room(cfg), fitted=fits[k], groups_per_launch=32, max_chunks_per_block=cap,
                                    transfer=transfer, **SCENE)
        assert res.redone == 0  # else pick another seed: the redone launch runs on another schedule
        _cache[key] = res
    return _cache[key]


def _same(a, b):
    return (a is None and b is None) or torch.equal(a, b)


# ---- 1. per set the bits of predict_scene ------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap,transfer", VARIANTS)
@pytest.mark.parametrize("name", list(CASES))
def test_every_set_has_the_bits_of_predict_scene(name, cap, transfer):
    learner, cfg, fits = _learner(name)
    scan = _room(cfg)
    K, C = len(fits), cfg["n_way"] + 1
    for G in (1, 3, 32):  # 3 leaves a remainder launch, 32 is one short launch
        res = learner.predict_scene_sets(scan, fits, groups_per_launch=G, max_chunks_per_block=cap, transfer=transfer, **SCENE)
        assert res.redone == 0
        assert res.scores.shape == (scan.shape[0], K, C) and res.scores.dtype == torch.float32
        assert res.set_labels.shape == (scan.shape[0], K) and res.set_labels.dtype == torch.int64
        assert res.votes.dtype == torch.int32 and res.labels.dtype == torch.int64 and res.set_of.dtype == torch.int32
        for k in range(K):
            one = _single(name, k, cap, transfer)
            assert torch.equal(res.votes, one.votes), (name, G, k)
            assert torch.equal(res.scores[:, k], one.scores), (name, G, k, (res.scores[:, k] - one.scores).abs().max().item())
            assert torch.equal(res.set_labels[:, k], one.labels), (name, G, k)
            assert _same(res.source, one.source) and _same(res.neighbours, one.neighbours) and _same(res.weights, one.weights)
            assert (res.n_blocks, res.n_chunks, res.n_unlabelled, res.n_transferred, res.n_chunks_skipped) == \
                (one.n_blocks, one.n_chunks, one.n_unlabelled, one.n_transferred, one.n_chunks_skipped)
        assert (res.source is None) == (transfer is None) and (res.neighbours is None) == (transfer != "idw")
    assert (cap is None and res.n_chunks_skipped == 0 and res.n_chunks >= 8) or (res.n_chunks == 3 and res.n_chunks_skipped >= 5)
    assert (transfer is None) == (res.n_transferred == 0)
    # the sets differ: the comparison above is not K times the same table
    assert not torch.equal(res.scores[:, 0], res.scores[:, 1]) and not torch.equal(res.scores[:, 1], res.scores[:, 2])


# ---- 2. one encoder pass per launch --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_one_encoder_pass_per_launch(name, monkeypatch):
    from r3dfsseg_amd import ops
    learner, cfg, fits = _learner(name)
    scan = _room(cfg)
    calls = dict(enc=0, lp=0)
    enc, lp = learner.model.getFeatures_pm, ops.label_propagate

    def count(key, fn):
        def wrapped(*a, **kw):
            calls[key] += 1
            return fn(*a, **kw)
        return wrapped
    monkeypatch.setattr(learner.model, "getFeatures_pm", count("enc", enc))
    monkeypatch.setattr(ops, "label_propagate", count("lp", lp))
    for G in (1, 3, 32):
        calls.update(enc=0, lp=0)
        res = learner.predict_scene_sets(scan, fits, groups_per_launch=G, **SCENE)
        launches = -(-res.n_chunks // G)
        assert res.redone == 0 and res.n_chunks >= 8
        assert calls["enc"] == launches, (name, G, calls)               # not K times that
        assert calls["lp"] == (launches if name == "mpti" else 0), (name, G, calls)
    calls.update(enc=0, lp=0)
    one = learner.predict_scene(scan, fitted=fits[0], groups_per_launch=3, **SCENE)
    assert calls["enc"] == -(-one.n_chunks // 3)                        # the counter counts what it should


# ---- 3. the merge kernel alone ---------------------------------------------------------------------------------------------------
def _merge_on_device(sc, votes, source, classes, background):
    from r3dfsseg_amd import ops
    dev = lambda a: None if a is None else torch.from_numpy(a).cuda()
    return [t.cpu().numpy() for t in ops.scene_merge_sets(dev(sc), dev(votes), dev(source), dev(classes), background)]


@pytest.mark.parametrize("K,C,M", [(1, 2, 300), (3, 3, 1000), (2, 4, 257), (8, 8, 777)])  # (8, 8): all 64 columns
def test_merge_kernel_equals_the_restatement(K, C, M):
    sc, votes, source = R.crafted(K, C, M, seed=K + C)
    has = (votes > 0) | (source >= 0)
    assert M % 256 != 0 and (~has).any() and ((votes == 0) & has).any()
    rs = np.random.RandomState(1)
    classes = rs.randint(-5, 6, (K, C - 1)).astype(np.int32)  # ids repeat across the sets
    classes[0, 0], classes[K - 1, C - 2] = -2 ** 31, 2 ** 31 - 1
    for src, cls, bg in ((source, classes, -1), (None, classes, 2 ** 40 + 3), (source, R.default_classes(K, C - 1), -2 ** 63)):
        want = R.merge(sc, votes, src, cls, bg)
        got = _merge_on_device(sc, votes, src, cls, bg)
        for name, g, w in zip(("set_labels", "labels", "set_of", "margin"), got, want):
            assert g.dtype == w.dtype and g.shape == w.shape, name
            assert np.array_equal(g.view(np.int32) if name == "margin" else g, w.view(np.int32) if name == "margin" else w), \
                (name, K, C, np.nonzero((g != w).reshape(M, -1).any(1))[0][:10])
    set_labels, labels, set_of, margin = want
    assert (set_of >= 0).any() and (labels == -2 ** 63).any() and np.isinf(margin).any()


# ---- 4. end to end ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transfer", [None, "idw"])
@pytest.mark.parametrize("name", list(CASES))
def test_labels_are_the_restated_merge_of_the_scores(name, transfer):
    learner, cfg, fits = _learner(name)
    scan = _room(cfg)
    kw = dict(SCENE, groups_per_launch=4, transfer=transfer, max_chunks_per_block=None if transfer is None else 1)
    classes = [[3, 8], [8, 1], [12, 5]]
    res = learner.predict_scene_sets(scan, fits, classes=classes, background=40, **kw)
    src = None if res.source is None else res.source.cpu().numpy()
    want = R.merge(res.scores.cpu().numpy(), res.votes.cpu().numpy(), src, np.array(classes, np.int32), 40)
    for got, w in zip((res.set_labels, res.labels, res.set_of, res.margin), want):
        assert np.array_equal(got.cpu().numpy(), w)
    assert (res.set_of >= 0).any() and set(res.labels.unique().tolist()) <= {-1, 40, 3, 8, 1, 12, 5}
    assert res.n_unlabelled == int(((res.votes == 0) & (True if src is None else res.source < 0)).sum())
    again = learner.predict_scene_sets(scan, fits, classes=classes, background=40, **kw)
    for a in ("scores", "set_labels", "votes", "labels", "set_of", "margin"):
        assert torch.equal(getattr(again, a), getattr(res, a)), a
    # K = 1 with the default classes: the single set's label, shifted by one
    one = learner.predict_scene_sets(scan, fits[1:2], background=-9, **kw)
    sl = one.set_labels[:, 0]
    assert torch.equal(sl, _single(name, 1, kw["max_chunks_per_block"], transfer).labels)
    assert torch.equal(one.labels, torch.where(sl >= 1, sl - 1, torch.where(sl == 0, -9, -1)))
    assert torch.equal(one.set_of.long(), torch.where(sl >= 1, 0, -1))


# ---- 5. the head halves alone ------------------------------------------------------------------------------------------------------
def test_attach_sets_equals_attach_per_fit():
    from r3dfsseg_amd import ops
    learner, cfg, fits = _learner("mpti")
    m = learner.model
    K, G, N = 2, 3, cfg["pc_npts"]
    heads = [f.head for f in fits[:K]]
    assert not torch.equal(heads[0].nodes, heads[1].nodes)
    feat = torch.randn(G * N, m.feat_dim, device="cuda")

    def buffers(E):
        hb = ops.HeadBuffers(m.n_way, m.k_shot, N, N, m.n_subprototypes, m.k_connect, m.feat_dim, "cuda", E=E)
        hb.nodes.fill_(7.0)  # rows no call writes (prototype slots a fit left empty) compare equal
        hb.Y.fill_(7.0)
        return hb
    sets = buffers(G * K)
    ops.head_attach_queries_sets(sets, heads, ops.head_fit_table(heads, "cuda"), feat)
    n = sets.n_cap
    for k in range(K):
        one = buffers(G)
        ops.head_attach_queries(one, heads[k], feat)
        for g in range(G):
            s = g * K + k
            assert torch.equal(sets.nodes[s * n:(s + 1) * n], one.nodes[g * n:(g + 1) * n]), (k, g)
            assert torch.equal(sets.Y[s * n:(s + 1) * n], one.Y[g * n:(g + 1) * n]), (k, g)
            assert torch.equal(sets.desc[s], one.desc[g]) and torch.equal(sets.cluster_count[s], one.cluster_count[g]), (k, g)
            n_proto = int(one.desc[g, ops.HD_N_PROTO])
            assert 0 < n_proto <= heads[k].proto_cap and int(one.desc[g, ops.HD_N_NODES]) == n_proto + N
            assert torch.equal(sets.nodes[s * n + n_proto:s * n + n_proto + N], feat[g * N:(g + 1) * N])


@pytest.mark.parametrize("n_way,D,K,method,G,n_pts", [(2, 192, 3, "cosine", 3, 100), (7, 256, 8, "euclidean", 2, 70),
                                                      (1, 64, 32, "cosine", 1, 5), (3, 100, 5, "euclidean", 40, 9),
                                                      (4, 36, 1, "cosine", 2, 300)])
def test_similarity_sets_equals_similarity_per_table(n_way, D, K, method, G, n_pts):
    """Two label planes above three ways, all 64 prototype rows at D = 256 (the table then needs more LDS than a kernel gets by
    default), D that is no multiple of the wave, more groups than tiles, one set."""
    from r3dfsseg_amd import ops
    g = torch.Generator().manual_seed(n_way * 100 + K)
    gap = 7  # rows between the groups that belong to nobody
    feat = torch.randn(G * (n_pts + gap), D, generator=g).cuda()
    tables = torch.randn(K, n_way + 1, D, generator=g).cuda()
    Z = ops.protonet_similarity_sets(feat, tables, n_way, method, G, n_pts, q_sys_rows=n_pts + gap)
    planes = 1 if n_way <= 3 else 2
    Z = Z.reshape(planes, G, K, n_pts, 4)
    for k in range(K):
        one = ops.protonet_similarity(feat, tables[k], n_way, method, G, n_pts, q_sys_rows=n_pts + gap).reshape(planes, G, n_pts, 4)
        assert torch.isfinite(one).all() and torch.equal(Z[:, :, k], one), (k, (Z[:, :, k] - one).abs().max().item())
