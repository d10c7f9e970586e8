"""predict_scene's transfer="idw" -- the scores of a point without a vote interpolated from the three nearest voted points --
on the device (r3dfsseg_amd/scene.py, csrc/scene.hip) against the numpy restatement tests/scene_idw_ref.py.

Every comparison is torch.equal / np.array_equal: step 9' of the definition ("Labelling a scan") fixes
every operation and its order, so no tolerance is used in this file."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import scene_idw_ref as IR  # noqa: E402
import test_gpu_scene as TG  # noqa: E402  (its learners, its room, its rule for the uncapped scene)
import test_gpu_scene_sparse as TS  # noqa: E402  (its rule for the capped scene)

from r3dfsseg_amd import synthetic as S  # noqa: E402

pytestmark = pytest.mark.gpu

_same = TS._same


def _device_plan(g):
    from r3dfsseg_amd.scene import ScenePlan
    return ScenePlan(torch.from_numpy(g["scan"]).cuda(), g["N"], block_size=g["stride"] * g["r"], stride=g["stride"],
                     min_points=g["min_points"], max_chunks_per_block=g["cap"])


# ---- 1. vote and interpolation on given logits ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(IR.CASES))
def test_vote_and_idw_on_given_logits(name):
    from r3dfsseg_amd import ops
    ic = IR.case(name)  # asserts what the case exercises when it is built
    c = ic.c
    assert all(ic.has[k] for k in IR.CASES[name][1]) and ic.n_transferred > 0
    if name == "tiles":  # more candidates than one LDS tile, more receivers than one query tile
        dense = c.p.key == int(np.argmax(np.diff(c.p.cell_start)))
        assert int((dense & (c.votes > 0)).sum()) > ops.SCENE_TRANSFER_CAND_TILE
        assert int((dense & (c.votes == 0)).sum()) > ops.SCENE_TRANSFER_QUERY_TILE
    d = _device_plan(ic.geometry)
    scores, labels, votes = d.vote(torch.from_numpy(c.logits).cuda())
    assert _same(scores, c.scores) and _same(labels, c.labels) and _same(votes, c.votes)
    source, count, neighbours, weights = d.transfer(scores, labels, votes, mode="idw")
    assert _same(source, ic.source), int((source.cpu() != torch.from_numpy(ic.source)).sum())
    assert _same(neighbours, ic.neighbours), int((neighbours.cpu() != torch.from_numpy(ic.neighbours)).any(1).sum())
    assert _same(weights, ic.weights), int((weights.cpu() != torch.from_numpy(ic.weights)).any(1).sum())
    assert _same(scores, ic.i_scores), int((scores.cpu() != torch.from_numpy(ic.i_scores)).any(1).sum())
    assert _same(labels, ic.i_labels) and _same(votes, c.votes)  # votes stay 0 at a receiver
    n_tr = int(count.item())
    assert n_tr == ic.n_transferred and d.M - d.n_voted - n_tr == ic.n_unlabelled == int((labels == -1).sum())
    assert neighbours.is_cuda and weights.is_cuda and tuple(neighbours.shape) == tuple(weights.shape) == (d.M, 3)


def test_the_cases_cover_every_condition():
    assert IR.conditions_covered()


# ---- 2. the same votes through both modes ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small r=1 c=1", "wide N=4"])
def test_nearest_and_idw_share_source_count_and_voted_rows(name):
    ic = IR.case(name)
    d = _device_plan(ic.geometry)
    logits = torch.from_numpy(ic.c.logits).cuda()
    s0, l0, v0 = d.vote(logits)
    voted = v0 > 0
    s1, l1 = s0.clone(), l0.clone()
    source1, count1 = d.transfer(s1, l1, v0)  # mode="nearest" is the default
    n1 = int(count1.item())
    s2, l2 = s0.clone(), l0.clone()
    source2, count2, neighbours, weights = d.transfer(s2, l2, v0, mode="idw")
    assert torch.equal(source1, source2) and n1 == int(count2.item()) == ic.n_transferred
    for s, l in ((s1, l1), (s2, l2)):
        assert torch.equal(s[voted], s0[voted]) and torch.equal(l[voted], l0[voted])
    assert _same(s1, ic.c.t_scores) and _same(l1, ic.c.t_labels)  # the nearest transfer kept its bits
    got = ~voted & (source2 >= 0)
    assert ic.has["flip"] and not torch.equal(l1[got], l2[got])  # else this file could not tell the two apart
    assert torch.equal(neighbours[:, 0], source2)
    with pytest.raises(ValueError, match="transfer"):
        d.transfer(s2, l2, v0, mode="linear")


# ---- 3. end to end ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TG.CASES))
def test_capped_scene_equals_single_predict_calls_then_the_idw(name):
    learner, cfg = TG._learner(name)
    N = cfg["pc_npts"]
    scan = TG._room(cfg)
    # the nearest transfer leaves the voted rows as the votes made them, and step 9' reads no other row
    t_scores, t_labels, votes, t_source, n_tr, run = TS._capped_votes_by_single_calls(learner, scan, N, 1.0, 0.5, 100, 1)
    p = run.p
    scores, labels, source, n_idw, nbr, wgt = IR.idw(p, t_scores.numpy(), t_labels.numpy(), votes.numpy())
    assert run.n_run == p.n_blocks == 3 and run.n_skipped >= 5 and n_idw == n_tr > N and np.isfinite(scores).all()
    assert np.array_equal(source, t_source.numpy()) and np.array_equal(nbr[:, 0], source)
    first = None
    for G in (1, 2, 32):  # 2 leaves a remainder launch
        for _ in range(2):  # two calls give identical bits
            res = learner.predict_scene(scan, block_size=1.0, stride=0.5, min_points=100, groups_per_launch=G,
                                        max_chunks_per_block=1, transfer="idw")
            assert res.redone == 0 and (res.n_chunks, res.n_chunks_skipped, res.n_blocks) == (3, run.n_skipped, 3)
            assert torch.equal(res.votes.cpu(), votes) and _same(res.source, source), (name, G)
            assert _same(res.neighbours, nbr) and _same(res.weights, wgt), (name, G)
            assert _same(res.scores, scores), (name, G, np.abs(res.scores.cpu().numpy() - scores).max())
            assert _same(res.labels, labels), (name, G)
            assert res.n_transferred == n_tr and res.n_unlabelled == int((labels == -1).sum())
            assert res.neighbours.is_cuda and res.weights.is_cuda
            first = res if first is None else first
            for a, b in ((res.scores, first.scores), (res.labels, first.labels), (res.neighbours, first.neighbours),
                         (res.weights, first.weights), (res.source, first.source)):
                assert torch.equal(a, b)
    # "nearest" on the same scan: neither attribute
    near = learner.predict_scene(scan, block_size=1.0, stride=0.5, min_points=100, max_chunks_per_block=1, transfer="nearest")
    assert near.neighbours is None and near.weights is None and torch.equal(near.source, first.source)


# ---- 4. nobody receives ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TG.CASES))
def test_idw_without_receivers_leaves_the_votes(name):
    learner, cfg = TG._learner(name)
    room = TG._room(cfg)
    bad = room[:2].clone()
    bad[0, 0], bad[1, 2] = float("nan"), float("inf")
    scan = torch.cat([room[:100], bad, room[100:]])
    base = learner.predict_scene(scan, block_size=1.0, stride=0.5, min_points=100)
    res = learner.predict_scene(scan, block_size=1.0, stride=0.5, min_points=100, transfer="idw")
    assert base.neighbours is None and base.weights is None and base.n_unlabelled == 2
    assert res.n_transferred == 0 and res.n_chunks_skipped == 0 and res.n_unlabelled == 2 and res.redone == 0
    assert torch.equal(res.scores, base.scores) and torch.equal(res.labels, base.labels) and torch.equal(res.votes, base.votes)
    valid = torch.isfinite(scan[:, :3]).all(1).cuda()
    assert int((~valid).sum()) == 2 and (res.votes[valid] > 0).all()
    M = scan.shape[0]
    want = torch.full((M, 3), -1, dtype=torch.int64, device="cuda")
    want[valid, 0] = torch.nonzero(valid)[:, 0]
    assert torch.equal(res.neighbours, want) and torch.equal(res.source, want[:, 0])
    wgt = torch.zeros(M, 3, device="cuda")
    wgt[valid, 0] = 1
    assert torch.equal(res.weights, wgt)


# ---- 5. errors on the device path -----------------------------------------------------------------------------------------
def test_a_stale_fit_raises_with_idw():
    from r3dfsseg_amd.proto_learner import ProtoLearner
    cfg = S.make_cfg(**TG.CASES["proto"][1])
    learner = ProtoLearner(SimpleNamespace(**dict(cfg, model_checkpoint_path="synthetic")), mode="test")
    learner.fit(S.make_episode(cfg, seed=11)[0])
    scan = TG._room(cfg)
    assert learner.predict_scene(scan, stride=0.5, max_chunks_per_block=1, transfer="idw").n_transferred > 0
    with torch.no_grad():
        next(learner.model.parameters()).add_(1e-3)  # one in-place weight update
    with pytest.raises(ValueError, match="stale fit"):
        learner.predict_scene(scan, stride=0.5, max_chunks_per_block=1, transfer="idw")
