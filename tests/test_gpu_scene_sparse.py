"""predict_scene on a subsample -- a cap on the chunks of a block, and the transfer to the points without a vote -- on the
device (r3dfsseg_amd/scene.py, csrc/scene.hip) against the numpy restatement tests/scene_sparse_ref.py.

Every comparison is torch.equal / np.array_equal: steps 7a, 8' and 9 of the definition ("Labelling a
scan") fix every operation and its order, so no tolerance is used in this file."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import scene_cases as SC  # noqa: E402
import scene_sparse_ref as SR  # noqa: E402
import test_gpu_scene as TG  # noqa: E402  (its learners, its room, its rule for the uncapped scene)
from scene_ref import RefPlan  # noqa: E402

from r3dfsseg_amd import synthetic as S  # noqa: E402

pytestmark = pytest.mark.gpu


def _scan_of(name):
    which, r, cap, _ = SR.CASES[name]
    if which == "small":
        return SC.small_scan()[0], SC.SMALL, r, cap
    return SC.medium_scan(), SC.MEDIUM, r, cap


def _device_plan(scan, par, r, cap):
    from r3dfsseg_amd.scene import ScenePlan
    return ScenePlan(torch.from_numpy(scan).cuda(), par["N"], block_size=par["stride"] * r, stride=par["stride"],
                     min_points=par["min_points"], max_chunks_per_block=cap)


def _run_clouds(d, C=9):
    """(prepared clouds (n_run, C, N), slot map (n_run, N)) of every chunk that runs, one launch."""
    out = torch.empty(d.n_run, C, d.N, device="cuda")
    sm = torch.empty(d.n_run, d.N, device="cuda", dtype=torch.int32)
    d.prepare(0, out, 3, 6, slot_map=sm)
    return out, sm


def _same(dev, want):
    want = torch.from_numpy(np.ascontiguousarray(want))
    return dev.dtype == want.dtype and torch.equal(dev.cpu(), want)


# ---- 1. the plan under a cap ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SR.CASES))
def test_plan_under_a_cap(name):
    from r3dfsseg_amd import ops
    from r3dfsseg_amd.scene import staging
    scan, par, r, cap = _scan_of(name)
    c = SR.case(name)
    run = c.run
    d = _device_plan(scan, par, r, cap)
    assert (d.n_chunks, d.n_run, d.n_skipped, d.n_blocks) == (c.p.n_chunks, run.n_run, run.n_skipped, c.p.n_blocks)
    assert run.n_skipped > 0 and d.n_voted == int((c.votes > 0).sum())
    assert _same(d.run_chunk0, run.run_chunk0) and _same(d.run_block, run.run_block)
    assert _same(d.block_chunk0, c.p.block_chunk0) and _same(d.chunk_block, c.p.chunk_block)  # the full tables stay
    want = run.prepared()
    cm, sm = _run_clouds(d)                                   # contiguous channel-major
    assert _same(sm, run.slot_map) and _same(cm, want)
    pm = staging(run.n_run, 9, d.N, "cuda")                   # point-major rows, viewed (G, C, N)
    assert ops.is_point_major_view(pm) and not pm.is_contiguous()
    pm.transpose(1, 2).fill_(float("nan"))
    sm2 = torch.empty_like(sm)
    d.prepare(0, pm, 3, 6, slot_map=sm2)
    assert torch.equal(pm, cm) and torch.equal(sm2, sm)
    # a launch that starts in the middle and takes the remainder
    part = torch.empty(run.n_run - 2, 9, d.N, device="cuda")
    d.prepare(2, part, 3, 6)
    assert torch.equal(part, cm[2:])


@pytest.mark.parametrize("r", [1, 2])
def test_a_cap_that_skips_nothing_equals_the_existing_entry_points(r):
    scan, _ = SC.small_scan()
    p = SC.small_plan(r)
    nc_max = int(np.diff(p.block_chunk0).max())
    full = _device_plan(scan, SC.SMALL, r, None)
    logits = torch.from_numpy(SR.random_logits(p.n_chunks, p.N, 5)).cuda()
    want_clouds, want_sm = _run_clouds(full)
    want_vote = full.vote(logits)
    assert _same(want_sm, p.slot_map) and full.n_run == p.n_chunks and full.n_skipped == 0
    for cap in (nc_max, nc_max + 1, 2 ** 40):
        d = _device_plan(scan, SC.SMALL, r, cap)
        assert (d.n_run, d.n_skipped, d.n_chunks, d.n_voted) == (p.n_chunks, 0, p.n_chunks, full.n_voted)
        assert torch.equal(d.run_chunk0, full.block_chunk0) and torch.equal(d.run_block, full.chunk_block)
        clouds, sm = _run_clouds(d)
        assert torch.equal(clouds, want_clouds) and torch.equal(sm, want_sm)
        for a, b in zip(d.vote(logits), want_vote):
            assert a.dtype == b.dtype and torch.equal(a, b)


# ---- 2. vote and transfer on given logits ---------------------------------------------------------------------------------
def _vote_and_transfer(d, c):
    """The device's step 8' and step 9 on the case's logits against the case; -> what the device returned."""
    scores, labels, votes = d.vote(torch.from_numpy(c.logits).cuda())
    assert _same(scores, c.scores) and _same(labels, c.labels) and _same(votes, c.votes)
    source, count = d.transfer(scores, labels, votes)
    assert _same(source, c.source), int((source.cpu() != torch.from_numpy(c.source)).sum())
    assert _same(scores, c.t_scores) and _same(labels, c.t_labels) and _same(votes, c.votes)  # votes stay 0 at a receiver
    n_tr = int(count.item())
    assert n_tr == c.n_transferred and d.M - d.n_voted - n_tr == c.n_unlabelled == int((labels == -1).sum())
    return scores, labels, votes, source


@pytest.mark.parametrize("name", list(SR.CASES))
def test_vote_and_transfer_on_given_logits(name):
    scan, par, r, cap = _scan_of(name)
    c = SR.case(name)  # asserts what the case exercises when it is built
    assert all(c.has[k] for k in SR.CASES[name][3]) and c.n_transferred > 0
    _vote_and_transfer(_device_plan(scan, par, r, cap), c)


def test_the_cases_cover_every_condition():
    assert SR.conditions_covered()


# ---- 3. no source -----------------------------------------------------------------------------------------------------------
def test_points_without_a_candidate_stay_unlabelled():
    scan = SC.wide_scan()
    par = dict(SC.WIDE, min_points=2)
    p = RefPlan(scan, par["N"], block_size=1.0, stride=1.0, min_points=2)
    assert p.n_cells == 65536
    c = SR.Case(p, None, seed=2)
    alone = p.valid & (c.votes == 0) & (c.source < 0)
    assert c.has["no_source"] and c.has["dropped"] and c.n_transferred > 0 and c.run.n_skipped == 0
    assert alone.sum() > 100 and (np.diff(p.cell_start)[p.key[alone]] == 1).all()  # isolated single-point cells
    assert (c.t_labels[alone] == -1).all() and c.n_unlabelled == int(alone.sum()) + int((~p.valid).sum())
    d = _device_plan(scan, par, 1, None)
    _, labels, _, source = _vote_and_transfer(d, c)
    where = torch.from_numpy(alone)
    assert (source.cpu()[where] == -1).all() and (labels.cpu()[where] == -1).all()


# ---- 4. more candidates than one LDS tile, more queries than one workgroup -------------------------------------------------
def test_transfer_across_candidate_and_query_tiles():
    from r3dfsseg_amd import ops
    T = SR.TILES
    scan = SR.tile_scan()
    p = RefPlan(scan, T["N"], block_size=1.0, stride=1.0, min_points=T["min_points"])
    assert (p.ncx, p.ncy, p.r) == (2, 2, 1) and scan.shape[0] == T["M"]
    c = SR.Case(p, T["cap"], seed=4, by_cell=True)
    dense = int(np.argmax(np.diff(p.cell_start)))
    in_dense = p.key == dense
    assert in_dense.sum() >= T["dense"]
    n_voted, n_unvoted = int((in_dense & (c.votes > 0)).sum()), int((in_dense & (c.votes == 0)).sum())
    assert n_voted > ops.SCENE_TRANSFER_CAND_TILE and n_unvoted > ops.SCENE_TRANSFER_QUERY_TILE
    assert n_unvoted % ops.SCENE_TRANSFER_QUERY_TILE != 0 and int((c.votes > 0).sum()) % ops.SCENE_TRANSFER_CAND_TILE != 0
    assert c.has["capped"] and c.has["neighbour"] and c.n_unlabelled == 0
    _vote_and_transfer(_device_plan(scan, T, 1, T["cap"]), c)


# ---- 5. end to end ---------------------------------------------------------------------------------------------------------
def _capped_votes_by_single_calls(learner, scan, N, block_size, stride, min_points, cap):
    """The rule: model.predict on every chunk that runs ALONE, the sum of step 8' in torch (chunk after chunk, slot after
    slot: the slots of one wrap-around round are distinct points, so a round is one indexed add), then the numpy transfer.
    -> (scores, labels, votes, source, n_transferred, run plan)."""
    from r3dfsseg_amd.scene import ScenePlan
    m = learner.model
    p = RefPlan(scan.numpy(), N, block_size=block_size, stride=stride, min_points=min_points)
    run = SR.RunPlan(p, cap)
    d = ScenePlan(scan.cuda(), N, block_size=block_size, stride=stride, min_points=min_points, max_chunks_per_block=cap)
    chunks, sm = _run_clouds(d)
    assert _same(sm, run.slot_map)
    K = m.n_way + 1
    scores, votes = torch.zeros(p.M, K), torch.zeros(p.M, dtype=torch.int32)
    with torch.no_grad():
        for c in range(run.n_run):
            logits, loss = m.predict(learner.fitted, chunks[c][None])
            if hasattr(m, "lp_converged"):
                assert m.lp_converged()  # else the scene would be redone on another schedule: pick another seed
            assert logits.shape == (1, K, N) and loss is None
            z = logits[0].cpu()
            ln = p.chunks[run.run[c]][2]
            for t0 in range(0, N, ln):
                idx = torch.from_numpy(run.slot_map[c, t0:t0 + ln].astype(np.int64))
                scores[idx] = scores[idx] + z[:, t0:t0 + ln].t()
                votes[idx] += 1
    labels = torch.where(votes > 0, torch.from_numpy(scores.numpy().argmax(1)), torch.tensor(-1))
    ts, tl, source, n_tr = SR.transfer(p, scores.numpy(), labels.numpy(), votes.numpy())
    return torch.from_numpy(ts), torch.from_numpy(tl), votes, torch.from_numpy(source), n_tr, run


@pytest.mark.parametrize("name", list(TG.CASES))
def test_capped_scene_equals_single_predict_calls_then_the_transfer(name):
    learner, cfg = TG._learner(name)
    N = cfg["pc_npts"]
    scan = TG._room(cfg)
    scores, labels, votes, source, n_tr, run = _capped_votes_by_single_calls(learner, scan, N, 1.0, 0.5, 100, 1)
    p = run.p
    assert run.n_run == p.n_blocks == 3 and run.n_skipped >= 5 and n_tr > N and torch.isfinite(scores).all()
    for G in (1, 2, 32):  # 2 leaves a remainder launch
        res = learner.predict_scene(scan, block_size=1.0, stride=0.5, min_points=100, groups_per_launch=G,
                                    max_chunks_per_block=1, transfer="nearest")
        assert res.redone == 0 and (res.n_chunks, res.n_chunks_skipped, res.n_blocks) == (3, run.n_skipped, 3)
        assert torch.equal(res.votes.cpu(), votes) and torch.equal(res.source.cpu(), source), (name, G)
        assert torch.equal(res.scores.cpu(), scores), (name, G, (res.scores.cpu() - scores).abs().max().item())
        assert torch.equal(res.labels.cpu(), labels), (name, G)
        assert res.n_transferred == n_tr and res.n_unlabelled == int((labels == -1).sum())
        assert res.source.dtype == torch.int64 and res.source.is_cuda
    # a cap alone: the same votes, nothing transferred
    cap = learner.predict_scene(scan, block_size=1.0, stride=0.5, min_points=100, max_chunks_per_block=1)
    assert cap.source is None and cap.n_transferred == 0 and torch.equal(cap.votes.cpu(), votes)
    assert cap.n_unlabelled == int((votes == 0).sum()) == int((cap.labels == -1).sum())
    assert (cap.n_chunks, cap.n_chunks_skipped) == (3, run.n_skipped)
    voted = votes > 0
    assert torch.equal(cap.scores.cpu()[voted], scores[voted]) and (cap.scores.cpu()[~voted] == 0).all()


@pytest.mark.parametrize("name", list(TG.CASES))
def test_defaults_are_unchanged_and_the_transfer_alone_leaves_voted_points(name):
    learner, cfg = TG._learner(name)
    N = cfg["pc_npts"]
    room = TG._room(cfg)
    # today's result, by today's rule
    scores, labels, votes, p = TG._votes_by_single_calls(learner, room, N, 1.0, 0.5, 100)
    res = learner.predict_scene(room, block_size=1.0, stride=0.5, min_points=100)
    assert res.source is None and res.n_transferred == 0 and res.n_chunks_skipped == 0 and res.n_chunks == p.n_chunks
    assert torch.equal(res.votes.cpu(), votes) and torch.equal(res.scores.cpu(), scores) and torch.equal(res.labels.cpu(), labels)
    # blocks of one cell, and 20 points in a cell of their own beside the room: a dropped block next to kept ones
    near = room[:20].clone()
    near[:, 0] = room[:, 0].max() + 0.05 + 0.02 * torch.arange(20)
    scan = torch.cat([room[:300], near, room[300:]])
    base = learner.predict_scene(scan, block_size=0.5, stride=0.5, min_points=100)
    res = learner.predict_scene(scan, block_size=0.5, stride=0.5, min_points=100, transfer="nearest")
    v = base.votes > 0
    assert base.n_unlabelled == 20 == int((~v).sum()) and not v[300:320].any()
    assert torch.equal(res.votes, base.votes) and (res.n_chunks, res.n_chunks_skipped, res.redone) == (base.n_chunks, 0, 0)
    assert torch.equal(res.scores[v], base.scores[v]) and torch.equal(res.labels[v], base.labels[v])
    assert torch.equal(res.source[v], torch.nonzero(v)[:, 0])
    bv = base.votes.cpu().numpy()
    ts, tl, source, n_tr = SR.transfer(RefPlan(scan.numpy(), N, block_size=0.5, stride=0.5, min_points=100),
                                       base.scores.cpu().numpy(), base.labels.cpu().numpy(), bv)
    assert n_tr == 20 == res.n_transferred and res.n_unlabelled == 0
    assert _same(res.source, source) and _same(res.scores, ts) and _same(res.labels, tl)


# ---- 6. errors on the device path ---------------------------------------------------------------------------------------
def test_errors_on_the_device_path_with_the_new_arguments():
    from r3dfsseg_amd import ops
    from r3dfsseg_amd.proto_learner import ProtoLearner
    from r3dfsseg_amd.scene import ScenePlan
    cfg = S.make_cfg(**TG.CASES["proto"][1])
    learner = ProtoLearner(SimpleNamespace(**dict(cfg, model_checkpoint_path="synthetic")), mode="test")
    learner.fit(S.make_episode(cfg, seed=11)[0])
    scan = TG._room(cfg)
    # a short workspace at the new entry points is an error code, not an overrun
    d = ScenePlan(scan.cuda(), cfg["pc_npts"], 1.0, 0.5, 100, max_chunks_per_block=1)
    short = d.sws[:-1]
    with pytest.raises(RuntimeError, match="sparse workspace"):
        ops.scene_run_tables(d.M, d.ncx, d.ncy, d.r, d.N, d.chunk_cap, d.ws, 1, short)
    out = torch.empty(d.n_run, 9, d.N, device="cuda")
    with pytest.raises(RuntimeError, match="sparse workspace"):
        ops.scene_prepare(d.scan, d.ncx, d.ncy, d.r, d.N, d.chunk_cap, d.ws, 0, out, 3, 6, sws=short)
    logits = torch.zeros(d.n_run, 3, d.N, device="cuda")
    with pytest.raises(RuntimeError, match="sparse workspace"):
        ops.scene_vote(d.M, d.ncx, d.ncy, d.r, d.N, d.chunk_cap, d.ws, logits, sws=short)
    scores, labels, votes = d.vote(logits)
    with pytest.raises(RuntimeError, match="sparse workspace"):
        ops.scene_transfer(d.scan, d.ncx, d.ncy, d.chunk_cap, d.ws, short, scores, labels, votes)
    with pytest.raises(RuntimeError, match="workspace"):
        ops.scene_transfer(d.scan, d.ncx, d.ncy, d.chunk_cap, d.ws[:-1], d.sws, scores, labels, votes)
    with pytest.raises(ValueError, match="logits of"):
        d.vote(torch.zeros(d.n_chunks, 3, d.N, device="cuda"))
    assert learner.predict_scene(scan, stride=0.5, max_chunks_per_block=1, transfer="nearest").n_transferred > 0
    with torch.no_grad():
        next(learner.model.parameters()).add_(1e-3)  # one in-place weight update
    with pytest.raises(ValueError, match="stale fit"):
        learner.predict_scene(scan, stride=0.5, max_chunks_per_block=1, transfer="nearest")
