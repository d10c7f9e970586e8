"""predict_scene on the device (r3dfsseg_amd/scene.py, csrc/scene.hip, csrc/scene_sort.hip) against the numpy restatement tests/scene_ref.py.

Every comparison is torch.equal / np.array_equal: the definition ("Labelling a scan") fixes every operation
and its order, so no tolerance is used in this file."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import scene_cases as SC  # noqa: E402
from scene_ref import RefPlan  # noqa: E402

from r3dfsseg_amd import synthetic as S  # noqa: E402

pytestmark = pytest.mark.gpu


def _device_plan(scan, N, r, stride, min_points):
    from r3dfsseg_amd.scene import ScenePlan
    return ScenePlan(torch.from_numpy(scan).cuda(), N, block_size=stride * r, stride=stride, min_points=min_points)


def _slot_map(plan, C=9):
    """(prepared clouds (n_chunks, C, N) in the contiguous layout, slot map (n_chunks, N)) of every chunk, one launch."""
    out = torch.empty(plan.n_chunks, C, plan.N, device="cuda")
    sm = torch.empty(plan.n_chunks, plan.N, device="cuda", dtype=torch.int32)
    plan.prepare(0, out, 3, 6, slot_map=sm)
    return out, sm


def _same_plan(d, p):
    """The device plan d against the restatement p: every table of steps 1-5."""
    assert (d.x0, d.y0, d.xmax, d.ymax) == (p.x0, p.y0, p.xmax, p.ymax) and d.n_valid == int(p.valid.sum())
    assert (d.ncx, d.ncy, d.r, d.nbx, d.nby) == (p.ncx, p.ncy, p.r, p.nbx, p.nby)
    assert np.array_equal(d.cell_start.cpu().numpy(), p.cell_start)           # counts and offsets of the cells
    assert np.array_equal(d.order.cpu().numpy(), p.order)                     # the stable sort
    assert np.array_equal(d.sorted_key.cpu().numpy()[:d.n_valid], p.key[p.order])
    pos = d.pos.cpu().numpy()
    assert np.array_equal(pos[p.order], np.arange(d.n_valid)) and (pos[~p.valid] >= d.n_valid).all()
    assert (d.n_blocks, d.n_chunks) == (p.n_blocks, p.n_chunks)
    assert np.array_equal(d.block_points.cpu().numpy(), p.block_points)
    assert np.array_equal(d.block_chunk0.cpu().numpy(), p.block_chunk0)
    assert np.array_equal(d.chunk_block.cpu().numpy(), p.chunk_block)         # the chunk table
    assert d.n_voted == len(set(q for b, lst in enumerate(p.block_list) if p.kept[b] for q in lst))
    _, sm = _slot_map(d)
    assert np.array_equal(sm.cpu().numpy(), p.slot_map)                       # which scan point sits in which slot


# ---- 1. the plan, small: one tile, one radix pass, every branch of the chunk rule ----------------------------------------
@pytest.mark.parametrize("r", [2, 1])
def test_plan_small(r):
    scan, info = SC.small_scan()
    assert info["on_boundary"] >= 20 and info["n_dup"] >= 5 and info["n_bad"] == 3
    p = SC.small_plan(r)
    _same_plan(_device_plan(scan, SC.SMALL["N"], r, SC.SMALL["stride"], SC.SMALL["min_points"]), p)


@pytest.mark.parametrize("r", [1, 2])
def test_without_a_cap_every_chunk_is_a_run_chunk(r):
    """r3d_scene_plan alone leaves the record of a cap nobody reaches -- run chunks = chunks, none skipped, the same voted
    points -- and ScenePlan's run tables are then the plan's own chunk tables."""
    from r3dfsseg_amd import ops
    scan, _ = SC.small_scan()
    p = SC.small_plan(r)
    d = _device_plan(scan, SC.SMALL["N"], r, SC.SMALL["stride"], SC.SMALL["min_points"])
    assert d.cap is None and d.sws is None  # no run tables were written
    at = ops.scene_workspace(d.M, d.ncx, d.ncy, d.chunk_cap, "cuda")[1]["rec"]
    rec = d.ws[at:at + 8].tolist()
    assert rec[0] == p.n_chunks > 0 and rec[2] > 0
    assert rec[4] == rec[0] and rec[5] == 0 and rec[6] == rec[2]
    assert (d.n_run, d.n_skipped, d.n_voted) == (rec[0], 0, rec[2])
    assert torch.equal(d.run_chunk0, d.block_chunk0) and torch.equal(d.run_block, d.chunk_block)
    assert d.run_chunk0.data_ptr() == d.block_chunk0.data_ptr() and d.run_block.data_ptr() == d.chunk_block.data_ptr()


# ---- 2. more than one tile and more than one radix pass ----------------------------------------------------------------------
@pytest.mark.parametrize("r", [1, 4])
def test_plan_many_tiles_two_radix_passes(r):
    scan = SC.medium_scan()
    assert scan.shape[0] == 70001 > 2048 * 34
    p = SC.medium_plan(r)
    assert p.n_cells >= 256  # keys need a second 8-bit digit
    _same_plan(_device_plan(scan, SC.MEDIUM["N"], r, SC.MEDIUM["stride"], SC.MEDIUM["min_points"]), p)


def test_plan_three_radix_passes_at_65536_cells():
    p = SC.wide_plan()
    assert p.n_cells == 65536 and (np.diff(p.cell_start) > 1).any()
    _same_plan(_device_plan(SC.wide_scan(), SC.WIDE["N"], 1, SC.WIDE["stride"], SC.WIDE["min_points"]), p)


# ---- 3. prepared clouds --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", [2, 1])
def test_prepared_clouds_in_both_layouts(r):
    from r3dfsseg_amd import ops
    from r3dfsseg_amd.scene import staging
    scan, _ = SC.small_scan()
    p = SC.small_plan(r)
    want = p.prepared()
    assert want.shape == (p.n_chunks, 9, 256) and np.isfinite(want).all()
    d = _device_plan(scan, 256, r, 0.5, SC.SMALL["min_points"])
    cm, _ = _slot_map(d)                                   # contiguous channel-major
    assert np.array_equal(cm.cpu().numpy(), want)
    pm = staging(p.n_chunks, 9, 256, "cuda")               # point-major rows, viewed (G, C, N)
    assert ops.is_point_major_view(pm) and not pm.is_contiguous()
    pm.transpose(1, 2).fill_(float("nan"))
    d.prepare(0, pm, 3, 6)
    assert torch.equal(pm, cm) and np.array_equal(pm.transpose(1, 2).contiguous().cpu().numpy(), want.transpose(0, 2, 1))
    # a launch that starts in the middle and takes the remainder
    part = torch.empty(p.n_chunks - 3, 9, 256, device="cuda")
    d.prepare(3, part, 3, 6)
    assert torch.equal(part, cm[3:])
    # the flat block (block 0: all its points share one z): XYZ's z channel is 0, not the reference's 0 / 0
    assert p.chunk_block[0] == 0 and p.chunk_block[1] != 0
    assert (want[0, 8] == 0).all() and (want[0, 2] == 0).all() and (cm[0, 8] == 0).all() and not torch.isnan(cm).any()
    # xyz and xyzXYZ models: the same channels without the colour
    d3 = _device_plan(np.ascontiguousarray(scan[:, :3]), 256, r, 0.5, SC.SMALL["min_points"])
    for rgb_ch, XYZ_ch, C in ((-1, 3, 6), (-1, -1, 3)):
        out = torch.empty(p.n_chunks, C, 256, device="cuda")
        d3.prepare(0, out, rgb_ch, XYZ_ch)
        assert np.array_equal(out.cpu().numpy(), p.prepared(rgb=False, XYZ=XYZ_ch >= 0))


# ---- 4. end to end ---------------------------------------------------------------------------------------------------------
# name -> (learner, cfg overrides, noise_ratio of the support episode, eval flag of the fit)
CASES = {
    "proto": ("proto_learner.ProtoLearner", dict(n_way=2, k_shot=1, pc_npts=256, dist_method="cosine"), 0.0, False),
    "contrast": ("proto_contrast_learner.ProtoContrastLearner", dict(n_way=2, k_shot=5, pc_npts=512), 0.4, False),
    "mpti": ("mpti_learner.MPTILearner_V3", dict(n_way=2, k_shot=2, pc_npts=512, n_subprototypes=20), 0.0, True),
}
_cache = {}


def _learner(name):
    """(learner with a fitted support set, cfg), built once per session."""
    if name not in _cache:
        import importlib
        path, over, noise, ev = CASES[name]
        mod, cls = path.split(".")
        cfg = S.make_cfg(**over)
        learner = getattr(importlib.import_module("r3dfsseg_amd." + mod), cls)(
            SimpleNamespace(**dict(cfg, model_checkpoint_path="synthetic")), mode="test")
        learner.fit(S.make_episode(cfg, seed=11, noise_ratio=noise)[0], eval=ev)
        _cache[name] = (learner, cfg)
    return _cache[name]


def _room(cfg, seed=5):
    """A 2 m x 1 m room of 6 N points: at stride 0.5 and r = 2 three blocks of about 3 N points, so 9 to 12 chunks."""
    N = cfg["pc_npts"]
    return S.make_scene(cfg, seed=seed, extent=(1.999, 0.999, 3.0), n_points=6 * N - 70)[0]


def _votes_by_single_calls(learner, scan, N, block_size, stride, min_points):
    """The rule: model.predict on every prepared chunk ALONE, then the sum of step 8 in torch -- chunk after chunk (block id
    ascending), and inside a chunk slot after slot: the slots of one wrap-around round are distinct points, so a round is
    one indexed add.  -> (scores, labels, votes, plan)."""
    from r3dfsseg_amd.scene import ScenePlan
    m = learner.model
    p = RefPlan(scan.numpy(), N, block_size=block_size, stride=stride, min_points=min_points)
    d = ScenePlan(scan.cuda(), N, block_size=block_size, stride=stride, min_points=min_points)
    chunks, sm = _slot_map(d)
    assert np.array_equal(sm.cpu().numpy(), p.slot_map)
    K = m.n_way + 1
    scores, votes = torch.zeros(p.M, K), torch.zeros(p.M, dtype=torch.int32)
    with torch.no_grad():
        for c in range(p.n_chunks):
            logits, loss = m.predict(learner.fitted, chunks[c][None])
            if hasattr(m, "lp_converged"):
                assert m.lp_converged()  # else the scene would be redone on another schedule: pick another seed
            assert logits.shape == (1, K, N) and loss is None
            z = logits[0].cpu()
            ln = p.chunks[c][2]
            for t0 in range(0, N, ln):
                idx = torch.from_numpy(p.slot_map[c, t0:t0 + ln].astype(np.int64))
                scores[idx] = scores[idx] + z[:, t0:t0 + ln].t()
                votes[idx] += 1
    labels = torch.where(votes > 0, torch.from_numpy(scores.numpy().argmax(1)), torch.tensor(-1))
    return scores, labels, votes, p


@pytest.mark.parametrize("name", list(CASES))
def test_scene_equals_single_predict_calls_summed_in_order(name):
    learner, cfg = _learner(name)
    N = cfg["pc_npts"]
    scan = _room(cfg)
    scores, labels, votes, p = _votes_by_single_calls(learner, scan, N, 1.0, 0.5, 100)
    assert 8 <= p.n_chunks <= 12 and p.r == 2 and (p.block_points[p.kept] >= N // 2).all() and p.n_blocks == 3
    assert torch.isfinite(scores).all()
    for G in (1, 3, 32):  # 3 leaves a remainder launch, 32 is one short launch
        res = learner.predict_scene(scan, block_size=1.0, stride=0.5, min_points=100, groups_per_launch=G)
        assert res.redone == 0 and (res.n_chunks, res.n_blocks) == (p.n_chunks, p.n_blocks)
        assert res.labels.dtype == torch.int64 and res.votes.dtype == torch.int32 and res.scores.shape == (p.M, cfg["n_way"] + 1)
        assert torch.equal(res.votes.cpu(), votes), (name, G)
        assert torch.equal(res.scores.cpu(), scores), (name, G, (res.scores.cpu() - scores).abs().max().item())
        assert torch.equal(res.labels.cpu(), labels), (name, G)
        assert res.n_unlabelled == int((votes == 0).sum()) == 0


def test_heavy_wrap_around():
    """A 40-point block at N = 256: one chunk whose 40 members fill 6.4 rounds of slots."""
    learner, cfg = _learner("proto")
    scan = S.make_scene(cfg, seed=9, extent=(0.9, 0.9, 2.0), n_points=40)[0]
    scores, labels, votes, p = _votes_by_single_calls(learner, scan, 256, 1.0, None, 1)
    assert p.n_chunks == 1 and p.chunks[0][2] == 40 and sorted(set(votes.tolist())) == [6, 7]
    res = learner.predict_scene(scan, min_points=1)
    assert torch.equal(res.votes.cpu(), votes) and torch.equal(res.scores.cpu(), scores) and torch.equal(res.labels.cpu(), labels)


# ---- 5. bookkeeping --------------------------------------------------------------------------------------------------------
def test_bookkeeping_of_invalid_points_and_dropped_blocks():
    learner, cfg = _learner("proto")
    room = _room(cfg)
    far = room[:20].clone()
    far[:, 0] += 5.0                      # 20 points five metres away: their blocks stay below min_points
    bad = room[:3].clone()
    bad[0, 0], bad[1, 1], bad[2, 2] = float("nan"), float("inf"), float("-inf")
    scan = torch.cat([bad[:1], room[:700], far, bad[1:], room[700:]])
    out = torch.zeros(scan.shape[0], dtype=torch.bool)
    out[0] = out[701:723] = True
    p = RefPlan(scan.numpy(), cfg["pc_npts"], block_size=1.0, stride=0.5, min_points=100)
    want_votes = torch.from_numpy(p.vote(np.zeros((p.n_chunks, 3, p.N), np.float32))[2])
    assert torch.equal(want_votes == 0, out) and (p.block_points[~p.kept] > 0).any()  # invalid points, points of dropped blocks
    res = learner.predict_scene(scan, block_size=1.0, stride=0.5, min_points=100, groups_per_launch=4)
    lab, sc, vo = res.labels.cpu(), res.scores.cpu(), res.votes.cpu()
    assert torch.equal(vo, want_votes)
    assert (lab[out] == -1).all() and (vo[out] == 0).all() and (sc[out] == 0).all()
    assert (lab[~out] >= 0).all() and (lab[~out] <= cfg["n_way"]).all() and (vo[~out] >= 1).all()
    assert res.n_unlabelled == 23 == int((lab == -1).sum()) and (res.n_blocks, res.n_chunks) == (p.n_blocks, p.n_chunks)
    assert int(vo.sum()) == res.n_chunks * cfg["pc_npts"]
    again = learner.predict_scene(scan, block_size=1.0, stride=0.5, min_points=100, groups_per_launch=4)
    dev = learner.predict_scene(scan.cuda(), block_size=1.0, stride=0.5, min_points=100, groups_per_launch=4)
    for other in (again, dev):
        assert torch.equal(other.labels, res.labels) and torch.equal(other.scores, res.scores) and torch.equal(other.votes, res.votes)
        assert (other.n_blocks, other.n_chunks, other.n_unlabelled, other.redone) == (res.n_blocks, res.n_chunks, 23, 0)


# ---- 6. errors on the device path ---------------------------------------------------------------------------------------
def test_errors_on_the_device_path():
    from r3dfsseg_amd.proto_learner import ProtoLearner
    cfg = S.make_cfg(**CASES["proto"][1])
    learner = ProtoLearner(SimpleNamespace(**dict(cfg, model_checkpoint_path="synthetic")), mode="test")
    learner.fit(S.make_episode(cfg, seed=11)[0])
    scan = _room(cfg)
    nowhere = scan.clone()
    nowhere[:, 1] = float("nan")
    with pytest.raises(ValueError, match="no point with finite"):
        learner.predict_scene(nowhere)
    wide = scan[:2].clone()
    wide[1, 0] += 300.0
    wide[1, 1] += 300.0
    with pytest.raises(ValueError, match="at most 65536"):
        learner.predict_scene(wide, min_points=1)
    assert learner.predict_scene(scan, stride=0.5).n_chunks > 0
    with torch.no_grad():
        next(learner.model.parameters()).add_(1e-3)  # one in-place weight update
    with pytest.raises(ValueError, match="stale fit"):
        learner.predict_scene(scan, stride=0.5)


# ---- 7. the bounds alone, both records ------------------------------------------------------------------------------------
BOUNDS_THREADS = 1024 * 256  # the bounds grid: a longer scan sends its threads through their stride loop a second time


def _bounds_scan(M, ld, seed, all_invalid=False):
    """A seeded scan whose extremes and invalid rows are placed: in a scan longer than the grid every extreme lies behind
    BOUNDS_THREADS and invalid rows lie on both sides of it; one invalid row holds values beyond every extreme."""
    rng = np.random.default_rng(seed)
    scan = rng.uniform(-50.0, 50.0, (M, ld)).astype(np.float32)
    lo = BOUNDS_THREADS if M > BOUNDS_THREADS else 0
    if M - lo >= 6:
        at = lo + rng.choice(M - lo, 6, replace=False)
        for a in range(3):
            scan[at[a], a] = -100.0 - a
            scan[at[3 + a], a] = 200.0 + a
    bad = np.zeros(M, bool)
    if all_invalid:
        bad[:] = True
    elif M >= 63:
        free = np.setdiff1d(np.arange(M), at)
        sides = [free[free < lo], free[free >= lo]] if lo else [free]
        for side in sides:
            bad[rng.choice(side, 6, replace=False)] = True
    rows = np.flatnonzero(bad)
    for k, i in enumerate(rows):
        scan[i, k % 3] = (np.nan, np.inf, -np.inf)[k % 3]
    if len(rows):  # values that would move every other extreme, in a row that does not count
        scan[rows[0], 1:3] = (-1e6, 1e6)
        scan[rows[1], 0] = 1e6
    return scan


@pytest.mark.parametrize("M,ld,all_invalid", [(M, ld, False) for M in (1, 63, 257, BOUNDS_THREADS + 300) for ld in (3, 6)] +
                         [(63, 3, True)])
def test_bounds_of_both_records(M, ld, all_invalid):
    """r3d_scene_bounds (xy) and r3d_scene_grow_bounds (xyz) against numpy's minima, maxima and count over the valid rows:
    minima and maxima are exact and the count is an integer, so values are compared with == and nothing has a tolerance."""
    from r3dfsseg_amd import ops
    scan = _bounds_scan(M, ld, seed=1000 + M + ld, all_invalid=all_invalid)
    valid = np.isfinite(scan[:, :3]).all(axis=1)
    n = int(valid.sum())
    assert n == (0 if all_invalid else M - (12 if M > BOUNDS_THREADS else 6 if M >= 63 else 0))
    mn = scan[valid, :3].min(axis=0) if n else np.full(3, np.inf, np.float32)
    mx = scan[valid, :3].max(axis=0) if n else np.full(3, -np.inf, np.float32)
    if M > BOUNDS_THREADS:  # what the second trip has to find, and to skip
        assert (~valid[:BOUNDS_THREADS]).sum() == 6 and (~valid[BOUNDS_THREADS:]).sum() == 6
        for a in range(3):
            col = np.where(valid, scan[:, a], np.nan)
            assert np.nanargmin(col) >= BOUNDS_THREADS and np.nanargmax(col) >= BOUNDS_THREADS
    dev = torch.from_numpy(scan).cuda()
    rec = ops.scene_bounds(dev).cpu()
    assert rec[:4].numpy().tolist() == [mn[0], mn[1], mx[0], mx[1]]
    assert rec.view(torch.int32)[4:].tolist() == [n, 0, 0, 0]
    ws = ops.scene_grow_workspace(M, "cuda")
    ops.scene_grow_bounds(dev, ws)
    rec = ws[:16].cpu()
    assert rec[:6].view(torch.float32).numpy().tolist() == mn.tolist() + mx.tolist()
    assert rec[6:].tolist() == [n] + [0] * 9
