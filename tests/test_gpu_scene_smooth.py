"""smooth_scene on the device (r3dfsseg_amd/scene_smooth.py, csrc/scene_smooth.hip) against the numpy restatement
tests/scene_smooth_ref.py (which tests/test_scene_smooth_host.py checks against float64 and against numbers worked by hand).

Integers are compared as equal, floats bit for bit where finite and NaN where NaN, host ints and the grid as equal: the
definition ("Smoothing a labelled scan") fixes every operation and its order, so no tolerance is used in
this file."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import scene_segments_ref  # noqa: E402
import scene_smooth_cases as C  # noqa: E402
import scene_smooth_ref as R  # noqa: E402

from r3dfsseg_amd import scene, scene_grow, scene_match, scene_objects, scene_segments, scene_smooth as S  # noqa: E402

pytestmark = pytest.mark.gpu

f32 = np.float32
FLOATS = ("scores", "voxel_scores", "voxel_evidence")
INTS = (("labels", np.int64), ("votes", np.int32), ("source_votes", np.int32), ("smoothed", np.bool_), ("voxel_index", np.int32),
        ("voxel_labels", np.int64), ("voxel_members", np.int32), ("voxel_ring", np.int32))
COUNTS = ("n_voxels", "n_member_voxels", "n_filled_voxels", "n_smoothed", "n_changed", "n_filled", "n_unlabelled", "n_invalid")
_cache = {}


def _cached(key, build):
    if key not in _cache:
        _cache[key] = build()
    return _cache[key]


def _result(case, device="cuda"):
    return scene.SceneResult(labels=torch.from_numpy(case["labels"]).to(device), scores=torch.from_numpy(case["scores"]).to(device),
                             votes=torch.from_numpy(case["votes"]).to(device), n_blocks=3, n_chunks=7,
                             n_unlabelled=int((case["labels"] == -1).sum()), redone=0)


def _same_bits(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype == f32, what
    nan = np.isnan(b)
    assert np.array_equal(np.isnan(a), nan), what
    assert np.array_equal(a[~nan].view(np.uint32), b[~nan].view(np.uint32)), what


def _same(got, want):
    """Every field of a SmoothResult against the restatement's dict."""
    for name in FLOATS:
        _same_bits(getattr(got, name).cpu().numpy(), want[name], name)
    for name, dtype in INTS:
        a = getattr(got, name).cpu().numpy()
        assert a.dtype == dtype == want[name].dtype and np.array_equal(a, want[name]), name
    assert {k: getattr(got, k) for k in COUNTS} == {k: want[k] for k in COUNTS}
    assert got.grid == want["grid"]
    if want.get("voxel_means") is None:
        assert got.voxel_means is None
    else:
        _same_bits(got.voxel_means.cpu().numpy(), want["voxel_means"], "voxel_means")


def _check(name, case, **kw):
    """One call against the restatement of a named case (computed once per set of arguments); res is as it was."""
    want = _cached(("ref", name) + tuple(sorted(kw.items())),
                   lambda: R.smooth(case["scan"], case["scores"], case["votes"], case["labels"], voxel=C.VOX, **kw))
    res = _result(case)
    before = [t.clone() for t in (res.scores, res.votes, res.labels)]
    got = S.smooth_scene(res, case["scan"], voxel=C.VOX, **kw)
    _same(got, want)
    for t, clone in zip((res.scores, res.votes, res.labels), before):
        assert torch.equal(t.view(torch.uint8), clone.view(torch.uint8))
    assert got.source_votes is res.votes and (got.n_blocks, got.n_chunks, got.redone) == (3, 7, 0) and got.source is None
    return got, want


# ---- 1. the evidence ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iterations", [0, 3])
def test_voxels_of_1_256_257_and_513_contributors(iterations):
    """Contributor ranks, not points, are cut into tiles of 256: every voxel holds as many voteless points again, and column
    0 cancels so that any other order or tiling gives another sum."""
    case = _cached("contributors", C.contributors_case)
    got, want = _check("contributors", case, iterations=iterations)
    assert got.voxel_members.tolist() == list(C.CONTRIBUTORS) and got.n_voxels == 4
    assert np.array_equal(got.voxel_evidence.cpu().numpy()[:, 0].view(np.uint32), case["Y0"].view(np.uint32))
    assert torch.equal(got.voxel_scores, got.voxel_evidence) and got.voxel_scores.data_ptr() != got.voxel_evidence.data_ptr()
    assert got.votes.tolist() == [1] * len(case["scan"]) and got.smoothed.all()  # the voteless points of a voted voxel too


# ---- 2. V and C at the edges of a wave and a workgroup ------------------------------------------------------------------------
@pytest.mark.parametrize("V,Cn,connectivity", [(1, 2, 26), (63, 3, 6), (64, 5, 26), (65, 64, 6), (257, 3, 26), (257, 64, 26), (64, 64, 6)])
def test_voxel_and_column_counts_at_the_edges(V, Cn, connectivity):
    case = _cached(("strip", V, Cn), lambda: C.strip_case(V, Cn))
    got, want = _check(("strip", V, Cn), case, connectivity=connectivity, iterations=3, alpha=0.75)
    assert got.n_voxels == V and got.scores.shape == (len(case["scan"]), Cn)
    if V > 1:
        assert got.n_filled_voxels > 0 and got.n_invalid > 0 and got.n_member_voxels + got.n_filled_voxels == V
        invalid = ~np.isfinite(case["scan"]).all(1)
        assert not got.smoothed.cpu().numpy()[invalid].any() and (got.voxel_index.cpu().numpy()[invalid] == -1).all()
        assert np.array_equal(got.scores.cpu().numpy()[invalid].view(np.uint32), case["scores"][invalid].view(np.uint32))


# ---- 3. rings -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("iterations", [2, 4])
def test_a_chain_of_voteless_voxels_is_filled_one_ring_a_sweep(iterations, connectivity):
    case = _cached("chain", C.chain_case)
    got, want = _check("chain", case, connectivity=connectivity, iterations=iterations)
    reached = [0, 1, 2, 3, 4][:iterations + 1]
    assert got.voxel_ring.tolist() == reached + [-1] * (5 - len(reached)) + [0, -1]  # (8, 0, 0) voted, (8, 3, 0) never reached
    assert got.voxel_labels.tolist()[-1] == -1 and got.labels.tolist()[-1] == -1 and got.n_unlabelled == 1
    if iterations == 2:  # the points of the two voxels out of reach keep the bits of res
        assert got.votes.tolist()[4:6] == [0, 0] and got.labels.tolist()[4:6] == [1, 1]
        assert np.array_equal(got.scores.cpu().numpy()[4:6].view(np.uint32), case["scores"][4:6].view(np.uint32))
    assert got.voxel_scores[5].tolist() == got.voxel_evidence[5].tolist() == [-0.5, 4.0]  # isolated: no neighbour, Z stays Y


def test_a_negative_zero_from_the_only_live_neighbour_stays_negative():
    got, want = _check("negative zero", C.negative_zero_case(), iterations=1)
    assert np.array_equal(got.voxel_scores.cpu().numpy().view(np.uint32), np.array([[-0.0, 0.0]] * 2, f32).view(np.uint32))


def test_an_inf_and_a_nan_logit_spread_as_ieee_says():
    case = _cached("nonfinite", C.nonfinite_case)
    got, want = _check("nonfinite", case, iterations=2)
    z = got.voxel_scores.cpu().numpy()
    assert np.isnan(z[:, 1]).all() and np.isinf(z[:, 0]).all() and np.isfinite(z[:, 2]).all()  # 3 x 3: all within two sweeps


# ---- 4. alpha 0, no sweep, both connectivities, colours, invalid points, receivers --------------------------------------------
@pytest.mark.parametrize("kw", [dict(iterations=0), dict(alpha=0.0, iterations=5), dict(connectivity=6), dict(connectivity=26),
                                dict(connectivity=26, colour_tol=0.25), dict(connectivity=6, colour_tol=0.0, iterations=64, alpha=0.5)],
                         ids=["no sweep", "alpha 0", "6", "26", "26 colour", "6 colour 64 sweeps"])
def test_random_occupancy(kw):
    case = _cached("random", lambda: C.random_case(21))
    got, want = _check("random", case, **kw)
    receivers = (case["votes"] == 0) & (case["labels"] >= 0)
    assert got.n_voxels > 300 and got.n_invalid > 0 and receivers.sum() > 50 and got.n_changed > 0
    if kw.get("alpha") == 0.0:  # the evidence stays, voteless voxels are still filled
        member = got.voxel_ring == 0
        assert torch.equal(got.voxel_scores[member], got.voxel_evidence[member]) and got.n_filled_voxels > 0
    if kw.get("iterations") == 0:
        assert got.n_filled_voxels == 0 and torch.equal(got.voxel_scores, got.voxel_evidence)


def test_more_points_than_one_round_of_the_spread_kernel():
    """The spread kernel runs at most 1024 workgroups of 256 points a round: 290 664 points take a second round of some."""
    case = _cached("many", C.many_points_case)
    assert len(case["scan"]) > 1024 * 256
    got, want = _check("many", case, iterations=2)
    assert got.n_smoothed + got.n_invalid == len(case["scan"]) and got.voxel_members.max() > 512


@pytest.mark.parametrize("connectivity", [6, 26])
def test_consecutive_keys_across_a_row_or_a_slab_are_no_neighbours(connectivity):
    case = _cached("wrap", C.wrap_case)
    got, want = _check("wrap", case, connectivity=connectivity, iterations=2)
    assert got.grid == C.GC.WRAP_GRID and got.n_voxels == 7
    z, y = got.voxel_scores.cpu().numpy(), got.voxel_evidence.cpu().numpy()
    vi = got.voxel_index.cpu().numpy()
    row = lambda v: vi[np.flatnonzero((case["coords"] == v).all(1))[0]]
    for a, b in C.GC.WRAP_PAIRS[:2]:  # no neighbour at all: the row stays the evidence
        assert np.array_equal(z[row(a)], y[row(a)]) and np.array_equal(z[row(b)], y[row(b)])
    assert not np.array_equal(z[row(C.GC.WRAP_CORNER)], y[row(C.GC.WRAP_CORNER)])  # (4, 3, 1) below the corner is one


def test_the_colour_gate_between_two_slabs_and_a_nan_colour():
    case = _cached("slabs", C.slabs_case)
    free, _ = _check("slabs", case, iterations=10)
    gated, _ = _check("slabs", case, iterations=10, colour_tol=C.COLOUR_TOL)
    vi = gated.voxel_index.cpu().numpy()
    upper = np.unique(vi[case["coords"][:, 2] == 1])
    nan_row = vi[np.flatnonzero((case["coords"] == case["nan_voxel"]).all(1))[0]]
    assert torch.isnan(gated.voxel_means[nan_row]).any() and free.voxel_means is None
    assert torch.equal(gated.voxel_scores[nan_row], gated.voxel_evidence[nan_row])  # it joined nothing
    assert not torch.equal(free.voxel_scores[nan_row], free.voxel_evidence[nan_row])
    zg, zf = gated.voxel_scores.cpu().numpy()[upper], free.voxel_scores.cpu().numpy()[upper]
    assert (zg[:, 1] > zf[:, 1]).all()  # without the gate the lower slab's logits leak into the upper one


def test_a_scan_without_a_valid_point():
    case = C.chain_case()
    scan = case["scan"].copy()
    scan[:, 1] = np.nan
    res = _result(case)
    got = S.smooth_scene(res, scan, voxel=C.VOX)
    _same(got, R.smooth(scan, case["scores"], case["votes"], case["labels"], voxel=C.VOX))
    assert got.grid == (0, 0, 0) and got.n_voxels == 0 and got.n_invalid == len(scan) and got.voxel_scores.shape == (0, 2)
    assert got.scores.data_ptr() != res.scores.data_ptr()


# ---- 5. the same bits ---------------------------------------------------------------------------------------------------------
def test_two_calls_and_a_host_or_a_device_scan_give_the_same_bits():
    case = _cached("random", lambda: C.random_case(21))
    res = _result(case)
    kw = dict(voxel=C.VOX, connectivity=26, iterations=6, colour_tol=0.25)
    a = S.smooth_scene(res, case["scan"], **kw)
    b = S.smooth_scene(res, case["scan"], **kw)
    c = S.smooth_scene(res, torch.from_numpy(case["scan"]).cuda(), **kw)
    d = S.smooth_scene(res, torch.from_numpy(case["scan"]), **kw)
    for other in (b, c, d):
        for name in FLOATS + tuple(n for n, _ in INTS) + ("voxel_means",):
            x, y = getattr(a, name), getattr(other, name)
            assert x.dtype == y.dtype and torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)), name
        assert [getattr(a, k) for k in COUNTS] == [getattr(other, k) for k in COUNTS] and a.grid == other.grid


# ---- 6. the calls beside it ---------------------------------------------------------------------------------------------------
def test_the_grid_and_the_voxels_are_those_of_build_segments():
    case = _cached("random", lambda: C.random_case(21))
    sm = S.smooth_scene(_result(case), case["scan"], voxel=C.VOX, colour_tol=0.25)
    grown = scene_grow.build_segments(case["scan"], voxel=C.VOX, colour_tol=0.25, connectivity=26)
    assert sm.grid == grown.grid and sm.n_voxels == grown.n_voxels and sm.n_invalid == grown.n_invalid
    assert torch.equal(sm.voxel_index, grown.voxel_index)
    assert torch.equal(sm.voxel_means.view(torch.int32), grown.voxel_means.view(torch.int32))


def test_pool_segments_takes_the_result_as_it_is():
    case = _cached("random", lambda: C.random_case(21))
    sm = S.smooth_scene(_result(case), case["scan"], voxel=C.VOX, iterations=2)
    seg = (case["coords"][:, 0] // 2 * 64 + case["coords"][:, 1] // 3).astype(np.int64)
    seg[::17] = -1
    got = scene_segments.pool_segments(sm, torch.from_numpy(seg))
    want = scene_segments_ref.pool(sm.scores.cpu().numpy(), sm.votes.cpu().numpy(), sm.labels.cpu().numpy(), seg)
    for name in ("scores", "segment_scores"):
        _same_bits(getattr(got, name).cpu().numpy(), want[name], name)
    for name in ("labels", "pooled", "segment_index", "segment_ids", "segment_points", "segment_members", "segment_labels"):
        assert np.array_equal(getattr(got, name).cpu().numpy(), want[name]), name
    assert got.n_segments == want["n_segments"] > 10 and got.n_pooled == want["n_pooled"] > 0 and got.votes is sm.votes


def test_on_the_noisy_room_the_objects_get_fewer_and_better():
    """The room of S7, 15 % of its voxels flipped: every isolated wrong voxel is an object of its own before, and the two
    halves come out nearly whole after."""
    room = _cached("room", lambda: C.room_case(flip=0.15))
    res = _result(room)
    sm = S.smooth_scene(res, room["scan"], voxel=C.VOX)
    scan, truth = torch.from_numpy(room["scan"]).cuda(), torch.from_numpy(room["truth"]).cuda()
    true_objects = scene_objects.extract_objects(scan, truth, voxel=C.VOX)
    assert true_objects.n_objects == 2
    pq = {}
    for name, labels in (("before", res.labels), ("after", sm.labels)):
        objects = scene_objects.extract_objects(scan, labels, voxel=C.VOX)
        match = scene_match.match_objects(objects.objects, true_objects.objects, iou=(0.5,))
        pq[name] = (objects.n_objects, match.summary[0.5]["all"]["pq"])
    print("objects and pq at 0.5: %r" % (pq,))
    assert pq["after"][0] < pq["before"][0] and pq["after"][1] > pq["before"][1]
    assert sm.n_changed > 0 and int((sm.labels.cpu().numpy() != room["truth"]).sum()) < room["wrong"].sum() / 2


# ---- 7. end to end ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap,transfer", [(None, None), (1, "nearest")])
def test_end_to_end_proto(cap, transfer):
    from test_gpu_scene import _learner, _room
    learner, cfg = _learner("proto")
    scan = _room(cfg)
    res = learner.predict_scene(scan, block_size=1.0, stride=0.5, min_points=100, max_chunks_per_block=cap, transfer=transfer)
    got = learner.smooth_scene(res, scan, voxel=0.125, iterations=3)
    assert isinstance(got, S.SmoothResult) and isinstance(got, scene.SceneResult)
    want = R.smooth(scan.numpy(), res.scores.cpu().numpy(), res.votes.cpu().numpy(), res.labels.cpu().numpy(), voxel=0.125,
                    iterations=3)
    _same(got, want)
    assert got.n_voxels > 50 and got.n_smoothed > 0 and got.source is res.source and got.n_chunks == res.n_chunks
    if transfer:  # receivers take part as receivers: they have no vote and are smoothed all the same
        assert res.n_transferred > 0 and got.smoothed[res.votes == 0].any()
    objects = learner.extract_objects(scan, got.labels)
    assert objects.n_objects >= 1
