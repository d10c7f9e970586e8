"""match_objects ("Matching objects against ground truth", M1-M8), without a device: the numpy restatement
tests/scene_match_ref.py against a brute-force dense P x T count and against hand-worked numbers, every ValueError of the
argument check, and the C ABI."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import scene_match_cases as MC  # noqa: E402
import scene_match_ref as MR  # noqa: E402

from r3dfsseg_amd import _lib, fitted, ops, scene_match as SM  # noqa: E402

f32 = np.float32
ENTRY_POINTS = ("ids", "rows", "pairs", "best")


# ---- the restatement against a dense count -----------------------------------------------------------------------------------
def _dense(pred, truth, pred_labels, truth_labels, iou, ignore):
    """M1-M7 from a dense P x T table of intersections, row by row."""
    pred, truth = pred.copy(), truth.copy()
    if ignore:
        pred[truth < 0] = -1
    pid, tid = np.unique(pred[pred >= 0]), np.unique(truth[truth >= 0])
    P, T = len(pid), len(tid)
    n = np.zeros((P, T), np.int64)
    for a, b in zip(pred, truth):
        if a >= 0 and b >= 0:
            n[np.searchsorted(pid, a), np.searchsorted(tid, b)] += 1
    live = np.ones(len(pred), bool) if not ignore else truth >= 0
    pp = np.array([(live & (pred == v)).sum() for v in pid])
    tp = np.array([(live & (truth == v)).sum() for v in tid])
    first = lambda col, v, lab: lab[np.flatnonzero(live & (col == v))[0]]
    pc = None if pred_labels is None else np.array([first(pred, v, pred_labels) for v in pid])
    tc = None if pred_labels is None else np.array([first(truth, v, truth_labels) for v in tid])
    pairs = [(p, t) for p in range(P) for t in range(T) if n[p, t] > 0]
    val = {(p, t): f32(n[p, t]) / f32(pp[p] + tp[t] - n[p, t]) for p, t in pairs}
    ok = {k: pc is None or pc[k[0]] == tc[k[1]] for k in pairs}
    pred_best, truth_best = [-1] * P, [-1] * T
    for p in range(P):
        cand = [(-val[(p, t)], t) for t in range(T) if (p, t) in val and ok[(p, t)]]
        if cand:
            pred_best[p] = pairs.index((p, min(cand)[1]))
    for t in range(T):
        cand = [(-val[(p, t)], p) for p in range(P) if (p, t) in val and ok[(p, t)]]
        if cand:
            truth_best[t] = pairs.index((min(cand)[1], t))
    th = np.sort(np.asarray(iou, f32))
    match = [int((val[k] >= th).sum()) if pred_best[k[0]] == i == truth_best[k[1]] else 0 for i, k in enumerate(pairs)]
    return dict(pred_ids=pid, truth_ids=tid, pred_points=pp, truth_points=tp, pred_classes=pc, truth_classes=tc,
                pair_pred=[k[0] for k in pairs], pair_truth=[k[1] for k in pairs], pair_points=[n[k] for k in pairs],
                pair_iou=np.array([val[k] for k in pairs], f32), pred_best=pred_best, truth_best=truth_best, pair_match=match)


@pytest.mark.parametrize("labelled", [False, True])
@pytest.mark.parametrize("ignore", [False, True])
@pytest.mark.parametrize("seed", range(6))
def test_the_restatement_equals_a_dense_count(seed, ignore, labelled):
    rs = np.random.RandomState(seed)
    M = int(rs.randint(20, 400))
    pred, truth = rs.randint(-2, 9, M).astype(np.int64) * 17, rs.randint(-1, 7, M).astype(np.int64) * 1000003
    pl = rs.randint(0, 3, M).astype(np.int64)[np.maximum(pred // 17, 0)] if labelled else None  # a class per id ...
    tl = rs.randint(0, 3, M).astype(np.int64)[np.maximum(truth // 1000003, 0)] if labelled else None
    if labelled:
        pl[rs.rand(M) < 0.02] = 5  # ... and a few points that differ
    iou = (0.1, 0.3, 0.5)
    got, want = MR.match(pred, truth, pl, tl, iou, ignore), _dense(pred, truth, pl, tl, iou, ignore)
    for k, v in want.items():
        if v is None:
            assert got[k] is None
        elif k == "pair_iou":
            assert np.array_equal(got[k].view(np.uint32), v.view(np.uint32))
        else:
            assert np.array_equal(got[k], np.asarray(v)), k
    assert got["n_pairs"] == len(want["pair_iou"]) > 3 and got["n_pred"] == len(want["pred_ids"])
    live = truth >= 0 if ignore else np.ones(M, bool)
    assert got["n_ignored"] == int((~live).sum()) and got["n_pred_unassigned"] == int((live & (pred < 0)).sum())
    assert got["n_truth_unassigned"] == int((live & (truth < 0)).sum())
    assert np.array_equal(got["pred_ids"][got["pred_index"][live & (pred >= 0)]], pred[live & (pred >= 0)])
    assert (got["pred_index"][~(live & (pred >= 0))] == -1).all()
    assert np.array_equal(got["truth_ids"][got["truth_index"][truth >= 0]], truth[truth >= 0])
    if labelled:
        mixed = sum(len(set(pl[live & (pred == v)].tolist())) > 1 for v in want["pred_ids"])
        assert got["n_mixed_pred"] == mixed and got["n_mixed_truth"] == 0


# ---- hand-worked numbers ---------------------------------------------------------------------------------------------------------
def _lists(got, *names):
    return [got[n].tolist() for n in names]


def _bits(v):
    return np.asarray(v, f32).view(np.uint32).tolist()


def test_split_and_merge_by_hand():
    two_thirds, one_third = f32(200) / f32(300), f32(100) / f32(300)
    s = MR.match(**MC.split_case())
    assert _lists(s, "pred_ids", "pred_points", "truth_ids", "truth_points") == [[3, 9], [200, 100], [7], [300]]
    assert _lists(s, "pair_pred", "pair_truth", "pair_points") == [[0, 1], [0, 0], [200, 100]]
    assert _bits(s["pair_iou"]) == _bits([two_thirds, one_third])
    assert _lists(s, "pred_best", "truth_best", "pair_match") == [[0, 1], [0], [2, 0]]
    m = MR.match(**MC.merge_case())
    assert _lists(m, "pair_pred", "pair_truth", "pair_points") == [[0, 0], [0, 1], [200, 100]]
    assert _lists(m, "pred_best", "truth_best", "pair_match") == [[0], [0, 1], [2, 0]] and _bits(m["pair_iou"]) == _bits(s["pair_iou"])
    for got, (fp, fn) in ((s, (1, 0)), (m, (0, 1))):
        for tau in (0.25, 0.5):
            a = got["summary"][tau]["all"]
            assert (a["tp"], a["fp"], a["fn"]) == (1, fp, fn) and a["sq"] == float(two_thirds) and a["pq"] == float(two_thirds) / 1.5
            assert a["precision"] == 1 / (1 + fp) and a["recall"] == 1 / (1 + fn) and a["f1"] == 2 / 3
        a = got["summary"][0.75]["all"]
        assert (a["tp"], a["fp"], a["fn"]) == (0, 1 + fp, 1 + fn) and math.isnan(a["sq"]) and a["pq"] == 0.0
        assert a["precision"] == a["recall"] == a["f1"] == 0.0 and list(got["summary"][0.5]) == ["all"]


def test_tie_by_hand():
    t = MR.match(**MC.tie_case())
    assert _lists(t, "pred_ids", "truth_ids", "truth_points") == [[4], [10, 20], [5, 5]]
    assert _lists(t, "pair_pred", "pair_truth", "pair_points") == [[0, 0], [0, 1], [2, 2]]
    assert _bits(t["pair_iou"]) == _bits([f32(2) / f32(7)] * 2)
    assert _lists(t, "pred_best", "truth_best", "pair_match") == [[0], [0, 1], [1, 0]]  # the lowest truth row wins
    assert (t["n_pred_unassigned"], t["n_truth_unassigned"]) == (6, 0)
    m = MR.match(**MC.tie_mirror_case())
    assert _lists(m, "pair_pred", "pair_truth") == [[0, 1], [0, 0]]
    assert _lists(m, "pred_best", "truth_best", "pair_match") == [[0, 1], [0], [1, 0]]  # the lowest pred row wins


def test_classes_by_hand():
    c = MR.match(**MC.classes_case())
    assert _lists(c, "pred_ids", "pred_points", "pred_classes") == [[1, 2, 3], [10, 8, 6], [4, 9, 2]]
    assert _lists(c, "truth_ids", "truth_points", "truth_classes") == [[50, 60, 70, 80], [14, 7, 5, 6], [9, 4, 4, 2]]
    assert _lists(c, "pair_pred", "pair_truth", "pair_points") == [[0, 0, 1, 2], [0, 1, 0, 3], [6, 3, 8, 6]]
    assert _bits(c["pair_iou"]) == _bits([f32(6) / f32(18), f32(3) / f32(14), f32(8) / f32(14), f32(1)])
    # pair 0 has the greatest IoU of pred 0 and unequal classes: pair 1 is its best
    assert _lists(c, "pred_best", "truth_best", "pair_match") == [[1, 2, 3], [2, 1, -1, 3], [0, 0, 2, 3]]
    assert (c["n_mixed_pred"], c["n_mixed_truth"]) == (1, 1)
    s = c["summary"][0.5]
    assert list(s) == ["all", 2, 4, 9]
    assert [(s[k]["tp"], s[k]["fp"], s[k]["fn"]) for k in s] == [(2, 1, 2), (1, 0, 0), (0, 1, 2), (1, 0, 0)]
    assert s["all"]["sq"] == (float(f32(8) / f32(14)) + 1.0) / 2 and s["all"]["pq"] == (float(f32(8) / f32(14)) + 1.0) / 3.5
    assert math.isnan(s[4]["sq"]) and s[4]["pq"] == 0.0 and s[2]["pq"] == 1.0
    assert c["summary"][0.75]["all"]["tp"] == 1 and c["summary"][0.25][9]["tp"] == 1


def test_the_cases_hold_what_they_are_meant_to():
    ident = MR.match(**MC.identity_case())
    assert ident["n_pred"] == ident["n_truth"] == ident["n_pairs"] == 9 and ident["pred_ids"][-1] == 2 ** 31 - 2
    assert (ident["pair_iou"] == 1).all() and (ident["pair_match"] == 3).all() and ident["summary"][0.75]["all"]["pq"] == 1.0
    single = MR.match(**MC.singletons_case())
    assert single["n_pairs"] == single["n_pred"] == 4097 and (single["pair_match"] == 3).all()
    assert not np.array_equal(single["pair_truth"], np.arange(4097))
    fan = MR.match(**MC.fan_case())
    run = np.flatnonzero(fan["pair_pred"] == MC.FAN_BEFORE)
    assert len(run) == MC.FAN_TRUTHS > 256 and run[0] == MC.FAN_BEFORE < 2048 < run[-1]
    assert fan["pred_best"][MC.FAN_BEFORE] == MC.FAN_BEFORE + 204 > 2048  # the first of three equal maxima
    assert (fan["pair_iou"][run] == fan["pair_iou"][run].max()).sum() == 3
    mirror = MR.match(**MC.fan_mirror_case())
    fan_truth = int(np.argmax(mirror["truth_points"]))
    assert (mirror["pair_truth"] == fan_truth).sum() == MC.FAN_TRUTHS
    assert mirror["pair_pred"][mirror["truth_best"][fan_truth]] == fan["pair_truth"][fan["pred_best"][MC.FAN_BEFORE]]
    for name in ("pred-all-negative", "truth-all-negative", "truth-all-negative-ignored", "both-all-negative"):
        e = MR.match(**MC.CASES[name]())
        assert e["n_pred"] == e["n_truth"] == e["n_pairs"] == 0 and (e["pred_index"] == -1).all() and e["pair_iou"].shape == (0,)
        a = e["summary"][0.5]["all"]
        assert (a["tp"], a["fp"], a["fn"]) == (0, 0, 0) and all(math.isnan(a[k]) for k in ("precision", "recall", "f1", "sq", "pq"))
    assert MR.match(**MC.CASES["truth-all-negative-ignored"]())["n_ignored"] == 3000
    apart = MR.match(**MC.disjoint_case())
    assert (apart["n_pred"], apart["n_truth"], apart["n_pairs"]) == (4, 3, 0) and apart["pred_points"].tolist() == [75] * 4
    assert (apart["pred_best"] == -1).all() and (apart["truth_best"] == -1).all() and apart["pred_classes"].tolist() == [0, 1, 0, 1]
    assert [(v["tp"], v["fp"], v["fn"]) for v in apart["summary"][0.5].values()] == [(0, 4, 3), (0, 2, 2), (0, 2, 1)]
    assert apart["summary"][0.5]["all"]["pq"] == 0.0 and math.isnan(apart["summary"][0.5]["all"]["sq"])
    on, off = MR.match(**MC.negatives_case(True)), MR.match(**MC.negatives_case(False))
    assert on["n_ignored"] == off["n_truth_unassigned"] > 700 and on["n_truth_unassigned"] == 0
    assert on["n_pred_unassigned"] < off["n_pred_unassigned"] and (on["pred_points"] < off["pred_points"]).all()
    assert np.array_equal(on["pair_points"], off["pair_points"]) and (on["pair_iou"] > off["pair_iou"]).all()
    for M in MC.EDGE_SIZES:
        e = MR.match(**MC.edge_case(M))
        assert 1 <= e["n_pred"] <= 7 and 1 <= e["n_truth"] <= 7 and (M < 2047 or (e["n_pred"] == e["n_truth"] == 7))
    lab = MR.match(**MC.labelled_random_case())
    assert lab["n_pairs"] > 100 and 0 < int((lab["pair_match"] > 0).sum()) and list(lab["summary"][0.05]) == ["all", 0, 1, 2]


def test_the_module_s_summary_equals_the_restatement_s():
    """scene_match.summarise (vectorised, np.cumsum) against the loops of the restatement: equal as float64, NaN for NaN."""
    for name in ("classes", "labelled-random", "fan", "split", "both-all-negative", "disjoint"):
        want = MR.match(**MC.CASES[name]())
        got = SM.summarise(want["iou"], want["n_pred"], want["n_truth"], want["pred_classes"], want["truth_classes"],
                           want["pair_pred"], want["pair_iou"], want["pair_match"])
        assert MR.same_summary(got, want["summary"])


# ---- the argument check ------------------------------------------------------------------------------------------------------
def _args(**over):
    a = dict(pred=np.zeros(10, np.int64), truth=np.zeros(10, np.int32))
    a.update(over)
    return a


@pytest.mark.parametrize("over", [
    dict(pred=[0] * 10), dict(pred=None), dict(truth="ids"), dict(pred=np.zeros((10, 1), np.int64)), dict(truth=np.zeros((2, 5), np.int32)),
    dict(pred=np.zeros(10, np.float32)), dict(pred=np.zeros(10, np.int16)), dict(truth=torch.zeros(10, dtype=torch.uint8)),
    dict(truth=torch.zeros(10, dtype=torch.bool)), dict(truth=np.zeros(9, np.int64)), dict(pred=np.zeros(0, np.int64), truth=np.zeros(0, np.int64)),
    dict(pred_labels=np.zeros(10, np.int64)), dict(truth_labels=np.zeros(10, np.int64)),
    dict(pred_labels=np.zeros(10, np.int64), truth_labels=np.zeros(11, np.int64)),
    dict(pred_labels=np.zeros(10, np.float64), truth_labels=np.zeros(10, np.int64)),
    dict(pred_labels=np.zeros(10, np.int64), truth_labels=[0] * 10),
    dict(pred_labels=np.zeros((10, 1), np.int32), truth_labels=np.zeros(10, np.int32)),
    dict(iou=()), dict(iou=(0.0,)), dict(iou=(0.5, 1.5)), dict(iou=(-0.25,)), dict(iou=(float("nan"),)), dict(iou=0.5), dict(iou="0.5"),
    dict(iou=("0.5",)), dict(iou=(True,)), dict(iou=(1e-60,)), dict(iou=tuple([0.5] * 9)), dict(iou=None),
    dict(ignore_unannotated=1), dict(ignore_unannotated=None), dict(ignore_unannotated="yes"),
])
def test_bad_arguments_raise_before_a_device_is_needed(over, monkeypatch):
    launched = []
    for name in ("scene_match_workspace", "scene_match_ids", "scene_match_rows", "scene_match_pairs", "scene_match_best"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: launched.append(_n))
    with pytest.raises(ValueError, match="match_objects"):
        SM.match_objects(**_args(**over))
    learner = fitted.FittedLearner.__new__(fitted.FittedLearner)  # the forward needs no model
    with pytest.raises(ValueError, match="match_objects"):
        learner.match_objects(**_args(**over))
    assert launched == []


def test_good_arguments_pass():
    pred, truth, pl, tl, iou, ignore = SM.check_match_args(**_args(iou=[0.75, 0.25, 1], ignore_unannotated=np.True_))
    assert isinstance(pred, torch.Tensor) and truth.dtype == torch.int32 and pl is None and tl is None
    assert iou == (0.25, 0.75, 1.0) and ignore is True
    out = SM.check_match_args(**_args(pred=torch.zeros(10, dtype=torch.int32), pred_labels=np.zeros(10, np.int32),
                                      truth_labels=torch.zeros(10, dtype=torch.int64), iou=np.array([0.5], f32)))
    assert out[2].dtype == torch.int32 and out[3].dtype == torch.int64 and out[4] == (0.5,) and out[5] is False
    assert SM.check_match_args(**_args(iou=tuple([0.5] * SM.MAX_IOU)))[4] == tuple([0.5] * 8)


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------
def test_the_abi_is_additive():
    assert _lib.ABI_VERSION == 6
    header = open(_lib.HEADER_PATH).read()
    assert "int r3d_abi_version(void); /* 6:" in header and _lib.load().r3d_abi_version() == 6
    names = ["r3d_scene_match_%s" % n for n in ("ws_words",) + ENTRY_POINTS]
    assert set(names) <= set(_lib.header_symbols()) and set(names) <= set(_lib._SIGS)
    assert [n for n in _lib.header_symbols() if n.startswith("r3d_scene_match_")] == sorted(names)
    at = [header.index("int r3d_scene_match_%s(" % n) for n in ENTRY_POINTS]
    assert at == sorted(at) and header.index("int r3d_scene_obj_ids(") < at[0]  # behind extract_objects, in the call's order
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in names)
    assert (ops.MATCH_R_MAX1, ops.MATCH_R_NNEG, ops.MATCH_R_NIGNORED, ops.MATCH_R_NBAD, ops.MATCH_R_BADMAX) == (0, 2, 4, 5, 6)
    assert (ops.MATCH_R_ROWS, ops.MATCH_R_MIXED, ops.MATCH_R_NBOTH, ops.MATCH_R_NPAIRS) == (8, 10, 12, 13)
    assert SM.SUMMARY_FIELDS == MR.FIELDS and ops.SCENE_MATCH_REC == 32 and ops.SCENE_MATCH_IOU == SM.MAX_IOU == 8


def test_the_library_exports_the_new_entry_points_and_refuses_bad_arguments():
    """No device is needed for an argument check: every entry point returns before it launches.  Per entry point a wrong
    workspace size, a wrong id (or label) width and M out of range; the message names the entry point."""
    lib = _lib.load()
    M = 1000
    words = lib.r3d_scene_match_ws_words(M)
    assert words > 32 + 13 * M and lib.r3d_scene_match_ws_words(1) > 32
    assert lib.r3d_scene_match_ws_words(0) == -1 and lib.r3d_scene_match_ws_words(2 ** 27 + 1) == -1
    assert lib.r3d_scene_match_ws_words(2 ** 27) > 13 * 2 ** 27
    one = 1  # a non-null pointer that is never read
    ids = lambda M=M, words=words, pb=8, tb=4: lib.r3d_scene_match_ids(one, pb, one, tb, M, 0, one, words, None)
    rows = lambda M=M, words=words, pb=4, lb=8: lib.r3d_scene_match_rows(one, pb, one, 8, one, lb, one, 4, M, 0, 5, 5, M, M, one, one, one,
                                                                         words, None)
    pairs = lambda M=M, words=words, lb=4: lib.r3d_scene_match_pairs(M, 3, 3, one, one, one, lb, one, 8, one, one, one, one, one, one, one,
                                                                     words, None)
    best = lambda M=M, words=words, n_iou=3: lib.r3d_scene_match_best(M, 3, 3, 5, one, one, None, None, one, n_iou, one, one, one, one, one,
                                                                      one, one, one, one, words, None)
    calls = {"ids": [lambda: ids(words=words - 1), lambda: ids(pb=2), lambda: ids(tb=16), lambda: ids(M=0), lambda: ids(M=2 ** 27 + 1)],
             "rows": [lambda: rows(words=words - 1), lambda: rows(pb=1), lambda: rows(lb=3), lambda: rows(M=0), lambda: rows(M=2 ** 27 + 1)],
             "pairs": [lambda: pairs(words=words - 1), lambda: pairs(lb=0), lambda: pairs(M=-4), lambda: pairs(M=2 ** 27 + 1)],
             "best": [lambda: best(words=words - 1), lambda: best(n_iou=0), lambda: best(n_iou=9), lambda: best(M=0),
                      lambda: best(M=2 ** 27 + 1)]}
    assert sorted(calls) == sorted(ENTRY_POINTS)
    for name, bad in calls.items():
        for call in bad:
            assert call() != 0 and b"r3d_scene_match_%s:" % name.encode() in lib.r3d_last_error_string()
    # more rows or pairs than points, labels for one column only
    assert lib.r3d_scene_match_pairs(M, M + 1, 3, one, one, None, 0, None, 0, one, one, None, one, one, None, one, words, None) != 0
    assert lib.r3d_scene_match_best(M, 3, 3, M + 1, one, one, None, None, one, 3, one, one, one, one, one, one, one, one, one, words, None) != 0
    assert lib.r3d_scene_match_rows(one, 4, one, 4, one, 4, None, 0, M, 0, 5, 5, M, M, one, one, one, words, None) != 0
    assert b"r3d_scene_match_rows" in lib.r3d_last_error_string()
