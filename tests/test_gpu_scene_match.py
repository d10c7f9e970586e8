"""match_objects on the device (r3dfsseg_amd/scene_match.py, csrc/scene_match.hip) against the numpy restatement
tests/scene_match_ref.py (which tests/test_scene_match_host.py checks against a dense count and hand-worked numbers).

Every comparison is on integers, bit for bit on pair_iou and on the float64 of the summary: the definition (INTEGRATION.md,
"Matching objects against ground truth") fixes every operation and its order, so no tolerance is used in this file."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import scene_match_cases as MC  # noqa: E402
import scene_match_ref as MR  # noqa: E402

from r3dfsseg_amd import fitted, ops, scene_match as SM, scene_objects as SO  # noqa: E402

pytestmark = pytest.mark.gpu

TABLES = (("pred_ids", np.int64), ("pred_points", np.int32), ("pred_index", np.int32), ("pred_best", np.int32),
          ("truth_ids", np.int64), ("truth_points", np.int32), ("truth_index", np.int32), ("truth_best", np.int32),
          ("pair_pred", np.int32), ("pair_truth", np.int32), ("pair_points", np.int32), ("pair_match", np.uint8))
CLASS_TABLES = ("pred_classes", "truth_classes")
COUNTS = ("n_pred", "n_truth", "n_pairs", "n_pred_unassigned", "n_truth_unassigned", "n_ignored", "n_mixed_pred", "n_mixed_truth")
_cache = {}


def _cached(key, build):
    if key not in _cache:
        _cache[key] = build()
    return _cache[key]


def _case(name):
    return _cached(("case", name), MC.CASES[name])


def _want(name):
    """The restatement of a named case, computed once."""
    return _cached(("ref", name), lambda: MR.match(**_case(name)))


def _same(got, want):
    """Every field of an ObjectMatch against the restatement's dict."""
    for name, dtype in TABLES:
        a = getattr(got, name).cpu().numpy()
        assert a.dtype == want[name].dtype == dtype and np.array_equal(a, want[name]), name
    for name in CLASS_TABLES:
        if want[name] is None:
            assert getattr(got, name) is None
        else:
            a = getattr(got, name).cpu().numpy()
            assert a.dtype == np.int64 and np.array_equal(a, want[name]), name
    assert {k: getattr(got, k) for k in COUNTS} == {k: want[k] for k in COUNTS}
    a = got.pair_iou.cpu().numpy()
    assert a.dtype == np.float32 and np.array_equal(a.view(np.uint32), want["pair_iou"].view(np.uint32))
    assert got.iou == want["iou"] and MR.same_summary(got.summary, want["summary"])


def _as(case, width, device):
    """The case's columns in one id width (labels in the other), on the host or on the device."""
    other = {np.int32: np.int64, np.int64: np.int32}[width]
    out = dict(case)
    for k, dt in (("pred", width), ("truth", width), ("pred_labels", other), ("truth_labels", other)):
        if k in out:
            out[k] = torch.from_numpy(out[k].astype(dt)).cuda() if device else out[k].astype(dt)
    return out


# ---- 1. every case against the restatement ------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("width", [np.int32, np.int64], ids=["int32", "int64"])
@pytest.mark.parametrize("name", sorted(MC.CASES))
def test_every_case_equals_the_restatement(name, width, device):
    got = SM.match_objects(**_as(_case(name), width, device))
    _same(got, _want(name))
    if name == "identity":
        assert got.n_pairs == 9 and (got.pair_iou == 1).all() and int(got.pred_ids[-1]) == 2 ** 31 - 2
    if name == "singletons":
        assert got.n_pairs == 4097
    if name == "fan":
        assert int(got.pred_best[MC.FAN_BEFORE]) == MC.FAN_BEFORE + 204
    if name in ("split", "merge"):
        assert [got.summary[t]["all"]["tp"] for t in (0.25, 0.5, 0.75)] == [1, 1, 0]


def test_columns_of_different_widths():
    case = _case("labelled-random")
    mixed = dict(case, pred=torch.from_numpy(case["pred"].astype(np.int32)).cuda(), truth=case["truth"],
                 pred_labels=case["pred_labels"], truth_labels=torch.from_numpy(case["truth_labels"].astype(np.int32)))
    _same(SM.match_objects(**mixed), _want("labelled-random"))


# ---- 2. promises ----------------------------------------------------------------------------------------------------------------
def _fields(got):
    return ([getattr(got, k).cpu().numpy() for k, _ in TABLES] + [got.pair_iou.cpu().numpy().view(np.uint32)] +
            [[getattr(got, k) for k in COUNTS]])


@pytest.mark.parametrize("name", ["fan-mirror", "labelled-random", "negatives-ignored"])
def test_two_calls_give_the_same_bits(name):
    args = _as(_case(name), np.int64, True)
    a, b = SM.match_objects(**args), SM.match_objects(**args)
    assert all(np.array_equal(x, y) for x, y in zip(_fields(a), _fields(b))) and MR.same_summary(a.summary, b.summary)


def test_ids_that_are_too_large_raise_after_the_first_read(monkeypatch):
    launched = []
    for name in ("scene_match_rows", "scene_match_pairs", "scene_match_best"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, **k: launched.append(_n))
    reads = []
    read = SM.read_record
    monkeypatch.setattr(SM, "read_record", lambda ws: reads.append(1) or read(ws))
    case = _case("split")
    pred = case["pred"].copy()
    pred[:3] = (2 ** 31 - 1, 2 ** 40, 2 ** 31 - 1)
    truth = case["truth"].copy()
    truth[7] = 2 ** 33
    with pytest.raises(ValueError, match=r"match_objects: 4 object ids are 2\^31 - 1 or more \(the largest: %d\)" % 2 ** 40):
        SM.match_objects(pred, truth)
    with pytest.raises(ValueError, match=r"match_objects: 1 object ids .*largest: 2147483647"):
        SM.match_objects(case["pred"].astype(np.int32), np.where(np.arange(300) == 5, 2 ** 31 - 1, case["truth"]).astype(np.int32),
                         ignore_unannotated=True)
    assert launched == [] and len(reads) == 2
    monkeypatch.undo()
    pred[:3] = 2 ** 31 - 2  # the largest legal id
    truth[7] = 7
    assert SM.match_objects(pred, truth).pred_ids.tolist() == [3, 9, 2 ** 31 - 2]


def test_a_call_reads_the_host_four_times(monkeypatch):
    reads = []
    read, tables = SM.read_record, SM.read_tables
    monkeypatch.setattr(SM, "read_record", lambda ws: reads.append("record") or read(ws))
    monkeypatch.setattr(SM, "read_tables", lambda *a: reads.append("tables") or tables(*a))
    SM.match_objects(**_case("classes"))
    assert reads == ["record", "record", "record", "tables"]
    del reads[:]
    SM.match_objects(**_case("pred-all-negative"))  # nothing behind the id pass
    assert reads == ["record"]


# ---- 3. composition -------------------------------------------------------------------------------------------------------------
def test_the_room_through_the_learner():
    """What a user runs: objects from the true labels and from labels with a band of points flipped, both by extract_objects,
    matched per class through FittedLearner.match_objects."""
    scan, labels, flipped, voxel = _cached("room", MC.room_inputs)
    assert 500 < int((flipped != labels).sum()) < len(scan) // 2
    truth = SO.extract_objects(scan, labels, voxel=voxel, connectivity=26, min_points=4)
    pred = SO.extract_objects(scan, flipped, voxel=voxel, connectivity=26, min_points=4)
    learner = fitted.FittedLearner.__new__(fitted.FittedLearner)  # the forward needs no model
    got = learner.match_objects(pred.objects, truth.objects, torch.from_numpy(flipped), torch.from_numpy(labels), iou=(0.25, 0.5))
    want = MR.match(pred.objects.cpu().numpy(), truth.objects.cpu().numpy(), flipped, labels, iou=(0.25, 0.5))
    _same(got, want)
    assert got.n_pred == pred.n_objects and got.n_truth == truth.n_objects and torch.equal(got.pred_points, pred.object_points)
    assert torch.equal(got.pred_classes, pred.object_labels) and got.n_mixed_pred == got.n_mixed_truth == 0
    assert got.n_pairs > got.n_truth and list(got.summary[0.5]) == ["all", 0, 1, 2]
    assert got.n_pred > got.n_truth and got.summary[0.5]["all"]["fp"] > 0  # the band cuts objects in two
    assert 0 < got.summary[0.5]["all"]["tp"] <= got.n_truth and 0.0 < got.summary[0.25]["all"]["pq"] < 1.0
    whole = learner.match_objects(truth.objects, truth.objects, torch.from_numpy(labels), torch.from_numpy(labels))
    assert whole.summary[0.75]["all"] == {"tp": truth.n_objects, "fp": 0, "fn": 0, "precision": 1.0, "recall": 1.0, "f1": 1.0,
                                          "sq": 1.0, "pq": 1.0}
