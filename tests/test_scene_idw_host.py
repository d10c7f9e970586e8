"""Host side of predict_scene's transfer="idw" (r3dfsseg_amd/scene.py): the argument is taken or refused with no device
present, the result keeps its constructor, the new entry point refuses bad arguments before any launch, and the numpy
restatement the GPU tests compare with (tests/scene_idw_ref.py) has the properties step 9' of the definition promises
("Labelling a scan").  Every comparison is np.array_equal: the definition fixes every operation."""
import ctypes
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import scene_idw_ref as IR  # noqa: E402
import scene_sparse_ref as SR  # noqa: E402

from r3dfsseg_amd import _lib, fitted as F, scene, synthetic as S  # noqa: E402
from r3dfsseg_amd.mpti import MPTI_SelfAtten  # noqa: E402
from r3dfsseg_amd.protonet import ProtoNet, ProtoNet_Contrast  # noqa: E402

f32 = np.float32
SMALL = ["small r=1 c=1", "small r=2 c=1", "all inf"]


def _cpu_model(cls):
    return cls(SimpleNamespace(**S.make_cfg(n_way=2, k_shot=1, pc_npts=64))).eval()


@pytest.mark.parametrize("cls", [ProtoNet, ProtoNet_Contrast, MPTI_SelfAtten])
def test_idw_is_accepted_and_its_misspellings_are_refused_before_any_device_work(cls):
    m = _cpu_model(cls)
    f = F.FittedSupport(m, protos=torch.zeros(1, 3, m.feat_dim))
    scan = torch.zeros(100, 6)
    assert scene.check_scene_args(m, scan, 1.0, None, 100, 32, None, "idw")[1] == 1
    assert scene.check_scene_args(m, scan, 1.0, 0.5, 100, 32, 1, "idw")[1] == 2
    scene.check_sparse_args(None, "idw")
    for bad in ("linear", "Nearest", "IDW", "idw3", 1):
        with pytest.raises(ValueError, match="transfer"):
            m.predict_scene(f, scan, transfer=bad)
        with pytest.raises(ValueError, match="transfer"):
            scene.check_sparse_args(None, bad)


def test_the_result_keeps_its_constructor():
    res = scene.SceneResult(1, 2, 3, 4, 5, 6, 7)
    assert res.neighbours is None and res.weights is None and res.source is None
    res = scene.SceneResult(1, 2, 3, 4, 5, 6, 7, 8, 9, 10)  # the positional arguments of before
    assert (res.source, res.n_transferred, res.n_chunks_skipped) == (8, 9, 10) and res.neighbours is None and res.weights is None
    res = scene.SceneResult(1, 2, 3, 4, 5, 6, 7, neighbours="n", weights="w")
    assert (res.neighbours, res.weights) == ("n", "w")
    assert _lib.ABI_VERSION == 6


def _candidates(p, votes, rcv):
    return np.concatenate([[q for q in p.cells[k] if votes[q] > 0] for k in SR.neighbour_cells(p, int(p.key[rcv]))]).astype(np.int64)


@pytest.mark.parametrize("name", SMALL)
def test_properties_of_the_restated_interpolation(name):
    ic = IR.case(name)
    c, p = ic.c, ic.p
    votes, source, nbr, wgt = c.votes, ic.source, ic.neighbours, ic.weights
    M = p.M
    # source and the count are the nearest transfer's on the same votes
    t_scores, t_labels, t_source, t_n = SR.transfer(p, c.scores, c.labels, votes)
    assert np.array_equal(source, t_source) and ic.n_transferred == t_n > 0
    got = (votes == 0) & (source >= 0)
    # voted and invalid rows, and receivers without a candidate, are as the vote left them
    assert np.array_equal(ic.i_scores[~got], c.scores[~got]) and np.array_equal(ic.i_labels[~got], c.labels[~got])
    voted = votes > 0
    assert np.array_equal(nbr[voted], np.stack([np.arange(M)[voted], np.full(voted.sum(), -1), np.full(voted.sum(), -1)], 1))
    assert np.array_equal(wgt[voted], np.tile(np.array([1, 0, 0], f32), (voted.sum(), 1)))
    rest = ~voted & ~got
    assert (nbr[rest] == -1).all() and (wgt[rest] == 0).all() and (~p.valid <= rest).all()
    assert nbr.dtype == np.int64 and wgt.dtype == f32 and ic.i_scores.dtype == f32
    # at a receiver: the first neighbour is the source; missing ones come last, with weight 0
    assert np.array_equal(nbr[got, 0], source[got]) and (votes[nbr[got][nbr[got] >= 0]] > 0).all()
    have = nbr[got] >= 0
    assert (have[:, :-1] >= have[:, 1:]).all() and (wgt[got][~have] == 0).all()
    assert (ic.i_labels[got] >= 0).all() and np.array_equal(ic.i_labels[got], ic.i_scores[got].argmax(1))
    assert ic.n_unlabelled == M - int(voted.sum()) - ic.n_transferred
    # the (d, index) pairs of a receiver are strictly increasing and no other candidate is lexicographically smaller
    for rcv in np.nonzero(got)[0][::3]:
        cand = _candidates(p, votes, rcv)
        n = min(3, len(cand))
        q = nbr[rcv, :n]
        assert (q >= 0).all() and (nbr[rcv, n:] == -1).all() and len(set(q)) == n and np.isin(q, cand).all()
        dq = SR.distance(p.scan, q, rcv)
        pairs = list(zip(dq.tolist(), q.tolist()))
        assert all(a < b for a, b in zip(pairs, pairs[1:]))
        others = np.setdiff1d(cand, q)
        if len(others):
            do = SR.distance(p.scan, others, rcv)
            assert min(zip(do.tolist(), others.tolist())) > pairs[-1]
        assert np.array_equal(wgt[rcv, :n], IR.weights_of(dq))
    # the cell-restricted search equals a search over all voted points filtered by cell distance
    all_voted = np.nonzero(voted)[0]
    cx, cy = p.key % p.ncx, p.key // p.ncx
    for rcv in np.nonzero(got)[0][::5]:
        near = all_voted[(np.abs(cx[all_voted] - cx[rcv]) <= 1) & (np.abs(cy[all_voted] - cy[rcv]) <= 1)]
        d = SR.distance(p.scan, near, rcv)
        o = np.lexsort((near, d))[:3]
        assert np.array_equal(near[o], nbr[rcv][nbr[rcv] >= 0])
    # loop form equals vectorised form, whatever the row blocking
    for rows in (256, 5):
        by_cell = IR.idw_by_cell(p, c.scores, c.labels, votes, rows=rows)
        for a, b in zip(by_cell, (ic.i_scores, ic.i_labels, source, ic.n_transferred, nbr, wgt)):
            assert np.array_equal(a, b)
    # step 4 again from neighbours, weights, scores and votes: the receivers' scores bit for bit
    q = np.maximum(nbr[got], 0)
    with np.errstate(over="ignore", invalid="ignore"):
        m = c.scores[q] / votes[q].astype(f32)[:, :, None]  # (receivers, 3, K)
        w = wgt[got]
        acc, wsum = w[:, 0:1] * m[:, 0], w[:, 0]
        for j in (1, 2):
            use = have[:, j]
            acc = np.where(use[:, None], acc + w[:, j:j + 1] * m[:, j], acc)
            wsum = np.where(use, wsum + w[:, j], wsum)
        again = np.where((wsum == 0)[:, None], m[:, 0], acc / wsum[:, None])
    assert again.dtype == f32 and np.array_equal(again, ic.i_scores[got])


def test_the_cases_cover_every_condition():
    assert IR.conditions_covered()
    wide1 = IR.case("wide N=1 c=1")
    got = (wide1.c.votes == 0) & (wide1.source >= 0)
    n = (wide1.neighbours[got] >= 0).sum(1)
    assert int((n == 1).sum()) > 100 and int((n == 2).sum()) >= 1 and not (n == 3).any()
    wide4 = IR.case("wide N=4")
    got = (wide4.c.votes == 0) & (wide4.source >= 0)
    assert ((wide4.neighbours[got] >= 0).sum(1) == 2).all() and wide4.has["no_source"]
    far = IR.case("all inf")
    assert (far.weights[far.far] == 0).all() and far.source[far.far] >= 0 and far.i_labels[far.far] >= 0


def test_weights_and_the_fallback():
    w = IR.weights_of(np.array([0.0, 1.0, np.inf, 3e38], f32))
    assert w.dtype == f32 and w[0] == f32(1.0) / f32(1e-8) and w[1] == f32(1.0) / (f32(1.0) + f32(1e-8)) and w[2] == 0 and w[3] > 0
    m = np.array([[1.0, -2.0], [3.0, 5.0], [7.0, 11.0]], f32)
    assert np.array_equal(IR.interpolate(m, np.zeros(3, f32)), m[0])                     # wsum == 0: the nearest one's means
    assert np.array_equal(IR.interpolate(m[:1], w[1:2]), (w[1] * m[0]) / w[1])           # one neighbour: no special case
    two = IR.interpolate(m[:2], w[:2])
    assert np.array_equal(two, (w[0] * m[0] + w[1] * m[1]) / (w[0] + w[1]))
    assert np.array_equal(IR.interpolate(m, np.array([w[0], 0, 0], f32)), (w[0] * m[0]) / w[0])  # farther ones at +inf


def test_the_new_entry_point_refuses_null_pointers_and_short_workspaces():
    lib = _lib.load()
    err = lambda: lib.r3d_last_error_string().decode()
    p = ctypes.c_void_p(64)  # never dereferenced: every call below fails its argument checks before any launch
    assert _lib.ABI_VERSION == 6 and "r3d_scene_transfer" in _lib.header_symbols()
    # ABI 6 merged the twins into the entry points they were named after
    assert not {"r3d_scene_" + twin for twin in ("prepare_run", "vote_run", "transfer_idw")} & set(_lib.header_symbols())
    words, sw = lib.r3d_scene_ws_words(1000, 6, 4, 50), lib.r3d_scene_sparse_ws_words(1000, 6, 4, 50)

    def idw(n=words, sn=sw, K=3, scan=p, ws=p, sws=p, scores=p, labels=p, votes=p, src=p, nbr=p, wgt=p):
        return lib.r3d_scene_transfer(scan, 6, 1000, 6, 4, 50, ws, n, sws, sn, K, scores, labels, votes, src, nbr, wgt, None)
    for name in ("scan", "ws", "sws", "scores", "labels", "votes", "src", "nbr", "wgt"):
        assert idw(**{name: None}) != 0 and "null" in err(), name
    assert idw(n=words - 1) != 0 and "workspace" in err()
    assert idw(sn=sw - 1) != 0 and "sparse workspace" in err()
    assert idw(K=65) != 0 and "n_classes" in err()
    assert idw(K=0) != 0 and "n_classes" in err()
    # the messages are those of r3d_scene_transfer
    tr = lambda n, sn, K=3: lib.r3d_scene_transfer(p, 6, 1000, 6, 4, 50, p, n, p, sn, K, p, p, p, p, None, None, None)
    for kw, args in ((dict(n=words - 1), (words - 1, sw)), (dict(sn=sw - 1), (words, sw - 1)), (dict(K=65), (words, sw, 65))):
        assert idw(**kw) != 0
        mine = err()
        assert tr(*args) != 0 and err() == mine
