"""Host side of predict_scene (r3dfsseg_amd/scene.py): properties of the numpy restatement the GPU tests compare with
(tests/scene_ref.py), argument errors raised with no device present, and the new entry points' own argument checks."""
import ctypes
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import scene_cases as SC  # noqa: E402
from scene_ref import RefPlan  # noqa: E402

from r3dfsseg_amd import _lib, fitted as F, scene, synthetic as S  # noqa: E402
from r3dfsseg_amd.mpti import MPTI_SelfAtten  # noqa: E402
from r3dfsseg_amd.protonet import ProtoNet, ProtoNet_Contrast  # noqa: E402


def _plans():
    yield "small r=1", SC.small_plan(1)
    yield "small r=2", SC.small_plan(2)
    room, _ = S.make_scene(S.make_cfg(), seed=2, extent=(3.0, 2.0, 3.0), n_points=6000)
    yield "room r=2", RefPlan(room.numpy(), 128, block_size=1.0, stride=0.5, min_points=50)
    yield "room r=3", RefPlan(room.numpy(), 200, block_size=1.5, stride=0.5, min_points=1)


@pytest.mark.parametrize("name,p", list(_plans()), ids=lambda v: v if isinstance(v, str) else "")
def test_properties_of_the_restatement(name, p):
    N = p.N
    assert p.n_chunks > 0 and p.slot_map.shape == (p.n_chunks, N)
    for b, lst in enumerate(p.block_list):
        c0, c1 = p.block_chunk0[b], p.block_chunk0[b + 1]
        if not p.kept[b]:
            assert c0 == c1
            continue
        assert c1 - c0 == -(-len(lst) // N)
        seen = np.concatenate([np.unique(p.slot_map[c]) for c in range(c0, c1)])
        # every point of a kept block sits in exactly one chunk of that block (block lists hold valid points only)
        assert len(seen) == len(lst) and set(seen.tolist()) == set(lst) and p.valid[lst].all()
        for c in range(c0, c1):
            _, j, ln = p.chunks[c]
            assert 1 <= ln <= N and ln == -(-(len(lst) - j) // (c1 - c0))
    scores, labels, votes = p.vote(np.ones((p.n_chunks, 3, N), np.float32))
    assert int(votes.sum()) == p.n_chunks * N
    assert (votes[~p.valid] == 0).all() and (labels[votes == 0] == -1).all() and (labels[votes > 0] == 0).all()
    assert (scores[:, 0] == votes).all()
    in_blocks = np.zeros(p.M, np.int32)
    for lst in p.block_list:
        in_blocks[lst] += 1
    assert in_blocks.max() <= p.r * p.r
    if p.r == 1:
        assert in_blocks.max() == 1  # each point at most one block


def test_make_scene_is_seeded_and_labelled():
    cfg = S.make_cfg(n_way=2)
    a, la = S.make_scene(cfg, seed=4, extent=(2.0, 1.0, 3.0), n_points=500)
    b, lb = S.make_scene(cfg, seed=4, extent=(2.0, 1.0, 3.0), n_points=500)
    assert a.shape == (500, 6) and a.dtype == torch.float32 and la.dtype == torch.int64
    assert torch.equal(a, b) and torch.equal(la, lb)
    assert set(la.tolist()) == {0, 1, 2} and float(a[:, 0].min()) < -10 and 0 <= float(a[:, 3:].min()) and float(a[:, 3:].max()) <= 255


def _cpu_model(cls=ProtoNet, **over):
    cfg = S.make_cfg(n_way=2, k_shot=1, pc_npts=64, **over)
    m = cls(SimpleNamespace(**cfg))
    return m.eval(), cfg


@pytest.mark.parametrize("cls", [ProtoNet, ProtoNet_Contrast, MPTI_SelfAtten])
def test_argument_errors_come_before_any_device_work(cls):
    m, cfg = _cpu_model(cls)
    f = F.FittedSupport(m, protos=torch.zeros(1, 3, m.feat_dim))
    scan = torch.zeros(100, 6)
    with pytest.raises(ValueError, match="scan must be"):
        m.predict_scene(f, scan[:, :5])
    with pytest.raises(ValueError, match="scan must be"):
        m.predict_scene(f, scan[None])
    with pytest.raises(ValueError, match="scan must be"):
        m.predict_scene(f, scan[:, :3])               # no colour for a model with rgb
    with pytest.raises(ValueError, match="float32"):
        m.predict_scene(f, scan.double())
    with pytest.raises(ValueError, match="integer in 1..4"):
        m.predict_scene(f, scan, block_size=1.0, stride=0.4)
    with pytest.raises(ValueError, match="integer in 1..4"):
        m.predict_scene(f, scan, block_size=1.0, stride=0.2)
    with pytest.raises(ValueError, match="min_points"):
        m.predict_scene(f, scan, min_points=0)
    with pytest.raises(ValueError, match="groups_per_launch"):
        m.predict_scene(f, scan, groups_per_launch=0)
    m.train()
    with pytest.raises(NotImplementedError):
        m.predict_scene(f, scan)


def test_attributes_a_scan_cannot_supply():
    for attribs, dim, ok in (("xyz", 3, True), ("xyzXYZ", 6, True), ("xyzrgb", 6, True), ("rgbXYZ", 6, False), ("xyzrgb", 9, False)):
        m, _ = _cpu_model(pc_in_dim=dim, pc_attribs=attribs)
        scan = torch.zeros(10, 6 if "rgb" in attribs else 3)
        if ok:
            assert scene.check_scene_args(m, scan, 1.0, None, 100, 32)[3:] == scene.ATTRIBS[attribs]
        else:
            with pytest.raises(ValueError, match="pc_attribs"):
                m.predict_scene(None, scan)
    assert _cpu_model()[0].pc_attribs == "xyzrgbXYZ"
    assert scene.overlap_ratio(1.0, None) == (1, np.float32(1.0)) and scene.overlap_ratio(1.5, 0.5)[0] == 3
    assert scene.overlap_ratio(1.0, 0.25 * (1 + 1e-8))[0] == 4


def test_learners_have_predict_scene():
    from r3dfsseg_amd.mpti_learner import MPTILearner_V3
    from r3dfsseg_amd.proto_contrast_learner import ProtoContrastLearner
    from r3dfsseg_amd.proto_learner import ProtoLearner
    for L in (MPTILearner_V3, ProtoLearner, ProtoContrastLearner):
        assert callable(L.predict_scene) and callable(L._scene_launch)
    with pytest.raises(ValueError, match="call fit"):
        F.FittedLearner().predict_scene(torch.zeros(10, 6))


def test_entry_points_refuse_null_pointers_and_short_workspaces():
    lib = _lib.load()
    err = lambda: lib.r3d_last_error_string().decode()
    p = ctypes.c_void_p(64)  # never dereferenced: every call below fails its argument checks before any launch
    assert _lib.ABI_VERSION == 6
    assert lib.r3d_scene_bounds_ws_words(1000) == 5 * 4 and lib.r3d_scene_bounds_ws_words(10 ** 7) == 5 * 1024
    assert lib.r3d_scene_bounds(None, 6, 1000, p, p, 20, None) != 0 and "null" in err()
    assert lib.r3d_scene_bounds(p, 6, 1000, p, p, 19, None) != 0 and "workspace" in err()
    assert lib.r3d_scene_bounds(p, 6, 2 ** 27 + 1, p, p, 1 << 20, None) != 0 and "2^27" in err()
    words = lib.r3d_scene_ws_words(1000, 6, 4, 50)
    assert words > 5 * 1000 and lib.r3d_scene_ws_words(1000, 300, 300, 50) == -1 and lib.r3d_scene_ws_words(0, 6, 4, 50) == -1
    offs = (ctypes.c_long * 8)()
    assert lib.r3d_scene_ws_offsets(1000, 6, 4, 50, offs) == 0
    o = list(offs)
    assert len(set(o)) == 8 and all(0 <= v and v % 4 == 0 for v in o) and o[7] + 8 == words
    assert lib.r3d_scene_ws_offsets(1000, 6, 4, 50, None) != 0
    plan = lambda scan, ws, n, **k: lib.r3d_scene_plan(scan, 6, 1000, 0.0, 0.0, k.get("s", 0.5), k.get("ncx", 6), 4, k.get("r", 2),
                                                        256, k.get("mp", 100), 50, ws, n, None)
    assert plan(None, p, words) != 0 and "null" in err()
    assert plan(p, None, words) != 0 and "null" in err()
    assert plan(p, p, words - 1) != 0 and "workspace" in err()
    assert plan(p, p, words, r=5) != 0 and "1 .. 4" in err()
    assert plan(p, p, words, mp=0) != 0 and "min_points" in err()
    assert plan(p, p, words, s=0.0) != 0 and "cell size" in err()
    assert plan(p, p, 1 << 30, ncx=70000) != 0 and "cells" in err()
    prep = lambda scan, ws, out, n, **k: lib.r3d_scene_prepare(scan, k.get("ld", 6), 1000, 6, 4, 2, 256, 50, ws, n, None, 0,
                                                               k.get("c0", 0), k.get("G", 8), k.get("C", 9), k.get("rgb", 3), k.get("XYZ", 6), out,
                                                               9 * 256, 1, 9, None, None)
    assert prep(p, p, None, words) != 0 and "null" in err()
    assert prep(p, p, p, words - 1) != 0 and "workspace" in err()
    assert prep(p, p, p, words, c0=45) != 0 and "chunk table" in err()
    assert prep(p, p, p, words, C=6) != 0 and "does not hold" in err()
    assert prep(p, p, p, words, ld=3) != 0 and "colour" in err()
    vote = lambda ws, lg, n, **k: lib.r3d_scene_vote(1000, 6, 4, 2, 256, 50, ws, n, None, 0, lg, k.get("nch", 10), 3, p, p, p, None)
    assert vote(p, None, words) != 0 and "null" in err()
    assert vote(p, p, words - 1) != 0 and "workspace" in err()
    assert vote(p, p, words, nch=51) != 0 and "n_chunks" in err()
