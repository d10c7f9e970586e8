"""smooth_scene without a device: the numpy restatement tests/scene_smooth_ref.py (which the GPU tests compare the kernels
with bit for bit) against float64 sweeps with a dense matrix, against numbers worked by hand, and against the property that
makes the function worth calling ("Smoothing a labelled scan", S7); every refusal of the host checks; the
signatures and the entry points' own argument checks."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import scene_smooth_cases as C  # noqa: E402
import scene_smooth_ref as R  # noqa: E402

from r3dfsseg_amd import _lib, fitted as F, scene, scene_segments, scene_smooth as S  # noqa: E402

f32 = np.float32
EPS32 = float(np.finfo(f32).eps)


def _ref(case, **kw):
    return R.smooth(case["scan"], case["scores"], case["votes"], case["labels"], voxel=C.VOX, **kw)


# ---- the restatement against float64 ------------------------------------------------------------------------------------------
def _dense_float64(case, got, connectivity, alpha, iterations, nbrs=None):
    """S2-S4 in float64: Y as plain means, the sweeps with a dense V x V adjacency matrix built from the voxels' coordinates
    (or, with a colour gate, from the restatement's neighbour lists: which voxels are joined is no matter of rounding).
    alpha and 1 - alpha are the float32 values the definition uses, widened.  -> (Z (V, C) float64, ring, n_max)."""
    V, vi = got["n_voxels"], got["voxel_index"]
    scores, votes = case["scores"].astype(np.float64), case["votes"]
    contrib = (vi >= 0) & (votes > 0)
    members = np.bincount(vi[contrib], minlength=V)
    Y = np.zeros((V, scores.shape[1]))
    np.add.at(Y, vi[contrib], scores[contrib] / votes[contrib, None])
    Y[members > 0] /= members[members > 0, None]
    if nbrs is None:
        coord = np.zeros((V, 3), np.int64)
        coord[vi[vi >= 0]] = case["coords"][vi >= 0] - case["coords"][vi >= 0].min(0)
        d = np.abs(coord[:, None, :] - coord[None, :, :])
        A = (d.max(2) == 1) if connectivity == 26 else (d.sum(2) == 1)
    else:
        A = np.zeros((V, V), bool)
        for v, nb in enumerate(nbrs):
            A[v, nb] = True
    a = float(f32(alpha))
    b = float(f32(1) - f32(alpha))
    Z, ring = Y.copy(), np.where(members > 0, 0, -1)
    for t in range(iterations):
        At = A & ((ring >= 0) & (ring <= t))[None, :]
        n = At.sum(1)
        m = (At.astype(np.float64) @ Z) / np.maximum(n, 1)[:, None]
        has, mem = n > 0, members > 0
        Zn = Z.copy()
        Zn[has & mem] = b * Y[has & mem] + a * m[has & mem]
        Zn[has & ~mem] = m[has & ~mem]
        ring = np.where(has & ~mem & (ring < 0), t + 1, ring)
        Z = Zn
    return Z, ring, int(members.max())


@pytest.mark.parametrize("connectivity", [6, 26])
@pytest.mark.parametrize("iterations", [0, 1, 7])
def test_the_restatement_agrees_with_float64_sweeps(connectivity, iterations):
    """The bound.  u = eps32 / 2 is the unit roundoff.  S2: a row c_p carries one division, u |c|; n of them added one at a
    time carry at most (n - 1) u n max|c| to first order, divided by n that is (n - 1) u max|c|, and the division adds u: Y
    is off by at most (n_max + 1) u max|c|.  S4: m sums at most 26 values (25 additions) and divides, 26 u max|Z|; b Y + a m
    adds three roundings: fewer than 30 u max|Z| a sweep, and |Z| <= max|c| because every sweep is a convex combination of
    rows of Y -- for the same reason the errors of the sweep before and of Y enter with weights that sum to 1 and add at
    most linearly: after t sweeps (30 t + n_max + 1) u max|c|.  The issue states the first-order bound with eps32 in the
    place of u and n_max + 2, and doubles it for the higher-order terms: (30 t + n_max + 2) eps32 max|c| * 2, four times
    what the derivation needs."""
    case = C.random_case(11)
    alpha = 0.8
    got = _ref(case, connectivity=connectivity, alpha=alpha, iterations=iterations)
    Z, ring, n_max = _dense_float64(case, got, connectivity, alpha, iterations)
    assert np.array_equal(ring, got["voxel_ring"]) and got["n_voxels"] > 300 and (ring < 0).sum() + (ring > 0).sum() > 0
    assert iterations == 0 or (ring > 0).sum() > 0  # some voxels hold voteless points only and are filled
    cmax = float(np.abs(case["scores"][case["votes"] > 0] / case["votes"][case["votes"] > 0, None]).max())
    bound = 2 * (30 * iterations + n_max + 2) * EPS32 * cmax
    err = float(np.abs(got["voxel_scores"].astype(np.float64) - Z).max())
    print("connectivity %d, %d sweeps: max error %.3g, bound %.3g" % (connectivity, iterations, err, bound))
    assert err <= bound
    if iterations:  # and the check can fail: the sweeps moved the rows by far more than the bound
        assert float(np.abs(got["voxel_scores"] - got["voxel_evidence"]).max()) > 1000 * bound


def test_the_restatement_agrees_with_float64_sweeps_behind_a_colour_gate():
    case = C.random_case(13)
    got = _ref(case, connectivity=26, alpha=0.6, iterations=5, colour_tol=0.25)
    grown = R.scene_grow_ref.grow(case["scan"], C.VOX, 0.25, 6)
    nbrs = R.neighbours_of(grown, 26, 0.25)
    free = R.neighbours_of(grown, 26, None)
    assert sum(map(len, nbrs)) < sum(map(len, free))  # the gate cuts edges
    Z, ring, n_max = _dense_float64(case, got, 26, 0.6, 5, nbrs)
    cmax = float(np.abs(case["scores"][case["votes"] > 0] / case["votes"][case["votes"] > 0, None]).max())
    assert np.array_equal(ring, got["voxel_ring"])
    assert float(np.abs(got["voxel_scores"].astype(np.float64) - Z).max()) <= 2 * (30 * 5 + n_max + 2) * EPS32 * cmax


def test_the_sweeps_converge_to_the_linear_system_of_s7():
    """(I - alpha P) Z = (1 - alpha) Y with P the row-normalised adjacency, solved in float64: a sweep contracts the distance
    to that fixed point by alpha, so after 64 sweeps with alpha = 1 / 2 what is left of the first distance, at most 2
    max|c|, is below 2^-63 of it, and the float32 sweeps are within the bound of the test above of the float64 ones."""
    case = C.slabs_case()  # every voxel has members and neighbours
    alpha, iterations = 0.5, 64
    got = _ref(case, connectivity=26, alpha=alpha, iterations=iterations)
    V = got["n_voxels"]
    assert (got["voxel_members"] > 0).all() and V == 32
    A = np.zeros((V, V))
    for v, nb in enumerate(R.neighbours_of(R.scene_grow_ref.grow(case["scan"], C.VOX, None, 6), 26)):
        A[v, nb] = 1
    P = A / A.sum(1, keepdims=True)
    rows = case["scores"].astype(np.float64) / case["votes"][:, None]
    Y = np.stack([rows[got["voxel_index"] == v].mean(0) for v in range(V)])
    Z = np.linalg.solve(np.eye(V) - alpha * P, (1 - alpha) * Y)
    cmax = float(np.abs(rows).max())
    bound = 2 * (30 * iterations + int(got["voxel_members"].max()) + 2) * EPS32 * cmax + 2.0 ** -63 * 2 * cmax
    err = float(np.abs(got["voxel_scores"] - Z).max())
    print("64 sweeps against the solve: max error %.3g, bound %.3g" % (err, bound))
    assert err <= bound and float(np.abs(got["voxel_evidence"] - Z).max()) > 1000 * bound


# ---- numbers worked by hand ---------------------------------------------------------------------------------------------------
def _chain3(votes_c):
    """Voxels A B C in a line, one point each, rows (8, 0), (0, 2), (-4, 0) with one vote (C: votes_c)."""
    coords = np.array([(0, 0, 0), (1, 0, 0), (2, 0, 0)], np.int64)
    scores = np.array([[8, 0], [0, 2], [-4, 0]], f32)
    votes = np.array([1, 1, votes_c], np.int32)
    if votes_c == 0:
        scores[2] = (5, 5)  # a voteless point's row is no evidence
    return C.case_of(C.GC.scan_of(coords)[:, :3].copy(), scores, votes, coords=coords)


def test_a_chain_of_three_voxels_by_hand():
    """alpha = 1 / 2.  All voted, Y = (8, 0), (0, 2), (-4, 0):
      sweep 1: A: m = Y_B = (0, 2), Z = (4, 1); B: m = ((8, 0) + (-4, 0)) / 2 = (2, 0), Z = (1, 1); C: m = (0, 2), Z = (-2, 1)
      sweep 2: A: m = (1, 1), Z = (4.5, 0.5); B: m = ((4, 1) + (-2, 1)) / 2 = (1, 1), Z = (0.5, 1.5); C: m = (1, 1), Z = (-1.5, 0.5)
    C voteless, Y_C = 0, ring -1:
      sweep 1: A as before, (4, 1); B: only A is live, m = (8, 0), Z = (4, 1); C: m = Y_B = (0, 2), Z = (0, 2), ring 1
      sweep 2: A: m = (4, 1), Z = (6, 0.5); B: A and C live, m = ((4, 1) + (0, 2)) / 2 = (2, 1.5), Z = (1, 1.75); C: m = (4, 1)"""
    full = _chain3(1)
    for connectivity in (6, 26):
        one = _ref(full, connectivity=connectivity, alpha=0.5, iterations=1)
        assert one["voxel_scores"].tolist() == [[4, 1], [1, 1], [-2, 1]] and one["voxel_labels"].tolist() == [0, 0, 1]
        two = _ref(full, connectivity=connectivity, alpha=0.5, iterations=2)
        assert two["voxel_scores"].tolist() == [[4.5, 0.5], [0.5, 1.5], [-1.5, 0.5]] and two["voxel_labels"].tolist() == [0, 1, 1]
        assert two["voxel_ring"].tolist() == [0, 0, 0] and two["votes"].tolist() == [1, 1, 1] and two["smoothed"].all()
        assert full["labels"].tolist() == [0, 1, 1] and (one["n_changed"], two["n_changed"]) == (1, 0)  # B's tie goes to class 0
        assert (two["n_smoothed"], two["n_filled"], two["n_unlabelled"]) == (3, 0, 0)
    hole = _chain3(0)
    zero = _ref(hole, alpha=0.5, iterations=0)
    assert zero["voxel_scores"].tolist() == [[8, 0], [0, 2], [0, 0]] and zero["voxel_ring"].tolist() == [0, 0, -1]
    assert zero["voxel_labels"].tolist() == [0, 1, -1] and zero["labels"].tolist() == [0, 1, -1]
    assert zero["scores"][2].tolist() == [5, 5] and zero["votes"].tolist() == [1, 1, 0] and zero["smoothed"].tolist() == [True, True, False]
    one = _ref(hole, alpha=0.5, iterations=1)
    assert one["voxel_scores"].tolist() == [[4, 1], [4, 1], [0, 2]] and one["voxel_ring"].tolist() == [0, 0, 1]
    two = _ref(hole, alpha=0.5, iterations=2)
    assert two["voxel_scores"].tolist() == [[6, 0.5], [1, 1.75], [4, 1]] and two["voxel_ring"].tolist() == [0, 0, 1]
    assert two["voxel_labels"].tolist() == [0, 1, 0] and two["labels"].tolist() == [0, 1, 0] and two["votes"].tolist() == [1, 1, 1]
    assert (two["n_member_voxels"], two["n_filled_voxels"], two["n_smoothed"], two["n_changed"], two["n_filled"]) == (2, 1, 3, 0, 1)
    # alpha = 0 leaves the evidence where there is some, and still fills
    still = _ref(hole, alpha=0.0, iterations=3)
    assert still["voxel_scores"].tolist() == [[8, 0], [0, 2], [0, 2]] and still["voxel_ring"].tolist() == [0, 0, 1]


def test_filling_goes_one_ring_a_sweep_and_keeps_signed_zeros():
    chain = C.chain_case()
    two = _ref(chain, alpha=0.8, iterations=2)
    assert two["voxel_ring"].tolist() == [0, 1, 2, -1, -1, 0, -1] and two["n_filled_voxels"] == 2 and two["n_filled"] == 0
    assert two["labels"].tolist()[4:6] == [1, 1] and two["scores"][4].tolist() == [-1.25, 0.5] and two["votes"].tolist()[2:6] == [1, 1, 0, 0]
    assert two["voxel_evidence"][0].tolist() == [2, 1] and two["voxel_scores"][5].tolist() == [-0.5, 4]  # the isolated one keeps Y
    four = _ref(chain, alpha=0.8, iterations=4)
    assert four["voxel_ring"].tolist() == [0, 1, 2, 3, 4, 0, -1] and four["n_unlabelled"] == 1 and four["n_smoothed"] == 7
    z = _ref(C.negative_zero_case(), alpha=0.8, iterations=1)
    assert np.array_equal(z["voxel_scores"].view(np.uint32), np.array([[-0.0, 0.0], [-0.0, 0.0]], f32).view(np.uint32))


# ---- S7: what the sweeps are good for -----------------------------------------------------------------------------------------
def _wrong_voxels(case, got, among=None):
    """Wrong labels before and after, counted over the points (one point a voxel) of `among`."""
    among = np.ones(len(case["truth"]), bool) if among is None else among
    return int((case["labels"][among] != case["truth"][among]).sum()), int((got["labels"][among] != case["truth"][among]).sum())


@pytest.mark.parametrize("connectivity", [6, 26])
def test_alpha_decides_whether_an_isolated_error_is_overturned(connectivity):
    """The room of S7, seed fixed: 16 x 16 x 8 voxels, two half-spaces with logits +-1, 15 % of the voxels flipped."""
    room = C.room_case(flip=0.15)
    before = int(room["wrong"].sum())
    assert 250 < before < 400
    for iterations in (1, 4, 10):
        got = _ref(room, connectivity=connectivity, alpha=0.8, iterations=iterations)
        was, now = _wrong_voxels(room, got)
        print("connectivity %d, alpha 0.8, %d sweeps: %d -> %d wrong voxels" % (connectivity, iterations, was, now))
        assert was == before and now < was / 2
    # alpha = 1 / 2: Z = (Y + m) / 2 with |m_j| <= 1 = |Y_j|, so a voxel's own class is never the strictly smaller one.  It can
    # TIE, when m = -Y exactly, that is when every neighbour holds -Y exactly: only in sweep 1, which reads Z_0 = Y.  From
    # sweep 2 on a neighbour u of such a voxel v has v's opposite row among its own neighbours, so |Z_t[u]| < 1, |m| < 1 at
    # v, and v's row is strictly on the side of Y_v again.  So none changes after 2, 4 and 10 sweeps; after exactly one,
    # the rows of the voxels whose whole neighbourhood disagrees are (0, 0), the arg-max gives a tie to class 0, and those
    # are all that change.
    for iterations in (2, 4, 10):
        got = _ref(room, connectivity=connectivity, alpha=0.5, iterations=iterations)
        print("connectivity %d, alpha 0.5, %d sweeps: %d labels changed" % (connectivity, iterations, got["n_changed"]))
        assert got["n_changed"] == 0 and np.array_equal(got["labels"], room["labels"])
    got = _ref(room, connectivity=connectivity, alpha=0.5, iterations=1)
    changed = got["labels"] != room["labels"]
    own = np.take_along_axis(got["scores"], room["labels"][:, None], 1)[:, 0]
    other = np.take_along_axis(got["scores"], 1 - room["labels"][:, None], 1)[:, 0]
    print("connectivity %d, alpha 0.5, 1 sweep: %d ties go to class 0" % (connectivity, changed.sum()))
    assert (own >= other).all() and np.array_equal(changed, (own == other) & (room["labels"] == 1)) and changed.sum() == got["n_changed"]
    assert (got["scores"][changed] == 0).all() and (got["labels"][changed] == 0).all()


@pytest.mark.parametrize("connectivity", [6, 26])
def test_stripped_voxels_are_filled_and_the_rest_still_improves(connectivity):
    room = C.room_case(flip=0.15, strip=0.30)
    live = ~room["stripped"]
    got = _ref(room, connectivity=connectivity, alpha=0.8, iterations=10)
    assert room["stripped"].sum() > 500 and (room["labels"][room["stripped"]] == -1).all()
    assert got["n_unlabelled"] == 0 and got["n_filled"] == int(room["stripped"].sum()) == got["n_filled_voxels"]
    was, now = _wrong_voxels(room, got, live)
    print("connectivity %d, 30 %% stripped: %d -> %d wrong live voxels" % (connectivity, was, now))
    assert now < was / 2


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def _res(M=10, Cn=3, scores=None, votes=None, labels=None):
    return scene.SceneResult(labels=torch.zeros(M, dtype=torch.int64) if labels is None else labels,
                             scores=torch.zeros(M, Cn) if scores is None else scores,
                             votes=torch.ones(M, dtype=torch.int32) if votes is None else votes, n_blocks=1, n_chunks=1,
                             n_unlabelled=0, redone=0)


def test_argument_errors_are_raised_without_a_device():
    ok, res = np.zeros((10, 6), f32), _res()
    sets = scene.SceneSetsResult(torch.zeros(10, 2, 3), torch.zeros(10, 2, dtype=torch.int64), res.votes, res.labels,
                                 torch.zeros(10, dtype=torch.int32), torch.zeros(10), 1, 1, 0, 0)
    with pytest.raises(ValueError, match="res is a SceneSetsResult; only a scene.SceneResult is smoothed"):
        S.smooth_scene(sets, ok)
    with pytest.raises(ValueError, match="res is a SegmentResult; only a scene.SceneResult is smoothed"):
        S.smooth_scene(scene_segments.SegmentResult(scores=res.scores, votes=res.votes, labels=res.labels), ok)
    for wrong in (None, {"scores": 1}, res.scores):
        with pytest.raises(ValueError, match="res must be a scene.SceneResult"):
            S.smooth_scene(wrong, ok)
    for wrong in (_res(scores=torch.zeros(10, 3, dtype=torch.float64)), _res(scores=torch.zeros(10)), _res(scores=torch.zeros(10, 0)),
                  _res(votes=torch.ones(10, dtype=torch.int64)), _res(votes=torch.ones(9, dtype=torch.int32)),
                  _res(labels=torch.zeros(10, dtype=torch.int32)), _res(labels=torch.zeros(10, 1, dtype=torch.int64)),
                  _res(scores=np.zeros((10, 3), f32))):
        with pytest.raises(ValueError, match="res does not hold the tensors of a SceneResult"):
            S.smooth_scene(wrong, ok)
    with pytest.raises(ValueError, match="65 score columns"):
        S.smooth_scene(_res(Cn=65), ok)
    for wrong in (np.zeros(10, f32), np.zeros((10, 2), f32), np.zeros((10, 4), f32), np.zeros((0, 3), f32), [[0.0, 0.0, 0.0]], None):
        with pytest.raises(ValueError, match="smooth_scene: scan must be"):
            S.smooth_scene(res, wrong)
    with pytest.raises(ValueError, match="smooth_scene: scan must be float32"):
        S.smooth_scene(res, np.zeros((10, 3), np.float64))
    with pytest.raises(ValueError, match="a scan of 11 points for the 10 points of res"):
        S.smooth_scene(res, np.zeros((11, 3), f32))
    for v in (0, -0.05, float("nan"), float("inf"), 1e-60, None, True):
        with pytest.raises(ValueError, match="smooth_scene: voxel .* must be a finite float > 0"):
            S.smooth_scene(res, ok, voxel=v)
    for c in (4, 18, 6.0, "26", None, True):
        with pytest.raises(ValueError, match="smooth_scene: connectivity .* must be 6 or 26"):
            S.smooth_scene(res, ok, connectivity=c)
    for a in (1, 1.0, -0.1, 1.5, float("nan"), float("inf"), 0.99999999, None, "0.8", True):
        with pytest.raises(ValueError, match=r"alpha .* must be a real number in \[0, 1\)"):
            S.smooth_scene(res, ok, alpha=a)
    for n in (-1, 65, 10.0, None, "10", True):
        with pytest.raises(ValueError, match="iterations .* must be an integer in 0 .. 64"):
            S.smooth_scene(res, ok, iterations=n)
    for t in (-0.1, float("nan"), float("inf"), "0.1", True, 1e60):
        with pytest.raises(ValueError, match="smooth_scene: colour_tol .* must be None or a finite float >= 0"):
            S.smooth_scene(res, ok, colour_tol=t)
    with pytest.raises(ValueError, match="colour_tol 0.1 given, but a scan of 3 columns has no colour"):
        S.smooth_scene(res, np.zeros((10, 3), f32), colour_tol=0.1)
    # every argument in order: the tensors of a hand-built result on the host are the one thing left to refuse
    for kw in (dict(), dict(alpha=0, iterations=0, connectivity=6), dict(alpha=np.float32(0.5), iterations=np.int64(64), colour_tol=0)):
        with pytest.raises(ValueError, match="the tensors of res must be on the device"):
            S.smooth_scene(res, ok, **kw)


def test_signatures_and_abi():
    names = ["res", "scan", "voxel", "connectivity", "alpha", "iterations", "colour_tol"]
    assert list(inspect.signature(S.smooth_scene).parameters) == names
    assert list(inspect.signature(F.FittedLearner.smooth_scene).parameters) == ["self"] + names
    for fn in (S.smooth_scene, F.FittedLearner.smooth_scene):
        defaults = {k: p.default for k, p in inspect.signature(fn).parameters.items() if k in names[2:]}
        assert defaults == dict(voxel=0.05, connectivity=26, alpha=0.8, iterations=10, colour_tol=None)
    from r3dfsseg_amd import mpti_learner, proto_contrast_learner, proto_learner
    for cls in (mpti_learner.MPTILearner_V3, proto_learner.ProtoLearner, proto_contrast_learner.ProtoContrastLearner):
        assert cls.smooth_scene is F.FittedLearner.smooth_scene
    assert issubclass(S.SmoothResult, scene.SceneResult) and not issubclass(S.SmoothResult, scene.SceneSetsResult)
    assert _lib.ABI_VERSION == 6
    smooth = [n for n in _lib.header_symbols() if n.startswith("r3d_scene_smooth_")]
    assert smooth == ["r3d_scene_smooth_" + n for n in ("evidence", "graph", "spread", "sweep")]


def test_entry_points_check_their_arguments():
    lib = _lib.load()
    err = lambda: lib.r3d_last_error_string().decode()
    p, q = ctypes.c_void_p(64), ctypes.c_void_p(128)  # never dereferenced: every call below fails its checks before any launch
    M, V = 1000, 100
    words = lib.r3d_scene_grow_ws_words(M)
    ev = lambda **kw: lib.r3d_scene_smooth_evidence(kw.get("M", M), kw.get("nx", 4), 4, 4, kw.get("C", 3), kw.get("scores", p), p,
                                                    kw.get("V", V), p, p, p, p, kw.get("words", words), None)
    assert ev(scores=None) != 0 and "null pointer" in err()
    assert ev(words=words - 1) != 0 and "workspace of" in err()
    assert ev(C=65) != 0 and "65 score columns" in err()
    assert ev(C=0) != 0 and "0 score columns" in err()
    assert ev(V=0) != 0 and "0 voxels of 1000 points" in err()
    assert ev(V=M + 1) != 0 and "1001 voxels of 1000 points" in err()
    assert ev(nx=1025) != 0 and "1025 x 4 x 4 voxels" in err()
    assert ev(M=0) != 0 and "M 0" in err()
    gr = lambda **kw: lib.r3d_scene_smooth_graph(M, 4, 4, 4, kw.get("V", V), kw.get("conn", 26), kw.get("mean", None),
                                                 kw.get("tol", 0.0), kw.get("nbr", p), p, kw.get("words", words), None)
    assert gr(nbr=None) != 0 and "null pointer" in err()
    assert gr(conn=18) != 0 and "connectivity 18" in err()
    assert gr(mean=p, tol=-1.0) != 0 and "colour_tol -1" in err()
    assert gr(mean=p, tol=float("nan")) != 0 and "colour_tol" in err()
    assert gr(words=10) != 0 and "workspace of" in err()
    assert gr(V=M + 1) != 0 and "voxels of" in err()
    sw = lambda **kw: lib.r3d_scene_smooth_sweep(M, kw.get("V", V), kw.get("C", 3), kw.get("n", 2), kw.get("alpha", 0.8), kw.get("Y", p),
                                                 p, kw.get("z0", p), kw.get("z1", q), p, None)
    assert sw(Y=None) != 0 and "null pointer" in err()
    assert sw(n=65) != 0 and "65 sweeps" in err()
    assert sw(n=-1) != 0 and "-1 sweeps" in err()
    assert sw(alpha=1.0) != 0 and "alpha 1" in err()
    assert sw(alpha=-0.5) != 0 and "alpha -0.5" in err()
    assert sw(alpha=float("nan")) != 0 and "alpha" in err()
    assert sw(z1=None) != 0 and "two arrays" in err()
    assert sw(z0=None, n=1) != 0 and "two arrays" in err()
    assert sw(z1=p) != 0 and "two arrays" in err()
    assert sw(C=65) != 0 and "65 score columns" in err()
    assert sw(V=0) != 0 and "0 voxels" in err()
    sp = lambda **kw: lib.r3d_scene_smooth_spread(kw.get("M", M), kw.get("C", 3), kw.get("V", V), p, p, p, p, p, p, p, p, p, p, p,
                                                  kw.get("counts", p), None)
    assert sp(counts=None) != 0 and "null pointer" in err()
    assert sp(C=0) != 0 and "0 score columns" in err()
    assert sp(V=M + 1) != 0 and "1001 voxels" in err()
    assert sp(M=2 ** 27 + 1) != 0 and "2^27" in err()
