"""The scans of the smooth_scene tests (host and GPU), each with the fields of a hand-built SceneResult, so no model is needed.

A case is a dict: scan (M, 3 or 6) float32, scores (M, C) float32, votes (M,) int32, labels (M,) int64, and what the test
needs to know about it (coords: the voxel of every point).  The scans come from scene_grow_cases.scan_of: an edge of 0.5 and
fractions that are multiples of 1 / 8, so every coordinate is exact in float32 and the voxel of a point is its coordinate
less the lowest one."""
import numpy as np

import scene_grow_cases as GC
import scene_segments_ref
import scene_sets_ref

f32 = np.float32
VOX = GC.VOX


def labels_of(scores, votes):
    """The labels predict_scene gives: the arg-max of a voted row, -1 without a vote."""
    out = np.full(len(scores), -1, np.int64)
    with np.errstate(invalid="ignore"):
        for p in np.flatnonzero(np.asarray(votes) > 0):
            out[p] = scene_sets_ref.argmax_lowest(scores[p])[0]
    return out


def case_of(scan, scores, votes, labels=None, **more):
    scores, votes = np.ascontiguousarray(scores, f32), np.asarray(votes, np.int32)
    assert scan.dtype == f32 and scores.shape[0] == scan.shape[0] == votes.shape[0]
    return dict(scan=scan, scores=scores, votes=votes, labels=labels_of(scores, votes) if labels is None else labels, **more)


def voted(rs, n, C, max_votes=4):
    """n rows of summed logits: small integers over eight, times the votes -- sums of a few hundred stay exact."""
    votes = rs.randint(1, max_votes + 1, n).astype(np.int32)
    return (rs.randint(-16, 17, (n, C)) / 8.0 * votes[:, None]).astype(f32), votes


# ---- 1. the tiles of the evidence: voxels of 1, 256, 257 and 513 contributors
CONTRIBUTORS = (1, 256, 257, 513)


def contributors_case(C=3):
    """Four voxels in a row along x, two cells apart (no neighbours), voxel i with CONTRIBUTORS[i] voted points whose column
    0 holds scene_segments_ref.cancelling_rows in scan order (the sum depends on the order and on the tiles), times the
    point's votes; between them about as many voteless points, which count for no rank; the scan order is shuffled with the
    order inside every voxel kept.  -> the case; Y0 (4,) float32: column 0 of the evidence by P3."""
    rs = np.random.RandomState(31)
    coords, col0, votes, group, want = [], [], [], [], []
    for g, n in enumerate(CONTRIBUTORS):
        rows = scene_segments_ref.cancelling_rows(n)[:, 0] if n >= 3 else np.full(n, 0.75, f32)
        want.append(scene_segments_ref.pool_rows(rows[:, None])[0] / f32(n))
        slots = np.sort(rs.permutation(2 * n)[:n])  # which of the voxel's 2 n points are the contributors
        v, c = np.zeros(2 * n, np.int32), np.full(2 * n, 7.0, f32)
        v[slots] = rs.randint(1, 4, n)
        c[slots] = rows * v[slots]  # 1e8 * 3 is exact in float32, and so is the division back
        coords += [(2 * g, 0, 0)] * (2 * n)
        col0 += list(c)
        votes += list(v)
        group += [g] * (2 * n)
    coords, group = np.array(coords, np.int64), np.array(group)
    scores = (rs.randint(-8, 9, (len(coords), C)) / 4.0).astype(f32) * np.maximum(np.array(votes, f32), 1)[:, None]
    scores[:, 0] = col0
    perm = GC.shuffled_within(group, np.random.RandomState(32))
    frac = rs.randint(1, 8, coords.shape) / 8.0
    return case_of(GC.scan_of(coords[perm], frac[perm])[:, :3].copy(), scores[perm], np.array(votes, np.int32)[perm],
                   coords=coords[perm], Y0=np.array(want, f32))


# ---- 2. V and C at the edges of a wave and a workgroup
def strip_case(V, C, seed=0):
    """V voxels that fill a strip three cells wide (x fastest: voxel i at (i % 3, i // 3, 0)), 1 .. 3 points each, about a
    sixth of them voteless and a few invalid; every fifth voxel holds voteless points only."""
    rs = np.random.RandomState(100 + 7 * V + C + seed)
    voxels = np.array([(i % 3, i // 3, 0) for i in range(V)], np.int64)
    per = rs.randint(1, 4, V)
    coords = np.repeat(voxels, per, 0)
    owner = np.repeat(np.arange(V), per)
    scores, votes = voted(rs, len(coords), C)
    votes[(rs.rand(len(coords)) < 1 / 6.0) | (owner % 5 == 4)] = 0
    if V == 1:
        votes[:] = np.maximum(votes, 1)
    scores[votes == 0] = 0
    perm = rs.permutation(len(coords))
    coords, scores, votes = coords[perm], scores[perm], votes[perm]
    scan = GC.scan_of(coords, rs.randint(1, 8, coords.shape) / 8.0)[:, :3].copy()
    if V > 1:  # a few more points, invalid ones, voted and not, between the others: copies of rows with one coordinate spoilt
        n_bad = max(2, len(coords) // 40)
        src, at = rs.randint(0, len(coords), n_bad), np.sort(rs.randint(0, len(coords), n_bad))
        bad = scan[src].copy()
        bad[np.arange(n_bad), rs.randint(0, 3, n_bad)] = rs.choice(np.array([np.nan, np.inf, -np.inf], f32), n_bad)
        bad_scores, bad_votes = voted(rs, n_bad, C)
        bad_votes[::2] = 0
        scan, scores, votes = np.insert(scan, at, bad, 0), np.insert(scores, at, bad_scores, 0), np.insert(votes, at, bad_votes)
        coords = np.insert(coords, at, -1, 0)
    return case_of(scan, scores, votes, coords=coords)


# ---- 3. filling ring by ring: a voted voxel, then four voteless ones in a line; an isolated voxel beside them
def chain_case(C=2):
    """Voxels (0..4, 0, 0): the first holds two voted points, the other four one voteless point each with scores and a label
    of their own (a receiver's); (8, 0, 0) is isolated and voted; (8, 3, 0) is isolated and voteless."""
    coords = np.array([(0, 0, 0), (0, 0, 0), (1, 0, 0), (2, 0, 0), (3, 0, 0), (4, 0, 0), (8, 0, 0), (8, 3, 0)], np.int64)
    scores = np.zeros((len(coords), C), f32)
    scores[0, :2], scores[1, :2] = (6.0, -2.0), (1.0, 3.0)   # votes 2 and 1: rows (3, -1) and (1, 3), Y = (2, 1)
    scores[2:6, 0], scores[2:6, 1] = -1.25, 0.5              # what a transfer left in the receivers
    scores[6, :2] = (-0.5, 4.0)
    votes = np.array([2, 1, 0, 0, 0, 0, 1, 0], np.int32)
    labels = np.array([0, 1, 1, 1, 1, 1, 1, -1], np.int64)
    return case_of(GC.scan_of(coords)[:, :3].copy(), scores, votes, labels, coords=coords)


# ---- 4. signed zeros, infinities and NaNs
def negative_zero_case():
    """(0, 0, 0) voted with the row (-0.0, 0.0), (1, 0, 0) voteless: filled, its row is the only live neighbour's, -0.0 kept
    (0.0 + -0.0 would be 0.0)."""
    coords = np.array([(0, 0, 0), (1, 0, 0)], np.int64)
    return case_of(GC.scan_of(coords)[:, :3].copy(), np.array([[-0.0, 0.0], [1.0, 2.0]], f32), np.array([3, 0], np.int32),
                   coords=coords)


def nonfinite_case(C=3):
    """A 3 x 3 x 1 block of voted voxels; the centre's second point holds an inf in column 0 and a NaN in column 1."""
    rs = np.random.RandomState(41)
    voxels = [(x, y, 0) for y in range(3) for x in range(3)]
    coords = np.array(voxels + [(1, 1, 0)], np.int64)
    scores, votes = voted(rs, len(coords), C)
    scores[-1, 0], scores[-1, 1] = np.inf, np.nan
    return case_of(GC.scan_of(coords)[:, :3].copy(), scores, votes, coords=coords)


# ---- 5. colour: two slabs that touch, and a voxel whose mean is NaN
COLOUR_TOL = 0.5


def slabs_case(C=2):
    """Two 4 x 4 slabs, z = 0 with colour 0.25 and logits (+1, -1), z = 1 with colour 1.0 and logits (-1, +1), two points a
    voxel; one voxel of the upper slab holds a NaN colour.  With COLOUR_TOL no edge crosses the slabs and the NaN voxel
    has no neighbour; without it every voxel has neighbours in both."""
    rs = np.random.RandomState(51)
    voxels = np.array([(x, y, z) for z in range(2) for y in range(4) for x in range(4)], np.int64)
    coords = np.repeat(voxels, 2, 0)
    z = coords[:, 2]
    colours = np.where(z[:, None] == 0, 0.25, 1.0).astype(f32).repeat(3, 1)
    nan_voxel = (2, 1, 1)
    colours[(coords == nan_voxel).all(1), 1] = np.nan
    votes = rs.randint(1, 4, len(coords)).astype(np.int32)
    sign = np.where(z == 0, 1.0, -1.0)
    scores = np.zeros((len(coords), C), f32)
    scores[:, 0], scores[:, 1] = sign * votes, -sign * votes
    scores += (rs.randint(-2, 3, scores.shape) / 8.0 * votes[:, None]).astype(f32)
    perm = rs.permutation(len(coords))
    frac = rs.randint(1, 8, coords.shape) / 8.0
    return case_of(GC.scan_of(coords[perm], frac[perm], colours[perm]), scores[perm], votes[perm], coords=coords[perm],
                   nan_voxel=nan_voxel)


# ---- 6. consecutive keys across a row end and a slab end (scene_grow_cases.wrap_case)
def wrap_case(C=3):
    scan, coords = GC.wrap_case()
    scores, votes = voted(np.random.RandomState(61), len(scan), C)
    return case_of(scan[:, :3].copy(), scores, votes, coords=coords)


# ---- 7. random occupancy, colours, invalid points, receivers
def random_case(seed, C=5, grid=(8, 12, 12)):
    """scene_grow_cases.random_case with invalid points; a fifth of the points voteless, half of those with a receiver's
    label and scores."""
    scan, coords = GC.random_case(seed, grid, voxel=VOX)
    scan = GC.with_invalid(scan, seed + 1)
    rs = np.random.RandomState(seed + 2)
    scores, votes = voted(rs, len(scan), C)
    voteless = rs.rand(len(scan)) < 0.2
    votes[voteless] = 0
    labels = labels_of(scores, votes)
    receivers = voteless & (rs.rand(len(scan)) < 0.5)
    scores[voteless & ~receivers] = 0
    labels[receivers] = rs.randint(0, C, int(receivers.sum()))
    return case_of(scan, scores, votes, labels, coords=coords)


def many_points_case(seed=23, C=3, copies=88):
    """random_case's scan `copies` times over, every copy with votes and scores of its own: more points (88 x 3303) than
    the 1024 workgroups of the spread kernel hold in one round of 256, and voxels of up to 864 contributors."""
    base = random_case(seed, C, grid=(8, 12, 12))
    rs = np.random.RandomState(seed + 5)
    n = len(base["scan"])
    scores, votes = voted(rs, n * copies, C)
    voteless = rs.rand(n * copies) < 0.2
    votes[voteless] = 0
    scores[voteless] = 0
    return case_of(np.tile(base["scan"], (copies, 1)), scores, votes, coords=np.tile(base["coords"], (copies, 1)))


# ---- 8. the room of S7: two half-spaces, a share of the voxels flipped, a share stripped of their votes
ROOM = (16, 16, 8)


def room_case(flip=0.15, strip=0.0, seed=3, points_per_voxel=1):
    """A full 16 x 16 x 8 grid, class 0 for x < 8 and class 1 beyond, logits (+1, -1) and (-1, +1), one vote a point; `flip`
    of the voxels carry the other class's logits, `strip` of them no vote at all.  -> the case with truth (M,) int64, the
    true class of every point, and wrong (M,) bool, the flipped ones."""
    rs = np.random.RandomState(seed)
    nx, ny, nz = ROOM
    iz, iy, ix = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    voxels = np.stack([ix.ravel(), iy.ravel(), iz.ravel()], 1)
    truth_v = (voxels[:, 0] >= nx // 2).astype(np.int64)
    flipped = rs.rand(len(voxels)) < flip
    stripped = rs.rand(len(voxels)) < strip
    coords = np.repeat(voxels, points_per_voxel, 0)
    rep = lambda a: np.repeat(a, points_per_voxel, 0)
    seen = np.where(rep(flipped), 1 - rep(truth_v), rep(truth_v))
    scores = np.where(seen[:, None] == np.arange(2)[None, :], 1.0, -1.0).astype(f32)
    votes = np.where(rep(stripped), 0, 1).astype(np.int32)
    scores[votes == 0] = 0
    perm = rs.permutation(len(coords))
    return case_of(GC.scan_of(coords[perm])[:, :3].copy(), scores[perm], votes[perm], coords=coords[perm], truth=rep(truth_v)[perm],
                   wrong=rep(flipped)[perm], stripped=rep(stripped)[perm])
