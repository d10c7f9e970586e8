"""The inputs of tests/test_gpu_proto_edges.py -- r3d_head_prototypes_batched (csrc/head_proto.hip) at its block, tile and
chunk edges and under ties -- in plain numpy / torch, each case with the edge it claims; tests/test_proto_cases_host.py
holds every claim to the oracle (O.fps, O.get_multiple_prototypes, O.fps_sample_count) without a GPU.

Feature generators.  lattice: integer-valued rows, so FPS distances are exact integers and equal distances are common; the
assignment distances ((x - s) + 1e-6 per channel) tie as well.  few_distinct: n rows drawn from fewer distinct rows than
FPS is asked to sample, so FPS runs out of rows, selects a position twice and the unique step gives m < kseg (blocks
sampled with replacement).  gauss: randn * 0.1 with a hub row and duplicated rows (head_ref.graph_nodes).

Every case is a batch of THREE episodes of one geometry with different masks and features; counts[e][w] = foreground
points of way w in episode e (forced exactly), the background is the rest."""
import functools
from collections import namedtuple

import numpy as np
import torch

from oracle import r3d_oracle as O

HP_BLOCK, AS_TILE, CM_CHUNK, COMPACT_TILE, HP_MAXK = 256, 16, 2048, 1024, 128  # csrc/head_proto.hip
NQ = 37  # query rows behind every episode's support rows (37 D is no multiple of the append kernel's 256 threads)


# ----------------------------------------------------------------------------------------------------------------------
# features
# ----------------------------------------------------------------------------------------------------------------------
def lattice(n, D, levels=2, seed=0):
    """(n, D) fp32 rows in {0, .., levels - 1}^D."""
    return torch.from_numpy(np.random.RandomState(seed).randint(0, levels, (n, D)).astype(np.float32))


def few_distinct(n, D, distinct, seed=0, levels=2):
    """(n, D) fp32: n rows drawn (with replacement) from `distinct` different lattice rows, every one drawn at least once."""
    rs = np.random.RandomState(seed)
    base = np.unique(rs.randint(0, levels, (4 * distinct + 8, D)), axis=0)
    assert len(base) >= distinct and n >= distinct
    base = base[rs.permutation(len(base))[:distinct]].astype(np.float32)
    pick = np.concatenate((np.arange(distinct), rs.randint(0, distinct, n - distinct)))
    return torch.from_numpy(base[pick[rs.permutation(n)]])


def gauss(n, D, seed=0):
    """(n, D) fp32 randn * 0.1 (the existing head tests) with, where they fit, the hub (row 5 = the mean of all rows) and
    the duplicates (rows 3 and n / 2 + 7; rows n / 2 + 8 and n / 2 + 9) of head_ref.graph_nodes."""
    x = (np.random.RandomState(seed).randn(n, D) * 0.1).astype(np.float32)
    if n > 5:
        x[5] = x.mean(0)
    h = n // 2
    if h + 9 < n and h + 7 > 5:
        x[h + 7] = x[3]
        x[h + 8] = x[h + 9]
    return torch.from_numpy(x)


# ----------------------------------------------------------------------------------------------------------------------
# masks
# ----------------------------------------------------------------------------------------------------------------------
def masks(n_way, k_shot, N, seg_counts, seed, last=None):
    """support_y (n_way, k_shot, N) int64 whose way w has seg_counts[w] foreground points, split over its shots.
    last = "fg": the last row of every way's capacity (row N - 1 of its last shot) is foreground -- the last listed point of
    the segment sits in the last row it could; last = "bg": that row is background in every way, so the background's last
    listed point is the last support row; None: wherever the permutation puts them."""
    rs = np.random.RandomState(seed)
    y = torch.zeros(n_way, k_shot, N, dtype=torch.int64)
    for w, c in enumerate(seg_counts):
        per = [c // k_shot + (1 if k < c % k_shot else 0) for k in range(k_shot)]
        for k in range(k_shot):
            if last is None or k < k_shot - 1:
                rows = rs.permutation(N)[:per[k]]
            elif last == "fg":
                assert per[k] >= 1
                rows = np.concatenate((rs.permutation(N - 1)[:per[k] - 1], [N - 1]))
            else:
                assert last == "bg" and per[k] <= N - 1
                rows = rs.permutation(N - 1)[:per[k]]
            y[w, k, torch.from_numpy(np.asarray(rows, dtype=np.int64))] = 1
    return y


def segment_ids(y, keep=None):
    """Per segment (background, way 0, ...) the support rows the reference lists, ascending (torch.nonzero order).  keep
    (n_way, k_shot) of 0 / 1: a dropped shot's foreground leaves its way's list; the background list is untouched."""
    n_way, k_shot, N = y.shape
    segs = [torch.nonzero(y.reshape(-1) == 0).squeeze(1)]
    for w in range(n_way):
        fg = y[w] == 1
        if keep is not None:
            fg = fg & (torch.as_tensor(keep)[w].reshape(k_shot, 1) != 0)
        segs.append(torch.nonzero(fg.reshape(-1)).squeeze(1) + w * k_shot * N)
    return segs


# ----------------------------------------------------------------------------------------------------------------------
# the table
# ----------------------------------------------------------------------------------------------------------------------
# kind: "lattice" | "gauss" | "collapse" (lattice, the rows of the background and of way 0 replaced by few_distinct draws from
# distinct[e] rows).  keep: None, or per episode (n_way, k_shot) of 0 / 1.  last: see masks().
Case = namedtuple("Case", "name edge n_way k_shot N k D kind counts keep levels distinct last seed")


def _case(name, edge, n_way, k_shot, N, k, D, kind, counts, keep=None, levels=2, distinct=None, last=None, seed=0):
    assert len(counts) == 3 and all(len(c) == n_way for c in counts)
    return Case(name, edge, n_way, k_shot, N, k, D, kind, tuple(tuple(c) for c in counts), keep, levels, distinct, last, seed)


# A: n_way 3, k_shot 1, N 768, k 40.  Episode 0: segments on both sides of one workgroup; episode 1: of two; episode 2: 300
# points draw 41 samples (k + 1) over two workgroups, 41 points are k + 1 points (the smallest sampled segment), 40 are identity.
A_COUNTS = ((255, 256, 257), (511, 512, 513), (300, 41, 40))
A_EDGE = "the 256-point workgroup (HP_BLOCK) of gather, FPS and assign: 255 / 256 / 257 and 511 / 512 / 513 points; 300 -> 41 " \
         "samples over two workgroups, 41 = k + 1 points, 40 = identity"
# B: n_way 2, k_shot 2, N 640: S N = 2560 support rows, 1280 per way (more than one 1024-element tile of the compaction).
B_TILE = ((1025, 512), (1025, 511), (510, 1025))    # background 1023, 1024, 1025
B_CHUNK = ((257, 256), (256, 256), (255, 256))      # background 2047, 2048, 2049
# C: k on both sides of one and two 16-seed tiles, one seed, and HP_MAXK - 1.  n_way 2, k_shot 1, N 320 (S N = 640).
# special[k] = the smallest segment that draws k + 1 samples (O.fps_sample_count); k = 1, 16, 32, 33 never draw k + 1 below
# 2600 points and k = 17 first at 1033 points -- those cases hold k samples everywhere.
C_SPECIAL = {15: 19, 31: 51, 127: 150}
C_KS = (1, 15, 16, 17, 31, 32, 33, 127)
D_WIDTHS = (5, 65, 128, 129, 192, 193, 256)         # (64: case "A lattice")


def _c_counts(k):
    s = C_SPECIAL.get(k, 2 * k + 3)
    # episode 0: the k + 1 draw (or an ordinary segment) and the smallest sampled segment; 1: identity on both sides of k and
    # one point fewer; 2: two ordinary segments, the background smaller
    return ((s, k + 1), (k, max(1, k - 1)), (s + 7, min(3 * k + 2, 300) if k > 1 else 5))


def _table():
    t = [_case("A lattice", A_EDGE, 3, 1, 768, 40, 64, "lattice", A_COUNTS, last="fg", seed=11),
         _case("A gauss", A_EDGE + "; cluster means against float64", 3, 1, 768, 40, 192, "gauss", A_COUNTS, last="fg", seed=12)]
    for kind, seed in (("lattice", 21), ("gauss", 22)):
        t.append(_case("B tile " + kind, "the 1024-element tile of r3d_head_compact_kernel: background lists of 1023 / 1024 / 1025 points "
                       "and a foreground list of 1025 points spread over both shots, its last point in the last row of its capacity",
                       2, 2, 640, 40, 64, kind, B_TILE, last="fg", seed=seed))
        t.append(_case("B chunk " + kind, "the 2048-position chunk (CM_CHUNK) of r3d_cluster_partial_kernel: background lists of 2047 / "
                       "2048 / 2049 points, the last one in the last support row", 2, 2, 640, 40, 64, kind, B_CHUNK, last="bg",
                       seed=seed + 2))
    for k in C_KS:
        what = "k = %d: %s" % (k, {1: "one seed, one round", 15: "19 points draw 16 seeds: exactly one 16-seed tile (AS_TILE)",
                                   16: "one full tile of seeds, never k + 1", 17: "one seed in the second tile",
                                   31: "51 points draw 32 seeds: exactly two tiles", 32: "two full tiles, never k + 1",
                                   33: "one seed in the third tile",
                                   127: "150 points draw 128 samples = HP_MAXK: the bitonic sort of finalize without a sentinel "
                                        "slot, eight seed tiles"}[k])
        t.append(_case("C k=%d" % k, what, 2, 1, 320, k, 132 if k == 127 else 20, "lattice", _c_counts(k), seed=30 + k))
    for D in D_WIDTHS:
        t.append(_case("D D=%d" % D, "feature width %d on the geometry of A: %s" % (
            D, "FULL = true" if D in (128, 192, 256) else "FULL = false, channel clamps of gather and cluster, the c + 8 <= D "
            "remainder of assign"), 3, 1, 768, 40, D, "lattice", A_COUNTS, levels=16 if D == 5 else 2, last="fg", seed=40 + D))
    t.append(_case("E collapse", "FPS runs out of distinct rows in the background AND in way 0 (30, 12 and 1 distinct rows): a "
                   "position is selected twice, m < kseg, every later segment's HD_SEG_POFF shifts", 2, 1, 768, 40, 64, "collapse",
                   ((600, 300), (300, 41), (257, 513)), distinct=(30, 12, 1), seed=50))
    keep = (((1, 0, 1), (0, 1, 0)), ((1, 1, 1), (1, 1, 1)), ((0, 1, 1), (1, 0, 0)))
    f_counts = ((300, 130), (90, 257), (126, 200))
    t.append(_case("F keep", "shot_keep drops shots from the foreground lists (never all shots of a way), the background list is "
                   "untouched; episode 1 keeps every shot", 2, 3, 256, 40, 64, "lattice", f_counts, keep=keep, seed=60))
    t.append(_case("F none", "the masks of 'F keep' without a shot_keep array", 2, 3, 256, 40, 64, "lattice", f_counts, seed=60))
    t.append(_case("P planes", "n_way 5: the one-hot label rows in two planes of four columns; segments of 3, 10, 11 and 40 points "
                   "at k = 10", 5, 1, 128, 10, 64, "lattice", ((3, 10, 11, 40, 100), (40, 11, 10, 3, 60), (12, 12, 12, 12, 12)), seed=70))
    return t


TABLE = _table()
BY_NAME = {c.name: c for c in TABLE}
assert len(BY_NAME) == len(TABLE)

Episode = namedtuple("Episode", "y feat keep segs")  # y (n_way, k_shot, N) int64; feat (S N + NQ, D) fp32; keep or None; ids


@functools.lru_cache(maxsize=None)
def episodes(name):
    """The three episodes of a case (built once, never changed)."""
    c = BY_NAME[name]
    S = c.n_way * c.k_shot
    out = []
    for e in range(3):
        y = masks(c.n_way, c.k_shot, c.N, c.counts[e], 100 * c.seed + e, c.last)
        keep = None if c.keep is None else torch.tensor(c.keep[e], dtype=torch.int64)
        segs = segment_ids(y, keep)
        rows, seed = S * c.N + NQ, 1000 * c.seed + 10 * e
        if c.kind == "gauss":
            feat = gauss(rows, c.D, seed)
        else:
            feat = lattice(rows, c.D, c.levels, seed)
            if c.kind == "collapse":
                for s in (0, 1):
                    feat[segs[s]] = few_distinct(len(segs[s]), c.D, c.distinct[e], seed + 1 + s, c.levels)
        out.append(Episode(y, feat, keep, segs))
    return out


# ----------------------------------------------------------------------------------------------------------------------
# the oracle's decisions
# ----------------------------------------------------------------------------------------------------------------------
SegRef = namedtuple("SegRef", "ids count kseg sel seeds m assign counts mean64 mean32")


def segment_reference(f, k, ids=None):
    """One segment's rows f (n, D) fp32 -> the oracle's decisions: kseg samples in FPS order (kseg = 0: identity, n <= k),
    the sorted unique seeds (positions), m, assignments, cluster sizes, and the cluster means in float64 (and the oracle's
    fp32 means)."""
    n = f.shape[0]
    mean32, asg, m, seed_rows = O.get_multiple_prototypes(f, k)
    if n > k:
        kseg = O.fps_sample_count(n, k)
        sel = O.fps(f, kseg)
        seeds = torch.unique(sel)
        assert torch.equal(f[seeds], seed_rows)
    else:
        kseg, sel, seeds = 0, torch.zeros(0, dtype=torch.int64), torch.arange(n)
    counts = torch.bincount(asg, minlength=m)
    mean64 = torch.zeros(m, f.shape[1], dtype=torch.float64).index_add(0, asg, f.double()) / counts.double()[:, None]
    return SegRef(ids, n, kseg, sel, seeds, m, asg, counts, mean64, mean32)


@functools.lru_cache(maxsize=None)
def reference(name):
    """[episode][segment] -> SegRef (computed once per case and shared)."""
    c = BY_NAME[name]
    return [[segment_reference(ep.feat[ids], c.k, ids) for ids in ep.segs] for ep in episodes(name)]


# ----------------------------------------------------------------------------------------------------------------------
# ties, replayed in numpy
# ----------------------------------------------------------------------------------------------------------------------
def fps_ties(f, sel):
    """Replay FPS on integer-valued rows (distances exact) -> (replay equals sel, rounds whose maximum is held by more than
    one position, rounds whose tied maxima lie in different 256-point blocks)."""
    x = f.double().numpy()
    sel = sel.numpy()
    md = np.full(len(x), np.inf)
    same, tied, cross = True, 0, 0
    for r in range(len(sel) - 1):
        md = np.minimum(md, ((x - x[sel[r]]) ** 2).sum(1))
        win = np.nonzero(md == md.max())[0]
        same &= bool(win[0] == sel[r + 1])
        tied += len(win) > 1
        cross += len(set((win // HP_BLOCK).tolist())) > 1
    return same, int(tied), int(cross)


def assign_distances(f, seed_rows):
    """(n, m) fp32 distances of the assignment: sqrt of the channel-ascending fmaf chain of ((x - s) + 1e-6)^2, the fma
    emulated in float64 (the product of two fp32 is exact there)."""
    x, s = f.numpy(), seed_rows.numpy()
    acc = np.zeros((x.shape[0], s.shape[0]), np.float32)
    for c in range(x.shape[1]):
        df = ((x[:, None, c] - s[None, :, c]) + np.float32(1e-6)).astype(np.float64)
        acc = (df * df + acc.astype(np.float64)).astype(np.float32)
    return np.sqrt(acc)


def assign_ties(f, seeds, assign):
    """-> (the first minimum of the replayed distances equals `assign` everywhere, points whose minimum is held by more than
    one seed, points whose tied seeds lie in different 16-seed tiles)."""
    d = assign_distances(f, f[seeds])
    tie = d == d.min(1, keepdims=True)
    same = bool((tie.argmax(1) == assign.numpy()).all())
    tiles = np.arange(d.shape[1]) // AS_TILE
    many = tie.sum(1) > 1
    cross = sum(1 for i in np.nonzero(many)[0] if len(set(tiles[tie[i]].tolist())) > 1)
    return same, int(many.sum()), int(cross)
