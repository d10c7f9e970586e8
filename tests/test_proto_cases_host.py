"""The claims of tests/proto_cases.py held to the oracle (O.fps, O.get_multiple_prototypes, O.fps_sample_count) -- no GPU.
What tests/test_gpu_proto_edges.py asks of r3d_head_prototypes_batched depends on its inputs really reaching the edges the
table names: exact list lengths, k or k + 1 samples, ties between candidates of different workgroups and between seeds of
different tiles, FPS running out of distinct rows.  These are conditions on the inputs, not measurements: a seed that misses
one is replaced in the table until the oracle alone meets it."""
import numpy as np
import pytest
import torch

import proto_cases as C
from oracle import r3d_oracle as O

NAMES = [c.name for c in C.TABLE]
LATTICE = [c.name for c in C.TABLE if c.kind in ("lattice", "collapse")]


def test_the_table_names_every_edge_it_promises():
    by = C.BY_NAME
    assert {by[n].D for n in NAMES if n.startswith("D ")} | {by["A lattice"].D} == {5, 64, 65, 128, 129, 192, 193, 256}
    assert {by[n].k for n in NAMES if n.startswith("C ")} == {1, 15, 16, 17, 31, 32, 33, 127}
    assert max(c.k for c in C.TABLE) + 1 == C.HP_MAXK
    assert {c.kind for c in C.TABLE} == {"lattice", "gauss", "collapse"}
    assert any(c.n_way > 3 for c in C.TABLE), "two label planes"
    assert by["F keep"].keep is not None and by["F none"].keep is None and by["F none"].counts == by["F keep"].counts
    for c in C.TABLE:
        assert c.edge and c.k < C.HP_MAXK and 1 <= c.D <= 256


@pytest.mark.parametrize("name", NAMES)
def test_list_lengths_are_the_stated_ones(name):
    """Every segment holds exactly the stated number of points (under shot_keep: of its kept shots; the background is
    untouched), no segment is empty, and the lists are torch.nonzero's."""
    c = C.BY_NAME[name]
    S = c.n_way * c.k_shot
    for e, ep in enumerate(C.episodes(name)):
        assert ep.feat.shape == (S * c.N + C.NQ, c.D) and ep.feat.dtype == torch.float32
        per_shot = ep.y.sum(2)
        assert per_shot.sum(1).tolist() == list(c.counts[e])
        assert len(ep.segs[0]) == S * c.N - sum(c.counts[e])
        assert torch.equal(ep.segs[0], torch.nonzero(ep.y.reshape(-1) == 0).squeeze(1))
        for w in range(c.n_way):
            kept = per_shot[w] if ep.keep is None else per_shot[w] * ep.keep[w]
            assert len(ep.segs[1 + w]) == int(kept.sum()) > 0
            assert ep.keep is None or int(ep.keep[w].sum()) > 0, "never all shots of a way (the detector restores them)"
            flat = ep.y[w].reshape(-1)
            assert (flat[ep.segs[1 + w] - w * c.k_shot * c.N] == 1).all()
            if c.last == "fg":
                assert int(ep.segs[1 + w][-1]) == (w + 1) * c.k_shot * c.N - 1
        if c.last == "bg":
            assert int(ep.segs[0][-1]) == S * c.N - 1
    if c.keep is not None:
        drops = [int((1 - torch.tensor(k)).sum()) for k in c.keep]
        assert drops[0] > 0 and drops[1] == 0 and drops[2] > 0  # (episode 1 keeps every shot)
        assert any(len(ep.segs[1]) < int(ep.y[0].sum()) for ep in C.episodes(name))


def test_sample_counts_k_or_k_plus_1():
    """torch_cluster's float-rounded count at the sizes the table relies on."""
    f = O.fps_sample_count
    assert f(300, 40) == 41 and f(41, 40) == 40 and f(255, 40) == f(256, 40) == f(257, 40) == 40
    assert f(511, 40) == f(512, 40) == f(513, 40) == 40
    assert f(19, 15) == 16 and f(51, 31) == 32 and f(150, 127) == 128 == C.HP_MAXK
    for k in (1, 16, 32, 33):  # never k + 1 below 2600 points
        assert all(f(n, k) == k for n in range(k + 1, 2600)), k
    assert [n for n in range(18, 2600) if f(n, 17) == 18][0] == 1033  # k = 17: first at 1033 points, beyond case C
    for k, n in C.C_SPECIAL.items():
        assert [i for i in range(k + 1, n + 1) if f(i, k) == k + 1] == [n], "the smallest segment that draws k + 1"


def test_geometry_edges_of_a_and_b():
    a = C.reference("A lattice")
    assert [[r.count for r in ep[1:]] for ep in a] == [[255, 256, 257], [511, 512, 513], [300, 41, 40]]
    assert [r.kseg for r in a[2][1:]] == [41, 40, 0] and [r.m for r in a[2][1:]] == [41, 40, 40]
    for kind in ("lattice", "gauss"):
        t, ch = C.episodes("B tile " + kind), C.episodes("B chunk " + kind)
        cap = 2 * 640
        assert cap > C.COMPACT_TILE and 4 * 640 > C.COMPACT_TILE
        assert [len(ep.segs[0]) for ep in t] == [1023, 1024, 1025] and [len(ep.segs[0]) for ep in ch] == [2047, 2048, 2049]
        for e, w in ((0, 0), (1, 0), (2, 1)):  # the 1025-point list: both shots, entries on both sides of element 1024
            ids = t[e].segs[1 + w] - w * cap
            assert len(ids) == 1025 and t[e].y[w].sum(1).tolist() == [513, 512]
            assert int((ids < C.COMPACT_TILE).sum()) > 0 and int(ids[-1]) == cap - 1
        # the background of 2049 points: its last position is alone in the second chunk of the cluster sums
        assert 2049 - C.CM_CHUNK == 1


@pytest.mark.parametrize("name", NAMES)
def test_case_c_and_every_case_outcomes(name):
    """m, kseg and the identity rule per segment; no empty cluster, no NaN prototype; the offsets fit the node buffer."""
    c = C.BY_NAME[name]
    for e, segs in enumerate(C.reference(name)):
        for s, r in enumerate(segs):
            assert r.count > 0 and r.m >= 1 and int(r.counts.min()) >= 1
            assert torch.isfinite(r.mean64).all() and torch.isfinite(r.mean32).all(), "a NaN prototype"
            if r.count <= c.k:
                assert r.kseg == 0 and r.m == r.count and torch.equal(r.assign, torch.arange(r.count))
            else:
                assert r.kseg in (c.k, c.k + 1) and r.kseg == O.fps_sample_count(r.count, c.k) and len(r.sel) == r.kseg
                assert r.m == len(r.seeds) <= r.kseg and int(r.sel[0]) == 0
                if c.kind != "collapse" or s > 1:
                    assert r.m == r.kseg, "a repeated selection outside case E"
            if c.kind != "gauss":  # integer rows: every cluster sum is an exact integer below 2^24 in any order
                f = C.episodes(name)[e].feat[r.ids]
                assert torch.equal(f, f.round()) and float(f.min()) >= 0 and float(f.max()) * r.count < 2 ** 24
        assert sum(r.m for r in segs) <= (c.n_way + 1) * (c.k + 1)
    if name.startswith("C "):
        ref = C.reference(name)
        want = c.k + 1 if c.k in C.C_SPECIAL else c.k
        assert ref[0][1].kseg == want and ref[0][1].count == C.C_SPECIAL.get(c.k, 2 * c.k + 3)
        assert ref[0][2].count == c.k + 1 and ref[0][2].kseg == c.k                      # the smallest sampled segment
        assert [r.kseg for r in ref[1][1:]] == [0, 0] and ref[1][1].count == c.k          # identity at n == k and below
        if c.k in C.C_SPECIAL:
            assert want % C.AS_TILE == 0, "k + 1 seeds fill their tiles exactly"


@pytest.mark.parametrize("name", LATTICE)
def test_lattice_cases_tie_where_the_kernels_merge(name):
    """Every lattice case whose geometry allows it has at least one FPS round whose tied maxima lie in two different
    256-point blocks (the persistent kernel's 64-bit key / cand_better decide) and at least one point whose nearest seeds
    tie across two 16-seed tiles (the 64-bit atomicMin decides); the numpy replays agree with the oracle on every decision."""
    c = C.BY_NAME[name]
    eps, ref = C.episodes(name), C.reference(name)
    fps_cross = seed_cross = fps_tied = seed_tied = 0
    can_fps = can_seed = False
    for e, segs in enumerate(ref):
        for r in segs:
            f = eps[e].feat[r.ids]
            if r.kseg:
                same, tied, cross = C.fps_ties(f, r.sel)
                assert same, "the replay of FPS differs from the oracle"
                fps_tied, fps_cross = fps_tied + tied, fps_cross + cross
                can_fps |= r.count > C.HP_BLOCK and r.kseg > 2
            if not r.kseg:
                continue  # identity: no distance is taken, a point is its own prototype even beside a duplicate row
            same, tied, cross = C.assign_ties(f, r.seeds, r.assign)
            assert same, "the replayed first minimum differs from the oracle's assignment"
            seed_tied, seed_cross = seed_tied + tied, seed_cross + cross
            can_seed |= r.m > C.AS_TILE
    print("PC| %-12s FPS rounds tied %d (across 256-blocks %d)  points tied %d (across 16-seed tiles %d)"
          % (name, fps_tied, fps_cross, seed_tied, seed_cross))
    assert fps_cross >= 1 or not can_fps
    assert seed_cross >= 1 or not can_seed
    if name in ("A lattice", "B tile lattice", "B chunk lattice", "E collapse", "F keep", "F none") or name.startswith("D "):
        assert can_fps and can_seed
    if name.startswith("C ") and c.k >= 17:
        assert can_seed


def test_collapse_selects_positions_twice():
    """E: in the background and in way 0 of every episode FPS runs out of distinct rows: kseg selections, fewer distinct
    positions, m = the number of distinct rows; the segments behind them start at shifted node rows."""
    c = C.BY_NAME["E collapse"]
    for e, (ep, segs) in enumerate(zip(C.episodes(c.name), C.reference(c.name))):
        for s in (0, 1):
            r = segs[s]
            distinct = len(np.unique(ep.feat[r.ids].numpy(), axis=0))
            assert distinct == c.distinct[e] < c.k
            assert r.kseg >= c.k and r.m == distinct < r.kseg
            assert len(set(r.sel.tolist())) == distinct, "FPS visits every distinct row before it repeats one"
            assert r.sel.tolist().count(0) == r.kseg - distinct + 1, "out of rows, every distance is zero: position 0 again"
        assert segs[0].m + segs[1].m < 2 * c.k  # HD_SEG_POFF of way 1 is not 2 k
        assert segs[2].m == min(segs[2].count, segs[2].kseg or segs[2].count)
