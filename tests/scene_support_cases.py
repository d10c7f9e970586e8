"""Seeded labels for the fit_scene tests on scene_cases.small_scan() and medium_scan(), and their numpy restatements
(tests/scene_support_ref.py), built once per session.  n_way = 2, k_shot = 2; way 1 is class 7, way 2 class -4."""
import numpy as np

import scene_cases as SC
from scene_support_ref import RefSupport

f32 = np.float32
CLASSES = (7, -4)
A, B = CLASSES
K_SHOT, MIN_RATIO, MIN_FG = 2, 0.05, 10
NEGATIVE, BIG = -9, 2 ** 32 + 7   # class ids of no way; BIG cut to 32 bits would read as class 7
BIG_AS_INT32 = 2 ** 31 - 1        # what stands for BIG in the int32 copy of the labels

# per r: the recipe below, in order.  ("paint", block, class, count or "thr" / "thr+1", cells or None): label 0 members of the
# block's cloud (inside `cells`, if given) get the class until the cloud holds `count` of it; then the cloud's points are
# frozen: no later step labels them.  ("fill", block, class): every point of the block.  ("off", block, class): the points
# of the block that are NOT members of its cloud (a count over the whole block would see them).  short: the step the
# second label set leaves out.
RECIPES = {
    1: dict(steps=[("paint", 0, A, 80, None), ("paint", 0, B, 50, None), ("paint", 4, A, 60, None), ("paint", 9, A, 60, None),
                   ("paint", 10, A, "thr+1", None), ("paint", 12, A, "thr", None), ("paint", 16, B, 30, None),
                   ("fill", 22, B), ("off", 4, A)],
            chosen=[[0, 4], [0, 16]], tie=(A, 4, 9), at_thr=(A, 12), above_thr=(A, 10), exact=B, dropped_full=(B, 22),
            short=("paint", 16, B)),
    2: dict(steps=[("paint", 0, A, 80, None), ("paint", 0, B, 50, None), ("fill", 1, B),
                   ("paint", 14, A, "thr+1", None), ("paint", 11, A, "thr", [(2, 2), (2, 3)]),
                   ("paint", 5, A, 60, None), ("paint", 9, A, 60, None), ("off", 5, A)],
            chosen=[[0, 5], [0, 2]], tie=(A, 5, 9), at_thr=(A, 11), above_thr=(A, 14), exact=B, dropped_full=(B, 1),
            short=("fill", 1, B)),
}

_cache = {}


def _members(plan, b):
    lst = plan.block_list[b]
    return lst[0::-(-len(lst) // plan.N)]


def _thr(plan, b):
    return max(int(np.floor(f32(len(_members(plan, b))) * f32(MIN_RATIO))), MIN_FG)


def _labels_for(r, short):
    plan = SC.small_plan(r)
    rs = np.random.RandomState(100 + r)
    labels = np.zeros(plan.M, np.int64)
    frozen = {}  # point -> the block whose cloud froze it
    rec = RECIPES[r]
    for step in rec["steps"]:
        kind, b, cls = step[:3]
        if short and step[:3] == rec["short"]:  # the short label set: way 2 loses one of its two eligible blocks
            continue
        if kind == "fill":
            labels[plan.block_list[b]] = cls
        elif kind == "off":
            members = set(_members(plan, b))
            for p in plan.block_list[b]:
                if p not in members and p not in frozen and labels[p] == 0:
                    labels[p] = cls
        else:
            count, cells = step[3], step[4]
            want = {"thr": _thr(plan, b), "thr+1": _thr(plan, b) + 1}.get(count, count)
            members = _members(plan, b)
            keys = None if cells is None else {cy * plan.ncx + cx for cx, cy in cells}
            need = want - sum(1 for p in members if labels[p] == cls)
            pool = np.array([p for p in members if labels[p] == 0 and frozen.get(p, b) == b and (keys is None or plan.key[p] in keys)])
            assert 0 <= need <= len(pool), (r, step, need, len(pool))
            labels[pool[rs.permutation(len(pool))[:need]]] = cls
            for p in members:
                frozen.setdefault(p, b)
    free = np.array([p for p in range(plan.M) if labels[p] == 0 and plan.valid[p]])
    odd = free[rs.permutation(len(free))[:80]]
    labels[odd[:40]], labels[odd[40:]] = NEGATIVE, BIG
    labels[~plan.valid] = A  # class labels on the three non-finite points: never read
    return labels


def small_labels(r, short=False):
    """(M,) int64 labels for the small scan at overlap r; short: way 2 is left with k_shot - 1 eligible blocks."""
    key = ("labels", r, short)
    if key not in _cache:
        _cache[key] = _labels_for(r, short)
        if not short:
            _check_promises(r, _cache[key])
    return _cache[key]


def as_int32(labels):
    """The int32 copy: BIG, which int32 cannot hold, becomes another id of no way."""
    return np.where(labels == BIG, BIG_AS_INT32, labels).astype(np.int32)


def small_support(r, short=False):
    key = ("support", r, short)
    if key not in _cache:
        _cache[key] = RefSupport(SC.small_plan(r), small_labels(r, short), CLASSES, K_SHOT, MIN_RATIO, MIN_FG)
    return _cache[key]


def _check_promises(r, labels):
    """The recipe's promises, checked on the restatement."""
    plan, rec = SC.small_plan(r), RECIPES[r]
    ref = RefSupport(plan, labels, CLASSES, K_SHOT, MIN_RATIO, MIN_FG)
    way = {A: 0, B: 1}
    blocks, fgs = ref.pick()
    assert blocks.tolist() == rec["chosen"], (r, blocks.tolist(), ref.fg.tolist(), ref.thr.tolist())
    cls, b = rec["at_thr"]   # fg == thr: not eligible
    assert plan.kept[b] and ref.fg[b, way[cls]] == ref.thr[b] and b not in ref.eligible[way[cls]]
    cls, b = rec["above_thr"]  # fg == thr + 1: eligible
    assert ref.fg[b, way[cls]] == ref.thr[b] + 1 and b in ref.eligible[way[cls]]
    cls, lo, hi = rec["tie"]  # two eligible blocks with equal fg: the lower id is chosen, the higher is not
    w = way[cls]
    assert lo < hi and ref.fg[lo, w] == ref.fg[hi, w] and lo in ref.eligible[w] and hi in ref.eligible[w]
    assert lo in blocks[w] and hi not in blocks[w] and ref.n_eligible[w] > K_SHOT
    assert ref.n_eligible[way[rec["exact"]]] == K_SHOT  # a way with exactly k_shot eligible blocks
    assert set(blocks[0]) & set(blocks[1])  # a block chosen by two ways
    assert any(ref.length[b] < plan.N for b in blocks.reshape(-1))  # a chosen block whose mask wraps with the slots
    cls, b = rec["dropped_full"]  # a dropped block full of a class: more of it than any chosen block, never chosen
    assert not plan.kept[b] and (labels[plan.block_list[b]] == cls).all() and b not in blocks
    assert len(plan.block_list[b]) > ref.thr.max() and len(plan.block_list[b]) > MIN_FG and (ref.fg[b] == 0).all()
    assert (labels[~plan.valid] == A).all() and int((~plan.valid).sum()) == 3
    assert (labels == NEGATIVE).sum() == 40 and (labels == BIG).sum() == 40 and BIG > 2 ** 31 and NEGATIVE not in CLASSES
    # a count over the whole block, or over the wrapped slots, would differ from fg for a chosen block
    b = rec["chosen"][0][1]
    assert (labels[plan.block_list[b]] == A).sum() > ref.fg[b, 0]
    short = RefSupport(plan, small_labels(r, short=True), CLASSES, K_SHOT, MIN_RATIO, MIN_FG)
    assert short.n_eligible[way[rec["exact"]]] == K_SHOT - 1 and short.n_eligible[way[A]] >= K_SHOT


def medium_labels():
    """(M,) int64 labels for the medium scan: every id of small_labels, drawn point by point."""
    if "medium" not in _cache:
        rs = np.random.RandomState(21)
        ids = np.array([0, A, B, NEGATIVE, BIG], np.int64)
        _cache["medium"] = ids[rs.choice(5, SC.MEDIUM["M"], p=[0.5, 0.25, 0.15, 0.05, 0.05])]
    return _cache["medium"]


def medium_support(r=2):
    key = ("medium_support", r)
    if key not in _cache:
        _cache[key] = RefSupport(SC.medium_plan(r), medium_labels(), CLASSES, K_SHOT, MIN_RATIO, MIN_FG)
    return _cache[key]
