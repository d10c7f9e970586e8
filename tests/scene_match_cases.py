"""The columns of the match_objects tests (host and GPU): named cases, all small.  A case is a dict of the arguments of
match_objects -- pred, truth (int64; the tests also pass them as int32), optionally pred_labels, truth_labels, iou,
ignore_unannotated."""
import numpy as np

TOP = 2 ** 31 - 2  # the largest legal id
EDGE_SIZES = (1, 63, 64, 65, 2047, 2048, 2049, 4097)


def _shuffled(seed, *columns):
    perm = np.random.RandomState(seed).permutation(len(columns[0]))
    return tuple(np.asarray(c, np.int64)[perm] for c in columns)


def identity_case():
    """pred == truth: 4097 points in 9 objects whose ids are sparse up to 2^31 - 2 (four radix passes); every IoU is 1."""
    ids = np.array([0, 5, 255, 256, 65535, 65536, 2 ** 24, 2 ** 30 + 12345, TOP], np.int64)
    col = ids[np.random.RandomState(1).randint(0, len(ids), 4097)]
    col[:9] = ids  # every object is there
    return dict(pred=col, truth=col.copy())


def split_case():
    """A truth of 300 points cut into preds of 200 and 100: IoUs 2/3 and 1/3, one match at 0.5, none at 0.75."""
    pred, truth = _shuffled(2, [3] * 200 + [9] * 100, [7] * 300)
    return dict(pred=pred, truth=truth)


def merge_case():
    c = split_case()
    return dict(pred=c["truth"], truth=c["pred"])


def tie_case():
    """A pred of 4 points, two in each of two truths of 5 points: both IoUs are 2/7 and the lowest truth row wins."""
    pred, truth = _shuffled(3, [4] * 4 + [-1] * 6, [20, 20, 10, 10] + [20] * 3 + [10] * 3)
    return dict(pred=pred, truth=truth)


def tie_mirror_case():
    c = tie_case()
    return dict(pred=c["truth"], truth=c["pred"])


def singletons_case():
    """4097 points, each its own object on both sides; truth holds a permuted id."""
    M = 4097
    rs = np.random.RandomState(4)
    return dict(pred=np.arange(M, dtype=np.int64) * 3 + 1, truth=rs.permutation(M).astype(np.int64) * 5)


FAN_BEFORE, FAN_TRUTHS = 1900, 300  # pairs in front of the fan's run, and its length: pairs 1900 .. 2199, across 2048


def fan_case():
    """One pred that overlaps 300 truths -- more than a wave, more than a workgroup of 256 -- behind 1900 singleton pairs, so
    that its run of pairs lies across position 2048 and across several multiples of 256.  Truth j of the fan shares 1 .. 5
    points with it and has 0 .. 2 more outside; the greatest IoU (5 of 5 points) comes three times, first at j = 204."""
    pred, truth = [], []
    for i in range(FAN_BEFORE):  # pred ids 0 .. 1899 in front of the fan's 5000; truth ids behind the fan's truths
        pred.append(i)
        truth.append(100000 + i)
    for j in range(FAN_TRUTHS):
        shared, outside = (j * 7) % 5 + 1, (j // 3) % 3
        if j in (204, 250, 299):
            shared, outside = 5, 0
        elif shared == 5:
            outside = 1 + j % 2  # 5 of 6 or 7 points: below the three
        pred += [5000] * shared + [-1] * outside
        truth += [1000 + j] * (shared + outside)
    pred, truth = _shuffled(5, pred, truth)
    return dict(pred=pred, truth=truth)


def fan_mirror_case():
    """The fan transposed: one truth overlaps 300 preds (truth_best through the atomic maximum)."""
    c = fan_case()
    return dict(pred=c["truth"], truth=c["pred"])


def edge_case(M):
    """M points, random sparse ids, about 7 objects per side, a few points in no object."""
    rs = np.random.RandomState(100 + M)
    ids_p = np.array([2, 40, 300, 70000, 2 ** 25, 2 ** 30, TOP], np.int64)
    ids_t = np.array([0, 255, 256, 65536, 2 ** 24 - 1, 2 ** 24, TOP - 1], np.int64)
    pred, truth = ids_p[rs.randint(0, 7, M)], ids_t[rs.randint(0, 7, M)]
    if M > 1:
        pred[rs.rand(M) < 0.1] = -1
        truth[rs.rand(M) < 0.1] = -3
    return dict(pred=pred, truth=truth)


def negatives_case(ignore, pred_all=False, truth_all=False, M=3000):
    """30 % negatives per column, on their own points; or a column that is all negative."""
    rs = np.random.RandomState(6)
    pred, truth = rs.randint(0, 12, M).astype(np.int64) * 1000, rs.randint(0, 9, M).astype(np.int64) * 77
    pred[rs.rand(M) < 0.3] = -1
    truth[rs.rand(M) < 0.3] = -2
    if pred_all:
        pred[:] = -1
    if truth_all:
        truth[:] = -5
    return dict(pred=pred, truth=truth, ignore_unannotated=ignore)


def classes_case():
    """Pred 1 (class 4, 10 points) shares 6 points with truth 50 (class 9: not eligible) and 3 with truth 60 (class 4): the
    next one wins.  Pred 2 (class 9, 8 points) lies in truth 50.  Truth 70 (class 4, 5 points) has no pred.  One object per
    side is mixed: pred 3 and truth 80 (the same 6 points) carry class 2 at their first point and class 7 at another."""
    pred = [1] * 6 + [1] * 3 + [1] + [2] * 8 + [-1] * 4 + [-1] * 5 + [3] * 6
    truth = [50] * 6 + [60] * 3 + [-1] + [50] * 8 + [60] * 4 + [70] * 5 + [80] * 6
    pred_labels = [4] * 10 + [9] * 8 + [0] * 9 + [2, 2, 7, 2, 2, 2]
    truth_labels = [9] * 6 + [4] * 3 + [0] + [9] * 8 + [4] * 4 + [4] * 5 + [2, 2, 2, 2, 7, 7]
    return dict(pred=np.array(pred, np.int64), truth=np.array(truth, np.int64), pred_labels=np.array(pred_labels, np.int64),
                truth_labels=np.array(truth_labels, np.int64))


def labelled_random_case(M=2500):
    """Random objects whose class is a function of the id on each side, so that eligibility cuts across the pairs."""
    rs = np.random.RandomState(7)
    pred, truth = rs.randint(-1, 15, M).astype(np.int64), rs.randint(-1, 11, M).astype(np.int64)
    return dict(pred=pred * 11, truth=truth * 13, pred_labels=np.where(pred < 0, 0, pred % 3), truth_labels=np.where(truth < 0, 0, truth % 3),
                iou=(0.05, 0.1, 0.5))


def disjoint_case():
    """Both columns have rows and no point lies in a row of each: no pair, every best partner -1, with class tables."""
    half = np.arange(600) < 300
    pred, truth = np.where(half, np.arange(600) % 4 * 9, -1), np.where(half, -1, np.arange(600) % 3 * 5)
    return dict(pred=pred.astype(np.int64), truth=truth.astype(np.int64), pred_labels=(pred % 2).astype(np.int64),
                truth_labels=(truth % 2).astype(np.int64))


CASES = {"identity": identity_case, "disjoint": disjoint_case, "split": split_case, "merge": merge_case, "tie": tie_case, "tie-mirror": tie_mirror_case,
         "singletons": singletons_case, "fan": fan_case, "fan-mirror": fan_mirror_case, "classes": classes_case,
         "labelled-random": labelled_random_case,
         "negatives": lambda: negatives_case(False), "negatives-ignored": lambda: negatives_case(True),
         "pred-all-negative": lambda: negatives_case(False, pred_all=True),
         "truth-all-negative": lambda: negatives_case(False, truth_all=True),
         "truth-all-negative-ignored": lambda: negatives_case(True, truth_all=True),
         "both-all-negative": lambda: negatives_case(False, pred_all=True, truth_all=True)}
CASES.update({"edge-%d" % M: (lambda M=M: edge_case(M)) for M in EDGE_SIZES})


def room_inputs(n_points=20000):
    """The composition a user runs: synthetic.make_room, its true classes (floor, walls, boxes) and the same classes with a
    band of points flipped -- everything between two heights becomes class 1.  -> (scan, true labels, flipped labels, voxel);
    the objects of both come from extract_objects."""
    import scene_objects_cases as OC
    scan, labels, _, voxel = OC.room_case(n_points)
    z = scan[:, 2]
    lo = z.min() + 0.3 * (z.max() - z.min())
    band = (z >= lo) & (z < lo + 0.25)
    return scan, labels, np.where(band, 1, labels).astype(np.int64), voxel
