"""Plain numpy restatement of partial noise in the device cut ("Cutting episodes on the device", steps
P0-P7), written from the definition: the slots, draws and cloud arithmetic are those of tests/episode_cut_ref.py; the mask
edit is np.unique over the instance ids of the slots and Python integers.  The tests compare the kernel with it bit for
bit."""
import numpy as np

from episode_cut_ref import draw, prepare, slots, stream

DROP_ABOVE = 0xB3333333  # floor(0.7 * 2^32): the drop is drawn when draw(hA, 1) is above it


def edit(lab, inst, c, seed, key):
    """P2-P7 on the labels and instance ids of a cloud's N slots -> (mask0, mask, info (8,) int32)."""
    lab, inst = np.asarray(lab), np.asarray(inst).astype(np.int64)
    key = int(key) & 0xffffffff
    hA = stream(seed, (2 * key) & 0xffffffff)
    mask0 = lab == c                                                          # P2
    objs, first = np.unique(inst, return_index=True)                          # P3: ascending as signed, the lowest slot
    K = len(objs)
    eligible = [int(o) for o, t in zip(objs, first) if lab[t] != c]
    fg = [int(o) for o in objs if mask0[inst == o].any()]
    multi = K > 1 and bool((lab != lab[0]).any())
    e, f = len(eligible), len(fg)
    mask = mask0.copy()
    did = o_flip = n_flip = o_drop = n_drop = 0
    if multi and e > 0:                                                       # P4
        o_flip = eligible[(int(draw(hA, 0)) * e) >> 32]
        n_flip = int((inst == o_flip).sum())
        mask = mask | (inst == o_flip)
        did |= 1
    if int(draw(hA, 1)) > DROP_ABOVE and f > 0:                               # P5: fg was taken before the flip
        o = fg[(int(draw(hA, 2)) * f) >> 32]
        dropped = mask & ~(inst == o)
        if dropped.any():
            mask, o_drop, n_drop = dropped, o, int((inst == o).sum())
            did |= 2
        else:                                                                 # it would empty the mask: not applied
            did |= 4
    return mask0, mask, np.array([K, e, f, did, o_flip, n_flip, o_drop, n_drop], np.int64).astype(np.int32)


def legal(flags, pos, S, m_A, has_instances):
    """P0 and the flag rules of the plain cut."""
    if flags & ~7 or ((flags & 1) == 1) != (pos >= S):
        return False
    return not flags & 4 or (pos < S and m_A == 0 and has_instances)


def cut_batch_partial(points, labels, instances, offsets, desc, classes, S, Q, N, seed, attribs="xyzrgbXYZ"):
    """cut_batch of episode_cut_ref with flags bit 2 and instances (T,) int32 or None -> its dict plus info
    (E (S + Q), 8) int32.  Every descriptor must be legal (a refused cloud is the caller's to leave out of a comparison)."""
    desc, classes = np.asarray(desc), np.asarray(classes)
    x, mask, gt, qy, sm, info = [], [], [], [], [], []
    for b, (block, c, m_A, flags, key) in enumerate(desc.tolist()):
        e, pos = divmod(b, S + Q)
        assert legal(flags, pos, S, m_A, instances is not None), (b, flags, m_A)
        o0, o1 = int(offsets[block]), int(offsets[block + 1])
        lab = labels[o0:o1]
        sl = slots(lab, N, c, m_A, seed, key)                                 # P1: B / B' with m_A = 0 under bit 2
        assert sl.min() >= 0 and sl.max() < o1 - o0
        x.append(prepare(points[o0 + sl], attribs))
        sm.append(o0 + sl)
        l = lab[sl]
        rec = np.zeros(8, np.int32)
        if pos < S:
            m0 = m = l == c
            if flags & 4:
                m0, m, rec = edit(l, instances[o0:o1][sl], c, seed, key)
            mask.append(m.astype(np.int32))                                   # P6
            gt.append(np.zeros(N, np.int32) if flags & 2 else m0.astype(np.int32))
        else:
            y = np.zeros(N, np.int64)
            for k in range(classes.shape[1] - 1, -1, -1):
                y[l == classes[e, k]] = k + 1
            qy.append(y)
        info.append(rec)
    qy = np.stack(qy) if qy else np.zeros((0, N), np.int64)
    return dict(x=np.stack(x), mask=np.stack(mask), gt_mask=np.stack(gt), query_y=qy, gt_query_y=qy.copy(),
                slot_map=np.stack(sm).astype(np.int32), info=np.stack(info))
