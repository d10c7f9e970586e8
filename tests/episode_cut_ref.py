"""Plain numpy restatement of the device cut ("Cutting episodes on the device"): the draw functions and
steps A-D, written from the definition.  Integer arithmetic in uint64 masked to 32 bits, `np.lexsort((i, draw))` for the
order by (draw, index); the cloud's float32 arithmetic is that of tests/scene_ref.py's step 6.  The tests compare the
kernel with it bit for bit; ties between equal draws are decided here."""
import numpy as np

f32 = np.float32
M32 = np.uint64(0xffffffff)
ATTRIBS = {"xyz": (False, False), "xyzrgb": (True, False), "xyzXYZ": (False, True), "xyzrgbXYZ": (True, True)}  # rgb, XYZ


def _u(x):
    return np.asarray(x).astype(np.uint64) & M32


def mix(x):
    x = _u(x)
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7feb352d)) & M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846ca68b)) & M32
    return x ^ (x >> np.uint64(16))


def stream(seed, key):
    s, k = _u(seed), _u(key)
    return (mix((k * np.uint64(0x9E3779B1) + s) & M32) + ((s * np.uint64(0x85EBCA77)) & M32)) & M32


def draw(h, i):
    return mix(_u(h) ^ ((_u(i) * np.uint64(0x9E3779B1) + np.uint64(0x632BE5AB)) & M32))


def select(cand, h, m):
    """The m candidates (local indices) with the smallest (draw(h, i), i), by ascending i."""
    cand = np.asarray(cand, np.int64)
    assert 0 <= m <= len(cand), (m, len(cand))
    d = np.asarray(draw(h, cand))  # module-level lookup: a test may patch `draw`
    order = np.lexsort((cand, d))
    return np.sort(cand[order[:m]])


def slots(labels, N, c, m_A, seed, key):
    """Steps A, B / B': the N local indices of the cloud."""
    labels = np.asarray(labels)
    n = len(labels)
    key = int(key) & 0xffffffff
    hA, hB = stream(seed, (2 * key) & 0xffffffff), stream(seed, (2 * key + 1) & 0xffffffff)
    a = select(np.nonzero(labels == c)[0], hA, m_A)
    m_B = N - m_A
    if n >= N:
        b = select(np.arange(n), hB, m_B)
    else:
        b = ((np.asarray(draw(hB, np.arange(m_B))) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)
    return np.concatenate([a, b]).astype(np.int64)


def prepare(rows, attribs):
    """Step C on the gathered rows (N, 6) float32 -> (C, N) float32."""
    rgb, XYZ = ATTRIBS[attribs]
    rows = np.asarray(rows, f32)
    xyz = rows[:, 0:3] - rows[:, 0:3].min(0)
    ch = [xyz]
    if rgb:
        ch.append(rows[:, 3:6] / f32(255.0))
    if XYZ:
        ext = xyz.max(0)
        with np.errstate(invalid="ignore", divide="ignore"):
            ch.append(np.where(ext > 0, xyz / ext, f32(0)).astype(f32))  # a flat axis: 0
    return np.concatenate(ch, 1).astype(f32).T


def cut_batch(points, labels, offsets, desc, classes, S, Q, N, seed, attribs="xyzrgbXYZ"):
    """points (T, 6) f32, labels (T,) i32, offsets (n_blocks + 1,), desc (E (S + Q), 5), classes (E, n_way) ->
    dict of x (E (S + Q), C, N) f32, mask / gt_mask (E S, N) i32, query_y / gt_query_y (E Q, N) i64, slot_map i32."""
    desc, classes = np.asarray(desc), np.asarray(classes)
    E = classes.shape[0]
    x, mask, gt, qy, sm = [], [], [], [], []
    for b, (block, c, m_A, flags, key) in enumerate(desc.tolist()):
        e, pos = divmod(b, S + Q)
        assert ((flags & 1) == 1) == (pos >= S) and flags & ~3 == 0
        o0, o1 = int(offsets[block]), int(offsets[block + 1])
        lab = labels[o0:o1]
        sl = slots(lab, N, c, m_A, seed, key)
        assert sl.min() >= 0 and sl.max() < o1 - o0
        x.append(prepare(points[o0 + sl], attribs))
        sm.append(o0 + sl)
        l = lab[sl]
        if pos < S:  # D, support
            m = (l == c).astype(np.int32)
            mask.append(m)
            gt.append(np.zeros_like(m) if flags & 2 else m)
        else:        # D, query
            y = np.zeros(N, np.int64)
            for k in range(classes.shape[1] - 1, -1, -1):
                y[l == classes[e, k]] = k + 1
            qy.append(y)
    qy = np.stack(qy) if qy else np.zeros((0, N), np.int64)
    return dict(x=np.stack(x), mask=np.stack(mask), gt_mask=np.stack(gt), query_y=qy, gt_query_y=qy.copy(),
                slot_map=np.stack(sm).astype(np.int32))
