"""Stage-by-stage restatement of csrc/aux_heads.hip on the CPU (numpy), for tests/test_gpu_aux_kernels.py;
tests/test_aux_ref_host.py holds it to the fp32 oracle (oracle/r3d_oracle.py) without a GPU.

Every function takes a ``dtype``: float64 is the reference, float32 is the same formula in the kernels' precision.  With
``chain=True`` (float32 only) every sum the kernels form -- over the points of a box or a cloud, over the channels of a
dot product or a norm, over the seeds of a row, over the shots of a prototype -- is ONE running fp32 sum over its terms in
index order (``np.cumsum`` in float32).  The kernels add sequentially over up to N terms, so the bars of the GPU tests come
from this evaluation and not from numpy's pairwise fp32 sums.

What decides MEMBERSHIP of a point in a box is fixed in fp32 by the reference and by the kernel alike (grid_sampling,
models/mpti.py:316-371): the box bounds are fp32 here whatever ``dtype`` is.

The second half builds the inputs of the detection and head cases, shared by the host test and the GPU test."""
import numpy as np
import torch

BOXES = ((1, 0, 0), (2, 0, 0), (2, 0, 1), (2, 1, 0), (2, 1, 1))  # (n_x = n_y, i_x, i_y): box 0 scale (1,1,1), 1..4 (2,2,1)


def _dt(dtype):
    return {torch.float64: np.float64, torch.float32: np.float32}.get(dtype, dtype)


def _np(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _sum(x, axis, chain):
    """Sum over one axis in x's own dtype: numpy's (pairwise) sum, or one running fp32 sum in index order."""
    if not chain:
        return x.sum(axis=axis)
    assert x.dtype == np.float32
    if x.shape[axis] == 0:
        return np.zeros(np.delete(x.shape, axis), np.float32)
    return np.take(np.cumsum(x, axis=axis, dtype=np.float32), -1, axis=axis)


def rel(got, want):
    """max |got - want| / max |want| (0 / 0 = 0)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if want.size == 0:
        return 0.0
    d, s = np.abs(got - want).max(), np.abs(want).max()
    return float(d / s) if s > 0 else float(d)


# ----------------------------------------------------------------------------------------------------------------------
# 1. clean-shot detection (models/mpti.py:87-223, 316-371)
# ----------------------------------------------------------------------------------------------------------------------
def box_members(support_x, support_y):
    """(S, 5, N) bool: foreground point p of shot s lies in box b.  fp32, with the operations of O.grid_sampling:
    d = (max - min) / n, lo = min + i * d, hi = lo + d, >= / <= (a point on a split plane lies in two boxes)."""
    sx = torch.as_tensor(_np(support_x)).float()
    sy = torch.as_tensor(_np(support_y))
    S, _, N = sx.shape
    mem = torch.zeros(S, 5, N, dtype=torch.bool)
    for s in range(S):
        fg = sy[s] == 1
        if not fg.any():
            continue
        P = sx[s, :3]
        mn, mx = P[:, fg].min(1).values, P[:, fg].max(1).values
        for b, (n, ix, iy) in enumerate(BOXES):
            d = [(mx[0] - mn[0]) / n, (mx[1] - mn[1]) / n, (mx[2] - mn[2]) / 1]
            lo = [mn[0] + ix * d[0], mn[1] + iy * d[1], mn[2] + 0 * d[2]]
            m = fg.clone()
            for a in range(3):
                m &= (P[a] >= lo[a]) & (P[a] <= lo[a] + d[a])
            mem[s, b] = m
    return mem.numpy()


def box_stats(support_x, support_y, feat, dtype=torch.float64, chain=False):
    """support_x (S, Cin, N), support_y (S, N), feat (S, N, D) -> cnt (S, 5) int64, sum (S, 5, D) in `dtype`."""
    dt = _dt(dtype)
    mem = box_members(support_x, support_y)
    f = _np(feat).astype(dt)
    S, N, D = f.shape
    out = np.zeros((S, 5, D), dt)
    for s in range(S):
        for b in range(5):
            out[s, b] = _sum(f[s][mem[s, b]], 0, chain)
    return mem.sum(-1).astype(np.int64), out


def decide(cnt, bsum, n_way, k_shot, dtype=torch.float64, chain=False):
    """mean_pl_support_y / mean_pl_support_y_multi_scale on box statistics.  -> dict:
    rec[way][scale] = dict(seeds (ns, D) box means before F.normalize, owner (ns,) shot of a seed, cs (ns,) row sums,
                           mean, pos (k_shot,), tot (k_shot,));
    flags (2, n_way, k_shot) int, keep (n_way, k_shot) int.
    A shot without seeds at a scale takes flag 0 there (the kernel's `tot > 0 && ...`; the reference cannot run on it)."""
    dt = _dt(dtype)
    cnt, bsum = _np(cnt), _np(bsum).astype(dt)
    D = bsum.shape[-1]
    flags = np.zeros((2, n_way, k_shot), np.int64)
    rec = [[None, None] for _ in range(n_way)]
    for way in range(n_way):
        for scale, boxes in enumerate(((0,), (1, 2, 3, 4))):
            rows, owner = [], []
            for k in range(k_shot):  # seeds in shot order, then box order (x outer, y inner), non-empty boxes only
                s = way * k_shot + k
                for b in boxes:
                    if cnt[s, b] > 0:
                        rows.append(bsum[s, b] / dt(cnt[s, b]))
                        owner.append(k)
            ns = len(rows)
            owner = np.asarray(owner, np.int64)
            seeds = np.stack(rows) if ns else np.zeros((0, D), dt)
            nrm = np.sqrt(_sum(seeds * seeds, 1, chain))
            sn = seeds / np.maximum(nrm, dt(1e-12))[:, None]  # F.normalize
            cos = _sum(sn[:, None, :] * sn[None, :, :], 2, chain)
            cos[np.arange(ns), np.arange(ns)] = 0
            if scale == 0:
                cos = cos * cos * cos
            cs = _sum(cos, 1, chain)
            mean = _sum(cs, 0, chain) / dt(ns) if ns else dt(np.nan)
            above = cs > mean
            tot = np.array([(owner == k).sum() for k in range(k_shot)])
            pos = np.array([above[owner == k].sum() for k in range(k_shot)])
            for k in range(k_shot):
                flags[scale, way, k] = int(tot[k] > 0 and dt(pos[k]) / dt(tot[k]) > dt(0.5))
            rec[way][scale] = dict(seeds=seeds, owner=owner, cs=cs, mean=mean, pos=pos, tot=tot)
    keep = ((flags[0] + flags[1]) / 2.0 >= 0.5).astype(np.int64)
    for way in range(n_way):
        if not keep[way].any():  # a way that would lose every shot keeps all of them (mpti.py:216-219)
            keep[way] = 1
    return dict(rec=rec, flags=flags, keep=keep)


# ----------------------------------------------------------------------------------------------------------------------
# 2. ProtoNet head (models/protonet.py:295-349; 892-915 for keep)
# ----------------------------------------------------------------------------------------------------------------------
def pooled(feat, support_y, dtype=torch.float64, chain=False):
    """getMaskedFeatures: feat (S, N, D), support_y (S, N) in {0, 1} -> (S, 2, D): foreground, background means,
    sum(feat * mask) / (mask.sum() + 1e-5)."""
    dt = _dt(dtype)
    f, y = _np(feat).astype(dt), _np(support_y)
    N = y.shape[1]
    nfg = (y == 1).sum(1)
    fg = _sum(f * (y == 1).astype(dt)[:, :, None], 1, chain) / (nfg.astype(dt) + dt(1e-5))[:, None]
    bg = _sum(f * (y == 0).astype(dt)[:, :, None], 1, chain) / ((N - nfg).astype(dt) + dt(1e-5))[:, None]
    return np.stack((fg, bg), 1)


def prototypes(pool, n_way, k_shot, keep=None, dtype=torch.float64, chain=False):
    """getPrototype: (n_way + 1, D), background first: background over ALL shots, foreground of a way over its kept shots."""
    dt = _dt(dtype)
    pool = _np(pool).astype(dt)
    S = n_way * k_shot
    out = [_sum(pool[:, 1], 0, chain) / dt(S)]
    for w in range(n_way):
        ks = [w * k_shot + k for k in range(k_shot) if keep is None or int(_np(keep).reshape(-1)[w * k_shot + k]) != 0]
        out.append(_sum(pool[ks, 0], 0, chain) / dt(len(ks)))
    return np.stack(out)


def similarity(protos, q, method, scaler=10.0, dtype=torch.float64, chain=False):
    """calculateSimilarity: protos (C, D), q (n, D) -> (n, C).  cosine: dot / max(|q| |p|, 1e-8) * scaler; euclidean:
    -||q - p + 1e-6||^2 (torch 1.8's pairwise_distance: the eps inside the norm)."""
    dt = _dt(dtype)
    p, q = _np(protos).astype(dt), _np(q).astype(dt)
    if method == "cosine":
        dot = _sum(q[:, None, :] * p[None, :, :], 2, chain)
        qn, pn = np.sqrt(_sum(q * q, 1, chain)), np.sqrt(_sum(p * p, 1, chain))
        return dot / np.maximum(qn[:, None] * pn[None, :], dt(1e-8)) * dt(scaler)
    assert method == "euclidean"
    df = (q[:, None, :] - p[None, :, :]) + dt(1e-6)
    dist = np.sqrt(_sum(df * df, 2, chain))
    return -(dist * dist)


# ----------------------------------------------------------------------------------------------------------------------
# 3. the integer reducers
# ----------------------------------------------------------------------------------------------------------------------
def miou_hist(pred, gt, lut, n_classes, hist=None):
    """r3d_miou_accumulate: (3, n_classes) = GT | predicted | true positive per test class.  Labels and predictions are
    CLAMPED into the look-up table, [0, n_lut - 1], before the look-up; a true positive is gt == pred before clamping."""
    pred, gt, lut = _np(pred).astype(np.int64).ravel(), _np(gt).astype(np.int64).ravel(), _np(lut).astype(np.int64)
    hist = np.zeros((3, n_classes), np.uint64) if hist is None else hist.copy()
    gi, pi = lut[np.clip(gt, 0, len(lut) - 1)], lut[np.clip(pred, 0, len(lut) - 1)]
    hist[0] += np.bincount(gi, minlength=n_classes).astype(np.uint64)
    hist[1] += np.bincount(pi, minlength=n_classes).astype(np.uint64)
    hist[2] += np.bincount(gi[gt == pred], minlength=n_classes).astype(np.uint64)
    return hist


# ----------------------------------------------------------------------------------------------------------------------
# 4. inputs of the detection cases
# ----------------------------------------------------------------------------------------------------------------------
# (n_way, k_shot, N, D, variant, Cin).  Variants: "plain" coordinates in [0, 1); "dyadic" multiples of 1/64 with points ON
# the split planes and the maxima, and a shot whose foreground lies on the diagonal (boxes (0,1) and (1,0) empty);
# "ragged" random fp32 coordinates offset by 1e3; "empty" a shot without foreground inside way 0 and a last way without
# any.  (A box row or column that holds the extreme of the foreground is never empty, so three empty boxes cannot occur.)
DETECT_CASES = [
    (2, 5, 512, 192, "plain", 9), (1, 1, 70, 33, "plain", 3), (2, 2, 300, 64, "plain", 9), (3, 3, 200, 65, "plain", 3),
    (2, 4, 256, 160, "plain", 9), (2, 3, 320, 193, "plain", 9), (4, 8, 128, 256, "plain", 3), (7, 4, 96, 224, "plain", 9),
    (3, 3, 200, 65, "dyadic", 9), (2, 4, 256, 160, "dyadic", 3), (2, 2, 300, 64, "dyadic", 9),
    (1, 1, 70, 33, "ragged", 9), (2, 3, 320, 193, "ragged", 3), (7, 4, 96, 224, "ragged", 9),
    (2, 5, 512, 192, "empty", 9), (3, 3, 200, 65, "empty", 3),
]
# the layout test runs these as E = 3 episodes (seeds 0, 1, 2) in one call
LAYOUT_CASES = [(3, 3, 200, 65, "dyadic", 9), (2, 3, 320, 193, "ragged", 3), (2, 5, 512, 192, "empty", 9)]
DETECT_RUNS = [(c, 0) for c in DETECT_CASES] + [(c, s) for c in LAYOUT_CASES for s in (1, 2)]  # every (case, seed) in use
SIGMA = 0.05  # spread of a point's feature round its direction


def case_id(c):
    return "%dw%ds-N%d-D%d-%s-C%d" % c


def shot_roles(n_way, k_shot, variant):
    """Per way the role of each shot.  With u the way's direction and e_q four directions of the shot's own, one per
    quadrant, all orthonormal: 'clean' u + b e_q with b <= 0.2 (seeds within 0.02 of u in cosine); 'far' u + 1.2 e_q
    (cosine 0.64 with a clean seed, 0.41 between its own); 'noisy' e_q alone (cosine 0 with everything); 'single' (the only
    shot of a way) u + (0.1, 0.2, 1.0, 1.5)_q e_q; 'diag' (dyadic: foreground on the diagonal, the low quadrant clean and
    the larger high quadrant noisy: a share of exactly 1/2 at scale (2,2,1)); 'nofg' (no foreground point).  Every way
    with three or more seeds at a scale holds a tight group and at least one seed far from it, so that the mean of the
    row sums falls between the groups with margins of order 0.1 (tests/test_aux_ref_host.py measures them)."""
    roles = []
    for w in range(n_way):
        if k_shot == 1:
            r = ["single"]
        elif k_shot == 2:
            r = ["clean", "noisy" if w == 0 else "far"]  # two seeds at scale (1,1,1): row sums tie exactly
        else:
            m = (1 + w % 2) if k_shot >= 4 else w % 2
            r = ["clean"] * k_shot
            for j in range(m):
                r[(w + 2 * j) % k_shot] = "noisy"
            if m == 0:
                r[-1] = "far"
        if variant == "dyadic" and w == 0 and k_shot >= 3:
            r[max(k for k in range(k_shot) if r[k] == "clean")] = "diag"
        if variant == "empty":
            if w == 0:
                r[1] = "nofg"
            if w == n_way - 1:
                r = ["nofg"] * k_shot
        roles.append(r)
    return roles


def detection_inputs(case, seed=0):
    """-> dict(support_x (S, Cin, N) f32, support_y (S, N) int32, feat (S, N, D) f32, roles)."""
    n_way, k_shot, N, D, variant, Cin = case
    S = n_way * k_shot
    rs = np.random.RandomState(1000 * seed + 7 * N + D + 13 * S + len(variant))
    basis = np.linalg.qr(rs.randn(D, D))[0].T  # orthonormal rows: way directions, then shot directions, then 4 per shot
    assert n_way + 5 * S <= D
    roles = shot_roles(n_way, k_shot, variant)
    sx = rs.rand(S, Cin, N).astype(np.float32)
    sy = (rs.rand(S, N) < 0.5).astype(np.int32)
    feat = rs.randn(S, N, D).astype(np.float32) / np.float32(np.sqrt(D))  # background rows: anything finite
    for w in range(n_way):
        for k in range(k_shot):
            s, role = w * k_shot + k, roles[w][k]
            if role == "nofg":
                sy[s] = 0
                continue
            sy[s, :8] = 1  # (at least the eight special points of a dyadic shot)
            fg = np.flatnonzero(sy[s] == 1)
            if variant == "ragged":
                sx[s, :3] = (rs.rand(3, N) * np.array([[3.0], [2.0], [1.0]]) + 1000.0).astype(np.float32)
            elif variant == "dyadic":
                g = rs.randint(0, 127, (3, N))
                if role == "diag":  # low quadrant [0, 62]^2 (30 %), high quadrant [64, 126]^2 (70 %), nothing on a plane
                    hi = rs.rand(N) < 0.7
                    g[:2] = np.where(hi[None, :], rs.randint(64, 127, (2, N)), rs.randint(0, 63, (2, N)))
                    g[:, fg[0]], g[:, fg[1]] = 0, 126
                else:
                    r = lambda: rs.randint(0, 127)
                    sp = [(0, 0, 0), (126, 126, 126), (63, r(), r()), (r(), 63, r()), (63, 63, r()), (126, r(), r()),
                          (r(), 126, r()), (r(), r(), 126)]
                    for i, pt in enumerate(sp):
                        g[:, fg[i]] = pt
                sx[s, :3] = (g / 64.0 + 2.0).astype(np.float32)
            P = sx[s, :3].astype(np.float64)
            mid = (P[:, fg].min(1) + P[:, fg].max(1)) / 2
            quad = 2 * (P[0] > mid[0]) + (P[1] > mid[1])
            u, e, eq = basis[w], basis[n_way + s], basis[n_way + S + 4 * s:n_way + S + 4 * s + 4]
            noise = SIGMA * rs.randn(N, D) / np.sqrt(D)
            if role == "clean":
                f = u[None, :] + (0.05 + 0.03 * k + 0.02 * quad)[:, None] * eq[quad]
            elif role == "far":
                f = u[None, :] + 1.2 * eq[quad]
            elif role == "single":
                f = u[None, :] + np.array([0.1, 0.2, 1.0, 1.5])[quad][:, None] * eq[quad]
            elif role == "noisy":
                f = eq[quad]
            else:  # diag
                f = np.where((quad == 0)[:, None], u[None, :] + 0.1 * e[None, :], eq[1][None, :])
            feat[s, fg] = (f + noise)[fg].astype(np.float32)
    return dict(support_x=sx, support_y=sy, feat=feat, roles=roles)


def has_empty_shot(case):
    return case[4] == "empty"


# ----------------------------------------------------------------------------------------------------------------------
# 5. inputs of the head cases
# ----------------------------------------------------------------------------------------------------------------------
# (n_way, k_shot, N, n_q, D, variant): "unit" features of unit scale, "offset" a common offset of 50 and spread 0.1
HEAD_CASES = [(2, 1, 70, 1, 33, "unit"), (3, 2, 300, 2, 64, "offset"), (2, 5, 264, 2, 192, "unit"), (5, 2, 200, 1, 256, "offset"),
              (7, 1, 128, 2, 193, "unit"), (4, 1, 96, 1, 96, "unit")]


def head_case_id(c):
    return "%dw%ds-N%d-q%d-D%d-%s" % c


def head_inputs(case, seed=0):
    """-> dict(sfeat (S, N, D) f32, support_y (S, N) int32, qfeat (n_q * N, D) f32, keep (S,) int32 or None).
    Shot 0's mask is all foreground and shot 1's all background (pooled rows with the divisor 0 + 1e-5: exactly 0).
    The foreground rows of way 0 all hold ONE vector of multiples of 1/16: their masked sums are exact in fp32 in any order,
    so the class-1 prototype has the same bits in every correct fp32 evaluation, the chain-order restatement included.
    Query row 0 is that prototype, row 1 lies 1e-5 from it in every channel, row 2 is zero."""
    n_way, k_shot, N, n_q, D, variant = case
    S = n_way * k_shot
    rs = np.random.RandomState(2000 * seed + 3 * N + D + 11 * S)
    cent = rs.randn(n_way + 1, D)
    sy = (rs.rand(S, N) < 0.4).astype(np.int32)
    sy[0], sy[1] = 1, 0
    cls = np.where(sy == 1, (np.arange(S) // k_shot + 1)[:, None], 0)
    off, sc = (50.0, 0.1) if variant == "offset" else (0.0, 1.0)
    sfeat = off + sc * (cent[cls] + 0.5 * rs.randn(S, N, D))
    qfeat = off + sc * (cent[rs.randint(0, n_way + 1, n_q * N)] + 0.5 * rs.randn(n_q * N, D))
    const = off + rs.randint(-32, 33, D) / 16.0
    for s in range(k_shot):
        sfeat[s][sy[s] == 1] = const
    sfeat, qfeat = sfeat.astype(np.float32), qfeat.astype(np.float32)
    p1 = prototypes(pooled(sfeat, sy, torch.float32, True), n_way, k_shot, None, torch.float32, True)[1]
    qfeat[0], qfeat[1], qfeat[2] = p1, p1 + np.float32(1e-5), 0.0
    keep = None
    if k_shot >= 2 and n_way >= 2:  # one shot dropped in two ways
        keep = np.ones(S, np.int32)
        keep[0 * k_shot + 1] = 0
        keep[1 * k_shot + 0] = 0
    return dict(sfeat=sfeat, support_y=sy, qfeat=qfeat, keep=keep)


_refs = {}


def detect_reference(case, seed=0):
    """Inputs and, in float64 ('f64') and chain-order float32 ('c32'), (cnt, box sums, decide(...)) of a detection case;
    computed once and shared."""
    key = ("d", seed) + tuple(case)
    if key not in _refs:
        inp = detection_inputs(case, seed)
        out = dict(inp=inp)
        for name, (dt, chain) in dict(f64=(torch.float64, False), c32=(torch.float32, True)).items():
            cnt, bsum = box_stats(inp["support_x"], inp["support_y"], inp["feat"], dt, chain)
            out[name] = (cnt, bsum, decide(cnt, bsum, case[0], case[1], dt, chain))
        _refs[key] = out
    return _refs[key]


def detect_e32(case, seed=0):
    """quantity -> relative max-norm error of the chain-order float32 restatement against float64."""
    r = detect_reference(case, seed)
    e = dict(box_sum=rel(r["c32"][1], r["f64"][1]))
    for scale, name in enumerate(("cs1", "cs2")):
        got = np.concatenate([r["c32"][2]["rec"][w][scale]["cs"] for w in range(case[0])])
        want = np.concatenate([r["f64"][2]["rec"][w][scale]["cs"] for w in range(case[0])])
        e[name] = rel(got, want)
    return e


def head_reference(case):
    """Inputs and, in float64 ('f64') and chain-order float32 ('c32'): pooled, proto / proto_keep, Z[method] / Z_keep[method],
    and Zeps[method] = rows 0, 1 against class 1 of similarity(the fp32 table taken as given)."""
    key = ("h",) + tuple(case)
    if key not in _refs:
        n_way, k_shot = case[0], case[1]
        inp = head_inputs(case)
        out = dict(inp=inp)
        table = None
        for name, (dt, chain) in dict(c32=(torch.float32, True), f64=(torch.float64, False)).items():
            pl = pooled(inp["sfeat"], inp["support_y"], dt, chain)
            r = dict(pooled=pl, proto=prototypes(pl, n_way, k_shot, None, dt, chain), Z={}, Z_keep={}, Zeps={})
            if name == "c32":
                table = r["proto"]
            if inp["keep"] is not None:
                r["proto_keep"] = prototypes(pl, n_way, k_shot, inp["keep"], dt, chain)
            for method in ("cosine", "euclidean"):
                r["Z"][method] = similarity(r["proto"], inp["qfeat"], method, 10.0, dt, chain)
                r["Zeps"][method] = similarity(table[1:2], inp["qfeat"][:2], method, 10.0, dt, chain)[:, 0]
                if inp["keep"] is not None:
                    r["Z_keep"][method] = similarity(r["proto_keep"], inp["qfeat"], method, 10.0, dt, chain)
            out[name] = r
        _refs[key] = out
    return _refs[key]


def rel_entry(got, want):
    """max over the entries of |got - want| / |want|."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float((np.abs(got - want) / np.abs(want)).max())


def head_e32(case):
    r = head_reference(case)
    c, f = r["c32"], r["f64"]
    e = dict(pooled=rel(c["pooled"], f["pooled"]), proto=rel(c["proto"], f["proto"]))
    if "proto_keep" in c:
        e["proto"] = max(e["proto"], rel(c["proto_keep"], f["proto_keep"]))
    for method, name in (("cosine", "Zcos"), ("euclidean", "Zeuc")):
        e[name] = rel(c["Z"][method], f["Z"][method])
        if c["Z_keep"]:
            e[name] = max(e[name], rel(c["Z_keep"][method], f["Z_keep"][method]))
    e["Zeps"] = rel_entry(c["Zeps"]["euclidean"], f["Zeps"]["euclidean"])
    return e
