"""csrc/aux_heads.hip kernel by kernel against float64, through the C ABI (the test owns every buffer):
A. r3d_clean_shot_detect_batched stage by stage -- box counts, box sums, row sums of both scales, flags;
B. the ProtoNet evaluation head in every launch form -- pooled means, prototype table, similarity rows;
C. the integer reducers r3d_count_correct_batched and r3d_miou_accumulate.

References: tests/aux_ref.py (held to the fp32 oracle, and every detection case shown decidable without rounding, in
tests/test_aux_ref_host.py).

Bars.  Every figure is max |got - ref64| / max |ref64| over the named block (``Zeps``: per entry).  Each test prints it
beside ``e32``, the error of the chain-order float32 restatement (one running fp32 sum per sum the kernels form) against
float64 on that input.  A bar is 4 x the worst e32 of its quantity over this module's cases -- measured on the CPU against
the reference's arithmetic, never against the kernel's; the factor covers one fp32 summation order against another --
and never above CEIL = 1e-3.  tests/test_aux_ref_host.py recomputes the e32 and holds this table to them.  Counts, flags,
histograms, zero columns and every "bit for bit" carry no tolerance."""
import numpy as np
import pytest
import torch

import aux_ref as R

pytestmark = pytest.mark.gpu

CEIL = 1e-3
# quantity -> bar = 4 x the worst chain-order e32 over the module's cases
BAR = dict(box_sum=2.3e-6,   # 5.62e-7 (2w5s-N512-D192-empty)
           cs1=5.9e-6,       # 1.48e-6 (7w4s-N96-D224-plain), scale (1,1,1): cubed
           cs2=1.7e-6,       # 4.23e-7 (4w8s-N128-D256-plain), scale (2,2,1): 32 seeds
           pooled=2.7e-6,    # 6.79e-7 (5w2s-N200-D256-offset)
           proto=1.5e-6,     # 3.77e-7 (3w2s-N300-D64-offset)
           Zcos=5.4e-6,      # 1.35e-6 (5w2s-N200-D256-offset)
           Zeuc=3.7e-6,      # 9.33e-7 (5w2s-N200-D256-offset)
           Zeps=1.0e-5)      # 2.52e-6 (5w2s-N200-D256-offset): a query row equal to a prototype, per entry
assert max(BAR.values()) <= CEIL

NAN_WORD = 0x7FC00000  # the bytes a call does not own hold this before and after
SENTINEL = -7.5        # dbg_cos_sum beyond the seeds that exist


@pytest.fixture(scope="module")
def lib():
    from r3dfsseg_amd import _lib
    return _lib.load()


def _p(t):
    from r3dfsseg_amd.ops import _p as p
    return p(t)


def _st():
    from r3dfsseg_amd.ops import _st as st
    return st()


def _check(rc):
    from r3dfsseg_amd import _lib
    _lib.check(rc)


def _hold(case, errs, e32, prefix="AK"):
    """Print every figure beside its e32, then assert every one (a key 'Zcos:keep' takes the bar of 'Zcos')."""
    for k, v in errs.items():
        print("%s| %-30s %-16s err %.2e  e32 %.2e  bar %.1e" % (prefix, case, k, v, e32.get(k.split(":")[0], float("nan")),
                                                               BAR[k.split(":")[0]]))
    bad = {k: v for k, v in errs.items() if not v <= BAR[k.split(":")[0]]}
    assert not bad, (case, bad)


# ----------------------------------------------------------------------------------------------------------------------
# A. clean-shot detection
# ----------------------------------------------------------------------------------------------------------------------
def _detect(lib, case, episodes, wide=False, gaps=False, poison=True):
    """One call over len(episodes) episodes.  wide: the features are columns [5, 5 + D) of a matrix of D + 37; gaps: two
    query clouds' worth of rows between the episodes' support rows and 100 words between their scratch.  Everything the call
    does not own holds NaN (poison=False: zero).  -> per episode dict(box_sum (S, 5, 256), box_cnt (S, 5), dbg (n_way, 2, 4 k), keep (S,))."""
    n_way, k_shot, N, D, _, Cin = case
    S, E = n_way * k_shot, len(episodes)
    words = lib.r3d_clean_ws_words(n_way, k_shot)
    assert words >= S * 5 * 256 + S * 5
    ws_stride = words + (100 if gaps else 0)
    ep_rows = (S + (2 if gaps else 0)) * N
    ldf, c0 = (D + 37, 5) if wide else (D, 0)
    mat = torch.full((E * ep_rows, ldf), float("nan") if poison else 0.0)
    for e, inp in enumerate(episodes):
        mat[e * ep_rows:e * ep_rows + S * N, c0:c0 + D] = torch.from_numpy(inp["feat"]).view(S * N, D)
    matd = mat.cuda()
    sx = torch.from_numpy(np.stack([i["support_x"] for i in episodes])).cuda()
    sy = torch.from_numpy(np.stack([i["support_y"] for i in episodes])).cuda()
    keep = torch.full((E, S), -99, dtype=torch.int32, device="cuda")
    dbg = torch.full((E, n_way, 2, 4 * k_shot), SENTINEL, device="cuda")
    ws = torch.full((E * ws_stride,), NAN_WORD if poison else 0, dtype=torch.int32, device="cuda")
    _check(lib.r3d_clean_shot_detect_batched(E, _p(matd[:, c0:c0 + D]), ldf, ep_rows, D, _p(sx), Cin, _p(sy), n_way, k_shot, N,
                                             _p(keep), _p(dbg), _p(ws), ws_stride, _st()))
    torch.cuda.synchronize()
    assert torch.equal(matd.cpu().view(torch.int32), mat.view(torch.int32))  # inputs and the bytes round them: untouched
    wsh = ws.cpu().view(E, ws_stride)
    n_sum, n_cnt = S * 5 * 256, S * 5
    assert (wsh[:, n_sum + n_cnt:] == (NAN_WORD if poison else 0)).all()  # the spare words and the gap between two episodes' scratch
    out = []
    for e in range(E):
        out.append(dict(box_sum=wsh[e, :n_sum].clone().view(torch.float32).view(S, 5, 256).numpy(),
                        box_cnt=wsh[e, n_sum:n_sum + n_cnt].view(S, 5).numpy().astype(np.int64),
                        dbg=dbg[e].cpu().numpy(), keep=keep[e].cpu().numpy().astype(np.int64)))
    return out


def _flags_from_row_sums(cs, rec, k_shot):
    """The vote on row sums as given (fp32): cs > mean, per-shot share > 0.5; no seed: 0."""
    if len(cs) == 0:
        return np.zeros(k_shot, np.int64)
    mean = np.cumsum(cs, dtype=np.float32)[-1] / np.float32(len(cs))
    above = cs > mean
    return np.array([int((rec["owner"] == k).sum() > 0 and above[rec["owner"] == k].mean() > 0.5) for k in range(k_shot)])


def _hold_detection(tag, case, seed, got):
    n_way, k_shot, N, D = case[:4]
    ref = R.detect_reference(case, seed)
    cnt, bsum, dec = ref["f64"]
    assert np.array_equal(got["box_cnt"], cnt), (tag, got["box_cnt"], cnt)
    assert (got["box_sum"][..., D:] == 0).all() and np.isfinite(got["box_sum"]).all()
    errs = dict(box_sum=R.rel(got["box_sum"][..., :D], bsum))
    flags = np.zeros((2, n_way, k_shot), np.int64)
    for scale, name in enumerate(("cs1", "cs2")):
        mine, want = [], []
        for way in range(n_way):
            rec = dec["rec"][way][scale]
            ns = len(rec["cs"])
            row = got["dbg"][way, scale]
            assert (row[ns:] == np.float32(SENTINEL)).all(), (tag, way, scale, ns, row)  # untouched beyond the seeds
            assert np.isfinite(row[:ns]).all()
            mine.append(row[:ns]); want.append(rec["cs"])
            flags[scale, way] = _flags_from_row_sums(row[:ns], rec, k_shot)
        errs[name] = R.rel(np.concatenate(mine), np.concatenate(want))
    _hold(tag, errs, R.detect_e32(case, seed))
    assert np.array_equal(flags, dec["flags"]), (tag, flags, dec["flags"])  # the vote on the device's own row sums
    assert np.array_equal(got["keep"].reshape(n_way, k_shot), dec["keep"]), (tag, got["keep"], dec["keep"])
    return errs


@pytest.mark.parametrize("case", R.DETECT_CASES, ids=R.case_id)
def test_detection_stage_by_stage(lib, case):
    """Contiguous features, one episode; ws poisoned.  Measured on the MI355X, worst over the cases of this test and of the
    layout test (worst chain-order e32 beside it): box_sum 1.74e-7 (5.62e-7), cs1 5.77e-7 (1.48e-6), cs2 2.65e-7 (4.23e-7)."""
    got = _detect(lib, case, [R.detect_reference(case)["inp"]])[0]
    _hold_detection(R.case_id(case), case, 0, got)
    if R.has_empty_shot(case):  # the rule of include/r3d.h: no seed at a scale -> flag 0 there; a way without any: all kept
        n_way, k_shot = case[:2]
        keep = got["keep"].reshape(n_way, k_shot)
        roles = R.shot_roles(n_way, k_shot, case[4])
        assert roles[0][1] == "nofg" and keep[0, 1] == 0 and keep[0].any()
        assert set(roles[-1]) == {"nofg"} and (keep[-1] == 1).all()
        assert (got["box_cnt"].reshape(n_way, k_shot, 5)[-1] == 0).all()
        assert (got["dbg"][-1] == np.float32(SENTINEL)).all()


@pytest.mark.parametrize("case", R.LAYOUT_CASES, ids=R.case_id)
def test_detection_layout_three_episodes_in_a_wide_matrix(lib, case):
    """E = 3 episodes of different content in one call: features a column slice (ldf = D + 37, first column 5), query rows
    between the episodes' support rows, ws_stride = r3d_clean_ws_words + 100; everything not owned poisoned.  Each episode
    meets its own float64 reference and equals its own contiguous, unpoisoned E = 1 call bit for bit."""
    eps = [R.detect_reference(case, s)["inp"] for s in range(3)]
    got = _detect(lib, case, eps, wide=True, gaps=True)
    for s in range(3):
        _hold_detection("%s ep %d" % (R.case_id(case), s), case, s, got[s])
    wide1 = _detect(lib, case, eps[:1], wide=True)[0]
    for s in range(3):
        alone = _detect(lib, case, [eps[s]], poison=False)[0]
        for k in alone:
            assert alone[k].tobytes() == got[s][k].tobytes(), (s, k)
            assert s > 0 or alone[k].tobytes() == wide1[k].tobytes(), k


# ----------------------------------------------------------------------------------------------------------------------
# B. ProtoNet evaluation head
# ----------------------------------------------------------------------------------------------------------------------
METHODS = {"cosine": 0, "euclidean": 1}
ZBAR = {"cosine": "Zcos", "euclidean": "Zeuc"}


class _Head:
    """Device buffers of one head case: [support rows | query rows] as columns [0, D) of a matrix of D + 3 (NaN outside)."""

    def __init__(self, lib, case):
        self.lib, self.case = lib, case
        n_way, k_shot, N, n_q, D, _ = case
        inp = R.head_reference(case)["inp"]
        self.S, self.nqp, self.C, self.planes = n_way * k_shot, n_q * N, n_way + 1, 2 if n_way > 3 else 1
        ld = self.ld = D + 3
        mat = torch.full((self.S * N + self.nqp, ld), float("nan"))
        mat[:self.S * N, :D] = torch.from_numpy(inp["sfeat"]).view(self.S * N, D)
        mat[self.S * N:, :D] = torch.from_numpy(inp["qfeat"])
        self.mat = mat.cuda()
        self.sfeat, self.qfeat = self.mat[:, :D], self.mat[self.S * N:, :D]
        self.sy = torch.from_numpy(inp["support_y"]).cuda()
        self.keep = None if inp["keep"] is None else torch.from_numpy(inp["keep"]).cuda()
        self.words = lib.r3d_protonet_head_ws_words(1, n_way, k_shot)
        assert self.words == self.S * 2 * 256

    def ws(self):
        return torch.full((self.words,), float("nan"), device="cuda")

    def Z(self, rows=None):
        return torch.full((self.planes, rows or self.nqp, 4), float("nan"), device="cuda")

    def cols(self, Z):
        """(rows, n_way + 1) of a Z buffer; the columns beyond n_way are exactly 0 in both planes."""
        full = torch.cat([Z[p] for p in range(self.planes)], 1).cpu()
        assert (full[:, self.C:] == 0).all()
        return full[:, :self.C].numpy()

    def pooled(self, ws):
        h = ws.cpu().view(self.S, 2, 256)
        D = self.case[4]
        assert torch.isnan(h[..., D:]).all()  # the pooled rows are D wide: the rest of the scratch is not written
        return h[..., :D].numpy()

    # ---- the routes -------------------------------------------------------------------------------------------------
    def head(self, method):
        n_way, k_shot, N, _, D, _ = self.case
        Z, ws = self.Z(), self.ws()
        _check(self.lib.r3d_protonet_head(_p(self.sfeat), self.ld, _p(self.qfeat), self.ld, D, _p(self.sy), n_way, k_shot, N,
                                          self.nqp, METHODS[method], 10.0, _p(Z), _p(ws), _st()))
        return Z, ws

    def batched(self, method, keep="none"):
        n_way, k_shot, N, _, D, _ = self.case
        Z, ws = self.Z(), self.ws()
        a = (1, _p(self.sfeat), self.ld, _p(self.qfeat), self.ld, 0, D, _p(self.sy))
        b = (n_way, k_shot, N, self.nqp, METHODS[method], 10.0, _p(Z), _p(ws), self.words, _st())
        if isinstance(keep, str):
            _check(self.lib.r3d_protonet_head_batched(*a, *b))
        else:
            _check(self.lib.r3d_protonet_head_keep_batched(*a, _p(keep), *b))
        return Z, ws

    def table(self, keep=None):
        n_way, k_shot, N, _, D, _ = self.case
        protos, ws = torch.full((self.C, D), float("nan"), device="cuda"), self.ws()
        _check(self.lib.r3d_protonet_prototypes_batched(1, _p(self.sfeat), self.ld, 0, D, _p(self.sy), _p(keep), n_way, k_shot,
                                                        N, _p(protos), _p(ws), self.words, _st()))
        return protos, ws

    def sim(self, protos, method, n_sys=1, stride=0):
        n_way, _, N, _, D, _ = self.case
        Z = self.Z()
        n_pts = self.nqp // n_sys
        _check(self.lib.r3d_protonet_similarity_batched(n_sys, _p(self.qfeat), self.ld, n_pts, D, _p(protos), stride, n_way,
                                                        n_pts, METHODS[method], 10.0, _p(Z), _st()))
        return Z

    def sets(self, tables, stride, method):
        """tables: flat device floats, table k at k * stride -> Z (planes, K * nqp, 4), set k rows [k nqp, (k + 1) nqp)."""
        n_way, D = self.case[0], self.case[4]
        K = 1 if stride == 0 else (tables.numel() + stride - self.C * D) // stride
        Z = self.Z(K * self.nqp)
        _check(self.lib.r3d_protonet_similarity_sets(1, K, _p(self.qfeat), self.ld, 0, D, _p(tables), stride, n_way, self.nqp,
                                                     METHODS[method], 10.0, _p(Z), _st()))
        return Z, K


def _bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.fixture(scope="module")
def heads(lib):
    cache = {}

    def get(case):
        if case not in cache:
            cache[case] = _Head(lib, case)
        return cache[case]
    return get


@pytest.mark.parametrize("case", R.HEAD_CASES, ids=R.head_case_id)
def test_head_pooled_means_and_prototype_table(heads, case):
    """pooled (read from ws) and the table of r3d_protonet_prototypes_batched as quantities of their own, with and without
    keep.  A shot whose mask is all foreground / all background: the other pooled row is exactly 0.  The class-1 prototype
    has the bits of the chain-order restatement (its sums are exact by construction): query row 0 IS that prototype.
    Measured on the MI355X (worst over the cases; worst chain-order e32 beside it): pooled 6.79e-7 (6.79e-7: the pooling
    kernels ARE one chain per channel), proto 3.77e-7 (3.77e-7)."""
    h = heads(case)
    ref = R.head_reference(case)
    protos, ws = h.table()
    torch.cuda.synchronize()
    pl = h.pooled(ws)
    assert (pl[0, 1] == 0).all() and (pl[1, 0] == 0).all()  # divisor 0 + 1e-5 under a sum of exact zeros
    errs = dict(pooled=R.rel(pl, ref["f64"]["pooled"]), proto=R.rel(protos.cpu().numpy(), ref["f64"]["proto"]))
    assert np.array_equal(protos[1].cpu().numpy().view(np.int32), ref["c32"]["proto"][1].view(np.int32))
    assert np.array_equal(protos[1].cpu().numpy().view(np.int32), ref["inp"]["qfeat"][0].view(np.int32))
    if h.keep is not None:
        pk, wk = h.table(h.keep)
        assert _bits(wk, ws)  # pooling does not look at keep
        errs["proto:keep"] = R.rel(pk.cpu().numpy(), ref["f64"]["proto_keep"])
        ones, _ = h.table(torch.ones_like(h.keep))
        assert _bits(ones, protos)
    _, w1 = h.head("cosine")
    _, w2 = h.batched("cosine")
    assert _bits(w1, ws) and _bits(w2, ws)  # every route pools the same bits
    _hold(R.head_case_id(case), errs, R.head_e32(case))


@pytest.mark.parametrize("method", ["cosine", "euclidean"])
@pytest.mark.parametrize("case", R.HEAD_CASES, ids=R.head_case_id)
def test_head_every_route_against_float64(heads, case, method):
    """r3d_protonet_head, _head_batched, _head_keep_batched (NULL, ones, a pattern), _prototypes_batched + _similarity_batched
    (one system; one system per query cloud with proto_stride 0) and _similarity_sets (one table, stride 0) give the SAME
    bits (include/r3d.h) and those bits meet float64.  Rows 0 and 1 (equal to the class-1 prototype; 1e-5 from it) are held
    per entry under euclidean: the value comes from the eps alone.  Row 2 is zero: cosine exactly 0 (the 1e-8 floor).
    Measured on the MI355X (worst over the cases, keep included; worst chain-order e32 beside it): Zcos 6.11e-7 (1.35e-6),
    Zeuc 2.61e-7 (9.33e-7), Zeps 1.89e-7 (2.52e-6)."""
    h = heads(case)
    n_way, k_shot, N, n_q, D, _ = case
    ref = R.head_reference(case)
    Z1, _ = h.head(method)
    protos, _ = h.table()
    routes = dict(batched=h.batched(method)[0], keep_null=h.batched(method, None)[0],
                  two_calls=h.sim(protos, method), sets_one=h.sets(protos.view(-1), 0, method)[0])
    if h.keep is not None:
        routes["keep_ones"] = h.batched(method, torch.ones_like(h.keep))[0]
    if n_q > 1:
        routes["per_cloud"] = h.sim(protos, method, n_sys=n_q, stride=0)
    torch.cuda.synchronize()
    for name, Z in routes.items():
        assert _bits(Z, Z1), name
    got = h.cols(Z1)
    assert np.isfinite(got).all()
    errs = {ZBAR[method]: R.rel(got, ref["f64"]["Z"][method])}
    if method == "euclidean":
        errs["Zeps"] = R.rel_entry(got[:2, 1], ref["f64"]["Zeps"][method])
    else:
        assert (got[2] == 0).all()
    if h.keep is not None:
        Zk, _ = h.batched(method, h.keep)
        pk, _ = h.table(h.keep)
        assert _bits(h.sim(pk, method), Zk)
        errs[ZBAR[method] + ":keep"] = R.rel(h.cols(Zk), ref["f64"]["Z_keep"][method])
    _hold("%s %s" % (R.head_case_id(case), method), errs, R.head_e32(case))


@pytest.mark.parametrize("method", ["cosine", "euclidean"])
@pytest.mark.parametrize("case", R.HEAD_CASES, ids=R.head_case_id)
def test_head_similarity_sets(heads, case, method):
    """K = 3 tables at a stride larger than a table, and as many tables as fill 64 prototype rows where n_way + 1 divides
    64: set k's rows have the bits of r3d_protonet_similarity_batched on table k alone, and meet float64 similarity against
    the tables as given.  Measured on the MI355X: Zcos 6.11e-7 (K = 3), 4.37e-7 (K = 16); Zeuc 2.34e-7 (K = 16)."""
    h = heads(case)
    n_way, D = case[0], case[4]
    base, _ = h.table()
    second = h.table(h.keep)[0] if h.keep is not None else base * 0.5
    for K in [3] + ([64 // h.C] if 64 % h.C == 0 else []):
        tabs = [base, second, base.roll(1, 0)] + [base + 0.01 * k for k in range(3, K)]
        stride = h.C * D + 5
        flat = torch.full(((K - 1) * stride + h.C * D,), float("nan"), device="cuda")
        for k, t in enumerate(tabs):
            flat[k * stride:k * stride + h.C * D] = t.reshape(-1)
        Z, K_ = h.sets(flat, stride, method)
        assert K_ == K
        torch.cuda.synchronize()
        errs = {}
        for k, t in enumerate(tabs):
            Zk = Z[:, k * h.nqp:(k + 1) * h.nqp]
            assert _bits(Zk, h.sim(t.contiguous(), method)), (K, k)
            want = R.similarity(t.cpu().numpy(), R.head_reference(case)["inp"]["qfeat"], method)
            key = "%s:K%d" % (ZBAR[method], K)
            errs[key] = max(errs.get(key, 0.0), R.rel(h.cols(Zk), want))
        _hold("%s %s" % (R.head_case_id(case), method), errs, R.head_e32(case))


# ----------------------------------------------------------------------------------------------------------------------
# C. the integer reducers
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_pts", [1, 63, 64, 255, 256, 257, 1000])
def test_count_correct_batched(lib, n_pts):
    """E = 3 episodes: none correct, all correct, a random part; the labels of the random episode hold a value >= 2^31 whose
    low word equals the prediction there (a comparison in 32 bits would count it)."""
    rs = np.random.RandomState(n_pts)
    pred = rs.randint(0, 4, (3, n_pts)).astype(np.int32)
    lab = np.empty((3, n_pts), np.int64)
    lab[0], lab[1] = pred[0] + 1, pred[1]
    lab[2] = np.where(rs.rand(n_pts) < 0.5, pred[2], pred[2] + 2)
    lab[2, n_pts // 2] = (1 << 32) + int(pred[2, n_pts // 2])
    lab[2, 0] = (1 << 31) + 1
    want = (pred.astype(np.int64) == lab).sum(1)
    assert want[0] == 0 and want[1] == n_pts
    correct = torch.full((3,), -1, dtype=torch.int32, device="cuda")
    pred_d, lab_d = torch.from_numpy(pred).cuda(), torch.from_numpy(lab).cuda()
    _check(lib.r3d_count_correct_batched(3, _p(pred_d), _p(lab_d), n_pts, _p(correct), _st()))
    assert np.array_equal(correct.cpu().numpy().astype(np.int64), want), (correct, want)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 5000])
def test_miou_accumulate(lib, n):
    """n_lut 2 .. 8; labels and predictions outside [0, n_lut), negative included, are CLAMPED into the table (include/r3d.h);
    a second update adds to the first.  Against the numpy restatement, and against O.evaluate_metric where everything lies
    inside the table."""
    from oracle import r3d_oracle as O
    rs = np.random.RandomState(n)
    for n_lut in range(2, 9):
        n_classes = n_lut + 2
        test_classes = list(range(10, 10 + n_classes - 1))
        l2c = rs.choice(test_classes, n_lut - 1, replace=False)
        lut = np.array([0] + [test_classes.index(int(c)) + 1 for c in l2c], np.int32)
        # the table sits inside a buffer of the test's: the word after it is a valid class that is not the last entry's
        lut_dev = torch.from_numpy(np.concatenate((lut, np.zeros(1, np.int32)))).cuda()
        for lo, hi in ((0, n_lut), (-3, n_lut + 3)):
            hist = torch.zeros(3, n_classes, dtype=torch.int64, device="cuda")
            want, preds, gts = None, [], []
            for _ in range(2):
                pred, gt = rs.randint(lo, hi, n).astype(np.int32), rs.randint(lo, hi, n).astype(np.int64)
                preds.append(pred); gts.append(gt)
                pred_d, gt_d = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()
                _check(lib.r3d_miou_accumulate(_p(pred_d), _p(gt_d), n, _p(lut_dev), n_lut, n_classes, _p(hist), _st()))
                torch.cuda.synchronize()
                want = R.miou_hist(pred, gt, lut, n_classes, want)
            got = hist.cpu().numpy().astype(np.uint64)
            assert np.array_equal(got, want), (n, n_lut, lo, got, want)
            if lo == 0:
                _, iou = O.evaluate_metric(preds, gts, [l2c, l2c], test_classes)
                with np.errstate(invalid="ignore", divide="ignore"):
                    mine = got[2] / (got[0] + got[1] - got[2]).astype(np.float64)
                assert np.array_equal(mine, iou, equal_nan=True)
