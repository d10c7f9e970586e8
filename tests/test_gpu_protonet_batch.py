"""ProtoNet on the batched path: r3d_protonet_head_batched (the evaluation head for E episodes in one launch pair) against
r3d_protonet_head episode by episode -- bit for bit --, and ProtoLearner.train_batch / test_batch against the per-episode
learner calls they stand for.

Bars of the learner comparisons are those tests/test_gpu_learner_batch.py holds MPTILearner_V3.train_batch / test_batch to:
pred torch.equal, loss 2e-5, accuracy exact; parameters after one Adam step within 1e-6 where the gradient is "solid"
(|g| >= 1e-3 max|g|: Adam turns an element whose gradient is rounding noise into a step of ~lr with the noise's sign) and
within 2.1e-3 everywhere; BatchNorm running statistics and num_batches_tracked exact."""
import ctypes
import os
import socket
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

pytestmark = pytest.mark.gpu


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


# ----------------------------------------------------------------------------- the kernels, through the C ABI
# (n_way, k_shot, D, N, n_q): D = 160 is not a multiple of 64 (channel clamp), n_way = 5 needs the second plane of label
# columns, N = 500 / 300 are not multiples of 64 (nor of the pooling loop's 8 rows in flight)
HEAD_CASES = [(2, 5, 192, 512, 2), (5, 1, 160, 500, 2), (2, 1, 160, 2048, 1), (5, 5, 192, 300, 1)]
E_HEAD = 3


def _head_problem(n_way, k_shot, D, N, n_q, seed):
    """E episodes in ONE feature matrix: a column slice of a wider matrix (leading dimension != D), per episode
    [support rows | query rows | 37 padding rows of NaN]; every episode has a shot without foreground and one that is all
    foreground."""
    gen = torch.Generator().manual_seed(seed)
    S, n_pts = n_way * k_shot, n_q * N
    ep_rows = S * N + n_pts + 37
    buf = torch.randn(E_HEAD * ep_rows, D + 12, generator=gen) + 0.5
    buf.view(E_HEAD, ep_rows, D + 12)[:, S * N + n_pts:] = float("nan")
    sy = (torch.rand(E_HEAD, n_way, k_shot, N, generator=gen) < 0.3).to(torch.int32)
    sy[:, 0, 0] = 0
    sy[:, -1, -1] = 1
    return buf.cuda()[:, 5:5 + D], sy.cuda(), ep_rows


@pytest.mark.parametrize("method", ["cosine", "euclidean"])
@pytest.mark.parametrize("case", range(len(HEAD_CASES)))
def test_batched_head_is_bit_identical_to_the_single_head(case, method):
    from r3dfsseg_amd import ops
    n_way, k_shot, D, N, n_q = HEAD_CASES[case]
    S, n_pts = n_way * k_shot, n_q * N
    feat, sy, ep_rows = _head_problem(n_way, k_shot, D, N, n_q, 300 + case)
    Zb = ops.protonet_head_batched(feat[:S * N], feat[S * N:], sy, n_way, k_shot, N, method, E_HEAD, ep_rows, n_pts)
    planes = 1 if n_way <= 3 else 2
    assert Zb.shape == (planes * E_HEAD * n_pts, 4)
    Zb = Zb.view(planes, E_HEAD, n_pts, 4)
    for e in range(E_HEAD):
        rows = feat[e * ep_rows:(e + 1) * ep_rows]
        Zs = ops.protonet_head(rows[:S * N], rows[S * N:S * N + n_pts], sy[e], n_way, k_shot, N, method).view(planes, n_pts, 4)
        assert torch.isfinite(Zs).all()
        assert torch.equal(Zb[:, e], Zs), (case, method, e, float((Zb[:, e] - Zs).abs().max()))
    assert torch.isfinite(Zb).all(), "padding rows must not leak into Z"
    # one episode through the batched entry point: the same bits again (and feat_ep_rows is not looked at)
    Z1 = ops.protonet_head_batched(feat[:S * N], feat[S * N:], sy[0], n_way, k_shot, N, method, 1, 0, n_pts)
    assert torch.equal(Z1.view(planes, n_pts, 4), Zb[:, 0])


def test_batched_head_refusals_launch_nothing():
    from r3dfsseg_amd import _lib
    lib = _lib.load()
    n_way, k_shot, D, N, n_q = 2, 1, 192, 64, 2
    S, n_pts, E = 2, 128, 2
    ep_rows = S * N + n_pts
    feat = torch.randn(E * ep_rows, D, device="cuda")
    sy = torch.ones(E * S, N, dtype=torch.int32, device="cuda")
    words = lib.r3d_protonet_head_ws_words(E, n_way, k_shot)
    assert words == E * S * 2 * 256
    ws = torch.empty(words + 4, device="cuda")
    Z = torch.full((E * n_pts, 4), -7.0, device="cuda")
    ok = dict(n_ep=E, sfeat=_p(feat), qfeat=_p(feat[S * N:]), rows=ep_rows, D=D, sy=_p(sy), n_way=n_way, method=0, Z=_p(Z), ws=_p(ws),
              words=words)

    def call(**over):
        a = dict(ok, **over)
        return lib.r3d_protonet_head_batched(a["n_ep"], a["sfeat"], D, a["qfeat"], D, a["rows"], a["D"], a["sy"], a["n_way"], k_shot,
                                             N, n_pts, a["method"], 10.0, a["Z"], a["ws"], a["words"], None)
    for over, text in ((dict(sfeat=None), b"null pointer"), (dict(sy=None), b"null pointer"), (dict(n_way=8), b"unsupported shape"),
                       (dict(D=257), b"unsupported shape"), (dict(method=2), b"Distance computation method (2) is unknown"),
                       (dict(n_ep=0), b"episodes"), (dict(n_ep=65536), b"episodes"), (dict(rows=S * N - 1), b"rows between them"),
                       (dict(words=words - 1), b"workspace"), (dict(ws=_p(ws[1:])), b"16-byte aligned")):
        assert call(**over) != 0, over
        assert text in lib.r3d_last_error_string(), (over, lib.r3d_last_error_string())
    torch.cuda.synchronize()
    assert (Z == -7.0).all(), "a refused call launches nothing"
    assert call() == 0
    torch.cuda.synchronize()
    assert not (Z == -7.0).any()


def test_count_correct_per_episode():
    from r3dfsseg_amd import ops
    gen = torch.Generator().manual_seed(5)
    pred = torch.randint(0, 3, (5, 2, 777), generator=gen, dtype=torch.int32).cuda()
    lab = torch.randint(0, 3, (5, 2, 777), generator=gen, dtype=torch.int64).cuda()
    lab[3] = pred[3]
    got = ops.count_correct(pred, lab)
    assert got.dtype == torch.int32 and got.tolist() == (pred == lab).sum(dim=(1, 2)).tolist() and got[3].item() == 2 * 777


# ----------------------------------------------------------------------------- learner
def _cfg(**over):
    from r3dfsseg_amd import synthetic as S
    return S.make_cfg(**dict(dict(n_way=2, k_shot=2, pc_npts=512, pretrain_checkpoint_path="synthetic", model_checkpoint_path=None,
                                  lr=1e-3, step_size=5000, gamma=0.5), **over))


def _learner(cfg, mode="train"):
    from r3dfsseg_amd.proto_learner import ProtoLearner
    return ProtoLearner(SimpleNamespace(**cfg), mode=mode)  # (attention dropout stays ON: p = 0.1)


def _episodes(cfg, seeds, train=True):
    from r3dfsseg_amd import synthetic as S
    out = []
    for s in seeds:
        data, _ = S.make_episode(cfg, seed=s, noise_ratio=0.5, train=train)
        out.append([t.cuda() for t in data])
    return out


def _by_hand_step(L, eps):
    """What train_batch stands for: E times {training forward of episode e, loss.backward() accumulating}, gradients divided
    by E, one Adam step.  Returns per-episode (loss, accuracy) and the mean gradient."""
    L.model.train()
    L.optimizer.zero_grad()
    res = []
    for ep in eps:
        logits, loss = L.model(ep[0], ep[1], ep[2], ep[3])
        loss.backward()
        res.append((float(loss.detach()), float((logits.argmax(1) == ep[3]).sum().item()) / ep[3].numel()))
    for p in L.model.parameters():
        p.grad.div_(len(eps))
    grad = torch.cat([p.grad.reshape(-1) for p in L.model.parameters()]).clone()
    L.optimizer.step()
    L.lr_scheduler.step()
    return res, grad


def _flat(model):
    return torch.cat([p.detach().reshape(-1) for p in model.parameters()])


def _assert_same_step(A, B, grad, what):
    """Parameters and BatchNorm buffers of two learners after steps that are equal up to the order of the sum over episodes:
    the split of tests/test_gpu_learner_batch.py (solid entries 1e-6, Adam's sign-noise entries 2.1e-3, buffers exact)."""
    pa, pb = _flat(A.model), _flat(B.model)
    solid = grad.abs() >= 1e-3 * grad.abs().max()
    d = (pa - pb).abs()
    print("%s: parameters max |diff| %.2e on the %d solid entries, %.2e on all %d" % (what, float(d[solid].max()), int(solid.sum()),
                                                                                   float(d.max()), d.numel()))
    assert d[solid].max().item() < 1e-6 and d.max().item() < 2.1e-3
    for (k, va), (_, vb) in zip(A.model.named_buffers(), B.model.named_buffers()):
        assert torch.equal(va, vb), k


def test_test_batch_equals_test_per_episode():
    cfg = _cfg(pretrain_checkpoint_path=None, model_checkpoint_path="synthetic")
    L = _learner(cfg, mode="test")
    eps = _episodes(cfg, range(60, 64), train=False)
    got = L.test_batch(eps, None)
    assert len(got) == 4
    b = L._batch(eps)
    with torch.no_grad():
        logits_b = L.model.forward_episodes(b)[0]
    for e, ep in enumerate(eps):
        pred, loss, acc = L.test(ep, None)
        with torch.no_grad():
            logits = L.model(ep[0], ep[1], ep[2], ep[3])[0]
        assert got[e][0].shape == pred.shape and got[e][0].dtype == pred.dtype and torch.equal(got[e][0], pred)
        assert got[e][2] == acc
        # The bars of tests/test_gpu_learner_batch.py would be 2e-5 on the loss.  Here every stage is bit-identical per episode:
        # the evaluation encoder over 4 (S + Q) clouds against S + Q clouds (kNN per cloud, row-independent GEMMs, attention
        # with its key split per episode), the batched head by construction, the logits / loss kernel per episode -- measured
        # on MI355X: 0.0 on loss and logits of all four episodes -- so the logits and the loss are held to equality.
        assert torch.equal(logits_b[e], logits)
        assert torch.equal(got[e][1], loss)


def test_train_batch_equals_the_by_hand_accumulated_step():
    cfg = _cfg()
    eps = _episodes(cfg, range(40, 44))
    A, B = _learner(cfg), _learner(cfg)
    want, grad = _by_hand_step(B, eps)
    got = A.train_batch(eps, None)
    assert len(got) == 4 and all(len(o) == 2 for o in got)
    for e, ((loss, acc), (wloss, wacc)) in enumerate(zip(got, want)):
        print("episode %d: loss %.6f (by hand %.6f), accuracy %.6f (by hand %.6f)" % (e, float(loss), wloss, acc, wacc))
        assert abs(float(loss) - wloss) < 2e-5 and acc == wacc and 0.0 <= acc <= 1.0
    ga = torch.cat([p.grad.reshape(-1) for p in A.model.parameters()])
    print("mean gradient: max |diff| / max |g| = %.2e" % (float((ga - grad).abs().max()) / float(grad.abs().max())))
    _assert_same_step(A, B, grad, "train_batch against by hand")
    assert int(A.model.encoder.conv.layer[1].num_batches_tracked.item()) == 8  # two getFeatures calls per episode
    for (k, va), (_, vb) in zip(A.model.named_buffers(), B.model.named_buffers()):
        if k.endswith("num_batches_tracked"):
            assert int(va) == int(vb) == 8, k
    assert A.lr_scheduler.last_epoch == 1 and A.model._drop_seed == B.model._drop_seed == 8
    # a conv bias in front of a training-mode BatchNorm keeps an exactly zero gradient (as test_learner_train_step asserts
    # for train()), so Adam leaves it where it is
    n = 0
    for k, p in A.model.named_parameters():
        if k.startswith("base_learner.convs") and k.endswith(".0.bias"):
            assert float(p.grad.abs().max()) == 0.0, k
            n += 1
    assert n == A.model.base_learner.num_convs >= 1


def test_train_batch_gradients_are_bit_identical_run_to_run():
    import copy
    cfg = _cfg()
    eps = _episodes(cfg, range(40, 43))
    L = _learner(cfg)
    state = copy.deepcopy(L.model.state_dict())
    opt = copy.deepcopy(L.optimizer.state_dict())
    L.train_batch(eps, None)
    g1 = L._batch_trainer.bucket.flat.clone()
    L.model.load_state_dict(state)
    L.optimizer.load_state_dict(opt)
    L.model._drop_seed = 0
    L.train_batch(eps, None)
    assert torch.equal(L._batch_trainer.bucket.flat, g1) and float(g1.abs().max()) > 0.0


def _assert_same_steps(A, B, grads, what):
    """_assert_same_step after several steps: an entry is solid when its gradient was solid in EVERY step (a sign flip in
    any one step moves it by 2 lr)."""
    solid = torch.ones_like(grads[0], dtype=torch.bool)
    for g in grads:
        solid &= g.abs() >= 1e-3 * g.abs().max()
    d = (_flat(A.model) - _flat(B.model)).abs()
    print("%s: parameters max |diff| %.2e on the %d solid entries, %.2e on all %d" % (what, float(d[solid].max()), int(solid.sum()),
                                                                                   float(d.max()), d.numel()))
    assert d[solid].max().item() < 1e-6 and d.max().item() < 2.1e-3
    # (from the second step on the two runs' weights differ in the last bits, and with them the batch statistics: the running
    # statistics are exact after ONE step from equal weights -- test_train_batch_equals_the_by_hand_accumulated_step -- and
    # here only their count is)
    for (k, va), (_, vb) in zip(A.model.named_buffers(), B.model.named_buffers()):
        if k.endswith("num_batches_tracked"):
            assert int(va) == int(vb), k


def test_train_and_train_batch_interleave_on_their_own_gradients():
    cfg = _cfg()
    eps = _episodes(cfg, range(40, 45))
    b1, e, b2 = eps[:2], eps[2], eps[3:5]
    A, B = _learner(cfg), _learner(cfg)
    A.train_batch(b1, None)
    A.train(e, None)
    A.test(e[:4] + [None, None, e[6]], None)  # an evaluation in between moves nothing
    A.train_batch(b2, None)
    grads = [_by_hand_step(B, b1)[1], _by_hand_step(B, [e])[1], _by_hand_step(B, b2)[1]]
    assert A.lr_scheduler.last_epoch == B.lr_scheduler.last_epoch == 3
    assert int(A.model.encoder.conv.layer[1].num_batches_tracked.item()) == 10
    _assert_same_steps(A, B, grads, "train_batch, train, train_batch against by hand")
    # and the other order: a train_batch() after a train() steps on the batch's gradient alone
    C, Dl = _learner(cfg), _learner(cfg)
    C.train(e, None)
    C.train_batch(b1, None)
    grads = [_by_hand_step(Dl, [e])[1], _by_hand_step(Dl, b1)[1]]
    _assert_same_steps(C, Dl, grads, "train, train_batch against by hand")


def test_python_refusals():
    cfg = _cfg()
    L = _learner(cfg)
    eps = _episodes(cfg, [40])
    with pytest.raises(ValueError, match="empty"):
        L.train_batch([], None)
    with pytest.raises(ValueError, match="empty"):
        L.test_batch([])
    cfg2 = _cfg(pc_npts=256)
    other = _episodes(cfg2, [41])
    with pytest.raises(ValueError, match="ONE shape"):
        L.train_batch([eps[0], other[0]], None)
    with pytest.raises(ValueError, match="ONE shape"):
        L.test_batch([eps[0], other[0]])
    lm = _learner(_cfg(use_attention=False))
    with pytest.raises(NotImplementedError, match="use_attention=False"):
        lm.train_batch(eps, None)


# ----------------------------------------------------------------------------- reference parity through the batch
@pytest.mark.parametrize("patched", [False, True], ids=["free", "patched"])
@pytest.mark.parametrize("method", ["cosine", "euclidean"])
def test_batch_of_the_golden_episode_twice_against_reference_outputs(method, patched):
    """The episode of tests/golden/protonet_train.npz twice in one batch (E = 2, dropout 0 as the generator): each episode's
    loss and logits, and the summed parameter gradients / 2, against the reference's own step at the bars of
    tests/test_gpu_protonet_train.py::test_protonet_training_step_against_reference_outputs."""
    from r3dfsseg_amd import protonet_train
    from r3dfsseg_amd.batch import EpisodeBatch
    from test_gpu_golden_head import _bars, _reference_near_tie_rows
    from test_gpu_protonet_train import _C_BARS, _train_model
    from test_protonet_train_golden import protonet_train_fixture
    cfg, sd, data, g = protonet_train_fixture()
    bar = _bars("protonet_train", patched, True)
    for k in ("dloss", "gnorm", "gmed", "gmax"):
        bar[k] = min(bar[k], _C_BARS[k])
    m = _train_model(cfg, sd, method)
    m._trace = None
    E = 2
    clouds = cfg["n_way"] * cfg["k_shot"] + data[2].shape[0]
    if patched:
        one = _reference_near_tie_rows(g, cfg["n_way"] * cfg["k_shot"])
        m.encoder.idx_patch = lambda layer, idx: torch.cat([one(layer, idx[e * clouds:(e + 1) * clouds]) for e in range(E)], 0)
    ep = [t.cuda() for t in data[:4]]
    params = [p for p in m.parameters() if p.requires_grad]
    sink = [torch.zeros_like(p) for p in params]
    loss, logits, pred, correct = protonet_train.explicit_train_batch(m, EpisodeBatch.from_episodes([ep, ep]), sink)
    pre = method + "/"
    ref = torch.from_numpy(g[pre + "logits"])
    tag = "protonet batch %s %s" % (method, "patched" if patched else "free")
    for e in range(E):
        lg = logits[e].detach().cpu()
        err = (lg - ref).abs() / ref.abs().clamp(min=1.0)
        frac = float((err <= 1e-4).float().mean())
        agree = float((lg.argmax(1) == ref.argmax(1)).float().mean())
        dloss = abs(float(loss[e]) - float(g[pre + "loss"]))
        print("%s episode %d: logits within 1e-4: %.4f (max %.2e), arg-max agreement %.4f, |loss - ref| %.2e"
              % (tag, e, frac, float(err.max()), agree, dloss))
        assert frac >= bar["frac"] and agree >= bar["agree"] and dloss <= bar["dloss"]
        assert bar["emax"] is None or float(err.max()) <= bar["emax"]
        assert torch.equal(pred[e].cpu().to(torch.int64), lg.argmax(1))
        assert int(correct[e]) == int((pred[e].cpu().to(torch.int64) == data[3]).sum())
    assert torch.equal(logits[0], logits[1]) and torch.equal(loss[0], loss[1])  # the same episode: the same bits
    rel = {}
    for (pname, p), gsum in zip(m.named_parameters(), sink):
        gn = float(g[pre + "gnorm/" + pname])
        gv = (gsum / E).reshape(-1).cpu().double()
        pick, want = g[pre + "gpick/" + pname], g[pre + "gval/" + pname]
        e_ = float(np.linalg.norm(gv.numpy()[pick] - want) / max(np.linalg.norm(want), 1e-12))
        if gn < 1e-6:  # a conv bias in front of a training-mode BatchNorm: identically zero; the reference leaves rounding noise
            assert float(gv.norm()) < 1e-6, pname
            rel[pname] = (0.0, 0.0)
            continue
        rel[pname] = (abs(float(gv.norm()) - gn) / max(gn, 1e-12), e_)
    assert len(rel) == 35
    wn = max(v[0] for v in rel.values())
    ws_ = sorted(v[1] for v in rel.values())
    print("%s: gradient norms max rel diff %.2e; sampled entries rel-L2 median %.2e max %.2e" % (tag, wn, ws_[len(ws_) // 2], ws_[-1]))
    assert wn <= bar["gnorm"] and ws_[len(ws_) // 2] <= bar["gmed"] and ws_[-1] <= bar["gmax"], \
        {k: v for k, v in rel.items() if v[0] > bar["gnorm"] or v[1] > bar["gmed"]}


# ----------------------------------------------------------------------------- two ranks on one device
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    from r3dfsseg_amd import dist as D
    assert D.init("gloo") == world
    torch.cuda.set_device(0)
    cfg = _cfg()
    eps = _episodes(cfg, range(40, 44))
    L = _learner(cfg)
    # this rank's two episodes are episodes 2 rank, 2 rank + 1 of the step: the dropout seeds one rank would hand them
    L.model._drop_seed = 4 * rank
    res = L.train_batch(eps[2 * rank:2 * rank + 2], None)
    torch.cuda.synchronize()
    out[rank] = dict(params=_flat(L.model).cpu(), grad=L._batch_trainer.bucket.flat.cpu(), loss=[float(r[0]) for r in res],
                     acc=[r[1] for r in res])
    torch.distributed.destroy_process_group()


def test_two_ranks_of_train_batch_equal_one_rank():
    cfg = _cfg()
    eps = _episodes(cfg, range(40, 44))
    L = _learner(cfg)
    res = L.train_batch(eps, None)
    torch.cuda.synchronize()
    want_params, want_grad = _flat(L.model).cpu(), L._batch_trainer.bucket.flat.cpu()
    want = [(float(r[0]), r[1]) for r in res]
    del L
    torch.cuda.empty_cache()
    world, port = 2, _free_port()
    with mp.get_context("spawn").Manager() as mgr:  # (never fork a process that has touched the GPU)
        out = mgr.dict()
        mp.spawn(_rank_worker, args=(world, port, out), nprocs=world, join=True)
        out = dict(out)
    assert torch.equal(out[0]["grad"], out[1]["grad"]) and torch.equal(out[0]["params"], out[1]["params"])
    for r in range(2):
        for i in range(2):
            assert abs(out[r]["loss"][i] - want[2 * r + i][0]) < 2e-5 and out[r]["acc"][i] == want[2 * r + i][1]
    solid = want_grad.abs() >= 1e-3 * want_grad.abs().max()
    d = (out[0]["params"] - want_params).abs()
    print("two ranks against one: gradient max |diff| / max |g| %.2e; parameters max |diff| %.2e solid, %.2e all"
          % (float((out[0]["grad"] - want_grad).abs().max()) / float(want_grad.abs().max()), float(d[solid].max()), float(d.max())))
    assert d[solid].max().item() < 1e-6 and d.max().item() < 2.1e-3
