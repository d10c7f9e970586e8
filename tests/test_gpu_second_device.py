"""What the library remembers about a kernel belongs to a DEVICE (csrc/error.hip: r3d_kernel_lds, r3d_kernel_resident): the
dynamic LDS a kernel has been allowed is set on the current device's copy of it, and the workgroups a chip holds at once
size every grid whose workgroups wait for each other.  A process that has served device 0 must ask again on device 1.

Each case runs on device 0 first -- the order that fills a process-wide memory with device 0's answers -- and then, from
the same host inputs, under torch.cuda.device(1).  The ops raise on any return code but R3D_OK (a refused launch is such a
return, not a device fault), and the outputs of device 1 must have the bits of device 0's.  Shapes: the smallest that still
need what is remembered --
  * label propagation at D = 256 (tests/cg_cases.py "d256", 205 nodes): r3d_cg_aggregate_kernel asks for
    (64 * 257 + 4 * 256) * 4 = 69 888 B of dynamic LDS whatever n is, above the 64 KiB a kernel gets unasked; the LDS form of
    the SpMV is forced, which sizes its grid by the resident count;
  * episode_cut_partial at N = 8192: 128 KiB of dynamic LDS, on a pool of one block of 8192 points;
  * ops.edgeconv at B = 1, N = 64, K = 20: a persistent grid sized by the resident count.
With fewer than two devices the module skips."""
import numpy as np
import pytest
import torch

import cg_cases as CC
from test_gpu_cg_coarse import LDS, _buffers, _load
from test_gpu_episode_partial import _Hand, _rows

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two devices in one process")]


def _label_propagation(ops):
    from r3dfsseg_amd import _lib
    lib = _lib.load()
    c = CC.get("d256")
    assert c.D == 256 and (64 * (c.D | 1) + 4 * c.D) * 4 == 69888 > 64 * 1024
    hb = _buffers(ops, c.n_cap, c.D, 1)
    nbr = _load(ops, hb, [c])
    old = lib.r3d_debug_set_cg_spmv_lds_min_blocks(LDS)
    try:
        Z = ops.label_propagate(hb, nbr, CC.SIGMA, CC.ALPHA, 300, 1e-6)
        torch.cuda.synchronize()
    finally:
        lib.r3d_debug_set_cg_spmv_lds_min_blocks(old)
    agg, MW, Einv, _ = hb.coarse(0)
    stats = hb.stats[0].cpu()
    assert stats[0] == 1, "not converged: %s" % stats.tolist()
    return dict(Z=Z[:c.n].cpu(), stats=stats, agg=agg.cpu(), MW=MW.cpu(), Einv=Einv.cpu())


CUT_N, CUT_CLASS = 8192, 5


def _episode_cut_partial(ops):
    from r3dfsseg_amd.block_pool import ATTRIB_SETS, BlockPool
    rs = np.random.RandomState(0)
    block = _rows(rs.choice([CUT_CLASS, 7, 0], CUT_N), rs.randint(-20, 20, CUT_N), 9)
    pool = BlockPool.from_source(_Hand({"big": block}, {CUT_CLASS: ["big"]}), instances=True)
    dev = pool.device
    C, rgb_ch, XYZ_ch = ATTRIB_SETS["xyzrgbXYZ"]
    mk = lambda *s, dt: torch.full(s, -7, device=dev, dtype=dt)
    out = dict(x=mk(1, C, CUT_N, dt=torch.float32), mask=mk(1, CUT_N, dt=torch.int32), gt_mask=mk(1, CUT_N, dt=torch.int32),
               slot_map=mk(1, CUT_N, dt=torch.int32), info=mk(1, 8, dt=torch.int32))
    none = torch.empty(0, CUT_N, device=dev, dtype=torch.int64)
    desc = torch.tensor([[0, CUT_CLASS, 0, 6, 5]], dtype=torch.int32, device=dev)   # one support cloud, partial noise
    classes = torch.tensor([[CUT_CLASS]], dtype=torch.int32, device=dev)
    ops.episode_cut_partial(pool.points, pool.labels, pool.offsets, desc, classes, 1, 0, CUT_N, 9, out["x"], rgb_ch, XYZ_ch,
                            out["mask"], out["gt_mask"], none, none, out["slot_map"], pool.instances, out["info"])
    torch.cuda.synchronize()
    assert out["info"][0, 3].item() & 1, "no object was flipped: the partial path did not run"
    return {k: v.cpu() for k, v in out.items()}


def _edgeconv(ops):
    B, N, K = 1, 64, 20
    g = torch.Generator().manual_seed(3)
    PQ = torch.randn(B * N, 128, generator=g)
    idx = torch.randint(0, N, (B, N, K), generator=g, dtype=torch.int32)
    W2 = torch.randn(64, 64, generator=g) / 8
    s2, t2 = torch.randn(64, generator=g), torch.randn(64, generator=g)
    out = torch.full((B * N, 64), float("nan"), device="cuda")
    am = ops.edgeconv(PQ.cuda(), idx.cuda(), W2.cuda(), s2.cuda(), t2.cuda(), out, B, N, want_argmax=True)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    return dict(out=out.cpu(), argmax=am.cpu())


@pytest.mark.parametrize("case", [_label_propagation, _episode_cut_partial, _edgeconv], ids=lambda f: f.__name__.strip("_"))
def test_device_1_after_device_0(case):
    from r3dfsseg_amd import ops
    got = []
    for dev in (0, 1):
        with torch.cuda.device(dev):
            got.append(case(ops))
    for k, a in got[0].items():
        b = got[1][k]
        assert a.dtype == b.dtype and a.shape == b.shape, k
        bits = (lambda t: t.view(torch.int32)) if a.dtype == torch.float32 else (lambda t: t)
        assert torch.equal(bits(a), bits(b)), "%s: device 1 differs from device 0" % k
