"""Episodes cut on the device from a resident pool of labelled blocks (definition: INTEGRATION.md, "Cutting episodes on
the device").

The reference turns block files into episodes on the host: per cloud two `np.random.choice` calls and a gather
(dataloaders/loader.py:219-237), 10 to 16 clouds per episode.  Here the blocks live on the device (`BlockPool`), the
episode PLAN -- which blocks, which noisy shots, which flags: a few dozen integers -- is still made on the host by the
rules of `episode_sampler.episode_rules` (`EpisodePlanner`), and ONE kernel launch (csrc/episode_cut.hip) cuts all
E (S + Q) clouds of a batch into an `EpisodeBatch` (`DeviceEpisodeSampler`).

The random stream of the point draws is this library's own (the stateless hash of the device augmentation, keyed by
(seed, cloud key)), not numpy's; tests/episode_cut_ref.py restates it in numpy and the kernel is held to it bit for bit.
Partial noise (noise_type="partial": a noisy shot is a block of the way's own class with one wrong OBJECT flipped into its
mask and, with probability 0.3, one right object taken out; loader.py:239-322, 741-779) needs a pool built with
instances=True: the planner answers the reference's "poor block" re-draw from the pool's books, the mask edit is steps
P0-P7 of the definition in the same launch (r3d_episode_cut_partial; tests/episode_partial_ref.py restates it), and
EpisodeBatch.partial_info records per cloud what was flipped and dropped.
Not here: the four background clouds of the train layout (no model here reads them, EpisodeBatch does not carry them)."""
import numpy as np
import torch

from . import ops
from .episode_sampler import episode_rules

MAX_BLOCK_POINTS = ops.CUT_MAX_BLOCK_POINTS
FLAG_QUERY, FLAG_GT_ZERO, FLAG_PARTIAL = ops.CUT_FLAG_QUERY, ops.CUT_FLAG_GT_ZERO, ops.CUT_FLAG_PARTIAL
ATTRIB_SETS = {"xyz": (3, -1, -1), "xyzrgb": (6, 3, -1), "xyzXYZ": (6, -1, 3), "xyzrgbXYZ": (9, 3, 6)}  # C, rgb_ch, XYZ_ch


class BlockPool:
    """The blocks of a source, concatenated: points (T, 6) fp32 rows x y z r g b, labels (T,) int32, offsets
    (n_blocks + 1,) int64 on `device`; on the host names, index[name], class2scans restricted to the pooled names and
    count(block, cls), the points of class cls in a block (one bincount per block, taken while the array is in hand).
    Built with instances=True also: instances (T,) int32 on `device`, the object id of every point (the LAST column of a
    block, as the reference indexes it: data[:, -1]), and on the host n_objects / n_classes (n_blocks,), the distinct object
    ids / labels of every block.  Without: instances, n_objects and n_classes are None."""

    def __init__(self, points, labels, offsets, names, class2scans, counts, instances=None, n_objects=None, n_classes=None):
        self.points, self.labels, self.offsets = points, labels, offsets
        self.instances, self.n_objects, self.n_classes = instances, n_objects, n_classes
        self.names = list(names)
        self.index = {n: i for i, n in enumerate(self.names)}
        self.class2scans = class2scans
        self._counts = counts                       # per block {class: points}
        self.sizes = np.diff(offsets.cpu().numpy())  # host copy of the block sizes

    @staticmethod
    def from_source(source, names=None, device="cuda", instances=False):
        """source: any object with load(name) -> (n, >= 7) rows x y z r g b label ... and a class2scans dict (the contract of
        SyntheticBlocks and of the reference's block files).  names: the blocks to pool (default: every name listed in
        class2scans, in order of first appearance).  instances: also pool the object ids, the last of >= 8 columns."""
        if names is None:
            names = list(dict.fromkeys(str(n) for c in source.class2scans for n in source.class2scans[c]))
        names = [str(n) for n in names]
        if not names or len(set(names)) != len(names):
            raise ValueError("BlockPool: %d names, %d distinct (need at least one, each once)" % (len(names), len(set(names))))
        pts, labs, counts, offsets = [], [], [], [0]
        insts, n_obj, n_cls = [], [], []
        for name in names:
            blk = np.asarray(source.load(name))
            if blk.ndim != 2 or blk.shape[1] < 7:
                raise ValueError("BlockPool: block %s has shape %s (rows x y z r g b label ...)" % (name, blk.shape))
            n = blk.shape[0]
            if not 1 <= n <= MAX_BLOCK_POINTS:
                raise ValueError("BlockPool: block %s has %d points (1 .. 2^20)" % (name, n))
            lab = blk[:, 6]
            li = lab.astype(np.int64)
            if not (np.all(np.isfinite(lab)) and np.all(li == lab) and li.min() >= -2 ** 31 and li.max() < 2 ** 31):
                raise ValueError("BlockPool: block %s has a label that is not an int32" % name)
            ids, cnt = np.unique(li, return_counts=True)  # (a bincount that also takes negative ids)
            counts.append({int(i): int(k) for i, k in zip(ids, cnt)})
            if instances:
                if blk.shape[1] < 8:
                    raise ValueError("BlockPool: block %s has shape %s (instances=True: rows x y z r g b label ... instance)"
                                     % (name, blk.shape))
                ins = blk[:, -1]
                ii = ins.astype(np.int64)
                if not (np.all(np.isfinite(ins)) and np.all(ii == ins) and ii.min() >= -2 ** 31 and ii.max() < 2 ** 31):
                    raise ValueError("BlockPool: block %s has an instance id that is not an int32" % name)
                insts.append(ii.astype(np.int32))
                n_obj.append(len(np.unique(ii)))
                n_cls.append(len(ids))
            pts.append(blk[:, :6].astype(np.float32))
            labs.append(li.astype(np.int32))
            offsets.append(offsets[-1] + n)
            if offsets[-1] >= 2 ** 31:
                raise ValueError("BlockPool: %d points in all (fewer than 2^31)" % offsets[-1])
        pooled = set(names)
        c2s = {c: [str(n) for n in v if str(n) in pooled] for c, v in source.class2scans.items()}
        dev = torch.device(device)
        return BlockPool(torch.from_numpy(np.concatenate(pts)).to(dev), torch.from_numpy(np.concatenate(labs)).to(dev),
                         torch.tensor(offsets, dtype=torch.int64).to(dev), names, c2s, counts,
                         *((torch.from_numpy(np.concatenate(insts)).to(dev), np.array(n_obj), np.array(n_cls))
                           if instances else ()))

    def __len__(self):
        return len(self.names)

    @property
    def device(self):
        return self.points.device

    def count(self, block, cls):
        """Points of class cls in block (an index or a name)."""
        b = self.index[block] if isinstance(block, str) else int(block)
        return self._counts[b].get(int(cls), 0)

    def size(self, block):
        b = self.index[block] if isinstance(block, str) else int(block)
        return int(self.sizes[b])


def share(nv, n, N):
    """m_A, the points the cloud's class keeps (loader.py:227-231, Python floats as there)."""
    return nv if n < N else int(nv / float(n) * N)


class EpisodePlan:
    """One episode's plan: desc (S + Q, 5) int32 rows {block, share_class, m_A, flags, key} in x_all order (the key column
    is filled when the plan is cut: key = counter * (S + Q) + i), sampled_classes (n_way,), support_flag (n_way, k_shot)."""

    def __init__(self, desc, sampled_classes, support_flag, n_way, k_shot, n_queries):
        self.desc, self.sampled_classes, self.support_flag = desc, sampled_classes, support_flag
        self.n_way, self.k_shot, self.n_queries = n_way, k_shot, n_queries

    def keyed(self, counter):
        d = self.desc.copy()
        d[:, 4] = ((int(counter) * len(d) + np.arange(len(d))) & 0xffffffff).astype(np.uint32).view(np.int32)
        return d


class EpisodePlanner:
    """NoiseEpisodeSampler's rules (episode_sampler.episode_rules: one code for both) over a BlockPool, recording a
    descriptor where the host sampler cuts a cloud.  It draws from the same host stream in the same order for the plan;
    the per-cloud point draws are not taken from it, so its stream differs from the host sampler's from the first cloud on."""

    def __init__(self, pool, classes, n_way=2, k_shot=5, n_queries=1, num_point=2048, mode="test", noise_ratio=0.4,
                 noise_type="sym", noise_pair_dict=None, seed=0):
        if mode not in ("train", "test"):
            raise NotImplementedError("Unkown mode %s! [Options: train/test]" % mode)
        if mode == "train":
            noise_type = "train"
            if not isinstance(noise_ratio, list):
                raise ValueError("train mode draws its noise ratio from a list")
        if noise_type == "partial" and pool.instances is None:
            raise NotImplementedError("partial noise flips whole objects into the mask, which needs instance ids: build the "
                                      "pool with BlockPool.from_source(..., instances=True), or let "
                                      "episode_sampler.NoiseEpisodeSampler do it on the host")
        if noise_type not in ("train", "sym", "ood", "pair", "partial"):
            raise NotImplementedError("noise type %s" % noise_type)
        self.pool, self.classes = pool, np.array(classes)
        self.n_way, self.k_shot, self.n_queries, self.num_point = n_way, k_shot, n_queries, num_point
        self.mode, self.noise_ratio, self.noise_type, self.noise_pair_dict = mode, noise_ratio, noise_type, noise_pair_dict
        self.rng = np.random.RandomState(seed)

    def sample_classes(self):
        return self.rng.choice(self.classes, self.n_way, replace=False)  # loader.py:618

    def plan(self, sampled_classes=None):
        sc = np.array(sampled_classes) if sampled_classes is not None else self.sample_classes()
        pool, N = self.pool, self.num_point

        def cut(scans, cls, support, partial):
            if partial:  # the mask is edited, not shared out: a uniform sample (loader.py:222-223), steps P0-P7
                return [[pool.index[str(s)], int(cls), 0, FLAG_PARTIAL] for s in scans]
            out = []
            for s in scans:
                b = pool.index[str(s)]
                m_A = share(pool.count(b, cls), pool.size(b), N)
                if support and m_A == 0:  # the mask would be empty: the reference asserts against it (loader.py:350)
                    raise ValueError("block %s keeps no point of class %d in a cloud of %d (it holds %d of %d points): a "
                                     "support mask may not be empty" % (s, cls, N, pool.count(b, cls), pool.size(b)))
                out.append([b, int(cls), m_A, 0 if support else FLAG_QUERY])
            return out

        def poor(name):  # loader.py:755-763, from the pool's books: no block is loaded
            b = pool.index[str(name)]
            return pool.n_objects[b] < 3 or pool.n_classes[b] < 3

        def stuck(cls, candidates):  # where the reference's re-draw loop would never end
            if all(poor(s) for s in candidates):
                raise ValueError("class %d: every one of its %d unused blocks has fewer than 3 objects or fewer than 3 "
                                 "classes: no block to draw a partial-noise shot from" % (cls, len(candidates)))

        ways, black, _ = episode_rules(self.rng, self.classes, pool.class2scans, sc, self.k_shot, self.n_queries, self.mode,
                                       self.noise_ratio, self.noise_type, self.noise_pair_dict, cut, poor, stuck)
        rows = [[d[0], d[1], d[2], d[3] | (FLAG_GT_ZERO if z else 0), 0] for shots, gt_zero, _, _ in ways
                for d, z in zip(shots, gt_zero)]
        rows += [d + [0] for _, _, _, queries in ways for d in queries]
        self.last_black_list = black
        return EpisodePlan(np.array(rows, np.int32).reshape(-1, 5), sc.astype(np.int32),
                           np.stack([w[2] for w in ways]).astype(np.int32), self.n_way, self.k_shot, self.n_queries)


class DeviceEpisodeSampler:
    """Episodes as EpisodeBatch objects on the pool's device.  batch(E): E plans on the host, ONE descriptor upload, ONE
    launch; gt_support_y, gt_query_y and support_flag are filled, .sampled_classes is (E, n_way) on the host, .slot_map
    (E, S + Q, N) int32 the pool row of every point, .partial_info (E, S + Q, 8) int32 under noise_type="partial" (per cloud
    {K, e, f, did, o_flip, n_flip, o_drop, n_drop}, step P7; None otherwise).  The cloud key of cloud i of the episode with
    counter c is c (S + Q) + i, the convention of augment.py: a batch at counter c equals E single cuts at c, c + 1, ... bit
    for bit; the counter advances by E per batch, as the augmentation's does.  layout: "cm" contiguous channel-major
    clouds, "pm" point-major rows handed on as (.., C, N) views, which the encoder reads as they lie."""

    def __init__(self, pool, classes, n_way=2, k_shot=5, n_queries=1, num_point=2048, mode="test", noise_ratio=0.4,
                 noise_type="sym", noise_pair_dict=None, seed=0, pc_attribs="xyzrgbXYZ", layout="cm"):
        if pc_attribs not in ATTRIB_SETS:
            raise ValueError("pc_attribs %r (one of %s)" % (pc_attribs, ", ".join(ATTRIB_SETS)))
        if layout not in ("cm", "pm"):
            raise ValueError("layout %r ('cm' or 'pm')" % layout)
        self.planner = EpisodePlanner(pool, classes, n_way, k_shot, n_queries, num_point, mode, noise_ratio, noise_type,
                                      noise_pair_dict, seed)
        self.pool, self.seed, self.pc_attribs, self.layout = pool, int(seed), pc_attribs, layout
        self.n_way, self.k_shot, self.n_queries, self.num_point = n_way, k_shot, n_queries, num_point
        self.counter = 0

    def plan(self, sampled_classes=None):
        return self.planner.plan(sampled_classes)

    def batch(self, E, counter=None):
        return self.cut([self.plan() for _ in range(E)], counter)

    def check(self, desc):
        """The host's view of the kernel's own checks: raises before anything is launched."""
        pool, N = self.pool, self.num_point
        S, Q = self.n_way * self.k_shot, self.n_way * self.n_queries
        for i, (b, c, m_A, flags, _) in enumerate(desc.tolist()):
            if not 0 <= b < len(pool):
                raise ValueError("cloud %d: block %d outside the pool of %d" % (i, b, len(pool)))
            if flags & FLAG_PARTIAL and (self.planner.noise_type != "partial" or pool.instances is None or flags & FLAG_QUERY
                                         or i % (S + Q) >= S or m_A != 0):  # P0
                raise ValueError("cloud %d: flags %d ask for partial noise, which is cut only by a partial-noise sampler over a "
                                 "pool with instance ids, on a support cloud with m_A == 0 (m_A %d)" % (i, flags, m_A))
            if not 0 <= m_A <= min(N, pool.count(b, c)):
                raise ValueError("cloud %d: m_A %d outside 0 .. min(N %d, the %d points of class %d in block %s)"
                                 % (i, m_A, N, pool.count(b, c), c, pool.names[b]))

    def cut(self, plans, counter=None):
        from .batch import EpisodeBatch
        if counter is None:
            counter = self.counter
            self.counter += len(plans)
        pool, N, E = self.pool, self.num_point, len(plans)
        n_way, k_shot = self.n_way, self.k_shot
        S, Q = n_way * k_shot, n_way * self.n_queries  # clouds per episode: n_queries query clouds per way
        if not pool.points.is_cuda:
            raise RuntimeError("DeviceEpisodeSampler.cut: the pool is on %s; the cut is a HIP kernel (there is no host "
                               "fallback: NoiseEpisodeSampler is the host sampler)" % pool.device)
        for p in plans:
            if (p.n_way, p.k_shot, p.n_queries) != (n_way, k_shot, self.n_queries):
                raise ValueError("a plan of another episode shape")
        desc = np.concatenate([p.keyed(int(counter) + e) for e, p in enumerate(plans)])
        self.check(desc)
        classes = np.stack([p.sampled_classes for p in plans]).astype(np.int32)
        dev = pool.device
        host = torch.from_numpy(np.concatenate([desc.reshape(-1), classes.reshape(-1)]))  # one upload
        both = host.to(dev)
        desc_d, classes_d = both[:desc.size].view(-1, 5), both[desc.size:].view(E, n_way)
        C, rgb_ch, XYZ_ch = ATTRIB_SETS[self.pc_attribs]
        B = E * (S + Q)
        if self.layout == "pm":
            x = torch.empty(B, N, C, device=dev, dtype=torch.float32).transpose(1, 2)
        else:
            x = torch.empty(B, C, N, device=dev, dtype=torch.float32)
        mask = torch.empty(E * S, N, device=dev, dtype=torch.int32)
        gt_mask = torch.empty_like(mask)
        qy = torch.empty(E * Q, N, device=dev, dtype=torch.int64)
        gt_qy = torch.empty_like(qy)
        slot_map = torch.empty(B, N, device=dev, dtype=torch.int32)
        info = None
        if self.planner.noise_type == "partial":
            info = torch.empty(B, 8, device=dev, dtype=torch.int32)
            ops.episode_cut_partial(pool.points, pool.labels, pool.offsets, desc_d, classes_d, S, Q, N, self.seed, x, rgb_ch,
                                    XYZ_ch, mask, gt_mask, qy, gt_qy, slot_map, pool.instances, info)
        else:
            ops.episode_cut(pool.points, pool.labels, pool.offsets, desc_d, classes_d, S, Q, N, self.seed, x, rgb_ch, XYZ_ch,
                            mask, gt_mask, qy, gt_qy, slot_map)
        flag = torch.from_numpy(np.stack([p.support_flag for p in plans])).to(dev)
        b = EpisodeBatch.from_x_all(x.unflatten(0, (E, S + Q)) if self.layout == "cm" else
                                    x.transpose(1, 2).unflatten(0, (E, S + Q)).transpose(2, 3),
                                    n_way, k_shot, mask.view(E, n_way, k_shot, N), qy.view(E, Q, N),
                                    gt_mask.view(E, n_way, k_shot, N), gt_qy.view(E, Q, N), flag)
        b.sampled_classes = classes
        b.slot_map = slot_map.view(E, S + Q, N)
        b.partial_info = info.view(E, S + Q, 8) if info is not None else None
        b.plans = list(plans)
        return b
