"""Training augmentation (--pc_augm) of prepared clouds on the device.

The reference augments on the host, inside its block sampler (dataloaders/loader.py:205-213 calls augment_pointcloud,
loader.py:354-373, between the min-shift and the XYZ channels).  A prepared cloud still holds that min-shifted xyz in
channels 0-2, so the same function can run on clouds that are already resident on the device (EpisodeBatch, EpisodeFeeder
over cached .h5 files): scale, z-rotation, mirrors and clipped Gaussian jitter on xyz, XYZ recomputed from the result, rgb
copied.  One kernel launch (csrc/augment.hip), no host pass and no copy.

Random numbers: stateless.  A cloud's matrix and jitter are a function of (seed, cloud key); the cloud key of cloud i
(x_all order: S support clouds, then Q query clouds) of the episode with counter c is c * (S + Q) + i.  A batch of E
episodes starting at counter c therefore equals E single calls with counters c, c + 1, ... bit for bit -- the convention
the dropout seeds follow.  The Gaussian is the library's own, not numpy's stream.

The host-side restatement of the same transform (python `random` / numpy streams, float64) is
episode_sampler.augment_pointcloud."""
import torch

from . import ops

CFG_KEYS = ("scale", "rot", "mirror_prob", "jitter")


def config_from_args(args):
    """The reference's PC_AUGMENT_CONFIG (mpti_train_noise.py:29-33) with its argparse defaults (:202-209)."""
    return {"scale": getattr(args, "pc_augm_scale", 0), "rot": getattr(args, "pc_augm_rot", 1),
            "mirror_prob": getattr(args, "pc_augm_mirror_prob", 0), "jitter": getattr(args, "pc_augm_jitter", 1)}


def _like(x):
    """An uninitialised tensor of x's shape and layout (point-major views stay point-major views)."""
    if ops.is_point_major_view(x):
        return torch.empty(x.transpose(-1, -2).shape, device=x.device, dtype=torch.float32).transpose(-1, -2)
    return torch.empty(x.shape, device=x.device, dtype=torch.float32)


def augment_clouds(x, cfg, seed, first_key=0, XYZ_ch=None, mats=None, noise=None, out=None, return_mats=False,
                   seed_dev=None):
    """x (B, C, N) fp32 on the device, contiguous channel-major or a point-major view (ops.input_layouts) -> the augmented
    clouds in the same layout.  cfg: the reference's dict {'scale', 'rot', 'mirror_prob', 'jitter'}.  Cloud b draws from
    (seed, first_key + b).  XYZ_ch: first of the normalised XYZ channels (default: 6 for 9 channels, none otherwise).
    mats (B, 9) / noise (B, N, 3): use these matrices / this jitter instead of drawing them.  out: where to write (x
    itself is allowed).  return_mats: also return the (B, 9) matrices used."""
    missing = [k for k in CFG_KEYS if k not in cfg]
    if missing:
        raise KeyError("pc_augm config lacks %s" % missing)
    if x.dim() != 3 or not x.is_cuda:
        raise ValueError("augment_clouds: x must be a (B, C, N) tensor on the device, got %s" % (tuple(x.shape),))
    if x.dtype != torch.float32:
        x = x.float()
    if not (ops.is_point_major_view(x) or x.is_contiguous()):
        x = x.contiguous()
    B, C, N = x.shape
    if XYZ_ch is None:
        XYZ_ch = 6 if C == 9 else -1
    if out is None:
        out = _like(x)
    dev = x.device
    mats = None if mats is None else torch.as_tensor(mats, dtype=torch.float32, device=dev).reshape(B, 9).contiguous()
    noise = None if noise is None else torch.as_tensor(noise, dtype=torch.float32, device=dev).reshape(B, N, 3).contiguous()
    mats_out = torch.empty(B, 9, device=dev, dtype=torch.float32) if return_mats else None
    ops.augment_clouds(x, out, cfg["scale"], cfg["rot"], cfg["mirror_prob"], cfg["jitter"], seed, first_key, 0, XYZ_ch,
                       seed_dev=seed_dev, mats=mats, noise=noise, mats_out=mats_out)
    return (out, mats_out) if return_mats else out


def augment_episode(data, cfg, seed, counter):
    """data: a train- or test-layout list (loader.py:1666-1671 / 1679-1683) -> a new list whose entries 0 and 2 (support
    and query clouds) are augmented copies on the device; every other entry is passed on as it is.  The background
    clouds of the train layout (entry 8) are left alone: no model here reads them.  Cloud keys: counter * (S + Q) +
    index, support clouds first (x_all order)."""
    sx, qx = data[0].cuda(), data[2].cuda()
    C, N = sx.shape[-2], sx.shape[-1]
    S, Q = sx.numel() // (C * N), qx.shape[0]
    key0 = int(counter) * (S + Q)
    out = list(data)
    out[0] = augment_clouds(sx.reshape(S, C, N), cfg, seed, key0).reshape(sx.shape)
    out[2] = augment_clouds(qx, cfg, seed, key0 + S)
    return out


def augment_batch(b, cfg, seed, counter):
    """EpisodeBatch.augmented: one launch over the E (S + Q) clouds of b.x_all; episode e uses counter + e."""
    E, SQ, C, N = b.x_all.shape
    x_all = augment_clouds(b.x_all.reshape(E * SQ, C, N), cfg, seed, int(counter) * SQ).reshape(E, SQ, C, N)
    new = object.__new__(type(b))
    new.__dict__.update(b.__dict__)
    S = SQ - b.query_x.shape[1]
    new.x_all = x_all
    # support_x / query_x keep what EpisodeBatch promises of them (dense, in x_all's layout): two device copies.  The
    # training launch sequences read the clouds through x_all alone.
    if ops.is_point_major_view(x_all):
        dense = lambda t: t.transpose(-1, -2).contiguous().transpose(-1, -2)
    else:
        dense = lambda t: t.contiguous()
    new.support_x = dense(x_all[:, :S]).reshape(b.support_x.shape)
    new.query_x = dense(x_all[:, S:])
    return new


class LearnerAugment:
    """The learners' switch: ``args.device_augm`` (default absent / False) turns the device augmentation on for train() /
    train_batch() when ``args.pc_augm`` is set too, with the reference's ``args.pc_augm_scale / _rot / _mirror_prob /
    _jitter`` and the seed ``args.device_augm_seed`` (default 0).  Deliberately NOT ``args.pc_augm`` alone: the
    reference's datasets already augment on the host under that flag, and honouring it blindly would augment twice.
    Each learner owns one of these, and with it its own episode counter."""

    def __init__(self, args):
        self.on = bool(getattr(args, "device_augm", False)) and bool(getattr(args, "pc_augm", False))
        self.seed = int(getattr(args, "device_augm_seed", 0) or 0)
        self.cfg = config_from_args(args)
        self.counter = 0

    def episode(self, data):
        if not self.on:
            return data
        data = augment_episode(data, self.cfg, self.seed, self.counter)
        self.counter += 1
        return data

    def batch(self, b):
        if not self.on:
            return b
        out = augment_batch(b, self.cfg, self.seed, self.counter)
        self.counter += b.E
        return out
