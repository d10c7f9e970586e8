"""Build the support set from an annotated scan, on the device.

fit() takes (n_way, k_shot, C, pc_npts) clouds and binary masks that the reference's loader cut out of a room, sampled,
min-shifted and normalised on the host (dataloaders/loader.py:202-352, eligibility from dataloaders/s3dis.py:55-70).
fit_scene takes the room itself -- the (M, 6) rows predict_scene takes -- and a class id per point, and builds those clouds
and masks with the plan, the chunk rule and the arithmetic of predict_scene.  The reference has no such function, so the
behaviour is defined here ("Fitting from an annotated scan"; tests/scene_support_ref.py restates it in
numpy).  It draws no random number: the same inputs give the same bits.

  S1. the plan of predict_scene, without a cap                                  scene.ScenePlan       host reads 1, 2
  S2. the cloud of a kept block: its chunk 0 -- list positions 0, nc, 2 nc, ..., len = ceil(n / nc) members,
      slot t = member t mod len
  S3. fg[b, w]: the members of block b's cloud labelled classes[w - 1]          r3d_scene_support_counts
  S4. thr[b] = max((int)floorf((float)len * min_ratio), min_fg); way w's shots are the blocks with fg > thr, by fg
      descending, then block id ascending, the first k_shot                     r3d_scene_support_pick   host read 3
  S5. support_x[w, i] = the prepared cloud of block shot_block[w, i], chunk 0; support_y[w, i, t] =
      (labels[slot_map[w, i, t]] == classes[w - 1])                             r3d_scene_prepare_blocks
      then model.fit_support(support_x, support_y, eval=eval), unchanged

This module holds the host logic; the kernels are csrc/scene.hip."""
import numbers

import numpy as np
import torch

from . import ops, scene

INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


class SceneSupport:
    """What fit_scene returns.  fitted: the FittedSupport (also stored in learner.fitted).  On the device: support_x
    (n_way, k_shot, C, N) fp32; support_y (n_way, k_shot, N) int32, 1 where the slot's point carries the way's class;
    shot_block, shot_fg (n_way, k_shot) int32: the chosen blocks and their foreground counts; slot_map (n_way, k_shot, N)
    int32: the scan index in every slot.  n_eligible: a host list, the eligible blocks of every way."""

    def __init__(self, fitted, support_x, support_y, shot_block, shot_fg, slot_map, n_eligible):
        self.fitted, self.support_x, self.support_y = fitted, support_x, support_y
        self.shot_block, self.shot_fg, self.slot_map, self.n_eligible = shot_block, shot_fg, slot_map, n_eligible


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def check_support_args(model, scan, labels, classes, block_size, stride, min_points, min_ratio, min_fg):
    """Raises before anything needs a device.  -> (scan and labels as tensors, classes as a list of ints, r, s, rgb_ch,
    XYZ_ch)."""
    if model.training:
        raise NotImplementedError("fit_scene is the inference path; call model.eval() first")
    scan, r, s, rgb_ch, XYZ_ch = scene.check_scene_args(model, scan, block_size, stride, min_points, 1)
    if isinstance(labels, np.ndarray):
        labels = torch.from_numpy(labels)
    if not isinstance(labels, torch.Tensor) or tuple(labels.shape) != (scan.shape[0],):
        raise ValueError("fit_scene: labels must be (M,) = (%d,), one class id per scan point, got %s"
                         % (scan.shape[0], tuple(labels.shape) if isinstance(labels, torch.Tensor) else type(labels).__name__))
    if labels.dtype not in (torch.int32, torch.int64):
        raise ValueError("fit_scene: labels must be int32 or int64, got %s" % labels.dtype)
    try:
        classes = list(classes)
    except TypeError:
        raise ValueError("fit_scene: classes must be %d distinct ints, got %r" % (model.n_way, classes))
    if len(classes) != model.n_way or not all(_is_int(c) for c in classes) or len(set(int(c) for c in classes)) != len(classes):
        raise ValueError("fit_scene: classes must be n_way = %d distinct ints (way w is classes[w - 1]), got %r"
                         % (model.n_way, classes))
    classes = [int(c) for c in classes]
    if len(classes) > ops.SCENE_SUPPORT_MAX_WAYS:
        raise ValueError("fit_scene: %d ways (at most %d)" % (len(classes), ops.SCENE_SUPPORT_MAX_WAYS))
    for c in classes:
        if c < INT32_MIN or c > INT32_MAX:
            raise ValueError("fit_scene: class id %d does not fit in int32" % c)
    if isinstance(min_ratio, bool) or not isinstance(min_ratio, numbers.Real) or not (0.0 <= float(min_ratio) < 1.0) \
            or not np.float32(min_ratio) < 1.0:
        raise ValueError("fit_scene: min_ratio %r must be a number in [0, 1)" % (min_ratio,))
    if not _is_int(min_fg) or min_fg < 0 or min_fg > INT32_MAX:
        raise ValueError("fit_scene: min_fg %r must be an integer >= 0" % (min_fg,))
    return scan, labels, classes, r, s, rgb_ch, XYZ_ch


def count_and_pick(plan, labels, classes_dev, k_shot, min_ratio, min_fg):
    """S3 and S4 on the device -> (fg (blocks, n_way), shot_block, shot_fg, rec (8,)); nothing is read back."""
    fg = ops.scene_support_counts(plan.M, *plan._geometry(), labels, classes_dev)
    return (fg,) + ops.scene_support_pick(plan.M, *plan._geometry(), fg, k_shot, min_ratio, min_fg)


def check_eligible(n_eligible, classes, k_shot):
    """S4's error: a way with fewer than k_shot eligible blocks."""
    for w, (n, c) in enumerate(zip(n_eligible, classes)):
        if n < k_shot:
            raise ValueError("fit_scene: way %d (class id %d) has %d eligible block%s, k_shot = %d are needed (a block is "
                             "eligible when its cloud holds more than max(floor(len * min_ratio), min_fg) points of the class)"
                             % (w + 1, c, n, "" if n == 1 else "s", k_shot))


def prepare_shots(plan, shot_block, labels, classes_dev, C, rgb_ch, XYZ_ch, out=None):
    """S5 on the device: shot_block (n_way, k_shot) -> (support_x (n_way, k_shot, C, N), support_y (n_way, k_shot, N) int32,
    slot_map (n_way, k_shot, N) int32).  out: a (n_way * k_shot, C, N) buffer in the layout wanted (default contiguous)."""
    n_way, k_shot = shot_block.shape
    S, N, dev = n_way * k_shot, plan.N, plan.scan.device
    if out is None:
        out = torch.empty(S, C, N, device=dev, dtype=torch.float32)
    slot_map = torch.empty(S, N, device=dev, dtype=torch.int32)
    mask = torch.empty(S, N, device=dev, dtype=torch.int32)
    cloud_class = classes_dev.repeat_interleave(k_shot).contiguous()
    ops.scene_prepare_blocks(plan.scan, *plan._geometry(), shot_block.reshape(S), out, rgb_ch, XYZ_ch, slot_map, labels,
                             cloud_class, mask)
    return out.view(n_way, k_shot, C, N), mask.view(n_way, k_shot, N), slot_map.view(n_way, k_shot, N)


def fit_scene(model, scan, labels, classes, block_size=1.0, stride=None, min_points=100, min_ratio=0.05, min_fg=100, eval=False):
    """model.fit_scene: see the module text.  -> SceneSupport."""
    scan, labels, classes, r, s, rgb_ch, XYZ_ch = check_support_args(model, scan, labels, classes, block_size, stride,
                                                                     min_points, min_ratio, min_fg)
    scan, labels = scan.cuda(), labels.cuda().contiguous()
    classes_dev = torch.tensor(classes, dtype=torch.int32, device=scan.device)
    plan = scene.ScenePlan(scan, model.n_points, block_size, stride, min_points)
    fg, shot_block, shot_fg, rec = count_and_pick(plan, labels, classes_dev, model.k_shot, min_ratio, int(min_fg))
    n_eligible = rec[:model.n_way].tolist()  # the one host read this adds to the plan's two
    check_eligible(n_eligible, classes, model.k_shot)  # before the encoder runs
    support_x, support_y, slot_map = prepare_shots(plan, shot_block, labels, classes_dev, model.in_channels, rgb_ch, XYZ_ch)
    fitted = model.fit_support(support_x, support_y, eval=eval)
    return SceneSupport(fitted, support_x, support_y, shot_block, shot_fg, slot_map, n_eligible)
