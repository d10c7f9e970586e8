"""A support set fitted once, query clouds segmented against it as they arrive.

In .eval() mode BatchNorm uses running statistics and dropout is off, so what the support set contributes to an episode is
a fixed table: the prototypes of models/protonet.py:837-842,892-915 (ProtoNet, ProtoNet_Contrast) or the multi-prototype
node rows of models/mpti.py:488-489 (MPTI_SelfAtten).  model.fit_support(...) computes it and returns a FittedSupport that
owns the device tables -- no features, no support clouds --; model.predict(fitted, query_x) runs the query clouds through
the encoder and the query half of the head only.  The rule: predict on a query group gives THE SAME BITS as forward() on the
episode made of that support set and that group (tests/test_gpu_fitted.py).

A FittedSupport is bound to the weights it was fitted with.  Its key is, per parameter and buffer, the `_version` counter
(what DGCNN._fold keys its folded weights on) and the storage address, plus a 64-bit sum over the words of all of them: the
counters see optimizer steps, load_state_dict and every in-place operation on the tensors themselves, but a write through
`.data` has a version counter of its own and only the contents show it.  predict() recomputes the key -- for device
modules one concatenation, one sum and one host read -- and raises ValueError on a stale fit before it launches anything
of its own.

This module holds the host logic (argument checks, the key, the object); the launches are in protonet.py and mpti.py.
"""
import torch


def _tensors(module):
    return list(module.parameters()) + list(module.buffers())


def version_key(module):
    """(versions, addresses) of the module's parameters and buffers: host only, no device work."""
    ts = _tensors(module)
    return tuple(t._version for t in ts), tuple(t.data_ptr() for t in ts)


def content_sum(module):
    """64-bit sum of the 32-bit words of every parameter and buffer (one host read on a device module)."""
    with torch.no_grad():
        words = [t.detach().reshape(-1).view(torch.int32) for t in _tensors(module) if t.numel()]
        if not words:
            return 0
        return int(torch.cat(words).sum(dtype=torch.int64).item())


def model_key(module):
    return version_key(module) + (content_sum(module),)


class FittedHead:
    """The one-system head state of an MPTI fit: what r3d_head_attach_queries_batched reads.  nodes (proto_cap, D): the
    prototype rows (the first desc[HD_N_PROTO] are filled); Y: their label rows, label_rows per plane; desc (32,) int32;
    cluster_count (label_rows,) int32."""

    def __init__(self, nodes, Y, label_rows, desc, cluster_count, proto_cap):
        self.nodes, self.Y, self.label_rows, self.desc, self.cluster_count, self.proto_cap = \
            nodes, Y, label_rows, desc, cluster_count, proto_cap


class FittedSupport:
    """What fit_support returns.  protos: (1, n_way + 1, D) prototype table, background first (ProtoNet family) or None;
    head: FittedHead (MPTI) or None; shot_keep: (n_way * k_shot,) int32 if the clean-shot detection ran, else None;
    shape: (n_way, k_shot, in_channels, n_points); eval: the eval flag of the fit; schedule: 'default' or 'conservative'
    (fitted with lp_iters: one FPS launch per round); key: model_key of the model at fit time."""

    def __init__(self, model, protos=None, head=None, shot_keep=None, eval=False, schedule="default", n_queries=None):
        self.model_class = type(model).__name__
        self.model_id = id(model)
        self.shape = (model.n_way, model.k_shot, model.in_channels, model.n_points)
        self.protos, self.head, self.shot_keep = protos, head, shot_keep
        self.eval = bool(eval)
        self.schedule = schedule
        self.n_queries = n_queries
        self.key = model_key(model)

    def is_stale(self, model, key=None):
        """Why this fit no longer belongs to `model` (a string), or None.  key: model_key(model) taken by the caller, who
        checks several fits against one reading of the model (predict_scene_sets); default: read it here."""
        if id(model) != self.model_id or type(model).__name__ != self.model_class:
            return "it was fitted by another model object"
        vk = version_key(model) if key is None else key[:2]
        if vk != self.key[:2]:
            return "parameters or running statistics were updated or replaced since fit_support (version counters)"
        if (content_sum(model) if key is None else key[2]) != self.key[2]:
            return "parameter or running-statistic values changed in place since fit_support (content sum)"
        return None


def check_fit_args(model, support_x, support_y):
    """Raises before anything needs a device.  -> S = n_way * k_shot."""
    if model.training:
        raise NotImplementedError("fit_support is the inference path (running-statistics BatchNorm, no dropout: the support "
                                  "set's contribution is then a fixed table); call model.eval() first")
    want_x = (model.n_way, model.k_shot, model.in_channels, model.n_points)
    if not isinstance(support_x, torch.Tensor) or tuple(support_x.shape) != want_x:
        raise ValueError("fit_support: support_x must be (n_way, k_shot, in_channels, n_points) = %s, got %s"
                         % (want_x, tuple(support_x.shape) if isinstance(support_x, torch.Tensor) else type(support_x)))
    want_y = (model.n_way, model.k_shot, model.n_points)
    if not isinstance(support_y, torch.Tensor) or tuple(support_y.shape) != want_y:
        raise ValueError("fit_support: support_y must be (n_way, k_shot, n_points) = %s, got %s"
                         % (want_y, tuple(support_y.shape) if isinstance(support_y, torch.Tensor) else type(support_y)))
    return model.n_way * model.k_shot


def check_predict_args(model, fitted, query_x, query_y, key=None):
    """Raises before any launch.  -> (G, n_q, grouped): query_x is (n_q, C, N) -- one group, grouped False -- or
    (G, n_q, C, N).  key: see FittedSupport.is_stale."""
    if model.training:
        raise NotImplementedError("predict is the inference path; call model.eval() first")
    if not isinstance(fitted, FittedSupport):
        raise ValueError("predict: `fitted` must be what fit_support returned, got %s" % type(fitted).__name__)
    if not isinstance(query_x, torch.Tensor) or query_x.dim() not in (3, 4):
        raise ValueError("predict: query_x must be (n_q, in_channels, n_points) or (G, n_q, in_channels, n_points)")
    grouped = query_x.dim() == 4
    C, N = fitted.shape[2], fitted.shape[3]
    if tuple(query_x.shape[-2:]) != (C, N) or query_x.shape[-3] < 1 or (grouped and query_x.shape[0] < 1):
        raise ValueError("predict: query clouds of shape %s do not match the fit: (in_channels, n_points) = (%d, %d)"
                         % (tuple(query_x.shape), C, N))
    if fitted.shape != (model.n_way, model.k_shot, model.in_channels, model.n_points):
        raise ValueError("predict: the fit's episode shape %s is not this model's" % (fitted.shape,))
    if query_y is not None and tuple(query_y.shape) != tuple(query_x.shape[:-2]) + (N,):
        raise ValueError("predict: query_y of shape %s does not label query_x of shape %s"
                         % (tuple(query_y.shape), tuple(query_x.shape)))
    why = fitted.is_stale(model, key)
    if why is not None:
        raise ValueError("predict: stale fit -- %s; call fit_support again" % why)
    return (query_x.shape[0] if grouped else 1), query_x.shape[-3], grouped


class FittedSets(tuple):
    """K FittedSupports of one model, checked together (check_sets_args), as predict_scene_sets hands them to a launch.
    table: what the model's head reads them through, built on the first launch and kept for the call -- the (K, n_way + 1,
    D) prototype tables in one tensor (ProtoNet family) or the device table of addresses of ops.head_fit_table (MPTI)."""
    table = None


def check_sets_args(model, fits):
    """predict_scene_sets' `fits`, before anything needs a device: a non-empty list or tuple of FittedSupports of this
    model that hold its kind of table, K * (n_way + 1) <= 64, one schedule; every fit passes check_predict_args against ONE
    reading of the model's key (one host read for a device model, not K).  -> FittedSets."""
    if model.training:
        raise NotImplementedError("predict_scene_sets is the inference path; call model.eval() first")
    if not isinstance(fits, (list, tuple)) or len(fits) == 0:
        raise ValueError("predict_scene_sets: `fits` must be a non-empty list or tuple of what fit() returned, got %s"
                         % (type(fits).__name__ if not isinstance(fits, (list, tuple)) else "an empty one"))
    K, C = len(fits), model.n_way + 1
    if K * C > 64:
        raise ValueError("predict_scene_sets: %d support sets of %d classes make %d score columns (at most 64)" % (K, C, K * C))
    key = None
    query = torch.empty(1, 1, model.in_channels, model.n_points, device="meta")  # a shape, no memory
    for k, f in enumerate(fits):
        if isinstance(f, FittedSupport) and key is None:
            key = model_key(model)
        try:
            check_predict_args(model, f, query, None, key=key)
        except ValueError as e:
            raise ValueError("predict_scene_sets: fits[%d] -- %s" % (k, e)) from None
        if getattr(f, model.fit_table) is None:
            raise ValueError("predict_scene_sets: fits[%d] holds no %s (it was fitted by %s)"
                             % (k, "MPTI head state" if model.fit_table == "head" else "prototype table", f.model_class))
        if f.schedule != fits[0].schedule:
            raise ValueError("predict_scene_sets: fits[%d] was fitted on the %s schedule, fits[0] on the %s one"
                             % (k, f.schedule, fits[0].schedule))
    return FittedSets(fits)


def support_pair(data_or_support):
    """An episode list (entries 0 and 1) or a (support_x, support_y) pair -> (support_x, support_y)."""
    if len(data_or_support) < 2:
        raise ValueError("fit: an episode list or a (support_x, support_y) pair is needed")
    return data_or_support[0], data_or_support[1]


class FittedLearner(object):
    """fit() / predict() of the learners (needs self.model): annotate a handful of support clouds once, then label query
    clouds as they arrive.  test(), test_batch() and train*() are untouched by it."""

    fitted = None  # the FittedSupport of the latest fit()

    def fit(self, data_or_support, eval=False):
        """data_or_support: an episode list (entries 0 and 1 are used) or a (support_x, support_y) pair.  Stores and
        returns the FittedSupport."""
        support_x, support_y = support_pair(data_or_support)
        self.model.eval()
        with torch.no_grad():
            self.fitted = self.model.fit_support(support_x.cuda(), support_y.cuda(), eval=eval)
        return self.fitted

    def _predict_once(self, fitted, query_x, query_y, lp_iters=None):
        """-> (pred (G, n_q, N) int64, loss (G,) or None, correct (G,) int32 on the device or None)."""
        from . import ops
        grouped = check_predict_args(self.model, fitted, query_x, query_y)[2]
        qx = query_x if grouped else query_x[None]
        qy = query_y if (grouped or query_y is None) else query_y[None]
        logits, loss, pred = self.model._predict_groups(fitted, qx, qy, lp_iters)
        correct = ops.count_correct(pred, qy.to(torch.int64).contiguous()) if qy is not None else None
        return pred.to(torch.int64), (loss if qy is not None else None), correct

    def _predict_result(self, query_x, pred, loss, correct):
        n = query_x.shape[-3] * query_x.shape[-1]
        acc = [c / n for c in correct.tolist()] if correct is not None else [None] * pred.shape[0]  # (the call's host read)
        res = [(pred[g], loss[g] if loss is not None else None, acc[g]) for g in range(pred.shape[0])]
        return res if query_x.dim() == 4 else res[0]

    def predict(self, query_x, query_y=None, fitted=None):
        """query_x (n_q, C, N) -> (pred (n_q, N), loss, accuracy) with test()'s meaning, or (G, n_q, C, N) -> a list of G such
        tuples from ONE launch sequence; loss and accuracy are None without query_y.  fitted: default the latest fit()."""
        fitted = self._fitted_or_raise(fitted)
        self.model.eval()
        query_x = query_x.cuda()
        query_y = query_y.cuda() if query_y is not None else None
        with torch.no_grad():
            pred, loss, correct = self._predict_once(fitted, query_x, query_y)
        return self._predict_result(query_x, pred, loss, correct)

    def _scene_launch(self, fitted, query_x):
        """One launch of predict_scene: query_x (G, 1, C, N) -> (logits (G, 1, n_way + 1, N), redone)."""
        return self.model._predict_groups(fitted, query_x, None)[0], False

    def predict_scene(self, scan, block_size=1.0, stride=None, min_points=100, groups_per_launch=32, fitted=None,
                      max_chunks_per_block=None, transfer=None):
        """Label a whole scan -- (M, 6) rows `x y z r g b`, host or device; (M, 3) for a model without rgb -- against the
        fitted support set: scene.SceneResult with a label, the summed logits and the vote count per scan point
        (scene.py; INTEGRATION.md, "Labelling a scan").  fitted: default the latest fit().  max_chunks_per_block=c runs
        only c chunks of a block; transfer="nearest" labels the points without a vote from their nearest voted neighbour,
        transfer="idw" from the mean logits of the three nearest, weighted by inverse squared distance."""
        fitted = self._fitted_or_raise(fitted)
        self.model.eval()
        with torch.no_grad():
            return self.model.predict_scene(fitted, scan, block_size, stride, min_points, groups_per_launch,
                                            launch=self._scene_launch, max_chunks_per_block=max_chunks_per_block,
                                            transfer=transfer)

    def _scene_launch_sets(self, fits, query_x):
        """One launch of predict_scene_sets: query_x (G, 1, C, N) -> (logits (G, K * (n_way + 1), N), redone)."""
        return self.model._predict_groups_sets(fits, query_x).reshape(query_x.shape[0], -1, query_x.shape[-1]), False

    def predict_scene_sets(self, scan, fits, classes=None, block_size=1.0, stride=None, min_points=100, groups_per_launch=32,
                           max_chunks_per_block=None, transfer=None, background=-1):
        """Label a whole scan against K fitted support sets at once -- fits: a list of what fit() returned, K * (n_way + 1)
        <= 64 -- with ONE plan and ONE encoder pass per launch: scene.SceneSetsResult with, per set, the scores and labels
        predict_scene(scan, fitted=fits[k], ...) gives bit for bit, and one merged class id per point (scene.py;
        INTEGRATION.md, "Labelling a scan against several support sets").  classes: K sequences of n_way class ids, way w of
        set k is classes[k][w - 1]; default k * n_way + (w - 1).  background: the id of a labelled point no set claims; the
        default -1 is also the id of a point without a label -- `votes` and `set_labels` tell them apart.  The other
        arguments are predict_scene's; head memory of MPTI grows with K * groups_per_launch (scene.py)."""
        self.model.eval()
        with torch.no_grad():
            return self.model.predict_scene_sets(fits, scan, classes, block_size, stride, min_points, groups_per_launch,
                                                 launch=self._scene_launch_sets, max_chunks_per_block=max_chunks_per_block,
                                                 transfer=transfer, background=background)

    def pool_segments(self, res, segments, min_members=1, classes=None, background=-1):
        """One label per segment of a labelled scan: res is what predict_scene or predict_scene_sets returned, segments (M,)
        int32 or int64 ids of a partition of its points (instances, supervoxels; negative: in no segment; host or device).
        Per segment the mean logits of its voted points, summed in a fixed order, and their arg-max; every point of a
        segment with at least min_members voted points takes them, any other point keeps what res holds: a
        scene_segments.SegmentResult (scene_segments.py; INTEGRATION.md, "Pooling scores over segments").  classes and
        background: those of the predict_scene_sets call, for its result only.  Needs no fit and changes neither res nor the
        learner."""
        from . import scene_segments
        return scene_segments.pool_segments(res, segments, min_members, classes, background)

    def build_segments(self, scan, voxel=0.05, colour_tol=None, connectivity=6, min_points=1):
        """The segments pool_segments takes, grown from the scan itself: scan (M, 3) or (M, >= 6) float32 rows x y z [r g b],
        host or device.  Points fall into voxels of edge `voxel`; occupied voxels that touch (connectivity 6: by a face, 26:
        also by an edge or a corner) and, with colour_tol, whose mean colours differ by at most colour_tol in every channel
        are joined; a connected component with at least min_points points is a segment: a scene_grow.GrownSegments whose
        .segments goes to pool_segments as it is (scene_grow.py; INTEGRATION.md, "Building segments").  Needs no fit and no
        model."""
        from . import scene_grow
        return scene_grow.build_segments(scan, voxel, colour_tol, connectivity, min_points)

    def grow_segments(self, scan, voxel=0.05, colour_tol=None, connectivity=6, min_points=1, normal_tol=None):
        """build_segments with one more criterion, normal_tol: None, or the largest angle in degrees (0 .. 90) between the
        surface normals of two neighbouring voxels that still joins them -- so a floor and a wall, which touch, fall apart.
        A voxel's normal comes from the occupied voxels among the 27 around it; a voxel with fewer than 4 of them has none
        and stays alone.  Combines with colour_tol (both must hold) and needs no colour columns (scene_grow.py;
        INTEGRATION.md, "Building segments", G3c, G3n, G4)."""
        from . import scene_grow
        return scene_grow.grow_segments(scan, voxel, colour_tol, connectivity, min_points, normal_tol)

    def absorb_segments(self, scan, voxel=0.05, colour_tol=None, connectivity=6, min_points=1, normal_tol=None, absorb=0):
        """grow_segments with one more step, absorb: the number of rings, 0 .. 64, by which the voxels that min_points
        dropped -- with normal_tol the slivers along the edge between two planes -- are taken into the kept segment most
        of their neighbours belong to.  The segments and their ids are those of grow_segments; only -1s become ids
        (scene_grow.py; INTEGRATION.md, "Building segments", G6a)."""
        from . import scene_grow
        return scene_grow.absorb_segments(scan, voxel, colour_tol, connectivity, min_points, normal_tol, absorb)

    def smooth_scene(self, res, scan, voxel=0.05, connectivity=26, alpha=0.8, iterations=10, colour_tol=None):
        """The scores of a labelled scan propagated over its voxel graph, between predict_scene and extract_objects: res is
        what predict_scene returned, scan the scan it labels.  The voted logits are pooled per voxel of edge `voxel`, swept
        `iterations` times over the voxel adjacency graph (Z <- (1 - alpha) Y + alpha (mean of the neighbours' Z); a voxel
        without a voted point is filled from its neighbours, one ring a sweep) and spread back: a scene_smooth.SmoothResult,
        which is a SceneResult, so its .labels go to extract_objects and it goes to pool_segments as it is
        (scene_smooth.py; INTEGRATION.md, "Smoothing a labelled scan").  Needs no fit and no model and changes neither res
        nor the learner."""
        from . import scene_smooth
        return scene_smooth.smooth_scene(res, scan, voxel, connectivity, alpha, iterations, colour_tol)

    def extract_objects(self, scan, labels, voxel=0.05, connectivity=26, min_points=1, ignore=()):
        """Object instances from a labelled scan: labels (M,) int32 or int64 are the .labels of what predict_scene,
        predict_scene_sets or pool_segments returned, or ground truth (negative: no class; ignore: class ids that form no
        objects).  The points of one class in cells of edge `voxel` that touch are one object: a scene_objects.SceneObjects
        with the object of every point and, per object, its class, points, cells, box and centroid; its .objects goes to
        pool_segments as it is (scene_objects.py; INTEGRATION.md, "Objects from a labelled scan").  Needs no fit and no
        model."""
        from . import scene_objects
        return scene_objects.extract_objects(scan, labels, voxel, connectivity, min_points, ignore)

    def match_objects(self, pred, truth, pred_labels=None, truth_labels=None, iou=(0.25, 0.5, 0.75), ignore_unannotated=False):
        """How good the objects are: pred, truth (M,) int32 or int64 object ids of the same points (negative: in no object),
        e.g. the .objects of extract_objects on predicted and on true labels; with pred_labels and truth_labels (both or
        neither) only objects of one class are paired.  Pairs of objects that share a point, their IoU, every object's best
        partner and the mutual bests at the thresholds `iou`: a scene_match.ObjectMatch whose .summary holds precision,
        recall, F1 and panoptic quality per threshold and class (scene_match.py; INTEGRATION.md, "Matching objects against
        ground truth").  Needs no fit and no model."""
        from . import scene_match
        return scene_match.match_objects(pred, truth, pred_labels, truth_labels, iou, ignore_unannotated)

    def fit_scene(self, scan, labels, classes, block_size=1.0, stride=None, min_points=100, min_ratio=0.05, min_fg=100,
                  eval=False):
        """fit() from an annotated scan instead of cut-out clouds: scan as for predict_scene, labels (M,) int32 or int64
        class ids (host or device), classes: n_way distinct ints, way w = classes[w - 1].  Per way the k_shot blocks whose
        cloud holds most points of the class become the shots (scene_support.py; INTEGRATION.md, "Fitting from an annotated
        scan").  Stores the FittedSupport and returns the scene_support.SceneSupport that holds it; a way with fewer than
        k_shot eligible blocks raises ValueError and leaves the latest fit as it was."""
        self.model.eval()
        with torch.no_grad():
            sup = self.model.fit_scene(scan, labels, classes, block_size, stride, min_points, min_ratio, min_fg, eval=eval)
        self.fitted = sup.fitted
        return sup

    def _fitted_or_raise(self, fitted):
        fitted = self.fitted if fitted is None else fitted
        if fitted is None:
            raise ValueError("predict: no fitted support set -- call fit() first or pass fitted=")
        return fitted
