"""Host-side mirror of the reference's models/mpti.py::MPTI_SelfAtten.

Same constructor (an argparse-style ``args`` namespace, models/mpti.py:46-83), same
forward() signature and return values (models/mpti.py:414-415, 573-577) and the same
state-dict keys, so it drops into MPTILearner_V3 / mpti_train_noise.py / eval_noise.py.
All tensor work runs in libr3d_hip.so; this file only orders the launches.
"""
import torch
import torch.nn as nn

from . import ops
from .dgcnn import EpisodeSlot, FewShotFeatures  # noqa: F401  (EpisodeSlot: batched.py and episode_graph.py import it from here)


class MPTI_SelfAtten(FewShotFeatures):
    fit_table = "head"  # the field of a fitted.FittedSupport this model's predict reads

    def __init__(self, args):
        super().__init__(args)
        self.n_subprototypes = args.n_subprototypes
        self.k_connect = args.k_connect
        self.sigma = args.sigma
        self.n_classes = self.n_way + 1
        self.shot_seed = getattr(args, "shot_seed", 1)
        self.proj = nn.Linear(self.feat_dim, 128)
        # solver knobs of the sparse label propagation (no reference counterpart: the reference
        # inverts the dense matrix, mpti.py:775)
        self.lp_max_iter = getattr(args, "lp_max_iter", 200)
        self.lp_tol = getattr(args, "lp_tol", 1e-6)
        self.shot_level_clean_ratio = 0
        # CG launch budget: iterations are enqueued without knowing when the solver converges
        # (no host sync in forward).  The budget follows the iteration count observed on earlier
        # episodes (read back asynchronously); callers that synchronise anyway (learner.test)
        # call lp_converged() and re-run with the full lp_max_iter in the rare miss.
        self._lp_budget = min(32, self.lp_max_iter)
        self._lp_probe = None
        self._lp_force = False  # True: the conservative schedule (full CG budget, exact 201-NN kernel, FPS per round)
        # parity tests only: callable (nbr (E, n_cap, k + 1) int32) -> nbr that replaces rows of the device's own 201-NN
        # lists (the reference's choice on its near-tie rows, tests/test_gpu_golden_head.py); None in every product path
        self.nbr_patch = None

    # ------------------------------------------------------------------ head buffers
    @property
    def _head(self):
        return self._slot.last

    def _head_buffers(self, n_q, device, E=1):
        """The head buffers of E episodes (one set per (shape, batch size) and slot, kept between calls)."""
        key = (n_q, str(device), E)
        slot = self._slot
        if key not in slot.heads:
            keep = {k: v for k, v in slot.heads.items() if k[2] != E}  # one single-episode and one batched set stay
            keep[key] = ops.HeadBuffers(self.n_way, self.k_shot, self.n_points, n_q * self.n_points,
                                        self.n_subprototypes, self.k_connect, self.feat_dim, device, E=E)
            slot.heads = keep
        slot.heads[key].fps_one_launch = slot.fps_one_launch
        slot.last = (key, slot.heads[key])
        return slot.heads[key]

    def _lp_next_budget(self):
        if self._lp_force:
            return self.lp_max_iter
        if self._slot.fixed_budget is not None:
            return min(self.lp_max_iter, self._slot.fixed_budget)
        if self._lp_probe is not None:
            host, ev = self._lp_probe
            if ev.query():
                h = host.view(-1, 2)  # one {converged, iterations} pair per system of the batch
                conv, iters = int(h[:, 0].min()), int(h[:, 1].max())
                if conv:  # (half as many again + 8: a launch after convergence costs ~2.5 us, a miss redoes the whole step)
                    self._lp_budget = min(self.lp_max_iter, max(16, iters + iters // 2 + 8))
                else:
                    self._lp_budget = min(self.lp_max_iter, self._lp_budget * 2)
                self._lp_probe = None
        return self._lp_budget

    def _lp_post(self, hb):
        if self._slot.fixed_budget is not None:  # frozen launch sequence: convergence is checked by the graph owner
            return
        if self._lp_probe is None:
            host = torch.empty(hb.stats.numel(), dtype=torch.int32, pin_memory=True)
            host.copy_(hb.stats.view(-1), non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self._lp_probe = (host, ev)

    def lp_converged(self, backward=False):
        """Host check (synchronises): did the last forward's label propagation converge AND did the
        201-NN append kernel stay inside its survivor buffer AND did the one-launch FPS finish?  False -> call
        forward again with lp_iters=self.lp_max_iter (which also selects the always-exact insertion kNN kernel).
        backward=True: the adjoint solve of the last backward pass must have converged as well."""
        bad, overflow = self._head[1].status(backward)[:2].tolist()  # one device-to-host copy
        return bad == 0 and overflow == 0

    # ------------------------------------------------------------------ forward (mpti.py:414-577)
    def forward(self, support_x, support_y, query_x, query_y, gt_support_y=None, gt_query_y=None, train=False,
                logger=None, step=None, path=None, sampled_classes=None, bg_pcd_x=None, bg_pcd_y=None,
                support_c=None, support_flag=None, pcd_1024=None, label_1024=None, pcd_cutout=None,
                label_cutout=None, eval=False, lp_iters=None):
        self._lp_force = bool(lp_iters)
        if train:  # the reference keys the 7-tuple / contrastive path on this argument alone (mpti.py:465,573)
            if not self.training:
                raise NotImplementedError("train=True needs model.train(): the training kernels use batch-statistics "
                                          "BatchNorm and attention dropout (models/mpti_learner.py:58-63)")
            from . import head_train
            return head_train.mpti_train_forward(self, support_x, support_y, query_x, query_y, gt_support_y,
                                                 gt_query_y, logger, support_flag)
        if self.training:
            raise NotImplementedError("train=False on a model in .train() mode (batch-statistics BatchNorm in an "
                                      "inference forward) is not built; call model.eval() first as "
                                      "models/mpti_learner.py:93 does")
        logits, loss = self._forward_eval(support_x[None], support_y[None], query_x[None],
                                          query_y[None] if query_y is not None else None, eval, lp_iters)
        return logits[0], loss[0]

    def forward_episodes(self, batch, eval=False, lp_iters=None):
        """Inference forward of the E episodes of `batch` (batch.EpisodeBatch) in ONE launch sequence -> (logits
        (E, n_q, n_way + 1, N), loss (E,)): per episode what forward(..., eval=eval) returns for it (a capability of this
        build; the reference evaluates one episode per call, eval_noise.py:85-91).  lp_converged() then speaks for every
        system of the batch."""
        if self.training:
            raise NotImplementedError("forward_episodes is the inference path; training batches go through "
                                      "batched.EpisodeBatchRunner / head_train.explicit_train_batch")
        self._lp_force = bool(lp_iters)
        return self._forward_eval(batch.support_x, batch.support_y, batch.query_x, batch.query_y, eval, lp_iters)

    # ------------------------------------------------------------------ a support set fitted once (fitted.py)
    def fit_support(self, support_x, support_y, eval=False, lp_iters=None, n_queries=None):
        """The support half of _forward_eval, once: encoder over the S support clouds, clean-shot detection (eval=True), FPS,
        assignment and cluster means -> fitted.FittedSupport owning the prototype rows, their labels, desc and cluster
        counts of ONE system.  lp_iters: fit on the conservative schedule (one FPS launch per round).  One host read, as
        test(): a persistent-FPS time-out refits with one launch per round, so the table is never one lp_converged() would
        have rejected.  n_queries: see ProtoNet.fit_support."""
        from . import fitted as F
        S, N = F.check_fit_args(self, support_x, support_y), self.n_points
        sx = support_x.reshape(S, self.in_channels, N)
        feat = self.getFeatures_pm(sx, group=S + (n_queries or self.n_way))
        shot_keep = ops.clean_shot_detect(feat, sx, support_y, self.n_way, self.k_shot, N) if eval else None
        # a head of one system whose only "query" row is a support row it was given: the prototype half is all that is kept
        hb = ops.HeadBuffers(self.n_way, self.k_shot, N, 1, self.n_subprototypes, self.k_connect, self.feat_dim, feat.device)
        hb.fps_one_launch = self._slot.fps_one_launch and not lp_iters
        sy = support_y.reshape(1, S, N).to(torch.int32).contiguous()
        ops.head_prototypes(hb, sy, shot_keep, feat, feat)
        if int(hb.desc[0, ops.HD_FPS_TIMEOUT].item()) != 0:  # (the fit's host read)
            hb.fps_one_launch = False
            ops.head_prototypes(hb, sy, shot_keep, feat, feat)
        cap = hb.n_cap - 1
        head = F.FittedHead(hb.nodes[:cap], hb.Y, hb.n_cap, hb.desc[0], hb.cluster_count[0], cap)
        return F.FittedSupport(self, head=head, shot_keep=shot_keep, eval=eval,
                               schedule="conservative" if lp_iters else "default", n_queries=n_queries)

    def _predict_groups(self, fitted, query_x, query_y, lp_iters=None):
        """query_x (G, n_q, C, N), query_y (G, n_q, N) or None -> logits (G, n_q, n_way + 1, N), loss (G,), pred (G, n_q, N)
        int32: G systems [fitted prototypes | group g's query rows] in one launch sequence; the graph, the label
        propagation and the logits are _forward_eval's."""
        self._lp_force = bool(lp_iters)
        G, n_q, N = query_x.shape[0], query_x.shape[1], self.n_points
        feat = self._query_features(query_x)
        hb = self._head_buffers(n_q, feat.device, G)
        ops.head_attach_queries(hb, fitted.head, feat)
        labels = query_y.reshape(G, n_q, N).to(torch.int64).contiguous() if query_y is not None else None
        logits, loss, pred = self._attached_head(hb, n_q, labels, lp_iters)
        return logits.reshape(G, n_q, self.n_classes, N), loss.reshape(G), pred.reshape(G, n_q, N)

    def _propagate(self, hb, exact, lp_iters=None):
        """From the node matrices of hb's E systems to their Z, in eval, predict and training (head_train.lp_forward) alike:
        the 201-NN graph (exact: the insertion kernel), then the label propagation on lp_iters or the budgeted number of
        CG iterations -> the budget used (the adjoint solve sizes its own from it)."""
        nbr = ops.knn_nodes(hb, exact=exact)
        if self.nbr_patch is not None:
            nbr = self.nbr_patch(nbr)
        if self._trace is not None:
            self._trace["nbr"] = nbr
        budget = lp_iters or self._lp_next_budget()
        ops.label_propagate(hb, nbr, self.sigma, 0.99, budget, self.lp_tol)
        self._lp_post(hb)
        return budget

    def _attached_head(self, hb, n_q, query_y, lp_iters):
        """What follows the node matrices in _forward_eval, _predict_groups and _predict_groups_sets: the graph, the label
        propagation and the logits of hb's E systems, one launch sequence -> query_logits_ce's (logits, loss, pred).
        query_y: (E, n_q, N) labels or None."""
        self._propagate(hb, bool(lp_iters), lp_iters)
        labels = query_y.reshape(hb.E, n_q, hb.N).to(torch.int64).contiguous() if query_y is not None else None
        self.num_prototypes_dev = hb.desc[:, ops.HD_N_PROTO]
        return ops.query_logits_ce(hb, n_q, self.n_classes, labels)

    def _predict_groups_sets(self, fits, query_x, lp_iters=None):
        """_predict_groups against K fitted systems with ONE encoder pass and ONE head sequence: fits: fitted.FittedSets (or
        a list of FittedSupports), query_x (G, n_q, C, N) -> logits (G, K, n_q, n_way + 1, N); [:, k] has the bits of
        _predict_groups(fits[k], query_x, None, lp_iters).  The K * G systems [prototypes of fit k | query rows of group g]
        are ordered group-major (system g * K + k) in a HeadBuffers of E = K * G; lp_converged() then speaks for all."""
        from . import fitted as F
        fits = fits if isinstance(fits, F.FittedSets) else F.FittedSets(fits)
        self._lp_force = bool(lp_iters)
        G, n_q, N, K = query_x.shape[0], query_x.shape[1], self.n_points, len(fits)
        feat = self._query_features(query_x)
        if fits.table is None:
            fits.table = ops.head_fit_table([f.head for f in fits], feat.device)
        hb = self._head_buffers(n_q, feat.device, G * K)
        ops.head_attach_queries_sets(hb, [f.head for f in fits], fits.table, feat)
        logits = self._attached_head(hb, n_q, None, lp_iters)[0]
        return logits.reshape(G, K, n_q, self.n_classes, N)

    def predict(self, fitted, query_x, query_y=None, lp_iters=None):
        """Segment query clouds against a fitted support set: query_x (n_q, C, N) -> (logits (n_q, n_way + 1, N), loss), or
        (G, n_q, C, N) -> (logits (G, n_q, n_way + 1, N), loss (G,)); any n_q >= 1; loss is None without query_y.  Per group
        the bits of forward(..., eval=fitted.eval, lp_iters=lp_iters) on the episode [that support set | that group];
        lp_converged() then speaks for the G systems, as after forward_episodes.  ValueError, before any launch, for a shape
        that does not match the fit or a fit whose weights have changed since (fitted.py)."""
        from . import fitted as F
        _, _, grouped = F.check_predict_args(self, fitted, query_x, query_y)
        if fitted.head is None:
            raise ValueError("predict: the fit holds no MPTI head state (it was fitted by %s)" % fitted.model_class)
        qx = query_x if grouped else query_x[None]
        qy = query_y if (grouped or query_y is None) else query_y[None]
        logits, loss, _ = self._predict_groups(fitted, qx, qy, lp_iters)
        if not grouped:
            logits, loss = logits[0], loss[0]
        return logits, (loss if query_y is not None else None)

    def _forward_eval(self, support_x, support_y, query_x, query_y, eval, lp_iters):
        """support_x (E, n_way, k_shot, C, N), support_y (E, n_way, k_shot, N), query_x (E, n_q, C, N), query_y (E, n_q, N)."""
        E = support_x.shape[0]
        S = self.n_way * self.k_shot
        N = self.n_points
        n_q = query_x.shape[1]
        sx = support_x.reshape(E, S, self.in_channels, N)
        # eval-mode BatchNorm uses running statistics, so all clouds of all episodes share one pass; rows per episode:
        # its S support clouds, then its n_q query clouds
        feat = self.getFeatures_pm(ops.cat_clouds(sx, query_x, 1).reshape(E * (S + n_q), self.in_channels, N), group=S + n_q)
        ep_rows = (S + n_q) * N
        sfeat, qfeat = feat, feat[S * N:]
        shot_keep = None
        if eval:
            # clean-shot detection (mpti.py:87-223, 316-371, called at :440-442), eval only: 0 = the shot's foreground
            # points are ignored when the class prototypes are built (the reference's pl_support_y, which is
            # constant within a shot)
            shot_keep = ops.clean_shot_detect(sfeat, support_x, support_y, self.n_way, self.k_shot, N, E=E,
                                              feat_ep_rows=ep_rows)
        hb = self._head_buffers(n_q, feat.device, E)
        if lp_iters:  # the conservative re-run: one FPS launch per round as well
            hb.fps_one_launch = False
        sy = support_y.reshape(E, S, N).to(torch.int32).contiguous()
        ops.head_prototypes(hb, sy, shot_keep, sfeat, qfeat, ep_rows)
        if self._trace is not None:
            self._trace.update(sfeat=feat[:S * N], qfeat=feat[S * N:ep_rows], feat=feat, shot_keep=shot_keep)
        return self._attached_head(hb, n_q, query_y, lp_iters)[:2]
