"""Plain numpy restatement of fit_scene's definition ("Fitting from an annotated scan"): S2-S5 on top of
scene_ref.RefPlan (S1).  Written from the definition, loops and all; the tests compare the device's counts, choice of shots,
clouds and masks with it bit for bit.  fit_support itself is not restated."""
import numpy as np

f32 = np.float32


class RefSupport:
    """S2-S4 for a RefPlan, labels (M,) of any integer dtype and `classes`, n_way distinct ints.  fg (blocks, n_way) int32,
    length (blocks,): len of a kept block's cloud, 0 for a dropped block; thr (blocks,); eligible[w]: block ids in the order
    of the choice; n_eligible.  pick() is S4's choice, shots() S5."""

    def __init__(self, plan, labels, classes, k_shot, min_ratio=0.05, min_fg=100):
        labels = np.asarray(labels)
        assert labels.shape == (plan.M,) and labels.dtype.kind == "i"
        self.plan, self.labels, self.classes, self.k_shot = plan, labels, [int(c) for c in classes], int(k_shot)
        nb, n_way = len(plan.block_list), len(self.classes)
        self.fg = np.zeros((nb, n_way), np.int32)
        self.length, self.thr = np.zeros(nb, np.int64), np.zeros(nb, np.int64)
        self.members = {}
        for b, lst in enumerate(plan.block_list):
            if not plan.kept[b]:
                continue
            # S2: the cloud is chunk 0 of the block, as step 5 cut it
            c = int(plan.block_chunk0[b])
            assert plan.chunks[c][0] == b and plan.chunks[c][1] == 0
            n = len(lst)
            nc = -(-n // plan.N)
            members = lst[0::nc]
            assert len(members) == plan.chunks[c][2] == -(-n // nc) <= plan.N
            self.members[b], self.length[b] = members, len(members)
            # S3: every member once
            for w, cls in enumerate(self.classes):
                self.fg[b, w] = sum(1 for p in members if int(labels[p]) == cls)
            # S4: fp32, one multiplication
            self.thr[b] = max(int(np.floor(f32(len(members)) * f32(min_ratio))), int(min_fg))
        self.eligible = []
        for w in range(n_way):
            el = [b for b in range(nb) if plan.kept[b] and self.fg[b, w] > self.thr[b]]
            self.eligible.append(sorted(el, key=lambda b: (-int(self.fg[b, w]), b)))
        self.n_eligible = [len(e) for e in self.eligible]

    def pick(self):
        """-> (shot_block, shot_fg), both (n_way, k_shot) int32; ValueError for a way with fewer than k_shot eligible blocks."""
        for w, el in enumerate(self.eligible):
            if len(el) < self.k_shot:
                raise ValueError("way %d (class id %d) has %d eligible blocks, k_shot = %d"
                                 % (w + 1, self.classes[w], len(el), self.k_shot))
        blocks = np.array([el[:self.k_shot] for el in self.eligible], np.int32)
        fgs = np.array([[self.fg[b, w] for b in row] for w, row in enumerate(blocks)], np.int32)
        return blocks, fgs

    def shots(self, rgb=True, XYZ=True):
        """S5 -> (support_x (n_way, k_shot, C, N) f32, support_y (n_way, k_shot, N) int32, slot_map (n_way, k_shot, N) int32):
        the clouds are rows of RefPlan.prepared(), the slots rows of RefPlan.slot_map."""
        blocks, _ = self.pick()
        plan = self.plan
        chunk = plan.block_chunk0[blocks]                    # chunk 0 of every chosen block
        prepared = plan.prepared(rgb=rgb, XYZ=XYZ)
        slot_map = plan.slot_map[chunk]
        x = prepared[chunk]
        y = np.zeros(slot_map.shape, np.int32)
        for w, cls in enumerate(self.classes):
            for i in range(self.k_shot):
                for t in range(plan.N):
                    y[w, i, t] = int(self.labels[slot_map[w, i, t]]) == cls
        return x.astype(f32), y, slot_map.astype(np.int32)
