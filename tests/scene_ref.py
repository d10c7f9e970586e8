"""Plain numpy float32 restatement of predict_scene's definition ("Labelling a scan"): steps 1-6 and 8.
Written from the definition, loops and all; the tests compare the device's plan, prepared clouds and votes with it bit
for bit.  Step 7 (the model) is not restated: vote() takes the chunk logits as an argument."""
import numpy as np

f32 = np.float32


class RefPlan:
    """Steps 1-5 for scan (M, >= 3) float32, N points per cloud."""

    def __init__(self, scan, N, block_size=1.0, stride=None, min_points=100):
        scan = np.asarray(scan, f32)
        self.scan, self.N, self.M = scan, N, scan.shape[0]
        # 1. valid points and origin
        self.valid = np.isfinite(scan[:, 0]) & np.isfinite(scan[:, 1]) & np.isfinite(scan[:, 2])
        if not self.valid.any():
            raise ValueError("no valid point")
        v = scan[self.valid]
        self.x0, self.y0, self.xmax, self.ymax = v[:, 0].min(), v[:, 1].min(), v[:, 0].max(), v[:, 1].max()
        # 2. cells
        s = f32(block_size if stride is None else stride)
        self.s = s
        ratio = float(block_size) / float(block_size if stride is None else stride)
        self.r = r = int(round(ratio))
        if r < 1 or r > 4 or abs(ratio - r) > 1e-6 * r:
            raise ValueError("block_size / stride")
        self.ncx = int(np.floor((self.xmax - self.x0) / s)) + 1
        self.ncy = int(np.floor((self.ymax - self.y0) / s)) + 1
        self.n_cells = self.ncx * self.ncy
        self.key = np.full(self.M, -1, np.int64)
        for p in np.nonzero(self.valid)[0]:
            cx = int(np.floor((scan[p, 0] - self.x0) / s))  # float32 - float32, / float32: IEEE, one rounding each
            cy = int(np.floor((scan[p, 1] - self.y0) / s))
            self.key[p] = cy * self.ncx + cx
        # 3. cell lists: ascending scan index inside a cell
        self.cells = [[] for _ in range(self.n_cells)]
        for p in range(self.M):
            if self.valid[p]:
                self.cells[self.key[p]].append(p)
        self.order = np.array([p for c in self.cells for p in c], np.int32)
        self.cell_start = np.concatenate([[0], np.cumsum([len(c) for c in self.cells])]).astype(np.int32)
        # 4. blocks
        self.nbx, self.nby = max(self.ncx - r + 1, 1), max(self.ncy - r + 1, 1)
        self.block_list = []
        for by in range(self.nby):
            for bx in range(self.nbx):
                lst = []
                for cy in range(by, min(by + r, self.ncy)):
                    for cx in range(bx, min(bx + r, self.ncx)):
                        lst += self.cells[cy * self.ncx + cx]
                self.block_list.append(lst)
        self.block_points = np.array([len(b) for b in self.block_list], np.int32)
        self.kept = self.block_points >= min_points
        self.n_blocks = int(self.kept.sum())
        # 5. chunks: (block, j), numbered by block id, then j; slot t holds member t mod len
        self.chunks, self.block_chunk0 = [], [0]
        slot_map = []
        for b, lst in enumerate(self.block_list):
            if self.kept[b]:
                n = len(lst)
                nc = -(-n // N)
                for j in range(nc):
                    members = lst[j::nc]
                    assert len(members) == -(-(n - j) // nc) <= N
                    self.chunks.append((b, j, len(members)))
                    slot_map.append([members[t % len(members)] for t in range(N)])
            self.block_chunk0.append(len(self.chunks))
        self.n_chunks = len(self.chunks)
        self.block_chunk0 = np.array(self.block_chunk0, np.int32)
        self.chunk_block = np.array([c[0] for c in self.chunks], np.int32)
        self.slot_map = np.array(slot_map, np.int32).reshape(self.n_chunks, N)

    # 6. prepared clouds (loader.py:105-119 in fp32): (n_chunks, C, N)
    def prepared(self, rgb=True, XYZ=True):
        out = []
        for sm in self.slot_map:
            pts = self.scan[sm]
            xyz = pts[:, 0:3] - pts[:, 0:3].min(0)
            ch = [xyz]
            if rgb:
                ch.append(pts[:, 3:6] / f32(255.0))
            if XYZ:
                ext = xyz.max(0)
                with np.errstate(invalid="ignore", divide="ignore"):
                    ch.append(np.where(ext > 0, xyz / ext, f32(0)).astype(f32))  # an axis of zero extent: 0
            out.append(np.concatenate(ch, 1).astype(f32).T)
        return np.stack(out) if out else np.zeros((0, 3 * (1 + rgb + XYZ), self.N), f32)

    # 8. votes: chunks ascend with the block id, so walking chunks then slots is "block id ascending, then slot ascending"
    def vote(self, logits):
        """logits (n_chunks, K, N) float32 -> (scores (M, K) f32, labels (M,) i64, votes (M,) i32)."""
        logits = np.asarray(logits, f32)
        K = logits.shape[1]
        scores, votes = np.zeros((self.M, K), f32), np.zeros(self.M, np.int32)
        for c in range(self.n_chunks):
            for t in range(self.N):
                p = self.slot_map[c, t]
                scores[p] = scores[p] + logits[c, :, t]  # fp32, one appearance at a time
                votes[p] += 1
        labels = np.where(votes > 0, scores.argmax(1), -1).astype(np.int64)  # numpy's argmax: the first maximum
        return scores, labels, votes
