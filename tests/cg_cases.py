"""The systems of tests/test_gpu_cg_coarse.py: the smallest at which each path of the coarse-space kernels is taken.
tests/test_cg_ref_host.py asserts, without a GPU, the property each case was chosen for (``prop``) and the preconditions
the GPU tests rest on; the GPU tests build the same cases and compare with tests/cg_ref.py.

A case is features x (n, D) fp32, a right-hand side Y (n, 4) (one-hot labels on the first rows, column 3 ALL ZERO in
every case), neighbour lists nbr (n, K + 1) int64 and the descriptor's n_proto.  The lists are index decisions and are not
under test here (tests/test_gpu_knn_paths.py): they are made on the host -- the exact K nearest rows in float64, or lists
written for chosen row lengths -- and injected, the way tests/test_gpu_cg_spmv_stream.py does."""
from types import SimpleNamespace

import numpy as np
import torch

import cg_ref as C

K = 8              # neighbours per node (kp1 = 9)
SIGMA, ALPHA = 1.0, 0.99
CAP_EXTRA = 40     # n_cap = n + CAP_EXTRA: rows n .. n_cap exist and must stay out of every result
N_LABELLED = 20    # rows that carry a label when there are fewer prototypes than that


def features(n, D, seed, sep=0.0, intrinsic=0, scale=0.06):
    """Three gaussian clusters (tests/head_ref.py::graph_nodes without its duplicates), pushed `sep` standard deviations
    apart along three axes when sep > 0 (test_gpu_head.py::test_label_propagation_on_clustered_features).  intrinsic > 0:
    the spread inside a cluster lives in the first `intrinsic` channels (5 % of it in the others), so that a graph of K = 8
    neighbours has the smooth within-cluster modes the 200-neighbour graphs of the trained encoder have."""
    rs = np.random.RandomState(seed)
    centers = rs.randn(3, D).astype(np.float32) * scale * 2
    lab = rs.randint(0, 3, n)
    noise = rs.randn(n, D).astype(np.float32) * scale
    if intrinsic:
        noise[:, intrinsic:] *= np.float32(0.05)
    x = centers[lab] + noise
    if sep:
        x = x + np.eye(3, D, dtype=np.float32)[lab] * np.float32(sep * scale)
    return torch.from_numpy(x.astype(np.float32)), torch.from_numpy(lab.astype(np.int64))


def knn_lists(x, k=K):
    """(n, k + 1) int64: the node itself, then its k nearest other rows in float64 (stable order among equals)."""
    xd = x.double()
    d = torch.cdist(xd, xd)
    d[torch.arange(len(x)), torch.arange(len(x))] = -1.0
    return torch.argsort(d, dim=1, stable=True)[:, :k + 1].contiguous()


def chunk_lists(n):
    """Lists written for ROW LENGTHS of the symmetrised graph (r3d_cg_mw_kernel walks a row in chunks of 256 entries): one
    hub everybody lists (n - 1 entries: three chunks at n > 513), node A listed by 255 plain nodes (256 entries with the
    hub: exactly one chunk), node B by 256 (257 entries: one entry in the second chunk), a plain node lists the hub, its
    three successors on a ring of the plain nodes and, the first 255 / 256 of them, A / B: 9 entries at the most.  Unused
    slots hold the node itself (the diagonal is dropped).  -> (nbr, rowlen (n,), hub, A, B)"""
    hub, A, B = 7, 129, n - 3
    plain = [i for i in range(n) if i not in (hub, A, B)]
    P = len(plain)
    assert P >= 256 + 3
    nbr = np.empty((n, K + 1), dtype=np.int64)
    nbr[:, :] = np.arange(n)[:, None]
    nbr[A, 1] = hub
    nbr[B, 1] = hub
    for p, i in enumerate(plain):
        nbr[i, 1:6] = [hub, plain[(p + 1) % P], plain[(p + 2) % P], plain[(p + 3) % P], A if p < 255 else i]
        nbr[i, 6] = B if p < 256 else i
    nbr = torch.from_numpy(nbr)
    rowlen = C.pattern(nbr).sum(1).numpy()
    return nbr, rowlen, hub, A, B


def _case(name, n, n_proto, D, seed, prop, sep=0.0, intrinsic=0, lists="knn", dup=()):
    x, lab = features(n, D, seed, sep, intrinsic)
    src = C.seeds(n_proto, n)
    for lo, hi in dup:  # seed `hi` gets the row of seed `lo`
        x[src[hi]] = x[src[lo]]
    n_lab = min(n, max(n_proto, N_LABELLED))
    Y = torch.zeros(n, 4)
    Y[torch.arange(n_lab), lab[:n_lab]] = 1
    c = SimpleNamespace(name=name, n=n, n_proto=n_proto, D=D, k=K, sigma=SIGMA, alpha=ALPHA, x=x, Y=Y, prop=prop, dup=tuple(dup),
                        n_cap=n + CAP_EXTRA, lists=lists)
    if lists == "chunks":
        c.nbr, c.rowlen, c.hub, c.A, c.B = chunk_lists(n)
    else:
        c.nbr = knn_lists(x)
    return c


# (name, n, n_proto, D, seed, property, ...).  The random seeds were searched ON THE HOST, in float64, for the preconditions
# tests/test_cg_ref_host.py asserts for every case -- never by anything the device gave:
#   * no node's aggregate decision lies within 1e-4 (relative) of a tie;
#   * the solve needs at least 8 iterations at tol 1e-6 (the early-iterate tests stop at 6);
#   * the fp32 restatement's own error of r_1, r_2, r_3, r_6 stays below CEIL / 4 = 2.5e-4 (31 and 33 nodes around 12
#     prototypes are solved to 1e-4 |b| in six steps, and fp32 then holds r_6 to 1e-3 only: they take 4 and 5 prototypes);
#   * the two-level solve needs no more iterations than plain CG, in float64 and in fp32;
#   * at tol 1e-6 AND 1e-7 the float64 residual passes the test by a factor 2 and missed it by a factor 2 one iteration
#     earlier, and the fp32 restatement's count does not move when every entry of S is perturbed by about one ulp
#     (cg_ref.perturbed_counts) -- COUNT_WINDOW below: the count is then not decided by rounding.
_SPECS = (
    ("proto1", 150, 1, 64, 561, "few"), ("proto2", 151, 2, 64, 342, "few"), ("proto20", 149, 20, 64, 123, "few"),
    ("proto63", 153, 63, 64, 84, "few"),
    ("proto64", 300, 64, 64, 65, "edge"), ("proto65", 301, 65, 64, 186, "edge"), ("proto90", 299, 90, 64, 287, "edge"),
    ("dup70", 303, 70, 64, 868, "dup", dict(dup=((10, 11), (40, 50)))),
    ("d4", 201, 66, 4, 89, "width"), ("d64", 202, 66, 64, 110, "width"), ("d132", 203, 66, 132, 31, "width"),
    ("d252", 199, 66, 252, 1132, "width"), ("d256", 205, 66, 256, 553, "width"),
    ("chunks", 601, 70, 64, 54, "chunks", dict(lists="chunks")),
    ("n31", 31, 4, 64, 35, "rows"), ("n33", 33, 5, 64, 35, "rows"), ("n255", 255, 64, 64, 137, "rows"),
    ("n257", 257, 64, 64, 378, "rows"), ("n513", 513, 80, 64, 159, "rows"),
    ("trained", 603, 90, 64, 1420, "trained", dict(sep=6.0, intrinsic=2)),
)
NAMES = tuple(s[0] for s in _SPECS)
TOLS = (1e-6, 1e-7)
# (case, tol) pairs whose iteration count is held to the window of the two host runs: all but four.  tests/test_cg_ref_host.py
# asserts the float64 side of each reason, and of the pairs IN the window that eight perturbed fp32 runs leave it alone:
#   * "chunks", both tolerances: its ring-and-hub graph converges by a factor ~3 per iteration, so NO iteration passes the
#     test by 2 after missing it by 2;
#   * "proto1" and "proto2" at 1e-7: with one or two aggregates the coarse space is little more than D^1/2 1, x_0 is large
#     (max |x| ~ 15 for max |b| = 1) and the fp32 residual is not monotone near 1e-7 |b| (it passes 0.45, 3.4, 3.9, 2.9, 0.18
#     times the threshold in the fp32 restatement): one-ulp perturbations of S move the restatement's own fp32 count
#     between 17 and 21 (16 and 20), whatever the random seed -- no fp32 solver has "a" count there.
# "chunks" is still held to `converged` and to plain CG's count; the two UNSTABLE pairs to `converged` and to float64's
# count - 1 .. + UNSTABLE_SPREAD + 1: the fp32 restatement, perturbed, stops either with float64 or 4 iterations later in
# both cases (profiles/r33_cg_coarse.md: 17 or 21, 16 or 20) -- and not to plain float64 CG's 17, which lies INSIDE that
# spread.  Which of the two a host's own fp32 run gives depends on its BLAS, so no host test asserts it.
UNSTABLE = (("proto1", 1e-7), ("proto2", 1e-7))
UNSTABLE_SPREAD = 4
NO_WINDOW = (("chunks", 1e-6), ("chunks", 1e-7)) + UNSTABLE
COUNT_WINDOW = tuple((name, tol) for name in NAMES for tol in TOLS if (name, tol) not in NO_WINDOW)
_cache = {}


def get(name):
    if name not in _cache:
        s = next(s for s in _SPECS if s[0] == name)
        _cache[name] = _case(*s[:6], **(s[6] if len(s) > 6 else {}))
    return _cache[name]


# the batch of test f: two systems of different n and n_proto in ONE capacity (that of the larger + CAP_EXTRA)
BATCH = ("proto20", "n257")
