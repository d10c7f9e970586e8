"""N2: the reference's `.h5` episode container (dataloaders/loader.py:1687-1721) through the HDF5 C library.

tests/golden/episode_ref.h5 was written by the reference's own `write_episode` under real h5py
(oracle/gen_golden_h5.py, run with the interpreter of the image that has h5py).  Read here: every dataset with the
reference's dtype and values.  Written here: read back; and compared with tests/golden/episode_h5lite.h5, a file
written here that the reference's `read_episode` under real h5py read back correctly.
"""
import hashlib
import os
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from r3dfsseg_amd import episode_io as EIO, h5lite  # noqa: E402

REF_FILE = os.path.join(ROOT, "tests", "golden", "episode_ref.h5")
H5LITE_FILE = os.path.join(ROOT, "tests", "golden", "episode_h5lite.h5")
REF_READ_DIGEST = "49e8dd1d1ce5f2b990def3d19dddd7d578318f6fe0e01f585caa11feff3c2136"

needs_hdf5 = pytest.mark.skipif(not h5lite.available(), reason="no HDF5 C library (>= 1.10) on this host")


def episode(seed=21, n_way=2, k_shot=3, N=96):  # as oracle/gen_golden_h5.py::episode
    rs = np.random.RandomState(seed)
    return (rs.uniform(0, 1, (n_way, k_shot, N, 9)), rs.randint(0, 2, (n_way, k_shot, N)),
            rs.uniform(0, 1, (n_way, N, 9)), rs.randint(0, n_way + 1, (n_way, N)), np.array([3, 8]),
            rs.randint(0, 5, (n_way, k_shot, N)), rs.randint(0, 5, (n_way, N)), rs.randint(0, 2, (n_way, k_shot, N)))


def digest(arrays):
    h = hashlib.sha256()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(("%s %s " % (a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


@needs_hdf5
def test_reads_the_file_the_reference_wrote():
    got = EIO.read_episode(REF_FILE)
    want = episode()
    assert len(got) == 8
    for (name, dt), g, w in zip(EIO.EPISODE_FIELDS, got, want):
        assert g.dtype == dt and g.shape == w.shape, (name, g.dtype, g.shape)
        assert np.array_equal(g, w.astype(dt)), name  # write_episode's dtype= conversion (float64 -> float32, int64 -> int32)
    # stored types, not only values: float32 clouds, int64 labels, int32 elsewhere (loader.py:1691-1701)
    raw = h5lite.read_datasets(REF_FILE, [n for n, _ in EIO.EPISODE_FIELDS])
    assert [a.dtype for a in raw] == [np.dtype(dt) for _, dt in EIO.EPISODE_FIELDS]
    # and the collate on top of it: (n_way, k, N, 9) -> (n_way, k, 9, N)
    out, classes = EIO.collate_test(got)
    assert tuple(out[0].shape) == (2, 3, 9, 96) and list(classes) == [3, 8]
    assert np.array_equal(out[0].numpy(), np.swapaxes(got[0], 2, 3))


@needs_hdf5
def test_write_read_round_trip_and_errors(tmp_path):
    ep = episode(seed=5, n_way=3, k_shot=1, N=40)
    fn = str(tmp_path / "7.h5")
    EIO.write_episode(fn, ep)
    back = EIO.read_episode(fn)
    for (name, dt), b, w in zip(EIO.EPISODE_FIELDS, back, ep):
        assert b.dtype == dt and np.array_equal(b, np.asarray(w, dtype=dt)), name
    # the feeder lists and reads .h5 caches in index order (loader.py:1623-1636)
    EIO.write_episode(str(tmp_path / "10.h5"), ep)
    files = EIO.list_episode_files(str(tmp_path))
    assert [os.path.basename(f) for f in files] == ["7.h5", "10.h5"]
    assert len(list(EIO.EpisodeFeeder(files, device="cpu"))) == 2
    # a file without the contract's datasets, and something that is not HDF5 at all
    h5lite.write_datasets(str(tmp_path / "bad.h5"), [("support_ptclouds", np.zeros((1, 1, 4, 9), np.float32))])
    with pytest.raises(ValueError, match="support_masks"):
        EIO.read_episode(str(tmp_path / "bad.h5"))
    (tmp_path / "junk.h5").write_bytes(b"not an hdf5 file")
    with pytest.raises(h5lite.H5Error):
        EIO.read_episode(str(tmp_path / "junk.h5"))
    # empty and scalar-free edge: a zero-length dataset keeps its shape and type
    h5lite.write_datasets(str(tmp_path / "empty.h5"), [("a", np.zeros((0, 9), np.float32)), ("b", np.arange(6, dtype=np.int64).reshape(2, 3))])
    a, b = h5lite.read_datasets(str(tmp_path / "empty.h5"), ["a", "b"])
    assert a.shape == (0, 9) and a.dtype == np.float32 and np.array_equal(b, np.arange(6).reshape(2, 3)) and b.dtype == np.int64


@needs_hdf5
def test_the_reference_reads_what_this_writes(tmp_path):
    """tests/golden/episode_h5lite.h5 is the seed-9 episode as written here; the reference's `read_episode` under real
    h5py read it back as REF_READ_DIGEST (oracle/gen_golden_h5.py --h5lite, then --check).  A fresh write must be that
    file byte for byte, but for the modification time HDF5 stamps into each dataset's object header."""
    ep = episode(seed=9)
    assert digest([np.asarray(a, dtype=dt) for a, (_, dt) in zip(ep, EIO.EPISODE_FIELDS)]) == REF_READ_DIGEST
    fn = str(tmp_path / "0.h5")
    t0 = int(time.time())
    EIO.write_episode(fn, ep)
    t1 = int(time.time())
    got = np.fromfile(fn, np.uint8)
    want = np.fromfile(H5LITE_FILE, np.uint8)
    assert got.shape == want.shape
    stamps = [j for j in range(got.size - 3) if t0 <= int(got[j:j + 4].view("<u4")[0]) <= t1]
    assert len(stamps) == len(EIO.EPISODE_FIELDS)  # one per dataset
    assert len({int(want[j:j + 4].view("<u4")[0]) for j in stamps}) == 1  # the golden's own write time, in the same places
    for j in stamps:
        got[j:j + 4] = want[j:j + 4] = 0
    assert np.array_equal(got, want)
