"""CPU-side checks of the batched ProtoNet entry points: declared in include/r3d.h, bound in _lib._SIGS with matching argument
counts, exported by the cross-compiled library -- and the C ABI version is still 5 (the entry points are additive)."""
import ctypes
import os
import re

from r3dfsseg_amd import _lib

NEW = {"r3d_protonet_head_ws_words": 3, "r3d_protonet_head_batched": 18, "r3d_count_correct_batched": 6}


def _header_prototypes():
    txt = open(_lib.HEADER_PATH).read()
    txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
    txt = re.sub(r"//[^\n]*", " ", txt)
    return {name: [a for a in (x.strip() for x in args.split(",")) if a and a != "void"]
            for name, args in re.findall(r"\b(r3d_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", txt, flags=re.S)}


def test_header_and_binding_declare_the_batched_protonet_head():
    protos = _header_prototypes()
    for name, n_args in NEW.items():
        assert name in protos, name
        assert name in _lib._SIGS, name
        assert len(protos[name]) == len(_lib._SIGS[name][1]) == n_args, (name, protos[name], _lib._SIGS[name][1])
    assert _lib._SIGS["r3d_protonet_head_ws_words"][0] is _lib.c_l
    assert _lib._SIGS["r3d_protonet_head_batched"][0] is _lib.c_i
    assert _lib.ABI_VERSION == 6


def test_library_exports_the_batched_protonet_head_under_abi_5():
    from r3dfsseg_amd import build
    path = build.build()
    assert os.path.exists(path)
    lib = ctypes.CDLL(path)
    for name in NEW:
        assert hasattr(lib, name), name
    lib.r3d_abi_version.restype = ctypes.c_int
    assert lib.r3d_abi_version() == 6
    # the scratch size is host arithmetic: S * 2 * 256 floats per episode, negative for a shape the kernels do not carry
    f = lib.r3d_protonet_head_ws_words
    f.restype, f.argtypes = ctypes.c_long, [ctypes.c_int] * 3
    assert f(1, 2, 5) == 10 * 2 * 256 and f(32, 2, 5) == 32 * 10 * 2 * 256
    assert f(0, 2, 5) < 0 and f(65536, 2, 5) < 0 and f(1, 8, 1) < 0 and f(1, 0, 1) < 0 and f(1, 2, 0) < 0


def test_batched_head_refuses_bad_arguments_on_the_host():
    """Refusals come before any launch, so they can be seen without a GPU (error convention of include/r3d.h)."""
    lib = _lib.load()
    p = ctypes.c_void_p(256)  # never dereferenced: every call below is refused on the host
    D, N, n_pts = 192, 64, 128
    ok = dict(n_ep=1, sfeat=p, ldf=D, qfeat=p, ldq=D, rows=0, D=D, sy=p, n_way=2, k_shot=1, N=N, n_pts=n_pts, method=0,
              Z=p, ws=p, words=2 * 2 * 256)

    def call(**over):
        a = dict(ok, **over)
        return lib.r3d_protonet_head_batched(a["n_ep"], a["sfeat"], a["ldf"], a["qfeat"], a["ldq"], a["rows"], a["D"], a["sy"],
                                             a["n_way"], a["k_shot"], a["N"], a["n_pts"], a["method"], 10.0, a["Z"], a["ws"],
                                             a["words"], None)
    for over, text in ((dict(sfeat=None), b"null pointer"), (dict(Z=None), b"null pointer"), (dict(ws=None), b"null pointer"),
                       (dict(n_way=8), b"unsupported shape"), (dict(n_way=0), b"unsupported shape"),
                       (dict(D=257), b"unsupported shape"), (dict(D=0), b"unsupported shape"),
                       (dict(method=2), b"Distance computation method (2) is unknown"),
                       (dict(n_ep=0), b"episodes"), (dict(n_ep=65536, words=1 << 40), b"episodes"),
                       (dict(n_ep=2, rows=2 * N - 1, words=2 * 2 * 2 * 256), b"rows between them"),
                       (dict(words=2 * 2 * 256 - 1), b"workspace"), (dict(ws=ctypes.c_void_p(260)), b"16-byte aligned")):
        assert call(**over) != 0, over
        assert text in lib.r3d_last_error_string(), (over, lib.r3d_last_error_string())
