"""ctypes binding of libr3d_hip.so (the C ABI declared in include/r3d.h).

This is the stub a maintainer of the reference would add next to models/ to call the
MI355X kernels.  There is NO fallback: if the shared library is missing or a symbol is
absent, importing an op raises -- the product path never computes on the CPU.
"""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("R3D_LIB") or os.path.join(_HERE, "libr3d_hip.so")  # R3D_LIB: probe builds (tools/probe)
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "r3d.h")

c_f = ctypes.c_void_p      # device pointers travel as void*
c_i = ctypes.c_int
c_l = ctypes.c_long
c_fl = ctypes.c_float
c_d = ctypes.c_double
c_u = ctypes.c_uint

_SCALARS = {"unsigned": c_u, "double": c_d, "float": c_fl, "long": c_l, "int": c_i, "int32_t": c_i}


def _ctype(decl, what):
    """ctypes class of `decl`, a C declaration of a type followed by a name: any pointer travels as void*, a scalar by value
    as its C type.  Anything else raises instead of guessing (int64_t by value among them: none exists, and as c_int it
    would lose its upper half)."""
    words = [w for w in decl.replace("*", " * ").split() if w != "const"]
    if "*" in words:
        return c_f
    if len(words) == 2 and words[0] in _SCALARS:
        return _SCALARS[words[0]]
    raise RuntimeError("r3dfsseg_amd: cannot bind %s: unrecognised declaration %r" % (what, " ".join(decl.split())))


def parse_header(txt):
    """(names, signatures) of the `r3d_*` functions a C header declares: the sorted names, and name -> (restype, [argtypes])
    for ctypes.  One pass over the text without its comments serves both.  Every name needs a prototype
    `type r3d_name(parameters);` whose types _ctype knows; else this raises and names the function."""
    txt = re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", txt, flags=re.S))
    names = sorted(set(re.findall(r"\b(r3d_[a-z0-9_]+)\s*\(", txt)))
    sigs = {}
    for ret, name, params in re.findall(r"([A-Za-z_][A-Za-z0-9_ \*]*?)\b(r3d_[a-z0-9_]+)\s*\(([^;{()]*)\)\s*;", txt):
        if name in sigs:
            raise RuntimeError("r3dfsseg_amd: %s is declared twice" % name)
        params = [p.strip() for p in params.split(",")]
        if params in (["void"], [""]):
            params = []
        if ret.replace("*", " * ").split() == ["const", "char", "*"]:
            res = ctypes.c_char_p
        elif "*" in ret:
            raise RuntimeError("r3dfsseg_amd: cannot bind %s: unrecognised return type %r" % (name, ret.strip()))
        else:
            res = _ctype(ret + " " + name, "the return type of " + name)
        sigs[name] = (res, [_ctype(p_, "parameter %d of %s" % (i, name)) for i, p_ in enumerate(params)])
    if sorted(sigs) != names:
        raise RuntimeError("r3dfsseg_amd: no prototype parsed for %s" % ", ".join(sorted(set(names) - set(sigs))))
    return names, sigs


_TOKEN = re.compile(r"\s*(?:(0[xX][0-9a-fA-F]+|[0-9]+)[lL]?(?![0-9A-Za-z_.])|([A-Za-z_][A-Za-z0-9_]*)|(<<|[-+*|()]))")
_BINARY = (("|",), ("<<",), ("+", "-"), ("*",))  # loosest first, as C ranks them


def _const_value(expr, known, name):
    """Value of `expr`, the right-hand side of `#define name`: integer literals (decimal, hex, an L suffix), constants
    already in `known`, + - * << |, unary + and -, parentheses.  Anything else raises and names the constant."""
    def bad(why):
        return RuntimeError("r3dfsseg_amd: cannot evaluate %s: %s in %r" % (name, why, expr))

    toks, at = [], 0
    while expr[at:].strip():
        m = _TOKEN.match(expr, at)
        if not m:
            raise bad("unrecognised text")
        toks.append(m.group(1, 2, 3))
        at = m.end()
    toks.reverse()  # a stack: the next token is toks[-1]

    def atom():
        if not toks:
            raise bad("an operand is missing")
        num, ident, op = toks.pop()
        if num is not None:
            return int(num, 0)
        if ident is not None:
            if ident not in known:
                raise bad("%s is not defined above it" % ident)
            return known[ident]
        if op in "+-":
            return atom() if op == "+" else -atom()
        if op == "(":
            v = binary(0)
            if not toks or toks.pop()[2] != ")":
                raise bad("an unclosed parenthesis")
            return v
        raise bad("a misplaced %r" % op)

    def binary(level):
        if level == len(_BINARY):
            return atom()
        v = binary(level + 1)
        while toks and toks[-1][2] in _BINARY[level]:
            op, w = toks.pop()[2], binary(level + 1)
            v = v | w if op == "|" else v << w if op == "<<" else v + w if op == "+" else v - w if op == "-" else v * w
        return v

    v = binary(0)
    if toks:
        raise bad("text behind the expression")
    return v


def parse_constants(txt):
    """{name: int} of the `#define R3D_<NAME> <value>` lines of a C header, comments removed, in the order of the text.  A
    define without a value (the include guard) is skipped.  A value is what _const_value takes; a float, a function-like
    macro, a name used before its definition or a second definition of a name raises and names the constant."""
    txt = re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", txt, flags=re.S))
    consts = {}
    for name, params, expr in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(R3D_[A-Za-z0-9_]*)(\()?([^\n]*)$", txt, flags=re.M):
        if params:
            raise RuntimeError("r3dfsseg_amd: cannot evaluate %s: a function-like macro" % name)
        if not expr.strip():
            continue
        if name in consts:
            raise RuntimeError("r3dfsseg_amd: %s is defined twice" % name)
        consts[name] = _const_value(expr, consts, name)
    return consts


# the binding IS the header: read once, at import
_HEADER = open(HEADER_PATH).read()
_SYMBOLS, _SIGS = parse_header(_HEADER)
CONSTANTS = parse_constants(_HEADER)  # every number of the contract: ops exports them without the prefix


def header_symbols():
    """Function names declared in include/r3d.h."""
    return list(_SYMBOLS)


_lib = None


ABI_VERSION = CONSTANTS["R3D_ABI_VERSION"]


def load():
    """Load the shared library and bind every declared symbol; raises if anything is missing."""
    global _lib
    if _lib is not None:
        return _lib
    # torch first: its bundled HIP runtime must be the one already mapped when our library's
    # libamdhip64 dependency is resolved (two runtimes in one process see no device)
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "r3dfsseg_amd: %s not found -- build it with `python -m r3dfsseg_amd.build` "
            "(hipcc, gfx950). There is no CPU fallback." % LIB_PATH)
    cdll = ctypes.CDLL(LIB_PATH)
    lib = _Bound()
    lib._cdll = cdll
    for name, (res, args) in _SIGS.items():
        try:
            fn = getattr(cdll, name)
        except AttributeError:
            raise RuntimeError("r3dfsseg_amd: symbol %s missing from %s" % (name, LIB_PATH))
        fn.restype = res
        fn.argtypes = args
        setattr(lib, name, fn)
    if lib.r3d_abi_version() != ABI_VERSION:  # a stale build would be CALLED with this round's argument lists
        raise RuntimeError("r3dfsseg_amd: %s has C ABI version %d, this package binds version %d -- rebuild it "
                           "(`python -m r3dfsseg_amd.build --force`)" % (LIB_PATH, lib.r3d_abi_version(), ABI_VERSION))
    _lib = lib
    mode = os.environ.get("R3D_MATRIX_ARITH")  # "fp32" | "bf16x3": see r3d_set_matrix_arith in include/r3d.h
    if mode is not None:
        if mode not in ("fp32", "bf16x3"):
            raise RuntimeError("R3D_MATRIX_ARITH=%r: expected fp32 or bf16x3" % mode)
        check(lib.r3d_set_matrix_arith(1 if mode == "bf16x3" else 0))
    mask = os.environ.get("R3D_GEMM_BX3")  # tuning knob: r3d_debug_set_gemm_bx3 in include/r3d.h
    if mask is not None:
        check(lib.r3d_debug_set_gemm_bx3(int(mask)))
    return lib


class _Bound:
    """The bound entry points as plain attributes (one per symbol of include/r3d.h)."""


_call_log = None  # list collecting (fn, args) of the library calls of one timed region (bench.py's roofline leg)


def record_calls(on):
    """Route every entry point through a recorder (on=True) or back to the raw ctypes functions (on=False).
    While on, calls made with `_call_log` set to a list are appended to it, so that a timed region can be
    launched again back to back (ops.KernelTimer with repeat > 0)."""
    lib = load()
    for name in _SIGS:
        raw = getattr(lib._cdll, name)
        if not on:
            setattr(lib, name, raw)
            continue

        def wrapper(*args, _raw=raw):
            rc = _raw(*args)
            if _call_log is not None:
                _call_log.append((_raw, args))
            return rc
        setattr(lib, name, wrapper)


def check(rc):
    if rc != 0:
        raise RuntimeError("r3d: " + load().r3d_last_error_string().decode())
