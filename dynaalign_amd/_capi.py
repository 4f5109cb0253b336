"""ctypes binding of libdynaalign_hip.so -- the C ABI declared in include/dynaalign.h.

This module is the Python-side equivalent of the Rcpp glue in r_glue/: it only
marshals arguments.  All compute happens in the HIP library; if the library (or
a GPU) is missing, calls fail loudly -- there is no CPU fallback.
"""
import ctypes as C
import os
import re

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "lib", "libdynaalign_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_PKG), "include", "dynaalign.h")

DA_OK = 0
DA_ERR_EMPTY_INPUT, DA_ERR_BAD_K, DA_ERR_BAD_NHASH, DA_ERR_BAD_MATRIX = 1, 2, 3, 4
DA_ERR_BAD_RESIDUE_SEQ1, DA_ERR_BAD_RESIDUE_SEQ2, DA_ERR_NOMEM, DA_ERR_NO_DEVICE = 5, 6, 7, 8
DA_ERR_HIP, DA_ERR_UNSUPPORTED, DA_ERR_BAD_ARG = 9, 10, 11
DA_OUT_F64, DA_OUT_COMPACT, DA_OUT_PACK32 = 0, 1, 2
DA_KNN_UNION, DA_KNN_MUTUAL = 0, 1   # da_dev_knn_edges: which pairs of the nearest-neighbour lists become edges
DA_TOPK_MAX = 1024   # da_dev_topk_rows: the candidates of a row are sorted in a fixed LDS buffer

_SCALARS = {"int": C.c_int, "int32_t": C.c_int, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "size_t": C.c_size_t, "double": C.c_double}


def _ctype(text, name, ret=False):
    """the ctypes type of one parameter (its name, if any, still attached) or return type as the header spells it"""
    words = [w for w in text.replace("*", " * ").split() if w not in ("const", "struct", "extern", "DA_API")]
    if "*" in words:
        return C.c_char_p if words[:2] == ["char", "*"] and words.count("*") == 1 else C.c_void_p
    if not ret and len(words) > 1 and re.fullmatch(r"[A-Za-z_]\w*", words[-1]):
        words = words[:-1]
    if ret and words == ["void"]:
        return None
    if len(words) != 1 or words[0] not in _SCALARS:
        raise ValueError("%s: no ctypes type for %r in include/dynaalign.h" % (name, " ".join(text.split())))
    return _SCALARS[words[0]]


def header_prototypes(path=HEADER_PATH, text=None):
    """name -> (restype, argtypes) of every ``ret da_name(args);`` include/dynaalign.h declares (``text``: header text in place of the
    file).  A pointer is a void *, except char *; the scalars are those of _SCALARS.  Anything else -- another scalar type, a
    function-pointer or array parameter, a da_ name that is followed by a parenthesis but is no declaration this reader understands --
    raises with the function's name: there is no default type."""
    txt = open(path).read() if text is None else text
    txt = re.sub(r"/\*.*?\*/|//[^\n]*", " ", txt, flags=re.S)
    txt = re.sub(r"^[ \t]*#.*$", " ", txt, flags=re.M)
    out = {}
    for ret, name, args in re.findall(r"([A-Za-z_][\w\s*]*?)\b(da_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", txt):
        args = [] if args.strip() in ("", "void") else args.split(",")
        out[name] = (_ctype(ret, name, ret=True), [_ctype(a, name) for a in args])
    for m in re.finditer(r"\b(da_[a-z0-9_]+)\s*\(", txt):
        if m.group(1) not in out:
            raise ValueError("%s: no declaration this reader understands at %r" % (m.group(1), " ".join(txt[m.start():m.start() + 120].split())))
    return out


# name -> (restype, argtypes) of every function include/dynaalign.h declares, read from the header itself when this module is imported:
# a new entry point needs its declaration there and nothing here.  load() applies whatever this dict holds when it runs.
SIGNATURES = header_prototypes()

DA_EXCHANGE = {"rows": 0, "allgather": 1, "peercopy": 2}
DA_PHASES = ("setup", "compute", "exchange", "finalize", "d2h", "total")


class DaUniquePlan(C.Structure):
    """struct da_unique_plan (include/dynaalign.h): device pointers into the plan's workspace"""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_int32), ("n", C.c_int64), ("unique", C.c_int64),
                ("d_uidx", C.c_void_p), ("d_ufirst", C.c_void_p), ("d_ulast", C.c_void_p), ("d_ubytes", C.c_void_p),
                ("d_uoffsets", C.c_void_p), ("d_minfirst", C.c_void_p), ("d_maxlast", C.c_void_p)]


class DaSimilarityStats(C.Structure):
    """struct da_similarity_stats (include/dynaalign.h)"""
    _fields_ = [("mean_similarity", C.c_double), ("median_similarity", C.c_double), ("min_similarity", C.c_double),
                ("max_similarity", C.c_double), ("pairs", C.c_int64), ("most_similar_pair", C.c_int64 * 2),
                ("least_similar_pair", C.c_int64 * 2), ("most_similar_upper", C.c_int64 * 2), ("least_similar_upper", C.c_int64 * 2)]


ROW_EXTREMA_WORDS = 5   # struct da_row_extrema: {min_key, min_col, max_key, max_col, diag_key}, 32 bits each


class DaOpts(C.Structure):
    """struct da_opts (include/dynaalign.h)"""
    _fields_ = [("struct_size", C.c_uint32), ("n_devices", C.c_int32), ("devices", C.POINTER(C.c_int32)),
                ("exchange", C.c_int32), ("reserved", C.c_uint32), ("phase_ms", C.POINTER(C.c_double))]


def make_opts(devices=None, exchange="rows"):
    """-> (DaOpts, keepalive): the struct for da_similarity_*_opts; keepalive[1] receives the phase times (ms)"""
    devs = [] if devices is None else [int(d) for d in devices]
    if exchange not in DA_EXCHANGE:
        raise ValueError("exchange must be one of %s" % sorted(DA_EXCHANGE))
    dev_arr = (C.c_int32 * max(len(devs), 1))(*devs)
    phases = (C.c_double * len(DA_PHASES))()
    o = DaOpts(C.sizeof(DaOpts), len(devs), C.cast(dev_arr, C.POINTER(C.c_int32)), DA_EXCHANGE[exchange], 0,
               C.cast(phases, C.POINTER(C.c_double)))
    return o, (dev_arr, phases)


_lib = None


class DynaAlignError(RuntimeError):
    """Raised for any non-zero status; .code is the da_status, str() the library's message
    (for the reference's own error conditions: the reference's message text)."""

    def __init__(self, code, message):
        super().__init__(message)
        self.code = code


def header_symbols(path=HEADER_PATH):
    """Function names declared in include/dynaalign.h."""
    txt = open(path).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(da_[a-z0-9_]+)\s*\(", txt)))


def load(path=None):
    """dlopen the HIP library (once) and set prototypes.  Raises if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    path = path or os.environ.get("DYNAALIGN_LIB", LIB_PATH)
    if not os.path.exists(path):
        raise DynaAlignError(
            DA_ERR_NO_DEVICE,
            "libdynaalign_hip.so not found at %s -- build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(dynaalign_amd has no CPU fallback)" % path)
    try:  # if torch is around, let its bundled libamdhip64.so.7 be the one HIP runtime in the process
        import torch  # noqa: F401
    except Exception:
        pass
    lib = C.CDLL(path, mode=C.RTLD_GLOBAL)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    _lib = _Library(lib)
    return _lib


def _switches():
    return tuple(sorted((k, v) for k, v in os.environ.items() if k.startswith("DYNAALIGN_")))


class _Library:
    """The loaded library.  The C side parses its DYNAALIGN_* switches once (da_common.hpp Config); tests, bench.py and the tools flip
    switches inside one process, so this front end calls the library's reload hook whenever the process's DYNAALIGN_* environment
    differs from what it was at the previous call -- the library itself never looks at the environment again."""

    def __init__(self, cdll):
        object.__setattr__(self, "_cdll", cdll)
        object.__setattr__(self, "_seen", _switches())

    def __getattr__(self, name):
        fn = getattr(self._cdll, name)
        if name != "da_config_reload":
            now = _switches()
            if now != self._seen:
                self._cdll.da_config_reload()
                object.__setattr__(self, "_seen", now)
        return fn


def check(rc):
    if rc != DA_OK:
        raise DynaAlignError(rc, load().da_last_error().decode("latin-1"))


def ptr(a):
    """numpy array -> void* (None passes NULL)"""
    return None if a is None else a.ctypes.data
