"""ctypes binding of libsmx.so, derived from include/smx.h (and the headers it includes, EXT_HEADERS and MORE_HEADERS) when this module is
imported: the entry points' signatures, the fields of the three structs and the SMX_* constants are read from the
header's text, so an entry point is declared there and nowhere else on the Python side.  No CPU fallback: if the library is missing the import of the product path
fails with a build hint."""
from __future__ import annotations

import ctypes
import os
import re
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
# SMX_LIB selects an experimental build of the same ABI (tuning only)
LIB_PATH = os.environ.get("SMX_LIB") or os.path.join(_HERE, "csrc", "libsmx.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "smx.h")      # the layout csrc/build.sh relies on too
# headers that smx.h includes (the reader does not follow #include): entry points added since the table of smx.h's own
# signatures was recorded (tests/golden/abi_signatures.txt); theirs is tests/golden/abi_signatures_ext.txt
EXT_HEADERS = ("smx_freq.h",)
# headers added after THAT table was recorded: one table per header ({header: prototypes}, _SIGS_MORE), each recorded in a
# file of its own (smx_fconv.h: tests/golden/abi_signatures_fconv.txt, smx_quant.h: tests/golden/abi_signatures_quant.txt,
# smx_rowfft.h: tests/golden/abi_signatures_rowfft.txt)
MORE_HEADERS = ("smx_fconv.h", "smx_quant.h", "smx_rowfft.h")


class SmxError(RuntimeError):
    pass


class smx_plan(ctypes.Structure):           # the _fields_ of these three are the header's (below)
    pass


class smx_options(ctypes.Structure):
    pass


class smx_shape(ctypes.Structure):
    pass


_lock = threading.Lock()
_lib = None

_P = ctypes.c_void_p
_SZ = ctypes.c_size_t

# the header's vocabulary: scalar types, and the pointers that are not a plain address (what stands before the `*`)
_SCALARS = {"int": ctypes.c_int, "long long": ctypes.c_longlong, "size_t": _SZ, "float": ctypes.c_float,
            "unsigned long long": ctypes.c_ulonglong}
_POINTERS = {"const char": ctypes.c_char_p, "smx_plan": ctypes.POINTER(smx_plan),
             "const smx_shape": ctypes.POINTER(smx_shape), "size_t": ctypes.POINTER(_SZ)}
_STRUCT = re.compile(r"typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;")


def _ctype(entry: str, decl: str):
    """`decl`: a result type, or one parameter with or without its name"""
    words = decl.replace("*", " * ").split()
    if "*" in words:
        return _POINTERS.get(" ".join(words[:words.index("*")]), _P)
    for cand in (words, words[:-1]):
        if " ".join(cand) in _SCALARS:
            return _SCALARS[" ".join(cand)]
    raise SmxError(f"smx.h: {entry}: the type {' '.join(words[:-1] or words)!r} is not one the binding knows "
                   f"({', '.join(_SCALARS)}, or a pointer): teach _lib._SCALARS before declaring it.")


def read_header(text: str):
    """(prototypes {entry: (restype, [argtypes])}, integer defines {SMX_NAME: value}, struct fields {struct: [names]})
    of the header's text.  No C parser: comments go first (they hold `smx_...(` and parentheses), then the preprocessor
    lines and the typedef'd structs (int fields only, several declarators a line), and what is left is prototypes:
    `type smx_name(parameters);` over any number of lines, (void) for none, types from the vocabulary above."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    defines = {n: int(v) for n, v in
               re.findall(r"^[ \t]*#[ \t]*define[ \t]+(SMX_\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$", text, flags=re.M)}
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    structs = {}
    for body, name in _STRUCT.findall(text):
        decls = [d.split(None, 1) for d in body.split(";") if d.strip()]
        for d in decls:
            if d[0] != "int" or len(d) != 2 or not re.fullmatch(r"[\w\s,]+", d[1]):
                raise SmxError(f"smx.h: struct {name}: the field {' '.join(d)!r} is not a plain int")
        structs[name] = [f for d in decls for f in d[1].replace(",", " ").split()]
    sigs = {}
    for res, name, params in re.findall(r"([\w\s*]+?)\b(smx_\w+)\s*\(([^()]*)\)\s*;", _STRUCT.sub("", text)):
        params = [] if params.strip() in ("", "void") else params.split(",")
        sigs[name] = (_ctype(name, res), [_ctype(name, p) for p in params])
    return sigs, defines, structs


def _read_header_file():
    if not os.path.exists(HEADER_PATH):
        raise SmxError(f"{HEADER_PATH} not found: the ctypes binding is read from the C header, which the source tree "
                       f"keeps beside the package directory. There is no built-in copy of the signatures.")
    with open(HEADER_PATH) as f:
        return read_header(f.read())


def _read_ext_headers(names=None):
    """(prototypes, integer defines) of the EXT_HEADERS (or `names`) beside smx.h: entry points and constants only, no
    structs, and no name that smx.h already declares"""
    sigs, defines = {}, {}
    for name in EXT_HEADERS if names is None else names:
        path = os.path.join(os.path.dirname(HEADER_PATH), name)
        if not os.path.exists(path):
            raise SmxError(f"{path} not found: smx.h includes it, and the ctypes binding of its entry points is read from it.")
        with open(path) as f:
            s, d, st = read_header(f.read())
        if st or set(s) & (set(sigs) | set(_SIGS)):
            raise SmxError(f"{name}: an extension header declares entry points of its own and no structs")
        sigs.update(s)
        defines.update(d)
    return sigs, defines


_SIGS, _DEFINES, _FIELDS = _read_header_file()
_SIGS_EXT, _DEFINES_EXT = _read_ext_headers()
_SIGS_MORE, _DEFINES_MORE = {}, {}
for _h in MORE_HEADERS:
    _SIGS_MORE[_h], _DEFINES_MORE[_h] = _read_ext_headers((_h,))
    if set(_SIGS_MORE[_h]) & set(_SIGS_EXT):
        raise SmxError(f"{_h}: an extension header declares entry points of its own")
for _s in (smx_plan, smx_options, smx_shape):
    _s._fields_ = [(n, ctypes.c_int) for n in _FIELDS[_s.__name__]]
globals().update(_DEFINES)                  # SMX_PATH_*, SMX_IO_*, SMX_PHASE_*, SMX_ERR_* ...: every integer #define
globals().update(_DEFINES_EXT)
for _d in _DEFINES_MORE.values():
    globals().update(_d)


_SINCE = {"smx_diag_clock": 302, "smx_dwconv3_workspace_bytes": 302, "smx_dwconv3_forward": 302,
          "smx_dwconv3_backward": 302, "smx_spectral_ln_supported": 302, "smx_spectral_ln_forward": 302,
          "smx_spectral_ln_backward": 302, "smx_planar_cmul_forward": 302, "smx_planar_cmul_backward": 302,
          "smx_planar_add": 302, "smx_planar_split": 302, "smx_spectral_gate_workspace_bytes": 303,
          "smx_spectral_gate_forward": 303, "smx_spectral_gate_backward": 303, "smx_mix_workspace_bytes": 303,
          "smx_mix_forward": 303, "smx_mix_backward": 303, "smx_enh_supported": 303, "smx_enh_workspace_bytes": 303,
          "smx_rope_norm_forward": 303, "smx_rope_norm_backward": 303, "smx_residual_norm_forward": 303,
          "smx_residual_norm_backward": 303, "smx_gate_blend_forward": 303, "smx_gate_blend_backward": 303,
          "smx_io_supported": 303, "smx_forward_io": 303, "smx_backward_io": 303, "smx_conv_io_supported": 303,
          "smx_conv_forward_io": 303, "smx_conv_backward_io": 303, "smx_block_io_supported": 303,
          "smx_block_forward_io": 303, "smx_block_backward_io": 303}        # entry points younger than the oldest library the A/B tools still load


def load(path: str):
    """dlopen one build of the library and declare its signatures (tools/ab_inproc.py loads several)."""
    import torch  # noqa: F401  (maps torch's libamdhip64 before ours resolves it)
    h = ctypes.CDLL(path)
    for name, (res, args) in {**_SIGS, **_SIGS_EXT, **{n: v for t in _SIGS_MORE.values() for n, v in t.items()}}.items():
        if name in _SINCE and h.smx_version() < _SINCE[name]:
            continue                       # an older build loaded beside the current one (A/B tools only)
        fn = getattr(h, name)
        fn.restype = res
        fn.argtypes = args
    check_build_flags((h.smx_build_flags() or b"").decode(), path)
    return h


def check_build_flags(flags: str, path: str) -> None:
    """Refuse a library built with -DSMX_AB_* (csrc/build.sh with a mis-set SMX_EXTRA): same ABI, same
    smx_version(), garbage results."""
    if "SMX_AB_" in flags and os.environ.get("SMX_ALLOW_ABLATION") != "1":
        raise SmxError(f"{path} is a timing-ablation build ({flags.strip()}): it returns wrong results by design. "
                       f"Rebuild with csrc/build.sh (no SMX_EXTRA), or set SMX_ALLOW_ABLATION=1 for tools/ab.sh.")


def lib():
    """Load libsmx.so once.  torch must be imported first so the HIP runtime torch uses is the
    one this library binds to (same SONAME, already mapped)."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise SmxError(
                f"{LIB_PATH} not found: the HIP library is not built. Run "
                f"`python -c 'import __graft_entry__ as g; g.build()'` or "
                f"`{os.path.join(_HERE, 'csrc', 'build.sh')}`. There is no CPU fallback.")
        _lib = load(LIB_PATH)
    return _lib


def check(rc: int) -> None:
    if rc != 0:
        msg = lib().smx_last_error()
        raise SmxError(f"libsmx error {rc}: {msg.decode() if msg else '?'}")


def plan(B: int, N: int, D: int, F: int) -> smx_plan:
    p = smx_plan()
    check(lib().smx_plan_query(B, N, D, F, ctypes.byref(p)))
    return p


def io_supported(B: int, N: int, D: int, F: int, io: int) -> bool:
    """True when the plan of this layer shape (current options) reads and writes `io` elements natively."""
    return bool(lib().smx_io_supported(B, N, D, F, io))


def block_io_supported(B: int, N: int, D: int, F: int, io: int) -> bool:
    """True when the fused block line of this shape (current options) reads and writes `io` elements natively."""
    return bool(lib().smx_block_io_supported(B, N, D, F, io))


def conv_io_supported(B: int, R: int, D: int, n_fft: int, io: int) -> bool:
    """True when smx_conv_* runs this shape (current options) with `io` rows natively (the single-launch plan)."""
    sh = smx_shape(B, R, D, n_fft // 2 + 1, n_fft, n_fft // 2 + 1)
    return bool(lib().smx_conv_io_supported(ctypes.byref(sh), io))


def workspace_bytes(B: int, N: int, D: int, F: int) -> int:
    s = _SZ()
    check(lib().smx_workspace_bytes(B, N, D, F, ctypes.byref(s)))
    return int(s.value)


def plan_ex(sh: smx_shape) -> smx_plan:
    p = smx_plan()
    check(lib().smx_plan_query_ex(ctypes.byref(sh), ctypes.byref(p)))
    return p


def workspace_bytes_ex(sh: smx_shape) -> int:
    s = _SZ()
    check(lib().smx_workspace_bytes_ex(ctypes.byref(sh), ctypes.byref(s)))
    return int(s.value)


def set_option(name: str, value: int) -> None:
    """Process-wide default of a plan knob (include/smx.h).  Nothing needs clearing on the Python side: every
    per-shape memo in functional.py is keyed by opts_key(), which changes with the library's options epoch."""
    check(lib().smx_set_option(name.encode(), int(value)))


_tls = threading.local()


def opts_key() -> tuple:
    """What the plan of a shape depends on besides the shape: the library's process-wide options epoch and this
    thread's scoped overrides (options())."""
    return (int(lib().smx_options_epoch()), getattr(_tls, "stack", ()))


def current_options():
    """The innermost options this thread has pushed, as a dict (None: the process-wide defaults apply)."""
    st = getattr(_tls, "stack", ())
    return dict(zip((n for n, _ in smx_options._fields_), st[-1])) if st else None


def effective_options() -> dict:
    """The options in force for this thread right now, ALWAYS a full dict: the innermost scoped push, or a snapshot of
    the process-wide defaults.  What an autograd node notes in forward and re-applies around its backward, so that
    neither the autograd thread's empty scope nor a set_option() between the two halves can make them plan
    differently (another workspace layout, another save layout of the one-launch convolution)."""
    cur = current_options()
    if cur is not None:
        return cur
    o = smx_options()
    check(lib().smx_options_default(ctypes.byref(o)))
    return {n: int(getattr(o, n)) for n, _ in smx_options._fields_}


class options:
    """`with _lib.options(nsplit=2, fourstep=0): ...` -- the calls made by THIS thread inside the block plan with
    these knobs instead of the process-wide defaults (smx_options_push / smx_options_pop): plan choice as an
    argument of the calling context, so two users of one process can run different plans."""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        o = smx_options()
        check(lib().smx_options_default(ctypes.byref(o)))
        for k, v in self.kw.items():
            if not hasattr(o, k):
                raise ValueError(f"unknown plan option {k!r}")
            setattr(o, k, int(v))
        check(lib().smx_options_push(ctypes.byref(o)))
        vals = tuple(getattr(o, n) for n, _ in smx_options._fields_)
        _tls.stack = getattr(_tls, "stack", ()) + (vals,)
        return self

    def __exit__(self, *a):
        _tls.stack = _tls.stack[:-1]
        check(lib().smx_options_pop())
