"""The ctypes binding that _lib derives from include/smx.h, without a GPU and without the library.

tests/golden/abi_signatures.txt is the binding as it stood while it was a hand-kept table (written once by render()
below from that table): every entry's result and argument types, the field lists of the three structs, and the SMX_*
values the Python side spelled as literals.  The derived binding must equal it line for line.  The reader itself is
then tried on small made-up headers."""
import ctypes
import os

import pytest

from conftest import GOLDEN

from tensor_cuda_fft_amd import _lib

CODES = {ctypes.c_int: "i", ctypes.c_longlong: "q", ctypes.c_size_t: "z", ctypes.c_float: "f",
         ctypes.c_char_p: "s", ctypes.c_void_p: "P"}
CODES.setdefault(ctypes.c_ulonglong, "Q")          # where size_t is unsigned long long, ctypes has one object for both
STRUCTS = ("smx_plan", "smx_options", "smx_shape")
CONSTANTS = ("SMX_PATH_DECIMATED", "SMX_PATH_DIRECT", "SMX_PATH_DECIM16", "SMX_IO_F32", "SMX_IO_BF16", "SMX_IO_F16",
             "SMX_PHASE_SPECTRUM", "SMX_PHASE_INVERSE", "SMX_PHASE_PARAMS", "SMX_PHASE_ALL", "SMX_EMA_ALIGNED",
             "SMX_EMA_POLAR", "SMX_XENT_MEAN", "SMX_XENT_SUM", "SMX_XENT_NONE", "SMX_FILTER_PACK_READY")


def spell(t) -> str:
    """one ctypes type: a letter for a scalar, char* and void*; [target] for a typed pointer, so that
    POINTER(smx_shape), POINTER(c_size_t) and c_void_p all read differently"""
    if t in CODES:
        return CODES[t]
    target = t._type_                              # KeyError / AttributeError: a type this file does not know
    return "[" + (CODES[target] if target in CODES else target.__name__) + "]"


def render(sigs: dict, fields: dict, constants: dict) -> list:
    """sigs {entry: (restype, [argtypes])}, fields {struct: _fields_}, constants {SMX_NAME: value} as the lines of
    abi_signatures.txt: entries by name, struct fields in their order"""
    lines = [f"{name} {spell(res)}({''.join(spell(a) for a in args)})" for name, (res, args) in sorted(sigs.items())]
    lines += [f"struct {s} " + " ".join(f"{n}:{spell(t)}" for n, t in fields[s]) for s in STRUCTS]
    lines += [f"const {c} {constants[c]}" for c in CONSTANTS]
    return lines


def test_derived_binding_equals_the_recorded_table():
    want = open(os.path.join(GOLDEN, "abi_signatures.txt")).read().splitlines()
    got = render(_lib._SIGS, {s: getattr(_lib, s)._fields_ for s in STRUCTS},
                 {c: getattr(_lib, c) for c in CONSTANTS})
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w
    assert spell(ctypes.POINTER(_lib.smx_shape)) != spell(ctypes.c_void_p) != spell(ctypes.POINTER(ctypes.c_size_t))


def test_the_glue_names_the_header_values():
    """the public constants keep their names and are the header's values"""
    from tensor_cuda_fft_amd import functional as fn
    assert (fn.PHASE_SPECTRUM, fn.PHASE_INVERSE, fn.PHASE_PARAMS, fn.PHASE_ALL) == (1, 2, 4, 7)
    assert fn.EMA_MODES == {"aligned": 0, "polar": 1}
    assert fn._XENT_REDUCTION == {"mean": 0, "sum": 1, "none": 2}
    assert (_lib.SMX_IO_F32, _lib.SMX_IO_BF16, _lib.SMX_IO_F16) == (0, 1, 2)
    assert (_lib.SMX_PATH_DECIMATED, _lib.SMX_PATH_DIRECT, _lib.SMX_PATH_DECIM16) == (1, 2, 3)
    assert _lib.SMX_VERSION == 303 and _lib.SMX_ERR_WORKSPACE == -4


# ---- the reader on made-up headers ----------------------------------------------------------------------------------
TEXT = """
/* made.h -- smx_fake(int) is mentioned here, and so is an unbalanced ( parenthesis,
 * over two lines */
#ifndef SMX_H_
#define SMX_H_
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif
#define SMX_X (-4)     /* a comment with smx_other( in it */
#define SMX_Y 12
#define SMX_RATIO 1.5
#define SMX_NAME "text"
#define SMX_SUM (SMX_Y + 1)
typedef struct smx_pair {
  int a, b,
      c;        /* between fields: int smx_hidden(int); */
  int d;
} smx_pair;
int smx_none(void);
unsigned long long smx_count(void);
const char* smx_text(int code);
int
smx_three(const float* x,   /* the input ( */
          long long n, size_t bytes,
          float scale, void* stream);
int smx_ptrs(const long long* targets, unsigned long long* out2, const smx_shape* shape, smx_plan* plan,
             size_t* bytes, smx_options* opts, const smx_options* in, const char* name, const void* raw);
int smx_wide(unsigned long long seed, int);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_reader_on_a_made_up_header():
    P, I, LL, SZ, ULL = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_size_t, ctypes.c_ulonglong
    sigs, defines, structs = _lib.read_header(TEXT)
    assert sigs == {
        "smx_none": (I, []),
        "smx_count": (ULL, []),
        "smx_text": (ctypes.c_char_p, [I]),
        "smx_three": (I, [P, LL, SZ, ctypes.c_float, P]),
        "smx_ptrs": (I, [P, P, ctypes.POINTER(_lib.smx_shape), ctypes.POINTER(_lib.smx_plan), ctypes.POINTER(SZ),
                         P, P, ctypes.c_char_p, P]),
        "smx_wide": (I, [ULL, I]),                     # a parameter without a name
    }
    assert list(sigs) == ["smx_none", "smx_count", "smx_text", "smx_three", "smx_ptrs", "smx_wide"]
    assert defines == {"SMX_X": -4, "SMX_Y": 12}       # no value, a float, a string, an expression: ignored
    assert structs == {"smx_pair": ["a", "b", "c", "d"]}


@pytest.mark.parametrize("proto, entry, ctype", [
    ("int smx_bad(const float* x, double alpha, void* stream);", "smx_bad", "double"),
    ("short smx_res(int n);", "smx_res", "short"),
    ("int smx_long(long n);", "smx_long", "long"),
    ("int smx_byval(smx_shape shape);", "smx_byval", "smx_shape"),
])
def test_reader_refuses_a_type_outside_its_vocabulary(proto, entry, ctype):
    with pytest.raises(_lib.SmxError) as e:
        _lib.read_header("int smx_fine(int n);\n" + proto + "\n")
    assert entry in str(e.value) and repr(ctype) in str(e.value) and "smx_fine" not in str(e.value)


def test_reader_refuses_a_struct_field_that_is_not_an_int():
    with pytest.raises(_lib.SmxError, match="smx_box.*float w"):
        _lib.read_header("typedef struct smx_box { int a; float w; } smx_box;")


def test_missing_header_is_an_error_not_a_fallback(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "HEADER_PATH", str(tmp_path / "include" / "smx.h"))
    with pytest.raises(_lib.SmxError, match="smx.h not found"):
        _lib._read_header_file()
