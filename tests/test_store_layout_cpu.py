"""The placement of the write-back rows of the streaming stores (option "st_layout", csrc/smx_kernels.h store_layout,
csrc/smx_launch.h st_tile_mask) as a pure-Python model: which of a thread's 16 rows per tile are stored with the
write-back policy, for every (layout, count, tile residue r, wave w).  No GPU.

    mask(u) = bit u of rot16(base, s),  rot16(m, s): bit u of the result = bit (u + s) mod 16 of m
    base = 0x1111 / 0x0101 / 0x0001 / 0 for count 4 / 2 / 1 / 0 (period 16 / count); layout -1: the low `count` bits
    s = 0 | r | r >> 2 | w | w + r for layout 0 | 1 | 2 | 3 | 4

What the layouts exist for is balance: over the 16 residues x 4 waves of a workgroup every row u is deferred equally
often.  With four write-back rows (period 4) that holds for each of the layouts 1-4, and with s = r or s = w + r
(layouts 1, 4) for every count.  Layouts 2 and 3 draw s from FOUR values (r >> 2 of 16 residues, the wave index), so with
count 2 (period 8) or 1 (period 16) they cannot reach all 16 rows whatever the rotation's direction or origin: 4 values
of s times `count` bits reach at most 4 * count rows.  For those four (layout, count) pairs the test asks for the
most that can hold: exactly 4 * count rows are reached, each equally often.
"""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUTS = (-1, 0, 1, 2, 3, 4)
COUNTS = (0, 1, 2, 4)


def rot16(m, s):
    s &= 15
    return ((m >> s) | (m << (16 - s))) & 0xFFFF


def store_layout(count, layout):
    """(st_mask, st_rsh, st_wsh) as csrc/smx_kernels.h store_layout() fills them; a shift of 30 switches a term off"""
    rsh = wsh = 30
    if layout < 0 or layout > 4:
        return (1 << count) - 1, rsh, wsh
    base = {4: 0x1111, 2: 0x0101, 1: 0x0001, 0: 0}[count]
    if layout in (1, 4):
        rsh = 0
    if layout == 2:
        rsh = 2
    if layout in (3, 4):
        wsh = 0
    return base, rsh, wsh


def tile_mask(count, layout, r, w):
    base, rsh, wsh = store_layout(count, layout)
    return rot16(base, (r >> rsh) + (w >> wsh))


def test_rot16_is_a_rotation():
    for m in (0x1111, 0x0101, 0x0001, 0x8001, 0xFFFF, 0):
        for s in range(40):
            got = rot16(m, s)
            assert got == sum(((m >> ((u + s) % 16)) & 1) << u for u in range(16))
            assert bin(got).count("1") == bin(m).count("1")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("count", COUNTS)
def test_every_tile_defers_exactly_count_rows(layout, count):
    for r in range(256):                       # residues up to the longest decimation (L = 256)
        for w in range(4):
            assert bin(tile_mask(count, layout, r, w)).count("1") == count


@pytest.mark.parametrize("count", (1, 2, 4))
def test_fixed_patterns(count):
    for r in range(16):
        for w in range(4):
            assert tile_mask(count, -1, r, w) == (1 << count) - 1                      # the thread's first rows
            assert tile_mask(count, 0, r, w) == sum(1 << u for u in range(0, 16, 16 // count))


def test_layout_1_is_the_measured_row_granular_form():
    """row (u, r) write-back iff (u + r) mod 4 = 0; layout 4 adds the wave index"""
    for r in range(16):
        for w in range(4):
            for u in range(16):
                assert (tile_mask(4, 1, r, w) >> u) & 1 == ((u + r) % 4 == 0)
                assert (tile_mask(4, 4, r, w) >> u) & 1 == ((u + r + w) % 4 == 0)
                assert (tile_mask(4, 2, r, w) >> u) & 1 == ((u + (r >> 2)) % 4 == 0)
                assert (tile_mask(4, 3, r, w) >> u) & 1 == ((u + w) % 4 == 0)


def _hits(count, layout):
    h = [0] * 16
    for r in range(16):
        for w in range(4):
            m = tile_mask(count, layout, r, w)
            for u in range(16):
                h[u] += (m >> u) & 1
    return h


@pytest.mark.parametrize("layout", (1, 2, 3, 4))
@pytest.mark.parametrize("count", (1, 2, 4))
def test_balance_over_a_workgroup(layout, count):
    h = _hits(count, layout)
    assert sum(h) == 64 * count
    if layout in (2, 3) and count < 4:         # four values of s, period > 4: see the module docstring
        reached = [x for x in h if x]
        assert len(reached) == 4 * count and set(reached) == {64 * count // (4 * count)}
    else:
        assert set(h) == {4 * count}           # every u equally often


def test_model_matches_the_sources():
    """the constants of the model are the ones in the C++ (a changed base mask or shift must change this file too)"""
    csrc = os.path.join(ROOT, "tensor-cuda-fft-_amd", "csrc")
    k = open(os.path.join(csrc, "smx_kernels.h")).read()
    body = k[k.index("static inline void store_layout("):]
    body = body[:body.index("\n}\n")]
    assert "a.st_rsh = a.st_wsh = 30;" in body
    assert "(1u << c) - 1u" in body
    assert re.search(r"c == 4 \? 0x1111u : c == 2 \? 0x0101u : c == 1 \? 0x0001u : 0u", body)
    assert "if (layout == 1 || layout == 4) a.st_rsh = 0;" in body
    assert "if (layout == 2) a.st_rsh = 2;" in body
    assert "if (layout == 3 || layout == 4) a.st_wsh = 0;" in body
    la = open(os.path.join(csrc, "smx_launch.h")).read()
    assert "return ((m >> s) | (m << (16u - s))) & 0xffffu;" in la
    assert "rot16(a.st_mask, (unsigned)((r >> a.st_rsh) + sw))" in la
    d = open(os.path.join(csrc, "smx_decim.hip")).read()
    assert "(__builtin_amdgcn_readfirstlane(t) >> 2) >> a.st_wsh" in d      # wave w = t >> 2, 64 lanes = 4 row groups


def test_option_names_are_accepted():
    from tensor_cuda_fft_amd import _lib
    try:
        for name in ("st_layout", "st_layout_fwd", "st_layout_bwd"):
            for v in (-2, -1, 0, 1, 2, 3, 4):
                _lib.set_option(name, v)
        with pytest.raises(_lib.SmxError):
            _lib.set_option("st_layout_sideways", 1)
    finally:
        _lib.set_option("st_layout", -2)
