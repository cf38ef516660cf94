"""Where the compiled cosine_i8_screen runs its tile test (csrc/cosine_screen_i8.hip), read off the gfx950 assembly.

The test of a tile (an i32 -> f32 conversion, two multiplies, an fma and a compare per query tile and register row) runs one tile
late, a slice per k-step inside the next tile's matrix span, where the matrix pipe covers it and the ring's pieces keep being
issued.  Nothing in the source language keeps it there: left alone the compiler moves the slices out of the span or behind its
last MFMA, and pairs the two query tiles' products into packed-f32 instructions between the MFMAs (the form DESIGN section 7
found losing products there).  For the four d = 768 instantiations this module checks that the span holds the 16 x NQT
conversions of the test and no v_pk_*_f32 at all; for d = 384 it prints the counts.

A guard against the schedule being undone quietly; not a speed claim."""
import re

from test_screen_i8_schedule import EXPECTED, MFMA, compiled, pytestmark  # noqa: F401  (the fixture compiles the file once more)

CVT = re.compile(r"^\s*v_cvt_f32_i32(_e32|_e64)?\s")
PK_F32 = re.compile(r"^\s*v_pk_\w+_f32\b")


def _span(lines):
    at = [i for i, l in enumerate(lines) if MFMA.match(l)]
    assert at, "no v_mfma_i32_32x32x32_i8 in the kernel"
    return lines[at[0]:at[-1] + 1]


def test_tile_test_sits_inside_the_matrix_span(compiled):
    asm, _ = compiled
    for key in sorted(EXPECTED):
        d, nqt, _f = key
        span = _span(asm[key])
        n_cvt = sum(1 for l in span if CVT.match(l))
        n_pk = sum(1 for l in span if PK_F32.match(l))
        print("cosine_i8_screen<d=%d, NQT=%d, FILT=%s>: %d v_cvt_f32_i32 and %d v_pk_*_f32 between the first and the last MFMA"
              % (key + (n_cvt, n_pk)))
        if d == 768:
            assert n_cvt == 16 * nqt, (key, n_cvt)
            assert n_pk == 0, (key, [l.strip() for l in span if PK_F32.match(l)])
