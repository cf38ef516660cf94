"""What the compiled cosine_i8_screen does with a tile's survivors (csrc/cosine_screen_i8.hip), read off the gfx950
assembly.

A passing tile test leaves its s~ and e_r in two registers of the lane.  When no lane of the wave tested more than one pair in,
the survivors are appended from those registers: the lane's slot from v_mbcnt over the ballot of the lanes that have a pair, the
key from one fma and one subtraction, two LDS stores.  The wave is alone on its SIMD and nothing runs behind this code, so the
design promises that it reads neither the metadata slot nor the sums again (no ds_read, no s_set_gpr_idx), runs no DPP chain and
no loop, and that the two capture registers cost no spill.  Nothing in the source language holds the compiler to that.  For every
instantiation the launcher can pick this module checks:

  * no scratch and no VGPR spill, occupancy 1;
  * after the last MFMA exactly one block computes a lane rank (v_mbcnt_lo / v_mbcnt_hi): the append.  It is straight-line, holds
    one ds_write_b64 and one ds_write_b32, and no ds_read, s_set_gpr_idx_on, DPP, v_readlane, v_cvt_f32_i32 or v_mul_f32;
  * the choice of that block is made before anything is read again: from the last MFMA down to the first DPP instruction (where
    the path of the tiles with a lane at two pairs begins) there is no ds_read and no s_set_gpr_idx_on;
  * the captures are selects inside the span: between the first and the last MFMA there is no branch and no write of exec,
    and at least 16 x (NQT + 1) v_cndmask_b32 -- one per tested pair for s~, and one per register row for e_r if the compiler
    merges the query tiles' selects of the same row's e_r (it need not; the count is printed).

A guard against the path being undone quietly; not a speed claim."""
import re

from test_screen_i8_schedule import EXPECTED, MFMA, compiled, pytestmark  # noqa: F401  (the fixture compiles the file once more)

LABEL = re.compile(r"^(\.LBB\d+_\d+):|^; %bb\.\d+:")
MBCNT = re.compile(r"^\s*v_mbcnt_(lo|hi)_u32_b32\b")
FORBIDDEN = re.compile(r"^\s*(ds_read\w*|s_set_gpr_idx_on|v_readlane_b32|v_cvt_f32_i32\w*|v_mul_f32\w*|s_cbranch\w*|\w+_dpp)\b")
REREAD = re.compile(r"^\s*(ds_read\w*|s_set_gpr_idx_on)\b")
DPP = re.compile(r"^\s*\w+_dpp\b|\brow_shr:|\brow_bcast:")
CNDMASK = re.compile(r"^\s*v_cndmask_b32")


def _after_span(lines):
    at = [i for i, l in enumerate(lines) if MFMA.match(l)]
    assert at, "no v_mfma_i32_32x32x32_i8 in the kernel"
    return lines[at[0]:at[-1] + 1], lines[at[-1] + 1:]


def _blocks(lines):
    out, cur = [], []
    for l in lines:
        if LABEL.match(l):
            out.append(cur)
            cur = []
        cur.append(l)
    out.append(cur)
    return out


def test_capture_registers_do_not_spill(compiled):
    asm, remarks = compiled
    for key in sorted(EXPECTED):
        r = remarks[key]
        assert int(r["ScratchSize [bytes/lane]"]) == 0 and int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, (key, r)
        assert int(r["Occupancy [waves/SIMD]"]) == 1, (key, r)
        assert not [l for l in asm[key] if re.match(r"^\s*scratch_(load|store)", l)], key


def test_append_from_the_captures_reads_nothing_again(compiled):
    asm, _ = compiled
    for key in sorted(EXPECTED):
        _, tail = _after_span(asm[key])
        ranked = [b for b in _blocks(tail) if any(MBCNT.match(l) for l in b)]
        assert len(ranked) == 1, (key, len(ranked))
        block = ranked[0]
        bad = [l.strip() for l in block if FORBIDDEN.match(l) or DPP.search(l)]
        n64 = sum(1 for l in block if re.match(r"^\s*ds_write_b64\b", l))
        n32 = sum(1 for l in block if re.match(r"^\s*ds_write_b32\b", l))
        print("cosine_i8_screen<d=%d, NQT=%d, FILT=%s>: the append from the captures is %d instructions"
              % (key + (sum(1 for l in block if re.match(r"^\s+[a-z]", l)),)))
        assert not bad, (key, bad)
        assert (n64, n32) == (1, 1), (key, n64, n32)


def test_path_is_chosen_before_anything_is_read_again(compiled):
    asm, _ = compiled
    for key in sorted(EXPECTED):
        _, tail = _after_span(asm[key])
        first_dpp = next((i for i, l in enumerate(tail) if DPP.search(l)), None)
        assert first_dpp is not None, key
        bad = [l.strip() for l in tail[:first_dpp] if REREAD.match(l)]
        assert not bad, (key, bad)


def test_captures_are_selects_inside_the_span(compiled):
    asm, _ = compiled
    for key in sorted(EXPECTED):
        d, nqt, _f = key
        span, _ = _after_span(asm[key])
        n = sum(1 for l in span if CNDMASK.match(l))
        print("cosine_i8_screen<d=%d, NQT=%d, FILT=%s>: %d v_cndmask_b32 between the first and the last MFMA" % (key + (n,)))
        bad = [l.strip() for l in span if re.match(r"^\s*(s_cbranch\w*|s_\w+_saveexec_b64|s_mov_b64 exec\b)", l)]
        assert not bad, (key, bad)
        assert n >= 16 * (nqt + 1), (key, n)
