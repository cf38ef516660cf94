"""The compiled schedule of the three bf16 screen kernels that share csrc/oi_screen_tile.h, read off the gfx950 assembly.

cosine_copy_screen (cosine_screen_copy.hip), vo_stream_kernel (oi_volume.h: cosine_volume.hip with VoCount, cosine_summary.hip with
SmSum) and cosine_screen_filter (cosine_prefilter.hip) stream a corpus through a per-wave LDS ring that is filled by LDS-DMA loads
hipcc cannot see and ordered by counted waits, s_waitcnt vmcnt(4 (P - 1)) with P slots ahead.  One load the compiler does know
about in the wrong place and it waits with vmcnt(0) inside the tile loop: the ring drains, nothing fails, the stream slows down.
This module compiles the four files the way openintel_amd/build.py does and checks, for each of the 28 instantiations the
launchers can pick:

  * no scratch, no VGPR or SGPR spill, occupancy 1;
  * NQT x D / 16 v_mfma_f32_32x32x16_bf16: one unrolled tile;
  * between the first and the last MFMA every s_waitcnt that names vmcnt is the counted one, and there are NKC - 1 of them
    (NKC ring slots per tile: the wait in front of slot 0 sits before the first MFMA).

A guard against the ring being drained quietly; not a speed claim."""
import os
import re
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor

import pytest

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")

FILES = ("cosine_screen_copy.hip", "cosine_volume.hip", "cosine_summary.hip", "cosine_prefilter.hip")
COPY = re.compile(r"^_Z\d+cosine_copy_screenILi(\d+)ELi(\d+)ELi(\d+)ELb([01])EE")
VO = re.compile(r"^_Z\d+vo_stream_kernelILi(\d+)ELi(\d+)ELi(\d+)ELb([01])E\d+(VoCount|SmSum)E")
F32 = re.compile(r"^_Z\d+cosine_screen_filterILi(\d+)ELi(\d+)EE")
MFMA = re.compile(r"^\s*v_mfma_f32_32x32x16_bf16\b")
VMCNT = re.compile(r"^\s*s_waitcnt\b.*\bvmcnt\((\d+)\)")
NBUF = 8   # OI_COPY_NBUF_DEFAULT and VO_NBUF: the depth the product launches

EXPECTED = ({("copy", d, nqt, filt) for d in (384, 768) for nqt in (1, 2) for filt in (False, True)}
            | {(t, d, nqt, filt) for t in ("VoCount", "SmSum") for d in (384, 768) for nqt in (1, 2) for filt in (False, True)}
            | {("f32", d, nqt, False) for d in (384, 768) for nqt in (1, 2)})


def _key(mangled):
    m = COPY.match(mangled)
    if m:
        return ("copy", int(m.group(1)), int(m.group(2)), m.group(4) == "1") if int(m.group(3)) == NBUF else None
    m = VO.match(mangled)
    if m:
        return (m.group(5), int(m.group(1)), int(m.group(2)), m.group(4) == "1") if int(m.group(3)) == NBUF else None
    m = F32.match(mangled)
    return ("f32", int(m.group(1)), int(m.group(2)), False) if m else None


def ring(key):
    """(NKC, P) of an instantiation: ring slots per tile and slots in flight ahead of the one being consumed."""
    fam, d = key[0], key[1]
    if fam == "f32":   # 32 floats per slot row; the compile-time ring's depth divides the tile's slot count
        nkc = d // 32
        return nkc, (8 if nkc % 8 == 0 else 6 if nkc % 6 == 0 else nkc) - 1
    return d // 64, NBUF - 1


def _compile(src):
    from openintel_amd import build as b
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        r = subprocess.run([b.HIPCC, *b.FLAGS, "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage",
                            os.path.join(b.CSRC, src), "-o", out], capture_output=True, text=True, cwd=tmp)
        assert r.returncode == 0, r.stderr[-4000:]
        with open(out) as f:
            return f.read(), r.stderr


@pytest.fixture(scope="module")
def compiled():
    """({instantiation: assembly lines}, {instantiation: {remark name: value}}) of the four files with the library's flags."""
    asm, remarks = {}, {}
    with ThreadPoolExecutor(max_workers=4) as ex:
        for text, err in ex.map(_compile, FILES):
            name, body = None, []
            for line in text.splitlines():
                m = re.match(r"^(_Z\w+):", line)
                if m:
                    name, body = m.group(1), []
                elif name and line.startswith(".Lfunc_end"):
                    if _key(name):
                        assert _key(name) not in asm, name
                        asm[_key(name)] = body
                    name = None
                elif name:
                    body.append(line)
            cur = None
            for line in err.splitlines():
                m = re.search(r"remark:\s+(.*?)\s+\[-Rpass-analysis=kernel-resource-usage\]", line)
                if not m:
                    continue
                k, _, v = m.group(1).partition(": ")
                if k == "Function Name":
                    cur = _key(v)
                    if cur:
                        remarks[cur] = {}
                elif cur:
                    remarks[cur][k.strip()] = v.strip()
    return asm, remarks


def test_every_instantiation_fits_the_register_file(compiled):
    asm, remarks = compiled
    assert len(EXPECTED) == 28
    assert set(asm) == EXPECTED and set(remarks) == EXPECTED, (sorted(asm), sorted(remarks))
    for key in sorted(EXPECTED):
        r = remarks[key]
        print("%s<d=%d, NQT=%d, FILT=%s>:" % key, ", ".join("%s %s" % kv for kv in sorted(r.items())))
        assert int(r["ScratchSize [bytes/lane]"]) == 0, (key, r)
        assert int(r["VGPRs Spill"]) == 0, (key, r)
        assert int(r["SGPRs Spill"]) == 0, (key, r)
        assert int(r["Occupancy [waves/SIMD]"]) == 1, (key, r)
        assert not [l for l in asm[key] if re.match(r"^\s*scratch_(load|store)", l)], key


def test_the_ring_is_never_drained_inside_the_matrix_span(compiled):
    asm, _ = compiled
    for key in sorted(EXPECTED):
        _fam, d, nqt, _filt = key
        nkc, p = ring(key)
        lines = asm[key]
        at = [i for i, l in enumerate(lines) if MFMA.match(l)]
        waits = [int(m.group(1)) for m in (VMCNT.match(l) for l in lines[at[0]:at[-1] + 1]) if m] if at else []
        print("%s<d=%d, NQT=%d, FILT=%s>:" % key, "%d MFMAs, %d instructions, vmcnt waits between the first and the last MFMA: %s"
              % (len(at), sum(1 for l in lines if re.match(r"^\s+[a-z]\w+", l) and not l.lstrip().startswith(".")), waits))
        assert len(at) == nqt * (d // 16), (key, len(at))                # one unrolled tile: the span is the tile loop's
        assert waits == [4 * (p - 1)] * (nkc - 1), (key, waits)


# ---------------------------------------------------------------- the bf16 corpus scorer (cosine_bf16.hip) on the same ring
SOLO = re.compile(r"^_Z\d+cosine_bf16_filterILi(\d+)ELi(\d+)ELb([01])EE")
PAIR = re.compile(r"^_Z\d+cosine_bf16_pairILi(\d+)ELi(\d+)EE")
QSPLIT = re.compile(r"^_Z\d+cosine_bf16_qsplitILi(\d+)EE")
BF16_SOLO = {("solo", d, nqt, filt) for d, nqt in ((384, 1), (384, 2), (768, 1), (768, 2), (1024, 1)) for filt in (False, True)}
BF16_PAIR = {("pair", 384, 3, False), ("pair", 768, 3, False), ("pair", 1024, 2, False), ("pair", 1024, 3, False)}
BF16_QSPLIT = {("qsplit", 1024, 0, False), ("qsplit", 1024, 2, False)}
# The one known exception, with the parent commit's numbers (0d5fd47..f7194e8: 20 bytes of scratch, 4 spilled VGPRs, TWO
# vmcnt(0) between its first and last MFMA, one of them its wait ladder's end): 96 queries x 512 k are 384 registers of B
# operands beside 48 accumulators, hipcc keeps four of them in scratch and reloads them once per tile, and a scratch reload is
# a vector-memory operation the ring's counted waits cannot tell from a DMA piece.  It must not grow.
PAIR_1024_3 = ("pair", 1024, 3, False)
PAIR_1024_3_SCRATCH, PAIR_1024_3_VGPR_SPILL, PAIR_1024_3_DRAINS = 20, 4, 1


def _bf16_key(mangled):
    m = SOLO.match(mangled)
    if m:
        return ("solo", int(m.group(1)), int(m.group(2)), m.group(3) == "1")
    m = PAIR.match(mangled)
    if m:
        return ("pair", int(m.group(1)), int(m.group(2)), False)
    m = QSPLIT.match(mangled)
    return ("qsplit", 1024, int(m.group(1)), False) if m else None


def bf16_ring(key):
    """(K width of a wave, NKC, P) of a solo or pair instantiation: cb_solo_nbuf / cb_pair_nbuf of cosine_bf16.hip."""
    fam, d = key[0], key[1]
    kw = d if fam == "solo" else d // 2
    nkc = kw // 64
    nbuf = nkc if fam == "pair" else (8 if nkc % 8 == 0 else 6 if nkc % 6 == 0 else nkc)
    return kw, nkc, nbuf - 1


@pytest.fixture(scope="module")
def bf16_compiled():
    """({instantiation: assembly lines}, {instantiation: {remark name: value}}) of cosine_bf16.hip with the library's flags."""
    text, err = _compile("cosine_bf16.hip")
    asm, remarks, name, body, cur = {}, {}, None, [], None
    for line in text.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name, body = m.group(1), []
        elif name and line.startswith(".Lfunc_end"):
            if _bf16_key(name):
                asm[_bf16_key(name)] = body
            name = None
        elif name:
            body.append(line)
    for line in err.splitlines():
        m = re.search(r"remark:\s+(.*?)\s+\[-Rpass-analysis=kernel-resource-usage\]", line)
        if m:
            k, _, v = m.group(1).partition(": ")
            if k == "Function Name":
                cur = _bf16_key(v)
                if cur:
                    remarks[cur] = {}
            elif cur:
                remarks[cur][k.strip()] = v.strip()
    assert set(asm) == set(remarks) == BF16_SOLO | BF16_PAIR | BF16_QSPLIT, sorted(asm)
    return asm, remarks


def _assert_fits(keys, remarks, asm):
    for key in sorted(keys):
        r = remarks[key]
        print("%s<%d, %d, FILT=%s>:" % key, ", ".join("%s %s" % kv for kv in sorted(r.items())))
        scratch, vspill = (PAIR_1024_3_SCRATCH, PAIR_1024_3_VGPR_SPILL) if key == PAIR_1024_3 else (0, 0)
        assert int(r["ScratchSize [bytes/lane]"]) <= scratch, (key, r)
        assert int(r["VGPRs Spill"]) <= vspill, (key, r)
        assert int(r["SGPRs Spill"]) == 0, (key, r)
        assert int(r["Occupancy [waves/SIMD]"]) == 1, (key, r)
        if not scratch:
            assert not [l for l in asm[key] if re.match(r"^\s*scratch_(load|store)", l)], key


def test_bf16_solo_and_qsplit_fit_the_register_file(bf16_compiled):
    asm, remarks = bf16_compiled
    assert len(BF16_SOLO) == 10
    _assert_fits(BF16_SOLO | BF16_QSPLIT, remarks, asm)
    for key in BF16_QSPLIT:
        assert sum(1 for l in asm[key] if MFMA.match(l)) == 64, key


def test_bf16_pair_fits_the_register_file(bf16_compiled):
    """The pair kernel sits at the SGPR limit (104 of 104 at d = 1024): with its segment counters ahead of the thresholds in the
    argument list, as in the other two kernels, hipcc spilled 4 SGPRs to VGPR lanes in three of the four instantiations (the
    note above cosine_bf16_pair)."""
    asm, remarks = bf16_compiled
    _assert_fits(BF16_PAIR, remarks, asm)


def test_bf16_ring_is_never_drained_inside_the_matrix_span(bf16_compiled):
    asm, _ = bf16_compiled
    for key in sorted(BF16_SOLO | BF16_PAIR):
        kw, nkc, p = bf16_ring(key)
        lines = asm[key]
        at = [i for i, l in enumerate(lines) if MFMA.match(l)]
        waits = [int(m.group(1)) for m in (VMCNT.match(l) for l in lines[at[0]:at[-1] + 1]) if m]
        print("%s<%d, %d, FILT=%s>:" % key, "%d MFMAs, vmcnt waits between the first and the last MFMA: %s" % (len(at), waits))
        assert len(at) == key[2] * (kw // 16), (key, len(at))
        if key == PAIR_1024_3:   # (the scratch reload's vmcnt(0): see PAIR_1024_3)
            assert waits.count(0) <= PAIR_1024_3_DRAINS, (key, waits)
            waits = [x for x in waits if x]
        assert waits == [4 * (p - 1)] * (nkc - 1), (key, waits)


def test_expected_waits_are_the_documented_ones():
    """vmcnt(24) x 5 / x 11 for the two copy-ring kernels at d = 384 / 768, vmcnt(16) x 11 and vmcnt(24) x 23 for the f32 screen."""
    got = {(k[0] == "f32", k[1]): (4 * (ring(k)[1] - 1), ring(k)[0] - 1) for k in EXPECTED}
    assert got == {(False, 384): (24, 5), (False, 768): (24, 11), (True, 384): (16, 11), (True, 768): (24, 23)}
