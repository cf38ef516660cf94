"""The compiled schedule of cosine_i8_screen's tile loop (csrc/cosine_screen_i8.hip), read off the gfx950 assembly.

The kernel runs one wave per SIMD, so an LDS round trip that a wave waits for in full is time nothing else fills.  Its tile loop
therefore reads the row fragment and the queries' lo fragments a k-step ahead of the MFMAs that use them, into registers no MFMA
in flight reads, and retires them with counted s_waitcnt lgkmcnt(N), N > 0.  Nothing in the source language guarantees that order:
the compiler is free to sink the reads back next to their use on a later edit (it did, before the schedule was pinned).  This
module compiles the file the way openintel_amd/build.py does and checks, for every instantiation the launcher can pick:

  * no scratch and no VGPR spill (the query block, two fragment sets and the accumulators fit the register file);
  * d = 768: no `s_waitcnt lgkmcnt(0)` between the first and the last v_mfma_i32_32x32x32_i8 of the kernel (the whole tile
    loop's matrix span; before the schedule was pinned: 47 with two query tiles, 21 with one);
  * d = 384: the count is printed, without a limit.

A guard against the schedule being undone quietly; not a speed claim."""
import os
import re
import subprocess
import tempfile

import pytest

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")

INST = re.compile(r"cosine_i8_screenILi(\d+)ELi(\d+)ELi(\d+)ELb([01])EE")
MFMA = re.compile(r"^\s*v_mfma_i32_32x32x32_i8\b")
LGKM0 = re.compile(r"^\s*s_waitcnt\b.*\blgkmcnt\(0\)")
EXPECTED = {(d, nqt, filt) for d in (384, 768) for nqt in (1, 2) for filt in (False, True)}


def _key(mangled):
    m = INST.search(mangled)
    return (int(m.group(1)), int(m.group(2)), m.group(4) == "1") if m else None


@pytest.fixture(scope="module")
def compiled():
    """({instantiation: assembly lines}, {instantiation: {remark name: value}}) of cosine_screen_i8.hip with the library's flags."""
    from openintel_amd import build as b
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        r = subprocess.run([b.HIPCC, *b.FLAGS, "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage",
                            os.path.join(b.CSRC, "cosine_screen_i8.hip"), "-o", out], capture_output=True, text=True, cwd=tmp)
        assert r.returncode == 0, r.stderr[-4000:]
        with open(out) as f:
            text = f.read()
    asm, name, body = {}, None, []
    for line in text.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name, body = m.group(1), []
        elif name and line.startswith(".Lfunc_end"):
            if _key(name):
                asm[_key(name)] = body
            name = None
        elif name:
            body.append(line)
    remarks, cur = {}, None
    for line in r.stderr.splitlines():
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


def _lgkm0_in_mfma_span(lines):
    at = [i for i, l in enumerate(lines) if MFMA.match(l)]
    assert at, "no v_mfma_i32_32x32x32_i8 in the kernel"
    return sum(1 for l in lines[at[0]:at[-1] + 1] if LGKM0.match(l)), len(at)


def test_every_instantiation_fits_the_register_file(compiled):
    asm, remarks = compiled
    assert set(asm) == EXPECTED and set(remarks) == EXPECTED, (sorted(asm), sorted(remarks))
    for key in sorted(EXPECTED):
        r = remarks[key]
        print("cosine_i8_screen<d=%d, NQT=%d, FILT=%s>:" % key, ", ".join("%s %s" % kv for kv in sorted(r.items())))
        assert int(r["ScratchSize [bytes/lane]"]) == 0, (key, r)
        assert int(r["VGPRs Spill"]) == 0, (key, r)
        assert int(r["Occupancy [waves/SIMD]"]) == 1, (key, r)
        assert not [l for l in asm[key] if re.match(r"^\s*scratch_(load|store)", l)], key


def test_no_full_lds_wait_inside_the_matrix_span(compiled):
    asm, _ = compiled
    counts = {}
    for key in sorted(EXPECTED):
        n0, n_mfma = _lgkm0_in_mfma_span(asm[key])
        counts[key] = n0
        d, nqt, _f = key
        print("cosine_i8_screen<d=%d, NQT=%d, FILT=%s>: %d s_waitcnt lgkmcnt(0) between the first and the last of %d MFMAs"
              % (key + (n0, n_mfma)))
        assert n_mfma == 2 * nqt * (d // 32), (key, n_mfma)   # one unrolled tile: the span is the tile loop's
    bad = {k: v for k, v in counts.items() if k[0] == 768 and v != 0}
    assert not bad, bad

