"""The compiled resources of the two f32 cosine kernels written on csrc/oi_ksplit_tile.h, read off hipcc's kernel-resource-usage
remarks and the gfx950 assembly.

cosine_ksplit16_filter<D, NQT, FILT> (cosine_ksplit.hip, 12 product instantiations) and cosine_split_filter<D, NQT> (cosine_split.hip,
4) keep a wave's K-slice of the whole query block in registers and sit close to the 512-register file.  For each of the 16:

  * scratch 0 bytes;
  * VGPR spill no more than before the two kernels shared their ring and epilogue: 0, and 1 for cosine_ksplit16_filter<1024, 2, false>;
  * the MFMA count is a positive multiple of one tile's, 2 NKC groups of 16 k with NKC = D / 128 ring slots per tile and wave:
      K-split  2 NKC x 4 k-steps x 2 NQT query tiles of 16 x 2 row tiles of 16   (v_mfma_f32_16x16x4_f32),
      split    2 NKC x 6 NQT                                                      (v_mfma_f32_32x32x16_bf16)
    (the compiler keeps one or two copies of the tile, depending on how it peels the first iteration);
  * no fewer LDS-DMA loads (buffer_load_dwordx4 ... lds) than before: the prologue's 4 P pieces and 4 per ring slot of every copy of
    the tile, P = NBUF - 1 slots ahead.

A guard on what the compiler allocated and kept; not a speed claim."""
import os
import re
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor

import pytest

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")

FILES = ("cosine_ksplit.hip", "cosine_split.hip")
KSPLIT = re.compile(r"^_Z\d+cosine_ksplit16_filterILi(\d+)ELi(\d+)ELb([01])EE")
SPLIT = re.compile(r"^_Z\d+cosine_split_filterILi(\d+)ELi(\d+)ELi0EE")
MFMA = {"ksplit": re.compile(r"^\s*v_mfma_f32_16x16x4_f32\b"), "split": re.compile(r"^\s*v_mfma_f32_32x32x16_bf16\b")}
DMA = re.compile(r"^\s*buffer_load_dwordx4\b.*\blds\b")

EXPECTED = ({("ksplit", d, nqt, filt) for d in (384, 768, 1024) for nqt in (1, 2) for filt in (False, True)}
            | {("split", d, nqt, False) for d in (384, 768) for nqt in (1, 2)})

# LDS-DMA loads of each instantiation before the shared header: 4 P + 4 NKC per copy of the tile.  Two copies everywhere but in
# three: both split instantiations at d = 768 (so ("split", 768) is a ONE-copy figure, 20 + 24) and K-split <1024, 2, true>
DMA_BEFORE = {("ksplit", 384): 32, ("ksplit", 768): 68, ("ksplit", 1024): 76, ("split", 384): 32, ("split", 768): 44}
DMA_BEFORE_ONE_COPY = {("ksplit", 1024, 2, True): 44}
SPILL_BEFORE = {("ksplit", 1024, 2, False): 1}


def _key(mangled):
    m = KSPLIT.match(mangled)
    if m:
        return ("ksplit", int(m.group(1)), int(m.group(2)), m.group(3) == "1")
    m = SPLIT.match(mangled)
    return ("split", int(m.group(1)), int(m.group(2)), False) if m else None


def tile_mfmas(key):
    """MFMAs of one 32-row tile in one wave."""
    fam, d, nqt, _filt = key
    nkc = d // 128
    return 2 * nkc * 4 * 2 * nqt * 2 if fam == "ksplit" else 2 * nkc * 6 * nqt


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
    """({instantiation: assembly lines}, {instantiation: {remark name: value}}) of the two files with the library's flags."""
    asm, remarks = {}, {}
    with ThreadPoolExecutor(max_workers=2) as ex:
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


def test_every_instantiation_keeps_its_query_block_in_registers(compiled):
    asm, remarks = compiled
    assert len(EXPECTED) == 16
    assert set(asm) == EXPECTED and set(remarks) == EXPECTED, (sorted(asm), sorted(remarks))
    for key in sorted(EXPECTED):
        r = remarks[key]
        print("%s<d=%d, NQT=%d, FILT=%s>:" % key, ", ".join("%s %s" % kv for kv in sorted(r.items())))
        assert int(r["ScratchSize [bytes/lane]"]) == 0, (key, r)
        assert int(r["VGPRs Spill"]) <= SPILL_BEFORE.get(key, 0), (key, r)
        assert not [l for l in asm[key] if re.match(r"^\s*scratch_(load|store)", l)], key


def test_whole_tiles_of_matrix_instructions_and_every_dma_piece(compiled):
    asm, _ = compiled
    for key in sorted(EXPECTED):
        lines = asm[key]
        mfmas = sum(1 for l in lines if MFMA[key[0]].match(l))
        dmas = sum(1 for l in lines if DMA.match(l))
        print("%s<d=%d, NQT=%d, FILT=%s>:" % key, "%d MFMAs (%d per tile), %d LDS-DMA loads" % (mfmas, tile_mfmas(key), dmas))
        assert mfmas > 0 and mfmas % tile_mfmas(key) == 0, (key, mfmas, tile_mfmas(key))
        assert dmas >= DMA_BEFORE_ONE_COPY.get(key, DMA_BEFORE[key[:2]]), (key, dmas)


def test_tile_counts_are_the_documented_ones():
    """384 MFMAs per tile for the K-split kernel at d = 768 with 64 queries (its header's figure), 144 for the split kernel."""
    assert tile_mfmas(("ksplit", 768, 2, False)) == 384 and tile_mfmas(("split", 768, 2, False)) == 144
