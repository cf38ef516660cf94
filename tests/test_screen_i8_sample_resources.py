"""The compiled resources of the int8 route's sample pass, read off hipcc's kernel-resource-usage remarks for gfx950.

i8s_sample_kernel (csrc/cosine_screen_i8.hip) holds a tile's row fragments and the hi query fragments over the whole K in
registers beside two accumulator sets, one wave per SIMD; sample_rank_kernel (csrc/sample_rank.hip) holds up to 32 keys per
thread of its 1024-thread workgroup.  Neither may touch scratch:

  * every i8s_sample_kernel<D, NQT> (D 384 / 768, NQT 1 / 2): scratch 0 bytes, VGPR spill 0, one wave per SIMD;
  * sample_rank_kernel: scratch 0 bytes, VGPR spill 0, VGPRs <= 128 (four waves per SIMD).

Only the remarks are read: a guard on what the compiler allocated, not a speed claim."""
import os
import re
import subprocess
import tempfile

import pytest

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")


def _remarks(source, kernel_re):
    """{mangled kernel name: {remark name: value}} of csrc/<source> compiled with the library's flags."""
    from openintel_amd import build as b
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([b.HIPCC, *b.FLAGS, "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage",
                            os.path.join(b.CSRC, source), "-o", os.path.join(tmp, "out.s")], capture_output=True, text=True, cwd=tmp)
    assert r.returncode == 0, r.stderr[-4000:]
    out, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(.*?)\s+\[-Rpass-analysis=kernel-resource-usage\]", line)
        if not m:
            continue
        k, _, v = m.group(1).partition(": ")
        if k == "Function Name":
            cur = v if kernel_re.match(v) else None
            if cur:
                assert cur not in out, v
                out[cur] = {}
        elif cur:
            out[cur][k.strip()] = v.strip()
    for name, r_ in sorted(out.items()):
        print(name + ":", ", ".join("%s %s" % kv for kv in sorted(r_.items())))
    return out


def test_the_sample_kernel_keeps_its_fragments_in_registers():
    out = _remarks("cosine_screen_i8.hip", re.compile(r"^_Z\d+i8s_sample_kernelILi(384|768)ELi(1|2)E"))
    assert len(out) == 4, sorted(out)
    for name, r in out.items():
        assert int(r["ScratchSize [bytes/lane]"]) == 0, (name, r)
        assert int(r["VGPRs Spill"]) == 0, (name, r)
        assert int(r["SGPRs Spill"]) == 0, (name, r)
        assert int(r["Occupancy [waves/SIMD]"]) == 1, (name, r)  # (the whole-SIMD claim: v255 and a255 are touched)


def test_the_rank_kernel_keeps_its_keys_in_registers():
    out = _remarks("sample_rank.hip", re.compile(r"^_Z\d+sample_rank_kernel"))
    assert len(out) == 1, sorted(out)
    (r,) = out.values()
    assert int(r["ScratchSize [bytes/lane]"]) == 0, r
    assert int(r["VGPRs Spill"]) == 0, r
    assert int(r["VGPRs"]) <= 128, r
