"""The compiled resources of the two select kernels (csrc/select.hip), read off hipcc's kernel-resource-usage remarks for gfx950.

select_flat_kernel keeps up to 32 keys per thread in registers and sits at the 128-VGPR line of its 1024-thread workgroup.  Its
margin state (SelMargin, with the per-row record by value) has to stay in registers too: when the record's address went through a
conditional it lived in 32 bytes of scratch, with a dependent reload in front of every per-row gather.  select_topk_kernel borrows
sel_threshold and sel_finish from the flat kernel and must not take more LDS for it than it had with its own copies.

  * select_flat_kernel: scratch 0 bytes, VGPR spill 0, VGPRs <= 128, LDS <= 74 864 bytes;
  * select_topk_kernel: scratch 0 bytes, LDS <= 82 976 bytes.

Only the remarks are read: a guard on what the compiler allocated, not a speed claim."""
import os
import re
import subprocess
import tempfile

import pytest

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")

KERNEL = re.compile(r"^_Z\d+(select_flat_kernel|select_topk_kernel)\d")


@pytest.fixture(scope="module")
def remarks():
    """{kernel: {remark name: value}} of select.hip compiled with the library's flags."""
    from openintel_amd import build as b
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([b.HIPCC, *b.FLAGS, "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage",
                            os.path.join(b.CSRC, "select.hip"), "-o", os.path.join(tmp, "select.s")], capture_output=True, text=True, cwd=tmp)
    assert r.returncode == 0, r.stderr[-4000:]
    out, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(.*?)\s+\[-Rpass-analysis=kernel-resource-usage\]", line)
        if not m:
            continue
        k, _, v = m.group(1).partition(": ")
        if k == "Function Name":
            km = KERNEL.match(v)
            cur = km.group(1) if km else None
            if cur:
                assert cur not in out, v
                out[cur] = {}
        elif cur:
            out[cur][k.strip()] = v.strip()
    assert set(out) == {"select_flat_kernel", "select_topk_kernel"}, sorted(out)
    for name, r_ in sorted(out.items()):
        print(name + ":", ", ".join("%s %s" % kv for kv in sorted(r_.items())))
    return out


def test_the_flat_select_keeps_its_state_in_registers(remarks):
    r = remarks["select_flat_kernel"]
    assert int(r["ScratchSize [bytes/lane]"]) == 0, r
    assert int(r["VGPRs Spill"]) == 0, r
    assert int(r["VGPRs"]) <= 128, r
    assert int(r["LDS Size [bytes/block]"]) <= 74864, r


def test_the_segment_walking_select_fits_its_lds(remarks):
    r = remarks["select_topk_kernel"]
    assert int(r["ScratchSize [bytes/lane]"]) == 0, r
    assert int(r["LDS Size [bytes/block]"]) <= 82976, r
