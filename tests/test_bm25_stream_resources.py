"""The compiled resources of the two product instantiations of bm25_stream_kernel (csrc/bm25_stream.hip), read off hipcc's
kernel-resource-usage remarks and off the assembly for gfx950.

The kernel keeps BS_RING LDS-DMA chunks in flight that hipcc does not see.  Two things the compiler can do to it silently:

  * keep a stage's state in scratch memory (the refill of the ring is a macro because icur / inxt captured by reference once
    lived there, with a reload in front of every visit);
  * wait for one of ITS OWN loads with `s_waitcnt vmcnt(0)` inside the stream loop, which drains the whole ring (the register pin
    of d_idf / d_cb in bs_load_runs, the queue draw whose result is used at once).  Statically that shows as one more full wait
    inside the kernel's function.

For bm25_stream_kernel<32768, false, false> (a plain search) and <32768, false, true> (a filtered one):

  * scratch 0 bytes per lane, VGPR spill 0;
  * `s_waitcnt vmcnt(0)` instructions in the function: at most 44 (unfiltered) and 51 (filtered), what the single-body kernel
    this file was split from had.

A guard on what the compiler emitted, not a speed claim."""
import os
import re
import subprocess
import tempfile

import pytest

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")

KERNELS = {"_Z18bm25_stream_kernelILi32768ELb0ELb0EEv6BsArgs": "unfiltered", "_Z18bm25_stream_kernelILi32768ELb0ELb1EEv6BsArgs": "filtered"}
FULL_WAITS = {"unfiltered": 44, "filtered": 51}


@pytest.fixture(scope="module")
def compiled():
    """{instantiation: ({remark name: value}, [instruction lines of the function])} of bm25_stream.hip with the library's flags."""
    from openintel_amd import build as b
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "bm25_stream.s")
        r = subprocess.run([b.HIPCC, *b.FLAGS, "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage",
                            os.path.join(b.CSRC, "bm25_stream.hip"), "-o", out], capture_output=True, text=True, cwd=tmp)
        assert r.returncode == 0, r.stderr[-4000:]
        with open(out) as f:
            asm = f.read().splitlines()
    remarks, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(.*?)\s+\[-Rpass-analysis=kernel-resource-usage\]", line)
        if not m:
            continue
        k, _, v = m.group(1).partition(": ")
        if k == "Function Name":
            cur = KERNELS.get(v.strip())
            if cur:
                assert cur not in remarks, v
                remarks[cur] = {}
        elif cur:
            remarks[cur][k.strip()] = v.strip()
    code, cur = {}, None
    for line in asm:
        m = re.search(r"-- Begin function (\S+)", line)
        if m:
            cur = code.setdefault(KERNELS[m.group(1)], []) if m.group(1) in KERNELS else None
            continue
        if "-- End function" in line or ".amdhsa_kernel" in line:
            cur = None
        text = line.split(";")[0].strip()
        if cur is not None and text and not text.startswith(".") and not text.endswith(":"):
            cur.append(text)
    assert set(remarks) == set(code) == set(KERNELS.values()), (sorted(remarks), sorted(code))
    for name in sorted(remarks):
        print(name + ":", len(code[name]), "instructions,", full_waits(code[name]), "full waits,",
              ", ".join("%s %s" % kv for kv in sorted(remarks[name].items())))
    return {name: (remarks[name], code[name]) for name in remarks}


def full_waits(code):
    return sum(1 for i in code if re.match(r"s_waitcnt\b.*\bvmcnt\(0\)", i))  # (alone or with other counters)


@pytest.mark.parametrize("name", sorted(FULL_WAITS))
def test_the_stream_kernel_keeps_its_state_in_registers(compiled, name):
    r, _ = compiled[name]
    assert int(r["ScratchSize [bytes/lane]"]) == 0, r
    assert int(r["VGPRs Spill"]) == 0, r


@pytest.mark.parametrize("name", sorted(FULL_WAITS))
def test_no_full_wait_was_added_inside_the_stream_kernel(compiled, name):
    _, code = compiled[name]
    assert len(code) > 3000, len(code)  # (the function was found and is the whole kernel)
    assert full_waits(code) <= FULL_WAITS[name], full_waits(code)
