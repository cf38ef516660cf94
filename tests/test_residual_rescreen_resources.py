"""The compiled resources of the residual plane's two kernels (csrc/screen_i8_residual.hip), read off hipcc's
kernel-resource-usage remarks and the assembly for gfx950.

  * i8r_make_kernel holds a row's twelve residuals per lane in f64 between its two passes; i8r_rescreen_kernel holds the query's
    h and l fragments and four survivors' rows per wave.  Neither may touch scratch or spill;
  * the rescreen runs beside the BM25 leg and behind MFMA kernels of other streams: its f32 steps are single v_fma_f32 /
    v_mul_f32 / v_add_f32, never a packed-f32 form -- no v_pk_*_f32 in either kernel's assembly.

Only the compiler's output is read: a guard on what it made of the source, not a speed claim."""
import os
import re
import subprocess
import tempfile

import pytest

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")

KERNELS = re.compile(r"^_Z\d+(i8r_make_kernel|i8r_rescreen_kernel)")


@pytest.fixture(scope="module")
def compiled():
    """(remarks {mangled kernel: {name: value}}, assembly {mangled kernel: [instruction lines]}) of one compilation."""
    from openintel_amd import build as b
    with tempfile.TemporaryDirectory() as tmp:
        out_s = os.path.join(tmp, "out.s")
        r = subprocess.run([b.HIPCC, *b.FLAGS, "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage",
                            os.path.join(b.CSRC, "screen_i8_residual.hip"), "-o", out_s], capture_output=True, text=True, cwd=tmp)
        assert r.returncode == 0, r.stderr[-4000:]
        asm_lines = open(out_s).read().splitlines()
    remarks, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(.*?)\s+\[-Rpass-analysis=kernel-resource-usage\]", line)
        if not m:
            continue
        k, _, v = m.group(1).partition(": ")
        if k == "Function Name":
            cur = v if KERNELS.match(v) else None
            if cur:
                remarks[cur] = {}
        elif cur:
            remarks[cur][k.strip()] = v.strip()
    asm, cur = {}, None
    for line in asm_lines:
        m = re.search(r"-- Begin function (\S+)", line)
        if m:
            cur = asm.setdefault(m.group(1), []) if KERNELS.match(m.group(1)) else None
        elif "-- End function" in line:
            cur = None
        elif cur is not None:
            code = line.split(";")[0].strip()
            if code and not code.startswith("."):
                cur.append(code)
    for name, r_ in sorted(remarks.items()):
        print(name + ":", ", ".join("%s %s" % kv for kv in sorted(r_.items())), "| %d instructions" % len(asm.get(name, [])))
    return remarks, asm


def test_neither_kernel_touches_scratch(compiled):
    remarks, _ = compiled
    assert len(remarks) == 2, sorted(remarks)
    for name, r in remarks.items():
        assert int(r["ScratchSize [bytes/lane]"]) == 0, (name, r)
        assert int(r["VGPRs Spill"]) == 0, (name, r)
        assert int(r["SGPRs Spill"]) == 0, (name, r)


def test_no_packed_f32_forms(compiled):
    _, asm = compiled
    assert len(asm) == 2, sorted(asm)
    for name, code in asm.items():
        assert len(code) > 50, (name, len(code))
        packed = [l for l in code if re.match(r"v_pk_\w*_f32\b", l)]
        assert not packed, (name, packed[:4])
