"""The compiled resources of the mention kernels (csrc/mention.hip), read off hipcc's kernel-resource-usage remarks for gfx950.

mn_match_kernel keeps a task's 32768 match counts as byte counters in 32 KB of LDS and must leave room for a second workgroup on a
CU; nothing of it, in any of its four instantiations (key axis x filter), may live in scratch.

  * every kernel of the file: scratch 0 bytes, VGPR spill 0, SGPR spill 0;
  * every mn_match_kernel instantiation: LDS (static, it asks for no dynamic LDS) <= 64 KB;
  * the file uses no inline assembly.

Only the remarks are read: a guard on what the compiler allocated, not a speed claim."""
import os
import re
import subprocess
import tempfile

import pytest

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")

KERNEL = re.compile(r"^_Z\d+(mn_plan_kernel|mn_match_kernel|mn_finish_kernel)(.*)$")


@pytest.fixture(scope="module")
def remarks():
    """{mangled kernel name: {remark name: value}} of mention.hip compiled with the library's flags."""
    from openintel_amd import build as b
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([b.HIPCC, *b.FLAGS, "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage",
                            os.path.join(b.CSRC, "mention.hip"), "-o", os.path.join(tmp, "mention.s")], capture_output=True, text=True, cwd=tmp)
    assert r.returncode == 0, r.stderr[-4000:]
    out, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(.*?)\s+\[-Rpass-analysis=kernel-resource-usage\]", line)
        if not m:
            continue
        k, _, v = m.group(1).partition(": ")
        if k == "Function Name":
            cur = v if KERNEL.match(v) else None
            if cur:
                assert cur not in out, v
                out[cur] = {}
        elif cur:
            out[cur][k.strip()] = v.strip()
    for name, r_ in sorted(out.items()):
        print(name + ":", ", ".join("%s %s" % kv for kv in sorted(r_.items())))
    return out


def test_the_file_holds_the_three_kernels_and_all_four_match_instantiations(remarks):
    kinds = sorted(KERNEL.match(n).group(1) for n in remarks)
    assert kinds == ["mn_finish_kernel"] + ["mn_match_kernel"] * 4 + ["mn_plan_kernel"], sorted(remarks)
    assert {KERNEL.match(n).group(2)[:10] for n in remarks if "mn_match" in n} == {"ILb0ELb0EE", "ILb0ELb1EE", "ILb1ELb0EE", "ILb1ELb1EE"}


def test_no_kernel_uses_scratch_or_spills(remarks):
    for name, r in remarks.items():
        assert int(r["ScratchSize [bytes/lane]"]) == 0, (name, r)
        assert int(r["VGPRs Spill"]) == 0, (name, r)
        assert int(r["SGPRs Spill"]) == 0, (name, r)


def test_two_match_workgroups_fit_a_cu(remarks):
    from openintel_amd import build as b
    src = open(os.path.join(b.CSRC, "mention.hip")).read()
    assert "extern __shared__" not in src                       # no dynamic LDS: the static figure is the whole of it
    for name, r in remarks.items():
        if "mn_match_kernel" in name:
            assert 32768 <= int(r["LDS Size [bytes/block]"]) <= 64 * 1024, (name, r)


def test_the_file_has_no_inline_assembly():
    from openintel_amd import build as b
    src = open(os.path.join(b.CSRC, "mention.hip")).read()
    assert not re.search(r"\basm\b|__asm", src)
