#!/usr/bin/env python3
"""Is the gfx950 assembly of every kernel what it was at REV (default HEAD~1)?

    python tools/asm_identity.py [REV] [-k SUBSTRING] [-j JOBS]

The gate of a refactor that must not move device code: every csrc/*.hip of REV (from `git archive`, in a temporary
directory) and of the working tree is compiled with the library's own flags plus --cuda-device-only -S, for the product
build and for the variant builds the tools use, and the two .s files are compared after dropping the lines that name
__hip_cuid_<hash> (a per-translation-unit hash).  One line per (file, variant); exit status 1 on any difference.
-k: only the (file, variant) lines containing SUBSTRING.
"""
import argparse
import io
import os
import subprocess
import sys
import tarfile
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openintel_amd import build as oib  # noqa: E402

DMA_FILES = ["cosine_prefilter", "cosine_screen_copy", "cosine_screen_i8", "cosine_split", "cosine_bf16", "cosine_ksplit"]
ABL = "-DOI_ABLATION"


def variants(names):
    out = [(n, []) for n in names] + [(n, [ABL]) for n in names]
    out += [(n, ["-DOI_NO_NT"]) for n in DMA_FILES if n in names]
    out += [("cosine_screen_copy", [ABL, d]) for d in ("-DSC_AGG_NO_DMA=1", "-DSC_AGG_NO_DMA", "-DSC_AGG_NO_MFMA")]
    out += [("cosine_screen_i8", [ABL, d]) for d in ("-DI8S_NO_DMA", "-DI8S_NO_MFMA")]
    return [(n, d) for n, d in out if n in names]


def asm(tree, name, defs, out_dir):
    """The device assembly of tree/openintel_amd/csrc/name.hip without the cuid lines, or the compiler's complaint."""
    csrc = os.path.join(tree, "openintel_amd", "csrc")
    flags = [f for f in oib.FLAGS if not f.startswith("-I")] + ["-I" + os.path.join(tree, "include"), "-I" + csrc]
    out = os.path.join(out_dir, name + "".join(defs).replace("=", "_") + ".s")
    r = subprocess.run([oib.HIPCC, *flags, *defs, "--cuda-device-only", "-S", os.path.join(csrc, name + ".hip"), "-o", out],
                       capture_output=True, text=True)
    if r.returncode != 0:
        return None, r.stderr[-2000:]
    with open(out) as f:
        return [l for l in f if "__hip_cuid_" not in l], ""


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("rev", nargs="?", default="HEAD~1")
    ap.add_argument("-k", default="")
    ap.add_argument("-j", type=int, default=min(16, os.cpu_count() or 4))
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        old = os.path.join(tmp, "old")
        tar = subprocess.run(["git", "-C", ROOT, "archive", a.rev, "openintel_amd/csrc", "include"], check=True, capture_output=True)
        tarfile.open(fileobj=io.BytesIO(tar.stdout)).extractall(old)
        names = [s[:-4] for s in oib.sources() if os.path.exists(os.path.join(old, "openintel_amd", "csrc", s))]
        jobs = [(n, d) for n, d in variants(names) if a.k in n + " " + " ".join(d)]
        for side in ("old_s", "new_s"):
            os.makedirs(os.path.join(tmp, side))

        def one(job):
            (o, eo), (n, en) = asm(old, *job, os.path.join(tmp, "old_s")), asm(ROOT, *job, os.path.join(tmp, "new_s"))
            if o is None or n is None:
                return job, -1, len(o or n or []), eo or en
            return job, len(o) - sum(x == y for x, y in zip(o, n)) + max(0, len(n) - len(o)), len(n), ""

        bad = 0
        with ThreadPoolExecutor(max_workers=max(1, a.j)) as ex:
            for (name, defs), diff, lines, err in ex.map(one, jobs):
                verdict = "identical" if diff == 0 else ("DOES NOT COMPILE\n" + err if diff < 0 else "DIFFERS in %d lines" % diff)
                print("%-22s %-34s %7d lines  %s" % (name + ".hip", " ".join(defs) or "(product)", lines, verdict), flush=True)
                bad += diff != 0
        print("%d of %d differ from %s" % (bad, len(jobs), a.rev))
        return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
