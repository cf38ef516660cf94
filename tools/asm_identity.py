#!/usr/bin/env python3
"""Is the gfx950 assembly of every kernel what it was at REV (default HEAD~1)?

    python tools/asm_identity.py [REV] [-k SUBSTRING] [-j JOBS] [--per-kernel [--json FILE] [--rename 'OLD=NEW' ...]]

The gate of a refactor that must not move device code: every csrc/*.hip of REV (from `git archive`, in a temporary
directory) and of the working tree is compiled with the library's own flags plus --cuda-device-only -S, for the product
build and for the variant builds the tools use, and the two .s files are compared after dropping the lines that name
__hip_cuid_<hash> (a per-translation-unit hash).  One line per (file, variant); exit status 1 on any difference.
-k: only the (file, variant) lines containing SUBSTRING.

--per-kernel: the gate of a change that removes or adds kernels.  Each .s is cut at its function symbols (the compiler's
"Begin function" marks: kernels with their descriptors, and the device functions that were not inlined), comments are
dropped and so is the function's index in local labels (.LBB7_24 -> .LBB_24, .Ltmp, .Lfunc_*), which moves when a
neighbour goes.  Functions in both trees are compared, with the differing lines printed; those only in REV are listed as
removed, those only in the working tree as added.  Exit status 1 if a function in both trees differs.  --json: the table.

--rename 'OLD=NEW' (repeatable): a function of REV whose demangled name (c++filt -p: no parameter list) matches the regular
expression OLD in full is compared with the working tree's function whose demangled name is NEW (\\1.. are OLD's groups), e.g.
--rename 'cosine_volume_screen<(.*)>=vo_stream_kernel<\\1, VoCount>'.  The pair is one row, "REV name -> tree name", identical
or DIFFERS like any other.  Within a compared body the function's own symbol is a placeholder on both sides, so the kernel
descriptor and its .set lines compare.
"""
import argparse
import difflib
import io
import json
import os
import re
import shutil
import subprocess
import sys
import tarfile
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from openintel_amd import build as oib  # noqa: E402

DMA_FILES = ["cosine_prefilter", "cosine_screen_copy", "cosine_screen_i8", "cosine_split", "cosine_bf16", "cosine_ksplit",
             "cosine_volume", "cosine_summary", "cosine_groups", "cosine_share"]
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


BEGIN = re.compile(r"-- Begin function (\S+)")
LABEL = re.compile(r"\.L(BB|JTI|CPI|tmp|func_begin|func_end)\d+")


def functions(lines):
    """{symbol: normalised lines} of one .s: from a function's Begin mark to the next one's (or the end of the code)."""
    out, cur = {}, None
    for l in lines:
        m = BEGIN.search(l)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif l.lstrip().startswith((".p2alignl", ".amdgpu_metadata")) or ".AMDGPU.gpr_maximums" in l:
            cur = None
        l = LABEL.sub(r".L\1", l.split(";")[0]).strip()
        if cur is not None and l and not l.startswith((".section", ".text")):  # (a section line names the NEXT function)
            cur.append(l)
    return out


def demangled(symbols):
    """{symbol: its demangled name without the parameter list}"""
    tool = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    if not tool:
        sys.exit("--rename matches demangled names and needs c++filt (or llvm-cxxfilt) on the PATH: none found")
    symbols = sorted(symbols)
    out = subprocess.run([tool, "-p"], input="\n".join(symbols), check=True, capture_output=True, text=True).stdout.splitlines()
    return dict(zip(symbols, out))


def renamed(fo, fn, renames):
    """{REV symbol: tree symbol} of the functions a --rename pairs (both must exist, the tree's not in REV under its own name)"""
    if not renames or not fo or not fn:
        return {}
    names = demangled(set(fo) | set(fn))
    by_name = {names[s]: s for s in fn if s not in fo}
    pairs = {}
    for so in fo:
        for pat, new in renames:
            m = re.fullmatch(pat, names[so])
            if m and so not in fn and m.expand(new) in by_name:
                pairs[so] = by_name[m.expand(new)]
                break
    return pairs


def per_kernel(job, old, new, renames=()):
    """Rows (file, variant, function, verdict, differing lines) of one (file, variant)."""
    fo, fn = functions(old), functions(new)
    pairs = renamed(fo, fn, renames)
    rows = []
    for sym in sorted((set(fo) | set(fn)) - set(pairs.values())):
        to = pairs.get(sym, sym)
        if to not in fn or sym not in fo:
            rows.append((sym, "removed" if sym in fo else "added", []))
            continue
        a, b = ([l.replace(s, "<self>") for l in f] for s, f in ((sym, fo[sym]), (to, fn[to])))
        d = [l for l in difflib.unified_diff(a, b, "REV", "tree", n=0, lineterm="") if l[:2] not in ("--", "++", "@@")]
        rows.append((sym if to == sym else sym + " -> " + to, "DIFFERS in %d lines" % len(d) if d else "identical (%d lines)" % len(b), d))
    return [(job[0] + ".hip", " ".join(job[1]) or "(product)", *r) for r in rows]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("rev", nargs="?", default="HEAD~1")
    ap.add_argument("-k", default="")
    ap.add_argument("-j", type=int, default=min(16, os.cpu_count() or 4))
    ap.add_argument("--per-kernel", action="store_true")
    ap.add_argument("--json", default="")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW")
    a = ap.parse_args()
    renames = [tuple(r.split("=", 1)) for r in a.rename]
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
            if a.per_kernel:
                return job, 0, len(n), per_kernel(job, o, n, renames)
            return job, len(o) - sum(x == y for x, y in zip(o, n)) + max(0, len(n) - len(o)), len(n), ""

        bad, table = 0, []
        with ThreadPoolExecutor(max_workers=max(1, a.j)) as ex:
            for (name, defs), diff, lines, err in ex.map(one, jobs):
                if a.per_kernel and diff == 0:
                    for f, v, fun, verdict, d in err:
                        print("%-22s %-34s %-22s %s" % (f, v, verdict, fun), flush=True)
                        for l in d[:40]:
                            print("        " + l)
                        bad += verdict.startswith("DIFFERS")
                        table.append({"file": f, "variant": v, "function": fun, "verdict": verdict, "diff": d})
                    continue
                verdict = "identical" if diff == 0 else ("DOES NOT COMPILE\n" + err if diff < 0 else "DIFFERS in %d lines" % diff)
                print("%-22s %-34s %7d lines  %s" % (name + ".hip", " ".join(defs) or "(product)", lines, verdict), flush=True)
                bad += diff != 0
        if a.json:
            with open(a.json, "w") as f:
                json.dump(table, f, indent=1)
        print("%d of %d differ from %s" % (bad, len(table) if a.per_kernel else len(jobs), a.rev))
        return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
