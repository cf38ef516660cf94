#!/usr/bin/env python3
"""One steady-state hybrid step out of a rocprofv3 --kernel-trace CSV, launch by launch.

    python tools/trace_one_step.py TRACE_DIR [--json OUT.json]

Prints every launch of the middle step in start order: start (us from the step's first launch), duration, queue, kernel, grid.
A step begins at the query staging launch (pf_stage_queries_kernel; on the int8 route of later builds i8s_stage_both_kernel).
Each select_flat_kernel launch is named by what precedes it on its queue: the margin select of screen chunk i, the bf16 margin
select after the rescreen, the final sorted select after the rescoring, the gated selects behind the gated exact kernel, the BM25
leg's select.  The int8 route's sample pass (i8s_sample_kernel) and its rank launch (sample_rank_kernel) get roles of their own, and
the HEAD of a step is measured: from the end of the staging launch to the start of the first screen launch that runs under a
threshold -- screen chunk 2 behind a pooled first chunk, screen chunk 1 behind a sample pass.  --json also writes the table, the
per-role medians over all steps but the first three and the last, the median head, and the end of each leg before the fusion
(which leg ends last)."""
import csv
import glob
import json
import statistics
import sys

STAGE = ("pf_stage_queries_kernel", "i8s_stage_both_kernel")


def short(name):
    # "void name<...>(args)" -> name; a name that opens with "(anonymous namespace)::" (torch's own kernels) keeps its tail
    head = name.replace("(anonymous namespace)::", "").split("(")[0].split("<")[0].split("::")[-1].split()
    return head[-1][-40:] if head else name[-40:]


def load(d):
    f = glob.glob(d + "/*/*kernel_trace.csv") + glob.glob(d + "/**/*kernel_trace.csv", recursive=True)
    rows = sorted(csv.DictReader(open(f[0])), key=lambda r: int(r["Start_Timestamp"]))
    return [{"name": short(r["Kernel_Name"]), "full": r["Kernel_Name"].split("(")[0][-60:], "start": int(r["Start_Timestamp"]),
             "end": int(r["End_Timestamp"]), "queue": r["Queue_Id"], "grid": r["Grid_Size_X"]} for r in rows]


def steps_of(rows):
    idx = [i for i, r in enumerate(rows) if r["name"] in STAGE]
    return [rows[a:b] for a, b in zip(idx, idx[1:])]


def label(step):
    """role of every launch of one step (None = its own name)"""
    last = {}          # queue -> name of the launch before
    chunk = 0
    out = []
    for r in step:
        role = None
        if "screen" in r["name"] and ("i8_screen" in r["name"] or "screen_copy" in r["name"] or "screen_filter" in r["name"]):
            chunk += 1
            role = "screen chunk %d" % chunk
        elif r["name"] == "i8s_sample_kernel":
            role = "sample pass"
        elif r["name"] == "sample_rank_kernel":
            role = "sample rank"
        elif r["name"] == "select_flat_kernel":
            prev = last.get(r["queue"], "")
            if "screen" in prev and "rescreen" not in prev:
                role = "select: margin, chunk %d" % chunk
            elif "rescreen" in prev:
                role = "select: bf16 margin after the rescreen"
            elif "rescore" in prev:
                role = "select: final sorted"
            elif "ksplit" in prev or "cosine" in prev:
                role = "select: gated"
            elif "bm25" in prev:
                role = "select: BM25 leg"
            else:
                role = "select: after " + prev
        out.append(role)
        last[r["queue"]] = r["name"]
    return out


def table(step):
    t0 = step[0]["start"]
    return [{"start_us": round((r["start"] - t0) / 1e3, 1), "dur_us": round((r["end"] - r["start"]) / 1e3, 1), "queue": r["queue"],
             "kernel": r["name"], "role": role, "grid": r["grid"]} for r, role in zip(step, label(step))]


def head(step):
    """us from the end of the staging launch to the start of the first thresholded screen launch (None: fewer screen launches)"""
    roles = label(step)
    want = "screen chunk 1" if "sample pass" in roles else "screen chunk 2"
    at = [r for r, role in zip(step, roles) if role == want]
    return round((at[0]["start"] - step[0]["end"]) / 1e3, 1) if at else None


def legs(step):
    """end of the cosine leg (the last launch before rrf on rrf's queue) and of the BM25 leg (the last launch on another queue)"""
    t0 = step[0]["start"]
    rrf = [r for r in step if r["name"] == "rrf_kernel"]
    if not rrf:
        return None
    main = rrf[0]["queue"]
    cos = [r for r in step if r["queue"] == main and r["start"] < rrf[0]["start"]]
    bm = [r for r in step if r["queue"] != main and r["start"] < rrf[0]["start"]]
    return {"cosine_leg_end_us": round((max(r["end"] for r in cos) - t0) / 1e3, 1) if cos else None,
            "bm25_leg_end_us": round((max(r["end"] for r in bm) - t0) / 1e3, 1) if bm else None,
            "rrf_start_us": round((rrf[0]["start"] - t0) / 1e3, 1), "step_end_us": round((max(r["end"] for r in step) - t0) / 1e3, 1)}


def main():
    rows = load(sys.argv[1])
    steps = steps_of(rows)
    mid = steps[len(steps) // 2]
    for e in table(mid):
        print("%9.1f +%8.1f q=%s %s%s grid=%s" % (e["start_us"], e["dur_us"], e["queue"], e["kernel"], "  [%s]" % e["role"] if e["role"] else "", e["grid"]))
    print(legs(mid))
    print("head: %s us from the end of staging to the first thresholded screen launch" % head(mid))
    if "--json" in sys.argv:
        steady = steps[3:-1] if len(steps) > 6 else steps
        per = {}
        for s in steady:
            seen = {}
            for e in table(s):
                key = e["role"] or e["kernel"]
                n = seen[key] = seen.get(key, 0) + 1
                per.setdefault(key if n == 1 else "%s #%d" % (key, n), []).append(e["dur_us"])
        lg = [legs(s) for s in steady]
        lg = [x for x in lg if x and x["bm25_leg_end_us"] is not None]
        heads = [h for h in (head(s) for s in steady) if h is not None]
        out = {"steps_in_trace": len(steps), "steady_steps": len(steady), "one_step": table(mid), "one_step_legs": legs(mid),
               "median_head_us": round(statistics.median(heads), 1) if heads else None,
               "median_dur_us": {k: round(statistics.median(v), 1) for k, v in per.items()},
               "launches_per_step": {k: round(len(v) / len(steady), 2) for k, v in per.items()},
               "median_legs": {k: round(statistics.median(x[k] for x in lg), 1) for k in lg[0]} if lg else None,
               "cosine_leg_ends_last_in": sum(1 for x in lg if x["cosine_leg_end_us"] >= x["bm25_leg_end_us"]), "of_steps": len(lg)}
        json.dump(out, open(sys.argv[sys.argv.index("--json") + 1], "w"), indent=1)


if __name__ == "__main__":
    main()
