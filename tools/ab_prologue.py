#!/usr/bin/env python
"""A/B of the decode prologue changes on ONE box: alternate child processes of `python bench.py --steps K --streams N` over
    parent     a built checkout of the parent commit (--parent DIR; left out without it)
    head_full  this tree with SET_PRO_ROWLIST=0 (the hoisted caption projections over all B*T rows: the single fill only)
    head       this tree as it ships (row list + single fill)
in that order, ROUNDS times per stream count, and write every run's `value` / `ms_per_step` with medians, spread and the pass
condition (every window of the later configuration faster than every window of the earlier one, same box) as JSON.

    python tools/ab_prologue.py [--parent DIR] [--pairs 5] [--steps 300] [--streams 7,1] [--out profiles/prologue_bench.json]

The switch is read once per process, hence child processes; each is bounded by --timeout and a failing child ends the run.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def one(root, steps, streams, env_extra, timeout):
    env = dict(os.environ, **env_extra)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", str(steps), "--streams", str(streams)],
                       env=env, cwd=root, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-3000:])
        raise SystemExit("bench.py failed with status %d in %s" % (r.returncode, root))
    line = json.loads(r.stdout.strip().splitlines()[-1])
    return {"value": line["value"], "ms_per_step": line["ms_per_step"]}


def summary(runs):
    v = [r["value"] for r in runs]
    m = [r["ms_per_step"] for r in runs]
    return {"runs": runs, "median_value": statistics.median(v), "min_value": min(v), "max_value": max(v),
            "spread_pct": round(100.0 * (max(v) - min(v)) / statistics.median(v), 3), "median_ms_per_step": statistics.median(m)}


def compare(a, b):
    return {"median_gain_pct": round(100.0 * (b["median_value"] / a["median_value"] - 1.0), 3),
            "median_ms_per_step_saved": round(a["median_ms_per_step"] - b["median_ms_per_step"], 5),
            "every_window_faster": b["min_value"] > a["max_value"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="built checkout of the parent commit")
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--streams", default="7,1")
    ap.add_argument("--timeout", type=int, default=120)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prologue_bench.json"))
    args = ap.parse_args()
    configs = [("head_full", ROOT, {"SET_PRO_ROWLIST": "0"}), ("head", ROOT, {"SET_PRO_ROWLIST": "1"})]
    if args.parent:
        configs.insert(0, ("parent", os.path.abspath(args.parent), {}))
    res = {"command": "python bench.py --steps %d --streams N; %s alternated in this order" % (args.steps, " / ".join(c[0] for c in configs)),
           "rounds": args.pairs}
    for n in (int(x) for x in args.streams.split(",")):
        runs = {name: [] for name, _, _ in configs}
        for i in range(args.pairs):
            for name, root, env in configs:
                runs[name].append(one(root, args.steps, n, env, args.timeout))
            print("streams %d round %d: %s" % (n, i, "  ".join("%s %.1f" % (k, v[-1]["value"]) for k, v in runs.items())), flush=True)
        s = {k: summary(v) for k, v in runs.items()}
        entry = dict(s)
        entry["row_list (head vs head_full)"] = compare(s["head_full"], s["head"])
        if args.parent:
            entry["single_fill (head_full vs parent)"] = compare(s["parent"], s["head_full"])
            entry["whole (head vs parent)"] = compare(s["parent"], s["head"])
        res["streams_%d" % n] = entry
        with open(args.out, "w") as f:                     # (rewritten after every stream count: a later failure keeps the earlier)
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps({k: {c: w for c, w in v.items() if " vs " in c} for k, v in res.items() if k.startswith("streams_")}))


if __name__ == "__main__":
    main()
