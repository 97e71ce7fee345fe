#!/usr/bin/env python
"""A/B of SET_DEAD_WORK on ONE box: alternate child processes of `python bench.py --steps K --streams N` with the switch set
("old": the discarded last timestep and the zero-state products run) and unset ("new"), old first, PAIRS times per stream
count, and write every run's `value` / `ms_per_step` with medians, spread and the pass condition (every new window faster
than every old window of the same box) as JSON.

    python tools/ab_dead_work.py [--pairs 5] [--steps 300] [--streams 7,1] [--out profiles/dead_work_bench.json]

The switch is read once per process, hence child processes; each is bounded by --timeout and a failing child ends the run.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def one(steps, streams, dead, timeout):
    env = dict(os.environ, SET_DEAD_WORK="1" if dead else "0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", str(steps), "--streams", str(streams)],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0:
        sys.stderr.write(r.stderr[-3000:])
        raise SystemExit("bench.py failed with status %d" % r.returncode)
    line = json.loads(r.stdout.strip().splitlines()[-1])
    return {"value": line["value"], "ms_per_step": line["ms_per_step"]}


def summary(runs):
    v = [r["value"] for r in runs]
    m = [r["ms_per_step"] for r in runs]
    return {"runs": runs, "median_value": statistics.median(v), "min_value": min(v), "max_value": max(v),
            "spread_pct": round(100.0 * (max(v) - min(v)) / statistics.median(v), 3), "median_ms_per_step": statistics.median(m)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--streams", default="7,1")
    ap.add_argument("--timeout", type=int, default=120)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dead_work_bench.json"))
    args = ap.parse_args()
    res = {"command": "python bench.py --steps %d --streams N, SET_DEAD_WORK=1 (old) / unset (new) alternated, old first"
                      % args.steps, "pairs": args.pairs}
    for n in (int(x) for x in args.streams.split(",")):
        old, new = [], []
        for i in range(args.pairs):
            old.append(one(args.steps, n, True, args.timeout))
            new.append(one(args.steps, n, False, args.timeout))
            print("streams %d pair %d: old %.1f  new %.1f" % (n, i, old[-1]["value"], new[-1]["value"]), flush=True)
        o, w = summary(old), summary(new)
        res["streams_%d" % n] = {
            "old": o, "new": w,
            "median_gain_pct": round(100.0 * (w["median_value"] / o["median_value"] - 1.0), 3),
            "every_new_window_faster_than_every_old": w["min_value"] > o["max_value"]}
        with open(args.out, "w") as f:                     # (rewritten after every stream count: a later failure keeps the earlier)
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps({k: {"gain_pct": v["median_gain_pct"], "pass": v["every_new_window_faster_than_every_old"]}
                      for k, v in res.items() if k.startswith("streams_")}))


if __name__ == "__main__":
    main()
