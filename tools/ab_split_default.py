"""A/B of the bf16-split default (EXPERIMENTS 10): child processes of `python bench.py --steps 300 --streams N`, alternated
parent / head with SET_GEMM_SPLIT=0 / head default, five rounds at --streams 7 and five at --streams 1, on one box in one job.

    python tools/ab_split_default.py --parent DIR [--rounds 5] [--steps 300] [--out profiles/split_default_bench.json]

DIR is a built checkout of the parent commit.  Every child runs under its own time limit; the first child that fails, is
killed by a signal or runs into its limit ends the job (nothing more is started on the GPU)."""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bench(root, streams, steps, env_extra, limit):
    env = {k: v for k, v in os.environ.items() if k != "SET_GEMM_SPLIT"}
    env.update(env_extra)
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", "10", "--streams", str(streams)],
                       cwd=root, env=env, capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        sys.exit("bench.py failed in %s (rc %d):\n%s" % (root, r.returncode, r.stderr[-2000:]))
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    return d["value"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--limit", type=int, default=120, help="seconds per child")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "split_default_bench.json"))
    a = ap.parse_args()
    arms = (("parent", a.parent, {}), ("head_split0", HERE, {"SET_GEMM_SPLIT": "0"}), ("head", HERE, {}))
    doc = {"what": "bench.py value (decode-steps/s), child processes alternated parent / head SET_GEMM_SPLIT=0 / head default",
           "steps": a.steps, "rounds": a.rounds, "streams": {}}
    for streams in (7, 1):
        vals = {name: [] for name, _, _ in arms}
        for r in range(a.rounds):
            for name, root, env in arms:
                vals[name].append(bench(root, streams, a.steps, env, a.limit))
                print("streams %d round %d %-12s %.1f" % (streams, r, name, vals[name][-1]), flush=True)
        p, h, h0 = vals["parent"], vals["head"], vals["head_split0"]
        med = lambda v: sorted(v)[len(v) // 2]
        doc["streams"][str(streams)] = {
            "values": vals, "median": {k: med(v) for k, v in vals.items()},
            "ratio_head_to_parent": round(med(h) / med(p), 4),
            "ratio_head_split0_to_parent": round(med(h0) / med(p), 4),
            "parent_spread_pct": round(100.0 * (max(p) - min(p)) / med(p), 3),
            "every_head_window_above_every_parent_window": min(h) > max(p),
            "no_head_window_below_every_parent_window": min(h) >= min(p),
            "head_split0_inside_parent_spread": min(p) <= med(h0) <= max(p)}
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    print(json.dumps({k: {kk: vv for kk, vv in v.items() if kk != "values"} for k, v in doc["streams"].items()}, indent=1))


if __name__ == "__main__":
    main()
