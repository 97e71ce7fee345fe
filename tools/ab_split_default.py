"""A/B of a bf16-split default (EXPERIMENTS 10, 11): child processes of `python bench.py --steps 300 --streams N`, alternated
parent / head under a control switch / head default, five rounds at --streams 7 and five at --streams 1, on one box in one job.

    python tools/ab_split_default.py --parent DIR [--control SET_PRO_SPLIT=0] [--rounds 5] [--steps 300]
                                     [--out profiles/prologue_split_bench.json]

DIR is a built checkout of the parent commit.  The control switch is the one that gives head the parent's behaviour
(SET_PRO_SPLIT=0: the greedy prologue back on the fp32 kernels; SET_GEMM_SPLIT=0 for EXPERIMENTS 10's A/B, whose parent had no
split kernel in the decode).  Before the rounds, `bench.py --dump-outputs` of the three arms is compared with the parent's
(`outputs_bench_batch`: seq equal, max |d seq_logp|, whether seq_logp has the parent's bits).  Every child runs under its own time limit; the first child that fails, is killed by a signal or
runs into its limit ends the job (nothing more is started on the GPU)."""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ("SET_GEMM_SPLIT", "SET_PRO_SPLIT")


def bench(root, streams, steps, env_extra, limit):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(env_extra)
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", "10", "--streams", str(streams)],
                       cwd=root, env=env, capture_output=True, text=True, timeout=limit)
    if r.returncode != 0:
        sys.exit("bench.py failed in %s (rc %d):\n%s" % (root, r.returncode, r.stderr[-2000:]))
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    return d["value"]


def outputs(arms, limit):
    """`bench.py --dump-outputs` of every arm, compared with the first (the parent): seq equal, max |d seq_logp|, seq_logp bits"""
    import tempfile
    import numpy as np
    got = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, root, env_extra in arms:
            d = os.path.join(tmp, name)
            env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
            env.update(env_extra)
            r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "3", "--dump-outputs", d],
                               cwd=root, env=env, capture_output=True, text=True, timeout=limit)
            if r.returncode != 0:
                sys.exit("bench.py --dump-outputs failed in %s (rc %d):\n%s" % (root, r.returncode, r.stderr[-2000:]))
            got[name] = (np.load(os.path.join(d, "seq.npy")), np.load(os.path.join(d, "seq_logp.npy")))
    pseq, plp = got[arms[0][0]]
    return {name: {"seq_equal_to_parent": bool(np.array_equal(seq, pseq)),
                   "max_abs_dlogp_to_parent": float(np.abs(lp.astype(np.float64) - plp).max()),
                   "logp_bits_equal_to_parent": bool(np.array_equal(lp.view(np.uint32), plp.view(np.uint32)))}
            for name, (seq, lp) in got.items() if name != arms[0][0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--control", default="SET_PRO_SPLIT=0", help="NAME=VALUE: head with the parent's behaviour")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--limit", type=int, default=120, help="seconds per child")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "prologue_split_bench.json"))
    a = ap.parse_args()
    cname, cval = a.control.split("=", 1)
    if cname not in SWITCHES:
        sys.exit("--control: one of %s" % (SWITCHES,))
    arms = (("parent", a.parent, {}), ("head_control", HERE, {cname: cval}), ("head", HERE, {}))
    doc = {"what": "bench.py value (decode-steps/s), child processes alternated parent / head %s / head default" % a.control,
           "control": a.control, "steps": a.steps, "rounds": a.rounds, "streams": {}}
    doc["outputs_bench_batch"] = outputs(arms, a.limit)
    print(json.dumps(doc["outputs_bench_batch"]), flush=True)
    for streams in (7, 1):
        vals = {name: [] for name, _, _ in arms}
        for r in range(a.rounds):
            for name, root, env in arms:
                vals[name].append(bench(root, streams, a.steps, env, a.limit))
                print("streams %d round %d %-12s %.1f" % (streams, r, name, vals[name][-1]), flush=True)
        p, h, h0 = vals["parent"], vals["head"], vals["head_control"]
        med = lambda v: sorted(v)[len(v) // 2]
        spread = (max(p) - min(p)) / med(p)
        doc["streams"][str(streams)] = {
            "values": vals, "median": {k: med(v) for k, v in vals.items()},
            "ratio_head_to_parent": round(med(h) / med(p), 4),
            "ratio_head_control_to_parent": round(med(h0) / med(p), 4),
            "parent_spread_pct": round(100.0 * spread, 3),
            "every_head_window_above_every_parent_window": min(h) > max(p),
            "ratio_exceeds_parent_spread": med(h) / med(p) - 1.0 > spread,
            "no_head_window_below_every_parent_window": min(h) >= min(p),
            "head_control_inside_parent_spread": min(p) <= med(h0) <= max(p)}
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    print(json.dumps({k: {kk: vv for kk, vv in v.items() if kk != "values"} for k, v in doc["streams"].items()}, indent=1))


if __name__ == "__main__":
    main()
