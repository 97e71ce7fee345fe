#!/usr/bin/env python
"""DCNet's beam search of ONE previous caption per call (evaluate.beam_search_dcnet, the reference's convention) at full
dimensions (D = 1024, A = 512, V = 10000, T = 18: the dcnet_full_b4 model), k = 3, 16 prompts, on one MI355X:
  * two workloads — the plain weights, whose searches run into the 50-step limit, and the same weights with fc.bias[<end>]
    raised by --boost, whose searches end after a pick or two (mostly prologue);
  * two arms in ONE process — the persistent launch (set_dcnet_beam_persistent) and, with SET_DEC_PERSISTENT=0 (read on every
    call), the per-step kernels (set_dcnet_step + set_beam_pick_f32 + set_beam_gather_f32: the route before the launch existed);
  * interleaved A B A B prompt by prompt, --rounds rounds; per arm the median of every round, the median of those and their
    spread (max - min) between rounds; token equality between the arms.
One JSON line, also written to --out.  Kernel statistics: run it under `rocprofv3 --kernel-trace --stats -d <dir> -o run --`
in a separate run (no counters in that run); per-pick phases inside the launch: SET_PDEC_STAMPS=1 in a separate run.

    python tools/bench_dcnet_beam.py [--prompts 16] [--rounds 3] [--boost 4.0] [--n-best N] [--out profiles/dcnet_beam_bench.json]
"""
import argparse, json, math, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prompts", type=int, default=16); ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--beam", type=int, default=3)
    ap.add_argument("--boost", type=float, default=4.0, help="fc.bias[<end>] raise of the ending workload")
    ap.add_argument("--n-best", type=int, default=0, help="time the searches with n_best=N (0: off, the default)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from show_edit_tell_amd import dcnet, evaluate, synth
    dev = torch.device("cuda", 0)
    NI, T, V, D, A, Cc, E, k = a.prompts, 18, 10000, 1024, 512, 512, 1024, a.beam
    wm = synth.word_map(V)
    prev, plen = (torch.from_numpy(x).to(dev) for x in synth.prev_captions(36, NI, T, V, 5))

    def model(boost):
        sd = synth.dcnet_state(18, V, D, A, Cc, E, emb_scale=3.0, fc_scale=8.0, gain=3.0)
        sd["fc.bias"] = sd["fc.bias"].copy(); sd["fc.bias"][wm["<end>"]] += boost
        sd["caption_encoder.embed.embedding.weight"] = sd["embed.embedding.weight"]
        m = dcnet.DAE(wm, None, D, A, Cc, E); m.load_state_dict({n: torch.from_numpy(v) for n, v in sd.items()})
        return m.to(dev).eval()

    def timed(fn):
        torch.cuda.synchronize(); t = time.perf_counter(); out = fn(); torch.cuda.synchronize()
        return time.perf_counter() - t, out

    kw = {"n_best": a.n_best} if a.n_best else {}              # (the result gains the n-best list as a third element)
    one = lambda b: (prev[b:b + 1], plen[b:b + 1])
    env0 = os.environ.get("SET_DEC_PERSISTENT")
    result = {"config": "DCNet D=%d A=%d V=%d T=%d, k=%d, %d prompts, %d rounds, arms alternated prompt by prompt" % (D, A, V, T, k, NI, a.rounds),
              "n_best": a.n_best}
    try:
        for name, boost in (("step_limit", 0.0), ("ending", a.boost)):
            dae = model(boost)
            for b in range(NI):                                   # warm-up: token table, LDS setup, workspaces of both arms
                for v in ("1", "0", "1", "0"):
                    os.environ["SET_DEC_PERSISTENT"] = v
                    evaluate.beam_search_dcnet(dae, *one(b), wm, k)
            os.environ["SET_DEC_PERSISTENT"] = "1"
            assert evaluate._beam_search_dcnet_persistent(dae, *one(0), wm, k) is not None, "the persistent launch is not taken"
            rounds = {"persistent": [], "per_step": []}
            lens, same, limit = [], 0, 0
            for _ in range(a.rounds):
                tp, ts = [], []
                for b in range(NI):
                    os.environ["SET_DEC_PERSISTENT"] = "1"
                    t1, (sp, scp, *_) = timed(lambda: evaluate.beam_search_dcnet(dae, *one(b), wm, k, **kw))
                    os.environ["SET_DEC_PERSISTENT"] = "0"
                    t0, (ss, scs, *_) = timed(lambda: evaluate.beam_search_dcnet(dae, *one(b), wm, k, **kw))
                    tp.append(t1); ts.append(t0)
                    lens.append(len(sp)); same += int(sp == ss); limit += int(math.isnan(scp))
                rounds["persistent"].append(1e3 * statistics.median(tp)); rounds["per_step"].append(1e3 * statistics.median(ts))
            med = {arm: statistics.median(v) for arm, v in rounds.items()}
            spread = {arm: max(v) - min(v) for arm, v in rounds.items()}
            result[name] = {
                "end_boost": boost,
                "persistent_ms_median": round(med["persistent"], 3), "per_step_ms_median": round(med["per_step"], 3),
                "persistent_ms_round_medians": [round(x, 3) for x in rounds["persistent"]],
                "per_step_ms_round_medians": [round(x, 3) for x in rounds["per_step"]],
                "spread_between_rounds_ms": round(max(spread.values()), 3),
                "persistent_over_per_step": round(med["persistent"] / med["per_step"], 3),
                "per_step_minus_persistent_ms": round(med["per_step"] - med["persistent"], 3),
                "mean_tokens": round(sum(lens) / len(lens), 2), "searches_at_step_limit": "%d/%d" % (limit, len(lens)),
                "same_tokens": "%d/%d" % (same, len(lens)),
            }
            del dae
    finally:
        if env0 is None:
            os.environ.pop("SET_DEC_PERSISTENT", None)
        else:
            os.environ["SET_DEC_PERSISTENT"] = env0
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
