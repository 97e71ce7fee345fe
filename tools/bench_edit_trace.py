#!/usr/bin/env python
"""The edit trace (evaluate.edit_trace: forced decode of given tokens that records caption attention, selected slot, copy gate,
visual attention and the forced word's log-probability per step) at full dimensions (D = 1024, A = 512, F = 2048, V = 10000,
R = 36, T = 18: the editnet_full_b4 model), S = 18 forced steps, B = 4 and B = 128 rows, on one MI355X:
  * arm A — the forced trace decode (set_editnet_edit_trace: prologue + per step the step's kernels, gate_cnew(c_new) as a
    grouped GEMM and the record launch);
  * arm B — the no-grad teacher-forced forward of the same tokens (DecoderC.forward -> set_editnet_xe_forward) with
    SET_DEC_PERSISTENT=0 (read on every call), i.e. on the same per-step kernels, without a record;
  * interleaved A B A B call by call in ONE process, --rounds rounds of --iters pairs; per arm the median of every round, the
    median of those and their spread (max - min) between rounds.
The figure to read is the trace's added time per step over arm B: (A - B) / S.  One JSON line, also written to --out.

    python tools/bench_edit_trace.py [--iters 20] [--rounds 3] [--out profiles/edit_trace_bench.json]
"""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20); ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batches", default="4,128")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from show_edit_tell_amd import editnet, evaluate, synth
    dev = torch.device("cuda", 0)
    T, V, D, A, F, R, S = 18, 10000, 1024, 512, 2048, 36, 18
    wm = synth.word_map(V)
    sd = synth.editnet_state(12, V, D, A, F, emb_scale=3.0, fc_scale=8.0, gain=3.0)
    sd["caption_encoder.embed.embedding.weight"] = sd["embed.embedding.weight"]
    dec = editnet.DecoderC(wm, D, D, D, A, F)
    dec.load_state_dict({n: torch.from_numpy(v) for n, v in sd.items()})
    dec = dec.to(dev).eval()

    def timed(fn):
        torch.cuda.synchronize(); t = time.perf_counter(); out = fn(); torch.cuda.synchronize()
        return time.perf_counter() - t, out

    env0 = os.environ.get("SET_DEC_PERSISTENT")
    result = {"config": "EditNet D=%d A=%d F=%d V=%d R=%d T=%d, S=%d forced steps, %d rounds of %d alternated pairs"
                        % (D, A, F, V, R, T, S, a.rounds, a.iters)}
    try:
        os.environ["SET_DEC_PERSISTENT"] = "0"
        for B in (int(x) for x in a.batches.split(",")):
            prev, plen = (torch.from_numpy(x).to(dev) for x in synth.prev_captions(37, B, T, V, 5))
            X = torch.from_numpy(synth.features(37, B, R, F)).to(dev)
            words = torch.from_numpy(synth.integers(37, "trace.tok", (B, S + 1), 1, V - 3)).to(dev).long()
            words[:, 0] = wm["<start>"]
            lens = torch.full((B, 1), S + 1, dtype=torch.long, device=dev)

            def arm_a():
                return evaluate.edit_trace(dec, X, prev, plen, wm, words, lengths=lens)

            def arm_b():
                with torch.no_grad():
                    return dec(X, words, lens, prev, plen)

            for _ in range(3):                                    # warm-up: token table, workspaces of both arms
                arm_a(); arm_b()
            rounds = {"trace": [], "forward": []}
            for _ in range(a.rounds):
                ta, tb = [], []
                for _ in range(a.iters):
                    ta.append(timed(arm_a)[0]); tb.append(timed(arm_b)[0])
                rounds["trace"].append(1e3 * statistics.median(ta)); rounds["forward"].append(1e3 * statistics.median(tb))
            med = {arm: statistics.median(v) for arm, v in rounds.items()}
            spread = {arm: max(v) - min(v) for arm, v in rounds.items()}
            # the two arms decode the same steps: the forward's logits reproduce the trace's log-probabilities
            tr, pred = arm_a(), arm_b()[0]
            lp = torch.log_softmax(pred, 2).gather(2, words[:, 1:, None])[:, :, 0]
            result["B%d" % B] = {
                "trace_ms_median": round(med["trace"], 3), "forward_ms_median": round(med["forward"], 3),
                "trace_ms_round_medians": [round(x, 3) for x in rounds["trace"]],
                "forward_ms_round_medians": [round(x, 3) for x in rounds["forward"]],
                "spread_between_rounds_ms": round(max(spread.values()), 3),
                "trace_minus_forward_ms": round(med["trace"] - med["forward"], 3),
                "added_us_per_step": round(1e3 * (med["trace"] - med["forward"]) / S, 2),
                "trace_over_forward": round(med["trace"] / med["forward"], 3),
                "max_abs_logp_difference": float((lp - tr.logp).abs().max()),
            }
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
