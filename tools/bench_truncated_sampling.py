#!/usr/bin/env python
"""Temperature / top-k / top-p in the sampled pick (include/set_hip.h SetSampleOpts) on one MI355X, B = 128 rows, V = 9490:
  * the pick alone (set_sample_pick_opts_f32 on (B, V) logits with a leading dimension of 9492 floats: the register path) in four
    configurations — neutral (the untruncated kernel), top_k = 50, top_p = 0.9, both.  One sample = --calls back-to-back launches
    between two device events, reported per launch; the four configurations alternate sample by sample in ONE process,
    --rounds rounds of --iters samples each; per configuration the median of every round, the median of those and their spread;
  * the EditNet fused sampled rollout (editnet_rl.DecoderC, D = 1024, A = 512, F = 2048, R = 36, T = 18, 18 words) with neutral
    options and with top_k = 50 + top_p = 0.9, alternated call by call, host clock around a device synchronise.
The neutral figures are the yardstick; the figure to read is what truncation adds to them.  One JSON line, also written to --out.

    python tools/bench_truncated_sampling.py [--iters 20] [--rounds 3] [--calls 200] [--out profiles/truncated_sampling_bench.json]
"""
import argparse, ctypes as C, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

CONFIGS = [("neutral", (1.0, 0, 1.0)), ("top_k50", (1.0, 50, 1.0)), ("top_p0.9", (1.0, 0, 0.9)), ("top_k50_top_p0.9", (1.0, 50, 0.9))]


def rounds_of(arms, rounds, iters):
    """arms {name: fn -> one sample}; the arms alternate sample by sample"""
    out = {name: [] for name in arms}
    for _ in range(rounds):
        got = {name: [] for name in arms}
        for _ in range(iters):
            for name, fn in arms.items():
                got[name].append(fn())
        for name in arms:
            out[name].append(statistics.median(got[name]))
    return out


def summary(r, digits):
    return {name: {"median": round(statistics.median(v), digits), "round_medians": [round(x, digits) for x in v],
                   "spread_between_rounds": round(max(v) - min(v), digits)} for name, v in r.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20); ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from show_edit_tell_amd import _lib as L, editnet_rl, synth
    lib = L.load()
    dev = torch.device("cuda", 0)
    B, V, ld, max_len = 128, 9490, 9492, 18
    st = L.stream_of(dev)
    g = torch.Generator(device="cpu").manual_seed(5)
    buf = torch.zeros(B, ld)
    buf[:, :V] = torch.randn(B, V, generator=g) * 2.0
    buf = buf.to(dev)
    seq, it = torch.zeros(B, max_len, dtype=torch.long, device=dev), torch.zeros(B, dtype=torch.long, device=dev)
    unf, alive = torch.ones(B, dtype=torch.int32, device=dev), torch.ones(max_len + 2, dtype=torch.int32, device=dev)
    raw, lse, lp = torch.empty(B, dtype=torch.long, device=dev), torch.empty(B, device=dev), torch.empty(B, device=dev)

    def pick_sample(o):
        opts = L.SampleOpts(temperature=o[0], top_k=o[1], top_p=o[2])

        def fn():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(a.calls):               # t = 1: the state is the caller's, no initialising launch in the window
                L.check(lib.set_sample_pick_opts_f32(L.ptr(buf), ld, B, V, 1, max_len, V - 1, 7, i, L.ptr(seq), L.ptr(it), L.ptr(unf),
                                                     L.ptr(alive), L.ptr(raw), L.ptr(lse), L.ptr(lp), st, C.byref(opts)))
            e1.record()
            e1.synchronize()
            return 1e3 * e0.elapsed_time(e1) / a.calls                      # us per launch
        return fn

    arms = {name: pick_sample(o) for name, o in CONFIGS}
    for fn in arms.values():
        fn()
    pick = summary(rounds_of(arms, a.rounds, a.iters), 2)
    base = pick["neutral"]["median"]
    for name in pick:
        pick[name]["added_us_over_neutral"] = round(pick[name]["median"] - base, 2)

    T, D, A, F, R = 18, 1024, 512, 2048, 36
    wm = synth.word_map(V)
    sd = synth.editnet_state(12, V, D, A, F, emb_scale=3.0, fc_scale=8.0, gain=3.0)
    sd["caption_encoder.embed.embedding.weight"] = sd["embed.embedding.weight"]
    dec = editnet_rl.DecoderC(wm, D, D, D, A, F)
    dec.load_state_dict({n: torch.from_numpy(v) for n, v in sd.items()})
    dec = dec.to(dev).eval()
    prev, plen = (torch.from_numpy(x).to(dev) for x in synth.prev_captions(37, B, T, V, 5))
    X = torch.from_numpy(synth.features(37, B, R, F)).to(dev)

    def rollout_sample(kw):
        def fn():
            torch.cuda.synchronize(); t = time.perf_counter()
            with torch.no_grad():
                dec(wm, prev, plen, X, sample_max=False, sample_rl=True, **kw)
            torch.cuda.synchronize()
            return 1e3 * (time.perf_counter() - t)                          # ms per rollout
        return fn

    arms = {"neutral": rollout_sample({}), "top_k50_top_p0.9": rollout_sample(dict(top_k=50, top_p=0.9))}
    for _ in range(3):                                                      # warm-up: token table, workspace
        for fn in arms.values():
            fn()
    roll = summary(rounds_of(arms, a.rounds, a.iters), 3)
    roll["top_k50_top_p0.9"]["added_ms_over_neutral"] = round(roll["top_k50_top_p0.9"]["median"] - roll["neutral"]["median"], 3)
    roll["top_k50_top_p0.9"]["added_us_per_word"] = round(
        1e3 * (roll["top_k50_top_p0.9"]["median"] - roll["neutral"]["median"]) / max_len, 2)
    result = {"config": "B=%d V=%d ld=%d; pick: us per launch, %d launches per sample; rollout: EditNet D=%d A=%d F=%d R=%d T=%d, "
                        "%d words, ms per call; %d rounds of %d alternated samples"
                        % (B, V, ld, a.calls, D, A, F, R, T, max_len, a.rounds, a.iters),
              "pick_us": pick, "editnet_sampled_rollout_ms": roll}
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
