#!/usr/bin/env python
"""The Gumbel-max sampler (include/set_hip.h "Gumbel-max draw") against the inverse-CDF sampler on one MI355X, full-size
EditNet (D = 1024, A = 512, F = 2048, R = 36, T = 18, 18 words), V = 9490:
  * evaluate.sample_captions for ONE image at n_samples = 1, 5 and 16 rows, in three arms alternated call by call in ONE process:
      "cdf"               today's route (the per-step loop with the inverse-CDF pick), unchanged
      "gumbel_per_step"   sampler="gumbel" with SET_DEC_PERSISTENT=0 (set_editnet_sample_gumbel)
      "gumbel_persistent" sampler="gumbel" (set_editnet_gumbel_persistent: one launch)
    host clock around a device synchronise, ms per call; --rounds rounds of --iters samples each, per arm the median of every
    round, the median of those and the spread between rounds;
  * the per-step pick alone at the same row counts: set_gumbel_pick_f32 against set_sample_pick_f32 on (B, V) logits with a
    leading dimension of 9492 floats (the register path), --calls back-to-back launches between two device events, us per launch.
The "cdf" arm is the yardstick.  One JSON line, also written to --out.

    python tools/bench_gumbel_sampling.py [--iters 20] [--rounds 3] [--calls 200] [--out profiles/gumbel_sampling_bench.json]
"""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

ROWS = (1, 5, 16)


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
    from show_edit_tell_amd import _lib as L, editnet_rl, evaluate, synth
    lib = L.load()
    dev = torch.device("cuda", 0)
    V, ld, max_len = 9490, 9492, 18
    T, D, A, F, R = 18, 1024, 512, 2048, 36
    wm = synth.word_map(V)
    sd = synth.editnet_state(12, V, D, A, F, emb_scale=3.0, fc_scale=8.0, gain=3.0)
    sd["caption_encoder.embed.embedding.weight"] = sd["embed.embedding.weight"]
    dec = editnet_rl.DecoderC(wm, D, D, D, A, F)
    dec.load_state_dict({n: torch.from_numpy(v) for n, v in sd.items()})
    dec = dec.to(dev).eval()
    prev, plen = (torch.from_numpy(x).to(dev) for x in synth.prev_captions(37, 1, T, V, 5))
    X = torch.from_numpy(synth.features(37, 1, R, F)).to(dev)

    def captions_sample(n, sampler, persistent):
        def fn():
            old = os.environ.get("SET_DEC_PERSISTENT")
            if not persistent:
                os.environ["SET_DEC_PERSISTENT"] = "0"           # (read by the library at every call)
            try:
                torch.cuda.synchronize(); t = time.perf_counter()
                evaluate.sample_captions(dec, X, prev, plen, wm, n_samples=n, sampler=sampler)
                torch.cuda.synchronize()
                return 1e3 * (time.perf_counter() - t)               # ms per call
            finally:
                if not persistent:
                    if old is None:
                        del os.environ["SET_DEC_PERSISTENT"]
                    else:
                        os.environ["SET_DEC_PERSISTENT"] = old
        return fn

    captions = {}
    for n in ROWS:
        arms = {"cdf": captions_sample(n, "cdf", True), "gumbel_per_step": captions_sample(n, "gumbel", False),
                "gumbel_persistent": captions_sample(n, "gumbel", True)}
        for _ in range(3):                                           # warm-up: token table, workspaces
            for fn in arms.values():
                fn()
        lib.set_profile_enable(1)
        arms["gumbel_persistent"]()
        tags = [r["tag"] for r in L.profile_report()]
        lib.set_profile_enable(0)
        s = summary(rounds_of(arms, a.rounds, a.iters), 3)
        s["gumbel_persistent"]["took_the_persistent_launch"] = "persistent_gumbel" in tags
        for name in ("gumbel_per_step", "gumbel_persistent"):
            s[name]["ratio_to_cdf"] = round(s[name]["median"] / s["cdf"]["median"], 3)
        captions["rows_%d" % n] = s

    st = L.stream_of(dev)
    pick = {}
    for B in ROWS:
        g = torch.Generator(device="cpu").manual_seed(5)
        buf = torch.zeros(B, ld)
        buf[:, :V] = torch.randn(B, V, generator=g) * 2.0
        buf = buf.to(dev)
        seq, it = torch.zeros(B, max_len, dtype=torch.long, device=dev), torch.zeros(B, dtype=torch.long, device=dev)
        unf, alive = torch.ones(B, dtype=torch.int32, device=dev), torch.ones(max_len + 2, dtype=torch.int32, device=dev)
        raw, lse, lp = torch.empty(B, dtype=torch.long, device=dev), torch.empty(B, device=dev), torch.empty(B, device=dev)

        def pick_sample(gumbel):
            def fn():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for i in range(a.calls):               # t = 1: the state is the caller's, no initialising launch in the window
                    if gumbel:
                        L.check(lib.set_gumbel_pick_f32(L.ptr(buf), ld, B, V, 1, max_len, V - 1, 7, i, L.ptr(seq), L.ptr(it), L.ptr(unf),
                                                        L.ptr(alive), L.ptr(raw), L.ptr(lse), L.ptr(lp), st, None))
                    else:
                        L.check(lib.set_sample_pick_f32(L.ptr(buf), ld, B, V, 1, max_len, V - 1, 7, i, L.ptr(seq), L.ptr(it), L.ptr(unf),
                                                        L.ptr(alive), L.ptr(raw), L.ptr(lse), L.ptr(lp), st))
                e1.record()
                e1.synchronize()
                return 1e3 * e0.elapsed_time(e1) / a.calls                      # us per launch
            return fn

        arms = {"sample_pick": pick_sample(False), "gumbel_pick": pick_sample(True)}
        for fn in arms.values():
            fn()
        s = summary(rounds_of(arms, a.rounds, a.iters), 2)
        s["gumbel_pick"]["added_us_over_sample_pick"] = round(s["gumbel_pick"]["median"] - s["sample_pick"]["median"], 2)
        pick["rows_%d" % B] = s

    result = {"config": "EditNet D=%d A=%d F=%d R=%d T=%d V=%d, %d words, one image; sample_captions: ms per call; pick: ld=%d, us per "
                        "launch, %d launches per sample; %d rounds of %d alternated samples"
                        % (D, A, F, R, T, V, max_len, ld, a.calls, a.rounds, a.iters),
              "sample_captions_ms": captions, "pick_us": pick}
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
