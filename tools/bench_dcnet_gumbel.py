#!/usr/bin/env python
"""DCNet's Gumbel-max sampled decode as one persistent launch (include/set_hip.h set_dcnet_gumbel_persistent) against the
per-step loops on one MI355X: dcnet_full_b4's model (D = 1024, A = 512, C = 512, V = 10000, T = 18, 18 words),
evaluate.sample_captions for ONE previous caption at n_samples = 1, 4, 5 and 8 rows, in three arms alternated call by call in ONE
process (the protocol of tools/bench_gumbel_sampling.py):
      "cdf"               sampler="cdf": the per-step loop with the inverse-CDF pick
      "gumbel_per_step"   sampler="gumbel" with SET_DEC_PERSISTENT=0 (set_dcnet_sample_gumbel) — the route before the launch existed
      "gumbel_persistent" sampler="gumbel" (set_dcnet_gumbel_persistent: one launch)
host clock around a device synchronise, ms per call; --rounds rounds of --iters samples each, per arm the median of every round,
the median of those and the spread between rounds.  4 rows are measured twice: T = 18 (the resident kernel variant) and the same
caption padded with zero columns to T = 24 (above PDEC_TREG: the general variant).  "gumbel_per_step" is the yardstick: a row
count belongs on the persistent launch only if it is faster there by more than the spread between rounds.
One JSON line, also written to --out.

    python tools/bench_dcnet_gumbel.py [--iters 20] [--rounds 3] [--out profiles/dcnet_gumbel_bench.json]
"""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import time
import torch

from bench_gumbel_sampling import rounds_of, summary

ROWS = (1, 4, 5, 8)
PAD_T = 24


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20); ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from show_edit_tell_amd import _lib as L, dcnet_rl, evaluate, synth
    lib = L.load()
    dev = torch.device("cuda", 0)
    T, V, D, A, Cc, E = 18, 10000, 1024, 512, 512, 1024
    wm = synth.word_map(V)
    sd = synth.dcnet_state(18, V, D, A, Cc, E, emb_scale=3.0, fc_scale=8.0, gain=3.0)
    sd["caption_encoder.embed.embedding.weight"] = sd["embed.embedding.weight"]
    dae = dcnet_rl.DAE(wm, None, D, A, Cc, E)
    dae.load_state_dict({n: torch.from_numpy(v) for n, v in sd.items()})
    dae = dae.to(dev).eval()
    prev, plen = (torch.from_numpy(x).to(dev) for x in synth.prev_captions(36, 1, T, V, 5))
    prev_pad = torch.cat([prev, torch.zeros(1, PAD_T - T, dtype=prev.dtype, device=dev)], 1).contiguous()

    def captions_sample(p, n, sampler, persistent):
        def fn():
            old = os.environ.get("SET_DEC_PERSISTENT")
            if not persistent:
                os.environ["SET_DEC_PERSISTENT"] = "0"           # (read by the library at every call)
            try:
                torch.cuda.synchronize(); t = time.perf_counter()
                evaluate.sample_captions(dae, p, plen, wm, n_samples=n, sampler=sampler)
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
    for name, p, n in [("rows_%d" % n, prev, n) for n in ROWS] + [("rows_4_T%d_general" % PAD_T, prev_pad, 4)]:
        arms = {"cdf": captions_sample(p, n, "cdf", True), "gumbel_per_step": captions_sample(p, n, "gumbel", False),
                "gumbel_persistent": captions_sample(p, n, "gumbel", True)}
        for _ in range(3):                                           # warm-up: token table, workspaces
            for fn in arms.values():
                fn()
        lib.set_profile_enable(1)
        arms["gumbel_persistent"]()
        tags = [r["tag"] for r in L.profile_report()]
        lib.set_profile_enable(0)
        s = summary(rounds_of(arms, a.rounds, a.iters), 3)
        s["gumbel_persistent"]["took_the_persistent_launch"] = "persistent_gumbel" in tags
        for arm in ("cdf", "gumbel_persistent"):
            s[arm]["ratio_to_gumbel_per_step"] = round(s[arm]["median"] / s["gumbel_per_step"]["median"], 3)
        spread = max(s["gumbel_per_step"]["spread_between_rounds"], s["gumbel_persistent"]["spread_between_rounds"])
        s["persistent_faster_by_more_than_the_spread"] = bool(
            s["gumbel_per_step"]["median"] - s["gumbel_persistent"]["median"] > spread)
        captions[name] = s

    result = {"config": "DCNet D=%d A=%d C=%d V=%d T=%d (general-variant arm: T=%d), %d words, one previous caption; "
                        "sample_captions: ms per call; %d rounds of %d alternated samples"
                        % (D, A, Cc, V, T, PAD_T, dae.max_len, a.rounds, a.iters),
              "sample_captions_ms": captions}
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
