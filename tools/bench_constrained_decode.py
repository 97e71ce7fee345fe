#!/usr/bin/env python
"""Constrained greedy and sampled decoding (include/set_hip.h "Constrained greedy and sampled picks") on one MI355X, V = 9490:
  * the pick alone at B = 5 and B = 128 rows, timestep t = 10 of 18, greedy and sampled, through set_pick_slabs_opts_f32 (the
    unconstrained yardstick of the same run) and set_pick_slabs_constrained_f32 under three settings: neutral constraints,
    no_repeat_ngram = 3 with two banned words (ld = 9492: the register path), and the same on the scalar layout (ld = 9490, beside
    the unconstrained pick on that layout).  One sample = --calls back-to-back launches between two device events, reported per
    launch; the arms alternate sample by sample in ONE process, --rounds rounds of --iters samples; per arm the median of every
    round, the median of those and their spread, and the ratio to the unconstrained arm of the same layout;
  * whole greedy and sampled decodes (18 words) of EditNet (D = 1024, A = 512, F = 2048, R = 36, T = 18) and DCNet (D = E = 1024,
    A = C = 512) at B = 128 and B = 5 with and without constraints=BeamConstraints(no_repeat_ngram=3, min_length=4, two banned
    words), alternated call by call, host clock around a device synchronise.  (At B = 5 the unconstrained greedy decode is one
    persistent launch; a constrained call runs the per-step kernels.)
One JSON line, also written to --out.

    python tools/bench_constrained_decode.py [--iters 10] [--rounds 3] [--calls 200] [--out profiles/constrained_decode_bench.json]
"""
import argparse, ctypes as C, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

SHORT_LAUNCH_US = 4.0        # what one more short launch per timestep costs in this project's stamps (EXPERIMENTS)


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
    ap.add_argument("--iters", type=int, default=10); ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from show_edit_tell_amd import _lib as L, dcnet_rl, editnet_rl, synth
    from show_edit_tell_amd.evaluate import BeamConstraints
    lib = L.load()
    dev = torch.device("cuda", 0)
    V, max_len, t = 9490, 18, 10
    st = L.stream_of(dev)
    banned = torch.tensor([3, 17], dtype=torch.long, device=dev)
    neutral = L.BeamConstraintsC(0, 0, 0.0, 0, None)
    active = L.BeamConstraintsC(3, 0, 0.0, 2, banned.data_ptr())
    pick = {}
    for B in (5, 128):
        g = torch.Generator(device="cpu").manual_seed(5)
        x = torch.randn(B, V, generator=g) * 2.0
        bufs = {}
        for ld in (9492, 9490):
            buf = torch.zeros(B * ld + 8)
            buf[:B * ld].view(B, ld)[:, :V] = x
            bufs[ld] = buf.to(dev)
        seq = torch.randint(1, 6, (B, max_len), generator=g).to(dev)       # a small alphabet: trigrams repeat, rule c has hits
        it = torch.zeros(B, dtype=torch.long, device=dev)
        unf, alive = torch.ones(B, dtype=torch.int32, device=dev), torch.ones(max_len + 2, dtype=torch.int32, device=dev)
        logp = torch.zeros(B, max_len, device=dev)
        raw, lse, lp = torch.empty(B, dtype=torch.long, device=dev), torch.empty(B, device=dev), torch.empty(B, device=dev)

        def arm(mode, ld, cons):
            args = L.PickArgs(logits=bufs[ld].data_ptr(), ld=ld, stride=0, end_idx=V - 1, seq=seq.data_ptr(), seq_logp=logp.data_ptr(),
                              it=it.data_ptr(), unfinished=unf.data_ptr(), alive=alive.data_ptr(), seed=7, offset=0,
                              raw_ids=raw.data_ptr(), lse=lse.data_ptr(), step_logp=lp.data_ptr(), n=1, B=B, V=V, t=t, max_len=max_len,
                              D=4, mode=mode)

            def fn():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for i in range(a.calls):
                    args.offset = i
                    if cons is None:
                        L.check(lib.set_pick_slabs_opts_f32(C.byref(args), None, st))
                    else:
                        L.check(lib.set_pick_slabs_constrained_f32(C.byref(args), None, C.byref(cons), st))
                e1.record()
                e1.synchronize()
                return 1e3 * e0.elapsed_time(e1) / a.calls                  # us per launch
            return fn

        for mode, mname in ((L.PICK_GREEDY, "greedy"), (L.PICK_SAMPLE, "sample")):
            arms = {"unconstrained": arm(mode, 9492, None), "neutral": arm(mode, 9492, neutral), "ngram3_2banned": arm(mode, 9492, active),
                    "scalar_unconstrained": arm(mode, 9490, None), "scalar_ngram3_2banned": arm(mode, 9490, active)}
            for fn in arms.values():
                fn()
            r = summary(rounds_of(arms, a.rounds, a.iters), 2)
            for name in r:
                base = r["scalar_unconstrained" if name.startswith("scalar") else "unconstrained"]["median"]
                r[name]["ratio_to_unconstrained"] = round(r[name]["median"] / base, 3)
                r[name]["added_us"] = round(r[name]["median"] - base, 2)
            pick["B%d_%s" % (B, mname)] = r

    T, D, A, F, R, Cc = 18, 1024, 512, 2048, 36, 512
    wm = synth.word_map(V)
    sd = synth.editnet_state(12, V, D, A, F, emb_scale=3.0, fc_scale=8.0, gain=3.0)
    sd["caption_encoder.embed.embedding.weight"] = sd["embed.embedding.weight"]
    dec = editnet_rl.DecoderC(wm, D, D, D, A, F)
    dec.load_state_dict({n: torch.from_numpy(v) for n, v in sd.items()})
    dec = dec.to(dev).eval()
    dae = dcnet_rl.DAE(wm, None, D, A, Cc, D)
    sd = synth.dcnet_state(18, V, D, A, Cc, D, 3.0, 8.0, 3.0)
    sd["caption_encoder.embed.embedding.weight"] = sd["embed.embedding.weight"]
    dae.load_state_dict({n: torch.from_numpy(v) for n, v in sd.items()})
    dae = dae.to(dev).eval()
    bc = BeamConstraints(no_repeat_ngram=3, min_length=4, banned_words=[3, 17])
    decodes = {}
    for B in (128, 5):
        prev, plen = (torch.from_numpy(x).to(dev) for x in synth.prev_captions(37, B, T, V, 5))
        X = torch.from_numpy(synth.features(37, B, R, F)).to(dev)

        def call(model, inputs, sample, kw):
            def fn():
                torch.cuda.synchronize(); t0 = time.perf_counter()
                with torch.no_grad():
                    model(wm, *inputs, sample_max=not sample, sample_rl=sample, **kw)
                torch.cuda.synchronize()
                return 1e3 * (time.perf_counter() - t0)                     # ms per decode
            return fn

        for mname, model, inputs in (("editnet", dec, (prev, plen, X)), ("dcnet", dae, (prev, plen))):
            for sample in (False, True):
                arms = {"unconstrained": call(model, inputs, sample, {}), "constrained": call(model, inputs, sample, dict(constraints=bc))}
                for _ in range(3):                                          # warm-up: token table, workspace
                    for fn in arms.values():
                        fn()
                r = summary(rounds_of(arms, a.rounds, a.iters), 3)
                r["constrained"]["ratio_to_unconstrained"] = round(r["constrained"]["median"] / r["unconstrained"]["median"], 3)
                r["constrained"]["added_us_per_word"] = round(1e3 * (r["constrained"]["median"] - r["unconstrained"]["median"]) / max_len, 2)
                decodes["%s_B%d_%s" % (mname, B, "sample" if sample else "greedy")] = r
    result = {"config": "V=%d t=%d of %d; pick: us per launch, %d launches per sample, ld 9492 (register path) / 9490 (scalar_*); "
                        "decodes: ms per call of 18 words; %d rounds of %d alternated samples; one short launch ~ %.0f us"
                        % (V, t, max_len, a.calls, a.rounds, a.iters, SHORT_LAUNCH_US),
              "pick_us": pick, "decode_ms": decodes}
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
