#!/usr/bin/env python
"""Beam search over ADAPTIVE features (10-100 valid regions zero padded to R=100, an image mean per image) at full
dimensions, k=3, on one MI355X:
  * the batched search over NI images at once (evaluate.beam_search_adaptive_batched, per-step fused kernels);
  * one image per call (evaluate.beam_search_adaptive, the reference's convention): the persistent launch vs the per-step
    path on the same images, switched with SET_DEC_PERSISTENT (read on every call) and alternated image by image;
  * for reference, the fixed-feature persistent one-image search (R=36) from the same run.
One JSON line.  Kernel statistics: run it under `rocprofv3 --kernel-trace --stats -d <dir> -o run --` in a separate run.

    python tools/bench_adaptive_beam.py [--images 64] [--per-image 16] [--rounds 3] [--boost 2.0] [--n-best N]
"""
import argparse, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64); ap.add_argument("--per-image", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=3); ap.add_argument("--beam", type=int, default=3)
    ap.add_argument("--boost", type=float, default=2.0, help="fc.bias[<end>] raise: multi-word searches")
    ap.add_argument("--n-best", type=int, default=0, help="time the adaptive searches with n_best=N (0: off, the default)")
    a = ap.parse_args()
    from show_edit_tell_amd import editnet, editnet_adaptive, evaluate, synth
    dev = torch.device("cuda", 0)
    NI, R, F, T, V, D, A, k = a.images, 100, 2048, 20, 10000, 1024, 512, a.beam
    wm = synth.word_map(V)
    sd = synth.editnet_state(16, V, D, A, F, emb_scale=3.0, fc_scale=8.0, gain=3.0)
    sd["fc.bias"] = sd["fc.bias"].copy(); sd["fc.bias"][wm["<end>"]] += a.boost
    sd["caption_encoder.embed.embedding.weight"] = sd["embed.embedding.weight"]
    state = {n: torch.from_numpy(v) for n, v in sd.items()}
    dec = editnet_adaptive.DecoderC(wm, D, D, D, A, F); dec.load_state_dict(state); dec = dec.to(dev).eval()
    fixed = editnet.DecoderC(wm, D, D, D, A, F); fixed.load_state_dict(state); fixed = fixed.to(dev).eval()
    Xn, mean_n, nvalid = synth.adaptive_features(35, NI, R, F, 10)
    X, mean = torch.from_numpy(Xn).to(dev), torch.from_numpy(mean_n).to(dev)
    prev, plen = (torch.from_numpy(x).to(dev) for x in synth.prev_captions(35, NI, T, V, 5))
    X36 = torch.from_numpy(synth.features(35, NI, 36, F)).to(dev)

    kw = {"n_best": a.n_best} if a.n_best else {}              # (the results gain the n-best lists as one more element)

    def timed(fn):
        torch.cuda.synchronize(); t = time.perf_counter(); out = fn(); torch.cuda.synchronize()
        return time.perf_counter() - t, out

    # ---- batched search over NI images
    evaluate.beam_search_adaptive_batched(dec, X, mean, prev, plen, wm, k)                         # warm-up
    t_b = [timed(lambda: evaluate.beam_search_adaptive_batched(dec, X, mean, prev, plen, wm, k, return_scores=True, **kw))
           for _ in range(a.rounds)]
    seqs_b = t_b[0][1][0]

    # ---- one image per call: persistent vs per-step, alternated on the same images; fixed features for reference
    n1 = min(a.per_image, NI)
    one = lambda b: (X[b:b + 1], mean[b:b + 1], prev[b:b + 1], plen[b:b + 1])
    env0 = os.environ.get("SET_DEC_PERSISTENT")
    per = {"persistent": [], "per_step": [], "fixed_persistent": []}
    lens, agree = [], 0
    try:
        for b in range(n1):                                                                     # warm-up (token table, LDS setup)
            for v in ("1", "0"):
                os.environ["SET_DEC_PERSISTENT"] = v
                evaluate.beam_search_adaptive(dec, *one(b), wm, k)
            os.environ["SET_DEC_PERSISTENT"] = "1"
            evaluate.beam_search_editnet(fixed, X36[b:b + 1], prev[b:b + 1], plen[b:b + 1], wm, k)
        for _ in range(a.rounds):
            for b in range(n1):
                os.environ["SET_DEC_PERSISTENT"] = "1"
                tp, (sp, *_) = timed(lambda: evaluate.beam_search_adaptive(dec, *one(b), wm, k, **kw))
                os.environ["SET_DEC_PERSISTENT"] = "0"
                ts, (ss, *_) = timed(lambda: evaluate.beam_search_adaptive(dec, *one(b), wm, k, **kw))
                os.environ["SET_DEC_PERSISTENT"] = "1"
                tf, _ = timed(lambda: evaluate.beam_search_editnet(fixed, X36[b:b + 1], prev[b:b + 1], plen[b:b + 1], wm, k))
                per["persistent"].append(tp); per["per_step"].append(ts); per["fixed_persistent"].append(tf)
                lens.append(len(sp)); agree += int(sp == ss)
    finally:
        if env0 is None:
            os.environ.pop("SET_DEC_PERSISTENT", None)
        else:
            os.environ["SET_DEC_PERSISTENT"] = env0
    ms = lambda xs: round(1e3 * statistics.median(xs), 3)
    t_pers, t_step = ms(per["persistent"]), ms(per["per_step"])
    print(json.dumps({
        "config": "adaptive features R=%d (valid %d..%d), D=%d, V=%d, k=%d, <end> boost %.1f" % (
            R, int(nvalid.min()), int(nvalid.max()), D, V, k, a.boost),
        "n_best": a.n_best,
        "batched_images": NI, "batched_ms": round(1e3 * min(t for t, _ in t_b), 2),
        "batched_ms_per_image": round(1e3 * min(t for t, _ in t_b) / NI, 3),
        "batched_mean_tokens": round(sum(len(s) for s in seqs_b) / NI, 2),
        "one_image_images": n1, "one_image_rounds": a.rounds,
        "one_image_persistent_ms_median": t_pers, "one_image_per_step_ms_median": t_step,
        "one_image_persistent_over_per_step": round(t_pers / t_step, 3),
        "one_image_persistent_min_ms": round(1e3 * min(per["persistent"]), 3),
        "one_image_per_step_min_ms": round(1e3 * min(per["per_step"]), 3),
        "one_image_mean_tokens": round(sum(lens) / len(lens), 2),
        "one_image_same_tokens": "%d/%d" % (agree, len(lens)),
        "fixed_features_R36_persistent_ms_median": ms(per["fixed_persistent"]),
    }))


if __name__ == "__main__":
    main()
