"""A/B on one MI355X: what the diverse (group) beam-search pick costs (include/set_hip.h set_beam_pick_diverse_f32,
evaluate.beam_search_diverse*).
  * the pick alone at V = 9490, ld = 9492, for (k, G) = (6, 3), (8, 4), (8, 2) and NI = 1 / 16 images, one model and the two-model
    ensemble: set_beam_pick_constrained_f32 at the same k and the diverse pick with penalty 0.5, both with neutral constraints,
    in the same run; --calls back-to-back launches between two device events, us per call.  The state is reset before every
    sample (outside the timed window) and <end> is a word no row can pick (logit -inf), so every slot stays alive and every row
    is read at every call.  The diverse pick's two launches are split by the library's own profile scopes (beam_rows*: one
    workgroup per row, the constrained pick's unchanged rows kernel; beam_merge_groups: one wave per image).
  * one whole search of one image: evaluate.beam_search_editnet_batched with k = 2 and a live constraint (the per-step path a
    group of beam_search_diverse(beam_size=6, groups=3) is) against beam_search_diverse(beam_size=6, groups=3), ms per call.
The arms alternate sample by sample; 3 rounds of 20, the spread between round medians reported.  Ratios only: nothing here
has a threshold.  One JSON line, also written to --out.

    python tools/bench_beam_diverse.py [--iters 20] [--rounds 3] [--calls 100] [--out profiles/beam_diverse_bench.json]
"""
import argparse, ctypes as C, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from tools.bench_gumbel_sampling import rounds_of, summary

KGS, NIS = ((6, 3), (8, 4), (8, 2)), (1, 16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20); ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from show_edit_tell_amd import _lib as L, editnet_rl, evaluate, synth
    lib = L.load()
    dev = torch.device("cuda", 0)
    V, ld, Lmax, cur = 9490, 9492, 20, 12
    st = L.stream_of(dev)

    def timed(body, before):
        def fn():
            before()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                body()
            e1.record()
            e1.synchronize()
            return 1e3 * e0.elapsed_time(e1) / a.calls                              # us per call
        return fn

    pick = {}
    neutral = L.BeamConstraintsC(0, 0, 0.0, 0, None)
    for NI in NIS:
        for k, G in KGS:
            B = NI * k
            g = torch.Generator(device="cpu").manual_seed(5)
            bufs = []
            for _ in range(2):
                buf = torch.zeros(B, ld)
                buf[:, :V] = torch.randn(B, V, generator=g) * 2.0
                buf[:, V - 1] = float("-inf")                                        # <end>: a word no row can pick
                bufs.append(buf.to(dev))
            scores = torch.zeros(NI, k, device=dev)
            k_left = torch.full((NI,), k, dtype=torch.int32, device=dev)
            hist = torch.randint(3, 40, (NI, k, Lmax), generator=g).to(dev)          # few distinct words: trigrams repeat
            seqs = [hist.clone(), hist.clone()]
            bs, bq, bl = torch.zeros(NI, device=dev), torch.zeros(NI, Lmax, dtype=torch.long, device=dev), torch.zeros(NI, dtype=torch.int32, device=dev)
            ds, dq = torch.zeros(NI, k, device=dev), torch.zeros(NI, k, Lmax, dtype=torch.long, device=dev)
            dl, nd = torch.zeros(NI, k, dtype=torch.int32, device=dev), torch.zeros(NI, dtype=torch.int32, device=dev)
            words, rows = torch.zeros(B, dtype=torch.long, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
            dg = torch.zeros(NI, k, dtype=torch.int32, device=dev)
            g_left = torch.full((NI, G), k // G, dtype=torch.int32, device=dev)
            ws = torch.empty(lib.set_beam_pick_diverse_workspace_bytes(NI, k), dtype=torch.uint8, device=dev)

            def reset():
                scores.copy_(-torch.arange(k, dtype=torch.float32, device=dev).repeat(NI, 1))

            def arms_of(second):
                head = (L.ptr(bufs[0]), L.ptr(bufs[1]) if second else None, ld, NI, k, V, V - 1, cur, Lmax, L.ptr(scores), L.ptr(k_left),
                        L.ptr(seqs[0]), L.ptr(seqs[1]), L.ptr(bs), L.ptr(bq), L.ptr(bl), L.ptr(words), L.ptr(rows))
                done = (L.ptr(ds), L.ptr(dq), L.ptr(dl), L.ptr(nd))

                def cons():
                    L.check(lib.set_beam_pick_constrained_f32(*head, *done, C.byref(neutral), L.ptr(ws), ws.numel(), st))

                def div():
                    L.check(lib.set_beam_pick_diverse_f32(*head, *done, L.ptr(dg), L.ptr(g_left), G, 0.5, C.byref(neutral), L.ptr(ws),
                                                          ws.numel(), st))
                return {"constrained": timed(cons, reset), "diverse": timed(div, reset)}, div

            for name, second in (("one_model", False), ("ensemble", True)):
                arms, run_diverse = arms_of(second)
                for fn in arms.values():
                    fn()
                s = summary(rounds_of(arms, a.rounds, a.iters), 2)
                reset()
                lib.set_profile_enable(1)
                for _ in range(50):
                    run_diverse()
                torch.cuda.synchronize()
                rep = {r["tag"]: r for r in L.profile_report()}
                lib.set_profile_enable(0)
                ku = {t: round(1e3 * r["ms"] / r["launches"], 2) for t, r in rep.items()
                      if t.startswith("beam_rows") or t == "beam_merge_groups"}
                s["diverse"]["kernel_us"] = ku
                rows_us = sum(v for t, v in ku.items() if t.startswith("beam_rows"))
                s["diverse"]["merge_to_rows"] = round(ku.get("beam_merge_groups", 0.0) / rows_us, 3) if rows_us else None
                s["diverse"]["ratio_to_constrained"] = round(s["diverse"]["median"] / s["constrained"]["median"], 3)
                pick["%s_NI_%d_k_%d_G_%d" % (name, NI, k, G)] = s

    T, D, A, F, R = 18, 1024, 512, 2048, 36
    wm = synth.word_map(V)
    sd = synth.editnet_state(12, V, D, A, F, emb_scale=3.0, fc_scale=8.0, gain=3.0)
    sd["caption_encoder.embed.embedding.weight"] = sd["embed.embedding.weight"]
    dec = editnet_rl.DecoderC(wm, D, D, D, A, F)
    dec.load_state_dict({n: torch.from_numpy(v) for n, v in sd.items()})
    dec = dec.to(dev).eval()
    prev, plen = (torch.from_numpy(x).to(dev) for x in synth.prev_captions(37, 1, T, V, 5))
    X = torch.from_numpy(synth.features(37, 1, R, F)).to(dev)
    cons = evaluate.BeamConstraints(banned_words=("<pad>",))            # live: the per-step path with the constrained pick

    def call(fn):
        def run():
            torch.cuda.synchronize(); t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return 1e3 * (time.perf_counter() - t)                                  # ms per call
        return run

    arms = {"search_k2_constrained": call(lambda: evaluate.beam_search_editnet_batched(dec, X, prev, plen, wm, 2, max_steps=20, constraints=cons)),
            "search_diverse_k6_G3": call(lambda: evaluate.beam_search_diverse(dec, X, prev, plen, wm, beam_size=6, groups=3,
                                                                            diversity_penalty=0.5, max_steps=20, constraints=cons))}
    for _ in range(3):
        for fn in arms.values():
            fn()
    search = summary(rounds_of(arms, a.rounds, a.iters), 3)
    search["search_diverse_k6_G3"]["ratio_to_one_group_alone"] = round(search["search_diverse_k6_G3"]["median"] / search["search_k2_constrained"]["median"], 3)

    result = {"config": "pick: V=%d ld=%d cur_len=%d, neutral constraints, penalty 0.5, state reset before every sample, every slot alive, us per call, %d calls per sample; "
                        "search: EditNet D=%d A=%d F=%d R=%d T=%d, one image, max_steps=20, per-step path, ms per call; "
                        "%d rounds of %d alternated samples" % (V, ld, cur, a.calls, D, A, F, R, T, a.rounds, a.iters),
              "pick_us": pick, "search_ms": search}
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
