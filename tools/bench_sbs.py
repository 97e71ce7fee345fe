"""A/B on one MI355X: what stochastic beam search costs (include/set_hip.h set_sbs_pick_f32, evaluate.sample_captions_distinct).
  * the pick alone at V = 9490 for k = 3 / 5 / 8 slots and NI = 1 / 16 images: set_sbs_pick_f32 on logits with ld 9492 (the
    register path, what sample_captions_distinct gives it) and on the same logits with ld 9490 (the scalar path), against
    set_beam_pick_f32 and against ONE model step (set_editnet_step) at the same NI k rows; --calls back-to-back launches
    between two device events, us per call.  The slot state is reset before every sample (outside the timed window) and <end>
    is a word no row can draw (logit -inf), so every slot stays open and every row is read at every call; within a sample phi
    and G drift and len saturates at Lmax, which changes no work.  The pick's two launches are split by the library's own
    profile scopes (sbs_rows / sbs_rows_scalar: one workgroup per row; sbs_merge: one wave per image).
  * evaluate.sample_captions_distinct(n_samples=5) of one image against evaluate.sample_captions(n_samples=5, sampler="cdf"),
    ms per call.
The arms alternate sample by sample; 3 rounds of 20, the spread between round medians reported.  One JSON line, also written to
--out.

    python tools/bench_sbs.py [--iters 20] [--rounds 3] [--calls 100] [--out profiles/sbs_bench.json]
"""
import argparse, ctypes as C, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from tools.bench_gumbel_sampling import rounds_of, summary

KS, NIS = (3, 5, 8), (1, 16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20); ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    from show_edit_tell_amd import _lib as L, editnet_rl, evaluate, synth
    lib = L.load()
    dev = torch.device("cuda", 0)
    V, ld, Lmax = 9490, 9492, 20
    T, D, A, F, R = 18, 1024, 512, 2048, 36
    wm = synth.word_map(V)
    sd = synth.editnet_state(12, V, D, A, F, emb_scale=3.0, fc_scale=8.0, gain=3.0)
    sd["caption_encoder.embed.embedding.weight"] = sd["embed.embedding.weight"]
    dec = editnet_rl.DecoderC(wm, D, D, D, A, F)
    dec.load_state_dict({n: torch.from_numpy(v) for n, v in sd.items()})
    dec = dec.to(dev).eval()
    st = L.stream_of(dev)

    def timed(body, before=None):
        def fn():
            if before is not None:
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
    for NI in NIS:
        prev, plen = (torch.from_numpy(x).to(dev) for x in synth.prev_captions(37, NI, T, V, 5))
        X = torch.from_numpy(synth.features(37, NI, R, F)).to(dev)
        with torch.no_grad():
            for _ in range(2):                                                       # (the token table exists from the second call on)
                dec(wm, prev, plen, X, True, False)
        for k in KS:
            B = NI * k
            g = torch.Generator(device="cpu").manual_seed(5)
            buf = torch.zeros(B, ld)
            buf[:, :V] = torch.randn(B, V, generator=g) * 2.0
            buf[:, V - 1] = float("-inf")                                            # <end>: a word no row can draw
            buf = buf.to(dev)
            flat = buf[:, :V].contiguous()                                           # ld = V = 9490: the scalar path
            # the stochastic pick: every slot live and open, so every row is read at every call
            phi = torch.zeros(NI, k, device=dev)
            G = -torch.arange(k, dtype=torch.float32, device=dev).repeat(NI, 1).contiguous()
            fin, length = torch.zeros(NI, k, dtype=torch.int32, device=dev), torch.zeros(NI, k, dtype=torch.int32, device=dev)
            n_open = torch.full((NI,), k, dtype=torch.int32, device=dev)
            seqs = [torch.zeros(NI, k, Lmax, dtype=torch.long, device=dev) for _ in range(2)]
            words, rows = torch.zeros(B, dtype=torch.long, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
            ws = torch.empty(lib.set_sbs_workspace_bytes(NI, k), dtype=torch.uint8, device=dev)
            sa = L.SbsArgs(logits=buf.data_ptr(), ld=ld, end_idx=V - 1, seed=7, offset=3, phi=phi.data_ptr(), G=G.data_ptr(),
                           finished=fin.data_ptr(), len=length.data_ptr(), seqs_in=seqs[0].data_ptr(), seqs_out=seqs[1].data_ptr(),
                           words=words.data_ptr(), rows=rows.data_ptr(), n_open=n_open.data_ptr(), ws=ws.data_ptr(),
                           ws_bytes=ws.numel(), NI=NI, k=k, V=V, t=1, Lmax=Lmax)

            def sbs():
                sa.logits, sa.ld = buf.data_ptr(), ld
                L.check(lib.set_sbs_pick_f32(C.byref(sa), None, st))

            def sbs_scalar():
                sa.logits, sa.ld = flat.data_ptr(), V
                L.check(lib.set_sbs_pick_f32(C.byref(sa), None, st))

            # the deterministic beam pick on the same logits: k_left stays k as long as no hypothesis emits <end> (V: no word)
            scores = torch.zeros(NI, k, device=dev)
            k_left = torch.full((NI,), k, dtype=torch.int32, device=dev)
            bs, bq, bl = torch.zeros(NI, device=dev), torch.zeros(NI, Lmax, dtype=torch.long, device=dev), torch.zeros(NI, dtype=torch.int32, device=dev)

            def beam():
                L.check(lib.set_beam_pick_f32(L.ptr(buf), None, ld, NI, k, V, V, 1, Lmax, L.ptr(scores), L.ptr(k_left), L.ptr(seqs[0]),
                                              L.ptr(seqs[1]), L.ptr(bs), L.ptr(bq), L.ptr(bl), L.ptr(words), L.ptr(rows), st))

            m = evaluate._FusedModel(dec, (X, None, prev, plen), (X,), k, Lmax)
            step_words = torch.full((B,), int(wm["<start>"]), dtype=torch.long, device=dev)
            step_logits = torch.empty(B, V, device=dev)

            def step():
                m.step(step_words, step_logits)

            def reset():
                phi.zero_(); length.zero_(); scores.zero_()
                G.copy_(-torch.arange(k, dtype=torch.float32, device=dev).repeat(NI, 1))

            arms = {"sbs_pick": timed(sbs, reset), "sbs_pick_scalar": timed(sbs_scalar, reset), "beam_pick": timed(beam, reset),
                    "model_step": timed(step)}
            for fn in arms.values():
                fn()
            s = summary(rounds_of(arms, a.rounds, a.iters), 2)
            reset()
            lib.set_profile_enable(1)
            for _ in range(50):
                sbs()
            for _ in range(50):
                sbs_scalar()
            torch.cuda.synchronize()
            rep = {r["tag"]: r for r in L.profile_report()}
            lib.set_profile_enable(0)
            s["sbs_pick"]["kernel_us"] = {t: round(1e3 * rep[t]["ms"] / rep[t]["launches"], 2) for t in ("sbs_rows", "sbs_rows_scalar", "sbs_merge") if t in rep}
            s["sbs_pick"]["ratio_to_beam_pick"] = round(s["sbs_pick"]["median"] / s["beam_pick"]["median"], 3)
            s["sbs_pick_scalar"]["ratio_to_register_path"] = round(s["sbs_pick_scalar"]["median"] / s["sbs_pick"]["median"], 3)
            s["sbs_pick"]["ratio_to_model_step"] = round(s["sbs_pick"]["median"] / s["model_step"]["median"], 3)
            pick["NI_%d_k_%d" % (NI, k)] = s

    prev, plen = (torch.from_numpy(x).to(dev) for x in synth.prev_captions(37, 1, T, V, 5))
    X = torch.from_numpy(synth.features(37, 1, R, F)).to(dev)

    def call(fn):
        def run():
            torch.cuda.synchronize(); t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return 1e3 * (time.perf_counter() - t)                                  # ms per call
        return run

    arms = {"sample_captions_cdf": call(lambda: evaluate.sample_captions(dec, X, prev, plen, wm, n_samples=5, sampler="cdf")),
            "sample_captions_distinct": call(lambda: evaluate.sample_captions_distinct(dec, X, prev, plen, wm, n_samples=5))}
    for _ in range(3):
        for fn in arms.values():
            fn()
    cap = summary(rounds_of(arms, a.rounds, a.iters), 3)
    cap["sample_captions_distinct"]["ratio_to_cdf"] = round(cap["sample_captions_distinct"]["median"] / cap["sample_captions_cdf"]["median"], 3)
    out = evaluate.sample_captions_distinct(dec, X, prev, plen, wm, n_samples=5)
    cap["sample_captions_distinct"]["distinct"] = len({tuple(e[0]) for e in out[0]})
    seq, _ = evaluate.sample_captions(dec, X, prev, plen, wm, n_samples=5)
    cap["sample_captions_cdf"]["distinct"] = len({tuple(r) for r in seq[0].cpu().tolist()})

    result = {"config": "EditNet D=%d A=%d F=%d R=%d T=%d V=%d; pick: ld=%d (scalar arm: ld=V), t=1, state reset before every sample, every slot open, us per call, %d calls per sample; "
                        "captions: one image, 5 samples, %d words, ms per call; %d rounds of %d alternated samples"
                        % (D, A, F, R, T, V, ld, a.calls, dec.max_len, a.rounds, a.iters),
              "pick_us": pick, "captions_ms": cap}
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
