"""A/B on one MI355X: what the EditNet + DCNet ensemble costs in stochastic beam search (include/set_hip.h
set_sbs_pick_ensemble_f32, evaluate.sample_captions_distinct_ensemble).
  * the pick alone at V = 9490 for k = 3 / 5 / 8 slots and NI = 1 / 16 images: set_sbs_pick_ensemble_f32 on two logits buffers
    with ld 9492 (the register path, both rows held) against set_sbs_pick_f32 on the first of them, and both on ld = V = 9490
    (the scalar path).  The state is reset before every sample so that every slot is live and open; kernel times come from the
    library's profile scopes (sbs_rows_ens / sbs_rows_ens_scalar / sbs_rows / sbs_rows_scalar, sbs_merge).
  * five distinct ensemble captions of ONE image (evaluate.sample_captions_distinct_ensemble, n_samples = 5) against
    evaluate.beam_search_ensemble_batched at k = 5 over the same image, host time per call with a device synchronisation.
Arms alternate inside a round (tools/bench_gumbel_sampling.rounds_of); reported: the median of the round medians and their
spread.

    python tools/bench_sbs_ensemble.py [--iters 20] [--rounds 3] [--calls 100] [--out profiles/sbs_ensemble_bench.json]
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
    from show_edit_tell_amd import _lib as L, dcnet_rl, editnet_rl, evaluate, synth
    lib = L.load()
    dev = torch.device("cuda", 0)
    V, ld, Lmax = 9490, 9492, 20
    T, D, A, F, R, Cd, Ed = 18, 1024, 512, 2048, 36, 512, 1024
    wm = synth.word_map(V)
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
        for k in KS:
            B = NI * k
            g = torch.Generator(device="cpu").manual_seed(5)
            bufs, flats = [], []
            for _ in range(2):
                buf = torch.zeros(B, ld)
                buf[:, :V] = torch.randn(B, V, generator=g) * 2.0
                buf[:, V - 1] = float("-inf")                                        # <end>: a word no row can draw
                buf = buf.to(dev)
                bufs.append(buf)
                flats.append(buf[:, :V].contiguous())                                # ld = V = 9490: the scalar path
            phi = torch.zeros(NI, k, device=dev)
            G = -torch.arange(k, dtype=torch.float32, device=dev).repeat(NI, 1).contiguous()
            fin, length = torch.zeros(NI, k, dtype=torch.int32, device=dev), torch.zeros(NI, k, dtype=torch.int32, device=dev)
            n_open = torch.full((NI,), k, dtype=torch.int32, device=dev)
            seqs = [torch.zeros(NI, k, Lmax, dtype=torch.long, device=dev) for _ in range(2)]
            words, rows = torch.zeros(B, dtype=torch.long, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
            ws = torch.empty(lib.set_sbs_workspace_bytes(NI, k), dtype=torch.uint8, device=dev)
            sa = L.SbsArgs(logits=bufs[0].data_ptr(), ld=ld, end_idx=V - 1, seed=7, offset=3, phi=phi.data_ptr(), G=G.data_ptr(),
                           finished=fin.data_ptr(), len=length.data_ptr(), seqs_in=seqs[0].data_ptr(), seqs_out=seqs[1].data_ptr(),
                           words=words.data_ptr(), rows=rows.data_ptr(), n_open=n_open.data_ptr(), ws=ws.data_ptr(),
                           ws_bytes=ws.numel(), NI=NI, k=k, V=V, t=1, Lmax=Lmax)

            def arm(two, src, lead):
                def body():
                    sa.logits, sa.ld = src[0].data_ptr(), lead
                    if two:
                        L.check(lib.set_sbs_pick_ensemble_f32(C.byref(sa), src[1].data_ptr(), None, st))
                    else:
                        L.check(lib.set_sbs_pick_f32(C.byref(sa), None, st))
                return body

            def reset():
                phi.zero_(); length.zero_()
                G.copy_(-torch.arange(k, dtype=torch.float32, device=dev).repeat(NI, 1))

            bodies = {"ensemble_pick": arm(True, bufs, ld), "one_model_pick": arm(False, bufs, ld),
                      "ensemble_pick_scalar": arm(True, flats, V), "one_model_pick_scalar": arm(False, flats, V)}
            arms = {n: timed(b, reset) for n, b in bodies.items()}
            for fn in arms.values():
                fn()
            s = summary(rounds_of(arms, a.rounds, a.iters), 2)
            reset()
            lib.set_profile_enable(1)
            for b in bodies.values():
                for _ in range(50):
                    b()
            torch.cuda.synchronize()
            rep = {r["tag"]: r for r in L.profile_report()}
            lib.set_profile_enable(0)
            s["kernel_us"] = {t: round(1e3 * rep[t]["ms"] / rep[t]["launches"], 2)
                              for t in ("sbs_rows_ens", "sbs_rows_ens_scalar", "sbs_rows", "sbs_rows_scalar", "sbs_merge") if t in rep}
            s["ensemble_pick"]["ratio_to_one_model"] = round(s["ensemble_pick"]["median"] / s["one_model_pick"]["median"], 3)
            s["ensemble_pick_scalar"]["ratio_to_one_model"] = round(s["ensemble_pick_scalar"]["median"] / s["one_model_pick_scalar"]["median"], 3)
            s["ensemble_pick_scalar"]["ratio_to_register_path"] = round(s["ensemble_pick_scalar"]["median"] / s["ensemble_pick"]["median"], 3)
            pick["NI_%d_k_%d" % (NI, k)] = s

    sd = synth.editnet_state(12, V, D, A, F, emb_scale=3.0, fc_scale=8.0, gain=3.0)
    sd["caption_encoder.embed.embedding.weight"] = sd["embed.embedding.weight"]
    dec = editnet_rl.DecoderC(wm, D, D, D, A, F)
    dec.load_state_dict({n: torch.from_numpy(v) for n, v in sd.items()})
    dec = dec.to(dev).eval()
    sdd = synth.dcnet_state(13, V, D, A, Cd, Ed, 3.0, 8.0, 3.0)
    sdd["caption_encoder.embed.embedding.weight"] = sdd["embed.embedding.weight"]
    dae = dcnet_rl.DAE(wm, None, D, A, Cd, Ed)
    dae.load_state_dict({n: torch.from_numpy(v) for n, v in sdd.items()})
    dae = dae.to(dev).eval()
    prev, plen = (torch.from_numpy(x).to(dev) for x in synth.prev_captions(37, 1, T, V, 5))
    X = torch.from_numpy(synth.features(37, 1, R, F)).to(dev)
    with torch.no_grad():
        for _ in range(2):                                                           # (the token tables exist from the second call on)
            dec(wm, prev, plen, X, True, False)
            dae(wm, prev, plen, True, False)

    def call(fn):
        def run():
            torch.cuda.synchronize(); t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return 1e3 * (time.perf_counter() - t)                                  # ms per call
        return run

    steps = dec.max_len
    arms = {"beam_search_ensemble_batched_k5": call(lambda: evaluate.beam_search_ensemble_batched(dec, dae, X, prev, plen, wm, 5, max_steps=steps)),
            "sample_captions_distinct_ensemble": call(lambda: evaluate.sample_captions_distinct_ensemble(dec, dae, X, prev, plen, wm, n_samples=5)),
            "sample_captions_distinct_editnet": call(lambda: evaluate.sample_captions_distinct(dec, X, prev, plen, wm, n_samples=5))}
    for _ in range(3):
        for fn in arms.values():
            fn()
    cap = summary(rounds_of(arms, a.rounds, a.iters), 3)
    cap["sample_captions_distinct_ensemble"]["ratio_to_beam"] = round(
        cap["sample_captions_distinct_ensemble"]["median"] / cap["beam_search_ensemble_batched_k5"]["median"], 3)
    cap["sample_captions_distinct_ensemble"]["ratio_to_one_model"] = round(
        cap["sample_captions_distinct_ensemble"]["median"] / cap["sample_captions_distinct_editnet"]["median"], 3)
    out = evaluate.sample_captions_distinct_ensemble(dec, dae, X, prev, plen, wm, n_samples=5)
    cap["sample_captions_distinct_ensemble"]["distinct"] = len({tuple(e[0]) for e in out[0]})

    result = {"config": "EditNet D=%d A=%d F=%d R=%d + DCNet C=%d E=%d, T=%d V=%d; pick: ld=%d (scalar arms: ld=V), t=1, state reset before every "
                        "sample, every slot open, us per call, %d calls per sample; captions: one image, 5 samples / beam 5, at most %d "
                        "steps, ms per call; %d rounds of %d alternated samples"
                        % (D, A, F, R, Cd, Ed, T, V, ld, a.calls, steps, a.rounds, a.iters),
              "pick_us": pick, "captions_ms": cap}
    print(json.dumps(result))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
