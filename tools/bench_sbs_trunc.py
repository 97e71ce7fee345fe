"""A/B on one MI355X: what top-k / top-p truncation costs in the stochastic beam search (include/set_hip.h
set_sbs_pick_opts_f32 / set_sbs_pick_ensemble_opts_f32, evaluate.sample_captions_distinct*).
  * the one-model pick at V = 9490 on the padded (register) route, ld 9492, for k = 3 / 5 / 8 slots and NI = 1 / 16 images, under
    neutral options, top_k = 50, top_p = 0.9 and both; --calls back-to-back launches between two device events, us per call.
    The neutral arm of the same run is the yardstick.  State and logits are bench_sbs.py's: every slot live and open, <end> a
    word no row can draw, the state reset before every sample outside the timed window.
  * the ensemble pick (a second set of logits) the same at k = 5;
  * the scalar route (ld = V = 9490), one model and ensemble, the same at k = 5: every descent pass re-reads the row there;
  * evaluate.sample_captions_distinct(n_samples=5) of one image, neutral against top_p = 0.9, and the same for
    sample_captions_distinct_ensemble, ms per call.
The rows launch is split from the merge by the library's profile scopes.  The arms alternate sample by sample; 3 rounds of 20, the
spread between round medians reported.  One JSON line, also written to --out.

    python tools/bench_sbs_trunc.py [--iters 20] [--rounds 3] [--calls 100] [--out profiles/sbs_trunc_bench.json]
"""
import argparse, ctypes as C, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from tools.bench_gumbel_sampling import rounds_of, summary

KS, NIS = (3, 5, 8), (1, 16)
OPTS = {"neutral": (0, 1.0), "top_k_50": (50, 1.0), "top_p_0.9": (0, 0.9), "top_k_50_top_p_0.9": (50, 0.9)}
ROWS_TAGS = ("sbs_rows", "sbs_rows_scalar", "sbs_rows_ens", "sbs_rows_ens_scalar", "sbs_rows_trunc", "sbs_rows_trunc_scalar",
             "sbs_rows_ens_trunc", "sbs_rows_ens_trunc_scalar")


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

    def pick_arms(NI, k, ens, scalar):
        """{option name: timed pick}, the reset and a per-arm single call (for the profile scopes)"""
        B = NI * k
        bufs = []
        for s in (5, 6)[:2 if ens else 1]:
            g = torch.Generator(device="cpu").manual_seed(s)
            buf = torch.zeros(B, ld)
            buf[:, :V] = torch.randn(B, V, generator=g) * 2.0
            buf[:, V - 1] = float("-inf")                                            # <end>: a word no row can draw
            buf = buf.to(dev)
            bufs.append(buf[:, :V].contiguous() if scalar else buf)                  # ld = V = 9490: the scalar path
        phi = torch.zeros(NI, k, device=dev)
        G = -torch.arange(k, dtype=torch.float32, device=dev).repeat(NI, 1).contiguous()
        fin, length = torch.zeros(NI, k, dtype=torch.int32, device=dev), torch.zeros(NI, k, dtype=torch.int32, device=dev)
        n_open = torch.full((NI,), k, dtype=torch.int32, device=dev)
        seqs = [torch.zeros(NI, k, Lmax, dtype=torch.long, device=dev) for _ in range(2)]
        words, rows = torch.zeros(B, dtype=torch.long, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
        ws = torch.empty(lib.set_sbs_workspace_bytes(NI, k), dtype=torch.uint8, device=dev)
        sa = L.SbsArgs(logits=bufs[0].data_ptr(), ld=V if scalar else ld, end_idx=V - 1, seed=7, offset=3, phi=phi.data_ptr(),
                       G=G.data_ptr(), finished=fin.data_ptr(), len=length.data_ptr(), seqs_in=seqs[0].data_ptr(),
                       seqs_out=seqs[1].data_ptr(), words=words.data_ptr(), rows=rows.data_ptr(), n_open=n_open.data_ptr(),
                       ws=ws.data_ptr(), ws_bytes=ws.numel(), NI=NI, k=k, V=V, t=1, Lmax=Lmax)
        keep = (bufs, phi, G, fin, length, n_open, seqs, words, rows, ws)

        def reset():
            phi.zero_(); length.zero_(); fin.zero_(); n_open.fill_(k)
            G.copy_(-torch.arange(k, dtype=torch.float32, device=dev).repeat(NI, 1))

        def body(top_k, top_p):
            o = L.SampleOpts(temperature=1.0, top_k=top_k, top_p=top_p)

            def run(keep=keep):
                if ens:
                    L.check(lib.set_sbs_pick_ensemble_opts_f32(C.byref(sa), bufs[1].data_ptr(), C.byref(o), st))
                else:
                    L.check(lib.set_sbs_pick_opts_f32(C.byref(sa), C.byref(o), st))
            return run

        bodies = {name: body(*tk_tp) for name, tk_tp in OPTS.items()}
        return {name: timed(fn, reset) for name, fn in bodies.items()}, bodies, reset

    def measure(NI, k, ens=False, scalar=False):
        arms, bodies, reset = pick_arms(NI, k, ens, scalar)
        for fn in arms.values():
            fn()
        s = summary(rounds_of(arms, a.rounds, a.iters), 2)
        for name, fn in bodies.items():                                             # the rows launch alone, per arm
            reset()
            lib.set_profile_enable(1)
            for _ in range(50):
                fn()
            torch.cuda.synchronize()
            rep = {r["tag"]: r for r in L.profile_report()}
            lib.set_profile_enable(0)
            s[name]["kernel_us"] = {t: round(1e3 * rep[t]["ms"] / rep[t]["launches"], 2) for t in ROWS_TAGS + ("sbs_merge",) if t in rep}
            s[name]["added_us"] = round(s[name]["median"] - s["neutral"]["median"], 2)
            s[name]["ratio_to_neutral"] = round(s[name]["median"] / s["neutral"]["median"], 3)
        return s

    pick = {"NI_%d_k_%d" % (NI, k): measure(NI, k) for NI in NIS for k in KS}
    ens = {"NI_%d_k_5" % NI: measure(NI, 5, ens=True) for NI in NIS}
    scalar = {"NI_%d_k_5" % NI: measure(NI, 5, scalar=True) for NI in NIS}
    ens_scalar = {"NI_%d_k_5" % NI: measure(NI, 5, ens=True, scalar=True) for NI in NIS}

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

    one = lambda **kw: evaluate.sample_captions_distinct(dec, X, prev, plen, wm, n_samples=5, **kw)
    two = lambda **kw: evaluate.sample_captions_distinct_ensemble(dec, dae, X, prev, plen, wm, n_samples=5, **kw)
    arms = {"distinct_neutral": call(one), "distinct_top_p_0.9": call(lambda: one(top_p=0.9)),
            "distinct_ensemble_neutral": call(two), "distinct_ensemble_top_p_0.9": call(lambda: two(top_p=0.9))}
    for _ in range(3):
        for fn in arms.values():
            fn()
    cap = summary(rounds_of(arms, a.rounds, a.iters), 3)
    for base in ("distinct", "distinct_ensemble"):
        cap[base + "_top_p_0.9"]["ratio_to_neutral"] = round(cap[base + "_top_p_0.9"]["median"] / cap[base + "_neutral"]["median"], 3)
    cap["distinct_top_p_0.9"]["distinct"] = len({tuple(e[0]) for e in one(top_p=0.9)[0]})
    cap["distinct_ensemble_top_p_0.9"]["distinct"] = len({tuple(e[0]) for e in two(top_p=0.9)[0]})

    result = {"config": "pick: V=%d, ld=%d (scalar arms: ld=V), t=1, randn * 2 logits, state reset before every sample, every slot open, us "
                        "per call, %d calls per sample; captions: EditNet D=%d A=%d F=%d R=%d (+ DCNet C=%d E=%d), T=%d, one image, 5 "
                        "samples, %d words, ms per call; %d rounds of %d alternated samples"
                        % (V, ld, a.calls, D, A, F, R, Cd, Ed, T, dec.max_len, a.rounds, a.iters),
              "pick_us": pick, "ensemble_pick_us": ens, "scalar_pick_us": scalar, "ensemble_scalar_pick_us": ens_scalar, "captions_ms": cap}
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
