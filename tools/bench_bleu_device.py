#!/usr/bin/env python
"""BLEU on the device (writes profiles/bleu_device_bench.json):

  - the score kernel at 5 / 320 / 1280 hypotheses against 5 references each and the preparation launch for 320 references
    (the library's event pair around each launch, device events around `reps` back-to-back calls, one call + synchronise);
  - validation_bleu of 5000 captions (device, ids already there) against the pure-Python bleu.Bleu on the same ids;
  - one SCST step at B = 64 images x 5 samples with reward="device": the call as it was before bleu_weight existed,
    bleu_weight=0.0 and bleu_weight=0.5, alternating in one process, with the repeat-to-repeat spread of each arm.

    python tools/bench_bleu_device.py [--rounds 7] [--reps 50] [--steps 5] [--out profiles/bleu_device_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch


def med_min(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4), "rounds": len(xs)}


def corpus(rng, n_sets, V):
    return [[[int(w) for w in rng.integers(1, V, int(rng.integers(7, 18)))] + [0] for _ in range(5)] for _ in range(n_sets)]


def hypotheses(rng, gt, N, V, L=20):
    """near-copies of references (so that grams match), 0-terminated rows of L ids; row b belongs to set b % len(gt)"""
    H = np.zeros((N, L), dtype=np.int64)
    for b in range(N):
        c = [w for w in gt[b % len(gt)][int(rng.integers(0, 5))] if w][:L - 1]
        for _ in range(3):
            c[int(rng.integers(0, len(c)))] = int(rng.integers(1, V))
        H[b, :len(c)] = c
    return H, (np.arange(N) % len(gt)).astype(np.int32)


def timed(fn, rounds, reps):
    fn(); torch.cuda.synchronize()
    ev, wall = [], []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record(); torch.cuda.synchronize()
        ev.append(1e3 * e0.elapsed_time(e1) / reps)
        t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
        wall.append(1e6 * (time.perf_counter() - t0))
    return ev, wall


def kernel_times(dev, rounds, reps):
    from show_edit_tell_amd import _lib, bleu
    lib = _lib.load()
    rng = np.random.default_rng(2)
    V = 1000
    gt = corpus(rng, 64, V)
    sc, host = bleu.DeviceBleu(dev), bleu.Bleu()
    refs = sc.prepare_refs(gt)
    ref_tok = torch.zeros(320, refs.L, dtype=torch.int64, device=dev)
    out = {}

    def kernel_alone(fn, tag):
        lib.set_profile_enable(1)
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        rep = {r["tag"]: r for r in _lib.profile_report()}
        lib.set_profile_enable(0)
        return round(1e3 * rep[tag]["ms"] / rep[tag]["launches"], 3)

    prep = lambda: sc._prepare(ref_tok, None)
    ev, wall = timed(prep, rounds, reps)
    out["prepare_320_refs"] = {"us_kernel_event_pair_around_the_launch": kernel_alone(prep, "bleu_prepare"),
                               "us_per_call_back_to_back_events": med_min(ev), "us_one_call_and_synchronise_host_clock": med_min(wall)}
    for N in (5, 320, 1280):
        H, so = hypotheses(rng, gt, N, V)
        Hd, sod = torch.from_numpy(H).to(dev), torch.from_numpy(so).to(dev)
        want_st, want_sc = host.score_token_ids(H, so, gt)
        st, got = sc.score_token_ids(Hd, sod, refs)
        assert np.array_equal(st.cpu().numpy(), want_st)
        fn = lambda: sc.score_token_ids(Hd, sod, refs)
        ev, wall = timed(fn, rounds, reps)
        out["score_N=%d" % N] = {"max_abs_err_vs_python_scorer": float(np.abs(got.cpu().numpy() - want_sc).max()),
                                 "us_kernel_event_pair_around_the_launch": kernel_alone(fn, "bleu_score"),
                                 "us_per_call_back_to_back_events": med_min(ev), "us_one_call_and_synchronise_host_clock": med_min(wall)}
    return out


def validation_times(dev, rounds):
    from show_edit_tell_amd import bleu, evaluate
    rng = np.random.default_rng(3)
    V, N = 1000, 5000
    gt = corpus(rng, N, V)
    H, _ = hypotheses(rng, gt, N, V)
    Hd = torch.from_numpy(H).to(dev)
    host = bleu.Bleu()
    lens = [int(np.flatnonzero(r == 0)[0]) for r in H]
    stripped = bleu.strip_end(gt)

    def on_host():
        return host.corpus_from_stats(host.score_token_ids(Hd.cpu().numpy(), np.arange(N), stripped, hyp_lens=lens)[0])

    def on_device():
        return evaluate.validation_bleu(Hd, None, gt, dev)
    want, got = on_host(), on_device().cpu().numpy()
    res = {"captions": N, "bleu_1_4": [round(float(x), 6) for x in got], "max_abs_err_vs_python_scorer": float(np.abs(got - np.array(want)).max())}
    for name, fn, n in (("python_Bleu_ms_host_clock", on_host, 3), ("validation_bleu_ms_host_clock_prepare_score_reduce", on_device, rounds * 3)):
        wall = []
        for _ in range(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
            wall.append(1e3 * (time.perf_counter() - t0))
        res[name] = med_min(wall)
    sc = bleu.device_scorer(dev)
    refs = sc.prepare_refs(gt, count_end=False)
    ld = torch.tensor(lens, dtype=torch.int32, device=dev)
    wall = []
    for _ in range(rounds * 3):
        torch.cuda.synchronize()
        t0 = time.perf_counter(); sc.corpus_score(Hd, torch.arange(N, dtype=torch.int32, device=dev), refs, ld); torch.cuda.synchronize()
        wall.append(1e3 * (time.perf_counter() - t0))
    res["corpus_score_ms_host_clock_references_already_prepared"] = med_min(wall)
    return res


def scst_times(dev, steps, rounds):
    from show_edit_tell_amd import ciderd, dcnet_rl, editnet_rl, synth
    from show_edit_tell_amd.train import dcnet_scst_train_step, scst_train_step
    B, R, F, T, V, D, A = 64, 36, 2048, 20, 10000, 1024, 512
    wm = synth.word_map(V)
    rng = np.random.default_rng(41)
    allcaps = np.zeros((B, 5, 20), dtype=np.int64)
    for b in range(B):
        for j in range(5):
            n = int(rng.integers(6, 17))
            allcaps[b, j, 0] = wm["<start>"]; allcaps[b, j, 1:1 + n] = rng.integers(1, V - 4, n); allcaps[b, j, 1 + n] = wm["<end>"]
    gt = ciderd.ground_truth_lists(allcaps, wm)
    df, docs = ciderd.document_frequency([[ciderd.tokens_to_str(c) for c in caps] for caps in gt])
    scorer = ciderd.CiderD(df, docs)
    prev, plen = (torch.from_numpy(x).to(dev) for x in synth.prev_captions(41, B, T, V, 5))
    arms = {"call_without_bleu_weight": {}, "bleu_weight_0": {"bleu_weight": 0.0}, "bleu_weight_0.5": {"bleu_weight": 0.5}}
    out = {}
    for net in ("editnet", "dcnet"):
        if net == "editnet":
            model = editnet_rl.DecoderC(wm, D, D, D, A, F)
            sd = synth.editnet_state(14, V, D, A, F, emb_scale=3.0, fc_scale=8.0, gain=3.0)
            X = torch.from_numpy(synth.features(41, B, R, F)).to(dev)
        else:
            model = dcnet_rl.DAE(wm, None)
            sd = synth.dcnet_state(18, V, emb_scale=3.0, fc_scale=8.0, gain=3.0)
        sd["caption_encoder.embed.embedding.weight"] = sd["embed.embedding.weight"]
        model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        model = model.to(dev)
        opt = torch.optim.Adam(model.parameters(), lr=5e-5)

        def step(kw):
            if net == "editnet":
                return scst_train_step(model, opt, wm, X, prev, plen, gt, scorer, n_samples=5, reward="device", **kw)
            return dcnet_scst_train_step(model, opt, wm, prev, plen, gt, scorer, n_samples=5, reward="device", **kw)
        for kw in arms.values():
            step(kw)
        torch.cuda.synchronize()
        ms = {a: [] for a in arms}
        for _ in range(rounds):                       # the arms alternate inside one process
            for a, kw in arms.items():
                t0 = time.perf_counter()
                for _ in range(steps):
                    step(kw)
                torch.cuda.synchronize()
                ms[a].append(1e3 * (time.perf_counter() - t0) / steps)
        res = {"ms_per_step_" + a: med_min(v) for a, v in ms.items()}
        base = ms["call_without_bleu_weight"]
        res["spread_of_the_call_without_bleu_weight_ms_max_minus_min"] = round(max(base) - min(base), 4)
        res["bleu_weight_0_minus_call_without_ms_median"] = round(statistics.median(ms["bleu_weight_0"]) - statistics.median(base), 4)
        res["bleu_weight_0.5_minus_call_without_ms_median"] = round(statistics.median(ms["bleu_weight_0.5"]) - statistics.median(base), 4)
        res["steps_per_round"] = steps
        out[net] = res
        del model, opt
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--skip-scst", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "bleu_device_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the GPU: there is no CPU fallback"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res = {"how": "python tools/bench_bleu_device.py --rounds %d --reps %d --steps %d on one MI355X.  us_kernel...: the mean of one "
                  "event pair around each of `reps` launches (the kernel and ~1-2 us of event cost); us_per_call_back_to_back: device "
                  "events around `reps` Python calls, which is the host's enqueue rate (tensor allocation + ctypes) when that is "
                  "slower than the kernel; host clocks end in a synchronise; median, minimum and maximum over the rounds.  SCST: "
                  "the three arms alternate in one process; `call_without_bleu_weight` is the call the step's users made before the "
                  "argument existed (the same statements run as with bleu_weight=0.0), its max - min over the rounds is the "
                  "repeat-to-repeat spread the other arms are read against" % (a.rounds, a.reps, a.steps),
           "shapes": "64 sets x 5 references of 8..18 ids, hypotheses of <= 20 ids (L = 20), vocabulary 1000; row b belongs to set b % 64; "
                     "validation: 5000 captions, each with its own 5 references",
           "kernels": kernel_times(dev, a.rounds, a.reps),
           "validation_5000_captions": validation_times(dev, a.rounds)}
    if not a.skip_scst:
        res["scst_step_B64_x5_samples_reward_device"] = scst_times(dev, a.steps, a.rounds)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
