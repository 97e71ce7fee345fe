#!/usr/bin/env python
"""ROUGE-L on the device (writes profiles/rouge_device_bench.json):

  - the score kernel at 5 ... 1280 hypotheses against 5 references each, beside set_bleu_device_score on the same rows and the
    same prepared records in the same run (the library's event pair around each launch, device events around `reps`
    back-to-back calls, one call + synchronise);
  - validation_scores of 5000 captions (device, ids already there) against the pure-Python rouge.RougeL + bleu.Bleu on the
    same ids;
  - one SCST step at B = 64 images x 5 samples with reward="device": the call as it was before rouge_weight existed,
    rouge_weight=0.0 and rouge_weight=0.5, alternating in one process, with the repeat-to-repeat spread of each arm.

    python tools/bench_rouge_device.py [--rounds 7] [--reps 50] [--steps 5] [--out profiles/rouge_device_bench.json]

--scst-plain-only --root DIR: only the step's call without the argument, with the package of another checkout (the parent
commit) — run alternately with this tree's in one session, its medians are what `rouge_weight=0` is compared with.
"""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
import numpy as np
import torch


def med_min(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4), "rounds": len(xs)}


def corpus(rng, n_sets, V):
    return [[[int(w) for w in rng.integers(1, V, int(rng.integers(7, 18)))] + [0] for _ in range(5)] for _ in range(n_sets)]


def hypotheses(rng, gt, N, V, L=20):
    """near-copies of references (so that words match in order), 0-terminated rows of L ids; row b belongs to set b % len(gt)"""
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
    from show_edit_tell_amd import _lib, bleu, rouge
    lib = _lib.load()
    rng = np.random.default_rng(2)
    V = 1000
    gt = corpus(rng, 64, V)
    rsc, bsc, host = rouge.DeviceRougeL(dev), bleu.DeviceBleu(dev), rouge.RougeL()
    refs = bsc.prepare_refs(gt)                                   # one preparation, both kernels
    out = {}

    def kernel_alone(fn, tag):
        lib.set_profile_enable(1)
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        rep = {r["tag"]: r for r in _lib.profile_report()}
        lib.set_profile_enable(0)
        return round(1e3 * rep[tag]["ms"] / rep[tag]["launches"], 3)

    for N in (5, 20, 80, 320, 1280):
        H, so = hypotheses(rng, gt, N, V)
        Hd, sod = torch.from_numpy(H).to(dev), torch.from_numpy(so).to(dev)
        want_st, want_sc = host.score_token_ids(H, so, gt)
        st, got = rsc.score_token_ids(Hd, sod, refs)
        assert np.array_equal(st.cpu().numpy(), want_st)
        res = {"max_abs_err_vs_python_scorer": float(np.abs(got.cpu().numpy() - want_sc).max())}
        for name, tag, fn in (("rouge", "rouge_score", lambda: rsc.score_token_ids(Hd, sod, refs)),
                              ("bleu", "bleu_score", lambda: bsc.score_token_ids(Hd, sod, refs))):
            ev, wall = timed(fn, rounds, reps)
            res[name] = {"us_kernel_event_pair_around_the_launch": kernel_alone(fn, tag),
                         "us_per_call_back_to_back_events": med_min(ev), "us_one_call_and_synchronise_host_clock": med_min(wall)}
        out["score_N=%d" % N] = res
    return out


def validation_times(dev, rounds):
    from show_edit_tell_amd import bleu, evaluate, rouge
    rng = np.random.default_rng(3)
    V, N = 1000, 5000
    gt = corpus(rng, N, V)
    H, _ = hypotheses(rng, gt, N, V)
    Hd = torch.from_numpy(H).to(dev)
    hb, hr = bleu.Bleu(), rouge.RougeL()
    lens = [int(np.flatnonzero(r == 0)[0]) for r in H]
    stripped = bleu.strip_end(gt)

    def on_host():
        ids = Hd.cpu().numpy()
        b = hb.corpus_from_stats(hb.score_token_ids(ids, np.arange(N), stripped, hyp_lens=lens)[0])
        return list(b) + [float(hr.score_token_ids(ids, np.arange(N), stripped, hyp_lens=lens)[1].mean())]

    def on_device():
        return evaluate.validation_scores(Hd, None, gt, dev)
    want = on_host()
    d = on_device()
    got = [float(d[k]) for k in ("Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4", "ROUGE_L")]
    res = {"captions": N, "bleu_1_4_rouge_l": [round(x, 6) for x in got],
           "max_abs_err_vs_python_scorers": float(np.abs(np.array(got) - np.array(want)).max())}
    for name, fn, n in (("python_Bleu_and_RougeL_ms_host_clock", on_host, 3),
                        ("validation_scores_ms_host_clock_prepare_two_scores_reduce", on_device, rounds * 3),
                        ("validation_bleu_alone_ms_host_clock", lambda: evaluate.validation_bleu(Hd, None, gt, dev), rounds * 3),
                        ("validation_rouge_l_alone_ms_host_clock", lambda: evaluate.validation_rouge_l(Hd, None, gt, dev), rounds * 3)):
        wall = []
        for _ in range(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
            wall.append(1e3 * (time.perf_counter() - t0))
        res[name] = med_min(wall)
    return res


def scst_times(dev, steps, rounds, plain_only=False):
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
    arms = {"call_without_rouge_weight": {}}
    if not plain_only:
        arms.update({"rouge_weight_0": {"rouge_weight": 0.0}, "rouge_weight_0.5": {"rouge_weight": 0.5}})
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
        base = ms["call_without_rouge_weight"]
        res["spread_of_the_call_without_rouge_weight_ms_max_minus_min"] = round(max(base) - min(base), 4)
        if not plain_only:
            res["rouge_weight_0_minus_call_without_ms_median"] = round(statistics.median(ms["rouge_weight_0"]) - statistics.median(base), 4)
            res["rouge_weight_0.5_minus_call_without_ms_median"] = round(statistics.median(ms["rouge_weight_0.5"]) - statistics.median(base), 4)
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
    ap.add_argument("--scst-plain-only", action="store_true", help="only the SCST step's call without rouge_weight")
    ap.add_argument("--root", default=HERE, help="the checkout whose package is measured (default: this one)")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "rouge_device_bench.json"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    assert torch.cuda.is_available(), "this benchmark measures the GPU: there is no CPU fallback"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if a.scst_plain_only:
        res = {"root": os.path.abspath(a.root), "scst_step_B64_x5_samples_reward_device": scst_times(dev, a.steps, a.rounds, True)}
    else:
        res = {"how": "python tools/bench_rouge_device.py --rounds %d --reps %d --steps %d on one MI355X.  us_kernel...: the mean of "
                      "one event pair around each of `reps` launches (the kernel and ~1-2 us of event cost); us_per_call_back_to_back: "
                      "device events around `reps` Python calls, which is the host's enqueue rate (tensor allocation + ctypes) when "
                      "that is slower than the kernel; host clocks end in a synchronise; median, minimum and maximum over the rounds.  "
                      "rouge / bleu: set_rouge_device_score and set_bleu_device_score on the same rows and records in the same run.  "
                      "SCST: the three arms alternate in one process; `call_without_rouge_weight` is the call the step's users made "
                      "before the argument existed, its max - min over the rounds is the repeat-to-repeat spread the other arms are "
                      "read against" % (a.rounds, a.reps, a.steps),
               "shapes": "64 sets x 5 references of 8..18 ids, hypotheses of <= 20 ids (L = 20), vocabulary 1000; row b belongs to set "
                         "b % 64; validation: 5000 captions, each with its own 5 references",
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
