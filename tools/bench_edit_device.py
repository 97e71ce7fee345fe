#!/usr/bin/env python
"""Word edit distance on the device (writes profiles/edit_device_bench.json):

  - the score kernel at 5 ... 1280 hypotheses against 5 references each, beside set_rouge_device_score on the same rows and
    the same prepared records in the same run, the yardstick (the library's event pair around each launch, device events
    around `reps` back-to-back calls, one call + synchronise);
  - the align kernel at the same row counts: every hypothesis against one reference of its set as the source;
  - validation_edit and edit_statistics of 5000 captions (device, ids already there) against the pure-Python
    editdist.EditDistance on the same ids.

    python tools/bench_edit_device.py [--rounds 7] [--reps 50] [--out profiles/edit_device_bench.json]
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
    from show_edit_tell_amd import _lib, editdist, rouge
    lib = _lib.load()
    rng = np.random.default_rng(2)
    V = 1000
    gt = corpus(rng, 64, V)
    esc, rsc, host = editdist.DeviceEditDistance(dev), rouge.DeviceRougeL(dev), editdist.EditDistance()
    refs = esc.prepare_refs(gt)                                   # one preparation, both score kernels
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
        S = np.zeros_like(H)
        for b in range(N):                                        # the source of row b: the first reference of its set
            c = gt[so[b]][0]
            S[b, :len(c)] = c
        Hd, Sd, sod = torch.from_numpy(H).to(dev), torch.from_numpy(S).to(dev), torch.from_numpy(so).to(dev)
        want_st, want_sc = host.score_token_ids(H, so, gt)
        st, got = esc.score_token_ids(Hd, sod, refs)
        assert np.array_equal(st.cpu().numpy(), want_st)
        want_al = host.align_token_ids(H, S)
        got_al = esc.align_token_ids(Hd, Sd)
        assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(got_al, want_al))
        res = {"max_abs_err_vs_python_scorer": float(np.abs(got.cpu().numpy() - want_sc).max()), "alignment_equals_python_scorer": True}
        for name, tag, fn in (("edit_score", "edit_score", lambda: esc.score_token_ids(Hd, sod, refs)),
                              ("rouge_score", "rouge_score", lambda: rsc.score_token_ids(Hd, sod, refs)),
                              ("edit_align", "edit_align", lambda: esc.align_token_ids(Hd, Sd))):
            ev, wall = timed(fn, rounds, reps)
            res[name] = {"us_kernel_event_pair_around_the_launch": kernel_alone(fn, tag),
                         "us_per_call_back_to_back_events": med_min(ev), "us_one_call_and_synchronise_host_clock": med_min(wall)}
        res["edit_score_over_rouge_score_kernel_time"] = round(
            res["edit_score"]["us_kernel_event_pair_around_the_launch"] / res["rouge_score"]["us_kernel_event_pair_around_the_launch"], 3)
        out["N=%d" % N] = res
    return out


def validation_times(dev, rounds):
    from show_edit_tell_amd import bleu, editdist, evaluate, synth
    rng = np.random.default_rng(3)
    V, N = 1000, 5000
    wm = synth.word_map(V + 4)                                    # the words are 1 .. V, the markers lie above them
    gt = corpus(rng, N, V)
    H, _ = hypotheses(rng, gt, N, V)
    Hd = torch.from_numpy(H).to(dev)
    host = editdist.EditDistance()
    lens = [int(np.flatnonzero(r == 0)[0]) for r in H]
    stripped = bleu.strip_end(gt)
    # the model's input of row b: the first reference of its set, in the vocabulary's convention (<start> ... <end> <pad>)
    prev = np.full((N, 22), wm["<pad>"], dtype=np.int64)
    plen = np.zeros((N, 1), dtype=np.int64)
    for b in range(N):
        c = [wm["<start>"]] + [w for w in gt[b][0] if w] + [wm["<end>"]]
        prev[b, :len(c)], plen[b, 0] = c, len(c)
    assert not ({wm["<start>"], wm["<pad>"], wm["<end>"]} & set(int(w) for w in np.unique(H[H > 0]))), "ids collide with the markers"
    prev_d, plen_d = torch.from_numpy(prev).to(dev), torch.from_numpy(plen).to(dev)
    S = np.zeros((N, 22), dtype=np.int64)
    for b in range(N):
        S[b, :len(stripped[b][0])] = stripped[b][0]
    slens = [len(stripped[b][0]) for b in range(N)]

    def validation_on_host():
        return host.corpus_score(Hd.cpu().numpy(), np.arange(N), stripped, hyp_lens=lens)

    def statistics_on_host():
        st = host.align_token_ids(Hd.cpu().numpy(), S, hyp_lens=lens, src_lens=slens)[0]
        return {"unchanged_frac": float(st[:, 7].mean()), "mean_dist": float(st[:, 0].mean()), "edit_rate": float(st[:, 0].sum() / st[:, 2].sum())}

    want_v, want_s = validation_on_host(), statistics_on_host()
    got_v = {k: float(v) for k, v in evaluate.validation_edit(Hd, None, gt, dev).items()}
    d = evaluate.edit_statistics(prev_d, plen_d, Hd, wm, dev)
    got_s = {k: float(d[k]) for k in want_s}
    res = {"captions": N, "validation_edit": {k: round(v, 6) for k, v in got_v.items()}, "edit_statistics": {k: round(v, 6) for k, v in got_s.items()},
           "max_abs_err_vs_python_scorer": max([abs(got_v[k] - want_v[k]) for k in want_v] + [abs(got_s[k] - want_s[k]) for k in want_s])}
    for name, fn, n in (("python_EditDistance_corpus_score_ms_host_clock", validation_on_host, 3),
                        ("python_EditDistance_align_token_ids_ms_host_clock", statistics_on_host, 3),
                        ("validation_edit_ms_host_clock_prepare_score_reduce", lambda: evaluate.validation_edit(Hd, None, gt, dev), rounds * 3),
                        ("edit_statistics_ms_host_clock_normalise_align_reduce", lambda: evaluate.edit_statistics(prev_d, plen_d, Hd, wm, dev), rounds * 3)):
        wall = []
        for _ in range(n):
            torch.cuda.synchronize()
            t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
            wall.append(1e3 * (time.perf_counter() - t0))
        res[name] = med_min(wall)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "edit_device_bench.json"))
    a = ap.parse_args()
    sys.path.insert(0, HERE)
    assert torch.cuda.is_available(), "this benchmark measures the GPU: there is no CPU fallback"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res = {"how": "python tools/bench_edit_device.py --rounds %d --reps %d on one MI355X.  us_kernel...: the mean of one event pair "
                  "around each of `reps` launches (the kernel and ~1-2 us of event cost); us_per_call_back_to_back: device events "
                  "around `reps` Python calls, which is the host's enqueue rate (tensor allocation + ctypes) when that is slower "
                  "than the kernel; host clocks end in a synchronise; median, minimum and maximum over the rounds.  edit_score / "
                  "rouge_score: set_edit_device_score and set_rouge_device_score on the same rows and records in the same run; "
                  "edit_align: set_edit_device_align of the same rows against the first reference of their sets" % (a.rounds, a.reps),
           "shapes": "64 sets x 5 references of 8..18 ids, hypotheses of <= 20 ids (L = 20), vocabulary 1000; row b belongs to set "
                     "b % 64; 5000 captions: each with its own 5 references, the first of them the model's input",
           "kernels": kernel_times(dev, a.rounds, a.reps),
           "5000_captions": validation_times(dev, a.rounds)}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
