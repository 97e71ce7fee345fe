#!/usr/bin/env python
"""CIDEr-D on the device against the host route (writes profiles/ciderd_device_bench.json):

  - the vectorise and score kernels (device events around `reps` back-to-back launches, and one launch + synchronise as a host
    clock) at 384 hypotheses (320 samples + 64 greedy) against 64 sets x 5 references, L = 20, and at N = 5 and N = 1280;
  - the host route on the same inputs: ids to the host, CiderD.score_token_ids, scores back to the device;
  - one SCST step with reward="host" and reward="device", alternating, at B = 64 images x 5 samples: EditNet and DCNet.

    python tools/bench_ciderd_device.py [--rounds 7] [--reps 50] [--steps 5] [--out profiles/ciderd_device_bench.json]
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
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "rounds": len(xs)}


def corpus(rng, n_sets, V):
    """5 references of 7..17 words per image and a df table over them (ids stringified, as the reward plumbing does)"""
    from show_edit_tell_amd import ciderd
    gt = [[[int(w) for w in rng.integers(1, V, int(rng.integers(7, 18)))] + [0] for _ in range(5)] for _ in range(n_sets)]
    df, docs = ciderd.document_frequency([[ciderd.tokens_to_str(c) for c in caps] for caps in gt])
    return gt, ciderd.CiderD(df, docs)


def hypotheses(rng, gt, N, V, L=20):
    """near-copies of references (so that grams match), 0-terminated rows of L ids; row b belongs to set b % len(gt)"""
    H = np.zeros((N, L), dtype=np.int64)
    for b in range(N):
        c = [w for w in gt[b % len(gt)][int(rng.integers(0, 5))] if w][:L - 1]
        for _ in range(3):
            c[int(rng.integers(0, len(c)))] = int(rng.integers(1, V))
        H[b, :len(c)] = c
    return H, (np.arange(N) % len(gt)).astype(np.int32)


def kernel_times(dev, rounds, reps):
    from show_edit_tell_amd import _lib, ciderd
    lib = _lib.load()
    rng = np.random.default_rng(2)
    V = 1000
    gt, scorer = corpus(rng, 64, V)
    dsc = scorer.device(dev)
    out = {}
    for N in (384, 5, 1280):
        H, so = hypotheses(rng, gt, N, V)
        Hd, sod = torch.from_numpy(H).to(dev), torch.from_numpy(so).to(dev)
        refs = dsc.prepare_refs(gt)
        ref_tok = torch.zeros(320, refs.L, dtype=torch.int64, device=dev)
        want = scorer.score_token_ids(H, so, gt)
        got = dsc.score_token_ids(Hd, sod, refs).cpu().numpy()
        err = float(np.abs(got - want).max())
        calls = {"vectorise_320_refs": lambda: dsc.vectorise(ref_tok), "score": lambda: dsc.score_token_ids(Hd, sod, refs)}
        res = {"max_abs_err_vs_host_scorer": err}
        for name, fn in calls.items():
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
            # the kernel alone: the library's profile scopes record one event pair around every launch
            lib.set_profile_enable(1)
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            rep = {r["tag"]: r for r in _lib.profile_report()}
            lib.set_profile_enable(0)
            tag = "ciderd_vectorise" if name.startswith("vectorise") else "ciderd_score"
            res[name] = {"us_kernel_event_pair_around_the_launch": round(1e3 * rep[tag]["ms"] / rep[tag]["launches"], 3),
                         "us_per_call_back_to_back_events": med_min(ev), "us_one_call_and_synchronise_host_clock": med_min(wall)}

        def host_route():
            h = Hd.cpu().numpy()
            s = scorer.score_token_ids(h, so, gt)
            return torch.from_numpy(s).to(dev)

        def device_route():
            return dsc.score_token_ids(Hd, sod, dsc.prepare_refs(gt))
        for name, fn in (("host_route_copy_score_copy", host_route), ("device_route_prepare_refs_and_score", device_route)):
            fn(); torch.cuda.synchronize()
            wall = []
            for _ in range(rounds * 3):
                t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
                wall.append(1e6 * (time.perf_counter() - t0))
            res[name] = {"us_host_clock": med_min(wall)}
        out["N=%d" % N] = res
    return out


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

        def step(route):
            if net == "editnet":
                return scst_train_step(model, opt, wm, X, prev, plen, gt, scorer, n_samples=5, reward=route)
            return dcnet_scst_train_step(model, opt, wm, prev, plen, gt, scorer, n_samples=5, reward=route)
        for route in ("host", "device"):
            step(route)
        torch.cuda.synchronize()
        ms = {"host": [], "device": []}
        for _ in range(rounds):                       # the two routes alternate inside one process
            for route in ("host", "device"):
                t0 = time.perf_counter()
                for _ in range(steps):
                    step(route)
                torch.cuda.synchronize()
                ms[route].append(1e3 * (time.perf_counter() - t0) / steps)
        out[net] = {"ms_per_step_reward_host": med_min(ms["host"]), "ms_per_step_reward_device": med_min(ms["device"]),
                    "steps_per_round": steps}
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
                                                  "ciderd_device_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark measures the GPU: there is no CPU fallback"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res = {"how": "python tools/bench_ciderd_device.py --rounds %d --reps %d --steps %d on one MI355X.  us_kernel...: the mean of one "
                  "event pair around each of `reps` launches (the kernel and ~1-2 us of event cost); us_per_call_back_to_back: device "
                  "events around `reps` Python calls, which is the host's enqueue rate (tensor allocation + ctypes) when that is "
                  "slower than the kernel; host clocks end in a synchronise; median and minimum over the rounds; the two SCST "
                  "routes alternate in one process" % (a.rounds, a.reps, a.steps),
           "shapes": "64 sets x 5 references of 8..18 ids, hypotheses of <= 20 ids (L = 20), vocabulary 1000; row b belongs to set b % 64",
           "kernels": kernel_times(dev, a.rounds, a.reps)}
    if not a.skip_scst:
        res["scst_step_B64_x5_samples"] = scst_times(dev, a.steps, a.rounds)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
