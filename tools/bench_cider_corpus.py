#!/usr/bin/env python
"""Corpus CIDEr on the device (writes profiles/cider_corpus_bench.json):

  - the table build (set_ciderd_device_create_corpus: allocation, memset, cd_build_k) at 64 sets x 5 = 320 and 5000 sets x 5 =
    25 000 references of 7..17 ids, ids already on the device: the library's event pair around the build launch, and the whole
    call + synchronise on the host clock; table bytes and load factor (distinct grams / capacity);
  - evaluate.validation_cider of 5000 captions x 5 references against the route it replaces, in the same run: Python
    ciderd.document_frequency over decimal strings -> CiderD(...).device(dev) (the host loop of set_ciderd_device_create) ->
    prepare_refs -> score_token_ids -> mean; and against the pure-Python ciderd.corpus_cider on the same ids;
  - validation_scores(cider=True) minus validation_scores() on the same input.

    python tools/bench_cider_corpus.py [--rounds 7] [--reps 20] [--out profiles/cider_corpus_bench.json]
"""
import argparse
import ctypes as C
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
    """near-copies of references, 0-terminated rows of L ids; row b belongs to set b % len(gt)"""
    H = np.zeros((N, L), dtype=np.int64)
    for b in range(N):
        c = [w for w in gt[b % len(gt)][int(rng.integers(0, 5))] if w][:L - 1]
        for _ in range(3):
            c[int(rng.integers(0, len(c)))] = int(rng.integers(1, V))
        H[b, :len(c)] = c
    return H


def host_clock(fn, n):
    wall = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
        wall.append(1e3 * (time.perf_counter() - t0))
    return med_min(wall)


def build_times(dev, rounds, reps):
    from show_edit_tell_amd import _lib, ciderd
    from show_edit_tell_amd.device_metric import pack_ref_sets, strip_end
    lib = _lib.load()
    out = {}
    for n_sets in (64, 5000):
        sets = strip_end(corpus(np.random.default_rng(2), n_sets, 1000))
        tok, ln, off, R, L, max_set = pack_ref_sets(sets, "CIDEr", True)
        t, l, o = (torch.from_numpy(x).to(dev) for x in (tok, ln, off))
        bound = int(np.maximum(ln[:, None].astype(np.int64) - np.arange(4)[None, :], 0).sum())
        cap = 2
        while cap < 2 * bound:
            cap *= 2
        distinct = len(ciderd.document_frequency([[" ".join(map(str, c)) for c in refs] for refs in sets])[0])

        def create():
            h = C.c_void_p()
            _lib.check(lib.set_ciderd_device_create_corpus(t.data_ptr(), t.stride(0), l.data_ptr(), R, L, o.data_ptr(), n_sets, max_set,
                                                           bound, 4, 6.0, _lib.stream_of(dev), C.byref(h)), "create_corpus")
            return h

        def once():
            lib.set_ciderd_device_destroy(create())
        once(); torch.cuda.synchronize()
        lib.set_profile_enable(1)
        for _ in range(reps):
            once()
        torch.cuda.synchronize()
        rep = {r["tag"]: r for r in _lib.profile_report()}["ciderd_build"]
        lib.set_profile_enable(0)
        out["references=%d" % R] = {"sets": n_sets, "L": L, "gram_bound": bound, "distinct_grams": distinct, "capacity_slots": cap,
                                    "table_bytes": 16 * (cap + 1), "load_factor": round(distinct / cap, 4),
                                    "us_build_kernel_event_pair_around_the_launch": round(1e3 * rep["ms"] / rep["launches"], 3),
                                    "ms_create_and_destroy_host_clock_alloc_memset_kernel_free": host_clock(once, rounds * 3)}
    return out


def validation_times(dev, rounds):
    from show_edit_tell_amd import ciderd, evaluate
    from show_edit_tell_amd.device_metric import strip_end
    rng = np.random.default_rng(3)
    V, N = 1000, 5000
    gt = corpus(rng, N, V)
    Hd = torch.from_numpy(hypotheses(rng, gt, N, V)).to(dev)
    idx = torch.arange(N, dtype=torch.int32, device=dev)
    s = lambda c: " ".join(map(str, c))

    def replaced_route():
        stripped = strip_end(gt)
        df, docs = ciderd.document_frequency([[s(c) for c in refs] for refs in stripped])
        sc = ciderd.DeviceCiderD(ciderd.CiderD(df, docs), dev)
        refs = sc.prepare_refs(stripped)
        is0 = Hd == 0
        lens = torch.where(is0.any(1), is0.int().argmax(1), torch.full((N,), Hd.shape[1], dtype=torch.int64, device=dev))
        return sc.score_token_ids(Hd, idx, refs, hyp_lens=lens).mean()

    def pure_python():
        H = Hd.cpu().numpy()
        gts = {i: [s(c) for c in refs] for i, refs in enumerate(strip_end(gt))}
        res = [{"image_id": i, "caption": [s(r[:int(np.flatnonzero(r == 0)[0])])]} for i, r in enumerate(H)]
        return ciderd.corpus_cider(gts, res)[0]

    got = float(evaluate.validation_cider(Hd, None, gt, dev))
    res = {"captions": N, "references": 5 * N, "CIDEr": round(got, 6),
           "abs_diff_vs_replaced_route": abs(got - float(replaced_route())), "abs_diff_vs_python_corpus_cider": abs(got - pure_python())}
    for name, fn, n in (("python_corpus_cider_ms_host_clock", pure_python, 3),
                        ("replaced_route_python_df_host_table_upload_prepare_score_ms_host_clock", replaced_route, 3),
                        ("validation_cider_ms_host_clock_pack_upload_build_vectorise_score_mean", lambda: evaluate.validation_cider(Hd, None, gt, dev), rounds * 3),
                        ("validation_scores_ms_host_clock", lambda: evaluate.validation_scores(Hd, None, gt, dev), rounds * 3),
                        ("validation_scores_cider_ms_host_clock", lambda: evaluate.validation_scores(Hd, None, gt, dev, cider=True), rounds * 3)):
        res[name] = host_clock(fn, n)
    res["validation_scores_cider_minus_plain_ms_median"] = round(res["validation_scores_cider_ms_host_clock"]["median"]
                                                                 - res["validation_scores_ms_host_clock"]["median"], 4)
    res["validation_scores_cider_minus_plain_ms_min"] = round(res["validation_scores_cider_ms_host_clock"]["min"]
                                                              - res["validation_scores_ms_host_clock"]["min"], 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "cider_corpus_bench.json"))
    a = ap.parse_args()
    sys.path.insert(0, HERE)
    assert torch.cuda.is_available(), "this benchmark measures the GPU: there is no CPU fallback"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    res = {"how": "python tools/bench_cider_corpus.py --rounds %d --reps %d on one MI355X.  us_build_kernel...: the mean of one event "
                  "pair around each of `reps` cd_build_k launches (the kernel and ~1-2 us of event cost); host clocks end in a "
                  "synchronise; median, minimum and maximum over the rounds.  All routes of the validation block run in one process on "
                  "the same ids; the Python routes are timed 3 times" % (a.rounds, a.reps),
           "shapes": "references of 7..17 ids (count_end=False: <end> stripped), 5 per set, vocabulary 1000, n = 4; captions of <= 20 "
                     "ids (L = 20), caption b belongs to set b",
           "table_build": build_times(dev, a.rounds, a.reps),
           "validation_5000_captions": validation_times(dev, a.rounds)}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
