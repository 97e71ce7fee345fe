#!/usr/bin/env python
"""Temperature / top-k / top-p in self-critical training (include/set_hip.h set_sample_logp_bwd_opts_f32) on one MI355X:
  * the backward of the sampled log-prob over the T * B = 18 * 128 rows of a rollout at V = 9490: ONE launch of the new kernel
    with a NULL key and no options (neutral) and with the keys of top_k = 50 + top_p = 0.9 at T = 0.8, on logs padded to a leading
    dimension of 9492 floats (its 16-byte path, what the nodes log with options) and on unpadded logs (9490: its scalar path), next
    to the 18 launches of set_sample_logp_bwd_f32 the neutral path of the nodes issues (unpadded logs, padded gradient rows).  One
    sample = --calls repetitions between two device events, reported per T * B rows; the arms alternate sample by sample,
    --rounds rounds of --iters samples; per arm the median of every round, the median of those and their spread;
  * train.scst_train_step of the full-size EditNet at the size of tests/test_hip_train.py::test_scst_full_size_five_samples (4
    images, 5 samples each), neutral and with top_k = 50 + top_p = 0.9, alternated step by step, host clock around a device
    synchronise.  With --root pointing at a checkout of another commit its package is measured instead (a commit without the
    options runs the neutral arm only): the two neutral figures of one box and one session are the comparison to read.
One JSON line, also written to --out.

    python tools/bench_truncated_scst.py [--iters 10] [--rounds 3] [--calls 20] [--root DIR] [--out profiles/truncated_scst_bench.json]
"""
import argparse, ctypes as C, inspect, json, os, statistics, sys, time


def rounds_of(arms, rounds, iters):
    """arms {name: fn -> one sample}; the arms alternate sample by sample"""
    out = {name: [] for name in arms}
    for _ in range(rounds):
        got = {name: [] for name in arms}
        for _ in range(iters):
            for name, fn in arms.items():
                got[name].append(fn())
        for name in arms:
            out[name].append(statistics.median(got[name]))
    return out


def summary(r, digits):
    return {name: {"median": round(statistics.median(v), digits), "round_medians": [round(x, digits) for x in v],
                   "spread_between_rounds": round(max(v) - min(v), digits)} for name, v in r.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10); ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    sys.path.insert(0, os.path.join(os.path.abspath(a.root), "tests"))
    import numpy as np
    import torch
    from show_edit_tell_amd import _lib as L, ciderd, train
    lib = L.load()
    dev = torch.device("cuda", 0)
    st = L.stream_of(dev)
    result = {"root": os.path.basename(os.path.abspath(a.root))}

    if hasattr(lib, "set_sample_logp_bwd_opts_f32") and "set_sample_logp_bwd_opts_f32" not in L.MISSING:
        T, B, V, n4 = 18, 128, 9490, 9492
        R = T * B
        g_ = torch.Generator(device="cpu").manual_seed(5)
        x = torch.randn(R, V, generator=g_) * 2.0
        flat, padded = x.to(dev), torch.zeros(R, n4, device=dev)
        padded[:, :V] = flat
        opts = L.SampleOpts(temperature=0.8, top_k=50, top_p=0.9)
        raw, lse, lp = torch.empty(R, dtype=torch.long, device=dev), torch.empty(R, device=dev), torch.empty(R, device=dev)
        key = torch.empty(R, dtype=torch.int32, device=dev)
        seq, it = torch.zeros(B, T, dtype=torch.long, device=dev), torch.zeros(B, dtype=torch.long, device=dev)
        unf, alive = torch.ones(B, dtype=torch.int32, device=dev), torch.ones(T + 2, dtype=torch.int32, device=dev)
        for t in range(T):                  # the keys, ids and lse of the truncated distribution (t = 1: the state is the caller's)
            r = slice(t * B, (t + 1) * B)
            L.check(lib.set_sample_pick_opts_key_f32(padded[r].data_ptr(), n4, B, V, 1, T, V - 1, 7, t, L.ptr(seq), L.ptr(it),
                                                     L.ptr(unf), L.ptr(alive), raw[r].data_ptr(), lse[r].data_ptr(),
                                                     lp[r].data_ptr(), st, C.byref(opts), key[r].data_ptr()))
        lse_n = torch.logsumexp(flat.double(), 1).float()
        g = torch.randn(R, generator=g_).to(dev)
        d = torch.zeros(R, n4, device=dev)

        def timed(body):
            def fn():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.calls):
                    body()
                e1.record()
                e1.synchronize()
                return 1e3 * e0.elapsed_time(e1) / a.calls                   # us per T * B rows
            return fn

        def new(src, ld, ls, k, o):
            return lambda: L.check(lib.set_sample_logp_bwd_opts_f32(L.ptr(src), ld, L.ptr(ls), L.ptr(raw), None if k is None else L.ptr(k),
                                                                    L.ptr(g), L.ptr(d), n4, R, V, None if o is None else C.byref(o), st))

        def old():
            for t in range(T):
                r = slice(t * B, (t + 1) * B)
                L.check(lib.set_sample_logp_bwd_f32(flat[r].data_ptr(), V, lse_n[r].data_ptr(), raw[r].data_ptr(), g[r].data_ptr(),
                                                    d[r].data_ptr(), n4, B, V, st))

        arms = {"existing_18_launches_ld9490": timed(old),
                "new_neutral_ld9492": timed(new(padded, n4, lse_n, None, None)),
                "new_neutral_ld9490_scalar": timed(new(flat, V, lse_n, None, None)),
                "new_top_k50_top_p0.9_T0.8_ld9492": timed(new(padded, n4, lse, key, opts))}
        for fn in arms.values():
            fn()
        result["backward_us_per_2304_rows"] = summary(rounds_of(arms, a.rounds, a.iters), 2)
        result["backward_bytes_per_call"] = 8 * R * V

    # ---- the self-critical step
    from hip_adapter import editnet_modules, to_dev
    d_, _, rl = editnet_modules("editnet_full_b4")
    wm = d_["wm"]
    prev, plen, X = to_dev(d_["prev"]), to_dev(d_["plen"]), to_dev(d_["X"])
    Bi = X.shape[0]
    rng = np.random.default_rng(3)
    allcaps = np.zeros((Bi, 5, 12), dtype=np.int64)
    for b in range(Bi):
        for j in range(5):
            n = int(rng.integers(3, 9))
            allcaps[b, j, 0] = wm["<start>"]
            allcaps[b, j, 1:1 + n] = rng.integers(1, len(wm) - 4, n)
            allcaps[b, j, 1 + n] = wm["<end>"]
    gt = ciderd.ground_truth_lists(allcaps, wm)
    df, docs = ciderd.document_frequency([[ciderd.tokens_to_str(c) for c in caps] for caps in gt])
    scorer = ciderd.CiderD(df, 50)
    opt = torch.optim.Adam(rl.parameters(), lr=1e-6)

    def step(kw):
        def fn():
            torch.cuda.synchronize(); t = time.perf_counter()
            train.scst_train_step(rl, opt, wm, X, prev, plen, gt, scorer, n_samples=5, **kw)
            torch.cuda.synchronize()
            return 1e3 * (time.perf_counter() - t)                          # ms per step
        return fn

    arms = {"neutral": step({})}
    if "top_k" in inspect.signature(train.scst_train_step).parameters:
        arms["top_k50_top_p0.9_T0.8"] = step(dict(temperature=0.8, top_k=50, top_p=0.9))
    for _ in range(3):
        for fn in arms.values():
            fn()
    result["editnet_scst_step_ms"] = summary(rounds_of(arms, a.rounds, a.iters), 3)
    result["config"] = ("backward: T*B=18*128 rows, V=9490, %d calls per sample; step: editnet_full_b4 (4 images x 5 samples), ms per "
                        "step; %d rounds of %d alternated samples" % (a.calls, a.rounds, a.iters))
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
