#!/usr/bin/env python
"""The DCNet MSE stage (dcnet_with_mse.py) on one MI355X, against the XE stage it extends:
  * train.dcnet_mse_train_step vs train.dcnet_xe_train_step at the at-size DCNet shape (B=128, captions of 20 words, prev
    captions of 20, D=1024, V=10000), train mode, fwd + bwd + clip + Adam; alternated windows, the better of two each;
  * the B=4 no-grad teacher-forced forward through set_dcnet_xe_forward_hidden with and without last_hidden (the persistent
    launch: the LH variant vs the plain one), and the whole six-output forward (+ the ground-truth encoder pass).
One JSON line.  Kernel statistics: run `--only mse` (and `--only xe`) under `rocprofv3 --kernel-trace --stats -d <dir> -o run --`.

    python tools/bench_dcnet_mse.py [--steps 10] [--windows 2] [--train-only] [--only xe|mse]
"""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

V, D, A, T = 10000, 1024, 512, 20


def _timed(fn, n):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10); ap.add_argument("--windows", type=int, default=2)
    ap.add_argument("--train-only", action="store_true")
    ap.add_argument("--only", choices=("xe", "mse"), help="time one of the two train steps only (profiling runs)")
    a = ap.parse_args()
    from show_edit_tell_amd import dcnet, dcnet_with_mse, synth
    from show_edit_tell_amd.train import dcnet_mse_train_step, dcnet_xe_train_step
    dev = torch.device("cuda", 0)
    wm = synth.word_map(V)
    sd = {k: torch.from_numpy(v) for k, v in synth.dcnet_state(17, V, D, A, D // 2, D, 3.0, 8.0, 3.0).items()}

    def stage1():
        m = dcnet.DAE(wm, None, D, A, D // 2, D)
        m.load_state_dict(sd, strict=False)
        return m.to(dev)

    out = {"config": "B=128, captions 20, prev captions %d, D=%d, V=%d, train mode, fwd + bwd + clip 0.25 + Adam" % (T, D, V)}
    B = 128
    prev, plen = (torch.from_numpy(x).to(dev) for x in synth.prev_captions(7, B, T, V, 5))
    caps, clen = (torch.from_numpy(x).to(dev) for x in synth.captions(7, B, V, 20, 20))
    xe = stage1()
    torch.manual_seed(0)
    ar = dcnet_with_mse.DAEWithAR(dae=stage1())
    opt_xe = torch.optim.Adam(xe.parameters(), lr=5e-4)
    opt_ar = torch.optim.Adam(ar.parameters(), lr=5e-4)
    step_xe = lambda: dcnet_xe_train_step(xe, opt_xe, caps, clen, prev, plen)
    step_mse = lambda: dcnet_mse_train_step(ar, opt_ar, caps, clen, prev, plen)
    if a.only:
        step = step_xe if a.only == "xe" else step_mse
        for _ in range(3):
            step()
        print(json.dumps({"only": a.only, "train_step_ms": round(1e3 * min(_timed(step, a.steps) for _ in range(a.windows)), 3)}))
        return
    for _ in range(3):
        step_xe(); step_mse()
    w_xe, w_mse = [], []
    for _ in range(a.windows):                      # alternated windows: box drift hits both alike
        w_xe.append(_timed(step_xe, a.steps))
        w_mse.append(_timed(step_mse, a.steps))
    t_xe, t_mse = min(w_xe), min(w_mse)
    out.update(xe_train_step_ms=round(1e3 * t_xe, 3), mse_train_step_ms=round(1e3 * t_mse, 3),
               mse_extra_ms=round(1e3 * (t_mse - t_xe), 3), mse_over_xe=round(t_mse / t_xe, 4),
               xe_windows_ms=[round(1e3 * t, 3) for t in w_xe], mse_windows_ms=[round(1e3 * t, 3) for t in w_mse])
    if not a.train_only:
        B = 4
        prev, plen = (torch.from_numpy(x).to(dev) for x in synth.prev_captions(3, B, T, V, 5))
        caps, clen = (torch.from_numpy(x).to(dev) for x in synth.captions(3, B, V, 20, 20))
        m = dcnet_with_mse.DAEWithAR(dae=stage1()).eval()
        dae = m.dae
        with torch.no_grad():
            clen_s, si = clen.squeeze(1).sort(dim=0, descending=True, stable=True)
            cs, ps, pls = caps[si].contiguous(), prev[si].contiguous(), plen[si].reshape(-1).contiguous()
            dl = (clen_s - 1).tolist()
            without = lambda: dae._xe_forward_hidden(cs, dl, ps, pls, want_last=False)
            with_last = lambda: dae._xe_forward_hidden(cs, dl, ps, pls, want_last=True)
            whole = lambda: m(caps, clen, prev, plen)
            for _ in range(3):
                without(); with_last(); whole()
            w0, w1, w2 = [], [], []
            for _ in range(a.windows):
                w0.append(_timed(without, 20)); w1.append(_timed(with_last, 20)); w2.append(_timed(whole, 20))
            p_without, l_without = without()
            p_with, last = with_last()
        out.update(b4_forward_without_last_hidden_ms=round(1e3 * min(w0), 3),
                   b4_forward_with_last_hidden_ms=round(1e3 * min(w1), 3),
                   b4_six_output_forward_ms=round(1e3 * min(w2), 3),
                   b4_same_scores_with_and_without=bool(torch.equal(p_without, p_with)),
                   b4_last_hidden_finite=bool(torch.isfinite(last).all()))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
