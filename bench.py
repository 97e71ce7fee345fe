#!/usr/bin/env python
"""Headline benchmark: EditNet decode-steps/sec at B=128 (36x2048 features, prev-caption len 20).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

A plain run sets up, warms up, picks the stream count (untimed probe, below), times exactly K steps in ONE window, writes
the outputs of the last timed step if `--dump-outputs DIR` is given and prints the result line.  `--full` adds everything
else: the repeated windows (`repeat`; `value` is then the median window when a window is shorter than 0.5 s), the
single-stream and pipelined figures, the XE forward, the per-kernel profile (`roofline`, `kernels`), `train`, `secondary`,
`cpu_baseline` and `experimental`.

`--dump-outputs DIR` writes what the last timed step returned to its caller (rank 0's batch): DIR/seq.npy (greedy token ids,
float64, B x 18) and DIR/seq_logp.npy (their log-probabilities, float32, B x 18).  Inputs and weights are seeded, so two
runs with the same arguments decode the same batch.

`--gpus N` with N > 1 and no WORLD_SIZE in the environment re-launches itself under
`torch.distributed.run` with N ranks (one per GPU, RCCL); under torchrun the flag is informational and
the ranks come from RANK / LOCAL_RANK / WORLD_SIZE.

One bench "step" = one pass of the hot path over one batch: the free-running greedy decode of
the reference's `editnet_rl.py:485-549` for a batch of 128 images — the per-sequence prologue
(caption encoder + hoisted projections) plus 19 decode timesteps — entirely on the GPU through
the C ABI (no host sync inside).  The metric counts decode timesteps:
    value = n_gpus * K * 19 / wall_time          [decode-steps/sec, B=128 rows each]
Inputs and weights are synthetic (seeded generator, random-init weights of the reference's
architecture, V = 10 000) and are resident in HBM before the timed region.  Multi-GPU: the path
shards by batch with replicated weights and no data-path collective: each rank
decodes its own 128-image batch (weak scaling); timing is barrier / sync bracketed, max over ranks.
Each decode is a strictly sequential chain of small kernels over 128 rows, so several independent B=128 batches are
kept in flight per GPU, each on its own HIP stream and workspace (the K timed steps are still K complete B=128
decodes; nothing is skipped or shared).  By default (`--streams 0`) an untimed probe before the timed region picks the
count among 3 / 7 / 11 (`batches_in_flight_per_gpu`, `stream_probe_decode_steps_per_sec`); `--streams N` pins it;
`single_stream_*` (top level) is the one-batch-at-a-time figure measured in the same run.

Extra objects on the JSON line (`--full` only):
  roofline      dominant kernel = the fp32-MFMA grouped GEMM `gemm_nt_f32`; achieved = algorithmic FLOPs of its
                launches / their summed duration, measured with HIP events on the launch stream in a second,
                identical, profiled pass (`value` comes from the un-instrumented pass)
  kernels       the same event timing for every kernel family (ms per bench step)
  repeat        the timed region repeated (median / min / max decode-steps/sec over the windows)
  train         the path's one exchange step: EditNet XE training step at B=128 per GPU (editnet.py:558-581,
                train mode) with the bucketed gradient all-reduce; ms per step with and without the collectives
  secondary     (N = 1) the path's other callers, timed in the same run: SCST step (configs[4]), adaptive features
                (configs[3]), DCNet / B=4 greedy decode (configs[0] shape), batched beam search (row f2); tools/secondary.py
  cpu_baseline  the as-written torch-CPU restatement of the reference loop (oracle/editnet_torch.py) and the numpy
                port (oracle/editnet_np.py) timed on this box's host cores, bounded samples
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

B, R, F, T, V, D, A = 128, 36, 2048, 20, 10000, 1024, 512
MAX_LEN = 18
STEPS_PER_DECODE = MAX_LEN + 1          # editnet_rl.py:503 runs max_len + 1 timesteps
STREAM_CANDIDATES = (3, 7, 11)          # batches in flight probed by --streams 0 (see main)
PEAK_FP32_MFMA_TFLOPS = 157.3           # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, dense
PEAK_HBM_GBS = 8000.0
TRAIN_TFLOP_PER_STEP = 1.23             # contractions of one B=128 XE training step as executed
SURVEY_GFLOP_PER_TIMESTEP = 16.88       # SURVEY.md 8d, B = 128, eval mode, loop invariants hoisted
EXECUTED_GFLOP_PER_DECODE = 281.0       # contractions one B = 128 greedy decode executes here (token table active), DESIGN.md 3
PMC_FILES = ("r06_pmc_bench_traffic.json", "r05_pmc_bench_traffic.json", "r04_pmc_bench_traffic.json", "r03_pmc_bench_traffic.json", "r02_pmc_bench_traffic.json", "r01_pmc_bench_traffic.json")


def pmc_traffic():
    """HBM bytes per launch of the dominant kernel from the committed rocprofv3 --pmc passes
    (tools/pmc_bench.sh -> tools/pmc_traffic.py); counters cannot be read from inside this process."""
    for name in PMC_FILES:
        try:
            with open(os.path.join(ROOT, "profiles", name)) as f:
                d = json.load(f)
                d["file"] = "profiles/" + name
                return d
        except OSError:
            continue
    return None


# The decode step's three launches of the dominant kernel, by workgroup count (F/A 698 -> grid 704, B and D 768): what the
# counters say against the bytes the launch NEEDS — weights once + activation rows once + ONE copy of the outputs
# (MB; B: 29.4 + 0.5 in, 3.7 out; D: 50.3 + 1.6 in, 2.1 out; F/A: 91.4 + 1.0 in, 9.3 out) — fetch and write amplification
# reported separately (the write side is the split-K slabs: every slab is one more copy of the output)
STEP_LAUNCH_NEED_MB = {"704": (92.4, 9.3), "768": ((29.9 + 51.9) / 2, (3.7 + 2.1) / 2)}


def _step_traffic(tr):
    if not tr or "by_workgroups" not in tr:
        return None
    out = {}
    for wgs, (need_in, need_out) in STEP_LAUNCH_NEED_MB.items():
        m = tr["by_workgroups"].get(wgs)
        if m and m.get("write_MB") is not None:
            out["F/A (fc + next gates1 + h2h)" if wgs == "704" else "B, D (mean of the two 768-workgroup launches)"] = {
                "fetch_MB": m["fetch_MB"], "write_MB": m["write_MB"], "needed_in_MB": round(need_in, 1),
                "needed_out_MB": round(need_out, 1), "fetch_amplification": round(m["fetch_MB"] / need_in, 2),
                "write_amplification": round(m["write_MB"] / need_out, 2)}
    return out or None


# ------------------------------------------------------------------------------------------------
# CPU baseline (rank 0, N = 1 only): the oracle is test infrastructure; here it is the thing timed
# BESIDE the product, never inside it.
# ------------------------------------------------------------------------------------------------
def _median(xs):
    xs = sorted(xs)
    n = len(xs)
    return xs[n // 2] if n % 2 else 0.5 * (xs[n // 2 - 1] + xs[n // 2])


def _time_decodes(fn, budget_s, min_n=2, max_n=10, warm=1):
    for _ in range(warm):
        fn()
    ts, t_begin = [], time.perf_counter()
    while len(ts) < max_n and (len(ts) < min_n or time.perf_counter() - t_begin < budget_s):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return ts


def cpu_baseline(budget_s=float(os.environ.get("SET_CPU_BASELINE_BUDGET", "10"))):
    """decode-steps/sec of the reference's greedy loop on the host cores.

    `value` = the as-written torch-CPU restatement (oracle/editnet_torch.py: the op stream of
    editnet_rl.py:503-547, nothing hoisted, torch's CPU BLAS) at B=128: 3 warm-ups, median of 10 decodes at
    the best of 8 / 32 / all-physical-core thread counts (each probed with a short sample first; all listed
    under `variants`, with B=4 = BASELINE.json configs[0]) and the numpy/OpenBLAS port with hoisted invariants (oracle/editnet_np.py)."""
    import numpy as np
    import torch
    from oracle import editnet_np as EN
    from oracle import editnet_torch as ET
    from show_edit_tell_amd import synth
    logical = os.cpu_count() or 1
    try:
        import psutil
        physical = psutil.cpu_count(logical=False) or logical
    except Exception:
        physical = logical
    sd = synth.editnet_state(14, V, D, A, F, emb_scale=3.0, fc_scale=8.0, gain=3.0)
    wm = synth.word_map(V)
    X = synth.features(25, B, R, F)
    prev, plen = synth.prev_captions(25, B, T, V, 5)
    P_t = ET.params_from_numpy(sd)
    Xt, prevt, plent = torch.from_numpy(X), torch.from_numpy(prev), torch.from_numpy(plen)
    variants = []

    def run_torch(nthreads, bs, budget):
        torch.set_num_threads(nthreads)
        fn = lambda: ET.greedy_decode(P_t, wm["<start>"], wm["<end>"], prevt[:bs], plent[:bs], Xt[:bs])
        ts = _time_decodes(fn, budget)
        return dict(impl="torch-cpu as written (oracle/editnet_torch.py)", batch=bs, threads=nthreads, decodes=len(ts),
                    median_s_per_decode=round(_median(ts), 4),
                    decode_steps_per_sec=round(STEPS_PER_DECODE / _median(ts), 3))

    saved = torch.get_num_threads()
    # oversubscribing the small per-step ops hurts: time 8 (the SURVEY §6 probe), 32 and all physical cores, and
    # let the CPU put its best foot forward
    counts = sorted({min(8, logical), min(32, physical), physical})
    b128 = [run_torch(n, B, budget_s / 3) for n in counts]              # probe: which thread count the CPU likes best ...
    best_n = max(b128, key=lambda v: v["decode_steps_per_sec"])["threads"]
    variants += b128
    # ... and the reported figure at that count by SURVEY §8d's protocol: >= 3 warm-ups, median of >= 10 full decodes
    torch.set_num_threads(best_n)
    fn_main = lambda: ET.greedy_decode(P_t, wm["<start>"], wm["<end>"], prevt, plent, Xt)
    ts_main = _time_decodes(fn_main, budget_s, min_n=10, max_n=10, warm=3)
    main_v = dict(impl="torch-cpu as written (oracle/editnet_torch.py), 3 warm-ups + 10 decodes", batch=B, threads=best_n,
                  decodes=len(ts_main), median_s_per_decode=round(_median(ts_main), 4),
                  decode_steps_per_sec=round(STEPS_PER_DECODE / _median(ts_main), 3))
    variants.append(main_v)
    variants.append(run_torch(main_v["threads"], 4, budget_s / 4))
    torch.set_num_threads(saved)
    # numpy port (loop invariants hoisted = the GPU path's algorithm on the CPU)
    threads_np = min(logical, 32)
    try:
        from threadpoolctl import threadpool_limits
        limiter = threadpool_limits(limits=threads_np)
    except Exception:
        limiter, threads_np = None, logical
    P_n = EN.cast_params(sd)
    ts = _time_decodes(lambda: EN.greedy_decode(P_n, wm["<start>"], wm["<end>"], prev, plen, X), budget_s, max_n=6)
    if limiter is not None:
        limiter.restore_original_limits()
    variants.append(dict(impl="numpy port, invariants hoisted (oracle/editnet_np.py)", batch=B, threads=threads_np,
                         decodes=len(ts), median_s_per_decode=round(_median(ts), 4),
                         decode_steps_per_sec=round(STEPS_PER_DECODE / _median(ts), 3)))
    blas = "mkl" if torch.backends.mkl.is_available() else "non-mkl"
    return dict(value=main_v["decode_steps_per_sec"], unit="decode-steps/sec", cores=main_v["threads"], kind="port",
                sample="median of %d full greedy decodes after 3 warm-ups (encoder + 19 timesteps) of the B=128 workload, as-written torch "
                       "fp32 restatement of editnet_rl.py:485-549 (torch %s, %s BLAS), best of %s threads on a host with %d "
                       "physical / %d logical cpus; numpy %s for the port variant" % (
                           main_v["decodes"], torch.__version__, blas, counts, physical, logical, np.__version__),
                variants=variants)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def spawn_ranks(n):
    """`python bench.py --gpus N` without torchrun: re-launch under torch.distributed.run, one rank per GPU."""
    import torch
    have = torch.cuda.device_count()
    if have < n and not os.environ.get("SET_BENCH_ONE_DEVICE"):
        raise SystemExit("bench.py --gpus %d: only %d GPU(s) visible (set SET_BENCH_ONE_DEVICE=1 SET_BENCH_BACKEND=gloo "
                         "to exercise the multi-rank path on one device)" % (n, have))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr",
           "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "8")
    return subprocess.call(cmd, env=env)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=300, help="timed bench steps (complete B=128 decodes); default gives a ~1 s region")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--full", action="store_true",
                    help="also run every measurement beside the headline (repeated windows, single-stream / pipelined figures, "
                         "XE forward, per-kernel profile, train, secondary, cpu_baseline, experimental); the --no-* and "
                         "--repeat / --train-steps options apply to these")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs as DIR/seq.npy (float64) and DIR/seq_logp.npy (float32)")
    ap.add_argument("--repeat", type=int, default=5, help="extra repetitions of the timed region (median reported under 'repeat')")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--no-train", action="store_true", help="skip the XE training-step leg ('train' object)")
    ap.add_argument("--no-secondary", action="store_true",
                    help="skip the 'secondary' object (SCST step, adaptive features, DCNet / B=4 greedy, batched beam search)")
    ap.add_argument("--train-steps", type=int, default=6)
    ap.add_argument("--streams", type=int, default=int(os.environ.get("SET_BENCH_STREAMS", "0")),
                    help="independent batches in flight per GPU (each on its own HIP stream + workspace)")
    args = ap.parse_args()

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(spawn_ranks(args.gpus))

    import torch
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    dist = None
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the decode path has no CPU fallback")
    # SET_BENCH_BACKEND=gloo + SET_BENCH_ONE_DEVICE=1: exercise the multi-rank code path on a 1-GPU box
    backend = os.environ.get("SET_BENCH_BACKEND", "nccl")
    if os.environ.get("SET_BENCH_ONE_DEVICE"):
        local_rank = 0
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.cuda.set_device(local_rank)
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend)
    dev = torch.device("cuda", local_rank)
    torch.cuda.set_device(dev)

    from show_edit_tell_amd import _lib, editnet, editnet_rl, synth
    wm = synth.word_map(V)
    dec = editnet_rl.DecoderC(wm, D, D, D, A, F)
    sd = synth.editnet_state(14, V, D, A, F, emb_scale=3.0, fc_scale=8.0, gain=3.0)
    sd["caption_encoder.embed.embedding.weight"] = sd["embed.embedding.weight"]
    dec.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    dec = dec.to(dev).eval()
    seed = 25 + rank
    X = torch.from_numpy(synth.features(seed, B, R, F)).to(dev)
    prev_np, plen_np = synth.prev_captions(seed, B, T, V, 5)
    prev, plen = torch.from_numpy(prev_np).to(dev), torch.from_numpy(plen_np).to(dev)

    # batches in flight per GPU: every batch decodes on its own HIP stream.  --streams 0 (default) probes a few counts
    # before the timed region and keeps the best (how HIP streams map onto the hardware queues decides how well the
    # launches of different decodes interleave: 3, 7 and 11 streams measured 6.46 / 6.59 / 6.62 k on one box, 4 streams
    # 5.9 k; the probe makes the choice robust); --streams N pins it, --streams 1 is the single-stream figure.
    pool = [torch.cuda.Stream(dev) for _ in range(max(1, args.streams if args.streams > 0 else max(STREAM_CANDIDATES)))]
    streams = pool[:args.streams] if args.streams > 1 else (None if args.streams == 1 else pool[:STREAM_CANDIDATES[0]])

    def run(k):
        out = None
        if streams is None:
            for _ in range(k):
                out = dec(wm, prev, plen, X, True, False)
            return out
        cur = torch.cuda.current_stream(dev)
        for s in streams:
            s.wait_stream(cur)
        for i in range(k):
            with torch.cuda.stream(streams[i % len(streams)]):
                out = dec(wm, prev, plen, X, True, False)
        for s in streams:
            cur.wait_stream(s)
        return out

    def barrier():
        torch.cuda.synchronize(dev)
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize(dev)

    def max_over_ranks(x):
        if dist is None:
            return x
        t = torch.tensor([x], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    def timed_region():
        barrier()
        t0 = time.perf_counter()
        out = run(args.steps)
        barrier()
        return max_over_ranks(time.perf_counter() - t0), out

    stream_probe = None
    with torch.no_grad():
        run(args.warmup)
        if args.streams == 0:
            # untimed probe: 48 decodes per candidate; every rank must make the same choice (max over ranks of the time)
            stream_probe = {}
            for n in STREAM_CANDIDATES:
                streams = pool[:n]
                run(n)
                barrier()
                t0 = time.perf_counter()
                run(48)
                barrier()
                stream_probe[n] = max_over_ranks(time.perf_counter() - t0)
            best = min(stream_probe, key=stream_probe.get)
            streams = pool[:best]
            args.streams = best
            stream_probe = {str(n): round(48 * STEPS_PER_DECODE / t, 1) for n, t in stream_probe.items()}
            run(args.warmup)
        elapsed, out = timed_region()                      # the first window of exactly K timed steps
        first_elapsed = elapsed
        windows = []
        if args.full:
            # short regions (the driver's --steps 20 is a 60-ms window) are repeated at least 15 times and `value` is the
            # MEDIAN window: one window of 20 decodes moves by a few percent with host jitter; every window is exactly K steps
            # between barrier + synchronize on both sides, max over ranks
            n_win = max(args.repeat, int(os.environ.get("SET_BENCH_MIN_WINDOWS", "15"))) if elapsed < 0.5 else args.repeat
            for _ in range(max(0, n_win - 1)):
                e, out = timed_region()
                windows.append(e)
            if elapsed < 0.5:
                elapsed = _median([elapsed] + windows)
        seq, seq_logp = out
        if args.dump_outputs and rank == 0:
            # the last timed decode's (seq, seq_logp), copied to the host before anything else reuses the workspaces
            dump = {"seq": seq.cpu().numpy().astype("float64"), "seq_logp": seq_logp.float().cpu().numpy()}

        single = None
        pipelined = None
        if args.full and streams is not None and rank == 0:
            # one batch at a time (what a caller that issues one decode after the other sees): windows of K decodes until
            # >= 0.5 s has been timed (3 ... 15 windows), median window — a single 80-ms window right after the multi-stream
            # region measured anything between 3.4 k and 4.7 k on the same build
            torch.cuda.synchronize(dev)
            keep, streams = streams, None
            run(max(3, min(args.warmup, 5)))
            singles, total = [], 0.0
            while len(singles) < 3 or (total < 0.5 and len(singles) < 15):
                torch.cuda.synchronize(dev)
                ts = time.perf_counter()
                run(args.steps)
                torch.cuda.synchronize(dev)
                singles.append(time.perf_counter() - ts)
                total += singles[-1]
            single = _median(singles)
            # the same single caller with pipeline.DevicePrefetcher(begin_ahead=...): the prologue of decode i+1 (caption encoder
            # + hoisted projections, independent of decode i) runs on the prefetcher's copy stream while decode i's timestep
            # loop runs on the caller's; reported separately, never as single_stream_*
            from show_edit_tell_amd.pipeline import DevicePrefetcher

            def run_pipelined(k, whole):
                # whole = False: only the prologue of the next batch runs ahead (one side stream); True: decoder.decode_ahead —
                # whole decodes of the next three batches run ahead on three side streams (inference loops, fixed weights)
                ahead = (lambda b: dec.decode_ahead(wm, b[1], b[2], b[0])) if whole else (lambda b: dec.begin_ahead(b[1], b[2], b[0]))
                pf = DevicePrefetcher(((X, prev, plen) for _ in range(k)), dev, depth=3 if whole else 2,
                                      streams=3 if whole else 1, begin_ahead=ahead)
                out = None
                for b in pf:
                    out = dec(wm, b[1], b[2], b[0], True, False)
                return out
            pipelined = {}
            try:
                ref_seq = run(1)[0]
                for mode, whole in (("prologue_ahead", False), ("decode_ahead", True)):
                    run_pipelined(max(3, min(args.warmup, 5)), whole)
                    hits0 = int(dec.__dict__.get("_ahead_hits", 0))
                    pipes, total = [], 0.0
                    while len(pipes) < 3 or (total < 0.5 and len(pipes) < 15):
                        torch.cuda.synchronize(dev)
                        ts = time.perf_counter()
                        out_p = run_pipelined(args.steps, whole)
                        torch.cuda.synchronize(dev)
                        pipes.append(time.perf_counter() - ts)
                        total += pipes[-1]
                    pipelined[mode] = {"decode_steps_per_sec": round(args.steps * STEPS_PER_DECODE / _median(pipes), 2),
                                       "ids_equal_unpipelined": bool(torch.equal(out_p[0], ref_seq)),
                                       "decodes_served_ahead": int(dec.__dict__.get("_ahead_hits", 0)) - hits0,
                                       "decodes": len(pipes) * args.steps}
            except Exception as e:
                pipelined["error"] = repr(e)[:200]
            streams = keep
        # secondary figure: teacher-forced XE forward (editnet.py:479-548, eval mode), same batch, 19 timesteps
        xe_rate = None
        caps = clen = None
        if args.full:
            caps_np, clen_np = synth.captions(seed, B, V, 20, 20)
            caps, clen = torch.from_numpy(caps_np).to(dev), torch.from_numpy(clen_np).to(dev)
        if args.full and rank == 0:
            xe_fwd = lambda: editnet.DecoderC.forward(dec, X, caps, clen, prev, plen, False, 0.0)
            for _ in range(2):
                xe_fwd()
            torch.cuda.synchronize(dev)
            tx = time.perf_counter()
            nx = max(10, args.steps // 8)
            for _ in range(nx):
                xe_fwd()
            torch.cuda.synchronize(dev)
            xe_rate = nx * STEPS_PER_DECODE / (time.perf_counter() - tx)
        prof = None
        if args.full and rank == 0 and not args.no_profile:
            keep, streams = streams, None                 # per-kernel timing is taken on ONE stream
            lib = _lib.load()
            lib.set_profile_enable(1)
            torch.cuda.synchronize(dev)
            t1 = time.perf_counter()
            nprof = min(args.steps, 40)
            run(nprof)
            torch.cuda.synchronize(dev)
            prof_elapsed = time.perf_counter() - t1
            prof = _lib.profile_report()
            lib.set_profile_enable(0)
            streams = keep

    if args.dump_outputs and rank == 0:
        import numpy as np
        os.makedirs(args.dump_outputs, exist_ok=True)
        for name, arr in dump.items():
            np.save(os.path.join(args.dump_outputs, name + ".npy"), arr)

    train = None
    if args.full and not args.no_train:
        try:
            train = train_leg(args, dec, wm, X, caps, clen, prev, plen, dev, dist, rank, world, barrier, max_over_ranks)
        except Exception as e:          # the secondary leg must never take the headline line down with it
            train = {"error": repr(e)[:300]}

    if rank != 0:
        if dist is not None:
            dist.destroy_process_group()
        return

    n_gpus = world
    total_steps = n_gpus * args.steps * STEPS_PER_DECODE
    line = {
        "metric": "decode-steps/sec (B=128, 36x2048 feats, seqlen=20)",
        "value": round(total_steps / elapsed, 2),
        "unit": "decode-steps/sec",
        "n_gpus": n_gpus,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(1e3 * elapsed / args.steps, 4),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "f32",
        "data": "synthetic",
        "single_stream_decode_steps_per_sec": None if single is None else round(args.steps * STEPS_PER_DECODE / single, 2),
        "single_stream_ms_per_step": None if single is None else round(1e3 * single / args.steps, 4),
        # one caller, decodes issued one after the other, through pipeline.DevicePrefetcher(begin_ahead=...): the prologue of
        # decode i+1 overlaps the timestep loop of decode i (second stream + workspace inside the package, nothing else changes
        # for the caller); ids checked against the un-pipelined decode in the same run
        "single_caller_pipelined_decode_steps_per_sec": (pipelined or {}).get("prologue_ahead", {}).get("decode_steps_per_sec"),
        "single_caller_pipelined": pipelined,
        "batches_in_flight_per_gpu": max(1, args.streams),
        "stream_probe_decode_steps_per_sec": stream_probe,
        # SURVEY.md 8d's own bound: 16.88 GFLOP per B=128 timestep against the 157.3 TFLOP/s fp32-MFMA peak (107 us)
        "end_to_end_frac": round(SURVEY_GFLOP_PER_TIMESTEP * 1e9 * (total_steps / elapsed) / n_gpus / (PEAK_FP32_MFMA_TFLOPS * 1e12), 4),
        # the same with the FLOPs the path actually EXECUTES per decode (207.9 GFLOP of step GEMMs with the token
        # table, 46.5 prologue GEMMs, 21.5 encoder recurrence, 5.1 copy gate = 281 GFLOP; SURVEY's 16.88 x 19 = 320.7 counts
        # 5.6 GFLOP per timestep that hoisting removed) / time / peak
        "executed_frac": round(EXECUTED_GFLOP_PER_DECODE * 1e9 * (total_steps / STEPS_PER_DECODE / elapsed) / n_gpus
                               / (PEAK_FP32_MFMA_TFLOPS * 1e12), 4),
        "single_stream_end_to_end_frac": None if single is None else round(
            SURVEY_GFLOP_PER_TIMESTEP * 1e9 * (args.steps * STEPS_PER_DECODE / single) / (PEAK_FP32_MFMA_TFLOPS * 1e12), 4),
        "config": {"workload": "EditNet greedy decode (editnet_rl.py:485-549): prologue + 19 timesteps per bench step",
                   "batch_per_gpu": B, "regions": R, "feat_dim": F, "prev_caption_len": T, "vocab": V,
                   "decoder_dim": D, "attention_dim": A, "timesteps_per_bench_step": STEPS_PER_DECODE,
                   "mode": "eval (loop-invariant projections hoisted)", "parallelism": "dp%d (no collective)" % n_gpus,
                   "us_per_timestep_incl_prologue": round(1e6 * elapsed / (args.steps * STEPS_PER_DECODE), 2),
                   "xe_forward_single_stream_decode_steps_per_sec": None if xe_rate is None else round(xe_rate, 2),
                   "distinct_tokens_in_last_batch": int(torch.unique(seq).numel())},
    }
    if args.full:
        rates = sorted(total_steps / e for e in [first_elapsed] + windows)
        line["repeat"] = {"windows": len(rates), "steps_per_window": args.steps, "median": round(_median(rates), 2),
                          "min": round(rates[0], 2), "max": round(rates[-1], 2), "timed_region_s": round(elapsed, 4),
                          "value_is": "median window" if first_elapsed < 0.5 else "first window",
                          # rounds 1-2 reported the FIRST window; kept as a named field so that round-over-round comparisons
                          # stay like for like
                          "first_window": round(total_steps / first_elapsed, 2)}
    if prof is not None:
        by = {p["tag"]: p for p in prof}
        gemm_tags = sorted((t for t in by if t.startswith("gemm_nt_f32")), key=lambda t: -by[t]["ms"])
        g = by[gemm_tags[0]] if gemm_tags else None      # the dominant kernel = the GEMM tile variant with most time
        if g and g["ms"] > 0:
            tf = g["flops"] / (g["ms"] * 1e-3) / 1e12
            tr = pmc_traffic()
            line["roofline"] = {
                "kernel": gemm_tags[0].replace(">", ",2,2>") + " (v_mfma_f32_32x32x2_f32)", "bound": "mfma",
                "achieved": round(tf, 2), "peak": PEAK_FP32_MFMA_TFLOPS, "unit": "TFLOP/s",
                "frac": round(tf / PEAK_FP32_MFMA_TFLOPS, 4),
                "traffic": None if tr is None else round(tr["traffic_bytes_per_launch"] / 1e6, 2),
                "traffic_unit": "MB HBM per launch (rocprofv3 PMC FETCH_SIZE x2 + WRITE_SIZE, %s)" % (tr or {}).get("file"),
                "algorithmic_MB_per_launch": round(g["bytes"] / g["launches"] / 1e6, 2),
                "traffic_step_launches": _step_traffic(tr),
                "launches": g["launches"], "avg_us_per_launch": round(1e3 * g["ms"] / g["launches"], 2),
                "algorithmic_gflop_per_launch": round(g["flops"] / g["launches"] / 1e9, 4),
                "algorithmic_GBs": round(g["bytes"] / (g["ms"] * 1e-3) / 1e9, 1),
                "timing": "HIP events on the launch stream, second identical pass of %d steps (profiled ms_per_step %.3f)"
                          % (nprof, 1e3 * prof_elapsed / nprof)}
        def _kernel(p):
            gbs, tfl = p["bytes"] / max(p["ms"], 1e-9) / 1e6, p["flops"] / max(p["ms"], 1e-9) / 1e9
            mfma = p["flops"] > 0
            return {"launches_per_step": round(p["launches"] / nprof, 2), "ms_per_step": round(p["ms"] / nprof, 4),
                    "us_per_launch": round(1e3 * p["ms"] / max(p["launches"], 1), 2), "GBs": round(gbs, 1), "TFLOPs": round(tfl, 2),
                    "bound": "mfma" if mfma else "hbm",
                    "frac": round(tfl / PEAK_FP32_MFMA_TFLOPS if mfma else gbs / PEAK_HBM_GBS, 4)}
        line["kernels"] = {p["tag"]: _kernel(p) for p in prof}
    if train is not None:
        line["train"] = train
    if args.full and not args.no_secondary and n_gpus == 1:
        from tools import secondary
        line["secondary"] = secondary.all_secondary(dev)
    if args.full and not args.no_cpu_baseline and n_gpus == 1:
        line["cpu_baseline"] = cpu_baseline()
    if args.full and not args.no_secondary and n_gpus == 1 and os.environ.get("SET_LIB_VARIANT") != "exp":
        line["experimental"] = experimental_leg(args, line)
    print(json.dumps(line))
    if dist is not None:
        dist.destroy_process_group()


def experimental_leg(args, line):
    """NEVER `value`, `dtype` or `roofline`: the same decode with the grouped GEMM's >= 65-row launches on the bf16 matrix pipe
    — every fp32 operand split exactly into three bf16 values while a k-tile is staged, six of the nine partial products
    accumulated in fp32 (csrc/experimental/gemm_variants.inc gemm_nt_split_bf16; error vs fp64 = the fp32 kernel's).  It lives
    in the EXPERIMENTAL build of the library (build.py --exp -> csrc/libset_hip_exp.so), loaded only by a child process with
    SET_LIB_VARIANT=exp; the shipped library does not contain it.  What the fp32-MFMA wall costs the headline."""
    here = os.path.dirname(os.path.abspath(__file__))
    lib = os.path.join(here, "show-edit-tell_amd", "csrc", "libset_hip_exp.so")
    if not os.path.exists(lib):
        return {"skipped": "experimental library not built (python -m show_edit_tell_amd.build --exp)"}
    out = {"what": "emulated-fp32 GEMM on bf16 MFMA (3-way exact split, 6 products, fp32 accumulate), SET_GEMM_SPLIT=1 on the "
                   "experimental library variant; same metric, same workload, child process",
           "fp32_value_this_run": line.get("value")}
    try:
        env = dict(os.environ, SET_LIB_VARIANT="exp", SET_GEMM_SPLIT="1")
        cmd = [sys.executable, os.path.join(here, "bench.py"), "--full", "--no-cpu-baseline", "--no-train", "--no-secondary", "--repeat", "2",
               "--steps", str(max(args.steps, 60)), "--warmup", str(args.warmup)]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=420)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        d = json.loads(lines[-1])
        out.update(value=d["value"], single_stream_decode_steps_per_sec=d.get("single_stream_decode_steps_per_sec"),
                   batches_in_flight_per_gpu=d.get("batches_in_flight_per_gpu"),
                   gemm_us_per_launch={k: v["us_per_launch"] for k, v in d.get("kernels", {}).items() if "gemm_nt" in k},
                   ratio_to_fp32=round(d["value"] / line["value"], 3) if line.get("value") else None)
        # accuracy: max |error| against fp64 over the decode step's three launch shapes, both kernels
        errs = {}
        for mode in ("0", "1"):
            r2 = subprocess.run([sys.executable, os.path.join(here, "tools", "gemm_microbench.py"), "128", "4096", "3072", "128", "10000",
                                 "1024", "128", "4096", "2048"], env=dict(env, SET_GEMM_SPLIT=mode, ITERS="5"), capture_output=True,
                                text=True, timeout=240)
            errs["fp32_mfma" if mode == "0" else "bf16_split"] = [float(ln.split("maxerr")[1]) for ln in r2.stdout.splitlines() if "maxerr" in ln]
        out["max_abs_err_vs_fp64_K3072_K1024_K2048"] = errs
    except Exception as e:
        out["error"] = repr(e)[:300]
    return out


def train_leg(args, dec, wm, X, caps, clen, prev, plen, dev, dist, rank, world, barrier, max_over_ranks):
    """BASELINE.json configs[1]/[2]: EditNet XE training step (editnet.py:558-581) at B=128 per GPU, train mode
    (dropout on, nothing hoisted), forward + backward + bucketed gradient all-reduce (RCCL) + clip 0.25 + Adam.
    Every rank runs the same number of steps; timing is barrier bracketed, max over ranks."""
    import torch
    from show_edit_tell_amd import editnet
    from show_edit_tell_amd.train import xe_train_step
    xe = editnet.DecoderC(wm, D, D, D, A, F)
    xe.load_state_dict(dec.state_dict())
    xe = xe.to(dev)
    opt = torch.optim.Adam(xe.parameters(), lr=5e-4)         # editnet.py:749; clip + step run on set_clip_adam_f32 (optim.py)
    K = max(2, args.train_steps)
    clen_host = clen.cpu()                  # the data loader's host copy of the lengths (editnet.py:560-563 moves them to the device)

    windows = []

    def timed(reduce, n_windows=3):
        """median of n_windows barrier-bracketed windows of K steps (the step is host-launch heavy, so a single short
        window picks up host jitter: 26-37 ms seen for the same build on one box)"""
        for _ in range(3):
            xe_train_step(xe, opt, X, caps, clen, prev, plen, False, 0.0, reduce=reduce, caplens_host=clen_host)
        ts, losses = [], []
        for _ in range(n_windows):
            barrier()
            t0 = time.perf_counter()
            losses += [xe_train_step(xe, opt, X, caps, clen, prev, plen, False, 0.0, reduce=reduce, caplens_host=clen_host)[0]
                       for _ in range(K)]
            barrier()
            ts.append(max_over_ranks(time.perf_counter() - t0))
        windows.append([round(1e3 * t / K, 3) for t in ts])
        return sorted(ts)[len(ts) // 2], losses

    t_dp, losses = timed(True)
    out = {"workload": "EditNet XE training step (editnet.py:558-581): train mode, B=128 per GPU, 19 timesteps, "
                       "fwd + bwd + gradient all-reduce + clip 0.25 + Adam",
           "n_gpus": world, "steps": K, "ms_per_train_step": round(1e3 * t_dp / K, 3), "windows_ms": windows[0],
           "train_decode_steps_per_sec": round(world * K * STEPS_PER_DECODE / t_dp, 2),
           "gradient_MB": round(sum(p.numel() for p in xe.parameters()) * 4 / 1e6, 1),
           # 1.23 TFLOP of contractions per step (forward as executed + backward)
           "achieved_TFLOPs_per_gpu": round(TRAIN_TFLOP_PER_STEP / (t_dp / K), 1),
           "frac_of_fp32_mfma_peak": round(TRAIN_TFLOP_PER_STEP / (t_dp / K) / PEAK_FP32_MFMA_TFLOPS, 4),
           "loss_first": round(losses[0], 4), "loss_last": round(losses[-1], 4)}
    if world > 1:
        t_local, _ = timed(False)
        # the collective alone: the step's flat gradient buckets (`.grad` are views of them) all-reduced back to back
        from show_edit_tell_amd.train import _all_reduce_sum
        fb = xe.__dict__.get("_grad_buckets")
        ar_ms = None
        if fb is not None:
            for _ in range(2):
                for f in fb.flat:
                    _all_reduce_sum(dist, f, None)
            barrier()
            t0 = time.perf_counter()
            for _ in range(5):
                works = [_all_reduce_sum(dist, f, None, async_op=True) for f in fb.flat]
                for w_ in works:
                    if w_ is not None:
                        w_.wait()
            barrier()
            ar_ms = round(1e3 * max_over_ranks(time.perf_counter() - t0) / 5, 3)
        # which devices / backend the ranks really ran on (all-gathered)
        seen = [None] * world
        dist.all_gather_object(seen, {"rank": rank, "device": torch.cuda.current_device(),
                                      "name": torch.cuda.get_device_name(), "backend": dist.get_backend()})
        # the collective library and the fabric the ranks talk over (rank 0's view; best effort, never fatal)
        fabric = {}
        if rank == 0:
            try:
                fabric["rccl_version"] = ".".join(str(v) for v in torch.cuda.nccl.version())
            except Exception as e:
                fabric["rccl_version"] = "unavailable: %r" % (e,)
            for key in ("NCCL_DEBUG", "RCCL_MSCCL_ENABLE", "NCCL_ALGO", "NCCL_PROTO", "HSA_ENABLE_IPC_MODE_LEGACY"):
                if key in os.environ:
                    fabric[key] = os.environ[key]
            try:
                topo = subprocess.run(["rocm-smi", "--showtopo"], capture_output=True, text=True, timeout=60).stdout
                # keep the link-type and hop tables, drop banners
                keep = [ln for ln in topo.splitlines() if ln.strip() and not set(ln.strip()) <= set("=-")]
                fabric["rocm_smi_showtopo"] = keep[:80]
            except Exception as e:
                fabric["rocm_smi_showtopo"] = "unavailable: %r" % (e,)
        out["fabric"] = fabric
        out.update(ms_per_train_step_no_allreduce=round(1e3 * t_local / K, 3),
                   allreduce_exposed_ms=round(1e3 * (t_dp - t_local) / K, 3), allreduce_ms=ar_ms,
                   allreduce_buckets=None if fb is None else [round(f.numel() * 4 / 1e6, 1) for f in fb.flat],
                   ranks_seen=seen,
                   allreduce="SUM all-reduce in place on persistent flat gradient buckets (`.grad` tensors are views), "
                             "fc's bucket launched at the start of the backward, the others as the deferred weight-gradient "
                             "contractions finish (train.FlatGradBuckets / BucketedAllReduce)")
    del opt, xe
    torch.cuda.empty_cache()
    if world == 1 and not args.no_secondary:
        # the exchange step on a ONE-rank RCCL group (tools/rccl_one_rank.py), in a child process with a timeout: what the
        # collectives cost before any byte crosses xGMI — the baseline for an N > 1 run's allreduce_exposed_ms / allreduce_ms
        try:
            r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools", "rccl_one_rank.py"),
                                "--steps", str(K)], capture_output=True, text=True, timeout=300)
            lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
            out["one_rank_rccl"] = json.loads(lines[-1]) if lines else {"error": (r.stderr or r.stdout)[-300:]}
        except Exception as e:
            out["one_rank_rccl"] = {"error": repr(e)[:300]}
    return out


if __name__ == "__main__":
    main()
