"""Raw output bits of the vocabulary-row picks, for comparing two builds of the library (a refactor against its parent).

    python tools/pick_bits.py --out new.npz [--lib path/to/libset_hip.so] [--family pick|beam]      (on the GPU, once per build)
    python tools/pick_bits.py --compare parent.npz new.npz [--json verdict.json]

Only the public C ABI of include/set_hip.h is used, so the tool runs unchanged on an older commit's library.  Inputs are random
normal logits (rounding order shows, unlike the integer-valued rows of the exact tests) on fixed seeds.  The beam/* family drives
every per-step beam pick as a chain of BEAM_STEPS steps from cur_len = 1 with the pick's own outputs fed back, every output array
recorded after every step: at V = 5 <end> is picked often, so a chain crosses completions, a shrinking k_left, finished images, a
full completion list and, under the "tight" constraints (one word left beside <end>, which min_len holds back), an exhausted group.
"""
import argparse
import ctypes as C
import itertools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VS = (5, 1023, 1025, 9490, 12288, 12289)
OPTS = tuple((temp, k, pp) for temp in (1.0, 0.7) for k, pp in ((0, 1.0), (7, 1.0), (0, 0.9), (7, 0.5)))
B, K, D, LMAX, MAXLEN = 3, 3, 8, 4, 4
# what the run cannot reach through the public entries (written into the verdict file)
NOT_COMPARED = ["gumbel_pick_k with a tail, several slabs or a bias: set_gumbel_pick_f32 takes one slab and neither; those instantiations "
                "are compared only through the whole-decode tests",
                "beam/*: the persistent beam kernels' pb_pick (its own file, LDS state and history format; not a per-step pick)",
                "beam/*: the return codes of refused arguments (no output array; tests/test_beam_constrained_cpu.py, "
                "tests/test_beam_diverse_cpu.py and tests/test_nbest_beam_cpu.py pin them without a device)"]
BEAM_VS, BEAM_KS, BEAM_GROUPS, BEAM_NI, BEAM_STEPS, BEAM_LMAX = (5, 1023, 1025, 9490), (1, 3, 8), ((4, 2), (6, 3), (8, 1)), 3, 6, 8


def lds(V):
    """the padded leading dimension (register path up to 12288 words) and one that is no multiple of 4 (scalar path)"""
    return ((V + 63) // 64 * 64, V + 1 if (V + 1) & 3 else V + 2)


class Opts(C.Structure):
    _fields_ = [("temperature", C.c_float), ("top_k", C.c_int32), ("top_p", C.c_float), ("pad_", C.c_int32)]


class Tail(C.Structure):
    _fields_ = [("g0", C.c_void_p), ("g0_stride", C.c_int64), ("g0_ld", C.c_int64), ("pre", C.c_void_p), ("ldpre", C.c_int64),
                ("tab", C.c_void_p), ("ld_tab", C.c_int64), ("c_in", C.c_void_p), ("c_out", C.c_void_p), ("h_out", C.c_void_p),
                ("g0_n", C.c_int32), ("col0", C.c_int32), ("nrows", C.c_int32), ("D", C.c_int32)]


class PickArgs(C.Structure):
    _fields_ = [("logits", C.c_void_p), ("ld", C.c_int64), ("stride", C.c_int64), ("bias", C.c_void_p), ("end_idx", C.c_int64),
                ("seq", C.c_void_p), ("seq_logp", C.c_void_p), ("it", C.c_void_p), ("unfinished", C.c_void_p), ("alive", C.c_void_p),
                ("table", C.c_void_p), ("emb_out", C.c_void_p), ("seed", C.c_uint64), ("offset", C.c_uint64),
                ("raw_ids", C.c_void_p), ("lse", C.c_void_p), ("step_logp", C.c_void_p), ("tail", C.c_void_p),
                ("n", C.c_int32), ("B", C.c_int32), ("V", C.c_int32), ("t", C.c_int32), ("max_len", C.c_int32), ("D", C.c_int32),
                ("mode", C.c_int32), ("pad_", C.c_int32)]


class Cons(C.Structure):
    _fields_ = [("no_repeat_ngram", C.c_int32), ("min_len", C.c_int32), ("length_alpha", C.c_float), ("n_banned", C.c_int32),
                ("banned", C.c_void_p)]


class SbsArgs(C.Structure):
    _fields_ = [("logits", C.c_void_p), ("ld", C.c_int64), ("end_idx", C.c_int64), ("seed", C.c_uint64), ("offset", C.c_uint64),
                ("phi", C.c_void_p), ("G", C.c_void_p), ("finished", C.c_void_p), ("len", C.c_void_p), ("seqs_in", C.c_void_p),
                ("seqs_out", C.c_void_p), ("words", C.c_void_p), ("rows", C.c_void_p), ("n_open", C.c_void_p), ("ws", C.c_void_p),
                ("ws_bytes", C.c_size_t), ("NI", C.c_int32), ("k", C.c_int32), ("V", C.c_int32), ("t", C.c_int32), ("Lmax", C.c_int32),
                ("pad_", C.c_int32)]


def raw(t):
    a = t.detach().cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.float32 else a


def run_beam(lib, res, check, p, dev):
    """beam/<entry>/m<models>/V/ld/k/G/s<step>/<array>: plain, n-best, constrained and diverse (neutral, live, tight) picks"""
    import torch
    lib.set_beam_pick_constrained_workspace_bytes.restype = C.c_size_t
    gen = torch.Generator().manual_seed(20261020)
    NI, L = BEAM_NI, BEAM_LMAX
    banned = torch.tensor([1, 2, 0], dtype=torch.int64, device=dev)
    cons = {"neutral": Cons(0, 0, 0.0, 0, None), "live": Cons(2, 2, 0.7, 2, banned.data_ptr()), "tight": Cons(2, 4, 0.7, 3, banned.data_ptr())}
    entries = [(e, k, 1) for e in ("pick", "nbest", "cons_neutral", "cons_live", "cons_tight") for k in BEAM_KS]
    entries += [(e, k, G) for e in ("div_neutral", "div_live", "div_tight") for k, G in BEAM_GROUPS]
    i32, i64, neg = torch.int32, torch.int64, float("-inf")
    for V, nm, (entry, k, G) in itertools.product(BEAM_VS, (1, 2), entries):
        for ld in lds(V):
            g, end = k // G, min(3, V - 1)
            o = dict(scores=torch.full((NI, k), neg, device=dev), k_left=torch.full((NI,), k, dtype=i32, device=dev),
                     best_score=torch.full((NI,), neg, device=dev), best_seq=torch.zeros(NI, L, dtype=i64, device=dev),
                     best_len=torch.zeros(NI, dtype=i32, device=dev), words=torch.zeros(NI * k, dtype=i64, device=dev),
                     rows=torch.zeros(NI * k, dtype=i32, device=dev))
            o["scores"][:, ::g] = 0.0
            seqs = [torch.zeros(NI, k, L, dtype=i64, device=dev) for _ in range(2)]
            if entry != "pick":
                o.update(done_score=torch.full((NI, k), neg, device=dev), done_seq=torch.zeros(NI, k, L, dtype=i64, device=dev),
                         done_len=torch.zeros(NI, k, dtype=i32, device=dev), n_done=torch.zeros(NI, dtype=i32, device=dev))
            if entry.startswith("div"):
                o.update(done_group=torch.zeros(NI, k, dtype=i32, device=dev), g_left=torch.full((NI, G), g, dtype=i32, device=dev))
            ws_bytes = lib.set_beam_pick_constrained_workspace_bytes(NI, k)
            ws = torch.zeros(max(ws_bytes, 16), dtype=torch.uint8, device=dev)
            for step in range(1, BEAM_STEPS + 1):
                lg = [(torch.randn(NI * k, ld, generator=gen, dtype=torch.float32) * 2.0).to(dev) for _ in range(nm)]
                tag = "beam/%s/m%d/V%d/ld%d/k%d/G%d/s%d" % (entry, nm, V, ld, k, G, step)
                head = (p(lg[0]), p(lg[1]) if nm == 2 else None, C.c_int64(ld), NI, k, V, C.c_int64(end), step, L, p(o["scores"]),
                        p(o["k_left"]), p(seqs[0]), p(seqs[1]), p(o["best_score"]), p(o["best_seq"]), p(o["best_len"]), p(o["words"]),
                        p(o["rows"]))
                done = tuple(p(o[n]) for n in ("done_score", "done_seq", "done_len", "n_done")) if entry != "pick" else ()
                tail = (C.byref(cons[entry.split("_")[-1]]), p(ws), C.c_size_t(ws_bytes), None) if "_" in entry else ()
                if entry == "pick":
                    check(lib.set_beam_pick_f32(*head, None), tag)
                elif entry == "nbest":
                    check(lib.set_beam_pick_nbest_f32(*head, *done, None), tag)
                elif entry.startswith("cons"):
                    check(lib.set_beam_pick_constrained_f32(*head, *done, *tail), tag)
                else:
                    check(lib.set_beam_pick_diverse_f32(*head, *done, p(o["done_group"]), p(o["g_left"]), G, C.c_float(0.5), *tail), tag)
                seqs.reverse()
                for n, v in list(o.items()) + [("seqs", seqs[0]), ("seqs_other", seqs[1])]:
                    res[tag + "/" + n] = raw(v)


def run(lib_path, out, family):
    import torch
    lib = C.CDLL(lib_path)
    lib.set_sbs_workspace_bytes.restype = C.c_size_t
    dev = "cuda:0"
    res = {}
    gen = torch.Generator().manual_seed(20261019)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float32).to(dev)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None

    def check(rc, tag):
        torch.cuda.synchronize()
        assert rc == 0, (tag, rc)

    if family in ("all", "beam"):
        run_beam(lib, res, check, p, dev)
    if family in ("all", "pick"):
        run_pick(lib, res, check, p, rnd, dev)
    np.savez_compressed(out, **res)
    print("pick_bits: %d arrays -> %s" % (len(res), out))


def run_pick(lib, res, check, p, rnd, dev):
    import torch
    for V in VS:
        for ld in lds(V):
            for n, with_bias, with_tail in itertools.product((1, 3), (False, True), (False, True)):
                logits = rnd(n, B, ld) * 2.0
                bias = rnd(V) if with_bias else None
                table = rnd(V, D)
                g0, pre, tab, c_in = rnd(2, B, 4 * D), rnd(B, 4 * D), rnd(V, 4 * D), rnd(B, D)
                # greedy and sampled (every option set) through set_pick_slabs*; the Gumbel-max pick has its own entry, which takes one
                # slab and neither bias nor tail (temperature only)
                modes = [("greedy", 0, None)] + [("sample", 1, o) for o in OPTS]
                if n == 1 and not with_bias and not with_tail:
                    modes += [("gumbel", 1, o) for o in OPTS if o[1] == 0 and o[2] == 1.0]
                for name, mode, o in modes:
                    for t in (0, 2, 3):                  # t = 3: alive[2] == 0, the loop has been left
                        tag = "pick/%s/V%d/ld%d/n%d/b%d/tail%d/t%d/%s" % (name, V, ld, n, with_bias, with_tail, t, o)
                        seq = torch.zeros(B, MAXLEN, dtype=torch.int64, device=dev)
                        seq_logp = torch.zeros(B, MAXLEN, device=dev)
                        it = torch.ones(B, dtype=torch.int64, device=dev)
                        unf = torch.tensor([1, 0, 1], dtype=torch.int32, device=dev)
                        alive = torch.tensor([3, 2, 0, 0], dtype=torch.int32, device=dev)
                        emb = torch.zeros(B, D, device=dev)
                        ids = torch.zeros(B, dtype=torch.int64, device=dev)
                        lse, slp = torch.zeros(B, device=dev), torch.zeros(B, device=dev)
                        c_out, h_out = torch.zeros(B, D, device=dev), torch.zeros(B, D, device=dev)
                        tl = Tail(p(g0), B * 4 * D, 4 * D, p(pre), 4 * D, p(tab), 4 * D, p(c_in), p(c_out), p(h_out), 2, 0, V, D)
                        a = PickArgs(p(logits), ld, B * ld, p(bias), min(3, V - 1), p(seq), p(seq_logp), p(it), p(unf), p(alive),
                                     p(table), p(emb), 77, 5, p(ids), p(lse), p(slp),
                                     C.cast(C.pointer(tl), C.c_void_p) if with_tail else None, n, B, V, t, MAXLEN, D, mode, 0)
                        if name == "greedy":
                            check(lib.set_pick_slabs_f32(C.byref(a), None), tag)
                        elif name == "sample":
                            op = Opts(o[0], o[1], o[2], 0)
                            check(lib.set_pick_slabs_opts_f32(C.byref(a), C.byref(op), None), tag)
                        else:
                            op = Opts(o[0], o[1], o[2], 0)
                            check(lib.set_gumbel_pick_f32(p(logits), C.c_int64(ld), B, V, t, MAXLEN, C.c_int64(min(3, V - 1)), C.c_uint64(77),
                                                          C.c_uint64(5), p(seq), p(it), p(unf), p(alive), p(ids), p(lse), p(slp), None,
                                                          C.byref(op)), tag)
                        for k, v in (("seq", seq), ("seq_logp", seq_logp), ("it", it), ("unfinished", unf), ("alive", alive), ("emb", emb),
                                     ("raw_ids", ids), ("lse", lse), ("step_logp", slp), ("c_out", c_out), ("h_out", h_out)):
                            res[tag + "/" + k] = raw(v)
        # stochastic beam search: one image x K slots, one and two models, plain and *_opts entries
        for ld in lds(V):
            l1, l2 = rnd(K, ld) * 2.0, rnd(K, ld) * 2.0
            ws_bytes = lib.set_sbs_workspace_bytes(1, K)
            ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=dev)
            for ens, o, t in itertools.product((False, True), OPTS, (0, 2)):
                trunc = o[1] != 0 or o[2] != 1.0
                tag = "sbs/%s/V%d/ld%d/t%d/%s" % ("ens" if ens else "one", V, ld, t, o)
                live = 1 if t == 0 else K
                phi = torch.tensor([0.0, -1.5, -2.25][:K], device=dev)
                G = torch.tensor([0.0, -0.5, -1.75][:K], device=dev)
                if t == 0:
                    G[1:] = float("-inf")
                fin = torch.zeros(K, dtype=torch.int32, device=dev)
                ln = torch.full((K,), t, dtype=torch.int32, device=dev)
                s_in = torch.arange(K * LMAX, dtype=torch.int64, device=dev).reshape(1, K, LMAX) % max(V - 1, 1) + (1 if V > 1 else 0)
                s_out = torch.zeros(1, K, LMAX, dtype=torch.int64, device=dev)
                words = torch.zeros(K, dtype=torch.int64, device=dev)
                rows = torch.zeros(K, dtype=torch.int32, device=dev)
                n_open = torch.tensor([live], dtype=torch.int32, device=dev)
                a = SbsArgs(p(l1), ld, min(3, V - 1), 99, 3, p(phi), p(G), p(fin), p(ln), p(s_in), p(s_out), p(words), p(rows),
                            p(n_open), p(ws), ws_bytes, 1, K, V, t, LMAX, 0)
                op = Opts(o[0], o[1], o[2], 0)
                if ens:
                    f = lib.set_sbs_pick_ensemble_opts_f32 if trunc else lib.set_sbs_pick_ensemble_f32
                    check(f(C.byref(a), p(l2), C.byref(op), None), tag)
                else:
                    f = lib.set_sbs_pick_opts_f32 if trunc else lib.set_sbs_pick_f32
                    check(f(C.byref(a), C.byref(op), None), tag)
                for k, v in (("phi", phi), ("G", G), ("finished", fin), ("len", ln), ("seqs", s_out), ("words", words), ("rows", rows),
                             ("n_open", n_open)):
                    res[tag + "/" + k] = raw(v)
    # kept_key is an output of the sampled pick's own entry
    for V, o in itertools.product(VS, OPTS):
        ld = (V + 63) // 64 * 64
        logits = rnd(B, ld) * 2.0
        outs = dict(seq=torch.zeros(B, MAXLEN, dtype=torch.int64, device=dev), it=torch.ones(B, dtype=torch.int64, device=dev),
                    unf=torch.ones(B, dtype=torch.int32, device=dev), alive=torch.zeros(MAXLEN, dtype=torch.int32, device=dev),
                    ids=torch.zeros(B, dtype=torch.int64, device=dev), lse=torch.zeros(B, device=dev), slp=torch.zeros(B, device=dev),
                    key=torch.zeros(B, dtype=torch.int32, device=dev))
        op = Opts(o[0], o[1], o[2], 0)
        tag = "key/V%d/%s" % (V, o)
        check(lib.set_sample_pick_opts_key_f32(p(logits), C.c_int64(ld), B, V, 0, MAXLEN, C.c_int64(min(3, V - 1)), C.c_uint64(7), C.c_uint64(1),
                                               p(outs["seq"]), p(outs["it"]), p(outs["unf"]), p(outs["alive"]), p(outs["ids"]),
                                               p(outs["lse"]), p(outs["slp"]), None, C.byref(op), p(outs["key"])), tag)
        for k, v in outs.items():
            res[tag + "/" + k] = raw(v)


def compare(fa, fb, js):
    a, b = np.load(fa), np.load(fb)
    names = sorted(set(a.files) | set(b.files))
    bad = [n for n in names if n not in a.files or n not in b.files or a[n].shape != b[n].shape or not np.array_equal(a[n], b[n])]
    kinds = sorted({n.rsplit("/", 1)[1] for n in names})
    verdict = "identical: %d arrays" % len(names) if not bad else "DIFFERENT: %d of %d arrays" % (len(bad), len(names))
    print("pick_bits:", verdict)
    for n in bad[:40]:
        print("  differs:", n)
    if js:
        with open(js, "w") as f:
            cases = sorted({n.rsplit("/", 1)[0] for n in names})
            json.dump({"tool": "tools/pick_bits.py --compare A B --json FILE; A, B written by --out on one GPU from two builds",
                       "verdict": verdict, "arrays": len(names), "cases": len(cases),
                       "cases_by_entry": {e: sum(c.startswith(e + "/") for c in cases) for e in sorted({c.split("/V")[0] for c in cases})},
                       "outputs": kinds, "not_compared": NOT_COMPARED, "different": bad}, f, indent=1)
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--lib", default=os.path.join(ROOT, "show-edit-tell_amd", "csrc", "libset_hip.so"))
    ap.add_argument("--compare", nargs=2)
    ap.add_argument("--json")
    ap.add_argument("--family", default="all", choices=("all", "pick", "beam"))
    ns = ap.parse_args()
    if ns.compare:
        sys.exit(compare(ns.compare[0], ns.compare[1], ns.json))
    run(ns.lib, ns.out, ns.family)
