"""Raw bytes of the device metrics' records and scores (csrc/ciderd_device.hip, csrc/bleu_device.hip, csrc/rouge_device.hip,
csrc/editdist_device.hip), for comparing two builds of the library (a refactor against its parent).

    python tools/metric_bits.py --out new.npz                                     (on the GPU, once per build)
    python tools/metric_bits.py --compare parent.npz new.npz [--json verdict.json]

Only the public C ABI is used (include/set_hip.h set_ciderd_device_*, set_bleu_device_*, set_rouge_device_score and
set_edit_device_*, through _lib's prototypes), so the file runs unchanged in a checkout of an older commit.  Dumped, each under both length conventions (rows cut after their first
0; explicit lengths, among them a negative one and one beyond L):
  set_ciderd_device_vectorise records and set_ciderd_device_score scores and pairs for n = 1, 2, 4;
  set_bleu_device_prepare records and set_bleu_device_score statistics, scores and pairs;
  set_rouge_device_score (beta 1.2) and set_edit_device_score statistics, scores and pairs from those records;
  set_edit_device_align statistics, hyp_ops, hyp_src and src_ops of the hypotheses against the reference rows as sources.
Inputs, on fixed seeds: 72 reference rows and 72 hypotheses (near-copies of references) with lengths 0, 1, 2, 3, 4, 5, 63, 64
rotating, ids 1..6 so that counts repeat, a few ids up to 65533, one of 65534 (a row the packing refuses) and one row with three such ids in a row, a 0 and junk
behind every row's length, a leading dimension of 70 for L = 64; reference sets of 0 (CIDEr-D only), 1 and 5 references; one
set index outside the sets; a df table built from the references' 1..4-grams.  Every output buffer is filled with a sentinel
first, so bytes that a build leaves alone compare too.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

L, LD, ROWS, MAX_SET, PAIR_LD = 64, 70, 72, 5, 6
LENGTHS = (0, 1, 2, 3, 4, 5, 63, 64)
BETA = 1.2
SENTINEL = -0x0123456789ABCDEF
DEV = "cuda:0"


def rows(seed):
    """(ROWS, LD) ids: LENGTHS[r % 8] ids of 1..6, a 0 behind them, junk behind the 0 and in the columns beyond L"""
    rng = np.random.default_rng(seed)
    H = rng.integers(1, 7, (ROWS, LD)).astype(np.int64)
    n = np.array([LENGTHS[r % len(LENGTHS)] for r in range(ROWS)])
    for r in range(ROWS):
        if n[r] < L:
            H[r, n[r]] = 0
    return H, n


def inputs():
    rng = np.random.default_rng(77)
    refs, ref_n = rows(21)
    for r, c, w in ((6, 10, 65533), (7, 3, 40000), (14, 0, 65533), (15, 62, 12345), (23, 63, 65533)):
        refs[r, c] = w
    refs[31, 5] = 65534                                             # cannot be packed: that row is refused
    refs[39, 10:13] = (65534, -1, 70000)                            # grams of order 2 and 3 made of such ids alone: key 0
    hyps, hyp_n = refs.copy(), ref_n.copy()                         # near-copies: many shared grams, clipped counts
    hyps = np.roll(hyps, 8, axis=0)                                 # the same length class, another row
    for r in range(ROWS):
        for _ in range(int(rng.integers(0, 4))):
            if hyp_n[r]:
                hyps[r, int(rng.integers(0, hyp_n[r]))] = int(rng.integers(1, 7))
    hyps[44, 2] = 65534
    given = lambda n: np.where(np.arange(ROWS) == 9, -3, np.where(np.arange(ROWS) == 15, LD, n)).astype(np.int32)

    def offsets(sizes):
        off = [0]
        while off[-1] + sizes[(len(off) - 1) % len(sizes)] <= ROWS:
            off.append(off[-1] + sizes[(len(off) - 1) % len(sizes)])
        return np.asarray(off, dtype=np.int64)
    off_cd, off_bl = offsets((0, 1, 5)), offsets((1, 5))

    def set_of(off):
        s = (np.arange(ROWS) % (len(off) - 1)).astype(np.int32)
        s[5], s[50] = len(off) - 1, -1                              # outside the sets
        return s
    # df table: every 1..4-gram of the first 20 references as the 0 rule cuts them, counted per group of 5 rows ("documents");
    # the other references hold grams that the table never saw
    df = {}
    for d in range(0, 20, 5):
        seen = set()
        for r in range(d, d + 5):
            s = refs[r, :min(ref_n[r] + 1, L)].tolist()
            for k in range(1, 5):
                seen.update(tuple(s[i:i + k]) for i in range(len(s) - k + 1))
        for g in seen:
            if max(g) < 65534:
                df[g] = df.get(g, 0) + 1
    grams = sorted(df)
    toks = np.zeros((len(grams), 4), dtype=np.int64)
    for i, g in enumerate(grams):
        toks[i, :len(g)] = g
    return dict(refs=refs, ref_lens=given(ref_n), hyps=hyps, hyp_lens=given(hyp_n), off_cd=off_cd, off_bl=off_bl,
                set_cd=set_of(off_cd), set_bl=set_of(off_bl), df_tok=toks, df_len=np.array([len(g) for g in grams], dtype=np.int32),
                df_cnt=np.array([df[g] for g in grams], dtype=np.float64), docs=4.0)


def run(out):
    import torch
    from show_edit_tell_amd import _lib
    lib = _lib.load()
    st = lambda: _lib.stream_of(torch.device(DEV))
    x = inputs()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    buf = lambda n, dt: torch.full((n,), SENTINEL, dtype=torch.int64, device=DEV).view(dt)
    ptr = lambda t: None if t is None else t.data_ptr()
    refs, hyps = dev(x["refs"]), dev(x["hyps"])
    lens = {"zero_rule": (None, None), "lengths": (dev(x["ref_lens"]), dev(x["hyp_lens"]))}
    res = {"input/" + k: v for k, v in x.items() if isinstance(v, np.ndarray)}
    raw = lambda t: t.cpu().numpy().view(np.uint8)
    for n in (1, 2, 4):
        h = C.c_void_p()
        _lib.check(lib.set_ciderd_device_create(x["df_tok"].ctypes.data, x["df_len"].ctypes.data, x["df_cnt"].ctypes.data,
                                                len(x["df_len"]), x["docs"], n, 6.0, st(), C.byref(h)), "set_ciderd_device_create")
        off, so = dev(x["off_cd"]), dev(x["set_cd"])
        for conv, (rl, hl) in lens.items():
            tag = "ciderd/n%d/%s/" % (n, conv)
            words = ROWS * (8 + 8 * L)
            assert lib.set_ciderd_device_vec_bytes(ROWS, L) == 8 * words
            recs = buf(words, torch.int64)
            _lib.check(lib.set_ciderd_device_vectorise(h, refs.data_ptr(), LD, ptr(rl), ROWS, L, recs.data_ptr(), st()),
                       "set_ciderd_device_vectorise")
            scores, pairs = buf(ROWS, torch.float64), buf(ROWS * PAIR_LD, torch.float64)
            _lib.check(lib.set_ciderd_device_score(h, hyps.data_ptr(), LD, ptr(hl), ROWS, L, so.data_ptr(), recs.data_ptr(), L,
                                                   int(x["off_cd"][-1]), off.data_ptr(), len(x["off_cd"]) - 1, MAX_SET,
                                                   scores.data_ptr(), pairs.data_ptr(), PAIR_LD, st()), "set_ciderd_device_score")
            torch.cuda.synchronize()
            res[tag + "records"], res[tag + "scores"], res[tag + "pairs"] = raw(recs), raw(scores), raw(pairs)
        lib.set_ciderd_device_destroy(h)
    off, so = dev(x["off_bl"]), dev(x["set_bl"])
    for conv, (rl, hl) in lens.items():
        tag = "bleu/%s/" % conv
        words = ROWS * (8 + 4 * L)
        assert lib.set_bleu_device_ref_bytes(ROWS, L) == 8 * words
        recs = buf(words, torch.int64)
        _lib.check(lib.set_bleu_device_prepare(refs.data_ptr(), LD, ptr(rl), ROWS, L, recs.data_ptr(), st()), "set_bleu_device_prepare")
        stats = buf(ROWS * 5, torch.int32)                           # 10 int32 per row
        scores, pairs = buf(ROWS * 4, torch.float64), buf(ROWS * PAIR_LD, torch.float64)
        _lib.check(lib.set_bleu_device_score(hyps.data_ptr(), LD, ptr(hl), ROWS, L, so.data_ptr(), recs.data_ptr(), L,
                                             int(x["off_bl"][-1]), off.data_ptr(), len(x["off_bl"]) - 1, MAX_SET, stats.data_ptr(),
                                             scores.data_ptr(), pairs.data_ptr(), PAIR_LD, st()), "set_bleu_device_score")
        torch.cuda.synchronize()
        res[tag + "records"], res[tag + "stats"], res[tag + "scores"], res[tag + "pairs"] = raw(recs), raw(stats), raw(scores), raw(pairs)
        for name, extra in (("rouge", (BETA,)), ("edit", ())):       # the two other readers of BLEU's records
            entry = "set_%s_device_score" % name
            stats = buf(ROWS * 2, torch.int32)                       # 4 int32 per row
            scores, pairs = buf(ROWS, torch.float64), buf(ROWS * PAIR_LD, torch.float64)
            _lib.check(getattr(lib, entry)(hyps.data_ptr(), LD, ptr(hl), ROWS, L, so.data_ptr(), recs.data_ptr(), L, int(x["off_bl"][-1]),
                                           off.data_ptr(), len(x["off_bl"]) - 1, MAX_SET, *extra, stats.data_ptr(), scores.data_ptr(),
                                           pairs.data_ptr(), PAIR_LD, st()), entry)
            torch.cuda.synchronize()
            res["%s/%s/stats" % (name, conv)], res["%s/%s/scores" % (name, conv)], res["%s/%s/pairs" % (name, conv)] = raw(stats), raw(scores), raw(pairs)
        # the hypotheses against the reference rows as sources: 8 int32 of statistics, L int8 + L int32 + L int8 per row
        stats, hyp_ops, hyp_src, src_ops = buf(ROWS * 4, torch.int32), buf(ROWS * L // 8, torch.int8), buf(ROWS * L // 2, torch.int32), buf(ROWS * L // 8, torch.int8)
        _lib.check(lib.set_edit_device_align(hyps.data_ptr(), LD, ptr(hl), ROWS, L, refs.data_ptr(), LD, ptr(rl), L, stats.data_ptr(),
                                             hyp_ops.data_ptr(), L, hyp_src.data_ptr(), src_ops.data_ptr(), L, st()), "set_edit_device_align")
        torch.cuda.synchronize()
        tag = "edit_align/%s/" % conv
        res[tag + "stats"], res[tag + "hyp_ops"], res[tag + "hyp_src"], res[tag + "src_ops"] = raw(stats), raw(hyp_ops), raw(hyp_src), raw(src_ops)
    # the inputs do what they are there for: finite and refused rows, counts above 1, both set sizes
    s = res["ciderd/n4/zero_rule/scores"].view(np.float64)
    b = res["bleu/zero_rule/stats"].view(np.int32).reshape(ROWS, 10)
    assert np.isnan(s).sum() >= 3 and (s[~np.isnan(s)] > 0).sum() > 10, s
    assert (b[:, 0] == -1).sum() >= 3 and (b[:, 1] > 0).sum() > 20 and (b[:, 3] > 0).sum() > 5 and b[:, 8].max() == 64, b
    # ROUGE-L and edit distance: refused rows, common subsequences, distance 0 and above, a chosen reference that is not the first of 5
    r = res["rouge/zero_rule/stats"].view(np.int32).reshape(ROWS, 4)
    e = res["edit/zero_rule/stats"].view(np.int32).reshape(ROWS, 4)
    a = res["edit_align/zero_rule/stats"].view(np.int32).reshape(ROWS, 8)
    five = np.diff(x["off_bl"])[np.clip(x["set_bl"], 0, len(x["off_bl"]) - 2)] == 5
    assert (r[:, 0] == -1).sum() >= 3 and (r[:, 0] > 0).sum() > 20 and (r[:, 3] > 0).sum() > 20, r
    assert (e[:, 0] == -1).sum() >= 3 and (e[:, 0] == 0).sum() >= 1 and (e[:, 0] > 0).sum() > 20 and (e[five, 3] > 0).sum() >= 3, e
    assert (a[:, 0] == -1).sum() >= 2 and (a[:, 0] > 0).sum() > 20 and (a[:, 4] > 0).sum() > 5 and (a[:, 5] + a[:, 6] > 0).sum() > 5, a
    np.savez_compressed(out, **res)
    print("metric_bits: %d arrays -> %s" % (len(res), out))


def compare(fa, fb, js):
    a, b = np.load(fa), np.load(fb)
    names = sorted(set(a.files) | set(b.files))
    per = {}
    for n in names:
        same = n in a.files and n in b.files and a[n].shape == b[n].shape and a[n].dtype == b[n].dtype and np.array_equal(a[n], b[n])
        per[n] = "identical" if same else "DIFFERENT"
    bad = [n for n in names if per[n] != "identical"]
    verdict = ("identical" if not bad else "DIFFERENT") + ": %d arrays, %d bytes" % (len(names), sum(a[n].nbytes for n in a.files))
    print("metric_bits:", verdict)
    for n in bad:
        print("  differs:", n)
    if js:
        with open(js, "w") as f:
            json.dump({"tool": "tools/metric_bits.py --compare A B --json FILE; dumps written by --out on one GPU, one per build",
                       "verdict": verdict, "different": bad, "arrays": per}, f, indent=1)
            f.write("\n")
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2)
    ap.add_argument("--json")
    ns = ap.parse_args()
    if ns.compare:
        sys.exit(compare(ns.compare[0], ns.compare[1], ns.json))
    run(ns.out)
