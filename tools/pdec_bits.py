"""Raw bits of every output of the persistent decode launches (csrc/decode_persistent.hip, decode_persistent_wide.hip,
decode_persistent_ensemble.hip), for comparing two states of the kernels (a refactor against its parent), in the manner of
tools/pick_bits.py and tools/seq_bits.py.

    python tools/pdec_bits.py --out new.json                      (on the GPU, once per tree)
    python tools/pdec_bits.py --compare parent.json new.json

Only the models' public entry points are used, so the file runs unchanged in a checkout of an older commit.  Every case runs
once with fixed seeds on the synthetic full-size models of the persistent benchmarks (D = 1024, A = 512: the dimensions the
launches accept) and dumps tokens, log-probs / scores (fp32 as their uint32 bits), n-best lists and the profile tags of the
call (`persistent_*`: the launch was taken; --compare fails on a case without one).  The beam entries also dump the launch's
own output buffers as the device wrote them (`beam_raw`: history words, parents and — n-best — scores of every pick made and
slot < k, the result words, best word and best score), read where evaluate.py reads them back.
Cases: EditNet greedy at 1, 3, 16 rows; EditNet teacher-forced forward; EditNet beam + n-best at k = 1, 3, 4 (fixed features)
and k = 3 over adaptive features with 100 zero-padded regions (the two-register softmax); EditNet Gumbel rollout; DCNet greedy
at 1, 3, 8 rows; DCNet teacher-forced forward; DCNet beam at k = 1, 3, 4; DCNet Gumbel rollout; ensemble beam + n-best at
k = 1, 3, 4.  Every beam case runs twice: on the plain models (the searches run into the step limit: NaN score, no completed
hypothesis) and, `/ending`, on models whose fc.bias[<end>] is raised by 4 (the benchmarks' ending workload: hypotheses complete,
finite best scores, non-empty n-best lists).  The previous captions are ragged (lengths 1 .. T): every batch has rows whose
caption mask zeroes scores.
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DEV = "cuda:0"
T, V, D, A, Cc, E, R, F = 18, 9490, 1024, 512, 512, 1024, 36, 2048


def bits(x):
    """nested lists of ints: fp32 as uint32 bits, integers as they are; an array above 4096 elements as its digest"""
    import torch
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    if isinstance(x, np.ndarray):
        x = np.ascontiguousarray(x.view(np.uint32) if x.dtype == np.float32 else x)
        if x.size > 4096:                        # (the teacher-forced scores, B x L x V): shape and digest of the raw bytes
            return {"shape": list(x.shape), "dtype": str(x.dtype), "sha256": hashlib.sha256(x.tobytes()).hexdigest()}
        return x.tolist()
    if isinstance(x, float):
        return int(np.float32(x).view(np.uint32))
    if isinstance(x, (list, tuple)):
        return [bits(v) for v in x]
    return int(x)


def run(out):
    import torch
    from show_edit_tell_amd import _lib, dcnet, dcnet_rl, editnet, editnet_adaptive, editnet_rl, evaluate, synth
    lib = _lib.load()
    wm = synth.word_map(V)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)

    def load(m, sd, boost=0.0):
        sd = dict(sd)
        sd["fc.bias"] = sd["fc.bias"].copy(); sd["fc.bias"][wm["<end>"]] += boost
        sd["caption_encoder.embed.embedding.weight"] = sd["embed.embedding.weight"]
        m.load_state_dict({n: torch.from_numpy(v) for n, v in sd.items()}, strict=False)
        return m.to(DEV).eval()

    se = synth.editnet_state(17, V, D, A, F, emb_scale=3.0, fc_scale=8.0, gain=3.0)
    sd = synth.dcnet_state(18, V, D, A, Cc, E, emb_scale=3.0, fc_scale=8.0, gain=3.0)
    e_rl, e_xe, e_ad = (load(c(wm, D, D, D, A, F), se) for c in (editnet_rl.DecoderC, editnet.DecoderC, editnet_adaptive.DecoderC))
    d_rl, d_xe = (load(c(wm, None, D, A, Cc, E), sd) for c in (dcnet_rl.DAE, dcnet.DAE))
    e_xe_end, e_ad_end = (load(c(wm, D, D, D, A, F), se, 4.0) for c in (editnet.DecoderC, editnet_adaptive.DecoderC))
    d_xe_end = load(dcnet.DAE(wm, None, D, A, Cc, E), sd, 4.0)
    prev_n, plen_n = (x.copy() for x in synth.prev_captions(36, 16, T, V, 5))
    plen_n.reshape(-1)[:4] = (T, 1, 7, T - 1)           # ragged: masked positions in rows 1 .. 3
    for i in range(4):
        prev_n[i, int(plen_n.reshape(-1)[i]):] = 0
    prev, plen = t(prev_n), t(plen_n)
    X = t(synth.features(35, 16, R, F))
    Xa_n, mean_n, _ = synth.adaptive_features(35, 2, 100, F, 10)
    Xa, mean = t(Xa_n), t(mean_n)
    caps, clen = (t(x) for x in synth.captions(41, 3, V, 12, 5))               # teacher-forced words, ragged lengths

    res, raw = {}, []
    answer = evaluate._PersistentBeamOut.answer

    def answer_and_keep(self, word_map, name, n_best=None, k=4):              # the launch's output buffer, before the trace-back
        host = self.buf.cpu().numpy()
        r = host[self.o_res:self.o_res + 16].view("int32")
        made = max(int(r[3]), 0)
        keep = {"hist_word": host[:self.n_hw].view("int64").reshape(-1, 4)[:made, :k],
                "hist_parent": host[self.o_hp:self.o_hp + self.n_hp].view("int32").reshape(-1, 4)[:made, :k],
                "result": r, "best_word": host[self.n_hw:self.n_hw + 8].view("int64"),
                "best_score": host[self.o_bs:self.o_bs + 4].view("float32")}
        if self.hist_score is not None:
            keep["hist_score"] = host[self.o_hs:self.o_hs + self.n_hp].view("float32").reshape(-1, 4)[:made, :k]
        raw.append({n: bits(np.array(v)) for n, v in keep.items()})
        return answer(self, word_map, name, n_best, k)

    evaluate._PersistentBeamOut.answer = answer_and_keep

    def case(name, fn, warm=2):
        try:
            with torch.no_grad():
                for _ in range(warm):                                           # token table from the second call on
                    fn()
                lib.set_profile_enable(1)
                torch.manual_seed(11)
                del raw[:]
                o = fn()
                torch.cuda.synchronize()
                tags = sorted({r["tag"] for r in _lib.profile_report() if "persistent" in r["tag"]})
                lib.set_profile_enable(0)
            res[name] = {"out": bits(list(o) if isinstance(o, tuple) else o), "persistent_tags": tags}
            if raw:
                res[name]["beam_raw"] = list(raw)
        except Exception as e:                                                  # one case must not hide the others
            lib.set_profile_enable(0)
            res[name] = {"error": "%s: %s" % (type(e).__name__, e)}
        print(name, res[name].get("persistent_tags", res[name].get("error")), flush=True)

    one = lambda b: (prev[b:b + 1], plen[b:b + 1])
    for B in (1, 3, 16):
        case("editnet/greedy/B%d" % B, lambda: e_rl(wm, prev[:B], plen[:B], X[:B], True, False))
    case("editnet/forward/B3", lambda: e_xe(X[:3], caps, clen, prev[:3], plen[:3], False, 0.0)[:3])
    for end, xe, ad in (("", e_xe, e_ad), ("/ending", e_xe_end, e_ad_end)):
        for k in (1, 3, 4):
            case("editnet/beam/k%d%s" % (k, end), lambda: evaluate.beam_search_editnet(xe, X[1:2], *one(1), wm, k, n_best=k))
        case("editnet/beam_adaptive/k3" + end, lambda: evaluate.beam_search_adaptive(ad, Xa[:1], mean[:1], *one(2), wm, 3, n_best=3))
    case("editnet/gumbel/B5", lambda: evaluate.sample_captions(e_rl, X[2:3], *one(2), wm, n_samples=5, temperature=0.8, sampler="gumbel"))
    for B in (1, 3, 8):
        case("dcnet/greedy/B%d" % B, lambda: d_rl(wm, prev[:B], plen[:B], True, False))
    case("dcnet/forward/B3", lambda: d_xe(caps, clen, prev[:3], plen[:3])[:3])
    for end, dx in (("", d_xe), ("/ending", d_xe_end)):
        for k in (1, 3, 4):
            case("dcnet/beam/k%d%s" % (k, end), lambda: evaluate.beam_search_dcnet(dx, *one(1), wm, k, n_best=k))
    case("dcnet/gumbel/B5", lambda: evaluate.sample_captions(d_rl, *one(2), wm, n_samples=5, temperature=0.8, sampler="gumbel"))
    for end, xe, dx in (("", e_xe, d_xe), ("/ending", e_xe_end, d_xe_end)):
        for k in (1, 3, 4):
            case("ensemble/beam/k%d%s" % (k, end), lambda: evaluate.beam_search_ensemble(xe, dx, X[1:2], *one(1), wm, k, n_best=k))
    with open(out, "w") as f:
        json.dump(res, f, sort_keys=True, separators=(",", ":"))
    print("pdec_bits: %d cases (%d with an error) -> %s  sha256 %s" % (len(res), sum("error" in v for v in res.values()), out,
                                                                       hashlib.sha256(open(out, "rb").read()).hexdigest()))


def compare(fa, fb):
    a, b = json.load(open(fa)), json.load(open(fb))
    bad = sorted(n for n in set(a) | set(b) if a.get(n) != b.get(n))
    err = sorted(n for n in set(a) | set(b) if any("error" in x.get(n, {}) or not x.get(n, {}).get("persistent_tags") or
                                                   x[n]["persistent_tags"] == ["persistent_encoder"] for x in (a, b)))
    print("pdec_bits: %s: %d cases, %d with an error or off the persistent launch" % ("identical" if not bad else "DIFFERENT",
                                                                                        len(set(a) | set(b)), len(err)))
    for n in bad:
        print("  differs:", n)
    return 0 if not bad and not err else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2)
    ns = ap.parse_args()
    if ns.compare:
        sys.exit(compare(*ns.compare))
    run(ns.out)
