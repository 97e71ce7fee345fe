"""Raw bits of the two whole-sequence training nodes (xe_sequence.py, dcnet_sequence.py) and the library calls they make, for
comparing two states of the host-side code (a refactor against its parent).

    python tools/seq_bits.py --out new.npz [--deterministic]                     (on the GPU, once per tree)
    python tools/seq_bits.py --compare parent.npz new.npz [--json verdict.json] [--repro parent.npz parent2.npz]

Only the models' public entry points are used (DecoderC.forward / sample_rollout of editnet, editnet_adaptive and editnet_rl,
DAE.forward / sample_rollout of dcnet and dcnet_rl, DAEWithAR), so the file runs unchanged in a checkout of an older commit.
Every case dumps its outputs, every parameter gradient and the gradient of the image features, and `trace`: the names passed to
`_lib.check` during the case, in order (`check` is wrapped here, before any module of the package binds it).

Shapes are rows of tests/grad_grid.py (e_b17, a_r100, d_b9: the smallest with a train-mode seed and more than one row); the
caption lengths are set here: all equal, or ragged with a row that leaves after step 1.  Rollouts run at V = 204 and V = 203
((V + 3) & ~3 is where the padded score log differs from V), without options and with temperature 0.8, top-k 5, top-p 0.95.
--repro: two dumps of the SAME tree; an array that differs between them is not bit-reproducible and is held to that
difference instead of to zero.  --deterministic: torch.use_deterministic_algorithms(True), which takes the float atomics out of
torch's index_add_ (the embedding-table gradient, the one array a tree does not reproduce against itself); the library calls
are the same.
"""
import argparse
import contextlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

ROWS = dict(editnet="e_b17", adaptive="a_r100", dcnet="d_b9", dcnet_mse="d_b9")
FROZEN = dict(editnet=("copy_lstm.x2h.weight", "caption_attention.sc_affine.bias"),
              adaptive=("copy_lstm.x2h.weight", "caption_attention.sc_affine.bias"),
              dcnet=("language_lstm.weight_ih", "attention_lstm.bias_hh"),
              dcnet_mse=("dae.language_lstm.weight_ih", "dae.attention_lstm.bias_hh"))
ROLL = dict(temperature=0.8, top_k=5, top_p=0.95)
DEV = "cuda:0"


def raw(t):
    a = t.detach().cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.float32 else a


def captions(d, kind, ragged):
    """caps / clen of a grid row with the lengths set here: all L, or L, 2 (one decode step: leaves after step 1), 3, ..."""
    import grad_grid as G
    B, V = d["dims"]["B"], d["dims"]["V"]
    L = G.TABLES[kind][ROWS[kind]][9]
    lens = np.full(B, L, np.int64)
    if ragged:
        lens = 2 + (np.arange(B) * 3) % (L - 1)
        lens[0], lens[1], lens[B - 1] = L, 2, L
    toks = d["caps"][:, :L].copy()
    toks[toks == 0] = 1
    pos = np.arange(L)[None, :]
    toks = np.where(pos == 0, V - 2, toks)
    toks = np.where(pos == lens[:, None] - 1, V - 1, toks)
    toks = np.where(pos >= lens[:, None], 0, toks)
    return toks.astype(np.int64), lens.reshape(B, 1).astype(np.int64)


def module(kind, d):
    import torch
    from hip_adapter import load_numpy_state
    from show_edit_tell_amd import dcnet, dcnet_with_mse, editnet, editnet_adaptive
    m = d["dims"]
    if kind in ("editnet", "adaptive"):
        cls = editnet.DecoderC if kind == "editnet" else editnet_adaptive.DecoderC
        return load_numpy_state(cls(d["wm"], m["D"], m["D"], m["D"], m["A"], m["F"]), d["sd"])
    dae = load_numpy_state(dcnet.DAE(d["wm"], None, m["D"], m["A"], m["C"], m["E"]), d["sd"])
    if kind == "dcnet":
        return dae
    ar = dcnet_with_mse.DAEWithAR(dae=dae)
    ar.affine_hidden.load_state_dict({k.split(".", 1)[1]: torch.from_numpy(v.copy()) for k, v in d["affine"].items()})
    return ar.to(DEV).eval()


def teacher_forced(kind, ragged, train, frozen, ss, res, tag, trace):
    import torch
    import grad_grid as G
    from hip_adapter import to_dev
    from show_edit_tell_amd import autograd_ops as A, rng, xe_sequence
    from show_edit_tell_amd.train import xe_loss_sum
    d = G.build(kind, ROWS[kind])
    mod = module(kind, d)
    for k, p in mod.named_parameters():
        if frozen and k in FROZEN[kind]:
            p.requires_grad_(False)
    assert not frozen or sum(not p.requires_grad for p in mod.parameters()) == 2
    caps, clen = (to_dev(x) for x in captions(d, kind, ragged))
    prev, plen = to_dev(d["prev"]), to_dev(d["plen"])
    X = to_dev(d["X"]).requires_grad_(True) if "X" in d else None
    mod.train(train)
    seed = G.TRAIN["dcnet" if kind == "dcnet_mse" else kind][ROWS[kind]]
    del trace[:]
    fallbacks = xe_sequence.TRUNCATION_FALLBACKS
    with (rng.dropout_seed(seed) if train else contextlib.nullcontext()):
        if kind == "editnet":
            out = mod(X, caps, clen, prev, plen, ss > 0, ss)
        elif kind == "adaptive":
            out = mod(X, to_dev(d["image_mean"]), caps, clen, prev, plen, False, 0.0)
        else:
            out = mod(caps, clen, prev, plen)
    pred, caps_s, dl = out[:3]
    loss_sum, n_tok, _, _ = xe_loss_sum(pred, caps_s, dl)
    loss = loss_sum / n_tok
    res[tag + "/pred"] = raw(pred)
    res[tag + "/fallbacks"] = np.array([xe_sequence.TRUNCATION_FALLBACKS - fallbacks])   # 1: the node handed the batch back
    if kind == "adaptive":
        loss = loss + torch.nn.functional.mse_loss(out[5], out[4])
    elif kind == "dcnet_mse":
        loss = loss + A.mse_sum(out[5], out[4]) / out[5].numel()
    if kind in ("adaptive", "dcnet_mse"):
        res[tag + "/gd_final_hidden"], res[tag + "/last_hidden"] = raw(out[4]), raw(out[5])
    loss.backward()
    torch.cuda.synchronize()
    res[tag + "/loss"] = raw(loss.reshape(1))
    finish(mod, X, res, tag, trace)


def finish(mod, X, res, tag, trace):
    for k, p in mod.named_parameters():
        if p.grad is not None:
            res[tag + "/grad/" + k] = raw(p.grad)
    if X is not None and X.grad is not None:
        res[tag + "/grad/X"] = raw(X.grad)
    res[tag + "/trace"] = np.array(trace)


def rollout(kind, V, opts, res, tag, trace):
    import torch
    from show_edit_tell_amd import dcnet_rl, editnet_rl, synth
    D, A_, F, Cc, E, B, R = 64, 32, 64, 32, 64, 6, 5
    wm = synth.word_map(V)
    prev, plen = (torch.from_numpy(x).to(DEV) for x in synth.prev_captions(3, B, 12, V, 1))
    X = None
    if kind == "editnet":
        sd = synth.editnet_state(9, V, D, A_, F, emb_scale=3.0, fc_scale=4.0, gain=2.0)
        sd["caption_encoder.embed.embedding.weight"] = sd["embed.embedding.weight"]
        m = editnet_rl.DecoderC(wm, D, D, D, A_, F)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        X = torch.from_numpy(synth.features(5, B, R, F)).to(DEV).requires_grad_(True)
        head = (wm, prev, plen, X)
    else:
        m = dcnet_rl.DAE(wm, None, D, A_, Cc, E)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.dcnet_state(4, V, D, A_, Cc, E, 3.0, 4.0, 2.0).items()}, strict=False)
        head = (wm, prev, plen)
    m = m.to(DEV).train()
    torch.manual_seed(11)
    del trace[:]
    seq, logp = m.sample_rollout(*head, **opts) if opts else m(*head, sample_max=False, sample_rl=True)
    assert logp.requires_grad
    wgt = torch.linspace(0.5, 1.5, logp.numel(), device=DEV).view(logp.shape)
    (logp * wgt).sum().backward()
    torch.cuda.synchronize()
    res[tag + "/seq"], res[tag + "/logp"] = raw(seq), raw(logp)
    finish(m, X, res, tag, trace)


def run(out, deterministic):
    import torch
    from show_edit_tell_amd import _lib
    torch.use_deterministic_algorithms(bool(deterministic), warn_only=True)
    trace, real = [], _lib.check

    def check(rc, what=""):
        trace.append(what)
        return real(rc, what)

    _lib.check = check                     # before the package's other modules import it by name
    res = {}
    for kind in ("editnet", "adaptive", "dcnet", "dcnet_mse"):
        for ragged in (False, True):
            for train in (False, True):
                teacher_forced(kind, ragged, train, False, 0.0, res, "%s/%s/%s" % (kind, "ragged" if ragged else "uniform",
                                                                                  "train" if train else "eval"), trace)
        teacher_forced(kind, True, True, True, 0.0, res, kind + "/ragged/train/frozen", trace)
    for ragged in (False, True):
        teacher_forced("editnet", ragged, True, False, 0.5, res, "editnet/%s/train/ss" % ("ragged" if ragged else "uniform"), trace)
    for kind in ("editnet", "dcnet"):
        for V in (204, 203):
            for opts in (None, ROLL):
                rollout(kind, V, opts, res, "%s/rollout/V%d/%s" % (kind, V, "opts" if opts else "plain"), trace)
    np.savez_compressed(out, **res)
    print("seq_bits: %d arrays of %d cases -> %s" % (len(res), len({n.split("/pred")[0].split("/seq")[0] for n in res
                                                                    if n.endswith(("/pred", "/seq"))}), out))


def case_of(name):
    for mark in ("/grad/", "/pred", "/loss", "/fallbacks", "/trace", "/seq", "/logp", "/gd_final_hidden", "/last_hidden"):
        if mark in name:
            return name[:name.index(mark)]
    return name


def max_diff(x, y):
    """largest |x - y| of two raw dumps (fp32 arrays were stored as their uint32 bits)"""
    if x.shape != y.shape:
        return float("inf")
    if x.dtype == np.uint32:
        return float(np.abs(x.view(np.float32).astype(np.float64) - y.view(np.float32).astype(np.float64)).max()) if x.size else 0.0
    return float(np.abs(x.astype(np.float64) - y.astype(np.float64)).max()) if x.size else 0.0


def compare(fa, fb, js, repro):
    a, b = np.load(fa), np.load(fb)
    names = sorted(set(a.files) | set(b.files))
    loose = {}                             # array -> parent-to-parent difference, for arrays that the parent does not reproduce
    if repro:
        r0, r1 = np.load(repro[0]), np.load(repro[1])
        assert set(r0.files) == set(r1.files)
        loose = {n: max_diff(r0[n], r1[n]) for n in r0.files if r0[n].shape != r1[n].shape or not np.array_equal(r0[n], r1[n])}
    scale = lambda n: float(np.abs(a[n].view(np.float32)).max()) if a[n].dtype == np.uint32 and a[n].size else None
    traces = [n for n in names if n.endswith("/trace")]
    bad_trace = [n for n in traces if n not in a.files or n not in b.files or list(a[n]) != list(b[n])]
    bad, held, how = [], {}, {}
    for n in names:
        if n in traces:
            continue
        if n not in a.files or n not in b.files or a[n].shape != b[n].shape:
            bad.append(n)
        elif not np.array_equal(a[n], b[n]):
            dlt = max_diff(a[n], b[n])
            if n in loose and dlt <= loose[n]:
                held[n] = dict(parent_to_parent=loose[n], parent_to_result=dlt)
            else:
                bad.append(n)
                how[n] = dict(parent_to_result=dlt, parent_to_parent=loose.get(n, 0.0), largest_element=scale(n))
    ok = not bad and not bad_trace
    verdict = ("identical" if ok and not held else "within the parent's own difference" if ok else "DIFFERENT") + \
              ": %d arrays, %d traces" % (len(names) - len(traces), len(traces))
    print("seq_bits:", verdict)
    for n in (bad_trace + bad)[:40]:
        print("  differs:", n)
    if js:
        with open(js, "w") as f:
            json.dump({"tool": "tools/seq_bits.py --compare A B --json FILE [--repro A A2]; dumps written by --out on one GPU",
                       "verdict": verdict, "arrays": len(names) - len(traces), "traces": len(traces),
                       "library_calls_traced": int(sum(len(a[n]) for n in traces if n in a.files)),
                       "cases": sorted({case_of(n) for n in names}),
                       "parent_run_twice": bool(repro),
                       "not_reproducible_on_the_parent": {n: dict(parent_to_parent=loose[n], largest_element=scale(n)) for n in sorted(loose)},
                       "held_to_the_parent_difference": held, "different_traces": bad_trace, "different": bad, "different_by": how}, f, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--deterministic", action="store_true")
    ap.add_argument("--compare", nargs=2)
    ap.add_argument("--repro", nargs=2)
    ap.add_argument("--json")
    ns = ap.parse_args()
    if ns.compare:
        sys.exit(compare(ns.compare[0], ns.compare[1], ns.json, ns.repro))
    run(ns.out, ns.deterministic)
