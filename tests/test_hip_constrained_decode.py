"""GPU: whole constrained greedy and sampled decodes (set_*_greedy_constrained / set_*_sample_constrained and the `constraints=`
keyword of the models and of evaluate.sample_captions) on the small synthetic models, B = 3: EditNet with fixed and with adaptive
features, DCNet.  Each model comes in two variants of one fixture: as built (its unconstrained greedy captions repeat words and
n-grams and never end) and with fc.bias[<end>] raised by 3 (they end at the first step), so that the unconstrained decodes
violate every rule the constrained ones must obey."""
import ctypes as C

import numpy as np
import pytest
import torch

import pick_constrained_oracle as PCO
from hip_adapter import load_numpy_state, to_dev
from oracle import cases, dcnet_np as DN, editnet_np as EN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B = 3
KINDS = ["editnet", "adaptive", "dcnet"]
FIXTURE = {"editnet": "editnet_small", "adaptive": "editnet_adaptive_small", "dcnet": "dcnet_small"}
LOGP_TOL = 1e-4                                  # the project's target between two routes to the same logits
_cache = {}


def model(kind, boost):
    """(case dict, module, inputs tuple after word_map, numpy state dict) of a kind, rows 0 .. B-1, <end> bias raised by `boost`"""
    key = (kind, boost)
    if key in _cache:
        return _cache[key]
    from show_edit_tell_amd import dcnet_rl, editnet_adaptive, editnet_rl
    d = cases.build_dcnet(FIXTURE[kind]) if kind == "dcnet" else cases.build_editnet(FIXTURE[kind])
    c, wm = d["case"], d["wm"]
    sd = dict(d["sd"])
    sd["fc.bias"] = sd["fc.bias"].copy()
    sd["fc.bias"][wm["<end>"]] += np.float32(boost)
    if kind == "dcnet":
        m = load_numpy_state(dcnet_rl.DAE(wm, None, c["D"], c["A"], c["C"], c["E"]), sd)
        inputs, kw = (to_dev(d["prev"][:B]), to_dev(d["plen"][:B])), {}
    else:
        cls = editnet_rl.DecoderC
        if kind == "adaptive":
            class cls(editnet_rl.DecoderC):                                  # the free-running loop over the adaptive attention
                _visual_attention_cls = editnet_adaptive.VisualAttentionC
                _adaptive = 1
        m = load_numpy_state(cls(wm, c["D"], c["D"], c["D"], c["A"], c["F"]), sd)
        inputs = (to_dev(d["prev"][:B]), to_dev(d["plen"][:B]), to_dev(d["X"][:B]))
        kw = dict(image_mean=to_dev(d["image_mean"][:B])) if kind == "adaptive" else {}
    _cache[key] = (d, m, inputs, kw, sd)
    return _cache[key]


def decode(kind, boost, sample=False, **kw2):
    d, m, inputs, kw, _ = model(kind, boost)
    with torch.no_grad():
        seq, logp = m(d["wm"], *inputs, not sample, sample, **kw, **kw2)
    torch.cuda.synchronize()
    return seq.cpu().numpy(), logp.cpu().numpy()


def choose(seq0, wm):
    """(banned word, n) from the unconstrained output: its most frequent word, the largest n <= 3 with a repeated n-gram"""
    words, counts = np.unique(seq0[seq0 > 0], return_counts=True)
    banned = int(words[np.argmax(counts)])
    for n in (3, 2, 1):
        if any(PCO.violations(r, wm["<start>"], True, PCO.Cons(n), 0)[2] for r in seq0):
            return banned, n
    raise AssertionError("the unconstrained decode repeats nothing")


def constraints_for(kind):
    from show_edit_tell_amd.evaluate import BeamConstraints
    d = model(kind, 0.0)[0]
    seq0, _ = decode(kind, 0.0)
    banned, n = choose(seq0, d["wm"])
    # (word 0 ends a row like <end> does and cannot be told from it in seq: banned too, as a caller bans <pad>)
    return BeamConstraints(no_repeat_ngram=n, min_length=4, banned_words=[banned, 0]), PCO.Cons(n, 4, [banned, 0]), seq0


def total(seq, wm, cons):
    return np.sum([PCO.violations(r, wm["<start>"], True, cons, 0) for r in seq], axis=0)


@pytest.mark.parametrize("kind", KINDS)
def test_constrained_decodes_obey_the_rules_the_unconstrained_break(kind):
    bc, cons, seq0 = constraints_for(kind)
    wm = model(kind, 0.0)[0]["wm"]
    a0, _, c0 = total(seq0, wm, cons)
    assert a0 > 0 and c0 > 0, "the unconstrained decode violates neither a nor c"
    seq3, _ = decode(kind, 3.0)
    assert total(seq3, wm, cons)[1] > 0, "the unconstrained decode of the <end>-boosted variant ends late enough"
    for boost in (0.0, 3.0):
        for sample in (False, True):
            torch.manual_seed(5)
            seq, logp = decode(kind, boost, sample, constraints=bc, **(dict(top_k=50, top_p=0.95) if sample else {}))
            assert total(seq, wm, cons).tolist() == [0, 0, 0], (kind, boost, sample, seq)
            assert np.isfinite(logp).all() and (logp <= 0).all()


@pytest.mark.parametrize("kind", KINDS)
def test_none_and_neutral_are_todays_call(kind):
    from show_edit_tell_amd.evaluate import BeamConstraints
    for sample in (False, True):
        got = []
        for kw in ({}, dict(constraints=None), dict(constraints=BeamConstraints())):
            torch.manual_seed(11)
            got.append(decode(kind, 0.0, sample, **kw))
        for seq, logp in got[1:]:
            assert np.array_equal(seq, got[0][0]) and np.array_equal(logp.view(np.uint32), got[0][1].view(np.uint32))


@pytest.mark.parametrize("kind", KINDS)
def test_greedy_tokens_equal_the_numpy_oracle_stepped_with_the_mask(kind):
    bc, cons, _ = constraints_for(kind)
    d, m, _, _, sd = model(kind, 0.0)
    wm, max_len = d["wm"], m.max_len
    start, end = wm["<start>"], wm["<end>"]
    P = EN.cast_params(sd)
    if kind == "dcnet":
        S, step = DN.SeqState(P, d["prev"][:B], d["plen"][:B]), DN.step
    else:
        kw = dict(image_mean=d["image_mean"][:B], adaptive=True) if kind == "adaptive" else {}
        S, step = EN.SeqState(P, d["X"][:B], d["prev"][:B], d["plen"][:B], **kw), EN.step
    import pick_oracle as PO
    st = PO.new_state(B, max_len)
    it = np.full(B, start, np.int64)
    for t in range(max_len):
        x = np.asarray(step(S, it), np.float64)
        PCO.greedy_step(x, t, max_len, end, st, cons)
        it = st["it"].copy()
        if st["alive"][t] == 0:
            break
    seq, logp = decode(kind, 0.0, constraints=bc)
    assert np.array_equal(seq, st["seq"]), (seq, st["seq"])
    assert float(np.abs(logp - st["seq_logp"]).max()) <= LOGP_TOL


def _c_entries(kind, sample):
    from show_edit_tell_amd import _lib as L
    lib = L.load()
    name = "set_%s_%s_constrained" % ("dcnet" if kind == "dcnet" else "editnet", "sample" if sample else "greedy")
    return L, lib, getattr(lib, name)


@pytest.mark.parametrize("sample", [False, True], ids=["greedy", "sample"])
@pytest.mark.parametrize("kind", KINDS)
def test_fused_loop_equals_the_per_step_replay(kind, sample):
    """set_*_begin + per timestep set_*_step on the previous pick's tokens + set_pick_slabs_constrained_f32, against the fused
    entry with the same (seed, offset): tokens equal, seq_logp within the 1e-4 the two routes' logits agree to"""
    bc, cons, _ = constraints_for(kind)
    d, m, inputs, kw, _ = model(kind, 0.0)
    L, lib, fused = _c_entries(kind, sample)
    wm, max_len, V = d["wm"], m.max_len, d["case"]["V"]
    start, end = int(wm["<start>"]), int(wm["<end>"])
    dev = torch.device(DEV)
    st = L.stream_of(dev)
    prev, plen = inputs[0].long().contiguous(), inputs[1].reshape(-1).long().contiguous()
    X = inputs[2].float().contiguous() if kind != "dcnet" else None
    mean = kw.get("image_mean")
    dims = m._dims(B, prev.shape[1], max_len + 1) if kind == "dcnet" else m._dims(B, prev.shape[1], X.shape[1], max_len + 1)
    ws, w = m._workspace(dims), m._weights(dims)
    ids = torch.tensor(list(cons.banned), dtype=torch.long, device=dev)
    cs = L.BeamConstraintsC(cons.ngram, cons.min_len, 0.0, len(cons.banned), ids.data_ptr())
    opts = L.SampleOpts(temperature=0.9, top_k=40, top_p=0.95) if sample else None
    seed, offset = 77, 3
    seq = torch.empty(B, max_len, dtype=torch.long, device=dev)
    logp = torch.empty(B, max_len, dtype=torch.float32, device=dev)
    lead = (C.byref(w), C.byref(dims)) + ((L.ptr(X), L.ptr(mean)) if kind != "dcnet" else ()) + (L.ptr(prev), L.ptr(plen), start, end, max_len)
    out = (L.ptr(seq), L.ptr(logp), L.ptr(ws), ws.numel(), st)
    if sample:
        L.check(fused(*lead, seed, offset, *out, C.byref(opts), C.byref(cs)), "fused sample")
    else:
        L.check(fused(*lead, *out, C.byref(cs)), "fused greedy")
    torch.cuda.synchronize()
    # ---- the replay
    if kind == "dcnet":
        L.check(lib.set_dcnet_begin(C.byref(w), C.byref(dims), L.ptr(prev), L.ptr(plen), L.ptr(ws), ws.numel(), st), "begin")
    else:
        L.check(lib.set_editnet_begin(C.byref(w), C.byref(dims), L.ptr(X), L.ptr(mean), L.ptr(prev), L.ptr(plen), L.ptr(ws),
                                      ws.numel(), st), "begin")
    ld = (V + 3) // 4 * 4
    logits = torch.zeros(B, ld, device=dev)
    seq2 = torch.zeros(B, max_len, dtype=torch.long, device=dev)
    logp2 = torch.zeros(B, max_len, dtype=torch.float32, device=dev)
    it = torch.full((B,), start, dtype=torch.long, device=dev)
    unf = torch.ones(B, dtype=torch.int32, device=dev)
    alive = torch.zeros(max_len + 2, dtype=torch.int32, device=dev)
    for t in range(max_len):
        if kind == "dcnet":
            L.check(lib.set_dcnet_step(C.byref(w), C.byref(dims), L.ptr(it), 1, B, L.ptr(logits), ld, L.ptr(ws), ws.numel(), st), "step")
        else:
            L.check(lib.set_editnet_step(C.byref(w), C.byref(dims), L.ptr(X), L.ptr(it), 1, B, L.ptr(logits), ld, L.ptr(ws),
                                         ws.numel(), st), "step")
        a = L.PickArgs(logits=logits.data_ptr(), ld=ld, stride=0, end_idx=end, seq=seq2.data_ptr(), seq_logp=logp2.data_ptr(),
                       it=it.data_ptr(), unfinished=unf.data_ptr(), alive=alive.data_ptr(), seed=seed, offset=offset, n=1, B=B, V=V,
                       t=t, max_len=max_len, D=4, mode=1 if sample else 0)
        L.check(lib.set_pick_slabs_constrained_f32(C.byref(a), C.byref(opts) if sample else None, C.byref(cs), st), "pick")
    torch.cuda.synchronize()
    alive_h = alive.cpu().numpy()
    seq2_h, logp2_h = seq2.cpu().numpy(), logp2.cpu().numpy()
    assert np.array_equal(seq.cpu().numpy(), seq2_h), (seq.cpu().numpy(), seq2_h, alive_h)
    assert float(np.abs(logp.cpu().numpy() - logp2_h).max()) <= LOGP_TOL
    assert total(seq2_h, wm, cons).tolist() == [0, 0, 0]


@pytest.mark.parametrize("kind", ["editnet", "dcnet"])
def test_sample_captions_with_constraints(kind):
    from show_edit_tell_amd import evaluate
    bc, cons, _ = constraints_for(kind)
    d, m, inputs, kw, _ = model(kind, 0.0)
    args = ((inputs[2],) if kind != "dcnet" else ()) + (inputs[0], inputs[1], d["wm"])
    torch.manual_seed(3)
    seq, logp = evaluate.sample_captions(m, *args, n_samples=3, top_p=0.9, constraints=bc)
    torch.cuda.synchronize()
    assert tuple(seq.shape) == (B, 3, m.max_len)
    flat = seq.reshape(-1, m.max_len).cpu().numpy()
    assert total(flat, d["wm"], cons).tolist() == [0, 0, 0]
    assert len({tuple(r) for r in flat}) > 1
    torch.manual_seed(3)
    seq_b, logp_b = evaluate.sample_captions(m, *args, n_samples=3, top_p=0.9, constraints=bc)
    assert torch.equal(seq, seq_b) and torch.equal(logp, logp_b)


def test_refusals_where_gradients_flow_and_for_gumbel():
    from show_edit_tell_amd.evaluate import BeamConstraints
    d, m, inputs, kw, _ = model("editnet", 0.0)
    bc = BeamConstraints(no_repeat_ngram=2)
    with torch.no_grad():
        with pytest.raises(ValueError):
            m(d["wm"], *inputs, False, True, sampler="gumbel", constraints=bc)
        with pytest.raises(ValueError):
            m(d["wm"], *inputs, True, False, constraints=BeamConstraints(no_repeat_ngram=2, length_penalty=0.7))
        with pytest.raises(ValueError):
            m(d["wm"], *inputs, True, False, constraints=BeamConstraints(banned_words=["<end>"]))
    with pytest.raises(ValueError):
        m.sample_rollout(d["wm"], *inputs, constraints=bc)
    m.train()
    try:
        with pytest.raises(ValueError):
            m(d["wm"], *inputs, True, False, constraints=bc)
    finally:
        m.eval()
