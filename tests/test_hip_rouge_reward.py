"""GPU: the ROUGE-L term of the self-critical reward: ciderd.self_critical_reward_device with all three weights against
ciderd.self_critical_reward on the host route, and one SCST step of each model on the small synthetic nets with
rouge_weight = 0.5, device route against host route; rouge_weight = 0 is the step without the argument, bit for bit.

Tolerance: the one tests/test_hip_bleu_device.py asks of its mix — 1e-5 relative on float32 rewards (relative to the largest
magnitude of the tensor; for the step's mean reward and loss, to the value itself), and the same 1e-5 of the updated
parameters.  Both routes mix in double and cast once, and the device ROUGE-L has the host's bits, so what differs is
CIDEr-D's 1e-9 and a last float32 bit."""
import numpy as np
import pytest
import torch

from hip_adapter import dcnet_modules, editnet_modules, to_dev

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL_REL = 1e-5


@pytest.mark.parametrize("refs_as", ["prepared", "raw"])
def test_reward_mix_against_host(refs_as):
    """8 images x 3 samples, weights (0.7, 0.5, 0.4)"""
    from show_edit_tell_amd import bleu, ciderd, rouge
    rng = np.random.default_rng(8)
    gt = [[[int(w) for w in rng.integers(1, 58, int(rng.integers(5, 12)))] + [0] for _ in range(5)] for _ in range(8)]
    df, docs = ciderd.document_frequency([[ciderd.tokens_to_str(c) for c in caps] for caps in gt])
    sc = ciderd.CiderD(df, docs)

    def near(b):
        c = [w for w in gt[b][int(rng.integers(0, 5))] if w][:18]
        c[int(rng.integers(0, len(c)))] = int(rng.integers(1, 58))
        row = np.zeros(20, dtype=np.int64)
        row[:len(c)] = c
        return row
    greedy = np.stack([near(b) for b in range(8)])
    sampled = np.stack([near(b % 8) for b in range(24)])
    want = ciderd.self_critical_reward(sc, sampled, np.tile(greedy, (3, 1)), gt * 3, 0.7, bleu.Bleu(), 0.5, rouge.RougeL(), 0.4)
    without = ciderd.self_critical_reward(sc, sampled, np.tile(greedy, (3, 1)), gt * 3, 0.7, bleu.Bleu(), 0.5)
    assert np.abs(want - without).max() > 0.02                   # the ROUGE-L term is there
    dsc, bsc, rsc = sc.device(DEV), bleu.device_scorer(DEV), rouge.device_scorer(DEV)
    if refs_as == "prepared":
        brefs = bsc.prepare_refs(gt)
        rrefs = brefs                                            # one preparation, both scorers
    else:
        brefs = rrefs = gt
    got = ciderd.self_critical_reward_device(dsc, to_dev(sampled), to_dev(greedy), dsc.prepare_refs(gt), None, 0.7, bsc, brefs, 0.5,
                                             rsc, rrefs, 0.4)
    assert got.dtype == torch.float32 and tuple(got.shape) == (24, 20) and got.is_cuda
    err = np.abs(got.cpu().numpy().astype(np.float64) - want.astype(np.float64)).max()
    print("reward: largest |device - host| = %.3e, largest |reward| = %.3e" % (err, np.abs(want).max()))
    assert err <= TOL_REL * np.abs(want).max()
    # the ROUGE-L term without a BLEU scorer, its own references
    got = ciderd.self_critical_reward_device(dsc, to_dev(sampled), to_dev(greedy), gt, None, 0.7, rouge_scorer=rsc,
                                             rouge_refs=rsc.prepare_refs(gt) if refs_as == "prepared" else gt, rouge_weight=0.4)
    want = ciderd.self_critical_reward(sc, sampled, np.tile(greedy, (3, 1)), gt * 3, 0.7, rouge_scorer=rouge.RougeL(), rouge_weight=0.4)
    assert np.abs(got.cpu().numpy().astype(np.float64) - want.astype(np.float64)).max() <= TOL_REL * np.abs(want).max()
    with pytest.raises(ValueError, match="rouge_refs"):
        ciderd.self_critical_reward_device(dsc, to_dev(sampled), to_dev(greedy), gt, None, 0.7, rouge_scorer=rsc, rouge_weight=0.4)


def _scst_refs(wm, B, model_greedy):
    """the set-up of tests/test_hip_bleu_device.py: 5 random captions per image over the real vocabulary — and the model's own
    greedy caption as the first, so that rewards are not all zero"""
    from show_edit_tell_amd import ciderd
    V = len(wm)
    rng = np.random.default_rng(3)
    allcaps = np.zeros((B, 5, 24), dtype=np.int64)
    for b in range(B):
        for j in range(5):
            n = int(rng.integers(3, 9))
            words = rng.integers(1, V - 4, n)
            if j == 0:
                g = [int(w) for w in model_greedy[b] if int(w) > 0][:20]
                words = np.array(g if g else [1], dtype=np.int64)
                n = len(words)
            allcaps[b, j, 0] = wm["<start>"]
            allcaps[b, j, 1:1 + n] = words
            allcaps[b, j, 1 + n] = wm["<end>"]
    gt = ciderd.ground_truth_lists(allcaps, wm)
    df, docs = ciderd.document_frequency([[ciderd.tokens_to_str(c) for c in caps] for caps in gt])
    return gt, ciderd.CiderD(df, max(docs, 2))


def _scst_run(net, **kw):
    from show_edit_tell_amd import train
    if net == "editnet":
        d, _, rl = editnet_modules("editnet_small")
        inputs = (to_dev(d["X"]), to_dev(d["prev"]), to_dev(d["plen"]))
        greedy_in = (to_dev(d["prev"]), to_dev(d["plen"]), to_dev(d["X"]))
        step = train.scst_train_step
    else:
        d, _, rl = dcnet_modules("dcnet_small")
        inputs = (to_dev(d["prev"]), to_dev(d["plen"]))
        greedy_in = inputs
        step = train.dcnet_scst_train_step
    wm = d["wm"]
    with torch.no_grad():
        g, _ = rl(wm, *greedy_in, sample_max=True, sample_rl=False)
    gt, scorer = _scst_refs(wm, inputs[0].shape[0], g.cpu().numpy())
    opt = torch.optim.Adam(rl.parameters(), lr=1e-3)
    torch.manual_seed(4)
    out = step(rl, opt, wm, *inputs, gt, scorer, n_samples=3, **kw)
    params = [p.detach().cpu().clone() for p in rl.parameters()]
    assert all(torch.isfinite(p).all() for p in params)
    return out, params


@pytest.fixture(scope="module")
def plain_steps():
    """the step without the argument, once per (net, route): shared by the tests below and left unchanged"""
    return {(net, route): _scst_run(net, reward=route) for net in ("editnet", "dcnet") for route in ("host", "device")}


@pytest.mark.parametrize("net", ["editnet", "dcnet"])
def test_scst_step_with_rouge_term_device_matches_host(net, plain_steps):
    """two identical models and seeds, one step each with reward="host" and reward="device", rouge_weight = 0.5"""
    (r_h, l_h), p_h = _scst_run(net, reward="host", rouge_weight=0.5)
    (r_d, l_d), p_d = _scst_run(net, reward="device", rouge_weight=0.5)
    (r_0, _), _ = plain_steps[(net, "host")]
    par = max(float((a - b).abs().max() / a.abs().max().clamp_min(1e-30)) for a, b in zip(p_h, p_d))
    print("reward host %.9g device %.9g (without the ROUGE-L term %.9g), loss host %.9g device %.9g, parameters rel %.3e"
          % (r_h, r_d, r_0, l_h, l_d, par))
    assert np.isfinite([r_h, l_h, r_d, l_d]).all()
    assert abs(r_h - r_0) > 1e-3                                  # the ROUGE-L term moved the reward
    assert abs(r_h - r_d) <= TOL_REL * abs(r_h)
    assert abs(l_h - l_d) <= TOL_REL * abs(l_h)
    assert par <= TOL_REL


@pytest.mark.parametrize("net", ["editnet", "dcnet"])
def test_scst_step_with_all_three_terms_device_matches_host(net):
    """cider + BLEU + ROUGE-L: on the device route the BLEU records are prepared once and serve both scorers"""
    (r_h, l_h), p_h = _scst_run(net, reward="host", bleu_weight=0.3, rouge_weight=0.5)
    (r_d, l_d), p_d = _scst_run(net, reward="device", bleu_weight=0.3, rouge_weight=0.5)
    par = max(float((a - b).abs().max() / a.abs().max().clamp_min(1e-30)) for a, b in zip(p_h, p_d))
    print("reward host %.9g device %.9g, loss host %.9g device %.9g, parameters rel %.3e" % (r_h, r_d, l_h, l_d, par))
    assert abs(r_h - r_d) <= TOL_REL * abs(r_h) and abs(l_h - l_d) <= TOL_REL * abs(l_h) and par <= TOL_REL


@pytest.mark.parametrize("net", ["editnet", "dcnet"])
@pytest.mark.parametrize("route", ["host", "device"])
def test_scst_step_rouge_weight_zero_is_the_step_without_it(net, route, plain_steps):
    (r_a, l_a), p_a = plain_steps[(net, route)]
    (r_b, l_b), p_b = _scst_run(net, reward=route, rouge_weight=0.0)
    assert r_a == r_b and l_a == l_b
    assert all(torch.equal(a, b) for a, b in zip(p_a, p_b))
