"""GPU: the tie rule of WHOLE greedy decodes.  A model of vocabulary 2 V0 whose fc weight, fc bias and embedding are [W0; W0],
[b0; b0], [E0; E0] (special tokens where the V0 model has them) scores word v and word v + V0 alike at every step: every arg-max is
an exact tie and the only right word is the one below V0 ("first index on ties": csrc/epilogue.hip greedy_pick_k with the
planner's real slabs, bias and tail on the per-step path; the per-workgroup (max, index, sum) triples that
csrc/decode_persistent*.hip merge on the persistent launches).  Words must equal the numpy oracle's greedy decode of the V0 model
(parity.check_greedy_rows with tests/test_hip_shapes.py's margin 1e-3 and its cap on near-tie rows) and log-probs its log-probs
minus ln 2.  V0 is odd, so the twins fall into different lanes, tiles and workgroups.

Precondition, checked where a path hands out its logits (the teacher-forced forward: the per-step loop over set_editnet_step /
set_dcnet_step, and the persistent launch's teacher-forced mode): the two halves of every logit row are bitwise equal — a logit
depends on its fc row and the K order only."""
from collections import OrderedDict

import numpy as np
import pytest
import torch

import parity
from hip_adapter import load_numpy_state, to_dev
from show_edit_tell_amd import _lib, synth

pytestmark = pytest.mark.gpu
LN2 = float(np.log(2.0))
MARGIN = 1e-3
SMALL = dict(D=128, A=64, F=256, R=36, T=9)                          # the per-step rows of tests/test_hip_shapes.py
FULL_E = dict(D=1024, A=512, F=2048, R=36, T=18)                     # tests/test_hip_persistent_decode.py (editnet_full_b4)
FULL_D = dict(D=1024, A=512, C=512, E=1024, T=18)                    # (dcnet_full_b4)


def _tags(fn):
    lib = _lib.load()
    lib.set_profile_enable(1)
    fn()
    torch.cuda.synchronize()
    names = [r["tag"] for r in _lib.profile_report()]
    lib.set_profile_enable(0)
    return names


def doubled(sd0, V0):
    """(word map of 2 V0 words with <start> / <end> where the V0 map has them, the state with every vocabulary row twice)"""
    wm = OrderedDict(synth.word_map(V0))
    for i in range(V0):
        wm["twin%d" % i] = V0 + i
    sd = OrderedDict((k, v.copy()) for k, v in sd0.items())
    for k in ("fc.weight", "fc.bias", "embed.embedding.weight"):
        sd[k] = np.concatenate([sd0[k], sd0[k]], 0)
    return wm, sd


def written_steps(seq_o):
    """columns the loop writes before it is left: up to and including the step at which the last row finishes"""
    S = seq_o.shape[1]
    first0 = [int(np.nonzero(r == 0)[0][0]) if (r == 0).any() else S for r in seq_o]
    return min(max(first0) + 1, S)


def check_decode(model, sd0, wm0, V0, prev, plen, X, seq, logp):
    seq, logp = seq.cpu().numpy(), logp.cpu().numpy()
    assert (seq < V0).all(), ("a tie went to the higher twin", np.argwhere(seq >= V0)[:4], seq[seq >= V0][:4])
    seq_o, logp_o, margins, top2 = parity.oracle_greedy_reference(model, sd0, wm0, prev, plen, X)
    assert ((margins >= MARGIN).all(0)).mean() > 0.8                # (the input seeds are chosen so that the ORACLE's rows pass this cap)
    n = written_steps(seq_o)
    ref = np.zeros_like(logp_o)
    ref[:, :n] = logp_o[:, :n] - np.float32(LN2)
    return parity.check_greedy_rows(seq, logp, seq_o, ref, margins, top2, int(wm0["<end>"]), MARGIN)


def check_halves(pred, V0, what):
    """the teacher-forced logits of the doubled model: columns v and v + V0 hold the same bits"""
    p = pred.cpu().numpy().view(np.uint32)
    a, b = p[..., :V0], p[..., V0:]
    if not np.array_equal(a, b):
        at = np.argwhere(a != b)[0]
        raise AssertionError("%s: logits of the twins differ, first at row/step %s columns (%d, %d): %r vs %r (%d differing of %d)" % (
            what, tuple(at[:-1]), at[-1], at[-1] + V0, pred.cpu().numpy()[tuple(at[:-1])][at[-1]],
            pred.cpu().numpy()[tuple(at[:-1])][at[-1] + V0], int((a != b).sum()), a.size))


@pytest.mark.parametrize("V0", [101, 1003])
@pytest.mark.parametrize("B", [1, 4, 16, 17, 70])
def test_editnet_greedy_with_every_word_twice(B, V0):
    """B = 1, 4, 16 at full dimensions: the persistent launches (taken: asserted by the profile tag).  B = 17, 70: the per-step
    loop, whose pick runs with the planner's slabs, the fc bias and the LSTM tail."""
    from show_edit_tell_amd import editnet, editnet_rl
    persistent = B <= 16
    c = FULL_E if persistent else SMALL
    sd0 = synth.editnet_state(31, V0, c["D"], c["A"], c["F"], emb_scale=3.0, fc_scale=8.0, gain=3.0)
    wm0 = synth.word_map(V0)
    wm, sd = doubled(sd0, V0)
    args = (wm, c["D"], c["D"], c["D"], c["A"], c["F"])
    rl = load_numpy_state(editnet_rl.DecoderC(*args), sd)
    xe = load_numpy_state(editnet.DecoderC(*args), sd)
    X = synth.features(107 + B, B, c["R"], c["F"])
    prev, plen = synth.prev_captions(107 + B, B, c["T"], V0, min_len=1)
    caps, clen = synth.captions(107 + B, B, V0, L=12, min_len=3)
    run = (wm, to_dev(prev), to_dev(plen), to_dev(X), True, False)
    teach = (to_dev(X), to_dev(caps), to_dev(clen), to_dev(prev), to_dev(plen), False, 0.0)
    with torch.no_grad():
        for _ in range(2):                                           # (the token table is built on the second call)
            rl(*run)
            xe(*teach)
        names = _tags(lambda: rl(*run))
        assert ("persistent_decode" in names) == persistent, names
        seq, logp = rl(*run)
        pred = xe(*teach)[0]
        torch.cuda.synchronize()
    check_halves(pred, V0, "editnet teacher-forced B %d V0 %d" % (B, V0))
    check_decode("editnet", sd0, wm0, V0, prev, plen, X, seq, logp)


@pytest.mark.parametrize("V0", [101, 1003])
@pytest.mark.parametrize("B", [4, 17])
def test_dcnet_greedy_with_every_word_twice(B, V0):
    """B = 4: the persistent launch (asserted); B = 17: the per-step loop."""
    from show_edit_tell_amd import dcnet, dcnet_rl
    c = FULL_D
    sd0 = synth.dcnet_state(32, V0, c["D"], c["A"], c["C"], c["E"], emb_scale=3.0, fc_scale=8.0, gain=3.0)
    wm0 = synth.word_map(V0)
    wm, sd = doubled(sd0, V0)
    args = (wm, None, c["D"], c["A"], c["C"], c["E"])
    rl = load_numpy_state(dcnet_rl.DAE(*args), sd)
    xe = load_numpy_state(dcnet.DAE(*args), sd)
    prev, plen = synth.prev_captions(109 + B, B, c["T"], V0, min_len=1)
    caps, clen = synth.captions(109 + B, B, V0, L=12, min_len=3)
    run = (wm, to_dev(prev), to_dev(plen), True, False)
    teach = (to_dev(caps), to_dev(clen), to_dev(prev), to_dev(plen))
    with torch.no_grad():
        for _ in range(2):
            rl(*run)
            xe(*teach)
        names = _tags(lambda: rl(*run))
        assert ("persistent_decode" in names) == (B == 4), names
        seq, logp = rl(*run)
        pred = xe(*teach)[0]
        torch.cuda.synchronize()
    check_halves(pred, V0, "dcnet teacher-forced B %d V0 %d" % (B, V0))
    check_decode("dcnet", sd0, wm0, V0, prev, plen, None, seq, logp)
