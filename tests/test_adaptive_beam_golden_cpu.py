"""CPU: the oracle's numpy beam search over ADAPTIVE features against tests/golden/beam_adaptive_*.npz, the outputs of
the reference's own adaptive evaluate() loop (`adaptive_features/editnet_adaptive.py:614-735`, written by
tools/make_adaptive_beam_golden.py).  The search gets each image's own mean (over its valid regions) and masks the
zero-padded regions; tests/test_hip_adaptive_beam.py compares the HIP searches with the same fixtures."""
import numpy as np
import pytest

import beam_parity
from oracle import beam_np, cases, editnet_np as EN

# golden -> adaptive case of oracle/cases.py (boosts and beam sizes are read from the golden)
GOLDENS = {"beam_adaptive_small": "editnet_adaptive_small", "beam_adaptive_full_b4": "editnet_adaptive_full_b4"}


class AdaptiveBeam:
    """beam_np.EditNetBeam for adaptive features: the image mean comes with the image, the visual attention embeds the
    regions every step (SeqState keeps no att1)."""

    def __init__(self, P, X1, mean1, prev1, plen1, k):
        self.S = EN.SeqState(P, np.repeat(X1, k, 0), np.repeat(prev1, k, 0), np.repeat(plen1, k, 0),
                             image_mean=np.repeat(mean1, k, 0), adaptive=True)

    def step(self, words):
        return EN.step(self.S, words, len(words))

    def reindex(self, idx):
        S = self.S
        for n in ("X", "H", "M", "final_hidden", "mask", "image_mean", "att1_c", "h1", "c1", "h2", "c2"):
            setattr(S, n, getattr(S, n)[idx])


def boosted_params(sd, V, boost):
    sd = dict(sd)
    sd["fc.bias"] = sd["fc.bias"].copy()
    sd["fc.bias"][V - 1] += np.float32(boost)
    return EN.cast_params(sd)


def firm_expected(g):
    """Finished searches whose two best completed hypotheses are further apart than MARGIN_MIN: check_one compares
    those strictly."""
    n = 0
    for key in g:
        if key.endswith(".infinite"):
            pre = key[: -len("infinite")]
            n += int(((~g[key]) & (g[pre + "margin"] > beam_parity.MARGIN_MIN)).sum())
    return n


@pytest.mark.parametrize("name", sorted(GOLDENS))
def test_oracle_adaptive_beam_vs_reference_beam(name):
    d = cases.build_editnet(GOLDENS[name])
    g = beam_parity.load(name)
    c, wm = d["case"], d["wm"]
    assert np.array_equal(g["nvalid"], d["nvalid"])
    V = c["V"]
    firm = 0
    for boost in g["boosts"]:
        P = boosted_params(d["sd"], V, float(boost))
        model = "adaptive_e%d" % int(round(float(boost) * 10))
        for k in g["beams"]:
            k = int(k)
            for b in range(c["B"]):
                st = AdaptiveBeam(P, d["X"][b:b + 1], d["image_mean"][b:b + 1], d["prev"][b:b + 1], d["plen"][b:b + 1], k)
                seq, score, _ = beam_np.beam_loop([st], lambda ls: EN._log_softmax(ls[0], 1), wm["<start>"], wm["<end>"], V, k)
                firm += beam_parity.check_one(g, k, model, b, seq, score)
    want = firm_expected(g)
    assert want >= 1
    assert firm >= want, (firm, want)
