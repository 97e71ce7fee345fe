"""Test helper: the awkward-shape grid of the gradient parity tests and its float64 autograd results.

One table per model; `build(kind, name)` turns a row into numpy inputs and weights (show_edit_tell_amd.synth, no golden
file), `oracle(kind, name, train)` runs oracle/xe_grad_torch.py on them ONCE per session (module-level cache: the GPU tests
compare both routes and both weight-gradient modes with the same float64 result).  tests/test_xe_grad_oracle_cpu.py
asserts for every row that the float64 forward has no hard-select near-tie (select_gap_min >= 1e-4) and no ReLU
pre-activation within fp32 summation noise of zero (kink_count == 0): seeds were picked on the CPU so that both hold, and the
GPU comparison therefore excuses no row, parameter or element.

What the rows cover between them: B = 1, 3, 17, 37, 63, 64, 65, 127, 130, 200 (the 16-, 64- and 128-row switches from both
sides); R = 1, 2, 5, 36, 100; valid-region counts 1, 47, 48, 49, R; a valid region that the
train-mode dropout zeroes entirely (a_dead); previous captions all of length 1 / all of length T / ragged including 1; T = 1; caption lengths all equal / all minimal / ragged with ties; D/A/F = 64/32/64, 128/64/256,
512/64/128, 2048/64/128 and the full 1024/512/2048; V = 37, 203, 514, 1003 (V & 3 != 0 with >= 64 rows per timestep:
e_b65, e_b127, a_b65, d_b65)."""
import functools

import numpy as np

from oracle import xe_grad_torch as XG
from show_edit_tell_amd import synth

SCALES = dict(gain=3.0, emb_scale=3.0, fc_scale=8.0)

# prev: "one" = every previous caption has length 1, "full" = length T, "ragged" = 1 .. T with row 0 forced to 1
# caps: "equal" = every caption has length L, "min" = length 2 (one decode step), "ragged" = 2 .. L with a forced tie
EDITNET = {
    #            B    T   R    D     A    F     V     prev      caps     L  seed
    "e_b1":     (1,   1,  1,   64,   32,  64,   37,   "one",    "equal",  5, 1),
    "e_b3":     (3,   5,  2,   64,   32,  128,  203,  "ragged", "min",    2, 2),
    "e_b17":    (17,  7,  5,   128,  64,  256,  514,  "ragged", "ragged", 8, 3),
    "e_b37":    (37,  4,  36,  64,   32,  64,   1003, "full",   "equal",  5, 4),
    "e_b63":    (63,  6,  7,   64,   32,  128,  203,  "ragged", "ragged", 7, 5),
    "e_b64":    (64,  3,  2,   64,   32,  64,   37,   "one",    "equal",  4, 6),
    "e_b65":    (65,  3,  5,   64,   32,  64,   1003, "ragged", "equal",  4, 7),
    "e_b127":   (127, 4,  2,   64,   32,  64,   514,  "ragged", "ragged", 5, 8),
    "e_b130":   (130, 5,  5,   64,   32,  64,   203,  "ragged", "equal",  3, 9),
    "e_b200":   (200, 3,  100, 64,   32,  128,  37,   "ragged", "ragged", 4, 10),
    "e_d512":   (9,   6,  4,   512,  64,  128,  203,  "ragged", "ragged", 6, 11),
    "e_d2048":  (5,   4,  3,   2048, 64,  128,  37,   "ragged", "ragged", 4, 12),
    "e_full":   (4,   3,  36,  1024, 512, 2048, 203,  "ragged", "ragged", 4, 13),
}
# nvalid: forced valid-region counts of the first rows (the rest are drawn from 1 .. R)
ADAPTIVE = {
    #            B    T   R    D     A    F     V     prev      caps     L  seed  nvalid
    "a_b1":     (1,   1,  1,   64,   32,  64,   37,   "one",    "equal",  4, 21, (1,)),
    "a_r100":   (4,   5,  100, 64,   32,  64,   203,  "ragged", "ragged", 6, 22, (1, 47, 48, 100)),
    "a_r49":    (6,   4,  49,  128,  64,  256,  37,   "full",   "ragged", 5, 23, (49, 1, 48, 47, 10, 2)),
    "a_b65":    (65,  3,  12,  64,   32,  64,   1003, "ragged", "equal",  4, 24, (12, 1)),
    "a_dead":   (3,   4,  6,   64,   32,  64,   203,  "ragged", "ragged", 5, 25, (6, 3, 2)),
}
# a_dead: region DEAD[1] of row DEAD[0] (the row with all R regions valid and the longest caption: live at every step) has
# tiny features and att_embed.0.bias is negative except at the columns DEAD[2], so that region's embedded row has exactly two
# non-zero entries.  In eval mode it is unmasked; in train mode the step's dropout zeroes the whole row whenever it drops both
# columns — the input of the reference's count-based truncation (editnet_adaptive.py:455-456): the row's LAST valid region
# falls out of the context at those steps.  The train seed is picked so that this happens at some steps and not at others.
DEAD = (0, 2, (5, 40))
DCNET = {
    #            B    T   D     A    C    E     V     prev      caps     L  seed
    "d_b1":     (1,   1,  64,   32,  32,  64,   37,   "one",    "equal",  5, 31),
    "d_b9":     (9,   6,  128,  64,  64,  128,  514,  "ragged", "ragged", 7, 32),
    "d_b65":    (65,  3,  64,   32,  32,  64,   1003, "ragged", "equal",  4, 33),
    "d_b130":   (130, 5,  64,   32,  32,  64,   203,  "ragged", "ragged", 4, 34),
    "d_full":   (5,   4,  1024, 512, 512, 1024, 203,  "full",   "ragged", 4, 35),
}
DCNET_MSE = ("d_b9", "d_b65")                 # the stage-2 loss through DAEWithAR (D == 2 C)
# train mode (dropout seeds above 2**32): B = 1 and R = 1 (e_b1), >= 64 rows with V & 3 != 0 (e_b65, a_b65, d_b65)
TRAIN = {
    "editnet": {"e_b1": 0x1_0000_0001 + 11, "e_b17": 0x5_1234_5678, "e_b65": 0xABCD_0000_0007, "e_d512": 0x7_7654_3210},
    "adaptive": {"a_r100": 0x2_0000_0017, "a_b65": 0x9_0000_0018, "a_dead": 0x4_0000_0001},
    "dcnet": {"d_b1": 0x3_0000_001F, "d_b9": 0xC_0000_0020},
}
TABLES = dict(editnet=EDITNET, adaptive=ADAPTIVE, dcnet=DCNET, dcnet_mse={k: DCNET[k] for k in DCNET_MSE})


def _prev(seed, B, T, V, mode):
    prev, plen = synth.prev_captions(seed, B, T, V, min_len=1)
    if mode == "one":
        plen[:] = 1
    elif mode == "full":
        plen[:] = T
    else:
        plen[0, 0] = 1
    prev = synth.integers(seed, "prev.tok", (B, T), 1, V - 3) * (np.arange(T)[None, :] < plen)
    return prev.astype(np.int64), plen.astype(np.int64)


def _caps(seed, B, V, L, mode):
    if mode == "equal":
        lens = np.full(B, L, np.int64)
    elif mode == "min":
        lens = np.full(B, 2, np.int64)
    else:
        lens = synth.integers(seed, "cap.len", (B,), 2, L + 1)
        if B >= 3:
            lens[0], lens[B - 1] = L, L            # a tie between the first and the last row, and the full length
    W = max(L, 2)
    toks = synth.integers(seed, "cap.tok", (B, W), 1, V - 3)
    pos = np.arange(W)[None, :]
    toks = np.where(pos == 0, V - 2, toks)
    toks = np.where(pos == lens[:, None] - 1, V - 1, toks)
    toks = np.where(pos >= lens[:, None], 0, toks)
    return toks.astype(np.int64), lens.reshape(B, 1).astype(np.int64)


def affine_state(seed, D):
    k = 1.0 / np.sqrt(D)
    return {"affine_hidden.weight": synth.uniform(seed, "affine_hidden.weight", (D, D), -k, k),
            "affine_hidden.bias": synth.uniform(seed, "affine_hidden.bias", (D,), -k, k)}


@functools.lru_cache(maxsize=None)
def build(kind, name):
    row = TABLES[kind][name]
    if kind in ("editnet", "adaptive"):
        B, T, R, D, A, F, V, pm, cm, L, seed = row[:11]
        d = dict(dims=dict(B=B, T=T, R=R, D=D, A=A, F=F, V=V), sd=synth.editnet_state(seed, V, D, A, F, **SCALES))
        if kind == "adaptive":
            X = synth.features(seed, B, R, F)
            n = synth.integers(seed, "features.nvalid", (B,), 1, R + 1)
            n[:len(row[11])] = row[11]
            X = X * (np.arange(R)[None, :] < n[:, None])[:, :, None].astype(np.float32)
            if name == "a_dead":
                b, r, cols = DEAD
                X[b, r] *= np.float32(1e-4)
                bias = -(np.abs(d["sd"]["visual_attention.att_embed.0.bias"]) + np.float32(0.05))
                bias[list(cols)] = np.float32(0.3)
                d["sd"] = dict(d["sd"])
                d["sd"]["visual_attention.att_embed.0.bias"] = bias.astype(np.float32)
            d.update(X=X, image_mean=(X.sum(1) / n[:, None].astype(np.float32)).astype(np.float32), nvalid=n)
        else:
            d.update(X=synth.features(seed, B, R, F))
    else:
        B, T, D, A, C, E, V, pm, cm, L, seed = row
        sd = synth.dcnet_state(seed, V, D, A, C, E, **SCALES)
        d = dict(dims=dict(B=B, T=T, D=D, A=A, C=C, E=E, V=V), sd=sd)
        if kind == "dcnet_mse":
            d["affine"] = affine_state(seed, D)
    d["prev"], d["plen"] = _prev(seed, B, T, V, pm)
    d["caps"], d["clen"] = _caps(seed, B, V, L, cm)
    d["wm"] = synth.word_map(V)
    return d


def oracle_state(kind, d):
    """the numpy state dict under the names the module's named_parameters() uses"""
    if kind != "dcnet_mse":
        return d["sd"]
    sd = {"dae." + k: v for k, v in d["sd"].items()}
    sd.update(d["affine"])
    return sd


@functools.lru_cache(maxsize=None)
def oracle(kind, name, train=False):
    """float64 loss, scores, gradients and audits of one grid row (oracle.xe_grad_torch.gradients); train: under the
    dropout masks of TRAIN's seed for that row"""
    d = build(kind, name)
    dm = d["dims"]
    P = XG.leaf_params(oracle_state(kind, d))
    masks = None
    if train:
        seed = TRAIN["dcnet" if kind == "dcnet_mse" else kind][name]
        masks = XG.philox_masks(seed, d["clen"], d["plen"], dm["D"], R=dm.get("R", 0),
                                enc2=kind in ("adaptive", "dcnet_mse"), E=dm.get("E"))
    tail = (d["caps"], d["clen"], d["prev"], d["plen"], masks)
    if kind == "editnet":
        out = XG.editnet_xe(P, d["X"], *tail)
    elif kind == "adaptive":
        out = XG.adaptive_xe(P, d["X"], d["image_mean"], *tail)
    elif kind == "dcnet":
        out = XG.dcnet_xe(P, *tail)
    else:
        out = XG.dcnet_mse_xe(P, *tail)
    return XG.gradients(P, out)


def check_grads(named_grads, ref, what):
    """parity.check_grad_arrays against the float64 gradients `ref` ({name: array}) and their own norms"""
    import parity
    norms = {k: float(np.sqrt((np.asarray(r, np.float64) ** 2).sum())) for k, r in ref.items()}
    return parity.check_grad_arrays(named_grads, ref, norms, what)
