"""ORACLE (test infrastructure, not product): the decode PROLOGUE of EditNet and DCNet (set_editnet_begin / set_dcnet_begin),
one STAGE at a time, in float64.

The companion of tests/step_stage_oracle.py for everything that happens once per sequence: the caption encoder's recurrence,
final_hidden, mask, the hoisted projections and pre1.  Every stage takes its inputs explicitly, so a GPU test feeds a stage the
DEVICE's own inputs to it (tests/test_hip_prologue_stages.py): rounding is not carried from stage to stage, no row is filtered
and a failure names a stage.  The recurrence is ONE stage (tokens and weights in, H / Mem out), because the persistent encoder
is one launch.

`P` is a state_dict cast with oracle.editnet_np.cast_params: float64 for the reference stages; the same functions evaluated on
a float32 `P` are "the float32 numpy oracle's stage" whose error the tests print next to the device's.  Every other input is
cast to P's dtype on entry.  tests/test_prologue_stage_oracle_cpu.py pins the chained stages to oracle/editnet_np.py and
oracle/dcnet_np.py (the recurrences are written differently here: per-row positions, the reverse direction as len - 1 - t).
"""
import numpy as np

from oracle.editnet_np import _linear, _sigmoid


def _dt(P):
    return P["embed.embedding.weight"].dtype


def _f(P, x):
    return np.asarray(x, _dt(P))


def _embed(P, tok):
    """EmbeddingC.forward / Embedding.forward, eval mode (editnet.py:300-304; dcnet.py:199-206): relu(E[tok])"""
    return np.maximum(P["embed.embedding.weight"][np.asarray(tok, np.int64)], 0)


def _recurrence(xg, w_hh, b_hh, lens, reverse, want_c):
    """T cell updates (gate order i, f, g, o) on the hoisted input projection xg (B,T,4D): step t visits row b while t < len_b,
    at position t (forward) or len_b - 1 - t (reverse: nn.LSTM's backward direction on a packed batch); h and c carry over;
    positions behind a row's length stay zero -> out_h (B,T,D), out_c or None"""
    B, T, D4 = xg.shape
    D = D4 // 4
    h = np.zeros((B, D), xg.dtype)
    c = np.zeros((B, D), xg.dtype)
    out_h = np.zeros((B, T, D), xg.dtype)
    out_c = np.zeros((B, T, D), xg.dtype) if want_c else None
    for t in range(T):
        rows = np.flatnonzero(lens > t)
        if not rows.size:
            break
        pos = lens[rows] - 1 - t if reverse else np.full(rows.size, t)
        gates = xg[rows, pos] + h[rows] @ w_hh.T + b_hh
        i, f, g, o = np.split(gates, 4, axis=1)
        cn = _sigmoid(f) * c[rows] + _sigmoid(i) * np.tanh(g)
        hn = _sigmoid(o) * np.tanh(cn)
        h[rows], c[rows] = hn, cn
        out_h[rows, pos] = hn
        if want_c:
            out_c[rows, pos] = cn
    return out_h, out_c


def _lens(lens, B):
    lens = np.asarray(lens, np.int64).reshape(-1)
    assert lens.shape == (B,) and lens.min() >= 1, "every length is at least 1 (the reference cannot pack a zero length)"
    return lens


def _last(S, lens, pos=None):
    """S[b, len_b - 1] (pos = None) or S[b, pos]"""
    rows = np.arange(S.shape[0])
    return S[rows, lens - 1 if pos is None else pos]


# ---------------------------------------------------------------------------------------------
# EditNet (editnet.py:319-348 CaptionEncoderC, :364-381, :281, :441-442, :503, :527-532), eval mode
# ---------------------------------------------------------------------------------------------
def encoder(P, seq, lens):
    """CaptionEncoderC.forward's recurrence from tokens and weights (editnet.py:329-338): relu(embed), x2h, T LSTMCellC updates
    -> H, Mem (B,T,D), T = seq.shape[1]"""
    seq = np.asarray(seq, np.int64)
    lens = _lens(lens, seq.shape[0])
    p = "caption_encoder.lstm_encoder_cell."
    xg = _linear(_embed(P, seq), P, p + "x2h")
    return _recurrence(xg, P[p + "h2h.weight"], P[p + "h2h.bias"], lens, False, True)


def final_hidden(P, H, lens):
    """tanh(affine_hn(h_last)), h_last[b] = H[b, len_b - 1] (editnet.py:339-345)"""
    H = _f(P, H)
    return np.tanh(_linear(_last(H, _lens(lens, H.shape[0])), P, "caption_encoder.affine_hn"))


def mask(P, Mem):
    """(Mem.sum(2) != 0) (editnet.py:340; dcnet.py:239 on the encoder outputs)"""
    return (_f(P, Mem).sum(2) != 0).astype(_dt(P))


def att1_c(P, H):
    """cap_features_att(H) (editnet.py:370; dcnet.py:261 on enc)"""
    return _linear(_f(P, H), P, "caption_attention.cap_features_att")


def cap_proj(P, H):
    """[context_gate.W[:, 2D:3D] H_t | sc_affine.W H_t] (B,T,2D), no bias: the halves of editnet.py:378-379 that are linear in
    the attention context"""
    H = _f(P, H)
    D = H.shape[2]
    return np.concatenate([H @ P["caption_attention.context_gate.weight"][:, 2 * D:3 * D].T,
                           H @ P["caption_attention.sc_affine.weight"].T], 2)


def mem_proj(P, Mem):
    """gate_cmem.W Mem_t (B,T,D), no bias (editnet.py:281)"""
    return _f(P, Mem) @ P["copy_lstm.gate_cmem.weight"].T


def fe(P, X):
    """relu(att_embed(X)) (editnet.py:441), every region row"""
    return np.maximum(_linear(_f(P, X), P, "visual_attention.att_embed.0"), 0)


def att1(P, fe_):
    """features_att(fe) (editnet.py:442)"""
    return _linear(_f(P, fe_), P, "visual_attention.features_att")


def pd_pv(P, X):
    """X copy_lstm.x2h.W[:, 2D:]^T (B,R,4D), no bias: the region half of copy_lstm.x2h (editnet.py:537-541), hoisted for the
    persistent small-batch decode"""
    D = P["attention_lstm.weight_ih"].shape[0] // 4
    return _f(P, X) @ P["copy_lstm.x2h.weight"][:, 2 * D:].T


def rmask(P, X, fe_):
    """the adaptive model's valid-region mask (editnet_adaptive.py:440-449; step_stage_oracle.region_mask) on the given fe:
    region r counts iff r < n_b = #rows of X[b] with a non-zero sum, and fe[b, r] has a non-zero sum (fe >= 0: any entry)"""
    X, fe_ = _f(P, X), _f(P, fe_)
    n = (X.sum(2) != 0).sum(1)
    return ((np.arange(X.shape[1])[None, :] < n[:, None]) & (fe_.sum(2) != 0)).astype(_dt(P))


def image_mean(P, X):
    """mean over the R regions (editnet.py:503)"""
    return _f(P, X).mean(1)


def pre1(P, final_hidden_, image_mean_):
    """the loop-invariant part of the attention LSTM's gates (editnet.py:527-532): weight_ih columns [D,2D) on final_hidden
    and [3D,3D+F) on image_mean, + bias_ih + bias_hh"""
    fh, im = _f(P, final_hidden_), _f(P, image_mean_)
    D = fh.shape[1]
    W = P["attention_lstm.weight_ih"]
    return fh @ W[:, D:2 * D].T + im @ W[:, 3 * D:].T + P["attention_lstm.bias_ih"] + P["attention_lstm.bias_hh"]


def editnet_stages(P, seq, lens, X, dev=None, adaptive=False, pv=False, mean=None):
    """Every stage, each on `dev`'s version of its inputs (keys H, M, fe, final_hidden, image_mean: what the device left);
    dev = None chains the stages on their own outputs.  mean: the caller's image_mean (adaptive features), copied as it is."""
    out = {}
    out["H"], out["M"] = encoder(P, seq, lens)
    d = out if dev is None else dev
    out["final_hidden"] = final_hidden(P, d["H"], lens)
    out["mask"] = mask(P, d["M"])
    out["att1_c"] = att1_c(P, d["H"])
    out["cap_proj"] = cap_proj(P, d["H"])
    out["mem_proj"] = mem_proj(P, d["M"])
    out["fe"] = fe(P, X)
    out["att1"] = att1(P, d["fe"])
    if pv:
        out["pd_pv"] = pd_pv(P, X)
    if adaptive:
        out["rmask"] = rmask(P, X, d["fe"])
    out["image_mean"] = image_mean(P, X) if mean is None else _f(P, mean)
    out["pre1"] = pre1(P, d["final_hidden"], d["image_mean"])
    return out


# ---------------------------------------------------------------------------------------------
# DCNet (dcnet.py:220-243 CaptionEncoder, :261, :336-346), eval mode
# ---------------------------------------------------------------------------------------------
def dc_encoder(P, seq, lens):
    """the BiLSTM over the packed batch (dcnet.py:217,233) -> enc (B,T,2C) = [forward | reverse]"""
    seq = np.asarray(seq, np.int64)
    lens = _lens(lens, seq.shape[0])
    p = "caption_encoder.lstm_encoder."
    x = _embed(P, seq)
    halves = []
    for sfx, reverse in (("", False), ("_reverse", True)):
        xg = x @ P[p + "weight_ih_l0" + sfx].T + P[p + "bias_ih_l0" + sfx]
        halves.append(_recurrence(xg, P[p + "weight_hh_l0" + sfx], P[p + "bias_hh_l0" + sfx], lens, reverse, False)[0])
    return np.concatenate(halves, 2)


def dc_final_hidden(P, enc, lens):
    """tanh(concat W [hf_last | hb_last]) (dcnet.py:241-242): hf_last = enc[b, len_b - 1, :C], hb_last = enc[b, 0, C:]"""
    enc = _f(P, enc)
    C = enc.shape[2] // 2
    lens = _lens(lens, enc.shape[0])
    last = np.concatenate([_last(enc, lens)[:, :C], _last(enc, lens, 0)[:, C:]], 1)
    return np.tanh(_linear(last, P, "caption_encoder.concat"))


def dc_pd_pc(P, enc):
    """enc language_lstm.W_ih[:, D:]^T (B,T,4D), no bias: the context half of language_lstm's input product (dcnet.py:345-346),
    hoisted for the persistent small-batch decode"""
    D = P["attention_lstm.weight_ih"].shape[0] // 4
    return _f(P, enc) @ P["language_lstm.weight_ih"][:, D:].T


def dc_pre1(P, final_hidden_):
    """attention_lstm.weight_ih columns [E, E+2C) on final_hidden + bias_ih + bias_hh (dcnet.py:336-340)"""
    fh = _f(P, final_hidden_)
    E = P["embed.embedding.weight"].shape[1]
    return (fh @ P["attention_lstm.weight_ih"][:, E:E + fh.shape[1]].T + P["attention_lstm.bias_ih"]
            + P["attention_lstm.bias_hh"])


def dcnet_stages(P, seq, lens, dev=None, pc=False):
    """as editnet_stages; dev keys enc, final_hidden"""
    out = {"enc": dc_encoder(P, seq, lens)}
    d = out if dev is None else dev
    out["final_hidden"] = dc_final_hidden(P, d["enc"], lens)
    out["mask"] = mask(P, d["enc"])
    out["att1_c"] = att1_c(P, d["enc"])
    if pc:
        out["pd_pc"] = dc_pd_pc(P, d["enc"])
    out["pre1"] = dc_pre1(P, d["final_hidden"])
    return out
