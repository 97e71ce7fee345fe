"""ORACLE (test infrastructure, not product): the decode timestep of EditNet and DCNet, one STAGE at a time, in float64.

oracle/editnet_np.py and oracle/dcnet_np.py restate a whole timestep; a test that chains them can only say "the step is off".
Here every stage takes its inputs explicitly, so a GPU test can feed a stage the DEVICE's own inputs to it and compare the
device's output of that stage alone (tests/test_hip_step_stages.py): rounding is not carried from stage to stage, the hard
arg-max of `select` is judged on the alpha_c it was actually given, and a failure names a stage.

`P` is a state_dict cast to float64 (oracle.editnet_np.cast_params(sd, np.float64)); every other input is cast to float64 on
entry and every result is float64.  The arithmetic follows oracle/editnet_np.py / oracle/dcnet_np.py and the reference lines
cited there; tests/test_step_stage_oracle_cpu.py pins the chained stages to those oracles.
"""
import numpy as np

from oracle.editnet_np import _linear, _sigmoid, _softmax

F64 = np.float64


def _f(x):
    return np.asarray(x, F64)


def _embed(P, tok):
    """EmbeddingC.forward, eval mode (editnet.py:300-304; dcnet.py:199-206): relu(E[tok])"""
    return np.maximum(P["embed.embedding.weight"][np.asarray(tok, np.int64)], 0)


def _lstm_cell(P, prefix, x, h, c):
    """nn.LSTMCell, gate order i, f, g, o"""
    gates = (x @ P[prefix + ".weight_ih"].T + P[prefix + ".bias_ih"] + h @ P[prefix + ".weight_hh"].T + P[prefix + ".bias_hh"])
    i, f, g, o = np.split(gates, 4, axis=1)
    c_new = _sigmoid(f) * c + _sigmoid(i) * np.tanh(g)
    return _sigmoid(o) * np.tanh(c_new), c_new


def _additive_scores(P, p, att1, h1, dec, full, act):
    att2 = _linear(h1, P, p + dec)
    return act(att1 + att2[:, None, :]) @ P[p + full + ".weight"][0] + P[p + full + ".bias"][0]


# ---------------------------------------------------------------------------------------------
# EditNet (editnet.py:527-545 / editnet_rl.py:505-513), eval mode
# ---------------------------------------------------------------------------------------------
def attention_lstm(P, tok, final_hidden, h2_prev, image_mean, h1_prev, c1_prev):
    """attention_lstm(cat([emb, final_hidden, h2, image_mean])) (editnet.py:527-532) -> h1, c1"""
    x1 = np.concatenate([_embed(P, tok), _f(final_hidden), _f(h2_prev), _f(image_mean)], 1)
    return _lstm_cell(P, "attention_lstm", x1, _f(h1_prev), _f(c1_prev))


def caption_attention(P, H, att1_c, h1, tok, mask):
    """CaptionAttentionC.forward with the context gate (editnet.py:364-381) -> alpha_c, attend_cap"""
    p = "caption_attention."
    H, h1, word = _f(H), _f(h1), _embed(P, tok)
    e = _additive_scores(P, p, _f(att1_c), h1, "cap_decoder_att", "cap_full_att", np.tanh)
    e = np.where(np.asarray(mask) == 0, -1e10, e)
    alpha_c = _softmax(e, 1)
    context = (H * alpha_c[:, :, None]).sum(1)
    zt = _sigmoid(_linear(np.concatenate([word, h1, context], 1), P, p + "context_gate"))
    tc = np.tanh(_linear(np.concatenate([word, h1], 1), P, p + "tc_affine"))
    return alpha_c, zt * np.tanh(_linear(context, P, p + "sc_affine")) + (1 - zt) * tc


def visual_attention(P, X, att1, h1, rmask=None):
    """VisualAttentionC.forward (editnet.py:439-447); with `rmask` (B,R) the adaptive form (editnet_adaptive.py:438-457):
    scores of regions with rmask == 0 are filled with -1e10, the context runs over the raw features -> alpha, attend_img"""
    X = _f(X)
    e = _additive_scores(P, "visual_attention.", _f(att1), _f(h1), "decoder_att", "full_att", lambda v: np.maximum(v, 0))
    if rmask is not None:
        e = np.where(np.asarray(rmask) == 0, -1e10, e)
    alpha = _softmax(e, 1)
    return alpha, (X * alpha[:, :, None]).sum(1)


def select_index(alpha_c):
    """the row SelectC's hard mode picks: the FIRST arg-max of the given weights (select_rows_k / the caption body's tie rule)"""
    return np.asarray(alpha_c).argmax(1)


def select(Mem, alpha_c):
    """SelectC.forward, hard mode (editnet.py:403-421): Mem[b, j*] * (a + (1 - a)), a = alpha_c[b, j*]; the factor is evaluated
    in float32 on the float32 value of a, as the reference and the kernel do"""
    Mem = _f(Mem)
    rows = np.arange(Mem.shape[0])
    j = select_index(alpha_c)
    a = np.asarray(alpha_c)[rows, j].astype(np.float32)
    w = a * np.float32(1) + (np.float32(1) - a)
    return Mem[rows, j] * w.astype(F64)[:, None]


def copy_lstm(P, h1, attend_cap, attend_img, h2_prev, c2_prev, sel):
    """CopyLSTMCellC.forward on cat([h1, attend_cap, attend_img]) (editnet.py:265-285, :537-541) -> h2, c2"""
    p = "copy_lstm."
    x = np.concatenate([_f(h1), _f(attend_cap), _f(attend_img)], 1)
    sel = _f(sel)
    gates = _linear(x, P, p + "x2h") + _linear(_f(h2_prev), P, p + "h2h")
    i, f, g, o = np.split(gates, 4, axis=1)
    c_new = _sigmoid(f) * _f(c2_prev) + _sigmoid(i) * np.tanh(g)
    copy_gate = _sigmoid(_linear(c_new, P, p + "gate_cnew") + _linear(sel, P, p + "gate_cmem"))
    c2 = copy_gate * sel + (1 - copy_gate) * c_new
    return _sigmoid(o) * np.tanh(c2), c2


def fc(P, h2):
    """fc(h2), eval mode: the dropout is the identity (editnet.py:545; dcnet.py:347)"""
    return _linear(_f(h2), P, "fc")


def region_mask(P, X):
    """The valid-region mask of the adaptive visual attention, the rule written above region_masks_k (editnet_adaptive.py:
    440-449): n_b = number of rows of X[b] with a non-zero sum; region r counts iff r < n_b (pack_padded_sequence keeps the
    FIRST n_b rows) and its embedded row relu(att_embed(X[b, r])) has a non-zero sum -> (B,R) of 0 / 1"""
    X = _f(X)
    n = (X.sum(2) != 0).sum(1)
    fe = np.maximum(_linear(X, P, "visual_attention.att_embed.0"), 0)
    return ((np.arange(X.shape[1])[None, :] < n[:, None]) & (fe.sum(2) != 0)).astype(F64)


def adaptive_att1(P, X):
    """features_att(att_embed(X)) with the embedded rows behind n_b zero, as the packed sequence pads them
    (editnet_adaptive.py:443-451) -> (B,R,A)"""
    X = _f(X)
    n = (X.sum(2) != 0).sum(1)
    fe = np.maximum(_linear(X, P, "visual_attention.att_embed.0"), 0)
    fe = fe * (np.arange(X.shape[1])[None, :] < n[:, None])[:, :, None]
    return _linear(fe, P, "visual_attention.features_att")


# ---------------------------------------------------------------------------------------------
# DCNet (dcnet.py:336-347 / dcnet_rl.py:306-312), eval mode
# ---------------------------------------------------------------------------------------------
def dc_attention_lstm(P, tok, final_hidden, h2_prev, h1_prev, c1_prev):
    """attention_lstm(cat([emb, final_hidden, h2])) (dcnet.py:336-340) -> h1, c1"""
    x1 = np.concatenate([_embed(P, tok), _f(final_hidden), _f(h2_prev)], 1)
    return _lstm_cell(P, "attention_lstm", x1, _f(h1_prev), _f(c1_prev))


def dc_caption_attention(P, enc, att1_c, h1, mask):
    """CaptionAttention.forward (dcnet.py:254-270): additive attention, no gate -> alpha_c, attend_cap"""
    enc = _f(enc)
    e = _additive_scores(P, "caption_attention.", _f(att1_c), _f(h1), "cap_decoder_att", "cap_full_att", np.tanh)
    e = np.where(np.asarray(mask) == 0, -1e10, e)
    alpha_c = _softmax(e, 1)
    return alpha_c, (enc * alpha_c[:, :, None]).sum(1)


def dc_language_lstm(P, h1, attend_cap, h2_prev, c2_prev):
    """language_lstm(cat([h1, attend_cap])) (dcnet.py:345-346) -> h2, c2"""
    return _lstm_cell(P, "language_lstm", np.concatenate([_f(h1), _f(attend_cap)], 1), _f(h2_prev), _f(c2_prev))
