"""ORACLE / TEST INFRASTRUCTURE — never imported by the product package.

float64, differentiable torch-CPU restatement of the teacher-forced forwards, for gradient parity at shapes no
reference-autograd golden was captured for:

  editnet_xe    DecoderC.forward of the reference's `editnet.py:479-548` (sub-modules `:226-447`)
  adaptive_xe   `adaptive_features/editnet_adaptive.py:438-457, 489-562` (masked visual attention, image mean given,
                gd_final_hidden / decoder_last_hidden for the CE + MSE loss `:594-596`)
  dcnet_xe      DAE.forward of `dcnet.py:199-270, 303-350`
  dcnet_mse_xe  the six-output DAE + DAEWithAR of `dcnet_with_mse.py:303-360`

Written functionally over a {state_dict key: float64 leaf tensor} mapping like oracle/editnet_torch.py (whose
dtype-agnostic per-operator functions are reused); no reference text is copied.  The loss is the packed cross-entropy of
`editnet.py:571-577`; `gradients()` runs torch autograd on the CPU.  tests/test_xe_grad_oracle_cpu.py pins every function
to the reference's own autograd gradients stored in tests/golden, in eval and in train mode.

Row order: the caption-length sort is the STABLE descending one the package uses (any order of tied rows is a valid
outcome of the reference's unstable sort); the caption encoders are written per row ("advance while t < len"), which is
what the reference's internal sort + shrinking batch prefix computes.

Train mode: `masks` (see `philox_masks`) holds one keep mask per dropout site and timestep, generated with
oracle.philox_np exactly the way oracle/make_train_golden.py feeds them to the reference's classes: y = x * keep / (1 - p).

Two audits are accumulated in `aud` while a forward runs (the conditions under which a comparison in fp32 needs no
allowance):
  select_gap_min  smallest top-1 - top-2 gap of alpha_c over all rows / timesteps with more than one unmasked position
                  (SelectC is a hard arg-max: below rounding noise the other memory row may legitimately be taken)
  kink_count      number of ReLU pre-activations within fp32 summation noise of zero: `att_embed` with
                  |p| <= 1e-6 * max(1, |W x| + |b|), and relu(att1 + att2) of the visual attention with
                  |p| <= 1e-6 * max(1, |att1| + |att2|) (masked / padded regions of the adaptive model are not counted)
  truncated_steps adaptive model: number of timesteps at which the count-based truncation removes an unmasked region (a
                  valid region's embedded row is entirely zero there, so the unmasked regions are not packed at the front)
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from . import philox_np as PH
from .editnet_torch import attention_lstm, caption_attention, copy_lstm, lstm_cell_c, select_hard

F64 = torch.float64
P_DROP = 0.5            # every nn.Dropout of the three models


def leaf_params(sd_np):
    """float64 leaf tensors with requires_grad from a numpy state dict (the shared embedding appears once)"""
    return {k: torch.from_numpy(np.asarray(v, dtype=np.float64).copy()).requires_grad_(True) for k, v in sd_np.items()
            if k != "caption_encoder.embed.embedding.weight"}


def new_audit():
    return {"select_gap_min": float("inf"), "kink_count": 0, "truncated_steps": 0}


def _t64(x):
    return torch.from_numpy(np.asarray(x, dtype=np.float64).copy())


def _ti(x):
    return torch.from_numpy(np.asarray(x, dtype=np.int64).copy())


def _lin(P, name, x):
    return F.linear(x, P[name + ".weight"], P[name + ".bias"])


def _drop(x, keep):
    """nn.Dropout(0.5) with a supplied keep mask (None: eval mode, the identity)"""
    if keep is None:
        return x
    assert tuple(keep.shape) == tuple(x.shape), (keep.shape, x.shape)
    return x * torch.from_numpy(np.ascontiguousarray(keep)).to(x.dtype) / (1.0 - P_DROP)


def _sort(clen):
    clen = np.asarray(clen).reshape(-1)
    sort_ind = np.argsort(-clen, kind="stable")
    return sort_ind, clen[sort_ind]


def _audit_gap(aud, alpha, mask):
    many = mask.sum(1) > 1
    if bool(many.any()):
        top = alpha.detach()[many].topk(2, dim=1).values
        aud["select_gap_min"] = min(aud["select_gap_min"], float((top[:, 0] - top[:, 1]).min()))


# ---------------------------------------------------------------------------------------------------------------------
# EditNet
# ---------------------------------------------------------------------------------------------------------------------
def embed(P, ids, keep=None):
    """EmbeddingC.forward (editnet.py:300-304) / Embedding.forward of DCNet (dcnet.py:199-206)"""
    return _drop(torch.relu(F.embedding(ids, P["embed.embedding.weight"])), keep)


def caption_encoder_c(P, seq, lens, keep=None):
    """CaptionEncoderC.forward (editnet.py:319-348): per row, the cell advances while t < len; H / M rows behind a
    caption's length stay zero, final_hidden = tanh(affine(last h)), mask = M.sum(2) != 0"""
    lens = torch.as_tensor(np.asarray(lens).reshape(-1))
    tmax = int(lens.max())
    B = seq.shape[0]
    D = P["caption_encoder.affine_hn.weight"].shape[0]
    emb = embed(P, seq[:, :tmax], keep)
    h, c = torch.zeros(B, D, dtype=F64), torch.zeros(B, D, dtype=F64)
    Hs, Ms = [], []
    for t in range(tmax):
        act = (lens > t).to(F64).unsqueeze(1)
        hn, cn = lstm_cell_c(P, "caption_encoder.lstm_encoder_cell", emb[:, t], h, c)
        h, c = act * hn + (1 - act) * h, act * cn + (1 - act) * c
        Hs.append(act * hn)
        Ms.append(act * cn)
    H, M = torch.stack(Hs, 1), torch.stack(Ms, 1)
    mask = (M.detach().sum(2) != 0).to(F64)
    return H, M, torch.tanh(_lin(P, "caption_encoder.affine_hn", h)), mask


def _region_embedding(P, X, aud, nvalid=None):
    """relu(att_embed.0(X)) (editnet.py:441) before its dropout; adaptive: only the first nvalid[b] regions are embedded
    (the packed rows of editnet_adaptive.py:440-448), the padded ones stay exactly zero"""
    W, b = P["visual_attention.att_embed.0.weight"], P["visual_attention.att_embed.0.bias"]
    wx = F.linear(X, W)
    pre = wx + b
    near = pre.detach().abs() <= 1e-6 * torch.clamp(wx.detach().abs() + b.detach().abs(), min=1.0)
    Y = torch.relu(pre)
    if nvalid is not None:
        live = (torch.arange(X.shape[1])[None, :] < nvalid[:, None])
        near = near & live[:, :, None]
        Y = Y * live[:, :, None].to(F64)
    aud["kink_count"] += int(near.sum())
    return Y


def _visual_attention(P, X, fe, h1, aud, adaptive):
    """VisualAttentionC.forward behind the region embedding `fe` (editnet.py:442-447; editnet_adaptive.py:449-456: score
    mask from the embedded rows' sums, alpha and the features truncated to the largest unmasked COUNT of the batch prefix,
    not renormalised)"""
    att1 = _lin(P, "visual_attention.features_att", fe)
    att2 = _lin(P, "visual_attention.decoder_att", h1).unsqueeze(1)
    pre = att1 + att2
    near = pre.detach().abs() <= 1e-6 * torch.clamp(att1.detach().abs() + att2.detach().abs(), min=1.0)
    e = _lin(P, "visual_attention.full_att", torch.relu(pre)).squeeze(2)
    if not adaptive:
        aud["kink_count"] += int(near.sum())
        return (X * F.softmax(e, dim=1).unsqueeze(2)).sum(1)
    att_masks = fe.detach().sum(2) != 0
    aud["kink_count"] += int((near & att_masks[:, :, None]).sum())
    alpha = F.softmax(e.masked_fill(~att_masks, -1e10), dim=1)
    n = int(att_masks.sum(1).max())
    last = (att_masks.to(F64) * torch.arange(1, att_masks.shape[1] + 1, dtype=F64)).max(1).values     # 1 + last unmasked index
    aud["truncated_steps"] += int(bool((last > n).any()))
    return (X[:, :n] * alpha[:, :n].unsqueeze(2)).sum(1)


def _editnet(P, X, caps, clen, prev, plen, masks, image_mean, adaptive):
    aud = new_audit()
    sort_ind, clen_s = _sort(clen)
    dl = (clen_s - 1).tolist()
    X = _t64(np.asarray(X)[sort_ind])
    caps_s = _ti(np.asarray(caps)[sort_ind])
    prev_s, plen_s = _ti(np.asarray(prev)[sort_ind]), np.asarray(plen).reshape(-1)[sort_ind]
    B, R = X.shape[0], X.shape[1]
    D, V = P["fc.weight"].shape[1], P["fc.weight"].shape[0]
    m = masks or {}
    H, M, final_hidden, mask = caption_encoder_c(P, prev_s, plen_s, m.get("enc"))
    gd_final = None
    nvalid = None
    if adaptive:
        _, _, gd_final, _ = caption_encoder_c(P, caps_s, clen_s, m.get("enc2"))          # editnet_adaptive.py:516
        mean = _t64(np.asarray(image_mean)[sort_ind])
        nvalid = (X.sum(2) != 0).sum(1)
    else:
        mean = X.mean(1)
    Y = _region_embedding(P, X, aud, nvalid)
    h1, c1, h2, c2 = (torch.zeros(B, D, dtype=F64) for _ in range(4))
    Tm = max(dl)
    pred = torch.zeros(B, Tm, V, dtype=F64)
    last = [None] * B
    for t in range(Tm):
        bt = sum(l > t for l in dl)
        emb = embed(P, caps_s[:bt, t], m["embed"][t] if masks else None)
        h1, c1 = attention_lstm(P, torch.cat([emb, final_hidden[:bt], h2[:bt], mean[:bt]], 1), h1[:bt], c1[:bt])
        attend_cap, alpha_c = caption_attention(P, H[:bt], h1, emb, mask[:bt])
        _audit_gap(aud, alpha_c, mask[:bt])
        fe = _drop(Y[:bt], m["region"][t].reshape(bt, R, D) if masks else None)
        attend_img = _visual_attention(P, X[:bt], fe, h1, aud, adaptive)
        sel = select_hard(M[:bt], alpha_c)
        h2, c2 = copy_lstm(P, torch.cat([h1, attend_cap, attend_img], 1), h2[:bt], c2[:bt], sel)
        pred[:bt, t] = _lin(P, "fc", _drop(h2, m["out"][t] if masks else None))
        for b in range(bt):
            last[b] = h2[b]
    out = dict(pred=pred, caps=caps_s, dl=dl, sort_ind=sort_ind, aud=aud)
    if adaptive:
        out.update(gd_final=gd_final, last_hidden=torch.stack(last, 0))
    return out


def editnet_xe(P, X, caps, clen, prev, plen, masks=None):
    return _editnet(P, X, caps, clen, prev, plen, masks, None, False)


def adaptive_xe(P, X, image_mean, caps, clen, prev, plen, masks=None):
    return _editnet(P, X, caps, clen, prev, plen, masks, image_mean, True)


# ---------------------------------------------------------------------------------------------------------------------
# DCNet
# ---------------------------------------------------------------------------------------------------------------------
def _lstm_dir(P, sfx, x, lens, reverse):
    """one direction of the packed nn.LSTM (dcnet.py:217,233): per row over its own valid positions"""
    p = "caption_encoder.lstm_encoder."
    W_ih, W_hh = P[p + "weight_ih_l0" + sfx], P[p + "weight_hh_l0" + sfx]
    b = P[p + "bias_ih_l0" + sfx] + P[p + "bias_hh_l0" + sfx]
    B, T, _ = x.shape
    C = W_hh.shape[1]
    h, c = torch.zeros(B, C, dtype=F64), torch.zeros(B, C, dtype=F64)
    outs = [None] * T
    for t in (range(T - 1, -1, -1) if reverse else range(T)):
        act = (lens > t).to(F64).unsqueeze(1)
        i, f, g, o = (F.linear(x[:, t], W_ih) + F.linear(h, W_hh) + b).chunk(4, 1)
        cn = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        hn = torch.sigmoid(o) * torch.tanh(cn)
        h, c = act * hn + (1 - act) * h, act * cn + (1 - act) * c
        outs[t] = act * hn
    return torch.stack(outs, 1), h


def dcnet_caption_encoder(P, src, lens, keep=None):
    """CaptionEncoder.forward (dcnet.py:220-243)"""
    lens = torch.as_tensor(np.asarray(lens).reshape(-1))
    tmax = int(lens.max())
    x = embed(P, src[:, :tmax], keep)
    of, hf = _lstm_dir(P, "", x, lens, False)
    ob, hb = _lstm_dir(P, "_reverse", x, lens, True)
    outputs = torch.cat([of, ob], 2)
    mask = (outputs.detach().sum(2) != 0).to(F64)
    return outputs, torch.tanh(_lin(P, "caption_encoder.concat", torch.cat([hf, hb], 1))), mask


def dcnet_caption_attention(P, feats, h1, mask):
    """CaptionAttention.forward (dcnet.py:254-270)"""
    att1 = _lin(P, "caption_attention.cap_features_att", feats)
    att2 = _lin(P, "caption_attention.cap_decoder_att", h1)
    e = _lin(P, "caption_attention.cap_full_att", torch.tanh(att1 + att2.unsqueeze(1))).squeeze(2)
    alpha = F.softmax(e.masked_fill(mask == 0, -1e10), dim=1)
    return (feats * alpha.unsqueeze(2)).sum(1)


def _nn_lstm_cell(P, pre, x, h, c):
    g = F.linear(x, P[pre + ".weight_ih"], P[pre + ".bias_ih"]) + F.linear(h, P[pre + ".weight_hh"], P[pre + ".bias_hh"])
    i, f, gg, o = g.chunk(4, 1)
    c_new = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(gg)
    return torch.sigmoid(o) * torch.tanh(c_new), c_new


def _dcnet(P, caps, clen, prev, plen, masks, hidden):
    sort_ind, clen_s = _sort(clen)
    dl = (clen_s - 1).tolist()
    caps_s = _ti(np.asarray(caps)[sort_ind])
    prev_s, plen_s = _ti(np.asarray(prev)[sort_ind]), np.asarray(plen).reshape(-1)[sort_ind]
    B = caps_s.shape[0]
    D, V = P["fc.weight"].shape[1], P["fc.weight"].shape[0]
    m = masks or {}
    gd_final = None
    if hidden:                                                                    # dcnet_with_mse.py:322
        _, gd_final, _ = dcnet_caption_encoder(P, caps_s, clen_s, m.get("enc2"))
    enc, final_hidden, mask = dcnet_caption_encoder(P, prev_s, plen_s, m.get("enc"))
    h1, c1, h2, c2 = (torch.zeros(B, D, dtype=F64) for _ in range(4))
    Tm = max(dl)
    pred = torch.zeros(B, Tm, V, dtype=F64)
    last = [torch.zeros(D, dtype=F64)] * B
    for t in range(Tm):
        bt = sum(l > t for l in dl)
        emb = embed(P, caps_s[:bt, t], m["embed"][t] if masks else None)
        h1, c1 = _nn_lstm_cell(P, "attention_lstm", torch.cat([emb, final_hidden[:bt], h2[:bt]], 1), h1[:bt], c1[:bt])
        attend_cap = dcnet_caption_attention(P, enc[:bt], h1, mask[:bt])
        h2, c2 = _nn_lstm_cell(P, "language_lstm", torch.cat([h1, attend_cap], 1), h2[:bt], c2[:bt])
        pred[:bt, t] = _lin(P, "fc", _drop(h2, m["out"][t] if masks else None))
        for b in range(bt):
            last[b] = h2[b]
    out = dict(pred=pred, caps=caps_s, dl=dl, sort_ind=sort_ind, aud=new_audit())
    if hidden:
        out.update(gd_final=gd_final, last_hidden=torch.stack(last, 0))
    return out


def dcnet_xe(P, caps, clen, prev, plen, masks=None):
    return _dcnet(P, caps, clen, prev, plen, masks, False)


def dcnet_mse_xe(P, caps, clen, prev, plen, masks=None):
    """DAEWithAR.forward (dcnet_with_mse.py:345-360); P holds the DAE's keys with the `dae.` prefix and `affine_hidden.*`"""
    inner = {k[4:]: v for k, v in P.items() if k.startswith("dae.")}
    out = _dcnet(inner, caps, clen, prev, plen, masks, True)
    out["last_hidden"] = _lin(P, "affine_hidden", out["last_hidden"])
    return out


# ---------------------------------------------------------------------------------------------------------------------
# loss, gradients, masks
# ---------------------------------------------------------------------------------------------------------------------
def xe_loss(out):
    """CrossEntropyLoss (mean) over the packed rows (editnet.py:571-577) — train.xe_loss_sum / n_tok"""
    pred, caps_s, dl = out["pred"], out["caps"], out["dl"]
    tot, n = 0.0, 0
    for b, L in enumerate(dl):
        if L:
            tot = tot + F.cross_entropy(pred[b, :L], caps_s[b, 1:L + 1], reduction="sum")
            n += L
    return tot / n


def total_loss(out):
    """CE, plus MSELoss(decoder_last_hidden, gd_final_hidden) where the forward returns the two
    (editnet_adaptive.py:594-596, dcnet_with_mse.py:388-392)"""
    loss = xe_loss(out)
    if "gd_final" in out:
        loss = loss + F.mse_loss(out["last_hidden"], out["gd_final"])
    return loss


def gradients(P, out):
    """loss.backward() by torch autograd; returns a plain-numpy result"""
    loss = total_loss(out)
    for p in P.values():
        p.grad = None
    loss.backward()
    res = dict(loss=float(loss.detach()), pred=out["pred"].detach().numpy(), dl=out["dl"], sort_ind=out["sort_ind"],
               grads={k: (p.grad.numpy() if p.grad is not None else None) for k, p in P.items()},
               select_gap_min=out["aud"]["select_gap_min"], kink_count=out["aud"]["kink_count"],
               truncated_steps=out["aud"]["truncated_steps"])
    for k in ("gd_final", "last_hidden"):
        if k in out:
            res[k] = out[k].detach().numpy()
    return res


def philox_masks(seed, clen, plen, D, R=0, enc2=False, E=None):
    """keep masks of a train-mode forward with `rng.dropout_seed(seed)`, addressed as show_edit_tell_amd/rng.py addresses
    them (rows = the stably sorted batch; oracle/make_train_golden.py): the previous-caption encoder's embedding
    (B * Tmax, E) at SITE_ENC_EMBED, with `enc2` the ground-truth pass at SITE_ENC2_EMBED, and per timestep t the word
    embedding (bt, E) at (SITE_EMBED, t), with R > 0 the region embedding (bt * R, D) at (SITE_REGION, t), and the output
    dropout (bt, D) at (SITE_OUT, t)."""
    E = D if E is None else E
    sort_ind, clen_s = _sort(clen)
    plen_s = np.asarray(plen).reshape(-1)[sort_ind]
    B = len(clen_s)
    dl = (clen_s - 1).tolist()
    bts = [sum(l > t for l in dl) for t in range(max(dl))]

    def enc_keep(site, lens):
        tmax = int(max(lens))
        return PH.dropout_keep(seed, PH.site_offset(site), B * tmax, E, P_DROP).reshape(B, tmax, E)

    m = dict(enc=enc_keep(PH.SITE_ENC_EMBED, plen_s),
             embed=[PH.dropout_keep(seed, PH.site_offset(PH.SITE_EMBED, t), bt, E, P_DROP) for t, bt in enumerate(bts)],
             out=[PH.dropout_keep(seed, PH.site_offset(PH.SITE_OUT, t), bt, D, P_DROP) for t, bt in enumerate(bts)])
    if enc2:
        m["enc2"] = enc_keep(PH.SITE_ENC2_EMBED, clen_s)
    if R:
        m["region"] = [PH.dropout_keep(seed, PH.site_offset(PH.SITE_REGION, t), bt * R, D, P_DROP)
                       for t, bt in enumerate(bts)]
    return m
