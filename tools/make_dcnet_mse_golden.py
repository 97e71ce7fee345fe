#!/usr/bin/env python
"""Golden vectors of the DCNet MSE stage from the reference's own classes (`dcnet_with_mse.py`, authoring container only).

    python tools/make_dcnet_mse_golden.py      # writes tests/golden/dcnet_mse_<case>.npz and dcnet_mse_<case>_train.npz

`dcnet_with_mse.py` does not parse under Python 3: the docstring of `DAEWithAR` (:346-348) is indented deeper than the class
body.  Here the three lines are re-indented in memory, only the ClassDefs are kept and executed (as
oracle/ref_slice.load_classes does), and `DAEWithAR` is built without its checkpoint-loading __init__ (__new__ +
nn.Module.__init__ + its two attributes), `affine_hidden` from `affine_state` below.  Cases: dcnet_small and dcnet_full_b4
of oracle/cases.py (distinct caption lengths: the reference's unstable sort is the package's stable one).

eval mode (`eval.*`): sort order, scores (full for the small case, summaries at full size, as the other DCNet goldens),
gd_final_hidden, decoder_last_hidden after the affine, CE / MSE / total loss and the gradient of every parameter in the
`grad.` / `gradnorm.` / `gradslice.` schema of tests/test_hip_train_mode.py.  train mode (`train.*`): the same with the
Philox keep masks of show_edit_tell_amd/rng.py injected (oracle.make_train_golden.InjectedDropout): the caption positions
at (SITE_EMBED, t), the ground-truth encoder pass at SITE_ENC2_EMBED, the previous-caption encoder at SITE_ENC_EMBED, the
output dropout at (SITE_OUT, t).  Fixed zip time stamps and member order: two runs write bit-identical files.
"""
from __future__ import annotations

import ast
import io
import math
import os
import sys
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import cases  # noqa: E402
from show_edit_tell_amd import synth  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
# (case, train-mode dropout seed)
MSE_CASES = (("dcnet_small", 0x789A_BCDE_F012), ("dcnet_full_b4", 0x89AB_CDEF_0123))


def affine_state(c):
    """`affine_hidden` of the cases: nn.Linear(D, D)'s default range U(-1/sqrt(D), 1/sqrt(D)) from the case's weight seed"""
    D = c["D"]
    k = 1.0 / math.sqrt(D)
    return {"affine_hidden.weight": synth.uniform(c["wseed"], "affine_hidden.weight", (D, D), -k, k),
            "affine_hidden.bias": synth.uniform(c["wseed"], "affine_hidden.bias", (D,), -k, k)}


def golden_name(case, train):
    return "dcnet_mse_" + case[len("dcnet_"):] + ("_train" if train else "")


def load_classes():
    import torch
    import torch.nn as nn
    import torch.nn.functional as F
    from torch.nn.utils.rnn import PackedSequence, pack_padded_sequence, pad_packed_sequence
    from oracle import ref_slice
    path = os.path.join(ref_slice.REF_ROOT, "dcnet_with_mse.py")
    lines = open(path).read().split("\n")
    assert [lines[i].strip() for i in (345, 346, 347)] == ['"""', "Implements DAE with MSE Optimiztion", '"""'], lines[345:348]
    for i in (345, 346, 347):
        lines[i] = "    " + lines[i].strip()
    tree = ast.parse("\n".join(lines), filename=path)
    keep = ("Embedding", "CaptionEncoder", "CaptionAttention", "DAE", "DAEWithAR")
    body = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name in keep]
    ns = dict(torch=torch, nn=nn, F=F, math=math, np=np, device=torch.device("cpu"),
              pack_padded_sequence=pack_padded_sequence, pad_packed_sequence=pad_packed_sequence,
              PackedSequence=PackedSequence, Dataset=object)
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), ns)
    return {n.name: ns[n.name] for n in body}


def save_npz(path, arrays):
    """np.savez_compressed with a fixed member time stamp and order (numpy stamps members with the current time)."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o600 << 16
            z.writestr(info, buf.getvalue())


def make(name, seed, train):
    import torch
    import torch.nn as nn
    from torch.nn.utils.rnn import pack_padded_sequence
    from oracle import philox_np as PH, ref_slice
    from oracle.make_train_golden import InjectedDropout, _encoder_keep, _grads, _store_pred
    T_ = torch.from_numpy
    _np = lambda t: t.detach().cpu().numpy()
    cls = load_classes()
    d = cases.build_dcnet(name)
    c, wm = d["case"], d["wm"]
    small = c["D"] < 1024
    B, D, E, V = c["B"], c["D"], c["E"], c["V"]
    dae = ref_slice.load_state(cls["DAE"](wm, None, D, c["A"], c["C"], E), d["sd"])
    ar = cls["DAEWithAR"].__new__(cls["DAEWithAR"])          # (its __init__ loads 'BEST_checkpoint_3_dae.pth.tar')
    nn.Module.__init__(ar)
    ar.dae = dae
    ar.affine_hidden = nn.Linear(D, D)
    ar.affine_hidden.load_state_dict({k.split(".", 1)[1]: T_(v.copy()) for k, v in affine_state(c).items()})
    prev, plen, caps, clen = (T_(d[k]) for k in ("prev", "plen", "caps", "clen"))
    clen_s, sort_ind = clen.squeeze(1).sort(dim=0, descending=True)
    assert len(set(clen_s.tolist())) == B                   # distinct lengths: the unstable sort is the stable one
    dl = (clen_s - 1).tolist()
    Tm = max(dl)
    bts = [sum(l > t for l in dl) for t in range(Tm)]
    plen_s = plen[sort_ind]
    p = 0.5
    if train:
        def embed_keep(call, x):
            if call == 0:                   # dcnet_with_mse.py:319: all caption positions at once; position t feeds step t only
                keep = np.ones(tuple(x.shape), bool)
                for t in range(Tm):
                    keep[:bts[t], t] = PH.dropout_keep(seed, PH.site_offset(PH.SITE_EMBED, t), bts[t], E, p)
                return keep
            if call == 1:                   # :322 caption_encoder(sorted ground-truth captions)
                return _encoder_keep(seed, PH.SITE_ENC2_EMBED, p, clen_s.tolist(), x.shape, None)
            assert call == 2                # :323 caption_encoder(previous captions)
            return _encoder_keep(seed, PH.SITE_ENC_EMBED, p, _np(plen_s).reshape(-1), x.shape, None)

        def out_keep(t, x):
            return PH.dropout_keep(seed, PH.site_offset(PH.SITE_OUT, t), bts[t], D, p)

        dae.embed.dropout = InjectedDropout(p, embed_keep)
        dae.dropout = InjectedDropout(p, out_keep)
    ar.train(train)
    ar.zero_grad()
    pred, caps_s, dlr, si, gd_fh, last_h = ar(caps, clen, prev, plen)
    assert dlr == dl and torch.equal(si, sort_ind)
    if train:
        assert dae.embed.dropout.calls == 3 and dae.dropout.calls == Tm
    ce = nn.CrossEntropyLoss()(pack_padded_sequence(pred, dl, batch_first=True).data,
                               pack_padded_sequence(caps_s[:, 1:], dl, batch_first=True).data)
    mse = nn.MSELoss()(last_h, gd_fh)
    loss = ce + mse
    loss.backward()
    pre = "train." if train else "eval."
    out = {pre + "sort_ind": _np(sort_ind), pre + "ce": np.float64(ce.item()), pre + "mse": np.float64(mse.item()),
           pre + "loss": np.float64(loss.item()), pre + "gd_final": _np(gd_fh), pre + "last_hidden": _np(last_h),
           "keys": np.array(sorted(ar.state_dict()))}
    if train:
        out[pre + "seed"] = np.uint64(seed)
    _store_pred(_np(pred), small, V, out, pre)
    _grads(ar, small, out, pre)
    return out


def main(argv):
    import torch
    from oracle import ref_slice
    assert ref_slice.have_reference(), "needs the reference checkout (authoring container only)"
    torch.manual_seed(0)
    want = set(argv[1:])
    for name, seed in MSE_CASES:
        if want and name not in want:
            continue
        for train in (False, True):
            path = os.path.join(OUT, golden_name(name, train) + ".npz")
            o = make(name, seed, train)
            save_npz(path, o)
            pre = "train." if train else "eval."
            print("%-36s %8.1f KiB  ce %.6f  mse %.6f" % (os.path.basename(path), os.path.getsize(path) / 1024,
                                                         o[pre + "ce"], o[pre + "mse"]))


if __name__ == "__main__":
    main(sys.argv)
