"""CPU: the DCNet MSE-stage goldens (tests/golden/dcnet_mse_*.npz, tools/make_dcnet_mse_golden.py: the reference's own
`dcnet_with_mse.py` classes) against the numpy oracle, and the module surface of show_edit_tell_amd.dcnet_with_mse:
the reference's state_dict keys, and a strict hand-off of its state to the stage-3 dcnet_rl.DAEWithAR."""
import numpy as np
import pytest
import torch

import parity
from oracle import cases, dcnet_np as DN
from oracle.editnet_np import _log_softmax
from tools.make_dcnet_mse_golden import affine_state, golden_name


def _oracle_mse(name):
    """dcnet_with_mse.py:303-343 + DAEWithAR.forward + the train() loss in numpy, eval mode"""
    d = cases.build_dcnet(name)
    c = d["case"]
    P = DN.cast_params(d["sd"])
    aff = affine_state(c)
    clen = d["clen"].reshape(-1)
    sort_ind = np.argsort(-clen, kind="stable")
    caps, clen_s = d["caps"][sort_ind], clen[sort_ind]
    prev, plen = d["prev"][sort_ind], d["plen"][sort_ind]
    dl = (clen_s - 1).tolist()
    _, gd_final, _ = DN.caption_encoder(P, caps, clen_s)
    S = DN.SeqState(P, prev, plen)
    B, D = caps.shape[0], S.h2.shape[1]
    last = np.zeros((B, D), np.float32)
    ce, n = 0.0, 0
    for t in range(max(dl)):
        bt = sum(l > t for l in dl)
        logits = DN.step(S, caps[:bt, t], bt)
        logp = _log_softmax(logits.astype(np.float64), 1)
        ce -= logp[np.arange(bt), caps[:bt, t + 1]].sum()
        n += bt
        last[:bt] = S.h2                                     # dcnet_with_mse.py:341
    last = last @ aff["affine_hidden.weight"].T + aff["affine_hidden.bias"]
    mse = float(((last.astype(np.float64) - gd_final) ** 2).mean())
    return sort_ind, gd_final, last, ce / n, mse


@pytest.mark.parametrize("name", ["dcnet_small", "dcnet_full_b4"])
def test_oracle_reproduces_the_mse_golden(name):
    g = parity.load(golden_name(name, False))
    sort_ind, gd_final, last, ce, mse = _oracle_mse(name)
    assert np.array_equal(sort_ind, g["eval.sort_ind"])
    parity.assert_close(gd_final, g["eval.gd_final"], parity.STATE_TOL, "gd_final_hidden")
    parity.assert_close(last, g["eval.last_hidden"], parity.STATE_TOL, "decoder_last_hidden (after affine_hidden)")
    assert abs(ce - float(g["eval.ce"])) < 1e-4
    assert abs(mse - float(g["eval.mse"])) < 1e-5
    assert abs(ce + mse - float(g["eval.loss"])) < 1e-4
    # ragged caption lengths: the last-step selection matters (rows end at different steps)
    assert len(set(np.asarray(cases.build_dcnet(name)["clen"]).reshape(-1).tolist())) > 1


@pytest.mark.parametrize("name", ["dcnet_small", "dcnet_full_b4"])
def test_mse_goldens_present_and_consistent(name):
    ge, gt = parity.load(golden_name(name, False)), parity.load(golden_name(name, True))
    assert int(gt["train.seed"]) > 2 ** 32
    for g, pre in ((ge, "eval."), (gt, "train.")):
        norms = [k for k in g if k.startswith(pre + "gradnorm.")]
        assert len(norms) == len(g["keys"]) - 1 and all(np.isfinite(g[k]) for k in norms)   # (the shared embedding once)
        assert float(g[pre + "gradnorm.affine_hidden.weight"]) > 0
        assert abs(float(g[pre + "ce"]) + float(g[pre + "mse"]) - float(g[pre + "loss"])) < 1e-6
    assert abs(float(gt["train.loss"]) - float(ge["eval.loss"])) > 1e-3     # the masks really acted


def _modules(name):
    from show_edit_tell_amd import dcnet, dcnet_rl, dcnet_with_mse
    d = cases.build_dcnet(name)
    c = d["case"]
    args = (d["wm"], None, c["D"], c["A"], c["C"], c["E"])
    stage1 = dcnet.DAE(*args)
    ar = dcnet_with_mse.DAEWithAR(dae=stage1)
    return d, args, stage1, ar, dcnet_rl, dcnet_with_mse


def test_dae_with_ar_state_dict_keys_are_the_references():
    g = parity.load(golden_name("dcnet_small", False))
    d, args, stage1, ar, dcnet_rl, M = _modules("dcnet_small")
    assert sorted(ar.state_dict()) == g["keys"].tolist()
    assert ar.dae is stage1 and type(stage1) is M.DAE               # taken over in place, as unpickling does
    assert isinstance(ar.affine_hidden, torch.nn.Linear) and tuple(ar.affine_hidden.weight.shape) == (64, 64)
    with pytest.raises(TypeError):
        M.DAEWithAR(dae=dcnet_rl.DAE(*args))


def test_stage2_state_loads_strictly_into_stage3():
    d, args, stage1, ar, dcnet_rl, M = _modules("dcnet_small")
    with torch.no_grad():
        for i, p in enumerate(ar.parameters()):
            p.copy_(torch.full_like(p, 0.01 * (i + 1)))
    rl = dcnet_rl.DAEWithAR(dae=dcnet_rl.DAE(*args))
    rl.load_state_dict(ar.state_dict(), strict=True)
    for k, v in ar.state_dict().items():
        assert torch.equal(rl.state_dict()[k], v), k


def test_whole_module_save_load_round_trip(tmp_path):
    d, args, stage1, ar, dcnet_rl, M = _modules("dcnet_small")
    path = str(tmp_path / "dae_ar.pth.tar")
    torch.save({"dae_ar": ar}, path)
    back = torch.load(path, weights_only=False)["dae_ar"]
    assert type(back) is M.DAEWithAR and type(back.dae) is M.DAE
    assert back.dae.caption_encoder._owner() is back.dae
    for k, v in ar.state_dict().items():
        assert torch.equal(back.state_dict()[k], v), k
