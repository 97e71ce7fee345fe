"""CPU: the float64 autograd restatement (oracle/xe_grad_torch.py) against the REFERENCE's own autograd values stored in
tests/golden — loss and every parameter gradient, eval mode and train mode (Philox keep masks regenerated in numpy) — which
is what makes it an oracle for tests/test_hip_grad_shapes.py; and, for every row of that test's grid (tests/grad_grid.py),
the two conditions under which the GPU comparison excuses nothing: no hard-select near-tie and no ReLU kink."""
import numpy as np
import pytest

import grad_grid as G
import parity
from oracle import cases, xe_grad_torch as XG
from tools.make_dcnet_mse_golden import affine_state, golden_name


def _pin(res, g, pre, loss_key, what):
    """loss within 1e-4 and the project's gradient criterion (parity.check_grad_arrays) against the golden's stored values"""
    assert abs(res["loss"] - float(g[loss_key])) < 1e-4, (what, res["loss"], float(g[loss_key]))
    names = [k[len(pre + "gradnorm."):] for k in g if k.startswith(pre + "gradnorm.")]
    parity.check_grad_arrays(res["grads"].items(), {k: g[pre + "grad." + k] for k in names},
                             {k: float(g[pre + "gradnorm." + k]) for k in names}, what + " vs the reference")


def _editnet_case(name, train):
    d = cases.build_editnet(name)
    c = d["case"]
    adaptive = name in cases.ADAPTIVE_CASES
    g = parity.load(("train_" if train else "") + name)
    masks = None
    if train:
        masks = XG.philox_masks(int(g["train.seed"]), d["clen"], d["plen"], c["D"], R=c["R"], enc2=adaptive)
    P = XG.leaf_params(d["sd"])
    tail = (d["caps"], d["clen"], d["prev"], d["plen"], masks)
    out = XG.adaptive_xe(P, d["X"], d["image_mean"], *tail) if adaptive else XG.editnet_xe(P, d["X"], *tail)
    return g, XG.gradients(P, out)


@pytest.mark.parametrize("name", ["editnet_small", "editnet_adaptive_small"])
def test_editnet_eval_gradients_equal_the_references(name):
    g, res = _editnet_case(name, False)
    parity.assert_close(res["pred"][parity.unsort(res["sort_ind"])], g["xe_pred"][parity.unsort(g["xe_sort_ind"])],
                        parity.LOGIT_TOL, "scores")
    _pin(res, g, "", "grad_loss", name + " eval")


@pytest.mark.parametrize("name", ["editnet_small", "editnet_adaptive_small"])
def test_editnet_train_mode_gradients_equal_the_references(name):
    g, res = _editnet_case(name, True)
    assert np.array_equal(res["sort_ind"], g["train.sort_ind"])
    parity.assert_close(res["pred"], g["train.pred"], parity.LOGIT_TOL, "train-mode scores")
    if "gd_final" in res:
        parity.assert_close(res["gd_final"], g["train.gd_final"], parity.STATE_TOL, "gd_final_hidden")
        parity.assert_close(res["last_hidden"], g["train.last_hidden"], parity.STATE_TOL, "decoder_last_hidden")
    _pin(res, g, "train.", "train.loss", name + " train")


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
def test_dcnet_gradients_equal_the_references(train):
    name = "dcnet_small"
    d = cases.build_dcnet(name)
    c = d["case"]
    g = parity.load(("train_" if train else "") + name)
    masks = XG.philox_masks(int(g["train.seed"]), d["clen"], d["plen"], c["D"], E=c["E"]) if train else None
    P = XG.leaf_params(d["sd"])
    res = XG.gradients(P, XG.dcnet_xe(P, d["caps"], d["clen"], d["prev"], d["plen"], masks))
    if train:
        parity.assert_close(res["pred"], g["train.pred"], parity.LOGIT_TOL, "train-mode scores")
        _pin(res, g, "train.", "train.loss", name + " train")
    else:
        _pin(res, g, "", "grad_loss", name + " eval")


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
def test_dcnet_mse_gradients_equal_the_references(train):
    name = "dcnet_small"
    d = cases.build_dcnet(name)
    c = d["case"]
    g = parity.load(golden_name(name, train))
    pre = "train." if train else "eval."
    masks = None
    if train:
        masks = XG.philox_masks(int(g["train.seed"]), d["clen"], d["plen"], c["D"], enc2=True, E=c["E"])
    sd = {"dae." + k: v for k, v in d["sd"].items()}
    sd.update(affine_state(c))
    P = XG.leaf_params(sd)
    res = XG.gradients(P, XG.dcnet_mse_xe(P, d["caps"], d["clen"], d["prev"], d["plen"], masks))
    parity.assert_close(res["pred"], g[pre + "pred"], parity.LOGIT_TOL, pre + "scores")
    parity.assert_close(res["gd_final"], g[pre + "gd_final"], parity.STATE_TOL, pre + "gd_final_hidden")
    parity.assert_close(res["last_hidden"], g[pre + "last_hidden"], parity.STATE_TOL, pre + "decoder_last_hidden")
    _pin(res, g, pre, pre + "loss", name + " MSE " + pre)


GRID = [(kind, name, False) for kind, tab in G.TABLES.items() for name in tab] + \
       [(kind, name, True) for kind, tab in G.TRAIN.items() for name in tab]


@pytest.mark.parametrize("kind,name,train", GRID, ids=["%s-%s-%s" % (k, n, "train" if t else "eval") for k, n, t in GRID])
def test_grid_rows_need_no_allowance(kind, name, train):
    """select_gap_min >= 1e-4 is ten times the 1e-5 that tests/test_hip_shapes.py treats as rounding noise of the hard
    arg-max; kink_count == 0: no ReLU pre-activation where another fp32 summation order may take the other branch"""
    res = G.oracle(kind, name, train)
    print(kind, name, "train" if train else "eval", "loss %.6f" % res["loss"], "select gap %.3e" % res["select_gap_min"],
          "kinks", res["kink_count"])
    assert np.isfinite(res["loss"])
    assert all(v is not None and np.isfinite(v).all() for v in res["grads"].values())
    assert res["select_gap_min"] >= 1e-4, res["select_gap_min"]
    assert res["kink_count"] == 0, res["kink_count"]
    # the reference's count-based truncation (editnet_adaptive.py:455-456) acts in exactly one place of the grid: the train-mode
    # run of a_dead, where the dropout zeroes a non-trailing valid region of the longest row at some steps and not at others
    if (kind, name, train) == ("adaptive", "a_dead", True):
        assert 1 <= res["truncated_steps"] < max(res["dl"]), res["truncated_steps"]
    else:
        assert res["truncated_steps"] == 0, res["truncated_steps"]
    d = G.build(kind, name)
    dl = res["dl"]
    assert res["pred"].shape == (d["dims"]["B"], max(dl), d["dims"]["V"])
    for b, L in enumerate(dl):
        assert not res["pred"][b, L:].any()


def test_count_truncation_detector():
    """xe_sequence.count_truncation_bites (what sends an adaptive batch from the sequence node to the per-operator route):
    True exactly when a live row has an unmasked region at an index >= the largest unmasked count of the live rows"""
    import torch
    from show_edit_tell_amd.xe_sequence import count_truncation_bites as bites
    packed = torch.tensor([[1., 1, 1, 0], [1, 1, 0, 0], [1, 0, 0, 0]])
    hole = torch.tensor([[1., 0, 1, 1], [1, 1, 0, 0], [1, 0, 0, 0]])            # row 0: count 3, last unmasked index 3
    assert not bites(packed, [3, 2])
    assert bites(hole, [3, 1])
    assert not bites(torch.stack([packed, hole]), [3, 0])                        # the hole sits in a step with no live row
    assert bites(torch.stack([packed, hole.flip(0)]), [3, 3])                    # ... and in the last row of a live step
    covered = torch.tensor([[1., 0, 1, 0], [1, 1, 1, 0]])                        # another live row's count covers the index
    assert not bites(covered, [2]) and bites(covered, [1])
