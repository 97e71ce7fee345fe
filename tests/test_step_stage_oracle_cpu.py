"""CPU: the float64 stage oracle (tests/step_stage_oracle.py) chained over a few timesteps IS the whole-step oracle run in
float64 (oracle/editnet_np.py, oracle/dcnet_np.py, themselves pinned to the reference's goldens), and every shape of the GPU
grid (tests/step_stage_grid.py) still reaches the route its id names."""
import numpy as np
import pytest

import step_stage_grid as G
import step_stage_oracle as SO
from oracle import cases, dcnet_np as DN, editnet_np as EN

STEPS = 4
LIMIT = 1e-12          # the same arithmetic in float64 on both sides: relative to max|ref| of each tensor


def _same(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.dtype == np.float64 and got.shape == ref.shape, (what, got.dtype, got.shape, ref.shape)
    err, scale = float(np.abs(got - ref).max()), float(np.abs(ref).max())
    assert err <= LIMIT * scale, "%s: %.3e > %.0e * %.3e" % (what, err, LIMIT, scale)


def _chain_editnet(name, adaptive):
    d = cases.build_editnet(name)
    c = d["case"]
    P = EN.cast_params(d["sd"], np.float64)
    X = d["X"].astype(np.float64)
    mean = d["image_mean"].astype(np.float64) if adaptive else None
    S = EN.SeqState(P, X, d["prev"], d["plen"], mean, adaptive)
    B, D = c["B"], c["D"]
    att1 = SO.adaptive_att1(P, X) if adaptive else S.att1
    rmask = SO.region_mask(P, X) if adaptive else None
    h1, c1, h2, c2 = (np.zeros((B, D)) for _ in range(4))
    toks = cases.synth.integers(c["iseed"], "step.toks", (STEPS, B), 0, c["V"])
    for t in range(STEPS):
        tr = []
        EN.step(S, toks[t], None, tr)
        o = tr[0]
        h1, c1 = SO.attention_lstm(P, toks[t], S.final_hidden, h2, S.image_mean, h1, c1)
        alpha_c, attend_cap = SO.caption_attention(P, S.H, S.att1_c, h1, toks[t], S.mask)
        alpha, attend_img = SO.visual_attention(P, X, att1, h1, rmask)
        sel = SO.select(S.M, alpha_c)
        h2, c2 = SO.copy_lstm(P, h1, attend_cap, attend_img, h2, c2, sel)
        logits = SO.fc(P, h2)
        L = o["alpha"].shape[1]                         # the adaptive oracle cuts alpha behind the longest valid prefix
        assert not alpha[:, L:].any()
        got = dict(h1=h1, c1=c1, alpha_c=alpha_c, attend_cap=attend_cap, alpha=alpha[:, :L], attend_img=attend_img, sel=sel,
                   h2=h2, c2=c2, logits=logits)
        for k, v in got.items():
            _same(v, o[k], "%s step %d %s" % (name, t, k))


def test_editnet_stages_chain_to_the_step_oracle():
    _chain_editnet("editnet_small", False)


def test_adaptive_stages_chain_to_the_step_oracle():
    """the masked form of the visual stage (explicit att1 and rmask) against the adaptive oracle, which derives both itself"""
    _chain_editnet("editnet_adaptive_small", True)


def test_dcnet_stages_chain_to_the_step_oracle():
    d = cases.build_dcnet("dcnet_small")
    c = d["case"]
    P = DN.cast_params(d["sd"], np.float64)
    S = DN.SeqState(P, d["prev"], d["plen"])
    B, D = c["B"], c["D"]
    h1, c1, h2, c2 = (np.zeros((B, D)) for _ in range(4))
    toks = cases.synth.integers(c["iseed"], "step.toks", (STEPS, B), 0, c["V"])
    for t in range(STEPS):
        tr = []
        DN.step(S, toks[t], None, tr)
        o = tr[0]
        h1, c1 = SO.dc_attention_lstm(P, toks[t], S.final_hidden, h2, h1, c1)
        alpha_c, attend_cap = SO.dc_caption_attention(P, S.enc, S.att1_c, h1, S.mask)
        h2, c2 = SO.dc_language_lstm(P, h1, attend_cap, h2, c2)
        got = dict(h1=h1, c1=c1, alpha_c=alpha_c, attend_cap=attend_cap, h2=h2, c2=c2, logits=SO.fc(P, h2))
        for k, v in got.items():
            _same(v, o[k], "dcnet_small step %d %s" % (t, k))


def test_select_takes_the_first_arg_max_and_the_float32_factor():
    Mem = np.arange(2 * 3 * 4, dtype=np.float64).reshape(2, 3, 4) + 1
    alpha = np.array([[0.25, 0.5, 0.5], [0.1, 0.1, 0.1]], np.float32)
    sel = SO.select(Mem, alpha)
    assert sel.dtype == np.float64
    assert np.array_equal(SO.select_index(alpha), [1, 0])
    a = alpha[[0, 1], [1, 0]]
    w = (a * np.float32(1) + (np.float32(1) - a)).astype(np.float64)
    assert np.array_equal(sel, Mem[[0, 1], [1, 0]] * w[:, None])


# ---- the routes the GPU grid relies on -------------------------------------------------------------------------------------
def _assert_route(got, want, what):
    for k, v in want.items():
        assert got[k] == v, "%s: %s is %r, the grid entry is there for %r" % (what, k, got[k], v)


@pytest.mark.parametrize("gid", sorted(G.EDITNET_GRID))
def test_editnet_grid_entry_reaches_its_route(gid):
    e, dims = G.EDITNET_GRID[gid], G.editnet_dims(gid)
    assert dims["D"] % 32 == 0 and dims["A"] % 32 == 0 and dims["F"] % 32 == 0        # csrc/editnet.hip:63 check_dims
    for B, bt in e["runs"]:
        assert 1 <= bt <= B
        r = G.editnet_route(bt, dims["D"], dims["F"], dims["R"])
        _assert_route(r, e["route"], "%s %dx%d" % (gid, B, bt))
        assert (bt < B) == (gid == "shrunk")
        _assert_route(r, G.RUN_ROUTES.get((gid, B, bt), {}), "%s %dx%d" % (gid, B, bt))
    assert (gid == "nofuse") == (not G.editnet_route(17, dims["D"], dims["F"], dims["R"])["table"])


def test_editnet_grid_sits_on_both_sides_of_every_threshold():
    r = lambda gid, i=0: G.editnet_route(G.EDITNET_GRID[gid]["runs"][i][1], *(G.editnet_dims(gid)[k] for k in "DFR"))
    assert (r("rows16")["fused"], r("rows17")["fused"]) == (False, True)
    assert (r("rows64")["v2"], r("rows65")["v2"]) == (True, False)
    assert (r("rows64")["wide"], r("rows65")["wide"]) == (False, True)
    assert r("nofuse")["fused"] is False and G.EDITNET_GRID["nofuse"]["runs"][0][1] >= 17
    # the two slice widths of the 65+-row launch and the 128-column slices of a small batch
    assert (r("fslice_mid")["fsn"], r("fslice_mid")["fcols"]) == (2, 2048)
    assert (r("adaptive_mid")["fsn"], r("adaptive_mid")["fcols"]) == (2, 1024) and G.editnet_dims("adaptive_mid")["R"] > 48
    assert (r("fslice_small")["fsn"], r("fslice_small")["fcols"], r("fslice_small")["dsn"]) == (16, 256, 2)
    assert (r("fslice_small", 1)["fsn"], r("fslice_small", 1)["fcols"], r("fslice_small", 1)["dsn"]) == (32, 128, 2)
    assert len(G.editnet_cases()) == 2 * sum(len(e["runs"]) for e in G.EDITNET_GRID.values()) - 1


@pytest.mark.parametrize("gid", sorted(G.DCNET_GRID))
def test_dcnet_grid_entry_reaches_its_route(gid):
    e, dims = G.DCNET_GRID[gid], G.dcnet_dims(gid)
    for B, bt in e["runs"]:
        assert 1 <= bt <= B
        _assert_route(G.dcnet_route(bt, dims["D"], dims["C"]), e["route"], "%s %dx%d" % (gid, B, bt))
    # csrc/dcnet.hip:216-218: at C = 32 the kernels take no token table, so the DCNet grid runs without one
    assert G.dcnet_route(1, dims["D"], dims["C"])["table"] is False


def test_predicates_at_the_reference_shapes():
    """the restated conditions against what the comments in csrc/attention.hip say about the shapes they were tuned at"""
    assert G.vis_fsn(128, 2048, 36) == 1                 # "at B=128: one slice per sample"
    assert G.vis_fsn(4, 2048, 36) == 16                  # small batches: slices down to 128 columns
    assert G.vis_fsn(64, 2048, 100) == 2                 # adaptive features: two slices per sample
    assert G.cap_dsn(4, 1024) == 8 and G.cap_dsn(64, 1024) == 1
