"""CPU: the float64 prologue stages (tests/prologue_stage_oracle.py) chained ARE the prologue of the committed oracles run in
float64 (oracle/editnet_np.py, oracle/dcnet_np.py, themselves pinned to the reference's goldens); every shape of the GPU grid
(tests/prologue_stage_grid.py) reaches the route its id names under the setting it runs with; the entries together reach every
tile variant of the persistent encoder's <2,*> and <8,*> instantiations; and on every entry the float32 numpy stage stays under
HALF of the bound the GPU test applies to the device (an entry that does not is to be made shorter or given gentler weights:
the tolerance is never raised)."""
import numpy as np
import pytest

import parity
import prologue_stage_grid as G
import prologue_stage_oracle as PO
import step_stage_oracle as SO
from oracle import cases, dcnet_np as DN, editnet_np as EN

LIMIT = 1e-12          # the same arithmetic in float64 on both sides: relative to max|ref| of each tensor


def _same(got, ref, what):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.dtype == np.float64 and got.shape == ref.shape, (what, got.dtype, got.shape, ref.shape)
    err, scale = float(np.abs(got - ref).max()), float(np.abs(ref).max())
    assert scale > 0, what
    assert err <= LIMIT * scale, "%s: %.3e > %.0e * %.3e" % (what, err, LIMIT, scale)


def _nobias(x, P, name):
    return EN._linear(x, P, name) - P[name + ".bias"]


@pytest.mark.parametrize("name", ["editnet_small", "editnet_small_b24", "editnet_adaptive_small"])
def test_editnet_stages_chain_to_the_oracle(name):
    d = cases.build_editnet(name)
    adaptive = "image_mean" in d
    P = EN.cast_params(d["sd"], np.float64)
    X = d["X"].astype(np.float64)
    lens = d["plen"].reshape(-1)
    assert lens.max() == d["prev"].shape[1]                 # the oracle pads to the longest caption
    S = EN.SeqState(P, X, d["prev"], d["plen"], d["image_mean"].astype(np.float64) if adaptive else None, adaptive)
    got = PO.editnet_stages(P, d["prev"], lens, X, adaptive=adaptive, pv=True, mean=d["image_mean"] if adaptive else None)
    z = np.zeros_like(S.H)
    want = dict(H=S.H, M=S.M, final_hidden=S.final_hidden, mask=S.mask, att1_c=S.att1_c, att1=EN.visual_att1(P, X),
                image_mean=S.image_mean, mem_proj=_nobias(S.M, P, "copy_lstm.gate_cmem"),
                cap_proj=np.concatenate([_nobias(np.concatenate([z, z, S.H], 2), P, "caption_attention.context_gate"),
                                         _nobias(S.H, P, "caption_attention.sc_affine")], 2),
                pd_pv=_nobias(np.concatenate([np.zeros(X.shape[:2] + (2 * S.H.shape[2],)), X], 2), P, "copy_lstm.x2h"))
    B, D = S.final_hidden.shape
    x1 = np.concatenate([np.zeros((B, D)), S.final_hidden, np.zeros((B, D)), S.image_mean], 1)
    want["pre1"] = x1 @ P["attention_lstm.weight_ih"].T + P["attention_lstm.bias_ih"] + P["attention_lstm.bias_hh"]
    for k, v in want.items():
        _same(got[k], v, "%s %s" % (name, k))
    assert np.array_equal(got["mask"], np.arange(S.H.shape[1])[None, :] < lens[:, None])
    if adaptive:
        assert np.array_equal(got["rmask"], SO.region_mask(P, X))
        _same(got["att1"] * got["rmask"][:, :, None], SO.adaptive_att1(P, X) * got["rmask"][:, :, None], name + " att1")


@pytest.mark.parametrize("name", ["dcnet_small", "dcnet_small_end"])
def test_dcnet_stages_chain_to_the_oracle(name):
    d = cases.build_dcnet(name)
    c = d["case"]
    P = DN.cast_params(d["sd"], np.float64)
    lens = d["plen"].reshape(-1)
    assert lens.max() == d["prev"].shape[1]
    S = DN.SeqState(P, d["prev"], d["plen"])
    got = PO.dcnet_stages(P, d["prev"], lens, pc=True)
    B, D, E = c["B"], c["D"], c["E"]
    x1 = np.concatenate([np.zeros((B, E)), S.final_hidden, np.zeros((B, D))], 1)
    x2 = np.concatenate([np.zeros(S.enc.shape[:2] + (D,)), S.enc], 2)
    want = dict(enc=S.enc, final_hidden=S.final_hidden, mask=S.mask, att1_c=S.att1_c,
                pre1=x1 @ P["attention_lstm.weight_ih"].T + P["attention_lstm.bias_ih"] + P["attention_lstm.bias_hh"],
                pd_pc=x2 @ P["language_lstm.weight_ih"].T)
    for k, v in want.items():
        _same(got[k], v, "%s %s" % (name, k))


def test_reverse_direction_visits_len_minus_one_minus_t():
    """a row of length 2 in a batch padded to 3: the reverse half at position 1 is the FIRST reverse step (zero state), and
    position 0 the second"""
    d = cases.build_dcnet("dcnet_small")
    P = DN.cast_params(d["sd"], np.float64)
    C = d["case"]["C"]
    seq = np.array([[5, 7, 0], [3, 9, 11]])
    enc = PO.dc_encoder(P, seq, [2, 3])
    alone = PO.dc_encoder(P, seq[:1, :2], [2])
    _same(enc[0, :2], alone[0], "a row does not depend on its batch")
    assert not enc[0, 2].any()
    first = PO.dc_encoder(P, seq[:1, 1:2], [1])               # the word at position 1 alone
    _same(enc[0, 1, C:], first[0, 0, C:], "reverse half at the last valid position")
    assert np.abs(enc[0, 1, :C] - first[0, 0, :C]).max() > 1e-3


# ---- the routes the GPU grid relies on -------------------------------------------------------------------------------------
ENTRIES = [(m, g) for m in sorted(G.GRIDS) for g in G.GRIDS[m]]


@pytest.mark.parametrize("model,gid", ENTRIES, ids=["%s-%s" % e for e in ENTRIES])
def test_grid_entry_reaches_its_route(model, gid):
    e, r = G.entry(model, gid), G.route(model, gid)
    dims = e["dims"]
    for k, v in e["route"].items():
        assert r[k] == v, "%s: %s is %r, the grid entry is there for %r" % (gid, k, r[k], v)
    assert e["setting"] in G.SETTINGS
    if model == "dcnet":                                   # csrc/dcnet.hip:33-42 check_dims
        assert all(dims[k] % 32 == 0 for k in "DACE") and dims["D"] + 2 * dims["C"] == 2 * dims["E"]
        assert r["pc"] is False                             # no entry computes pd_pc (it needs D = E = 1024, A = 512, <= 8 rows)
    elif model == "editnet":                               # csrc/editnet.hip:59-66
        assert all(dims[k] % 32 == 0 for k in "DAF")
        assert r["pv"] is False                             # no entry computes pd_pv (it needs D = 1024, A = 512, <= 16 rows)
    # the conditions on the inputs
    inp = G.inputs(model, gid)
    lens, seq = inp["lens"], inp["seq"]
    assert lens.min() >= 1 and lens.max() == e["T"]
    valid = np.arange(e["T"])[None, :] < lens[:, None]
    assert (seq[valid] == 0).any() and (seq[valid] == dims["V"] - 1).any() and not seq[~valid].any()
    if isinstance(G.GRIDS[model][gid]["lens"], tuple):
        assert tuple(G.nactive_of(lens, e["T"])) == G.GRIDS[model][gid]["lens"]
        order = np.argsort(-lens, kind="stable")
        assert not np.array_equal(order, np.arange(e["B"])) and len(set(lens.tolist())) < e["B"]
    # persistent entries run under a setting that admits them; the same shape under the other settings does not
    if r["enc"] == "persistent":
        assert not G.persistent(e["B"], G.enc_dim(model, dims), "off")
        assert r["inst"][1] == G.enc_dim(model, dims) // 64


def test_grid_reaches_every_tile_variant():
    """NT = 2: 1 and 2 tiles; NT = 8: 1, 2, 4, 6 and 8 — each under both models' launches where the issue places them"""
    seen = {}
    for model, gid in ENTRIES:
        r = G.route(model, gid)
        if r["enc"] == "persistent":
            seen.setdefault(r["inst"][0], set()).update(r["variants"])
    assert seen[2] == {1, 2} and seen[8] == {1, 2, 4, 6, 8}
    dc = G.route("dcnet", "dc_pers8_b100")
    assert set(dc["variants"]) == {1, 2, 4, 6, 8}
    # every CHANGE of variant between consecutive steps of the <8,8> entry: 8 -> 6 -> 4 -> 2 -> 1
    e = G.entry("editnet", "pers8_b128")
    v = [G.tile_variant(8, n) for n in G.nactive_of(e["lens"], e["T"])]
    assert v == [8, 8, 6, 6, 6, 6, 4, 4, 4, 4, 2, 2, 1, 1]


def test_grid_sits_on_both_sides_of_every_threshold():
    r = lambda gid, m="editnet": G.route(m, gid)
    assert (r("pers_b32")["enc"], r("pers_b33_default")["enc"]) == ("persistent", "fused")          # maxb = 32
    assert (r("pers8_b128")["enc"], r("pers8_b129")["enc"]) == ("persistent", "fused")              # maxb = 128
    assert (r("pers_b32")["inst"], r("pers8_b33")["inst"]) == ((2, 8), (8, 8))                      # NT = 2 up to 32 rows
    assert (r("pers_b16")["variants"], r("pers_b17")["variants"]) == ([1], [2, 1])
    assert r("fusedstep_d512_b17")["enc"] == r("fusedstep_d512_b128")["enc"] == "fused"
    assert G.entry("editnet", "fusedstep_d512_b128")["lens"].tolist() == G.entry("editnet", "pers8_b128")["lens"].tolist()
    assert (r("fused_t1")["rows"], r("fused_b31")["rows"], r("fused_adaptive_b33")["rows"]) == (False, True, False)
    assert r("unfused_b70")["table"] is False and r("fused_b31")["table"] is True
    # odd and even T among the persistent entries (the ping-pong leaves the final state in (T & 1) ? hbuf1 : hbuf0)
    T = {g: G.entry("editnet", g)["T"] for g in ("pers_b1", "pers_b16", "pers_b17", "pers_b32", "pers_t1")}
    assert T["pers_b1"] % 2 == 1 and T["pers_b32"] % 2 == 0 and T["pers_t1"] == 1
    assert G.entry("editnet", "pers_b1")["lens"].tolist() == [T["pers_b1"]]       # its one row runs to the last step
    assert len([1 for e in ENTRIES if G.entry(*e)["dims"].get("D") == 1024]) == 1


def test_persistent_d64_instantiations_are_unreachable():
    """encoder_persistent.hip builds <2,1>, <8,1> and <16,1> for D = 64 and persistent_encoder_ok admits D = 64, but both
    callers ask for `fused` (D % 128 == 0) first: no D reaches them."""
    assert G.persistent_encoder_ok(4, 64) and G.instantiation(4, 64) == (2, 1) and G.instantiation(200, 64) == (16, 1)
    for D in range(32, 2049, 32):
        for B in (1, 32):
            if G.persistent(B, D):
                assert D in (512, 1024) and G.instantiation(B, D)[1] in (8, 16)


# ---- the float32 oracle against the bounds ---------------------------------------------------------------------------------
_STATE = {}


def _params(model, dims):
    key = (model,) + tuple(sorted(dims.items()))
    if key not in _STATE:
        _STATE.clear()
        sd = G.state(model, dims)
        _STATE[key] = (EN.cast_params(sd, np.float64), EN.cast_params(sd))
    return _STATE[key]


def _ratio(got, ref, tol):
    scale = float(np.abs(ref).max())
    assert scale > 0
    return parity.maxerr(got, ref) / (tol * min(scale, 1.0))


@pytest.mark.parametrize("model,gid", ENTRIES, ids=["%s-%s" % e for e in ENTRIES])
def test_float32_stages_stay_under_half_of_every_bound(model, gid):
    """the float32 numpy prologue stands in for the device: every stage in float32 on ITS outputs against the float64 stage on
    the same inputs, as a fraction of parity.STATE_TOL * min(max|ref|, 1)"""
    e, inp = G.entry(model, gid), G.inputs(model, gid)
    P, P32 = _params(model, e["dims"])
    if model == "dcnet":
        dev = {k: v.astype(np.float32) for k, v in PO.dcnet_stages(P32, inp["seq"], inp["lens"], pc=True).items()}
        ref = PO.dcnet_stages(P, inp["seq"], inp["lens"], dev, pc=True)
    elif model == "op":
        H, M = PO.encoder(P32, inp["seq"], inp["lens"])
        dev = dict(H=H, M=M, final_hidden=PO.final_hidden(P32, H, inp["lens"]))
        Hr, Mr = PO.encoder(P, inp["seq"], inp["lens"])
        ref = dict(H=Hr, M=Mr, final_hidden=PO.final_hidden(P, H, inp["lens"]))
    else:
        ad = bool(e["dims"]["adaptive"])
        dev = PO.editnet_stages(P32, inp["seq"], inp["lens"], inp["X"], adaptive=ad, pv=True, mean=inp["mean"])
        dev = {k: v.astype(np.float32) for k, v in dev.items()}
        ref = PO.editnet_stages(P, inp["seq"], inp["lens"], inp["X"], dev, adaptive=ad, pv=True, mean=inp["mean"])
    worst = {}
    for k, v in ref.items():
        if k in ("mask", "rmask"):
            assert np.array_equal(dev[k], v), k
        else:
            worst[k] = _ratio(dev[k], v, parity.STATE_TOL)
    print(gid, {k: round(v, 3) for k, v in worst.items()})
    assert max(worst.values()) < 0.5, worst
