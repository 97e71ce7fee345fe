"""GPU: every stage of the decode PROLOGUE (set_editnet_begin / set_dcnet_begin, and the set_caption_encoder_f32 operator)
against its float64 restatement, at the shapes where the prologue changes route.

The caption encoder's recurrence runs as one persistent launch (csrc/encoder_persistent.hip, seven instantiations, the tile
count dispatched per step), as the fused per-step kernel (csrc/gemm_fused.hip) or unfused; which one is decided by the dims, the
row count and two switches that are read once per process.  So one child process per setting of tests/prologue_stage_grid.py
(default, SET_ENC_PERSISTENT_MAXB=128, SET_ENC_PERSISTENT=0) runs its cases one after another: it fills the prologue's outputs
with NaN, calls the prologue through the C ABI, reads every product back through set_*_ws_tensor and saves them with the
weights it used.  The parent evaluates tests/prologue_stage_oracle.py on the DEVICE's own inputs to each stage (the recurrence
from tokens and weights; final_hidden on the device's H[b, len_b - 1]; the projections on the device's H / Mem / enc / fe; pre1
on the device's final_hidden and image_mean), so rounding is not carried forward and every row of every case is compared.
Every case whose prologue takes the inference token table runs without and with it, judged by the same float64 stages.  The
routes are asserted on the CPU (tests/test_prologue_stage_oracle_cpu.py) and, here, by the library's own profile: a case meant
for the persistent encoder shows a `persistent_encoder` launch, every other case shows none and shows its own kernel.  A launch
the library refused (another process owns the device's persistent launches) is reported as a skip AFTER the stages have been
judged on the kernel that ran instead: never a pass on the wrong kernel.

Tolerance: parity.STATE_TOL for every stage, relative to max|ref| of the tensor AND absolute (stage_judge.judge).  Exact
checks: H / Mem / enc are bit-zero behind a row's length, mask is exactly 1.0 / 0.0, padded rows of att1_c hold the bias bit
for bit and those of cap_proj / mem_proj +0, the region mask and a caller's image_mean are exact, no NaN is left anywhere, the
status word behind the persistent encoder's barrier words is 0, and the row list holds the valid rows where it is in use.

PROLOGUE_STAGES_ERRORS_OUT=<path> additionally writes, per model, grid id and stage, the largest error as a fraction of its
bound, next to the same figure for the float32 numpy oracle's stage on the same inputs (profiles/prologue_stages_errors.json).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import parity
import prologue_stage_grid as G
import prologue_stage_oracle as PO
from oracle import editnet_np as EN
from stage_judge import judge, write_report

pytestmark = pytest.mark.gpu

RATIOS = {}            # (model, grid id) -> stage -> [largest hip ratio, largest float32-oracle ratio]
STATUS_WORD = 17 * 32  # csrc/grid_barrier.h: GBAR_WORDS = (8 + 1 + 8) * GBAR_STRIDE unsigned words, the status word behind them

_CHILD = r"""
import ctypes as C, json, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.join(os.getcwd(), "tests")); sys.path.insert(0, os.getcwd())
import prologue_stage_grid as G
from hip_adapter import load_numpy_state, to_dev
from show_edit_tell_amd import _lib, synth
out_path, setting = sys.argv[1], sys.argv[2]
for k, v in G.SETTINGS[setting].items():
    assert os.environ.get(k) == v, (k, os.environ.get(k))
lib = _lib.load()
NAN = float("nan")
out, models = {}, {}
EDIT_KEEP = ("embed.", "caption_encoder.lstm", "caption_encoder.affine", "caption_attention.cap_features_att",
             "caption_attention.context_gate.weight", "caption_attention.sc_affine.weight", "copy_lstm.gate_cmem.weight",
             "visual_attention.att_embed", "visual_attention.features_att", "attention_lstm.weight_ih", "attention_lstm.bias")
DC_KEEP = ("embed.", "caption_encoder.lstm", "caption_encoder.concat", "caption_attention.cap_features_att",
           "attention_lstm.weight_ih", "attention_lstm.bias")


def model_of(kind, gid):
    dims = G.entry(kind, gid)["dims"]
    key = G.model_key(kind, dims)
    if key not in models:
        models.clear()                                    # one model on the device at a time
        sd = G.state(kind, dims)
        wm = synth.word_map(dims["V"])
        if kind == "dcnet":
            from show_edit_tell_amd import dcnet
            m = dcnet.DAE(wm, None, dims["D"], dims["A"], dims["C"], dims["E"])
            keep = DC_KEEP + (("language_lstm.weight_ih",) if G.route(kind, gid).get("pc") else ())
        else:
            from show_edit_tell_amd import editnet, editnet_adaptive
            cls = editnet_adaptive.DecoderC if dims.get("adaptive") else editnet.DecoderC
            D = dims["D"]
            m = cls(wm, D, D, D, dims.get("A", 32), dims.get("F", 32))
            keep = EDIT_KEEP + (("copy_lstm.x2h.weight",) if G.route(kind, gid).get("pv") else ())
        models[key] = load_numpy_state(m, sd)
        for name, p in models[key].state_dict().items():       # the weights as the device holds them
            if name.startswith(keep):
                out["W:%s|%s" % (key, name)] = p.detach().cpu().numpy()
    return models[key]


def weights(model, dims, table):
    if not table:
        w = model._weights()
        assert not w.tok_table
        return w
    for _ in range(2):                                    # the table is built once the same weights were seen twice
        w = model._weights(dims)
    assert w.tok_table, "no token table attached"
    return w


def profiled(call, what):
    torch.cuda.synchronize()
    lib.set_profile_enable(1)
    _lib.check(call(), what)
    torch.cuda.synchronize()
    prof = {p["tag"]: p["launches"] for p in _lib.profile_report()}
    lib.set_profile_enable(0)
    return json.dumps(prof)


with torch.no_grad():
    for case in G.cases(setting):
        kind, gid, table = case
        cid = G.case_id(case)
        e, inp = G.entry(kind, gid), G.inputs(kind, gid)
        dm, B, T = e["dims"], e["B"], e["T"]
        model = model_of(kind, gid)
        seq, lens = to_dev(inp["seq"]), to_dev(inp["lens"])
        st = _lib.stream_of(seq.device)
        if kind == "op":
            D = dm["D"]
            enc = model.caption_encoder
            cell = enc.lstm_encoder_cell
            w = _lib.EditNetWeights()
            w.embed = enc.embed.embedding.weight.data_ptr()
            w.enc_x2h_w, w.enc_x2h_b = cell.x2h.weight.data_ptr(), cell.x2h.bias.data_ptr()
            w.enc_h2h_w, w.enc_h2h_b = cell.h2h.weight.data_ptr(), cell.h2h.bias.data_ptr()
            w.enc_aff_w, w.enc_aff_b = enc.affine_hn.weight.data_ptr(), enc.affine_hn.bias.data_ptr()
            res = {k: torch.full(shp, NAN, dtype=torch.float32, device=seq.device)
                   for k, shp in dict(H=(B, T, D), M=(B, T, D), final_hidden=(B, D), mask=(B, T)).items()}
            ws = torch.empty(lib.set_caption_encoder_workspace_bytes(B, T, D), dtype=torch.uint8, device=seq.device)
            out[cid + "|prof"] = profiled(lambda: lib.set_caption_encoder_f32(
                C.byref(w), _lib.ptr(seq), _lib.ptr(lens), _lib.ptr(res["H"]), _lib.ptr(res["M"]), _lib.ptr(res["final_hidden"]),
                _lib.ptr(res["mask"]), B, T, D, dm["V"], _lib.ptr(ws), ws.numel(), st), "set_caption_encoder_f32")
            for k, v in res.items():
                out[cid + "|" + k] = v.cpu().numpy()
            continue
        r = G.route(kind, gid)
        if kind == "editnet":
            D, A, F, R = dm["D"], dm["A"], dm["F"], dm["R"]
            dims = model._dims(B, T, R, 19)
            shapes = dict(H=(B, T, D), M=(B, T, D), final_hidden=(B, D), mask=(B, T), att1_c=(B, T, A), cap_proj=(B, T, 2 * D),
                          mem_proj=(B, T, D), fe=(B, R, D), att1=(B, R, A), image_mean=(B, F), pre1=(B, 4 * D))
            if dm["adaptive"]:
                shapes["rmask"] = (B, R)
            if r["pv"]:
                shapes["pd_pv"] = (B, R, 4 * D)
        else:
            D, A, Cc = dm["D"], dm["A"], dm["C"]
            dims = model._dims(B, T, 19)
            shapes = dict(enc=(B, T, 2 * Cc), final_hidden=(B, 2 * Cc), mask=(B, T), att1_c=(B, T, A), pre1=(B, 4 * D))
            if r["pc"]:
                shapes["pd_pc"] = (B, T, 4 * D)
        ws = model._new_workspace(dims)
        w = weights(model, dims, table)
        get = lambda name, shp, dt=torch.float32: model.ws_tensor(dims, name, shp, dt, ws=ws)
        for k, shp in shapes.items():
            get(k, shp).fill_(NAN)
        if kind == "editnet":
            get("pro_count", (1,), torch.int32).fill_(-1)
            X = to_dev(inp["X"])
            mean = None if inp["mean"] is None else to_dev(inp["mean"])
            call = lambda: lib.set_editnet_begin(C.byref(w), C.byref(dims), _lib.ptr(X), _lib.ptr(mean), _lib.ptr(seq),
                                                 _lib.ptr(lens), _lib.ptr(ws), ws.numel(), st)
        else:
            call = lambda: lib.set_dcnet_begin(C.byref(w), C.byref(dims), _lib.ptr(seq), _lib.ptr(lens), _lib.ptr(ws),
                                               ws.numel(), st)
        out[cid + "|prof"] = profiled(call, "begin " + cid)
        for k, shp in shapes.items():
            out[cid + "|" + k] = get(k, shp).cpu().numpy()
        out[cid + "|status"] = get("enc_bar", (18 * 32,), torch.int32).cpu().numpy()[17 * 32:17 * 32 + 1]
        if kind == "editnet":
            n = get("pro_count", (1,), torch.int32).cpu().numpy()
            out[cid + "|pro_count"] = n
            out[cid + "|pro_rows"] = get("pro_rows", (B * T,), torch.int32).cpu().numpy()[:max(int(n[0]), 0)]
        del ws
torch.cuda.synchronize()
np.savez(out_path, **out)
"""


@pytest.fixture(scope="module", autouse=True)
def _error_report():
    yield
    path = os.environ.get("PROLOGUE_STAGES_ERRORS_OUT")
    if not path or not RATIOS:
        return
    write_report(path, "[hip, float32 numpy oracle]: largest |stage output - float64 stage| / (tol * min(max|ref|, 1)) over the "
                 "token-table settings of a grid id, each stage on the device's own inputs to it; tol = parity.STATE_TOL", RATIOS)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """what each setting's child process left: one child per setting, one after another; a child that faults, aborts, is
    killed or times out fails the fixture, and no further child is started"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tmp = str(tmp_path_factory.mktemp("prologue_stages"))
    res = {}
    for setting, switches in G.SETTINGS.items():
        f = os.path.join(tmp, setting + ".npz")
        env = {k: v for k, v in os.environ.items() if k not in ("SET_ENC_PERSISTENT", "SET_ENC_PERSISTENT_MAXB")}
        env.update(switches)
        r = subprocess.run([sys.executable, "-c", _CHILD, f, setting], env=env, cwd=root, capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, "child %r exited with %d:\n%s" % (setting, r.returncode, r.stderr[-3000:])
        res[setting] = np.load(f)
    return res


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


_PARAMS = {}


def _params(setting, data, key):
    """(float64, float32) parameters the child of `setting` saved for a model"""
    if (setting, key) not in _PARAMS:
        _PARAMS.clear()
        pre = "W:%s|" % key
        sd = {k[len(pre):]: data[k] for k in data.files if k.startswith(pre)}
        assert sd, key
        _PARAMS[(setting, key)] = (EN.cast_params(sd, np.float64), EN.cast_params(sd))
    return _PARAMS[(setting, key)]


def _check_route(model, gid, r, e, prof):
    """the library's own launch record against the route the entry is there for -> reason to skip, or None"""
    T, dirs = e["T"], 2 if model == "dcnet" else 1
    refused = None
    if r["enc"] == "persistent":
        if "persistent_encoder" not in prof:
            refused = ("the library refused the persistent encoder launch (another process owns this device's persistent "
                       "launches, or the grid is not resident at once); the stages were judged on %s" % sorted(prof))
        else:
            assert prof["persistent_encoder"] == 1 and "fused_encoder_step" not in prof, prof
            return None
    else:
        assert "persistent_encoder" not in prof, prof
    if r["enc"] == "unfused":
        assert prof.get("encoder_pointwise") == dirs * T and "fused_encoder_step" not in prof, prof
    else:
        assert prof.get("fused_encoder_step") == dirs * T and "encoder_pointwise" not in prof, prof
    return refused


@pytest.mark.parametrize("case", G.cases(), ids=G.case_id)
def test_prologue_stages(runs, case):
    model, gid, table = case
    e, inp, r = G.entry(model, gid), G.inputs(model, gid), G.route(model, gid)
    dm, B, T, lens, seq = e["dims"], e["B"], e["T"], inp["lens"], inp["seq"]
    data = runs[e["setting"]]
    cid = G.case_id(case)
    dev = {k[len(cid) + 1:]: data[k] for k in data.files if k.startswith(cid + "|")}
    prof = json.loads(str(dev.pop("prof")))
    P, P32 = _params(e["setting"], data, G.model_key(model, dm))
    key = (model, gid)
    pad = np.arange(T)[None, :] >= lens[:, None]
    if model == "dcnet":
        ref = PO.dcnet_stages(P, seq, lens, dev, pc=r["pc"])
        o32 = PO.dcnet_stages(P32, seq, lens, dev, pc=r["pc"])
        recurrent, exact = ("enc",), ("mask",)
    elif model == "op":
        ref = dict(zip("HM", PO.encoder(P, seq, lens)), final_hidden=PO.final_hidden(P, dev["H"], lens), mask=PO.mask(P, dev["M"]))
        o32 = dict(zip("HM", PO.encoder(P32, seq, lens)), final_hidden=PO.final_hidden(P32, dev["H"], lens))
        recurrent, exact = ("H", "M"), ("mask",)
    else:
        kw = dict(adaptive=bool(dm["adaptive"]), pv=r["pv"], mean=inp["mean"])
        ref = PO.editnet_stages(P, seq, lens, inp["X"], dev, **kw)
        o32 = PO.editnet_stages(P32, seq, lens, inp["X"], dev, **kw)
        recurrent = ("H", "M")
        exact = ("mask",) + (("rmask", "image_mean") if dm["adaptive"] else ())
    assert set(ref) <= set(dev), sorted(set(ref) - set(dev))
    # ---- nothing is left unwritten
    for k in ref:
        assert dev[k].dtype == np.float32 and not np.isnan(dev[k]).any(), "%s: NaN left in %s" % (cid, k)
    # ---- every stage, every row
    for k, v in ref.items():
        what = "%s %s" % (cid, k)
        if k in exact:
            assert np.array_equal(dev[k], v.astype(np.float32)), what
        else:
            judge(RATIOS, key, ("encoder." + k) if k in recurrent else k, dev[k], v, parity.STATE_TOL, what, o32[k])
    # ---- exact checks
    valid32 = (~pad).astype(np.float32)
    assert np.array_equal(_bits(dev["mask"]), _bits(valid32)), cid + " mask is not exactly 1.0 / 0.0"
    for k in recurrent:
        assert not _bits(dev[k])[pad].any(), "%s: %s is not bit-zero behind a row's length" % (cid, k)
    if model != "op":
        bias = P32["caption_attention.cap_features_att.bias"]
        want = _bits(np.float32(0.0) + bias)
        assert np.array_equal(_bits(dev["att1_c"])[pad], np.broadcast_to(want, (int(pad.sum()), want.size))), cid + " att1_c padded rows"
        if "persistent_encoder" in prof:                  # (the launch clears the words; without one they are never written)
            assert int(dev["status"][0]) == 0, cid + ": a grid barrier of the persistent encoder timed out"
    if model == "editnet":
        assert not _bits(dev["cap_proj"])[pad].any(), cid + " cap_proj padded rows"
        assert not _bits(dev["mem_proj"])[pad].any(), cid + " mem_proj padded rows"
        rows = np.flatnonzero(~pad.reshape(-1))
        if r["rows"]:
            assert int(dev["pro_count"][0]) == rows.size and np.array_equal(dev["pro_rows"], rows), cid + " row list"
        else:
            assert int(dev["pro_count"][0]) == -1, cid + ": a row list was written"
    # ---- the kernel that ran
    refused = _check_route(model, gid, r, e, prof)
    if refused:
        pytest.skip(refused)
