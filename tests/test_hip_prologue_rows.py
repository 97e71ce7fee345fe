"""GPU: the decode prologue's hoisted caption projections contract the valid caption rows only (csrc/editnet.hip begin_impl,
csrc/gemm_f32.hip GATE = 2, csrc/gemm_fused.hip encoder_order_k<true>).

Rows of H / Mem beyond a caption's length are exactly zero, so the full products leave 0 + bias (att1_c) or +0 (cap_proj,
mem_proj) there.  With the row list the grouped launch covers the rows b*T + t, t < len[b], through a list that the encoder's
row-ranking launch writes on the device; the same launch stores the padded rows' values.  Tile shape and K order of every
computed element are those of the full launch, so everything must be BIT-identical to `SET_PRO_ROWLIST=0` (the full launch).
The switch is read once per process: one child process per setting serves every test (as tests/test_hip_dead_work.py does).

Cases (D = 128: the fused encoder step, whose row-ranking launch builds the list; A = 64, F = 128, R = 4, V = 64):
  b3    B = 3,  T = 5, lengths (1, 5, 3): 9 valid rows of 15.  15 rows run on the <= 16-row kernel class, which has no row
        tiles to skip: this launch stays full under both settings and the case pins that boundary
  b13   B = 13, T = 5, every length 5: 65 valid rows, no padding; one entry past a 64-row tile (clamped tail of the last tile)
  b16   B = 16, T = 8, every length 4: exactly 64 valid rows, the list ends on a tile boundary and the second tile exits
  b70   B = 70, T = 7, lengths cycling 1..7: 280 valid rows of 490, several tiles, the last live one partly filled
Before each prologue the three outputs are filled with NaN, so a padded row that nobody wrote would show.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CASES = {"b3": (3, 5, (1, 5, 3)), "b13": (13, 5, (5,) * 13), "b16": (16, 8, (4,) * 16),
         "b70": (70, 7, tuple(1 + i % 7 for i in range(70)))}
COUNT_CASE = "b70"
MAX_LEN = 6

_CHILD = r"""
import ctypes as C, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.join(os.getcwd(), "tests")); sys.path.insert(0, os.getcwd())
from oracle import cases
from hip_adapter import editnet_modules, to_dev
from show_edit_tell_amd import _lib
os.environ["SET_TOKEN_TABLE"] = "1"
CASES = eval(sys.argv[2])
out = {}
lib = _lib.load()
with torch.no_grad():
    for name, (B, T, lens) in CASES.items():
        cname = "prorows_" + name
        cases.DP_CASES[cname] = dict(D=128, A=64, F=128, V=64, R=4, T=T, B=B, wseed=11, iseed=70 + B, ragged_caps=True,
                                     **cases.SCALES)
        d, xe, rl = editnet_modules(cname)
        plen = np.asarray(lens, dtype=np.int64).reshape(B, 1)
        prev = (np.where(d["prev"] > 0, d["prev"], 1) * (np.arange(T)[None, :] < plen)).astype(np.int64)
        rl.max_len = int(sys.argv[3])
        X, prev_d, plen_d = to_dev(d["X"]), to_dev(prev), to_dev(plen)
        seq, lp = rl(d["wm"], prev_d, plen_d, X, True, False)
        out[name + "/seq"] = seq.cpu().numpy()
        out[name + "/seq_logp"] = lp.cpu().numpy()
        if name == sys.argv[4]:                       # launch counts of one greedy decode
            torch.cuda.synchronize()
            lib.set_profile_enable(1)
            rl(d["wm"], prev_d, plen_d, X, True, False)
            torch.cuda.synchronize()
            prof = _lib.profile_report()
            lib.set_profile_enable(0)
            out["count"] = np.array([sum(p["launches"] for p in prof if p["tag"].startswith(("gemm_nt_f32", "gemv_nt_f32")))])
        # the prologue alone, its outputs poisoned first
        dims = rl._dims(B, T, 4, rl.max_len + 1)
        ws = rl._workspace(dims)
        w = rl._weights(dims)
        assert w.tok_table
        shapes = {"att1_c": (B, T, 64), "cap_proj": (B, T, 256), "mem_proj": (B, T, 128), "H": (B, T, 128), "M": (B, T, 128),
                  "final_hidden": (B, 128), "mask": (B, T)}
        for k in ("att1_c", "cap_proj", "mem_proj"):
            rl.ws_tensor(dims, k, shapes[k]).fill_(float("nan"))
        rl.ws_tensor(dims, "pro_count", (1,), torch.int32).fill_(-1)
        plen_flat = plen_d.reshape(-1).contiguous()
        _lib.check(lib.set_editnet_begin(C.byref(w), C.byref(dims), _lib.ptr(X), None, _lib.ptr(prev_d), _lib.ptr(plen_flat),
                                         _lib.ptr(ws), ws.numel(), _lib.stream_of(X.device)), "begin")
        torch.cuda.synchronize()
        for k, shp in shapes.items():
            out[name + "/" + k] = rl.ws_tensor(dims, k, shp).cpu().numpy()
        out[name + "/pro_count"] = rl.ws_tensor(dims, "pro_count", (1,), torch.int32).cpu().numpy()
        n = max(int(out[name + "/pro_count"][0]), 0)
        out[name + "/pro_rows"] = rl.ws_tensor(dims, "pro_rows", (B * T,), torch.int32).cpu().numpy()[:n]
        out[name + "/ca_feat_b"] = d["sd"]["caption_attention.cap_features_att.bias"]
torch.cuda.synchronize()
np.savez(sys.argv[1], **out)
"""


@pytest.fixture(scope="module")
def ab(tmp_path_factory):
    """everything the prologue and the greedy decode leave, with the row list ("new") and with the full launch ("old")"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tmp = str(tmp_path_factory.mktemp("prologue_rows"))
    res = {}
    for label, val in (("new", "1"), ("old", "0")):
        f = os.path.join(tmp, label + ".npz")
        env = dict(os.environ, SET_PRO_ROWLIST=val)
        r = subprocess.run([sys.executable, "-c", _CHILD, f, repr(CASES), str(MAX_LEN), COUNT_CASE], env=env, cwd=root,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        res[label] = dict(np.load(f))
    return res


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("name", sorted(CASES))
def test_row_list_changes_no_output(ab, name):
    """seq, seq_logp of the greedy decode (token table active) and att1_c, cap_proj, mem_proj (+ the encoder's outputs) after
    set_editnet_begin are the same bits with the row list as with the full launch."""
    new, old = ab["new"], ab["old"]
    for k in ("seq", "seq_logp", "att1_c", "cap_proj", "mem_proj", "H", "M", "final_hidden", "mask"):
        a, b = new[name + "/" + k], old[name + "/" + k]
        assert a.shape == b.shape and a.dtype == b.dtype, k
        if a.dtype == np.float32:
            assert np.array_equal(_bits(a), _bits(b)), k
        else:
            assert np.array_equal(a, b), k
    assert not np.isnan(new[name + "/seq_logp"]).any()


@pytest.mark.parametrize("name", sorted(CASES))
def test_padded_rows_and_list(ab, name):
    """Padded rows hold what the full products leave there — att1_c the bias bit for bit, cap_proj / mem_proj +0 (sign bit
    clear) — under both settings; where the list is in use (more than 16 rows) it is the valid rows in row-major order."""
    B, T, lens = CASES[name]
    pad = np.arange(T)[None, :] >= np.asarray(lens)[:, None]
    for label in ("new", "old"):
        r = ab[label]
        bias = r[name + "/ca_feat_b"].astype(np.float32)
        want = _bits(np.float32(0.0) + bias)
        assert np.array_equal(_bits(r[name + "/att1_c"])[pad], np.broadcast_to(want, (int(pad.sum()), want.size))), label
        assert not _bits(r[name + "/cap_proj"])[pad].any(), label
        assert not _bits(r[name + "/mem_proj"])[pad].any(), label
        for k in ("att1_c", "cap_proj", "mem_proj"):
            assert not np.isnan(r[name + "/" + k]).any(), (label, k)
    valid = np.flatnonzero(~pad.reshape(-1))
    if B * T > 16:
        assert int(ab["new"][name + "/pro_count"][0]) == valid.size
        assert np.array_equal(ab["new"][name + "/pro_rows"], valid)
    else:
        assert int(ab["new"][name + "/pro_count"][0]) == -1          # the <= 16-row class keeps the full launch
    assert int(ab["old"][name + "/pro_count"][0]) == -1


def test_launch_counts(ab):
    """The list adds no launch: the same number of grouped-GEMM launches per greedy decode with it as without (the library's
    own profile; prologue 5 + 3 per timestep, tests/test_hip_dead_work.py)."""
    new, old = int(ab["new"]["count"][0]), int(ab["old"]["count"][0])
    print("GEMM launches per decode: %d with the row list, %d without" % (new, old))
    assert new == old == 5 + 3 * MAX_LEN
