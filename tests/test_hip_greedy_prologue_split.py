"""GPU: the greedy decode of 65+ rows runs its PROLOGUE's grouped GEMM launches on the bf16-split kernel as well
(csrc/editnet.hip rollout() opens the SplitScope around begin_impl; the hoisted caption projections keep their row list,
csrc/gemm_split_bf16.inc gemm_nt_split_bf16<2>), and set_editnet_begin_greedy is that prologue for a workspace prepared ahead.
Whole decodes and prologues under four settings, each in one child process (the switches are read once per process):
  default     nothing set
  pro0        SET_PRO_SPLIT=0: the scope opens after the prologue (the behaviour before this change)
  fp32        SET_GEMM_SPLIT=0: the fp32 kernels everywhere
  rowlist0    SET_PRO_ROWLIST=0: the caption projections as full launches

Model: the small one of tests/test_hip_prologue_rows.py (D = 128, A = 64, F = 128, R = 4, V = 64, T = 5, ragged previous
captions: lengths 1..5), token table on.  Batches of 64 rows (below the class), 65, 70, 128 (the tile exactly) and 490 (several
tiles in every prologue product, pre1 included), each at max_len 1 and 6.  The split product is not the fp32 chain bit for bit,
so a pick between two near-equal logits could differ: the input seeds are chosen so that the float64 oracle's top-two logit
gap is at least 1e-3 at every pick (5e-4 for r490_l6, see MIN_GAPS; the CPU test below asserts it on the oracle alone), ten
(five) times the 1e-4 the kernels may differ by.

A prologue's grouped launches are five: the encoder's final affine (caption encoder: fp32 in every scope) and the four
products `cap projections`, `att_embed`, `features_att`, `pre1`.

`pro0` against the parent commit is bit-equal by construction (the same scope at the same place); this file has no second
build to check it against, the benchmark's output dump compares the two builds (profiles/prologue_split_bench.json)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import test_hip_greedy_split as G

SPLIT_TAG = G.SPLIT_TAG
MIN_GAP = G.MIN_GAP
# name -> (rows, max_len, input seed)
CASES = {
    "r64_l1": (64, 1, 301), "r64_l6": (64, 6, 301), "r65_l1": (65, 1, 301), "r65_l6": (65, 6, 301),
    "r70_l1": (70, 1, 301), "r70_l6": (70, 6, 301), "r128_l1": (128, 1, 301), "r128_l6": (128, 6, 301),
    "r490_l1": (490, 1, 302), "r490_l6": (490, 6, 320),
}
# 2940 picks: no seed of 700 tried reaches 1e-3 there.  Two computations that are each within 1e-4 of the exact logits can order
# the top two differently only below a gap of 2e-4; 5e-4 keeps two and a half times that.
MIN_GAPS = {"r490_l6": 5e-4}
BEGIN_CASES = ("r64_l6", "r65_l6", "r70_l6", "r128_l6")      # the prologue entries alone, and begin_greedy + greedy_begun
OTHER_ROUTES_CASE = "r70_l6"
SETTINGS = {"default": {}, "pro0": {"SET_PRO_SPLIT": "0"}, "fp32": {"SET_GEMM_SPLIT": "0"}, "rowlist0": {"SET_PRO_ROWLIST": "0"}}
D, A, R = 128, 64, 4
# what a prologue leaves: name -> shape for (B, T); the first four are the caption encoder's, the others the four products'
INTERMEDIATES = {"H": lambda B, T: (B, T, D), "M": lambda B, T: (B, T, D), "final_hidden": lambda B, T: (B, D),
                 "mask": lambda B, T: (B, T), "att1_c": lambda B, T: (B, T, A), "cap_proj": lambda B, T: (B, T, 2 * D),
                 "mem_proj": lambda B, T: (B, T, D), "fe": lambda B, T: (B, R, D), "att1": lambda B, T: (B, R, A),
                 "pre1": lambda B, T: (B, 4 * D)}
PRODUCTS = ("att1_c", "cap_proj", "mem_proj", "fe", "att1", "pre1")


def register(name):
    """the case as oracle.cases knows it (the model and inputs tests/test_hip_greedy_split.py builds for the same seed) -> its key
    there.  Nothing of that module is changed: its own tests walk its CASES."""
    from oracle import cases
    B, _, iseed = CASES[name]
    key = "greedy_prologue_split_" + name
    cases.DP_CASES[key] = dict(D=D, A=A, F=128, V=64, R=R, T=G.T, B=B, wseed=11, iseed=iseed, ragged_caps=True, **cases.SCALES)
    return key


def oracle_decode(name):
    """float64 oracle -> (seq, smallest top-two logit gap over every pick that was made)"""
    from oracle import cases, editnet_np as EN
    d = cases.build_editnet(register(name))
    wm, max_len = d["wm"], CASES[name][1]
    trace = []
    seq, _ = EN.greedy_decode(EN.cast_params(d["sd"], np.float64), wm["<start>"], wm["<end>"], d["prev"], d["plen"],
                              d["X"].astype(np.float64), max_len=max_len, trace=trace)
    gap = np.inf
    for step in trace[:max_len]:                       # (the step after the last pick is discarded)
        top = np.sort(step["logits"], axis=1)[:, -2:]
        gap = min(gap, float((top[:, 1] - top[:, 0]).min()))
    return seq, gap


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_top_two_gap(name):
    """CPU: the greedy tokens of these cases do not depend on the kernel (see the top)."""
    _, gap = oracle_decode(name)
    print("%s: smallest top-two gap %.3e" % (name, gap))
    assert gap >= MIN_GAPS.get(name, MIN_GAP), (name, gap)


_CHILD = r"""
import ctypes as C, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.join(os.getcwd(), "tests")); sys.path.insert(0, os.getcwd())
os.environ["SET_TOKEN_TABLE"] = "1"
import test_hip_greedy_prologue_split as P
from hip_adapter import editnet_modules, to_dev
from show_edit_tell_amd import _lib
lib = _lib.load()
out = {}
GEMM = ("gemm_nt", "gemv_nt")


def profiled(fn):
    # -> (result, grouped-GEMM launches on the split kernel, on every other kernel)
    torch.cuda.synchronize()
    lib.set_profile_enable(1)
    try:
        r = fn()
        torch.cuda.synchronize()
        prof = [e for e in _lib.profile_report() if e["tag"].startswith(GEMM)]
    finally:
        lib.set_profile_enable(0)
    split = sum(e["launches"] for e in prof if e["tag"] == P.SPLIT_TAG)
    return r, np.array([split, sum(e["launches"] for e in prof) - split])


def bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


with torch.no_grad():
    for name in sorted(P.CASES):
        B, max_len, _ = P.CASES[name]
        d, xe, rl = editnet_modules(P.register(name))
        rl.max_len = max_len
        T = d["prev"].shape[1]
        X, prev, plen = to_dev(d["X"]), to_dev(d["prev"]), to_dev(d["plen"])
        args = (d["wm"], prev, plen, X)
        rl(*args, True, False)                                         # (the token table is built here)
        (seq, lp), n = profiled(lambda: rl(*args, True, False))
        out[name + "/seq"], out[name + "/seq_logp"], out[name + "/launches"] = seq.cpu().numpy(), lp.cpu().numpy(), n
        out[name + "/valid_rows"] = np.array([int(d["plen"].sum())])
        if name == P.OTHER_ROUTES_CASE:
            torch.manual_seed(5)
            _, out["sampled/launches"] = profiled(lambda: rl(*args, False, True))
            _, out["teacher_forced/launches"] = profiled(lambda: xe(X, to_dev(d["caps"]), to_dev(d["clen"]), prev, plen, False, 0.0))
        if name not in P.BEGIN_CASES:
            continue
        dims = rl._dims(B, T, 4, max_len + 1)
        ws, w = rl._workspace(dims), rl._weights(dims)
        assert w.tok_table
        plen_flat = plen.reshape(-1).contiguous()
        shape = lambda s: s(B, T)
        for entry in ("set_editnet_begin", "set_editnet_begin_greedy"):
            for k in P.PRODUCTS:                                         # poisoned first: a row nobody wrote would show
                rl.ws_tensor(dims, k, shape(P.INTERMEDIATES[k])).fill_(float("nan"))
            rl.ws_tensor(dims, "pro_count", (1,), torch.int32).fill_(-1)
            call = lambda: _lib.check(getattr(lib, entry)(C.byref(w), C.byref(dims), _lib.ptr(X), None, _lib.ptr(prev), _lib.ptr(plen_flat),
                                                           _lib.ptr(ws), ws.numel(), _lib.stream_of(X.device)), entry)
            _, out[name + "/" + entry + "/launches"] = profiled(call)
            for k, s in P.INTERMEDIATES.items():
                out[name + "/" + entry + "/" + k] = rl.ws_tensor(dims, k, shape(s)).cpu().numpy()
            out[name + "/" + entry + "/pro_count"] = rl.ws_tensor(dims, "pro_count", (1,), torch.int32).cpu().numpy()
        # the workspace now holds set_editnet_begin_greedy's prologue: the loop alone on it
        seq2 = torch.empty_like(seq); lp2 = torch.empty_like(lp)
        _lib.check(lib.set_editnet_greedy_begun(C.byref(w), C.byref(dims), _lib.ptr(X), int(d["wm"]["<start>"]), int(d["wm"]["<end>"]),
                                                max_len, _lib.ptr(seq2), _lib.ptr(lp2), _lib.ptr(ws), ws.numel(),
                                                _lib.stream_of(X.device)), "set_editnet_greedy_begun")
        torch.cuda.synchronize()
        out[name + "/begun_same_bits"] = np.array([torch.equal(seq, seq2) and bits(lp, lp2)])
np.savez(sys.argv[1], **out)
"""


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tmp = str(tmp_path_factory.mktemp("greedy_prologue_split"))
    res = {}
    for label, extra in SETTINGS.items():
        f = os.path.join(tmp, label + ".npz")
        env = {k: v for k, v in os.environ.items() if k not in ("SET_GEMM_SPLIT", "SET_PRO_SPLIT", "SET_PRO_ROWLIST")}
        env.update(extra)
        r = subprocess.run([sys.executable, "-c", _CHILD, f], env=env, cwd=root, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (label, r.stderr[-3000:])
        res[label] = dict(np.load(f))
    return res


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_default_against_prologue_on_fp32(runs, name):
    """default against SET_PRO_SPLIT=0: the same tokens, seq_logp within the project's 1e-4; from 65 rows on exactly the four
    prologue products moved to the split kernel, at 64 rows nothing moved and nothing changed"""
    rows = CASES[name][0]
    new, old, fp32 = runs["default"], runs["pro0"], runs["fp32"]
    assert np.array_equal(new[name + "/seq"], old[name + "/seq"]), name
    err = float(np.abs(new[name + "/seq_logp"].astype(np.float64) - old[name + "/seq_logp"]).max())
    print("%s: max |seq_logp(default) - seq_logp(SET_PRO_SPLIT=0)| = %.3e" % (name, err))
    assert not np.isnan(new[name + "/seq_logp"]).any()
    assert err <= 1e-4, (name, err)
    n_new, n_old, n_fp32 = (list(r[name + "/launches"]) for r in (new, old, fp32))
    assert sum(n_new) == sum(n_old) == sum(n_fp32) and n_fp32[0] == 0, (n_new, n_old, n_fp32)
    if rows < 65:
        assert n_new == n_old == n_fp32, (name, n_new, n_old, n_fp32)
        for r in (old, fp32):
            assert np.array_equal(_bits(new[name + "/seq_logp"]), _bits(r[name + "/seq_logp"])), name
    else:
        assert n_new[0] - n_old[0] == 4, (name, n_new, n_old)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_default_agrees_with_the_oracle(runs, name):
    seq, _ = oracle_decode(name)
    assert np.array_equal(runs["default"][name + "/seq"], seq), name


@pytest.mark.gpu
def test_other_routes_keep_the_fp32_kernels(runs):
    for route in ("sampled", "teacher_forced"):
        n = list(runs["default"][route + "/launches"])
        assert n[0] == 0 and n[1] > 0, (route, n)


@pytest.mark.gpu
@pytest.mark.parametrize("name", BEGIN_CASES)
def test_begin_stays_fp32(runs, name):
    """set_editnet_begin: no launch on the split kernel, every intermediate the bits of SET_GEMM_SPLIT=0"""
    new, fp32 = runs["default"], runs["fp32"]
    n = list(new[name + "/set_editnet_begin/launches"])
    assert n == [0, 5], n
    for k in INTERMEDIATES:
        a, b = new[name + "/set_editnet_begin/" + k], fp32[name + "/set_editnet_begin/" + k]
        assert not np.isnan(a).any(), k
        assert np.array_equal(_bits(a), _bits(b)), (name, k)


@pytest.mark.gpu
@pytest.mark.parametrize("name", BEGIN_CASES)
def test_begin_greedy_is_the_greedy_decodes_prologue(runs, name):
    """set_editnet_begin_greedy: the four products on the split kernel from 65 rows on (none at 64, where it is
    set_editnet_begin bit for bit); the row list was built inside the scope (pro_count = the valid caption rows; -1 under
    SET_PRO_ROWLIST=0); set_editnet_greedy_begun on its workspace gives the bits of set_editnet_greedy under every setting"""
    rows = CASES[name][0]
    new = runs["default"]
    n = list(new[name + "/set_editnet_begin_greedy/launches"])
    assert n == ([4, 1] if rows >= 65 else [0, 5]), (name, n)
    assert int(new[name + "/set_editnet_begin_greedy/pro_count"][0]) == int(new[name + "/valid_rows"][0])
    assert int(runs["rowlist0"][name + "/set_editnet_begin_greedy/pro_count"][0]) == -1
    for k in INTERMEDIATES:
        a, b = new[name + "/set_editnet_begin_greedy/" + k], new[name + "/set_editnet_begin/" + k]
        assert not np.isnan(a).any(), k
        if rows < 65:
            assert np.array_equal(_bits(a), _bits(b)), (name, k)
        else:
            err = float(np.abs(a.astype(np.float64) - b).max())
            assert err <= 1e-4, (name, k, err)
    for label in SETTINGS:
        assert runs[label][name + "/begun_same_bits"][0], (name, label)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in sorted(CASES) if CASES[n][0] in (65, 128, 490)])
def test_row_list_changes_no_bit(runs, name):
    """default against SET_PRO_ROWLIST=0: the caption projections on the split kernel with the list and as full launches"""
    new, old = runs["default"], runs["rowlist0"]
    assert list(new[name + "/launches"]) == list(old[name + "/launches"])
    assert np.array_equal(new[name + "/seq"], old[name + "/seq"]), name
    assert np.array_equal(_bits(new[name + "/seq_logp"]), _bits(old[name + "/seq_logp"])), name
    if name in BEGIN_CASES:
        for k in INTERMEDIATES:
            assert np.array_equal(_bits(new[name + "/set_editnet_begin_greedy/" + k]),
                                  _bits(old[name + "/set_editnet_begin_greedy/" + k])), (name, k)
