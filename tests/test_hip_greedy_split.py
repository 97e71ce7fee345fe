"""The no-grad greedy rollout of EditNet runs its grouped GEMM launches of 65+ rows on the bf16-split kernel
(csrc/gemm_split_bf16.inc; csrc/editnet.hip rollout() opens the SplitScope, csrc/gemm_f32.hip decides per launch).  Whole
decodes with the default against SET_GEMM_SPLIT=0 (the fp32 kernels for every launch), each setting in its own child process
(the switch is read once per process).

Model: the small one of tests/test_hip_prologue_rows.py (D = 128, A = 64, F = 128, R = 4, V = 64), token table on.
Cases: 64 rows (below the class: no launch may change), 65 (one row in the second half of the 128-row tile), 70, 128 (the tile
exactly), each at max_len 1 (prologue + one timestep: the lone last fc) and 6 (merged F/A launches in between); `r70_end`
boosts <end> so that every row finishes early and the loop gate returns the later timesteps' launches at once.

What is asserted on the GPU: equal seq, seq_logp within 1e-4 (the project's logit target), the split kernel's profile tag
present at 65+ rows and absent at 64, absent from a sampled rollout and from a teacher-forced forward of the same model.
The split product is not the fp32 chain bit for bit, so a pick between two near-equal logits could legitimately differ: the
seeds below are chosen so that the float64 oracle's top-two logit gap is at least 1e-3 at every pick, which the CPU test of
this file asserts on the oracle alone.  No GPU assertion rests on an "either" pick."""
import os
import subprocess
import sys

import numpy as np
import pytest

SPLIT_TAG = "gemm_nt_f32<128,64>:bf16x3"
MIN_GAP = 1e-3
T = 5
# name -> (rows, max_len, input seed, end boost)
CASES = {
    "r64_l1": (64, 1, 301, 0.0), "r64_l6": (64, 6, 301, 0.0),
    "r65_l1": (65, 1, 301, 0.0), "r65_l6": (65, 6, 301, 0.0),
    "r70_l1": (70, 1, 301, 0.0), "r70_l6": (70, 6, 301, 0.0),
    "r128_l1": (128, 1, 301, 0.0), "r128_l6": (128, 6, 301, 0.0),
    "r70_end": (70, 6, 320, 3.5),       # 3, 2, 2 rows alive after picks 0, 1, 2; none after pick 3
}
OTHER_ROUTES_CASE = "r70_l6"          # the sampled rollout and the teacher-forced forward are profiled on this one


def register(name):
    """the case as oracle.cases knows it -> its key there"""
    from oracle import cases
    B, _, iseed, boost = CASES[name]
    key = "greedy_split_" + name
    c = dict(D=128, A=64, F=128, V=64, R=4, T=T, B=B, wseed=11, iseed=iseed, ragged_caps=True, **cases.SCALES)
    if boost:
        c["end_boost"] = boost
    cases.DP_CASES[key] = c
    return key


def oracle_decode(name):
    """float64 oracle -> (seq, smallest top-two logit gap over every pick that was made)"""
    from oracle import cases, editnet_np as EN
    d = cases.build_editnet(register(name))
    wm, max_len = d["wm"], CASES[name][1]
    trace = []
    P = EN.cast_params(d["sd"], np.float64)
    seq, _ = EN.greedy_decode(P, wm["<start>"], wm["<end>"], d["prev"], d["plen"], d["X"].astype(np.float64), max_len=max_len,
                              trace=trace)
    gap = np.inf
    for step in trace[:max_len]:                       # (the step after the last pick is discarded)
        top = np.sort(step["logits"], axis=1)[:, -2:]
        gap = min(gap, float((top[:, 1] - top[:, 0]).min()))
    return seq, gap


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_top_two_gap(name):
    """CPU: at every pick of every row the float64 oracle's two largest logits are at least 1e-3 apart — ten times the 1e-4
    the two GEMM kernels may differ by — so the greedy tokens of the cases above do not depend on the kernel."""
    seq, gap = oracle_decode(name)
    print("%s: smallest top-two gap %.3e" % (name, gap))
    assert gap >= MIN_GAP, (name, gap)
    if name == "r70_end":                              # every row has finished two timesteps before the last one
        assert not seq[:, 3:].any() and seq[:, 0].any(), seq[:4]


_CHILD = r"""
import os, sys
import numpy as np, torch
sys.path.insert(0, os.path.join(os.getcwd(), "tests")); sys.path.insert(0, os.getcwd())
os.environ["SET_TOKEN_TABLE"] = "1"
import test_hip_greedy_split as G
from hip_adapter import editnet_modules, to_dev
from show_edit_tell_amd import _lib
lib = _lib.load()
out = {}


def profiled(fn):
    torch.cuda.synchronize()
    lib.set_profile_enable(1)
    try:
        r = fn()
        torch.cuda.synchronize()
        tags = sorted(e["tag"] for e in _lib.profile_report() if e["tag"].startswith(("gemm_nt", "gemv_nt")))
    finally:
        lib.set_profile_enable(0)
    return r, tags


with torch.no_grad():
    for name in sorted(G.CASES):
        d, xe, rl = editnet_modules(G.register(name))
        rl.max_len = G.CASES[name][1]
        args = (d["wm"], to_dev(d["prev"]), to_dev(d["plen"]), to_dev(d["X"]))
        rl(*args, True, False)                                         # (the token table is built here)
        (seq, lp), tags = profiled(lambda: rl(*args, True, False))
        out[name + "/seq"], out[name + "/seq_logp"] = seq.cpu().numpy(), lp.cpu().numpy()
        out[name + "/tags"] = np.array(tags)
        seq2, lp2 = rl(*args, True, False)
        out[name + "/same_bits_twice"] = np.array([torch.equal(seq, seq2) and torch.equal(lp.view(torch.int32), lp2.view(torch.int32))])
        if name == G.OTHER_ROUTES_CASE:
            torch.manual_seed(5)
            _, tags_s = profiled(lambda: rl(*args, False, True))
            out["sampled/tags"] = np.array(tags_s)
            _, tags_x = profiled(lambda: xe(to_dev(d["X"]), to_dev(d["caps"]), to_dev(d["clen"]), to_dev(d["prev"]),
                                            to_dev(d["plen"]), False, 0.0))
            out["teacher_forced/tags"] = np.array(tags_x)
np.savez(sys.argv[1], **out)
"""


@pytest.fixture(scope="module")
def ab(tmp_path_factory):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tmp = str(tmp_path_factory.mktemp("greedy_split"))
    res = {}
    for label, val in (("default", None), ("fp32", "0")):
        f = os.path.join(tmp, label + ".npz")
        env = {k: v for k, v in os.environ.items() if k != "SET_GEMM_SPLIT"}
        if val is not None:
            env["SET_GEMM_SPLIT"] = val
        r = subprocess.run([sys.executable, "-c", _CHILD, f], env=env, cwd=root, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        res[label] = dict(np.load(f))
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_greedy_default_against_fp32(ab, name):
    rows = CASES[name][0]
    new, old = ab["default"], ab["fp32"]
    assert np.array_equal(new[name + "/seq"], old[name + "/seq"]), name
    err = float(np.abs(new[name + "/seq_logp"].astype(np.float64) - old[name + "/seq_logp"]).max())
    print("%s: max |seq_logp(default) - seq_logp(fp32 kernels)| = %.3e" % (name, err))
    assert not np.isnan(new[name + "/seq_logp"]).any()
    assert err <= 1e-4, (name, err)
    assert (SPLIT_TAG in new[name + "/tags"]) == (rows >= 65), (name, new[name + "/tags"])
    assert SPLIT_TAG not in old[name + "/tags"], (name, old[name + "/tags"])
    assert new[name + "/same_bits_twice"][0] and old[name + "/same_bits_twice"][0]
    if rows < 65:                                      # below the class nothing changes at all
        assert np.array_equal(new[name + "/seq_logp"].view(np.uint32), old[name + "/seq_logp"].view(np.uint32))


@pytest.mark.gpu
def test_greedy_agrees_with_the_oracle(ab):
    """the tokens both settings agree on are the float64 oracle's (whose picks are 1e-3 clear of a tie)"""
    for name in sorted(CASES):
        seq, _ = oracle_decode(name)
        assert np.array_equal(ab["default"][name + "/seq"], seq), name


@pytest.mark.gpu
def test_loop_gate_case_finishes_early(ab):
    """r70_end: every row has finished after three picks; the later timesteps' launches return at once (loop gate) and leave
    zeros in seq and seq_logp, under the split kernel as under the fp32 kernels"""
    for label in ("default", "fp32"):
        seq, lp = ab[label]["r70_end/seq"], ab[label]["r70_end/seq_logp"]
        assert not seq[:, 3:].any(), label
        assert not lp[:, 4:].any(), label
    assert SPLIT_TAG in ab["default"]["r70_end/tags"]


@pytest.mark.gpu
def test_other_routes_keep_the_fp32_kernels(ab):
    for route in ("sampled", "teacher_forced"):
        tags = ab["default"][route + "/tags"]
        assert len(tags) and SPLIT_TAG not in tags, (route, tags)
