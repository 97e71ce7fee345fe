"""GPU: the bf16-split grouped GEMM (csrc/gemm_split_bf16.inc) through set_gemm_nt_group_f32 inside set_gemm_nt_greedy_scope —
planned and launched as the greedy rollout's launches are — by default against SET_GEMM_SPLIT=0 (the fp32 kernels), each
setting in one child process (the switch is read once per process).

Exact pass (helpers of tests/test_hip_gemm_nt.py): operands are integers of [-8, 8].  Every bf16 plane of such a value is the
value itself or zero, every partial product and partial sum an integer below 2^24, so the split path — like the fp32 one —
must equal the int64 product BIT FOR BIT, into NaN-guarded outputs that are compared whole.  Rows 65, 127, 128, 129 (class
edge, 128-row tile edge), N = 64, 72, 200 (column tails), K of one k-tile and of three (two plus the loop's odd tail), slices
that end on a segment end and that cross one, 1 / 2 / 3 tasks, unsplit (bias epilogue) and split (slab epilogue).  64 rows with
the same arguments stay on the fp32 kernel (profile tag).

Rounding pass: normal floats against float64.  The split path's maximum error must be at most MARGIN times the fp32 path's on
the same inputs (the fp32 path is the reference: the kernels every other caller keeps).  MARGIN comes from the measured
ratios at these shapes (profiles/gemm_split_errors.json, 28 cases, five seeds): their mean is 0.89 — the split path is the
more accurate one on average — and single cases scatter from 0.62 to 1.43, because the maximum over 14 000 - 25 000 outputs
is a heavy-tailed statistic of either path.  MARGIN = 1.6 is that spread (worst / mean = 1.61) applied to parity.

Range: A scaled by 2^-100, 1 and 2^100 (exact scalings) must keep that bound relative to the scale.  One NaN, +inf or -inf
in A or W must give what the fp32 path gives in the affected outputs (NaN where it gives NaN, the same infinity where it gives
one) and leave the others as they are without it, bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SPLIT_TAG = "gemm_nt_f32<128,64>:bf16x3"
MARGIN = 1.6
ROWS = (65, 127, 128, 129)
NS = (64, 72, 200)
FLOAT_SHAPES = ((128, 192, 1024), (70, 200, 3072))     # (M, N, K): the K of the decode step's launches
SEEDS = (0, 1, 2, 3, 4)
SCALES = (-100, 0, 100)

_CHILD = r"""
import os, sys
import numpy as np, torch
sys.path.insert(0, os.path.join(os.getcwd(), "tests")); sys.path.insert(0, os.getcwd())
import test_hip_gemm_nt as T
import test_hip_gemm_split as S
from show_edit_tell_amd.autograd_ops import gemm_nt_group
from show_edit_tell_amd import _lib
out = {}


def exact(key, probs, **kw):
    # run() compares every canvas whole against the int64 product (raises on any difference)
    ks, cls, tags, _ = T.run(probs, key, greedy_scope=True, **kw)
    out["tags/" + key] = np.array(tags)
    out["ks/" + key] = np.array(ks)
    return ks


for M in S.ROWS + (64,):
    for N in S.NS:
        for Ks, splits in (((32,), (1,)), ((96,), (1, 2))):
            for ksplit in splits:
                p = T.Prob(T._rng(21, M, N, Ks[0], ksplit), M, N, Ks, ksplit=ksplit)
                exact("M%d_N%d_K%d_ks%d" % (M, N, Ks[0], ksplit), [p])
    # slices [0,2) [2,4): the first ends on the segment end; (96, 32) in two slices: the second crosses it; unsplit: crosses
    for Ks, ksplit in (((64, 64), 2), ((96, 32), 2), ((32, 64, 32), 1)):
        p = T.Prob(T._rng(22, M, len(Ks), ksplit), M, 72, Ks, ksplit=ksplit)
        assert T._straddles(Ks, ksplit) == (Ks != (64, 64))
        exact("M%d_seg%s_ks%d" % (M, "+".join(map(str, Ks)), ksplit), [p])
    for n in (2, 3):
        probs = [T.Prob(T._rng(23, M, n, 0), M, 200, (96,), ksplit=2), T.Prob(T._rng(23, M, n, 1), M, 64, (32, 64), ksplit=1),
                 T.Prob(T._rng(23, M, n, 2), M, 72, (64,), ksplit=1, act=T.ACT_RELU)][:n]
        for adjacent in (False, True):
            exact("M%d_tasks%d_adj%d" % (M, n, adjacent), probs, adjacent=adjacent, vec=not adjacent)
# loop gate: alive = 0 writes nothing (run(written=False) compares the untouched canvases), alive = 1 the exact result
one, zero = (torch.tensor([v], dtype=torch.int32, device=T.DEV) for v in (1, 0))
p = T.Prob(T._rng(24), 129, 200, (96, 32), ksplit=1)
exact("gate_alive1", [p], alive=one)
exact("gate_alive0", [p], alive=zero, written=False)


def product(a, w, ksplit, M, N):
    c = torch.full((M + 2, N + 8), float("nan"), device=T.DEV)
    gemm_nt_group([dict(segs=[(a, w)], C=c[1:M + 1, 4:4 + N], ksplit=ksplit)], greedy_scope=True)
    torch.cuda.synchronize()
    h = c.cpu().numpy()
    inside = h[1:M + 1, 4:4 + N].copy()
    h[1:M + 1, 4:4 + N] = np.nan
    assert np.isnan(h).all(), "stores outside C"
    return inside


for (M, N, K) in S.FLOAT_SHAPES:
    for seed in S.SEEDS:
        rng = np.random.default_rng([31, M, N, K, seed])
        a, w = rng.standard_normal((M, K)).astype(np.float32), rng.standard_normal((N, K)).astype(np.float32)
        ref = a.astype(np.float64) @ w.astype(np.float64).T
        wd = torch.from_numpy(w).to(T.DEV)
        for e in (S.SCALES if seed == 0 else (0,)):
            s = np.float32(2.0) ** e
            ad = torch.from_numpy(a * s).to(T.DEV)                     # exact scaling
            for ksplit in (1, 4):
                got = product(ad, wd, ksplit, M, N)
                again = product(ad, wd, ksplit, M, N)
                assert np.array_equal(got.view(np.uint32), again.view(np.uint32)), "two runs, two results"
                err = np.abs(got.astype(np.float64) * 2.0 ** -e - ref).max()
                out["err/M%d_N%d_K%d_seed%d_scale%d_ks%d" % (M, N, K, seed, e, ksplit)] = np.array([err])
# one special value in one operand element
M, N, K = 70, 72, 96
rng = np.random.default_rng([32])
a, w = rng.standard_normal((M, K)).astype(np.float32), rng.standard_normal((N, K)).astype(np.float32)
for ksplit in (1, 3):
    out["special/plain_ks%d" % ksplit] = product(torch.from_numpy(a).to(T.DEV), torch.from_numpy(w).to(T.DEV), ksplit, M, N)
    for vname, v in (("nan", np.nan), ("pinf", np.inf), ("ninf", -np.inf)):
        for op in ("A", "W"):
            a2, w2 = a.copy(), w.copy()
            (a2 if op == "A" else w2)[S.SPECIAL_AT] = v
            out["special/%s_%s_ks%d" % (vname, op, ksplit)] = product(torch.from_numpy(a2).to(T.DEV), torch.from_numpy(w2).to(T.DEV),
                                                                      ksplit, M, N)
np.savez(sys.argv[1], **out)
"""
SPECIAL_AT = (37, 41)            # (row of the operand, k): the second k-tile, so with three slices the middle slab carries it


@pytest.fixture(scope="module")
def ab(tmp_path_factory):
    return _children(str(tmp_path_factory.mktemp("gemm_split")))


def _children(tmp):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = {}
    for label, val in (("default", None), ("fp32", "0")):
        f = os.path.join(tmp, label + ".npz")
        env = {k: v for k, v in os.environ.items() if k != "SET_GEMM_SPLIT"}
        if val is not None:
            env["SET_GEMM_SPLIT"] = val
        r = subprocess.run([sys.executable, "-c", _CHILD, f], env=env, cwd=root, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (label, r.stdout[-2000:], r.stderr[-3000:])
        res[label] = dict(np.load(f))
    return res


def test_exact_cases_ran_on_the_expected_kernels(ab):
    """the children have already compared every output whole with the int64 product; here: who computed it"""
    keys = sorted(k for k in ab["default"] if k.startswith("tags/"))
    assert len(keys) == 82 and keys == sorted(k for k in ab["fp32"] if k.startswith("tags/"))
    for k in keys:
        rows64 = k.startswith("tags/M64_")
        new, old = list(ab["default"][k]), list(ab["fp32"][k])
        assert SPLIT_TAG not in old and len(old) == 1, (k, old)
        if rows64:
            assert new == old and new[0].startswith(("gemm_nt_f32_asm<64,64>", "gemm_nt_f32<64,64>")), (k, new)
        else:
            assert new == [SPLIT_TAG], (k, new)
        ks = k.replace("tags/", "ks/")
        assert np.array_equal(ab["default"][ks], ab["fp32"][ks]), ks          # the splits asked for were served by both


def test_error_against_float64_is_the_fp32_kernels(ab):
    rows = _error_rows(ab)
    assert len(rows) == len(FLOAT_SHAPES) * 2 * (len(SEEDS) + len(SCALES) - 1)
    for r in rows:
        print("%(case)s: split %(split)0.3e  fp32 %(fp32)0.3e  ratio %(ratio)0.3f" % r)
    print("worst ratio %.3f (MARGIN %.2f)" % (max(r["ratio"] for r in rows), MARGIN))
    bad = [r for r in rows if not r["split"] <= MARGIN * r["fp32"]]
    assert not bad, bad


def _error_rows(ab):
    rows = []
    for k in sorted(k for k in ab["default"] if k.startswith("err/")):
        e_split, e_fp32 = float(ab["default"][k][0]), float(ab["fp32"][k][0])
        rows.append(dict(case=k[4:], split=e_split, fp32=e_fp32, ratio=e_split / e_fp32))
    return rows


@pytest.mark.parametrize("ksplit", [1, 3])
@pytest.mark.parametrize("op", ["A", "W"])
@pytest.mark.parametrize("vname", ["nan", "pinf", "ninf"])
def test_special_values(ab, vname, op, ksplit):
    key = "special/%s_%s_ks%d" % (vname, op, ksplit)
    new, old, plain = ab["default"][key], ab["fp32"][key], ab["default"]["special/plain_ks%d" % ksplit]
    hit = np.zeros(new.shape, bool)
    if op == "A":
        hit[SPECIAL_AT[0], :] = True
    else:
        hit[:, SPECIAL_AT[0]] = True
    assert not np.isfinite(old[hit]).any()                                   # what the fp32 path gives there: inf or NaN
    assert np.array_equal(new[hit], old[hit], equal_nan=True), (key, new[hit][:8], old[hit][:8])
    assert np.array_equal(new[~hit].view(np.uint32), plain[~hit].view(np.uint32)), key


if __name__ == "__main__":       # python tests/test_hip_gemm_split.py OUT.json: the measured errors (profiles/gemm_split_errors.json)
    import json
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        rows = _error_rows(_children(tmp))
    doc = {"what": "max |C - float64 product| of set_gemm_nt_group_f32 (greedy scope), standard-normal operands: the bf16-split "
                   "kernel (default) against the fp32 kernels (SET_GEMM_SPLIT=0) on the same inputs; A scaled by 2^scale",
           "shapes_M_N_K": FLOAT_SHAPES, "seeds": SEEDS, "worst_ratio": max(r["ratio"] for r in rows),
           "best_ratio": min(r["ratio"] for r in rows), "margin_of_the_test": MARGIN, "cases": rows}
    with open(sys.argv[1], "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("worst ratio %.3f, best %.3f over %d cases" % (doc["worst_ratio"], doc["best_ratio"], len(rows)))
