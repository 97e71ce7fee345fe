"""GPU: the compacted row list on the bf16-split grouped GEMM (csrc/gemm_split_bf16.inc gemm_nt_split_bf16<2>), through
set_gemm_nt_group_f32 inside set_gemm_nt_greedy_scope with a row list, as the greedy decode's prologue launches its hoisted
caption projections.  One child process with SET_GEMM_SPLIT unset (the switch is read once per process) runs every launch and
records, per case, the kernel tags and what went wrong (nothing, when the case holds); the tests below read that record.

Exact pass (helpers of tests/test_hip_gemm_nt.py).  Operands are integers of [-8, 8], K <= 288 <= 1024: every bf16 plane of
such a value is the value itself or zero and every partial sum an integer below 2^24, so the listed rows must equal the int64
product BIT FOR BIT.  C lies in a canvas of NaN sentinels with guard rows and is compared whole: rows the list does not name,
and the guards, keep their sentinel.  M = 300 (three 128-row tiles, the last with 44 rows); list counts 0, 1, 127, 128, 129,
257, 300 (nothing; one row; either side of one tile; one row into the third tile; everything); lists in order, permuted and
with repeats; two tasks (N = 64 bias + ReLU, N = 65 no bias) and four tasks (N = 200 bias, 64 bias + ReLU, 65, 200 ReLU without
bias, K segments (64), (32, 64), (288), (96)) sharing one list, as the prologue's `cap projections` launch does.

Clamp pass.  List entries -1 and M act as rows 0 and M - 1 (A and C inside NaN guards, the list inside zeros); counts -1 and
M + 5 act as 0 and M.

Rounding pass.  Standard-normal operands, (M, N, K) = (300, 200, 1024): the listed rows of the list launch equal the same rows
of the full split launch bit for bit; their error against the float64 product stays within the ratio bound of
profiles/gemm_split_errors.json (margin_of_the_test, 1.6) of the fp32 128x64 kernel's, measured in the same run on the same
list.

Tag and refusals.  Every list launch above ran on the split kernel's tag.  A list on a split-K problem and a list together
with the loop gate answer SET_ERR_ARG inside the scope as outside; 16 rows (the class without row tiles) SET_ERR_UNSUPPORTED."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SPLIT_TAG = "gemm_nt_f32<128,64>:bf16x3"
FP32_TAG = "gemm_nt_f32<128,64>"
M = 300
COUNTS = (0, 1, 127, 128, 129, 257, 300)
LISTS = ("ordered", "permuted", "repeats")
TASKS = (2, 4)
CLAMP_COUNTS = (-1, M + 5)
ROUND_SHAPE = (300, 200, 1024)
ROUND_COUNT = 257
ROUND_SEEDS = (0, 1)

_CHILD = r"""
import os, sys
import numpy as np, torch
sys.path.insert(0, os.path.join(os.getcwd(), "tests")); sys.path.insert(0, os.getcwd())
import test_hip_gemm_nt as T
import test_hip_split_rowlist as R
from show_edit_tell_amd.autograd_ops import gemm_nt_group
out = {}
M = R.M


def dev_list(lst):
    # the list inside a larger int tensor of zeros
    h = np.zeros(len(lst) + 32, np.int32)
    h[16:16 + len(lst)] = lst
    return torch.from_numpy(h).to(T.DEV)[16:16 + len(lst)]


def probs_of(rng, n):
    p = [T.Prob(rng, M, 64, (64,), act=T.ACT_RELU, a_guard=T.G), T.Prob(rng, M, 65, (32, 64), bias=False, a_guard=T.G)]
    if n == 4:
        p = [T.Prob(rng, M, 200, (288,), a_guard=T.G)] + p + [T.Prob(rng, M, 200, (96,), bias=False, act=T.ACT_RELU, a_guard=T.G)]
    return p


def case(key, probs, lst, cnt, rows, **kw):
    # run() compares every canvas whole with the expected image and raises on any difference
    try:
        count = torch.tensor([cnt], dtype=torch.int32, device=T.DEV)
        ks, cls, tags, _ = T.run(probs, key, rows=rows, greedy_scope=True, row_list=dev_list(lst), row_count=count, **kw)
        assert cls == 128 and ks == [1] * len(probs), (cls, ks)
        out["tags/" + key] = np.array(tags)
        out["fail/" + key] = np.array("")
    except AssertionError as e:
        out["fail/" + key] = np.array(str(e)[:500] or "assertion")


for kind in R.LISTS:
    rng = T._rng(41, R.LISTS.index(kind))
    lst = {"ordered": np.arange(M), "permuted": rng.permutation(M), "repeats": rng.integers(0, M, M)}[kind].astype(np.int32)
    for n in R.TASKS:
        probs = probs_of(rng, n)
        for cnt in R.COUNTS:
            case("%s_tasks%d_count%d" % (kind, n, cnt), probs, lst, cnt, np.unique(lst[:cnt]), adjacent=(n == 2 and cnt == 129),
                 vec=not (n == 2 and cnt == 129))
# clamp pass
rng = T._rng(42)
probs = probs_of(rng, 2)
lst = rng.permutation(M).astype(np.int32)
lst[[1, 140]] = (-1, M)
rows = np.unique(np.clip(lst[:150], 0, M - 1))
assert 0 in rows and M - 1 in rows
case("clamp_indices", probs, lst, 150, rows)
for cnt in R.CLAMP_COUNTS:
    eff = min(max(cnt, 0), M)
    case("clamp_count%d" % cnt, probs, lst, cnt, np.unique(np.clip(lst[:eff], 0, M - 1)))

# rounding pass
Mr, Nr, Kr = R.ROUND_SHAPE


def product(a, w, scope, lst=None, cnt=0, hint=0):
    c = torch.full((Mr + 2, Nr + 8), float("nan"), device=T.DEV)
    kw = {}
    if lst is not None:
        kw = dict(row_list=dev_list(lst), row_count=torch.tensor([cnt], dtype=torch.int32, device=T.DEV))
    torch.cuda.synchronize()
    T._lib.load().set_profile_enable(1)
    try:
        gemm_nt_group([dict(segs=[(a, w)], C=c[1:Mr + 1, 4:4 + Nr], ksplit=1)], greedy_scope=scope, bm_hint=hint, **kw)
        torch.cuda.synchronize()
        tags = sorted(e["tag"] for e in T._lib.profile_report() if e["tag"].startswith(("gemm_nt", "gemv_nt")))
    finally:
        T._lib.load().set_profile_enable(0)
    h = c.cpu().numpy()
    inside = h[1:Mr + 1, 4:4 + Nr].copy()
    h[1:Mr + 1, 4:4 + Nr] = np.nan
    assert np.isnan(h).all(), "stores outside C"
    return inside, tags


for seed in R.ROUND_SEEDS:
    rng = np.random.default_rng([43, seed])
    a, w = rng.standard_normal((Mr, Kr)).astype(np.float32), rng.standard_normal((Nr, Kr)).astype(np.float32)
    ref = a.astype(np.float64) @ w.astype(np.float64).T
    ad, wd = torch.from_numpy(a).to(T.DEV), torch.from_numpy(w).to(T.DEV)
    lst = rng.permutation(Mr).astype(np.int32)
    listed = np.sort(lst[:R.ROUND_COUNT])
    full, tags_full = product(ad, wd, True)
    part, tags_part = product(ad, wd, True, lst, R.ROUND_COUNT)
    fp32, tags_fp32 = product(ad, wd, False, lst, R.ROUND_COUNT, hint=128)
    k = "round/seed%d/" % seed
    out[k + "tags"] = np.array(tags_full + tags_part + tags_fp32)
    unlisted = np.setdiff1d(np.arange(Mr), listed)
    out[k + "unlisted_untouched"] = np.array([np.isnan(part[unlisted]).all() and np.isnan(fp32[unlisted]).all()])
    out[k + "same_bits"] = np.array([np.array_equal(part[listed].view(np.uint32), full[listed].view(np.uint32))])
    out[k + "err_split"] = np.array([np.abs(part[listed].astype(np.float64) - ref[listed]).max()])
    out[k + "err_fp32"] = np.array([np.abs(fp32[listed].astype(np.float64) - ref[listed]).max()])

# refusals
rng = T._rng(44)
count = torch.tensor([3], dtype=torch.int32, device=T.DEV)
one = torch.tensor([1], dtype=torch.int32, device=T.DEV)
lst_d = dev_list(rng.permutation(129).astype(np.int32))
p = T.Prob(rng, 129, 64, (96,), ksplit=2)
cv = T.Canvas(129, T._ld(64, True))
rc_split, _, _ = gemm_nt_group([dict(segs=p.segs, C=cv.view(4, 64), ksplit=2)], row_list=lst_d, row_count=count, code=True,
                               greedy_scope=True)
q = T.Prob(rng, 129, 64, (96,))
rc_gate, _, _ = gemm_nt_group([dict(segs=q.segs, C=cv.view(4, 64), ksplit=1)], row_list=lst_d, row_count=count, alive=one,
                              code=True, greedy_scope=True)
s = T.Prob(rng, 16, 64, (96,))
cs = T.Canvas(16, T._ld(64, True))
rc_16, _, _ = gemm_nt_group([dict(segs=s.segs, C=cs.view(4, 64), ksplit=1)], row_list=lst_d, row_count=count, code=True,
                            greedy_scope=True)
torch.cuda.synchronize()
cv.check("refused (split-K, loop gate)")
cs.check("refused (16-row class)")
out["refusals"] = np.array([rc_split, rc_gate, rc_16])
np.savez(sys.argv[1], **out)
"""


@pytest.fixture(scope="module")
def rec(tmp_path_factory):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    f = os.path.join(str(tmp_path_factory.mktemp("split_rowlist")), "rec.npz")
    env = {k: v for k, v in os.environ.items() if k != "SET_GEMM_SPLIT"}
    r = subprocess.run([sys.executable, "-c", _CHILD, f], env=env, cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    return dict(np.load(f))


def _held(rec, key):
    assert str(rec["fail/" + key]) == "", (key, str(rec["fail/" + key]))
    assert list(rec["tags/" + key]) == [SPLIT_TAG], (key, rec["tags/" + key])


@pytest.mark.parametrize("cnt", COUNTS)
@pytest.mark.parametrize("n", TASKS)
@pytest.mark.parametrize("kind", LISTS)
def test_exact_listed_rows(rec, kind, n, cnt):
    _held(rec, "%s_tasks%d_count%d" % (kind, n, cnt))


@pytest.mark.parametrize("key", ["clamp_indices"] + ["clamp_count%d" % c for c in CLAMP_COUNTS])
def test_clamps(rec, key):
    _held(rec, key)


@pytest.mark.parametrize("seed", ROUND_SEEDS)
def test_rounding_listed_rows_are_the_full_split_launch(rec, seed):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "profiles", "gemm_split_errors.json")) as f:
        margin = float(json.load(f)["margin_of_the_test"])
    k = "round/seed%d/" % seed
    e_split, e_fp32 = float(rec[k + "err_split"][0]), float(rec[k + "err_fp32"][0])
    print("seed %d: split %.3e  fp32 %.3e  ratio %.3f (bound %.2f)" % (seed, e_split, e_fp32, e_split / e_fp32, margin))
    assert list(rec[k + "tags"]) == [SPLIT_TAG, SPLIT_TAG, FP32_TAG], rec[k + "tags"]
    assert rec[k + "unlisted_untouched"][0]
    assert rec[k + "same_bits"][0]
    assert e_split <= margin * e_fp32, (e_split, e_fp32)


def test_refusals(rec):
    """SET_ERR_ARG = 1: a list on a split-K problem, a list together with the loop gate; SET_ERR_UNSUPPORTED = 2: 16 rows"""
    assert list(rec["refusals"]) == [1, 1, 2], rec["refusals"]
