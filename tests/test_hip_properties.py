"""GPU, BASELINE.json full size (B=128, 36x2048, T=20, V=10000): size-independent properties of the
decode path that need no oracle run — run-to-run determinism, batch-permutation equivariance,
padding invariance, sub-batch consistency, stream independence."""
import numpy as np
import pytest
import torch

import parity
from hip_adapter import editnet_modules, to_dev

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def setup():
    d, xe, rl = editnet_modules("editnet_full_b128")
    return d, xe, rl, to_dev(d["X"]), to_dev(d["prev"]), to_dev(d["plen"])


def _greedy(rl, wm, prev, plen, X):
    with torch.no_grad():
        seq, logp = rl(wm, prev, plen, X, True, False)
    torch.cuda.synchronize()
    return seq.cpu().numpy(), logp.cpu().numpy()


def test_determinism_and_stream_independence(setup):
    d, xe, rl, X, prev, plen = setup
    first = _greedy(rl, d["wm"], prev, plen, X)       # 1st call: no token table yet (summation order differs)
    a = _greedy(rl, d["wm"], prev, plen, X)           # from the 2nd call on the folded token table is used
    b = _greedy(rl, d["wm"], prev, plen, X)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), "two runs must be bit-identical"
    # first call vs token-table call: judged row by row with the REFERENCE's per-step top-1/top-2 margins of this very case
    # (tests/golden/editnet_full_b128.npz): rows without a near-tie are bit-identical, a near-tie row agrees up to that step
    margins = parity.load("editnet_full_b128")["greedy_margin"]
    n_amb = parity.check_two_paths_rows(first[0], first[1], a[0], a[1], margins, tol=1e-4)
    assert n_amb <= 6, n_amb
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        c = _greedy(rl, d["wm"], prev, plen, X)
    assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1]), "a different stream / workspace must not matter"


def test_batch_permutation_equivariance(setup):
    d, xe, rl, X, prev, plen = setup
    a = _greedy(rl, d["wm"], prev, plen, X)
    perm = torch.from_numpy(np.random.RandomState(0).permutation(X.shape[0])).to(X.device)
    b = _greedy(rl, d["wm"], prev[perm].contiguous(), plen[perm].contiguous(), X[perm].contiguous())
    p = perm.cpu().numpy()
    assert np.array_equal(a[0][p], b[0]) and np.array_equal(a[1][p], b[1]), "rows are independent samples"


def test_padding_invariance(setup):
    """Extra <pad> columns on the previous captions (T=20 -> 26) change nothing: masked positions carry
    exactly zero attention weight (exp(-1e10 - max) == 0) and the encoder stops at each length."""
    d, xe, rl, X, prev, plen = setup
    a = _greedy(rl, d["wm"], prev, plen, X)
    prev2 = torch.cat([prev, torch.zeros(prev.shape[0], 6, dtype=prev.dtype, device=prev.device)], 1).contiguous()
    b = _greedy(rl, d["wm"], prev2, plen, X)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_padding_invariance_small_batch(setup):
    """the same property on the small-batch kernels (4 rows: gemv row class, 512-thread attention launch whose two thread
    halves own FIXED blocks of positions, persistent encoder): bit-identical with six more <pad> columns"""
    d, xe, rl, X, prev, plen = setup
    p4, l4, X4 = prev[:4].contiguous(), plen[:4].contiguous(), X[:4].contiguous()
    a = _greedy(rl, d["wm"], p4, l4, X4)
    p4b = torch.cat([p4, torch.zeros(4, 6, dtype=prev.dtype, device=prev.device)], 1).contiguous()
    b = _greedy(rl, d["wm"], p4b, l4, X4)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    full = _greedy(rl, d["wm"], prev, plen, X)            # and the rows agree with their decode inside the full batch
    same = (full[0][:4] == a[0]).all(1)
    assert same.all() or np.abs(full[1][:4][same] - a[1][same]).max() < 1e-4


def test_sub_batch_consistency(setup):
    """Rows decoded alone (B=32 -> 64x64 GEMM tiles, other split-K plan) agree with the same rows decoded
    inside the full batch to fp32 summation-order noise; tokens bit-exact away from near-ties."""
    d, xe, rl, X, prev, plen = setup
    a = _greedy(rl, d["wm"], prev, plen, X)
    b = _greedy(rl, d["wm"], prev[:32].contiguous(), plen[:32].contiguous(), X[:32].contiguous())
    margins = parity.load("editnet_full_b128")["greedy_margin"][:, :32]
    n_amb = parity.check_two_paths_rows(a[0][:32], a[1][:32], b[0], b[1], margins, tol=1e-4)
    assert n_amb <= 3, n_amb


def test_xe_rows_beyond_decode_length_are_zero_and_prefix_consistent(setup):
    d, xe, rl, X, prev, plen = setup
    caps, clen = to_dev(d["caps"]), to_dev(d["clen"])
    with torch.no_grad():
        pred, caps_s, dl, sort_ind = xe(X, caps, clen, prev, plen, False, 0.0)
    pred = pred.cpu().numpy()
    for b, L in enumerate(dl):
        assert not pred[b, L:].any()
        assert np.abs(pred[b, :L]).max() > 0
    assert list(dl) == sorted(dl, reverse=True)


def test_device_prefetcher_roundtrip(setup):
    from show_edit_tell_amd.pipeline import DevicePrefetcher
    d, xe, rl, X, prev, plen = setup
    host = [(torch.from_numpy(d["X"][i * 32:(i + 1) * 32].copy()), torch.from_numpy(d["prev"][i * 32:(i + 1) * 32].copy()))
            for i in range(4)]
    got = list(DevicePrefetcher(host, X.device, depth=2))
    assert len(got) == 4
    for (hx, hp), (dx, dp) in zip(host, got):
        assert dx.is_cuda and torch.equal(dx.cpu(), hx) and torch.equal(dp.cpu(), hp)


def test_split_precision_gemm_keeps_parity():
    """The bf16-split emulated-fp32 GEMM (csrc/gemm_split_bf16.inc, in both library variants) on EVERY launch it can take
    (SET_GEMM_SPLIT=1, here on the experimental library variant) must be fp32-grade: rerun the golden
    parity tests of the full-size model (greedy tokens bit-exact, logits within 1e-4) and the fp64 linear check with the
    switch on.  Library variant and switch are read once per process, hence the child process."""
    import os
    import subprocess
    import sys
    from show_edit_tell_amd import build
    build.build(variant="exp")
    env = dict(os.environ, SET_GEMM_SPLIT="1", SET_LIB_VARIANT="exp")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    which = subprocess.run([sys.executable, "-c", "from show_edit_tell_amd import _lib; print(_lib.LIB_PATH)"], env=env, cwd=root,
                           capture_output=True, text=True, timeout=300)
    assert which.stdout.strip().endswith("libset_hip_exp.so"), which.stdout + which.stderr
    cmd = [sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
           os.path.join(root, "tests", "test_hip_editnet.py"), os.path.join(root, "tests", "test_hip_ops.py"),
           "-k", "full_b128 or full_b4 or v9490 or linear_shapes or token_table"]
    out = subprocess.run(cmd, env=env, cwd=root, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert " passed" in out.stdout and "failed" not in out.stdout


@pytest.mark.parametrize("env_extra", [{"SET_GEMM_KGROUPS": "2"}, {"SET_GEMM_VEC_EPILOGUE": "0"}],
                         ids=["8-wave k-group kernel", "scalar epilogue stores"])
def test_gemm_kernel_variants_keep_parity(env_extra):
    """Opt-in / fallback variants of the grouped GEMM (csrc/gemm_f32.hip): the 8-wave workgroup with an intra-workgroup
    K split (SET_GEMM_KGROUPS=2) and the scalar epilogue (SET_GEMM_VEC_EPILOGUE=0) must pass the same golden parity
    tests as the default kernel.  The switches are read once per process, hence the child process.  (The 8-wave kernel lives
    in the experimental library variant only: SET_LIB_VARIANT=exp.)"""
    import os
    import subprocess
    import sys
    env = dict(os.environ, **env_extra)
    if "SET_GEMM_KGROUPS" in env_extra:
        from show_edit_tell_amd import build
        build.build(variant="exp")
        env["SET_LIB_VARIANT"] = "exp"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
           os.path.join(root, "tests", "test_hip_editnet.py"), os.path.join(root, "tests", "test_hip_ops.py"),
           "-k", "full_b128 or full_b4 or v9490 or linear_shapes"]
    out = subprocess.run(cmd, env=env, cwd=root, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert " passed" in out.stdout and "failed" not in out.stdout


def test_pick_without_the_lstm_tail_keeps_parity():
    """Free-running loops: the pick kernel finishes the next timestep's attention-LSTM cell by default (LstmTail,
    csrc/epilogue.hip).  SET_PICK_TAIL=0 restores the separate lstm_pointwise launch; the greedy / sampled rollout tests
    of both models must pass either way (the default route is what the rest of the suite runs)."""
    import os
    import subprocess
    import sys
    env = dict(os.environ, SET_PICK_TAIL="0")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
           os.path.join(root, "tests", "test_hip_editnet.py"), os.path.join(root, "tests", "test_hip_dcnet.py"),
           os.path.join(root, "tests", "test_hip_sampling.py"), "-k", "greedy or rollout or sample"]
    out = subprocess.run(cmd, env=env, cwd=root, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert " passed" in out.stdout and "failed" not in out.stdout
