"""GPU: the free-running decode loops no longer execute work whose result nobody reads (csrc/editnet.hip rollout,
csrc/dcnet.hip dcnet_rollout, csrc/gemm_fused.hip fused_encoder_step):

* the reference's timestep `max_len`, which it computes and discards (editnet_rl.py:503,517-518; dcnet_rl.py:305,315-316),
  is not run; the fc of timestep `max_len - 1` launches alone, on the split-K plan and row tile it had inside the merged
  fc + next-phase-A launch;
* with the token table the phase-A products of timestep 0 ([h2 | h1] W and h2h(h2) over the zero state) are not launched,
  and the encoder step at t = 0 skips its contraction over the zero h.

`SET_DEAD_WORK=1` restores all of it.  The switch is read once per process, so both settings run in child processes (as
tests/test_hip_finished_rows.py does for SET_LOOP_GATE); one child per setting serves both tests.  Outputs must be
BIT-identical: every removed product is exactly zero or unread, and no surviving sum changes its order.

Dims.  The reduced dims of the small goldens (D = 64, A = 32, F = 128; DCNet D = E = 64, C = 32) at 17 rows, so that the
fused copy gate (from 17 rows) is on the path and the persistent small-batch launch (<= 16 rows) is not; SET_DEC_PERSISTENT=0
besides, for the 6-row case of test_hip_finished_rows.py where every row finishes within a few steps.  At those dims two of
the changed paths are not reachable: the fused encoder step needs D % 128 == 0 and DCNet's token table C % 128 == 0.  Two
cases one size class up (EditNet D = 128; DCNet C = 128, D = E = 256) cover them; they are still a few milliseconds a decode.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MAX_LENS = (1, 2, 18)
EDITNET = ("dw_editnet_b17", "dw_editnet_d128", "editnet_small_end")
DCNET = ("dw_dcnet_b17", "dw_dcnet_c128", "dcnet_small_end")
COUNT_CASE = "dw_editnet_d128"

_CHILD = r"""
import os, sys
import numpy as np, torch
sys.path.insert(0, os.path.join(os.getcwd(), "tests")); sys.path.insert(0, os.getcwd())
from oracle import cases
from hip_adapter import dcnet_modules, editnet_modules, to_dev
from show_edit_tell_amd import _lib
S = cases.SCALES
cases.DP_CASES["dw_editnet_b17"] = dict(cases.SMALL, V=203, R=7, T=9, B=17, wseed=11, iseed=51, ragged_caps=True, **S)
cases.DP_CASES["dw_editnet_d128"] = dict(D=128, A=32, F=128, V=203, R=7, T=9, B=17, wseed=11, iseed=52, ragged_caps=True, **S)
cases.DCNET_ALL["dw_dcnet_b17"] = dict(D=64, A=32, C=32, E=64, V=203, T=9, B=17, wseed=17, iseed=53, ragged_caps=True, **S)
cases.DCNET_ALL["dw_dcnet_c128"] = dict(D=256, A=32, C=128, E=256, V=203, T=9, B=17, wseed=17, iseed=54, ragged_caps=True, **S)
max_lens = [int(x) for x in sys.argv[2].split(",")]
out = {}

def decodes(kind, name):
    if kind == "editnet":
        d, xe, rl = editnet_modules(name)
        args = (d["wm"], to_dev(d["prev"]), to_dev(d["plen"]), to_dev(d["X"]))
    else:
        d, xe, rl = dcnet_modules(name)
        args = (d["wm"], to_dev(d["prev"]), to_dev(d["plen"]))
    for table in ("0", "1"):                      # "0": what the first no-grad call of a model runs, "1": every later one
        os.environ["SET_TOKEN_TABLE"] = table
        for L in max_lens:
            rl.max_len = L
            for mode, flags in (("greedy", (True, False)), ("sample", (False, True))):
                torch.manual_seed(1234 + L)       # the Philox seed of a sampled rollout is drawn from torch's generator
                seq, lp = rl(*args, *flags)
                key = "%s/tab%s/L%d/%s" % (name, table, L, mode)
                out[key + "/seq"] = seq.cpu().numpy()
                out[key + "/lp"] = lp.cpu().numpy()
    return rl, args

with torch.no_grad():
    for name in sys.argv[3].split(","):
        rl, args = decodes("editnet", name)
        if name == sys.argv[5]:
            lib = _lib.load()
            for L in max_lens:                    # launch counts of ONE greedy decode, table active (left on by decodes())
                rl.max_len = L
                torch.cuda.synchronize()
                lib.set_profile_enable(1)
                rl(*args, True, False)
                torch.cuda.synchronize()
                prof = _lib.profile_report()
                lib.set_profile_enable(0)
                gemm = sum(p["launches"] for p in prof if p["tag"].startswith(("gemm_nt_f32", "gemv_nt_f32")))
                att = sum(p["launches"] for p in prof if p["tag"] == "step_attention")
                out["count/L%d" % L] = np.array([gemm, att])
    for name in sys.argv[4].split(","):
        decodes("dcnet", name)
torch.cuda.synchronize()
np.savez(sys.argv[1], **out)
"""


@pytest.fixture(scope="module")
def ab(tmp_path_factory):
    """outputs of every decode with the switch unset ("new") and set ("old"), one child process each"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tmp = str(tmp_path_factory.mktemp("dead_work"))
    res = {}
    for label, val in (("new", "0"), ("old", "1")):
        f = os.path.join(tmp, label + ".npz")
        env = dict(os.environ, SET_DEAD_WORK=val, SET_DEC_PERSISTENT="0")
        r = subprocess.run([sys.executable, "-c", _CHILD, f, ",".join(map(str, MAX_LENS)), ",".join(EDITNET), ",".join(DCNET),
                            COUNT_CASE], env=env, cwd=root, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        res[label] = dict(np.load(f))
    return res


def test_dead_work_switch_changes_no_output(ab):
    """seq and seq_logp of every decode are the same arrays with and without the discarded timestep / the zero products:
    EditNet and DCNet, greedy and sampled (fixed seed: the Philox counters are per (seed, offset, t) and do not move),
    max_len 1 (skipped phase A and lone fc in one timestep), 2 and 18, with the token table and without, at 17 rows on the
    per-step loop, and on the cases whose rows all finish within a few steps (loop gate meets the new bound)."""
    new, old = ab["new"], ab["old"]
    keys = sorted(k for k in new if not k.startswith("count/"))
    assert keys == sorted(k for k in old if not k.startswith("count/"))
    assert len(keys) == (len(EDITNET) + len(DCNET)) * 2 * len(MAX_LENS) * 2 * 2
    bad = [k for k in keys if not np.array_equal(new[k], old[k])]
    assert not bad, bad
    assert (new["editnet_small_end/tab1/L18/greedy/seq"][:, -1] == 0).all()       # the rows did finish early
    # the sampled rollouts are not the greedy ones under another name
    assert not np.array_equal(new["dw_editnet_b17/tab1/L18/sample/seq"], new["dw_editnet_b17/tab1/L18/greedy/seq"])


def test_launch_counts(ab):
    """One EditNet greedy decode with the token table on the per-step loop, by the library's own launch profile
    (set_profile_enable / profile_report).  GEMM family = the tags of gemm_group's kernels (gemm_nt_f32*, gemv_nt_f32*); the
    fused small-tile kernels (encoder step, copy gate) carry other tags.
      prologue: enc affine, cap projections, att_embed, features_att, pre1                      = 5
      timestep: B, D, fc (+ next phase A inside the same launch)                                = 3 each
      before:   phase A of timestep 0 on its own, and the discarded timestep max_len            = 6 + 3 (max_len + 1)
    The prologue's 5 holds where the encoder recurrence runs fused (D % 128 == 0, here D = 128); at D = 64 the unfused
    encoder adds its x2h and T - 1 h2h launches, which is why the D = 128 case is the one counted."""
    for L in MAX_LENS:
        gemm, att = (int(x) for x in ab["new"]["count/L%d" % L])
        gemm_old, att_old = (int(x) for x in ab["old"]["count/L%d" % L])
        print("max_len %d: GEMM launches %d (switch set: %d), step_attention %d (%d)" % (L, gemm, gemm_old, att, att_old))
        assert att == L and att_old == L + 1
        assert gemm == 5 + 3 * L
        assert gemm_old == 6 + 3 * (L + 1)
