"""How the per-stage float64 tests (tests/test_hip_step_stages.py, tests/test_hip_prologue_stages.py) judge one stage's device
output against its float64 restatement, and the error report both can write."""
import json

import numpy as np

import parity


def judge(ratios, key, stage, got, ref, tol, what, f32=None):
    """got (device) against ref (float64 stage): relative to max|ref| and absolute; records the ratios first, in
    ratios[key][stage] = [largest device ratio, largest float32-oracle ratio]"""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == np.float32, (what, got.shape, ref.shape, got.dtype)
    assert np.isfinite(got).all(), what
    scale = float(np.abs(ref).max())
    assert scale > 0, what + ": the float64 stage is identically zero, nothing would be compared"
    bound = tol * min(scale, 1.0)
    err = parity.maxerr(got, ref)
    rec = ratios.setdefault(key, {}).setdefault(stage, [0.0, 0.0])
    rec[0] = max(rec[0], err / bound)
    if f32 is not None:
        rec[1] = max(rec[1], parity.maxerr(f32, ref) / bound)
    print("%-46s err %.3e  max|ref| %.3e  ratio %.3f" % (what, err, scale, err / bound))
    assert err <= tol * scale, "%s: max abs err %.3e > %.1e * max|ref| %.3e" % (what, err, tol, scale)
    parity.assert_close(got, ref, tol, what)


def write_report(path, unit, ratios):
    """one line per (model, grid id): {stage: [device, float32 oracle]}"""
    lines = ['"unit": ' + json.dumps(unit)]
    for (model, gid), stages in sorted(ratios.items()):
        lines.append(json.dumps("%s/%s" % (model, gid)) + ": "
                     + json.dumps({k: [round(v[0], 4), round(v[1], 4)] for k, v in stages.items()}))
    with open(path, "w") as f:
        f.write("{\n " + ",\n ".join(lines) + "\n}\n")
