#!/usr/bin/env python
"""Beam-search golden vectors for the ADAPTIVE-features EditNet, from the reference's own loop (authoring container only).

    python tools/make_adaptive_beam_golden.py        # rewrites tests/golden/beam_adaptive_{small,full_b4}.npz

The reference evaluates its adaptive model with the per-image beam search of `adaptive_features/editnet_adaptive.py`
`evaluate()`: the loop variables are (img, img_mean, image_id, previous_caption, prev_caplen), the image mean comes with
the image (it is the mean over the VALID regions, not over all R slots) and the visual attention masks the zero-padded
regions.  That loop body is sliced and `/`->`//` patched by oracle/ref_beam.py and run on the reference's own adaptive
`DecoderC` (oracle/ref_slice.py) with the synthetic weights of oracle/cases.py, `fc.bias[<end>]` raised by each boost
below.  Stored are numbers only, in the schema tests/beam_parity.check_one reads (`k{k}.{model}.{field}`, one model name
per boost, e.g. `adaptive_e25`), plus the boosts and the valid-region counts; inputs and weights are rebuilt from the
seeds.  The archive is written with fixed member time stamps, so two runs give bit-identical files.
"""
from __future__ import annotations

import io
import os
import sys
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import cases, ref_beam, ref_slice  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
LMAX = 64

# golden name -> (adaptive case of oracle/cases.py, beam sizes, <end> boosts).  Each boost gives a mix of searches that
# finish within a few steps and searches that run into the 50-step limit after k shrank (some with completed hypotheses).
CASES = {
    "beam_adaptive_small": ("editnet_adaptive_small", (1, 3, 5), (2.5, 4.0)),
    "beam_adaptive_full_b4": ("editnet_adaptive_full_b4", (1, 2, 3, 4), (3.5, 5.0)),
}


def model_name(boost):
    return "adaptive_e%d" % int(round(boost * 10))


def boosted(sd, V, boost):
    sd = dict(sd)
    sd["fc.bias"] = sd["fc.bias"].copy()
    sd["fc.bias"][V - 1] += np.float32(boost)
    return sd


def _record(res):
    seq, comp, comp_scores, infinite = res
    seq = [int(w) for w in seq]
    sc = sorted((float(s) for s in comp_scores), reverse=True)
    return dict(seq=np.asarray(seq + [-1] * (LMAX - len(seq)), np.int64), n=np.int64(len(seq)),
                score=np.float64(sc[0] if (sc and not infinite) else np.nan), ncomplete=np.int64(len(comp)),
                infinite=np.bool_(bool(infinite)),
                margin=np.float64(sc[0] - sc[1] if len(sc) > 1 else np.inf))


def save_npz(path, arrays):
    """np.savez_compressed with a fixed member time stamp and order (numpy stamps members with the current time)."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[key]), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o600 << 16
            z.writestr(info, buf.getvalue())


def make(name):
    case, beams, boosts = CASES[name]
    d = cases.build_editnet(case)
    c, wm = d["case"], d["wm"]
    beam_one, names = ref_beam.load_beam_fn(os.path.join("adaptive_features", "editnet_adaptive.py"), "evaluate", ["decoder"])
    assert names == ["img", "img_mean", "image_id", "previous_caption", "prev_caplen"], names
    cls = ref_slice.editnet_adaptive()["DecoderC"]
    T_ = torch.from_numpy
    out = {"boosts": np.asarray(boosts, np.float64), "beams": np.asarray(beams, np.int64),
           "nvalid": np.asarray(d["nvalid"], np.int64)}
    summary = []
    with torch.no_grad():
        for boost in boosts:
            model = model_name(boost)
            dec = ref_slice.load_state(cls(wm, c["D"], c["D"], c["D"], c["A"], c["F"]), boosted(d["sd"], c["V"], boost)).eval()
            for k in beams:
                recs = []
                for b in range(c["B"]):
                    img, mean = T_(d["X"][b:b + 1]), T_(d["image_mean"][b:b + 1])
                    prev, plen = T_(d["prev"][b:b + 1]), T_(d["plen"][b:b + 1])
                    recs.append(_record(beam_one(dec, wm, k, img, mean, torch.tensor([[b]]), prev, plen)))
                for field in recs[0]:
                    out["k%d.%s.%s" % (k, model, field)] = np.stack([r[field] for r in recs])
                inf = out["k%d.%s.infinite" % (k, model)]
                nc = out["k%d.%s.ncomplete" % (k, model)]
                summary.append("%s k=%d: %d/%d at the limit (completed there: %s)" % (
                    model, k, int(inf.sum()), c["B"], nc[inf].tolist()))
    path = os.path.join(OUT, name + ".npz")
    save_npz(path, out)
    print("%-22s %6.1f KiB" % (name, os.path.getsize(path) / 1024))
    for s in summary:
        print("    " + s)


def main(argv):
    assert ref_slice.have_reference(), "needs the reference sources (authoring container only)"
    torch.manual_seed(0)
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    want = set(argv[1:])
    for name in CASES:
        if not want or name in want:
            make(name)


if __name__ == "__main__":
    main(sys.argv)
