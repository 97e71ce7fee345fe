"""Golden vectors on disk: tests/golden/<name>.npz, spilling into <name>.part2.npz, <name>.part3.npz, ... so that no
file holds more than PART_BYTES.  save() packs whole arrays into parts by their compressed size; load() merges the parts
back into one dict, so a caller never sees the split."""
from __future__ import annotations

import glob
import io
import os

import numpy as np

PART_BYTES = 960 << 10          # a committed file stays below 1 MiB with room for the zip directory


def _part_paths(stem):
    return sorted(glob.glob(glob.escape(stem) + ".part*.npz"), key=lambda p: int(p.rsplit(".part", 1)[1][:-4]))


def save(stem, arrays):
    """write `arrays` as stem.npz (+ stem.partK.npz); stale parts of an earlier save are removed"""
    for p in _part_paths(stem):
        os.remove(p)
    sizes = {}
    for k, v in arrays.items():
        b = io.BytesIO()
        np.savez_compressed(b, **{k: v})
        sizes[k] = len(b.getvalue())
    parts, cur, used = [], {}, 0
    for k in arrays:
        if cur and used + sizes[k] > PART_BYTES:
            parts.append(cur)
            cur, used = {}, 0
        cur[k] = arrays[k]
        used += sizes[k]
    parts.append(cur)
    paths = [stem + ".npz"] + ["%s.part%d.npz" % (stem, i) for i in range(2, len(parts) + 1)]
    for path, part in zip(paths, parts):
        np.savez_compressed(path, **part)
    return paths


def load(stem):
    out = {}
    for path in [stem + ".npz"] + _part_paths(stem):
        with np.load(path) as z:
            for k in z.files:
                assert k not in out, "%s: %s repeats a key of an earlier part" % (path, k)
                out[k] = z[k]
    return out


def size(stem):
    """bytes on disk over all parts"""
    return sum(os.path.getsize(p) for p in [stem + ".npz"] + _part_paths(stem))

