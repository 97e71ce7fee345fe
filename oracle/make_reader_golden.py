"""ORACLE tooling (authoring container only): what the reference's own COCOTrainDataset.__getitem__ (editnet.py:46-74,
AST-sliced from the reference, oracle/ref_slice.py; its HDF5 datasets replaced by arrays) returns as the image tensor for
every sample of tests/test_pipeline_cpu.py's fixed dataset.

    python -m oracle.make_reader_golden           # rewrites tests/golden/reader_getitem.npz

Only numbers computed by the reference are stored (key `img`, one row per sample index)."""
from __future__ import annotations

import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_slice  # noqa: E402
from oracle.make_golden import OUT  # noqa: E402


def main():
    assert ref_slice.have_reference(), "needs the reference sources (authoring container only)"
    from test_pipeline_cpu import _fixed_dataset
    with tempfile.TemporaryDirectory() as tmp:
        ds = _fixed_dataset(tmp)
    cls = ref_slice.load_classes("editnet.py", ("COCOTrainDataset",))["COCOTrainDataset"]
    obj = cls.__new__(cls)
    n = len(ds["captions"])
    obj.train_features, obj.val_features, obj.cpi = ds["tr"], ds["va"], ds["cpi"]
    obj.captions, obj.caplens, obj.names = ds["captions"], ds["caplens"], ds["names"]
    obj.caption_util, obj.objdet, obj.dataset_size = ds["util"], ds["objdet"], n
    img = np.stack([obj[i][0].numpy() for i in range(n)])
    path = os.path.join(OUT, "reader_getitem.npz")
    np.savez_compressed(path, img=img)
    print("reader_getitem.npz %.1f KiB: img %s %s" % (os.path.getsize(path) / 1024, img.shape, img.dtype))


if __name__ == "__main__":
    main()
