"""Generates tests/golden/mask_morph.npz: a few small u8 masks and what scipy.ndimage's grey morphology makes of each -- a 5x5
grey_closing followed by a 5x5 grey_opening, mode='nearest' (replicated edges never win a max or a min, so outside taps are skipped).
tests/test_mask_morph_host.py holds rule_morph to these bytes, with or without scipy installed.
      python tests/golden/make_mask_morph_golden.py"""
import os
import sys

import numpy as np
import scipy
from scipy import ndimage as ndi

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def main():
    from tests.test_mask_morph_host import make
    out = {"scipy_version": np.array(scipy.__version__)}
    cases = {"blobs": make("blobs", 2025, (64, 64)), "half": make("half", 2026, (33, 47)), "classes": make("classes", 2027, (48, 20)),
             "bytes": make("bytes", 2028, (17, 64)), "dense": make("dense", 2029, (64, 31)), "frame0": make("frame0", 0, (9, 12)),
             "narrow": make("blobs", 2030, (40, 3))}
    kw = dict(size=(5, 5), mode="nearest")
    for name, m in cases.items():
        out[name + "_mask"] = m
        out[name + "_morph"] = ndi.grey_opening(ndi.grey_closing(m, **kw), **kw)
    np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "mask_morph.npz"), **out)


if __name__ == "__main__":
    main()
