"""Generates tests/golden/mask_components.npz: a few small u8 masks and, for both connectivities, the labels (smallest raster index
of every pixel's connected component of equal value) and areas that scipy.ndimage.label gives, value by value
(tests/test_components_host.py scipy_components).  tests/test_components_host.py holds rule_components to these words, with or
without scipy installed.
      python tests/golden/make_mask_components_golden.py"""
import os
import sys

import numpy as np
import scipy

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def main():
    from tests.test_components_host import scipy_components
    from tests.test_mask_morph_host import make
    out = {"scipy_version": np.array(scipy.__version__)}
    cases = {"blobs": make("blobs", 2025, (40, 48)), "half": make("half", 2026, (17, 23)), "classes": make("classes", 2027, (24, 20)),
             "bytes": make("bytes", 2028, (9, 32)), "sparse": make("sparse", 2029, (32, 31)), "frame0": make("frame0", 0, (9, 12)),
             "narrow": make("blobs", 2030, (40, 3)), "batch": make("blobs", 2031, (2, 24, 24))}
    for name, m in cases.items():
        out[name + "_mask"] = m
        for connectivity in (4, 8):
            labels, areas = scipy_components(m, connectivity)
            out["%s_labels%d" % (name, connectivity)] = labels
            out["%s_areas%d" % (name, connectivity)] = areas
    np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "mask_components.npz"), **out)


if __name__ == "__main__":
    main()
