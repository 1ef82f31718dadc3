"""Generates tests/golden/draw_mask_golden.npz: one small image (24 x 20 x 3, extreme pixel values among random ones), a mask with
the values 0..3, and what the reference's utils.get_draw_mask returns for them at alpha 0.25, 0.5, 0.75 and 1.0, with and without
skip_background.  tests/test_preview_host.py holds rule_overlay and preview.make_lut to these bytes.

The reference's utils.py is imported at run time from the directory given on the command line; its `import cv2` is met by an empty
stand-in module (get_draw_mask is numpy only).  Only the arrays are kept.
      python tests/golden/make_draw_mask_golden.py REFERENCE_DIR"""
import importlib.util
import os
import sys
import types

import numpy as np

ALPHAS = (0.25, 0.5, 0.75, 1.0)


def main(reference_dir):
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    spec = importlib.util.spec_from_file_location("reference_utils", os.path.join(reference_dir, "utils.py"))
    utils = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(utils)

    rng = np.random.default_rng(2026)
    H, W = 24, 20
    img = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
    img[:4, :5] = 255
    img[4:8, :5] = 0
    img[8:12, :5] = (255, 0, 254)
    img[12:16, :5] = (1, 127, 128)
    mask = (rng.integers(0, 4, (H // 4, W // 5)).astype(np.uint8).repeat(4, axis=0).repeat(5, axis=1))
    mask[:16, :5] = np.arange(16)[:, None] % 4             # every value over every extreme
    mask[20:, 15:] = rng.integers(0, 4, (4, 5))
    out = {"img": img, "mask": mask, "alphas": np.array(ALPHAS)}
    out["colour_values"] = np.array([v for v, _c in utils.get_seg_color_map()], np.int64)
    out["colours"] = np.stack([c for _v, c in utils.get_seg_color_map()]).astype(np.uint8)
    for alpha in ALPHAS:
        for skip in (True, False):
            drawn = utils.get_draw_mask(img, mask, alpha=alpha, color_map=None, skip_background=skip)
            assert drawn.dtype == np.uint8 and drawn.shape == img.shape
            out["drawn_%03d_%s" % (round(alpha * 100), "skip" if skip else "all")] = drawn
    np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "draw_mask_golden.npz"), **out)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
