"""Generates tests/golden/jpeg_roundtrip.npz: three small RGB images and the pixels Pillow's libjpeg-turbo decodes from its own
quality-95 4:2:0 file of each -- what a reader of the dataset's img_*.jpg sees.  tests/test_jpeg_roundtrip_host.py holds
rule_roundtrip to these bytes, with or without Pillow installed.      python tests/golden/make_jpeg_roundtrip_golden.py"""
import io
import os
import sys

import numpy as np
from PIL import Image, features

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def main():
    from tests.test_jpeg_roundtrip_host import checker, noise, smooth
    out = {"libjpeg_turbo_version": np.array(features.version_feature("libjpeg_turbo") or "unknown")}
    cases = {"smooth": smooth(48, 48), "noise": noise(2025, 32, 48), "checker": checker(16, 32)}
    for name, img in cases.items():
        b = io.BytesIO()
        Image.fromarray(img, "RGB").save(b, "JPEG", quality=95, subsampling=2)
        out[name + "_rgb"] = img
        out[name + "_q95_decoded"] = np.asarray(Image.open(io.BytesIO(b.getvalue())).convert("RGB"))
    np.savez_compressed(os.path.join(os.path.dirname(os.path.abspath(__file__)), "jpeg_roundtrip.npz"), **out)


if __name__ == "__main__":
    main()
