"""The JPEG round trip of the training stream without a GPU (include/gsa_jpeg_roundtrip.h; jpeg.roundtrip;
ImageGenerator.training_batches(jpeg_quality=...)).

``rule_roundtrip(img, quality)`` is the canonical rule in numpy int64: libjpeg's 4:2:0 encoder up to the quantised coefficients,
then its decoder's pixel path (dequantise, islow IDCT, h2v2 fancy upsampling, YCbCr -> RGB).  It is PINNED here, with zero
mismatching bytes allowed, against
* Pillow's (libjpeg-turbo's) decode of Pillow's own file,
* Pillow's decode of the project's file (the oracle encoder's header + scan with restart markers),
* a committed fixture of Pillow's decoded pixels (tests/golden/jpeg_roundtrip.npz), which holds without Pillow.
The GPU tests (tests/test_gpu_jpeg_roundtrip.py) hold the kernels to this rule bit for bit.  Also here: the argument checks of
the C entry points and of the stream's keyword, none of which needs a device."""
import io
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ITU-T T.81 Annex K.1, natural order
BASE_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                      14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                      49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], np.int64).reshape(8, 8)
BASE_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                        47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32, np.int64).reshape(8, 8)


# -- the rule ------------------------------------------------------------------------------------------------------------------
def quant_table(base, quality):
    """IJG quality scaling: q < 50 -> 5000/q, else 200 - 2q; table = clamp((base*scale + 50)/100, 1, 255)."""
    quality = min(max(int(quality), 1), 100)
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((base * scale + 50) // 100, 1, 255)


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct8(v, last):
    """One 8-point forward pass along the last axis (jfdctint: CONST_BITS 13, PASS1_BITS 2); ``last``: the column pass."""
    v = [v[..., i] for i in range(8)]
    t0, t7, t1, t6 = v[0] + v[7], v[0] - v[7], v[1] + v[6], v[1] - v[6]
    t2, t5, t3, t4 = v[2] + v[5], v[2] - v[5], v[3] + v[4], v[3] - v[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    sh = 15 if last else 11
    o = [None] * 8
    if last:
        o[0], o[4] = _descale(t10 + t11, 2), _descale(t10 - t11, 2)
    else:
        o[0], o[4] = (t10 + t11) << 2, (t10 - t11) << 2
    z1 = (t12 + t13) * 4433
    o[2], o[6] = _descale(z1 + t13 * 6270, sh), _descale(z1 - t12 * 15137, sh)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    a4, a5, a6, a7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2 = z1 * -7373, z2 * -20995
    z3, z4 = z3 * -16069 + z5, z4 * -3196 + z5
    o[7], o[5], o[3], o[1] = _descale(a4 + z1 + z3, sh), _descale(a5 + z2 + z4, sh), _descale(a6 + z2 + z3, sh), _descale(a7 + z1 + z4, sh)
    return np.stack(o, -1)


def _idct8(d, n):
    """One 8-point inverse pass along the last axis (jidctint), descale by ``n`` (11: column pass, 18: row pass)."""
    d = [d[..., i] for i in range(8)]
    z1 = (d[2] + d[6]) * 4433
    t2, t3 = z1 - d[6] * 15137, z1 + d[2] * 6270
    t0, t1 = (d[0] + d[4]) << 13, (d[0] - d[4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = d[7], d[5], d[3], d[1]
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * 9633
    a0, a1, a2, a3 = a0 * 2446, a1 * 16819, a2 * 25172, a3 * 12299
    z1, z2 = z1 * -7373, z2 * -20995
    z3, z4 = z3 * -16069 + z5, z4 * -3196 + z5
    a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
    return np.stack([_descale(x, n) for x in (t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3)], -1)


def _codec_plane(p, q):
    """(H, W) int64 samples 0..255 -> the samples the decoder rebuilds from the plane's quantised 8x8 blocks."""
    H, W = p.shape
    b = (p - 128).reshape(H // 8, 8, W // 8, 8).transpose(0, 2, 1, 3)              # (by, bx, row, col)
    c = _fdct8(b, False)                                                            # rows
    c = _fdct8(c.swapaxes(-1, -2), True).swapaxes(-1, -2)                           # columns
    q8 = q * 8
    k = np.sign(c) * ((np.abs(c) + (q8 >> 1)) // q8)
    d = k * q
    s = _idct8(d.swapaxes(-1, -2), 11).swapaxes(-1, -2)                             # columns first
    s = _idct8(s, 18)                                                               # then rows
    s = np.clip(s + 128, 0, 255)
    return s.transpose(0, 2, 1, 3).reshape(H, W)


def _upsample(p):
    """h2v2 fancy upsampling of one (H/2, W/2) plane; the edge rows and columns of the image are replicated."""
    h, w = p.shape
    r = np.arange(h)
    out = np.empty((2 * h, 2 * w), np.int64)
    for v, far in ((0, np.maximum(r - 1, 0)), (1, np.minimum(r + 1, h - 1))):
        s = 3 * p + p[far]
        left = np.concatenate([s[:, :1], s[:, :-1]], 1)
        right = np.concatenate([s[:, 1:], s[:, -1:]], 1)
        out[v::2, 0::2] = (3 * s + left + 8) >> 4
        out[v::2, 1::2] = (3 * s + right + 7) >> 4
    return out


def rule_roundtrip(img, quality):
    """(H, W, 3) or (n, H, W, 3) u8, H and W multiples of 16 -> the u8 pixels a libjpeg decoder returns for the quality-``quality``
    4:2:0 baseline file of each image.  Every image of a batch on its own."""
    img = np.asarray(img)
    if img.ndim == 4:
        return np.stack([rule_roundtrip(a, quality) for a in img]) if len(img) else img.copy()
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3 and img.shape[0] % 16 == 0 and img.shape[1] % 16 == 0
    r, g, b = (img[..., i].astype(np.int64) for i in range(3))
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    bias = np.tile(np.array([1, 2], np.int64), img.shape[1] // 4)                   # alternates along the OUTPUT columns

    def box(p):
        return (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2

    ql, qc = quant_table(BASE_LUMA, quality), quant_table(BASE_CHROMA, quality)
    y = _codec_plane(y, ql)
    cb = _upsample(_codec_plane(box(cb), qc)) - 128
    cr = _upsample(_codec_plane(box(cr), qc)) - 128
    out = np.stack([y + ((91881 * cr + 32768) >> 16), y + ((-22554 * cb - 46802 * cr + 32768) >> 16), y + ((116130 * cb + 32768) >> 16)], -1)
    return np.clip(out, 0, 255).astype(np.uint8)


# -- the inputs ----------------------------------------------------------------------------------------------------------------
def noise(seed, H, W):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def saturated(seed, H, W):
    """{0, 255} noise: the largest swings the colour conversion and the clamps can meet."""
    return (np.random.default_rng(seed).integers(0, 2, (H, W, 3)) * 255).astype(np.uint8)


def checker(H, W):
    """The 1-px black / white checker: all of a block's energy in its highest frequency."""
    yy, xx = np.mgrid[0:H, 0:W]
    return np.ascontiguousarray(np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[..., None], 3, -1))


def smooth(H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    return np.stack([(128 + 100 * np.sin(xx / 5.0 + yy / 9.0)), (yy * 7 + xx * 3) % 256, 255 - (yy * 255) // max(H - 1, 1)], -1).astype(np.uint8)


def pin_images():
    return {"noise16": noise(1, 16, 16), "noise32x48": noise(2, 32, 48), "saturated48x16": saturated(3, 48, 16),
            "checker32x48": checker(32, 48), "black": np.zeros((16, 16, 3), np.uint8), "white": np.full((16, 32, 3), 255, np.uint8),
            "smooth64": smooth(64, 64)}


def _need_pillow_jpeg():
    features = pytest.importorskip("PIL.features")
    if not features.check("jpg"):
        pytest.skip("Pillow without JPEG support")


def pillow_decode(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def pillow_roundtrip(img, quality):
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(img, "RGB").save(b, "JPEG", quality=quality, subsampling=2)
    return pillow_decode(b.getvalue())


def _mismatches(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype == np.uint8
    return int((got != want).sum())


# -- the three pins ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quality", [85, 95, 100])
def test_rule_equals_pillows_decode_of_pillows_file(quality):
    _need_pillow_jpeg()
    for name, img in pin_images().items():
        assert _mismatches(rule_roundtrip(img, quality), pillow_roundtrip(img, quality)) == 0, "%s q%d" % (name, quality)


@pytest.mark.parametrize("quality,restart", [(85, 1), (95, 4), (100, 3)])
def test_rule_equals_pillows_decode_of_the_projects_file(quality, restart):
    """The oracle encoder's file (header + scan with restart markers, what csrc/gsa_jpeg.hip writes byte for byte): restart markers
    do not change the pixels."""
    _need_pillow_jpeg()
    from oracle import jpeg_binding as J
    for name, img in pin_images().items():
        data = J.encode(img, quality, restart)
        assert _mismatches(rule_roundtrip(img, quality), pillow_decode(data)) == 0, "%s q%d ri%d" % (name, quality, restart)


def test_rule_reproduces_the_committed_decoded_pixels():
    """The same pin without Pillow: what libjpeg-turbo decoded from its own q95 files (tests/golden/make_jpeg_roundtrip_golden.py)."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_roundtrip.npz"))
    keys = sorted(k[:-4] for k in g.files if k.endswith("_rgb"))
    assert len(keys) == 3
    for k in keys:
        img, want = g[k + "_rgb"], g[k + "_q95_decoded"]
        assert img.shape[0] <= 48 and img.shape[1] <= 48
        assert _mismatches(rule_roundtrip(img, 95), want) == 0, k
        assert not np.array_equal(img, want), "%s: the codec changed nothing, the case pins nothing" % k


def test_rule_treats_every_image_of_a_batch_alone():
    batch = np.stack([noise(5, 32, 32), smooth(32, 32), checker(32, 32)])
    out = rule_roundtrip(batch, 95)
    assert out.shape == batch.shape and out.dtype == np.uint8
    for i in range(3):
        assert np.array_equal(out[i], rule_roundtrip(batch[i], 95))
    assert rule_roundtrip(batch[:0], 95).shape == (0, 32, 32, 3)


# -- the C ABI and the keyword validation --------------------------------------------------------------------------------------
def test_roundtrip_header_symbols_are_exported():
    from tests.common import header_declarations
    assert set(header_declarations("gsa_jpeg_roundtrip.h")[1]) == {"gsa_jpeg_roundtrip_workspace_bytes", "gsa_jpeg_roundtrip"}


def test_roundtrip_rejects_bad_arguments_before_touching_the_gpu(hip_library):
    """Argument validation of gsa_jpeg_roundtrip happens on the host (no HIP call precedes it): sizes that are not multiples of 16,
    a negative batch, null / misaligned / aliased pointers, a short workspace, a quality outside 1..100; an empty batch is a
    successful no-op."""
    from gan_segmentation_amd._lib import load_library
    size, rt = load_library().fn("gsa_jpeg_roundtrip_workspace_bytes"), load_library().fn("gsa_jpeg_roundtrip")
    assert size(1, 64, 64) == 64 * 64 * 3 // 2 and size(3, 32, 48) == 3 * 32 * 48 * 3 // 2 and size(0, 64, 64) == 0
    for bad in ((1, 100, 64), (1, 64, 8), (-1, 64, 64), (1, 0, 64), (1, 65536 + 16, 64), (1, 64, 65536 + 16)):
        assert size(*bad) == -1, bad
    ws = size(1, 64, 64)
    good = dict(n=1, H=64, W=64, rgb=4096, q=95, ws=1 << 16, wsb=ws, out=1 << 20)

    def call(**kw):
        a = dict(good, **kw)
        return rt(None, a["n"], a["H"], a["W"], a["rgb"], a["q"], a["ws"], a["wsb"], a["out"])

    for bad in (dict(n=-1), dict(H=60), dict(W=8), dict(H=0), dict(H=65536 + 16), dict(rgb=None), dict(rgb=4097), dict(ws=None),
                dict(ws=(1 << 16) + 8), dict(wsb=ws - 1), dict(out=None), dict(out=(1 << 20) + 4), dict(out=4096), dict(q=0),
                dict(q=101), dict(q=-5), dict(n=1 << 20, H=4096, W=4096, wsb=1 << 62)):
        assert call(**bad) == -1, bad
    assert call(n=0, wsb=0) == 0


class _Net:
    def __init__(self, nc):
        self.nc = nc


def _bare_generator(nc=3, max_res_log2=9, downscale=1):
    """An ImageGenerator with no device behind it: whatever touches the GPU fails with AttributeError."""
    from gan_segmentation_amd.image_generator import ImageGenerator
    gen = ImageGenerator.__new__(ImageGenerator)
    gen.max_res_log2, gen.output_downscale, gen.netG, gen._decoder = max_res_log2, downscale, _Net(nc), object()
    return gen


def test_training_batches_checks_jpeg_quality_at_the_call():
    for q in (95.0, "95", True, 0, 101, -1):
        with pytest.raises(ValueError, match="jpeg_quality"):
            _bare_generator(3).training_batches(4, jpeg_quality=q)
    for nc in (1, 4):
        with pytest.raises(ValueError, match="three image channels"):
            _bare_generator(nc).training_batches(4, mean=(0.5,) * nc, std=(1.0,) * nc, jpeg_quality=95)
    with pytest.raises(ValueError, match="multiple of 16"):
        _bare_generator(3, max_res_log2=5, downscale=4).training_batches(4, crop=None, jpeg_quality=95)      # 8 px pairs
    for kw in (dict(jpeg_quality=95), dict(jpeg_quality=np.int64(1)), dict(jpeg_quality=100), dict(jpeg_quality=None), dict()):
        stream = _bare_generator(3).training_batches(4, crop=480, num_samples=8, **kw)     # valid: nothing runs until the first next()
        with pytest.raises(AttributeError):
            next(stream)


def test_roundtrip_checks_its_tensor_before_any_gpu_work():
    import torch
    from gan_segmentation_amd import jpeg
    for img in (torch.zeros((1, 16, 16, 3), dtype=torch.uint8), torch.zeros((1, 16, 16, 3), dtype=torch.float32)):
        with pytest.raises(ValueError):
            jpeg.roundtrip(img)
    with pytest.raises(ValueError, match="quality"):
        jpeg.check_quality(0)
    assert jpeg.check_quality(np.int32(95)) == 95
