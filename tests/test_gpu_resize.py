"""The pair resize on the GPU (csrc/gsa_resize.hip, resize_ops.resize_pair, the OUTPUT_SIZE keys): every output
byte against tests/resize_ref.py, at the shapes at which the kernel can go wrong -- one pixel, an identity, odd sizes, sizes that
straddle the 32 x 8 output tiles and the staged chunks, the ratio limit, every channel count and both access forms -- and at the limits
the header documents."""
import numpy as np
import pytest

from gan_segmentation_amd import resize_ops
from tests import resize_ref as ref

pytestmark = pytest.mark.gpu


def _differ(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, "%s: %s %s instead of %s %s" % (what, got.dtype, got.shape, want.dtype, want.shape)
    bad = np.argwhere(got != want)
    assert not len(bad), "%s: %d of %d bytes differ from the rule, first at %s: %d instead of %d" % (
        what, len(bad), want.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


def _check(torch, img, mask, size, mode="vote", sums=ref.weighted_sums):
    """One call on the device; the inputs must come back unchanged and every output byte equal the rule."""
    d_img = None if img is None else torch.from_numpy(img).cuda()
    d_mask = None if mask is None else torch.from_numpy(mask).cuda()
    got_img, got_mask = resize_ops.resize_pair(d_img, d_mask, size, mode)
    what = "%s -> %s %s" % ((img if img is not None else mask).shape, size, mode)
    if img is None:
        assert got_img is None
    else:
        _differ(got_img.cpu().numpy(), ref.resize_image(img, size, sums=sums), what + ": image")
        assert np.array_equal(d_img.cpu().numpy(), img), what + ": the image was written to"
    if mask is None:
        assert got_mask is None
    else:
        _differ(got_mask.cpu().numpy(), ref.resize_mask(mask, size, mode, sums=sums), what + ": mask")
        assert np.array_equal(d_mask.cpu().numpy(), mask), what + ": the mask was written to"
    return got_img, got_mask


@pytest.mark.parametrize("shape,size", ref.SHAPES, ids=lambda s: "%dx%d" % s)
def test_shapes(torch_cuda, shape, size):
    H, W = shape
    img, mask = ref.random_pair(H + W, 2, H, W, 3)
    _check(torch_cuda, img, mask, size)
    _check(torch_cuda, img, mask, size, "nearest")


def test_a_batch_of_three_at_256_by_320(torch_cuda):
    img, mask = ref.random_pair(7, 3, 256, 320, 3)
    _check(torch_cuda, img, mask, (96, 112))
    _check(torch_cuda, img, mask, (96, 112), "nearest")


@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_channels_modes_and_every_mask_value(torch_cuda, C):
    """(33, 47) takes the byte form for every C but 4, (32, 48) the dword form for all; the masks hold all 256 values."""
    for (H, W), size in (((33, 47), (16, 16)), ((32, 48), (10, 13)), ((130, 259), (33, 65))):
        img = ref.random_pair(C, 2, H, W, C)[0]
        mask = ref.every_value_mask(C, 2, H, W)
        assert len(np.unique(mask)) == 256 or H * W < 4096
        _check(torch_cuda, img, mask, size)
        _check(torch_cuda, img, mask, size, "nearest")


def test_a_window_of_several_chunks(torch_cuda):
    """Ratio 16 on both axes with four channels: 2052 bytes a staged image row, 11 rows a chunk, 129 rows under a tile."""
    img, mask = ref.random_pair(4, 1, 144, 528, 4)
    _check(torch_cuda, img, mask, (9, 33))


def test_ties_by_hand(torch_cuda):
    for mask, size, want in ref.hand_cases():
        got = _check(torch_cuda, None, mask, size)[1]
        assert np.array_equal(got.cpu().numpy(), want)


def test_image_only_mask_only_and_out_views(torch_cuda):
    """The call forms: one half absent, and ``out=`` tensors that start 1, 2 and 3 bytes into a buffer -- and inputs that do."""
    torch = torch_cuda
    img, mask = ref.random_pair(5, 2, 40, 72, 3)
    size = (17, 30)
    want_img, want_mask = ref.resize_pair(img, mask, size)
    _check(torch, img, None, size)
    _check(torch, None, mask, size)
    _check(torch, None, mask, size, "nearest")
    d_img, d_mask = torch.from_numpy(img).cuda(), torch.from_numpy(mask).cuda()
    for off in (1, 2, 3):
        buf_i = torch.full((want_img.size + 8,), 0xA5, dtype=torch.uint8, device="cuda")
        buf_m = torch.full((want_mask.size + 8,), 0xA5, dtype=torch.uint8, device="cuda")
        out_i = buf_i[off:off + want_img.size].view(want_img.shape)
        out_m = buf_m[4 - off:4 - off + want_mask.size].view(want_mask.shape)
        got = resize_ops.resize_pair(d_img, d_mask, size, out=(out_i, out_m))
        assert got[0] is out_i and got[1] is out_m
        _differ(out_i.cpu().numpy(), want_img, "out= image at offset %d" % off)
        _differ(out_m.cpu().numpy(), want_mask, "out= mask at offset %d" % (4 - off))
        for buf, lo, size_ in ((buf_i, off, want_img.size), (buf_m, 4 - off, want_mask.size)):
            rest = torch.cat([buf[:lo], buf[lo + size_:]]).cpu().numpy()
            assert (rest == 0xA5).all(), "bytes outside the out= view were written"
        # inputs off their dwords: the byte form of the staging
        src_i = torch.empty((img.size + 8,), dtype=torch.uint8, device="cuda")
        src_m = torch.empty((mask.size + 8,), dtype=torch.uint8, device="cuda")
        in_i, in_m = src_i[off:off + img.size].view(img.shape), src_m[off:off + mask.size].view(mask.shape)
        in_i.copy_(d_img)
        in_m.copy_(d_mask)
        got = resize_ops.resize_pair(in_i, in_m, size)
        _differ(got[0].cpu().numpy(), want_img, "image input at offset %d" % off)
        _differ(got[1].cpu().numpy(), want_mask, "mask input at offset %d" % off)
    only = resize_ops.resize_pair(d_img, d_mask, size, out=(None, torch.empty(want_mask.shape, dtype=torch.uint8, device="cuda")))
    _differ(only[0].cpu().numpy(), want_img, "out=(None, mask_out)")
    for bad in ((d_img[:, :17, :30].contiguous()[:1], None), (None, d_mask), (torch.empty(want_img.shape, dtype=torch.uint8), None), "x",
                (torch.empty(want_mask.shape, dtype=torch.uint8, device="cuda"), None)):
        with pytest.raises(ValueError, match="out"):
            resize_ops.resize_pair(d_img, d_mask, size, out=bad)
    with pytest.raises(ValueError, match="out"):
        resize_ops.resize_pair(None, d_mask, size, out=(torch.empty(want_img.shape, dtype=torch.uint8, device="cuda"), None))
    empty = resize_ops.resize_pair(d_img[:0], d_mask[:0], size)
    assert empty[0].shape == (0, 17, 30, 3) and empty[1].shape == (0, 17, 30)


def test_a_sample_does_not_depend_on_its_batch(torch_cuda):
    torch = torch_cuda
    img, mask = ref.random_pair(8, 5, 61, 75, 3)
    d_img, d_mask = torch.from_numpy(img).cuda(), torch.from_numpy(mask).cuda()
    for mode in ("vote", "nearest"):
        all_i, all_m = resize_ops.resize_pair(d_img, d_mask, (23, 40), mode)
        for k in range(5):
            one_i, one_m = resize_ops.resize_pair(d_img[k:k + 1], d_mask[k:k + 1], (23, 40), mode)
            assert torch.equal(one_i[0], all_i[k]) and torch.equal(one_m[0], all_m[k]), "sample %d alone differs from its row of the batch" % k
    _differ(all_i.cpu().numpy(), ref.resize_image(img, (23, 40)), "batch of 5")


# ---- the limits the header documents ---------------------------------------------------------------------------------------------
def test_the_largest_plane_all_255_does_not_overflow(torch_cuda):
    """1 x 4096 x 4096 x 1, H * W = 2^24, ratio 16: every numerator is 255 * 2^24 + 2^23, the largest there is."""
    torch = torch_cuda
    img = torch.full((1, 4096, 4096, 1), 255, dtype=torch.uint8, device="cuda")
    mask = torch.full((1, 4096, 4096), 255, dtype=torch.uint8, device="cuda")
    out_i, out_m = resize_ops.resize_pair(img, mask, 256)
    assert out_i.shape == (1, 256, 256, 1) and out_m.shape == (1, 256, 256)
    assert bool((out_i == 255).all()) and bool((out_m == 255).all())
    mask.fill_(7)
    img.fill_(1)
    out_i, out_m = resize_ops.resize_pair(img, mask, 256)
    assert bool((out_i == 1).all()) and bool((out_m == 7).all())


@pytest.mark.parametrize("shape", [(4096, 4096), (16384, 1024), (2048, 8192)], ids=lambda s: "%dx%d" % s)
def test_an_identity_on_the_largest_plane(torch_cuda, shape):
    """H * W = h * w = 2^24: the weight of the one tap of every pixel is 2^24 itself, one more than a 24-bit factor holds.  The image
    bytes are non-zero and come back as they went in; so does the mask."""
    torch = torch_cuda
    H, W = shape
    gen = torch.Generator(device="cuda").manual_seed(H)
    img = torch.randint(1, 256, (1, H, W, 1), dtype=torch.uint8, device="cuda", generator=gen)
    mask = torch.randint(0, 8, (1, H, W), dtype=torch.uint8, device="cuda", generator=gen)
    out_i, out_m = resize_ops.resize_pair(img, mask, (H, W))
    assert int(img.min()) >= 1 and int(img.max()) == 255
    bad = int((out_i != img).sum())
    assert bad == 0, "%d of %d image bytes of the identity differ, first output byte %d for %d" % (bad, img.numel(), int(out_i.flatten()[0]), int(img.flatten()[0]))
    assert torch.equal(out_m, mask)
    # one axis an identity, the other halved: weights of 2^23, and the mean of two non-zero bytes
    half_i, _m = resize_ops.resize_pair(img, None, (H, W // 2))
    pairs = img.view(1, H, W // 2, 2).to(torch.int32).sum(dim=-1)
    assert torch.equal(half_i[..., 0], ((pairs + 1) // 2).to(torch.uint8))


def test_a_side_of_65535(torch_cuda):
    """65535 x 256 -> 4096 x 16: the longest side, H * W just below 2^24, ratio just below 16 on both axes; held to the prefix form
    of the rule, which tests/test_resize_host.py holds to the other two."""
    rng = np.random.default_rng(65535)
    H, W = 65535, 256
    img = rng.integers(0, 256, (1, H, W, 1)).astype(np.uint8)
    mask = np.repeat(rng.integers(0, 3, (1, H, W // 4)).astype(np.uint8), 4, axis=2)
    mask[mask == 2] = 255
    mask[:, ::7, ::5] = 1
    _check(torch_cuda, img, mask, (4096, 16), sums=ref.prefix_sums)


def test_refusals_write_nothing(torch_cuda):
    """A ratio above 16, an output that overlaps an input through views of one buffer, and a half-null pair: refused by the wrapper
    with ValueError and by the entry with GSA_ERR_INVALID, the outputs untouched."""
    torch = torch_cuda
    from gan_segmentation_amd import _lib
    from gan_segmentation_amd._runtime import current_stream_ptr
    fn = _lib.load_library().fn("gsa_pair_resize")
    stream = current_stream_ptr(torch.device("cuda", 0))
    buf = torch.full((65 * 64 * 3 + 65 * 64 + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
    img = buf[:65 * 64 * 3].view(1, 65, 64, 3)
    mask = buf[65 * 64 * 3:65 * 64 * 4].view(1, 65, 64)
    out_i = buf[65 * 64 * 4:65 * 64 * 4 + 48].view(1, 4, 4, 3)
    out_m = buf[65 * 64 * 4 + 48:65 * 64 * 4 + 64].view(1, 4, 4)
    with pytest.raises(ValueError, match="1/16"):
        resize_ops.resize_pair(img, mask, 4, out=(out_i, out_m))
    assert fn(stream, 1, 65, 64, 3, 4, 4, 0, img.data_ptr(), mask.data_ptr(), out_i.data_ptr(), out_m.data_ptr()) == -1
    # (64, 64) -> (4, 4) is in range: the output over the image's last bytes, over the mask's first, and over the other output
    img, mask = buf[:64 * 64 * 3].view(1, 64, 64, 3), buf[64 * 64 * 3:64 * 64 * 4].view(1, 64, 64)
    over_i = buf[64 * 64 * 3 - 1:64 * 64 * 3 + 47].view(1, 4, 4, 3)
    over_m = buf[64 * 64 * 3:64 * 64 * 3 + 16].view(1, 4, 4)
    far = 65 * 64 * 4
    for o_i, o_m in ((over_i, out_m), (out_i, over_m), (out_i, buf[far + 47:far + 63].view(1, 4, 4))):
        with pytest.raises(ValueError, match="overlap"):
            resize_ops.resize_pair(img, mask, 4, out=(o_i, o_m))
        assert fn(stream, 1, 64, 64, 3, 4, 4, 0, img.data_ptr(), mask.data_ptr(), o_i.data_ptr(), o_m.data_ptr()) == -1
    for args in ((None, mask.data_ptr(), out_i.data_ptr(), out_m.data_ptr()), (img.data_ptr(), mask.data_ptr(), None, out_m.data_ptr()),
                 (img.data_ptr(), None, out_i.data_ptr(), out_m.data_ptr()), (img.data_ptr(), mask.data_ptr(), out_i.data_ptr(), None),
                 (None, None, None, None)):
        assert fn(stream, 1, 64, 64, 3, 4, 4, 0, *args) == -1
    torch.cuda.synchronize()
    assert bool((buf == 0xA5).all()), "a refused call wrote something"


# ---- generate ----------------------------------------------------------------------------------------------------------------------
def test_cli_output_size_key(torch_cuda, tmp_path):
    """OUTPUT_DOWNSCALE: 2 then OUTPUT_SIZE: 48 on bedrooms (256 -> 128 -> 48 px), with PAIR_STATS: every mask file decodes to
    resize_pair of the run's own generate_indexed pair, every image file to the JPEG round trip of the resized image (what
    tests/test_gpu_jpeg_roundtrip.py shows a written file decodes to), and the statistics rows are those of the resized pairs."""
    pytest.importorskip("PIL.features")
    from PIL import Image
    from gan_segmentation_amd import jpeg, pair_stats
    from tests.test_gpu_downscale import _build, _cli_dirs
    torch = torch_cuda
    gcfg, gp, dcfg, dp, run = _cli_dirs(tmp_path, "resized")
    base = run(OUTPUT_DOWNSCALE=2, OUTPUT_SIZE=48, PAIR_STATS=True)
    out = base / "dataset" / "train_generated"
    gen = _build(gcfg, gp, dcfg, dp, 2, output_downscale=2)
    pairs = [gen.generate_indexed(0, 2), gen.generate_indexed(2, 1)]
    assert tuple(pairs[0][0].shape) == (2, 128, 128, 3)
    img = torch.cat([resize_ops.resize_pair(i, m, 48)[0] for i, m in pairs])
    mask = torch.cat([resize_ops.resize_pair(i, m, 48)[1] for i, m in pairs])
    _differ(mask.cpu().numpy(), ref.resize_mask(torch.cat([m for _i, m in pairs]).cpu().numpy(), (48, 48)), "the resized masks")
    _differ(img.cpu().numpy(), ref.resize_image(torch.cat([i for i, _m in pairs]).cpu().numpy(), (48, 48)), "the resized images")
    decoded = jpeg.roundtrip(img).cpu().numpy()
    for k in range(3):
        _differ(np.asarray(Image.open(out / ("mask_%06d.png" % k))), mask[k].cpu().numpy(), "mask_%06d.png" % k)
        im = Image.open(out / ("img_%06d.jpg" % k))
        assert im.size == (48, 48) and im.mode == "RGB"
        _differ(np.asarray(im.convert("RGB")), decoded[k], "img_%06d.jpg" % k)
    index, rows, H, W, C = pair_stats.merge_shards(str(out))
    assert (H, W, C) == (48, 48, 3) and index.tolist() == [0, 1, 2]
    _differ(rows, pair_stats.pair_stats(img, mask).cpu().numpy(), "pair_stats rows")
    assert sorted(p.name for p in out.iterdir() if not p.name.endswith(".npz")) == sorted(
        ["img_%06d.jpg" % k for k in range(3)] + ["mask_%06d.png" % k for k in range(3)])



def test_cli_output_size_nearest_and_a_rectangle(torch_cuda, tmp_path):
    """OUTPUT_SIZE: [48, 64] with OUTPUT_MASK_RESIZE: nearest: 48 rows of 64 pixels, the masks sampled, not voted."""
    from PIL import Image
    from tests.test_gpu_downscale import _build, _cli_dirs
    torch = torch_cuda
    gcfg, gp, dcfg, dp, run = _cli_dirs(tmp_path, "nearest")
    out = run(OUTPUT_DOWNSCALE=2, OUTPUT_SIZE=[48, 64], OUTPUT_MASK_RESIZE="nearest") / "dataset" / "train_generated"
    gen = _build(gcfg, gp, dcfg, dp, 2, output_downscale=2)
    masks = torch.cat([gen.generate_indexed(0, 2)[1], gen.generate_indexed(2, 1)[1]])
    near = resize_ops.resize_pair(None, masks, (48, 64), "nearest")[1].cpu().numpy()
    _differ(near, ref.resize_mask(masks.cpu().numpy(), (48, 64), "nearest"), "the sampled masks")
    for k in range(3):
        _differ(np.asarray(Image.open(out / ("mask_%06d.png" % k))), near[k], "nearest mask_%06d.png" % k)
        assert Image.open(out / ("img_%06d.jpg" % k)).size == (64, 48)
