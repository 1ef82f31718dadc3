"""The mask clean-up on the GPU (include/gsa_mask.h gsa_mask_morph; mask_ops.morph_mask; ImageGenerator(mask_morph=True); the
MASK_MORPH key): bit for bit the rule of tests/test_mask_morph_host.py, over ALL pixels -- nothing is excluded."""
import os

import numpy as np
import pytest

from tests.test_gpu_augment import _build, _host, _same_bits
from tests.test_mask_morph_host import KINDS, RANDOM_KINDS, SEAM_SHAPES, SMALL_SHAPES, blobs, make, rule_morph

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The tile of csrc/gsa_mask.hip: the seam shapes below are chosen for it (asserted against the source text).
TILE_W = TILE_H = 64


def _morph(torch, m, **kw):
    from gan_segmentation_amd import mask_ops
    d = torch.from_numpy(m).cuda()
    out = mask_ops.morph_mask(d, **kw)
    assert out.shape == d.shape and out.dtype == torch.uint8 and out.is_contiguous() and out.data_ptr() != d.data_ptr()
    got = out.cpu().numpy()
    assert np.array_equal(d.cpu().numpy(), m), "the input was written to"
    return got


def _check(torch, m, what):
    got, want = _morph(torch, m), rule_morph(m)
    bad = got != want
    assert not bad.any(), "%s %s: %d of %d bytes differ from the rule, first at %s" % (
        what, m.shape, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]))
    return got


def _check_all_kinds(torch, shape):
    """Every input kind at one shape against the rule.  From 16 px on, every random kind must also be CHANGED by the rule (a copy
    kernel cannot pass); below that a window covers most of the image and the rule may well return a random input as it is
    (tests/test_mask_morph_host.py::test_every_random_input_is_changed_by_the_rule holds the same line on the CPU)."""
    for kind in KINDS:
        m = make(kind, sum(shape), shape)
        got = _check(torch, m, kind)
        if kind in RANDOM_KINDS and min(shape[1:]) >= 16:
            assert not np.array_equal(got, m), "%s %s: the rule changed nothing, a copy would pass" % (kind, shape)


@pytest.mark.parametrize("shape", SMALL_SHAPES)
def test_shapes_smaller_than_the_apron(torch_cuda, shape):
    """Both sides of the image clip inside one apron; odd widths take the byte-wise path, (2, 16, 16) the dword path."""
    _check_all_kinds(torch_cuda, shape)


def test_the_tile_is_the_one_these_tests_assume():
    src = open(os.path.join(ROOT, "gan-segmentation_amd", "csrc", "gsa_mask.hip")).read()
    assert "constexpr int kTileW = %d;" % TILE_W in src and "constexpr int kTileH = %d;" % TILE_H in src
    assert "const dim3 grid((unsigned)(tiles_per_plane * n)), block(kThreads);" in src      # one workgroup per tile: no grid cap to cross
    for _n, H, W in SEAM_SHAPES[:1]:
        assert H // TILE_H >= 2 and H % TILE_H and W // TILE_W >= 2 and W % TILE_W      # two full tiles and a partial one each way
    assert any(W % 4 for _n, _H, W in SEAM_SHAPES) and any(W % 4 == 0 for _n, _H, W in SEAM_SHAPES)      # both access paths


@pytest.mark.parametrize("shape", SEAM_SHAPES + [(2, 64, 128)])
def test_tile_seams(torch_cuda, shape):
    """(1, 200, 328): 3 full tiles and one of 8 rows down, 5 and one of 8 columns across; (1, 40, 56): less than one tile;
    (1, 130, 70): a 2-row and a 6-column remainder and a width that is no multiple of 4; (2, 64, 128): whole tiles only."""
    _check_all_kinds(torch_cuda, shape)


def test_a_view_that_is_not_dword_aligned(torch_cuda):
    """Planes of 15 x 20 = 300 bytes behind a 1-byte offset: W is a multiple of 4 but the pointers are not aligned."""
    from gan_segmentation_amd import mask_ops
    torch = torch_cuda
    m = make("blobs", 7, (3, 15, 20))
    buf = torch.zeros(1 + m.size, dtype=torch.uint8, device="cuda")
    d = buf[1:].view(3, 15, 20)
    d.copy_(torch.from_numpy(m))
    assert d.data_ptr() % 4 == 1
    assert np.array_equal(mask_ops.morph_mask(d).cpu().numpy(), rule_morph(m))
    obuf = torch.full((3 + m.size,), 77, dtype=torch.uint8, device="cuda")
    out = obuf[3:].view(3, 15, 20)
    mask_ops.morph_mask(d, out=out)
    assert np.array_equal(out.cpu().numpy(), rule_morph(m)) and (obuf[:3] == 77).all()


def test_images_of_a_batch_do_not_leak_into_each_other(torch_cuda):
    """n = 3 at 32 x 32, [all 1, all 0, blobs]: smaller than a tile, so the apron of every image lies over its neighbours' memory."""
    batch = np.stack([np.ones((32, 32), np.uint8), np.zeros((32, 32), np.uint8), blobs(5, (32, 32))])
    got = _check(torch_cuda, batch, "batch")
    for k in range(3):
        alone = _morph(torch_cuda, batch[k:k + 1])
        assert np.array_equal(got[k], alone[0]), "image %d of the batch differs from image %d alone" % (k, k)
    assert got[0].all() and not got[1].any(), "the constants did not stay constant"
    assert not np.array_equal(got[2], batch[2])


def test_two_dimensional_input_out_argument_and_the_empty_batch(torch_cuda):
    from gan_segmentation_amd import mask_ops
    torch = torch_cuda
    m = make("blobs", 11, (2, 40, 56))
    d = torch.from_numpy(m).cuda()
    out = torch.empty_like(d)
    assert mask_ops.morph_mask(d, out=out) is out
    assert np.array_equal(out.cpu().numpy(), rule_morph(m)) and np.array_equal(d.cpu().numpy(), m)
    plane = mask_ops.morph_mask(d[1])
    assert plane.shape == (40, 56) and np.array_equal(plane.cpu().numpy(), rule_morph(m[1]))
    empty = mask_ops.morph_mask(d[:0])
    assert empty.shape == (0, 40, 56) and empty.dtype == torch.uint8


def test_value_errors(torch_cuda):
    from gan_segmentation_amd import mask_ops
    torch = torch_cuda
    d = torch.from_numpy(make("half", 1, (2, 16, 16))).cuda()
    flat = torch.zeros(3 * 16 * 16, dtype=torch.uint8, device="cuda")
    a, b = flat[:2 * 256].view(2, 16, 16), flat[256:].view(2, 16, 16)       # two overlapping views of one buffer
    for bad in (dict(mask=d.float()), dict(mask=d[:, :, ::2]), dict(mask=d.cpu()), dict(mask=d, out=d), dict(mask=a, out=b),
                dict(mask=b, out=a), dict(mask=d, out=torch.empty_like(d)[:1]), dict(mask=d, out=torch.empty_like(d).float()),
                dict(mask=d, out=torch.empty_like(d).cpu()), dict(mask=d.view(1, 2, 16, 16))):
        with pytest.raises(ValueError):
            mask_ops.morph_mask(**bad)


# ---- the generator -----------------------------------------------------------------------------------------------------------
# The reduced synthetic generator of the augment tests (128 px pairs).  Its decoder's masks are almost all foreground with a few
# specks: these tests prove the plumbing -- that the rule runs, on the right tensor, at the right place; the kernel's correctness
# rests on the direct cases above.
def _pair(t):
    return t[0].cpu().numpy(), t[1].cpu().numpy()


def _check_plumbing(raw, cleaned, what):
    (img0, mask0), (img1, mask1) = raw, cleaned
    assert np.array_equal(img1, img0), "%s: mask_morph changed the image" % what
    want = rule_morph(mask0)
    assert not np.array_equal(want, mask0), "%s: the rule leaves the raw mask as it is, the case proves nothing" % what
    assert np.array_equal(mask1, want), "%s: %d mask bytes differ from the rule on the raw mask" % (what, int((mask1 != want).sum()))


@pytest.mark.parametrize("kw", [dict(), dict(output_downscale=2), dict(style_mix_prob=1.0)], ids=["plain", "downscale2", "mixed"])
def test_generate_indexed_returns_the_rule_on_the_raw_mask(torch_cuda, kw):
    plain, morph = _build("reduced", 3, **kw), _build("reduced", 3, mask_morph=True, **kw)
    for first, n in ((10, 3), (13, 2)):
        _check_plumbing(_pair(plain.generate_indexed(first, n, seed=4)), _pair(morph.generate_indexed(first, n, seed=4)),
                        "samples %d..%d" % (first, first + n - 1))
    assert morph.generate_indexed(10, 3, seed=4)[1].shape[1] == 128 // kw.get("output_downscale", 1)


def test_out_receives_the_cleaned_mask(torch_cuda):
    torch = torch_cuda
    plain, morph = _build("reduced", 3), _build("reduced", 3, mask_morph=True)
    img = torch.empty((3, 128, 128, 3), dtype=torch.uint8, device="cuda")
    mask = torch.full((3, 128, 128), 9, dtype=torch.uint8, device="cuda")
    got = morph.generate_indexed(20, 3, seed=4, out=(img, mask))
    assert got[0] is img and got[1] is mask
    _check_plumbing(_pair(plain.generate_indexed(20, 3, seed=4)), _pair((img, mask)), "out=")


def test_generate_batch_and_batch_w_get_it_too(torch_cuda):
    plain, morph = _build("reduced", 3), _build("reduced", 3, mask_morph=True)
    z, noise = plain.netG.draw_indexed(30, 3, 4)
    _check_plumbing(_pair(plain.generate_batch(z, noise)), _pair(morph.generate_batch(z, noise)), "generate_batch")
    dl = plain.netG.mapping(z)[:, None, :].repeat(1, plain.netG.num_style_layers, 1).contiguous()
    _check_plumbing(_pair(plain.generate_batch_w(dl, noise)), _pair(morph.generate_batch_w(dl, noise)), "generate_batch_w")


def test_replayed_graph_keeps_writing_the_scratch_mask(torch_cuda):
    """graph_mode "1", captured at the second call: four identical calls into preallocated outputs, every one the rule on the raw
    mask -- the eager morph launch behind a replayed graph reads what the graph wrote."""
    torch = torch_cuda
    plain, morph = _build("reduced", 3), _build("reduced", 3, mask_morph=True)
    morph.graph_mode, morph.graph_after = "1", 2
    z, noise = plain.netG.draw_indexed(40, 3, 4)
    raw = _pair(plain.generate_batch(z, noise))
    img = torch.empty((3, 128, 128, 3), dtype=torch.uint8, device="cuda")
    mask = torch.empty((3, 128, 128), dtype=torch.uint8, device="cuda")
    for call in range(4):
        img.fill_(3)
        mask.fill_(9)
        morph.generate_batch(z, noise, out=(img, mask))
        _check_plumbing(raw, _pair((img, mask)), "call %d" % call)
    assert morph.graphs_captured() >= 1


def test_training_batches_warp_the_cleaned_mask(torch_cuda):
    from gan_segmentation_amd import augment
    plain, morph = _build("reduced", 3), _build("reduced", 3, mask_morph=True)
    kw = dict(crop=96, seed=4, first_index=10, num_samples=5)
    a = [(_host(image, label), first) for image, label, first in plain.training_batches(3, **kw)]
    b = [(_host(image, label), first) for image, label, first in morph.training_batches(3, **kw)]
    assert [f for _, f in a] == [f for _, f in b] == [10, 13]
    changed = 0
    for ((image0, _label0), first), ((image1, label1), _f) in zip(a, b):
        n = min(3, 15 - first)
        _same_bits(image1, image0, "image of batch %d" % first)
        img, mask = plain.generate_indexed(first, n, seed=4)
        want = rule_morph(mask.cpu().numpy())
        changed += int((want != mask.cpu().numpy()).sum())
        matrices = augment.plan_matrices(4, first, n, 128, 128, 96, "train")
        cleaned = torch_cuda.from_numpy(want).cuda()
        _image, label = augment.augment_pairs(img, cleaned, matrices, augment.output_size(128, 128, 96))
        _same_bits(label1, label.cpu().numpy(), "label of batch %d" % first)
    assert changed > 0, "the rule changed no raw mask"


# ---- the CLI -----------------------------------------------------------------------------------------------------------------
def test_cli_mask_morph_key(torch_cuda, tmp_path):
    """MASK_MORPH: true on bedrooms (3 samples): every mask_*.png is the rule on the mask of a MASK_MORPH: false run, every img_*.jpg
    the same bytes."""
    from PIL import Image
    from tests.test_gpu_downscale import _cli_dirs
    runs = {}
    for name, keys in (("off", dict(MASK_MORPH=False)), ("on", dict(MASK_MORPH=True))):
        _gcfg, _gp, _dcfg, _dp, run = _cli_dirs(tmp_path, name)
        runs[name] = run(**keys) / "dataset" / "train_generated"
        assert len(list(runs[name].iterdir())) == 6
    changed = 0
    for i in range(3):
        assert (runs["on"] / ("img_%06d.jpg" % i)).read_bytes() == (runs["off"] / ("img_%06d.jpg" % i)).read_bytes()
        raw = np.asarray(Image.open(runs["off"] / ("mask_%06d.png" % i)))
        got = np.asarray(Image.open(runs["on"] / ("mask_%06d.png" % i)))
        assert raw.shape == (256, 256) and np.array_equal(got, rule_morph(raw)), "mask %d" % i
        changed += int((got != raw).sum())
    assert changed > 0, "the rule changed no mask: the run proves nothing"
