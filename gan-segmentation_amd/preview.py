"""ctypes binding of the on-device pair previews (csrc/gsa_overlay.h, csrc/gsa_overlay.hip) -- the
counterpart of reference utils.get_draw_mask (utils.py:69-102), which tints an image with the class colours of its mask and which
the reference's annotator shows after every epoch and saves as ``vis_img_%06d.jpg`` beside every sample.

``overlay(img, mask)`` blends the class colours of ``mask`` over ``img`` on the GPU -- for ``alpha = k/128`` bit for bit what
``get_draw_mask`` returns -- with another weight on the class outlines and an optional f x f box thumbnail;
``contact_sheet(img, mask, cols)`` lays the thumbnails of a batch out as one image.  Both enqueue one kernel (two for a sheet with
empty cells) on the current stream of the tensors' device.  No CPU fallback.  ``make_lut`` builds the (256, 6) table the kernel
reads: per mask value a colour, a weight for the inside of a region and one for its outline.

``write_previews`` is what ``generate``'s ``PREVIEW_EVERY`` key calls.  ``python -m gan_segmentation_amd.preview DIR`` makes
contact sheets of a written dataset from its ``img_%06d.jpg`` / ``mask_%06d.png`` files: it does not depend on how many ranks wrote
them."""
import argparse
import os
import sys

import numpy as np

FACTORS = (1, 2, 4, 8, 16)
MAX_EXTENT = 65535
FULL_WEIGHT = 128           # the weights of a table row are in 1/128

# mask value -> colour, in the image's channel order.  The reference's map (utils.get_seg_color_map): background, foreground, negative.
REFERENCE_COLOURS = {0: (0, 0, 0), 1: (13, 198, 20), 2: (54, 30, 211)}
# the same, with colours for the classes 3..7 of the larger decoders and a grey for 255, so that an ignore band shows
DATASET_COLOURS = {**REFERENCE_COLOURS, 3: (255, 176, 0), 4: (0, 190, 255), 5: (255, 64, 160), 6: (150, 90, 255), 7: (255, 255, 64),
                   255: (128, 128, 128)}


def _weight(v, what):
    """A blend weight in [0, 1] that is a multiple of 1/128 -> its numerator 0..128.  ValueError otherwise."""
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
        raise ValueError("%s must be a multiple of 1/128 in [0, 1], got %r" % (what, v))
    k = float(v) * FULL_WEIGHT
    if not 0 <= k <= FULL_WEIGHT or k != int(k):
        raise ValueError("%s must be a multiple of 1/128 in [0, 1] (the blend is (k*c + (128-k)*p) >> 7), got %r" % (what, v))
    return int(k)


def make_lut(colours=None, alpha=0.5, skip_background=True, outline=None):
    """The (256, 6) uint8 table of ``overlay``: row v = ``c0 c1 c2 c3 w_in w_edge`` for mask value v.  ``colours``: {value: colour of
    1 to 4 components} (default ``REFERENCE_COLOURS``; a missing component is 255); ``alpha``: the weight of the colour inside a
    region; ``outline``: the weight on edge pixels (``None``: as inside); both multiples of 1/128 in [0, 1], ValueError otherwise.
    ``skip_background`` leaves value 0 without a colour, as the reference does.  A value without a colour keeps both weights 0: its
    pixels, outline included, are the image's."""
    w_in = _weight(alpha, "alpha")
    w_edge = w_in if outline is None else _weight(outline, "outline")
    lut = np.zeros((256, 6), np.uint8)
    for value, colour in (REFERENCE_COLOURS if colours is None else colours).items():
        colour = tuple(colour)
        if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not 0 <= int(value) <= 255:
            raise ValueError("a mask value must be an int in 0..255, got %r" % (value,))
        if not 1 <= len(colour) <= 4 or any(isinstance(c, bool) or not isinstance(c, (int, np.integer)) or not 0 <= int(c) <= 255 for c in colour):
            raise ValueError("a colour is 1 to 4 ints in 0..255, got %r for value %d" % (colour, value))
        if int(value) == 0 and skip_background:
            continue
        lut[int(value)] = colour + (255,) * (4 - len(colour)) + (w_in, w_edge)
    return lut


_device_luts = {}


def _lut_on(lut, device):
    """``lut`` as a (256, 6) uint8 tensor on ``device``: a device tensor is checked, a numpy table is uploaded once per device."""
    import torch
    from ._runtime import is_device_tensor
    if isinstance(lut, torch.Tensor):
        if not is_device_tensor(lut, torch.uint8, shape=(256, 6), device=device):
            raise ValueError("lut must be a contiguous uint8 tensor (256, 6) on %s" % (device,))
        return lut
    table = np.ascontiguousarray(make_lut() if lut is None else lut)
    if table.shape != (256, 6) or table.dtype != np.uint8:
        raise ValueError("lut must be a (256, 6) uint8 table (make_lut), got %s %s" % (table.shape, table.dtype))
    key = (str(device), table.tobytes())
    if key not in _device_luts:
        _device_luts[key] = torch.from_numpy(table.copy()).to(device)
    return _device_luts[key]


def check_factor(v, what="factor"):
    """A thumbnail factor as an int: 1, 2, 4, 8 or 16.  ValueError otherwise; a bool is not a number here."""
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or int(v) not in FACTORS:
        raise ValueError("%s must be 1, 2, 4, 8 or 16, got %r" % (what, v))
    return int(v)


def check_preview_every(v):
    """The PREVIEW_EVERY key as an int >= 0, 0 meaning off.  ValueError otherwise."""
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or int(v) < 0:
        raise ValueError("PREVIEW_EVERY must be an int >= 0, got %r" % (v,))
    return int(v)


def check_preview_downscale(v):
    """The PREVIEW_DOWNSCALE key as an int: 1, 2, 4, 8 or 16.  ValueError otherwise."""
    return check_factor(v, "PREVIEW_DOWNSCALE")


def sheet_shape(n, H, W, C, cols, factor):
    """The shape of the sheet of n samples: (ceil(n / cols) * H/factor, cols * W/factor, C)."""
    return (-(-n // cols) * (H // factor), cols * (W // factor), C)


def _sheet(img, mask, cols, lut, factor, out, who):
    """The checked call: img (n, H, W, C), mask (n, H, W) -> the sheet of ``sheet_shape`` (new, or ``out`` viewed as it)."""
    import torch
    from ._runtime import is_device_tensor, launch
    n, H, W, C = img.shape
    factor = check_factor(factor)
    if isinstance(cols, bool) or not isinstance(cols, (int, np.integer)) or int(cols) < 1:
        raise ValueError("cols must be an int >= 1, got %r" % (cols,))
    if not 1 <= C <= 4:
        raise ValueError("%s takes images of 1 to 4 channels, got %d" % (who, C))
    if not 1 <= H <= MAX_EXTENT or not 1 <= W <= MAX_EXTENT or H * W >= 2 ** 31:
        raise ValueError("%s takes planes whose sides are 1..%d px with fewer than 2^31 pixels, got %dx%d" % (who, MAX_EXTENT, H, W))
    if H % factor or W % factor:
        raise ValueError("factor %d does not divide %dx%d" % (factor, H, W))
    shape = sheet_shape(n, H, W, C, int(cols), factor)
    if shape[0] * shape[1] * C >= 2 ** 31:
        raise ValueError("a sheet holds fewer than 2^31 bytes, got %s" % (shape,))
    dev = img.device
    table = _lut_on(lut, dev)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=dev)
    else:
        if not is_device_tensor(out, torch.uint8, device=dev) or out.numel() != shape[0] * shape[1] * C:
            raise ValueError("out must be a contiguous uint8 tensor of %d bytes on %s" % (shape[0] * shape[1] * C, dev))
        for t, what in ((img, "img"), (mask, "mask"), (table, "lut")):
            a, b = out.data_ptr(), t.data_ptr()
            if out.numel() and t.numel() and a < b + t.numel() and b < a + out.numel():
                raise ValueError("out must not be, or overlap, %s" % what)
    if n:
        launch("gsa_overlay", dev, n, H, W, C, img.data_ptr(), mask.data_ptr(), table.data_ptr(), factor, int(cols), out.data_ptr())
    return out


def _pair(img, mask, who):
    """img (n, H, W, C) or (H, W, C), mask (n, H, W) or (H, W), both contiguous uint8 CUDA tensors on one device -> the 4-D and 3-D
    views and whether the caller passed a single sample."""
    import torch
    from ._runtime import is_device_tensor
    if not is_device_tensor(img, torch.uint8, dims=(3, 4)):
        raise ValueError("img must be a contiguous uint8 CUDA tensor (H, W, C) or (n, H, W, C)")
    if not is_device_tensor(mask, torch.uint8, shape=tuple(img.shape[:-1]), device=img.device):
        raise ValueError("mask must be a contiguous uint8 tensor %s on %s for %s" % (tuple(img.shape[:-1]), img.device, who))
    single = img.dim() == 3
    return (img[None], mask[None], True) if single else (img, mask, False)


def overlay(img, mask, lut=None, factor=1, out=None):
    """img (n, H, W, C) or (H, W, C) contiguous uint8 CUDA tensor with C in 1..4, mask (n, H, W) or (H, W) contiguous uint8 on the same
    device, H and W in 1..65535 and multiples of ``factor`` (1, 2, 4, 8 or 16) -> the overlays (n, H/factor, W/factor, C) (or without
    n; new, or ``out``, a contiguous uint8 tensor of that many bytes that overlaps no input): every pixel blended with the colour of
    its mask value by the weights of ``lut`` -- a ``make_lut`` table (numpy: uploaded once and cached per device; ``None``:
    ``make_lut()``, the reference's overlay) or a (256, 6) uint8 tensor on the device -- edge pixels by the outline weight, then
    box-filtered by ``factor`` (the rule of csrc/gsa_overlay.h).  Enqueued on the current stream of ``img``'s device; the inputs are
    not written.  ValueError on anything else; no CPU fallback."""
    img4, mask3, single = _pair(img, mask, "overlay")
    n, H, W, C = img4.shape
    sheet = _sheet(img4, mask3, 1, lut, factor, out, "overlay")
    factor = int(factor)
    return sheet.view((H // factor, W // factor, C) if single else (n, H // factor, W // factor, C))


def contact_sheet(img, mask, cols, lut=None, factor=4, out=None):
    """The thumbnails of ``overlay(img, mask, lut, factor)`` as ONE image (ceil(n / cols) * H/factor, cols * W/factor, C): sample i in
    the cell at row ``i // cols``, column ``i % cols``, cells without a sample 0; every byte is written.  Arguments and conventions
    as ``overlay``."""
    img4, mask3, _single = _pair(img, mask, "contact_sheet")
    sheet = _sheet(img4, mask3, cols, lut, factor, out, "contact_sheet")
    return sheet.view(sheet_shape(img4.shape[0], img4.shape[1], img4.shape[2], img4.shape[3], int(cols), int(factor)))


def save_jpeg(path, array):
    """array (H, W, 1 or 3) u8 -> a JPEG at quality 95 (PIL)."""
    from PIL import Image
    array = np.ascontiguousarray(array)
    if array.ndim != 3 or array.shape[-1] not in (1, 3):
        raise ValueError("a preview file takes 1 or 3 channels, got %s" % (array.shape,))
    Image.fromarray(array[..., 0] if array.shape[-1] == 1 else array, "L" if array.shape[-1] == 1 else "RGB").save(path, quality=95)


def preview_indices(first_index, n, every):
    """The positions i in a batch of n samples from global index ``first_index`` whose index is a multiple of ``every`` (none if 0)."""
    return [i for i in range(n) if every > 0 and (first_index + i) % every == 0]


_generate_lut = None


def write_previews(dst_dir, img, mask, first_index, every, factor=1, lut=None):
    """``vis_%06d.jpg`` in ``dst_dir`` for every sample of the batch img (n, H, W, C), mask (n, H, W) (device tensors, the pair as
    written) whose global index ``first_index + i`` is a multiple of ``every``: the overlay in ``DATASET_COLOURS`` at alpha 0.5 with a
    solid outline (or ``lut``), box-filtered by ``factor``.  The samples are selected on the device, overlaid on the current stream
    and copied to the host; which files exist depends on the indices only.  -> the paths written."""
    import torch
    global _generate_lut
    picks = preview_indices(int(first_index), int(img.shape[0]), every)
    if not picks:
        return []
    if lut is None:
        if _generate_lut is None:
            _generate_lut = make_lut(DATASET_COLOURS, alpha=0.5, outline=1.0)
        lut = _generate_lut
    if len(picks) == img.shape[0]:
        sel_img, sel_mask = img, mask
    else:
        at = torch.tensor(picks, dtype=torch.int64, device=img.device)
        sel_img, sel_mask = img.index_select(0, at), mask.index_select(0, at)
    host = overlay(sel_img.contiguous(), sel_mask.contiguous(), lut, factor).cpu().numpy()
    paths = []
    for k, i in enumerate(picks):
        paths.append(os.path.join(dst_dir, "vis_%06d.jpg" % (first_index + i)))
        save_jpeg(paths[-1], host[k])
    return paths


# ---- the command-line tool -------------------------------------------------------------------------------------------------------
def _sheet_on_device(imgs, masks, cols, lut, factor):
    """imgs (n, H, W, C), masks (n, H, W) host arrays -> the sheet as a host array, made on cuda:0."""
    import torch
    from ._runtime import require_gpu
    require_gpu()
    dev = torch.device("cuda", 0)
    return contact_sheet(torch.from_numpy(imgs).to(dev), torch.from_numpy(masks).to(dev), cols, lut, factor).cpu().numpy()


def _read_pair(directory, index):
    from PIL import Image
    img = np.asarray(Image.open(os.path.join(directory, "img_%06d.jpg" % index)))
    mask = np.asarray(Image.open(os.path.join(directory, "mask_%06d.png" % index)))
    if img.ndim == 2:
        img = img[..., None]
    if mask.ndim != 2 or mask.dtype != np.uint8 or img.dtype != np.uint8 or img.shape[:2] != mask.shape:
        raise ValueError("sample %d: a u8 image and a single-channel u8 mask of one size expected, got %s %s and %s %s"
                         % (index, img.shape, img.dtype, mask.shape, mask.dtype))
    return img, mask


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m gan_segmentation_amd.preview",
                                 description="contact sheets (preview_sheet_%06d.jpg, named by their first sample) of a written dataset")
    ap.add_argument("directory", help="the directory that holds img_%%06d.jpg and mask_%%06d.png")
    ap.add_argument("--cols", type=int, default=8, help="cells per row; a sheet holds cols * cols samples")
    ap.add_argument("--downscale", type=int, default=8, help="thumbnail factor: 1, 2, 4, 8 or 16")
    ap.add_argument("--first", type=int, default=0, help="first sample index")
    ap.add_argument("--count", type=int, default=64, help="number of samples")
    ap.add_argument("--alpha", type=float, default=0.5, help="weight of the class colour, a multiple of 1/128")
    ap.add_argument("--outline", type=float, default=1.0, help="weight on the class outlines, a multiple of 1/128")
    args = ap.parse_args(argv)
    try:
        factor = check_factor(args.downscale, "--downscale")
        if args.cols < 1 or args.first < 0 or args.count < 1:
            raise ValueError("--cols and --count must be at least 1 and --first at least 0")
        lut = make_lut(DATASET_COLOURS, alpha=args.alpha, outline=args.outline)
    except ValueError as e:
        print("preview: %s" % e, file=sys.stderr)
        return 2
    written = 0
    index, last = args.first, args.first + args.count
    while index < last:
        pairs = []
        while index + len(pairs) < min(last, index + args.cols * args.cols) and all(
                os.path.exists(os.path.join(args.directory, name % (index + len(pairs)))) for name in ("img_%06d.jpg", "mask_%06d.png")):
            pairs.append(_read_pair(args.directory, index + len(pairs)))
        if not pairs:
            break
        if len({p[0].shape for p in pairs}) != 1:
            print("preview: the samples from %d on differ in size" % index, file=sys.stderr)
            return 1
        sheet = _sheet_on_device(np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs]), args.cols, lut, factor)
        path = os.path.join(args.directory, "preview_sheet_%06d.jpg" % index)
        save_jpeg(path, sheet)
        print("%s: samples %d..%d" % (path, index, index + len(pairs) - 1))
        written += 1
        if len(pairs) < args.cols * args.cols:
            break                               # the dataset, or the range, ends here
        index += len(pairs)
    if not written:
        print("preview: no img_%06d.jpg / mask_%06d.png pair in %s" % (args.first, args.first, args.directory), file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
