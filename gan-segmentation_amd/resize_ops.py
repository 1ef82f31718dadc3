"""ctypes binding of the on-device pair resize (csrc/gsa_resize.h, csrc/gsa_resize.hip) -- the counterpart of the
``cv2.resize`` calls in the reference's dataset loaders, which resize every sample on the host: a uint8 image batch and / or a uint8
mask batch shrunk to any smaller-or-equal size.  The image takes the exact area mean of the source pixels an output pixel covers;
the mask takes the value that covers the largest area ("vote") or the pixel at ``floor(i * H / h), floor(j * W / w)`` ("nearest",
the index rule of ``cv2.INTER_NEAREST``).

``resize_pair(img, mask, size)`` enqueues one kernel on the current stream of the tensors' device.  Every byte is specified by the
rule in the header, in integers; a sample's result does not depend on the batch it is in.  ``generate`` applies it to every pair with
the config key ``OUTPUT_SIZE``.  No CPU fallback."""
import numpy as np

# csrc/gsa_resize.h
RESIZE_VOTE = 0
RESIZE_NEAREST = 1
RESIZE_MAX_RATIO = 16           # H <= 16 * h and W <= 16 * w
RESIZE_MAX_PIXELS = 1 << 24     # H * W of one source plane
MASK_MODES = {"vote": RESIZE_VOTE, "nearest": RESIZE_NEAREST}
MAX_EXTENT = 65535
SLOTS = 9                       # slot(v) = min(v, 8); the vote writes slot 8 as 255


def axis_weights(L, l):
    """The rule's weights of one axis as a dense (l, L) int64 matrix: ``a[i, y] = max(0, min((i + 1) * L, (y + 1) * l) - max(i * L,
    y * l))``, the overlap of output pixel i and source pixel y in a scale where the source pixel is l long and the output pixel L.
    Every row sums to L and every column to l.  ``1 <= l <= L``; ValueError otherwise."""
    for v in (L, l):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError("axis_weights takes two ints, got %r and %r" % (L, l))
    L, l = int(L), int(l)
    if not 1 <= l <= L:
        raise ValueError("axis_weights needs 1 <= l <= L, got L = %d, l = %d" % (L, l))
    i, y = np.arange(l, dtype=np.int64)[:, None], np.arange(L, dtype=np.int64)[None, :]
    return np.maximum(0, np.minimum((i + 1) * L, (y + 1) * l) - np.maximum(i * L, y * l))


def check_size(size, H, W, what="size"):
    """The target size as ``(h, w)``: an int (both sides) or a pair of ints with ``1 <= h <= H <= 16 * h`` and ``1 <= w <= W <=
    16 * w``.  ValueError, with ``what`` in the message, otherwise; a bool or a float is not a size."""
    sides = (size, size) if not isinstance(size, (tuple, list)) else tuple(size)
    if len(sides) != 2 or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in sides):
        raise ValueError("%s must be an int or a pair (h, w) of ints, got %r" % (what, size))
    h, w = int(sides[0]), int(sides[1])
    for name, l, L in (("height", h, int(H)), ("width", w, int(W))):
        if not 1 <= l <= L:
            raise ValueError("%s: the %s %d must be in 1..%d, the source's (the resize only shrinks)" % (what, name, l, L))
        if L > RESIZE_MAX_RATIO * l:
            raise ValueError("%s: the %s %d is less than 1/%d of the source's %d" % (what, name, l, RESIZE_MAX_RATIO, L))
    return h, w


def check_mask_mode(v, what="mask_mode"):
    """``"vote"`` or ``"nearest"`` -> the C entry's mode number.  ValueError otherwise."""
    if not isinstance(v, str) or v not in MASK_MODES:
        raise ValueError("%s must be \"vote\" or \"nearest\", got %r" % (what, v))
    return MASK_MODES[v]


def _overlaps(a, b):
    pa, pb, sa, sb = a.data_ptr(), b.data_ptr(), a.numel() * a.element_size(), b.numel() * b.element_size()
    return bool(sa and sb and pa < pb + sb and pb < pa + sa)


def resize_pair(img=None, mask=None, size=None, mask_mode="vote", out=None):
    """img (n, H, W, C) with C in 1..4 and / or mask (n, H, W), contiguous uint8 CUDA tensors of one pair batch (either may be None)
    -> ``(img_out, mask_out)``, (n, h, w, C) and (n, h, w) uint8 tensors with None for an absent half.  ``size``: an int or ``(h,
    w)`` with ``1 <= h <= H <= 16 * h`` and ``1 <= w <= W <= 16 * w``; H and W at most 65535 with ``H * W <= 2^24``.

    The image's output pixel is the area mean of the source pixels it covers, rounded half up, exactly (``axis_weights``).  With
    ``mask_mode="vote"`` the mask's output pixel is the value that covers the largest area of it, counted in the nine slots
    ``min(v, 8)``: the lowest slot wins a tie, and slot 8 is written as 255 -- every input value 8..254 comes out as 255, the ignore
    label.  With ``mask_mode="nearest"`` it is ``mask[floor(i * H / h), floor(j * W / w)]``, any value passed through.

    ``out``: a pair ``(img_out, mask_out)`` of tensors to write into (None for an absent half, or to have that one allocated); they
    must overlap neither an input nor each other.  One kernel on the current stream of the tensors' device; the inputs are not
    written.  ValueError on anything else, before any GPU work; no CPU fallback."""
    import torch
    from ._runtime import is_device_tensor, launch
    if img is None and mask is None:
        raise ValueError("resize_pair needs an image, a mask or both")
    if img is not None and (not is_device_tensor(img, torch.uint8, dims=(4,)) or not 1 <= img.shape[-1] <= 4):
        raise ValueError("img must be a contiguous uint8 CUDA tensor (n, H, W, C) with C in 1..4")
    if mask is not None and not is_device_tensor(mask, torch.uint8, dims=(3,)):
        raise ValueError("mask must be a contiguous uint8 CUDA tensor (n, H, W)")
    first = img if img is not None else mask
    dev, (n, H, W) = first.device, (int(s) for s in first.shape[:3])
    if img is not None and mask is not None and (mask.device != dev or tuple(mask.shape) != tuple(img.shape[:3])):
        raise ValueError("mask must be a uint8 tensor %s on %s, as img is, got %s on %s" % (tuple(img.shape[:3]), dev, tuple(mask.shape), mask.device))
    if not 1 <= H <= MAX_EXTENT or not 1 <= W <= MAX_EXTENT or H * W > RESIZE_MAX_PIXELS:
        raise ValueError("resize_pair takes planes whose sides are 1..%d px with at most 2^24 pixels, got %dx%d" % (MAX_EXTENT, H, W))
    h, w = check_size(size, H, W)
    mode = check_mask_mode(mask_mode)
    C = int(img.shape[-1]) if img is not None else 1
    if out is None:
        out = (None, None)
    if not isinstance(out, (tuple, list)) or len(out) != 2:
        raise ValueError("out must be a pair (img_out, mask_out)")
    img_out, mask_out = out
    if (img is None and img_out is not None) or (mask is None and mask_out is not None):
        raise ValueError("out holds a tensor for a half that is not given")
    if img_out is not None and not is_device_tensor(img_out, torch.uint8, shape=(n, h, w, C), device=dev):
        raise ValueError("out[0] must be a contiguous uint8 tensor %s on %s" % ((n, h, w, C), dev))
    if mask_out is not None and not is_device_tensor(mask_out, torch.uint8, shape=(n, h, w), device=dev):
        raise ValueError("out[1] must be a contiguous uint8 tensor %s on %s" % ((n, h, w), dev))
    given = [t for t in (img_out, mask_out) if t is not None]
    if any(_overlaps(o, i) for o in given for i in (img, mask) if i is not None) or (len(given) == 2 and _overlaps(*given)):
        raise ValueError("out must overlap neither an input nor its other half")
    if img is not None and img_out is None:
        img_out = torch.empty((n, h, w, C), dtype=torch.uint8, device=dev)
    if mask is not None and mask_out is None:
        mask_out = torch.empty((n, h, w), dtype=torch.uint8, device=dev)
    if n:
        launch("gsa_pair_resize", dev, n, H, W, C, h, w, mode, img.data_ptr() if img is not None else None,
               mask.data_ptr() if mask is not None else None, img_out.data_ptr() if img is not None else None,
               mask_out.data_ptr() if mask is not None else None)
    return img_out, mask_out


def check_output_size(v, side, what="OUTPUT_SIZE"):
    """The ``OUTPUT_SIZE`` key of ``generate``: None (off), or an int or a list ``[h, w]`` of ints, each a multiple of 16 and at least
    16 (the JPEG and PNG encoders take multiples of 16), at most ``side`` -- the side R / f of the generated pair -- and at least 1/16
    of it -> None or ``(h, w)``.  ValueError with the key's name otherwise."""
    if v is None:
        return None
    h, w = check_size(v, side, side, what)
    for l in (h, w):
        if l < 16 or l % 16:
            raise ValueError("%s: every side must be a multiple of 16 and at least 16, got %r" % (what, v))
    return h, w


def check_output_mask_resize(v, what="OUTPUT_MASK_RESIZE"):
    """The ``OUTPUT_MASK_RESIZE`` key of ``generate``: "vote" or "nearest", as given.  ValueError with the key's name otherwise."""
    check_mask_mode(v, what)
    return v
