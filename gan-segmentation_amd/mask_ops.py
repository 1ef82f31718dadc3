"""ctypes binding of the on-device mask clean-up (include/gsa_mask.h, csrc/gsa_mask.hip) -- the
counterpart of reference utils.morph_mask (utils.py:105-109): a 5x5 close followed by a 5x5 open of a class-index mask.

``morph_mask(mask)`` enqueues one kernel on the current stream of ``mask``'s device and returns the cleaned mask;
``ImageGenerator(..., mask_morph=True)`` applies it to the mask of every fused call.  No CPU fallback."""
import torch

from ._runtime import is_device_tensor, launch

MAX_EXTENT = 65535


def _check(t, what):
    if not is_device_tensor(t, torch.uint8, dims=(2, 3)):
        raise ValueError("%s must be a contiguous uint8 CUDA tensor (H, W) or (n, H, W)" % what)


def morph_mask(mask, out=None):
    """mask (H, W) or (n, H, W) contiguous uint8 CUDA tensor, H and W in 1..65535 -> a tensor of the same shape (new, or ``out``,
    which must be another tensor whose memory does not overlap ``mask``'s): D(E(E(D(mask)))) with the 5x5 all-ones element, taps
    outside the image skipped at every stage, every image of a batch on its own (the rule of include/gsa_mask.h).  Enqueued on the
    current stream of ``mask``'s device; the input is not written.  ValueError on anything else; no CPU fallback."""
    _check(mask, "mask")
    H, W = mask.shape[-2:]
    n = mask.shape[0] if mask.dim() == 3 else 1
    if not 1 <= H <= MAX_EXTENT or not 1 <= W <= MAX_EXTENT:
        raise ValueError("morph_mask takes masks whose sides are 1..%d px, got %dx%d" % (MAX_EXTENT, H, W))
    dev = mask.device
    if out is not None:
        _check(out, "out")
        if tuple(out.shape) != tuple(mask.shape) or out.device != dev:
            raise ValueError("out must be a contiguous uint8 tensor %s on %s" % (tuple(mask.shape), dev))
        a, b, size = mask.data_ptr(), out.data_ptr(), mask.numel()
        if out is mask or (size and a < b + size and b < a + size):
            raise ValueError("out must not be, or overlap, the input mask")
    if out is None:
        out = torch.empty_like(mask)
    if n:
        launch("gsa_mask_morph", dev, n, H, W, mask.data_ptr(), out.data_ptr())
    return out
