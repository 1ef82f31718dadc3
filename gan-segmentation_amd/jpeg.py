"""ctypes binding of the on-device baseline JPEG encoder (include/gsa_jpeg.h, csrc/gsa_jpeg.hip) -- the image
half of the dataset writer (reference main.py:100-101 ``cv2.imwrite(img_%06d.jpg)``).

``JpegEncoder(n, H, W)`` owns the device workspace and output buffers for batches of up to ``n`` images;
``encode(img)`` enqueues the kernels on the current stream of ``img`` and returns device tensors
``(scan (n, stride) u8, lengths (n,) i32)``; a file is ``encoder.header + scan[i, :lengths[i]]``.  No CPU fallback.

``roundtrip(img)`` (include/gsa_jpeg_roundtrip.h) returns the pixels a reader of those files would decode,
bit for bit, without writing them: what ``ImageGenerator.training_batches(jpeg_quality=...)`` feeds the augmentation."""
import ctypes

import torch

from . import _lib
from ._runtime import current_stream_ptr, is_device_tensor, launch

DEFAULT_QUALITY = 95     # cv2.imwrite's default JPEG quality (the reference passes none)
DEFAULT_RESTART = 4      # MCUs (16x16 px) per restart interval = one wave of the entropy-coding kernel: 1024 independent
#                          waves per 1024^2 image, +0.25 % bytes; measured on 8 FFHQ-size images: 0.09 ms for restart 1, 2 or 4


def header(H, W, quality=DEFAULT_QUALITY, restart=DEFAULT_RESTART):
    """The bytes in front of the entropy-coded data (SOI .. SOS), host side."""
    buf = ctypes.create_string_buffer(1024)
    n = _lib.load_library().fn("gsa_jpeg_header")(H, W, quality, restart, ctypes.cast(buf, ctypes.c_void_p), 1024)
    if n < 0 or n > 1024:
        raise _lib.GsaError("gsa_jpeg_header failed (%d)" % n)
    return buf.raw[:n]


class JpegEncoder:
    def __init__(self, n, H, W, device, quality=DEFAULT_QUALITY, restart=DEFAULT_RESTART, out_stride=None):
        fn = _lib.load_library().fn
        self.n, self.H, self.W, self.quality, self.restart = n, H, W, quality, restart
        self.device = torch.device(device)
        ws = fn("gsa_jpeg_workspace_bytes")(n, H, W, restart)
        worst = fn("gsa_jpeg_max_scan_bytes")(H, W, restart)
        if ws < 0 or worst < 0:
            raise ValueError("JPEG encoder: images must be multiples of 16 px (got %dx%d), restart in 1..65535; other "
                             "sizes go through the host encoder (DatasetWriter(gpu_jpeg=False) / JPEG_ON_GPU: false)" % (H, W))
        self.header = header(H, W, quality, restart)
        # default stride: the size of the raw pixels (a q95 scan is ~1/7 of it; noise at q100 can exceed it -> the
        # call reports the size needed as a negative length and encode() retries with the worst-case stride)
        self.out_stride = int(min(worst, out_stride if out_stride is not None else H * W * 3))
        self.worst = int(worst)
        self._ws = torch.empty(ws, dtype=torch.uint8, device=self.device)
        self._alloc_out()

    def _alloc_out(self):
        self.out = torch.empty((self.n, self.out_stride), dtype=torch.uint8, device=self.device)
        self.lengths = torch.empty(self.n, dtype=torch.int32, device=self.device)

    def encode(self, img):
        """img: (k, H, W, 3) uint8 CUDA tensor, k <= n.  -> (scan (k, stride) u8, lengths (k,) i32), stream-ordered."""
        if not is_device_tensor(img, torch.uint8):
            raise ValueError("encode takes a contiguous uint8 CUDA tensor")
        k = img.shape[0]
        if k > self.n or tuple(img.shape[1:]) != (self.H, self.W, 3):
            raise ValueError("image batch %s does not fit the encoder (%d, %d, %d, 3)" % (tuple(img.shape), self.n, self.H, self.W))
        launch("gsa_jpeg_encode", img.device, k, self.H, self.W, img.data_ptr(), self.quality, self.restart, self._ws.data_ptr(),
               self._ws.numel(), self.out.data_ptr(), self.out_stride, self.lengths.data_ptr())
        return self.out[:k], self.lengths[:k]

    def grow(self):
        """Switch to the worst-case stride (after a negative length)."""
        self.out_stride = self.worst
        self._alloc_out()

    def files(self, img):
        """Convenience (tests, small jobs): encode and return the complete files as ``bytes`` (synchronises)."""
        scan, lengths = self.encode(img)
        ln = lengths.cpu().numpy()
        if (ln < 0).any():
            self.grow()
            scan, lengths = self.encode(img)
            ln = lengths.cpu().numpy()
        host = scan.cpu().numpy()
        return [self.header + host[i, :ln[i]].tobytes() for i in range(len(ln))]


# -- the round trip (include/gsa_jpeg_roundtrip.h) -------------------------------------------------------------------------------
_ROUNDTRIP_WORKSPACES = {}       # (device index, stream, bytes) -> u8 tensor; a handful of sizes per process
_ROUNDTRIP_WORKSPACES_MAX = 8


def check_quality(quality, what="quality"):
    """``quality`` as an int in 1..100 (the encoder's range); ValueError otherwise."""
    import numbers
    if isinstance(quality, bool) or not isinstance(quality, numbers.Integral) or not 1 <= int(quality) <= 100:
        raise ValueError("%s must be an int in 1..100, got %r" % (what, quality))
    return int(quality)


def check_roundtrip_shape(H, W, channels):
    """The shapes the round trip takes (4:2:0 colour files of whole 16x16-px MCUs); ValueError otherwise."""
    if int(channels) != 3:
        raise ValueError("the JPEG round trip takes three image channels, got %d" % channels)
    if int(H) < 16 or int(W) < 16 or int(H) % 16 or int(W) % 16 or int(H) > 65535 or int(W) > 65535:
        raise ValueError("the JPEG round trip takes images whose sides are a multiple of 16 px (16..65535), got %dx%d" % (H, W))


def roundtrip(img, quality=DEFAULT_QUALITY, out=None):
    """img (n, H, W, 3) contiguous uint8 CUDA tensor, H and W multiples of 16 -> a tensor of the same shape (new, or ``out``, which
    must not be ``img``): the pixels a libjpeg decoder returns for the quality-``quality`` 4:2:0 file of every image, bit for bit what
    a reader of ``JpegEncoder``'s files sees.  Enqueued on the current stream of ``img``'s device; the workspace (1.5 bytes per
    pixel) is cached per device, stream and size.  No CPU fallback."""
    quality = check_quality(quality)
    if not is_device_tensor(img, torch.uint8, dims=(4,)):
        raise ValueError("roundtrip takes a contiguous uint8 CUDA tensor (n, H, W, 3)")
    n, H, W, C = img.shape
    check_roundtrip_shape(H, W, C)
    dev = img.device
    if out is not None:
        if not is_device_tensor(out, torch.uint8, shape=img.shape, device=dev) or (n and out.data_ptr() == img.data_ptr()):
            raise ValueError("out must be another contiguous uint8 tensor %s on %s" % (tuple(img.shape), dev))
    if out is None:
        out = torch.empty_like(img)
    if n == 0:
        return out
    need = _lib.load_library().fn("gsa_jpeg_roundtrip_workspace_bytes")(n, H, W)
    if need < 0:
        raise _lib.GsaError("gsa_jpeg_roundtrip_workspace_bytes failed (%d)" % need)
    key = (dev.index, current_stream_ptr(dev), need)
    ws = _ROUNDTRIP_WORKSPACES.get(key)
    if ws is None:
        if len(_ROUNDTRIP_WORKSPACES) >= _ROUNDTRIP_WORKSPACES_MAX:
            _ROUNDTRIP_WORKSPACES.pop(next(iter(_ROUNDTRIP_WORKSPACES)))
        ws = _ROUNDTRIP_WORKSPACES[key] = torch.empty(need, dtype=torch.uint8, device=dev)
    launch("gsa_jpeg_roundtrip", dev, n, H, W, img.data_ptr(), quality, ws.data_ptr(), ws.numel(), out.data_ptr())
    return out
