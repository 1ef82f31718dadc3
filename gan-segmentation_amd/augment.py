"""The on-device training stream: augmentation plan (host) and ctypes binding of include/gsa_augment.h (csrc/gsa_augment.hip).

What the reference's consumer does to every pair on host threads -- HorizontalFlip, ShiftScaleRotate with a constant border,
PadIfNeeded, RandomCrop, ToTensor, Normalize, the mask border turned into the ignore label -- is one affine map per sample plus a
per-channel scale and bias.  The map is planned here; the kernel applies it to the pair the generate entries left in HBM
(DESIGN.md section 12).

The plan is a pure function of ``(seed, global sample index)``, like the latents (``Generator.draw_indexed``) and the style-mixing
plan (``style_mix``): a sample is augmented the same way whatever batch, rank or GPU count produces it.  For global index ``i``:

    u_0 = splitmix64((seed ^ 0x4155474D454E5421) ^ i)          ("AUGMENT!")
    u_k = splitmix64(u_{k-1}),   r_k = (u_k >> 11) * 2**-53     (uniform in [0, 1))

Mode ``"train"`` takes seven draws, in this order (every one is drawn whether or not its limit is zero):

    r_0  flip      mirror the columns when r_0 < flip                        (flip: a probability, default 0.5)
    r_1  angle     = rotate * (2 r_1 - 1) degrees                            (default rotate = 15)
    r_2  scale     = 1 + scale * (2 r_2 - 1)                                 (default scale = 0.25)
    r_3  dx        = shift * (2 r_3 - 1) * W  pixels                         (default shift = 0.0625)
    r_4  dy        = shift * (2 r_4 - 1) * H  pixels
    r_5  ox        = min(floor(r_5 * (PW - crop + 1)), PW - crop)            (crop origin, columns)
    r_6  oy        = min(floor(r_6 * (PH - crop + 1)), PH - crop)            (crop origin, rows)

The forward map takes a source pixel index (x, y) (integer = pixel centre) to an output pixel index:

    1. flip:            x <- (W - 1) - x
    2. rotate + scale:  [x; y] <- scale * [cos -sin; sin cos] (angle) * [x - cx; y - cy] + [cx; cy],   (cx, cy) = ((W-1)/2, (H-1)/2)
    3. shift:           [x; y] <- [x + dx; y + dy]
    4. central pad of the W x H canvas to PW x PH = max(W, crop) x max(H, crop):  x <- x + (PW - W) // 2,  y <- y + (PH - H) // 2
    5. crop:            x <- x - ox,  y <- y - oy

Mode ``"center"`` takes no draw: steps 4 and 5 only, with the central origin ``ox = (PW - crop) // 2``, ``oy = (PH - crop) // 2``.
``crop=None`` leaves steps 4 and 5 out: the output has the source's size.

The forward map is composed and inverted in float64 and rounded ONCE to fp32: row ``[a b c d e f]`` of the result maps an output
pixel index to source coordinates, which is what the kernel takes.  All unsigned 64-bit arithmetic wraps modulo 2**64.
"""
import numpy as np

from .style_mix import uniform_draws

AUGMENT_SEED_XOR = 0x4155474D454E5421
_M64 = (1 << 64) - 1
NUM_DRAWS = 7
MODES = ("train", "center")
DEFAULT_LIMITS = {"flip": 0.5, "rotate": 15.0, "scale": 0.25, "shift": 0.0625}
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
IGNORE_LABEL = 255
MAX_CHANNELS = 4


# -- the plan ------------------------------------------------------------------------------------------------------------------
def uniforms(seed, first_index, n):
    """float64 (n, 7): the draws r_0 .. r_6 of the global samples ``first_index .. first_index+n-1`` (module docstring)."""
    return uniform_draws(seed, AUGMENT_SEED_XOR, first_index, n, NUM_DRAWS)


def check_crop(crop):
    """``crop`` as an int (a positive multiple of 4) or None; ValueError otherwise."""
    if crop is None:
        return None
    if isinstance(crop, bool) or not isinstance(crop, (int, np.integer)) or int(crop) < 4 or int(crop) % 4:
        raise ValueError("crop must be None or a positive multiple of 4, got %r" % (crop,))
    return int(crop)


def check_mode(mode):
    if mode not in MODES:
        raise ValueError("mode must be one of %s, got %r" % (MODES, mode))
    return mode


def _limits(limits):
    unknown = sorted(set(limits) - set(DEFAULT_LIMITS))
    if unknown:
        raise ValueError("unknown augmentation limit(s) %s (known: %s)" % (unknown, sorted(DEFAULT_LIMITS)))
    out = dict(DEFAULT_LIMITS)
    out.update({k: float(v) for k, v in limits.items()})
    if not 0.0 <= out["flip"] <= 1.0:
        raise ValueError("flip is a probability in [0, 1], got %r" % out["flip"])
    if out["rotate"] < 0 or out["shift"] < 0 or not 0.0 <= out["scale"] < 1.0:
        raise ValueError("rotate and shift must be >= 0 and scale in [0, 1), got %r" % out)
    return out


def output_size(H, W, crop):
    """(out_h, out_w) of a plan: the crop, or the source's size when ``crop`` is None."""
    crop = check_crop(crop)
    return (int(H), int(W)) if crop is None else (crop, crop)


def plan_parameters(seed, first_index, n, H, W, crop, mode="train", **limits):
    """The drawn parameters of the global samples ``first_index .. first_index+n-1`` as a dict of (n,) arrays: ``flip`` (bool),
    ``angle`` (degrees), ``scale``, ``dx``, ``dy`` (pixels), ``ox``, ``oy`` (crop origin in the padded canvas, int64) and the
    scalars ``pad_x``, ``pad_y`` (the central padding in front)."""
    crop, mode, lim = check_crop(crop), check_mode(mode), _limits(limits)
    H, W, n = int(H), int(W), int(n)
    if H < 1 or W < 1 or n < 0:
        raise ValueError("plan: H, W >= 1 and n >= 0 wanted, got H=%d W=%d n=%d" % (H, W, n))
    PW, PH = (W, H) if crop is None else (max(W, crop), max(H, crop))
    cw, ch = (W, H) if crop is None else (crop, crop)
    p = {"pad_x": (PW - W) // 2, "pad_y": (PH - H) // 2}
    if mode == "center":
        p.update(flip=np.zeros(n, bool), angle=np.zeros(n), scale=np.ones(n), dx=np.zeros(n), dy=np.zeros(n),
                 ox=np.full(n, (PW - cw) // 2, np.int64), oy=np.full(n, (PH - ch) // 2, np.int64))
        return p
    r = uniforms(seed, first_index, n)
    p["flip"] = r[:, 0] < lim["flip"]
    p["angle"] = lim["rotate"] * (2.0 * r[:, 1] - 1.0)
    p["scale"] = 1.0 + lim["scale"] * (2.0 * r[:, 2] - 1.0)
    p["dx"] = lim["shift"] * (2.0 * r[:, 3] - 1.0) * W
    p["dy"] = lim["shift"] * (2.0 * r[:, 4] - 1.0) * H
    p["ox"] = np.minimum(np.floor(r[:, 5] * (PW - cw + 1)).astype(np.int64), PW - cw)
    p["oy"] = np.minimum(np.floor(r[:, 6] * (PH - ch + 1)).astype(np.int64), PH - ch)
    return p


def forward_matrices(params, H, W):
    """float64 (n, 2, 3): the forward map (source pixel index -> output pixel index) of ``plan_parameters``' result."""
    n = len(params["angle"])
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    th = np.deg2rad(params["angle"])
    co, si, s = np.cos(th), np.sin(th), params["scale"]
    sign = np.where(params["flip"], -1.0, 1.0)                   # step 1: x <- (W-1) - x  is  sign*x + (W-1 or 0)
    fo = np.where(params["flip"], W - 1.0, 0.0)
    m = np.empty((n, 2, 3), np.float64)
    # steps 2, 3 on (sign*x + fo, y), then the integer translation of steps 4, 5
    m[:, 0, 0] = s * co * sign
    m[:, 0, 1] = -s * si
    m[:, 1, 0] = s * si * sign
    m[:, 1, 1] = s * co
    tx = params["pad_x"] - params["ox"]
    ty = params["pad_y"] - params["oy"]
    m[:, 0, 2] = (s * co * (fo - cx) - s * si * (0.0 - cy)) + cx + params["dx"] + tx
    m[:, 1, 2] = (s * si * (fo - cx) + s * co * (0.0 - cy)) + cy + params["dy"] + ty
    return m


def invert(forward):
    """float64 (n, 2, 3) affine maps -> their inverses, float64 (n, 2, 3)."""
    a, b, c = forward[:, 0, 0], forward[:, 0, 1], forward[:, 0, 2]
    d, e, f = forward[:, 1, 0], forward[:, 1, 1], forward[:, 1, 2]
    det = a * e - b * d
    inv = np.empty_like(forward)
    inv[:, 0, 0], inv[:, 0, 1] = e / det, -b / det
    inv[:, 1, 0], inv[:, 1, 1] = -d / det, a / det
    inv[:, 0, 2] = 0.0 - (inv[:, 0, 0] * c + inv[:, 0, 1] * f)
    inv[:, 1, 2] = 0.0 - (inv[:, 1, 0] * c + inv[:, 1, 1] * f)
    return inv + 0.0            # -0.0 -> +0.0


def plan_matrices(seed, first_index, n, H, W, crop, mode="train", **limits):
    """float32 (n, 6): per sample the row ``[a b c d e f]`` that maps an output pixel index to source pixel-index coordinates
    (module docstring).  ``limits``: ``flip``, ``rotate``, ``scale``, ``shift``; all zero with ``crop=None`` is the identity."""
    params = plan_parameters(seed, first_index, n, H, W, crop, mode, **limits)
    return np.ascontiguousarray(invert(forward_matrices(params, int(H), int(W))).reshape(-1, 6).astype(np.float32))


def normalisation(mean=IMAGENET_MEAN, std=IMAGENET_STD):
    """(scale, bias) float32 arrays with ``u8 * scale + bias == (u8 / 255 - mean) / std`` up to rounding:
    ``scale = 1 / (255 * std)``, ``bias = -mean / std``, formed in float64 and rounded once."""
    mean, std = np.atleast_1d(np.asarray(mean, np.float64)), np.atleast_1d(np.asarray(std, np.float64))
    if mean.shape != std.shape or mean.ndim != 1 or not 1 <= len(mean) <= MAX_CHANNELS:
        raise ValueError("mean and std must have the same length (1..%d values, one per channel)" % MAX_CHANNELS)
    if not (np.all(np.isfinite(mean)) and np.all(np.isfinite(std)) and np.all(std > 0)):
        raise ValueError("mean must be finite and std positive")
    return (1.0 / (255.0 * std)).astype(np.float32), (-mean / std).astype(np.float32)


def stream_batches(first_index, batch, num_samples=None, rank=0, world=1):
    """The ``(first index, size)`` batches rank ``rank`` of ``world`` draws from the global sequence: batch k starts at
    ``first_index + k*batch`` and goes to the rank with ``k % world == rank``, so the union over the ranks does not depend on
    ``world``.  ``num_samples=None`` never ends; otherwise the last batch is short.  A generator."""
    first_index, batch, rank, world = int(first_index), int(batch), int(rank), int(world)
    if batch < 1 or world < 1 or not 0 <= rank < world or first_index < 0:
        raise ValueError("stream: batch >= 1, first_index >= 0 and 0 <= rank < world wanted, got batch=%d first_index=%d rank=%d "
                         "world=%d" % (batch, first_index, rank, world))
    if num_samples is not None and int(num_samples) < 0:
        raise ValueError("num_samples must be None or >= 0, got %r" % (num_samples,))
    return _stream_batches(first_index, batch, None if num_samples is None else int(num_samples), rank, world)


def _stream_batches(first_index, batch, num_samples, rank, world):
    k = rank
    while num_samples is None or k * batch < num_samples:
        size = batch if num_samples is None else min(batch, num_samples - k * batch)
        yield first_index + k * batch, size
        k += world


def check_shapes(H, W, channels, out_size):
    """Validate the kernel's shape arguments on the host (ValueError); returns ``(out_h, out_w)``."""
    if isinstance(out_size, (int, np.integer)) and not isinstance(out_size, bool):
        out_size = (out_size, out_size)
    try:
        oh, ow = (int(v) for v in out_size)
    except (TypeError, ValueError):
        raise ValueError("out_size must be an int or (out_h, out_w), got %r" % (out_size,))
    if oh < 4 or ow < 4 or oh % 4 or ow % 4:
        raise ValueError("the output size must be positive multiples of 4, got %dx%d" % (oh, ow))
    if not 1 <= int(channels) <= MAX_CHANNELS:
        raise ValueError("the augment kernel takes 1..%d channels, got %d" % (MAX_CHANNELS, channels))
    if int(H) < 1 or int(W) < 1:
        raise ValueError("the source must be at least 1x1, got %dx%d" % (H, W))
    return oh, ow


# -- the kernel ----------------------------------------------------------------------------------------------------------------
def augment_pairs(img, mask, matrices, out_size, scale=None, bias=None, dtype=None, ignore_label=IGNORE_LABEL):
    """img (n, H, W, C) u8 and mask (n, H, W) u8 device tensors (what ``ImageGenerator.generate_batch`` returns), matrices (n, 6)
    fp32 (a device tensor, or a numpy array that is uploaded) -> (image (n, C, out_h, out_w) ``dtype``, label (n, out_h, out_w) u8):
    new device tensors, enqueued on the current stream.  ``scale``, ``bias``: per-channel floats (``normalisation``; default: the
    ImageNet statistics, three channels); ``dtype``: torch.float32 (default) or torch.bfloat16."""
    import torch
    from ._runtime import is_device_tensor, launch
    dtype = torch.float32 if dtype is None else dtype
    if dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("dtype must be torch.float32 or torch.bfloat16, got %r" % (dtype,))
    if img.dim() != 4 or mask.dim() != 3 or tuple(mask.shape) != tuple(img.shape[:3]):
        raise ValueError("augment_pairs takes img (n, H, W, C) and mask (n, H, W), got %s and %s" % (tuple(img.shape), tuple(mask.shape)))
    n, H, W, C = img.shape
    oh, ow = check_shapes(H, W, C, out_size)
    if not 0 <= int(ignore_label) <= 255:
        raise ValueError("ignore_label must be in 0..255, got %r" % (ignore_label,))
    if scale is None and bias is None:
        scale, bias = normalisation()
    scale, bias = np.ascontiguousarray(scale, np.float32).ravel(), np.ascontiguousarray(bias, np.float32).ravel()
    if len(scale) != C or len(bias) != C:
        raise ValueError("scale and bias need one value per channel (%d), got %d and %d" % (C, len(scale), len(bias)))
    for t in (img, mask):
        if not is_device_tensor(t, torch.uint8, device=img.device):
            raise ValueError("augment_pairs takes contiguous uint8 tensors on one GPU")
    dev = img.device
    if isinstance(matrices, np.ndarray):
        # through pinned memory, so that the upload is stream-ordered and the host does not wait for the batch in front of it
        matrices = torch.from_numpy(np.ascontiguousarray(matrices, np.float32)).pin_memory().to(dev, non_blocking=True)
    if not is_device_tensor(matrices, torch.float32, shape=(n, 6), device=dev):
        raise ValueError("matrices must be a contiguous float32 (%d, 6) tensor on %s" % (n, dev))
    image = torch.empty((n, C, oh, ow), dtype=dtype, device=dev)
    label = torch.empty((n, oh, ow), dtype=torch.uint8, device=dev)
    if n:
        launch("gsa_augment_pairs", dev, n, H, W, C, img.data_ptr(), mask.data_ptr(), matrices.data_ptr(), scale.ctypes.data,
               bias.ctypes.data, oh, ow, 1 if dtype == torch.bfloat16 else 0, int(ignore_label), image.data_ptr(), label.data_ptr())
    return image, label
