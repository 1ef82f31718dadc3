"""Photometric augmentation of the training stream: the plan (host) and the ctypes binding of include/gsa_photometric.h
(csrc/gsa_photometric.hip).

What the reference's consumer does to the VALUES of an image on host threads -- RandomContrast, RandomBrightness, RGBShift, a
Gaussian Blur, GaussNoise -- is one kernel on the u8 image batch in front of the warp: ``b = blur(p)``, ``c = b*alpha + offset[ch]``,
``v = c + noise_sigma*g``, ``out = uint8(floor(clamp(v, 0, 255) + 0.5))`` (the header has the rule to the bit).  The mask is untouched.

The plan is a pure function of ``(seed, global sample index)``, like ``augment.plan_matrices``: a sample is changed the same way
whatever batch, rank or GPU count produces it.  For global index ``i``:

    u_0 = splitmix64((seed ^ 0x50484F544F4D4554) ^ i)          ("PHOTOMET")
    u_k = splitmix64(u_{k-1}),   r_k = (u_k >> 11) * 2**-53     (uniform in [0, 1))

Ten draws, in this order (every one is drawn whether or not its limit is zero):

    r_0       contrast     alpha = 1 + contrast * (2 r_0 - 1)                              (default contrast = 0.2)
    r_1       brightness   beta = 255 * brightness * (2 r_1 - 1)                           (default brightness = 0.2)
    r_2..r_5  shifts       offset[c] = beta + rgb_shift * (2 r_{2+c} - 1),  c = 0..3       (default rgb_shift = 20)
    r_6, r_7  blur         sigma = blur_sigma * r_7 when r_6 < blur_prob, else 0           (defaults 0.5, 1.0)
    r_8, r_9  noise        noise = noise_sigma * r_9 when r_8 < noise_prob, else 0         (defaults 0.5, 7.0)

The seven blur weights come from ``sigma`` in float64: ``exp(-k^2 / (2 sigma^2))`` for k = -3..3, values below 2**-64 set to zero (the
device never sees a denormal product), normalised to sum 1, rounded ONCE to fp32; ``sigma == 0`` gives the identity 0 0 0 1 0 0 0.
A row of the plan is ``alpha, offset[0..3], noise, w[0..6], 0, 0, 0``: 16 fp32 values.  With every limit zero the rows make the kernel
the identity.  All unsigned 64-bit arithmetic wraps modulo 2**64.
"""
import numpy as np

from .style_mix import uniform_draws

PHOTOMETRIC_SEED_XOR = 0x50484F544F4D4554
_M64 = (1 << 64) - 1
NUM_DRAWS = 10
ROW = 16
RADIUS = 3
MAX_BLUR_SIGMA = 1.5
MAX_CHANNELS = 4
MIN_EXTENT = RADIUS + 1
DEFAULT_LIMITS = {"contrast": 0.2, "brightness": 0.2, "rgb_shift": 20.0, "blur_prob": 0.5, "blur_sigma": 1.0, "noise_prob": 0.5,
                  "noise_sigma": 7.0}
ZERO_LIMITS = {k: 0.0 for k in DEFAULT_LIMITS}


# -- the plan ------------------------------------------------------------------------------------------------------------------
def uniforms(seed, first_index, n):
    """float64 (n, 10): the draws r_0 .. r_9 of the global samples ``first_index .. first_index+n-1`` (module docstring)."""
    return uniform_draws(seed, PHOTOMETRIC_SEED_XOR, first_index, n, NUM_DRAWS)


def check_limits(limits):
    """The limits as a complete dict of floats (defaults filled in); ValueError on an unknown or out-of-range one."""
    unknown = sorted(set(limits) - set(DEFAULT_LIMITS))
    if unknown:
        raise ValueError("unknown photometric limit(s) %s (known: %s)" % (unknown, sorted(DEFAULT_LIMITS)))
    out = dict(DEFAULT_LIMITS)
    for k, v in limits.items():
        if isinstance(v, (bool, str)) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v):
            raise ValueError("photometric limit %s must be a finite number, got %r" % (k, v))
        out[k] = float(v)
    for k in ("blur_prob", "noise_prob"):
        if not 0.0 <= out[k] <= 1.0:
            raise ValueError("%s is a probability in [0, 1], got %r" % (k, out[k]))
    if not 0.0 <= out["contrast"] < 1.0:
        raise ValueError("contrast must be in [0, 1), got %r" % out["contrast"])
    for k in ("brightness", "rgb_shift", "noise_sigma"):
        if out[k] < 0.0:
            raise ValueError("%s must be >= 0, got %r" % (k, out[k]))
    if not 0.0 <= out["blur_sigma"] <= MAX_BLUR_SIGMA:
        raise ValueError("blur_sigma must be in [0, %g] (the kernel's radius is %d), got %r" % (MAX_BLUR_SIGMA, RADIUS, out["blur_sigma"]))
    return out


def check_keyword(photometric):
    """The ``photometric`` keyword of ``ImageGenerator.training_batches``: None (off) -> None, True -> the default limits, a dict
    -> its checked limits; ValueError for anything else."""
    if photometric is None:
        return None
    if photometric is True:
        return dict(DEFAULT_LIMITS)
    if isinstance(photometric, dict):
        return check_limits(photometric)
    raise ValueError("photometric must be None, True or a dict of limits (%s), got %r" % (sorted(DEFAULT_LIMITS), photometric))


def blur_weights(sigma):
    """float32 (n, 7) blur weights of the float64 (n,) ``sigma`` (module docstring); identity where sigma == 0."""
    sigma = np.atleast_1d(np.asarray(sigma, np.float64))
    k = np.arange(-RADIUS, RADIUS + 1, dtype=np.float64)
    on = 2.0 * sigma ** 2 > 0                    # a sigma whose square underflows is no blur either
    safe = np.where(on, sigma, 1.0)
    with np.errstate(over="ignore"):
        w = np.exp(-(k[None, :] ** 2) / (2.0 * safe[:, None] ** 2))
    w[w < 2.0 ** -64] = 0.0
    w = w / w.sum(axis=1, keepdims=True)
    w[~on] = (k == 0).astype(np.float64)
    return w.astype(np.float32)


def plan_parameters(seed, first_index, n, **limits):
    """The drawn parameters of the global samples ``first_index .. first_index+n-1`` as a dict of float64 arrays: ``alpha`` (n,),
    ``beta`` (n,), ``offset`` (n, 4), ``sigma`` (n,; 0 = no blur), ``noise`` (n,; 0 = no noise)."""
    lim, n = check_limits(limits), int(n)
    if n < 0:
        raise ValueError("plan: n >= 0 wanted, got %d" % n)
    r = uniforms(seed, first_index, n)
    beta = 255.0 * lim["brightness"] * (2.0 * r[:, 1] - 1.0)
    return {
        "alpha": 1.0 + lim["contrast"] * (2.0 * r[:, 0] - 1.0),
        "beta": beta,
        "offset": beta[:, None] + lim["rgb_shift"] * (2.0 * r[:, 2:6] - 1.0),
        "sigma": np.where(r[:, 6] < lim["blur_prob"], lim["blur_sigma"] * r[:, 7], 0.0),
        "noise": np.where(r[:, 8] < lim["noise_prob"], lim["noise_sigma"] * r[:, 9], 0.0),
    }


def photometric_plan(seed, first_index, n, **limits):
    """float32 (n, 16): per sample the row ``alpha, offset[0..3], noise_sigma, w[0..6], 0, 0, 0`` the kernel takes (module
    docstring).  ``limits``: contrast, brightness, rgb_shift, blur_prob, blur_sigma, noise_prob, noise_sigma; all zero is the identity."""
    p = plan_parameters(seed, first_index, n, **limits)
    rows = np.zeros((int(n), ROW), np.float32)
    rows[:, 0] = p["alpha"]
    rows[:, 1:5] = p["offset"]
    rows[:, 5] = p["noise"]
    rows[:, 6:13] = blur_weights(p["sigma"])
    return rows


def check_shape(H, W, channels):
    """Validate the kernel's shape arguments on the host (ValueError)."""
    H, W, channels = int(H), int(W), int(channels)
    if not 1 <= channels <= MAX_CHANNELS:
        raise ValueError("the photometric kernel takes 1..%d channels, got %d" % (MAX_CHANNELS, channels))
    if H < MIN_EXTENT or W < MIN_EXTENT:
        raise ValueError("the photometric kernel takes images of at least %dx%d (reflect-101 at radius %d), got %dx%d"
                         % (MIN_EXTENT, MIN_EXTENT, RADIUS, H, W))
    if H * W > 1 << 31 or W * channels >= 1 << 31:
        raise ValueError("the photometric kernel takes at most 2^31 pixels per image, got %dx%d" % (H, W))


# -- the kernel ----------------------------------------------------------------------------------------------------------------
def photometric(img, params, seed, first_index):
    """img (n, H, W, C) contiguous u8 device tensor (what ``ImageGenerator.generate_indexed`` returns), params (n, 16) fp32 (a
    device tensor, or a numpy array that is uploaded), sample k being the global sample ``first_index + k`` of ``seed`` -> a new
    (n, H, W, C) u8 tensor: the rule of include/gsa_photometric.h, enqueued on the current stream of ``img``'s device.  The input
    is not written.  ValueError on anything else; no CPU fallback."""
    import torch
    from ._runtime import is_device_tensor, launch
    if not is_device_tensor(img, torch.uint8, dims=(4,)):
        raise ValueError("photometric takes a contiguous uint8 CUDA tensor (n, H, W, C)")
    n, H, W, C = img.shape
    check_shape(H, W, C)
    dev = img.device
    if isinstance(params, np.ndarray):
        if params.shape != (n, ROW):
            raise ValueError("params must be (%d, %d), got %s" % (n, ROW, params.shape))
        # through pinned memory, so that the upload is stream-ordered and the host does not wait for the batch in front of it
        params = torch.from_numpy(np.ascontiguousarray(params, np.float32)).pin_memory().to(dev, non_blocking=True)
    if not is_device_tensor(params, torch.float32, shape=(n, ROW), device=dev):
        raise ValueError("params must be a contiguous float32 (%d, %d) tensor on %s" % (n, ROW, dev))
    seed, first_index = int(seed) & _M64, int(first_index) & _M64
    out = torch.empty_like(img)
    if n:
        launch("gsa_photometric", dev, n, H, W, C, img.data_ptr(), params.data_ptr(), seed, first_index, out.data_ptr())
    return out
