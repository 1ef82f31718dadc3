"""ctypes binding of the on-device decoder losses (csrc/gsa_loss.h, csrc/gsa_loss.hip): the softmax
cross-entropy of ``train_ops.softmax_ce`` with per-class weights, a per-pixel weight read from the boundary distance of the labels, a
focal factor and a choice of normaliser -- what ``trainer.DecoderTrainer(..., loss=LossSpec(...))``, ``SegSolver.fit(..., loss=...)``
and the config key ``TRAIN_LOSS`` train the decoder with.  Without a spec nothing changes: the trainer calls ``softmax_ce``.

``LossSpec`` holds the options and validates them, ``boundary_weight_table`` is the weight of a pixel by its squared distance to the
nearest label boundary, ``class_weights_from_masks`` computes the two class-weight vectors of ``pair_stats.summarise`` from
annotation masks, and ``softmax_loss`` enqueues the two kernels on the current stream of the logits' device.  Results are the same
bits from run to run and do not depend on the batch a sample is in.  No CPU fallback.

``region_loss`` is the region term beside them (csrc/gsa_region.h, csrc/gsa_region.hip): per sample and class
the soft Tversky index of the softmax against the labels -- soft Dice, soft Jaccard -- with its loss and gradient, which
``LossSpec(region=...)`` adds to the cross-entropy term of a training step."""
import math

import numpy as np

from . import _lib

# csrc/gsa_loss.h
LOSS_TABLE = 1026           # floats of a boundary table: dist2 0..1024, then one entry for everything else (BOUNDARY_FAR)
LOSS_MAX_BLOCKS = 512       # workgroups that walk one sample
LOSS_SUMS = 4
SUM_W, SUM_B, SUM_S, SUM_T = range(LOSS_SUMS)       # columns of ``sums``: weights, focal mass, weighted loss, valid pixels
NORMALISE = {"mean": 0, "valid": 1, "focal": 2}
MIN_CLASSES, MAX_CLASSES = 2, 64
MAX_GAMMA = 8.0
MAX_RADIUS = 32             # mask_ops.BOUNDARY_MAX_RADIUS: radius^2 <= 1024 = LOSS_TABLE - 2
CLASS_WEIGHT_SCHEMES = ("median", "inverse")
SPEC_KEYS = ("gamma", "normalise", "class_weights", "boundary", "region")
BOUNDARY_KEYS = ("weight", "sigma", "radius")
# csrc/gsa_region.h
REGION_MAX_CLASSES = 16     # classes of the region term: 2 .. 16
REGION_MAX_BLOCKS = 512     # workgroups that walk one sample
REGION_SUMS = 3
SUM_I, SUM_P, SUM_G = range(REGION_SUMS)            # rows of the region ``sums``: intersection, predicted mass, labelled pixels
REGION_CLASSES = {"present": 0, "all": 1}
REGION_KEYS = ("weight", "alpha", "beta", "smooth", "classes")
REGION_DEFAULTS = {"alpha": 0.5, "beta": 0.5, "smooth": 1.0, "classes": "present"}


def _number(v):
    return not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating)) and math.isfinite(float(v))


def check_gamma(v, what="gamma"):
    """The focal exponent as a float: 0 (off) or 1 .. 8.  ValueError otherwise: the gradient of q^gamma needs q^(gamma - 1) at q -> 0."""
    if not _number(v) or not (float(v) == 0.0 or 1.0 <= float(v) <= MAX_GAMMA):
        raise ValueError("%s must be 0 or a number in 1..%g, got %r" % (what, MAX_GAMMA, v))
    return float(v)


def check_normalise(v, what="normalise"):
    """The normaliser's name: "mean" (S / HW), "valid" (S / W) or "focal" (S / B).  ValueError otherwise."""
    if not isinstance(v, str) or v not in NORMALISE:
        raise ValueError("%s must be one of %s, got %r" % (what, ", ".join(repr(k) for k in NORMALISE), v))
    return v


def check_class_weights(v, what="class_weights", num_classes=None, schemes=True):
    """None, one of ``CLASS_WEIGHT_SCHEMES`` (where ``schemes``), or 2 .. 64 finite numbers >= 0 (``num_classes`` of them where given)
    -> None, the string, or a tuple of floats.  ValueError otherwise."""
    if v is None:
        return None
    if isinstance(v, str):
        if schemes and v in CLASS_WEIGHT_SCHEMES:
            return v
        raise ValueError("%s must be a list of numbers%s, got %r"
                         % (what, " or one of %s" % ", ".join(repr(k) for k in CLASS_WEIGHT_SCHEMES) if schemes else "", v))
    if isinstance(v, np.ndarray):
        v = v.tolist()
    if not isinstance(v, (list, tuple)) or not all(_number(x) and float(x) >= 0.0 for x in v):
        raise ValueError("%s must be a list of finite numbers >= 0, got %r" % (what, v))
    if not MIN_CLASSES <= len(v) <= MAX_CLASSES or (num_classes is not None and len(v) != num_classes):
        raise ValueError("%s must hold %s numbers, got %d" % (what, "%d..%d" % (MIN_CLASSES, MAX_CLASSES) if num_classes is None
                                                             else "%d" % num_classes, len(v)))
    return tuple(float(x) for x in v)


def check_boundary(v, what="boundary"):
    """None, or a mapping with exactly the keys weight (>= 0), sigma (> 0) and radius (int 1 .. 32) -> None or a dict of
    (float, float, int).  ValueError otherwise, naming the key."""
    if v is None:
        return None
    if not isinstance(v, dict):
        raise ValueError("%s must be a mapping with the keys %s, got %r" % (what, ", ".join(BOUNDARY_KEYS), v))
    unknown = sorted(str(k) for k in v if k not in BOUNDARY_KEYS)
    missing = [k for k in BOUNDARY_KEYS if k not in v]
    if unknown or missing:
        raise ValueError("%s: %s" % (what, "; ".join(([("unknown key %s" % k) for k in unknown]) + [("missing key %s" % k) for k in missing])))
    w, s, r = v["weight"], v["sigma"], v["radius"]
    if not _number(w) or float(w) < 0.0:
        raise ValueError("%s: weight must be a number >= 0, got %r" % (what, w))
    if not _number(s) or float(s) <= 0.0:
        raise ValueError("%s: sigma must be a number > 0, got %r" % (what, s))
    if isinstance(r, bool) or not isinstance(r, (int, np.integer)) or not 1 <= int(r) <= MAX_RADIUS:
        raise ValueError("%s: radius must be an int in 1..%d, got %r" % (what, MAX_RADIUS, r))
    return {"weight": float(w), "sigma": float(s), "radius": int(r)}


def check_tversky(alpha, beta, smooth, classes, what="region"):
    """alpha, beta and smooth as floats >= 0 with alpha + beta > 0, and the name of the class set, "present" or "all".  ValueError
    otherwise, naming the argument."""
    for name, v in (("alpha", alpha), ("beta", beta), ("smooth", smooth)):
        if not _number(v) or float(v) < 0.0:
            raise ValueError("%s: %s must be a number >= 0, got %r" % (what, name, v))
    if float(alpha) + float(beta) == 0.0:
        raise ValueError("%s: alpha + beta must be > 0, got alpha %r and beta %r" % (what, alpha, beta))
    if not isinstance(classes, str) or classes not in REGION_CLASSES:
        raise ValueError("%s: classes must be one of %s, got %r" % (what, ", ".join(repr(k) for k in REGION_CLASSES), classes))
    return float(alpha), float(beta), float(smooth), classes


def check_region(v, what="region"):
    """None, or a mapping with the key weight (>= 0) and keys among alpha, beta (>= 0, not both 0; default 0.5: soft Dice), smooth
    (>= 0, default 1) and classes ("present", the default, or "all") -> None or a dict of all five.  ValueError otherwise, naming
    the key."""
    if v is None:
        return None
    if not isinstance(v, dict):
        raise ValueError("%s must be a mapping with keys among %s, got %r" % (what, ", ".join(REGION_KEYS), v))
    unknown = sorted(str(k) for k in v if k not in REGION_KEYS)
    missing = [k for k in ("weight",) if k not in v]
    if unknown or missing:
        raise ValueError("%s: %s" % (what, "; ".join(([("unknown key %s" % k) for k in unknown]) + [("missing key %s" % k) for k in missing])))
    w = v["weight"]
    if not _number(w) or float(w) < 0.0:
        raise ValueError("%s: weight must be a number >= 0, got %r" % (what, w))
    o = dict(REGION_DEFAULTS, **{k: v[k] for k in REGION_KEYS[1:] if k in v})
    alpha, beta, smooth, classes = check_tversky(o["alpha"], o["beta"], o["smooth"], o["classes"], what)
    return {"weight": float(w), "alpha": alpha, "beta": beta, "smooth": smooth, "classes": classes}


def boundary_weight_table(radius, weight, sigma):
    """float32[LOSS_TABLE]: the weight of a pixel by the squared distance d to the nearest pixel of another label, as
    ``mask_ops.boundary_distance`` gives it: 1 + weight * exp(-d / (2 sigma^2)) for 1 <= d <= radius^2, and exactly 1 for d = 0 (no
    pixel has it), for d > radius^2 and for the last entry, the one of BOUNDARY_FAR.  float64, rounded once."""
    b = check_boundary({"weight": weight, "sigma": sigma, "radius": radius})
    d = np.arange(LOSS_TABLE, dtype=np.float64)
    t = 1.0 + b["weight"] * np.exp(-d / (2.0 * b["sigma"] ** 2))
    t[0] = 1.0
    t[b["radius"] ** 2 + 1:] = 1.0
    return t.astype(np.float32)


class LossSpec:
    """The options of the decoder's loss (the rule is in csrc/gsa_loss.h).  ``gamma``: focal exponent, 0 or 1..8; ``normalise``:
    "mean" (over H * W, the reference's SoftmaxCELoss), "valid" (over the sum of the weights) or "focal" (over the sum of the weights
    times the focal factor: the reference's NormalizedFocalLossSoftmax); ``class_weights``: None, ``num_classes`` numbers >= 0, or
    "median" / "inverse", which ``SegSolver.fit`` computes from its annotation masks (``with_class_weights``);
    ``boundary``: None or ``dict(weight=, sigma=, radius=)``, the per-pixel factor of ``boundary_weight_table``; ``region``: None or
    ``dict(weight=, alpha=, beta=, smooth=, classes=)`` (``check_region``): ``weight`` times the region term of ``region_loss`` is
    added to the loss, with the spec's numeric class weights.  ValueError on anything else, the message beginning with ``what``."""

    def __init__(self, gamma=0.0, normalise="mean", class_weights=None, boundary=None, region=None, what="LossSpec"):
        self.gamma = check_gamma(gamma, "%s: gamma" % what)
        self.normalise = check_normalise(normalise, "%s: normalise" % what)
        self.class_weights = check_class_weights(class_weights, "%s: class_weights" % what)
        self.boundary = check_boundary(boundary, "%s: boundary" % what)
        self.region = check_region(region, "%s: region" % what)

    @classmethod
    def from_mapping(cls, v, what="loss"):
        """A mapping with keys among ``SPEC_KEYS`` (a config value) -> LossSpec.  Unknown keys are a ValueError."""
        if not isinstance(v, dict):
            raise ValueError("%s must be a mapping with keys among %s, got %r" % (what, ", ".join(SPEC_KEYS), v))
        unknown = sorted(str(k) for k in v if k not in SPEC_KEYS)
        if unknown:
            raise ValueError("%s: unknown key%s %s (known: %s)" % (what, "s" if len(unknown) > 1 else "", ", ".join(unknown), ", ".join(SPEC_KEYS)))
        return cls(what=what, **v)

    @property
    def needs_masks(self):
        """Whether ``class_weights`` is still the name of a scheme."""
        return isinstance(self.class_weights, str)

    def with_class_weights(self, weights):
        """A copy with ``class_weights`` replaced by numbers."""
        return LossSpec(self.gamma, self.normalise, weights, self.boundary, self.region)

    def table(self):
        """``boundary_weight_table`` of the spec's boundary, or None."""
        return None if self.boundary is None else boundary_weight_table(**self.boundary)

    def as_dict(self):
        return {"gamma": self.gamma, "normalise": self.normalise,
                "class_weights": list(self.class_weights) if isinstance(self.class_weights, tuple) else self.class_weights,
                "boundary": dict(self.boundary) if self.boundary else None,
                "region": dict(self.region) if self.region else None}

    def __repr__(self):
        return "LossSpec(%s)" % ", ".join("%s=%r" % kv for kv in self.as_dict().items())


def check_spec(v, what="loss"):
    """None, a LossSpec or a mapping of its keywords -> None or a LossSpec."""
    if v is None or isinstance(v, LossSpec):
        return v
    return LossSpec.from_mapping(v, what)


def class_weights_from_masks(masks, num_classes, scheme="median"):
    """The class weights of ``pair_stats.summarise`` from label masks: ``masks`` an iterable of integer arrays of one size, class
    indices with anything outside 0 .. ``num_classes`` - 1 (the ignore label -1) counted as a pixel of no class.  ``scheme``:
    "median" (weights_median_frequency) or "inverse" (weights_inverse_frequency).  -> a list of ``num_classes`` entries, None for a
    class that no mask holds, as ``summarise`` reports it.  Host code; ValueError on no mask, differing sizes or a bad argument."""
    from .pair_stats import frequency_weights
    if scheme not in CLASS_WEIGHT_SCHEMES:
        raise ValueError("scheme must be one of %s, got %r" % (", ".join(repr(k) for k in CLASS_WEIGHT_SCHEMES), scheme))
    if isinstance(num_classes, bool) or not isinstance(num_classes, (int, np.integer)) or not MIN_CLASSES <= int(num_classes) <= MAX_CLASSES:
        raise ValueError("num_classes must be an int in %d..%d, got %r" % (MIN_CLASSES, MAX_CLASSES, num_classes))
    num_classes = int(num_classes)
    pixels, presence, shape, m = [0] * num_classes, [0] * num_classes, None, 0
    for mask in masks:
        a = np.asarray(mask)
        if a.dtype.kind not in "iu" or a.size == 0:
            raise ValueError("a mask must be a non-empty integer array, got dtype %s, shape %s" % (a.dtype, a.shape))
        if shape is None:
            shape = a.shape
        elif a.shape != shape:
            raise ValueError("masks of differing sizes: %s and %s" % (shape, a.shape))
        a = a.astype(np.int64).reshape(-1)
        counts = np.bincount(a[(a >= 0) & (a < num_classes)], minlength=num_classes)
        for s in range(num_classes):
            pixels[s] += int(counts[s])
            presence[s] += 1 if counts[s] else 0
        m += 1
    if not m:
        raise ValueError("no masks to take class weights from")
    plane = int(np.prod(shape))
    inverse, median_f = frequency_weights(pixels, presence, plane, m * plane, num_classes)
    return median_f if scheme == "median" else inverse


def _device_f32(v, count, device, what):
    import torch
    if isinstance(v, torch.Tensor):
        if not (v.is_cuda and v.device == device and v.dtype == torch.float32 and v.is_contiguous() and v.numel() == count):
            raise ValueError("%s must be a contiguous float32 tensor of %d elements on %s" % (what, count, device))
        return v
    a = np.ascontiguousarray(v, dtype=np.float32).reshape(-1)
    if a.size != count or not np.isfinite(a).all():
        raise ValueError("%s must hold %d finite numbers" % (what, count))
    return torch.from_numpy(a).to(device)


def workspace_bytes(n, HW):
    """gsa_loss_workspace_bytes: n * min(ceil(HW / 256), LOSS_MAX_BLOCKS) * 32."""
    size = _lib.load_library().fn("gsa_loss_workspace_bytes")(int(n), int(HW))
    if size < 0:
        raise ValueError("no workspace for n = %r, HW = %r" % (n, HW))
    return int(size)


def softmax_loss(logits, labels, spec=None, gamma=0.0, normalise="mean", class_weights=None, dist2=None, table=None, grad=True,
                 grad_scale=1.0, workspace=None):
    """logits (n, K, H, W) or (n, K, HW) contiguous float32 CUDA tensor, K in 2..64; labels: a contiguous int8 tensor of n * HW
    elements on the same device, a pixel being valid iff its label is in 0 .. K - 1.  The options come from ``spec`` (a LossSpec with
    numeric class weights) or, without one, from the keywords ``gamma``, ``normalise`` and ``class_weights`` (K numbers, or a
    float32 device tensor of them).  ``dist2`` and ``table`` go together: the int16 plane of ``mask_ops.boundary_distance`` of the
    labels and the LOSS_TABLE weights (numbers or a device tensor; by default the table of the spec's boundary); a spec with a
    boundary needs ``dist2``.  ``grad=False``: forward only, for a validation loss.  ``workspace``: a uint8 device tensor of at least
    ``workspace_bytes(n, HW)`` bytes to reuse, else one is allocated.
    -> (loss float32 (n,), sums float64 (n, 4) = [W, B, S, T], dlogits as logits or None); dlogits = grad_scale * d loss[n] / d logits.
    Two kernels on the current stream of the logits' device; ValueError on anything else; no CPU fallback."""
    import torch
    from ._runtime import is_device_tensor, launch
    if not is_device_tensor(logits, torch.float32, dims=(3, 4)):
        raise ValueError("logits must be a contiguous float32 CUDA tensor (n, K, H, W) or (n, K, HW)")
    n, K = int(logits.shape[0]), int(logits.shape[1])
    HW = int(np.prod(logits.shape[2:]))
    dev = logits.device
    if not MIN_CLASSES <= K <= MAX_CLASSES or HW <= 0:
        raise ValueError("logits must hold %d..%d classes and at least one pixel, got shape %s" % (MIN_CLASSES, MAX_CLASSES, tuple(logits.shape)))
    if n * K * HW >= 2 ** 40:
        raise ValueError("logits of %d elements: at most 2^40 - 1" % (n * K * HW))
    if not is_device_tensor(labels, torch.int8, device=dev) or labels.numel() != n * HW:
        raise ValueError("labels must be a contiguous int8 tensor of %d elements on %s" % (n * HW, dev))
    if spec is not None:
        if not isinstance(spec, LossSpec):
            raise ValueError("spec must be a LossSpec, got %r" % (spec,))
        if spec.needs_masks:
            raise ValueError("class_weights %r must be turned into numbers first (LossSpec.with_class_weights)" % spec.class_weights)
        gamma, normalise = spec.gamma, spec.normalise
        class_weights = spec.class_weights if class_weights is None else class_weights
        if spec.boundary is not None:
            if dist2 is None:
                raise ValueError("a spec with a boundary needs dist2, the plane of mask_ops.boundary_distance of the labels")
            table = spec.table() if table is None else table
    gamma, normalise = check_gamma(gamma), check_normalise(normalise)
    if not _number(grad_scale):
        raise ValueError("grad_scale must be a finite number, got %r" % (grad_scale,))
    if (dist2 is None) != (table is None):
        raise ValueError("dist2 and table go together")
    cw = None
    if class_weights is not None:
        if not isinstance(class_weights, torch.Tensor):
            class_weights = check_class_weights(class_weights, num_classes=K, schemes=False)
        cw = _device_f32(class_weights, K, dev, "class_weights")
    tab = None
    if dist2 is not None:
        if not is_device_tensor(dist2, torch.int16, device=dev) or dist2.numel() != n * HW:
            raise ValueError("dist2 must be a contiguous int16 tensor of %d elements on %s" % (n * HW, dev))
        tab = _device_f32(table, LOSS_TABLE, dev, "table")
    loss = torch.empty(n, device=dev, dtype=torch.float32)
    sums = torch.empty((n, LOSS_SUMS), device=dev, dtype=torch.float64)
    dlogits = torch.empty_like(logits) if grad else None
    if n:
        need = workspace_bytes(n, HW)
        if workspace is None:
            workspace = torch.empty(need, device=dev, dtype=torch.uint8)
        elif not is_device_tensor(workspace, torch.uint8, device=dev) or workspace.numel() < need or workspace.data_ptr() % 8:
            raise ValueError("workspace must be a contiguous, 8-byte aligned uint8 tensor of at least %d bytes on %s" % (need, dev))
        launch("gsa_loss_softmax", dev, n, K, HW, logits.data_ptr(), labels.data_ptr(), cw.data_ptr() if cw is not None else None,
               dist2.data_ptr() if dist2 is not None else None, tab.data_ptr() if tab is not None else None, gamma,
               NORMALISE[normalise], float(grad_scale), workspace.data_ptr(), sums.data_ptr(), loss.data_ptr(),
               dlogits.data_ptr() if grad else None)
    return loss, sums, dlogits


def region_workspace_bytes(n, classes, HW):
    """gsa_region_workspace_bytes: n * min(ceil(HW / 256), REGION_MAX_BLOCKS) * 3 * classes * 8."""
    size = _lib.load_library().fn("gsa_region_workspace_bytes")(int(n), int(classes), int(HW))
    if size < 0:
        raise ValueError("no workspace for n = %r, classes = %r, HW = %r" % (n, classes, HW))
    return int(size)


def region_loss(logits, labels, alpha=0.5, beta=0.5, smooth=1.0, classes="present", class_weights=None, grad=True, grad_scale=1.0,
                into=None, workspace=None):
    """The region term of csrc/gsa_region.h: per sample the weighted mean over the chosen classes of 1 - TI_k, TI_k the soft
    Tversky index of the softmax against the labels (alpha = beta = 0.5: soft Dice; alpha = beta = 1: soft Jaccard; alpha weighs
    false positives, beta false negatives; ``smooth`` is added to numerator and denominator).
    logits (n, K, H, W) or (n, K, HW) contiguous float32 CUDA tensor, K in 2..16; labels: a contiguous int8 tensor of n * HW
    elements on the same device, a pixel being valid iff its label is in 0 .. K - 1.  ``classes``: "present" (the classes that a
    valid pixel of the sample has) or "all"; ``class_weights``: K numbers or a float32 device tensor of them.  ``grad=False``:
    forward only.  ``into``: a gradient tensor like logits to accumulate into with one fp32 add an element -- the ``dlogits`` of
    ``softmax_loss``, say; it is returned as dlogits, and ignored pixels keep their bits.  ``workspace``: a uint8 device tensor of at
    least ``region_workspace_bytes(n, K, HW)`` bytes to reuse, else one is allocated.
    -> (loss float32 (n,), sums float64 (n, 3, K) = [I, P, G], index float32 (n, K) = TI_k, 0 for a class outside the set, dlogits
    as logits or None); dlogits = grad_scale * d loss[n] / d logits.  Two kernels on the current stream of the logits' device;
    ValueError on anything else; no CPU fallback."""
    import torch
    from ._runtime import is_device_tensor, launch
    if not is_device_tensor(logits, torch.float32, dims=(3, 4)):
        raise ValueError("logits must be a contiguous float32 CUDA tensor (n, K, H, W) or (n, K, HW)")
    n, K = int(logits.shape[0]), int(logits.shape[1])
    HW = int(np.prod(logits.shape[2:]))
    dev = logits.device
    if not MIN_CLASSES <= K <= REGION_MAX_CLASSES or HW <= 0:
        raise ValueError("logits must hold %d..%d classes and at least one pixel, got shape %s"
                         % (MIN_CLASSES, REGION_MAX_CLASSES, tuple(logits.shape)))
    if n * K * HW >= 2 ** 40:
        raise ValueError("logits of %d elements: at most 2^40 - 1" % (n * K * HW))
    if not is_device_tensor(labels, torch.int8, device=dev) or labels.numel() != n * HW:
        raise ValueError("labels must be a contiguous int8 tensor of %d elements on %s" % (n * HW, dev))
    alpha, beta, smooth, classes = check_tversky(alpha, beta, smooth, classes, "region_loss")
    if not _number(grad_scale):
        raise ValueError("grad_scale must be a finite number, got %r" % (grad_scale,))
    cw = None
    if class_weights is not None:
        if not isinstance(class_weights, torch.Tensor):
            class_weights = check_class_weights(class_weights, num_classes=K, schemes=False)
        cw = _device_f32(class_weights, K, dev, "class_weights")
    if into is not None:
        if not grad:
            raise ValueError("into needs grad=True")
        if not is_device_tensor(into, torch.float32, shape=logits.shape, device=dev):
            raise ValueError("into must be a contiguous float32 tensor of shape %s on %s" % (tuple(logits.shape), dev))
    loss = torch.empty(n, device=dev, dtype=torch.float32)
    sums = torch.empty((n, REGION_SUMS, K), device=dev, dtype=torch.float64)
    index = torch.empty((n, K), device=dev, dtype=torch.float32)
    dlogits = (into if into is not None else torch.empty_like(logits)) if grad else None
    if n:
        need = region_workspace_bytes(n, K, HW)
        if workspace is None:
            workspace = torch.empty(need, device=dev, dtype=torch.uint8)
        elif not is_device_tensor(workspace, torch.uint8, device=dev) or workspace.numel() < need or workspace.data_ptr() % 8:
            raise ValueError("workspace must be a contiguous, 8-byte aligned uint8 tensor of at least %d bytes on %s" % (need, dev))
        launch("gsa_region_tversky", dev, n, K, HW, logits.data_ptr(), labels.data_ptr(), cw.data_ptr() if cw is not None else None,
               alpha, beta, smooth, REGION_CLASSES[classes], float(grad_scale), 1 if into is not None else 0, workspace.data_ptr(),
               sums.data_ptr(), index.data_ptr(), loss.data_ptr(), dlogits.data_ptr() if grad else None)
    return loss, sums, index, dlogits
