"""ctypes binding of the on-device mask clean-up (include/gsa_mask.h, csrc/gsa_mask.hip) -- the
counterpart of reference utils.morph_mask (utils.py:105-109): a 5x5 close followed by a 5x5 open of a class-index mask.

``morph_mask(mask)`` enqueues one kernel on the current stream of ``mask``'s device and returns the cleaned mask;
``ImageGenerator(..., mask_morph=True)`` applies it to the mask of every fused call.  No CPU fallback.

Also the binding of the mask components (include/gsa_components.h, csrc/gsa_components.hip), which the
reference does not have: ``components(mask)`` labels the connected components of equal value and gives their areas,
``despeckle(mask, min_area)`` replaces every component smaller than ``min_area`` pixels -- a clean-up with an area threshold where
the morphology has a window size -- and can return per-sample component counts; ``ImageGenerator(..., mask_min_area=k)`` applies it
to the mask of every fused call, after ``mask_morph``.

And the binding of the boundary distance (include/gsa_boundary.h, csrc/gsa_boundary.hip), which the
reference does not have either: ``boundary_distance(mask)`` gives every pixel's squared Euclidean distance to the nearest pixel of
another value, up to a radius; ``ignore_band(mask, radius)`` writes a label (255, the value the consumers ignore) wherever that
distance is at most ``radius``^2 -- VOC's void border, on both sides of every class boundary; ``ImageGenerator(...,
mask_ignore_band=r)`` applies it to the mask of every fused call, last.

And the binding of the image-guided refinement (csrc/gsa_refine.h, csrc/gsa_refine.hip), the one operator here
that looks at the pair's image: ``refine(img, mask)`` gives every pixel the class its neighbours of similar colour agree on -- a
joint bilateral vote, in integers, with the weights of ``refine_tables``; ``ImageGenerator(..., mask_refine=k)`` applies k passes of
it to the mask of every fused call, FIRST.

And the binding of the mask agreement (csrc/gsa_compare.h, csrc/gsa_compare.hip), the one operator here that
takes TWO masks: ``compare(pred, target, band)`` counts per sample the pixels of every (band code, target slot, prediction slot)
combination -- the table ``metrics.MaskAgreement`` reads accuracy, mIoU, trimap accuracy and boundary IoU from.
``apply_filters(img, mask, classes, ...)`` is the clean-up chain of ``ImageGenerator`` as a free function on any pair, so that a
chain can be held against an annotation before a dataset run (``SegSolver.evaluate_masks``)."""
import numpy as np
import torch

from ._runtime import is_device_tensor, launch

MAX_EXTENT = 65535

# The summary row of ``despeckle(..., return_stats=True)``: COMP_ROW int64 words per sample (include/gsa_components.h).  Slots as
# pair_stats: slot k < 8 is mask value k, slot 8 every value >= 8.
COMP_SLOTS = 9
COMP_NCOMP = 0              # + s: number of components whose value falls in slot s
COMP_LARGEST = 9            # + s: the largest area among them, 0 if there is none
COMP_SMALL = 18             # number of components with area < min_area
COMP_SMALL_PIXELS = 19      # sum of their areas
COMP_ROW = 20
FILL_NEIGHBOUR = -1
CONNECTIVITIES = (4, 8)
MAX_AREA = 2 ** 31 - 1

# include/gsa_boundary.h
BOUNDARY_FAR = 32767        # dist2 of a pixel with no other value within the radius
BOUNDARY_MAX_RADIUS = 32

# csrc/gsa_refine.h
REFINE_MAX_RADIUS = 5
REFINE_MAX_CLASSES = 8
REFINE_MAX_ITERATIONS = 8
REFINE_TABLE_BYTES = 256 + 11 * 11

# csrc/gsa_compare.h: word f * 81 + slot(target) * 9 + slot(pred) of a row, f = (in the target's band) + 2 * (in the prediction's)
COMPARE_SLOTS = 9
COMPARE_BANDS = 4
COMPARE_ROW = COMPARE_BANDS * COMPARE_SLOTS * COMPARE_SLOTS


def _check(t, what):
    if not is_device_tensor(t, torch.uint8, dims=(2, 3)):
        raise ValueError("%s must be a contiguous uint8 CUDA tensor (H, W) or (n, H, W)" % what)


def _other_tensor(out, what, dtype, mask):
    """``out`` checked as the result ``what`` of ``mask``'s shape: contiguous, of ``dtype``, on the same device, not overlapping it."""
    if not is_device_tensor(out, dtype, shape=mask.shape, device=mask.device):
        raise ValueError("%s must be a contiguous %s tensor %s on %s" % (what, str(dtype).replace("torch.", ""), tuple(mask.shape), mask.device))
    a, b, size, other = mask.data_ptr(), out.data_ptr(), mask.numel(), out.numel() * out.element_size()
    if out is mask or (size and a < b + other and b < a + size):
        raise ValueError("%s must not be, or overlap, the input mask" % what)
    return out


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
    out = torch.empty_like(mask) if out is None else _other_tensor(out, "out", torch.uint8, mask)
    if n:
        launch("gsa_mask_morph", mask.device, n, H, W, mask.data_ptr(), out.data_ptr())
    return out


def check_connectivity(v, what="connectivity"):
    """4 or 8 as an int (ValueError otherwise; a bool is not a number here)."""
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or int(v) not in CONNECTIVITIES:
        raise ValueError("%s must be 4 or 8, got %r" % (what, v))
    return int(v)


def check_min_area(v, what="min_area"):
    """An area threshold in pixels as an int: 0 .. 2^31 - 1 (0 and 1 change nothing).  ValueError otherwise."""
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= MAX_AREA:
        raise ValueError("%s must be an int in 0..%d, got %r" % (what, MAX_AREA, v))
    return int(v)


def check_fill(v, what="fill"):
    """``"neighbour"`` or an int 0..255 -> the C entry's fill argument (-1 for "neighbour").  ValueError otherwise."""
    if isinstance(v, str) and v == "neighbour":
        return FILL_NEIGHBOUR
    if isinstance(v, (bool, str)) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= 255:
        raise ValueError("%s must be \"neighbour\" or an int in 0..255, got %r" % (what, v))
    return int(v)


def _plane_shape(mask, who):
    _check(mask, "mask")
    H, W = mask.shape[-2:]
    if not 1 <= H <= MAX_EXTENT or not 1 <= W <= MAX_EXTENT or H * W >= 2 ** 31:
        raise ValueError("%s takes masks whose sides are 1..%d px with fewer than 2^31 pixels, got %dx%d" % (who, MAX_EXTENT, H, W))
    return (mask.shape[0] if mask.dim() == 3 else 1), H, W


def _scratch_pair(scratch, mask):
    """The (labels, areas) working tensors of a call: new ones, or the caller's checked pair."""
    if scratch is None:
        return (torch.empty(mask.shape, dtype=torch.int32, device=mask.device),
                torch.empty(mask.shape, dtype=torch.int32, device=mask.device))
    labels, areas = scratch
    for t in (labels, areas):
        if not is_device_tensor(t, torch.int32, shape=mask.shape, device=mask.device):
            raise ValueError("scratch must be two contiguous int32 tensors %s on %s" % (tuple(mask.shape), mask.device))
    if labels.data_ptr() == areas.data_ptr() and labels.numel():
        raise ValueError("scratch must be two different tensors")
    return labels, areas


def components(mask, connectivity=8):
    """mask (H, W) or (n, H, W) contiguous uint8 CUDA tensor -> ``(labels, areas)``, two int32 tensors of the same shape: for every
    pixel the smallest raster index ``y * W + x`` of its connected component (its first pixel) and the component's pixel count.  A
    component is a maximal set of pixels of equal raw value joined by horizontal and vertical steps (``connectivity=4``) or by
    diagonal ones as well (8, cv2's default and ours); every value forms components, 0 included; every image of a batch is a plane
    of its own (the rule of include/gsa_components.h).  Enqueued on the current stream of ``mask``'s device; the input is not
    written.  ValueError on anything else; no CPU fallback."""
    n, H, W = _plane_shape(mask, "components")
    connectivity = check_connectivity(connectivity)
    labels, areas = _scratch_pair(None, mask)
    if n:
        launch("gsa_mask_components", mask.device, n, H, W, connectivity, 0, FILL_NEIGHBOUR, mask.data_ptr(), labels.data_ptr(),
               areas.data_ptr(), None, None)
    return labels, areas


def despeckle(mask, min_area, connectivity=8, fill="neighbour", out=None, return_stats=False, scratch=None):
    """mask (H, W) or (n, H, W) contiguous uint8 CUDA tensor -> a tensor of the same shape (new, or ``out``, which must not overlap
    ``mask``) in which every pixel of a component (see ``components``) of fewer than ``min_area`` pixels is replaced: by ``fill`` if
    that is an int 0..255, or with ``fill="neighbour"`` by the input value of the pixel left of the component's first pixel (the one
    above it if the first pixel is in column 0) -- for an enclosed island or hole the enclosing region; the component that holds
    pixel (0, 0) has no such neighbour and is kept.  One pass on the input's values: a small speck nested in a small speck takes
    the outer speck's input value, so a second call can still change something.  ``min_area <= 1`` changes nothing.

    ``return_stats=True`` returns ``(out, rows)`` with ``rows`` (n, COMP_ROW) int64 on the device (``(COMP_ROW,)`` for a 2-D mask):
    component counts and largest areas per value slot, and the number and pixel sum of the components below ``min_area``
    (``COMP_*`` above); they do not depend on ``fill``.  ``scratch``: two int32 tensors of ``mask``'s shape to work in (8 bytes per
    pixel) instead of new ones; they hold the labels and areas afterwards.  Enqueued on the current stream of ``mask``'s device; the
    input is not written.  ValueError on anything else; no CPU fallback."""
    n, H, W = _plane_shape(mask, "despeckle")
    min_area, connectivity, fill = check_min_area(min_area), check_connectivity(connectivity), check_fill(fill)
    if out is not None:
        _other_tensor(out, "out", torch.uint8, mask)
    labels, areas = _scratch_pair(scratch, mask)
    if out is None:
        out = torch.empty_like(mask)
    rows = torch.empty((n, COMP_ROW), dtype=torch.int64, device=mask.device) if return_stats else None
    if n:
        launch("gsa_mask_components", mask.device, n, H, W, connectivity, min_area, fill, mask.data_ptr(), labels.data_ptr(), areas.data_ptr(),
               out.data_ptr(), rows.data_ptr() if return_stats else None)
    if return_stats:
        return out, (rows[0] if mask.dim() == 2 else rows)
    return out


def check_band(v, what="radius"):
    """A band radius in pixels as an int: 0 .. 32, 0 meaning off (only the ``ImageGenerator`` keyword and the config key take it;
    the functions below want 1 .. 32).  ValueError otherwise; a bool is not a number here."""
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= BOUNDARY_MAX_RADIUS:
        raise ValueError("%s must be an int in 0..%d, got %r" % (what, BOUNDARY_MAX_RADIUS, v))
    return int(v)


def check_label(v, what="label"):
    """The value the band writes as an int: 0 .. 255.  ValueError otherwise."""
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= 255:
        raise ValueError("%s must be an int in 0..255, got %r" % (what, v))
    return int(v)


def _radius(v, what):
    r = check_band(v, what)
    if r == 0:
        raise ValueError("%s must be an int in 1..%d, got %r" % (what, BOUNDARY_MAX_RADIUS, v))
    return r


def boundary_distance(mask, max_radius=BOUNDARY_MAX_RADIUS, out=None):
    """mask (H, W) or (n, H, W) contiguous uint8 CUDA tensor -> an int16 tensor of the same shape (new, or ``out``): every pixel's
    squared Euclidean distance to the nearest pixel of its plane with another raw value where that is at most ``max_radius``^2
    (``max_radius`` 1..32), and ``BOUNDARY_FAR`` (32767) elsewhere.  The outside of the image is not another value: an image edge
    makes no boundary, and a constant plane is FAR everywhere (the rule of include/gsa_boundary.h).  What boundary-weighted
    losses, one-sided bands and trimaps are built from.  Enqueued on the current stream of ``mask``'s device; the input is not
    written.  ValueError on anything else; no CPU fallback."""
    n, H, W = _plane_shape(mask, "boundary_distance")
    radius = _radius(max_radius, "max_radius")
    dist2 = torch.empty(mask.shape, dtype=torch.int16, device=mask.device) if out is None else _other_tensor(out, "out", torch.int16, mask)
    if n:
        launch("gsa_mask_boundary", mask.device, n, H, W, radius, 0, mask.data_ptr(), dist2.data_ptr(), None)
    return dist2


def ignore_band(mask, radius, label=255, out=None, return_distance=False):
    """mask (H, W) or (n, H, W) contiguous uint8 CUDA tensor -> a tensor of the same shape (new, or ``out``, which must not overlap
    ``mask``) that holds ``label`` (0..255) wherever a pixel of another value lies within ``radius`` (1..32) pixels, Euclidean,
    ``radius``^2 inclusive, and the input's value elsewhere: a band on both sides of every class boundary.  One pass on the input's
    values; a pixel that already holds ``label`` is a value like any other; image edges make no band.
    ``return_distance=True`` returns ``(out, dist2)`` with ``dist2`` as ``boundary_distance(mask, radius)`` gives it, from the same
    launch.  Enqueued on the current stream of ``mask``'s device; the input is not written.  ValueError on anything else; no CPU
    fallback."""
    n, H, W = _plane_shape(mask, "ignore_band")
    radius, label = _radius(radius, "radius"), check_label(label)
    out = torch.empty_like(mask) if out is None else _other_tensor(out, "out", torch.uint8, mask)
    dist2 = torch.empty(mask.shape, dtype=torch.int16, device=mask.device) if return_distance else None
    if n:
        launch("gsa_mask_boundary", mask.device, n, H, W, radius, label, mask.data_ptr(), dist2.data_ptr() if return_distance else None,
               out.data_ptr())
    return (out, dist2) if return_distance else out


def check_refine_iterations(v, what="iterations"):
    """A number of refinement passes as an int: 0 .. 8, 0 meaning off (only the ``ImageGenerator`` keyword and the config key take it;
    ``refine`` wants 1 .. 8).  ValueError otherwise; a bool is not a number here."""
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= REFINE_MAX_ITERATIONS:
        raise ValueError("%s must be an int in 0..%d, got %r" % (what, REFINE_MAX_ITERATIONS, v))
    return int(v)


def check_refine_radius(v, what="radius"):
    """The window radius of the vote as an int: 1 .. 5.  ValueError otherwise."""
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= int(v) <= REFINE_MAX_RADIUS:
        raise ValueError("%s must be an int in 1..%d, got %r" % (what, REFINE_MAX_RADIUS, v))
    return int(v)


def check_refine_classes(v, what="classes"):
    """The class count K of the vote as an int: 2 .. 8; mask values >= K are frozen.  ValueError otherwise."""
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 2 <= int(v) <= REFINE_MAX_CLASSES:
        raise ValueError("%s must be an int in 2..%d, got %r" % (what, REFINE_MAX_CLASSES, v))
    return int(v)


def check_refine_sigma(v, what="sigma"):
    """A width of the vote's weights as a float: finite and > 0.  ValueError otherwise; a bool is not a number here."""
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v) or not float(v) > 0.0:
        raise ValueError("%s must be a finite number > 0, got %r" % (what, v))
    return float(v)


def refine_tables(radius=3, sigma_space=2.0, sigma_colour=32.0):
    """The weights of the vote as the C entry reads them: a numpy (377,) uint8 array, ``wr[256]`` then ``ws[11][11]`` row-major with the
    entry of the offset (dy, dx) at ``(dy + 5) * 11 + (dx + 5)``, computed in float64:

        wr[d]      = rint(255 * exp(-d^2 / (2 * sigma_colour^2)))
        ws[dy][dx] = max(1, rint(255 * exp(-(dx^2 + dy^2) / (2 * sigma_space^2))))  inside the radius, 0 outside

    ``d`` is the SUM over the channels of the absolute differences of two pixels, clamped to 255 -- not a Euclidean norm and not a
    mean: for an RGB pair it is up to three times a per-channel difference, and ``sigma_colour`` is in those units."""
    radius = check_refine_radius(radius)
    sigma_space, sigma_colour = check_refine_sigma(sigma_space, "sigma_space"), check_refine_sigma(sigma_colour, "sigma_colour")
    d = np.arange(256, dtype=np.float64)
    wr = np.rint(255.0 * np.exp(-d * d / (2.0 * sigma_colour * sigma_colour)))
    o = np.arange(-REFINE_MAX_RADIUS, REFINE_MAX_RADIUS + 1, dtype=np.float64)
    ws = np.maximum(1.0, np.rint(255.0 * np.exp(-(o[:, None] ** 2 + o[None, :] ** 2) / (2.0 * sigma_space * sigma_space))))
    ws[(np.abs(o)[:, None] > radius) | (np.abs(o)[None, :] > radius)] = 0.0
    return np.concatenate([wr, ws.reshape(-1)]).astype(np.uint8)


_device_tables = {}


def _tables_on(tables, device, radius, sigma_space, sigma_colour):
    """The 377 weights as a uint8 tensor on ``device``: a device tensor is checked; a numpy table, or the one of the parameters, is
    uploaded once per device and content."""
    if isinstance(tables, torch.Tensor):
        if not is_device_tensor(tables, torch.uint8, shape=(REFINE_TABLE_BYTES,), device=device):
            raise ValueError("tables must be a contiguous uint8 tensor (%d,) on %s" % (REFINE_TABLE_BYTES, device))
        return tables
    if tables is None:
        key = (str(device), radius, sigma_space, sigma_colour)
    else:
        tables = np.ascontiguousarray(tables)
        if tables.shape != (REFINE_TABLE_BYTES,) or tables.dtype != np.uint8:
            raise ValueError("tables must be a (%d,) uint8 array (refine_tables), got %s %s" % (REFINE_TABLE_BYTES, tables.shape, tables.dtype))
        key = (str(device), tables.tobytes())
    if key not in _device_tables:
        host = refine_tables(radius, sigma_space, sigma_colour) if tables is None else tables.copy()
        _device_tables[key] = torch.from_numpy(host).to(device)
    return _device_tables[key]


def refine(img, mask, iterations=1, radius=3, classes=8, tables=None, sigma_space=2.0, sigma_colour=32.0, out=None, scratch=None):
    """img (H, W, C) or (n, H, W, C) and mask (H, W) or (n, H, W), contiguous uint8 CUDA tensors of one pair batch, C in 1..4 -> a
    tensor of ``mask``'s shape (new, or ``out``, which must not overlap ``mask``): ``iterations`` (1..8) passes of the joint
    bilateral vote of csrc/gsa_refine.h.  In a pass every pixel whose value is below ``classes`` (2..8) takes the class with the
    largest sum of ``ws[dy][dx] * wr[d]`` over the pixels of its (2 * ``radius`` + 1)^2 window (``radius`` 1..5) that lie in the same
    image and hold a class, ``d`` being the summed absolute colour difference to the pixel itself; it keeps its own value on a tie
    with it, and takes the smallest class on any other tie.  Values >= ``classes`` -- the ignore label 255 -- stay and cast no vote.

    ``tables``: the 377 weights (``refine_tables``) as a numpy array or a device tensor; None takes those of ``radius``,
    ``sigma_space`` and ``sigma_colour``.  A numpy table is uploaded once per device.  ``scratch``: a uint8 tensor of ``mask``'s shape
    for the passes before the last to alternate with ``out`` (the last pass writes ``out``) instead of a new one; it must overlap
    neither ``mask`` nor ``out``.  Enqueued on the current stream of ``mask``'s device; ``img`` and ``mask`` are not written.
    ValueError on anything else; no CPU fallback."""
    n, H, W = _plane_shape(mask, "refine")
    if not is_device_tensor(img, torch.uint8, dims=(mask.dim() + 1,), device=mask.device) or tuple(img.shape[:-1]) != tuple(mask.shape) \
            or not 1 <= img.shape[-1] <= 4:
        raise ValueError("img must be a contiguous uint8 tensor %s + (C,) with C in 1..4 on %s" % (tuple(mask.shape), mask.device))
    iterations = check_refine_iterations(iterations)
    if iterations == 0:
        raise ValueError("iterations must be an int in 1..%d, got %r" % (REFINE_MAX_ITERATIONS, iterations))
    radius, classes = check_refine_radius(radius), check_refine_classes(classes)
    if tables is None:
        sigma_space, sigma_colour = check_refine_sigma(sigma_space, "sigma_space"), check_refine_sigma(sigma_colour, "sigma_colour")
    dev_tables = _tables_on(tables, mask.device, radius, sigma_space, sigma_colour)
    out = torch.empty_like(mask) if out is None else _other_tensor(out, "out", torch.uint8, mask)
    if iterations > 1:
        scratch = torch.empty_like(mask) if scratch is None else _other_tensor(scratch, "scratch", torch.uint8, mask)
        _other_tensor(scratch, "scratch", torch.uint8, out)
    src = mask
    for i in range(iterations):
        dst = out if (iterations - 1 - i) % 2 == 0 else scratch
        if n:
            launch("gsa_mask_refine", mask.device, n, H, W, img.shape[-1], classes, radius, img.data_ptr(), src.data_ptr(),
                   dev_tables.data_ptr(), dst.data_ptr())
        src = dst
    return out


def _overlaps(a, b):
    """Whether the memory of two tensors overlaps (an empty one overlaps nothing)."""
    pa, pb, sa, sb = a.data_ptr(), b.data_ptr(), a.numel() * a.element_size(), b.numel() * b.element_size()
    return bool(sa and sb and pa < pb + sb and pb < pa + sa)


def compare(pred, target, band=0, out=None, scratch=None):
    """pred and target (H, W) or (n, H, W), contiguous uint8 CUDA tensors of equal shape on one device -> an int64 tensor
    (n, COMPARE_ROW) on that device ((COMPARE_ROW,) for 2-D masks; new, or ``out``): per sample the number of pixels of every
    combination of band code, target value and predicted value (the rule of csrc/gsa_compare.h).  Word ``f * 81 + slot(target) * 9 +
    slot(pred)`` with ``slot(v) = min(v, 8)`` -- the values 0..7 each, everything from 8 up together, the ignore label 255 included
    -- and ``f = (the pixel lies in target's band) + 2 * (it lies in pred's band)``.  A mask's band is what ``ignore_band(mask,
    band)`` would overwrite: the pixels within ``band`` px, Euclidean, of a pixel of another value of the same mask; image edges make
    no band.  ``band`` is 0..32; with 0 no band is computed and ``f`` is 0 everywhere, so the words from 81 on are zero.  With
    ``band > 0`` ``boundary_distance(.., max_radius=band)`` runs on both masks first, into ``scratch`` (two int16 tensors of the masks'
    shape: target's distances, then pred's) when given.  The 324 words of a sample sum to H * W; every word of the result is
    overwritten.  ``rows.view(-1, 4, 9, 9)`` indexes it as [band code, target slot, prediction slot]; ``metrics.MaskAgreement`` turns
    it into accuracy, mIoU, trimap accuracy and boundary IoU.  Enqueued on the current stream of the masks' device; the inputs are
    not written.  ValueError on anything else; no CPU fallback."""
    n, H, W = _plane_shape(pred, "compare")
    if not is_device_tensor(target, torch.uint8, shape=pred.shape, device=pred.device):
        raise ValueError("target must be a contiguous uint8 tensor %s on %s, as pred is" % (tuple(pred.shape), pred.device))
    band = check_band(band, "band")
    shapes = ((n, COMPARE_ROW),) if pred.dim() == 3 else ((1, COMPARE_ROW), (COMPARE_ROW,))
    if out is None:
        out = torch.empty((n, COMPARE_ROW), dtype=torch.int64, device=pred.device)
    elif not is_device_tensor(out, torch.int64, device=pred.device) or tuple(out.shape) not in shapes:
        raise ValueError("out must be a contiguous int64 tensor %s on %s" % (" or ".join(str(s) for s in shapes), pred.device))
    elif _overlaps(out, pred) or _overlaps(out, target):
        raise ValueError("out must not overlap pred or target")
    dist = (None, None)
    if scratch is not None:
        if not isinstance(scratch, (tuple, list)) or len(scratch) != 2 or \
                not all(is_device_tensor(t, torch.int16, shape=pred.shape, device=pred.device) for t in scratch):
            raise ValueError("scratch must be two contiguous int16 tensors %s on %s" % (tuple(pred.shape), pred.device))
        if _overlaps(scratch[0], scratch[1]) or any(_overlaps(t, o) for t in scratch for o in (pred, target, out)):
            raise ValueError("scratch must be two different tensors that overlap neither mask nor out")
    if band:
        dist = (boundary_distance(target, band, out=None if scratch is None else scratch[0]),
                boundary_distance(pred, band, out=None if scratch is None else scratch[1]))
    if n:
        launch("gsa_mask_compare", pred.device, n, H, W, band, target.data_ptr(), pred.data_ptr(),
               dist[0].data_ptr() if band else None, dist[1].data_ptr() if band else None, out.data_ptr())
    return out[0] if pred.dim() == 2 and out.dim() == 2 else out


FILTER_DEFAULTS = dict(refine=0, refine_radius=3, refine_sigma_space=2.0, refine_sigma_colour=32.0, morph=False, min_area=0,
                       connectivity=8, fill="neighbour", ignore_band=0, ignore_label=255)


def check_filters(what="filters", **keywords):
    """The keywords of ``apply_filters`` checked with the ``check_*`` functions above, without a tensor in sight -> the complete
    keyword dict, defaults filled in (``fill`` as given, not as the C entry's number).  ValueError on a bad value and on a name that
    is no keyword of ``apply_filters``."""
    unknown = sorted(set(keywords) - set(FILTER_DEFAULTS))
    if unknown:
        raise ValueError("%s: %s is no keyword of apply_filters (%s)" % (what, ", ".join(map(repr, unknown)), ", ".join(FILTER_DEFAULTS)))
    kw = dict(FILTER_DEFAULTS, **keywords)
    if not isinstance(kw["morph"], bool):
        raise ValueError("%s: morph must be True or False, got %r" % (what, kw["morph"]))
    check_fill(kw["fill"], what + ": fill")
    return dict(kw, refine=check_refine_iterations(kw["refine"], what + ": refine"),
                refine_radius=check_refine_radius(kw["refine_radius"], what + ": refine_radius"),
                refine_sigma_space=check_refine_sigma(kw["refine_sigma_space"], what + ": refine_sigma_space"),
                refine_sigma_colour=check_refine_sigma(kw["refine_sigma_colour"], what + ": refine_sigma_colour"),
                min_area=check_min_area(kw["min_area"], what + ": min_area"),
                connectivity=check_connectivity(kw["connectivity"], what + ": connectivity"),
                ignore_band=check_band(kw["ignore_band"], what + ": ignore_band"),
                ignore_label=check_label(kw["ignore_label"], what + ": ignore_label"))


_refine, _ignore_band = refine, ignore_band         # apply_filters has keywords of these names


def apply_filters(img, mask, classes, refine=0, refine_radius=3, refine_sigma_space=2.0, refine_sigma_colour=32.0, morph=False, min_area=0,
                  connectivity=8, fill="neighbour", ignore_band=0, ignore_label=255):
    """The mask clean-up chain of ``ImageGenerator`` (its ``mask_*`` keywords without the prefix) on any pair, in its order: ``refine``
    passes of ``refine(img, mask, classes=classes)`` with the three ``refine_*`` parameters, then ``morph_mask`` if ``morph``, then
    ``despeckle(min_area, connectivity, fill)`` if ``min_area > 1``, then ``ignore_band(ignore_band, ignore_label)`` if ``ignore_band >
    0``.  img (H, W, C) or (n, H, W, C) and mask (H, W) or (n, H, W) as ``refine`` takes them; ``classes`` 2..8, the class count the
    refinement votes among.  Every keyword is checked before any device work, whether its stage is on or not.  Returns a new tensor;
    with everything off, ``mask`` itself.  ``img`` is only looked at when ``refine > 0``."""
    kw = check_filters(refine=refine, refine_radius=refine_radius, refine_sigma_space=refine_sigma_space, refine_sigma_colour=refine_sigma_colour,
                       morph=morph, min_area=min_area, connectivity=connectivity, fill=fill, ignore_band=ignore_band, ignore_label=ignore_label)
    classes = check_refine_classes(classes)
    _check(mask, "mask")
    if kw["refine"]:
        mask = _refine(img, mask, kw["refine"], kw["refine_radius"], classes, sigma_space=kw["refine_sigma_space"],
                       sigma_colour=kw["refine_sigma_colour"])
    if kw["morph"]:
        mask = morph_mask(mask)
    if kw["min_area"] > 1:
        mask = despeckle(mask, kw["min_area"], kw["connectivity"], kw["fill"])
    if kw["ignore_band"]:
        mask = _ignore_band(mask, kw["ignore_band"], kw["ignore_label"])
    return mask
