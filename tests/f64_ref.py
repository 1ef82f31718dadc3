"""Float64 CPU references and comparison rules for the decoder-training kernels (include/gsa_train.h) and, at the end, float64
references of the counter-based inputs (gsa_fill_inputs) and of the evaluation kernel (gsa_segmentation_eval).

Two ways of comparing a kernel result with its reference:

* exact mode -- inputs are small integers (x, dy, w in [-3, 3], integer bias) and every partial sum stays below 2**24,
  so every product and every partial sum is exact in fp32 whatever the summation, MFMA or atomic order.  The kernel
  must then be bit-equal to the float64 reference: a skipped, doubled or misplaced term always shows.
  ``assert_exact`` compares; ``conv_exact_limits`` checks the 2**24 premise from the shape alone.
* bounded mode -- random floats, compared element by element: ``|got - ref| <= rho * bound`` where ``bound`` is the same
  operation applied to the magnitudes of the operands (for a sum of products: the sum of |products|) and
  ``rho = c * 2**-24 * sqrt(N)`` for a dot product of length N (``rho_dot``).  ``assert_bounded`` compares and returns
  the worst ratio ``|got - ref| / (rho * bound)``.

A plain module, imported by the tests; no GPU needed here."""
import math

import torch
import torch.nn.functional as F

U = 2.0 ** -24          # unit roundoff of fp32
EXACT_LIMIT = 2 ** 24   # integers below this are exact in fp32


# ---- references ---------------------------------------------------------------------------------------------------
def conv_ref(x0, x1, w, b, up, dy, dtype=torch.float64):
    """Forward, input gradient and weight / bias gradient of the decoder convolution over concat(x0, x1) (x1 may be
    None), nearest-x2 upsampled when ``up``, padding K // 2 -- by torch autograd on the CPU in ``dtype``.
    -> dict: out (n,Cout,H,W), dxu (gradient w.r.t. the upsampled concat, what gsa_train_conv(transposed=1) writes),
    dx (w.r.t. the concat before upsampling), dw, db."""
    cpu = lambda t: None if t is None else t.detach().to("cpu", dtype)
    x0, x1, w, b, dy = cpu(x0), cpu(x1), cpu(w), cpu(b), cpu(dy)
    xin = (torch.cat([x0, x1], 1) if x1 is not None else x0).requires_grad_(True)
    wr = w.clone().requires_grad_(True)
    br = b.clone().requires_grad_(True) if b is not None else None
    xu = F.interpolate(xin, scale_factor=2, mode="nearest") if up else xin
    xu.retain_grad()
    y = F.conv2d(xu, wr, br, padding=w.shape[2] // 2)
    y.backward(dy)
    return {"out": y.detach(), "dxu": xu.grad, "dx": xin.grad, "dw": wr.grad,
            "db": br.grad if br is not None else dy.sum(dim=(0, 2, 3))}


def conv_bound(x0, x1, w, b, up, dy):
    """The same operations on |x|, |w|, |b|, |dy| in float64: for each output element, the sum of the magnitudes of its
    terms -- the scale that rounding errors of the kernel's sums are measured against."""
    a = lambda t: None if t is None else t.detach().to("cpu", torch.float64).abs()
    return conv_ref(a(x0), a(x1), a(w), a(b), up, a(dy))


def conv_exact_limits(Cin, Cout, K, n, H, W, xmax=3, wmax=3, bmax=0, accumulate=True):
    """Assert that every partial sum of the exact-mode convolution stays below 2**24 (so that fp32 is exact in any
    order), from the shape alone: forward |sum| <= bmax + xmax*wmax*K*K*Cin (twice that with accumulate), input gradient
    xmax*wmax*K*K*Cout (times 4 after the 2x2 sum of upsample2_bwd), weight gradient xmax*xmax*n*H*W, bias gradient
    xmax*n*H*W."""
    fwd = (bmax + xmax * wmax * K * K * Cin) * (2 if accumulate else 1)
    dgrad = 4 * xmax * wmax * K * K * Cout
    wgrad = xmax * xmax * n * H * W
    for what, v in (("forward", fwd), ("dgrad", dgrad), ("wgrad", wgrad)):
        assert v < EXACT_LIMIT, "exact mode needs |partial sums| < 2**24: %s reaches %d" % (what, v)


def small_ints(shape, gen, lo=-3, hi=3):
    """fp32 tensor of integers uniform in [lo, hi]."""
    return torch.randint(lo, hi + 1, shape, generator=gen).to(torch.float32)


# ---- comparisons --------------------------------------------------------------------------------------------------
def assert_exact(got, ref, what=""):
    """Bit equality with a float64 reference whose values are integers below 2**24 (exact mode)."""
    got = got.detach().to("cpu", torch.float64)
    ref = ref.detach().to("cpu", torch.float64)
    assert got.shape == ref.shape, "%s: shape %s vs %s" % (what, tuple(got.shape), tuple(ref.shape))
    assert bool((ref.abs() < EXACT_LIMIT).all()) and bool((ref == ref.round()).all()), "%s: reference leaves exact range" % what
    bad = got != ref
    if bool(bad.any()):
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError("%s: %d of %d elements differ; first at %s: got %r, want %r"
                             % (what, int(bad.sum()), bad.numel(), i, float(got[i]), float(ref[i])))


def rho_dot(N, c):
    """Relative error allowance for fp32 dot products of length N in any order: c * 2**-24 * sqrt(N)."""
    return c * U * math.sqrt(N)


def assert_bounded(got, ref, bound, rho, what="", atol=0.0):
    """|got - ref| <= rho * bound + atol element by element (bound >= 0, float64); with atol 0 an element whose bound is 0
    must be exact.  -> the worst ratio |got - ref| / (rho * bound + atol)."""
    got = got.detach().to("cpu", torch.float64)
    ref = ref.detach().to("cpu", torch.float64)
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(ref)
    assert got.shape == ref.shape, "%s: shape %s vs %s" % (what, tuple(got.shape), tuple(ref.shape))
    err = (got - ref).abs()
    allow = rho * bound + atol
    bad = ~(err <= allow)                   # NaN fails too
    if bool(bad.any()):
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError("%s: %d of %d elements outside rho*bound (rho %.3e); first at %s: got %r, want %r, bound %r"
                             % (what, int(bad.sum()), bad.numel(), rho, i, float(got[i]), float(ref[i]), float(bound[i])))
    pos = allow > 0
    return float((err[pos] / allow[pos]).max()) if bool(pos.any()) else 0.0


# ---- the launch geometry of the persistent kernels -----------------------------------------------------------------
# Restated from gan-segmentation_amd/csrc/gsa_train.hip so that a test can assert that its shape really makes blocks and
# waves walk several units; the line numbers are those of the formulas restated.  If the launch code changes, change
# these with it.
CONV_BLOCKS = 2048      # gsa_train_conv, gsa_train.hip:541        gx = ceil(2048 / (otiles * n))
WGRAD_BLOCKS = 1024     # gsa_train_conv_wgrad, gsa_train.hip:567,575  gx = ceil(1024 / pairs)


def mfma_path(H, W):
    """gsa_train_conv / gsa_train_conv_wgrad take the matrix-core kernels when W % 4 == 0 and H*W % 16 == 0
    (and 16-byte aligned tensors, which torch allocations are)."""
    return W % 4 == 0 and (H * W) % 16 == 0


def conv_units_per_block(n, Cout, H, W):
    """Fewest 64-pixel units a block of conv_mfma_kernel walks.  gsa_train.hip:540-543: groups = (H*W/16 + 3) / 4,
    otiles = ceil(Cout/16), gx = min(ceil(2048 / (otiles*n)), groups), grid (gx, otiles, n); :113,133: block (x, z)
    walks u = x + gx*z, step gx*n, over units = n*groups."""
    assert mfma_path(H, W)
    groups = (H * W // 16 + 3) // 4
    otiles = (Cout + 15) // 16
    gx = min((CONV_BLOCKS + otiles * n - 1) // (otiles * n), groups)
    return (n * groups) // (gx * n)


def wgrad_units_per_wave(n, Cin, Cout, H, W):
    """Fewest 64-pixel units a wave of wgrad_mfma_kernel walks.  gsa_train.hip:566-568: units = n*ceil(H*W/64),
    pairs = ceil(Cout/16)*ceil(Cin/16), gx = clamp(ceil(1024/pairs), 1, ceil(units/4)); :281,283: wave w of block x walks
    u = 4x + w, step 4*gx."""
    assert mfma_path(H, W)
    units = n * ((H * W + 63) // 64)
    pairs = ((Cout + 15) // 16) * ((Cin + 15) // 16)
    gx = max(1, min((WGRAD_BLOCKS + pairs - 1) // pairs, (units + 3) // 4))
    return units // (4 * gx)


def wgrad_tiles_per_block(n, Cin, Cout, H, W):
    """Fewest 16x16 tiles a block of the vector-ALU wgrad_kernel walks.  gsa_train.hip:575-576: work = tiles*n,
    gx = clamp(ceil(1024/pairs), 1, work); :205: block x walks work items x, x + gx, ..."""
    assert not mfma_path(H, W)
    work = ((H + 15) // 16) * ((W + 15) // 16) * n
    pairs = ((Cout + 15) // 16) * ((Cin + 15) // 16)
    gx = max(1, min((WGRAD_BLOCKS + pairs - 1) // pairs, work))
    return work // gx


# ---- float64 references of the kernels around the convolution path --------------------------------------------------
# numpy only; the references above need torch's autograd, these are plain formulas.
def box_muller_f64(u):
    """The transform of fill_normal_kernel in float64.  u: (..., 4) uniforms in (0, 1] -- oracle/ref_philox.uniforms, the fp32
    values the kernel forms from the Philox words (their integer stream is pinned by the Random123 known-answer vectors of
    tests/test_philox.py); they are taken as exact, and everything after them -- the logarithm, the root, 2 pi u, cosine, sine
    and the products -- is float64 here and fp32 in the kernel and in oracle/ref_philox.fill_normal.
    -> (..., 4) float64: (r0 cos a0, r0 sin a0, r1 cos a1, r1 sin a1) with r = sqrt(-2 ln u_even), a = 2 pi u_odd."""
    import numpy as np
    u = np.asarray(u, np.float64)
    out = np.empty(u.shape, np.float64)
    for h in range(2):
        r = np.sqrt(-2.0 * np.log(u[..., 2 * h]))
        a = (2.0 * np.pi) * u[..., 2 * h + 1]
        out[..., 2 * h] = r * np.cos(a)
        out[..., 2 * h + 1] = r * np.sin(a)
    return out


def fill_normal_f64(n, per_sample, first_index, plane, seed):
    """-> (n, per_sample) float64: what gsa_fill_inputs writes for (seed, plane, samples first_index ..), in float64."""
    from oracle import ref_philox
    return box_muller_f64(ref_philox.uniforms(n, per_sample, first_index, plane, seed)).reshape(n, per_sample)


# the largest |x| Box-Muller can give: the smallest uniform is (0 + 0.5) * 2^-24 = 2^-25; the factor allows for the fp32 roundings of
# the logarithm, the root and the product
NORMAL_ABS_MAX = math.sqrt(-2.0 * math.log(2.0 ** -25)) * (1.0 + 2.0 ** -20)


def weighted_softmax_ce_f64(logits, labels):
    """(N,K,H,W) logits, (N,H,W) integer labels -> (N,) float64: the mean over ALL H*W pixels of -log_softmax(logits)[label] on the
    pixels whose label is in 0..K-1 and 0 elsewhere (-1 = ignore; a label >= K counts as ignored, as gsa_segmentation_eval
    treats it).  Every step in float64, one sample at a time."""
    import numpy as np
    N, K = logits.shape[:2]
    out = np.zeros(N, np.float64)
    for i in range(N):
        x = logits[i].astype(np.float64).reshape(K, -1)
        lab = np.asarray(labels[i]).reshape(-1).astype(np.int64)
        ok = (lab >= 0) & (lab < K)
        m = x.max(axis=0)
        lse = m + np.log(np.exp(x - m).sum(axis=0))
        picked = np.take_along_axis(x, np.clip(lab, 0, K - 1)[None], axis=0)[0]
        out[i] = np.where(ok, lse - picked, 0.0).sum() / lab.size
    return out


def confusion_i64(logits, labels, K):
    """-> (K, K) int64: counts of (label, argmax) over the pixels whose label is in 0..K-1; argmax takes the first maximum."""
    import numpy as np
    pred = np.argmax(logits, axis=1).reshape(-1)
    lab = np.asarray(labels).reshape(-1).astype(np.int64)
    ok = (lab >= 0) & (lab < K)
    return np.bincount(lab[ok] * K + pred[ok], minlength=K * K).reshape(K, K).astype(np.int64)
