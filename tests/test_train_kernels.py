"""The decoder-training kernels (include/gsa_train.h) against float64 CPU references, at the shapes real training runs
(batch 1 at up to 1024 px) and at the edges of their staging and grid-stride loops.

Two comparison modes (tests/f64_ref.py):
* exact -- small-integer inputs whose partial sums all stay below 2**24: the kernel must be BIT-EQUAL to float64,
  whatever its summation, MFMA or atomic order;
* bounded -- random floats, element by element: |got - ref| <= rho * bound with bound = the same operation on the
  magnitudes of the operands, rho = C_DOT * 2**-24 * sqrt(N) for a dot product of length N, and per-operator bounds for
  BatchNorm, softmax-CE and Adam (stated at each test).  The worst ratio |got - ref| / (rho * bound) seen is printed at
  the end of the module (pytest -s).

Measured on an MI355X, worst |got - ref| / (rho * bound) over the module with C_DOT = 2: forward 0.33, dgrad 0.51,
upsample2_bwd 0.09, wgrad 0.054, bias gradient 0.010; BatchNorm 0.28, softmax-CE 0.11, Adam 0.29 at C_BN = 16, C_CE = 8,
C_ADAM = 8 (the constants below are half those: about twice the measured worst).  Every exact-mode case is bit-equal.
The module takes about a minute on a 16-CPU slot (the float64 references dominate)."""
import numpy as np
import pytest

from tests import f64_ref as R

pytestmark = pytest.mark.gpu

C_DOT = 2.0      # conv, dgrad, wgrad, bias gradient, upsample2_bwd: rho = C_DOT * 2**-24 * sqrt(N)
C_BN = 8.0       # BatchNorm: rho = C_BN * 2**-24 against the bounds of _bn_ref
C_CE = 2.0       # softmax-CE: rho = C_CE * 2**-24 against the bounds of test_softmax_ce
C_ADAM = 4.0     # Adam: rho = C_ADAM * 2**-24 against the bounds of test_adam_add_upsample_past_grid_cap

WORST = {}


def _note(what, ratio):
    WORST[what] = max(WORST.get(what, 0.0), ratio)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nworst |got - ref| / (rho * bound):")
    for k in sorted(WORST):
        print("  %-12s %.4f" % (k, WORST[k]))


@pytest.fixture(scope="module")
def T():
    import torch
    assert torch.cuda.is_available()
    return torch


def _d(t):
    return None if t is None else t.to("cuda").contiguous()


# ---- convolution, input gradient, weight gradient -----------------------------------------------------------------
# (n, C0, C1, Cout, K, up, Hs, Ws, persistent): persistent cases must make every block of the forward / dgrad kernel and
# every wave of the wgrad kernel walk at least two 64-pixel units (or, on the vector-ALU path, every wgrad block two tiles)
CONV_CASES = {
    "1024_16to32": (1, 16, 0, 32, 3, 0, 1024, 1024, True),
    "1024_32to32": (1, 32, 0, 32, 3, 0, 1024, 1024, True),
    "512_up_two_source": (1, 32, 32, 32, 3, 1, 256, 256, True),
    "256_n3": (3, 32, 0, 32, 3, 0, 256, 256, True),
    "512_k1_up": (1, 64, 0, 32, 1, 1, 256, 256, True),
    # several 64-channel LDS slices, the concat boundary inside a 4-channel group of a later slice, dgrad split at 70
    "cin100_cout17": (2, 70, 30, 17, 3, 0, 32, 32, False),
    "cin130_cout3_up": (2, 70, 60, 3, 3, 1, 16, 16, False),          # last slice 2 channels: zero tail
    "cin576_cout2": (2, 70, 506, 2, 3, 0, 24, 24, False),
    "cin130_cout17_k1": (2, 70, 60, 17, 1, 0, 16, 16, False),
    # vector-ALU fallbacks
    "fallback_w102": (2, 40, 24, 96, 3, 0, 102, 102, True),          # W % 4 != 0; wgrad_kernel walks 2 tiles per block
    "fallback_hw140": (2, 32, 0, 16, 3, 0, 7, 20, False),            # W % 4 == 0 but H*W % 16 != 0
}


def _assert_persistent(n, Cin, Cout, H, W):
    if R.mfma_path(H, W):
        assert R.conv_units_per_block(n, Cout, H, W) >= 2, "forward: a block walks one unit"
        assert R.conv_units_per_block(n, Cin, H, W) >= 2, "dgrad: a block walks one unit"
        assert R.wgrad_units_per_wave(n, Cin, Cout, H, W) >= 2, "wgrad: a wave walks one unit"
    else:
        assert R.wgrad_tiles_per_block(n, Cin, Cout, H, W) >= 2, "wgrad: a block walks one tile"


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "bounded"])
@pytest.mark.parametrize("case", list(CONV_CASES))
def test_conv_dgrad_wgrad(T, case, exact):
    """Forward (+ accumulate), input gradient split over two destinations (+ accumulate), upsample2_bwd of it
    (+ accumulate), weight and bias gradient added to non-zero dw / db."""
    from gan_segmentation_amd import train_ops as ops
    n, C0, C1, Cout, K, up, Hs, Ws, persistent = CONV_CASES[case]
    H, W, Cin = Hs << up, Ws << up, C0 + C1
    assert R.mfma_path(H, W) == (not case.startswith("fallback")), "the case does not take the path it is named for"
    if persistent:
        _assert_persistent(n, Cin, Cout, H, W)
    g = T.Generator().manual_seed(sum(CONV_CASES[case][:8]) + exact)
    if exact:
        R.conv_exact_limits(Cin, Cout, K, n, H, W, bmax=8)
        mk = lambda *s: R.small_ints(s, g)
        b = R.small_ints((Cout,), g, -8, 8)
    else:
        mk = lambda *s: T.randn(*s, generator=g)
        b = T.randn(Cout, generator=g)
    x0, x1 = mk(n, C0, Hs, Ws), (mk(n, C1, Hs, Ws) if C1 else None)
    w, dy = mk(Cout, Cin, K, K), mk(n, Cout, H, W)
    w0, b0 = mk(Cout, Cin, K, K), mk(Cout)          # what dw / db hold before the wgrad call adds to them
    ref = R.conv_ref(x0, x1, w, b, up, dy)
    bnd = None if exact else R.conv_bound(x0, x1, w, b, up, dy)

    def check(what, got, want, bound, N, scale=1.0):
        if exact:
            R.assert_exact(got, want, "%s %s" % (case, what))
        else:
            _note(what.split()[0], R.assert_bounded(got, want, bound * scale, R.rho_dot(N, C_DOT), "%s %s" % (case, what)))

    b_ = lambda k: None if bnd is None else bnd[k]
    out, _ = ops.conv(_d(x0), _d(x1), _d(w), _d(b), up=up)
    check("forward", out, ref["out"], b_("out"), Cin * K * K)
    out2, _ = ops.conv(_d(x0), _d(x1), _d(w), _d(b), up=up, out0=out.clone(), accumulate=True)
    check("forward accumulate", out2, 2 * ref["out"], b_("out"), Cin * K * K, 2.0)

    dxu0, dxu1 = ops.conv(_d(dy), None, _d(w), None, transposed=True, cout0=C0)
    check("dgrad x0", dxu0, ref["dxu"][:, :C0], None if bnd is None else bnd["dxu"][:, :C0], Cout * K * K)
    if C1:
        check("dgrad x1", dxu1, ref["dxu"][:, C0:], None if bnd is None else bnd["dxu"][:, C0:], Cout * K * K)
    acc0, acc1 = ops.conv(_d(dy), None, _d(w), None, transposed=True, cout0=C0, out0=dxu0.clone(),
                          out1=dxu1.clone() if C1 else None, accumulate=True)
    check("dgrad accumulate", acc0, 2 * ref["dxu"][:, :C0], None if bnd is None else bnd["dxu"][:, :C0], Cout * K * K, 2.0)
    if C1:
        check("dgrad accumulate", acc1, 2 * ref["dxu"][:, C0:], None if bnd is None else bnd["dxu"][:, C0:], Cout * K * K, 2.0)
    if up:
        dx0 = ops.upsample2_bwd(dxu0)
        check("upsample2_bwd", dx0, ref["dx"][:, :C0], None if bnd is None else bnd["dx"][:, :C0], 4 * Cout * K * K)
        dx0 = ops.upsample2_bwd(dxu0, dx=dx0, accumulate=True)
        check("upsample2_bwd accumulate", dx0, 2 * ref["dx"][:, :C0], None if bnd is None else bnd["dx"][:, :C0],
              4 * Cout * K * K, 2.0)

    dw, db = _d(w0), _d(b0)
    ops.conv_wgrad(_d(x0), _d(x1), _d(dy), K, dw, db, up=up)
    check("wgrad", dw, w0.double() + ref["dw"], None if bnd is None else w0.double().abs() + bnd["dw"], n * H * W)
    check("bias_grad", db, b0.double() + ref["db"], None if bnd is None else b0.double().abs() + bnd["db"], n * H * W)


# ---- BatchNorm + LeakyReLU + Dropout ------------------------------------------------------------------------------
def _bn_inputs(T, n, C, H, W, seed, masked):
    """v with channel 0 at mean 100, std 1 (the float64 variance is what keeps it right) and the rest at assorted scales;
    elements whose z = gamma*xhat + beta lies within 1e-3 of 0 are moved off it, so that fp32 and float64 agree on the
    LeakyReLU branch of the backward pass."""
    g = T.Generator().manual_seed(seed)
    v = T.randn(n, C, H, W, generator=g) * (T.rand(C, generator=g) * 3 + 0.25)[None, :, None, None] \
        + (T.randn(C, generator=g) * 2)[None, :, None, None]
    v[:, 0] = T.randn(n, H, W, generator=g) + 100.0
    gamma = T.rand(C, generator=g) + 0.5
    beta = T.randn(C, generator=g) * 0.3
    rm, rv = T.randn(C, generator=g), T.rand(C, generator=g) + 0.5
    mask = (T.rand(n, C, H, W, generator=g) < 0.5).to(T.uint8) if masked else None
    dy = T.randn(n, C, H, W, generator=g)
    vd = v.double()
    mean = vd.mean(dim=(0, 2, 3), keepdim=True)
    sd = (vd.var(dim=(0, 2, 3), unbiased=False, keepdim=True) + 1e-5).sqrt()
    z = gamma.double()[None, :, None, None] * (vd - mean) / sd + beta.double()[None, :, None, None]
    near = z.abs() < 1e-3
    v = T.where(near, v + (0.01 * sd).float().expand_as(v), v)
    return v, gamma, beta, rm, rv, mask, dy


def _bn_ref(v, gamma, beta, rm, rv, mask, scale, dy):
    """float64 BatchNorm (training) + LeakyReLU(0.2) + mask, forward and backward, with the error bounds of each output:
    e = (|v| + |mean|) * inv is how far a rounding of mean / v - mean / inv can move xhat (in units of 2**-24)."""
    import torch
    v, gamma, beta, dy = v.double(), gamma.double()[None, :, None, None], beta.double()[None, :, None, None], dy.double()
    dims = (0, 2, 3)
    mean = v.mean(dim=dims, keepdim=True)
    var = ((v - mean) ** 2).mean(dim=dims, keepdim=True)
    inv = 1.0 / (var + 1e-5).sqrt()
    xh = (v - mean) * inv
    z = gamma * xh + beta
    ms = torch.ones_like(v) * scale if mask is None else mask.double() * scale
    y = torch.where(z > 0, z, 0.2 * z) * ms
    e = (v.abs() + mean.abs()) * inv
    dz = dy * torch.where(z > 0, 1.0, 0.2) * ms
    A, B = dz.mean(dim=dims, keepdim=True), (dz * xh).mean(dim=dims, keepdim=True)
    M1, Be = dz.abs().mean(dim=dims, keepdim=True), (dz.abs() * e).mean(dim=dims, keepdim=True)
    dv = gamma * inv * (dz - A - xh * B)
    flat = lambda t: t.reshape(-1)
    return {
        "y": (y, (gamma.abs() * e + beta.abs()) * ms),
        "mean": (flat(mean), flat(v.abs().mean(dim=dims))),
        "var": (flat(var), flat(var)),
        "running_mean": (0.9 * rm.double() + 0.1 * flat(mean), 0.9 * rm.double().abs() + 0.1 * flat(mean).abs()),
        "running_var": (0.9 * rv.double() + 0.1 * flat(var), 0.9 * rv.double().abs() + 0.1 * flat(var)),
        "dv": (dv, gamma.abs() * inv * (dz.abs() + A.abs() + M1 + xh.abs() * (B.abs() + Be) + e * B.abs())),
        "dgamma": (flat((dz * xh).sum(dim=dims)), flat((dz.abs() * e).sum(dim=dims))),
        "dbeta": (flat(dz.sum(dim=dims)), flat(dz.abs().sum(dim=dims))),
        "zmin": float(z.abs().min()),
    }


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("entry", ["fused", "sums"])
@pytest.mark.parametrize("shape", [(1, 32, 1024, 1024), (2, 5, 33, 33)], ids=["C32_1024sq", "oddHW"])
def test_bn_lrelu(T, shape, entry, masked):
    """Forward and backward, plain and *_sums entry points; C = 32 at 1024^2 runs bn_apply / bn_bwd_apply past their
    8192-block cap (16 passes).  Bounds, rho = C_BN * 2**-24: y <- scale*(|gamma|*e + |beta|), mean <- mean|v|,
    var <- var, running <- 0.9|running| + 0.1|batch|, dv <- |gamma|*inv*(|dz| + |A| + mean|dz| + |xhat|*(|B| + mean(|dz|*e))
    + e*|B|) with A, B the batch means of dz, dz*xhat; dgamma <- sum |dz|*e, dbeta <- sum |dz| (see _bn_ref)."""
    from gan_segmentation_amd import train_ops as ops
    n, C, H, W = shape
    v, gamma, beta, rm, rv, mask, dy = _bn_inputs(T, n, C, H, W, seed=C + H, masked=masked)
    scale = 2.0 if masked else 1.0
    ref = _bn_ref(v, gamma, beta, rm, rv, mask, scale, dy)
    assert ref["zmin"] >= 1e-4, "an element sits on the LeakyReLU kink"
    rm_d, rv_d = _d(rm), _d(rv)
    if entry == "fused":
        y, mean, var = ops.bn_lrelu_fwd(_d(v), _d(gamma), _d(beta), rm_d, rv_d, mask=_d(mask), drop_scale=scale)
    else:
        y, mean, var, count = ops.sync_bn_lrelu_fwd(_d(v), _d(gamma), _d(beta), rm_d, rv_d, lambda t: None, mask=_d(mask),
                                                    drop_scale=scale)
        assert count == n * H * W
    rho = C_BN * R.U
    got = {"y": y, "mean": mean, "var": var, "running_mean": rm_d, "running_var": rv_d}
    for k, t in got.items():
        _note("bn", R.assert_bounded(t, ref[k][0], ref[k][1], rho, "bn %s %s" % (shape, k)))
    gd = _d(dy)
    dgam, dbet = T.zeros(C, device="cuda"), T.zeros(C, device="cuda")
    if entry == "fused":
        ops.bn_lrelu_bwd(_d(v), _d(gamma), _d(beta), mean, var, gd, dgam, dbet, mask=_d(mask), drop_scale=scale)
    else:
        ops.sync_bn_lrelu_bwd(_d(v), _d(gamma), _d(beta), mean, var, count, gd, dgam, dbet, lambda t: None, mask=_d(mask),
                              drop_scale=scale)
    for k, t in (("dv", gd), ("dgamma", dgam), ("dbeta", dbet)):
        _note("bn", R.assert_bounded(t, ref[k][0], ref[k][1], rho, "bn %s %s" % (shape, k)))


# ---- softmax cross-entropy ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("HW", [1024, 512 * 512, 1024 * 1024])
@pytest.mark.parametrize("classes", [2, 3, 5, 8])
def test_softmax_ce(T, classes, HW):
    """Logits uniform in [-60, 60]; sample 0 with a quarter of its labels -1, sample 1 with all of them -1 (loss and
    gradient exactly 0).  Bounds, rho = C_CE * 2**-24, with m = max logit, E = sum_o sm_o*|l_o - m|, K = classes:
    dlogits <- (sm*(|l - m| + E + K + 5) + |sm - onehot|) * grad_scale/HW + 2**-126/rho (exp underflow),
    loss <- mean over pixels of w*(|m| + |lse| + |l_label| + E + K + 4) + sqrt(HW) * mean |term| (the fp32 sum)."""
    import torch
    from gan_segmentation_amd import train_ops as ops
    g = T.Generator().manual_seed(classes * 7 + HW)
    n, gs = 2, 0.5
    logits = (T.rand(n, classes, HW, generator=g) * 2 - 1) * 60
    labels = T.randint(0, classes, (n, HW), generator=g)
    labels[0][T.rand(HW, generator=g) < 0.25] = -1
    labels[1] = -1
    loss, dl = ops.softmax_ce(_d(logits.reshape(n, classes, HW, 1)), _d(labels.to(T.int8).reshape(n, HW, 1)), grad_scale=gs)
    loss, dl = loss.cpu(), dl.cpu().reshape(n, classes, HW)
    assert float(loss[1]) == 0.0 and bool((dl[1] == 0).all()), "an all-ignored sample must give loss and gradient 0"
    l = logits.double()
    wgt = (labels > -1).double()
    lc = labels.clamp(min=0)
    m = l.max(dim=1, keepdim=True).values
    lse = torch.logsumexp(l, dim=1, keepdim=True)
    sm = (l - lse).exp()
    onehot = torch.nn.functional.one_hot(lc, classes).permute(0, 2, 1).double()
    E = (sm * (l - m).abs()).sum(dim=1, keepdim=True)
    dref = (sm - onehot) * wgt[:, None] * gs / HW
    dbnd = (sm * ((l - m).abs() + E + classes + 5) + (sm - onehot).abs()) * gs / HW
    rho = C_CE * R.U
    _note("softmax_ce", R.assert_bounded(dl, dref, dbnd, rho, "dlogits", atol=2.0 ** -126))
    ll = l.gather(1, lc[:, None])[:, 0]
    term = wgt * (lse[:, 0] - ll)
    lref = term.mean(dim=1)
    lbnd = (wgt * (m[:, 0].abs() + lse[:, 0].abs() + ll.abs() + E[:, 0] + classes + 4)).mean(dim=1) \
        + HW ** 0.5 * term.abs().mean(dim=1)
    _note("softmax_ce", R.assert_bounded(loss, lref, lbnd, rho, "loss"))


# ---- element-wise kernels past the 8192-block cap of grid_for -----------------------------------------------------
BIG = 3000001    # > 8192 blocks * 256 threads, odd; = 853 * 3517


def test_adam_add_upsample_past_grid_cap(T):
    """Adam with weight decay, add (also in place) and upsample2_bwd (+ accumulate) over 3 000 001 elements.  add is one
    correctly rounded fp32 addition: bit-equal to the float64 sum rounded to fp32.  upsample2_bwd runs in exact mode.
    Adam bounds, rho = C_ADAM * 2**-24, with g' = g*rescale + wd*w: m <- b1|m| + (1-b1)G, v <- b2 v + (1-b2)G^2 with
    G = |g*rescale| + |wd*w|, w <- |w| + lr_t*(m_bound + |m'|*(1 + v_bound/v'))/(sqrt(v') + eps)."""
    from gan_segmentation_amd import train_ops as ops
    g = T.Generator().manual_seed(17)
    w, gr, m = (T.randn(BIG, generator=g) for _ in range(3))
    v = T.randn(BIG, generator=g).abs() + 0.1
    f = lambda x: float(np.float32(x))              # the kernel takes fp32 scalars
    t, b1, b2, eps, rescale, wd = 3, f(0.9), f(0.999), f(1e-8), f(0.5), f(0.01)
    lr_t = f(1e-3 * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t))
    wd_, md, vd = _d(w), _d(m), _d(v)
    ops.adam(wd_, _d(gr), md, vd, lr_t, b1, b2, eps, rescale=rescale, wd=wd)
    W_, G_, M_, V_ = w.double(), gr.double(), m.double(), v.double()
    gg = G_ * rescale + wd * W_
    mm = b1 * M_ + (1 - b1) * gg
    vv = b2 * V_ + (1 - b2) * gg * gg
    wn = W_ - lr_t * mm / (vv.sqrt() + eps)
    Gb = (G_ * rescale).abs() + (wd * W_).abs()
    mb = b1 * M_.abs() + (1 - b1) * Gb
    vb = b2 * V_ + (1 - b2) * Gb * Gb
    wb = W_.abs() + lr_t * (mb + mm.abs() * (1 + vb / vv)) / (vv.sqrt() + eps)
    rho = C_ADAM * R.U
    for what, got, want, bnd in (("adam m", md, mm, mb), ("adam v", vd, vv, vb), ("adam w", wd_, wn, wb)):
        _note("adam", R.assert_bounded(got, want, bnd, rho, what))

    a, b = T.randn(BIG, generator=g), T.randn(BIG, generator=g)
    want = (a.double() + b.double()).float()
    assert T.equal(ops.add(_d(a), _d(b)).cpu(), want)
    ad = _d(a)
    ops.add(ad, _d(b), out=ad)
    assert T.equal(ad.cpu(), want)

    dy_up = R.small_ints((1, 1, 2 * 853, 2 * 3517), g)
    dx0 = R.small_ints((1, 1, 853, 3517), g)
    dx = ops.upsample2_bwd(_d(dy_up), dx=_d(dx0), accumulate=True)
    want = dx0.double() + dy_up.double().reshape(1, 1, 853, 2, 3517, 2).sum(dim=(3, 5))
    R.assert_exact(dx, want, "upsample2_bwd accumulate")


# ---- dropout mask -------------------------------------------------------------------------------------------------
def _dropout_ref(count, seed, stream_id, keep):
    """CPU restatement of dropout_mask_kernel: Philox4x32-10, counter (q, q >> 32, stream_id, 0x44524F50) for the quad q
    of elements 4q..4q+3, key (seed, seed >> 32); keep iff ((word >> 8) + 0.5) * 2**-24 < keep, evaluated exactly.
    -> (mask, the 24-bit words)."""
    from oracle.ref_philox import philox4x32_10
    quads = (count + 3) // 4
    q = np.arange(quads, dtype=np.uint64)
    ctr = np.stack([(q & np.uint64(0xFFFFFFFF)).astype(np.uint32), (q >> np.uint64(32)).astype(np.uint32),
                    np.full(quads, stream_id, np.uint32), np.full(quads, 0x44524F50, np.uint32)], axis=-1)
    x = philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32)).reshape(-1)[:count] >> np.uint32(8)
    u = (x.astype(np.float64) + 0.5) * 2.0 ** -24
    return (u < float(np.float32(keep))).astype(np.uint8), x


@pytest.mark.parametrize("keep", [0.5, 1.0])
def test_dropout_mask_bit_exact(T, keep):
    """9 000 003 elements (past the 8192-block cap, count % 4 == 3).  Seed 12, stream 7 draws the largest 24-bit word
    0xFFFFFF at element 264008: in fp32 its uniform (2**24 - 0.5) * 2**-24 rounds to 1.0, which used to drop that element
    even at keep 1."""
    from gan_segmentation_amd import train_ops as ops
    count, seed, sid = 9000003, 12, 7
    want, words = _dropout_ref(count, seed, sid, keep)
    assert words[264008] == 0xFFFFFF
    got = ops.dropout_mask((count,), seed, sid, keep, "cuda").cpu().numpy()
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, "%d elements differ, first at %d (word %#x)" % (bad.size, bad[0], words[bad[0]])
