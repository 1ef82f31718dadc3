"""The region term's kernels (csrc/gsa_region.h) against the float64 autograd restatement of tests/region_ref.py, with the method of
tests/test_gpu_loss.py: element by element |got - ref| <= rho * bound, the bound written out in tests/region_ref.py,
rho = C_REGION * 2**-24; and the exact properties the two-pass reduction gives.

Inputs: n = 3; sample 0 with a quarter of its labels -1 and a few equal to K, -2 and 127 (ignored, not clamped), sample 1 all -1,
sample 2 a copy of sample 0; class weights in [0.25, 4].  Two draws of the logits a shape: uniform in [-60, 60] (saturated) and in
[-3, 3] (soft probabilities, where P_k and I_k really differ).  Shapes: HW in {1, 255, 257, 1000} with K in {2, 3, 8}, K = 16 at
HW = 257, and HW = 2 * 256 * GSA_REGION_MAX_BLOCKS + 3 at K = 2, where the block cap is reached and every workgroup walks at least two
strides.  Every shape runs (alpha, beta) in {(0.5, 0.5), (0.3, 0.7), (1, 1)} x smooth in {0, 1} x both class modes x with and
without class weights; the largest shape runs six of those 24 that hold every value of every option (its float64 reference takes a
third of a second a case), the others all of them.  HW = 1000 is a multiple of four (16-byte loads), the other sizes are not (the
same pixels by scalar loads).

C_REGION: measured on an MI355X with C_REGION = 1, the worst |got - ref| / (rho * bound) over the module was
    dlogits 0.77, loss 0.68, index 0.58, sums 0.32
(loss and index are one rounding to fp32 of a double result, half an ulp against a bound of one, plus the sums' share).  Twice the
worst, rounded up to an integer, is 2: C_REGION = 2, the constant of tests/test_gpu_loss.py's C_LOSS and C_CE, and below the 8 at
which the bound expression would have to be called incomplete.  The worst ratio seen is printed at the end of the module
(pytest -s)."""
import functools
import itertools

import pytest

from tests import f64_ref as R
from tests import region_ref

pytestmark = pytest.mark.gpu

C_REGION = 2.0      # rho = C_REGION * 2**-24 against tests/region_ref.bounds
GS = 0.5            # grad_scale
AB = ((0.5, 0.5), (0.3, 0.7), (1.0, 1.0))
SMOOTH = (0.0, 1.0)
MODES = ("present", "all")
OPTIONS = list(itertools.product(AB, SMOOTH, MODES, (False, True)))
# the largest shape: every (alpha, beta) with each smooth once, the modes and the weights alternating
OPTIONS_CAP = [(AB[0], 0.0, "present", False), (AB[0], 1.0, "all", True), (AB[1], 0.0, "all", True), (AB[1], 1.0, "present", False),
               (AB[2], 0.0, "present", True), (AB[2], 1.0, "all", False)]
DRAWS = {"saturated": 60.0, "soft": 3.0}

WORST = {}


def _note(what, ratio):
    WORST[what] = max(WORST.get(what, 0.0), ratio)


def _bounded(got, ref, bound, rho, what, key):
    """tests/f64_ref.assert_bounded, the worst ratio noted before the assertion speaks."""
    import torch
    g, r = got.detach().to("cpu", torch.float64), ref.detach().to("cpu", torch.float64)
    allow = rho * torch.as_tensor(bound, dtype=torch.float64).expand_as(r)
    pos = allow > 0
    if bool(pos.any()):
        _note(key, float(((g - r).abs()[pos] / allow[pos]).max()))
    R.assert_bounded(got, ref, bound, rho, what)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nworst |got - ref| / (rho * bound), C_REGION = %g:" % C_REGION)
    for k in sorted(WORST):
        print("  %-16s %.4f" % (k, WORST[k]))


def _cap():
    from gan_segmentation_amd import loss_ops
    return loss_ops.REGION_MAX_BLOCKS


def _shapes():
    return [(HW, K) for HW in (1, 255, 257, 1000) for K in (2, 3, 8)] + [(257, 16), ("cap", 2)]


def _hw(HW):
    return 2 * 256 * _cap() + 3 if HW == "cap" else HW


@functools.lru_cache(maxsize=None)
def _inputs(HW, K, draw):
    """(logits (3, K, HW) fp32, labels (3, HW) int8, cw (K,) fp32) on the host: drawn once a shape and draw, shared by its cases and
    never written."""
    import torch
    g = torch.Generator().manual_seed(1000 * K + HW + (7 if draw == "soft" else 0))
    logits = (torch.rand(3, K, HW, generator=g) * 2 - 1) * DRAWS[draw]
    labels = torch.randint(0, K, (3, HW), generator=g)
    labels[0][torch.rand(HW, generator=g) < 0.25] = -1
    if HW >= 255:
        odd = torch.randperm(HW, generator=g)[:12]
        labels[0][odd[:4]], labels[0][odd[4:8]], labels[0][odd[8:]] = K, -2, 127
    labels[1] = -1
    labels[2] = labels[0]
    logits[2] = logits[0]
    cw = torch.rand(K, generator=g) * 3.75 + 0.25
    return logits, labels.to(torch.int8), cw


@functools.lru_cache(maxsize=None)
def _on_device(HW, K, draw):
    return tuple(t.cuda().contiguous() for t in _inputs(HW, K, draw))


def _run(logits, labels, ab, smooth, mode, cw=None, **kw):
    from gan_segmentation_amd import loss_ops
    return loss_ops.region_loss(logits, labels, ab[0], ab[1], smooth, mode, class_weights=cw, grad_scale=GS, **kw)


def _same_bits(a, b):
    import torch
    a, b = a.cpu().contiguous().reshape(-1), b.cpu().contiguous().reshape(-1)
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


@pytest.mark.parametrize("draw", sorted(DRAWS))
@pytest.mark.parametrize("HW,K", _shapes())
def test_against_float64_autograd(torch_cuda, HW, K, draw):
    """loss, sums, index and dlogits within rho * bound of the float64 reference for every option; the exact properties with them:
    G is the reference's count, the all-ignored sample is 0 everywhere, ignored pixels have gradient 0, the copy of sample 0 has its
    bits, a second call and the sample alone give the same bits, without dlogits loss, sums and index are the same bits, and
    ``into=base`` is base + dlogits in fp32 on the valid pixels and base's own bits, a planted -0.0 included, on the others."""
    torch = torch_cuda
    options = OPTIONS_CAP if HW == "cap" else OPTIONS
    HW = _hw(HW)
    logits, labels, cw = _inputs(HW, K, draw)
    zl, zy, zc = _on_device(HW, K, draw)
    rho = C_REGION * R.U
    ignored = (labels[0] < 0) | (labels[0] >= K)
    valid = ((labels >= 0) & (labels < K))[:, None].expand(3, K, HW)
    base = torch.randn(3, K, HW, generator=torch.Generator().manual_seed(HW + K))
    base[1, :, ::2] = -0.0
    base[0][:, ignored] = torch.where(torch.arange(int(ignored.sum())) % 2 == 0, -0.0, 1.5).expand(K, -1)
    for ab, smooth, mode, weighted in options:
        what = "HW %d K %d %s alpha %g beta %g smooth %g %s %s" % (HW, K, draw, ab[0], ab[1], smooth, mode, "weighted" if weighted else "plain")
        dcw = zc if weighted else None
        out = _run(zl, zy, ab, smooth, mode, dcw)
        loss, sums, index, dl = (t.cpu() for t in out)
        kw = dict(alpha=ab[0], beta=ab[1], smooth=smooth, mode=MODES.index(mode), cw=cw if weighted else None, grad_scale=GS)
        lref, sref, iref, dref = region_ref.region_f64(logits, labels, **kw)
        bnd = region_ref.bounds(logits, labels, rho=rho, **kw)
        assert all(bool(torch.isfinite(t).all()) for t in (loss, sums, index, dl)), what
        _bounded(sums, sref, bnd["sums"], rho, what + ": sums", "sums")
        _bounded(index, iref, bnd["index"], rho, what + ": index", "index")
        _bounded(loss, lref, bnd["loss"], rho, what + ": loss", "loss")
        _bounded(dl, dref, bnd["dlogits"], rho, what + ": dlogits", "dlogits")
        assert bool((sums[:, 2] == sref[:, 2]).all()), what + ": G is a count"
        # ---- exact: ignored pixels and the all-ignored sample
        assert float(loss[1]) == 0.0 and bool((sums[1] == 0).all()) and bool((index[1] == 0).all()) and bool((dl[1] == 0).all()), what
        assert bool((dl[0][:, ignored] == 0).all()), what + ": an ignored pixel has gradient 0"
        # ---- exact: position in the batch, repetition, batch size, forward only, accumulation
        assert all(_same_bits(t[2], t[0]) for t in (loss, sums, index, dl)), what + ": sample 2 is sample 0"
        again = _run(zl, zy, ab, smooth, mode, dcw)
        assert all(_same_bits(a, b) for a, b in zip(again, (loss, sums, index, dl))), what + ": a second call"
        alone = _run(zl[:1], zy[:1], ab, smooth, mode, dcw)
        assert all(_same_bits(a, b[:1]) for a, b in zip(alone, (loss, sums, index, dl))), what + ": the sample alone"
        fwd = _run(zl, zy, ab, smooth, mode, dcw, grad=False)
        assert fwd[3] is None and all(_same_bits(a, b) for a, b in zip(fwd[:3], (loss, sums, index))), what + ": forward only"
        target = base.cuda()
        acc = _run(zl, zy, ab, smooth, mode, dcw, into=target)
        assert acc[3] is target and all(_same_bits(a, b) for a, b in zip(acc[:3], (loss, sums, index))), what + ": into"
        assert _same_bits(target, torch.where(valid, base + dl, base)), what + ": into is one fp32 add, and none on an ignored pixel"


def test_half_and_half_closed_form(torch_cuda):
    """All-zero logits, K = 2, every pixel valid, G_0 = G_1 = 128 at HW = 256: p = 0.5 exactly, I_k = 64, P_k = 128, and TI_k is
    the rational number the rule gives."""
    torch = torch_cuda
    HW = 256
    logits = torch.zeros(1, 2, HW, device="cuda")
    labels = (torch.arange(HW) % 2).to(torch.int8).reshape(1, HW).cuda()
    for ab, smooth, mode in itertools.product(AB, SMOOTH, MODES):
        loss, sums, index, dl = _run(logits, labels, ab, smooth, mode)
        assert sums.cpu().tolist() == [[[64.0, 64.0], [128.0, 128.0], [128.0, 128.0]]]
        ti = (64.0 + smooth) / ((1.0 - ab[0] - ab[1]) * 64.0 + ab[0] * 128.0 + ab[1] * 128.0 + smooth)
        assert index.shape == (1, 2) and index.cpu().reshape(-1).tolist() == pytest.approx([ti, ti], rel=1e-6)
        assert float(loss) == pytest.approx(1.0 - ti, rel=1e-6)
        assert bool(torch.isfinite(dl).all()) and float(dl.abs().max()) > 0


def test_a_class_that_no_pixel_has(torch_cuda):
    """smooth = 0, K = 3, labels in {0, 1}: in "all" mode class 2 scores TI = 0 and counts in A; in "present" mode it does not count."""
    torch = torch_cuda
    g = torch.Generator().manual_seed(11)
    HW = 300
    logits = (torch.rand(1, 3, HW, generator=g) * 6 - 3).cuda()
    labels = torch.randint(0, 2, (1, HW), generator=g).to(torch.int8).cuda()
    present = _run(logits, labels, (0.5, 0.5), 0.0, "present")
    everything = _run(logits, labels, (0.5, 0.5), 0.0, "all")
    assert _same_bits(present[1], everything[1]) and _same_bits(present[2], everything[2])
    ti = present[2][0].cpu().double()
    assert float(ti[2]) == 0.0 and float(present[1][0, 2, 2]) == 0.0 and float(present[1][0, 1, 2]) > 0
    assert float(present[0]) == pytest.approx(float(((1 - ti[0]) + (1 - ti[1])) / 2), rel=1e-6)
    assert float(everything[0]) == pytest.approx(float(((1 - ti[0]) + (1 - ti[1]) + 1.0) / 3), rel=1e-6)
    assert bool(torch.isfinite(present[3]).all()) and bool(torch.isfinite(everything[3]).all())


def test_a_sample_without_a_valid_pixel_has_no_class(torch_cuda):
    """A == 0 whatever the mode and smooth: loss, index and gradient are 0, and ``into`` keeps every bit."""
    torch = torch_cuda
    logits = torch.randn(2, 3, 40, generator=torch.Generator().manual_seed(3)).cuda()
    labels = torch.tensor([-1, 3, -128, 127] * 10, dtype=torch.int8).repeat(2, 1).cuda()
    for smooth, mode in itertools.product(SMOOTH, MODES):
        loss, sums, index, dl = _run(logits, labels, (0.3, 0.7), smooth, mode)
        assert not bool(loss.any()) and not bool(sums.any()) and not bool(index.any()) and not bool(dl.any())
        base = torch.full_like(logits, -0.0)
        assert _same_bits(_run(logits, labels, (0.3, 0.7), smooth, mode, into=base)[3], torch.full_like(logits, -0.0))


def test_value_errors(torch_cuda):
    torch = torch_cuda
    from gan_segmentation_amd import loss_ops
    logits, labels, cw = _on_device(255, 3, "soft")
    ok = loss_ops.region_loss(logits, labels, class_weights=cw.tolist())
    assert _same_bits(ok[0], loss_ops.region_loss(logits.reshape(3, 3, 51, 5), labels.reshape(3, 51, 5), class_weights=cw)[0])
    wide = torch.zeros(1, 17, 8, device="cuda")
    for bad in (dict(logits=logits.cpu()), dict(logits=logits.double()), dict(logits=logits[:, :1]), dict(logits=logits[:, :, ::2]),
                dict(logits=wide, labels=torch.zeros(1, 8, dtype=torch.int8, device="cuda")),
                dict(labels=labels.long()), dict(labels=labels[:, :-1]), dict(labels=labels.cpu()),
                dict(alpha=-0.1), dict(alpha=float("nan")), dict(alpha="0.5"), dict(beta=-1), dict(beta=float("inf")),
                dict(alpha=0, beta=0), dict(smooth=-1.0), dict(smooth=None), dict(classes="some"), dict(classes=0),
                dict(class_weights=[1.0, 2.0]), dict(class_weights=cw[:2]), dict(class_weights=cw.double()), dict(class_weights="median"),
                dict(class_weights=[1.0, -1.0, 1.0]), dict(grad_scale=float("nan")), dict(grad_scale="1"),
                dict(into=torch.zeros_like(logits), grad=False), dict(into=torch.zeros_like(logits).double()),
                dict(into=torch.zeros_like(logits)[:2]), dict(into=torch.zeros_like(logits).cpu()),
                dict(workspace=torch.empty(8, device="cuda", dtype=torch.uint8)),
                dict(workspace=torch.empty(4096, device="cuda", dtype=torch.float32))):
        args = dict(dict(logits=logits, labels=labels), **bad)
        with pytest.raises(ValueError):
            loss_ops.region_loss(**args)
    empty = loss_ops.region_loss(logits[:0], labels[:0])
    assert empty[0].shape == (0,) and empty[1].shape == (0, 3, 3) and empty[2].shape == (0, 3) and empty[3].shape == (0, 3, 255)
