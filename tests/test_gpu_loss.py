"""The decoder losses' kernels (csrc/gsa_loss.h) against the float64 autograd restatement of tests/loss_ref.py, with the method of
tests/test_train_kernels.py: element by element |got - ref| <= rho * bound, bound = the same expression on the magnitudes of the
operands (written out in tests/loss_ref.py), rho = C_LOSS * 2**-24; and the exact properties the two-pass reduction gives.

Inputs as test_softmax_ce: logits uniform in [-60, 60], n = 3; sample 0 with a quarter of its labels -1 and a few equal to K and
to -2 (ignored, not clamped), sample 1 all -1, sample 2 a copy of sample 0; dist2 drawn from {1..1024, 32767}, class weights in
[0.25, 4].  Shapes: HW in {1, 255, 257, 1000} with K in {2, 3, 8}, K = 64 at HW = 257, and HW = 2 * 256 * GSA_LOSS_MAX_BLOCKS + 3 at
K = 2, where the block cap is reached and every workgroup walks at least two strides.  Every shape runs the three normalisers with
gamma in {0, 1, 2, 3.5}, without weights and with both; the largest shape runs gamma in {0, 2} only.

The plain mode (gamma 0, no weights, "mean", labels in {-1, 0..K-1}) is held to the bounds of test_softmax_ce at its C_CE = 2.

Measured on an MI355X, worst |got - ref| / (rho * bound) over the module at C_LOSS = 2: dlogits 0.42, sums 0.28, loss 0.09, so
C_LOSS is about twice the worst at 1 (that module's convention); the plain mode at C_CE = 2: dlogits 0.71, loss 0.03.  The worst
ratio seen is printed at the end of the module (pytest -s)."""
import functools

import numpy as np
import pytest

from tests import f64_ref as R
from tests import loss_ref

pytestmark = pytest.mark.gpu

C_CE = 2.0          # tests/test_train_kernels.py's constant for softmax-CE: the plain mode may be no less accurate
C_LOSS = 2.0        # every other mode: rho = C_LOSS * 2**-24 against tests/loss_ref.bounds
GS = 0.5            # grad_scale
NORMS = ("mean", "valid", "focal")
GAMMAS = (0.0, 1.0, 2.0, 3.5)

WORST = {}


def _note(what, ratio):
    WORST[what] = max(WORST.get(what, 0.0), ratio)


def _bounded(got, ref, bound, rho, what, key, atol=0.0):
    """tests/f64_ref.assert_bounded, the worst ratio noted before the assertion speaks."""
    import torch
    g, r = got.detach().to("cpu", torch.float64), ref.detach().to("cpu", torch.float64)
    allow = rho * torch.as_tensor(bound, dtype=torch.float64).expand_as(r) + atol
    pos = allow > 0
    if bool(pos.any()):
        _note(key, float(((g - r).abs()[pos] / allow[pos]).max()))
    R.assert_bounded(got, ref, bound, rho, what, atol=atol)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nworst |got - ref| / (rho * bound), C_LOSS = %g, C_CE = %g:" % (C_LOSS, C_CE))
    for k in sorted(WORST):
        print("  %-16s %.4f" % (k, WORST[k]))


def _cap():
    from gan_segmentation_amd import loss_ops
    return loss_ops.LOSS_MAX_BLOCKS


def _shapes():
    out = [(HW, K) for HW in (1, 255, 257, 1000) for K in (2, 3, 8)] + [(257, 64)]
    return out + [("cap", 2)]


def _hw(HW):
    return 2 * 256 * _cap() + 3 if HW == "cap" else HW


@functools.lru_cache(maxsize=None)
def _inputs(HW, K):
    """(logits (3, K, HW) fp32, labels (3, HW) int8, dist2 (3, HW) int16, cw (K,) fp32, table (1026,) fp32) on the host: drawn once a
    shape, shared by its cases and never written."""
    import torch
    from gan_segmentation_amd import loss_ops
    g = torch.Generator().manual_seed(1000 * K + HW)
    logits = (torch.rand(3, K, HW, generator=g) * 2 - 1) * 60
    labels = torch.randint(0, K, (3, HW), generator=g)
    labels[0][torch.rand(HW, generator=g) < 0.25] = -1
    if HW >= 255:
        odd = torch.randperm(HW, generator=g)[:12]
        labels[0][odd[:4]], labels[0][odd[4:8]], labels[0][odd[8:]] = K, -2, 127
    labels[1] = -1
    labels[2] = labels[0]
    logits[2] = logits[0]
    d2 = torch.randint(1, 1026, (3, HW), generator=g)
    d2[d2 == 1025] = 32767
    d2[2] = d2[0]
    cw = torch.rand(K, generator=g) * 3.75 + 0.25
    table = torch.from_numpy(loss_ops.boundary_weight_table(32, 4.0, 12.0))
    return logits, labels.to(torch.int8), d2.to(torch.int16), cw, table


def _run(logits, labels, norm, gamma, cw=None, d2=None, table=None, grad=True):
    from gan_segmentation_amd import loss_ops
    d = lambda t: None if t is None else t.to("cuda").contiguous()
    return loss_ops.softmax_loss(d(logits), d(labels), gamma=gamma, normalise=norm, class_weights=d(cw), dist2=d(d2), table=d(table),
                                 grad=grad, grad_scale=GS)


def _same_bits(a, b):
    import torch
    a, b = a.cpu().reshape(-1), b.cpu().reshape(-1)
    return a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


@pytest.mark.parametrize("weights", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("HW,K", _shapes())
def test_against_float64_autograd(torch_cuda, HW, K, norm, weights):
    """loss, sums and dlogits within rho * bound of the float64 reference for every gamma; the exact properties with them: the
    all-ignored sample is 0 everywhere, the copy of sample 0 has its bits, a second call and the sample alone give the same bits, and
    without dlogits loss and sums are the same bits."""
    torch = torch_cuda
    big = HW == "cap"
    HW = _hw(HW)
    logits, labels, d2, cw, table = _inputs(HW, K)
    extra = dict(cw=cw, d2=d2, table=table) if weights else {}
    rho = C_LOSS * R.U
    for gamma in ((0.0, 2.0) if big else GAMMAS):
        what = "HW %d K %d %s gamma %g %s" % (HW, K, norm, gamma, "weighted" if weights else "plain")
        loss, sums, dl = _run(logits, labels, norm, gamma, **extra)
        loss, sums, dl = loss.cpu(), sums.cpu(), dl.cpu()
        kw = dict(cw=extra.get("cw"), d2=extra.get("d2"), tab=extra.get("table"), gamma=gamma, normalise=NORMS.index(norm), grad_scale=GS)
        lref, sref, dref = loss_ref.loss_f64(logits, labels, **kw)
        bnd = loss_ref.bounds(logits, labels, rho=rho, **kw)
        assert bool(torch.isfinite(loss).all() and torch.isfinite(sums).all() and torch.isfinite(dl).all()), what
        _bounded(sums, sref, bnd["sums"], rho, what + ": sums", "sums")
        _bounded(loss, lref, bnd["loss"], rho, what + ": loss", "loss")
        _bounded(dl, dref, bnd["dlogits"], rho, what + ": dlogits", "dlogits")
        assert bool((sums[:, 3] == sref[:, 3]).all()), what + ": T is a count"
        # ---- exact: ignored pixels and the all-ignored sample
        assert float(loss[1]) == 0.0 and bool((sums[1] == 0).all()) and bool((dl[1] == 0).all()), what
        ignored = (labels[0] < 0) | (labels[0] >= K)
        assert bool((dl[0][:, ignored] == 0).all()), what + ": an ignored pixel has gradient 0"
        # ---- exact: position in the batch, repetition, batch size, forward only
        assert _same_bits(loss[2], loss[0]) and _same_bits(sums[2], sums[0]) and _same_bits(dl[2], dl[0]), what + ": sample 2 is sample 0"
        again = _run(logits, labels, norm, gamma, **extra)
        assert all(_same_bits(a, b) for a, b in zip(again, (loss, sums, dl))), what + ": a second call"
        alone = _run(logits[:1], labels[:1], norm, gamma, **{k: (v[:1] if k == "d2" else v) for k, v in extra.items()})
        assert all(_same_bits(a, b[:1]) for a, b in zip(alone, (loss, sums, dl))), what + ": the sample alone"
        fwd = _run(logits, labels, norm, gamma, grad=False, **extra)
        assert fwd[2] is None and _same_bits(fwd[0], loss) and _same_bits(fwd[1], sums), what + ": forward only"


@pytest.mark.parametrize("HW,K", _shapes())
def test_plain_mode_meets_the_bounds_of_softmax_ce(torch_cuda, HW, K):
    """gamma 0, no weights, "mean", labels in {-1, 0..K-1}: the bounds of tests/test_train_kernels.py::test_softmax_ce, word for
    word, at its C_CE."""
    torch = torch_cuda
    HW = _hw(HW)
    logits, labels, _d2, _cw, _table = _inputs(HW, K)
    labels = torch.where((labels < -1) | (labels >= K), torch.full_like(labels, -1), labels)        # in range: -1 or a class
    loss, _sums, dl = _run(logits, labels, "mean", 0.0)
    l = logits.double()
    lab = labels.long()
    wgt = (lab > -1).double()
    lc = lab.clamp(min=0)
    m = l.max(dim=1, keepdim=True).values
    lse = torch.logsumexp(l, dim=1, keepdim=True)
    sm = (l - lse).exp()
    onehot = torch.nn.functional.one_hot(lc, K).permute(0, 2, 1).double()
    E = (sm * (l - m).abs()).sum(dim=1, keepdim=True)
    dref = (sm - onehot) * wgt[:, None] * GS / HW
    dbnd = (sm * ((l - m).abs() + E + K + 5) + (sm - onehot).abs()) * GS / HW
    rho = C_CE * R.U
    _bounded(dl, dref, dbnd, rho, "dlogits", "plain dlogits", atol=2.0 ** -126)
    ll = l.gather(1, lc[:, None])[:, 0]
    term = wgt * (lse[:, 0] - ll)
    lref = term.mean(dim=1)
    lbnd = (wgt * (m[:, 0].abs() + lse[:, 0].abs() + ll.abs() + E[:, 0] + K + 4)).mean(dim=1) + HW ** 0.5 * term.abs().mean(dim=1)
    _bounded(loss, lref, lbnd, rho, "loss", "plain loss")


def test_plain_mode_is_the_loss_of_softmax_ce(torch_cuda):
    """On labels in {-1, 0..K-1} the new entry and gsa_train_softmax_ce compute one loss: they agree to fp32 rounding."""
    torch = torch_cuda
    from gan_segmentation_amd import train_ops
    logits, labels, _d2, _cw, _table = _inputs(1000, 3)
    labels = torch.where((labels < -1) | (labels >= 3), torch.full_like(labels, -1), labels)
    loss, sums, dl = _run(logits, labels, "mean", 0.0)
    old_loss, old_dl = train_ops.softmax_ce(logits.cuda().reshape(3, 3, 1000, 1), labels.cuda().reshape(3, 1000, 1), grad_scale=GS)
    assert torch.allclose(loss, old_loss, rtol=1e-5, atol=0) and torch.allclose(dl, old_dl.reshape(dl.shape), rtol=1e-4, atol=1e-9)
    assert bool((sums[:, 0] == sums[:, 1]).all() and (sums[:, 0] == sums[:, 3]).all()), "without weights W = B = T"


def test_out_of_range_labels_are_ignored_not_clamped(torch_cuda):
    """A label K, -2 or 127 changes nothing against the same pixel labelled -1."""
    torch = torch_cuda
    logits, labels, d2, cw, table = _inputs(1000, 3)
    assert int(((labels[0] >= 3) | (labels[0] < -1)).sum()) == 12
    masked = torch.where((labels < -1) | (labels >= 3), torch.full_like(labels, -1), labels)
    for norm in NORMS:
        a = _run(logits, labels, norm, 2.0, cw=cw, d2=d2, table=table)
        b = _run(logits, masked, norm, 2.0, cw=cw, d2=d2, table=table)
        assert all(_same_bits(x, y) for x, y in zip(a, b)), norm


def test_table_index(torch_cuda):
    """dist2 0..1024 reads its own entry, everything else -- negative, 1025 .. 32766, BOUNDARY_FAR -- the last one: with a table of
    small integers W is an exact sum."""
    torch = torch_cuda
    d = torch.tensor([0, 1, 2, 1023, 1024, 1025, 1026, 5000, 32766, 32767, -1, -7, -32768], dtype=torch.int16)
    HW = d.numel()
    table = (torch.arange(1026) % 7 + 1).float()
    table[1025] = 100.0
    logits = torch.zeros(1, 2, HW)
    labels = torch.zeros(1, HW, dtype=torch.int8)
    _loss, sums, _dl = _run(logits, labels, "valid", 0.0, d2=d.reshape(1, HW), table=table, grad=False)
    want = sum(float(table[int(v)]) if 0 <= int(v) <= 1024 else 100.0 for v in d)
    assert float(sums[0, 0]) == want and float(sums[0, 3]) == HW
    assert float(sums[0, 2]) == pytest.approx(want * np.log(2.0), rel=1e-6)


def test_no_focal_mass(torch_cuda):
    """normalise "focal", gamma 2, every valid pixel with a label margin of 200: the other classes' exponentials underflow, q = 0
    and B = 0.  The loss is 0, the gradient exactly 0, nothing is non-finite -- where the reference's eps terms would divide."""
    torch = torch_cuda
    g = torch.Generator().manual_seed(5)
    n, K, HW = 2, 3, 700
    labels = torch.randint(-1, K, (n, HW), generator=g)
    logits = torch.rand(n, K, HW, generator=g) * 10 - 5
    logits += 200.0 * torch.nn.functional.one_hot(labels.clamp(min=0), K).permute(0, 2, 1)
    for gamma in (1.0, 2.0, 3.5):
        loss, sums, dl = _run(logits, labels.to(torch.int8), "focal", gamma)
        assert bool((loss == 0).all()) and bool((dl == 0).all()) and bool((sums[:, 1:3] == 0).all()), gamma
        assert bool((sums[:, 0] == sums[:, 3]).all()) and bool((sums[:, 3] == (labels >= 0).sum(dim=1).cuda()).all())
        assert bool(torch.isfinite(sums).all())
    loss, sums, dl = _run(logits, labels.to(torch.int8), "valid", 0.0)          # the same pixels without the focal factor: plain zeros too
    assert bool(torch.isfinite(loss).all() and torch.isfinite(dl).all()) and bool((sums[:, 1] == sums[:, 3]).all())


@pytest.mark.parametrize("weights", [False, True], ids=["plain", "weighted"])
def test_gamma_zero_makes_focal_the_valid_mean(torch_cuda, weights):
    """With gamma = 0 the focal mass B is W: "focal" agrees with the float64 reference of "valid" within its bound."""
    logits, labels, d2, cw, table = _inputs(1000, 8)
    extra = dict(cw=cw, d2=d2, table=table) if weights else {}
    loss, sums, dl = _run(logits, labels, "focal", 0.0, **extra)
    kw = dict(cw=extra.get("cw"), d2=extra.get("d2"), tab=extra.get("table"), gamma=0.0, normalise=1, grad_scale=GS)
    lref, sref, dref = loss_ref.loss_f64(logits, labels, **kw)
    rho = C_LOSS * R.U
    bnd = loss_ref.bounds(logits, labels, rho=rho, **kw)
    _bounded(sums, sref, bnd["sums"], rho, "sums", "sums")
    _bounded(loss, lref, bnd["loss"], rho, "loss", "loss")
    _bounded(dl, dref, bnd["dlogits"], rho, "dlogits", "dlogits")
    assert bool((sums[:, 0] == sums[:, 1]).all())


def _raw(torch, logits, labels, grad, pad=64):
    """gsa_loss_softmax called directly with loss, sums, the workspace and dlogits inside canary-filled buffers
    -> (loss, sums, dlogits or None, the buffers' guard regions as a list of (name, tensor, expected value))."""
    from gan_segmentation_amd import loss_ops
    from gan_segmentation_amd._runtime import launch
    n, K, HW = logits.shape
    dev = logits.device
    need = loss_ops.workspace_bytes(n, HW)
    lossb = torch.full((n + 2 * pad,), -7.0, device=dev)
    sumsb = torch.full((n * 4 + 2 * pad,), -7.0, device=dev, dtype=torch.float64)
    wsb = torch.full((need + 2 * pad * 8,), 0xA5, device=dev, dtype=torch.uint8)
    dlb = torch.full((logits.numel() + 2 * pad,), -7.0, device=dev)
    launch("gsa_loss_softmax", dev, n, K, HW, logits.data_ptr(), labels.data_ptr(), None, None, None, 2.0, 2, GS,
           wsb[pad * 8:].data_ptr(), sumsb[pad:].data_ptr(), lossb[pad:].data_ptr(), dlb[pad:].data_ptr() if grad else None)
    guards = [("loss", torch.cat([lossb[:pad], lossb[pad + n:]]), -7.0), ("sums", torch.cat([sumsb[:pad], sumsb[pad + 4 * n:]]), -7.0),
              ("workspace", torch.cat([wsb[:pad * 8], wsb[pad * 8 + need:]]), 0xA5),
              ("dlogits", torch.cat([dlb[:pad], dlb[pad + logits.numel():]]) if grad else dlb, -7.0)]
    return lossb[pad:pad + n], sumsb[pad:pad + 4 * n], (dlb[pad:pad + logits.numel()] if grad else None), guards


@pytest.mark.parametrize("HW", [257, 1000])
def test_forward_only_writes_loss_and_sums_and_nothing_else(torch_cuda, HW):
    torch = torch_cuda
    logits, labels, _d2, _cw, _table = _inputs(HW, 3)
    zl, zy = logits.cuda(), labels.cuda()
    keep_l, keep_y = zl.clone(), zy.clone()
    loss, sums, dl, guards = _raw(torch, zl, zy, True)
    floss, fsums, none, fguards = _raw(torch, zl, zy, False)
    assert none is None and _same_bits(floss, loss) and _same_bits(fsums, sums)
    for name, t, value in guards + fguards:
        assert bool((t == value).all()), "%s: a canary was overwritten" % name
    assert torch.equal(zl, keep_l) and torch.equal(zy, keep_y), "the inputs are not written"
    ref = _run(logits, labels, "focal", 2.0)
    assert _same_bits(ref[0], loss) and _same_bits(ref[1].reshape(-1), sums) and _same_bits(ref[2].reshape(-1), dl)


def test_value_errors(torch_cuda):
    torch = torch_cuda
    from gan_segmentation_amd import loss_ops
    from gan_segmentation_amd.loss_ops import LossSpec
    logits, labels, d2, cw, table = (t.cuda() for t in _inputs(255, 3))
    ok = loss_ops.softmax_loss(logits, labels, LossSpec(gamma=2, normalise="focal", class_weights=cw.tolist(),
                                                         boundary={"weight": 4.0, "sigma": 12.0, "radius": 32}), dist2=d2)
    kw = _run(logits.cpu(), labels.cpu(), "focal", 2.0, cw=cw.cpu(), d2=d2.cpu(), table=table.cpu())
    assert _same_bits(ok[0], kw[0]) and _same_bits(ok[1], kw[1])           # a spec and the keywords say the same (grad_scale differs)
    for bad in (dict(logits=logits.cpu()), dict(logits=logits.double()), dict(logits=logits[:, :1]), dict(logits=logits[:, :, ::2]),
                dict(labels=labels.long()), dict(labels=labels[:, :-1]), dict(gamma=0.5), dict(normalise="sum"),
                dict(class_weights=[1.0, 2.0]), dict(class_weights=cw[:2]), dict(class_weights=cw.double()),
                dict(dist2=d2), dict(table=table), dict(dist2=d2.int(), table=table), dict(dist2=d2, table=table[:-1]),
                dict(grad_scale=float("nan")), dict(spec=LossSpec(class_weights="median")), dict(spec={"gamma": 2}),
                dict(spec=LossSpec(boundary={"weight": 1.0, "sigma": 1.0, "radius": 2})),
                dict(workspace=torch.empty(8, device="cuda", dtype=torch.uint8))):
        args = dict(dict(logits=logits, labels=labels), **bad)
        with pytest.raises(ValueError):
            loss_ops.softmax_loss(**args)
    empty = loss_ops.softmax_loss(logits[:0], labels[:0])
    assert empty[0].shape == (0,) and empty[1].shape == (0, 4) and empty[2].shape == (0, 3, 255)
