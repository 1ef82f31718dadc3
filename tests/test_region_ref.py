"""tests/region_ref.py checked against itself on the CPU: the float64 autograd reference against a plain numpy double-loop
restatement of csrc/gsa_region.h (gradient formula included) at HW = 7, K = 3, and against a central finite difference of its own
loss; and its bounds, which must be 0 exactly where the outputs are exact."""
import numpy as np
import pytest
import torch

from tests import region_ref

CASES = [dict(alpha=0.5, beta=0.5, smooth=1.0, mode=0), dict(alpha=0.3, beta=0.7, smooth=0.0, mode=1),
         dict(alpha=1.0, beta=1.0, smooth=1.0, mode=1), dict(alpha=0.3, beta=0.7, smooth=0.0, mode=0)]


def _tiny():
    g = torch.Generator().manual_seed(7)
    logits = ((torch.rand(3, 3, 7, generator=g) * 2 - 1) * 3).float()
    labels = torch.tensor([[0, 1, 1, -1, 0, 3, 1],         # class 2 absent; -1 and 3 ignored
                           [-1, -1, -1, -1, -1, -1, -1],
                           [2, 2, 0, 1, 1, 0, 2]])
    cw = torch.tensor([0.5, 2.0, 3.25])
    return logits, labels, cw


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("case", CASES)
def test_autograd_reference_is_the_double_loop_rule(case, weighted):
    logits, labels, cw = _tiny()
    kw = dict(case, cw=cw if weighted else None, grad_scale=0.75)
    got = region_ref.region_f64(logits, labels, **kw)
    want = region_ref.region_loops(logits.numpy(), labels.numpy(), **dict(kw, cw=cw.numpy() if weighted else None))
    for name, g, w in zip(("loss", "sums", "index", "dlogits"), got, want):
        assert np.allclose(g.numpy(), w, rtol=1e-12, atol=1e-15), (name, g, w)
    loss, sums, index, dl = got
    assert float(loss[1]) == 0.0 and not sums[1].any() and not index[1].any() and not dl[1].any()
    assert not dl[0][:, [3, 5]].any(), "an ignored pixel has gradient 0"
    assert sums[0, 2].tolist() == [2.0, 3.0, 0.0]
    if case["mode"] == 0:
        assert float(index[0, 2]) == 0.0, "an absent class is outside the set"
    elif case["smooth"] == 0.0:
        assert float(index[0, 2]) == 0.0 and float(sums[0, 1, 2]) > 0, "in the set, and scoring 0"


def test_gradient_is_the_finite_difference_of_the_loss():
    logits, labels, cw = _tiny()
    kw = dict(alpha=0.3, beta=0.7, smooth=1.0, mode=0, cw=cw)
    _loss, _sums, _index, dl = region_ref.region_f64(logits, labels, **kw)
    z = logits.double()
    h = 1e-6
    for s, k, i in [(0, 0, 0), (0, 2, 1), (0, 1, 4), (2, 2, 6), (2, 0, 3), (0, 1, 3)]:
        hi, lo = z.clone(), z.clone()
        hi[s, k, i] += h
        lo[s, k, i] -= h
        # region_f64 evaluates what it is given in float64: the perturbed logits need not be fp32 values
        fd = (float(region_ref.region_f64(hi, labels, **kw)[0].sum()) - float(region_ref.region_f64(lo, labels, **kw)[0].sum())) / (2 * h)
        assert fd == pytest.approx(float(dl[s, k, i]), rel=1e-6, abs=1e-9), (s, k, i)


def test_bounds_are_zero_where_the_outputs_are_exact():
    logits, labels, cw = _tiny()
    b = region_ref.bounds(logits, labels, alpha=0.3, beta=0.7, smooth=1.0, mode=0, cw=cw)
    assert b["loss"].shape == (3,) and b["sums"].shape == (3, 3, 3) and b["index"].shape == (3, 3) and b["dlogits"].shape == (3, 3, 7)
    assert not b["sums"][:, 2].any(), "G is a count"
    assert not b["loss"][1].any() and not b["sums"][1].any() and not b["index"][1].any() and not b["dlogits"][1].any()
    assert not b["dlogits"][0][:, [3, 5]].any() and float(b["index"][0, 2]) == 0.0
    assert bool((b["dlogits"][2] > 0).all()) and bool((b["index"][2] > 0).all()) and float(b["loss"][0]) > 0
