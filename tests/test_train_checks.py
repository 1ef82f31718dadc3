"""The comparison rules of tests/f64_ref.py can fail: on the CPU, references perturbed the way a wrong kernel would be
(a 64-pixel unit of the weight gradient dropped or doubled, a border tap lost, the last channel of the last 64-channel
slice lost, x0 / x1 swapped at the concat boundary) are rejected at the shapes of tests/test_train_kernels.py, while a
float32 evaluation of the same operations (another summation order) is accepted.  No GPU needed.

In bounded mode a dropped or doubled unit of a 1024^2 weight gradient is a change of about sqrt(64) products in a sum of
2**20, far inside any rounding allowance for that sum: only exact mode sees it, which is why exact mode exists."""
import pytest
import torch
import torch.nn.functional as F

from tests import f64_ref as R
from tests.test_train_kernels import C_DOT, CONV_CASES


def _inputs(case, exact, seed=0):
    n, C0, C1, Cout, K, up, Hs, Ws, _ = CONV_CASES[case]
    g = torch.Generator().manual_seed(seed)
    mk = (lambda *s: R.small_ints(s, g)) if exact else (lambda *s: torch.randn(*s, generator=g))
    x0, x1 = mk(n, C0, Hs, Ws), (mk(n, C1, Hs, Ws) if C1 else None)
    w, b, dy = mk(Cout, C0 + C1, K, K), mk(Cout), mk(n, Cout, Hs << up, Ws << up)
    return x0, x1, w, b, up, dy


def _checker(exact, case, bnd):
    n, C0, C1, Cout, K, up, Hs, Ws, _ = CONV_CASES[case]
    N = {"out": (C0 + C1) * K * K, "dxu": Cout * K * K, "dw": n * (Hs << up) * (Ws << up), "db": n * (Hs << up) * (Ws << up)}

    def check(key, got, ref):
        if exact:
            R.assert_exact(got, ref, key)
        else:
            R.assert_bounded(got, ref, bnd[key], R.rho_dot(N[key], C_DOT), key)
    return check


def _unit_wgrad(x, dy, L0):
    """Contribution of the 64 pixels L0..L0+63 of sample 0 (one row segment, W >= 64) to dW of a 3x3 convolution."""
    W = x.shape[3]
    y, x0 = divmod(L0, W)
    xp = F.pad(x[0].double(), (1, 1, 1, 1))
    d = dy[0, :, y, x0:x0 + 64].double()
    out = torch.empty(dy.shape[1], x.shape[1], 3, 3, dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            out[:, :, ky, kx] = d @ xp[:, y + ky, x0 + kx:x0 + kx + 64].T
    return out


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "bounded"])
def test_persistent_shape_rejects_lost_units_and_taps(exact):
    case = "1024_16to32"
    x0, x1, w, b, up, dy = _inputs(case, exact)
    ref = R.conv_ref(x0, x1, w, b, up, dy)
    bnd = None if exact else R.conv_bound(x0, x1, w, b, up, dy)
    check = _checker(exact, case, bnd)
    f32 = R.conv_ref(x0, x1, w, b, up, dy, dtype=torch.float32)
    for key in ("out", "dxu", "dw", "db"):
        check(key, f32[key], ref[key])                       # another summation order: accepted

    W = x0.shape[3]
    # a border tap lost: output (0, :, 517, W-2) without tap (1, 2), which reads the last input column
    tap = torch.einsum("c,oc->o", x0[0, :, 517, W - 1].double(), w[:, :, 1, 2].double())
    assert bool((tap != 0).any())
    bad = ref["out"].clone()
    bad[0, :, 517, W - 2] -= tap
    with pytest.raises(AssertionError):
        check("out", bad, ref["out"])
    if exact:
        # one 64-pixel unit of the weight gradient dropped / doubled (in bounded mode at 2**20 pixels this is within rounding)
        unit = _unit_wgrad(x0, dy, 64 * 5000)
        assert bool((unit != 0).any())
        for bad in (ref["dw"] - unit, ref["dw"] + unit):
            with pytest.raises(AssertionError):
                check("dw", bad, ref["dw"])


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "bounded"])
def test_staging_shape_rejects_lost_channel_and_swapped_sources(exact):
    case = "cin130_cout3_up"            # C0 = 70, C1 = 60: slices of 64 + 64 + 2 channels, the boundary inside group 68..71
    x0, x1, w, b, up, dy = _inputs(case, exact, seed=1)
    ref = R.conv_ref(x0, x1, w, b, up, dy)
    bnd = None if exact else R.conv_bound(x0, x1, w, b, up, dy)
    check = _checker(exact, case, bnd)
    f32 = R.conv_ref(x0, x1, w, b, up, dy, dtype=torch.float32)
    for key in ("out", "dxu", "dw", "db"):
        check(key, f32[key], ref[key])

    # the last channel of the final slice left out
    w_lost = w.clone()
    w_lost[:, -1] = 0
    lost = R.conv_ref(x0, x1, w_lost, b, up, dy)
    with pytest.raises(AssertionError):
        check("out", lost["out"], ref["out"])
    with pytest.raises(AssertionError):
        check("dxu", lost["dxu"], ref["dxu"])
    # x0 and x1 swapped at the concat boundary: channel 69 read from x1, channel 70 from x0
    s0, s1 = x0.clone(), x1.clone()
    s0[:, -1], s1[:, 0] = x1[:, 0], x0[:, -1]
    swapped = R.conv_ref(s0, s1, w, b, up, dy)
    with pytest.raises(AssertionError):
        check("out", swapped["out"], ref["out"])
    with pytest.raises(AssertionError):
        check("dw", swapped["dw"], ref["dw"])


def test_persistent_cases_walk_several_units():
    """The launch restatement of tests/f64_ref.py: every case marked persistent in tests/test_train_kernels.py walks >= 2
    units per block / wave (raise CONV_BLOCKS or WGRAD_BLOCKS there and this fails), and the pre-existing shapes of
    tests/test_train_ops.py walk exactly one."""
    from tests.test_train_kernels import _assert_persistent
    for name, (n, C0, C1, Cout, K, up, Hs, Ws, persistent) in CONV_CASES.items():
        if persistent:
            _assert_persistent(n, C0 + C1, Cout, Hs << up, Ws << up)
    assert R.conv_units_per_block(2, 32, 80, 80) == 1 and R.wgrad_units_per_wave(2, 16, 32, 80, 80) == 1
