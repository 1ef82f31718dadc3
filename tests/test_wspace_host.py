"""W-space controls on the host side, without a GPU: the style-mixing plan and the truncation override."""
import numpy as np
import pytest

from gan_segmentation_amd import style_mix as M
from gan_segmentation_amd import weights as W

_M64 = (1 << 64) - 1


def _splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def _plan_ref(seed, index, prob, L):
    """The rule of style_mix's docstring restated on Python ints."""
    seed_b = (seed & _M64) ^ 0x5354594C454D4958
    u1 = _splitmix64(seed_b ^ index)
    u2 = _splitmix64(u1)
    return (u1 >> 11) * 2.0 ** -53 < prob, 1 + u2 % (L - 1)


def test_splitmix64_known_values():
    # SplitMix64 of the state sequence from 0 (the generator's published first outputs)
    assert int(M.splitmix64(np.uint64(0))) == 0xE220A8397B1DCDAF
    assert _splitmix64(0) == 0xE220A8397B1DCDAF


@pytest.mark.parametrize("seed", [0, 7, 2 ** 64 - 1])
@pytest.mark.parametrize("prob", [0.1, 0.5, 0.9])
def test_mix_plan_matches_the_stated_rule(seed, prob):
    L = 18
    mix, cutoff = M.mix_plan(seed, 0, 1000, prob, L)
    assert mix.dtype == np.bool_ and cutoff.dtype == np.int32 and mix.shape == cutoff.shape == (1000,)
    for i in range(1000):
        m, c = _plan_ref(seed, i, prob, L)
        assert bool(mix[i]) == m and int(cutoff[i]) == c, i
    assert 0 < mix.sum() < 1000


@pytest.mark.parametrize("L", [2, 12, 18])
def test_mix_plan_extremes_and_cutoff_range(L):
    mix0, c0 = M.mix_plan(3, 0, 500, 0.0, L)
    mix1, c1 = M.mix_plan(3, 0, 500, 1.0, L)
    assert not mix0.any() and mix1.all()
    assert np.array_equal(c0, c1)
    assert c1.min() >= 1 and c1.max() <= L - 1
    if L > 2:
        assert len(np.unique(c1)) == L - 1      # every cutoff occurs over 500 draws


def test_mix_plan_is_shard_invariant():
    whole = M.mix_plan(11, 0, 10, 0.5, 14)
    parts = [M.mix_plan(11, 0, 4, 0.5, 14), M.mix_plan(11, 4, 6, 0.5, 14)]
    for k in range(2):
        assert np.array_equal(whole[k], np.concatenate([p[k] for p in parts]))
    far = M.mix_plan(11, 2 ** 40, 3, 0.5, 14)
    for j in range(3):
        m, c = _plan_ref(11, 2 ** 40 + j, 0.5, 14)
        assert bool(far[0][j]) == m and int(far[1][j]) == c


def test_layer_select():
    sel = M.layer_select(np.array([True, False, True]), np.array([1, 3, 4]), 6)
    assert sel.shape == (3, 6)
    assert sel[0].tolist() == [False, True, True, True, True, True]
    assert not sel[1].any()
    assert sel[2].tolist() == [False, False, False, False, True, True]


def test_truncation_override():
    cfg = W.reduced_generator_config(7)
    L = W.num_style_layers(cfg)
    gp = W.synthetic_generator_params(cfg, seed=2)
    before = {k: v.copy() for k, v in gp.items()}
    out = W.with_truncation_psi(gp, 0.5, L)
    assert out["truncation_psi"].dtype == np.float32 and out["truncation_psi"].tolist() == [0.5] * L
    assert out["latent_avg"] is gp["latent_avg"]
    v = np.linspace(0.3, 1.0, L)
    assert np.array_equal(W.with_truncation_psi(gp, list(v), L)["truncation_psi"], v.astype(np.float32))
    # the caller's dict is left alone
    assert all(np.array_equal(gp[k], before[k]) for k in gp) and gp.keys() == before.keys()
    # None: the params unchanged
    same = W.with_truncation_psi(gp, None, L)
    assert same.keys() == gp.keys() and all(np.array_equal(same[k], before[k]) for k in gp)


@pytest.mark.parametrize("bad", [[0.5] * 3, [0.5] * 13, [[0.5] * 12], float("nan"), [0.7] * 11 + [float("inf")]])
def test_truncation_override_rejects(bad):
    cfg = W.reduced_generator_config(7)
    L = W.num_style_layers(cfg)
    assert L == 12
    with pytest.raises(ValueError):
        W.with_truncation_psi(W.synthetic_generator_params(cfg, seed=2), bad, L)
