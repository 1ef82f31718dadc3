"""The exactly summable bf16 fixtures (tests/exact_bf16.py) on the oracle alone: no GPU, no code under test.

tests/test_gpu_bf16_exact.py holds the bf16 HIP path to the bf16 oracle bit for bit on these fixtures.  That is a fair demand only if
summation order cannot change a single accumulation, and it is a useful one only if the fixtures are lively and react to every weight.
Both are shown here:
 * precondition -- Oracle.exact_headroom() >= MIN_HEADROOM bits for every fixture, on the z path and on the W path, generator and
   decoder together.  headroom = 24 - log2(sum|a*w| / q) > 0 means every partial sum in every order is a multiple of q below 2^24 q,
   hence exact in fp32; the 2 bits of margin make that hold for any adder that keeps at least 22 bits below its largest aligned term;
 * the witness is no rubber stamp -- ordinary weights, and a fixture with a single weight replaced by 1/3, report negative headroom;
 * liveness -- w depends on z, no operand tensor sits on a handful of bf16 codes, every class occurs, no colour saturates;
 * sensitivity -- one weight step in each convolution family, and one bf16 step of an AdaIN bias, changes the oracle's output.
"""
import hashlib

import numpy as np
import pytest

from tests.common import reduced_setup, unsaturated_colours, w_spread
from tests.exact_bf16 import EXACT_CASES, STEP, checked_samples, exact_dlatents, exact_setup, take

MIN_HEADROOM = 2.0      # bits
MIN_CODES = 32          # distinct bf16 codes per operand tensor


def _digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _inputs(name, batch):
    gcfg, gp, dcfg, dp, z, noise = exact_setup(name, batch)
    zc, nc = take(z, noise, checked_samples(batch))
    return gcfg, gp, dcfg, dp, zc, nc


@pytest.mark.parametrize("name,batch", EXACT_CASES)
def test_precondition_every_accumulation_is_exactly_summable(oracle_lib, name, batch):
    gcfg, gp, dcfg, dp, z, noise = _inputs(name, batch)
    o = oracle_lib.Oracle(gcfg, gp, dcfg, dp, precision="bf16", witness=True)
    assert o.exact_headroom() == float("inf"), "nothing ran yet"
    _rgb, _img, feats = o.generator(z, noise)
    o.decoder(feats)
    hz = o.exact_headroom()
    dl = exact_dlatents(o, gcfg, batch)[checked_samples(batch)]
    _rgb, _img, feats = o.generator_w(dl, noise)
    o.decoder(feats)
    hw = o.exact_headroom()
    print("%s batch %d: headroom %.2f bits (z path), %.2f bits (W path)" % (name, batch, hz, hw))
    assert hz >= MIN_HEADROOM and hw >= MIN_HEADROOM, (hz, hw)
    # the fused pair entry walks the same accumulations
    o.generate(z[:1], [a[:1] for a in noise])
    assert MIN_HEADROOM <= o.exact_headroom() < float("inf")


def test_witness_is_silent_in_fp32_mode_and_rejects_ordinary_weights(oracle_lib):
    gcfg, gp, dcfg, dp, z, noise = reduced_setup(7, batch=1)
    o32 = oracle_lib.Oracle(gcfg, gp, dcfg, dp, witness=True)
    o32.decoder(o32.generator(z, noise)[2])
    assert o32.exact_headroom() == float("inf"), "the witness watches the bf16 mode only"
    unarmed = oracle_lib.Oracle(gcfg, gp, dcfg, dp, precision="bf16")
    unarmed.generator(z, noise, want_feats=False)
    with pytest.raises(oracle_lib.OracleError, match="not armed"):      # never an answer that reads as "exact"
        unarmed.exact_headroom()
    o = oracle_lib.Oracle(gcfg, gp, dcfg, dp, precision="bf16", witness=True)
    feats = o.generator(z, noise)[2]
    hg = o.exact_headroom()
    o.decoder(feats)
    hd = o.exact_headroom()
    print("ordinary synthetic weights: headroom %.2f bits (generator), %.2f bits (decoder)" % (hg, hd))
    assert hg < 0 and hd < 0


def test_witness_rejects_one_weight_of_one_third(oracle_lib):
    """bf16(1/3) = 171 * 2^-9 against the fixture's k * 2^-3: q shrinks by 2^6, so a call with less than 6 bits of headroom goes negative.
    E32c's 512-channel convolutions have about 4.5."""
    gcfg, gp, _dcfg, _dp, z, noise = _inputs("E32c", 1)
    o = oracle_lib.Oracle(gcfg, gp, precision="bf16", witness=True)
    o.generator(z, noise)
    good = o.exact_headroom()
    bad = dict(gp)
    bad["4_conv_2_weight"] = gp["4_conv_2_weight"].copy()
    bad["4_conv_2_weight"][3, 5, 1, 1] = 1.0 / 3.0
    o = oracle_lib.Oracle(gcfg, bad, precision="bf16", witness=True)
    o.generator(z, noise)
    h = o.exact_headroom()
    print("E32c: headroom %.2f bits, with one weight of 1/3: %.2f bits" % (good, h))
    assert MIN_HEADROOM <= good < 6.0 and h < 0


@pytest.mark.parametrize("name,batch", EXACT_CASES)
def test_fixture_is_lively(oracle_lib, name, batch):
    gcfg, gp, dcfg, dp, z, noise = _inputs(name, batch)
    o = oracle_lib.Oracle(gcfg, gp, dcfg, dp, precision="bf16", witness=True)
    spread = w_spread(o.mapping(np.random.default_rng(1).standard_normal((4, 512)).astype(np.float32)))
    assert spread > 0.1, "w must depend on z, spread %.3g" % spread
    _rgb, img, feats = o.generator(z, noise)
    _logits, mask = o.decoder(feats)
    codes = o.exact_operand_codes()
    print("%s batch %d: w spread %.2f, fewest bf16 codes in an operand tensor %d, classes %s" % (
        name, batch, spread, codes, np.bincount(mask.ravel()).tolist()))
    assert codes >= MIN_CODES, "an operand tensor or stored activation uses only %d bf16 codes" % codes
    assert len(np.unique(mask)) == dcfg["num_classes"], "classes in the mask: %s" % np.unique(mask)
    assert unsaturated_colours(img) == list(range(gcfg["channels"]))
    for s in range(1, len(z)):
        assert not np.array_equal(img[s], img[0]), "samples 0 and %d give the same image" % s


def _steps(gcfg, dcfg):
    """(family, parameter, index, step): one step in each convolution family at its lowest and at its highest level, and an AdaIN bias.
    The 3x3 / 4x4 steps sit on a corner tap: the zero padding then makes the change differ over the plane.  (A centre-tap step at 4 px
    adds nearly the same amount to all 16 pixels of its channel -- the operands sit in [1.3, 1.75] -- and the instance norm takes that
    out again before anything downstream reads it.)"""
    top, n = 2 ** gcfg["max_res_log2"], len(dcfg["in_channels"])
    gen = [("conv_2", "4_conv_2_weight"), ("conv_2", "%d_conv_2_weight" % top), ("conv_1", "8_conv_1_weight"),
           ("conv_1", "%d_conv_1_weight" % min(top, 64))]
    if top >= 128:
        gen += [("deconv_1", "128_deconv_1_weight"), ("deconv_1", "%d_deconv_1_weight" % top)]
    out = [(fam, key, (1, 2, 0, 0), STEP) for fam, key in sorted(set(gen))]
    out.append(("adain bias", "4_adain_1_dense_affine_bias", (-1,), 2.0 ** -7))           # yb = 1.5 of the last channel: one bf16 step
    out.append(("adain bias", "%d_adain_2_dense_affine_bias" % top, (0,), 2.0 ** -11))    # ys = -0.9375 of channel 0: one bf16 step
    dec = [("cvt", "cvt_block_0.0.weight"), ("cvt", "cvt_block_%d.0.weight" % (n - 1))]
    for i in sorted({0, n - 2}):
        dec += [("res a", "main_block_%d.1.base_layers.0.weight" % i), ("res b", "main_block_%d.1.base_layers.3.weight" % i)]
    out += [(fam, key, (1, 2, 0, 0), STEP) for fam, key in dec]
    out += [("shortcut", "main_block_%d.1.shortcut.0.weight" % i, (1, 2, 0, 0), 0.25) for i in sorted({1, n - 2})]
    return out


@pytest.mark.parametrize("name,batch", [c for c in EXACT_CASES if c[1] <= 3])
def test_one_weight_step_changes_the_output(oracle_lib, name, batch):
    gcfg, gp, dcfg, dp, z, noise = _inputs(name, batch)
    z, noise = z[:1], [a[:1] for a in noise]
    o = oracle_lib.Oracle(gcfg, gp, dcfg, dp, precision="bf16")
    rgb, _img, feats = o.generator(z, noise)
    logits, _mask = o.decoder(feats)
    base = {"g": _digest(rgb), "d": _digest(logits)}
    families = set()
    for fam, key, index, step in _steps(gcfg, dcfg):
        which = "d" if "block" in key else "g"
        params = dict(gp if which == "g" else dp)
        params[key] = params[key].copy()
        params[key][index] += np.float32(step)
        if which == "g":
            out = oracle_lib.Oracle(gcfg, params, precision="bf16").generator(z, noise, want_feats=False)[0]
        else:
            out = oracle_lib.Oracle(None, None, dcfg, params, precision="bf16").decoder(feats)[0]
        changed = int((out != (rgb if which == "g" else logits)).sum())
        print("%s: %s %s%s + %g changes %d of %d values" % (name, fam, key, list(index), step, changed, out.size))
        assert _digest(out) != base[which], "%s: one step in %s%s is invisible" % (name, key, list(index))
        families.add(fam)
    want = {"conv_1", "conv_2", "adain bias", "cvt", "res a", "res b", "shortcut"} | ({"deconv_1"} if gcfg["max_res_log2"] >= 7 else set())
    assert families == want
