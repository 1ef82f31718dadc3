"""The score histograms' kernels (csrc/gsa_scores.h) against ``rule_scores`` of tests/test_scores_host.py: every
word of every row, exactly -- the kernel counts integers and the rule is specified to the bit.

Every call writes into a row tensor pre-filled with garbage (every word is overwritten, nothing accumulates).  Shapes: HW of 1, 5,
255, 256, 257 and around the workgroup's stretch (GSA_SCORE_STRETCH - 1, exact, + 1, and two stretches and a bit: more than one
workgroup a sample), with K in {2, 3, 8}, n in {1, 2, 5} and shift in {0, 5, 8}; one 2 x 2 x 1024^2 case, where the block cap is
reached and every workgroup strides.  Both forms of the kernel: the aligned one (HW a multiple of 4, logits 16-byte and labels
4-byte aligned) and the scalar one, entered because of HW and because of either pointer."""
import functools

import numpy as np
import pytest

from tests.test_scores_host import BINS, rule_scores

pytestmark = pytest.mark.gpu

LABEL_POOL = (-1, -128, 127)            # and K, added per case: the ignored labels among the valid ones


def _stretch():
    from gan_segmentation_amd import score_ops
    return score_ops.SCORE_STRETCH


@functools.lru_cache(maxsize=None)
def _random_case(n, K, HW, spread=6.0, seed=0):
    """(logits (n, K, HW) float32, labels (n, HW) int8) on the host, drawn once a shape and never written: normal logits, so the
    margins cover a few hundred bins at shift 5 and both clamps at shift 8; a fifth of the labels ignored."""
    rng = np.random.default_rng(1000003 * seed + 1009 * HW + 31 * K + n)
    z = (rng.standard_normal((n, K, HW)) * spread).astype(np.float32)
    y = rng.integers(0, K, (n, HW)).astype(np.int8)
    ignored = rng.random((n, HW)) < 0.2
    y[ignored] = rng.choice(np.array(LABEL_POOL + (K,), np.int8), size=int(ignored.sum()))
    z.setflags(write=False)
    y.setflags(write=False)
    return z, y


def _garbage(shape, dev):
    import torch
    return torch.randint(-2 ** 62, 2 ** 62, shape, dtype=torch.int64, device=dev)


def _device_rows(z, y, shift, z_offset=0, y_offset=0):
    """score_histogram of host arrays; the logits start ``z_offset`` floats and the labels ``y_offset`` bytes into their buffers."""
    import torch
    from gan_segmentation_amd import score_ops
    dev = torch.device("cuda", 0)
    zb = torch.empty(z.size + z_offset, dtype=torch.float32, device=dev)
    yb = torch.empty(y.size + y_offset, dtype=torch.int8, device=dev)
    zt, yt = zb[z_offset:].view(z.shape), yb[y_offset:].view(y.shape)
    zt.copy_(torch.from_numpy(np.array(z)))
    yt.copy_(torch.from_numpy(np.array(y)))
    assert zt.data_ptr() % 16 == (4 * z_offset) % 16 and yt.data_ptr() % 4 == y_offset % 4
    out = _garbage((z.shape[0], z.shape[1], 2, BINS), dev)
    got = score_ops.score_histogram(zt, yt, shift=shift, out=out)
    assert got is out
    return out.cpu().numpy()


def _check(z, y, shift, **kw):
    got, want = _device_rows(z, y, shift, **kw), rule_scores(z, y, shift)
    bad = np.argwhere(got != want)
    assert not len(bad), "%d words differ, the first at %s: got %d, want %d" % (len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])])
    return got


def _shapes():
    S = 2048
    hws = (1, 5, 255, 256, 257, S - 1, S, S + 1, 2 * S + 4, 2 * S + 7)
    ns, shifts = (1, 2, 5), (0, 5, 8)
    return [(hw, K, ns[(i + j) % 3], shifts[(i + 2 * j) % 3]) for i, hw in enumerate(hws) for j, K in enumerate((2, 3, 8))]


@pytest.mark.parametrize("HW,K,n,shift", _shapes())
def test_every_word_is_the_rule(HW, K, n, shift):
    assert _stretch() == 2048, "the shapes above stand around the stretch"
    z, y = _random_case(n, K, HW)
    got = _check(z, y, shift)
    valid = ((y >= 0) & (y < K)).sum(axis=1)
    assert np.array_equal(got.sum(axis=(2, 3)), np.repeat(valid[:, None], K, axis=1))


@pytest.mark.parametrize("K", [4, 5, 6, 7])
def test_the_class_counts_in_between(K):
    for HW in (1000, 1003):
        _check(*_random_case(2, K, HW), 5)


@pytest.mark.parametrize("shift", [0, 5, 8])
def test_margins_on_the_bin_edges_and_the_specials(shift):
    """Two classes, z_1 the base and z_0 = base + margin, formed so that the fp32 difference IS the margin: on bin edges k / 2^shift
    and one ulp to either side, exactly 0, subnormal, beyond both clamps, infinite and NaN.  Both labels, so both histograms."""
    f = np.float32
    scale = 2.0 ** shift
    edges = np.array([k / scale for k in (-512, -511, -510, -100, -1, 0, 1, 2, 100, 510, 511, 512, 513)], f)
    margins = np.concatenate([edges, np.nextafter(edges, f(np.inf)), np.nextafter(edges, f(-np.inf)),
                              np.array([0.0, -0.0, 1e-45, -1e-45, 2.0 ** -127, 1e-38, -1e-38, 600.0, -600.0, 1e30, -1e30, 3e38, -3e38], f)])
    z0, z1 = margins.copy(), np.zeros_like(margins)
    # a subnormal difference of two normal numbers; inf and NaN in either place
    extra0 = np.array([1.5 * 2.0 ** -126, 2.0 ** -126, np.inf, -np.inf, np.inf, -np.inf, np.nan, 1.0, np.nan, np.inf, 3e38], f)
    extra1 = np.array([2.0 ** -126, 1.5 * 2.0 ** -126, np.inf, -np.inf, -np.inf, np.inf, 1.0, np.nan, np.nan, 1.0, -3e38], f)
    z = np.stack([np.concatenate([z0, extra0]), np.concatenate([z1, extra1])])[None]
    z = np.concatenate([z, z], axis=2)
    HW = z.shape[2]
    y = np.concatenate([np.zeros(HW // 2, np.int8), np.ones(HW // 2, np.int8)])[None]
    got = _check(z, y, shift)
    # the denormal mode of the build: a subnormal positive margin is in bin 512, not flushed into 511
    sub = np.array([[[1e-45, 1.5 * 2.0 ** -126], [0.0, 2.0 ** -126]]], f)
    rows = _check(sub, np.zeros((1, 2), np.int8), shift)
    assert rows[0, 0, 1, 512] == 2 and rows[0, 1, 0, 511] == 2 and rows.sum() == 4
    assert got.sum() == 2 * HW


def test_ties_among_two_and_among_all_classes():
    f = np.float32
    z = np.array([[[2.0, 1.0, 3.0, 0.0, np.nan, -np.inf], [2.0, 1.0, 3.0, 0.0, 1.0, -np.inf], [0.0, 1.0, 3.0, -1.0, 2.0, -np.inf]]], f)
    y = np.array([[0, 1, 2, 2, 0, 1]], np.int8)
    got = _check(z, y, 0)
    assert got[0, 0, 1, 511] == 1 and got[0, 1, 0, 511] == 3, "a tie gives both classes the margin 0: bin 511, not the winner's side"
    assert got[0, :, :, 512:].sum() == 0
    _check(z, y, 8)


def test_every_label_value_and_an_all_ignored_sample():
    K, HW = 3, 700
    z, _y = _random_case(3, K, HW)
    y = np.resize(np.arange(-128, 128, dtype=np.int16), (3, HW)).astype(np.int8)
    y[1] = np.resize(np.array(LABEL_POOL + (K,), np.int8), HW)          # nothing valid
    got = _check(z, y, 5)
    assert got[1].sum() == 0 and got[0].sum() > 0


@pytest.mark.parametrize("kind", ["confident", "noise"])
def test_confident_logits_and_noise(kind):
    """Confident: more than 99 % of the pixels in four words (own class in bin 1023, the other in bin 0), the rest near the boundary --
    the case the clamp words are counted per wave for.  Noise: uniform logits, every lane another bin."""
    rng = np.random.default_rng(7)
    n, K, HW = 2, 2, 3 * 4096
    y = (rng.random((n, HW)) < 0.3).astype(np.int8)
    if kind == "confident":
        z = np.where(np.arange(K)[None, :, None] == y[:, None, :], 30.0, -30.0).astype(np.float32)
        few = rng.random((n, HW)) < 0.005
        z[:, 0][few] = rng.standard_normal(int(few.sum())).astype(np.float32)
        z[:, 1][few] = rng.standard_normal(int(few.sum())).astype(np.float32)
    else:
        z = rng.uniform(-8, 8, (n, K, HW)).astype(np.float32)
    y[0, ::97] = -1
    got = _check(z, y, 5)
    if kind == "confident":
        four = got[:, 0, 1, 1023] + got[:, 0, 0, 0] + got[:, 1, 1, 1023] + got[:, 1, 0, 0]
        assert (four > 0.99 * got.sum(axis=(1, 2, 3))).all()
    else:
        assert (got > 0).sum() > 1500


@pytest.mark.parametrize("HW", [1024, 1021])
@pytest.mark.parametrize("z_offset,y_offset", [(0, 0), (4, 4), (1, 0), (2, 0), (3, 0), (0, 1), (0, 2), (0, 3), (1, 3), (4, 2)])
def test_logits_and_labels_anywhere_in_their_buffers(HW, z_offset, y_offset):
    """Logits 4, 8, 12 (and 16) bytes into their buffer, labels 1 to 3 (and 4) bytes into theirs: with HW = 1024 the aligned form at
    (0, 0) and (4, 4) and the scalar form for either pointer; with HW = 1021 the scalar form for HW."""
    z, y = _random_case(2, 3, HW)
    _check(z, y, 5, z_offset=z_offset, y_offset=y_offset)


def test_a_side_stream_and_the_batch_position():
    """The same rows on a side stream; a sample's row alone is its row at any position in a batch."""
    import torch
    from gan_segmentation_amd import score_ops
    z, y = _random_case(5, 3, 2 * 2048 + 8)
    want = rule_scores(z, y, 5)
    dev = torch.device("cuda", 0)
    zt, yt = torch.from_numpy(np.array(z)).to(dev), torch.from_numpy(np.array(y)).to(dev)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        out = _garbage((5, 3, 2, BINS), dev)
        score_ops.score_histogram(zt, yt, out=out)
    side.synchronize()
    assert np.array_equal(out.cpu().numpy(), want)
    for i in range(5):
        alone = score_ops.score_histogram(zt[i:i + 1], yt[i:i + 1]).cpu().numpy()
        assert np.array_equal(alone[0], want[i]), i
    order = [4, 2, 0, 3, 1]
    perm = score_ops.score_histogram(zt[order].contiguous(), yt[order].contiguous()).cpu().numpy()
    assert np.array_equal(perm, want[order])


def test_ffhq_size():
    """2 x 2 x 1024^2: 512 stretches a sample, the cap of workgroups reached, every workgroup eight trips."""
    from gan_segmentation_amd import score_ops
    HW = 1024 * 1024
    assert HW > score_ops.SCORE_STRETCH * score_ops.SCORE_MAX_BLOCKS
    rng = np.random.default_rng(11)
    y = (rng.random((2, HW)) < 0.4).astype(np.int8)
    z = (np.where(np.arange(2)[None, :, None] == y[:, None, :], 4.0, -4.0) + rng.standard_normal((2, 2, HW)) * 6).astype(np.float32)
    y[rng.random((2, HW)) < 0.1] = -1
    _check(z, y, 5)


def test_wrapper_arguments():
    import torch
    from gan_segmentation_amd import score_ops
    dev = torch.device("cuda", 0)
    z, y = _random_case(2, 3, 256)
    zt, yt = torch.from_numpy(np.array(z)).to(dev), torch.from_numpy(np.array(y)).to(dev)
    want = rule_scores(z, y, 5)
    rows = score_ops.score_histogram(zt.view(2, 3, 16, 16), yt.view(2, 16, 16))
    assert rows.shape == (2, 3, 2, BINS) and rows.dtype == torch.int64 and rows.device == zt.device
    assert np.array_equal(rows.cpu().numpy(), want)
    assert np.array_equal(score_ops.score_histogram(zt, yt, shift=5, out=rows).cpu().numpy(), want), "nothing accumulates"
    # empty input: no launch, an empty result; out of the wrong kind is refused all the same
    empty = score_ops.score_histogram(zt[:0], yt[:0])
    assert empty.shape == (0, 3, 2, BINS)
    keep = _garbage((0, 3, 2, BINS), dev)
    assert score_ops.score_histogram(zt[:0], yt[:0], out=keep) is keep
    for args, kw, match in (((zt.cpu(), yt), {}, "logits"), ((zt.double(), yt), {}, "logits"), ((zt[:, :, ::2], yt), {}, "logits"),
                            ((zt[:, :1].contiguous(), yt), {}, "classes"), ((torch.zeros(1, 9, 4, device=dev), yt), {}, "classes"),
                            ((zt, yt.to(torch.int16)), {}, "labels"), ((zt, yt[:1]), {}, "labels"), ((zt, yt.cpu()), {}, "labels"),
                            ((zt, yt), {"shift": 9}, "shift"), ((zt, yt), {"shift": 2.0}, "shift"),
                            ((zt, yt), {"out": rows[:1]}, "out"), ((zt, yt), {"out": rows.to(torch.int32)}, "out"),
                            ((zt, yt), {"out": rows.cpu()}, "out")):
        with pytest.raises(ValueError, match=match):
            score_ops.score_histogram(*args, **kw)


# ---- end to end --------------------------------------------------------------------------------------------------------------------
def test_solver_evaluate_scores_end_to_end(tmp_path, oracle_lib, capsys, monkeypatch):
    """The set-up of tests/test_metrics.py::test_solver_evaluate_end_to_end.  At margin 0 the curves give class 1's IoU of
    ``evaluate``'s confusion matrix, exactly; the rows are the rule's on the decoder's logits; `evaluate` prints the line with the
    key and not without it."""
    import torch
    from PIL import Image
    from gan_segmentation_amd import annotation_io, main as cli, params as P, weights as W
    from gan_segmentation_amd.metrics import ScoreCurves
    from gan_segmentation_amd.seg_solver import SegSolver
    from tests.common import reduced_setup
    gcfg, gp, dcfg, dp, z, noise = reduced_setup(6, batch=3)
    o = oracle_lib.Oracle(gcfg, gp, dcfg, dp)
    _rgb, img, feats = o.generator(z, noise)
    R = img.shape[1]
    rng = np.random.default_rng(5)
    data = tmp_path / "eval"
    labels = []
    for i in range(3):
        annotation_io.export_sample(str(data), i, img[i], [f[i] for f in feats])
        m = rng.choice(np.array([20, 128, 230], np.uint8), size=(R, R), p=[0.2, 0.4, 0.4])   # ignore / background / class 1
        Image.fromarray(m, "L").save(str(data / ("mask_%06d.png" % i)))
        labels.append(annotation_io.preprocess_mask(m))
    ckpt = tmp_path / "checkpoints"
    ckpt.mkdir()
    P.save_params(str(ckpt / "checkpoint_last.params"), W.complete_decoder_params(dcfg, dp))
    solver = SegSolver(6, str(data), str(ckpt), gpu_ids=[0], in_channels=W.generator_channels(gcfg))
    nclass = dcfg["num_classes"]
    assert nclass == 2
    conf = np.zeros((nclass, nclass), np.int64)
    want = ScoreCurves(nclass, shift=5)
    for i in range(3):
        f_i = [f[i] for f in feats]
        conf += solver.evaluate_batch(f_i, labels[i][None])[1]
        logits, _mask = solver.net(*f_i, want_mask=True)
        want.update_rows(rule_scores(logits.cpu().numpy().reshape(1, nclass, R * R), labels[i].reshape(1, R * R), 5))
    curves = solver.evaluate_scores(str(data))
    assert np.array_equal(curves.hist, want.hist)
    at0 = curves.at(1, 0.0)
    assert (at0["tp"], at0["fp"], at0["fn"]) == (conf[1, 1], conf[0, 1], conf[1, 0])
    assert at0["iou"] == int(conf[1, 1]) / int(conf[1, 1] + conf[0, 1] + conf[1, 0])
    assert np.array_equal(solver.evaluate_scores(str(data), shift=8).hist.sum(axis=(1, 2)), curves.hist.sum(axis=(1, 2)))
    # the CLI: the line appears with the key, and without it `evaluate` prints what it printed before
    monkeypatch.setattr(cli, "_solver", lambda cfg, keep_weights=False: solver)
    cfg = {"BASE_DIR": str(tmp_path), "GAN": "bedrooms"}
    assert cli.evaluate(dict(cfg)) == 0
    plain = capsys.readouterr().out
    assert cli.evaluate(dict(cfg, EVAL_SCORES=False, EVAL_SCORE_SHIFT=3)) == 0
    assert capsys.readouterr().out == plain and plain.count("\n") == 1 and "scores:" not in plain
    assert cli.evaluate(dict(cfg, EVAL_SCORES=True)) == 0
    with_key = capsys.readouterr().out
    assert with_key.startswith(plain) and with_key.count("\n") == 2
    line = with_key[len(plain):]
    assert line == "scores: %s\n" % ", ".join("%s: %.4f" % kv for kv in curves.get_name_value())
    assert line.startswith("scores: mean-auc: ") and "1-iou@0: %.4f" % at0["iou"] in line
    torch.cuda.synchronize()
