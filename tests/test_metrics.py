"""Evaluation arithmetic: the confusion-matrix bookkeeping of the product against the
literal restatement of the reference's histogram code (oracle/ref_metrics.py), and -- on the GPU -- the device
kernel and ``SegSolver.evaluate`` against both."""
import os

import numpy as np
import pytest

from gan_segmentation_amd.metrics import SegmentationMetric
from oracle import ref_metrics


def _random_case(rng, n, k, R, ignore_frac=0.2):
    logits = rng.standard_normal((n, k, R, R)).astype(np.float32) * 3
    labels = rng.integers(0, k, (n, R, R)).astype(np.int32)
    labels[rng.random((n, R, R)) < ignore_frac] = -1
    return logits, labels


def _confusion(logits, labels, k):
    pred = np.argmax(logits, 1)
    c = np.zeros((k, k), np.int64)
    ok = labels >= 0
    np.add.at(c, (labels[ok], pred[ok]), 1)
    return c


@pytest.mark.parametrize("k", [2, 3, 5])
def test_confusion_bookkeeping_equals_reference_histograms(k):
    rng = np.random.default_rng(k)
    logits, labels = _random_case(rng, 3, k, 32)
    m = SegmentationMetric(k, skip_bg=True)
    m.update_confusion(_confusion(logits[:2], labels[:2], k))       # two updates accumulate like the reference's
    m.update_confusion(_confusion(logits[2:], labels[2:], k))
    (_n1, _n2), (acc, miou) = m.get()
    acc_o, miou_o, _loss = ref_metrics.evaluate(logits, labels, k)
    assert acc == acc_o and miou == miou_o


def test_metric_edge_cases():
    m = SegmentationMetric(2)
    m.update_confusion(np.array([[5, 0], [0, 0]]))      # class 1 never labelled nor predicted: dropped like the reference does
    names, (acc, miou) = m.get()
    assert names == ["accuracy", "mean-iou"] and acc == pytest.approx(1.0) and np.isnan(miou)
    m.reset()
    m.update_confusion(np.array([[3, 1], [2, 4]]))
    _names, (acc, miou) = m.get()
    assert acc == pytest.approx(0.7) and miou == pytest.approx(4 / 7)
    logits = np.array([[[[0.0]], [[0.0]]]], np.float32)           # a tie -> first maximum -> class 0
    assert ref_metrics.weighted_softmax_ce(logits, np.array([[[1]]]))[0] == pytest.approx(np.log(2.0))
    assert ref_metrics.weighted_softmax_ce(logits, np.array([[[-1]]]))[0] == 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("k", [2, 3, 8])
def test_device_eval_kernel(k):
    import torch
    from gan_segmentation_amd._runtime import DeviceModel, current_stream_ptr
    rng = np.random.default_rng(10 + k)
    logits, labels = _random_case(rng, 3, k, 64)
    logits[0, :, 0, 0] = 1.5                                  # a tie: first maximum wins
    model = DeviceModel(0)
    dev = model.device
    lg = torch.from_numpy(logits).to(dev)
    lb = torch.from_numpy(labels.astype(np.int8)).to(dev)
    conf = torch.zeros((k, k), dtype=torch.int64, device=dev)
    lossf = torch.zeros((3,), dtype=torch.int64, device=dev)
    for _ in range(2):                                        # the buffers accumulate
        model.ctx.segmentation_eval(current_stream_ptr(dev), 3, k, 64, 64, lg.data_ptr(), lb.data_ptr(), conf.data_ptr(), lossf.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(conf.cpu().numpy(), 2 * _confusion(logits, labels, k))          # integers: exact
    loss = lossf.cpu().numpy().astype(np.float64) / 2.0 ** 32 / (64 * 64) / 2
    ref = ref_metrics.weighted_softmax_ce(logits, labels)
    assert np.abs(loss - ref).max() <= 2e-6 * max(1.0, ref.max())
    from gan_segmentation_amd import _lib
    with pytest.raises(_lib.GsaError, match="2..8 classes"):
        model.ctx.segmentation_eval(current_stream_ptr(dev), 3, 9, 64, 64, lg.data_ptr(), lb.data_ptr(), conf.data_ptr(), lossf.data_ptr())


@pytest.mark.gpu
def test_solver_evaluate_end_to_end(tmp_path, oracle_lib):
    """SegSolver.evaluate over annotator sample files == the oracle decoder + the reference's metric code."""
    from PIL import Image
    from gan_segmentation_amd import annotation_io, weights as W
    from gan_segmentation_amd.seg_solver import SegSolver
    from tests.common import reduced_setup
    gcfg, gp, dcfg, dp, z, noise = reduced_setup(6, batch=3)
    o = oracle_lib.Oracle(gcfg, gp, dcfg, dp)
    _rgb, img, feats = o.generator(z, noise)
    R = img.shape[1]
    rng = np.random.default_rng(5)
    data = tmp_path / "data"
    masks = []
    for i in range(3):
        annotation_io.export_sample(str(data), i, img[i], [f[i] for f in feats])
        m = rng.choice(np.array([20, 128, 230], np.uint8), size=(R, R), p=[0.2, 0.4, 0.4])   # ignore / background / class 1
        Image.fromarray(m, "L").save(str(data / ("mask_%06d.png" % i)))
        masks.append(annotation_io.preprocess_mask(m))
    ckpt = tmp_path / "checkpoints"
    ckpt.mkdir()
    from gan_segmentation_amd import params as P
    P.save_params(str(ckpt / "checkpoint_last.params"), W.complete_decoder_params(dcfg, dp))
    solver = SegSolver(6, str(data), str(ckpt), gpu_ids=[0], in_channels=W.generator_channels(gcfg))
    assert solver.is_trained
    out_dir = tmp_path / "eval_out"
    result = dict(solver.evaluate(str(data), output_dir=str(out_dir)))
    # oracle side: logits of the canonical decoder on the SAME stored features (pickles hold them exactly)
    logits_o, _mask_o = o.decoder(feats)
    labels = np.stack(masks)
    acc_o, miou_o, loss_o = ref_metrics.evaluate(logits_o, labels, dcfg["num_classes"])
    assert result["accuracy"] == acc_o and result["mean-iou"] == miou_o          # integer counts behind both
    assert abs(result["total-loss"] - loss_o.mean()) <= 2e-6 * max(1.0, loss_o.mean())
    for i in range(3):
        for name in ("img_%06d.jpg", "mask_%06d.png", "gt_mask_%06d.png", "metrics_%06d.txt"):
            assert os.path.exists(str(out_dir / (name % i)))
    gt = np.asarray(Image.open(str(out_dir / "gt_mask_000001.png")))
    assert set(np.unique(gt)) <= {0, 128, 255} and np.array_equal(gt == 255, masks[1] == 1)


# ---- FFHQ size: the stride loop of seg_eval_kernel -------------------------------------------------------------------
# launch_seg_eval (csrc/gsa_kernels.hip) caps grid.x at 1024 workgroups of 256 pixels; an image of more than EVAL_PIXELS_PER_PASS
# pixels makes every thread walk several pixels.  Of the product's sizes only 1024^2 (FFHQ evaluation) does.
EVAL_PIXELS_PER_PASS = 1024 * 256


def test_the_eval_grid_cap_is_the_one_these_tests_assume():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gan-segmentation_amd", "csrc", "gsa_kernels.hip")).read()
    assert "const dim3 grid(std::min((HW + 255) / 256, 1024), n);" in src


@pytest.mark.parametrize("k,scale", [(2, 3.0), (8, 3.0), (2, 30.0), (8, 30.0), (5, 30.0)])
def test_float64_log_softmax_against_the_restatement(k, scale):
    """tests/f64_ref.weighted_softmax_ce_f64 (float64 throughout) and oracle/ref_metrics.weighted_softmax_ce (fp32 per pixel) agree
    within the bound the device is held to, 2e-6 * max(1, ref); the integer counts of both formulations are equal."""
    from tests import f64_ref
    rng = np.random.default_rng(k)
    logits, labels = _random_case(rng, 2, k, 256)
    logits = (logits / 3 * scale).astype(np.float32)
    ref = f64_ref.weighted_softmax_ce_f64(logits, labels)
    d = np.abs(ref_metrics.weighted_softmax_ce(logits, labels) - ref)
    print("K = %d, scale %g: fp32 restatement vs float64: max %.3e (loss %.4f)" % (k, scale, d.max(), ref.max()))
    assert (d <= 2e-6 * np.maximum(1.0, ref)).all()
    assert np.array_equal(f64_ref.confusion_i64(logits, labels, k), _confusion(logits, labels, k))


def _device_eval(logits, labels, k, calls=1):
    """gsa_segmentation_eval `calls` times into the same zeroed buffers -> (confusion (k,k) int64, loss_fixed (n,) int64)."""
    import torch
    from gan_segmentation_amd._runtime import DeviceModel, current_stream_ptr
    model = DeviceModel(0)
    dev = model.device
    n, _k, H, W = logits.shape
    lg = torch.from_numpy(logits).to(dev)
    lb = torch.from_numpy(labels.astype(np.int8)).to(dev)
    conf = torch.zeros((k, k), dtype=torch.int64, device=dev)
    lossf = torch.zeros((n,), dtype=torch.int64, device=dev)
    for _ in range(calls):
        model.ctx.segmentation_eval(current_stream_ptr(dev), n, k, H, W, lg.data_ptr(), lb.data_ptr(), conf.data_ptr(), lossf.data_ptr())
    torch.cuda.synchronize()
    return conf.cpu().numpy(), lossf.cpu().numpy()


def _loss(loss_fixed, HW, calls=1):
    return loss_fixed.astype(np.float64) / 2.0 ** 32 / HW / calls


_FULL_SIZE = ([(1024, 1024, k, 2) for k in range(2, 9)]      # four passes of the capped grid, every class count
              + [(1024, 1024, 5, 8),                         # the same at 8 samples (grid.y)
                 (768, 768, 3, 3),                           # 2.25 passes: a partial third pass
                 (512, 512, 8, 2),                           # exactly the cap: one pass, no second
                 (33, 33, 4, 3)])                            # 1089 pixels: not a multiple of 256


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [3.0, 30.0])
@pytest.mark.parametrize("H,W,k,n", _FULL_SIZE)
def test_device_eval_kernel_at_full_size(torch_cuda, H, W, k, n, scale):
    """Logits N(0, scale^2), 20 % of the pixels ignored: the counts equal a numpy int64 count after one call and after two
    accumulating calls; the loss is within 2e-6 * max(1, ref) of the float64 log-softmax, per sample.
    Measured on an MI355X, |device - float64| / max(1, ref): 1.0e-9 .. 2.8e-9 at 1024^2, 768^2 and 512^2 (every class count, both scales,
    one call and two), 5.3e-9 at 33 x 33 (the fp32 numpy restatement on the CPU: 4e-10 .. 4e-8)."""
    from tests import f64_ref
    if (H, W) in ((1024, 1024), (768, 768)):
        assert H * W > EVAL_PIXELS_PER_PASS, "the case must take the stride loop"
    rng = np.random.default_rng(1000 * k + H + n)
    logits = (rng.standard_normal((n, k, H, W), dtype=np.float32) * np.float32(scale))
    labels = rng.integers(0, k, (n, H, W)).astype(np.int32)
    labels[rng.random((n, H, W)) < 0.2] = -1
    logits[0, :, 0, 0] = 1.5                                  # a tie: first maximum wins
    want = f64_ref.confusion_i64(logits, labels, k)
    ref = f64_ref.weighted_softmax_ce_f64(logits, labels)
    worst = 0.0
    for calls in (1, 2):
        conf, lossf = _device_eval(logits, labels, k, calls)
        assert np.array_equal(conf, calls * want), "%d call(s): counts differ:\n%s\nwant\n%s" % (calls, conf, calls * want)
        d = np.abs(_loss(lossf, H * W, calls) - ref) / np.maximum(1.0, ref)
        worst = max(worst, float(d.max()))
        print("%dx%d K=%d n=%d scale %g, %d call(s): |loss - float64| / max(1, ref) = %.3e (loss %.4f)" % (H, W, k, n, scale, calls, d.max(), ref.max()))
        assert (d <= 2e-6).all(), "%d call(s): loss %s vs float64 %s" % (calls, _loss(lossf, H * W, calls), ref)


@pytest.mark.gpu
def test_device_eval_kernel_edges_at_full_size(torch_cuda):
    """1024^2, 3 classes, four samples in one call: (0) every logit of a pixel equal -- prediction 0 everywhere, loss ln 3 on the
    labelled pixels; (1) entirely ignored -- its loss word stays 0 and it adds no count; (2) every label the same class, nothing
    ignored; (3) random, with the tie pixel of test_device_eval_kernel."""
    from tests import f64_ref
    H = W = 1024
    k, n = 3, 4
    assert H * W > EVAL_PIXELS_PER_PASS
    rng = np.random.default_rng(77)
    logits = rng.standard_normal((n, k, H, W), dtype=np.float32) * np.float32(3)
    labels = rng.integers(0, k, (n, H, W)).astype(np.int32)
    labels[rng.random((n, H, W)) < 0.2] = -1
    logits[0] = logits[0, :1]                                 # the same value in every class, a different one per pixel
    labels[1] = -1
    labels[2] = 2
    logits[3, :, 0, 0] = 1.5
    conf, lossf = _device_eval(logits, labels, k)
    assert np.array_equal(conf, f64_ref.confusion_i64(logits, labels, k))
    ref = f64_ref.weighted_softmax_ce_f64(logits, labels)
    loss = _loss(lossf, H * W)
    assert (np.abs(loss - ref) <= 2e-6 * np.maximum(1.0, ref)).all(), "%s vs %s" % (loss, ref)
    assert lossf[1] == 0 and ref[1] == 0.0
    assert abs(loss[0] - np.log(3.0) * np.mean(labels[0] >= 0)) <= 2e-6
    # each sample alone: sample 0 predicts class 0 only, sample 1 counts nothing, sample 2 fills row 2 only
    for i in range(3):
        c, lf = _device_eval(logits[i:i + 1], labels[i:i + 1], k)
        assert np.array_equal(c, f64_ref.confusion_i64(logits[i:i + 1], labels[i:i + 1], k))
        assert lf[0] == lossf[i], "sample %d: the loss word depends on the batch" % i
        if i == 0:
            assert c[:, 1:].sum() == 0 and c.sum() == (labels[0] >= 0).sum()
        if i == 1:
            assert c.sum() == 0
        if i == 2:
            assert c[:2].sum() == 0 and c[2].sum() == H * W


@pytest.mark.gpu
def test_device_eval_kernel_drops_labels_beyond_the_class_count(torch_cuda):
    """include/gsa.h: a label outside 0..classes-1 is treated like -1 (ignored), whatever its value -- no count, no loss, and
    nothing written outside the classes x classes counts."""
    from tests import f64_ref
    H = W = 1024
    k = 3
    rng = np.random.default_rng(78)
    logits = rng.standard_normal((2, k, H, W), dtype=np.float32) * np.float32(3)
    labels = rng.integers(0, k, (2, H, W)).astype(np.int32)
    inside = labels.copy()
    beyond = rng.random((2, H, W)) < 0.3
    labels[beyond] = rng.choice(np.array([3, 4, 7, 8, 100, 127, -2, -128]), size=int(beyond.sum()))
    inside[beyond] = -1
    conf, lossf = _device_eval(logits, labels, k)
    conf_i, lossf_i = _device_eval(logits, inside, k)
    assert np.array_equal(conf, conf_i) and np.array_equal(lossf, lossf_i)
    assert np.array_equal(conf, f64_ref.confusion_i64(logits, labels, k))
    ref = f64_ref.weighted_softmax_ce_f64(logits, labels)
    assert (np.abs(_loss(lossf, H * W) - ref) <= 2e-6 * np.maximum(1.0, ref)).all()
