"""DecoderTrainer and SegSolver.fit with a loss_ops.LossSpec: the raw gradients of one step against the
float64 decoder of oracle/ref_train.py followed by the float64 loss of tests/loss_ref.py and ``backward()``, and a fit that reads
its class weights from the annotation masks."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_gradients_with_every_option_match_float64_autograd():
    """The decoder of tests/test_trainer.py::test_gradients_match_autograd_directly (max_res_log2 5, lr 0) on a batch of 2 with
    gamma 2, "focal", class weights and a boundary table: the gradients within that test's tolerance (2e-3 * scale + 1e-6) of
    float64 autograd through the whole graph, the normaliser included; ``last_sums`` to 1e-6 relative."""
    import torch
    from gan_segmentation_amd import weights as W
    from gan_segmentation_amd.loss_ops import LossSpec
    from gan_segmentation_amd.trainer import DecoderTrainer
    from oracle import ref_train
    from tests import loss_ref
    from tests.test_boundary_host import rule_boundary
    mr, n = 5, 2
    gcfg = W.reduced_generator_config(mr)
    chans = W.generator_channels(gcfg)
    dcfg = W.decoder_config(mr, in_channels=chans)
    dp = W.synthetic_decoder_params(dcfg, seed=6)
    rng = np.random.default_rng(1)
    feats = [rng.standard_normal((n, c, 4 << i, 4 << i)).astype(np.float32) for i, c in enumerate(chans)]
    R = 4 << (len(chans) - 1)
    yy, xx = np.mgrid[0:R, 0:R]
    labels = np.stack([((yy - 14) ** 2 + (xx - 12) ** 2 < 81), (xx + yy > 30)]).astype(np.int64)      # regions, so that boundaries are lines
    labels[0, :3] = -1                                                                                   # an unlabelled strip
    labels[1][rng.random((R, R)) < 0.05] = -1
    spec = LossSpec(gamma=2.0, normalise="focal", class_weights=[0.5, 3.0], boundary={"weight": 4.0, "sigma": 2.0, "radius": 5})
    tr = DecoderTrainer(dcfg, dp, lr=0.0, seed=2, loss=spec)             # lr 0: parameters stay, gradients remain readable
    assert tr.last_sums is None
    masks = tr.dropout_masks([(n, dcfg["features"][i], 4 << i, 4 << i) for i in range(len(chans))])
    loss = tr.step(feats, labels, masks=masks)

    p = {k: torch.tensor(np.asarray(a, np.float32).astype(np.float64), requires_grad=not k.endswith(("running_mean", "running_var")))
         for k, a in dp.items()}
    logits, _running = ref_train.forward_train(dcfg, p, [torch.tensor(f.astype(np.float64)) for f in feats],
                                               [torch.tensor(mk.cpu().numpy()) for mk in masks])
    # the labels' u8 plane (-1 -> 255) and its boundary distance by the host rule of tests/test_boundary_host.py
    d2 = torch.from_numpy(rule_boundary(np.where(labels < 0, 255, labels).astype(np.uint8), 5).astype(np.int64)).reshape(n, -1)
    y = torch.from_numpy(labels).reshape(n, -1)
    z = logits.reshape(n, 2, -1)
    _valid, _onehot, _m, _sm, q, _py, CE, _lse, _zy, w = loss_ref._pieces(z, y, torch.tensor([0.5, 3.0], dtype=torch.float64), d2,
                                                                          torch.from_numpy(spec.table()).double())
    b = w * q ** 2.0
    Wn, B, S, T = w.sum(dim=1), b.sum(dim=1), (b * CE).sum(dim=1), ((y >= 0) & (y < 2)).double().sum(dim=1)
    per_sample = S / B
    per_sample.sum().backward()
    per_sample = per_sample.detach()
    assert abs(loss - float(per_sample.mean())) <= 2e-5 * max(1.0, float(per_sample.mean()))
    for k, t in p.items():
        if not t.requires_grad:
            continue
        gref = t.grad.numpy() if t.grad is not None else np.zeros(t.shape)
        got = tr.g[k].cpu().numpy()
        scale = max(1e-6, np.abs(gref).max())
        assert np.abs(got - gref).max() <= 2e-3 * scale + 1e-6, "%s: %.3e of %.3e" % (k, np.abs(got - gref).max(), scale)
    sums = tr.last_sums.cpu().numpy()
    want = torch.stack([Wn, B, S, T], dim=1).detach().numpy()
    assert sums.shape == (n, 4) and np.allclose(sums, want, rtol=1e-6, atol=0), (sums, want)
    assert (sums[:, 3] == want[:, 3]).all() and (sums[:, 0] > sums[:, 3] * 0.5).all()

    plain = DecoderTrainer(dcfg, dp, lr=0.0, seed=2)                     # no spec: today's path, and no sums
    plain.step(feats, labels, masks=masks)
    assert plain.loss is None and plain.last_sums is None
    assert not np.allclose(plain.g["main_block_3.0.weight"].cpu().numpy(), tr.g["main_block_3.0.weight"].cpu().numpy())


def test_trainer_refuses_what_it_cannot_run():
    from gan_segmentation_amd import weights as W
    from gan_segmentation_amd.loss_ops import LossSpec
    from gan_segmentation_amd.trainer import DecoderTrainer
    gcfg = W.reduced_generator_config(5)
    dcfg = W.decoder_config(5, in_channels=W.generator_channels(gcfg))
    dp = W.synthetic_decoder_params(dcfg, seed=6)
    for bad in (LossSpec(class_weights="median"), LossSpec(class_weights=[1.0, 2.0, 3.0]), {"gama": 1}, "focal"):
        with pytest.raises(ValueError):
            DecoderTrainer(dcfg, dp, loss=bad)
    assert DecoderTrainer(dcfg, dp, loss={"normalise": "valid"}).loss.normalise == "valid"


def test_fit_with_class_weights_from_its_masks(tmp_path, capsys):
    """fit with the checked value of TRAIN_LOSS: {class_weights: "median", normalise: "valid"} on a tiny annotation directory: the
    weights are those of loss_ops.class_weights_from_masks on the stored masks, the epoch lines carry T/B, a checkpoint is written."""
    from PIL import Image
    from gan_segmentation_amd import annotation_io, loss_ops, main as cli, weights as W
    from gan_segmentation_amd.seg_solver import SegSolver
    mr = 5
    gcfg = W.reduced_generator_config(mr)
    chans = W.generator_channels(gcfg)
    rng = np.random.default_rng(3)
    R = 4 << (len(chans) - 1)
    data = tmp_path / "data"
    yy, xx = np.mgrid[0:R, 0:R]
    stored = []
    for i in range(3):
        feats = [rng.standard_normal((c, 4 << l, 4 << l)).astype(np.float32) for l, c in enumerate(chans)]
        inside = (yy - R / 2 - i) ** 2 + (xx - R / 2 + i) ** 2 < (R / 4.5) ** 2          # a small disc: the class is a minority
        feats[-1][0] = np.where(inside, 1.5, -1.5) + 0.3 * feats[-1][0]
        annotation_io.export_sample(str(data), i, np.zeros((R, R, 3), np.uint8), feats)
        m = np.where(inside, 230, 128).astype(np.uint8)
        m[:2] = 20                                                                          # a strip of ignored pixels
        Image.fromarray(m, "L").save(str(data / ("mask_%06d.png" % i)))
        stored.append(annotation_io.preprocess_mask(m))
    want = loss_ops.class_weights_from_masks(stored, 2, "median")
    assert want[1] > want[0] > 0
    solver = SegSolver(mr, str(data), str(tmp_path / "checkpoints"), gpu_ids=[0], keep_weights=False, in_channels=chans)
    lines = []
    history = solver.fit(epochs=2, log=lines.append, loss=cli.check_train_loss({"class_weights": "median", "normalise": "valid"}))
    assert len(history) == 2 and all(np.isfinite(history))
    assert lines[0] == "loss class weights: %s" % ", ".join("%.6f" % w for w in want)
    epochs = [l for l in lines if l.startswith("Epoch[")]
    assert len(epochs) == 2 and all("Train-total-loss=" in l and " T/B=" in l for l in epochs)
    assert float(epochs[0].split("T/B=")[1]) == pytest.approx(np.mean([(m >= 0).sum() / sum(want[c] * (m == c).sum() for c in (0, 1))
                                                                        for m in stored]), rel=1e-5)
    assert solver.is_trained and (tmp_path / "checkpoints" / "checkpoint_last.params").exists()
    plain = solver.fit(epochs=1, log=lines.append)                      # no spec: the reference's line and nothing else
    assert len(plain) == 1 and lines[-1].startswith("Epoch[1] Train-total-loss=") and "T/B" not in lines[-1]
