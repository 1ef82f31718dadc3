"""``python -m gan_segmentation_amd.main [generate|train|evaluate]`` -- the actions of reference main.py:44-104
with the same ``config.yml`` keys (reference config.yml.example:1-8); `generate` is the hot path, `train` and
`evaluate` drive ``SegSolver.fit`` / ``SegSolver.evaluate``.  The Tk `annotation` GUI
is out of scope.

Writes ``img_%06d.jpg`` (RGB image; the reference flips to BGR only because cv2 expects it)
and ``mask_%06d.png`` (single channel, class index) into BASE_DIR/dataset/train_generated, at R/f px with the additive
key ``OUTPUT_DOWNSCALE: f`` (1, 2, 4 or 8; default 1).  The additive key ``OUTPUT_SIZE`` (an int or ``[h, w]``, every side a
multiple of 16, at most R/f and at least 1/16 of it; absent by default: off) then shrinks every pair on the GPU to that size
(``resize_ops.resize_pair``: the image's exact area mean, the mask by the additive key ``OUTPUT_MASK_RESIZE``, "vote" -- the default, the
class that covers most of the pixel; values 8..254 come out as 255 -- or "nearest"), after every mask filter below and before the files,
``PAIR_STATS`` and the previews, which are then those of the resized pair.  The additive key ``MASK_MORPH: true`` (default false) cleans every mask on
the GPU with the 5x5 close + open of reference utils.morph_mask before it is written (``mask_ops.morph_mask``).  The additive keys
``MASK_MIN_AREA: k`` (default 0: off), ``MASK_CONNECTIVITY`` (4 or 8, default 8) and ``MASK_FILL`` ("neighbour", the default, or
0..255) replace every connected component of fewer than k pixels, after the morphology (``mask_ops.despeckle``).  The additive keys
``MASK_IGNORE_BAND: r`` (0..32 px, default 0: off) and ``MASK_IGNORE_LABEL`` (0..255, default 255) then write the label into every
pixel within r pixels of a pixel of another class, on both sides of every class boundary (``mask_ops.ignore_band``): the stored
``mask_*.png`` holds 255 there, the value the reference's dataset readers map to -1.  The additive keys ``MASK_REFINE: k`` (0..8 passes, default 0: off),
``MASK_REFINE_RADIUS`` (1..5, default 3), ``MASK_REFINE_SIGMA_SPACE`` (default 2.0) and ``MASK_REFINE_SIGMA_COLOUR`` (default 32.0, in
summed absolute channel differences) run an image-guided vote on every mask BEFORE all of the above (``mask_ops.refine``): a pixel
takes the class that its neighbours of similar colour in the pair's own image agree on.  The additive key
``PAIR_STATS: true`` (default false) adds one ``pair_stats_<first>_<last + 1>.npz`` per rank with the per-sample statistics of the
written pairs (``pair_stats.pair_stats``); ``python -m gan_segmentation_amd.pair_stats DIR`` merges them into a report.
The additive key ``PREVIEW_EVERY: k`` (integer >= 0, default 0: off) also writes ``vis_%06d.jpg`` for every sample whose global
index is a multiple of k: the mask of the pair as written (after downscale, morphology, area filter and ignore band) laid over its
image in ``preview.DATASET_COLOURS`` at alpha 0.5 with solid class outlines (``preview.overlay``), box-filtered by the additive key
``PREVIEW_DOWNSCALE: f`` (1, 2, 4, 8 or 16; default 1).  Which of them exist depends on the index only, not on the batch size or
the number of ranks.  Previews are diagnostics, not part of the dataset contract: they are not byte-specified as files (PIL encodes
them, at quality 95), and they are not withheld by the device check that withholds a bad batch's pair files.
``python -m gan_segmentation_amd.preview DIR`` makes contact sheets of a written dataset from its files.
`evaluate` takes the additive key ``EVAL_MASK_CHAINS`` (a mapping: chain name -> mapping of ``mask_ops.apply_filters`` keywords such as
``morph: true`` or ``ignore_band: 2``, empty for the raw mask; absent by default: the reference's one line and nothing else) and prints
one more line per chain: accuracy, mean-iou, band-accuracy, boundary-iou, abstained and changed of the decoder's mask passed through
that chain, against the annotations under BASE_DIR/eval (``SegSolver.evaluate_masks``); the additive key ``EVAL_BAND`` (0..32 px,
default 2) is the radius of the boundary band the two boundary figures are taken in.  The additive key ``EVAL_SCORES: true`` (default
false) prints one more line after those: mean-auc, mean-ap, the reference's 100*(1-mean-auc) and 100*(1-mean-ap), and per class the best
margin threshold with its IoU, the IoU at margin 0 and the share of clamped pixels, read from the histograms of the decoder's logit
margins (``SegSolver.evaluate_scores``, csrc/gsa_scores.h); the additive key ``EVAL_SCORE_SHIFT`` (0..8, default 5) gives them 2^shift bins
per logit unit.
`train` takes the additive key ``TRAIN_LOSS`` (a mapping with keys among ``gamma``: 0 or 1..8, the focal exponent; ``normalise``:
"mean", "valid" or "focal"; ``class_weights``: a list of one number per class, or "median" / "inverse", computed from the annotation
masks under BASE_DIR/data; ``boundary``: a mapping with ``weight``, ``sigma`` and ``radius``, 1..32 px; ``region``: a mapping with
``weight`` and optionally ``alpha``, ``beta``, ``smooth`` and ``classes``, such as ``{weight: 1.0, alpha: 0.3, beta: 0.7}``, which adds
weight times the soft Tversky (Dice, Jaccard) loss of csrc/gsa_region.h; absent by default: the
reference's loss and nothing else) and trains the decoder with the loss of ``loss_ops`` (csrc/gsa_loss.h), the epoch lines then
carrying the mean T/B as well, and with a region term the mean index of every class.
With torchrun (one process per GPU) the sample indices are sharded across ranks and every rank
writes its own files -- no collective is needed when the sink is the filesystem.
"""
import argparse
import os
import sys

import numpy as np
import yaml


def load_config_file(path):
    with open(path) as f:
        return yaml.safe_load(f)   # reference utils.py:112-115


def devices_for_rank(cfg, world, local_rank):
    """(GAN device list, solver device list) of this process.  One process (the reference's way, main.py:79-88):
    the whole ``GAN_GPU_IDS`` / ``SOLVER_GPU_IDS`` lists, batch split over them in-process.  Under torchrun (one
    process per GPU): rank r drives ``GAN_GPU_IDS[r % len]`` alone (an empty list = device ``local_rank``)."""
    gan_ids = list(cfg.get("GAN_GPU_IDS") or [])
    solver_ids = list(cfg.get("SOLVER_GPU_IDS") or gan_ids)
    if world > 1:
        gpu = gan_ids[local_rank % len(gan_ids)] if gan_ids else local_rank
        return [gpu], [gpu]
    if not gan_ids:
        raise RuntimeError("GAN_GPU_IDS is empty: the MI355X path has no CPU context (reference image_generator.py:17)")
    return gan_ids, solver_ids[:1] if solver_ids else gan_ids[:1]


def shard_batches(n_generate, batch, world, rank):
    """(first global sample index, samples) of every batch THIS rank produces: rank r owns the contiguous slice
    ``dist.shard_bounds(n_generate, world, r)`` of the file indices and walks it in batches, the last one short
    (reference main.py:93-99 with image_generator.py:88-92).  The slices of all ranks partition [0, n_generate)."""
    from .dist import shard_bounds
    lo, hi = shard_bounds(n_generate, world, rank)
    index = lo
    while index < hi:
        bs = min(batch, hi - index)
        yield index, bs
        index += bs


def generate(cfg, limit=None, workers=None):
    import torch
    from . import dist as gdist
    from .dataset_writer import DatasetWriter, DeviceCheckFailed
    from .image_generator import ImageGenerator
    from .pair_stats import check_pair_stats
    from .preview import check_preview_downscale, check_preview_every, write_previews
    from .resize_ops import check_output_mask_resize, check_output_size, resize_pair
    from .seg_solver import SegSolver
    from .weights import GAN_MAX_RES_LOG2

    # ranks never exchange anything here (every rank writes its own files), so no process group is created:
    # RANK / WORLD_SIZE / LOCAL_RANK alone decide the shard
    rank, world, local_rank = gdist.env_ranks()
    root_dir, gan, gan_dir = cfg["BASE_DIR"], cfg["GAN"], cfg["GAN_DIR"]
    gan_ids, solver_ids = devices_for_rank(cfg, world, local_rank)
    n_generate = cfg.get("GENERATE_NUM", 10000) if limit is None else limit
    batch = cfg["GAN_BATCH_SIZE_PER_GPU"] * len(gan_ids)      # reference main.py:87
    seed = int(cfg.get("SEED", 0))             # additive key: seed of the counter-based latents/noise
    precision = cfg.get("PRECISION", "fp32")   # additive key: "bf16" = bf16 MFMA operands (BASELINE config 5)
    truncation_psi = cfg.get("TRUNCATION_PSI")                # additive key: replaces the weight file's truncation vector
    style_mix_prob = float(cfg.get("STYLE_MIX_PROB", 0.0))    # additive key: share of style-mixed samples (style_mix.py)
    # additive key: write the pairs at R/f (box-filtered image, block-summed logits' argmax); checked before any model is loaded
    downscale = ImageGenerator.check_output_downscale(cfg.get("OUTPUT_DOWNSCALE", 1), GAN_MAX_RES_LOG2[gan])
    mask_morph = ImageGenerator.check_mask_morph(cfg.get("MASK_MORPH", False))    # additive key, checked here as well
    # additive keys, checked here as well: the component filter (off by default)
    mask_min_area = ImageGenerator.check_mask_min_area(cfg.get("MASK_MIN_AREA", 0))
    mask_connectivity = ImageGenerator.check_mask_connectivity(cfg.get("MASK_CONNECTIVITY", 8))
    mask_fill = ImageGenerator.check_mask_fill(cfg.get("MASK_FILL", "neighbour"))
    # additive keys, checked here as well: the ignore band around class boundaries (off by default), applied last
    mask_ignore_band = ImageGenerator.check_mask_ignore_band(cfg.get("MASK_IGNORE_BAND", 0))
    mask_ignore_label = ImageGenerator.check_mask_ignore_label(cfg.get("MASK_IGNORE_LABEL", 255))
    # additive keys, checked here as well: the image-guided refinement of the mask (off by default), applied first
    mask_refine = ImageGenerator.check_mask_refine(cfg.get("MASK_REFINE", 0))
    mask_refine_radius = ImageGenerator.check_mask_refine_radius(cfg.get("MASK_REFINE_RADIUS", 3))
    mask_refine_sigma_space = ImageGenerator.check_mask_refine_sigma_space(cfg.get("MASK_REFINE_SIGMA_SPACE", 2.0))
    mask_refine_sigma_colour = ImageGenerator.check_mask_refine_sigma_colour(cfg.get("MASK_REFINE_SIGMA_COLOUR", 32.0))
    # additive keys, checked here as well: the pair resized to any smaller size behind the filters (off by default)
    output_size = check_output_size(cfg.get("OUTPUT_SIZE"), 2 ** GAN_MAX_RES_LOG2[gan] // downscale)
    output_mask_resize = check_output_mask_resize(cfg.get("OUTPUT_MASK_RESIZE", "vote"))
    stats = check_pair_stats(cfg.get("PAIR_STATS", False))    # additive key, checked here as well: every rank writes its own shard file
    # additive keys, checked here as well: vis_%06d.jpg for the samples whose index is a multiple of k (off by default)
    preview_every = check_preview_every(cfg.get("PREVIEW_EVERY", 0))
    preview_downscale = check_preview_downscale(cfg.get("PREVIEW_DOWNSCALE", 1))

    solver = SegSolver(GAN_MAX_RES_LOG2[gan], os.path.join(root_dir, "data"), os.path.join(root_dir, "checkpoints"),
                       gpu_ids=solver_ids, keep_weights=False, precision=precision)
    if not solver.is_trained:
        print("train Decoder first!")   # reference main.py:82-84
        return -1
    netG = ImageGenerator(gpu_ids=gan_ids, gan_dir=gan_dir, gan=gan, batch_size=batch, precision=precision,
                          truncation_psi=truncation_psi, style_mix_prob=style_mix_prob, output_downscale=downscale,
                          mask_morph=mask_morph, mask_min_area=mask_min_area, mask_connectivity=mask_connectivity, mask_fill=mask_fill,
                          mask_refine=mask_refine, mask_refine_radius=mask_refine_radius, mask_refine_sigma_space=mask_refine_sigma_space,
                          mask_refine_sigma_colour=mask_refine_sigma_colour,
                          mask_ignore_band=mask_ignore_band, mask_ignore_label=mask_ignore_label)
    netG.attach_decoder(solver.cfg, solver.net)
    dst_dir = os.path.join(root_dir, "dataset", "train_generated")
    os.makedirs(dst_dir, exist_ok=True)

    # the writer copies each batch out through pinned buffers and encodes it on a thread pool while the
    # GPU already computes the next one
    # additive keys JPEG_ON_GPU / PNG_ON_GPU (default on): the files are compressed by the HIP kernels behind
    # include/gsa_jpeg.h and include/gsa_png.h; the host threads only frame and write them
    on_gpu = bool(cfg.get("JPEG_ON_GPU", True))
    try:
        with DatasetWriter(dst_dir, workers=workers, gpu_jpeg=on_gpu, gpu_png=bool(cfg.get("PNG_ON_GPU", on_gpu)),
                           stats=stats) as writer:
            for index, bs in shard_batches(n_generate, batch, world, rank):
                # latents and noise keyed on the global sample index: the files are the same for any number of ranks
                img, mask = netG.generate_indexed(index, bs, seed=seed)
                if output_size is not None:
                    img, mask = resize_pair(img, mask, output_size, output_mask_resize)
                # the device-side checks travel with the batch: 8 bytes copied behind its kernels, read by the writer before it
                # releases the batch's files -- a run of 10 000 samples stops at the first bad batch instead of reporting at close()
                writer.submit(img, mask, index, status=netG.snapshot_status())
                if preview_every:       # a diagnostic beside the writer, not through its ring: overlay on the device, PIL on this thread
                    write_previews(dst_dir, img, mask, index, preview_every, preview_downscale)
    except DeviceCheckFailed as e:
        print("generate: %s" % e, file=sys.stderr)
        return -2
    torch.cuda.synchronize()
    return 0


def export_for_annotation(cfg, count):
    """Headless stand-in for the sampling half of the annotator (reference seg_annotator.py:286-337): generate `count`
    samples and save what the GUI saves next to a drawn mask -- BASE_DIR/data/img_%06d.jpg and feat_%06d.pickle.  When a decoder
    checkpoint exists, also vis_img_%06d.jpg, the reference's name and content (seg_annotator.py:330-346): the current decoder's
    prediction over the image, ``preview.REFERENCE_COLOURS`` at alpha 0.5, background skipped, no outline."""
    import torch
    from . import annotation_io, preview
    from .image_generator import ImageGenerator
    gpu = list(cfg["GAN_GPU_IDS"])[0]
    netG = ImageGenerator(gpu_ids=[gpu], gan_dir=cfg["GAN_DIR"], gan=cfg["GAN"], batch_size=cfg["GAN_BATCH_SIZE_PER_GPU"],
                          precision=cfg.get("PRECISION", "fp32"), seed=int(cfg.get("SEED", 0)),
                          truncation_psi=cfg.get("TRUNCATION_PSI"))     # annotation samples are never style-mixed
    dst = os.path.join(cfg["BASE_DIR"], "data")
    ckpt = os.path.join(cfg["BASE_DIR"], "checkpoints")
    trained = os.path.isdir(ckpt) and any(os.path.splitext(f)[1] == ".params" for f in os.listdir(ckpt))     # SegSolver.load's test
    solver = _solver(cfg, keep_weights=True) if trained else None       # without a checkpoint no decoder is created
    lut = preview.make_lut(preview.REFERENCE_COLOURS, alpha=0.5, skip_background=True)
    for i, (img, feats) in enumerate(netG.get_images(count)):
        annotation_io.export_sample(dst, i, img, feats)
        if trained:                 # the reference's create_image_iterator / next_image: predict from the features, draw, save
            mask = solver.predict(feats, keep_on_device=True)[..., 0].to(torch.uint8).contiguous()
            vis = preview.overlay(torch.from_numpy(np.ascontiguousarray(img)).to(mask.device)[None], mask, lut)
            preview.save_jpeg(os.path.join(dst, "vis_img_%06d.jpg" % i), vis[0].cpu().numpy())
    print("wrote %d samples (img + feat%s) to %s" % (count, " + vis_img" if trained else "", dst))
    return 0


def _solver(cfg, keep_weights=False):
    from .seg_solver import SegSolver
    from .weights import GAN_MAX_RES_LOG2
    root_dir, gan = cfg["BASE_DIR"], cfg["GAN"]
    gpu_ids = list(cfg.get("SOLVER_GPU_IDS", cfg.get("GAN_GPU_IDS", [0])))[:1]
    return SegSolver(GAN_MAX_RES_LOG2[gan], os.path.join(root_dir, "data"), os.path.join(root_dir, "checkpoints"),
                     gpu_ids=gpu_ids, keep_weights=keep_weights, precision=cfg.get("PRECISION", "fp32"))


def check_train_loss(v):
    """The TRAIN_LOSS key: None (absent: the reference's loss), or a mapping with keys among gamma (0 or 1..8), normalise ("mean",
    "valid" or "focal"), class_weights (a list of numbers, "median" or "inverse"), boundary (a mapping with weight, sigma and
    radius) and region (a mapping with weight and, optionally, alpha, beta, smooth and classes: ``loss_ops.check_region``)
    -> None or a ``loss_ops.LossSpec``.  ValueError otherwise, the message naming the key."""
    from . import loss_ops
    if v is None:
        return None
    return loss_ops.LossSpec.from_mapping(v, "TRAIN_LOSS")


def train(cfg, epochs=None):
    """The `train` action (reference main.py:54-60): fit the decoder on BASE_DIR/data, save the checkpoint.  With the additive key
    ``TRAIN_LOSS`` the loss of ``loss_ops`` replaces the reference's (``SegSolver.fit(loss=...)``)."""
    loss = check_train_loss(cfg.get("TRAIN_LOSS"))      # additive key, checked before any model is loaded
    solver = _solver(cfg, keep_weights=False)
    history = solver.fit(epochs=epochs, log=print, loss=loss)
    print("final loss: %.6f" % history[-1])
    return 0


def check_eval_mask_chains(v):
    """The EVAL_MASK_CHAINS key: None (absent), or a non-empty mapping of a name to a mapping of ``mask_ops.apply_filters`` keywords
    (None for none: the raw mask) -> None or {name: complete keyword dict}.  ValueError otherwise."""
    from . import mask_ops
    if v is None:
        return None
    if not isinstance(v, dict) or not v:
        raise ValueError("EVAL_MASK_CHAINS must be a mapping: chain name -> mapping of apply_filters keywords, got %r" % (v,))
    chains = {}
    for name, kw in v.items():
        kw = {} if kw is None else kw
        if not isinstance(name, str) or not isinstance(kw, dict) or not all(isinstance(k, str) for k in kw):
            raise ValueError("EVAL_MASK_CHAINS: chain %r must be a mapping of apply_filters keywords, got %r" % (name, kw))
        chains[name] = mask_ops.check_filters("EVAL_MASK_CHAINS: chain %r" % (name,), **kw)
    return chains


def check_eval_band(v):
    """The EVAL_BAND key: the radius of the boundary band of the chain report as an int, 0 .. 32 px (ValueError otherwise)."""
    from . import mask_ops
    return mask_ops.check_band(v, "EVAL_BAND")


def check_eval_scores(v):
    """The EVAL_SCORES key: a bool (ValueError otherwise)."""
    if not isinstance(v, bool):
        raise ValueError("EVAL_SCORES must be true or false, got %r" % (v,))
    return v


def check_eval_score_shift(v):
    """The EVAL_SCORE_SHIFT key: 2^shift bins per logit unit in the score histograms, an int 0 .. 8 (ValueError otherwise)."""
    from . import score_ops
    return score_ops.check_shift(v, "EVAL_SCORE_SHIFT")


def evaluate(cfg):
    """The `evaluate` action (reference main.py:61-73) over BASE_DIR/eval.  With the additive key ``EVAL_MASK_CHAINS`` one more line
    per chain: the decoder's mask through that filter chain against the annotations (``SegSolver.evaluate_masks``).  With the
    additive key ``EVAL_SCORES`` one more line: the figures of ``metrics.ScoreCurves`` (``SegSolver.evaluate_scores``)."""
    # additive keys, checked before any model is loaded
    chains = check_eval_mask_chains(cfg.get("EVAL_MASK_CHAINS"))
    band = check_eval_band(cfg.get("EVAL_BAND", 2))
    scores = check_eval_scores(cfg.get("EVAL_SCORES", False))
    score_shift = check_eval_score_shift(cfg.get("EVAL_SCORE_SHIFT", 5))
    solver = _solver(cfg)
    if not solver.is_trained:
        print("train Decoder first!")
        return -1
    eval_dir = os.path.join(cfg["BASE_DIR"], "eval")
    result = solver.evaluate(eval_dir)
    print(", ".join("%s: %.4f" % (name, value) for name, value in result))
    if chains is not None:
        for chain, values in solver.evaluate_masks(eval_dir, chains, band=band).items():
            print("%s: %s" % (chain, ", ".join("%s: %.4f" % (name, value) for name, value in values)))
    if scores:
        curves = solver.evaluate_scores(eval_dir, shift=score_shift)
        print("scores: %s" % ", ".join("%s: %.4f" % (name, value) for name, value in curves.get_name_value()))
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("action", nargs="?", choices=("annotation", "train", "evaluate", "generate"), default="generate")
    ap.add_argument("--config", default="config.yml")
    ap.add_argument("--limit", type=int, default=None, help="override GENERATE_NUM")
    ap.add_argument("--workers", type=int, default=None, help="encoder threads (default: the CPU share of the process)")
    ap.add_argument("--epochs", type=int, default=None, help="train: override the reference's 24 epochs")
    ap.add_argument("--count", type=int, default=None, help="annotation: number of samples to generate and export")
    args = ap.parse_args(argv)
    np.random.seed(0)
    cfg = load_config_file(args.config)
    if args.action == "annotation":
        if args.count is None:
            print("the Tk annotation GUI is out of scope (SURVEY.md section 8); `annotation --count N` writes the img/feat "
                  "files the GUI saves for N generated samples (masks are then drawn with any image editor)")
            return 2
        return export_for_annotation(cfg, args.count)
    if args.action == "train":
        return train(cfg, args.epochs)
    if args.action == "evaluate":
        return evaluate(cfg)
    return generate(cfg, args.limit, args.workers)


if __name__ == "__main__":
    sys.exit(main())
