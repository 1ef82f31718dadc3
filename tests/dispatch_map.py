"""Measured dispatch map: which kernel template instance runs each layer of a step at a given batch size.

Profile level 2 labels every launch "<kernel signature> | <layer>" with the kernel the launch helper actually launched
(tests/test_gpu_parity.py::test_profile_labels_are_the_launched_kernels).  One step of each path -- the fused z step
(generate_batch) and the two-call path (netG(..., want_image=True), then _decoder) -- gives the set of (layer, kernel)
pairs the batch runs.  The labels name template instances, not grids: a persistent launch and a one-tile launch of the
same kernel look the same here (tests/test_gpu_batch_sweep.py lists those thresholds beside SWEEP).

    python -m tests.dispatch_map [gan] [precision]

prints the batches in 1..SWEEP_MAX[gan] (tests/common.py: ffhq 64, cars 128, bedrooms 256) at which the map changes, and what changes there.
"""
import sys

import numpy as np

from tests.common import SWEEP_MAX, sweep_setup

PATHS = ("generate", "two_call")


def build(gan, precision, batch=None):
    """One ImageGenerator reserved for `batch` (default: the model's sweep maximum), eager (no hipGraph replay), and its sweep inputs
    on the device once."""
    batch = SWEEP_MAX[gan] if batch is None else batch
    import torch
    from gan_segmentation_amd.image_generator import ImageGenerator
    gcfg, gp, dcfg, dp, z, noise = sweep_setup(gan)
    gen = ImageGenerator.from_params(gcfg, gp, dcfg, dp, gpu_ids=[0], batch_size=batch, precision=precision)
    gen.graph_mode = "0"
    gen.netG._model.ensure_batch(batch)
    dev = gen.netG._model.device
    zt = torch.from_numpy(np.ascontiguousarray(z[:batch])).to(dev)
    nt = [torch.from_numpy(np.ascontiguousarray(a[:batch])).to(dev) for a in noise]
    return gen, zt, nt


def run_path(gen, path, z, noise):
    """One step of `path` on device inputs; returns the outputs (device tensors)."""
    if path == "generate":
        return gen.generate_batch(z, noise)
    rgb, feats, img = gen.netG(z, noise=noise, want_image=True)
    logits, mask = gen._decoder(*feats, want_mask=True)
    return rgb, feats, img, logits, mask


def path_map(gen, path, z, noise, batch):
    """{(layer, kernel signature)} of one step of `path` on samples 0..batch-1."""
    import torch
    ctx = gen.netG._model.ctx
    ctx.profile_enable(2)
    try:
        ctx.profile_reset()
        run_path(gen, path, z[:batch], [a[:batch] for a in noise])
        torch.cuda.synchronize()
        entries = ctx.profile_entries()
    finally:
        ctx.profile_enable(0)
    pairs = set()
    for e in entries:
        kernel, _, layer = e["name"].partition(" | ")
        pairs.add((layer, kernel))
    return frozenset(pairs)


def dispatch_map(gen, z, noise, batch):
    """The union of both paths' (layer, kernel) pairs at `batch`."""
    return frozenset().union(*(path_map(gen, p, z, noise, batch) for p in PATHS))


def breakpoints(maps):
    """maps: {batch: map} over consecutive batches -> [(batch, added, removed)] where the map differs from batch - 1's."""
    bs = sorted(maps)
    return [(b, sorted(maps[b] - maps[a]), sorted(maps[a] - maps[b])) for a, b in zip(bs, bs[1:]) if maps[a] != maps[b]]


def main(argv):
    import torch
    gan = argv[0] if len(argv) > 0 else "ffhq"
    precision = argv[1] if len(argv) > 1 else "fp32"
    gen, z, noise = build(gan, precision)
    maps = {b: dispatch_map(gen, z, noise, b) for b in range(1, SWEEP_MAX[gan] + 1)}
    bps = breakpoints(maps)
    print("%s %s: %d (layer, kernel) pairs over batches 1..%d; the map changes at %s" % (
        gan, precision, len(frozenset().union(*maps.values())), SWEEP_MAX[gan], [b for b, _, _ in bps]))
    for b, added, removed in bps:
        print("batch %d:" % b)
        for layer, kernel in added:
            print("  + %-22s %s" % (layer, kernel))
        for layer, kernel in removed:
            print("  - %-22s %s" % (layer, kernel))
    del gen
    torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
