"""``ImageGenerator`` with the call surface of reference image_generator.py:6-124.

    netG = ImageGenerator(gpu_ids, gan_dir, gan='ffhq', batch_size=4, return_latents=False)
    for img, feats in netG.get_images(n): ...       # img (R,R,3) u8 RGB, feats [C,R_r,R_r] fp32

Host-visible behaviour follows the reference: batches of ``batch_size`` latents, the last one
short (``:88-92``), per-sample yield of ``(img, feats[, latent_z_np])`` where ``latent_z_np`` is
the WHOLE batch array (``:105,122``).  Additions: explicit latents/noise for reproducibility,
``keep_on_device`` to skip the 132.8 MB/sample host round trip of the reference
(``:103-114``), and ``generate_batch`` -- the fused generator+decoder step used by
``main.py generate`` -- which never materialises the features.

The two StyleGAN sampling controls: ``truncation_psi`` replaces the weight file's truncation vector (a float or
2*(max_res_log2-1) floats); ``style_mix_prob > 0`` makes ``generate_indexed`` mix the styles of two latents per sample by the
shard-invariant plan of ``style_mix``, through the per-layer (W-space) step ``gsa_generate_w``.  ``generate_batch_w`` runs that
step on caller-made dlatents.  The W path runs eager: it is never captured into a hipGraph.  With the defaults every call runs
the z path exactly as before.

``output_downscale`` (1, 2, 4 or 8; fixed at construction) makes every fused call -- ``generate_batch``, ``generate_batch_w``,
``generate_indexed``, style-mixed or not -- return the pair at R/f through ``gsa_generate_downscaled``: the image is the mean of
toRGB's fp32 values over each f x f block before the uint8 truncation, the mask the argmax of the block-summed logits (the rule of
include/gsa.h and DESIGN.md section 11).  ``get_images`` and everything that feeds the annotator or the decoder stay full size.

``training_batches`` is the consumer side without files: an iterator of augmented, normalised NCHW batches with their labels, made
on the GPU from ``generate_indexed`` pairs by the plan and the kernel of ``augment``.

``mask_morph=True`` (fixed at construction, off by default) cleans the mask of every fused call -- the same calls as above, and
therefore ``training_batches`` -- with ``mask_ops.morph_mask``, the 5x5 close + open of reference utils.morph_mask (DESIGN.md
section 14): the mask returned is the rule applied to what the same call returns without the option, the image is untouched.

``mask_min_area=k`` (fixed at construction; 0, the default, and 1 are off) passes the mask of every fused call through
``mask_ops.despeckle``: every connected component of fewer than k pixels (``mask_connectivity`` 4 or 8) takes the value of its
neighbour or the constant ``mask_fill`` (the rule of include/gsa_components.h) -- after ``mask_morph``
when both are on, and before anything reads the mask.  The labels and areas it works in are kept per replica, batch size and
stream: 8 bytes per mask pixel, 256 MiB for ffhq at batch 32.  The image is untouched.

``mask_ignore_band=r`` (fixed at construction; 0, the default, is off; up to 32) writes ``mask_ignore_label`` (255, the value the
consumers ignore: ``labels="int64"`` of the training stream maps it to -1, the pair statistics count it in slot 8) into the mask of
every fused call wherever a pixel of another value lies within r pixels -- ``mask_ops.ignore_band``, the rule of
include/gsa_boundary.h, DESIGN.md section 18: a band on both sides of every class boundary, at the output resolution, applied
LAST, after ``mask_morph`` and the component filter, and before anything reads the mask.  The image is untouched.

``mask_refine=k`` (fixed at construction; 0, the default, is off; up to 8) runs k passes of ``mask_ops.refine`` on the mask of every
fused call: a joint bilateral vote that moves the class boundaries onto the edges of the pair's own image (the rule of
csrc/gsa_refine.h), with the weights of ``mask_refine_radius`` (3), ``mask_refine_sigma_space`` (2.0) and
``mask_refine_sigma_colour`` (32.0) and the attached decoder's class count -- FIRST, on the pair as written (after
``output_downscale``), before ``mask_morph``, the component filter and the band.  The image is read, never written.
"""
import os

import numpy as np
import torch

from . import augment as _augment
from . import jpeg as _jpeg
from . import mask_ops as _mask_ops
from . import photometric as _photometric
from . import style_mix as _style_mix
from . import weights as _weights
from ._runtime import current_stream_ptr, is_device_tensor, split_sizes, to_device_f32
from .dataset_writer import STATUS_RING_DEPTH
from .networks_seg import Decoder
from .networks_stylegan import Generator


_GRAPH_CAPTURES_MAX = 16


class ImageGenerator:
    style_mix_prob = 0.0
    output_downscale = 1
    mask_morph = False
    mask_min_area = 0
    mask_connectivity = 8
    mask_fill = "neighbour"
    mask_refine = 0
    mask_refine_radius = 3
    mask_refine_sigma_space = 2.0
    mask_refine_sigma_colour = 32.0
    mask_ignore_band = 0
    mask_ignore_label = 255

    def __init__(self, gpu_ids, gan_dir, gan="ffhq", batch_size=4, return_latents=False, seed=0, precision="fp32",
                 truncation_psi=None, style_mix_prob=0.0, output_downscale=1, mask_morph=False, mask_min_area=0, mask_connectivity=8,
                 mask_fill="neighbour", mask_refine=0, mask_refine_radius=3, mask_refine_sigma_space=2.0, mask_refine_sigma_colour=32.0,
                 mask_ignore_band=0, mask_ignore_label=255):
        cfg = self._get_config(max_res_log2=_weights.GAN_MAX_RES_LOG2[gan])
        self._setup(cfg, os.path.join(gan_dir, "stylegan-%s.params" % gan), gpu_ids, batch_size, return_latents, seed, precision,
                    truncation_psi, style_mix_prob, output_downscale, mask_morph, mask_min_area, mask_connectivity, mask_fill,
                    mask_refine, mask_refine_radius, mask_refine_sigma_space, mask_refine_sigma_colour, mask_ignore_band, mask_ignore_label)

    @classmethod
    def from_params(cls, gcfg, gparams, dcfg=None, dparams=None, gpu_ids=(0,), batch_size=4,
                    return_latents=False, seed=0, precision="fp32", truncation_psi=None, style_mix_prob=0.0, output_downscale=1,
                    mask_morph=False, mask_min_area=0, mask_connectivity=8, mask_fill="neighbour", mask_refine=0, mask_refine_radius=3,
                    mask_refine_sigma_space=2.0, mask_refine_sigma_colour=32.0, mask_ignore_band=0, mask_ignore_label=255):
        """Build from in-memory weights (tests, benchmarks: no pretrained files exist here)."""
        self = cls.__new__(cls)
        self._setup(dict(gcfg), gparams, gpu_ids, batch_size, return_latents, seed, precision, truncation_psi, style_mix_prob,
                    output_downscale, mask_morph, mask_min_area, mask_connectivity, mask_fill,
                    mask_refine, mask_refine_radius, mask_refine_sigma_space, mask_refine_sigma_colour, mask_ignore_band, mask_ignore_label)
        if dcfg is not None:
            self.attach_decoder(dcfg, dparams)
        return self

    def _setup(self, cfg, gparams, gpu_ids, batch_size, return_latents, seed, precision, truncation_psi, style_mix_prob,
               output_downscale, mask_morph, mask_min_area=0, mask_connectivity=8, mask_fill="neighbour", mask_refine=0,
               mask_refine_radius=3, mask_refine_sigma_space=2.0, mask_refine_sigma_colour=32.0, mask_ignore_band=0, mask_ignore_label=255):
        """What both constructors do: the options, checked before any file or device is touched; one generator replica per gpu
        id, loaded from ``gparams`` (a ``.params`` path, read once, or a ``{name: array}`` dict); the seeds."""
        self.cfg = cfg
        self.max_res_log2 = cfg["max_res_log2"]
        self.output_downscale = self.check_output_downscale(output_downscale, self.max_res_log2)
        self.mask_morph = self.check_mask_morph(mask_morph)
        self.mask_min_area = self.check_mask_min_area(mask_min_area)
        self.mask_connectivity = self.check_mask_connectivity(mask_connectivity)
        self.mask_fill = self.check_mask_fill(mask_fill)
        self.mask_refine = self.check_mask_refine(mask_refine)
        self.mask_refine_radius = self.check_mask_refine_radius(mask_refine_radius)
        self.mask_refine_sigma_space = self.check_mask_refine_sigma_space(mask_refine_sigma_space)
        self.mask_refine_sigma_colour = self.check_mask_refine_sigma_colour(mask_refine_sigma_colour)
        self.mask_ignore_band = self.check_mask_ignore_band(mask_ignore_band)
        self.mask_ignore_label = self.check_mask_ignore_label(mask_ignore_label)
        self.latent_size = cfg["latent_size"]
        self.return_latents = return_latents
        self.batch_size = batch_size
        self.ctx = list(gpu_ids)      # the reference's device list (image_generator.py:17): one weight replica per entry
        if len(self.ctx) == 0:
            raise RuntimeError("the MI355X path has no CPU context: pass at least one gpu id "
                               "(the reference falls back to mx.cpu(), image_generator.py:17)")
        self.precision = precision
        self.style_mix_prob = self._check_mix_prob(style_mix_prob)
        if isinstance(gparams, (str, bytes)):
            from . import params as _params
            gparams = _params.load_params(gparams)
        self._gens = []
        for dev in self.ctx:
            g = self._get_G(self.cfg, dev)
            g.load_parameters(gparams, ignore_extra=True, truncation_psi=truncation_psi)
            self._gens.append(g)
        self.netG = self._gens[0]
        self._decoder = None
        self._decoders = []
        self._rng = torch.Generator(device="cpu")
        self._rng.manual_seed(seed)
        for g in self._gens:
            g.seed(seed)

    @staticmethod
    def _check_mix_prob(p):
        p = float(p)
        if not 0.0 <= p <= 1.0:
            raise ValueError("style_mix_prob must be in [0, 1], got %r" % p)
        return p

    @staticmethod
    def check_output_downscale(f, max_res_log2):
        """The output downscale factor f as an int: 1, 2, 4 or 8, a real downscale (f > 1) leaving at least 16 px of the
        2**max_res_log2 output (ValueError otherwise).  Factor 1 asks for nothing: a generator of 4 or 8 px, which the library accepts
        without a decoder, passes."""
        if isinstance(f, bool) or not isinstance(f, (int, np.integer)) or int(f) not in (1, 2, 4, 8):
            raise ValueError("output_downscale must be 1, 2, 4 or 8, got %r" % (f,))
        f = int(f)
        if f > 1 and (2 ** max_res_log2) // f < 16:
            raise ValueError("output_downscale %d leaves %d px of the %d px output (at least 16 needed)"
                             % (f, (2 ** max_res_log2) // f, 2 ** max_res_log2))
        return f

    @staticmethod
    def check_mask_morph(v):
        """The mask clean-up switch: a real bool (ValueError otherwise -- 1, "yes" or None are not an answer)."""
        if not isinstance(v, bool):
            raise ValueError("mask_morph must be True or False, got %r" % (v,))
        return v

    @staticmethod
    def check_mask_min_area(v):
        """The area threshold of the component filter as an int: 0 .. 2^31 - 1 pixels, 0 and 1 meaning off (ValueError otherwise)."""
        return _mask_ops.check_min_area(v, "mask_min_area")

    @staticmethod
    def check_mask_connectivity(v):
        """The component filter's connectivity as an int: 4 or 8 (ValueError otherwise)."""
        return _mask_ops.check_connectivity(v, "mask_connectivity")

    @staticmethod
    def check_mask_fill(v):
        """What the component filter writes into a small component: "neighbour" or an int 0..255 (ValueError otherwise)."""
        return "neighbour" if _mask_ops.check_fill(v, "mask_fill") == _mask_ops.FILL_NEIGHBOUR else int(v)

    @staticmethod
    def check_mask_refine(v):
        """The number of refinement passes as an int: 0 .. 8, 0 meaning off (ValueError otherwise)."""
        return _mask_ops.check_refine_iterations(v, "mask_refine")

    @staticmethod
    def check_mask_refine_radius(v):
        """The window radius of the refinement as an int: 1 .. 5 (ValueError otherwise)."""
        return _mask_ops.check_refine_radius(v, "mask_refine_radius")

    @staticmethod
    def check_mask_refine_sigma_space(v):
        """The spatial width of the refinement's weights in pixels as a float > 0 (ValueError otherwise)."""
        return _mask_ops.check_refine_sigma(v, "mask_refine_sigma_space")

    @staticmethod
    def check_mask_refine_sigma_colour(v):
        """The colour width of the refinement's weights, in summed absolute channel differences, as a float > 0 (ValueError otherwise)."""
        return _mask_ops.check_refine_sigma(v, "mask_refine_sigma_colour")

    @staticmethod
    def check_mask_ignore_band(v):
        """The radius of the ignore band as an int: 0 .. 32 pixels, 0 meaning off (ValueError otherwise)."""
        return _mask_ops.check_band(v, "mask_ignore_band")

    @staticmethod
    def check_mask_ignore_label(v):
        """The value the ignore band writes as an int: 0 .. 255 (ValueError otherwise)."""
        return _mask_ops.check_label(v, "mask_ignore_label")

    def _get_G(self, config, device):
        return Generator(config, device=device, precision=self.precision)

    def _get_config(self, max_res_log2=9):
        return _weights.generator_config(max_res_log2)  # reference image_generator.py:46-74

    def attach_decoder(self, dcfg, dparams):
        """Load a decoder into the context of every generator replica so that ``generate_batch`` can run the fused
        path (the features never leave the kernels' layout).  ``dparams``: a ``{name: array}`` dict, a ``.params``
        path, or a loaded ``Decoder`` (e.g. ``SegSolver.net``) whose weights are copied -- that object stays
        independent, as two gluon blocks would."""
        if isinstance(dparams, Decoder):
            if dparams._tensors is None:
                raise RuntimeError("the decoder to attach has no parameters loaded")
            dcfg, dparams = dparams.cfg, dparams._tensors
        self._decoders = []
        for g in self._gens:
            if g._model.decoder_cfg is not None:        # re-attach: a fresh decoder slot in the same context
                g._model.decoder_cfg = None
            dec = Decoder(dcfg, len(self._gens), model=g._model)
            dec.load_parameters(dparams)
            self._decoders.append(dec)
        self._decoder = self._decoders[0]
        return self._decoder

    @staticmethod
    def _transform_gan_back(img, cfg):
        """numpy restatement of reference image_generator.py:76-84 (kept for callers that hold
        fp32 rgb; the device path produces the same bytes in toRGB's epilogue)."""
        lo, hi = cfg["imrange"]
        img = np.transpose(img, (0, 2, 3, 1))
        img = (img - np.float32(lo)) / np.float32(hi - lo)
        img = np.clip(img, 0.0, 1.0)
        return (np.float32(255.0) * img).astype(np.uint8)

    def draw_latents(self, n):
        return torch.randn((n, self.latent_size), generator=self._rng, dtype=torch.float32)

    # -- reference surface ------------------------------------------------------------------
    def get_images(self, n, latents=None, noise=None, keep_on_device=False):
        n_batches = n // self.batch_size + (1 if n % self.batch_size > 0 else 0)
        n_generated = 0
        for _ in range(n_batches):
            bs = min(self.batch_size, n - n_generated)
            if latents is not None:
                latent_z = torch.as_tensor(np.asarray(latents[n_generated:n_generated + bs], dtype=np.float32))
            else:
                latent_z = self.draw_latents(bs)
            nz = None
            if noise is not None:
                nz = [a[n_generated:n_generated + bs] for a in noise]
            # data-parallel split over the device list, host-side gather (reference :95-114); the launches of all
            # devices are enqueued before the first result is awaited
            parts = []
            for r, lo, hi in split_sizes(bs, len(self._gens)):
                g = self._gens[r]
                with torch.cuda.device(g._model.device):
                    parts.append(g(latent_z[lo:hi], noise=None if nz is None else [a[lo:hi] for a in nz], want_image=True))
            latent_z_np = latent_z.numpy()
            if not keep_on_device:
                for g in self._gens:
                    torch.cuda.synchronize(g._model.device)
                imgs = np.concatenate([p[2].cpu().numpy() for p in parts], axis=0)
                feats = [np.concatenate([p[1][i].cpu().numpy() for p in parts], axis=0) for i in range(len(parts[0][1]))]
            else:
                dev0 = self._gens[0]._model.device
                imgs = torch.cat([p[2].to(dev0) for p in parts], dim=0) if len(parts) > 1 else parts[0][2]
                feats = ([torch.cat([p[1][i].to(dev0) for p in parts], dim=0) for i in range(len(parts[0][1]))]
                         if len(parts) > 1 else parts[0][1])
            n_generated += bs
            for i in range(bs):
                img = imgs[i]
                fs = [f[i] for f in feats]
                if self.return_latents:
                    yield img, fs, latent_z_np
                else:
                    yield img, fs

    # -- fused hot path ---------------------------------------------------------------------
    def generate_indexed(self, first_index, n, seed=0, out=None):
        """``generate_batch`` for the global samples ``first_index .. first_index+n-1`` with counter-based latents
        and noise (``Generator.draw_indexed``): the dataset does not depend on how it is sharded.  With ``style_mix_prob > 0``
        the samples are style-mixed by the plan of ``style_mix`` (also a function of the global index) on the eager W path."""
        if self.style_mix_prob > 0:
            return self._generate_indexed_mixed(first_index, n, seed, out)
        if len(self._gens) == 1:
            z, noise = self.netG.draw_indexed(first_index, n, seed)
            return self.generate_batch(z, noise, out=out)
        parts = []
        for r, lo, hi in split_sizes(n, len(self._gens)):
            g = self._gens[r]
            with torch.cuda.device(g._model.device):
                z, noise = g.draw_indexed(first_index + lo, hi - lo, seed)
                parts.append(self._generate_on(r, z, noise))
        return self._collect(parts, n, out)

    def training_batches(self, batch, crop=480, mode="train", seed=0, first_index=0, num_samples=None, rank=0, world=1,
                         mean=_augment.IMAGENET_MEAN, std=_augment.IMAGENET_STD, dtype=torch.float32, labels="uint8",
                         ignore_label=_augment.IGNORE_LABEL, jpeg_quality=None, photometric=None, **limits):
        """The training stream: an iterator of ``(image (n, C, crop, crop) dtype, label (n, crop, crop), first_index)``.

        Batch k of the global sequence holds the samples ``first_index + k*batch ..`` and goes to the rank with ``k % world == rank``
        (``augment.stream_batches``); ``num_samples=None`` streams without end, otherwise the last batch is short.  Every batch is
        ``generate_indexed`` of its indices (so precision, truncation, style mixing, ``output_downscale`` and several gpu ids work
        as there), warped by ``augment.plan_matrices(seed, index, ...)`` (``mode``: "train" or "center"; ``limits``: flip, rotate,
        scale, shift; ``crop=None`` keeps the pair's size) and normalised with ``mean`` / ``std`` by one kernel on the same stream.
        ``dtype``: torch.float32 or torch.bfloat16.  ``labels="uint8"`` keeps ``ignore_label`` (255) outside the image;
        ``labels="int64"`` maps it to -1 as the reference's loader does.  The yielded tensors are new every batch and ordered on
        the caller's current stream: the consumer may keep them.  ``jpeg_quality=q`` (an int in 1..100; 95 is what ``main.py generate``
        stores) passes every image through ``jpeg.roundtrip`` in front of the warp: the stream then carries exactly the pixels a
        reader of the dataset's quality-q JPEG files would decode (three channels and a pair size that is a multiple of 16 wanted;
        the mask is untouched, PNG is lossless).  ``None``, the default, leaves the image as generated.  ``photometric`` changes the
        pixels' values between the round trip and the warp (``photometric.photometric``: contrast, brightness, channel shift, a
        Gaussian blur, noise; the warp's border stays black and the mask is untouched): ``True`` takes the default limits, a dict
        gives limits (``photometric.DEFAULT_LIMITS`` names them), ``None``, the default, leaves the values alone.  Its plan is a
        function of ``(seed, index)`` like the warp's.  Arguments are checked here, before any GPU work."""
        if self._decoder is None:
            raise RuntimeError("attach_decoder() first")
        crop, mode = _augment.check_crop(crop), _augment.check_mode(mode)
        if labels not in ("uint8", "int64"):
            raise ValueError("labels must be \"uint8\" or \"int64\", got %r" % (labels,))
        if dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("dtype must be torch.float32 or torch.bfloat16, got %r" % (dtype,))
        if not 0 <= int(ignore_label) <= 255:
            raise ValueError("ignore_label must be in 0..255, got %r" % (ignore_label,))
        R, nc = 2 ** self.max_res_log2 // self.output_downscale, self.netG.nc
        out_size = _augment.check_shapes(R, R, nc, _augment.output_size(R, R, crop))
        scale, bias = _augment.normalisation(mean, std)
        if len(scale) != nc:
            raise ValueError("mean and std need one value per image channel (%d), got %d" % (nc, len(scale)))
        _augment.plan_matrices(seed, first_index, 0, R, R, crop, mode, **limits)        # the limits' own checks
        if jpeg_quality is not None:
            jpeg_quality = _jpeg.check_quality(jpeg_quality, "jpeg_quality")
            _jpeg.check_roundtrip_shape(R, R, nc)
        photometric = _photometric.check_keyword(photometric)
        if photometric is not None:
            _photometric.check_shape(R, R, nc)
        batches = _augment.stream_batches(first_index, batch, num_samples, rank, world)
        return self._training_batches(batches, seed, R, crop, mode, limits, out_size, scale, bias, dtype, labels, int(ignore_label),
                                      jpeg_quality, photometric)

    def _training_batches(self, batches, seed, R, crop, mode, limits, out_size, scale, bias, dtype, labels, ignore_label,
                          jpeg_quality=None, photometric=None):
        dev0 = self._gens[0]._model.device
        for first, n in batches:
            img, mask = self.generate_indexed(first, n, seed=seed)
            if jpeg_quality is not None:
                with torch.cuda.device(dev0):
                    img = _jpeg.roundtrip(img, jpeg_quality)
            if photometric is not None:
                rows = _photometric.photometric_plan(seed, first, n, **photometric)
                with torch.cuda.device(dev0):
                    img = _photometric.photometric(img, rows, seed, first)
            matrices = _augment.plan_matrices(seed, first, n, R, R, crop, mode, **limits)
            with torch.cuda.device(dev0):
                image, label = _augment.augment_pairs(img, mask, matrices, out_size, scale=scale, bias=bias, dtype=dtype,
                                                      ignore_label=ignore_label)
                if labels == "int64":
                    label = label.to(torch.int64)
                    label[label == ignore_label] = -1
            yield image, label, first

    def _generate_indexed_mixed(self, first_index, n, seed, out):
        if self._decoder is None:
            raise RuntimeError("attach_decoder() first")
        parts = []
        for r, lo, hi in split_sizes(n, len(self._gens)):
            g = self._gens[r]
            with torch.cuda.device(g._model.device):
                dl, noise = self._mixed_dlatents(g, first_index + lo, hi - lo, seed)
                parts.append(self._generate_on_w(r, dl, noise, out if len(self._gens) == 1 else None))
        if len(self._gens) == 1:
            return parts[0]
        return self._collect(parts, n, out)

    def _mixed_dlatents(self, g, first_index, n, seed):
        """(dlatents (n, L, latent), noise) of the global samples first_index.. on replica ``g``: layer l of a sample is
        mapping(z) or, mixed and l >= cutoff, mapping(z_b) (``style_mix``); mapping runs once per latent set of n rows."""
        z, noise = g.draw_indexed(first_index, n, seed)
        z_b = g.draw_indexed_latents(first_index, n, _style_mix.mix_seed(seed))
        L = g.num_style_layers
        mix, cutoff = _style_mix.mix_plan(seed, first_index, n, self.style_mix_prob, L)
        sel = torch.from_numpy(_style_mix.layer_select(mix, cutoff, L)).to(g._model.device)
        w_a, w_b = g.mapping(z), g.mapping(z_b)
        return torch.where(sel[:, :, None], w_b[:, None, :], w_a[:, None, :]).contiguous(), noise

    def _check_out(self, out, n, dev):
        R, nc = 2 ** self.max_res_log2 // self.output_downscale, self.netG.nc
        img, mask = out
        for t, shape in ((img, (n, R, R, nc)), (mask, (n, R, R))):
            if not is_device_tensor(t, torch.uint8, shape=shape, device=dev):
                raise ValueError("out tensors must be contiguous uint8 %s on %s" % (shape, dev))
        return img, mask

    def _pair_buffers(self, r, n, out):
        """(img, raw mask, final mask) of a fused step of ``n`` samples on replica ``r``: new tensors, or the checked ``out``; the
        step writes the raw mask, ``_finish_mask`` turns it into the final one (the same tensor without ``mask_refine``,
        ``mask_morph``, ``mask_min_area`` and ``mask_ignore_band``)."""
        g = self._gens[r]
        dev = g._model.device
        if out is None:
            R = 2 ** self.max_res_log2 // self.output_downscale
            img = torch.empty((n, R, R, g.nc), device=dev, dtype=torch.uint8)
            mask = torch.empty((n, R, R), device=dev, dtype=torch.uint8)
        else:
            img, mask = self._check_out(out, n, dev)
        return img, self._raw_mask(r, mask), mask

    def _generate_on(self, r, z, noise, out=None):
        """The fused step on replica ``r`` (its own device and stream)."""
        g = self._gens[r]
        z, noise, n = g._prepare(z, noise)
        img, raw, final = self._pair_buffers(r, n, out)
        self._run_step(g._model, g._model.device, n, z, [a.data_ptr() for a in noise], img, raw)
        return img, self._finish_mask(r, raw, final, img)

    def _raw_mask(self, r, mask):
        """Where the step of replica ``r`` writes its mask: ``mask`` itself, or with ``mask_refine``, ``mask_morph``, ``mask_min_area``
        or ``mask_ignore_band`` a scratch tensor kept per replica, batch size and stream (calls on one stream are ordered, so they may
        share it) -- the same address every call, so a captured graph that bakes it in stays valid whatever ``mask`` is."""
        if not self.mask_refine and not self.mask_morph and self.mask_min_area <= 1 and not self.mask_ignore_band:
            return mask
        return self._mask_scratch("raw", r, mask, torch.uint8)

    def _mask_scratch(self, what, r, mask, dtype):
        """The scratch tensor ``what`` of ``mask``'s shape: kept per replica, batch size and stream."""
        cache = self.__dict__.setdefault("_raw_masks", {})
        key = (what, r, mask.shape[0], torch.cuda.current_stream(mask.device).cuda_stream)
        t = cache.get(key)
        if t is None:
            t = cache[key] = torch.empty(mask.shape, dtype=dtype, device=mask.device)
        return t

    def _refine_classes(self):
        """K of the refinement: the class count of the attached decoder, its last feature count (2..8; ValueError otherwise)."""
        return _mask_ops.check_refine_classes(int(self._decoder.cfg["features"][-1]), "the attached decoder's class count")

    def _finish_mask(self, r, raw, final, img):
        """The mask a fused call of replica ``r`` returns: the raw one passed through the ``mask_refine`` passes of the image-guided
        vote against ``img``, the pair's image as written, then through ``mask_morph``, then through the component filter of
        ``mask_min_area`` and last through the ignore band of ``mask_ignore_band``, whichever are on --
        eager launches behind the step on the same stream (never part of a captured graph), before anything reads the mask.  The
        filter's labels and areas (int32 each: 8 bytes per pixel, 256 MiB for ffhq at batch 32) and the masks between two stages
        are scratch of the same kind as the raw mask."""
        if raw is final:
            return final
        filtered, banded = self.mask_min_area > 1, self.mask_ignore_band > 0

        def target(what, last):
            # a stage writes the final mask if it is the last one that is on, a scratch tensor of its own otherwise
            return final if last else self._mask_scratch(what, r, final, torch.uint8)
        if self.mask_refine:
            raw = _mask_ops.refine(img, raw, self.mask_refine, self.mask_refine_radius, self._refine_classes(),
                                   sigma_space=self.mask_refine_sigma_space, sigma_colour=self.mask_refine_sigma_colour,
                                   out=target("refined", not self.mask_morph and not filtered and not banded),
                                   scratch=self._mask_scratch("refining", r, final, torch.uint8) if self.mask_refine > 1 else None)
        if self.mask_morph:
            raw = _mask_ops.morph_mask(raw, out=target("morphed", not filtered and not banded))
        if filtered:
            scratch = (self._mask_scratch("labels", r, final, torch.int32), self._mask_scratch("areas", r, final, torch.int32))
            raw = _mask_ops.despeckle(raw, self.mask_min_area, self.mask_connectivity, self.mask_fill, out=target("filtered", not banded),
                                      scratch=scratch)
        if banded:
            _mask_ops.ignore_band(raw, self.mask_ignore_band, self.mask_ignore_label, out=final)
        return final

    def _run_step(self, model, dev, n, z, nptrs, img, mask):
        """The z step into ``img`` / ``mask``: eager, or replayed from a hipGraph."""
        if self._graph_wanted(model, n):
            # A small step is a latency chain of ~100 launches of 10-60 us: when the very same call comes again (same batch,
            # same input and output addresses -- a steady loop over preallocated or recycled tensors) often enough it is replayed
            # from a captured hipGraph (+2-3 % at batch <= 2 and in bf16 mode; nothing at batch 8, where it stays eager).  The key holds
            # every pointer the graph bakes in, so a replay always reads the current inputs and writes the current outputs; the
            # epoch changes whenever the context's workspace, weights or stream structure change AND whenever a call of the
            # context failed (a failed pass leaves statistic rows the next EAGER pass re-zeroes -- a replay would not).
            key = (n, z.data_ptr(), tuple(nptrs), img.data_ptr(), mask.data_ptr(), torch.cuda.current_stream(dev).cuda_stream,
                   model.ctx.graph_epoch, self.output_downscale)
            cache = model.__dict__.setdefault("_graphs", {})
            hit = cache.get(key)
            if hit is not None:
                hit.replay()
                return
            seen = model.__dict__.setdefault("_graph_seen", {})
            seen[key] = seen.get(key, 0) + 1
            # Capturing costs about as much as a few steps: a call is captured only after it has come `graph_after` (32) times
            # -- a steady loop (main.py generate: thousands of steps), never a one-off call -- and a model captures at most
            # `_GRAPH_CAPTURES_MAX` times in its life (a caller whose addresses keep changing stays eager instead of re-capturing)
            if (seen[key] >= self.graph_after and model.ctx._checked_first_step
                    and model.__dict__.get("_graph_captures", 0) < _GRAPH_CAPTURES_MAX):
                if len(cache) >= 8:
                    cache.pop(next(iter(cache)))
                if len(seen) > 64:
                    seen.clear()
                graph = self._capture(model, dev, n, z, nptrs, img, mask, self.output_downscale)
                model.__dict__["_graph_captures"] = model.__dict__.get("_graph_captures", 0) + 1      # only a capture that succeeded counts
                graph.replay()
                cache[key] = graph
                return
        self._step(model.ctx, current_stream_ptr(dev), n, z, nptrs, img, mask, self.output_downscale)

    @staticmethod
    def _step(ctx, stream, n, z, nptrs, img, mask, factor, dlatents=None, num_layers=0):
        """One fused step from ``z`` or (``z`` None) from per-layer ``dlatents``: gsa_generate / gsa_generate_w, or
        gsa_generate_downscaled when the pair is written at 1/factor resolution.  The one place that chooses the entry."""
        zp = None if z is None else z.data_ptr()
        dp = None if dlatents is None else dlatents.data_ptr()
        if factor != 1:
            ctx.generate_downscaled(stream, n, zp, dp, num_layers, nptrs, factor, img.data_ptr(), mask.data_ptr())
        elif dlatents is None:
            ctx.generate(stream, n, zp, nptrs, img.data_ptr(), mask.data_ptr())
        else:
            ctx.generate_w(stream, n, dp, num_layers, nptrs, img.data_ptr(), mask.data_ptr())

    def _generate_on_w(self, r, dlatents, noise, out=None):
        """The fused step from per-layer dlatents on replica ``r`` (gsa_generate_w); always eager."""
        g = self._gens[r]
        dl, noise, n = g._prepare_w(dlatents, noise)
        img, raw, final = self._pair_buffers(r, n, out)
        self._step(g._model.ctx, current_stream_ptr(g._model.device), n, None, [a.data_ptr() for a in noise], img, raw,
                   self.output_downscale, dl, g.num_style_layers)
        return img, self._finish_mask(r, raw, final, img)

    @staticmethod
    def _capture(model, dev, n, z, nptrs, img, mask, factor=1):
        """Capture one fused step into a hipGraph on a capture stream of our own: ``CUDAGraph.capture_begin/capture_end``
        directly -- not the ``torch.cuda.graph`` context manager, whose device-wide synchronize, ``gc.collect`` and
        ``empty_cache()`` would stall the caller's steady loop and could move its recycled tensors to new addresses."""
        cur = torch.cuda.current_stream(dev)
        side = model.__dict__.get("_capture_stream")
        if side is None:
            side = model.__dict__["_capture_stream"] = torch.cuda.Stream(device=dev)
        graph = torch.cuda.CUDAGraph()
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            graph.capture_begin(capture_error_mode="thread_local")
            try:
                ImageGenerator._step(model.ctx, side.cuda_stream, n, z, nptrs, img, mask, factor)
            except BaseException:
                # the step failed while it was being recorded: end the (now invalid) capture, but let the ORIGINAL error through --
                # capture_end raises on an invalidated capture and would hide it
                try:
                    graph.capture_end()
                except Exception:
                    pass
                cur.wait_stream(side)
                raise
            graph.capture_end()
        cur.wait_stream(side)
        return graph

    def _graph_wanted(self, model, n):
        """hipGraph replay of the fused step: mode "0" never, "1" always, default = where it measured faster (bf16 mode, fp32
        batches of at most 2); never while per-launch profiling events are on.  ``self.graph_mode`` / ``self.graph_after``
        override the environment's GSA_GRAPH / GSA_GRAPH_AFTER."""
        mode = self.graph_mode if self.graph_mode is not None else os.environ.get("GSA_GRAPH", "")
        if mode == "0" or model.ctx.profiling or len(self._gens) != 1:
            return False
        return mode == "1" or self.precision == "bf16" or n <= 2

    graph_mode = None       # None: GSA_GRAPH decides; "0" / "1"

    @property
    def graph_after(self):
        v = self.__dict__.get("_graph_after")
        return v if v is not None else int(os.environ.get("GSA_GRAPH_AFTER", "32"))

    @graph_after.setter
    def graph_after(self, v):
        self.__dict__["_graph_after"] = v

    def graphs_captured(self):
        """Number of hipGraphs the replicas hold (bench.py reports whether its timed loop replayed one)."""
        return sum(len(g._model.__dict__.get("_graphs", {})) for g in self._gens)

    def snapshot_status(self):
        """In-flight form of the device-side checks (include/gsa.h gsa_status_snapshot): enqueues, behind the kernels of the
        batch just submitted on every replica's current stream, an 8-byte copy of the context's two sticky words into a pinned
        host slot and returns those slots ([2] int32 tensors, one per replica) WITHOUT synchronising.  The reader -- the
        ``DatasetWriter`` dispatcher, before it releases that batch's files -- looks at them once an event recorded behind this
        call has completed; non-zero = that batch (or an earlier one since the last clean look) must be discarded."""
        ring = self.__dict__.get("_status_ring")
        if ring is None:
            ring = self.__dict__["_status_ring"] = [torch.zeros((STATUS_RING_DEPTH, 2), dtype=torch.int32).pin_memory() for _ in self._gens]
            self.__dict__["_status_next"] = 0
        k = self.__dict__["_status_next"]
        self.__dict__["_status_next"] = (k + 1) % STATUS_RING_DEPTH
        views = []
        dev0 = self._gens[0]._model.device
        for g, slots in zip(self._gens, ring):
            dev = g._model.device
            view = slots[k]
            with torch.cuda.device(dev):
                g._model.ctx.status_snapshot(current_stream_ptr(dev), view.data_ptr())
                if dev != dev0:
                    # the reader synchronises with the FIRST device's stream (where the collected pairs live): make that stream
                    # wait for this replica's copy too, or the slot could be read before it has landed
                    ev = torch.cuda.Event()
                    ev.record(torch.cuda.current_stream(dev))
                    torch.cuda.current_stream(dev0).wait_event(ev)
            views.append(view)
        return views

    def _collect(self, parts, n, out):
        """Per-device results -> one (img, mask) pair on the first device, in sample order."""
        dev0 = self._gens[0]._model.device
        img = torch.cat([p[0].to(dev0, non_blocking=True) for p in parts], dim=0)
        mask = torch.cat([p[1].to(dev0, non_blocking=True) for p in parts], dim=0)
        if out is not None:
            oi, om = self._check_out(out, n, dev0)
            oi.copy_(img)
            om.copy_(mask)
            return oi, om
        return img, mask

    def _generate_split(self, on, x, noise, out):
        """``on`` (``_generate_on`` or ``_generate_on_w``) of the batch ``x``: on the one replica, or split over the replicas like
        the reference's ``split_and_load`` and collected on the first device."""
        if self._decoder is None:
            raise RuntimeError("attach_decoder() first")
        if len(self._gens) == 1:
            return on(0, x, noise, out)
        n = len(x)
        parts = []
        for r, lo, hi in split_sizes(n, len(self._gens)):
            with torch.cuda.device(self._gens[r]._model.device):
                parts.append(on(r, x[lo:hi], None if noise is None else [a[lo:hi] for a in noise]))
        return self._collect(parts, n, out)

    def generate_batch(self, z, noise=None, out=None):
        """latents (N,512) [+ noise planes] -> (img (N,R,R,3) u8, mask (N,R,R) u8) on the GPU (R/f with output_downscale f).
        The per-batch body of ``main.py generate`` (reference main.py:97-99) in one call.
        ``out=(img, mask)``: write into these contiguous uint8 device tensors instead of new ones
        (e.g. the fused send buffer of ``dist.PairGatherer``).  With several gpu ids the batch is split over the
        replicas like the reference's ``split_and_load`` and the pairs are collected on the first device."""
        return self._generate_split(self._generate_on, z, noise, out)

    def generate_batch_w(self, dlatents, noise=None, out=None):
        """``generate_batch`` from per-layer latents: dlatents (N, L, 512), untruncated (the loaded ``truncation_psi`` is
        applied per layer), L = 2*(max_res_log2-1).  Split over the replicas like ``generate_batch``; eager (no hipGraph)."""
        return self._generate_split(self._generate_on_w, dlatents, noise, out)
