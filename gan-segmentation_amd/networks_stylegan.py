"""``Generator`` with the call surface of reference networks_stylegan.py:76-197, executed by
the HIP library.

    netG = Generator(config)                       # reference networks_stylegan.py:78-112
    netG.load_parameters(path, ignore_extra=True)  # reference image_generator.py:21-22
    rgb, features = netG(z)                        # reference networks_stylegan.py:165-197

``rgb`` is (N,3,R,R) fp32 and ``features`` the list of (N,C_r,R_r,R_r) fp32 block outputs,
as torch tensors on the GPU (the analogue of the reference's device NDArrays).

The W space, StyleGAN's standard controls: ``w = netG.mapping(z)`` is the untruncated mapping output (N,512) and
``netG.synthesis(dlatents)`` runs the same network from per-layer latents (N, L, 512), L = 2*(max_res_log2-1) in the order
of ``truncation_psi`` and of the noise planes (level lv uses layers 2lv and 2lv+1).  ``load_parameters(...,
truncation_psi=v)`` replaces the file's truncation vector (a float or L floats) before the weights are committed.

Differences from the reference, all additive: the AddNoise planes, which the reference
draws from MXNet's global RNG inside the network (networks_stylegan.py:297-300), can be
passed explicitly (``noise=[...]``) so that results are reproducible; without them they are
drawn on the device from ``torch.Generator``.
"""
import numpy as np
import torch

from . import params as _params
from . import weights as _weights
from ._runtime import DeviceModel, current_stream_ptr, to_device_f32


class Generator:
    def __init__(self, config, device=0, precision="fp32", model=None, **kwargs):
        self.config = dict(config)
        for key in ("fmap_base", "fmap_decay", "fmap_max", "base_scale_x", "base_scale_y", "use_wscale",
                    "fix_noise", "channels", "latent_size", "max_res_log2"):
            if key not in self.config:
                raise KeyError("Generator config is missing %r" % key)  # reference :81-91
        self.fix_noise = bool(self.config["fix_noise"])
        self.nc = self.config["channels"]
        self.latent_size = self.config["latent_size"]
        self.max_res_log2 = self.config["max_res_log2"]
        self.precision = precision
        # its own context: a second Generator on the same GPU must not touch this one's weights or configuration
        self._model = model if model is not None else DeviceModel(device, precision)
        if self._model.generator_cfg is not None:
            raise RuntimeError("this context already holds a Generator")
        self._model.ctx.generator_init(self.config)
        self._model.generator_cfg = self.config
        self._model.invalidate_workspace()
        self._loaded = False
        self._fixed_noise = None
        self._rng = torch.Generator(device=self._model.device)
        self._rng.manual_seed(0)

    # -- parameters -----------------------------------------------------------------------
    def num_features(self, res_log2):
        return _weights.num_features(self.config, res_log2)

    def load_parameters(self, source, ignore_extra=True, ctx=None, allow_missing=False, truncation_psi=None):
        """``source``: a ``.params`` path or a ``{name: ndarray}`` dict (either naming scheme).  ``truncation_psi``: None keeps the
        file's vector; a float or a sequence of ``num_style_layers`` floats replaces it (``weights.with_truncation_psi``)."""
        if allow_missing:
            raise NotImplementedError("allow_missing is not supported (the reference does not use it)")
        tensors = _params.load_params(source) if isinstance(source, (str, bytes)) else dict(source)
        tensors = _weights.complete_generator_params(self.config, tensors, ignore_extra=ignore_extra)
        tensors = _weights.with_truncation_psi(tensors, truncation_psi, self.num_style_layers)
        self._model.ctx.generator_load(tensors)
        self._model.invalidate_workspace()
        self._loaded = True

    @property
    def num_style_layers(self):
        return _weights.num_style_layers(self.config)

    def seed(self, seed):
        self._rng.manual_seed(int(seed))

    # -- forward --------------------------------------------------------------------------
    def noise_shapes(self, batch):
        return [(batch, 1, 2 ** r, 2 ** r) for r in range(2, self.max_res_log2 + 1) for _ in range(2)]

    def draw_noise(self, batch):
        dev = self._model.device
        if self.fix_noise and self._fixed_noise is not None and self._fixed_noise[0].shape[0] == batch:
            return self._fixed_noise
        noise = [torch.randn(s, device=dev, dtype=torch.float32, generator=self._rng) for s in self.noise_shapes(batch)]
        if self.fix_noise:
            self._fixed_noise = noise
        return noise

    def draw_indexed(self, first_index, n, seed=0):
        """(z (n,latent), [noise planes]) on the device as a pure function of (seed, global sample index): sample
        ``first_index + k`` gets the same bytes whatever batch, rank or GPU count asks for it (``gsa_fill_inputs``,
        Philox4x32-10 + Box-Muller)."""
        if not self._loaded:
            raise RuntimeError("Generator parameters are not loaded")
        dev = self._model.device
        z = torch.empty((n, self.latent_size), device=dev, dtype=torch.float32)
        noise = [torch.empty(s, device=dev, dtype=torch.float32) for s in self.noise_shapes(n)]
        self._model.ctx.fill_inputs(current_stream_ptr(dev), n, seed, first_index, z.data_ptr(), [a.data_ptr() for a in noise])
        return z, noise

    def draw_indexed_latents(self, first_index, n, seed=0):
        """z (n, latent) alone, as ``draw_indexed`` draws it for (seed, global sample index)."""
        if not self._loaded:
            raise RuntimeError("Generator parameters are not loaded")
        z = torch.empty((n, self.latent_size), device=self._model.device, dtype=torch.float32)
        self._model.ctx.fill_inputs(current_stream_ptr(self._model.device), n, seed, first_index, z.data_ptr(), None)
        return z

    def _prepare_noise(self, noise, n):
        if noise is None:
            return self.draw_noise(n)
        noise = [to_device_f32(a, self._model.device) for a in noise]
        shapes = self.noise_shapes(n)
        if len(noise) != len(shapes) or any(tuple(a.shape) != s for a, s in zip(noise, shapes)):
            raise ValueError("noise must be %d planes shaped (N,1,R,R), R=4,4,8,8,..." % len(shapes))
        return noise

    def _prepare_w(self, dlatents, noise):
        if not self._loaded:
            raise RuntimeError("Generator parameters are not loaded")
        dl = to_device_f32(dlatents, self._model.device)
        if dl.dim() != 3 or dl.shape[1] != self.num_style_layers or dl.shape[2] != self.latent_size:
            raise ValueError("dlatents must have shape (N, %d, %d)" % (self.num_style_layers, self.latent_size))
        n = dl.shape[0]
        noise = self._prepare_noise(noise, n)
        self._model.ensure_batch(n)
        return dl, noise, n

    def _prepare(self, z, noise):
        if not self._loaded:
            raise RuntimeError("Generator parameters are not loaded")
        dev = self._model.device
        z = to_device_f32(z, dev)
        if z.dim() != 2 or z.shape[1] != self.latent_size:
            raise ValueError("z must have shape (N, %d)" % self.latent_size)
        n = z.shape[0]
        noise = self._prepare_noise(noise, n)
        self._model.ensure_batch(n)
        return z, noise, n

    def _outputs(self, n, want_features, want_image):
        dev = self._model.device
        R = 2 ** self.max_res_log2
        rgb = torch.empty((n, self.nc, R, R), device=dev, dtype=torch.float32)
        img = torch.empty((n, R, R, self.nc), device=dev, dtype=torch.uint8) if want_image else None
        feats = None
        if want_features:
            chans = _weights.generator_channels(self.config)
            feats = [torch.empty((n, c, 4 << i, 4 << i), device=dev, dtype=torch.float32) for i, c in enumerate(chans)]
        return rgb, img, feats

    def mapping(self, z):
        """The mapping network alone (reference networks_stylegan.py:128-139): z (N, latent) -> w (N, latent), untruncated."""
        if not self._loaded:
            raise RuntimeError("Generator parameters are not loaded")
        dev = self._model.device
        z = to_device_f32(z, dev)
        if z.dim() != 2 or z.shape[1] != self.latent_size:
            raise ValueError("z must have shape (N, %d)" % self.latent_size)
        n = z.shape[0]
        self._model.ensure_batch(n)
        w = torch.empty((n, self.latent_size), device=dev, dtype=torch.float32)
        self._model.ctx.mapping_forward(current_stream_ptr(dev), n, z.data_ptr(), w.data_ptr())
        return w

    def synthesis(self, dlatents, noise=None, want_features=True, want_image=False):
        """The network from per-layer latents ``dlatents`` (N, L, latent), untruncated (the committed ``truncation_psi`` is
        applied per layer); returns what ``__call__`` returns.  ``dlatents[:, l] = mapping(z)`` for every l gives ``self(z)``
        bit for bit."""
        dl, noise, n = self._prepare_w(dlatents, noise)
        dev = self._model.device
        rgb, img, feats = self._outputs(n, want_features, want_image)
        self._model.ctx.generator_forward_w(
            current_stream_ptr(dev), n, dl.data_ptr(), self.num_style_layers, [a.data_ptr() for a in noise], rgb.data_ptr(),
            img.data_ptr() if img is not None else None, [f.data_ptr() for f in feats] if feats else None)
        if want_image:
            return rgb, feats, img
        return rgb, feats

    def __call__(self, z, noise=None, want_features=True, want_image=False):
        z, noise, n = self._prepare(z, noise)
        dev = self._model.device
        rgb, img, feats = self._outputs(n, want_features, want_image)
        self._model.ctx.generator_forward(
            current_stream_ptr(dev), n, z.data_ptr(), [a.data_ptr() for a in noise], rgb.data_ptr(),
            img.data_ptr() if img is not None else None, [f.data_ptr() for f in feats] if feats else None)
        if want_image:
            return rgb, feats, img
        return rgb, feats

    forward = __call__


# The north-star wording calls the synthesis part "SynthesisNetwork"; the reference has one class.
SynthesisNetwork = Generator
