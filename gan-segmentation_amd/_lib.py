"""ctypes binding of the C ABI declared in the headers under include/: one signature table, bound in one place.

``load_library()`` opens the HIP library built in-tree by ``__graft_entry__.build()``
(csrc/libgsa_hip.so).  There is no CPU fallback: if the library is missing or a call
fails, a ``GsaError`` is raised.  (The CPU oracle has a ctypes table of its own in
oracle/binding.py; this module never opens it.)
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
HIP_LIBRARY = os.path.join(_HERE, "csrc", "libgsa_hip.so")
EXPERIMENTS_LIBRARY = os.path.join(_HERE, "csrc", "libgsa_hip_exp.so")      # `make experiments`: + the measured-slower kernels behind their switches
if os.environ.get("GSA_HIP_LIBRARY"):      # tests / A-B runs: another build of the same library (a file name inside csrc/, or a path)
    _alt = os.environ["GSA_HIP_LIBRARY"]
    HIP_LIBRARY = _alt if os.path.isabs(_alt) else os.path.join(_HERE, "csrc", _alt)

class GsaError(RuntimeError):
    pass


PRECISIONS = {"fp32": 0, "bf16": 1}     # gsa_precision


class GeneratorConfig(ctypes.Structure):
    _fields_ = [("max_res_log2", ctypes.c_int32), ("fmap_base", ctypes.c_int32),
                ("fmap_decay", ctypes.c_double), ("fmap_max", ctypes.c_int32),
                ("latent_size", ctypes.c_int32), ("channels", ctypes.c_int32),
                ("use_wscale", ctypes.c_int32)]


class DecoderConfig(ctypes.Structure):
    _fields_ = [("num_feats", ctypes.c_int32), ("start_res", ctypes.c_int32),
                ("use_bn", ctypes.c_int32), ("features", ctypes.POINTER(ctypes.c_int32)),
                ("in_channels", ctypes.POINTER(ctypes.c_int32))]


_c = ctypes
_vp, _i32, _i64, _u64, _f32, _int = _c.c_void_p, _c.c_int32, _c.c_int64, _c.c_uint64, _c.c_float, _c.c_int
_vpp = _c.POINTER(_vp)
_bn = [_vp, _i32, _i32, _i32]       # stream, n, C, HW: the head of every batch-norm entry

# Every function the headers under include/ declare: header -> {name: (result type, argument types)}.  The ONE place a C signature
# is restated in Python; tests/test_abi_and_host.py checks it against the headers' text, kind by kind.
SIGNATURES = {
    "gsa.h": {
        "gsa_create": (_int, [_int, _vpp]),
        "gsa_destroy": (None, [_vp]),
        "gsa_last_error": (_c.c_char_p, [_vp]),
        "gsa_generator_init": (_int, [_vp, _c.POINTER(GeneratorConfig)]),
        "gsa_generator_set_param": (_int, [_vp, _c.c_char_p, _vp, _i32, _c.POINTER(_i64)]),
        "gsa_generator_commit": (_int, [_vp]),
        "gsa_decoder_init": (_int, [_vp, _c.POINTER(DecoderConfig)]),
        "gsa_decoder_set_param": (_int, [_vp, _c.c_char_p, _vp, _i32, _c.POINTER(_i64)]),
        "gsa_decoder_commit": (_int, [_vp]),
        "gsa_reserve": (_int, [_vp, _i32]),
        "gsa_generator_forward": (_int, [_vp, _vp, _i32, _vp, _vpp, _i32, _vp, _vp, _vpp, _i32]),
        "gsa_decoder_forward": (_int, [_vp, _vp, _i32, _vpp, _i32, _vp, _vp]),
        "gsa_generate": (_int, [_vp, _vp, _i32, _vp, _vpp, _i32, _vp, _vp]),
        "gsa_mapping_forward": (_int, [_vp, _vp, _i32, _vp, _vp]),
        "gsa_generator_forward_w": (_int, [_vp, _vp, _i32, _vp, _i32, _vpp, _i32, _vp, _vp, _vpp, _i32]),
        "gsa_generate_w": (_int, [_vp, _vp, _i32, _vp, _i32, _vpp, _i32, _vp, _vp]),
        "gsa_generate_downscaled": (_int, [_vp, _vp, _i32, _vp, _vp, _i32, _vpp, _i32, _i32, _vp, _vp]),
        "gsa_set_overlap": (_int, [_vp, _i32]),
        "gsa_set_precision": (_int, [_vp, _i32]),
        "gsa_segmentation_eval": (_int, [_vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
        "gsa_fill_inputs": (_int, [_vp, _vp, _i32, _u64, _u64, _vp, _vpp, _i32]),
        "gsa_profile_enable": (_int, [_vp, _i32]),
        "gsa_profile_collect": (_int, [_vp]),
        "gsa_profile_entry": (_int, [_vp, _i32, _c.POINTER(_c.c_char_p), _c.POINTER(_c.c_double), _c.POINTER(_i64),
                                     _c.POINTER(_c.c_double), _c.POINTER(_c.c_double), _c.POINTER(_c.c_double)]),
        "gsa_profile_reset": (_int, [_vp]),
        "gsa_version": (_c.c_char_p, []),
        "gsa_check": (_int, [_vp]),
        "gsa_status_snapshot": (_int, [_vp, _vp, _vp]),
        "gsa_debug_inject": (_int, [_vp, _i32, _i32]),
    },
    "gsa_train.h": {
        "gsa_train_conv": (_int, [_vp, _i32, _vp, _i32, _vp, _i32, _i32, _i32, _i32, _vp, _i32, _i32, _i32, _vp, _vp, _i32, _vp, _i32]),
        "gsa_train_conv_wgrad": (_int, [_vp, _i32, _vp, _i32, _vp, _i32, _i32, _i32, _i32, _vp, _i32, _i32, _vp, _vp]),
        "gsa_train_bn_lrelu_fwd": (_int, _bn + [_vp, _vp, _vp, _f32, _f32, _vp, _vp, _vp, _vp, _vp, _f32, _vp]),
        "gsa_train_bn_lrelu_bwd": (_int, _bn + [_vp, _vp, _vp, _f32, _vp, _vp, _vp, _f32, _vp, _vp, _vp]),
        "gsa_train_bn_sums": (_int, _bn + [_vp, _vp]),
        "gsa_train_bn_lrelu_fwd_sums": (_int, _bn + [_c.c_double, _vp, _vp, _vp, _f32, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _f32, _vp]),
        "gsa_train_bn_bwd_sums": (_int, _bn + [_vp, _vp, _vp, _f32, _vp, _vp, _vp, _f32, _vp, _vp]),
        "gsa_train_bn_lrelu_bwd_sums": (_int, _bn + [_c.c_double, _vp, _vp, _vp, _f32, _vp, _vp, _vp, _f32, _vp, _vp, _vp, _vp, _vp]),
        "gsa_train_softmax_ce": (_int, _bn + [_vp, _vp, _vp, _vp, _f32]),
        "gsa_train_upsample2_bwd": (_int, [_vp, _i32, _i32, _i32, _i32, _vp, _vp, _i32]),
        "gsa_train_add": (_int, [_vp, _i64, _vp, _vp, _vp]),
        "gsa_train_dropout_mask": (_int, [_vp, _i64, _u64, _c.c_uint32, _f32, _vp]),
        "gsa_train_adam": (_int, [_vp, _i64, _vp, _vp, _vp, _vp, _f32, _f32, _f32, _f32, _f32, _f32]),
    },
    "gsa_jpeg.h": {
        "gsa_jpeg_header": (_i64, [_i32, _i32, _i32, _i32, _vp, _i64]),
        "gsa_jpeg_workspace_bytes": (_i64, [_i32, _i32, _i32, _i32]),
        "gsa_jpeg_max_scan_bytes": (_i64, [_i32, _i32, _i32]),
        "gsa_jpeg_encode": (_int, [_vp, _i32, _i32, _i32, _vp, _i32, _i32, _vp, _i64, _vp, _i64, _vp]),
    },
    "gsa_jpeg_roundtrip.h": {
        "gsa_jpeg_roundtrip_workspace_bytes": (_i64, [_i32, _i32, _i32]),
        "gsa_jpeg_roundtrip": (_int, [_vp, _i32, _i32, _i32, _vp, _i32, _vp, _i64, _vp]),
    },
    "gsa_png.h": {
        "gsa_png_workspace_bytes": (_i64, [_i32, _i32, _i32]),
        "gsa_png_max_stream_bytes": (_i64, [_i32, _i32]),
        "gsa_png_encode": (_int, [_vp, _i32, _i32, _i32, _vp, _vp, _i64, _vp, _i64, _vp]),
    },
    "gsa_augment.h": {
        "gsa_augment_pairs": (_int, [_vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp]),
    },
    "gsa_mask.h": {
        "gsa_mask_morph": (_int, [_vp, _i32, _i32, _i32, _vp, _vp]),
    },
    "gsa_photometric.h": {
        "gsa_photometric": (_int, [_vp, _i32, _i32, _i32, _i32, _vp, _vp, _u64, _u64, _vp]),
    },
    "gsa_stats.h": {
        "gsa_pair_stats": (_int, [_vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp]),
    },
    "gsa_components.h": {
        "gsa_mask_components": (_int, [_vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    },
    "gsa_boundary.h": {
        "gsa_mask_boundary": (_int, [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp]),
    },
}

# The same rows for the entries whose header is not under include/ yet: path below the package -> {name: (result type, argument types)}.
# tests/test_overlay_abi.py checks it against the header's text, as SIGNATURES is checked (DESIGN.md section 21 says why it is apart).
EXTRA_SIGNATURES = {
    "csrc/gsa_overlay.h": {
        "gsa_overlay": (_int, [_vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _i32, _i32, _vp]),
    },
}

# The table that later features add their rows to: one key per header beside its unit, path below the package -> {name: (result
# type, argument types)}, bound after the two tables above.  Each header has a test of its own that checks its row against the
# header's text (tests/test_refine_abi.py for the first); no test pins this table's list of keys.  Folding all three tables into
# include/ and SIGNATURES is the follow-up that edits the tests which pin those two.
UNIT_SIGNATURES = {
    "csrc/gsa_refine.h": {
        "gsa_mask_refine": (_int, [_vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    },
    "csrc/gsa_compare.h": {
        "gsa_mask_compare": (_int, [_vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    },
    "csrc/gsa_loss.h": {
        "gsa_loss_workspace_bytes": (_i64, [_i32, _i32]),
        "gsa_loss_softmax": (_int, [_vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _f32, _i32, _f32, _vp, _vp, _vp, _vp]),
    },
    "csrc/gsa_scores.h": {
        "gsa_score_histogram": (_int, [_vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp]),
    },
    "csrc/gsa_resize.h": {
        "gsa_pair_resize": (_int, [_vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    },
    "csrc/gsa_region.h": {
        "gsa_region_workspace_bytes": (_i64, [_i32, _i32, _i32]),
        "gsa_region_tversky": (_int, [_vp, _i32, _i32, _i32, _vp, _vp, _vp, _f32, _f32, _f32, _i32, _f32, _i32, _vp, _vp, _vp, _vp, _vp]),
    },
}


class Api:
    """Function table of one shared library: every entry of ``SIGNATURES``, then of ``EXTRA_SIGNATURES``, then of ``UNIT_SIGNATURES``, bound once.  ``fn(name)`` returns an entry by its full name;
    the entries of include/gsa.h are attributes without the prefix as well (``api.create``, ``api.generate``, ...)."""

    def __init__(self, path, prefix="gsa_"):
        if not os.path.exists(path):
            raise GsaError("native library %s not found -- run `python -c 'import __graft_entry__ as g; "
                           "g.build()'` (there is no CPU fallback)" % path)
        self.path = path
        self.prefix = prefix
        # The process must end up with ONE HIP runtime: torch brings its own libamdhip64, and a library that pulled
        # in another copy first leaves the GPU invisible to one of the two -- so torch is imported before the dlopen.
        import torch  # noqa: F401
        self.lib = ctypes.CDLL(path)
        self._fns = {}
        for header, group in list(SIGNATURES.items()) + list(EXTRA_SIGNATURES.items()) + list(UNIT_SIGNATURES.items()):
            for name, (res, args) in group.items():
                try:
                    fn = getattr(self.lib, name)
                except AttributeError:
                    raise GsaError("%s does not export %s" % (path, name))
                fn.restype = res
                fn.argtypes = args
                self._fns[name] = fn
                if header == "gsa.h":
                    setattr(self, name[len(prefix):], fn)

    def fn(self, name):
        """The bound entry ``name`` (full name, e.g. "gsa_mask_morph")."""
        return self._fns[name]


_hip_api = None


def load_library():
    """The HIP library (cached).  Raises GsaError if it has not been built."""
    global _hip_api
    if _hip_api is None:
        _hip_api = Api(HIP_LIBRARY, "gsa_")
    return _hip_api


def _ptr_array(ptrs):
    arr = (ctypes.c_void_p * len(ptrs))()
    for i, p in enumerate(ptrs):
        arr[i] = p if p else None
    return arr


class Context:
    """One ``gsa_ctx``: a generator and/or decoder resident on one device."""

    def __init__(self, api, device=0):
        self.api = api
        self._h = ctypes.c_void_p()
        rc = api.create(int(device), ctypes.byref(self._h))
        if rc != 0:
            raise GsaError("create(device=%d) failed: %s" % (device, self._msg(None)))
        self.device = device
        self.generator_cfg = None
        self.decoder_cfg = None
        self.precision = "fp32"
        self._checked_first_step = False
        # hipGraph replay of small steps (image_generator._generate_on): graphs bake in the workspace pointers, the stream
        # structure (set_overlap) and must not contain profiling events -- any of these changing starts a new epoch
        self.graph_epoch = 0
        self.profiling = False

    def _msg(self, h):
        m = self.api.last_error(h)
        return m.decode("utf-8", "replace") if m else "unknown error"

    def _check(self, rc, what):
        if rc < 0:
            # any failing call ends the graph epoch: a pass that died half way leaves statistic rows that only the next EAGER
            # pass re-zeroes (gsa_api.cpp run_generator), and a failed commit / reserve leaves nothing a captured graph may use
            self.graph_epoch += 1
            raise GsaError("%s failed (%d): %s" % (what, rc, self._msg(self._h)))
        return rc

    def check(self):
        """gsa_check: synchronise the device and raise GsaError if a device-side check failed since the last clean one (the
        fused mapping network's exchange timed out; an instance-norm statistic left its fixed-point range)."""
        self._check(self.api.check(self._h), "check")

    def status_snapshot(self, stream, host_ptr):
        """gsa_status_snapshot: enqueue the 8-byte copy of the two sticky words to pinned host memory (no synchronisation)."""
        self._check(self.api.status_snapshot(self._h, stream, host_ptr), "status_snapshot")

    def debug_inject(self, kind, arg=0):
        """gsa_debug_inject (tests only)."""
        self._check(self.api.debug_inject(self._h, int(kind), int(arg)), "debug_inject")

    def _after_step(self):
        # ONE synchronising check per context, after its first step: a violated co-residency assumption or out-of-range
        # activations would otherwise yield wrong pairs with a zero status (the calls are stream-ordered); close() checks again
        if not self._checked_first_step:
            self._checked_first_step = True
            self.check()

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            try:
                if self._checked_first_step:
                    self.check()
            finally:
                self.api.destroy(self._h)
                self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- model setup ---------------------------------------------------------------
    def generator_init(self, cfg):
        gc = GeneratorConfig(int(cfg["max_res_log2"]), int(cfg["fmap_base"]), float(cfg["fmap_decay"]),
                             int(cfg["fmap_max"]), int(cfg["latent_size"]), int(cfg["channels"]),
                             1 if cfg["use_wscale"] else 0)
        if int(cfg.get("base_scale_x", 4)) != 4 or int(cfg.get("base_scale_y", 4)) != 4:
            raise GsaError("only the 4x4 base resolution of the reference config is supported")
        self._check(self.api.generator_init(self._h, ctypes.byref(gc)), "generator_init")
        self.generator_cfg = dict(cfg)

    def _set_params(self, fn, params, what):
        ignored = []
        for name, arr in params.items():
            a = np.ascontiguousarray(arr, dtype=np.float32)
            dims = (ctypes.c_int64 * max(a.ndim, 1))(*a.shape)
            rc = self._check(fn(self._h, name.encode("utf-8"), a.ctypes.data, a.ndim, dims),
                             "%s(%s)" % (what, name))
            if rc == 1:
                ignored.append(name)
        return ignored

    def generator_load(self, params):
        ignored = self._set_params(self.api.generator_set_param, params, "generator_set_param")
        self.graph_epoch += 1       # the commit frees and re-uploads the weight panels a captured graph bakes in
        self._check(self.api.generator_commit(self._h), "generator_commit")
        return ignored

    def decoder_init(self, cfg):
        feats = (ctypes.c_int32 * len(cfg["features"]))(*cfg["features"])
        inch = (ctypes.c_int32 * len(cfg["in_channels"]))(*cfg["in_channels"])
        if len(cfg["features"]) != len(cfg["in_channels"]) + 1:
            raise GsaError("decoder cfg: len(features) must be len(in_channels)+1")
        dc = DecoderConfig(len(cfg["in_channels"]), int(cfg["start_res"]), 1 if cfg["use_bn"] else 0,
                           feats, inch)
        self._check(self.api.decoder_init(self._h, ctypes.byref(dc)), "decoder_init")
        self.decoder_cfg = dict(cfg)

    def decoder_load(self, params):
        self._set_params(self.api.decoder_set_param, params, "decoder_set_param")
        self.graph_epoch += 1
        self._check(self.api.decoder_commit(self._h), "decoder_commit")

    def reserve(self, max_batch):
        self.graph_epoch += 1
        self._check(self.api.reserve(self._h, int(max_batch)), "reserve")

    # -- forward calls: every tensor argument is a raw address (int) or None -------------
    def generator_forward(self, stream, n, z, noise, rgb=None, img=None, feats=None):
        fp = _ptr_array(feats) if feats is not None else None
        self._check(self.api.generator_forward(self._h, stream, n, z, _ptr_array(noise), len(noise), rgb, img, fp,
                                               len(feats) if feats is not None else 0), "generator_forward")
        self._after_step()

    def decoder_forward(self, stream, n, feats, logits=None, mask=None):
        self._check(self.api.decoder_forward(self._h, stream, n, _ptr_array(feats), len(feats), logits, mask),
                    "decoder_forward")

    def generate(self, stream, n, z, noise, img, mask):
        self._check(self.api.generate(self._h, stream, n, z, _ptr_array(noise), len(noise), img, mask), "generate")
        self._after_step()

    def mapping_forward(self, stream, n, z, w):
        """gsa_mapping_forward: z (n, latent) -> the untruncated w (n, latent), into the caller's buffer."""
        self._check(self.api.mapping_forward(self._h, stream, n, z, w), "mapping_forward")
        self._after_step()

    def generator_forward_w(self, stream, n, dlatents, num_layers, noise, rgb=None, img=None, feats=None):
        """gsa_generator_forward_w: generator_forward from per-layer dlatents (n, num_layers, latent)."""
        fp = _ptr_array(feats) if feats is not None else None
        self._check(self.api.generator_forward_w(self._h, stream, n, dlatents, num_layers, _ptr_array(noise), len(noise), rgb, img, fp,
                                                 len(feats) if feats is not None else 0), "generator_forward_w")
        self._after_step()

    def generate_w(self, stream, n, dlatents, num_layers, noise, img, mask):
        """gsa_generate_w: the fused step from per-layer dlatents."""
        self._check(self.api.generate_w(self._h, stream, n, dlatents, num_layers, _ptr_array(noise), len(noise), img, mask),
                    "generate_w")
        self._after_step()

    def generate_downscaled(self, stream, n, z, dlatents, num_layers, noise, factor, img, mask):
        """gsa_generate_downscaled: the fused step from z or (z None) per-layer dlatents, the pair at 1/factor resolution."""
        self._check(self.api.generate_downscaled(self._h, stream, n, z, dlatents, num_layers, _ptr_array(noise), len(noise), int(factor),
                                                 img, mask), "generate_downscaled")
        self._after_step()

    def set_precision(self, precision):
        """"fp32" (default, bit-exact canonical path) or "bf16" (bf16 MFMA operands); before the weights are loaded."""
        self._check(self.api.set_precision(self._h, PRECISIONS[precision]), "set_precision")
        self.precision = precision

    def fill_inputs(self, stream, n, seed, first_index, z=None, noise=None):
        self._check(self.api.fill_inputs(self._h, stream, n, int(seed) & (2 ** 64 - 1), int(first_index), z,
                                         _ptr_array(noise) if noise is not None else None,
                                         len(noise) if noise is not None else 0), "fill_inputs")

    def segmentation_eval(self, stream, n, classes, H, W, logits, labels, confusion, loss_fixed):
        self._check(self.api.segmentation_eval(self._h, stream, n, classes, H, W, logits, labels, confusion, loss_fixed),
                    "segmentation_eval")

    def set_overlap(self, levels):
        self.graph_epoch += 1
        self._check(self.api.set_overlap(self._h, int(levels)), "set_overlap")

    # -- measurement ----------------------------------------------------------------------
    def profile_enable(self, on=True):
        self.graph_epoch += 1
        self.profiling = bool(int(on))
        self._check(self.api.profile_enable(self._h, int(on)), "profile_enable")

    def profile_reset(self):
        self._check(self.api.profile_reset(self._h), "profile_reset")

    def profile_entries(self):
        n = self._check(self.api.profile_collect(self._h), "profile_collect")
        out = []
        for i in range(n):
            name = ctypes.c_char_p()
            ms, fl, by, af = ctypes.c_double(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
            cnt = ctypes.c_int64()
            self._check(self.api.profile_entry(self._h, i, ctypes.byref(name), ctypes.byref(ms),
                                               ctypes.byref(cnt), ctypes.byref(fl), ctypes.byref(by), ctypes.byref(af)),
                        "profile_entry")
            out.append({"name": name.value.decode(), "ms": ms.value, "launches": cnt.value,
                        "flops": fl.value, "bytes": by.value, "alg_flops": af.value})
        return out
