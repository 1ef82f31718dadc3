"""The host arithmetic of the weight commit without a GPU (csrc/gsa_pack.h: the gsa_pack_* entries of the HIP library).

Every packed layout is the contract between the commit, the MFMA kernels and the oracle.  Here each one is restated in numpy as an
index map -- reshape the (cout, channel, tap) tensor to (g, n, cb, kq, j, t) and transpose to the packed order [g][cb][t][kq][n][j]
-- and compared exactly: cout = 16g + n, channel = 4J*cb + J*kq + j, J = 4 (J = 2 for the F(4x4,3x3) panel).  The shapes are
non-square and no powers of two, so that swapped indices or swapped sizes cannot cancel; the values are distinct.  The tap rules
are restated in the precision and order DESIGN.md fixes: effective weights with two fp32 roundings, fp32 sums ky-then-kx ascending
for the sub-pixel taps, float64 transforms rounded once for the Winograd panels.  No tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

SHAPES = [(32, 16), (16, 48), (48, 32)]
SCALES = [(1, 1.0), (0, 1.0), (1, 0.01)]      # (use_wscale, lr_mult)
STD = np.float32(0.7311)
_F, _I, _P = C.c_float, C.c_int, C.c_void_p
_WEIGHT = [_P, _I, _I, _F, _I, _F, _P]
_ARGS = {"conv3": _WEIGHT, "deconv": _WEIGHT, "upconv": _WEIGHT, "wino": _WEIGHT, "wino43": _WEIGHT, "conv1": [_P, _I, _I, _P],
         "final": [_P, _I, _I, _P], "bf16": [_P, C.c_size_t, _P], "bn_fold": [_P, _P, _P, _P, _P, _I, _P, _P],
         "constant": [_P, _I, _P], "mapping": [_P, _I, _F, _I, _P]}


@pytest.fixture(scope="module")
def pack(hip_library):
    import torch  # noqa: F401  -- before the dlopen, as gan_segmentation_amd._lib.Api does: one HIP runtime per process
    lib = C.CDLL(hip_library)
    fns = {}
    for name, args in _ARGS.items():
        fns[name] = getattr(lib, "gsa_pack_" + name)
        fns[name].restype, fns[name].argtypes = None, args
    fns["bf16_rne"] = lib.gsa_pack_bf16_rne
    fns["bf16_rne"].restype, fns["bf16_rne"].argtypes = C.c_uint16, [_F]

    def call(name, out_shape, *args, dtype=np.float32):
        """gsa_pack_<name>(*args, out) -> out; arrays go by pointer.  The buffer starts as NaN / 0xFFFF: an unwritten element shows."""
        out = np.full(out_shape, np.nan if dtype == np.float32 else 0xFFFF, dtype)
        keep = [np.ascontiguousarray(a) if isinstance(a, np.ndarray) else a for a in args]
        fns[name](*[a.ctypes.data if isinstance(a, np.ndarray) else a for a in keep], out.ctypes.data)
        return out
    call.rne = fns["bf16_rne"]
    return call


def draw(shape, seed):
    """Distinct float32 values from a seeded generator (a draw of twice the size, its duplicates dropped, shuffled)."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    u = np.unique(rng.standard_normal(2 * n).astype(np.float32))
    rng.shuffle(u)
    assert u.size >= n
    return u[:n].reshape(shape).copy()


def eff(w, use_std, lr):
    """(w * std) * lr_mult: two fp32 roundings."""
    v = w * STD if use_std else w
    return v * np.float32(lr)


def blocked(x, J=4):
    """(O, I, T) -> [O/16][I/4J][T][kq = 4][n = 16][J]"""
    O, I, T = x.shape
    return x.reshape(O // 16, 16, I // (4 * J), 4, J, T).transpose(0, 2, 5, 3, 1, 4)


@pytest.mark.parametrize("us,lr", SCALES)
@pytest.mark.parametrize("O,I", SHAPES)
def test_pack_conv3(pack, O, I, us, lr):
    w = draw((O, I, 3, 3), 1)
    assert np.array_equal(pack("conv3", (O // 16, I // 16, 9, 4, 16, 4), w, O, I, STD, us, lr), blocked(eff(w, us, lr).reshape(O, I, 9)))


@pytest.mark.parametrize("us,lr", SCALES)
@pytest.mark.parametrize("O,I", SHAPES)
def test_pack_deconv(pack, O, I, us, lr):
    w = draw((I, O, 4, 4), 2)       # IOHW
    want = blocked(eff(w, us, lr).transpose(1, 0, 2, 3).reshape(O, I, 16))
    assert np.array_equal(pack("deconv", want.shape, w, I, O, STD, us, lr), want)


@pytest.mark.parametrize("us,lr", SCALES)
@pytest.mark.parametrize("O,I", SHAPES)
def test_pack_upconv(pack, O, I, us, lr):
    """Wd[a][b] = sum over ky in S(a), kx in S(b) of W[ky][kx]: fp32, ky then kx ascending, the first term assigned."""
    w = draw((O, I, 3, 3), 3)
    e = eff(w, us, lr)
    S = [[2], [1, 2], [0, 1], [0]]
    wd = np.empty((O, I, 4, 4), np.float32)
    for a in range(4):
        for b in range(4):
            terms = [e[:, :, ky, kx] for ky in S[a] for kx in S[b]]
            acc = terms[0]
            for t in terms[1:]:
                acc = acc + t       # float32 + float32
            wd[:, :, a, b] = acc
    assert wd.dtype == np.float32
    assert np.array_equal(pack("upconv", (O // 16, I // 16, 16, 4, 16, 4), w, O, I, STD, us, lr), blocked(wd.reshape(O, I, 16)))


@pytest.mark.parametrize("O,I", SHAPES)
def test_pack_conv1_takes_the_raw_weights(pack, O, I):
    w = draw((O, I), 4)
    assert np.array_equal(pack("conv1", (O // 16, I // 16, 1, 4, 16, 4), w, O, I), blocked(w.reshape(O, I, 1)))


def wino_u(e):
    """U = G g G^T of F(2x2,3x3) in float64, association (k0 +- k1) + k2, halved; rows first, then columns; cast once."""
    k = e.astype(np.float64)

    def g(k0, k1, k2):
        return [k0, 0.5 * ((k0 + k1) + k2), 0.5 * ((k0 - k1) + k2), k2]
    r = g(k[:, :, 0], k[:, :, 1], k[:, :, 2])                        # r[a]: (O, I, 3)
    u = np.stack([np.stack(g(ra[..., 0], ra[..., 1], ra[..., 2]), -1) for ra in r], -2)      # (O, I, a, b)
    return u.astype(np.float32)


@pytest.mark.parametrize("us,lr", SCALES)
@pytest.mark.parametrize("O,I", SHAPES)
def test_pack_wino(pack, O, I, us, lr):
    w = draw((O, I, 3, 3), 5)
    want = blocked(wino_u(eff(w, us, lr)).reshape(O, I, 16))
    assert np.array_equal(pack("wino", want.shape, w, O, I, STD, us, lr), want)


def wino43_u(e):
    """U = G g G^T with Lavin & Gray's 6x3 G in float64, each row of three products summed (p0 + p1) + p2; cast once."""
    G = np.array([[0.25, 0, 0], [-1.0 / 6, -1.0 / 6, -1.0 / 6], [-1.0 / 6, 1.0 / 6, -1.0 / 6], [1.0 / 24, 1.0 / 12, 1.0 / 6],
                  [1.0 / 24, -1.0 / 12, 1.0 / 6], [0, 0, 1]])
    k = e.astype(np.float64)[:, :, None]                             # (O, I, 1, ky, kx)
    Gy = G[:, :, None]                                               # (i, ky, 1)
    r = (Gy[:, 0] * k[:, :, :, 0] + Gy[:, 1] * k[:, :, :, 1]) + Gy[:, 2] * k[:, :, :, 2]      # (O, I, i, kx)
    r = r[:, :, :, None]                                             # (O, I, i, 1, kx)
    u = (r[..., 0] * G[:, 0] + r[..., 1] * G[:, 1]) + r[..., 2] * G[:, 2]                     # (O, I, i, j)
    return u.astype(np.float32)


@pytest.mark.parametrize("us,lr", SCALES)
@pytest.mark.parametrize("O,I", SHAPES + [(16, 64)])
def test_pack_wino43_has_eight_channel_blocks(pack, O, I, us, lr):
    w = draw((O, I, 3, 3), 6)
    want = blocked(wino43_u(eff(w, us, lr)).reshape(O, I, 36), J=2)
    assert want.shape == (O // 16, I // 8, 36, 4, 16, 2)
    assert np.array_equal(pack("wino43", want.shape, w, O, I, STD, us, lr), want)


@pytest.mark.parametrize("K", [1, 2, 8])
@pytest.mark.parametrize("I", [16, 48])
def test_pack_final(pack, K, I):
    w = draw((K, I, 3, 3), 7)
    want = w.reshape(K, I // 16, 16, 9).transpose(1, 3, 2, 0)        # [cb][tap][c16][K]
    assert np.array_equal(pack("final", want.shape, w, K, I), want)


def _f32(bits):
    return np.array([bits], np.uint32).view(np.float32)[0]


@pytest.mark.parametrize("bits,want", [
    (0x3F808000, 0x3F80),      # a tie, the lower neighbour even: down
    (0x3F818000, 0x3F82),      # a tie, the lower neighbour odd: up
    (0x3F808001, 0x3F81), (0x3F817FFF, 0x3F81), (0xBF818000, 0xBF82),
    (0x3FFFFFFF, 0x4000),      # the carry runs through the mantissa into the exponent
    (0x7F7FFFFF, 0x7F80),      # ... and from the largest finite value to infinity
    (0x7F800000, 0x7F80), (0xFF800000, 0xFF80),                      # infinities
    (0x7FC00001, 0x7FC0), (0x7F800001, 0x7FC0), (0xFFFFFFFF, 0xFFFF),      # NaNs stay NaNs (a payload in the low half alone too)
    (0x00000000, 0x0000), (0x80000000, 0x8000)])
def test_bf16_rne(pack, bits, want):
    assert pack.rne(_f32(bits)) == want
    assert pack("bf16", (1,), np.array([bits], np.uint32).view(np.float32), 1, dtype=np.uint16)[0] == want


def test_bf16_repack_is_elementwise_rne(pack):
    import torch
    x = draw((9 * 256,), 8)
    x[::7] = (x[::7].view(np.uint32) & 0xFFFF0000 | 0x8000).view(np.float32)      # exact ties among them
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(pack("bf16", x.shape, x, x.size, dtype=np.uint16), want)


def test_bn_fold(pack):
    """s = gamma / sqrtf(var + 1e-5f); k = fmaf(bias - mean, s, beta): the product is exact in float64, one rounding at the end."""
    n = 48
    g, b, m, bias = (draw((n,), 10 + i) for i in range(4))
    v = np.abs(draw((n,), 14)) + np.float32(0.01)
    s = np.full(n, np.nan, np.float32)
    k = pack("bn_fold", (n,), g, b, m, v, bias, n, s)      # (..., s, k): s is written in place, k is the entry's last argument
    want_s = g / np.sqrt(v + np.float32(1e-5))
    assert want_s.dtype == np.float32
    want_k = ((bias - m).astype(np.float64) * want_s.astype(np.float64) + b.astype(np.float64)).astype(np.float32)
    assert np.array_equal(s, want_s) and np.array_equal(k, want_k)


def test_commit_transposes(pack):
    """The constant tensor (C,4,4) -> [pixel][channel]; a mapping weight (L,L) [j][k] -> [k][j], effective at lr_mult 0.01."""
    w = draw((48, 4, 4), 20)
    assert np.array_equal(pack("constant", (16, 48), w, 48), w.reshape(48, 16).T)
    m = draw((48, 48), 21)
    for us in (0, 1):
        assert np.array_equal(pack("mapping", (48, 48), m, 48, STD, us), eff(m, us, 0.01).T)
