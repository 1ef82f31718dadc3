"""The region-overlap loss of csrc/gsa_region.h in float64 torch, with the gradient from autograd, and the element-wise error bounds
that tests/test_gpu_region.py holds the kernels to (no test in here; tests/test_region_ref.py checks this module against a numpy
double loop and a finite difference, tests/test_gpu_region.py and tests/test_gpu_region_trainer.py import it).

``region_f64`` is the specification and nothing else: the gradient comes out of ``backward()`` through the sums, the index and the
softmax, not out of the header's restated formula.  alpha, beta, smooth, grad_scale and the class weights are rounded to fp32 first,
as the C entry receives them; everything after that is float64.

``bounds`` gives, for the same inputs, a bound on |got - ref| in units of rho = C * 2**-24 for every output: the error of each
fp32 operand carried through the same expressions, tests/f64_ref.assert_bounded's convention, with U = 2**-24 the unit roundoff of
one fp32 operation.  With m the pixel's largest logit, p its softmax, d_k = |z_k - m|, E = sum_k p_k d_k, K the class count and
tiny = 2**-126 / rho (what underflows in fp32 is lost whole):

    p_k     <- p_k (d_k + E + K + 5) + tiny                  as tests/loss_ref.py: the exponent's rounding is a relative error d_k
    I_k,P_k <- the sums of the pixels' bounds, and for the double sums themselves, added in another order than the reference's,
               HW * 2**-52 / rho times the sum;  G_k is exact
    N_k     <- bound(I_k);   D_k <- |1 - alpha - beta| bound(I_k) + alpha bound(P_k)      (smooth, beta G_k: exact operands)
    TI_k    <- (bound(N_k) + TI_k bound(D_k)) / D_k, and + TI_k for the rounding of ``index`` to fp32
    L       <- sum_k (a_k c_k / A) bound(TI_k) + |L|         the sum is double, its result rounded once
    g_k     <- the two coefficients by the quotient rule: with w_k = a_k c_k / A,
               own:   w_k ((bound(D_k) + (1 - beta) bound(N_k)) / D_k^2 + 2 |D_k - (1 - beta) N_k| bound(D_k) / D_k^3)
               other: w_k alpha (bound(N_k) / D_k^2 + 2 N_k bound(D_k) / D_k^3)
    s_i     <- sum_k (bound(g_k,i) p_k + |g_k,i| bound(p_k))     s_i = sum_k g_k,i p_k, formed in double
    dz_j    <- |grad_scale| (bound(p_j) |g_j - s| + p_j (bound(g_j) + bound(s))) + |dz_j| + tiny
               the difference g_j - s is formed in double from its operands, so it carries their errors and none of its own; the
               last term is the one rounding to fp32.
An output whose bound is 0 must be exact.
"""
import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24


def _f32(v):
    return float(np.float32(v))


def _pieces(z, y, cw, alpha, beta, smooth, mode):
    """What both functions share, differentiable in z: (valid, onehot, p, I, P, G, N, D, TI, a, w, A, L)."""
    K = z.shape[1]
    valid = (y >= 0) & (y < K)
    onehot = F.one_hot(y.clamp(0, K - 1), K).permute(0, 2, 1).to(z.dtype) * valid[:, None].to(z.dtype)
    m = z.detach().max(dim=1, keepdim=True).values
    ex = (z - m).exp()
    p = ex / ex.sum(dim=1, keepdim=True)
    pv = p * valid[:, None].to(z.dtype)
    I, P, G = (pv * onehot).sum(dim=2), pv.sum(dim=2), onehot.sum(dim=2)                  # (n, K)
    N = I + smooth
    D = (1.0 - alpha - beta) * I + alpha * P + beta * G + smooth
    a = (D > 0) & (G.sum(dim=1, keepdim=True) > 0) & ((G > 0) if mode == 0 else torch.ones_like(G, dtype=torch.bool))
    one = torch.ones_like(D)
    TI = torch.where(a, N / torch.where(a, D, one), torch.zeros_like(D))
    c = torch.ones(K, dtype=z.dtype) if cw is None else cw.to(z.dtype)
    ac = a.to(z.dtype) * c
    A = ac.sum(dim=1)                                                                       # (n,)
    live = A != 0
    w = torch.where(live[:, None], ac / torch.where(live, A, torch.ones_like(A))[:, None], torch.zeros_like(ac))
    L = (w * (1.0 - TI)).sum(dim=1)
    return valid, onehot, p, I, P, G, N, D, TI, a, w, A, L


def _rounded(cw, alpha, beta, smooth, grad_scale):
    cw = None if cw is None else cw.detach().float().double()
    return cw, _f32(alpha), _f32(beta), _f32(smooth), _f32(grad_scale)


def region_f64(logits, labels, alpha=0.5, beta=0.5, smooth=1.0, mode=0, cw=None, grad_scale=1.0):
    """logits (n, K, HW) (fp32 values, evaluated in float64), labels (n, HW) integers, cw (K,) or None, mode 0 ("present") or 1
    ("all") -> (loss (n,), sums (n, 3, K) = [I, P, G], index (n, K), dlogits (n, K, HW) = grad_scale * d sum(loss) / d logits)."""
    cw, alpha, beta, smooth, grad_scale = _rounded(cw, alpha, beta, smooth, grad_scale)
    z = logits.detach().double().clone().requires_grad_(True)
    _valid, _onehot, _p, I, P, G, _N, _D, TI, _a, _w, _A, L = _pieces(z, labels.long(), cw, alpha, beta, smooth, mode)
    (grad_scale * L.sum()).backward()
    return L.detach(), torch.stack([I, P, G], dim=1).detach(), TI.detach(), z.grad.detach()


def bounds(logits, labels, alpha=0.5, beta=0.5, smooth=1.0, mode=0, cw=None, grad_scale=1.0, rho=U):
    """-> {"loss": (n,), "sums": (n, 3, K), "index": (n, K), "dlogits": (n, K, HW)}: the bounds of the module's docstring, in units
    of ``rho``."""
    cw, alpha, beta, smooth, grad_scale = _rounded(cw, alpha, beta, smooth, grad_scale)
    tiny = 2.0 ** -126 / rho
    with torch.no_grad():
        z = logits.detach().double()
        n, K, HW = z.shape
        valid, onehot, p, I, P, G, N, D, TI, a, w, _A, L = _pieces(z, labels.long(), cw, alpha, beta, smooth, mode)
        v = valid[:, None].double()
        m = z.max(dim=1, keepdim=True).values
        dist = (z - m).abs()
        E = (p * dist).sum(dim=1, keepdim=True)
        b_p = p * (dist + E + K + 5) + tiny
        eps64 = HW * 2.0 ** -52 / rho                    # two double sums of HW terms in different orders
        b_I = (b_p * onehot).sum(dim=2) + eps64 * I
        b_P = (b_p * v).sum(dim=2) + eps64 * P
        b_N = b_I
        b_D = abs(1.0 - alpha - beta) * b_I + alpha * b_P
        Ds = torch.where(a, D, torch.ones_like(D))
        on = a.double()
        b_TI = on * (b_N + TI * b_D) / Ds
        b_L = (w * b_TI).sum(dim=1) + L.abs()
        own = w * (D - (1.0 - beta) * N) / Ds ** 2                                  # -g where y == k
        other = w * alpha * N / Ds ** 2                                             # +g where y != k
        b_own = w * ((b_D + (1.0 - beta) * b_N) / Ds ** 2 + 2 * (D - (1.0 - beta) * N).abs() * b_D / Ds ** 3)
        b_other = w * alpha * (b_N / Ds ** 2 + 2 * N * b_D / Ds ** 3)
        g = -own[:, :, None] * onehot + other[:, :, None] * (1 - onehot)            # (n, K, HW)
        b_g = b_own[:, :, None] * onehot + b_other[:, :, None] * (1 - onehot)
        s = (g * p).sum(dim=1, keepdim=True)
        b_s = (b_g * p + g.abs() * b_p).sum(dim=1, keepdim=True)
        dz = abs(grad_scale) * p * (g - s)
        b_dz = v * (abs(grad_scale) * (b_p * (g - s).abs() + p * (b_g + b_s)) + dz.abs() + tiny)
        return {"loss": b_L, "sums": torch.stack([b_I, b_P, torch.zeros_like(G)], dim=1), "index": b_TI + TI, "dlogits": b_dz}


def region_loops(logits, labels, alpha=0.5, beta=0.5, smooth=1.0, mode=0, cw=None, grad_scale=1.0):
    """The header's rule, gradient formula included, as plain double loops over numpy arrays: what tests/test_region_ref.py holds
    ``region_f64`` to at a tiny size.  Same arguments and results (numpy arrays)."""
    z = np.asarray(logits, np.float64)
    y = np.asarray(labels, np.int64)
    n, K, HW = z.shape
    alpha, beta, smooth, grad_scale = _f32(alpha), _f32(beta), _f32(smooth), _f32(grad_scale)
    c = np.ones(K) if cw is None else np.asarray(cw, np.float32).astype(np.float64)
    loss, sums, index, dz = np.zeros(n), np.zeros((n, 3, K)), np.zeros((n, K)), np.zeros((n, K, HW))
    for s in range(n):
        p = np.zeros((K, HW))
        for i in range(HW):
            m = max(z[s, k, i] for k in range(K))
            se = sum(np.exp(z[s, k, i] - m) for k in range(K))
            for k in range(K):
                p[k, i] = np.exp(z[s, k, i] - m) / se
            if 0 <= y[s, i] < K:
                for k in range(K):
                    sums[s, 1, k] += p[k, i]
                sums[s, 0, y[s, i]] += p[y[s, i], i]
                sums[s, 2, y[s, i]] += 1
        N, D, a = np.zeros(K), np.zeros(K), np.zeros(K)
        for k in range(K):
            I, P, G = sums[s, :, k]
            N[k] = I + smooth
            D[k] = (1.0 - alpha - beta) * I + alpha * P + beta * G + smooth
            a[k] = 1.0 if D[k] > 0 and sums[s, 2].sum() > 0 and (mode == 1 or G > 0) else 0.0
            index[s, k] = N[k] / D[k] if a[k] else 0.0
        A = sum(a[k] * c[k] for k in range(K))
        if A == 0:
            continue
        loss[s] = sum(a[k] * c[k] * (1.0 - index[s, k]) for k in range(K)) / A
        for i in range(HW):
            if not 0 <= y[s, i] < K:
                continue
            g = np.zeros(K)
            for k in range(K):
                if not a[k]:
                    continue
                if y[s, i] == k:
                    g[k] = -(a[k] * c[k] / A) * (D[k] - (1.0 - beta) * N[k]) / D[k] ** 2
                else:
                    g[k] = (a[k] * c[k] / A) * alpha * N[k] / D[k] ** 2
            dot = sum(g[k] * p[k, i] for k in range(K))
            for j in range(K):
                dz[s, j, i] = grad_scale * p[j, i] * (g[j] - dot)
    return loss, sums, index, dz
