"""The decoder losses of csrc/gsa_loss.h in float64 torch, with the gradient from autograd, and the element-wise error bounds that
tests/test_gpu_loss.py holds the kernels to (no test in here; tests/test_gpu_loss.py and tests/test_gpu_loss_trainer.py import it).

``loss_f64`` is the specification and nothing else: the gradient of mode "focal" comes out of ``backward()`` through the
normaliser, not out of a restated formula.

``bounds`` gives, for the same inputs, a bound on |got - ref| in units of rho = C * 2**-24 for every output: the same expressions on
the magnitudes of their operands, tests/f64_ref.assert_bounded's convention, with U = 2**-24 the unit roundoff of one fp32 operation.
With m the pixel's largest logit, sm its softmax, d_k = |z_k - m|, E = sum_k sm_k d_k, A = sum_{k != y} sm_k d_k, K the class count
and tiny = 2**-126 / rho (what underflows in fp32 is lost whole):

    sm_k    <- sm_k (d_k + E + K + 5) + tiny                     as test_softmax_ce: the exponent's rounding is a relative error d_k
    q       <- A + q (E + K + 5) + tiny                          the sum of the other classes over the sum of all
    CE      <- |m| + |lse| + |z_y| + E + K + 4                   as test_softmax_ce's loss terms
    w       <- w if it is a product of a class weight and a table entry, else 0 (exact)
    beta    <- gamma q^(gamma-1) (bound of q) + 3 beta + tiny    (0 at gamma = 0: beta is 1 exactly)
    h       <- gamma ((gamma-1) q^(gamma-2) (bound of q) p_y + q^(gamma-1) (bound of p_y)) + 3 h + tiny
    W, B, S <- the sums of the pixels' bounds: bound(w), bound(w) beta + w bound(beta), bound(b) |CE| + b bound(CE), and for the
               double sums themselves, added in another order than the reference's, HW * 2**-52 / rho times the sum of the
               magnitudes;  T is exact
    L = S/D <- (bound(S) + |L| bound(D)) / D + |L|               D = HW (exact), W or B; 0 where D = 0: the result is exact
    dz_k    <- |grad_scale| / D * (w G bound(e_k) + (w bound(G) + bound(w) G) |e_k| + w G |e_k| (3 + bound(D) / D)) + tiny
               with e_k = sm_k, and -q at k = y; G = beta + h |CE| + [focal] |L| h the magnitude of g - L h, and
               bound(G) = bound(beta) + bound(h) |CE| + h bound(CE) + [focal] (bound(L) h + |L| bound(h)) + 2 G;
               and, for the float64 reference itself, whose autograd forms e_y as p_y - 1, 2**-50 / rho * w G (sm_k + [k == y]).
"""
import torch
import torch.nn.functional as F

U = 2.0 ** -24
FAR_INDEX = 1025


def _pieces(z, y, cw, d2, tab):
    """What both functions share, differentiable in z: (valid, onehot, m, sm, q, py, CE, lse, zy, w)."""
    K = z.shape[1]
    valid = (y >= 0) & (y < K)
    yc = y.clamp(0, K - 1)
    onehot = F.one_hot(yc, K).permute(0, 2, 1).to(z.dtype)
    m = z.detach().max(dim=1, keepdim=True).values
    ex = (z - m).exp()
    se = ex.sum(dim=1)
    so = (ex * (1 - onehot)).sum(dim=1)
    zy = (z * onehot).sum(dim=1)
    lse = m[:, 0] + se.log()
    CE = lse - zy
    q = so / se
    sm = ex / se[:, None]
    py = (sm * onehot).sum(dim=1)
    w = valid.to(z.dtype)
    if cw is not None:
        w = w * cw.to(z.dtype)[yc]
    if d2 is not None:
        d = d2.long()
        w = w * tab.to(z.dtype)[torch.where((d >= 0) & (d <= FAR_INDEX - 1), d, torch.full_like(d, FAR_INDEX))]
    return valid, onehot, m, sm, q, py, CE, lse, zy, w


def loss_f64(logits, labels, cw=None, d2=None, tab=None, gamma=0.0, normalise=0, grad_scale=1.0):
    """logits (n, K, HW) (rounded to fp32 values, evaluated in float64), labels (n, HW) integers, cw (K,), d2 (n, HW) integers and
    tab (1026,) or None -> (loss (n,), sums (n, 4) = [W, B, S, T], dlogits (n, K, HW) = grad_scale * d sum(loss) / d logits)."""
    z = logits.detach().double().clone().requires_grad_(True)
    valid, _onehot, _m, _sm, q, _py, CE, _lse, _zy, w = _pieces(z, labels.long(), cw, d2, tab)
    beta = torch.ones_like(q) if gamma == 0 else q ** gamma
    b = w * beta
    W, B, S, T = w.sum(dim=1), b.sum(dim=1), (b * CE).sum(dim=1), valid.double().sum(dim=1)
    D = (torch.full_like(S, z.shape[2]), W, B)[normalise]
    L = torch.where(D != 0, S / torch.where(D != 0, D, torch.ones_like(D)), torch.zeros_like(S))
    (grad_scale * L.sum()).backward()
    return L.detach(), torch.stack([W, B, S, T], dim=1).detach(), z.grad.detach()


def bounds(logits, labels, cw=None, d2=None, tab=None, gamma=0.0, normalise=0, grad_scale=1.0, rho=U):
    """-> {"loss": (n,), "sums": (n, 4), "dlogits": (n, K, HW)}: the bounds of the module's docstring, in units of ``rho``."""
    assert gamma in (0.0, 1.0) or gamma >= 2.0, "q^(gamma - 2) is not bounded at q = 0 for 1 < gamma < 2"
    tiny = 2.0 ** -126 / rho
    with torch.no_grad():
        z = logits.detach().double()
        n, K, HW = z.shape
        valid, onehot, m, sm, q, py, CE, lse, zy, w = _pieces(z, labels.long(), cw, d2, tab)
        dist = (z - m).abs()
        E = (sm * dist).sum(dim=1)
        A = (sm * (1 - onehot) * dist).sum(dim=1)
        dy = (dist * onehot).sum(dim=1)
        b_sm = sm * (dist + E[:, None] + K + 5) + tiny
        b_q = A + q * (E + K + 5) + tiny
        b_py = py * (dy + E + K + 5) + tiny
        b_CE = m[:, 0].abs() + lse.abs() + zy.abs() + E + K + 4
        b_w = w if (cw is not None and d2 is not None) else torch.zeros_like(w)
        aCE = CE.abs()
        if gamma == 0:
            beta, h = torch.ones_like(q), torch.zeros_like(q)
            b_beta, b_h = torch.zeros_like(q), torch.zeros_like(q)
        else:
            qg1 = q ** (gamma - 1)
            beta, h = qg1 * q, gamma * qg1 * py
            b_beta = gamma * qg1 * b_q + 3 * beta + tiny
            b_qg1 = (gamma - 1) * q ** (gamma - 2) * b_q if gamma >= 2 else torch.zeros_like(q)
            b_h = gamma * (b_qg1 * py + qg1 * b_py) + 3 * h + tiny
        b = w * beta
        b_b = b_w * beta + w * b_beta
        W, B, S = w.sum(dim=1), b.sum(dim=1), (b * CE).sum(dim=1)
        eps64 = HW * 2.0 ** -52 / rho                    # two double sums of HW terms in different orders
        b_W, b_B = b_w.sum(dim=1) + eps64 * W, b_b.sum(dim=1) + eps64 * B
        b_S = (b_b * aCE + b * b_CE).sum(dim=1) + eps64 * (b * aCE).sum(dim=1)
        zero = torch.zeros_like(S)
        D, b_D = ((torch.full_like(S, HW), zero), (W, b_W), (B, b_B))[normalise]
        live = D != 0
        Ds = torch.where(live, D, torch.ones_like(D))
        L = torch.where(live, S / Ds, zero).abs()
        b_L = torch.where(live, (b_S + L * b_D) / Ds + L, zero)
        focal = 1.0 if normalise == 2 else 0.0
        Lp, b_Lp = (focal * L)[:, None], (focal * b_L)[:, None]
        G = beta + h * aCE + Lp * h
        b_G = b_beta + b_h * aCE + h * b_CE + b_Lp * h + Lp * b_h + 2 * G
        e = sm * (1 - onehot) + q[:, None] * onehot
        b_e = b_sm * (1 - onehot) + b_q[:, None] * onehot
        rel = (3 + b_D / Ds)[:, None, None]
        inner = (w * G)[:, None] * b_e + (w * b_G + b_w * G)[:, None] * e + (w * G)[:, None] * e * rel
        # the reference's own rounding: autograd forms e_y as p_y - 1 in float64, which is 0 below q = 2**-53 where -q is not
        inner = inner + 2.0 ** -50 / rho * (w * G)[:, None] * (sm + onehot)
        b_dz = torch.where(live[:, None, None], abs(grad_scale) / Ds[:, None, None] * inner, torch.zeros_like(inner)) + tiny
        return {"loss": b_L, "sums": torch.stack([b_W, b_B, b_S, zero], dim=1), "dlogits": b_dz}
