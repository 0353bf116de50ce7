"""Float64 restatement of the Matern-5/2 kernel with derivative observations, written from the formulas (the oracle of
tests/test_matern52grad_cpu.py and tests/test_gpu_matern52grad.py; no project code).

Interleaved ordering: row i (d + 1) + a is component a of point i, a = 0 the value, a = 1..d the partial derivatives.  With z = x / l per
dimension, delta = z_i - z_j, rho = |delta|^2, s = sqrt(5 rho), e = exp(-s) the radial factors are

    k = (1 + s + s^2 / 3) e      g = (5/3) (1 + s) e  (= -2 dk/drho)      w = (25/3) e  (= -2 dg/drho)      u = (125/3) e / s  (= -2 dw/drho)

(u only ever multiplies terms of order rho^2: it is taken as 0 where s < 1e-12).  Blocks of a pair:

    K[i0, j0] = k    K[i0, jb] = g delta_b / l_b    K[ia, j0] = -g delta_a / l_a    K[ia, jb] = (g [a = b] - w delta_a delta_b) / (l_a l_b)

Product, with r~_b = r_b / l_b and B = delta . r~_j:

    out_i0 = sum_j [ k r_j0 + g B ]        out_ia = (1 / l_a) sum_j [ g r~_ja - delta_a (g r_j0 + w B) ]

Bilinear form, with l~_a = l_a / lengthscale_a, A = delta . l~_i, C = l~_i . r~_j, M = l_i0 B - r_j0 A + C:

    G[0]     = l^T K r = sum_ij [ k l0 r0 + g M - w A B ]
    G[1 + a] = -sum_ij [ delta_a^2 (g l0 r0 + w M - u A B) - 2 g (delta_a (l0 r~_a - r0 l~_a) + l~_a r~_a) + 2 w delta_a (l~_a B + r~_a A) ]
    d(l^T K r) / d lengthscale_a = -G[1 + a] / lengthscale_a

x: [n, d]; ls: 1 or d values (any shape)."""
import torch


def _ls(ls, d):
    ls = torch.as_tensor(ls).double().reshape(-1)
    return ls.expand(d) if ls.numel() == 1 else ls


def _pairs(x1, x2, ls):
    """delta [n, m, d], the radial factors (k, g, w, u) [n, m], the lengthscales [d]."""
    d = x1.shape[-1]
    l = _ls(ls, d)
    delta = x1.double().unsqueeze(1) / l - x2.double().unsqueeze(0) / l
    rho = delta.pow(2).sum(-1)
    # (autograd: the square root is taken of positive values only; where rho == 0 every derivative of rho is 0 as well, so s = 0 with no gradient
    # is the exact derivative there, not an approximation)
    s = torch.where(rho > 0, (5.0 * torch.where(rho > 0, rho, torch.ones_like(rho))).sqrt(), torch.zeros_like(rho))
    e = torch.exp(-s)
    u = torch.where(s > 1e-12, (125.0 / 3.0) * e / s.clamp_min(1e-300), torch.zeros_like(s))
    return delta, ((1.0 + s + s * s / 3.0) * e, (5.0 / 3.0) * (1.0 + s) * e, (25.0 / 3.0) * e, u), l


def pair_covariances(x1, x2, ls):
    """k [n, m]: what the tests' guard on the share of mixed pairs looks at."""
    return _pairs(x1, x2, ls)[1][0]


def dense(x1, x2, ls):
    """K [n (d + 1), m (d + 1)] in float64: the (d + 1) x (d + 1) block of every pair."""
    delta, (k, g, w, _), l = _pairs(x1, x2, ls)
    n, m, d = delta.shape
    blk = torch.zeros(n, d + 1, m, d + 1, dtype=torch.float64)
    blk[:, 0, :, 0] = k
    for b in range(d):
        blk[:, 0, :, 1 + b] = g * delta[..., b] / l[b]
        blk[:, 1 + b, :, 0] = -g * delta[..., b] / l[b]
        for a in range(d):
            blk[:, 1 + a, :, 1 + b] = (g * (1.0 if a == b else 0.0) - w * delta[..., a] * delta[..., b]) / (l[a] * l[b])
    return blk.reshape(n * (d + 1), m * (d + 1))


def diag(x, ls):
    d = x.shape[-1]
    return torch.cat([torch.ones(x.shape[0], 1, dtype=torch.float64), ((5.0 / 3.0) / _ls(ls, d).pow(2)).expand(x.shape[0], d)], -1).reshape(-1)


def matvec(x1, x2, ls, V):
    """K @ V for V [m (d + 1), t] by the product formulas (never forms K); [n (d + 1), t] in float64."""
    delta, (k, g, w, _), l = _pairs(x1, x2, ls)
    n, m, d = delta.shape
    r = V.double().reshape(m, d + 1, -1)
    r0, rt = r[:, 0], r[:, 1:] / l.reshape(1, d, 1)                                 # [m, t], [m, d, t]
    Bv = torch.einsum("ijb,jbt->ijt", delta, rt)                                    # [n, m, t]
    out0 = torch.einsum("ij,jt->it", k, r0) + torch.einsum("ij,ijt->it", g, Bv)
    h = g.unsqueeze(-1) * r0.unsqueeze(0) + w.unsqueeze(-1) * Bv
    outa = (torch.einsum("ij,jat->iat", g, rt) - torch.einsum("ija,ijt->iat", delta, h)) / l.reshape(1, d, 1)
    return torch.cat([out0.unsqueeze(1), outa], 1).reshape(n * (d + 1), -1)


def sums(x1, x2, ls, L, R):
    """The 1 + d sums G over all pairs and all columns for L [n (d + 1), t], R [m (d + 1), t] (module docstring)."""
    delta, (k, g, w, u), l = _pairs(x1, x2, ls)
    n, m, d = delta.shape
    lv, rv = L.double().reshape(n, d + 1, -1), R.double().reshape(m, d + 1, -1)
    lt, rt = lv[:, 1:] / l.reshape(1, d, 1), rv[:, 1:] / l.reshape(1, d, 1)
    l0, r0 = lv[:, 0].unsqueeze(1), rv[:, 0].unsqueeze(0)                           # [n, 1, t], [1, m, t]
    A = torch.einsum("ijb,ibt->ijt", delta, lt)
    Bv = torch.einsum("ijb,jbt->ijt", delta, rt)
    C = torch.einsum("ibt,jbt->ijt", lt, rt)
    M = l0 * Bv - r0 * A + C
    k, g, w, u = (t.unsqueeze(-1) for t in (k, g, w, u))
    out = [(k * l0 * r0 + g * M - w * A * Bv).sum()]
    for a in range(d):
        da = delta[..., a].unsqueeze(-1)
        la, ra = lt[:, a].unsqueeze(1), rt[:, a].unsqueeze(0)
        out.append(-(da.pow(2) * (g * l0 * r0 + w * M - u * A * Bv) - 2.0 * g * (da * (l0 * ra - r0 * la) + la * ra)
                     + 2.0 * w * da * (la * Bv + ra * A)).sum())
    return torch.stack(out)


def hyper_grads(sums_, ls, outputscale=1.0):
    """(d/d lengthscale [1 or d values, in the shape of ``ls``], d/d outputscale) of outputscale * sum_c l_c^T K r_c from the sums."""
    ls_t = torch.as_tensor(ls).double()
    g = -outputscale * sums_[1:] / _ls(ls, sums_.numel() - 1)
    return (g.sum().reshape(ls_t.shape) if ls_t.numel() == 1 else g.reshape(ls_t.shape)), sums_[0]
