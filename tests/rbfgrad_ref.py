"""Float64 restatement of the RBF kernel with derivative observations, written from the formulas (the oracle of tests/test_rbfgrad_cpu.py and
tests/test_gpu_rbfgrad.py; no project code).

Interleaved ordering: row i (d + 1) + a is component a of point i, a = 0 the value, a = 1..d the partial derivatives.  With z = x / l per
dimension, delta = z_i - z_j, k = exp(-|delta|^2 / 2) and r~_b = r_b / l_b for a right-hand side r with per-point components (r_0, r_1..r_d):

    q_ij   = r_j0 + delta . r~_j
    out_i0 = sum_j k q_ij
    out_ia = (1 / l_a) sum_j k (r~_ja - delta_a q_ij)

and for a left vector l (l~_a = l_a / lengthscale_a), p_ij = l_i0 - delta . l~_i, f_ij = p q + l~_i . r~_j:

    l^T K r = sum_ij k f_ij
    d(l^T K r) / d lengthscale_a = -(1 / lengthscale_a) sum_ij k [ -delta_a^2 f + 2 delta_a (p r~_ja - l~_ia q) + 2 l~_ia r~_ja ]

x: [n, d]; ls: 1 or d values (any shape)."""
import torch


def _ls(ls, d):
    ls = torch.as_tensor(ls).double().reshape(-1)
    return ls.expand(d) if ls.numel() == 1 else ls


def _pairs(x1, x2, ls):
    d = x1.shape[-1]
    l = _ls(ls, d)
    delta = x1.double().unsqueeze(1) / l - x2.double().unsqueeze(0) / l          # [n, m, d]
    return delta, torch.exp(-0.5 * delta.pow(2).sum(-1)), l


def rbfgrad_dense(x1, x2, ls):
    """K [n (d + 1), m (d + 1)] in float64: the (d + 1) x (d + 1) block of every pair read off the product formulas above."""
    delta, k, l = _pairs(x1, x2, ls)
    n, m, d = delta.shape
    blk = torch.zeros(n, d + 1, m, d + 1, dtype=torch.float64)
    blk[:, 0, :, 0] = k
    for b in range(d):
        blk[:, 0, :, 1 + b] = k * delta[..., b] / l[b]
        blk[:, 1 + b, :, 0] = -k * delta[..., b] / l[b]
        for a in range(d):
            blk[:, 1 + a, :, 1 + b] = k * ((1.0 if a == b else 0.0) - delta[..., a] * delta[..., b]) / (l[a] * l[b])
    return blk.reshape(n * (d + 1), m * (d + 1))


def rbfgrad_diag(x, ls):
    d = x.shape[-1]
    return torch.cat([torch.ones(x.shape[0], 1, dtype=torch.float64), (1.0 / _ls(ls, d).pow(2)).expand(x.shape[0], d)], -1).reshape(-1)


def rbfgrad_matvec(x1, x2, ls, V):
    """K @ V for V [m (d + 1), t] by the product formulas (never forms K); [n (d + 1), t] in float64."""
    delta, k, l = _pairs(x1, x2, ls)
    n, m, d = delta.shape
    r = V.double().reshape(m, d + 1, -1)
    rt = r[:, 1:] / l.reshape(1, d, 1)                                              # [m, d, t]
    q = r[:, 0].unsqueeze(0) + torch.einsum("ijb,jbt->ijt", delta, rt)              # [n, m, t]
    out0 = torch.einsum("ij,ijt->it", k, q)
    outa = (torch.einsum("ij,jat->iat", k, rt) - torch.einsum("ij,ija,ijt->iat", k, delta, q)) / l.reshape(1, d, 1)
    return torch.cat([out0.unsqueeze(1), outa], 1).reshape(n * (d + 1), -1)


def rbfgrad_sums(x1, x2, ls, L, R):
    """The 1 + d sums over all pairs and all columns for L [n (d + 1), t], R [m (d + 1), t]:
        G[0] = sum k f,    G[1 + a] = sum k [ -delta_a^2 f + 2 delta_a (p r~_a - l~_a q) + 2 l~_a r~_a ]."""
    delta, k, l = _pairs(x1, x2, ls)
    n, m, d = delta.shape
    lv, rv = L.double().reshape(n, d + 1, -1), R.double().reshape(m, d + 1, -1)
    lt, rt = lv[:, 1:] / l.reshape(1, d, 1), rv[:, 1:] / l.reshape(1, d, 1)
    p = lv[:, 0].unsqueeze(1) - torch.einsum("ijb,ibt->ijt", delta, lt)
    q = rv[:, 0].unsqueeze(0) + torch.einsum("ijb,jbt->ijt", delta, rt)
    f = p * q + torch.einsum("ibt,jbt->ijt", lt, rt)
    g = [torch.einsum("ij,ijt->", k, f)]
    for a in range(d):
        da = delta[..., a].unsqueeze(-1)
        la, ra = lt[:, a].unsqueeze(1), rt[:, a].unsqueeze(0)
        g.append(torch.einsum("ij,ijt->", k, -da.pow(2) * f + 2.0 * da * (p * ra - la * q) + 2.0 * la * ra))
    return torch.stack(g)


def rbfgrad_hyper_grads(sums, ls, outputscale=1.0):
    """(d/d lengthscale [1 or d values, in the shape of ``ls``], d/d outputscale) of outputscale * sum_c l_c^T K r_c from the sums."""
    ls_t = torch.as_tensor(ls).double()
    g = -outputscale * sums[1:] / _ls(ls, sums.numel() - 1)
    return (g.sum().reshape(ls_t.shape) if ls_t.numel() == 1 else g.reshape(ls_t.shape)), sums[0]
