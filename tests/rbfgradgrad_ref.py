"""Float64 restatement of the RBF kernel with first- and second-derivative observations, written from the Hermite formula as plain loops over the
components (the oracle of tests/test_rbfgradgrad_cpu.py and tests/test_gpu_rbfgradgrad.py; no project code).

A point has C = 2 d + 1 components: the value (c = 0), d/dx_a (c = a, 1 <= a <= d) and d2/dx_a^2 (c = d + a); row i C + c is component c of point i.
A component's derivative orders are alpha = 0, e_a or 2 e_a.  With u_q = (x_iq - x_jq) / l_q, k = exp(-|u|^2 / 2) and the probabilists' Hermite
polynomials He_n (He_0 = 1, He_1 = u, He_{n+1} = u He_n - n He_{n-1}):

    K[(i, alpha), (j, beta)] = k prod_q (-1)^{alpha_q} He_{alpha_q + beta_q}(u_q) / l_q^{alpha_q + beta_q}

Lengthscale derivative: dK/dl_a is (1 / l_a) times the same block with He_s(u_a), s = alpha_a + beta_a, replaced by He_{s+2}(u_a) + He_s(u_a).

x: [n, d]; ls: 1 or d values (any shape)."""
import torch


def _ls(ls, d):
    ls = torch.as_tensor(ls).double().reshape(-1)
    return ls.expand(d) if ls.numel() == 1 else ls


def hermite(n, u):
    """He_n(u) by the recurrence."""
    a, b = torch.ones_like(u), u
    if n == 0:
        return a
    for k in range(1, n):
        a, b = b, u * b - k * a
    return b


def orders(c, d):
    """The derivative orders [d] of component c."""
    o = [0] * d
    if 1 <= c <= d:
        o[c - 1] = 1
    elif c > d:
        o[c - d - 1] = 2
    return o


def _u_k(x1, x2, ls):
    d = x1.shape[-1]
    l = _ls(ls, d)
    u = x1.double().unsqueeze(1) / l - x2.double().unsqueeze(0) / l
    return u, torch.exp(-0.5 * u.pow(2).sum(-1)), l


def pair_covariances(x1, x2, ls):
    """k [n, m]: what the tests' guard on the share of mixed pairs looks at."""
    return _u_k(x1, x2, ls)[1]


def dense(x1, x2, ls, shifted=None):
    """K [n C, m C] in float64, entry by entry.  ``shifted``: a dimension a -- the block with He_s(u_a) replaced by He_{s+2}(u_a) + He_s(u_a)."""
    u, k, l = _u_k(x1, x2, ls)
    n, m, d = u.shape
    C = 2 * d + 1
    blk = torch.zeros(n, C, m, C, dtype=torch.float64)
    He = [[hermite(s, u[..., q]) for s in range(7)] for q in range(d)]      # He[q][s] = He_s(u_q), once for all components
    for ca in range(C):
        al = orders(ca, d)
        for cb in range(C):
            be = orders(cb, d)
            e = k
            for q in range(d):
                s = al[q] + be[q]
                if s == 0 and shifted != q:
                    continue                                                 # He_0 = 1
                h = He[q][s + 2] + He[q][s] if shifted == q else He[q][s]
                e = e * (-1.0) ** al[q] * h / l[q] ** s
            blk[:, ca, :, cb] = e
    return blk.reshape(n * C, m * C)


def diag(x, ls):
    """1, 1 / l_a^2, 3 / l_a^4 per point."""
    d = x.shape[-1]
    l = _ls(ls, d)
    return torch.cat([torch.ones(1, dtype=torch.float64), 1.0 / l.pow(2), 3.0 / l.pow(4)]).repeat(x.shape[0])


def sums(x1, x2, ls, L, R):
    """The 1 + d sums of the fused derivative kernel for L [n C, t], R [m C, t]: [sum l^T K r | -sum l^T K^(a) r per dimension]
    (d/dl_a = -outputscale sums[1 + a] / l_a)."""
    d = x1.shape[-1]
    out = [(L.double() * (dense(x1, x2, ls) @ R.double())).sum()]
    for a in range(d):
        out.append(-(L.double() * (dense(x1, x2, ls, shifted=a) @ R.double())).sum())
    return torch.stack(out)
