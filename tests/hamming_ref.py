"""Float64 oracle of the inverse-multiquadric Hamming covariance, written from the formula (not from the library, not from the reference's code):

    k(x, x') = ((1 + alpha) / (alpha + c))^beta = k0 (1 + c / alpha)^(-beta),   c = the number of positions in which the two sequences differ,

on TOKENS (integer tensors [n, T]); ``one_hot`` makes the flattened encoding ``gpytorch/kernels/hamming_kernel.py`` takes, ``tokens`` undoes it."""
import torch


def one_hot(tok, vocab_size, dtype=torch.float32):
    """[n, T] integer tokens -> [n, T V] one-hot rows in ``dtype``."""
    return torch.nn.functional.one_hot(tok.long(), vocab_size).reshape(tok.shape[0], -1).to(dtype)


def random_tokens(n, t, vocab_size, seed, close_to=None, flips=2):
    """Seeded [n, T] tokens; with ``close_to`` ([k, T]) the first min(n, k) rows are copies of it with at most ``flips`` positions redrawn, so that small
    distances (and c = 0) occur between the two clouds."""
    g = torch.Generator().manual_seed(seed)
    tok = torch.randint(0, vocab_size, (n, t), generator=g)
    if close_to is not None:
        k = min(n, close_to.shape[0])
        tok[:k] = close_to[:k]
        for f in range(flips):
            rows = torch.arange(f, k, flips + 1)          # every (flips + 1)-th row keeps an exact copy
            pos = torch.randint(0, t, (rows.numel(),), generator=g)
            tok[rows, pos] = torch.randint(0, vocab_size, (rows.numel(),), generator=g)
    return tok


def tokens(x, vocab_size):
    """[n, T V] one-hot rows -> [n, T] tokens (argmax per position)."""
    return x.detach().cpu().reshape(x.shape[0], -1, vocab_size).argmax(-1)


def hamming_counts(tok1, tok2=None):
    """c [n, m] as float64 on the CPU."""
    tok1 = tok1.detach().cpu()
    tok2 = tok1 if tok2 is None else tok2.detach().cpu()
    return (tok1.unsqueeze(1) != tok2.unsqueeze(0)).sum(-1).to(torch.float64)


def hamming_kt(c, alpha, beta):
    """k~ = (1 + c / alpha)^(-beta) in float64 (autograd-visible in alpha and beta)."""
    return (1.0 + c / alpha).pow(-beta)


def hamming_k(c, alpha, beta):
    """k = ((1 + alpha) / (alpha + c))^beta in float64 (autograd-visible in alpha and beta)."""
    return ((1.0 + alpha) / (alpha + c)).pow(beta)


def f64(v):
    return torch.as_tensor(v).detach().to(device="cpu", dtype=torch.float64)


def hamming_grad_sums(c, alpha, beta, W):
    """(G0, Gs, Gb) in float64: G0 = sum W k~, Gs = sum W s dk~/ds at s = c / alpha, Gb = sum W dk~/dbeta at fixed s -- closed forms."""
    c, alpha, beta, W = f64(c), f64(alpha), f64(beta), f64(W)
    s = c / alpha
    kt = (1.0 + s).pow(-beta)
    return torch.stack([(W * kt).sum(), (W * kt * (-beta * s / (1.0 + s))).sum(), (W * kt * (-torch.log1p(s))).sum()])
