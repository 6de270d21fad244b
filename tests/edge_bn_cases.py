"""Inputs, the float64 reference and the rounding bounds of the BatchNorm + ReLU + max tests (tests/test_edge_bn_cpu.py,
tests/test_gpu_edge_bn.py): plain torch in float64, nothing of the op layer.

z (B, C, k, N), M = B k N values per channel; the reference is relu(F.batch_norm(z, ...)) and .max(dim=2):

    batch statistics:   mean = sum z / M,  var = sum (z - mean)^2 / M (biased),  invstd = 1 / sqrt(var + eps)
    running statistics: mean = running_mean,  var = running_var
    xhat = (z - mean) invstd,  y = gamma xhat + beta,  r = relu(y),  pooled = max_j r
    g_y = (g_r + [j == arg] g_pool) (y > 0),  gbeta = sum g_y,  ggamma = sum g_y xhat
    gz = gamma invstd (g_y - gbeta / M - xhat ggamma / M)      (running statistics: gamma invstd g_y)

The backward reference takes the mask y > 0 and arg from the kernel's own forward (r > 0 and its arg) once those are checked
-- arg points at a maximal element of the kernel's r, it is the lowest such j, r is within its bound -- so a float32 /
float64 disagreement about the sign of a y next to 0 or about two nearly equal maxima excludes no element from any check.

Input families, offset + spread * randn: (0, 1); (3, 1); (1000, 1) -- a one-pass variance E[z^2] - mean^2 loses its digits
there; (0, 1e-3) -- var is 0.1 of eps, so eps outside the root shows.

Bounds: |got - ref| <= t * u * mag elementwise, u = 2^-24.  Per channel mbar = mean |z|, std = sqrt(var),
kappa = 1 + mbar / std:

    mag_y      = |gamma| invstd ((|z| + mbar) + |z - mean| (1 + 2 mbar / std)) + |beta|
    mag_gz     = kappa |gamma| invstd (|g_y| + sum |g_y| / M + (|xhat| + 1) sum |g_y xhat| / M)
    mag_ggamma = kappa sum |g_y xhat|,      mag_gbeta = sum |g_y|
    mag_mean = mbar,  mag_var = var (1 + 2 mbar / std),  mag_invstd = invstd (1 + 2 mbar / std)

t.  The kernels add in double (a lane's values, wave_sum's six levels, the workgroup's waves, then the B slabs in order):
their longest chain, the 128 float4 a lane of the backward sums meets in the (1, 2, 64, 1028) slab plus 6 + 8 + B steps, is
under 600 roundings of 2^-53 on the sum of the magnitudes, 1e-6 of u.  No summation enters t; what does is the float32 roundings of one element, 0.5 u
each, counted against the term of mag they act on:
  y       the mean rounded to float32 and the subtraction z - mean: 0.5 + 0.5 on (|z| + mbar); invstd rounded to float32
          (0.5), eps taken as float32 (0.25 on var + eps at most), gamma * invstd (0.5) and the fma's rounding (0.5) on
          |z - mean| (..) and |beta|: 1.75 at most on any term.  T_Y = 2.  The statistics are held to the same 2 (one
          rounding each, 0.5, and eps's 0.25).
  gbeta   g_r + g_pool (0.5 per term) and the sum's rounding to float32 (0.5).  T_GBETA = 2.
  ggamma  per product: g_y (0.5), xhat (z - mean, invstd's own rounding and eps, the product with invstd: 1.75), g_y * xhat
          (0.5), the sum's rounding (0.5): 3.25 on sum |g_y xhat|; and the float32 mean's rounding delta <= 0.5 u mbar, the
          SAME for every element, which moves ggamma by delta invstd sum g_y <= 0.5 u (kappa - 1) sum |g_y| -- covered by
          kappa sum |g_y xhat| as long as sum |g_y| <= 9 sum |g_y xhat|, which xhat's unit variance gives every case here
          (reference() reports the ratio).  T_GGAMMA = 8.
  gz      |g_y|: its own rounding, the two subtractions, gamma * invstd (1.25) and the last product: 3.25.  sum |g_y| / M:
          the sum over M as gbeta's (1.0), the subtractions and the products (2.75), and through xhat * (ggamma / M) the
          common delta again, 0.5 max |xhat|, under 3.5 with max |xhat| < 7 (randn over at most 1.4e5 values).
          (|xhat| + 1) sum |g_y xhat| / M: xhat (1.75 relative, 0.5 absolute: the + 1), ggamma / M (3.25 + 0.5), the
          product, the subtraction, gamma * invstd and the last product (2.75): 8.75.  T_GZ = 12.
The float32 composition in torch (the parent's route) stays within these bounds at the CPU tests' shapes
(tests/test_edge_bn_cpu.py prints its shares and asserts them); a one-pass variance, an unbiased batch variance, eps outside
the root, a missing mean term in gz and a mask taken from g instead of y each miss them by far."""
import torch

U = 2.0 ** -24
T_Y, T_GZ, T_GGAMMA, T_GBETA = 2, 12, 8, 2
EPS = 1e-5
MOMENTUM = 0.1
FAMILIES = [(0.0, 1.0), (3.0, 1.0), (1000.0, 1.0), (0.0, 1e-3)]
# the last two: k n / 4 = 5120 is the longest slab the statistics kernel holds in registers, 5140 the first it reads twice
SHAPES = [(1, 1, 1, 4), (2, 3, 20, 8), (3, 5, 7, 68), (2, 64, 20, 260), (1, 2, 64, 1028), (2, 2, 20, 1024), (2, 2, 20, 1028)]


def make_case(shape, family, seed=11):
    """-> dict of float32 CPU tensors: z, g_r (B,C,k,N), g_pool (B,C,N), gamma, beta, running_mean, running_var (C).  The
    running statistics lie near the family's own (mean within 0.1 spread, variance within 0.5 .. 1.5 spread^2)."""
    B, C, k, N = shape
    offset, spread = family
    gen = torch.Generator().manual_seed(seed + 7919 * B + 131 * C + 17 * k + N + 1000003 * FAMILIES.index(family))
    r = lambda *s: torch.randn(*s, generator=gen)
    return {"z": (offset + spread * r(B, C, k, N)).float(), "g_r": r(B, C, k, N), "g_pool": r(B, C, N),
            "gamma": r(C), "beta": 0.5 * r(C),
            "running_mean": (offset + 0.1 * spread * r(C)).float(),
            "running_var": (spread * spread * (0.5 + torch.rand(C, generator=gen))).float()}


def _v(t):
    return t.view(1, -1, 1, 1)


def reference(z, gamma, beta, eps=EPS, running=None):
    """float64 forward results and magnitudes; running = (running_mean, running_var) or None for batch statistics."""
    z, gamma, beta = (t.detach().cpu().double() for t in (z, gamma, beta))
    M = z.numel() // z.shape[1]
    if running is None:
        mean = z.mean(dim=(0, 2, 3))
        var = ((z - _v(mean)) ** 2).sum(dim=(0, 2, 3)) / M
    else:
        mean, var = (t.detach().cpu().double() for t in running)
    invstd = 1 / torch.sqrt(var + eps)
    std = torch.sqrt(var)
    mbar = z.abs().mean(dim=(0, 2, 3))
    ratio = mbar / std
    xhat = (z - _v(mean)) * _v(invstd)
    y = xhat * _v(gamma) + _v(beta)
    r = torch.relu(y)
    mag_y = _v(gamma.abs() * invstd) * ((z.abs() + _v(mbar)) + (z - _v(mean)).abs() * _v(1 + 2 * ratio)) + _v(beta.abs())
    return {"M": M, "mean": mean, "var": var, "invstd": invstd, "std": std, "mbar": mbar, "kappa": 1 + ratio, "xhat": xhat,
            "y": y, "r": r, "pooled": r.max(dim=2)[0], "mag_y": mag_y, "mag_pooled": mag_y.max(dim=2)[0],
            "mag_mean": mbar, "mag_var": var * (1 + 2 * ratio), "mag_invstd": invstd * (1 + 2 * ratio),
            "gamma": gamma, "beta": beta, "batch": running is None}


def reference_backward(fwd, mask, arg, g_r=None, g_pool=None):
    """float64 gradients and magnitudes from reference()'s dict, the mask y > 0 (bool, (B,C,k,N)) and arg (B,C,N)."""
    xhat, gamma, invstd, M = fwd["xhat"], fwd["gamma"], fwd["invstd"], fwd["M"]
    g = torch.zeros_like(xhat) if g_r is None else g_r.detach().cpu().double().clone()
    if g_pool is not None:
        g.scatter_add_(2, arg.cpu().long().unsqueeze(2), g_pool.detach().cpu().double().unsqueeze(2))
    g_y = torch.where(mask.cpu(), g, torch.zeros_like(g))
    s = lambda t: t.sum(dim=(0, 2, 3))
    gbeta, ggamma = s(g_y), s(g_y * xhat)
    a_beta, a_gamma = s(g_y.abs()), s((g_y * xhat).abs())
    w = _v(gamma * invstd)
    gz = w * (g_y - _v(gbeta) / M - xhat * _v(ggamma) / M) if fwd["batch"] else w * g_y
    mag_gz = _v(fwd["kappa"]) * w.abs() * (g_y.abs() + _v(a_beta) / M + (xhat.abs() + 1) * _v(a_gamma) / M)
    return {"gz": gz, "ggamma": ggamma, "gbeta": gbeta, "mag_gz": mag_gz, "mag_ggamma": fwd["kappa"] * a_gamma,
            "mag_gbeta": a_beta, "g_y": g_y,
            "abs_ratio": float((a_beta / a_gamma.clamp_min(1e-300)).max()) if bool((a_gamma > 0).any()) else 0.0}


def share(got, want, mag, t):
    """The largest |got - want| / (t u mag) over the elements; an element whose bound is 0 has to be exact."""
    err = (got.detach().cpu().double() - want).abs()
    bound = t * U * mag
    assert bool((err[bound == 0] == 0).all())
    return float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0


def compose(z, gamma, beta, running_mean, running_var, training, eps=EPS, momentum=MOMENTUM):
    """The parent's route op for op at the tensors' own dtype: -> (r, pooled, arg)."""
    r = torch.relu(torch.nn.functional.batch_norm(z, running_mean, running_var, gamma, beta, training, momentum, eps))
    pooled, arg = r.max(dim=2)
    return r, pooled, arg
