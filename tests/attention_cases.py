"""What the attention tests share (tests/test_attention_cpu.py, tests/test_gpu_attention.py): the shapes, the input families,
the float64 reference with its elementwise error bound, and the two families whose result is known exactly.  Plain torch on
the CPU, nothing of the op layer.

Tensors are made "by head", (B, H, N, D); packed(t) is the (B, N, H * D) layout of the projections that the operator and
the C entry point take, by_head(t, H) its inverse.

The bound, elementwise and to first order, for any tile size >= 32 and any summation order; u = 2^-24, T = ceil(Nk / 32),
s, m_i = max_j s_ij and p = softmax(s) in float64:
    E_ij     = (D + 2) u scale sum_c |q_ic| |k_jc|                      the score's fmaf chain and the scale
    rho_ij   = E_ij + (2 |s_ij - m_i| + 3 T + 6) u                      the exponent's argument, one rescale chain (it
                                                                        telescopes to at most |s_ij - m_i|), the exponential
    rhobar_i = sum_j p_ij rho_ij + Nk u                                 the row sum
    bound_ic = sum_j p_ij (rho_ij + rhobar_i + (Nk + 2) u) |v_jc|       the output sums
(the error of the row maximum cancels between numerator and denominator).  share = max |got - ref| / bound must be <= 1."""
import math

import torch

U = 2.0 ** -24

# (B, H, Nq, Nk, D)
SHAPES = (
    (1, 1, 1, 1, 32),          # degenerate
    (2, 4, 64, 64, 128),       # DCP's heads at the golden clouds' 64 points
    (1, 2, 33, 70, 32),        # partial tiles on both axes
    (2, 1, 5, 200, 96),        # a width that is no power of two
    (1, 1, 257, 96, 64),       # one row past a 256-row block
    (1, 1, 40, 1024, 128),     # cfg 5's key count, many rescales
)
FAMILIES = ("random", "peaked", "shifted", "tied")
EXACT_FAMILIES = ("flat", "one_hot")


def shape_id(shape):
    return "x".join(map(str, shape))


def packed(t):
    """(B, H, N, D) -> (B, N, H * D), contiguous."""
    b, h, n, d = t.shape
    return t.transpose(1, 2).reshape(b, n, h * d).contiguous()


def by_head(t, heads):
    """(B, N, H * D) -> (B, H, N, D)."""
    b, n, hd = t.shape
    return t.reshape(b, n, heads, hd // heads).transpose(1, 2)


def default_scale(shape):
    return 1.0 / math.sqrt(shape[4])


def inputs(shape, family, seed=3):
    """q (B, H, Nq, D), k and v (B, H, Nk, D), float32, of one random family."""
    B, H, Nq, Nk, D = shape
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, H, Nq, D, generator=g)
    k = torch.randn(B, H, Nk, D, generator=g)
    v = torch.randn(B, H, Nk, D, generator=g)
    if family == "peaked":                      # near one-hot rows
        q = q * 8
    elif family == "shifted":                   # a large common offset that the maximum must remove
        q, k = q + 3.0, k + 3.0
    elif family == "tied":                      # key j = key j mod 2
        k = k[:, :, torch.arange(Nk) % 2, :].contiguous()
    else:
        assert family == "random", family
    return q, k, v


def reference(q, k, v, scale):
    """-> (softmax(scale q k^T) v, the bound), both float64 (B, H, Nq, D)."""
    D, Nk = q.shape[-1], k.shape[-2]
    T = math.ceil(Nk / 32)
    q, k, v = q.double(), k.double(), v.double()
    s = (q @ k.transpose(-1, -2)) * scale
    m = s.max(-1, keepdim=True)[0]
    p = torch.softmax(s, -1)
    E = (D + 2) * U * abs(scale) * (q.abs() @ k.abs().transpose(-1, -2))
    rho = E + (2 * (s - m).abs() + 3 * T + 6) * U
    rhobar = (p * rho).sum(-1, keepdim=True) + Nk * U
    bound = (p * (rho + rhobar + (Nk + 2) * U)) @ v.abs()
    return p @ v, bound


def share(got, ref, bound):
    """max |got - ref| / bound; inf where `got` is not finite."""
    err = (got.double() - ref).abs() / bound
    return float("inf") if not bool(torch.isfinite(err).all()) else float(err.max())


def composed(q, k, v, scale):
    """The module's five steps on by-head tensors in their own dtype (registration/models/dcp.py: MultiHeadedAttention)."""
    return torch.softmax(q @ k.transpose(-1, -2) / (1.0 / scale), -1) @ v


# ------------------------------------------------------------------------------------------------ the exact families

def exact_inputs(shape, family, seed=4):
    """-> (q, k, v, want): `want` (B, H, Nq, D) float64 is the exact result.
      flat     all keys of a (cloud, head) equal, v small integers in [-4, 4]: every weight is exactly 1 before the division,
               the sum exactly Nk, the output sum_j v_j / Nk.
      one_hot  k_j = e_(j mod D) for j < min(2 D, Nk), zero rows after; q_i = 256 sqrt(D) e_pi(i), pi random among the keys
               that exist; v small integers.  With scale = 1 / sqrt(D) the matching scores are 256 and all others 0, whose
               weights underflow to exactly 0 in float32: out_i = the mean of the matching rows, (v_pi + v_(pi + D)) / 2 when
               both exist."""
    B, H, Nq, Nk, D = shape
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(-4, 5, (B, H, Nk, D), generator=g).float()
    if family == "flat":
        q = torch.randn(B, H, Nq, D, generator=g)
        k = torch.randn(B, H, 1, D, generator=g).expand(B, H, Nk, D).contiguous()
        want = (v.double().sum(-2, keepdim=True) / Nk).expand(B, H, Nq, D)
        return q, k, v, want
    assert family == "one_hot", family
    live = min(2 * D, Nk)
    k = torch.zeros(B, H, Nk, D)
    j = torch.arange(live)
    k[:, :, j, j % D] = 1.0
    pi = torch.randint(0, min(D, Nk), (B, H, Nq), generator=g)
    q = torch.zeros(B, H, Nq, D)
    q.scatter_(3, pi.unsqueeze(3), 256.0 * math.sqrt(D))
    first = torch.gather(v, 2, pi.unsqueeze(3).expand(B, H, Nq, D)).double()
    second_at = pi + D
    has_second = (second_at < live).unsqueeze(3)
    second = torch.gather(v, 2, second_at.clamp(max=Nk - 1).unsqueeze(3).expand(B, H, Nq, D)).double()
    want = torch.where(has_second, (first + second) / 2, first)
    return q, k, v, want


def ulps_off(got, want):
    """max |got - want| in units of the float32 ulp of `want` (the spacing of float32 at |want|; at 0, the smallest normal's)."""
    want32 = want.float().double().abs().clamp_min(2.0 ** -126)
    ulp = torch.exp2(torch.floor(torch.log2(want32)) - 23)
    off = (got.double() - want).abs() / ulp
    return float("inf") if not bool(torch.isfinite(off).all()) else float(off.max())


def assert_exact(got, want, family):
    """flat: within 2 ulp of sum_j v_j / Nk; one_hot: equal to the bit."""
    if family == "flat":
        assert ulps_off(got, want) <= 2.0, ulps_off(got, want)
    else:
        assert torch.equal(got.double(), want), float((got.double() - want).abs().max())


# ------------------------------------------------------------------------------------ a 32-key online softmax in float32

def tiled(q, k, v, scale, tile=32, drop_last_key=False):
    """The kernel's scheme in torch float32 (not its bits): tiles of `tile` keys, running maximum and sum, exp2 of the
    difference times log2 e."""
    if drop_last_key:
        k, v = k[..., :-1, :], v[..., :-1, :]
    Nk = k.shape[-2]
    m = torch.full(q.shape[:-1] + (1,), -float("inf"))
    l = torch.zeros_like(m)
    o = torch.zeros(q.shape[:-1] + (v.shape[-1],))
    c = torch.tensor(math.log2(math.e), dtype=torch.float32)
    sc = torch.tensor(scale, dtype=torch.float32)
    for j in range(0, Nk, tile):
        s = (q @ k[..., j:j + tile, :].transpose(-1, -2)) * sc
        mn = torch.maximum(m, s.max(-1, keepdim=True)[0])
        a, p = torch.exp2((m - mn) * c), torch.exp2((s - mn) * c)
        l = l * a + p.sum(-1, keepdim=True)
        o = o * a + p @ v[..., j:j + tile, :]
        m = mn
    return o / l
