"""Inputs, the float64 reference and the rounding bounds of the LayerNorm tests (tests/test_layer_norm_cpu.py,
tests/test_gpu_layer_norm.py): plain torch in float64, nothing of the op layer.

Per row of d values z (= x + delta rounded to float32 once, or x), eps added to the UNBIASED std:

    mean = sum(z) / d,  c = z - mean,  std = sqrt(sum(c c) / (d - 1)),  U = 1 / (std + eps),  y = a c U + b
    gh = gy a,  gz = U (gh - mean gh) - c (sum gh c) U^2 / ((d - 1) std)  [+ gres],  ga = sum_r gy c U,  gb = sum_r gy
    (the second term of gz is 0 where std == 0: torch's std backward masks a zero std)

Input families, each row offset + spread * randn: (0, 1); (3, 1); (1000, 1) -- a one-pass variance E[z^2] - mean^2 loses
all its digits there; (0, 1e-3) -- std is comparable to nothing but eps * 1000, so eps inside the square root, U^3 in
place of U^2 / std and a biased std all show.

Bounds: |got - ref| <= t * u * mag elementwise, u = 2^-24.  With mbar = mean |z| of the row and kappa = 1 + mbar / std:

  mag_y  = |a| / (std + eps) * ((|z_i| + mbar) + |c_i| (1 + 2 mbar / std)) + |b|
           c_i = z_i - mean carries an absolute error of u (|z_i| + mbar) per rounding of the mean's sum; std a relative
           error of kappa-like size (1 + 2 mbar / std per rounding: each c_j is off by u mbar, of std's own size times
           mbar / std), which reaches y through |c_i| U.
  mag_gz = kappa * (U (|gh_i| + mean |gh|) + (|c_i| + std) * sum_j |gh_j c_j| * U^2 / ((d - 1) std))   [+ |gres_i|]
           every factor that comes from z (c, std, U) is off by a relative kappa u per rounding; the sums by u times the
           sums of the magnitudes.  With gres the last float add rounds once more on |gz| + |gres_i| <= mag + |gres_i|.
  mag_ga = sum_r |gy c U| kappa_r,     mag_gb = sum_r |gy|

t = 32 for y and gz: the longest chain of a one-wave-per-row kernel at d <= 1024 is 16 serial additions in a lane and 6
tree levels (22 roundings on a sum's magnitude), and under ten elementary roundings around it.  t = rows + 8 for ga and gb:
rows - 1 additions in any order, and the product's roundings.
mag_ga has no absolute term: it asks for every product gy c U to a RELATIVE kappa u, also where c_i is small next to std.
A centred value formed in float32 from a float32 mean carries the mean's rounding, an absolute u mbar, so over few rows the
float32 composition misses this bound (measured at the GPU tests' shapes: up to 600 times at rows = 1, 2.9 at rows = 3, 1.8
at rows = 4; inside it from rows = 5, at 1e-3 of it at rows = 257).  The kernel's backward pass meets it at every shape
because it re-centres z on the mean taken to double (csrc/layer_norm.hip); the bound stays as it is.
A row with std == 0 has no kappa.  Such rows appear only in the constant-row tests, whose values (0, and 3 at a d that is a
power of two) make every sum over z exact, so c = 0 and std = 0 exactly, in float32 as in float64: there kappa counts as 1,
the second term of gz is 0 and only the sums over gh round.

The float32 composition in torch (the parent's route) stays at or below 1.6 of u * mag in every family at d = 4, 8, 60, 512
(tests/test_layer_norm_cpu.py asserts 2), so t = 32 hides nothing; a biased std, a one-pass variance, eps inside the square
root, a missing mean term, d in place of d - 1 and U^3 in place of U^2 / std each exceed 1e3 of u * mag in some family."""
import torch

U = 2.0 ** -24
T_ROW = 32
EPS = 1e-6
FAMILIES = [(0.0, 1.0), (3.0, 1.0), (1000.0, 1.0), (0.0, 1e-3)]
ROWS = (1, 3, 4, 5, 257)
DIMS = (4, 8, 60, 256, 512, 1024)


def t_cols(rows):
    return rows + 8


def make_case(rows, d, family, seed=3):
    """-> dict of float32 CPU tensors: x, delta (rows, d), a, b (d), gy, gres (rows, d).  x + delta keeps the family's offset
    (delta is centred on 0 with the family's spread)."""
    offset, spread = family
    gen = torch.Generator().manual_seed(seed + 7919 * rows + 31 * d + FAMILIES.index(family))
    r = lambda *s: torch.randn(*s, generator=gen)
    return {"x": (offset + spread * r(rows, d)).float(), "delta": (spread * r(rows, d)).float(), "a": r(d), "b": r(d),
            "gy": r(rows, d), "gres": r(rows, d)}


def reference(z, a, b, gy, gres=None, eps=EPS):
    """float64 results and magnitudes for float32 (or float64) inputs; z is what is normalised."""
    z, a, b, gy = (t.detach().cpu().double() for t in (z, a, b, gy))
    d = z.shape[-1]
    mean = z.mean(-1, keepdim=True)
    c = z - mean
    std = torch.sqrt((c * c).sum(-1, keepdim=True) / (d - 1))
    flat = std == 0
    safe = torch.where(flat, torch.ones_like(std), std)
    Uu = 1 / (std + eps)
    mbar = z.abs().mean(-1, keepdim=True)
    ratio = torch.where(flat, torch.zeros_like(std), mbar / safe)
    kappa = 1 + ratio
    y = a * c * Uu + b
    mag_y = a.abs() * Uu * ((z.abs() + mbar) + c.abs() * (1 + 2 * ratio)) + b.abs()
    gh = gy * a
    coef = torch.where(flat, torch.zeros_like(std), (gh * c).sum(-1, keepdim=True) * Uu * Uu / ((d - 1) * safe))
    gz = Uu * (gh - gh.mean(-1, keepdim=True)) - c * coef
    mag_coef = torch.where(flat, torch.zeros_like(std), (gh * c).abs().sum(-1, keepdim=True) * Uu * Uu / ((d - 1) * safe))
    mag_gz = kappa * (Uu * (gh.abs() + gh.abs().mean(-1, keepdim=True)) + (c.abs() + std) * mag_coef)
    if gres is not None:
        gres = gres.detach().cpu().double()
        gz = gz + gres
        mag_gz = mag_gz + gres.abs()
    return {"y": y, "gz": gz, "ga": (gy * c * Uu).sum(0), "gb": gy.sum(0), "mean": mean, "std": std, "U": Uu,
            "mag_y": mag_y, "mag_gz": mag_gz, "mag_ga": ((gy * c * Uu).abs() * kappa).sum(0), "mag_gb": gy.abs().sum(0)}


def share(got, want, mag, t):
    """The largest |got - want| / (t u mag) over the elements; an element whose bound is 0 has to be exact."""
    err = (got.detach().cpu().double() - want).abs()
    bound = t * U * mag
    assert bool((err[bound == 0] == 0).all())
    return float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0


def compose(z, a, b, eps=EPS):
    """The module's formula op for op, at the tensors' own dtype."""
    centred = z - z.mean(-1, keepdim=True)
    return a * centred / (z.std(-1, keepdim=True) + eps) + b
