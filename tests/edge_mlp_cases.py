"""Cases and the independent reference of the edge-MLP tests (tests/test_edge_mlp_cpu.py, tests/test_gpu_edge_mlp.py): plain
torch with an explicit gather, nothing of the op layer.

Per cloud, point n, slot j, stage i = 1 .. s (K_1 = 2c, K_i = w_{i-1}):

    e_0[:, j] = [x[:, idx[j, n]] ; x[:, n]]
    e_i[:, j] = relu(scale_i * (W_i e_{i-1}[:, j]) + shift_i)
    out[off_i : off_i + w_i, n] = max_j e_i[:, j]

The bound of the random cases: |got - ref| <= t * 2^-24 * mag elementwise (first-order gamma_t; any summation order,
FMA or not), with

    t_0 = 0,  t_i = t_{i-1} + K_i + 2     K_i rounded multiply-adds, the affine map as at most two operations
    mag_0 = |e_0|,  mag_i = |scale_i| * (|W_i| mag_{i-1}) + |shift_i|

ReLU and the max over k add nothing (both are 1-Lipschitz, fmaf is monotone): the output's mag is the max over k of the
slots' mag.  `extra` roundings per stage are added to t_i where scale and shift are themselves rounded results (the module
test), with `shift_mags` in place of |shift|."""
import torch

U = 2.0 ** -24

DGCNN_WIDTHS = (64, 64, 128, 256)
# (B, c, n, k, widths): degenerate; DGCNN's widths with n * k no multiple of 32 and one partial tile; one point past a
# tile / wave boundary; the k limit; the widest first stage, the c limit and several tiles per cloud; a width that is no
# power of two
SHAPES = [(2, 3, 1, 1, (32,)), (2, 3, 50, 20, DGCNN_WIDTHS), (3, 3, 129, 5, (32,)), (1, 3, 70, 64, DGCNN_WIDTHS),
          (2, 4, 300, 16, (256, 32)), (2, 1, 67, 3, (32, 64, 96))]
PATTERNS = ["random", "one_point", "self", "point0"]


def fan_ins(c, widths):
    return [2 * c] + list(widths[:-1])


def make_idx(pattern, B, k, N, gen):
    """(B, k, N) int32 neighbour lists, all in [0, N)."""
    if pattern == "random":            # k distinct points per list (k <= N in every shape above)
        idx = torch.rand(B, N, N, generator=gen).argsort(dim=2)[:, :, :k].transpose(1, 2)
    elif pattern == "one_point":       # every slot of a list names the same point
        idx = torch.randint(N, (B, 1, N), generator=gen).expand(B, k, N)
    elif pattern == "self":
        idx = torch.arange(N).view(1, 1, N).expand(B, k, N)
    else:                              # everybody names point 0
        idx = torch.zeros(B, k, N, dtype=torch.long)
    return idx.contiguous().int()


def make_case(shape, pattern, kind, seed=7):
    """-> dict(x, idx, weights, scales, shifts), float32 CPU tensors.
    exact:  small integers -- x and shift in [-2, 2], scale in {-1, 1, 2}, weights in {-1, 0, 1} with three non-zeros a row
            (two where a row has only two entries)
    random: randn, the weights scaled by 1 / sqrt(K)."""
    B, c, N, k, widths = shape
    gen = torch.Generator().manual_seed(seed + 1000 * SHAPES.index(shape) + PATTERNS.index(pattern))
    idx = make_idx(pattern, B, k, N, gen)
    weights, scales, shifts = [], [], []
    if kind == "exact":
        x = torch.randint(-2, 3, (B, c, N), generator=gen).float()
        for K, wd in zip(fan_ins(c, widths), widths):
            W = torch.zeros(wd, K)
            cols = torch.rand(wd, K, generator=gen).argsort(dim=1)[:, :min(3, K)]
            W.scatter_(1, cols, (torch.randint(0, 2, cols.shape, generator=gen) * 2 - 1).float())
            weights.append(W)
            scales.append(torch.tensor([-1.0, 1.0, 2.0])[torch.randint(0, 3, (wd,), generator=gen)])
            shifts.append(torch.randint(-2, 3, (wd,), generator=gen).float())
    else:
        x = torch.randn(B, c, N, generator=gen)
        for K, wd in zip(fan_ins(c, widths), widths):
            weights.append(torch.randn(wd, K, generator=gen) / K ** 0.5)
            scales.append(torch.randn(wd, generator=gen))
            shifts.append(torch.randn(wd, generator=gen))
    return {"x": x, "idx": idx, "weights": weights, "scales": scales, "shifts": shifts}


def compose(x, idx, weights, scales, shifts):
    """The composition in plain torch at the tensors' own dtype and device -> (B, sum w, N)."""
    B, c, N = x.shape
    k = idx.shape[1]
    flat = idx.long().reshape(B, 1, k * N).expand(B, c, k * N)
    e = torch.cat((torch.gather(x, 2, flat).reshape(B, c, k, N), x.unsqueeze(2).expand(B, c, k, N)), dim=1)
    outs = []
    for W, sc, sh in zip(weights, scales, shifts):
        e = torch.relu(sc.view(1, -1, 1, 1) * torch.einsum("oc,bckn->bokn", W, e) + sh.view(1, -1, 1, 1))
        outs.append(e.max(dim=2)[0])
    return torch.cat(outs, dim=1)


def reference(x, idx, weights, scales, shifts, extra=0, shift_mags=None):
    """float64 CPU reference -> dict: out, mag (B, sum w, N), t (1, sum w, 1)."""
    x = x.detach().cpu().double()
    ii = idx.detach().cpu().long()
    weights, scales, shifts = ([t.detach().cpu().double() for t in ts] for ts in (weights, scales, shifts))
    shift_mags = [s.abs() for s in shifts] if shift_mags is None else [s.detach().cpu().double() for s in shift_mags]
    B, c, N = x.shape
    k = ii.shape[1]
    assert int(ii.min()) >= 0 and int(ii.max()) < N
    flat = ii.reshape(B, 1, k * N).expand(B, c, k * N)
    e = torch.cat((torch.gather(x, 2, flat).reshape(B, c, k, N), x.unsqueeze(2).expand(B, c, k, N)), dim=1)
    mag = e.abs()
    t, outs, mags, ts = 0, [], [], []
    for W, sc, sh, shm in zip(weights, scales, shifts, shift_mags):
        e = torch.relu(sc.view(1, -1, 1, 1) * torch.einsum("oc,bckn->bokn", W, e) + sh.view(1, -1, 1, 1))
        mag = sc.abs().view(1, -1, 1, 1) * torch.einsum("oc,bckn->bokn", W.abs(), mag) + shm.view(1, -1, 1, 1)
        t = t + W.shape[1] + 2 + extra
        outs.append(e.max(dim=2)[0])
        mags.append(mag.max(dim=2)[0])
        ts.append(torch.full((1, W.shape[0], 1), float(t), dtype=torch.float64))
    return {"out": torch.cat(outs, 1), "mag": torch.cat(mags, 1), "t": torch.cat(ts, 1)}


def bound_share(got, ref):
    """The largest |got - ref| / (t * 2^-24 * mag) over the elements (0 where both are 0 and the bound is too)."""
    err = (got.detach().cpu().double() - ref["out"]).abs()
    bound = ref["t"] * U * ref["mag"]
    assert bool((err[bound == 0] == 0).all())
    return float((err / bound.clamp_min(1e-300)).max())
