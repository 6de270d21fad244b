"""The Morton index itself (csrc/cs_sort.h), read back from the scratch of the three `*_sorted` entry points on an
MI355X (run with -m gpu).  The other tests pin what the searches compute from the index; these pin its layout:

(a) the non-padding entries carry every original index 0..cnt-1 exactly once, with the input's coordinates bit for bit;
(b) the Morton cell -- recomputed in float32 with the kernel's operations -- never decreases along the order;
(c) the padding is the documented entry up to the documented padded count, and nothing is written behind it;
(d) side layout (Chamfer, kNN): every tile box and batch box is the min / max of its non-padding members, a tile of
    padding only holds {+inf, -inf}.

The order inside a cell is left to the LDS atomics and is not asserted."""
import numpy as np
import pytest
import torch
from conftest import rand_clouds

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
TILE, BATCH = 16, 1024
SIDE_PAD = np.array([0x7f800000, 0x7f800000, 0x7f800000, 0x7fffffff], np.uint32)   # {+inf, +inf, +inf, kCsPad}
FPS_PAD = np.array([0, 0, 0, 0xffffffff], np.uint32)                               # {0, 0, 0, -1}


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _spread4(v):   # bit i -> bit 3i
    v = v & 0xF
    v = (v | (v << 4)) & 0xC3
    v = (v | (v << 2)) & 0x249
    return v


def morton_cells(cloud, pts):
    """Cells of `pts` in the grid of `cloud` (cnt, 3), with the kernel's float32 operations: fminf / fmaxf skip NaN."""
    lo, hi = np.fmin.reduce(cloud, axis=0), np.fmax.reduce(cloud, axis=0)
    ext = F32(0)
    with np.errstate(invalid="ignore", over="ignore"):
        for a in range(3):
            ext = np.fmax(ext, F32(hi[a] - lo[a]))
        if not ext > 0 or not ext < F32(3.0e38):
            ext = F32(1)
        invh = F32(16) / ext
        v = np.fmin(np.fmax((pts - lo) * invh, F32(0)), F32(15))   # a NaN becomes 0
    assert v.dtype == F32
    i = v.astype(np.int32)
    return _spread4(i[:, 0]) | (_spread4(i[:, 1]) << 1) | (_spread4(i[:, 2]) << 2)


def check_points(entries, cloud, npad, pad):
    """(a), (b), (c) on one cloud's entries: uint32 (npad, 4)."""
    cnt = cloud.shape[0]
    assert entries.shape == (npad, 4)
    np.testing.assert_array_equal(entries[cnt:], np.broadcast_to(pad, (npad - cnt, 4)))
    orig = entries[:cnt, 3].astype(np.int64)
    np.testing.assert_array_equal(np.sort(orig), np.arange(cnt))
    np.testing.assert_array_equal(entries[:cnt, :3], cloud.view(np.uint32)[orig])
    cells = morton_cells(cloud, entries[:cnt, :3].view(F32))
    assert cells.min() >= 0 and cells.max() < 4096
    assert (np.diff(cells) >= 0).all()


def check_side(raw, cloud):
    """One side of the Chamfer / kNN layout: raw = its bytes as uint32 words."""
    cnt = cloud.shape[0]
    cp = (cnt + BATCH - 1) // BATCH * BATCH
    assert raw.size == (cp * 16 + cp // TILE * 32 + cp // BATCH * 32) // 4
    entries = raw[:cp * 4].reshape(cp, 4)
    check_points(entries, cloud, cp, SIDE_PAD)
    tbox = raw[cp * 4: cp * 4 + cp // TILE * 8].reshape(cp // TILE, 2, 4)
    bbox = raw[cp * 4 + cp // TILE * 8:].reshape(cp // BATCH, 2, 4)
    # (d) padding takes part as +inf in the minimum and -inf in the maximum: an all-padding tile is {+inf, -inf}
    xyz = entries[:, :3].view(F32).copy()
    real = (np.arange(cp) < cnt)[:, None]
    tlo = np.fmin.reduce(np.where(real, xyz, F32(np.inf)).reshape(cp // TILE, TILE, 3), axis=1)
    thi = np.fmax.reduce(np.where(real, xyz, F32(-np.inf)).reshape(cp // TILE, TILE, 3), axis=1)
    np.testing.assert_array_equal(tbox[:, 0, :3].view(F32), tlo)
    np.testing.assert_array_equal(tbox[:, 1, :3].view(F32), thi)
    np.testing.assert_array_equal(bbox[:, 0, :3].view(F32), np.fmin.reduce(tlo.reshape(cp // BATCH, BATCH // TILE, 3), axis=1))
    np.testing.assert_array_equal(bbox[:, 1, :3].view(F32), np.fmax.reduce(thi.reshape(cp // BATCH, BATCH // TILE, 3), axis=1))
    assert not tbox[:, :, 3].any() and not bbox[:, :, 3].any()    # .w = 0
    if cp - cnt >= TILE:
        assert (tbox[-1, 0, :3].view(F32) == np.inf).all() and (tbox[-1, 1, :3].view(F32) == -np.inf).all()


def check_pair_scratch(scratch, first, second):
    """scratch: uint8 tensor; per cloud side 0 = `first` (b, n0, 3), then side 1 = `second` (b, n1, 3)."""
    raw = scratch.cpu().numpy().view(np.uint32)

    def words(c):
        cp = (c + BATCH - 1) // BATCH * BATCH
        return (cp * 16 + cp // TILE * 32 + cp // BATCH * 32) // 4
    w0, w1 = words(first.shape[1]), words(second.shape[1])
    for c in range(first.shape[0]):
        at = c * (w0 + w1)
        check_side(raw[at: at + w0], first[c])
        check_side(raw[at + w0: at + w0 + w1], second[c])
    return first.shape[0] * (w0 + w1) * 4   # bytes the sides take


def chamfer_index(a, c):
    from mvp_benchmark_amd import _lib
    b, n, m = a.shape[0], a.shape[1], c.shape[1]
    d1, d2 = torch.zeros(b, n, device=DEV), torch.zeros(b, m, device=DEV)
    i1 = torch.zeros(b, n, dtype=torch.int32, device=DEV)
    i2 = torch.zeros(b, m, dtype=torch.int32, device=DEV)
    nbytes = _lib.chamfer_scratch_bytes(b, n, m)
    scratch = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device=DEV)
    _lib.call("mvp_chamfer_forward_sorted", DEV, b, n, m, dev(a), dev(c), d1, d2, i1, i2, scratch, nbytes)
    torch.cuda.synchronize()
    assert check_pair_scratch(scratch, a, c) == nbytes


def fps_index(x, m=2):
    from mvp_benchmark_amd import _lib
    b, n = x.shape[0], x.shape[1]
    p = (n + 1023) // 1024
    npad = 1024 * (6 if p <= 6 else 8 if p <= 8 else 12 if p <= 12 else 16)
    temp = torch.full((b, n), 1e10, device=DEV)
    idx = torch.zeros(b, m, dtype=torch.int32, device=DEV)
    nbytes = _lib.fps_scratch_bytes(b, n)
    scratch = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device=DEV)
    _lib.call("mvp_furthest_point_sampling_sorted", DEV, b, n, m, dev(x), temp, idx, scratch, nbytes)
    torch.cuda.synchronize()
    raw = scratch.cpu().numpy().view(np.uint32)
    for c in range(b):   # cloud c at c * npad entries
        check_points(raw[c * npad * 4: (c + 1) * npad * 4].reshape(npad, 4), x[c], npad, FPS_PAD)
    assert (raw[b * npad * 4:] == 0xABABABAB).all()    # nothing behind the last cloud's padding
    assert ((idx.cpu().numpy() >= 0) & (idx.cpu().numpy() < n)).all()


def degenerate(name, x):
    """x (b, cnt, 3) in [0, 1) -> the degenerate cloud `name`."""
    x = x.copy()
    if name == "identical":        # extent 0: one cell
        x[:] = x[:, :1]
    elif name == "flat":           # one axis constant
        x[:, :, 1] = F32(0.25)
    elif name == "offset":         # coordinates in [1e6, 1e6 + 1]
        x += F32(1e6)
    elif name == "nonfinite":      # a NaN and a +inf, neither in point 0
        x[:, 5, 1] = np.nan
        x[:, 9, 0] = np.inf
    return x


DEGENERATE = ("identical", "flat", "offset", "nonfinite")


# (1, 2048, 8192): both thresholds of the sorted path met exactly; (2, 2500, 7000): both sides off the 1024 grid
@pytest.mark.parametrize("b,n,m", [(1, 2048, 8192), (2, 2500, 7000)])
def test_chamfer_index(b, n, m):
    chamfer_index(rand_clouds(n + 1, b, n, 3), rand_clouds(m + 2, b, m, 3))


@pytest.mark.parametrize("name", DEGENERATE)
def test_chamfer_index_degenerate(name):
    chamfer_index(degenerate(name, rand_clouds(11, 1, 2048, 3)), degenerate(name, rand_clouds(12, 1, 8192, 3)))


# both routes into the sorted search: n >= 4096 with m >= 1024, and the square one from 2048 points
@pytest.mark.parametrize("k,n,m", [(4, 4096, 1024), (4, 2049, 2050)])
def test_knn_index(k, n, m):
    from mvp_benchmark_amd import _lib
    b = 2
    xyz, ctr = rand_clouds(n + 3, b, n, 3), rand_clouds(m + 4, b, m, 3)
    idx = torch.zeros(b, m, k, dtype=torch.int32, device=DEV)
    d2 = torch.zeros(b, m, k, device=DEV)
    nbytes = _lib.knn_scratch_bytes(b, n, m)
    scratch = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device=DEV)
    _lib.call("mvp_knn_sorted", DEV, b, n, m, k, dev(xyz), dev(ctr), idx, d2, scratch, nbytes)
    torch.cuda.synchronize()
    used = check_pair_scratch(scratch, ctr, xyz)    # side 0: the queries, side 1: the candidates
    # behind the sides: the fix-up counters and lists
    assert used == nbytes - ((b * m * 4 + 15) // 16 * 16) - ((b * 4 + 15) // 16 * 16)


# points per lane 6, 8, 12, 16
@pytest.mark.parametrize("b,n", [(2, 4097), (1, 6145), (1, 8193), (1, 12289)])
def test_fps_index(b, n):
    fps_index(rand_clouds(n, b, n, 3))


@pytest.mark.parametrize("name", DEGENERATE)
def test_fps_index_degenerate(name):
    fps_index(degenerate(name, rand_clouds(13, 2, 4097, 3)))
