"""Chamfer / kNN / three_nn / ball_query / FPS on an MI355X (run with -m gpu) outside the unit cube and on non-finite
coordinates.

Part A: the clouds of tests/test_gpu_ops.py mapped into other frames (tests/test_geometry_frames_cpu.py: negative
origin, extents far from 1, zero extent on one / two / three axes, thousands of exact ties, subnormal coordinates,
disjoint sides).  Indices and distances are BIT-identical to the CPU oracle.  (In the `subnormal` frame every squared
distance underflows to 0 whether or not differences of subnormals are flushed: the frame stresses the sort kernels --
a subnormal extent, invh = +inf, 0 * inf in the cell index -- and the all-ties paths, not the denormal mode.)

Part B: the contract of include/mvpops.h for non-finite coordinates.  Chamfer: both forward kernels against the plain
NumPy statement of the contract, on lattice coordinates (every finite distance exact) with NaN / +-inf / overflowing
coordinates on either side; every index is checked to be in range on the host BEFORE the backward kernel consumes
it.  three_nn, ball_query and mvp_knn: what the kernels do with NaN / inf, pinned; mvp_knn_sorted: equal to mvp_knn.
The FPS kernels are not run on non-finite input (csrc/fps.hip assumes `best >= 0` and NaN-free minima)."""
import numpy as np
import pytest
import torch
from conftest import rand_clouds
from test_geometry_frames_cpu import (BALL_QUERY_SHAPE, BALL_RADIUS, CHAMFER_SHAPES, FPS_SHAPES, FRAMES, KNN_SHAPES,
                                      NAN_BITS, ONE_SIDED, POISONS, THREE_NN_SHAPE, TWO_SIDED, ball_centres,
                                      chamfer_contract, frame_pair, has_subnormal, lattice_clouds, poison)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _chamfer(name, a, c):
    """One forward entry point through the C ABI -> (dist1, dist2, idx1, idx2) as numpy; scratch pre-filled with 0xAB."""
    from mvp_benchmark_amd import _lib
    b, n, m = a.shape[0], a.shape[1], c.shape[1]
    ta, tc = dev(a), dev(c)
    d1, d2 = torch.zeros(b, n, device=DEV), torch.zeros(b, m, device=DEV)
    i1 = torch.full((b, n), -7, dtype=torch.int32, device=DEV)
    i2 = torch.full((b, m), -7, dtype=torch.int32, device=DEV)
    if name.endswith("sorted"):
        nbytes = _lib.chamfer_scratch_bytes(b, n, m)
        scratch = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device=DEV)
        _lib.call(name, DEV, b, n, m, ta, tc, d1, d2, i1, i2, scratch, nbytes)
    else:
        _lib.call(name, DEV, b, n, m, ta, tc, d1, d2, i1, i2)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (d1, d2, i1, i2))


# ====================================================================================================== Part A: frames
@pytest.mark.parametrize("b,n,m", CHAMFER_SHAPES)
@pytest.mark.parametrize("name", TWO_SIDED)
def test_chamfer_in_frame(oracle, name, b, n, m):
    """Both forward kernels and cd() equal each other and the oracle; `small` also equals the unscaled cloud's result
    scaled by exactly 2^-40 (scaling by a power of two commutes with every rounding while nothing underflows)."""
    from mvp_benchmark_amd.metrics import cd
    raw_a, raw_c = rand_clouds(n + 3, b, n, 3), rand_clouds(m + 5, b, m, 3)
    a, c = frame_pair(name, raw_a, raw_c)
    if name == "subnormal":
        assert all(has_subnormal(x) for x in a) and all(has_subnormal(x) for x in c)
    want = oracle.chamfer_forward(a, c)
    plain = _chamfer("mvp_chamfer_forward", a, c)
    srt = _chamfer("mvp_chamfer_forward_sorted", a, c)
    for got in (plain, srt, tuple(t.cpu().numpy() for t in cd()(dev(a), dev(c)))):
        for g, w in zip(got, want):
            np.testing.assert_array_equal(g, w)
    if name == "small":
        unit = oracle.chamfer_forward(raw_a, raw_c)
        np.testing.assert_array_equal(srt[2], unit[2])
        np.testing.assert_array_equal(srt[3], unit[3])
        np.testing.assert_array_equal(srt[0], unit[0] * F32(2.0 ** -40))
        np.testing.assert_array_equal(srt[1], unit[1] * F32(2.0 ** -40))


@pytest.mark.parametrize("k,n,m", KNN_SHAPES)
@pytest.mark.parametrize("name", TWO_SIDED)
def test_knn_in_frame(oracle, name, k, n, m):
    """mvp_knn and mvp_knn_sorted: indices and distances equal the oracle's replay of the reference's heap.  (`large`:
    squared distances pass the reference's 1e10 heap seed, which clips the lists -- equality with the oracle is the
    only claim there.)  The recompute counter: every query where all k + 1 nearest tie, almost none where the frame is
    an exact image of the unit cube."""
    from mvp_benchmark_amd import _lib
    b = 2
    ctr, xyz = frame_pair(name, rand_clouds(701 + k, b, m, 3), rand_clouds(700 + k, b, n, 3))
    want_i, want_d = oracle.knn(k, xyz, ctr, return_dist=True)        # (b, k, m), (b, m, k)
    txyz, tctr = dev(xyz), dev(ctr)
    nbytes = _lib.knn_scratch_bytes(b, n, m)
    scratch = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device=DEV)
    for entry in ("mvp_knn", "mvp_knn_sorted"):
        idx = torch.full((b, m, k), -7, dtype=torch.int32, device=DEV)
        d2 = torch.zeros(b, m, k, device=DEV)
        extra = (scratch, nbytes) if entry.endswith("sorted") else ()
        _lib.call(entry, DEV, b, n, m, k, txyz, tctr, idx, d2, *extra)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(idx.cpu().numpy().transpose(0, 2, 1), want_i, err_msg=entry)
        np.testing.assert_array_equal(d2.cpu().numpy(), want_d, err_msg=entry)
    # the counters of the fix-up pass sit in front of the id lists (as test_knn_sorted_variant_is_bit_identical reads them)
    cnt_at = nbytes - ((b * m * 4 + 15) // 16 * 16) - ((b * 4 + 15) // 16 * 16)
    recomputed = scratch[cnt_at: cnt_at + b * 4].view(torch.int32).cpu().numpy()
    print("knn %s (%d, %d, %d): recomputed per cloud %s" % (name, k, n, m, recomputed.tolist()))
    if name in ("identical", "two-point", "subnormal"):
        assert (recomputed == m).all()
    elif name in ("centred", "negative", "small"):
        assert recomputed.sum() <= 2


@pytest.mark.parametrize("entry,b,n,m,w", FPS_SHAPES)
@pytest.mark.parametrize("name", ONE_SIDED)
def test_fps_in_frame(oracle, name, entry, b, n, m, w):
    """The register-resident, the Morton-sorted and the cluster kernel: indices AND the running minima left in `temp`
    equal the oracle's.  `identical`, `two-point`, `subnormal` and `offset` make every round a tie round."""
    import oracle as orc
    from mvp_benchmark_amd import _lib
    x = FRAMES[name](rand_clouds(n * 7 + m, b, n, 3))
    want_t = np.full((b, n), 1e10, F32)
    want_i = np.zeros((b, m), np.int32)
    assert orc.lib().orc_furthest_point_sampling(b, n, m, orc._pf(x), orc._pf(want_t), orc._pi(want_i)) == 0
    tx = dev(x)
    temp = torch.full((b, n), 1e10, device=DEV)
    idx = torch.full((b, m), -7, dtype=torch.int32, device=DEV)
    if entry.endswith("sorted"):
        nbytes = _lib.fps_scratch_bytes(b, n)
        ws = torch.full((nbytes,), 0xCD, dtype=torch.uint8, device=DEV)
        _lib.call(entry, DEV, b, n, m, tx, temp, idx, ws, nbytes)
    elif entry.endswith("cluster"):
        nbytes = _lib.fps_cluster_scratch_bytes(b)
        ws = torch.full((nbytes,), 0xCD, dtype=torch.uint8, device=DEV)
        _lib.call(entry, DEV, b, n, m, w, tx, temp, idx, ws, nbytes)
    else:
        _lib.call(entry, DEV, b, n, m, tx, temp, idx)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(idx.cpu().numpy(), want_i)
    np.testing.assert_array_equal(temp.cpu().numpy(), want_t)


def _oracle_three_nn_squared(tgt, src):
    import oracle as orc
    b, n, m = tgt.shape[0], tgt.shape[1], src.shape[1]
    d2, idx = np.zeros((b, n, 3), F32), np.zeros((b, n, 3), np.int32)
    assert orc.lib().orc_three_nn(b, n, m, orc._pf(tgt), orc._pf(src), orc._pf(d2), orc._pi(idx)) == 0
    return d2, idx


def _three_nn(tgt, src):
    from mvp_benchmark_amd import _lib
    b, n, m = tgt.shape[0], tgt.shape[1], src.shape[1]
    d2 = torch.zeros(b, n, 3, device=DEV)
    idx = torch.full((b, n, 3), -7, dtype=torch.int32, device=DEV)
    _lib.call("mvp_three_nn", DEV, b, n, m, dev(tgt), dev(src), d2, idx)
    torch.cuda.synchronize()
    return d2.cpu().numpy(), idx.cpu().numpy()


@pytest.mark.parametrize("name", TWO_SIDED)
def test_three_nn_in_frame(oracle, name):
    from mvp_benchmark_amd.mm3d_pn2 import three_nn
    b, n, m = THREE_NN_SHAPE
    tgt, src = frame_pair(name, rand_clouds(n, b, n, 3), rand_clouds(m, b, m, 3))
    want_d2, want_i = _oracle_three_nn_squared(tgt, src)
    d2, idx = _three_nn(tgt, src)
    np.testing.assert_array_equal(idx, want_i)
    np.testing.assert_array_equal(d2, want_d2)
    np.testing.assert_array_equal(three_nn(dev(tgt), dev(src))[1].cpu().numpy(), want_i)


@pytest.mark.parametrize("name", TWO_SIDED)
def test_ball_query_in_frame(oracle, name):
    from mvp_benchmark_amd.mm3d_pn2 import ball_query
    b, n, m, s = BALL_QUERY_SHAPE
    raw = rand_clouds(n, b, n, 3)
    ctr, xyz = frame_pair(name, ball_centres(raw, m, 77), raw)
    r = BALL_RADIUS[name]
    idx = ball_query(0.0, r, s, dev(xyz), dev(ctr))
    np.testing.assert_array_equal(idx.cpu().numpy(), oracle.ball_query(0.0, r, s, xyz, ctr))


# ========================================================================================= Part B: non-finite coordinates
# (entry point, b, n, m): the sorted kernel (the second shape leaves padding entries in the sorted sets: 4100 -> 5120),
# the exhaustive kernel with Q = 1, 2 (b * max(n, m) = 262144) and 4 queries per lane
NONFINITE_SHAPES = [("mvp_chamfer_forward_sorted", 2, 4096, 4096), ("mvp_chamfer_forward_sorted", 1, 4100, 4200),
                    ("mvp_chamfer_forward", 2, 300, 100), ("mvp_chamfer_forward", 64, 4096, 40),
                    ("mvp_chamfer_forward", 256, 4096, 40)]
_clean_lattice = {}


def _poisoned(kind, b, n, m):
    if (b, n, m) not in _clean_lattice:
        _clean_lattice[(b, n, m)] = (lattice_clouds(n, b, n), lattice_clouds(m + 1, b, m))
    return poison(kind, *_clean_lattice[(b, n, m)])


def _assert_meets_contract(got, want, n, m, what):
    d1, d2, i1, i2 = got
    # every index in range before anything else looks at (or gathers with) it
    assert ((i1 >= 0) & (i1 < m)).all() and ((i2 >= 0) & (i2 < n)).all(), what
    for g, w in zip((i1, i2), want[2:]):
        np.testing.assert_array_equal(g, w, err_msg=what)
    for g, w in zip((d1, d2), want[:2]):
        np.testing.assert_array_equal(_bits(g), _bits(w), err_msg=what)     # bit for bit: the NaN is 0x7fc00000
        assert (_bits(g)[np.isnan(g)] == NAN_BITS).all()


@pytest.mark.parametrize("entry,b,n,m", NONFINITE_SHAPES)
@pytest.mark.parametrize("kind", POISONS)
def test_chamfer_nonfinite_contract(kind, entry, b, n, m):
    """What these cases are after (from reading the kernels as they were before the contract was written down): the
    exhaustive kernel folded NaN away with fminf and wrote (+inf, 0) for a NaN query, and looked for the arg-min of an
    all-+inf query in sub-tile 0 only; the sorted kernel minimised {distance bits, index}, so a NaN query got NaN with
    the lowest original index among the tiles its wave happened to visit, and the padding index 0x7fffffff when every
    real candidate was NaN."""
    a, c = _poisoned(kind, b, n, m)
    want = chamfer_contract(a, c)
    got = _chamfer(entry, a, c)
    _assert_meets_contract(got, want, n, m, entry)
    if entry.endswith("sorted"):          # the two kernels meet it bit for bit with each other
        _assert_meets_contract(_chamfer("mvp_chamfer_forward", a, c), want, n, m, "mvp_chamfer_forward")


@pytest.mark.parametrize("kind", POISONS)
def test_chamfer_backward_after_nonfinite_forward(kind):
    """mvp_chamfer_backward on the indices of a poisoned forward (checked to be in range first), finite graddist: a
    gradient component is finite exactly where every term that the contract's pairing adds to it is finite."""
    from mvp_benchmark_amd import _lib
    b, n, m = 2, 300, 100
    a, c = _poisoned(kind, b, n, m)
    want = chamfer_contract(a, c)
    got = _chamfer("mvp_chamfer_forward", a, c)
    _assert_meets_contract(got, want, n, m, "mvp_chamfer_forward")
    i1, i2 = got[2], got[3]
    g1, g2 = rand_clouds(3, b, n) + F32(0.5), rand_clouds(4, b, m) + F32(0.5)
    ga, gc = torch.zeros(b, n, 3, device=DEV), torch.zeros(b, m, 3, device=DEV)
    _lib.call("mvp_chamfer_backward", DEV, b, n, m, dev(a), dev(c), ga, gc, dev(g1), dev(g2), dev(i1), dev(i2))
    torch.cuda.synchronize()
    ra, rc = np.zeros((b, n, 3)), np.zeros((b, m, 3))
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(b):
            t1 = 2.0 * g1[i, :, None] * (a[i].astype(np.float64) - c[i, i1[i]])       # (n, 3): own term of a_j, scattered onto c_idx1[j]
            t2 = 2.0 * g2[i, :, None] * (c[i].astype(np.float64) - a[i, i2[i]])
            ra[i] += t1
            np.add.at(rc[i], i1[i], -t1)
            rc[i] += t2
            np.add.at(ra[i], i2[i], -t2)
    for got_g, ref in ((ga.cpu().numpy(), ra), (gc.cpu().numpy(), rc)):
        assert (np.isfinite(got_g) == np.isfinite(ref)).all()
        fin = np.isfinite(ref)
        np.testing.assert_allclose(got_g[fin], ref[fin], rtol=1e-5, atol=1e-5)
    if kind != "all_nan_cloud":
        assert np.isfinite(ga.cpu().numpy()).mean() > 0.9       # the poison stays local


def _nonfinite_small_clouds():
    """n = 200 points, m = 70 centres / queries per cloud; cloud 0 carries the poison, cloud 1 is clean."""
    xyz, ctr = rand_clouds(21, 2, 200, 3), rand_clouds(22, 2, 70, 3)
    xyz[0, 0, 0] = xyz[0, 17, 1] = xyz[0, 64, 2] = xyz[0, 199, 0] = np.nan      # NaN points
    xyz[0, 3, 1] = np.inf
    xyz[0, 130, 2] = -np.inf
    ctr[0, 1, 0] = np.nan                                                       # NaN queries
    ctr[0, 69, 2] = np.nan
    ctr[0, 5, 1] = np.inf                                                       # every distance +inf or NaN
    ctr[0, 6] = 1e30                                                            # every distance overflows
    return xyz, ctr


def test_three_nn_nonfinite_is_never_selected():
    """The bests start at (+inf, 0) and move on strict `<`: NaN and +inf distances are never selected; with fewer than
    three others the slots left keep (+inf, 0)."""
    xyz, ctr = _nonfinite_small_clouds()                       # unknown = ctr (2, 70, 3), known = xyz (2, 200, 3)
    d2, idx = _three_nn(ctr, xyz)
    assert ((idx >= 0) & (idx < 200)).all()
    with np.errstate(invalid="ignore", over="ignore"):
        d = ((ctr[:, :, None].astype(np.float64) - xyz[:, None]) ** 2).sum(-1).astype(F32)    # float64 sum, rounded: order only
    d = np.where(np.isnan(d), np.inf, d)
    order = np.argsort(d, axis=2, kind="stable")[:, :, :3]
    for q in (1, 69, 5, 6):                                    # NaN queries, the inf query, the overflowing query
        assert np.isposinf(d2[0, q]).all() and (idx[0, q] == 0).all()
    ok = np.isfinite(np.take_along_axis(d, order, 2)).all(2)
    assert ok.sum() == 2 * 70 - 4
    np.testing.assert_array_equal(idx[ok], order[ok])
    assert np.isfinite(d2[ok]).all() and (np.diff(d2[ok], axis=1) >= 0).all()
    # a known set with only two usable points: the third slot keeps (+inf, 0)
    few = np.full((1, 5, 3), np.nan, F32)
    few[0, 1], few[0, 3] = (0.25, 0.5, 0.5), (0.75, 0.5, 0.5)
    d2, idx = _three_nn(np.full((1, 4, 3), 0.5, F32) * np.array([0.8, 1, 1], F32), few)
    np.testing.assert_array_equal(idx, np.tile(np.array([1, 3, 0], np.int32), (1, 4, 1)))
    assert np.isfinite(d2[..., :2]).all() and np.isposinf(d2[..., 2]).all()


def test_ball_query_nonfinite_is_no_hit():
    """A NaN distance is no hit: a centre with a NaN coordinate gets a row of zeros, NaN points are skipped (so are
    points at an infinite distance)."""
    from mvp_benchmark_amd import _lib
    from mvp_benchmark_amd.mm3d_pn2 import ball_query
    xyz, ctr = _nonfinite_small_clouds()
    s, r = 16, 0.35
    idx = torch.full((2, 70, s), -7, dtype=torch.int32, device=DEV)
    _lib.call("mvp_ball_query", DEV, 2, 200, 70, 0.0, r, s, dev(ctr), dev(xyz), idx)
    torch.cuda.synchronize()
    idx = idx.cpu().numpy()
    assert ((idx >= 0) & (idx < 200)).all()
    np.testing.assert_array_equal(ball_query(0.0, r, s, dev(xyz), dev(ctr)).cpu().numpy(), idx)
    for q in (1, 69, 5, 6):
        assert (idx[0, q] == 0).all()
    with np.errstate(invalid="ignore", over="ignore"):
        d = ((ctr[:, :, None].astype(np.float64) - xyz[:, None]) ** 2).sum(-1)
    hit = d < np.float64(F32(r) * F32(r)) * (1 - 1e-6)          # clear hits; NaN compares false
    near = np.abs(d - np.float64(F32(r) * F32(r))) <= np.float64(F32(r) * F32(r)) * 1e-6
    for i in range(2):
        for q in range(70):
            if near[i, q].any():
                continue                                        # (a distance within rounding of the radius: not this test's subject)
            hits = np.flatnonzero(hit[i, q])[:s]
            want = np.zeros(s, np.int64) if hits.size == 0 else np.concatenate([hits, np.full(s - hits.size, hits[0])])
            np.testing.assert_array_equal(idx[i, q], want)
    bad = [0, 17, 64, 199, 3, 130]
    assert not np.isin(idx[0][hit[0].any(1)], bad[1:]).any()     # (index 0 is also the fill value of an empty row)


def _knn_pair(entry, k, xyz, ctr):
    from mvp_benchmark_amd import _lib
    b, n, m = xyz.shape[0], xyz.shape[1], ctr.shape[1]
    idx = torch.full((b, m, k), -7, dtype=torch.int32, device=DEV)
    d2 = torch.zeros(b, m, k, device=DEV)
    extra = ()
    if entry.endswith("sorted"):
        nbytes = _lib.knn_scratch_bytes(b, n, m)
        extra = (torch.full((nbytes,), 0xAB, dtype=torch.uint8, device=DEV), nbytes)
    _lib.call(entry, DEV, b, n, m, k, dev(xyz), dev(ctr), idx, d2, *extra)
    torch.cuda.synchronize()
    return idx.cpu().numpy(), d2.cpu().numpy()


def test_knn_nonfinite_is_never_admitted():
    """The heap starts at (1e10, 0) and admits on strict `<`: NaN, +inf and distances >= 1e10 never enter; unfilled
    slots keep (1e10, 0), last."""
    from mvp_benchmark_amd.mm3d_pn2 import knn
    xyz, ctr = _nonfinite_small_clouds()
    ctr[0, 7] = 2e5                                             # squared distances of 1.2e11 >= 1e10: never admitted
    k = 8
    idx, d2 = _knn_pair("mvp_knn", k, xyz, ctr)
    assert ((idx >= 0) & (idx < 200)).all()
    for q in (1, 69, 5, 6, 7):
        assert (idx[0, q] == 0).all() and (d2[0, q] == F32(1e10)).all()
    with np.errstate(invalid="ignore", over="ignore"):
        d = ((ctr[:, :, None].astype(np.float64) - xyz[:, None]) ** 2).sum(-1)
    d = np.where(np.isnan(d), np.inf, d)
    order = np.argsort(d, axis=2, kind="stable")[:, :, :k]
    ok = np.ones((2, 70), bool)
    ok[0, [1, 69, 5, 6, 7]] = False
    np.testing.assert_array_equal(idx[ok], order[ok])           # random clouds: the k nearest are pairwise different
    assert (d2[ok] < 3).all() and (np.diff(d2[ok], axis=1) >= 0).all()
    np.testing.assert_array_equal(knn(k, dev(xyz), dev(ctr), False).cpu().numpy(), idx.transpose(0, 2, 1))
    # fewer admissible candidates than k: the slots left keep (1e10, 0)
    few = np.full((1, 12, 3), np.nan, F32)
    few[0, 2], few[0, 9], few[0, 11] = (0.1, 0, 0), (0.2, 0, 0), (np.inf, 0, 0)
    idx, d2 = _knn_pair("mvp_knn", 4, few, np.zeros((1, 3, 3), F32))
    np.testing.assert_array_equal(idx, np.tile(np.array([2, 9, 0, 0], np.int32), (1, 3, 1)))
    np.testing.assert_array_equal(d2, np.tile(np.array([F32(0.1) * F32(0.1), F32(0.2) * F32(0.2), 1e10, 1e10], F32), (1, 3, 1)))


@pytest.mark.parametrize("k,n,m", KNN_SHAPES)
def test_knn_sorted_nonfinite_equals_exhaustive(k, n, m):
    """mvp_knn_sorted on NaN / inf / overflowing queries and candidates: equal to mvp_knn on the same input.  (By
    reading: a non-finite distance never passes `d < dd[KL-1]`, such queries end with equal 1e10 slots and are
    recomputed by the exhaustive heap; boxes are built with fmin / fmax, which drop NaN, and only ever under-estimate.)"""
    xyz, ctr = rand_clouds(31, 2, n, 3), rand_clouds(32, 2, m, 3)
    xyz[0, [0, 5, n // 2, n - 1], [0, 1, 2, 0]] = np.nan
    xyz[0, 100:116, 1] = np.nan
    xyz[0, 7, 0], xyz[0, 300, 2] = np.inf, -np.inf
    ctr[0, [0, 9, m - 1], [0, 1, 2]] = np.nan
    ctr[0, 3, 0], ctr[0, 4, 1] = np.inf, -np.inf
    ctr[0, 11] = 1e30
    ctr[0, 12] = 2e5
    xyz[1] = np.nan                                             # a cloud whose candidates are all NaN
    want_i, want_d = _knn_pair("mvp_knn", k, xyz, ctr)
    assert ((want_i >= 0) & (want_i < n)).all()
    got_i, got_d = _knn_pair("mvp_knn_sorted", k, xyz, ctr)
    assert ((got_i >= 0) & (got_i < n)).all()
    np.testing.assert_array_equal(got_i, want_i)
    np.testing.assert_array_equal(_bits(got_d), _bits(want_d))
    assert (want_d[1] == F32(1e10)).all() and (want_i[1] == 0).all()
    for q in (0, 9, m - 1, 3, 4, 11, 12):
        assert (want_d[0, q] == F32(1e10)).all()
