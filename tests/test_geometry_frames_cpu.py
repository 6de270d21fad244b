"""Inputs and expectations of tests/test_gpu_geometry_frames.py, checked without a GPU.

Every GPU test of Chamfer / kNN / three_nn / ball_query / FPS used to draw its clouds from [0,1)^3, the one frame in
which the data-dependent parts of the spatial-index kernels (`lo`, `ext`, `invh = 16 / ext` of the sort kernels, the
box-pruning arithmetic) never see a negative origin, an extent far from 1, a zero extent or thousands of exact ties.
This module defines

  * FRAMES: maps applied to `rand_clouds` output (float32 arithmetic, contiguous result), and checks that each keeps
    the property it is named for;
  * `chamfer_contract`: the plain NumPy float32 statement of mvp_chamfer_forward's contract for non-finite input
    (include/mvpops.h), `lattice_clouds` / `poison`: the inputs it is tested on -- and checks that the statement
    equals the oracle's Chamfer where no poison is applied;
  * the shapes the GPU module uses, and checks that the oracle (for finite input: the reference's algorithm)
    accepts every frame at those shapes.
"""
import numpy as np
import pytest
from conftest import rand_clouds

F32 = np.float32
NAN_BITS = 0x7fc00000        # the quiet, positive NaN the contract names

# (b, n, m): the two smallest shapes past the sorted kernel's gate (n, m >= 2048 and n * m >= 2^24)
CHAMFER_SHAPES = [(2, 4096, 4096), (1, 2048, 8192)]
# (k, n candidates, m queries): both routes into mvp_knn_sorted (n >= 4096 and m >= 1024; square from 2048)
KNN_SHAPES = [(16, 4096, 1024), (16, 2048, 2048)]
# (entry point, b, n, m, w)
FPS_SHAPES = [("mvp_furthest_point_sampling", 2, 1537, 200, 0),
              ("mvp_furthest_point_sampling_sorted", 2, 4097, 256, 0),
              ("mvp_furthest_point_sampling_sorted", 1, 6000, 256, 0),
              ("mvp_furthest_point_sampling_cluster", 2, 8192, 128, 2)]
THREE_NN_SHAPE = (2, 300, 100)        # b, n unknown, m known
BALL_QUERY_SHAPE = (2, 1000, 70, 16)  # b, n points, m centres, nsample


def _c(a):
    a = np.ascontiguousarray(a, dtype=F32)
    assert a.dtype == F32
    return a


def _set_axes(x, **axes):
    x = x.copy()
    for name, v in axes.items():
        x[..., "xyz".index(name)] = F32(v)
    return x


ANISO = np.array([1.0, 2.0 ** -10, 2.0 ** -20], F32)

# one-sided frames: cloud (b, n, 3) in [0,1)^3 -> cloud
FRAMES = {
    "centred": lambda x: _c(x - F32(0.5)),
    "negative": lambda x: _c(-x),
    "offset": lambda x: _c(x + F32(1024)),                    # ulp 2^-13: thousands of exact distance ties
    "small": lambda x: _c(x * F32(2.0 ** -20)),
    "large": lambda x: _c(x * F32(2.0 ** 20)),
    "sheet": lambda x: _c(_set_axes(x, z=0.25)),
    "line": lambda x: _c(_set_axes(x, y=0.5, z=0.25)),
    "anisotropic": lambda x: _c(x * ANISO),
    "identical": lambda x: _c(np.broadcast_to(x[:, :1], x.shape)),
    "two-point": lambda x: _c(x[:, np.arange(x.shape[1]) % 2]),
    "subnormal": lambda x: _c(x * F32(2.0 ** -140)),
}
ONE_SIDED = list(FRAMES)
TWO_SIDED = ONE_SIDED + ["apart"]     # queries x + 8 against candidates x: every candidate box is disjoint from every query box

# radius of ball_query per frame: 0.2 in the frame's own scale (anisotropic: its widest axis keeps scale 1); subnormal:
# 2^-140, whose square is 0 in float32, so only d2 == 0 hits; apart: 8 (every distance is above 7 * sqrt(3): no hit)
BALL_RADIUS = {name: 0.2 for name in TWO_SIDED}
BALL_RADIUS.update({"small": 0.2 * 2.0 ** -20, "large": 0.2 * 2.0 ** 20, "subnormal": 2.0 ** -140, "apart": 8.0})


def frame_pair(name, queries, candidates):
    """(queries, candidates) of a two-sided operator in frame `name`."""
    if name == "apart":
        return _c(queries + F32(8)), _c(candidates)
    return FRAMES[name](queries), FRAMES[name](candidates)


def has_subnormal(x):
    a = np.abs(x)
    return bool(((a > 0) & (a < np.finfo(F32).tiny)).any())


def ball_centres(xyz_raw, m, seed):
    """m centres in [0,1)^3: the first half are points of the cloud (d2 == 0 hits), the rest independent."""
    b = xyz_raw.shape[0]
    return np.concatenate([xyz_raw[:, 5:5 + m // 2], rand_clouds(seed, b, m - m // 2, 3)], 1)


# ------------------------------------------------------------------------------------------------ non-finite contract
def chamfer_contract_one_way(q, c):
    """mvp_chamfer_forward's contract (include/mvpops.h), one direction, in plain NumPy float32: per query the minimum
    over the candidates whose distance is not NaN (+inf is a value like any other) and the LOWEST index at that
    minimum; a query for which every distance is NaN gets (NaN, 0).  q (b, n, 3), c (b, m, 3) -> dist (b, n), idx (b, n).
    Meant for inputs whose finite distances are exact in float32 whatever the order of the sum (lattice coordinates)."""
    b, n, _ = q.shape
    dist = np.empty((b, n), F32)
    idx = np.empty((b, n), np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(b):
            d = np.zeros((n, c.shape[1]), F32)
            for a in range(3):
                t = c[i, None, :, a] - q[i, :, None, a]        # candidate minus query, like the kernels
                d += t * t
            nan = np.isnan(d)
            mn = np.where(nan, F32(np.inf), d).min(1)
            first = (d == mn[:, None]).argmax(1)               # NaN equals nothing: the first NON-NaN candidate at the minimum
            none = nan.all(1)
            dist[i] = np.where(none, F32(np.nan), mn)
            idx[i] = np.where(none, 0, first)
    return dist, idx


def chamfer_contract(xyz1, xyz2):
    d1, i1 = chamfer_contract_one_way(xyz1, xyz2)
    d2, i2 = chamfer_contract_one_way(xyz2, xyz1)
    return d1, d2, i1, i2


def lattice_clouds(seed, b, n):
    """Coordinates that are multiples of 1/16 in [0,1): every finite squared distance is exact, and ties abound."""
    return _c(np.random.default_rng(seed).integers(0, 16, (b, n, 3)).astype(F32) / F32(16))


POISONS = ["nan_query", "nan_candidates", "inf_both_sides", "overflow_query", "all_nan_cloud"]


def poison(kind, xyz1, xyz2):
    """Returns poisoned copies of (xyz1, xyz2).  Chamfer runs both directions, so each side is queries and candidates."""
    a, c = xyz1.copy(), xyz2.copy()
    n, m = a.shape[1], c.shape[1]
    last = a.shape[0] - 1
    if kind == "nan_query":                 # a NaN in one coordinate of 3 queries
        a[0, 0, 0] = a[0, min(7, n - 1), 1] = a[last, n - 1, 2] = np.nan
    elif kind == "nan_candidates":          # 5 single candidates, candidate 0 among them, and a whole 16-candidate sub-tile
        for k, ax in zip([0, 5, m // 2 + 1, m - 3, m - 1], [0, 1, 2, 0, 1]):
            c[0, k, ax] = np.nan
        c[last, 0, 2] = np.nan
        c[0, 16:32, 1] = np.nan
    elif kind == "inf_both_sides":          # +inf and -inf coordinates on either side; same-signed pairs give NaN distances
        a[0, 3, 0] = np.inf
        a[0, min(9, n - 1), 1] = -np.inf
        a[last, n - 2, 2] = np.inf
        c[0, 2, 0] = np.inf
        c[0, 11, 2] = -np.inf
        c[last, 0, 1] = -np.inf
    elif kind == "overflow_query":          # every distance of one query overflows to +inf while candidates 0..15 are NaN
        a[0, 1] = 1e30
        a[last, n - 1] = -1e30
        c[:, :16, 0] = np.nan
    elif kind == "all_nan_cloud":           # one cloud that is all NaN
        c[0] = np.nan
    else:
        raise KeyError(kind)
    return a, c


# ---------------------------------------------------------------------------------------------------------- CPU tests
def _raw(seed, b, n):
    return rand_clouds(seed, b, n, 3)


@pytest.mark.parametrize("name", ONE_SIDED)
def test_frame_keeps_its_property(name):
    x = _raw(11, 2, 4097)
    y = FRAMES[name](x)
    assert y.dtype == F32 and y.flags["C_CONTIGUOUS"] and y.shape == x.shape and np.isfinite(y).all()
    lo, hi = y.min(1), y.max(1)          # (b, 3)
    ext = hi - lo
    if name == "centred":
        assert (lo < 0).all() and (hi > 0).all()
    elif name == "negative":
        assert (hi <= 0).all() and (lo < -0.9).all()
    elif name == "offset":
        assert (lo >= 1024).all() and (np.unique(y[0, :, 0]).size <= 8192)       # 13 bits below the offset
    elif name == "small":
        assert (ext < 2.0 ** -20).all() and (ext > 2.0 ** -21).all()
    elif name == "large":
        assert (ext > 2.0 ** 19).all()
    elif name == "sheet":
        assert (ext[:, 2] == 0).all() and (ext[:, :2] > 0.9).all()
    elif name == "line":
        assert (ext[:, 1:] == 0).all() and (ext[:, 0] > 0.9).all()
    elif name == "anisotropic":
        assert (ext[:, 0] > 0.9).all() and (ext[:, 1] < 2.0 ** -10).all() and (ext[:, 2] < 2.0 ** -20).all() and (ext[:, 2] > 0).all()
    elif name == "identical":
        assert (ext == 0).all() and (y == y[:, :1]).all()
    elif name == "two-point":
        assert (y[:, 0::2] == y[:, :1]).all() and (y[:, 1::2] == y[:, 1:2]).all() and (ext.max(1) > 0).all()
    elif name == "subnormal":
        for cloud in y:
            assert has_subnormal(cloud)
        assert (hi < np.finfo(F32).tiny).all()
        # 16 / ext overflows: the sort kernels' invh is +inf in this frame
        with np.errstate(over="ignore"):
            assert np.isinf(F32(16) / ext.max(1)).all()


def test_apart_boxes_are_disjoint():
    q, c = frame_pair("apart", _raw(1, 2, 4096), _raw(2, 2, 4096))
    assert (q.min(1) > c.max(1) + 6.9).all()         # on every axis: no candidate box can touch a query box


def test_ball_radii_square_as_intended():
    assert F32(BALL_RADIUS["subnormal"]) > 0 and F32(BALL_RADIUS["subnormal"]) * F32(BALL_RADIUS["subnormal"]) == 0
    assert set(BALL_RADIUS) == set(TWO_SIDED)


@pytest.mark.parametrize("b,n,m", [(2, 300, 100), (2, 4096, 4096), (3, 4096, 40)])
def test_contract_reference_equals_oracle_on_clean_lattice(oracle, b, n, m):
    """With the poison removed the NumPy statement of the contract IS the oracle's Chamfer (bit for bit)."""
    a, c = lattice_clouds(n, b, n), lattice_clouds(m + 1, b, m)
    want = oracle.chamfer_forward(a, c)
    for got, ref in zip(chamfer_contract(a, c), want):
        np.testing.assert_array_equal(got, ref)


def test_contract_reference_on_poison():
    """The statement itself, on cases small enough to read."""
    q = np.array([[[0, 0, 0], [np.nan, 0, 0], [1e30, 0, 0], [np.inf, 0, 0]]], F32)
    c = np.array([[[np.nan, 0, 0], [1, 0, 0], [np.inf, 0, 0], [1, 0, 0]]], F32)
    d, i = chamfer_contract_one_way(q, c)
    assert d[0, 0] == 1 and i[0, 0] == 1                            # NaN candidate 0 is never the nearest; lowest index of the tie
    assert d.view(np.uint32)[0, 1] == NAN_BITS and i[0, 1] == 0     # every distance NaN
    assert np.isposinf(d[0, 2]) and i[0, 2] == 1                    # +inf is a value: first candidate at +inf
    assert np.isposinf(d[0, 3]) and i[0, 3] == 1                    # inf - inf is NaN: candidate 2 does not count
    for kind in POISONS:
        a, p = poison(kind, lattice_clouds(1, 2, 300), lattice_clouds(2, 2, 100))
        assert not (np.isfinite(a).all() and np.isfinite(p).all())
        d1, d2, i1, i2 = chamfer_contract(a, p)
        assert ((i1 >= 0) & (i1 < 100)).all() and ((i2 >= 0) & (i2 < 300)).all()
        assert (i1[np.isnan(d1)] == 0).all() and (i2[np.isnan(d2)] == 0).all()
        nanbits = d1.view(np.uint32)[np.isnan(d1)]
        assert (nanbits == NAN_BITS).all()


@pytest.mark.parametrize("name", TWO_SIDED)
def test_oracle_accepts_frame_chamfer_knn_three_nn_ball_query(oracle, name):
    for b, n, m in CHAMFER_SHAPES:
        a, c = frame_pair(name, _raw(n + 3, b, n), _raw(m + 5, b, m))
        d1, d2, i1, i2 = oracle.chamfer_forward(a, c)
        assert np.isfinite(d1).all() and np.isfinite(d2).all() and (d1 >= 0).all()
        assert ((i1 >= 0) & (i1 < m)).all() and ((i2 >= 0) & (i2 < n)).all()
        if name == "apart":
            assert (d1 > 3 * 49 - 1).all()
        if name == "identical":
            assert (i1 == 0).all() and (i2 == 0).all()
    for k, n, m in KNN_SHAPES:
        ctr, xyz = frame_pair(name, _raw(701 + k, 2, m), _raw(700 + k, 2, n))
        idx, d = oracle.knn(k, xyz, ctr, return_dist=True)
        assert idx.shape == (2, k, m) and ((idx >= 0) & (idx < n)).all() and (np.diff(d, axis=2) >= 0).all()
    b, n, m = THREE_NN_SHAPE
    tgt, src = frame_pair(name, _raw(n, b, n), _raw(m, b, m))
    dist, idx = oracle.three_nn(tgt, src)
    assert np.isfinite(dist).all() and ((idx >= 0) & (idx < m)).all()
    b, n, m, s = BALL_QUERY_SHAPE
    raw = _raw(n, b, n)
    ctr, xyz = frame_pair(name, ball_centres(raw, m, 77), raw)
    idx = oracle.ball_query(0.0, BALL_RADIUS[name], s, xyz, ctr)
    assert ((idx >= 0) & (idx < n)).all()
    if name == "apart":
        assert (idx == 0).all()
    elif name == "subnormal":
        assert (idx == np.arange(s)).all()              # every squared distance underflows to 0: the first nsample points
    elif name not in ("identical", "two-point"):        # (those collapse the centres and the cloud onto different points)
        assert (idx[:, : m // 2].max(2) > 0).all()      # a centre that is a point of the cloud has hits


@pytest.mark.parametrize("name", ONE_SIDED)
def test_oracle_accepts_frame_fps(oracle, name):
    for _entry, b, n, m, _w in FPS_SHAPES:
        x = FRAMES[name](_raw(n * 7 + m, b, n))
        idx = oracle.furthest_point_sample(x, m)
        assert idx.shape == (b, m) and (idx[:, 0] == 0).all() and ((idx >= 0) & (idx < n)).all()
        if name not in ("identical", "two-point", "subnormal", "offset"):
            assert all(len(set(row)) == m for row in idx.tolist())       # distinct points while distances stay positive
