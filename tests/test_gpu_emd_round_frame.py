"""GPU parity tests of the frame around the search in a gathered-bid round of the EMD auction (csrc/emd_lean.hip and its
fragments): the position draw that a list of at most a bidder per wave skips, the bidder counts and the first bid
position that the end of a round hands to the next one, and the one test in front of the events of a round's end (last
round, launch boundary, hand-over to the resident kernel, collapse to member 0, everybody assigned).  Every result is
compared with the exhaustive CPU oracle bit for bit -- assignment, distances, rounds, bids -- through the C ABI
(utils/metrics/EMD/emd_cuda.cu:95-226).

What the knobs allow (csrc/emd.hip: emd_apply_knobs): mvp_emd_configure takes cluster widths 1, 2, 4 and 8 and a
resident_cap of 1..64.  Widths 3 and 5 exist only in the tiered launch, which serves 33..64 clouds of more than 4096
points from round 300 on, so they are tested on a batch of 64 clouds; "no hand-over to the resident kernel" is
resident_cap = 1 (the cluster collapses to member 0 at 16 persons, long before one is left)."""
import numpy as np
import pytest
import torch

from conftest import rand_clouds

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 0.004


def dev(a):
    return torch.tensor(a, device=DEV)


@pytest.fixture
def knobs():
    """mvp_emd_configure for one test; the defaults come back afterwards."""
    from mvp_benchmark_amd import _lib
    yield _lib.emd_configure
    _lib.emd_configure(cluster=0, same_xcd=1, split=_lib.EMD_DEFAULT_SPLIT, resident_cap=16)


def _run(x1, x2, eps, iters):
    from mvp_benchmark_amd import _lib
    b, n = x1.shape[:2]
    nbytes = _lib.emd_scratch_bytes(b, n)
    scratch = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    dist = torch.zeros(b, n, device=DEV)
    ass = torch.zeros(b, n, dtype=torch.int32, device=DEV)
    _lib.call("mvp_emd_forward", DEV, b, n, x1 if torch.is_tensor(x1) else dev(x1), x2 if torch.is_tensor(x2) else dev(x2),
              dist, ass, eps, iters, scratch, nbytes)
    torch.cuda.synchronize()
    return dist.cpu().numpy(), ass.cpu().numpy(), _lib.emd_records(scratch, nbytes, b)


_ORACLE = {}


def _check(oracle, x1, x2, eps, iters, key=None):
    """`key` names the input: the oracle's result of (key, eps, iters) is computed once and shared by the tests that
    differ only in the library's knobs."""
    d, a, rec = _run(x1, x2, eps, iters)
    if key is None:
        od, oa, ost = oracle.emd_forward(x1, x2, eps, iters, return_stats=True)
    else:
        if (key, eps, iters) not in _ORACLE:
            _ORACLE[key, eps, iters] = oracle.emd_forward(x1, x2, eps, iters, return_stats=True)
        od, oa, ost = _ORACLE[key, eps, iters]
    np.testing.assert_array_equal(a, oa)
    np.testing.assert_array_equal(d, od)
    np.testing.assert_array_equal(rec["rounds"], ost[:, 0])
    np.testing.assert_array_equal(rec["bids"], ost[:, 1])
    assert (rec["next_round"] == 0).all()
    return rec


_CLOUDS = {}
_TRACES = {}


def _clouds(b, n):
    if (b, n) not in _CLOUDS:
        _CLOUDS[b, n] = (rand_clouds(300 + n // 1024 + b, b, n, 3), rand_clouds(400 + n // 1024 + b, b, n, 3))
    return _CLOUDS[b, n]


def _trace(oracle, b, n, rounds=700):
    """Unassigned persons at the start of every round (b, rounds), from the oracle, once per shape.  (The rounds before
    the last one do not depend on the number of rounds: a shorter auction sees the same counts.)"""
    if (b, n) not in _TRACES:
        x1, x2 = _clouds(b, n)
        _TRACES[b, n] = oracle.emd_forward_ex(x1, x2, EPS, rounds)[3]
    return _TRACES[b, n]


def _round_with(trace, lo, hi, latest):
    """The earliest / latest round r >= 80 at whose start some cloud has more than lo and every cloud at most hi unassigned persons,
    with at most 256 in every cloud for the 8 rounds before (the gathered-bid rounds are entered a round after that count
    is reached; the lean kernel takes a cloud at least 64 rounds before the end).  The auction of r + 1 rounds has r as
    its forced last round (emd_cuda.cu:196-215)."""
    ok = (trace > lo).any(0) & (trace <= hi).all(0)
    calm = (trace <= 256).all(0)
    rounds = range(80, trace.shape[1])
    for r in (reversed(rounds) if latest else rounds):
        if ok[r] and calm[r - 8:r].all():
            return r
    return None


@pytest.mark.parametrize("draw", [True, False], ids=["draw", "nodraw"])
@pytest.mark.parametrize("width", [2, 8])
@pytest.mark.parametrize("n", [2048, 4096])
def test_forced_last_round_with_and_without_position_draw(oracle, knobs, n, width, draw):
    """The auction's forced last round inside the gathered-bid rounds, once where a member still has more than 16
    bidders -- more than a bidder per wave: the waves draw further list positions from the shared counter -- and once
    where no list is longer than 16 and nobody draws.  The number of rounds comes from a sweep over the oracle's count of
    unassigned persons per round.  Draw: a cloud with more than 16 x width persons has more than 16 in some list
    whatever the split.  No draw: at most 32 persons per cloud, and a cloud with more than the 16 at which it leaves the
    cluster's rounds, over lists that the evictions fill round-robin.  On 8 members these clouds never have more than
    128 persons 64 rounds after the lean kernel took them: there the earliest such round, the one with the most persons,
    stands in (8 members with drawn positions: the 16384-point case of test_round_end_events_around_round_300, 100..220
    persons at round 300)."""
    knobs(cluster=width, split=5, resident_cap=16)
    x1, x2 = _clouds(2, n)
    tr = _trace(oracle, 2, n)
    if draw:
        r = _round_with(tr, 16 * width, 256, latest=False)
        if r is None and width == 8:
            r = 80
    else:
        r = _round_with(tr, 16, 32, latest=True)
    assert r is not None and r >= 80, "these seeds no longer give such a round"
    rec = _check(oracle, x1, x2, EPS, r + 1, key=(2, n))
    assert (rec["gathered_rounds"] > 0).all(), rec["gathered_rounds"]


@pytest.mark.parametrize("resident_cap", [1, 16])
@pytest.mark.parametrize("iters", [299, 300, 301, 302])
@pytest.mark.parametrize("b,n,width", [(2, 4096, 2), (2, 4096, 8), (1, 16384, 8)])
def test_round_end_events_around_round_300(oracle, knobs, b, n, width, iters, resident_cap):
    """Auctions that end at and next to round 300 (where a batch of the headline's size changes launches), with the
    hand-over to the resident kernel at 16 persons -- the count at which the cluster collapses to member 0 too -- and
    with practically none (resident_cap 1): the forced last round, the hand-over and the collapse fall into the same
    or into neighbouring rounds.  (16384 points are above the resident kernel's size: there the knob changes nothing.)"""
    knobs(cluster=width, split=5, resident_cap=resident_cap)
    x1, x2 = _clouds(b, n)
    rec = _check(oracle, x1, x2, EPS, iters, key=(b, n))
    assert (rec["gathered_rounds"] > 0).all(), rec["gathered_rounds"]


def test_launch_boundary_and_tiered_widths_3_and_5(oracle, knobs):
    """64 clouds of 5120 points, 600 rounds, default knobs: the lean launch stops in front of round 300 (the round
    threshold of the end-of-round test is the launch's, not the auction's), the tiered launch deals the workgroups out
    again -- cluster widths 8, 5, 4, 3 and 2, the instances of the round loop that no knob reaches -- and runs the
    gathered-bid rounds to the forced last round.  Two clouds of widths 3 and 5 and one of every other width against the oracle."""
    from mvp_benchmark_amd import _lib
    knobs(cluster=0, same_xcd=1, split=_lib.EMD_DEFAULT_SPLIT, resident_cap=16)
    b, n, iters = 64, 5120, 600
    x1n, x2n = rand_clouds(511, b, n, 3), rand_clouds(512, b, n, 3)
    d, a, rec = _run(dev(x1n), dev(x2n), EPS, iters)
    assert (rec["next_round"] == 0).all() and (rec["gathered_rounds"] > 0).all()
    assert (rec["final_launch"] == 2).all(), rec["final_launch"]
    widths = rec["final_width"]
    assert {3, 5} <= set(widths.tolist()), widths
    pick = np.concatenate([np.flatnonzero(widths == w)[:2 if w in (3, 5) else 1] for w in sorted(set(widths.tolist()))])
    od, oa, ost = oracle.emd_forward(x1n[pick], x2n[pick], EPS, iters, return_stats=True)
    np.testing.assert_array_equal(a[pick], oa)
    np.testing.assert_array_equal(d[pick], od)
    np.testing.assert_array_equal(rec["rounds"][pick], ost[:, 0])
    np.testing.assert_array_equal(rec["bids"][pick], ost[:, 1])


def test_auction_converges_after_gathered_rounds(oracle, knobs):
    """A prediction near its ground truth at eps 0.02: everybody is assigned long before the 3000 rounds are over.  The
    cloud (8192 points: no resident tail) runs gathered-bid rounds, collapses to member 0 at 16 persons and ends when
    nobody is left -- a cluster always collapses before its count can reach zero, so `everybody assigned` is met by the
    rounds behind the collapse; the gathered-bid rounds meet the collapse itself."""
    knobs(cluster=8, split=5)
    gt = rand_clouds(902, 1, 8192, 3)
    pred = (gt + np.float32(0.07) * (rand_clouds(903, 1, 8192, 3) - np.float32(0.5))).astype(np.float32)
    rec = _check(oracle, pred, gt, 0.02, 3000)   # (the oracle: nobody left after round 2322, 17..256 bidders in 16 rounds after round 70)
    assert (rec["rounds"] < 3000).all(), rec["rounds"]
    assert (rec["gathered_rounds"] > 0).all(), rec["gathered_rounds"]


def test_members_with_empty_lists(oracle, knobs):
    """2048 points on 8 members: a few bidders over eight lists -- members whose list is empty raise their word at the
    top of the round instead of with their last bid."""
    knobs(cluster=8, split=5, resident_cap=1)
    x1, x2 = _clouds(2, 2048)
    rec = _check(oracle, x1, x2, EPS, 3000)
    assert (rec["gathered_rounds"] > 0).all(), rec["gathered_rounds"]


def test_agent_scope_stores(oracle, knobs):
    """same_xcd = 0 at width 8: records, member words and state stores written through."""
    knobs(cluster=8, same_xcd=0, split=5)
    x1, x2 = _clouds(2, 4096)
    rec = _check(oracle, x1, x2, EPS, 700)
    assert (rec["gathered_rounds"] > 0).all(), rec["gathered_rounds"]
