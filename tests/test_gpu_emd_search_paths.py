"""GPU parity tests of the paths of the one-bidder-per-wave search of the EMD auction (csrc/emd_search_wave.inc,
included into emd_auction_kernel's rounds of at most 192 bidders per workgroup and into every round of the lean
kernels): the seed's four chunks, the node test, the leaf-test steps, the list of surviving leaves with one and with
more than one visit step, leaves of more than 16 slots, the linear scan.  Every case is compared with the exhaustive CPU
oracle bit for bit -- distances, assignment, rounds, bids (utils/metrics/EMD/emd_cuda.cu:95-226)."""
import numpy as np
import pytest
import torch

from conftest import rand_clouds

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


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
    _lib.call("mvp_emd_forward", DEV, b, n, torch.tensor(x1, device=DEV), torch.tensor(x2, device=DEV),
              dist, ass, eps, iters, scratch, nbytes)
    torch.cuda.synchronize()
    return dist.cpu().numpy(), ass.cpu().numpy(), _lib.emd_records(scratch, nbytes, b)


def _check(oracle, x1, x2, eps, iters):
    d, a, rec = _run(x1, x2, eps, iters)
    od, oa, ost = oracle.emd_forward(x1, x2, eps, iters, return_stats=True)
    np.testing.assert_array_equal(a, oa)
    np.testing.assert_array_equal(d, od)
    np.testing.assert_array_equal(rec["rounds"], ost[:, 0])
    np.testing.assert_array_equal(rec["bids"], ost[:, 1])
    assert (rec["next_round"] == 0).all()
    return rec


def _sphere_pair(seed, b, n):
    """Independent samples of a sphere's surface (mvp_benchmark_amd.synthetic.prediction_pair)."""
    from mvp_benchmark_amd.synthetic import prediction_pair
    g = torch.Generator().manual_seed(seed)
    pred, gt = prediction_pair("sphere", "indep", g, b, n)
    return pred.numpy().astype(np.float32), gt.numpy().astype(np.float32)


def test_leaf_list_one_and_two_visit_steps_2048(oracle, knobs):
    """(2, 2048) uniform, cluster of 2, 400 rounds, gathered-bid rounds: a search lists 7.8 leaves on average (one or two
    leaf-test steps, one visit step with rows behind the list's end); 2.2 % of the searches list more than
    4 * kVisitLoads = 16 leaves and run a second visit step -- counted on the CPU with tools/emd_index_study.c (exact
    auction, leaves of 16 Hilbert-ordered slots, nodes of 16 leaves) on exactly these clouds, rounds 64..399."""
    knobs(cluster=2, split=5)
    x1, x2 = rand_clouds(811, 2, 2048, 3), rand_clouds(812, 2, 2048, 3)
    rec = _check(oracle, x1, x2, 0.004, 400)
    assert (rec["gathered_rounds"] > 0).all(), rec["gathered_rounds"]


def test_leaf_list_two_visit_steps_16384(oracle, knobs):
    """(1, 16384) uniform, cluster of 8, 330 rounds: the first kernel's and the lean kernel's rounds of one bidder per
    wave, plain and with gathered bids, on 1024 leaves of 16 slots in 64 nodes.  (A batch of one cloud stays on the
    8-wide lean kernel; the tiered launch needs 33 clouds and runs the same search: tests/test_gpu_emd_gathered.py's full
    batches.)  THE LIST'S OVERFLOW PATH RUNS: tools/emd_index_study.c on exactly these clouds, rounds 64..329 -- 9.2
    leaves listed per search, 6.0 % of the 52 403 searches list more than 4 * kVisitLoads = 16 and take a second visit
    step, the longest search of a round takes 2.06 steps on average."""
    knobs(cluster=8, split=5)
    x1, x2 = rand_clouds(821, 1, 16384, 3), rand_clouds(822, 1, 16384, 3)
    rec = _check(oracle, x1, x2, 0.004, 330)
    assert (rec["gathered_rounds"] > 0).all(), rec["gathered_rounds"]


def test_leaf_list_sphere_surface_2048(oracle, knobs):
    """Independent samples of a sphere's surface at (2, 2048), cluster of 2: flat, elongated boxes (6.6 leaves listed per
    search, 0.3 % of the searches with a second visit step by the same count)."""
    knobs(cluster=2, split=5)
    x1, x2 = _sphere_pair(5, 2, 2048)
    _check(oracle, x1, x2, 0.004, 400)


def test_leaves_of_32_slots(oracle):
    """(1, 17408), 60 rounds: the smallest cloud above 16384 points -- a leaf holds two 16-slot chunks (kch = 2: the
    visit's inner loop), no gathered-bid rounds.  ((1, 32768) costs the CPU oracle 45 s.)"""
    x1, x2 = rand_clouds(831, 1, 17408, 3), rand_clouds(832, 1, 17408, 3)
    _check(oracle, x1, x2, 0.004, 60)


@pytest.mark.parametrize("n", [1024, 2048])
def test_linear_scan_fallback(oracle, knobs, n):
    """A tight blob against a spread cloud: after a few rounds every object is dear, the whole cloud is within reach of
    every search -- all nodes pass and all 64 leaves of the first step -- and the search scans the objects linearly."""
    knobs(cluster=8)
    x2 = rand_clouds(841 + n, 1, n, 3)
    x1 = (np.float32(0.5) + np.float32(0.01) * (rand_clouds(842 + n, 1, n, 3) - np.float32(0.5))).astype(np.float32)
    _check(oracle, x1, x2, 0.004, 50)


def _lattice_pair(b):
    """1024 objects on a 16 x 8 x 8 lattice of spacing 1/16 (every coordinate and every squared distance exact in
    float32) and 1024 persons, TWO on each object with an even first index: the pair contests its object, the loser sees
    up to six neighbours at exactly equal distance and price -- equal values, decided by the tie rule on original
    indices."""
    i, j, k = np.meshgrid(np.arange(16), np.arange(8), np.arange(8), indexing="ij")
    obj = (np.stack([i, j, k], -1).reshape(-1, 3).astype(np.float32) + np.float32(0.5)) / np.float32(16)
    per = np.repeat(obj[(i % 2 == 0).reshape(-1)], 2, axis=0)
    x1 = np.stack([np.roll(per, 7 * c, axis=0)[:: 1 if c % 2 == 0 else -1] for c in range(b)])
    x2 = np.stack([obj[np.random.default_rng(870 + c).permutation(1024)] for c in range(b)])
    return np.ascontiguousarray(x1, dtype=np.float32), np.ascontiguousarray(x2, dtype=np.float32)


@pytest.mark.parametrize("cluster,split", [(8, 5), (2, 2), (1, 0)])
def test_seed_degeneracies_on_a_lattice(oracle, knobs, cluster, split):
    """Lattice clouds at (2, 1024): equal values everywhere, so the tie rule on ORIGINAL indices decides bids in the seed
    and in the fold.  With a cluster of 8 a member has 128 bidders in round 0 (below the 192 of the four-per-wave rounds):
    the first round already runs this search with FRESH bidders (p1 = p2 = -1: rows 0 and 1 of the seed have no chunk);
    a person's best and second best are lattice neighbours (often slots of ONE chunk: row 1 dropped) around its own
    position (the home chunk or its sibling: rows 2 / 3 dropped)."""
    knobs(cluster=cluster, split=split)
    x1, x2 = _lattice_pair(2)
    rec = _check(oracle, x1, x2, 0.004, 300)
    assert (rec["rounds"] > 20).all(), rec["rounds"]


def test_lean_kernel_several_searches_per_wave(oracle):
    """(3, 3072), default cluster, 120 rounds: the hand-over to the lean kernel happens inside the run, with up to 192
    bidders on a member's 16 waves -- a wave runs several searches in sequence per round."""
    from mvp_benchmark_amd import _lib
    x1, x2 = rand_clouds(851, 3, 3072, 3), rand_clouds(852, 3, 3072, 3)
    rec = _check(oracle, x1, x2, 0.004, 120)
    assert ((rec["first_handover"] > 0) & (rec["first_handover"] < 120)).all(), rec["first_handover"]
    assert _lib.EMD_DEFAULT_SPLIT == 5


def test_forced_last_round_in_gathered_rounds(oracle, knobs):
    """iters = 401 on (2, 2048), cluster of 2: the forced last round (emd_cuda.cu:196-215) is a gathered-bid round -- the
    bid records' tags of the last round."""
    knobs(cluster=2, split=5, resident_cap=1)
    x1, x2 = rand_clouds(861, 2, 2048, 3), rand_clouds(862, 2, 2048, 3)
    rec = _check(oracle, x1, x2, 0.004, 401)
    assert (rec["gathered_rounds"] > 0).all(), rec["gathered_rounds"]
