"""GPU parity tests of the wait of a gathered-bid round of the EMD auction (csrc/emd_lean_round_gathered.inc,
csrc/emd_lean_bid.inc): the waves that settle the round's bids load their bid records in the same trip as the members'
words they poll, and read them again only where a record's tags are not the round's.  Every result is compared with
the exhaustive CPU oracle bit for bit -- assignment, distances, rounds, bids -- through the C ABI, with the clouds, seeds
and helpers of
tests/test_gpu_emd_round_frame.py (these shapes reach gathered-bid rounds with these knobs)."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_emd_round_frame import EPS, _check, _clouds, _run, knobs  # noqa: F401  (knobs: a fixture)

pytestmark = pytest.mark.gpu


def _gathered(rec):
    assert (rec["gathered_rounds"] > 0).all(), rec["gathered_rounds"]


def test_words_of_members_with_empty_lists_are_waited_for(oracle, knobs):
    """2048 points on 8 members, to the end of the auction and without the resident tail: most members' lists are empty,
    their words are raised at the top of the round, and every record of the round can be valid long before the last
    word is -- the words vouch for the drained stores of the members without a bid, so the wait must not end on the
    records."""
    knobs(cluster=8, split=5, resident_cap=1)
    x1, x2 = _clouds(2, 2048)
    _gathered(_check(oracle, x1, x2, EPS, 3000))


@pytest.mark.parametrize("width", [2, 8])
def test_drawn_positions(oracle, knobs, width):
    """4096 points, 700 rounds: lists of more than 16 bidders, so the waves draw further positions and a member's last
    record -- the one that raises its word -- is stored long after its first ones."""
    knobs(cluster=width, split=5)
    x1, x2 = _clouds(2, 4096)
    _gathered(_check(oracle, x1, x2, EPS, 700, key=(2, 4096)))


def test_agent_scope_stores_and_loads(oracle, knobs):
    """same_xcd = 0 at width 8: records and words are written through, and the early record loads meet
    them at agent scope."""
    knobs(cluster=8, same_xcd=0, split=5)
    x1, x2 = _clouds(2, 4096)
    _gathered(_check(oracle, x1, x2, EPS, 700, key=(2, 4096)))


@pytest.mark.parametrize("iters", [299, 301])
def test_forced_last_round_and_launch_boundary_next_to_round_300(oracle, knobs, iters):
    """16384 points at width 8, ending a round before and a round behind round 300: the forced last round inside the
    gathered-bid rounds, and the launch boundary -- the count of these rounds, whose parity picks the bid area and
    whose value makes the tags, goes on across the launches."""
    knobs(cluster=8, split=5)
    x1, x2 = _clouds(1, 16384)
    _gathered(_check(oracle, x1, x2, EPS, iters, key=(1, 16384)))


_CHILD = (
    "import sys, hashlib, numpy as np, torch\n"
    "sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)\n"
    "from mvp_benchmark_amd import _lib\n"
    "_lib.LIB_PATH = _lib.LIB_PATH.replace('libmvpops.so', 'libmvpops_hooks.so')\n"   # the build with -DMVP_TEST_HOOKS: reads MVP_EMD_POLL_DISTRUST
    "from test_gpu_emd_round_frame import _clouds, _run\n"
    "n, width, iters = (int(a) for a in sys.argv[1:4])\n"
    "_lib.emd_configure(cluster=width)\n"
    "x1, x2 = _clouds(2, n)\n"
    "d, a, rec = _run(x1, x2, 0.004, iters)\n"
    "assert (rec['gathered_rounds'] > 0).all() and (rec['next_round'] == 0).all()\n"
    "print(hashlib.sha1(d.tobytes() + a.tobytes() + rec['rounds'].tobytes() + rec['bids'].tobytes()).hexdigest())\n"
)


@pytest.mark.parametrize("n,width,iters", [(2048, 8, 3000), (4096, 2, 700)])
def test_record_reread_kept_alive(oracle, knobs, n, width, iters):
    """The re-read of the bid records runs only for a record that arrived behind its member's word.  libmvpops_hooks.so
    with MVP_EMD_POLL_DISTRUST=1 takes the records that came with the words for untagged in every other gathered-bid
    round, so the re-read runs there: a child process with the switch, one without it and the release library (default
    knobs but the width) give the same bits, and the release library's are the oracle's."""
    knobs(cluster=width)
    x1, x2 = _clouds(2, n)
    d, a, rec = _run(x1, x2, EPS, iters)
    _gathered(_check(oracle, x1, x2, EPS, iters, key=(2, n)))
    want = hashlib.sha1(d.tobytes() + a.tobytes() + rec["rounds"].tobytes() + rec["bids"].tobytes()).hexdigest()
    tests = os.path.dirname(os.path.abspath(__file__))
    code = _CHILD % {"root": os.path.dirname(tests), "tests": tests}
    outs = []
    for extra in ({}, {"MVP_EMD_POLL_DISTRUST": "1"}):
        env = {k: v for k, v in os.environ.items() if k != "MVP_EMD_POLL_DISTRUST"}
        env.update(extra)
        r = subprocess.run([sys.executable, "-c", code, str(n), str(width), str(iters)], env=env, capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(r.stdout.strip().splitlines()[-1])
    assert outs[0] == outs[1] == want, (outs, want)
