"""The launch sequence of mvp_emd_forward, read on the CPU.

csrc/emd_plan.h plans which EMD kernels one call launches, in which order, with which grid and scalar arguments, and what
follows when a cooperative launch is refused.  tests/emd_plan_check.cpp walks that planner for the cases below and prints
one line per launch; this test compiles it with the host compiler, runs it and compares the output with the traces written
out here.  The traces were derived by hand from the launch rules as the host code stated them before the planner existed
(emd_forward_with / emd_lean_launch), not from the planner's output.

Default knobs unless the case says otherwise: cluster 8, same_xcd 1, split 5, plan_round 300, plan_every 4096,
plan_widths 0, res_cap 16; 256 CUs; iters 3000.  fast_ok: 1 same-XCD stores, 2 gathered-bid rounds (split 5), 4 poll
distrust; the first kernel gets bit 0 only and every W1 launch gets 0."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EXPECTED = """\
== 1 b64 n16384
first W4 coop grid 256 lean 64 fast_ok 1
lean W4 RESN 0 coop grid 256 fast_ok 3 it_stop 300 which 1 u_stop 0
tiers W4 coop grid 256 fast_ok 3 it_stop 3000 which 2 pattern 0x0
== 2 b64 n16384 tiers refused
first W4 coop grid 256 lean 64 fast_ok 1
lean W4 RESN 0 coop grid 256 fast_ok 3 it_stop 300 which 1 u_stop 0
tiers W4 coop grid 256 fast_ok 3 it_stop 3000 which 2 pattern 0x0 -> refused
lean W4 RESN 0 coop grid 256 fast_ok 3 it_stop 3000 which 2 u_stop 0
== 3 b64 n16384 first refused
first W4 coop grid 256 lean 64 fast_ok 1 -> refused
first W1 plain grid 64 lean 64 fast_ok 0
lean W1 RESN 0 plain grid 64 fast_ok 0 it_stop 3000 which 1 u_stop 0
== 4 b2 n4096
first W8 coop grid 64 lean 64 fast_ok 1
lean W8 RESN 4096 coop grid 64 fast_ok 3 it_stop 3000 which 1 u_stop 16
resident RESN 4096 plain grid 2
== 5 b2 n4096 fused refused
first W8 coop grid 64 lean 64 fast_ok 1
lean W8 RESN 4096 coop grid 64 fast_ok 3 it_stop 3000 which 1 u_stop 16 -> refused
lean W8 RESN 0 coop grid 64 fast_ok 3 it_stop 3000 which 1 u_stop 16
resident RESN 4096 plain grid 2
== 5b b2 n4096 fused refused, then the plain lean launch too
first W8 coop grid 64 lean 64 fast_ok 1
lean W8 RESN 4096 coop grid 64 fast_ok 3 it_stop 3000 which 1 u_stop 16 -> refused
lean W8 RESN 0 coop grid 64 fast_ok 3 it_stop 3000 which 1 u_stop 16 -> refused, no answer
error
== 6 b2 n4096 split3 res_cap8
first W8 coop grid 64 lean 64 fast_ok 1
lean W8 RESN 0 coop grid 64 fast_ok 1 it_stop 3000 which 1 u_stop 8
resident RESN 4096 plain grid 2
== 7 b2 n4096 split1 cluster2
first W2 coop grid 16 lean 64 fast_ok 1
lean W2 RESN 0 coop grid 16 fast_ok 1 it_stop 3000 which 1 u_stop 0
== 8a b64 n16384 split0
first W4 coop grid 256 lean 0 fast_ok 1
== 8b b64 n16384 iters64
first W4 coop grid 256 lean 0 fast_ok 1
== 9 b40 n4096 split2
first W4 coop grid 160 lean 64 fast_ok 1
lean W4 RESN 0 coop grid 160 fast_ok 1 it_stop 300 which 1 u_stop 0
tiers W4 coop grid 160 fast_ok 1 it_stop 3000 which 2 pattern 0x0
== 10 b40 n4096 split2 plan_round600 plan_every700
first W4 coop grid 160 lean 64 fast_ok 1
lean W4 RESN 0 coop grid 160 fast_ok 1 it_stop 600 which 1 u_stop 0
tiers W4 coop grid 160 fast_ok 1 it_stop 1300 which 2 pattern 0x0
tiers W4 coop grid 160 fast_ok 1 it_stop 2000 which 2 pattern 0x0
tiers W4 coop grid 160 fast_ok 1 it_stop 2700 which 2 pattern 0x0
tiers W4 coop grid 160 fast_ok 1 it_stop 3000 which 2 pattern 0x0
== 10b the same, third tiered launch refused
first W4 coop grid 160 lean 64 fast_ok 1
lean W4 RESN 0 coop grid 160 fast_ok 1 it_stop 600 which 1 u_stop 0
tiers W4 coop grid 160 fast_ok 1 it_stop 1300 which 2 pattern 0x0
tiers W4 coop grid 160 fast_ok 1 it_stop 2000 which 2 pattern 0x0
tiers W4 coop grid 160 fast_ok 1 it_stop 2700 which 2 pattern 0x0 -> refused
lean W4 RESN 0 coop grid 160 fast_ok 1 it_stop 3000 which 2 u_stop 0
== 11a b64 n16384 iters555
first W4 coop grid 256 lean 64 fast_ok 1
lean W4 RESN 0 coop grid 256 fast_ok 3 it_stop 555 which 1 u_stop 0
== 11b b64 n16384 iters556
first W4 coop grid 256 lean 64 fast_ok 1
lean W4 RESN 0 coop grid 256 fast_ok 3 it_stop 300 which 1 u_stop 0
tiers W4 coop grid 256 fast_ok 3 it_stop 556 which 2 pattern 0x0
== 12 b32 n16384
first W8 coop grid 256 lean 64 fast_ok 1
lean W8 RESN 0 coop grid 256 fast_ok 3 it_stop 3000 which 1 u_stop 0
== 12 b33 n16384
first W4 coop grid 160 lean 64 fast_ok 1
lean W4 RESN 0 coop grid 160 fast_ok 3 it_stop 300 which 1 u_stop 0
tiers W4 coop grid 160 fast_ok 3 it_stop 3000 which 2 pattern 0x0
== 12 b64 n16384
first W4 coop grid 256 lean 64 fast_ok 1
lean W4 RESN 0 coop grid 256 fast_ok 3 it_stop 300 which 1 u_stop 0
tiers W4 coop grid 256 fast_ok 3 it_stop 3000 which 2 pattern 0x0
== 12 b65 n16384
first W2 coop grid 144 lean 64 fast_ok 1
lean W2 RESN 0 coop grid 144 fast_ok 3 it_stop 3000 which 1 u_stop 0
== 12 b129 n16384
first W1 plain grid 129 lean 64 fast_ok 0
lean W1 RESN 0 plain grid 129 fast_ok 0 it_stop 3000 which 1 u_stop 0
== 13 b64 n2048
first W4 coop grid 256 lean 64 fast_ok 1
lean W4 RESN 2048 coop grid 256 fast_ok 3 it_stop 3000 which 1 u_stop 16
resident RESN 2048 plain grid 64
== 14a b64 n16384 widths 8,5,4,4,3,3,3,2
first W4 coop grid 256 lean 64 fast_ok 1
lean W4 RESN 0 coop grid 256 fast_ok 3 it_stop 300 which 1 u_stop 0
tiers W4 coop grid 256 fast_ok 3 it_stop 3000 which 2 pattern 0x23334458
== 14b b64 n16384 widths 8,5,4,4,3,3,3,3
first W4 coop grid 256 lean 64 fast_ok 1
lean W4 RESN 0 coop grid 256 fast_ok 3 it_stop 3000 which 1 u_stop 0
== 14c b64 n16384 widths 7,5,4,4,3,3,3,3
first W4 coop grid 256 lean 64 fast_ok 1
lean W4 RESN 0 coop grid 256 fast_ok 3 it_stop 3000 which 1 u_stop 0
== 14d b40 n4096 split2 widths 7,5,4,4,3,3,3,3 (5 slots per XCD: not read)
first W4 coop grid 160 lean 64 fast_ok 1
lean W4 RESN 0 coop grid 160 fast_ok 1 it_stop 300 which 1 u_stop 0
tiers W4 coop grid 160 fast_ok 1 it_stop 3000 which 2 pattern 0x0
== 15a b64 n4096 split2
first W4 coop grid 256 lean 64 fast_ok 1
lean W4 RESN 0 coop grid 256 fast_ok 1 it_stop 300 which 1 u_stop 0
tiers W4 coop grid 256 fast_ok 1 it_stop 3000 which 2 pattern 0x0
== 15b b64 n4096 split5
first W4 coop grid 256 lean 64 fast_ok 1
lean W4 RESN 4096 coop grid 256 fast_ok 3 it_stop 3000 which 1 u_stop 16
resident RESN 4096 plain grid 64
== 16 b2 n4096 poll_distrust
first W8 coop grid 64 lean 64 fast_ok 1
lean W8 RESN 4096 coop grid 64 fast_ok 7 it_stop 3000 which 1 u_stop 16
resident RESN 4096 plain grid 2
== 17 b2 n4096 cus0
first W1 plain grid 2 lean 64 fast_ok 0
lean W1 RESN 4096 plain grid 2 fast_ok 0 it_stop 3000 which 1 u_stop 16
resident RESN 4096 plain grid 2
"""


def _compiler():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++", os.environ.get("HIPCC"), "hipcc", "/opt/rocm/bin/hipcc"):
        path = shutil.which(name) if name else None
        if path:
            return path
    pytest.fail("no C++ compiler (c++, g++, clang++ or hipcc) to build tests/emd_plan_check.cpp with")


def _cases(text):
    out, name = {}, None
    for line in text.splitlines():
        if line.startswith("== "):
            name = line[3:]
            assert name not in out, name
            out[name] = []
        else:
            out[name].append(line)
    return out


def test_emd_launch_plan_matches_the_traces(tmp_path):
    exe = str(tmp_path / "emd_plan_check")
    subprocess.run([_compiler(), "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "mvp_benchmark_amd", "csrc"),
                    os.path.join(ROOT, "tests", "emd_plan_check.cpp"), "-o", exe], check=True, timeout=300)
    got = subprocess.run([exe], capture_output=True, text=True, check=True, timeout=60).stdout
    got, want = _cases(got), _cases(EXPECTED)
    assert list(got) == list(want)
    for name in want:
        assert got[name] == want[name], name
