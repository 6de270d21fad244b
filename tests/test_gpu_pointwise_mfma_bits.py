"""The output bits of every instance of the MFMA GEMM kernels (csrc/pointwise_mfma.hip: forward / data gradient, row
maximum, split-K, weight gradient) against tests/golden/pointwise_mfma_bits.json, recorded from the build before the three
kernels shared one K loop.  The order of every matrix instruction is part of the kernels' contract (the split-K tests lean on
it); a tolerance against float64, or split-K against the plain kernel, does not see a reordering both sides share.

Cases, inputs (no RNG) and digests: tests/golden/make_pointwise_mfma_bits.py."""
import importlib.util
import os

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_pointwise_mfma_bits", os.path.join(HERE, "golden", "make_pointwise_mfma_bits.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

CASES = rec.cases()
GOLDEN = rec.load_fixture()


def test_the_fixture_holds_exactly_the_cases():
    assert sorted(GOLDEN) == sorted(name for name, _ in CASES)
    kinds = [c["kind"] for _, c in CASES]
    assert (kinds.count("fwd"), kinds.count("max"), kinds.count("splitk"), kinds.count("wgrad")) == (18, 2, 24, 32)


@pytest.mark.parametrize("name,case", CASES, ids=[name for name, _ in CASES])
def test_output_bits(name, case):
    assert rec.run(case) == GOLDEN[name]
