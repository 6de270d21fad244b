"""The numbers of the four 1x1-convolution entry points (mvp_benchmark_amd/pointwise.py) on every case
tests/test_pointwise_routes.py replays for its call trace (groups i and iii of the recorded fixture, under each case's
selectors) and on the extra cases of tests/pointwise_value_cases.py: outputs and every requested gradient against the
float64 closed forms, computed on the GPU with PyTorch operators.

Per case and family (exact: integers in [-4, 4], EQUAL; random: randn, within gamma(t) * mag element by element):
    values        outputs and gradients under the family's rule, on tensors copied out of their views;
    presence      every input that requires a gradient gets one that is not None, nothing else gets any;
    twin          a case with an offset / permuted tensor or an offset grad_out gives the bits of the same values in dense
                  tensors wherever the planners name the same route for that pass on both;
    twice         a second run gives the same bits on every route the header declares reproducible.
A batch of 0 goes through the same checks: empty outputs, zero parameter gradients of the parameters' shapes."""
import pytest
import torch

import pointwise_value_cases as pv

pytestmark = pytest.mark.gpu
rec = pv.rec
DEV = "cuda:0"


def run(c, t, gos):
    trace, outs, grads = rec.run_case(c, t, grad_out=gos, profiled=False)
    assert "error" not in trace, trace
    return outs, grads


def same_bits_where(planned, other, t, first, second, what, reproducible_only=False):
    """first / second = (outputs, gradients) of two runs under the plans `planned` / `other`: equal output by output and
    gradient by gradient wherever both plans name the same route for the pass behind it (reproducible_only: and the
    header declares that route reproducible)."""
    names = [("fwd", "out%d" % i) for i in range(len(first[0]))] + [(pv.PASS_OF[name], name) for name, _ in rec.grad_inputs(t)]
    tensors = zip(list(first[0]) + list(first[1] or ()), list(second[0]) + list(second[1] or ()))
    compared = 0
    for (which, name), (a, b) in zip(names, tensors):
        if planned[which] != other[which]:
            continue
        if reproducible_only and not pv.reproducible(planned[which]):
            continue
        assert torch.equal(a.detach(), b.detach()), "%s of %s: %s differs (route %s)" % (name, pv.case_id(planned["case"]), what, planned[which])
        compared += 1
    return compared


@pytest.mark.parametrize("c", pv.CASES, ids=pv.case_id)
def test_values_and_gradients_against_float64(c):
    from mvp_benchmark_amd import pointwise as pw
    full = rec.full(c)
    with pv.selectors(pw, c):
        planned = dict(pv.planned_routes(pw, c), case=c)
    with pv.selectors(pw, pv.twin_of(c)):
        dense = dict(pv.planned_routes(pw, pv.twin_of(c)), case=c)
    for family in pv.FAMILIES:
        t, gos = pv.make_tensors(c, family, DEV)
        outs, grads = run(c, t, gos)
        pv.check_gradient_presence(t, grads)
        assert [tuple(o.shape) for o in outs] == [tuple(s) for s in pv.out_shapes(c)]
        for (name, v), g in zip(rec.grad_inputs(t), grads or ()):
            assert g.shape == v.shape, name
        n = pv.compare(c, family, t, gos, outs, grads)
        print("compared %s %s: %d elements" % (family, pv.case_id(c), n))
        if full["B"] == 0:
            assert all(o.numel() == 0 for o in outs)
            for (name, v), g in zip(rec.grad_inputs(t), grads or ()):
                assert name == "x" or (g.shape == v.shape and not bool(g.any())), name
        if pv.has_layout(c):
            t2 = {k: pv.dense_copy(v) for k, v in t.items()}
            gos2 = None if gos is None else [g.contiguous().clone() for g in gos]
            assert all(v is None or (v.is_contiguous() and v.data_ptr() % 16 == 0) for v in list(t2.values()) + (gos2 or []))
            twin = run(pv.twin_of(c), t2, gos2)
            pv.compare(pv.twin_of(c), family, t2, gos2, *twin)
            same_bits_where(planned, dense, t, (outs, grads), twin, "the dense twin")
        again = run(c, t, gos)
        same_bits_where(planned, planned, t, (outs, grads), again, "a second run", reproducible_only=True)
