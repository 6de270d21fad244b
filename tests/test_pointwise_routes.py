"""Which kernels a 1x1-convolution layer takes (mvp_benchmark_amd/pointwise.py), pinned against
tests/golden/pointwise_routes.json: the library entry points and PyTorch operators every case ran on the commit before
the routing planner existed (tests/golden/make_pointwise_routes.py recorded it there, unmodified).

CPU: for every row the Layer description is built by hand, the planner runs under the row's selectors, and the planned
routes must imply exactly the recorded trace (ROUTE_CALLS / ROUTE_OPS below say what a route name runs).
GPU: the rows of groups i and iii are replayed through the public entry points and the live trace must equal the
recorded one.  The rows marked fix "b" (grad_out a view at an odd offset: the recorded trace is an MVP_EBADARG refusal
or a detour) must take the trace of their aligned twin instead and give the same gradients bit for bit."""
import importlib.util
import os

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_pointwise_routes", os.path.join(HERE, "golden", "make_pointwise_routes.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

MFMA, MFMA_MAX = "mvp_pointwise_mfma_ex", "mvp_pointwise_mfma_max"
ROUTE_CALLS = {"dgrad": {"mfma": [MFMA], "small": ["mvp_pointwise_dgrad"]},
               "wgrad": {"mfma": ["mvp_pointwise_wgrad_mfma_ex"], "small": ["mvp_pointwise_wgrad"]}}
ROUTE_OPS = {"dgrad": {"gemm": {"gemm"}}, "wgrad": {"gemm": {"einsum", "gemm"}, "miopen": {"conv_backward"}}}


def fixture():
    rows = rec.load_fixture()
    by_key = {rec.key(c): t for c, t in rows}
    return rows, by_key


def twin(c):
    return {k: v for k, v in c.items() if k not in ("go", "fix")}


def layer_of(pw, c):
    """The Layer of a case, by hand (no tensors)."""
    length = 1
    for s in c["tail"]:
        length *= s
    return pw.Layer(cuda=True, f32=True, dim=2 + len(c["tail"]), B=c["B"], cin=c["cin"], cout=c["cout"],
                    L=length if c["B"] else 0, x_dense=c["x"] != "permuted", w_dense=c["w"] != "permuted",
                    x_aligned=c["x"] != "offset", w_aligned=c["w"] != "offset", nonempty=c["B"] > 0)


class Trace:
    def __init__(self):
        self.calls, self.ops, self.fn = [], set(), set()

    def add(self, other):
        self.calls += other.calls
        self.ops |= other.ops
        self.fn |= other.fn
        return self

    def as_dict(self):
        return {"calls": self.calls, "ops": sorted(self.ops), "fn": sorted(self.fn)}


def conv_trace(pw, d, relu, has_bias, grad, library_is_gemm):
    """What pointwise_conv runs, from its plans."""
    t = Trace()
    plan = pw._plan_conv(d, bool(grad))
    assert plan.via == ("none" if not grad and pw.USE_MFMA else plan.via)
    if plan.fwd == "mfma":
        t.calls.append(MFMA)
    else:
        t.ops.add("gemm" if library_is_gemm and plan.via != "autograd" else "conv")
    if plan.via == "function":
        t.fn.add("_PointwiseConvBackward")
        back = pw._plan_conv_backward(plan.layer, relu, has_bias, "x" in grad, "w" in grad, has_bias and "b" in grad)
        for which, route in (("dgrad", back.dgrad), ("wgrad", back.wgrad)):
            t.calls += ROUTE_CALLS[which].get(route, [])
            if not (which == "wgrad" and route == "gemm" and "w" not in grad):       # (the bias gradient alone is a sum)
                t.ops |= ROUTE_OPS[which].get(route, set())
        if back.premask:
            t.ops.add("threshold_backward")
        assert (back.wgrad_bytes > 0) == (back.wgrad == "mfma")
    elif grad:
        t.fn.add("ConvolutionBackward0")
        t.ops.add("conv_backward")
        if relu:
            t.ops.add("threshold_backward")
    return t


def planned_trace(pw, c):
    """The trace the planners imply for a case (selectors already set)."""
    c = rec.full(c)
    d, fl, grad, gemm = layer_of(pw, c), c["flags"], c["grad"], pw.LIBRARY_IS_GEMM
    relu = bool(fl.get("relu"))
    fresh = d._replace(x_dense=True, x_aligned=True)              # relu(x): a new tensor
    t = Trace()
    if c["entry"] == "conv":
        t = conv_trace(pw, d, relu, c["bias"], grad, gemm)
    elif c["entry"] == "fused":
        res, cb = bool(fl.get("residual")), bool(fl.get("cloud_bias"))
        if pw._plan_fused(d, "x" in grad, relu, res) == "fused":
            t.calls.append(MFMA)
            if grad:
                t.fn.add("_PointwiseConvFusedBackward")
                if (relu or fl.get("relu_after")) and (res or cb):
                    t.ops.add("threshold_backward")
                t.calls += [MFMA] * ("x" in grad) + ROUTE_CALLS["wgrad"]["mfma"] * ("w" in grad or "b" in grad)
        else:
            inner = "".join(g for g in grad if g in ("xw" if cb else "xwb"))
            t = conv_trace(pw, fresh if fl.get("relu_in") else d, relu and not cb, c["bias"] and not cb, inner, gemm)
            if grad and ((fl.get("relu_in") and "x" in grad) or (cb and relu) or fl.get("relu_after")):
                t.ops.add("threshold_backward")
    elif c["entry"] == "dual":
        d2 = d._replace(cout=c["cout2"])
        if pw._plan_dual(d, d2, "x" in grad) == "stacked":
            t.calls.append(MFMA)
            if grad:
                t.fn.add("_PointwiseConvDualBackward")
                t.calls += [MFMA] * (2 * ("x" in grad)) + ROUTE_CALLS["wgrad"]["mfma"] * (2 * ("w" in grad))
        else:
            t = conv_trace(pw, d, False, False, grad, gemm).add(conv_trace(pw, d2, False, False, grad, gemm))
            t.calls.sort()                                           # (autograd orders the two backward nodes)
    else:
        plan = pw._plan_max(d, bool(grad))
        if plan.fwd == "fused":
            t.calls.append(MFMA_MAX)
        else:
            t = conv_trace(pw, d, False, c["bias"], grad if plan.via == "autograd" else "", gemm)
        if plan.via == "function":
            t.fn.add("_PointwiseConvMaxBackward")
            if pw._plan_max_backward(d._replace(dim=3)) == "sparse":
                t.calls.append("mvp_pointwise_max_backward")
            elif "w" in grad:
                t.ops |= {"einsum", "gemm"}
    return t.as_dict()


def test_planned_routes_imply_the_recorded_traces():
    """Every row of the fixture (all three groups), on the CPU: Layer by hand -> planner -> trace."""
    from mvp_benchmark_amd import pointwise as pw
    rows, by_key = fixture()
    assert len(rows) > 300 and {c["group"] for c, _ in rows} == {"i", "ii", "iii"}
    saved = {k: getattr(pw, k) for k in rec.DEFAULTS}
    bad = []
    try:
        for c, recorded in rows:
            if c.get("fix") == "b":
                recorded = by_key[rec.key(twin(c))]
            for k, v in dict(rec.DEFAULTS, **c.get("sel", {})).items():
                setattr(pw, k, v)
            planned = planned_trace(pw, c)
            if "error" in recorded:
                # the one refusal recorded outside the fix "b" rows: mvp_pointwise_wgrad (MVP_EBADARG) for an x that is a view
                # at an odd offset -- the plan now gives that weight gradient to the library
                assert c["x"] == "offset" and recorded["calls"][-1] == "mvp_pointwise_wgrad", c
                recorded = {"calls": recorded["calls"][:-1], "ops": sorted(set(recorded["ops"]) | {"conv_backward"}), "fn": recorded["fn"]}
            if c["entry"] == "dual" and not recorded["fn"] == ["_PointwiseConvDualBackward"]:
                recorded = dict(recorded, calls=sorted(recorded["calls"]))
            if planned != recorded:
                bad.append((c, planned, recorded))
    finally:
        for k, v in saved.items():
            setattr(pw, k, v)
    assert not bad, "%d rows, first: %r" % (len(bad), bad[:3])


def test_fused_plan_composes_relu_with_a_residual_and_foreign_operands():
    """The soundness fixes the fixture cannot hold (their recorded behaviour was the wrong one): relu together with a
    residual, and a residual / cloud_bias that is not float32, take the composed route."""
    from mvp_benchmark_amd import pointwise as pw
    c = rec.full(rec.case("iii", "fused", 8, 128, 128, (1, 3072)))
    d = layer_of(pw, c)
    assert pw._plan_fused(d, True) == "fused" and pw._plan_fused(d, True, relu=True) == "fused"
    assert pw._plan_fused(d, True, residual=True) == "fused"
    assert pw._plan_fused(d, True, relu=True, residual=True) == "composed"
    assert pw._plan_fused(d, False, relu=True, residual=True) == "composed"
    assert pw._plan_fused(d, True, float32_operands=False) == "composed"
    assert pw._float32(None, torch.zeros(2)) and not pw._float32(torch.zeros(2), torch.zeros(2, dtype=torch.float64))


REPLAY = [(n, c) for n, (c, _) in enumerate(rec.load_fixture()) if c["group"] != "ii"]
OFFSET_GRAD_OUT = [c for c in rec.all_cases() if c.get("fix") == "b"]


@pytest.mark.gpu
def test_live_traces_equal_the_recorded_ones():
    """Groups i and iii through the public entry points: the same library calls and operators as recorded."""
    rows, by_key = fixture()
    assert len(REPLAY) > 300
    bad = []
    for n, c in REPLAY:
        recorded = by_key[rec.key(twin(c))] if c.get("fix") == "b" else rows[n][1]
        if "error" in recorded and c.get("fix") != "b":          # (see the CPU test: the refused weight gradient)
            recorded = {"calls": recorded["calls"][:-1], "ops": sorted(set(recorded["ops"]) | {"conv_backward"}), "fn": recorded["fn"]}
        live = rec.run_case(c)[0]
        if live != recorded:
            bad.append((c, live, recorded))
    assert not bad, "%d rows, first: %r" % (len(bad), bad[:3])


@pytest.mark.gpu
@pytest.mark.parametrize("c", OFFSET_GRAD_OUT, ids=lambda c: "%s-%d-relu%d" % (c["entry"], c["cin"], bool(c.get("flags", {}).get("relu"))))
def test_offset_view_grad_out_gives_the_gradients_of_its_aligned_copy(c):
    """grad_out a view one float into its storage (not 16-byte aligned) through _PointwiseConv (96 -> 96 at 16384
    positions, 24 -> 24; with and without relu), _PointwiseConvFused and _PointwiseConvDual: every gradient torch.equal to
    the one from an aligned copy of the same values."""
    from mvp_benchmark_amd import pointwise as pw
    t = rec.build_inputs(c)
    inputs = [v for v in t.values() if v is not None and v.requires_grad]
    outs = rec.call_entry(pw, c, t)
    assert type(outs[0].grad_fn).__name__ in ("_PointwiseConvBackward", "_PointwiseConvFusedBackward", "_PointwiseConvDualBackward")
    aligned = rec.grad_outs(twin(c), outs)
    views = []
    for g in aligned:
        buf = torch.empty(g.numel() + 1, device=g.device)
        buf[1:] = g.flatten()
        views.append(buf[1:].view(g.shape))
        assert views[-1].data_ptr() % 16 == 4 and g.data_ptr() % 16 == 0
    want = torch.autograd.grad(outs, inputs, aligned, retain_graph=True)
    got = torch.autograd.grad(outs, inputs, views)
    assert len(got) == len(inputs) >= 2
    for a, b in zip(got, want):
        assert torch.equal(a, b)

