"""The float64 references of tests/pointwise_value_cases.py, checked without a GPU: against autograd of the same functions
written with F.conv1d, relu, + and max; that the exact family cannot round at any replayed or extra shape; that every
extra case takes the route it is listed under; and the entry points themselves on host tensors (the composed / autograd
routes and the PyTorch formulation of the conv -> max backward) under the extra cases' gradient subsets."""
import json

import pytest
import torch
import torch.nn.functional as F

import pointwise_value_cases as pv

rec = pv.rec


def small(c):
    """The case at 2 x (5 -> 6 [and 3]) x 8 positions (4-d: 2 x 4), everything else kept."""
    c = rec.full(c)
    out = dict(c, B=2 if c["B"] else 0, cin=5, cout=6, tail=[8] if len(c["tail"]) == 1 else [2, 4], cout2=3 if c["cout2"] else 0, sel={})
    return {k: v for k, v in out.items() if rec.CASE_DEFAULTS.get(k) != v}


def flag_sets():
    """One small case per distinct entry point, flag set, bias, gradient subset, input rank and layout of the case list."""
    seen, out = set(), []
    for c in pv.CASES:
        s = small(c)
        k = json.dumps({k: v for k, v in s.items() if k not in ("group", "boundary", "fix")}, sort_keys=True)
        if k not in seen:
            seen.add(k)
            out.append(s)
    return out


FLAG_SETS = flag_sets()


def composed(c, t64):
    """The entry point written with F.conv1d, relu, + and max on float64 leaves -> tuple of outputs."""
    c = rec.full(c)
    fl = c["flags"]
    x = t64["x"]
    flat = x.flatten(2)

    def conv(inp, w, b=None):
        return F.conv1d(inp, w.flatten(1).unsqueeze(2), b)

    if c["entry"] == "dual":
        return tuple(conv(flat, w).view((x.size(0), w.size(0)) + tuple(x.shape[2:])) for w in (t64["w"], t64["w2"]))
    if c["entry"] == "max":
        return (conv(flat, t64["w"], t64["b"]).max(dim=2)[0],)
    inp = torch.relu(flat) if fl.get("relu_in") else flat
    if t64["cb"] is not None:
        one = t64["cb"] if t64["b"] is None else t64["cb"] + t64["b"]
        h = conv(inp, t64["w"]) + one.unsqueeze(2)
    else:
        h = conv(inp, t64["w"], t64["b"])
    if fl.get("relu"):
        h = torch.relu(h)
    if t64["res"] is not None:
        h = h + t64["res"].flatten(2)
    if fl.get("relu_after"):
        h = torch.relu(h)
    return (h.view((x.size(0), t64["w"].size(0)) + tuple(x.shape[2:])),)


@pytest.mark.parametrize("family", pv.FAMILIES)
def test_references_equal_autograd_of_the_composed_float64_function(family):
    """Closed forms against torch.autograd.grad of the float64 graph: equal on integers, within 1e-12 relative on randn
    (the two sum in different orders)."""
    assert len(FLAG_SETS) > 40
    entries = set()
    for c in FLAG_SETS:
        t, gos = pv.make_tensors(c, family, "cpu")
        t64 = {k: None if v is None else v.detach().double().requires_grad_(v.requires_grad) for k, v in t.items()}
        outs = composed(c, t64)
        ref = pv.reference(c, t, gos)
        assert len(outs) == len(ref["out"]) == len(pv.out_shapes(c))
        pairs = [("out", o.detach(), r[0]) for o, r in zip(outs, ref["out"])]
        wanted = rec.grad_inputs(t)
        assert set(ref["grad"]) == {name for name, _ in wanted}
        if wanted:
            grads = torch.autograd.grad(outs, [t64[name] for name, _ in wanted], [g.double() for g in gos])
            pairs += [(name, g, ref["grad"][name][0]) for (name, _), g in zip(wanted, grads)]
        for name, got, want in pairs:
            assert got.shape == want.shape, (c, name)
            if family == "exact":
                assert torch.equal(got, want), (c, name)
            else:
                scale = float(want.abs().max()) if want.numel() else 0.0
                assert float((got - want).abs().max() if want.numel() else 0.0) <= 1e-12 * scale, (c, name)
        # the mags: at least the value's size, the shapes' bound in the exact family, the term counts of the right shape
        for name, (value, mag, terms) in [("out", r) for r in ref["out"]] + list(ref["grad"].items()):
            assert mag.shape == value.shape and bool((mag >= value.abs()).all()), (c, name)
            assert (pv.gamma(terms) * mag).shape == value.shape
            if family == "exact" and mag.numel():
                assert float(mag.max()) <= pv.exact_mag_bounds(c)[name], (c, name)
        entries.add(rec.full(c)["entry"])
    assert entries == {"conv", "fused", "dual", "max"}


def test_first_maximum_and_relu_at_zero_are_the_conventions_under_test():
    """On integers the maximum is tied and activations are exactly 0 all over: the reference sends the gradient to the first
    maximum and through no activation that is 0."""
    c = rec.case("extra", "max", 2, 2, 6, (64,), grad="xwb")
    t, gos = pv.make_tensors(c, "exact", "cpu")
    ref = pv.reference(c, t, gos)
    pre = F.conv1d(t["x"].detach().double(), t["w"].detach().double(), t["b"].detach().double())
    tied = (pre == pre.amax(2, keepdim=True)).sum(2) > 1
    assert bool(tied.any())
    for b, co in tied.nonzero().tolist():
        first = int((pre[b, co] == pre[b, co].max()).nonzero()[0])
        assert int(ref["idx"][b, co]) == first
    c = rec.case("extra", "fused", 2, 5, 6, (256,), flags=dict(relu=1), grad="xwb")
    t, gos = pv.make_tensors(c, "exact", "cpu")
    ref = pv.reference(c, t, gos)
    y = ref["out"][0][0]
    zero = (y == 0) & (F.conv1d(t["x"].detach().double(), t["w"].detach().double(), t["b"].detach().double()) == 0)
    assert bool(zero.any())
    gb = torch.where(y > 0, gos[0].double(), torch.zeros(())).sum((0, 2))
    assert torch.equal(ref["grad"]["b"][0], gb)


def test_exact_family_cannot_round_at_any_case():
    """From the shapes alone: every mag of every replayed and extra case stays below 2^24."""
    assert len(pv.REPLAY) > 300 and len(pv.EXTRA) > 30
    worst = 0
    for c in pv.CASES:
        for name, bound in pv.exact_mag_bounds(c).items():
            assert bound < pv.cg.EXACT_LIMIT, (c, name, bound)
            worst = max(worst, bound)
    print("largest mag bound: %d of %d" % (worst, int(pv.cg.EXACT_LIMIT)))
    ids = [pv.case_id(c) for c in pv.CASES]
    assert len(set(ids)) == len(ids)


def test_every_extra_case_takes_the_route_it_is_listed_under():
    from mvp_benchmark_amd import pointwise as pw
    for c, want in pv.EXTRA:
        with pv.selectors(pw, c):
            planned = pv.planned_routes(pw, c)
        assert {k: planned[k] for k in want} == want, (c, planned)
    # every layout variant has its dense twin in the list
    keys = {rec.key(c) for c in pv.CASES}
    for c, _ in pv.EXTRA:
        if pv.has_layout(c):
            assert rec.key(pv.twin_of(c)) in keys, c


@pytest.mark.parametrize("family", pv.FAMILIES)
@pytest.mark.parametrize("c", [small(c) for c, _ in pv.EXTRA], ids=lambda c: pv.case_id(c))
def test_entry_points_on_host_tensors_equal_the_reference(c, family):
    """The composed / autograd routes and the PyTorch formulation of the conv -> max backward, float32 on the CPU, under the
    extra cases' layouts and gradient subsets."""
    t, gos = pv.make_tensors(c, family, "cpu")
    trace, outs, grads = rec.run_case(c, t, grad_out=gos, profiled=False)
    assert "error" not in trace and trace["calls"] == [], trace
    pv.check_gradient_presence(t, grads)
    assert pv.compare(c, family, t, gos, outs, grads) > 0
