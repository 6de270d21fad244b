"""What the value tests of the 1x1-convolution entry points share (tests/test_pointwise_values_cpu.py,
tests/test_gpu_pointwise_values.py): float64 references of pointwise_conv, pointwise_conv_fused, pointwise_conv_dual and
pointwise_conv_max (mvp_benchmark_amd/pointwise.py) with their gradients as closed forms, the routes the planners name for
a case pass by pass, the extra cases the recorded fixture does not hold, and the comparison of one run with its reference.
Plain torch operators on whatever device the tensors are on; nothing of the op layer but its planners.

The cases are the ones tests/test_pointwise_routes.py replays for their call traces (groups i and iii of
tests/golden/make_pointwise_routes.py) plus EXTRA below; the tensors come from the recorder's build_inputs / grad_outs in
one of the two families of tests/conv_gradient_cases.py:
    exact    every tensor, grad_out included, holds integers in [-4, 4]: while every `mag` (the sum of the absolute values
             of the terms behind an element) stays below 2^24 no route rounds, whatever its summation order, and outputs
             and gradients EQUAL the reference.  Exact zeros of the activations are common, so the ReLU' convention at 0
             (aten.threshold_backward: 0 where the activation is <= 0) is under test.
    random   randn: every element within gamma(t) * mag of the reference, t = the number of float32 operations behind the
             element (the reduction length plus the epilogue's additions).  A ReLU's mask is taken from the operator's own
             float32 output (itself held to the bound), so a pre-activation within rounding of 0 cannot fail a gradient.
             Two configurations keep their gradients to the exact family -- the conv -> max entry (a near-tie of the
             maximum) and relu together with a residual (the inner mask is not visible in the output); their forward
             values still take the bound.
"""
import contextlib

import torch

import conv_gradient_cases as cg
import test_pointwise_routes as routes
from conv_gradient_cases import assert_equal, assert_exactly_representable, assert_within, gamma, values  # noqa: F401

rec = routes.rec
FAMILIES = cg.FAMILIES
LAYOUT_KEYS = ("x", "w", "go", "res", "cb")
VALUE_MAX = 4                        # the exact family's largest absolute value (conv_gradient_cases.values)


def threshold(g, a):
    """aten.threshold_backward(g, a, 0): 0 where a <= 0, g elsewhere."""
    return torch.where(a <= 0, torch.zeros_like(g), g)


def _conv(w2, x3):
    return torch.einsum("oi,bil->bol", w2, x3)


def _dgrad(w2, g3):
    return torch.einsum("oi,bol->bil", w2, g3)


def _wgrad(g3, x3):
    return torch.einsum("bol,bil->oi", g3, x3)


def _f64(t):
    return None if t is None else t.detach().double()


def out_shapes(c):
    """The shapes of the entry point's outputs, from the case alone."""
    c = rec.full(c)
    tail = tuple(c["tail"])
    if c["entry"] == "max":
        return [(c["B"], c["cout"])]
    if c["entry"] == "dual":
        return [(c["B"], c["cout"]) + tail, (c["B"], c["cout2"]) + tail]
    return [(c["B"], c["cout"]) + tail]


# ---------------------------------------------------------------------------------------------------------- the references
# Each returns {"out": [(value, mag, terms), ...], "grad": {name: (value, mag, terms)}} in float64: the names are those of
# build_inputs' tensors, `grad` holds the ones that require a gradient (nothing where gos is None).  y_op: the operator's
# own float32 outputs; where given, every ReLU' whose activation is an output is masked by them.

def ref_layer(t, flags, gos=None, y_op=None):
    """conv: [relu](W x + b); fused: act2(act1(W in(x) + (b + cb[b])) + res)."""
    x, w, b, res, cb = (t[k] for k in ("x", "w", "b", "res", "cb"))
    x3, w2 = _f64(x).flatten(2), _f64(w).flatten(1)
    B, cin, L = x3.shape
    cout = w2.size(0)
    shape = (B, cout) + tuple(x.shape[2:])
    xin = torch.relu(x3) if flags.get("relu_in") else x3
    pre, mag, terms = _conv(w2, xin), _conv(w2.abs(), xin.abs()), cin
    if b is not None or cb is not None:
        # the bias and the per-cloud vector are summed first (_one_bias): one addend per output
        one = _f64(b).view(1, cout, 1) if cb is None else _f64(cb).reshape(B, cout, 1) if b is None else \
            _f64(cb).reshape(B, cout, 1) + _f64(b).view(1, cout, 1)
        one_mag = (0 if b is None else _f64(b).abs().view(1, cout, 1)) + (0 if cb is None else _f64(cb).abs().reshape(B, cout, 1))
        pre, mag, terms = pre + one, mag + one_mag, terms + 1 + (b is not None and cb is not None)
    h = torch.relu(pre) if flags.get("relu") else pre
    z = h
    if res is not None:
        z, mag, terms = h + _f64(res).flatten(2), mag + _f64(res).flatten(2).abs(), terms + 1
    y = torch.relu(z) if flags.get("relu_after") else z
    ref = {"out": [(y.view(shape), mag.view(shape), terms)], "grad": {}}
    if gos is None:
        return ref
    g = _f64(gos[0]).flatten(2)
    outer = y if y_op is None else _f64(y_op[0]).flatten(2)
    if flags.get("relu_after"):
        g = threshold(g, outer)
    if res is not None and res.requires_grad:
        ref["grad"]["res"] = (g.view(shape), g.abs().view(shape), 0)
    if flags.get("relu"):
        # (with a residual the inner activation is no output: the reference's own -- the exact family)
        g = threshold(g, h if res is not None or y_op is None else outer)
    ga = g.abs()
    if cb is not None and cb.requires_grad:
        ref["grad"]["cb"] = (g.sum(2), ga.sum(2), L)
    if b is not None and b.requires_grad:
        ref["grad"]["b"] = (g.sum((0, 2)), ga.sum((0, 2)), B * L)
    if w.requires_grad:
        ref["grad"]["w"] = (_wgrad(g, xin).view(w.shape), _wgrad(ga, xin.abs()).view(w.shape), B * L)
    if x.requires_grad:
        gx = _dgrad(w2, g)
        if flags.get("relu_in"):
            gx = threshold(gx, x3)
        ref["grad"]["x"] = (gx.view(x.shape), _dgrad(w2.abs(), ga).view(x.shape), cout)
    return ref


def ref_dual(t, flags, gos=None, y_op=None):
    """(W1 x, W2 x); gx = W1^T g1 + W2^T g2 (the second product's epilogue adds the first)."""
    x, w1, w2 = t["x"], t["w"], t["w2"]
    x3 = _f64(x).flatten(2)
    B, cin, L = x3.shape
    ref = {"out": [], "grad": {}}
    for w in (w1, w2):
        shape = (B, w.size(0)) + tuple(x.shape[2:])
        wd = _f64(w).flatten(1)
        ref["out"].append((_conv(wd, x3).view(shape), _conv(wd.abs(), x3.abs()).view(shape), cin))
    if gos is None:
        return ref
    g1, g2 = (_f64(g).flatten(2) for g in gos)
    for name, w, g in (("w", w1, g1), ("w2", w2, g2)):
        if w.requires_grad:
            ref["grad"][name] = (_wgrad(g, x3).view(w.shape), _wgrad(g.abs(), x3.abs()).view(w.shape), B * L)
    if x.requires_grad:
        a, b = _f64(w1).flatten(1), _f64(w2).flatten(1)
        ref["grad"]["x"] = ((_dgrad(a, g1) + _dgrad(b, g2)).view(x.shape),
                            (_dgrad(a.abs(), g1.abs()) + _dgrad(b.abs(), g2.abs())).view(x.shape), a.size(0) + b.size(0) + 1)
    return ref


def ref_max(t, flags, gos=None, y_op=None):
    """(W x + b).max over the positions; the gradient goes to the FIRST position that attains the maximum (what torch.max
    reports).  The value's mag is the largest mag among the positions: |max a - max b| <= max |a - b|."""
    x, w, b = t["x"], t["w"], t["b"]
    x3, w2 = _f64(x).flatten(2), _f64(w).flatten(1)
    B, cin, L = x3.shape
    cout = w2.size(0)
    pre, mag, terms = _conv(w2, x3), _conv(w2.abs(), x3.abs()), cin
    if b is not None:
        pre, mag, terms = pre + _f64(b).view(1, cout, 1), mag + _f64(b).abs().view(1, cout, 1), terms + 1
    val = pre.amax(2)
    at = torch.arange(L, device=pre.device).view(1, 1, L).expand_as(pre)
    idx = torch.where(pre == val.unsqueeze(2), at, torch.full_like(at, L)).amin(2)          # (B, cout): the first maximum
    ref = {"out": [(val, mag.amax(2), terms)], "grad": {}, "idx": idx}
    if gos is None:
        return ref
    g = _f64(gos[0])
    where = idx.unsqueeze(1).expand(B, cin, cout)                    # [b, ci, co] -> the position (b, co) won
    if b is not None and b.requires_grad:
        ref["grad"]["b"] = (g.sum(0), g.abs().sum(0), B)
    if w.requires_grad:
        cols = torch.gather(x3, 2, where)
        ref["grad"]["w"] = (torch.einsum("bo,bio->oi", g, cols).view(w.shape),
                            torch.einsum("bo,bio->oi", g.abs(), cols.abs()).view(w.shape), B)
    if x.requires_grad:
        prods = g.unsqueeze(1) * w2.t().unsqueeze(0)                 # [b, ci, co] = g[b, co] w[co, ci]
        count = torch.zeros(B, L, dtype=torch.int64, device=g.device).scatter_add_(1, idx, torch.ones_like(idx))
        ref["grad"]["x"] = (torch.zeros_like(x3).scatter_add_(2, where, prods).view(x.shape),
                            torch.zeros_like(x3).scatter_add_(2, where, prods.abs()).view(x.shape),
                            count.unsqueeze(1).expand(B, cin, L).reshape(x.shape))
    return ref


REFERENCES = {"conv": ref_layer, "fused": ref_layer, "dual": ref_dual, "max": ref_max}


def reference(c, t, gos=None, y_op=None):
    c = rec.full(c)
    return REFERENCES[c["entry"]](t, c["flags"], gos, y_op)


def gradients_take_the_bound(c):
    """The random family holds this case's gradients to the bound (else: the exact family alone; see the module's text)."""
    c = rec.full(c)
    return c["entry"] != "max" and not (c["flags"].get("relu") and c["flags"].get("residual"))


def exact_mag_bounds(c):
    """The largest `mag` each output and gradient of a case can have in the exact family, from the shapes alone: every
    value is at most 4 in absolute value, every product at most 16."""
    c = rec.full(c)
    v, B, cin, cout, c2 = VALUE_MAX, c["B"], c["cin"], c["cout"], c["cout2"]
    L = 1
    for s in c["tail"]:
        L *= s
    fl = c["flags"]
    if c["entry"] == "max":
        # a cloud's channels may all win the same position: cout terms behind an element of gx
        return {"out": v * v * cin + v * c["bias"], "x": v * v * cout, "w": v * v * B, "b": v * B}
    if c["entry"] == "dual":
        return {"out": v * v * cin, "x": v * v * (cout + c2), "w": v * v * B * L, "w2": v * v * B * L}
    return {"out": v * v * cin + v * (bool(c["bias"]) + bool(fl.get("cloud_bias")) + bool(fl.get("residual"))),
            "x": v * v * cout, "w": v * v * B * L, "b": v * B * L, "cb": v * L, "res": v}


# -------------------------------------------------------------------------------------------- the routes the planners name
@contextlib.contextmanager
def selectors(pw, c):
    """The module under the route selectors of a case."""
    saved = {k: getattr(pw, k) for k in rec.DEFAULTS}
    try:
        for k, v in dict(rec.DEFAULTS, **rec.full(c)["sel"]).items():
            setattr(pw, k, v)
        yield
    finally:
        for k, v in saved.items():
            setattr(pw, k, v)


def _conv_routes(pw, d, relu, has_bias, grad):
    plan = pw._plan_conv(d, bool(grad))
    r = {"top": plan.via, "fwd": plan.fwd, "dgrad": None, "wgrad": None, "premask": False}
    if plan.via == "function":
        back = pw._plan_conv_backward(plan.layer, relu, has_bias, "x" in grad, "w" in grad, has_bias and "b" in grad)
        r.update(dgrad=back.dgrad, wgrad=back.wgrad, premask=back.premask)
    elif grad:
        r.update(dgrad="autograd" if "x" in grad else None, wgrad="autograd" if "w" in grad or (has_bias and "b" in grad) else None)
    return r


def planned_routes(pw, c):
    """{"top", "fwd", "dgrad", "wgrad", "premask"}: what the planners name for a case, the selectors already set.  `top` is
    the entry point's own choice (function / autograd / none; fused / composed; stacked / separate), the others the route
    of each pass (a pair where the dual entry runs two layers; None: the pass does not run)."""
    c = rec.full(c)
    d, fl, grad = routes.layer_of(pw, c), c["flags"], c["grad"]
    relu = bool(fl.get("relu"))
    if c["entry"] == "conv":
        return _conv_routes(pw, d, relu, c["bias"], grad)
    if c["entry"] == "fused":
        res, cb = bool(fl.get("residual")), bool(fl.get("cloud_bias"))
        if pw._plan_fused(d, "x" in grad, relu, res) == "fused":
            return {"top": "fused", "fwd": "fused", "dgrad": "fused" if "x" in grad else None,
                    "wgrad": "fused" if "w" in grad or "b" in grad else None, "premask": False}
        inner = "".join(g for g in grad if g in ("xw" if cb else "xwb"))
        fresh = d._replace(x_dense=True, x_aligned=True) if fl.get("relu_in") else d          # relu(x): a new tensor
        return dict(_conv_routes(pw, fresh, relu and not cb, c["bias"] and not cb, inner), top="composed")
    if c["entry"] == "dual":
        d2 = d._replace(cout=c["cout2"])
        if pw._plan_dual(d, d2, "x" in grad) == "stacked":
            return {"top": "stacked", "fwd": "stacked", "dgrad": "stacked" if "x" in grad else None,
                    "wgrad": "stacked" if "w" in grad else None, "premask": False}
        a, b = _conv_routes(pw, d, False, False, grad), _conv_routes(pw, d2, False, False, grad)
        return {"top": "separate", "fwd": (a["fwd"], b["fwd"]), "dgrad": (a["dgrad"], b["dgrad"]),
                "wgrad": (a["wgrad"], b["wgrad"]), "premask": False}
    plan = pw._plan_max(d, bool(grad))
    if plan.via == "autograd":
        return dict(_conv_routes(pw, d, False, c["bias"], grad), top="autograd")
    fwd = "fused" if plan.fwd == "fused" else _conv_routes(pw, d, False, c["bias"], "")["fwd"]
    back = pw._plan_max_backward(d._replace(dim=3)) if plan.via == "function" else None
    return {"top": plan.via, "fwd": fwd, "dgrad": back if "x" in grad else None,
            "wgrad": back if "w" in grad or (c["bias"] and "b" in grad) else None, "premask": False}


# the routes the header declares reproducible from run to run (include/mvpops.h): the MFMA kernels (plain, split-K, the fused
# and stacked forms, the row maximum), the few-channel kernels and the sparse conv -> max backward; not the library's
REPRODUCIBLE = {"mfma", "splitk", "small", "fused", "stacked", "sparse"}
PASS_OF = {"x": "dgrad", "w": "wgrad", "w2": "wgrad", "b": "wgrad", "res": "top", "cb": "top"}


def reproducible(route):
    return all(r in REPRODUCIBLE for r in (route if isinstance(route, tuple) else (route,)))


# ---------------------------------------------------------------------------------------------------------- the extra cases
def _extra(want, entry, B, cin, cout, tail, **kw):
    return rec.case("extra", entry, B, cin, cout, tail, **kw), want


def _extras():
    out = []
    fused_shape = (4, 32, 32, (4096,))               # 16384 positions: the fewest the fused route takes
    res_flags = dict(residual=1, relu_after=1)
    for res in ("dense", "offset", "permuted"):      # (the dense one is the twin of the other two)
        out.append(_extra({"top": "fused"}, "fused", *fused_shape, flags=res_flags, grad="xwbr", res=res))
        out.append(_extra({"top": "composed"}, "fused", 2, 32, 32, (64,), flags=res_flags, grad="xwbr", res=res))
    cb_flags = dict(cloud_bias=1, relu=1)
    for cb in ("dense", "permuted"):                 # cloud_bias a transposed (Cout, B) tensor
        out.append(_extra({"top": "fused"}, "fused", *fused_shape, flags=cb_flags, grad="xwbc", cb=cb))
        out.append(_extra({"top": "composed"}, "fused", 2, 32, 32, (64,), flags=cb_flags, grad="xwbc", cb=cb))
    # one input alone needs a gradient
    for grad in ("x", "b"):
        out.append(_extra({"top": "fused"}, "fused", *fused_shape, flags=dict(relu_in=1, relu=1), grad=grad))
        out.append(_extra({"top": "composed"}, "fused", 2, 32, 32, (64,), flags=dict(relu_in=1, relu=1), grad=grad))
    out.append(_extra({"top": "stacked"}, "dual", 4, 32, 32, (4096,), bias=False, cout2=64, grad="x"))
    out.append(_extra({"top": "separate"}, "dual", 2, 32, 32, (64,), bias=False, cout2=64, grad="x"))
    # the bias alone (a frozen weight) on each route of the weight gradient
    for relu in (0, 1):
        out.append(_extra({"wgrad": "mfma", "dgrad": None}, "conv", 4, 96, 96, (4096,), flags={"relu": relu}, grad="b"))
        out.append(_extra({"wgrad": "small", "dgrad": None}, "conv", 2, 24, 24, (256,), flags={"relu": relu}, grad="b"))
        out.append(_extra({"wgrad": "gemm", "dgrad": None}, "conv", 2, 96, 96, (1027,), flags={"relu": relu}, grad="b"))
        out.append(_extra({"wgrad": "miopen", "dgrad": None}, "conv", 2, 96, 96, (256,), flags={"relu": relu}, grad="b"))
    # conv -> max: each gradient alone, on the sparse kernel and (x a permuted view) on the PyTorch formulation
    for grad in ("x", "w", "b", "wb"):
        need = {"dgrad": None} if grad != "x" else {"wgrad": None}
        out.append(_extra(dict(need, top="function", **{"dgrad" if grad == "x" else "wgrad": "sparse"}),
                          "max", 3, 40, 33, (20,), grad=grad))
        out.append(_extra(dict(need, top="function", **{"dgrad" if grad == "x" else "wgrad": "torch"}),
                          "max", 3, 40, 33, (20,), grad=grad, x="permuted"))
    # 4-d inputs (B, C, H, W)
    out.append(_extra({"top": "fused"}, "fused", 2, 32, 32, (8, 1024), flags=dict(relu_in=1, residual=1, relu_after=1), grad="xwbr"))
    out.append(_extra({"top": "function", "fwd": "fused", "dgrad": "sparse", "wgrad": "sparse"}, "max", 3, 40, 33, (4, 5), grad="xwb"))
    out.append(_extra({"top": "function", "fwd": "library", "dgrad": "torch", "wgrad": "torch"}, "max", 3, 40, 33, (4, 5),
                      grad="xwb", x="permuted"))
    return out


EXTRA = _extras()                                    # [(case, the routes it is listed under)]
REPLAY = [c for _, c in routes.REPLAY]
CASES = REPLAY + [c for c, _ in EXTRA]


def case_id(c):
    c = rec.full(c)
    fl = "+".join(sorted(c["flags"])) or "plain"
    lay = "".join("-%s_%s" % (k, c[k]) for k in LAYOUT_KEYS if c[k] != "dense")
    sel = "".join("-%s=%s" % (k.replace("MFMA_", "").lower(), v) for k, v in sorted(c["sel"].items()))
    return "%s-%s-%dx%d-%dx%s%s-%s-g_%s%s%s" % (c["group"], c["entry"], c["B"], c["cin"], c["cout"], "x".join(map(str, c["tail"])),
                                               "-%d" % c["cout2"] if c["cout2"] else "", fl, c["grad"] or "none",
                                               "" if c["bias"] else "-nobias", lay + sel)


def has_layout(c):
    c = rec.full(c)
    return any(c[k] != "dense" for k in LAYOUT_KEYS)


def twin_of(c):
    """The same case with every tensor dense."""
    return {k: v for k, v in c.items() if k not in LAYOUT_KEYS + ("fix", "boundary")}


def dense_copy(v):
    """A tensor's values in a fresh dense, aligned block, requiring a gradient where the tensor does."""
    return None if v is None else v.detach().contiguous().clone().requires_grad_(v.requires_grad)


# -------------------------------------------------------------------------------------------------- one run, one comparison
def make_tensors(c, family, device):
    """(tensors, grad_outs | None) of a case in a family; grad_out is built from the case's output shapes."""
    t = rec.build_inputs(c, family=family, device=device)
    if not rec.grad_inputs(t):
        return t, None
    shaped = [torch.empty(s, device="meta") for s in out_shapes(c)]
    g = torch.Generator().manual_seed(1)
    return t, [rec._tensor(tuple(o.shape), rec.full(c)["go"], g, family, device) for o in shaped]


def check_gradient_presence(t, grads):
    """Every input that requires a gradient received one; nothing was accumulated into any tensor."""
    wanted = rec.grad_inputs(t)
    assert (grads is None and not wanted) or len(grads) == len(wanted), (len(wanted), grads is None)
    for (name, _), g in zip(wanted, grads or ()):
        assert g is not None, "no gradient for %s" % name
    for name, v in t.items():
        assert v is None or v.grad is None, name


def compare(c, family, t, gos, outs, grads):
    """Outputs and gradients of one run against the float64 reference under the family's rule -> elements compared."""
    what = case_id(c)
    ref = reference(c, t, gos, y_op=outs if family == "random" else None)
    bounds = exact_mag_bounds(c)
    count = 0
    assert len(outs) == len(ref["out"])
    named = [("out", o, r) for o, r in zip(outs, ref["out"])]
    if family == "exact" or gradients_take_the_bound(c):
        wanted = rec.grad_inputs(t)
        assert set(ref["grad"]) == {name for name, _ in wanted}, (sorted(ref["grad"]), [n for n, _ in wanted])
        named += [(name, g, ref["grad"][name]) for (name, _), g in zip(wanted, grads or ())]
    if family == "exact":
        for name, _, (_, mag, _) in named:              # before any comparison
            assert mag.numel() == 0 or float(mag.max()) <= bounds[name] < cg.EXACT_LIMIT, (what, name, float(mag.max()))
    for name, got, (want, mag, terms) in named:
        got = got.detach().contiguous()                  # (copied out of its view)
        if family == "exact":
            assert_equal(got, want, "%s %s" % (name, what))
        else:
            assert_within(got, want, mag, terms, "%s %s" % (name, what))
        count += got.numel()
    return count
