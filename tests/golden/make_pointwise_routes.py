"""Record which kernels every 1x1-convolution layer takes (mvp_benchmark_amd/pointwise.py) as
tests/golden/pointwise_routes.json.

Needs the GPU:
    python tests/golden/make_pointwise_routes.py
It drives the PUBLIC entry points only (pointwise_conv, pointwise_conv_fused, pointwise_conv_dual, pointwise_conv_max)
under the module's route selectors, so the same file runs unmodified on any commit: the committed fixture is what the
commit BEFORE the routing planner computed, and tests/test_pointwise_routes.py holds the planner (CPU) and the live
module (GPU) to it.

A row = a case and the index of the trace it produced.
  case   entry point, B / cin / cout / trailing dimensions, how x, the weight and grad_out lie in memory ("dense", "offset":
         a view one float into its storage, "permuted": a non-contiguous view), bias, the entry point's flags, which
         inputs require a gradient ("" = inference), the selectors that differ from DEFAULTS; fields at their default
         are left out.
  trace  calls: the library entry points in call order (the name `call` of the module, wrapped);
         ops:   which of the watched PyTorch operators ran, forward and backward (the CPU-side operator profiler: the
                backward pass runs on autograd's thread) -- operator classes, never kernel or solver names;
         fn:    the autograd nodes of the result's graph that are convolutions (_Pointwise* Functions or the library's);
         error: the exception's type where the call raised one.
Groups: "i" the parametrize lists of the pointwise tests of tests/test_gpu_harness.py, "ii" every distinct layer of one
training step of VRCNet / PCN / ECG and of PCN's eval step (collected by wrapping the entry points), "iii" the smallest
shapes on each side of every boundary of the routing rules.
"""
import importlib
import itertools
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIXTURE = os.path.join(HERE, "pointwise_routes.json")
DEV = "cuda:0"

DEFAULTS = dict(USE_MFMA=True, MFMA_TRAIN=True, MFMA_DGRAD=True, MFMA_WGRAD_MIN_CIN=1, MFMA_WGRAD_MIN_POSITIONS=16384,
                MFMA_MIN_CH=1, MFMA_SKINNY_FWD_MAX_CIN=136, LIBRARY_IS_GEMM=False)
CASE_DEFAULTS = dict(x="dense", w="dense", go="dense", bias=True, flags={}, grad="", sel={}, cout2=0, fix="", boundary="",
                     res="dense", cb="dense")      # (res / cb: the layouts of the residual and of cloud_bias -- no recorded row sets them)
WATCH = {"aten::convolution": "conv", "aten::convolution_backward": "conv_backward", "aten::bmm": "gemm",
         "aten::baddbmm": "gemm", "aten::mm": "gemm", "aten::matmul": "gemm", "aten::einsum": "einsum",
         "aten::threshold_backward": "threshold_backward"}
# what the coverage check demands of the written fixture: every kernel route of every pass is taken by some row
REQUIRED_CALLS = ("mvp_pointwise_mfma_ex", "mvp_pointwise_dgrad", "mvp_pointwise_wgrad_mfma_ex", "mvp_pointwise_wgrad",
                  "mvp_pointwise_mfma_max", "mvp_pointwise_max_backward")
REQUIRED_OPS = ("conv", "conv_backward", "gemm", "einsum", "threshold_backward")


def case(group, entry, B, cin, cout, tail, **kw):
    c = dict(group=group, entry=entry, B=B, cin=cin, cout=cout, tail=list(tail))
    kw["flags"] = {k: v for k, v in kw.get("flags", {}).items() if v}
    c.update({k: v for k, v in kw.items() if CASE_DEFAULTS[k] != v})
    return c


def full(c):
    return dict(CASE_DEFAULTS, **c)


def key(c):
    c = {k: v for k, v in c.items() if k not in ("group", "boundary", "fix")}
    return json.dumps(c, sort_keys=True)


# ---- group i: the parametrize lists of tests/test_gpu_harness.py ------------------------------------------------------------
WGRAD_TEST = [((32, 48, 16, 1024), 24, True), ((4, 24, 16, 3072), 24, False), ((8, 256, 1, 768), 16, True), ((8, 64, 3072), 4, True),
              ((3, 16, 1, 300), 64, True), ((2, 512, 1, 384), 32, False), ((2, 130, 5, 44), 33, True), ((1, 1, 4), 1, True),
              ((2, 7, 1028), 5, True), ((3, 64, 16, 516), 64, True), ((2, 33, 2052), 49, False), ((5, 17, 3, 8), 9, True)]
AUTOGRAD_TEST = ((128, 256, 768, False, 513), (128, 256, 768, True, 32), (64, 64, 512, True, 32), (256, 3, 300, False, 513),
                 (24, 24, 256, False, 513), (515, 128, 384, True, 32), (1090, 256, 256, False, 513), (96, 160, 1000, True, 32),
                 (272, 8, 768, True, 1), (3, 128, 512, True, 1), (8, 128, 768, True, 1), (68, 2, 1024, True, 1))
FUSED_TEST = [(8, 128, 128, 3072), (8, 16, 64, 3072), (64, 68, 2, 3072), (64, 512, 512, 384), (16, 256, 128, 1536)]
FUSED_FLAGS = [dict(relu_in=1), dict(relu_in=1, relu=1), dict(relu_in=1, residual=1, relu_after=1), dict(residual=1, relu_after=1),
               dict(residual=1), dict(relu=1, cloud_bias=1), dict(cloud_bias=1)]
MAX_TEST = [(8, 512, 1024, 2048), (3, 40, 33, 20), (64, 128, 96, 384), (2, 7, 9, 16384), (5, 64, 1024, 64), (1, 3, 2, 1)]


def _grad(bias, *more):
    return "".join(("x", "w", "b" if bias else "") + more)


def group_i():
    out = []
    for shape, cout, bias in WGRAD_TEST:
        B, cin, tail = shape[0], shape[1], shape[2:]
        for sel in ({}, {"MFMA_TRAIN": False}, {"USE_MFMA": False}):
            out.append(case("i", "conv", B, cin, cout, tail, bias=bias, grad=_grad(bias), sel=sel))
        if tail[-1] > 1:
            out.append(case("i", "conv", B, cin, cout, tail[:-1] + (tail[-1] - 1,), bias=bias, grad=_grad(bias)))
    for cin, cout, L, dgrad, wmin in AUTOGRAD_TEST:
        sel = {"MFMA_WGRAD_MIN_POSITIONS": 0, "MFMA_DGRAD": dgrad, "MFMA_WGRAD_MIN_CIN": wmin}
        for relu in (0, 1):
            out.append(case("i", "conv", 4, cin, cout, (L,), flags={"relu": relu}, grad="xwb", sel=sel))
    for B, cin, cout, L in FUSED_TEST:
        for fl in FUSED_FLAGS:
            out.append(case("i", "fused", B, cin, cout, (1, L), flags=fl,
                            grad=_grad(True, "r" if fl.get("residual") else "", "c" if fl.get("cloud_bias") else "")))
        out.append(case("i", "fused", B, cin, cout, (1, L), bias=False, flags=dict(relu_in=1, relu=1), grad="xw"))
        if cout % 32 == 0 and cin % 4 == 0:
            out.append(case("i", "dual", B, cin, cout, (1, L), bias=False, cout2=cout // 2 if cout > 32 else cout, grad="xw"))
    for B, cin, cout, L in MAX_TEST:
        out.append(case("i", "max", B, cin, cout, (L,), grad="xwb"))
    return out


# ---- group iii: both sides of every boundary of the rules ---------------------------------------------------------------------
BOUNDARIES = []      # a row's "boundary" field is "<index into this list>/<side>"


def _both(out, name, a, b, entry="conv", relus=(0, 1), grads=("", "xwb"), **b_only):
    """A boundary: the cases `a` and `b` (B, cin, cout, tail) differ by the one quantity the rule tests -- the shape, or a
    keyword (`b_only`) that side b alone carries."""
    if name not in BOUNDARIES:
        BOUNDARIES.append(name)
    number = BOUNDARIES.index(name)
    for side, (B, cin, cout, tail) in enumerate((a, b)):
        for relu, grad in itertools.product(relus, grads):
            out.append(case("iii", entry, B, cin, cout, tail, flags={"relu": relu}, grad=grad, boundary="%d/%d" % (number, side),
                            **(b_only if side else {})))


def group_iii():
    out = []
    _both(out, "cin 64|65, 3-d", (2, 64, 64, (256,)), (2, 65, 64, (256,)))
    _both(out, "cout 64|65, 4-d", (2, 64, 64, (4, 64)), (2, 64, 65, (4, 64)))
    _both(out, "L 1028|1027, small", (2, 32, 32, (1028,)), (2, 32, 32, (1027,)))
    _both(out, "L 1028|1027", (2, 96, 128, (1028,)), (2, 96, 128, (1027,)))
    _both(out, "positions 16384|16380", (4, 96, 96, (4096,)), (4, 96, 96, (4092,)))
    _both(out, "forward reduction 512|516", (64, 512, 128, (384,)), (64, 516, 128, (384,)))
    _both(out, "dgrad reduction 512|516", (64, 128, 512, (384,)), (64, 128, 516, (384,)))
    _both(out, "reduction 512|516 at L 124", (64, 512, 128, (124,)), (64, 516, 128, (124,)))
    _both(out, "output tiles 512|448", (8, 516, 1024, (1024,)), (8, 516, 1024, (896,)))
    _both(out, "skinny cin 136|140", (4, 136, 16, (4096,)), (4, 140, 16, (4096,)))
    _both(out, "cin % 4 with cout > 64", (4, 132, 96, (4096,)), (4, 130, 96, (4096,)))
    for shape in ((4, 96, 96, (4096,)), (2, 24, 24, (256,))):
        _both(out, "x dense|offset %d" % shape[1], shape, shape, x="offset")
        _both(out, "x dense|permuted %d" % shape[1], shape, shape, x="permuted")
        _both(out, "w dense|offset %d" % shape[1], shape, shape, w="offset")
        _both(out, "batch %d|0 at %d" % (shape[0], shape[1]), shape, (0,) + shape[1:])
    _both(out, "conv-max L 4428|4432", (2, 64, 1024, (4428,)), (2, 64, 1024, (4432,)), entry="max", relus=(0,))
    _both(out, "conv-max 7 -> 9 L 1024|16384", (2, 7, 9, (1024,)), (2, 7, 9, (16384,)), entry="max", relus=(0,))
    _both(out, "conv-max skinny cin 136|140", (4, 136, 16, (1024,)), (4, 140, 16, (1024,)), entry="max", relus=(0,))
    # the backward-route selectors (test_pointwise_conv_autograd_through_mfma's settings) and the global switches
    shapes = ((4, 96, 96, (4096,)), (4, 128, 256, (768,)), (2, 24, 24, (256,)), (2, 96, 96, (1027,)), (8, 1864, 768, (256,)))
    for B, cin, cout, tail in shapes:
        for dgrad, wmin in ((False, 513), (True, 32), (True, 1)):
            sel = {"MFMA_WGRAD_MIN_POSITIONS": 0, "MFMA_DGRAD": dgrad, "MFMA_WGRAD_MIN_CIN": wmin}
            for relu in (0, 1):
                out.append(case("iii", "conv", B, cin, cout, tail, flags={"relu": relu}, grad="xwb", sel=sel))
        for sel in ({"MFMA_TRAIN": False}, {"USE_MFMA": False}, {"LIBRARY_IS_GEMM": True}):
            for relu, grad in ((0, ""), (1, "xwb")):
                out.append(case("iii", "conv", B, cin, cout, tail, flags={"relu": relu}, grad=grad, sel=sel))
        # what needs a gradient decides whether grad_out is masked up front
        for grad, sel in itertools.product(("x", "wb"), ({}, {"MFMA_DGRAD": False})):
            out.append(case("iii", "conv", B, cin, cout, tail, flags={"relu": 1}, grad=grad, sel=sel))
    # the fused / dual entry points off their one-GEMM route
    for B, cin, cout, tail in ((8, 128, 128, (1, 3072)), (8, 130, 128, (1, 3072)), (2, 128, 128, (1, 3072)), (8, 1864, 768, (256,))):
        for grad in ("", "w", "xwb"):
            out.append(case("iii", "fused", B, cin, cout, tail, flags=dict(relu_in=1, relu=1), grad=grad))
            out.append(case("iii", "fused", B, cin, cout, tail, flags=dict(cloud_bias=1, relu=1), grad=grad + ("c" if grad else "")))
            out.append(case("iii", "dual", B, cin, cout, tail, bias=False, cout2=64, grad=grad.replace("b", "")))
    out.append(case("iii", "dual", 8, 128, 48, (1, 3072), bias=False, cout2=64, grad="xw"))           # c1 % 32 != 0
    out.append(case("iii", "fused", 8, 128, 128, (1, 3072), x="permuted", flags=dict(relu_in=1), grad="xwb"))
    out.append(case("iii", "fused", 8, 128, 128, (1, 3072), w="offset", flags=dict(relu_in=1), grad="xwb"))
    # grad_out an offset view (the rows whose trace the planner's backward no longer follows: `fix`)
    for relu in (0, 1):
        out.append(case("iii", "conv", 4, 96, 96, (4096,), flags={"relu": relu}, grad="xwb", go="offset", fix="b"))
        out.append(case("iii", "conv", 4, 24, 24, (4096,), flags={"relu": relu}, grad="xwb", go="offset", fix="b"))
        out.append(case("iii", "conv", 4, 24, 24, (4096,), flags={"relu": relu}, grad="xwb"))
    out.append(case("iii", "fused", 8, 128, 128, (1, 3072), flags=dict(relu_in=1), grad="xwb", go="offset", fix="b"))
    out.append(case("iii", "dual", 8, 128, 128, (1, 3072), bias=False, cout2=64, grad="xw", go="offset", fix="b"))
    return out


# ---- group ii: the layers of the models' steps ---------------------------------------------------------------------------------
def _view_of(t):
    return "permuted" if not t.is_contiguous() else "offset" if t.data_ptr() % 16 else "dense"


def collect_model_layers():
    """One training step of VRCNet / PCN / ECG and one eval step of PCN with the public entry points wrapped: the case of
    every top-level call (a composed route's inner pointwise_conv is the entry point's own business)."""
    import mvp_benchmark_amd.pointwise as pw
    seen, depth = [], [0]

    def wrap(name, describe):
        orig = getattr(pw, name)

        def wrapped(*a, **kw):
            if depth[0] == 0 and a[0].is_cuda and a[0].dtype == torch.float32:
                seen.append(describe(*a, **kw))
            depth[0] += 1
            try:
                return orig(*a, **kw)
            finally:
                depth[0] -= 1
        setattr(pw, name, wrapped)
        return orig

    def rg(*ts):
        on = torch.is_grad_enabled()
        return "".join(n for n, t in zip("xwbrc", ts) if on and t is not None and t.requires_grad)

    def base(entry, x, w, **kw):
        return case("ii", entry, x.size(0), w.size(1), w.size(0), tuple(x.shape[2:]), x=_view_of(x), w=_view_of(w), **kw)

    def d_conv(x, weight, bias=None, relu=False):
        return base("conv", x, weight, bias=bias is not None, flags={"relu": 1} if relu else {}, grad=rg(x, weight, bias))

    def d_fused(x, weight, bias=None, relu_in=False, relu=False, residual=None, relu_after=False, cloud_bias=None):
        flags = {k: 1 for k, v in dict(relu_in=relu_in, relu=relu, residual=residual is not None, relu_after=relu_after,
                                       cloud_bias=cloud_bias is not None).items() if v}
        return base("fused", x, weight, bias=bias is not None, flags=flags, grad=rg(x, weight, bias, residual, cloud_bias))

    def d_dual(x, w1, w2):
        return base("dual", x, w1, bias=False, cout2=w2.size(0), grad=rg(x, w1))

    def d_max(x, weight, bias=None):
        return base("max", x, weight, bias=bias is not None, grad=rg(x, weight, bias))

    originals = {n: wrap(n, d) for n, d in (("pointwise_conv", d_conv), ("pointwise_conv_fused", d_fused),
                                            ("pointwise_conv_dual", d_dual), ("pointwise_conv_max", d_max))}
    try:
        import train                                  # (the models bind the wrapped names at import)
        g = torch.Generator().manual_seed(0)
        for name in ("vrcnet", "pcn", "ecg"):
            args = train.load_config(os.path.join(ROOT, "completion", "cfgs", name + ".yaml"))
            args.load_model = None
            net = importlib.import_module("models." + name).Model(args).to(DEV).train()
            gt = torch.rand(32, 2048, 3, generator=g).to(DEV)
            _, _, loss = net(gt.transpose(2, 1).contiguous(), gt, alpha=0.5)
            loss.mean().backward()
            del net, loss
        args = train.load_config(os.path.join(ROOT, "completion", "cfgs", "pcn_eval16k.yaml"))
        args.eval_emd = False
        net = importlib.import_module("models.pcn").Model(args).to(DEV).eval()
        with torch.no_grad():
            net(torch.rand(32, 3, 2048, generator=g).to(DEV), torch.rand(32, 16384, 3, generator=g).to(DEV), prefix="val")
        del net
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    finally:
        for n, orig in originals.items():
            setattr(pw, n, orig)
    return seen


# ---- running a case ------------------------------------------------------------------------------------------------------------
def _draw(size, family, g):
    """The values of a tensor: randn (family None: what the fixture was recorded on), or a family of
    tests/conv_gradient_cases.py ("exact": integers in [-4, 4], "random": randn)."""
    if family is None:
        return torch.randn(size, generator=g)
    if os.path.dirname(HERE) not in sys.path:
        sys.path.insert(0, os.path.dirname(HERE))
    from conv_gradient_cases import values
    return values(tuple(size), family, g)


def _tensor(shape, view, g, family=None, device=DEV):
    """float32 tensor of `shape` on `device`: dense, one float into its storage, or a permuted (channels-last; 2-d:
    transposed) view."""
    n = 1
    for s in shape:
        n *= s
    if view == "offset":
        return _draw((n + 1,), family, g).to(device)[1:].view(shape)
    if view == "permuted":
        perm = (0,) + tuple(range(2, len(shape))) + (1,) if len(shape) > 2 else (1, 0)
        inv = [perm.index(i) for i in range(len(shape))]
        return _draw([shape[p] for p in perm], family, g).to(device).permute(inv)
    return _draw(shape, family, g).to(device)


def build_inputs(c, seed=0, family=None, device=DEV):
    """The tensors of a case: dict with x, w, b, w2, res, cb (None where absent), requires_grad set from c["grad"]."""
    c = full(c)
    g = torch.Generator().manual_seed(seed)
    B, cin, cout, tail = c["B"], c["cin"], c["cout"], tuple(c["tail"])
    ones = (1,) * len(tail)
    t = dict(x=_tensor((B, cin) + tail, c["x"], g, family, device), w=_tensor((cout, cin) + ones, c["w"], g, family, device),
             b=None, w2=None, res=None, cb=None)
    if c["bias"]:
        t["b"] = _draw((cout,), family, g).to(device)
    if c["cout2"]:
        t["w2"] = _draw((c["cout2"], cin) + ones, family, g).to(device)
    if c["flags"].get("residual"):
        t["res"] = _tensor((B, cout) + tail, c["res"], g, family, device)
    if c["flags"].get("cloud_bias"):
        t["cb"] = _tensor((B, cout), c["cb"], g, family, device)
    for letter, name in (("x", "x"), ("w", "w"), ("b", "b"), ("r", "res"), ("c", "cb")):
        if letter in c["grad"] and t[name] is not None:
            t[name].requires_grad_()
    if "w" in c["grad"] and t["w2"] is not None:
        t["w2"].requires_grad_()
    return t


def call_entry(pw, c, t):
    """The case's entry point on the tensors of build_inputs -> tuple of outputs."""
    c = full(c)
    fl = c["flags"]
    if c["entry"] == "conv":
        return (pw.pointwise_conv(t["x"], t["w"], t["b"], relu=bool(fl.get("relu"))),)
    if c["entry"] == "fused":
        return (pw.pointwise_conv_fused(t["x"], t["w"], t["b"], relu_in=bool(fl.get("relu_in")), relu=bool(fl.get("relu")),
                                        residual=t["res"], relu_after=bool(fl.get("relu_after")), cloud_bias=t["cb"]),)
    if c["entry"] == "dual":
        return tuple(pw.pointwise_conv_dual(t["x"], t["w"], t["w2"]))
    return (pw.pointwise_conv_max(t["x"], t["w"], t["b"]),)


def grad_outs(c, outs, seed=1, family=None):
    g = torch.Generator().manual_seed(seed)
    return [_tensor(tuple(o.shape), full(c)["go"], g, family, o.device) for o in outs]


def grad_inputs(t):
    """[(name, tensor)] of the tensors of build_inputs that require a gradient, in the order run_case returns theirs."""
    return [(k, v) for k, v in t.items() if v is not None and v.requires_grad]


def _graph_convs(outs):
    names, stack, seen = set(), [o.grad_fn for o in outs if o.grad_fn is not None], set()
    while stack:
        node = stack.pop()
        if node in seen:
            continue
        seen.add(node)
        name = type(node).__name__
        if name.startswith("_Pointwise") or name.startswith("Convolution"):
            names.add(name)
        stack.extend(n for n, _ in node.next_functions if n is not None)
    return sorted(names)


def run_case(c, tensors=None, grad_out=None, profiled=True):
    """-> (trace, outputs, gradients): the case run under its selectors with `call` wrapped and the operator profiler on
    (profiled=False: without it, trace["ops"] stays empty).  gradients: one per entry of grad_inputs(tensors), in that
    order, for grad_out (default: grad_outs(c, outputs)); None where the graph gave that input none -- the trace does not
    care, the value tests assert on it."""
    import contextlib
    import mvp_benchmark_amd.pointwise as pw
    from mvp_benchmark_amd._lib import MvpOpsError
    from torch.profiler import ProfilerActivity, profile
    c = full(c)
    saved = {k: getattr(pw, k) for k in DEFAULTS}
    calls, orig_call = [], pw.call

    def traced(name, *a):
        calls.append(name)
        return orig_call(name, *a)

    outs = grads = None
    trace = {"calls": calls, "ops": [], "fn": []}
    for k, v in dict(DEFAULTS, **c["sel"]).items():
        setattr(pw, k, v)
    pw.call = traced
    try:
        t = tensors or build_inputs(c)
        inputs = [v for _, v in grad_inputs(t)]
        with (profile(activities=[ProfilerActivity.CPU]) if profiled else contextlib.nullcontext()) as prof:
            try:
                with torch.enable_grad():
                    outs = call_entry(pw, c, t)
                    trace["fn"] = _graph_convs(outs)
                    if inputs:
                        grads = torch.autograd.grad(outs, inputs, grad_out or grad_outs(c, outs), allow_unused=True)
            except MvpOpsError as exc:         # a host-side refusal of the arguments (nothing was launched); anything else,
                if "HIP" in str(exc):          # a HIP error included, ends the run
                    raise
                trace["error"] = type(exc).__name__
            if t["x"].is_cuda:
                torch.cuda.synchronize()
        if profiled:
            trace["ops"] = sorted({WATCH[e.key] for e in prof.key_averages() if e.key in WATCH})
    finally:
        pw.call = orig_call
        for k, v in saved.items():
            setattr(pw, k, v)
    return trace, outs, grads


def all_cases():
    """The fixed case list of groups i and iii (group ii comes from the models' steps)."""
    out, seen = [], set()
    for c in group_i() + group_iii():
        k = key(c)
        if k in seen:
            continue
        seen.add(k)
        out.append(c)
    return out


def load_fixture():
    with open(FIXTURE) as f:
        blob = json.load(f)
    return [(c, blob["traces"][i]) for c, i in blob["rows"]]


def main():
    for path in (os.path.join(ROOT, "completion"), ROOT):          # (run as a script: the package and the models' modules)
        if path not in sys.path:
            sys.path.insert(0, path)
    assert torch.cuda.is_available(), "the recorder needs the GPU"
    cases = all_cases()
    have = {key(c) for c in cases}
    for c in collect_model_layers():
        if key(c) not in have:              # (duplicate descriptors dropped: a model row costs nothing to test, but bytes)
            have.add(key(c))
            cases.append(c)
    traces, rows = [], []
    for n, c in enumerate(cases):
        trace = run_case(c)[0]
        if trace not in traces:
            traces.append(trace)
        rows.append([c, traces.index(trace)])
        torch.cuda.empty_cache()
        print("%4d/%d %s -> %s" % (n + 1, len(cases), json.dumps(c, sort_keys=True), json.dumps(trace)), flush=True)
    # coverage: every kernel route of every pass in some row, a row on each side of every boundary
    calls = {name for t in traces for name in t["calls"]}
    ops = {op for t in traces for op in t["ops"]}
    fns = {fn for t in traces for fn in t["fn"]}
    assert all(name in calls for name in REQUIRED_CALLS), sorted(calls)
    assert all(op in ops for op in REQUIRED_OPS), sorted(ops)
    assert {"_PointwiseConvBackward", "_PointwiseConvFusedBackward", "_PointwiseConvDualBackward", "_PointwiseConvMaxBackward",
            "ConvolutionBackward0"} <= fns, sorted(fns)
    recorded = {key(c) for c, _ in rows}
    sides = {}
    for c in group_iii():
        if c.get("boundary"):
            assert key(c) in recorded, c
            sides.setdefault(c["boundary"][:-2], {}).setdefault(c["boundary"][-1], set()).add(key(c))
    assert all(set(s) == {"0", "1"} and not (s["0"] & s["1"]) for s in sides.values()), sides
    assert {"ii", "i", "iii"} == {c["group"] for c, _ in rows}
    with open(FIXTURE, "w") as f:
        json.dump({"defaults": DEFAULTS, "traces": traces, "rows": rows}, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print("wrote %s: %d rows, %d traces, %d bytes; torch %s" % (FIXTURE, len(rows), len(traces), os.path.getsize(FIXTURE),
                                                               torch.__version__))


if __name__ == "__main__":
    main()
