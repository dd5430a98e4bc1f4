"""No GPU: tests/conv_family_checks.py itself.  The checker passes a float32 torch stand-in for hip_ops on the two smallest
shapes of every record, fails each planted fault by the name of the quantity, and its table covers hip_ops."""
import os
import re
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

import conv_family_checks as C
from conv2d_f32_helpers import ROOT

CPU = torch.device("cpu")


def torch_f32_ops(fam):
    """The three entry points of `fam` in float32 CPU torch: the family's op and its autograd."""
    def grads(x, w, dy, dy_gate):
        x, w = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
        dyg = dy if dy_gate is None else dy * (dy_gate > 0)
        return (*torch.autograd.grad(fam.op(x, w, None, **fam.op_kw), (x, w), dyg), dyg.transpose(0, 1).flatten(1).sum(1))

    def fwd(x, w, b, relu=False, **kw):
        y = fam.op(x, w, b, **fam.op_kw)
        return y.relu() if relu else y

    def bwd_data(dy, dy_gate, w, x_gate, x_shape, **kw):
        dx = grads(torch.zeros(x_shape), w, dy, dy_gate)[0]
        return dx if x_gate is None else dx * (x_gate > 0)

    def bwd_weight(x, dy, dy_gate, w_shape, **kw):
        return grads(x, torch.zeros(w_shape), dy, dy_gate)[1:]

    return SimpleNamespace(**dict(zip(fam.entry_points(), (fwd, bwd_data, bwd_weight))))


@pytest.mark.parametrize("fam", C.FAMILIES, ids=lambda f: f.name)
def test_checker_accepts_float32_torch(fam):
    for shape in sorted(fam.shapes, key=lambda s: torch.Size(s).numel())[:2]:      # the two smallest, at every channel pair
        for c_in, c_out in fam.pairs:
            C.check_family(torch_f32_ops(fam), CPU, fam, c_in, c_out, shape)


# ---- planted faults: the pass at fault is the stand-in's true pass `f` behind a wrapper ------------------------------------
FWD, DX, DW = 0, 1, 2      # index into Family.entry_points()


def _drop_tap(f):
    def fwd(x, w, b, **kw):
        w = w.clone()
        w[1, 5, 2, 0] = 0.0
        return f(x, w, b, **kw)
    return fwd


def _one_bit_on_second_call(f):
    calls = []

    def faulty(*a):
        out = f(*a)
        calls.append(1)
        if len(calls) % 2:
            return out
        first = (out[0] if isinstance(out, tuple) else out).clone()
        first.view(torch.int32).view(-1)[0] ^= 1
        return (first, *out[1:]) if isinstance(out, tuple) else first
    return faulty


def _on_dw(edit):
    """The weight gradient with edit(dw) in place of dw."""
    return lambda f: lambda *a: (edit(f(*a)[0]), f(*a)[1])


def _opened(gate):
    """A gate whose exact zeros read as open."""
    return None if gate is None else gate + (gate == 0)


def _conv_order(dw):
    return dw.transpose(0, 1).contiguous()


def _double_tap_1(dw):
    dw = dw.clone()
    dw[:, :, 1] *= 2
    return dw


def _touch(index):
    """The data gradient with a tiny nonzero at dx[index]."""
    def make(f):
        def bwd_data(*a):
            dx = f(*a).clone()
            dx[index] += 1e-20
            return dx
        return bwd_data
    return make


def _abs(gate):
    """A gate whose negatives read as open."""
    return None if gate is None else gate.abs()


def _swap_frames(dw):
    return torch.cat((dw[32:64], dw[:32], dw[64:]))


S2 = ("conv2d_s2", 32, 32, (2, 4, 4))      # even sides: an unread last row and column
WIDE = ("conv2d_wide_s2", 128, 128, (2, 5, 7))
# what is wrong: (family, c_in, c_out, shape), the pass, true pass -> faulty pass, the failing assertion's message
FAULTS = {
    "one (channel, tap) of the weight dropped": (WIDE, FWD, _drop_tap, r"y relu \+ bias"),
    "bias ignored": (S2, FWD, lambda f: lambda x, w, b, **kw: f(x, w, None, **kw), r"y relu \+ bias"),
    "relu applied at relu=False": (S2, FWD, lambda f: lambda x, w, b, relu: f(x, w, b, relu=True), r"y bias, no relu"),
    "dy_gate ignored in dx": (S2, DX, lambda f: lambda dy, dg, w, xg, s: f(dy, None, w, xg, s), r"dx gates True True"),
    "dy_gate ignored in dw": (S2, DW, lambda f: lambda x, dy, dg, s: (f(x, dy, None, s)[0], f(x, dy, dg, s)[1]), r"dy_gate True: dw:"),
    "x_gate ignored": (S2, DX, lambda f: lambda dy, dg, w, xg, s: f(dy, dg, w, None, s), r"dx gates True True"),
    "an x_gate of exactly 0 left open": (S2, DX, lambda f: lambda dy, dg, w, xg, s: f(dy, dg, w, _opened(xg), s), r"dx gates True True"),
    "a dy_gate of exactly 0 left open": (S2, DW, lambda f: lambda x, dy, dg, s: f(x, dy, _opened(dg), s), r"dy_gate True: dw:"),
    "a negative x_gate left open": (S2, DX, lambda f: lambda dy, dg, w, xg, s: f(dy, dg, w, _abs(xg), s), r"dx gates True True"),
    "a negative dy_gate left open": (S2, DW, lambda f: lambda x, dy, dg, s: f(x, dy, _abs(dg), s), r"dy_gate True: dw:"),
    "a nonzero in the unread last column of dx": (S2, DX, _touch((0, 0, 0, -1)), r"unread last column"),
    "a nonzero in the unread last row of dx": (S2, DX, _touch((0, 0, -1, 0)), r"unread last row"),
    "dw with two frames swapped": (("convt2d_s2_frames", 128, 32, (2, 2, 5)), DW, _on_dw(_swap_frames), r"dy_gate True: dw"),
    "a head's second forward differs in one bit": (("conv2d_head_s2", 32, 1, (2, 4, 5)), FWD, _one_bit_on_second_call, r"y forward: the bits"),
    "dw in Conv order, square": (("convt2d_s2", 32, 32, (2, 2, 5)), DW, _on_dw(_conv_order), r"dy_gate True: dw:"),
    "dw in Conv order": (("convt2d_s2", 32, 16, (2, 2, 5)), DW, _on_dw(_conv_order), r"dw shape"),
    "db from ungated dy": (S2, DW, lambda f: lambda x, dy, dg, s: (f(x, dy, dg, s)[0], f(x, dy, None, s)[1]), r"dy_gate True: db:"),
    "a second weight gradient differs in one bit": (S2, DW, _one_bit_on_second_call, r"dw, db: the bits differ run to run"),
    "3-D: one depth tap of dw doubled": (("conv3d_s2", 8, 32, (2, 3, 4, 4)), DW, _on_dw(_double_tap_1), r"dw depth tap 1"),
}


@pytest.mark.parametrize("fault", FAULTS)
def test_checker_rejects(fault):
    (name, c_in, c_out, shape), which, make, message = FAULTS[fault]
    fam = C.BY_NAME[name]
    ops = torch_f32_ops(fam)
    entry = fam.entry_points()[which]
    setattr(ops, entry, make(getattr(ops, entry)))
    with pytest.raises(AssertionError, match=message):
        C.check_family(ops, CPU, fam, c_in, c_out, shape)


# ---- the layers that come in two strides, on float32 torch stand-ins ----------------------------------------------------------
def _weight_grads(op, op_kw, x, dy, dy_gate, w_shape):
    w = torch.zeros(w_shape, requires_grad=True)
    dyg = dy if dy_gate is None else dy * (dy_gate > 0)
    return torch.autograd.grad(op(x, w, None, **op_kw), w, dyg)[0], dyg.sum((0, 2, 3))


def _first_layer_ops(twin, n_in, build):
    """fwd(*inputs, w, b, ...) and bwd_weight(*inputs, dy, w_shape, ...) of a first layer whose float32 input is
    build(*inputs), n_in tensors."""
    return SimpleNamespace(**{
        f"{twin.stem}_fwd_f32": lambda *a: F.conv2d(build(*a[:n_in]), a[n_in], a[n_in + 1], **twin.op_kw).relu(),
        f"{twin.stem}_bwd_weight_f32": lambda *a: _weight_grads(F.conv2d, twin.op_kw, build(*a[:n_in]), a[n_in], None, a[n_in + 1])})


@pytest.mark.parametrize("twin", C.STRIPE_LAYERS, ids=lambda t: t.stem)
def test_stripe_checker_accepts_float32_torch(twin):
    from nb10_reference import stripe_plane64
    ops = _first_layer_ops(twin, 2, lambda hist, starts: torch.cat((hist.double(), stripe_plane64(starts, *hist.shape[2:])), 1).float())
    for n_hist in C.N_HIST:
        C.check_stripe_layer(ops, CPU, twin, n_hist, twin.shapes[1])


@pytest.mark.parametrize("twin", C.COUNTS_LAYERS, ids=lambda t: t.stem)
def test_counts_checkers_accept_float32_torch(twin):
    from nb15_reference import input64
    ops = _first_layer_ops(twin, 3, lambda hist, flow, hor: input64(hist, flow, hor).float())
    C.check_counts_layer(ops, CPU, twin, twin.shapes[-1])
    C.check_counts_layer_input_dtypes(ops, CPU, twin)


@pytest.mark.parametrize("twin", C.HORIZON_LAYERS, ids=lambda t: t.stem)
def test_horizon_checker_accepts_float32_torch(twin):
    def x33(x, horizon):
        return torch.cat((x, horizon.view(-1, 1, 1, 1).expand(x.shape[0], 1, *x.shape[2:])), 1)

    def fwd(x, horizon, w, b, relu):
        y = F.conv_transpose2d(x33(x, horizon), w, b, **twin.op_kw)
        return y.relu() if relu else y
    ops = torch_f32_ops(C.BY_NAME[twin.plain])
    setattr(ops, f"{twin.stem}_fwd_f32", fwd)
    setattr(ops, f"{twin.stem}_bwd_weight_f32",
            lambda x, horizon, dy, dy_gate, w_shape: _weight_grads(F.conv_transpose2d, twin.op_kw, x33(x, horizon), dy, dy_gate, w_shape))
    for shape in twin.shapes[:3]:
        C.check_horizon_conv_transpose(ops, CPU, twin, shape)


# ---- the table against the library -----------------------------------------------------------------------------------------
def test_table_covers_hip_ops():
    from predict_pv_yield_amd import hip_ops
    stems = {n[:-len("_bwd_data_f32")] for n in dir(hip_ops) if n.endswith("_bwd_data_f32") and not n.startswith("_")}
    tabled = {f.stem or f.name for f in C.FAMILIES}
    assert stems - tabled - set(C.EXEMPT) == set(), "a conv family of hip_ops is neither in FAMILIES nor in EXEMPT"
    assert (tabled | set(C.EXEMPT)) - stems == set(), "FAMILIES or EXEMPT names a family hip_ops does not have"
    assert tabled & set(C.EXEMPT) == set()
    for fam in C.FAMILIES:
        for name in fam.entry_points():
            assert callable(getattr(hip_ops, name, None)), name
    for twin in C.STRIPE_LAYERS + C.COUNTS_LAYERS + C.HORIZON_LAYERS:
        for name in [f"{twin.stem}_fwd_f32", f"{twin.stem}_bwd_weight_f32"] + [f"{twin.plain}_bwd_data_f32"] * bool(twin.plain):
            assert callable(getattr(hip_ops, name, None)), name
    assert len(C.BY_NAME) == len(C.FAMILIES) and len(C.TWINS) == 6, "two records share a name"
    for stem, (reason, test) in C.EXEMPT.items():      # the covering test is there
        path, _, func = test.split(" ")[0].partition("::")
        assert reason and os.path.exists(os.path.join(ROOT, path)), (stem, test)
        assert re.search(rf"^def {func}\(", open(os.path.join(ROOT, path)).read(), re.M) if func else True, (stem, test)


def test_every_record_is_run_by_a_gpu_test():
    """cases_of / twin_shapes note which test runs a record as the GPU test files are imported: none is left out."""
    import glob
    import importlib
    for path in glob.glob(os.path.join(ROOT, "tests", "test_gpu_*.py")):
        if "conv_family_checks" in open(path).read():
            importlib.import_module(os.path.basename(path)[:-3])
    assert set(C.RUN_BY) == set(C.BY_NAME) | set(C.TWINS), set(C.BY_NAME) | set(C.TWINS) - set(C.RUN_BY)
