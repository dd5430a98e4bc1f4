"""The kernel-level check of every plain f32 conv family of hip_ops, stated once: forward, data gradient and weight / bias
gradient against float64 on the CPU.  The tests of a family keep their ids in the notebook's or experiment's own file
(tests/test_gpu_nbXX.py, tests/test_gpu_exp00X.py): each is parametrised by cases_of (twin_shapes for a layer that comes in
two strides) over the record's channel pairs and shapes under its old id format, and calls the checker.
tests/test_conv_family_checks_cpu.py runs the checker without a GPU on a float32 torch stand-in, with and without planted
faults, and holds the table to hip_ops and to those files.

A family is the three entry points  <stem>_fwd_f32(x, weight, bias, relu),  <stem>_bwd_data_f32(dy, dy_gate, weight, x_gate,
x_shape)  and  <stem>_bwd_weight_f32(x, dy, dy_gate, weight_shape).  The float64 references all come from one place: autograd
through the family's torch op (F.conv2d, F.conv_transpose2d or F.conv3d with the family's stride and padding), so Conv and
ConvTranspose, 2-D and 3-D need no adjoint written by hand.  The scale of an element's bound is the same op on the absolute
values: its output for the forward, its input gradient for dx.

Tolerances are conv2d_f32_helpers': ELEM_TOL per element relative to the element's float64 sum of |products| (an element whose
sum is exactly 0 must be exactly 0), NORM_TOL relative norm for the reductions dw and db.  The kernels multiply in exact f32
with f32 accumulation; a float32 running sum's error relative to sum|p| does not grow with K.

Shapes are those of the layer's input without the channel axis: (batch, height, width), or (batch, depth, height, width).
"""
import math
from typing import Callable, NamedTuple

import pytest
import torch
import torch.nn.functional as F

from conv2d_f32_helpers import NORM_TOL, _rel, _within
from notebook_model_checks import _counts, _g, _randn

GATES = ((True, True), (False, False))                # (dy_gate, x_gate): every gradient with and without its gates
ALL_GATES = ((True, True), (True, False), (False, True), (False, False))
HEAD_GATES = ((False, True), (False, False))          # no ReLU follows a head: x_gate only


class Family(NamedTuple):
    name: str                       # the key in BY_NAME; the hip_ops stem unless `stem` is given
    op: Callable                    # the float64 reference: F.conv2d, F.conv_transpose2d or F.conv3d
    op_kw: dict                     # its stride and padding
    kernel: tuple                   # (3, 3) or (2, 3, 3)
    pairs: tuple                    # ((c_in, c_out), ...)
    shapes: tuple
    seed: Callable                  # (c_in, c_out, *shape) -> the generator's seed
    stem: str = ""
    kwargs: dict = {}               # passed through to the three entry points
    gates: tuple = GATES
    x_is_relu_output: bool = False  # the input is a ReLU output, as in the model: half of it exact zeros
    relu: bool = True               # False: a head, whose forward is called without `relu`; its forward's bits are compared too
    no_dx_at_c_in: tuple = ()       # input channel counts at which the family has no data gradient
    reads_every_row: bool = True    # False: stride 2 without padding leaves the last row / column of an even side unread
    dw_groups: int = 1              # dw also in this many equal groups of its first axis, each against float64 on its own
    same_bits: bool = True          # two weight-gradient calls give identical bits (False needs a reason beside it)

    @property
    def transposed(self):
        return self.op is F.conv_transpose2d

    def entry_points(self):
        return tuple(f"{self.stem or self.name}_{p}_f32" for p in ("fwd", "bwd_data", "bwd_weight"))


_s2 = {"stride": 2}
_s122 = {"stride": (1, 2, 2)}

FAMILIES = (
    # experiment 002 (csrc/conv2d_f32.hip)
    Family("conv2d", F.conv2d, {}, (3, 3), ((32, 32), (32, 4)),
           ((32, 30, 30), (32, 28, 28), (1, 3, 3), (3, 7, 11), (1, 13, 13), (3, 13, 13)),
           lambda ci, co, n, h, w: n * 1000 + h * 10 + w + co, x_is_relu_output=True),
    # experiment 001 (csrc/conv2d_pool_f32.hip)
    Family("conv2d144", F.conv2d, {}, (3, 3), ((144, 144),), ((2, 13, 13), (1, 3, 3), (3, 7, 11), (1, 45, 50)),
           lambda ci, co, n, h, w: n * 1000 + h * 10 + w + 7, x_is_relu_output=True),
    # notebook 16 (csrc/conv2d_ae_f32.hip).  Widths 128, 127, 44, 38, 36, 11 -- multiples and non-multiples of every tile
    # extent; the last at a size that takes the general Conv3d route (>= 32768 output positions)
    Family("conv2d_ae", F.conv2d, {}, (3, 3), ((16, 32), (32, 32)),
           ((1, 128, 128), (1, 21, 127), (2, 44, 44), (3, 38, 38), (2, 36, 36), (2, 11, 11), (3, 128, 128)),
           lambda ci, co, n, h, w: 200 + w + ci, gates=GATES + ((True, False),)),
    Family("convt2d_ae", F.conv_transpose2d, {}, (3, 3), ((32, 32), (32, 16), (16, 16), (16, 1)),
           ((1, 40, 40), (2, 3, 126), (3, 10, 9), (2, 46, 46), (1, 1, 1)),
           lambda ci, co, n, h, w: 400 + w + ci + co, gates=ALL_GATES),
    # notebooks 14 / 15 (csrc/conv2d_s2_f32.hip).  One output; one output with an unread row and column; an unread column
    # only; even sides over several tiles; the model's second layer at full size; full width over several row bands
    Family("conv2d_s2", F.conv2d, _s2, (3, 3), ((16, 32), (32, 32)),
           ((1, 3, 3), (2, 4, 4), (3, 7, 12), (2, 26, 26), (1, 63, 63), (2, 15, 128)),
           lambda ci, co, n, h, w: 200 + w + ci, reads_every_row=False),
    # (1, 5, 60) -> 11 x 121 takes two column bands
    Family("convt2d_s2", F.conv_transpose2d, _s2, (3, 3), ((32, 32), (32, 16), (16, 1)),
           ((1, 1, 1), (2, 2, 5), (3, 7, 7), (1, 15, 15), (2, 31, 31), (1, 5, 60), (2, 40, 3)),
           lambda ci, co, n, h, w: 400 + w + ci + co),
    # notebook 07 (csrc/conv2d_frames_f32.hip): 128 -> 32 along the frame seam, four frames of 32 channels; (2, 5, 60) ->
    # 11 x 121 takes two column bands.  dw per frame: a dropped, doubled or swapped frame shows
    Family("convt2d_s2_frames", F.conv_transpose2d, _s2, (3, 3), ((128, 32),),
           ((1, 1, 1), (2, 2, 5), (3, 7, 7), (1, 15, 15), (2, 5, 60), (2, 40, 3)),
           lambda ci, co, n, h, w: 1100 + w + h, dw_groups=4),
    # notebook 08 (csrc/conv3d_s2_f32.hip): (2, 3, 3) at stride (1, 2, 2).  One output; an unread row and column over two
    # output depths; an unread column only, three output depths (interior input depths receive two taps); even sides over
    # several tiles; the model's second layer at full size; full width over several row bands
    Family("conv3d_s2", F.conv3d, _s122, (2, 3, 3), ((1, 8), (8, 32), (32, 32)),
           ((1, 2, 3, 3), (2, 3, 4, 4), (3, 4, 7, 12), (2, 2, 26, 26), (1, 3, 63, 63), (2, 2, 15, 128)),
           lambda ci, co, n, d, h, w: 800 + w + 7 * d + ci, no_dx_at_c_in=(1,), reads_every_row=False),
    # notebook 09 (csrc/conv2d_wide_s2_f32.hip).  The tile planners of the gather and scatter forms take smaller tiles while
    # the grid stays under 512 blocks, so these small shapes all run the smallest tile.  One output; non-square; even sides
    # (dx's last row and column exactly 0); full width (63 output columns, every column band the planner makes); the model's
    # own third-layer plane
    Family("conv2d_wide_s2", F.conv2d, _s2, (3, 3), ((64, 128), (128, 128)),
           ((1, 3, 3), (2, 5, 7), (2, 8, 10), (1, 4, 128), (2, 31, 31)),
           lambda ci, co, n, h, w: 900 + 7 * w + ci, reads_every_row=False),
    # tiny planes at a batch large enough that the larger tiles and weight-gradient slabs of several tiles are taken: gather
    # at 256 positions per block + scatter at 128 class positions + slabs of 6 tiles; gather at 128 positions per block
    Family("conv2d_wide_s2_tiles128", F.conv2d, _s2, (3, 3), ((128, 128),), ((256, 9, 9),),
           lambda ci, co, n, h, w: 950 + w + ci, stem="conv2d_wide_s2", reads_every_row=False),
    Family("conv2d_wide_s2_tiles64", F.conv2d, _s2, (3, 3), ((64, 128),), ((128, 17, 35),),
           lambda ci, co, n, h, w: 950 + w + ci, stem="conv2d_wide_s2", reads_every_row=False),
    # -> 3 x 3, every output from one source; small non-square; -> 11 x 65; -> 7 x 127, the widest; the model's first decoder
    # plane
    Family("convt2d_wide_s2", F.conv_transpose2d, _s2, (3, 3), ((128, 128),),
           ((1, 1, 1), (2, 2, 3), (1, 5, 32), (1, 3, 63), (2, 15, 15)),
           lambda ci, co, n, h, w: 1100 + 7 * w + h),
    # a full grid of tiny planes: the scatter at 128 class positions and the gather at 256 positions per block
    Family("convt2d_wide_s2_tiles", F.conv_transpose2d, _s2, (3, 3), ((128, 128),), ((256, 2, 3),),
           lambda ci, co, n, h, w: 1150 + w, stem="convt2d_wide_s2"),
    Family("convt2d_head", F.conv_transpose2d, {}, (3, 3), ((128, 1), (32, 1)),
           ((1, 1, 1), (2, 4, 5), (3, 10, 47), (1, 63, 63), (1, 3, 126)),
           lambda ci, co, n, h, w: 500 + w + ci, gates=HEAD_GATES, relu=False),
    # notebook 10 (csrc/conv2d_wide_f32.hip).  Padding 0: one output; non-square; more than one column band; full width
    Family("conv2d_wide_pad0", F.conv2d, {"padding": 0}, (3, 3), ((64, 128), (128, 128)),
           ((1, 3, 3), (2, 5, 7), (2, 9, 50), (1, 6, 128)),
           lambda ci, co, n, h, w: 300 + 7 * w + ci, stem="conv2d_wide", kwargs={"padding": 0}),
    # padding 2: every output touches padding; non-square; an odd width over one band; three column bands of the output
    Family("conv2d_wide_pad2", F.conv2d, {"padding": 2}, (3, 3), ((64, 128), (128, 128)),
           ((1, 1, 1), (2, 2, 5), (2, 7, 47), (1, 12, 124)),
           lambda ci, co, n, h, w: 300 + 7 * w + ci + 2, stem="conv2d_wide", kwargs={"padding": 2}),
    Family("conv2d_head_s2", F.conv2d, {"stride": 2, "padding": 2}, (3, 3), ((128, 1), (32, 1)),
           ((1, 1, 1), (2, 4, 5), (3, 10, 47), (2, 9, 46), (1, 126, 126)),
           lambda ci, co, n, h, w: 500 + w + ci, gates=HEAD_GATES, relu=False),
    # notebook 12 (csrc/conv3d_wide_f32.hip): (2, 3, 3) at padding (pd, 1, 1).  Depth padding 0: one voxel (eight of nine taps
    # padding); odd sides; several row bands; full width (three column bands); an odd width over one band
    Family("conv3d_wide_pd0", F.conv3d, {"padding": (0, 1, 1)}, (2, 3, 3), ((64, 128), (128, 128)),
           ((1, 2, 1, 1), (2, 3, 5, 7), (2, 4, 9, 50), (1, 2, 6, 128), (2, 3, 7, 47)),
           lambda ci, co, n, d, h, w: 300 + 7 * w + ci + 13 * d, stem="conv3d_wide", kwargs={"padding": (0, 1, 1)}),
    # depth padding 1: each output slice sees one real and one skipped slice; small; wide
    Family("conv3d_wide_pd1", F.conv3d, {"padding": (1, 1, 1)}, (2, 3, 3), ((64, 128), (128, 128)),
           ((1, 1, 1, 1), (2, 2, 2, 5), (1, 2, 12, 124)),
           lambda ci, co, n, d, h, w: 300 + 7 * w + ci + 1 + 13 * d, stem="conv3d_wide", kwargs={"padding": (1, 1, 1)}),
    Family("conv2d_head_s2p1", F.conv2d, {"stride": 2, "padding": 1}, (3, 3), ((256, 1), (32, 1)),
           ((1, 1, 1), (2, 4, 5), (3, 10, 47), (2, 9, 46), (1, 128, 128)),
           lambda ci, co, n, h, w: 500 + w + ci, gates=HEAD_GATES, relu=False),
)

BY_NAME = {f.name: f for f in FAMILIES}
RUN_BY = {}      # record or twin -> the GPU test that runs it, filled as the test files are imported


def _claim(names, fn):
    for name in names:
        assert RUN_BY.setdefault(name, fn.__qualname__) == fn.__qualname__, f"{name} is run by two tests"


def cases_of(names, ids):
    """Parametrise a GPU test (device, fam, c_in, c_out, shape) over every channel pair and shape of the named records, so what
    the GPU runs is what the table says.  `ids` is the test's id format over shape, c_in, c_out and tag; `names` may map each
    record to its tag (the padding in an id)."""
    tags = names if isinstance(names, dict) else dict.fromkeys([names] if isinstance(names, str) else names, "")
    params = [pytest.param(BY_NAME[n], c_in, c_out, s, id=ids.format(shape="-".join(map(str, s)), c_in=c_in, c_out=c_out, tag=t))
              for n, t in tags.items() for c_in, c_out in BY_NAME[n].pairs for s in BY_NAME[n].shapes]

    def mark(fn):
        _claim(tags, fn)
        return pytest.mark.parametrize("fam, c_in, c_out, shape", params)(fn)
    return mark


def twin_shapes(stem):
    """Parametrise a GPU test (device, twin, shape, ...) over the shapes of a layer that comes in two strides."""
    def mark(fn):
        _claim([stem], fn)
        return pytest.mark.parametrize("twin, shape", [pytest.param(TWINS[stem], s, id="-".join(map(str, s)))
                                                       for s in TWINS[stem].shapes])(fn)
    return mark

# every other public *_bwd_data_f32 stem of hip_ops: why it is no record here, and the test that covers it
EXEMPT = {
    "conv3d_general": ("bf16 operands, masks and stride / padding arguments: another surface and another tolerance",
                       "tests/test_gpu_conv3d_bf16_numerics.py"),
    "conv2d144_pool": ("a fused max pool: codes in place of dy_gate, gradients routed through the kernel's picks",
                       "tests/test_gpu_exp001.py::test_pooled_layer_against_float64"),
    "conv2d_ae_pool": ("a fused max pool: codes in place of dy_gate, gradients routed through the kernel's picks",
                       "tests/test_gpu_nb16.py::test_pooled_conv_against_float64"),
    "conv2d_wide_p2": ("conv2d_wide(padding=2) under the three-pass signature, one line each; the record conv2d_wide_pad2 "
                       "calls conv2d_wide itself, and notebook 10's model runs its padded layers through these three",
                       "tests/test_gpu_notebook_models.py::test_model_against_golden"),
    "conv3d_head_d2": ("conv2d_head_s2p1 on a depth-2 view, no gates",
                       "tests/test_gpu_nb12.py::test_head_depth2_view_against_float64_conv3d"),
}


# ---- the check of one family at one case ------------------------------------------------------------------------------------
def _norm(got, ref, what):
    err = _rel(got, ref)
    print(f"{what}: {err:.2e} (bound {NORM_TOL})")
    assert err <= NORM_TOL, f"{what}: relative norm {err:.2e} over the bound {NORM_TOL}"


def _same_bits(first, second, what):
    first, second = (t if isinstance(t, tuple) else (t,) for t in (first, second))
    assert all(torch.equal(a, b) for a, b in zip(first, second)), f"{what}: the bits differ run to run"


def check_forwards(fwd, args, b, pre, absref, relu=True, what="y"):
    """fwd(*args, bias, ...) on the device against the float64 pre-activation `pre` and its sum of |products|: ReLU + bias, bias
    alone, neither.  A head (relu=False) is called without `relu`: bias, no bias, and the same bits on a second call."""
    pre, bd = pre.detach(), b.to(args[-1].device)
    plain = pre - b.double().view(1, -1, *([1] * (pre.dim() - 2)))
    call = (lambda bias, r: fwd(*args, bias, relu=r)) if relu else (lambda bias, r: fwd(*args, bias))
    y = call(bd, True)
    assert tuple(y.shape) == tuple(pre.shape), f"{what} shape {tuple(y.shape)}"
    if relu:
        _within(y, pre.relu(), absref, what=f"{what} relu + bias")
        y = call(bd, False)
    else:
        _same_bits(y, call(bd, False), f"{what} forward")
    _within(y, pre, absref, what=f"{what} bias, no relu")
    _within(call(None, False), plain, absref, what=f"{what} plain")


def check_weight_grads(bwd_weight, dw64, db64, w_shape, groups=1, same_bits=True, what=""):
    """(dw, db) = bwd_weight() against float64: shapes, relative norms (a 3-D dw per depth tap, each of `groups` row groups
    on its own as well), and a second call's bits."""
    dw, db = bwd_weight()
    assert tuple(dw.shape) == tuple(w_shape), f"{what}dw shape {tuple(dw.shape)}"
    assert tuple(db.shape) == tuple(db64.shape), f"{what}db shape {tuple(db.shape)}"
    if len(w_shape) == 5:
        for kd in range(w_shape[2]):      # each depth tap on its own: the halves of dw may come from separate launches
            _norm(dw[:, :, kd], dw64[:, :, kd], f"{what}dw depth tap {kd}")
    else:
        _norm(dw, dw64, f"{what}dw")
    rows = w_shape[0] // groups
    for i in range(groups if groups > 1 else 0):
        _norm(dw[i * rows:(i + 1) * rows], dw64[i * rows:(i + 1) * rows], f"{what}dw rows {i * rows}..")
    _norm(db, db64, f"{what}db")
    if same_bits:
        _same_bits((dw, db), bwd_weight(), f"{what}dw, db")
    return dw, db


def check_dx(dx, dx64, absdx, what, unread_edge=False):
    """dx per element (a 3-D one per depth slice: edge depths receive one depth tap, interior ones two); the unread last row /
    column of an even side exactly 0."""
    assert tuple(dx.shape) == tuple(dx64.shape), f"{what} shape {tuple(dx.shape)}"
    if unread_edge and dx.shape[-2] % 2 == 0:
        assert (dx[..., -1, :] == 0).all(), f"{what}: the unread last row of dx is not exactly 0"
    if unread_edge and dx.shape[-1] % 2 == 0:
        assert (dx[..., :, -1] == 0).all(), f"{what}: the unread last column of dx is not exactly 0"
    if dx.dim() == 5:
        for z in range(dx.shape[2]):
            _within(dx[:, :, z], dx64[:, :, z], absdx[:, :, z], what=f"{what} depth {z} of {dx.shape[2]}")
    else:
        _within(dx, dx64, absdx, what=what)


def _close_some(g, *gates):
    """A third of each gate set to exactly 0.  A gate is open where > 0: the normal draw gives the negatives, this the zeros,
    and both must close.  Drawn after everything else, so the tensors of a case are those of the same seed without it."""
    return [gate * (torch.rand(gate.shape, generator=g) > 1 / 3) for gate in gates]


def grads64(pre, leaves, dy64):
    """Float64 gradients of the reference op's output `pre` at `leaves` for the output gradient dy64."""
    return torch.autograd.grad(pre, leaves, dy64, retain_graph=True)


def draw_case(fam, c_in, c_out, shape):
    """x, w, b, dy's generator: the family's seed rule, weights at fan-in scale, in the weight layout of the family's op."""
    g = _g(fam.seed(c_in, c_out, *shape))
    x = _randn(g, shape[0], c_in, *shape[1:])
    if fam.x_is_relu_output:
        x = x.relu()
    w_shape = (c_in, c_out, *fam.kernel) if fam.transposed else (c_out, c_in, *fam.kernel)
    return g, x, _randn(g, *w_shape, scale=(math.prod(fam.kernel) * c_in) ** -0.5), _randn(g, c_out, scale=0.1)


def check_family(K, device, fam, c_in, c_out, shape):
    """The three passes of `fam` (entry points looked up on K) at one case against float64."""
    fwd, bwd_data, bwd_weight = (getattr(K, name) for name in fam.entry_points())
    kw = fam.kwargs
    g, x, w, b = draw_case(fam, c_in, c_out, shape)
    has_dx = c_in not in fam.no_dx_at_c_in
    x64 = x.double().requires_grad_(has_dx)
    w64, b64 = w.double().requires_grad_(True), b.double().requires_grad_(True)
    pre = fam.op(x64, w64, b64, **fam.op_kw)
    absref = fam.op(x64.detach().abs(), w64.detach().abs(), b64.detach().abs(), **fam.op_kw)
    xd, wd = x.to(device), w.to(device)
    check_forwards(lambda *a, **k: fwd(*a, **k, **kw), (xd, wd), b, pre, absref, relu=fam.relu)

    dy, dy_gate, x_gate = _randn(g, *pre.shape), _randn(g, *pre.shape), _randn(g, *x.shape)
    dy_gate, x_gate = _close_some(g, dy_gate, x_gate)
    dyd, dy_gate_d, x_gate_d = dy.to(device), dy_gate.to(device), x_gate.to(device)
    scale = fam.op(x64, w64.detach().abs(), None, **fam.op_kw) if has_dx else None      # linear in x: its gradient is |w|'s
    for use_dg in (True, False):                 # one float64 backward and one weight gradient per dy, not per gate pair
        x_gates = [xg for dg, xg in fam.gates if dg == use_dg]
        if not x_gates:
            continue
        dyg = dy.double() * (dy_gate > 0) if use_dg else dy.double()
        gate_d = dy_gate_d if use_dg else None
        *dx64, dw64, db64 = grads64(pre, ((x64,) if has_dx else ()) + (w64, b64), dyg)
        check_weight_grads(lambda: bwd_weight(xd, dyd, gate_d, tuple(w.shape), **kw), dw64, db64, tuple(w.shape),
                           groups=fam.dw_groups, same_bits=fam.same_bits, what=f"dy_gate {use_dg}: ")
        if not has_dx:
            continue
        absdx, = grads64(scale, (x64,), dyg.abs())
        for use_xg in x_gates:
            dx = bwd_data(dyd, gate_d, wd, x_gate_d if use_xg else None, tuple(x.shape), **kw)
            check_dx(dx, dx64[0] * (x_gate > 0) if use_xg else dx64[0], absdx, f"dx gates {use_dg} {use_xg}",
                     unread_edge=not fam.reads_every_row)


# ---- first layers that synthesise input channels, and the horizon ConvTranspose2d: each in two strides -----------------------
N_HIST = (4, 1)      # history frames before the stripe channel


class Twin(NamedTuple):
    stem: str                       # hip_ops stem of the forward and the weight gradient
    op_kw: dict                     # the float64 reference op's stride
    shapes: tuple                   # (batch, height, width)
    seed: Callable
    bits_shape: tuple = ()          # counts layers: the shape of the int16 / f32 identical-bits test
    plain: str = ""                 # horizon layers: the family whose data gradient serves the 32 real channels


# notebooks 10 and 09: the last shape of the stride-2 layer takes weight-gradient slabs of two tiles
STRIPE_LAYERS = (
    Twin("conv2d_wide_stripe", {}, ((1, 128, 128), (2, 9, 50), (3, 20, 54)), lambda n_hist, n, h, w: 100 + w + n_hist),
    Twin("conv2d_wide_s2_stripe", _s2, ((1, 128, 128), (2, 9, 50), (3, 20, 54), (9, 128, 128)),
         lambda n_hist, n, h, w: 100 + w + n_hist + n),
)
# notebooks 16 and 15.  Stride 1: widths 128, 127, 44, 38, 36, 11 -- multiples and non-multiples of every tile extent
COUNTS_LAYERS = (
    Twin("conv2d_ae_counts", {}, ((1, 128, 128), (1, 21, 127), (2, 44, 44), (3, 38, 38), (2, 36, 36), (2, 11, 11)),
         lambda n, h, w: 100 + w, bits_shape=(2, 38, 36)),
    Twin("conv2d_s2_counts", _s2, ((1, 128, 128), (2, 31, 32), (3, 54, 47)), lambda n, h, w: 100 + w, bits_shape=(2, 54, 47)),
)
# notebooks 05 and 08: 33 -> 32 with the horizon as the last input channel.  Stride 1: (2, 5, 63) -> 65 wide takes two column
# bands, (2, 3, 126) is 128 wide, (1, 58, 58) is the model's own.  Stride 2: (2, 5, 60) -> 11 x 121 takes two column bands
HORIZON_LAYERS = (
    Twin("convt2d_ae_horizon", {}, ((1, 1, 1), (2, 2, 5), (3, 7, 7), (2, 5, 63), (2, 3, 126), (1, 58, 58)),
         lambda n, h, w: 1500 + w + h, plain="convt2d_ae"),
    Twin("convt2d_s2_horizon", _s2, ((1, 1, 1), (2, 2, 5), (3, 7, 7), (1, 15, 15), (2, 5, 60), (2, 40, 3)),
         lambda n, h, w: 1000 + w + h, plain="convt2d_s2"),
)

TWINS = {t.stem: t for t in STRIPE_LAYERS + COUNTS_LAYERS + HORIZON_LAYERS}


def _conv_params(g, c_out, c_in):
    return _randn(g, c_out, c_in, 3, 3, scale=(9 * c_in) ** -0.5), _randn(g, c_out, scale=0.1)


def _out_shape(op_kw, n, c_out, h, w):
    plane = F.conv2d(torch.empty(1, 1, h, w, device="meta"), torch.empty(1, 1, 3, 3, device="meta"), **op_kw)
    return (n, c_out, *plane.shape[2:])


def check_first_layer(fwd, bwd_weight, x64, w, b, dy, op_kw, what):
    """A first layer that builds its input itself, against F.conv2d on the materialised float64 input x64: the forward with
    ReLU, and (dw, db) for the ungated dy, twice.  fwd() and bwd_weight() are the calls, arguments bound.  Returns dw."""
    w64, b64 = w.double().requires_grad_(True), b.double().requires_grad_(True)
    pre = F.conv2d(x64, w64, b64, **op_kw)
    assert tuple(pre.shape) == tuple(dy.shape)
    y = fwd()
    assert tuple(y.shape) == tuple(pre.shape), f"{what} y shape {tuple(y.shape)}"
    absref = F.conv2d(x64.abs(), w64.detach().abs(), b64.detach().abs(), **op_kw)
    _within(y, pre.detach().relu(), absref, what=f"{what} forward")
    return check_weight_grads(bwd_weight, *grads64(pre, (w64, b64), dy.double()), tuple(w.shape), what=f"{what} ")[0]


def check_stripe_layer(K, device, twin, n_hist, shape):
    """The starts rotate through column 0, mid-image, clipped at the right edge, at / beyond the width (an all-zero plane) and
    a negative one (clipped at the left edge by the kernel rule)."""
    from nb10_reference import STRIPE_WIDTH, stripe_plane64
    fwd, bwd_weight = getattr(K, f"{twin.stem}_fwd_f32"), getattr(K, f"{twin.stem}_bwd_weight_f32")
    n, h, w = shape
    g = _g(twin.seed(n_hist, n, h, w))
    hist = _randn(g, n, n_hist, h, w)
    wt, b = _conv_params(g, 64, n_hist + 1)
    dy = _randn(g, *_out_shape(twin.op_kw, n, 64, h, w))
    hd, wd, bd, dyd = hist.to(device), wt.to(device), b.to(device), dy.to(device)
    pool = [0, w // 2, w - 2, w, w + 3, -3]
    for k in range(len(pool)):
        starts = torch.tensor([pool[(k + i) % len(pool)] for i in range(n)], dtype=torch.int32)
        sd = starts.to(device)
        x64 = torch.cat((hist.double(), stripe_plane64(starts, h, w)), dim=1)
        dw = check_first_layer(lambda: fwd(hd, sd, wd, bd, STRIPE_WIDTH),
                               lambda: bwd_weight(hd, sd, dyd, tuple(wt.shape), STRIPE_WIDTH), x64, wt, b, dy, twin.op_kw,
                               f"stripe starts {starts.tolist()}")
        if int(x64[:, n_hist].sum()) == 0:      # the stripe channel's own gradient: exact zeros where the plane is empty
            assert (dw[:, n_hist] == 0).all(), "the gradient of an empty stripe plane's channel is not exactly 0"


def _counts_case(K, device, twin, seed, shape, integer_flow=False):
    n, h, w = shape
    g = _g(seed)
    hist, flow, hor = _counts(g, n, h, w, integer_flow=integer_flow)
    wt, b = _conv_params(g, 16, 6)
    dy = _randn(g, *_out_shape(twin.op_kw, n, 16, h, w))
    fwd, bwd_weight = getattr(K, f"{twin.stem}_fwd_f32"), getattr(K, f"{twin.stem}_bwd_weight_f32")
    hord, wd, bd, dyd = hor.to(device), wt.to(device), b.to(device), dy.to(device)

    def passes(hist_dtype, flow_dtype):
        hi, fl = hist.to(device=device, dtype=hist_dtype), flow.to(device=device, dtype=flow_dtype)
        return (lambda: fwd(hi, fl, hord, wd, bd)), (lambda: bwd_weight(hi, fl, hord, dyd, (16, 6, 3, 3)))
    return passes, (hist, flow, hor, wt, b, dy)


def check_counts_layer(K, device, twin, shape):
    from nb15_reference import input64
    passes, (hist, flow, hor, wt, b, dy) = _counts_case(K, device, twin, twin.seed(*shape), shape)
    check_first_layer(*passes(torch.int16, torch.float32), input64(hist, flow, hor), wt, b, dy, twin.op_kw, "counts")


def check_counts_layer_input_dtypes(K, device, twin):
    """int16 and f32 history / flow inputs holding the same integers give identical bits in y, dw and db."""
    passes, _ = _counts_case(K, device, twin, 7, twin.bits_shape, integer_flow=True)
    outs = []
    for dtypes in ((torch.int16, torch.int16), (torch.float32, torch.float32), (torch.int16, torch.float32)):
        fwd, bwd_weight = passes(*dtypes)
        outs.append((fwd(), *bwd_weight()))
    for other in outs[1:]:
        _same_bits(outs[0], other, "counts layer across input dtypes")


def check_horizon_conv_transpose(K, device, twin, shape):
    """ConvTranspose2d 33 -> 32 against float64 autograd on the materialised 33-channel input: the three forwards; dw whole, its
    horizon row and its real rows each on their own; the 32 real channels' dx through the plain family on weight[:32]."""
    fwd, bwd_weight = getattr(K, f"{twin.stem}_fwd_f32"), getattr(K, f"{twin.stem}_bwd_weight_f32")
    bwd_data = getattr(K, f"{twin.plain}_bwd_data_f32")
    n, h, w = shape
    g = _g(twin.seed(n, h, w))
    x = _randn(g, n, 32, h, w)
    horizon = torch.tensor([0.0, -1.3, 0.7][:n]) if n > 1 else torch.tensor([-0.4])      # zero and both signs
    wt, b = _randn(g, 33, 32, 3, 3, scale=(9 * 33) ** -0.5), _randn(g, 32, scale=0.1)
    xd, hd, wd = x.to(device), horizon.to(device), wt.to(device)
    x33 = torch.cat((x.double(), horizon.double().view(n, 1, 1, 1).expand(n, 1, h, w)), dim=1).requires_grad_(True)
    w64, b64 = wt.double().requires_grad_(True), b.double().requires_grad_(True)
    pre = F.conv_transpose2d(x33, w64, b64, **twin.op_kw)
    absref = F.conv_transpose2d(x33.detach().abs(), w64.detach().abs(), b64.detach().abs(), **twin.op_kw)
    check_forwards(fwd, (xd, hd, wd), b, pre, absref, what="horizon convT y")
    dy, dy_gate, x_gate = _randn(g, *pre.shape), _randn(g, *pre.shape), _randn(g, *x.shape)
    dy_gate, x_gate = _close_some(g, dy_gate, x_gate)
    dyd = dy.to(device)
    scale = F.conv_transpose2d(x33, w64.detach().abs(), None, **twin.op_kw)
    for use_dg, use_xg in GATES:
        dyg = dy.double() * (dy_gate > 0) if use_dg else dy.double()
        gate_d = dy_gate.to(device) if use_dg else None
        dx64, dw64, db64 = grads64(pre, (x33, w64, b64), dyg)
        dw, _ = check_weight_grads(lambda: bwd_weight(xd, hd, dyd, gate_d, tuple(wt.shape)), dw64, db64, tuple(wt.shape),
                                   what=f"horizon convT dy_gate {use_dg}: ")
        _norm(dw[32], dw64[32], f"dy_gate {use_dg}: dw horizon row")
        _norm(dw[:32], dw64[:32], f"dy_gate {use_dg}: dw real rows")
        # the 32 real channels' data gradient: the plain entry point on the first 32 rows of the weight (contiguous)
        dx = bwd_data(dyd, gate_d, wd[:32], x_gate.to(device) if use_xg else None, tuple(x.shape))
        dx64, absdx = dx64[:, :32], grads64(scale, (x33,), dyg.abs())[0][:, :32]
        check_dx(dx, dx64 * (x_gate > 0) if use_xg else dx64, absdx, f"horizon convT dx gates {use_dg} {use_xg}")
