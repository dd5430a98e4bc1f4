"""CPU: the Python glue of the 34 exact-f32 Conv2d / ConvTranspose2d / normalised-MSE wrappers of hip_ops.py, without a
GPU and without the library.  get_lib, require_cuda, check and current_stream_ptr are replaced on hip_ops; the stand-in
library records every call and answers 0.  For each wrapper the tables below pin what it hands to the C ABI (symbols in
order, every pointer by its role, every integer as it stands), what it returns, which workspace keys it creates, and the
type and whole text of its argument errors.  The tables were recorded from the hand-written wrappers before they were
folded into one implementation per pass: they are the contract, so a change to the glue never edits them.

Roles: an input tensor by its argument name, out0 / out1 the returned tensors in order, ws:<key> a workspace of
hip_ops._workspaces, &bytes the size_t a workspace query writes, stream the current stream, NULL a null pointer."""
import ctypes
import os
import re

import pytest
import torch

from predict_pv_yield_amd import _lib
from predict_pv_yield_amd import hip_ops as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "pv_yield_hip.h")
f32, i16, u8, f64 = torch.float32, torch.int16, torch.uint8, torch.float64
STREAM = 0x57AEA0
QUERY_BYTES = 4096          # what a workspace query answers unless the case says otherwise


class T:
    """A tensor argument: zeros of this shape; contiguous=False makes a transposed view of the same shape."""

    def __init__(self, *shape, dtype=f32, contiguous=True):
        self.shape, self.dtype, self.contiguous = shape, dtype, contiguous

    def make(self):
        if self.contiguous:
            return torch.zeros(self.shape, dtype=self.dtype)
        return torch.zeros(self.shape[:-2] + (self.shape[-1], self.shape[-2]), dtype=self.dtype).transpose(-1, -2)

    def __repr__(self):
        extra = "" if self.dtype == f32 else f", dtype={_DTYPE_NAMES[self.dtype]}"
        return f"T({', '.join(map(str, self.shape))}{extra}{'' if self.contiguous else ', contiguous=False'})"


_DTYPE_NAMES = {i16: "i16", u8: "u8", f64: "f64"}


class Recorder:
    """Stands in for the ctypes library: every attribute is a function that records its arguments and returns 0; a
    byref(c_size_t) argument receives the byte count the case chose for that symbol."""

    def __init__(self, events, answers):
        self._events, self._answers = events, answers

    def __getattr__(self, name):
        def fn(*args):
            self._events.append((name, args))
            for a in args:
                if hasattr(a, "_obj"):
                    a._obj.value = self._answers.get(name, QUERY_BYTES)
            return 0
        return fn


def _role(arg, roles):
    if isinstance(arg, torch.Tensor):
        return roles[arg.data_ptr()]
    if isinstance(arg, ctypes.c_void_p):
        return "NULL" if not arg.value else roles.get(arg.value, hex(arg.value))
    if arg is None:
        return "NULL"
    if hasattr(arg, "_obj"):
        return "&bytes"
    assert type(arg) is int, (type(arg), arg)
    return str(arg)


def run(monkeypatch, fn, args, answers):
    """Calls hip_ops.<fn>(*args.values()) under the stand-ins.  Returns (events as text, results as text, workspace keys,
    the exception or None)."""
    events, labels = [], []
    lib = Recorder(events, answers)
    monkeypatch.setattr(K, "_workspaces", {})                   # undone with the other patches when the test ends
    monkeypatch.setattr(K, "get_lib", lambda: lib)
    monkeypatch.setattr(K, "require_cuda", lambda *ts: events.append(("require_cuda", ts)))
    monkeypatch.setattr(K, "check", lambda status, what="": labels.append((status, what)))
    monkeypatch.setattr(K, "current_stream_ptr", lambda: ctypes.c_void_p(STREAM))
    values = {k: v.make() if isinstance(v, T) else v for k, v in args.items()}
    roles = {STREAM: "stream"}
    for k, v in values.items():
        if isinstance(v, torch.Tensor):
            assert v.numel() > 0 and v.data_ptr() not in roles
            roles[v.data_ptr()] = k
    out, error = None, None
    try:
        out = getattr(K, fn)(*values.values())
    except Exception as e:                                      # noqa: BLE001 -- the table names the type
        error = e
    outs = list(out) if isinstance(out, tuple) else ([] if out is None else [out])
    for i, t in enumerate(outs):
        if t is not None:
            roles[t.data_ptr()] = f"out{i}"
    for (key, device), buf in K._workspaces.items():
        assert device == "cpu"
        roles[buf.data_ptr()] = f"ws:{key}"
    symbols = [name for name, _ in events if name != "require_cuda"]
    assert labels == [(0, s) for s in symbols]                  # check() is handed each status under the full symbol name
    text = [" ".join([name] + [_role(a, roles) for a in a_]) for name, a_ in events]
    results = ["None" if t is None else f"{tuple(t.shape)} {str(t.dtype).split('.')[1]}" for t in outs]
    return text, results, sorted(key for key, _ in K._workspaces), error


def check_glue_case(monkeypatch, glue_case):
    """One row (wrapper, arguments, calls, results, workspace keys) of a notebook's GLUE table (tests/test_nbXX_cpu.py): what the
    wrapper hands to the C ABI."""
    fn, args, want_calls, want_results, want_keys = glue_case
    text, results, keys, error = run(monkeypatch, fn, args, {})
    assert error is None, error
    assert [t.split(" ")[0] if t.startswith("require_cuda") else t for t in text] == want_calls
    assert results == want_results and keys == want_keys


def check_new_symbols(new_symbols, notebook=None):
    """A notebook's entry points (name -> parameter count) are declared in the header with that many parameters, bound with as
    many argtypes and exported by the library; the header names the notebook."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = {name: params.count(",") + 1 for name, params in re.findall(r"\b(pv_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)}
    for name, arity in new_symbols.items():
        assert declared.get(name) == arity, (name, declared.get(name))
        assert len(_lib.SIGNATURES[name]) == arity, name
    lib = _lib.get_lib()
    assert all(hasattr(lib, name) for name in new_symbols)
    assert notebook is None or notebook in open(HEADER).read()


def case(fn, answers=None, **args):
    return fn, args, answers or {}


SAT2 = dict(sat=T(6, 9, 11, 12), x_coords=T(2, 11), y_coords=T(2, 9))              # experiments/002: 2 examples x 3 frames
SAT1 = dict(sat=T(2, 5, 9, 11, 1), x_coords=T(2, 11), y_coords=T(2, 9))            # experiments/001: 5 frames, 3 used
COUNTS = dict(history=T(2, 4, 9, 11, dtype=i16), flow_pred=T(2, 9, 11), horizon=T(2))
COUNTS_REV = dict(history=T(2, 4, 9, 11), flow_pred=T(2, 9, 11, dtype=i16), horizon=T(2))
COUNTS_EVEN = dict(history=T(2, 4, 10, 12, dtype=i16), flow_pred=T(2, 10, 12), horizon=T(2))
COUNTS_EVEN_REV = dict(history=T(2, 4, 10, 12), flow_pred=T(2, 10, 12, dtype=i16), horizon=T(2))
X32, X144, X16 = (2, 32, 9, 11), (2, 144, 9, 11), (2, 16, 9, 11)
W144 = (144, 144, 3, 3)

# id -> (wrapper, its arguments in order, what each workspace query answers).  Planes are 9 x 11 (and 10 x 12 where an even
# side takes another branch of the stride-2 rule); the ConvTranspose2d layers go 32 -> 16 so that a swapped weight axis shows.
CASES = {
    # experiments/002
    "conv2d_coords_fwd": case("conv2d_coords_fwd_f32", **SAT2, weight=T(32, 17, 3, 3), bias=T(32), t_per_example=3),
    "conv2d_coords_fwd/nobias": case("conv2d_coords_fwd_f32", **SAT2, weight=T(32, 17, 3, 3), bias=None, t_per_example=3),
    "conv2d_fwd": case("conv2d_fwd_f32", x=T(*X32), weight=T(4, 32, 3, 3), bias=T(4), relu=True),
    "conv2d_fwd/none": case("conv2d_fwd_f32", x=T(*X32), weight=T(4, 32, 3, 3), bias=None, relu=False),
    "conv2d_bwd_data": case("conv2d_bwd_data_f32", dy=T(2, 4, 7, 9), dy_gate=T(2, 4, 7, 9), weight=T(4, 32, 3, 3),
                            x_gate=T(*X32), x_shape=X32),
    "conv2d_bwd_data/none": case("conv2d_bwd_data_f32", dy=T(2, 4, 7, 9), dy_gate=None, weight=T(4, 32, 3, 3), x_gate=None,
                                 x_shape=X32),
    "conv2d_bwd_weight": case("conv2d_bwd_weight_f32", x=T(*X32), dy=T(2, 4, 7, 9), dy_gate=T(2, 4, 7, 9),
                              weight_shape=(4, 32, 3, 3)),
    "conv2d_bwd_weight/none": case("conv2d_bwd_weight_f32", x=T(*X32), dy=T(2, 4, 7, 9), dy_gate=None,
                                   weight_shape=(4, 32, 3, 3)),
    "conv2d_coords_bwd_weight": case("conv2d_coords_bwd_weight_f32", **SAT2, dy=T(6, 32, 7, 9), t_per_example=3,
                                     weight_shape=(32, 17, 3, 3)),
    # experiments/001
    "conv2d144_sat_pool_fwd": case("conv2d144_sat_pool_fwd_f32", **SAT1, weight=T(144, 8, 3, 3), bias=T(144), n_frames=3),
    "conv2d144_sat_pool_fwd/5x5": case("conv2d144_sat_pool_fwd_f32", sat=T(2, 5, 5, 5, 1), x_coords=T(2, 5), y_coords=T(2, 5),
                                       weight=T(144, 8, 3, 3), bias=T(144), n_frames=3),
    "conv2d144_pool_fwd": case("conv2d144_pool_fwd_f32", x=T(*X144), weight=T(*W144), bias=T(144)),
    "conv2d144_pool_fwd/5x5": case("conv2d144_pool_fwd_f32", x=T(1, 144, 5, 5), weight=T(*W144), bias=T(144)),
    "conv2d144_fwd": case("conv2d144_fwd_f32", x=T(*X144), weight=T(*W144), bias=T(144), relu=True),
    "conv2d144_fwd/none": case("conv2d144_fwd_f32", x=T(*X144), weight=T(*W144), bias=None, relu=False),
    "conv2d144_bwd_data": case("conv2d144_bwd_data_f32", dy=T(2, 144, 7, 9), dy_gate=T(2, 144, 7, 9), weight=T(*W144),
                               x_gate=T(*X144), x_shape=X144),
    "conv2d144_bwd_data/none": case("conv2d144_bwd_data_f32", dy=T(2, 144, 7, 9), dy_gate=None, weight=T(*W144), x_gate=None,
                                    x_shape=X144),
    "conv2d144_pool_bwd_data": case("conv2d144_pool_bwd_data_f32", dy_pooled=T(2, 144, 2, 3), codes=T(2, 144, 2, 3, dtype=u8),
                                    weight=T(*W144), x_gate=T(*X144), x_shape=X144),
    "conv2d144_pool_bwd_data/none": case("conv2d144_pool_bwd_data_f32", dy_pooled=T(1, 144, 1, 1),
                                         codes=T(1, 144, 1, 1, dtype=u8), weight=T(*W144), x_gate=None,
                                         x_shape=(1, 144, 5, 5)),
    "conv2d144_bwd_weight": case("conv2d144_bwd_weight_f32", x=T(*X144), dy=T(2, 144, 7, 9), dy_gate=T(2, 144, 7, 9),
                                 weight_shape=W144),
    "conv2d144_bwd_weight/none": case("conv2d144_bwd_weight_f32", x=T(*X144), dy=T(2, 144, 7, 9), dy_gate=None,
                                      weight_shape=W144),
    "conv2d144_pool_bwd_weight": case("conv2d144_pool_bwd_weight_f32", x=T(*X144), dy_pooled=T(2, 144, 2, 3),
                                      codes=T(2, 144, 2, 3, dtype=u8), weight_shape=W144),
    "conv2d144_pool_bwd_weight/5x5": case("conv2d144_pool_bwd_weight_f32", x=T(1, 144, 5, 5), dy_pooled=T(1, 144, 1, 1),
                                          codes=T(1, 144, 1, 1, dtype=u8), weight_shape=W144),
    "conv2d144_sat_pool_bwd_weight": case("conv2d144_sat_pool_bwd_weight_f32", **SAT1, dy_pooled=T(2, 144, 2, 3),
                                          codes=T(2, 144, 2, 3, dtype=u8), n_frames=3),
    # notebooks/16_maxpool.ipynb
    "conv2d_ae_counts_fwd": case("conv2d_ae_counts_fwd_f32", **COUNTS, weight=T(16, 6, 3, 3), bias=T(16)),
    "conv2d_ae_counts_fwd/rev": case("conv2d_ae_counts_fwd_f32", **COUNTS_REV, weight=T(16, 6, 3, 3), bias=T(16)),
    "conv2d_ae_counts_bwd_weight": case("conv2d_ae_counts_bwd_weight_f32", **COUNTS, dy=T(2, 16, 7, 9),
                                        weight_shape=(16, 6, 3, 3)),
    "conv2d_ae_counts_bwd_weight/rev": case("conv2d_ae_counts_bwd_weight_f32", **COUNTS_REV, dy=T(2, 16, 7, 9),
                                            weight_shape=(16, 6, 3, 3)),
    "conv2d_ae_fwd": case("conv2d_ae_fwd_f32", x=T(*X16), weight=T(32, 16, 3, 3), bias=T(32), relu=True),
    "conv2d_ae_fwd/none": case("conv2d_ae_fwd_f32", x=T(*X16), weight=T(32, 16, 3, 3), bias=None, relu=False),
    "conv2d_ae_bwd_data": case("conv2d_ae_bwd_data_f32", dy=T(2, 32, 7, 9), dy_gate=T(2, 32, 7, 9), weight=T(32, 16, 3, 3),
                               x_gate=T(*X16), x_shape=X16),
    "conv2d_ae_bwd_data/none": case("conv2d_ae_bwd_data_f32", dy=T(2, 32, 7, 9), dy_gate=None, weight=T(32, 16, 3, 3),
                                    x_gate=None, x_shape=X16),
    "conv2d_ae_bwd_weight": case("conv2d_ae_bwd_weight_f32", x=T(*X16), dy=T(2, 32, 7, 9), dy_gate=T(2, 32, 7, 9),
                                 weight_shape=(32, 16, 3, 3)),
    "conv2d_ae_bwd_weight/none": case("conv2d_ae_bwd_weight_f32", x=T(*X16), dy=T(2, 32, 7, 9), dy_gate=None,
                                      weight_shape=(32, 16, 3, 3)),
    "conv2d_ae_pool_fwd": case("conv2d_ae_pool_fwd_f32", x=T(*X32), weight=T(16, 32, 3, 3), bias=T(16)),
    "conv2d_ae_pool_fwd/no_workspace": case("conv2d_ae_pool_fwd_f32", {"pv_conv2d_ae_pool_fwd_workspace_bytes": 0}, x=T(*X32),
                                            weight=T(16, 32, 3, 3), bias=T(16)),
    "conv2d_ae_pool_fwd/5x5": case("conv2d_ae_pool_fwd_f32", x=T(1, 32, 5, 5), weight=T(16, 32, 3, 3), bias=T(16)),
    "conv2d_ae_pool_bwd_data": case("conv2d_ae_pool_bwd_data_f32", dy_pooled=T(2, 16, 2, 3), codes=T(2, 16, 2, 3, dtype=u8),
                                    weight=T(16, 32, 3, 3), x_gate=T(*X32), x_shape=X32),
    "conv2d_ae_pool_bwd_data/none": case("conv2d_ae_pool_bwd_data_f32", dy_pooled=T(1, 16, 1, 1), codes=T(1, 16, 1, 1, dtype=u8),
                                         weight=T(16, 32, 3, 3), x_gate=None, x_shape=(1, 32, 5, 5)),
    "conv2d_ae_pool_bwd_weight": case("conv2d_ae_pool_bwd_weight_f32", x=T(*X32), dy_pooled=T(2, 16, 2, 3),
                                      codes=T(2, 16, 2, 3, dtype=u8), weight_shape=(16, 32, 3, 3)),
    "conv2d_ae_pool_bwd_weight/5x5": case("conv2d_ae_pool_bwd_weight_f32", x=T(1, 32, 5, 5), dy_pooled=T(1, 16, 1, 1),
                                          codes=T(1, 16, 1, 1, dtype=u8), weight_shape=(16, 32, 3, 3)),
    "convt2d_ae_fwd": case("convt2d_ae_fwd_f32", x=T(*X32), weight=T(32, 16, 3, 3), bias=T(16), relu=True),
    "convt2d_ae_fwd/none": case("convt2d_ae_fwd_f32", x=T(*X32), weight=T(32, 16, 3, 3), bias=None, relu=False),
    "convt2d_ae_bwd_data": case("convt2d_ae_bwd_data_f32", dy=T(2, 16, 11, 13), dy_gate=T(2, 16, 11, 13),
                                weight=T(32, 16, 3, 3), x_gate=T(*X32), x_shape=X32),
    "convt2d_ae_bwd_data/none": case("convt2d_ae_bwd_data_f32", dy=T(2, 16, 11, 13), dy_gate=None, weight=T(32, 16, 3, 3),
                                     x_gate=None, x_shape=X32),
    "convt2d_ae_bwd_weight": case("convt2d_ae_bwd_weight_f32", x=T(*X32), dy=T(2, 16, 11, 13), dy_gate=T(2, 16, 11, 13),
                                  weight_shape=(32, 16, 3, 3)),
    "convt2d_ae_bwd_weight/none": case("convt2d_ae_bwd_weight_f32", x=T(*X32), dy=T(2, 16, 11, 13), dy_gate=None,
                                       weight_shape=(32, 16, 3, 3)),
    "mse_crop_norm": case("mse_crop_norm_f32", y_hat=T(2, 9, 11), target=T(2, 25, 27, dtype=i16), need_grad=True),
    "mse_crop_norm/f32_nograd": case("mse_crop_norm_f32", y_hat=T(2, 9, 11), target=T(2, 25, 27), need_grad=False),
    "mse_crop_norm/default": case("mse_crop_norm_f32", y_hat=T(3, 9, 11), target=T(3, 25, 27)),
    # notebooks/14_back_to_2d_conv_AE.ipynb, 15_int16.ipynb
    "conv2d_s2_counts_fwd": case("conv2d_s2_counts_fwd_f32", **COUNTS, weight=T(16, 6, 3, 3), bias=T(16)),
    "conv2d_s2_counts_fwd/even_rev": case("conv2d_s2_counts_fwd_f32", **COUNTS_EVEN_REV, weight=T(16, 6, 3, 3), bias=T(16)),
    "conv2d_s2_counts_bwd_weight": case("conv2d_s2_counts_bwd_weight_f32", **COUNTS_EVEN, dy=T(2, 16, 4, 5),
                                        weight_shape=(16, 6, 3, 3)),
    "conv2d_s2_counts_bwd_weight/odd_rev": case("conv2d_s2_counts_bwd_weight_f32", **COUNTS_REV, dy=T(2, 16, 4, 5),
                                                weight_shape=(16, 6, 3, 3)),
    "conv2d_s2_fwd": case("conv2d_s2_fwd_f32", x=T(*X16), weight=T(32, 16, 3, 3), bias=T(32), relu=True),
    "conv2d_s2_fwd/even_none": case("conv2d_s2_fwd_f32", x=T(2, 16, 10, 12), weight=T(32, 16, 3, 3), bias=None, relu=False),
    "conv2d_s2_fwd/12x13": case("conv2d_s2_fwd_f32", x=T(2, 16, 12, 13), weight=T(32, 16, 3, 3), bias=T(32)),
    "conv2d_s2_bwd_data": case("conv2d_s2_bwd_data_f32", dy=T(2, 32, 4, 5), dy_gate=T(2, 32, 4, 5), weight=T(32, 16, 3, 3),
                               x_gate=T(*X16), x_shape=X16),
    "conv2d_s2_bwd_data/even_none": case("conv2d_s2_bwd_data_f32", dy=T(2, 32, 4, 5), dy_gate=None, weight=T(32, 16, 3, 3),
                                         x_gate=None, x_shape=(2, 16, 10, 12)),
    "conv2d_s2_bwd_weight": case("conv2d_s2_bwd_weight_f32", x=T(*X16), dy=T(2, 32, 4, 5), dy_gate=T(2, 32, 4, 5),
                                 weight_shape=(32, 16, 3, 3)),
    "conv2d_s2_bwd_weight/even_none": case("conv2d_s2_bwd_weight_f32", x=T(2, 16, 10, 12), dy=T(2, 32, 4, 5), dy_gate=None,
                                           weight_shape=(32, 16, 3, 3)),
    "convt2d_s2_fwd": case("convt2d_s2_fwd_f32", x=T(*X32), weight=T(32, 16, 3, 3), bias=T(16), relu=True),
    "convt2d_s2_fwd/none": case("convt2d_s2_fwd_f32", x=T(*X32), weight=T(32, 16, 3, 3), bias=None, relu=False),
    "convt2d_s2_bwd_data": case("convt2d_s2_bwd_data_f32", dy=T(2, 16, 19, 23), dy_gate=T(2, 16, 19, 23),
                                weight=T(32, 16, 3, 3), x_gate=T(*X32), x_shape=X32),
    "convt2d_s2_bwd_data/none": case("convt2d_s2_bwd_data_f32", dy=T(2, 16, 19, 23), dy_gate=None, weight=T(32, 16, 3, 3),
                                     x_gate=None, x_shape=X32),
    "convt2d_s2_bwd_weight": case("convt2d_s2_bwd_weight_f32", x=T(*X32), dy=T(2, 16, 19, 23), dy_gate=T(2, 16, 19, 23),
                                  weight_shape=(32, 16, 3, 3)),
    "convt2d_s2_bwd_weight/none": case("convt2d_s2_bwd_weight_f32", x=T(*X32), dy=T(2, 16, 19, 23), dy_gate=None,
                                       weight_shape=(32, 16, 3, 3)),
    "mse_window_norm": case("mse_window_norm_f32", y_hat=T(2, 9, 11), target=T(2, 12, 14, dtype=i16), row0=1, col0=2,
                            need_grad=True),
    "mse_window_norm/f32_nograd": case("mse_window_norm_f32", y_hat=T(2, 9, 11), target=T(2, 12, 14), row0=1, col0=2,
                                       need_grad=False),
    "mse_window_norm/default": case("mse_window_norm_f32", y_hat=T(3, 9, 11), target=T(3, 10, 12, dtype=i16)),
}

# id -> (what reaches require_cuda and the C ABI, in order; the results; the workspace keys created)
EXPECTED = {
    'conv2d_coords_fwd': (
        ['require_cuda sat x_coords y_coords weight bias',
         'pv_conv2d_coords_fwd_f32 sat x_coords y_coords weight bias out0 6 3 9 11 32 stream'],
        ['(6, 32, 7, 9) float32'], []),
    'conv2d_coords_fwd/nobias': (
        ['require_cuda sat x_coords y_coords weight NULL',
         'pv_conv2d_coords_fwd_f32 sat x_coords y_coords weight NULL out0 6 3 9 11 32 stream'],
        ['(6, 32, 7, 9) float32'], []),
    'conv2d_fwd': (
        ['require_cuda x weight bias',
         'pv_conv2d_fwd_f32 x weight bias out0 2 32 4 9 11 1 stream'],
        ['(2, 4, 7, 9) float32'], []),
    'conv2d_fwd/none': (
        ['require_cuda x weight NULL',
         'pv_conv2d_fwd_f32 x weight NULL out0 2 32 4 9 11 0 stream'],
        ['(2, 4, 7, 9) float32'], []),
    'conv2d_bwd_data': (
        ['require_cuda dy dy_gate weight x_gate',
         'pv_conv2d_bwd_data_f32 dy dy_gate weight out0 x_gate 2 32 4 9 11 stream'],
        ['(2, 32, 9, 11) float32'], []),
    'conv2d_bwd_data/none': (
        ['require_cuda dy NULL weight NULL',
         'pv_conv2d_bwd_data_f32 dy NULL weight out0 NULL 2 32 4 9 11 stream'],
        ['(2, 32, 9, 11) float32'], []),
    'conv2d_bwd_weight': (
        ['require_cuda x dy dy_gate',
         'pv_conv2d_bwd_weight_workspace_bytes 2 32 4 9 11 &bytes',
         'pv_conv2d_bwd_weight_f32 x dy dy_gate out0 out1 2 32 4 9 11 ws:conv2d_wgrad 4096 stream'],
        ['(4, 32, 3, 3) float32', '(4,) float32'], ['conv2d_wgrad']),
    'conv2d_bwd_weight/none': (
        ['require_cuda x dy NULL',
         'pv_conv2d_bwd_weight_workspace_bytes 2 32 4 9 11 &bytes',
         'pv_conv2d_bwd_weight_f32 x dy NULL out0 out1 2 32 4 9 11 ws:conv2d_wgrad 4096 stream'],
        ['(4, 32, 3, 3) float32', '(4,) float32'], ['conv2d_wgrad']),
    'conv2d_coords_bwd_weight': (
        ['require_cuda sat x_coords y_coords dy',
         'pv_conv2d_bwd_weight_workspace_bytes 6 17 32 9 11 &bytes',
         'pv_conv2d_coords_bwd_weight_f32 sat x_coords y_coords dy out0 out1 6 3 9 11 32 ws:conv2d_wgrad 4096 stream'],
        ['(32, 17, 3, 3) float32', '(32,) float32'], ['conv2d_wgrad']),
    'conv2d144_sat_pool_fwd': (
        ['require_cuda sat x_coords y_coords weight bias',
         'pv_conv2d144_sat_pool_fwd_f32 sat x_coords y_coords weight bias out0 out1 2 5 3 9 11 144 stream'],
        ['(2, 144, 2, 3) float32', '(2, 144, 2, 3) uint8'], []),
    'conv2d144_sat_pool_fwd/5x5': (
        ['require_cuda sat x_coords y_coords weight bias',
         'pv_conv2d144_sat_pool_fwd_f32 sat x_coords y_coords weight bias out0 out1 2 5 3 5 5 144 stream'],
        ['(2, 144, 1, 1) float32', '(2, 144, 1, 1) uint8'], []),
    'conv2d144_pool_fwd': (
        ['require_cuda x weight bias',
         'pv_conv2d144_pool_fwd_f32 x weight bias out0 out1 2 144 144 9 11 stream'],
        ['(2, 144, 2, 3) float32', '(2, 144, 2, 3) uint8'], []),
    'conv2d144_pool_fwd/5x5': (
        ['require_cuda x weight bias',
         'pv_conv2d144_pool_fwd_f32 x weight bias out0 out1 1 144 144 5 5 stream'],
        ['(1, 144, 1, 1) float32', '(1, 144, 1, 1) uint8'], []),
    'conv2d144_fwd': (
        ['require_cuda x weight bias',
         'pv_conv2d144_fwd_f32 x weight bias out0 2 144 144 9 11 1 stream'],
        ['(2, 144, 7, 9) float32'], []),
    'conv2d144_fwd/none': (
        ['require_cuda x weight NULL',
         'pv_conv2d144_fwd_f32 x weight NULL out0 2 144 144 9 11 0 stream'],
        ['(2, 144, 7, 9) float32'], []),
    'conv2d144_bwd_data': (
        ['require_cuda dy dy_gate weight x_gate',
         'pv_conv2d144_bwd_data_f32 dy dy_gate weight out0 x_gate 2 144 144 9 11 stream'],
        ['(2, 144, 9, 11) float32'], []),
    'conv2d144_bwd_data/none': (
        ['require_cuda dy NULL weight NULL',
         'pv_conv2d144_bwd_data_f32 dy NULL weight out0 NULL 2 144 144 9 11 stream'],
        ['(2, 144, 9, 11) float32'], []),
    'conv2d144_pool_bwd_data': (
        ['require_cuda dy_pooled codes weight x_gate',
         'pv_conv2d144_pool_bwd_data_f32 dy_pooled codes weight out0 x_gate 2 144 144 9 11 stream'],
        ['(2, 144, 9, 11) float32'], []),
    'conv2d144_pool_bwd_data/none': (
        ['require_cuda dy_pooled codes weight NULL',
         'pv_conv2d144_pool_bwd_data_f32 dy_pooled codes weight out0 NULL 1 144 144 5 5 stream'],
        ['(1, 144, 5, 5) float32'], []),
    'conv2d144_bwd_weight': (
        ['require_cuda x dy dy_gate',
         'pv_conv2d144_bwd_weight_workspace_bytes 2 144 144 9 11 0 &bytes',
         'pv_conv2d144_bwd_weight_f32 x dy dy_gate out0 out1 2 144 144 9 11 ws:conv2d144_wgrad 4096 stream'],
        ['(144, 144, 3, 3) float32', '(144,) float32'], ['conv2d144_wgrad']),
    'conv2d144_bwd_weight/none': (
        ['require_cuda x dy NULL',
         'pv_conv2d144_bwd_weight_workspace_bytes 2 144 144 9 11 0 &bytes',
         'pv_conv2d144_bwd_weight_f32 x dy NULL out0 out1 2 144 144 9 11 ws:conv2d144_wgrad 4096 stream'],
        ['(144, 144, 3, 3) float32', '(144,) float32'], ['conv2d144_wgrad']),
    'conv2d144_pool_bwd_weight': (
        ['require_cuda x dy_pooled codes',
         'pv_conv2d144_bwd_weight_workspace_bytes 2 144 144 9 11 1 &bytes',
         'pv_conv2d144_pool_bwd_weight_f32 x dy_pooled codes out0 out1 2 144 144 9 11 ws:conv2d144_wgrad 4096 stream'],
        ['(144, 144, 3, 3) float32', '(144,) float32'], ['conv2d144_wgrad']),
    'conv2d144_pool_bwd_weight/5x5': (
        ['require_cuda x dy_pooled codes',
         'pv_conv2d144_bwd_weight_workspace_bytes 1 144 144 5 5 1 &bytes',
         'pv_conv2d144_pool_bwd_weight_f32 x dy_pooled codes out0 out1 1 144 144 5 5 ws:conv2d144_wgrad 4096 stream'],
        ['(144, 144, 3, 3) float32', '(144,) float32'], ['conv2d144_wgrad']),
    'conv2d144_sat_pool_bwd_weight': (
        ['require_cuda sat x_coords y_coords dy_pooled codes',
         'pv_conv2d144_bwd_weight_workspace_bytes 2 8 144 9 11 1 &bytes',
         'pv_conv2d144_sat_pool_bwd_weight_f32 sat x_coords y_coords dy_pooled codes out0 out1 2 5 3 9 11 144 ws:conv2d144_wgrad 4096 stream'],
        ['(144, 8, 3, 3) float32', '(144,) float32'], ['conv2d144_wgrad']),
    'conv2d_ae_counts_fwd': (
        ['require_cuda history flow_pred horizon',
         'require_cuda weight bias',
         'pv_conv2d_ae_counts_fwd_f32 history 1 flow_pred 0 horizon weight bias out0 2 9 11 16 stream'],
        ['(2, 16, 7, 9) float32'], []),
    'conv2d_ae_counts_fwd/rev': (
        ['require_cuda history flow_pred horizon',
         'require_cuda weight bias',
         'pv_conv2d_ae_counts_fwd_f32 history 0 flow_pred 1 horizon weight bias out0 2 9 11 16 stream'],
        ['(2, 16, 7, 9) float32'], []),
    'conv2d_ae_counts_bwd_weight': (
        ['require_cuda history flow_pred horizon',
         'require_cuda dy',
         'pv_conv2d_ae_bwd_weight_workspace_bytes 2 6 16 9 11 0 &bytes',
         'pv_conv2d_ae_counts_bwd_weight_f32 history 1 flow_pred 0 horizon dy out0 out1 2 9 11 16 ws:conv2d_ae_wgrad 4096 stream'],
        ['(16, 6, 3, 3) float32', '(16,) float32'], ['conv2d_ae_wgrad']),
    'conv2d_ae_counts_bwd_weight/rev': (
        ['require_cuda history flow_pred horizon',
         'require_cuda dy',
         'pv_conv2d_ae_bwd_weight_workspace_bytes 2 6 16 9 11 0 &bytes',
         'pv_conv2d_ae_counts_bwd_weight_f32 history 0 flow_pred 1 horizon dy out0 out1 2 9 11 16 ws:conv2d_ae_wgrad 4096 stream'],
        ['(16, 6, 3, 3) float32', '(16,) float32'], ['conv2d_ae_wgrad']),
    'conv2d_ae_fwd': (
        ['require_cuda x weight bias',
         'pv_conv2d_ae_fwd_f32 x weight bias out0 2 16 32 9 11 1 stream'],
        ['(2, 32, 7, 9) float32'], []),
    'conv2d_ae_fwd/none': (
        ['require_cuda x weight NULL',
         'pv_conv2d_ae_fwd_f32 x weight NULL out0 2 16 32 9 11 0 stream'],
        ['(2, 32, 7, 9) float32'], []),
    'conv2d_ae_bwd_data': (
        ['require_cuda dy dy_gate weight x_gate',
         'pv_conv2d_ae_bwd_data_f32 dy dy_gate weight out0 x_gate 2 16 32 9 11 stream'],
        ['(2, 16, 9, 11) float32'], []),
    'conv2d_ae_bwd_data/none': (
        ['require_cuda dy NULL weight NULL',
         'pv_conv2d_ae_bwd_data_f32 dy NULL weight out0 NULL 2 16 32 9 11 stream'],
        ['(2, 16, 9, 11) float32'], []),
    'conv2d_ae_bwd_weight': (
        ['require_cuda x dy dy_gate',
         'pv_conv2d_ae_bwd_weight_workspace_bytes 2 16 32 9 11 0 &bytes',
         'pv_conv2d_ae_bwd_weight_f32 x dy dy_gate out0 out1 2 16 32 9 11 ws:conv2d_ae_wgrad 4096 stream'],
        ['(32, 16, 3, 3) float32', '(32,) float32'], ['conv2d_ae_wgrad']),
    'conv2d_ae_bwd_weight/none': (
        ['require_cuda x dy NULL',
         'pv_conv2d_ae_bwd_weight_workspace_bytes 2 16 32 9 11 0 &bytes',
         'pv_conv2d_ae_bwd_weight_f32 x dy NULL out0 out1 2 16 32 9 11 ws:conv2d_ae_wgrad 4096 stream'],
        ['(32, 16, 3, 3) float32', '(32,) float32'], ['conv2d_ae_wgrad']),
    'conv2d_ae_pool_fwd': (
        ['require_cuda x weight bias',
         'pv_conv2d_ae_pool_fwd_workspace_bytes 2 32 16 9 11 &bytes',
         'pv_conv2d_ae_pool_fwd_f32 x weight bias out0 out1 2 32 16 9 11 ws:conv2d_ae_pool_fwd 4096 stream'],
        ['(2, 16, 2, 3) float32', '(2, 16, 2, 3) uint8'], ['conv2d_ae_pool_fwd']),
    'conv2d_ae_pool_fwd/no_workspace': (
        ['require_cuda x weight bias',
         'pv_conv2d_ae_pool_fwd_workspace_bytes 2 32 16 9 11 &bytes',
         'pv_conv2d_ae_pool_fwd_f32 x weight bias out0 out1 2 32 16 9 11 NULL 0 stream'],
        ['(2, 16, 2, 3) float32', '(2, 16, 2, 3) uint8'], []),
    'conv2d_ae_pool_fwd/5x5': (
        ['require_cuda x weight bias',
         'pv_conv2d_ae_pool_fwd_workspace_bytes 1 32 16 5 5 &bytes',
         'pv_conv2d_ae_pool_fwd_f32 x weight bias out0 out1 1 32 16 5 5 ws:conv2d_ae_pool_fwd 4096 stream'],
        ['(1, 16, 1, 1) float32', '(1, 16, 1, 1) uint8'], ['conv2d_ae_pool_fwd']),
    'conv2d_ae_pool_bwd_data': (
        ['require_cuda dy_pooled codes weight x_gate',
         'pv_conv2d_ae_pool_bwd_data_f32 dy_pooled codes weight out0 x_gate 2 32 16 9 11 stream'],
        ['(2, 32, 9, 11) float32'], []),
    'conv2d_ae_pool_bwd_data/none': (
        ['require_cuda dy_pooled codes weight NULL',
         'pv_conv2d_ae_pool_bwd_data_f32 dy_pooled codes weight out0 NULL 1 32 16 5 5 stream'],
        ['(1, 32, 5, 5) float32'], []),
    'conv2d_ae_pool_bwd_weight': (
        ['require_cuda x dy_pooled codes',
         'pv_conv2d_ae_bwd_weight_workspace_bytes 2 32 16 9 11 1 &bytes',
         'pv_conv2d_ae_pool_bwd_weight_f32 x dy_pooled codes out0 out1 2 32 16 9 11 ws:conv2d_ae_wgrad 4096 stream'],
        ['(16, 32, 3, 3) float32', '(16,) float32'], ['conv2d_ae_wgrad']),
    'conv2d_ae_pool_bwd_weight/5x5': (
        ['require_cuda x dy_pooled codes',
         'pv_conv2d_ae_bwd_weight_workspace_bytes 1 32 16 5 5 1 &bytes',
         'pv_conv2d_ae_pool_bwd_weight_f32 x dy_pooled codes out0 out1 1 32 16 5 5 ws:conv2d_ae_wgrad 4096 stream'],
        ['(16, 32, 3, 3) float32', '(16,) float32'], ['conv2d_ae_wgrad']),
    'convt2d_ae_fwd': (
        ['require_cuda x weight bias',
         'pv_convt2d_ae_fwd_f32 x weight bias out0 2 32 16 9 11 1 stream'],
        ['(2, 16, 11, 13) float32'], []),
    'convt2d_ae_fwd/none': (
        ['require_cuda x weight NULL',
         'pv_convt2d_ae_fwd_f32 x weight NULL out0 2 32 16 9 11 0 stream'],
        ['(2, 16, 11, 13) float32'], []),
    'convt2d_ae_bwd_data': (
        ['require_cuda dy dy_gate weight x_gate',
         'pv_convt2d_ae_bwd_data_f32 dy dy_gate weight out0 x_gate 2 32 16 9 11 stream'],
        ['(2, 32, 9, 11) float32'], []),
    'convt2d_ae_bwd_data/none': (
        ['require_cuda dy NULL weight NULL',
         'pv_convt2d_ae_bwd_data_f32 dy NULL weight out0 NULL 2 32 16 9 11 stream'],
        ['(2, 32, 9, 11) float32'], []),
    'convt2d_ae_bwd_weight': (
        ['require_cuda x dy dy_gate',
         'pv_convt2d_ae_bwd_weight_workspace_bytes 2 32 16 9 11 &bytes',
         'pv_convt2d_ae_bwd_weight_f32 x dy dy_gate out0 out1 2 32 16 9 11 ws:convt2d_ae_wgrad 4096 stream'],
        ['(32, 16, 3, 3) float32', '(16,) float32'], ['convt2d_ae_wgrad']),
    'convt2d_ae_bwd_weight/none': (
        ['require_cuda x dy NULL',
         'pv_convt2d_ae_bwd_weight_workspace_bytes 2 32 16 9 11 &bytes',
         'pv_convt2d_ae_bwd_weight_f32 x dy NULL out0 out1 2 32 16 9 11 ws:convt2d_ae_wgrad 4096 stream'],
        ['(32, 16, 3, 3) float32', '(16,) float32'], ['convt2d_ae_wgrad']),
    'mse_crop_norm': (
        ['require_cuda y_hat target',
         'pv_mse_crop_norm_f32 y_hat target 1 2 9 11 25 27 out0 out1 ws:mse_crop_norm 8 stream'],
        ['(1,) float32', '(2, 9, 11) float32'], ['mse_crop_norm']),
    'mse_crop_norm/f32_nograd': (
        ['require_cuda y_hat target',
         'pv_mse_crop_norm_f32 y_hat target 0 2 9 11 25 27 out0 NULL ws:mse_crop_norm 8 stream'],
        ['(1,) float32', 'None'], ['mse_crop_norm']),
    'mse_crop_norm/default': (
        ['require_cuda y_hat target',
         'pv_mse_crop_norm_f32 y_hat target 0 3 9 11 25 27 out0 out1 ws:mse_crop_norm 12 stream'],
        ['(1,) float32', '(3, 9, 11) float32'], ['mse_crop_norm']),
    'conv2d_s2_counts_fwd': (
        ['require_cuda history flow_pred horizon',
         'require_cuda weight bias',
         'pv_conv2d_s2_counts_fwd_f32 history 1 flow_pred 0 horizon weight bias out0 2 9 11 16 stream'],
        ['(2, 16, 4, 5) float32'], []),
    'conv2d_s2_counts_fwd/even_rev': (
        ['require_cuda history flow_pred horizon',
         'require_cuda weight bias',
         'pv_conv2d_s2_counts_fwd_f32 history 0 flow_pred 1 horizon weight bias out0 2 10 12 16 stream'],
        ['(2, 16, 4, 5) float32'], []),
    'conv2d_s2_counts_bwd_weight': (
        ['require_cuda history flow_pred horizon',
         'require_cuda dy',
         'pv_conv2d_s2_bwd_weight_workspace_bytes 2 6 16 10 12 &bytes',
         'pv_conv2d_s2_counts_bwd_weight_f32 history 1 flow_pred 0 horizon dy out0 out1 2 10 12 16 ws:conv2d_s2_wgrad 4096 stream'],
        ['(16, 6, 3, 3) float32', '(16,) float32'], ['conv2d_s2_wgrad']),
    'conv2d_s2_counts_bwd_weight/odd_rev': (
        ['require_cuda history flow_pred horizon',
         'require_cuda dy',
         'pv_conv2d_s2_bwd_weight_workspace_bytes 2 6 16 9 11 &bytes',
         'pv_conv2d_s2_counts_bwd_weight_f32 history 0 flow_pred 1 horizon dy out0 out1 2 9 11 16 ws:conv2d_s2_wgrad 4096 stream'],
        ['(16, 6, 3, 3) float32', '(16,) float32'], ['conv2d_s2_wgrad']),
    'conv2d_s2_fwd': (
        ['require_cuda x weight bias',
         'pv_conv2d_s2_fwd_f32 x weight bias out0 2 16 32 9 11 1 stream'],
        ['(2, 32, 4, 5) float32'], []),
    'conv2d_s2_fwd/even_none': (
        ['require_cuda x weight NULL',
         'pv_conv2d_s2_fwd_f32 x weight NULL out0 2 16 32 10 12 0 stream'],
        ['(2, 32, 4, 5) float32'], []),
    'conv2d_s2_fwd/12x13': (
        ['require_cuda x weight bias',
         'pv_conv2d_s2_fwd_f32 x weight bias out0 2 16 32 12 13 1 stream'],
        ['(2, 32, 5, 6) float32'], []),
    'conv2d_s2_bwd_data': (
        ['require_cuda dy dy_gate weight x_gate',
         'pv_conv2d_s2_bwd_data_f32 dy dy_gate weight out0 x_gate 2 16 32 9 11 stream'],
        ['(2, 16, 9, 11) float32'], []),
    'conv2d_s2_bwd_data/even_none': (
        ['require_cuda dy NULL weight NULL',
         'pv_conv2d_s2_bwd_data_f32 dy NULL weight out0 NULL 2 16 32 10 12 stream'],
        ['(2, 16, 10, 12) float32'], []),
    'conv2d_s2_bwd_weight': (
        ['require_cuda x dy dy_gate',
         'pv_conv2d_s2_bwd_weight_workspace_bytes 2 16 32 9 11 &bytes',
         'pv_conv2d_s2_bwd_weight_f32 x dy dy_gate out0 out1 2 16 32 9 11 ws:conv2d_s2_wgrad 4096 stream'],
        ['(32, 16, 3, 3) float32', '(32,) float32'], ['conv2d_s2_wgrad']),
    'conv2d_s2_bwd_weight/even_none': (
        ['require_cuda x dy NULL',
         'pv_conv2d_s2_bwd_weight_workspace_bytes 2 16 32 10 12 &bytes',
         'pv_conv2d_s2_bwd_weight_f32 x dy NULL out0 out1 2 16 32 10 12 ws:conv2d_s2_wgrad 4096 stream'],
        ['(32, 16, 3, 3) float32', '(32,) float32'], ['conv2d_s2_wgrad']),
    'convt2d_s2_fwd': (
        ['require_cuda x weight bias',
         'pv_convt2d_s2_fwd_f32 x weight bias out0 2 32 16 9 11 1 stream'],
        ['(2, 16, 19, 23) float32'], []),
    'convt2d_s2_fwd/none': (
        ['require_cuda x weight NULL',
         'pv_convt2d_s2_fwd_f32 x weight NULL out0 2 32 16 9 11 0 stream'],
        ['(2, 16, 19, 23) float32'], []),
    'convt2d_s2_bwd_data': (
        ['require_cuda dy dy_gate weight x_gate',
         'pv_convt2d_s2_bwd_data_f32 dy dy_gate weight out0 x_gate 2 32 16 9 11 stream'],
        ['(2, 32, 9, 11) float32'], []),
    'convt2d_s2_bwd_data/none': (
        ['require_cuda dy NULL weight NULL',
         'pv_convt2d_s2_bwd_data_f32 dy NULL weight out0 NULL 2 32 16 9 11 stream'],
        ['(2, 32, 9, 11) float32'], []),
    'convt2d_s2_bwd_weight': (
        ['require_cuda x dy dy_gate',
         'pv_convt2d_s2_bwd_weight_workspace_bytes 2 32 16 9 11 &bytes',
         'pv_convt2d_s2_bwd_weight_f32 x dy dy_gate out0 out1 2 32 16 9 11 ws:convt2d_s2_wgrad 4096 stream'],
        ['(32, 16, 3, 3) float32', '(16,) float32'], ['convt2d_s2_wgrad']),
    'convt2d_s2_bwd_weight/none': (
        ['require_cuda x dy NULL',
         'pv_convt2d_s2_bwd_weight_workspace_bytes 2 32 16 9 11 &bytes',
         'pv_convt2d_s2_bwd_weight_f32 x dy NULL out0 out1 2 32 16 9 11 ws:convt2d_s2_wgrad 4096 stream'],
        ['(32, 16, 3, 3) float32', '(16,) float32'], ['convt2d_s2_wgrad']),
    'mse_window_norm': (
        ['require_cuda y_hat target',
         'pv_mse_window_norm_f32 y_hat target 1 2 9 11 12 14 1 2 out0 out1 ws:mse_window_norm 8 stream'],
        ['(1,) float32', '(2, 9, 11) float32'], ['mse_window_norm']),
    'mse_window_norm/f32_nograd': (
        ['require_cuda y_hat target',
         'pv_mse_window_norm_f32 y_hat target 0 2 9 11 12 14 1 2 out0 NULL ws:mse_window_norm 8 stream'],
        ['(1,) float32', 'None'], ['mse_window_norm']),
    'mse_window_norm/default': (
        ['require_cuda y_hat target',
         'pv_mse_window_norm_f32 y_hat target 1 3 9 11 10 12 0 0 out0 out1 ws:mse_window_norm 12 stream'],
        ['(1,) float32', '(3, 9, 11) float32'], ['mse_window_norm']),
}

# (case, the arguments replaced, the error's type and whole text, what had reached require_cuda before it was raised);
# no error is raised after anything has reached the C ABI
ERRORS = [
    ('conv2d_coords_fwd', dict(x_coords=T(2, 9)), ValueError,
     'conv2d_coords_fwd_f32: x_coords [2, 11] and y_coords [2, 9] expected, got (2, 9) / (2, 9)',
     []),
    ('conv2d_coords_fwd', dict(y_coords=T(3, 9)), ValueError,
     'conv2d_coords_fwd_f32: x_coords [2, 11] and y_coords [2, 9] expected, got (2, 11) / (3, 9)',
     []),
    ('conv2d_coords_fwd', dict(t_per_example=4), ValueError,
     'conv2d_coords_fwd_f32: sat [N, H, W, 12] with N a multiple of t_per_example=4, got (6, 9, 11, 12)',
     []),
    ('conv2d_coords_fwd', dict(sat=T(6, 9, 11, 11)), ValueError,
     'conv2d_coords_fwd_f32: sat [N, H, W, 12] with N a multiple of t_per_example=3, got (6, 9, 11, 11)',
     []),
    ('conv2d_coords_fwd', dict(weight=T(32, 12, 3, 3)), ValueError,
     'conv2d_coords_fwd_f32: weight [C_out, 17, 3, 3] expected, got (32, 12, 3, 3)',
     []),
    ('conv2d_coords_fwd', dict(bias=T(17)), ValueError,
     'conv2d_coords_fwd_f32: bias [32] expected, got (17,)',
     []),
    ('conv2d_coords_fwd', dict(sat=T(6, 9, 11, 12, dtype=f64)), TypeError,
     'conv2d kernels take contiguous float32 tensors',
     ['require_cuda sat x_coords y_coords weight bias']),
    ('conv2d_coords_fwd', dict(x_coords=T(2, 11, contiguous=False)), TypeError,
     'conv2d kernels take contiguous float32 tensors',
     ['require_cuda sat x_coords y_coords weight bias']),
    ('conv2d_fwd', dict(weight=T(4, 16, 3, 3)), ValueError,
     'conv2d_fwd_f32: weight [C_out, 32, 3, 3] expected for x (2, 32, 9, 11), got (4, 16, 3, 3)',
     []),
    ('conv2d_fwd', dict(weight=T(4, 32, 3)), ValueError,
     'conv2d_fwd_f32: weight [C_out, 32, 3, 3] expected for x (2, 32, 9, 11), got (4, 32, 3)',
     []),
    ('conv2d_fwd', dict(bias=T(32)), ValueError,
     'conv2d_fwd_f32: bias [4] expected, got (32,)',
     []),
    ('conv2d_fwd', dict(x=T(2, 32, 9, 11, contiguous=False)), TypeError,
     'conv2d kernels take contiguous float32 tensors',
     ['require_cuda x weight bias']),
    ('conv2d_fwd', dict(weight=T(4, 32, 3, 3, dtype=f64)), TypeError,
     'conv2d kernels take contiguous float32 tensors',
     ['require_cuda x weight bias']),
    ('conv2d_bwd_data', dict(weight=T(4, 16, 3, 3)), ValueError,
     'conv2d_bwd_data_f32: weight [C_out, 32, 3, 3] expected for x (2, 32, 9, 11), got (4, 16, 3, 3)',
     []),
    ('conv2d_bwd_data', dict(dy=T(2, 4, 7, 8)), ValueError,
     'conv2d_bwd_data_f32: dy / dy_gate (2, 4, 7, 9) expected, got (2, 4, 7, 8)',
     []),
    ('conv2d_bwd_data', dict(dy_gate=T(2, 4, 8, 9)), ValueError,
     'conv2d_bwd_data_f32: dy / dy_gate (2, 4, 7, 9) expected, got (2, 4, 7, 9)',
     []),
    ('conv2d_bwd_data', dict(x_gate=T(2, 32, 9, 10)), ValueError,
     'conv2d_bwd_data_f32: x_gate (2, 32, 9, 11) expected',
     []),
    ('conv2d_bwd_data', dict(dy=T(2, 4, 7, 9, contiguous=False)), TypeError,
     'conv2d kernels take contiguous float32 tensors',
     ['require_cuda dy dy_gate weight x_gate']),
    ('conv2d_bwd_data', dict(x_gate=T(2, 32, 9, 11, dtype=i16)), TypeError,
     'conv2d kernels take contiguous float32 tensors',
     ['require_cuda dy dy_gate weight x_gate']),
    ('conv2d_bwd_weight', dict(weight_shape=(4, 16, 3, 3)), ValueError,
     'conv2d_bwd_weight_f32: weight [C_out, 32, 3, 3] expected for x (2, 32, 9, 11), got (4, 16, 3, 3)',
     []),
    ('conv2d_bwd_weight', dict(dy=T(2, 4, 9, 7)), ValueError,
     'conv2d_bwd_weight_f32: dy / dy_gate (2, 4, 7, 9) expected, got (2, 4, 9, 7)',
     []),
    ('conv2d_bwd_weight', dict(dy_gate=T(2, 4, 7, 10)), ValueError,
     'conv2d_bwd_weight_f32: dy / dy_gate (2, 4, 7, 9) expected, got (2, 4, 7, 9)',
     []),
    ('conv2d_bwd_weight', dict(dy_gate=T(2, 4, 7, 9, contiguous=False)), TypeError,
     'conv2d kernels take contiguous float32 tensors',
     ['require_cuda x dy dy_gate']),
    ('conv2d_bwd_weight', dict(x=T(2, 32, 9, 11, dtype=f64)), TypeError,
     'conv2d kernels take contiguous float32 tensors',
     ['require_cuda x dy dy_gate']),
    ('conv2d_coords_bwd_weight', dict(y_coords=T(2, 11)), ValueError,
     'conv2d_coords_bwd_weight_f32: x_coords [2, 11] and y_coords [2, 9] expected, got (2, 11) / (2, 11)',
     []),
    ('conv2d_coords_bwd_weight', dict(weight_shape=(32, 12, 3, 3)), ValueError,
     'conv2d_coords_bwd_weight_f32: weight (32, 17, 3, 3) and dy (6, 32, 7, 9) expected, got (32, 12, 3, 3) / (6, 32, 7, 9)',
     []),
    ('conv2d_coords_bwd_weight', dict(dy=T(6, 32, 7, 8)), ValueError,
     'conv2d_coords_bwd_weight_f32: weight (32, 17, 3, 3) and dy (6, 32, 7, 9) expected, got (32, 17, 3, 3) / (6, 32, 7, 8)',
     []),
    ('conv2d_coords_bwd_weight', dict(dy=T(6, 32, 7, 9, contiguous=False)), TypeError,
     'conv2d kernels take contiguous float32 tensors',
     ['require_cuda sat x_coords y_coords dy']),
    ('conv2d144_sat_pool_fwd', dict(sat=T(2, 5, 9, 11)), ValueError,
     'conv2d144_sat_pool_fwd_f32: sat_data [B, T, H, W, 1] expected, got (2, 5, 9, 11)',
     []),
    ('conv2d144_sat_pool_fwd', dict(n_frames=6), ValueError,
     'conv2d144_sat_pool_fwd_f32: n_frames=6 must lie in 1..T=5',
     []),
    ('conv2d144_sat_pool_fwd', dict(sat=T(2, 5, 4, 4, 1), x_coords=T(2, 4), y_coords=T(2, 4)), ValueError,
     'conv2d144_sat_pool_fwd_f32: images of at least 5 x 5 expected, got 4 x 4',
     []),
    ('conv2d144_sat_pool_fwd', dict(x_coords=T(2, 9)), ValueError,
     'conv2d144_sat_pool_fwd_f32: x_coords [2, 11] and y_coords [2, 9] expected, got (2, 9) / (2, 9)',
     []),
    ('conv2d144_sat_pool_fwd', dict(weight=T(144, 10, 3, 3)), ValueError,
     'conv2d144_sat_pool_fwd_f32: weight [144, 8, 3, 3] expected, got (144, 10, 3, 3)',
     []),
    ('conv2d144_sat_pool_fwd', dict(bias=T(8)), ValueError,
     'conv2d144_sat_pool_fwd_f32: bias [144] expected',
     []),
    ('conv2d144_sat_pool_fwd', dict(bias=None), ValueError,
     'conv2d144_sat_pool_fwd_f32: bias [144] expected',
     []),
    ('conv2d144_sat_pool_fwd', dict(sat=T(2, 5, 9, 11, 1, dtype=i16)), TypeError,
     'conv2d kernels take contiguous float32 tensors',
     ['require_cuda sat x_coords y_coords weight bias']),
    ('conv2d144_pool_fwd', dict(x=T(2, 32, 9, 11)), ValueError,
     'conv2d144_pool_fwd_f32: x [N, 144, H, W] expected, got (2, 32, 9, 11)',
     []),
    ('conv2d144_pool_fwd', dict(weight=T(144, 32, 3, 3)), ValueError,
     'conv2d144_pool_fwd_f32: weight [144, 144, 3, 3] expected, got (144, 32, 3, 3)',
     []),
    ('conv2d144_pool_fwd', dict(x=T(1, 144, 4, 4)), ValueError,
     'conv2d144_pool_fwd_f32: images of at least 5 x 5 expected, got (1, 144, 4, 4)',
     []),
    ('conv2d144_pool_fwd', dict(bias=T(32)), ValueError,
     'conv2d144_pool_fwd_f32: bias [144] expected',
     []),
    ('conv2d144_pool_fwd', dict(bias=None), ValueError,
     'conv2d144_pool_fwd_f32: bias [144] expected',
     []),
    ('conv2d144_pool_fwd', dict(x=T(2, 144, 9, 11, contiguous=False)), TypeError,
     'conv2d kernels take contiguous float32 tensors',
     ['require_cuda x weight bias']),
    ('conv2d144_fwd', dict(x=T(2, 32, 9, 11)), ValueError,
     'conv2d144_fwd_f32: x [N, 144, H, W] expected, got (2, 32, 9, 11)',
     []),
    ('conv2d144_fwd', dict(weight=T(32, 144, 3, 3)), ValueError,
     'conv2d144_fwd_f32: weight [144, 144, 3, 3] expected, got (32, 144, 3, 3)',
     []),
    ('conv2d144_fwd', dict(x=T(1, 144, 2, 9)), ValueError,
     'conv2d144_fwd_f32: images of at least 3 x 3 expected, got (1, 144, 2, 9)',
     []),
    ('conv2d144_fwd', dict(bias=T(32)), ValueError,
     'conv2d144_fwd_f32: bias [144] expected, got (32,)',
     []),
    ('conv2d144_fwd', dict(bias=T(144, dtype=f64)), TypeError,
     'conv2d kernels take contiguous float32 tensors',
     ['require_cuda x weight bias']),
    ('conv2d144_bwd_data', dict(weight=T(144, 32, 3, 3)), ValueError,
     'conv2d144_bwd_data_f32: weight [144, 144, 3, 3] expected, got (144, 32, 3, 3)',
     []),
    ('conv2d144_bwd_data', dict(dy=T(2, 144, 7, 8)), ValueError,
     'conv2d144_bwd_data_f32: dy / dy_gate (2, 144, 7, 9) expected, got (2, 144, 7, 8)',
     []),
    ('conv2d144_bwd_data', dict(x_gate=T(2, 144, 9, 10)), ValueError,
     'conv2d144_bwd_data_f32: x_gate (2, 144, 9, 11) expected',
     []),
    ('conv2d144_bwd_data', dict(dy_gate=T(2, 144, 7, 9, contiguous=False)), TypeError,
     'conv2d kernels take contiguous float32 tensors',
     ['require_cuda dy dy_gate weight x_gate']),
    ('conv2d144_pool_bwd_data', dict(weight=T(144, 32, 3, 3)), ValueError,
     'conv2d144_pool_bwd_data_f32: weight [144, 144, 3, 3] expected, got (144, 32, 3, 3)',
     []),
    ('conv2d144_pool_bwd_data', dict(x_shape=(1, 144, 4, 4)), ValueError,
     'conv2d144_pool_bwd_data_f32: images of at least 5 x 5 expected, got (1, 144, 4, 4)',
     []),
    ('conv2d144_pool_bwd_data', dict(dy_pooled=T(2, 144, 3, 3)), ValueError,
     'conv2d144_pool_bwd_data_f32: dy_pooled / codes (2, 144, 2, 3) expected, got (2, 144, 3, 3) / (2, 144, 2, 3)',
     []),
    ('conv2d144_pool_bwd_data', dict(codes=T(2, 144, 2, 2, dtype=u8)), ValueError,
     'conv2d144_pool_bwd_data_f32: dy_pooled / codes (2, 144, 2, 3) expected, got (2, 144, 2, 3) / (2, 144, 2, 2)',
     []),
    ('conv2d144_pool_bwd_data', dict(x_gate=T(2, 144, 9, 10)), ValueError,
     'conv2d144_pool_bwd_data_f32: x_gate (2, 144, 9, 11) expected',
     []),
    ('conv2d144_pool_bwd_data', dict(codes=T(2, 144, 2, 3)), TypeError,
     'conv2d144_pool_bwd_data_f32: codes must be a contiguous uint8 tensor',
     ['require_cuda dy_pooled codes weight x_gate']),
    ('conv2d144_pool_bwd_data', dict(codes=T(2, 144, 2, 3, dtype=u8, contiguous=False)), TypeError,
     'conv2d144_pool_bwd_data_f32: codes must be a contiguous uint8 tensor',
     ['require_cuda dy_pooled codes weight x_gate']),
    ('conv2d144_pool_bwd_data', dict(dy_pooled=T(2, 144, 2, 3, dtype=f64)), TypeError,
     'conv2d kernels take contiguous float32 tensors',
     ['require_cuda dy_pooled codes weight x_gate']),
    ('conv2d144_bwd_weight', dict(weight_shape=(144, 32, 3, 3)), ValueError,
     'conv2d144_bwd_weight_f32: weight [144, 144, 3, 3] expected, got (144, 32, 3, 3)',
     []),
    ('conv2d144_bwd_weight', dict(dy=T(2, 144, 7, 8)), ValueError,
     'conv2d144_bwd_weight_f32: dy / dy_gate (2, 144, 7, 9) expected, got (2, 144, 7, 8)',
     []),
    ('conv2d144_bwd_weight', dict(dy_gate=T(2, 144, 7, 8)), ValueError,
     'conv2d144_bwd_weight_f32: dy / dy_gate (2, 144, 7, 9) expected, got (2, 144, 7, 9)',
     []),
    ('conv2d144_bwd_weight', dict(x=T(2, 144, 9, 11, contiguous=False)), TypeError,
     'conv2d kernels take contiguous float32 tensors',
     ['require_cuda x dy dy_gate']),
    ('conv2d144_pool_bwd_weight', dict(weight_shape=(144, 32, 3, 3)), ValueError,
     'conv2d144_pool_bwd_weight_f32: weight [144, 144, 3, 3] expected, got (144, 32, 3, 3)',
     []),
    ('conv2d144_pool_bwd_weight', dict(x=T(1, 144, 4, 4)), ValueError,
     'conv2d144_pool_bwd_weight_f32: images of at least 5 x 5 expected, got (1, 144, 4, 4)',
     []),
    ('conv2d144_pool_bwd_weight', dict(dy_pooled=T(2, 144, 3, 3)), ValueError,
     'conv2d144_pool_bwd_weight_f32: dy_pooled / codes (2, 144, 2, 3) expected, got (2, 144, 3, 3) / (2, 144, 2, 3)',
     []),
    ('conv2d144_pool_bwd_weight', dict(codes=T(2, 144, 2, 3, dtype=i16)), TypeError,
     'conv2d144_pool_bwd_weight_f32: codes must be a contiguous uint8 tensor',
     ['require_cuda x dy_pooled codes']),
    ('conv2d144_pool_bwd_weight', dict(x=T(2, 144, 9, 11, dtype=f64)), TypeError,
     'conv2d kernels take contiguous float32 tensors',
     ['require_cuda x dy_pooled codes']),
    ('conv2d144_sat_pool_bwd_weight', dict(y_coords=T(2, 11)), ValueError,
     'conv2d144_sat_pool_bwd_weight_f32: x_coords [2, 11] and y_coords [2, 9] expected, got (2, 11) / (2, 11)',
     []),
    ('conv2d144_sat_pool_bwd_weight', dict(n_frames=0), ValueError,
     'conv2d144_sat_pool_bwd_weight_f32: n_frames=0 must lie in 1..T=5',
     []),
    ('conv2d144_sat_pool_bwd_weight', dict(sat=T(2, 5, 4, 4, 1), x_coords=T(2, 4), y_coords=T(2, 4)), ValueError,
     'conv2d144_sat_pool_bwd_weight_f32: images of at least 5 x 5 expected, got 4 x 4',
     []),
    ('conv2d144_sat_pool_bwd_weight', dict(dy_pooled=T(2, 144, 3, 3)), ValueError,
     'conv2d144_sat_pool_bwd_weight_f32: dy_pooled / codes (2, 144, 2, 3) expected, got (2, 144, 3, 3) / (2, 144, 2, 3)',
     []),
    ('conv2d144_sat_pool_bwd_weight', dict(codes=T(2, 144, 2, 3)), TypeError,
     'conv2d144_sat_pool_bwd_weight_f32: codes must be a contiguous uint8 tensor',
     ['require_cuda sat x_coords y_coords dy_pooled codes']),
    ('conv2d144_sat_pool_bwd_weight', dict(dy_pooled=T(2, 144, 2, 3, contiguous=False)), TypeError,
     'conv2d kernels take contiguous float32 tensors',
     ['require_cuda sat x_coords y_coords dy_pooled codes']),
    ('conv2d_ae_counts_fwd', dict(history=T(2, 5, 9, 11, dtype=i16)), ValueError,
     'conv2d_ae_counts_fwd_f32: history [N, 4, H, W] expected, got (2, 5, 9, 11)',
     []),
    ('conv2d_ae_counts_fwd', dict(flow_pred=T(2, 9, 10)), ValueError,
     'conv2d_ae_counts_fwd_f32: flow prediction [2, 9, 11] and horizon [2] expected, got (2, 9, 10) / (2,)',
     []),
    ('conv2d_ae_counts_fwd', dict(horizon=T(3)), ValueError,
     'conv2d_ae_counts_fwd_f32: flow prediction [2, 9, 11] and horizon [2] expected, got (2, 9, 11) / (3,)',
     []),
    ('conv2d_ae_counts_fwd', dict(history=T(2, 4, 9, 11, dtype=u8)), TypeError,
     'conv2d_ae_counts_fwd_f32: counts must be contiguous int16 or float32 tensors, got torch.uint8',
     ['require_cuda history flow_pred horizon']),
    ('conv2d_ae_counts_fwd', dict(flow_pred=T(2, 9, 11, contiguous=False)), TypeError,
     'conv2d_ae_counts_fwd_f32: counts must be contiguous int16 or float32 tensors, got torch.float32',
     ['require_cuda history flow_pred horizon']),
    ('conv2d_ae_counts_fwd', dict(horizon=T(2, dtype=f64)), TypeError,
     'conv2d kernels take contiguous float32 tensors',
     ['require_cuda history flow_pred horizon']),
    ('conv2d_ae_counts_fwd', dict(weight=T(16, 4, 3, 3)), ValueError,
     'conv2d_ae_counts_fwd_f32: weight [C_out, 6, 3, 3] expected, got (16, 4, 3, 3)',
     ['require_cuda history flow_pred horizon']),
    ('conv2d_ae_counts_fwd', dict(bias=T(6)), ValueError,
     'conv2d_ae_counts_fwd_f32: bias [16] expected',
     ['require_cuda history flow_pred horizon']),
    ('conv2d_ae_counts_fwd', dict(bias=None), ValueError,
     'conv2d_ae_counts_fwd_f32: bias [16] expected',
     ['require_cuda history flow_pred horizon']),
    ('conv2d_ae_counts_fwd', dict(weight=T(16, 6, 3, 3, dtype=f64)), TypeError,
     'conv2d kernels take contiguous float32 tensors',
     ['require_cuda history flow_pred horizon',
      'require_cuda weight bias']),
    ('conv2d_ae_counts_bwd_weight', dict(history=T(2, 9, 11, dtype=i16)), ValueError,
     'conv2d_ae_counts_bwd_weight_f32: history [N, 4, H, W] expected, got (2, 9, 11)',
     []),
    ('conv2d_ae_counts_bwd_weight', dict(flow_pred=T(2, 1, 9, 11)), ValueError,
     'conv2d_ae_counts_bwd_weight_f32: flow prediction [2, 9, 11] and horizon [2] expected, got (2, 1, 9, 11) / (2,)',
     []),
    ('conv2d_ae_counts_bwd_weight', dict(horizon=T(2, 1)), ValueError,
     'conv2d_ae_counts_bwd_weight_f32: flow prediction [2, 9, 11] and horizon [2] expected, got (2, 9, 11) / (2, 1)',
     []),
    ('conv2d_ae_counts_bwd_weight', dict(weight_shape=(16, 4, 3, 3)), ValueError,
     'conv2d_ae_counts_bwd_weight_f32: weight (16, 6, 3, 3) and dy (2, 16, 7, 9) expected, got (16, 4, 3, 3) / (2, 16, 7, 9)',
     ['require_cuda history flow_pred horizon']),
    ('conv2d_ae_counts_bwd_weight', dict(dy=T(2, 16, 7, 8)), ValueError,
     'conv2d_ae_counts_bwd_weight_f32: weight (16, 6, 3, 3) and dy (2, 16, 7, 9) expected, got (16, 6, 3, 3) / (2, 16, 7, 8)',
     ['require_cuda history flow_pred horizon']),
    ('conv2d_ae_counts_bwd_weight', dict(history=T(2, 4, 1, 11, dtype=i16), flow_pred=T(2, 1, 11), dy=T(2, 16, 1, 9)), ValueError,
     'conv2d_ae_counts_bwd_weight_f32: weight (16, 6, 3, 3) and dy (2, 16, -1, 9) expected, got (16, 6, 3, 3) / (2, 16, 1, 9)',
     ['require_cuda history flow_pred horizon']),
    ('conv2d_ae_counts_bwd_weight', dict(dy=T(2, 16, 7, 9, contiguous=False)), TypeError,
     'conv2d kernels take contiguous float32 tensors',
     ['require_cuda history flow_pred horizon',
      'require_cuda dy']),
    ('conv2d_ae_counts_bwd_weight', dict(flow_pred=T(2, 9, 11, dtype=f64)), TypeError,
     'conv2d_ae_counts_bwd_weight_f32: counts must be contiguous int16 or float32 tensors, got torch.float64',
     ['require_cuda history flow_pred horizon']),
    ('conv2d_ae_fwd', dict(weight=T(32, 32, 3, 3)), ValueError,
     'conv2d_ae_fwd_f32: x [N, C_in, H, W] and weight [C_out, C_in, 3, 3] expected, got (2, 16, 9, 11) / (32, 32, 3, 3)',
     []),
    ('conv2d_ae_fwd', dict(x=T(16, 9, 11)), ValueError,
     'conv2d_ae_fwd_f32: x [N, C_in, H, W] and weight [C_out, C_in, 3, 3] expected, got (16, 9, 11) / (32, 16, 3, 3)',
     []),
    ('conv2d_ae_fwd', dict(bias=T(16)), ValueError,
     'conv2d_ae_fwd_f32: bias [32] expected, got (16,)',
     []),
    ('conv2d_ae_fwd', dict(x=T(2, 16, 9, 11, dtype=i16)), TypeError,
     'conv2d kernels take contiguous float32 tensors',
     ['require_cuda x weight bias']),
    ('conv2d_ae_bwd_data', dict(weight=T(32, 32, 3, 3)), ValueError,
     'conv2d_ae_bwd_data_f32: x [N, C_in, H, W] and weight [C_out, C_in, 3, 3] expected, got (2, 16, 9, 11) / (32, 32, 3, 3)',
     []),
    ('conv2d_ae_bwd_data', dict(dy=T(2, 16, 7, 9)), ValueError,
     'conv2d_ae_bwd_data_f32: dy / dy_gate (2, 32, 7, 9) expected, got (2, 16, 7, 9)',
     []),
    ('conv2d_ae_bwd_data', dict(dy_gate=T(2, 32, 9, 7)), ValueError,
     'conv2d_ae_bwd_data_f32: dy / dy_gate (2, 32, 7, 9) expected, got (2, 32, 7, 9)',
     []),
    ('conv2d_ae_bwd_data', dict(x_gate=T(2, 16, 11, 9)), ValueError,
     'conv2d_ae_bwd_data_f32: x_gate (2, 16, 9, 11) expected',
     []),
    ('conv2d_ae_bwd_data', dict(weight=T(32, 16, 3, 3, contiguous=False)), TypeError,
     'conv2d kernels take contiguous float32 tensors',
     ['require_cuda dy dy_gate weight x_gate']),
    ('conv2d_ae_bwd_weight', dict(weight_shape=(32, 32, 3, 3)), ValueError,
     'conv2d_ae_bwd_weight_f32: x [N, C_in, H, W] and weight [C_out, C_in, 3, 3] expected, got (2, 16, 9, 11) / (32, 32, 3, 3)',
     []),
    ('conv2d_ae_bwd_weight', dict(dy=T(2, 32, 8, 9)), ValueError,
     'conv2d_ae_bwd_weight_f32: dy / dy_gate (2, 32, 7, 9) expected, got (2, 32, 8, 9)',
     []),
    ('conv2d_ae_bwd_weight', dict(dy_gate=T(2, 32, 7, 9, dtype=f64)), TypeError,
     'conv2d kernels take contiguous float32 tensors',
     ['require_cuda x dy dy_gate']),
    ('conv2d_ae_pool_fwd', dict(weight=T(16, 16, 3, 3)), ValueError,
     'conv2d_ae_pool_fwd_f32: x [N, C_in, H, W] and weight [C_out, C_in, 3, 3] expected, got (2, 32, 9, 11) / (16, 16, 3, 3)',
     []),
    ('conv2d_ae_pool_fwd', dict(bias=T(32)), ValueError,
     'conv2d_ae_pool_fwd_f32: bias [16] expected',
     []),
    ('conv2d_ae_pool_fwd', dict(bias=None), ValueError,
     'conv2d_ae_pool_fwd_f32: bias [16] expected',
     []),
    ('conv2d_ae_pool_fwd', dict(x=T(1, 32, 4, 4)), ValueError,
     'images of at least 5 x 5 expected (one whole 3x3 pool window after the 3x3 conv), got 4 x 4',
     ['require_cuda x weight bias']),
    ('conv2d_ae_pool_fwd', dict(x=T(1, 32, 5, 4)), ValueError,
     'images of at least 5 x 5 expected (one whole 3x3 pool window after the 3x3 conv), got 5 x 4',
     ['require_cuda x weight bias']),
    ('conv2d_ae_pool_fwd', dict(x=T(2, 32, 9, 11, contiguous=False)), TypeError,
     'conv2d kernels take contiguous float32 tensors',
     ['require_cuda x weight bias']),
    ('conv2d_ae_pool_fwd', dict(x=T(1, 32, 4, 4, dtype=f64)), TypeError,
     'conv2d kernels take contiguous float32 tensors',
     ['require_cuda x weight bias']),
    ('conv2d_ae_pool_bwd_data', dict(weight=T(16, 16, 3, 3)), ValueError,
     'conv2d_ae_pool_bwd_data_f32: x [N, C_in, H, W] and weight [C_out, C_in, 3, 3] expected, got (2, 32, 9, 11) / (16, 16, 3, 3)',
     []),
    ('conv2d_ae_pool_bwd_data', dict(x_shape=(1, 32, 4, 4)), ValueError,
     'images of at least 5 x 5 expected (one whole 3x3 pool window after the 3x3 conv), got 4 x 4',
     []),
    ('conv2d_ae_pool_bwd_data', dict(dy_pooled=T(2, 32, 2, 3)), ValueError,
     'conv2d_ae_pool_bwd_data_f32: dy_pooled / codes (2, 16, 2, 3) expected, got (2, 32, 2, 3) / (2, 16, 2, 3)',
     []),
    ('conv2d_ae_pool_bwd_data', dict(codes=T(2, 16, 3, 2, dtype=u8)), ValueError,
     'conv2d_ae_pool_bwd_data_f32: dy_pooled / codes (2, 16, 2, 3) expected, got (2, 16, 2, 3) / (2, 16, 3, 2)',
     []),
    ('conv2d_ae_pool_bwd_data', dict(x_gate=T(2, 32, 9, 10)), ValueError,
     'conv2d_ae_pool_bwd_data_f32: x_gate (2, 32, 9, 11) expected',
     []),
    ('conv2d_ae_pool_bwd_data', dict(codes=T(2, 16, 2, 3)), TypeError,
     'conv2d_ae_pool_bwd_data_f32: codes must be a contiguous uint8 tensor',
     ['require_cuda dy_pooled codes weight x_gate']),
    ('conv2d_ae_pool_bwd_data', dict(x_gate=T(2, 32, 9, 11, contiguous=False)), TypeError,
     'conv2d kernels take contiguous float32 tensors',
     ['require_cuda dy_pooled codes weight x_gate']),
    ('conv2d_ae_pool_bwd_weight', dict(weight_shape=(16, 16, 3, 3)), ValueError,
     'conv2d_ae_pool_bwd_weight_f32: x [N, C_in, H, W] and weight [C_out, C_in, 3, 3] expected, got (2, 32, 9, 11) / (16, 16, 3, 3)',
     []),
    ('conv2d_ae_pool_bwd_weight', dict(x=T(1, 32, 4, 4)), ValueError,
     'images of at least 5 x 5 expected (one whole 3x3 pool window after the 3x3 conv), got 4 x 4',
     []),
    ('conv2d_ae_pool_bwd_weight', dict(dy_pooled=T(2, 16, 3, 3)), ValueError,
     'conv2d_ae_pool_bwd_weight_f32: dy_pooled / codes (2, 16, 2, 3) expected, got (2, 16, 3, 3) / (2, 16, 2, 3)',
     []),
    ('conv2d_ae_pool_bwd_weight', dict(codes=T(2, 16, 2, 3, dtype=u8, contiguous=False)), TypeError,
     'conv2d_ae_pool_bwd_weight_f32: codes must be a contiguous uint8 tensor',
     ['require_cuda x dy_pooled codes']),
    ('conv2d_ae_pool_bwd_weight', dict(dy_pooled=T(2, 16, 2, 3, dtype=f64)), TypeError,
     'conv2d kernels take contiguous float32 tensors',
     ['require_cuda x dy_pooled codes']),
    ('convt2d_ae_fwd', dict(weight=T(16, 32, 3, 3)), ValueError,
     'convt2d_ae_fwd_f32: x [N, C_in, H, W] and weight [C_in, C_out, 3, 3] expected, got (2, 32, 9, 11) / (16, 32, 3, 3)',
     []),
    ('convt2d_ae_fwd', dict(weight=T(32, 16, 3, 2)), ValueError,
     'convt2d_ae_fwd_f32: x [N, C_in, H, W] and weight [C_in, C_out, 3, 3] expected, got (2, 32, 9, 11) / (32, 16, 3, 2)',
     []),
    ('convt2d_ae_fwd', dict(bias=T(32)), ValueError,
     'convt2d_ae_fwd_f32: bias [16] expected, got (32,)',
     []),
    ('convt2d_ae_fwd', dict(bias=T(16, dtype=f64)), TypeError,
     'conv2d kernels take contiguous float32 tensors',
     ['require_cuda x weight bias']),
    ('convt2d_ae_bwd_data', dict(weight=T(16, 32, 3, 3)), ValueError,
     'convt2d_ae_bwd_data_f32: x [N, C_in, H, W] and weight [C_in, C_out, 3, 3] expected, got (2, 32, 9, 11) / (16, 32, 3, 3)',
     []),
    ('convt2d_ae_bwd_data', dict(dy=T(2, 32, 11, 13)), ValueError,
     'convt2d_ae_bwd_data_f32: dy / dy_gate (2, 16, 11, 13) expected, got (2, 32, 11, 13)',
     []),
    ('convt2d_ae_bwd_data', dict(dy_gate=T(2, 16, 7, 9)), ValueError,
     'convt2d_ae_bwd_data_f32: dy / dy_gate (2, 16, 11, 13) expected, got (2, 16, 11, 13)',
     []),
    ('convt2d_ae_bwd_data', dict(x_gate=T(2, 16, 9, 11)), ValueError,
     'convt2d_ae_bwd_data_f32: x_gate (2, 32, 9, 11) expected',
     []),
    ('convt2d_ae_bwd_data', dict(dy=T(2, 16, 11, 13, contiguous=False)), TypeError,
     'conv2d kernels take contiguous float32 tensors',
     ['require_cuda dy dy_gate weight x_gate']),
    ('convt2d_ae_bwd_weight', dict(weight_shape=(16, 32, 3, 3)), ValueError,
     'convt2d_ae_bwd_weight_f32: x [N, C_in, H, W] and weight [C_in, C_out, 3, 3] expected, got (2, 32, 9, 11) / (16, 32, 3, 3)',
     []),
    ('convt2d_ae_bwd_weight', dict(dy=T(2, 32, 11, 13)), ValueError,
     'convt2d_ae_bwd_weight_f32: dy / dy_gate (2, 16, 11, 13) expected, got (2, 32, 11, 13)',
     []),
    ('convt2d_ae_bwd_weight', dict(dy_gate=T(2, 16, 11, 12)), ValueError,
     'convt2d_ae_bwd_weight_f32: dy / dy_gate (2, 16, 11, 13) expected, got (2, 16, 11, 13)',
     []),
    ('convt2d_ae_bwd_weight', dict(x=T(2, 32, 9, 11, contiguous=False)), TypeError,
     'conv2d kernels take contiguous float32 tensors',
     ['require_cuda x dy dy_gate']),
    ('mse_crop_norm', dict(y_hat=T(2, 1, 9, 11)), ValueError,
     'mse_crop_norm_f32: y_hat [N, P, Q] and target [N, T, U] expected, got (2, 1, 9, 11) / (2, 25, 27)',
     []),
    ('mse_crop_norm', dict(target=T(3, 25, 27, dtype=i16)), ValueError,
     'mse_crop_norm_f32: y_hat [N, P, Q] and target [N, T, U] expected, got (2, 9, 11) / (3, 25, 27)',
     []),
    ('mse_crop_norm', dict(y_hat=T(2, 9, 11, dtype=f64)), TypeError,
     'conv2d kernels take contiguous float32 tensors',
     ['require_cuda y_hat target']),
    ('mse_crop_norm', dict(target=T(2, 25, 27, dtype=u8)), TypeError,
     'mse_crop_norm_f32: counts must be contiguous int16 or float32 tensors, got torch.uint8',
     ['require_cuda y_hat target']),
    ('mse_crop_norm', dict(target=T(2, 25, 27, dtype=i16, contiguous=False)), TypeError,
     'mse_crop_norm_f32: counts must be contiguous int16 or float32 tensors, got torch.int16',
     ['require_cuda y_hat target']),
    ('conv2d_s2_counts_fwd', dict(history=T(2, 5, 9, 11, dtype=i16)), ValueError,
     'conv2d_s2_counts_fwd_f32: history [N, 4, H, W] expected, got (2, 5, 9, 11)',
     []),
    ('conv2d_s2_counts_fwd', dict(flow_pred=T(2, 11, 9)), ValueError,
     'conv2d_s2_counts_fwd_f32: flow prediction [2, 9, 11] and horizon [2] expected, got (2, 11, 9) / (2,)',
     []),
    ('conv2d_s2_counts_fwd', dict(horizon=T(1)), ValueError,
     'conv2d_s2_counts_fwd_f32: flow prediction [2, 9, 11] and horizon [2] expected, got (2, 9, 11) / (1,)',
     []),
    ('conv2d_s2_counts_fwd', dict(history=T(2, 4, 9, 11, dtype=f64)), TypeError,
     'conv2d_s2_counts_fwd_f32: counts must be contiguous int16 or float32 tensors, got torch.float64',
     ['require_cuda history flow_pred horizon']),
    ('conv2d_s2_counts_fwd', dict(history=T(2, 4, 9, 11, dtype=i16, contiguous=False)), TypeError,
     'conv2d_s2_counts_fwd_f32: counts must be contiguous int16 or float32 tensors, got torch.int16',
     ['require_cuda history flow_pred horizon']),
    ('conv2d_s2_counts_fwd', dict(weight=T(16, 6, 3)), ValueError,
     'conv2d_s2_counts_fwd_f32: weight [C_out, 6, 3, 3] expected, got (16, 6, 3)',
     ['require_cuda history flow_pred horizon']),
    ('conv2d_s2_counts_fwd', dict(bias=T(6)), ValueError,
     'conv2d_s2_counts_fwd_f32: bias [16] expected',
     ['require_cuda history flow_pred horizon']),
    ('conv2d_s2_counts_fwd', dict(bias=None), ValueError,
     'conv2d_s2_counts_fwd_f32: bias [16] expected',
     ['require_cuda history flow_pred horizon']),
    ('conv2d_s2_counts_fwd', dict(bias=T(16, dtype=f64)), TypeError,
     'conv2d kernels take contiguous float32 tensors',
     ['require_cuda history flow_pred horizon',
      'require_cuda weight bias']),
    ('conv2d_s2_counts_bwd_weight', dict(flow_pred=T(2, 10, 11)), ValueError,
     'conv2d_s2_counts_bwd_weight_f32: flow prediction [2, 10, 12] and horizon [2] expected, got (2, 10, 11) / (2,)',
     []),
    ('conv2d_s2_counts_bwd_weight', dict(horizon=T(4)), ValueError,
     'conv2d_s2_counts_bwd_weight_f32: flow prediction [2, 10, 12] and horizon [2] expected, got (2, 10, 12) / (4,)',
     []),
    ('conv2d_s2_counts_bwd_weight', dict(weight_shape=(16, 4, 3, 3)), ValueError,
     'conv2d_s2_counts_bwd_weight_f32: weight (16, 6, 3, 3) and dy (2, 16, 4, 5) expected, got (16, 4, 3, 3) / (2, 16, 4, 5)',
     ['require_cuda history flow_pred horizon']),
    ('conv2d_s2_counts_bwd_weight', dict(dy=T(2, 16, 5, 5)), ValueError,
     'conv2d_s2_counts_bwd_weight_f32: weight (16, 6, 3, 3) and dy (2, 16, 4, 5) expected, got (16, 6, 3, 3) / (2, 16, 5, 5)',
     ['require_cuda history flow_pred horizon']),
    ('conv2d_s2_counts_bwd_weight', dict(dy=T(2, 16, 8, 10)), ValueError,
     'conv2d_s2_counts_bwd_weight_f32: weight (16, 6, 3, 3) and dy (2, 16, 4, 5) expected, got (16, 6, 3, 3) / (2, 16, 8, 10)',
     ['require_cuda history flow_pred horizon']),
    ('conv2d_s2_counts_bwd_weight', dict(dy=T(2, 16, 4, 5, dtype=f64)), TypeError,
     'conv2d kernels take contiguous float32 tensors',
     ['require_cuda history flow_pred horizon',
      'require_cuda dy']),
    ('conv2d_s2_counts_bwd_weight', dict(history=T(2, 4, 10, 12, dtype=u8)), TypeError,
     'conv2d_s2_counts_bwd_weight_f32: counts must be contiguous int16 or float32 tensors, got torch.uint8',
     ['require_cuda history flow_pred horizon']),
    ('conv2d_s2_fwd', dict(weight=T(32, 32, 3, 3)), ValueError,
     'conv2d_s2_fwd_f32: x [N, C_in, H, W] and weight [C_out, C_in, 3, 3] expected, got (2, 16, 9, 11) / (32, 32, 3, 3)',
     []),
    ('conv2d_s2_fwd', dict(bias=T(16)), ValueError,
     'conv2d_s2_fwd_f32: bias [32] expected, got (16,)',
     []),
    ('conv2d_s2_fwd', dict(bias=T(32, dtype=f64)), TypeError,
     'conv2d kernels take contiguous float32 tensors',
     ['require_cuda x weight bias']),
    ('conv2d_s2_bwd_data', dict(weight=T(32, 32, 3, 3)), ValueError,
     'conv2d_s2_bwd_data_f32: x [N, C_in, H, W] and weight [C_out, C_in, 3, 3] expected, got (2, 16, 9, 11) / (32, 32, 3, 3)',
     []),
    ('conv2d_s2_bwd_data', dict(dy=T(2, 32, 7, 9)), ValueError,
     'conv2d_s2_bwd_data_f32: dy / dy_gate (2, 32, 4, 5) expected, got (2, 32, 7, 9)',
     []),
    ('conv2d_s2_bwd_data', dict(dy=T(2, 32, 5, 5)), ValueError,
     'conv2d_s2_bwd_data_f32: dy / dy_gate (2, 32, 4, 5) expected, got (2, 32, 5, 5)',
     []),
    ('conv2d_s2_bwd_data', dict(dy_gate=T(2, 32, 4, 4)), ValueError,
     'conv2d_s2_bwd_data_f32: dy / dy_gate (2, 32, 4, 5) expected, got (2, 32, 4, 5)',
     []),
    ('conv2d_s2_bwd_data', dict(x_gate=T(2, 16, 10, 12)), ValueError,
     'conv2d_s2_bwd_data_f32: x_gate (2, 16, 9, 11) expected',
     []),
    ('conv2d_s2_bwd_data', dict(x_gate=T(2, 16, 9, 11, contiguous=False)), TypeError,
     'conv2d kernels take contiguous float32 tensors',
     ['require_cuda dy dy_gate weight x_gate']),
    ('conv2d_s2_bwd_weight', dict(weight_shape=(32, 32, 3, 3)), ValueError,
     'conv2d_s2_bwd_weight_f32: x [N, C_in, H, W] and weight [C_out, C_in, 3, 3] expected, got (2, 16, 9, 11) / (32, 32, 3, 3)',
     []),
    ('conv2d_s2_bwd_weight', dict(dy=T(2, 32, 7, 9)), ValueError,
     'conv2d_s2_bwd_weight_f32: dy / dy_gate (2, 32, 4, 5) expected, got (2, 32, 7, 9)',
     []),
    ('conv2d_s2_bwd_weight', dict(dy_gate=T(2, 16, 4, 5)), ValueError,
     'conv2d_s2_bwd_weight_f32: dy / dy_gate (2, 32, 4, 5) expected, got (2, 32, 4, 5)',
     []),
    ('conv2d_s2_bwd_weight', dict(x=T(2, 16, 9, 11, dtype=f64)), TypeError,
     'conv2d kernels take contiguous float32 tensors',
     ['require_cuda x dy dy_gate']),
    ('convt2d_s2_fwd', dict(weight=T(16, 32, 3, 3)), ValueError,
     'convt2d_s2_fwd_f32: x [N, C_in, H, W] and weight [C_in, C_out, 3, 3] expected, got (2, 32, 9, 11) / (16, 32, 3, 3)',
     []),
    ('convt2d_s2_fwd', dict(bias=T(32)), ValueError,
     'convt2d_s2_fwd_f32: bias [16] expected, got (32,)',
     []),
    ('convt2d_s2_fwd', dict(weight=T(32, 16, 3, 3, contiguous=False)), TypeError,
     'conv2d kernels take contiguous float32 tensors',
     ['require_cuda x weight bias']),
    ('convt2d_s2_bwd_data', dict(weight=T(16, 32, 3, 3)), ValueError,
     'convt2d_s2_bwd_data_f32: x [N, C_in, H, W] and weight [C_in, C_out, 3, 3] expected, got (2, 32, 9, 11) / (16, 32, 3, 3)',
     []),
    ('convt2d_s2_bwd_data', dict(dy=T(2, 32, 19, 23)), ValueError,
     'convt2d_s2_bwd_data_f32: dy / dy_gate (2, 16, 19, 23) expected, got (2, 32, 19, 23)',
     []),
    ('convt2d_s2_bwd_data', dict(dy=T(2, 16, 18, 22)), ValueError,
     'convt2d_s2_bwd_data_f32: dy / dy_gate (2, 16, 19, 23) expected, got (2, 16, 18, 22)',
     []),
    ('convt2d_s2_bwd_data', dict(dy_gate=T(2, 16, 11, 13)), ValueError,
     'convt2d_s2_bwd_data_f32: dy / dy_gate (2, 16, 19, 23) expected, got (2, 16, 19, 23)',
     []),
    ('convt2d_s2_bwd_data', dict(x_gate=T(2, 16, 9, 11)), ValueError,
     'convt2d_s2_bwd_data_f32: x_gate (2, 32, 9, 11) expected',
     []),
    ('convt2d_s2_bwd_data', dict(dy_gate=T(2, 16, 19, 23, dtype=f64)), TypeError,
     'conv2d kernels take contiguous float32 tensors',
     ['require_cuda dy dy_gate weight x_gate']),
    ('convt2d_s2_bwd_weight', dict(weight_shape=(16, 32, 3, 3)), ValueError,
     'convt2d_s2_bwd_weight_f32: x [N, C_in, H, W] and weight [C_in, C_out, 3, 3] expected, got (2, 32, 9, 11) / (16, 32, 3, 3)',
     []),
    ('convt2d_s2_bwd_weight', dict(dy=T(2, 32, 19, 23)), ValueError,
     'convt2d_s2_bwd_weight_f32: dy / dy_gate (2, 16, 19, 23) expected, got (2, 32, 19, 23)',
     []),
    ('convt2d_s2_bwd_weight', dict(dy_gate=T(2, 16, 19, 22)), ValueError,
     'convt2d_s2_bwd_weight_f32: dy / dy_gate (2, 16, 19, 23) expected, got (2, 16, 19, 23)',
     []),
    ('convt2d_s2_bwd_weight', dict(dy=T(2, 16, 19, 23, contiguous=False)), TypeError,
     'conv2d kernels take contiguous float32 tensors',
     ['require_cuda x dy dy_gate']),
    ('mse_window_norm', dict(y_hat=T(9, 11)), ValueError,
     'mse_window_norm_f32: y_hat [N, P, Q] and target [N, T, U] expected, got (9, 11) / (2, 12, 14)',
     []),
    ('mse_window_norm', dict(target=T(1, 12, 14, dtype=i16)), ValueError,
     'mse_window_norm_f32: y_hat [N, P, Q] and target [N, T, U] expected, got (2, 9, 11) / (1, 12, 14)',
     []),
    ('mse_window_norm', dict(y_hat=T(2, 9, 11, contiguous=False)), TypeError,
     'conv2d kernels take contiguous float32 tensors',
     ['require_cuda y_hat target']),
    ('mse_window_norm', dict(target=T(2, 12, 14, dtype=f64)), TypeError,
     'mse_window_norm_f32: counts must be contiguous int16 or float32 tensors, got torch.float64',
     ['require_cuda y_hat target']),
]


WRAPPERS = sorted({fn for fn, _, _ in CASES.values()})


def test_the_tables_cover_all_34_wrappers():
    assert len(WRAPPERS) == 34 and all(callable(getattr(K, fn)) for fn in WRAPPERS)
    assert set(EXPECTED) == set(CASES)
    with_errors = {CASES[cid][0] for cid, *_ in ERRORS}
    assert with_errors == set(WRAPPERS)


@pytest.mark.parametrize("cid", list(CASES))
def test_wrapper_calls_results_and_workspace_keys(monkeypatch, cid):
    fn, args, answers = CASES[cid]
    saved = K._workspaces
    events, results, keys, error = run(monkeypatch, fn, args, answers)
    monkeypatch.undo()
    assert K._workspaces is saved
    assert error is None
    assert (events, results, keys) == EXPECTED[cid]


@pytest.mark.parametrize("row", range(len(ERRORS)), ids=lambda i: f"{ERRORS[i][0]}-{i}")
def test_argument_errors_type_text_and_order(monkeypatch, row):
    cid, replaced, exc_type, message, before = ERRORS[row]
    fn, args, answers = CASES[cid]
    events, _, keys, error = run(monkeypatch, fn, {**args, **replaced}, answers)
    assert type(error) is exc_type and str(error) == message
    assert events == before and keys == []                      # nothing reached the C ABI, no workspace was made


def test_declared_parameter_counts_match_the_bound_argtypes():
    """Every function include/pv_yield_hip.h declares is bound with as many argtypes as it has parameters."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    declared = {}
    for name, params in re.findall(r"\b(pv_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        params = params.strip()
        declared[name] = 0 if params in ("", "void") else params.count(",") + 1
    assert set(declared) == set(_lib.SIGNATURES)
    mismatched = {n: (declared[n], len(_lib.SIGNATURES[n])) for n in declared if declared[n] != len(_lib.SIGNATURES[n])}
    assert not mismatched
