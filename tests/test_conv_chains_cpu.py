"""CPU: what each of the eight chain builders of conv2d_functional.py / conv3d_wide_functional.py hands to its autograd
Functions, without a GPU and without the library.  Every Function's apply is replaced by a recorder that returns its input
tensor; the recorded sequence is (Function, ops tuple by name, relu, x_is_relu_output, dy_pregated) per layer, None where a
Function has no such argument.  The table below was recorded from the builders while each still passed its gating flags as
positional booleans, before they were derived from a layer's position: it is the contract, so a change to the builders never
edits it.  A synthesised-input first layer is recorded as "first layer" with its (forward, weight gradient) pair and its
dy_pregated; which class carries it is not part of the table (the pairs of experiments/002's and notebook 12's first layers
had no name of their own when the table was recorded, and are named as they are now)."""
import types

import pytest
import torch

from predict_pv_yield_amd import conv2d_functional as C2
from predict_pv_yield_amd import conv3d_wide_functional as C3

FIRST = "first layer"

EXPECTED = {
    'sat_encoder_f32': [
        ('first layer', 'COORDS_OPS', True, None, True),
        ('ConvReLU', 'CONV2D_OPS', True, True, True),
        ('ConvReLU', 'CONV2D_OPS', True, True, False),
    ],
    'sat_encoder001_f32': [
        ('SatConvPool', None, True, None, None),
        ('ConvPool', 'CONV2D144_POOL_OPS', True, False, None),
        ('ConvReLU', 'CONV2D144_OPS', True, False, False),
    ],
    'nb16_autoencoder_f32': [
        ('first layer', 'COUNTS_AE_OPS', True, None, True),
        ('ConvReLU', 'CONV2D_AE_OPS', True, True, True),
        ('ConvReLU', 'CONV2D_AE_OPS', True, True, True),
        ('ConvPool', 'CONV2D_AE_POOL_OPS', True, True, None),
        ('ConvReLU', 'CONVT2D_AE_OPS', True, False, True),
        ('ConvReLU', 'CONVT2D_AE_OPS', True, True, True),
        ('ConvReLU', 'CONVT2D_AE_OPS', True, True, True),
        ('ConvReLU', 'CONVT2D_AE_OPS', False, True, False),
    ],
    'nb15_autoencoder_f32': [
        ('first layer', 'COUNTS_S2_OPS', True, None, True),
        ('ConvReLU', 'CONV2D_S2_OPS', True, True, True),
        ('ConvReLU', 'CONV2D_S2_OPS', True, True, True),
        ('ConvReLU', 'CONV2D_S2_OPS', True, True, True),
        ('ConvReLU', 'CONVT2D_S2_OPS', True, True, True),
        ('ConvReLU', 'CONVT2D_S2_OPS', True, True, True),
        ('ConvReLU', 'CONVT2D_S2_OPS', False, True, False),
    ],
    'nb10_just_conv_f32': [
        ('first layer', 'STRIPE_WIDE_OPS', True, None, True),
        ('ConvReLU', 'CONV2D_WIDE_OPS', True, True, True),
        ('ConvReLU', 'CONV2D_WIDE_P2_OPS', True, True, True),
        ('ConvReLU', 'CONV2D_HEAD_S2_OPS', False, True, False),
    ],
    'nb09_stripe_ae_f32': [
        ('first layer', 'STRIPE_WIDE_S2_OPS', True, None, True),
        ('ConvReLU', 'CONV2D_WIDE_S2_OPS', True, True, True),
        ('ConvReLU', 'CONV2D_WIDE_S2_OPS', True, True, True),
        ('ConvReLU', 'CONVT2D_WIDE_S2_OPS', True, True, True),
        ('ConvReLU', 'CONVT2D_WIDE_S2_OPS', True, True, True),
        ('ConvReLU', 'CONVT2D_HEAD_OPS', False, True, False),
    ],
    'nb12_just_3d_conv_f32': [
        ('first layer', 'HORIZON_WIDE_OPS', True, None, True),
        ('ConvReLU', 'CONV3D_WIDE_OPS[0]', True, True, True),
        ('ConvReLU', 'CONV3D_WIDE_OPS[1]', True, True, True),
        ('ConvReLU', 'CONV3D_WIDE_OPS[0]', True, True, True),
        ('ConvReLU', 'CONV3D_HEAD_D2_OPS', False, True, False),
    ],
    'nb08_hist_depth_f32': [
        ('ConvReLU', 'CONV3D_S2_OPS', True, False, True),
        ('ConvReLU', 'CONV3D_S2_OPS', True, True, True),
        ('ConvReLU', 'CONV3D_S2_OPS', True, True, True),
        ('HorizonConvTransposeReLU', None, True, True, True),
        ('ConvReLU', 'CONVT2D_S2_OPS', True, True, True),
        ('ConvReLU', 'CONVT2D_HEAD_OPS', False, True, False),
    ],
}


def ops_name(ops):
    """The name under which one of the two modules holds this very tuple (NAME[key] inside a dict of tuples)."""
    for mod in (C2, C3):
        for name, value in vars(mod).items():
            if not name.endswith("_OPS"):
                continue
            if value is ops:
                return name
            if isinstance(value, dict):
                for key, item in value.items():
                    if item is ops:
                        return f"{name}[{key}]"
    raise KeyError(ops)


class Modules:
    """Stands in for an nn.Sequential or a list of layers: item i has a weight and a bias, which no recorder looks at."""

    def __getitem__(self, i):
        return types.SimpleNamespace(weight=f"weight{i}", bias=f"bias{i}")


def builders():
    z = torch.zeros
    history, flow_pred, horizon, stripe_start = z(2, 4, 8, 8), z(2, 8, 8), z(2), z(2, dtype=torch.int32)
    m = Modules()
    return {
        "sat_encoder_f32": lambda: C2.sat_encoder_f32(z(6, 8, 8, 12), z(2, 8), z(2, 8), m[0], m[1], m[2], 3),
        "sat_encoder001_f32": lambda: C2.sat_encoder001_f32(z(2, 5, 8, 8, 1), z(2, 8), z(2, 8), m[0], m[1], m[2], 3),
        "nb16_autoencoder_f32": lambda: C2.nb16_autoencoder_f32(history, flow_pred, horizon, [m[i] for i in range(4)],
                                                                [m[i] for i in range(4)]),
        "nb15_autoencoder_f32": lambda: C2.nb15_autoencoder_f32(history, flow_pred, horizon, m),
        "nb10_just_conv_f32": lambda: C2.nb10_just_conv_f32(history, stripe_start, m),
        "nb09_stripe_ae_f32": lambda: C2.nb09_stripe_ae_f32(history, stripe_start, m, m),
        "nb12_just_3d_conv_f32": lambda: C3.nb12_just_3d_conv_f32(history, horizon, m),
        "nb08_hist_depth_f32": lambda: C3.nb08_hist_depth_f32(history, horizon, m, m),
    }


def test_the_table_names_every_chain_builder():
    assert set(EXPECTED) == set(builders())
    for name in EXPECTED:
        assert callable(getattr(C2, name, None) or getattr(C3, name))


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_builder_hands_its_functions_what_the_table_pins(monkeypatch, name):
    log = []

    def record(row, out):
        log.append(row)
        return out

    recorders = {
        C2.SynthConvReLU: lambda ops, inputs, w, b, scalars, dg: record((FIRST, ops_name(ops), True, None, dg), inputs[0]),
        C2.ConvReLU: lambda ops, x, w, b, relu, xg, dg: record(("ConvReLU", ops_name(ops), relu, xg, dg), x),
        C2.ConvPool: lambda ops, x, w, b, xg: record(("ConvPool", ops_name(ops), True, xg, None), x),
        C2.SatConvPool: lambda sat, xc, yc, w, b, n: record(("SatConvPool", None, True, None, None), sat),
        C3.HorizonConvTransposeReLU: lambda x, hz, w, b, xg, dg: record(("HorizonConvTransposeReLU", None, True, xg, dg), x),
    }
    for function, recorder in recorders.items():
        monkeypatch.setattr(function, "apply", staticmethod(recorder))
    builders()[name]()
    assert log == EXPECTED[name]
    for row in log:                                     # the flags are booleans as they stand, not merely truthy
        assert all(flag is None or type(flag) is bool for flag in row[2:])
