"""torch.autograd.Function wrappers over the Conv2d 3x3 "valid" kernels (csrc/conv2d_f32.hip), exact f32.

Reference operators replaced (experiments/002_cnn_processes_single_sat_image_then_rnn.py):
  F.relu(self.sat_conv1(torch.cat((sat_data, center_marker, x_coords, y_coords, pixel_x, pixel_y), dim=1)))   :180-209
  F.relu(self.sat_conv2(out)), F.relu(self.sat_conv3(out))                                                   :210-211
As in functional.Conv3dGeneralF32, the ReLU gating of an activation gradient is moved into the kernel that produces it:
x_is_relu_output -> this layer's dx leaves already zeroed where x <= 0 (the lower layer's pre-activation gradient);
dy_pregated -> the incoming dy was gated that way by the next layer, so backward reads it without touching y again
(set only inside sat_encoder_f32, where that pairing holds by construction).
"""
import torch

from . import hip_ops as K


class CoordsConv2dReLU(torch.autograd.Function):
    """First layer: sat [N, H, W, 12] channels-last, x_coords [N / t, W], y_coords [N / t, H]; the 17-channel input is
    synthesised inside the kernels (forward and weight gradient), never stored.  No gradient flows to the inputs."""

    @staticmethod
    def forward(ctx, sat, x_coords, y_coords, weight, bias, t_per_example, dy_pregated):
        sat, x_coords, y_coords = sat.contiguous(), x_coords.contiguous(), y_coords.contiguous()
        y = K.conv2d_coords_fwd_f32(sat, x_coords, y_coords, weight.contiguous(), bias.contiguous(), t_per_example)
        ctx.save_for_backward(sat, x_coords, y_coords, None if dy_pregated else y)
        ctx.t_per_example, ctx.weight_shape = t_per_example, tuple(weight.shape)
        return y

    @staticmethod
    def backward(ctx, dy):
        sat, x_coords, y_coords, y = ctx.saved_tensors
        dy = dy.contiguous()
        if y is not None:
            dy = K.relu_gate_f32(dy, y)
        dw, db = K.conv2d_coords_bwd_weight_f32(sat, x_coords, y_coords, dy, ctx.t_per_example, ctx.weight_shape)
        return None, None, None, dw, db, None, None


class Conv2dReLU(torch.autograd.Function):
    """nn.Conv2d(32, C_out in {32, 4}, 3) (+ ReLU) on NCHW f32."""

    @staticmethod
    def forward(ctx, x, weight, bias, relu, x_is_relu_output, dy_pregated):
        x = x.contiguous()
        y = K.conv2d_fwd_f32(x, weight.contiguous(), bias.contiguous() if bias is not None else None, relu)
        ctx.save_for_backward(x, weight, y if (relu and not dy_pregated) else None)
        ctx.has_bias, ctx.x_is_relu_output = bias is not None, x_is_relu_output
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, y = ctx.saved_tensors
        dy = dy.contiguous()
        weight = weight.contiguous()
        dx = None
        if ctx.needs_input_grad[0]:
            dx = K.conv2d_bwd_data_f32(dy, y, weight, x if ctx.x_is_relu_output else None, tuple(x.shape))
        dw, db = K.conv2d_bwd_weight_f32(x, dy, y, tuple(weight.shape))
        return dx, dw, (db if ctx.has_bias else None), None, None, None


def coords_conv2d_relu(sat, x_coords, y_coords, weight, bias, t_per_example):
    """relu(sat_conv1(17-channel input of experiments/002...py:180-208)); gradients to weight and bias only."""
    return CoordsConv2dReLU.apply(sat, x_coords, y_coords, weight, bias, int(t_per_example), False)


def conv2d_relu(x, weight, bias, relu=True, x_is_relu_output=False):
    """nn.Conv2d(32, C_out, 3)(x) (+ ReLU).  x_is_relu_output: x is a ReLU output, so dx may leave gated by x > 0 (the lower
    layer's pre-activation gradient; the ReLU's own backward would zero those entries anyway)."""
    return Conv2dReLU.apply(x, weight, bias, bool(relu), bool(x_is_relu_output), False)


def sat_encoder_f32(sat, x_coords, y_coords, conv1, conv2, conv3, t_per_example):
    """relu(conv3(relu(conv2(relu(conv1(17-channel input)))))) of experiments/002...py:180-211; conv1..3 are nn.Conv2d.
    The two inner activations have exactly one consumer each, the next layer's conv, whose data gradient leaves gated by
    them (x_is_relu_output): so their producers skip gating the arriving gradient again (dy_pregated).  That pairing is
    only valid inside this chain, which is why the flag is not offered by coords_conv2d_relu / conv2d_relu."""
    y1 = CoordsConv2dReLU.apply(sat, x_coords, y_coords, conv1.weight, conv1.bias, int(t_per_example), True)
    y2 = Conv2dReLU.apply(y1, conv2.weight, conv2.bias, True, True, True)
    return Conv2dReLU.apply(y2, conv3.weight, conv3.bias, True, True, False)
