"""torch.autograd.Function wrappers over the 144-channel Conv2d 3x3 "valid" kernels with fused MaxPool2d(3)
(csrc/conv2d_pool_f32.hip), exact f32.

Reference operators replaced (experiments/001_CNN_concat_all_timesteps_as_channels.py):
  self.maxpool(F.relu(self.sat_conv1(torch.cat((frames, center_marker, x_coords, y_coords, pixel_x, pixel_y), dim=1))))
                                                                                                      :264-307
  self.maxpool(F.relu(self.sat_conv2(out)))                                                           :308-309
  F.relu(self.sat_conv3(out))                                                                         :310
The pooled layers return relu(max_pool2d(z, 3)) (equal to max_pool2d(relu(z), 3)) and keep one byte per pooled output: the
winning window position, or "dead" where the maximum is <= 0.  Their backward expands the pooled gradient through those
codes, which carry the ReLU gate as well (a dead window passes nothing), so no gradient arriving at a pooled layer needs
gating, and conv2d_functional's pre-gated pairing (dy_pregated) has no use here: the one ReLU output without a pool, conv3's,
goes to fc1, whose data gradient is not gated, so conv3 gates its own dy by its output.
x_is_relu_output -> this layer's dx leaves zeroed where x <= 0.  Above a pooled layer that gate equals the codes' (the pooled
output is 0 exactly where its window is dead), so sat_encoder001_f32 leaves it off.
"""
import torch

from . import hip_ops as K


class SatConvPool(torch.autograd.Function):
    """First layer: sat [B, T, H, W, 1], frames 0..n_frames-1 stacked as channels plus five synthesised channels, built
    inside the kernels (forward and weight gradient), never stored.  No gradient flows to the inputs."""

    @staticmethod
    def forward(ctx, sat, x_coords, y_coords, weight, bias, n_frames):
        sat, x_coords, y_coords = sat.contiguous(), x_coords.contiguous(), y_coords.contiguous()
        y, codes = K.conv2d144_sat_pool_fwd_f32(sat, x_coords, y_coords, weight.contiguous(), bias.contiguous(), n_frames)
        ctx.save_for_backward(sat, x_coords, y_coords, codes)
        ctx.n_frames = n_frames
        return y

    @staticmethod
    def backward(ctx, dy):
        sat, x_coords, y_coords, codes = ctx.saved_tensors
        dw, db = K.conv2d144_sat_pool_bwd_weight_f32(sat, x_coords, y_coords, dy.contiguous(), codes, ctx.n_frames)
        return None, None, None, dw, db, None


class ConvPool(torch.autograd.Function):
    """relu(max_pool2d(nn.Conv2d(144, 144, 3)(x), 3)) on NCHW f32."""

    @staticmethod
    def forward(ctx, x, weight, bias, x_is_relu_output):
        x = x.contiguous()
        y, codes = K.conv2d144_pool_fwd_f32(x, weight.contiguous(), bias.contiguous())
        ctx.save_for_backward(x, weight, codes)
        ctx.x_is_relu_output = x_is_relu_output
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, codes = ctx.saved_tensors
        dy, weight = dy.contiguous(), weight.contiguous()
        dx = None
        if ctx.needs_input_grad[0]:
            dx = K.conv2d144_pool_bwd_data_f32(dy, codes, weight, x if ctx.x_is_relu_output else None, tuple(x.shape))
        dw, db = K.conv2d144_pool_bwd_weight_f32(x, dy, codes, tuple(weight.shape))
        return dx, dw, db, None


class Conv144ReLU(torch.autograd.Function):
    """nn.Conv2d(144, 144, 3) (+ ReLU) on NCHW f32."""

    @staticmethod
    def forward(ctx, x, weight, bias, relu, x_is_relu_output):
        x = x.contiguous()
        y = K.conv2d144_fwd_f32(x, weight.contiguous(), bias.contiguous() if bias is not None else None, relu)
        ctx.save_for_backward(x, weight, y if relu else None)
        ctx.has_bias, ctx.x_is_relu_output = bias is not None, x_is_relu_output
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight, y = ctx.saved_tensors
        dy, weight = dy.contiguous(), weight.contiguous()
        dx = None
        if ctx.needs_input_grad[0]:
            dx = K.conv2d144_bwd_data_f32(dy, y, weight, x if ctx.x_is_relu_output else None, tuple(x.shape))
        dw, db = K.conv2d144_bwd_weight_f32(x, dy, y, tuple(weight.shape))
        return dx, dw, (db if ctx.has_bias else None), None, None


def sat_conv_pool_f32(sat, x_coords, y_coords, weight, bias, n_frames):
    """maxpool(relu(sat_conv1(stacked frames + 5 channels))) of experiments/001...py:264-307; gradients to weight and bias
    only."""
    return SatConvPool.apply(sat, x_coords, y_coords, weight, bias, int(n_frames))


def conv_pool_f32(x, weight, bias, x_is_relu_output=False):
    """maxpool(relu(nn.Conv2d(144, 144, 3)(x))).  x_is_relu_output: dx leaves gated by x > 0."""
    return ConvPool.apply(x, weight, bias, bool(x_is_relu_output))


def conv144_relu(x, weight, bias, relu=True, x_is_relu_output=False):
    """nn.Conv2d(144, 144, 3)(x) (+ ReLU).  x_is_relu_output: dx leaves gated by x > 0."""
    return Conv144ReLU.apply(x, weight, bias, bool(relu), bool(x_is_relu_output))


def sat_encoder001_f32(sat, x_coords, y_coords, conv1, conv2, conv3, n_frames):
    """relu(conv3(pool(relu(conv2(pool(relu(conv1(stacked input)))))))) of experiments/001...py:264-310; conv1..3 are
    nn.Conv2d.  [B, 144, 11, 11] at 128 x 128.  conv2 and conv3 read pooled outputs, whose layers route the gradient through
    their codes, so their dx is not gated again."""
    y1 = SatConvPool.apply(sat, x_coords, y_coords, conv1.weight, conv1.bias, int(n_frames))
    y2 = ConvPool.apply(y1, conv2.weight, conv2.bias, False)
    return Conv144ReLU.apply(y2, conv3.weight, conv3.bias, True, False)
