"""torch.autograd.Function wrappers over the exact-f32 (2, 3, 3) Conv3d kernels of csrc/conv3d_wide_f32.hip.

Reference operators replaced: notebooks/12_just_3d_conv.ipynb (raw lines of the .ipynb file)
    self.conv(cat(hist_images.unsqueeze(1), forecast horizon broadcast as a second channel)): nn.Sequential of Conv3d 2 -> 64
    -> 128 -> 128 -> 128 (kernel (2, 3, 3), padding (0 | 1, 1, 1)) and Conv3d 128 -> 1 (stride (1, 2, 2)), ReLU between :1397-1420

Gating follows conv2d_functional: ConvReLU (which only hands tensors to its family's three entry points, so it serves
NCDHW tensors unchanged) lets each data gradient leave gated by the layer's input (x_is_relu_output), and the layer below then
reads the arriving gradient without touching its own output (dy_pregated).  Both are flags fixed when the chain is built: no
tensor is handed from one backward node to another here, so there is nothing to keep in a _backward_pass.PassTable.
"""
from functools import partial

import torch

from . import hip_ops as K
from .conv2d_functional import ConvReLU

# (forward, data gradient, weight gradient) of the wide family, one tuple per depth padding, and of the depth-2 head
CONV3D_WIDE_OPS = {pd: (partial(K.conv3d_wide_fwd_f32, padding=(pd, 1, 1)),
                        partial(K.conv3d_wide_bwd_data_f32, padding=(pd, 1, 1)),
                        partial(K.conv3d_wide_bwd_weight_f32, padding=(pd, 1, 1))) for pd in (0, 1)}
CONV3D_HEAD_D2_OPS = (K.conv3d_head_d2_fwd_f32, K.conv3d_head_d2_bwd_data_f32, K.conv3d_head_d2_bwd_weight_f32)


class HorizonConvReLU(torch.autograd.Function):
    """First layer of notebook 12: history [N, D, H, W] f32 plus the forecast horizon [N] as a second input channel, constant
    over depth and the image, built inside the kernels (forward and weight gradient), never stored.  No gradient flows to the
    inputs."""

    @staticmethod
    def forward(ctx, history, horizon, weight, bias, dy_pregated):
        history, horizon = history.contiguous(), horizon.contiguous()
        y = K.conv3d_wide_horizon_fwd_f32(history, horizon, weight.contiguous(), bias.contiguous())
        ctx.save_for_backward(history, horizon, None if dy_pregated else y)
        ctx.weight_shape = tuple(weight.shape)
        return y

    @staticmethod
    def backward(ctx, dy):
        history, horizon, y = ctx.saved_tensors
        dy = dy.contiguous()
        if y is not None:
            dy = K.relu_gate_f32(dy, y)
        dw, db = K.conv3d_wide_horizon_bwd_weight_f32(history, horizon, dy, ctx.weight_shape)
        return None, None, dw, db, None


def horizon_conv_relu(history, horizon, weight, bias):
    """relu(conv.0(cat(history.unsqueeze(1), horizon channel))) of 12_just_3d_conv.ipynb:1398-1399, 1413-1418; gradients to
    weight and bias only."""
    return HorizonConvReLU.apply(history, horizon, weight, bias, False)


def conv3d_wide_relu(x, weight, bias, relu=True, x_is_relu_output=False, padding=(0, 1, 1)):
    """nn.Conv3d(64 or 128, 128, (2, 3, 3), padding=(0 or 1, 1, 1))(x) (+ ReLU), planes up to 128 wide.  x_is_relu_output: dx
    leaves gated by x > 0."""
    padding = tuple(int(p) for p in padding)
    if len(padding) != 3 or padding[0] not in CONV3D_WIDE_OPS or padding[1:] != (1, 1):
        raise ValueError(f"conv3d_wide: padding (0, 1, 1) or (1, 1, 1) expected, got {padding}")
    return ConvReLU.apply(CONV3D_WIDE_OPS[padding[0]], x, weight, bias, bool(relu), bool(x_is_relu_output), False)


def conv3d_head_d2(x, weight, bias, x_is_relu_output=False):
    """nn.Conv3d(C, 1, (2, 3, 3), stride=(1, 2, 2), padding=(0, 1, 1))(x) on an input of depth 2, no ReLU.
    x_is_relu_output: dx leaves gated by x > 0."""
    return ConvReLU.apply(CONV3D_HEAD_D2_OPS, x, weight, bias, False, bool(x_is_relu_output), False)


def nb12_just_3d_conv_f32(history, horizon, conv):
    """self.conv(cat(hist_images.unsqueeze(1), horizon channel)) of 12_just_3d_conv.ipynb:1397-1420; conv = the notebook's
    nn.Sequential (modules 0, 2, 4, 6, 8 nn.Conv3d; the nn.ReLU modules between them are fused into the layers' kernels).
    history [N, 4, H, W], horizon [N] f32 -> [N, 1, 1, (H - 1) // 2 + 1, (W - 1) // 2 + 1].  Every inner ReLU output has one
    consumer, the next layer, whose data gradient leaves gated by it (x_is_relu_output), so its producer skips gating the
    arriving gradient (dy_pregated): no ReLU or mask kernel runs on its own.  The pairing only holds inside this chain."""
    y = HorizonConvReLU.apply(history, horizon, conv[0].weight, conv[0].bias, True)
    y = ConvReLU.apply(CONV3D_WIDE_OPS[0], y, conv[2].weight, conv[2].bias, True, True, True)
    y = ConvReLU.apply(CONV3D_WIDE_OPS[1], y, conv[4].weight, conv[4].bias, True, True, True)
    y = ConvReLU.apply(CONV3D_WIDE_OPS[0], y, conv[6].weight, conv[6].bias, True, True, True)
    return ConvReLU.apply(CONV3D_HEAD_D2_OPS, y, conv[8].weight, conv[8].bias, False, True, False)
