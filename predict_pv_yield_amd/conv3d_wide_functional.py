"""torch.autograd.Function wrappers over the exact-f32 (2, 3, 3) Conv3d kernels of csrc/conv3d_wide_f32.hip and
csrc/conv3d_s2_f32.hip.

Reference operators replaced: notebooks/12_just_3d_conv.ipynb (raw lines of the .ipynb file)
    self.conv(cat(hist_images.unsqueeze(1), forecast horizon broadcast as a second channel)): nn.Sequential of Conv3d 2 -> 64
    -> 128 -> 128 -> 128 (kernel (2, 3, 3), padding (0 | 1, 1, 1)) and Conv3d 128 -> 1 (stride (1, 2, 2)), ReLU between :1397-1420
notebooks/08_multiple_historical_images_as_separate_channels.ipynb (raw lines of the .ipynb file)
    self.encoder_conv(hist_images.unsqueeze(1)): Conv3d 1 -> 8 -> 32 -> 32, kernel (2, 3, 3), stride (1, 2, 2), a ReLU after
    each                                                                                                       :1365-1372, 1383-1385
    self.decoder_conv(cat(encoder_out, forecast horizon plane)): ConvTranspose2d 33 -> 32 -> 32 stride 2 with ReLU,
    ConvTranspose2d 32 -> 1                                                                                    :1374-1380, 1388-1392

Gating follows conv2d_functional, whose ConvReLU only hands tensors to its family's three entry points and so serves NCDHW
tensors unchanged; the chain builders list their layers for conv_chain, which derives both flags from position.  They are
fixed when the chain is built: no tensor is handed from one backward node to another here, so there is nothing to keep in a
_backward_pass.PassTable.
"""
from functools import partial

import torch

from . import hip_ops as K
from .conv2d_functional import CONVT2D_HEAD_OPS, CONVT2D_S2_OPS, ConvReLU, SynthConvReLU, conv_chain

# (forward, data gradient, weight gradient) of the wide family, one tuple per depth padding, and of the depth-2 head
CONV3D_WIDE_OPS = {pd: (partial(K.conv3d_wide_fwd_f32, padding=(pd, 1, 1)),
                        partial(K.conv3d_wide_bwd_data_f32, padding=(pd, 1, 1)),
                        partial(K.conv3d_wide_bwd_weight_f32, padding=(pd, 1, 1))) for pd in (0, 1)}
CONV3D_HEAD_D2_OPS = (K.conv3d_head_d2_fwd_f32, K.conv3d_head_d2_bwd_data_f32, K.conv3d_head_d2_bwd_weight_f32)
# notebook 08: the strided depth-2 Conv3d layers
CONV3D_S2_OPS = (K.conv3d_s2_fwd_f32, K.conv3d_s2_bwd_data_f32, K.conv3d_s2_bwd_weight_f32)
# (forward, weight gradient) of notebook 12's first layer, whose second input channel is the forecast horizon
HORIZON_WIDE_OPS = (K.conv3d_wide_horizon_fwd_f32, K.conv3d_wide_horizon_bwd_weight_f32)


def horizon_conv_relu(history, horizon, weight, bias):
    """relu(conv.0(cat(history.unsqueeze(1), horizon channel))) of 12_just_3d_conv.ipynb:1398-1399, 1413-1418; gradients to
    weight and bias only."""
    return SynthConvReLU.apply(HORIZON_WIDE_OPS, (history, horizon), weight, bias, {}, False)


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
    nn.Sequential (modules 0, 2, 4, 6, 8 nn.Conv3d).  history [N, 4, H, W], horizon [N] f32 -> [N, 1, 1, (H - 1) // 2 + 1,
    (W - 1) // 2 + 1]."""
    return conv_chain(None, [(HORIZON_WIDE_OPS, conv[0], (history, horizon)), (CONV3D_WIDE_OPS[0], conv[2]),
                             (CONV3D_WIDE_OPS[1], conv[4]), (CONV3D_WIDE_OPS[0], conv[6]), (CONV3D_HEAD_D2_OPS, conv[8])],
                      last_relu=False)


class HorizonConvTransposeReLU(torch.autograd.Function):
    """First decoder layer of notebook 08: nn.ConvTranspose2d(33, 32, 3, stride=2) (+ ReLU) on x [N, 32, H, W] f32 plus the
    forecast horizon [N] as a 33rd input channel, constant over the image, built inside the kernels (forward and weight
    gradient), never stored.  The horizon has no gradient; the 32 real channels' data gradient is the plain stride-2
    ConvTranspose2d's on the first 32 rows of the weight (contiguous, so a view)."""

    @staticmethod
    def forward(ctx, x, horizon, weight, bias, x_is_relu_output, dy_pregated):
        x, horizon = x.contiguous(), horizon.contiguous()
        y = K.convt2d_s2_horizon_fwd_f32(x, horizon, weight.contiguous(), bias.contiguous(), True)
        ctx.save_for_backward(x, horizon, weight, None if dy_pregated else y)
        ctx.x_is_relu_output = x_is_relu_output
        return y

    @staticmethod
    def backward(ctx, dy):
        x, horizon, weight, y = ctx.saved_tensors
        dy, weight = dy.contiguous(), weight.contiguous()
        dx = None
        if ctx.needs_input_grad[0]:
            dx = K.convt2d_s2_bwd_data_f32(dy, y, weight[:K.CONVT_HORIZON_C], x if ctx.x_is_relu_output else None,
                                           tuple(x.shape))
        dw, db = K.convt2d_s2_horizon_bwd_weight_f32(x, horizon, dy, y, tuple(weight.shape))
        return dx, None, dw, db, None, None


def conv3d_s2_relu(x, weight, bias, relu=True, x_is_relu_output=False):
    """nn.Conv3d(C_in, C_out, (2, 3, 3), stride=(1, 2, 2))(x) (+ ReLU) for (C_in, C_out) = (1, 8), (8, 32), (32, 32), planes up
    to 128 wide.  x_is_relu_output: dx leaves gated by x > 0."""
    return ConvReLU.apply(CONV3D_S2_OPS, x, weight, bias, bool(relu), bool(x_is_relu_output), False)


def horizon_conv_transpose_relu(x, horizon, weight, bias, x_is_relu_output=False):
    """relu(decoder_conv.0(cat(x, horizon plane))) of 08_...ipynb:1375-1376, 1388-1391; no gradient to the horizon."""
    return HorizonConvTransposeReLU.apply(x, horizon, weight, bias, bool(x_is_relu_output), False)


def nb08_hist_depth_f32(history, horizon, encoder_conv, decoder_conv):
    """self.decoder_conv(cat(self.encoder_conv(hist_images.unsqueeze(1)) without its depth axis, horizon plane)) of
    08_...ipynb:1382-1392; encoder_conv / decoder_conv = the notebook's two nn.Sequential (modules 0, 2, 4 nn.Conv3d /
    nn.ConvTranspose2d).  history [N, 4, H, W], horizon [N] f32 -> [N, 1, 4 e + 5, 4 f + 5] for an encoder output of e x f.
    Depth 4 -> 3 -> 2 -> 1; dropping the depth axis of size 1 and adding the one of the input are views."""
    enc, dec = encoder_conv, decoder_conv
    return conv_chain(history.unsqueeze(1), [(CONV3D_S2_OPS, enc[0]), (CONV3D_S2_OPS, enc[2]), (CONV3D_S2_OPS, enc[4]),
                                             lambda y: y.squeeze(2), (HorizonConvTransposeReLU, dec[0], (horizon,)),
                                             (CONVT2D_S2_OPS, dec[2]), (CONVT2D_HEAD_OPS, dec[4])], last_relu=False)
