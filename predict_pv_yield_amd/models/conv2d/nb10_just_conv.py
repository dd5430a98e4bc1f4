"""LitAutoEncoder of the plain Conv2d frame predictor -- host-side mirror of notebooks/10_just_conv.ipynb (the cell that
defines LitAutoEncoder with CHANNELS = 128, N_HIST_IMAGES = 4, STRIPE_WIDTH = 128 // 24, raw lines 1374-1436 of the .ipynb
file; the four nn.Conv2d at 1386-1392).

  input  x[HISTORICAL_SAT_IMAGES]  [B, 4, H, W]   float32, normalised by the loader (H = W = 128 in the notebook)
         x[FORECAST_HORIZON]       [B]            timesteps ahead, 1..23 (int64 in the notebook; any integer or float dtype)
         x[TARGET_SAT_IMAGE]       [B, h_t, w_t]  float32, normalised; (h_t, w_t) == the output's sides (H = 128: 64)
  graph  a fifth input plane carries the horizon as a MetNet-style stripe: start = int(horizon * 5), 1.0 on columns start <=
         c < start + 5, else 0 (STRIPE_WIDTH = 5 is a constant, not derived from W; columns at or beyond W do not exist, so
         start >= W gives an all-zero plane);
         self.conv = Sequential(Conv2d 5 -> 64, ReLU, Conv2d 64 -> 128, ReLU, Conv2d 128 -> 128 padding 2, ReLU,
         Conv2d 128 -> 1 stride 2 padding 2): a side s becomes s - 2, s - 4, s - 2, (s - 1) // 2 + 1 (128 -> 64)
  loss   F.mse_loss(y_hat, target.unsqueeze(1)), no crop, no re-normalisation; Adam(lr=1e-3)

Same attribute / state_dict names as the notebook (conv.0.weight ... conv.6.bias; 225 537 parameters).  self.conv is a
parameter holder: every layer, the loss and the optimiser run on the gfx950 kernels behind include/pv_yield_hip.h
(pv_conv2d_wide_*, pv_conv2d_head_s2_*, pv_mse_loss_f32, pv_adam_step_f32).  The stripe plane is never stored: the first
layer's kernels synthesise it from one int32 start column per example, which torch computes on the device as
(horizon * 5).trunc() -- the notebook's per-example int(...) forces a host synchronisation per example, which is not
reproduced, so a step can be captured as a graph.  Deliberate differences from the notebook: it runs on the MI355X only
(CPU tensors raise a RuntimeError); a target whose sides are not the output's raises a ValueError where torch would
broadcast; and a negative horizon (outside the notebook's 1..23) follows the kernel rule start <= c < start + 5, 0 <= c <
W, where Python's negative slice indices would count from the right edge.
"""
import torch
from torch import nn

from .._notebook_ae import NotebookAutoEncoder
from .._notebook_ae import check_target_side as _check_target_side
from ..conv3d.flow_autoencoder import FORECAST_HORIZON, HISTORICAL_SAT_IMAGES, TARGET_SAT_IMAGE  # noqa: F401

STRIDE = 1
CHANNELS = 128
N_HIST_IMAGES = 4
STRIPE_WIDTH = 128 // 24      # input img size / num timesteps
MIN_IMAGE_SIDE = 5            # 5 -> 3 -> 1 -> 3 -> 2: the smallest side the two unpadded 3x3 convolutions accept


def output_side(image_side: int) -> int:
    """Side of y_hat for an input side (128 -> 64, 47 -> 24)."""
    if image_side < MIN_IMAGE_SIDE:
        raise ValueError(f"nb10 LitAutoEncoder needs images of at least {MIN_IMAGE_SIDE} x {MIN_IMAGE_SIDE} pixels (two "
                         f"unpadded 3x3 convolutions), got {image_side}")
    side = image_side - 2 - 2 + 2          # conv.0, conv.2 (padding 0), conv.4 (padding 2)
    return (side + 2 * 2 - 3) // 2 + 1      # conv.6: stride 2, padding 2


def check_target_side(image_shape, target_shape) -> None:
    """image_shape: (H, W) of the history images; the target must be [B, output_side(H), output_side(W)]."""
    _check_target_side("nb10", output_side, image_shape, target_shape)


class LitAutoEncoder(NotebookAutoEncoder):
    name = "nb10_just_conv"
    nb = "nb10"
    output_side, check_target_side = staticmethod(output_side), staticmethod(check_target_side)

    def __init__(self, lr: float = 0.001):
        super().__init__()
        self.lr = float(lr)

        self.conv = nn.Sequential(
            nn.Conv2d(in_channels=N_HIST_IMAGES + 1, out_channels=CHANNELS // 2, kernel_size=3, stride=1),
            nn.ReLU(),
            nn.Conv2d(in_channels=CHANNELS // 2, out_channels=CHANNELS, kernel_size=3, stride=1),
            nn.ReLU(),
            nn.Conv2d(in_channels=CHANNELS, out_channels=CHANNELS, kernel_size=3, stride=1, padding=2),
            nn.ReLU(),
            nn.Conv2d(in_channels=CHANNELS, out_channels=1, kernel_size=3, stride=2, padding=2),
        )

    def forward(self, x):
        from ...conv2d_functional import nb10_just_conv_f32, stripe_start_from_horizon
        hist_images, horizon = self.history_and_horizon(x)
        # the stripe plane is synthesised by the first layer's kernels from one start column per example
        stripe_start = stripe_start_from_horizon(horizon, STRIPE_WIDTH)
        return nb10_just_conv_f32(hist_images, stripe_start, self.conv)

    def loss(self, y_hat, y):
        from ...functional import mse_loss
        return mse_loss(y_hat, y.to(device=y_hat.device, dtype=torch.float32).unsqueeze(1))
