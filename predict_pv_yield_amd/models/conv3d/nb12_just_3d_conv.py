"""LitAutoEncoder of the depth-2 Conv3d frame predictor -- host-side mirror of notebooks/12_just_3d_conv.ipynb (the cell that
defines LitAutoEncoder with CHANNELS = 128, N_HIST_IMAGES = 4, KERNEL = (2, 3, 3), raw lines 1388-1440 of the .ipynb file; the
five nn.Conv3d at 1398-1406).

  input  x[HISTORICAL_SAT_IMAGES]  [B, 4, H, W]   float32, normalised by the loader (H = W = 128 in the notebook)
         x[FORECAST_HORIZON]       [B]            float32, normalise_forecast_horizon(timesteps): (h - mean) / std of
                                                  arange(1, 25) (12_just_3d_conv.ipynb:757-768)
         x[TARGET_SAT_IMAGE]       [B, h_t, w_t]  float32, normalised; (h_t, w_t) == the output's sides (H = 128: 64)
  graph  the four history frames are the depth axis of one input channel; a second channel carries the horizon, constant over
         depth and the image: [B, 2, 4, H, W];
         self.conv = Sequential(Conv3d 2 -> 64 padding (0, 1, 1), ReLU, Conv3d 64 -> 128 padding (0, 1, 1), ReLU, Conv3d 128 ->
         128 padding (1, 1, 1), ReLU, Conv3d 128 -> 128 padding (0, 1, 1), ReLU, Conv3d 128 -> 1 stride (1, 2, 2) padding
         (0, 1, 1)), all with kernel (2, 3, 3): depth 4 -> 3 -> 2 -> 3 -> 2 -> 1, a side s stays s until the last layer makes
         it (s - 1) // 2 + 1 (128 -> 64)
  loss   F.mse_loss(y_hat.squeeze(), target), no crop, no re-normalisation; Adam(lr=1e-4)

Same attribute / state_dict names as the notebook (conv.0.weight ... conv.8.bias; 742 337 parameters).  self.conv is a
parameter holder: every layer, the loss and the optimiser run on the gfx950 kernels behind include/pv_yield_hip.h
(pv_conv3d_wide_*, pv_conv2d_head_s2p1_*, pv_mse_loss_f32, pv_adam_step_f32).  The two-channel input is never stored: the first
layer's kernels read the horizon of each example from device memory, so a step can be captured as a graph.  Deliberate
differences from the notebook: it runs on the MI355X only (CPU tensors raise a RuntimeError); a target whose sides are not the
output's raises a ValueError where torch would broadcast; and y_hat keeps its batch axis at B = 1 (the notebook's squeeze()
drops it, which F.mse_loss then broadcasts back).
"""
import torch
from torch import nn

from .._notebook_ae import NotebookAutoEncoder
from .._notebook_ae import check_target_side as _check_target_side
from .flow_autoencoder import FORECAST_HORIZON, HISTORICAL_SAT_IMAGES, TARGET_SAT_IMAGE  # noqa: F401

STRIDE = 1
CHANNELS = 128
N_HIST_IMAGES = 4
KERNEL = (2, 3, 3)  # depth (timestep), height, width


def output_side(image_side: int) -> int:
    """Side of y_hat for an input side (128 -> 64, 47 -> 24, 1 -> 1)."""
    if image_side < 1:
        raise ValueError(f"nb12 LitAutoEncoder needs images of at least 1 x 1 pixel, got {image_side}")
    return (image_side + 2 * 1 - 3) // 2 + 1      # conv.0 - conv.6 keep the side (padding 1); conv.8: stride 2, padding 1


def check_target_side(image_shape, target_shape) -> None:
    """image_shape: (H, W) of the history images; the target must be [B, output_side(H), output_side(W)]."""
    _check_target_side("nb12", output_side, image_shape, target_shape)


class LitAutoEncoder(NotebookAutoEncoder):
    name = "nb12_just_3d_conv"
    nb = "nb12"
    output_side, check_target_side = staticmethod(output_side), staticmethod(check_target_side)

    def __init__(self, lr: float = 0.0001):
        super().__init__()
        self.lr = float(lr)

        self.conv = nn.Sequential(
            nn.Conv3d(in_channels=2, out_channels=CHANNELS // 2, kernel_size=KERNEL, padding=(0, 1, 1)),
            nn.ReLU(),
            nn.Conv3d(in_channels=CHANNELS // 2, out_channels=CHANNELS, kernel_size=KERNEL, padding=(0, 1, 1)),
            nn.ReLU(),
            nn.Conv3d(in_channels=CHANNELS, out_channels=CHANNELS, kernel_size=KERNEL, padding=(1, 1, 1)),
            nn.ReLU(),
            nn.Conv3d(in_channels=CHANNELS, out_channels=CHANNELS, kernel_size=KERNEL, padding=(0, 1, 1)),
            nn.ReLU(),
            nn.Conv3d(in_channels=CHANNELS, out_channels=1, kernel_size=KERNEL, stride=(1, 2, 2), padding=(0, 1, 1)),
        )

    def forward(self, x):
        from ...conv3d_wide_functional import nb12_just_3d_conv_f32
        # the horizon channel is synthesised by the first layer's kernels from one value per example
        return nb12_just_3d_conv_f32(*self.history_and_horizon(x, torch.float32), self.conv)

    def loss(self, y_hat, y):
        from ...functional import mse_loss
        return mse_loss(y_hat.reshape(y.shape), y.to(device=y_hat.device, dtype=torch.float32))
