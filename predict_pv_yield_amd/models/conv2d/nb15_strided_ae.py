"""LitAutoEncoder of the stride-2 notebooks -- host-side mirror of notebooks/15_int16.ipynb (the cell that defines
LitAutoEncoder with CHANNELS = 32, KERNEL = 3, STRIDE = 2, raw lines 13737-13802 of the .ipynb file, and
normalise_images_in_model at 13721-13728).  notebooks/14_back_to_2d_conv_AE.ipynb defines the same stack with Adam(lr=1e-4)
on images its loader has normalised already: lr is a constructor argument (configs/model/nb14_strided_ae.yaml), a
pre-normalised input mode is not built.

  input  x[HISTORICAL_SAT_IMAGES]     [B, 4, S, S]   raw 10-bit counts, int16 or float32 (S = 128 in the notebook)
         x[OPTICAL_FLOW_PREDICTIONS]  [B, S, S]      t0 image advected to the target time, raw counts
         x[FORECAST_HORIZON]          [B]            normalise_forecast_horizon(seconds); not normalised again
         x[TARGET_SAT_IMAGE]          [B, T, T]      raw counts; T == output side + 1 (S = 128: T = 64)
  graph  images = (cat(history, flow prediction).float() - 93.23458) / 115.34247; the horizon is a sixth plane;
         self.conv = Sequential(Conv2d 6 -> 16, ReLU, Conv2d 16 -> 32, ReLU, Conv2d 32 -> 32, ReLU, Conv2d 32 -> 32, ReLU,
         ConvTranspose2d 32 -> 32, ReLU, ConvTranspose2d 32 -> 16, ReLU, ConvTranspose2d 16 -> 1), all k3 s2 p0.  A Conv2d
         maps a side s to (s - 3) // 2 + 1, a ConvTranspose2d to 2 s + 1: S = 128 gives 63, 31, 15, 7, 15, 31, 63
  loss   F.mse_loss(y_hat.squeeze(), normalise(target)[..., :-1, :-1]); Adam(lr=1e-3)

Same attribute / state_dict names as the notebook (conv.0.weight ... conv.12.bias; 38 033 parameters).  self.conv is a
parameter holder: every layer, the loss and the optimiser run on the gfx950 kernels behind include/pv_yield_hip.h
(pv_conv2d_s2_*, pv_convt2d_s2_*, pv_mse_window_norm_f32, pv_adam_step_f32); the one torch kernel of a step scales the loss
gradient [B, P, P] by the root gradient, as functional.MSELossF32 does.  Deliberate differences from the notebook: it runs
on the MI355X only (CPU tensors raise a RuntimeError), and a target whose side is not the output side + 1 raises a
ValueError where torch would broadcast or fail later.
"""
from torch import nn

from .._notebook_ae import NotebookAutoEncoder
from .._notebook_ae import check_target_side as _check_target_side
from ..conv3d.flow_autoencoder import (FORECAST_HORIZON, HISTORICAL_SAT_IMAGES, OPTICAL_FLOW_PREDICTIONS,  # noqa: F401
                                       TARGET_SAT_IMAGE, normalise_forecast_horizon)

CHANNELS = 32
KERNEL = 3
STRIDE = 2
N_ENCODER = 4                 # stride-2 Conv2d layers
N_DECODER = 3                 # stride-2 ConvTranspose2d layers
SAT_IMAGE_MEAN = 93.23458
SAT_IMAGE_STD = 115.34247
MIN_IMAGE_SIDE = 31           # 31 -> 15 -> 7 -> 3 -> 1: the smallest side four k3 s2 convolutions accept


def output_side(image_side: int) -> int:
    """Side of y_hat for an S x S input (S = 128: 63)."""
    if image_side < MIN_IMAGE_SIDE:
        raise ValueError(f"nb15 LitAutoEncoder needs images of at least {MIN_IMAGE_SIDE} x {MIN_IMAGE_SIDE} pixels (four 3x3 "
                         f"stride-2 convolutions), got {image_side}")
    side = image_side
    for _ in range(N_ENCODER):
        side = (side - KERNEL) // STRIDE + 1
    for _ in range(N_DECODER):
        side = (side - 1) * STRIDE + KERNEL
    return side


def target_side(image_side: int) -> int:
    """Side of TARGET_SAT_IMAGE: y[..., :-1, :-1] must line up with the output (S = 128: 64)."""
    return output_side(image_side) + 1


def check_target_side(image_shape, target_shape) -> None:
    """image_shape: (H, W) of the history images; the target must be [B, target_side(H), target_side(W)]."""
    _check_target_side("nb15", target_side, image_shape, target_shape,
                       lambda want: f" (y[..., :-1, :-1] leaves the {want[0] - 1} x {want[1] - 1} output)")


class LitAutoEncoder(NotebookAutoEncoder):
    name = "nb15_strided_ae"
    nb = "nb15"
    output_side, check_target_side = staticmethod(output_side), staticmethod(check_target_side)

    def __init__(self, lr: float = 0.001):
        super().__init__()
        self.lr = float(lr)

        self.conv = nn.Sequential(
            # Encoder
            nn.Conv2d(in_channels=6, out_channels=CHANNELS // 2, kernel_size=KERNEL, stride=STRIDE),
            nn.ReLU(),
            nn.Conv2d(in_channels=CHANNELS // 2, out_channels=CHANNELS, kernel_size=KERNEL, stride=STRIDE),
            nn.ReLU(),
            nn.Conv2d(in_channels=CHANNELS, out_channels=CHANNELS, kernel_size=KERNEL, stride=STRIDE),
            nn.ReLU(),
            nn.Conv2d(in_channels=CHANNELS, out_channels=CHANNELS, kernel_size=KERNEL, stride=STRIDE),
            nn.ReLU(),

            # Decoder
            nn.ConvTranspose2d(in_channels=CHANNELS, out_channels=CHANNELS, kernel_size=KERNEL, stride=STRIDE),
            nn.ReLU(),
            nn.ConvTranspose2d(in_channels=CHANNELS, out_channels=CHANNELS // 2, kernel_size=KERNEL, stride=STRIDE),
            nn.ReLU(),
            nn.ConvTranspose2d(in_channels=CHANNELS // 2, out_channels=1, kernel_size=KERNEL, stride=STRIDE),
        )

    def forward(self, x):
        from ...conv2d_functional import nb15_autoencoder_f32
        return nb15_autoencoder_f32(*self.counts_and_horizon(x), self.conv)

    def loss(self, y_hat, y):
        from ...conv2d_functional import mse_window_norm
        # normalisation and y[..., :-1, :-1] happen inside the loss kernel: the window of the output's size at (0, 0)
        return mse_window_norm(y_hat.squeeze(1), self.counts(y), 0, 0)
