"""LitAutoEncoder of the last notebook of the series -- host-side mirror of notebooks/16_maxpool.ipynb (the cell that defines
LitAutoEncoder, raw lines 13737-13830 of the .ipynb file, and normalise_images_in_model at 13721-13728).

  input  x[HISTORICAL_SAT_IMAGES]     [B, 4, S, S]   raw 10-bit counts, int16 or float32 (S = 128 in the notebook)
         x[OPTICAL_FLOW_PREDICTIONS]  [B, S, S]      t0 image advected to the target time, raw counts
         x[FORECAST_HORIZON]          [B]            normalise_forecast_horizon(seconds); not normalised again
         x[TARGET_SAT_IMAGE]          [B, T, T]      raw counts; T - 16 == (S - 8) // 3 + 8 (S = 128: T = 64)
  graph  images = (cat(history, flow prediction).float() - 93.23458) / 115.34247; the horizon is a sixth plane;
         Conv2d 6 -> 16 -> 32 -> 32 -> 32 (k3, ReLU), MaxPool2d(3) (whole windows), ConvTranspose2d 32 -> 32 -> 16 -> 16 (k3,
         ReLU) -> 1: [B, 1, P + 8, P + 8] with P = (S - 8) // 3
  loss   F.mse_loss(y_hat.squeeze(), normalise(target)[..., 8:-8, 8:-8]); Adam(lr=1e-3)

Same attribute / state_dict names as the notebook (encoder_conv1..4, decoder_conv1..4; maxpool and maxunpool exist without
parameters, the unpool is never called).  nn.Conv2d / nn.ConvTranspose2d are parameter holders: every layer, the loss and
the optimiser run on the gfx950 kernels behind include/pv_yield_hip.h (pv_conv2d_ae_*, pv_convt2d_ae_*,
pv_mse_crop_norm_f32, pv_adam_step_f32); the one torch kernel of a step scales the loss gradient [B, P + 8, P + 8] by the
root gradient, as functional.MSELossF32 does.  Deliberate differences from the notebook: it runs on the MI355X only (CPU tensors
raise a RuntimeError), and a target whose side does not line up with the output raises a ValueError where torch would
broadcast a 1 x 1 crop silently.
"""
from torch import nn

from .._notebook_ae import NotebookAutoEncoder
from .._notebook_ae import check_target_side as _check_target_side
from ..conv3d.flow_autoencoder import (FORECAST_HORIZON, HISTORICAL_SAT_IMAGES, OPTICAL_FLOW_PREDICTIONS,  # noqa: F401
                                       TARGET_SAT_IMAGE, normalise_forecast_horizon)

CHANNELS = 32
KERNEL = 3
CROP = 8                      # y[..., 8:-8, 8:-8]
SAT_IMAGE_MEAN = 93.23458
SAT_IMAGE_STD = 115.34247
MIN_IMAGE_SIDE = 4 * (KERNEL - 1) + KERNEL   # four valid 3x3 convs, then one whole pool window: 11


def output_side(image_side: int) -> int:
    """Side of y_hat for an S x S input: (S - 8) // 3 + 8 (S = 128: 48)."""
    if image_side < MIN_IMAGE_SIDE:
        raise ValueError(f"nb16 LitAutoEncoder needs images of at least {MIN_IMAGE_SIDE} x {MIN_IMAGE_SIDE} pixels (four 3x3 "
                         f"convolutions, then one whole 3x3 pool window), got {image_side}")
    return (image_side - 4 * (KERNEL - 1)) // KERNEL + 4 * (KERNEL - 1)


def target_side(image_side: int) -> int:
    """Side of TARGET_SAT_IMAGE that lines up with the output after the 8-pixel crop (S = 128: 64)."""
    return output_side(image_side) + 2 * CROP


def check_target_side(image_shape, target_shape) -> None:
    """image_shape: (H, W) of the history images; the target must be [B, target_side(H), target_side(W)]."""
    _check_target_side("nb16", target_side, image_shape, target_shape,
                       lambda want: f" (the {CROP}-pixel crop leaves the {want[0] - 2 * CROP} x {want[1] - 2 * CROP} output)")


class LitAutoEncoder(NotebookAutoEncoder):
    name = "nb16_maxpool_ae"
    nb = "nb16"
    output_side, check_target_side = staticmethod(output_side), staticmethod(check_target_side)

    def __init__(self):
        super().__init__()

        self.encoder_conv1 = nn.Conv2d(in_channels=6, out_channels=CHANNELS // 2, kernel_size=KERNEL)
        self.encoder_conv2 = nn.Conv2d(in_channels=CHANNELS // 2, out_channels=CHANNELS, kernel_size=KERNEL)
        self.encoder_conv3 = nn.Conv2d(in_channels=CHANNELS, out_channels=CHANNELS, kernel_size=KERNEL)
        self.encoder_conv4 = nn.Conv2d(in_channels=CHANNELS, out_channels=CHANNELS, kernel_size=KERNEL)

        self.maxpool = nn.MaxPool2d(kernel_size=KERNEL, return_indices=True)
        self.maxunpool = nn.MaxUnpool2d(kernel_size=KERNEL)

        self.decoder_conv1 = nn.ConvTranspose2d(in_channels=CHANNELS, out_channels=CHANNELS, kernel_size=KERNEL)
        self.decoder_conv2 = nn.ConvTranspose2d(in_channels=CHANNELS, out_channels=CHANNELS // 2, kernel_size=KERNEL)
        self.decoder_conv3 = nn.ConvTranspose2d(in_channels=CHANNELS // 2, out_channels=CHANNELS // 2, kernel_size=KERNEL)
        self.decoder_conv4 = nn.ConvTranspose2d(in_channels=CHANNELS // 2, out_channels=1, kernel_size=KERNEL)

    def forward(self, x):
        from ...conv2d_functional import nb16_autoencoder_f32
        enc = (self.encoder_conv1, self.encoder_conv2, self.encoder_conv3, self.encoder_conv4)
        dec = (self.decoder_conv1, self.decoder_conv2, self.decoder_conv3, self.decoder_conv4)
        return nb16_autoencoder_f32(*self.counts_and_horizon(x), enc, dec)

    def loss(self, y_hat, y):
        from ...conv2d_functional import mse_crop_norm
        # normalisation and the 8-pixel crop of the target happen inside the loss kernel
        return mse_crop_norm(y_hat.squeeze(1), self.counts(y))
