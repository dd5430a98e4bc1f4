"""LitAutoEncoder of the reference's first experiment -- host-side mirror of
experiments/001_CNN_concat_all_timesteps_as_channels.py:225-380.

The HRV frames 0..history_len of each example are stacked as channels (channel index = frame), five synthesised channels
follow (centre marker, normalised geo x / y, pixel x / y: :278-301), and three 3x3 "valid" convolutions 12 -> 144 -> 144 ->
144 with ReLU, the first two each followed by MaxPool2d(3), give 144 x 11 x 11 = 17 424 features (channel-major, the
reference's flatten order).  fc1 (-> 256), then the head: fc1's output, the PV history, the flattened NWP [10, 19, 2, 2],
four datetime features x 19 and the PV-system embedding (1 115 values) through fc2..fc5 to forecast yields.  Loss = NMAE,
metrics MSE / NMAE for Train and Validation (:352-364), Adam lr 0.001 (:378-380).  The experiment trains in f32
(pl.Trainer(gpus=1)): every product here is exact f32 (conv2d_functional on csrc/conv2d_pool_f32.hip, fc layers and
embedding on the f32 kernels of experiment 003).

Same constructor (history_len, forecast_len), attribute / state_dict names and batch keys.  NWP_SIZE, N_DATETIME_FEATURES and
fc5's width come from the module-level params, as in the reference.  Deliberate differences from the reference:
  - one keyword more, n_pv_systems=940: the reference sizes the embedding from its module-level data module (:260-262);
  - validation_step does not plot an example to Neptune (:370-374);
  - it runs on the MI355X only: CPU tensors raise a RuntimeError (there is no CPU path);
  - it takes 128 x 128 x 1 images only (fc1's width, 144 x 11 x 11, fixes the size) and raises a ValueError otherwise.
"""
import torch
from torch import nn

from ...lightning import LightningModule

params = dict(
    batch_size=32,
    history_len=6,    #: Number of timesteps of history, not including t0.
    forecast_len=12,  #: Number of timesteps of forecast.
    nwp_channels=("t", "dswrf", "prate", "r", "sde", "si10", "vis", "lcc", "mcc", "hcc"),
)

SAT_X_MEAN = 309000.0
SAT_X_STD = 316387.42073603
SAT_Y_MEAN = 519000.0
SAT_Y_STD = 406454.17945938

TOTAL_SEQ_LEN = params["history_len"] + params["forecast_len"] + 1
CHANNELS = 144
KERNEL = 3
EMBEDDING_DIM = 16
NWP_SIZE = 10 * 2 * 2 * TOTAL_SEQ_LEN  # channels x width x height
N_DATETIME_FEATURES = 4 * TOTAL_SEQ_LEN
IMAGE_SIZE_PIXELS = 128                # 128 -> 126 -> 42 -> 40 -> 13 -> 11: fc1 takes CHANNELS * 11 * 11


class LitAutoEncoder(LightningModule):
    name = "exp001_cnn"

    def __init__(self, history_len=params["history_len"], forecast_len=params["forecast_len"], n_pv_systems=940):
        super().__init__()
        self.history_len = history_len
        self.forecast_len = forecast_len

        self.sat_conv1 = nn.Conv2d(in_channels=history_len + 6, out_channels=CHANNELS, kernel_size=KERNEL)
        self.sat_conv2 = nn.Conv2d(in_channels=CHANNELS, out_channels=CHANNELS, kernel_size=KERNEL)
        self.sat_conv3 = nn.Conv2d(in_channels=CHANNELS, out_channels=CHANNELS, kernel_size=KERNEL)

        self.maxpool = nn.MaxPool2d(kernel_size=KERNEL)

        self.fc1 = nn.Linear(in_features=CHANNELS * 11 * 11, out_features=256)
        self.fc2 = nn.Linear(in_features=256 + EMBEDDING_DIM + NWP_SIZE + N_DATETIME_FEATURES + history_len + 1,
                             out_features=128)
        self.fc3 = nn.Linear(in_features=128, out_features=128)
        self.fc4 = nn.Linear(in_features=128, out_features=128)
        self.fc5 = nn.Linear(in_features=128, out_features=params["forecast_len"])

        if EMBEDDING_DIM:
            self.pv_system_id_embedding = nn.Embedding(num_embeddings=n_pv_systems, embedding_dim=EMBEDDING_DIM)

    def forward(self, x):
        from ... import functional as Fn
        from ...conv2d_functional import sat_encoder001_f32
        # ******************* Satellite imagery *************************
        # Shape: batch_size, seq_length, width, height, channel
        sat_data = x["sat_data"]
        if not sat_data.is_cuda:
            raise RuntimeError("predict_pv_yield_amd exp001.LitAutoEncoder runs on the MI355X only: move the module and the "
                               "batch to cuda (there is no CPU fallback)")
        n_frames = self.history_len + 1
        s = IMAGE_SIZE_PIXELS
        if sat_data.dim() != 5 or tuple(sat_data.shape[2:]) != (s, s, 1) or sat_data.shape[1] < n_frames:
            raise ValueError(f"exp001.LitAutoEncoder takes sat_data [B, T >= {n_frames}, {s}, {s}, 1] (HRV only): fc1's "
                             f"{CHANNELS} x 11 x 11 inputs fix the image size; got {tuple(sat_data.shape)}")
        batch_size = sat_data.shape[0]
        # frames 0..history_len stacked as channels, plus the five extra channels: built inside the kernels
        out = sat_encoder001_f32(sat_data.float(), x["sat_x_coords"].float(), x["sat_y_coords"].float(), self.sat_conv1,
                                 self.sat_conv2, self.sat_conv3, n_frames)
        out = out.reshape(batch_size, CHANNELS * 11 * 11)
        out = Fn.linear_f32(out, self.fc1.weight, self.fc1.bias, relu=True)

        # *********************** NWP Data **************************************
        # Shape: batch_size, channel, seq_length, width, height
        nwp_data = x["nwp"].float().reshape(batch_size, -1)

        out = torch.cat(
            (out, x["pv_yield"][:, : self.history_len + 1].float(), nwp_data, x["hour_of_day_sin"].float(),
             x["hour_of_day_cos"].float(), x["day_of_year_sin"].float(), x["day_of_year_cos"].float()), dim=1)

        # Embedding of PV system ID
        if EMBEDDING_DIM:
            pv_row = x["pv_system_row_number"].to(dtype=torch.int64)
            out = torch.cat((out, Fn.embedding(self.pv_system_id_embedding.weight, pv_row)), dim=1)

        # Fully connected layers.
        out = Fn.linear_f32(out, self.fc2.weight, self.fc2.bias, relu=True)
        out = Fn.linear_f32(out, self.fc3.weight, self.fc3.bias, relu=True)
        out = Fn.linear_f32(out, self.fc4.weight, self.fc4.bias, relu=True)
        return Fn.linear_f32(out, self.fc5.weight, self.fc5.bias, relu=True)

    def _training_or_validation_step(self, batch, is_train_step):
        from ...functional import forecast_losses
        y_hat = self(batch)
        y = batch["pv_yield"][:, -self.forecast_len:].float()
        mse_loss, nmae_loss, _, _ = forecast_losses(y_hat, y)      # one launch; nmae carries the gradient
        tag = "Train" if is_train_step else "Validation"
        self.log_dict({f"MSE/{tag}": mse_loss}, on_step=is_train_step, on_epoch=True)
        self.log_dict({f"NMAE/{tag}": nmae_loss}, on_step=is_train_step, on_epoch=True)
        return nmae_loss

    def training_step(self, batch, batch_idx):
        return self._training_or_validation_step(batch, is_train_step=True)

    def validation_step(self, batch, batch_idx):
        # the experiment also plots an example to Neptune here (:370-374): left out
        return self._training_or_validation_step(batch, is_train_step=False)

    def configure_optimizers(self):
        from ...optim import HipAdam
        return HipAdam(self.parameters(), lr=0.001)
