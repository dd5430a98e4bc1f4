"""LitModel of the reference's second experiment -- host-side mirror of
experiments/002_cnn_processes_single_sat_image_then_rnn.py:83-316.

Every 5-minute satellite image of the stack is one example: [B, T, W, H, 12] -> B*T images, each given five extra
channels (centre marker, normalised geo x / y, pixel x / y: :140-162, :180-208) and passed through three 3x3 "valid"
convolutions 17 -> 32 -> 32 -> 4 with ReLU; the 4 x 26 x 26 = 2704 features (channel-major, the reference's flatten order)
go through fc1 (+ PV-system embedding) .. fc5 to 8 features per time step, which -- with the flattened NWP values
(10 x 2 x 2), four datetime features and, for the encoder, the PV history -- feed a 2-layer GRU encoder over the history and
a 2-layer GRU decoder over the forecast steps; decoder_fc1/2 give one yield per forecast step.  Loss = NMAE, metrics MSE /
NMAE for Train and Validation (:255-275), Adam lr 0.001 (:298).  The experiment trains in f32 (pl.Trainer(gpus=1)): every
product here is exact f32 (conv2d_functional on csrc/conv2d_f32.hip, fc and GRU on the f32 kernels of experiment 003).

Same constructor (history_len, forecast_len), same attribute / state_dict names and the same batch keys (experiment 003's
plus `sat_x_coords` [B, H] and `sat_y_coords` [B, W], metres).  Deliberate differences from the reference:
  - any batch size works: the reference sizes its centre-marker and pixel-coordinate buffers from params['batch_size'] in
    __init__ (:140-162) and so only runs at B = 32; here the kernels synthesise those channels per image;
  - the output is always [B, forecast_len]: the reference's `.squeeze()` (:250) also drops the batch axis at B = 1;
  - validation_step does not plot an example to Neptune (:277-286);
  - it runs on the MI355X only: CPU tensors raise a RuntimeError (there is no CPU path).
"""
from typing import Optional

import torch
from torch import nn

from ...lightning import LightningModule
from .._flow_join import check_knobs, joined_frames

params = dict(
    batch_size=32,
    history_len=6,    #: Number of timesteps of history, not including t0.
    forecast_len=12,  #: Number of timesteps of forecast.
    image_size_pixels=32,
    nwp_channels=("t", "dswrf", "prate", "r", "sde", "si10", "vis", "lcc", "mcc", "hcc"),
    sat_channels=("HRV", "IR_016", "IR_039", "IR_087", "IR_097", "IR_108", "IR_120", "IR_134", "VIS006", "VIS008", "WV_062",
                  "WV_073"),
)

SAT_X_MEAN = 309000.0
SAT_X_STD = 316387.42073603
SAT_Y_MEAN = 519000.0
SAT_Y_STD = 406454.17945938

TOTAL_SEQ_LEN = params["history_len"] + params["forecast_len"] + 1
CHANNELS = 32
N_CHANNELS_LAST_CONV = 4
KERNEL = 3
EMBEDDING_DIM = 16
NWP_SIZE = len(params["nwp_channels"]) * 2 * 2  # channels x width x height
N_DATETIME_FEATURES = 4
CNN_OUTPUT_SIZE = N_CHANNELS_LAST_CONV * ((params["image_size_pixels"] - 6) ** 2)
FC_OUTPUT_SIZE = 8
RNN_HIDDEN_SIZE = 16


class LitModel(LightningModule):
    name = "exp002_cnn_then_rnn"
    flow_join_in_forward = True

    def __init__(self, history_len=params["history_len"], forecast_len=params["forecast_len"], future_frames: str = "true",
                 flow_channel: Optional[int] = None):
        super().__init__()
        # future_frames (new, optional): "optical_flow" closes the experiment's TODO at :167 (models/_flow_join.py)
        check_knobs(future_frames, flow_channel)
        self.future_frames = future_frames
        self.flow_channel = flow_channel
        self.history_len = history_len
        self.forecast_len = forecast_len
        self.total_seq_len = history_len + forecast_len + 1

        self.sat_conv1 = nn.Conv2d(in_channels=len(params["sat_channels"]) + 5, out_channels=CHANNELS, kernel_size=KERNEL)
        self.sat_conv2 = nn.Conv2d(in_channels=CHANNELS, out_channels=CHANNELS, kernel_size=KERNEL)
        self.sat_conv3 = nn.Conv2d(in_channels=CHANNELS, out_channels=N_CHANNELS_LAST_CONV, kernel_size=KERNEL)

        self.fc1 = nn.Linear(in_features=CNN_OUTPUT_SIZE, out_features=256)
        self.fc2 = nn.Linear(in_features=256 + EMBEDDING_DIM, out_features=128)
        self.fc3 = nn.Linear(in_features=128, out_features=64)
        self.fc4 = nn.Linear(in_features=64, out_features=32)
        self.fc5 = nn.Linear(in_features=32, out_features=FC_OUTPUT_SIZE)
        if EMBEDDING_DIM:
            self.pv_system_id_embedding = nn.Embedding(num_embeddings=940, embedding_dim=EMBEDDING_DIM)
        # plus 1 for history
        self.encoder_rnn = nn.GRU(input_size=FC_OUTPUT_SIZE + N_DATETIME_FEATURES + 1 + NWP_SIZE, hidden_size=RNN_HIDDEN_SIZE,
                                  num_layers=2, batch_first=True)
        self.decoder_rnn = nn.GRU(input_size=FC_OUTPUT_SIZE + N_DATETIME_FEATURES + NWP_SIZE, hidden_size=RNN_HIDDEN_SIZE,
                                  num_layers=2, batch_first=True)
        self.decoder_fc1 = nn.Linear(in_features=RNN_HIDDEN_SIZE, out_features=8)
        self.decoder_fc2 = nn.Linear(in_features=8, out_features=1)

    def encode_images(self, x):
        """[B*T, 2704]: the three convolutions over every satellite image, flattened channel-major (:180-213)."""
        from ...conv2d_functional import sat_encoder_f32
        sat_data = x["sat_data"]
        if not sat_data.is_cuda:
            raise RuntimeError("predict_pv_yield_amd exp002.LitModel runs on the MI355X only: move the module and the batch to "
                               "cuda (there is no CPU fallback)")
        batch_size, seq_len, width, height, n_chans = sat_data.shape
        sat_data = joined_frames(self, sat_data, self.forecast_len, "NTHWC")
        # Stack timesteps as examples (to make a large batch)
        new_batch_size = batch_size * seq_len
        sat_data = sat_data.float().reshape(new_batch_size, width, height, n_chans)
        out = sat_encoder_f32(sat_data, x["sat_x_coords"].float(), x["sat_y_coords"].float(), self.sat_conv1, self.sat_conv2,
                              self.sat_conv3, seq_len)
        return out.reshape(new_batch_size, -1)

    def forward(self, x):
        from ... import functional as Fn
        from ... import perceiver_functional as PF
        # ******************* Satellite imagery *************************
        # Shape: batch_size, seq_length, width, height, channel
        batch_size = x["sat_data"].shape[0]
        out = self.encode_images(x)
        out = Fn.linear_f32(out, self.fc1.weight, self.fc1.bias, relu=True)

        # ********************** Embedding of PV system ID ********************
        if EMBEDDING_DIM:
            pv_row = x["pv_system_row_number"].to(dtype=torch.int64).repeat_interleave(self.total_seq_len)
            out = torch.cat((out, Fn.embedding(self.pv_system_id_embedding.weight, pv_row)), dim=1)

        out = Fn.linear_f32(out, self.fc2.weight, self.fc2.bias, relu=True)
        out = Fn.linear_f32(out, self.fc3.weight, self.fc3.bias, relu=True)
        out = Fn.linear_f32(out, self.fc4.weight, self.fc4.bias, relu=True)
        out = Fn.linear_f32(out, self.fc5.weight, self.fc5.bias, relu=True)

        # ******************* PREP DATA FOR RNN *******************************
        out = out.reshape(batch_size, self.total_seq_len, FC_OUTPUT_SIZE)

        # *********************** NWP Data ************************************
        # Shape: batch_size, channel, seq_length, width, height; the RNN expects seq_len to be dim 1
        nwp_data = x["nwp"].float().permute(0, 2, 1, 3, 4)
        batch_size, nwp_seq_len, n_nwp_chans, nwp_width, nwp_height = nwp_data.shape
        nwp_data = nwp_data.reshape(batch_size, nwp_seq_len, n_nwp_chans * nwp_width * nwp_height)

        rnn_input = torch.cat(
            (out, nwp_data, x["hour_of_day_sin"].unsqueeze(-1), x["hour_of_day_cos"].unsqueeze(-1),
             x["day_of_year_sin"].unsqueeze(-1), x["day_of_year_cos"].unsqueeze(-1)), dim=2).float()

        pv_yield_history = x["pv_yield"][:, : self.history_len + 1].unsqueeze(-1).float()
        encoder_input = torch.cat((rnn_input[:, : self.history_len + 1], pv_yield_history), dim=2)

        _, encoder_hidden = PF.gru(encoder_input, self.encoder_rnn)
        decoder_output, _ = PF.gru(rnn_input[:, -self.forecast_len:], self.decoder_rnn, encoder_hidden)
        # decoder_output is shape batch_size, seq_len, rnn_hidden_size
        b, t, h = decoder_output.shape
        decoder_output = Fn.linear_f32(decoder_output.reshape(b * t, h), self.decoder_fc1.weight, self.decoder_fc1.bias, relu=True)
        decoder_output = Fn.linear_f32(decoder_output, self.decoder_fc2.weight, self.decoder_fc2.bias, relu=False)
        return decoder_output.reshape(b, t)

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
        # the experiment also plots an example to Neptune here (:277-286): left out
        return self._training_or_validation_step(batch, is_train_step=False)

    def configure_optimizers(self):
        from ...optim import HipAdam
        return HipAdam(self.parameters(), lr=0.001)
