"""Synthetic dict batches and a DataModule for experiments/001_CNN_concat_all_timesteps_as_channels.py (the experiment's own
NowcastingDataModule streams from a bucket, outside the hot path): data/seeded.py with HRV only and geo coordinates."""
from ..models.conv2d.exp001 import params
from .seeded import SeededBatchDataModule, SeededBatchDataset, make_fake_sat_batch


def make_fake_exp001_batch(batch_size: int = 32, image_size_pixels: int = 128, generator=None,
                           history_len=params["history_len"], forecast_len=params["forecast_len"]):
    """Seeded dict batch with the experiment's keys and shapes: sat_data [B, T, S, S, 1] (HRV only), sat_x_coords /
    sat_y_coords [B, S], nwp [B, 10, T, 2, 2], four datetime features and pv_yield [B, T], pv_system_row_number [B]."""
    return make_fake_sat_batch(batch_size, image_size_pixels, 1, generator, True, history_len, forecast_len)


class FakeExp001Dataset(SeededBatchDataset):
    make_batch = staticmethod(make_fake_exp001_batch)


class Exp001DataModule(SeededBatchDataModule):
    dataset = FakeExp001Dataset
