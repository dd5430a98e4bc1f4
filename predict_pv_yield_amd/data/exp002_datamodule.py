"""Synthetic dict batches and a DataModule for experiments/002_cnn_processes_single_sat_image_then_rnn.py (the experiment's
own loader reads prepared NetCDF batches from a bucket, outside the hot path): data/seeded.py with geo coordinates."""
from ..models.conv2d.exp002 import params
from .seeded import SeededBatchDataModule, SeededBatchDataset, make_fake_sat_batch


def make_fake_exp002_batch(batch_size: int = 32, image_size_pixels: int = 32, generator=None,
                           history_len=params["history_len"], forecast_len=params["forecast_len"]):
    """Seeded dict batch with the experiment's keys and shapes: experiment 003's keys plus sat_x_coords / sat_y_coords [B, S]."""
    return make_fake_sat_batch(batch_size, image_size_pixels, len(params["sat_channels"]), generator, True, history_len,
                               forecast_len)


class FakeExp002Dataset(SeededBatchDataset):
    make_batch = staticmethod(make_fake_exp002_batch)

    def __init__(self, batch_size: int = 32, image_size_pixels: int = 32, length: int = 4, seed: int = 1234):
        super().__init__(batch_size, image_size_pixels, length, seed)


class Exp002DataModule(SeededBatchDataModule):
    dataset = FakeExp002Dataset

    def __init__(self, batch_size: int = 32, image_size_pixels: int = 32, n_train_data: int = 8, n_val_data: int = 2,
                 seed: int = 1234):
        super().__init__(batch_size, image_size_pixels, n_train_data, n_val_data, seed)
