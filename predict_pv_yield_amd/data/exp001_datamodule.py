"""Synthetic dict batches and a DataModule for experiments/001_CNN_concat_all_timesteps_as_channels.py (the experiment's own
NowcastingDataModule streams from a bucket, outside the hot path).  Whole batches per item, equal shards per rank, like
data/exp002_datamodule.py."""
import torch

from ..distributed import shard_indices
from ..lightning import LightningDataModule
from ..models.conv2d.exp001 import params
from .exp003_datamodule import _Slice

PIXEL_METRES = 2000.0   # spacing of the fake geo coordinates (one value per pixel column / row)


def make_fake_exp001_batch(batch_size: int = 32, image_size_pixels: int = 128, generator=None,
                           history_len=params["history_len"], forecast_len=params["forecast_len"]):
    """Seeded dict batch with the experiment's keys and shapes: sat_data [B, T, S, S, 1] (HRV only), sat_x_coords /
    sat_y_coords [B, S] (metres near the experiment's means; x grows along the image's last axis, y shrinks down its rows),
    nwp [B, 10, T, 2, 2], four datetime features and pv_yield [B, T], pv_system_row_number [B]; T = history + forecast + 1."""
    g = generator
    t = history_len + forecast_len + 1
    s = image_size_pixels
    phase = torch.rand(batch_size, 1, generator=g) * 6.2831853
    steps = torch.arange(t, dtype=torch.float32)[None] * 0.02
    ramp = torch.arange(s, dtype=torch.float32)[None] * PIXEL_METRES
    x0 = 309000.0 + (torch.rand(batch_size, 1, generator=g) - 0.5) * 400000.0
    y0 = 519000.0 + (torch.rand(batch_size, 1, generator=g) - 0.5) * 500000.0
    return {
        "sat_data": torch.randn(batch_size, t, s, s, 1, generator=g),
        "sat_x_coords": x0 + ramp,
        "sat_y_coords": y0 - ramp,
        "pv_system_row_number": torch.randint(0, 940, (batch_size,), generator=g),
        "nwp": torch.randn(batch_size, len(params["nwp_channels"]), t, 2, 2, generator=g),
        "hour_of_day_sin": torch.sin(phase + steps), "hour_of_day_cos": torch.cos(phase + steps),
        "day_of_year_sin": torch.sin(phase * 0.5 + steps * 0.01), "day_of_year_cos": torch.cos(phase * 0.5 + steps * 0.01),
        "pv_yield": torch.rand(batch_size, t, generator=g),
    }


class FakeExp001Dataset(torch.utils.data.Dataset):
    """Each item is a whole seeded batch (DataLoader(batch_size=None)), like the experiment's own loader."""

    def __init__(self, batch_size: int = 32, image_size_pixels: int = 128, length: int = 4, seed: int = 1234):
        self.batch_size, self.image_size_pixels, self.length, self.seed = batch_size, image_size_pixels, length, seed

    def __len__(self):
        return self.length

    def __getitem__(self, idx):
        if idx >= self.length:
            raise IndexError(idx)
        return make_fake_exp001_batch(self.batch_size, self.image_size_pixels, torch.Generator().manual_seed(self.seed + idx))


class Exp001DataModule(LightningDataModule):
    def __init__(self, batch_size: int = 32, image_size_pixels: int = 128, n_train_data: int = 8, n_val_data: int = 2,
                 seed: int = 1234):
        super().__init__()
        self.batch_size, self.image_size_pixels = batch_size, image_size_pixels
        self.n_train_data, self.n_val_data, self.seed = n_train_data, n_val_data, seed

    def _loader(self, n, seed):
        ds = _Slice(FakeExp001Dataset(self.batch_size, self.image_size_pixels, length=n, seed=seed), shard_indices(n))
        return torch.utils.data.DataLoader(ds, batch_size=None, num_workers=0)

    def train_dataloader(self):
        return self._loader(self.n_train_data, self.seed)

    def val_dataloader(self):
        return self._loader(self.n_val_data, self.seed + 100000)

    def test_dataloader(self):
        return self._loader(self.n_val_data, self.seed + 200000)
