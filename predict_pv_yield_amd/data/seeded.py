"""Seeded synthetic dict batches and the DataModule behind the fake datamodules of experiments 001, 002 and 003 (their own
loaders read prepared batches or zarr stores from a bucket, outside the hot path).  Whole batches per item, equal shards
per rank (padded by wrapping) like data/dataloader.py."""
import torch

from ..distributed import shard_indices
from ..lightning import LightningDataModule

PIXEL_METRES = 2000.0   # spacing of the fake geo coordinates (one value per pixel column / row)
N_NWP_CHANNELS = 10


def make_fake_sat_batch(batch_size, image_size_pixels, n_sat_channels, generator=None, with_coords=False, history_len=6,
                        forecast_len=12):
    """Seeded dict batch with the experiments' keys: sat_data [B, T, S, S, n_sat_channels], pv_system_row_number [B], nwp
    [B, 10, T, 2, 2], four datetime features and pv_yield [B, T]; T = history + forecast + 1.  with_coords adds sat_x_coords
    / sat_y_coords [B, S] after sat_data: metres near the experiments' means, x growing along the image's last axis, y
    shrinking down its rows (their offsets are drawn before sat_data)."""
    g = generator
    t = history_len + forecast_len + 1
    s = image_size_pixels
    phase = torch.rand(batch_size, 1, generator=g) * 6.2831853
    steps = torch.arange(t, dtype=torch.float32)[None] * 0.02
    batch = {}
    if with_coords:
        ramp = torch.arange(s, dtype=torch.float32)[None] * PIXEL_METRES
        x0 = 309000.0 + (torch.rand(batch_size, 1, generator=g) - 0.5) * 400000.0
        y0 = 519000.0 + (torch.rand(batch_size, 1, generator=g) - 0.5) * 500000.0
    batch["sat_data"] = torch.randn(batch_size, t, s, s, n_sat_channels, generator=g)
    if with_coords:
        batch["sat_x_coords"], batch["sat_y_coords"] = x0 + ramp, y0 - ramp
    batch["pv_system_row_number"] = torch.randint(0, 940, (batch_size,), generator=g)
    batch["nwp"] = torch.randn(batch_size, N_NWP_CHANNELS, t, 2, 2, generator=g)
    batch.update(hour_of_day_sin=torch.sin(phase + steps), hour_of_day_cos=torch.cos(phase + steps),
                 day_of_year_sin=torch.sin(phase * 0.5 + steps * 0.01), day_of_year_cos=torch.cos(phase * 0.5 + steps * 0.01),
                 pv_yield=torch.rand(batch_size, t, generator=g))
    return batch


class SeededBatchDataset(torch.utils.data.Dataset):
    """Each item is a whole seeded batch (DataLoader(batch_size=None)), like the experiments' own loaders: item i is
    make_batch(batch_size, image_size_pixels, a generator seeded with seed + i).  Subclasses set make_batch."""
    make_batch = None

    def __init__(self, batch_size: int = 32, image_size_pixels: int = 128, length: int = 4, seed: int = 1234):
        self.batch_size, self.image_size_pixels, self.length, self.seed = batch_size, image_size_pixels, length, seed

    def __len__(self):
        return self.length

    def __getitem__(self, idx):
        if idx >= self.length:
            raise IndexError(idx)
        return self.make_batch(self.batch_size, self.image_size_pixels, torch.Generator().manual_seed(self.seed + idx))


class _Slice(torch.utils.data.Dataset):
    def __init__(self, base, indices):
        self.base, self.indices = base, list(indices)

    def __len__(self):
        return len(self.indices)

    def __getitem__(self, i):
        if i >= len(self):
            raise IndexError(i)
        return self.base[self.indices[i]]


class SeededBatchDataModule(LightningDataModule):
    """Train / val / test loaders over this rank's shard of a SeededBatchDataset subclass (set as dataset)."""
    dataset = None

    def __init__(self, batch_size: int = 32, image_size_pixels: int = 128, n_train_data: int = 8, n_val_data: int = 2,
                 seed: int = 1234):
        super().__init__()
        self.batch_size, self.image_size_pixels = batch_size, image_size_pixels
        self.n_train_data, self.n_val_data, self.seed = n_train_data, n_val_data, seed

    def _loader(self, n, seed):
        ds = _Slice(self.dataset(self.batch_size, self.image_size_pixels, length=n, seed=seed), shard_indices(n))
        return torch.utils.data.DataLoader(ds, batch_size=None, num_workers=0)

    def train_dataloader(self):
        return self._loader(self.n_train_data, self.seed)

    def val_dataloader(self):
        return self._loader(self.n_val_data, self.seed + 100000)

    def test_dataloader(self):
        return self._loader(self.n_val_data, self.seed + 200000)
