"""Synthetic example dicts and a DataModule for notebooks/12_just_3d_conv.ipynb.  The super-batches and the order of draws
are those of data/nb10_datamodule.py (make_fake_super_batch, draw_example: the notebook's super_batch_to_example /
sample_squares cells are the same in both notebooks); what differs is FORECAST_HORIZON, which this notebook normalises in the
loader (normalise_forecast_horizon, 12_just_3d_conv.ipynb:757-768): float32 (h - mean) / std of arange(1, 25).  The batch
keeps the notebook's three keys: HISTORICAL_SAT_IMAGES [B, 4, S, S] f32, FORECAST_HORIZON [B] f32, TARGET_SAT_IMAGE [B, s, s]
f32 with s = (S - 1) // 2 + 1."""
from functools import partial

import numpy as np

from ..models.conv3d.nb12_just_3d_conv import output_side
from . import nb10_datamodule as nb10
from .nb10_datamodule import Nb10DataModule, draw_example, make_fake_super_batch  # noqa: F401

FCST_HORIZON_SEQ = np.arange(1, 25, dtype=np.float32)
FCST_HORIZON_MEAN = FCST_HORIZON_SEQ.mean()
FCST_HORIZON_STD = FCST_HORIZON_SEQ.std()


def normalise_forecast_horizon(forecast_horizon: int) -> np.float32:
    """Timesteps 1..24 (5 minutes each) to the notebook's float32 network input."""
    forecast_horizon = np.float32(forecast_horizon)
    forecast_horizon -= FCST_HORIZON_MEAN
    forecast_horizon /= FCST_HORIZON_STD
    return forecast_horizon


super_batch_to_example = partial(nb10.super_batch_to_example, horizon_form=normalise_forecast_horizon)
make_fake_nb12_batch = partial(nb10.make_fake_batch, side_rule=output_side, horizon_form=normalise_forecast_horizon)


class Nb12DataModule(Nb10DataModule):
    """Nb10DataModule's seeded batches (same super-batches, same draws) with the horizon normalised as notebook 12 does."""

    make_batch = staticmethod(make_fake_nb12_batch)
