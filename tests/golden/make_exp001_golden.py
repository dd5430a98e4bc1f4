"""Generates tests/golden/exp001_small.npz by EXECUTING THE REFERENCE'S OWN MODULE SOURCE
(experiments/001_CNN_concat_all_timesteps_as_channels.py of the upstream repository) on the CPU.

Run on a machine that holds the upstream tree (PV_REFERENCE, default /root/reference):
    python tests/golden/make_exp001_golden.py

The module imports packages that contribute no arithmetic to LitAutoEncoder.forward / configure_optimizers; they are
replaced by import stubs *in this generator only*: pytorch_lightning (LightningModule -> torch.nn.Module with a CPU `device`
and a no-op log_dict; a Trainer whose fit does nothing), neptune.new.*, nowcasting_dataset.datamodule (a data module whose
prepare_data / setup do nothing and whose pv_data_source.pv_metadata has 940 rows), nowcasting_dataset.geospatial and
tilemapbase.  Inputs and initial parameters are drawn by draw_batch / draw_parameters below from
numpy.random.default_rng(seed), so the test regenerates them and the fixture only holds results: the forward output, both
losses, every parameter's gradient and every parameter after one torch.optim.Adam(lr=0.001) step -- for parameters of more
than SAMPLE_ABOVE elements as a fixed seeded sample of entries plus the full float64 sum and norm of the gradient.  No
reference source text is stored.
"""
import os
import sys
import types

import numpy as np
import torch

REF = os.environ.get("PV_REFERENCE", "/root/reference")
SRC = os.path.join("experiments", "001_CNN_concat_all_timesteps_as_channels.py")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "exp001_small.npz")

SEED = 2001
BATCH, SEQ, PIXELS = 2, 19, 128
SAMPLE_ABOVE = 20000
N_SAMPLES = 4096


def draw_batch(seed=SEED, batch=BATCH, seq=SEQ, pixels=PIXELS):
    """The batch as float32 / int64 numpy arrays (experiments/001's keys)."""
    rng = np.random.default_rng(seed)
    ramp = np.arange(pixels, dtype=np.float64) * 2000.0
    x0 = 309000.0 + rng.uniform(-200000.0, 200000.0, (batch, 1))
    y0 = 519000.0 + rng.uniform(-250000.0, 250000.0, (batch, 1))
    phase = rng.uniform(0.0, 6.2831853, (batch, 1))
    steps = np.arange(seq)[None] * 0.02
    f32 = np.float32
    return {
        "sat_data": rng.standard_normal((batch, seq, pixels, pixels, 1)).astype(f32),
        "sat_x_coords": (x0 + ramp).astype(f32),
        "sat_y_coords": (y0 - ramp).astype(f32),
        "pv_system_row_number": rng.integers(0, 940, batch).astype(np.int64),
        "nwp": rng.standard_normal((batch, 10, seq, 2, 2)).astype(f32),
        "hour_of_day_sin": np.sin(phase + steps).astype(f32), "hour_of_day_cos": np.cos(phase + steps).astype(f32),
        "day_of_year_sin": np.sin(phase * 0.5 + steps * 0.01).astype(f32),
        "day_of_year_cos": np.cos(phase * 0.5 + steps * 0.01).astype(f32),
        "pv_yield": rng.uniform(0.0, 1.0, (batch, seq)).astype(f32),
    }


def draw_parameters(shapes, seed=SEED + 1):
    """{name: float32 array}: uniform(-s, s), s = 1/sqrt(fan-in) (0.1 for vectors), drawn in sorted-name order."""
    rng = np.random.default_rng(seed)
    out = {}
    for name in sorted(shapes):
        shape = tuple(shapes[name])
        s = 1.0 / np.sqrt(np.prod(shape[1:])) if len(shape) > 1 else 0.1
        out[name] = rng.uniform(-s, s, shape).astype(np.float32)
    return out


def sampled(numel):
    return numel > SAMPLE_ABOVE


def sample_index(numel, seed=SEED + 2):
    return np.sort(np.random.default_rng(seed).choice(numel, N_SAMPLES, replace=False))


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


def install_stubs():
    class LightningModule(torch.nn.Module):
        device = torch.device("cpu")

        def log_dict(self, d, **kw):
            self.logged = {k: float(v) for k, v in d.items()}

    class Trainer:
        def __init__(self, *a, **kw):
            pass

        def fit(self, *a, **kw):
            pass

    class NeptuneLogger:
        version = None

        def __init__(self, *a, **kw):
            pass

    class NowcastingDataModule:
        def __init__(self, *a, **kw):
            self.pv_data_source = types.SimpleNamespace(pv_metadata=range(940))

        def prepare_data(self):
            pass

        def setup(self):
            pass

    _stub("pytorch_lightning", LightningModule=LightningModule, Trainer=Trainer)
    _stub("neptune")
    _stub("neptune.new")
    _stub("neptune.new.integrations")
    _stub("neptune.new.integrations.pytorch_lightning", NeptuneLogger=NeptuneLogger)
    _stub("neptune.new.types", File=None)
    _stub("nowcasting_dataset")
    _stub("nowcasting_dataset.datamodule", NowcastingDataModule=NowcastingDataModule)
    _stub("nowcasting_dataset.geospatial", osgb_to_lat_lon=None)
    _stub("tilemapbase", init=lambda **kw: None)


def main():
    install_stubs()
    ns = {"__name__": "exp001_reference"}
    path = os.path.join(REF, SRC)
    exec(compile(open(path).read(), path, "exec"), ns)
    torch.manual_seed(0)
    model = ns["LitAutoEncoder"]()
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    init = draw_parameters(shapes)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in init.items()})
    batch = {k: torch.from_numpy(v) for k, v in draw_batch().items()}

    y_hat = model(batch)
    y = batch["pv_yield"][:, -model.forecast_len:]
    loss = model.training_step(batch, 0)
    mse = torch.nn.functional.mse_loss(y_hat, y)
    opt = model.configure_optimizers()
    opt.zero_grad()
    loss.backward()
    grads = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
    opt.step()
    after = {k: p.detach().clone() for k, p in model.named_parameters()}

    out = {"y_hat": y_hat.detach().numpy(), "nmae": np.float32(loss.item()), "mse": np.float32(mse.item()),
           "param_names": np.array(sorted(shapes)), "seed": np.int64(SEED)}
    for k in grads:
        g, a = grads[k].numpy(), after[k].numpy()
        if sampled(g.size):
            idx = sample_index(g.size)
            out[f"grad/{k}/sample"] = g.reshape(-1)[idx]
            out[f"after/{k}/sample"] = a.reshape(-1)[idx]
            out[f"grad/{k}/sum"] = np.float64(g.astype(np.float64).sum())
            out[f"grad/{k}/norm"] = np.float64(np.linalg.norm(g.astype(np.float64)))
        else:
            out[f"grad/{k}"] = g
            out[f"after/{k}"] = a
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: nmae {loss.item():.6f} mse {mse.item():.6f}, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
