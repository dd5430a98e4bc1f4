"""Helpers shared by tests/test_gpu_exp001.py and tests/test_gpu_exp002.py, the exact-f32 Conv2d models' GPU tests."""
import importlib.util
import os

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ELEM_TOL = 1e-6      # per element, relative to its sum of |products|
NORM_TOL = 1e-5      # relative norm of a reduction (weight / bias gradient)


def _golden_module(experiment):
    """tests/golden/make_<experiment>_golden.py, the script that made the experiment's golden fixture."""
    spec = importlib.util.spec_from_file_location(f"make_{experiment}_golden", os.path.join(ROOT, "tests", "golden",
                                                                                           f"make_{experiment}_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def params64(state, requires_grad=True):
    """A state_dict (or name -> array) as float64 CPU leaves: the parameters of a tests/nbXX_reference.py forward64."""
    return {k: torch.as_tensor(v).detach().cpu().double().clone().requires_grad_(requires_grad) for k, v in state.items()}


def _rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _within(got, ref64, absref64, tol=ELEM_TOL, what=""):
    err = (got.double().cpu() - ref64).abs()
    bound = tol * absref64 + 1e-30
    worst = (err / bound).max().item()
    assert worst <= 1.0, f"{what}: error {worst:.2f} x the bound {tol} x sum|products|"


def _to(batch, device):
    return {k: v.to(device) for k, v in batch.items()}


def _ops():
    from predict_pv_yield_amd import hip_ops as K
    return K
