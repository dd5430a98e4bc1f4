"""CPU: the table of tests/notebook_model_checks.py.  Every notebook frame predictor in the package has a record; the checks
each record switches on are the ones its own test file had before the checks were stated once (a literal, so that a change to a
record never edits it by accident: adding a check to a notebook is a change to this table too); and what a record says about its
golden fixture and its optimizer is what the fixture and the model say."""
import glob
import os

import numpy as np
import pytest

import notebook_model_checks as C
from conv2d_f32_helpers import ROOT

EVERY = {"golden", "full_size", "replay"}
CHECKS = {
    "nb05": EVERY | {"deterministic"},
    "nb07": EVERY | {"batch_of_one", "deterministic", "fit", "graph_fit"},
    "nb08": EVERY | {"batch_of_one", "deterministic", "fit", "graph_fit"},
    "nb09": EVERY | {"graph_fit"},
    "nb10": EVERY | {"graph_fit"},
    "nb12": EVERY | {"graph_fit"},
    "nb15": EVERY | {"deterministic", "fit", "graph_fit"},
    "nb16": EVERY | {"deterministic", "fit", "graph_fit"},
}
# (full sizes, steps replayed, training batches beyond the Trainer's eager steps, what the two bit-for-bit runs train on)
FORMS = {"nb05": (2, 5, None, "golden"), "nb07": (2, 5, 3, "drawn"), "nb08": (2, 5, 3, "drawn"), "nb09": (1, 3, 2, None),
         "nb10": (1, 3, 2, None), "nb12": (1, 3, 2, None), "nb15": (2, 5, 3, "drawn"), "nb16": (2, 5, 3, "drawn")}


def test_every_notebook_model_has_a_case():
    modules = sorted(os.path.relpath(p, ROOT)[:-3].replace(os.sep, ".")
                     for p in glob.glob(os.path.join(ROOT, "predict_pv_yield_amd", "models", "conv[23]d", "nb*.py"))
                     if "class LitAutoEncoder" in open(p).read())
    assert modules == sorted(case.model for case in C.CASES.values()) and len(modules) == len(CHECKS)
    assert all(name == case.name for name, case in C.CASES.items())


@pytest.mark.parametrize("name", sorted(CHECKS))
def test_case_has_the_checks_of_the_table(name):
    case = C.CASES[name]
    assert case.checks() == CHECKS[name]
    assert (len(case.full_sizes), case.replay_steps, case.graph_fit_extra, case.deterministic) == FORMS[name]
    assert case.replay_from_golden == (case.deterministic == "golden")
    # the fit checks name a datamodule and, for the checkpoint, its keys: the model's own, in order
    if case.checks() & {"fit", "graph_fit"}:
        assert callable(case.dm_cls())
    model = case.model_cls()()
    if "fit" in case.checks():
        assert case.state_keys == list(model.state_dict())
    # the learning rate that picks the Adam bounds is the model's own
    assert model.configure_optimizers().param_groups[0]["lr"] == case.lr and case.lr in C.ADAM_BOUNDS
    if case.routed:
        assert case.R.ROUTED_TOL == 2e-2 and any(k.startswith(case.routed) for k in model.state_dict())
    # the golden cases a record says store parameters after three steps are the ones the fixture stores
    gold = np.load(case.golden)
    first = next(iter(model.state_dict()))
    assert tuple(tag for tag in ("a", "b") if f"{tag}/step3/{first}" in gold.files) == case.step3_tags
    for tag in ("a", "b"):
        assert f"{tag}/y_hat" in gold.files and len(gold[f"{tag}/losses"]) == 3
