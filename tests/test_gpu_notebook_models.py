"""GPU: every notebook frame predictor's model-level checks (tests/notebook_model_checks.py: the checks, the record per
notebook and the table of which notebook has which check).  Ids begin with the notebook: `-k nb08` selects one."""
import pytest

import notebook_model_checks as C

pytestmark = pytest.mark.gpu
AB = ("a", "b")


def _having(check):
    return [case for case in C.CASES.values() if check in case.checks()]


def _params(pairs):
    """(case, item) pairs as pytest params with ids nbXX or nbXX-item."""
    return [pytest.param(case, item, id=case.name if item is None else f"{case.name}-{item}") for case, item in pairs]


@pytest.mark.parametrize("case, tag", _params((c, tag) for c in _having("golden") for tag in AB))
def test_model_against_golden(device, case, tag):
    C.check_model_against_golden(device, case, tag)


@pytest.mark.parametrize("case, size", _params((c, f"{size[0]}x{size[1]}") for c in _having("full_size") for size in c.full_sizes))
def test_full_size_forward_and_loss(device, case, size):
    b, s, shape = next(fs for fs in case.full_sizes if f"{fs[0]}x{fs[1]}" == size)
    C.check_full_size_forward_and_loss(device, case, b, s, shape)


@pytest.mark.parametrize("case, _", _params((c, None) for c in _having("batch_of_one")))
def test_batch_axis_survives_a_batch_of_one(device, case, _):
    C.check_batch_of_one(device, case)


@pytest.mark.parametrize("case, tag", _params((c, tag) for c in _having("deterministic")
                                              for tag in (AB if c.deterministic == "golden" else (None,))))
def test_two_eager_runs_are_equal_bit_for_bit(device, case, tag):
    C.check_two_eager_runs_are_equal_bit_for_bit(device, case, tag)


@pytest.mark.parametrize("case, tag", _params((c, tag) for c in _having("replay")
                                              for tag in (AB if c.replay_from_golden else (None,))))
def test_train_step_replays_as_a_hip_graph(device, case, tag):
    C.check_train_step_replays_as_a_hip_graph(device, case, tag)


@pytest.mark.parametrize("case, _", _params((c, None) for c in _having("fit")))
def test_trainer_fit_on_the_fake_datamodule(device, case, _, tmp_path):
    C.check_trainer_fit_on_the_fake_datamodule(device, case, tmp_path)


@pytest.mark.parametrize("case, _", _params((c, None) for c in _having("graph_fit")))
def test_trainer_fit_with_hip_graph_matches_the_eager_fit(device, case, _):
    C.check_trainer_fit_with_hip_graph_matches_the_eager_fit(device, case)
