"""GPU: the operand copies kernels read instead of the f32 master weights, and whether they are still current after the master
changed in a way their cache key cannot see -- HIP-graph replays (raw-pointer writes, no Python), load_state_dict while a
captured step lives, a Trainer in graph mode validating between epochs.

The copies: `_pv_packed` (bf16 fragment images of conv weights), `_pv_split2` (two-term half-float split of an fp32 conv
weight, Conv3dF32OnF16x2), `_pv_bf16_shadow` (fc1's bf16 operand).  The oracle is a cold twin: a model of the same config
that loaded the model's state_dict() and has built none of them yet.  The same kernels on the same weights give the same
bits, so outputs are compared with torch.equal.  Each case also checks that the cached route really ran (a shape that fell
back to another path would pass without testing anything).  experiment 002 and 003 keep no such copies today: they stay in
the matrix as guards.
"""
import copy

import pytest
import torch

from predict_pv_yield_amd import functional as F

pytestmark = pytest.mark.gpu

# the shapes of tests/test_gpu_training.py::test_hip_graph_train_step_matches_eager: the fp32 layers take the half-float form
# (batch * To * Ho * Wo >= 65536: functional.conv_f16x2_takes)
CONV3D_KW = dict(include_pv_yield=False, include_nwp=False, forecast_minutes=30, history_minutes=55, number_of_conv3d_layers=4,
                 conv3d_channels=32, image_size_pixels=64, number_sat_channels=11, fc1_output_features=128,
                 fc2_output_features=128, fc3_output_features=64, output_variable="pv_yield")

# the copy getters each route calls on its way to the kernels
ROUTE = {"conv3d-bf16": ("packed_conv_weight", "bf16_shadow_of"), "conv3d-fp32": ("split2_conv_weight",),
         "exp002": (), "exp003-f32": (), "exp003-bf16": ()}


def _to(batch, device):
    return {k: v.to(device) for k, v in batch.items()}


def _case(name, device):
    """(make_model, batch(seed), lr) of a model of the matrix."""
    if name.startswith("conv3d"):
        from predict_pv_yield_amd.models.conv3d.model import Model
        precision = name.split("-")[1]

        def batch(seed):
            g = torch.Generator(device=device).manual_seed(seed)
            return {"satellite": {"data": torch.randn(4, 11, 18, 64, 64, generator=g, device=device)},
                    "pv": {"pv_yield": torch.rand(4, 18, 128, generator=g, device=device)}}
        return (lambda: Model(**CONV3D_KW, precision=precision)), batch, 5e-4
    if name == "exp002":
        from predict_pv_yield_amd.data.exp002_datamodule import make_fake_exp002_batch
        from predict_pv_yield_amd.models.conv2d.exp002 import LitModel
        return LitModel, (lambda seed: _to(make_fake_exp002_batch(32, 32, torch.Generator().manual_seed(seed)), device)), 1e-3
    from predict_pv_yield_amd.models.perceiver.exp003 import LitModel, make_fake_exp003_batch
    operand_dtype = name.split("-")[1]
    return ((lambda: LitModel(operand_dtype=operand_dtype)),
            (lambda seed: _to(make_fake_exp003_batch(2, 64, torch.Generator().manual_seed(seed)), device)), 5e-4)


def _count_copy_getters(monkeypatch):
    """Counts the calls of functional's copy getters (the autograd Functions look them up in the module at call time)."""
    calls = {}
    for name in ("packed_conv_weight", "split2_conv_weight", "bf16_shadow_of"):
        real = getattr(F, name)

        def counted(*a, _real=real, _name=name, **kw):
            calls[_name] = calls.get(_name, 0) + 1
            return _real(*a, **kw)
        monkeypatch.setattr(F, name, counted)
    return calls


def _no_grad_forward(model, batch):
    was = model.training
    model.eval()
    try:
        with torch.no_grad():
            y = model(batch)
    finally:
        model.train(was)
    torch.cuda.synchronize()
    return y


def _assert_equals_cold_twin(model, make, batch, device, calls, route, what):
    calls.clear()
    y = _no_grad_forward(model, batch)
    for name in route:
        assert calls.get(name, 0) > 0, f"{what}: the forward did not take the cached route ({name} not called): {calls}"
    twin = make().to(device)
    twin.load_state_dict(model.state_dict())
    y_twin = _no_grad_forward(twin, batch)
    assert torch.equal(y, y_twin), f"{what}: max |diff| {(y.float() - y_twin.float()).abs().max().item()}"


@pytest.mark.parametrize("name", list(ROUTE))
def test_no_grad_forward_after_replays_equals_a_cold_twin(device, monkeypatch, name):
    """capture; a no-grad forward (builds the caches); two replays on new batches; a no-grad forward == cold twin; and once more
    (a cache stored under the key it had after the capture is caught by the second round)."""
    from predict_pv_yield_amd.graphs import GraphedTrainStep
    from predict_pv_yield_amd.optim import HipAdam
    make, batch, lr = _case(name, device)
    calls = _count_copy_getters(monkeypatch)
    torch.manual_seed(3)
    model = make().to(device)
    opt = HipAdam(model.parameters(), lr=lr, capturable=True)
    batches = [batch(s) for s in range(6)]
    step = GraphedTrainStep(model, opt, batches[0], warmup=2)
    try:
        _assert_equals_cold_twin(model, make, batches[5], device, calls, ROUTE[name], "after the capture")
        if name == "conv3d-fp32":
            assert sum(getattr(p, "_pv_split2", None) is not None for p in model.parameters()) >= 3
        for r in range(2):
            step(batches[1 + 2 * r])
            step(batches[2 + 2 * r])
            _assert_equals_cold_twin(model, make, batches[5], device, calls, ROUTE[name], f"after replay round {r + 1}")
    finally:
        step.close()


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_load_state_dict_between_replays(device, monkeypatch, precision):
    """capture; replay; snapshot model + optimiser; two more replays; load the snapshot into both; replay on batch b.  Loss and
    parameters equal, bit for bit, those of an eager capturable-HipAdam twin that loaded the same snapshot and stepped on b
    (eager capturable steps and replays agree bitwise: test_gpu_training.py::test_hip_graph_train_step_matches_eager); then a
    no-grad forward equals a cold twin.  bf16: the graph's own packed conv images and fc1 shadow must follow the load."""
    from predict_pv_yield_amd.graphs import GraphedTrainStep
    from predict_pv_yield_amd.optim import HipAdam
    name = f"conv3d-{precision}"
    make, batch, lr = _case(name, device)
    calls = _count_copy_getters(monkeypatch)
    torch.manual_seed(7)
    model = make().to(device)
    opt = HipAdam(model.parameters(), lr=lr, capturable=True)
    batches = [batch(10 + s) for s in range(6)]
    step = GraphedTrainStep(model, opt, batches[0], warmup=2)
    try:
        step(batches[1])
        torch.cuda.synchronize()
        snap_model = {k: v.detach().clone() for k, v in model.state_dict().items()}
        snap_opt = copy.deepcopy(opt.state_dict())
        step(batches[2])
        step(batches[3])
        model.load_state_dict(snap_model)
        opt.load_state_dict(copy.deepcopy(snap_opt))
        loss = float(step(batches[4]))
        torch.cuda.synchronize()

        twin = make().to(device)
        twin.load_state_dict(snap_model)
        twin_opt = HipAdam(twin.parameters(), lr=lr, capturable=True)
        twin_opt.load_state_dict(copy.deepcopy(snap_opt))
        twin_opt.zero_grad(set_to_none=True)
        twin_loss = twin.training_step(batches[4], 0)
        twin_loss.backward()
        twin_opt.step()
        torch.cuda.synchronize()
        twin_loss = float(twin_loss.detach())
        assert loss == twin_loss, (loss, twin_loss)
        for (k, p), q in zip(model.named_parameters(), twin.parameters()):
            assert torch.equal(p, q), k
        assert opt.device_step() == twin_opt.device_step() == 4          # 2 warm-up steps, 1 replay; the reloaded one

        _assert_equals_cold_twin(model, make, batches[5], device, calls, ROUTE[name], "after the load and a replay")
    finally:
        step.close()


def test_trainer_in_graph_mode_validates_with_current_fp32_weights(device, monkeypatch, tmp_path):
    """Trainer(hip_graph=True) on the fp32 Conv3D model (half-float conv form), with a validation loader and two epochs: the
    validation metrics and parameters of the eager Trainer, bit for bit.  Both runs step a capturable HipAdam (the graph
    Trainer's twin): the host-scalar Adam differs from it by float rounding (test_hip_graph_train_step_matches_eager)."""
    from predict_pv_yield_amd import lightning as pl
    from predict_pv_yield_amd.graphs import GraphedTrainStep
    from predict_pv_yield_amd.models.conv3d.model import Model
    from predict_pv_yield_amd.optim import HipAdam
    monkeypatch.chdir(tmp_path)
    replays = [0]
    real_call, real_split2 = GraphedTrainStep.__call__, F.split2_conv_weight

    def counted_call(self, b):
        replays[0] += 1
        return real_call(self, b)
    monkeypatch.setattr(GraphedTrainStep, "__call__", counted_call)
    _, batch, _ = _case("conv3d-fp32", device)
    train = [batch(20 + s) for s in range(5)]       # 3 eager steps, the capture, then replays: every epoch after the first
    val = [batch(40 + s) for s in range(2)]
    results = []
    for graph in (False, True):
        torch.manual_seed(33)
        model = Model(**CONV3D_KW, precision="fp32")
        model.configure_optimizers = lambda m=model: HipAdam(m.parameters(), lr=5e-4, capturable=True)
        eval_split2, replays[0] = [0], 0

        def counted_split2(w, _m=model):
            if not _m.training:
                eval_split2[0] += 1
            return real_split2(w)
        monkeypatch.setattr(F, "split2_conv_weight", counted_split2)
        trainer = pl.Trainer(gpus=1, max_epochs=2, hip_graph=graph, log_every_n_steps=1)
        trainer.fit(model, train, val)
        torch.cuda.synchronize()
        assert trainer.current_epoch == 2
        assert eval_split2[0] > 0, "validation did not run the half-float conv form"
        assert replays[0] == (7 if graph else 0), replays[0]      # graph: the capture's step and every later one replay
        results.append(({k: v.detach().clone() for k, v in model.state_dict().items()}, dict(trainer.callback_metrics)))
    (p0, m0), (p1, m1) = results
    assert any("Validation" in k for k in m0), sorted(m0)
    assert m0.keys() == m1.keys()
    bad = {k: (m0[k], m1[k]) for k in m0 if not m0[k] == m1[k]}
    assert not bad, bad
    for k in p0:
        assert torch.equal(p0[k], p1[k]), k
