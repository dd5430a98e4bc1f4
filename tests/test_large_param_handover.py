"""CPU: the one record per large matrix through which fc1's gradient reaches HipAdam (predict_pv_yield_amd/_large_param.py,
DESIGN.md §3.5c) -- the record itself, and what HipAdam, functional.LinearF32 and distributed.negotiate_grad_sync do to it.
No kernel runs: the optimiser is built on a CPU nn.Linear(8, 4) and never stepped."""
import types

import pytest
import torch
from torch import nn

from predict_pv_yield_amd import _large_param as L
from predict_pv_yield_amd import distributed as D
from predict_pv_yield_amd import functional as F
from predict_pv_yield_amd._large_param import LargeParam, clear_parked, large_of
from predict_pv_yield_amd.optim import HipAdam

SLOT_KINDS = (L.OPERANDS_BF16, L.PAIR_F32, L.PAIR_KSHARD, L.GRAD_BF16)      # (L.GRAD_SHARD travels in `_pv_grad_shard`)
ENTRY_POINTS = ("fused_backward", "eager_update", "kshard_backward")


@pytest.fixture
def lin(monkeypatch):
    monkeypatch.setattr(HipAdam, "FUSE_MIN_NUMEL", 1)
    return nn.Linear(8, 4)


def _park_everything(w, kind):
    """Something of `kind` parked on w, an applied mark and an operand all-gather in flight: every state a backward leaves."""
    rec = large_of(w)
    if kind == L.GRAD_SHARD:
        w._pv_grad_shard = torch.zeros(2, 8)
    else:
        rec.parked = (kind, (torch.zeros(1),))
    rec.applied, rec.shadow_work = True, "gather"


def _parked(w):
    return large_of(w).parked, getattr(w, "_pv_grad_shard", None)


# ---- the record ------------------------------------------------------------------------------------------------------------
def test_a_fresh_record_is_mode_autograd_with_nothing_parked():
    rec = LargeParam()
    assert (rec.mode, rec.parked, rec.applied, rec.takes_f32_pending, rec.kshard, rec.shadow_work) == \
        ("autograd", None, False, False, None, None)
    assert [getattr(rec, name) for name in ENTRY_POINTS] == [None] * 3
    with pytest.raises(AttributeError):
        rec.pending = 1                                     # a misspelt field fails loudly


def test_park_take_and_clear():
    w, payload = nn.Parameter(torch.zeros(4, 8)), (torch.zeros(3, 8), torch.zeros(3, 4))
    rec = w._pv_large = LargeParam()
    rec.mode, rec.takes_f32_pending = "fused", True
    rec.parked = (L.PAIR_F32, payload)
    # the one taker outside step(): a second LinearF32.backward takes the pair back (and only that kind), emptying the slot
    with pytest.MonkeyPatch.context() as mp:
        _linear_f32_backward(mp, w, torch.zeros(3, 8), torch.zeros(3, 4))
    assert rec.parked is None and w.grad is not None
    rec.parked = (L.OPERANDS_BF16, payload)
    with pytest.MonkeyPatch.context() as mp:
        _linear_f32_backward(mp, w, torch.zeros(3, 8), torch.zeros(3, 4))
    assert rec.parked == (L.OPERANDS_BF16, payload)         # another kind: left alone
    rec.applied, rec.shadow_work, w._pv_grad_shard = True, "gather", payload[1]
    clear_parked(w)
    assert _parked(w) == (None, None) and rec.applied and rec.shadow_work == "gather"


def test_reset_creates_the_record_empties_the_slot_and_removes_the_entry_points():
    w, fn = nn.Parameter(torch.zeros(4, 8)), lambda: None
    rec = L.reset(w, "bf16")
    assert rec is large_of(w) and isinstance(rec, LargeParam) and rec.mode == "bf16"
    rec.parked, w._pv_grad_shard = (L.GRAD_BF16, torch.zeros(1)), torch.zeros(1)
    rec.applied, rec.kshard, rec.shadow_work, rec.eager_update = True, {"k0": 0}, "gather", fn
    assert L.reset(w, "fused", takes_f32_pending=True) is rec
    assert (rec.mode, rec.applied, rec.takes_f32_pending) == ("fused", False, True) and _parked(w) == (None, None)
    assert [getattr(rec, name) for name in ENTRY_POINTS] == [None] * 3
    assert rec.kshard == {"k0": 0} and rec.shadow_work == "gather"


def test_a_parameter_nobody_owns_has_no_record_and_every_reader_treats_it_as_autograd(monkeypatch):
    w = nn.Parameter(torch.zeros(4, 8))
    assert large_of(w) is None
    clear_parked(w)                                         # (nothing there: no error, no attribute created)
    assert not hasattr(w, "_pv_grad_shard") and large_of(w) is None
    # LinearF32.backward: an ordinary gradient
    assert _linear_f32_backward(monkeypatch, w, torch.zeros(2, 8), torch.ones(2, 4)).shape == w.shape and large_of(w) is None
    # bf16_shadow_of: nothing to wait for; the cached operand copy is returned as it is
    w._pv_bf16_shadow, w._pv_bf16_shadow_version = torch.zeros(4, 8, dtype=torch.bfloat16), w._version
    assert F.bf16_shadow_of(w) is w._pv_bf16_shadow
    # linear_bf16: the plain function, not the K-sharded one
    routed = []
    monkeypatch.setattr(F, "LinearBF16", types.SimpleNamespace(apply=lambda *a: routed.append("plain")))
    monkeypatch.setattr(F, "LinearBF16KSharded", types.SimpleNamespace(apply=lambda *a: routed.append("ksharded")))
    F.linear_bf16(torch.zeros(2, 8), w, None)
    assert routed == ["plain"]
    monkeypatch.undo()
    # LinearBF16.backward: asks the kernel for the f32 weight gradient and returns it to autograd; nothing is parked
    asked = {}
    monkeypatch.setattr(F.K, "linear_bwd_bf16", lambda x, wb, dy, y, **kw: asked.update(kw) or ("dx", "dw", "db"))
    ctx = types.SimpleNamespace(saved_tensors=(torch.zeros(2, 8), w._pv_bf16_shadow, None), needs_input_grad=(True, True, False),
                                has_bias=False, weight_param=w, x_is_relu_output=False)
    assert F.LinearBF16.backward(ctx, torch.ones(2, 4)) == ("dx", "dw", None, None, None)
    assert asked["need_dw"] is True and large_of(w) is None


# ---- HipAdam ---------------------------------------------------------------------------------------------------------------
def test_hipadam_creates_a_record_in_mode_fused(lin):
    opt = HipAdam(lin.parameters())
    rec = large_of(lin.weight)
    assert opt.large_params() == [lin.weight] and large_of(lin.bias) is None
    assert isinstance(rec, LargeParam) and rec.mode == opt.large_grad_mode == "fused" and rec.parked is None


@pytest.mark.parametrize("mode", ["fused", "bf16", "sharded", "ksharded", "autograd"])
@pytest.mark.parametrize("kind", SLOT_KINDS + (L.GRAD_SHARD,))
def test_a_mode_switch_resets_parked_work_and_applied(lin, mode, kind):
    opt, w = HipAdam(lin.parameters()), lin.weight
    w._pv_on_grad = callback = lambda g, param=None: None
    _park_everything(w, kind)
    opt.set_large_grad_mode(mode)
    rec = large_of(w)
    assert _parked(w) == (None, None) and rec.applied is False and rec.shadow_work == "gather"
    assert w._pv_on_grad is callback                        # an installed gradient-sync callback survives the switch
    # without a process group every rank count is 1: "ksharded" has nothing to shard over and lands on "sharded"
    assert rec.mode == opt.large_grad_mode == {"ksharded": "sharded"}.get(mode, mode) and rec.kshard is None


@pytest.mark.parametrize("capturable", [False, True])
@pytest.mark.parametrize("overlap", [False, True])
def test_each_mode_installs_exactly_its_entry_points(lin, overlap, capturable):
    opt = HipAdam(lin.parameters(), overlap_large_update=overlap, capturable=capturable)
    rec = large_of(lin.weight)
    for mode in ("fused", "bf16", "sharded", "ksharded", "autograd", "fused"):
        opt.set_large_grad_mode(mode)
        want = {"fused": ["eager_update" if overlap else "fused_backward"]}.get(mode, [])
        assert [name for name in ENTRY_POINTS if getattr(rec, name) is not None] == want
        assert all(callable(getattr(rec, name)) for name in want)
        assert rec.takes_f32_pending is (mode == "fused" and not capturable)
    opt.set_fuse_large_linear(False)
    assert rec.mode == "autograd" and not rec.takes_f32_pending


@pytest.mark.parametrize("kind", SLOT_KINDS + (L.GRAD_SHARD,))
def test_zero_grad_drops_parked_work_of_every_kind_and_keeps_applied_and_the_gather(lin, kind):
    opt, w = HipAdam(lin.parameters()), lin.weight
    _park_everything(w, kind)
    w.grad = torch.ones_like(w)
    opt.zero_grad()
    rec = large_of(w)
    assert _parked(w) == (None, None) and w.grad is None and rec.applied is True and rec.shadow_work == "gather"
    assert rec.mode == "fused" and rec.fused_backward is not None


def test_a_new_hipadam_forgets_the_previous_optimisers_column_shard(lin):
    HipAdam(lin.parameters())
    large_of(lin.weight).kshard = {"k0": 0, "k1": 8, "step": 7}
    HipAdam(lin.parameters())
    assert large_of(lin.weight).kshard is None


# ---- functional.LinearF32.backward -----------------------------------------------------------------------------------------
def _linear_f32_backward(monkeypatch, w, x, dy):
    """LinearF32.backward on CPU tensors: the fc1-sized branch (threshold lowered), K.gemm replaced by a torch product.  No dx,
    no bias, no ReLU, so gemm is the only kernel it calls."""
    monkeypatch.setattr(F, "LINEAR_F32_GEMM_K", 8)
    monkeypatch.setattr(F.K, "gemm", lambda a, b: a @ b)
    ctx = types.SimpleNamespace(saved_tensors=(x, w, None), needs_input_grad=(False, True, False, False), has_bias=False,
                                weight_param=w)
    return F.LinearF32.backward(ctx, dy)[1]


def test_linear_f32_backward_parks_converts_an_earlier_pair_or_computes_dw(lin, monkeypatch):
    opt, w = HipAdam(lin.parameters()), lin.weight
    x1, g1, x2, g2 = torch.randn(3, 8), torch.randn(3, 4), torch.randn(3, 8), torch.randn(3, 4)
    # fused and eligible: the pair is parked, no gradient is formed
    assert _linear_f32_backward(monkeypatch, w, x1, g1) is None
    kind, (px, pg) = large_of(w).parked
    assert kind == L.PAIR_F32 and px is x1 and torch.equal(pg, g1) and w.grad is None
    # a second backward before step(): the parked pair becomes .grad, this call returns its own dw for autograd to add
    dw2 = _linear_f32_backward(monkeypatch, w, x2, g2)
    assert large_of(w).parked is None and torch.equal(w.grad, g1.t() @ x1) and torch.equal(dw2, g2.t() @ x2)
    # ... and with a .grad in place a third one parks nothing
    assert torch.equal(_linear_f32_backward(monkeypatch, w, x1, g1), g1.t() @ x1) and large_of(w).parked is None
    # not eligible: another mode, a capturable optimiser, more rows than the kernel's LDS holds
    w.grad = None
    opt.set_large_grad_mode("autograd")
    assert torch.equal(_linear_f32_backward(monkeypatch, w, x1, g1), g1.t() @ x1) and large_of(w).parked is None
    HipAdam(lin.parameters(), capturable=True)
    assert large_of(w).mode == "fused"
    assert torch.equal(_linear_f32_backward(monkeypatch, w, x1, g1), g1.t() @ x1) and large_of(w).parked is None
    HipAdam(lin.parameters())
    monkeypatch.setattr(F, "F32_PENDING_MAX_ROWS", 2)
    assert torch.equal(_linear_f32_backward(monkeypatch, w, x1, g1), g1.t() @ x1) and large_of(w).parked is None


# ---- the cleanup after a failed trial step (distributed.negotiate_grad_sync) -----------------------------------------------
class _FailingTrial(nn.Module):
    """A model whose trial step leaves `kind` parked on its weight (plus an applied mark, a gather in flight and a bf16 operand
    copy) and then fails, as a step that raised half-way through backward would."""

    def __init__(self, lin, kind):
        super().__init__()
        self.lin, self.kind = lin, kind

    def training_step(self, batch, i):
        _park_everything(self.lin.weight, self.kind)
        self.lin.weight._pv_bf16_shadow = torch.zeros(4, 8, dtype=torch.bfloat16)
        raise RuntimeError("trial step failed")


@pytest.mark.parametrize("kind", SLOT_KINDS + (L.GRAD_SHARD,))
def test_the_cleanup_after_a_failed_trial_step_and_zero_grad_clear_the_same_parked_state(lin, kind, monkeypatch, tmp_path):
    opt, w = HipAdam(lin.parameters()), lin.weight
    _park_everything(w, kind)
    opt.zero_grad()
    after_zero_grad = _parked(w)
    monkeypatch.setenv("PV_DIST_SINGLE_RANK", "1")          # a one-rank gloo group counts as distributed: the real code path
    torch.distributed.init_process_group("gloo", init_method=f"file://{tmp_path}/store", rank=0, world_size=1)
    try:
        with pytest.raises(SystemExit, match="no gradient-exchange mode works"):
            D.negotiate_grad_sync(_FailingTrial(lin, kind), opt, None, "autograd")
    finally:
        torch.distributed.destroy_process_group()
    rec = large_of(w)
    assert _parked(w) == after_zero_grad == (None, None)
    assert rec.applied is True                              # (only step() and a mode switch clear it)
    assert rec.shadow_work is None and not hasattr(w, "_pv_bf16_shadow")
