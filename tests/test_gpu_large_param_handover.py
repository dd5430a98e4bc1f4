"""GPU: every single-process kind of parked fc1 gradient (predict_pv_yield_amd/_large_param.py) goes from its
producer in functional.py through HipAdam.step() into exactly the update kernel it names.  One Linear weight of 128 x 256 (two
moment tiles), a batch of 4, two optimiser steps.  The twin is a set of plain tensors updated by calling the same hip_ops
function with the same operands and step number, so every comparison is the same kernel on the same inputs: bit-equal."""

import pytest
import torch

from predict_pv_yield_amd import _large_param as L
from predict_pv_yield_amd._large_param import large_of

pytestmark = pytest.mark.gpu
N, KDIM, B, ROWS = 128, 256, 4, (0, 64)
HP = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
KINDS = (L.OPERANDS_BF16, L.PAIR_F32, L.GRAD_BF16, L.GRAD_SHARD)


def _setup(kind, device, monkeypatch):
    """(weight, optimiser, forward) with the optimiser in the mode, and the switches set, that make backward park `kind`."""
    from predict_pv_yield_amd import distributed as D
    from predict_pv_yield_amd import functional as F
    from predict_pv_yield_amd import optim
    monkeypatch.setattr(optim.HipAdam, "FUSE_MIN_NUMEL", 1)
    monkeypatch.setattr(optim, "FUSE_DX_INTO_UPDATE", False)        # "fused" without the one-pass backward: the operands are parked
    monkeypatch.setattr(F, "LINEAR_F32_GEMM_K", KDIM)               # LinearF32's fc1-sized branch at this width
    g = torch.Generator(device="cpu").manual_seed(11)
    w = torch.nn.Parameter((torch.randn(N, KDIM, generator=g) * 0.05).to(device))
    opt = optim.HipAdam([w], **HP)
    opt.grad_scale = 0.5
    assert large_of(w).mode == "fused"
    if kind == L.GRAD_BF16:
        opt.set_large_grad_mode("bf16")
    elif kind == L.GRAD_SHARD:
        # one rank of a sharded job on one device, as bench.py emulates it: the row range fixed, the exchange left out, the
        # hand-over installed through the two attributes that stay on the parameter
        monkeypatch.setattr(D, "row_shard", lambda n_rows, rank=None, world=None: ROWS)
        monkeypatch.setattr(D, "all_gather_rows", lambda full, async_op=True: None)
        opt.set_large_grad_mode("sharded")
        assert opt.large_grad_mode == "sharded"
        w._pv_on_grad = lambda gb, param=None: setattr(param, "_pv_grad_shard", gb[ROWS[0]:ROWS[1]])

    def forward(x):
        if kind == L.PAIR_F32:
            return F.linear_f32(x, w, None, relu=True)
        return F.linear_bf16(x.to(torch.bfloat16), w, None, relu=True)
    return w, opt, forward


def _parked(w, kind):
    """The payload of `kind` parked on w (asserting it is there, and nothing else is)."""
    rec, shard = large_of(w), getattr(w, "_pv_grad_shard", None)
    if kind == L.GRAD_SHARD:
        assert rec.parked is None and shard is not None and shard.dtype == torch.bfloat16
        return shard
    assert shard is None and rec.parked is not None and rec.parked[0] == kind
    return rec.parked[1]


class _Twin:
    """p, exp_avg, exp_avg_sq (and the bf16 operand copy, where the kind keeps one) as plain tensors."""

    def __init__(self, w, kind):
        from predict_pv_yield_amd import hip_ops as K
        self.p = w.detach().clone()
        self.m, self.v = torch.zeros_like(self.p), torch.zeros_like(self.p)
        self.shadow = None if kind == L.PAIR_F32 else K.cast_f32_to_bf16(self.p)

    def apply(self, kind, payload, step, grad_scale):
        from predict_pv_yield_amd import hip_ops as K
        if kind == L.OPERANDS_BF16:
            K.linear_wgrad_adam_bf16(*payload, self.p, self.m, self.v, self.shadow, step, **HP)
        elif kind == L.PAIR_F32:
            K.linear_wgrad_adam_f32(*payload, None, self.p, self.m, self.v, step, **HP)
        elif kind == L.GRAD_BF16:
            K.adam_step_bf16grad(self.p, payload, self.m, self.v, step, **HP, bf16_shadow=self.shadow, grad_scale=grad_scale)
        else:
            r0, r1 = ROWS
            K.adam_step_bf16grad(self.p[r0:r1], payload, self.m[r0:r1], self.v[r0:r1], step, **HP,
                                 bf16_shadow=self.shadow[r0:r1], grad_scale=grad_scale)

    def apply_grad(self, grad, step, grad_scale):
        from predict_pv_yield_amd import hip_ops as K
        K.adam_step_multi([(self.p, grad, self.m, self.v, self.shadow)], step, **HP, grad_scale=grad_scale)

    def assert_equal(self, w, opt):
        from predict_pv_yield_amd.functional import bf16_shadow_of
        m, v = opt.moments(w)
        assert torch.equal(w.detach(), self.p) and torch.equal(m, self.m) and torch.equal(v, self.v)
        assert int(opt.state[w]["step"].item()) == self.steps
        if self.shadow is not None:
            assert torch.equal(bf16_shadow_of(w), self.shadow)


def _backward(forward, device, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x, dy = torch.randn(B, KDIM, generator=g).to(device), torch.randn(B, N, generator=g).to(device)
    forward(x).backward(dy)


@pytest.mark.parametrize("kind", KINDS)
def test_step_takes_the_parked_entry_and_applies_exactly_its_update_kernel(kind, device, monkeypatch):
    w, opt, forward = _setup(kind, device, monkeypatch)
    twin, w0 = _Twin(w, kind), w.detach().clone()
    for step in (1, 2):
        opt.zero_grad()
        _backward(forward, device, seed=step)
        assert w.grad is None
        payload = _parked(w, kind)
        twin.apply(kind, payload, step, opt.grad_scale)
        twin.steps = step
        opt.step()
        assert large_of(w).parked is None and getattr(w, "_pv_grad_shard", None) is None and w.grad is None
        assert not large_of(w).applied
        twin.assert_equal(w, opt)
    assert not torch.equal(w.detach(), w0)                  # (the updates moved the weights)


@pytest.mark.parametrize("kind", KINDS)
def test_with_a_grad_present_step_takes_the_plain_path_and_the_parked_entry_stays(kind, device, monkeypatch):
    w, opt, forward = _setup(kind, device, monkeypatch)
    twin = _Twin(w, kind)
    opt.zero_grad()
    _backward(forward, device, seed=1)
    payload = _parked(w, kind)
    grad = torch.randn(N, KDIM, generator=torch.Generator(device="cpu").manual_seed(5)).to(device)
    w.grad = grad.clone()
    twin.apply_grad(grad, 1, opt.grad_scale)
    twin.steps = 1
    opt.step()
    assert _parked(w, kind) is payload and torch.equal(w.grad, grad)
    twin.assert_equal(w, opt)
    opt.zero_grad()                                         # ... until zero_grad()
    assert large_of(w).parked is None and getattr(w, "_pv_grad_shard", None) is None and w.grad is None
