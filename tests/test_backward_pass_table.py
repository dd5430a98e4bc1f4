"""CPU: the lifetime rule of what one backward node leaves for another (predict_pv_yield_amd/_backward_pass.py, DESIGN.md
§3.5b), on the table itself and through the helpers of functional.py / perceiver_functional.py that sit on it.  A backward
pass here is a chain of tiny autograd.Functions on a CPU tensor, each of which calls one Python function from its backward."""
import gc
import weakref

import pytest
import torch

from predict_pv_yield_amd import functional as F
from predict_pv_yield_amd import perceiver_functional as PF
from predict_pv_yield_amd._backward_pass import PassTable


class _Node(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, fn):
        ctx.fn = fn
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        ctx.fn()
        return g, None


def backward_pass(*fns):
    """One backward pass whose nodes call fns in the given order, one node each."""
    y = torch.ones(2, requires_grad=True)
    for fn in reversed(fns):
        y = _Node.apply(y, fn)
    y.sum().backward()


def test_backward_pass_runs_its_nodes_in_order_under_one_task_id():
    seen = []
    backward_pass(*[lambda i=i: seen.append((i, torch._C._current_graph_task_id())) for i in range(3)])
    assert [i for i, _ in seen] == [0, 1, 2]
    assert len({task for _, task in seen}) == 1 and seen[0][1] >= 0
    assert torch._C._current_graph_task_id() < 0


# ---- the table -------------------------------------------------------------------------------------------------------------
def test_put_in_one_node_is_taken_once_by_another_node_of_the_pass():
    table, t, got = PassTable(), torch.zeros(4), []
    backward_pass(lambda: table.put(t, "v"), lambda: got.append(table.take(t)), lambda: got.append(table.take(t)))
    assert got == ["v", None] and len(table) == 0 and not table


def test_get_leaves_the_entry_and_drop_removes_it():
    table, t, got = PassTable(), torch.zeros(4), []

    def node():
        table.put(t, "v")
        got.append((table.get(t), table.get(t), len(table), bool(table)))
        table.drop(t)
        got.append((table.get(t), len(table), bool(table)))
        table.drop(t)                                      # (nothing there: no error)
    backward_pass(node)
    assert got == [("v", "v", 1, True), (None, 0, False)]


@pytest.mark.parametrize("access", ["put", "take", "get"])
def test_an_unconsumed_entry_is_invisible_in_the_next_pass(access):
    table, t, other, got = PassTable(), torch.zeros(4), torch.zeros(3), []
    backward_pass(lambda: table.put(t, "v"))
    assert len(table) == 1 and table.passes == 1           # (nobody consumed it)

    def first_access_of_pass_2():
        if access == "put":
            table.put(other, "w")
        else:
            getattr(table, access)(other)
        got.append(len(table))
        got.append(table.take(t))
    backward_pass(first_access_of_pass_2, lambda: got.append(table.passes))
    assert got == [1 if access == "put" else 0, None, 2]
    assert table.passes == 2


def test_outside_a_backward_pass_nothing_is_stored_or_found():
    table, t, got = PassTable(), torch.zeros(4), []
    table.put(t, "v")
    assert len(table) == 0 and table.take(t) is None and table.get(t) is None and table.passes == 0
    backward_pass(lambda: table.put(t, "v"))
    assert table.take(t) is None and table.get(t) is None  # a live entry, asked for from outside its pass
    backward_pass(lambda: got.append(table.take(t)))
    assert got == [None]


def test_a_view_of_the_same_address_with_another_element_count_does_not_hit():
    table, t, got = PassTable(), torch.zeros(4), []
    assert t[:2].data_ptr() == t.data_ptr()
    backward_pass(lambda: table.put(t, "v"),
                  lambda: got.extend([table.get(t[:2]), table.take(t[:2]), table.take(t.view(2, 2))]))
    assert got == [None, None, "v"]


def test_hold_keeps_the_keyed_tensor_until_the_entry_is_taken():
    table, refs, got = PassTable(), [], []

    def producer():
        t = torch.zeros(4)
        refs.append(weakref.ref(t))
        table.put(t, "v")
        del t
        got.append(refs[0]() is not None)

    def consumer():
        got.append(refs[0]() is not None)
        got.append(table.take(refs[0]()))
        got.append(refs[0]() is None)
    backward_pass(producer, consumer)
    assert got == [True, True, "v", True]


def test_hold_keeps_the_keyed_tensor_until_the_pass_changes():
    table, refs, got = PassTable(), [], []

    def producer():
        t = torch.zeros(4)
        refs.append(weakref.ref(t))
        table.put(t, "v")
    backward_pass(producer)
    gc.collect()
    assert refs[0]() is not None and len(table) == 1       # between the passes: still held
    backward_pass(lambda: got.append(table.get(torch.zeros(1))), lambda: got.append(refs[0]() is None))
    assert got == [None, True]


def test_without_hold_the_keyed_tensor_is_released_at_once():
    table, got = PassTable(), []

    def producer():
        t = torch.zeros(4)
        ref = weakref.ref(t)
        table.put(t, "v", hold=False)
        got.append(table.get(t))
        del t
        got.append(ref() is None)
    backward_pass(producer)
    assert got == ["v", True]


def test_each_table_has_its_own_pass_marker():
    a, b, t = PassTable(), PassTable(), torch.zeros(4)
    backward_pass(lambda: a.put(t, 1), lambda: b.put(t, 2))
    backward_pass(lambda: a.get(t))
    assert (a.passes, b.passes) == (2, 1) and len(a) == 0 and len(b) == 1


# ---- pre-gated dx (functional.py) --------------------------------------------------------------------------------------------
def test_a_pregated_mark_is_consumed_once():
    t, got = torch.zeros(4), []
    backward_pass(lambda: F._mark_pregated(t), lambda: got.append(F._take_pregated(t)), lambda: got.append(F._take_pregated(t)))
    assert got == [True, False]


def test_a_pregated_mark_of_one_backward_is_not_honoured_in_the_next():
    t, got = torch.zeros(4), []
    backward_pass(lambda: F._mark_pregated(t))
    backward_pass(lambda: got.append(F._take_pregated(t)))
    assert got == [False]


def test_a_pregated_mark_outside_a_backward_is_never_honoured():
    t, got = torch.zeros(4), []
    F._mark_pregated(t)
    assert F._take_pregated(t) is False
    F._mark_pregated(t)
    backward_pass(lambda: got.append(F._take_pregated(t)))
    assert got == [False]
    backward_pass(lambda: F._mark_pregated(t))
    assert F._take_pregated(t) is False                    # marked inside a pass, asked for outside it


def test_a_pregated_mark_is_not_honoured_for_another_element_count():
    t, got = torch.zeros(4), []
    backward_pass(lambda: F._mark_pregated(t), lambda: got.extend([F._take_pregated(t[:2]), F._take_pregated(t)]))
    assert got == [False, True]


def test_a_pregated_tensor_stays_alive_while_it_is_marked():
    refs, got = [], []

    def producer():
        t = torch.zeros(4)
        refs.append(weakref.ref(t))
        F._mark_pregated(t)

    def consumer():
        got.append(refs[0]() is not None)
        got.append(F._take_pregated(refs[0]()))
        got.append(refs[0]() is None)
    backward_pass(producer, consumer)
    assert got == [True, True, True]


# ---- gradients of tied weights (perceiver_functional.py) -------------------------------------------------------------------
def _param():
    return torch.nn.Parameter(torch.zeros(3))


def test_a_parameter_applied_three_times_keeps_its_first_gradient_until_the_third_arrives():
    p, buf, got = _param(), torch.zeros(3), []
    for _ in range(3):
        PF._note_use(p)
    assert p._pv_uses == 3

    def first():
        key, acc = PF._tied_slot(p)
        got.append((key is not None, acc))
        PF._tied_keep(key, buf)
        got.append(len(PF._TIED))

    def later():
        key, acc = PF._tied_slot(p)
        got.append((key is not None, acc is buf))
    backward_pass(first, later, later, lambda: got.append((len(PF._TIED), bool(PF._TIED), p._pv_uses)))
    assert got == [(True, None), 1, (True, True), (True, True), (0, False, 0)]


def test_a_parameter_applied_once_registers_nothing():
    p, got = _param(), []
    PF._note_use(p)
    backward_pass(lambda: got.append(PF._tied_slot(p)))
    assert got == [(None, None)] and not PF._TIED and p._pv_uses == 0
    PF._tied_keep(None, torch.zeros(3))                    # what the call sites do with that key: nothing
    assert not PF._TIED


def test_a_tied_slot_outside_a_backward_is_empty():
    p = _param()
    PF._note_use(p)
    PF._note_use(p)
    assert PF._tied_slot(p) == (None, None) and p._pv_uses == 2


def test_uses_noted_under_no_grad_or_of_a_frozen_parameter_do_not_count():
    p, frozen = _param(), torch.nn.Parameter(torch.zeros(3), requires_grad=False)
    with torch.no_grad():
        for _ in range(3):
            PF._note_use(p)
    PF._note_use(frozen)
    PF._note_use(None)
    assert getattr(p, "_pv_uses", 0) == 0 and getattr(frozen, "_pv_uses", 0) == 0


def test_counts_of_a_graph_that_was_never_backpropagated_are_dropped_after_a_later_backward():
    p, q, got = _param(), _param(), []
    PF._note_use(p)
    PF._note_use(p)                                        # a forward whose graph is thrown away
    PF._note_use(q)
    backward_pass(lambda: PF._tied_slot(q))                # a later backward pass that uses tied-gradient slots
    PF._note_use(p)                                        # the next forward applies p once
    assert p._pv_uses == 1
    backward_pass(lambda: got.append(PF._tied_slot(p)))
    assert got == [(None, None)] and p._pv_uses == 0 and not PF._TIED


def test_tied_gradients_switched_off(monkeypatch):
    p, got = _param(), []
    PF._note_use(p)
    PF._note_use(p)
    monkeypatch.setattr(PF, "ACCUMULATE_TIED_GRADS", False)
    backward_pass(lambda: got.append(PF._tied_slot(p)))
    assert got == [(None, None)] and p._pv_uses == 2


# ---- gradient of a shared activation (perceiver_functional.py) -------------------------------------------------------------
def test_only_a_tensor_tagged_shared_gets_a_slot():
    plain, shared, got = torch.zeros(4), PF.mark_shared(torch.zeros(4)), []
    backward_pass(lambda: got.append(PF._shared_activation_slot(plain)),
                  lambda: got.append(PF._shared_activation_slot(shared)))
    assert got[0] == (None, None)
    assert got[1][0] is not None and got[1][1] is None
    assert PF._shared_activation_slot(shared) == (None, None)      # outside a backward pass


def test_the_first_arrival_of_a_shared_activations_gradient_serves_the_pass_and_not_the_next():
    kv, dkv, got = PF.mark_shared(torch.zeros(4)), torch.zeros(4), []

    def first():
        key, acc = PF._shared_activation_slot(kv)
        got.append(acc)
        PF._SHARED_ACT.put(key, dkv, hold=False)           # as AttentionF32.backward does

    def later():
        got.append(PF._shared_activation_slot(kv)[1] is dkv)
    backward_pass(first, later, later)
    assert got == [None, True, True]
    del got[:]
    backward_pass(lambda: got.append(PF._shared_activation_slot(kv)[1]))
    assert got == [None]
