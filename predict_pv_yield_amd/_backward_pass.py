"""What one autograd node's backward leaves for another node of the SAME backward pass: the producer of a
gradient applies a gate, measures a maximum or finishes a split while it has the data in registers, and the consumer looks the
by-product up by the tensor it receives."""
import torch


class PassTable:
    """Values keyed by a tensor's storage, (data_ptr, numel), that live for one backward pass: the first access from another pass
    (another torch._C._current_graph_task_id()) empties the table and counts in `passes`.  Outside a backward pass (task id < 0)
    nothing is stored and nothing is found.
    hold: the entry keeps the keyed tensor itself until it is taken or the pass changes, so the caching allocator cannot hand
    "its" address to a later tensor of the same pass, which would then find a stale entry.  An entry nobody consumes keeps one
    tensor alive until the next pass touches the table.  hold=False is for keys that all exist before the pass starts and outlive
    it (forward activations): they coexist, so they cannot alias, and holding them would only delay their release."""

    def __init__(self):
        self._entries, self._task, self.passes = {}, -1, 0

    def _in_pass(self) -> bool:
        task = torch._C._current_graph_task_id()
        if task < 0:
            return False
        if task != self._task:
            self._entries.clear()
            self._task = task
            self.passes += 1
        return True

    def put(self, t: torch.Tensor, value, hold: bool = True) -> None:
        if self._in_pass():
            self._entries[(t.data_ptr(), t.numel())] = (value, t if hold else None)

    def get(self, t: torch.Tensor):
        hit = self._entries.get((t.data_ptr(), t.numel())) if self._in_pass() else None
        return hit[0] if hit is not None else None

    def take(self, t: torch.Tensor):
        hit = self._entries.pop((t.data_ptr(), t.numel()), None) if self._in_pass() else None
        return hit[0] if hit is not None else None

    def drop(self, t: torch.Tensor) -> None:
        self._entries.pop((t.data_ptr(), t.numel()), None)

    def __len__(self) -> int:
        return len(self._entries)
