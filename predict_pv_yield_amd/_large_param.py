"""What HipAdam and the autograd glue share about ONE large matrix (fc1's weight), as one record stored on the parameter
(DESIGN.md §3.5c).  A parameter without a record is nobody's large matrix and behaves as mode "autograd".  Two hand-overs stay
attributes of the parameter itself, because code outside the package installs them there: the gradient-sync callback that
functional.LinearBF16.backward calls, and the rows of the summed gradient that this callback leaves for step()."""
MODES = ("fused", "bf16", "sharded", "ksharded", "autograd")
# Kinds of parked work.  A mode reaches exactly one producer, so ONE slot (`parked`: None or (kind, payload)) holds them all.
OPERANDS_BF16 = "operands_bf16"     # (x, dy, y)       LinearBF16, "fused" where no one-pass form covers the shape
PAIR_F32 = "pair_f32"               # (x, g)           LinearF32, "fused"
PAIR_KSHARD = "pair_kshard"         # (x_cols, g_all)  LinearBF16KSharded, "ksharded" where no one-pass form covers the shape
GRAD_BF16 = "grad_bf16"             # bf16 gradient    LinearBF16, "bf16", and "sharded" with nothing to scatter
GRAD_SHARD = "grad_shard"           # this rank's rows of the summed bf16 gradient: on the parameter, never in the slot


class LargeParam:
    __slots__ = ("mode", "parked", "applied", "takes_f32_pending", "kshard", "shadow_work",
                 "fused_backward", "eager_update", "kshard_backward")

    def __init__(self):
        self.mode, self.parked, self.takes_f32_pending = "autograd", None, False
        self.applied = False        # True from a one-pass backward (which has updated the matrix) until step()
        self.kshard = None          # "ksharded": this rank's column shard (HipAdam._make_column_shard): optimiser state
        self.shadow_work = None     # "sharded": the all-gather of the bf16 operand rows; functional.bf16_shadow_of waits for it
        self.fused_backward = self.eager_update = self.kshard_backward = None      # HipAdam's in-backward entry points


def large_of(p):
    """p's record, or None when no HipAdam owns p as a large matrix."""
    return getattr(p, "_pv_large", None)


def clear_parked(p) -> None:
    """Drops what a backward() left on p for a step() that never came: the slot and the gradient shard.  Not `applied` (only
    step() and a mode switch clear it: a second backward() must still raise) and not `shadow_work`."""
    if large_of(p) is not None:
        p._pv_large.parked = None
    if getattr(p, "_pv_grad_shard", None) is not None:
        p._pv_grad_shard = None


def reset(p, mode, takes_f32_pending=False) -> LargeParam:
    """A mode switch on p's record (created here if p has none): nothing parked, no update applied, no entry point installed.
    `kshard` and `shadow_work` stay."""
    if large_of(p) is None:
        p._pv_large = LargeParam()
    clear_parked(p)
    rec = p._pv_large
    rec.mode, rec.applied, rec.takes_f32_pending = mode, False, takes_f32_pending
    rec.fused_backward = rec.eager_update = rec.kshard_backward = None
    return rec
