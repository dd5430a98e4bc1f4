"""GPU: the experiment-002 and notebook-16 Conv2d entry points agree bit for bit where both accept a shape.

Both families run the one tiled forward-like kernel of csrc/conv2d_tile_f32.h, under different tile planners: experiment
002 takes full-width bands of rows, notebook 16 tiles of at most 64 columns.  An output element's sum depends only on the
(tap, channel group) order, never on the tile it falls in, so the forward and the data gradient must give the same bits
under either planner.  (The weight gradients sum positions in tile order and differ by design; they are held to float64 in
test_gpu_exp002.py / test_gpu_nb16.py.)

Shapes (n, h, w): one output position; ragged last row bands; the model's own; and w_out = 78, which notebook 16 splits
into two column bands of 39 while experiment 002 keeps one band -- the seam where the two tilings really differ.  All stay
at most 96 wide and below 32 768 output positions, so neither family leaves for the general Conv3d kernel.
"""
import pytest
import torch

from conv2d_f32_helpers import _ops

pytestmark = pytest.mark.gpu

SHAPES = [(1, 3, 3), (3, 7, 11), (3, 13, 13), (32, 30, 30), (1, 5, 80), (2, 9, 80)]


@pytest.mark.parametrize("n,h,w", SHAPES)
def test_exp002_and_nb16_entry_points_agree_bitwise(device, n, h, w):
    K = _ops()
    g = torch.Generator().manual_seed(n * 10000 + h * 100 + w)
    x = torch.randn(n, 32, h, w, generator=g).relu().to(device)
    wt = (torch.randn(32, 32, 3, 3, generator=g) / 17.0).to(device)
    b = (torch.randn(32, generator=g) * 0.1).to(device)
    dy = torch.randn(n, 32, h - 2, w - 2, generator=g).to(device)
    gate = torch.randn(n, 32, h - 2, w - 2, generator=g).relu().to(device)

    for relu in (False, True):
        y = K.conv2d_fwd_f32(x, wt, b, relu=relu)
        y_ae = K.conv2d_ae_fwd_f32(x, wt, b, relu=relu)
        assert torch.equal(y, y_ae), f"forward relu={relu}: {int((y != y_ae).sum())} elements differ"
    for dy_gate in (gate, None):
        for x_gate in (x, None):
            dx = K.conv2d_bwd_data_f32(dy, dy_gate, wt, x_gate, tuple(x.shape))
            dx_ae = K.conv2d_ae_bwd_data_f32(dy, dy_gate, wt, x_gate, tuple(x.shape))
            assert torch.equal(dx, dx_ae), (f"dgrad dy_gate={dy_gate is not None} x_gate={x_gate is not None}: "
                                            f"{int((dx != dx_ae).sum())} elements differ")
