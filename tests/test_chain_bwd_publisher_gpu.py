"""Chain backward (lstm_chain_bwd.hip): the publisher waves of the bottom H = 16 stage over input widths.

The four publisher waves share a [16][Din] dx tile in 64-element slices (wave pj takes slices pj, pj + 4,
...). The slice count of a wave and the LDS offsets of a lane's elements are computed once per launch, so the
widths below are those at which they differ (Din is the input width rounded up to 4, 16 Din the tile):

    din   Din   16 Din   slices of wave 0 / 1 / 2 / 3   256 % Din
     4     4      64     1 / 0 / 0 / 0                   0   three waves publish nothing
    12    12     192     1 / 1 / 1 / 0                   4   a lane's row and column carry between slices
    18    20     320     2 / 1 / 1 / 1                  16   the CML width: waves with different counts
    36    36     576     3 / 2 / 2 / 2                   4   KX = 2
    64    64    1024     4 / 4 / 4 / 4                   0   the widest tile the chain takes

Every case compares the chain with the per-layer kernels with the bounds of test_chain_bwd_steps_gpu.py
(output 1e-5, every gradient 5e-3 in relative norm; the input gradient is the publishers' output), asks for
three bitwise-equal launches, no spin timeout, the epoch counter advanced by 6, and a zero gradient in the
rows past M. T = 28 leaves an un-pooling tail; M = 40 is three row tiles with 8 padding rows."""
import pytest

import test_chain_bwd_steps_gpu as S

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("din", [4, 12, 18, 36, 64])
def test_chain_bwd_publisher_input_widths_match_per_layer(cuda_device, monkeypatch, din):
    S._check_chain_vs_per_layer(cuda_device, monkeypatch, S._layer(cuda_device, din=din), 28, 40, 6, din=din)
