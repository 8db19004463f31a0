"""The fixed summation order of the batch loss sum (ssnt_fwd_bwd_sum_device), restated in numpy for
the GPU tests that hold ``loss_sum`` to it bit for bit. Test infrastructure only."""
import numpy as np


def wave_order_sum(loss):
    """64 lane-strided f32 partial sums, then an xor butterfly (lattice_dev.h wave_loss_sum)."""
    acc = np.zeros(64, np.float32)
    for i, v in enumerate(np.asarray(loss, np.float32)):
        acc[i % 64] = np.float32(acc[i % 64] + v)
    off = 32
    while off >= 1:
        acc = (acc + acc[np.arange(64) ^ off]).astype(np.float32)
        off //= 2
    return acc[0]
