"""The oracle's phase correlation with a guard on its own surfaces, shared by the GPU drift tests."""
import numpy as np


def guarded_oracle(a, b, ups):
    """the oracle's shift, after asserting on its own |cc| surfaces (numpy alone) that each winner is ahead of the runner-up by a
    relative 1e-9: far above float64 rounding, so equality with the oracle does not hang on the last bits of either transform"""
    from oracle import oracle as orc
    shifts, coarse, fine = orc.phase_cross_correlation_surfaces(a, b, ups)
    for name, s in (("coarse", coarse), ("upsampled", fine)):
        if s is not None:
            top = np.partition(s.ravel(), s.size - 2)[-2:]
            assert top[1] - top[0] > 1e-9 * top[1], "%s surface: winner %r, runner-up %r" % (name, top[1], top[0])
    return shifts
