"""Host: blur_image's refolding of arrays with more than 65535 planes or rows, with the device call replaced by the oracle.
What is checked here is the host logic alone -- every launch stays within the grid limits, and the pieces put together are the
oracle's filter of the whole array; tests/test_gpu_gauss_regimes.py runs the same shapes on the device."""
import numpy as np
import pytest


@pytest.fixture()
def bim_on_oracle(monkeypatch):
    from oracle import oracle as orc
    from tissue_image_processing_amd import basic_image_manipulations as bim
    seen = []

    def gaussian3d(vol, taps, dtype):
        assert vol.flags.c_contiguous and vol.ndim == 3 and vol.dtype == (np.float32, np.float64)[dtype]
        seen.append(vol.shape)
        out = vol
        for ax, t in enumerate(taps):
            if t is not None:
                out = orc.correlate1d(out, t, ax)
        return out.copy() if out is vol else out

    monkeypatch.setattr(bim, "_gaussian3d", gaussian3d)
    return bim, orc, seen


@pytest.mark.parametrize("shape,sigma", [((65537, 1, 3), (0, 0, 1)), ((70000, 4), (0, 1.5)), ((70000, 4), (1.5, 0)),
                                         ((3, 2, 11000, 5), (0, 0, 0, 1)), ((65537, 3, 2), (0, 1, 0)), ((65537, 3, 2), (1, 1, 1)),
                                         ((3, 70000, 2), (1, 0, 0)), ((131075, 2), (0, 1)), ((70000, 4), (0, 0)),
                                         ((65535, 4), (1, 1)), ((70000,), (2,))])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_refolded_blur_equals_whole_array_filter(bim_on_oracle, shape, sigma, dtype):
    bim, orc, seen = bim_on_oracle
    rng = np.random.default_rng(len(shape))
    img = (rng.standard_normal(shape) * 10.0 ** rng.uniform(-3, 3, shape)).astype(dtype)
    keep = img.copy()
    out = bim.blur_image(img, sigma)
    assert out.dtype == img.dtype and out.shape == img.shape and out is not img
    np.testing.assert_array_equal(img, keep)
    np.testing.assert_array_equal(out, orc.blur_image(img, sigma))
    assert all(z <= 65535 and y <= 65535 for z, y, _ in seen), seen


def test_refolded_blur_of_an_integer_table(bim_on_oracle):
    bim, orc, seen = bim_on_oracle
    img = np.random.default_rng(1).integers(0, 4000, (70000, 4)).astype(np.uint16)
    ref = img.astype(np.float64)
    for sg in [(1.5, 0), (0, 1.5)]:
        ref = np.trunc(orc.blur_image(ref, sg))
    np.testing.assert_array_equal(bim.blur_image(img, 1.5), ref.astype(np.uint16))
    assert all(z <= 65535 and y <= 65535 for z, y, _ in seen), seen
