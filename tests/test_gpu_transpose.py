"""GPU: tip_transpose2d_dev (csrc/tip_transpose.hip) is numpy's `.T` bit for bit, for 4- and 8-byte elements, at shapes that
cover one partial tile, tile edges in either axis and in both (the tile is 64 x 64), and more than one workgroup."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 257), (257, 1), (63, 65), (64, 64), (65, 63), (130, 37), (300, 515)]


def make_plane(shape, elem_bytes, seed):
    rng = np.random.default_rng(seed)
    if elem_bytes == 4:
        return rng.integers(-2 ** 31, 2 ** 31, shape, dtype=np.int64).astype(np.int32)
    a = rng.normal(0, 1e3, shape)
    flat = a.reshape(-1)
    special = np.array([0x7ff8000000000001, 0x7ff80000deadbeef, 0xfff8000000000123, 0x7ff0000000000001,      # NaNs, distinct payloads
                        0x8000000000000000, 0x7ff0000000000000, 0xfff0000000000000], np.uint64).view(np.float64)  # -0.0, +inf, -inf
    pos = rng.permutation(flat.size)[:special.size]          # (a 1 x 1 plane takes the first: a NaN with a payload)
    flat[pos] = special[:pos.size]
    return a


def transpose_dev(a):
    from tissue_image_processing_amd import _lib
    a = np.ascontiguousarray(a)
    rows, cols = a.shape
    d_in = _lib.DeviceBuffer(a.nbytes).upload(a)
    d_out = _lib.DeviceBuffer(a.nbytes)
    _lib.transpose2d_dev(d_in.ptr, d_out.ptr, rows, cols, a.itemsize)
    d_back = _lib.DeviceBuffer(a.nbytes)
    _lib.transpose2d_dev(d_out.ptr, d_back.ptr, cols, rows, a.itemsize)
    return d_out.download((cols, rows), a.dtype), d_back.download((rows, cols), a.dtype)


def bits(a):
    return a.view(np.uint64 if a.itemsize == 8 else np.uint32)


@pytest.mark.parametrize("elem_bytes", [4, 8])
@pytest.mark.parametrize("shape", SHAPES)
def test_transpose_equals_numpy(shape, elem_bytes):
    a = make_plane(shape, elem_bytes, seed=shape[0] * 1000 + shape[1])
    if elem_bytes == 8:
        assert np.isnan(a).any()
    got, back = transpose_dev(a)
    np.testing.assert_array_equal(bits(got), bits(np.ascontiguousarray(a.T)))
    np.testing.assert_array_equal(bits(back), bits(a))          # transposing twice gives the input back


def test_argument_errors():
    from tissue_image_processing_amd import _lib
    d_a, d_b = _lib.DeviceBuffer(1024), _lib.DeviceBuffer(1024)
    with pytest.raises(ValueError):
        _lib.transpose2d_dev(d_a.ptr, d_b.ptr, 8, 8, 2)           # element size
    with pytest.raises(ValueError):
        _lib.transpose2d_dev(d_a.ptr, d_b.ptr, 0, 8, 4)           # zero extent
    with pytest.raises(ValueError):
        _lib.transpose2d_dev(d_a.ptr, d_b.ptr, 8, 0, 8)
    with pytest.raises(ValueError):
        _lib.transpose2d_dev(d_a.ptr, d_a.ptr, 8, 8, 4)           # in == out
    with pytest.raises(ValueError):
        _lib.transpose2d_dev(None, d_b.ptr, 8, 8, 4)              # null pointer
    _lib.transpose2d_dev(d_a.ptr, d_b.ptr, 8, 8, 4)               # (the thread's error state does not stick)
    _lib.check(_lib.lib().tip_sync())
