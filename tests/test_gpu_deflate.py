"""GPU: csrc/tip_deflate.hip against its Python restatement (tests/deflate_restate.py) -- the device stream byte for byte, the
CRC against zlib.crc32 -- on every case of tests/deflate_cases.py and through both entry forms; the argument errors; the bound."""
import ctypes
import zlib

import numpy as np
import pytest

import deflate_cases as dc
import deflate_restate as dr

pytestmark = pytest.mark.gpu


def _device_form(data, e):
    from tissue_image_processing_amd import _deflate, _lib
    cap = _deflate.runs_bound(len(data))
    src = _lib.DeviceBuffer(max(len(data), 1))
    dst = _lib.DeviceBuffer(max(cap, 1))
    if data:
        src.upload(np.frombuffer(data, np.uint8))
    size, crc = _deflate.deflate_runs_dev(src.ptr, len(data), e, dst.ptr, cap)
    assert 0 <= size <= cap
    return (dst.download((size,), np.uint8).tobytes() if size else b""), crc


@pytest.mark.parametrize("name", dc.NAMES)
def test_device_stream_is_the_restatement(name):
    from tissue_image_processing_amd import _deflate
    _, data, e = dc.BY_NAME[name]
    want = dc.restated(name)
    for form, (stream, crc) in (("dev", _device_form(data, e)), ("host", _deflate.deflate_runs(data, e))):
        assert crc == zlib.crc32(data), (name, form)
        assert len(stream) == len(want), (name, form, len(stream), len(want))
        assert stream == want, (name, form, next(i for i in range(len(want)) if stream[i] != want[i]))


def test_unaligned_source():
    """A source that does not start on a dword (a row of a uint8 map): the staging loop's byte path."""
    from tissue_image_processing_amd import _deflate, _lib
    _, types = dc.voronoi_pair()
    data = types.tobytes()
    src, dst = _lib.DeviceBuffer(len(data)), _lib.DeviceBuffer(_deflate.runs_bound(len(data)))
    src.upload(types)
    for skip in (1, 3):
        size, crc = _deflate.deflate_runs_dev(src.ptr + skip, len(data) - skip, 1, dst.ptr, dst.nbytes)
        assert crc == zlib.crc32(data[skip:])
        assert dst.download((size,), np.uint8).tobytes() == dr.deflate_runs(data[skip:], 1)


def test_argument_errors_and_the_call_after_them():
    from tissue_image_processing_amd import _deflate, _lib
    lib = _lib.lib()
    _, data, e = dc.BY_NAME["voronoi_labels"]
    cap = _deflate.runs_bound(len(data))
    src, dst = _lib.DeviceBuffer(len(data)), _lib.DeviceBuffer(cap)
    src.upload(np.frombuffer(data, np.uint8))
    size, crc = ctypes.c_int64(-1), ctypes.c_uint32(0)
    out = (ctypes.byref(size), ctypes.byref(crc))
    host_src, host_dst = np.frombuffer(data, np.uint8), np.empty(cap, np.uint8)
    for entry, s, d in ((lib.tip_deflate_runs_dev, src.ptr, dst.ptr), (lib.tip_deflate_runs, _lib.ptr(host_src), _lib.ptr(host_dst))):
        assert entry(None, len(data), e, d, cap, *out) == _lib.TIP_ERR_ARG             # a null pointer
        assert entry(s, len(data), e, d, cap, None, out[1]) == _lib.TIP_ERR_ARG
        assert entry(s, len(data), 3, d, cap, *out) == _lib.TIP_ERR_ARG                # elem_bytes outside {1, 2, 4}
        assert entry(s, len(data) - 1, e, d, cap, *out) == _lib.TIP_ERR_ARG            # nbytes no multiple of elem_bytes
        assert entry(s, len(data), e, d, cap - 1, *out) == _lib.TIP_ERR_ARG            # cap below the bound
        assert "bound" in _lib.last_error()
        assert entry(s, len(data), e, d, cap, *out) == 0                                # ... and the next valid call succeeds
        assert size.value == len(dc.restated("voronoi_labels")) and crc.value == zlib.crc32(data)
    assert dst.download((size.value,), np.uint8).tobytes() == dc.restated("voronoi_labels")


def test_bound_entry_is_the_restatements_worst_case():
    """tip_deflate_runs_bound against the restatement's bound, and the restated stream of the worst input -- no repeat, no byte
    below 144: nine bits each -- fills it exactly; noise stays below it."""
    from tissue_image_processing_amd import _deflate
    for n in (0, 1, 255, 65535, 65536, 65537, 3 * 65536 + 12, 2048 * 2048 * 4):
        assert _deflate.runs_bound(n) == dr.bound(n), n
    _, worst, _ = dc.BY_NAME["worst_e1"]
    assert len(dc.restated("worst_e1")) == _deflate.runs_bound(len(worst))
    _, noise, _ = dc.BY_NAME["noise_e1"]
    assert len(dc.restated("noise_e1")) < _deflate.runs_bound(len(noise))
