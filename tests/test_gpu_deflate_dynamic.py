"""GPU: the dynamic-code deflate entries of csrc/tip_deflate.hip (tip_deflate_dynamic, tip_deflate_dynamic_dev) against their Python
specification (tests/deflate_dynamic_restate.py) -- the device stream byte for byte, the CRC against zlib.crc32, through both entry
forms -- on the cases of tests/deflate_dynamic_cases.py: the rows rule's maps, one distance symbol, none, a chunk that stays fixed,
a dynamic chunk in front of a fixed one, a tree deeper than 15 bits; from an unaligned source; the argument errors; the run-only
rule; and the fixed entries after a dynamic call."""
import ctypes
import zlib

import numpy as np
import pytest

import deflate_dynamic_cases as cases
import deflate_dynamic_restate as dd
import deflate_restate as dr
import deflate_rows_restate as rr

pytestmark = pytest.mark.gpu

ALL = dict(cases.CASES, **cases.EMPTY)


def _want(name):
    return cases.restated(name) if name in cases.CASES else b""


def _device_form(data, e, row_bytes, skip=0):
    from tissue_image_processing_amd import _deflate, _lib
    n = len(data) - skip
    cap = _deflate.runs_bound(n)
    src = _lib.DeviceBuffer(max(len(data), 1))
    dst = _lib.DeviceBuffer(max(cap, 1))
    if data:
        src.upload(np.frombuffer(data, np.uint8))
    size, crc = _deflate.deflate_dynamic_dev(src.ptr + skip, n, e, row_bytes, dst.ptr, cap)
    assert 0 <= size <= cap
    return (dst.download((size,), np.uint8).tobytes() if size else b""), crc


def _same(stream, want, tag):
    first = next((i for i in range(min(len(stream), len(want))) if stream[i] != want[i]), None)
    assert stream == want, (tag, "first differing offset", first, "lengths", len(stream), len(want))


@pytest.mark.parametrize("name", list(ALL))
def test_device_stream_is_the_restatement(name):
    from tissue_image_processing_amd import _deflate
    data, e, row_bytes = ALL[name]
    want = _want(name)
    for form, (stream, crc) in (("dev", _device_form(data, e, row_bytes)), ("host", _deflate.deflate_dynamic(data, e, row_bytes))):
        assert crc == zlib.crc32(data), (name, form)
        assert len(stream) <= _deflate.runs_bound(len(data)), (name, form)
        _same(stream, want, (name, form))
    assert dr.inflate(want) == data


@pytest.mark.parametrize("name,skip", [("tiled_types", 1), ("width_37_u8", 3)])
def test_unaligned_source(name, skip):
    """A source 1 or 3 bytes into an allocation: the staging loop's byte path and the byte reads of the row above."""
    data, e, row_bytes = cases.CASES[name]
    stream, crc = _device_form(data, e, row_bytes, skip)
    assert crc == zlib.crc32(data[skip:])
    _same(stream, dd.deflate_dynamic(data[skip:], e, row_bytes), (name, skip))


@pytest.mark.parametrize("name", ["voronoi_labels", "tiled_types"])
def test_row_bytes_zero_is_the_run_only_rule(name):
    from tissue_image_processing_amd import _deflate
    data, e, _ = cases.CASES[name]
    want = dd.deflate_dynamic(data, e, None)
    assert want != cases.restated(name)
    for form, (stream, crc) in (("dev", _device_form(data, e, 0)), ("host", _deflate.deflate_dynamic(data, e, 0)),
                                ("host, None", _deflate.deflate_dynamic(data, e))):
        assert crc == zlib.crc32(data), (name, form)
        _same(stream, want, (name, form))


def test_argument_errors_and_the_call_after_them():
    from tissue_image_processing_amd import _deflate, _lib
    lib = _lib.lib()
    data, e, row_bytes = cases.CASES["voronoi_labels"]
    want = cases.restated("voronoi_labels")
    cap = _deflate.runs_bound(len(data))
    src, dst = _lib.DeviceBuffer(len(data)), _lib.DeviceBuffer(cap)
    src.upload(np.frombuffer(data, np.uint8))
    size, crc = ctypes.c_int64(-1), ctypes.c_uint32(0)
    out = (ctypes.byref(size), ctypes.byref(crc))
    host_src, host_dst = np.frombuffer(data, np.uint8), np.empty(cap, np.uint8)
    for entry, s, d in ((lib.tip_deflate_dynamic_dev, src.ptr, dst.ptr), (lib.tip_deflate_dynamic, _lib.ptr(host_src), _lib.ptr(host_dst))):
        for bad in (-512, row_bytes + 2, 3):                                             # negative, no multiple of elem_bytes
            assert entry(s, len(data), e, bad, d, cap, *out) == _lib.TIP_ERR_ARG
            assert "row_bytes" in _lib.last_error()
        assert entry(s, len(data), e, row_bytes, d, cap - 1, *out) == _lib.TIP_ERR_ARG   # cap below the runs bound
        assert "bound" in _lib.last_error()
        assert entry(s, len(data), 3, row_bytes, d, cap, *out) == _lib.TIP_ERR_ARG
        assert entry(s, len(data) - 1, e, row_bytes, d, cap, *out) == _lib.TIP_ERR_ARG   # nbytes no multiple of elem_bytes
        assert entry(None, len(data), e, row_bytes, d, cap, *out) == _lib.TIP_ERR_ARG
        assert entry(s, len(data), e, row_bytes, d, cap, *out) == 0                      # ... and the next valid call succeeds
        assert size.value == len(want) and crc.value == zlib.crc32(data)
    assert dst.download((size.value,), np.uint8).tobytes() == want
    assert host_dst[:size.value].tobytes() == want


@pytest.mark.parametrize("name", ["voronoi_labels", "tiled_types"])
def test_the_fixed_entries_after_a_dynamic_call(name):
    from tissue_image_processing_amd import _deflate
    data, e, row_bytes = cases.CASES[name]
    _same(_deflate.deflate_dynamic(data, e, row_bytes)[0], cases.restated(name), (name, "dynamic"))
    _same(_deflate.deflate_rows(data, e, row_bytes)[0], rr.deflate_rows(data, e, row_bytes), (name, "rows"))
    _same(_deflate.deflate_runs(data, e)[0], dr.deflate_runs(data, e), (name, "runs"))
