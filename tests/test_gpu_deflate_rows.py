"""GPU: the rows rule of csrc/tip_deflate.hip (tip_deflate_rows, tip_deflate_rows_dev) against its Python restatement
(tests/deflate_rows_restate.py) -- the device stream byte for byte, the CRC against zlib.crc32, through both entry forms -- on maps
whose rows straddle segment and chunk edges, at the candidate distances' limits, from an unaligned source; the argument errors."""
import ctypes
import zlib

import numpy as np
import pytest

import deflate_cases as dc
import deflate_restate as dr
import deflate_rows_restate as rr

pytestmark = pytest.mark.gpu


def _maps():
    labels, types = dc.voronoi_pair()
    big_l, big_t = np.tile(labels, (6, 3)).astype(np.int32), np.tile(types, (6, 3))
    out = {
        "voronoi_labels": (labels.tobytes(), 4, 512),                  # one partial chunk
        "voronoi_types": (types.tobytes(), 1, 128),
        "tiled_labels": (big_l.tobytes(), 4, 1536),                    # 13.5 chunks; the row above lies in the chunk before
        "tiled_u16": (big_l.astype(np.uint16).tobytes(), 2, 768),      # 6.75 chunks
        "tiled_types": (big_t.tobytes(), 1, 384),                      # 3.4 chunks
        "crop_40x2048": (np.tile(labels, (1, 16))[:40].copy().tobytes(), 4, 8192),      # a row is 32 segments, as in production
        "width_37_u8": (big_t[:, :37].copy().tobytes(), 1, 37),        # odd distances 37, 38, 36: no dword of the row above is aligned
        "width_2_i32": (big_l[:, :2].copy().tobytes(), 4, 8),          # P - e = e is dropped
    }
    for e, array in ((4, big_l), (1, big_t)):
        for row_bytes in (32768, 32768 + e, 32768 + 2 * e):            # three candidates' limit: P and P - e, P - e alone, none
            out["far_%d_e%d" % (row_bytes, e)] = (array.tobytes(), e, row_bytes)
    for name in dc.NAMES:
        if name.startswith("edge_") or name == "worst_e1":
            _, data, e = dc.BY_NAME[name]
            out[name] = (data, e, 256)
    for e in (1, 2, 4):
        out["empty_e%d" % e] = (b"", e, 64)
    return out


MAPS = _maps()
_restated = {}


def restated(name):
    if name not in _restated:
        data, e, row_bytes = MAPS[name]
        _restated[name] = rr.deflate_rows(data, e, row_bytes)
    return _restated[name]


def _device_form(data, e, row_bytes, skip=0):
    from tissue_image_processing_amd import _deflate, _lib
    n = len(data) - skip
    cap = _deflate.runs_bound(n)
    src = _lib.DeviceBuffer(max(len(data), 1))
    dst = _lib.DeviceBuffer(max(cap, 1))
    if data:
        src.upload(np.frombuffer(data, np.uint8))
    size, crc = _deflate.deflate_rows_dev(src.ptr + skip, n, e, row_bytes, dst.ptr, cap)
    assert 0 <= size <= cap
    return (dst.download((size,), np.uint8).tobytes() if size else b""), crc


def _same(stream, want, tag):
    assert len(stream) == len(want), (tag, len(stream), len(want))
    assert stream == want, (tag, next(i for i in range(len(want)) if stream[i] != want[i]))


@pytest.mark.parametrize("name", list(MAPS))
def test_device_stream_is_the_restatement(name):
    from tissue_image_processing_amd import _deflate
    data, e, row_bytes = MAPS[name]
    want = restated(name)
    for form, (stream, crc) in (("dev", _device_form(data, e, row_bytes)), ("host", _deflate.deflate_rows(data, e, row_bytes))):
        assert crc == zlib.crc32(data), (name, form)
        _same(stream, want, (name, form))
    assert dr.inflate(want) == data and len(want) <= dr.bound(len(data))


@pytest.mark.parametrize("e", [4, 1])
def test_without_a_candidate_it_is_the_runs_entrys_stream(e):
    from tissue_image_processing_amd import _deflate
    data, _, row_bytes = MAPS["far_%d_e%d" % (32768 + 2 * e, e)]
    runs, crc = _deflate.deflate_runs(data, e)
    assert (runs, crc) == _deflate.deflate_rows(data, e, row_bytes)
    assert runs == dr.deflate_runs(data, e)
    assert restated("far_%d_e%d" % (32768 + e, e)) != runs                   # one candidate left is another stream


@pytest.mark.parametrize("name,skip", [("tiled_types", 1), ("tiled_types", 2), ("tiled_u16", 2), ("width_37_u8", 1)])
def test_unaligned_source(name, skip):
    """A source 1 or 2 bytes into an allocation: the staging loop's byte path and the byte reads of the row above."""
    data, e, row_bytes = MAPS[name]
    stream, crc = _device_form(data, e, row_bytes, skip)
    assert crc == zlib.crc32(data[skip:])
    _same(stream, rr.deflate_rows(data[skip:], e, row_bytes), (name, skip))


def test_argument_errors_and_the_call_after_them():
    from tissue_image_processing_amd import _deflate, _lib
    lib = _lib.lib()
    data, e, row_bytes = MAPS["voronoi_labels"]
    cap = _deflate.runs_bound(len(data))
    src, dst = _lib.DeviceBuffer(len(data)), _lib.DeviceBuffer(cap)
    src.upload(np.frombuffer(data, np.uint8))
    size, crc = ctypes.c_int64(-1), ctypes.c_uint32(0)
    out = (ctypes.byref(size), ctypes.byref(crc))
    host_src, host_dst = np.frombuffer(data, np.uint8), np.empty(cap, np.uint8)
    for entry, s, d in ((lib.tip_deflate_rows_dev, src.ptr, dst.ptr), (lib.tip_deflate_rows, _lib.ptr(host_src), _lib.ptr(host_dst))):
        for bad in (0, -512, row_bytes + 2, 3):                                          # not positive, no multiple of elem_bytes
            assert entry(s, len(data), e, bad, d, cap, *out) == _lib.TIP_ERR_ARG
            assert "row_bytes" in _lib.last_error()
        assert entry(s, len(data), e, row_bytes, d, cap - 1, *out) == _lib.TIP_ERR_ARG   # cap below the runs bound
        assert "bound" in _lib.last_error()
        assert entry(s, len(data), 3, row_bytes, d, cap, *out) == _lib.TIP_ERR_ARG
        assert entry(s, len(data), e, row_bytes, d, cap, *out) == 0                      # ... and the next valid call succeeds
        assert size.value == len(restated("voronoi_labels")) and crc.value == zlib.crc32(data)
    assert dst.download((size.value,), np.uint8).tobytes() == restated("voronoi_labels")
