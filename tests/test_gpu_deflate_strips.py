"""GPU: the strip-wise zlib encoder of csrc/tip_deflate.hip (tip_deflate_strips, tip_deflate_strips_dev) against its Python
restatement (tests/deflate_strips_restate.py): every strip's stream byte for byte through both entry forms and under both codes,
zlib.decompress of every strip, the compacted layout (page-major table, even offsets, zero pad bytes, the total, the bound), a
strip of exactly 65536 bytes and the one row more that is refused, more strips than workgroups; the argument errors."""
import ctypes
import zlib

import numpy as np
import pytest

import deflate_strips_cases as sc
import deflate_strips_restate as sr

pytestmark = pytest.mark.gpu


def _device_form(pages, rps, codes):
    """-> (compacted bytes, table, total) of tip_deflate_strips_dev on an uploaded copy of the pages"""
    from tissue_image_processing_amd import _deflate, _lib
    n_pages, rows, cols = pages.shape
    item = pages.dtype.itemsize
    cap = _deflate.strips_bound(n_pages, rows, cols * item, rps)
    assert cap == sr.bound(n_pages, rows, cols * item, rps)
    src, dst = _lib.DeviceBuffer(max(pages.nbytes, 1)), _lib.DeviceBuffer(max(cap, 1))
    if pages.size:
        src.upload(pages)
    table, total = _deflate.deflate_strips_dev(src.ptr, n_pages, rows, cols * item, item, rps, codes, dst.ptr, cap)
    assert 0 <= total <= cap
    return (dst.download((total,), np.uint8).tobytes() if total else b""), table, total


@pytest.mark.parametrize("codes", sr.CODES)
@pytest.mark.parametrize("name", sc.NAMES)
def test_device_streams_are_the_restatement(name, codes):
    from tissue_image_processing_amd import _deflate
    pages, rps = sc.CASES[name]
    want = sc.restated(name, codes)
    raw = sr.raw_strips(pages, rps)
    want_bytes, want_table = sr.compact(want)
    got, table, total = _device_form(pages, rps, codes)
    assert total == len(want_bytes) and [tuple(int(v) for v in row) for row in table] == want_table, name
    assert all(int(o) % 2 == 0 for o, _ in table)
    assert got == want_bytes, (name, next(i for i in range(len(want_bytes)) if got[i] != want_bytes[i]))
    host = _deflate.deflate_strips(pages, rps, codes)
    assert host == want, name
    assert _deflate.split_strips(np.frombuffer(got, np.uint8), table, pages.shape[0]) == want
    for page, raw_page in zip(host, raw):
        assert len(page) == len(raw_page)
        for stream, strip in zip(page, raw_page):
            assert zlib.decompress(stream) == strip
            assert len(stream) <= sr.strip_bound(len(strip))


def test_noise_grows_but_stays_inside_the_bound():
    pages, rps = sc.CASES["noise_40x48_rps7_u8"]
    for codes in sr.CODES:
        streams = sc.restated("noise_40x48_rps7_u8", codes)
        raw = sr.raw_strips(pages, rps)
        assert all(len(s) > len(r) for s, r in zip(streams[0], raw[0]))      # the case is what its name says


def test_one_row_more_than_a_chunk_is_unsupported():
    from tissue_image_processing_amd import _deflate, _lib
    pages, _ = sc.CASES["full_8x4096_rps8_u16"]
    lib = _lib.lib()
    cap = _deflate.strips_bound(1, 8, 8192, 9)
    src, dst = _lib.DeviceBuffer(pages.nbytes), _lib.DeviceBuffer(cap)
    src.upload(pages)
    table, total = np.zeros((1, 2), np.int64), ctypes.c_int64(-1)
    host_dst = np.empty(cap, np.uint8)
    for entry, s, d in ((lib.tip_deflate_strips_dev, src.ptr, dst.ptr), (lib.tip_deflate_strips, _lib.ptr(pages), _lib.ptr(host_dst))):
        assert entry(s, 1, 8, 8192, 2, 9, 1, d, cap, _lib.ptr(table), ctypes.byref(total)) == -5
        assert _lib.TIP_ERR_UNSUPPORTED == -5 and "65536" in _lib.last_error()
        assert entry(s, 1, 8, 8192, 2, 8, 1, d, cap, _lib.ptr(table), ctypes.byref(total)) == 0
        want = sc.restated("full_8x4096_rps8_u16", "dynamic")[0][0]
        assert total.value == len(want) + (len(want) & 1) and [int(v) for v in table[0]] == [0, len(want)]


def test_argument_errors_and_the_call_after_them():
    from tissue_image_processing_amd import _deflate, _lib
    lib = _lib.lib()
    name = "ragged_40x48_rps7_u16"
    pages, rps = sc.CASES[name]
    n_pages, rows, cols = pages.shape
    row_bytes = cols * 2
    cap = _deflate.strips_bound(n_pages, rows, row_bytes, rps)
    want_bytes, want_table = sr.compact(sc.restated(name, "fixed"))
    src, dst = _lib.DeviceBuffer(pages.nbytes), _lib.DeviceBuffer(cap)
    src.upload(pages)
    table, total = np.zeros((len(want_table), 2), np.int64), ctypes.c_int64(-1)
    tab, tot = _lib.ptr(table), ctypes.byref(total)
    host_dst = np.empty(cap, np.uint8)
    for entry, s, d in ((lib.tip_deflate_strips_dev, src.ptr, dst.ptr), (lib.tip_deflate_strips, _lib.ptr(pages), _lib.ptr(host_dst))):
        ARG = _lib.TIP_ERR_ARG
        assert entry(None, n_pages, rows, row_bytes, 2, rps, 0, d, cap, tab, tot) == ARG
        assert entry(s, n_pages, rows, row_bytes, 2, rps, 0, None, cap, tab, tot) == ARG
        assert entry(s, n_pages, rows, row_bytes, 2, rps, 0, d, cap, None, tot) == ARG
        assert entry(s, n_pages, rows, row_bytes, 2, rps, 0, d, cap, tab, None) == ARG
        for elem in (0, 3, 4):
            assert entry(s, n_pages, rows, row_bytes, elem, rps, 0, d, cap, tab, tot) == ARG
            assert "elem_bytes" in _lib.last_error()
        for bad_row in (0, -96, 95):                                                    # not positive, no multiple of elem_bytes
            assert entry(s, n_pages, rows, bad_row, 2, rps, 0, d, cap, tab, tot) == ARG
            assert "row_bytes" in _lib.last_error()
        for bad_rps in (0, -1):
            assert entry(s, n_pages, rows, row_bytes, 2, bad_rps, 0, d, cap, tab, tot) == ARG
            assert "rows_per_strip" in _lib.last_error()
        assert entry(s, n_pages, rows, row_bytes, 2, rps, 2, d, cap, tab, tot) == ARG
        assert entry(s, n_pages, rows, row_bytes, 2, rps, 0, d, cap - 1, tab, tot) == ARG
        assert "bound" in _lib.last_error()
        assert entry(s, n_pages, rows, row_bytes, 2, rps, 0, d, cap, tab, tot) == 0       # ... and the next valid call succeeds
        assert total.value == len(want_bytes) and [tuple(int(v) for v in row) for row in table] == want_table
    assert dst.download((total.value,), np.uint8).tobytes() == want_bytes
    assert host_dst[:total.value].tobytes() == want_bytes
    out = ctypes.c_int64(0)
    assert lib.tip_deflate_strips_bound(1, 8, 16, 0, ctypes.byref(out)) == _lib.TIP_ERR_ARG
    assert lib.tip_deflate_strips_bound(1, 8, 16, 4, None) == _lib.TIP_ERR_ARG
