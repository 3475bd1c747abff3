"""GPU: csrc/tip_inflate.hip -- the device decoder on the whole case list of tests/inflate_cases.py against the expected bytes,
the named statuses and the guards, as tests/test_inflate_host.py checks the host decoder; a call of 300 strips of mixed sizes
(the work distribution); the table checks; and the 16-bit TIFF row pass against numpy.  No random mutation runs here: that
belongs to the host sanitizer program (tools/inflate_hostcheck.cpp)."""
import zlib

import numpy as np
import pytest

import inflate_cases as ic

pytestmark = pytest.mark.gpu


def _device_form(src, strips, wrapper, dst):
    """tip_inflate_strips_dev on uploaded copies -> (status, n_bad); dst is downloaded back in place"""
    from tissue_image_processing_amd import _inflate, _lib
    d_src, d_tab = _lib.DeviceBuffer(max(src.size, 1)), _lib.DeviceBuffer(max(strips.nbytes, 1))
    d_dst, d_status = _lib.DeviceBuffer(max(dst.size, 1)), _lib.DeviceBuffer(max(4 * len(strips), 4))
    if src.size:
        d_src.upload(src)
    d_tab.upload(strips)
    d_dst.upload(dst)
    n_bad = _inflate.inflate_strips_dev(d_src.ptr, src.size, d_tab.ptr, len(strips), wrapper, d_dst.ptr, dst.size, d_status.ptr)
    dst[:] = d_dst.download((dst.size,), np.uint8)
    return d_status.download((len(strips),), np.int32), n_bad


@pytest.mark.parametrize("which", ["valid", "all"])       # the valid streams first, then the hand-made invalid ones among them
@pytest.mark.parametrize("wrapper", [0, 1])
def test_device_decoder_on_the_case_list(wrapper, which):
    from tissue_image_processing_amd import _inflate
    cases = [c for c in (ic.VALID if which == "valid" else ic.CASES) if c[2] == wrapper]
    src, strips, dst0 = ic.pack(cases)
    host_dst = dst0.copy()
    host_status, host_bad = _inflate.inflate_strips_host(src, strips, wrapper, host_dst)
    for form in (_device_form, _inflate.inflate_strips):
        dst = dst0.copy()
        status, n_bad = form(src, strips, wrapper, dst)
        ic.check_packed(cases, strips, dst, status, _inflate.STATUS)
        assert n_bad == host_bad == sum(c[5] != "OK" for c in cases)
        assert np.array_equal(status, host_status)
        ok = np.zeros(dst.size, bool)                         # a failed strip's own bytes are unspecified; everything else is the host's
        for (_, _, d_off, d_len), st in zip(strips, status):
            ok[d_off:d_off + d_len] = st != 0
        assert np.array_equal(dst[~ok], host_dst[~ok])


def test_three_hundred_strips_of_mixed_sizes():
    """More strips than one round of waves takes, lengths from 0 to 70 000 bytes in no order, destinations scattered with guards
    between them: every strip's bytes, every guard, and the statuses of the host decoder."""
    from tissue_image_processing_amd import _inflate
    rng = np.random.default_rng(300)
    sizes = rng.integers(1, 6000, 300)
    sizes[rng.choice(300, 40, replace=False)] = 0
    sizes[137] = 70000
    sizes[[5, 250]] = [1, 258]
    datas = []
    for k, n in enumerate(sizes):
        kind = k % 3
        d = (np.minimum(rng.geometric(0.05, n), 255) if kind == 0 else rng.integers(0, 256, n) if kind == 1
             else np.repeat(rng.integers(0, 256, n // 50 + 1), 50)[:n]).astype(np.uint8)
        datas.append(d.tobytes())
    cases = [("strip%d" % k, zlib.compress(d, 1 + k % 9), 1, d, len(d), "OK") for k, d in enumerate(datas)]
    order = rng.permutation(300)                               # the table's order is not the buffers' order
    src, strips, dst0 = ic.pack([cases[i] for i in order])
    back = np.argsort(order)
    strips, cases_in_table = strips[back], cases
    dst = dst0.copy()
    status, n_bad = _device_form(src, strips, 1, dst)
    assert n_bad == 0 and not status.any()
    ic.check_packed(cases_in_table, strips, dst, status, _inflate.STATUS)
    host = dst0.copy()
    _inflate.inflate_strips_host(src, strips, 1, host)
    assert np.array_equal(dst, host)


def test_more_strips_than_waves_in_the_grid():
    """9000 tiny strips: the grid holds at most 8 workgroups of four waves per CU, so waves take a second strip from the list."""
    from tissue_image_processing_amd import _inflate
    rng = np.random.default_rng(9000)
    datas = [bytes(rng.integers(0, 4, n, dtype=np.uint8)) for n in rng.integers(0, 40, 9000)]
    cases = [("s%d" % k, zlib.compress(d), 1, d, len(d), "OK") for k, d in enumerate(datas)]
    src, strips, dst = ic.pack(cases)
    status, n_bad = _device_form(src, strips, 1, dst)
    assert n_bad == 0 and not status.any()
    ic.check_packed(cases, strips, dst, status, _inflate.STATUS)


def test_table_errors_and_the_call_after_them():
    from tissue_image_processing_amd import _inflate, _lib
    _, stream, _, data, n, _ = ic.BY_NAME["fixed_raw"]
    src = np.frombuffer(stream, np.uint8)
    d_src, d_dst, d_tab, d_status = _lib.DeviceBuffer(src.size).upload(src), _lib.DeviceBuffer(2 * n), _lib.DeviceBuffer(64), _lib.DeviceBuffer(8)
    d_dst.upload(np.zeros(2 * n, np.uint8))

    def call(rows):
        if rows:
            d_tab.upload(np.array(rows, np.int64))
        return _inflate.inflate_strips_dev(d_src.ptr, src.size, d_tab.ptr, len(rows), 0, d_dst.ptr, 2 * n, d_status.ptr)

    for rows in ([(0, src.size, 0, n), (0, src.size, n - 1, n)], [(0, src.size + 1, 0, n)], [(0, src.size, n + 1, n)], [(0, src.size, -1, n)]):
        with pytest.raises(ValueError):
            call(rows)
        assert not d_dst.download((2 * n,), np.uint8).any()         # nothing was written
    with pytest.raises(ValueError):
        _inflate.inflate_strips_dev(d_src.ptr, src.size, d_tab.ptr, 1, 2, d_dst.ptr, 2 * n, d_status.ptr)
    with pytest.raises(ValueError):
        _inflate.inflate_strips_dev(None, src.size, d_tab.ptr, 1, 0, d_dst.ptr, 2 * n, d_status.ptr)
    assert call([(0, src.size, 0, n), (0, src.size, n, n)]) == 0
    assert d_dst.download((2 * n,), np.uint8).tobytes() == data + data
    assert call([]) == 0


@pytest.mark.parametrize("row_elems", [1, 63, 64, 65, 1000])
def test_tiff_finish_rows(row_elems):
    """Rows of 1, 63, 64, 65 and 1000 samples, 1, 3, 5 and 9 rows (no count fills the workgroups of four): byte swap, then the
    running sum modulo 2^16, against numpy; predictor 1 without a swap changes nothing; predictor 3 is refused."""
    from tissue_image_processing_amd import _inflate, _lib
    rng = np.random.default_rng(row_elems)
    for n_rows in (1, 3, 5, 9):
        a = rng.integers(0, 65536, (n_rows + 1, row_elems), dtype=np.uint16)      # one row more than the call covers: it must stay
        buf = _lib.DeviceBuffer(a.nbytes)
        for predictor in (1, 2):
            for swap in (0, 1):
                buf.upload(a)
                _inflate.tiff_finish_u16_dev(buf.ptr, n_rows, row_elems, predictor, swap)
                got = buf.download(a.shape, np.uint16)
                want = a[:n_rows].byteswap() if swap else a[:n_rows]
                if predictor == 2:
                    want = np.cumsum(want, axis=1, dtype=np.uint16)
                assert np.array_equal(got[:n_rows], want), (n_rows, predictor, swap)
                assert np.array_equal(got[n_rows], a[n_rows])
        with pytest.raises(ValueError):
            _inflate.tiff_finish_u16_dev(buf.ptr, n_rows, row_elems, 3, 0)
