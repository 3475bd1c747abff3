"""The inflate of csrc/tip_inflate.hip from Python: many independent deflate streams (a compressed TIFF's strips) decoded on
the device, the same decoder on the host (the tests' reference), and the row pass that finishes 16-bit TIFF samples."""
import ctypes

import numpy as np

from . import _lib

# tip_inflate_status (include/tissue_hip.h)
STATUS = dict(OK=0, BAD_HEADER=1, BAD_BLOCK_TYPE=2, BAD_STORED=3, BAD_LENGTHS=4, BAD_SYMBOL=5, BAD_DISTANCE=6, INPUT_END=7,
              OUTPUT_FULL=8, OUTPUT_SHORT=9, BAD_ADLER=10)
STATUS_NAME = {v: k for k, v in STATUS.items()}
STATUS_TEXT = {0: "ok", 1: "bad zlib header", 2: "reserved block type", 3: "stored LEN/NLEN mismatch", 4: "invalid code lengths",
               5: "invalid symbol", 6: "distance before the start of the strip's output", 7: "input exhausted",
               8: "output would exceed the strip", 9: "output shorter than the strip", 10: "Adler-32 mismatch"}


def _table(strips):
    strips = np.ascontiguousarray(strips, dtype=np.int64)
    if strips.ndim != 2 or strips.shape[1] != 4:
        raise ValueError("strips: (n, 4) int64 rows of src_off, src_len, dst_off, dst_len (got shape %s)" % (strips.shape,))
    return strips


def _host_form(entry, src, strips, wrapper, dst):
    strips = _table(strips)
    src = np.ascontiguousarray(src, dtype=np.uint8)
    if not (isinstance(dst, np.ndarray) and dst.dtype == np.uint8 and dst.flags.c_contiguous and dst.flags.writeable):
        raise ValueError("dst: a writeable C-contiguous uint8 array")
    status = np.zeros(max(len(strips), 1), np.int32)
    n_bad = ctypes.c_int32(0)
    keep_src = src if src.size else np.zeros(1, np.uint8)        # (an empty array has no address to hand over)
    keep_dst = dst if dst.size else np.zeros(1, np.uint8)
    keep_tab = strips if strips.size else np.zeros((1, 4), np.int64)
    _lib.check(entry(_lib.ptr(keep_src), src.size, _lib.ptr(keep_tab), len(strips), int(wrapper), _lib.ptr(keep_dst), dst.size,
                     _lib.ptr(status), ctypes.byref(n_bad)))
    return status[:len(strips)], int(n_bad.value)


def inflate_strips_host(src, strips, wrapper, dst):
    """tip_inflate_strips_host: the decoder on the CPU, no device.  dst (uint8) is filled in place -> (status per strip, n_bad)."""
    return _host_form(_lib.load().tip_inflate_strips_host, src, strips, wrapper, dst)


def inflate_strips(src, strips, wrapper, dst):
    """tip_inflate_strips: host arrays staged through the device -> (status per strip, n_bad)."""
    return _host_form(_lib.lib().tip_inflate_strips, src, strips, wrapper, dst)


def inflate_strips_dev(src_ptr, src_bytes, strips_ptr, n_strips, wrapper, dst_ptr, dst_bytes, status_ptr):
    """tip_inflate_strips_dev on device addresses -> the number of strips whose status is not 0; waits once."""
    n_bad = ctypes.c_int32(0)
    _lib.check(_lib.lib().tip_inflate_strips_dev(src_ptr, int(src_bytes), strips_ptr, int(n_strips), int(wrapper), dst_ptr, int(dst_bytes),
                                                 status_ptr, ctypes.byref(n_bad)))
    return int(n_bad.value)


def tiff_finish_u16_dev(stack_ptr, n_rows, row_elems, predictor, swap_bytes):
    """tip_tiff_finish_u16_dev: in place, asynchronous -- byte swap of every 16-bit sample, then (predictor 2) every row's running sum."""
    rc = _lib.lib().tip_tiff_finish_u16_dev(stack_ptr, int(n_rows), int(row_elems), int(predictor), int(bool(swap_bytes)))
    if rc == -5:
        raise ValueError(_lib.last_error())
    _lib.check(rc)
