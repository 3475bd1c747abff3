"""Drop-in for the array operators of the reference's basic_image_manipulations.py (bim.py), running on MI355X.

Same function names, argument meaning, return dtypes and error behaviour as the reference:
    put_channel_axis_first(image, axes)                              bim.py:199-231   (pure view logic, host)
    blur_image(image, std)                                           bim.py:373-390   -> tip_gaussian3d_w
    watershed_segmentation(image, imgthresh, stdeviation, blocksize) bim.py:446-476   -> tip_watershed_segmentation
    read_image_in_chunks / get_image_dimensions / concatenate_time_points / read_tiff / save_tiff
                                                                     bim.py:28-188, 478-495 (host I/O around the GPU path;
                                                                     image sources: arrays, .npy, TIFF stacks, aicsimageio objects)
"""

import numpy as np

from . import _lib

UINT8_MAXVAL = 255
UINT16_MAXVAL = 65535
_GRID_MAX = 65535      # the z and y extents of a launch are grid dimensions (correlate1d_dev refuses more)


def _gaussian_kernel1d(sigma, radius):
    """Taps exactly as scipy's Python layer builds them (scipy/ndimage/filters.py:_gaussian_kernel1d, order 0):
    host numpy, like scipy itself, so that a process that also imports scipy sees identical taps."""
    sigma2 = sigma * sigma
    x = np.arange(-radius, radius + 1)
    phi_x = np.exp(-0.5 / sigma2 * x ** 2)
    phi_x = phi_x / phi_x.sum()
    return phi_x


def gaussian_taps(sigma, truncate=4.0):
    sd = float(sigma)
    lw = int(truncate * sd + 0.5)
    return np.ascontiguousarray(_gaussian_kernel1d(sd, lw)[::-1], dtype=np.float64)


def put_channel_axis_first(image, axes):
    """bim.py:199-231: (array, order) with the channel axis moved to the front and the remaining axes in the
    reference's canonical order C, [T], [Z], X, Y.  The reference only reorders when "C" is present and not already
    first; otherwise the array comes back untouched with the identity order."""
    where = {name: axes.find(name) for name in "CTZXY"}
    if where["C"] <= 0:
        return image, tuple(np.arange(len(axes)))
    order = tuple(where[name] for name in "CTZXY" if name in "CXY" or where[name] >= 0)
    return np.transpose(image, axes=order), order


def _normalize_sigma(std, ndim):
    sig = np.ravel(np.asarray(std, dtype=np.float64))
    if sig.size == 1:
        sig = np.repeat(sig, ndim)
    if sig.size != ndim:
        # scipy's _ni_support._normalize_sequence
        raise RuntimeError("sequence argument must have length equal to input rank")
    return sig


def blur_image(image, std):
    """bim.py:373-390: scipy.ndimage.gaussian_filter(image, std, mode='nearest'); same shape and dtype out.

    float32 / float64 arrays of any rank run on the GPU with scipy's exact arithmetic (double accumulation in
    scipy's tap order, rounding to the array dtype after each axis).  Integer images follow scipy's rule
    "output dtype == input dtype": they are filtered in float64 and truncated on store, as scipy's C core does.

    Sizes: any extents that fit host and device memory.  One launch takes at most 65535 planes and 65535 rows (they are
    grid dimensions); an array with more of either -- a long movie folded into (leading, axis, trailing), a tall table --
    is filtered axis after axis in launches refolded below that limit (_blur_axis_refolded), with the same bits.
    """
    image = np.asarray(image)
    if image.ndim < 1:
        raise ValueError("blur_image needs an array of rank >= 1")
    sig = _normalize_sigma(std, image.ndim)
    if image.ndim > 3:
        # scipy filters axis after axis, rounding to the array dtype in between: for any rank that is one pass per axis over
        # the (leading, axis, trailing) view of the array, each of them a rank-3 call below
        cur = np.ascontiguousarray(image)
        for ax in range(image.ndim):
            if sig[ax] > 1e-15:
                lead = int(np.prod(image.shape[:ax], dtype=np.int64))
                trail = int(np.prod(image.shape[ax + 1:], dtype=np.int64))
                cur = blur_image(cur.reshape(lead, image.shape[ax], trail), (0.0, sig[ax], 0.0)).reshape(image.shape)
        return cur if cur is not image else image.copy()
    if np.issubdtype(image.dtype, np.integer) or image.dtype == bool:
        # scipy keeps the input dtype: every axis pass accumulates in double and the C core casts the result back to
        # the integer type (truncation toward zero) before the next axis sees it
        cur = image.astype(np.float64)
        for ax in range(image.ndim):
            if sig[ax] > 1e-15:
                one = np.zeros(image.ndim)
                one[ax] = sig[ax]
                cur = np.trunc(blur_image(cur, tuple(one)))
        return cur.astype(image.dtype)
    src = image
    if image.dtype == np.float32:
        dtype = 0
    elif image.dtype == np.float64:
        dtype = 1
    else:
        raise TypeError("blur_image on MI355X supports float32/float64/integer images (got %s)" % image.dtype)
    src = np.ascontiguousarray(src)
    if src.size == 0:
        return src.copy()
    shape3 = (1,) * (3 - src.ndim) + src.shape
    taps = [None, None, None]
    for ax in range(src.ndim):
        if sig[ax] > 1e-15:
            taps[ax + 3 - src.ndim] = gaussian_taps(sig[ax])
    vol = src.reshape(shape3)
    if shape3[0] <= _GRID_MAX and shape3[1] <= _GRID_MAX:
        return _gaussian3d(vol, taps, dtype).reshape(src.shape)
    # a longer z or y extent does not fit one launch: axis after axis (the rounding to the array dtype in between is scipy's
    # too), every pass refolded so that no launch sees more than _GRID_MAX planes or rows
    cur = vol
    for ax in range(3):
        if taps[ax] is not None:
            cur = _blur_axis_refolded(cur, ax, taps[ax], dtype)
    return (cur.copy() if cur is vol else cur).reshape(src.shape)


def _gaussian3d(vol, taps, dtype):
    """one tip_gaussian3d_w call on a contiguous (z, y, x) array; taps: per axis, None for an axis that is not filtered"""
    out = np.empty_like(vol)
    args = []
    for t in taps:
        args += [_lib.ptr(t), 0 if t is None else t.size]
    _lib.check(_lib.lib().tip_gaussian3d_w(_lib.ptr(vol), _lib.ptr(out), dtype, vol.shape[0], vol.shape[1], vol.shape[2], *args))
    return out


def _blur_rows(rows, t, dtype):
    """the x pass of any number of independent rows: planes of _GRID_MAX rows, and one more launch for the rest"""
    n_rows, n = rows.shape
    full = n_rows // _GRID_MAX
    if full > _GRID_MAX:
        raise ValueError("blur_image: %d independent lines (at most %d * %d)" % (n_rows, _GRID_MAX, _GRID_MAX))
    out = np.empty_like(rows)
    cut = full * _GRID_MAX
    if full:
        out[:cut] = _gaussian3d(rows[:cut].reshape(full, _GRID_MAX, n), (None, None, t), dtype).reshape(cut, n)
    if cut < n_rows:
        out[cut:] = _gaussian3d(rows[cut:].reshape(1, n_rows - cut, n), (None, None, t), dtype).reshape(n_rows - cut, n)
    return out


def _blur_axis_refolded(vol, ax, t, dtype):
    """One axis pass of a contiguous rank-3 array as launches of at most _GRID_MAX planes and rows.  The unfiltered extents are
    independent lines, so the array is the (leading, axis, trailing) view of itself: an x pass of leading rows when nothing
    trails, else a y pass of trailing-wide rows, a stack of leading planes at a time; a filtered axis that is itself longer
    than _GRID_MAX (and not the last) is moved to the end on the host, filtered as rows and moved back."""
    lead = int(np.prod(vol.shape[:ax], dtype=np.int64))
    n = vol.shape[ax]
    trail = int(np.prod(vol.shape[ax + 1:], dtype=np.int64))
    if trail == 1:
        return _blur_rows(vol.reshape(lead, n), t, dtype).reshape(vol.shape)
    v = vol.reshape(lead, n, trail)
    if n > _GRID_MAX:
        rows = np.ascontiguousarray(v.transpose(0, 2, 1)).reshape(lead * trail, n)
        back = _blur_rows(rows, t, dtype).reshape(lead, trail, n).transpose(0, 2, 1)
        return np.ascontiguousarray(back).reshape(vol.shape)
    out = np.empty_like(v)
    for a in range(0, lead, _GRID_MAX):
        out[a:a + _GRID_MAX] = _gaussian3d(v[a:a + _GRID_MAX], (None, t, None), dtype)
    return out.reshape(vol.shape)


def watershed_segmentation(image, imgthresh, stdeviation, blocksize):
    """bim.py:446-476 (the 4-argument definition, which shadows the 3-argument one at bim.py:417-443).

    threshold_local(generic max) -> zero below threshold -> blur_image(stdeviation) -> skimage watershed with
    watershed_line=True.  Returns int32 labels, 0 on watershed lines.
    """
    from . import _segmentation
    return _segmentation.watershed_segmentation(image, imgthresh, stdeviation, blocksize)


def calculate_drift(first_image, second_image, sub_pixel_precision=True):
    """bim.py:522-536: global 2-D drift between two frames by phase cross-correlation (shift[-2:])."""
    from ._registration import phase_cross_correlation
    if sub_pixel_precision:
        shift, error, diffphase = phase_cross_correlation(first_image, second_image, upsample_factor=100)
    else:
        shift, error, diffphase = phase_cross_correlation(first_image, second_image)
    return shift[-2:]


# ---- display / export array operations ------------------------------------------------------------
def _as_float_like_skimage(image):
    """skimage.util.img_as_float as skimage.filters.gaussian applies it (unsigned integers scaled by 1 / dtype max in
    float64, floats untouched)."""
    image = np.asarray(image)
    if image.dtype.kind == "u":
        return np.multiply(image, 1.0 / np.iinfo(image.dtype).max, dtype=np.float64)
    if image.dtype.kind == "f":
        return image
    raise TypeError("band_pass_filter on MI355X takes unsigned integer or float images (got %s)" % image.dtype)


def band_pass_filter(image, lowsigma, highsigma):
    """bim.py:393-414: skimage.filters.difference_of_gaussians = gaussian(low) - gaussian(high), edges replicated.
    Both blurs run on the device with scipy's exact tap arithmetic (blur_image)."""
    f = _as_float_like_skimage(image)
    if np.any(np.asarray(highsigma, dtype=float) < np.asarray(lowsigma, dtype=float)):
        raise ValueError("high_sigma must be equal to or larger thanlow_sigma for all axes")   # skimage's wording
    return blur_image(f, lowsigma) - blur_image(f, highsigma)


def _scoreatpercentile(values, per):
    """scipy.stats.scoreatpercentile (default 'fraction' interpolation): the two neighbouring order statistics come from
    the device (radix select, no sort), scipy's weighting from the host."""
    from . import _segmentation as seg
    flat = np.ascontiguousarray(values, dtype=np.float64).reshape(1, -1)
    idx = per / 100.0 * (flat.size - 1)
    i = int(idx)
    lo, hi = seg.label_order_stats(None, flat, 1, np.array([i], np.int64))
    if i == idx:
        return lo[0]
    w = np.array([(i + 1) - idx, idx - i], float)
    return np.add.reduce(np.array([lo[0], hi[0]]) * w) / w.sum()


def set_channel_brightness(image, max_possible_val, method='bestFit', clearExtreamPrecentage=1, minimum_pixel_val=0):
    """bim.py:299-348: saturate the extreme percentiles, shift / scale to [0, 1] (+ 1 / max_possible_val).  `image` is a
    float64 channel and is clipped in place like upstream; skimage's adjust_gamma with gamma 1 is the identity."""
    if clearExtreamPrecentage > 0:
        new_maximum = _scoreatpercentile(image, 100 - clearExtreamPrecentage)
        new_minimum = _scoreatpercentile(image, clearExtreamPrecentage)
        if minimum_pixel_val > 0:
            new_minimum = max(new_minimum, minimum_pixel_val)
        image[image > new_maximum] = new_maximum
    else:
        new_minimum = minimum_pixel_val
    if method in ('minMax', 'bestFit'):
        image = image - new_minimum
        image = image / np.max(image)
        image = image + 1 / max_possible_val
        image[image < 0] = 0
    return image


def set_brightness(image, axes, metadata={}, method='bestFit', clearExtreamPrecentage=1, minVal=0, maxVal=0):
    """bim.py:233-297: per-channel brightness adjustment to floats in [0, 1]; with metadata, (image, adjusted copy of it)."""
    from copy import deepcopy
    kind = np.asarray(image).dtype
    top = maxVal if maxVal else (255 if kind == np.uint8 else 65535 if kind == np.uint16 else 1)
    adjusted = np.array(image, dtype=np.float64)
    floor = metadata['min'] if (metadata and 'min' in metadata) else max(minVal, 0)
    if axes.find("C") >= 0:
        adjusted, order = put_channel_axis_first(adjusted, axes)
        for channel in range(adjusted.shape[0]):
            adjusted[channel] = set_channel_brightness(adjusted[channel], top, method, clearExtreamPrecentage, floor)
        adjusted = np.transpose(adjusted, axes=np.argsort(order))
    else:
        adjusted = set_channel_brightness(adjusted, top, method, clearExtreamPrecentage, floor)
    if not metadata:
        return adjusted
    meta = deepcopy(metadata)
    if 'min' in meta:
        meta['min'] = 0
    if 'max' in meta:
        meta['max'] = top
    if 'Ranges' in meta:
        meta['Ranges'] = (0, top) * int(len(meta['Ranges']) // 2)
    return adjusted, meta


def stretch_for_display(disp_img, min_percent, max_percent):
    """The display stretch of gui.py:445-452 / 468-475 (display_frame: the zo and atoh planes of the composite): both level
    percentiles of the plane (np.percentile, linear), a maximum equal to the minimum is moved up by one, then
    255 * max(plane - lo, 0) / (hi - lo) clipped at 255, in float64.  The two order statistics -- the only dense-array work --
    come from the device radix select (tip_label_order_stats_f64); the arithmetic on them is numpy's."""
    from . import _segmentation as seg
    img = np.asarray(disp_img)
    lo = seg.percentile_frame(img, float(min_percent))
    hi = seg.percentile_frame(img, float(max_percent))
    if hi == lo:
        hi += 1
    out = img - lo
    np.putmask(out, out < 0, 0)
    out = 255 * out / (hi - lo)
    np.putmask(out, out > 255, 255)
    return out


def tiff_normalise(image, data_type=""):
    """The conversion save_tiff applies before writing (bim.py:183-186): images that are not already of the requested
    unsigned type are scaled so that their maximum becomes the type's maximum, and rounded."""
    image = np.asarray(image)
    if data_type and image.dtype != data_type and data_type in ('uint8', 'uint16'):
        top = 255 if data_type == 'uint8' else 65535
        image = np.round((image / np.max(image)) * top).astype(data_type)
    return image


def save_tiff(path, image, metadata=None, axes="", data_type="", compression=None, predictor=1, rowsperstrip=None):
    """bim.py:160-188.  Upstream hands the array to aicsimageio's OME-TIFF writer; here a self-contained baseline TIFF
    writer stores every (Y, X) plane of the normalised array as one page (little-endian, uncompressed, min-is-black) with
    the axes string and shape in the first page's ImageDescription -- what ImageJ / tifffile / the reference's read_tiff
    open as a stack.  `metadata` with a to_xml() method (or a string) is appended to that description; other objects are
    reported once as not written.

    compression="zlib" (opt-in; uint8 / uint16 only) writes every page as deflate strips instead (Compression 8, host zlib, one
    stream per strip of `rowsperstrip` rows -- by default about 64 KB of raw data) with predictor 1 or 2 (horizontal
    differencing).  Without these arguments the file is byte for byte what it always was."""
    import struct
    if compression not in (None, "zlib"):
        raise ValueError("save_tiff: compression %r (None or 'zlib')" % (compression,))
    if compression is None and (predictor != 1 or rowsperstrip is not None):
        raise ValueError("save_tiff: predictor and rowsperstrip belong to compression='zlib'")
    if predictor not in (1, 2):
        raise ValueError("save_tiff: predictor %r (1: none, 2: horizontal differencing)" % (predictor,))
    image = tiff_normalise(image, data_type)
    if image.dtype == np.float64:
        image = image.astype(np.float32)
    if image.dtype not in (np.uint8, np.uint16, np.float32, np.int32):
        raise TypeError("save_tiff writes uint8 / uint16 / int32 / float32 pages (got %s)" % image.dtype)
    if image.ndim < 2:
        raise ValueError("save_tiff needs at least a 2-D image")
    planes = np.ascontiguousarray(image).reshape((-1,) + image.shape[-2:]).astype(image.dtype.newbyteorder("<"))
    rows, cols = planes.shape[1:]
    bits = planes.dtype.itemsize * 8
    fmt = 3 if planes.dtype.kind == "f" else (2 if planes.dtype.kind == "i" else 1)
    desc = ("axes=%s shape=%s" % (axes, "x".join(str(v) for v in image.shape))).encode("ascii") + b"\0"
    if metadata is not None:
        # upstream hands the OME metadata to aicsimageio's writer; here its XML (if it has one) rides in the description
        xml = metadata.to_xml() if hasattr(metadata, "to_xml") else (metadata if isinstance(metadata, (str, bytes)) else None)
        if xml is None:
            import warnings
            warnings.warn("save_tiff: metadata of type %s is not written (no OME-XML writer here)" % type(metadata).__name__)
        else:
            desc = desc[:-1] + b"\n" + (xml if isinstance(xml, bytes) else xml.encode("utf-8", "replace")) + b"\0"
    desc += b"\0" * (len(desc) & 1)                       # TIFF 6.0: every IFD starts on a word boundary
    if compression == "zlib":
        return _save_tiff_zlib(path, planes, desc, predictor, rowsperstrip)
    plane_bytes = rows * cols * planes.dtype.itemsize
    pad = plane_bytes & 1                                   # (odd-sized uint8 planes)
    if planes.nbytes + planes.shape[0] * 256 + len(desc) >= 2 ** 32:
        raise ValueError("save_tiff: classic TIFF holds less than 4 GiB; split the movie")
    with open(path, "wb") as fh:
        fh.write(struct.pack("<2sHI", b"II", 42, 8))
        offset = 8
        for k in range(planes.shape[0]):
            entries = [(256, 4, 1, cols), (257, 4, 1, rows), (258, 3, 1, bits), (259, 3, 1, 1), (262, 3, 1, 1),
                       (277, 3, 1, 1), (278, 4, 1, rows), (279, 4, 1, rows * cols * planes.dtype.itemsize), (339, 3, 1, fmt)]
            extra = desc if k == 0 else b""
            ifd_size = 2 + 12 * (len(entries) + 1 + (1 if extra else 0)) + 4
            data_at = offset + ifd_size + len(extra)
            entries.append((273, 4, 1, data_at))
            if extra:
                entries.append((270, 2, len(extra), offset + ifd_size))
            entries.sort()
            nxt = data_at + plane_bytes + pad if k + 1 < planes.shape[0] else 0
            fh.write(struct.pack("<H", len(entries)))
            for tag, typ, cnt, val in entries:
                fh.write(struct.pack("<HHII", tag, typ, cnt, val))
            fh.write(struct.pack("<I", nxt))
            fh.write(extra)
            fh.write(planes[k].tobytes())
            fh.write(b"\0" * pad)
            offset = nxt
    return


def _save_tiff_zlib(path, planes, desc, predictor, rowsperstrip):
    """save_tiff's deflate form: per page the strip offsets and byte counts follow the IFD, then the strips (zlib streams)."""
    import os
    import struct
    import zlib
    if planes.dtype not in (np.uint8, np.uint16):
        raise TypeError("save_tiff: compression='zlib' writes uint8 / uint16 pages (got %s)" % planes.dtype)
    n_pages, rows, cols = planes.shape
    item = planes.dtype.itemsize
    if rowsperstrip is None:
        rowsperstrip = max(1, min(rows, 65536 // max(1, cols * item)))
    rowsperstrip = int(rowsperstrip)
    if rowsperstrip < 1:
        raise ValueError("save_tiff: rowsperstrip %d" % rowsperstrip)
    rowsperstrip = min(rowsperstrip, rows)
    n_strips = -(-rows // rowsperstrip)
    from concurrent.futures import ThreadPoolExecutor
    threads = max(1, min(16, os.cpu_count() or 1))

    def page_strips(k):
        plane = planes[k]
        if predictor == 2:
            plane = np.concatenate([plane[:, :1], np.diff(plane, axis=1)], axis=1).astype(planes.dtype)      # modulo 2^bits
        return [plane[r:r + rowsperstrip] for r in range(0, rows, rowsperstrip)]

    # (zlib releases the interpreter lock: the strips of a few pages are compressed side by side; the file does not depend on it)
    with open(path, "wb") as fh, ThreadPoolExecutor(threads) as pool:
        fh.write(struct.pack("<2sHI", b"II", 42, 8))
        offset = 8
        done = {}
        for k in range(n_pages):
            if k not in done:
                ahead = range(k, min(n_pages, k + max(1, threads // n_strips)))
                raw = [part for j in ahead for part in page_strips(j)]
                out = list(pool.map(lambda part: zlib.compress(part.tobytes(), 6), raw))
                done = {j: out[i * n_strips:(i + 1) * n_strips] for i, j in enumerate(ahead)}
            strips = done[k]
            sizes = [len(s) for s in strips]
            strips = [s + b"\0" * (len(s) & 1) for s in strips]           # (every strip starts on a word boundary)
            extra = desc if k == 0 else b""
            entries = [(256, 4, 1, cols), (257, 4, 1, rows), (258, 3, 1, item * 8), (259, 3, 1, 8), (262, 3, 1, 1), (277, 3, 1, 1),
                       (278, 4, 1, rowsperstrip), (339, 3, 1, 1)]
            if predictor == 2:
                entries.append((317, 3, 1, 2))
            ifd_size = 2 + 12 * (len(entries) + 2 + (1 if extra else 0)) + 4
            tables_at = offset + ifd_size                                   # offsets, then byte counts: LONGs (inline when one strip)
            table_bytes = 8 * n_strips if n_strips > 1 else 0
            extra_at = tables_at + table_bytes
            data_at = extra_at + len(extra)
            starts = [data_at + sum(len(s) for s in strips[:i]) for i in range(n_strips)]
            end = data_at + sum(len(s) for s in strips)
            if end >= 2 ** 32:
                raise ValueError("save_tiff: classic TIFF holds less than 4 GiB; split the movie")
            entries.append((273, 4, n_strips, tables_at if n_strips > 1 else starts[0]))
            entries.append((279, 4, n_strips, tables_at + 4 * n_strips if n_strips > 1 else sizes[0]))
            if extra:
                entries.append((270, 2, len(extra), extra_at))
            entries.sort()
            nxt = end if k + 1 < n_pages else 0
            fh.write(struct.pack("<H", len(entries)))
            for tag, typ, cnt, val in entries:
                fh.write(struct.pack("<HHII", tag, typ, cnt, val))
            fh.write(struct.pack("<I", nxt))
            if n_strips > 1:
                fh.write(struct.pack("<%dI" % n_strips, *starts) + struct.pack("<%dI" % n_strips, *sizes))
            fh.write(extra)
            fh.write(b"".join(strips))
            offset = nxt
    return


def write_tiff_strips(path, shape, axes, dtype, rowsperstrip, pages, bigtiff=None):
    """A deflate-strip TIFF from strips that are compressed ALREADY (movie.export_tiff: zlib streams made on the GPUs).  shape: the
    whole array's, (..., Y, X), every leading index one page in C order; dtype uint8 or uint16; `pages` yields, per page, the list
    of its finished strip streams (one per `rowsperstrip` rows, the last strip the rows that are left).  Pages are written as they
    arrive; nothing but the current page is held.

    The layout is save_tiff(compression="zlib")'s: little-endian, Compression 8, no Predictor tag, per page the strip offsets and
    byte counts behind the IFD (inline for one strip), then the strips on word boundaries; "axes=... shape=..." in page 0's
    ImageDescription.  bigtiff=True writes BigTIFF (magic 43, 8-byte offsets and counts); None chooses it when the classic form
    would reach 4 GiB -- from the strips themselves when `pages` is a list, otherwise, the sizes not being known before the first
    page is written, from the uncompressed size.  A classic file that reaches 4 GiB after all raises ValueError."""
    import struct
    dtype = np.dtype(dtype)
    if dtype not in (np.uint8, np.uint16):
        raise TypeError("write_tiff_strips writes uint8 / uint16 pages (got %s)" % dtype)
    shape = tuple(int(v) for v in shape)
    if len(shape) < 2 or min(shape) < 1:
        raise ValueError("write_tiff_strips needs a shape (..., Y, X) of positive extents, not %r" % (shape,))
    rows, cols = shape[-2:]
    n_pages = int(np.prod(shape[:-2], dtype=np.int64))
    rowsperstrip = int(rowsperstrip)
    if rowsperstrip < 1:
        raise ValueError("write_tiff_strips: rowsperstrip %d" % rowsperstrip)
    rowsperstrip = min(rowsperstrip, rows)
    n_strips = -(-rows // rowsperstrip)
    desc = ("axes=%s shape=%s" % (axes, "x".join(str(v) for v in shape))).encode("ascii") + b"\0"
    desc += b"\0" * (len(desc) & 1)
    if bigtiff is None:
        if isinstance(pages, (list, tuple)):
            payload = sum(len(s) + (len(s) & 1) for page in pages for s in page)
        else:
            payload = n_pages * rows * cols * dtype.itemsize
        bigtiff = payload + len(desc) + 16 + n_pages * (16 + 20 * 11 + 16 * n_strips) >= 2 ** 32      # (the larger form's tables)
    big = bool(bigtiff)
    # classic: 2-byte entry count, 12-byte entries, LONG (4) offsets; BigTIFF: 8-byte count, 20-byte entries, LONG8 (16) offsets
    cnt_fmt, ent_fmt, off_fmt, off_type, word = ("<Q", "<HHQQ", "Q", 16, 8) if big else ("<H", "<HHII", "I", 4, 4)
    written = 0
    with open(path, "wb") as fh:
        fh.write(struct.pack("<2sHHHQ", b"II", 43, 8, 0, 16) if big else struct.pack("<2sHI", b"II", 42, 8))
        offset = 16 if big else 8
        for k, strips in enumerate(pages):
            if k >= n_pages:
                raise ValueError("write_tiff_strips: more than the %d pages of shape %r" % (n_pages, shape))
            strips = [bytes(s) for s in strips]
            if len(strips) != n_strips:
                raise ValueError("write_tiff_strips: page %d came with %d strips, not %d" % (k, len(strips), n_strips))
            sizes = [len(s) for s in strips]
            extra = desc if k == 0 else b""
            entries = [(256, 4, 1, cols), (257, 4, 1, rows), (258, 3, 1, dtype.itemsize * 8), (259, 3, 1, 8), (262, 3, 1, 1), (277, 3, 1, 1),
                       (278, 4, 1, rowsperstrip), (339, 3, 1, 1)]
            ifd_size = struct.calcsize(cnt_fmt) + struct.calcsize(ent_fmt) * (len(entries) + 2 + (1 if extra else 0)) + word
            tables_at = offset + ifd_size                                   # offsets, then byte counts (inline when one strip)
            table_bytes = 2 * word * n_strips if n_strips > 1 else 0
            extra_at = tables_at + table_bytes
            data_at = extra_at + len(extra)
            starts, at = [], data_at
            for n in sizes:
                starts.append(at)
                at += n + (n & 1)                                           # (every strip starts on a word boundary)
            end = at
            if not big and end >= 2 ** 32:
                raise ValueError("write_tiff_strips: classic TIFF holds less than 4 GiB; pass bigtiff=True")
            entries.append((273, off_type, n_strips, tables_at if n_strips > 1 else starts[0]))
            entries.append((279, off_type, n_strips, tables_at + word * n_strips if n_strips > 1 else sizes[0]))
            if extra:
                entries.append((270, 2, len(extra), extra_at))
            entries.sort()
            nxt = end if k + 1 < n_pages else 0
            fh.write(struct.pack(cnt_fmt, len(entries)))
            for entry in entries:
                fh.write(struct.pack(ent_fmt, *entry))
            fh.write(struct.pack("<" + off_fmt, nxt))
            if n_strips > 1:
                fh.write(struct.pack("<%d%s" % (n_strips, off_fmt), *starts) + struct.pack("<%d%s" % (n_strips, off_fmt), *sizes))
            fh.write(extra)
            for s in strips:
                fh.write(s + b"\0" * (len(s) & 1))
            offset = end
            written += 1
    if written != n_pages:
        raise ValueError("write_tiff_strips: %d pages arrived for shape %r (%d pages)" % (written, shape, n_pages))
    return path


# ---- image sources and the chunk iterator (bim.py:28-159, 478-495) -------------------------------------------------------
# The reference opens everything through aicsimageio (absent in this image).  Here an image source is anything that can
# say its (T, C, Z, Y, X) extents and hand out 5-D sub-blocks:
#   * a numpy array / memmap of rank 5 (TCZYX), or a list / tuple of them (one per scene = microscope position);
#   * a path to a .npy file (memory-mapped) or to a TIFF stack of uncompressed or deflate strips (the reader below, lazy:
#     only the pages a block needs are decoded; axes from save_tiff's, tifffile's or ImageJ's ImageDescription);
#   * an object with aicsimageio's interface (set_scene, dims, get_image_dask_data) -- a real AICSImage where that
#     package is installed; any other path is handed to aicsimageio and fails loudly without it.
class ImageDims(tuple):
    """(T, C, Z, Y, X) with aicsimageio-style attribute access (dims.T, dims.C, ...)."""
    __slots__ = ()
    _names = "TCZYX"

    def __new__(cls, t, c, z, y, x):
        return tuple.__new__(cls, (int(t), int(c), int(z), int(y), int(x)))

    def __getattr__(self, name):
        i = ImageDims._names.find(name)
        if i < 0 or len(name) != 1:
            raise AttributeError(name)
        return self[i]


class _ArraySource(object):
    def __init__(self, scenes):
        self.scenes = scenes
        self.scene = 0

    def set_scene(self, series):
        if not (0 <= series < len(self.scenes)):
            raise IndexError("scene %d of %d" % (series, len(self.scenes)))
        self.scene = series

    @property
    def dims(self):
        return ImageDims(*self.scenes[self.scene].shape)

    def block(self, t, c, z, y, x):
        return np.asarray(self.scenes[self.scene][t, c, z, y, x])


class _AicsSource(object):
    def __init__(self, img):
        self.img = img
        self.data = None

    def set_scene(self, series):
        self.img.set_scene(series)
        self.data = None

    @property
    def dims(self):
        d = self.img.dims
        return ImageDims(d.T, d.C, d.Z, d.Y, d.X)

    def block(self, t, c, z, y, x):
        if self.data is None:
            self.data = self.img.get_image_dask_data()
        chunk = self.data[t, c, z, y, x]
        return np.asarray(chunk.compute() if hasattr(chunk, "compute") else chunk)


def _as_tczyx(arr, axes):
    """View of `arr` (axes named by `axes`, a subset of TCZYX in any order) as a 5-D TCZYX array."""
    arr = np.asarray(arr) if not isinstance(arr, np.memmap) else arr
    axes = axes.upper()
    if len(axes) != arr.ndim or any(a not in "TCZYX" for a in axes) or len(set(axes)) != len(axes):
        raise ValueError("axes %r do not describe an array of rank %d" % (axes, arr.ndim))
    order = [axes.index(a) for a in "TCZYX" if a in axes]
    view = np.transpose(arr, order)
    shape, k = [], 0
    for a in "TCZYX":
        if a in axes:
            shape.append(view.shape[k])
            k += 1
        else:
            shape.append(1)
    return view.reshape(shape)


def open_image(source, series=0):
    """The image-source object for `source` (see above), positioned on scene `series`."""
    import os
    if hasattr(source, "block") and hasattr(source, "dims"):
        src = source
    elif hasattr(source, "get_image_dask_data"):
        src = _AicsSource(source)
    elif isinstance(source, (list, tuple)):
        src = _ArraySource([_as_tczyx(a, "TCZYX"[5 - np.ndim(a):]) for a in source])
    elif isinstance(source, np.ndarray):
        src = _ArraySource([_as_tczyx(source, "TCZYX"[5 - source.ndim:])])
    elif isinstance(source, (str, bytes, os.PathLike)):
        path = os.fspath(source)
        ext = os.path.splitext(path)[1].lower()
        if ext == ".npy":
            arr = np.load(path, mmap_mode="r")
            src = _ArraySource([_as_tczyx(arr, "TCZYX"[5 - arr.ndim:])])
        elif ext in (".tif", ".tiff"):
            src = _TiffSource(path)
        else:
            try:
                from aicsimageio import AICSImage
                from aicsimageio.readers import bioformats_reader
            except ImportError as e:
                raise _lib.TissueHipError("reading %r needs aicsimageio (with bioformats), which is not installed: %s; "
                                          "convert the movie to .npy / TIFF or pass an array" % (path, e))
            src = _AicsSource(AICSImage(path, reader=bioformats_reader.BioformatsReader))
    else:
        raise TypeError("cannot open %r as an image" % (type(source),))
    src.set_scene(series)
    return src


def get_image_dimensions(path, series=0):
    """bim.py:80-83."""
    return open_image(path, series).dims


def read_image_in_chunks(path, series=0, dx=0, dy=0, dz=0, dc=0, dt=0, apply_function=None, output=None,
                         **apply_function_params):
    """bim.py:89-159: generator over the (dt, dc, dz, dy, dx) blocks of scene `series`, x fastest, then y, z, c, t.
    Without `apply_function` the blocks themselves are yielded; with it, its result per block -- and, when `output`
    is given, each result is also reshaped into the block's place in `output` (a 5-D TCZYX array, or a list of them when
    the function returns a tuple; an output axis shorter than the image is clipped, which is how the projection's
    z axis of length 1 takes a whole z range).  `path` is any image source of open_image()."""
    src = open_image(path, series)
    ext = src.dims                                    # (T, C, Z, Y, X)
    step = [d if d else e for d, e in zip((dt, dc, dz, dy, dx), ext)]
    starts = [range(0, e, s) for e, s in zip(ext, step)]
    for t in starts[0]:
        for c in starts[1]:
            for z in starts[2]:
                for y in starts[3]:
                    for x in starts[4]:
                        lo = (t, c, z, y, x)
                        hi = tuple(min(a + s, e) for a, s, e in zip(lo, step, ext))
                        chunk = src.block(*[slice(a, b) for a, b in zip(lo, hi)])
                        if apply_function is None:
                            yield chunk
                            continue
                        result = apply_function(chunk, **apply_function_params)
                        if output is None:
                            continue                  # (bim.py:121-146 yields nothing in this case)
                        single = not isinstance(result, tuple)
                        results = [result] if single else list(result)
                        outputs = [output] if single else output
                        for res, out in zip(results, outputs):
                            a = [min(p, n) for p, n in zip(lo, out.shape)]
                            b = [min(q, n) for q, n in zip(hi, out.shape)]
                            box = tuple(slice(p, q) for p, q in zip(a, b))
                            out[box] = np.reshape(res, [q - p for p, q in zip(a, b)])
                        yield result


def _tiff_axes_from_description(desc, npages, rows, cols):
    """(axes, shape) from the first page's ImageDescription: save_tiff's "axes=... shape=...", tifffile's own JSON
    {"shape": [...], "axes": "..."}, ImageJ's hyperstack keys, else a plain page stack."""
    import re
    if desc.startswith("{"):
        import json
        try:
            meta = json.loads(desc)
        except ValueError:
            meta = None
        if isinstance(meta, dict) and isinstance(meta.get("shape"), list) and all(isinstance(v, int) for v in meta["shape"]):
            shape, axes = tuple(meta["shape"]), meta.get("axes")
            if int(np.prod(shape)) == npages * rows * cols and shape[-2:] == (rows, cols):
                if not (isinstance(axes, str) and len(axes) == len(shape)):
                    axes = "Q" * (len(shape) - 2) + "YX"      # (tifffile's name for axes it was not told)
                return axes.upper(), shape
    m = re.search(r"axes=([A-Za-z]*) shape=([0-9x]+)", desc)
    if m and m.group(2):
        shape = tuple(int(v) for v in m.group(2).split("x"))
        if int(np.prod(shape)) == npages * rows * cols:
            return m.group(1).upper(), shape
    if desc.startswith("ImageJ="):
        keys = dict(line.split("=", 1) for line in desc.splitlines() if "=" in line)
        t, z, c = int(keys.get("frames", 1)), int(keys.get("slices", 1)), int(keys.get("channels", 1))
        if t * z * c == npages:
            axes, shape = "", ()
            for name, n in (("T", t), ("Z", z), ("C", c)):
                if n > 1:
                    axes += name
                    shape += (n,)
            return axes + "YX", shape + (rows, cols)
    if npages > 1:
        return "QYX", (npages, rows, cols)           # (tifffile's name for an unknown page axis)
    return "YX", (rows, cols)


TIFF_DEFLATE = (8, 32946)          # Compression: Adobe deflate and the legacy code; both are zlib streams (RFC 1950), one per strip


class TiffPage(object):
    """One IFD of a strip-organised TIFF, as tiff_page_table reads it: no pixel data."""
    __slots__ = ("index", "cols", "rows", "bits", "sample_format", "samples", "compression", "predictor", "rows_per_strip",
                 "offsets", "counts", "tiled", "description")

    @property
    def strips(self):
        return -(-self.rows // self.rows_per_strip)

    def strip_rows(self, k):
        return min(self.rows_per_strip, self.rows - k * self.rows_per_strip)


class TiffTable(object):
    """tiff_page_table's result: the pages, the file's byte order ("<" or ">"), classic or BigTIFF, and the memory map the
    offsets point into."""

    def __init__(self, path, buf, byte_order, big, pages):
        self.path, self.buf, self.byte_order, self.big, self.pages = path, buf, byte_order, big, pages

    @property
    def description(self):
        return self.pages[0].description if self.pages else ""


def tiff_page_table(path):
    """The IFDs of a TIFF / BigTIFF file through a memory map -- extents, bits, sample format, compression, predictor, rows per
    strip, strip offsets and byte counts per page; the file's byte order and flavour -- without touching pixel data."""
    import mmap
    import struct
    with open(path, "rb") as fh:
        try:
            buf = mmap.mmap(fh.fileno(), 0, access=mmap.ACCESS_READ)
        except ValueError:
            buf = b""                         # (an empty file cannot be mapped)
    if len(buf) < 8 or buf[:2] not in (b"II", b"MM"):
        raise ValueError("%s is not a TIFF file" % path)
    bo = "<" if buf[:2] == b"II" else ">"
    magic, = struct.unpack(bo + "H", buf[2:4])
    if magic == 42:                       # classic: 4-byte offsets, 12-byte entries, 2-byte entry count
        big, ifd = False, struct.unpack(bo + "I", buf[4:8])[0]
    elif magic == 43:                     # BigTIFF: 8-byte offsets, 20-byte entries, 8-byte entry count
        big, ifd = True, struct.unpack(bo + "Q", buf[8:16])[0]
    else:
        raise ValueError("%s: not a TIFF / BigTIFF file (magic %d)" % (path, magic))
    sizes = {1: 1, 2: 1, 3: 2, 4: 4, 6: 1, 8: 2, 9: 4, 16: 8, 17: 8}
    codes = {1: "B", 3: "H", 4: "I", 6: "b", 8: "h", 9: "i", 16: "Q", 17: "q"}
    cnt_fmt, ent_size, inline, off_fmt = ("Q", 20, 8, "Q") if big else ("H", 12, 4, "I")
    pages = []
    while ifd:
        hdr = struct.calcsize(cnt_fmt)
        n, = struct.unpack(bo + cnt_fmt, buf[ifd:ifd + hdr])
        tags = {}
        for k in range(n):
            e = buf[ifd + hdr + ent_size * k: ifd + hdr + ent_size * (k + 1)]
            tag, typ = struct.unpack(bo + "HH", e[:4])
            cnt, = struct.unpack(bo + off_fmt, e[4:4 + inline])
            raw = e[4 + inline:]
            if typ not in sizes:
                continue
            nbytes = sizes[typ] * cnt
            at = struct.unpack(bo + off_fmt, raw)[0] if nbytes > inline else 0
            data = raw[:nbytes] if nbytes <= inline else buf[at:at + nbytes]
            tags[tag] = bytes(data) if typ == 2 else struct.unpack(bo + "%d%s" % (cnt, codes[typ]), data)
        ifd, = struct.unpack(bo + off_fmt, buf[ifd + hdr + ent_size * n: ifd + hdr + ent_size * n + inline])
        pg = TiffPage()
        pg.index = len(pages)
        pg.cols, pg.rows, pg.bits = tags[256][0], tags[257][0], tags.get(258, (1,))[0]
        pg.sample_format, pg.samples = tags.get(339, (1,))[0], tags.get(277, (1,))[0]
        pg.compression, pg.predictor = tags.get(259, (1,))[0], tags.get(317, (1,))[0]
        pg.tiled = 322 in tags or 324 in tags
        pg.rows_per_strip = max(1, min(tags.get(278, (pg.rows,))[0], pg.rows))
        pg.offsets = tags.get(273, ())
        pg.counts = tags.get(279, (pg.rows * pg.cols * (pg.bits // 8),) if len(pg.offsets) == 1 else ())
        pg.description = tags[270].split(b"\0")[0].decode("latin-1") if 270 in tags else ""
        pages.append(pg)
    return TiffTable(path, buf, bo, big, pages)


def _tiff_check_page(path, pg):
    """What is read here: strips of one sample per pixel, uncompressed (any 8 / 16 / 32 / 64-bit type) or deflate (8- and 16-bit
    unsigned), predictor 1, or 2 on 8- and 16-bit unsigned.  Anything else raises with the tag value met."""
    where = "%s: page %d" % (path, pg.index)
    if pg.tiled:
        raise ValueError("%s is tiled (TileWidth / TileLength present); only strips are read here" % where)
    if pg.samples != 1:
        raise ValueError("%s: SamplesPerPixel %d; multi-sample pages are not read here" % (where, pg.samples))
    if pg.compression != 1 and pg.compression not in TIFF_DEFLATE:
        names = {5: "LZW", 6: "old JPEG", 7: "JPEG", 32773: "PackBits", 50000: "zstd", 34925: "LZMA"}
        raise ValueError("%s: compression %d%s; only uncompressed (1) and deflate (8, 32946) strips are read here"
                         % (where, pg.compression, " (%s)" % names[pg.compression] if pg.compression in names else ""))
    if pg.predictor not in (1, 2):
        raise ValueError("%s: predictor %d%s; only 1 (none) and 2 (horizontal differencing) are read here"
                         % (where, pg.predictor, " (floating point)" if pg.predictor == 3 else ""))
    plain = pg.compression == 1 and pg.predictor == 1
    if not plain and not (pg.sample_format == 1 and pg.bits in (8, 16)):
        raise ValueError("%s: compressed or differenced pages are read as 8- or 16-bit unsigned only (BitsPerSample %d, SampleFormat %d)"
                         % (where, pg.bits, pg.sample_format))
    if pg.sample_format not in (1, 2, 3) or pg.bits not in (8, 16, 32, 64):
        raise ValueError("%s: BitsPerSample %d, SampleFormat %d are not read here" % (where, pg.bits, pg.sample_format))
    if not plain and (len(pg.offsets) != pg.strips or len(pg.counts) != pg.strips):
        raise ValueError("%s: %d strip offsets and %d byte counts for %d strips" % (where, len(pg.offsets), len(pg.counts), pg.strips))


def _tiff_page_dtype(table, pg):
    return np.dtype("%s%s%d" % (table.byte_order, {1: "u", 2: "i", 3: "f"}[pg.sample_format], pg.bits // 8))


def _tiff_decode_page(table, pg):
    """Page pg as a (rows, cols) array in the FILE's byte order: strips joined (uncompressed) or inflated by zlib one by one, then
    the horizontal predictor undone on native-order samples (libtiff's order: byte swap, then accumulate)."""
    import zlib
    dtype, buf = _tiff_page_dtype(table, pg), table.buf
    if pg.compression == 1:
        raw = b"".join(buf[o:o + c] for o, c in zip(pg.offsets, pg.counts))
    else:
        parts = []
        for k, (o, c) in enumerate(zip(pg.offsets, pg.counts)):
            want = pg.strip_rows(k) * pg.cols * dtype.itemsize
            try:
                part = zlib.decompress(buf[o:o + c])
            except zlib.error as e:
                raise ValueError("%s: page %d strip %d does not inflate: %s" % (table.path, pg.index, k, e))
            if len(part) != want:
                raise ValueError("%s: page %d strip %d inflates to %d bytes, not %d" % (table.path, pg.index, k, len(part), want))
            parts.append(part)
        raw = b"".join(parts)
    plane = np.frombuffer(raw, dtype=dtype, count=pg.rows * pg.cols).reshape(pg.rows, pg.cols)
    if pg.predictor == 2:
        native = dtype.newbyteorder("=")
        plane = np.cumsum(plane.astype(native), axis=1, dtype=native).astype(dtype)
    return plane


def _tiff_checked_table(path):
    table = tiff_page_table(path)
    if not table.pages:
        raise ValueError("%s holds no image" % path)
    first = table.pages[0]
    for pg in table.pages:
        _tiff_check_page(path, pg)
        if (pg.rows, pg.cols, pg.bits, pg.sample_format) != (first.rows, first.cols, first.bits, first.sample_format):
            raise ValueError("%s: pages of different size or type" % path)
    return table


def read_tiff(path):
    """bim.py:28-51: (image, axes, shape, metadata) of a TIFF file.  Self-contained reader for what this package, ImageJ and
    tifffile's defaults write -- classic TIFF and BigTIFF, either byte order, strips of one sample per pixel: uncompressed 8 / 16 /
    32-bit unsigned, signed or float pages, or deflate (compression 8 / 32946, inflated with the standard library's zlib) 8- and
    16-bit unsigned pages, with predictor 1 or 2; pages of one size.  Anything else raises ValueError naming the tag value met."""
    table = _tiff_checked_table(path)
    pages = [_tiff_decode_page(table, pg) for pg in table.pages]
    rows, cols = pages[0].shape
    desc = table.description
    axes, shape = _tiff_axes_from_description(desc, len(pages), rows, cols)
    image = np.stack(pages).astype(pages[0].dtype.newbyteorder("=")).reshape(shape)
    metadata = dict(line.split("=", 1) for line in desc.splitlines() if "=" in line) if desc.startswith("ImageJ=") else None
    return image, axes, image.shape, metadata


class _TiffSource(object):
    """A TIFF stack as a lazy image source: dims from the page table, block() decodes only the pages it is asked for.  The
    description's axes say which page holds which (t, c, z) -- TCZ, ImageJ's TZC or any other order of the page axes."""

    def __init__(self, path):
        self.table = _tiff_checked_table(path)
        first = self.table.pages[0]
        axes, shape = _tiff_axes_from_description(self.table.description, len(self.table.pages), first.rows, first.cols)
        axes = axes if axes else "TCZYX"[5 - len(shape):]
        if (len(axes) != len(shape) or any(a not in "TCZYX" for a in axes) or len(set(axes)) != len(axes) or axes[-2:] != "YX"):
            raise ValueError("axes %r do not describe an array of rank %d" % (axes, len(shape)))
        self.axes, self.shape = axes, tuple(int(v) for v in shape)
        self.page_axes, self.page_shape = axes[:-2], self.shape[:-2]
        self.dtype = _tiff_page_dtype(self.table, first).newbyteorder("=")
        self._decoded = {}            # the pages of the last block(): the chunk iterator asks for the same pages x by x, y by y

    def set_scene(self, series):
        if series != 0:
            raise IndexError("scene %d of 1" % series)

    @property
    def dims(self):
        ext = dict(zip(self.axes, self.shape))
        return ImageDims(*[ext.get(a, 1) for a in "TCZYX"])

    def page_index(self, t, c, z):
        """the page that holds plane (t, c, z)"""
        at = dict(T=t, C=c, Z=z)
        k = 0
        for a, n in zip(self.page_axes, self.page_shape):
            k = k * n + at[a]
        return k

    def block(self, t, c, z, y, x):
        d = self.dims
        ts, cs, zs = (range(*s.indices(n)) if isinstance(s, slice) else [s] for s, n in zip((t, c, z), d[:3]))
        last, self._decoded = self._decoded, {}

        def plane(ti, ci, zi):
            k = self.page_index(ti, ci, zi)
            if k not in self._decoded:
                self._decoded[k] = last[k] if k in last else _tiff_decode_page(self.table, self.table.pages[k])
            return self._decoded[k]

        planes = [[[plane(ti, ci, zi)[y, x] for zi in zs] for ci in cs] for ti in ts]
        out = np.array(planes, dtype=self.dtype)
        for axis, s in reversed(list(enumerate((t, c, z)))):
            if not isinstance(s, slice):
                out = out.squeeze(axis)           # an integer index drops its axis, as on an array
        return out


def concatenate_time_points(files):
    """bim.py:478-495: the per-movie projection files (.npy, time first) as one uint16 movie.  A later movie with fewer
    channels (axes 1 .. ndim-3) than the first is zero-padded at the FRONT of that axis.  (The reference also means to
    resize frames of a different (Y, X) size but passes skimage a nested tuple and raises there; so does this.)"""
    movies = []
    for f in files:
        img = np.load(f).astype("uint16")
        if movies:
            first = movies[0]
            for dim in range(1, img.ndim - 2):
                missing = first.shape[dim] - img.shape[dim]
                if missing > 0:
                    pad = [(0, 0)] * img.ndim
                    pad[dim] = (missing, 0)
                    img = np.pad(img, pad_width=pad, constant_values=0)
            if img.shape[-2:] != first.shape[-2:]:
                raise ValueError("concatenate_time_points: frame size %s differs from the first movie's %s"
                                 % (img.shape[-2:], first.shape[-2:]))
        movies.append(img)
    return np.concatenate(movies, axis=0)


# ---- the remaining small operators and readers of bim.py -------------------------------------------------------------------
def binary_image(image, axes, thresholds):
    """bim.py:350-369: per channel, values above the threshold become 1, then values below it become 0 -- two passes in that
    order, so for a threshold above 1 the freshly written ones are zeroed again (as upstream) and values EQUAL to the
    threshold keep their value; `thresholds` is a scalar or one value per channel (the first one when the image has no
    channel axis, or the channel axis leads).  An elementwise pass over a display image: host numpy."""
    adjusted = np.copy(image)
    per_channel = hasattr(thresholds, "__len__")
    if axes.find("C") > 0:
        moved, order = put_channel_axis_first(adjusted, axes)
        for channel in range(moved.shape[0]):
            thr = thresholds[channel] if per_channel else thresholds
            plane = moved[channel]
            np.putmask(plane, plane > thr, 1)
            np.putmask(plane, plane < thr, 0)
        return np.transpose(moved, axes=np.argsort(order))
    thr = thresholds[0] if per_channel else thresholds
    np.putmask(adjusted, adjusted > thr, 1)
    np.putmask(adjusted, adjusted < thr, 0)
    return adjusted


def _whole(src):
    T, C, Z, Y, X = src.dims
    return src.block(slice(0, T), slice(0, C), slice(0, Z), slice(0, Y), slice(0, X))


def read_whole_image(path):
    """bim.py:54-57: (data TCZYX, dims, metadata) of the first scene."""
    src = open_image(path)
    return _whole(src), src.dims, getattr(getattr(src, "img", None), "metadata", None)


def read_virtual_image(path):
    """bim.py:59-62: upstream returns the lazy (dask) array; here the source object itself plays that role: index it
    through `.block(t, c, z, y, x)` slices, nothing is read before."""
    src = open_image(path)
    return src, src.dims, getattr(getattr(src, "img", None), "metadata", None)


def read_part_of_image(path, x_range, y_range, z_range, c_range, t_range, dims_order="TCZXY"):
    """bim.py:64-77: a sub-block of the first scene.  Kept as upstream wrote it: the z slice ends at c_range[1] (not
    z_range[1]), and a `dims_order` other than the default transposes the TCZYX block by the index of each letter of
    "TCZXY" in `dims_order`."""
    src = open_image(path)
    data = src.block(slice(t_range[0], t_range[1]), slice(c_range[0], c_range[1]), slice(z_range[0], c_range[1]),
                     slice(y_range[0], y_range[1]), slice(x_range[0], x_range[1]))
    default = "TCZXY"
    if default != dims_order:
        data = np.transpose(data, [dims_order.index(default[i]) for i in range(len(default))])
    return data, src.dims, getattr(getattr(src, "img", None), "metadata", None)


def extract_all_frames_from_a_scene(path, scene_index, max_frames=None):
    """bim.py:497-509: generator over the time points of one scene, each as a (Z, C, Y, X) array (upstream asks its reader for
    "TZCYX" order), at most `max_frames` of them."""
    src = open_image(path, scene_index)
    T, C, Z, Y, X = src.dims
    for t in range(min(T, max_frames) if max_frames else T):
        frame = src.block(slice(t, t + 1), slice(0, C), slice(0, Z), slice(0, Y), slice(0, X))[0]
        yield np.transpose(frame, (1, 0, 2, 3))
    return 0


class _BigTiffAppender(object):
    """Streaming BigTIFF writer (magic 43, 8-byte offsets): every (Y, X) plane appended becomes one page -- uncompressed,
    min-is-black, one strip -- so a movie larger than memory (or than classic TIFF's 4 GiB) can be written frame by frame."""

    def __init__(self, path):
        import struct
        self._s = struct
        self.fh = open(path, "wb")
        self.fh.write(struct.pack("<2sHHHQ", b"II", 43, 8, 0, 0))       # the first-IFD offset (bytes 8..15) is patched later
        self.link = 8                                                  # file position of the pointer to the next IFD

    def write_plane(self, plane):
        s = self._s
        plane = np.ascontiguousarray(plane)
        if plane.ndim != 2 or plane.dtype not in (np.uint8, np.uint16, np.float32, np.int32):
            raise TypeError("BigTIFF pages are 2-D uint8 / uint16 / int32 / float32 planes (got %s %s)" % (plane.dtype, plane.shape))
        rows, cols = plane.shape
        raw = plane.astype(plane.dtype.newbyteorder("<")).tobytes()
        at = self.fh.seek(0, 2)
        at += (-at) % 8
        self.fh.seek(at)
        self.fh.write(raw)
        ifd = at + len(raw)
        ifd += (-ifd) % 8
        fmt = 3 if plane.dtype.kind == "f" else (2 if plane.dtype.kind == "i" else 1)
        entries = [(256, 4, 1, cols), (257, 4, 1, rows), (258, 3, 1, plane.dtype.itemsize * 8), (259, 3, 1, 1), (262, 3, 1, 1),
                   (273, 16, 1, at), (277, 3, 1, 1), (278, 4, 1, rows), (279, 16, 1, len(raw)), (339, 3, 1, fmt)]
        self.fh.seek(ifd)
        self.fh.write(s.pack("<Q", len(entries)))
        for tag, typ, cnt, val in entries:
            self.fh.write(s.pack("<HHQQ", tag, typ, cnt, val))
        nxt = self.fh.tell()
        self.fh.write(s.pack("<Q", 0))
        self.fh.seek(self.link)
        self.fh.write(s.pack("<Q", ifd))
        self.link = nxt

    def close(self):
        self.fh.close()


def virtually_concatenate_time_points(files, position_indices, output_path="output.tif"):
    """bim.py:511-520: stream every time point of scene `position_indices[i] - 1` of `files[i]` into one BigTIFF, one
    (Z, C, Y, X) frame at a time (upstream: tifffile.TiffWriter(bigtiff=True).write per frame): pages in frame, z, channel
    order."""
    out = _BigTiffAppender(output_path)
    try:
        for path, scene in zip(files, position_indices):
            for frame in extract_all_frames_from_a_scene(path, scene - 1):
                for plane in frame.reshape((-1,) + frame.shape[-2:]):
                    out.write_plane(plane)
    finally:
        out.close()
