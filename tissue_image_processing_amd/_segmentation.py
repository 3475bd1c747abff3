"""Device pipelines behind basic_image_manipulations.watershed_segmentation and the labelling helpers."""
import ctypes

import numpy as np

from . import _lib


def _taps(sigma):
    from .basic_image_manipulations import gaussian_taps
    return gaussian_taps(sigma) if float(sigma) > 1e-15 else None


def watershed(image, watershed_line=True, return_flags=False):
    """skimage.segmentation.watershed(image, markers=None, connectivity=1, watershed_line=True) (bim.py:475, pl.py:194).

    flags: bit0 = value ties between non-marker neighbours (serial push-age order not reproduced bit for bit),
    bit1 = two-valued image handled by the generation-synchronous BFS, bits 2.. = global-minimum fallback steps."""
    img = np.ascontiguousarray(image, dtype=np.float64)
    if img.ndim != 2:
        raise ValueError("watershed on MI355X takes 2-D images")
    labels = np.empty(img.shape, np.int32)
    flags = ctypes.c_int32(0)
    _lib.check(_lib.lib().tip_watershed_f64(_lib.ptr(img), _lib.ptr(labels), img.shape[0], img.shape[1],
                                            1 if watershed_line else 0, ctypes.byref(flags)))
    return (labels, flags.value) if return_flags else labels


def watershed_segmentation(image, imgthresh, stdeviation, blocksize, return_flags=False):
    """bim.py:446-476."""
    image = np.asarray(image)
    if image.ndim != 2:
        raise ValueError("watershed_segmentation takes a 2-D image")
    if image.dtype not in (np.float32, np.float64) and not np.issubdtype(image.dtype, np.integer):
        raise TypeError("watershed_segmentation on MI355X takes float or integer images (got %s)" % image.dtype)
    if blocksize % 2 == 0:
        blocksize += 1
    lib = _lib.lib()
    Y, X = image.shape
    labels = np.empty((Y, X), np.int32)
    flags = ctypes.c_int32(0)
    if image.dtype == np.float64:
        img = np.ascontiguousarray(image)
        d_img = _lib.DeviceBuffer(img.nbytes).upload(img)
        d_lab = _lib.DeviceBuffer(labels.nbytes)
        taps = _taps(stdeviation)
        _lib.check(lib.tip_watershed_segmentation_f64_dev(
            d_img.ptr, d_lab.ptr, Y, X, imgthresh, _lib.ptr(taps), 0 if taps is None else taps.size, int(blocksize),
            ctypes.byref(flags)))
        _lib.check(lib.tip_sync())
        labels = d_lab.download((Y, X), np.int32)
        d_img.free()
        d_lab.free()
    else:
        # float32 / integer image: the reference keeps the image dtype through thresholding and blurring
        # (bim.py:463-474); integer-valued landscapes have value ties, see the `flags` bit0 note in watershed()
        from .basic_image_manipulations import blur_image
        img64 = np.ascontiguousarray(image, dtype=np.float64)
        mx = np.empty_like(img64)
        _lib.check(lib.tip_rankfilter2d(_lib.ptr(img64), _lib.ptr(mx), 1, Y, X, blocksize, blocksize, 0, 1, 1))
        seg = np.copy(image)
        seg[seg < imgthresh * mx] = 0
        blurred = blur_image(seg, stdeviation)
        labels, fl = watershed(blurred, True, return_flags=True)
        flags.value = fl
    return (labels, flags.value) if return_flags else labels


def label(input, background=None, return_num=False, connectivity=None):
    """skimage.measure.label for 2-D integer images with connectivity 1 (ti.py:2922, 3470)."""
    a = np.asarray(input)
    if a.ndim != 2:
        raise ValueError("label on MI355X takes 2-D images")
    if connectivity != 1:
        raise NotImplementedError("label on MI355X implements connectivity=1 (what the reference passes)")
    if a.dtype == bool:
        a = a.astype(np.int32)
    if not np.issubdtype(a.dtype, np.integer):
        raise TypeError("label takes integer images")
    if a.size and (a.min() < -2 ** 31 or a.max() > 2 ** 31 - 1):
        raise ValueError("label values must fit int32")
    a32 = np.ascontiguousarray(a, dtype=np.int32)
    bg = 0 if background is None else int(background)
    out = np.empty(a32.shape, np.int32)
    n = ctypes.c_int32(0)
    _lib.check(_lib.lib().tip_label4_i32(_lib.ptr(a32), bg, _lib.ptr(out), a32.shape[0], a32.shape[1], ctypes.byref(n)))
    out = out.astype(np.int64)  # skimage returns the platform integer
    return (out, n.value) if return_num else out


def rank_filter(a, size, footprint_kind=0, mode="reflect", is_max=True):
    a = np.asarray(a)
    if a.ndim != 2:
        raise ValueError("2-D images only")
    if a.dtype == np.float64:
        dt = 1
    elif a.dtype == np.int32:
        dt = 2
    else:
        raise TypeError("rank filters take float64 or int32 images (got %s)" % a.dtype)
    ky, kx = (size, size) if np.isscalar(size) else size
    src = np.ascontiguousarray(a)
    out = np.empty_like(src)
    _lib.check(_lib.lib().tip_rankfilter2d(_lib.ptr(src), _lib.ptr(out), dt, src.shape[0], src.shape[1], int(ky), int(kx),
                                           int(footprint_kind), {"constant": 0, "reflect": 1}[mode], 1 if is_max else 0))
    return out


def maximum_filter(a, size=None, footprint=None, mode="reflect"):
    """scipy.ndimage.maximum_filter for the reference's call shapes (rectangles, and the 3x3 cross footprint)."""
    if footprint is not None:
        return rank_filter(a, 3, 1, mode, True)
    return rank_filter(a, size, 0, mode, True)


def minimum_filter(a, size=None, footprint=None, mode="reflect"):
    if footprint is not None:
        return rank_filter(a, 3, 1, mode, False)
    return rank_filter(a, size, 0, mode, False)


def regionprops_arrays(labels, intensity=None, n=None):
    """Per-label reductions (tip_regionprops_i32) -> dict of arrays over labels 1..n."""
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    if n is None:
        n = int(labels.max()) if labels.size else 0
    area = np.zeros(n, np.int64)
    bbox = np.zeros((n, 4), np.int64)
    sy = np.zeros(n, np.int64)
    sx = np.zeros(n, np.int64)
    pc = np.zeros((n, 3), np.int64)
    inten = None if intensity is None else np.ascontiguousarray(intensity, dtype=np.float64)
    isum = None if intensity is None else np.zeros(n, np.float64)
    if n > 0:
        _lib.check(_lib.lib().tip_regionprops_i32(_lib.ptr(labels), _lib.ptr(inten), labels.shape[0], labels.shape[1], n,
                                                  _lib.ptr(area), _lib.ptr(bbox), _lib.ptr(sy), _lib.ptr(sx), _lib.ptr(pc),
                                                  _lib.ptr(isum)))
    with np.errstate(invalid="ignore", divide="ignore"):
        cy = sy / area
        cx = sx / area
    sq2 = np.sqrt(2.0)
    perim = pc[:, 0] * 1.0 + pc[:, 1] * sq2 + pc[:, 2] * ((1 + sq2) / 2)
    out = dict(label=np.arange(1, n + 1), area=area, bbox=bbox, cy=cy, cx=cx, perimeter=perim)
    if isum is not None:
        with np.errstate(invalid="ignore", divide="ignore"):
            out["intensity_mean"] = isum / area
    return out


def neighbor_pairs(labels, cap=None):
    """Unique (hi, lo) pairs: a pixel labelled lo > 0 whose zero-padded 5x5 maximum is hi (ti.py:1822-1835)."""
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    grow = cap is None   # default capacity: planar label maps have ~3 pairs per cell; noisy maps get a bigger table
    if cap is None:
        cap = max(1024, 16 * (int(labels.max()) + 1))
    while True:
        pairs = np.empty((cap, 2), np.int32)
        n = ctypes.c_int64(0)
        rc = _lib.lib().tip_neighbor_pairs_i32(_lib.ptr(labels), labels.shape[0], labels.shape[1], _lib.ptr(pairs), cap,
                                               ctypes.byref(n))
        if rc == _lib.TIP_ERR_OVERFLOW and grow and cap < 8 * labels.size:
            cap *= 8
            continue
        _lib.check(rc)
        break
    p = pairs[:n.value].astype(np.int64)
    if p.size:
        p = p[np.lexsort((p[:, 1], p[:, 0]))]
    return p


def contact_pairs(labels, cap=None):
    """{(hi, lo): pixels} for the contact-length rule of ti.py:1844-1872: pixels whose cross-footprint maximum of the labels
    is hi and whose cross-footprint minimum (zeros replaced by max + 1) is lo, hi > lo >= 1.  One device pass."""
    pairs, counts = contact_triples(labels, cap)
    return {(int(h), int(l)): int(c) for (h, l), c in zip(pairs.tolist(), counts.tolist())}


def label_order_stats(labels, img, nlab, ranks):
    """(lo, hi): per label l+1 the values of 0-based ranks ranks[l] and ranks[l] + 1 among img's pixels of that label
    (hi == lo when there is no next one); ranks[l] < 0 skips the label.  labels None: one rank over the whole frame."""
    img = np.ascontiguousarray(img, dtype=np.float64)
    ranks = np.ascontiguousarray(ranks, dtype=np.int64)
    lab = None if labels is None else np.ascontiguousarray(labels, dtype=np.int32)
    lo = np.empty(nlab, np.float64)
    hi = np.empty(nlab, np.float64)
    _lib.check(_lib.lib().tip_label_order_stats_f64(_lib.ptr(lab), _lib.ptr(img), img.shape[0], img.shape[1], nlab,
                                                    _lib.ptr(ranks), _lib.ptr(lo), _lib.ptr(hi)))
    return lo, hi


def _lerp_percentile(lo, hi, gamma):
    """numpy's 'linear' percentile from the two neighbouring order statistics (function_base._lerp)."""
    diff = hi - lo
    return np.where(gamma >= 0.5, hi - diff * (1 - gamma), lo + diff * gamma)


def percentile_per_label(labels, img, nlab, counts, q):
    """np.percentile(img[labels == l + 1], q) for every label with counts[l] > 0 (others: nan), exact."""
    counts = np.asarray(counts, dtype=np.int64)
    present = counts > 0
    virt = (counts - 1) * (q / 100.0)
    prev = np.clip(np.floor(virt).astype(np.int64), 0, np.maximum(counts - 1, 0))
    gamma = virt - np.floor(virt)
    lo, hi = label_order_stats(labels, img, nlab, np.where(present, prev, -1))
    hi = np.where(prev + 1 <= counts - 1, hi, lo)
    return np.where(present, _lerp_percentile(lo, hi, gamma), np.nan)


def percentile_frame(img, q):
    """np.percentile(img, q) over all pixels, exact (radix select on the device, numpy's interpolation on the host)."""
    img = np.asarray(img)
    n = img.size
    virt = (n - 1) * (q / 100.0)
    prev = int(np.floor(virt))
    gamma = virt - np.floor(virt)
    lo, hi = label_order_stats(None, img.reshape(1, -1) if img.ndim != 2 else img, 1, np.array([prev], np.int64))
    hi = hi if prev + 1 <= n - 1 else lo
    return float(_lerp_percentile(lo, hi, gamma)[0])


def cell_types_dev(labels_ptr, marker_ptr, y, x, n, percentage_above_threshold, threshold, peak_window_size, peak_taps,
                   type_index, min_cell_area, max_cell_area, out_type_ptr, out_valid_ptr, out_mean_ptr, out_type_map_ptr):
    """calc_cell_types of one frame on device buffers (tip_cell_types_i32_dev), asynchronous on the calling thread's stream.
    Pointers are device addresses: labels int32 (y, x) 1..n, marker float64 (y, x); per row (n) type / valid uint8 and mean
    float64, and the uint8 (y, x) type map.  peak_taps: the sigma-7 taps (host float64 array) when peak_window_size > 0."""
    taps = None if not peak_window_size else np.ascontiguousarray(peak_taps, dtype=np.float64)
    q_over_100 = (100 - percentage_above_threshold) / 100.0      # percentile_per_label's q / 100.0, q = 100 - p
    _lib.check(_lib.lib().tip_cell_types_i32_dev(
        labels_ptr, marker_ptr, y, x, n, q_over_100, threshold, int(peak_window_size), _lib.ptr(taps),
        0 if taps is None else taps.size, int(type_index), min_cell_area, max_cell_area, out_type_ptr, out_valid_ptr,
        out_mean_ptr, out_type_map_ptr))


def _cell_columns(cy, cx, area, type, feat):
    """the table's columns as the C-ABI takes them (float64 / int64 / uint8, contiguous); feat None: no feature column"""
    cy = np.ascontiguousarray(cy, dtype=np.float64)
    cx = np.ascontiguousarray(cx, dtype=np.float64)
    area = np.ascontiguousarray(area, dtype=np.int64)
    type = np.ascontiguousarray(type, dtype=np.uint8)
    feat = None if feat is None else np.ascontiguousarray(feat, dtype=np.float64)
    n = cy.size
    if any(a is not None and a.size != n for a in (cx, area, type, feat)):
        raise ValueError("the cell table's columns differ in length")
    return cy, cx, area, type, feat, n


def window_stats(qy, qx, r2, cy, cx, area, type, feat=None, sel_bit=-1, sel_positive=True):
    """tip_window_stats_f64: per centre (qy[i], qx[i]) the rows with (cx - qx)**2 + (cy - qy)**2 < r2 -> (n_in, area_in, n_sel,
    sum_sel); n_sel / sum_sel count the rows that also pass the type selector (sel_bit -1: all of them)."""
    qy = np.ascontiguousarray(qy, dtype=np.float64).reshape(-1)
    qx = np.ascontiguousarray(qx, dtype=np.float64).reshape(-1)
    if qy.size != qx.size:
        raise ValueError("qy and qx differ in length")
    cy, cx, area, type, feat, n = _cell_columns(cy, cx, area, type, feat)
    m = qy.size
    n_in, area_in, n_sel = np.zeros(m, np.int64), np.zeros(m, np.int64), np.zeros(m, np.int64)
    sum_sel = np.zeros(m, np.float64)
    _lib.check(_lib.lib().tip_window_stats_f64(
        _lib.ptr(qy), _lib.ptr(qx), m, r2, _lib.ptr(cy), _lib.ptr(cx), _lib.ptr(area), _lib.ptr(type), _lib.ptr(feat), n,
        int(sel_bit), 1 if sel_positive else 0, _lib.ptr(n_in), _lib.ptr(area_in), _lib.ptr(n_sel), _lib.ptr(sum_sel)))
    return n_in, area_in, n_sel, sum_sel


SPATIAL_MODES = {"density": 0, "type_fraction": 1, "mean": 2}


def spatial_grid_shape(shape, step):
    """number of grid points range(step // 2, extent, step) per axis"""
    return tuple(len(range(step // 2, int(e), step)) for e in shape)


def spatial_map(shape, step, r2, cy, cx, area, type, feat=None, sel_bit=-1, sel_positive=True, mode="density"):
    """tip_spatial_map_f64: the (Y, X) float64 map of Tissue.calculate_spatial_data and the grid's n_sel counts."""
    Y, X = int(shape[0]), int(shape[1])
    cy, cx, area, type, feat, n = _cell_columns(cy, cx, area, type, feat)
    out = np.empty((Y, X), np.float64)
    n_sel = np.zeros(spatial_grid_shape((Y, X), int(step)), np.int64)
    _lib.check(_lib.lib().tip_spatial_map_f64(
        Y, X, int(step), r2, _lib.ptr(cy), _lib.ptr(cx), _lib.ptr(area), _lib.ptr(type), _lib.ptr(feat), n, int(sel_bit),
        1 if sel_positive else 0, SPATIAL_MODES[mode], _lib.ptr(out), _lib.ptr(n_sel)))
    return out, n_sel


def spatial_map_dev(shape, step, r2, cy_ptr, cx_ptr, area_ptr, type_ptr, feat_ptr, n, sel_bit, sel_positive, mode, map_ptr,
                    n_sel_ptr=None):
    """tip_spatial_map_f64_dev: the same on DEVICE buffers (addresses), asynchronous on the calling thread's stream; the map
    stays in the caller's device buffer map_ptr ((Y, X) float64), the grid's n_sel counts in n_sel_ptr when given."""
    _lib.check(_lib.lib().tip_spatial_map_f64_dev(
        shape[0], shape[1], int(step), r2, cy_ptr, cx_ptr, area_ptr, type_ptr, feat_ptr, n, int(sel_bit),
        1 if sel_positive else 0, SPATIAL_MODES[mode], map_ptr, n_sel_ptr))


def window_stats_dev(qy_ptr, qx_ptr, m, r2, cy_ptr, cx_ptr, area_ptr, type_ptr, feat_ptr, n, sel_bit, sel_positive, n_in_ptr,
                     area_in_ptr, n_sel_ptr, sum_sel_ptr):
    """tip_window_stats_f64_dev: device addresses in and out, asynchronous on the calling thread's stream."""
    _lib.check(_lib.lib().tip_window_stats_f64_dev(
        qy_ptr, qx_ptr, m, r2, cy_ptr, cx_ptr, area_ptr, type_ptr, feat_ptr, n, int(sel_bit), 1 if sel_positive else 0,
        n_in_ptr, area_in_ptr, n_sel_ptr, sum_sel_ptr))


# ---- neighbour-graph features (csrc/tip_graph.hip) ------------------------------------------------------------------------------
GRAPH_MODES = {"all": 0, "valid": 1, "invalid": 2, "type": 3}


def contact_triples(labels, cap=None):
    """tip_contact_pairs_i32 as arrays: ((k, 2) int32 (hi, lo) rows, (k,) int64 pixel counts), in no particular order."""
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    big = int(labels.max()) + 1
    grow = cap is None
    if cap is None:
        cap = max(4096, 16 * big)
    while True:
        pairs = np.empty((cap, 2), np.int32)
        counts = np.empty(cap, np.int64)
        n = ctypes.c_int64(0)
        rc = _lib.lib().tip_contact_pairs_i32(_lib.ptr(labels), labels.shape[0], labels.shape[1], big, _lib.ptr(pairs),
                                              _lib.ptr(counts), cap, ctypes.byref(n))
        if rc == _lib.TIP_ERR_OVERFLOW and grow and cap < 8 * labels.size:
            cap *= 8
            continue
        _lib.check(rc)
        break
    return pairs[:n.value].copy(), counts[:n.value].copy()


def contact_pairs_dev(labels_ptr, y, x, big, pairs_ptr, counts_ptr, cap):
    """tip_contact_pairs_i32_dev: the triples of a DEVICE label map left in device buffers of `cap` rows; returns their number
    (the call waits for the stream)."""
    n = ctypes.c_int64(0)
    _lib.check(_lib.lib().tip_contact_pairs_i32_dev(labels_ptr, y, x, big, pairs_ptr, counts_ptr, cap,
                                                    ctypes.byref(n)))
    return int(n.value)


def _bytes_column(a, n, name):
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=np.uint8).reshape(-1)
    if a.size != n:
        raise ValueError("%s has %d entries for %d rows" % (name, a.size, n))
    return a


def _graph_args(offsets, adj, valid, empty, type, query):
    """the CSR, the per-row bytes and the query rows as the C-ABI takes them; query None: every row"""
    offsets = np.ascontiguousarray(offsets, dtype=np.int32).reshape(-1)
    adj = np.ascontiguousarray(adj, dtype=np.int32).reshape(-1)
    if offsets.size < 1:
        raise ValueError("offsets needs n + 1 entries")
    n = offsets.size - 1
    valid, empty, type = (_bytes_column(a, n, name) for a, name in ((valid, "valid"), (empty, "empty"), (type, "type")))
    query = None if query is None else np.ascontiguousarray(query, dtype=np.int32).reshape(-1)
    m = n if query is None else query.size
    return offsets, adj, n, valid, empty, type, query, m


def _two_calls(entry, head, first, counts, dtypes, want_rows=True):
    """The two-call convention of the entries whose rows have no known length: one call with the per-row outputs `first` (among
    them `counts`, the rows' lengths) and no rows; the exclusive scan of the lengths on the host; a second call that fills one
    zeroed array per dtype at those offsets.  Returns (offsets int64[m + 1], one array per dtype), or () without want_rows."""
    no_rows = (None,) * (1 + len(dtypes))
    _lib.check(entry(*head, *[_lib.ptr(a) for a in first], *no_rows, 0))
    if not want_rows:
        return ()
    off = np.zeros(counts.size + 1, np.int64)
    off[1:] = np.cumsum(counts)
    rows = [np.zeros(int(off[-1]), dt) for dt in dtypes]
    if off[-1]:
        _lib.check(entry(*head, *(None,) * len(first), _lib.ptr(off), *[_lib.ptr(r) for r in rows], off[-1]))
    return (off, *rows)


def _selector(mode, sel_bit):
    return GRAPH_MODES[mode] if isinstance(mode, str) else int(mode), -1 if sel_bit is None else int(sel_bit)


def neighbor_csr(pairs, n, working=None, cap=None):
    """tip_neighbor_csr_i32: (offsets int32[n + 1], adj int32[...]) from (hi, lo) pair rows; working: one byte per row or None."""
    pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    working = _bytes_column(working, int(n), "working")
    cap = 2 * pairs.shape[0] if cap is None else int(cap)
    offsets = np.zeros(int(n) + 1, np.int32)
    adj = np.zeros(cap, np.int32)
    n_adj = ctypes.c_int64(0)
    _lib.check(_lib.lib().tip_neighbor_csr_i32(_lib.ptr(pairs), pairs.shape[0], n, _lib.ptr(working), _lib.ptr(offsets),
                                               _lib.ptr(adj), cap, ctypes.byref(n_adj)))
    return offsets, adj[:n_adj.value].copy()


def neighbor_csr_dev(pairs_ptr, n_pairs, n, working_ptr, offsets_ptr, adj_ptr, cap, want_count=False):
    """tip_neighbor_csr_i32_dev on device addresses; asynchronous unless want_count (then the entry count comes back)."""
    n_adj = ctypes.c_int64(0)
    _lib.check(_lib.lib().tip_neighbor_csr_i32_dev(pairs_ptr, n_pairs, n, working_ptr, offsets_ptr, adj_ptr, cap,
                                                   ctypes.byref(n_adj) if want_count else None))
    return int(n_adj.value) if want_count else None


def graph_counts(offsets, adj, valid, empty, type, query=None, mode="all", sel_bit=None, sel_positive=True):
    """tip_graph_counts_i32: one int64 count per query row (mode "all" / "valid" / "invalid" / "type")."""
    offsets, adj, n, valid, empty, type, query, m = _graph_args(offsets, adj, valid, empty, type, query)
    mode, bit = _selector(mode, sel_bit)
    out = np.zeros(m, np.int64)
    _lib.check(_lib.lib().tip_graph_counts_i32(
        _lib.ptr(offsets), _lib.ptr(adj), n, adj.size, _lib.ptr(valid), _lib.ptr(empty), _lib.ptr(type), _lib.ptr(query), m,
        mode, bit, 1 if sel_positive else 0, _lib.ptr(out)))
    return out


def graph_counts_dev(offsets_ptr, adj_ptr, n, n_adj, valid_ptr, empty_ptr, type_ptr, query_ptr, m, mode, sel_bit, sel_positive, out_ptr):
    mode, bit = _selector(mode, sel_bit)
    _lib.check(_lib.lib().tip_graph_counts_i32_dev(
        offsets_ptr, adj_ptr, n, n_adj, valid_ptr, empty_ptr, type_ptr, query_ptr, m, mode, bit, 1 if sel_positive else 0,
        out_ptr))


def graph_second(offsets, adj, valid, type, query=None, sel_bit=None, sel_positive=True, members=True):
    """tip_graph_second_i32: (sizes int64[m], member_offsets int64[m + 1], members int32[...]) of find_second_order_neighbors;
    members=False: the sizes alone."""
    offsets, adj, n, valid, _, type, query, m = _graph_args(offsets, adj, valid, None, type, query)
    bit = -1 if sel_bit is None else int(sel_bit)
    sizes = np.zeros(m, np.int64)
    head = (_lib.ptr(offsets), _lib.ptr(adj), n, adj.size, _lib.ptr(valid), _lib.ptr(type), _lib.ptr(query), m, bit,
            1 if sel_positive else 0)
    rows = _two_calls(_lib.lib().tip_graph_second_i32, head, (sizes,), sizes, (np.int32,), members)
    return (sizes, *rows) if members else sizes


def graph_second_dev(offsets_ptr, adj_ptr, n, n_adj, valid_ptr, type_ptr, query_ptr, m, sel_bit, sel_positive, sizes_ptr,
                     member_offsets_ptr=None, members_ptr=None, members_cap=0):
    _lib.check(_lib.lib().tip_graph_second_i32_dev(
        offsets_ptr, adj_ptr, n, n_adj, valid_ptr, type_ptr, query_ptr, m, -1 if sel_bit is None else int(sel_bit),
        1 if sel_positive else 0, sizes_ptr, member_offsets_ptr, members_ptr, members_cap))


def contact_sums(pairs, counts, offsets, adj, valid, type, query=None, mode="all", sel_bit=None, sel_positive=True, values=False):
    """tip_contact_sums_i32: sums int64[m] of the contact pixels towards the selected neighbours; values=True: (sums,
    value_offsets int64[m + 1], value_labels int32[...], values int64[...]), the selected neighbours ascending by label."""
    offsets, adj, n, valid, _, type, query, m = _graph_args(offsets, adj, valid, None, type, query)
    pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    counts = np.ascontiguousarray(counts, dtype=np.int64).reshape(-1)
    if counts.size != pairs.shape[0]:
        raise ValueError("%d pairs with %d counts" % (pairs.shape[0], counts.size))
    mode, bit = _selector(mode, sel_bit)
    sums, n_sel = np.zeros(m, np.int64), np.zeros(m, np.int64)
    head = (_lib.ptr(pairs), _lib.ptr(counts), counts.size, _lib.ptr(offsets), _lib.ptr(adj), n, adj.size, _lib.ptr(valid),
            _lib.ptr(type), _lib.ptr(query), m, mode, bit, 1 if sel_positive else 0)
    rows = _two_calls(_lib.lib().tip_contact_sums_i32, head, (sums, n_sel), n_sel, (np.int64, np.int32), values)
    if not values:
        return sums
    voff, val, lab = rows
    return sums, voff, lab, val


def contact_sums_dev(pairs_ptr, counts_ptr, n_triples, offsets_ptr, adj_ptr, n, n_adj, valid_ptr, type_ptr, query_ptr, m, mode, sel_bit,
                     sel_positive, sums_ptr, n_sel_ptr=None, value_offsets_ptr=None, values_ptr=None, value_labels_ptr=None, values_cap=0):
    mode, bit = _selector(mode, sel_bit)
    _lib.check(_lib.lib().tip_contact_sums_i32_dev(
        pairs_ptr, counts_ptr, n_triples, offsets_ptr, adj_ptr, n, n_adj, valid_ptr, type_ptr, query_ptr, m, mode, bit,
        1 if sel_positive else 0, sums_ptr, n_sel_ptr, value_offsets_ptr, values_ptr, value_labels_ptr, values_cap))


# ---- hexatic order and neighbour correlations (csrc/tip_order.hip) ----------------------------------------------------------------
def _points(py, px):
    py = np.ascontiguousarray(py, dtype=np.float64).reshape(-1)
    px = np.ascontiguousarray(px, dtype=np.float64).reshape(-1)
    if py.size != px.size:
        raise ValueError("py and px differ in length")
    return py, px


def delaunay_neighbors(py, px, members=True):
    """tip_delaunay_neighbors_f64: (sizes int64[n], member_offsets int64[n + 1], members int32[...]) -- per point the 0-based
    positions of its Delaunay neighbours, ascending; members=False: the sizes alone.  ValueError for a non-finite coordinate and
    for two points with the same coordinates (scipy's Qhull silently drops the later twin)."""
    py, px = _points(py, px)
    n = py.size
    if n > 1 and np.isfinite(py).all() and np.isfinite(px).all() and np.unique(np.stack([py, px], axis=1), axis=0).shape[0] != n:
        raise ValueError("delaunay_neighbors: two points have the same coordinates")
    sizes = np.zeros(n, np.int64)
    head = (_lib.ptr(py), _lib.ptr(px), n)
    rows = _two_calls(_lib.lib().tip_delaunay_neighbors_f64, head, (sizes,), sizes, (np.int32,), members)
    return (sizes, *rows) if members else sizes


def delaunay_neighbors_dev(py_ptr, px_ptr, n, sizes_ptr, member_offsets_ptr=None, members_ptr=None, members_cap=0):
    """tip_delaunay_neighbors_f64_dev: device addresses, asynchronous on the calling thread's stream; no duplicate check."""
    _lib.check(_lib.lib().tip_delaunay_neighbors_f64_dev(py_ptr, px_ptr, n, sizes_ptr, member_offsets_ptr, members_ptr,
                                                         members_cap))


def psin(cy, cx, member_offsets, members, query=None, order=6):
    """tip_psin_f64: float64[m], psi_order of every query row (None: row q) over its 1-based member labels, looked up in cy, cx."""
    cy, cx = _points(cy, cx)
    moff = np.ascontiguousarray(member_offsets, dtype=np.int64).reshape(-1)
    mem = np.ascontiguousarray(members, dtype=np.int32).reshape(-1)
    if moff.size < 1:
        raise ValueError("member_offsets needs m + 1 entries")
    m = moff.size - 1
    query = None if query is None else np.ascontiguousarray(query, dtype=np.int32).reshape(-1)
    if query is not None and query.size != m:
        raise ValueError("%d query rows with %d member rows" % (query.size, m))
    out = np.zeros(m, np.float64)
    _lib.check(_lib.lib().tip_psin_f64(_lib.ptr(cy), _lib.ptr(cx), cy.size, _lib.ptr(query), m, _lib.ptr(moff),
                                       _lib.ptr(mem), mem.size, int(order), _lib.ptr(out)))
    return out


def psin_dev(cy_ptr, cx_ptr, n, query_ptr, m, member_offsets_ptr, members_ptr, n_members, order, out_ptr):
    _lib.check(_lib.lib().tip_psin_f64_dev(cy_ptr, cx_ptr, n, query_ptr, m, member_offsets_ptr, members_ptr, n_members,
                                           int(order), out_ptr))


def graph_neighbor_state(offsets, adj, member, state, query=None):
    """tip_graph_neighbor_state_f64: (nb_sum float64[m], nb_cnt int64[m]) over the neighbours flagged in `member`."""
    offsets, adj, n, member, _, _, query, m = _graph_args(offsets, adj, member, None, None, query)
    if member is None:
        raise ValueError("member is needed")
    state = np.ascontiguousarray(state, dtype=np.float64).reshape(-1)
    if state.size != n:
        raise ValueError("state has %d entries for %d rows" % (state.size, n))
    nb_sum, nb_cnt = np.zeros(m, np.float64), np.zeros(m, np.int64)
    _lib.check(_lib.lib().tip_graph_neighbor_state_f64(
        _lib.ptr(offsets), _lib.ptr(adj), n, adj.size, _lib.ptr(member), _lib.ptr(state), _lib.ptr(query), m, _lib.ptr(nb_sum),
        _lib.ptr(nb_cnt)))
    return nb_sum, nb_cnt


def graph_neighbor_state_dev(offsets_ptr, adj_ptr, n, n_adj, member_ptr, state_ptr, query_ptr, m, nb_sum_ptr, nb_cnt_ptr):
    _lib.check(_lib.lib().tip_graph_neighbor_state_f64_dev(offsets_ptr, adj_ptr, n, n_adj, member_ptr, state_ptr, query_ptr, m,
                                                           nb_sum_ptr, nb_cnt_ptr))


def order_features_dev(py_ptr, px_ptr, n, order, psi_ptr, degree_ptr):
    """tip_order_features_f64_dev: Delaunay degree (int64) and psi_order (float64) of n device points, left in device buffers."""
    _lib.check(_lib.lib().tip_order_features_f64_dev(py_ptr, px_ptr, n, int(order), psi_ptr, degree_ptr))


# ---- the sensory-region filter (csrc/tip_hull.hip) ------------------------------------------------------------------------------------
NoHullError = _lib.NoHullError      # a ValueError: fewer than three distinct points, or all on one line


def _hull_result(rc, hull, n_hull):
    if rc == _lib.TIP_ERR_OVERFLOW:
        raise _lib.TissueHipError("the hull has %d vertices, capacity %d" % (n_hull.value, hull.size))
    _lib.check(rc)
    return hull[:int(n_hull.value)].copy()


def convex_hull(px, py, cap=None):
    """tip_convex_hull_f64: int32 positions of the hull's vertices, counter-clockwise in the (x, y) plane from the lexicographically
    smallest; a point on an edge is no vertex, the lowest position stands for coincident points.  NoHullError (a ValueError) for
    fewer than three distinct points or all on one line, ValueError for a non-finite coordinate.  cap: the list's capacity (the
    number of points by default); a smaller hull list raises TissueHipError naming the size needed."""
    px, py = _points(px, py)
    hull = np.zeros(max(px.size if cap is None else int(cap), 1), np.int32)
    n_hull = ctypes.c_int64(0)
    rc = _lib.lib().tip_convex_hull_f64(_lib.ptr(px), _lib.ptr(py), px.size, _lib.ptr(hull), hull.size if cap is None else int(cap),
                                        ctypes.byref(n_hull))
    return _hull_result(rc, hull, n_hull)


def points_outside_hull(px, py, hull, qx, qy):
    """tip_points_outside_hull_f64: uint8[m], 1 where query (qx, qy) lies strictly outside the convex polygon hull (positions into
    px, py as convex_hull returns them), 0 on its boundary and inside."""
    px, py = _points(px, py)
    qx, qy = _points(qx, qy)
    hull = np.ascontiguousarray(hull, dtype=np.int32).reshape(-1)
    out = np.zeros(qx.size, np.uint8)
    _lib.check(_lib.lib().tip_points_outside_hull_f64(_lib.ptr(px), _lib.ptr(py), px.size, _lib.ptr(hull), hull.size, _lib.ptr(qx),
                                                      _lib.ptr(qy), qx.size, _lib.ptr(out)))
    return out


def invalidate_cells_dev(labels_ptr, types_ptr, n_pix, outside_ptr, n):
    """tip_invalidate_cells_u8_dev on device addresses: types[p] = 255 where outside[labels[p] - 1]; asynchronous."""
    _lib.check(_lib.lib().tip_invalidate_cells_u8_dev(labels_ptr, types_ptr, int(n_pix), outside_ptr, int(n)))


def _sensory_rows(cx, cy, type, valid, empty):
    cx, cy = _points(cx, cy)
    rows = [None if a is None else np.ascontiguousarray(a, dtype=np.uint8).reshape(-1) for a in (type, valid, empty)]
    if (rows[0] is None) != (rows[1] is None):
        raise ValueError("type and valid come together")
    if any(a is not None and a.size != cx.size for a in rows):
        raise ValueError("the rows' columns differ in length")
    return (cx, cy, *rows)


def _sensory_call(entry, head, cx, cy, type, valid, empty):
    n = cx.size
    outside = np.zeros(n, np.uint8)
    hull = np.zeros(max(n, 1), np.int32)
    n_hull = ctypes.c_int64(0)
    rc = entry(*head, _lib.ptr(cx), _lib.ptr(cy), _lib.ptr(type), _lib.ptr(valid), _lib.ptr(empty), n, _lib.ptr(outside),
               _lib.ptr(hull), n, ctypes.byref(n_hull))
    return outside, _hull_result(rc, hull, n_hull)


def sensory_region_dev(labels_ptr, types_ptr, n_pix, cx, cy, type, valid, empty=None):
    """tip_sensory_region_i32_dev: the rows with type == 1, valid == 1 and empty == 0 (host uint8 rows; type and valid None: every
    row) span the hull; -> (outside uint8[n], hull int32[h] of row positions), every row tested, and with labels_ptr / types_ptr
    (DEVICE maps of n_pix pixels; both None: no map) 255 painted on the outside rows' pixels.  NoHullError when there is no hull --
    nothing is painted then --, ValueError for a non-finite centroid."""
    rows = _sensory_rows(cx, cy, type, valid, empty)
    return _sensory_call(_lib.lib().tip_sensory_region_i32_dev, (labels_ptr, types_ptr, int(n_pix)), *rows)


def sensory_region_host(cx, cy, type, valid, empty=None):
    """tip_sensory_region_host: the same selection, hull and test on the CPU (no device), the device forms' checker."""
    rows = _sensory_rows(cx, cy, type, valid, empty)
    return _sensory_call(_lib.load().tip_sensory_region_host, (), *rows)


# ---- event detection of one frame pair (csrc/tip_events.hip) ------------------------------------------------------------------------
def border_rows(labels, n=None):
    """tip_border_rows_i32: uint8[n], 1 where label r + 1 touches the map's border (Tissue.detect_edge_cells as row flags)."""
    labels = np.ascontiguousarray(labels, dtype=np.int32)
    if labels.ndim != 2:
        raise ValueError("border_rows takes a 2-D label map")
    if n is None:
        n = int(labels.max()) if labels.size else 0
    flags = np.zeros(int(n), np.uint8)
    _lib.check(_lib.lib().tip_border_rows_i32(_lib.ptr(labels), labels.shape[0], labels.shape[1], int(n), _lib.ptr(flags)))
    return flags


def border_rows_dev(labels_ptr, y, x, n, flags_ptr):
    """tip_border_rows_i32_dev: device addresses, asynchronous on the calling thread's stream."""
    _lib.check(_lib.lib().tip_border_rows_i32_dev(labels_ptr, y, x, int(n), flags_ptr))


def lookup_exact_dev(labels_ptr, y, x, qy, qx):
    """tip_lookup_i32_dev: int32 labels[qy, qx] of a DEVICE label map at host query points, -1 outside the frame."""
    qy = np.ascontiguousarray(qy, dtype=np.int64).reshape(-1)
    qx = np.ascontiguousarray(qx, dtype=np.int64).reshape(-1)
    if qy.size != qx.size:
        raise ValueError("qy and qx differ in length")
    out = np.empty(qy.size, np.int32)
    _lib.check(_lib.lib().tip_lookup_i32_dev(labels_ptr, y, x, _lib.ptr(qy), _lib.ptr(qx), qy.size, _lib.ptr(out)))
    return out


EVENT_OUTPUTS = (("delam", np.uint8), ("diff", np.uint8), ("division", np.uint8), ("n_match", np.int32), ("mother_row", np.int32))


def _event_frame(frame, more=()):
    """one frame's rows as the C-ABI takes them: id int64, sel / pos uint8, the CSR int32, then the columns named in `more`"""
    ids = np.ascontiguousarray(frame["id"], dtype=np.int64).reshape(-1)
    n = ids.size
    offsets = np.ascontiguousarray(frame["offsets"], dtype=np.int32).reshape(-1)
    adj = np.ascontiguousarray(frame["adj"], dtype=np.int32).reshape(-1)
    if offsets.size != n + 1:
        raise ValueError("offsets has %d entries for %d rows" % (offsets.size, n))
    out = dict(id=ids, sel=_bytes_column(frame["sel"], n, "sel"), pos=_bytes_column(frame["pos"], n, "pos"), offsets=offsets, adj=adj)
    for name, dtype in more:
        out[name] = np.ascontiguousarray(frame[name], dtype=dtype).reshape(-1)
        if out[name].size != n:
            raise ValueError("%s has %d entries for %d rows" % (name, out[name].size, n))
    sel_ids = ids[out["sel"] != 0]
    if np.unique(sel_ids).size != sel_ids.size:
        raise ValueError("event_flags: an id occurs twice among a frame's valid, non-empty rows")
    return out


def event_flags(prev, cur, first_edge_ids):
    """tip_event_flags_i32 for one frame pair.  prev: dict(id, sel, pos, offsets, adj); cur: the same plus edge and under; ->
    dict(delam, diff uint8 over the previous rows; division uint8, n_match, mother_row int32 over the current rows).  An id that
    occurs twice among a frame's sel rows is a ValueError."""
    p, c = _event_frame(prev), _event_frame(cur, (("edge", np.uint8), ("under", np.int32)))
    first = np.ascontiguousarray(first_edge_ids, dtype=np.int64).reshape(-1)
    sizes = {"delam": p["id"].size, "diff": p["id"].size}
    out = {name: np.zeros(sizes.get(name, c["id"].size), dtype) for name, dtype in EVENT_OUTPUTS}
    _lib.check(_lib.lib().tip_event_flags_i32(
        *[_lib.ptr(p[k]) for k in ("id", "sel", "pos", "offsets", "adj")], p["id"].size, p["adj"].size,
        *[_lib.ptr(c[k]) for k in ("id", "sel", "pos", "offsets", "adj")], c["id"].size, c["adj"].size,
        _lib.ptr(c["edge"]), _lib.ptr(c["under"]), _lib.ptr(first), first.size, *[_lib.ptr(out[name]) for name, _ in EVENT_OUTPUTS]))
    return out


def event_flags_dev(prev_ptrs, n_prev, n_adj_prev, cur_ptrs, n_cur, n_adj_cur, edge_ptr, under_ptr, first_edge_ids_ptr, n_first_edge, out_ptrs):
    """tip_event_flags_i32_dev: device addresses -- prev_ptrs / cur_ptrs = (id, sel, pos, offsets, adj), out_ptrs = (delam, diff,
    division, n_match, mother_row) -- asynchronous on the calling thread's stream; no uniqueness check."""
    _lib.check(_lib.lib().tip_event_flags_i32_dev(*prev_ptrs, n_prev, n_adj_prev, *cur_ptrs, n_cur, n_adj_cur, edge_ptr, under_ptr,
                                                  first_edge_ids_ptr, n_first_edge, *out_ptrs))
