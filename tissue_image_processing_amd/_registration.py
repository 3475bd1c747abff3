"""phase_cross_correlation on MI355X (tip_phase_correlation): the drop-in for the skimage call behind
Tissue.update_drift / calculate_refine_drift (ti.py:1941-2035) and bim.calculate_drift (bim.py:522-536)."""
import numpy as np

from . import _lib


def phase_cross_correlation(reference_image, moving_image, upsample_factor=1, space="real", return_error=True):
    """Returns (shifts, error, phasediff) like skimage 0.18; error and phasediff are not computed (None): the reference
    discards them at every call site (ti.py:1976, 2029; bim.py:533-535)."""
    if space.lower() != "real":
        raise NotImplementedError("only space='real' (the reference's usage)")
    a = np.asarray(reference_image)
    b = np.asarray(moving_image)
    if a.shape != b.shape:
        raise ValueError("images must be same shape")
    if a.ndim != 2:
        raise NotImplementedError("2-D frames only")
    if a.dtype != b.dtype:
        a = a.astype(np.float64)
        b = b.astype(np.float64)
    if a.dtype == np.uint16:
        dt = 3
    elif a.dtype == np.float32:
        dt = 0
    else:
        a = a.astype(np.float64)
        b = b.astype(np.float64)
        dt = 1
    a = np.ascontiguousarray(a)
    b = np.ascontiguousarray(b)
    ny, nx = a.shape
    for n in (ny, nx):
        if n < 2 or n > 4096:
            raise NotImplementedError("MI355X phase correlation takes extents in [2, 4096] (got %dx%d)" % (ny, nx))
    out = np.zeros((1, 4), np.int64)
    _lib.check(_lib.lib().tip_phase_correlation(_lib.ptr(a), _lib.ptr(b), dt, ny, nx, int(upsample_factor), _lib.ptr(out)))
    return _finish_shifts(out, ny, nx, upsample_factor)[0], None, None


def _finish_shifts(out, ny, nx, upsample_factor):
    """skimage's closing arithmetic on the integer peaks the library returns, for n correlations of one extent at once:
    out (n, 4) = whole-pixel peak (row, col), upsampled-DFT peak (row, col); returns the (n, 2) shifts."""
    shape = np.array([ny, nx])
    shifts = out[:, :2].astype(np.float64)
    midpoints = np.array([np.fix(s / 2) for s in shape])
    shifts = np.where(shifts > midpoints, shifts - shape, shifts)
    if upsample_factor > 1:
        uf = float(upsample_factor)
        shifts = np.round(shifts * uf) / uf
        dftshift = np.fix(np.ceil(uf * 1.5) / 2.0)
        maxima = out[:, 2:].astype(np.float64) - dftshift
        shifts = shifts + maxima / uf
    return shifts


_DTYPE_CODES = {"float32": 0, "float64": 1, "uint16": 3}


def phase_cross_correlation_dev(ref_ptr, mov_ptr, ny, nx, upsample_factor=100, dtype="float64"):
    """The same on two device-resident (ny, nx) planes (device addresses); returns the shift array."""
    dt = _DTYPE_CODES[dtype]
    out = np.zeros((1, 4), np.int64)
    _lib.check(_lib.lib().tip_phase_correlation_dev(ref_ptr, mov_ptr, dt, ny, nx, int(upsample_factor), _lib.ptr(out)))
    return _finish_shifts(out, ny, nx, upsample_factor)[0]


# ---- local drifts (ti.py:2149-2175): one refined drift per window of a frame pair ----------------------------------------
def local_drift_windows(shape, step_size=100, window_size=700):
    """The (row0, row1, col0, col1) windows upstream slides over a frame: starts every step_size pixels while
    start < extent - window_size; a window that could not be followed by another whole one runs to the frame's edge."""
    H, W = shape
    out = []
    for r0 in range(0, H - window_size, step_size):
        r1 = H if r0 + step_size + window_size > H else r0 + window_size
        for c0 in range(0, W - window_size, step_size):
            c1 = W if c0 + step_size + window_size > W else c0 + window_size
            out.append((r0, r1, c0, c1))
    return out


def _overlap(n, shift):
    """Offsets (into the previous window, into the current window) and length of the overlap calculate_refine_drift crops
    along one axis for a floored coarse shift (ti.py:1945-1973)."""
    if shift > 0:
        return shift, 0, n - shift
    if shift < 0:
        return 0, -shift, n + shift
    return 0, 0, n


def phase_cross_correlation_windows_dev(ref_ptr, mov_ptr, frame_shape, origins, ny, nx, upsample_factor=100, dtype="float64",
                                        max_batch=0):
    """phase_cross_correlation_dev on n windows of one device-resident frame pair in one call
    (tip_phase_correlation_windows_dev): ref_ptr / mov_ptr are (frame_y, frame_x) planes, window w the ny x nx block at
    origins[w] = (ref row, ref col, mov row, mov col).  Returns the (n, 2) shifts, row w exactly what
    phase_cross_correlation_dev gives on the two cropped windows.  max_batch: windows per pass (0: what fits the library's
    workspace budget); the result does not depend on it."""
    org = np.ascontiguousarray(origins, dtype=np.int32).reshape(-1, 4)
    n = org.shape[0]
    out = np.zeros((n, 4), np.int64)
    _lib.check(_lib.lib().tip_phase_correlation_windows_dev(ref_ptr, mov_ptr, _DTYPE_CODES[dtype], int(frame_shape[0]),
                                                            int(frame_shape[1]), n, _lib.ptr(org), int(ny), int(nx),
                                                            int(upsample_factor), int(max_batch), _lib.ptr(out)))
    return _finish_shifts(out, ny, nx, upsample_factor)


def correlate_windows_by_extent(ref_ptr, mov_ptr, frame_shape, origins, extents, dtype="float64", upsample_factor=100):
    """The (n, 2) shifts of n windows of any extents on one device-resident frame pair: origins (n, 4) as above, extents
    [(ny, nx), ...] per window; one phase_cross_correlation_windows_dev call per distinct extent, in the order of its first
    window (local_drift_windows gives at most four: the edge windows run to the frame's edge)."""
    origins = np.asarray(origins, np.int32).reshape(-1, 4)
    groups = {}
    for i, ext in enumerate(extents):
        groups.setdefault(tuple(ext), []).append(i)
    shifts = np.empty((len(origins), 2), np.float64)
    for (ny, nx), idx in groups.items():
        shifts[idx] = phase_cross_correlation_windows_dev(ref_ptr, mov_ptr, frame_shape, origins[idx], ny, nx, upsample_factor,
                                                          dtype=dtype)
    return shifts


def local_drifts(first_image, second_image, initial_shift_x=0, initial_shift_y=0, step_size=100, window_size=700):
    """[(window, shift_x, shift_y)] in upstream's loop order: Tissue.calculate_refine_drift on every window of the pair
    (ti.py:2152-2166).  Both frames are uploaded once; correlate_windows_by_extent (upsample factor 100) crops the windows out
    of them on the device and returns what the per-window call returns."""
    a = np.asarray(first_image)
    b = np.asarray(second_image)
    if a.shape != b.shape or a.ndim != 2:
        raise ValueError("local_drifts takes two 2-D frames of one shape")
    if a.dtype != b.dtype or a.dtype not in (np.uint16, np.float32, np.float64):
        a = a.astype(np.float64)
        b = b.astype(np.float64)
    a = np.ascontiguousarray(a)
    b = np.ascontiguousarray(b)
    name = {np.dtype(np.uint16): "uint16", np.dtype(np.float32): "float32", np.dtype(np.float64): "float64"}[a.dtype]
    H, W = a.shape
    windows = local_drift_windows((H, W), step_size, window_size)
    if not windows:
        return []
    rx, ry = int(np.floor(initial_shift_x)), int(np.floor(initial_shift_y))
    origins, extents = [], []
    for (r0, r1, c0, c1) in windows:
        pr, cr, ny = _overlap(r1 - r0, rx)
        pc, cc, nx = _overlap(c1 - c0, ry)
        if ny < 2 or nx < 2:
            raise NotImplementedError("MI355X phase correlation takes extents in [2, 4096] (got %dx%d)" % (ny, nx))
        origins.append((r0 + pr, c0 + pc, r0 + cr, c0 + cc))
        extents.append((ny, nx))
    da, db = _lib.DeviceBuffer(a.nbytes).upload(a), _lib.DeviceBuffer(b.nbytes).upload(b)
    try:
        shifts = correlate_windows_by_extent(da.ptr, db.ptr, (H, W), origins, extents, dtype=name)
    finally:
        for buf in (da, db):
            buf.free()
    return [(win, rx + sh[-2], ry + sh[-1]) for win, sh in zip(windows, shifts)]


def sample_local_drift(drifts, rows, cols):
    """local_shifts_x / local_shifts_y of ti.py:2149-2168 at the pixels (rows, cols): the mean of the shifts of the
    windows that contain the pixel, added up in upstream's loop order (NaN where no window does: 0 / 0 upstream)."""
    rows = np.asarray(rows)
    cols = np.asarray(cols)
    sx = np.zeros(rows.shape)
    sy = np.zeros(rows.shape)
    cnt = np.zeros(rows.shape)
    for (r0, r1, c0, c1), dx, dy in drifts:
        inside = (rows >= r0) & (rows < r1) & (cols >= c0) & (cols < c1)
        sx[inside] += dx
        sy[inside] += dy
        cnt[inside] += 1
    with np.errstate(invalid="ignore", divide="ignore"):
        return sx / cnt, sy / cnt


# ---- PIV drift (ti.py:2061-2070): TV-L1 optical flow between two frames -------------------------------------------------
_OF_DTYPES = {np.dtype(np.float32): 0, np.dtype(np.float64): 1, np.dtype(np.uint16): 3, np.dtype(np.uint8): 4}


def _of_args(reference_image, moving_image, prefilter, dtype):
    a = np.asarray(reference_image)
    b = np.asarray(moving_image)
    if a.shape != b.shape:
        raise ValueError("Input images should have the same shape")
    if np.dtype(dtype).char not in 'efdg':
        raise ValueError("Only floating point data type are valid for optical flow")
    if prefilter:
        raise NotImplementedError("optical_flow_tvl1: prefilter=True is not supported on MI355X (the reference never passes it)")
    if np.dtype(dtype) != np.float32:
        raise NotImplementedError("optical_flow_tvl1: only dtype=float32 (the reference's default)")
    if a.ndim != 2:
        raise NotImplementedError("optical_flow_tvl1: 2-D frames only")
    if a.dtype not in _OF_DTYPES:
        a = a.astype(np.float64)
    if b.dtype not in _OF_DTYPES:
        b = b.astype(np.float64)
    if a.dtype != b.dtype:            # each frame converts on its own (skimage's _convert); float64 keeps both exact
        a = a.astype(np.float32) if a.dtype.kind == "f" else _to_unit_f32(a)
        b = b.astype(np.float32) if b.dtype.kind == "f" else _to_unit_f32(b)
    if min(a.shape) < 2:
        raise ValueError("optical_flow_tvl1: frames need at least 2 rows and 2 columns (np.gradient)")
    return np.ascontiguousarray(a), np.ascontiguousarray(b)


def _to_unit_f32(img):
    return np.multiply(img, 1.0 / np.iinfo(img.dtype).max, dtype=np.float32)


def optical_flow_tvl1(reference_image, moving_image, *, attachment=15, tightness=0.3, num_warp=5, num_iter=10, tol=1e-4,
                      prefilter=False, dtype=np.float32):
    """skimage.registration.optical_flow_tvl1 (0.18.3) on MI355X: the (2, M, N) float32 flow, row displacement first.
    prefilter=True, float64 flows and 3-D frames are not supported (NotImplementedError); the reference uses none of them."""
    flow, _ = optical_flow_tvl1_levels(reference_image, moving_image, attachment=attachment, tightness=tightness,
                                       num_warp=num_warp, num_iter=num_iter, tol=tol, prefilter=prefilter, dtype=dtype)
    return flow


def optical_flow_tvl1_levels(reference_image, moving_image, *, attachment=15, tightness=0.3, num_warp=5, num_iter=10,
                             tol=1e-4, prefilter=False, dtype=np.float32):
    """optical_flow_tvl1 that also returns the warps each pyramid level ran (coarse to fine)."""
    a, b = _of_args(reference_image, moving_image, prefilter, dtype)
    flow = np.empty((2,) + a.shape, np.float32)
    warps = np.zeros(10, np.int32)
    _lib.check(_lib.lib().tip_optical_flow_tvl1(_lib.ptr(a), _lib.ptr(b), _OF_DTYPES[a.dtype], a.shape[0], a.shape[1],
                                                attachment, tightness, int(num_warp), int(num_iter), tol, _lib.ptr(flow),
                                                _lib.ptr(warps), 10))
    return flow, [int(w) for w in warps[:pyramid_levels(a.shape)]]


def pyramid_levels(shape):
    """Levels of skimage's get_pyramid(downscale=2, nlevel=10, min_size=16)."""
    n, m = 1, min(shape)
    while n < 10 and m > 32:
        shape = tuple((s + 1) // 2 for s in shape)
        m = min(shape)
        n += 1
    return n


def optical_flow_tvl1_dev(ref_ptr, mov_ptr, ny, nx, flow_ptr, dtype="float32", attachment=15, tightness=0.3, num_warp=5,
                          num_iter=10, tol=1e-4):
    """The same on device-resident (ny, nx) frames; the (2, ny, nx) float32 flow goes to the device address flow_ptr.
    Asynchronous on the calling thread's stream."""
    dt = {"float32": 0, "float64": 1, "uint16": 3, "uint8": 4}[dtype]
    _lib.check(_lib.lib().tip_optical_flow_tvl1_dev(ref_ptr, mov_ptr, dt, ny, nx, attachment, tightness, int(num_warp),
                                                    int(num_iter), tol, flow_ptr, None, 0))


# ---- PIV step of the sharded movie tracker (movie.process_movie(use_piv=True); ti.py:2061-2106) ---------------------------
def _piv_rows(prev_table):
    cy = np.ascontiguousarray(prev_table["cy"], dtype=np.float64)
    cx = np.ascontiguousarray(prev_table["cx"], dtype=np.float64)
    present = np.ascontiguousarray(np.asarray(prev_table["area"]) > 0, dtype=np.uint8)
    if not (cy.shape == cx.shape == present.shape) or cy.ndim != 1:
        raise ValueError("piv lookup: cy, cx and area must be 1-D arrays of one length")
    return cy, cx, present


def piv_lookup_dev(prev_ptr, cur_ptr, labels_ptr, ny, nx, prev_table, flow_ptr=None, attachment=15, tightness=0.3,
                   num_warp=5, num_iter=10, tol=1e-4):
    """tip_piv_lookup_max3_i32_dev: the TV-L1 flow between two device-resident float64 (ny, nx) planes (frame t-1, frame t;
    each truncated to uint16 first, as the GUI loads the movie), sampled at the rows of frame t-1's table (dict with cy, cx,
    area) with upstream's transposed indexing, and frame t's 3x3-max-filtered device label map looked up at the moved
    centroids.  Returns int32 hits (-1: outside the frame or an absent row); raises IndexError where numpy would.
    flow_ptr: a device (2, ny, nx) float32 buffer that receives the flow (default: it stays in the library's workspace)."""
    cy, cx, present = _piv_rows(prev_table)
    hit = np.empty(cy.shape, np.int32)
    _lib.check(_lib.lib().tip_piv_lookup_max3_i32_dev(
        prev_ptr, cur_ptr, labels_ptr, ny, nx, _lib.ptr(cy), _lib.ptr(cx), _lib.ptr(present), cy.size, attachment, tightness,
        int(num_warp), int(num_iter), tol, flow_ptr, _lib.ptr(hit)))
    return hit


def piv_sample_dev(flow_ptr, labels_ptr, ny, nx, prev_table):
    """tip_piv_sample_max3_i32_dev: piv_lookup_dev's sampling and look-up on a given device (2, ny, nx) float32 flow."""
    cy, cx, present = _piv_rows(prev_table)
    hit = np.empty(cy.shape, np.int32)
    _lib.check(_lib.lib().tip_piv_sample_max3_i32_dev(flow_ptr, labels_ptr, ny, nx, _lib.ptr(cy), _lib.ptr(cx),
                                                      _lib.ptr(present), cy.size, _lib.ptr(hit)))
    return hit
