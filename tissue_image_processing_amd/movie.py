"""Frame-sharded time-lapse processing: one process per GPU, frame t -> rank t % world.

Every per-frame stage (projection, segmentation, cell tables) is independent, so the data path needs no
collective.  The one exchange step is track stitching (tissue_info.track_cells_iterator, ti.py:2037-2113):

  1. all ranks all-gather the small per-frame centroid tables (cy, cx; a few thousand rows per frame);
  2. the rank that owns frame t looks the drift-corrected centroids of frame t-1 up in ITS resident label map
     (3x3 max-filtered, ti.py:2081) -- the only dense-array part of the tracker stays next to the data;
  3. the resulting index arrays (one int per cell) are gathered to rank 0 (RCCL gather = grouped send/recv over
     xGMI, a direct all-to-one, KBs per frame), which runs the sequential id propagation.

With `estimate_drift=True` the frame-to-frame drift (Tissue.update_drift, ti.py:1982-2035) is computed inside the
sharded driver as well: the owner of frame t needs frame t-1's reference-channel projection, which lives on rank
(t-1) % world -- one point-to-point transfer of a (Y, X) float64 plane per frame (33.5 MB at 2048^2, rank r -> r+1 over
xGMI, all pairs at once) -- and runs the phase correlation next to its own plane.  `stitcher="linker"` replaces the
label-lookup tracker by the trackpy-model linker (ti.py:1881-1933, linking.FrameLinker) on rank 0, after the last round;
`stitcher="device_linker"` is that linker with its link finding on the GPU (linking.DeviceFrameLinker, tip_link_frame_f64), fed
round by round while the next round computes.

With `use_piv=True` the same plane exchange feeds the tracker's PIV mode (ti.py:2061-2106) instead: the owner of frame t
runs the TV-L1 flow from frame t-1's plane to its own (both truncated to uint16 first, as the GUI loads the movie), samples
it at frame t-1's centroids with upstream's transposed indexing and looks the moved centroids up in its label map -- one
device call per frame (tip_piv_lookup_max3_i32_dev), the flow never leaves the GPU.  Drifts are not written.

With `local_drifts=...` the drift is a MAP (Tissue.fix_one_frame_tracking_using_local_drifts, ti.py:2149-2173): the owner of
frame t correlates every window of the pair (frame t-1's plane, its own) in one batched device call per window extent
(tip_phase_correlation_windows_dev), and every centroid of frame t-1 moves by the mean shift of the windows that contain it
before it is looked up -- the mode between one rigid shift and the dense flow.  The window shifts stay on the owner
(backend.local_drifts[t]).

With `GpuFrameBackend(cell_types=...)` the owner of frame t also classifies its cells as calc_cell_types does (ti.py:2338-2408)
on the resident labels and Atoh-channel projection (one device call, tip_cell_types_i32_dev): the per-row columns type, valid
and mean_intensity, named in the backend's `extra_columns`, travel with the centroid tables, and the type map stays on the
owner GPU next to the label map.

With `GpuFrameBackend(cell_types=..., sensory_region=True)` the owner then applies the GUI's "remove non-sensory cells" step
(Tissue.remove_cells_outside_of_sensory_region, ti.py:2781-2792) to the frame, right after its typing and before everything that
reads `valid` or the type map: the convex hull of the hair cells' centroids is built on the device, every row outside it gets
valid = 0 and its pixels 255 in the resident type map (one device call, tip_sensory_region_i32_dev).  The frame's dict gains the
column `in_sensory_region`, `backend.sensory_hulls[t]` the hull's rows; a frame whose hair cells span no hull stays unfiltered and
is listed in `backend.sensory_skipped`.  Neighbour and order columns, the archive, events and the exported TIFF follow from the
filtered `valid` and map with no change of their own.

With `GpuFrameBackend(segmentation="unet")` every frame is segmented as the GUI's "use Unet?" path does (gui.py:2059-2063):
network and closing / watershed tail through FramePipeline.segment_unet, whose labels (and, with keep_hc, HC map) come back in
frame orientation (Y, X) and are copied on the device into the buffers the classical segmentation fills, so that every stage
above runs on them unchanged.  Each pipeline has its own predictor and each worker thread its own torch stream.

With `GpuFrameBackend(archive=True)` the owner of frame t also deflates the frame's label map and type map on the device
(tip_deflate_runs_dev, tip_deflate_rows_dev with archive=dict(matches="rows"), tip_deflate_dynamic_dev with codes="dynamic") and keeps the streams and the frame's tables; `save_seg`, called on every rank after `process_movie`, turns
them into the `.seg` archive Tissue.load reads -- the maps never reach the host uncompressed.

`find_events`, called on every rank after `process_movie` like `save_seg`, detects the cell events -- delaminations, divisions,
differentiations (Tissue.find_events_iterator, ti.py:636-789) -- with the label-map reads on the owners' GPUs (tip_border_rows_i32_dev,
tip_lookup_i32_dev) and one device pass per frame pair over the table rows (tip_event_flags_i32); rank 0 gets the events table, which
`save_seg(..., events=...)` writes into the archive (events.py).

`tiff_frame_source(path, decode=...)` is a frame_source over a TIFF stack, deflate-compressed ones included: with
decode="device" a frame arrives as its compressed strips (CompressedFrame) and the owner inflates them on its GPU into the stack
the projection reads (FramePipeline.inflate_stack: tip_inflate_strips_dev, tip_tiff_finish_u16_dev) -- the upload moves the
compressed bytes; a strip that does not inflate raises ValueError on the owner before the frame is projected.

`backend` supplies the per-frame compute so the same driver runs on GPUs (GpuFrameBackend) and, for the
multi-process CPU tests, on a stand-in backend with the gloo process group.
"""

import collections
import threading

import numpy as np

from ._collectives import gather_varlen, pack_records, unpack_records


class CompressedFrame(object):
    """One time point of a deflate-compressed TIFF as tiff_frame_source(decode="device") hands it to GpuFrameBackend: `buffer`, one
    (pinned where a GPU is there) host array holding the frame's compressed strips one after another and, from `table_at` on, the
    strip table -- four int64 per strip: src_off, src_len, dst_off, dst_len, the destinations being the strips' places in the
    (C, Z, Y, X) uint16 stack, whatever the file's page order; `pages` / `strip_of_page`: which page and strip each row is (for
    the error text); `shape`, `predictor` (1 or 2) and `swap_bytes` (the file's byte order is not the host's)."""

    def __init__(self, path, t, buffer, src_bytes, table_at, n_strips, pages, strip_of_page, shape, predictor, swap_bytes, release=None):
        self.path, self.t, self.buffer, self.src_bytes, self.table_at, self.n_strips = path, t, buffer, src_bytes, table_at, n_strips
        self.pages, self.strip_of_page, self.shape, self.predictor, self.swap_bytes = pages, strip_of_page, shape, predictor, swap_bytes
        self._release = release

    @property
    def nbytes(self):
        return self.table_at + 32 * self.n_strips

    def host_ptr(self):
        return self.buffer.data_ptr() if hasattr(self.buffer, "data_ptr") else self.buffer.ctypes.data

    def strips(self):
        """the strip table as an (n, 4) int64 array (a view of the buffer)"""
        raw = self.buffer.numpy() if hasattr(self.buffer, "numpy") else self.buffer
        return raw[self.table_at:self.table_at + 32 * self.n_strips].view(np.int64).reshape(-1, 4)

    def release(self):
        """the buffer goes back to its source (after the upload)"""
        if self._release is not None:
            self._release(self.buffer)
            self._release, self.buffer = None, None


# decode="auto" inflates on the device when a frame has at least this many strips' worth of parallel work (frame bytes over the
# largest strip's bytes; the strip count when strips are equal).  Measured on one MI355X at 2048^2 x 30 x 2 (profiles/
# tiff_inflate_time.json): 7 680 strips of 64 KB -- device 0.065 s a frame against 0.39-0.59 s for zlib on 16 host threads; 60
# strips of 8 MB (one per page) -- device 1.81 s against 0.40 s.  One wave decodes one strip, so the device's time falls as
# 1 / strips and meets the host's at about 60 * 1.81 / 0.40 = 272 strips; the threshold is the next power of two.
AUTO_DEVICE_MIN_STRIPS = 512


def tiff_frame_source(path, series=0, decode="auto", backend="gpu"):
    """A frame_source for process_movie over a TIFF stack: source(t) is time point t as a (C, Z, Y, X) uint16 array
    (decode="host": the strips inflated by zlib on the calling thread) or as a CompressedFrame (decode="device": the compressed
    strips and their table, which GpuFrameBackend uploads and inflates on its GPU, tip_inflate_strips_dev).  decode="auto" is
    "device" when a GPU backend consumes the frames (backend="gpu"), the file is 16-bit deflate strips and a frame holds at
    least AUTO_DEVICE_MIN_STRIPS strips' worth of parallel work, else "host"; 8-bit files are converted on the host.  The source carries `dims` (T, C, Z, Y, X), `decode` and `n_frames`."""
    import threading
    from . import tiff
    from .basic_image_manipulations import open_image
    if decode not in ("auto", "host", "device"):
        raise ValueError("decode must be 'auto', 'host' or 'device', not %r" % (decode,))
    src = open_image(path, series)
    if not isinstance(src, tiff.TiffSource):
        raise ValueError("tiff_frame_source: %r is not a TIFF stack" % (path,))
    T, C, Z, Y, X = src.dims
    table = src.table
    first = table.pages[0]
    device_ok = first.bits == 16 and first.sample_format == 1 and all(pg.compression in tiff.TIFF_DEFLATE for pg in table.pages)
    if decode == "device" and not device_ok:
        raise ValueError("tiff_frame_source: decode='device' needs 16-bit unsigned deflate strips (%s has BitsPerSample %d, compression %d)"
                         % (path, first.bits, first.compression))
    if decode == "auto":
        largest = max(pg.strip_rows(0) for pg in table.pages) * X * 2
        parallel = (C * Z * Y * X * 2) // max(1, largest)
        decode = "device" if (device_ok and backend == "gpu" and parallel >= AUTO_DEVICE_MIN_STRIPS) else "host"
    import sys
    swap = (table.byte_order == "<") != (sys.byteorder == "little")
    lock, spare = threading.Lock(), []

    def take(nbytes):
        with lock:
            for k, b in enumerate(spare):
                if b.shape[0] >= nbytes:
                    return spare.pop(k)
        try:
            import torch
            return torch.empty(nbytes, dtype=torch.uint8, pin_memory=torch.cuda.is_available())
        except ImportError:
            return np.empty(nbytes, np.uint8)

    def give_back(buf):
        with lock:
            if len(spare) < 8:
                spare.append(buf)

    def host_frame(t):
        return np.ascontiguousarray(src.block(slice(t, t + 1), slice(0, C), slice(0, Z), slice(0, Y), slice(0, X))[0], dtype=np.uint16)

    def device_frame(t):
        rows, at = [], 0
        for c in range(C):
            for z in range(Z):
                pg = table.pages[src.page_index(t, c, z)]
                if pg.predictor != first.predictor:
                    raise ValueError("%s: pages with different predictors" % path)
                base = (c * Z + z) * Y * X * 2
                for k, (o, n) in enumerate(zip(pg.offsets, pg.counts)):
                    rows.append((at, n, base + k * pg.rows_per_strip * X * 2, pg.strip_rows(k) * X * 2, pg.index, k, o))
                    at += n
        table_at = (at + 7) & ~7
        buf = take(table_at + 32 * len(rows))
        raw = buf.numpy() if hasattr(buf, "numpy") else buf
        for s_off, n, _, _, _, _, o in rows:
            raw[s_off:s_off + n] = np.frombuffer(table.buf, np.uint8, n, o)
        strips = np.array([r[:4] for r in rows], np.int64).reshape(-1, 4)
        raw[table_at:table_at + strips.nbytes] = strips.view(np.uint8).ravel()
        return CompressedFrame(path, t, buf, at, table_at, len(rows), np.array([r[4] for r in rows]), np.array([r[5] for r in rows]),
                               (C, Z, Y, X), first.predictor, swap, release=give_back)

    source = device_frame if decode == "device" else host_frame
    source.dims, source.decode, source.n_frames = src.dims, decode, T
    return source


class _Job(object):
    """One process_frames call: a shared frame iterator the workers pull from."""

    def __init__(self, it, frame_source, nworkers):
        import threading
        self.it, self.frame_source = it, frame_source
        self.lock, self.done = threading.Lock(), threading.Semaphore(0)
        self.out, self.errors = {}, []


class _FrameWorker(object):
    """A worker thread of GpuFrameBackend with its own library context and FramePipeline, alive until it is sent None."""

    def __init__(self, backend):
        import queue
        import threading
        self.backend = backend
        self.jobs = queue.Queue()
        self.thread = threading.Thread(target=self.run, daemon=True)
        self.thread.start()

    def join(self):
        self.thread.join()

    def run(self):
        from . import _lib
        from .pipeline import FramePipeline
        b = self.backend
        if b.segmentation == "unet":      # the threads do not share torch's default stream: no frame waits for another's network
            import torch
            with torch.cuda.stream(torch.cuda.Stream(b.device)):
                self.serve(b, _lib, FramePipeline)
        else:
            self.serve(b, _lib, FramePipeline)

    def serve(self, b, _lib, FramePipeline):
        pipe, setup_error = None, None
        try:
            _lib.init(b.device)
            pipe = FramePipeline(*b._shape, **b._kw)
        except BaseException as e:
            setup_error = e
        try:
            while True:
                job = self.jobs.get()
                if job is None:
                    return
                try:
                    if setup_error is not None:
                        raise setup_error
                    while True:
                        with job.lock:
                            t = next(job.it, None)
                        if t is None:
                            break
                        job.out[t] = b._process_with(pipe, t, job.frame_source(t))
                except BaseException as e:      # a dead worker must fail the movie, not shorten it silently
                    job.errors.append(e)
                finally:
                    job.done.release()
        finally:
            b._predictors.pop(id(pipe), None)    # (U-Net mode: this pipeline's predictor goes with it)
            pipe = None                          # (its DeviceBuffers go back before the context that launched on them)
            try:
                _lib.load().tip_shutdown()
            except Exception:
                pass


class GpuFrameBackend(object):
    """Per-frame compute on this rank's MI355X through FramePipeline.  What later stages need stays resident per owned
    frame: the int32 label map (tracker look-ups) and, when drift is estimated, the reference channel's projection plane
    -- both kept with device-to-device copies.  The planes are torch tensors so that RCCL can send them as they are.
    close() is what releases process_frames' worker threads and their library contexts: each worker holds its backend, so a
    backend dropped without close() keeps them for the life of the process.

    keep_projection=True also keeps, per owned frame, all C projection planes (float64 (C, Y, X)) and the int64 z-map -- what
    export_projection writes as the projected movie and its z-maps.  That is 8 C Y X + 8 Y X bytes of device memory a frame: 100 MB
    at 2048 x 2048 with C = 2, so a rank's share of a long movie has to fit its GPU (a float32 copy would halve it and is not
    built).  close() frees them."""

    CELL_TYPE_COLUMNS = (("type", np.uint8), ("valid", np.uint8), ("mean_intensity", np.float64))
    CELL_TYPE_OPTIONS = ("atoh_channel", "threshold", "percentage_above_threshold", "peak_window_size", "type_index",
                         "min_cell_area", "max_cell_area")

    SEGMENTATIONS = ("classical", "unet")
    ARCHIVE_MATCHES = ("runs", "rows")
    ARCHIVE_CODES = ("fixed", "dynamic")

    def __init__(self, C, Z, Y, X, device=None, keep_planes=False, inflight=1, cell_types=None, segmentation="classical",
                 unet_weights=None, unet_channels=(1, 0), predictor_factory=None, keep_hc=False, neighbor_features=False,
                 order_features=False, archive=False, keep_projection=False, sensory_region=False, **kw):
        from .pipeline import FramePipeline
        from . import _lib
        # archive: False, True or dict(type_name="HC", matches="runs") -- every frame's label map (and, with cell_types, its type
        # map) is deflated on its own GPU right after the frame's tables (tip_deflate_runs_dev on that frame's pipeline and stream,
        # so it overlaps the other frames in flight) and the stream (about a sixth of the map) is kept on the host in archive_frames[t]
        # together with what cell_tables() found -- area, bbox, coordinate sums, perimeter counts, neighbour pairs -- and the type
        # rows: the parts save_seg turns into the frame's `.seg` members.  type_name: the archive's name of the type cell_types
        # marks.  matches: "runs", or "rows" for matches to the row above as well (tip_deflate_rows_dev with the map's row length:
        # a smaller stream from a slower call).  codes: "fixed", or "dynamic" for per-chunk Huffman codes under either
        # `matches` (tip_deflate_dynamic_dev: a smaller stream again); it is kept beside the dict, in archive_codes.
        if archive is True:
            archive = {}
        if archive is not False and archive is not None and not isinstance(archive, dict):
            raise ValueError("archive must be False, True or dict(type_name=..., matches=..., codes=...)")
        self.archive_codes = "fixed"
        if isinstance(archive, dict):
            archive = dict(archive)
            self.archive_codes = archive.pop("codes", "fixed")
            if self.archive_codes not in self.ARCHIVE_CODES:
                raise ValueError("archive: codes must be one of %s, not %r" % (", ".join(repr(c) for c in self.ARCHIVE_CODES), self.archive_codes))
        self.archive = None if not isinstance(archive, dict) else dict({"type_name": "HC", "matches": "runs"}, **archive)
        if self.archive is not None and set(self.archive) != {"type_name", "matches"}:
            raise ValueError("archive: unknown key(s) %s (known: type_name, matches, codes)" % sorted(set(self.archive) - {"type_name", "matches"}))
        if self.archive is not None and self.archive["matches"] not in self.ARCHIVE_MATCHES:
            raise ValueError("archive: matches must be one of %s, not %r" % (", ".join(repr(m) for m in self.ARCHIVE_MATCHES), self.archive["matches"]))
        if self.archive is not None and (cell_types or {}).get("type_index", 0) != 0:
            raise ValueError("archive: the archive names one type, bit 0 of the type byte (cell_types' type_index must be 0)")
        self.archive_frames = {}   # frame -> dict(labels=(stream, crc), types=(stream, crc) or None, area, bbox, ..., pairs, type rows)
        # segmentation: "classical" (FramePipeline.segment: threshold, blur, watershed on channel 0) or "unet", the GUI's "use
        # Unet?" path (FramePipeline.segment_unet_frame: network + closing / watershed tail on the (atoh, zo) planes
        # unet_channels, labels (Y, X) copied on the device into the pipeline's label buffer).  Every pipeline -- this one and each worker's -- then owns
        # a predictor, built the first time that pipeline segments: predictor_factory(device), by default
        # SegmentationPredictor(unet_weights, (2, X, Y), device=device).  keep_hc: every frame's HC map stays resident (fetch_hc).
        if segmentation not in self.SEGMENTATIONS:
            raise ValueError("segmentation must be one of %s, not %r" % (", ".join(repr(s) for s in self.SEGMENTATIONS), segmentation))
        if segmentation == "classical":
            given = [name for name, v in (("unet_weights", unet_weights), ("predictor_factory", predictor_factory), ("keep_hc", keep_hc))
                     if v is not None and v is not False]
            if given:
                raise ValueError("%s: only with segmentation='unet' (segmentation is one of %s)"
                                 % (", ".join(given), ", ".join(repr(s) for s in self.SEGMENTATIONS)))
        else:
            kw = dict(kw, use_torch=True)      # the projection is a torch tensor the predictor reads in place
        self.segmentation, self.unet_weights, self.unet_channels = segmentation, unet_weights, tuple(unet_channels)
        self.predictor_factory, self.keep_hc = predictor_factory, bool(keep_hc)
        self._predictors = {}   # id(pipeline) -> its SegmentationPredictor (U-Net mode), built on first use
        self.hc_maps = {}       # frame -> DeviceBuffer (float64 HC map (Y, X)), with keep_hc
        self.unet_modes = {}    # frame -> the arithmetic its network pass really ran in (model.last_mode; "miopen": torch's layers, "bf16x6" under f16x3: the range fallback)
        self.ws_flags = {}      # frame -> flags of its tail's watershed (U-Net mode)
        self._shape, self._kw = (C, Z, Y, X), kw
        # cell_types: None, or FramePipeline.cell_types' keyword arguments (atoh_channel, threshold, percentage_above_threshold,
        # peak_window_size, type_index, min_cell_area, max_cell_area) -- every frame is then typed on the device after its
        # cell tables, its dict gains the per-row columns below and its type map stays resident (fetch_cell_types)
        self.cell_types = None if cell_types is None else dict(cell_types)
        unknown = set(self.cell_types or ()) - set(self.CELL_TYPE_OPTIONS)
        if unknown:
            raise ValueError("cell_types: unknown option(s) %s (known: %s)" % (sorted(unknown), ", ".join(self.CELL_TYPE_OPTIONS)))
        self.extra_columns = self.CELL_TYPE_COLUMNS if cell_types is not None else ()
        # sensory_region: every typed frame is then filtered as Tissue.remove_cells_outside_of_sensory_region does (FramePipeline.
        # sensory_region, right after the type call): rows outside the hull of the hair cells -- type == 1, valid == 1, area > 0 --
        # get valid = 0 and 255 on their pixels of the resident type map; the frame's dict gains in_sensory_region (uint8) and
        # sensory_hulls[t] the hull's row positions.  A frame without a hull (fewer than three hair cells, or all on one line) stays
        # unfiltered, its column all ones, and is listed in sensory_skipped; the backend warns once (RuntimeWarning).
        self.sensory_region = bool(sensory_region)
        if self.sensory_region:
            if cell_types is None:
                raise ValueError("sensory_region: the filter needs the frames' cell types (cell_types=...)")
            if self.cell_types.get("type_index", 0) != 0:
                raise ValueError("sensory_region: hair cells are the rows with type == 1, bit 0 alone (cell_types' type_index must be 0)")
            self.extra_columns = tuple(self.extra_columns) + (("in_sensory_region", np.uint8),)
        self.sensory_hulls = {}     # frame -> int32 row positions of its hull's vertices, counter-clockwise
        self.sensory_skipped = []   # frames left unfiltered: their hair cells span no hull; kept in ascending order
        self._sensory_warned = False
        self._sensory_lock = threading.Lock()      # (frames in flight finish on worker threads)
        # neighbor_features: every frame's dict also gains the neighbour-graph columns of FramePipeline.neighbor_features (int64
        # per row), computed after the frame's type call; the hc_* / sc_* columns only together with cell_types.  Without
        # cell_types a row is valid as calculate_frame_cellinfo has it: its area strictly between 0.1 and 10 mean areas.
        self.neighbor_features = bool(neighbor_features)
        if self.neighbor_features:
            from .pipeline import FramePipeline as _FP
            names = _FP.NEIGHBOR_COLUMNS + (_FP.TYPED_NEIGHBOR_COLUMNS if cell_types is not None else ())
            self.extra_columns = tuple(self.extra_columns) + tuple((name, np.int64) for name in names)
        # order_features: every frame's dict also gains FramePipeline.order_features' columns psi6 (float64) and voronoi_neighbors
        # (int64) over its valid rows -- valid as cell_types has them, else by the area rule above; independent of neighbor_features
        self.order_features = bool(order_features)
        if self.order_features:
            self.extra_columns = tuple(self.extra_columns) + tuple(FramePipeline.ORDER_COLUMNS)
        self.device = device
        self.pipe = FramePipeline(C, Z, Y, X, device=device, **kw)
        if device is None:
            self.device = _lib.device_for_thread()
        self.C, self.Y, self.X = C, Y, X
        self.keep_planes = keep_planes
        self.keep_projection = bool(keep_projection)
        self.projections = {}   # frame -> DeviceBuffer (float64 projection planes (C, Y, X)), with keep_projection
        self.zmaps = {}         # frame -> DeviceBuffer (int64 z-map (Y, X)), with keep_projection
        self.inflight = max(1, int(inflight))
        self.labels = {}   # frame -> DeviceBuffer (int32 label map)
        self.planes = {}   # frame -> torch tensor (Y, X) float64 on this GPU
        self.type_maps = {}   # frame -> DeviceBuffer (uint8 type map), with cell_types
        self.local_drifts = {}   # frame -> [(window, row shift, column shift)] of local_drift_lookup
        self._workers = []  # persistent worker threads (process_frames)
        self._event_sets = {}   # frame -> its rows' neighbour sets as the archive's reader iterates them (event_rows)

    def process_frame(self, t, stack_u16):
        return self._process_with(self.pipe, t, stack_u16)

    def process_frames(self, frames, frame_source):
        """All of this rank's frames, `inflight` at a time: worker threads, each with its own HIP stream, workspaces and
        FramePipeline (the library is re-entrant per thread), pull frames from a shared iterator -- one frame's host->device
        upload overlaps the other frames' kernels, and the latency-bound watershed of one overlaps the projection of
        another.  frame_source(t) is called from the worker threads.

        The workers live as long as the backend (process_movie calls this once per round): a thread's library context -- its HIP
        stream, workspace pool and order-statistic state -- and its pipeline buffers are created once and released by close(),
        so a long movie neither re-allocates them every round nor piles up one context per round."""
        import threading
        frames = list(frames)
        if self.inflight <= 1 or len(frames) <= 1:
            return {t: self.process_frame(t, frame_source(t)) for t in frames}
        n = min(self.inflight, len(frames))
        while len(self._workers) < n:
            self._workers.append(_FrameWorker(self))
        job = _Job(iter(frames), frame_source, n)
        for w in self._workers[:n]:
            w.jobs.put(job)
        for _ in range(n):
            job.done.acquire()
        if job.errors:
            raise job.errors[0]
        return job.out

    def close(self):
        """Ends the worker threads; each releases its pipeline buffers and its library context (tip_shutdown) on the way out --
        in U-Net mode its predictor and its torch stream too; this pipeline's predictor goes as well (a later frame builds
        a new one).  The projections and z-maps of keep_projection are freed."""
        workers, self._workers = self._workers, []
        for w in workers:
            w.jobs.put(None)
        for w in workers:
            w.join()
        self._predictors.clear()
        for kept in (self.projections, self.zmaps):
            for buf in kept.values():
                buf.free()
            kept.clear()
        for name in ("_projection_encoder", "_zmap_pages"):
            setattr(self, name, None)

    def _predictor_for(self, p):
        """Pipeline p's own predictor, built on the thread that first segments with p."""
        pred = self._predictors.get(id(p))
        if pred is None:
            if self.predictor_factory is not None:
                pred = self.predictor_factory(self.device)
            else:
                from .prediction_local import SegmentationPredictor
                pred = SegmentationPredictor(self.unet_weights, (2, self.X, self.Y), device=self.device)
            self._predictors[id(p)] = pred
        return pred

    def _segment_unet(self, p, t):
        """Frame t's U-Net segmentation on pipeline p: labels in p.d_labels as (Y, X), as segment() leaves them; the frame's
        network mode and watershed flags are noted, and with keep_hc its HC map is kept like the label map."""
        pred = self._predictor_for(p)
        p.segment_unet_frame(pred, self.unet_channels[0], self.unet_channels[1], keep_hc=self.keep_hc)
        self.unet_modes[t], self.ws_flags[t] = getattr(pred.model, "last_mode", None), int(pred.last_flags)
        if self.keep_hc:
            self.hc_maps[t] = self._keep(p, p.d_hc.ptr, 8)

    def _keep(self, p, src_ptr, itemsize, dst=None, planes=1):
        """A device copy of `planes` (Y, X) maps of pipeline p, on p's stream: into the tensor dst, or a new DeviceBuffer."""
        from . import _lib
        nbytes = planes * self.Y * self.X * itemsize
        keep = _lib.DeviceBuffer(nbytes) if dst is None else dst
        _lib.check(p.lib.tip_memcpy_d2d(keep.ptr if dst is None else dst.data_ptr(), src_ptr, nbytes))
        return keep

    @staticmethod
    def _valid_by_area(area):
        """calculate_frame_cellinfo's rule: a row is valid when its area lies strictly between 0.1 and 10 mean areas."""
        mean = area.mean() if area.size else 0.0
        return (area > 0.1 * mean) & (area < 10 * mean)

    def fetch_hc(self, t):
        """Frame t's HC map (float64 (Y, X): 255 inside the eroded closed class map, 0 elsewhere), downloaded."""
        return self.hc_maps[t].download((self.Y, self.X), np.float64)

    def _process_with(self, p, t, stack_u16):
        from . import _lib
        if isinstance(stack_u16, CompressedFrame):      # a compressed TIFF time point: inflated on this pipeline's stream
            d_stack = p.inflate_stack(stack_u16)
        elif hasattr(stack_u16, "data_ptr"):        # a (pinned) torch tensor: copied straight from its storage
            nbytes = stack_u16.numel() * stack_u16.element_size()
            d_stack = _lib.DeviceBuffer(nbytes)
            _lib.check(p.lib.tip_memcpy_h2d(d_stack.ptr, stack_u16.data_ptr(), nbytes))
        else:
            d_stack = p.upload_stack(stack_u16)
        p.project(d_stack)
        if self.keep_projection:      # (d_proj may be the U-Net mode's torch view: its address is all the copy needs)
            self.projections[t] = self._keep(p, p.d_proj.ptr, 8, planes=self.C)
            self.zmaps[t] = self._keep(p, p.d_zmap.ptr, 8)
        if self.segmentation == "unet":
            self._segment_unet(p, t)
        else:
            p.segment(0)
        self.labels[t] = self._keep(p, p.d_labels.ptr, 4)
        if self.keep_planes:
            import torch
            plane = self.empty_plane()
            # (the block may still be in use by kernels queued on torch's stream: order the library's copy after them)
            _lib.check(p.lib.tip_wait_stream(torch.cuda.current_stream(plane.device).cuda_stream))
            self.planes[t] = self._keep(p, p.d_proj.ptr + p.ref * self.Y * self.X * 8, 8, dst=plane)
        tab = p.cell_tables()          # (synchronises: the small per-cell arrays come to the host)
        d_stack.free()
        area = tab["area"].astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            cy = tab["sumy"] / area
            cx = tab["sumx"] / area
        out = dict(area=tab["area"], cy=np.where(area > 0, cy, 0.0), cx=np.where(area > 0, cx, 0.0))
        if self.cell_types is not None:
            tmap = _lib.DeviceBuffer(self.Y * self.X)      # the frame's type map is painted straight into its own buffer
            out.update(p.cell_types(n=tab["area"].size, type_map_ptr=tmap.ptr, **self.cell_types))   # (synchronises)
            self.type_maps[t] = tmap
        n = tab["area"].size
        if self.sensory_region:
            self._filter_sensory_region(p, t, n, out)
        valid = out["valid"] if self.cell_types is not None else self._valid_by_area(tab["area"])
        if self.neighbor_features:      # (untyped without cell_types: no "type" column)
            out.update(p.neighbor_features(n, valid, out.get("type"), type_index=(self.cell_types or {}).get("type_index", 0)))
        if self.order_features:
            out.update(p.order_features(n, valid, out["cy"], out["cx"]))
        if self.archive is not None:
            self.archive_frames[t] = self._archive_parts(p, t, tab, out)
        return out

    def _filter_sensory_region(self, p, t, n, out):
        """Frame t's sensory-region filter on pipeline p's thread: out's valid becomes the filtered one, out gains
        in_sensory_region, the frame's resident type map is repainted.  No hull: the frame stays as it is, with one warning."""
        from . import _lib
        try:
            res = p.sensory_region(n, out["cy"], out["cx"], out["type"], out["valid"], type_map_ptr=self.type_maps[t].ptr)
        except _lib.NoHullError as e:
            import bisect
            out["in_sensory_region"] = np.ones(n, np.uint8)
            with self._sensory_lock:
                bisect.insort(self.sensory_skipped, t)
                first, self._sensory_warned = not self._sensory_warned, True
            if first:
                import warnings
                warnings.warn("frame %d is left unfiltered, its hair cells span no sensory region (%s); further such frames are "
                              "listed in sensory_skipped without a warning" % (t, e), RuntimeWarning)
            return
        out["in_sensory_region"] = (1 - res["outside"]).astype(np.uint8)
        out["valid"] = (out["valid"] * out["in_sensory_region"]).astype(np.uint8)
        self.sensory_hulls[t] = res["hull"]

    def _archive_parts(self, p, t, tab, out):
        """Frame t's archive parts on pipeline p's thread: the kept label map (int32) and type map (uint8) deflated on the device
        into p's stream buffer, only the streams downloaded, plus the frame's tables as cell_tables() returned them."""
        from . import _lib
        from ._deflate import deflate_dynamic_dev, deflate_rows_dev, deflate_runs_dev, runs_bound
        P = self.Y * self.X
        rows, dynamic = self.archive["matches"] == "rows", self.archive_codes == "dynamic"
        if getattr(p, "_stream_buf", None) is None:
            p._stream_buf = _lib.DeviceBuffer(max(runs_bound(P * 4), 1))
        dst = p._stream_buf

        def encode(src_ptr, nbytes, elem_bytes):
            if dynamic:
                size, crc = deflate_dynamic_dev(src_ptr, nbytes, elem_bytes, self.X * elem_bytes if rows else 0, dst.ptr, dst.nbytes)
            elif rows:
                size, crc = deflate_rows_dev(src_ptr, nbytes, elem_bytes, self.X * elem_bytes, dst.ptr, dst.nbytes)
            else:
                size, crc = deflate_runs_dev(src_ptr, nbytes, elem_bytes, dst.ptr, dst.nbytes)
            return dst.download((size,), np.uint8).tobytes(), crc

        parts = {k: np.array(tab[k]) for k in ("area", "bbox", "sumy", "sumx", "pc", "pairs")}
        parts["labels"] = encode(self.labels[t].ptr, P * 4, 4)
        parts["types"] = None
        if self.cell_types is not None:
            parts["types"] = encode(self.type_maps[t].ptr, P, 1)
            parts.update({k: np.array(out[k]) for k in ("type", "valid", "mean_intensity")})
        return parts

    def fetch_cell_types(self, t):
        """Frame t's type map (uint8 (Y, X): a valid cell's type, 255 on invalid cells and label 0), downloaded."""
        return self.type_maps[t].download((self.Y, self.X), np.uint8)

    def export_page_strips(self, t, ids, rowsperstrip, codes="dynamic"):
        """Frame t's export pages as TIFF strips (export_tiff): the resident label map becomes the uint16 page of track ids
        ids[label - 1] and, when the frame was typed, its type map the page with 0 -> 2 and 255 -> 0 (tip_export_maps_u16_dev); both
        are deflated strip by strip where they are (tip_deflate_strips_dev) and only the streams come to the host -> per page the
        list of its strips' zlib streams.  Called on the thread that owns this backend's pipeline."""
        from .tiff_export import PageEncoder
        if getattr(self, "_page_encoder", None) is None:
            self._page_encoder = PageEncoder(self.Y, self.X)
        types = self.type_maps[t].ptr if self.cell_types is not None else None
        return self._page_encoder.encode(self.labels[t].ptr, types, ids, rowsperstrip, codes)

    def fetch_projection(self, t):
        """Frame t's projection planes (float64 (C, Y, X)), downloaded; needs keep_projection."""
        return self.projections[t].download((self.C, self.Y, self.X), np.float64)

    def fetch_zmap(self, t):
        """Frame t's z-map (int64 (Y, X)), downloaded; needs keep_projection."""
        return self.zmaps[t].download((self.Y, self.X), np.int64)

    def projection_max(self, t):
        """The maximum of frame t's resident projection planes (tip_max_f64_dev): its part of the movie's normalisation."""
        from ._deflate import max_f64_dev
        return max_f64_dev(self.projections[t].ptr, self.C * self.Y * self.X)

    def projection_page_strips(self, t, scale_max, rowsperstrip, codes="dynamic", predictor=1):
        """Frame t's projection planes as TIFF strips (export_projection): the uint16 pages save_tiff(..., data_type="uint16") writes
        for a movie whose maximum is scale_max (tip_projection_pages_u16_dev; differenced along x for predictor 2), deflated strip
        by strip where they are (tip_deflate_strips_dev) -> per channel the list of its strips' zlib streams.  Called on the
        thread that owns this backend's pipeline."""
        from .tiff_export import ProjectionEncoder
        if getattr(self, "_projection_encoder", None) is None:
            self._projection_encoder = ProjectionEncoder(self.C, self.Y, self.X)
        return self._projection_encoder.encode(self.projections[t].ptr, scale_max, rowsperstrip, codes, predictor)

    def zmap_u16(self, t):
        """Frame t's z-map as export_projection saves it: astype("uint16") on the device (tip_zmap_u16_dev), then downloaded."""
        from . import _lib
        from ._deflate import zmap_u16_dev
        if getattr(self, "_zmap_pages", None) is None:
            self._zmap_pages = _lib.DeviceBuffer(self.Y * self.X * 2)
        zmap_u16_dev(self.zmaps[t].ptr, self.Y * self.X, self._zmap_pages.ptr)
        return self._zmap_pages.download((self.Y, self.X), np.uint16)

    def lookup(self, t, qy, qx):
        from . import _lib
        qy = np.ascontiguousarray(qy, dtype=np.int64)
        qx = np.ascontiguousarray(qx, dtype=np.int64)
        out = np.empty(qy.shape, np.int32)
        _lib.check(self.pipe.lib.tip_lookup_max3_i32_dev(self.labels[t].ptr, self.Y, self.X, _lib.ptr(qy), _lib.ptr(qx),
                                                          qy.size, _lib.ptr(out)))
        return out

    # -- events (find_events) ---------------------------------------------------------------------------------
    def lookup_exact(self, t, qy, qx):
        """Frame t's label map at (qy, qx), -1 outside the frame: lookup without the 3x3 maximum (tip_lookup_i32_dev)."""
        from ._segmentation import lookup_exact_dev
        return lookup_exact_dev(self.labels[t].ptr, self.Y, self.X, qy, qx)

    def border_rows(self, t):
        """uint8 per row of frame t: its cell touches the border of the resident label map (tip_border_rows_i32_dev reads the
        2 (Y + X) border pixels; only the flags come to the host)."""
        from . import _lib
        from ._segmentation import border_rows_dev
        n = self._kept(t)["area"].size
        d_flags = _lib.DeviceBuffer(max(n, 1))
        border_rows_dev(self.labels[t].ptr, self.Y, self.X, n, d_flags.ptr)
        flags = d_flags.download((n,), np.uint8)
        d_flags.free()
        return flags

    def _kept(self, t):
        if self.archive is None:
            raise ValueError("the event pass needs the frames' archive parts: GpuFrameBackend(..., archive=True)")
        return self.archive_frames[t]

    def event_rows(self, t):
        """Frame t's rows for the event pass, from its kept parts: sel (valid in the end: by the area rule, or the typing's), pos
        (positive for the archive's type; zeros untyped) and the CSR of exactly the neighbour sets frame_table writes
        (seg_archive.neighbor_sets: with the typing's second pass, which clears the newly valid rows' sets -- built from the sets,
        not from one working mask).  The sets stay with the backend, in the order a reader of the archive iterates them."""
        from .events import as_archived, positive_rows, sets_to_csr
        from .seg_archive import neighbor_sets
        kept = self._kept(t)
        typed = kept.get("types") is not None
        sets, _, _, valid = neighbor_sets(kept, typed)
        self._event_sets[t] = as_archived(sets)
        offsets, adj = sets_to_csr(sets)
        pos = positive_rows(kept["type"]) if typed else np.zeros(valid.size, np.uint8)
        return dict(sel=valid.astype(np.uint8), pos=pos, offsets=offsets, adj=adj)

    def classify_pair(self, t, prev, cur, first_edge_ids):
        """The frame pair (t - 1, t) on this GPU (tip_event_flags_i32): prev / cur are the two frames' rows (id, sel, pos, offsets,
        adj; cur also edge and under), first_edge_ids the first frame's border ids -> the row lists of events.found_rows; a
        division with several matching neighbours takes its mother from frame t's own sets (event_rows(t) came first)."""
        from ._segmentation import event_flags
        from .events import found_rows
        return found_rows(event_flags(prev, cur, first_edge_ids), prev, cur, self._event_sets[t])

    # -- drift (T2) ------------------------------------------------------------------------------------------
    def plane(self, t):
        return self.planes[t]

    def empty_plane(self):
        import torch
        from . import _lib
        return torch.empty((self.Y, self.X), dtype=torch.float64, device=torch.device("cuda", _lib.device_for_thread() or 0))

    def _received(self, what, prev_plane):
        """What every drift step starts with: the backend keeps planes, and the plane received from the neighbour is complete."""
        import torch
        if not self.keep_planes:
            raise ValueError("%s needs the reference-channel planes: GpuFrameBackend(..., keep_planes=True)" % what)
        torch.cuda.current_stream(prev_plane.device).synchronize()

    def piv_lookup(self, t, prev_plane, prev_table):
        """The PIV step of the tracker for frame t (ti.py:2061-2106): TV-L1 flow from frame t-1's reference-channel plane
        (prev_plane, received from the neighbour rank) to frame t's, both truncated to uint16 on the device; frame t-1's
        centroids (prev_table: area, cy, cx) moved by the flow sampled as upstream samples it (row flow at (round(cx),
        round(cy)), numpy's wrap and IndexError rules) and looked up in frame t's 3x3-max-filtered label map.  Returns int32
        hits (-1: outside the frame or an absent row); raises IndexError where upstream's numpy indexing would."""
        from ._registration import piv_lookup_dev
        self._received("piv_lookup", prev_plane)
        return piv_lookup_dev(prev_plane.data_ptr(), self.planes[t].data_ptr(), self.labels[t].ptr, self.Y, self.X, prev_table)

    def local_drift_lookup(self, t, prev_plane, prev_table, step_size=100, window_size=700):
        """The local-drift step of the tracker for frame t >= 1: every window of _registration.local_drift_windows((Y, X),
        step_size, window_size) is correlated between frame t-1's plane (prev_plane) and frame t's -- float64, zero coarse
        shift, upsample factor 100, what drift() does for the whole plane -- in one batched device call per window extent;
        row i of prev_table (area, cy, cx) moves by the mean (row, column) shift of the windows that contain
        (round(cy_i), round(cx_i)) and is looked up in frame t's label map: local_drift_hits.  The window shifts stay in
        self.local_drifts[t] as [(window, row shift, column shift)]."""
        from ._registration import local_drift_windows, correlate_windows_by_extent
        self._received("local_drift_lookup", prev_plane)
        _check_window_fits(self.Y, self.X, window_size)
        windows = local_drift_windows((self.Y, self.X), step_size, window_size)
        shifts = correlate_windows_by_extent(prev_plane.data_ptr(), self.planes[t].data_ptr(), (self.Y, self.X),
                                             [(r0, c0, r0, c0) for r0, _, c0, _ in windows],
                                             [(r1 - r0, c1 - c0) for r0, r1, c0, c1 in windows])
        self.local_drifts[t] = [(win, float(sh[0]), float(sh[1])) for win, sh in zip(windows, shifts)]
        return local_drift_hits(self.local_drifts[t], prev_table, lambda qy, qx: self.lookup(t, qy, qx))

    def drift(self, t, prev_plane):
        """(row shift, column shift) that registers frame t onto frame t-1: Tissue.update_drift without a stage table
        (ti.py:1982-2035 -> calculate_refine_drift with a zero coarse shift -> phase_cross_correlation(upsample 100))."""
        from ._registration import phase_cross_correlation_dev
        self._received("drift", prev_plane)
        sh = phase_cross_correlation_dev(prev_plane.data_ptr(), self.planes[t].data_ptr(), self.Y, self.X, 100)
        return float(sh[0]), float(sh[1])


def local_drift_hits(drifts, prev_table, lookup):
    """The look-up half of the local-drift step.  drifts: [((r0, r1, c0, c1), row shift, column shift)] in window loop order;
    row i of prev_table gets the mean shift of the windows that contain (round(cy_i), round(cx_i)) -- the shifts summed in
    loop order, then one division by the count (ti.py:2165-2169, _registration.sample_local_drift) -- and the result is
    lookup(round(cy - d_row), round(cx - d_col)) as int32.  A point that no window contains (upstream: 0 / 0) finds nothing: -1."""
    from ._registration import sample_local_drift
    cy = np.asarray(prev_table["cy"], dtype=np.float64)
    cx = np.asarray(prev_table["cx"], dtype=np.float64)
    d_row, d_col = sample_local_drift(drifts, np.round(cy).astype(np.int64), np.round(cx).astype(np.int64))
    covered = ~np.isnan(d_row)
    qy = np.where(covered, np.round(cy - np.where(covered, d_row, 0.0)), -1).astype(np.int64)
    qx = np.where(covered, np.round(cx - np.where(covered, d_col, 0.0)), -1).astype(np.int64)
    return np.where(covered, lookup(qy, qx), -1).astype(np.int32)


def _check_window_fits(Y, X, window_size):
    if Y <= window_size or X <= window_size:      # upstream's window loop is then empty and divides 0 by 0
        raise ValueError("local_drifts: the %dx%d frame must exceed window_size %d in both extents" % (Y, X, window_size))


LOCAL_DRIFT_DEFAULTS = dict(step_size=100, window_size=700)      # upstream's (ti.py:2115)


def local_drift_options(local_drifts):
    """None, or the step_size / window_size of process_movie's `local_drifts` (None; True: upstream's; a dict of either)."""
    if local_drifts is None or local_drifts is False:
        return None
    opts = dict(LOCAL_DRIFT_DEFAULTS)
    if local_drifts is not True:
        if not isinstance(local_drifts, dict):
            raise ValueError("local_drifts must be None, True or dict(step_size=..., window_size=...)")
        unknown = set(local_drifts) - set(opts)
        if unknown:
            raise ValueError("local_drifts: unknown key(s) %s (known: step_size, window_size)" % sorted(unknown))
        opts.update(local_drifts)
    opts = {k: int(v) for k, v in opts.items()}
    if opts["step_size"] < 1 or opts["window_size"] < 2:
        raise ValueError("local_drifts: step_size >= 1 and window_size >= 2 (got %(step_size)d, %(window_size)d)" % opts)
    return opts


def assign_track_ids(prev_ids, hit, n_cur, start_ids=None):
    """One step of the label-lookup tracker's id bookkeeping (ti.py:2041-2046, 2092-2106).

    prev_ids[i] = track id of row i of the previous frame; hit[i] = label (row + 1) of the current frame found under
    that row's drift-corrected centroid, 0 / -1 when nothing was hit.  Each previous id is handed on at most once and
    each current row receives at most one id (first occurrence in np.unique order, as upstream); rows left without an
    id get fresh ones above the largest id in use.  With start_ids the step only fills the zeros (first frame)."""
    if start_ids is not None:
        ids = np.asarray(start_ids, dtype=np.int64).copy()
    else:
        ids = np.zeros(n_cur, np.int64)
        row = np.asarray(hit, dtype=np.int64) - 1
        sel = row >= 0
        carried, row = np.asarray(prev_ids)[sel], row[sel]
        _, first = np.unique(carried, return_index=True)      # a previous id is used once ...
        carried, row = carried[first], row[first]
        _, first = np.unique(row, return_index=True)          # ... and a current row is claimed once
        ids[row[first]] = carried[first]
    fresh = ids == 0
    top = ids.max() if ids.size else 0
    ids[fresh] = np.arange(top + 1, top + fresh.sum() + 1)
    return ids


def propagate_ids(tables, lookups):
    """Sequential part of the tracker on rank 0.  tables[t]: dict(area, cy, cx) over row index = label - 1;
    lookups[t] (t >= 1): for every row of frame t-1 the 3x3-max-filtered label of frame t under its drift-corrected
    centroid (-1 = outside / absent row).  Returns the per-frame id arrays as the reference leaves them in cells_info.label."""
    n0 = tables[0]["area"].size
    # calculate_frame_cellinfo leaves label = row + 1 for present rows and 0 for absent ones (ti.py:893)
    first = np.where(tables[0]["area"] > 0, np.arange(1, n0 + 1), 0)
    out = [assign_track_ids(None, None, n0, start_ids=first)]
    for t in range(1, len(tables)):
        out.append(assign_track_ids(out[-1], lookups[t], tables[t]["area"].size))
    return out


def exchange_planes(sends, recvs, backend, rank, world, dist):
    """Plane hand-off for drift estimation: frame t's owner needs frame t-1's reference-channel plane, which lives on rank
    (t-1) % world.  `sends`: this rank's frames whose planes go to rank (rank+1) % world; `recvs`: frames t-1 owned by rank
    (rank-1) % world whose planes arrive here -- both in increasing order on either side of a pair, all pairs at once
    (grouped isend/irecv: over RCCL each pair has its own xGMI link, no ring).  Returns {t: plane of frame t-1}."""
    prev = {}
    if world == 1:
        for t in recvs:
            prev[t + 1] = backend.plane(t)
        return prev
    # gloo (the CPU test harness) moves host tensors only: device planes are staged through the host there; RCCL sends
    # the device planes as they are
    staged = dist.get_backend() == "gloo"
    ops, landing = [], {}
    for t in sends:
        src = backend.plane(t)
        ops.append(dist.P2POp(dist.isend, src.cpu() if staged and src.is_cuda else src, (rank + 1) % world))
    for t in recvs:
        prev[t + 1] = backend.empty_plane()
        landing[t + 1] = prev[t + 1].cpu() if staged and prev[t + 1].is_cuda else prev[t + 1]
        ops.append(dist.P2POp(dist.irecv, landing[t + 1], (rank - 1) % world))
    if ops:
        for req in dist.batch_isend_irecv(ops):
            req.wait()
    for t, buf in landing.items():
        if buf is not prev[t]:
            prev[t].copy_(buf)
    return prev


LINKER_OPTIONS = dict(search_range=100, adaptive_stop=10, adaptive_step=0.95, memory=3)      # ti.py:1881-1933's call


class _IdLinker(object):
    """Track ids from the trackpy-model linker (ti.py:1881-1933), frame after frame: features are the present rows'
    (cy, cx, area) shifted by the cumulative drift; id = particle + 1, absent rows 0."""

    def __init__(self, linker):
        self.linker = linker
        self.total = np.zeros(2)
        self.ids = []

    def add(self, tb, drift):
        """The next frame's table and the drift between the previous frame and it."""
        from .linking import embed
        if self.ids:
            self.total = self.total + np.asarray(drift, dtype=np.float64)
        present = np.flatnonzero(tb["area"] > 0)
        particles = self.linker.link(embed(tb["cy"][present] + self.total[0], tb["cx"][present] + self.total[1], tb["area"][present]))
        ids = np.zeros(tb["area"].size, np.int64)
        ids[present] = np.asarray(particles, dtype=np.int64) + 1
        self.ids.append(ids)


def link_ids(tables, drifts):
    """stitcher="linker": the ids of _IdLinker over all tables on rank 0, with the linker of linking.make_linker (the host's
    unless TISSUE_HIP_LINKER=device)."""
    from .linking import make_linker
    linked = _IdLinker(make_linker(**LINKER_OPTIONS))
    for t, tb in enumerate(tables):
        linked.add(tb, drifts[t])
    return linked.ids


DriftSource = collections.namedtuple("DriftSource", "kind planes local")


def _drift_source(stitcher, estimate_drift, use_piv, local_drifts, backend):
    """The one drift source of a process_movie call; every combination the driver does not run is a ValueError here.  kind:
    "given" (the `drifts` rows), "estimate" (backend.drift), "piv" (backend.piv_lookup) or "local" (backend.local_drift_lookup
    with the options `local`); planes: frame t-1's plane travels to frame t's owner."""
    local = local_drift_options(local_drifts)
    chosen = [kind for kind, on in (("estimate", estimate_drift), ("piv", use_piv), ("local", local is not None)) if on]
    if len(chosen) > 1:
        raise ValueError("estimate_drift, use_piv and local_drifts are three drift sources: pass one of them")
    if stitcher not in ("lookup", "linker", "device_linker"):
        raise ValueError("stitcher must be 'lookup', 'linker' or 'device_linker'")
    kind = chosen[0] if chosen else "given"
    if kind in ("piv", "local"):      # the owner's look-up is the backend's own step
        flag, method = {"piv": ("use_piv", "piv_lookup"), "local": ("local_drifts", "local_drift_lookup")}[kind]
        if stitcher != "lookup":
            raise ValueError("%s needs stitcher='lookup' (the trackpy-model linker has no such mode)" % flag)
        if not hasattr(backend, method) or not getattr(backend, "keep_planes", True):
            raise ValueError("%s needs a backend with %s and planes (GpuFrameBackend(keep_planes=True))" % (flag, method))
    if kind == "local":
        Y, X = getattr(backend, "Y", None), getattr(backend, "X", None)
        if Y is None or X is None:
            raise ValueError("local_drifts needs a backend that knows its frame extents (Y, X)")
        _check_window_fits(Y, X, local["window_size"])
    return DriftSource(kind, kind != "given", local)


def plan_rounds(n_frames, rank, world, block_frames=None):
    """`rank`'s frames per round: round k holds the global frames [k B W, (k+1) B W), B = block_frames (None: the whole shard
    in one round).  Every rank gets the same number of rounds, at least one; a round may leave a rank without a frame."""
    from .pipeline import frames_for_rank
    per_round = (int(block_frames) if block_frames else max(1, -(-n_frames // world))) * world
    rounds = [[] for _ in range(max(1, -(-n_frames // per_round)))]
    for t in frames_for_rank(n_frames, rank, world):
        rounds[t // per_round].append(t)
    return rounds


def _compute_round(frames, frame_source, backend):
    """{t: the backend's dict} for one round's frames of this rank; runs on the driver's compute thread."""
    if hasattr(backend, "process_frames") and frames:      # several frames in flight on this rank's GPU
        return backend.process_frames(frames, frame_source)
    return {t: backend.process_frame(t, frame_source(t)) for t in frames}


def _drift_step(mine, local, drifts, backend, held_planes, source):
    """Writes tables' "drift": the given row, or for the "estimate" source the owner's estimate against the held plane of frame t-1."""
    for t in mine:
        if source.kind == "estimate" and t >= 1:
            drifts[t] = backend.drift(t, held_planes.pop(t))
        local[t]["drift"] = drifts[t].copy()


TABLE_FIELDS = (("area", np.int64), ("cy", np.float64), ("cx", np.float64), ("drift", np.float64))      # then the backend's extra_columns
LOOKUP_FIELDS = (("hits", np.int64),)


def _exchange_tables(mine, local, extra, dist, rank, world, device):
    """The round's cell tables on every rank, {t: dict} (_collectives' records of TABLE_FIELDS + extra, all-gathered).  One
    process: the backend's own dicts, as they are."""
    if world == 1:
        return {t: local[t] for t in mine}
    fields = TABLE_FIELDS + tuple(extra)
    parts = gather_varlen(pack_records({t: local[t] for t in mine}, fields), dist, rank, world, device)
    return {t: tb for part in parts for t, tb in unpack_records(part, fields).items()}


def _owner_lookups(mine, tables, backend, held_planes, source):
    """For each of this rank's frames t >= 1 the label of frame t under every row of frame t-1, -1 for absent (zero-area) rows:
    backend.lookup at the drift-corrected centroids, or by the source's kind backend.piv_lookup on the held plane, whose first
    exception ends the loop, or backend.local_drift_lookup on it with the source's options.  Returns ({t: hits}, (failed frame or
    -1, kind 1: IndexError / 2: other), the exception)."""
    hits = {}
    for t in [t for t in mine if t >= 1]:
        prev = tables[t - 1]
        if source.kind == "piv":
            try:
                res = backend.piv_lookup(t, held_planes.pop(t), prev)
            except Exception as e:            # the round's collectives still run: _agree_on_piv_failure tells every rank
                return hits, (t, 1 if isinstance(e, IndexError) else 2), e
        elif source.kind == "local":
            res = backend.local_drift_lookup(t, held_planes.pop(t), prev, **source.local)
        else:
            dy, dx = tables[t]["drift"]
            res = backend.lookup(t, np.round(prev["cy"] - dy).astype(np.int64), np.round(prev["cx"] - dx).astype(np.int64))
        hits[t] = np.where(prev["area"] > 0, res, -1)
    return hits, (-1, 0), None


def _agree_on_piv_failure(failed, error, rank, world, dist, device):
    """All-gather of every rank's first failing PIV frame of the round; if there is one, every rank raises for the lowest:
    its owner its own exception, the others an error that names frame and rank."""
    allv = [failed]
    if world > 1:
        import torch
        mine = torch.tensor(list(failed), dtype=torch.int64, device=device)
        allv = [torch.zeros(2, dtype=torch.int64, device=device) for _ in range(world)]
        dist.all_gather(allv, mine)
    hits = [(int(v[0]), int(v[1]), r) for r, v in enumerate(allv) if int(v[0]) >= 0]
    if hits:
        t_bad, kind, owner = min(hits)
        if owner == rank and t_bad == failed[0]:
            raise error
        if kind == 1:
            raise IndexError("use_piv: frame %d's flow sampling is out of bounds on rank %d" % (t_bad, owner))
        raise RuntimeError("use_piv: frame %d's PIV look-up failed on rank %d" % (t_bad, owner))


def _gather_lookups(hits, dist, rank, world, device):
    """The round's look-ups on rank 0, {t: int64 hits} (records of LOOKUP_FIELDS, gathered); {} on the other ranks.  One process:
    `hits` as it is."""
    if world == 1:
        return hits
    flat = pack_records({t: dict(hits=h) for t, h in hits.items()}, LOOKUP_FIELDS)
    parts = gather_varlen(flat, dist, rank, world, device, root=0) or ()
    return {t: r["hits"] for part in parts for t, r in unpack_records(part, LOOKUP_FIELDS).items()}


def _link_round(linked, tables):
    """stitcher="device_linker" on rank 0: the frames that have arrived and are next in order go to the linker.  A round's
    frames are one contiguous block, so after round k every frame below (k + 1) B W is linked."""
    while len(linked.ids) in tables:
        tb = tables[len(linked.ids)]
        linked.add(tb, tb["drift"])


def _stitch(tables, lookups, stitcher, linked=None):
    """Rank 0's sequential part -> (tables per frame, track ids per frame).  linked: the _IdLinker that has seen every round."""
    tabs = [tables[t] for t in range(len(tables))]
    if stitcher == "device_linker":
        return tabs, linked.ids
    if stitcher == "linker":
        return tabs, link_ids(tabs, [tb["drift"] for tb in tabs])
    return tabs, propagate_ids(tabs, [None] + [lookups[t] for t in range(1, len(tabs))])


def process_movie(n_frames, frame_source, backend, rank=0, world=1, dist=None, device="cpu", drifts=None,
                  estimate_drift=False, stitcher="lookup", block_frames=None, use_piv=False, local_drifts=None):
    """Runs the sharded pipeline.  frame_source(t) -> uint16 stack (or whatever backend.process_frame takes).
    Returns on rank 0: (tables per frame, track ids per frame); on other ranks (None, None).  tables[t]["drift"] holds
    the (row, column) drift used between frames t-1 and t (estimated by frame t's owner when estimate_drift).  A backend
    with `extra_columns` ((name, dtype) pairs, e.g. GpuFrameBackend(cell_types=...)'s type / valid / mean_intensity) has
    those per-row columns carried to rank 0's tables too, at any world size; without them the exchange is unchanged.

    use_piv=True: the tracker's PIV mode (Tissue.track_cells_iterator(use_piv=True), ti.py:2061-2106).  Planes are exchanged
    as for estimate_drift, and the owner of frame t >= 1 calls backend.piv_lookup(t, plane of frame t-1, table of frame t-1)
    instead of shifting the centroids by a drift and calling backend.lookup; tables[t]["drift"] keeps the `drifts` row given.
    It needs a backend with planes (GpuFrameBackend(keep_planes=True)) and the "lookup" stitcher, and excludes
    estimate_drift (ValueError).  Upstream's transposed sampling makes only square frames safe: where its numpy indexing
    raises, every rank raises IndexError for the lowest failing frame of that round -- each rank first takes part in the
    round's small all-gather of failures and joins its worker thread, so no collective is left waiting and no further
    round starts.  Any other exception of a round (a backend's, a collective's) leaves the same way: the one compute thread,
    which serves every round, finishes the round it has begun before the exception reaches the caller.

    local_drifts: None, True (upstream's step_size 100, window_size 700) or dict(step_size=..., window_size=...): the local-drift
    map as the drift source (Tissue.fix_one_frame_tracking_using_local_drifts' map, ti.py:2149-2173).  Planes are exchanged as for
    estimate_drift, and the owner of frame t >= 1 calls backend.local_drift_lookup(t, plane of frame t-1, table of frame t-1,
    step_size, window_size): every centroid moves by the mean shift of the windows that contain it.  tables[t]["drift"] keeps
    the `drifts` row given; the window shifts stay on the owner (backend.local_drifts[t]).  It needs a backend with planes, frame
    extents (Y, X) above window_size and the "lookup" stitcher, and excludes estimate_drift and use_piv (ValueError, before any
    frame is computed).

    stitcher="device_linker": the linker of stitcher="linker" with its link finding on the GPU (linking.DeviceFrameLinker; the
    same ids, the same exclusions: no use_piv, no local_drifts).  Rank 0 links a round's frames as soon as _exchange_tables has
    delivered them, while the compute thread works on the next round, so with block_frames the linking is no tail after the
    last frame either.  stitcher="linker" links all tables at the end, with the linker TISSUE_HIP_LINKER names (default host).

    The movie is worked off in ROUNDS of `block_frames` frames per rank (plan_rounds; None: the whole shard in one round, no
    overlap).  While a thread computes round k+1 (_compute_round), this one runs round k's exchange: planes to the neighbour rank
    (exchange_planes), drift (_drift_step), all-gather of the cell tables (_exchange_tables), owner-side look-ups (_owner_lookups;
    with use_piv the failure agreement, _agree_on_piv_failure), gather of the index arrays to rank 0 (_gather_lookups) -- so the
    stitching traffic and the drift correlations hide behind the next frames' kernels instead of forming a tail after the last
    frame; rank 0 then stitches (_stitch).  Every rank runs the same rounds and joins their collectives, with empty payloads
    when it has no frame in one, so any n_frames works, including fewer frames than ranks."""
    from concurrent.futures import ThreadPoolExecutor
    source = _drift_source(stitcher, estimate_drift, use_piv, local_drifts, backend)
    drifts = np.zeros((n_frames, 2)) if drifts is None else np.array(drifts, dtype=np.float64)
    extra = tuple(getattr(backend, "extra_columns", ()))      # further per-row columns every frame's dict carries
    rounds = plan_rounds(n_frames, rank, world, block_frames)
    upstream = plan_rounds(n_frames, (rank - 1) % world, world, block_frames)      # the neighbour whose planes arrive here
    tables, lookups, held_planes = {}, {}, {}
    linked = None
    if stitcher == "device_linker" and rank == 0:
        from .linking import DeviceFrameLinker
        linked = _IdLinker(DeviceFrameLinker(**LINKER_OPTIONS))
    with ThreadPoolExecutor(1) as pool:               # (left only when the compute thread is idle, also by an exception)
        pending = pool.submit(_compute_round, rounds[0], frame_source, backend)
        for k, mine in enumerate(rounds):
            local = pending.result()
            if k + 1 < len(rounds):                   # the next round computes while this one is exchanged
                pending = pool.submit(_compute_round, rounds[k + 1], frame_source, backend)
            if source.planes:                         # frame t's plane goes to the owner of frame t+1, if there is one
                held_planes.update(exchange_planes([t for t in mine if t + 1 < n_frames],
                                                   [t for t in upstream[k] if t + 1 < n_frames], backend, rank, world, dist))
            _drift_step(mine, local, drifts, backend, held_planes, source)
            tables.update(_exchange_tables(mine, local, extra, dist, rank, world, device))
            if linked is not None:
                _link_round(linked, tables)
            if stitcher != "lookup":
                continue
            hits, failed, error = _owner_lookups(mine, tables, backend, held_planes, source)
            if source.kind == "piv":
                _agree_on_piv_failure(failed, error, rank, world, dist, device)
            lookups.update(_gather_lookups(hits, dist, rank, world, device))
    return _stitch(tables, lookups, stitcher, linked) if rank == 0 else (None, None)


def find_events(n_frames, backend, tables, ids, rank=0, world=1, dist=None, device="cpu", drifts=None):
    """Detects the movie's cell events -- delaminations, divisions, differentiations -- as Tissue.find_events_iterator(1, n_frames,
    differentiation_type_name=<the archive's type>) would on the saved archive, without a label map leaving its GPU.  Collective
    like save_seg: EVERY rank calls it after process_movie with process_movie's results (rank 0: tables and ids per frame; the
    others: None, None) and the backend that ran the movie with archive=... (its kept parts hold the neighbour pairs; ValueError
    otherwise).  Returns the events DataFrame on rank 0 -- what save_seg(..., events=...) writes as events_data.pkl -- and None
    elsewhere.  An untyped movie has no differentiations.

    Rank 0 hands out ids, centroids and drift rows (drifts: None = tables[t]["drift"], the rows drifts.npy will hold).  Every
    owner publishes its frames' rows -- sel, pos, the CSR of the table's neighbour sets (backend.event_rows), the border flags of
    its map (backend.border_rows) -- and the labels of its map under the NEXT frame's rows at int(round(c)) + int(drift), the drift
    truncated first (backend.lookup_exact); the owner of frame t then classifies the pair (t - 1, t) on its GPU
    (backend.classify_pair) and the flagged rows travel to rank 0, which builds the table through Tissue.add_event
    (events.events_table).  Six collectives per call whatever n_frames is -- a broadcast, an all-gather and a gather, each after
    its size exchange (_collectives.broadcast_varlen, gather_varlen) -- with empty payloads from ranks that own nothing, so any
    n_frames works, including fewer frames than ranks.

    ValueError, on every rank, when a frame has no table or a drift row is not finite; on the owner (the other ranks then raise
    RuntimeError instead of waiting) when an id occurs twice among a frame's valid, non-empty rows."""
    from .events import find_events as _find_events
    return _find_events(n_frames, backend, tables, ids, rank, world, dist, device, drifts)


def save_seg(path, n_frames, backend, tables, ids, rank=0, world=1, dist=None, device="cpu", channel_names=(), events=None):
    """Writes a finished movie as `<path>.seg`, the archive Tissue.load and the unmodified GUI open.  Collective: EVERY rank calls
    it after process_movie, with process_movie's results (rank 0: tables and ids per frame; the others: None, None) and the
    backend that ran the movie with archive=True or dict(type_name=...) (GpuFrameBackend).  Returns the path on rank 0, None
    elsewhere.

    Rank 0 hands the owners the track ids of their frames.  Each owner wraps its frames' device-deflated label and type maps as
    `.npy` members (the array header in front as a stored block, CRCs combined: _deflate.npy_member) and builds
    frame_k_data.pkl from the tables it kept -- what set_labels, calculate_frame_cellinfo, calc_cell_types(plane, ..., type_name)
    when the backend types cells, and `label` = ids[t] leave in a Tissue; no device pass runs again -- deflated with the host's
    zlib, being small.  The members travel to rank 0 as records in one gather (_collectives.gather_varlen); rank 0 adds drifts.npy (the
    tables[t]["drift"] rows), valid_frames.npy (ones), the events table (`events`, rank 0's DataFrame from find_events; None: an empty
    one, the archive as it was before there were events), the type and channel names and shape_fitting_data.json, and writes the zip itself (seg_archive.write_raw_zip: members and order of
    Tissue._archive_members).  An archive that would need zip64 raises ValueError before anything is written."""
    from .seg_archive import save_seg as _save_seg
    return _save_seg(path, n_frames, backend, tables, ids, rank, world, dist, device, channel_names, events)


def export_tiff(path, n_frames, backend, ids, rank=0, world=1, dist=None, device="cpu", rowsperstrip=None, codes="dynamic", bigtiff=None):
    """Writes a finished movie's tracked labels and cell types as the TIFF of the GUI's "Export segmentation"
    (Tissue.export_segmentation_and_cell_types_to_tiff): T x C x 1 x Y x X uint16 with deflate strips, channel 0 the tracking labels
    ids[t][label - 1] (0 on label 0), channel 1 -- only when the backend typed its cells (C = 2, else 1) -- the type map with 0 -> 2
    and 255 -> 0.  Collective like save_seg: EVERY rank calls it after process_movie, with process_movie's ids on rank 0 (None
    elsewhere); it needs no archive=, the maps are resident either way.  Returns the path on rank 0, None elsewhere.

    Rank 0 hands the owners the track ids of their frames (one broadcast).  Each owner turns its frames' resident maps into uint16
    pages and those into one zlib stream per strip on its GPU (backend.export_page_strips: tip_export_maps_u16_dev, then
    tip_deflate_strips_dev) -- no map reaches the host uncompressed.  The strips travel to rank 0 as records in one gather
    (_collectives.gather_varlen), and rank 0 writes them with tiff.write_tiff_strips, which it tells every
    strip's size, so bigtiff=None gives BigTIFF exactly when the classic file would reach 4 GiB.  Rank 0 holds the movie's
    compressed strips once.

    rowsperstrip: None = tiff.default_rows_per_strip(Y, 2 X), as many rows as 64 KB hold -- the most the strip encoder takes;
    codes: "dynamic" (per-strip Huffman codes where they are shorter) or "fixed".  The file does not depend on the world size.
    ValueError on EVERY rank, before anything is written, when a frame was not processed by its owner's backend or holds a track
    id outside [0, 65535] (the owners all-gather what they found first); ValueError on the owner when ids do not cover a frame's
    labels."""
    from .tiff_export import export_tiff as _export_tiff
    return _export_tiff(path, n_frames, backend, ids, rank, world, dist, device, rowsperstrip, codes, bigtiff)


def export_projection(path, n_frames, backend, rank=0, world=1, dist=None, device="cpu", rowsperstrip=None, codes="dynamic", predictor=1,
                      bigtiff=None, zmap=True, metadata=None):
    """Writes a finished movie's projection as the `positionN.tif` of movie_surface_projection -- T x C x Y x X uint16 with deflate
    strips, what save_tiff(path, movie, axes="TCYX", data_type="uint16") stores: every sample scaled by the WHOLE movie's maximum
    to 65535 and rounded (tiff.tiff_normalise) -- and, with zmap=True, `zmap_<name>.npy` beside it (`name`: path's basename
    without ".tif"), uint16 (T, 1, 1, Y, X), where Tissue.load_height_map looks for it.  Collective like export_tiff: EVERY rank
    calls it after process_movie with the backend that ran the movie with keep_projection=True.  Returns (path, the z-map's path or
    None) on rank 0, None elsewhere.

    The owners all-gather their frames' maxima (tip_max_f64_dev, 8 bytes a frame) and every rank takes the largest.  Each owner
    turns its frames' resident float64 planes into uint16 pages and those into one zlib stream per strip on its GPU
    (backend.projection_page_strips: tip_projection_pages_u16_dev, then tip_deflate_strips_dev); the strips travel to rank 0 in one
    gather and rank 0 writes them with tiff.write_tiff_strips.  The uint16 z-maps (tip_zmap_u16_dev) travel raw in a second gather.

    rowsperstrip: None = tiff.default_rows_per_strip(Y, 2 X); codes: "dynamic" or "fixed"; predictor: 1, or 2 for horizontal
    differencing (tag 317; on synthetic data it did not pay, which is why it is not the default); bigtiff as in export_tiff;
    metadata: an object with to_xml() or a string, written into the description as save_tiff does.  The file does not depend on the
    world size.  ValueError on EVERY rank, before anything is written: a frame whose owner kept no projection (the owners
    all-gather what they lack first), a row over 64 KB (X > 32768: a strip is one chunk of the encoder), a maximum that is
    negative or not finite."""
    from .tiff_export import export_projection as _export_projection
    return _export_projection(path, n_frames, backend, rank, world, dist, device, rowsperstrip, codes, predictor, bigtiff, zmap, metadata)
