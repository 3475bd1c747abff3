"""Device-resident per-frame pipeline (projection -> segmentation -> cell tables) and frame sharding.

One process per GPU; frames are independent units (sp.py:211 loop, gui.py:1840 loop), so a movie shards
`frame t -> rank t % world` with no data-path collective; only the per-frame cell tables are gathered to rank 0
for track stitching (tissue_info.track_cells_iterator, ti.py:2037-2113), which is sequential over frames.
"""
import ctypes

import numpy as np

from . import _lib
from .basic_image_manipulations import gaussian_taps


class FramePipeline:
    """Keeps one frame's buffers resident in HBM between stages (inputs uploaded once, outputs fetched on demand)."""

    def __init__(self, C, Z, Y, X, reference_channel=0, airyscan=False, atoh_shift=0,
                 imgthresh=0.03, stdeviation=3.0, blocksize=3, device=None, use_torch=False):
        if device is not None:
            _lib.init(device)
        self.lib = _lib.lib()
        self.C, self.Z, self.Y, self.X = C, Z, Y, X
        self.ref, self.airy, self.atoh = reference_channel, airyscan, atoh_shift
        self.imgthresh, self.std, self.block = imgthresh, stdeviation, blocksize
        self.t05, self.t1, self.t2, self.t30 = (gaussian_taps(s) for s in (0.5, 1.0, 2.0, 30.0))
        self.tseg = gaussian_taps(stdeviation)
        P = Y * X
        self._proj_t = None
        if use_torch:  # projection buffer owned by torch so that the U-Net path consumes it without a copy
            import torch

            class _View(object):
                pass
            dev = torch.device("cuda", _lib.device_for_thread() or 0)
            self._proj_t = torch.empty((C, Y, X), dtype=torch.float64, device=dev)
            self.d_proj = _View()
            self.d_proj.ptr = self._proj_t.data_ptr()
            self.d_proj.download = lambda shape, dtype, t=self._proj_t: t.cpu().numpy()
        else:
            self.d_proj = _lib.DeviceBuffer(C * P * 8)
        self.d_zmap = _lib.DeviceBuffer(P * 8)
        self.d_labels = _lib.DeviceBuffer(P * 4)
        self.flags = ctypes.c_int32(0)
        self.n_labels = 0

    def upload_stack(self, stack_u16):
        stack_u16 = np.ascontiguousarray(stack_u16, dtype=np.uint16)
        assert stack_u16.shape == (self.C, self.Z, self.Y, self.X)
        buf = _lib.DeviceBuffer(stack_u16.nbytes)
        buf.upload(stack_u16)
        return buf

    def inflate_stack(self, frame):
        """A movie.CompressedFrame -> the resident (C, Z, Y, X) uint16 stack project() reads: one upload of the compressed strips and
        their table, tip_inflate_strips_dev straight into the stack buffer, tip_tiff_finish_u16_dev (byte order, predictor) in
        place -- all on this thread's stream.  A strip that does not inflate raises ValueError naming its page, strip and status
        before anything is projected."""
        from . import _inflate
        assert tuple(frame.shape) == (self.C, self.Z, self.Y, self.X)
        nbytes = self.C * self.Z * self.Y * self.X * 2
        packed, status = _lib.DeviceBuffer(frame.nbytes), _lib.DeviceBuffer(4 * max(frame.n_strips, 1))
        _lib.check(self.lib.tip_memcpy_h2d(packed.ptr, frame.host_ptr(), frame.nbytes))
        pages, strip_of_page, path, t = frame.pages, frame.strip_of_page, frame.path, frame.t
        stack = _lib.DeviceBuffer(nbytes)
        n_bad = _inflate.inflate_strips_dev(packed.ptr, frame.src_bytes, packed.ptr + frame.table_at, frame.n_strips, 1, stack.ptr, nbytes,
                                            status.ptr)
        frame.release()
        if n_bad:
            st = status.download((frame.n_strips,), np.int32)
            k = int(np.flatnonzero(st)[0])
            stack.free()
            raise ValueError("%s: frame %d, page %d strip %d does not inflate: status %d (%s); %d strip(s) of the frame failed"
                             % (path, t, pages[k], strip_of_page[k], st[k], _inflate.STATUS_TEXT.get(int(st[k]), "?"), n_bad))
        _inflate.tiff_finish_u16_dev(stack.ptr, self.C * self.Z * self.Y, self.X, frame.predictor, frame.swap_bytes)
        packed.free()
        status.free()
        return stack

    def project(self, d_stack):
        """P0-P9 (sp.py:17-85) on a resident uint16 stack; asynchronous."""
        _lib.check(self.lib.tip_project_u16_dev(
            d_stack.ptr, self.C, self.Z, self.Y, self.X, 0, self.Z, 0, self.ref, 1 if self.airy else 0, self.atoh,
            _lib.ptr(self.t05), _lib.ptr(self.t1), _lib.ptr(self.t2), _lib.ptr(self.t30), self.d_proj.ptr, self.d_zmap.ptr))

    def segment(self, channel=0):
        """W1-W3 (bim.py:446-476) on the resident projection of `channel`."""
        P = self.Y * self.X
        img = self.d_proj.ptr + channel * P * 8
        _lib.check(self.lib.tip_watershed_segmentation_f64_dev(
            img, self.d_labels.ptr, self.Y, self.X, self.imgthresh, _lib.ptr(self.tseg), self.tseg.size, self.block,
            ctypes.byref(self.flags)))

    def segment_unet(self, predictor, atoh_channel=1, zo_channel=0):
        """U1-U5 (pl.py:90-198) on the resident projection: (atoh, zo) planes transposed to (X, Y) as gui.py:2059-2061
        hands them over; labels stay on the device (int32 (X, Y))."""
        import torch
        if getattr(self, "_proj_t", None) is None:
            raise RuntimeError("FramePipeline(use_torch=True) is needed for the U-Net path")
        # the projection was written on the library's stream: torch's current stream waits for it (no host round trip)
        _lib.check(self.lib.tip_stream_wait_tip(torch.cuda.current_stream(self._proj_t.device).cuda_stream))
        # (atoh, zo) planes, each transposed: one straight gather + a strided view (prepare_image transposes back while it reads)
        img = self._proj_t[[atoh_channel, zo_channel]].transpose(1, 2)
        lab, hc = predictor.predict(img, return_device=True)
        self._unet_labels = lab
        return lab, hc

    def segment_unet_frame(self, predictor, atoh_channel=1, zo_channel=0, keep_hc=False):
        """segment_unet with the result left where segment() leaves its own: the int32 labels in self.d_labels as (Y, X) --
        cell_tables(), cell_types(...) and fetch_labels() then work as after segment(), the label count being the tail's --
        and, with keep_hc, the float64 HC map in self.d_hc (fetch_hc()).

        No transpose is needed: segment_unet hands predict the TRANSPOSED planes (2, X, Y) and predict returns its results
        transposed against its input (pl.py:102, 194: labels of shape (input.shape[2], input.shape[1])), so the two cancel
        and the tensors come back in frame orientation (Y, X), aligned with the projection.  They are copied on the library's
        stream behind the tail (device to device, nothing waits here).  The copies read torch tensors, so both stay referenced
        by the pipeline until the next U-Net call has passed the tail's tip_sync: a block must not go back to torch's caching
        allocator while the library's stream still reads it."""
        lab, hc = self.segment_unet(predictor, atoh_channel, zo_channel)
        if tuple(lab.shape) != (self.Y, self.X) or tuple(hc.shape) != (self.Y, self.X):
            raise RuntimeError("segment_unet returned %s labels for a %d x %d frame" % (tuple(lab.shape), self.Y, self.X))
        P = self.Y * self.X
        _lib.check(self.lib.tip_memcpy_d2d(self.d_labels.ptr, lab.data_ptr(), P * 4))
        if keep_hc:
            if getattr(self, "d_hc", None) is None:
                self.d_hc = _lib.DeviceBuffer(P * 8)
            _lib.check(self.lib.tip_memcpy_d2d(self.d_hc.ptr, hc.data_ptr(), P * 8))
        self._unet_hc = hc          # (the labels are held as self._unet_labels)

    def fetch_hc(self):
        """The HC map of the last segment_unet_frame(keep_hc=True): float64 (Y, X), downloaded."""
        if getattr(self, "d_hc", None) is None:
            raise RuntimeError("no HC map is resident: segment_unet_frame(..., keep_hc=True) keeps it")
        return self.d_hc.download((self.Y, self.X), np.float64)

    def cell_tables(self, max_cells=None, labels_ptr=None, shape=None):
        """C1-C2 (ti.py:880-909, 1815-1842): per-cell reductions + neighbour pairs on the resident label map; the small
        per-cell arrays come back to the host (they are what a rank gathers for track stitching)."""
        P = self.Y * self.X
        lab_ptr = self.d_labels.ptr if labels_ptr is None else labels_ptr
        LY, LX = (self.Y, self.X) if shape is None else shape
        ncells = max_cells or int(self.lib.tip_last_watershed_labels())   # labels are 1..ncells
        if ncells <= 0:
            self.tables = dict(area=np.zeros(0, np.int64), bbox=np.zeros((0, 4), np.int64), sumy=np.zeros(0, np.int64),
                               sumx=np.zeros(0, np.int64), pc=np.zeros((0, 3), np.int64), pairs=np.zeros((0, 2), np.int32))
            return self.tables
        # ONE device block for every table -- [area n | bbox 4n | sumy n | sumx n | pc 3n] int64, then the pair list -- so
        # that the tables come back in a single device-to-host copy (six separate downloads were six round trips of
        # ~45 us each: 0.3 ms of a 5.9 ms frame)
        if getattr(self, "_tables", None) is None or self._tables[0] < ncells:
            cap = max(1024, int(ncells * 1.5))
            self._tables = (cap, _lib.DeviceBuffer(cap * (80 + 128)))
        cap, d_tab = self._tables
        n = ncells
        base = d_tab.ptr
        o_area, o_bbox, o_sy, o_sx, o_pc, o_pairs = 0, 8 * n, 40 * n, 48 * n, 56 * n, 80 * n
        _lib.check(self.lib.tip_regionprops_i32_dev(lab_ptr, None, LY, LX, n, base + o_area, base + o_bbox, base + o_sy,
                                                    base + o_sx, base + o_pc, None))
        npairs = ctypes.c_int64(0)
        _lib.check(self.lib.tip_neighbor_pairs_i32_dev(lab_ptr, LY, LX, base + o_pairs, 16 * cap, ctypes.byref(npairs)))
        npair = int(npairs.value)
        blob = d_tab.download((80 * n + 8 * npair,), np.uint8)
        i64 = blob[:80 * n].view(np.int64)
        self.tables = dict(
            area=i64[:n], bbox=i64[n:5 * n].reshape(n, 4), sumy=i64[5 * n:6 * n], sumx=i64[6 * n:7 * n],
            pc=i64[7 * n:10 * n].reshape(n, 3), pairs=blob[80 * n:].view(np.int32).reshape(npair, 2))
        return self.tables

    def cell_types(self, atoh_channel=1, threshold=0.1, percentage_above_threshold=90, peak_window_size=0, type_index=0,
                   min_cell_area=0.1, max_cell_area=10, n=None, type_map_ptr=None):
        """C5 (Tissue.calc_cell_types, ti.py:2338-2408, on a fresh table) on the resident label map with the resident projection
        of `atoh_channel` as the marker: one device call (tip_cell_types_i32_dev).  The type map stays resident in
        self.d_types (uint8 (Y, X): a valid cell's type, 255 elsewhere), or in the device buffer at type_map_ptr; the per-row
        arrays over labels 1..n (n: the last watershed's label count by default) -- type (uint8, 1 << type_index or 0), valid
        (uint8) and mean_intensity (float64, NaN for absent labels) -- come back in one copy, which also completes the map."""
        if not 0 <= atoh_channel < self.C:
            raise ValueError("atoh_channel %d: the projection has %d channels" % (atoh_channel, self.C))
        P = self.Y * self.X
        n = int(self.lib.tip_last_watershed_labels()) if n is None else int(n)
        if type_map_ptr is None:
            if getattr(self, "d_types", None) is None:
                self.d_types = _lib.DeviceBuffer(P)
            type_map_ptr = self.d_types.ptr
        # ONE device block [mean n | type n | valid n] so that the rows come back in a single device-to-host copy
        if getattr(self, "_ct", None) is None or self._ct[0] < n:
            cap = max(1024, int(n * 1.5))
            self._ct = (cap, _lib.DeviceBuffer(cap * 10))
        d_rows = self._ct[1].ptr
        if peak_window_size and getattr(self, "t7", None) is None:
            self.t7 = gaussian_taps(7.0)           # find_local_maxima's blur (ti.py:141-144)
        from ._segmentation import cell_types_dev
        cell_types_dev(self.d_labels.ptr, self.d_proj.ptr + atoh_channel * P * 8, self.Y, self.X, n, percentage_above_threshold,
                       threshold, peak_window_size, getattr(self, "t7", None), type_index, min_cell_area, max_cell_area,
                       d_rows + 8 * n, d_rows + 9 * n, d_rows, type_map_ptr)
        if n <= 0:
            self.sync()
            return dict(type=np.zeros(0, np.uint8), valid=np.zeros(0, np.uint8), mean_intensity=np.zeros(0, np.float64))
        blob = self._ct[1].download((10 * n,), np.uint8)
        return dict(type=blob[8 * n:9 * n].copy(), valid=blob[9 * n:].copy(), mean_intensity=blob[:8 * n].view(np.float64))

    NEIGHBOR_COLUMNS = ("n_neighbors", "valid_neighbors", "second_neighbors", "contact_length")
    TYPED_NEIGHBOR_COLUMNS = ("hc_neighbors", "sc_neighbors", "hc_second_neighbors", "sc_second_neighbors", "hc_contact_length",
                              "sc_contact_length")

    def neighbor_features(self, n, valid, type=None, type_index=0):
        """The neighbour-graph columns of the n table rows (csrc/tip_graph.hip) on the resident label map and the pair list that
        cell_tables() left on the device: CSR with working = the valid rows (the table calculate_frame_cellinfo builds), contact
        triples, then per row the degree, the valid neighbours, the size of find_second_order_neighbors' set and the summed
        contact length -- and, with the rows' type bytes, the same four restricted to neighbours positive (hc_*) / not positive
        (sc_*) for bit `type_index` (the two typed second-neighbour columns are the set sizes, not upstream's all-zero column).
        valid / type: host uint8 arrays of n rows.  Every column is int64; they come back in ONE device-to-host copy."""
        from . import _segmentation as seg
        n = int(n)
        names = self.NEIGHBOR_COLUMNS + (self.TYPED_NEIGHBOR_COLUMNS if type is not None else ())
        if n <= 0:
            return {name: np.zeros(0, np.int64) for name in names}
        if getattr(self, "tables", None) is None or getattr(self, "_tables", None) is None or self.tables["area"].size != n:
            raise RuntimeError("neighbor_features(n=%d) follows cell_tables() of the same frame" % n)
        valid = np.ascontiguousarray(valid, dtype=np.uint8).reshape(-1)
        type = None if type is None else np.ascontiguousarray(type, dtype=np.uint8).reshape(-1)
        if valid.size != n or (type is not None and type.size != n):
            raise ValueError("valid / type need %d rows" % n)
        npair = int(self.tables["pairs"].shape[0])
        d_pairs = self._tables[1].ptr + 80 * n
        cap_adj, cap_tri = max(2 * npair, 1), max(4096, 16 * (n + 1))
        # ONE device block: [columns 10 n int64 | triple counts | offsets n + 1 | adj | triple pairs | valid n | type n]
        o_cnt = 80 * n
        o_off = o_cnt + 8 * cap_tri
        o_adj = o_off + 4 * (n + 1)
        o_tri = o_adj + 4 * cap_adj
        o_valid = o_tri + 8 * cap_tri
        o_type = o_valid + n
        need = o_type + n
        if getattr(self, "_nf", None) is None or self._nf.nbytes < need:
            self._nf = _lib.DeviceBuffer(int(need * 1.5))
        base = self._nf.ptr
        rows = np.concatenate([valid, type if type is not None else np.zeros(n, np.uint8)])
        _lib.check(self.lib.tip_memcpy_h2d(base + o_valid, _lib.ptr(rows), 2 * n))
        seg.neighbor_csr_dev(d_pairs, npair, n, base + o_valid, base + o_off, base + o_adj, cap_adj)
        ntri = seg.contact_pairs_dev(self.d_labels.ptr, self.Y, self.X, n + 1, base + o_tri, base + o_cnt, cap_tri)
        graph = (base + o_off, base + o_adj, n, cap_adj)
        col = lambda name: base + 8 * n * names.index(name)      # noqa: E731
        seg.graph_counts_dev(*graph, base + o_valid, None, None, None, n, "all", None, True, col("n_neighbors"))
        seg.graph_counts_dev(*graph, base + o_valid, None, None, None, n, "valid", None, True, col("valid_neighbors"))
        seg.graph_second_dev(*graph, base + o_valid, None, None, n, None, True, col("second_neighbors"))
        seg.contact_sums_dev(base + o_tri, base + o_cnt, ntri, *graph, None, None, None, n, "all", None, True, col("contact_length"))
        if type is not None:
            for prefix, positive in (("hc", True), ("sc", False)):
                seg.graph_counts_dev(*graph, base + o_valid, None, base + o_type, None, n, "type", type_index, positive,
                                     col(prefix + "_neighbors"))
                seg.graph_second_dev(*graph, base + o_valid, base + o_type, None, n, type_index, positive,
                                     col(prefix + "_second_neighbors"))
                seg.contact_sums_dev(base + o_tri, base + o_cnt, ntri, *graph, None, base + o_type, None, n, "type", type_index,
                                     positive, col(prefix + "_contact_length"))
        block = self._nf.download((len(names) * n,), np.int64)
        return {name: block[i * n:(i + 1) * n] for i, name in enumerate(names)}

    ORDER_COLUMNS = (("psi6", np.float64), ("voronoi_neighbors", np.int64))

    def order_features(self, n, valid, cy, cx, order=6):
        """The hexatic order of the n table rows (csrc/tip_order.hip): the rows with valid == 1 are the points, their Delaunay
        neighbours are found on the device and psi_order is taken over them (find_nearest_neighbors_using_voroni_tesselation +
        calc_psin, ti.py:2545-2583).  Returns psi6 (float64) and voronoi_neighbors (int64, the number of Delaunay neighbours), 0 for
        the other rows and everywhere when fewer than 4 rows are valid (upstream's rule).  valid, cy, cx: host arrays of n rows.
        One device block: the points go up in one copy, the two columns come back in one."""
        from . import _segmentation as seg
        n = int(n)
        valid = np.ascontiguousarray(valid, dtype=np.uint8).reshape(-1)
        cy = np.ascontiguousarray(cy, dtype=np.float64).reshape(-1)
        cx = np.ascontiguousarray(cx, dtype=np.float64).reshape(-1)
        if valid.size != n or cy.size != n or cx.size != n:
            raise ValueError("valid / cy / cx need %d rows" % n)
        out = dict(psi6=np.zeros(n, np.float64), voronoi_neighbors=np.zeros(n, np.int64))
        rows = np.flatnonzero(valid == 1)
        m = rows.size
        if m < 4:
            return out
        if getattr(self, "_of", None) is None or self._of.nbytes < 32 * m:
            self._of = _lib.DeviceBuffer(48 * m)
        base = self._of.ptr                     # [py m | px m | psi m | degree m], 8 bytes each
        pts = np.concatenate([cy[rows], cx[rows]])
        if not np.isfinite(pts).all():
            raise ValueError("order_features: a valid row has a non-finite centroid")
        _lib.check(self.lib.tip_memcpy_h2d(base, _lib.ptr(pts), 16 * m))
        seg.order_features_dev(base, base + 8 * m, m, order, base + 16 * m, base + 24 * m)
        blob = np.empty(16 * m, np.uint8)
        _lib.check(self.lib.tip_memcpy_d2h(_lib.ptr(blob), base + 16 * m, 16 * m))
        out["psi6"][rows] = blob[:8 * m].view(np.float64)
        out["voronoi_neighbors"][rows] = blob[8 * m:].view(np.int64)
        return out

    def sensory_region(self, n, cy, cx, type, valid, type_map_ptr=None):
        """The sensory-region filter of the n table rows (Tissue.remove_cells_outside_of_sensory_region, ti.py:2781-2792; csrc/
        tip_hull.hip) next to the resident label map: the hull of the hair cells' centroids -- rows with type == 1, valid == 1 and
        area > 0 (the areas cell_tables() left) --, every row tested against it, and 255 painted on the outside rows' pixels of the
        type map at type_map_ptr (self.d_types by default).  One device call (tip_sensory_region_i32_dev): the rows go up in one
        copy, outside (uint8, 1 = strictly outside) and hull (int32 row positions, counter-clockwise) come back in one.  Raises
        _lib.NoHullError, the map untouched, when the hair cells span no hull.  cy, cx, type, valid: host arrays of n rows."""
        from . import _segmentation as seg
        n = int(n)
        if getattr(self, "tables", None) is None or self.tables["area"].size != n:
            raise RuntimeError("sensory_region(n=%d) follows cell_tables() of the same frame" % n)
        if type_map_ptr is None:
            if getattr(self, "d_types", None) is None:
                raise RuntimeError("sensory_region follows cell_types() of the same frame")
            type_map_ptr = self.d_types.ptr
        outside, hull = seg.sensory_region_dev(self.d_labels.ptr, type_map_ptr, self.Y * self.X, cx, cy, type, valid,
                                               (self.tables["area"] <= 0).astype(np.uint8))
        return dict(outside=outside, hull=hull)

    def fetch_cell_types(self):
        return self.d_types.download((self.Y, self.X), np.uint8)

    def sync(self):
        _lib.check(self.lib.tip_sync())

    def fetch_projection(self):
        return (self.d_proj.download((self.C, self.Y, self.X), np.float64),
                self.d_zmap.download((self.Y, self.X), np.int64))

    def fetch_labels(self):
        return self.d_labels.download((self.Y, self.X), np.int32)


def frames_for_rank(n_frames, rank, world):
    """frame t -> rank t % world."""
    return list(range(rank, n_frames, world))
