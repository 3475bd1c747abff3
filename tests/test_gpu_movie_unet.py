"""GPU: the sharded movie driver in U-Net segmentation mode (GpuFrameBackend(segmentation="unet"), FramePipeline.segment_unet_frame).

The single-frame path -- FramePipeline.project, segment_unet, `.cpu().numpy()`, golden-pinned through predict -- is the truth:
the driver's label maps, HC maps, tables, cell types and track ids must equal what follows from those labels, exactly, at
world 1 and world 2.

Orientation.  segment_unet hands predict the transposed planes (2, X, Y), and predict returns its results transposed against
its input (tests/test_gpu_unet.py::test_predict_shapes_and_padding: a (2, 100, 70) image gives (70, 100) labels): the two
cancel, segment_unet's tensors are shaped (Y, X) and lie on the projection pixel for pixel.  The truth is therefore those
tensors AS THEY ARE, not their `.T`, and their tables with shape=(Y, X), no column swapped; the non-square frame makes any
other reading fail on the shapes alone.

Shapes.  The movie is Z=6, Y=128, X=160, T=5: the network input is padded to (pow2(Y), pow2(X)) = 128 x 256, the smallest extent
on the hand-written kernel path (hip_path_ok: multiples of 64 x 256), non-square, with a front pad of 96 along X.  (Y=160, X=128
would be padded to 256 x 128, which is OFF that path: the network then runs through MIOpen, which is not reproducible call to
call, and the `last_mode` assertion below fails.)  For the same reason the PIV run's square movie is 256 x 256, the smallest
square frame on that path (128 x 128 is padded to 128 x 128: MIOpen).  It is not a smaller frame padded to 256 x 256:
calibrate_head sets the foreground fraction over the PADDED input, and where the front pad outweighs the frame (160 x 160: 61 %
pad) the whole calibrated half can fall on one side of the frame's edge and leave the frame itself without a single label.

Non-degeneracy.  Every predictor is random-init (seed 0) with its head calibrated to 0.5 foreground on the max-over-z of frame
0's stack; movie seed 8; drift row (-6.5, 4.3).  With these every frame has at least 8 labels and every step t-1 -> t has both
hits and misses in the tracker's look-up (asserted in test_single_pipeline_is_not_degenerate).  The PIV run: movie seed 7, the
same fraction, no drift row (PIV finds the shift); every frame has at least 8 labels (asserted there)."""
import numpy as np
import pytest

import _gpu_movie_unet_worker as W
from gloo_launch import run_ranks

pytestmark = pytest.mark.gpu


def mixin_types(labels, marker, threshold, percentage, window, min_cell_area=0.1, max_cell_area=10):
    """set_labels + calculate_frame_cellinfo + calc_cell_types("HC") on a fresh Tissue -> (type, valid, mean, type map)."""
    from tissue_image_processing_amd import tissue_info as ti
    t = ti.Tissue(1, max_cell_area=max_cell_area, min_cell_area=min_cell_area)
    t.set_labels(1, np.asarray(labels).copy(), reset_data=True)
    t.calculate_frame_cellinfo(1)
    t.calc_cell_types(marker, 1, "HC", threshold, percentage, window)
    ci = t.get_cells_info(1)
    return (ci["type"].to_numpy().astype(np.uint8), ci["valid"].to_numpy().astype(np.uint8),
            ci["mean_intensity_HC"].to_numpy().astype(np.float64), np.asarray(t.get_cell_types(1)))


def assert_same_types(got, want):
    typ, valid, mean, tmap = got
    wtyp, wvalid, wmean, wmap = want
    np.testing.assert_array_equal(typ, wtyp)
    np.testing.assert_array_equal(valid, wvalid)
    np.testing.assert_allclose(mean, wmean, rtol=1e-12)          # (float64 atomics in the intensity sums; NaN where absent)
    assert np.array_equal(np.isnan(mean), np.isnan(wmean))
    np.testing.assert_array_equal(tmap, wmap)


def host_lookup(labels, qy, qx):
    """maximum_filter(labels, (3, 3), 'constant') at the query points, -1 outside the frame (ti.py:2081-2090)."""
    Yf, Xf = labels.shape
    pad = np.pad(labels, 1)
    out = np.full(qy.shape, -1, np.int32)
    for i in np.flatnonzero((qy >= 0) & (qy < Yf) & (qx >= 0) & (qx < Xf)):
        out[i] = pad[qy[i]:qy[i] + 3, qx[i]:qx[i] + 3].max()
    return out


def pair_set(pairs):
    return set(map(tuple, np.sort(np.asarray(pairs), axis=1).tolist()))


@pytest.fixture(scope="module")
def truth():
    """Per frame, from ONE single pipeline: the labels / HC map of segment_unet and the tables on its label tensor, the Atoh
    plane, and what segment_unet_frame leaves in the pipeline's own buffers.  Computed once, never changed."""
    from tissue_image_processing_amd.pipeline import FramePipeline
    stacks = W.movie_stacks()
    pred = W.predictor_factory(stacks)(0)
    pipe = FramePipeline(2, W.Z, W.Y, W.X, device=0, use_torch=True)
    frames = []
    for t in range(W.T):
        d = pipe.upload_stack(stacks[t])
        pipe.project(d)
        lab, hc = pipe.segment_unet(pred)
        tab_t = {k: v.copy() for k, v in pipe.cell_tables(labels_ptr=lab.data_ptr(), shape=(W.Y, W.X)).items()}
        f = dict(lab=lab.cpu().numpy(), hc_t=hc.cpu().numpy(), tab_t=tab_t, marker=pipe.fetch_projection()[0][1],
                 mode=pred.model.last_mode, flags=int(pred.last_flags))
        pipe.segment_unet_frame(pred, keep_hc=True)
        f["tab"] = {k: v.copy() for k, v in pipe.cell_tables().items()}
        f["labels"], f["hc"] = pipe.fetch_labels(), pipe.fetch_hc()
        rows = pipe.cell_types(**W.CELL_TYPES)
        f["types"] = (rows["type"], rows["valid"], rows["mean_intensity"].copy(), pipe.fetch_cell_types())
        f["mode_frame"] = pred.model.last_mode
        f["mixin"] = mixin_types(f["lab"], f["marker"], 0.03, 3, 3)      # (the golden-pinned mixin on the truth labels)
        frames.append(f)
        d.free()
    return frames


def truth_tables(truth):
    """area / cy / cx per frame as the driver derives them, from the tables on segment_unet's label tensor."""
    out = []
    for f in truth:
        tab = f["tab_t"]
        area = tab["area"].astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            cy, cx = tab["sumy"] / area, tab["sumx"] / area
        out.append(dict(area=tab["area"], cy=np.where(area > 0, cy, 0.0), cx=np.where(area > 0, cx, 0.0)))
    return out


def truth_lookups(truth):
    tabs, drifts = truth_tables(truth), W.drift_rows()
    hits = [None]
    for t in range(1, W.T):
        prev, (dy, dx) = tabs[t - 1], drifts[t]
        res = host_lookup(truth[t]["lab"], np.round(prev["cy"] - dy).astype(np.int64), np.round(prev["cx"] - dx).astype(np.int64))
        hits.append(np.where(prev["area"] > 0, res, -1))
    return tabs, hits


def test_single_pipeline_is_not_degenerate(truth):
    from tissue_image_processing_amd import _lib
    tabs, hits = truth_lookups(truth)
    for t, f in enumerate(truth):
        n = int(f["lab"].max())
        print("frame %d: %d labels, mode %s, flags %#x" % (t, n, f["mode"], f["flags"]),
              "" if t == 0 else "look-up hits %d misses %d" % ((hits[t] > 0).sum(), (hits[t] <= 0).sum()))
        assert f["lab"].shape == (W.Y, W.X) and n >= 8
        assert f["mode"] != "miopen" and f["mode_frame"] != "miopen"
        assert f["flags"] & _lib.WS_FLAG_TWO_VALUED and not f["flags"] & (_lib.WS_FLAG_SERIAL_EXACT | _lib.WS_FLAG_SERIAL_FINISH)
        if t:
            assert (hits[t] > 0).any() and (hits[t] <= 0).any()


def test_segment_unet_frame_is_the_single_frame_path(truth):
    for f in truth:
        np.testing.assert_array_equal(f["labels"], f["lab"])
        np.testing.assert_array_equal(f["hc"].view(np.uint64), f["hc_t"].view(np.uint64))
        got, want = f["tab"], f["tab_t"]
        for k in ("area", "pc", "sumy", "sumx", "bbox"):
            np.testing.assert_array_equal(got[k], want[k])
        assert pair_set(got["pairs"]) == pair_set(want["pairs"]) and len(got["pairs"]) == len(want["pairs"])
        assert_same_types(f["types"], f["mixin"])


@pytest.mark.parametrize("world", [1, 2])
def test_backend_equals_single_pipeline(truth, world, tmp_path):
    from tissue_image_processing_amd import _lib, movie
    out = str(tmp_path / "w.npz")
    run_ranks("_gpu_movie_unet_worker.py", world, (out,), timeout=600, local_rank="0")
    res, own = np.load(out), {}
    for r in range(world):
        own.update(np.load(out + ".rank%d.npz" % r))
    tabs, hits = truth_lookups(truth)
    want_ids = movie.propagate_ids(tabs, hits)
    assert int(res["n"]) == W.T
    for t, f in enumerate(truth):
        np.testing.assert_array_equal(own["labels_%d" % t], f["lab"])
        np.testing.assert_array_equal(own["hc_%d" % t].view(np.uint64), f["hc_t"].view(np.uint64))
        assert str(own["mode_%d" % t]) not in ("miopen", "None")
        flags = int(own["flags_%d" % t])
        assert flags & _lib.WS_FLAG_TWO_VALUED and not flags & (_lib.WS_FLAG_SERIAL_EXACT | _lib.WS_FLAG_SERIAL_FINISH)
        for k in ("area", "cy", "cx"):
            np.testing.assert_array_equal(res["%s_%d" % (k, t)], tabs[t][k])
        np.testing.assert_array_equal(res["drift_%d" % t], W.drift_rows()[t])
        assert_same_types((res["type_%d" % t], res["valid_%d" % t], res["mean_intensity_%d" % t], own["types_%d" % t]), f["mixin"])
        np.testing.assert_array_equal(res["ids_%d" % t], want_ids[t])


def test_piv_mode_ids_do_not_depend_on_frames_in_flight():
    """use_piv in U-Net mode on a square movie (the only case upstream's sampling allows): worker threads with their own
    predictors and torch streams (inflight=2, one round) give the label maps and ids of one frame at a time."""
    from tissue_image_processing_amd import movie
    N, frames = 256, 4
    stacks = W.movie_stacks(N, N, frames, seed=7)
    factory = W.predictor_factory(stacks)
    runs = []
    for inflight in (1, 2):
        backend = movie.GpuFrameBackend(2, W.Z, N, N, device=0, segmentation="unet", predictor_factory=factory, inflight=inflight,
                                        keep_planes=True)
        try:
            tabs, ids = movie.process_movie(frames, lambda t: stacks[t], backend, use_piv=True)
            runs.append((ids, [backend.labels[t].download((N, N), np.int32) for t in range(frames)], dict(backend.unet_modes)))
            # one predictor per pipeline that segmented: the main one alone, or the workers' and none for the main pipeline
            assert 1 <= len(backend._predictors) <= inflight and (id(backend.pipe) in backend._predictors) == (inflight == 1)
        finally:
            backend.close()
        assert not backend._predictors and not backend._workers
    (ids1, labels1, modes1), (ids2, labels2, modes2) = runs
    for t in range(frames):
        assert modes1[t] != "miopen" and modes2[t] != "miopen"
        assert int(labels1[t].max()) >= 8
        np.testing.assert_array_equal(labels2[t], labels1[t])
        np.testing.assert_array_equal(ids2[t], ids1[t])
        if t:
            assert np.intersect1d(ids1[t], ids1[t - 1]).size > 0      # tracks are carried from frame to frame


def test_classical_keyword_is_the_default():
    from tissue_image_processing_amd import movie
    frames = 3
    stacks = W.movie_stacks(frames=frames)
    drifts = W.drift_rows(frames)
    outs = []
    for kw in ({}, {"segmentation": "classical"}):
        backend = movie.GpuFrameBackend(2, W.Z, W.Y, W.X, device=0, **kw)
        try:
            outs.append(movie.process_movie(frames, lambda t: stacks[t], backend, drifts=drifts))
            assert backend.pipe._proj_t is None and not backend.unet_modes
        finally:
            backend.close()
    (tabs_a, ids_a), (tabs_b, ids_b) = outs
    for t in range(frames):
        assert sorted(tabs_a[t]) == sorted(tabs_b[t]) == ["area", "cx", "cy", "drift"]
        for k in tabs_a[t]:
            np.testing.assert_array_equal(tabs_a[t][k], tabs_b[t][k])
        np.testing.assert_array_equal(ids_a[t], ids_b[t])


def test_argument_errors():
    from tissue_image_processing_amd import movie
    with pytest.raises(ValueError, match="classical.*unet"):
        movie.GpuFrameBackend(2, W.Z, W.Y, W.X, device=0, segmentation="Unet")
    for kw in (dict(unet_weights="weights.h5"), dict(predictor_factory=lambda device: None), dict(keep_hc=True)):
        with pytest.raises(ValueError, match="classical.*unet"):
            movie.GpuFrameBackend(2, W.Z, W.Y, W.X, device=0, segmentation="classical", **kw)
        with pytest.raises(ValueError, match="classical.*unet"):
            movie.GpuFrameBackend(2, W.Z, W.Y, W.X, device=0, **kw)
