"""GPU: movie.save_seg -- a finished movie of GpuFrameBackend(archive=...) as a `.seg` archive whose label and type maps were
deflated on the device -- read back by Tissue.load and compared with the maps on the GPU and with the Tissue route
(set_labels, calculate_frame_cellinfo, calc_cell_types, label = ids[t]); two processes write the archive one process writes."""
import io
import zipfile

import numpy as np
import pandas as pd
import pytest

import _gpu_movie_seg_worker as w
from gloo_launch import run_ranks

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def movie_frames():
    return w.stacks()


def _run(tmp, name, frames, typed):
    """One process: the archive's path and what the run left on the GPU, downloaded."""
    backend, tabs, ids, path = w.run_movie(str(tmp / name), 0, 1, None, typed=typed, frames=frames)
    try:
        labels = [backend.labels[t].download((w.Y, w.X), np.int32) for t in range(w.T)]
        types = [backend.fetch_cell_types(t) for t in range(w.T)] if typed else None
        sizes = [(len(backend.archive_frames[t]["labels"][0]), len(backend.archive_frames[t]["types"][0]) if typed else 0) for t in range(w.T)]
    finally:
        backend.close()
    return dict(path=path, tabs=tabs, ids=ids, labels=labels, types=types, sizes=sizes)


@pytest.fixture(scope="module")
def typed_run(tmp_path_factory, movie_frames):
    return _run(tmp_path_factory.mktemp("seg"), "typed", movie_frames, True)


def _load(path):
    from tissue_image_processing_amd.tissue_info import Tissue
    tissue = Tissue(w.T)
    for _ in tissue.load(path):
        pass
    return tissue


def _tissue_route(labels, markers, ids):
    """What the existing route leaves per frame: set_labels, calculate_frame_cellinfo, calc_cell_types when typed, label = ids.
    Every frame is typed on a table to which the type is new, as FramePipeline.cell_types is defined (test_gpu_cell_types.py's
    mixin_types): calc_cell_types writes mean_intensity_<type> only then, so a Tissue that types its frames one after another
    leaves the column in the first of them alone.  The frames move into one Tissue afterwards."""
    from tissue_image_processing_amd.tissue_info import Tissue
    tissue = Tissue(w.T)
    for t in range(w.T):
        one = Tissue(1)
        one.set_labels(1, labels[t].copy(), reset_data=True)
        one.calculate_frame_cellinfo(1)
        if markers is not None:
            one.calc_cell_types(markers[t], 1, "HC", w.CELL_TYPES["threshold"], w.CELL_TYPES["percentage_above_threshold"],
                                w.CELL_TYPES["peak_window_size"])
        one.get_cells_info(1).loc[:, "label"] = np.asarray(ids[t], np.int64)
        tissue.set_labels(t + 1, one.get_labels(1))
        tissue.set_cells_info(t + 1, one.get_cells_info(1))
        tissue.set_cell_types(t + 1, one.get_cell_types(1))
    return tissue


def _markers(frames):
    from tissue_image_processing_amd.pipeline import FramePipeline
    pipe = FramePipeline(2, w.Z, w.Y, w.X, reference_channel=0, airyscan=False)
    out = []
    for t in range(w.T):
        d = pipe.upload_stack(frames[t])
        pipe.project(d)
        out.append(pipe.fetch_projection()[0][w.CELL_TYPES["atoh_channel"]])
        d.free()
    return out


def test_typed_movie_loads_as_the_tissue_route(typed_run, movie_frames):
    r = typed_run
    assert r["path"].endswith("typed.seg")
    with zipfile.ZipFile(r["path"]) as z:
        assert z.testzip() is None
        want = [n % (t + 1) for t in range(w.T) for n in ("frame_%d_labels.npy", "frame_%d_types.npy", "frame_%d_data.pkl")]
        assert z.namelist() == want + ["events_data.pkl", "drifts.npy", "valid_frames.npy", "shape_fitting_data.json",
                                       "cell_type_names.pkl", "channel_names.pkl", "fake_channels.pkl"]
        from tissue_image_processing_amd._deflate import npy_header
        head = len(npy_header((w.Y, w.X), np.int32))
        for t in range(w.T):      # the device's streams are what the archive holds: header block + stream + final block
            info = z.getinfo("frame_%d_labels.npy" % (t + 1))
            assert info.compress_size == 5 + head + r["sizes"][t][0] + 5 and info.file_size == head + w.Y * w.X * 4
    got = _load(r["path"])
    ref = _tissue_route(r["labels"], _markers(movie_frames), r["ids"])
    for t in range(w.T):
        assert got.get_labels(t + 1).dtype == np.int32 and np.array_equal(got.get_labels(t + 1), r["labels"][t])
        assert got.get_cell_types(t + 1).dtype == np.uint8 and np.array_equal(got.get_cell_types(t + 1), r["types"][t])
        assert np.array_equal(got.get_cell_types(t + 1), ref.get_cell_types(t + 1))
        pd.testing.assert_frame_equal(got.get_cells_info(t + 1), ref.get_cells_info(t + 1))
        assert np.array_equal(got.get_cells_info(t + 1)["label"].to_numpy(), r["ids"][t])
    assert np.array_equal(got.drifts, w.drifts()) and got.drifts.dtype == np.float64
    assert np.array_equal(got.valid_frames, np.ones(w.T, int))
    assert got.type_names == ["HC"] and got.channel_names == list(w.CHANNELS) and got.fake_channels == []
    assert len(got.events) == 0 and got.shape_fitting_results == [dict() for _ in range(w.T)]


def test_untyped_movie_has_no_type_members(tmp_path, movie_frames):
    from tissue_image_processing_amd.tissue_info import CELL_INFO_SPECS
    r = _run(tmp_path, "plain", movie_frames, False)
    with zipfile.ZipFile(r["path"]) as z:
        assert z.testzip() is None
        assert not [n for n in z.namelist() if n.endswith("_types.npy")]
        assert len(z.namelist()) == 2 * w.T + 7
    got = _load(r["path"])
    ref = _tissue_route(r["labels"], None, r["ids"])
    for t in range(w.T):
        assert np.array_equal(got.get_labels(t + 1), r["labels"][t]) and got.get_cell_types(t + 1) is None
        assert list(got.get_cells_info(t + 1).columns) == list(CELL_INFO_SPECS)
        pd.testing.assert_frame_equal(got.get_cells_info(t + 1), ref.get_cells_info(t + 1))
    assert got.type_names == []


def test_save_seg_needs_an_archiving_backend(movie_frames):
    from tissue_image_processing_amd import movie
    backend = movie.GpuFrameBackend(2, w.Z, w.Y, w.X, device=0)
    try:
        with pytest.raises(ValueError, match="archive"):
            movie.save_seg("nowhere", w.T, backend, [], [])
        with pytest.raises(ValueError, match="type_index"):
            movie.GpuFrameBackend(2, w.Z, w.Y, w.X, device=0, cell_types=dict(w.CELL_TYPES, type_index=1), archive=True)
        with pytest.raises(ValueError, match="archive"):
            movie.GpuFrameBackend(2, w.Z, w.Y, w.X, device=0, archive=dict(name="HC"))
    finally:
        backend.close()


def test_two_processes_write_the_same_archive(tmp_path, typed_run):
    out = str(tmp_path / "world2")
    run_ranks("_gpu_movie_seg_worker.py", 2, (out,), timeout=600, local_rank="0")
    with zipfile.ZipFile(typed_run["path"]) as one, zipfile.ZipFile(out + ".seg") as two:
        assert two.testzip() is None
        assert two.namelist() == one.namelist()
        for name in one.namelist():
            if name.endswith("_data.pkl") and name.startswith("frame_"):
                pd.testing.assert_frame_equal(pd.read_pickle(io.BytesIO(two.read(name)), compression=None),
                                              pd.read_pickle(io.BytesIO(one.read(name)), compression=None))
            else:
                assert two.read(name) == one.read(name), name
