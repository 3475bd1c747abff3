"""GPU: movie.save_seg with GpuFrameBackend(archive=dict(matches="rows")) -- the label and type maps deflated on the device with
matches to the row above -- on the small movie of _gpu_movie_seg_worker.py: Tissue.load gives the maps on the GPU and the tables
of the run-only archive, and every frame's stream is shorter than its run-only stream."""
import zipfile

import numpy as np
import pandas as pd
import pytest

import _gpu_movie_seg_worker as w

pytestmark = pytest.mark.gpu


def _run(path, frames, matches):
    from tissue_image_processing_amd import movie
    backend = movie.GpuFrameBackend(2, w.Z, w.Y, w.X, device=0, inflight=2, cell_types=w.CELL_TYPES,
                                    archive=dict(type_name="HC", matches=matches))
    try:
        tabs, ids = movie.process_movie(w.T, lambda t: frames[t], backend, 0, 1, None, "cpu", w.drifts(), block_frames=1)
        path = movie.save_seg(path, w.T, backend, tabs, ids, 0, 1, None, "cpu", channel_names=w.CHANNELS)
        return dict(path=path,
                    labels=[backend.labels[t].download((w.Y, w.X), np.int32) for t in range(w.T)],
                    types=[backend.fetch_cell_types(t) for t in range(w.T)],
                    sizes=[(len(backend.archive_frames[t]["labels"][0]), len(backend.archive_frames[t]["types"][0])) for t in range(w.T)])
    finally:
        backend.close()


def _load(path):
    from tissue_image_processing_amd.tissue_info import Tissue
    tissue = Tissue(w.T)
    for _ in tissue.load(path):
        pass
    return tissue


def test_rows_archive_loads_as_the_runs_archive(tmp_path):
    from tissue_image_processing_amd._deflate import npy_header
    frames = w.stacks()
    rows, runs = _run(str(tmp_path / "rows"), frames, "rows"), _run(str(tmp_path / "runs"), frames, "runs")
    head = len(npy_header((w.Y, w.X), np.int32))
    with zipfile.ZipFile(rows["path"]) as z, zipfile.ZipFile(runs["path"]) as z_runs:
        assert z.testzip() is None
        assert z.namelist() == z_runs.namelist()
        for t in range(w.T):      # the archive holds the device's rows streams: header block + stream + final block
            assert z.getinfo("frame_%d_labels.npy" % (t + 1)).compress_size == 5 + head + rows["sizes"][t][0] + 5
    got, ref = _load(rows["path"]), _load(runs["path"])
    for t in range(w.T):
        assert got.get_labels(t + 1).dtype == np.int32 and np.array_equal(got.get_labels(t + 1), rows["labels"][t])
        assert got.get_cell_types(t + 1).dtype == np.uint8 and np.array_equal(got.get_cell_types(t + 1), rows["types"][t])
        assert np.array_equal(rows["labels"][t], runs["labels"][t]) and np.array_equal(rows["types"][t], runs["types"][t])
        pd.testing.assert_frame_equal(got.get_cells_info(t + 1), ref.get_cells_info(t + 1))
        assert rows["sizes"][t][0] < runs["sizes"][t][0], (t, rows["sizes"][t], runs["sizes"][t])
        assert rows["sizes"][t][1] < runs["sizes"][t][1], (t, rows["sizes"][t], runs["sizes"][t])
    assert np.array_equal(got.drifts, ref.drifts) and got.type_names == ["HC"]


def test_matches_takes_runs_or_rows():
    from tissue_image_processing_amd import movie
    with pytest.raises(ValueError, match="matches"):
        movie.GpuFrameBackend(2, w.Z, w.Y, w.X, device=0, archive=dict(matches="best"))
    backend = movie.GpuFrameBackend(2, w.Z, w.Y, w.X, device=0, archive=True)
    try:
        assert backend.archive == dict(type_name="HC", matches="runs")
    finally:
        backend.close()
