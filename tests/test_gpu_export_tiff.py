"""GPU: the TIFF export without a map leaving its GPU uncompressed -- tip_export_maps_u16_dev against numpy, the Tissue mixin's
compression="device" files against what the reference's two export methods hand to save_tiff (tests/golden/export_tiff.npz), and
movie.export_tiff after process_movie against the maps on the GPU, in one process and in two."""
import ctypes
import os

import numpy as np
import pytest

import _gpu_movie_export_worker as w
from deflate_cases import voronoi_pair
from gloo_launch import run_ranks

pytestmark = pytest.mark.gpu


def _remap(types):
    out = types.astype(np.uint16)
    out[types == 0] = 2
    out[types == 255] = 0
    return out


# ---- the page kernel ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(96, 128), (33, 37)])      # four pixels per thread; 1221 pixels: one per thread
@pytest.mark.parametrize("typed", [True, False])
def test_export_maps_against_numpy(shape, typed):
    from tissue_image_processing_amd import _deflate, _lib
    labels, types = voronoi_pair(*shape)
    types = types.copy()
    types[1, :5] = (0, 1, 2, 254, 255)
    n = int(labels.max())
    ids = np.random.default_rng(3).permutation(n).astype(np.int64) * 7 + 11
    ids[0] = 65535
    P = labels.size
    d_labels, d_types, d_out = _lib.DeviceBuffer(P * 4).upload(labels), _lib.DeviceBuffer(P).upload(types), _lib.DeviceBuffer(P * 4)
    d_out.upload(np.full(2 * P, 0xABCD, np.uint16))
    _deflate.export_maps_u16_dev(d_labels.ptr, d_types.ptr if typed else None, P, ids, d_out.ptr)
    got = d_out.download((2,) + shape, np.uint16)
    np.testing.assert_array_equal(got[0], np.insert(ids, 0, 0)[labels].astype(np.uint16))
    np.testing.assert_array_equal(got[1], _remap(types) if typed else np.full(shape, 0xABCD, np.uint16))      # plane 1 is left alone


def test_export_maps_counts_bad_labels_and_rejects_wide_ids():
    from tissue_image_processing_amd import _deflate, _lib
    labels, _ = voronoi_pair()
    labels = labels.copy()
    n = int(labels.max())
    ids = np.arange(1, n + 1, dtype=np.int64) + 500
    P = labels.size
    labels[40, 50] = n + 1
    d_labels, d_out = _lib.DeviceBuffer(P * 4).upload(labels), _lib.DeviceBuffer(P * 2)
    n_bad = ctypes.c_int32(-1)
    lib = _lib.lib()
    assert lib.tip_export_maps_u16_dev(d_labels.ptr, None, P, _lib.ptr(ids), n, d_out.ptr, ctypes.byref(n_bad)) == 0
    assert n_bad.value == 1
    want = np.insert(ids, 0, 0)[np.where(labels > n, 0, labels)].astype(np.uint16)
    np.testing.assert_array_equal(d_out.download(labels.shape, np.uint16), want)
    with pytest.raises(ValueError, match="label outside"):
        _deflate.export_maps_u16_dev(d_labels.ptr, None, P, ids, d_out.ptr)
    labels[40, 50] = -3
    labels[41, 50:53] = n + 2
    d_labels.upload(labels)
    assert lib.tip_export_maps_u16_dev(d_labels.ptr, None, P, _lib.ptr(ids), n, d_out.ptr, ctypes.byref(n_bad)) == 0
    assert n_bad.value == 4
    wide = ids.copy()
    wide[3] = 65536
    assert lib.tip_export_maps_u16_dev(d_labels.ptr, None, P, _lib.ptr(wide), n, d_out.ptr, ctypes.byref(n_bad)) == -2
    assert "65536" in _lib.last_error()
    wide[3] = -1
    assert lib.tip_export_maps_u16_dev(d_labels.ptr, None, P, _lib.ptr(wide), n, d_out.ptr, ctypes.byref(n_bad)) == -2
    assert lib.tip_export_maps_u16_dev(None, None, P, _lib.ptr(ids), n, d_out.ptr, ctypes.byref(n_bad)) == -2
    labels[labels > n] = 0
    labels[labels < 0] = 0
    d_labels.upload(labels)
    assert lib.tip_export_maps_u16_dev(d_labels.ptr, None, P, _lib.ptr(ids), n, d_out.ptr, ctypes.byref(n_bad)) == 0 and n_bad.value == 0


# ---- the mixin ------------------------------------------------------------------------------------------------------------
def _golden_tissue(g):
    import pandas as pd
    from tissue_image_processing_amd.tissue_info import Tissue
    T = int(g["valid_frames"].size)
    tissue = Tissue(T)
    for f in range(T):
        tissue.set_labels(f + 1, g["labels_%d" % f].copy())
        tissue.set_cells_info(f + 1, pd.DataFrame(dict(label=g["ids_%d" % f])))
        tissue.set_cell_types(f + 1, g["cell_types_%d" % f].copy())
    tissue.valid_frames = g["valid_frames"].copy()
    return tissue


@pytest.mark.parametrize("compression", ["device", None])
def test_mixin_exports_equal_the_reference(golden, tmp_path, compression):
    from tissue_image_processing_amd import basic_image_manipulations as bim
    g = golden("export_tiff")
    tissue = _golden_tissue(g)
    assert (g["valid_frames"] == 0).sum() == 1 and g["valid_frames"].size >= 3
    for method, name in ((tissue.export_segmentation_and_cell_types_to_tiff, "export_both"), (tissue.export_segmentation_to_tiff, "export_labels")):
        assert method(str(tmp_path), name, compression=compression) == 0
        path = str(tmp_path / (name + ".tif"))
        image, axes, shape, _ = bim.read_tiff(path)
        assert axes == str(g["axes"]) == "TCZYX" and image.dtype == np.uint16
        np.testing.assert_array_equal(image, g[name])
        page = bim.tiff_page_table(path).pages[0]
        assert page.compression == (8 if compression == "device" else 1)
        if compression == "device":
            assert os.path.getsize(path) < g[name].nbytes
    with pytest.raises(ValueError, match="compression"):
        tissue.export_segmentation_to_tiff(str(tmp_path), "bad", compression="zlib")


# ---- the driver -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def movie_run(tmp_path_factory):
    """One process: the default file, a second file with 7 rows per strip and fixed codes from the same backend, and what the run
    left on the GPU, downloaded."""
    from tissue_image_processing_amd import movie
    tmp = tmp_path_factory.mktemp("export")
    backend, ids, path = w.run_movie(str(tmp / "world1.tif"), 0, 1, None)
    try:
        assert path == str(tmp / "world1.tif")
        labels = [backend.labels[t].download((w.Y, w.X), np.int32) for t in range(w.T)]
        types = [backend.fetch_cell_types(t) for t in range(w.T)]
        ragged = movie.export_tiff(str(tmp / "rps7_fixed.tif"), w.T, backend, ids, rowsperstrip=7, codes="fixed", bigtiff=True)
        with pytest.raises(ValueError, match=r"\[2\]"):
            kept = backend.labels.pop(2)
            try:
                movie.export_tiff(str(tmp / "missing.tif"), w.T, backend, ids)
            finally:
                backend.labels[2] = kept
        assert not os.path.exists(str(tmp / "missing.tif"))
    finally:
        backend.close()
    return dict(path=path, ragged=ragged, ids=ids, labels=labels, types=types)


def test_export_tiff_holds_the_backends_maps(movie_run):
    from tissue_image_processing_amd import basic_image_manipulations as bim
    want = np.zeros((w.T, 2, 1, w.Y, w.X), np.uint16)
    for t in range(w.T):
        assert 1 < movie_run["labels"][t].max() <= len(movie_run["ids"][t])
        want[t, 0, 0] = np.insert(np.asarray(movie_run["ids"][t], np.int64), 0, 0)[movie_run["labels"][t]].astype(np.uint16)
        want[t, 1, 0] = _remap(movie_run["types"][t])
    assert (want[:, 0] > 0).any() and (want[:, 1] == 0).any() and (want[:, 1] > 0).any()
    for key, big, rps in (("path", False, w.Y), ("ragged", True, 7)):
        image, axes, shape, _ = bim.read_tiff(movie_run[key])
        assert axes == "TCZYX" and shape == want.shape and image.dtype == np.uint16
        np.testing.assert_array_equal(image, want)
        table = bim.tiff_page_table(movie_run[key])
        assert table.big == big and len(table.pages) == 2 * w.T
        assert all(pg.rows_per_strip == rps and pg.compression == 8 and pg.predictor == 1 for pg in table.pages)
    assert os.path.getsize(movie_run["path"]) < want.nbytes


def test_two_processes_write_the_same_file(tmp_path, movie_run):
    out = str(tmp_path / "world2.tif")
    run_ranks("_gpu_movie_export_worker.py", 2, (out,), timeout=600, local_rank="0")
    assert open(out, "rb").read() == open(movie_run["path"], "rb").read()
