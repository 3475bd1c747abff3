"""GPU: the projected movie written from the GPUs -- csrc/tip_export.hip's page, maximum and z-map kernels against
tiff.tiff_normalise and numpy (the cases of tests/test_export_projection_host.py), movie.export_projection after process_movie
against the projections and z-maps the backend kept, in one process and in two, and movie_surface_projection's
compression="device" against its uncompressed file."""
import os

import numpy as np
import pytest

import _gpu_movie_projection_worker as w
from gloo_launch import run_ranks
from test_export_projection_host import PAGE_SHAPES, differenced, page_planes

pytestmark = pytest.mark.gpu


def _device_pages(a, scale_max, predictor, offset=0):
    """the page kernel on a device copy of `a` that starts `offset` samples into its buffers; what lies around the pages is kept"""
    from tissue_image_processing_amd import _deflate, _lib
    n = a.size
    d_src, d_out = _lib.DeviceBuffer((n + offset) * 8), _lib.DeviceBuffer((n + offset + 4) * 2)
    d_src.upload(np.concatenate([np.full(offset, 7.0e9), a.ravel()]))
    d_out.upload(np.full(n + offset + 4, 0xABCD, np.uint16))
    _deflate.projection_pages_u16_dev(d_src.ptr + 8 * offset, a.shape[0], a.shape[1], a.shape[2], scale_max, predictor, d_out.ptr + 2 * offset)
    got = d_out.download((n + offset + 4,), np.uint16)
    assert (got[:offset] == 0xABCD).all() and (got[offset + n:] == 0xABCD).all()      # nothing outside the pages is written
    return got[offset:offset + n].reshape(a.shape)


# ---- the kernels ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0, 1])      # 1: the addresses are not on 16 and 8 bytes -- one sample per thread
@pytest.mark.parametrize("shape", PAGE_SHAPES)
def test_device_pages_are_tiff_normalise(shape, offset):
    from tissue_image_processing_amd import _deflate
    from tissue_image_processing_amd.tiff import tiff_normalise
    a = page_planes(shape)
    want = tiff_normalise(a, "uint16")
    assert want.max() == 65535
    np.testing.assert_array_equal(_device_pages(a, a.max(), 1, offset), want)
    np.testing.assert_array_equal(_device_pages(a, a.max(), 2, offset), differenced(want))
    np.testing.assert_array_equal(_deflate.projection_pages_u16(a, a.max(), 2), differenced(want))      # the host twin agrees


def test_device_pages_round_ties_and_edges_as_numpy():
    a = np.array([[[4096.0, 1.0, 8191.999, 8192.0, 0.0]]])
    got = _device_pages(a, 8192.0, 1)
    np.testing.assert_array_equal(got, [[[32768, 8, 65535, 65535, 0]]])
    np.testing.assert_array_equal(_device_pages(np.tile(a, (1, 1, 4)), 8192.0, 1), np.tile(got, (1, 1, 4)))      # in the four-sample form


def test_device_pages_of_a_zero_plane_and_of_an_all_zero_movie():
    from tissue_image_processing_amd.tiff import tiff_normalise
    a = page_planes((2, 5, 7))
    a[0] = 0.0
    np.testing.assert_array_equal(_device_pages(a, a.max(), 1), tiff_normalise(a, "uint16"))
    for predictor in (1, 2):
        assert not _device_pages(np.zeros((2, 5, 7)), 0.0, predictor).any()


def test_device_predictor_2_wraps_and_restarts_every_row():
    rows = np.array([[65535.0, 0.0, 0.0, 65535.0, 7.0],
                     [3.0, 3.0, 65535.0, 1.0, 65535.0],
                     [2.0, 0.0, 65535.0, 65535.0, 0.0]])
    for planes in (rows[None], np.concatenate([rows, rows[:, :3]], axis=1)[None]):      # 5 columns: rows cross the fours; 8: they do not
        u = planes.astype(np.uint16)
        got = _device_pages(planes, 65535.0, 2)
        np.testing.assert_array_equal(got, differenced(u))
        np.testing.assert_array_equal(np.cumsum(got, axis=-1, dtype=np.uint16), u)
    assert _device_pages(rows[None], 65535.0, 2)[0, :, 0].tolist() == [65535, 3, 2]


def test_device_pages_reject_a_bad_maximum_and_another_predictor():
    from tissue_image_processing_amd import _lib
    a = page_planes((1, 2, 3))
    for bad in (-1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="scale_max"):
            _device_pages(a, bad, 1)
    with pytest.raises(_lib.TissueHipError, match="predictor 3"):
        _device_pages(a, 1.0, 3)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4099, 2048 * 1024 + 77])      # the last: every workgroup strides more than once
def test_device_maximum(n):
    from tissue_image_processing_amd import _deflate, _lib
    d = _lib.DeviceBuffer(n * 8)
    for at in sorted({0, n // 2, n - 1}):
        v = np.random.default_rng(n).random(n) - 0.5
        v[at] = 0.75
        d.upload(v)
        assert _deflate.max_f64_dev(d.ptr, n) == 0.75
    d.upload(-np.arange(1.0, n + 1))
    assert _deflate.max_f64_dev(d.ptr, n) == -1.0
    with pytest.raises(ValueError, match="at least one"):
        _deflate.max_f64_dev(d.ptr, 0)


@pytest.mark.parametrize("offset", [0, 1])
def test_device_zmap_wraps(offset):
    from tissue_image_processing_amd import _deflate, _lib
    z = np.concatenate([np.array([0, 5, 70000, -1], np.int64), np.random.default_rng(2).integers(-2 ** 40, 2 ** 40, 63)])
    for n in (4, 67):
        d_src, d_out = _lib.DeviceBuffer((n + offset) * 8), _lib.DeviceBuffer((n + offset + 4) * 2)
        d_src.upload(np.concatenate([np.zeros(offset, np.int64), z[:n]]))
        d_out.upload(np.full(n + offset + 4, 0xABCD, np.uint16))
        _deflate.zmap_u16_dev(d_src.ptr + 8 * offset, n, d_out.ptr + 2 * offset)
        got = d_out.download((n + offset + 4,), np.uint16)
        np.testing.assert_array_equal(got[offset:offset + n], z[:n].astype("uint16"))
        assert got[offset:offset + 4].tolist() == [0, 5, 4464, 65535]
        assert (got[:offset] == 0xABCD).all() and (got[offset + n:] == 0xABCD).all()


# ---- the driver -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def movie_run(tmp_path_factory):
    """One process: the default file and its z-maps, a second file with 7 rows per strip, fixed codes, predictor 2 as BigTIFF from the
    same backend, and what the run kept on the GPU, downloaded."""
    from tissue_image_processing_amd import movie
    tmp = tmp_path_factory.mktemp("projection")
    backend = w.run_movie(0, 1, None)
    try:
        first = movie.export_projection(str(tmp / "position1.tif"), w.T, backend)
        projections = np.stack([backend.fetch_projection(t) for t in range(w.T)])
        zmaps = np.stack([backend.fetch_zmap(t) for t in range(w.T)])
        maxima = [backend.projection_max(t) for t in range(w.T)]
        ragged = movie.export_projection(str(tmp / "ragged.tif"), w.T, backend, rowsperstrip=7, codes="fixed", predictor=2, bigtiff=True,
                                         zmap=False)
        last = backend.pipe.fetch_projection()
    finally:
        backend.close()
    assert not backend.projections and not backend.zmaps      # close() freed them
    return dict(first=first, ragged=ragged, projections=projections, zmaps=zmaps, maxima=maxima, last=last, tmp=tmp)


def test_the_backend_keeps_every_frames_projection(movie_run):
    p, z = movie_run["projections"], movie_run["zmaps"]
    assert p.shape == (w.T, w.C, w.Y, w.X) and p.dtype == np.float64 and z.shape == (w.T, w.Y, w.X) and z.dtype == np.int64
    np.testing.assert_array_equal(p[-1], movie_run["last"][0])      # the pipeline still holds the last frame
    np.testing.assert_array_equal(z[-1], movie_run["last"][1])
    assert len({p[t].tobytes() for t in range(w.T)}) == w.T and p.min() >= 0 and 0 <= z.min() < z.max() < w.Z
    assert movie_run["maxima"] == [p[t].max() for t in range(w.T)]


def test_export_projection_holds_the_kept_projections(movie_run):
    from tissue_image_processing_amd import basic_image_manipulations as bim
    path, zmap_path = movie_run["first"]
    assert path == str(movie_run["tmp"] / "position1.tif") and zmap_path == str(movie_run["tmp"] / "zmap_position1.npy")
    want = bim.tiff_normalise(movie_run["projections"], "uint16")
    assert want.max() == 65535 and min(want[t].max() for t in range(w.T)) < 65535      # the scale is the movie's, not a frame's
    image, axes, shape, _ = bim.read_tiff(path)
    assert axes == "TCYX" and shape == want.shape and image.dtype == np.uint16
    np.testing.assert_array_equal(image, want)
    table = bim.tiff_page_table(path)
    assert not table.big and len(table.pages) == w.T * w.C
    assert all(pg.rows_per_strip == w.Y and pg.compression == 8 and pg.predictor == 1 for pg in table.pages)
    zmaps = np.load(zmap_path)
    assert zmaps.shape == (w.T, 1, 1, w.Y, w.X) and zmaps.dtype == np.uint16
    np.testing.assert_array_equal(zmaps[:, 0, 0], movie_run["zmaps"].astype("uint16"))


def test_export_projection_with_predictor_2_fixed_codes_and_ragged_strips(movie_run):
    from tissue_image_processing_amd import basic_image_manipulations as bim
    path, zmap_path = movie_run["ragged"]
    assert zmap_path is None and not os.path.exists(str(movie_run["tmp"] / "zmap_ragged.npy"))
    image, axes, _, _ = bim.read_tiff(path)
    assert axes == "TCYX"
    np.testing.assert_array_equal(image, bim.tiff_normalise(movie_run["projections"], "uint16"))
    table = bim.tiff_page_table(path)
    assert table.big and len(table.pages) == w.T * w.C
    assert all(pg.rows_per_strip == 7 and pg.compression == 8 and pg.predictor == 2 for pg in table.pages)


def test_the_dynamic_file_is_smaller_than_the_raw_pages(movie_run):
    """The host form of the strip encoder on these very pages shrinks them under dynamic codes, so the file has to; nothing is
    asserted under fixed codes, where a literal from 144 up costs 9 bits."""
    from tissue_image_processing_amd import _deflate
    from tissue_image_processing_amd import basic_image_manipulations as bim
    pages = bim.tiff_normalise(movie_run["projections"], "uint16")
    streams = _deflate.deflate_strips(pages, w.Y, "dynamic")
    host_form = sum(len(s) for page in streams for s in page)
    size = os.path.getsize(movie_run["first"][0])
    print("raw %d bytes, host form's strips %d, the file %d" % (pages.nbytes, host_form, size))
    assert host_form < pages.nbytes
    assert size < w.T * w.C * w.Y * w.X * 2


def test_two_processes_write_the_same_files(tmp_path, movie_run):
    out = str(tmp_path / "position1.tif")
    run_ranks("_gpu_movie_projection_worker.py", 2, (out,), timeout=600, local_rank="0")
    assert open(out, "rb").read() == open(movie_run["first"][0], "rb").read()
    np.testing.assert_array_equal(np.load(str(tmp_path / "zmap_position1.npy")), np.load(movie_run["first"][1]))


def test_export_projection_without_kept_projections_names_the_frames(tmp_path):
    from tissue_image_processing_amd import movie
    backend = w.run_movie(0, 1, None, keep_projection=False)
    try:
        assert not backend.projections and not backend.zmaps
        with pytest.raises(ValueError, match=r"\[0, 1, 2, 3\].*keep_projection"):
            movie.export_projection(str(tmp_path / "none.tif"), w.T, backend)
        assert not os.listdir(str(tmp_path))
    finally:
        backend.close()


# ---- movie_surface_projection -----------------------------------------------------------------------------------------------
def test_movie_surface_projection_on_the_device_writes_the_same_movie(tmp_path):
    from tissue_image_processing_amd import basic_image_manipulations as bim, surface_projection as sp
    source = np.stack(w.stacks()[:2])      # an in-memory movie (T 2, C 2, Z, Y, X)
    images = {}
    for compression in (None, "device", "zlib"):
        odir = tmp_path / str(compression)
        odir.mkdir()
        sp.movie_surface_projection([source], 0, (1,), 1, str(odir), "max_averages", 1, False, 0, 0, 0, False, compression=compression)
        path = str(odir / "position1.tif")
        images[compression] = bim.read_tiff(path)
        assert bim.tiff_page_table(path).pages[0].compression == (1 if compression is None else 8)
        assert os.path.exists(str(odir / "zmap_position1.npy"))
    image, axes, shape, _ = images[None]
    assert axes == "TCYX" and shape == (2, w.C, w.Y, w.X) and image.dtype == np.uint16 and image.any()
    for compression in ("device", "zlib"):
        assert images[compression][1:3] == (axes, shape)
        np.testing.assert_array_equal(images[compression][0], image)
    with pytest.raises(ValueError, match="compression"):
        sp.movie_surface_projection([source], 0, (1,), 1, str(tmp_path), "max_averages", 1, False, 0, 0, 0, False, compression="lzw")


def test_save_projection_tiff_normalises_a_float64_movie_as_save_tiff_does(tmp_path):
    from tissue_image_processing_amd import basic_image_manipulations as bim
    from tissue_image_processing_amd.tiff_export import save_projection_tiff
    movie = np.stack([page_planes((2, 33, 130), seed=t) * (1.0 - 0.3 * t) for t in range(2)])
    plain, device = str(tmp_path / "plain.tif"), str(tmp_path / "device.tif")
    bim.save_tiff(plain, movie, metadata="<OME/>", axes="TCYX", data_type="uint16")
    assert save_projection_tiff(device, movie, metadata="<OME/>", rowsperstrip=8, predictor=2) == device
    want = bim.read_tiff(plain)
    got = bim.read_tiff(device)
    assert got[1:3] == want[1:3] == ("TCYX", movie.shape)
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[0], bim.tiff_normalise(movie, "uint16"))
    assert all(pg.predictor == 2 and pg.rows_per_strip == 8 for pg in bim.tiff_page_table(device).pages)


def test_unet_mode_keeps_the_same_projections(tmp_path):
    """In U-Net mode the pipeline's projection is a torch tensor; two frames in flight on two pipelines keep what the classical mode keeps."""
    import _gpu_movie_unet_worker as U
    from tissue_image_processing_amd import basic_image_manipulations as bim
    from tissue_image_processing_amd import movie
    stacks = U.movie_stacks(frames=2)
    kept = {}
    for mode, kw in (("classical", {}), ("unet", dict(segmentation="unet", predictor_factory=U.predictor_factory(stacks), inflight=2))):
        backend = movie.GpuFrameBackend(2, U.Z, U.Y, U.X, device=0, keep_projection=True, **kw)
        try:
            movie.process_movie(2, lambda t: stacks[t], backend, drifts=U.drift_rows(2))
            kept[mode] = (np.stack([backend.fetch_projection(t) for t in range(2)]), np.stack([backend.fetch_zmap(t) for t in range(2)]))
            if mode == "unet":
                path, zmap_path = movie.export_projection(str(tmp_path / "unet.tif"), 2, backend)
        finally:
            backend.close()
    assert kept["classical"][0].any() and kept["classical"][1].any()
    np.testing.assert_array_equal(kept["unet"][0], kept["classical"][0])
    np.testing.assert_array_equal(kept["unet"][1], kept["classical"][1])
    np.testing.assert_array_equal(bim.read_tiff(path)[0], bim.tiff_normalise(kept["unet"][0], "uint16"))
    np.testing.assert_array_equal(np.load(zmap_path)[:, 0, 0], kept["unet"][1].astype("uint16"))
