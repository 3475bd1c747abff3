"""CPU: the projected movie's export without a device -- the host twins of csrc/tip_export.hip's page, maximum and z-map kernels
(compiled from the kernels' per-sample functions) against tiff.tiff_normalise and numpy, write_tiff_strips' predictor and xml
arguments read back by tiff_page_table and read_tiff, and movie.export_projection on gloo with a backend whose pages come from
numpy and whose strips come from the host's zlib."""
import os
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from gloo_launch import run_ranks  # noqa: E402

PAGE_SHAPES = [(1, 1, 1), (2, 5, 7), (2, 33, 130)]      # one sample; 70 samples: 17 fours and a tail of 2; 32 fours and a half per row


def page_planes(shape, seed=0):
    """float64 planes whose maximum, 4003.25, is one of the samples; plane 0's first row is zero"""
    a = np.random.default_rng(seed).random(shape) * 4000.0
    a[0, 0] = 0.0
    a[-1, -1, -1] = 4003.25
    return a


def differenced(pages):
    return np.concatenate([pages[..., :1], np.diff(pages, axis=-1)], axis=-1).astype(np.uint16)


# ---- the page function ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", PAGE_SHAPES)
def test_host_pages_are_tiff_normalise(shape):
    from tissue_image_processing_amd import _deflate
    from tissue_image_processing_amd.tiff import tiff_normalise
    a = page_planes(shape)
    want = tiff_normalise(a, "uint16")
    assert want.dtype == np.uint16 and want.max() == 65535
    got = _deflate.projection_pages_u16(a, a.max(), 1)
    assert got.dtype == np.uint16 and got.shape == a.shape
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(_deflate.projection_pages_u16(a, a.max(), 2), differenced(want))


def test_host_pages_round_ties_and_edges_as_numpy():
    from tissue_image_processing_amd import _deflate
    a = np.array([[[4096.0, 1.0, 8191.999, 8192.0, 0.0]]])
    got = _deflate.projection_pages_u16(a, 8192.0, 1)
    np.testing.assert_array_equal(got, [[[32768, 8, 65535, 65535, 0]]])      # 32767.5 is a tie: to the even 32768
    np.testing.assert_array_equal(got, np.round((a / 8192.0) * 65535).astype("uint16"))


def test_host_pages_of_a_zero_plane_and_of_an_all_zero_movie():
    from tissue_image_processing_amd import _deflate
    from tissue_image_processing_amd.tiff import tiff_normalise
    a = page_planes((2, 5, 7))
    a[0] = 0.0
    got = _deflate.projection_pages_u16(a, a.max(), 1)
    assert not got[0].any() and got[1].max() == 65535
    np.testing.assert_array_equal(got, tiff_normalise(a, "uint16"))
    for predictor in (1, 2):
        assert not _deflate.projection_pages_u16(np.zeros((2, 5, 7)), 0.0, predictor).any()


def test_host_predictor_2_wraps_and_restarts_every_row():
    from tissue_image_processing_amd import _deflate
    m = 65535.0      # with this maximum a whole-numbered sample is its own page value
    rows = np.array([[65535.0, 0.0, 0.0, 65535.0, 7.0],
                     [3.0, 3.0, 65535.0, 1.0, 65535.0],      # the row above ends low, this one high ...
                     [2.0, 0.0, 65535.0, 65535.0, 0.0]])     # ... and column 0 is never differenced across rows
    u = _deflate.projection_pages_u16(rows[None], m, 1)[0]
    np.testing.assert_array_equal(u, rows.astype(np.uint16))
    got = _deflate.projection_pages_u16(rows[None], m, 2)[0]
    np.testing.assert_array_equal(got, differenced(u))
    assert got[0].tolist() == [65535, 1, 0, 65535, 8] and got[1, 0] == 3 and got[2, 0] == 2
    np.testing.assert_array_equal(np.cumsum(got, axis=1, dtype=np.uint16), u)      # what a reader does


def test_host_pages_reject_a_bad_maximum_and_another_predictor():
    from tissue_image_processing_amd import _deflate, _lib
    a = page_planes((1, 2, 3))
    for bad in (-1.0, np.inf, -np.inf, np.nan):
        with pytest.raises(ValueError, match="scale_max"):
            _deflate.projection_pages_u16(a, bad, 1)
    with pytest.raises(_lib.TissueHipError, match="predictor 3"):
        _deflate.projection_pages_u16(a, 1.0, 3)


# ---- the maximum and the z-map --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4099])
def test_host_maximum(n):
    from tissue_image_processing_amd import _deflate
    for at in sorted({0, n // 2, n - 1}):
        v = np.random.default_rng(n).random(n) - 0.5
        v[at] = 0.75
        assert _deflate.max_f64(v) == 0.75 == v.max()
    assert _deflate.max_f64(-np.arange(1.0, n + 1)) == -1.0      # every value negative


def test_host_maximum_of_nothing_is_an_error():
    from tissue_image_processing_amd import _deflate
    with pytest.raises(ValueError, match="at least one"):
        _deflate.max_f64(np.zeros(0))


def test_host_zmap_wraps():
    from tissue_image_processing_amd import _deflate
    z = np.array([0, 5, 70000, -1], np.int64)
    got = _deflate.zmap_u16(z)
    assert got.dtype == np.uint16 and got.tolist() == [0, 5, 4464, 65535]
    np.testing.assert_array_equal(got, z.astype("uint16"))
    big = np.random.default_rng(2).integers(-2 ** 40, 2 ** 40, (7, 9))
    np.testing.assert_array_equal(_deflate.zmap_u16(big), big.astype("uint16"))


# ---- the writer -----------------------------------------------------------------------------------------------------------
def _zlib_strips(pages, rps):
    return [[zlib.compress(p[r:r + rps].tobytes(), 6) for r in range(0, p.shape[0], rps)] for p in pages]


@pytest.mark.parametrize("big", [False, True])
def test_written_predictor_2_strips_are_read_back(tmp_path, big):
    from tissue_image_processing_amd import basic_image_manipulations as bim
    shape, rps = (3, 2, 23, 31), 7
    array = (np.random.default_rng(5).integers(0, 65536, shape)).astype(np.uint16)
    array[0, 0, 0, :4] = (65535, 0, 0, 65535)
    pages = _zlib_strips(differenced(array).reshape((-1,) + shape[-2:]), rps)
    path = str(tmp_path / "p2.tif")
    assert bim.write_tiff_strips(path, shape, "TCYX", np.uint16, rps, pages, bigtiff=big, predictor=2, xml="<OME>a movie</OME>") == path
    table = bim.tiff_page_table(path)
    assert table.big == big and len(table.pages) == 6
    assert all((pg.compression, pg.predictor, pg.rows_per_strip) == (8, 2, rps) for pg in table.pages)
    image, axes, got_shape, _ = bim.read_tiff(path)
    assert axes == "TCYX" and got_shape == shape and image.dtype == np.uint16
    np.testing.assert_array_equal(image, array)
    assert b"axes=TCYX shape=3x2x23x31\n<OME>a movie</OME>\0" in open(path, "rb").read()
    # the classic form is save_tiff's file
    if not big:
        same = str(tmp_path / "save_tiff.tif")
        bim.save_tiff(same, array, metadata="<OME>a movie</OME>", axes="TCYX", compression="zlib", predictor=2, rowsperstrip=rps)
        assert open(same, "rb").read() == open(path, "rb").read()


def test_the_new_arguments_default_to_the_old_file(tmp_path):
    from tissue_image_processing_amd import basic_image_manipulations as bim
    array = np.random.default_rng(6).integers(0, 900, (2, 11, 17)).astype(np.uint16)
    pages = _zlib_strips(array, 4)
    a, b = str(tmp_path / "a.tif"), str(tmp_path / "b.tif")
    bim.write_tiff_strips(a, array.shape, "TYX", np.uint16, 4, pages)
    bim.write_tiff_strips(b, array.shape, "TYX", np.uint16, 4, pages, predictor=1, xml=None)
    assert open(a, "rb").read() == open(b, "rb").read()
    assert all(pg.predictor == 1 for pg in bim.tiff_page_table(a).pages)
    with pytest.raises(ValueError, match="predictor"):
        bim.write_tiff_strips(a, array.shape, "TYX", np.uint16, 4, pages, predictor=3)


# ---- the driver -----------------------------------------------------------------------------------------------------------
def _export(tmp_path, world, n_frames, predictor=1, missing=-1):
    folder = tmp_path / ("w%d_n%d_p%d_m%d" % (world, n_frames, predictor, missing))
    folder.mkdir()
    path = str(folder / "position3.tif")
    run_ranks("_movie_projection_worker.py", world, (path, n_frames, predictor, missing), timeout=300)
    return path


def _zmap_file(path):
    return os.path.join(os.path.dirname(path), "zmap_position3.npy")


@pytest.mark.parametrize("predictor", [1, 2])
def test_export_projection_is_the_same_file_at_every_world_size(tmp_path, predictor):
    import _movie_projection_worker as w
    from tissue_image_processing_amd import basic_image_manipulations as bim
    n = 4
    frames = w.projection_movie(n)
    movie, zmaps = w.expected_movie(frames)
    # the scale is the movie's: a frame whose own maximum is lower would come out brighter on its own
    own = bim.tiff_normalise(frames[2][0], "uint16")
    assert movie[2].max() < 52000 and own.max() == 65535 and movie.max() == 65535
    paths = [_export(tmp_path, world, n, predictor) for world in (1, 2, 3)]
    files = [open(p, "rb").read() for p in paths]
    assert all(f == files[0] for f in files[1:])
    image, axes, shape, _ = bim.read_tiff(paths[-1])
    assert axes == "TCYX" and shape == (n, w.C, w.Y, w.X) and image.dtype == np.uint16
    np.testing.assert_array_equal(image, movie)
    assert all(pg.predictor == predictor and pg.rows_per_strip == w.ROWS_PER_STRIP for pg in bim.tiff_page_table(paths[0]).pages)
    for p in paths:
        got = np.load(_zmap_file(p))
        assert got.shape == (n, 1, 1, w.Y, w.X) and got.dtype == np.uint16
        np.testing.assert_array_equal(got, zmaps)
    assert (zmaps < 30).any() and zmaps.max() < 65536 and any(f[1].max() > 65535 for f in frames)      # the z-maps wrapped


def test_export_projection_with_fewer_frames_than_ranks(tmp_path):
    import _movie_projection_worker as w
    from tissue_image_processing_amd import basic_image_manipulations as bim
    a, b = _export(tmp_path, 1, 2), _export(tmp_path, 3, 2)
    assert open(a, "rb").read() == open(b, "rb").read()
    movie, zmaps = w.expected_movie(w.projection_movie(2))
    np.testing.assert_array_equal(bim.read_tiff(b)[0], movie)
    np.testing.assert_array_equal(np.load(_zmap_file(b)), zmaps)


@pytest.mark.parametrize("world", [1, 3])
def test_a_missing_projection_raises_on_every_rank(tmp_path, world):
    path = _export(tmp_path, world, 4, missing=2)
    assert not os.path.exists(path) and not os.path.exists(_zmap_file(path))
    for rank in range(world):
        message = open("%s.rank%d.err" % (path, rank)).read()
        assert "[2]" in message and "keep_projection" in message


def test_export_projection_checks_its_arguments_before_encoding(tmp_path):
    import _movie_projection_worker as w
    from tissue_image_processing_amd import movie
    backend = w.HostProjectionBackend(w.projection_movie(2), [0, 1])
    path = str(tmp_path / "unused.tif")
    with pytest.raises(ValueError, match="codes"):
        movie.export_projection(path, 2, backend, codes="best")
    with pytest.raises(ValueError, match="predictor"):
        movie.export_projection(path, 2, backend, predictor=3)
    with pytest.raises(ValueError, match="rowsperstrip"):
        movie.export_projection(path, 2, backend, rowsperstrip=0)
    backend.X = 32769      # a row over 64 KB
    with pytest.raises(ValueError, match="32769"):
        movie.export_projection(path, 2, backend)
    assert not backend.calls and not os.path.exists(path)


def test_export_projection_without_zmap_and_with_metadata(tmp_path):
    import _movie_projection_worker as w
    from tissue_image_processing_amd import basic_image_manipulations as bim
    from tissue_image_processing_amd import movie

    class Meta(object):
        def to_xml(self):
            return "<OME>three frames</OME>"

    frames = w.projection_movie(3)
    backend = w.HostProjectionBackend(frames, [0, 1, 2])
    path = str(tmp_path / "movie.tif")
    assert movie.export_projection(path, 3, backend, zmap=False, metadata=Meta()) == (path, None)
    assert os.listdir(str(tmp_path)) == ["movie.tif"]
    np.testing.assert_array_equal(bim.read_tiff(path)[0], w.expected_movie(frames)[0])
    assert b"\n<OME>three frames</OME>\0" in open(path, "rb").read()
    assert all(pg.rows_per_strip == w.Y for pg in bim.tiff_page_table(path).pages)      # the default: 64 KB hold the page
