"""CPU: the strip-wise zlib framing's restatement (tests/deflate_strips_restate.py) -- zlib inflates every strip, the maps shrink --,
basic_image_manipulations.write_tiff_strips read back by read_tiff, tiff_page_table and the lazy open_image in classic form and as
BigTIFF, the writers' files against their restated layouts (tests/tiff_layout_restate.py), tiff.py's strip geometry and the names
basic_image_manipulations re-exports, and movie.export_tiff on gloo with a backend whose strips come from the host's zlib."""
import os
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import deflate_strips_cases as sc  # noqa: E402
import deflate_strips_restate as sr  # noqa: E402
import tiff_layout_restate as lr  # noqa: E402
from gloo_launch import run_ranks  # noqa: E402


# ---- the restatement ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("codes", sr.CODES)
@pytest.mark.parametrize("name", sc.NAMES)
def test_zlib_inflates_every_restated_strip(name, codes):
    pages, rps = sc.CASES[name]
    streams, raw = sc.restated(name, codes), sr.raw_strips(pages, rps)
    assert len(streams) == len(raw) == pages.shape[0]
    for page, raw_page in zip(streams, raw):
        assert len(page) == len(raw_page) == -(-pages.shape[1] // rps)
        for stream, strip in zip(page, raw_page):
            assert stream[:2] == b"\x78\x01" and stream[-9:-4] == b"\x01\x00\x00\xff\xff"
            assert zlib.decompress(stream) == strip
            d = zlib.decompressobj()
            assert d.decompress(stream) == strip and d.eof and d.unused_data == b""      # nothing behind the Adler-32
            assert len(stream) <= sr.strip_bound(len(strip))
    data, table = sr.compact(streams)
    assert all(o % 2 == 0 for o, _ in table) and len(data) % 2 == 0
    assert len(data) <= sr.bound(pages.shape[0], pages.shape[1], pages.shape[2] * pages.dtype.itemsize, rps)
    for (o, n), stream in zip(table, [s for page in streams for s in page]):
        assert data[o:o + n] == stream


@pytest.mark.parametrize("codes", sr.CODES)
def test_the_voronoi_planes_shrink_at_least_eight_times(codes):
    pages = sc.ratio_pages()
    assert pages.shape == (2, 192, 256) and pages.dtype == np.uint16
    streams = sr.deflate_strips(pages, sc.RATIO_CASE["rows_per_strip"], codes)
    size = sum(len(s) for page in streams for s in page)
    print("%s codes: %d bytes of %d, %.2f times smaller" % (codes, size, pages.nbytes, pages.nbytes / size))
    assert pages.nbytes >= 8 * size


def test_a_strip_is_one_chunk_and_no_match_reaches_before_it():
    """Two equal strips: the second one's stream is the first one's (a match to the strip above would make it shorter)."""
    labels = sc.CASES["voronoi_96x128_rps16_u16"][0][0, :16]
    twice = np.concatenate([labels, labels])[None]
    for codes in sr.CODES:
        a, b = sr.deflate_strips(twice, 16, codes)[0]
        assert a == b


# ---- the writer -----------------------------------------------------------------------------------------------------------
def _zlib_pages(array, rps):
    planes = array.reshape((-1,) + array.shape[-2:])
    return [[zlib.compress(p[r:r + rps].tobytes(), 6) for r in range(0, p.shape[0], rps)] for p in planes]


WRITER_CASES = [("ragged", (3, 2, 1, 23, 31), np.uint16, 7),      # the last strip holds 2 rows; odd strip sizes occur
                ("one_strip", (2, 1, 1, 16, 24), np.uint16, 16),  # offsets and counts inline
                ("beyond", (2, 10, 12), np.uint16, 50),           # rowsperstrip above the page: one strip
                ("odd_u8", (4, 9, 13), np.uint8, 2),
                ("single_page", (11, 17), np.uint16, 3)]


@pytest.mark.parametrize("big", [False, True])
@pytest.mark.parametrize("name,shape,dtype,rps", WRITER_CASES)
def test_written_strips_are_read_back(tmp_path, name, shape, dtype, rps, big):
    from tissue_image_processing_amd import basic_image_manipulations as bim
    rng = np.random.default_rng(len(name))
    array = (rng.integers(0, 5, shape) * rng.integers(0, 300 if dtype == np.uint16 else 50, shape[-1])).astype(dtype)
    axes = "TCZYX"[5 - len(shape):]
    pages = _zlib_pages(array, min(rps, shape[-2]))
    assert name != "ragged" or any(len(s) & 1 for page in pages for s in page)      # (pad bytes are written)
    path = str(tmp_path / (name + ".tif"))
    assert bim.write_tiff_strips(path, shape, axes, dtype, rps, iter(pages), bigtiff=big) == path
    image, got_axes, got_shape, _ = bim.read_tiff(path)
    assert got_axes == axes and got_shape == shape and image.dtype == dtype
    np.testing.assert_array_equal(image, array)
    table = bim.tiff_page_table(path)
    assert table.big == big and table.byte_order == "<" and len(table.pages) == int(np.prod(shape[:-2]))
    flat = [s for page in pages for s in page]
    k = 0
    for pg in table.pages:
        assert (pg.compression, pg.predictor, pg.rows_per_strip, pg.bits) == (8, 1, min(rps, shape[-2]), 8 * np.dtype(dtype).itemsize)
        assert len(pg.offsets) == len(pg.counts) == pg.strips
        for o, c in zip(pg.offsets, pg.counts):
            assert o % 2 == 0 and bytes(table.buf[o:o + c]) == flat[k]
            k += 1
    assert k == len(flat)
    src = bim.open_image(path)
    full = array.reshape((1,) * (5 - len(shape)) + shape)
    assert tuple(src.dims) == full.shape
    t, c = full.shape[0] - 1, full.shape[1] - 1
    np.testing.assert_array_equal(src.block(t, c, 0, slice(1, 9), slice(2, 11)), full[t, c, 0, 1:9, 2:11])
    if not big and len(shape) > 2:      # the classic form is save_tiff(compression="zlib")'s file
        same = str(tmp_path / (name + "_save_tiff.tif"))
        bim.save_tiff(same, array, axes=axes, compression="zlib", rowsperstrip=rps)
        assert open(same, "rb").read() == open(path, "rb").read()


def test_the_writer_chooses_bigtiff_from_the_sizes(tmp_path):
    from tissue_image_processing_amd import basic_image_manipulations as bim
    array = np.zeros((2, 8, 8), np.uint16)
    pages = _zlib_pages(array, 8)
    small = bim.write_tiff_strips(str(tmp_path / "list.tif"), array.shape, "TYX", np.uint16, 8, pages)
    assert not bim.tiff_page_table(small).big
    # pages that arrive one by one: their sizes are not known, the uncompressed size decides -- 70000 pages of 256 x 128 uint16
    # are 4.3 GiB raw; the writer is stopped after its first page
    shape = (70000, 256, 128)
    strips = _zlib_pages(np.zeros((1, 256, 128), np.uint16), 256)[0]

    def one_page_then_stop():
        yield strips
        raise KeyboardInterrupt

    path = str(tmp_path / "stream.tif")
    with pytest.raises(KeyboardInterrupt):
        bim.write_tiff_strips(path, shape, "TYX", np.uint16, 256, one_page_then_stop())
    assert open(path, "rb").read(4) == b"II\x2b\x00"
    with pytest.raises(KeyboardInterrupt):
        bim.write_tiff_strips(path, (60000, 256, 128), "TYX", np.uint16, 256, one_page_then_stop())
    assert open(path, "rb").read(4) == b"II\x2a\x00"


def test_the_writer_rejects_what_it_cannot_write(tmp_path):
    from tissue_image_processing_amd import basic_image_manipulations as bim
    path = str(tmp_path / "bad.tif")
    pages = _zlib_pages(np.zeros((2, 8, 8), np.uint16), 3)
    with pytest.raises(TypeError):
        bim.write_tiff_strips(path, (2, 8, 8), "TYX", np.float32, 3, pages)
    with pytest.raises(ValueError, match="rowsperstrip"):
        bim.write_tiff_strips(path, (2, 8, 8), "TYX", np.uint16, 0, pages)
    with pytest.raises(ValueError, match="strips"):
        bim.write_tiff_strips(path, (2, 8, 8), "TYX", np.uint16, 4, pages)
    with pytest.raises(ValueError, match="pages"):
        bim.write_tiff_strips(path, (3, 8, 8), "TYX", np.uint16, 3, pages)
    with pytest.raises(ValueError, match="pages"):
        bim.write_tiff_strips(path, (1, 8, 8), "TYX", np.uint16, 3, pages)


# ---- the files' bytes against their restated layouts (tests/tiff_layout_restate.py) --------------------------------------------
@pytest.mark.parametrize("big", [False, True])
@pytest.mark.parametrize("name,shape,dtype,rps", WRITER_CASES)
def test_written_strips_are_the_restated_file(tmp_path, name, shape, dtype, rps, big):
    """The strips are arbitrary bytes of odd and even sizes: the writer never inflates them, and the pin does not depend on the zlib
    build."""
    from tissue_image_processing_amd import basic_image_manipulations as bim
    rng = np.random.default_rng(100 + len(name))
    n_pages, n_strips = int(np.prod(shape[:-2])), -(-shape[-2] // min(rps, shape[-2]))
    pages = [[rng.integers(0, 256, 2 * int(rng.integers(1, 20)) + ((i + j) & 1), dtype=np.uint8).tobytes() for j in range(n_strips)]
             for i in range(n_pages)]
    assert any(len(s) & 1 for page in pages for s in page) and any(not len(s) & 1 for page in pages for s in page)
    axes = "TCZYX"[5 - len(shape):]
    path = str(tmp_path / (name + ".tif"))
    bim.write_tiff_strips(path, shape, axes, dtype, rps, iter(pages), bigtiff=big)
    assert open(path, "rb").read() == lr.strip_file(shape, axes, np.dtype(dtype), rps, pages, bigtiff=big)


@pytest.mark.parametrize("dtype,shapes", [(np.uint16, [(1, 1, 2, 5, 7), (2, 1, 1, 5, 7)]), (np.uint8, [(1, 2, 1, 5, 7), (2, 1, 1, 5, 7)])])
def test_appended_bigtiff_is_the_restated_file(tmp_path, dtype, shapes):
    """virtually_concatenate_time_points on array sources: four pages, so three links are patched behind the header's.  A uint16
    plane of 5 x 7 is 70 bytes, a uint8 plane 35 (odd): the IFD behind either is moved to an 8-byte boundary, by 2 and by 5 bytes.
    (An IFD of ten entries is 216 bytes, so the plane behind it starts on a boundary without padding.)"""
    from tissue_image_processing_amd import basic_image_manipulations as bim
    rng = np.random.default_rng(9)
    movies = [rng.integers(0, 250, s).astype(dtype) for s in shapes]
    path = str(tmp_path / "cat.tif")
    bim.virtually_concatenate_time_points([[m] for m in movies], [1, 1], output_path=path)
    # every time point as (Z, C, Y, X): pages in frame, z, channel order
    planes = [m[t, c, z] for m in movies for t in range(m.shape[0]) for z in range(m.shape[2]) for c in range(m.shape[1])]
    assert len(planes) == 4 and planes[0].nbytes % 8 and (dtype != np.uint8 or planes[0].nbytes % 2)
    assert open(path, "rb").read() == lr.appended_bigtiff(planes)
    np.testing.assert_array_equal(bim.read_tiff(path)[0], np.stack(planes))


# (rows, rowsperstrip) -> the clamped rowsperstrip, the strip count, the rows of the last strip
STRIP_GEOMETRY = [((23, 7), (7, 4, 2)), ((16, 16), (16, 1, 16)), ((10, 50), (10, 1, 10)), ((1, 1), (1, 1, 1))]


@pytest.mark.parametrize("given,want", STRIP_GEOMETRY)
def test_strip_geometry_of_a_written_page(tmp_path, given, want):
    from tissue_image_processing_amd import basic_image_manipulations as bim
    (rows, rps), (clamped, n, last) = given, want
    path = str(tmp_path / "g.tif")
    bim.write_tiff_strips(path, (rows, 3), "YX", np.uint8, rps, [[b"ab"] * n])
    pg = bim.tiff_page_table(path).pages[0]
    assert (pg.rows_per_strip, pg.strips, pg.strip_rows(pg.strips - 1)) == (clamped, n, last)
    assert sum(pg.strip_rows(k) for k in range(pg.strips)) == rows


@pytest.mark.parametrize("given,want", STRIP_GEOMETRY)
def test_strip_geometry_helper(given, want):
    from tissue_image_processing_amd import tiff
    (rows, rps), (clamped, n, last) = given, want
    g = tiff.StripGeometry(rows, rps)
    assert (g.rows_per_strip, g.strips, g.strip_rows(n - 1)) == (clamped, n, last)
    assert sum(g.strip_rows(k) for k in range(n)) == rows


def test_default_rows_per_strip_is_what_64_kb_hold():
    from tissue_image_processing_amd import tiff
    assert tiff.STRIP_BYTES == 65536
    assert [tiff.default_rows_per_strip(r, b) for r, b in ((300, 400), (45, 140), (2048, 4096), (5, 100000), (7, 0))] == [163, 45, 16, 1, 7]


# dropin/basic_image_manipulations.__all__ before the TIFF code moved to tiff.py
DROPIN_NAMES = ['ImageDims', 'TIFF_DEFLATE', 'TiffPage', 'TiffTable', 'UINT16_MAXVAL', 'UINT8_MAXVAL', 'band_pass_filter', 'binary_image',
                'blur_image', 'calculate_drift', 'concatenate_time_points', 'extract_all_frames_from_a_scene', 'gaussian_taps',
                'get_image_dimensions', 'np', 'open_image', 'put_channel_axis_first', 'read_image_in_chunks', 'read_part_of_image',
                'read_tiff', 'read_virtual_image', 'read_whole_image', 'save_tiff', 'set_brightness', 'set_channel_brightness',
                'stretch_for_display', 'tiff_normalise', 'tiff_page_table', 'virtually_concatenate_time_points', 'watershed_segmentation',
                'write_tiff_strips']


def test_the_dropin_module_still_exports_every_name():
    import importlib.util
    from tissue_image_processing_amd import basic_image_manipulations as bim
    spec = importlib.util.spec_from_file_location("_dropin_bim", os.path.join(ROOT, "dropin", "basic_image_manipulations.py"))
    dropin = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(dropin)
    assert not set(DROPIN_NAMES) - set(dropin.__all__)
    for name in DROPIN_NAMES:
        assert getattr(dropin, name) is getattr(bim, name)


def test_the_tiff_module_is_a_leaf():
    """In a fresh interpreter tiff.py imports alone: no other module of the package comes with it."""
    import subprocess
    code = ("import sys; sys.path.insert(0, %r); import tissue_image_processing_amd.tiff as t; "
            "print(sorted(m for m in sys.modules if m.startswith('tissue_image_processing_amd.'))); "
            "print(t.TiffSource.__name__, t.write_tiff_strips.__name__)" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], check=True, capture_output=True, text=True, timeout=120).stdout.splitlines()
    assert out == ["['tissue_image_processing_amd.tiff']", "TiffSource write_tiff_strips"]


# ---- the driver -----------------------------------------------------------------------------------------------------------
def _export(tmp_path, world, n_frames, typed=1, missing=-1):
    path = str(tmp_path / ("w%d_n%d_t%d_m%d.tif" % (world, n_frames, typed, missing)))
    run_ranks("_tiff_export_worker.py", world, (path, n_frames, typed, missing), timeout=300)
    return path


@pytest.mark.parametrize("typed", [1, 0])
def test_export_tiff_is_the_same_file_at_every_world_size(tmp_path, typed):
    from _tiff_export_worker import expected_array, export_movie
    from tissue_image_processing_amd import basic_image_manipulations as bim
    n = 5
    want = expected_array(export_movie(n), typed)
    assert (want[:, 0].max(axis=(1, 2, 3)) > 100 * np.arange(n)).all()          # the ids are not the labels
    paths = [_export(tmp_path, world, n, typed) for world in ((1, 2, 4) if typed else (1, 2))]
    files = [open(p, "rb").read() for p in paths]
    assert all(f == files[0] for f in files[1:])
    image, axes, shape, _ = bim.read_tiff(paths[-1])
    assert axes == "TCZYX" and shape == (n, 2 if typed else 1, 1, 22, 30) and image.dtype == np.uint16
    np.testing.assert_array_equal(image, want)


def test_export_tiff_with_fewer_frames_than_ranks(tmp_path):
    from _tiff_export_worker import expected_array, export_movie
    from tissue_image_processing_amd import basic_image_manipulations as bim
    a, b = _export(tmp_path, 1, 3), _export(tmp_path, 4, 3)
    assert open(a, "rb").read() == open(b, "rb").read()
    np.testing.assert_array_equal(bim.read_tiff(b)[0], expected_array(export_movie(3), 1))


@pytest.mark.parametrize("world", [1, 2, 4])
def test_a_missing_frame_raises_on_every_rank(tmp_path, world):
    path = _export(tmp_path, world, 5, missing=3)
    assert not os.path.exists(path)
    for rank in range(world):
        assert "[3]" in open("%s.rank%d.err" % (path, rank)).read()


def test_export_tiff_rejects_wide_ids_before_encoding():
    from _tiff_export_worker import ZlibExportBackend, export_movie
    from tissue_image_processing_amd import movie
    frames = export_movie(2)
    backend = ZlibExportBackend(frames, [0, 1], True)
    ids = [frames[0][2], frames[1][2] + 65536]
    with pytest.raises(ValueError, match=r"\[1\].*65535"):
        movie.export_tiff("unused.tif", 2, backend, ids)
    assert not backend.calls
    with pytest.raises(ValueError, match="codes"):
        movie.export_tiff("unused.tif", 2, backend, ids, codes="best")
