"""GPU: compressed TIFF stacks through the movie driver -- movie.tiff_frame_source(decode="device") hands GpuFrameBackend the
compressed strips, FramePipeline.inflate_stack inflates them on the device into the stack project() reads.  The stack buffer
against the reference's arrays for every 16-bit fixture of tests/golden/tiff; process_movie on a compressed 3-frame movie
against the same movie passed as arrays, one and two frames in flight; a corrupted strip."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIFF = os.path.join(ROOT, "tests", "golden", "tiff")
Z, Y, X, T = 6, 128, 128, 3          # the smallest frame the movie GPU tests use (tests/_gpu_movie_graph_worker.py)


@pytest.mark.parametrize("name", ["zlib_rps7", "zlib_rps7_bigtiff", "zlib_predictor_bigendian", "zlib_one_strip", "zlib_imagej"])
def test_inflated_stack_is_the_reference_s_array(name):
    """little- and big-endian, predictor 1 and 2, six ragged strips a page and one, page order TCZ and ImageJ's TZC"""
    from tissue_image_processing_amd import basic_image_manipulations as bim
    from tissue_image_processing_amd import movie
    from tissue_image_processing_amd.pipeline import FramePipeline
    g = np.load(os.path.join(TIFF, "expected.npz"), allow_pickle=False)
    want = bim._as_tczyx(g[name + "__image"], str(g[name + "__axes"]))
    source = movie.tiff_frame_source(os.path.join(TIFF, name + ".tif"), decode="device")
    assert tuple(source.dims) == want.shape and source.decode == "device" and source.n_frames == 2
    pipe = FramePipeline(*want.shape[1:], device=0)
    for t in range(2):
        frame = source(t)
        assert isinstance(frame, movie.CompressedFrame) and frame.shape == want.shape[1:]
        stack = pipe.inflate_stack(frame)
        got = stack.download(want.shape[1:], np.uint16)
        stack.free()
        assert np.array_equal(got, want[t]), (name, t)
    assert np.array_equal(movie.tiff_frame_source(os.path.join(TIFF, name + ".tif"), decode="host")(1), want[1])
    assert movie.tiff_frame_source(os.path.join(TIFF, "zlib_u8.tif")).decode == "host"        # 8-bit files take the host path


@pytest.fixture(scope="module")
def compressed_movie(tmp_path_factory):
    """(path, frames): a 3-frame movie written by save_tiff(compression="zlib", predictor=2), and its frames as arrays"""
    from tissue_image_processing_amd import basic_image_manipulations as bim
    from tissue_image_processing_amd import synthetic
    sites_t, is_hc = synthetic.make_movie_sites(Y, X, T, seed=9)
    frames = [synthetic.make_stack(Z, Y, X, seed=90 + t, sites=sites_t[t], is_hc=is_hc) for t in range(T)]
    path = str(tmp_path_factory.mktemp("tiffmovie") / "movie.tif")
    bim.save_tiff(path, np.stack(frames), axes="TCZYX", compression="zlib", predictor=2, rowsperstrip=24)     # 128 = 5 * 24 + 8: a ragged strip
    return path, frames


def _run(frame_source, inflight):
    from tissue_image_processing_amd import movie
    backend = movie.GpuFrameBackend(2, Z, Y, X, device=0, inflight=inflight)
    try:
        tabs, ids = movie.process_movie(T, frame_source, backend, 0, 1, None, "cpu", np.zeros((T, 2)), block_frames=T)
        labels = [backend.labels[t].download((Y, X), np.int32) for t in range(T)]
    finally:
        backend.close()
    return tabs, ids, labels


@pytest.fixture(scope="module")
def array_run(compressed_movie):
    _, frames = compressed_movie
    return _run(lambda t: frames[t], 1)


@pytest.mark.parametrize("inflight", [1, 2])
def test_compressed_movie_is_the_array_movie(compressed_movie, array_run, inflight):
    from tissue_image_processing_amd import movie
    path, _ = compressed_movie
    source = movie.tiff_frame_source(path, decode="device")
    tabs, ids, labels = _run(source, inflight)
    ref_tabs, ref_ids, ref_labels = array_run
    for t in range(T):
        assert np.array_equal(labels[t], ref_labels[t]), t
        assert np.array_equal(ids[t], ref_ids[t]), t
        assert set(tabs[t]) == set(ref_tabs[t])
        for k in tabs[t]:
            assert np.array_equal(tabs[t][k], ref_tabs[t][k]), (t, k)


def test_corrupted_strip_names_its_page_and_strip(compressed_movie, tmp_path):
    """One byte flipped inside page 15's strip 2 (frame 1: channel 0, z 3): the owner raises before it projects that frame."""
    from tissue_image_processing_amd import basic_image_manipulations as bim
    from tissue_image_processing_amd import movie
    path, _ = compressed_movie
    blob = bytearray(open(path, "rb").read())
    pg = bim.tiff_page_table(path).pages[15]
    blob[pg.offsets[2] + pg.counts[2] // 2] ^= 0xFF
    bad = str(tmp_path / "bad.tif")
    open(bad, "wb").write(bytes(blob))
    with pytest.raises(ValueError, match=r"frame 1, page 15 strip 2\b"):
        _run(movie.tiff_frame_source(bad, decode="device"), 1)
    with pytest.raises(ValueError, match=r"page 15 strip 2\b"):
        bim.read_tiff(bad)


def test_auto_knows_the_strip_count(compressed_movie, tmp_path):
    """decode="auto": 72 strips a frame (24 rows each) stay on the host, 1 536 (one row each) go to the device; a CPU backend
    and an 8-bit or uncompressed file never do."""
    from tissue_image_processing_amd import basic_image_manipulations as bim
    from tissue_image_processing_amd import movie
    path, frames = compressed_movie
    assert 72 < movie.AUTO_DEVICE_MIN_STRIPS <= 1536
    assert movie.tiff_frame_source(path).decode == "host"
    fine = str(tmp_path / "rows.tif")
    bim.save_tiff(fine, np.stack(frames[:1]), axes="TCZYX", compression="zlib", rowsperstrip=1)
    assert movie.tiff_frame_source(fine).decode == "device"
    assert movie.tiff_frame_source(fine, backend="cpu").decode == "host"
    assert movie.tiff_frame_source(os.path.join(TIFF, "plain_rps7.tif")).decode == "host"
    with pytest.raises(ValueError):
        movie.tiff_frame_source(os.path.join(TIFF, "plain_rps7.tif"), decode="device")
