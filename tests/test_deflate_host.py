"""CPU: the run-only deflate rule as restated in tests/deflate_restate.py (zlib inflates every case to its input, within the
bound), the CRC-32 combine, the `.npy` member builder and the raw zip writer of the movie driver's `.seg` export."""
import io
import os
import zipfile
import zlib

import numpy as np
import pytest

import deflate_cases as dc
import deflate_restate as dr


@pytest.mark.parametrize("name", dc.NAMES)
def test_restated_stream_inflates_to_the_input(name):
    _, data, e = dc.BY_NAME[name]
    stream = dc.restated(name)
    assert dr.inflate(stream) == data
    assert len(stream) <= dr.bound(len(data))
    if not data:
        assert stream == b""


def test_restated_chunks_concatenate_by_bytes():
    """A chunk's stream does not depend on its neighbours: the stream of a buffer is the streams of its chunks, one after
    another -- and a run across the chunk edge starts again with a literal element (no match reaches before its chunk)."""
    _, data, e = dc.BY_NAME["edge_65540B_e4"]
    assert dc.restated("edge_65540B_e4") == dr.deflate_runs(data[:dr.CHUNK], e) + dr.deflate_runs(data[dr.CHUNK:], e)
    assert dr.chunk_tokens(data[:dr.CHUNK], e)[-1] == ("match", 19 * 4)          # the run reaches the first chunk's end ...
    assert dr.chunk_tokens(data[dr.CHUNK:], e) == [("lit", 1), ("lit", 2), ("lit", 3), ("lit", 4)]      # ... and goes on as literals


def test_rule_on_small_inputs():
    """The rule's thresholds, token by token."""
    assert dr.chunk_tokens(b"\x05" * 3, 1) == [("lit", 5)] * 3                      # a run of 2 bytes stays literals (e = 1)
    assert dr.chunk_tokens(b"\x05" * 4, 1) == [("lit", 5), ("match", 3)]
    assert dr.chunk_tokens(b"\x01\x02" * 2, 2) == [("lit", 1), ("lit", 2)] * 2      # ... and so does one of 2 bytes (e = 2)
    assert dr.chunk_tokens(b"\x01\x02" * 3, 2) == [("lit", 1), ("lit", 2), ("match", 4)]
    assert dr.chunk_tokens(b"\x01\x02\x03\x04" * 2, 4) == [("lit", 1), ("lit", 2), ("lit", 3), ("lit", 4), ("match", 4)]
    # segments of 256 bytes: the first holds the literal and a match of 255, the second starts with a match of its own
    assert dr.chunk_tokens(b"\x05" * 600, 1) == [("lit", 5), ("match", 255), ("match", 256), ("match", 88)]


def test_voronoi_maps_take_a_quarter_at_most():
    """A condition on the rule, not a measurement: label and type maps of SURVEY's cell density shrink to a quarter or less."""
    for name in ("voronoi_labels", "voronoi_types"):
        _, data, _ = dc.BY_NAME[name]
        assert 4 * len(dc.restated(name)) <= len(data), (name, len(dc.restated(name)), len(data))


def test_worst_case_fills_the_bound():
    _, data, _ = dc.BY_NAME["worst_e1"]
    assert len(dc.restated("worst_e1")) == dr.bound(len(data))


def test_bound_entry_needs_no_device():
    from tissue_image_processing_amd import _deflate
    for n in (0, 1, 65535, 65536, 65537, 2048 * 2048 * 4):
        assert _deflate.runs_bound(n) == dr.bound(n)


@pytest.mark.parametrize("split", [0, 1, 65536, 77777, 199999, 200000])
def test_crc_combine(split):
    from tissue_image_processing_amd._deflate import crc32_combine
    buf = np.random.default_rng(3).integers(0, 256, 200000, dtype=np.uint8).tobytes()
    assert crc32_combine(zlib.crc32(buf[:split]), zlib.crc32(buf[split:]), len(buf) - split) == zlib.crc32(buf)


def test_crc_combine_of_many_parts():
    from tissue_image_processing_amd._deflate import crc32_combine
    buf = np.random.default_rng(4).integers(0, 256, 5000, dtype=np.uint8).tobytes()
    crc, cuts = 0, [0, 1, 2, 258, 1000, 1000, 4999, 5000]
    for a, b in zip(cuts[:-1], cuts[1:]):
        crc = crc32_combine(crc, zlib.crc32(buf[a:b]), b - a)
    assert crc == zlib.crc32(buf)


def _npy_member(array, e):
    from tissue_image_processing_amd._deflate import npy_header, npy_member
    data = array.tobytes()
    return npy_member(npy_header(array.shape, array.dtype), dr.deflate_runs(data, e), zlib.crc32(data), len(data))


def test_npy_member_is_np_save():
    labels, types = dc.voronoi_pair()
    for array, e in ((labels, 4), (types, 1), (np.zeros((0, 7), np.int32), 4)):
        raw, crc, size = _npy_member(array, e)
        buf = io.BytesIO()
        np.save(buf, array)
        d = zlib.decompressobj(-15)
        assert d.decompress(raw) + d.flush() == buf.getvalue() and d.eof
        assert crc == zlib.crc32(buf.getvalue()) and size == len(buf.getvalue())


def _kept_from_labels(labels):
    """what the movie driver keeps of a frame, worked out on the host (perimeter counts and pairs made up)"""
    n = int(labels.max())
    yy, xx = np.mgrid[0:labels.shape[0], 0:labels.shape[1]]
    area = np.bincount(labels.ravel(), minlength=n + 1)[1:].astype(np.int64)
    sumy = np.bincount(labels.ravel(), yy.ravel(), minlength=n + 1)[1:].astype(np.int64)
    sumx = np.bincount(labels.ravel(), xx.ravel(), minlength=n + 1)[1:].astype(np.int64)
    bbox = np.array([[yy[labels == k].min(), xx[labels == k].min(), yy[labels == k].max() + 1, xx[labels == k].max() + 1]
                     if area[k - 1] else [0, 0, 0, 0] for k in range(1, n + 1)], np.int64)
    pc = np.stack([area // 3, area // 5, area // 7], axis=1)
    pairs = np.array([[k + 1, k] for k in range(1, n)][::-1], np.int32)
    return dict(area=area, sumy=sumy, sumx=sumx, bbox=bbox, pc=pc, pairs=pairs)


def test_raw_zip_writer_and_tissue_load(tmp_path):
    import pandas as pd
    from tissue_image_processing_amd import seg_archive
    from tissue_image_processing_amd.tissue_info import Tissue
    labels, types = dc.voronoi_pair()
    kept = _kept_from_labels(labels)
    n = kept["area"].size
    kept.update(type=(np.arange(n) % 3 == 2).astype(np.uint8), valid=np.ones(n, np.uint8), mean_intensity=np.linspace(0.5, 2.0, n))
    table = seg_archive.frame_table(kept, np.arange(n) + 100, type_name="HC")
    assert [int(v) for v in table["label"]] == list(range(100, 100 + n)) and table["neighbors"][1] == {1, 3}
    buf = io.BytesIO()
    table.to_pickle(buf, compression=None)
    drifts = np.array([[0.0, 0.0], [1.5, -2.0]])
    members = [("frame_1_labels.npy",) + _npy_member(labels, 4), ("frame_1_types.npy",) + _npy_member(types, 1),
               ("frame_1_data.pkl",) + seg_archive.deflate_small(buf.getvalue()),
               ("frame_2_labels.npy",) + _npy_member(labels[::-1].copy(), 4)]
    buf = io.BytesIO()
    np.save(buf, drifts)
    members.append(("drifts.npy",) + seg_archive.deflate_small(buf.getvalue()))
    path = seg_archive.write_raw_zip(str(tmp_path / "movie.seg"), members)
    with zipfile.ZipFile(path) as z:
        assert z.testzip() is None
        assert z.namelist() == [m[0] for m in members]
        assert all(i.compress_type == zipfile.ZIP_DEFLATED for i in z.infolist())
        assert np.array_equal(np.load(io.BytesIO(z.read("frame_1_labels.npy"))), labels)
        assert np.array_equal(np.load(io.BytesIO(z.read("frame_1_types.npy"))), types)
        pd.testing.assert_frame_equal(pd.read_pickle(io.BytesIO(z.read("frame_1_data.pkl")), compression=None), table)
    tissue = Tissue(2)
    for _ in tissue.load(path):
        pass
    assert np.array_equal(tissue.get_labels(1), labels) and tissue.get_labels(1).dtype == np.int32
    assert np.array_equal(tissue.get_labels(2), labels[::-1])
    assert np.array_equal(tissue.get_cell_types(1), types) and tissue.get_cell_types(2) is None
    pd.testing.assert_frame_equal(tissue.get_cells_info(1), table)
    assert np.array_equal(tissue.drifts, drifts)


def test_frame_table_without_types_has_no_type_columns():
    from tissue_image_processing_amd import seg_archive
    from tissue_image_processing_amd.tissue_info import CELL_INFO_SPECS
    labels, _ = dc.voronoi_pair()
    kept = _kept_from_labels(labels)
    table = seg_archive.frame_table(kept, np.arange(kept["area"].size) + 1)
    assert list(table.columns) == list(CELL_INFO_SPECS)
    assert seg_archive.frame_table(dict(kept, area=np.zeros(0, np.int64)), np.zeros(0)) is None


def test_zip64_is_refused_before_anything_is_written(tmp_path):
    from tissue_image_processing_amd import seg_archive
    path = str(tmp_path / "big.seg")
    with pytest.raises(ValueError, match="zip64"):
        seg_archive.write_raw_zip(path, [("small", b"\x03\x00", 0, 0), ("huge.npy", b"\x03\x00", 0, 0xFFFFFFFF)])
    assert not os.path.exists(path)
    with pytest.raises(ValueError, match="65535"):
        seg_archive.write_raw_zip(path, [("m%d" % i, b"\x03\x00", 0, 0) for i in range(0xFFFF)])
    assert not os.path.exists(path)
