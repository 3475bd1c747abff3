"""CPU: the "rows" deflate rule as restated in tests/deflate_rows_restate.py -- zlib inflates every case at every row length
to its input, within the run-only bound; without a candidate distance it is the run-only stream; the sizes on the Voronoi maps."""
import numpy as np
import pytest

import deflate_cases as dc
import deflate_restate as dr
import deflate_rows_restate as rr


def _row_lengths(e):
    return [p for p in (e, 2 * e, 3 * e, 37 * e, 256, 1536, 32768 - e, 32768, 32768 + e) if p % e == 0]


@pytest.mark.parametrize("name", dc.NAMES)
def test_restated_rows_stream_inflates_to_the_input(name):
    _, data, e = dc.BY_NAME[name]
    for row_bytes in _row_lengths(e):
        stream = rr.deflate_rows(data, e, row_bytes)
        assert dr.inflate(stream) == data, (name, row_bytes)
        assert len(stream) <= dr.bound(len(data)), (name, row_bytes, len(stream))


@pytest.mark.parametrize("name", dc.NAMES)
def test_without_a_candidate_it_is_the_run_only_stream(name):
    _, data, e = dc.BY_NAME[name]
    assert rr.candidates(e, 32768 + 2 * e) == []
    assert rr.deflate_rows(data, e, 32768 + 2 * e) == dc.restated(name)


def test_distance_code():
    """RFC 1951 3.2.5 at its edges: code 25 holds 6145 .. 8192 with 11 extra bits, code 29 ends at 32768 with 13."""
    assert rr.distance_bits(1) == (0, 5) and rr.distance_bits(4) == (dr._rev(3, 5), 5)
    assert rr.distance_bits(5) == (dr._rev(4, 5), 6) and rr.distance_bits(6) == (dr._rev(4, 5) | 1 << 5, 6)
    assert rr.distance_bits(8192) == (dr._rev(25, 5) | (8192 - 6145) << 5, 5 + 11)
    assert rr.distance_bits(8193) == (dr._rev(26, 5), 5 + 12)
    assert rr.distance_bits(32768) == (dr._rev(29, 5) | 8191 << 5, 5 + 13)
    assert rr.match_bits(258, 32768)[1] == 8 + 5 + 13 and rr.match_bits(131, 32768)[1] == 31


def test_rule_on_small_inputs():
    """The rule's thresholds and its tie, token by token (rows of 8 bytes)."""
    row = bytes(range(1, 9))
    assert rr.chunk_tokens(row * 2, 0, 1, 8) == [("lit", b) for b in row] + [("match", 8, 8)]
    # a row match of 3 bytes is too short (e = 1): literals; one of 4 is taken
    assert rr.chunk_tokens(row + b"\x01\x02\x03\x63", 0, 1, 8)[8:] == [("lit", 1), ("lit", 2), ("lit", 3), ("lit", 0x63)]
    assert rr.chunk_tokens(row + b"\x01\x02\x03\x04\x63", 0, 1, 8)[8:] == [("match", 4, 8), ("lit", 0x63)]
    # the row above shifted by one element either way: distances P + e and P - e
    assert rr.chunk_tokens(row + b"\x63" + row[:6], 0, 1, 8)[8:] == [("lit", 0x63), ("match", 6, 9)]
    assert rr.chunk_tokens(row + row[1:6], 0, 1, 8)[8:] == [("match", 5, 7)]
    # a constant map stays a run: no row match is LONGER than it
    assert rr.chunk_tokens(b"\x05" * 24, 0, 1, 8) == [("lit", 5), ("match", 23, 1)]
    # all three candidates match 5 bytes behind the 6 (the run starts one later): the tie goes to P
    assert rr.chunk_tokens(b"\x09" + b"\x05" * 8 + b"\x06" + b"\x05" * 5, 0, 1, 8)[3:] == [("lit", 6), ("match", 5, 8)]
    # a run longer than the row match is taken
    assert rr.chunk_tokens(row + b"\x01\x02\x03\x04\x04\x04\x04\x04\x04", 0, 1, 8)[8:] == [("match", 4, 8), ("match", 5, 1)]
    # int32: P - e = e is dropped for a two-element row, P + e = 12 is kept
    assert rr.candidates(4, 8) == [8, 12] and rr.candidates(4, 4) == [8] and rr.candidates(1, 32768) == [32768, 32767]


def test_a_match_reaches_into_the_chunk_before_but_not_before_the_buffer():
    labels, _ = dc.voronoi_pair()
    data = np.tile(labels, (6, 3)).astype(np.int32).tobytes()
    first = rr.chunk_tokens(data, 0, 4, 1536)
    assert all(t[0] == "lit" or t[2] == 4 for t in first[:first.index(next(t for t in first if t[0] == "match" and t[2] != 4))])
    pos = 0
    for t in first:                                    # no row match before a whole distance of input lies behind it
        assert t[0] == "lit" or t[2] <= pos, (t, pos)
        pos += 1 if t[0] == "lit" else t[1]
    second = rr.chunk_tokens(data, dr.CHUNK, 4, 1536)
    pos = 0
    reached_back = False
    for t in second:
        reached_back |= t[0] == "match" and t[2] > pos
        pos += 1 if t[0] == "lit" else t[1]
    assert reached_back


def test_sizes_on_the_voronoi_maps():
    """The rule's sizes at row_bytes = width * e, pinned; every one is below the run-only stream's."""
    labels, types = dc.voronoi_pair()
    big_l, big_t = np.tile(labels, (6, 3)).astype(np.int32), np.tile(types, (6, 3))
    for array, e, want in ((labels, 4, 1812), (types, 1, 1113), (big_l, 4, 34392), (big_l.astype(np.uint16), 2, 28140),
                           (big_t, 1, 21094)):
        data = array.tobytes()
        rows, runs = rr.deflate_rows(data, e, array.shape[1] * e), dr.deflate_runs(data, e)
        assert dr.inflate(rows) == data
        assert len(rows) == want, (array.shape, e, len(rows), want)
        assert len(rows) < len(runs), (array.shape, e, len(rows), len(runs))
