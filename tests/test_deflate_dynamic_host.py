"""CPU: the dynamic-code deflate stream as restated in tests/deflate_dynamic_restate.py -- zlib inflates every case to its input;
no chunk is longer than its fixed form, and is the fixed form's bytes where that was chosen; the codes are complete, at most 15
bits long and, where the limit did not bind, cost what an independent Huffman construction costs; the forms chosen and the
sizes on the Voronoi maps."""
import heapq
from fractions import Fraction

import pytest

import deflate_dynamic_cases as cases
import deflate_dynamic_restate as dd
import deflate_restate as dr
import deflate_rows_restate as rr

NAMES = list(cases.CASES)


def _fixed_stream(data, e, row_bytes):
    return dr.deflate_runs(data, e) if row_bytes is None else rr.deflate_rows(data, e, row_bytes)


def _fixed_chunks(data, e, row_bytes):
    """the fixed stream of every chunk: a chunk's tokens depend on the bytes before it, its bits do not"""
    if row_bytes is None:
        return [dr.encode_chunk(data[i:i + dr.CHUNK], e) for i in range(0, len(data), dr.CHUNK)]
    toks, starts = rr.tokens(data, e, row_bytes)
    return [rr.encode_tokens(toks[a:b]) for a, b in zip(starts[:-1], starts[1:])]


def _huffman_cost(counts):
    """sum of count * code length of an optimal prefix code, by the textbook heap: the sum of all merged weights"""
    heap = [c for c in counts if c > 0]
    heapq.heapify(heap)
    cost = 0
    while len(heap) > 1:
        w = heapq.heappop(heap) + heapq.heappop(heap)
        cost += w
        heapq.heappush(heap, w)
    return cost


def _kraft(lengths):
    return sum(Fraction(1, 1 << n) for n in lengths if n)


@pytest.mark.parametrize("name", NAMES)
def test_zlib_inflates_the_stream_to_the_input(name):
    data = cases.CASES[name][0]
    assert dr.inflate(cases.restated(name)) == data
    assert len(cases.restated(name)) <= dr.bound(len(data))


@pytest.mark.parametrize("name", list(cases.EMPTY))
def test_an_empty_input_is_an_empty_stream(name):
    assert dd.deflate_dynamic(*cases.EMPTY[name]) == b"" and dd.chunk_info(*cases.EMPTY[name]) == []


@pytest.mark.parametrize("name", NAMES)
def test_no_chunk_is_longer_than_its_fixed_form(name):
    data, e, row_bytes = cases.CASES[name]
    stream, at = cases.restated(name), 0
    fixed = _fixed_chunks(data, e, row_bytes)
    assert b"".join(fixed) == _fixed_stream(data, e, row_bytes) and len(fixed) == len(cases.info(name))
    for k, (chunk, want) in enumerate(zip(cases.info(name), fixed)):
        assert chunk["fixed_bytes"] == len(want) and chunk["size"] <= len(want), (name, k)
        assert chunk["form"] == ("dynamic" if chunk["dynamic_bytes"] < chunk["fixed_bytes"] else "fixed"), (name, k)
        assert chunk["size"] == chunk["dynamic_bytes" if chunk["form"] == "dynamic" else "fixed_bytes"], (name, k)
        if chunk["form"] == "fixed":
            assert stream[at:at + chunk["size"]] == want, (name, k)
        assert stream[at + chunk["size"] - 4:at + chunk["size"]] == dr.EMPTY_STORED, (name, k)
        at += chunk["size"]
    assert at == len(stream)


@pytest.mark.parametrize("name", NAMES)
def test_the_codes_are_complete_and_at_most_15_bits(name):
    for k, chunk in enumerate(cases.info(name)):
        for counts, lengths in ((chunk["lit_counts"], chunk["lit_lengths"]), (chunk["dist_counts"], chunk["dist_lengths"])):
            used = sum(c > 0 for c in counts)
            assert [n > 0 for n in lengths] == [c > 0 for c in counts], (name, k)
            assert max(lengths) <= 15, (name, k)
            if used >= 2:
                assert _kraft(lengths) == 1, (name, k)
            elif used == 1:
                assert sum(lengths) == 1, (name, k)                   # one symbol of length 1
        assert chunk["lit_counts"][256] == 1 and sum(c > 0 for c in chunk["lit_counts"]) >= 2
        assert sum(c > 0 for c in chunk["dist_counts"]) <= 4 and max(chunk["dist_lengths"]) <= 3


@pytest.mark.parametrize("name", NAMES)
def test_the_token_bits_are_an_independent_huffmans(name):
    for k, chunk in enumerate(cases.info(name)):
        for counts, lengths in ((chunk["lit_counts"], chunk["lit_lengths"]), (chunk["dist_counts"], chunk["dist_lengths"])):
            cost = sum(c * n for c, n in zip(counts, lengths))
            if sum(c > 0 for c in counts) == 1:
                assert cost == sum(counts)
            elif not chunk["limit_applied"] or len(counts) == 30:
                assert cost == _huffman_cost(counts), (name, k)
            else:
                assert cost > _huffman_cost(counts), (name, k)        # the limit costs bits, or it was not needed


def test_the_forms_chosen():
    assert [c["limit_applied"] for c in cases.info("limit15")] == [True]
    assert [c["form"] for c in cases.info("limit15")] == ["dynamic"] and max(cases.info("limit15")[0]["lit_lengths"]) == 15
    assert not any(c["limit_applied"] for name in NAMES if name != "limit15" for c in cases.info(name))
    assert [c["form"] for c in cases.info("tiny")] == ["fixed"]
    assert [c["form"] for c in cases.info("mixed")] == ["dynamic", "fixed"]
    assert [c["form"] for c in cases.info("noise")] == ["dynamic", "dynamic"]
    assert sum(cases.info("noise")[0]["dist_counts"]) == 0 and cases.info("noise")[0]["dist_lengths"] == [0] * 30
    assert [sum(c > 0 for c in chunk["dist_counts"]) for chunk in cases.info("all_equal")] == [1]
    assert cases.info("worst_e1")[0]["form"] == "dynamic"             # two literals of nine fixed bits each become one bit


def test_the_header_of_a_tiny_block():
    """8 zero bytes of int32: literals 0 x 4, one match (4, 4), end of block -- the block written out by hand."""
    info, = dd.chunk_info(bytes(8), 4)
    assert info["lit_lengths"][0] == 1 and info["lit_lengths"][256] == 2 and info["lit_lengths"][258] == 2
    assert info["dist_lengths"] == [0, 0, 0, 1] + [0] * 26
    # 3 + 5 + 5 + 4 + 57 header bits; lengths: 1, 255 zeros (18: 138, 18: 117), 2, 0, 2 | 0, 0, 0, 1: 4, 11, 11, 4, 4, 4, 17: 3 zeros 7, 4
    bits = 74 + 4 + 11 + 11 + 4 + 4 + 4 + 7 + 4 + 4 * 1 + (2 + 1) + 2
    assert info["dynamic_bytes"] == (bits + 3 + 7) // 8 + 4 == 21 and info["fixed_bytes"] == 12


def test_sizes_on_the_voronoi_maps():
    """The dynamic streams of the two Voronoi maps, pinned, strictly below their fixed streams (1812 and 1113 bytes)."""
    for name, fixed, want in (("voronoi_labels", 1812, 1206), ("voronoi_types", 1113, 707)):
        data, e, row_bytes = cases.CASES[name]
        assert len(rr.deflate_rows(data, e, row_bytes)) == fixed
        assert len(cases.restated(name)) == want < fixed, (name, len(cases.restated(name)))


