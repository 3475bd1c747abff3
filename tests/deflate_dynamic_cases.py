"""The inputs the dynamic-code deflate encoder is tested on, shared by the restatement's CPU test and the device test: CASES maps a
name to (bytes, elem_bytes, row_bytes or None); restated(name) and info(name) cache deflate_dynamic_restate's stream and
chunk_info of a case.  The maps are those of the rows rule's device test; the others are named in the tests."""
import numpy as np

import deflate_cases as dc
import deflate_dynamic_restate as dd


def _maps():
    labels, types = dc.voronoi_pair()
    big_l, big_t = np.tile(labels, (6, 3)).astype(np.int32), np.tile(types, (6, 3))
    out = {
        "voronoi_labels": (labels.tobytes(), 4, 512),                  # one partial chunk
        "voronoi_types": (types.tobytes(), 1, 128),
        "tiled_labels": (big_l.tobytes(), 4, 1536),                    # 13.5 chunks; the row above lies in the chunk before
        "tiled_u16": (big_l.astype(np.uint16).tobytes(), 2, 768),      # 6.75 chunks
        "tiled_types": (big_t.tobytes(), 1, 384),                      # 3.4 chunks
        "crop_40x2048": (np.tile(labels, (1, 16))[:40].copy().tobytes(), 4, 8192),      # a row is 32 segments, as in production
        "width_37_u8": (big_t[:, :37].copy().tobytes(), 1, 37),        # odd distances 37, 38, 36
        "width_2_i32": (big_l[:, :2].copy().tobytes(), 4, 8),          # P - e = e is dropped
    }
    for e, array in ((4, big_l), (1, big_t)):
        for row_bytes in (32768, 32768 + e, 32768 + 2 * e):            # three candidates' limit: P and P - e, P - e alone, none
            out["far_%d_e%d" % (row_bytes, e)] = (array.tobytes(), e, row_bytes)
    for name in dc.NAMES:
        if name.startswith("edge_") or name == "worst_e1":
            _, data, e = dc.BY_NAME[name]
            out[name] = (data, e, 256)
    return out


def _limit15(values=range(130, 147)):
    """One chunk (e = 1, run-only rule) whose 17 byte values occur 1, 2, 3, 5, 8, ... times: with the end of block's 1 the
    weights are Fibonacci's, Huffman's tree over them is a chain and its deepest leaves lie at 17 -- ordered so that no two
    neighbours are equal (all literals): the values by falling count onto the even places, then onto the odd ones; the commonest
    fills less than half."""
    counts, a, b = [], 1, 2
    for _ in values:
        counts.append(a)
        a, b = b, a + b
    flat = [v for c, v in sorted(zip(counts, values), reverse=True) for _ in range(c)]
    out = np.zeros(len(flat), np.uint8)
    half = (len(flat) + 1) // 2
    out[0::2], out[1::2] = flat[:half], flat[half:]
    assert 2 * max(counts) <= len(flat) and not (out[1:] == out[:-1]).any() and len(flat) <= dd.dr.CHUNK
    return out.tobytes()


def _build():
    rng = np.random.default_rng(23)
    labels, _ = dc.voronoi_pair()
    out = _maps()
    out["all_equal"] = (np.full(5000, 0x01020304, np.int32).tobytes(), 4, 400)       # a single distance symbol
    out["noise"] = (rng.integers(0, 256, 70000, dtype=np.uint8).tobytes(), 1, 700)   # no distance symbol; two dynamic chunks
    out["tiny"] = (bytes(8), 4, None)                                                # the fixed form wins
    out["mixed"] = (np.tile(labels, (2, 1)).astype(np.int32).tobytes()[:dd.dr.CHUNK] + bytes(8), 4, 512)      # dynamic, then fixed
    out["limit15"] = (_limit15(), 1, None)
    return out


CASES = _build()
EMPTY = {"empty_e%d" % e: (b"", e, 64) for e in (1, 2, 4)}
_cache = {}


def _both(name):
    if name not in _cache:
        _cache[name] = dd._encode(*CASES[name])
    return _cache[name]


def restated(name):
    return _both(name)[0]


def info(name):
    return _both(name)[1]
