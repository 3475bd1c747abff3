"""CPU: the numpy restatement of the neighbour-graph kernels (tests/graph_restate.py) equals every golden case the reference's own
methods produced (tests/golden/graph_features.npz), the goldens cover the situations the kernels can get wrong, and the header
and the library carry the new entries."""
import ctypes
import os

import numpy as np
import pytest

import graph_cases as gc
import graph_restate as gr

NEW_SYMBOLS = ["tip_neighbor_csr_i32", "tip_graph_counts_i32", "tip_graph_second_i32", "tip_contact_sums_i32", "tip_contact_pairs_i32"]


@pytest.mark.parametrize("tag", gc.FRAMES)
def test_restatement_equals_every_golden_case(tag):
    ran = 0
    for c in gc.cases(tag):
        got = gc.on_kernels(gr, c)
        if got is not None:
            gc.assert_same(got, gc.expected(c))
            ran += 1
    assert ran >= 22


@pytest.mark.parametrize("tag", gc.FRAMES)
def test_restated_csr_equals_the_reference_tables(tag):
    f = gc.frame(tag)
    pairs = gr.neighbor_pairs(f["labels"])
    off, adj = gr.neighbor_csr(pairs, f["n"], f["working"])          # calculate_frame_cellinfo: the valid rows work
    np.testing.assert_array_equal(off, f["offsets"])
    np.testing.assert_array_equal(adj, f["adj"])
    off, adj = gr.neighbor_csr(pairs, f["n"], None)                  # find_neighbors(only_for_labels=None)
    np.testing.assert_array_equal(off, f["all_offsets"])
    np.testing.assert_array_equal(adj, f["all_adj"])


def test_what_the_reference_raised():
    """the quirks DESIGN 5.8 records: which cases raise, and with what"""
    for c in gc.cases():
        if c["method"] == "nnt" and c["cell_type"] == "same":
            assert (c["status"], c["exc"]) == (2, "TypeError")
        elif c["method"] == "nnt" and (c["cell_type"] == "nope" or (c["second"] and c["cell_type"] in ("valid", "invalid"))):
            assert (c["status"], c["exc"]) == (2, "KeyError")
        else:
            assert c["status"] == 0, c
        if c["method"] == "nnt" and c["second"] and c["cell_type"] == "HC":
            assert not gc.expected(c).any()                          # the all-zero column
        if c["frame"] != "H":
            assert c["cells_kind"] == 0
    # the reference itself takes a row without neighbours in every case it does not raise on anyway
    assert all(c["cells_kind"] == 0 for c in gc.cases() if c["status"] == 0)


def test_golden_coverage():
    h = gc.frame("H")
    degree = np.diff(h["offsets"])
    hub = int(np.argmax(degree))
    assert degree[hub] > 64 and hub in h["cells"][0]                 # a row longer than a wavefront, and it is queried
    assert any(np.diff(gc.frame(t)["offsets"])[gc.frame(t)["cells"][0]].min() == 0 for t in gc.FRAMES)      # a queried degree-0 row
    for tag in gc.FRAMES:
        f = gc.frame(tag)
        assert (f["type"] == 255).any()
        rows = f["cells"][0]
        neighbours = [f["adj"][f["offsets"][r]:f["offsets"][r + 1]] - 1 for r in rows]
        assert any((f["valid"][nb] == 0).any() for nb in neighbours), "no invalid intermediate in " + tag
        assert any((f["empty"][nb] == 1).any() for nb in neighbours), "no empty_cell neighbour in " + tag
        assert 40 <= f["n"] <= 120


def test_header_and_library_carry_the_new_entries():
    import test_abi
    from tissue_image_processing_amd import _lib
    declared = test_abi.declared_symbols()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        for sym in (name, name + "_dev"):
            assert sym in declared and hasattr(lib, sym), sym


def test_mixin_has_upstreams_signatures():
    import inspect
    from tissue_image_processing_amd.tissue_info import TissueHipMixin as M
    want = {"calculate_n_neighbors_from_type": ["self", "frame", "cells", "cell_type", "positive_for_type", "second_neighbors"],
            "calculate_n_neighbors_by_type": ["self", "frame", "cells", "type_list"],
            "find_second_order_neighbors": ["self", "frame", "cells", "cell_type", "positive_for_type"],
            "calculate_contact_length": ["self", "frame", "cell_info", "max_filtered_labels", "min_filtered_labels", "cell_type",
                                         "positive_for_type"],
            "calculate_contact_lengths": ["self", "frame", "cells", "cell_type", "positive_for_type", "for_histogram"]}
    for name, args in want.items():
        assert list(inspect.signature(getattr(M, name)).parameters) == args
    assert os.path.exists(gc.GOLDEN)
