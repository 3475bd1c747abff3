"""CPU: the row form of event detection -- the numpy restatement of the event kernels (tests/events_restate.py) plus rank 0's
assembly (events.events_table) -- equals the reference's find_events_iterator on the golden movies and on their mutated copies, the
cases cover what the kernels can get wrong, movie.find_events gives one table at every world size, the header and the library
carry the new entries, and save_seg without events writes the archive it always wrote."""
import ctypes
import io
import pickle
import warnings
import zipfile
import zlib

import numpy as np
import pandas as pd
import pytest

import events_cases as ec
import events_restate as er
from gloo_launch import run_ranks

NEW_SYMBOLS = ["tip_border_rows_i32", "tip_border_rows_i32_dev", "tip_lookup_i32_dev", "tip_event_flags_i32", "tip_event_flags_i32_dev"]


@pytest.fixture(scope="module")
def compared():
    """every case once: {tag: (movie, the oracle's add_event calls, its table, the row form's calls, its table, its flags)}"""
    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for tag, movie in ec.all_cases():
            seen, table = ec.oracle(movie)
            calls = []
            got, flags = ec.row_form(movie, er, calls)
            out[tag] = (movie, seen, table, calls, got, flags)
    return out


@pytest.mark.parametrize("name", ec.MOVIES)
def test_restatement_gives_the_references_goldens(compared, name):
    """found_type / found_rows are the add_event calls of the reference's own run, table_* the table its add_event built."""
    g = ec.golden(name)
    _, _, _, calls, got, _ = compared[name]
    assert [c[0] for c in calls] == [str(v) for v in g["found_type"]]
    assert [list(c[1:]) for c in calls] == g["found_rows"].tolist()
    assert [str(v) for v in got["type"]] == [str(v) for v in g["table_type"]]
    assert [str(v) for v in got["source"]] == [str(v) for v in g["table_source"]]
    for k in ec.TABLE_COLUMNS:
        np.testing.assert_array_equal(np.asarray(got[k].to_numpy(), np.float64), g["table_" + k], err_msg=k)
    kinds = [c[0] for c in calls]
    assert (kinds.count("delamination"), kinds.count("differentiation"), kinds.count("division")) == ((5, 1, 0) if name == "overlays" else (0, 0, 1))


def test_restatement_equals_the_reference_on_every_mutated_case(compared):
    assert len(compared) - len(ec.MOVIES) >= 20
    for tag, (_, seen, table, calls, got, _) in compared.items():
        assert calls == seen, tag
        ec.assert_same_table(got, table)


def test_the_cases_cover_the_rules(compared):
    """Counted on the ORACLE's events: every kind at least three times, a division over a watershed line (label 0 under both
    centroids) and a division with two matching neighbours -- the latter two re-derived from the maps and tables, not from the
    flags under test."""
    kinds = [s[0] for _, seen, _, _, _, _ in compared.values() for s in seen]
    for kind in ("delamination", "differentiation", "division"):
        assert kinds.count(kind) >= 3, kind
    over_line = two_matches = 0
    for movie, seen, _, _, _, _ in compared.values():
        daughters = set(s[4] for s in seen if s[0] == "division")
        for t in range(1, ec.n_frames(movie)):
            prev, cur, _ = ec.pair_inputs(movie, t, er)
            before = set(prev["id"][prev["sel"] != 0].tolist())
            now = set(cur["id"][cur["sel"] != 0].tolist())
            edge_ids = set(cur["id"][cur["edge"] != 0].tolist())
            for r in np.flatnonzero(cur["sel"]):
                if int(cur["id"][r]) not in daughters or int(cur["id"][r]) in before:
                    continue
                over_line += int(cur["under"][r] == 0)
                named = [n for n in movie["tables"][t]["neighbors"][r] if n < cur["id"].size]
                same = [n for n in named if cur["under"][n] == cur["under"][r] and cur["under"][n] != -1 and int(cur["id"][n]) in before
                        and int(cur["id"][n]) in now and int(cur["id"][n]) not in edge_ids]
                two_matches += int(len(same) >= 2)
    assert over_line >= 1 and two_matches >= 1


def test_restated_border_and_lookup():
    lab = np.zeros((5, 7), np.int32)
    lab[0, 6], lab[2, 3], lab[4, 0], lab[1:4, 1] = 3, 2, 9, 1
    np.testing.assert_array_equal(er.border_rows(lab, 4), [0, 0, 1, 0])          # label 9 is above n: no part
    for movie in (ec.load_movie(n) for n in ec.MOVIES):
        for lab in movie["labels"]:
            n = int(lab.max())
            want = np.zeros(n, np.uint8)
            want[ec.ti.Tissue.detect_edge_cells(lab)] = 1
            np.testing.assert_array_equal(er.border_rows(lab, n), want)
    np.testing.assert_array_equal(er.lookup_exact(lab, [0, -1, 0, lab.shape[0]], [0, 0, lab.shape[1], 0]), [lab[0, 0], -1, -1, -1])


def test_duplicate_ids_and_bad_drifts_are_refused():
    from _movie_events_worker import EventsBackend, driver_inputs
    from tissue_image_processing_amd import movie as mv
    movie = ec.first_frames(ec.load_movie("overlays_small"), 3)
    tables, ids = driver_inputs(movie)
    backend = EventsBackend(movie, 0, 1)
    rows = np.flatnonzero(ec.frame_rows(movie, 1)["sel"])
    twice = [i.copy() for i in ids]
    twice[1][rows[1]] = twice[1][rows[0]]
    with pytest.raises(ValueError, match="two valid"):
        mv.find_events(3, backend, tables, twice)
    with pytest.raises(ValueError, match="not finite"):
        mv.find_events(3, backend, tables, ids, drifts=np.array([[0, 0], [np.nan, 0], [0, 0]]))
    with pytest.raises(ValueError, match="no table"):
        mv.find_events(3, backend, [tables[0], dict(tables[1], cy=np.zeros(0), cx=np.zeros(0), area=np.zeros(0)), tables[2]],
                       [ids[0], np.zeros(0, np.int64), ids[2]])
    with pytest.raises(ValueError, match="differ in length"):
        mv.find_events(3, backend, tables, [ids[0], ids[1][:-1], ids[2]])
    backend.archive = None
    with pytest.raises(ValueError, match="archive"):
        mv.find_events(3, backend, tables, ids)


def test_header_and_library_carry_the_new_entries():
    import test_abi
    from tissue_image_processing_amd import _abi, _lib
    declared = test_abi.declared_symbols()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for sym in NEW_SYMBOLS:
        assert sym in declared and sym in _abi.SIGNATURES and hasattr(lib, sym), sym


@pytest.fixture(scope="module")
def by_world(tmp_path_factory):
    out = {}
    for world in (1, 2, 3):
        path = tmp_path_factory.mktemp("events") / ("world%d.pkl" % world)
        run_ranks("_movie_events_worker.py", world, (path,), timeout=300)
        with open(path, "rb") as fh:
            out[world] = pickle.load(fh)
    return out


@pytest.mark.parametrize("frames", (5, 2))
@pytest.mark.parametrize("name", ec.MOVIES)
def test_find_events_gives_one_table_at_every_world_size(by_world, name, frames):
    """gloo, the restatement behind the backend's methods; 2 frames on 3 ranks: fewer frames than ranks"""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, want = ec.oracle(ec.first_frames(ec.load_movie(name), frames))
    for world in (1, 2, 3):
        got = by_world[world][(name, frames)]
        ec.assert_same_table(got, want)
        pd.testing.assert_frame_equal(got, by_world[1][(name, frames)])
    if frames == 5:
        assert len(want) == len(ec.golden(name)["table_type"])


# ---- save_seg --------------------------------------------------------------------------------------------------------------------
class _ArchivedBackend(object):
    """what save_seg reads of a backend: the kept parts of every frame (maps deflated by zlib here) and the frame extents"""

    def __init__(self, movie):
        from oracle import oracle as orc
        self.archive, self.cell_types = dict(type_name="HC", matches="runs"), None
        self.Y, self.X = movie["labels"][0].shape
        self.archive_frames = {}
        for t, lab in enumerate(movie["labels"]):
            lab = np.ascontiguousarray(lab, np.int32)
            rp = orc.regionprops(lab)
            n = rp["area"].size
            co = zlib.compressobj(6, zlib.DEFLATED, -15)
            stream = co.compress(lab.tobytes()) + co.flush(zlib.Z_SYNC_FLUSH)          # byte-aligned, not final
            self.archive_frames[t] = dict(labels=(stream, zlib.crc32(lab.tobytes())), types=None, area=rp["area"].astype(np.int64),
                                          bbox=np.zeros((n, 4), np.int64), sumy=np.zeros(n, np.int64), sumx=np.zeros(n, np.int64),
                                          pc=np.zeros((n, 3), np.int64), pairs=np.zeros((0, 2), np.int64))


def test_save_seg_without_events_is_the_archive_it_was(tmp_path):
    from _movie_events_worker import driver_inputs
    from tissue_image_processing_amd import movie as mv
    from tissue_image_processing_amd import tissue_info as ti
    movie = ec.first_frames(ec.load_movie("overlays_small"), 3)
    tables, _ = driver_inputs(movie)
    ids = [np.arange(1, int(lab.max()) + 1) for lab in movie["labels"]]
    backend = _ArchivedBackend(movie)
    plain = mv.save_seg(str(tmp_path / "plain"), 3, backend, tables, ids)
    none = mv.save_seg(str(tmp_path / "none"), 3, backend, tables, ids, events=None)
    assert open(plain, "rb").read() == open(none, "rb").read()
    with zipfile.ZipFile(plain) as z:          # ... and that is the empty table the archive has always held
        buf = io.BytesIO()
        ti.make_df(0, ti.EVENTS_INFO_SPEC).to_pickle(buf, compression=None)
        assert z.read("events_data.pkl") == buf.getvalue()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, table = ec.oracle(ec.load_movie("overlays_small"))
    assert len(table) == 1
    full = mv.save_seg(str(tmp_path / "full"), 3, backend, tables, ids, events=table)
    with zipfile.ZipFile(plain) as a, zipfile.ZipFile(full) as b:
        assert a.namelist() == b.namelist()
        for name in a.namelist():
            if name != "events_data.pkl":
                assert a.read(name) == b.read(name), name
        pd.testing.assert_frame_equal(pd.read_pickle(io.BytesIO(b.read("events_data.pkl")), compression=None), table)
    loaded = ti.Tissue(3)
    for _ in loaded.load(full):
        pass
    ec.assert_same_table(loaded.events, table)
