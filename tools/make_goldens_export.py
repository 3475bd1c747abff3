#!/opt/conda/bin/python3.9
"""Goldens for the TIFF exports: what the REFERENCE's `export_segmentation_and_cell_types_to_tiff` and `export_segmentation_to_tiff`
(ti.py:4040-4062) hand to `save_tiff`, on a small typed and tracked tissue.

    /opt/conda/bin/python3.9 tools/make_goldens_export.py     -> tests/golden/export_tiff.npz

The tissue: 4 frames of 56 x 72 Voronoi label maps (zero lines), a cell table per frame from the reference's own
`calculate_frame_cellinfo`, track ids that differ from row order (a seeded permutation plus 1000 per frame), a type map per frame
(1 on every third row, 0 on the others, 255 on invalid rows and lines) and frame 3 marked invalid.  `save_tiff` is replaced by a
recorder: the golden pins the arrays, axes and data type of the two calls, next to the inputs.  Only data is written.

At golden time this interpreter's tifffile also reads the files this repository's write_tiff_strips writes (classic and BigTIFF)
from strips made by zlib; the outcome is printed, not stored."""
import os
import sys
import tempfile
import types
import warnings
import zlib

warnings.filterwarnings("ignore")
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
REF = "/root/reference"
OUT = os.path.join(REPO, "tests", "golden")
sys.path.insert(0, REPO)


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m
    return m


_stub("aicsimageio", AICSImage=object)
_stub("aicsimageio.readers", czi_reader=None, bioformats_reader=None)
_stub("aicsimageio.writers", ome_tiff_writer=None)
_stub("trackpy")
sys.path.insert(0, os.path.join(REF, "tissue_analyzing_tool"))

import numpy as np  # noqa: E402
import tissue_info as ti  # noqa: E402  (reference)

if not hasattr(np, "bool"):          # ti.py:155 uses the alias numpy 1.24 removed
    np.bool = bool

T, NY, NX, INVALID_FRAME = 4, 56, 72, 3


def voronoi_labels(seed):
    rng = np.random.default_rng(seed)
    n = 14
    sy, sx = rng.uniform(0, NY, n), rng.uniform(0, NX, n)
    yy, xx = np.mgrid[0:NY, 0:NX]
    cell = np.argmin((yy[..., None] - sy) ** 2 + (xx[..., None] - sx) ** 2, axis=-1) + 1
    line = np.zeros((NY, NX), bool)
    line[:, :-1] |= cell[:, :-1] != cell[:, 1:]
    line[:-1, :] |= cell[:-1, :] != cell[1:, :]
    return np.where(line, 0, cell).astype(np.int32)


RECORDED = []


def recorder(path, image, metadata=None, axes="", data_type=""):
    RECORDED.append(dict(name=os.path.basename(path), image=np.array(image), axes=axes, data_type=data_type))


def main():
    tmp = tempfile.mkdtemp(prefix="tipgold_export_")
    t = ti.Tissue(T, os.path.join(tmp, "movie"), ["zo", "atoh"], load_to_memory=True)
    out = {}
    labs = [voronoi_labels(40 + f) for f in range(T)]
    for f in range(T):
        t.labels_list[f] = labs[f].copy()
    for f in range(T):
        t.set_labels(f + 1, labs[f].copy(), reset_data=False)
        t.calculate_frame_cellinfo(f + 1)
        t.cell_info_list[f] = t.cells_info.copy()
    for f in range(T):          # (after every frame has its table: the tissue writes its current table back when it changes frame)
        lab, ci = labs[f], t.get_cells_info(f + 1)
        n = ci.shape[0]
        ids = np.random.default_rng(7 + f).permutation(n).astype(np.int64) + 1 + 1000 * f
        ci["label"] = ids
        typ = (np.arange(n) % 3 == 0).astype(np.uint8)
        ci["type"] = typ
        t.cell_info_list[f] = ci
        lut = np.concatenate([[ti.INVALID_TYPE_INDEX], np.where(ci.valid.to_numpy() == 1, typ, ti.INVALID_TYPE_INDEX)]).astype(np.uint8)
        cell_types = lut[np.clip(lab, 0, n)]
        t.set_cell_types(f + 1, cell_types)
        out["labels_%d" % f] = lab
        out["ids_%d" % f] = ids
        out["cell_types_%d" % f] = cell_types
        assert (ids != np.arange(1, n + 1)).any() and (cell_types == 0).any() and (cell_types == 1).any() and (cell_types == 255).any()
    t.type_names = ["HC"]
    t.valid_frames[INVALID_FRAME - 1] = 0
    out["valid_frames"] = np.asarray(t.valid_frames, dtype=np.int64)
    ti.save_tiff = recorder
    assert t.export_segmentation_and_cell_types_to_tiff(tmp, "both") == 0
    assert t.export_segmentation_to_tiff(tmp, "labels") == 0
    both, labels = RECORDED
    assert (both["name"], both["axes"], both["data_type"]) == ("both.tif", "TCZYX", "uint16")
    assert (labels["name"], labels["axes"], labels["data_type"]) == ("labels.tif", "TCZYX", "uint16")
    assert both["image"].shape == (T, 2, 1, NY, NX) and labels["image"].shape == (T, 1, 1, NY, NX)
    assert not both["image"][INVALID_FRAME - 1].any() and not labels["image"][INVALID_FRAME - 1].any()
    for f in range(T):          # the tissue really held the inputs stored here
        if f != INVALID_FRAME - 1:
            assert np.array_equal(both["image"][f, 0, 0], np.insert(out["ids_%d" % f], 0, 0)[out["labels_%d" % f]].astype(np.uint16))
            assert np.array_equal(labels["image"][f, 0, 0], out["labels_%d" % f].astype(np.uint16))
            assert set(np.unique(both["image"][f, 1, 0])) == {0, 1, 2}
    out["export_both"], out["export_labels"] = both["image"], labels["image"]
    out["axes"] = np.array(both["axes"])
    np.savez_compressed(os.path.join(OUT, "export_tiff.npz"), **out)
    print("wrote export_tiff.npz", both["image"].shape, both["image"].dtype, labels["image"].shape)

    # ---- this interpreter's tifffile on a file of write_tiff_strips ------------------------------------------------------------
    import tifffile
    from tissue_image_processing_amd.tiff import write_tiff_strips
    planes = both["image"].reshape(-1, NY, NX)
    rps = 9
    pages = [[zlib.compress(p[r:r + rps].tobytes(), 6) for r in range(0, NY, rps)] for p in planes]
    for big in (False, True):
        path = os.path.join(tmp, "strips_big%d.tif" % big)
        write_tiff_strips(path, both["image"].shape, "TCZYX", np.uint16, rps, pages, bigtiff=big)
        with tifffile.TiffFile(path) as tf:
            got = tf.asarray()
            ok = got.reshape(both["image"].shape).dtype == np.uint16 and np.array_equal(got.reshape(both["image"].shape), both["image"])
            print("tifffile %s reads write_tiff_strips (bigtiff=%s, is_bigtiff=%s, %d pages): %s"
                  % (tifffile.__version__, big, tf.is_bigtiff, len(tf.pages), "equal" if ok else "DIFFERENT"))


if __name__ == "__main__":
    main()
