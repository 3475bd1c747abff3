"""CPU: the spatial-tiling driver of config 5 (tiling.py) with the gloo process group and an oracle-backed stand-in:
tiles + halo + a summed percentile histogram reproduce the untiled frame exactly, on 1 and on 2 ranks."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from gloo_launch import run_ranks  # noqa: E402


def _run(world, out):
    run_ranks("_tile_worker.py", world, (out,), timeout=600)


def test_tile_boxes_cover_the_plane_once():
    from tissue_image_processing_amd import tiling
    for (Y, X, ny, nx) in [(4096, 4096, 2, 4), (420, 500, 2, 2), (97, 1031, 1, 3), (50, 60, 3, 3)]:
        cover = np.zeros((Y, X), np.int32)
        for (y0, y1, x0, x1), (py0, py1, px0, px1) in tiling.tile_boxes(Y, X, ny, nx):
            cover[y0:y1, x0:x1] += 1
            assert py0 == max(0, y0 - tiling.HALO) and py1 == min(Y, y1 + tiling.HALO)
            assert px0 == max(0, x0 - tiling.HALO) and px1 == min(X, x1 + tiling.HALO)
        assert (cover == 1).all()


def test_tiled_frame_equals_untiled_on_1_and_2_ranks(tmp_path):
    from _tile_worker import test_stack
    from oracle import oracle as orc
    st = test_stack()
    proj, zmap = orc.time_point_surface_projection(st, "CZYX", 0, airyscan=False, z_map=True)
    labels = orc.watershed_segmentation(proj[0], 0.03, 3, 3)
    for world in (1, 2):
        out = str(tmp_path / ("w%d.npz" % world))
        _run(world, out)
        g = np.load(out)
        assert int((g["zmap"] != zmap).sum()) == 0
        np.testing.assert_array_equal(g["proj"], proj)
        np.testing.assert_array_equal(g["labels"], labels)
