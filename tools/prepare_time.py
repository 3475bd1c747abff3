"""Device time (HIP events) of SegmentationPredictor.prepare_image on the bench frame's projection (GPU box).

The input is what FramePipeline.segment_unet hands over: the (atoh, zo) planes of the projection of
synthetic.make_stack(30, 2048, 2048, seed=100), each transposed.  Prints one JSON line per round: median and min..max over the
timed calls, and the ratio of the median to seven reads of the image at 4 TB/s (the stage's budget: five digit passes, one spare
and the normalise pass).  TISSUE_HIP_LIB selects another build of the library (the parent commit's, for the comparison).

    python tools/prepare_time.py [--rounds 3] [--calls 50] [--warmup 5] [--label NAME]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--size", type=int, nargs=3, default=[2048, 2048, 30], metavar=("Y", "X", "Z"))
    ap.add_argument("--label", default=os.environ.get("TISSUE_HIP_LIB") and "other build" or "this tree")
    args = ap.parse_args()
    import numpy as np
    import torch
    from tissue_image_processing_amd import _lib, synthetic
    from tissue_image_processing_amd.pipeline import FramePipeline
    from tissue_image_processing_amd.prediction_local import SegmentationPredictor
    if not torch.cuda.is_available():
        raise SystemExit("prepare_time.py needs the GPU")
    _lib.init(0)
    Y, X, Z = args.size
    pipe = FramePipeline(2, Z, Y, X, reference_channel=0, airyscan=False, use_torch=True)
    pred = SegmentationPredictor(None, (2, X, Y), device=0)
    pipe.project(pipe.upload_stack(synthetic.make_stack(Z, Y, X, seed=100)))
    pipe.sync()
    img = pipe._proj_t[[1, 0]].transpose(1, 2)          # as FramePipeline.segment_unet
    nbytes = img.numel() * 8
    floor_ms = 7 * nbytes / 4e12 * 1e3
    for rnd in range(args.rounds):
        for _ in range(args.warmup):
            pred.prepare_image(img)
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.calls)]
        torch.cuda.synchronize()
        for e0, e1 in evs:
            e0.record()
            pred.prepare_image(img)
            e1.record()
        torch.cuda.synchronize()
        ms = np.array([e0.elapsed_time(e1) for e0, e1 in evs])
        print(json.dumps(dict(tool="prepare_time", label=args.label, lib=os.path.basename(_lib.LIB_PATH), round=rnd, calls=args.calls,
                              shape=list(img.shape), median_ms=round(float(np.median(ms)), 4), min_ms=round(float(ms.min()), 4),
                              max_ms=round(float(ms.max()), 4), seven_reads_at_4TBs_ms=round(floor_ms, 4),
                              median_over_seven_reads=round(float(np.median(ms)) / floor_ms, 2))), flush=True)


if __name__ == "__main__":
    main()
