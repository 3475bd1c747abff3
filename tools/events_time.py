"""Times movie.find_events against the host route it replaces -- Tissue.load of the archive, then find_events_iterator -- on the
frames of bench.py --workload movie (2048 x 2048 x 30, six frames, one GPU), five runs each, and writes profiles/events_time.json
(or argv[1]).  EV_SIZE=Y,X,Z, EV_FRAMES and EV_RUNS shrink it for a rehearsal."""
import json
import os
import sys
import tempfile
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
warnings.simplefilter("ignore")

import numpy as np      # noqa: E402
import torch      # noqa: E402
from tissue_image_processing_amd import movie, synthetic, _lib, events as ev      # noqa: E402
from tissue_image_processing_amd import tissue_info as ti      # noqa: E402

Y, X, Z = (int(v) for v in os.environ.get("EV_SIZE", "2048,2048,30").split(","))
T, RUNS, INFLIGHT = int(os.environ.get("EV_FRAMES", "6")), int(os.environ.get("EV_RUNS", "5")), 4
t0 = time.time()
sites_t, is_hc = synthetic.make_movie_sites(Y, X, T, seed=5)
stacks = [synthetic.make_stack(Z, Y, X, seed=200 + t, sites=sites_t[t], is_hc=is_hc) for t in range(T)]
print("frames made in %.1f s" % (time.time() - t0), flush=True)
backend = movie.GpuFrameBackend(2, Z, Y, X, device=0, keep_planes=True, inflight=INFLIGHT, archive=True)
t0 = time.time()
tabs, ids = movie.process_movie(T, lambda t: stacks[t], backend, 0, 1, None, "cpu", estimate_drift=True, block_frames=INFLIGHT)
print("process_movie %.2f s, rows per frame %s" % (time.time() - t0, [i.size for i in ids]), flush=True)

phase = {}
def timed(name, fn):
    def run(*a, **k):
        s = time.perf_counter()
        try:
            return fn(*a, **k)
        finally:
            phase[name] = phase.get(name, 0.0) + time.perf_counter() - s
    return run
for name in ev.BACKEND_METHODS:
    setattr(backend, name, timed(name, getattr(backend, name)))
ev.events_table = timed("events_table", ev.events_table)

table = movie.find_events(T, backend, tabs, ids)          # warm-up: code objects, workspaces
totals, phases = [], []
for _ in range(RUNS):
    phase.clear()
    _lib.lib().tip_sync()
    s = time.perf_counter()
    table = movie.find_events(T, backend, tabs, ids)
    totals.append(time.perf_counter() - s)
    phases.append(dict(phase))
kernels = []
_lib.prof_enable(True)
for _ in range(RUNS):          # kernel times in runs of their own: HIP events around every launch of the library's stream
    _lib.prof_reset()
    movie.find_events(T, backend, tabs, ids)
    rep = _lib.prof_report()
    kernels.append({k: rep[k][1] / 1e3 for k in ("border_rows", "lookup_exact", "events_init", "events_insert", "events_classify") if k in rep})
_lib.prof_enable(False)
tmp = tempfile.mkdtemp()
path = movie.save_seg(os.path.join(tmp, "movie"), T, backend, tabs, ids, events=table)
backend.close()
print("find_events", totals, flush=True)

loads, iters = [], []
for _ in range(RUNS):
    tissue = ti.Tissue(T)
    s = time.perf_counter()
    for _ in tissue.load(path):
        pass
    loads.append(time.perf_counter() - s)
    tissue.events = ti.make_df(0, ti.EVENTS_INFO_SPEC)
    s = time.perf_counter()
    for _ in tissue.find_events_iterator(1, T):
        pass
    iters.append(time.perf_counter() - s)
    print("host route", loads[-1], iters[-1], flush=True)
want = tissue.events
same = list(table.columns) == list(want.columns) and len(table) == len(want) and all(np.array_equal(table[c].to_numpy(), want[c].to_numpy()) for c in want.columns)

def stats(v):
    v = np.asarray(v, float)
    return dict(runs=[round(float(x), 6) for x in v], median=round(float(np.median(v)), 6), min=round(float(v.min()), 6), max=round(float(v.max()), 6))
kernel_sum = [sum(k.values()) for k in kernels]
out = dict(
    what="movie.find_events against the host route it replaces, same archive; seconds, host clock around calls that end synchronised",
    device=torch.cuda.get_device_name(0), frame=[Y, X, Z], frames=T, pairs=T - 1, rows_per_frame=[int(i.size) for i in ids],
    events=dict(total=len(want), kinds={k: int((want["type"] == k).sum()) for k in sorted(set(want["type"]))}, tables_equal=bool(same)),
    find_events=dict(total=stats(totals), per_pair=stats(np.asarray(totals) / (T - 1)),
                     kernels_total=stats(kernel_sum), kernels_per_pair=stats(np.asarray(kernel_sum) / (T - 1)),
                     kernel_share_of_total=round(float(np.median(kernel_sum) / np.median(totals)), 6),
                     kernels={k: stats([r.get(k, 0.0) for r in kernels]) for k in kernels[0]},
                     phases={k: stats([p.get(k, 0.0) for p in phases]) for k in phases[0]}),
    host_route=dict(load=stats(loads), find_events_iterator=stats(iters), total=stats(np.asarray(loads) + np.asarray(iters)),
                    per_pair=stats((np.asarray(loads) + np.asarray(iters)) / (T - 1))),
    notes="world 1, GpuFrameBackend(archive=True, keep_planes=True, inflight 4), bench.py --workload movie's frames (make_movie_sites seed 5, make_stack seed 200 + t), untyped; "
          "kernel times: the library's HIP-event profiler in %d runs of their own; phases: host clock inside one find_events call" % RUNS)
target = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "events_time.json")
json.dump(out, open(target, "w"), indent=1)
print(json.dumps(out["find_events"]["total"]), json.dumps(out["host_route"]["total"]), out["events"], flush=True)
