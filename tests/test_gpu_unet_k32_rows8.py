"""GPU: the K = 32 kernel on 8-row tiles (csrc/tip_unet_conv_k32.h, k_unet_conv_k32<UcLayout<2, 8, 2>>: 256 threads, a weight ring of
two pair steps, the workgroup's barrier BETWEEN pair steps), which only TIP_UNET_CONV_ROWS8_K32 of tip_unet_conv_ex_dev selects.
One launch at a time against the float64 evaluation of the same stencil, through unet_layers.run_layer: inside `flagged()` the
library run_layer sees hands its two calls to the _ex entries with the flag, so the flavour code (0, asserted by run_layer) and
K = 32 (asserted here) are checked in front of every launch, and every output sits between sentinel bands.

Grids: 8 x 32 (one tile); 24 x 64 (seams both ways, and 24 % 16 != 0 forces 8-row tiles for every tap count); 32 x 64 under
TIP_UNET_TILE8=1 (eight tiles: the only one of the three where the XCD workgroup order switches on, with 256 output channels).
Output channels 128 and 256, each with the XCD order on and off.  (taps, c0, c1) at the schedule's edges: (4, 16, 0) two pair
steps, the ring never wraps; (5, 16, 0), (9, 16, 0) an odd count, the tail step alone; (9, 32, 0) a pair straddling the chunk boundary
and the chunk prefetch; (6, 48, 0); (9, 16, 16), (7, 16, 32) the second input from its first chunk on, with a re-plan for another
channel count.  Epilogues, one case each: BatchNorm (the sweeps), bias only, pooled, fused head, raw output at stride 2, seeded."""
import contextlib
import ctypes
import functools

import numpy as np
import pytest

import unet_layers as ul
from unet_layers import HEAD_TOL, REGIONS, TOL, _assert_regions, _join, _split, bits, exact_case, random_case, run_case

pytestmark = pytest.mark.gpu

MODE, FLAG = "f16x3", 1          # TIP_UNET_CONV_ROWS8_K32
CASES = [(4, 16, 0), (5, 16, 0), (9, 16, 0), (9, 32, 0), (6, 48, 0), (9, 16, 16), (7, 16, 32)]
GRIDS = [(8, 32), (24, 64), (32, 64)]
COUTS = [128, 256]
EPILOGUE_CASE = (9, 32, 0)
HEAD_CASE = (9, 16, 16)          # (of CASES, one whose float64 probabilities are unsaturated in > 90 % of the pixels: a property of the data)
EH, EW = 24, 64


class _Flagged:
    """the library, its unflagged convolution entries answered by the _ex entries with the flag"""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def tip_unet_conv_dev(self, d, stream):
        return self._lib.tip_unet_conv_ex_dev(d, FLAG, stream)

    def tip_unet_conv_flavour(self, d):
        return self._lib.tip_unet_conv_flavour_ex(d, FLAG)


@contextlib.contextmanager
def flagged():
    from tissue_image_processing_amd import _lib
    real = _lib.lib
    _lib.lib = lambda: _Flagged(real())
    try:
        yield
    finally:
        _lib.lib = real


def _tune(h):
    """24 and 8 rows are no multiple of 16; at 32 rows the tuning asks for the 8-row tiles"""
    return {"TIP_UNET_TILE8": "1"} if h % 16 == 0 else {}


def _mfma_k(ntaps, c0, c1, h, w, cout, flags):
    from tissue_image_processing_amd import _lib
    dy, dx = ul.tap_offsets(ntaps)
    d = ul.describe(MODE, (h, w, c0), (h, w, c1) if c1 else None, ntaps, dy, dx, cout, out_h=h, out_w=w)
    return _lib.lib().tip_unet_conv_mfma_k_ex(ctypes.byref(d), flags)


def _run(c, ntaps, c0, c1, h, w, flag=True, **kw):
    """one launch of flavour 0 under the grid's tuning; (code, K) asserted first: (0, 32) with the flag, (0, 16) without"""
    from tissue_image_processing_amd import _lib
    with _lib.tuning(**_tune(h)):
        assert _mfma_k(ntaps, c0, c1, h, w, c["taps"].shape[2], FLAG if flag else 0) == (32 if flag else 16)
        if not flag:
            return run_case(MODE, 0, c, **kw)
        with flagged():
            return run_case(MODE, 0, c, **kw)


@pytest.mark.parametrize("cout", COUTS)
@pytest.mark.parametrize("h,w", GRIDS)
@pytest.mark.parametrize("ntaps,c0,c1", CASES)
def test_exact_data_equal_float64(ntaps, c0, c1, h, w, cout):
    """EXACT data: raw output equal to float64, seeded output equal to seed + sum, identical bits twice in a row and with the XCD
    order off; stored pieces equal to the split of the float64 result"""
    import torch
    from tissue_image_processing_amd import _lib
    c = exact_case(ntaps, c0, c1, cout, h, w)
    bn = dict(bias=c["bias"], scale=c["scale"], shift=c["shift"])
    raw = _run(c, ntaps, c0, c1, h, w, raw=True)["raw"]
    again = _run(c, ntaps, c0, c1, h, w, raw=True)["raw"]
    seeded = _run(c, ntaps, c0, c1, h, w, raw=True, seed=c["seed"])["raw"]
    stored = _run(c, ntaps, c0, c1, h, w, **bn)
    with _lib.tuning(TIP_UNET_XCD_MAP="0"):
        raw_plain = _run(c, ntaps, c0, c1, h, w, raw=True)["raw"]
        stored_plain = _run(c, ntaps, c0, c1, h, w, **bn)["out"]
    wrong = raw.double() != c["ref"]["sum"]
    print("%d of %d raw sums differ from float64" % (int(wrong.sum()), wrong.numel()))
    assert not bool(wrong.any()), "raw output differs from float64 at (y, x, channel) %s ..." % wrong.nonzero()[:4].tolist()
    assert torch.equal(seeded.double(), c["seeded"]), "seeded raw output differs from float64's seed + sum"
    assert torch.equal(bits(again), bits(raw)), "two identical launches differ"
    assert torch.equal(bits(raw_plain), bits(raw)), "TIP_UNET_XCD_MAP=0 changes the raw output"
    assert stored["status"] == 0
    want = _split(c["ref"]["out"].float(), 2, 1)
    assert torch.equal(bits(stored["out"]), bits(want)), "stored pieces differ from the split of the float64 result"
    assert torch.equal(bits(stored_plain), bits(stored["out"]))


@pytest.mark.parametrize("cout", COUTS)
@pytest.mark.parametrize("h,w", GRIDS)
@pytest.mark.parametrize("ntaps,c0,c1", CASES)
def test_random_data_within_layer_bounds(ntaps, c0, c1, h, w, cout):
    """RANDOM data: unet_layers' per-layer bound for f16x3 on the tensor, every border region and every tile seam; the flagged and
    the unflagged launch, each within that bound of float64, differ by at most twice the bound; the XCD order changes no bit"""
    import torch
    from tissue_image_processing_amd import _lib
    c = random_case(ntaps, c0, c1, cout, h, w)
    bn = dict(bias=c["bias"], scale=c["scale"], shift=c["shift"])
    res = _run(c, ntaps, c0, c1, h, w, **bn)
    old = _run(c, ntaps, c0, c1, h, w, flag=False, **bn)
    with _lib.tuning(TIP_UNET_XCD_MAP="0"):
        plain = _run(c, ntaps, c0, c1, h, w, **bn)
    assert res["status"] == 0 and old["status"] == 0
    assert torch.equal(bits(plain["out"]), bits(res["out"]))
    got, was = _join(res["out"], 1).double(), _join(old["out"], 1).double()
    what = "8-row K = 32, %d taps %d+%d->%d, %dx%d" % (ntaps, c0, c1, cout, h, w)
    _assert_regions(MODE, what, got, c["ref"]["out"], REGIONS)
    ul.assert_seams(MODE, what, got, c["ref"]["out"], 8)
    diff = float((got - was).abs().max()) / float(c["ref"]["out"].abs().max())
    print("%s: max |K = 32 - K = 16| / max |value| = %.2e" % (what, diff))
    assert diff <= 2 * TOL[MODE]


def test_the_xcd_order_switches_on_one_grid():
    """what the sweeps' XCD comparisons compare: ntiles % 8 == 0 and two channel blocks -- 32 x 64 with 256 output channels alone"""
    for h, w in GRIDS:
        for cout in COUTS:
            assert ((h // 8) * (w // 32) % 8 == 0 and cout > 128) == ((h, w, cout) == (32, 64, 256))


# ---- the epilogue's forms on the 8-row instance, one case each ------------------------------------------------------------------------

def test_bias_only_epilogue():
    c = random_case(*EPILOGUE_CASE, 256, EH, EW)
    res = _run(c, *EPILOGUE_CASE, EH, EW, bias=c["bias"])
    assert res["status"] == 0
    got = _join(res["out"], 1).double()
    assert float(c["ref_bias"].min()) < -0.1 * float(c["ref_bias"].abs().max())
    _assert_regions(MODE, "bias-only epilogue", got, c["ref_bias"], REGIONS)
    ul.assert_seams(MODE, "bias-only epilogue", got, c["ref_bias"], 8)


def test_pooled_output():
    """the pooled planes are exactly max_pool2d of the joined stored output, which is the launch's without pool_out bit for bit"""
    import torch
    c = random_case(*EPILOGUE_CASE, 256, EH, EW)
    bn = dict(bias=c["bias"], scale=c["scale"], shift=c["shift"])
    res = _run(c, *EPILOGUE_CASE, EH, EW, pool=True, **bn)
    alone = _run(c, *EPILOGUE_CASE, EH, EW, **bn)["out"]
    assert torch.equal(bits(res["out"]), bits(alone))
    assert torch.equal(_join(res["pool"]), torch.nn.functional.max_pool2d(_join(res["out"]).permute(2, 0, 1)[None], 2)[0].permute(1, 2, 0))
    _assert_regions(MODE, "pooled output", _join(res["pool"], 1).double(), c["ref"]["pool"], REGIONS)
    _assert_regions(MODE, "output next to the pooled one", _join(res["out"], 1).double(), c["ref"]["out"], ["all"])


def test_fused_head():
    """head_out (128 output channels) against float64's softmax and against tip_unet_head_dev on the same layer's stored planes"""
    c = random_case(*HEAD_CASE, 128, EH, EW)
    bn = dict(bias=c["bias"], scale=c["scale"], shift=c["shift"])
    fused = _run(c, *HEAD_CASE, EH, EW, head=(c["hw"], c["hb"]), **bn)
    stored = _run(c, *HEAD_CASE, EH, EW, **bn)["out"]
    assert fused["status"] == 0
    ref = c["ref"]["head"]
    assert float((ref * (1 - ref) > 0.05).double().mean()) > 0.9
    separate = ul.head_dev(MODE, stored, c["hw"], c["hb"], 0)
    e_f, e_fs = float((fused["head"].double() - ref).abs().max()), float((fused["head"].double() - separate.double()).abs().max())
    print("fused head: max |dp| vs float64 %.2e, fused vs separate %.2e" % (e_f, e_fs))
    assert e_f < HEAD_TOL[MODE] and e_fs < HEAD_TOL[MODE]


@pytest.mark.parametrize("oy,ox", [(0, 1), (1, 0)])
def test_raw_output_at_stride_two(oy, ox):
    """raw output through the stride-2 mapping with offsets: the class equal to float64, the other three parity classes keep the
    sentinel (run_layer)"""
    import torch
    e = exact_case(*EPILOGUE_CASE, 256, EH, EW)
    raw = _run(e, *EPILOGUE_CASE, EH, EW, raw=True, stride=2, oy=oy, ox=ox)["raw"]
    assert torch.equal(raw[oy::2, ox::2].double(), e["ref"]["sum"])


def test_seeded_layer():
    """the accumulator seed under the BatchNorm epilogue: float64's relu(seed + sum + bias) * scale + shift within the layer bound"""
    import torch
    c = random_case(*EPILOGUE_CASE, 256, EH, EW)
    seed = torch.randn((EH, EW, 256), generator=torch.Generator().manual_seed(77)) * float(c["ref"]["sum"].abs().max()) * 0.3
    ref = ul.reference(c["a0"], c["a1"], c["taps"], c["dy"], c["dx"], c["bias"], c["scale"], c["shift"], seed=seed)["out"]
    res = _run(c, *EPILOGUE_CASE, EH, EW, bias=c["bias"], scale=c["scale"], shift=c["shift"], seed=seed)
    assert res["status"] == 0
    got = _join(res["out"], 1).double()
    assert float((ref - c["ref"]["out"]).abs().max()) > 0.1 * float(ref.abs().max())        # the seed matters
    _assert_regions(MODE, "seeded layer", got, ref, REGIONS)
    ul.assert_seams(MODE, "seeded layer", got, ref, 8)


# ---- the network: the driver's switch ---------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _network_reference(trained_like):
    import torch
    from tissue_image_processing_amd import prediction_local as pl
    ref = pl._UNet(2, "cpu", dtype=torch.float64, seed=3)
    if trained_like:
        ref.randomize_statistics(4)
    x = torch.from_numpy(np.random.default_rng(0).random((1, 2, 64, 256)))
    return x, ref.forward(x)


@pytest.mark.parametrize("rows8", ["1", "0"])
@pytest.mark.parametrize("trained_like", [False, True])
def test_network_within_its_bound_flag_on_and_off(trained_like, rows8, monkeypatch):
    """test_gpu_unet_conv.py::test_network_hip_path_vs_float64 in mode f16x3 (class probabilities within 4e-6 of the float64 network)
    with TISSUE_HIP_UNET_ROWS8_K32 at its default and at 0; the launches are recorded: at 64 x 256 the pass's 8-row launches are the
    four 128-channel 3x3 layers (d0.c2, d1.c1, u2.c1 seeded, u2.c2) and, the bottleneck's grid being 8 x 32, mid.c1, mid.c2 and
    the four composed stencils of u0 (64 chunks of 4 to 9 taps: the longest loops the new instance runs here) -- all of four and
    more taps, and they take K = 32 exactly when the switch is on"""
    import torch
    from tissue_image_processing_amd import _lib, _unet_hip, prediction_local as pl
    monkeypatch.setenv("TISSUE_HIP_UNET_ARITH", MODE)
    if rows8 == "0":
        monkeypatch.setenv("TISSUE_HIP_UNET_ROWS8_K32", "0")
    else:
        monkeypatch.delenv("TISSUE_HIP_UNET_ROWS8_K32", raising=False)
    assert _unet_hip.conv_flags(MODE) == (FLAG if rows8 == "1" else 0) and _unet_hip.conv_flags("bf16x6") == 0
    launches = []

    class Counting:
        def __init__(self, lib):
            self._lib = lib

        def __getattr__(self, name):
            return getattr(self._lib, name)

        def tip_unet_conv_ex_dev(self, d, flags, stream):
            launches.append((self._lib.tip_unet_conv_flavour_ex(d, flags), self._lib.tip_unet_conv_mfma_k_ex(d, flags), flags))
            return self._lib.tip_unet_conv_ex_dev(d, flags, stream)

    real = _lib.lib
    monkeypatch.setattr(_lib, "lib", lambda: Counting(real()))
    gpu = pl._UNet(2, torch.device("cuda", 0), dtype=torch.float32, seed=3)
    if trained_like:
        gpu.randomize_statistics(4)
    x, exp = _network_reference(trained_like)
    xg = x.to("cuda").float()
    assert gpu.hip_path_ok(xg)
    out = gpu.forward(xg).cpu().double()
    assert gpu.last_mode == MODE
    err = float((out - exp).abs().max())
    print("f16x3 network 64x256, TISSUE_HIP_UNET_ROWS8_K32=%s (%s): max |dp| = %.2e"
          % (rows8, "biases + BatchNorm statistics" if trained_like else "identity BatchNorm", err))
    assert err < 4e-6
    assert all(f == (FLAG if rows8 == "1" else 0) for _, _, f in launches)
    rows8_k = [k for code, k, _ in launches if code == 0]
    assert len(rows8_k) == 10 and all(k == (32 if rows8 == "1" else 16) for k in rows8_k), launches
