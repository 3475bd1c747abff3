"""GPU: the fp16 range guard of the U-Net's default arithmetic (f16x3 stores activations as fp16 pieces of 16 v and clamps beyond
|v| = 4094): the device-side flag (csrc/tip_unet_conv.h: uc_range_flag), the policy TISSUE_HIP_UNET_RANGE and the rerun in bf16x6.

The overflowing networks are the SAME network mathematically: A = _UNet(seed 3) with randomize_statistics(4); B = A with one
layer's output multiplied by K = 2^k (its BatchNorm scale and shift, or a transposed convolution's weights and bias) and the weights
of every reader of that tensor divided by K -- powers of two, so exact.  Reference: the float64 CPU network of A, computed once;
tolerance 4e-6 on the probabilities, the bound test_gpu_unet_conv.py::test_network_hip_path_vs_float64 holds the float32-equivalent
modes to.  A's largest activation is 18 (mid.b1: 18.03) and its smallest per-layer maximum 4.1, so k = 14 overflows at every site."""
import ctypes
import threading
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 4e-6
ACT = 16.0                                                        # _unet_hip._F16_ACT_SCALE
# site -> (tensors multiplied by K, [(tensor divided by K, its input-channel slice)])
SITES = {
    "d0.b1": (("d0.b1.s", "d0.b1.t"), (("d0.c2.w", slice(None)),)),                                    # k_unet_conv_first
    "d0.b2": (("d0.b2.s", "d0.b2.t"), (("d1.c1.w", slice(None)), ("u2.c1.w", slice(128, None)))),    # pool epilogue + the skip
    "mid.b1": (("mid.b1.s", "mid.b1.t"), (("mid.c2.w", slice(None)),)),                                # plain convolution
    "mid.b2": (("mid.b2.s", "mid.b2.t"), (("u0.t.w", slice(None)),)),                                  # input of the composed level
    "u0.t": (("u0.t.w", "u0.t.b"), (("u0.c1.w", slice(0, 512)),)),                                     # bias-only branch (uncomposed)
}


def _net_a(dev):
    import torch
    from tissue_image_processing_amd import prediction_local as pl
    net = pl._UNet(2, dev, dtype=torch.float32, seed=3)
    net.randomize_statistics(4)
    return net


def _net_b(site, k, dev="cuda"):
    """A with the tensor at `site` scaled by 2^k and its readers by 2^-k"""
    net = _net_a(dev)
    up, down = SITES[site]
    K = 2.0 ** k
    for name in up:
        net.p[name] *= K
    for name, sl in down:
        if name.endswith(".t.w"):          # transposed convolution: (in, out, ky, kx)
            net.p[name][sl] /= K
        else:                              # convolution: (out, in, ky, kx)
            net.p[name][:, sl] /= K
    net._hipw.clear()
    net.reset_range()
    return net


@pytest.fixture(scope="module")
def case():
    """(input on the device, float64 reference probabilities of A on the host); computed once, never changed"""
    import torch
    x = torch.from_numpy(np.random.default_rng(0).random((1, 2, 64, 256)))
    from tissue_image_processing_amd import prediction_local as pl
    ref = pl._UNet(2, "cpu", dtype=torch.float64, seed=3)
    ref.randomize_statistics(4)
    exp = ref.forward(x)
    return x.to("cuda").float(), exp


@pytest.fixture()
def env(monkeypatch):
    for v in ("TISSUE_HIP_UNET_RANGE", "TISSUE_HIP_UNET_ARITH", "TISSUE_HIP_UNET_COMPOSE"):
        monkeypatch.delenv(v, raising=False)

    def set_env(**kw):
        for k, v in kw.items():
            monkeypatch.setenv("TISSUE_HIP_UNET_" + k, v)
    return set_env


def _err(p, exp):
    return float((p.cpu().double() - exp).abs().max())


def _quiet_forward(net, x):
    """a pass during which a RuntimeWarning is an error"""
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        return net.forward(x)


def _site_env(env, site):
    if site == "u0.t":
        env(COMPOSE="0")           # the up-sampled tensor exists (and is rounded to fp16) only without the composed level


@pytest.mark.parametrize("site", list(SITES))
def test_construction_is_the_same_network(site, case, env):
    """(passes without the guard) B in bf16x6 -- float32's exponent range -- is A to the bound"""
    import torch
    x, exp = case
    env(ARITH="bf16x6")
    pa = _quiet_forward(_net_a("cuda"), x)
    b = _net_b(site, 14)
    pb = _quiet_forward(b, x)
    err = _err(pb, exp)
    print("site %s, k 14, bf16x6: max |dp| vs float64 %.2e, bit-equal to A's bf16x6 result: %s" % (site, err, bool(torch.equal(pa, pb))))
    assert b.last_mode == "bf16x6" and b.range_exceeded is False
    assert err < TOL


@pytest.mark.parametrize("site", list(SITES))
def test_fallback(site, case, env):
    import torch
    x, exp = case
    _site_env(env, site)
    b = _net_b(site, 14)
    assert b.hip_path_ok(x)
    with pytest.warns(RuntimeWarning, match="fp16's range"):
        p1 = b.forward(x)
    err = _err(p1, exp)
    print("site %s, k 14, default mode and policy: ran %s, max |dp| vs float64 %.2e" % (site, b.last_mode, err))
    assert b.last_mode == "bf16x6" and b.range_exceeded is True
    assert err < TOL
    p2 = _quiet_forward(b, x)              # sticky: straight to bf16x6, no second warning
    assert torch.equal(p1, p2) and b.last_mode == "bf16x6"
    z = _quiet_forward_logits(b, x)
    assert b.last_mode == "bf16x6" and bool(torch.isfinite(z).all())
    b.reset_range()
    with pytest.warns(RuntimeWarning):     # the requested mode is tried again, and overflows again
        p3 = b.forward(x)
    assert torch.equal(p1, p3) and b.range_exceeded is True


def _quiet_forward_logits(net, x):
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        return net.forward(x, logits=True)


def test_composed_level_never_rounds_the_upsampled_tensor(case, env):
    """u0.t in the default composed mode: the transposed convolution is folded into the next convolution's weights, its output is
    never stored as fp16 pieces, so nothing overflows and nothing is flagged"""
    x, exp = case
    b = _net_b("u0.t", 14)
    p = _quiet_forward(b, x)
    err = _err(p, exp)
    print("site u0.t composed, k 14: ran %s (%s), max |dp| vs float64 %.2e" % (b.last_mode, b.last_compose, err))
    assert "u0" in b.last_compose
    assert b.last_mode == "f16x3" and b.range_exceeded is False
    assert err < TOL


@pytest.mark.parametrize("site", ["d0.b1", "mid.b1", "u0.t"])
def test_raise_policy(site, case, env):
    from tissue_image_processing_amd import prediction_local as pl, _lib
    x, _ = case
    _site_env(env, site)
    env(RANGE="raise")
    b = _net_b(site, 14)
    for _ in range(2):                     # nothing sticks: the second pass tries f16x3 again and says the same
        with pytest.raises(pl.UNetRangeError, match=r"f16x3.*4094.*TISSUE_HIP_UNET_ARITH=bf16x6.*TISSUE_HIP_UNET_RANGE=fallback") as ei:
            _quiet_forward(b, x)
        assert isinstance(ei.value, _lib.TissueHipError)
        assert b.range_exceeded is False and b.last_mode == "f16x3"
    with pytest.raises(pl.UNetRangeError):
        _quiet_forward_logits(b, x)


def test_off_policy_is_the_unguarded_pass(case, env):
    import torch
    x, _ = case
    env(RANGE="off")
    b = _net_b("mid.b1", 14)
    p = _quiet_forward(b, x)
    assert b.last_mode == "f16x3" and b.range_exceeded is False
    assert bool(torch.isfinite(p).all())


def test_no_false_positive(case, env):
    import torch
    x, exp = case
    a = _net_a("cuda")
    p = _quiet_forward(a, x)
    assert a.last_mode == "f16x3" and a.range_exceeded is False
    assert _err(p, exp) < TOL
    env(RANGE="off")
    assert torch.equal(p, _quiet_forward(a, x))


def test_threshold_between_k7_and_k8(case, env):
    """mid.b1's largest |v| is 18.03: times 2^7 = 2308 (stored 36 900) is inside the range, times 2^8 = 4615 is beyond 4094"""
    x, exp = case
    b7 = _net_b("mid.b1", 7)
    p7 = _quiet_forward(b7, x)
    err7 = _err(p7, exp)
    print("site mid.b1, k 7: ran %s, max |dp| vs float64 %.2e" % (b7.last_mode, err7))
    assert b7.last_mode == "f16x3" and b7.range_exceeded is False
    assert err7 < TOL
    b8 = _net_b("mid.b1", 8)
    with pytest.warns(RuntimeWarning):
        p8 = b8.forward(x)
    err8 = _err(p8, exp)
    print("site mid.b1, k 8: ran %s, max |dp| vs float64 %.2e" % (b8.last_mode, err8))
    assert b8.last_mode == "bf16x6" and b8.range_exceeded is True
    assert err8 < TOL


# ---- the flag itself, through the C-ABI ---------------------------------------------------------------------------------------------
def _status(lib, stream):
    from tissue_image_processing_amd import _lib
    flags = ctypes.c_int(-1)
    _lib.check(lib.tip_unet_range_read(stream, ctypes.byref(flags)))
    return flags.value


def _first_layer(lib, stream, dev, scale_value, channel=5):
    """tip_unet_conv_first_dev on 8 x 32 pixels, fp16 pieces: input 1 (channel 0), centre weight 1 into `channel`, bias 0, shift 0:
    that channel's value in front of the clamp is exactly scale_value -> (status word, stored hi / lo pieces of the channel)"""
    import torch
    from tissue_image_processing_amd import _lib
    H, W = 8, 32
    x = torch.zeros((2, H, W), dtype=torch.float32, device=dev)
    x[0] = 1.0
    wgt = torch.zeros((9, 2, 128), dtype=torch.float32, device=dev)
    wgt[4, 0, channel] = 1.0
    bias, shift = torch.zeros(128, device=dev), torch.zeros(128, device=dev)
    scale = torch.full((128,), float(scale_value), dtype=torch.float32, device=dev)
    out = torch.empty((2, H, W, 128), dtype=torch.float16, device=dev)
    _lib.check(lib.tip_unet_range_reset(stream))
    _lib.check(lib.tip_unet_conv_first_dev(x.data_ptr(), H, W, wgt.data_ptr(), bias.data_ptr(), scale.data_ptr(), shift.data_ptr(),
                                           out.data_ptr(), 2, 1, stream))
    st = _status(lib, stream)
    o = out.cpu().float()
    assert float(o[..., [c for c in range(128) if c != channel]].abs().max()) == 0.0
    return st, o[0, :, :, channel], o[1, :, :, channel]


def test_exact_limit_first_layer():
    import torch
    from tissue_image_processing_amd import _lib
    dev = torch.device("cuda", 0)
    lib = _lib.lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    st, hi, lo = _first_layer(lib, stream, dev, 65504.0)
    assert st == 0                                             # exactly the largest finite fp16: in range
    assert float(hi.min()) == float(hi.max()) == 65504.0 and float(lo.abs().max()) == 0.0
    over = np.nextafter(np.float32(65504.0), np.float32(np.inf))
    st, hi, lo = _first_layer(lib, stream, dev, over)
    assert st == 1
    assert float(hi.min()) == float(hi.max()) == 65504.0 and float(lo.abs().max()) == 0.0      # clamped as before
    st, hi, lo = _first_layer(lib, stream, dev, 65504.0)       # reset clears the word
    assert st == 0


@pytest.mark.parametrize("branch", ["batchnorm", "bias_only"])
def test_conv_epilogue_branches_flag(branch):
    """tip_unet_conv_dev with the descriptor of test_gpu_unet_conv.py::test_fp16_pieces_saturate_and_keep_subnormals (8 x 32 pixels,
    a one-tap stencil, bias[0] = 1e6): bit 0 is set and the output is what it was -- channel 0 clamped at 65504, the others exact;
    without the large bias the word stays 0"""
    import torch
    from tissue_image_processing_amd import prediction_local as pl, _lib, _unet_hip
    dev = torch.device("cuda", 0)
    lib = _lib.lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    H, W, C0, CO = 8, 32, 16, 128
    g = torch.Generator().manual_seed(3)
    a = (torch.rand((H, W, C0), generator=g) * 2 - 1) * 2.0 ** -9
    wt = torch.randn((1, C0, CO), generator=g)
    big = float(wt.abs().max())
    wscale = 2.0 ** (14 - int(np.floor(np.log2(big))))
    wp, inv = _unet_hip.split_pack((wt * wscale).to(dev), 2, 1), 1.0 / (ACT * wscale)
    rest = a * ACT
    hi = rest.to(torch.float16)
    pa = torch.stack([hi, (rest - hi.float()).to(torch.float16)], 0).contiguous().to(dev)
    out = torch.empty((2, H, W, CO), dtype=torch.float16, device=dev)
    scale, shift = torch.full((CO,), ACT).to(dev), torch.zeros(CO).to(dev)
    got = {}
    for b0 in (1e6, 0.0):
        bias = torch.zeros(CO)
        bias[0] = b0
        fb = bias.to(dev)
        d = pl._ConvDesc()
        d.in0, d.c0, d.in1, d.c1, d.h, d.w, d.planes, d.format = pa.data_ptr(), C0, None, 0, H, W, 2, 1
        d.weights, d.ntaps, d.cout = wp.data_ptr(), 1, CO
        d.dy[0], d.dx[0] = 0, 0
        d.bias = fb.data_ptr()
        if branch == "batchnorm":
            d.acc_scale, d.scale, d.shift = inv, scale.data_ptr(), shift.data_ptr()
        else:
            d.acc_scale, d.scale, d.shift = inv * ACT, None, None      # (a bias-only layer's accumulator factor and bias carry the scale)
        d.out, d.out_h, d.out_w, d.sy, d.sx, d.oy, d.ox = out.data_ptr(), H, W, 1, 1, 0, 0
        _lib.check(lib.tip_unet_range_reset(stream))
        _lib.check(lib.tip_unet_conv_dev(ctypes.byref(d), stream))
        got[b0] = (_status(lib, stream), out.cpu().float())
    st, o = got[1e6]
    assert st == 1
    assert bool(torch.isfinite(o).all()) and float(o[0, :, :, 0].min()) == 65504.0
    val = (o.sum(0) / ACT).double()[..., 1:]
    ref = torch.einsum("hwk,kc->hwc", a.double(), wt[0].double())[..., 1:]
    if branch == "batchnorm":
        ref = torch.relu(ref)
    assert float((val - ref).abs().max() / ref.abs().max()) < 2e-6
    st0, o0 = got[0.0]
    assert st0 == 0 and torch.equal(o0[..., 1:], o[..., 1:])


def test_status_word_is_per_thread():
    """Two threads, each with its own torch stream and its own library context: one launches an overflowing first layer, the
    other a clean one, both before either reads -- the first reads 1, the second 0."""
    import torch
    from tissue_image_processing_amd import _lib
    dev = torch.device("cuda", 0)
    lib = _lib.lib()
    over = np.nextafter(np.float32(65504.0), np.float32(np.inf))
    both = threading.Barrier(2, timeout=120)
    result, errors = {}, []

    def work(name, scale_value):
        try:
            _lib.init(0)
            s = torch.cuda.Stream(dev)
            with torch.cuda.stream(s):
                stream = ctypes.c_void_p(s.cuda_stream)
                H, W = 8, 32
                x = torch.ones((2, H, W), dtype=torch.float32, device=dev)
                wgt = torch.zeros((9, 2, 128), dtype=torch.float32, device=dev)
                wgt[4, 0, 5] = 1.0
                zero = torch.zeros(128, device=dev)
                scale = torch.full((128,), float(scale_value), dtype=torch.float32, device=dev)
                out = torch.empty((2, H, W, 128), dtype=torch.float16, device=dev)
                _lib.check(lib.tip_unet_range_reset(stream))
                _lib.check(lib.tip_unet_conv_first_dev(x.data_ptr(), H, W, wgt.data_ptr(), zero.data_ptr(), scale.data_ptr(), zero.data_ptr(),
                                                       out.data_ptr(), 2, 1, stream))
                both.wait()                # both launches are queued before either thread reads
                result[name] = _status(lib, stream)
                s.synchronize()
        except BaseException as e:
            both.abort()
            errors.append(e)
        finally:
            lib.tip_shutdown()             # this thread's context, its status word included

    threads = [threading.Thread(target=work, args=("over", over)), threading.Thread(target=work, args=("clean", 65504.0))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert result == {"over": 1, "clean": 0}


# ---- the movie driver ------------------------------------------------------------------------------------------------------------------
def test_movie_frames_record_the_fallback(env):
    """GpuFrameBackend in U-Net mode with predictors whose network overflows (mid.b1, k = 14): every frame's mode is bf16x6, and the
    label maps are those of the unscaled network A asked for bf16x6."""
    import _gpu_movie_unet_worker as W
    from tissue_image_processing_amd import movie
    from tissue_image_processing_amd.prediction_local import SegmentationPredictor
    frames = 2
    FRACTION = 0.1          # (calibrated foreground: A's smooth maps leave the tail no cell-sized blobs at the worker's 0.5, dozens at 0.1)
    stacks = W.movie_stacks(frames=frames)
    fixed = np.stack([stacks[0][1].max(0).T, stacks[0][0].max(0).T]).astype(np.float64)      # (2, X, Y), as W.predictor_factory has it

    def factory_for(make_net):
        def factory(device):
            pred = SegmentationPredictor(None, (2, W.X, W.Y), device=device)
            pred.model = make_net()
            padded, _ = pred.prepare_image(fixed)
            pred.model.calibrate_head(padded, FRACTION)
            return pred
        return factory

    def run(factory):
        backend = movie.GpuFrameBackend(2, W.Z, W.Y, W.X, device=0, segmentation="unet", predictor_factory=factory)
        try:
            movie.process_movie(frames, lambda t: stacks[t], backend, drifts=W.drift_rows(frames))
            routes = [p.last_route for p in backend._predictors.values()]
            return dict(backend.unet_modes), [backend.labels[t].download((W.Y, W.X), np.int32) for t in range(frames)], routes
        finally:
            backend.close()

    with pytest.warns(RuntimeWarning, match="fp16's range"):
        modes_b, labels_b, routes_b = run(factory_for(lambda: _net_b("mid.b1", 14)))
    assert modes_b == {t: "bf16x6" for t in range(frames)}
    assert routes_b == [dict(requested="f16x3", ran="bf16x6", range_exceeded=True)]
    env(ARITH="bf16x6")
    modes_a, labels_a, routes_a = run(factory_for(lambda: _net_a("cuda")))
    assert modes_a == {t: "bf16x6" for t in range(frames)}
    assert routes_a == [dict(requested="bf16x6", ran="bf16x6", range_exceeded=False)]
    for t in range(frames):
        print("frame %d: %d labels" % (t, int(labels_a[t].max())))
        assert int(labels_a[t].max()) >= 2
        np.testing.assert_array_equal(labels_b[t], labels_a[t])
