"""GPU: the hand-written U-Net layers (csrc/tip_unet_conv.h: implicit-GEMM convolutions on the 16-bit matrix cores with split
float32 operands) against float64 references of the same layers.  The network's trained-weight parity is unpinned (no
TensorFlow, no weights ship with the reference: pl.py:31-72 is restated in prediction_local._UNet); what is pinned here is
that the hand-written kernels compute the SAME network as the torch expressions, to the error bound the split arithmetic
states: per term <= 7.2e-7 relative (f16x3, the default: two fp16 pieces of scaled values, three products), 1.6e-5 (bf16x3:
two bf16 pieces, three products) resp. 9e-8 (bf16x6: three bf16 pieces, six products).  References are float64 evaluations of
the UNSPLIT float32 inputs and weights, so the split error is inside what is measured."""
import ctypes

import numpy as np
import pytest

from unet_layers import ACT, MODES, _join, _split

pytestmark = pytest.mark.gpu


@pytest.fixture()
def arith(monkeypatch):
    def set_mode(m):
        monkeypatch.setenv("TISSUE_HIP_UNET_ARITH", m)
    return set_mode


def _pack(net, taps, planes, fmt):
    """packed split weights and the accumulator factor of a BatchNorm layer (a bias-only layer's is ACT times that)"""
    if not fmt:
        return net._split_pack(taps, planes), 1.0
    big = float(taps.abs().max())
    wscale = 2.0 ** (14 - int(np.floor(np.log2(big))))
    return net._split_pack(taps * wscale, planes, fmt), 1.0 / (ACT * wscale)


@pytest.mark.parametrize("mode", ["f16x3", "bf16x3", "bf16x6"])
def test_single_layers_against_float64(mode, arith):
    """One 3x3 convolution with two concatenated inputs, one transposed convolution, the pooling and the head, each against
    torch float64 on the host ON THE UNSPLIT VALUES, with asymmetric random data (a transposed or mirrored tap / channel order
    cannot pass)."""
    import torch
    from tissue_image_processing_amd import prediction_local as pl, _lib
    arith(mode)
    planes, fmt = MODES[mode]
    tol = {"f16x3": 2e-6, "bf16x3": 4e-5, "bf16x6": 2e-6}[mode]
    store = torch.float16 if fmt else torch.bfloat16
    A = ACT if fmt else 1.0
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(11)
    net = pl._UNet(2, dev, dtype=torch.float32, seed=5)
    lib = _lib.lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    H, W, C0, C1, CO = 16, 64, 32, 16, 128
    a0 = torch.randn((H, W, C0), generator=g)
    a1 = torch.randn((H, W, C1), generator=g)
    wt = torch.randn((CO, C0 + C1, 3, 3), generator=g) * 0.1
    bias, scale, shift = torch.randn(CO, generator=g), torch.rand(CO, generator=g) + 0.5, torch.randn(CO, generator=g)
    taps = torch.stack([wt[:, :, ky, kx].t() for ky in range(3) for kx in range(3)], 0).to(dev)
    wp, inv = _pack(net, taps, planes, fmt)
    p0, p1 = _split(a0, planes, fmt).to(dev), _split(a1, planes, fmt).to(dev)
    out = torch.empty((planes, H, W, CO), dtype=store, device=dev)
    d = pl._ConvDesc()
    d.in0, d.c0, d.in1, d.c1, d.h, d.w, d.planes = p0.data_ptr(), C0, p1.data_ptr(), C1, H, W, planes
    d.format, d.acc_scale = fmt, inv
    d.weights, d.ntaps, d.cout = wp.data_ptr(), 9, CO
    for i in range(9):
        d.dy[i], d.dx[i] = i // 3 - 1, i % 3 - 1
    fb, fs, ft = bias.to(dev), (scale * A).to(dev), (shift * A).to(dev)
    d.bias, d.scale, d.shift = fb.data_ptr(), fs.data_ptr(), ft.data_ptr()
    d.out, d.out_h, d.out_w, d.sy, d.sx, d.oy, d.ox = out.data_ptr(), H, W, 1, 1, 0, 0
    fused_pool = torch.zeros((planes, H // 2, W // 2, CO), dtype=store, device=dev)
    d.pool_out = fused_pool.data_ptr()          # MaxPool2D(2) out of the same epilogue
    _lib.check(lib.tip_unet_conv_dev(ctypes.byref(d), stream))
    torch.cuda.synchronize()
    got = _join(out.cpu(), fmt).double()
    assert torch.equal(_join(fused_pool.cpu()), torch.nn.functional.max_pool2d(_join(out.cpu()).permute(2, 0, 1)[None], 2)[0].permute(1, 2, 0))
    # reference: float64 on the unsplit float32 inputs and weights
    x64 = torch.cat([a0, a1], 2).double().permute(2, 0, 1)[None]
    ref = torch.nn.functional.conv2d(x64, wt.double(), None, padding=1)[0].permute(1, 2, 0)
    ref = torch.relu(ref + bias.double()) * scale.double() + shift.double()
    err = float((got - ref).abs().max() / ref.abs().max())
    print("%s conv3x3: max error / max |value| = %.2e" % (mode, err))
    assert err < tol

    # transposed convolution 3x3 stride 2 'same' (= conv_transpose2d cropped to 2N), bias only
    CI, CO2 = 32, 128
    a = torch.randn((H, W, CI), generator=g)
    wtt = torch.randn((CI, CO2, 3, 3), generator=g) * 0.1
    bt = torch.randn(CO2, generator=g)
    pa = _split(a, planes, fmt).to(dev)
    up = torch.zeros((planes, 2 * H, 2 * W, CO2), dtype=store, device=dev)
    fbt = (bt * A).to(dev)
    per_axis = {0: [(0, 0), (2, -1)], 1: [(1, 0)]}
    keep = []
    for py in (0, 1):
        for px in (0, 1):
            tl = [(ky, dy, kx, dx) for ky, dy in per_axis[py] for kx, dx in per_axis[px]]
            wpk, inv_t = _pack(net, torch.stack([wtt[:, :, ky, kx] for ky, _, kx, _ in tl], 0).to(dev), planes, fmt)
            keep.append(wpk)
            d = pl._ConvDesc()
            d.in0, d.c0, d.in1, d.c1, d.h, d.w, d.planes = pa.data_ptr(), CI, None, 0, H, W, planes
            d.format, d.acc_scale = fmt, inv_t * A
            d.weights, d.ntaps, d.cout = wpk.data_ptr(), len(tl), CO2
            for i, t in enumerate(tl):
                d.dy[i], d.dx[i] = t[1], t[3]
            d.bias, d.scale, d.shift = fbt.data_ptr(), None, None
            d.out, d.out_h, d.out_w, d.sy, d.sx, d.oy, d.ox = up.data_ptr(), 2 * H, 2 * W, 2, 2, py, px
            _lib.check(lib.tip_unet_conv_dev(ctypes.byref(d), stream))
    torch.cuda.synchronize()
    got = _join(up.cpu(), fmt).double()
    ref = torch.nn.functional.conv_transpose2d(a.double().permute(2, 0, 1)[None], wtt.double(), bt.double(), stride=2)[0, :, :2 * H, :2 * W].permute(1, 2, 0)
    err = float((got - ref).abs().max() / ref.abs().max())
    print("%s conv-transpose: max error / max |value| = %.2e" % (mode, err))
    assert err < tol

    # MaxPool2D(2): exact on the split values
    pooled = torch.empty((planes, H // 2, W // 2, CO), dtype=store, device=dev)
    _lib.check(lib.tip_unet_pool2_dev(ctypes.c_void_p(out.data_ptr()), H, W, CO, planes, fmt, ctypes.c_void_p(pooled.data_ptr()), stream))
    torch.cuda.synchronize()
    want = torch.nn.functional.max_pool2d(_join(out.cpu()).permute(2, 0, 1)[None], 2)[0].permute(1, 2, 0)
    assert torch.equal(_join(pooled.cpu()), want)


def test_fp16_pieces_saturate_and_keep_subnormals(arith):
    """fp16 pieces: a value beyond the format's range (|v| >= 4094 with the 2^4 activation scale) saturates at the largest finite
    fp16 instead of becoming an infinity (whose product with a zero weight would poison the next layer), and low pieces in
    fp16's subnormal range survive both the conversion and the matrix core (a flushed low piece would cost 11 bits)."""
    import torch
    from tissue_image_processing_amd import prediction_local as pl, _lib
    arith("f16x3")
    dev = torch.device("cuda", 0)
    net = pl._UNet(2, dev, dtype=torch.float32, seed=5)
    lib = _lib.lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    H, W, C0, CO = 8, 32, 16, 128
    g = torch.Generator().manual_seed(3)
    # activations whose LOW pieces are subnormal (|v * 16| < 2^-3), identity-like 1x1 stencil: out[c] = sum_k a[k] w[k][c]
    a = (torch.rand((H, W, C0), generator=g) * 2 - 1) * 2.0 ** -9
    wt = torch.zeros((1, C0, CO))
    wt[0] = torch.randn((C0, CO), generator=g)
    wp, inv = _pack(net, wt.to(dev), 2, 1)
    pa = _split(a, 2, 1).to(dev)
    assert float(pa[1].float().abs().max()) < 2.0 ** -14            # every low piece is a subnormal fp16
    out = torch.empty((2, H, W, CO), dtype=torch.float16, device=dev)
    bias = torch.zeros(CO)
    bias[0] = 1e6                                                    # channel 0 overflows on purpose
    scale, shift = torch.full((CO,), ACT), torch.zeros(CO)
    d = pl._ConvDesc()
    d.in0, d.c0, d.in1, d.c1, d.h, d.w, d.planes, d.format, d.acc_scale = pa.data_ptr(), C0, None, 0, H, W, 2, 1, inv
    d.weights, d.ntaps, d.cout = wp.data_ptr(), 1, CO
    d.dy[0], d.dx[0] = 0, 0
    fb, fs, ft = bias.to(dev), scale.to(dev), shift.to(dev)
    d.bias, d.scale, d.shift = fb.data_ptr(), fs.data_ptr(), ft.data_ptr()
    d.out, d.out_h, d.out_w, d.sy, d.sx, d.oy, d.ox = out.data_ptr(), H, W, 1, 1, 0, 0
    _lib.check(lib.tip_unet_conv_dev(ctypes.byref(d), stream))
    torch.cuda.synchronize()
    o = out.cpu()
    assert bool(torch.isfinite(o.float()).all())
    assert float(o[0, :, :, 0].float().min()) == 65504.0            # saturated, not infinite
    got = _join(o, 1).double()[..., 1:]
    ref = torch.relu(torch.einsum("hwk,kc->hwc", a.double(), wt[0].double()))[..., 1:]
    err = float((got - ref).abs().max() / ref.abs().max())
    print("fp16 pieces with subnormal low pieces: max error / max |value| = %.2e" % err)
    assert err < 2e-6                                                # (a flushed low piece would leave ~2e-4)


@pytest.mark.parametrize("mode,tol", [("f16x3", 4e-6), ("bf16x3", 3e-5), ("bf16x6", 4e-6)])
@pytest.mark.parametrize("trained_like", [False, True])
def test_network_hip_path_vs_float64(mode, tol, trained_like, arith):
    """The whole network through the hand-written kernels (extents that are multiples of 64 x 256 take that path) against the
    float64 torch network on the host: class probabilities to `tol` absolute -- north_star's float tolerance is 1e-5; the
    float32-equivalent modes are held to 4e-6, the 16-bit-significand mode to its own bound.  trained_like: non-zero biases and
    non-identity BatchNorm statistics in every layer (dense activations with a trained network's dynamic range) instead of the
    he_normal / identity initialisation.  The MIOpen float32 path of the same network is held to 1e-4 by test_gpu_unet.py."""
    import torch
    from tissue_image_processing_amd import prediction_local as pl
    arith(mode)
    gpu = pl._UNet(2, torch.device("cuda", 0), dtype=torch.float32, seed=3)
    ref = pl._UNet(2, "cpu", dtype=torch.float64, seed=3)
    if trained_like:
        gpu.randomize_statistics(4)
        ref.randomize_statistics(4)
    rng = np.random.default_rng(0)
    x = torch.from_numpy(rng.random((1, 2, 64, 256)))
    xg = x.to("cuda").float()
    assert gpu.hip_path_ok(xg)
    out = gpu.forward(xg).cpu().double()
    assert gpu.last_mode == mode
    exp = ref.forward(x)
    err = float((out - exp).abs().max())
    z = gpu.forward(xg, logits=True).cpu().double()
    ze = ref.forward(x, logits=True)
    zerr = float((z - ze).abs().max() / ze.abs().max())
    print("%s network 64x256 (%s): max |dp| = %.2e, max logit error / max |logit| = %.2e"
          % (mode, "biases + BatchNorm statistics" if trained_like else "identity BatchNorm", err, zerr))
    assert err < tol
    arith("miopen")
    assert not gpu.hip_path_ok(xg)


def test_hip_and_miopen_paths_segment_alike(arith):
    """512 x 512 frame through predict() with both convolution paths: the class maps differ in a handful of pixels that sit
    within rounding of the 0.1 threshold (any two float32 convolution orders do), the segmentations agree (IoU)."""
    import torch
    from tissue_image_processing_amd import prediction_local as pl, synthetic
    N = 512
    sites = synthetic.make_sites(N, N, seed=8)[0]
    d1, d2, i1 = synthetic._two_nearest(sites, N, N)
    rng = np.random.default_rng(8)
    zo = 3000 * np.exp(-(d2 - d1) ** 2 / 4) + rng.poisson(100, (N, N))
    atoh = 1500 * (i1 % 3 == 0) + rng.poisson(100, (N, N))
    img = np.stack([atoh, zo]).astype(np.float64)
    pred = pl.SegmentationPredictor(None, img.shape)
    padded, _ = pred.prepare_image(img)
    arith("miopen")
    pred.model.calibrate_head(padded, 0.5)
    p_m = pred.model.forward(padded)[0, 0]
    arith("f16x3")
    p_h = pred.model.forward(padded)[0, 0]
    assert pred.model.last_mode == "f16x3"
    dmax = float((p_m - p_h).abs().max())
    flips = int(((p_m > 0.1) != (p_h > 0.1)).sum())
    print("512^2: max |dp0| between the MIOpen and the f16x3 paths %.2e, thresholded pixels that differ: %d of %d" % (dmax, flips, N * N))
    assert dmax < 1e-4 and flips < N * N * 1e-4


@pytest.mark.parametrize("shape", [(128, 512), (192, 256), (64, 768)])
@pytest.mark.parametrize("mode", ["f16x3", "bf16x3"])
def test_network_hip_path_other_extents(shape, mode, arith, monkeypatch):
    """Extents that mix the kernel's tile flavours over the levels: 16-row tiles with the four-step weight schedule, 16-row
    tiles with the two-chunk activation schedule (one- and two-tap classes), 8-row tiles where a level's grid is not a multiple
    of 16 rows (192 -> 24 rows at the bottleneck), non-square frames; and the 8-row flavour forced everywhere."""
    import torch
    from tissue_image_processing_amd import prediction_local as pl, _lib
    arith(mode)
    tol = 4e-6 if mode == "f16x3" else 3e-5
    gpu = pl._UNet(2, torch.device("cuda", 0), dtype=torch.float32, seed=7)
    ref = pl._UNet(2, "cpu", dtype=torch.float64, seed=7)
    gpu.randomize_statistics(9)
    ref.randomize_statistics(9)
    rng = np.random.default_rng(shape[0])
    x = torch.from_numpy(rng.random((1, 2) + shape))
    xg = x.to("cuda").float()
    assert gpu.hip_path_ok(xg)
    exp = ref.forward(x)
    err = float((gpu.forward(xg).cpu().double() - exp).abs().max())
    with _lib.tuning(TIP_UNET_TILE8="1"):
        err8 = float((gpu.forward(xg).cpu().double() - exp).abs().max())
    with _lib.tuning(TIP_UNET_TILE8="0"):
        err16 = float((gpu.forward(xg).cpu().double() - exp).abs().max())
    # the head as its own kernel on the stored split planes (the default fuses it into the last convolution's epilogue)
    fused = gpu.forward(xg)
    monkeypatch.setenv("TISSUE_HIP_UNET_SEPARATE_HEAD", "1")
    sep = gpu.forward(xg)
    errsep = float((sep.cpu().double() - exp).abs().max())
    dhead = float((sep - fused).abs().max())
    monkeypatch.delenv("TISSUE_HIP_UNET_SEPARATE_HEAD")
    # steps per barrier of the 3x3 16-row kernel (default three) and the workgroup order change the schedule, not the arithmetic
    for knob, val in (("TIP_UNET_SPB", "1"), ("TIP_UNET_XCD_MAP", "0")):
        with _lib.tuning(**{knob: val}):
            assert torch.equal(gpu.forward(xg), fused), (knob, val)
    print("%s %dx%d: max |dp| %.2e (8-row tiles everywhere: %.2e, 16-row wherever possible: %.2e, separate head: %.2e, fused vs separate head %.2e)"
          % (mode, shape[0], shape[1], err, err8, err16, errsep, dhead))
    assert err < tol and err8 < tol and err16 < tol and errsep < tol and dhead < tol


def test_two_steps_per_barrier_means_three():
    """TIP_UNET_SPB=2 named a schedule that is retired: every value above 1 now selects the three-step one (include/tissue_hip.h),
    so the pass is the default pass, bit for bit -- and not the one-step schedule's flavour or a refused launch."""
    import torch
    from tissue_image_processing_amd import prediction_local as pl, _lib
    gpu = pl._UNet(2, torch.device("cuda", 0), dtype=torch.float32, seed=7)
    gpu.randomize_statistics(9)
    xg = torch.from_numpy(np.random.default_rng(128).random((1, 2, 128, 512))).to("cuda").float()
    assert gpu.hip_path_ok(xg)
    default = gpu.forward(xg)
    with _lib.tuning(TIP_UNET_SPB="2"):
        assert torch.equal(gpu.forward(xg), default)
    assert gpu.last_mode == "f16x3"


def _bench_like_image(N, M, seed):
    from tissue_image_processing_amd import synthetic
    sites = synthetic.make_sites(N, M, seed=seed)[0]
    d1, d2, i1 = synthetic._two_nearest(sites, N, M)
    rng = np.random.default_rng(seed)
    zo = 3000 * np.exp(-(d2 - d1) ** 2 / 4) + rng.poisson(100, (N, M))
    atoh = 1500 * (i1 % 3 == 0) + rng.poisson(100, (N, M))
    return np.stack([atoh, zo]).astype(np.float64)


def test_network_arithmetic_at_headline_size(arith):
    """BASELINE config 3's network at size (2048 x 2048, the bench's kind of frame, biases and non-identity BatchNorm statistics in
    every layer): the default mode (f16x3) against the six-product float32-equivalent mode (bf16x6: different tile flavour, piece
    format and product count) and against MIOpen's float32 convolutions -- max |dp| <= 1e-5 between the two float32-equivalent
    hand-written modes (north_star's float tolerance), 1e-4 against MIOpen (its own float32 summation order); thresholded-pixel
    flips at 0.1 and the agreement of the label maps the tail makes from each are reported, and asserted small.  Also exercises what
    only the full grid does: every tile flavour at full grid size, the XCD workgroup order, halo windows far into multi-GB tensors."""
    import torch
    from tissue_image_processing_amd import prediction_local as pl
    N = 2048
    img = _bench_like_image(N, N, 6)
    pred = pl.SegmentationPredictor(None, img.shape)
    pred.model.randomize_statistics(2)
    padded, _ = pred.prepare_image(img)
    arith("f16x3")
    pred.model.calibrate_head(padded, 0.5)
    probs, labels = {}, {}
    for mode in ("f16x3", "bf16x6", "bf16x3", "miopen"):
        arith(mode)
        p = pred.model.forward(padded)
        assert pred.model.last_mode == mode
        probs[mode] = p[0, 0].clone()
        lab, _ = pred.segment_probability(probs[mode], return_device=True)
        labels[mode] = lab.clone()
        del p
    frac = float((probs["f16x3"] > 0.1).float().mean())
    assert 0.3 < frac < 0.7
    report = {}
    for mode in ("bf16x6", "bf16x3", "miopen"):
        dmax = float((probs["f16x3"] - probs[mode]).abs().max())
        flips = int(((probs["f16x3"] > 0.1) != (probs[mode] > 0.1)).sum())
        same = float((labels["f16x3"] == labels[mode]).float().mean())
        fg_a, fg_b = labels["f16x3"] > 0, labels[mode] > 0
        iou = float((fg_a & fg_b).sum()) / float((fg_a | fg_b).sum())
        report[mode] = (dmax, flips, same, iou)
        print("2048^2 f16x3 vs %s: max |dp0| %.2e, thresholded pixels that differ %d of %d, identical label pixels %.6f, foreground IoU %.6f"
              % (mode, dmax, flips, N * N, same, iou))
    d36 = float((probs["bf16x3"] - probs["bf16x6"]).abs().max())
    print("2048^2 bf16x3 vs bf16x6: max |dp0| %.2e" % d36)
    assert report["bf16x6"][0] <= 1e-5                       # the headline mode is float32-equivalent at size
    # (the calibrated head puts the MEDIAN pixel on the threshold, the worst case for flips: a few per million differences of 1e-6)
    assert report["bf16x6"][1] <= N * N * 1e-5 and report["bf16x6"][3] > 0.999
    assert report["miopen"][0] <= 1e-4 and report["miopen"][1] <= N * N * 1e-4 and report["miopen"][3] > 0.995
    assert d36 <= 1e-4                                       # (the 16-significand-bit mode: its own bound, reported)


def test_network_beyond_4gb_tensors(arith):
    """A 4096 x 2048 frame: the 128-channel tensors are 4.3 GB (two planes of 2.1 GB), beyond what one 32-bit buffer resource
    addresses -- the kernels address a tile's halo WINDOW, so the hand-written path takes any size (round 3 sent such frames to
    MIOpen).  Checked against MIOpen's float32 convolutions (1e-4) and the six-product mode (1e-5)."""
    import torch
    from tissue_image_processing_amd import prediction_local as pl
    H, W = 4096, 2048
    img = _bench_like_image(W, H, 12)            # (C, Y, X) = (2, 2048, 4096) -> network input (X', Y') = (4096, 2048)
    pred = pl.SegmentationPredictor(None, img.shape)
    pred.model.randomize_statistics(5)
    padded, _ = pred.prepare_image(img)
    assert tuple(padded.shape) == (1, 2, H, W)
    arith("f16x3")
    assert pred.model.hip_path_ok(padded)
    pred.model.calibrate_head(padded, 0.5)
    p_h = pred.model.forward(padded)[0, 0].clone()
    assert pred.model.last_mode == "f16x3"
    arith("bf16x6")
    p_6 = pred.model.forward(padded)[0, 0].clone()
    arith("miopen")
    p_m = pred.model.forward(padded)[0, 0].clone()
    d6, dm = float((p_h - p_6).abs().max()), float((p_h - p_m).abs().max())
    # the far corner and the rows around the 2^32-byte offsets of the level-1 tensors, explicitly
    rows = [0, 1, 2047, 2048, 2049, 4094, 4095]
    dr = float((p_h[rows] - p_6[rows]).abs().max())
    print("4096x2048: f16x3 vs bf16x6 max |dp0| %.2e (rows at the 4 GB line %.2e), vs MIOpen float32 %.2e" % (d6, dr, dm))
    assert d6 <= 1e-5 and dm <= 1e-4
