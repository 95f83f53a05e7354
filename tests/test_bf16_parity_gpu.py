"""GPU: the bf16 (config C3) kernels through the C ABI against float64 on the operands as stored, element by element, at the bound
of tests/bf16_parity.py: half a bf16 ulp plus c_bar units of fp32 accumulation slack, at most 1e-3 of the elements off the
float64 rounding (each by one bf16 step), no rounding bias.  c_bar of every case comes from the strictly sequential fp32 chain
of that case's own sums on the CPU, never from a kernel.  Then the exact statements (the bf16-output attention kernels, the
padded bf16 preprocessing, the bf16 max-pool), and the encoder's own weight preparation and dispatch at the 288 x 288 model's
shapes.  Every case prints one line: excess (units), c_bar, mismatch share, bias."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import bf16_parity as bp

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


def _has_ab():
    from cadre_amd import hip as h
    return h.has_ab_kernels()


needs_ab = pytest.mark.skipif(not _has_ab(), reason="A/B build only (CADRE_BUILD_AB=1)")


def ab(*args):
    return pytest.param(*args, marks=needs_ab)


def dev(x):
    return torch.as_tensor(x).cuda()


@pytest.fixture(scope="module")
def hip():
    from cadre_amd import hip as h
    h.lib()
    return h


def _randn(r, shape, s=1.0):
    return torch.from_numpy((r.standard_normal(shape) * s).astype(np.float32))


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _need_n(numel):
    """The bias statistic wants n >= 10 000: demanded wherever the case is large enough to give it (about a quarter of the
    elements of a ReLU'd map qualify); the small edge shapes of the lists are checked against their own six standard errors."""
    return 10000 if numel >= 100000 else 0


# ----------------------------------------------------------------------------- cadre_conv3x3_ring
RING_SHAPES = [
    (2, 18, 22, 64, 64, False, 1), (1, 72, 72, 64, 64, True, 1), (2, 36, 36, 128, 128, True, 1), (3, 18, 18, 256, 256, True, 1),
    (5, 9, 9, 512, 512, False, 1), (5, 9, 9, 512, 128, False, 1), (7, 9, 9, 128, 128, True, 1 | 16), (2, 21, 21, 64, 96, True, 0),
    (40, 9, 9, 128, 256, True, 1), (260, 9, 9, 256, 128, True, 1), (9, 30, 26, 64, 64, True, 1), (3, 50, 50, 128, 128, False, 1),
    (3, 60, 60, 128, 128, True, 1), (2, 36, 36, 64, 128, True, 1), (2, 30, 30, 128, 64, True, 1), (2, 20, 20, 128, 192, False, 0)]


@pytest.mark.parametrize("Fn,H,W,Cin,N,use_resid,act", RING_SHAPES)
def test_conv3x3_ring_bf16(hip, Fn, H, W, Cin, N, use_resid, act):
    """The shape list of test_conv3x3_ring: bf16 out with / without a bf16 residual, the residual before and after the ReLU, fp32
    out (no residual), the 64 -> 64 weight-stationary kernel — with the scale in the epilogue, and as the encoder calls it:
    scale = NULL and weights prepared as bf16(w * scale)."""
    from cadre_amd.encoder import _ring_w
    r = np.random.RandomState(Fn * 131 + H * 7 + Cin + N)
    x = _randn(r, (Fn, H, W, Cin)).to(BF)
    w32 = _randn(r, (N, Cin, 3, 3), 1.5 / np.sqrt(9 * Cin))
    sc = torch.from_numpy((0.5 + r.rand(N)).astype(np.float32))
    sh = _randn(r, (N,))
    res = _randn(r, (Fn, H, W, N)).to(BF) if use_resid else None
    xd, scd, shd, rd = dev(x), dev(sc), dev(sh), (dev(res) if use_resid else None)
    tag = "ring F=%d %dx%d %d->%d res=%d act=%d" % (Fn, H, W, Cin, N, use_resid, act)
    for folded in (False, True):
        w = (w32 * sc.view(-1, 1, 1, 1)).to(BF) if folded else w32.to(BF)
        s_ref, s_dev = (None, None) if folded else (sc, scd)
        acc, mac = bp.conv_acc(x, w, 1, 1)
        y, mag, cl = bp.epilogue(acc, mac, s_ref, sh, res, act)
        cb = bp.c_bar_of([bp.conv_products(x, w, 1, 1)], y, mag, s_ref, sh, res, act, what=tag)
        wr = _ring_w(w.float(), 64).to(BF).cuda()
        out = torch.full((Fn, H, W, N), 7.0, device="cuda", dtype=BF)
        hip.conv3x3_ring(xd, wr, s_dev, shd, rd, out, Fn, H, W, Cin, N, act)
        torch.cuda.synchronize()
        bp.check(out, y, mag, cb, cl, what=tag + (" folded" if folded else " scale") + " bf16out", need_bias_n=_need_n(y.numel()))
        if not use_resid:                    # the bf16 model's conv5a / conv5c feed PAM / CAM in fp32
            out32 = torch.full((Fn, H, W, N), 7.0, device="cuda", dtype=torch.float32)
            hip.conv3x3_ring(xd, wr, s_dev, shd, None, out32, Fn, H, W, Cin, N, act)
            torch.cuda.synchronize()
            bp.check(out32, y, mag, cb, cl, out_f32=True, what=tag + (" folded" if folded else " scale") + " f32out")


# ----------------------------------------------------------------------------- cadre_conv3x3_s2 / cadre_conv3x3_s1x
@pytest.mark.parametrize("Nimg,H,W,Cin,Cout,act", [(3, 18, 18, 64, 128, 1), (2, 36, 36, 128, 256, 1), (5, 8, 12, 64, 64, 0),
                                                   (1, 2, 2, 64, 32, 1), (7, 10, 6, 256, 160, 1), (2, 72, 72, 64, 128, 1),
                                                   (9, 6, 4, 192, 512, 0)])
def test_conv3x3_s2_bf16(hip, Nimg, H, W, Cin, Cout, act):
    from cadre_amd.encoder import _s2_w
    r = np.random.RandomState(Nimg * 1000 + H * 10 + Cin + Cout)
    x = _randn(r, (Nimg, H, W, Cin)).to(BF)
    sc = torch.from_numpy((0.5 + r.rand(Cout)).astype(np.float32))
    sh = _randn(r, (Cout,))
    w = (_randn(r, (Cout, Cin, 3, 3), 1.5 / np.sqrt(9 * Cin)) * sc.view(-1, 1, 1, 1)).to(BF)      # the fold of cadre_amd/encoder.py
    acc, mac = bp.conv_acc(x, w, 2, 1)
    y, mag, cl = bp.epilogue(acc, mac, None, sh, None, act)
    tag = "s2 F=%d %dx%d %d->%d act=%d" % (Nimg, H, W, Cin, Cout, act)
    cb = bp.c_bar_of([bp.conv_products(x, w, 2, 1)], y, mag, None, sh, None, act, what=tag)
    assert hip.lib().cadre_conv3x3_s2_supported(Nimg, H, W, Cin, Cout) == 1
    out = torch.full(tuple(y.shape), float("nan"), device="cuda", dtype=BF)
    hip.conv3x3_s2(dev(x), dev(_s2_w(w.float())).to(BF), None, dev(sh), out, Nimg, H, W, Cin, Cout, act)
    torch.cuda.synchronize()
    bp.check(out, y, mag, cb, cl, what=tag, need_bias_n=_need_n(y.numel()))


@pytest.mark.parametrize("Nimg,H,W,C1,Cd,Cout", [(3, 9, 9, 128, 64, 128), (2, 18, 18, 256, 128, 256), (5, 4, 6, 64, 64, 64),
                                                 (1, 1, 2, 128, 64, 32), (7, 5, 3, 256, 128, 160), (2, 36, 36, 128, 64, 128),
                                                 (3, 9, 9, 512, 256, 512), (4, 7, 46, 128, 128, 96), (3, 18, 18, 128, 0, 128),
                                                 (2, 36, 36, 64, 0, 64)])
def test_conv3x3_s1x_bf16(hip, Nimg, H, W, C1, Cd, Cout):
    """Including Cd == 0 (no shortcut) and Cd == C1 (a shortcut k-tile behind every chunk)."""
    from cadre_amd.encoder import _s1x_w
    r = np.random.RandomState(Nimg * 1000 + H * 10 + C1 + Cout)
    t = _randn(r, (Nimg, H, W, C1)).to(BF)
    x2 = _randn(r, (Nimg, 2 * H, 2 * W, max(Cd, 1))).to(BF)
    w2 = _randn(r, (Cout, C1, 3, 3), 1.5 / np.sqrt(9 * C1)).to(BF)
    wd = _randn(r, (Cout, Cd, 1, 1), 1.5 / np.sqrt(max(Cd, 1))).to(BF)
    sh = _randn(r, (Cout,))
    acc, mac = bp.conv_acc(t, w2, 1, 1)
    groups = [bp.conv_products(t, w2, 1, 1)]
    if Cd:
        a2, m2 = bp.shortcut_acc(x2, wd)
        acc, mac = acc + a2, mac + m2
        groups.append(bp.conv_products(x2, wd, 2, 0))
    y, mag, cl = bp.epilogue(acc, mac, None, sh, None, 1)
    tag = "s1x F=%d %dx%d C1=%d Cd=%d ->%d" % (Nimg, H, W, C1, Cd, Cout)
    cb = bp.c_bar_of(groups, y, mag, None, sh, None, 1, what=tag)
    assert hip.lib().cadre_conv3x3_s1x_supported(Nimg, H, W, C1, Cd, Cout) == 1
    out = torch.full(tuple(y.shape), float("nan"), device="cuda", dtype=BF)
    hip.conv3x3_s1x(dev(t), dev(x2) if Cd else None, dev(_s1x_w(w2.float(), wd.float())).to(BF), dev(sh), out, Nimg, H, W, C1, Cd, Cout, 1)
    torch.cuda.synchronize()
    bp.check(out, y, mag, cb, cl, what=tag, need_bias_n=_need_n(y.numel()))


# ----------------------------------------------------------------------------- cadre_gemm_bf16
@pytest.mark.parametrize("M,N,K,tile", [(300, 256, 512, 1), (70, 64, 192, 3), (600, 128, 4608, 4), (200, 64, 576, 2),
                                        (300, 64, 576, 10), (600, 128, 320, 11),
                                        (700, 512, 1152, 7), (256, 256, 64, 7)])
def test_gemm_bf16_dense(hip, M, N, K, tile):
    """Shapes and tiles of test_kernels_gpu.py::test_gemm_bf16_dense: scale, shift, bf16 residual, ReLU; bf16 out (flags 6) and fp32
    out (flags 4)."""
    r = np.random.RandomState(M + N)
    A, B = _randn(r, (M, K)).to(BF), _randn(r, (N, K), 1.5 / np.sqrt(K)).to(BF)
    sc = torch.from_numpy((0.5 + r.rand(N)).astype(np.float32))
    sh = _randn(r, (N,))
    res = _randn(r, (M, N)).to(BF)
    acc, mac = bp.dense_acc(A, B)
    y, mag, cl = bp.epilogue(acc, mac, sc, sh, res, 1)
    tag = "gemm_bf16 dense %dx%dx%d tile %d" % (M, N, K, tile)
    cb = bp.c_bar_of([bp.dense_products(A, B)], y, mag, sc, sh, res, 1, what=tag)
    Ad, Bd, rd, scd, shd = dev(A), dev(B), dev(res), dev(sc), dev(sh)
    out32 = torch.zeros(M, N, device="cuda")
    hip.gemm(Ad, Bd, out32, M, N, K, K, K, N, scale=scd, shift=shd, resid=rd, ldr=N, act=1, tile=tile, bf16=True, flags=4)
    torch.cuda.synchronize()
    bp.check(out32, y, mag, cb, cl, out_f32=True, what=tag + " flags=4")
    out16 = torch.zeros(M, N, device="cuda", dtype=BF)
    hip.gemm(Ad, Bd, out16, M, N, K, K, K, N, scale=scd, shift=shd, resid=rd, ldr=N, act=1, tile=tile, bf16=True, flags=6)
    torch.cuda.synchronize()
    bp.check(out16, y, mag, cb, cl, what=tag + " flags=6", need_bias_n=_need_n(y.numel()))


@pytest.mark.parametrize("Cin,Cout,H,W,k,s,p,tile", [(64, 64, 18, 22, 3, 1, 1, 0), (64, 128, 18, 22, 3, 2, 1, 0),
                                                      (64, 128, 17, 21, 1, 2, 0, 0), (512, 128, 9, 9, 3, 1, 1, 0),
                                                      (256, 256, 18, 18, 3, 1, 1, 7), (128, 512, 9, 9, 1, 1, 0, 7),
                                                      ab(64, 64, 18, 22, 3, 1, 1, 12), ab(128, 192, 11, 9, 3, 2, 1, 12)])
def test_gemm_bf16_implicit_conv(hip, Cin, Cout, H, W, k, s, p, tile):
    """a_mode 2 (shapes of test_conv_bf16): 1x1 and 3x3, stride 1 and 2, with a bf16 residual; bf16 out and fp32 out."""
    r = np.random.RandomState(Cin + Cout + k + 1)
    Nimg = 3
    x = _randn(r, (Nimg, H, W, Cin)).to(BF)
    w = _randn(r, (Cout, Cin, k, k), 1.5 / np.sqrt(Cin * k * k)).to(BF)
    sc = torch.from_numpy((0.5 + r.rand(Cout)).astype(np.float32))
    sh = _randn(r, (Cout,))
    acc, mac = bp.conv_acc(x, w, s, p)
    Ho, Wo = acc.shape[1], acc.shape[2]
    res = _randn(r, (Nimg, Ho, Wo, Cout)).to(BF)
    y, mag, cl = bp.epilogue(acc, mac, sc, sh, res, 1)
    tag = "gemm_bf16 a_mode 2 %d->%d %dx%d k%d s%d tile %d" % (Cin, Cout, H, W, k, s, tile)
    cb = bp.c_bar_of([bp.conv_products(x, w, s, p)], y, mag, sc, sh, res, 1, what=tag)
    xd, wd = dev(x), dev(w.permute(0, 2, 3, 1).reshape(Cout, -1).contiguous())
    K = k * k * Cin
    for flags in (6, 4):
        out = torch.full((Nimg, Ho, Wo, Cout), 7.0, device="cuda", dtype=BF if flags & 2 else torch.float32)
        hip.gemm(xd, wd, out, Nimg * Ho * Wo, Cout, K, 0, K, Cout, a_mode=2, scale=dev(sc), shift=dev(sh), resid=dev(res), ldr=Cout,
                 act=1, conv=(H, W, Cin, Ho, Wo, k, k, s, p), bf16=True, tile=tile, flags=flags)
        torch.cuda.synchronize()
        bp.check(out, y, mag, cb, cl, out_f32=not (flags & 2), what=tag + " flags=%d" % flags, need_bias_n=_need_n(y.numel()) if flags & 2 else 0)


@pytest.mark.parametrize("tile", [3, 10, ab(12)])
def test_gemm_bf16_padded_stem(hip, tile):
    """a_mode 4: the 7x7 / s2 stem on the zero-padded bf16 NHWC4 image, scale and shift in the epilogue, ReLU, bf16 out."""
    from cadre_amd.encoder import _stem_rows_bf16
    r = np.random.RandomState(9)
    Nimg, H, W = 5, 46, 58
    x = _randn(r, (Nimg, H, W, 4)).to(BF)
    x[..., 3] = 0
    w = _randn(r, (64, 4, 7, 7), 1.5 / 14.0).to(BF)
    sc = torch.from_numpy((0.5 + r.rand(64)).astype(np.float32))
    sh = _randn(r, (64,))
    acc, mac = bp.conv_acc(x, w, 2, 3)
    Ho, Wo = acc.shape[1], acc.shape[2]
    y, mag, cl = bp.epilogue(acc, mac, sc, sh, None, 1)
    tag = "gemm_bf16 a_mode 4 padded stem tile %d" % tile
    cb = bp.c_bar_of([bp.conv_products(x, w, 2, 3)], y, mag, sc, sh, None, 1, what=tag)
    Hp, Wp = max(H + 6, (Ho - 1) * 2 + 8), max(W + 6, (Wo - 1) * 2 + 8)
    Wp += Wp & 1
    xp = torch.zeros(Nimg, Hp, Wp, 4, dtype=BF)
    xp[:, 3:3 + H, 3:3 + W] = x
    wd = dev(_stem_rows_bf16(w.float())).to(BF)
    out = torch.full((Nimg, Ho, Wo, 64), 7.0, device="cuda", dtype=BF)
    K = wd.shape[1]
    hip.gemm(dev(xp), wd, out, Nimg * Ho * Wo, 64, K, 0, K, 64, a_mode=4, scale=dev(sc), shift=dev(sh), act=1,
             conv=(Hp, Wp, 4, Ho, Wo, 7, 7, 2, 0), bf16=True, flags=2, tile=tile)
    torch.cuda.synchronize()
    bp.check(out, y, mag, cb, cl, what=tag, need_bias_n=10000)


@pytest.mark.parametrize("M,tile", [(48, 3), (160, 0)])
def test_gemm_bf16_splitk_reduce_as_the_inter_task_first_layer(hip, M, tile):
    """K = 41472 in 16 slices (cadre_gemm_bf16 split_k) + cadre_splitk_reduce with bias and leaky ReLU 0.01: fp32 out, units only.
    Float64 on a sample of 16 rows of M."""
    N, K, split = 1536, 41472, 16
    g = torch.Generator().manual_seed(M)
    A = torch.randn(M, K, generator=g).to(BF)
    B = (torch.randn(N, K, generator=g) * (1.5 / np.sqrt(K))).to(BF)
    bias = torch.randn(N, generator=g) * 0.1
    rows = torch.from_numpy(np.sort(np.random.RandomState(M).choice(M, 16, replace=False)))
    acc, mac = bp.dense_acc(A[rows], B)
    y, mag, cl = bp.epilogue(acc, mac, None, bias, None, 2, 0.01)
    tag = "gemm_bf16 split-K 16 + splitk_reduce M=%d tile %d" % (M, tile)
    cb = bp.c_bar_of([bp.dense_products(A[rows], B)], y, mag, None, bias, None, 2, 0.01, what=tag)
    slabs = torch.full((split, M, N), float("nan"), device="cuda")
    out = torch.full((M, 2 * N), float("nan"), device="cuda")
    bd = dev(bias)
    hip.gemm(dev(A), dev(B), slabs, M, N, K, K, K, N, split_k=split, tile=tile, bf16=True)
    hip.check(hip.lib().cadre_splitk_reduce(hip.ptr(slabs), split, M * N, N, out.data_ptr() + 4 * N, 2 * N, M, N, None, hip.ptr(bd),
                                            2, 0.01, None, 0, hip.stream()), "cadre_splitk_reduce")
    torch.cuda.synchronize()
    assert torch.isnan(out[:, :N]).all()                          # (the other branch's half of `hid` is not touched)
    bp.check(out[:, N:].cpu()[rows], y, mag, cb, cl, out_f32=True, what=tag)


# ----------------------------------------------------------------------------- cadre_stem_pool, bf16 == 1
def _bn_fold(sd, bn, bias=None):
    from cadre_amd.encoder import _fold_bn
    t = {k: torch.as_tensor(v).float() for k, v in sd.items() if k.startswith(bn + ".")}
    return _fold_bn(t, bn, None if bias is None else torch.as_tensor(bias).float())


@pytest.mark.parametrize("H,W,Fn", [(84, 84, 3), (144, 256, 2), (288, 288, 2)])
def test_stem_pool_bf16(hip, H, W, Fn):
    """pack -> /255 -> conv 7x7 / s2 + folded BN + ReLU -> max-pool in one kernel, bf16 form: float64 on the /255 table values
    rounded to bf16 and on the taps bf16(w * scale), plus the shift, ReLU, max-pool.  Rounding is monotone: the pooled value is
    the rounded maximum and owes half an ulp."""
    from cadre_amd import synth
    from cadre_amd.encoder import _stem_taps
    sd = synth.encoder_spec(1, 1)                                  # (only the stem's tensors are needed)
    sd = {k: synth.make_tensor(k, s, kd, 7) for k, s, kd in sd if k.startswith("backbone.conv1") or k.startswith("backbone.bn1")}
    sc, sh = _bn_fold(sd, "backbone.bn1", sd["backbone.conv1.bias"])
    w = (torch.as_tensor(sd["backbone.conv1.weight"]).float() * sc.view(-1, 1, 1, 1)).to(BF)       # one rounding
    assert hip.lib().cadre_stem_pool_supported(H, W) == 1
    r = np.random.RandomState(H + W)
    rgb = r.randint(0, 256, (Fn, H, W, 3)).astype(np.uint8)
    route = ((r.rand(Fn, W, H) < 0.15) * 255).astype(np.uint8)
    route[Fn - 1] = 0
    lut = torch.from_numpy((np.arange(256) / 255.).astype(np.float32)).to(BF)
    x = torch.zeros(Fn, H, W, 4, dtype=BF)
    x[..., :3] = lut[torch.from_numpy(rgb).long()]
    x[..., 3] = torch.from_numpy((route > 0).transpose(0, 2, 1).astype(np.float32)).to(BF)      # agent.py:51-54: the route ends as {0, 1}
    acc, mac = bp.conv_acc(x, w, 2, 3)
    y, mag, cl = bp.epilogue(acc, mac, None, sh, None, 1)
    tag = "stem_pool bf16 %dx%d" % (H, W)
    cb = bp.c_bar_of([bp.conv_products(x, w, 2, 3)], y, mag, None, sh, None, 1, what=tag)
    py, pm, pc = bp.pool_ref(y, mag, cl)
    L = hip.lib()
    rgb_d, route_d = dev(rgb), dev(route)
    packed = torch.empty(Fn, H, W, dtype=torch.int32, device="cuda")
    fmax = torch.empty(Fn, dtype=torch.int32, device="cuda")
    hip.check(L.cadre_pack_obs(hip.ptr(rgb_d), hip.ptr(route_d), hip.ptr(packed), None, hip.ptr(fmax), Fn, H, W, None, Fn,
                               hip.stream()), "cadre_pack_obs")
    taps = dev(_stem_taps(w.float(), 56, row8=True)).to(BF)
    Hp, Wp = py.shape[1], py.shape[2]
    out = torch.full((Fn, Hp, Wp, 64), 7.0, device="cuda", dtype=BF)
    hip.check(L.cadre_stem_pool(hip.ptr(packed), hip.ptr(taps), None, hip.ptr(dev(sh)), hip.ptr(out), Fn, H, W, 1,
                                Hp * Wp * 64, Wp * 64, 64, 0, hip.stream()), "cadre_stem_pool")
    torch.cuda.synchronize()
    bp.check(out, py, pm, cb, pc, what=tag, need_bias_n=10000)


# ----------------------------------------------------------------------------- exact statements
def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


@pytest.mark.parametrize("h,w", [(3, 3), (5, 8), (9, 9), (10, 11), (11, 11), (8, 16), (12, 12), (11, 13), (16, 16), (20, 25)])
def test_pam_cam_bf16out_are_the_fp32_kernels_rounded(hip, h, w):
    """cadre_pam_bf16out / cadre_cam_bf16out ("same kernels writing y as bf16"): the output equals cadre_pam / cadre_cam on the same
    inputs converted with .to(torch.bfloat16), bit for bit, at the ten map sizes of test_pam_cam."""
    g = torch.Generator().manual_seed(h * w)
    Fn, Np = 3, h * w
    xd = dev((torch.randn(Fn, h, w, 128, generator=g) * 0.4).contiguous())
    wqkv = torch.randn(160, 128, generator=g) * 0.1
    bqkv = torch.randn(160, generator=g) * 0.1
    qkv = torch.empty(Fn * Np, 160, device="cuda")
    hip.gemm(xd, dev(wqkv), qkv, Fn * Np, 160, 128, 128, 128, 160, shift=dev(bqkv))
    L, st = hip.lib(), hip.stream()
    y32 = torch.full_like(xd, float("nan"))
    y16 = torch.full_like(xd, float("nan"), dtype=BF)
    hip.check(L.cadre_pam(xd.data_ptr(), qkv.data_ptr(), 0.5, y32.data_ptr(), Fn, Np, st), "cadre_pam")
    hip.check(L.cadre_pam_bf16out(xd.data_ptr(), qkv.data_ptr(), 0.5, y16.data_ptr(), Fn, Np, st), "cadre_pam_bf16out")
    torch.cuda.synchronize()
    assert not torch.isnan(y32).any()
    assert torch.equal(_bits(y16), _bits(y32.to(BF)))
    c32 = torch.full_like(xd, float("nan"))
    c16 = torch.full_like(xd, float("nan"), dtype=BF)
    hip.check(L.cadre_cam(xd.data_ptr(), 0.7, c32.data_ptr(), Fn, Np, st), "cadre_cam")
    hip.check(L.cadre_cam_bf16out(xd.data_ptr(), 0.7, c16.data_ptr(), Fn, Np, st), "cadre_cam_bf16out")
    torch.cuda.synchronize()
    assert not torch.isnan(c32).any()
    assert torch.equal(_bits(c16), _bits(c32.to(BF)))


@pytest.mark.parametrize("H,W", [(84, 84), (144, 256)])
def test_preprocess_bf16pad_is_preprocess_rounded_inside_an_untouched_border(hip, H, W):
    """cadre_preprocess_bf16pad with the encoder's Hp, Wp, 3, 3 (cadre_amd/encoder.py): the interior equals cadre_preprocess's fp32
    output rounded to bf16 in all four channels, route_norm and frame_max equal the fp32 variant's, and a border pre-filled with a
    sentinel bf16 pattern is untouched."""
    Fn = 3
    Ho, Wo = (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1
    Hp, Wp = max(H + 6, (Ho - 1) * 2 + 8), max(W + 6, (Wo - 1) * 2 + 8)
    Wp += Wp & 1
    r = np.random.RandomState(H + W)
    rgb = dev(r.randint(0, 256, (Fn, H, W, 3)).astype(np.uint8))
    route_np = ((r.rand(Fn, W, H) < 0.15) * r.randint(1, 256, (Fn, W, H))).astype(np.uint8)
    route_np[Fn - 1] = 0                                            # a frame whose route maximum is 0
    route = dev(route_np)
    lut = torch.from_numpy((np.arange(256) / 255.).astype(np.float32)).cuda()
    L, st = hip.lib(), hip.stream()
    out32 = torch.full((Fn, H, W, 4), float("nan"), device="cuda")
    rn32 = torch.full((Fn, W, H), 77, dtype=torch.uint8, device="cuda")
    fm32 = torch.full((Fn,), -1, dtype=torch.int32, device="cuda")
    hip.check(L.cadre_preprocess(hip.ptr(rgb), hip.ptr(route), hip.ptr(lut), hip.ptr(out32), hip.ptr(rn32), hip.ptr(fm32), Fn, H, W, st),
              "cadre_preprocess")
    SENT = 0x4B1D                                                    # a bf16 bit pattern no pixel takes (8 486 912.0)
    out16 = torch.full((Fn, Hp, Wp, 4), SENT, dtype=torch.int16, device="cuda")
    rn16 = torch.full((Fn, W, H), 78, dtype=torch.uint8, device="cuda")
    fm16 = torch.full((Fn,), -2, dtype=torch.int32, device="cuda")
    hip.check(L.cadre_preprocess_bf16pad(hip.ptr(rgb), hip.ptr(route), hip.ptr(lut), hip.ptr(out16), hip.ptr(rn16), hip.ptr(fm16),
                                         Fn, H, W, Hp, Wp, 3, 3, st), "cadre_preprocess_bf16pad")
    torch.cuda.synchronize()
    assert not torch.isnan(out32).any()
    got = out16.cpu()
    assert torch.equal(got[:, 3:3 + H, 3:3 + W], _bits(out32.to(BF)))
    assert torch.equal(rn16.cpu(), rn32.cpu()) and torch.equal(fm16.cpu(), fm32.cpu())
    border = torch.ones(Fn, Hp, Wp, 4, dtype=torch.bool)
    border[:, 3:3 + H, 3:3 + W] = False
    assert border.any() and bool((got[border] == SENT).all())


@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("H,W", [(15, 18), (72, 72), (1, 1), (2, 3)])
def test_maxpool3x3s2_bf16_is_exact(hip, H, W, C):
    g = torch.Generator().manual_seed(H * 100 + W + C)
    x = torch.randn(2, H, W, C, generator=g).to(BF)
    want = F.max_pool2d(x.float().permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).contiguous().to(BF)
    xd = dev(x)
    out = torch.full(tuple(want.shape), 7.0, device="cuda", dtype=BF)
    hip.check(hip.lib().cadre_maxpool3x3s2_bf16(xd.data_ptr(), out.data_ptr(), 2, H, W, C, hip.stream()), "cadre_maxpool3x3s2_bf16")
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(want))


# ----------------------------------------------------------------------------- the encoder's own preparation and dispatch, 288 x 288
FRAMES = {72: 48, 36: 192, 18: 256, 9: 512}         # frames per map size: every CU holds several persistent work items


@pytest.fixture(scope="module")
def enc288(hip):
    from cadre_amd import synth
    from cadre_amd.encoder import DANetEncoderHIP
    sd = synth.encoder_state(9, 9, 11)
    enc = DANetEncoderHIP(sd, 288, 288, "cuda:0", max_frames=512, dtype="bf16")
    return enc, {k: torch.as_tensor(v).float() for k, v in sd.items()}


def _sample_frames(Fn):
    return [0, 1, Fn // 2, Fn - 2, Fn - 1]


def _profiled(hip, fn):
    """Run fn() with the launch profile on: -> (result, [profile key + (K of the launch,)])."""
    hip.PROFILE = []
    try:
        res = fn()
        torch.cuda.synchronize()
        keys = [tuple(p[0]) + (p[4][2],) for p in hip.PROFILE]
    finally:
        hip.PROFILE = None
    return res, keys


def _enc_convs():
    """(name, attribute path, state-dict conv, bn or None, input px, resid kind, act override, out_f32)"""
    L = []
    px = 72
    for li in range(1, 5):
        for bi in range(2):
            i = (li - 1) * 2 + bi
            pre = "backbone.layer%d.%d" % (li, bi)
            s2 = li > 1 and bi == 0
            L.append(("b%d.conv1" % i, ("blocks", i, 0), pre + ".conv1", pre + ".bn1", px, False, None, False, 2 if s2 else 1))
            if s2:
                px //= 2
                L.append(("b%d.conv2+shortcut" % i, ("s1x", i), pre, None, px, False, None, False, 1))
            else:
                L.append(("b%d.conv2" % i, ("blocks", i, 1), pre + ".conv2", pre + ".bn2", px, True, None, False, 1))
    hd = "da_head."
    L += [("conv5a", ("conv5a",), hd + "conv5a.0", hd + "conv5a.1", 9, False, None, True, 1),
          ("conv5c", ("conv5c",), hd + "conv5c.0", hd + "conv5c.1", 9, False, None, True, 1),
          ("conv51", ("conv51",), hd + "conv51.0", hd + "conv51.1", 9, False, None, False, 1),
          ("conv52", ("conv52",), hd + "conv52.0", hd + "conv52.1", 9, True, 1 | 16, False, 1),
          ("conv8", ("conv8",), hd + "conv8.1", None, 9, False, None, False, 1),
          ("visual_conv", ("visual_conv",), "visual_conv", None, 9, False, None, False, 1),
          ("bc_conv", ("bc_conv",), "bc_conv", None, 9, False, None, False, 1)]
    return L


@pytest.mark.parametrize("case", _enc_convs(), ids=[c[0] for c in _enc_convs()])
def test_encoder_conv_dispatch_at_production_shapes(hip, enc288, case):
    """Every conv of the bf16 288 x 288 encoder through the encoder's OWN path (enc._conv with the arguments of _trunk; the
    hip.conv3x3_s1x call of _trunk for the down-sampling blocks) on the weights the encoder prepared itself, against
    conv -> BN(eval) -> (+ resid) -> ReLU restated in float64 from the state dict: scale / shift from encoder._fold_bn, the folded
    weight bf16(w * scale) in ONE rounding, for s1x the sum of both shifts.  The kernel runs on all frames (every CU loaded), the
    reference covers the first two, the last two and one in the middle.  The kernel taken is asserted from the launch profile."""
    enc, sd = enc288
    name, path, ck, bnk, px, use_resid, act_o, out_f32, stride = case
    Fn = FRAMES[px]
    fr = _sample_frames(Fn)
    g = torch.Generator(device="cuda").manual_seed(px + len(name))
    Lb = hip.lib()
    enc._pass_frames = Fn
    if path[0] == "s1x":
        i = path[1]
        c1, c2, down = enc.blocks[i]
        t = torch.randn(Fn, px, px, c2.cin, device="cuda", generator=g).to(BF)
        cur = torch.randn(Fn, 2 * px, 2 * px, down.cin, device="cuda", generator=g).to(BF)
        assert i in enc.s1x and enc.use_s1x and Lb.cadre_conv3x3_s1x_supported(Fn, px, px, c2.cin, down.cin, c2.cout) == 1
        w_f, sh_f = enc.s1x[i]
        out = torch.full((Fn, px, px, c2.cout), 7.0, device="cuda", dtype=BF)
        _, keys = _profiled(hip, lambda: hip.conv3x3_s1x(t, cur, w_f, sh_f, out, Fn, px, px, c2.cin, down.cin, c2.cout, 1))
        assert [k[0] for k in keys] == ["s1x"]
        s2_, h2 = _bn_fold(sd, ck + ".bn2")
        sd_, hd_ = _bn_fold(sd, ck + ".downsample.1")
        w2 = (sd[ck + ".conv2.weight"] * s2_.view(-1, 1, 1, 1)).to(BF)
        wd = (sd[ck + ".downsample.0.weight"] * sd_.view(-1, 1, 1, 1)).to(BF)
        shift = h2 + hd_
        tc, cc = t[fr].cpu(), cur[fr].cpu()
        a1, m1 = bp.conv_acc(tc, w2, 1, 1)
        a2, m2 = bp.shortcut_acc(cc, wd)
        y, mag, cl = bp.epilogue(a1 + a2, m1 + m2, None, shift, None, 1)
        cb = bp.c_bar_of([bp.conv_products(tc, w2, 1, 1), bp.conv_products(cc, wd, 2, 0)], y, mag, None, shift, None, 1, what=name)
        bp.check(out[fr], y, mag, cb, cl, what="encoder %s (s1x) F=%d %dpx" % (name, Fn, px), need_bias_n=10000)
        return
    c = enc
    for p in path:
        c = getattr(c, p) if isinstance(p, str) else c[p]
    x = torch.randn(Fn, px, px, c.cin, device="cuda", generator=g).to(BF)
    po = px // stride
    resid = torch.randn(Fn, po, po, c.cout, device="cuda", generator=g).to(BF) if use_resid else None
    (out, Ho, Wo), keys = _profiled(hip, lambda: enc._conv(c, x, Fn, px, px, "parity_" + name, resid=resid, act=act_o, out_f32=out_f32))
    assert (Ho, Wo) == (po, po)
    first = out.clone()
    for rep in range(4):                      # every CU loaded with several persistent items: the same bits on every launch
        out, _, _ = enc._conv(c, x, Fn, px, px, "parity_" + name, resid=resid, act=act_o, out_f32=out_f32)
        assert torch.equal(out, first), "%s: launch %d differs from the first" % (name, rep + 2)
    act = c.act if act_o is None else act_o
    if c.k == 3 and stride == 1:
        flags = 1 | (0 if out_f32 else 2) | (12 if use_resid else 0)
        assert Lb.cadre_conv3x3_ring_supported(Fn, px, px, c.cin, c.cout, flags) == 1
        assert [k[0] for k in keys] == ["ring"] and c.ring_folded
    elif c.k == 3:
        assert Lb.cadre_conv3x3_s2_supported(Fn, px, px, c.cin, c.cout) == 1
        assert [k[0] for k in keys] == ["s2"]
    else:
        assert [k[0] for k in keys] == ["bf16"] and keys[0][2] == 0          # the 1x1 convs: cadre_gemm_bf16, dense
    w = sd[ck + ".weight"]
    if bnk is not None:
        sc, shift = _bn_fold(sd, bnk)
        w = (w * sc.view(-1, 1, 1, 1)).to(BF)
    else:
        w, shift = w.to(BF), sd[ck + ".bias"]
    xc = x[fr].cpu()
    rc = None if resid is None else resid[fr].cpu()
    acc, mac = bp.conv_acc(xc, w, stride, c.pad)
    y, mag, cl = bp.epilogue(acc, mac, None, shift, rc, act)
    cb = bp.c_bar_of([bp.conv_products(xc, w, stride, c.pad)], y, mag, None, shift, rc, act, what=name)
    bp.check(out[fr], y, mag, cb, cl, out_f32=out_f32, what="encoder %s (%s) F=%d %dpx" % (name, keys[0][0], Fn, px),
             need_bias_n=0 if out_f32 else 10000)


@pytest.mark.parametrize("Fn", [128, 8])
def test_encoder_inter_task_first_layer(hip, enc288, Fn):
    """`hid` of the inter-task attention (fp32: units only) after a whole pass, against float64 on the bf16 `ita_w1`, the fp32 bias
    and leaky ReLU 0.01, for a sample of 32 rows.  F = 128 (> 64) takes cadre_gemm_bf16_w128 on the fragment-order matrix of
    _ita_frag, F = 8 takes tile 3 of cadre_gemm_bf16."""
    enc, sd = enc288
    r = np.random.RandomState(Fn)
    rgb = dev(r.randint(0, 256, (Fn, 288, 288, 3)).astype(np.uint8))
    route = dev(((r.rand(Fn, 288, 288) < 0.15) * 255).astype(np.uint8))
    taps = {}
    _, keys = _profiled(hip, lambda: enc.forward_nhwc(enc.preprocess(rgb, route), taps=taps))
    first = [k[:-1] for k in keys if k[-1] == 41472]               # the launches with K = 512 * 81: one per branch
    assert first == ([("gw128",)] * 2 if Fn > 64 else [("bf16", 3, 0)] * 2)
    hid = enc._buf("ita_hid", (Fn, 3072)).cpu()
    rows = torch.from_numpy(np.sort(r.choice(Fn, min(32, Fn), replace=False)))
    for b, nm in enumerate(("vis", "bc")):
        A = taps[nm].reshape(Fn, -1)[rows.cuda()].cpu()
        B = enc.ita_w1[b].cpu()
        ws = []
        for role in ("query", "key", "value"):                    # the documented matrix: NCHW flatten -> NHWC flatten, one rounding
            ws.append(sd["inter_task_att.%s_%s_layer.1.weight" % (("visual", "bc")[b], role)].view(512, 512, 81).permute(0, 2, 1).reshape(512, -1))
        assert torch.equal(_bits(B), _bits(torch.cat(ws).to(BF)))
        bias = torch.cat([sd["inter_task_att.%s_%s_layer.1.bias" % (("visual", "bc")[b], role)] for role in ("query", "key", "value")])
        acc, mac = bp.dense_acc(A, B)
        y, mag, cl = bp.epilogue(acc, mac, None, bias, None, 2, 0.01)
        tag = "encoder inter-task first layer %s F=%d" % (nm, Fn)
        cb = bp.c_bar_of([bp.dense_products(A, B)], y, mag, None, bias, None, 2, 0.01, what=tag)
        bp.check(hid[rows][:, 1536 * b:1536 * (b + 1)], y, mag, cb, cl, out_f32=True, what=tag)
