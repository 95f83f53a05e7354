"""GPU: the fp32 (config C2) kernels through the C ABI against float64 on the operands as stored, EVERY element, at the bound of
tests/f32_parity.py: |got - y64| <= c_bar 2^-24 mag, c_bar of every case from the CPU (the sequential fp32 chain of the case's own
products for the direct kernels; the fp32 Winograd emulation over its eight orders, in units of the Winograd magnitude, for the
Winograd kernels), doubled, asserted under the derived cap.  Per-channel scales are log-uniform over [1e-2, 1e1] with random sign.
Shapes: the lists of the `_matches_torch` tests in tests/test_kernels_gpu.py, nothing larger.  Every case prints one line:
excess (units) <= c_bar <= cap."""
import numpy as np
import pytest
import torch

from tests import f32_parity as fp

pytestmark = pytest.mark.gpu


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


# ----------------------------------------------------------------------------- cadre_gemm_f32: dense, every operand mode and tile
GEMM_SHAPES = [(200, 136, 544), (77, 50, 64), (300, 64, 96), (64, 2120, 544), (5, 33, 128), (300, 200, 544), (70, 300, 96), (300, 100, 160)]
GEMM_TILES = [0, 1, 2, 3, 4, 5, 6, 8, 9, 10]          # (0 = auto; test_gemm_modes lists 1, 2, 3, 8, 9, 10 and auto; 7 is bf16-only)


@pytest.mark.parametrize("a_mode,b_mode", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
def test_gemm_modes_every_tile(hip, M, N, K, a_mode, b_mode):
    """The shapes of test_gemm_modes x 4 operand modes x tiles 1 - 6, 8 - 10 and auto: scale, shift, residual, leaky ReLU 0.1.  ldc = N + 3
    (scalar epilogue) and, where N % 4 == 0, ldc = N + 4 (vector epilogue): the padding columns stay as filled."""
    if a_mode == 1 and M % 4:
        M += 4 - M % 4
    if b_mode == 1 and N % 4:
        N += 4 - N % 4
    r = np.random.RandomState(M * 7 + N + a_mode * 2 + b_mode)
    A, B = _randn(r, (M, K)), _randn(r, (N, K))
    sc, sh, res = fp.log_scales(r, N), _randn(r, (N,)), _randn(r, (M, N))
    acc, mac = fp.dense_acc(A, B)
    y, mag = fp.epilogue32(acc, mac, sc, sh, res, 2, 0.1)
    tag = "gemm_f32 %dx%dx%d a_mode %d b_mode %d" % (M, N, K, a_mode, b_mode)
    cb, cap = fp.c_bar_direct([fp.dense_products(A, B)], y, mag, sc, sh, res, 2, 0.1, what=tag)
    Ad = dev(A if a_mode == 0 else A.t().contiguous())
    Bd = dev(B if b_mode == 0 else B.t().contiguous())
    scd, shd, rd = dev(sc), dev(sh), dev(res)
    for tile in GEMM_TILES:
        for pad in (3, 4) if N % 4 == 0 else (3,):
            out = torch.full((M, N + pad), 7.0, device="cuda")
            hip.gemm(Ad, Bd, out, M, N, K, K if a_mode == 0 else M, K if b_mode == 0 else N, N + pad, a_mode, b_mode,
                     scale=scd, shift=shd, resid=rd, ldr=N, act=2, slope=0.1, tile=tile)
            torch.cuda.synchronize()
            o = out.cpu()
            assert bool((o[:, N:] == 7.0).all()), "%s tile %d: ldc padding written" % (tag, tile)
            fp.check32(o[:, :N], y, mag, cb, cap, what="%s tile %d ldc N+%d" % (tag, tile, pad))


@pytest.mark.parametrize("Cin,Cout,H,W,k,s,p,tile", [(64, 64, 18, 22, 3, 1, 1, 0), (64, 128, 18, 22, 3, 2, 1, 0),
                                                      (64, 128, 17, 21, 1, 2, 0, 0), (128, 160, 9, 9, 1, 1, 0, 0),
                                                      (4, 64, 30, 36, 7, 2, 3, 0), (128, 256, 18, 18, 3, 1, 1, 8),
                                                      (4, 64, 30, 36, 7, 2, 3, 8), (64, 64, 18, 22, 3, 1, 1, 10),
                                                      (4, 64, 30, 36, 7, 2, 3, 10), (128, 256, 10, 13, 3, 2, 1, 9),
                                                      ab(64, 64, 18, 22, 3, 1, 1, 12), ab(4, 64, 30, 36, 7, 2, 3, 12), ab(64, 128, 17, 21, 1, 2, 0, 12)])
def test_gemm_implicit_conv(hip, Cin, Cout, H, W, k, s, p, tile):
    """The list of test_conv_implicit_gemm: a_mode 2, and the Cin = 4 stem in a_mode 3; scale, shift, residual, ReLU."""
    from cadre_amd.encoder import _khwc
    r = np.random.RandomState(Cin + Cout + k + tile)
    Nimg = 3
    x = _randn(r, (Nimg, H, W, Cin))
    w = _randn(r, (Cout, Cin, k, k), 1.0 / (Cin * k * k) ** 0.5)
    sc, sh = fp.log_scales(r, Cout), _randn(r, (Cout,))
    acc, mac = fp.conv_acc(x, w, s, p)
    Ho, Wo = acc.shape[1], acc.shape[2]
    res = _randn(r, (Nimg, Ho, Wo, Cout))
    y, mag = fp.epilogue32(acc, mac, sc, sh, res, 1)
    tag = "gemm_f32 a_mode %d %d->%d %dx%d k%d s%d tile %d" % (3 if Cin == 4 else 2, Cin, Cout, H, W, k, s, tile)
    cb, cap = fp.c_bar_direct([fp.conv_products(x, w, s, p)], y, mag, sc, sh, res, 1, what=tag)
    wd = dev(_khwc(w))
    K = wd.shape[1]
    out = torch.full((Nimg, Ho, Wo, Cout), float("nan"), device="cuda")
    hip.gemm(dev(x), wd, out, Nimg * Ho * Wo, Cout, K, 0, K, Cout, a_mode=3 if Cin == 4 else 2, scale=dev(sc), shift=dev(sh),
             resid=dev(res), ldr=Cout, act=1, conv=(H, W, Cin, Ho, Wo, k, k, s, p), tile=tile)
    torch.cuda.synchronize()
    fp.check32(out.cpu(), y, mag, cb, cap, what=tag)


def test_gemm_batched_with_shared_a(hip):
    """The batched case of test_gemm_batched_and_splitk: 8 products, A shared by groups of 4 (z // 4), per-z bias."""
    r = np.random.RandomState(3)
    Z, M, N, K = 8, 96, 160, 544
    A, B, bias = _randn(r, (2, M, K)), _randn(r, (Z, N, K)), _randn(r, (Z, N))
    out = torch.full((Z, M, N), float("nan"), device="cuda")
    hip.gemm(dev(A), dev(B), out, M, N, K, K, K, N, shift=dev(bias), batch=Z, a_z=(4, 0, M * K), b_z=(1, 0, N * K),
             c_z=(1, 0, M * N), s_z=(1, 0, N))
    torch.cuda.synchronize()
    got = out.cpu()
    for z in range(Z):
        acc, mac = fp.dense_acc(A[z // 4], B[z])
        y, mag = fp.epilogue32(acc, mac, None, bias[z])
        tag = "gemm_f32 batched z=%d (A %d)" % (z, z // 4)
        cb, cap = fp.c_bar_direct([fp.dense_products(A[z // 4], B[z])], y, mag, None, bias[z], what=tag)
        fp.check32(got[z], y, mag, cb, cap, what=tag)


def test_gemm_splitk_slabs_and_reduce(hip):
    """K = 4608 in 6 slabs + cadre_splitk_reduce with bias and leaky ReLU 0.01 (test_gemm_batched_and_splitk)."""
    r = np.random.RandomState(4)
    M, N, K, S = 40, 200, 4608, 6
    A, B, bias = _randn(r, (M, K)), _randn(r, (N, K), 0.05), _randn(r, (N,))
    acc, mac = fp.dense_acc(A, B)
    y, mag = fp.epilogue32(acc, mac, None, bias, None, 2, 0.01)
    tag = "gemm_f32 split-K %d + splitk_reduce %dx%dx%d" % (S, M, N, K)
    cb, cap = fp.c_bar_direct([fp.dense_products(A, B)], y, mag, None, bias, None, 2, 0.01, what=tag)
    slabs = torch.full((S, M, N), float("nan"), device="cuda")
    hip.gemm(dev(A), dev(B), slabs, M, N, K, K, K, N, split_k=S)
    out = torch.full((M, N), float("nan"), device="cuda")
    bd = dev(bias)
    hip.check(hip.lib().cadre_splitk_reduce(slabs.data_ptr(), S, M * N, N, out.data_ptr(), N, M, N, None, bd.data_ptr(), 2, 0.01, None, 0,
                                            hip.stream()), "cadre_splitk_reduce")
    torch.cuda.synchronize()
    fp.check32(out.cpu(), y, mag, cb, cap, what=tag)


def test_gemm_batched_splitk_dh_shape(hip):
    """dh_{t-1} = dG_t . W_hh (test_gemm_batched_splitk): 8 nets, [24, 544] outputs, K = 2120, b_mode 1, 8 split-K slabs + reduce."""
    r = np.random.RandomState(8)
    Z, M, N, K, S = 8, 24, 544, 2120, 8
    A, Wt = _randn(r, (Z, M, K), 0.1), _randn(r, (Z, K, N), 0.1)
    slabs = torch.full((S, Z, M, N), float("nan"), device="cuda")
    hip.gemm(dev(A), dev(Wt), slabs, M, N, K, K, N, N, b_mode=1, batch=Z, a_z=(1, 0, M * K), b_z=(1, 0, K * N), c_z=(1, 0, M * N), split_k=S)
    out = torch.full((Z, M, N), float("nan"), device="cuda")
    hip.check(hip.lib().cadre_splitk_reduce(slabs.data_ptr(), S, Z * M * N, N, out.data_ptr(), N, Z * M, N, None, None, 0, 0.0, None, 0,
                                            hip.stream()), "cadre_splitk_reduce")
    torch.cuda.synchronize()
    got = out.cpu()
    for z in range(Z):
        Bz = Wt[z].t().contiguous()
        acc, mac = fp.dense_acc(A[z], Bz)
        y, mag = fp.epilogue32(acc, mac)
        tag = "gemm_f32 batched split-K dh z=%d" % z
        cb, cap = fp.c_bar_direct([fp.dense_products(A[z], Bz)], y, mag, what=tag)
        fp.check32(got[z], y, mag, cb, cap, what=tag)


# ----------------------------------------------------------------------------- Winograd
def _wino_inputs(r, Fn, H, W, Cin, N, use_resid):
    x = _randn(r, (Fn, H, W, Cin))
    w = _randn(r, (N, Cin, 3, 3), 1.0 / (9 * Cin) ** 0.5)
    sc, sh = fp.log_scales(r, N), _randn(r, (N,))
    res = _randn(r, (Fn, H, W, N)) if use_resid else None
    return x, w, sc, sh, res


def _line(tag, c):
    print("%s: c_bar %.3f (emulation %.3f), cap %d, mag_w / mag_direct median %.1f max %.1f, %d tiles emulated"
          % (tag, c["c_bar"], c["emu"], c["cap"], c["ratio"][0], c["ratio"][1], len(c["tiles"])))


WINO3_CASES = [(Fn, H, W, Cin, N, ur, act, m) for m in (2, 3, 4, 6)
               for (Fn, H, W, Cin, N, ur, act) in [(3, 9, 9, 64, 128, True, 1), (2, 18, 18, 32, 64, False, 1), (2, 7, 10, 16, 32, True, 17),
                                                   (1, 1, 1, 8, 8, False, 0), (5, 6, 5, 12, 20, True, 0)]] + [(1, 18, 18, 256, 256, True, 1, 6)]


@pytest.mark.parametrize("Fn,H,W,Cin,N,use_resid,act,m", WINO3_CASES)
def test_winograd_three_launch(hip, Fn, H, W, Cin, N, use_resid, act, m):
    """cadre_winograd_in -> batched cadre_gemm_f32 over the (m+2)^2 planes -> cadre_winograd_out: the list of
    test_winograd_conv3x3_matches_torch, and the production use of F(6x6): an 18 x 18 map with 256 -> 256 channels."""
    from cadre_amd.encoder import _winograd_u
    r = np.random.RandomState(Fn * 100 + H + m)
    x, w, sc, sh, res = _wino_inputs(r, Fn, H, W, Cin, N, use_resid)
    u = _winograd_u(w, m)
    tag = "winograd 3-launch F(%dx%d) F=%d %dx%d %d->%d res=%d act=%d" % (m, m, Fn, H, W, Cin, N, use_resid, act)
    c = fp.wino_case(x, w, u, m, sc, sh, res, act, what=tag)
    _line(tag, c)
    P, T = (m + 2) ** 2, Fn * -(-H // m) * -(-W // m)
    V = torch.full((P, T, Cin), float("nan"), device="cuda")
    Mx = torch.full((P, T, N), float("nan"), device="cuda")
    out = torch.full((Fn, H, W, N), float("nan"), device="cuda")
    L = hip.lib()
    xd, ud, scd, shd, rd = dev(x), dev(u), dev(sc), dev(sh), (dev(res) if use_resid else None)
    hip.check(L.cadre_winograd_in(hip.ptr(xd), hip.ptr(V), Fn, H, W, Cin, m, hip.stream()), "cadre_winograd_in")
    hip.gemm(V, ud, Mx, T, N, Cin, Cin, Cin, N, batch=P, a_z=(1, P, T * Cin), b_z=(1, P, N * Cin), c_z=(1, P, T * N))
    hip.check(L.cadre_winograd_out(hip.ptr(Mx), hip.ptr(scd), hip.ptr(shd), hip.ptr(rd), hip.ptr(out), Fn, H, W, N, act, m, hip.stream()),
              "cadre_winograd_out")
    torch.cuda.synchronize()
    fp.check32(out.cpu(), c["y"], c["mag"], c["c_bar"], c["cap"], what=tag)


@pytest.mark.parametrize("Fn,H,W,use_resid,act", [(3, 72, 72, True, 1), (2, 21, 21, False, 1), (5, 7, 10, True, 0), (1, 1, 1, False, 1),
                                                  (40, 9, 13, True, 1), (300, 6, 6, False, 1)])
def test_winograd_c64(hip, Fn, H, W, use_resid, act):
    """cadre_winograd_c64 (fused F(2x2), 64 -> 64): the list of test_winograd_c64_fused_matches_torch; the ruler from the kernel's own U
    layout, un-permuted."""
    from cadre_amd.encoder import _winograd_u_c64
    r = np.random.RandomState(Fn * 100 + H)
    x, w, sc, sh, res = _wino_inputs(r, Fn, H, W, 64, 64, use_resid)
    u8 = _winograd_u_c64(w)
    tag = "winograd_c64 F=%d %dx%d res=%d act=%d" % (Fn, H, W, use_resid, act)
    c = fp.wino_case(x, w, fp.u_from_c64(u8), 2, sc, sh, res, act, what=tag)
    _line(tag, c)
    out = torch.full((Fn, H, W, 64), float("nan"), device="cuda")
    xd, ud, scd, shd, rd = dev(x), dev(u8), dev(sc), dev(sh), (dev(res) if use_resid else None)
    hip.check(hip.lib().cadre_winograd_c64(hip.ptr(xd), hip.ptr(ud), hip.ptr(scd), hip.ptr(shd), hip.ptr(rd), hip.ptr(out), Fn, H, W, act,
                                           hip.stream()), "cadre_winograd_c64")
    torch.cuda.synchronize()
    fp.check32(out.cpu(), c["y"], c["mag"], c["c_bar"], c["cap"], what=tag)


def _fused_run(hip, x, ud, scd, shd, res, Fb, H, W, Cin, N, act, m):
    L = hip.lib()
    assert L.cadre_winograd_fused_capable(Fb, H, W, Cin, N, m) == 1
    V = torch.full((int(L.cadre_winograd_frag_elems(Fb, H, W, Cin, m)),), float("nan"), device="cuda")      # padding tiles: NaN
    out = torch.full((Fb, H, W, N), float("nan"), device="cuda")
    hip.winograd_fused(dev(x), V, ud, scd, shd, None if res is None else dev(res), out, Fb, H, W, Cin, N, act, m)
    torch.cuda.synchronize()
    return out


FUSED_CASES = [(Fn, H, W, Cin, N, ur, act, m) for m in (2, 3, 4)
               for (Fn, H, W, Cin, N, ur, act) in [(3, 9, 9, 64, 128, True, 1), (2, 18, 18, 32, 64, False, 1), (2, 7, 10, 32, 32, True, 17),
                                                   (1, 1, 1, 32, 32, False, 0), (5, 6, 5, 96, 160, True, 0), (9, 36, 36, 128, 128, True, 1),
                                                   (2, 36, 36, 128, 128, True, 1)]]


@pytest.mark.parametrize("Fn,H,W,Cin,N,use_resid,act,m", FUSED_CASES)
def test_winograd_fused(hip, Fn, H, W, Cin, N, use_resid, act, m):
    """cadre_winograd_in_frag -> cadre_winograd_gemm_out with NaN-padded V: the list of test_winograd_fused_matches_torch, and two frames of
    36 x 36 x 128 -> 128, which take the 16-tile item shape alone and the 64-tile shape inside a larger batch: the bound on both,
    and the same bits."""
    from cadre_amd.encoder import _winograd_u_frag
    r = np.random.RandomState(Fn * 100 + H + m)
    x, w, sc, sh, res = _wino_inputs(r, Fn, H, W, Cin, N, use_resid)
    uf = _winograd_u_frag(w, m)
    tag = "winograd fused F(%dx%d) F=%d %dx%d %d->%d res=%d act=%d" % (m, m, Fn, H, W, Cin, N, use_resid, act)
    c = fp.wino_case(x, w, fp.u_from_frag(uf, m, N, Cin), m, sc, sh, res, act, what=tag)
    _line(tag, c)
    ud, scd, shd = dev(uf), dev(sc), dev(sh)
    got = _fused_run(hip, x, ud, scd, shd, res, Fn, H, W, Cin, N, act, m)
    fp.check32(got.cpu(), c["y"], c["mag"], c["c_bar"], c["cap"], what=tag)
    if (Fn, H) != (2, 36):
        return
    L = hip.lib()
    tiles = lambda Fb: Fb * -(-H // m) * -(-W // m)
    assert L.cadre_winograd_fused_ntb(tiles(Fn), N) == 1
    big = next(Fb for Fb in (8, 16, 32, 64, 128) if L.cadre_winograd_fused_ntb(tiles(Fb), N) == 4)
    xb, rb = _randn(r, (big, H, W, Cin)), _randn(r, (big, H, W, N))
    xb[big - 3:big - 1], rb[big - 3:big - 1] = x, res
    gb = _fused_run(hip, xb, ud, scd, shd, rb, big, H, W, Cin, N, act, m)[big - 3:big - 1]
    fp.check32(gb.cpu(), c["y"], c["mag"], c["c_bar"], c["cap"], what=tag + " inside F=%d (64-tile items)" % big)
    assert torch.equal(gb, got), "%s: the 16-tile and the 64-tile item shapes give different bits" % tag


# ----------------------------------------------------------------------------- cadre_conv3x3_ring, fp32 operands
@pytest.mark.parametrize("Fn,H,W,Cin,N,use_resid,act", [
    (2, 18, 22, 64, 64, False, 1), (1, 72, 72, 64, 64, True, 1), (2, 36, 36, 128, 128, True, 1), (3, 18, 18, 256, 256, True, 1),
    (5, 9, 9, 512, 512, False, 1), (5, 9, 9, 512, 128, False, 1), (7, 9, 9, 128, 128, True, 1 | 16), (2, 21, 21, 64, 96, True, 0),
    (40, 9, 9, 128, 256, True, 1), (260, 9, 9, 256, 128, True, 1), (9, 30, 26, 64, 64, True, 1), (3, 50, 50, 128, 128, False, 1),
    (3, 60, 60, 128, 128, True, 1), (2, 36, 36, 64, 128, True, 1), (2, 30, 30, 128, 64, True, 1), (2, 20, 20, 128, 192, False, 0)])
def test_conv3x3_ring_f32(hip, Fn, H, W, Cin, N, use_resid, act):
    """The list of test_conv3x3_ring with fp32 operands, an fp32 residual before / after the ReLU, fp32 out."""
    from cadre_amd.encoder import _ring_w
    r = np.random.RandomState(Fn * 131 + H * 7 + Cin + N)
    x = _randn(r, (Fn, H, W, Cin))
    w = _randn(r, (N, Cin, 3, 3), 1.5 / np.sqrt(9 * Cin))
    sc, sh = fp.log_scales(r, N), _randn(r, (N,))
    res = _randn(r, (Fn, H, W, N)) if use_resid else None
    acc, mac = fp.conv_acc(x, w, 1, 1)
    y, mag = fp.epilogue32(acc, mac, sc, sh, res, act)
    tag = "ring f32 F=%d %dx%d %d->%d res=%d act=%d" % (Fn, H, W, Cin, N, use_resid, act)
    cb, cap = fp.c_bar_direct([fp.conv_products(x, w, 1, 1)], y, mag, sc, sh, res, act, what=tag)
    out = torch.full((Fn, H, W, N), float("nan"), device="cuda")
    hip.conv3x3_ring(dev(x), dev(_ring_w(w, 32)), dev(sc), dev(sh), dev(res) if use_resid else None, out, Fn, H, W, Cin, N, act)
    torch.cuda.synchronize()
    fp.check32(out.cpu(), y, mag, cb, cap, what=tag)


# ----------------------------------------------------------------------------- the fp32 fused front
@pytest.mark.parametrize("H,W,Fn", [(84, 84, 3), (144, 256, 2)])
def test_stem_pool_f32(hip, H, W, Fn):
    """cadre_pack_obs + cadre_stem_pool (bf16 == 0): /255 table -> conv 7x7 / s2 with the BN scale in the epilogue + shift + ReLU ->
    max-pool, test_fused_stem_pool's f32 cases: float64 on the fp32 table values and taps, pool_ref behind it (rounding is monotone:
    the pooled element is the element the float64 maximum picks, to its own bound)."""
    from cadre_amd import synth
    from cadre_amd.encoder import _fold_bn, _stem_taps
    sd = {k: torch.as_tensor(synth.make_tensor(k, s, kd, 7)).float() for k, s, kd in synth.encoder_spec(1, 1)
          if k.startswith("backbone.conv1") or k.startswith("backbone.bn1")}
    sc, sh = _fold_bn(sd, "backbone.bn1", sd["backbone.conv1.bias"])
    w = sd["backbone.conv1.weight"]
    assert hip.lib().cadre_stem_pool_supported(H, W) == 1
    r = np.random.RandomState(H + W)
    rgb = r.randint(0, 256, (Fn, H, W, 3)).astype(np.uint8)
    route = ((r.rand(Fn, W, H) < 0.15) * 255).astype(np.uint8)
    route[Fn - 1] = 0
    lut = torch.from_numpy((np.arange(256) / 255.).astype(np.float32))
    x = torch.zeros(Fn, H, W, 4)
    x[..., :3] = lut[torch.from_numpy(rgb).long()]
    x[..., 3] = torch.from_numpy((route > 0).transpose(0, 2, 1).astype(np.float32))      # agent.py:51-54: the route ends as {0, 1}
    acc, mac = fp.conv_acc(x, w, 2, 3)
    y, mag, cl = fp.epilogue(acc, mac, sc, sh, None, 1)
    tag = "stem_pool f32 %dx%d" % (H, W)
    cb, cap = fp.c_bar_direct([fp.conv_products(x, w, 2, 3)], y, mag, sc, sh, None, 1, what=tag)
    py, pm, _ = fp.pool_ref(y, mag, cl)
    L = hip.lib()
    rgb_d, route_d = dev(rgb), dev(route)
    packed = torch.empty(Fn, H, W, dtype=torch.int32, device="cuda")
    fmax = torch.empty(Fn, dtype=torch.int32, device="cuda")
    hip.check(L.cadre_pack_obs(hip.ptr(rgb_d), hip.ptr(route_d), hip.ptr(packed), None, hip.ptr(fmax), Fn, H, W, None, Fn, hip.stream()),
              "cadre_pack_obs")
    taps, scd, shd = dev(_stem_taps(w, 50)), dev(sc), dev(sh)
    Hp, Wp = py.shape[1], py.shape[2]
    out = torch.full((Fn, Hp, Wp, 64), float("nan"), device="cuda")
    hip.check(L.cadre_stem_pool(hip.ptr(packed), hip.ptr(taps), hip.ptr(scd), hip.ptr(shd), hip.ptr(out), Fn, H, W, 0,
                                Hp * Wp * 64, Wp * 64, 64, 0, hip.stream()), "cadre_stem_pool")
    torch.cuda.synchronize()
    fp.check32(out.cpu(), py, pm, cb, cap, what=tag)
