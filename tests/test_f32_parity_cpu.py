"""The fp32 parity bound of tests/f32_parity.py has teeth: it ACCEPTS the honest results (torch-CPU fp32 direct conv / matmul with the
fp32 epilogue; this module's own fp32 Winograd emulation for every m) and REJECTS every CPU-made mutant — among them two (†) that the
metric of the existing fp32 kernel tests, max|got - ref| / max|ref| < 2e-5 (1e-4 for F(6x6)) against torch-CPU fp32, lets through on
inputs with which the honest result passes that bar too: an error confined to an output channel whose folded scale is small, and one
confined to the partly-outside last tile row.  Every mutant prints the old metric next to its excess.  The Cook-Toom matrices the
ruler is built from satisfy the correlation identity exactly over the rationals.  No GPU."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import f32_parity as fp

MS = [2, 3, 4, 6]
OLD_BAR = {2: 2e-5, 3: 2e-5, 4: 2e-5, 6: 1e-4}           # tests/test_kernels_gpu.py::test_winograd_conv3x3_matches_torch
SMALL_N = 3                                              # the output channel whose scale is 1e-3 of the others
QUIET_C = 5                                              # the input channel whose activations are QUIET of the others
QUIET = {2: 1e-4, 3: 1e-4, 4: 1e-4, 6: 5e-4}


def _conv32(x, w, stride=1, pad=1):
    return F.conv2d(x.permute(0, 3, 1, 2), w, None, stride, pad).permute(0, 2, 3, 1).contiguous()


def _fin(z, c, act=None, scale=None, shift=None):
    """The fp32 epilogue of case c on a conv sum z ([F][H][W][N] array or tensor) -> fp32 tensor."""
    z = z.numpy() if isinstance(z, torch.Tensor) else z
    rn = None if c["resid"] is None else c["resid"].numpy()
    return torch.from_numpy(np.ascontiguousarray(fp.epilogue_np(z.astype(np.float32), c["scale"] if scale is None else scale,
                                                                c["shift"] if shift is None else shift, rn, c["act"] if act is None else act)))


@functools.lru_cache(maxsize=None)
def wino(m, act=1):
    """A map the tiles do not divide (one row / column of the last tile inside), Cin = 128, scales 0.5 ... 1.5 except channel SMALL_N
    (1e-3 of that), input channel QUIET_C quiet: the † inputs."""
    from cadre_amd.encoder import _winograd_u
    g = torch.Generator().manual_seed(100 * m + act)
    Fn, H, W, Cin, N = 2, 2 * m + 1, 2 * m + 1, 128, 32
    x = torch.randn(Fn, H, W, Cin, generator=g)
    x[..., QUIET_C] *= QUIET[m]
    w = torch.randn(N, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5
    scale = 0.5 + torch.rand(N, generator=g)
    scale[SMALL_N] *= 1e-3
    shift = torch.randn(N, generator=g)
    resid = torch.randn(Fn, H, W, N, generator=g)
    Up = _winograd_u(w, m)
    c = fp.wino_case(x, w, Up, m, scale, shift, resid, act, n_tiles=6, what="F(%dx%d)" % (m, m))
    assert len(c["tiles"]) < Fn * 9                       # c_bar from a SAMPLE of the tiles; the results below cover all of them
    c.update(x=x, w=w, U=Up, m=m, scale=scale, shift=shift, resid=resid, act=act, what="F(%dx%d,3x3) %s act %d" % (m, m, (Fn, H, W, Cin, N), act))
    c["z_emu"] = fp.wino_full(x, Up, m, c["D"])           # the honest Winograd conv sum, fp32, all tiles
    c["z32"] = _conv32(x, w).numpy()                      # the honest direct conv sum, torch-CPU fp32
    c["ref32"] = _fin(c["z32"], c)                        # the reference of the existing tests
    return c


@functools.lru_cache(maxsize=None)
def direct(kind):
    """conv: 3x3 / s1 conv (2, 9, 9, 128, 32) with ReLU; dense: 70 x 48 x 544 with leaky ReLU 0.1 (test_gemm_modes' epilogue)."""
    g = torch.Generator().manual_seed(7 + len(kind))
    if kind == "conv":
        x = torch.randn(2, 9, 9, 128, generator=g)
        w = torch.randn(32, 128, 3, 3, generator=g) / (9 * 128) ** 0.5
        N, act, slope = 32, 1, 0.01
        acc, mac = fp.conv_acc(x, w, 1, 1)
        groups = [fp.conv_products(x, w, 1, 1)]
        z32 = _conv32(x, w).numpy()
    else:
        x = torch.randn(70, 544, generator=g)
        w = torch.randn(48, 544, generator=g)
        N, act, slope = 48, 2, 0.1
        acc, mac = fp.dense_acc(x, w)
        groups = [fp.dense_products(x, w)]
        z32 = (x @ w.t()).numpy()
    scale = 0.5 + torch.rand(N, generator=g)
    scale[SMALL_N] *= 1e-3
    shift = torch.randn(N, generator=g)
    resid = torch.randn(*acc.shape, generator=g)
    y, mag = fp.epilogue32(acc, mac, scale, shift, resid, act, slope)
    c_bar, cap = fp.c_bar_direct(groups, y, mag, scale, shift, resid, act, slope, what=kind)
    c = dict(x=x, w=w, scale=scale, shift=shift, resid=resid, act=act, slope=slope, y=y, mag=mag, c_bar=c_bar, cap=cap, z32=z32,
             what="direct %s" % kind)
    c["ref32"] = _fin_direct(z32, c)
    return c


def _fin_direct(z, c, scale=None):
    v = torch.from_numpy(np.asarray(z, dtype=np.float32)) * (c["scale"] if scale is None else scale) + c["shift"] + c["resid"]
    return torch.relu(v) if c["act"] == 1 else torch.where(v < 0, v * np.float32(c["slope"]), v)


def _stats(c, got):
    st = fp.measure(got, c["y"], c["mag"], c["c_bar"], None, out_f32=True)
    return st, fp.failures(st, out_f32=True)


def _accept(c, got, name):
    st, bad = _stats(c, got)
    old = fp.old_metric(got, c["ref32"])
    print("%s, %s: excess %.3f units <= c_bar %.3f <= cap %d; old metric %.2e" % (c["what"], name, st["excess"], st["c_bar"], c["cap"], old))
    assert not bad, "%s: the bound rejects %s: %s" % (c["what"], name, "; ".join(bad))
    return st, old


def _reject(c, got, name):
    st, bad = _stats(c, got)
    old = fp.old_metric(got, c["ref32"])
    print("%s, MUTANT %s: old metric %.2e, excess %.3g units (c_bar %.3f) -> %s" % (c["what"], name, old, st["excess"], st["c_bar"],
                                                                                "; ".join(bad) or "ACCEPTED"))
    assert bad, "%s: the bound accepts the mutant '%s'" % (c["what"], name)
    return st, old


# ----------------------------------------------------------------------------- the matrices
@pytest.mark.parametrize("m", MS)
def test_cook_toom_identity_is_exact_over_the_rationals(m):
    for seed in range(3):
        assert fp.correlation_identity_holds(m, seed)
    AT, G, BT = fp.cook_toom(m)
    assert (len(AT), len(AT[0]), len(G), len(G[0]), len(BT), len(BT[0])) == (m, m + 2, m + 2, 3, m + 2, m + 2)


@pytest.mark.parametrize("m", MS)
def test_stored_u_is_this_modules_g_rescaled_and_the_layouts_unpermute(m):
    """row_scale reproduces encoder._winograd_u from this module's own G (asserted inside to one fp32 rounding), and the two fused
    layouts un-permute to the same planes, bit for bit."""
    from cadre_amd.encoder import _winograd_u, _winograd_u_c64, _winograd_u_frag
    g = torch.Generator().manual_seed(m)
    w = torch.randn(64, 64, 3, 3, generator=g)
    Up = _winograd_u(w, m)
    D = fp.row_scale(Up, w, m)
    print("F(%dx%d): row scale of the stored U against Cook-Toom G: %s" % (m, m, [str(d) for d in D]))
    if m == 2:
        assert torch.equal(fp.u_from_c64(_winograd_u_c64(w)), Up)
    if m != 6:
        assert torch.equal(fp.u_from_frag(_winograd_u_frag(w, m), m, 64, 64), Up)
    bad = Up.clone()
    bad[1] *= 1.5                                          # plane (0, 1) alone: no diagonal scaling of G explains it
    with pytest.raises(AssertionError):
        fp.row_scale(bad, w, m)


# ----------------------------------------------------------------------------- accepted
@pytest.mark.parametrize("kind", ["conv", "dense"])
def test_honest_direct_result_is_accepted(kind):
    c = direct(kind)
    _, old = _accept(c, c["ref32"], "torch-CPU fp32")
    assert 0 < c["c_bar"] <= c["cap"]


@pytest.mark.parametrize("act", [1, 17])
@pytest.mark.parametrize("m", MS)
def test_honest_winograd_emulation_is_accepted(m, act):
    """All tiles of the emulation, in two of the orders, under a c_bar taken from a sample of the tiles; the honest result passes the OLD
    bar on these inputs (the point of the † mutants below).  (The direct fp32 conv is NOT held to the Winograd bar: at F(2x2) its own
    K = 1152 chain errs by 3 - 4 direct units = 1.1 Winograd units, more than the Winograd form's 128-term chains.)"""
    c = wino(m, act)
    print("%s: c_bar %.3f, emulation's own worst %.3f units, cap %d, mag_w / mag_direct median %.1f max %.1f"
          % (c["what"], c["c_bar"], c["emu"], c["cap"], c["ratio"][0], c["ratio"][1]))
    _, old = _accept(c, _fin(c["z_emu"], c), "fp32 Winograd emulation, sequential")
    assert old < OLD_BAR[m]
    _accept(c, _fin(fp.wino_full(c["x"], c["U"], m, c["D"], rows_first=False, chunk=16), c), "fp32 Winograd emulation, column-first, chunks of 16")


# ----------------------------------------------------------------------------- rejected
@pytest.mark.parametrize("kind", ["conv", "dense"])
def test_direct_operands_cut_to_ten_mantissa_bits_are_rejected(kind):
    c = direct(kind)
    x, w = fp.trunc_mantissa(c["x"]), fp.trunc_mantissa(c["w"])
    z = _conv32(x, w).numpy() if kind == "conv" else (x @ w.t()).numpy()
    _reject(c, _fin_direct(z, c), "operands with a 10-bit mantissa")


@pytest.mark.parametrize("m", MS)
def test_winograd_operands_cut_to_ten_mantissa_bits_are_rejected(m):
    c = wino(m)
    z = fp.wino_full(c["x"], c["U"], m, c["D"], quant=fp.trunc_mantissa)
    _reject(c, _fin(z, c), "V and U with a 10-bit mantissa")


@pytest.mark.parametrize("m", MS)
def test_u_rounded_to_bf16_is_rejected(m):
    c = wino(m)
    z = fp.wino_full(c["x"], c["U"].to(torch.bfloat16).float(), m, c["D"])
    _reject(c, _fin(z, c), "U rounded to bf16")


@pytest.mark.parametrize("m", MS)
def test_small_scale_channel_off_by_a_thousandth_is_rejected_where_the_old_bar_passes(m):
    """† the conv sum of the channel whose scale is 1e-3 of the others, times 1 + 1e-3."""
    c = wino(m)
    z = c["z_emu"].copy()
    z[..., SMALL_N] *= np.float32(1.001)
    st, old = _reject(c, _fin(z, c), "† small-scale channel x (1 + 1e-3)")
    assert old < 2e-5
    assert np.unravel_index(st["worst"], tuple(c["y"].shape))[-1] == SMALL_N


@pytest.mark.parametrize("kind", ["conv", "dense"])
def test_small_scale_channel_off_by_a_thousandth_is_rejected_direct(kind):
    c = direct(kind)
    z = c["z32"].copy()
    z[..., SMALL_N] *= np.float32(1.001)
    _, old = _reject(c, _fin_direct(z, c), "† small-scale channel x (1 + 1e-3)")
    assert old < 2e-5
    assert fp.old_metric(c["ref32"], c["y"]) < 2e-5


@pytest.mark.parametrize("m", MS)
def test_dropped_tap_in_the_last_tile_row_is_rejected_where_the_old_bar_passes(m):
    """† the rows of the last tile row (one of its m rows lies inside the map) miss the centre tap of ONE input channel out of 128."""
    c = wino(m)
    h0 = (-(-c["x"].shape[1] // m) - 1) * m
    z = c["z_emu"].copy()
    z[:, h0:] -= (c["x"][:, h0:, :, QUIET_C:QUIET_C + 1] * c["w"][:, QUIET_C, 1, 1]).numpy()
    st, old = _reject(c, _fin(z, c), "† one tap of one input channel dropped in the last tile row")
    assert old < OLD_BAR[m]
    assert np.unravel_index(st["worst"], tuple(c["y"].shape))[1] >= h0


@pytest.mark.parametrize("act", [1, 17])
@pytest.mark.parametrize("m", MS)
def test_residual_on_the_wrong_side_of_the_relu_is_rejected(m, act):
    c = wino(m, act)
    _reject(c, _fin(c["z_emu"], c, act=act ^ 16), "residual %s the ReLU" % ("after" if act == 1 else "before"))


@pytest.mark.parametrize("m", MS)
def test_shift_added_twice_on_the_small_scale_channel_is_rejected(m):
    c = wino(m)
    shift = c["shift"].clone()
    shift[SMALL_N] *= 2
    st, _ = _reject(c, _fin(c["z_emu"], c, shift=shift), "shift added twice on the small-scale channel")
    assert np.unravel_index(st["worst"], tuple(c["y"].shape))[-1] == SMALL_N


@pytest.mark.parametrize("m", MS)
def test_left_out_k_chunk_of_one_plane_is_rejected(m):
    """Input channels 16 ... 31 of ONE of the (m + 2)^2 planes are not accumulated."""
    c = wino(m)
    Ub = c["U"].clone()
    Ub[(m + 2) + 1, :, 16:32] = 0
    _reject(c, _fin(fp.wino_full(c["x"], Ub, m, c["D"]), c), "one 16-channel k-chunk of plane (1, 1) left out")


def test_c_bar_is_below_the_derived_caps():
    for c in [direct("conv"), direct("dense")] + [wino(m) for m in MS]:
        print("%s: c_bar %.3f units, cap %d" % (c["what"], c["c_bar"], c["cap"]))
        assert 0 < c["c_bar"] <= c["cap"]
    assert fp.DIRECT_CAP(1152) == 1157 and fp.WINO_CAP(128, 6) == 128 + 32 + 8
