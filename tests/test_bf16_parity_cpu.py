"""The bf16 parity bound of tests/bf16_parity.py has teeth: on the trunk's conv shapes it ACCEPTS the honest result (torch-CPU fp32
conv, fp32 epilogue, one rounding to bf16) and REJECTS every CPU-made mutant of the epilogue, of the operand delivery and of the
host-side weight preparation — among them two (a truncating float -> bf16 conversion, a double rounding in front of the residual)
that the metric of the existing bf16 kernel tests, max|got - ref| / max|ref| < 1.5e-2, lets through.  No GPU."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import bf16_parity as bp

BF = torch.bfloat16

# (F, H, W, Cin, N): layer2 / layer3 / layer4 / layer1 convs of the 288 x 288 model
RING_SHAPES = [(2, 36, 36, 128, 128), (3, 18, 18, 256, 256), (5, 9, 9, 512, 512), (1, 72, 72, 64, 64)]
S2_SHAPE = (2, 36, 36, 128, 256)             # 3x3 / s2 conv1 of layer3.0
S1X_SHAPE = (3, 18, 18, 256, 128, 256)       # conv2 of layer3.0 with its 1x1 / s2 shortcut as K-extension: (F, H, W, C1, Cd, N)


def _nchw(t):
    return t.float().permute(0, 3, 1, 2)


def _conv32(x, w, stride=1, pad=1):
    return F.conv2d(_nchw(x), w.float(), None, stride, pad).permute(0, 2, 3, 1).contiguous()


def _fold(w32, scale):
    """The documented fold: bf16(w * scale), the product in fp32, ONE rounding."""
    return (w32 * scale.view(-1, 1, 1, 1)).to(BF)


def _fold_twice(w32, scale):
    """The wrong fold: bf16(bf16(w) * scale)."""
    return (w32.to(BF).float() * scale.view(-1, 1, 1, 1)).to(BF)


def _finish32(z, resid, act):
    """fp32 epilogue behind z = conv + shift: residual before / after the ReLU by act & 16."""
    if resid is not None and not (act & 16):
        z = z + resid.float()
    if act & 1:
        z = torch.relu(z)
    if resid is not None and (act & 16):
        z = z + resid.float()
    return z


@functools.lru_cache(maxsize=None)
def ring_case(shape, act):
    Fn, H, W, Cin, N = shape
    g = torch.Generator().manual_seed(Fn * 131 + H * 7 + Cin + N + act)
    x = torch.randn(Fn, H, W, Cin, generator=g).to(BF)
    w32 = torch.randn(N, Cin, 3, 3, generator=g) * (1.5 / np.sqrt(9 * Cin))
    scale = torch.rand(N, generator=g) + 0.5
    shift = torch.randn(N, generator=g)
    resid = torch.randn(Fn, H, W, N, generator=g).to(BF)
    w = _fold(w32, scale)
    acc, mac = bp.conv_acc(x, w, 1, 1)
    y, mag, clamped = bp.epilogue(acc, mac, None, shift, resid, act)
    c_bar = bp.c_bar_of([bp.conv_products(x, w, 1, 1)], y, mag, None, shift, resid, act, what="ring %s" % (shape,))
    return dict(x=x, w32=w32, w=w, scale=scale, shift=shift, resid=resid, act=act, y=y, mag=mag, clamped=clamped, c_bar=c_bar,
                z32=_conv32(x, w) + shift, what="conv3x3 s1 %s act %d" % (shape, act))


@functools.lru_cache(maxsize=None)
def s2_case():
    Fn, H, W, Cin, N = S2_SHAPE
    g = torch.Generator().manual_seed(52)
    x = torch.randn(Fn, H, W, Cin, generator=g).to(BF)
    w32 = torch.randn(N, Cin, 3, 3, generator=g) * (1.5 / np.sqrt(9 * Cin))
    scale = torch.rand(N, generator=g) + 0.5
    shift = torch.randn(N, generator=g)
    w = _fold(w32, scale)
    acc, mac = bp.conv_acc(x, w, 2, 1)
    y, mag, clamped = bp.epilogue(acc, mac, None, shift, None, 1)
    c_bar = bp.c_bar_of([bp.conv_products(x, w, 2, 1)], y, mag, None, shift, None, 1, what="s2")
    return dict(x=x, w32=w32, w=w, scale=scale, shift=shift, resid=None, act=1, y=y, mag=mag, clamped=clamped, c_bar=c_bar,
                z32=_conv32(x, w, 2, 1) + shift, what="conv3x3 s2 %s" % (S2_SHAPE,), stride=2)


@functools.lru_cache(maxsize=None)
def s1x_case():
    Fn, H, W, C1, Cd, N = S1X_SHAPE
    g = torch.Generator().manual_seed(53)
    t = torch.randn(Fn, H, W, C1, generator=g).to(BF)
    x2 = torch.randn(Fn, 2 * H, 2 * W, Cd, generator=g).to(BF)
    w2_32 = torch.randn(N, C1, 3, 3, generator=g) * (1.5 / np.sqrt(9 * C1))
    wd_32 = torch.randn(N, Cd, 1, 1, generator=g) * (1.5 / np.sqrt(Cd))
    s2, sd = torch.rand(N, generator=g) + 0.5, torch.rand(N, generator=g) + 0.5
    shift = torch.randn(N, generator=g) + torch.randn(N, generator=g)          # the sum of both shifts
    w2, wd = _fold(w2_32, s2), _fold(wd_32, sd)
    a1, m1 = bp.conv_acc(t, w2, 1, 1)
    a2, m2 = bp.shortcut_acc(x2, wd)
    y, mag, clamped = bp.epilogue(a1 + a2, m1 + m2, None, shift, None, 1)
    c_bar = bp.c_bar_of([bp.conv_products(t, w2, 1, 1), bp.conv_products(x2, wd, 2, 0)], y, mag, None, shift, None, 1, what="s1x")
    return dict(x=t, x2=x2, w32=w2_32, w=w2, wd=wd, scale=s2, shift=shift, resid=None, act=1, y=y, mag=mag, clamped=clamped,
                c_bar=c_bar, z32=_conv32(t, w2) + _conv32(x2, wd, 2, 0) + shift, what="conv3x3 s1x %s" % (S1X_SHAPE,))


def _stats(c, got):
    st = bp.measure(got, c["y"], c["mag"], c["c_bar"], c["clamped"])
    return st, bp.failures(st, need_bias_n=10000)


def _accept(c, got, name):
    st, bad = _stats(c, got)
    print(bp.line("%s, %s" % (c["what"], name), st))
    assert not bad, "%s: the bound rejects %s: %s" % (c["what"], name, "; ".join(bad))
    return st


def _reject(c, got, name):
    st, bad = _stats(c, got)
    print(bp.line("%s, MUTANT %s" % (c["what"], name), st) + " -> " + ("; ".join(bad) or "ACCEPTED"))
    assert bad, "%s: the bound accepts the mutant '%s'" % (c["what"], name)
    return st


def _honest(c, z32=None):
    return _finish32(c["z32"] if z32 is None else z32, c["resid"], c["act"]).to(BF)


def _all_cases():
    return [ring_case(s, 1) for s in RING_SHAPES] + [s2_case(), s1x_case()]


CASE_IDS = ["l2_36px_128", "l3_18px_256", "l4_9px_512", "l1_72px_64", "s2_36px_128_256", "s1x_18px_256_128"]

def _case(i):
    return ring_case(RING_SHAPES[i], 1) if i < 4 else (s2_case() if i == 4 else s1x_case())


@pytest.mark.parametrize("i", range(6), ids=CASE_IDS)
def test_honest_result_is_accepted(i):
    """torch-CPU fp32 conv + fp32 epilogue, rounded once to bf16: inside the bound, mismatch share far below the 1e-3 cap (the
    fp32 result alone differs from the float64 rounding in about 5e-5 of the elements), no rounding bias."""
    c = _case(i)
    st = _accept(c, _honest(c), "honest fp32 result")
    assert st["n_bias"] >= 10000


@pytest.mark.parametrize("act", [1, 17])
@pytest.mark.parametrize("i", range(4), ids=CASE_IDS[:4])
def test_honest_result_is_accepted_for_both_residual_positions(i, act):
    c = ring_case(RING_SHAPES[i], act)
    _accept(c, _honest(c), "honest fp32 result")


@pytest.mark.parametrize("i", range(6), ids=CASE_IDS)
def test_truncating_conversion_is_rejected(i):
    """float -> bf16 by dropping the low 16 bits: shows as a rounding bias of half an ulp towards zero."""
    c = _case(i)
    got = bp.trunc_bf16(_finish32(c["z32"], c["resid"], c["act"]))
    st = _reject(c, got, "truncating conversion")
    assert st["bias"] < -0.4                                   # (the outputs in the bias sample are positive: ReLU)
    assert bp.old_metric(got, _finish32(c["z32"], c["resid"], c["act"])) < 1.5e-2     # ... and the old metric lets it through


@pytest.mark.parametrize("i", range(4), ids=CASE_IDS[:4])
def test_double_rounding_before_the_residual_is_rejected(i):
    """conv + shift rounded to bf16, the residual added, rounded again."""
    c = _case(i)
    got = torch.relu(c["z32"].to(BF).float() + c["resid"].float()).to(BF)
    _reject(c, got, "double rounding")
    assert bp.old_metric(got, _finish32(c["z32"], c["resid"], c["act"])) < 1.5e-2     # the gap the new bar closes


@pytest.mark.parametrize("act", [1, 17])
@pytest.mark.parametrize("i", range(4), ids=CASE_IDS[:4])
def test_residual_on_the_wrong_side_of_the_relu_is_rejected(i, act):
    """act 1: the residual belongs BEFORE the ReLU, the mutant adds it after; act 17 (act & 16): the reverse."""
    c = ring_case(RING_SHAPES[i], act)
    got = _finish32(c["z32"], c["resid"], act ^ 16).to(BF)
    _reject(c, got, "residual %s the ReLU" % ("after" if act == 1 else "before"))


@pytest.mark.parametrize("i", range(6), ids=CASE_IDS)
def test_dropped_last_input_channel_is_rejected(i):
    c = _case(i)
    x = c["x"].clone()
    x[..., -1] = 0
    z = _conv32(x, c["w"], c.get("stride", 1), 1) + c["shift"]
    if "x2" in c:
        z = z + _conv32(c["x2"], c["wd"], 2, 0)
    _reject(c, _honest(c, z), "last input channel dropped")


@pytest.mark.parametrize("i", range(6), ids=CASE_IDS)
def test_dropped_tap_on_the_left_border_column_is_rejected(i):
    """Output column 0 only: the tap (kh, kw) = (0, 1) — one the border does NOT mask — contributes nothing."""
    c = _case(i)
    w_tap = torch.zeros_like(c["w"])
    w_tap[:, :, 0, 1] = c["w"][:, :, 0, 1]
    z = c["z32"].clone()
    z[:, :, 0] -= _conv32(c["x"], w_tap, c.get("stride", 1), 1)[:, :, 0]
    _reject(c, _honest(c, z), "one tap dropped on the left border column")


@pytest.mark.parametrize("i", range(6), ids=CASE_IDS)
def test_scale_folded_with_two_roundings_is_rejected(i):
    """bf16(bf16(w) * scale) instead of the documented bf16(w * scale) with the product in fp32."""
    c = _case(i)
    w_bad = _fold_twice(c["w32"], c["scale"])
    assert not torch.equal(w_bad, c["w"])
    z = _conv32(c["x"], w_bad, c.get("stride", 1), 1) + c["shift"]
    if "x2" in c:
        z = z + _conv32(c["x2"], c["wd"], 2, 0)
    _reject(c, _honest(c, z), "BN scale folded with two roundings")


def test_left_out_shortcut_k_tile_is_rejected():
    """cadre_conv3x3_s1x form: the last 64-channel k-tile of the shortcut is not accumulated."""
    c = s1x_case()
    wd = c["wd"].clone()
    wd[:, -64:] = 0
    z = _conv32(c["x"], c["w"]) + _conv32(c["x2"], wd, 2, 0) + c["shift"]
    _reject(c, _honest(c, z), "one shortcut k-tile left out")


def test_number_format_helpers():
    """ulp_bf16 / rne_bf16 against torch's own bf16 on values that fp32 holds exactly (there the two roundings coincide), and a
    value where rounding through fp32 would go wrong."""
    g = torch.Generator().manual_seed(1)
    v = torch.cat([torch.randn(20000, generator=g) * 3, torch.tensor([0.0, 1.0, -1.0, 255.0, 2.0 ** -126, 1.00390625, 1.01171875])])
    want = v.to(BF).double().numpy()
    assert np.array_equal(bp.rne_bf16(v.double().numpy()), want)
    assert bp.ulp_bf16(np.array([1.0, 1.99, 2.0, 0.75, 0.0]))[:4].tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8]
    y = 1.0 + 2.0 ** -8 + 2.0 ** -40                      # fp32 rounds this to the tie 1 + 2^-8, which then rounds to even: 1.0
    assert float(torch.tensor(y, dtype=torch.float64).float().to(BF)) == 1.0
    assert bp.rne_bf16(np.array([y]))[0] == 1.0 + 2.0 ** -7
    assert np.array_equal(bp.trunc_bf16(torch.tensor([1.0 + 2.0 ** -7 - 2.0 ** -20, -3.999])).double().numpy(), [1.0, -3.984375])


def test_c_bar_is_a_property_of_the_case_not_of_a_result():
    """c_bar comes from the sequential fp32 chain of the case's own sums: a few units, below the rigorous K + 4, and the same
    whatever result is later checked against it."""
    for c in _all_cases():
        print("%s: c_bar %.3f units" % (c["what"], c["c_bar"]))
        K = 9 * c["x"].shape[-1] + (c["x2"].shape[-1] if "x2" in c else 0)
        assert 0 < c["c_bar"] <= K + 4