"""CPU: the decoder branches — tests/decode_ref.py against the golden of the imported reference (tests/golden/make_decode_golden.py),
synth.decoder_spec, the host's weight packing and BatchNorm fold (cadre_amd/decoder.py), the C ABI additions, and the teeth of the
element-wise bound tests/test_decode_gpu.py applies to cadre_deconv3x3_s2."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from cadre_amd import decoder, synth
from tests import decode_ref as ref
from tests import f32_parity as fp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {"cadre_deconv3x3_s2_supported": 8, "cadre_deconv3x3_s2": 17, "cadre_deconv3x3_s2_out": 13, "cadre_argmax_rows": 6, "cadre_bc_head": 15}


# ----------------------------------------------------------------------------- the golden
@pytest.fixture(scope="module")
def restated(golden):
    g, enc = golden("decode_native"), golden("enc_native")
    sd = synth.decoder_state(int(g["seed"]))
    lat = torch.from_numpy(enc["latent"])
    return g, ref.decode(sd, lat, torch.from_numpy(g["speeds"])), ref.decode(sd, lat, None)


@pytest.mark.parametrize("name", ["rf", "seg1", "seg", "route", "light", "steer", "throttle"])
def test_decode_ref_reproduces_the_golden(restated, name):
    g, o, _ = restated
    err = ref.rel_max(ref.subsample(o)[name], g[name])
    print("%s: rel-max %.3e against the fp32 reference" % (name, err))
    assert g[name].dtype == np.float32 and err <= 1e-6


def test_decode_ref_without_speed_and_light_state(restated):
    g, o, o0 = restated
    assert ref.rel_max(o0["steer"], g["steer_nospeed"]) <= 1e-6 and ref.rel_max(o0["throttle"], g["throttle_nospeed"]) <= 1e-6
    assert not np.array_equal(g["steer"], g["steer_nospeed"])              # the speed path does something
    assert np.array_equal(o["light"].argmax(1).numpy(), g["light_state"])
    # what the speed does not reach is the same with and without it
    assert torch.equal(o["seg"], o0["seg"]) and torch.equal(o["light"], o0["light"])


def test_golden_holds_the_subsample_it_says(golden):
    g = golden("decode_native")
    assert np.array_equal(g["rows_out"], ref.ROWS_OUT) and int(g["ch_step"]) == ref.CH_STEP
    rows = set(int(r) for r in ref.ROWS_OUT)
    assert {0, 143} <= rows and any(r % 2 for r in rows) and any(r % 2 == 0 for r in rows)
    assert g["seg"].shape == (2, 8, len(rows), 256) and g["route"].shape == (2, 1, len(rows), 256)
    assert g["rf"].shape == (2, 128, 5, 8) and g["seg1"].shape == (2, 64, 9, 16)
    size = lambda n: os.path.getsize(os.path.join(ROOT, "tests", "golden", n))
    assert size("decode_native.npz") <= size("enc_288.npz")


def test_decoder_spec_is_the_reference_key_list(golden):
    g = golden("decode_native")
    spec = synth.decoder_spec()
    assert [k for k, _, _ in spec] == [str(k) for k in g["keys"]]
    assert [",".join(str(d) for d in s) for _, s, _ in spec] == [str(s) for s in g["shapes"]]
    assert len(spec) == 78 and sum(kd == "count" for _, _, kd in spec) == 8
    n_par = sum(int(np.prod(s)) for _, s, kd in spec if kd != "count")
    assert 19.0e6 < n_par < 19.2e6
    sd = synth.decoder_state(3)
    assert all(sd[k].shape == tuple(s) and sd[k].dtype == (np.int64 if kd == "count" else np.float32) for k, s, kd in spec)
    assert np.array_equal(sd[spec[0][0]], synth.decoder_state(3)[spec[0][0]]) and not np.array_equal(sd[spec[0][0]], synth.decoder_state(4)[spec[0][0]])
    # the encoder's spec is untouched (the committed goldens depend on it)
    assert not any(k.startswith(decoder.PREFIXES) for k, _, _ in synth.encoder_spec(5, 8))


def test_has_decoder_and_the_first_missing_key():
    sd = synth.decoder_state(0)
    assert decoder.has_decoder(sd) and not decoder.has_decoder(synth.encoder_state(5, 8))
    first = synth.decoder_spec()[0][0]
    assert decoder._first_missing({k: v for k, v in sd.items() if k != first}) == first
    assert decoder.has_decoder({k: v for k, v in sd.items() if not k.endswith("num_batches_tracked")})


# ----------------------------------------------------------------------------- packing and folding
@pytest.mark.parametrize("Cin,Cout", [(512, 256), (256, 128), (128, 64), (64, 32)])
def test_pack_deconv_round_trip_and_class_order(Cin, Cout):
    w = torch.from_numpy(np.random.RandomState(Cin).standard_normal((Cin, Cout, 3, 3)).astype(np.float32))
    flat = decoder.pack_deconv(w)
    assert flat.shape == (9 * Cin * Cout,) and flat.dtype == torch.float32
    back = decoder.unpack_deconv(flat, Cin, Cout)
    assert np.array_equal(back.numpy().view(np.uint32), w.numpy().view(np.uint32))
    # the layout the header documents, class by class, stated with decode_ref's own tap table
    o = 0
    for py in (0, 1):
        for px in (0, 1):
            taps = ref.class_taps(py, px)
            assert len(taps) == (1 + py) * (1 + px)
            blk = flat[o:o + Cout * len(taps) * Cin].reshape(Cout, len(taps), Cin)
            o += blk.numel()
            for t, (dy, dx, ky, kx) in enumerate(taps):
                assert t == dy * (1 + px) + dx
                assert torch.equal(blk[:, t, :], w[:, :, ky, kx].t()), (py, px, t)
    assert o == flat.numel()


@pytest.mark.parametrize("Cout", [1, 3, 8])
def test_pack_deconv_out_round_trip(Cout):
    w = torch.from_numpy(np.random.RandomState(Cout).standard_normal((32, Cout, 3, 3)).astype(np.float32))
    p = decoder.pack_deconv_out(w)
    CO = decoder.out_channels_padded(Cout)
    assert p.shape == (3, 3, 32, CO) and CO >= Cout and CO in (1, 2, 4, 8) and not p[..., Cout:].any()
    assert torch.equal(decoder.unpack_deconv_out(p, Cout), w) and float(p[2, 0, 5, 0]) == float(w[5, 0, 2, 0])


def test_chw_to_hwc_permutations():
    r = np.random.RandomState(0)
    w2 = torch.from_numpy(r.standard_normal((512 * 40, 8)).astype(np.float32))        # rows c * 40 + h * 8 + w (fewer columns: the same map)
    b2 = torch.from_numpy(r.standard_normal(512 * 40).astype(np.float32))
    w1 = torch.from_numpy(r.standard_normal((6, 512 * 40)).astype(np.float32))
    pw, pb, pc = decoder.chw_rows_to_hwc(w2), decoder.chw_rows_to_hwc(b2), decoder.chw_cols_to_hwc(w1)
    for c, h, w in ((0, 0, 0), (511, 4, 7), (17, 3, 2), (300, 0, 7)):
        src, dst = c * 40 + h * 8 + w, (h * 8 + w) * 512 + c
        assert torch.equal(pw[dst], w2[src]) and pb[dst] == b2[src] and torch.equal(pc[:, dst], w1[:, src])
    assert torch.equal(decoder.hwc_rows_to_chw(pw), w2) and torch.equal(decoder.hwc_rows_to_chw(pb), b2)
    assert torch.equal(decoder.hwc_cols_to_chw(pc), w1)
    # a product through the permuted pair is the product through the original pair: x -> rf (C-H-W) -> light, both permuted
    x = torch.from_numpy(r.standard_normal((3, 8)))
    assert torch.allclose((x @ w2.double().t()) @ w1.double().t(), (x @ pw.double().t()) @ pc.double().t(), rtol=1e-12, atol=1e-12)


def test_fold_matches_the_float64_fold_to_one_rounding():
    sd = synth.decoder_state(5)
    for m in ("visual_branch.reverse_image", "visual_branch.reverse_route"):
        for i in range(4):
            bn = "%s.%d" % (m, 3 * i + 1)
            args = [sd["%s.%d.bias" % (m, 3 * i)]] + [sd[bn + s] for s in (".weight", ".bias", ".running_mean", ".running_var")]
            sc, sh = decoder.fold_bn(*args)
            sc64, sh64 = ref.fold_bn64(*args)
            assert sc.dtype == sh.dtype == torch.float32
            assert bool(((sc.double() - sc64).abs() <= 2.0 ** -24 * sc64.abs()).all())
            assert bool(((sh.double() - sh64).abs() <= 2.0 ** -24 * sh64.abs() + 1e-45).all())


# ----------------------------------------------------------------------------- C ABI
def test_entry_points_are_exported_and_bound():
    from cadre_amd import hip
    L = ctypes.CDLL(hip.LIB_PATH)                                             # loads without a GPU
    hdr = open(os.path.join(ROOT, "include", "cadre_hip.h")).read()
    for name, nargs in NEW_SYMBOLS.items():
        assert hasattr(L, name) and name in hip.SYMBOLS and re.search(r"\bint %s\s*\(" % name, hdr), name
        assert len(hip.SYMBOLS[name]) == nargs, name
    assert hip.lib().cadre_abi_version() == hip.ABI_VERSION == 15          # entry points are only added
    assert '"deconv.hip"' in open(os.path.join(ROOT, "cadre_amd", "build.py")).read()
    from ppo_agent import decode as shim
    assert shim.DANetDecoderHIP is decoder.DANetDecoderHIP and shim.has_decoder is decoder.has_decoder


def test_supported_answers():
    from cadre_amd import hip
    f = hip.lib().cadre_deconv3x3_s2_supported
    for Cin, Cout, H, W, oph, opw in decoder.LEVELS:
        assert f(2, 64, H, W, Cin, Cout, oph, opw) == 1
    assert f(1, 1, 2, 3, 64, 32, 0, 0) == 1
    assert f(1, 1, 2, 3, 48, 32, 1, 1) == 0 and f(1, 1, 2, 3, 64, 24, 1, 1) == 0          # channels no multiple of 32
    assert f(1, 1, 2, 3, 64, 32, 2, 0) == 0 and f(0, 1, 2, 3, 64, 32, 1, 1) == 0 and f(1, 1, 0, 3, 64, 32, 1, 1) == 0
    assert f(2, 1024, 36, 64, 64, 32, 1, 1) == 0                             # level 4 of 1024 frames: the output is 2.4 GB
    assert f(2, 512, 36, 64, 64, 32, 1, 1) == 1
    assert f(1, 2 ** 31 - 1, 2 ** 15, 2 ** 15, 512, 256, 1, 1) == 0           # no overflow in the size arithmetic


def test_bad_arguments_are_refused_without_a_launch():
    """Every call below returns -1 from the host checks (nothing is launched: this machine has no GPU to launch on)."""
    from cadre_amd import hip
    L = hip.lib()
    P = 1 << 20                                                              # a non-null, 16-byte aligned address nobody dereferences
    err = lambda: L.cadre_last_error().decode()
    ok = dict(x=P, zs=0, w=P, scale=P, shift=P, out=P, Z=1, F=1, H=2, W=3, Cin=64, Cout=32, oph=1, opw=1, act=2, slope=0.01)

    def level(**kw):
        a = dict(ok, **kw)
        return L.cadre_deconv3x3_s2(a["x"], a["zs"], a["w"], a["scale"], a["shift"], a["out"], a["Z"], a["F"], a["H"], a["W"], a["Cin"], a["Cout"],
                                    a["oph"], a["opw"], a["act"], a["slope"], None)
    for name in ("x", "w", "scale", "shift", "out"):
        assert level(**{name: None}) == -1 and "null" in err(), name
    assert level(Cin=48) == -1 and "Cin % 32" in err()
    assert level(Cout=40) == -1
    assert level(F=2 ** 24, H=36, W=64) == -1 and "2 GiB" in err()
    assert level(act=3) == -1 and level(x=P + 4) == -1 and level(zs=8) == -1 and level(oph=2) == -1

    def last(x=P, w=P, bias=P, logits=P, cls=None, sig=None, F=1, H=3, W=4, Cout=8, oph=1, opw=1):
        return L.cadre_deconv3x3_s2_out(x, w, bias, logits, cls, sig, F, H, W, Cout, oph, opw, None)
    assert last(x=None) == -1 and last(w=None) == -1 and last(bias=None) == -1
    assert last(logits=None) == -1 and "no output" in err()
    assert last(Cout=9) == -1 and "Cout <= 8" in err()
    assert last(Cout=0) == -1 and last(sig=P) == -1 and last(F=2 ** 22, H=72, W=128) == -1 and last(x=P + 8) == -1
    assert L.cadre_argmax_rows(None, 4, 1, 4, P, None) == -1 and L.cadre_argmax_rows(P, 2, 1, 4, P, None) == -1
    head = lambda lat=P, ld=544, out=P, F=1, w=P: L.cadre_bc_head(lat, ld, None, w, P, P, P, P, P, P, P, out, F, 0.01, None)
    assert head(lat=None) == -1 and head(out=None) == -1 and head(w=None) == -1 and head(ld=511) == -1 and head(F=0) == -1


def test_decoder_refuses_a_cpu_device_and_a_checkpoint_without_the_branches():
    from cadre_amd import hip
    with pytest.raises(hip.CadreHipError, match="no CPU path"):
        decoder.DANetDecoderHIP(synth.decoder_state(0), "cpu")


# ----------------------------------------------------------------------------- the bound has teeth
def _case(seed=0, Fn=1, H=5, W=8, Cin=64, Cout=32, oph=0, opw=1, act=2):
    r = np.random.RandomState(seed)
    x = torch.from_numpy(r.standard_normal((Fn, H, W, Cin)).astype(np.float32))
    w = torch.from_numpy((r.standard_normal((Cin, Cout, 3, 3)) * np.sqrt(2.0 / (Cin * 2.25))).astype(np.float32))
    scale = fp.log_scales(r, Cout)
    shift = torch.from_numpy((r.standard_normal(Cout) * 0.1).astype(np.float32))
    y, mag = ref.level_ref(x, w, scale, shift, oph, opw, act)
    c_bar, cap = ref.level_c_bar(x, w, y, mag, scale, shift, oph, opw, act, what="teeth")
    return x, w, scale, shift, y, mag, c_bar, cap


def test_the_four_parity_sums_are_the_library_transposed_convolution():
    """decode_ref states the operation on its own; this pins the statement to torch's ConvTranspose2d once."""
    for oph, opw in ((0, 1), (1, 1), (0, 0), (1, 0)):
        x, w = _case(1, 2, 3, 4, 32, 32, oph, opw)[:2]
        acc, _ = ref.deconv_acc(x, w, oph, opw)
        want = torch.nn.functional.conv_transpose2d(x.double().permute(0, 3, 1, 2), w.double(), None, 2, 1, (oph, opw)).permute(0, 2, 3, 1)
        assert acc.shape == want.shape and float((acc - want).abs().max()) <= 1e-12


def test_bound_accepts_an_fp32_evaluation_and_has_teeth():
    x, w, scale, shift, y, mag, c_bar, cap = _case()
    assert cap == fp.DIRECT_CAP(4 * 64)
    # an fp32 evaluation in another order (torch's own kernel) passes
    got = torch.nn.functional.conv_transpose2d(x.permute(0, 3, 1, 2), w, None, 2, 1, (0, 1)).permute(0, 2, 3, 1) * scale + shift
    got = torch.where(got < 0, got * np.float32(0.01), got)
    fp.check32(got, y, mag, c_bar, cap, what="fp32 evaluation")
    # one tap of one parity class dropped
    for drop in ((1, 1, 1, 1), (0, 1, 0, 1), (1, 0, 0, 0), (0, 0, 0, 0)):
        bad, _ = ref.level_ref(x, w, scale, shift, 0, 1, 2, drop=drop)
        with pytest.raises(AssertionError, match="excess"):
            fp.check32(bad.float(), y, mag, c_bar, cap, what="tap %s dropped" % (drop,))
    # oph / opw swapped: another output shape; where both shapes have an element, the last column's taps differ
    swapped, _ = ref.level_ref(x, w, scale, shift, 1, 0, 2)
    with pytest.raises(AssertionError, match="shape"):
        fp.check32(swapped.float(), y, mag, c_bar, cap, what="oph / opw swapped")
    x2, w2, sc2, sh2, y2, mag2, c2, cap2 = _case(2, 1, 2, 3, 64, 32, 1, 1)
    for oph, opw in ((0, 1), (1, 0)):                      # fed into a buffer of the right shape: the missing row / column stays unwritten
        part, _ = ref.level_ref(x2, w2, sc2, sh2, oph, opw, 2)
        buf = torch.zeros_like(y2)
        buf[:, :part.shape[1], :part.shape[2]] = part
        with pytest.raises(AssertionError, match="excess"):
            fp.check32(buf.float(), y2, mag2, c2, cap2, what="output padding (%d, %d) for (1, 1)" % (oph, opw))
