"""GPU: the decoder kernels (csrc/deconv.hip) element by element against tests/decode_ref.py's float64 under the fp32 rule of
tests/f32_parity.py, and DANetDecoderHIP.decode / CadreAgent.decode against the golden of the imported reference.

Bars, none taken from the code under test:
  * cadre_deconv3x3_s2 and the logits of cadre_deconv3x3_s2_out: |got - y64| <= c_bar 2^-24 mag for EVERY element, c_bar from the
    sequential fp32 chain over the case's own products (K = 4 Cin slots for the cap), doubled.
  * class map: equals the float64 argmax wherever the float64 top-two margin exceeds twice the element's bound; at most 0.1 % of
    the positions may be left out for that reason (asserted).
  * sigmoid: bound_logit / 4 (the sigmoid's slope is at most 1/4) + c 2^-24, c = twice the worst error of an fp32 numpy emulation
    of the kernel's formula over the case's float64 logits (printed).
  * the whole decode: rel-max error against float64 at most 8 x the error the golden (the fp32 reference's result) has against the
    same float64 — both are fp32 chains of the same seven stages in another summation order.  bc and light_state are also compared
    with the golden directly: by the triangle inequality they then differ by at most 9 x the golden's own error.
"""
import numpy as np
import pytest
import torch

from cadre_amd import decoder, synth
from tests import decode_ref as ref
from tests import f32_parity as fp

pytestmark = pytest.mark.gpu
SENT = 12345.0
MARGIN = 1024


def dev():
    return torch.device("cuda:0")


def level_case(seed, Z, Fn, H, W, Cin, Cout, shared):
    r = np.random.RandomState(seed)
    nx = 1 if shared else Z
    x = torch.from_numpy(r.standard_normal((nx, Fn, H, W, Cin)).astype(np.float32))
    w = torch.from_numpy((r.standard_normal((Z, Cin, Cout, 3, 3)) * np.sqrt(2.0 / (Cin * 2.25))).astype(np.float32))
    scale = torch.stack([fp.log_scales(r, Cout) for _ in range(Z)])
    shift = torch.from_numpy((r.standard_normal((Z, Cout)) * 0.1).astype(np.float32))
    return x, w, scale, shift


def run_level(x, w, scale, shift, Z, Fn, H, W, Cin, Cout, oph, opw, act, shared):
    from cadre_amd import hip
    Ho, Wo = ref.out_hw(H, W, oph, opw)
    n = Z * Fn * Ho * Wo * Cout
    out = torch.full((n + MARGIN,), SENT, device=dev())
    wp = torch.stack([decoder.pack_deconv(w[z]) for z in range(Z)]).to(dev())
    assert hip.lib().cadre_deconv3x3_s2_supported(Z, Fn, H, W, Cin, Cout, oph, opw) == 1
    hip.deconv3x3_s2(x.to(dev()), 0 if shared else Fn * H * W * Cin, wp, scale.to(dev()), shift.to(dev()), out, Z, Fn, H, W, Cin, Cout, oph, opw,
                     act=act, slope=ref.SLOPE)
    torch.cuda.synchronize()
    got = out.cpu()
    assert bool((got[n:] == SENT).all()), "the margin behind the output was written"
    return got[:n].reshape(Z, Fn, Ho, Wo, Cout)


def check_level(seed, Z, Fn, H, W, Cin, Cout, oph, opw, act, shared):
    what = "deconv %dx%d op(%d,%d) F%d %d->%d Z%d%s act%d" % (H, W, oph, opw, Fn, Cin, Cout, Z, " shared" if shared else "", act)
    x, w, scale, shift = level_case(seed, Z, Fn, H, W, Cin, Cout, shared)
    got = run_level(x, w, scale, shift, Z, Fn, H, W, Cin, Cout, oph, opw, act, shared)
    assert bool(torch.isfinite(got).all())
    for z in range(Z):
        xz = x[0 if shared else z]
        y, mag = ref.level_ref(xz, w[z], scale[z], shift[z], oph, opw, act)
        c_bar, cap = ref.level_c_bar(xz, w[z], y, mag, scale[z], shift[z], oph, opw, act, what=what)
        assert cap == fp.DIRECT_CAP(4 * Cin)
        fp.check32(got[z], y, mag, c_bar, cap, what="%s z%d" % (what, z))


MAPS = [(2, 3), (5, 8)]
PADS = [(0, 1), (1, 1), (0, 0)]
ZMODES = [(1, False), (2, True), (2, False)]           # (Z, every module reads the same input: z stride 0)


@pytest.mark.parametrize("H,W", MAPS)
@pytest.mark.parametrize("oph,opw", PADS)
def test_deconv_level_64_32_every_combination(H, W, oph, opw):
    """Cin / Cout = 64 / 32 (the one-accumulator tile): F = 1 and 3, Z = 1, 2 with z stride 0 and non-zero, act 0 and 2."""
    seed = 0
    for Fn in (1, 3):
        for Z, shared in ZMODES:
            for act in (0, 2):
                seed += 1
                check_level(1000 * H + 100 * oph + 10 * opw + seed, Z, Fn, H, W, 64, 32, oph, opw, act, shared)


@pytest.mark.parametrize("H,W", MAPS)
@pytest.mark.parametrize("oph,opw", PADS)
def test_deconv_level_512_256(H, W, oph, opw):
    """Cin / Cout = 512 / 256 (the two-accumulator tile, 16 .. 64 k-tiles): the deployed level 1 is 5x8, (0, 1), Z = 2, shared input."""
    seed = 7000 + 1000 * H + 100 * oph + 10 * opw
    check_level(seed + 1, 2, 1, H, W, 512, 256, oph, opw, 2, True)
    check_level(seed + 2, 1, 3 if (H, W) == (2, 3) or (oph, opw) == (0, 1) else 1, H, W, 512, 256, oph, opw, 0, False)
    if (H, W) == (2, 3):
        check_level(seed + 3, 2, 3, H, W, 512, 256, oph, opw, 2, False)
    else:
        check_level(seed + 3, 2, 1, H, W, 512, 256, oph, opw, 0, False)


# ----------------------------------------------------------------------------- the last level
def out_case(seed, Fn, H, W, Cout):
    r = np.random.RandomState(seed)
    x = torch.from_numpy(r.standard_normal((Fn, H, W, 32)).astype(np.float32))
    w = torch.from_numpy((r.standard_normal((32, Cout, 3, 3)) * np.sqrt(2.0 / (32 * 2.25))).astype(np.float32))
    bias = torch.from_numpy((r.standard_normal(Cout) * 0.1).astype(np.float32))
    return x, w, bias


@pytest.mark.parametrize("H,W", [(3, 4), (9, 16)])
@pytest.mark.parametrize("Cout", [8, 1])
@pytest.mark.parametrize("Fn", [1, 3])
def test_deconv_out(H, W, Cout, Fn):
    from cadre_amd import hip
    what = "deconv_out %dx%d F%d Cout%d" % (H, W, Fn, Cout)
    x, w, bias = out_case(31 * H + 7 * Cout + Fn, Fn, H, W, Cout)
    Ho, Wo = 2 * H, 2 * W
    npos = Fn * Ho * Wo
    y, mag = ref.level_ref(x, w, None, bias, 1, 1, 0)
    c_bar, cap = ref.level_c_bar(x, w, y, mag, None, bias, 1, 1, 0, what=what)
    assert cap == fp.DIRECT_CAP(4 * 32)
    bound = c_bar * fp.U * mag                                             # per element
    d = dev()
    xd, wd, bd = x.to(d), decoder.pack_deconv_out(w).to(d), bias.to(d)
    logits = torch.full((npos * Cout + MARGIN,), SENT, device=d)
    cls = torch.full((npos + MARGIN,), 77, device=d, dtype=torch.uint8)
    sig = torch.full((npos + MARGIN,), SENT, device=d)
    use_sig = sig if Cout == 1 else None
    hip.deconv3x3_s2_out(xd, wd, bd, logits, cls, use_sig, Fn, H, W, Cout)
    torch.cuda.synchronize()
    lg, cl, sg = logits.cpu(), cls.cpu(), sig.cpu()
    assert bool((lg[npos * Cout:] == SENT).all()) and bool((cl[npos:] == 77).all())
    got = lg[:npos * Cout].reshape(Fn, Ho, Wo, Cout)
    fp.check32(got, y, mag, c_bar, cap, what=what)
    # class map against the float64 argmax where the float64 margin is decisive
    want = y.argmax(-1)
    if Cout > 1:
        top = torch.topk(y, 2, dim=-1)
        # (twice the larger of the two contenders' bounds)
        decisive = (top.values[..., 0] - top.values[..., 1]) > 2 * torch.gather(bound, -1, top.indices).max(-1).values
        left_out = 1.0 - float(decisive.double().mean())
        print("%s: %.4f %% of positions left out of the class-map comparison (cap 0.1 %%)" % (what, 100 * left_out))
        assert left_out <= 1e-3
    else:
        decisive = torch.ones_like(want, dtype=torch.bool)
    got_cls = cl[:npos].reshape(Fn, Ho, Wo).long()
    assert bool((got_cls[decisive] == want[decisive]).all())
    assert bool((got_cls < Cout).all())
    # a tie goes to the lowest index: the kernel's class is never above another channel with the same fp32 logit
    same = got == got.gather(-1, got_cls[..., None])
    assert bool((same.long().argmax(-1) == got_cls).all())
    if Cout == 1:
        y1 = y[..., 0].numpy()
        emu = ref.sigmoid_f32(y1.astype(np.float32)).astype(np.float64)
        exact32 = 1.0 / (1.0 + np.exp(-y1.astype(np.float32).astype(np.float64)))
        c = 2.0 * float(np.abs(emu - exact32).max() / fp.U)
        print("%s: sigmoid c = %.3f units of 2^-24 (twice the fp32 emulation's worst error)" % (what, c))
        assert 0 < c <= 8                                                 # exp, add, divide: a handful of roundings of values <= 1
        s64 = 1.0 / (1.0 + np.exp(-y1))
        gs = sg[:npos].reshape(Fn, Ho, Wo).numpy().astype(np.float64)
        lim = bound[..., 0].numpy() / 4 + c * fp.U
        ex = np.abs(gs - s64) / lim
        print("%s: sigmoid worst |got - s64| / bound = %.3f" % (what, ex.max()))
        assert np.isfinite(gs).all() and ex.max() <= 1.0
        assert bool((sg[npos:] == SENT).all())
    else:
        assert bool((sg == SENT).all())                                   # null pointer: nothing written
    # null output pointers leave their buffers alone; what is written has the same bits
    logits2 = torch.full_like(logits, SENT)
    cls2 = torch.full_like(cls, 77)
    hip.deconv3x3_s2_out(xd, wd, bd, None, cls2, None, Fn, H, W, Cout)
    hip.deconv3x3_s2_out(xd, wd, bd, logits2, None, None, Fn, H, W, Cout)
    torch.cuda.synchronize()
    assert torch.equal(cls2, cls) and torch.equal(logits2.view(torch.int32), logits.view(torch.int32))
    cls3 = torch.full_like(cls, 77)
    logits3 = torch.full_like(logits, SENT)
    if Cout == 1:
        sig3 = torch.full_like(sig, SENT)
        hip.deconv3x3_s2_out(xd, wd, bd, None, None, sig3, Fn, H, W, Cout)
        torch.cuda.synchronize()
        assert torch.equal(sig3.view(torch.int32), sig.view(torch.int32))
    assert bool((cls3 == 77).all()) and bool((logits3 == SENT).all())


# ----------------------------------------------------------------------------- the whole decode
@pytest.fixture(scope="module")
def whole(golden):
    g, enc = golden("decode_native"), golden("enc_native")
    sd = synth.decoder_state(int(g["seed"]))
    lat = torch.from_numpy(enc["latent"])
    speeds = torch.from_numpy(g["speeds"])
    o64, o64n = ref.decode(sd, lat, speeds), ref.decode(sd, lat, None)
    dec = decoder.DANetDecoderHIP(sd, dev(), max_frames=4)
    return dict(g=g, sd=sd, lat=lat, speeds=speeds, o64=o64, o64n=o64n, dec=dec)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    for x, y in zip(a, b):
        assert (x is None) == (y is None)
        if x is not None:
            assert torch.equal(_bits(x), _bits(y))


def test_decode_against_the_golden(whole):
    g, dec, o64 = whole["g"], whole["dec"], whole["o64"]
    lat = whole["lat"].to(dev())
    r = dec.decode(lat, speed=whole["speeds"], seg_logits=True)
    torch.cuda.synchronize()
    assert r.seg.dtype == torch.uint8 and tuple(r.seg.shape) == (2, 144, 256) and tuple(r.route.shape) == (2, 144, 256)
    assert r.light_state.dtype == torch.int32 and tuple(r.bc.shape) == (2, 2) and tuple(r.seg_logits.shape) == (2, 144, 256, 8)
    mine = dict(rf=dec.rf[:2].reshape(2, 5, 8, 512).permute(0, 3, 1, 2), seg1=dec.maps[0][:2 * 9 * 16 * 256].reshape(2, 9, 16, 256).permute(0, 3, 1, 2),
                seg=r.seg_logits.permute(0, 3, 1, 2), route=r.route[:, None], light=r.light_logits, steer=r.bc[:, 0], throttle=r.bc[:, 1])
    mine = ref.subsample({k: v.cpu() for k, v in mine.items()})
    want64 = ref.subsample(o64)
    for k in ("rf", "seg1", "seg", "route", "light", "steer", "throttle"):
        e_gold, e_mine = ref.rel_max(g[k], want64[k]), ref.rel_max(mine[k], want64[k])
        print("%-8s rel-max against float64: decode %.3e, golden (fp32 reference) %.3e" % (k, e_mine, e_gold))
        assert np.isfinite(mine[k]).all() and e_gold > 0 and e_mine <= 8 * e_gold, k
    # directly: the light state, and the controls within the triangle inequality of the bar above
    assert np.array_equal(r.light_state.cpu().numpy(), g["light_state"])
    for k in ("steer", "throttle"):
        assert ref.rel_max(mine[k], g[k]) <= 9 * ref.rel_max(g[k], want64[k])
    # the class map is the argmax of the decoder's own logits, lowest index first
    first_max = (r.seg_logits == r.seg_logits.max(-1, keepdim=True).values).long().argmax(-1)
    assert torch.equal(r.seg.long(), first_max)
    # without a speed
    r0 = dec.decode(lat, want=("bc",))
    o64n = whole["o64n"]
    for i, k in enumerate(("steer", "throttle")):
        gk = g[k + "_nospeed"]
        e_gold, e_mine = ref.rel_max(gk, o64n[k]), ref.rel_max(r0.bc[:, i].cpu(), o64n[k])
        print("%-8s (no speed) decode %.3e, golden %.3e" % (k, e_mine, e_gold))
        assert e_mine <= 8 * e_gold and ref.rel_max(r0.bc[:, i].cpu(), gk) <= 9 * e_gold
    assert r0.seg is None and r0.route is None and r0.light_logits is None and r0.seg_logits is None


def test_decode_is_batch_invariant_chunked_and_strided(whole):
    dec = whole["dec"]
    r = np.random.RandomState(5)
    lat5 = torch.cat([whole["lat"], torch.from_numpy((r.standard_normal((3, 512)) * 0.5).astype(np.float32))]).to(dev())
    sp5 = torch.tensor([3.0, 0.5, 0.0, 7.5, 1.25])
    one = dec.decode(lat5[:1], speed=sp5[:1], seg_logits=True)
    three = dec.decode(lat5[:3], speed=sp5[:3], seg_logits=True)
    _same([t[:1] for t in three], one)
    five = dec.decode(lat5, speed=sp5, seg_logits=True)                     # max_frames = 4: two chunks
    dec2 = decoder.DANetDecoderHIP(whole["sd"], dev(), max_frames=2)        # three chunks
    _same(dec2.decode(lat5, speed=sp5, seg_logits=True), five)
    _same([t[:3] for t in five], three)
    # strided rows (a storage's 544-float rows), sentinels in the other columns
    wide = torch.full((5, 544), SENT, device=dev())
    wide[:, :512] = lat5
    _same(dec.decode(wide, speed=sp5, seg_logits=True), five)
    assert bool((wide[:, 512:] == SENT).all())
    # only what is wanted runs: ("bc",) launches no deconvolution and gives the full call's bits
    from cadre_amd import hip
    n0 = hip.N_CALLS
    bc = dec.decode(lat5, speed=sp5, want=("bc",))
    assert hip.N_CALLS - n0 == 2                                           # cadre_bc_head, once per chunk of four rows
    assert torch.equal(_bits(bc.bc), _bits(five.bc))
    seg_only = dec.decode(lat5, want=("seg",))
    assert torch.equal(seg_only.seg, five.seg) and seg_only.route is None and seg_only.bc is None
    route_only = dec.decode(lat5, want=("route",))
    assert torch.equal(_bits(route_only.route), _bits(five.route))
    light_only = dec.decode(lat5, want=("light",))
    assert torch.equal(light_only.light_state, five.light_state) and torch.equal(_bits(light_only.light_logits), _bits(five.light_logits))
    torch.cuda.synchronize()


def test_decoder_refuses_what_it_cannot_take(whole):
    from cadre_amd import hip
    dec = whole["dec"]
    sd = dict(whole["sd"])
    first = synth.decoder_spec()[0][0]
    del sd[first]
    with pytest.raises(hip.CadreHipError, match=first.replace(".", r"\.")):
        decoder.DANetDecoderHIP(sd, dev())
    extra = dict(whole["sd"])
    extra["visual_branch.reverse_lidar.0.weight"] = np.zeros((512, 256, 3, 3), np.float32)
    assert decoder.DANetDecoderHIP(extra, dev(), max_frames=1).ignored_keys == ["visual_branch.reverse_lidar.0.weight"]
    with pytest.raises(hip.CadreHipError):
        dec.decode(whole["lat"])                                           # a CPU tensor
    with pytest.raises(hip.CadreHipError):
        dec.decode(torch.zeros(2, 511, device=dev()))
    with pytest.raises(hip.CadreHipError):
        dec.decode(whole["lat"].to(dev()), want=("depth",))


def test_agent_decode_bc_controls_and_light_state():
    from tests.test_act_batch_gpu import obs_of
    from ppo_agent.agent import CadreAgent
    from ppo_agent.imitation import controls_to_bins
    H = W = 84
    fh, fw = synth.feat_hw(H, W)
    state = dict(synth.encoder_state(fh, fw, 7))
    state.update(synth.decoder_state(7))
    cfg = dict(use_lstm=True, vae_device=0, device_num=0, vae_params="CoPM", measurement_dim=18, num_output=dict(steer=33, throttle=3),
               command_num=4, obs_hw=(H, W), weights_init="none", vae_state_dict=state)
    steer_tab, thr_tab = {i: (i - 16) / 16.0 for i in range(33)}, {0: [0, 0], 1: [0, 1], 2: [0.6, 0]}
    agent = CadreAgent(rank=0, model_cfg=cfg, frame=8, STEER_CONTROL=steer_tab, THROTTLE_CONTROL=thr_tab, ent_coeff=0.01, value_coeff=0.1,
                       clip_coeff=1.0, clip=0.1)
    agent.arena.load_numpy_state(synth.ppo_state(11))
    td = synth.synth_rollout(1, H, W, seed=77)[0]
    assert agent._decoder is None
    before = agent.act(obs_of(td), deterministic=True)
    assert agent._decoder is None                                          # act allocates no decoder
    lat = agent.get_latent_feature(obs_of(td))                             # fresh rows of 544 floats: a view the caller may keep
    want = agent.decoder().decode(lat, want=("light", "bc"))
    steer, throttle = agent.bc_controls(obs_of(td))
    assert torch.equal(_bits(steer), _bits(want.bc[:, 0])) and torch.equal(_bits(throttle), _bits(want.bc[:, 1]))
    assert int(agent.light_state(obs_of(td))) == int(want.light_state[0])
    sp = torch.linspace(0.0, 7.0, lat.shape[0])
    s2, t2 = agent.bc_controls(obs_of(td), speed=sp)
    w2 = agent.decoder().decode(lat, speed=sp, want=("bc",))
    assert torch.equal(_bits(s2), _bits(w2.bc[:, 0])) and not torch.equal(s2, steer)
    full = agent.decode(obs_of(td))
    assert tuple(full.seg.shape) == (lat.shape[0], 144, 256) and torch.equal(_bits(full.bc), _bits(want.bc))
    assert torch.equal(agent.decode(lat, want=("light",)).light_state, want.light_state)       # latent rows go in as they are
    # the encoder's own controls as imitation labels
    b_s, b_t = controls_to_bins(steer.cpu().numpy(), throttle.cpu().numpy(), np.zeros(lat.shape[0]), steer_tab, thr_tab)
    assert b_s.shape == b_t.shape == (lat.shape[0],) and 0 <= b_s.min() and b_s.max() < 33 and b_t.max() < 3
    after = agent.act(obs_of(td), deterministic=True)
    for a, b in zip(before[1] + before[2] + before[3], after[1] + after[2] + after[3]):
        assert torch.equal(_bits(a) if a.dtype == torch.float32 else a, _bits(b) if b.dtype == torch.float32 else b)
    assert torch.equal(_bits(before[0].contiguous()), _bits(after[0].contiguous()))
