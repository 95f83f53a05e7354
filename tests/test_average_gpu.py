"""GPU: weight averaging.  A: cadre_ema_update, cadre_arena_swap and cadre_arena_mean alone on synthetic buffers, against
the float64 statements of tests/average_ref.py; B: through the layers — the learner's optimiser step, the KL gate,
averaged_weights(), averaged snapshots, soup, checkpoints and train_vec."""
import os

import numpy as np
import pytest
import torch

from tests import average_ref as ref

pytestmark = pytest.mark.gpu

LENS = (1, 7, 256, 4099)          # odd sizes, one below a vector, several workgroups' worth, head and tail words
FRONT, BACK = 3, 5                # sentinel floats around the segments


@pytest.fixture(scope="module")
def hip():
    from cadre_amd import hip as h
    h.lib()
    return h


def bits(t):
    return t.detach().contiguous().view(-1).view(torch.int32)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def np_bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ----------------------------------------------------------------------------- A1: cadre_ema_update
class Ema(object):
    """Segments of LENS inside one allocation each for p and e, FRONT sentinel floats before and BACK behind; shift: both
    buffers start that many floats past the allocation's 16-byte boundary."""

    def __init__(self, hip, shift=0, decay=0.9, warmup=True, seed=0, equal=False, lens=LENS):
        r = np.random.RandomState(seed)
        self.hip, self.lens = hip, lens
        self.offs = np.concatenate([[FRONT], FRONT + np.cumsum(lens)]).astype(np.int64)
        n = int(self.offs[-1]) + BACK
        self.p_h = r.standard_normal(n).astype(np.float32)
        self.e_h = self.p_h.copy() if equal else (self.p_h + 0.1 * r.standard_normal(n)).astype(np.float32)
        self._p = torch.zeros(n + shift, device="cuda")
        self._e = torch.zeros(n + shift, device="cuda")
        assert self._p.data_ptr() % 16 == 0 and self._e.data_ptr() % 16 == 0
        self.p, self.e = self._p[shift:], self._e[shift:]
        self.p.copy_(torch.from_numpy(self.p_h))
        self.e.copy_(torch.from_numpy(self.e_h))
        self.seg = torch.from_numpy(self.offs).cuda()
        M = len(lens)
        st = np.zeros(hip.EMA_HEAD + M)
        st[hip.EMA_DECAY], st[hip.EMA_WARMUP] = decay, 1.0 if warmup else 0.0
        st[hip.EMA_HEAD:] = -7.0                                       # (junk: an applied update overwrites it)
        self.state = torch.from_numpy(st).cuda()
        self.work = torch.full((hip.EMA_WORK_HEAD + M * hip.EMA_GRID,), float("nan"), dtype=torch.float64, device="cuda")

    def update(self, stop="null"):
        h = self.hip
        flag = None if stop == "null" else torch.tensor([int(stop)], dtype=torch.int32, device="cuda")
        h.check(h.lib().cadre_ema_update(h.ptr(self.p), h.ptr(self.e), h.ptr(self.seg), len(self.lens), h.ptr(self.state),
                                         h.ptr(self.work), h.ptr(flag), h.stream()), "cadre_ema_update")
        torch.cuda.synchronize()
        return self.e.cpu().numpy(), self.state.cpu().numpy()


@pytest.mark.parametrize("shift", [0, 1])
def test_ema_update_values_sentinels_and_distance(hip, shift):
    c = Ema(hip, shift=shift, decay=0.9, warmup=True, seed=3 + shift)
    lo, hi = int(c.offs[0]), int(c.offs[-1])
    e0 = c.e_h
    for n_upd in range(3):                                           # warm-up decays 0.1, 2/11, 0.25: three different om
        e1, st = c.update()
        d = ref.decay_used(0.9, n_upd)
        assert st[hip.EMA_D] == d and st[hip.EMA_COUNT] == n_upd + 1 and st[hip.EMA_SKIPPED] == 0
        E, bound = ref.ema_expected(c.p_h[lo:hi], e0[lo:hi], d)
        err = np.abs(e1[lo:hi].astype(np.float64) - E)
        print("shift %d update %d: max |e - E| / bound = %.3f" % (shift, n_upd, float((err / bound).max())))
        assert (err <= bound).all()
        assert np_bits_equal(e1[:lo], c.e_h[:lo]) and np_bits_equal(e1[hi:], c.e_h[hi:])       # sentinels of e
        assert np_bits_equal(c.p.cpu().numpy(), c.p_h)                                       # p is only read
        want, counts = ref.dist2(c.p_h, e1, c.offs)
        got = st[hip.EMA_HEAD:]
        for m, (g, w, cnt) in enumerate(zip(got, want, counts)):
            print("  model %d (n = %d): dist2 %.17g, numpy %.17g, rel %.3g" % (m, cnt, g, w, abs(g - w) / w))
            assert abs(g - w) <= cnt * 2.0 ** -53 * w, (m, g, w)
        e0 = e1
    assert not np_bits_equal(e1[lo:hi], c.e_h[lo:hi])


def test_ema_update_stationary(hip):
    """p == e leaves e bit for bit and gives dist2 == 0.0 exactly."""
    for shift in (0, 1):
        c = Ema(hip, shift=shift, seed=8, equal=True)
        c.e_h[5] = c.p_h[5] = np.float32(-0.0)                      # (a negative zero keeps its sign)
        c.p.copy_(torch.from_numpy(c.p_h)); c.e.copy_(torch.from_numpy(c.e_h))
        e1, st = c.update()
        assert np_bits_equal(e1, c.e_h)
        assert (st[hip.EMA_HEAD:] == 0.0).all() and not np.signbit(st[hip.EMA_HEAD:]).any() and st[hip.EMA_COUNT] == 1


def test_ema_update_gate(hip):
    c = Ema(hip, seed=5)
    c.update()                                                       # one applied update: EMA_D and dist2 hold values
    e1, st1 = c.e.cpu().numpy(), c.state.cpu().numpy()
    e2, st2 = c.update(stop=1)
    assert np_bits_equal(e2, e1)
    keep = [k for k in range(len(st1)) if k != hip.EMA_SKIPPED]
    assert np_bits_equal(st2[keep], st1[keep]) and st2[hip.EMA_SKIPPED] == st1[hip.EMA_SKIPPED] + 1 == 1
    e3, st3 = c.update(stop=1)
    assert np_bits_equal(e3, e1) and st3[hip.EMA_SKIPPED] == 2 and st3[hip.EMA_COUNT] == 1
    # stop = NULL and *stop = 0 give identical bits
    a, b = Ema(hip, seed=6), Ema(hip, seed=6)
    ea, sa = a.update()
    eb, sb = b.update(stop=0)
    assert np_bits_equal(ea, eb) and np_bits_equal(sa, sb)


@pytest.mark.parametrize("warmup", [True, False])
def test_ema_update_warmup_sequence(hip, warmup):
    c = Ema(hip, decay=0.5, warmup=warmup, seed=2, lens=(1, 7))
    got = [c.update()[1][hip.EMA_D] for _ in range(21)]
    want = ref.warmup_sequence(0.5, 21, warmup)
    assert got == want, (got, want)
    assert (want[7] < 0.5 and want[8] == 0.5) if warmup else want == [0.5] * 21
    assert c.state.cpu().numpy()[hip.EMA_COUNT] == 21


def test_ema_update_is_deterministic(hip):
    runs = []
    for _ in range(2):
        c = Ema(hip, shift=1, seed=12)
        out = [c.update() for _ in range(2)]
        runs.append(out)
    for (e_a, s_a), (e_b, s_b) in zip(*runs):
        assert np_bits_equal(e_a, e_b) and np_bits_equal(s_a, s_b)


def test_ema_update_one_model_many_workgroups(hip):
    """One segment longer than one pass of the model's grid (2 x 256 x 256 vectors), off the 16-byte grid on both sides."""
    n = 4 * 2 * hip.EMA_GRID * 256 + 4 * 256 + 6
    c = Ema(hip, shift=1, seed=4, lens=(n,), decay=0.75, warmup=False)
    lo, hi = int(c.offs[0]), int(c.offs[-1])
    e1, st = c.update()
    E, bound = ref.ema_expected(c.p_h[lo:hi], c.e_h[lo:hi], 0.75)
    assert (np.abs(e1[lo:hi].astype(np.float64) - E) <= bound).all()
    assert np_bits_equal(e1[:lo], c.e_h[:lo]) and np_bits_equal(e1[hi:], c.e_h[hi:])
    want, counts = ref.dist2(c.p_h, e1, c.offs)
    assert abs(st[hip.EMA_HEAD] - want[0]) <= counts[0] * 2.0 ** -53 * want[0]


# ----------------------------------------------------------------------------- A2: cadre_arena_swap
@pytest.mark.parametrize("n", [0, 1, 3, 5, 4099])
def test_arena_swap(hip, n):
    G = 8                                                          # sentinel words (a multiple of 4: shift 0 is 16-byte aligned)
    r = np.random.RandomState(n)
    for sa in (0, 1):
        for sb in (0, 1):                                          # aligned or not on each side: all four combinations
            a_h, b_h = (r.randint(0, 2 ** 32, size=n + 2 * G + s, dtype=np.uint64).astype(np.uint32).view(np.int32) for s in (sa, sb))
            A, B = torch.from_numpy(a_h.copy()).cuda(), torch.from_numpy(b_h.copy()).cuda()
            a, b = A[G + sa:G + sa + n].view(torch.float32), B[G + sb:G + sb + n].view(torch.float32)
            assert A.data_ptr() % 16 == 0 and B.data_ptr() % 16 == 0
            assert n == 0 or (a.data_ptr() % 16 == 4 * sa and b.data_ptr() % 16 == 4 * sb)      # (an empty view has no address)
            call =lambda: hip.check(hip.lib().cadre_arena_swap(a.data_ptr(), b.data_ptr(), n, hip.stream()), "cadre_arena_swap")
            call()
            wa, wb = a_h.copy(), b_h.copy()
            wa[G + sa:G + sa + n], wb[G + sb:G + sb + n] = b_h[G + sb:G + sb + n], a_h[G + sa:G + sa + n]
            assert np.array_equal(A.cpu().numpy(), wa) and np.array_equal(B.cpu().numpy(), wb), (n, sa, sb)
            call()
            assert np.array_equal(A.cpu().numpy(), a_h) and np.array_equal(B.cpu().numpy(), b_h), (n, sa, sb)


def test_arena_swap_refuses_overlap(hip):
    t = torch.arange(64, dtype=torch.float32, device="cuda")
    keep = t.clone()
    for off in (0, 1, 15):
        rc = hip.lib().cadre_arena_swap(t.data_ptr(), t.data_ptr() + 4 * off, 16, hip.stream())
        assert rc < 0 and b"overlap" in hip.lib().cadre_last_error()
    assert hip.lib().cadre_arena_swap(t.data_ptr(), t.data_ptr() + 4 * 16, 16, hip.stream()) == 0      # adjacent is fine
    torch.cuda.synchronize()
    assert torch.equal(t[:16], keep[16:32]) and torch.equal(t[16:32], keep[:16]) and torch.equal(t[32:], keep[32:])


# ----------------------------------------------------------------------------- A3: cadre_arena_mean
def _mean(hip, srcs, weights, out, n):
    table = torch.tensor([s.data_ptr() for s in srcs], dtype=torch.int64).cuda()
    w = torch.tensor(weights, dtype=torch.float64).cuda()
    hip.check(hip.lib().cadre_arena_mean(hip.ptr(table), hip.ptr(w), len(srcs), out.data_ptr(), n, hip.stream()), "cadre_arena_mean")
    torch.cuda.synchronize()


def _guarded(host, shift=0, G=4):
    buf = torch.full((host.size + 2 * G + shift,), 777.0, device="cuda")
    v = buf[G + shift:G + shift + host.size]
    v.copy_(torch.from_numpy(host))
    return buf, v


def _guards_ok(buf, v, G=4):
    off = (v.data_ptr() - buf.data_ptr()) // 4
    return bool((buf[:off] == 777.0).all() and (buf[off + v.numel():] == 777.0).all())


@pytest.mark.parametrize("n", [1, 5, 4099])
def test_arena_mean(hip, n):
    r = np.random.RandomState(n)
    x = r.standard_normal(n).astype(np.float32)
    x[0] = np.float32(-0.0)
    # K = 1 with weight 1 is a bit copy; K = 2 and K = 4 over equal inputs at 1 / K reproduce the input bit for bit
    for K in (1, 2, 4):
        for shift in (0, 1):
            srcs = [_guarded(x, s % 4)[1] for s in range(K)]      # (the sources at every alignment)
            buf, out = _guarded(np.zeros(n, np.float32), shift)
            _mean(hip, srcs, [1.0 / K] * K, out, n)
            assert np_bits_equal(out.cpu().numpy(), x) and _guards_ok(buf, out), (K, shift)
    # K = 3 on random inputs with weights (0.5, 0.3, 0.2): within 1 fp32 ulp of the float64 statement
    hs = [r.standard_normal(n).astype(np.float32) * s for s in (1.0, 3.0, 0.01)]
    w = (0.5, 0.3, 0.2)
    want = ref.mean64(hs, w)
    outs = []
    for shift in (0, 3):
        srcs = [_guarded(h, k)[1] for k, h in enumerate(hs)]
        buf, out = _guarded(np.zeros(n, np.float32), shift)
        _mean(hip, srcs, w, out, n)
        got = out.cpu().numpy()
        assert (np.abs(got.astype(np.float64) - want) <= ref.ulp32(want)).all() and _guards_ok(buf, out)
        outs.append(got)
        # out == src_0 gives the same bits as a separate out
        buf0, s0 = _guarded(hs[0], shift)
        _mean(hip, [s0] + srcs[1:], w, s0, n)
        assert np_bits_equal(s0.cpu().numpy(), got) and _guards_ok(buf0, s0)
        for k in (1, 2):
            assert np_bits_equal(srcs[k].cpu().numpy(), hs[k])      # the other sources are only read
    assert np_bits_equal(outs[0], outs[1])


# ----------------------------------------------------------------------------- B: through the layers
def _agent(**kw):
    from tests.test_checkpoint_gpu import _agent as make
    return make(**kw)


def _step(agent, smp, lr=1e-3):
    from tests.test_checkpoint_gpu import _step as step
    step(agent, smp, lr)


@pytest.fixture(scope="module")
def smps():
    from tests.test_ppo_stats_gpu import samples
    return [samples(64, 4, 1 + i) for i in range(5)]


def _with_average(agent, decay=0.9, warmup=True):
    from cadre_amd.average import WeightAverage
    avg = WeightAverage(agent, decay=decay, warmup=warmup)
    agent.learner.set_weight_average(avg)
    return avg


def _arena_bits(agent):
    a = agent.arena
    return dict(params=a.params.clone(), exp_avg=a.exp_avg.clone(), exp_avg_sq=a.exp_avg_sq.clone(), step_dev=a.step_dev.clone())


@pytest.fixture(scope="module")
def trained(smps):
    """Five update + clip_adam steps (graphs on: the warm, capture and replay paths all run) without and with an average; the
    second run records the average before and the parameters after every step."""
    plain = _agent()
    assert plain.learner.use_graphs
    keys0 = None
    for s in smps:
        _step(plain, s)
    keys0 = set(plain.learner._graphs)
    avged = _agent()
    avg = _with_average(avged)
    steps = []
    for s in smps:
        before = avg.ema.clone()
        _step(avged, s)
        steps.append((before, avged.arena.params.clone(), avg.ema.clone(), avg.state.clone()))
    torch.cuda.synchronize()
    return plain, avged, avg, steps, keys0


def test_training_is_not_perturbed(hip, trained):
    plain, avged, avg, steps, keys0 = trained
    want, got = _arena_bits(plain), _arena_bits(avged)
    for k in want:
        assert same(got[k], want[k]), k
    for i, (before, params, after, state) in enumerate(steps):
        st = state.cpu().numpy()
        assert st[hip.EMA_COUNT] == i + 1 and st[hip.EMA_D] == ref.decay_used(0.9, i) and st[hip.EMA_SKIPPED] == 0
        E, bound = ref.ema_expected(params.cpu().numpy(), before.cpu().numpy(), st[hip.EMA_D])
        assert (np.abs(after.cpu().numpy().astype(np.float64) - E) <= bound).all(), i
        d2, counts = ref.dist2(params.cpu().numpy(), after.cpu().numpy(), avg._offs)
        for g, w, cnt in zip(st[hip.EMA_HEAD:], d2, counts):
            assert abs(g - w) <= cnt * 2.0 ** -53 * w
    assert int(avg.state[hip.EMA_COUNT].item()) == 5 == avged.arena.step
    # the graph key gains one element; without an average the keys are what they are without the module
    adam = lambda keys: sorted((k for k in keys if k and k[0] == "adam"), key=len)
    ema_key = ("ema", avg.ema.data_ptr(), avg.state.data_ptr(), avg.work.data_ptr())       # every address the graph holds
    assert all(ema_key == k[-1] for k in adam(avged.learner._graphs))
    assert [k[:-1] for k in adam(avged.learner._graphs)] == adam(keys0) and not any("ema" in str(k) for k in keys0)
    s = avg.summary()
    assert s["updates"] == 5 and s["skipped"] == 0 and s["decay_used"] == ref.decay_used(0.9, 4)
    assert sorted(s["distance"]) == sorted(avged.arena.model_names()) and all(v[0] > 0 and v[1] > 0 for v in s["distance"].values())
    assert avg.distance() == s["distance"]
    from cadre_amd.hip import CadreHipError
    with pytest.raises(CadreHipError, match="weight average"):
        avged.learner.clip_adam_sharded(0, avged.arena.total, lambda t: None)
    with pytest.raises(CadreHipError, match="another arena"):
        plain.learner.set_weight_average(avg)


def test_state_dict_round_trip_and_set_decay(hip, trained):
    from cadre_amd.average import WeightAverage
    _plain, avged, avg, _steps, _keys = trained
    sd = avg.state_dict()
    other = WeightAverage(avged, decay=0.5, warmup=False)
    other.load_state_dict(sd)
    assert same(other.ema, avg.ema) and same(other.state, avg.state)
    with pytest.raises(ValueError, match="missing"):
        other.load_state_dict({"ema": sd["ema"]})
    assert other.set_decay(0.25) == 0.25 and float(other.state[hip.EMA_DECAY].item()) == 0.25
    assert float(avg.state[hip.EMA_DECAY].item()) == 0.9
    with pytest.raises(ValueError, match="decay"):
        other.set_decay(1.0)


def test_gated_step_is_skipped_and_counted(hip):
    """target_kl set so that the gate closes at step k of 8: the average of the gated section equals, bit for bit, the one of
    a manual loop that takes the first k optimiser steps only; the skipped steps are counted, and after the section has
    reconciled arena.step it equals EMA_COUNT."""
    from ppo_agent.chief import chief_step
    from ppo_agent.models import Shared_grad_buffers
    from ppo_agent.train import learner_section
    from tests.test_learner_gpu import make_agent
    from tests.test_ppo_stats_gpu import cfg, storages

    def section(target_kl, stats, average):
        agent = make_agent(84, 84)
        avg = _with_average(agent) if average else None
        shared = Shared_grad_buffers(agent.model_dict, agent.device)
        pair = storages(64, 2, 21)
        torch.manual_seed(9)
        learner_section(agent, pair[0], pair[1], False, cfg(target_kl=target_kl), shared, stats=stats)
        torch.cuda.synchronize()
        return agent, avg
    st0 = {}
    section(None, st0, False)
    kl = [max(r["approx_kl"]) for r in st0["rows"]]
    k = next((j for j in range(1, len(kl)) if kl[j] > max(kl[:j])), None)
    assert k is not None, kl
    st = {}
    agent, avg = section((max(kl[:k]) + kl[k]) / 2 / 1.5, st, True)
    assert st["stopped_at_step"] == k and st["weight_average"]["updates"] == k and st["weight_average"]["skipped"] == 8 - k
    state = avg.state.cpu().numpy()
    assert agent.arena.step == k == state[hip.EMA_COUNT] and state[hip.EMA_SKIPPED] == 8 - k
    assert state[hip.EMA_D] == ref.decay_used(0.9, k - 1)
    # the manual loop: the same draws, chief_step after the first k steps only
    other = make_agent(84, 84)
    avg2 = _with_average(other)
    shared = Shared_grad_buffers(other.model_dict, other.device)
    pair = storages(64, 2, 21)
    torch.manual_seed(9)
    nv_s, nv_t = other.get_value(False, pair[0].get_last(as_tensor=True), pair[1].get_last(as_tensor=True))
    adv = [pair[0].compute_returns(nv_s), pair[1].compute_returns(nv_t)]
    step = 0
    for _ in range(4):
        i_s, i_t = pair[0].sample_indices(), pair[1].sample_indices()
        for a, b in zip(i_s, i_t):
            other.update_policy_from_storages([(pair[0], a, adv[0], pair[1], b, adv[1])], sync=False)
            if step < k:
                shared.add_gradient(other.model_dict)
                chief_step(shared, None, 250.0, zero_grads=False)
            step += 1
    torch.cuda.synchronize()
    assert same(other.arena.params, agent.arena.params)
    assert same(avg2.ema, avg.ema)                                    # the skipped steps left the average bit for bit
    s2 = avg2.state.cpu().numpy()
    assert s2[hip.EMA_SKIPPED] == 0 and np_bits_equal(np.delete(s2, hip.EMA_SKIPPED), np.delete(state, hip.EMA_SKIPPED))
    from ppo_agent.train import stats_line
    assert ", average: %d updates (%d skipped)" % (k, 8 - k) in stats_line(0, st)


def _obs(N=2):
    from tests.test_act_batch_gpu import env_streams, obs_of
    streams, _r = env_streams(N, 84, 84, 4, 1)
    return lambda: [obs_of(streams[e][0]) for e in range(N)]


def _act_bits(outs):
    return [(f.clone(), [x.clone() for x in a], [x.clone() for x in lp], [x.clone() for x in v]) for f, a, lp, v, _h in outs]


def _same_acts(x, y):
    for (f0, a0, l0, v0), (f1, a1, l1, v1) in zip(x, y):
        if not (same(f0, f1) and all(same(p, q) for p, q in zip(a0 + l0 + v0, a1 + l1 + v1))):
            return False
    return len(x) == len(y)


def test_averaged_weights_context(hip, trained, smps):
    from cadre_amd.hip import CadreHipError
    from tests.test_ppo_stats_gpu import dev
    plain, avged, avg, _steps, _keys = trained
    obs = _obs()
    ema0, params0 = avg.ema.clone(), avged.arena.params.clone()
    assert not same(ema0, params0)
    twin = _agent()                                                   # a second agent whose arena holds the average's values
    twin.arena.params.copy_(ema0)
    twin.arena.params[:0].zero_()
    want = _act_bits(twin.act_batch(obs(), deterministic=True))
    live = _act_bits(_agent_like(avged).act_batch(obs(), deterministic=True))
    with avged.averaged_weights() as inside:
        assert inside is avg and avged.learner._avg_swapped
        assert same(avged.arena.params, ema0) and same(avg.ema, params0)
        got = _act_bits(avged.act_batch(obs(), deterministic=True))
        with pytest.raises(CadreHipError, match="inside averaged_weights"):
            avged.update_policy(dev(smps[0][0]), dev(smps[0][1]))
        with pytest.raises(CadreHipError, match="inside averaged_weights"):
            avged.learner.clip_adam(lr=1e-3, max_grad_norm=250.0)
        with pytest.raises(CadreHipError, match="no nested entry"):
            with avged.averaged_weights():
                pass
        assert avged.learner._avg_swapped
    assert _same_acts(got, want)
    assert not _same_acts(got, live)                                  # (the average acts differently from the live weights)
    assert not avged.learner._avg_swapped and same(avged.arena.params, params0) and same(avg.ema, ema0)
    # an exception in the body still restores
    with pytest.raises(KeyError):
        with avged.averaged_weights():
            raise KeyError("x")
    assert not avged.learner._avg_swapped and same(avged.arena.params, params0) and same(avg.ema, ema0)
    # the next update step gives the bits of an agent that never entered the context: the packed weights were re-derived
    from tests.test_ppo_stats_gpu import samples
    extra = samples(64, 4, 77)
    _step(plain, extra)
    _step(avged, extra)
    torch.cuda.synchronize()
    want, got = _arena_bits(plain), _arena_bits(avged)
    for k in want:
        assert same(got[k], want[k]), k
    assert int(avg.state[hip.EMA_COUNT].item()) == 6


def _agent_like(agent):
    twin = _agent()
    twin.arena.params.copy_(agent.arena.params)
    twin.arena.params[:0].zero_()
    return twin


def test_averaged_snapshot(trained, tmp_path):
    from cadre_amd.hip import CadreHipError
    plain, avged, avg, _steps, _keys = trained
    params0 = avged.arena.params.clone()
    avged.save_snapshot(str(tmp_path / "avg.pt"), weights="average")
    avged.save_snapshot(str(tmp_path / "live.pt"))
    assert same(avged.arena.params, params0) and not avged.learner._avg_swapped
    f_avg = torch.load(str(tmp_path / "avg.pt"), map_location="cpu", weights_only=False)
    f_live = torch.load(str(tmp_path / "live.pt"), map_location="cpu", weights_only=False)
    assert sorted(f_avg) == sorted(f_live) and len(f_avg) == 12      # the reference's keys (it never writes throttle_lstm)
    fresh = _agent(ppo_seed=5)
    fresh.load_snapshot(str(tmp_path / "avg.pt"), None)
    n = differ = 0
    for name in f_avg:
        views = avg.views(name)
        for k, p in fresh.model_dict[name].named_parameters():
            assert same(p.data, views[k]), (name, k)
            differ += not same(p.data, avged.arena.views(avged.arena.params, name)[k])
            n += 1
    assert n > 40 and differ > n // 2                                 # (the file holds the average, not the live weights)
    with pytest.raises(CadreHipError, match="no weight average is set"):
        plain.save_snapshot(str(tmp_path / "none.pt"), weights="average")
    assert not os.path.exists(str(tmp_path / "none.pt"))


def test_soup_of_three_snapshots(hip, smps, tmp_path):
    from cadre_amd.average import soup
    from ppo_agent.agent import CadreAgent
    agent = _agent()
    paths = []
    for i in range(3):
        _step(agent, smps[i])
        paths.append(str(tmp_path / ("s%d.pt" % i)))
        agent.save_snapshot(paths[-1], fix_missing_lstm=True)
    files = [torch.load(p, map_location="cpu", weights_only=False) for p in paths]
    into = _agent(ppo_seed=5)
    v0 = into.arena.params._version
    assert soup(paths, into=into) is into
    torch.cuda.synchronize()
    assert into.arena.params._version > v0 and into.learner._wp_key is None
    worst = 0.0
    for name in files[0]:
        for k, p in into.model_dict[name].named_parameters():
            srcs = [f[name].state_dict()[k].numpy() for f in files]
            want = ref.mean64(srcs, [1.0 / 3] * 3)
            err = np.abs(p.data.cpu().numpy().astype(np.float64) - want) / ref.ulp32(want)
            worst = max(worst, float(err.max()))
    print("soup of three snapshots: worst error %.3f fp32 ulp of the float64 mean" % worst)
    assert worst <= 1.0
    # agents and arenas as sources, the destination among them, weights given
    a, b = _agent(ppo_seed=5), _agent(ppo_seed=6)
    pa, pb = a.arena.params.clone(), b.arena.params.clone()
    soup([a, b.arena], weights=(0.25, 0.75))
    want = ref.mean64([pa.cpu().numpy(), pb.cpu().numpy()], (0.25, 0.75))
    assert (np.abs(a.arena.params.cpu().numpy().astype(np.float64) - want) <= ref.ulp32(want)).all() and same(b.arena.params, pb)
    # an EnsembleEvaluator built on the result steps
    outs = CadreAgent.ensemble_act_batch([into], _obs()(), deterministic=True)
    assert outs is not None and np.isfinite(np.asarray(outs.controls, dtype=np.float64)).all()


# ----------------------------------------------------------------------------- checkpoints and train_vec
def test_checkpoint_mismatch_is_refused_and_nothing_moves(smps, tmp_path):
    from cadre_amd import checkpoint
    plain, avged = _agent(), _agent()
    avg = _with_average(avged)
    for ag in (plain, avged):
        _step(ag, smps[0])
    p_plain = checkpoint.capture(plain).save(tmp_path / "plain.pt")
    p_avg = checkpoint.capture(avged).save(tmp_path / "avg.pt")
    s_plain, s_avg = checkpoint.load(p_plain), checkpoint.load(p_avg)
    assert s_plain["weight_average"] is None and s_avg["weight_average"] == dict(decay=0.9, warmup=True)
    assert s_plain["names"] == ["params", "exp_avg", "exp_avg_sq", "step_dev"]
    assert s_avg["names"] == ["params", "exp_avg", "exp_avg_sq", "step_dev", "ema", "ema_state"]
    for ag in (plain, avged):
        _step(ag, smps[1])
    torch.cuda.synchronize()
    live = [_arena_bits(plain), _arena_bits(avged), avg.ema.clone(), avg.state.clone()]
    with pytest.raises(ValueError, match="mismatch in ema"):
        checkpoint.restore(avged, s_plain)                            # taken without the key, restored with it
    with pytest.raises(ValueError, match="mismatch in ema"):
        checkpoint.restore(plain, s_avg)                              # and the other way round
    torch.cuda.synchronize()
    for ag, want in zip((plain, avged), live):
        for k, v in _arena_bits(ag).items():
            assert same(v, want[k]), k
    assert same(avg.ema, live[2]) and same(avg.state, live[3])
    checkpoint.restore(avged, s_avg)                                  # the matching file goes in
    assert same(avg.ema.cpu(), s_avg["tensors"]["ema"]) and same(avg.state.cpu(), s_avg["tensors"]["ema_state"])
    assert same(avged.arena.params.cpu(), s_avg["tensors"]["params"]) and avged.arena.step == 1


def _vec_run(tmp_path, sub, callback, episodes, **kw):
    from ppo_agent.train import train_vec
    from tests.helpers import topology_cfgs
    from tests.test_checkpoint_gpu import _resume_env
    N, T = 2, 8
    (tmp_path / sub).mkdir()
    train_cfg, agent_cfg, env_cfg, rollout_cfg = topology_cfgs(str(tmp_path / sub), H=84, W=84, T=T, episodes=episodes)
    env_cfg.update(num_processes=N, port=[2000 + i for i in range(N)], routes=["r%d" % i for i in range(N)],
                   scenarios=["s"] * N, town=["Town01"] * N)
    env_cfg.update({k: kw.pop(k) for k in ("start_step", "seed_base") if k in kw})
    train_cfg.update(save_interval=10 ** 6, ppo_epoch=1, **kw)
    return train_vec(0, train_cfg, agent_cfg, env_cfg, rollout_cfg, N, env_cls=_resume_env(), callback=callback)


def test_train_vec_resume_with_average_is_bit_exact(hip, tmp_path):
    from tests.test_checkpoint_gpu import _assert_episode, _record
    EP, T = 4, 8
    keys = dict(reward_scaling=True, log_stats=True, adaptive_lr={"desired_kl": 1e-7, "min": 1e-6, "max": 1e-2},
                weight_average={"decay": 0.9})

    def record(kw):
        rec, host = _record(kw["agent"], kw["rollouts"], kw["reward_scaler"], kw["losses"])
        avg = kw["agent"].learner._avg
        rec.update(ema=avg.ema.clone(), ema_state=avg.state.clone())
        return rec, host
    straight, files = {}, {}

    def cb1(event, **kw):
        if event == "update":
            straight[kw["episode"]] = record(kw)
        if event == "checkpoint":
            files[kw["episode"]] = kw["path"]
    agent = _vec_run(tmp_path, "straight", cb1, EP, checkpoint_interval=1, **keys)
    assert sorted(straight) == list(range(EP)) and sorted(files) == list(range(EP))
    st = straight[EP - 1][0]["ema_state"].cpu().numpy()
    assert st[hip.EMA_COUNT] == straight[EP - 1][1]["step"] == agent.arena.step == 2 * EP
    models = os.listdir(str(tmp_path / "straight" / "models"))
    assert sorted(models) == ["ppo_model_0.pt", "ppo_model_0_avg.pt"]         # (save_interval: episode 0 only)
    resumed = []

    def cb3(event, **kw):
        if event == "start":
            assert same(kw["agent"].learner._avg.ema, straight[1][0]["ema"])
        if event == "update":
            _assert_episode(record(kw), straight[kw["episode"]], "resumed, episode %d" % kw["episode"])
            resumed.append(kw["episode"])
    _vec_run(tmp_path, "resumed", cb3, EP, resume_from=files[1], start_step=2 * T, seed_base=31337, **keys)
    assert resumed == [2, 3]
    assert torch.equal(torch.get_rng_state(), straight[EP - 1][1]["rng"])


def test_train_vec_key_absent_launches_nothing(hip, tmp_path):
    """train_vec without the key never calls cadre_ema_update (counted through a wrapper on hip.lib()), and its checkpoints
    carry exactly the names they carried before the key existed."""
    from cadre_amd import checkpoint
    calls = {}
    real = hip.lib()

    class Counting(object):
        def __getattr__(self, name):
            fn = getattr(real, name)
            if not callable(fn) or not name.startswith("cadre_"):
                return fn

            def counted(*a):
                calls[name] = calls.get(name, 0) + 1
                return fn(*a)
            return counted
    files = {}
    hip._lib = Counting()
    try:
        agent = _vec_run(tmp_path, "plain", lambda event, **kw: files.update({kw["episode"]: kw["path"]}) if event == "checkpoint" else None,
                         2, checkpoint_interval=1)
        assert agent.learner._avg is None
        # (host-side calls: the warm run and the capture; the replays of the captured graph make none)
        assert calls.get("cadre_clip_adam_graph", 0) >= 1 and "cadre_ema_update" not in calls and agent.arena.step == 4
        assert "cadre_arena_swap" not in calls and "cadre_arena_mean" not in calls
        calls.clear()
        with_key = _vec_run(tmp_path, "keyed", None, 2, weight_average={"decay": 0.9, "snapshot": False})
        assert calls.get("cadre_ema_update", 0) == calls.get("cadre_clip_adam_graph", 0) >= 1 and with_key.learner._avg is not None
        assert int(with_key.learner._avg.state[hip.EMA_COUNT].item()) == 4 == with_key.arena.step
        assert "cadre_arena_swap" not in calls                           # (snapshot: False)
    finally:
        hip._lib = real
    names = checkpoint.load(files[1])["names"]
    want = ["params", "exp_avg", "exp_avg_sq", "step_dev"] + ["storage%d.%s.%s" % (e, h, k) for e in range(2)
                                                               for h in checkpoint.HEADS for k in checkpoint.STORAGE_TENSORS]
    assert names == want
