"""Curiosity bonus on the device (cadre_amd/curiosity.py, csrc/curiosity.hip): exact properties, float64 parity of every stored element
within the a-priori first-order bound of tests/curiosity_ref.py, behaviour and the training loops with the key.

Shapes: D = 530 (production: 530 = 4 * 128 + 18, a k tail in the last chunk) and 37 (less than one chunk); T = 1, 5, 33 (row tails; 33
crosses one 32-row tile), N = 1, 3; hidden 128, embed 32 and 64."""
import os
import types

import numpy as np
import pytest
import torch

from tests import curiosity_ref as ref
from tests.test_curiosity_cpu import AMBIGUITY_CAP, PARITY_CASES, case_inputs

pytestmark = pytest.mark.gpu
SENT = -7.5
S_LEN, HID = 3, 128


@pytest.fixture(scope="module")
def hip():
    from cadre_amd import hip as h
    h.lib()
    return h


def host(t):
    return t.detach().cpu().numpy()


def storages_of(x, N, T, poison=False, seed=0):
    """N (steer, throttle) pairs whose newest frame rows are the rows of x [N T][D] in (worker, time) order.  poison: NaN in the
    pad columns and in every older frame of every window."""
    from ppo_agent.storage import RolloutStorage
    D = x.shape[1]
    g = torch.Generator()
    g.manual_seed(1000 + seed)
    out = []
    for w in range(N):
        pair = []
        for _h in range(2):
            s = RolloutStorage(T, 1, D, S_LEN, 32, True, 0.99, 0.95, device="cuda")
            s._obs.copy_(torch.randn(s._obs.shape, generator=g))
            if poison:
                s._obs.fill_(float("nan"))
            s.obs[:T, S_LEN - 1].copy_(torch.from_numpy(x[w * T:(w + 1) * T]))
            s.obs[T, S_LEN - 1].fill_(0.25)
            s.rewards.copy_(torch.randn(T + 1, 1, generator=g))
            s.value_preds.copy_(torch.randn(T + 1, 1, generator=g))
            s.masks.fill_(1.0)
            s.step = T
            pair.append(s)
        out.append(tuple(pair))
    return out


def module(D, N, H=HID, E=64, seed=3, coeff=0.5, **kw):
    from cadre_amd.curiosity import Curiosity
    return Curiosity(D, N, coeff=coeff, hidden=H, embed=E, seed=seed, device="cuda", **kw)


def saving_forward(cur, R):
    ws = cur._workspace(R)
    cur._forward(0, R, ws["err"], save=True)
    return ws


# ----------------------------------------------------------------------------- exact properties
@pytest.mark.parametrize("D,N,T,E", [(530, 3, 33, 64), (37, 1, 5, 32), (37, 1, 1, 64)])
def test_equal_towers_give_zero(D, N, T, E):
    """The predictor a copy of the target: err, r_int and every gradient element are exact zeros; mixed == rewards with ext_coeff 1."""
    x = np.random.RandomState(D + T).randn(N * T, D).astype(np.float32)
    st = storages_of(x, N, T)
    cur = module(D, N, E=E, coeff=0.7, update_proportion=1.0)
    cur.predictor.copy_(cur.target)
    err = cur.begin_section(st)
    assert tuple(err.shape) == (N, T) and not bool(err.any())
    for pair in st:
        for s in pair:
            assert torch.equal(s.rewards_mixed[:T], s.rewards[:T])
    cur.grads.fill_(SENT)
    saving_forward(cur, N * T)
    loss = cur.backward(N * T)
    assert not bool(cur.grads.any()) and float(loss[0]) == 0.0 and float(loss[1]) == N * T


def test_beta_zero_is_the_finishing_stage_of_today():
    """ext_coeff 1, coeff 0, nonzero errors: finish_rollouts(intrinsic=) gives the returns, advantages and value_preds[T] of the call
    without it, bit for bit; with coeff > 0 they differ."""
    from ppo_agent.storage import RolloutStorage
    D, N, T = 37, 3, 33
    x = np.random.RandomState(1).randn(N * T, D).astype(np.float32)
    nv = [torch.tensor([0.1 * k], device="cuda") for k in range(2 * N)]
    got = {}
    for tag, coeff in (("plain", None), ("zero", 0.0), ("on", 0.5)):
        st = storages_of(x, N, T)
        flat = [s for p in st for s in p]
        kw = {}
        if coeff is not None:
            cur = module(D, N, coeff=coeff)
            err = cur.begin_section(st)
            assert float(err.min()) > 0
            kw = dict(intrinsic=cur)
        RolloutStorage.finish_rollouts(flat, nv, **kw)
        got[tag] = [(s.returns.clone(), s.advantages.clone(), s.value_preds[T].clone()) for s in flat]
    for a, b, c in zip(got["plain"], got["zero"], got["on"]):
        assert all(torch.equal(u, v) for u, v in zip(a, b))
        assert not torch.equal(a[0], c[0]) and bool(torch.isfinite(c[0]).all()) and bool(torch.isfinite(c[1]).all())
    with pytest.raises(ValueError, match="reward_scaler"):
        from ppo_agent.storage import ReturnScaler
        RolloutStorage.finish_rollouts(flat, nv, intrinsic=cur, reward_scaler=ReturnScaler(N, 0.99, device="cuda"))


def test_batch_invariance():
    """The same feature row alone in a tile and deep inside a larger launch gives the same err bits."""
    D = 530
    rng = np.random.RandomState(9)
    xa, xb = rng.randn(5, D).astype(np.float32), rng.randn(99, D).astype(np.float32)
    xb[70] = xa[2]
    xb[3] = xa[4]
    a, b = module(D, 1), module(D, 3)
    for cur in (a, b):                                   # the same frozen statistics in both
        cur.state[ref.RND_N] = 50.0
        cur.state[ref.RND_HEAD:ref.RND_HEAD + D] = torch.linspace(-0.5, 0.5, D, dtype=torch.float64)
        cur.state[ref.RND_HEAD + D:ref.RND_HEAD + 2 * D] = torch.linspace(30.0, 80.0, D, dtype=torch.float64)
        cur.train(False)
    ea = a.begin_section(storages_of(xa, 1, 5)).reshape(-1)
    eb = b.begin_section(storages_of(xb, 3, 33)).reshape(-1)
    assert float(ea[2]) == float(eb[70]) > 0 and float(ea[4]) == float(eb[3]) and float(ea[0]) != float(eb[0])


def test_bounds_of_what_is_touched(hip):
    """NaN in the pad columns and in the older frames of every window, sentinels behind err [N][T], in rewards_mixed[T] and behind
    the gradient buffer: every output is finite, no sentinel moves, storage.rewards keeps its bits."""
    D, N, T = 530, 3, 33
    R = N * T
    x = np.random.RandomState(4).randn(R, D).astype(np.float32)
    st = storages_of(x, N, T, poison=True)
    flat = [s for p in st for s in p]
    raw = [s.rewards.clone() for s in flat]
    cur = module(D, N, update_proportion=1.0)
    for s in flat:
        cur.mixed_of(s).fill_(SENT)
    big_err = torch.full((R + 64,), SENT, device="cuda")
    cur._err = big_err[:R].view(N, T)
    big_g = torch.full((cur.P + 64,), SENT, device="cuda")
    cur.grads = big_g[:cur.P]
    err = cur.begin_section(st)
    assert err.data_ptr() == big_err.data_ptr()
    ws = saving_forward(cur, R)
    big_s = {k: torch.full((ws[k].numel() + 64,), SENT, device="cuda") for k in ("xh", "h1", "h2", "diff", "scratch")}
    for k, v in big_s.items():
        ws[k] = v[:ws[k].numel()].view(ws[k].shape)
    saving_forward(cur, R)
    cur.backward(R)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(big_err).all()) and bool((big_err[R:] == SENT).all()) and float(big_err[:R].min()) > 0
    assert bool(torch.isfinite(big_g).all()) and bool((big_g[cur.P:] == SENT).all()) and bool((big_g[:cur.P] != SENT).all())
    for k, v in big_s.items():
        n = ws[k].numel()
        assert bool(torch.isfinite(v).all()) and bool((v[n:] == SENT).all()), k
    assert bool(torch.isfinite(cur.state).all())
    for s, r0 in zip(flat, raw):
        assert torch.equal(s.rewards, r0) and float(s.rewards_mixed[T]) == SENT
        assert bool(torch.isfinite(s.rewards_mixed).all()) and bool((s.rewards_mixed[:T] != SENT).all())


def test_determinism_and_the_counter():
    """Two identical calls of each kernel from the same state give identical bits; the mask counter advances by the step's rows."""
    D, N, T = 37, 3, 33
    R = N * T
    x = np.random.RandomState(5).randn(R, D).astype(np.float32)
    st = storages_of(x, N, T)
    cur = module(D, N, E=32, update_proportion=0.5)
    s0 = cur.state.clone()
    out = []
    for _ in range(2):
        cur.state.copy_(s0)
        err = cur.begin_section(st).clone()
        after_section = cur.state.clone()
        ws = saving_forward(cur, R)
        loss = cur.backward(R).clone()
        out.append((err, after_section, torch.cat([s.rewards_mixed[:T] for p in st for s in p]).clone(), ws["xh"].clone(), ws["h1"].clone(),
                    ws["h2"].clone(), ws["diff"].clone(), cur.grads.clone(), loss, cur.state.clone()))
    for a, b in zip(*out):
        assert torch.equal(a, b)
    assert float(out[0][9][ref.RND_CTR]) == float(s0[ref.RND_CTR]) + R
    assert float(out[0][1][ref.RND_N]) == R and float(out[0][8][1]) > 0


def test_mask_draw_and_the_global_generator():
    """sum m is the count of the reference's statement of the generator from the block's key and counter; proportion 1 draws every row,
    0 none (exact zero gradients); nothing draws from torch's global generator."""
    D, N, T = 37, 3, 33
    R = N * T
    x = np.random.RandomState(6).randn(R, D).astype(np.float32)
    torch.manual_seed(123)
    before = torch.get_rng_state().clone()
    for prop in (0.25, 1.0, 0.0):
        st = storages_of(x, N, T)
        cur = module(D, N, E=32, seed=17, update_proportion=prop, epochs=1, minibatches=1)
        cur.begin_section(st)
        cur.state[ref.RND_CTR] = 12345.0
        ws = saving_forward(cur, R)
        cur.grads.fill_(SENT)
        loss = host(cur.backward(R))
        m = ref.mask(17, 12345, R, prop)
        assert loss[1] == m.sum() == {0.25: m.sum(), 1.0: R, 0.0: 0}[prop]
        assert np.array_equal(host(ws["scratch"][:R]) != 0, m)
        e = host(ws["err"][:R]).astype(np.float64)
        assert abs(loss[0] - (m * e).sum() / max(m.sum(), 1)) <= 1e-6 * max(loss[0], 1e-30)
        if prop == 0.0:
            assert not bool(cur.grads.any())
        else:
            assert bool(cur.grads.any()) and bool(torch.isfinite(cur.grads).all())
        cur.update(stats=True)
        assert cur.summary()["steps"] == 1
    assert torch.equal(torch.get_rng_state(), before)


def test_the_step_is_the_existing_optimiser(hip):
    """update() with one step leaves the predictor that cadre_rnd_backward followed by a direct cadre_clip_adam_graph call leaves."""
    D, N, T = 37, 1, 5
    x = np.random.RandomState(7).randn(N * T, D).astype(np.float32)
    st = storages_of(x, N, T)
    cur = module(D, N, E=32, update_proportion=1.0, epochs=1, minibatches=1, lr=1e-3)
    cur.begin_section(st)
    p0, s0 = cur.predictor.clone(), cur.state.clone()
    assert cur.update() == 1 and int(cur.step_dev) == 1
    p1 = cur.predictor.clone()
    assert not torch.equal(p0, p1)
    cur.predictor.copy_(p0)
    cur.state.copy_(s0)
    saving_forward(cur, N * T)
    cur.backward(N * T)
    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    step, norms = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(3, dtype=torch.float64, device="cuda")
    seg = torch.tensor([0, cur.P], dtype=torch.int64).cuda()
    hip.check(hip.lib().cadre_clip_adam_graph(hip.ptr(p), hip.ptr(cur.grads), hip.ptr(m), hip.ptr(v), hip.ptr(seg), 1, hip.ptr(norms), 1e30, 1e-3,
                                              0.9, 0.999, 1e-8, hip.ptr(step), hip.stream()), "cadre_clip_adam_graph")
    assert torch.equal(p, p1) and torch.equal(m, cur.exp_avg) and torch.equal(v, cur.exp_avg_sq)


# ----------------------------------------------------------------------------- float64 parity, every stored element
@pytest.mark.parametrize("D,R,H,E,seed", PARITY_CASES)
def test_parity_of_every_stored_element(D, R, H, E, seed):
    """Statistics at rtol 1e-9; xh, h1, h2, g - f, err, sigma, rewards_mixed and every gradient element within the reference's a-priori
    bound.  The ambiguity cap is asserted from the reference before the device is looked at."""
    N, T = {99: (3, 33), 5: (1, 5), 3: (3, 1)}[R]
    x, (n, mu, M2), f, g = case_inputs(D, R, H, E, seed)
    fw = ref.forward(x, n, mu, M2, f, g, H, E)
    assert max(ref.ambiguity(fw).values()) <= AMBIGUITY_CAP
    st = storages_of(x, N, T, poison=True, seed=seed)
    cur = module(D, N, H=H, E=E, seed=seed, coeff=0.5, ext_coeff=0.75, update_proportion=0.5)
    assert np.array_equal(host(cur.target), f) and np.array_equal(host(cur.predictor), g)
    carry0 = np.linspace(0.5, 1.5, N)
    cur.state[ref.RND_HEAD + 2 * D:] = torch.from_numpy(carry0).cuda()
    cur.state[ref.RND_CTR] = 999.0
    err = host(cur.begin_section(st))
    state = host(cur.state)
    assert state[ref.RND_N] == n == R
    assert np.allclose(state[ref.RND_HEAD:ref.RND_HEAD + D], mu, rtol=1e-9, atol=1e-12)
    assert np.allclose(state[ref.RND_HEAD + D:ref.RND_HEAD + 2 * D], M2, rtol=1e-9, atol=1e-12)
    ws = saving_forward(cur, R)
    report = {}
    for k in ("xh", "h1", "h2", "diff"):
        report[k] = ref.within(host(ws[k][:R]), fw[k])
    report["err"] = ref.within(err.reshape(-1), fw["err"])
    assert np.array_equal(host(ws["err"][:R]), err.reshape(-1))
    rewards = np.stack([host(s.rewards[:T, 0]) for p in st for s in p])
    stats, carry, sigma, mixed = ref.reward(err, carry0, (0.0, 0.0, 0.0), 0.99, 1e-8, 0.5, 0.75, rewards)
    assert state[ref.RND_RHO_N] == stats[0] and np.isclose(state[ref.RND_RHO_MEAN], stats[1], rtol=1e-9, atol=0)
    assert np.isclose(state[ref.RND_RHO_M2], stats[2], rtol=1e-9, atol=1e-300)
    assert np.isclose(state[ref.RND_SIGMA], sigma, rtol=1e-9, atol=0) and np.allclose(state[ref.RND_HEAD + 2 * D:], carry, rtol=1e-12, atol=0)
    report["mixed"] = ref.within(np.stack([host(s.rewards_mixed[:T, 0]) for p in st for s in p]), mixed)
    m = ref.mask(seed, 999, R, 0.5)
    (grad, e_grad), (dO, e_dO) = ref.backward(fw, g, m, H, E)
    loss = host(cur.backward(R))
    assert loss[1] == m.sum()
    report["dO"] = ref.within(host(ws["scratch"][R + 2:R + 2 + R * E]).reshape(R, E), (dO, e_dO))
    report["grad"] = ref.within(host(cur.grads), (grad, e_grad))
    print("D=%d R=%d E=%d worst |dev - ref| / bound, elements outside: %s" % (D, R, E, report))
    assert all(v[1] == 0 for v in report.values()), report
    assert m.sum() == 0 or np.abs(host(cur.grads)).max() > 0


def test_statistics_of_three_successive_rollouts():
    """Three begin_section calls of one module in training mode on rollouts of 99, 15 and 165 rows (T = 33, 5, 55) around different
    means: after every section the count, mu and M2 equal the reference's chained merge, and at the end numpy's one-pass float64 mean
    and variance of all 279 rows, at rtol 1e-9 (|mean| / std <= 10); the rho statistics, sigma and the carries equal the reference's
    merge chained from the section before (the device's err taken as exact)."""
    D, N = 37, 3
    rng = np.random.RandomState(21)
    X = [(rng.randn(N * t, D) * rng.uniform(0.5, 2.0, D) + rng.uniform(-3.0, 3.0, D) + k).astype(np.float32) for k, t in enumerate((33, 5, 55))]
    allx = np.concatenate(X).astype(np.float64)
    assert (np.abs(allx.mean(0)) / allx.std(0)).max() <= 10.0
    cur = module(D, N, E=32, seed=8)
    n_seen, stats, carry, chained = 0, (0.0, 0.0, 0.0), np.zeros(N), (0.0, np.zeros(D), np.zeros(D))
    for x in X:
        t = x.shape[0] // N
        st = storages_of(x, N, t, poison=True)
        err = host(cur.begin_section(st))
        state = host(cur.state)
        n_seen += N * t
        chained = ref.chan_merge(chained[0], chained[1], chained[2], x)
        mu, M2 = state[ref.RND_HEAD:ref.RND_HEAD + D], state[ref.RND_HEAD + D:ref.RND_HEAD + 2 * D]
        assert state[ref.RND_N] == n_seen == chained[0]
        assert np.allclose(mu, chained[1], rtol=1e-9, atol=0) and np.allclose(M2, chained[2], rtol=1e-9, atol=0)
        rewards = np.stack([host(s.rewards[:t, 0]) for p in st for s in p])
        stats, carry, sigma, mixed = ref.reward(err, carry, stats, 0.99, 1e-8, 0.5, 1.0, rewards)
        assert state[ref.RND_RHO_N] == stats[0] == n_seen
        assert np.isclose(state[ref.RND_RHO_MEAN], stats[1], rtol=1e-9, atol=0) and np.isclose(state[ref.RND_RHO_M2], stats[2], rtol=1e-9, atol=0)
        assert np.isclose(state[ref.RND_SIGMA], sigma, rtol=1e-9, atol=0)
        assert np.allclose(state[ref.RND_HEAD + 2 * D:], carry, rtol=1e-12, atol=0)
        assert ref.within(np.stack([host(s.rewards_mixed[:t, 0]) for p in st for s in p]), mixed)[1] == 0
    assert n_seen == 279 and float(err.min()) > 0
    assert np.allclose(mu, allx.mean(0), rtol=1e-9, atol=0) and np.allclose(M2 / n_seen, allx.var(0), rtol=1e-9, atol=0)


# ----------------------------------------------------------------------------- behaviour
def test_frozen_mode():
    """train(False): begin_section leaves statistics, carries, predictor and step counter bit-identical and still writes rewards_mixed;
    update() takes no step."""
    D, N, T = 37, 3, 5
    rng = np.random.RandomState(8)
    cur = module(D, N, E=32, epochs=1, minibatches=1)
    cur.begin_section(storages_of(rng.randn(N * T, D).astype(np.float32), N, T))
    cur.update()
    cur.train(False)
    s0, p0, k0 = cur.state.clone(), cur.predictor.clone(), cur.step_dev.clone()
    st = storages_of(rng.randn(N * T, D).astype(np.float32) + 1.0, N, T, seed=1)
    for pair in st:
        for s in pair:
            cur.mixed_of(s).fill_(SENT)
    err = cur.begin_section(st)
    assert cur.update() == 0
    assert torch.equal(cur.state, s0) and torch.equal(cur.predictor, p0) and torch.equal(cur.step_dev, k0)
    flat = [s for pair in st for s in pair]
    want = ref.mixed(host(err), float(s0[ref.RND_SIGMA]), 0.5, 1.0, np.stack([host(s.rewards[:T, 0]) for s in flat]))
    assert ref.within(np.stack([host(s.rewards_mixed[:T, 0]) for s in flat]), want)[1] == 0
    assert all(float(s.rewards_mixed[T]) == SENT for s in flat)


def test_distillation_works():
    """200 full-batch predictor steps at lr 1e-3 on 96 fixed rows: their mean err falls below its start and below the mean err of 96 rows
    drawn around another mean.  The float64 reference run shows both first."""
    D, H, E, R = 37, 128, 32, 96
    x, (n, mu, M2), f, g = case_inputs(D, R, H, E, 12)
    x2 = (np.random.RandomState(13).randn(R, D) + 1.5).astype(np.float32)
    e0 = ref.forward(x, n, mu, M2, f, g, H, E)["err"][0].mean()
    g64 = ref.adam_run(x, n, mu, M2, f, g, H, E, 200, 1e-3)
    e1 = ref.forward(x, n, mu, M2, f, g64, H, E)["err"][0].mean()
    e2 = ref.forward(x2, n, mu, M2, f, g64, H, E)["err"][0].mean()
    print("float64: start %.4e, after %.4e, other batch %.4e" % (e0, e1, e2))
    assert e1 < e0 and e1 < e2
    cur = module(D, 3, H=H, E=E, seed=12, update_proportion=1.0, epochs=200, minibatches=1, lr=1e-3)
    st = storages_of(x, 3, 32)
    d0 = float(cur.begin_section(st).mean())
    assert cur.update() == 200
    cur.train(False)
    d1 = float(cur.begin_section(st).mean())
    d2 = float(cur.begin_section(storages_of(x2, 3, 32)).mean())
    print("device:  start %.4e, after %.4e, other batch %.4e" % (d0, d1, d2))
    assert d1 < d0 and d1 < d2
    fw0 = ref.forward(x, n, mu, M2, f, g, H, E)
    assert abs(d0 - e0) <= fw0["err"][1].mean() + ref.U * e0                 # (the mean of the per-row bounds, one rounding of the mean)


def test_state_dict_round_trip():
    """state_dict() -> a fresh module -> load_state_dict(): the next begin_section writes the same rewards_mixed bits."""
    D, N, T = 37, 3, 5
    rng = np.random.RandomState(10)
    xa, xb = rng.randn(N * T, D).astype(np.float32), rng.randn(N * T, D).astype(np.float32)
    a = module(D, N, E=32, seed=4, epochs=1, minibatches=2)
    a.begin_section(storages_of(xa, N, T))
    a.update()
    sd = {k: v.cpu() for k, v in a.state_dict().items()}
    b = module(D, N, E=32, seed=99, epochs=1, minibatches=2)
    b.load_state_dict(sd)
    sa, sb = storages_of(xb, N, T), storages_of(xb, N, T)
    ea, eb = a.begin_section(sa), b.begin_section(sb)
    assert torch.equal(ea, eb) and torch.equal(a.state, b.state)
    for pa, pb in zip(sa, sb):
        for u, v in zip(pa, pb):
            assert torch.equal(u.rewards_mixed, v.rewards_mixed)
    a.update()
    b.update()
    assert torch.equal(a.predictor, b.predictor) and int(a.step_dev) == int(b.step_dev) == 4
    with pytest.raises(ValueError, match="does not fit"):
        module(D, N, E=64).load_state_dict(sd)


# ----------------------------------------------------------------------------- the learner section and the training loops
def run_sections(tmp, coeff, sections=2):
    """coeff None: no module; else a Curiosity with that coefficient.  Per section (losses, parameters, generator state, stats)."""
    from ppo_agent.train import learner_section_multi
    from tests.test_smooth_gpu import N_ENV, e2e_cfg, make, section_rollouts
    agent, shared = make(tmp)
    cur = None if coeff is None else module(agent.arena.D, N_ENV, coeff=coeff, epochs=1, minibatches=2)
    torch.manual_seed(77)
    out = []
    for e in range(sections):
        rollouts, dones = section_rollouts(e), [False, e == 1]
        st = {}
        losses = learner_section_multi(agent, rollouts, dones, e2e_cfg(), shared, stats=st, episode=e,
                                       **({} if cur is None else dict(curiosity=cur)))
        out.append((losses, agent.arena.params.clone(), torch.get_rng_state().clone(), st))
    torch.cuda.synchronize()
    return agent, cur, out


def test_zero_coefficient_leaves_the_run_without_the_key(tmp_path):
    """coeff = 0 with the module present: losses, parameters and the global generator after both sections equal the run without it; with
    coeff > 0 the parameters move and stay finite, and the section's stats carry the module's entry."""
    _a, cur, zero = run_sections(tmp_path / "a", 0.0)
    _b, _n, plain = run_sections(tmp_path / "b", None)
    for e in range(2):
        assert torch.equal(zero[e][2], plain[e][2]) and zero[e][0] == plain[e][0], e
        assert torch.equal(zero[e][1], plain[e][1]), e
        assert "curiosity" in zero[e][3] and "curiosity" not in plain[e][3]
    assert int(cur.step_dev) == 4 and float(cur.errors().min()) > 0
    _c, _cur, on = run_sections(tmp_path / "c", 0.5, sections=1)
    s = on[0][3]["curiosity"]
    print("section stats with the bonus: %s" % (s,))
    assert not torch.equal(on[0][1], plain[0][1]) and bool(torch.isfinite(on[0][1]).all())
    assert s["steps"] == 2 and s["mean_e"] > 0 and s["max_e"] >= s["mean_e"] and s["sigma"] > 0 and s["mean_abs_bonus"] > 0
    assert s["loss_after"] is not None and s["loss_before"] == s["mean_e"]
    from ppo_agent.train import stats_line
    assert "curiosity: e " in stats_line(0, on[0][3])
    from ppo_agent.train import learner_section_multi
    from tests.test_smooth_gpu import e2e_cfg, make, section_rollouts
    from ppo_agent.storage import ReturnScaler
    agent, shared = make(tmp_path / "d")
    with pytest.raises(ValueError, match="reward_scaling"):
        learner_section_multi(agent, section_rollouts(0), [False, False], e2e_cfg(), shared, curiosity=_cur,
                              reward_scaler=ReturnScaler(2, 0.99, device="cuda"))


def test_train_vec_and_train_with_the_key(tmp_path, hip):
    """Two episodes of train_vec with one and two environments and of train(): the key absent and the key None are today's run; with the
    key the run finishes, the log lines carry `curiosity:`, the block holds the last episode's beta, the learner captures no further graph
    between episodes, the parameters are finite and differ from the plain run; each refused combination names its key."""
    from cadre_amd.ppo_agent import train as T_
    from ppo_agent import train as train_mod
    from tests.helpers import SyntheticEnv, topology_cfgs
    graphs = []

    def run(tag, n_env=1, **extra):
        lines = []
        train_cfg, agent_cfg, env_cfg, rollout_cfg = topology_cfgs(str(tmp_path / tag), T=8, episodes=2)
        if n_env > 1:
            env_cfg.update(num_processes=n_env, port=[2000 + i for i in range(n_env)], routes=["r%d" % i for i in range(n_env)],
                           scenarios=["s"] * n_env, town=["Town01"] * n_env)
        train_cfg.update(save_interval=10 ** 6, **extra)
        os.makedirs(str(tmp_path / tag), exist_ok=True)
        del graphs[:]
        cb = lambda event, **st: graphs.append(len(st["agent"].learner._graphs)) if event == "update" else None
        agent = train_mod.train_vec(0, train_cfg, agent_cfg, env_cfg, rollout_cfg, n_env, env_cls=SyntheticEnv,
                                    logger=types.SimpleNamespace(log=lines.append), callback=cb)
        torch.cuda.synchronize()
        return agent, lines, list(graphs)
    key = dict(curiosity=dict(coeff=("linear", 1.0, 0.0), epochs=1, minibatches=2))
    for n_env in (1, 2):
        absent, _l, g_plain = run("a%d" % n_env, n_env, log_stats=True)
        none, plain_lines, _g = run("b%d" % n_env, n_env, log_stats=True, curiosity=None)
        assert torch.equal(absent.arena.params, none.arena.params) and getattr(none, "curiosity", None) is None
        agent, lines, g_on = run("c%d" % n_env, n_env, log_stats=True, **key)
        stat_lines = [s for s in lines if "approx kl" in s]
        print(stat_lines[-1])
        assert len(stat_lines) == 2 and all("curiosity: e " in s and "sigma" in s for s in stat_lines)
        assert not any("curiosity:" in s for s in plain_lines)
        cur = agent.curiosity
        assert float(cur.state[hip.RND_BETA]) == 0.5 and float(cur.state[hip.RND_N]) == 2 * 8 * n_env and int(cur.step_dev) == 4
        assert len(g_on) == 2 and g_on[0] == g_on[1] and g_on == g_plain     # no graph is captured between the episodes
        assert agent.arena.step == absent.arena.step and bool(torch.isfinite(agent.arena.params).all())
        assert not torch.equal(agent.arena.params, absent.arena.params)
    for extra, why in ((dict(sample_reuse=dict(rollouts=2)), "sample_reuse"), (dict(self_imitation=dict(rollouts=2, coeff=0.1)), "self_imitation"),
                       (dict(reward_scaling=True), "reward_scaling"), (dict(checkpoint_interval=1), "checkpoint_interval"),
                       (dict(resume_from=str(tmp_path / "none.pt")), "resume_from"), (dict(curiosity=dict(coeff=0.1, bonus=1)), "unknown")):
        with pytest.raises(ValueError, match=why):
            run("d", **dict(key, **extra))
    # train(): one environment
    made = []
    Base = T_.CadreAgent

    class Agent(Base):
        def __init__(self, *a, **kw):
            Base.__init__(self, *a, **kw)
            made.append(self)

    def run_one(tag, **extra):
        lines = []
        train_cfg, agent_cfg, env_cfg, rollout_cfg = topology_cfgs(str(tmp_path / tag), T=8, episodes=2)
        train_cfg.update(save_interval=10 ** 6, log_stats=True, **extra)
        os.makedirs(str(tmp_path / tag), exist_ok=True)
        orig, T_.CadreAgent = T_.CadreAgent, Agent
        try:
            T_.train(0, train_cfg, agent_cfg, env_cfg, rollout_cfg, env_cls=SyntheticEnv, logger=types.SimpleNamespace(log=lines.append))
        finally:
            T_.CadreAgent = orig
        torch.cuda.synchronize()
        return made[-1], [s for s in lines if "approx kl" in s]
    absent1, plain1 = run_one("one_a")
    none1, _l1 = run_one("one_b", curiosity=None)
    assert torch.equal(absent1.arena.params, none1.arena.params) and none1.curiosity is None and not any("curiosity:" in s for s in plain1)
    with1, one = run_one("one_c", curiosity=dict(coeff=0.25, epochs=1, minibatches=1))
    assert len(one) == 2 and all("curiosity: e " in s for s in one)
    assert float(with1.curiosity.state[hip.RND_BETA]) == 0.25 and int(with1.curiosity.step_dev) == 2
    assert bool(torch.isfinite(with1.arena.params).all()) and not torch.equal(with1.arena.params, absent1.arena.params)
    assert with1.arena.step == absent1.arena.step
