"""Cost constraints on the device (cadre_amd/constraint.py, csrc/constraint.hip): float64 parity of every stored element of the cost
critic within the a-priori first-order bound of tests/constraint_ref.py, the mix and the multiplier bit for bit / at rtol 1e-12, the
exact properties (lambda = 0 is the run without the module, batch invariance, bounds of what is touched, the step is the existing
optimiser), behaviour and the training loops with the key.

Shapes: D = 530 (production: 530 = 4 * 128 + 18, a k tail in the last chunk) and 37 (less than one chunk); (N, T) = (3, 33): 102 and 99
rows, partial last workgroups; (1, 5), (1, 2), (3, 2): fewer rows than one tile; hidden 128 and 32; T = 300 for the mix (more rows than
the workgroup has threads)."""
import os
import types

import numpy as np
import pytest
import torch

from tests import constraint_ref as ref
from tests.test_constraint_cpu import AMBIGUITY_CAP, PARITY_CASES
from tests.test_rollout_finish_gpu import np_scan

pytestmark = pytest.mark.gpu
SENT = -7.5
S_LEN = 3


@pytest.fixture(scope="module")
def hip():
    from cadre_amd import hip as h
    h.lib()
    return h


def host(t):
    return t.detach().cpu().numpy()


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def storages_of(x, N, T, poison=False, seed=0, flags=False):
    """N (steer, throttle) pairs; the newest frame row of row t <= T of storage w of head h is x[h][w (T + 1) + t].  poison: NaN in
    the pad columns and in every older frame of every window.  Costs >= 0 with zeros among them, masks with ends, and with `flags` a
    time-limit cut in every storage."""
    from ppo_agent.storage import RolloutStorage
    D = x[0].shape[1]
    g = torch.Generator()
    g.manual_seed(1000 + seed)
    out = []
    for w in range(N):
        pair = []
        for h in range(2):
            s = RolloutStorage(T, 1, D, S_LEN, 32, True, 0.99, 0.95, device="cuda")
            s._obs.copy_(torch.randn(s._obs.shape, generator=g))
            if poison:
                s._obs.fill_(float("nan"))
            s.obs[:, S_LEN - 1].copy_(torch.from_numpy(x[h][w * (T + 1):(w + 1) * (T + 1)]))
            s.rewards.copy_(torch.randn(T + 1, 1, generator=g))
            s.value_preds.copy_(torch.randn(T + 1, 1, generator=g))
            s.masks.copy_((torch.rand(T + 1, 1, generator=g) >= 0.2).float())
            c = torch.rand(T + 1, generator=g)
            s.costs = torch.where(c < 0.5, torch.zeros(()), c).cuda()
            if flags:
                s.time_limits[T // 2] = 1.0
                s._tl_used = True
            s.step = T
            pair.append(s)
        out.append(tuple(pair))
    return out


def module(D, N, H=128, seed=3, budget=0.1, **kw):
    from cadre_amd.constraint import CostConstraint
    return CostConstraint(D, N, budget=budget, hidden=H, seed=seed, device="cuda", **kw)


def rows_of(fw, idx):
    """The reference's forward restricted to the rows idx."""
    out = {k: fw[k][idx] for k in ("x", "amb1", "amb2", "pre1", "pre2")}
    out.update({k: (fw[k][0][idx], fw[k][1][idx]) for k in ("h1", "h2", "v")})
    return out


def step_rows(N, T):
    """Rows t < T of every storage, as indices into the (storage, row 0 .. T) order of the inputs."""
    return np.array([w * (T + 1) + t for w in range(N) for t in range(T)])


def saving_forward(con, h, lo, rows):
    ws = con._workspace(rows)
    con._forward(h, con._section[2], lo, rows, ws["values"][h], ws)
    return ws


# ----------------------------------------------------------------------------- float64 parity, every stored element
@pytest.mark.parametrize("D,N,T,H,seed", PARITY_CASES)
def test_parity_of_every_stored_element(D, N, T, H, seed):
    """cost_values, h1, h2, the loss and every gradient element within the reference's a-priori bound; cost_returns and cost_adv equal the
    strict-order float32 scan on the device's own cost_values, bit for bit.  The ambiguity cap is asserted from the reference before the
    device is looked at.  The storages hold NaN wherever nothing may be read."""
    x, towers = ref.case_inputs(D, N, T, H, seed)
    fws = [ref.forward(x[h], towers[h], H) for h in (0, 1)]
    assert max(max(ref.ambiguity(fw).values()) for fw in fws) <= AMBIGUITY_CAP
    st = storages_of(x, N, T, poison=True, seed=seed, flags=seed % 2 == 1)
    con = module(D, N, H=H, seed=seed, epochs=1, minibatches=1)
    assert np.array_equal(host(con.params), np.concatenate(towers))
    dones = [False, True, False][:N]
    con.begin_section(st, dones)
    cv, cr, ca = host(con.cost_values), host(con.cost_returns), host(con.cost_adv)
    report = {}
    R, idx = N * T, step_rows(N, T)
    for h in (0, 1):
        v, ev = fws[h]["v"]
        report["cost_values%d" % h] = ref.within(cv[h][:, :T], (v[idx].reshape(N, T), ev[idx].reshape(N, T)))
        keep = np.array([0.0 if d else 1.0 for d in dones])
        last = np.array([w * (T + 1) + T for w in range(N)])
        report["bootstrap%d" % h] = ref.within(cv[h][:, T], (v[last] * keep, ev[last] * keep))
        assert all(cv[h][w, T] == 0.0 for w in range(N) if dones[w])
        for w in range(N):
            s = st[w][h]
            keep_t = 1.0 - host(s.time_limits)[:, 0] if s._tl_used else None
            ret, adv, _V = np_scan(host(s.costs), cv[h][w], host(s.masks)[:, 0], cv[h][w, T], keep=keep_t)
            assert np.array_equal(cr[h][w, :T], ret) and np.array_equal(ca[h][w], adv) and cr[h][w, T] == 0.0, (h, w)
        ws = saving_forward(con, h, 0, R)
        sub = rows_of(fws[h], idx)
        for k, name in (("values", "v"), ("h1", "h1"), ("h2", "h2")):
            report["%s%d" % (k, h)] = ref.within(host(ws[k][h][:R]), sub[name])
        assert np.array_equal(host(ws["values"][h][:R]).reshape(N, T), cv[h][:, :T])       # (the same rows in both launches: the same bits)
        ret = cr[h][:, :T].reshape(-1)
        (grad, e_grad), (loss, e_loss), dv = ref.backward(sub, towers[h], ret, H)
        got = host(con.backward(h, 0, R))
        assert got[1] == R
        report["loss%d" % h] = ref.within(got[:1], (np.array([loss]), np.array([e_loss])))
        report["dv%d" % h] = ref.within(host(ws["scratch"][h][:R]), dv)
        report["grad%d" % h] = ref.within(host(con.grads[h * con.P:(h + 1) * con.P]), (grad, e_grad))
        assert np.abs(host(con.grads[h * con.P:(h + 1) * con.P])).max() > 0
    print("D=%d N=%d T=%d H=%d worst |dev - ref| / bound, elements outside: %s" % (D, N, T, H, report))
    assert all(v[1] == 0 for v in report.values()), report


# ----------------------------------------------------------------------------- the mix and the multiplier
@pytest.mark.parametrize("T,lam", [(33, (0.0, 0.75)), (300, (2.5, 1e-3)), (2, (1e-60, 100.0))])
def test_mix_bit_for_bit(T, lam):
    """cadre_lag_mix against numpy float32 statement by statement with a sequential float64 sum for m: any bit difference fails.  A head
    whose (float)lambda is 0 keeps every bit of its advantages, a -0 included."""
    D, N = 37, 3
    x, _t = ref.case_inputs(D, N, T, 32, 7)
    st = storages_of(x, N, T)
    con = module(D, N, H=32, lr_lambda=0.0)
    con.begin_section(st, None)
    g = torch.Generator()
    g.manual_seed(T)
    con.cost_adv.copy_(torch.randn(2, N, T, generator=g) * 3.0 + 0.5)
    con.cost_adv[0, 0, 0] = -0.0
    flat = [s for p in st for s in p]
    for s in flat:
        s.advantages.copy_(torch.randn(T, 1, generator=g))
        s.advantages[0] = -0.0
    before = [host(s.advantages)[:, 0].copy() for s in flat]
    con.set_lambda(lam)
    con.mix(st)
    ca = host(con.cost_adv)
    diag = host(con._diag)
    for k, s in enumerate(flat):
        w, h = k >> 1, k & 1
        want, m = ref.mix(before[k], ca[h, w], lam[h])
        assert np.array_equal(host(s.advantages)[:, 0].view(np.int32), want.view(np.int32)), (k, T)
        if np.float32(lam[h]) == 0:
            assert np.signbit(host(s.advantages)[0, 0])
        lf = np.float64(np.float32(lam[h]))
        p = np.abs((np.float32(lam[h]) * (ca[h, w] - m).astype(np.float32)).astype(np.float32)).astype(np.float64)
        den = np.float64(np.float32(np.float32(1.0) + np.float32(lam[h])))
        assert np.isclose(diag[k, 0], (p / den).mean(), rtol=1e-12, atol=0) and lf >= 0
        assert np.isclose(diag[k, 1], (np.abs(before[k].astype(np.float64)) / den).mean(), rtol=1e-12, atol=0)


@pytest.mark.parametrize("budget,end", [((5.0, 5.0), "floor"), ((0.0, 0.0), "ceiling")])
def test_lambda_three_sections(budget, end, hip):
    """J, the share of costly rows and lambda of both heads over three successive sections against the float64 rule at rtol 1e-12, ending
    at the floor (budget above every cost rate) and at the ceiling (budget 0)."""
    D, N, T = 37, 3, 33
    con = module(D, N, H=32, budget=budget, lambda_init=(0.4, 0.6), lr_lambda=(2.0, 3.0), lambda_max=1.5)
    lam = [0.4, 0.6]
    for sec in range(3):
        x, _t = ref.case_inputs(D, N, T, 32, 20 + sec)
        st = storages_of(x, N, T, seed=sec)
        con.begin_section(st, None)
        state = host(con.state).reshape(2, hip.LAG_STRIDE)
        for h in (0, 1):
            costs = np.stack([host(p[h].costs)[:T] for p in st])
            J, share, lam[h] = ref.lambda_step(costs, lam[h], budget[h], (2.0, 3.0)[h], 1.5)
            assert np.isclose(state[h, hip.LAG_J], J, rtol=1e-12, atol=0) and np.isclose(state[h, hip.LAG_SHARE], share, rtol=1e-12, atol=0)
            assert np.isclose(state[h, hip.LAG_LAMBDA], lam[h], rtol=1e-12, atol=0) and state[h, hip.LAG_UPDATES] == sec + 1
            assert 0 < share < 1 and J > 0
    assert lam == ([0.0, 0.0] if end == "floor" else [1.5, 1.5]) and host(con.lambdas()).tolist() == lam


# ----------------------------------------------------------------------------- exact properties
def run_sections(tmp, keys, sections=2):
    """keys None: no module; else a CostConstraint with those keys.  Per section (losses, parameters, moments, advantages, generator
    state, stats)."""
    from ppo_agent.train import learner_section_multi
    from tests.test_smooth_gpu import N_ENV, e2e_cfg, make, section_rollouts
    agent, shared = make(tmp)
    con = None if keys is None else module(agent.arena.D, N_ENV, epochs=1, minibatches=2, **keys)
    torch.manual_seed(77)
    out = []
    for e in range(sections):
        rollouts, dones = section_rollouts(e), [False, e == 1]
        g = torch.Generator()
        g.manual_seed(e)
        for pair in rollouts:
            for s in pair:
                c = torch.rand(s.num_steps + 1, generator=g)
                s.costs = torch.where(c < 0.5, torch.zeros(()), c).cuda()
        st = {}
        losses = learner_section_multi(agent, rollouts, dones, e2e_cfg(), shared, stats=st, episode=e,
                                       **({} if con is None else dict(constraint=con)))
        out.append((losses, agent.arena.params.clone(), agent.arena.exp_avg.clone(), agent.arena.exp_avg_sq.clone(),
                    [s.advantages.clone() for p in rollouts for s in p], torch.get_rng_state().clone(), st))
    torch.cuda.synchronize()
    return agent, con, out


def test_lambda_zero_is_the_run_without_the_key(tmp_path):
    """lambda_init = 0, lr_lambda = 0 with the module present: the advantages, the whole arena, the Adam moments, the three loss values and
    the global generator after both sections equal the run without it, bit for bit; with lambda > 0 the advantages and the parameters
    move and stay finite, and the section's stats carry the module's entry."""
    _a, con, zero = run_sections(tmp_path / "a", dict(lambda_init=0.0, lr_lambda=0.0))
    _b, _n, plain = run_sections(tmp_path / "b", None)
    for e in range(2):
        assert zero[e][0] == plain[e][0], e
        for i in (1, 2, 3, 5):
            assert torch.equal(bits(zero[e][i]), bits(plain[e][i])) if i != 5 else torch.equal(zero[e][i], plain[e][i]), (e, i)
        assert all(torch.equal(bits(u), bits(v)) for u, v in zip(zero[e][4], plain[e][4])), e
        assert "constraint" in zero[e][6] and "constraint" not in plain[e][6]
    s = zero[1][6]["constraint"]
    assert int(con.step_dev) == 4 and s["lambda"] == (0.0, 0.0) and s["J"][0] > 0 and s["mean_abs_cost_term"] == (0.0, 0.0)
    _c, _con, on = run_sections(tmp_path / "c", dict(lambda_init=(0.5, 2.0), lr_lambda=0.0), sections=1)
    s = on[0][6]["constraint"]
    print("section stats with the constraint: %s" % (s,))
    assert not torch.equal(on[0][1], plain[0][1]) and bool(torch.isfinite(on[0][1]).all())
    assert all(not torch.equal(u, v) and bool(torch.isfinite(u).all()) for u, v in zip(on[0][4], plain[0][4]))
    assert s["steps"] == 2 and s["lambda"] == (0.5, 2.0) and min(s["mean_abs_cost_term"]) > 0 and min(s["mean_abs_reward_term"]) > 0
    assert s["loss_after"] is not None and min(s["loss_before"]) > 0 and 0 < s["costly_share"][0] < 1 and s["lambda_updates"] == (1, 1)
    from ppo_agent.train import learner_section_multi, stats_line
    assert "constraint: J " in stats_line(0, on[0][6])
    from tests.test_smooth_gpu import e2e_cfg, make, section_rollouts
    agent, shared = make(tmp_path / "d")
    with pytest.raises(ValueError, match="smooth"):
        learner_section_multi(agent, section_rollouts(0), [False, False], e2e_cfg(), shared, constraint=_con, smooth=object())


def test_batch_invariance():
    """Rows computed alone, in chunks of 32 + 1 and all at once: equal bits of the value and of both saved activations."""
    D, N, T, H = 530, 3, 33, 128
    x, _t = ref.case_inputs(D, N, T, H, 9)
    st = storages_of(x, N, T)
    con = module(D, N, H=H)
    con.begin_section(st, None)
    R = N * T
    for h in (0, 1):
        ws = saving_forward(con, h, 0, R)
        full = [ws[k][h][:R].clone() for k in ("values", "h1", "h2")]
        assert float(full[0].abs().max()) > 0
        for lo in range(0, R, 33):
            n = min(33, R - lo)
            ws = saving_forward(con, h, lo, n)
            for a, k in zip(full, ("values", "h1", "h2")):
                assert torch.equal(bits(ws[k][h][:n]), bits(a[lo:lo + n])), (h, lo, k)
        for r in (0, 31, 32, 70, R - 1):
            ws = saving_forward(con, h, r, 1)
            for a, k in zip(full, ("values", "h1", "h2")):
                assert torch.equal(bits(ws[k][h][:1]), bits(a[r:r + 1])), (h, r, k)


def test_bounds_of_what_is_touched(hip):
    """NaN in the pad columns and in the older frames of every window, sentinels behind every output of the section's chain, of the mix
    and of a critic step, in the reserved fields of the state block and behind `advantages`: every output is finite, no sentinel moves,
    the settings of the block, the costs and the rewards keep their bits, and a cursor outside 0 .. T writes nothing."""
    D, N, T, H = 530, 3, 33, 128
    R = N * T
    x, _t = ref.case_inputs(D, N, T, H, 4)
    st = storages_of(x, N, T, poison=True)
    flat = [s for p in st for s in p]
    con = module(D, N, H=H, lambda_init=(0.5, 0.25), lr_lambda=(0.5, 0.0))
    pad = 64
    big = {}

    def guarded(name, shape, dtype=torch.float32):
        n = int(np.prod(shape))
        big[name] = (torch.full((n + 2 * pad,), SENT, dtype=dtype, device="cuda"), n)
        return big[name][0][pad:pad + n].view(shape)
    con.cost_values, con.cost_returns = guarded("values", (2, N, T + 1)), guarded("returns", (2, N, T + 1))
    con.cost_adv, con.cost_next = guarded("adv", (2, N, T)), guarded("next", (2, N))
    con._diag = guarded("diag", (2 * N, 2), torch.float64)
    con.grads = guarded("grads", (2 * con.P,))
    for k, s in enumerate(flat):
        s.advantages = guarded("adv_r%d" % k, (T, 1))
    con.state[hip.LAG_UPDATES + 1::hip.LAG_STRIDE] = SENT
    s0 = con.state.clone()
    raw = [(s.rewards.clone(), s.costs.clone()) for s in flat]
    con.begin_section(st, [False, True, False])
    from ppo_agent.storage import RolloutStorage
    RolloutStorage.finish_rollouts(flat, [torch.tensor([0.1 * k], device="cuda") for k in range(2 * N)])
    con.mix(st)
    ws = con._workspace(R)
    for k in ("values", "h1", "h2", "scratch"):
        ws[k] = guarded("ws_" + k, tuple(ws[k].shape))
    for h in (0, 1):
        saving_forward(con, h, 0, R)
        con.backward(h, 0, R)
    torch.cuda.synchronize()
    for name, (t, n) in big.items():
        assert bool((t[:pad] == SENT).all()) and bool((t[pad + n:] == SENT).all()), name
        body = t[pad:pad + n]
        if name == "returns":                                  # (row T of cost_returns is not written, as row T of returns is not)
            body = body.view(2, N, T + 1)[:, :, :T]
        assert bool(torch.isfinite(body).all()) and bool((body != SENT).all()), name
    state = con.state
    for f in (hip.LAG_BUDGET, hip.LAG_LR, hip.LAG_MAX, hip.LAG_UPDATES + 1):
        assert torch.equal(state[f::hip.LAG_STRIDE], s0[f::hip.LAG_STRIDE]), f
    assert float(state[hip.LAG_STRIDE + hip.LAG_LAMBDA]) == 0.25 and float(state[hip.LAG_LAMBDA]) != 0.5        # lr_lambda 0 / 0.5
    for s, (r0, c0) in zip(flat, raw):
        assert torch.equal(s.rewards, r0) and torch.equal(s.costs, c0)
    # cadre_cost_note: the slot of every storage, nothing else; a cursor outside 0 .. T and a null pointer are skipped
    tab = torch.tensor([hip.ptr(s.costs) for s in flat[:3]] + [0], dtype=torch.int64).cuda()
    slots = torch.tensor([0, T, T + 1, 2], dtype=torch.int32).cuda()
    vals = torch.tensor([9.0, 8.0, 7.0, 6.0], dtype=torch.float32).cuda()
    hip.check(hip.lib().cadre_cost_note(hip.ptr(tab), hip.ptr(slots), hip.ptr(vals), 4, T, hip.stream()), "cadre_cost_note")
    want = [c0.clone() for _r, c0 in raw]
    want[0][0], want[1][T] = 9.0, 8.0
    assert all(torch.equal(s.costs, w) for s, w in zip(flat, want))


def test_the_step_is_the_existing_optimiser(hip):
    """update() with one step leaves the towers that the two cadre_cost_backward calls followed by a direct cadre_clip_adam_graph call with
    two segments leave, bit for bit."""
    D, N, T = 37, 1, 5
    x, _t = ref.case_inputs(D, N, T, 32, 7)
    st = storages_of(x, N, T)
    con = module(D, N, H=32, epochs=1, minibatches=1, lr=1e-3, max_norm=0.5)
    con.begin_section(st, None)
    p0 = con.params.clone()
    assert con.update() == 1 and int(con.step_dev) == 1
    p1 = con.params.clone()
    assert not torch.equal(p0[:con.P], p1[:con.P]) and not torch.equal(p0[con.P:], p1[con.P:])
    con.params.copy_(p0)
    for h in (0, 1):
        saving_forward(con, h, 0, N * T)
        con.backward(h, 0, N * T)
    p, m, v = p0.clone(), torch.zeros_like(p0), torch.zeros_like(p0)
    step, norms = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(4, dtype=torch.float64, device="cuda")
    seg = torch.tensor([0, con.P, 2 * con.P], dtype=torch.int64).cuda()
    hip.check(hip.lib().cadre_clip_adam_graph(hip.ptr(p), hip.ptr(con.grads), hip.ptr(m), hip.ptr(v), hip.ptr(seg), 2, hip.ptr(norms), 0.5, 1e-3,
                                              0.9, 0.999, 1e-8, hip.ptr(step), hip.stream()), "cadre_clip_adam_graph")
    assert torch.equal(p, p1) and torch.equal(m, con.exp_avg) and torch.equal(v, con.exp_avg_sq)


# ----------------------------------------------------------------------------- behaviour
def test_the_critic_learns():
    """200 full-batch critic steps at lr 1e-3 on 96 fixed rows whose cost is a fixed function of x (gamma = 0: the cost return of a row is
    its cost): the loss falls below its start and below the loss against another cost function.  The float64 reference run shows both
    first.  No threshold is set."""
    D, H, N, T = 37, 128, 3, 32
    x, towers = ref.case_inputs(D, N, T, H, 12)
    rng = np.random.RandomState(13)
    a, b = rng.randn(2, D) / np.sqrt(D), rng.randn(2, D) / np.sqrt(D)
    idx = step_rows(N, T)
    for h in (0, 1):
        c1, c2 = np.abs(x[h][idx] @ a[h]).astype(np.float32), np.abs(x[h][idx] @ b[h]).astype(np.float32)
        e0 = ref.loss(x[h][idx], towers[h], c1, H)
        p64 = ref.adam_run(x[h][idx], towers[h], c1, H, 200, 1e-3)
        e1, e2 = ref.loss(x[h][idx], p64, c1, H), ref.loss(x[h][idx], p64, c2, H)
        print("float64 head %d: start %.4e, after %.4e, other cost %.4e" % (h, e0, e1, e2))
        assert e1 < e0 and e1 < e2
    con = module(D, N, H=H, seed=12, epochs=200, minibatches=1, lr=1e-3, gamma=0.0, tau=0.0)
    st = storages_of(x, N, T)
    other = []
    for w, pair in enumerate(st):
        for h, s in enumerate(pair):
            xs = x[h][w * (T + 1):(w + 1) * (T + 1)]
            s.costs = torch.from_numpy(np.abs(xs @ a[h]).astype(np.float32)).cuda()
            s.masks.fill_(1.0)
            other.append(np.abs(xs[:T] @ b[h]).astype(np.float32))
    con.begin_section(st, None)
    assert con.update(stats=True) == 200
    s = con.summary()
    after = host(con._after)[:, :, :T].astype(np.float64)
    for h in (0, 1):
        d0, d1 = s["loss_before"][h], s["loss_after"][h]
        d2 = 0.5 * ((after[h] - np.stack(other[h::2])) ** 2).mean()
        print("device head %d:  start %.4e, after %.4e, other cost %.4e" % (h, d0, d1, d2))
        assert d1 < d0 and d1 < d2


def test_frozen_mode_and_state_dict_round_trip():
    """train(False): begin_section writes J and the share, not lambda or the step count; update() takes no step.  state_dict() -> a fresh
    module -> load_state_dict(): the next section and its steps give the same bits."""
    D, N, T = 37, 3, 5
    xa, _t = ref.case_inputs(D, N, T, 32, 10)
    xb, _t = ref.case_inputs(D, N, T, 32, 11)
    a = module(D, N, H=32, seed=4, epochs=1, minibatches=2, lambda_init=0.3, lr_lambda=1.0)
    a.begin_section(storages_of(xa, N, T), None)
    a.update()
    sd = {k: v.cpu() for k, v in a.state_dict().items()}
    b = module(D, N, H=32, seed=99, epochs=1, minibatches=2, lambda_init=0.3, lr_lambda=1.0)
    b.load_state_dict(sd)
    sa, sb = storages_of(xb, N, T, seed=1), storages_of(xb, N, T, seed=1)
    a.begin_section(sa, [True, False, False])
    b.begin_section(sb, [True, False, False])
    assert torch.equal(a.state, b.state) and torch.equal(a.cost_adv, b.cost_adv) and torch.equal(a.cost_returns, b.cost_returns)
    a.update()
    b.update()
    assert torch.equal(a.params, b.params) and int(a.step_dev) == int(b.step_dev) == 4
    with pytest.raises(ValueError, match="does not fit"):
        module(D, N, H=64).load_state_dict(sd)
    a.train(False)
    s0, p0, k0 = a.state.clone(), a.params.clone(), a.step_dev.clone()
    a.begin_section(storages_of(xa, N, T, seed=2), None)
    assert a.update() == 0 and torch.equal(a.params, p0) and torch.equal(a.step_dev, k0)
    from cadre_amd import hip as H_
    st = a.state.view(2, H_.LAG_STRIDE)
    for f in (H_.LAG_LAMBDA, H_.LAG_BUDGET, H_.LAG_LR, H_.LAG_MAX, H_.LAG_UPDATES):
        assert torch.equal(st[:, f], s0.view(2, H_.LAG_STRIDE)[:, f]), f
    assert not torch.equal(st[:, H_.LAG_J], s0.view(2, H_.LAG_STRIDE)[:, H_.LAG_J])


def test_insert_batch_costs_and_insert_cost(hip):
    """insert_batch(costs=) writes the 2N costs of the step at the cursors in one more launch (a number to both heads, a pair per head);
    without the argument and without the tensor no launch is added; insert(cost=) writes the same slot."""
    from ppo_agent.storage import RolloutStorage
    N, T, D = 2, 4, 37
    mk = lambda: [tuple(RolloutStorage(T, 1, D, S_LEN, 32, True, 0.99, 0.95, device="cuda") for _h in (0, 1)) for _w in range(N)]
    outs = [(torch.randn(S_LEN, D).cuda(), (torch.tensor(1), torch.tensor(2)), (torch.tensor(-0.5), torch.tensor(-0.25)),
             (torch.tensor(0.1), torch.tensor(0.2))) for _w in range(N)]
    args = (outs, [[1.0, 2.0]] * N, [[1.0, 1.0]] * N, [0] * N)
    st = mk()
    n0 = hip.N_CALLS
    RolloutStorage.insert_batch(st, *args)
    assert hip.N_CALLS == n0 + 1 and all(getattr(s, "costs", None) is None for p in st for s in p)
    RolloutStorage.insert_batch(st, *args, costs=[0.5, (0.25, 0.0)])
    assert hip.N_CALLS == n0 + 3
    RolloutStorage.insert_batch(st, *args)                           # (the tensors exist: the slot is written, with 0)
    assert hip.N_CALLS == n0 + 5
    got = [host(s.costs).tolist() for p in st for s in p]
    assert got == [[0.0, 0.5, 0.0, 0.0, 0.0], [0.0, 0.5, 0.0, 0.0, 0.0], [0.0, 0.25, 0.0, 0.0, 0.0], [0.0] * 5]
    one = mk()[0][0]
    one.insert(outs[0][0], torch.tensor([1]), torch.tensor([0.0]), torch.tensor([0.0]), 1.0, torch.tensor([[1.0]]), None, 0)
    one.insert(outs[0][0], torch.tensor([1]), torch.tensor([0.0]), torch.tensor([0.0]), 1.0, torch.tensor([[1.0]]), None, 0, cost=0.5)
    assert host(one.costs).tolist() == [0.0, 0.5, 0.0, 0.0, 0.0]


# ----------------------------------------------------------------------------- the training loops
def test_train_vec_and_train_with_the_key(tmp_path, hip):
    """Two episodes of train_vec with two environments and of train(): the key absent and the key None are the same run; with the key the
    run finishes, the log lines carry `constraint:`, lambda moves in the direction of J - budget in both heads, the learner captures no
    further graph between episodes and the parameters are finite; once more with reward_scaling and action_mask beside it; a refused
    combination names its key before anything runs."""
    from cadre_amd.ppo_agent import train as T_
    from ppo_agent import train as train_mod
    from tests.helpers import SyntheticEnv, topology_cfgs

    class CostEnv(SyntheticEnv):
        """Every step costs the steer head 1 and the throttle head nothing: the cost rates are exactly 1 and 0 whichever rows the
        cursor's modulo-(T + 1) drift leaves in 0 .. T - 1."""
        def step(self, action):
            obs, reward, done, info = SyntheticEnv.step(self, action)
            info["cost"] = (1.0, 0.0)
            return obs, reward, done, info
    graphs = []

    def run(tag, n_env=2, **extra):
        lines = []
        train_cfg, agent_cfg, env_cfg, rollout_cfg = topology_cfgs(str(tmp_path / tag), T=8, episodes=2)
        env_cfg.update(num_processes=n_env, port=[2000 + i for i in range(n_env)], routes=["r%d" % i for i in range(n_env)],
                       scenarios=["s"] * n_env, town=["Town01"] * n_env)
        train_cfg.update(save_interval=10 ** 6, log_stats=True, **extra)
        os.makedirs(str(tmp_path / tag), exist_ok=True)
        del graphs[:]
        cb = lambda event, **st: graphs.append(len(st["agent"].learner._graphs)) if event == "update" else None
        agent = train_mod.train_vec(0, train_cfg, agent_cfg, env_cfg, rollout_cfg, n_env, env_cls=CostEnv,
                                    logger=types.SimpleNamespace(log=lines.append), callback=cb)
        torch.cuda.synchronize()
        return agent, [s for s in lines if "approx kl" in s], list(graphs)
    key = dict(cost_constraint=dict(budget=0.1, lambda_init=1.0, lr_lambda=0.5, epochs=1, minibatches=2))

    def check(agent, lines):
        con = agent.constraint
        st = host(con.state).reshape(2, hip.LAG_STRIDE)
        print(lines[-1])
        assert len(lines) == 2 and all("constraint: J " in s and "lambda" in s for s in lines)
        assert st[0, hip.LAG_J] == 1.0 > 0.1 and np.isclose(st[0, hip.LAG_LAMBDA], 1.9, rtol=1e-12, atol=0)      # above the budget: lambda rises
        assert st[1, hip.LAG_J] == 0.0 < 0.1 and np.isclose(st[1, hip.LAG_LAMBDA], 0.9, rtol=1e-12, atol=0)      # below it: lambda falls
        assert st[0, hip.LAG_SHARE] == 1.0 and st[1, hip.LAG_SHARE] == 0.0 and st[:, hip.LAG_UPDATES].tolist() == [2.0, 2.0] and int(con.step_dev) == 4
        assert bool(torch.isfinite(agent.arena.params).all()) and bool(torch.isfinite(con.params).all())
    absent, plain_lines, g_plain = run("a")
    none, _l, _g = run("b", cost_constraint=None)
    assert torch.equal(absent.arena.params, none.arena.params) and none.constraint is None and not any("constraint:" in s for s in plain_lines)
    agent, lines, g_on = run("c", **key)
    check(agent, lines)
    assert len(g_on) == 2 and g_on[0] == g_on[1] and g_on == g_plain         # no graph is captured between the episodes
    assert agent.arena.step == absent.arena.step and not torch.equal(agent.arena.params, absent.arena.params)
    from cadre_amd.actmask import allowed_from_controls
    agent_cfg = topology_cfgs(str(tmp_path / "x"), T=8, episodes=2)[1]
    word = allowed_from_controls(agent_cfg.STEER_CONTROL, -0.5, 0.5)
    agent, lines, _g = run("e", reward_scaling=True, action_mask=lambda obs, info: (word, 0b011), **key)
    check(agent, lines)
    assert all("reward scale" in s for s in lines) and agent.reward_scaler is not None
    # (every refusal by name: tests/test_constraint_cpu.py; here that the loops reach them before anything runs)
    for extra, why in ((dict(sample_reuse=dict(rollouts=2)), "sample_reuse"), (dict(checkpoint_interval=1), "checkpoint_interval")):
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
            T_.train(0, train_cfg, agent_cfg, env_cfg, rollout_cfg, env_cls=CostEnv, logger=types.SimpleNamespace(log=lines.append))
        finally:
            T_.CadreAgent = orig
        torch.cuda.synchronize()
        return made[-1], [s for s in lines if "approx kl" in s]
    absent1, plain1 = run_one("one_a")
    assert absent1.constraint is None and not any("constraint:" in s for s in plain1)
    with1, one = run_one("one_c", **key)
    check(with1, one)
    assert with1.arena.step == absent1.arena.step and not torch.equal(with1.arena.params, absent1.arena.params)
