"""GPU: the vectorised ensemble evaluation (ppo_agent/evaluate.py, csrc/ensemble.hip) — both kernels alone against
cadre_sample_rows and the float64 references of tests/ensemble_ref.py, EnsembleEvaluator against the existing API's loop
(`CadreAgent.ensemble_act` per environment + `avg_action`), stacking against every agent's own act_batch, re-sync after
the agents' parameters change, isolation from the agents' own state, deterministic actions and evaluate_vec."""
import numpy as np
import pytest
import torch

from cadre_amd import synth
from tests import ensemble_ref
from tests.test_act_batch_gpu import build_agent, env_streams, obs_of, rel

pytestmark = pytest.mark.gpu
H = W = 84
K = (33, 3)


def make_group(M, C, first_seed=11):
    """M agents with one encoder checkpoint and different PPO nets."""
    return [build_agent(H, W, C, ppo_seed=first_seed + m) for m in range(M)]


# ----------------------------------------------------------------------------- the kernels alone
def _sample_case(N, Mg, C, seed):
    from ppo_agent.agent import command_rows
    g = torch.Generator().manual_seed(seed)
    m0, M = 1, Mg + 2
    cmd = torch.randint(0, C, (N,), generator=g).tolist()
    if N >= C:
        cmd[:C] = list(range(C))[::-1]                       # every command, rows not in environment order
    pos, _seg = command_rows(cmd, C)
    O3 = torch.zeros(4 * Mg * C, N, 64)
    O3[:, :, :33] = torch.randn(4 * Mg * C, N, 33, generator=g) * 2
    q = torch.ones(N, M, 2, 64)
    for h in range(2):
        q[:, :, h, :K[h]] = torch.empty(N, M, K[h]).exponential_(1, generator=g)
    return m0, M, cmd, pos, O3, q


def _run_ens(O3_d, pos_d, cmd_d, N, C, Mg, m0, M, q_d, table):
    from cadre_amd import hip
    act = torch.full((N, M, 2), -7, dtype=torch.int64, device="cuda")
    lp = torch.full((N, M, 2), -7.0, device="cuda")
    v = torch.full((N, M, 2), -7.0, device="cuda")
    hip.check(hip.lib().cadre_sample_rows_ens(O3_d.data_ptr(), 64, N * 64, pos_d.data_ptr(), cmd_d.data_ptr(), N, C, Mg, m0, M,
                                              None if q_d is None else q_d.data_ptr(), K[0], K[1], act.data_ptr(), lp.data_ptr(),
                                              v.data_ptr(), None if table is None else table.data_ptr(), hip.stream()),
              "cadre_sample_rows_ens")
    return act.cpu(), lp.cpu(), v.cpu()


@pytest.mark.parametrize("N,Mg,C", [(1, 1, 1), (5, 4, 4), (3, 2, 6)])
def test_sample_rows_ens_kernel(N, Mg, C):
    """Random q: action, log-prob and value bit-identical to one cadre_sample_rows (/ _ord) call per agent on that agent's
    slice of O3.  q = NULL: the float64 reference's first-index argmax, a row with two bit-equal largest logits and the
    ordinal form included.  Entries of the agents outside [m0, m0 + Mg) stay untouched."""
    from cadre_amd import hip
    from tests.test_ordinal_gpu import ord_table, random_rank
    L = hip.lib()
    m0, M, cmd, pos, O3, q = _sample_case(N, Mg, C, 40 + N)
    # a tie: the two largest logits of (environment 0, agent Mg - 1, steer) are bit-equal, at bins 20 and 7
    zt = 2 * ensemble_ref.net_index(0, Mg - 1, cmd[0], Mg, C)
    O3[zt, pos[0], 20] = O3[zt, pos[0], 7] = O3[zt, pos[0], :33].max() + 0.5
    ranks = (random_rank(33, torch.Generator().manual_seed(1)), random_rank(3, torch.Generator().manual_seed(2)))
    O3_d, q_d = O3.cuda(), q.cuda()
    pos_d, cmd_d = torch.from_numpy(pos).cuda(), torch.tensor(cmd, dtype=torch.int32).cuda()
    for table in (None, ord_table((None, None)), ord_table(ranks), ord_table((ranks[0], None))):
        act, lp, v = _run_ens(O3_d, pos_d, cmd_d, N, C, Mg, m0, M, q_d, table)
        outside = [m for m in range(M) if not m0 <= m < m0 + Mg]
        assert bool((act[:, outside] == -7).all()) and bool((lp[:, outside] == -7.0).all()) and bool((v[:, outside] == -7.0).all())
        for j in range(Mg):
            # agent j's towers as the [4 C] tower block of an arena of its own
            idx = [2 * ensemble_ref.net_index(h, j, c, Mg, C) + t for h in range(2) for c in range(C) for t in range(2)]
            Oj = O3[idx].contiguous().cuda()
            qj = q[:, m0 + j].contiguous().cuda()
            a1 = torch.zeros(N, 2, dtype=torch.int64, device="cuda"); l1 = torch.zeros(N, 2, device="cuda"); v1 = torch.zeros(N, 2, device="cuda")
            args = (Oj.data_ptr(), 64, N * 64, pos_d.data_ptr(), cmd_d.data_ptr(), N, C, qj.data_ptr(), K[0], K[1], a1.data_ptr(),
                    l1.data_ptr(), v1.data_ptr())
            if table is None:
                hip.check(L.cadre_sample_rows(*args, hip.stream()), "cadre_sample_rows")
            else:
                hip.check(L.cadre_sample_rows_ord(*args, table.data_ptr(), hip.stream()), "cadre_sample_rows_ord")
            assert torch.equal(act[:, m0 + j], a1.cpu()) and torch.equal(lp[:, m0 + j], l1.cpu()) and torch.equal(v[:, m0 + j], v1.cpu())
    # greedy
    for table, rk in ((None, (None, None)), (ord_table(ranks), ranks), (ord_table((None, ranks[1])), (None, ranks[1]))):
        act, lp, v = _run_ens(O3_d, pos_d, cmd_d, N, C, Mg, m0, M, None, table)
        for e in range(N):
            for j in range(Mg):
                for h in range(2):
                    z = 2 * ensemble_ref.net_index(h, j, cmd[e], Mg, C)
                    row = O3[z, pos[e], :K[h]].double().numpy()
                    want, want_lp = ensemble_ref.greedy(row, rk[h])
                    lg = np.sort(row if rk[h] is None else ensemble_ref.ordinal_logits(row, rk[h]))
                    tied = rk[h] is None and z == zt and e == 0
                    assert tied or lg[-1] - lg[-2] > 1e-4          # (the data: no other near-tie a float32 softmax could flip)
                    assert int(act[e, m0 + j, h]) == want, (e, j, h)
                    assert abs(float(lp[e, m0 + j, h]) - want_lp) < 1e-5 * max(1.0, float(np.abs(lg - lg[-1] + want_lp).max()))
                    assert float(v[e, m0 + j, h]) == float(O3[z + 1, pos[e], 0])
        if table is None:
            assert int(act[0, m0 + Mg - 1, 0]) == 7             # the lowest index of the tie


@pytest.mark.parametrize("N", [1, 5])
@pytest.mark.parametrize("M", [1, 2, 3, 6])
def test_ensemble_controls_kernel(N, M):
    """Bit-identical to the float64 reference (which test_ensemble_eval_cpu pins to avg_action), the brake edges, and NaN
    for exactly the environment with a bin outside its table."""
    from cadre_amd import hip
    L = hip.lib()
    st = np.array([(i - 16) / 3.0 for i in range(33)])
    tt = np.array([[0, 0], [0, 1], [0.6, 0]], dtype=np.float64)
    r = np.random.RandomState(10 * N + M)
    acts = np.stack([r.randint(0, 33, (N, M)), r.randint(0, 3, (N, M))], -1).astype(np.int64)
    acts[0, :, 1] = ([1] + [0] * (M - 1))                        # one brake of 1: 1/M — 0.5 stays (M = 2), 1/3 becomes 0, M = 1 stays 1
    st_d, tt_d = torch.from_numpy(st).cuda(), torch.from_numpy(tt).cuda()

    def run(a):
        a_d = torch.from_numpy(a).cuda()
        out = torch.full((N, 3), 99.0, dtype=torch.float64, device="cuda")
        hip.check(L.cadre_ensemble_controls(a_d.data_ptr(), N, M, st_d.data_ptr(), 33, tt_d.data_ptr(), 3, out.data_ptr(),
                                            hip.stream()), "cadre_ensemble_controls")
        return out.cpu().numpy()
    got, want = run(acts), ensemble_ref.controls(acts, st, tt)
    assert got.tobytes() == want.tobytes()
    assert got[0, 2] == {1: 1.0, 2: 0.5}.get(M, 0.0)
    for bad_e, bad in ((N - 1, (33, 0)), (0, (-1, 0)), (N // 2, (0, 3)), (0, (2 ** 40, 0))):
        a2 = acts.copy()
        a2[bad_e, M - 1] = bad
        got2 = run(a2)
        assert np.isnan(got2[bad_e]).all()
        keep = [e for e in range(N) if e != bad_e]
        assert got2[keep].tobytes() == want[keep].tobytes()


# ----------------------------------------------------------------------------- the evaluator against the loop
def _loop_step(group, obs):
    """The existing API: ensemble_act per environment + avg_action."""
    rows = []
    for o in obs:
        ens = group[0].__class__.ensemble_act(group, o)
        rows.append((ens, group[0].avg_action([t[1] for t in ens])))
    return rows


def _flat(ens):
    f = ens[0][0].cpu()
    return (f, [[int(t[1][0]), int(t[1][1])] for t in ens], [[float(t[2][0]), float(t[2][1])] for t in ens],
            [[float(t[3][0]), float(t[3][1])] for t in ens])


def _check_against_loop(want, got, tag=""):
    """want / got: per step, per environment (flat ensemble, controls, route_fig)."""
    lp_w, lp_g, v_w, v_g = [], [], [], []
    for t, (wr, gr) in enumerate(zip(want, got)):
        assert len(wr) == len(gr)
        for e, ((wf, wa, wl, wv), wc, wroute), ((gf, ga, gl, gv), gc, groute) in zip(range(len(wr)), wr, gr):
            assert torch.equal(wf, gf), (tag, t, e)
            assert wa == ga, (tag, t, e, wa, ga)
            assert wc == gc, (tag, t, e, wc, gc)
            assert np.array_equal(wroute, groute), (tag, t, e)
            lp_w += sum(wl, []); lp_g += sum(gl, []); v_w += sum(wv, []); v_g += sum(gv, [])
    print("%s log-prob rel %.1e, value rel %.1e" % (tag, rel(lp_g, lp_w), rel(v_g, v_w)))
    assert rel(lp_g, lp_w) < 1e-6 and rel(v_g, v_w) < 1e-6


@pytest.mark.parametrize("N,M,C", [(1, 1, 4), (5, 3, 4), (3, 5, 4), (4, 3, 2), (3, 3, 6)])
def test_evaluator_equals_ensemble_act_loop(N, M, C):
    """EnsembleEvaluator.act over N environments == `for e: CadreAgent.ensemble_act(group, obs_e)` after the same seed:
    features bit-exact, actions equal, log-probs and values within 1e-6 relative (the bar between the batched and the
    one-row chain), the caller's route_fig mutated alike, the same global-RNG consumption, and
    `.controls[e] == lead.avg_action(...)` exactly — with the frames compared on the host and with `shifted` hints."""
    from ppo_agent.evaluate import EnsembleActBatch, EnsembleEvaluator
    T = 6
    streams, restarts = env_streams(N, H, W, C, T)
    ref = make_group(M, C)
    torch.manual_seed(123)
    want = []
    for t in range(T):
        obs = [obs_of(streams[e][t]) for e in range(N)]
        want.append([(_flat(ens), ctl, o["route_fig"]) for (ens, ctl), o in zip(_loop_step(ref, obs), obs)])
    rng_want = torch.rand(1).item()
    for hint in (False, True):
        ev = EnsembleEvaluator(make_group(M, C), max_envs=N)
        assert [g.Mg for g in ev.groups] == ensemble_ref.group_split(M, C)
        torch.manual_seed(123)
        got = []
        for t in range(T):
            obs = [obs_of(streams[e][t]) for e in range(N)]
            hints = [t > 0 and t != restarts[e] for e in range(N)] if hint else None
            out = ev.act(obs, shifted=hints)
            assert isinstance(out, EnsembleActBatch) and len(out) == N and all(len(r) == M for r in out)
            assert tuple(out.action.shape) == (N, M, 2) and out.action.dtype == torch.int64
            assert tuple(out.logp.shape) == tuple(out.value.shape) == (N, M, 2) and tuple(out.feat.shape) == (N, 8, 544)
            f, a, lp, v, hid = out[0][0]
            assert tuple(f.shape) == (8, 530) and a[0].dim() == 0 and tuple(lp[0].shape) == tuple(v[1].shape) == (1, 1)
            assert float(hid[0].abs().sum()) == 0.0
            assert all(isinstance(x, float) for row in out.controls for x in row) and len(out.controls) == N
            got.append([(_flat(out[e]), out.controls[e], obs[e]["route_fig"]) for e in range(N)])
        assert torch.rand(1).item() == rng_want                   # same RNG consumption as the loop
        _check_against_loop(want, got, "evaluator N=%d M=%d C=%d hints=%s:" % (N, M, C, hint))


def _feed_noise(monkeypatch, rows):
    """Every `exponential_` draw takes the next prepared row (the sampler noise of a run, in its draw order)."""
    it = iter(rows)

    def fake(self, lambd=1, generator=None):
        r = next(it)
        assert self.shape[-1] == r.numel()
        return self.copy_(r.view_as(self))
    monkeypatch.setattr(torch.Tensor, "exponential_", fake)


def test_stacking_changes_no_bit(monkeypatch):
    """For every agent m, `.logp[:, m]` and `.value[:, m]` of the evaluator (M = 6, C = 4: groups of 4 + 2, 32 and 16
    stacked nets) equal that agent's own act_batch (8 nets) on the same observations and the same q, bit for bit: the
    per-net work is the same rows, the same weights and the same kernels."""
    from ppo_agent.evaluate import EnsembleEvaluator
    N, M, C, T = 5, 6, 4, 3
    streams, _ = env_streams(N, H, W, C, T)
    group = make_group(M, C)
    g = torch.Generator().manual_seed(77)
    noise = [[[[torch.empty(K[h]).exponential_(1, generator=g) for h in range(2)] for m in range(M)] for e in range(N)]
             for t in range(T)]
    ev = EnsembleEvaluator(group, max_envs=N)
    _feed_noise(monkeypatch, [noise[t][e][m][h] for t in range(T) for e in range(N) for m in range(M) for h in range(2)])
    outs = []
    for t in range(T):
        out = ev.act([obs_of(streams[e][t]) for e in range(N)])
        outs.append((out.action.cpu(), out.logp.cpu(), out.value.cpu(), out.feat.cpu()))
    n_diff = 0
    worst = 0.0
    for m in range(M):
        solo = build_agent(H, W, C, ppo_seed=11 + m)
        _feed_noise(monkeypatch, [noise[t][e][m][h] for t in range(T) for e in range(N) for h in range(2)])
        for t in range(T):
            ab = solo.act_batch([obs_of(streams[e][t]) for e in range(N)])
            act, lp, v, feat = outs[t]
            assert torch.equal(feat, ab.feat.cpu())
            assert torch.equal(act[:, m], ab.action.cpu()), (m, t)
            n_diff += int((lp[:, m] != ab.logp.cpu()).sum()) + int((v[:, m] != ab.value.cpu()).sum())
            worst = max(worst, rel(lp[:, m], ab.logp.cpu()), rel(v[:, m], ab.value.cpu()))
    print("stacking: %d of %d log-probs / values differ, worst rel %.1e" % (n_diff, 4 * N * M * T, worst))
    assert n_diff == 0


def test_resync_after_snapshot_load_and_optimiser_step(tmp_path):
    """After group[1].load_snapshot(...) and after an in-place optimiser step on group[2], the next call equals the loop
    again; on the same observations exactly the changed agent's values move, and a call after no change copies nothing."""
    from cadre_amd.ppo_agent.models import _no_orthogonal_init
    from ppo_agent.evaluate import EnsembleEvaluator
    N, M, C = 2, 3, 4
    streams, _ = env_streams(N, H, W, C, 2)
    group = make_group(M, C)
    ev = EnsembleEvaluator(group, max_envs=N)

    def both(t, seed):
        obs = [obs_of(streams[e][t]) for e in range(N)]
        torch.manual_seed(seed)
        want = [[(_flat(ens), ctl, o["route_fig"]) for (ens, ctl), o in zip(_loop_step(group, obs), obs)]]
        obs = [obs_of(streams[e][t]) for e in range(N)]
        torch.manual_seed(seed)
        out = ev.act(obs)
        _check_against_loop(want, [[(_flat(out[e]), out.controls[e], obs[e]["route_fig"]) for e in range(N)]], "re-sync %d:" % seed)
        return out.value.cpu()
    v0 = both(0, 5)
    path = str(tmp_path / "other.pt")
    with _no_orthogonal_init():                                   # (the snapshot's containers are filled right away)
        build_agent(H, W, C, ppo_seed=31).save_snapshot(path, fix_missing_lstm=True)
    group[1].load_snapshot(path, None)
    v1 = both(0, 6)
    assert torch.equal(v1[:, 0], v0[:, 0]) and torch.equal(v1[:, 2], v0[:, 2]) and not torch.equal(v1[:, 1], v0[:, 1])
    a2 = group[2].arena
    a2.grads.copy_(torch.randn(a2.total, generator=torch.Generator().manual_seed(3)).to(a2.device) * 1e-2)
    group[2].learner.clip_adam(lr=1e-2)
    v2 = both(0, 7)
    assert torch.equal(v2[:, :2], v1[:, :2]) and not torch.equal(v2[:, 2], v1[:, 2])
    keys = [g.keys[:] for g in ev.groups]
    v3 = both(1, 8)                                               # nothing changed: no copy, still the loop
    assert [g.keys for g in ev.groups] == keys and tuple(v3.shape) == (N, M, 2)


def test_evaluator_leaves_the_agents_state_alone():
    """An act_batch run on the lead agent with `shifted` hints, with and without evaluator calls interleaved between its
    steps: bit-identical outputs, caches and `control._last_*`."""
    from ppo_agent.evaluate import EnsembleEvaluator
    N, C, T = 3, 4, 5
    streams, restarts = env_streams(N, H, W, C, T)
    other, _ = env_streams(2, H, W, C, T)
    plain, lead = build_agent(H, W, C), build_agent(H, W, C)
    group = [lead] + make_group(2, C, first_seed=12)
    ev = EnsembleEvaluator(group, max_envs=2)
    for t in range(T):
        hints = [t > 0 and t != restarts[e] for e in range(N)]
        res = []
        for ag in (plain, lead):
            obs = [obs_of(streams[e][t]) for e in range(N)]
            torch.manual_seed(50 + t)
            ab = ag.act_batch(obs, shifted=hints)
            res.append((ab.feat.cpu(), ab.action.cpu(), ab.logp.cpu(), ab.value.cpu(), [o["route_fig"] for o in obs]))
        for x, y in zip(res[0][:4], res[1][:4]):
            assert torch.equal(x, y), t
        assert all(np.array_equal(x, y) for x, y in zip(res[0][4], res[1][4]))
        for name in ("steer_ppo_0", "throttle_ppo_1"):
            la, lb = plain.model_dict[name].control, lead.model_dict[name].control
            assert (getattr(la, "_last_action", None) is None) == (getattr(lb, "_last_action", None) is None)
            if getattr(la, "_last_action", None) is not None:
                assert torch.equal(la._last_action.cpu(), lb._last_action.cpu()) and torch.equal(la._last_logp.cpu(), lb._last_logp.cpu())
        assert lead._cache is None and lead._ag is None
        ev.act([obs_of(other[e][t]) for e in range(2)], deterministic=bool(t % 2))     # between the lead agent's steps
        assert lead._cache is None and lead._ag is None
        assert torch.equal(plain._vec["ring"], lead._vec["ring"])


def test_deterministic_actions():
    """deterministic=True on act, act_batch and the evaluator (M = 1): the three agree (evaluator and act_batch bit for
    bit: one agent is the same arena; act's one-row chain within 1e-6), the greedy action is the first largest log-prob
    and the generator state is unchanged."""
    from ppo_agent.evaluate import EnsembleEvaluator
    N, C, T = 3, 4, 4
    streams, _ = env_streams(N, H, W, C, T)
    one, batch, solo = build_agent(H, W, C), build_agent(H, W, C), build_agent(H, W, C)
    ev = EnsembleEvaluator([solo], max_envs=N)
    torch.manual_seed(9)
    state = torch.get_rng_state()
    lp_a, lp_b = [], []
    for t in range(T):
        acts = [one.act(obs_of(streams[e][t]), deterministic=True) for e in range(N)]
        ab = batch.act_batch([obs_of(streams[e][t]) for e in range(N)], deterministic=True)
        out = ev.act([obs_of(streams[e][t]) for e in range(N)], deterministic=True)
        assert torch.equal(out.action[:, 0], ab.action) and torch.equal(out.logp[:, 0], ab.logp) and torch.equal(out.value[:, 0], ab.value)
        assert torch.equal(out.feat, ab.feat)
        for e in range(N):
            assert [int(acts[e][1][0]), int(acts[e][1][1])] == ab.action[e].tolist(), (t, e)
            assert out.controls[e] == batch.avg_action([ab[e][1]])
            lp_a += [float(acts[e][2][0]), float(acts[e][2][1])]
        lp_b += ab.logp.reshape(-1).tolist()
        # greedy: the log-prob returned is the largest of the row (recomputed from the towers the evaluator just ran)
        O3 = ev.groups[0].learner.workspace(N, 2 * C, 8)["O3"]
        from ppo_agent.agent import command_rows
        cmds = [int(streams[e][t]["command"]) for e in range(N)]
        pos, _ = command_rows(cmds, C)
        for e in range(N):
            for h in range(2):
                row = O3[2 * (h * C + cmds[e]), int(pos[e]), :K[h]].double().cpu().numpy()
                k, lp = ensemble_ref.greedy(row)
                assert int(out.action[e, 0, h]) == k and abs(float(out.logp[e, 0, h]) - lp) < 1e-5 * max(1.0, abs(lp))
    assert rel(lp_a, lp_b) < 1e-6
    assert torch.equal(torch.get_rng_state(), state)              # nothing was drawn


class _SynthEnv(object):
    """Open-loop synthetic environment: every reset starts a new synth_rollout stream; episode n lasts plan[n] steps; step t
    pays (t + 1, 0.5)."""

    def __init__(self, ident, plan, C):
        self.id, self.plan, self.C, self.resets, self.controls = ident, plan, C, 0, []

    def _obs(self):
        td = self.steps[self.t]
        return dict(rgb=td["rgb"], route_fig=td["route_fig"].copy(), measurements=td["measurements"], command=td["command"] % self.C)

    def reset(self):
        self.steps = synth.synth_rollout(self.plan[self.resets] + 1, H, W, seed=900 + 10 * self.id + self.resets)
        self.resets += 1
        self.t = 0
        self.controls.append([])
        return self._obs()

    def step(self, control):
        self.controls[-1].append(control)
        self.t += 1
        return self._obs(), [float(self.t), 0.5], self.t == self.plan[self.resets - 1], dict(env=self.id)


def test_evaluate_vec_with_synthetic_environments():
    """N = 3, M = 2, episodes = 5: five records with the scripted lengths and reward sums; the active list shrinks and the
    controls every environment received still equal the per-environment loop's (greedy: no generator order involved);
    two runs give identical records; the sampled mode runs the same schedule."""
    from ppo_agent.evaluate import EnsembleEvaluator, evaluate_vec
    C, M = 4, 2
    plans = [[3, 2], [2, 3], [6]]
    group = make_group(M, C)
    ev = EnsembleEvaluator(group, max_envs=3)
    sizes = []
    act0 = ev.act

    def spy(obs_list, **kw):
        sizes.append(len(obs_list))
        return act0(obs_list, **kw)
    ev.act = spy
    runs = []
    for seed in (1, 2):
        envs = [_SynthEnv(i, plans[i], C) for i in range(3)]
        torch.manual_seed(seed)
        state = torch.get_rng_state()
        recs = evaluate_vec(group, envs, 5, deterministic=True, evaluator=ev)
        assert torch.equal(torch.get_rng_state(), state)
        runs.append((recs, [e.controls for e in envs]))
    assert runs[0] == runs[1]
    recs, controls = runs[0]
    assert sorted(r["episode"] for r in recs) == list(range(5)) and [e.resets for e in envs] == [2, 2, 1]
    want_len = {(0, 0): 3, (1, 1): 2, (2, 2): 6, (1, 3): 3, (0, 4): 2}           # (env, episode): environment 1 restarts first
    assert {(r["env"], r["episode"]): r["length"] for r in recs} == want_len
    for r in recs:
        n = r["length"]
        assert r["reward_sum"] == (n * (n + 1) / 2.0, 0.5 * n) and r["info"] == dict(env=r["env"])
    assert sizes[0] == 3 and min(sizes) < 3                                       # the active list shrank
    # the loop, environment by environment, on fresh agents with the same weights
    ref = make_group(M, C)
    for i in range(3):
        env = _SynthEnv(i, plans[i], C)
        for n, plan_len in enumerate(plans[i]):
            o = env.reset()
            for t in range(plan_len):
                feat = ref[0].get_latent_feature(o)
                acts = [a.act_from_feature(feat, o["command"], deterministic=True)[1] for a in ref]
                assert controls[i][n][t] == ref[0].avg_action(acts), (i, n, t)
                o, _r, _d, _i = env.step(None)
    # sampled mode: the same schedule, five records
    envs = [_SynthEnv(i, plans[i], C) for i in range(3)]
    torch.manual_seed(3)
    state = torch.get_rng_state()
    recs = evaluate_vec(group, envs, 5, evaluator=ev)
    assert {(r["env"], r["episode"]): r["length"] for r in recs} == want_len
    assert not torch.equal(torch.get_rng_state(), state)                          # (sampled: the generator moved on)


def test_ensemble_act_batch_keeps_one_evaluator_per_group():
    from ppo_agent.agent import CadreAgent
    N, M, C = 2, 2, 4
    streams, _ = env_streams(N, H, W, C, 2)
    group, ref = make_group(M, C), make_group(M, C)
    torch.manual_seed(4)
    want = []
    for t in range(2):
        obs = [obs_of(streams[e][t]) for e in range(N)]
        want.append([(_flat(ens), ctl, o["route_fig"]) for (ens, ctl), o in zip(_loop_step(ref, obs), obs)])
    torch.manual_seed(4)
    got = []
    for t in range(2):
        obs = [obs_of(streams[e][t]) for e in range(N)]
        out = CadreAgent.ensemble_act_batch(group, obs)
        got.append([(_flat(out[e]), out.controls[e], obs[e]["route_fig"]) for e in range(N)])
    _check_against_loop(want, got, "ensemble_act_batch:")
    assert len(group[0]._ens_eval) == 1


def test_evaluator_with_ordinal_agents():
    """Two ordinal agents (the shipped non-monotone steering table): the evaluator, sampled and greedy, against the loop."""
    from ppo_agent.evaluate import EnsembleEvaluator
    from tests.test_ordinal_gpu import make_agent as ordinal_agent
    N, C, T = 3, 4, 3
    streams, _ = env_streams(N, H, W, C, T)
    group = [ordinal_agent(True, ppo_seed=11), ordinal_agent(True, ppo_seed=12)]
    ev = EnsembleEvaluator([ordinal_agent(True, ppo_seed=11), ordinal_agent(True, ppo_seed=12)], max_envs=N)
    assert ev.groups[0].arena.ord is not None and ev.groups[0].arena.ordinal_rank == group[0].ordinal_rank
    torch.manual_seed(21)
    want = []
    for t in range(T):
        obs = [obs_of(streams[e][t]) for e in range(N)]
        want.append([(_flat(ens), ctl, o["route_fig"]) for (ens, ctl), o in zip(_loop_step(group, obs), obs)])
    torch.manual_seed(21)
    got = []
    for t in range(T):
        obs = [obs_of(streams[e][t]) for e in range(N)]
        out = ev.act(obs)
        got.append([(_flat(out[e]), out.controls[e], obs[e]["route_fig"]) for e in range(N)])
    _check_against_loop(want, got, "ordinal evaluator:")
    # greedy: the loop's greedy form on the same agents
    obs = [obs_of(streams[e][0]) for e in range(N)]
    out = ev.act([obs_of(streams[e][0]) for e in range(N)], deterministic=True)
    for e, o in enumerate(obs):
        feat = group[0].get_latent_feature(o)
        acts = [a.act_from_feature(feat, o["command"], deterministic=True)[1] for a in group]
        assert [[int(a[0]), int(a[1])] for a in acts] == out.action[e].tolist()
        assert out.controls[e] == group[0].avg_action(acts)


def test_evaluate_loads_the_snapshots_and_runs_the_episodes(tmp_path):
    """evaluate() (eval.py:12-64): one agent per load_episode entry with that snapshot's weights, environment i built from
    entry i of the per-worker keys, eval_episode episodes; the controls are those of an ensemble with the saved weights."""
    import os
    from cadre_amd.ppo_agent.models import _no_orthogonal_init
    from ppo_agent.evaluate import evaluate
    from tests.helpers import AD, topology_cfgs
    _train, agent_cfg, env_cfg, rollout_cfg = topology_cfgs(str(tmp_path), H=H, W=W)
    env_cfg.update(port=[2000, 2001], routes=["r0", "r1"], scenarios=["s0", "s1"], town=["Town01", "Town02"])
    os.makedirs(str(tmp_path / "models"))
    with _no_orthogonal_init():                                   # (the snapshot's containers are filled right away)
        for ep, seed in ((0, 11), (3, 12)):
            build_agent(H, W, 4, ppo_seed=seed).save_snapshot(str(tmp_path / "models" / ("ppo_model_%d.pt" % ep)), fix_missing_lstm=True)
    eval_cfg = AD(pretrained_path=str(tmp_path), load_episode=[0, 3], eval_episode=3, deterministic=True)
    made = []

    class Env(_SynthEnv):
        def __init__(self, cfg):
            _SynthEnv.__init__(self, int(cfg["rank"]), [2, 3], 4)
            made.append((dict(cfg), self))
    recs = evaluate(eval_cfg, agent_cfg, env_cfg, rollout_cfg, num_envs=2, env_cls=Env)
    assert [(r["episode"], r["env"], r["length"]) for r in recs] == [(0, 0, 2), (1, 1, 2), (2, 0, 3)]
    assert [c["port"] for c, _e in made] == [2000, 2001] and [c["town"] for c, _e in made] == ["Town01", "Town02"]
    assert all(c["seq_length"] == 8 and c["pretrained_path"] == str(tmp_path) for c, _e in made)
    assert env_cfg["port"] == [2000, 2001]                        # the caller's config is not consumed
    ref = make_group(2, 4)
    env = _SynthEnv(0, [2, 3], 4)
    for n, plan_len in enumerate([2, 3]):
        o = env.reset()
        for t in range(plan_len):
            feat = ref[0].get_latent_feature(o)
            acts = [a.act_from_feature(feat, o["command"], deterministic=True)[1] for a in ref]
            assert made[0][1].controls[n][t] == ref[0].avg_action(acts), (n, t)
            o = env.step(None)[0]
