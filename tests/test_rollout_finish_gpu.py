"""GPU: the rollout-finishing stage (csrc/rollout_finish.hip) — cadre_gae_multi against per-storage cadre_gae (bit-exact with
the options off), the time-limit cut and the scaled scan against a numpy strict-order scan (float32, one operation per
statement, as oracle/ppo_ref.py writes GAE), the return statistics against a float64 numpy reference, insert_batch with
flags against insert(), and train_vec end to end."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GAMMA, TAU = 0.99, 0.95
f32 = np.float32


# ----------------------------------------------------------------------------- reference arithmetic
def np_scan(r, V, m, nv, keep=None, scale=None, clip=None):
    """storage.py:69-76 in float32, one rounding per operation; `keep` = 1 - time_limit multiplies gae after the
    recurrence, `scale` / `clip` rewrite the reward where it is read.  Returns (returns[:T], raw advantages, V)."""
    T = len(r) - 1
    V = V.astype(f32).copy()
    V[T] = f32(nv)
    g, gt = f32(GAMMA), f32(GAMMA * TAU)
    ret = np.zeros(T, dtype=f32)
    gae = f32(0.0)
    for t in range(T - 1, -1, -1):
        rt = f32(r[t])
        if scale is not None:
            rt = f32(rt * f32(scale))
            rt = f32(min(max(rt, f32(-clip)), f32(clip)))
        t1 = f32(g * V[t + 1])
        t2 = f32(t1 * m[t])
        t3 = f32(rt + t2)
        delta = f32(t3 - V[t])
        u1 = f32(gt * m[t])
        u2 = f32(u1 * gae)
        gae = f32(delta + u2)
        if keep is not None:
            gae = f32(gae * keep[t])
        ret[t] = f32(gae + V[t])
    adv = (ret - V[:T]).astype(f32)
    return ret, adv, V


def np_disc_returns(r, m, tl, carry):
    """G_t = r_t + gamma m'_{t-1} G_{t-1} in float64 over rows 0 .. T-1; carry = (G, m') of the row before row 0."""
    G, pm = carry
    out = []
    for t in range(len(r)):
        G = float(r[t]) + GAMMA * pm * G
        out.append(G)
        pm = float(m[t]) * (1.0 - float(tl[t]))
    return out, (G, pm)


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def make_storages(n, T, seed, flags=0.0):
    from ppo_agent.storage import RolloutStorage
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        s = RolloutStorage(T, 2, 32, 1, 32, True, GAMMA, TAU)
        s.rewards.copy_(torch.rand(T + 1, 1, generator=g) * 2.0 - 0.5)
        s.value_preds.copy_(torch.randn(T + 1, 1, generator=g) * 0.3)
        s.masks.copy_((torch.rand(T + 1, 1, generator=g) >= 0.1).float())
        if flags:
            s.time_limits.copy_((torch.rand(T + 1, 1, generator=g) < flags).float())
            s._tl_used = True
        s.to("cuda:0")
        out.append(s)
    nv = (torch.randn(n, generator=g) * 0.3).tolist()
    return out, nv


def host(s):
    return {k: getattr(s, k)[:, 0].cpu().numpy().copy() for k in ("rewards", "value_preds", "masks", "time_limits")}


# ----------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("normalise", [False, True])
@pytest.mark.parametrize("T", [8, 128, 200])
@pytest.mark.parametrize("n", [2, 8, 64])
def test_options_off_is_todays_gae(n, T, normalise):
    """finish_rollouts (one cadre_gae_multi launch) == n compute_returns (n cadre_gae launches), bit for bit."""
    from cadre_amd import hip
    from ppo_agent.storage import RolloutStorage
    a, nv = make_storages(n, T, 100 + n + T)
    b, _ = make_storages(n, T, 100 + n + T)
    c0 = hip.N_CALLS
    advs = RolloutStorage.finish_rollouts(a, nv, normalise=normalise)
    assert hip.N_CALLS - c0 == 1
    for k, (x, y) in enumerate(zip(a, b)):
        ref_adv = y.compute_returns(nv[k], normalise=normalise)
        assert advs[k] is x.advantages
        assert torch.equal(bits(x.returns[:T]), bits(y.returns[:T])), k
        assert torch.equal(bits(x.advantages), bits(ref_adv)), k
        assert torch.equal(bits(x.value_preds), bits(y.value_preds)), k
        assert x.value_preds[T].item() == f32(nv[k])


@pytest.mark.parametrize("T", [8, 200])
def test_time_limit_cut_against_numpy_scan(T):
    from ppo_agent.storage import RolloutStorage
    n = 8
    st, nv = make_storages(n, T, 7 + T, flags=0.2)
    before = [host(s) for s in st]
    assert sum(h["time_limits"][:T].sum() for h in before) > 0
    RolloutStorage.finish_rollouts(st, nv, normalise=False)
    for k, s in enumerate(st):
        h = before[k]
        keep = (f32(1.0) - h["time_limits"]).astype(f32)
        ret, adv, V = np_scan(h["rewards"], h["value_preds"], h["masks"], nv[k], keep=keep)
        got_ret, got_adv = s.returns[:T, 0].cpu().numpy(), s.advantages[:, 0].cpu().numpy()
        assert np.array_equal(got_ret.view(np.int32), ret.view(np.int32)), k
        assert np.array_equal(got_adv.view(np.int32), adv.view(np.int32)), k
        cut = h["time_limits"][:T] == 1
        assert np.array_equal(got_ret[cut], s.value_preds[:T, 0].cpu().numpy()[cut])
        assert not got_adv[cut].any()
    # compute_returns of a storage with flags takes the same kernel with n = 1
    one, _ = make_storages(1, T, 7 + T, flags=0.2)                # (the same draws as storage 0 above)
    adv1 = one[0].compute_returns(nv[0], normalise=False)
    assert torch.equal(bits(adv1), bits(st[0].advantages)) and torch.equal(bits(one[0].returns[:T]), bits(st[0].returns[:T]))


@pytest.mark.parametrize("normalise", [False, True])
def test_all_zero_flags_give_the_bits_of_no_flags(normalise):
    from ppo_agent.storage import RolloutStorage
    a, nv = make_storages(8, 128, 31)
    b, _ = make_storages(8, 128, 31)
    for s in b:
        s._tl_used = True                                        # the table carries the (all-zero) time_limits pointers
    RolloutStorage.finish_rollouts(a, nv, normalise=normalise)
    RolloutStorage.finish_rollouts(b, nv, normalise=normalise)
    for x, y in zip(a, b):
        assert torch.equal(bits(x.returns[:128]), bits(y.returns[:128])) and torch.equal(bits(x.advantages), bits(y.advantages))


def _refill(st, seed, T):
    g = torch.Generator().manual_seed(seed)
    for s in st:
        s.rewards.copy_(torch.rand(T + 1, 1, generator=g) * 3.0)
        s.value_preds.copy_(torch.randn(T + 1, 1, generator=g) * 0.3)
        s.masks.copy_((torch.rand(T + 1, 1, generator=g) >= 0.15).float())
        s.time_limits.copy_((torch.rand(T + 1, 1, generator=g) < 0.1).float())
        s._tl_used = True


def test_return_statistics_three_rollouts():
    """count / mean / M2 per head against float64 numpy on the concatenated discounted returns (1e-12 relative: float64
    sums over <= 10^4 values in another order), the scale formed from them, determinism, and update = 0."""
    from cadre_amd import hip
    from ppo_agent.storage import ReturnScaler, RolloutStorage
    N, T = 4, 50
    n = 2 * N
    runs = []
    for run in range(2):
        st, nv = make_storages(n, T, 11)
        rs = ReturnScaler(N, GAMMA, device="cuda:0")
        carry = [(0.0, 0.0)] * n
        seen = [[], []]
        for ro in range(3):
            _refill(st, 500 + ro, T)
            hs = [host(s) for s in st]
            RolloutStorage.finish_rollouts(st, nv, reward_scaler=rs)
            for k, h in enumerate(hs):
                G, carry[k] = np_disc_returns(h["rewards"][:T], h["masks"][:T], h["time_limits"][:T], carry[k])
                seen[k & 1] += G
            state = rs.state.cpu().numpy()
            for hd in (0, 1):
                x = np.array(seen[hd], dtype=np.float64)
                cnt, mean, M2 = state[3 * hd:3 * hd + 3]
                assert cnt == len(x) == (ro + 1) * N * T
                assert abs(mean - x.mean()) <= 1e-12 * abs(x.mean()), (ro, hd, mean, x.mean())
                m2 = ((x - x.mean()) ** 2).sum()
                assert abs(M2 - m2) <= 1e-12 * m2, (ro, hd, M2, m2)
                want = f32(1.0 / np.sqrt(M2 / cnt + 1e-8))           # (from the device's own float64 statistics: exact)
                assert f32(state[hip.RS_SCALE + hd]) == want and rs.scale()[hd].item() == want
            got_c = state[hip.RS_CARRY:].reshape(n, 2)
            for k in range(n):
                assert abs(got_c[k, 0] - carry[k][0]) <= 1e-12 * abs(carry[k][0]) and got_c[k, 1] == carry[k][1], k
        runs.append((rs.state.clone(), [s.returns.clone() for s in st], [s.advantages.clone() for s in st]))
    assert torch.equal(runs[0][0].view(torch.int64), runs[1][0].view(torch.int64))       # two runs: identical bits
    for i in (1, 2):
        for x, y in zip(runs[0][i], runs[1][i]):
            assert torch.equal(bits(x), bits(y))
    # update = 0: the block stays as it is, the stored scale is used
    frozen = rs.state.clone()
    rs.training = False
    _refill(st, 900, T)
    RolloutStorage.finish_rollouts(st, nv, reward_scaler=rs, normalise=False)
    assert torch.equal(rs.state.view(torch.int64), frozen.view(torch.int64))
    sc = rs.scale().tolist()
    h = host(st[1])
    ret, adv, _ = np_scan(h["rewards"], h["value_preds"], h["masks"], nv[1], keep=(f32(1.0) - h["time_limits"]).astype(f32),
                          scale=sc[1], clip=10.0)
    assert np.array_equal(st[1].advantages[:, 0].cpu().numpy().view(np.int32), adv.view(np.int32))


@pytest.mark.parametrize("clip", [10.0, 0.4])
def test_scaled_scan_against_numpy_with_the_device_scales(clip):
    """The float32 scales read back from the device + `clip` reproduce returns and raw advantages bit for bit; storage.rewards
    keeps the raw rewards.  clip = 0.4 binds on some rows."""
    from ppo_agent.storage import ReturnScaler, RolloutStorage
    N, T = 4, 128
    st, nv = make_storages(2 * N, T, 77, flags=0.05)
    rs = ReturnScaler(N, GAMMA, clip=clip, device="cuda:0")
    before = [host(s) for s in st]
    RolloutStorage.finish_rollouts(st, nv, normalise=False, reward_scaler=rs)
    sc = rs.scale().cpu().numpy()
    assert sc.dtype == np.float32 and (sc != 1.0).all()
    bound = 0
    for k, s in enumerate(st):
        h = before[k]
        bound += int((np.abs(h["rewards"][:T] * sc[k & 1]) > clip).sum())
        ret, adv, _ = np_scan(h["rewards"], h["value_preds"], h["masks"], nv[k], keep=(f32(1.0) - h["time_limits"]).astype(f32),
                              scale=sc[k & 1], clip=clip)
        assert np.array_equal(s.returns[:T, 0].cpu().numpy().view(np.int32), ret.view(np.int32)), k
        assert np.array_equal(s.advantages[:, 0].cpu().numpy().view(np.int32), adv.view(np.int32)), k
        assert np.array_equal(s.rewards[:, 0].cpu().numpy(), h["rewards"])
    assert (bound > 0) == (clip < 1.0)


def test_state_dict_continues_a_run_bit_for_bit():
    from ppo_agent.storage import ReturnScaler, RolloutStorage
    N, T = 4, 50
    out = []
    for resume in (False, True):
        st, nv = make_storages(2 * N, T, 11)
        rs = ReturnScaler(N, GAMMA, device="cuda:0")
        for ro in range(3):
            if resume and ro == 2:
                sd = {k: v.cpu() for k, v in rs.state_dict().items()}
                rs = ReturnScaler(N, GAMMA, device="cuda:0")
                rs.load_state_dict(sd)
            _refill(st, 500 + ro, T)
            RolloutStorage.finish_rollouts(st, nv, reward_scaler=rs)
        out.append((rs.state.clone(), [s.advantages.clone() for s in st], [s.returns.clone() for s in st]))
    assert torch.equal(out[0][0].view(torch.int64), out[1][0].view(torch.int64))
    for i in (1, 2):
        for x, y in zip(out[0][i], out[1][i]):
            assert torch.equal(bits(x), bits(y))


FIELDS = ("_obs", "_hn", "_cn", "action", "action_log_probs", "value_preds", "rewards", "masks", "command", "time_limits")


def test_insert_batch_with_flags_equals_pairs_of_insert():
    """11 steps into T = 4 storages (the cursor wraps at slot T): insert_batch(time_limits=...) == N pairs of
    insert(time_limit=...) on every storage tensor; without flags the tensors are those of today's insert_batch."""
    from ppo_agent.storage import RolloutStorage
    N, T, S, D = 3, 4, 8, 530
    g = torch.Generator().manual_seed(3)
    mk = lambda: [tuple(RolloutStorage(T, 2, D, S, D, True, GAMMA, TAU) for _ in range(2)) for _ in range(N)]
    ref, mine, plain, plain_ref = mk(), mk(), mk(), mk()
    for grp in (ref, mine, plain, plain_ref):
        for p in grp:
            for s in p:
                s.to("cuda:0")
    hidden = (torch.zeros(1, D, device="cuda"), torch.zeros(1, D, device="cuda"))
    for step in range(11):
        feat = torch.randn(N, S, 544, generator=g).cuda()
        action = torch.randint(0, 33, (N, 2), generator=g).cuda()
        logp = torch.randn(N, 2, generator=g).cuda()
        value = torch.randn(N, 2, generator=g).cuda()
        outs = [(feat[e, :, :D], [action[e, 0], action[e, 1]], [logp[e, 0:1].view(1, 1), logp[e, 1:2].view(1, 1)],
                 [value[e, 0:1].view(1, 1), value[e, 1:2].view(1, 1)], hidden) for e in range(N)]
        rewards = torch.rand(N, 2, generator=g).tolist()
        masks = (torch.rand(N, 2, generator=g) > 0.3).float().tolist()
        commands = torch.randint(0, 4, (N,), generator=g).tolist()
        tl = (torch.rand(N, 2, generator=g) < 0.4).tolist()
        flags = [tl[0][0], tuple(tl[1]), tuple(tl[2])]           # a bool, and (steer, throttle) pairs
        pairs = [(tl[0][0], tl[0][0]), tl[1], tl[2]]
        for e in range(N):
            f, a, lp, v, hid = outs[e]
            for h in range(2):
                ref[e][h].insert(f, a[h], lp[h], v[h], rewards[e][h], torch.tensor([[masks[e][h]]]), hid, commands[e],
                                 time_limit=pairs[e][h])
                plain_ref[e][h].insert(f, a[h], lp[h], v[h], rewards[e][h], torch.tensor([[masks[e][h]]]), hid, commands[e])
        RolloutStorage.insert_batch(mine, outs, rewards, masks, commands, time_limits=flags if step != 5 else None)
        if step == 5:                                            # None after flags were used: the rows' flags are cleared
            for e in range(N):
                for h in range(2):
                    ref[e][h].time_limits[(ref[e][h].step - 1) % (T + 1)] = 0.0
        RolloutStorage.insert_batch(plain, outs, rewards, masks, commands)
        for a_grp, b_grp in ((mine, ref), (plain, plain_ref)):
            for e in range(N):
                for h in range(2):
                    assert a_grp[e][h].step == b_grp[e][h].step
                    for k in FIELDS:
                        assert torch.equal(getattr(a_grp[e][h], k), getattr(b_grp[e][h], k)), (step, e, h, k)
    assert ref[0][0].step == 11 % (T + 1)
    assert any(s.time_limits.any().item() for p in mine for s in p)
    assert not any(s._tl_used or s.time_limits.any().item() for p in plain for s in p)


# ----------------------------------------------------------------------------- end to end
def _vec_cfgs(tmp_path, N, T, episodes):
    from tests.helpers import topology_cfgs
    train_cfg, agent_cfg, env_cfg, rollout_cfg = topology_cfgs(str(tmp_path), H=84, W=84, T=T, episodes=episodes)
    env_cfg.update(num_processes=N, port=[2000 + i for i in range(N)], routes=["r%d" % i for i in range(N)],
                   scenarios=["s"] * N, town=["Town01"] * N)
    train_cfg.update(save_interval=10 ** 6)
    return train_cfg, agent_cfg, env_cfg, rollout_cfg


def _env_cls():
    from tests.helpers import SyntheticEnv

    class TimeLimitEnv(SyntheticEnv):
        """SyntheticEnv that reports a step-budget cut on chosen steps: a bool, or a (steer, throttle) pair."""

        def step(self, action):
            i, rank = self.i, int(self.cfg["rank"])
            obs, reward, done, info = SyntheticEnv.step(self, action)
            if rank != 3:                                        # (environment 3 never reports the key)
                info["time_limit"] = (i % 5 == 3, i % 7 == 2) if rank == 1 else (i + rank) % 6 == 4
            return obs, reward, done, info
    return TimeLimitEnv


def test_train_vec_feature_off_is_the_parent_behaviour(tmp_path, monkeypatch):
    """4 environments, 2 episodes, no new option: the arena parameters equal, bit for bit, those of a run whose
    finish_rollouts loops compute_returns per storage (2N cadre_gae launches, the parent's form)."""
    from ppo_agent.storage import RolloutStorage
    from ppo_agent.train import train_vec
    from tests.helpers import SyntheticEnv
    N, T, EP = 4, 8, 2

    def run(sub):
        (tmp_path / sub).mkdir()
        train_cfg, agent_cfg, env_cfg, rollout_cfg = _vec_cfgs(tmp_path / sub, N, T, EP)
        agent = train_vec(0, train_cfg, agent_cfg, env_cfg, rollout_cfg, N, env_cls=SyntheticEnv)
        assert agent.reward_scaler is None
        return agent.arena.params.detach().clone()
    new = run("new")
    calls = []

    def looped(storages, next_values, normalise=True, reward_scaler=None, explained_variance=None):
        assert reward_scaler is None and not any(s._tl_used for s in storages)
        calls.append(len(storages))
        advs = [s.compute_returns(v, normalise=normalise) for s, v in zip(storages, next_values)]
        if explained_variance is not None:
            RolloutStorage.explained_variance(storages, explained_variance)
        return advs
    monkeypatch.setattr(RolloutStorage, "finish_rollouts", staticmethod(looped))
    old = run("old")
    assert calls == [2 * N] * EP
    assert torch.equal(bits(new), bits(old))


def test_train_vec_with_reward_scaling_and_time_limits(tmp_path):
    """3 episodes with reward_scaling=True and time-limit steps: finite losses, count = 3 N T per head, the scales equal
    the float64 reference on the recorded raw rewards (rounded to float32 once; one float32 ulp allowed: the device and
    numpy may round float64 values 1e-13 apart to different float32 neighbours), and a second run gives the same bits."""
    from ppo_agent.train import train_vec
    N, T, EP = 4, 8, 3

    def run(sub):
        (tmp_path / sub).mkdir()
        train_cfg, agent_cfg, env_cfg, rollout_cfg = _vec_cfgs(tmp_path / sub, N, T, EP)
        train_cfg.update(reward_scaling=True, log_stats=True)
        rec = dict(rollout=[], losses=[], scalers=set())

        def cb(event, agent, envs, rollouts, reward_scaler, **kw):
            rec["scalers"].add(id(reward_scaler))
            assert reward_scaler is agent.reward_scaler
            if event == "rollout":
                rec["rollout"].append([host(s) for p in rollouts for s in p])
            elif event == "update":
                rec["losses"].append(kw["losses"])
        lines = []

        class Log(object):
            def log(self, msg):
                lines.append(msg)
        agent = train_vec(0, train_cfg, agent_cfg, env_cfg, rollout_cfg, N, env_cls=_env_cls(), callback=cb, logger=Log())
        return agent, rec, lines
    agent, rec, lines = run("a")
    assert np.isfinite(np.array(rec["losses"], dtype=np.float64)).all()
    assert len(rec["scalers"]) == 1 and len(rec["rollout"]) == EP
    rs = agent.reward_scaler
    assert rs.count().tolist() == [EP * N * T] * 2
    assert sum(h["time_limits"].sum() for ro in rec["rollout"] for h in ro) > 0
    assert not any(h["time_limits"].any() for ro in rec["rollout"] for h in ro[6:8])      # environment 3: no key, no flag
    carry = [(0.0, 0.0)] * (2 * N)
    seen = [[], []]
    for ro in rec["rollout"]:
        for k, h in enumerate(ro):
            G, carry[k] = np_disc_returns(h["rewards"][:T], h["masks"][:T], h["time_limits"][:T], carry[k])
            seen[k & 1] += G
    got = rs.scale().cpu().numpy()
    for hd in (0, 1):
        x = np.array(seen[hd], dtype=np.float64)
        want = f32(1.0 / np.sqrt(((x - x.mean()) ** 2).sum() / len(x) + 1e-8))
        assert abs(float(got[hd]) - float(want)) <= float(np.spacing(want)), (hd, got[hd], want)
    assert sum("reward scale: " in ln for ln in lines) == EP
    agent2, rec2, _ = run("b")
    assert torch.equal(bits(agent.arena.params), bits(agent2.arena.params))
    assert torch.equal(rs.state.view(torch.int64), agent2.reward_scaler.state.view(torch.int64))


def test_train_single_env_with_reward_scaling_and_time_limits(tmp_path):
    """train() (one environment, learner_section): the scaler and the flags go through finish_rollouts with n = 2."""
    from ppo_agent.train import train
    from tests.helpers import topology_cfgs
    train_cfg, agent_cfg, env_cfg, rollout_cfg = topology_cfgs(str(tmp_path), H=84, W=84, T=8, episodes=2)
    train_cfg.update(reward_scaling={"clip": 5.0}, log_stats=True)
    lines = []

    class Log(object):
        def log(self, msg):
            lines.append(msg)
    train(0, train_cfg, agent_cfg, env_cfg, rollout_cfg, env_cls=_env_cls(), logger=Log())
    loss_lines = [ln for ln in lines if "value loss" in ln]
    scale_lines = [ln for ln in lines if "reward scale: " in ln]
    assert len(loss_lines) == len(scale_lines) == 2
    assert not any("nan" in ln or "inf" in ln for ln in loss_lines + scale_lines), lines
    scales = [float(x) for x in scale_lines[-1].rsplit("reward scale: ", 1)[1].split("/")]
    assert all(0.0 < x < 1e4 and x != 1.0 for x in scales), scales
