"""CPU: the host side of the vectorised ensemble evaluation (ppo_agent/evaluate.py) — the float64 reference of the control
average against CadreAgent.avg_action, the group split and the stacked-arena indexing, EpisodeSchedule, evaluate_vec with
scripted environments and a scripted evaluator, the argument checks of the two C-ABI entry points (before any launch) and
EnsembleEvaluator's refusals.  No kernel is launched."""
import os
import re

import numpy as np
import pytest
import torch

from tests import ensemble_ref

STEER = {i: (i - 16) / 3.0 for i in range(33)}                  # non-dyadic entries: i / 3
THROTTLE = {0: [0, 0], 1: [0, 1], 2: [0.6, 0]}


def _stub(steer=STEER, throttle=THROTTLE):
    from ppo_agent.agent import CadreAgent
    ag = CadreAgent.__new__(CadreAgent)
    ag.STEER_CONTROL, ag.THROTTLE_CONTROL = steer, throttle
    return ag


def _avg(ag, rows):
    return ag.avg_action([[torch.tensor(int(a0)), torch.tensor(int(a1))] for a0, a1 in rows])


def test_reference_controls_equal_avg_action_bit_for_bit():
    ag = _stub()
    st = [STEER[i] for i in range(33)]
    tt = [THROTTLE[i] for i in range(3)]
    r = np.random.RandomState(3)
    for M in range(1, 7):
        acts = np.stack([r.randint(0, 33, (40, M)), r.randint(0, 3, (40, M))], -1)
        got = ensemble_ref.controls(acts, st, tt)
        for e in range(40):
            want = _avg(ag, acts[e]) if M > 1 else ag.convert_action([torch.tensor(int(acts[e, 0, 0])), torch.tensor(int(acts[e, 0, 1]))])
            if M == 1:
                assert _avg(ag, acts[e]) == [float(v) for v in want]
            assert got[e].tolist() == [float(v) for v in want], (M, e)
    # the brake rule at its edges
    assert ensemble_ref.controls([[[5, 0], [5, 1]]], st, tt)[0, 2] == 0.5 == _avg(ag, [(5, 0), (5, 1)])[2]
    third = ensemble_ref.controls([[[5, 0], [5, 1], [5, 2]]], st, tt)[0]
    assert third[2] == 0.0 == _avg(ag, [(5, 0), (5, 1), (5, 2)])[2] and third[1] == _avg(ag, [(5, 0), (5, 1), (5, 2)])[1]
    assert ensemble_ref.controls([[[5, 1]]], st, tt)[0].tolist() == [STEER[5], 0.0, 1.0] == _avg(ag, [(5, 1)])
    # a bin outside its table: NaN in that environment only
    bad = ensemble_ref.controls([[[33, 0], [1, 1]], [[1, 0], [2, 1]], [[1, 3], [2, 1]], [[-1, 0], [2, 1]]], st, tt)
    assert np.isnan(bad[0]).all() and np.isnan(bad[2]).all() and np.isnan(bad[3]).all()
    assert bad[1].tolist() == _avg(ag, [(1, 0), (2, 1)])


def test_group_split():
    from ppo_agent.evaluate import group_split
    assert group_split(6, 4) == [4, 2]
    assert group_split(3, 6) == [2, 1]
    assert group_split(2, 16) == [1, 1]
    assert group_split(16, 1) == [16] and group_split(17, 1) == [16, 1] and group_split(5, 1) == [5]
    assert group_split(1, 4) == [1] and group_split(8, 4) == [4, 4]
    for M in range(1, 20):
        for C in range(1, 17):
            g = group_split(M, C)
            assert g == ensemble_ref.group_split(M, C) and sum(g) == M and all(1 <= n and n * C <= 16 for n in g)
    for M, C in ((0, 4), (3, 0), (3, 17)):
        with pytest.raises(ValueError):
            group_split(M, C)


def test_tiled_seg_and_net_index_against_brute_force():
    from ppo_agent.agent import command_rows
    from ppo_agent.evaluate import ens_net, tiled_seg
    r = np.random.RandomState(11)
    for C, Mg, N in ((4, 4, 9), (6, 2, 7), (2, 3, 5), (1, 16, 3), (16, 1, 20), (4, 1, 1)):
        cmds = r.randint(0, C, N)
        if C > 1:
            cmds[cmds == C - 1] = 0                              # an empty command
        cmds = cmds.tolist()
        pos, seg = command_rows(cmds, C)
        got = tiled_seg(seg, C, Mg)
        assert got.dtype == np.int32 and got.shape == (2 * Mg * C, 2) and got.flags["C_CONTIGUOUS"]
        assert np.array_equal(got, ensemble_ref.tiled_seg(cmds, C, Mg)), (C, Mg)
        for h in range(2):
            for j in range(Mg):
                for c in range(C):
                    g = ens_net(h, j, c, Mg, C)
                    assert g == ensemble_ref.net_index(h, j, c, Mg, C)
                    assert got[g].tolist() == seg[h * C + c].tolist()
                    # every environment of command c lies inside the run of every agent's net of that command
                    assert all(got[g][0] <= pos[e] < got[g][0] + got[g][1] for e in range(N) if cmds[e] == c)
        if C > 1:
            assert all(got[ens_net(h, j, C - 1, Mg, C)][1] == 0 for h in range(2) for j in range(Mg))


def _run_schedule(num_envs, episodes, lengths):
    """Drive a schedule with episode k lasting lengths[k] steps; returns (starts per env, finish order, active sizes)."""
    from ppo_agent.evaluate import EpisodeSchedule
    s = EpisodeSchedule(num_envs, episodes)
    left = {i: lengths[s.episode_of[i]] for i in s.active}
    starts = {i: 1 for i in s.active}
    order, sizes = [], []
    while s.active:
        sizes.append(len(s.active))
        assert s.started <= episodes and s.active == sorted(s.active)
        for i in list(s.active):
            left[i] -= 1
            if left[i] == 0:
                ep, again = s.finish(i)
                order.append(ep)
                if again:
                    left[i] = lengths[s.episode_of[i]]
                    starts[i] += 1
                else:
                    assert i not in s.active
    assert s.done() and s.started == s.finished == episodes
    return starts, order, sizes


def test_episode_schedule():
    from ppo_agent.evaluate import EpisodeSchedule
    starts, order, sizes = _run_schedule(3, 5, [4, 2, 3, 2, 5])
    assert sorted(order) == list(range(5)) and sum(starts.values()) == 5
    assert sizes[0] == 3 and sizes[-1] < 3                        # the active list shrinks
    starts, order, sizes = _run_schedule(4, 2, [3, 1])             # episodes < num_envs: two environments never start
    assert sorted(starts) == [0, 1] and sorted(order) == [0, 1] and max(sizes) == 2
    starts, order, _ = _run_schedule(3, 7, [1] * 7)                # not divisible
    assert sorted(order) == list(range(7)) and sorted(starts.values()) == [2, 2, 3]
    starts, order, _ = _run_schedule(1, 3, [2, 2, 2])
    assert order == [0, 1, 2] and starts == {0: 3}
    s = EpisodeSchedule(2, 0)
    assert s.active == [] and s.done()
    s = EpisodeSchedule(2, 2)
    s.finish(0)
    with pytest.raises(KeyError):
        s.finish(0)                                               # never a start beyond the budget, never a double finish
    assert s.started == 2
    for bad in ((0, 3), (2, -1)):
        with pytest.raises(ValueError):
            EpisodeSchedule(*bad)


class _Env(object):
    """Scripted environment: episode n of this environment lasts plan[n] steps; step t of it pays (t + 1, 0.25 * id)."""

    def __init__(self, ident, plan):
        self.id, self.plan, self.resets, self.t, self.controls = ident, list(plan), 0, 0, []

    def _obs(self):
        return dict(env=self.id, episode=self.resets - 1, t=self.t)

    def reset(self):
        self.resets += 1
        self.t = 0
        return self._obs()

    def step(self, control):
        self.controls.append(control)
        self.t += 1
        done = self.t == self.plan[self.resets - 1]
        return self._obs(), [float(self.t), 0.25 * self.id], done, dict(env=self.id, t=self.t)


class _Evaluator(object):
    """Scripted evaluator: records every call, answers with controls that name the environment."""

    def __init__(self):
        self.calls = []

    def act(self, obs_list, shifted=None, deterministic=False):
        from ppo_agent.evaluate import EnsembleActBatch
        self.calls.append(([dict(o) for o in obs_list], list(shifted), deterministic))
        out = EnsembleActBatch([None] * len(obs_list))
        out.controls = [[float(o["env"]), float(o["t"]), 0.0] for o in obs_list]
        return out


def test_evaluate_vec_with_scripted_environments():
    from ppo_agent.evaluate import evaluate_vec
    # episodes 0, 1, 2 start on environments 0, 1, 2; environment 1 finishes first and starts episode 3, environment 0
    # then starts episode 4; environment 1 finishes episode 3 with nothing left to start and leaves: 2 moves to position 1
    envs = [_Env(0, [3, 4]), _Env(1, [2, 2]), _Env(2, [8])]
    ev, seen = _Evaluator(), []
    recs = evaluate_vec(None, envs, 5, deterministic=True, callback=lambda event, **kw: seen.append((event, kw["record"]["episode"])),
                        evaluator=ev)
    assert [r["episode"] for r in recs] == [1, 0, 3, 4, 2]        # finishing order
    assert [r["env"] for r in recs] == [1, 0, 1, 0, 2]
    assert [r["length"] for r in recs] == [2, 3, 2, 4, 8]
    assert seen == [("episode", r["episode"]) for r in recs]
    for r in recs:
        n = r["length"]
        assert r["reward_sum"] == (n * (n + 1) / 2.0, 0.25 * r["env"] * n) and isinstance(r["reward_sum"][0], float)
        assert r["info"] == dict(env=r["env"], t=n)
    assert [e.resets for e in envs] == [2, 2, 1]
    assert all(det is True for _o, _h, det in ev.calls)
    # every environment was stepped with ITS controls, once per step of its episodes
    assert [len(e.controls) for e in envs] == [7, 4, 8]
    assert all(c[0] == float(e.id) for e in envs for c in e.controls)
    # hints: False for a reset environment and for one whose position moved, None (compare on the host) otherwise
    who = [[o["env"] for o in obs] for obs, _h, _d in ev.calls]
    hints = [h for _o, h, _d in ev.calls]
    assert who[0] == [0, 1, 2] and hints[0] == [False, False, False]
    assert hints[1] == [None, None, None]
    assert who[2] == [0, 1, 2] and hints[2] == [None, False, None]          # environment 1 was reset after 2 steps
    assert hints[3] == [False, None, None]                                   # environment 0 after 3
    assert who[4] == [0, 2] and hints[4] == [None, False]                    # environment 1 left: 2 moved to position 1
    assert hints[5] == [None, None]
    assert who[7] == [2] and hints[7] == [False]                             # environment 0 left: 2 moved to position 0
    assert len(ev.calls) == 8
    # fewer episodes than environments: the others are never reset or stepped
    envs = [_Env(0, [2]), _Env(1, [1]), _Env(2, [1])]
    recs = evaluate_vec(None, envs, 2, evaluator=_Evaluator())
    assert [(r["episode"], r["env"]) for r in recs] == [(1, 1), (0, 0)] and [e.resets for e in envs] == [1, 1, 0]
    assert evaluate_vec(None, [_Env(0, [1])], 0, evaluator=_Evaluator()) == []


def test_ensemble_entry_points_are_declared_exported_and_check_their_arguments():
    from cadre_amd import hip
    L = hip.lib()
    assert L.cadre_abi_version() == hip.ABI_VERSION == 15           # entry points are only added
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "cadre_hip.h")).read()
    for name in ("cadre_sample_rows_ens", "cadre_ensemble_controls"):
        assert name in hip.SYMBOLS and hasattr(L, name)
        assert re.search(r"\bint %s\(" % name, hdr), name
    P = 16                                          # (a non-null pointer value: never dereferenced, the checks come first)
    # (O3, ldo, z_str, pos, cmd, N, C, Mg, m0, M, q, K_steer, K_throttle, action, logp, value, ord, stream)
    ok = [P, 64, 64 * 5, P, P, 5, 4, 2, 1, 3, P, 33, 3, P, P, P, P, None]

    def sample(i, v):
        args = list(ok)
        args[i] = v
        return L.cadre_sample_rows_ens(*args)
    for i in (0, 3, 4, 13, 14, 15):
        assert sample(i, None) == -1 and b"cadre_sample_rows_ens: null operand" in L.cadre_last_error(), i
    for i, v in ((5, 0), (6, 0), (7, 0), (7, 5), (6, 9), (8, -1), (8, 2), (9, 2), (11, 0), (11, 65), (12, 0), (12, 65), (1, 32),
                 (2, 64 * 4)):
        assert sample(i, v) != 0 and b"cadre_sample_rows_ens: bad argument" in L.cadre_last_error(), (i, v)
    with pytest.raises(hip.CadreHipError, match="cadre_sample_rows_ens"):
        hip.check(sample(7, 5), "cadre_sample_rows_ens")
    # (action, N, M, steer_tab, K_steer, throttle_tab, K_throttle, controls, stream)
    ok_c = [P, 5, 3, P, 33, P, 3, P, None]

    def controls(i, v):
        args = list(ok_c)
        args[i] = v
        return L.cadre_ensemble_controls(*args)
    for i in (0, 3, 5, 7):
        assert controls(i, None) == -1 and b"cadre_ensemble_controls: null operand" in L.cadre_last_error(), i
    for i, v in ((1, 0), (2, 0), (4, 0), (6, 0), (1, -3)):
        assert controls(i, v) != 0 and b"cadre_ensemble_controls: bad argument" in L.cadre_last_error(), (i, v)


class _Arena(object):
    n_out = (33, 3)


class _Enc(object):
    def __init__(self, fp):
        self.fingerprint = fp


def _shell(**kw):
    ag = _stub(dict(STEER), dict(THROTTLE))
    ag.device = ag.vae_device = torch.device("cuda:0")
    ag.command_num, ag.lstm_input, ag.ordinal_rank, ag.arena, ag.vae_model = 4, 530, None, _Arena(), _Enc("a")
    for k, v in kw.items():
        setattr(ag, k, v)
    return ag


def test_evaluator_refuses_mixed_groups_before_any_device_work():
    from cadre_amd import hip
    from ppo_agent.evaluate import EnsembleEvaluator, check_group
    n_out, (st, tt) = check_group([_shell(), _shell(), _shell()])              # fine
    assert n_out == (33, 3) and st.dtype == tt.dtype == np.float64 and st.shape == (33,) and tt.shape == (3, 2)
    assert st[17] == 1.0 / 3.0 and tt[2].tolist() == [0.6, 0.0]
    arena5 = _Arena()
    arena5.n_out = (33, 5)
    steer2 = dict(STEER)
    steer2[4] = 0.125
    thr2 = dict(THROTTLE)
    thr2[2] = [0.7, 0]
    for field, kw in (("device", dict(device=torch.device("cuda:1"))), ("command_num", dict(command_num=6)),
                      ("num_output", dict(arena=arena5)), ("lstm_input", dict(lstm_input=274)),
                      ("ordinal_rank", dict(ordinal_rank=[list(range(33)), None])),
                      ("STEER_CONTROL", dict(STEER_CONTROL=steer2)), ("THROTTLE_CONTROL", dict(THROTTLE_CONTROL=thr2))):
        with pytest.raises((hip.CadreHipError, ValueError), match=field):
            EnsembleEvaluator([_shell(), _shell(), _shell(**kw)])
    with pytest.raises((hip.CadreHipError, ValueError), match="encoder"):
        EnsembleEvaluator([_shell(), _shell(vae_model=_Enc("b"))])
    with pytest.raises(ValueError, match="empty"):
        EnsembleEvaluator([])
    short = dict(STEER)
    del short[32]
    with pytest.raises(ValueError, match="STEER_CONTROL"):
        EnsembleEvaluator([_shell(STEER_CONTROL=short)])


def test_deterministic_is_an_argument_of_act_and_act_batch():
    import inspect
    from ppo_agent.agent import CadreAgent
    for fn in (CadreAgent.act, CadreAgent.act_batch, CadreAgent.act_from_feature, CadreAgent.ensemble_act_batch):
        p = inspect.signature(fn).parameters["deterministic"]
        assert p.default is False, fn
