"""GPU: PPO update diagnostics (cadre_ppo_loss_stats, cadre_grad_norms, cadre_explained_variance) and the target_kl early
stop (cadre_clip_adam_graph_gated) against the float64 oracle and against the ungated learner."""
import math
import re

import numpy as np
import pytest
import torch

from cadre_amd import synth
from tests.helpers import fill_storages
from tests.test_learner_gpu import make_agent

pytestmark = pytest.mark.gpu
CLIP = 0.1


def storages(T, mbn, seed, C=4):
    from ppo_agent.storage import RolloutStorage
    data = fill_storages(T, seed)
    pair = []
    for hd in ("steer", "throttle"):
        s = RolloutStorage(T, mbn, 530, 8, 530, True, 0.99, 0.95)
        for k, v in data[hd].items():
            getattr(s, k).copy_(torch.from_numpy(v % C if k == "command" else v))
        s.to("cuda:0")
        pair.append(s)
    return pair


def cfg(**kw):
    d = dict(use_adv_norm=True, ppo_epoch=4, max_grad_norm=250.0, lr=3e-4)
    d.update(kw)
    return d


def arena_params_f64(arena):
    return {n: {k: v.detach().double().cpu() for k, v in arena.views(arena.params, n).items()} for n in arena.model_names()}


def samples(B, C, seed, skip_cmd=None):
    r = np.random.RandomState(seed)
    cmds = [c for c in range(C) if c != skip_cmd]
    out = []
    for K in (33, 3):
        out.append((torch.from_numpy((r.standard_normal((8 * B, 530)) * 0.5).astype(np.float32)),
                    torch.from_numpy(r.randint(0, K, (B, 1)).astype(np.int64)),
                    torch.from_numpy((0.3 * r.standard_normal((B, 1))).astype(np.float32)),
                    torch.from_numpy(r.standard_normal((B, 1)).astype(np.float32)),
                    torch.ones(B, 1),
                    torch.from_numpy((-np.log(K) + 0.2 * r.standard_normal((B, 1))).astype(np.float32)),
                    torch.from_numpy(r.standard_normal((B, 1)).astype(np.float32)),
                    [torch.from_numpy((0.1 * r.standard_normal((B, 530))).astype(np.float32)),
                     torch.from_numpy((0.1 * r.standard_normal((B, 530))).astype(np.float32))],
                    torch.from_numpy(np.array(cmds)[r.randint(0, len(cmds), (B, 1))].astype(np.int32))))
    return out


def dev(tup):
    return tuple(x.cuda() if not isinstance(x, list) else [y.cuda() for y in x] for x in tup)


def oracle_head(params, head, smp, C):
    """float64 per-row log-probs and values of the oracle's nets (agent.py:170-182), picked by command."""
    from oracle import ppo_ref
    obs, act, old_v, ret, _m, old_lp, adv, hidden, cmd = smp
    obs = obs.double(); hidden = [hidden[0].double(), hidden[1].double()]
    lp = v = 0
    for c in range(C):
        x, _ = ppo_ref.lstm_forward(obs.clone(), hidden, params["%s_lstm_%d" % (head, c)])
        vc, lpc, _e = ppo_ref.evaluate_actions(x, act, params["%s_ppo_%d" % (head, c)])
        m = (cmd == c)
        lp, v = lp + lpc * m, v + vc * m
    return lp[:, 0], v[:, 0], old_lp.double()[:, 0], old_v.double()[:, 0]


@pytest.mark.parametrize("B,C,skip", [(64, 4, None), (256, 4, None), (64, 1, None), (256, 1, None), (40, 4, None),
                                      (64, 4, 2)])
def test_stats_match_oracle(B, C, skip):
    """approx_kl / old_approx_kl within 1e-6 of the float64 recomputation; clip fractions exact away from the clip edge.
    One optimiser step first (r != 1); B = 40 is a ragged (unsorted) minibatch; skip: a command net without rows."""
    from ppo_agent.chief import chief_step
    from ppo_agent.models import Shared_grad_buffers
    agent = make_agent(84, 84, command_num=C)
    shared = Shared_grad_buffers(agent.model_dict, agent.device)
    s0 = samples(B, C, 1, skip)
    agent.update_policy(dev(s0[0]), dev(s0[1]))
    shared.add_gradient(agent.model_dict)
    chief_step(shared, None, 250.0, zero_grads=False)
    s1 = samples(B, C, 2, skip)
    lrn = agent.learner
    lrn.set_update_modes(stats=True)
    row = torch.zeros(2, lrn.stats_fields(), device="cuda:0")
    agent.update_policy(dev(s1[0]), dev(s1[1]), stats_row=row)
    lrn.set_update_modes()
    got = row.cpu().double()
    params = arena_params_f64(agent.arena)
    for h, head in enumerate(("steer", "throttle")):
        lp, v, olp, ov = oracle_head(params, head, s1[h], C)
        lr = lp - olp
        r = lr.exp()
        assert abs(float(((r - 1) - lr).mean()) - float(got[h, 0])) < 1e-6, (head, float(got[h, 0]))
        assert abs(float((-lr).mean()) - float(got[h, 1])) < 1e-6, head
        assert abs(float(r.mean()) - float(got[h, 4])) < 1e-5, head
        assert abs(float(lr.abs().max()) - float(got[h, 5])) < 1e-5, head
        assert got[h, 6] == 1.0
        for k, dist in ((2, (r - 1).abs()), (3, (v - ov).abs())):
            n_kernel = int(round(float(got[h, k]) * B))
            lo, hi = int((dist > CLIP + 1e-5).sum()), int((dist > CLIP - 1e-5).sum())
            assert lo <= n_kernel <= hi, (head, k, lo, n_kernel, hi)
        assert 0 < float(got[h, 2]) < 1, "the case should exercise the clip (r spread by the synthetic old log-probs)"


@pytest.mark.parametrize("graphs", [False, True])
def test_stats_change_nothing(graphs):
    """Losses, every gradient and the parameters after chief_step: stats on == stats off, bit for bit (eager and replay)."""
    from ppo_agent.chief import chief_step
    from ppo_agent.models import Shared_grad_buffers
    runs = []
    for on in (False, True):
        agent = make_agent(84, 84)
        agent.learner.use_graphs = graphs
        shared = Shared_grad_buffers(agent.model_dict, agent.device)
        pair = storages(64, 1, 5)
        for s in pair:
            s.compute_returns(torch.tensor([0.2]))
        if on:
            agent.learner.set_update_modes(stats=True)
        g = torch.Generator().manual_seed(3)
        rec = []
        for step in range(3):                          # eager, eager + capture, replay
            i_s, i_t = torch.randperm(64, generator=g), torch.randperm(64, generator=g)
            row = torch.zeros(2, agent.learner.stats_fields(), device="cuda:0") if on else None
            l = agent.update_policy_from_storages([(pair[0], i_s, pair[0].advantages, pair[1], i_t, pair[1].advantages)],
                                                  stats_row=row)
            grads = agent.arena.grads.clone()
            shared.add_gradient(agent.model_dict)
            chief_step(shared, None, 250.0, zero_grads=False)
            rec.append((l, grads, agent.arena.params.clone()))
        agent.learner.set_update_modes()
        runs.append(rec)
    for (la, ga, pa), (lb, gb, pb) in zip(*runs):
        assert la == lb and torch.equal(ga, gb) and torch.equal(pa, pb)


def _section(target_kl=None, stats=None, seed=9, C=4):
    from ppo_agent.models import Shared_grad_buffers
    from ppo_agent.train import learner_section
    agent = make_agent(84, 84, command_num=C)
    shared = Shared_grad_buffers(agent.model_dict, agent.device)
    pair = storages(64, 2, 21, C)
    torch.manual_seed(seed)
    losses = learner_section(agent, pair[0], pair[1], False, cfg(target_kl=target_kl), shared, stats=stats)
    torch.cuda.synchronize()
    return agent, losses, torch.get_rng_state()


def _state(agent):
    a = agent.arena
    return [a.params.clone(), a.exp_avg.clone(), a.exp_avg_sq.clone(), a.step_dev.clone()]


def test_gate_that_never_fires_is_bit_identical():
    a0, l0, rng0 = _section()
    st = {}
    a1, l1, rng1 = _section(target_kl=1e9, stats=st)
    for x, y in zip(_state(a0), _state(a1)):
        assert torch.equal(x, y)
    assert l0 == l1 and torch.equal(rng0, rng1)
    assert st["updates_applied"] == st["steps"] == 8 and st["stopped_at_step"] is None
    assert a1.arena.step == int(a1.arena.step_dev.item()) == 8


def test_gate_fires_at_step_k():
    from ppo_agent.chief import chief_step
    from ppo_agent.models import Shared_grad_buffers
    st0 = {}
    _section(stats=st0)
    kl = [max(r["approx_kl"]) for r in st0["rows"]]
    k = next((j for j in range(1, len(kl)) if kl[j] > max(kl[:j])), None)    # 0-based: the first skipped step
    assert k is not None, kl
    tkl = (max(kl[:k]) + kl[k]) / 2 / 1.5
    st = {}
    agent, losses, rng = _section(target_kl=tkl, stats=st)
    assert st["stopped_at_step"] == k and st["updates_applied"] == k and len(losses[0]) == 8
    assert [r["applied"] for r in st["rows"]] == [i < k for i in range(8)]
    _a0, _l0, rng_ungated = _section()
    assert torch.equal(rng, rng_ungated)
    # manual loop: the same draws, chief_step after the first k steps only
    ref = make_agent(84, 84)
    shared = Shared_grad_buffers(ref.model_dict, ref.device)
    pair = storages(64, 2, 21)
    torch.manual_seed(9)
    nv_s, nv_t = ref.get_value(False, pair[0].get_last(as_tensor=True), pair[1].get_last(as_tensor=True))
    adv = [pair[0].compute_returns(nv_s), pair[1].compute_returns(nv_t)]
    step = 0
    for _ in range(4):
        i_s, i_t = pair[0].sample_indices(), pair[1].sample_indices()
        for a, b in zip(i_s, i_t):
            ref.update_policy_from_storages([(pair[0], a, adv[0], pair[1], b, adv[1])], sync=False)
            if step < k:
                shared.add_gradient(ref.model_dict)
                chief_step(shared, None, 250.0, zero_grads=False)
            step += 1
    for x, y in zip(_state(agent), _state(ref)):
        assert torch.equal(x, y)
    assert agent.arena.step == ref.arena.step == k == int(agent.arena.step_dev.item())
    # one act() afterwards: the same weights are used
    td = synth.synth_rollout(1, 84, 84, seed=4)[0]
    outs = []
    for ag in (agent, ref):
        torch.manual_seed(1)
        obs = dict(rgb=td["rgb"], route_fig=td["route_fig"].copy(), measurements=td["measurements"], command=td["command"])
        outs.append(ag.act(obs))
    for x, y in zip(outs[0][1:4], outs[1][1:4]):
        for u, w in zip(x, y):
            assert torch.equal(torch.as_tensor(u).cpu(), torch.as_tensor(w).cpu())


def test_explained_variance():
    from ppo_agent.storage import RolloutStorage
    pairs = [storages(32, 2, 40 + w) for w in range(3)]
    flat = [s for p in pairs for s in p]
    single = torch.zeros(len(flat), dtype=torch.float64, device="cuda:0")
    for i, s in enumerate(flat):
        s.compute_returns(torch.tensor([0.1 * i]), explained_variance=single[i:i + 1])
    batched = torch.zeros_like(single)
    RolloutStorage.explained_variance(flat, batched)
    assert torch.equal(single, batched)
    for i, s in enumerate(flat):
        R = s.returns[:32, 0].double().cpu().numpy(); V = s.value_preds[:32, 0].double().cpu().numpy()
        assert abs(float(single[i]) - (1 - np.var(R - V) / np.var(R))) < 1e-6
    s = flat[0]
    s.returns[:32].fill_(0.3)
    out = torch.zeros(1, dtype=torch.float64, device="cuda:0")
    RolloutStorage.explained_variance([s], out)
    assert math.isnan(float(out))


def test_grad_norms_are_pre_clip_model_norms():
    from ppo_agent.chief import chief_step
    from ppo_agent.models import Shared_grad_buffers
    agent = make_agent(84, 84)
    a = agent.arena
    shared = Shared_grad_buffers(agent.model_dict, agent.device)
    pair = storages(64, 1, 7)
    for s in pair:
        s.compute_returns(torch.tensor([0.0]))
    agent.learner.set_update_modes(stats=True)
    row = torch.zeros(2, agent.learner.stats_fields(), device="cuda:0")
    idx = torch.randperm(64)
    agent.update_policy_from_storages([(pair[0], idx, pair[0].advantages, pair[1], idx, pair[1].advantages)], stats_row=row)
    off = a.seg_off.cpu().tolist()
    want = [float(torch.linalg.vector_norm(a.grads[off[m]:off[m + 1]].double())) for m in range(2 * a.Z)]
    shared.add_gradient(agent.model_dict)
    chief_step(shared, None, 1.0, zero_grads=False)           # (clips: the row holds the norms before clipping)
    agent.learner.set_update_modes()
    got = row.cpu()
    C = a.C
    for m in range(2 * a.Z):
        g = float(got[(m % (2 * C)) // C, 8 + (m // (2 * C)) * C + m % C])
        assert abs(g - want[m]) <= 1e-6 * want[m], (m, g, want[m])


def test_train_vec_and_train_log_stats(tmp_path):
    """log_stats: one extra line per log interval with finite numbers; without it the log is the plain loss line."""
    from ppo_agent.train import train, train_vec
    from tests.helpers import SyntheticEnv
    from tests.test_act_batch_gpu import _vec_cfgs

    class Log:
        def __init__(self):
            self.lines = []

        def log(self, s):
            self.lines.append(s)
    for vec in (True, False):
        logs = []
        for log_stats in (False, True):
            train_cfg, agent_cfg, env_cfg, rollout_cfg = _vec_cfgs(tmp_path, 2, 8, 2)
            train_cfg["log_stats"] = log_stats
            lg = Log()
            torch.manual_seed(0)
            if vec:
                train_vec(0, train_cfg, agent_cfg, env_cfg, rollout_cfg, 2, env_cls=SyntheticEnv, logger=lg)
            else:
                train(0, train_cfg, agent_cfg, env_cfg, rollout_cfg, env_cls=SyntheticEnv, logger=lg)
            logs.append(lg.lines)
        _check_logs(*logs)


def _check_logs(plain, with_stats):
    assert all(l.startswith("Episode: ") and "value loss" in l for l in plain)
    assert [l for l in with_stats if "value loss" in l] == plain     # same numbers: diagnostics change nothing
    extra = [l for l in with_stats if "approx kl" in l]
    assert len(extra) == len(plain) > 0
    for l in extra:
        nums = [float(x) for x in re.findall(r"(?<![A-Za-z])(?:-?\d+(?:\.\d+)?(?:e[-+]?\d+)?|nan|inf)", l.split(",", 1)[1])]
        assert len(nums) == 9 and all(math.isfinite(x) for x in nums), l


def test_learner_section_multi_stats_and_gate():
    """learner_section_multi: explained variance of all 2N storages in one launch (= per-storage values), rows for every
    step, and a gate that never fires changes no bit."""
    from ppo_agent.models import Shared_grad_buffers
    from ppo_agent.storage import RolloutStorage
    from ppo_agent.train import learner_section_multi
    res = []
    for tkl in (None, 1e9):
        agent = make_agent(84, 84)
        shared = Shared_grad_buffers(agent.model_dict, agent.device)
        rollouts = [storages(32, 2, 60 + w) for w in range(3)]
        torch.manual_seed(2)
        st = {}
        l = learner_section_multi(agent, rollouts, [False, True, False], cfg(ppo_epoch=2, target_kl=tkl), shared, stats=st)
        res.append((l, agent.arena.params.clone(), st))
        ev = torch.zeros(6, dtype=torch.float64, device="cuda:0")
        RolloutStorage.explained_variance([s for p in rollouts for s in p], ev)
        assert [tuple(x) for x in ev.view(3, 2).tolist()] == st["explained_variance"]
        assert st["steps"] == len(st["rows"]) == 4 and st["updates_applied"] == 4
    assert res[0][0] == res[1][0] and torch.equal(res[0][1], res[1][1])
