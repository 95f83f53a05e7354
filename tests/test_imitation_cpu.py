"""CPU: the behaviour-cloning warm start without a device — exports and rejection paths of cadre_bc_loss / cadre_demo_rows,
the float64 references of tests/imitation_ref.py against closed forms, and the host logic of cadre_amd.imitation
(controls_to_bins, balance weights, Monte-Carlo returns' masks, the split by episode, train_cfg["pretrain"])."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import imitation_ref, ordinal_ref
from tests.helpers import topology_cfgs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------- C ABI
def test_entry_points_are_exported_and_bound():
    from cadre_amd import hip
    L = ctypes.CDLL(hip.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "cadre_hip.h")).read()
    for name in ("cadre_bc_loss", "cadre_demo_rows"):
        assert hasattr(L, name) and name in hip.SYMBOLS and re.search(r"\bint %s\s*\(" % name, hdr), name
    assert len(hip.SYMBOLS["cadre_bc_loss"]) == 29 and len(hip.SYMBOLS["cadre_demo_rows"]) == 10
    assert hip.lib().cadre_abi_version() == hip.ABI_VERSION == 15          # entry points are only added
    assert hip.BC_STATS_FIELDS == 6 and "#define CADRE_BC_STATS_FIELDS 6" in hdr
    src = open(os.path.join(ROOT, "cadre_amd", "build.py")).read()
    assert '"imitation.hip"' in src


def bc_args(**kw):
    """A well-formed argument list of cadre_bc_loss (fake non-NULL pointers: nothing is launched on a rejection)."""
    a = dict(logits=16, ldl=64, l_ns=64, values=16, ldv=1, v_ns=1, actions=16, commands=16, returns=16, weights=None, B=1, C=4,
             nS=33, nT=3, eps=0.0, bc=1.0, vc=0.1, ec=0.01, inv_b=1.0, losses=16, dl=16, dv=16, scratch=16, poison=None,
             stats=None, F=0, sscr=None, ord=None, stream=None)
    a.update(kw)
    return tuple(a.values())


@pytest.mark.parametrize("bad,msg", [
    (dict(B=0), b"bad argument"), (dict(C=0), b"bad argument"), (dict(nS=0), b"bad argument"), (dict(nS=65), b"bad argument"),
    (dict(nT=0), b"bad argument"), (dict(nT=65), b"bad argument"), (dict(ldl=32), b"bad argument"), (dict(ldl=2), b"bad argument"),
    (dict(ldl=128), b"bad argument"), (dict(logits=None), b"bad argument"), (dict(values=None), b"bad argument"),
    (dict(actions=None), b"bad argument"), (dict(commands=None), b"bad argument"), (dict(returns=None), b"bad argument"),
    (dict(losses=None), b"bad argument"), (dict(scratch=None), b"bad argument"),
    (dict(eps=1.0), b"label_smoothing"), (dict(eps=-0.01), b"label_smoothing"), (dict(eps=float("nan")), b"label_smoothing"),
    (dict(dl=None), b"go together"), (dict(dv=None), b"go together"),
    (dict(stats=16, F=5, sscr=16), b"stats"), (dict(stats=16, F=6, sscr=None), b"stats"),
])
def test_bc_loss_rejections_launch_nothing(bad, msg):
    from cadre_amd import hip
    L = hip.lib()
    assert L.cadre_bc_loss(*bc_args(**bad)) == -1
    err = L.cadre_last_error()
    assert b"cadre_bc_loss" in err and msg in err, err


def test_demo_rows_rejections_launch_nothing():
    from cadre_amd import hip
    L = hip.lib()
    good = dict(latent=16, ld_lat=512, n=12, window=16, meas=16, T=5, S=8, obs=16, ldo=544, stream=None)
    for bad in (dict(latent=None), dict(window=None), dict(meas=None), dict(obs=None), dict(n=0), dict(T=0), dict(S=0),
                dict(T=1 << 30, S=8), dict(ld_lat=508), dict(ld_lat=514), dict(ldo=530), dict(ldo=546), dict(ldo=2048),
                dict(latent=20), dict(obs=24)):
        a = dict(good)
        a.update(bad)
        assert L.cadre_demo_rows(*a.values()) == -1 and b"cadre_demo_rows" in L.cadre_last_error(), bad


# ----------------------------------------------------------------------------- the float64 reference
def ref_case(B=9, C=3, K=(33, 3), seed=0):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(2 * C, B, 64, generator=g, dtype=torch.float64).requires_grad_(True)
    values = torch.randn(2 * C, B, generator=g, dtype=torch.float64).requires_grad_(True)
    actions = torch.stack([torch.randint(0, K[0], (B,), generator=g), torch.randint(0, K[1], (B,), generator=g)])
    cmds = torch.randint(0, C, (2, B), generator=g)
    rets = torch.randn(2, B, generator=g, dtype=torch.float64)
    return logits, values, actions, cmds, rets


def test_reference_gradient_is_inv_b_times_p_minus_onehot():
    B, C, K = 9, 3, (33, 3)
    logits, values, actions, cmds, rets = ref_case(B, C, K)
    inv_b = 1.0 / B
    tv, tb, te, total, stats = imitation_ref.bc_loss(logits, values, actions, cmds, rets, None, K, (None, None), C, 0.0, 1.0, 0.0,
                                                     0.0, inv_b)
    total.backward()
    assert float(tv.detach()) == 0.0 and float(te.detach()) == 0.0 and float(values.grad.abs().max()) == 0.0
    for hd in range(2):
        for b in range(B):
            for c in range(C):
                g = logits.grad[hd * C + c, b]
                if c != int(cmds[hd, b]):
                    assert float(g.abs().max()) == 0.0
                    continue
                p = torch.softmax(logits.detach()[hd * C + c, b, :K[hd]], -1)
                onehot = torch.zeros(K[hd], dtype=torch.float64)
                onehot[actions[hd, b]] = 1.0
                assert float((g[:K[hd]] - inv_b * (p - onehot)).abs().max()) < 1e-15
                assert float(g[K[hd]:].abs().max()) == 0.0
    assert torch.equal(stats[:, 5], torch.ones(2, dtype=torch.float64)) and torch.equal(stats[:, 4], stats[:, 5])


def test_reference_smoothed_target_sums_to_one():
    for K, eps in ((33, 0.1), (3, 0.5), (64, 0.0), (1, 0.9)):
        t = imitation_ref.smoothed_target(torch.arange(K) % K, K, eps)
        assert float((t.sum(-1) - 1.0).abs().max()) < 1e-15
        assert abs(float(t[0, 0]) - ((1.0 - eps) + eps / K)) < 1e-15


def test_reference_full_gradient_closed_form():
    """w inv_b (bc (p - t) + ec p (lg + H)) and vc w inv_b (v - R): the formulas the kernel implements, against autograd."""
    B, C, K = 7, 2, (5, 3)
    logits, values, actions, cmds, rets = ref_case(B, C, K, seed=3)
    w = torch.rand(2, B, dtype=torch.float64) * 3.75 + 0.25
    eps, bc, vc, ec, inv_b = 0.1, 0.7, 0.3, 0.05, 1.0 / B
    total = imitation_ref.bc_loss(logits, values, actions, cmds, rets, w, K, (None, None), C, eps, bc, vc, ec, inv_b)[3]
    total.backward()
    for hd in range(2):
        for b in range(B):
            net = hd * C + int(cmds[hd, b])
            lg = torch.log_softmax(logits.detach()[net, b, :K[hd]], -1)
            p = lg.exp()
            H = -(p * lg).sum()
            t = imitation_ref.smoothed_target(actions[hd, b:b + 1], K[hd], eps)[0]
            want = w[hd, b] * inv_b * (bc * (p - t) + ec * p * (lg + H))
            assert float((logits.grad[net, b, :K[hd]] - want).abs().max()) < 1e-14
            assert abs(float(values.grad[net, b] - vc * w[hd, b] * inv_b * (values.detach()[net, b] - rets[hd, b]))) < 1e-14


def test_reference_ordinal_reduces_to_categorical_under_the_marker_and_skips_unlabelled_rows():
    B, C, K = 9, 3, (33, 3)
    logits, values, actions, cmds, rets = ref_case(B, C, K, seed=5)
    actions[0, 2], actions[1, 4], cmds[0, 6] = -1, 3, C
    args = (logits, values, actions, cmds, rets, None, K)
    cat = imitation_ref.bc_loss(*args, (None, None), C, 0.1, 1.0, 0.1, 0.01, 1.0 / B)
    rank = list(range(K[0]))
    mixed = imitation_ref.bc_loss(*args, (rank, None), C, 0.1, 1.0, 0.1, 0.01, 1.0 / B)
    assert float(cat[3].detach()) != float(mixed[3].detach())                          # the ordinal head is another distribution ...
    # ... and the marker (None) is exactly the categorical statement: normalised_logits(x, None) = log_softmax(x)
    x = logits.detach()[0, :, :K[0]]
    assert torch.equal(ordinal_ref.normalised_logits(x, None), x - x.logsumexp(-1, keepdim=True))
    assert abs(float(cat[4][0, 5]) - (B - 2) / B) < 1e-15 and abs(float(cat[4][1, 5]) - (B - 1) / B) < 1e-15
    cat[3].backward()
    assert float(logits.grad[:C, 2].abs().max()) == 0.0 and float(logits.grad[:C, 6].abs().max()) == 0.0
    assert float(logits.grad[C:, 4].abs().max()) == 0.0 and float(values.grad[C:, 4].abs().max()) == 0.0


# ----------------------------------------------------------------------------- host helpers
def test_controls_to_bins_on_the_shipped_shapes():
    from ppo_agent.imitation import controls_to_bins
    steer = {i: (i - 16) / 16.0 for i in range(33)}
    thr = {0: [0, 0], 1: [0, 1], 2: [0.6, 0]}
    s = [-1.0, -2.0, 0.0, 1.0, 3.0, 0.03, 0.04, 1 / 32, -1 / 32, 0.5 + 1 / 32]
    t = [0.0, 0.0, 0.6, 0.3, 0.29, 0.31, 0.9, 0.0, 0.0, 0.0]
    b = [0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.5, 0.49, 0.51]
    a_s, a_t = controls_to_bins(s, t, b, steer, thr)
    assert a_s.dtype == np.int64 and a_t.dtype == np.int64
    # exact midpoints (1/32 between bins 16 and 17, -1/32 between 15 and 16, 17/32 between 24 and 25) go to the lower index
    assert a_s.tolist() == [0, 0, 16, 32, 32, 16, 17, 16, 15, 24]
    # throttle 0.3 / brake 0 is the midpoint of bins 0 and 2; brake 0.5 the midpoint of bins 0 and 1: lower index
    assert a_t.tolist() == [0, 1, 2, 0, 0, 2, 2, 0, 0, 1]
    one = controls_to_bins(0.25, 0.6, 0.0, steer, thr)
    assert one[0].tolist() == [20] and one[1].tolist() == [2]
    with pytest.raises(ValueError):
        controls_to_bins([0.0, 1.0], [0.0], [0.0], steer, thr)


def test_balance_weights_flatten_the_command_histogram():
    from ppo_agent.imitation import balance_weights
    cmd = np.array([0, 0, 0, 0, 0, 1, 3, 3, 0, 1, 3, 3, 3], np.int32)      # command 2 never occurs
    w = balance_weights(cmd, "command")
    assert w.dtype == np.float32 and abs(float(w.astype(np.float64).sum()) - cmd.size) < 1e-5
    hist = [float(w[cmd == c].astype(np.float64).sum()) for c in (0, 1, 3)]
    assert max(hist) - min(hist) < 1e-5 and abs(hist[0] - cmd.size / 3.0) < 1e-5
    assert np.abs(w - imitation_ref.balance_weights(cmd)).max() < 1e-6
    assert balance_weights(cmd, None).tolist() == [1.0] * cmd.size
    with pytest.raises(ValueError):
        balance_weights(cmd, "action")


def test_monte_carlo_returns_of_two_episodes():
    """A two-episode record, a `done` in the middle of the first episode, the second truncated: the masks cut at `done`
    and at both episode ends, and the numpy loop over the whole set equals the loop per segment."""
    from ppo_agent.imitation import episode_masks
    r = np.random.RandomState(2)
    T1, T2 = 7, 5
    rew = r.rand(T1 + T2).astype(np.float32)
    done = np.zeros((T1 + T2, 2), np.uint8)
    done[3, 0] = 1                                                      # steer head only
    m = episode_masks(done, [T1, T1 + T2])
    assert m.dtype == np.float32 and m[:, 0].tolist() == [1, 1, 1, 0, 1, 1, 0, 1, 1, 1, 1, 0]
    assert m[:, 1].tolist() == [1, 1, 1, 1, 1, 1, 0, 1, 1, 1, 1, 0] and done[T1 + T2 - 1].tolist() == [0, 0]
    g = imitation_ref.mc_returns(rew, m[:, 0], 0.99)
    for lo, hi in ((0, 4), (4, 7), (7, 12)):                            # each segment on its own, in float64
        want, acc = np.zeros(hi - lo), 0.0
        for t in range(hi - 1, lo - 1, -1):
            acc = float(rew[t]) + 0.99 * acc
            want[t - lo] = acc
        assert np.abs(g[lo:hi] - want).max() < 1e-5
        assert g[hi - 1] == rew[hi - 1]                                 # nothing leaks across a cut
    from oracle import ppo_ref                                          # the project's strict scan with V = 0, tau = 1
    ret, _V = ppo_ref.gae_returns(np.append(rew, 0).astype(np.float32), np.zeros(T1 + T2 + 1, np.float32),
                                  np.append(m[:, 0], 0).astype(np.float32), 0.0, 0.99, 1.0)
    assert np.array_equal(ret[:-1], g)


def test_gae_chunks_cover_the_set():
    from ppo_agent import imitation
    for T in (2, 3, 2999, 3000, 3001, 6001, 7000):
        ch = imitation._gae_chunks(T)
        assert ch[-1][0] == 0 and ch[0][1] == T and all(2 <= hi - lo <= imitation.GAE_MAX_T for lo, hi in ch)
        assert all(ch[i][0] == ch[i + 1][1] for i in range(len(ch) - 1))
    with pytest.raises(ValueError):
        imitation._gae_chunks(1)


def cpu_demo(lengths, seed=0):
    """A DemoSet on the CPU (split / subsets are plain torch): row t of the set holds t in every field."""
    from ppo_agent.imitation import DemoSet, balance_weights
    T = sum(lengths)
    steer, throttle = DemoSet._storages(T, 530, 8, 530, 0.99, "cpu")
    ids = torch.arange(T, dtype=torch.float32)
    steer._obs[:T] = ids.view(T, 1, 1)
    cmd = np.random.RandomState(seed).randint(0, 4, T)
    for s in (steer, throttle):
        s.returns[:T, 0] = ids
        s.action[:T, 0] = torch.arange(T)
        s.command[:T, 0] = torch.from_numpy(cmd.astype(np.int32))
    bounds, t0 = [], 0
    for n in lengths:
        bounds.append((t0, t0 + n))
        t0 += n
    w = torch.from_numpy(balance_weights(cmd, "command")).view(T, 1)
    return DemoSet(steer, throttle, w, bounds, cmd, 0.99, "command", 1.0)


def test_split_never_puts_an_episode_on_both_sides():
    from ppo_agent.imitation import split_episodes
    lengths = [5, 3, 9, 2, 7, 4]
    demo = cpu_demo(lengths)
    assert demo.throttle._obs is demo.steer._obs                        # one copy of the window rows
    for seed in range(6):
        for frac in (0.01, 0.34, 0.5, 0.99):
            tr, va = split_episodes(len(lengths), frac, seed)
            assert tr and va and not set(tr) & set(va) and sorted(tr + va) == list(range(len(lengths)))
    train, val = demo.split(0.34, seed=1)
    ep_of = np.concatenate([[e] * n for e, n in enumerate(lengths)])
    rows_t = train.steer.returns[:train.T, 0].long().numpy()
    rows_v = val.steer.returns[:val.T, 0].long().numpy()
    assert train.T + val.T == demo.T and len(val.episodes) == 2
    assert not set(ep_of[rows_t]) & set(ep_of[rows_v])
    for sub, rows in ((train, rows_t), (val, rows_v)):
        assert sorted(rows.tolist()) == rows.tolist()
        assert torch.equal(sub.steer._obs[:sub.T, 3, 7], torch.from_numpy(rows).float())
        assert torch.equal(sub.throttle.action[:sub.T, 0], torch.from_numpy(rows))
        assert np.array_equal(sub.commands, demo.commands[rows])
        assert abs(float(sub.weights.double().sum()) - sub.T) < 1e-4      # balanced again per side
        assert [hi - lo for lo, hi in sub.episodes] == [n for e, n in enumerate(lengths) if e in set(ep_of[rows])]
    with pytest.raises(ValueError):
        cpu_demo([4]).split(0.5, 0)


# ----------------------------------------------------------------------------- train_cfg["pretrain"]
def test_pretrain_config_parsing():
    from ppo_agent.imitation import pretrain_config
    assert pretrain_config(None) is None
    cfg = pretrain_config(dict(episodes="/d", epochs=3, minibatch=32, lr=1e-3, label_smoothing=0.1, balance=None,
                               validation_fraction=0.2))
    assert (cfg["epochs"], cfg["minibatch"], cfg["lr"], cfg["label_smoothing"], cfg["balance"]) == (3, 32, 1e-3, 0.1, None)
    assert cfg["validation_fraction"] == 0.2 and cfg["return_scale"] == 1.0 and cfg["max_grad_norm"] is None
    assert pretrain_config(dict(episodes="/d"))["balance"] == "command"
    for bad in (dict(epochs=1), dict(episodes="/d", epoch=1), dict(episodes="/d", lr=0.0), dict(episodes="/d", minibatch=0),
                dict(episodes="/d", label_smoothing=1.0), dict(episodes="/d", balance="x"),
                dict(episodes="/d", validation_fraction=1.0), "dir"):
        with pytest.raises(ValueError):
            pretrain_config(bad)


class _Log(list):
    def __call__(self, *a):
        self.append(a)


def run_mocked_train(monkeypatch, tmp_path, vec, **extra):
    """train() / train_vec() with the device side replaced by recorders: the sequence of calls the loop makes."""
    import cadre_amd.imitation as imitation
    import cadre_amd.ppo_agent.models as models
    import cadre_amd.ppo_agent.train as train_mod
    calls = _Log()

    class Agent(object):
        def __init__(self, **kw):
            calls("agent")
            self.model_dict, self.reward_scaler = {}, None

        def act(self, obs):
            calls("act")
            return None, [torch.tensor(0), torch.tensor(0)], [0.0, 0.0], [0.0, 0.0], None

        def act_batch(self, obs):
            calls("act_batch", len(obs))
            return [(None, [torch.tensor(0), torch.tensor(0)]) for _ in obs]

        def convert_action(self, a):
            return [0.0, 0.0, 0.0]

        def save_snapshot(self, path):
            calls("snapshot")

    class Storage(object):
        def __init__(self, **kw):
            calls("storage")

        def to(self, dev):
            pass

        def insert(self, *a, **kw):
            calls("insert")

        @staticmethod
        def insert_batch(*a, **kw):
            calls("insert_batch")

    class Shared(object):
        def __init__(self, model_dict, device):
            calls("shared")

        @staticmethod
        def dist_world():
            return 0

    class Env(object):
        def __init__(self, cfg):
            self.work_dir = str(tmp_path)

        def reset(self):
            calls("reset")
            return dict(command=1, rgb=np.zeros(1), route_fig=np.zeros(1))

        def step(self, action):
            calls("step")
            return dict(command=1, rgb=np.zeros(1), route_fig=np.zeros(1)), [0.0, 0.0], False, {"action_done": [False, False]}

    def section(*a, **kw):
        calls("section")
        return [0.0], [0.0], [0.0]

    def pre(agent, cfg, gamma, max_grad_norm, shared, rank, logger):
        calls("pretrain", cfg["episodes"], gamma, max_grad_norm, rank)

    monkeypatch.setattr(train_mod, "CadreAgent", Agent)
    monkeypatch.setattr(train_mod, "RolloutStorage", Storage)
    monkeypatch.setattr(train_mod, "learner_section", section)
    monkeypatch.setattr(train_mod, "learner_section_multi", section)
    monkeypatch.setattr(models, "Shared_grad_buffers", Shared)
    monkeypatch.setattr(imitation, "pretrain_from_config", pre)
    if "resume_from" in extra:
        monkeypatch.setattr(train_mod._Checkpointer, "resume", lambda self, path: calls("resume") or 0)
    train_cfg, agent_cfg, env_cfg, rollout_cfg = topology_cfgs(str(tmp_path), T=2, episodes=1)
    train_cfg.update(extra)
    if vec:
        train_mod.train_vec(0, train_cfg, agent_cfg, env_cfg, rollout_cfg, 1, env_cls=Env, logger=None)
    else:
        train_mod.train(0, train_cfg, agent_cfg, env_cfg, rollout_cfg, env_cls=Env, logger=None)
    return list(calls)


@pytest.mark.parametrize("vec", [False, True])
def test_train_without_a_pretrain_key_makes_the_calls_it_made(monkeypatch, tmp_path, vec):
    base = run_mocked_train(monkeypatch, tmp_path, vec)
    assert ("pretrain",) not in [c[:1] for c in base] and base.count(("section",)) == 1
    assert run_mocked_train(monkeypatch, tmp_path, vec, pretrain=None) == base
    with_pre = run_mocked_train(monkeypatch, tmp_path, vec, pretrain=dict(episodes="/demos", epochs=2))
    i = with_pre.index(("pretrain", "/demos", 0.99, 250.0, 0))
    assert with_pre[:i] + with_pre[i + 1:] == base                      # one more call, nothing else moves ...
    assert with_pre[i + 1] == ("reset",) and ("shared",) in with_pre[:i]   # ... after the setup, before the first rollout
    resumed = run_mocked_train(monkeypatch, tmp_path, vec, pretrain=dict(episodes="/demos"), resume_from=str(tmp_path / "c.pt"))
    assert ("resume",) in resumed and not [c for c in resumed if c[0] == "pretrain"]    # a resumed run does not pretrain


def test_pretrain_key_is_refused_where_the_warm_start_would_be_lost():
    """A chief in another process, or shared nets in another arena than the agent's: the first update_model would overwrite
    the pretrained weights without a word, so the key raises before anything runs."""
    import cadre_amd.ppo_agent.train as train_mod
    from cadre_amd.hip import CadreHipError

    class Net(object):
        def __init__(self, arena):
            self._cadre_arena = arena

    class Agent(object):
        arena = object()
    agent = Agent()
    agent.model_dict = {"n": Net(agent.arena)}
    cfg = dict(pretrain=dict(episodes="/demos"), max_grad_norm=250.0)
    rc = type("RC", (), {"gamma": 0.99})()
    with pytest.raises(CadreHipError, match="in-process chief"):
        train_mod._pretrain(agent, cfg, rc, None, 0, None, None, None, traffic_light=object())
    with pytest.raises(CadreHipError, match="another parameter arena"):
        train_mod._pretrain(agent, cfg, rc, None, 0, None, None, {"n": Net(object())})
    assert train_mod._pretrain(agent, dict(pretrain=None), rc, None, 0, None, None, {"n": Net(object())}, object()) is None
    assert train_mod._pretrain(agent, cfg, rc, None, 0, None, "ckpt.pt", {"n": Net(object())}, object()) is None


def test_set_loss_refuses_a_bool_bc_coefficient():
    """The coefficient check is one for every loss mode: a bool is refused (it used to count as 1.0 here)."""
    from cadre_amd.learner import PPOLearnerHIP
    lrn = PPOLearnerHIP.__new__(PPOLearnerHIP)
    lrn._hp_on, lrn._bc, lrn.loss_mode = False, (0.0, 1.0), "ppo"
    with pytest.raises(ValueError, match="set_loss: bc_coeff=True"):
        lrn.set_loss("bc", bc_coeff=True)
    assert lrn._bc == (0.0, 1.0) and lrn.loss_mode == "ppo"
