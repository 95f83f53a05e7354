"""GPU: device-resident PPO hyper-parameters (the `_hp` entry points, PPOLearnerHIP.set_device_hyper / set_hyper /
set_adaptive_lr, train_cfg["schedules"] / ["adaptive_lr"]).  The reference for values is never the code under test: it is
the by-value path (driven step by step from the host) or the float64 oracle."""
import numpy as np
import pytest
import torch

from cadre_amd import synth
from tests.test_learner_gpu import LOSS_TOL, make_agent, per_model, rel
from tests.test_ppo_stats_gpu import _state, cfg, dev, samples, storages

pytestmark = pytest.mark.gpu
LR0 = 3e-4


def _shared(agent):
    from ppo_agent.models import Shared_grad_buffers
    return Shared_grad_buffers(agent.model_dict, agent.device)


def _full_state(agent):
    return _state(agent) + [agent.arena.grads.clone()]


# ----------------------------------------------------------------------------- 1. constant block == by-value
@pytest.mark.parametrize("pack", [False, True])
@pytest.mark.parametrize("mode", ["off", "stats", "gate"])
@pytest.mark.parametrize("graphs", [False, True])
def test_constant_block_equals_by_value(graphs, mode, pack):
    """A full learner section (4 epochs x 2 minibatches) with the block holding the construction values: losses, gradients,
    parameters, both Adam moments and step_dev equal the by-value section's, bit for bit (same instruction stream, the
    scalar merely comes from memory; (float)double is the rounding ctypes applies to the by-value arguments)."""
    from ppo_agent.train import learner_section
    res = []
    for hp in (False, True):
        agent = make_agent(84, 84)
        agent.learner.use_graphs = graphs
        agent.learner.fused_pack = pack
        if hp:
            agent.learner.set_device_hyper()
            assert agent.learner.device_hyper
        pair = storages(64, 2, 21)
        torch.manual_seed(9)
        st = {} if mode != "off" else None
        losses = learner_section(agent, pair[0], pair[1], False, cfg(target_kl=1e9 if mode == "gate" else None),
                                 _shared(agent), stats=st)
        torch.cuda.synchronize()
        res.append((losses, _full_state(agent), st, agent))
    (l0, s0, st0, a0), (l1, s1, st1, a1) = res
    assert l0 == l1
    for x, y in zip(s0, s1):
        assert torch.equal(x, y)
    assert int(a1.arena.step_dev.item()) == 8 == a1.arena.step
    if mode != "off":
        for r0, r1 in zip(st0["rows"], st1["rows"]):
            assert "lr" not in r0 and r1.pop("lr") == float(np.float32(LR0))
            assert r0 == r1
    if graphs:      # the device-hyper section ran its own graphs (mode ("hp",)), none keyed on lr / max_grad_norm
        keys = [k for k in a1.learner._graphs if k[0] != "warm"]
        assert keys and all((("hp",) in k) or k[:2] == ("adam", "hp") for k in keys), keys


def test_constant_block_equals_by_value_sharded():
    """The sharded pair with the shard [0, total): norms_hp / apply_hp against the by-value pair, three steps."""
    agents = [make_agent(84, 84), make_agent(84, 84)]
    agents[1].learner.set_device_hyper()
    s = samples(64, 4, 1)
    for step in range(3):
        for ag in agents:
            ag.update_policy(dev(s[0]), dev(s[1]))
            ag.learner.clip_adam_sharded(0, ag.arena.total, lambda t: None, lr=1e-3, max_grad_norm=0.5)
        for x, y in zip(_full_state(agents[0]), _full_state(agents[1])):
            assert torch.equal(x, y), step
    assert agents[1].learner.hyper("lr") == 1e-3 and agents[1].learner.hyper("max_grad_norm") == 0.5


# ----------------------------------------------------------------------------- 2. values move, graphs do not
def test_schedules_move_values_not_graphs():
    from ppo_agent.train import apply_schedules, learner_section, schedule_value
    E = 6
    sch = {"lr": ("linear", 3e-4, 3e-5), "clip": ("linear", 0.1, 0.02), "ent_coeff": ("linear", 0.01, 0.0)}
    a_hp, a_ref, a_leak = make_agent(84, 84), make_agent(84, 84), make_agent(84, 84)
    a_ref.learner.use_graphs = False
    sh = {id(a): _shared(a) for a in (a_hp, a_ref, a_leak)}
    pairs = {id(a): storages(64, 2, 21) for a in (a_hp, a_ref, a_leak)}
    n_hp, n_leak = [], []
    for e in range(E):
        v = {k: schedule_value(s, e, E) for k, s in sch.items()}
        # device-hyper agent: one set_hyper per episode, graphs replayed
        torch.manual_seed(100 + e)
        assert apply_schedules(a_hp, cfg(schedules=sch), e, E) == v
        st = {}
        l_hp = learner_section(a_hp, *pairs[id(a_hp)], False, cfg(schedules=sch), sh[id(a_hp)], stats=st)
        assert all(r["lr"] == float(np.float32(v["lr"])) for r in st["rows"])
        n_hp.append(len(a_hp.learner._graphs))
        # manual loop: the by-value path, eager, values set from the host
        torch.manual_seed(100 + e)
        a_ref.learner.clip, a_ref.learner.ec = v["clip"], v["ent_coeff"]
        l_ref = learner_section(a_ref, *pairs[id(a_ref)], False, cfg(lr=v["lr"]), sh[id(a_ref)])
        torch.cuda.synchronize()
        assert l_hp == l_ref, e
        assert torch.equal(a_hp.arena.params, a_ref.arena.params), e
        # today's path under graphs with the same lr list: one more optimiser graph per value
        torch.manual_seed(100 + e)
        learner_section(a_leak, *pairs[id(a_leak)], False, cfg(lr=v["lr"]), sh[id(a_leak)])
        n_leak.append(len(a_leak.learner._graphs))
    print("graphs kept per episode: device-hyper %s, by-value %s" % (n_hp, n_leak))
    assert n_hp[1:] == [n_hp[1]] * (E - 1), n_hp
    assert all(b > a for a, b in zip(n_leak[1:], n_leak[2:])), n_leak
    for x, y in zip(_state(a_hp), _state(a_ref)):
        assert torch.equal(x, y)


# ----------------------------------------------------------------------------- 3. the silent no-op is gone
def test_assigning_clip_after_capture_takes_effect():
    s = samples(64, 4, 1)
    d = (dev(s[0]), dev(s[1]))
    want = {}
    for c in (0.1, 0.02):
        ref = make_agent(84, 84)
        ref.learner.use_graphs = False
        ref.learner.clip = c
        want[c] = (ref.update_policy(*d), ref.arena.grads.clone())
    assert want[0.1][0] != want[0.02][0]                    # (the inputs exercise the clip)
    agent = make_agent(84, 84)
    assert agent.learner.use_graphs and not agent.learner.device_hyper
    for _ in range(3):                                      # eager, eager + capture, replay
        got = agent.update_policy(*d)
    captured = [k for k in agent.learner._graphs if k[0] == "all"]
    assert captured and got == want[0.1][0]
    agent.learner.clip = 0.1                                # the same value: the graph stays
    assert [k for k in agent.learner._graphs if k[0] == "all"] == captured
    agent.learner.clip = 0.02
    got = agent.update_policy(*d)
    assert got == want[0.02][0] and got != want[0.1][0]
    assert torch.equal(agent.arena.grads, want[0.02][1])
    for _ in range(2):                                      # captured again with the new value, and replayed
        assert agent.update_policy(*d) == want[0.02][0]
    assert [k for k in agent.learner._graphs if k[0] == "all"]


# ----------------------------------------------------------------------------- 4. oracle
def test_device_hyper_step_matches_oracle():
    """One device-hyper step at clip 0.03, ent_coeff 0.002, lr 1e-4 against the oracle at the same values:
    losses LOSS_TOL, per-parameter gradients 2e-4 of the model's max |g|, parameter sums 1e-5 (tests/test_learner_gpu.py)."""
    from oracle import ppo_ref
    B, C = 64, 4
    agent = make_agent(84, 84, command_num=C)
    params = ppo_ref.to_torch_params(synth.ppo_state(11, command_num=C), requires_grad=True)
    s = samples(B, C, 5)
    lrn = agent.learner
    lrn.set_device_hyper()
    lrn.set_hyper(clip=0.03, ent_coeff=0.002)
    assert (lrn.clip, lrn.ec) == (0.03, 0.002)
    want = ppo_ref.update_policy(params, s[0], s[1], ent_coeff=0.002, clip=0.03, command_num=C)
    got = agent.update_policy(dev(s[0]), dev(s[1]))
    print("losses: got %r want %r" % (got, want))
    assert rel(got, want) < LOSS_TOL
    default = ppo_ref.update_policy(ppo_ref.to_torch_params(synth.ppo_state(11, command_num=C), requires_grad=True), s[0], s[1],
                                    command_num=C)
    assert rel(default, want) > 10 * LOSS_TOL                # (the values matter on these inputs)
    worst = 0.0
    for mn, d in params.items():
        gv = agent.arena.views(agent.arena.grads, mn)
        scale = max(float(p.grad.abs().max()) for p in d.values())
        for k, p in d.items():
            err = float((gv[k].cpu() - p.grad).abs().max()) / max(scale, 1e-12)
            worst = max(worst, err)
            assert err < 2e-4, (mn, k, err)
    print("worst per-parameter gradient error (rel. to model max |g|): %.2e" % worst)
    names = agent.arena.model_names()
    adam = {m: {k: (torch.zeros_like(p), torch.zeros_like(p)) for k, p in d.items()} for m, d in params.items()}
    grads = {m: {k: p.grad for k, p in d.items()} for m, d in params.items()}
    before = [float(sum(p.data.double().sum() for p in params[n].values())) for n in names]
    ppo_ref.chief_step(params, grads, adam, 1, lr=1e-4)
    lrn.clip_adam(lr=1e-4, max_grad_norm=250.0)
    assert lrn.hyper("lr") == 1e-4
    want_ps = [float(sum(p.data.double().sum() for p in params[n].values())) for n in names]
    got_ps = per_model(agent.arena, agent.arena.params, names, lambda ts: float(sum(t.sum() for t in ts)))
    assert rel(got_ps, want_ps) < 1e-5
    # the step itself (the change of the sums) is lr-sized: within 1e-3 of the oracle's change
    d_want, d_got = np.array(want_ps) - np.array(before), np.array(got_ps) - np.array(before)
    print("parameter-sum change, got/want:", d_got / d_want)


# ----------------------------------------------------------------------------- 5. adaptive lr follows the rule exactly
def host_rule(lr, kl_pair, desired, factor, lr_min, lr_max):
    """The controller in float64 on the host, from the float32 approx_kl pair a step reported."""
    kl = max(float(kl_pair[0]), float(kl_pair[1]))
    if kl > 2.0 * desired:
        return max(lr_min, lr / factor), -1
    if 0.0 < kl < desired / 2.0:
        return min(lr_max, lr * factor), +1
    return lr, 0


def _adaptive_run(adaptive, sections=2, target_kl=None, lr0=LR0, seed=9):
    """`sections` learner sections (4 epochs x 2 minibatches each) on one agent; adaptive = None (constant lr0) or
    (desired, factor, lr_min, lr_max).  Returns (agent, rows of all sections)."""
    from ppo_agent.train import learner_section
    agent = make_agent(84, 84)
    shared = _shared(agent)
    pair = storages(64, 2, 21)
    if adaptive is not None:
        d, f, lo, hi = adaptive
        agent.learner.set_adaptive_lr(d, factor=f, lr_min=lo, lr_max=hi, lr=lr0)
    else:
        agent.learner.set_device_hyper()
    rows = []
    for sec in range(sections):
        torch.manual_seed(seed + sec)
        st = {}
        learner_section(agent, pair[0], pair[1], False, cfg(target_kl=target_kl, lr=lr0), shared, stats=st)
        rows += st["rows"]
    torch.cuda.synchronize()
    return agent, rows


def _manual_run(lrs, sections=2, applied=None, seed=9):
    """The by-value path, eager, one chief_step per minibatch with the host's lr list (applied[i] False: no step)."""
    from ppo_agent.chief import chief_step
    ref = make_agent(84, 84)
    ref.learner.use_graphs = False
    shared = _shared(ref)
    pair = storages(64, 2, 21)
    step = 0
    for sec in range(sections):
        torch.manual_seed(seed + sec)
        nv_s, nv_t = ref.get_value(False, pair[0].get_last(as_tensor=True), pair[1].get_last(as_tensor=True))
        adv = [pair[0].compute_returns(nv_s), pair[1].compute_returns(nv_t)]
        for _ in range(4):
            i_s, i_t = pair[0].sample_indices(), pair[1].sample_indices()
            for a, b in zip(i_s, i_t):
                ref.update_policy_from_storages([(pair[0], a, adv[0], pair[1], b, adv[1])], sync=False)
                if applied is None or applied[step]:
                    shared.add_gradient(ref.model_dict)
                    chief_step(shared, None, 250.0, lr=lrs[step], zero_grads=False)
                step += 1
    torch.cuda.synchronize()
    return ref


def _check_rule(rows, adaptive, lr0=LR0):
    lr, lrs, moves = lr0, [], []
    for i, r in enumerate(rows):
        if r["applied"]:
            lr, mv = host_rule(lr, r["approx_kl"], *adaptive)
        else:
            mv = 0
        lrs.append(lr)
        moves.append(mv)
        assert float(np.float32(lr)) == r["lr"], (i, lr, r["lr"], r["approx_kl"])
    return lrs, moves


def test_adaptive_lr_lowers_to_the_floor():
    ad = (1e-9, 1.5, 1e-4, 1e-2)
    agent, rows = _adaptive_run(ad)
    lrs, moves = _check_rule(rows, ad)
    print("kl:", [max(r["approx_kl"]) for r in rows], "lr:", lrs)
    assert moves == [-1] * 16 and lrs[:2] == [LR0 / 1.5, LR0 / 1.5 / 1.5] and lrs[2:] == [1e-4] * 14
    ref = _manual_run(lrs)
    for x, y in zip(_state(agent), _state(ref)):
        assert torch.equal(x, y)


def test_adaptive_lr_raises_to_the_cap():
    ad = (1e3, 1.5, 1e-5, 1e-3)
    agent, rows = _adaptive_run(ad)
    lrs, moves = _check_rule(rows, ad)
    print("kl:", [max(r["approx_kl"]) for r in rows], "lr:", lrs)
    assert moves == [+1] * 16 and lrs[:2] == [LR0 * 1.5, LR0 * 1.5 * 1.5] and lrs[2:] == [1e-3] * 14
    ref = _manual_run(lrs)
    for x, y in zip(_state(agent), _state(ref)):
        assert torch.equal(x, y)


MIXED_LR0 = 3e-4
MIXED_SECTIONS = 3


def test_adaptive_lr_mixed_case():
    """desired_kl = the median per-step KL of a constant-lr run of the same inputs; the host replay must contain at least
    one raise and one lowering (else the test is vacuous and fails)."""
    _a, rows0 = _adaptive_run(None, sections=MIXED_SECTIONS, lr0=MIXED_LR0)
    kl0 = [max(r["approx_kl"]) for r in rows0]
    desired = float(np.median(kl0))
    print("constant-lr kl:", kl0, "median:", desired)
    assert all(r["lr"] == float(np.float32(MIXED_LR0)) for r in rows0)
    ad = (desired, 1.5, 1e-5, 1e-2)
    agent, rows = _adaptive_run(ad, sections=MIXED_SECTIONS, lr0=MIXED_LR0)
    print("adaptive kl:", [max(r["approx_kl"]) for r in rows])
    lrs, moves = _check_rule(rows, ad, lr0=MIXED_LR0)
    print("lr:", lrs, "moves:", moves)
    assert +1 in moves and -1 in moves, "vacuous: the rule never moved lr both ways (%r)" % (moves,)
    ref = _manual_run(lrs, sections=MIXED_SECTIONS)
    for x, y in zip(_state(agent), _state(ref)):
        assert torch.equal(x, y)
    # lr carried over from section to section: the first step of section 2 continued from the last of section 1
    assert rows[8]["lr"] == float(np.float32(host_rule(lrs[7], rows[8]["approx_kl"], *ad)[0]))


# ----------------------------------------------------------------------------- 6. with the gate
def test_adaptive_lr_with_the_kl_gate():
    ad = (1e3, 1.5, 1e-5, 1e-2)                 # raises at every applied step (the cap is out of reach in 8 steps)
    _a, rows0 = _adaptive_run(ad, sections=1)
    kl = [max(r["approx_kl"]) for r in rows0]
    k = next((j for j in range(1, len(kl)) if kl[j] > max(kl[:j])), None)    # 0-based: the first skipped step
    print("kl:", kl, "k:", k)
    assert k is not None, kl
    tkl = (max(kl[:k]) + kl[k]) / 2 / 1.5
    agent, rows = _adaptive_run(ad, sections=1, target_kl=tkl)
    assert [r["applied"] for r in rows] == [i < k for i in range(8)]
    lrs, moves = _check_rule(rows, ad)
    assert moves == [+1] * k + [0] * (8 - k)
    assert [r["lr"] for r in rows[k:]] == [rows[k - 1]["lr"]] * (8 - k)       # lr stopped moving at k
    assert rows0[k]["lr"] > rows[k]["lr"]                                     # (without the gate it went on)
    assert agent.arena.step == k == int(agent.arena.step_dev.item())
    ref = _manual_run(lrs, sections=1, applied=[r["applied"] for r in rows])
    for x, y in zip(_state(agent), _state(ref)):
        assert torch.equal(x, y)


def test_adaptive_lr_refused_by_the_sharded_step():
    from cadre_amd import hip
    agent = make_agent(84, 84)
    s = samples(64, 4, 1)
    agent.learner.set_adaptive_lr(0.01)
    agent.update_policy(dev(s[0]), dev(s[1]))
    with pytest.raises(hip.CadreHipError, match="sharded"):
        agent.learner.clip_adam_sharded(0, agent.arena.total, lambda t: None)


def test_external_optimizer_lr_scheduler_replays():
    """chief_step with an optimizer whose lr a torch scheduler moves: in device-hyper mode no graph per value, and the
    parameters equal the by-value learner's."""
    from ppo_agent.chief import chief_step
    agents = [make_agent(84, 84), make_agent(84, 84)]
    agents[1].learner.set_device_hyper()
    s = samples(64, 4, 1)
    n = []
    for ag in agents:
        shared = _shared(ag)
        opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=1e-3)
        sched = torch.optim.lr_scheduler.ExponentialLR(opt, 0.8)
        cnt = []
        for step in range(6):
            ag.update_policy(dev(s[0]), dev(s[1]))
            shared.add_gradient(ag.model_dict)
            chief_step(shared, opt, 250.0, zero_grads=False)
            opt.step(); sched.step()
            cnt.append(len(ag.learner._graphs))
        n.append(cnt)
    print("graphs:", n)
    for x, y in zip(_state(agents[0]), _state(agents[1])):
        assert torch.equal(x, y)
    assert n[1][2:] == [n[1][2]] * 4 and n[0][-1] > n[0][2]


# ----------------------------------------------------------------------------- 7. train() / train_vec()
class _Log:
    def __init__(self):
        self.lines = []

    def log(self, s):
        self.lines.append(s)


@pytest.mark.parametrize("vec", [True, False])
def test_train_schedules_and_log_line(vec, tmp_path):
    from ppo_agent.train import schedule_value, train, train_vec
    from tests.helpers import SyntheticEnv
    from tests.test_act_batch_gpu import _vec_cfgs
    EP = 2

    def run(extra):
        train_cfg, agent_cfg, env_cfg, rollout_cfg = _vec_cfgs(tmp_path, 2, 8, EP)
        train_cfg["log_stats"] = True
        train_cfg.update(extra)
        lg = _Log()
        torch.manual_seed(0)
        if vec:
            train_vec(0, train_cfg, agent_cfg, env_cfg, rollout_cfg, 2, env_cls=SyntheticEnv, logger=lg)
        else:
            train(0, train_cfg, agent_cfg, env_cfg, rollout_cfg, env_cls=SyntheticEnv, logger=lg)
        return lg.lines
    plain = run({})
    assert len(plain) == 2 * EP and not any("lr:" in l for l in plain)
    # the block at the construction values: the same lines, byte for byte, plus the lr field
    const = run({"schedules": {"lr": 3e-4, "clip": 0.1, "ent_coeff": 0.01}})
    assert [l[:-len(", lr: 3.000e-04")] if "approx kl" in l else l for l in const] == plain
    assert all(l.endswith(", lr: 3.000e-04") for l in const if "approx kl" in l)
    sch = {"lr": ("linear", 3e-4, 3e-5), "clip": ("linear", 0.1, 0.02), "ent_coeff": lambda f: 0.01 * (1.0 - f)}
    lines = [l for l in run({"schedules": sch}) if "approx kl" in l]
    assert len(lines) == EP
    for e, l in enumerate(lines):
        assert l.startswith("Episode: %d," % e)
        assert l.endswith(", lr: {:.3e}".format(schedule_value(sch["lr"], e, EP))), l
    assert lines[1].endswith(", lr: 1.650e-04")
    with pytest.raises(ValueError, match="excludes"):
        run({"schedules": sch, "adaptive_lr": {"desired_kl": 0.01}})
    # adaptive_lr (+ target_kl) through the training loop: the lr field stays inside [min, max] and is a power of the factor
    # away from train_cfg.lr (a live rollout's first minibatch has KL ~ 0, so which steps move is not asserted here)
    ad = [l for l in run({"adaptive_lr": {"desired_kl": 1e3, "min": 1e-4, "max": 1e-3}, "target_kl": 1e9}) if "approx kl" in l]
    assert len(ad) == EP
    allowed = {"{:.3e}".format(min(1e-3, 3e-4 * 1.5 ** n)) for n in range(5)}
    for l in ad:
        assert l.rsplit(", lr: ", 1)[1] in allowed, l
