"""CPU: the demonstration term inside the PPO step — the float64 reference's identity, demo_mix_config, the stateless
DemoMixer draw, the coefficient schedule, and the two entry points by name (declared, bound, exported, refusing bad arguments
before any launch)."""
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import demo_mix_ref, imitation_ref, ordinal_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLIP, VC, CC, EC = 0.1, 0.1, 1.0, 0.01
EPS, DC, DVC = 0.1, 0.7, 0.3


def mixed_case(B, n_ppo, C, nS, nT, seed):
    """Random inputs with n_ppo PPO rows per head at random positions (other positions per head), valid commands."""
    g = torch.Generator().manual_seed(seed)
    K = (nS, nT)
    logits = torch.zeros(2 * C, B, 64, dtype=torch.float64)
    logits[:C, :, :nS] = torch.randn(C, B, nS, generator=g, dtype=torch.float64)
    logits[C:, :, :nT] = torch.randn(C, B, nT, generator=g, dtype=torch.float64)
    values = torch.randn(2 * C, B, generator=g, dtype=torch.float64)
    actions = torch.stack([torch.randint(0, nS, (B,), generator=g), torch.randint(0, nT, (B,), generator=g)])
    cmds = torch.randint(0, C, (2, B), generator=g, dtype=torch.int32)
    old_v, rets = torch.randn(2, B, generator=g), torch.randn(2, B, generator=g)
    adv = torch.randn(2, B, generator=g)
    old_lp = torch.stack([-math.log(K[hd]) + 0.2 * torch.randn(B, generator=g) for hd in range(2)])
    kind = torch.ones(2, B, dtype=torch.int32)
    for hd in range(2):
        kind[hd, torch.randperm(B, generator=g)[:n_ppo]] = 0
    adv = torch.where(kind == 0, adv, adv.abs() + 0.25)                   # demonstration rows: a positive weight
    ranks = (torch.randperm(nS, generator=g).tolist(), torch.randperm(nT, generator=g).tolist())
    return dict(logits=logits, values=values, actions=actions, cmds=cmds, old_v=old_v, rets=rets, old_lp=old_lp, adv=adv,
                kind=kind), K, ranks


@pytest.mark.parametrize("ordinal", [False, True])
def test_mixed_reference_is_ppo_reference_plus_bc_reference(ordinal):
    """Losses and gradients in float64: the mixed reference on B = 24 rows equals tests/ordinal_ref.ppo_loss on the PPO rows
    alone (a minibatch of its own, inv_b = 1 / rows) plus tests/imitation_ref.bc_loss on the demonstration rows alone."""
    B, n_ppo, C, nS, nT = 24, 10, 3, 33, 3
    inp, K, ranks = mixed_case(B, n_ppo, C, nS, nT, seed=5)
    rk = ranks if ordinal else (None, None)
    n_demo = B - n_ppo
    lg, vv = inp["logits"].clone().requires_grad_(True), inp["values"].clone().requires_grad_(True)
    out = demo_mix_ref.mixed_loss(lg, vv, inp["actions"], inp["cmds"], inp["old_v"], inp["rets"], inp["old_lp"], inp["adv"],
                                  inp["kind"], K, rk, C, CLIP, VC, CC, EC, 1.0 / n_ppo, EPS, DC, DVC, 1.0 / n_demo)
    out["total"].backward()
    # the PPO rows of each head as a minibatch of their own, the demonstration rows as another
    sub = {}
    for name, flag, n in (("ppo", 0, n_ppo), ("demo", 1, n_demo)):
        rows = [torch.nonzero(inp["kind"][hd] == flag).view(-1) for hd in range(2)]
        s_lg = torch.cat([inp["logits"][hd * C:(hd + 1) * C][:, rows[hd]] for hd in range(2)]).clone().requires_grad_(True)
        s_vv = torch.cat([inp["values"][hd * C:(hd + 1) * C][:, rows[hd]] for hd in range(2)]).clone().requires_grad_(True)
        pick = lambda t: torch.stack([t[hd][rows[hd]] for hd in range(2)])
        sub[name] = (rows, s_lg, s_vv, pick)
    rows, s_lg, s_vv, pick = sub["ppo"]
    tv, ta, te, total = ordinal_ref.ppo_loss(s_lg, s_vv, pick(inp["actions"]), pick(inp["cmds"]), pick(inp["old_v"]).double(),
                                             pick(inp["rets"]).double(), pick(inp["old_lp"]).double(), pick(inp["adv"]).double(),
                                             K, rk, C, CLIP, VC, CC, EC)
    total.backward()
    for got, want in zip(out["losses"], (tv, ta, te)):
        assert abs(float(got.detach()) - float(want.detach())) < 1e-12
    for hd in range(2):
        assert float((lg.grad[hd * C:(hd + 1) * C][:, rows[hd]] - s_lg.grad[hd * C:(hd + 1) * C]).abs().max()) < 1e-14
        assert float((vv.grad[hd * C:(hd + 1) * C][:, rows[hd]] - s_vv.grad[hd * C:(hd + 1) * C]).abs().max()) < 1e-14
    rows, s_lg, s_vv, pick = sub["demo"]
    bv, bb, be, total, stats = imitation_ref.bc_loss(s_lg, s_vv, pick(inp["actions"]), pick(inp["cmds"]), pick(inp["rets"]),
                                                     pick(inp["adv"]), K, rk, C, EPS, DC, DVC, 0.0, 1.0 / n_demo)
    total.backward()
    db, dv = (float(t.detach()) for t in out["demo_losses"])
    assert abs(db - float(bb.detach())) < 1e-12 and abs(dv - float(bv.detach())) < 1e-12
    assert float(torch.as_tensor(be).detach()) == 0.0 and float((out["demo_stats"] - stats).abs().max()) < 1e-12
    for hd in range(2):
        assert float((lg.grad[hd * C:(hd + 1) * C][:, rows[hd]] - s_lg.grad[hd * C:(hd + 1) * C]).abs().max()) < 1e-14
        assert float((vv.grad[hd * C:(hd + 1) * C][:, rows[hd]] - s_vv.grad[hd * C:(hd + 1) * C]).abs().max()) < 1e-14
    assert float(lg.grad.abs().max()) > 0 and abs(float(out["demo_stats"][0, 5]) - 1.0) < 1e-12


# ----------------------------------------------------------------------------- demo_mix_config
def test_demo_mix_config_defaults():
    from ppo_agent.imitation import DEMO_MIX_KEYS, demo_mix_config
    assert demo_mix_config(None) is None
    cfg = demo_mix_config(dict(episodes="/records"))
    assert cfg == dict(episodes="/records", coeff=1.0, value_coeff=0.0, blocks=1, label_smoothing=0.0, balance="command",
                       return_scale=1.0, seed=0)
    assert sorted(cfg) == sorted(DEMO_MIX_KEYS)
    f = lambda x: 1.0 - x
    full = demo_mix_config(dict(episodes=["a", "b"], coeff=["linear", 1, 0], value_coeff=0.5, blocks=2, label_smoothing=0.1,
                                balance=None, return_scale=0.25, seed=7))
    assert full["coeff"] == ("linear", 1, 0) and full["blocks"] == 2 and full["balance"] is None and full["seed"] == 7
    assert full["value_coeff"] == 0.5 and full["return_scale"] == 0.25 and full["label_smoothing"] == 0.1
    assert demo_mix_config(dict(episodes="d", coeff=f))["coeff"] is f


@pytest.mark.parametrize("bad", [
    "records", dict(), dict(coeff=1.0), dict(episodes="d", epochs=3), dict(episodes="d", coeff="linear"),
    dict(episodes="d", coeff=("linear", 1.0)), dict(episodes="d", coeff=("cosine", 1.0, 0.0)), dict(episodes="d", coeff=True),
    dict(episodes="d", coeff=float("nan")), dict(episodes="d", coeff=("linear", "a", 0.0)), dict(episodes="d", blocks=0),
    dict(episodes="d", blocks=1.5), dict(episodes="d", blocks=True), dict(episodes="d", label_smoothing=1.0),
    dict(episodes="d", label_smoothing=-0.1), dict(episodes="d", balance="row"), dict(episodes="d", value_coeff="x"),
    dict(episodes="d", value_coeff=float("inf")), dict(episodes="d", return_scale=None), dict(episodes="d", seed=0.5)])
def test_demo_mix_config_refusals(bad):
    from ppo_agent.imitation import demo_mix_config
    with pytest.raises(ValueError, match="demo_mix"):
        demo_mix_config(bad)


# ----------------------------------------------------------------------------- DemoMixer
class FakeSet(object):
    def __init__(self, T):
        self.T = T
        self.steer, self.throttle, self.weights = "steer", "throttle", "weights"

    def __len__(self):
        return self.T

    def batch(self, idx):
        return [(self.steer, idx, self.weights, self.throttle, idx, self.weights)]


def flat(entries):
    return torch.cat([e[1] for e in entries])


def test_demo_mixer_draw_is_a_pure_function_of_its_key():
    from ppo_agent.imitation import DemoMixer
    demo = FakeSet(100)
    a, b = DemoMixer(demo, blocks=2, seed=3, rank=1), DemoMixer(demo, blocks=2, seed=3, rank=1)
    e = a.entries(16, 4, 9)
    assert len(e) == 2 and all(x[1].numel() == 16 and x[1].dtype == torch.int64 and x[0] == "steer" and x[3] == "throttle"
                               and x[2] == "weights" and x[4] is x[1] for x in e)
    base = flat(e)
    assert int(base.min()) >= 0 and int(base.max()) < 100 and base.unique().numel() == 32          # a prefix of a permutation
    a.entries(16, 0, 0)                                                    # no state: another draw in between changes nothing
    assert torch.equal(flat(a.entries(16, 4, 9)), base) and torch.equal(flat(b.entries(16, 4, 9)), base)
    for other in (flat(a.entries(16, 5, 9)), flat(a.entries(16, 4, 10)), flat(DemoMixer(demo, 2, seed=3, rank=0).entries(16, 4, 9)),
                  flat(DemoMixer(demo, 2, seed=4, rank=1).entries(16, 4, 9)), flat(DemoMixer(FakeSet(101), 2, 3, 1).entries(16, 4, 9))):
        assert not torch.equal(other, base)
    assert not torch.equal(flat(a.entries(8, 4, 9)), base[:16])            # Bw and blocks are part of the key too
    assert not torch.equal(flat(DemoMixer(demo, 1, 3, 1).entries(16, 4, 9)), base[:16])


def test_demo_mixer_leaves_the_global_generator_alone():
    from ppo_agent.imitation import DemoMixer
    m = DemoMixer(FakeSet(50), blocks=1, seed=0, rank=0)
    torch.manual_seed(123)
    before = torch.get_rng_state().clone()
    np_before = np.random.get_state()[1].copy()
    for i in range(100):
        m.entries(16 if i % 2 else 64, i // 10, i % 10)
    assert torch.equal(torch.get_rng_state(), before) and np.array_equal(np.random.get_state()[1], np_before)


def test_demo_mixer_samples_with_replacement_only_when_it_must():
    from ppo_agent.imitation import DemoMixer
    exact = flat(DemoMixer(FakeSet(32), blocks=2).entries(16, 0, 0))       # blocks * Bw == len: still a permutation
    assert sorted(exact.tolist()) == list(range(32))
    more = flat(DemoMixer(FakeSet(10), blocks=2).entries(16, 0, 0))        # 32 rows from 10: with replacement
    assert more.numel() == 32 and int(more.min()) >= 0 and int(more.max()) < 10
    with pytest.raises(ValueError):
        DemoMixer(FakeSet(10), blocks=0)
    with pytest.raises(ValueError):
        DemoMixer(FakeSet(0))
    with pytest.raises(ValueError):
        DemoMixer(FakeSet(10)).entries(0, 0, 0)


def test_coefficient_schedule_values():
    from ppo_agent.imitation import demo_mix_config
    from ppo_agent.train import schedule_value
    lin = demo_mix_config(dict(episodes="d", coeff=("linear", 1.0, 0.0)))["coeff"]
    assert [schedule_value(lin, e, 4) for e in range(4)] == [1.0, 0.75, 0.5, 0.25]
    assert schedule_value(demo_mix_config(dict(episodes="d", coeff=0.3))["coeff"], 3, 4) == 0.3
    dapg = lambda x: 0.1 * 0.95 ** (100 * x)                               # DAPG's lambda0 lambda1^k as a callable
    assert schedule_value(demo_mix_config(dict(episodes="d", coeff=dapg))["coeff"], 50, 100) == 0.1 * 0.95 ** 50.0


def test_demo_mix_needs_the_fused_gather():
    from ppo_agent.train import demo_mixer

    class Cfg(dict):
        gamma = 0.99
    assert demo_mixer(None, dict(), Cfg()) is None and demo_mixer(None, dict(demo_mix=None), Cfg(), fused_gather=False) is None
    with pytest.raises(ValueError, match="fused_gather"):
        demo_mixer(None, dict(demo_mix=dict(episodes="d")), Cfg(), fused_gather=False)


# ----------------------------------------------------------------------------- the entry points, by name
def test_demo_mix_entry_points_declared_bound_exported():
    from cadre_amd import build, hip
    hdr = open(os.path.join(ROOT, "include", "cadre_hip.h")).read()
    L = hip.lib()
    for name in ("cadre_ppo_demo_loss", "cadre_mix_row_kinds"):
        assert re.search(r"\bint %s\(" % name, hdr) and name in hip.SYMBOLS and hasattr(L, name), name
    assert "demo_mix.hip" in build.SOURCES
    assert L.cadre_abi_version() == hip.ABI_VERSION == 15                  # entry points only added
    m = re.search(r"CADRE_HP_DEMO_COEFF = (\d+), CADRE_HP_DEMO_VALUE_COEFF = (\d+)", hdr)
    assert m and (int(m.group(1)), int(m.group(2))) == (hip.HP_DEMO_COEFF, hip.HP_DEMO_VALUE_COEFF) == (10, 11)
    assert hip.HP_INDEX["demo_coeff"] == 10 and hip.HP_INDEX["demo_value_coeff"] == 11 and hip.HP_FIELDS == 16
    assert all(hip.HP_INDEX[k] == v for k, v in hip.HP.items()) and len(set(hip.HP_INDEX.values())) == 12


def mix_args(**over):
    """Arguments of cadre_ppo_demo_loss that pass every check (pointers are never dereferenced on the host)."""
    p = 64
    a = dict(logits=p, ldl=64, l_ns=64, values=p, ldv=1, v_ns=1, actions=p, commands=p, old_values=p, returns=p, old_logp=p,
             adv=p, row_kind=p, B=8, C=4, nS=33, nT=3, hp=None, clip=0.1, vc=0.1, cc=1.0, ec=0.01, inv_b=0.25, eps=0.0, dc=1.0,
             dvc=0.0, inv_bd=0.25, losses=p, demo_losses=p, dl=p, dv=p, scratch=p, demo_scratch=p, poison=None, stats_row=None,
             F=0, stats_scratch=None, target_kl=0.0, stop=None, demo_stats=None, demo_F=0, ord=None, stream=None)
    assert set(over) <= set(a)
    a.update(over)
    return tuple(a.values())


@pytest.mark.parametrize("over,msg", [
    (dict(row_kind=None), b"row_kind"), (dict(eps=1.0), b"label_smoothing"), (dict(eps=-0.01), b"label_smoothing"),
    (dict(eps=float("nan")), b"label_smoothing"), (dict(inv_bd=0.0), b"inv_bd"), (dict(inv_bd=-1.0), b"inv_bd"),
    (dict(inv_bd=float("inf")), b"inv_bd"), (dict(inv_bd=float("nan")), b"inv_bd"),
    (dict(inv_bd=0.0, dc=0.0, dvc=0.5), b"inv_bd"), (dict(inv_bd=0.0, dc=0.0, demo_stats=64, demo_F=6), b"inv_bd"),
    (dict(inv_bd=0.0, dc=0.0, hp=64), b"inv_bd"),
    # the argument checks of the two kernels this extends
    (dict(logits=None), b"bad argument"), (dict(old_logp=None), b"bad argument"), (dict(losses=None), b"bad argument"),
    (dict(demo_losses=None), b"bad argument"), (dict(dl=None), b"bad argument"), (dict(dv=None), b"bad argument"),
    (dict(scratch=None), b"bad argument"), (dict(demo_scratch=None), b"bad argument"), (dict(B=0), b"bad argument"),
    (dict(C=0), b"bad argument"), (dict(nS=65), b"bad argument"), (dict(nT=0), b"bad argument"), (dict(ldl=32), b"bad argument"),
    (dict(ldl=65), b"bad argument"), (dict(stats_row=64, F=7, stats_scratch=64), b"stats argument"),
    (dict(stats_row=64, F=8), b"stats argument"), (dict(stats_row=64, F=8, stats_scratch=64, target_kl=0.1), b"stats argument"),
    (dict(stats_row=64, F=8, stats_scratch=64, target_kl=-1.0), b"stats argument"),
    (dict(demo_stats=64, demo_F=5), b"demo stats"), (dict(hp=68), b"hyper-parameter block")])
def test_ppo_demo_loss_refuses_before_any_launch(over, msg):
    """Negative status and a readable message, checked before any HIP call: this runs without a GPU."""
    from cadre_amd import hip
    L = hip.lib()
    assert L.cadre_ppo_demo_loss(*mix_args(**over)) == -1
    err = L.cadre_last_error()
    assert b"cadre_ppo_demo_loss" in err and msg in err, err


def test_mix_row_kinds_refuses_before_any_launch():
    from cadre_amd import hip
    L = hip.lib()
    for args in ((None, 8, 4, None, None), (None, 0, 0, 64, None), (None, 8, -1, 64, None), (None, 8, 9, 64, None)):
        assert L.cadre_mix_row_kinds(*args) == -1 and b"cadre_mix_row_kinds" in L.cadre_last_error()
    assert b"B_ppo" in L.cadre_last_error()
    # inv_bd is not needed when nothing reads it: by-value scalars, both demo coefficients zero, no demo stats row — the
    # check then falls through to the launch, so only the refusals above are exercised here


def test_learner_modes_without_a_device():
    """set_loss / set_demo_rows argument checks and the hipGraph key of the mixed mode, on an object that owns no arena."""
    from cadre_amd.learner import PPOLearnerHIP
    lrn = PPOLearnerHIP.__new__(PPOLearnerHIP)
    lrn._hp_on, lrn.stats, lrn.target_kl, lrn._adaptive, lrn.consensus = False, False, None, None, False
    lrn._bc, lrn._demo, lrn._demo_rows, lrn.loss_mode = (0.0, 1.0), (0.0, 0.0, 0.0), None, "ppo"
    lrn.a = type("A", (), {})()
    assert lrn._mode_key() == ()
    lrn.set_loss("ppo+demo", label_smoothing=0.1, demo_coeff=0.5, demo_value_coeff=0.25)
    lrn.set_demo_rows(12)
    assert lrn._mode_key() == (("demo", 0.1, 12, 0.5, 0.25),)
    lrn._hp_on = True                                                      # the coefficients live in the block: not in the key
    assert lrn._mode_key() == (("hp",), ("demo", 0.1, 12))
    lrn._hp_on = False
    lrn.set_loss("ppo")
    assert lrn._mode_key() == () and lrn._demo == (0.1, 0.5, 0.25)
    for kw in (dict(label_smoothing=1.0), dict(demo_coeff=float("nan")), dict(demo_value_coeff=float("inf"))):
        with pytest.raises(ValueError):
            lrn.set_loss("ppo+demo", **kw)
    with pytest.raises(ValueError):
        lrn.set_loss("demo")
    with pytest.raises(ValueError):
        lrn.set_demo_rows(-1)


@pytest.mark.parametrize("kw", [dict(demo_coeff=True), dict(demo_value_coeff=False)])
def test_set_loss_refuses_a_bool_demo_coefficient(kw):
    """The coefficient check is one for every loss mode: a bool is refused (it used to count as 1.0 / 0.0 here)."""
    from cadre_amd.learner import PPOLearnerHIP
    lrn = PPOLearnerHIP.__new__(PPOLearnerHIP)
    lrn._hp_on, lrn._demo, lrn.loss_mode = False, (0.0, 0.5, 0.25), "ppo"
    with pytest.raises(ValueError, match="set_loss: demo_coeff=.*, demo_value_coeff="):
        lrn.set_loss("ppo+demo", **kw)
    assert lrn._demo == (0.0, 0.5, 0.25) and lrn.loss_mode == "ppo"
