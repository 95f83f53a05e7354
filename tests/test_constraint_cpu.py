"""Cost constraints, host side: config validation and refusals, the entry points by name, argument checks that need no device, the
towers' initialisation, the float64 reference (tests/constraint_ref.py) against torch.autograd, the multiplier rule, the mix statement on
hand-made arrays, and the condition the GPU parity tests rest on: few ReLU units whose branch the error bound cannot decide."""
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import constraint_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cadre_cost_note", "cadre_cost_forward", "cadre_cost_backward", "cadre_cost_lambda", "cadre_lag_mix")
AMBIGUITY_CAP = 0.02
PARITY_CASES = [(530, 3, 33, 128, 3), (37, 1, 5, 128, 4), (530, 1, 2, 128, 5), (37, 3, 2, 32, 6)]      # (D, N, T, H, seed)


def test_config_defaults_and_validation():
    from cadre_amd.constraint import CONSTRAINT_KEYS, constraint_config
    assert constraint_config(None) is None
    c = constraint_config(dict(budget=0.1))
    assert set(c) == set(CONSTRAINT_KEYS)
    assert (c["budget"], c["lambda_init"], c["lr_lambda"], c["lambda_max"], c["gamma"], c["tau"], c["hidden"], c["epochs"], c["minibatches"]) == \
        ((0.1, 0.1), (0.0, 0.0), (0.05, 0.05), 100.0, None, None, 128, 4, 4)
    assert c["max_norm"] >= 1e30                                   # never clips
    c = constraint_config(dict(budget=(0.1, 0.2), lr_lambda=[0.0, 1.0], lambda_init=2, gamma=0.9, tau=1.0))
    assert (c["budget"], c["lr_lambda"], c["lambda_init"], c["gamma"], c["tau"]) == ((0.1, 0.2), (0.0, 1.0), (2.0, 2.0), 0.9, 1.0)
    bad = [dict(), dict(budget=-1.0), dict(budget="x"), dict(budget=(0.1,)), dict(budget=(0.1, 0.2, 0.3)), dict(budget=float("nan")),
           dict(budget=True), dict(budget=0.1, beta=2.0), dict(budget=0.1, hidden=100), dict(budget=0.1, hidden=288),
           dict(budget=0.1, gamma=1.5), dict(budget=0.1, tau=-0.1), dict(budget=0.1, lr=0.0), dict(budget=0.1, epochs=0),
           dict(budget=0.1, minibatches=1.5), dict(budget=0.1, lr_lambda=-0.1), dict(budget=0.1, lambda_max=0.0),
           dict(budget=0.1, lambda_init=5.0, lambda_max=1.0), dict(budget=0.1, lambda_init=float("inf")), dict(budget=0.1, seed=-1),
           dict(budget=0.1, max_norm=0.0), "on", 3]
    for b in bad:
        with pytest.raises(ValueError):
            constraint_config(b)
    with pytest.raises(ValueError, match="beta"):
        constraint_config(dict(budget=0.1, beta=2.0))


def test_refusals_name_their_key():
    from cadre_amd.constraint import constraint_refusals
    constraint_refusals()
    constraint_refusals(checkpoint_interval=0, world=1)
    for kw, word in ((dict(sample_reuse={"window": 2}), "sample_reuse"), (dict(self_imitation={}), "self_imitation"),
                     (dict(checkpoint_interval=2), "checkpoint_interval"), (dict(resume_from="x.pt"), "resume_from"),
                     (dict(world=2), "single rank"), (dict(fused_gather=False), "fused_gather"), (dict(demo_mix={}), "demo_mix"),
                     (dict(suggest={}), "suggest"), (dict(smoothness={}), "smoothness"), (dict(aux_phase={}), "aux_phase")):
        with pytest.raises(ValueError, match=word):
            constraint_refusals(**kw)


def test_train_helper_reads_the_key_and_refuses_before_building():
    """The key absent / None gives None without touching the agent; a refused combination raises before the module is built."""
    from cadre_amd.ppo_agent import train as T
    assert T.cost_constraint(None, dict()) is None and T.cost_constraint(None, dict(cost_constraint=None)) is None
    assert T._cost_kw(None, dict(cost=1.0), 0) == {}
    assert T._cost_kw(object(), dict(cost=(1.0, 2.0)), 1) == dict(cost=2.0) and T._cost_kw(object(), dict(), 0) == dict(cost=0.0)
    key = dict(cost_constraint=dict(budget=0.1))
    for extra, word in ((dict(self_imitation=dict(coeff=0.1)), "self_imitation"), (dict(sample_reuse=dict(window=2)), "sample_reuse"),
                        (dict(demo_mix=dict()), "demo_mix"), (dict(aux_phase=dict()), "aux_phase")):
        with pytest.raises(ValueError, match=word):
            T.cost_constraint(None, dict(key, **extra))
    with pytest.raises(ValueError, match="checkpoint_interval"):
        T.cost_constraint(None, key, ck_interval=2)
    with pytest.raises(ValueError, match="resume_from"):
        T.cost_constraint(None, key, ck_resume="ckpt.pt")
    with pytest.raises(ValueError, match="fused_gather"):
        T.cost_constraint(None, key, fused_gather=False)
    with pytest.raises(ValueError, match="unknown"):
        T.cost_constraint(None, dict(cost_constraint=dict(budget=0.1, bonus=1.0)))
    from cadre_amd.constraint import constraint_stats_text
    pair = (1.0, 2.0)
    line = T.stats_line(3, dict(rows=[dict(approx_kl=(0.0, 0.0), clip_fraction=(0.0, 0.0), grad_norm=(1.0,))], explained_variance=[(0.0, 0.0)],
                                updates_applied=1, steps=1,
                                constraint=dict(steps=2, J=pair, budget=pair, costly_share=pair, mean_abs_cost_term=None,
                                                mean_abs_reward_term=pair, loss_before=pair, loss_after=None, explained_variance=pair,
                                                lambda_updates=(1, 1), **{"lambda": pair})))
    assert "constraint: J 1.0000e+00/2.0000e+00" in line and "lambda 1.0000/2.0000" in line
    assert constraint_stats_text(dict(constraint=dict(steps=0))) == ", constraint: no rows"


def test_cost_from_message_and_cost_pair():
    from cadre_amd.constraint import cost_from_message, cost_pair
    table = {"collision": (0.0, 1.0), "collision static": (0.5, 1.0), "vehicle blocked": 0.25, "route deviation": (1.0, 0.0)}
    assert cost_from_message("collision static", table) == (0.5, 1.0)          # the exact key first
    assert cost_from_message("collision vehicles!", table) == (0.0, 1.0)       # then the longest prefix
    assert cost_from_message("vehicle blocked", table) == (0.25, 0.25) and cost_from_message("route deviation", table) == (1.0, 0.0)
    assert cost_from_message("", table) == cost_from_message("success", table) == cost_from_message(None, table) == (0.0, 0.0)
    assert cost_pair(2) == (2.0, 2.0) and cost_pair([0.0, 3.0]) == (0.0, 3.0)
    for bad in (-1.0, (1.0,), (0.0, float("nan")), "x", True):
        with pytest.raises(ValueError):
            cost_pair(bad)
    with pytest.raises(ValueError):
        cost_from_message("x", ["collision"])
    with pytest.raises(ValueError):
        cost_from_message("collision", {"collision": -1.0})


def test_entry_points_declared_bound_exported():
    from cadre_amd import build, hip
    hdr = open(os.path.join(ROOT, "include", "cadre_hip.h")).read()
    L = hip.lib()
    for name in NEW:
        assert hasattr(L, name) and name in hip.SYMBOLS and re.search(r"\bint %s\s*\(" % name, hdr), name
    assert "constraint.hip" in build.SOURCES
    assert L.cadre_abi_version() == hip.ABI_VERSION == 15                  # entry points only added
    for name in ("LAMBDA", "BUDGET", "LR", "MAX", "J", "SHARE", "UPDATES", "STRIDE"):
        assert int(re.search(r"#define CADRE_LAG_%s (\d+)" % name, hdr).group(1)) == getattr(hip, "LAG_" + name) == getattr(ref, "LAG_" + name)
    import ppo_agent.constraint as shim
    from cadre_amd.constraint import CostConstraint, cost_from_message
    assert shim.CostConstraint is CostConstraint and shim.cost_from_message is cost_from_message


def test_argument_checks_need_no_device():
    """Every entry point refuses bad sizes on the host (pointers are never dereferenced there), naming itself."""
    from cadre_amd import hip
    L, p = hip.lib(), 64
    base = dict(tab=p, n=2, Tr=6, S=3, ldo=544, D=530, H=128, row0=0, rows=12, tower=p, values=p, h1=None, h2=None, stream=None)
    fwd = lambda **o: L.cadre_cost_forward(*dict(base, **o).values())          # (insertion order = argument order)
    for o in (dict(D=0), dict(D=1025), dict(H=100), dict(H=288), dict(H=0), dict(ldo=529), dict(rows=0), dict(rows=13), dict(row0=-1),
              dict(row0=7, rows=6), dict(tab=None), dict(values=None), dict(tower=None), dict(Tr=0), dict(n=0), dict(S=0)):
        assert fwd(**o) < 0, o
        assert b"cadre_cost_forward" in L.cadre_last_error()
    bbase = dict(tab=p, n=2, Tr=5, S=3, ldo=544, D=530, H=128, row0=0, rows=10, tower=p, values=p, h1=p, h2=p, returns=p, ldr=6, grads=p,
                 loss=p, scratch=p, stream=None)
    bwd = lambda **o: L.cadre_cost_backward(*dict(bbase, **o).values())
    for o in (dict(D=0), dict(H=48), dict(ldr=4), dict(rows=11), dict(rows=0), dict(row0=6, rows=5), dict(h1=None), dict(returns=None),
              dict(grads=None), dict(scratch=None), dict(ldo=100)):
        assert bwd(**o) < 0, o
        assert b"cadre_cost_backward" in L.cadre_last_error()
    for a in ((None, p, p, 2, 5, None), (p, None, p, 2, 5, None), (p, p, None, 2, 5, None), (p, p, p, 0, 5, None), (p, p, p, 2, 0, None)):
        assert L.cadre_cost_note(*a) < 0 and b"cadre_cost_note" in L.cadre_last_error(), a
    for a in ((None, 2, 5, p, 1, None), (p, 2, 5, None, 1, None), (p, 0, 5, p, 1, None), (p, 2, 1, p, 1, None), (p, 2, 3001, p, 1, None)):
        assert L.cadre_cost_lambda(*a) < 0 and b"cadre_cost_lambda" in L.cadre_last_error(), a
    for a in ((None, 2, 5, p, None, None), (p, 2, 5, None, None, None), (p, 3, 5, p, None, None), (p, 0, 5, p, None, None),
              (p, 2, 1, p, None, None), (p, 2, 3001, p, None, None)):
        assert L.cadre_lag_mix(*a) < 0 and b"cadre_lag_mix" in L.cadre_last_error(), a


def test_storage_cost_argument_is_checked_on_the_host():
    """insert(cost=) on a CPU storage: no tensor before the first cost, then every insert writes the slot; bad costs are refused before
    anything is written."""
    from ppo_agent.storage import RolloutStorage
    s = RolloutStorage(4, 1, 6, 2, 6, True, 0.99, 0.95)
    row = lambda **kw: s.insert(torch.zeros(2, 6), torch.tensor([1]), torch.tensor([0.0]), torch.tensor([0.0]), 1.0, torch.tensor([[1.0]]), None,
                                0, **kw)
    row()
    assert getattr(s, "costs", None) is None
    row(cost=0.5)
    row()
    assert s.costs.tolist() == [0.0, 0.5, 0.0, 0.0, 0.0] and s.step == 3
    for bad in (-1.0, float("nan"), float("inf"), "x", True, (1.0, 2.0)):
        with pytest.raises(ValueError):
            row(cost=bad)
    assert s.step == 3
    with pytest.raises(ValueError, match="costs"):
        RolloutStorage.insert_batch([(s, s)], [None], [[0, 0]], [[1, 1]], [0], costs=[1.0, 2.0])
    with pytest.raises(ValueError, match="cost"):
        RolloutStorage.insert_batch([(s, s)], [None], [[0, 0]], [[1, 1]], [0], costs=[(1.0, -2.0)])


def test_towers_are_orthogonal_and_leave_the_global_generator():
    from cadre_amd.constraint import cost_tower_offsets, init_cost_tower
    torch.manual_seed(5)
    before = torch.get_rng_state().clone()
    gen = torch.Generator()
    gen.manual_seed(11)
    D, H = 37, 64
    p = init_cost_tower(D, H, gen)
    q = init_cost_tower(D, H, gen)
    assert torch.equal(torch.get_rng_state(), before)
    offs, P = cost_tower_offsets(D, H)
    assert p.numel() == P == D * H + H + H * H + H + H + 1 and (offs, P) == ref.tower_offsets(D, H) and not torch.equal(p, q)
    W1, b1, W2, b2, W3, b3 = ref.unpack(p.numpy(), D, H)
    assert not b1.any() and not b2.any() and not b3.any()
    assert np.allclose(W1 @ W1.T, 2.0 * np.eye(D), atol=1e-5)            # [D][H] input-major, D < H: the rows are orthogonal
    assert np.allclose(W2 @ W2.T, 2.0 * np.eye(H), atol=1e-5)
    assert np.allclose(W3.T @ W3, np.eye(1), atol=1e-5)                   # gain 1: a unit vector
    gen.manual_seed(11)
    assert torch.equal(init_cost_tower(D, H, gen), p)


def test_reference_gradient_against_autograd():
    """The reference's backward pass is the gradient torch.autograd (float64) gives for L = 0.5 mean (v - R)^2."""
    D, N, T, H = 37, 1, 12, 32
    x, towers = ref.case_inputs(D, N, T, H, 1)
    x, p = x[0], towers[0]
    R = x.shape[0]
    ret = np.random.RandomState(2).rand(R).astype(np.float32)
    fw = ref.forward(x, p, H)
    (grad, _e), (loss, _el), _dv = ref.backward(fw, p, ret, H)
    pg = torch.from_numpy(np.asarray(p, np.float64)).requires_grad_(True)
    o, _P = ref.tower_offsets(D, H)
    xt = torch.from_numpy(x).double()
    h1 = torch.relu(xt @ pg[o[0]:o[1]].view(D, H) + pg[o[1]:o[2]])
    h2 = torch.relu(h1 @ pg[o[2]:o[3]].view(H, H) + pg[o[3]:o[4]])
    v = h2 @ pg[o[4]:o[5]] + pg[o[5]]
    L = 0.5 * ((v - torch.from_numpy(ret).double()) ** 2).mean()
    L.backward()
    assert np.allclose(v.detach().numpy(), fw["v"][0], rtol=1e-12, atol=1e-14)
    assert abs(float(L.detach()) - loss) <= 1e-12 * abs(loss) and abs(ref.loss(x, p, ret, H) - loss) <= 1e-12 * abs(loss)
    scale = np.abs(pg.grad.numpy()).max()
    assert scale > 0 and np.abs(grad - pg.grad.numpy()).max() <= 1e-12 * scale


def test_lambda_rule():
    """Clamped at 0, clamped at lambda_max, moving in the direction of J - budget, frozen."""
    c = np.array([[0.0, 1.0, 0.0, 0.5], [0.0, 0.0, 2.0, 0.5]], np.float32)
    J, share, lam = ref.lambda_step(c, 1.0, 0.25, 0.5, 10.0)
    assert J == 0.5 and share == 0.5 and lam == 1.0 + 0.5 * 0.25
    assert ref.lambda_step(c, 0.05, 1.0, 0.5, 10.0)[2] == 0.0            # the floor
    assert ref.lambda_step(c, 9.9, 0.0, 1.0, 10.0)[2] == 10.0            # the ceiling
    assert ref.lambda_step(c, 1.0, 1.0, 0.5, 10.0)[2] < 1.0 < ref.lambda_step(c, 1.0, 0.0, 0.5, 10.0)[2]
    assert ref.lambda_step(c, 1.0, 0.0, 0.5, 10.0, train=False) == (0.5, 0.5, 1.0)


def test_mix_statement_on_hand_made_arrays():
    """lambda = 0 returns the reward advantages themselves (a -0 keeps its sign bit); lambda > 0: the four statements in float32."""
    a_r = np.array([-0.0, 1.0, -2.0, 0.5], np.float32)
    a_c = np.array([1.0, 3.0, -1.0, 1.0], np.float32)
    out, m = ref.mix(a_r, a_c, 0.0)
    assert out is a_r and m == 1.0 and np.signbit(out[0])
    assert ref.mix(a_r, a_c, 1e-60)[0] is a_r                            # (float)lambda == 0
    out, m = ref.mix(a_r, a_c, 1.0)
    assert m == 1.0 and out.dtype == np.float32 and out.tolist() == [0.0, -0.5, 0.0, 0.25]
    # the reason lambda == 0 must store nothing: with c = -0 (A_c = -0, m = +0) the statement q = A_r - p is -0 - (-0) = +0
    z, m = ref.mix(a_r, np.array([-0.0, 1.0, -1.0, 0.0], np.float32), 0.5)
    assert m == 0.0 and not np.signbit(m) and z[0] == 0.0 and not np.signbit(z[0]) and np.signbit(a_r[0])
    big = np.float32(3.0) * np.ones(5, np.float32)
    out, m = ref.mix(np.zeros(5, np.float32), big + np.arange(5, dtype=np.float32), 3.0)
    assert m == 5.0 and out.tolist() == [1.5, 0.75, 0.0, -0.75, -1.5]


@pytest.mark.parametrize("D,N,T,H,seed", PARITY_CASES)
def test_constraint_relu_ambiguity_cap(D, N, T, H, seed):
    """The condition of the GPU parity tests, from the reference alone: at most 2 % of the units of a layer lie within their own error
    bound of zero in the tests' inputs (unit-normal rows, orthogonal weights)."""
    x, towers = ref.case_inputs(D, N, T, H, seed)
    for h in (0, 1):
        fw = ref.forward(x[h], towers[h], H)
        amb = ref.ambiguity(fw)
        print("ambiguous units D=%d rows=%d head %d: %s" % (D, x[h].shape[0], h, amb))
        assert max(amb.values()) <= AMBIGUITY_CAP
        assert np.isfinite(fw["v"][0]).all() and np.isfinite(fw["v"][1]).all() and math.isfinite(ref.loss(x[h], towers[h], 0 * fw["v"][0], H))
