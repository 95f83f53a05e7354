"""Curiosity bonus, host side: config validation and refusals, the entry points by name, argument checks that need no device, the
float64 reference (tests/curiosity_ref.py) against torch.autograd, the Chan merge against one numpy pass, and the condition the
GPU parity tests rest on: few ReLU units whose branch the error bound cannot decide."""
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import curiosity_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cadre_rnd_obs_stats", "cadre_rnd_forward", "cadre_rnd_reward", "cadre_rnd_backward")
AMBIGUITY_CAP = 0.02


def case_inputs(D, R, H, E, seed, shift=0.0):
    """Rows of unit normals (x `shift`ed), statistics of those rows, two orthogonal towers: what the parity tests use."""
    from cadre_amd.curiosity import init_tower
    rng = np.random.RandomState(seed)
    x = (rng.randn(R, D) + shift).astype(np.float32)
    n, mu, M2 = ref.chan_merge(0.0, np.zeros(D), np.zeros(D), x)
    gen = torch.Generator()
    gen.manual_seed(seed)
    return x, (n, mu, M2), init_tower(D, H, E, gen).numpy(), init_tower(D, H, E, gen).numpy()


PARITY_CASES = [(530, 99, 128, 64, 3), (37, 99, 128, 32, 4), (530, 5, 128, 64, 5), (37, 3, 128, 64, 6)]


def test_config_defaults_and_validation():
    from cadre_amd.curiosity import CURIOSITY_KEYS, curiosity_config
    assert curiosity_config(None) is None
    c = curiosity_config(dict(coeff=0.5))
    assert set(c) == set(CURIOSITY_KEYS)
    assert (c["coeff"], c["ext_coeff"], c["gamma"], c["hidden"], c["embed"], c["lr"], c["update_proportion"], c["obs_clip"]) == \
        (0.5, 1.0, 0.99, 128, 64, 1e-4, 0.25, 5.0)
    assert c["max_norm"] >= 1e30                                   # never clips
    assert curiosity_config(dict(coeff=("linear", 1.0, 0.0)))["coeff"] == ("linear", 1.0, 0.0)
    f = lambda frac: 1.0 - frac
    assert curiosity_config(dict(coeff=f))["coeff"] is f
    bad = [dict(), dict(coeff=-1.0), dict(coeff="x"), dict(coeff=("linear", 1.0)), dict(coeff=("linear", -1.0, 0.0)), dict(coeff=1.0, beta=2.0),
           dict(coeff=1.0, hidden=100), dict(coeff=1.0, hidden=288), dict(coeff=1.0, embed=0), dict(coeff=1.0, embed=48),
           dict(coeff=1.0, gamma=1.5), dict(coeff=1.0, gamma=-0.1), dict(coeff=1.0, lr=0.0), dict(coeff=1.0, epochs=0),
           dict(coeff=1.0, minibatches=1.5), dict(coeff=1.0, update_proportion=1.1), dict(coeff=1.0, update_proportion=-0.1),
           dict(coeff=1.0, obs_clip=0.0), dict(coeff=1.0, seed=-1), dict(coeff=1.0, ext_coeff=-1.0), dict(coeff=1.0, max_norm=0.0),
           dict(coeff=float("nan")), dict(coeff=True), "on", 3]
    for b in bad:
        with pytest.raises(ValueError):
            curiosity_config(b)
    with pytest.raises(ValueError, match="beta"):
        curiosity_config(dict(coeff=1.0, beta=2.0))


def test_refusals_name_their_key():
    from cadre_amd.curiosity import curiosity_refusals
    curiosity_refusals()
    curiosity_refusals(reward_scaling=None, checkpoint_interval=0, world=1)
    for kw, word in ((dict(reward_scaling=True), "reward_scaling"), (dict(reward_scaling={"clip": 5.0}), "reward_scaling"),
                     (dict(self_imitation={}), "self_imitation"), (dict(sample_reuse={"window": 2}), "sample_reuse"),
                     (dict(checkpoint_interval=2), "checkpoint_interval"), (dict(resume_from="x.pt"), "resume_from"),
                     (dict(world=2), "single rank"), (dict(fused_gather=False), "fused_gather")):
        with pytest.raises(ValueError, match=word):
            curiosity_refusals(**kw)


def test_train_helper_reads_the_key_and_refuses_before_building():
    """The key absent / None gives None without touching the agent; a refused combination raises before the module is built."""
    from cadre_amd.ppo_agent import train as T
    assert T.curiosity(None, dict()) is None and T.curiosity(None, dict(curiosity=None)) is None
    assert T.apply_curiosity(None, 0, 2) is None
    for extra, word in ((dict(reward_scaling=True), "reward_scaling"), (dict(self_imitation=dict(coeff=0.1)), "self_imitation"),
                        (dict(sample_reuse=dict(window=2)), "sample_reuse")):
        with pytest.raises(ValueError, match=word):
            T.curiosity(None, dict(curiosity=dict(coeff=1.0), **extra))
    with pytest.raises(ValueError, match="checkpoint_interval"):
        T.curiosity(None, dict(curiosity=dict(coeff=1.0)), ck_interval=2)
    with pytest.raises(ValueError, match="resume_from"):
        T.curiosity(None, dict(curiosity=dict(coeff=1.0)), ck_resume="ckpt.pt")
    with pytest.raises(ValueError, match="fused_gather"):
        T.curiosity(None, dict(curiosity=dict(coeff=1.0)), fused_gather=False)
    with pytest.raises(ValueError, match="unknown"):
        T.curiosity(None, dict(curiosity=dict(coeff=1.0, bonus=1.0)))
    from cadre_amd.curiosity import curiosity_stats_text
    line = T.stats_line(3, dict(rows=[dict(approx_kl=(0.0, 0.0), clip_fraction=(0.0, 0.0), grad_norm=(1.0,))], explained_variance=[(0.0, 0.0)],
                                updates_applied=1, steps=1,
                                curiosity=dict(steps=2, mean_e=1.0, max_e=2.0, sigma=1.0, beta=0.5, mean_abs_bonus=0.5, mean_abs_ext=0.1,
                                               loss_before=1.0, loss_after=0.5)))
    assert "curiosity: e 1.0000e+00" in line and curiosity_stats_text(dict(curiosity=dict(steps=0))) == ", curiosity: no rows"


def test_entry_points_declared_bound_exported():
    from cadre_amd import build, hip
    hdr = open(os.path.join(ROOT, "include", "cadre_hip.h")).read()
    L = hip.lib()
    for name in NEW:
        assert hasattr(L, name) and name in hip.SYMBOLS and re.search(r"\bint %s\s*\(" % name, hdr), name
    assert "curiosity.hip" in build.SOURCES
    assert L.cadre_abi_version() == hip.ABI_VERSION == 15                  # entry points only added
    for name in ("N", "BETA", "EXT", "RHO_N", "RHO_MEAN", "RHO_M2", "SIGMA", "KEY", "CTR", "HEAD"):
        assert int(re.search(r"#define CADRE_RND_%s (\d+)" % name, hdr).group(1)) == getattr(hip, "RND_" + name) == getattr(ref, "RND_" + name)
    assert int(re.search(r"#define CADRE_HP_FIELDS (\d+)", hdr).group(1)) == hip.HP_FIELDS == 16      # the block stays as it is
    import ppo_agent.curiosity as shim
    from cadre_amd.curiosity import Curiosity
    assert shim.Curiosity is Curiosity


def test_argument_checks_need_no_device():
    """Every entry point refuses bad sizes on the host (pointers are never dereferenced there)."""
    from cadre_amd import hip
    L, p = hip.lib(), 64
    base = dict(tab=p, N=2, T=5, S=3, ldo=544, D=530, H=128, E=64, row0=0, rows=10, state=p, eps=1e-8, clip=5.0, f=p, g=p, err=p, xh=None,
                h1=None, h2=None, diff=None, stream=None)               # (insertion order = argument order)
    fwd = lambda **o: L.cadre_rnd_forward(*dict(base, **o).values())
    for o in (dict(D=0), dict(D=1025), dict(H=100), dict(H=288), dict(E=16), dict(ldo=529), dict(rows=0), dict(rows=11), dict(row0=-1),
              dict(row0=5, rows=6), dict(clip=0.0), dict(tab=None), dict(err=None), dict(T=0)):
        assert fwd(**o) < 0, o
        assert b"cadre_rnd_forward" in L.cadre_last_error()
    assert L.cadre_rnd_obs_stats(p, 2, 5, 3, 544, 530, 0, p, None) == 0            # update == 0: no launch
    for a in ((None, 2, 5, 3, 544, 530, 1, p, None), (p, 0, 5, 3, 544, 530, 1, p, None), (p, 2, 5, 3, 500, 530, 1, p, None),
              (p, 2, 5, 3, 2048, 1025, 1, p, None)):
        assert L.cadre_rnd_obs_stats(*a) < 0, a
    for a in ((p, 0, 5, p, p, 530, 0.99, 1e-8, 1, None), (p, 2, 5, p, p, 530, 1.5, 1e-8, 1, None), (p, 2, 5, p, p, 530, 0.99, 0.0, 1, None),
              (p, 2, 5, None, p, 530, 0.99, 1e-8, 1, None)):
        assert L.cadre_rnd_reward(*a) < 0, a
    for a in ((p, p, p, p, p, 0, 530, 128, 64, p, p, 100, p, p, p, None), (p, p, p, p, p, 5, 530, 128, 64, p, p, -1, p, p, p, None),
              (p, p, p, p, p, 5, 530, 128, 64, p, p, (1 << 24) + 1, p, p, p, None), (p, p, p, p, p, 5, 530, 96, 40, p, p, 5, p, p, p, None),
              (p, p, p, p, p, 5, 530, 128, 64, p, p, 5, None, p, p, None)):
        assert L.cadre_rnd_backward(*a) < 0, a


def test_towers_are_orthogonal_and_leave_the_global_generator():
    from cadre_amd.curiosity import init_tower, tower_offsets
    torch.manual_seed(5)
    before = torch.get_rng_state().clone()
    gen = torch.Generator()
    gen.manual_seed(11)
    D, H, E = 37, 64, 32
    p = init_tower(D, H, E, gen)
    q = init_tower(D, H, E, gen)
    assert torch.equal(torch.get_rng_state(), before)
    offs, P = tower_offsets(D, H, E)
    assert p.numel() == P == D * H + H + H * H + H + H * E + E and (offs, P) == ref.tower_offsets(D, H, E) and not torch.equal(p, q)
    W1, b1, W2, b2, W3, b3 = ref.unpack(p.numpy(), D, H, E)
    assert not b1.any() and not b2.any() and not b3.any()
    assert np.allclose(W1 @ W1.T, 2.0 * np.eye(D), atol=1e-5)            # [D][H] input-major, D < H: the rows are orthogonal
    assert np.allclose(W2 @ W2.T, 2.0 * np.eye(H), atol=1e-5)
    assert np.allclose(W3.T @ W3, np.eye(E), atol=1e-5)
    gen.manual_seed(11)
    assert torch.equal(init_tower(D, H, E, gen), p)


def test_reference_gradient_against_autograd():
    """The reference's backward pass is the gradient torch.autograd (float64) gives for L = sum m e / max(sum m, 1)."""
    D, R, H, E = 37, 13, 32, 32
    x, (n, mu, M2), f, g = case_inputs(D, R, H, E, 1)
    m = ref.mask(7, 100, R, 0.6)
    assert 0 < m.sum() < R
    fw = ref.forward(x, n, mu, M2, f, g, H, E)
    (grad, _e), _ = ref.backward(fw, g, m, H, E)
    xt = torch.from_numpy(x).double()
    sd = torch.sqrt(torch.from_numpy(M2 / n) + 1e-8)
    xh = torch.clamp((xt - torch.from_numpy(mu)) / sd, -5.0, 5.0)
    pg = torch.from_numpy(np.asarray(g, np.float64)).requires_grad_(True)

    def net(p):
        o, _P = ref.tower_offsets(D, H, E)
        h1 = torch.relu(xh @ p[o[0]:o[1]].view(D, H) + p[o[1]:o[2]])
        h2 = torch.relu(h1 @ p[o[2]:o[3]].view(H, H) + p[o[3]:o[4]])
        return h2 @ p[o[4]:o[5]].view(H, E) + p[o[5]:]
    e = ((net(pg) - net(torch.from_numpy(np.asarray(f, np.float64)))) ** 2).mean(1)
    mt = torch.from_numpy(m.astype(np.float64))
    L = (mt * e).sum() / max(float(mt.sum()), 1.0)
    L.backward()
    assert np.allclose(e.detach().numpy(), fw["err"][0], rtol=1e-12, atol=0)
    assert abs(float(L.detach()) - ref.loss(fw, m)) <= 1e-12 * abs(float(L.detach()))
    scale = np.abs(pg.grad.numpy()).max()
    assert scale > 0 and np.abs(grad - pg.grad.numpy()).max() <= 1e-12 * scale
    (zero, ze), _ = ref.backward(fw, g, np.zeros(R), H, E)
    assert not zero.any() and not ze.any()                               # sum m = 0: exact zeros


def test_chan_merge_of_three_rollouts_against_one_pass():
    """Three successive merges equal numpy's one-pass float64 mean and variance of all rows at rtol 1e-9 (|mean| / std <= 10)."""
    rng = np.random.RandomState(2)
    D = 37
    X = [(rng.randn(r, D) * rng.uniform(0.5, 2.0, D) + rng.uniform(-5.0, 5.0, D)).astype(np.float32) for r in (99, 5, 165)]
    n, mu, M2 = 0.0, np.zeros(D), np.zeros(D)
    for x in X:
        n, mu, M2 = ref.chan_merge(n, mu, M2, x)
    allx = np.concatenate(X).astype(np.float64)
    assert (np.abs(allx.mean(0)) / allx.std(0)).max() <= 10.0
    assert n == 269 and np.allclose(mu, allx.mean(0), rtol=1e-9, atol=0) and np.allclose(M2 / n, allx.var(0), rtol=1e-9, atol=0)
    e, carry = np.abs(rng.randn(3, 7)), np.array([0.0, 1.0, 2.0])
    rho, c = ref.rho_scan(e, carry, 0.9)
    assert np.array_equal(rho[:, 0], 0.9 * carry + e[:, 0]) and np.array_equal(rho[:, 3], 0.9 * rho[:, 2] + e[:, 3])
    assert np.array_equal(c, rho[:, -1])                                 # no reset: the last value is the next rollout's carry


def test_mask_generator_statement():
    """Proportion 1 is all ones, 0 all zeros; the draw depends on key and counter only and a run of draws is a shifted counter."""
    assert ref.mask(3, 0, 257, 1.0).all() and not ref.mask(3, 0, 257, 0.0).any()
    a = ref.mask(3, 50, 4096, 0.25)
    assert abs(a.mean() - 0.25) < 0.03
    assert np.array_equal(ref.mask(3, 60, 100, 0.25), a[10:110]) and not np.array_equal(ref.mask(4, 50, 4096, 0.25), a)
    from cadre_amd.curiosity import mask_threshold
    assert (mask_threshold(1.0), mask_threshold(0.0), mask_threshold(0.25)) == (1 << 24, 0, 1 << 22)


@pytest.mark.parametrize("D,R,H,E,seed", PARITY_CASES)
def test_relu_ambiguity_cap(D, R, H, E, seed):
    """The condition of the GPU parity tests, from the reference alone: at most 2 % of the units of a layer lie within their own
    error bound of zero in the tests' inputs (clipped unit normals, orthogonal weights)."""
    x, (n, mu, M2), f, g = case_inputs(D, R, H, E, seed)
    fw = ref.forward(x, n, mu, M2, f, g, H, E)
    amb = ref.ambiguity(fw)
    print("ambiguous units D=%d R=%d: %s" % (D, R, amb))
    assert max(amb.values()) <= AMBIGUITY_CAP
    assert np.isfinite(fw["err"][0]).all() and (fw["err"][0] > 0).all() and np.isfinite(fw["err"][1]).all()
