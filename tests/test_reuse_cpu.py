"""CPU: sample reuse without a device — exports and rejection paths of cadre_reuse_record / cadre_vtrace_multi, the reference
arithmetic of tests/reuse_ref.py (the fp32 emulation against the GAE emulation of the rollout-finish tests, against float64,
against hand-checkable cases, and its mutants), and the host logic of cadre_amd.reuse (train_cfg["sample_reuse"], the start-up
refusals, the window's slot rotation, the stateless permutations)."""
import ctypes
import math
import os
import re
import types

import numpy as np
import pytest
import torch

from tests import reuse_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
GAMMA, TAU = 0.99, 0.95                    # (the constants of tests/test_rollout_finish_gpu.py's np_scan)
G32, GT32 = f32(GAMMA), f32(GAMMA * TAU)


# ----------------------------------------------------------------------------- C ABI
def test_entry_points_are_exported_and_bound():
    from cadre_amd import hip
    L = ctypes.CDLL(hip.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "cadre_hip.h")).read()
    for name in ("cadre_reuse_record", "cadre_vtrace_multi"):
        assert hasattr(L, name) and name in hip.SYMBOLS and re.search(r"\bint %s\s*\(" % name, hdr), name
    assert len(hip.SYMBOLS["cadre_reuse_record"]) == 19 and len(hip.SYMBOLS["cadre_vtrace_multi"]) == 11
    assert hip.lib().cadre_abi_version() == hip.ABI_VERSION == 15          # entry points are only added
    assert hip.VTRACE_DIAG_FIELDS == 4 and "#define CADRE_VTRACE_DIAG_FIELDS 4" in hdr
    assert '"reuse.hip"' in open(os.path.join(ROOT, "cadre_amd", "build.py")).read()
    from ppo_agent import reuse as shim
    from cadre_amd import reuse
    assert shim.ReuseWindow is reuse.ReuseWindow and shim.reuse_config is reuse.reuse_config


def record_args(**kw):
    """A well-formed argument list of cadre_reuse_record (fake non-NULL pointers: nothing is launched on a rejection)."""
    a = dict(logits=16, ldl=64, l_ns=64, values=16, ldv=64, v_ns=64, commands=16, actions=16, pos=None, row_id=16, B=1, C=4,
             nS=33, nT=3, ord=None, logp=16, value=16, R=8, stream=None)
    a.update(kw)
    return tuple(a.values())


@pytest.mark.parametrize("bad,msg", [
    (dict(B=0), b"bad argument"), (dict(B=-3), b"bad argument"), (dict(C=0), b"bad argument"), (dict(nS=0), b"bad argument"),
    (dict(nS=65), b"bad argument"), (dict(nT=0), b"bad argument"), (dict(nT=65), b"bad argument"), (dict(ldl=32), b"bad argument"),
    (dict(ldl=2), b"bad argument"), (dict(ldl=128), b"bad argument"), (dict(ldv=0), b"bad argument"),
    (dict(logits=None), b"bad argument"), (dict(values=None), b"bad argument"), (dict(commands=None), b"bad argument"),
    (dict(actions=None), b"bad argument"), (dict(row_id=None), b"bad argument"), (dict(logp=None), b"bad argument"),
    (dict(value=None), b"bad argument"), (dict(R=0), b"R >= 1"), (dict(R=-1), b"R >= 1"),
])
def test_reuse_record_rejections_launch_nothing(bad, msg):
    from cadre_amd import hip
    L = hip.lib()
    assert L.cadre_reuse_record(*record_args(**bad)) == -1
    err = L.cadre_last_error()
    assert b"cadre_reuse_record" in err and msg in err, err


def test_vtrace_multi_rejects_bad_arguments_without_launching():
    from cadre_amd import hip
    L = hip.lib()
    P = 16                                           # fake non-NULL pointer: a rejection dereferences nothing
    good = [P, 8, 128, 0.99, 0.94, 1, None, 0.0, 1.0, 1.0]
    inf, nan = float("inf"), float("nan")
    for i, v, msg in ((0, None, b"null"), (1, 0, b"bad argument"), (1, 65536, b"bad argument"), (2, 1, b"bad argument"),
                      (2, 3001, b"bad argument"), (8, 0.0, b"truncation"), (8, -1.0, b"truncation"), (8, inf, b"truncation"),
                      (8, nan, b"truncation"), (9, 0.0, b"truncation"), (9, -2.0, b"truncation"), (9, inf, b"truncation"),
                      (9, nan, b"truncation")):
        bad = list(good)
        bad[i] = v
        assert L.cadre_vtrace_multi(*bad, None) == -1, (i, v)
        err = L.cadre_last_error()
        assert b"cadre_vtrace_multi" in err and msg in err, (i, v, err)
    for clip in (0.0, -1.0, nan):                    # reward scaling on: clip_r must be positive
        assert L.cadre_vtrace_multi(P, 8, 128, 0.99, 0.94, 1, P, clip, 1.0, 1.0, None) == -1
        assert b"cadre_vtrace_multi" in L.cadre_last_error()


# ----------------------------------------------------------------------------- the reference arithmetic
def case(T, seed, flags=0.0, sd=0.5):
    r = np.random.RandomState(seed)
    rew = (r.rand(T + 1) * 2.0 - 0.5).astype(f32)
    V = (r.randn(T + 1) * 0.3).astype(f32)
    m = (r.rand(T + 1) >= 0.1).astype(f32)
    tl = (r.rand(T + 1) < flags).astype(f32)
    lr = (r.randn(T) * sd).astype(f32)
    return rew, V, m, tl, lr


@pytest.mark.parametrize("T", [2, 3, 63, 64, 65, 130])
@pytest.mark.parametrize("flags", [0.0, 0.2])
def test_on_policy_emulation_is_the_gae_emulation_bit_for_bit(T, flags):
    """ratio == 1 and both bars >= 1: every factor is exactly 1, both chains are the GAE chain."""
    from tests.test_rollout_finish_gpu import np_scan
    rew, V, m, tl, _lr = case(T, 10 + T, flags)
    keep = (f32(1.0) - tl).astype(f32)
    for boot_keep, scale, clip, bars in ((1.0, None, None, (1.0, 1.0)), (0.0, None, None, (2.0, 1.5)), (1.0, 0.37, 0.8, (1.0, 7.0))):
        nv = V[T] if boot_keep else f32(0.0)
        ret, adv, V2 = np_scan(rew, V, m, nv, keep=keep if flags else None, scale=scale, clip=clip)
        got_ret, got_a, got_V, rho = rr.scan32(rew, V, m, keep if flags else None, np.ones(T, f32), boot_keep, G32, GT32,
                                               bars[0], bars[1], scale, clip)
        assert np.array_equal(got_ret.view(np.int32), ret.view(np.int32))
        assert np.array_equal(got_a.view(np.int32), adv.view(np.int32))
        assert np.array_equal(got_V.view(np.int32), V2.view(np.int32)) and (rho == 1).all()
        assert np.array_equal(rr.finish32(got_a, rho, False).view(np.int32), adv.view(np.int32))


def agrees(T, seed, bars, mutant=None, flags=0.2, boot_keep=1.0, normalise=False):
    """The fp32 scan against float64.  A row has at most 12 roundings of at most 2^-24 relative, each on a magnitude of at most
    `mag` (the largest of |V|, |v - V|, |A| and rho |delta| on the float64 side); an earlier row's error is carried on by
    gamma tau m c, the factor that carries the magnitude on, so relative to `mag` the errors add up to at most 12 T 2^-24.
    The last multiply by rho <= rho_max scales that; the normalisation divides by the float64 std and adds the mean's and
    the std's share, each below the raw bound: a factor 3."""
    rew, V, m, tl, lr = case(T, seed, flags)
    keep = (f32(1.0) - tl).astype(f32)
    ratio = np.exp(lr.astype(np.float64)).astype(f32)
    ret, adv, vT = rr.vtrace32(rew, V, m, keep, ratio, boot_keep, G32, GT32, bars[0], bars[1], normalise, mutant=mutant)
    vs, A, rho = rr.vtrace64(rew, V, m, keep, ratio, boot_keep, float(G32), float(GT32) / float(G32), bars[0], bars[1])
    want = rr.finish64(A, rho, normalise)
    V64 = V.astype(np.float64)
    mag = max(1.0, np.abs(V64).max(), np.abs(vs - V64[:T]).max(), np.abs(A).max(), rho.max() * 4.0)      # (|delta| < 4 here)
    tol = 12 * T * 2.0 ** -24 * mag
    tol_a = tol * rho.max() * (3.0 / A.std(ddof=1) if normalise else 1.0)
    return bool(np.abs(ret - vs).max() <= tol and np.abs(adv - want).max() <= tol_a)


@pytest.mark.parametrize("bars", [(1.0, 1.0), (2.0, 0.5), (1e6, 1e6)])
@pytest.mark.parametrize("normalise", [False, True])
def test_emulation_agrees_with_the_float64_recursion(bars, normalise):
    for T, seed in ((2, 1), (17, 2), (64, 3), (130, 4)):
        for boot_keep in (1.0, 0.0):
            assert agrees(T, seed, bars, boot_keep=boot_keep, normalise=normalise)


@pytest.mark.parametrize("mutant", ["rho_twice", "no_cw", "keep_one_chain"])
def test_mutants_of_the_scan_fail_the_float64_check(mutant):
    assert agrees(130, 4, (2.0, 0.5))
    assert not agrees(130, 4, (2.0, 0.5), mutant=mutant)


def test_the_bootstrap_is_a_select_not_a_product():
    """boot_keep = 0 with a negative V[T]: the select stores +0, the product -0 — other bits, and other bits downstream
    wherever the zero's sign survives."""
    rew, V, m, tl, lr = case(8, 5)
    V[8] = f32(-0.75)
    ones = np.ones(8, f32)
    _r, _a, V_sel, _ = rr.scan32(rew, V, m, None, ones, 0.0, G32, GT32, 1.0, 1.0)
    _r, _a, V_mul, _ = rr.scan32(rew, V, m, None, ones, 0.0, G32, GT32, 1.0, 1.0, mutant="boot_product")
    assert V_sel[8] == 0 and V_mul[8] == 0
    assert V_sel[8:].view(np.int32)[0] == 0 and V_mul[8:].view(np.int32)[0] != 0
    assert not np.array_equal(V_sel.view(np.int32), V_mul.view(np.int32))


def test_float64_vtrace_two_rows_by_hand():
    g, lam = 0.5, 0.5
    r, V, m = [1.0, 2.0, 0.0], [0.5, -1.0, 4.0], [1.0, 1.0, 1.0]
    ratio = [3.0, 0.25]                       # rho = (2, 0.25), c = (1, 0.25) at rho_bar 2, c_bar 1
    vs, A, rho = rr.vtrace64(r, V, m, None, ratio, 1.0, g, lam, 2.0, 1.0)
    d1 = 2.0 + 0.5 * 4.0 + 1.0                # 5
    d0 = 1.0 + 0.5 * -1.0 - 0.5               # 0
    n1 = 0.25 * d1                            # v_1 - V_1 = 1.25
    n0 = 2.0 * d0 + 0.25 * 1.0 * n1           # gamma lam c_0 (v_1 - V_1) = 0.3125
    assert vs.tolist() == [0.5 + n0, -1.0 + n1] and rho.tolist() == [2.0, 0.25]
    assert A.tolist() == [d0 + 0.25 * n1, d1]
    # a finished rollout bootstraps from zero
    vs0, A0, _ = rr.vtrace64(r, V, m, None, ratio, 0.0, g, lam, 2.0, 1.0)
    assert A0[1] == 2.0 + 1.0 and vs0[1] == -1.0 + 0.25 * 3.0


def test_float64_vtrace_without_truncation_is_the_importance_weighted_monte_carlo_return():
    T, g = 12, 0.9
    rew, V, m, _tl, lr = case(T, 7)
    m = np.ones(T + 1)
    w = np.exp(lr.astype(np.float64))
    vs, A, rho = rr.vtrace64(rew, V, m, None, w, 1.0, g, 1.0, math.inf, math.inf)
    V64, r64 = V.astype(np.float64), rew.astype(np.float64)
    delta = r64[:T] + g * V64[1:] - V64[:T]
    for s in range(T):
        want = V64[s] + sum(g ** (t - s) * np.prod(w[s:t + 1]) * delta[t] for t in range(s, T))
        assert abs(vs[s] - want) < 1e-12 * max(1.0, abs(want))
    assert np.array_equal(rho, w)


def test_a_cut_row_returns_its_value_and_has_no_advantage():
    T = 9
    rew, V, m, _tl, lr = case(T, 8)
    tl = np.zeros(T + 1, f32)
    tl[4] = 1.0
    keep = (f32(1.0) - tl).astype(f32)
    ratio = np.exp(lr.astype(np.float64)).astype(f32)
    vs, A, _ = rr.vtrace64(rew, V, m, keep, ratio, 1.0, 0.99, 0.95, 1.0, 1.0)
    assert vs[4] == float(V[4]) and A[4] == 0.0
    ret, adv, _vT = rr.vtrace32(rew, V, m, keep, ratio, 1.0, G32, GT32, 1.0, 1.0, False)
    assert ret[4] == V[4] and adv[4] == 0.0
    # the chain restarts behind the cut: row 3 sees nothing of rows 4 ..
    rew2, V2 = rew.copy(), V.copy()
    rew2[5:] += f32(3.0)
    V2[5:] -= f32(1.0)
    ret2, adv2, _ = rr.vtrace32(rew2, V2, m, keep, ratio, 1.0, G32, GT32, 1.0, 1.0, False)
    assert np.array_equal(ret2[:4], ret[:4]) and np.array_equal(adv2[:4], adv[:4])


def test_the_shuffle_tree_and_the_diagnostics():
    x = np.random.RandomState(3).randn(130)
    assert abs(rr.wave_sum_d(rr.lane_sums(x)) - x.sum()) < 1e-12
    ones = np.ones(17, f32)
    assert rr.diag64(np.zeros(17, f32), ones, 1.0).tolist() == [1.0, 0.0, 0.0, 1.0]
    d = rr.diag64(np.log(np.array([0.5, 4.0], np.float64)), np.array([0.5, 4.0], f32), 2.0)
    assert d[0] == 2.25 and d[1] == 0.5 and abs(d[2] - math.log(4.0)) < 1e-15 and d[3] == 2.5 ** 2 / (2 * 4.25)


# ----------------------------------------------------------------------------- train_cfg["sample_reuse"]
def test_reuse_config_acceptance_and_refusals():
    from cadre_amd.reuse import reuse_config
    assert reuse_config(None) is None
    assert reuse_config(dict(rollouts=2)) == dict(rollouts=2, rho_bar=1.0, c_bar=1.0, seed=0)
    assert reuse_config(dict(rollouts=np.int64(3), rho_bar=2, c_bar=0.5, seed=-7)) == dict(rollouts=3, rho_bar=2.0, c_bar=0.5, seed=-7)
    for bad in ("on", 2, dict(), dict(rho_bar=1.0), dict(rollouts=0), dict(rollouts=-1), dict(rollouts=1.0), dict(rollouts=True),
                dict(rollouts=2, rho_bar=0.0), dict(rollouts=2, rho_bar=-1.0), dict(rollouts=2, rho_bar=float("inf")),
                dict(rollouts=2, rho_bar=float("nan")), dict(rollouts=2, rho_bar="1"), dict(rollouts=2, c_bar=0),
                dict(rollouts=2, c_bar=True), dict(rollouts=2, c_bar=float("inf")), dict(rollouts=2, seed=0.5),
                dict(rollouts=2, lr=1e-3), dict(rollouts=2, rolouts=2)):
        with pytest.raises(ValueError, match="sample_reuse"):
            reuse_config(bad)


def test_the_start_up_refusals():
    from cadre_amd import hip
    from cadre_amd.reuse import reuse_runner
    agent = object()
    assert reuse_runner(agent, None) is None
    assert reuse_runner(agent, None, checkpoint_interval=4, fused_gather=False) is None       # key absent: nothing is checked
    sgb = types.SimpleNamespace(dist_world=lambda: 0)
    run = reuse_runner(agent, dict(rollouts=2), sgb)
    assert run.cfg["rollouts"] == 2 and run.window is None              # nothing is allocated before the first section
    with pytest.raises(hip.CadreHipError, match="in-process chief"):
        reuse_runner(agent, dict(rollouts=2), sgb, in_process_chief=False)
    with pytest.raises(hip.CadreHipError, match="single rank"):
        reuse_runner(agent, dict(rollouts=2), types.SimpleNamespace(dist_world=lambda: 2))
    with pytest.raises(ValueError, match="fused_gather"):
        reuse_runner(agent, dict(rollouts=2), sgb, fused_gather=False)
    with pytest.raises(ValueError, match="checkpoint"):
        reuse_runner(agent, dict(rollouts=2), sgb, checkpoint_interval=4)
    with pytest.raises(ValueError, match="checkpoint"):
        reuse_runner(agent, dict(rollouts=2), sgb, resume_from="ckpt_3.pt")
    with pytest.raises(ValueError, match="sample_reuse"):
        reuse_runner(agent, dict(rollouts=0), sgb)


def test_the_sections_refuse_a_window_on_the_tuple_path():
    from ppo_agent.train import learner_section
    with pytest.raises(ValueError, match="fused_gather"):
        learner_section(None, None, None, False, {}, None, fused_gather=False, reuse=object())
    with pytest.raises(ValueError, match="in-process chief"):
        learner_section(None, None, None, False, {}, None, in_process_chief=False, reuse=object())


def test_stats_line_appends_the_reuse_fields():
    from ppo_agent.train import stats_line
    rows = [dict(approx_kl=(0.1, 0.2), clip_fraction=(0.0, 0.5), grad_norm=[1.0, 2.0])]
    base = dict(rows=rows, explained_variance=[(0.5, 0.25)], updates_applied=1, steps=1)
    plain = stats_line(3, base)
    assert "reuse" not in plain
    line = stats_line(3, dict(base, reuse=dict(filled=2, ratio_mean=(1.01, 0.99), truncated=(0.25, 0.5),
                                                max_abs_log_ratio=(0.3, 0.2), effective_sample_share=(0.9, 0.8))))
    assert line.startswith(plain) and "reuse: 2 rollouts, ratio: 1.0100/0.9900, truncated: 0.2500/0.5000" in line
    assert "max |log ratio|: 0.3000/0.2000, effective samples: 0.9000/0.8000" in line
    assert stats_line(3, dict(base, reuse=dict(filled=0))).endswith("reuse: 0 rollouts")


# ----------------------------------------------------------------------------- the window
def test_the_permutations_are_pure_functions_of_their_key_and_leave_the_global_generator_alone():
    from cadre_amd.reuse import reuse_permutation
    torch.manual_seed(123)
    before = torch.get_rng_state().clone()
    a = reuse_permutation(0, 0, 3, 1, 0, 2, 128)
    b = reuse_permutation(0, 0, 3, 1, 0, 2, 128)
    assert torch.equal(torch.get_rng_state(), before)
    assert torch.equal(a, b) and torch.equal(a.sort().values, torch.arange(128)) and a.dtype == torch.int64
    seen = {tuple(a.tolist())}
    for key in ((1, 0, 3, 1, 0, 2, 128), (0, 1, 3, 1, 0, 2, 128), (0, 0, 4, 1, 0, 2, 128), (0, 0, 3, 0, 0, 2, 128),
                (0, 0, 3, 1, 1, 2, 128), (0, 0, 3, 1, 0, 3, 128)):
        seen.add(tuple(reuse_permutation(*key).tolist()))
    assert len(seen) == 7                                              # every field of the key moves the draw
    assert reuse_permutation(-1, 0, 0, 0, 0, 0, 5).numel() == 5        # a negative seed is a valid key
    with pytest.raises(ValueError):
        reuse_permutation(0, 0, -1, 0, 0, 0, 128)


def stand_in_agent():
    return types.SimpleNamespace(lstm_input=530, learner=types.SimpleNamespace(S=8), arena=types.SimpleNamespace(device="cpu"))


def make_rollouts(T, N, tag, g):
    from ppo_agent.storage import RolloutStorage
    out = []
    for e in range(N):
        pair = tuple(RolloutStorage(T, 2, 530, 8, 530, True, 0.99, 0.95) for _ in range(2))
        obs = torch.randn(T + 1, 8, 530, generator=g)
        for hd, s in enumerate(pair):
            s.obs.copy_(obs)
            s.hn.copy_(torch.randn(T + 1, 530, generator=g))
            s.cn.copy_(torch.randn(T + 1, 530, generator=g))
            s.command[:, 0] = torch.arange(T + 1, dtype=torch.int32) % 4
            s.action[:, 0] = (torch.arange(T + 1) + hd + tag) % 3
            base = 100.0 * tag + 10.0 * e + hd
            s.rewards[:, 0] = base + torch.arange(T + 1) / 10.0
            s.action_log_probs[:, 0] = -base - torch.arange(T + 1) / 10.0
            s.masks[:, 0] = (torch.arange(T + 1) % 3 != 0).float()
            s.time_limits[:, 0] = (torch.arange(T + 1) % 4 == 1).float()
        out.append(pair)
    return out


def test_window_slot_rotation_on_the_host():
    from cadre_amd.reuse import ReuseWindow
    T, N, M = 4, 2, 2
    P = T + 1
    win = ReuseWindow(stand_in_agent(), M, N, T, _device="cpu")
    assert win.R == M * N * P and win.throttle._obs is win.steer._obs and win.filled == 0
    assert win.steer.action_log_probs.data_ptr() == win.logp_now[0].data_ptr()
    assert win.throttle.value_preds.data_ptr() == win.value_now[1].data_ptr()
    assert win.entries(0, 0, 0, 2) == [] and win.summary() == dict(filled=0)
    win.refresh(True)                                                  # empty: a no-op, no device needed
    g = torch.Generator().manual_seed(0)
    kept = [make_rollouts(T, N, tag, g) for tag in range(3)]

    def holds(slot, roll, dones):
        for e in range(N):
            lo = win.base(slot, e)
            s, t = roll[e]
            assert torch.equal(win.steer._obs[lo:lo + P], s._obs)                      # all T + 1 rows, the bootstrap row included
            for h, (src, dst) in enumerate(((s, win.steer), (t, win.throttle))):
                for name in ("_hn", "_cn", "command", "action", "rewards", "masks", "time_limits"):
                    assert torch.equal(getattr(dst, name)[lo:lo + P], getattr(src, name)), name
                assert torch.equal(win.mu[h, lo:lo + P], src.action_log_probs)
            assert float(win.boot_keep[slot * N + e]) == (0.0 if dones[e] else 1.0)

    win.append(kept[0], [False, True])
    assert (win.filled, win.next) == (1, 1)
    holds(0, kept[0], [False, True])
    win.append(kept[1], [True, False])
    assert (win.filled, win.next) == (2, 0)
    holds(0, kept[0], [False, True]); holds(1, kept[1], [True, False])
    win.append(kept[2], [False, False])                                 # the oldest slot is overwritten
    assert (win.filled, win.next) == (2, 1)
    holds(0, kept[2], [False, False]); holds(1, kept[1], [True, False])
    assert float(win.steer.rewards[win.R]) == 0.0                      # the big storages' spare row is not written
    assert (win.gamma, win.tau) == (0.99, 0.95)
    with pytest.raises(ValueError, match="environments"):
        win.append(kept[0][:1], [False])
    for bad in (dict(rollouts=0), dict(rollouts=True), dict(num_envs=0), dict(num_steps=1), dict(rho_bar=0.0),
                dict(c_bar=float("inf")), dict(seed=0.5)):
        kw = dict(rollouts=2, num_envs=1, num_steps=4)
        kw.update(bad)
        with pytest.raises(ValueError, match="ReuseWindow"):
            ReuseWindow(stand_in_agent(), _device="cpu", **kw)


def test_window_entries_cut_private_permutations_and_leave_the_global_generator_alone():
    from cadre_amd.reuse import ReuseWindow, reuse_permutation
    T, N, M, Bw = 8, 2, 2, 4
    win = ReuseWindow(stand_in_agent(), M, N, T, seed=5, _device="cpu")
    g = torch.Generator().manual_seed(1)
    win.append(make_rollouts(T, N, 0, g), [False, False])
    torch.manual_seed(9)
    before = torch.get_rng_state().clone()
    ent = [win.entries(3, 1, j, Bw) for j in range(T // Bw)]
    again = [win.entries(3, 1, j, Bw) for j in range(T // Bw)]
    assert torch.equal(torch.get_rng_state(), before)
    assert all(len(e) == N for e in ent)                                # one entry per stale storage pair
    for e in range(N):
        for h, k in ((0, 1), (1, 4)):                                   # (head, position of its index vector in an entry)
            rows = torch.cat([ent[j][e][k] for j in range(T // Bw)])
            assert torch.equal(rows, torch.cat([again[j][e][k] for j in range(T // Bw)]))
            want = reuse_permutation(5, 0, 3, 1, 0, 2 * e + h, T) + win.base(0, e)
            assert torch.equal(rows, want)                              # the whole permutation, cut in order, bootstrap row never drawn
            assert ent[0][e][0] is win.steer and ent[0][e][3] is win.throttle and ent[0][e][2] is win.steer.advantages
    assert not torch.equal(win.entries(3, 2, 0, Bw)[0][1], ent[0][0][1])
    win.append(make_rollouts(T, N, 1, g), [False, True])
    assert len(win.entries(4, 0, 0, Bw)) == 2 * N
    with pytest.raises(ValueError, match="entries"):
        win.entries(4, 0, 2, Bw)                                        # past the storage's rows
    batches = win.record_batches()
    assert torch.equal(torch.cat(batches).unique(), torch.arange(win.rows_filled())) and all(b.numel() == batches[0].numel() for b in batches)
