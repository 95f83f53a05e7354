"""CPU: the PPG auxiliary phase without a device — exports and rejection paths of cadre_aux_record / cadre_aux_loss, the
float64 reference of tests/phasic_ref.py against closed forms, and the host logic of cadre_amd.phasic (train_cfg["aux_phase"],
the stateless permutation, the interval rule, the buffer's slot arithmetic)."""
import ctypes
import math
import os
import re
import types

import numpy as np
import pytest
import torch

from tests import phasic_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------- C ABI
def test_entry_points_are_exported_and_bound():
    from cadre_amd import hip
    L = ctypes.CDLL(hip.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "cadre_hip.h")).read()
    for name in ("cadre_aux_record", "cadre_aux_loss"):
        assert hasattr(L, name) and name in hip.SYMBOLS and re.search(r"\bint %s\s*\(" % name, hdr), name
    assert len(hip.SYMBOLS["cadre_aux_record"]) == 14 and len(hip.SYMBOLS["cadre_aux_loss"]) == 29
    assert hip.lib().cadre_abi_version() == hip.ABI_VERSION == 15          # entry points are only added
    assert hip.AUX_STATS_FIELDS == 6 and "#define CADRE_AUX_STATS_FIELDS 6" in hdr
    src = open(os.path.join(ROOT, "cadre_amd", "build.py")).read()
    assert '"phasic.hip"' in src
    from ppo_agent import phasic as shim
    from cadre_amd import phasic
    assert shim.aux_phase is phasic.aux_phase and shim.AuxBuffer is phasic.AuxBuffer and shim.aux_config is phasic.aux_config


def record_args(**kw):
    """A well-formed argument list of cadre_aux_record (fake non-NULL pointers: nothing is launched on a rejection)."""
    a = dict(logits=16, ldl=64, l_ns=64, commands=16, pos=None, row_id=16, B=1, C=4, nS=33, nT=3, ord=None, table=16, R=8,
             stream=None)
    a.update(kw)
    return tuple(a.values())


def loss_args(**kw):
    a = dict(logits=16, ldl=64, l_ns=64, values=16, ldv=1, v_ns=1, commands=16, returns=16, pos=None, row_id=16, table=16, R=8,
             B=1, C=4, nS=33, nT=3, beta=1.0, vc=1.0, inv_b=1.0, losses=16, dl=16, dv=16, scratch=16, poison=None, stats=None,
             F=0, sscr=None, ord=None, stream=None)
    a.update(kw)
    return tuple(a.values())


SHAPE_REJECTIONS = [
    (dict(B=0), b"bad argument"), (dict(B=-3), b"bad argument"), (dict(C=0), b"bad argument"), (dict(nS=0), b"bad argument"),
    (dict(nS=65), b"bad argument"), (dict(nT=0), b"bad argument"), (dict(nT=65), b"bad argument"), (dict(ldl=32), b"bad argument"),
    (dict(ldl=2), b"bad argument"), (dict(ldl=128), b"bad argument"), (dict(logits=None), b"bad argument"),
    (dict(commands=None), b"bad argument"), (dict(row_id=None), b"bad argument"), (dict(table=None), b"bad argument"),
    (dict(R=0), b"R >= 1"), (dict(R=-1), b"R >= 1"),
]


@pytest.mark.parametrize("bad,msg", SHAPE_REJECTIONS)
def test_aux_record_rejections_launch_nothing(bad, msg):
    from cadre_amd import hip
    L = hip.lib()
    assert L.cadre_aux_record(*record_args(**bad)) == -1
    err = L.cadre_last_error()
    assert b"cadre_aux_record" in err and msg in err, err


@pytest.mark.parametrize("bad,msg", SHAPE_REJECTIONS + [
    (dict(values=None), b"bad argument"), (dict(returns=None), b"bad argument"), (dict(losses=None), b"bad argument"),
    (dict(dl=None), b"bad argument"), (dict(dv=None), b"bad argument"), (dict(scratch=None), b"bad argument"),
    (dict(stats=16, F=5, sscr=16), b"stats"), (dict(stats=16, F=6, sscr=None), b"stats"),
])
def test_aux_loss_rejections_launch_nothing(bad, msg):
    from cadre_amd import hip
    L = hip.lib()
    assert L.cadre_aux_loss(*loss_args(**bad)) == -1
    err = L.cadre_last_error()
    assert b"cadre_aux_loss" in err and msg in err, err


# ----------------------------------------------------------------------------- the float64 reference
def ref_case(B=9, C=3, K=(33, 3), seed=0, R=None):
    g = torch.Generator().manual_seed(seed)
    R = 3 * B if R is None else R
    logits = torch.randn(2 * C, B, 64, generator=g, dtype=torch.float64).requires_grad_(True)
    values = torch.randn(2 * C, B, generator=g, dtype=torch.float64).requires_grad_(True)
    cmds = torch.randint(0, C, (2, B), generator=g)
    rets = torch.randn(2, B, generator=g, dtype=torch.float64)
    row_id = torch.stack([torch.randperm(R, generator=g)[:B] for _ in range(2)])
    table = torch.full((2, R, 64), float("-inf"), dtype=torch.float64)
    for hd in range(2):
        table[hd, :, :K[hd]] = torch.log_softmax(torch.randn(R, K[hd], generator=g, dtype=torch.float64), -1)
    return logits, values, cmds, rets, table, row_id


def test_reference_kl_with_itself_is_exactly_zero_with_zero_gradient():
    B, C, K = 9, 3, (33, 3)
    logits, values, cmds, rets, table, row_id = ref_case(B, C, K)
    for pos in (None, torch.stack([torch.randperm(B, generator=torch.Generator().manual_seed(4)) for _ in range(2)])):
        for ranks in ((None, None), (list(range(32, -1, -1)), [2, 0, 1])):
            own = phasic_ref.record(logits, cmds, row_id, pos, K, ranks, C, torch.zeros(2, 3 * B, 64, dtype=torch.float64))
            # the reference's p_old is softmax(lo) and its p is exp(lgn): at lo == lgn the KL is a sum of p * 0
            tv, tk, total, stats = phasic_ref.aux_loss(logits, values, cmds, rets, own, row_id, pos, K, ranks, C, 1.0, 0.0, 1.0 / B)
            assert float(tk.detach()) == 0.0 and float(tv.detach()) == 0.0 and float(stats[:, 1].abs().max()) == 0.0
            logits.grad = values.grad = None
            total.backward()
            # (autograd's p and the reference's softmax(lo) are two float64 roundings of one number: zero to a few ulp)
            assert float(logits.grad.abs().max()) < 1e-15 and float(values.grad.abs().max()) == 0.0
            assert torch.equal(stats[:, 5], torch.ones(2, dtype=torch.float64))


def test_reference_record_writes_log_softmax_and_minus_inf():
    B, C, K = 5, 2, (4, 3)
    logits, _v, cmds, _r, _t, row_id = ref_case(B, C, K, seed=2)
    sentinel = 7.0
    table = phasic_ref.record(logits, cmds, row_id, None, K, (None, None), C, torch.full((2, 3 * B, 64), sentinel, dtype=torch.float64))
    for hd in range(2):
        for u in range(B):
            r, c = int(row_id[hd, u]), int(cmds[hd, u])
            want = torch.log_softmax(logits.detach()[hd * C + c, u, :K[hd]], -1)
            assert float((table[hd, r, :K[hd]] - want).abs().max()) < 1e-15
            assert bool(torch.isinf(table[hd, r, K[hd]:]).all()) and float(table[hd, r, K[hd]]) < 0
        untouched = torch.ones(3 * B, dtype=torch.bool)
        untouched[row_id[hd]] = False
        assert float((table[hd, untouched] - sentinel).abs().max()) == 0.0


def test_reference_uniform_against_one_hot_ish_closed_forms():
    """Current policy uniform over K bins, stored policy (1 - e) on bin 0 and e / (K - 1) elsewhere:
    KL(old || uniform) = log K - H(old) = log K + (1 - e) log(1 - e) + e log(e / (K - 1)); and the other way round,
    stored uniform against the current one-hot-ish policy: KL(uniform || cur) = -log K - mean log cur."""
    K, e, C, B = 5, 0.2, 1, 1
    old = torch.full((K,), e / (K - 1), dtype=torch.float64)
    old[0] = 1.0 - e
    table = torch.full((2, 1, 64), float("-inf"), dtype=torch.float64)
    table[:, 0, :K] = old.log()
    logits = torch.zeros(2, 1, 64, dtype=torch.float64, requires_grad=True)
    values = torch.zeros(2, 1, dtype=torch.float64, requires_grad=True)
    z = torch.zeros(2, 1, dtype=torch.int64)
    _tv, tk, _t, stats = phasic_ref.aux_loss(logits, values, z, z.double(), table, z, None, (K, K), (None, None), C, 1.0, 0.0, 0.5)
    want = math.log(K) + (1 - e) * math.log(1 - e) + e * math.log(e / (K - 1))
    assert abs(float(tk.detach()) - want) < 1e-14 and abs(float(stats[0, 0]) - 0.5 * want) < 1e-14     # two heads x inv_b 0.5
    assert abs(float(stats[0, 1]) - want) < 1e-14 and abs(float(stats[0, 3]) - 0.5 * math.log(K)) < 1e-14
    table[:, 0, :K] = -math.log(K)
    lg = torch.zeros(2, 1, 64, dtype=torch.float64)
    lg[:, 0, :K] = old.log()
    lg.requires_grad_(True)
    _tv, tk, _t, _s = phasic_ref.aux_loss(lg, values, z, z.double(), table, z, None, (K, K), (None, None), C, 1.0, 0.0, 0.5)
    want2 = -math.log(K) - float(old.log().mean())
    assert abs(float(tk.detach()) - want2) < 1e-14
    # a stored bin of probability exactly 0 adds nothing (no 0 * inf)
    table[:, 0, 1] = float("-inf")
    table[:, 0, :K] = torch.log_softmax(table[0, 0, :K], -1)
    _tv, tk, _t, _s = phasic_ref.aux_loss(lg, values, z, z.double(), table, z, None, (K, K), (None, None), C, 1.0, 0.0, 0.5)
    assert math.isfinite(float(tk.detach()))


def test_reference_gradient_is_beta_inv_b_p_minus_p_old_and_value_term():
    B, C, K = 7, 2, (5, 3)
    logits, values, cmds, rets, table, row_id = ref_case(B, C, K, seed=3)
    pos = torch.stack([torch.randperm(B, generator=torch.Generator().manual_seed(6)) for _ in range(2)])
    beta, vc, inv_b = 0.7, 0.3, 1.0 / B
    cmds[0, 2], row_id[1, 4] = C, 3 * B                               # one bad command, one row_id past the table: counted out
    tv, tk, total, stats = phasic_ref.aux_loss(logits, values, cmds, rets, table, row_id, pos, K, (None, None), C, beta, vc, inv_b)
    total.backward()
    sq = 0.0
    for hd in range(2):
        counted = 0
        for u in range(B):
            b = int(pos[hd, u])
            c, r = int(cmds[hd, b]), int(row_id[hd, u])
            if not (0 <= c < C and 0 <= r < 3 * B):
                assert float(logits.grad[hd * C:(hd + 1) * C, b].abs().max()) == 0.0
                assert float(values.grad[hd * C:(hd + 1) * C, b].abs().max()) == 0.0
                continue
            counted += 1
            net = hd * C + c
            p = torch.softmax(logits.detach()[net, b, :K[hd]], -1)
            want = beta * inv_b * (p - table[hd, r, :K[hd]].exp())
            assert float((logits.grad[net, b, :K[hd]] - want).abs().max()) < 1e-15
            assert float(logits.grad[net, b, K[hd]:].abs().max()) == 0.0
            dv = float(values.detach()[net, b] - rets[hd, b])
            assert abs(float(values.grad[net, b]) - vc * inv_b * dv) < 1e-15
            sq += dv * dv
        assert float(stats[hd, 5]) == counted * inv_b and counted == B - 1
    assert abs(float(tv.detach()) - vc * 0.5 * sq * inv_b) < 1e-14       # the value term: vc * 0.5 * mean (v - R)^2


# ----------------------------------------------------------------------------- train_cfg["aux_phase"]
def test_aux_config_acceptance_and_refusals():
    from cadre_amd.phasic import aux_config
    assert aux_config(None) is None
    assert aux_config(dict(interval=4)) == dict(interval=4, epochs=2, minibatch=None, beta_clone=1.0, value_coeff=1.0, seed=0)
    full = dict(interval=np.int64(2), epochs=3, minibatch=32, beta_clone=0, value_coeff=0.5, seed=-7)
    assert aux_config(full) == dict(interval=2, epochs=3, minibatch=32, beta_clone=0.0, value_coeff=0.5, seed=-7)
    for bad in ("on", 4, dict(), dict(epochs=2), dict(interval=0), dict(interval=-1), dict(interval=1.0), dict(interval=True),
                dict(interval=2, epochs=-1), dict(interval=2, epochs=1.5), dict(interval=2, minibatch=0),
                dict(interval=2, minibatch=16.0), dict(interval=2, beta_clone=float("nan")), dict(interval=2, beta_clone="1"),
                dict(interval=2, value_coeff=float("inf")), dict(interval=2, value_coeff=True), dict(interval=2, seed=0.5),
                dict(interval=2, lr=1e-3), dict(interval=2, intervall=2)):
        with pytest.raises(ValueError, match="aux_phase"):
            aux_config(bad)


def test_the_permutation_is_a_pure_function_of_its_key_and_leaves_the_global_generator_alone():
    from cadre_amd.phasic import epoch_permutation
    torch.manual_seed(123)
    before = torch.get_rng_state().clone()
    a = epoch_permutation(0, 0, 3, 1, 32, 128)
    b = epoch_permutation(0, 0, 3, 1, 32, 128)
    assert torch.equal(torch.get_rng_state(), before)
    assert torch.equal(a, b) and torch.equal(a.sort().values, torch.arange(128)) and a.dtype == torch.int64
    seen = {tuple(a.tolist())}
    for key in ((1, 0, 3, 1, 32, 128), (0, 1, 3, 1, 32, 128), (0, 0, 4, 1, 32, 128), (0, 0, 3, 0, 32, 128), (0, 0, 3, 1, 16, 128)):
        seen.add(tuple(epoch_permutation(*key).tolist()))
    assert len(seen) == 6                                              # every field of the key moves the draw
    assert epoch_permutation(-1, 0, 0, 0, 1, 5).numel() == 5           # a negative seed is a valid key
    with pytest.raises(ValueError):
        epoch_permutation(0, 0, -1, 0, 32, 128)
    torch.manual_seed(123)
    want = torch.randperm(10)
    torch.manual_seed(123)
    epoch_permutation(5, 0, 0, 0, 2, 10)
    assert torch.equal(torch.randperm(10), want)                       # the PPO sampler's next draw is what it would have been


def test_the_checkpoint_interval_rule_and_the_start_up_refusals():
    from cadre_amd import hip
    from cadre_amd.phasic import aux_runner, check_intervals
    check_intervals(2, None)
    check_intervals(2, 4)
    check_intervals(2, 2, first_episode=6)
    check_intervals(1, 3, first_episode=5)
    with pytest.raises(ValueError, match="checkpoint_interval 3 is not a multiple of interval 2"):
        check_intervals(2, 3)
    with pytest.raises(ValueError, match="resumes at episode 3"):
        check_intervals(2, 4, first_episode=3)
    agent = object()
    assert aux_runner(agent, None) is None
    sgb = types.SimpleNamespace(dist_world=lambda: 0)
    run = aux_runner(agent, dict(interval=2), sgb, checkpoint_interval=4)
    assert run.cfg["interval"] == 2 and run.buffer is None             # nothing is allocated before the first rollout
    with pytest.raises(ValueError, match="multiple"):
        aux_runner(agent, dict(interval=2), sgb, checkpoint_interval=3)
    with pytest.raises(hip.CadreHipError, match="in-process chief"):
        aux_runner(agent, dict(interval=2), sgb, in_process_chief=False)
    with pytest.raises(hip.CadreHipError, match="single rank"):
        aux_runner(agent, dict(interval=2), types.SimpleNamespace(dist_world=lambda: 2))


# ----------------------------------------------------------------------------- the buffer
def test_record_pass_minibatches_cover_every_row():
    from cadre_amd.phasic import record_starts, slot_rows
    assert record_starts(128, 32) == [0, 32, 64, 96]
    assert record_starts(100, 32) == [0, 32, 64, 68]                   # the last minibatch is the last B rows
    assert record_starts(32, 32) == [0] and record_starts(33, 32) == [0, 1]
    for R, B in ((7, 3), (64, 64), (65, 64), (10, 1)):
        cover = set()
        for lo in record_starts(R, B):
            assert 0 <= lo and lo + B <= R
            cover.update(range(lo, lo + B))
        assert cover == set(range(R))
    with pytest.raises(ValueError):
        record_starts(16, 32)                                          # B > R
    with pytest.raises(ValueError):
        record_starts(16, 0)
    assert slot_rows(0, 16) == (0, 16) and slot_rows(2, 16) == (32, 48)


def test_aux_buffer_slot_arithmetic_on_the_host():
    from cadre_amd.phasic import AuxBuffer
    from ppo_agent.storage import RolloutStorage
    agent = types.SimpleNamespace(lstm_input=530, learner=types.SimpleNamespace(S=8), arena=types.SimpleNamespace(device="cpu"))
    T, N, slots = 4, 2, 3
    buf = AuxBuffer(agent, slots, N * T, _device="cpu")
    assert buf.R == 24 and buf.table.shape == (2, 24, 64) and buf.throttle._obs is buf.steer._obs and not buf.full
    assert buf.steer.num_steps == 24
    g = torch.Generator().manual_seed(0)

    def rollouts(tag):
        out = []
        for e in range(N):
            pair = tuple(RolloutStorage(T, 1, 530, 8, 530, True, 0.99, 0.95) for _ in range(2))
            obs = torch.randn(T + 1, 8, 530, generator=g)
            for hd, s in enumerate(pair):
                s.obs.copy_(obs)
                s.hn.copy_(torch.randn(T + 1, 530, generator=g))
                s.cn.copy_(torch.randn(T + 1, 530, generator=g))
                s.command[:, 0] = torch.arange(T + 1, dtype=torch.int32) % 4
                s.returns[:, 0] = 100.0 * tag + 10.0 * e + hd + torch.arange(T + 1) / 10.0
            out.append(pair)
        return out
    kept = []
    for tag in range(slots):
        r = rollouts(tag)
        kept.append(r)
        buf.append(r)
        assert buf.filled == tag + 1
    assert buf.full
    with pytest.raises(ValueError, match="filled"):
        buf.append(kept[0])
    for tag in range(slots):
        for e in range(N):
            lo = tag * N * T + e * T
            s, t = kept[tag][e]
            assert torch.equal(buf.steer._obs[lo:lo + T], s._obs[:T])
            for src, dst in ((s, buf.steer), (t, buf.throttle)):
                assert torch.equal(dst._hn[lo:lo + T], src._hn[:T]) and torch.equal(dst._cn[lo:lo + T], src._cn[:T])
                assert torch.equal(dst.command[lo:lo + T], src.command[:T]) and torch.equal(dst.returns[lo:lo + T], src.returns[:T])
    assert float(buf.steer.returns[24]) == 0.0                         # row R (the storages' spare row) is not written
    buf.clear()
    assert not buf.full and buf.filled == 0
    buf.append(kept[2])                                                # after clear() the first slot is rewritten
    assert torch.equal(buf.throttle.returns[:T], kept[2][0][1].returns[:T])
    with pytest.raises(ValueError, match="rows for a slot"):
        buf.append(kept[0][:1])
    ent = buf.entry(torch.arange(3))
    assert len(ent) == 1 and ent[0][0] is buf.steer and ent[0][3] is buf.throttle and torch.equal(ent[0][1], ent[0][4])
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError):
            AuxBuffer(agent, bad, 8, _device="cpu")
