"""CPU: rank consensus (train_cfg["rank_consensus"]) — the host mirrors of the two kernels against their definitions, the
argument checks of the two entry points (before any HIP call), and over gloo with two ranks: the three refusals lifted by
the key, all_reduce_small, and the refusals that stay."""
import ctypes
import os
import re
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import consensus_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


# ----------------------------------------------------------------------------- the mirrors
def test_kl_rule_mirror_decision_table():
    """Every case of the table against the outcome written out by hand (stop after, applied, lr after)."""
    want = {
        "just below 1.5 target": (0, 1.0, ref.LR0),
        "exactly at 1.5 target (strict >)": (0, 1.0, ref.LR0),
        "just above 1.5 target": (1, 0.0, ref.LR0),
        "above, throttle head": (1, 0.0, ref.LR0),
        "flag already set: stays set, lr untouched": (1, 0.0, ref.LR0),
        "flag already set, kl far above 2 desired": (1, 0.0, ref.LR0),
        "target 0: no check": (0, 1.0, ref.LR0),
        "target 0 without a flag": (0, 1.0, ref.LR_MIN),
        "desired 0: lr stays": (0, 1.0, ref.LR0),
        "kl > 2 desired: lr / factor": (0, 1.0, 3.9e-4 / 1.5),
        "kl > 2 desired: down to lr_min": (0, 1.0, ref.LR_MIN),
        "kl == 2 desired: stays (strict >)": (0, 1.0, ref.LR0),
        "0 < kl < desired / 2: lr * factor": (0, 1.0, 2.6e-4 * 1.5),
        "0 < kl < desired / 2: up to lr_max": (0, 1.0, ref.LR_MAX),
        "kl == 0: stays": (0, 1.0, ref.LR0),
        "negative kl (rounding): stays": (0, 1.0, ref.LR0),
        "NaN in both heads: no stop, lr stays": (0, 1.0, ref.LR0),
        "NaN in one head: the other decides": (1, 0.0, ref.LR0),
        "NaN in one head, small other: lr up": (0, 1.0, 2.6e-4 * 1.5),
        "gate fires and lr would move: lr stays": (1, 0.0, ref.LR0),
    }
    table = ref.decision_table()
    assert sorted(n for n, *_ in table) == sorted(want)
    for name, kl, tkl, stop, desired, lr0 in table:
        got = ref.kl_rule(kl, tkl, stop, desired, ref.hp_block(lr=lr0))
        assert got[0] == want[name][0] and got[1] == want[name][1], (name, got)
        assert got[2] == np.float64(want[name][2]), (name, got)         # (the same float64 operations: exact)
        assert ref.kl_rule(kl, tkl, stop, desired, None) == (got[0], got[1], None)      # (the gate does not depend on the block)
    # the threshold is float32: 1.5f * target_kl, and the comparison is strict
    t = F32(0.02)
    thr = F32(1.5) * t
    assert ref.kl_rule((thr, thr), t, 0, 0.0, None)[0] == 0 and ref.kl_rule((np.nextafter(thr, F32(1)), 0), t, 0, 0.0, None)[0] == 1


def test_chan_mirror_against_numpy_on_concatenated_data():
    """Merged (count, mean, M2) within 1e-12 relative of numpy on the concatenated samples (the bar of
    test_return_statistics_three_rollouts), for world 1, 2 and 5 with empty ranks; an empty head keeps count 0."""
    for world, data in ref.merge_cases().items():
        assert len(data) == world
        got = ref.chan_merge(ref.rank_stats(data))
        for h in range(2):
            x = np.concatenate([np.asarray(p[h], dtype=np.float64) for p in data])
            want = (float(x.size), float(x.mean()), float(((x - x.mean()) ** 2).sum()))
            for g, w in zip(got[3 * h:3 * h + 3], want):
                assert abs(g - w) <= 1e-12 * max(abs(w), 1e-300), (world, h, g, w)
        sc = ref.scale_of(got, 1e-8)
        assert all(s is not None and s.dtype == np.float32 and np.isfinite(s) for s in sc)
    empty = ref.chan_merge(np.zeros((3, 6)))
    assert not empty.any() and ref.scale_of(empty, 1e-8) == [None, None]
    # rank order matters only in the last bits: the reversed order stays within the same bar
    data = ref.merge_cases()[5]
    a, b = ref.chan_merge(ref.rank_stats(data)), ref.chan_merge(ref.rank_stats(data[::-1]))
    assert np.allclose(a, b, rtol=1e-12, atol=0.0)


# ----------------------------------------------------------------------------- the C ABI
def test_consensus_entry_points_declared_bound_exported():
    from cadre_amd import build, hip
    hdr = open(os.path.join(ROOT, "include", "cadre_hip.h")).read()
    declared = set(re.findall(r"\b(cadre_[a-z0-9_]+)\s*\(", hdr))
    L = ctypes.CDLL(hip.LIB_PATH)
    for name in ("cadre_kl_consensus", "cadre_return_scale_merge"):
        assert name in declared and name in hip.SYMBOLS and hasattr(L, name), name
    assert "consensus.hip" in build.SOURCES
    assert hip.lib().cadre_abi_version() == hip.ABI_VERSION == 15
    assert len(re.findall(r"#define CADRE_HP_[A-Z_]+ ", hdr)) == 11           # CADRE_HP_FIELDS + the ten indices: none added


def test_consensus_entry_points_reject_bad_arguments_without_launching():
    from cadre_amd import hip
    L = hip.lib()
    P = 16                                                       # (never dereferenced: rejected before any launch)
    kc = L.cadre_kl_consensus
    assert kc(None, 0.01, P, 0.0, None, None, 0, None) == -1 and b"cadre_kl_consensus" in L.cadre_last_error()
    assert kc(P, -1.0, P, 0.0, None, None, 0, None) == -1                   # negative target_kl
    assert kc(P, float("nan"), P, 0.0, None, None, 0, None) == -1
    assert kc(P, 0.01, None, 0.0, None, None, 0, None) == -1                # gate armed without a flag
    assert b"stop flag" in L.cadre_last_error()
    assert kc(P, 0.0, None, 0.01, None, None, 0, None) == -1                # adaptive lr without the block
    assert b"hyper-parameter block" in L.cadre_last_error()
    assert kc(P, 0.0, None, 0.01, 20, None, 0, None) == -1                  # block not 8-byte aligned
    assert kc(P, 0.01, P, 0.0, None, P, 7, None) == -1                      # F < CADRE_PPO_STATS_FIELDS
    assert b"stats row" in L.cadre_last_error()
    sm = L.cadre_return_scale_merge
    assert sm(None, 2, 1e-8, P, None, None) == -1 and b"cadre_return_scale_merge" in L.cadre_last_error()
    assert sm(P, 2, 1e-8, None, None, None) == -1
    assert sm(P, 0, 1e-8, P, None, None) == -1                              # world < 1
    assert sm(P, -3, 1e-8, P, P, None) == -1
    assert sm(P, 2, -1.0, P, None, None) == -1
    assert sm(P, 2, float("nan"), P, None, None) == -1
    assert sm(P, 2, float("inf"), P, None, None) == -1


# ----------------------------------------------------------------------------- the key on one rank
class _Ranks(object):
    def __init__(self, world, mode="allreduce"):
        self._w, self._m = world, mode

    def dist_world(self):
        return self._w

    def exchange_mode(self):
        return self._m


def test_rank_consensus_key_rules():
    from cadre_amd import hip
    from ppo_agent.train import _adaptive_lr, _check_scaler, _consensus_on, _rank_consensus, _reward_scaling, _target_kl
    from ppo_agent.storage import ReturnScaler
    assert _rank_consensus({}) is False and _rank_consensus({"rank_consensus": None}) is False
    assert _rank_consensus({"rank_consensus": False}) is False and _rank_consensus({"rank_consensus": True}) is True
    for bad in (1, 0, "yes", 1.0, [True]):
        with pytest.raises(ValueError, match="rank_consensus"):
            _rank_consensus({"rank_consensus": bad})
        with pytest.raises(ValueError, match="rank_consensus"):
            _target_kl({"target_kl": 0.02, "rank_consensus": bad}, None)
    on = {"rank_consensus": True, "target_kl": 0.02, "adaptive_lr": {"desired_kl": 0.01}, "reward_scaling": True}
    off = dict(on, rank_consensus=False)
    two = _Ranks(2)
    assert _target_kl(on, two) == 0.02
    assert _adaptive_lr(on, two) == dict(desired_kl=0.01, factor=1.5, lr_min=1e-5, lr_max=1e-2)
    assert _reward_scaling(on, two) == dict(clip=10.0, epsilon=1e-8)
    _check_scaler(ReturnScaler(1, 0.99), two, on)
    for call in (lambda: _target_kl(off, two), lambda: _adaptive_lr(off, two), lambda: _reward_scaling(off, two),
                 lambda: _check_scaler(ReturnScaler(1, 0.99), two, off), lambda: _check_scaler(ReturnScaler(1, 0.99), two)):
        with pytest.raises(hip.CadreHipError, match="single rank"):
            call()
    # the consensus path runs only where an exchange runs
    assert _consensus_on(on, two) and _consensus_on(on, _Ranks(1)) and not _consensus_on(on, _Ranks(0))
    assert not _consensus_on(on, None) and not _consensus_on(off, two)
    for call in (lambda: _target_kl(on, two, in_process_chief=False), lambda: _adaptive_lr(on, two, in_process_chief=False),
                 lambda: _rank_consensus(on, two, in_process_chief=False)):
        with pytest.raises(hip.CadreHipError, match="in-process chief"):
            call()
    for call in (lambda: _target_kl(on, _Ranks(2, "sharded")), lambda: _adaptive_lr(on, _Ranks(2, "sharded")),
                 lambda: _reward_scaling(on, _Ranks(2, "sharded"))):
        with pytest.raises(hip.CadreHipError, match="sharded"):
            call()


# ----------------------------------------------------------------------------- gloo, two ranks
def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    os.environ.pop("CADRE_GRAD_EXCHANGE", None)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    out = {}
    try:
        from cadre_amd import hip
        from cadre_amd.arena import PPOArena
        from ppo_agent.models import Model, Shared_grad_buffers, _no_orthogonal_init
        from ppo_agent.train import _adaptive_lr, _reward_scaling, _target_kl, learner_section, learner_section_multi
        arena = PPOArena("cpu", 530, {"steer": 33, "throttle": 3}, 4)
        with _no_orthogonal_init():
            md = {"steer_ppo_0": arena.bind("steer_ppo_0", Model(530, 33))}
        shared = Shared_grad_buffers(md, torch.device("cpu"))
        on = dict(use_adv_norm=True, ppo_epoch=1, max_grad_norm=250.0, target_kl=0.01, adaptive_lr={"desired_kl": 0.01},
                  reward_scaling={"clip": 5.0}, rank_consensus=True)

        def outcome(call):
            try:
                return ("value", call())
            except hip.CadreHipError as e:
                return ("refused", str(e))
            except Exception as e:                              # noqa: BLE001 (reported to the parent)
                return ("error", repr(e))
        out["with_key"] = [outcome(lambda: _target_kl(on, shared)), outcome(lambda: _adaptive_lr(on, shared)),
                           outcome(lambda: _reward_scaling(on, shared))]
        off = dict(on, rank_consensus=False)
        out["without_key"] = [outcome(lambda: _target_kl(off, shared)), outcome(lambda: _adaptive_lr(off, shared)),
                              outcome(lambda: _reward_scaling(off, shared)),
                              outcome(lambda: learner_section(None, None, None, False, dict(off, adaptive_lr=None), shared)),
                              outcome(lambda: learner_section_multi(None, [], [], dict(off, adaptive_lr=None), shared))]
        out["no_chief"] = [outcome(lambda: _target_kl(on, shared, in_process_chief=False)),
                           outcome(lambda: learner_section(None, None, None, False, on, shared, in_process_chief=False))]
        # all_reduce_small: SUM, in place, the same bits on both ranks; a gather is a sum of rows against zeros
        t = torch.tensor([0.1 * (rank + 1), 1e-3 / 3 * (rank + 2), 0.0, 0.0], dtype=torch.float32)
        shared.all_reduce_small(t)
        g = torch.zeros(world, 6, dtype=torch.float64)
        g[rank] = torch.arange(6, dtype=torch.float64) / 7 + rank
        shared.all_reduce_small(g)
        out["sum"], out["gather"] = t.numpy().tobytes(), g.numpy().tobytes()
        out["non_contiguous"] = outcome(lambda: shared.all_reduce_small(torch.zeros(4, 2)[:, 0]))[0]
        os.environ["CADRE_GRAD_EXCHANGE"] = "sharded"            # (the CPU arena divides into 2 aligned shards)
        out["mode"] = shared.exchange_mode()
        out["sharded"] = [outcome(lambda: _target_kl(on, shared)),
                          outcome(lambda: learner_section_multi(None, [], [], on, shared))]
        q.put((rank, out))
    finally:
        dist.destroy_process_group()


def test_the_key_lifts_the_refusals_with_two_ranks():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(60)
    assert [p.exitcode for p in procs] == [0, 0]
    for r in (0, 1):
        o = res[r]
        assert o["with_key"] == [("value", 0.01), ("value", dict(desired_kl=0.01, factor=1.5, lr_min=1e-5, lr_max=1e-2)),
                                 ("value", dict(clip=5.0, epsilon=1e-8))], o["with_key"]
        assert all(kind == "refused" and "single rank" in msg for kind, msg in o["without_key"]), o["without_key"]
        assert all(kind == "refused" and "in-process chief" in msg for kind, msg in o["no_chief"]), o["no_chief"]
        assert o["mode"] == "sharded"
        assert all(kind == "refused" and "sharded" in msg for kind, msg in o["sharded"]), o["sharded"]
        assert o["non_contiguous"] == "refused"
    assert res[0]["sum"] == res[1]["sum"] and res[0]["gather"] == res[1]["gather"]
    s = np.frombuffer(res[0]["sum"], dtype=np.float32)
    want = np.float32(0.1 * 1) + np.float32(0.1 * 2), np.float32(1e-3 / 3 * 2) + np.float32(1e-3 / 3 * 3)
    assert s[0] == want[0] and s[1] == want[1] and s[2] == 0 and s[3] == 0
    g = np.frombuffer(res[0]["gather"], dtype=np.float64).reshape(2, 6)
    assert np.array_equal(g, np.arange(6, dtype=np.float64) / 7 + np.arange(2, dtype=np.float64)[:, None])


def test_all_reduce_small_is_a_no_op_without_a_process_group():
    from cadre_amd.arena import PPOArena
    from ppo_agent.models import Model, Shared_grad_buffers, _no_orthogonal_init
    arena = PPOArena("cpu", 530, {"steer": 33, "throttle": 3}, 4)
    with _no_orthogonal_init():
        md = {"steer_ppo_0": arena.bind("steer_ppo_0", Model(530, 33))}
    shared = Shared_grad_buffers(md, torch.device("cpu"))
    assert shared.dist_world() == 0
    t = torch.tensor([1.0, 2.0])
    assert shared.all_reduce_small(t) is t and t.tolist() == [1.0, 2.0]
