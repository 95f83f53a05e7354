"""CPU: the rollout-finishing entry points (cadre_return_stats, cadre_gae_multi, cadre_insert_rows_tl) are declared,
exported and reject bad arguments before any HIP call; ReturnScaler validation and state_dict round trip on CPU tensors;
the train_cfg["reward_scaling"] rules and the several-ranks refusal."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cadre_return_stats", "cadre_gae_multi", "cadre_insert_rows_tl")


def test_new_symbols_declared_and_exported():
    from cadre_amd import build, hip
    hdr = open(os.path.join(ROOT, "include", "cadre_hip.h")).read()
    declared = set(re.findall(r"\b(cadre_[a-z0-9_]+)\s*\(", hdr))
    L = ctypes.CDLL(hip.LIB_PATH)
    for name in NEW:
        assert name in declared and name in hip.SYMBOLS and hasattr(L, name), name
    assert "rollout_finish.hip" in build.SOURCES
    assert hip.lib().cadre_abi_version() == 15                   # entry points are only added
    m = dict(re.findall(r"#define (CADRE_RS_[A-Z]+) (\d+)", hdr))
    assert (int(m["CADRE_RS_SCALE"]), int(m["CADRE_RS_CARRY"])) == (hip.RS_SCALE, hip.RS_CARRY)


def test_entry_points_reject_bad_arguments_without_launching():
    from cadre_amd import hip
    L = hip.lib()
    P = 16                                                       # (never dereferenced: rejected before any launch)
    ok = [P, 8, 128, 0.99, 1e-8, 1, P, P]
    for i, v in ((0, None), (6, None), (7, None), (1, 0), (1, 7), (1, 65536), (2, 1), (2, 3001), (3, -0.1), (3, 1.5),
                 (3, float("nan")), (4, -1.0), (4, float("nan")), (4, float("inf"))):
        bad = list(ok); bad[i] = v
        assert L.cadre_return_stats(*bad, None) == -1, (i, v)
        assert b"cadre_return_stats" in L.cadre_last_error()
    ok = [P, 8, 128, 0.99, 0.94, 1, None, 0.0]
    for i, v in ((0, None), (1, 0), (1, 65536), (2, 1), (2, 3001)):
        bad = list(ok); bad[i] = v
        assert L.cadre_gae_multi(*bad, None) == -1, (i, v)
        assert b"cadre_gae_multi" in L.cadre_last_error()
    for clip in (0.0, -1.0, float("nan")):                       # reward scaling on needs a clip
        assert L.cadre_gae_multi(P, 8, 128, 0.99, 0.94, 1, P, clip, None) == -1
        assert b"cadre_gae_multi" in L.cadre_last_error()
    ok = [P, P, 4, 8, 544, 544, 530, 530, 16, P, 544, P, P, P, P, P]
    for i, v in ((0, None), (1, None), (9, None), (11, None), (12, None), (13, None), (14, None), (15, None), (2, 0), (2, 3),
                 (3, 0), (8, 0), (6, 0), (7, 0), (4, 512), (5, 512), (10, 512)):
        bad = list(ok); bad[i] = v
        assert L.cadre_insert_rows_tl(*bad, None) == -1, (i, v)
        assert b"cadre_insert_rows_tl" in L.cadre_last_error()


def test_return_scaler_validation_and_state_dict_round_trip():
    from cadre_amd import hip
    from ppo_agent.storage import ReturnScaler
    for kw in (dict(n_envs=0), dict(n_envs=1.5), dict(n_envs=True), dict(gamma=1.5), dict(gamma=-0.1), dict(clip=0.0),
               dict(clip=float("inf")), dict(epsilon=-1e-8), dict(epsilon=float("nan")), dict(gamma=float("nan"))):
        args = dict(n_envs=2, gamma=0.99)
        args.update(kw)
        with pytest.raises(ValueError, match="ReturnScaler"):
            ReturnScaler(**args)
    rs = ReturnScaler(3, 0.99)
    assert (rs.clip, rs.epsilon, rs.training) == (10.0, 1e-8, True)
    assert rs.state.dtype == torch.float64 and rs.state.numel() == hip.RS_CARRY + 2 * 6
    assert rs.scale().dtype == torch.float32 and rs.scale().tolist() == [1.0, 1.0]
    sd0 = rs.state_dict()
    assert sorted(sd0) == ["M2", "carry", "count", "mean", "scale"]
    assert all(isinstance(v, torch.Tensor) for v in sd0.values())
    assert sd0["count"].tolist() == [0.0, 0.0] and tuple(sd0["carry"].shape) == (6, 2) and sd0["scale"].dtype == torch.float32
    g = torch.Generator().manual_seed(5)
    rs.state.copy_(torch.rand(rs.state.numel(), generator=g, dtype=torch.float64))
    rs.state[hip.RS_SCALE:hip.RS_CARRY] = torch.tensor([0.25, 3.0], dtype=torch.float64)
    sd = rs.state_dict()
    assert sd["count"].tolist() == [rs.state[0].item(), rs.state[3].item()]
    assert sd["M2"].tolist() == [rs.state[2].item(), rs.state[5].item()]
    other = ReturnScaler(3, 0.99)
    other.load_state_dict(sd)
    assert torch.equal(other.state, rs.state)
    sd["count"][0] = -1.0                                        # (state_dict hands out copies)
    assert rs.state[0].item() != -1.0
    with pytest.raises(ValueError, match="does not fit"):
        ReturnScaler(2, 0.99).load_state_dict(rs.state_dict())
    with pytest.raises(ValueError, match="missing"):
        other.load_state_dict({"count": sd["count"]})


def test_reward_scaling_config_rules():
    from ppo_agent.train import _reward_scaling, _time_limit_pair
    assert _reward_scaling({}) is None
    assert _reward_scaling({"reward_scaling": None}) is None
    assert _reward_scaling({"reward_scaling": True}) == dict(clip=10.0, epsilon=1e-8)
    assert _reward_scaling({"reward_scaling": {"clip": 5, "epsilon": 1e-6}}) == dict(clip=5.0, epsilon=1e-6)
    assert _reward_scaling({"reward_scaling": {}}) == dict(clip=10.0, epsilon=1e-8)
    for bad in (3, "yes", {"clip": 0.0}, {"clip": -1.0}, {"epsilon": -1.0}, {"clip": "x"}, {"gamma": 0.9}, {"clip": float("nan")},
                [10.0]):
        with pytest.raises(ValueError, match="reward_scaling"):
            _reward_scaling({"reward_scaling": bad})
    assert _time_limit_pair(True) == (True, True) and _time_limit_pair((0, 1)) == (False, True)


class _TwoRanks(object):
    @staticmethod
    def dist_world():
        return 2


def test_reward_scaling_refused_with_several_ranks():
    """Each rank would grow its own statistics: both learner sections and the config parser refuse before any device work."""
    from cadre_amd import hip
    from ppo_agent.storage import ReturnScaler
    from ppo_agent.train import _reward_scaling, learner_section, learner_section_multi
    cfg = dict(use_adv_norm=True, ppo_epoch=1, max_grad_norm=250.0)
    rs = ReturnScaler(1, 0.99)
    with pytest.raises(hip.CadreHipError, match="single rank"):
        learner_section(None, None, None, False, cfg, _TwoRanks(), reward_scaler=rs)
    with pytest.raises(hip.CadreHipError, match="single rank"):
        learner_section_multi(None, [], [], cfg, _TwoRanks(), reward_scaler=rs)
    with pytest.raises(hip.CadreHipError, match="single rank"):
        _reward_scaling({"reward_scaling": True}, _TwoRanks())
    assert _reward_scaling({}, _TwoRanks()) is None


def test_storage_time_limits_and_finish_rollouts_host_checks():
    from cadre_amd import hip
    from ppo_agent.storage import ReturnScaler, RolloutStorage
    mk = lambda T=8, gamma=0.99: RolloutStorage(T, 2, 530, 8, 530, True, gamma, 0.95)
    s = mk()
    assert tuple(s.time_limits.shape) == (9, 1) and s.time_limits.dtype == torch.float32 and not s.time_limits.any()
    obs = torch.zeros(8, 530)
    s.insert(obs, 1, 0.0, 0.0, 1.0, torch.ones(1, 1), None, 0)
    assert not s._tl_used
    s.insert(obs, 1, 0.0, 0.0, 1.0, torch.ones(1, 1), None, 0, time_limit=True)
    s.insert(obs, 1, 0.0, 0.0, 1.0, torch.ones(1, 1), None, 0)
    assert s._tl_used and s.time_limits[:, 0].tolist() == [0, 1, 0, 0, 0, 0, 0, 0, 0]
    s.to("cpu")                                                  # to() carries the flags
    assert s.time_limits[:, 0].tolist() == [0, 1, 0, 0, 0, 0, 0, 0, 0]
    with pytest.raises(ValueError, match="finish_rollouts"):
        RolloutStorage.finish_rollouts([], [])
    with pytest.raises(ValueError, match="finish_rollouts"):
        RolloutStorage.finish_rollouts([mk(), mk()], [0.0])
    for other in (mk(T=9), mk(gamma=0.9)):
        with pytest.raises(ValueError, match="same num_steps, gamma, tau and device"):
            RolloutStorage.finish_rollouts([mk(), other], [0.0, 0.0])
    with pytest.raises(hip.CadreHipError, match="HIP device"):   # no CPU path
        RolloutStorage.finish_rollouts([mk(), mk()], [0.0, 0.0])
    with pytest.raises(ValueError, match="two per environment"):
        RolloutStorage.finish_rollouts([mk(), mk()], [0.0, 0.0], reward_scaler=ReturnScaler(2, 0.99))
    with pytest.raises(ValueError, match="time-limit flags"):
        RolloutStorage.insert_batch([(mk(), mk())], [None], [[0, 0]], [[1, 1]], [0], time_limits=[True, False])


def test_stats_line_appends_the_reward_scales():
    from ppo_agent.train import stats_line
    rows = [dict(approx_kl=(0.001, 0.002), clip_fraction=(0.25, 0.5), grad_norm=[1.0, 3.5])]
    st = dict(rows=rows, explained_variance=[(0.5, 0.25)], updates_applied=1, steps=1)
    base = stats_line(0, st)
    st["reward_scale"] = (0.5, 2.0)
    assert stats_line(0, st) == base + ", reward scale: 5.0000e-01/2.0000e+00"
