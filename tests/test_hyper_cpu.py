"""CPU: device-resident hyper-parameters — the schedule arithmetic, the adaptive_lr rules of the learner section (excludes
a schedule for lr, refused at world size 2 over gloo), the argument checks of the `_hp` entry points (before any HIP
call) and the agreement of header, binding table and library on the new symbols."""
import ctypes
import os
import re
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HP_SYMBOLS = {"cadre_ppo_loss_hp", "cadre_ppo_loss_stats_hp", "cadre_grad_norms_hp", "cadre_clip_adam_graph_hp",
              "cadre_clip_adam_graph_hp_gated", "cadre_clip_adam_pack_graph_hp", "cadre_clip_adam_pack_graph_hp_gated",
              "cadre_clip_adam_norms_hp", "cadre_clip_adam_apply_hp"}


def test_schedule_value():
    from ppo_agent.train import schedule_value
    lin = ("linear", 3e-4, 3e-5)
    assert schedule_value(lin, 0, 6) == 3e-4                                         # start point, exactly
    assert schedule_value(lin, 3, 6) == 3e-4 + (3e-5 - 3e-4) * 3 / 6                 # midpoint
    assert schedule_value(lin, 5, 6) == 3e-4 + (3e-5 - 3e-4) * 5 / 6                 # last episode: one step before `end`
    assert schedule_value(("linear", 0.1, 0.02), 5, 10) == 0.1 + (0.02 - 0.1) * 5 / 10
    assert abs(schedule_value(("linear", 1.0, 0.0), 1, 2) - 0.5) == 0.0
    assert schedule_value(["linear", 2, 4], 1, 4) == 2.5                             # (a list, integers)
    assert schedule_value(0.05, 3, 7) == 0.05 and schedule_value(2, 0, 1) == 2.0     # constants
    assert schedule_value(lambda f: 1e-3 * (1.0 - f) ** 2, 1, 4) == 1e-3 * 0.75 ** 2
    seen = []
    schedule_value(lambda f: seen.append(f) or 1.0, 2, 8)
    assert seen == [0.25]
    for bad in (("linear", 1.0), ("cosine", 1.0, 0.0), ("linear", "a", 0.0), "linear", None, True, {"lr": 1},
                ("linear", 1.0, float("nan")), float("inf"), lambda f: "x", lambda f: float("nan")):
        with pytest.raises(ValueError):
            schedule_value(bad, 0, 4)
    for e, n in ((-1, 4), (4, 4), (0, 0), (1.5, 4), (0, 2.0)):
        with pytest.raises(ValueError):
            schedule_value(1.0, e, n)


def test_schedule_and_adaptive_lr_config_checks():
    from cadre_amd import hip
    from ppo_agent.train import _adaptive_lr, _schedules
    assert _schedules({}) == {} and _adaptive_lr({}, None) is None and _adaptive_lr({"adaptive_lr": None}, None) is None
    with pytest.raises(ValueError, match="unknown"):
        _schedules({"schedules": {"gamma": 0.9}})
    kw = _adaptive_lr({"adaptive_lr": {"desired_kl": 0.01}}, None)
    assert kw == dict(desired_kl=0.01, factor=1.5, lr_min=1e-5, lr_max=1e-2)
    kw = _adaptive_lr({"adaptive_lr": {"desired_kl": 0.02, "factor": 2.0, "min": 1e-4, "max": 1e-3},
                       "schedules": {"clip": ("linear", 0.1, 0.02)}, "target_kl": 0.05}, None)
    assert kw == dict(desired_kl=0.02, factor=2.0, lr_min=1e-4, lr_max=1e-3)
    with pytest.raises(ValueError, match="excludes"):
        _adaptive_lr({"adaptive_lr": {"desired_kl": 0.01}, "schedules": {"lr": ("linear", 3e-4, 3e-5)}}, None)
    for bad in ({"desired_kl": 0.0}, {"desired_kl": -1.0}, {"desired_kl": 0.01, "factor": 1.0}, {"factor": 2.0},
                {"desired_kl": 0.01, "min": 1e-3, "max": 1e-4}, {"desired_kl": 0.01, "min": 0.0},
                {"desired_kl": 0.01, "floor": 1e-5}, {"desired_kl": float("nan")}):
        with pytest.raises(ValueError):
            _adaptive_lr({"adaptive_lr": bad}, None)
    with pytest.raises(hip.CadreHipError, match="in-process chief"):
        _adaptive_lr({"adaptive_lr": {"desired_kl": 0.01}}, None, in_process_chief=False)


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from cadre_amd import hip
        from cadre_amd.arena import PPOArena
        from cadre_amd.learner import PPOLearnerHIP
        from ppo_agent.models import Model, Shared_grad_buffers, _no_orthogonal_init
        from ppo_agent.train import learner_section, learner_section_multi
        arena = PPOArena("cpu", 530, {"steer": 33, "throttle": 3}, 4)
        with _no_orthogonal_init():
            md = {"steer_ppo_0": arena.bind("steer_ppo_0", Model(530, 33))}
        shared = Shared_grad_buffers(md, torch.device("cpu"))
        cfg = dict(use_adv_norm=True, ppo_epoch=1, max_grad_norm=250.0, adaptive_lr={"desired_kl": 0.01})
        out = []
        for call in (lambda: learner_section(None, None, None, False, cfg, shared),
                     lambda: learner_section_multi(None, [], [], cfg, shared),
                     lambda: PPOLearnerHIP(arena).set_adaptive_lr(0.01)):      # (the learner's own check: before any device work)
            try:
                call()
                out.append("no error")
            except hip.CadreHipError as e:
                out.append("single rank" in str(e))
            except Exception as e:                              # noqa: BLE001 (reported to the parent)
                out.append(repr(e))
        q.put((rank, out))
    finally:
        dist.destroy_process_group()


def test_adaptive_lr_refused_with_two_ranks():
    """The controller moves a per-rank device value: with world size 2 both learner sections and the learner itself refuse
    it before any device work."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(60)
    assert res == {0: [True, True, True], 1: [True, True, True]}, res


def test_hp_symbols_in_header_table_and_library():
    from cadre_amd import hip
    hdr = open(os.path.join(ROOT, "include", "cadre_hip.h")).read()
    declared = set(re.findall(r"\b(cadre_[a-z0-9_]+)\s*\(", hdr))
    L = ctypes.CDLL(hip.LIB_PATH)
    for name in HP_SYMBOLS:
        assert name in declared and name in hip.SYMBOLS and hasattr(L, name), name
    assert hip.lib().cadre_abi_version() == hip.ABI_VERSION == 15
    # the named indices of the block: header and binding agree
    idx = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"#define CADRE_HP_([A-Z_]+) (\d+)", hdr)}
    assert idx.pop("fields") == hip.HP_FIELDS == 16
    assert idx == hip.HP and sorted(idx.values()) == list(range(10))
    assert int(re.search(r"#define CADRE_PPO_STATS_LR (\d+)", hdr).group(1)) == hip.PPO_STATS_LR == 7 < hip.PPO_STATS_FIELDS


def test_hp_entry_points_reject_bad_arguments_without_launching():
    from cadre_amd import hip
    L = hip.lib()
    P = 16                                                       # (never dereferenced: rejected before any launch)
    loss = [P, 64, 64 * 64, P, 64, 64 * 64, P, P, P, P, P, P, 64, 4, 33, 3, P, 1 / 64, P, P, P, P, None]
    HPI = 16
    for fn, tail in ((L.cadre_ppo_loss_hp, [None]), (L.cadre_ppo_loss_stats_hp, [P, 16, P, 0.0, None, None])):
        name = b"cadre_ppo_loss_stats_hp" if len(tail) > 1 else b"cadre_ppo_loss_hp"
        bad = list(loss); bad[HPI] = None                                               # NULL block
        assert fn(*bad, *tail) == -1 and name in L.cadre_last_error() and b"hyper-parameter block" in L.cadre_last_error()
        bad = list(loss); bad[HPI] = 20                                                 # misaligned block
        assert fn(*bad, *tail) == -1 and b"hyper-parameter block" in L.cadre_last_error()
        bad = list(loss); bad[14] = 65                                                  # n_out > 64 (as the by-value sibling)
        assert fn(*bad, *tail) == -1
        bad = list(loss); bad[13] = 0                                                   # C < 1
        assert fn(*bad, *tail) == -1
        bad = list(loss); bad[0] = None
        assert fn(*bad, *tail) == -1
    assert L.cadre_ppo_loss_stats_hp(*loss, None, 16, P, 0.0, None, None) == -1         # no stats row
    assert L.cadre_ppo_loss_stats_hp(*loss, P, 7, P, 0.0, None, None) == -1             # F < CADRE_PPO_STATS_FIELDS
    assert L.cadre_ppo_loss_stats_hp(*loss, P, 16, None, 0.0, None, None) == -1         # no partials scratch
    assert L.cadre_ppo_loss_stats_hp(*loss, P, 16, P, 0.01, None, None) == -1           # gate armed without a flag
    assert L.cadre_ppo_loss_stats_hp(*loss, P, 16, P, -1.0, P, None) == -1
    assert L.cadre_ppo_loss_stats_hp(*loss, P, 16, P, float("nan"), P, None) == -1

    adam = [P, P, P, P, P, 16, P, P, 0.9, 0.999, 1e-8, P]
    pack_tail = [8, 4 * 2120 * 544 + 2 * 2120, 2120 * 544, 2120, 544, 530, P, P, 34 * 4 * 34 * 256]
    cases = ((L.cadre_clip_adam_graph_hp, b"cadre_clip_adam_graph_hp", [], False),
             (L.cadre_clip_adam_graph_hp_gated, b"cadre_clip_adam_graph_hp_gated", [], True),
             (L.cadre_clip_adam_pack_graph_hp, b"cadre_clip_adam_pack_graph_hp", pack_tail, False),
             (L.cadre_clip_adam_pack_graph_hp_gated, b"cadre_clip_adam_pack_graph_hp_gated", pack_tail, True))
    for fn, name, mid, gated in cases:
        end = ([P] if gated else []) + [None]
        for i, v in ((7, None), (7, 12), (5, 0), (5, 255), (0, None), (11, None)):      # hp NULL / misaligned, n_models, params, step_dev
            bad = list(adam); bad[i] = v
            assert fn(*bad, *mid, *end) == -1, (name, i, v)
            assert name in L.cadre_last_error()
        if gated:
            assert fn(*adam, *mid, None, None) == -1                                    # no stop flag
        if mid:
            bad = list(mid); bad[4] = 512                                               # ldw != 544
            assert fn(*adam, *bad, *end) == -1 and b"built for W_hh" in L.cadre_last_error()
            bad = list(mid); bad[6] = None                                              # no forward copy
            assert fn(*adam, *bad, *end) == -1
    norms = [P, P, 16, P, P, 0.9, 0.999, P, 0, 1024]
    for i, v in ((4, None), (4, 4), (0, None), (2, 0), (8, 2), (9, 1022), (9, 0)):
        bad = list(norms); bad[i] = v
        assert L.cadre_clip_adam_norms_hp(*bad, None) == -1 and b"cadre_clip_adam_norms_hp" in L.cadre_last_error(), (i, v)
    apply_ = [P, P, P, P, P, 16, P, P, 0.9, 0.999, 1e-8, 0, 1024]
    for i, v in ((7, None), (7, 4), (0, None), (5, 0), (11, 2), (12, 1022), (12, 0)):
        bad = list(apply_); bad[i] = v
        assert L.cadre_clip_adam_apply_hp(*bad, None) == -1 and b"cadre_clip_adam_apply_hp" in L.cadre_last_error(), (i, v)
    assert L.cadre_grad_norms_hp(P, 4, P, 16, None, None) == -1 and b"cadre_grad_norms_hp" in L.cadre_last_error()
    assert L.cadre_grad_norms_hp(P, 4, P, 16, 12, None) == -1
    assert L.cadre_grad_norms_hp(None, 4, P, 16, P, None) == -1
    assert L.cadre_grad_norms_hp(P, 4, P, 15, P, None) == -1                            # F < 8 + 2 C
    assert L.cadre_grad_norms_hp(P, 0, P, 16, P, None) == -1


def test_learner_checks_without_a_device():
    """Argument validation of the learner's hyper-parameter interface that runs before any device work."""
    from cadre_amd import hip
    from cadre_amd.arena import PPOArena
    from cadre_amd.learner import PPOLearnerHIP
    lrn = PPOLearnerHIP(PPOArena("cpu", 530, {"steer": 33, "throttle": 3}, 4))
    assert (lrn.clip, lrn.vc, lrn.cc, lrn.ec) == (0.1, 0.1, 1.0, 0.01) and not lrn.device_hyper
    lrn.clip = 0.1                     # same value: nothing to drop, no device touched
    lrn.ec = 0.02                      # no captured graph yet: nothing to drop either
    assert lrn.ec == 0.02 and lrn._mode_key() == ()
    with pytest.raises(hip.CadreHipError, match="set_device_hyper"):
        lrn.set_hyper(lr=1e-4)
    for kw in (dict(desired_kl=0.0), dict(desired_kl=-1.0), dict(desired_kl=0.01, factor=1.0),
               dict(desired_kl=0.01, lr_min=0.0), dict(desired_kl=0.01, lr_min=1e-2, lr_max=1e-3),
               dict(desired_kl=0.01, lr=0.0), dict(desired_kl=float("nan"))):
        with pytest.raises(ValueError):
            lrn.set_adaptive_lr(**kw)
    lrn.set_adaptive_lr(None)          # off while off: nothing
