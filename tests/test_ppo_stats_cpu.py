"""CPU: argument checks of the update-diagnostics entry points (before any HIP call), the target_kl rules of the learner
section (world > 1 refused, over gloo), and the host-side formatting of the diagnostics."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp


def test_stats_entry_points_reject_bad_arguments_without_launching():
    from cadre_amd import hip
    L = hip.lib()
    P = 16                                                       # (never dereferenced: rejected before any launch)
    loss = [P, 64, 64 * 64, P, 64, 64 * 64, P, P, P, P, P, P, 64, 4, 33, 3, 0.1, 0.1, 1.0, 0.01, 1 / 64, P, P, P, P, None]
    assert L.cadre_ppo_loss_stats(*loss, None, 16, P, 0.0, None, None) == -1        # no stats row
    assert b"cadre_ppo_loss_stats" in L.cadre_last_error()
    assert L.cadre_ppo_loss_stats(*loss, P, 7, P, 0.0, None, None) == -1            # F < CADRE_PPO_STATS_FIELDS
    assert L.cadre_ppo_loss_stats(*loss, P, 16, None, 0.0, None, None) == -1        # no partials scratch
    assert L.cadre_ppo_loss_stats(*loss, P, 16, P, 0.01, None, None) == -1          # gate armed without a flag
    assert L.cadre_ppo_loss_stats(*loss, P, 16, P, -1.0, P, None) == -1             # negative target_kl
    assert L.cadre_ppo_loss_stats(*loss, P, 16, P, float("nan"), P, None) == -1
    bad = list(loss); bad[13] = 0                                                   # C < 1
    assert L.cadre_ppo_loss_stats(*bad, P, 16, P, 0.0, None, None) == -1
    adam = [P, P, P, P, P, 16, P, 250.0, 3e-4, 0.9, 0.999, 1e-8, P]
    assert L.cadre_clip_adam_graph_gated(*adam, None, None) == -1 and b"cadre_clip_adam_graph_gated" in L.cadre_last_error()
    bad = list(adam); bad[5] = 0
    assert L.cadre_clip_adam_graph_gated(*bad, P, None) == -1
    pack = adam + [8, 4 * 2120 * 544 + 2 * 2120, 2120 * 544, 2120, 544, 530, P, P, 34 * 4 * 34 * 256]
    assert L.cadre_clip_adam_pack_graph_gated(*pack, None, None) == -1
    assert b"cadre_clip_adam_pack_graph_gated" in L.cadre_last_error()
    bad = list(pack); bad[17] = 512                                                 # ldw != 544
    assert L.cadre_clip_adam_pack_graph_gated(*bad, P, None) == -1 and b"built for W_hh" in L.cadre_last_error()
    assert L.cadre_grad_norms(None, 4, P, 16, None) == -1 and b"cadre_grad_norms" in L.cadre_last_error()
    assert L.cadre_grad_norms(P, 4, P, 15, None) == -1                              # F < 8 + 2 C
    assert L.cadre_grad_norms(P, 0, P, 16, None) == -1
    assert L.cadre_explained_variance(None, 2, P, None) == -1 and b"cadre_explained_variance" in L.cadre_last_error()
    assert L.cadre_explained_variance(P, 0, P, None) == -1
    assert L.cadre_explained_variance(P, 2, None, None) == -1


def test_stats_loss_entry_point_rejects_what_the_plain_one_rejects():
    from cadre_amd import hip
    L = hip.lib()
    P = 16
    loss = [P, 64, 64 * 64, P, 64, 64 * 64, P, P, P, P, P, P, 64, 4, 65, 3, 0.1, 0.1, 1.0, 0.01, 1 / 64, P, P, P, P, None]
    assert L.cadre_ppo_loss(*loss, None) == -1                                      # n_out > 64
    assert L.cadre_ppo_loss_stats(*loss, P, 16, P, 0.0, None, None) == -1
    loss[0] = None
    loss[14] = 33
    assert L.cadre_ppo_loss_stats(*loss, P, 16, P, 0.0, None, None) == -1


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from cadre_amd import hip
        from cadre_amd.arena import PPOArena
        from ppo_agent.models import Model, Shared_grad_buffers, _no_orthogonal_init
        from ppo_agent.train import learner_section, learner_section_multi
        arena = PPOArena("cpu", 530, {"steer": 33, "throttle": 3}, 4)
        with _no_orthogonal_init():
            md = {"steer_ppo_0": arena.bind("steer_ppo_0", Model(530, 33))}
        shared = Shared_grad_buffers(md, torch.device("cpu"))
        cfg = dict(use_adv_norm=True, ppo_epoch=1, max_grad_norm=250.0, target_kl=0.01)
        out = []
        for call in (lambda: learner_section(None, None, None, False, cfg, shared),
                     lambda: learner_section_multi(None, [], [], cfg, shared)):
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


def test_target_kl_refused_with_two_ranks():
    """The gate is a per-rank device flag: with world size 2 both learner sections refuse target_kl before any device work."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(60)
    assert res == {0: [True, True], 1: [True, True]}, res


def test_target_kl_checks_on_one_rank():
    from cadre_amd import hip
    from ppo_agent.train import _target_kl
    assert _target_kl({}, None) is None
    assert _target_kl({"target_kl": None}, None) is None
    assert _target_kl({"target_kl": 0.02}, None) == 0.02
    with pytest.raises(ValueError):
        _target_kl({"target_kl": 0.0}, None)
    with pytest.raises(hip.CadreHipError, match="in-process chief"):
        _target_kl({"target_kl": 0.02}, None, in_process_chief=False)


def test_stats_line_format():
    from ppo_agent.train import stats_line
    rows = [dict(approx_kl=(0.001, 0.002), clip_fraction=(0.25, 0.5), grad_norm=[1.0, 3.5]),
            dict(approx_kl=(0.003, 0.004), clip_fraction=(0.75, 0.0), grad_norm=[2.0, 0.5])]
    st = dict(rows=rows, explained_variance=[(0.5, 0.25), (0.7, float("nan"))], updates_applied=1, steps=2)
    line = stats_line(3, st)
    assert line == ("Episode: 3, approx kl: 0.002000/0.003000, clip fraction: 0.5000/0.2500, explained variance: "
                    "0.6000/nan, updates applied: 1/2, max grad norm: 3.5000")
