"""CPU: host-side parts of CadreAgent.act_batch / RolloutStorage.insert_batch — argument checks of the three C-ABI entry
points (before any launch), the command sort of the batched rows, and act_batch's refusals.  No kernel is launched."""
import numpy as np
import pytest
import torch


def test_act_batch_entry_points_reject_bad_arguments_without_launching():
    from cadre_amd import hip
    L = hip.lib()
    P = 16                                          # (a non-null pointer value: never dereferenced, the checks come first)
    # cadre_act_windows(ring, ring_env_str, n_ring, fresh, ld_fresh, F, mode, first, meas, pos, N, S, X, ldx, DP, feat, ldf, stream)
    ok = [P, 8 * 512, 4, P, 512, 8, P, P, P, P, 4, 8, P, 544, 544, P, 544, None]

    def windows(**kw):
        names = ["ring", "ring_env_str", "n_ring", "fresh", "ld_fresh", "F", "mode", "first", "meas", "pos", "N", "S", "X",
                 "ldx", "DP", "feat", "ldf", "stream"]
        args = list(ok)
        for k, v in kw.items():
            args[names.index(k)] = v
        return L.cadre_act_windows(*args)
    for kw in (dict(ring=None), dict(fresh=None), dict(meas=None), dict(pos=None), dict(X=None), dict(mode=None)):
        assert windows(**kw) == -1 and b"cadre_act_windows: null operand" in L.cadre_last_error(), kw
    for kw in (dict(N=0), dict(N=5), dict(S=0), dict(F=0), dict(DP=529), dict(ldx=512), dict(ring_env_str=7 * 512),
               dict(ld_fresh=500), dict(ldf=530)):
        assert windows(**kw) == -1 and b"cadre_act_windows: bad argument" in L.cadre_last_error(), kw
    # cadre_sample_rows(O3, ldo, z_str, pos, cmd, N, C, q, K_steer, K_throttle, action, logp, value, stream)
    ok_s = [P, 64, 64 * 4, P, P, 4, 4, P, 33, 3, P, P, P, None]

    def sample(i, v):
        args = list(ok_s)
        args[i] = v
        return L.cadre_sample_rows(*args)
    for i in (0, 3, 4, 7, 10, 11, 12):
        assert sample(i, None) == -1 and b"cadre_sample_rows: null operand" in L.cadre_last_error(), i
    for i, v in ((5, 0), (6, 0), (6, 17), (8, 65), (9, 65), (8, 0), (1, 32), (2, 64 * 3)):
        assert sample(i, v) == -1 and b"cadre_sample_rows: bad argument" in L.cadre_last_error(), (i, v)
    # cadre_insert_rows(table, slot, n_dst, S, ldo, ldh, D, Hd, T, feat, ldf, action, logp, value, rm, cmd, stream)
    ok_i = [P, P, 4, 8, 544, 544, 530, 530, 8, P, 544, P, P, P, P, P, None]

    def insert(i, v):
        args = list(ok_i)
        args[i] = v
        return L.cadre_insert_rows(*args)
    for i in (0, 1, 9, 11, 12, 13, 14, 15):
        assert insert(i, None) == -1 and b"cadre_insert_rows: null operand" in L.cadre_last_error(), i
    for i, v in ((2, 0), (2, 3), (3, 0), (8, 0), (4, 500), (5, 500), (10, 100), (6, 0)):
        assert insert(i, v) == -1 and b"cadre_insert_rows: bad argument" in L.cadre_last_error(), (i, v)
    with pytest.raises(hip.CadreHipError, match="cadre_sample_rows"):
        hip.check(sample(8, 65), "cadre_sample_rows")


def test_command_rows_is_a_stable_sort_with_every_command():
    from ppo_agent.agent import command_rows
    cmds = [2, 0, 3, 2, 0, 1, 2]
    pos, seg = command_rows(cmds, 4)
    assert pos.dtype == np.int32 and seg.dtype == np.int32 and seg.shape == (8, 2)
    assert sorted(pos.tolist()) == list(range(7))
    order = np.argsort(pos)
    assert [cmds[i] for i in order] == sorted(cmds)
    assert order.tolist() == [1, 4, 5, 0, 3, 6, 2]                 # environments of one command keep their order
    assert seg[:4].tolist() == [[0, 2], [2, 1], [3, 3], [6, 1]]
    assert seg[4:].tolist() == seg[:4].tolist()                    # throttle nets: the same runs
    for c in range(4):                                             # every environment inside its command's run
        b, n = seg[c]
        assert all(b <= pos[e] < b + n for e in range(7) if cmds[e] == c)
    # a command without rows: count 0 (the kernels skip it)
    pos, seg = command_rows([1, 1, 3], 6)
    assert pos.tolist() == [0, 1, 2]
    assert seg[:6].tolist() == [[0, 0], [0, 2], [2, 0], [2, 1], [3, 0], [3, 0]]
    # N = 1
    pos, seg = command_rows([2], 4)
    assert pos.tolist() == [0] and seg[:4].tolist() == [[0, 0], [0, 0], [0, 1], [1, 0]]
    with pytest.raises(ValueError):
        command_rows([4], 4)
    with pytest.raises(ValueError):
        command_rows([], 4)


def _obs(S=8, H=12, W=20, command=1):
    return dict(rgb=np.zeros((S, H, W, 3), np.uint8), route_fig=np.zeros((S, W, H), np.uint8),
                measurements=np.zeros((S, 3)), command=command)


def test_act_batch_refuses_bad_batches_before_any_device_work():
    from cadre_amd import hip
    from ppo_agent.agent import CadreAgent, check_act_batch
    d0, d1 = torch.device("cuda:0"), torch.device("cuda:1")
    check_act_batch([_obs(), _obs(command=3)], None, 32, d0, d0, 4)           # fine
    with pytest.raises(hip.CadreHipError, match="vae_device"):
        check_act_batch([_obs()], None, 32, d0, d1, 4)
    with pytest.raises(hip.CadreHipError, match="max_envs = 2"):
        check_act_batch([_obs()] * 3, None, 2, d0, d0, 4)
    with pytest.raises(hip.CadreHipError, match="1 .. model_cfg.max_envs"):
        check_act_batch([], None, 32, d0, d0, 4)
    with pytest.raises(hip.CadreHipError, match="observation 1"):
        check_act_batch([_obs(), _obs(W=24)], None, 32, d0, d0, 4)
    with pytest.raises(hip.CadreHipError, match="observation 2"):
        check_act_batch([_obs(), _obs(), _obs(S=4)], None, 32, d0, d0, 4)
    with pytest.raises(hip.CadreHipError, match="command 4"):
        check_act_batch([_obs(command=4)], None, 32, d0, d0, 4)
    with pytest.raises(hip.CadreHipError, match="hints"):
        check_act_batch([_obs(), _obs()], [True], 32, d0, d0, 4)
    bad = _obs()
    bad["measurements"] = np.zeros((8, 2))
    with pytest.raises(hip.CadreHipError, match="observation 1"):
        check_act_batch([_obs(), bad], None, 32, d0, d0, 4)
    # the method checks before it touches a device (an agent shell without encoder or nets)
    ag = CadreAgent.__new__(CadreAgent)
    ag.device, ag.vae_device, ag.max_envs, ag.command_num = d0, d1, 32, 4
    with pytest.raises(hip.CadreHipError, match="share one GPU"):
        ag.act_batch([_obs()])
    ag.vae_device = d0
    with pytest.raises(hip.CadreHipError, match="max_envs"):
        ag.act_batch([_obs()] * 33)


def test_insert_batch_refuses_mismatched_arguments():
    from ppo_agent.storage import RolloutStorage
    a, b = RolloutStorage(4, 2, 530, 8, 530, True, 0.99, 0.95), RolloutStorage(4, 2, 530, 8, 530, True, 0.99, 0.95)
    c = RolloutStorage(5, 2, 530, 8, 530, True, 0.99, 0.95)
    with pytest.raises(ValueError, match="storage pairs"):
        RolloutStorage.insert_batch([(a, b)], [], [[0, 0]], [[1, 1]], [0])
    with pytest.raises(ValueError, match="geometry"):
        RolloutStorage.insert_batch([(a, c)], [None], [[0, 0]], [[1, 1]], [0])
    from cadre_amd import hip
    with pytest.raises(hip.CadreHipError, match="HIP device"):
        RolloutStorage.insert_batch([(a, b)], [None], [[0, 0]], [[1, 1]], [0])
    assert a.step == b.step == 0
