"""CPU: frame-table storages — the C ABI additions, the numpy statement of the frame scan (tests/frame_table_ref.py), the
config keys and the capacity arithmetic, and what a FrameStorage refuses."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from tests import frame_table_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {"cadre_gather_sorted_multi_ft": 27, "cadre_gather_minibatch_multi_ft": 24, "cadre_gather_minibatch_ft": 32,
               "cadre_gather_obs_ft": 11, "cadre_frames_scan": 10, "cadre_frames_copy": 15}


# ----------------------------------------------------------------------------- C ABI
def test_entry_points_are_exported_and_bound():
    from cadre_amd import hip
    L = ctypes.CDLL(hip.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "cadre_hip.h")).read()
    for name, nargs in NEW_SYMBOLS.items():
        assert hasattr(L, name) and name in hip.SYMBOLS and re.search(r"\bint %s\s*\(" % name, hdr), name
        assert len(hip.SYMBOLS[name]) == nargs, name
    # a twin takes its original's arguments (+ win and n_frames where the source is not a table record)
    assert hip.SYMBOLS["cadre_gather_sorted_multi_ft"] == hip.SYMBOLS["cadre_gather_sorted_multi"]
    assert hip.SYMBOLS["cadre_gather_minibatch_multi_ft"] == hip.SYMBOLS["cadre_gather_minibatch_multi"]
    assert len(hip.SYMBOLS["cadre_gather_minibatch_ft"]) == len(hip.SYMBOLS["cadre_gather_minibatch"]) + 2
    assert len(hip.SYMBOLS["cadre_gather_obs_ft"]) == len(hip.SYMBOLS["cadre_gather_obs"]) + 2
    assert hip.lib().cadre_abi_version() == hip.ABI_VERSION == 15          # entry points are only added
    assert '"frame_table.hip"' in open(os.path.join(ROOT, "cadre_amd", "build.py")).read()
    from ppo_agent import frames as shim
    from cadre_amd import frames
    assert shim.FrameStorage is frames.FrameStorage and shim.scan_frames is frames.scan_frames


# ----------------------------------------------------------------------------- the reference scan
S, D, LD = 8, 530, 544


def test_sliding_windows_give_T_plus_S_minus_1_frames():
    """T windows that slide over T + S - 1 distinct frames: row 0 is all new, every later row adds one."""
    rng = np.random.RandomState(0)
    T = 6
    stream = rng.standard_normal((T + S - 1, D)).astype(np.float32)
    obs = np.stack([stream[t:t + S] for t in range(T)])
    flags, ids, count = ref.scan(obs, D)
    assert count == T + S - 1
    assert np.array_equal(ids, np.arange(T)[:, None] + np.arange(S)[None, :])
    assert (flags[0] == ref.NEW).all() and (flags[1:, :S - 1] == ref.SLIDE).all() and (flags[1:, S - 1] == ref.NEW).all()
    frames, ids2 = ref.pack(obs, D, LD)
    assert np.array_equal(frames[:, :D], stream) and not frames[:, D:].any() and np.array_equal(ids2, ids)
    assert np.array_equal(ref.materialise(frames, ids, D).view(np.uint32), obs.view(np.uint32))


def test_a_reset_filled_window_adds_exactly_one_frame():
    rng = np.random.RandomState(1)
    obs = ref.sliding_obs(5, S, D, LD, rng, resets=(3,))
    flags, ids, count = ref.scan(obs, D)
    # row 0 (a fill): 1; rows 1, 2 slide: + 1 each; row 3 a reset fill: + 1; row 4 slides: + 1
    assert count == 5
    assert flags[3, 0] == ref.NEW and (flags[3, 1:] == ref.FILL).all() and (ids[3] == ids[3, 0]).all()
    assert flags[0, 0] == ref.NEW and (flags[0, 1:] == ref.FILL).all()
    # the row behind the reset slides over the filled window: S - 1 ids of the reset frame, then a new one
    assert (ids[4, :S - 1] == ids[3, 0]).all() and flags[4, S - 1] == ref.NEW
    assert np.array_equal(ref.materialise(*ref.pack(obs, D, LD), D).view(np.uint32), obs[:, :, :D].view(np.uint32))


def test_rows_without_equalities_are_all_new():
    rng = np.random.RandomState(2)
    P = 4
    obs = rng.standard_normal((P, S, LD)).astype(np.float32)
    flags, ids, count = ref.scan(obs, D)
    assert count == P * S and not flags.any() and np.array_equal(ids.ravel(), np.arange(P * S))


def test_what_counts_as_equal():
    """Column D - 1 alone makes a new frame, the pad alone does not, -0.0 is not +0.0, equal NaN bits are equal."""
    rng = np.random.RandomState(3)
    base = ref.sliding_obs(3, S, D, LD, rng)
    assert ref.scan(base, D)[2] == 3
    last = base.copy()
    last[2, 1, D - 1] += 1.0                                           # (row 2, s 1) was the slide of (row 1, s 2)
    flags, _ids, count = ref.scan(last, D)
    assert count == 4 and flags[2, 1] == ref.NEW and flags[2, 0] == ref.SLIDE and flags[2, 2] == ref.SLIDE
    pad = base.copy()
    pad[2, 1, D:] = 9.0
    assert ref.scan(pad, D)[2] == 3 and np.array_equal(ref.scan(pad, D)[1], ref.scan(base, D)[1])
    zero = base.copy()
    zero[1, 2, 7] = 0.0
    zero[2, 1, 7] = -0.0                                               # equal as floats, different bits
    assert zero[1, 2, 7] == zero[2, 1, 7] and ref.scan(zero, D)[0][2, 1] == ref.NEW
    nan = base.copy()
    nan[1, 2, 7] = nan[2, 1, 7] = np.float32("nan")                    # unequal as floats, identical bits
    assert ref.scan(nan, D)[0][2, 1] == ref.SLIDE and ref.scan(nan, D)[2] == 4         # (the marked frame itself is the 4th)


def test_the_slide_wins_over_the_fill():
    """A row that equals both the row above's next frame and its own left neighbour takes the slide's id (rule 1 first)."""
    rng = np.random.RandomState(4)
    obs = ref.sliding_obs(2, 3, 5, 8, rng)                             # row 0: frame a three times; row 1: a a b
    flags, ids, count = ref.scan(obs, 5)
    assert count == 2 and flags.tolist() == [[0, 2, 2], [1, 1, 0]] and ids.tolist() == [[0, 0, 0], [0, 0, 1]]


# ----------------------------------------------------------------------------- config keys and capacity
def test_frame_table_config_keys():
    from ppo_agent.imitation import _demo_key, demo_mix_config, pretrain_config
    assert "frame_table" not in pretrain_config(dict(episodes="/d")) and "frame_table" not in demo_mix_config(dict(episodes="/d"))
    assert pretrain_config(dict(episodes="/d", frame_table=True))["frame_table"] is True
    assert demo_mix_config(dict(episodes="/d", frame_table=False))["frame_table"] is False
    for parse, where in ((pretrain_config, "pretrain"), (demo_mix_config, "demo_mix")):
        for bad in (1, 0, "yes", None, 1.0):
            with pytest.raises(ValueError, match=r"train_cfg\.%s: frame_table must be a bool" % where):
                parse(dict(episodes="/d", frame_table=bad))
    k0, k1 = _demo_key(["a", "b"], 0.99, "command", 1.0), _demo_key(["a", "b"], 0.99, "command", 1.0, True)
    assert k0 != k1 and k0 == _demo_key(["a", "b"], 0.99, "command", 1.0, False)


def test_frames_per_row_config_and_capacity():
    from cadre_amd.frames import capacity_for, frames_per_row_ok
    from cadre_amd.phasic import AuxBuffer, aux_config
    assert "frames_per_row" not in aux_config(dict(interval=2))
    assert aux_config(dict(interval=2, frames_per_row=1.25))["frames_per_row"] == 1.25
    assert aux_config(dict(interval=2, frames_per_row=None))["frames_per_row"] is None
    for bad in (0, -1.0, float("nan"), float("inf"), "2", True, 16.5, 0.01):
        with pytest.raises(ValueError, match="frames_per_row"):
            aux_config(dict(interval=2, frames_per_row=bad))
    assert capacity_for(1024, 1.25, 8) == 1280 and capacity_for(10, 1.01, 8) == 11 and capacity_for(16, 0.125, 8) == 2
    assert capacity_for(7, 8, 8) == 56 and frames_per_row_ok(8, 8) and not frames_per_row_ok(8.5, 8)
    for bad in (0.1, 8.01, float("nan"), None, "1"):
        with pytest.raises(ValueError, match=r"\[1/S, S\]"):
            capacity_for(64, bad, 8)
    # a PPG buffer of 32 sections x 8 environments x 128 steps: window rows against frames at 1.1 per row
    R = 32 * 8 * 128
    assert R * 8 * 544 * 4 > 5.5e8 and capacity_for(R, 1.1, 8) * 544 * 4 + R * 8 * 4 < 8.0e7
    agent = types.SimpleNamespace(lstm_input=530, learner=types.SimpleNamespace(S=8), arena=types.SimpleNamespace(device="cpu"))
    buf = AuxBuffer(agent, 2, 8, frames_per_row=1.5, _device="cpu")
    assert buf.steer._frames.shape == (24, 544) and buf.steer._win.shape == (17, 8) and buf.steer._obs is None
    assert buf.throttle._frames is buf.steer._frames and buf.throttle._win is buf.steer._win and buf.frames_used == 0
    assert AuxBuffer(agent, 2, 8, _device="cpu").steer._obs.shape == (17, 8, 544)      # the default is today's buffer
    with pytest.raises(ValueError, match=r"\[1/S, S\]"):
        AuxBuffer(agent, 2, 8, frames_per_row=9.0, _device="cpu")


# ----------------------------------------------------------------------------- FrameStorage on the host
def test_frame_storage_fields_and_refusals():
    from cadre_amd.frames import FrameStorage, frame_pair
    from ppo_agent.storage import RolloutStorage
    st = FrameStorage(6, 1, 530, 8, 530, True, 0.99, 1.0, frame_capacity=10)
    plain = RolloutStorage(6, 1, 530, 8, 530, True, 0.99, 1.0)
    assert isinstance(st, RolloutStorage) and st._obs is None and st.n_frames == 0
    assert (st._ldo, st.seq_length, st._ldh, st.z_dims) == (plain._ldo, plain.seq_length, plain._ldh, plain.z_dims)
    assert st._frames.shape == (10, st._ldo) and st._win.shape == (7, 8) and st._win.dtype == torch.int32
    assert int(st._win.max()) == -1 and st.frame_bytes() == 10 * 544 * 4 + 7 * 8 * 4
    for k in ("_hn", "_cn", "command", "rewards", "value_preds", "returns", "action_log_probs", "action", "masks", "advantages"):
        assert getattr(st, k).shape == getattr(plain, k).shape and getattr(st, k).dtype == getattr(plain, k).dtype
    with pytest.raises(ValueError, match="from_episodes.*AuxBuffer"):
        st.insert(torch.zeros(8, 530), 0, 0.0, 0.0, 0.0, 1.0, None, 0)
    with pytest.raises(ValueError, match="from_episodes.*AuxBuffer"):
        RolloutStorage.insert_batch([(st, st)], [None], [[0.0, 0.0]], [[1.0, 1.0]], [0])
    a, b = frame_pair(6, 530, 8, 530, 0.99, "cpu", frame_capacity=4)
    assert b._frames is a._frames and b._win is a._win
    a._frames[1, :3] = torch.tensor([1.0, 2.0, 3.0])
    a._win[2, 5], a.n_frames = 1, 2
    a.returns[3] = 0.5
    kept = (a._frames.clone(), a._win.clone())
    a.to("cpu")                                                         # moves frames and ids with the other fields
    assert torch.equal(a._frames, kept[0]) and torch.equal(a._win, kept[1]) and a.n_frames == 2 and a._obs is None
    assert float(a.returns[3]) == 0.5
    for bad in (dict(), dict(frame_capacity=0), dict(frame_capacity=True), dict(frames=torch.zeros(4, 530)),
                dict(frames=torch.zeros(4, 544), win=torch.zeros(7, 8, dtype=torch.int64)),
                dict(frames=torch.zeros(4, 544), n_frames=5)):
        with pytest.raises(ValueError):
            FrameStorage(6, 1, 530, 8, 530, True, 0.99, 1.0, **bad)
