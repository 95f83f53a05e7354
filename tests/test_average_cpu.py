"""CPU: weight averaging — the train_cfg key and its refusals, the warm-up rule, the C ABI's new symbols and their refusals,
soup's refusals, and the snapshot / checkpoint metadata paths with mocks."""
import inspect
import types

import pytest
import torch

from tests import average_ref as ref


class _World(object):
    def __init__(self, n, mode="allreduce"):
        self.n, self.mode = n, mode

    def dist_world(self):
        return self.n

    def exchange_mode(self):
        return self.mode


# ----------------------------------------------------------------------------- the key
def test_average_config_keys():
    from cadre_amd.average import AVERAGE_KEYS, average_config
    assert AVERAGE_KEYS == ("decay", "warmup", "snapshot")
    assert average_config(None) is None
    assert average_config({"decay": 0.99}) == dict(decay=0.99, warmup=True, snapshot=True)
    assert average_config({"decay": 0.5, "warmup": False, "snapshot": False}) == dict(decay=0.5, warmup=False, snapshot=False)
    for bad in (0.0, 1.0, -0.1, 1.5, True, "0.9", None, float("nan")):
        with pytest.raises(ValueError, match="decay"):
            average_config({"decay": bad})
    with pytest.raises(ValueError, match="needs decay"):
        average_config({})
    with pytest.raises(ValueError, match="needs decay"):
        average_config({"warmup": True})
    with pytest.raises(ValueError, match="unknown.*tau"):
        average_config({"decay": 0.9, "tau": 1})
    with pytest.raises(ValueError, match="warmup"):
        average_config({"decay": 0.9, "warmup": 1})
    with pytest.raises(ValueError, match="snapshot"):
        average_config({"decay": 0.9, "snapshot": "yes"})
    with pytest.raises(ValueError, match="weight_average"):
        average_config(0.9)


def test_key_absent_builds_nothing():
    """Key absent / None: None from every layer, and the device is never initialised."""
    from cadre_amd.average import average_runner
    from ppo_agent.train import weight_average, weight_average_config
    was = torch.cuda.is_initialized()
    assert weight_average_config({}) is None and weight_average_config({"weight_average": None}) is None
    assert weight_average(object(), None) is None
    assert average_runner(object(), None, shared_grad_buffers=_World(4)) is None       # (nothing to refuse either)
    assert torch.cuda.is_initialized() == was


def test_average_refusals_by_name():
    from cadre_amd.average import average_refusals
    from ppo_agent.train import weight_average_config
    average_refusals()
    average_refusals(shared_grad_buffers=_World(0))
    average_refusals(shared_grad_buffers=_World(1), in_process_chief=True)
    with pytest.raises(ValueError, match="weight_average needs a single rank"):
        average_refusals(shared_grad_buffers=_World(2))
    with pytest.raises(ValueError, match="weight_average needs the in-process chief"):
        average_refusals(in_process_chief=False)
    with pytest.raises(ValueError, match="weight_average excludes the sharded optimiser"):
        average_refusals(shared_grad_buffers=_World(1, "sharded"))
    # through the training loops' helper: the key's own errors first, then the refusals — nothing is allocated
    with pytest.raises(ValueError, match="decay"):
        weight_average_config({"weight_average": {"decay": 2}}, _World(2))
    with pytest.raises(ValueError, match="single rank"):
        weight_average_config({"weight_average": {"decay": 0.9}}, _World(2))
    with pytest.raises(ValueError, match="in-process chief"):
        weight_average_config({"weight_average": {"decay": 0.9}}, _World(1), False)
    assert weight_average_config({"weight_average": {"decay": 0.9}}, _World(1)) == dict(decay=0.9, warmup=True, snapshot=True)
    # shared nets in another parameter arena than the agent's: the optimiser would step that arena
    mine, other = types.SimpleNamespace(arena=object()), _World(1)
    other.arena = object()
    with pytest.raises(ValueError, match="weight_average: the shared nets live in another parameter arena"):
        weight_average_config({"weight_average": {"decay": 0.9}}, other, True, mine)
    other.arena = mine.arena
    assert weight_average_config({"weight_average": {"decay": 0.9}}, other, True, mine)["decay"] == 0.9
    assert weight_average_config({}, other, True, mine) is None


def test_weight_average_refuses_bad_decay_before_touching_the_arena():
    from cadre_amd.average import WeightAverage
    for bad in (0, 1, 1.0, -1e-3, "x", True):
        with pytest.raises(ValueError, match="decay"):
            WeightAverage(object(), decay=bad)
    with pytest.raises(ValueError, match="warmup"):
        WeightAverage(object(), decay=0.9, warmup=None)


# ----------------------------------------------------------------------------- the warm-up rule
@pytest.mark.parametrize("decay", [0.9, 0.999, 0.5])
def test_warmup_sequence(decay):
    from cadre_amd.average import warmup_decay
    seq = ref.warmup_sequence(decay, 41)
    assert len(seq) == 41 and seq[0] == 0.1 and seq[1] == 2.0 / 11.0
    for n, d in enumerate(seq):
        assert d == min(decay, (1.0 + n) / (10.0 + n)) == warmup_decay(decay, n)        # the division is correctly rounded
        assert 0.0 < d <= decay
    assert all(a <= b for a, b in zip(seq, seq[1:]))
    first = next((n for n, d in enumerate(seq) if d == decay), None)
    # (1 + n) / (10 + n) >= decay  <=>  n >= (10 decay - 1) / (1 - decay): 8 at 0.5, 80 at 0.9, 8990 at 0.999
    assert first == (8 if decay == 0.5 else None)
    assert ref.warmup_sequence(decay, 41, warmup=False) == [decay] * 41 == [warmup_decay(decay, n, False) for n in range(41)]


# ----------------------------------------------------------------------------- the C ABI
def test_symbols_and_abi():
    from cadre_amd import hip
    i32, i64, vp = hip.i32, hip.i64, hip.vp
    assert hip.ABI_VERSION == 15
    assert hip.SYMBOLS["cadre_ema_update"] == [vp, vp, vp, i32, vp, vp, vp, vp]
    assert hip.SYMBOLS["cadre_arena_swap"] == [vp, vp, i64, vp]
    assert hip.SYMBOLS["cadre_arena_mean"] == [vp, vp, i32, vp, i64, vp]
    L = hip.lib()
    assert L.cadre_abi_version() == 15
    for name in ("cadre_ema_update", "cadre_arena_swap", "cadre_arena_mean"):
        assert getattr(L, name).argtypes == hip.SYMBOLS[name]
    assert (hip.EMA_DECAY, hip.EMA_WARMUP, hip.EMA_COUNT, hip.EMA_D, hip.EMA_SKIPPED, hip.EMA_HEAD) == (0, 1, 2, 3, 4, 8)
    import os
    hdr = open(os.path.join(os.path.dirname(hip.__file__), "..", "include", "cadre_hip.h")).read()
    for k, v in dict(DECAY=0, WARMUP=1, COUNT=2, D=3, SKIPPED=4, HEAD=8, GRID=hip.EMA_GRID, WORK_HEAD=hip.EMA_WORK_HEAD,
                     MAX_MODELS=hip.EMA_MAX_MODELS).items():
        assert "#define CADRE_EMA_%s %d\n" % (k, v) in hdr, k
    assert "#define CADRE_MEAN_MAX_SOURCES %d\n" % hip.MEAN_MAX_SOURCES in hdr


def test_entry_points_refuse_bad_arguments():
    """What the host can see is refused with a status and a message before anything is launched (no device needed)."""
    from cadre_amd import hip
    L = hip.lib()
    ok = (64, 128, 256, 1, 512, 1024, None, None)          # params, ema, seg_off, n_models, state, work, stop, stream

    def ema(**kw):
        names = ("params", "ema", "seg_off", "n_models", "state", "work", "stop", "stream")
        return L.cadre_ema_update(*[kw.get(n, v) for n, v in zip(names, ok)])
    for kw in (dict(params=None), dict(ema=None), dict(seg_off=None), dict(state=None), dict(work=None), dict(n_models=-1),
               dict(n_models=4097), dict(state=516), dict(work=1028), dict(seg_off=260), dict(params=66), dict(ema=130), dict(stop=6)):
        assert ema(**kw) < 0, kw
        assert b"cadre_ema_update" in L.cadre_last_error(), kw
    assert L.cadre_arena_swap(None, None, 0, None) == 0                       # nothing to do
    assert L.cadre_arena_swap(64, 128, -1, None) < 0
    assert L.cadre_arena_swap(None, 128, 4, None) < 0 and L.cadre_arena_swap(64, None, 4, None) < 0
    assert L.cadre_arena_swap(66, 128, 4, None) < 0 and L.cadre_arena_swap(64, 130, 4, None) < 0
    assert b"cadre_arena_swap" in L.cadre_last_error()
    for a, b, n in ((64, 64, 1), (64, 68, 2), (68, 64, 2), (64, 64 + 4 * 99, 100), (4096, 64, 1009)):
        assert L.cadre_arena_swap(a, b, n, None) < 0, (a, b, n)
        assert b"overlap" in L.cadre_last_error()
    assert L.cadre_arena_mean(None, None, 1, None, 0, None) == 0              # nothing to do
    for args in ((64, 128, 0, 256, 4), (64, 128, 65, 256, 4), (64, 128, 1, 256, -1), (None, 128, 1, 256, 4), (64, None, 1, 256, 4),
                 (64, 128, 1, None, 4), (68, 128, 1, 256, 4), (64, 132, 1, 256, 4), (64, 128, 1, 258, 4)):
        assert L.cadre_arena_mean(*args, None) < 0, args
        assert b"cadre_arena_mean" in L.cadre_last_error(), args


# ----------------------------------------------------------------------------- soup
def _arena(**kw):
    d = dict(D=530, C=4, n_out=(33, 3), hid=128, ordinal_rank=None)
    d.update(kw)
    return types.SimpleNamespace(**d)


def test_soup_refuses_bad_weights():
    from cadre_amd.average import check_soup_weights, soup
    assert check_soup_weights(None, 4) == [0.25] * 4
    assert check_soup_weights((0.5, 0.3, 0.2), 3) == [0.5, 0.3, 0.2]
    assert check_soup_weights([1], 1) == [1.0]
    for bad in ((0.5, 0.5, 0.5), (0.5, 0.6), (1.5, -0.5), (float("nan"), 1.0), (float("inf"), 0.0), ("a", 1.0), (0.5,),
                (0.5, 0.5 + 1e-9), (True, 0.0)):
        with pytest.raises(ValueError, match="weights"):
            check_soup_weights(bad, 2 if len(bad) != 3 else 3)
    with pytest.raises(ValueError, match="1 .. 64 sources"):
        check_soup_weights(None, 0)
    with pytest.raises(ValueError, match="1 .. 64 sources"):
        check_soup_weights(None, 65)
    # through soup(): refused before any source is touched (the mock arenas hold no tensors)
    srcs = [_arena(), _arena()]
    with pytest.raises(ValueError, match="weights must sum to 1"):
        soup(srcs, weights=(0.7, 0.7), into=_arena())
    with pytest.raises(ValueError, match="into= is needed"):
        soup(srcs)
    # a destination whose arena holds the average (inside averaged_weights()) is refused, as capture and restore are
    from cadre_amd.hip import CadreHipError
    swapped = types.SimpleNamespace(arena=_arena(), learner=types.SimpleNamespace(_avg_swapped=True))
    with pytest.raises(CadreHipError, match="soup inside averaged_weights"):
        soup(srcs, into=swapped)
    with pytest.raises(CadreHipError, match="soup inside averaged_weights"):
        soup(srcs, into=_arena(_learner=types.SimpleNamespace(_avg_swapped=True)))


@pytest.mark.parametrize("field,value", [("D", 512), ("C", 2), ("n_out", (33, 5)), ("hid", 64), ("ordinal_rank", [None, [2, 0, 1]])])
def test_soup_refuses_layouts_by_field(field, value):
    from cadre_amd.average import soup
    with pytest.raises(ValueError, match="layout mismatch in %s: source 1" % field):
        soup([_arena(), _arena(**{field: value})], into=_arena())


def test_soup_checks_a_snapshot_files_layout():
    from cadre_amd.average import _layout_of, _snapshot_layout, check_soup_layouts
    ppo = types.SimpleNamespace(state_dict=lambda: {"control.linear.0.weight": torch.zeros(128, 530),
                                                    "control.linear.4.weight": torch.zeros(3, 128)})
    lstm = types.SimpleNamespace(state_dict=lambda: {"rnn.weight_hh": torch.zeros(4 * 530, 530)})
    lay = _snapshot_layout({"throttle_ppo_0": ppo, "throttle_ppo_1": ppo, "steer_lstm_1": lstm})
    assert lay == dict(D=530, hid=128, n_out={"throttle": 3}, C=2)
    check_soup_layouts([lay], _layout_of(_arena(C=2)))
    with pytest.raises(ValueError, match="layout mismatch in C"):
        check_soup_layouts([lay], _layout_of(_arena()))
    with pytest.raises(ValueError, match="layout mismatch in n_out"):
        check_soup_layouts([lay], _layout_of(_arena(C=2, n_out=(33, 4))))


# ----------------------------------------------------------------------------- snapshot and checkpoint metadata (mocks)
def _mock_agent(avg=None, swapped=False):
    arena = types.SimpleNamespace(D=530, C=4, n_out=(33, 3), hid=128, total=40, ordinal_rank=None, params=torch.zeros(40),
                                  step_dev=torch.zeros(1, dtype=torch.int32), exp_avg=None, exp_avg_sq=None)
    lrn = types.SimpleNamespace(_avg=avg, _avg_swapped=swapped, _hp=None, device_hyper=False)
    return types.SimpleNamespace(arena=arena, learner=lrn, vae_model=types.SimpleNamespace(fingerprint=None))


def _mock_avg(decay=0.99, warmup=True):
    return types.SimpleNamespace(decay=decay, warmup=warmup, ema=torch.zeros(40), state=torch.zeros(8 + 16, dtype=torch.float64))


def _state(with_ema, meta):
    from cadre_amd import checkpoint
    tensors = {"params": torch.zeros(40), "step_dev": torch.zeros(1, dtype=torch.int32)}
    if with_ema:
        tensors.update(ema=torch.ones(40), ema_state=torch.zeros(24, dtype=torch.float64))
    names = list(tensors)
    return dict(format_version=checkpoint.FORMAT_VERSION, names=names, tensors=tensors,
                digests=torch.zeros(len(names), dtype=torch.int64),
                layout=dict(D=530, C=4, n_out=[33, 3], hid=128, total=40, ordinal_rank=None), fingerprint=None, step=0,
                device_hyper=False, scaler=None, storages=[], weight_average=meta)


def test_checkpoint_metadata_knows_the_average():
    from cadre_amd import checkpoint
    assert checkpoint.FORMAT_VERSION == 1
    assert checkpoint._average_meta(_mock_agent().learner) is None
    assert checkpoint._average_meta(_mock_agent(_mock_avg(0.5, False)).learner) == dict(decay=0.5, warmup=False)
    # names: today's without an average, "ema" and "ema_state" behind the scaler's slot with one
    plain, avg = _mock_agent(), _mock_agent(_mock_avg())
    assert [n for n, _t in checkpoint._ranges(plain, [], None)] == ["params", "step_dev"]
    assert [n for n, _t in checkpoint._ranges(avg, [], None)] == ["params", "step_dev", "ema", "ema_state"]
    # _check: both directions are a ValueError naming ema, before anything could be written
    meta = dict(decay=0.99, warmup=True)
    assert checkpoint._check(plain, _state(False, None), [], None) == ["params", "step_dev"]
    assert checkpoint._check(avg, _state(True, meta), [], None) == ["params", "step_dev", "ema", "ema_state"]
    with pytest.raises(ValueError, match="mismatch in ema: the file has"):
        checkpoint._check(plain, _state(True, meta), [], None)
    with pytest.raises(ValueError, match="mismatch in ema: the file lacks"):
        checkpoint._check(avg, _state(False, None), [], None)
    with pytest.raises(ValueError, match="mismatch in weight_average"):
        checkpoint._check(_mock_agent(_mock_avg(0.9)), _state(True, meta), [], None)
    with pytest.raises(ValueError, match="mismatch in weight_average"):
        checkpoint._check(_mock_agent(_mock_avg(0.99, False)), _state(True, meta), [], None)
    half = _state(True, meta)
    del half["tensors"]["ema_state"]
    half["names"].remove("ema_state")
    half["digests"] = half["digests"][:3]
    with pytest.raises(ValueError, match="ema / ema_state"):
        checkpoint._check(avg, half, [], None)
    bad = _state(True, meta)
    bad["tensors"]["ema"] = torch.ones(41)
    with pytest.raises(ValueError, match="mismatch in ema"):
        checkpoint._check(avg, bad, [], None)
    # a file from before the key (no "weight_average" entry) reads as one without an average
    old = _state(False, None)
    del old["weight_average"]
    assert checkpoint._check(plain, old, [], None) == ["params", "step_dev"]


def test_snapshot_weights_argument():
    from cadre_amd import average
    from cadre_amd.hip import CadreHipError
    from ppo_agent.agent import CadreAgent
    sig = inspect.signature(CadreAgent.save_snapshot)
    assert list(sig.parameters) == ["self", "model_path", "fix_missing_lstm", "weights"]
    assert sig.parameters["weights"].default == "live" and sig.parameters["fix_missing_lstm"].default is False
    agent = _mock_agent()
    agent.averaged_weights = lambda: average.averaged_weights(agent)
    with pytest.raises(ValueError, match="weights='mean'"):
        CadreAgent.save_snapshot(agent, "unused.pt", weights="mean")
    with pytest.raises(CadreHipError, match="no weight average is set"):
        CadreAgent.save_snapshot(agent, "unused.pt", weights="average")
    nested = _mock_agent(_mock_avg(), swapped=True)
    with pytest.raises(CadreHipError, match="no nested entry"):
        with average.averaged_weights(nested):
            pass
    assert nested.learner._avg_swapped is True


def test_stats_text():
    from cadre_amd.average import average_stats_text
    from ppo_agent.average import WeightAverage, soup                        # noqa: F401  (the drop-in import path)
    st = dict(weight_average=dict(updates=5, skipped=2, decay=0.999, decay_used=0.4, distance={"steer_lstm_0": (0.5, 1e-3),
                                                                                                "steer_ppo_0": (0.1, 2e-3)}))
    text = average_stats_text(st)
    assert text.startswith(", average: 5 updates (2 skipped), decay 0.400000") and "2.0000e-03 (steer_ppo_0)" in text
