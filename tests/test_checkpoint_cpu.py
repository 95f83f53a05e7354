"""CPU: the checkpoint digest's reference and its properties (the GPU tests lean on it), the exported symbols, the
train_cfg keys, and the file format."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import checkpoint_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------- the reference digest
def test_reference_wraps_and_matches_python_integers():
    r = np.random.RandomState(0)
    w = ref.random_words(r, 300)
    want = sum((int(x) + 1) * (((2 * i + 1) * 0x9E3779B97F4A7C15) % 2 ** 64) for i, x in enumerate(w)) % 2 ** 64
    assert ref.digest(w) == want
    assert ref.digest(np.zeros(0, np.uint32)) == 0
    assert ref.digest(w.view(np.float32)) == want            # any 4-byte view of the same bytes


def test_sum_is_order_independent():
    r = np.random.RandomState(1)
    t = ref.terms(ref.random_words(r, 4099))
    want = int(t.sum(dtype=np.uint64))
    for _ in range(5):
        assert int(t[r.permutation(t.size)].sum(dtype=np.uint64)) == want
    # partial sums of lanes / waves / workgroups, combined in any order
    for lanes in (64, 256, 1000):
        parts = np.array([int(t[k::lanes].sum(dtype=np.uint64)) for k in range(lanes)], dtype=np.uint64)
        assert int(parts[r.permutation(lanes)].sum(dtype=np.uint64)) == want


def test_every_single_bit_flip_of_257_words_changes_the_digest():
    r = np.random.RandomState(2)
    w = ref.random_words(r, 257)
    d0 = ref.digest(w)
    seen = set()
    for j in range(257):
        for b in range(32):
            v = w.copy()
            v[j] ^= np.uint32(1 << b)
            d = ref.digest(v)
            assert d != d0, (j, b)
            seen.add(d)
    assert len(seen) == 257 * 32                              # (and no two flips collide)


def test_swapping_two_unequal_words_changes_the_digest():
    r = np.random.RandomState(3)
    w = ref.random_words(r, 257)
    d0 = ref.digest(w)
    pairs = [(j, j + 1) for j in range(256)] + [(0, 256)] + [tuple(r.permutation(257)[:2]) for _ in range(200)]
    for a, b in pairs:
        if w[a] == w[b]:
            continue
        v = w.copy()
        v[a], v[b] = w[b], w[a]
        assert ref.digest(v) != d0, (a, b)


def test_length_counts():
    ds = [ref.digest(np.zeros(n, np.uint32)) for n in range(0, 300)]
    assert len(set(ds)) == len(ds)
    for n in (0, 1, 63, 64, 257, 4097):
        assert ref.digest(np.zeros(n, np.uint32)) != ref.digest(np.zeros(n + 1, np.uint32))


def test_package_digest_equals_the_reference():
    from cadre_amd import checkpoint
    r = np.random.RandomState(4)
    for n in (0, 1, 5, 257, 4097):
        w = ref.random_words(r, n)
        assert checkpoint.reference_digest(w) == ref.digest(w)


# ----------------------------------------------------------------------------- symbols
def test_symbols_exported_and_abi_unchanged():
    from cadre_amd import build, hip
    hdr = open(os.path.join(ROOT, "include", "cadre_hip.h")).read()
    declared = set(re.findall(r"\b(cadre_[a-z0-9_]+)\s*\(", hdr))
    L = ctypes.CDLL(hip.LIB_PATH)
    assert "cadre_state_capture" in declared and "cadre_state_capture" in hip.SYMBOLS and hasattr(L, "cadre_state_capture")
    assert "checkpoint.hip" in build.SOURCES
    assert hip.lib().cadre_abi_version() == hip.ABI_VERSION == 15
    assert "NOT a" in hdr and "cryptographic hash" in hdr    # the header says what the digest is not
    import ppo_agent.checkpoint as shim
    from cadre_amd import checkpoint
    for name in ("capture", "Capture", "load", "restore"):
        assert getattr(shim, name) is getattr(checkpoint, name)


def test_entry_point_refuses_bad_arguments():
    """What the host can see is refused with a status before anything is launched (no device needed)."""
    from cadre_amd import hip
    L = hip.lib()
    assert L.cadre_state_capture(None, 0, None, None, None) == 0
    assert L.cadre_state_capture(None, 1, None, None, None) < 0            # null table
    assert L.cadre_state_capture(8, -1, None, 8, None) < 0
    assert L.cadre_state_capture(8, 65536, None, 8, None) < 0
    assert L.cadre_state_capture(8, 1, None, None, None) < 0               # null digests
    assert L.cadre_state_capture(8, 1, 2, 8, None) < 0                     # staging off a 4-byte boundary
    assert b"cadre_state_capture" in L.cadre_last_error()


def test_capture_table_refuses_ranges_that_are_not_words():
    from cadre_amd import hip
    for rec in [(256, 0, 6), (256, 0, -4), (258, 0, 8), (256, 2, 8), (256, -4, 8), (0, 0, 8)]:
        with pytest.raises(hip.CadreHipError, match="multiple of 4"):
            hip.capture_table([(512, 0, 16), rec], "cpu")
    t = hip.capture_table([(512, 0, 16), (0, 16, 0), (1028, 20, 4)], "cpu")
    assert t.dtype == torch.int64 and t.tolist() == [[512, 0, 16], [0, 16, 0], [1028, 20, 4]]


# ----------------------------------------------------------------------------- train_cfg keys
class _World(object):
    def __init__(self, n):
        self.n = n

    def dist_world(self):
        return self.n


def test_train_cfg_keys():
    from cadre_amd import hip
    from ppo_agent.train import _checkpointing
    assert _checkpointing({}) == (None, None)
    assert _checkpointing({"checkpoint_interval": None, "resume_from": None}) == (None, None)
    assert _checkpointing({"checkpoint_interval": 0}) == (None, None)
    assert _checkpointing({"checkpoint_interval": 3, "resume_from": "a/b.pt"}) == (3, "a/b.pt")
    assert _checkpointing({"checkpoint_interval": np.int64(2)}, _World(1)) == (2, None)
    for bad in (-1, 1.5, True, "2", [1]):
        with pytest.raises(ValueError, match="checkpoint_interval"):
            _checkpointing({"checkpoint_interval": bad})
    for bad in (3, "", True, ["x"]):
        with pytest.raises(ValueError, match="resume_from"):
            _checkpointing({"resume_from": bad})
    with pytest.raises(hip.CadreHipError, match="checkpoint_interval needs a single rank"):
        _checkpointing({"checkpoint_interval": 1}, _World(2))
    with pytest.raises(hip.CadreHipError, match="resume_from needs a single rank"):
        _checkpointing({"resume_from": "x.pt"}, _World(2))
    assert _checkpointing({"checkpoint_interval": 0}, _World(2)) == (None, None)       # off: nothing to refuse


# ----------------------------------------------------------------------------- file format
def _hand_built_state():
    from cadre_amd import checkpoint
    r = np.random.RandomState(5)
    tensors = {"params": torch.from_numpy(ref.random_words(r, 40).view(np.float32).copy()),
               "step_dev": torch.tensor([7], dtype=torch.int32),
               "scaler": torch.from_numpy(r.standard_normal(12)),
               "storage0.steer.action": torch.from_numpy(r.randint(0, 33, (9, 1)).astype(np.int64))}
    names = list(tensors)
    digs = torch.tensor([ref.as_i64(ref.digest(tensors[n].numpy())) for n in names], dtype=torch.int64)
    return dict(format_version=checkpoint.FORMAT_VERSION, names=names, tensors=tensors, digests=digs,
                layout=dict(D=530, C=4, n_out=[33, 3], hid=128, total=40, ordinal_rank=[None, [2, 0, 1]]),
                fingerprint=["torch.float32", 84, 84, 1.5], step=7, device_hyper=False, adaptive=[0.01, 1.5, 1e-5, 1e-2],
                hp_host=[3e-4, float("nan")], hp_moved=False, hyper=[0.1, 0.1, 1.0, 0.01],
                scaler=dict(n_envs=1, gamma=0.99, clip=10.0, epsilon=1e-8, training=True),
                storages=[[dict(step=3, tl_used=True, num_steps=8), dict(step=3, tl_used=False, num_steps=8)]],
                rng_state=torch.get_rng_state(), episode=1, extra={"note": "x", "k": [1, 2.5, None]})


def _same(a, b):
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape and \
            torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, float) and a != a:
        return isinstance(b, float) and b != b
    return type(a) is type(b) and a == b


def test_file_round_trip_weights_only(tmp_path):
    from cadre_amd import checkpoint
    state = _hand_built_state()
    path = tmp_path / "ckpt_1.pt"
    assert checkpoint.write_state(state, path) == str(path)
    assert os.listdir(str(tmp_path)) == ["ckpt_1.pt"]                     # the temporary name is gone
    raw = torch.load(str(path), weights_only=True)
    assert _same(raw, state)
    back = checkpoint.load(path)
    assert _same(back, state)
    for n, d in zip(back["names"], back["digests"].tolist()):             # NaN payloads and -0.0 survive the file
        assert ref.as_i64(ref.digest(back["tensors"][n].numpy())) == d
    # a file that is no checkpoint, or another version
    torch.save({"x": 1}, str(tmp_path / "other.pt"))
    with pytest.raises(ValueError, match="format_version"):
        checkpoint.load(tmp_path / "other.pt")
    checkpoint.write_state(dict(state, format_version=99), tmp_path / "v99.pt")
    with pytest.raises(ValueError, match="format_version"):
        checkpoint.load(tmp_path / "v99.pt")


def test_failed_write_keeps_the_old_file(tmp_path):
    from cadre_amd import checkpoint
    path = tmp_path / "ckpt.pt"
    checkpoint.write_state(_hand_built_state(), path)
    before = open(str(path), "rb").read()
    with pytest.raises(Exception):
        checkpoint.write_state({"f": lambda: 0}, path)                    # not picklable: torch.save fails half way
    assert open(str(path), "rb").read() == before and os.listdir(str(tmp_path)) == ["ckpt.pt"]
