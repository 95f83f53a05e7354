"""Training checkpoints: stream-ordered capture of everything a resumed run needs, bit-exact restore.

`CadreAgent.save_snapshot` keeps the reference's on-disk format (pickled nn.Modules, a policy export).  A checkpoint is
the TRAINING state: the parameter arena, both Adam moments and the step count, the device hyper-parameter block, the
ReturnScaler block, every tensor of every storage with its cursor, and the global torch CPU generator.

    cap = capture(agent, rollouts, reward_scaler, episode=e)     # one launch on the compute stream, no host sync
    ...                                                          # the training stream goes on; the D2H copy runs beside it
    cap.save(path)                                               # waits for the copy only; atomic (temporary name + replace)
    restore(agent, load(path), rollouts, reward_scaler)          # verified against the stored digests before anything moves

capture() enqueues cadre_state_capture (csrc/checkpoint.hip): one launch copies all ranges into one staging buffer and
forms a 64-bit digest per range from the same read; a side stream then copies staging and digests to pinned host memory.
restore() uploads the ranges, runs the digest-only form of the same launch and compares before it writes anything.
The digest is an integrity check, not a cryptographic hash (include/cadre_hip.h).

Not captured: environment state (environments restart through reset()), the frozen encoder (identified by its
fingerprint: a mismatch is refused), several ranks, a sharded optimiser."""
import os

import numpy as np
import torch

from . import hip

FORMAT_VERSION = 1
LAYOUT_FIELDS = ("D", "C", "n_out", "hid", "total", "ordinal_rank")
STORAGE_TENSORS = ("_obs", "_hn", "_cn", "command", "rewards", "value_preds", "returns", "action_log_probs", "action",
                   "masks", "time_limits", "advantages", "_next")
STORAGE_GEOMETRY = ("num_steps", "mini_batch_num", "z_dims", "seq_length", "hid_size")
HEADS = ("steer", "throttle")
_DTYPES = {"float32": torch.float32, "float64": torch.float64, "int32": torch.int32, "int64": torch.int64}


def _rup(x, m):
    return (x + m - 1) // m * m


def reference_digest(words):
    """The digest of cadre_state_capture on the host: `words` = the range as a uint32 array (any array is viewed as
    its 32-bit words).  numpy uint64 array arithmetic wraps, which is the definition (mod 2^64).  Returns a Python int."""
    w = np.ascontiguousarray(words).reshape(-1).view(np.uint32).astype(np.uint64)
    i = np.arange(w.size, dtype=np.uint64)
    with np.errstate(over="ignore"):
        m = (np.uint64(2) * i + np.uint64(1)) * np.uint64(hip.DIGEST_K)
        return int(((w + np.uint64(1)) * m).sum(dtype=np.uint64))


def _pairs(rollouts):
    """rollouts: None, or [(steer_storage, throttle_storage), ...] per environment (one pair itself is accepted)."""
    if rollouts is None:
        return []
    rollouts = list(rollouts)
    if len(rollouts) == 2 and not isinstance(rollouts[0], (tuple, list)):
        rollouts = [tuple(rollouts)]
    for p in rollouts:
        if not isinstance(p, (tuple, list)) or len(p) != 2:
            raise ValueError("checkpoint: rollouts must be (steer, throttle) storage pairs")
    return [tuple(p) for p in rollouts]


def _ranges(agent, pairs, reward_scaler):
    """[(name, tensor)] in table order: everything that lives only in device memory of the running process."""
    a, lrn = agent.arena, agent.learner
    out = [("params", a.params)]
    if a.exp_avg is not None:
        out += [("exp_avg", a.exp_avg), ("exp_avg_sq", a.exp_avg_sq)]
    out.append(("step_dev", a.step_dev))
    if lrn.device_hyper:
        out.append(("hp", lrn._hp))
    if reward_scaler is not None:
        out.append(("scaler", reward_scaler.state))
    avg = getattr(lrn, "_avg", None)
    if avg is not None:                      # the weight average and its state block (cadre_amd.average.WeightAverage)
        out += [("ema", avg.ema), ("ema_state", avg.state)]
    for e, pair in enumerate(pairs):
        for h, s in zip(HEADS, pair):
            out += [("storage%d.%s.%s" % (e, h, k), getattr(s, k)) for k in STORAGE_TENSORS]
    dev = a.params.device
    for name, t in out:
        if t.device != dev:
            raise hip.CadreHipError("checkpoint: %s lives on %s, the arena on %s" % (name, t.device, dev))
        if not t.is_contiguous() or str(t.dtype).replace("torch.", "") not in _DTYPES:
            raise hip.CadreHipError("checkpoint: %s (%s, strides %s) is not a contiguous fp32 / fp64 / int32 / int64 tensor"
                                    % (name, t.dtype, t.stride()))
    return out


def _layout(arena):
    rank = arena.ordinal_rank
    return dict(D=int(arena.D), C=int(arena.C), n_out=[int(v) for v in arena.n_out], hid=int(arena.hid),
                total=int(arena.total), ordinal_rank=None if rank is None else [None if r is None else [int(x) for x in r]
                                                                                 for r in rank])


def _average_meta(lrn):
    """meta["weight_average"]: None, or the settings of the learner's weight average."""
    avg = getattr(lrn, "_avg", None)
    return None if avg is None else dict(decay=float(avg.decay), warmup=bool(avg.warmup))


def _fingerprint(agent):
    fp = getattr(agent.vae_model, "fingerprint", None)
    return None if fp is None else [v if isinstance(v, (int, float, str)) else str(v) for v in fp]


class _Stager:
    """Per-agent device and pinned-host staging of the checkpoint ranges: ONE device buffer and one pinned buffer, sized
    from the table and kept; the range tables are cached on the device, keyed by their records."""

    def __init__(self, device):
        self.device = device
        self.side = torch.cuda.Stream(device=device)
        self.staging = None        # device uint8
        self.host = None           # pinned uint8: what the last capture copied out
        self.digests = None        # device int64 (the uint64 bit patterns)
        self.host_digests = None   # pinned int64
        self.tables = {}
        self.done = None           # event on the side stream: the last capture's device-to-host copy has finished
        self.generation = 0

    def wait(self):
        if self.done is not None:
            self.done.synchronize()

    def room(self, nbytes, n_ranges):
        """Buffers for `nbytes` of staging and `n_ranges` digests (only ever grown; callers waited for the copy in flight)."""
        if self.staging is None or self.staging.numel() < nbytes:
            self.staging = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            self.host = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
        if self.digests is None or self.digests.numel() < n_ranges:
            self.digests = torch.zeros(n_ranges, dtype=torch.int64, device=self.device)
            self.host_digests = torch.zeros(n_ranges, dtype=torch.int64).pin_memory()

    def table(self, records):
        key = tuple(v for r in records for v in r)
        t = self.tables.get(key)
        if t is None:
            if len(self.tables) > 16:
                self.tables.clear()
            host = hip.capture_table(records, "cpu").pin_memory()       # pinned: the copy does not stall the host
            t = self.tables[key] = torch.empty_like(host, device=self.device)
            t.copy_(host, non_blocking=True)
            self._hosts = (getattr(self, "_hosts", []) + [host])[-17:]   # alive until the copy has run
        return t


def _stager(agent):
    st = agent.__dict__.get("_ckpt_stager")
    if st is None or st.device != agent.arena.params.device:
        st = agent._ckpt_stager = _Stager(agent.arena.params.device)
    return st


def write_state(state, path):
    """torch.save of a checkpoint dict under a temporary name in the directory of `path`, then os.replace."""
    path = os.fspath(path)
    tmp = "%s.tmp.%d" % (path, os.getpid())
    try:
        torch.save(state, tmp)
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return path


class Capture:
    """A checkpoint in flight: the device work is enqueued, the host-side values are taken.  `save(path)` writes it."""

    def __init__(self, stager, plan, meta, done, generation):
        self._stager, self._plan, self.meta, self._done, self._generation = stager, plan, meta, done, generation

    def ready(self):
        return self._done.query()

    def state(self):
        """The checkpoint as a dict of CPU tensors and plain containers (what save() writes).  Waits for the side
        stream's copy only."""
        st = self._stager
        if st.generation != self._generation:
            raise hip.CadreHipError("this capture's staging buffer was reused by a later capture or a restore: save a "
                                    "capture before the next one is taken")
        self._done.synchronize()
        tensors, names = {}, []
        for name, off, nbytes, dtype, shape in self._plan:
            t = st.host[off:off + nbytes].clone().view(_DTYPES[dtype]).reshape(shape)
            tensors[name] = t
            names.append(name)
        out = dict(self.meta)
        out.update(format_version=FORMAT_VERSION, names=names, tensors=tensors,
                   digests=st.host_digests[:len(names)].clone())
        return out

    def save(self, path):
        """Write the checkpoint to `path`: a temporary name in the same directory first, then os.replace (a reader never
        sees half a file).  Loads with torch.load(path, weights_only=True)."""
        return write_state(self.state(), path)


def capture(agent, rollouts=None, reward_scaler=None, episode=None, extra=None):
    """Enqueue a checkpoint of the training state on the current (compute) stream: ONE cadre_state_capture launch, an
    event, and on a side stream that waits for the event the asynchronous copy of staging and digests to pinned host
    memory.  The host is not synchronised (a second capture while the first one's copy is still in flight waits for that
    copy: there is one staging buffer).  Host-side values (step count, cursors, settings, the generator state, `episode`,
    `extra`) are read now.  Draws nothing from the global generator and builds no nn.Module.
    rollouts: [(steer_storage, throttle_storage), ...] per environment; extra: plain containers / CPU tensors only."""
    a, lrn = agent.arena, agent.learner
    if getattr(a, "_shard", None) is not None:
        raise hip.CadreHipError("checkpoint: this arena's Adam state is sharded over the data-parallel ranks (elements "
                                "[%d, %d)); the sharded optimiser is not captured" % a._shard)
    if getattr(lrn, "_avg_swapped", False):
        raise hip.CadreHipError("checkpoint: capture inside averaged_weights(): the arena holds the average")
    if not a.params.is_cuda:
        raise hip.CadreHipError("checkpoint: capture runs on the HIP device; the arena lives on %s" % a.params.device)
    if torch.cuda.is_current_stream_capturing():
        raise hip.CadreHipError("checkpoint: capture inside a stream capture (its copies would be baked into the graph)")
    pairs = _pairs(rollouts)
    ranges = _ranges(agent, pairs, reward_scaler)
    # staging offsets: 16-byte slots, each range shifted like its source so that both sides take the 16-byte path together
    plan, records, off = [], [], 0
    for name, t in ranges:
        nbytes = t.numel() * t.element_size()
        off = _rup(off, 16) + (t.data_ptr() & 15)
        plan.append((name, off, nbytes, str(t.dtype).replace("torch.", ""), [int(v) for v in t.shape]))
        records.append((t.data_ptr(), off, nbytes))
        off += nbytes
    st = _stager(agent)
    st.wait()                                  # the previous capture's copy still reads the staging buffer
    st.room(_rup(off, 16), len(records))
    table = st.table(records)
    st.generation += 1
    hip.state_capture(table, len(records), st.staging, st.digests)
    ev = torch.cuda.Event()
    ev.record()
    with torch.cuda.stream(st.side):
        st.side.wait_event(ev)
        st.host[:off].copy_(st.staging[:off], non_blocking=True)
        st.host_digests[:len(records)].copy_(st.digests[:len(records)], non_blocking=True)
        done = torch.cuda.Event()
        done.record(st.side)
    st.done = done
    # the compute stream may not rewrite staging / digests before the copy has read them: only capture() and restore()
    # write them, and both wait for `done` on the host first
    sc = reward_scaler
    meta = dict(
        layout=_layout(a), fingerprint=_fingerprint(agent), step=int(a.step),
        device_hyper=bool(lrn.device_hyper),
        adaptive=None if lrn._adaptive is None else [float(v) for v in lrn._adaptive],
        hp_host=None if lrn._hp_host is None else [float(v) for v in lrn._hp_host],
        hp_moved=bool(lrn._hp_moved),
        hyper=[float(lrn._clip), float(lrn._vc), float(lrn._cc), float(lrn._ec)],
        scaler=None if sc is None else dict(n_envs=int(sc.n_envs), gamma=float(sc.gamma), clip=float(sc.clip),
                                            epsilon=float(sc.epsilon), training=bool(sc.training)),
        storages=[[dict(step=int(s.step), tl_used=bool(s._tl_used), **{k: int(getattr(s, k)) for k in STORAGE_GEOMETRY})
                   for s in pair] for pair in pairs],
        rng_state=torch.get_rng_state().clone(),
        episode=None if episode is None else int(episode), extra=extra, weight_average=_average_meta(lrn))
    return Capture(st, plan, meta, done, st.generation)


def load(path):
    """The dict a Capture.save wrote (CPU tensors and plain containers; torch.load(..., weights_only=True))."""
    state = torch.load(os.fspath(path), map_location="cpu", weights_only=True)
    if not isinstance(state, dict) or "format_version" not in state:
        raise ValueError("%s is not a cadre_amd training checkpoint (no format_version)" % (path,))
    if state["format_version"] != FORMAT_VERSION:
        raise ValueError("checkpoint format_version %r; this build reads %d" % (state["format_version"], FORMAT_VERSION))
    missing = sorted({"names", "tensors", "digests", "layout", "step", "storages", "rng_state"} - set(state))
    if missing:
        raise ValueError("checkpoint %s lacks %r" % (path, missing))
    return state


def _check(agent, state, pairs, reward_scaler):
    """Layout metadata of the checkpoint against the live objects; ValueError naming the field.  Nothing is touched."""
    a = agent.arena
    mine = _layout(a)
    for f in LAYOUT_FIELDS:
        if state["layout"].get(f) != mine[f]:
            raise ValueError("checkpoint layout mismatch in %s: the file has %r, the agent %r" % (f, state["layout"].get(f), mine[f]))
    fp = _fingerprint(agent)
    if state.get("fingerprint") is not None and fp is not None and list(state["fingerprint"]) != list(fp):
        raise ValueError("checkpoint mismatch in fingerprint: it was taken with other encoder weights (the encoder is "
                         "frozen and not part of a checkpoint)")
    if getattr(a, "_shard", None) is not None:
        raise hip.CadreHipError("checkpoint: this arena's Adam state is sharded; restore needs the replicated optimiser")
    sc = state.get("scaler")
    if (sc is None) != (reward_scaler is None):
        raise ValueError("checkpoint mismatch in reward_scaler: the file %s one, the call %s one"
                         % ("has" if sc is not None else "lacks", "passes" if reward_scaler is not None else "lacks"))
    if sc is not None and int(sc["n_envs"]) != reward_scaler.n_envs:
        raise ValueError("checkpoint mismatch in reward_scaler.n_envs: the file has %d, the scaler %d"
                         % (sc["n_envs"], reward_scaler.n_envs))
    if len(state["storages"]) != len(pairs):
        raise ValueError("checkpoint mismatch in rollouts: the file has %d storage pairs, the call %d"
                         % (len(state["storages"]), len(pairs)))
    for e, (metas, pair) in enumerate(zip(state["storages"], pairs)):
        for h, m, s in zip(HEADS, metas, pair):
            for k in STORAGE_GEOMETRY:
                if int(m[k]) != int(getattr(s, k)):
                    raise ValueError("checkpoint mismatch in storage%d.%s.%s: the file has %r, the storage %r"
                                     % (e, h, k, m[k], getattr(s, k)))
    names, tensors = list(state["names"]), state["tensors"]
    if len(names) != state["digests"].numel() or set(names) != set(tensors):
        raise ValueError("checkpoint mismatch in names: %d names, %d digests, %d tensors"
                         % (len(names), state["digests"].numel(), len(tensors)))
    if ("exp_avg" in tensors) != ("exp_avg_sq" in tensors):
        raise ValueError("checkpoint mismatch in exp_avg / exp_avg_sq: only one of the moments is in the file")
    if bool(state.get("device_hyper")) != ("hp" in tensors):
        raise ValueError("checkpoint mismatch in device_hyper: the flag and the hp block disagree")
    # the destinations, by name (moments and hp block may not exist yet: they have the shapes of params / the block)
    lrn = agent.learner
    avg = getattr(lrn, "_avg", None)
    if ("ema" in tensors) != ("ema_state" in tensors):
        raise ValueError("checkpoint mismatch in ema / ema_state: only one of the two is in the file")
    if ("ema" in tensors) != (avg is not None):
        raise ValueError("checkpoint mismatch in ema: the file %s a weight average, the agent %s one (set_weight_average / "
                         "train_cfg.weight_average)" % ("has" if "ema" in tensors else "lacks", "has" if avg is not None else "lacks"))
    if state.get("weight_average") != _average_meta(lrn):
        raise ValueError("checkpoint mismatch in weight_average: the file was taken with %r, the agent's ema runs with %r"
                         % (state.get("weight_average"), _average_meta(lrn)))
    want = {"params": a.params, "exp_avg": a.params, "exp_avg_sq": a.params, "step_dev": a.step_dev}
    if avg is not None:
        want["ema"], want["ema_state"] = avg.ema, avg.state
    want["hp"] = lrn._hp if lrn._hp is not None else torch.empty(hip.HP_FIELDS, dtype=torch.float64, device="meta")
    if reward_scaler is not None:
        want["scaler"] = reward_scaler.state
    for e, pair in enumerate(pairs):
        for h, s in zip(HEADS, pair):
            for k in STORAGE_TENSORS:
                want["storage%d.%s.%s" % (e, h, k)] = getattr(s, k)
    need = {"params", "step_dev"} | {n for n in want if n.startswith("storage") or n == "scaler"}
    if not need <= set(names) or not set(names) <= set(want):
        raise ValueError("checkpoint mismatch in names: missing %r, unexpected %r"
                         % (sorted(need - set(names)), sorted(set(names) - set(want))))
    for n in names:
        t, d = tensors[n], want[n]
        if t.dtype != d.dtype or tuple(t.shape) != tuple(d.shape):
            raise ValueError("checkpoint mismatch in %s: the file has %s %s, the live tensor %s %s"
                             % (n, t.dtype, tuple(t.shape), d.dtype, tuple(d.shape)))
    return names


def restore(agent, state, rollouts=None, reward_scaler=None):
    """Put a loaded checkpoint back into `agent` (and the storages / scaler it was captured with).  Order:
    1. the layout metadata is checked (ValueError naming the field);
    2. every range is uploaded into the staging buffer, the digest-only launch runs over it and the digests are compared
       with the stored ones (CadreHipError naming the range) — up to here nothing of the live state has been written;
    3. the ranges are copied into place; step count, hyper-parameter mode and block, storage cursors and flags and the
       scaler's fields are set; everything derived from the parameters and the act-time window caches are dropped;
    4. the global generator state is set, last.
    A checkpoint without moments (taken before any optimiser step) leaves the arena where ensure_adam() starts: existing
    moments are zeroed in place (captured optimiser graphs hold their addresses)."""
    a, lrn = agent.arena, agent.learner
    if not a.params.is_cuda:
        raise hip.CadreHipError("checkpoint: restore runs on the HIP device; the arena lives on %s" % a.params.device)
    if getattr(lrn, "_avg_swapped", False):
        raise hip.CadreHipError("checkpoint: restore inside averaged_weights(): the arena holds the average")
    pairs = _pairs(rollouts)
    names = _check(agent, state, pairs, reward_scaler)
    tensors = state["tensors"]
    # ---- 2: upload + verify
    plan, records, off = [], [], 0
    for n in names:
        t = tensors[n]
        nbytes = t.numel() * t.element_size()
        off = _rup(off, 16)
        plan.append((n, off, nbytes))
        off += nbytes
    st = _stager(agent)
    st.wait()
    st.room(_rup(off, 16), len(names))
    st.generation += 1                          # (a capture not yet saved has lost its staging bytes)
    base = st.staging.data_ptr()
    for n, o, nbytes in plan:
        if nbytes:
            st.staging[o:o + nbytes].copy_(tensors[n].contiguous().reshape(-1).view(torch.uint8))
        records.append((base + o, o, nbytes))
    table = st.table(records)
    hip.state_capture(table, len(records), None, st.digests)
    got = st.digests[:len(names)].cpu()
    want = state["digests"].to(torch.int64).reshape(-1)
    for k, n in enumerate(names):
        if int(got[k]) != int(want[k]):
            raise hip.CadreHipError("checkpoint: range %s does not verify (digest %016x, stored %016x): the file is "
                                    "damaged; nothing was restored" % (n, int(got[k]) & (2 ** 64 - 1), int(want[k]) & (2 ** 64 - 1)))
    # ---- 3: into place
    has_moments = "exp_avg" in tensors
    if has_moments:
        a.ensure_adam()
    elif a.exp_avg is not None:
        a.exp_avg.zero_()
        a.exp_avg_sq.zero_()
    hp_on = bool(state.get("device_hyper"))
    lrn.set_device_hyper(hp_on)                 # (off also switches a running controller off)
    dest = {"params": a.params, "exp_avg": a.exp_avg, "exp_avg_sq": a.exp_avg_sq, "step_dev": a.step_dev, "hp": lrn._hp}
    if reward_scaler is not None:
        dest["scaler"] = reward_scaler.state
    avg = getattr(lrn, "_avg", None)
    if avg is not None:
        dest["ema"], dest["ema_state"] = avg.ema, avg.state
        avg._decay_set = None                  # (the block's decay is the file's now)
    for e, pair in enumerate(pairs):
        for h, s in zip(HEADS, pair):
            for k in STORAGE_TENSORS:
                dest["storage%d.%s.%s" % (e, h, k)] = getattr(s, k)
    for n, o, nbytes in plan:
        d = dest[n]
        if nbytes:
            d.copy_(st.staging[o:o + nbytes].view(d.dtype).view(d.shape))
    a.step = int(state["step"])
    clip, vc, cc, ec = (float(v) for v in state["hyper"])
    if hp_on:
        moved = (lrn._clip, lrn._vc, lrn._cc, lrn._ec) != (clip, vc, cc, ec)
        lrn._hp_host[:] = np.asarray(state["hp_host"], dtype=np.float64)
        lrn._clip, lrn._vc, lrn._cc, lrn._ec = clip, vc, cc, ec
        lrn._hp_moved = bool(lrn._hp_moved or moved or state.get("hp_moved"))
        ad = state.get("adaptive")
        lrn._adaptive = None if ad is None else tuple(float(v) for v in ad)
    else:
        lrn.clip, lrn.vc, lrn.cc, lrn.ec = clip, vc, cc, ec      # (a changed value drops the by-value update graphs)
    for metas, pair in zip(state["storages"], pairs):
        for m, s in zip(metas, pair):
            s.step, s._tl_used = int(m["step"]), bool(m["tl_used"])
    if reward_scaler is not None:
        sc = state["scaler"]
        reward_scaler.gamma, reward_scaler.clip = float(sc["gamma"]), float(sc["clip"])
        reward_scaler.epsilon, reward_scaler.training = float(sc["epsilon"]), bool(sc["training"])
    # everything derived from the parameters (as _SectionStats.finish does), and the act-time window caches: the first
    # act re-encodes its whole window, which by batch invariance gives the same feature bits
    lrn._wp_key = None
    lrn._adam_fresh = None
    agent._cache = None
    agent._vec = None
    # ---- 4
    torch.set_rng_state(state["rng_state"])
    return state.get("episode")
