"""PPG auxiliary phase: critic epochs on past rollouts under a KL clone of the policy.

Phasic Policy Gradient (Cobbe et al. 2020; the shared-trunk variant of its section 3.5): every `interval` rollouts a few
extra epochs run over ALL rows of those rollouts.  The critic is regressed at full weight on the value targets the PPO
update saw, and the policy is held where it was by a KL term against its own distributions, recorded at the start of the
phase.  More gradient steps per simulator step, no extra environment interaction, no policy drift.  The pieces:

    buf = AuxBuffer(agent, slots=interval, rows_per_slot=num_envs * num_steps)
    buf.append(rollouts)                       # after each learner section
    if buf.full:
        aux_phase(agent, buf, epochs=2, minibatch=64, shared_grad_buffers=sgb, optimizer=None, max_grad_norm=250.0, lr=3e-4)
        buf.clear()

The step is the update's own launch chain with the loss switched to cadre_aux_loss (CadreAgent.aux_from_storages); the
optimiser is the run's own (chief_step): Adam moments and step count continue.  train_cfg["aux_phase"] (aux_config) wires
it into train() / train_vec().
"""
import numpy as np
import torch

from . import hip

AUX_KEYS = ("interval", "epochs", "minibatch", "beta_clone", "value_coeff", "seed")
# accepted beside them; in the parsed dict only when given (absent: the dict, and the buffer, are what they always were)
AUX_FRAME_KEYS = ("frames_per_row",)


def slot_rows(slot, rows_per_slot):
    """[first row, end row) of slot `slot`."""
    return slot * rows_per_slot, (slot + 1) * rows_per_slot


def record_starts(R, B):
    """First rows of the record pass's minibatches: rows in order, B at a time; when B does not divide R the last
    minibatch is the last B rows (it overlaps the one before and rewrites identical values)."""
    R, B = int(R), int(B)
    if B < 1 or B > R:
        raise ValueError("aux_phase: minibatch %d for a buffer of %d rows" % (B, R))
    starts = list(range(0, R - B + 1, B))
    if starts[-1] + B < R:
        starts.append(R - B)
    return starts


def epoch_permutation(seed, rank, episode, epoch, B, R):
    """The row order of one training epoch: a permutation of R rows that is a pure function of its key, drawn from a private
    torch.Generator seeded through np.random.SeedSequence (as DemoMixer.indices) — never from the global CPU generator,
    whose stream belongs to the PPO sampler and act().  A resumed run draws what the uninterrupted run would have drawn."""
    key = [int(seed) & 0xFFFFFFFFFFFFFFFF, int(rank), int(episode), int(epoch), int(B), int(R)]
    if min(key[1:]) < 0 or int(B) < 1 or int(R) < 1:
        raise ValueError("epoch_permutation: rank=%r, episode=%r, epoch=%r, B=%r, R=%r" % (rank, episode, epoch, B, R))
    lo, hi = np.random.SeedSequence(key).generate_state(2, dtype=np.uint32)
    g = torch.Generator()
    g.manual_seed(((int(hi) << 32) | int(lo)) & 0x7FFFFFFFFFFFFFFF)
    return torch.randperm(int(R), generator=g)


class AuxBuffer(object):
    """The rows of the last `slots` learner sections on the device, `rows_per_slot` rows each (all environments of a
    section: num_envs * num_steps), R = slots * rows_per_slot.  They live in ONE pair of ordinary RolloutStorage objects
    (`steer`, `throttle`) with num_steps = R that share one `_obs` (both heads see the same windows, as DemoSet._storages),
    beside `table` float32 [2][R][64], the distributions cadre_aux_record writes.  Per row: the window, the LSTM state it
    started from, the command, and per head `returns` — the value targets exactly as the critic saw them in the PPO update,
    including any reward scaling.  Memory: about 17 KB per row (8 frames x `_ldo` floats of window, two LSTM states) plus
    512 B of table.
    `frames_per_row` (None: the buffer above): a finite number in [1 / S, S].  The two storages are then FrameStorages
    (cadre_amd.frames) that share a frame table of ceil(R * frames_per_row) rows and the window ids: `append` packs each
    section's rows into it (cadre_frames_scan / cadre_frames_copy — a window that slid, or that a reset filled with one
    frame, adds ONE frame: sliding rollouts need 1 frame per row, and up to S - 1 more per storage for a first window of S
    different frames) and refuses a section whose frames do not fit.  Every step of the phase reads the same bits either way."""

    def __init__(self, agent, slots, rows_per_slot, frames_per_row=None, _device=None):
        for name, v in (("slots", slots), ("rows_per_slot", rows_per_slot)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
                raise ValueError("AuxBuffer: %s must be an integer >= 1 (got %r)" % (name, v))
        self.slots, self.rows_per_slot = int(slots), int(rows_per_slot)
        self.R = self.slots * self.rows_per_slot
        self.filled = 0                # slots appended since the last clear()
        dev = agent.arena.device if _device is None else _device
        self.frames_per_row = frames_per_row
        self.frames_used = 0           # frame-table form: the bump pointer (frames in use since the last clear())
        if frames_per_row is None:
            from .imitation import DemoSet
            self.steer, self.throttle = DemoSet._storages(self.R, agent.lstm_input, agent.learner.S, agent.lstm_input, 0.0, dev)
        else:
            from .frames import capacity_for, frame_pair
            cap = capacity_for(self.R, frames_per_row, agent.learner.S)
            self.steer, self.throttle = frame_pair(self.R, agent.lstm_input, agent.learner.S, agent.lstm_input, 0.0, dev,
                                                   frame_capacity=cap)
        self.table = torch.zeros(2, self.R, 64, device=dev)

    @property
    def full(self):
        return self.filled == self.slots

    def clear(self):
        self.filled = 0
        self.frames_used = 0
        if self.frames_per_row is not None:
            self.steer.n_frames = self.throttle.n_frames = 0

    def append(self, rollouts):
        """rollouts = [(steer_storage, throttle_storage), ...] of one learner section, after it ran (their `returns` hold
        the section's value targets): device-to-device copies into the next slot.  Not a hot path.
        Frame-table form: the windows are packed instead of copied (frames.scan_frames / copy_frames: the scan, ONE small
        read-back of the storages' frame counts, the copy at the bump pointer).  A section that needs more frames than are left raises
        ValueError naming both numbers before anything of the buffer is written."""
        if self.full:
            raise ValueError("AuxBuffer.append: all %d slots are filled (run the phase, then clear())" % self.slots)
        n = sum(int(s.num_steps) for s, _t in rollouts)
        if n != self.rows_per_slot:
            raise ValueError("AuxBuffer.append: %d rows for a slot of %d" % (n, self.rows_per_slot))
        lo, _hi = slot_rows(self.filled, self.rows_per_slot)
        for s, t in rollouts:
            if t.num_steps != s.num_steps or (s._ldo, s.seq_length, s._ldh) != (self.steer._ldo, self.steer.seq_length, self.steer._ldh):
                raise ValueError("AuxBuffer.append: a storage pair whose geometry differs from the buffer's")
        if self.frames_per_row is not None:
            self._append_frames([s for s, _t in rollouts], lo)
        for s, t in rollouts:
            T = int(s.num_steps)
            if self.frames_per_row is None:
                self.steer._obs[lo:lo + T].copy_(s._obs[:T])
            for src, dst in ((s, self.steer), (t, self.throttle)):
                dst._hn[lo:lo + T].copy_(src._hn[:T])
                dst._cn[lo:lo + T].copy_(src._cn[:T])
                dst.command[lo:lo + T].copy_(src.command[:T])
                dst.returns[lo:lo + T].copy_(src.returns[:T])
            lo += T
        self.filled += 1

    def _append_frames(self, storages, lo):
        """The windows of one section into the frame table from row `lo`: storages of one length in one scan, else one by
        one.  All scans run, and all counts are known, before the first copy."""
        from . import frames as fr
        one_T = all(int(s.num_steps) == int(storages[0].num_steps) for s in storages)
        groups = [storages] if one_T else [[s] for s in storages]
        scans, need = [], 0
        for g in groups:
            s0 = g[0]
            if any(getattr(s, "_obs", None) is None for s in g):
                raise ValueError("AuxBuffer.append: the sections' storages are materialised RolloutStorages")
            scan = fr.scan_frames([s._obs for s in g], int(s0.num_steps), s0.seq_length, s0._ldo, s0.z_dims)
            counts = scan[3].cpu().tolist()                   # (the one small read-back per scan)
            scans.append((g, scan, counts))
            need += sum(counts)
        cap = self.steer._frames.shape[0]
        if need > cap - self.frames_used:
            raise ValueError("AuxBuffer.append: this section needs %d frames, %d of the buffer's %d are available "
                             "(frames_per_row=%r: raise it)" % (need, cap - self.frames_used, cap, self.frames_per_row))
        frame = self.frames_used
        for g, scan, counts in scans:
            s0, T = g[0], int(g[0].num_steps)
            base, row0 = [], []
            for c in counts:
                base.append(frame)
                row0.append(lo)
                frame += c
                lo += T
            fr.copy_frames(scan, T, s0.seq_length, s0._ldo, s0.z_dims, base, self.steer._frames, self.steer._win, row0)
        self.frames_used = frame
        self.steer.n_frames = self.throttle.n_frames = frame

    def entry(self, idx):
        """The one-entry `entry` argument of CadreAgent.aux_record_from_storages / aux_from_storages for rows `idx` (a CPU
        int64 tensor); the advantage slot is the storages' own zeros (the auxiliary loss does not read it)."""
        return [(self.steer, idx, self.steer.advantages, self.throttle, idx, self.throttle.advantages)]


def aux_phase(agent, buffer, epochs, minibatch, shared_grad_buffers, optimizer, max_grad_norm, lr, beta_clone=1.0,
              value_coeff=1.0, seed=0, rank=0, episode=0, log=None):
    """The auxiliary phase on the filled rows of `buffer` (an AuxBuffer; every slot must be filled).
    (a) Record pass: the current policy's distributions of all R rows go to buffer.table, rows in order in minibatches of
    B = `minibatch` (record_starts).  (b) `epochs` training epochs: each one permutation of the R rows (epoch_permutation,
    stateless, keyed by (seed, rank, episode, epoch, B, R)) cut into R // B steps with the tail dropped; each step is
    CadreAgent.aux_from_storages, shared_grad_buffers.add_gradient, chief_step(...) exactly as a PPO step of the learner
    section — the run's own optimiser, whose Adam moments and step count continue.  One host sync per epoch.
    Returns the per-epoch records: dicts with epoch, steps and the (steer, throttle) pairs kl, kl_max, value_error (mean
    |v - R|), value_loss (mean (v - R)^2) and entropy — means over the epoch's steps (kl_max: the maximum).  `log`: a callable
    (or an object with .log) that gets one line per epoch."""
    from .ppo_agent.chief import chief_step
    B, R = int(minibatch), buffer.R
    if not buffer.full:
        raise ValueError("aux_phase: %d of the buffer's %d slots are filled" % (buffer.filled, buffer.slots))
    starts = record_starts(R, B)
    if isinstance(epochs, bool) or int(epochs) != epochs or int(epochs) < 0:
        raise ValueError("aux_phase: epochs=%r" % (epochs,))
    F, dev = hip.AUX_STATS_FIELDS, agent.arena.device
    emit = None if log is None else (log.log if hasattr(log, "log") else log)
    order = torch.arange(R)
    for lo in starts:
        agent.aux_record_from_storages(buffer.entry(order[lo:lo + B]), buffer.table)
    records = []
    steps = R // B
    for epoch in range(int(epochs)):
        perm = epoch_permutation(seed, rank, episode, epoch, B, R)
        rows = torch.zeros(steps, 2, F, device=dev)
        for i in range(steps):
            agent.aux_from_storages(buffer.entry(perm[i * B:(i + 1) * B]), buffer.table, stats_row=rows[i], sync=False,
                                    beta_clone=beta_clone, value_coeff=value_coeff)
            shared_grad_buffers.add_gradient(agent.model_dict)
            chief_step(shared_grad_buffers, optimizer, max_grad_norm, lr=lr, zero_grads=False)
        host = torch.cat([rows.mean(0), rows[:, :, 1].max(0).values.view(2, 1)], 1).cpu().tolist()     # the epoch's one sync
        rec = dict(epoch=epoch, steps=steps, kl=(host[0][0], host[1][0]), kl_max=(host[0][F], host[1][F]),
                   value_error=(host[0][2], host[1][2]), entropy=(host[0][3], host[1][3]), value_loss=(host[0][4], host[1][4]))
        records.append(rec)
        if emit is not None:
            emit(aux_line(episode, rec))
    return records


def aux_line(episode, rec):
    """The log line of one epoch of the phase."""
    return ("Episode: {}, aux epoch: {}, kl: {:.6f}/{:.6f}, max kl: {:.6f}/{:.6f}, value error: {:.4f}/{:.4f}, "
            "value loss: {:.4f}/{:.4f}").format(episode, rec["epoch"], *(rec["kl"] + rec["kl_max"] + rec["value_error"]
                                                                       + rec["value_loss"]))


def aux_summary_line(episode, records):
    """The extra `log_stats` line of a run with train_cfg.aux_phase: first against last epoch of the phase."""
    a, b = records[0], records[-1]
    return ("Episode: {}, aux phase: {} epochs x {} steps, value error: {:.4f}/{:.4f} -> {:.4f}/{:.4f}, kl: {:.6f}/{:.6f}, "
            "entropy: {:.4f}/{:.4f}").format(episode, len(records), a["steps"], *(a["value_error"] + b["value_error"] + b["kl"]
                                                                                + b["entropy"]))


# ----------------------------------------------------------------------------- train_cfg["aux_phase"]
def _is_number(v):
    return (not isinstance(v, bool)) and isinstance(v, (int, float, np.integer, np.floating)) and bool(np.isfinite(v))


def _is_int(v):
    return (not isinstance(v, bool)) and isinstance(v, (int, np.integer))


def aux_config(train_cfg_value):
    """train_cfg["aux_phase"]: absent / None -> None (nothing runs, nothing is allocated, nothing is drawn); else a dict
    {"interval": rollouts per phase (required, an integer >= 1), "epochs" (2), "minibatch" (None = the PPO minibatch size),
    "beta_clone" (1.0), "value_coeff" (1.0), "seed" (0)} -> the dict with defaults filled in.  "frames_per_row" (optional;
    AuxBuffer(frames_per_row=): a finite number in [1 / S, S], S the window length — checked here against the widest window
    the kernels take, 16, and against the agent's S when the buffer is built) stays in the dict only when given."""
    cfg = train_cfg_value
    if cfg is None:
        return None
    if not isinstance(cfg, dict):
        raise ValueError("train_cfg.aux_phase: expected None or a dict (got %r)" % (cfg,))
    unknown = sorted(set(cfg) - set(AUX_KEYS + AUX_FRAME_KEYS))
    if unknown or "interval" not in cfg:
        raise ValueError("train_cfg.aux_phase: needs interval; known keys %r (unknown: %r)" % (AUX_KEYS, unknown))
    interval, epochs, mb, seed = cfg["interval"], cfg.get("epochs", 2), cfg.get("minibatch"), cfg.get("seed", 0)
    if not _is_int(interval) or interval < 1:
        raise ValueError("train_cfg.aux_phase: interval must be an integer >= 1 (got %r)" % (interval,))
    if not _is_int(epochs) or epochs < 0:
        raise ValueError("train_cfg.aux_phase: epochs must be an integer >= 0 (got %r)" % (epochs,))
    if mb is not None and (not _is_int(mb) or mb < 1):
        raise ValueError("train_cfg.aux_phase: minibatch must be None or an integer >= 1 (got %r)" % (mb,))
    if not _is_int(seed):
        raise ValueError("train_cfg.aux_phase: seed must be an integer (got %r)" % (seed,))
    for name in ("beta_clone", "value_coeff"):
        if name in cfg and not _is_number(cfg[name]):
            raise ValueError("train_cfg.aux_phase: %s=%r is not a finite number" % (name, cfg[name]))
    out = dict(interval=int(interval), epochs=int(epochs), minibatch=None if mb is None else int(mb),
               beta_clone=float(cfg.get("beta_clone", 1.0)), value_coeff=float(cfg.get("value_coeff", 1.0)), seed=int(seed))
    if "frames_per_row" in cfg:
        fpr = cfg["frames_per_row"]
        if fpr is not None:
            from .frames import MAX_S, frames_per_row_ok
            if not frames_per_row_ok(fpr):
                raise ValueError("train_cfg.aux_phase: frames_per_row must be None or a finite number in [1/S, S] for a window "
                                 "of S <= %d frames (got %r)" % (MAX_S, fpr))
            fpr = float(fpr)
        out["frames_per_row"] = fpr
    return out


def check_intervals(interval, checkpoint_interval, first_episode=0):
    """The checkpoint rule: a capture (after every checkpoint_interval-th episode) must fall on an episode whose phase has
    just run and emptied the buffer, so checkpoint_interval is a multiple of `interval` — the checkpoint format then does
    not change and a resumed run continues with the bits of the uninterrupted one.  For the same reason a run resumes at an
    episode that is a multiple of `interval`."""
    if checkpoint_interval is not None and int(checkpoint_interval) % int(interval):
        raise ValueError("train_cfg.aux_phase: checkpoint_interval %d is not a multiple of interval %d (a capture would "
                         "have to hold the buffer's rows)" % (checkpoint_interval, interval))
    if int(first_episode) % int(interval):
        raise ValueError("train_cfg.aux_phase: the run resumes at episode %d, not a multiple of interval %d (the rows "
                         "of the episodes before it are gone)" % (first_episode, interval))


class AuxRunner(object):
    """train_cfg["aux_phase"] inside train() / train_vec(): after_section(episode, ...) appends the section's rollouts and,
    when (episode + 1) % interval == 0, runs the phase and empties the buffer.  The buffer is allocated at the first append."""

    def __init__(self, agent, cfg, rank=0):
        self.agent, self.cfg, self.rank = agent, cfg, int(rank)
        self.buffer = None
        self.records = None            # the records of the phase that ran last

    def after_section(self, episode, rollouts, ppo_minibatch, shared_grad_buffers, optimizer, max_grad_norm, lr, log=None):
        """Returns the phase's records when it ran after this episode, else None."""
        cfg = self.cfg
        if self.buffer is None:
            self.buffer = AuxBuffer(self.agent, cfg["interval"], sum(int(s.num_steps) for s, _t in rollouts),
                                    frames_per_row=cfg.get("frames_per_row"))
        self.buffer.append(rollouts)
        if (episode + 1) % cfg["interval"]:
            return None
        B = ppo_minibatch if cfg["minibatch"] is None else cfg["minibatch"]
        try:
            self.records = aux_phase(self.agent, self.buffer, cfg["epochs"], B, shared_grad_buffers, optimizer, max_grad_norm,
                                     lr, beta_clone=cfg["beta_clone"], value_coeff=cfg["value_coeff"], seed=cfg["seed"],
                                     rank=self.rank, episode=episode, log=log)
        finally:
            self.buffer.clear()
        return self.records


def aux_runner(agent, train_cfg_value, shared_grad_buffers=None, rank=0, in_process_chief=True, checkpoint_interval=None,
               first_episode=0):
    """The AuxRunner of a training loop, or None when the key is absent / None.  Refused at start-up: a chief in another
    process (the phase steps the agent's own arena with the in-process optimiser step), several ranks (equal step counts
    per rank would make it work; it is not built), and the interval rules of check_intervals."""
    cfg = aux_config(train_cfg_value)
    if cfg is None:
        return None
    if not in_process_chief:
        raise hip.CadreHipError("train_cfg.aux_phase needs the in-process chief: the phase takes its optimiser steps on this "
                                "process's device")
    world = shared_grad_buffers.dist_world() if shared_grad_buffers is not None else 0
    if world > 1:
        raise hip.CadreHipError("train_cfg.aux_phase needs a single rank (world size %d): the multi-rank phase is not built"
                                % world)
    check_intervals(cfg["interval"], checkpoint_interval, first_episode)
    return AuxRunner(agent, cfg, rank)
