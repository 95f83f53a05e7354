"""Behaviour-cloning warm start from recorded episodes (cadre_amd.replay records).

A recorded PPO rollout is off-policy the moment the weights move, so PPO cannot reuse it — imitation can.  The pieces:

    demo = DemoSet.from_episodes(agent, replay.list_episodes(dir), gamma=0.99, balance="command")
    train, val = demo.split(0.1, seed=0)
    log = pretrain(agent, train, None, epochs=5, minibatch=64, lr=3e-4, max_grad_norm=250.0, validation=val)

`DemoSet` keeps a whole demonstration set on the device in ONE pair of ordinary RolloutStorage objects: every distinct
frame is encoded once by the agent's frozen encoder, cadre_demo_rows lays the window rows out in one launch, the critic
targets are discounted Monte-Carlo returns from the rollout-finishing scan (cadre_gae_multi with V = 0, tau = 1).
`pretrain` runs the update's own launch chain with the loss switched to cadre_bc_loss (CadreAgent.imitate_from_storages)
followed by the clip + Adam step.  A record's `action` is the demonstrated bin per head; -1 means "no label for this head"
(the row then only trains the other head).  Demonstrations recorded as continuous controls go through controls_to_bins.
"""
import os

import numpy as np
import torch

from . import hip, replay

GAE_MAX_T = 3000          # rows per cadre_gae_multi launch (include/cadre_hip.h)
PRETRAIN_KEYS = ("episodes", "epochs", "minibatch", "lr", "label_smoothing", "balance", "validation_fraction",
                 "max_grad_norm", "return_scale", "seed")
DEMO_MIX_KEYS = ("episodes", "coeff", "value_coeff", "blocks", "label_smoothing", "balance", "return_scale", "seed")
# accepted beside the keys above by both dicts; in the parsed dict only when given (absent: the dict is what it always was)
FRAME_KEYS = ("frame_table",)


# ----------------------------------------------------------------------------- host helpers
def controls_to_bins(steer, throttle, brake, STEER_CONTROL, THROTTLE_CONTROL):
    """Nearest bin per head for demonstrations recorded as continuous controls: steer against STEER_CONTROL {bin: value},
    (throttle, brake) against THROTTLE_CONTROL {bin: (throttle, brake)} by squared distance; ties go to the lower index.
    Scalars or arrays of one length -> (steer bins, throttle bins) int64 arrays."""
    st = np.array([float(STEER_CONTROL[i]) for i in range(len(STEER_CONTROL))], dtype=np.float64)
    tt = np.array([[float(v) for v in THROTTLE_CONTROL[i]] for i in range(len(THROTTLE_CONTROL))], dtype=np.float64)
    s = np.atleast_1d(np.asarray(steer, dtype=np.float64))
    tb = np.stack([np.atleast_1d(np.asarray(throttle, dtype=np.float64)), np.atleast_1d(np.asarray(brake, dtype=np.float64))], 1)
    if s.ndim != 1 or tb.shape[0] != s.shape[0]:
        raise ValueError("controls_to_bins: steer, throttle and brake must have one length")
    a_s = np.abs(s[:, None] - st[None, :]).argmin(1)                       # (argmin: the first minimum)
    a_t = ((tb[:, None, :] - tt[None, :, :]) ** 2).sum(-1).argmin(1)
    return a_s.astype(np.int64), a_t.astype(np.int64)


def balance_weights(commands, mode="command"):
    """Row weights of a demonstration set, float32 [T].  "command": w = T / (C_present * count[command of the row]) — the
    weighted command histogram is flat over the commands that occur, and sum(w) = T.  None: ones."""
    cmd = np.asarray(commands, dtype=np.int64).reshape(-1)
    if mode is None:
        return np.ones(cmd.size, dtype=np.float32)
    if mode != "command":
        raise ValueError("balance: expected \"command\" or None (got %r)" % (mode,))
    if cmd.size and cmd.min() < 0:
        raise ValueError("balance: negative command")
    count = np.bincount(cmd) if cmd.size else np.zeros(0, np.int64)
    present = int((count > 0).sum())
    return (cmd.size / (present * count[cmd].astype(np.float64))).astype(np.float32)


def episode_masks(done, ends):
    """1 - done per head, float32 [T][2], with the last row of every episode forced to 0: a record that ends without
    `done` is treated as ended (nothing is known about what followed).  ends: the exclusive end row of each episode."""
    m = 1.0 - np.asarray(done, dtype=np.float32).reshape(-1, 2)
    for e in ends:
        m[e - 1] = 0.0
    return m


def split_episodes(n_episodes, fraction, seed):
    """Episode indices (train, validation) of DemoSet.split: a seeded permutation, round(fraction * n) validation episodes,
    at least one on each side."""
    if n_episodes < 2:
        raise ValueError("split: %d episode(s); a split by episode needs two" % n_episodes)
    if not 0.0 < float(fraction) < 1.0:
        raise ValueError("split: fraction must be in (0, 1) (got %r)" % (fraction,))
    perm = np.random.RandomState(seed).permutation(n_episodes)
    n_val = min(n_episodes - 1, max(1, int(round(float(fraction) * n_episodes))))
    return sorted(perm[n_val:].tolist()), sorted(perm[:n_val].tolist())


def _gae_chunks(T):
    """[lo, hi) chunks of at most GAE_MAX_T rows, none shorter than 2 (the scan's minimum), back to front."""
    if T < 2:
        raise ValueError("a demonstration set needs at least 2 transitions (got %d)" % T)
    cuts = list(range(0, T, GAE_MAX_T)) + [T]
    if cuts[-1] - cuts[-2] < 2:
        cuts[-2] -= 1
    return [(cuts[i], cuts[i + 1]) for i in range(len(cuts) - 2, -1, -1)]


# ----------------------------------------------------------------------------- the demonstration set
class DemoSet(object):
    """A demonstration set on the device: `steer` / `throttle` RolloutStorage objects with num_steps = transitions (row t:
    obs = the window of transition t, action = the demonstrated bin, command, masks, rewards, returns = the discounted
    Monte-Carlo return times return_scale; hn / cn, value_preds and action_log_probs are zeros — act() hands out the zero
    state), `weights` float32 [T][1] (the row weights, which travel through the minibatch gather in the advantage slot),
    `episodes` [(first row, end row)], `commands` (host int array).
    `frame_table` (from_episodes(frame_table=True)): the two storages are FrameStorages (cadre_amd.frames) — every recorded
    frame's row once, `_frames` [n_frames][ldo], and the record's window indices, `_win` [T + 1][S], in place of the S = 8
    times larger window rows; the sets `split` cuts share `_frames`.  Every step reads the same bits either way."""

    def __init__(self, steer, throttle, weights, episodes, commands, gamma, balance, return_scale):
        self.steer, self.throttle, self.weights = steer, throttle, weights
        self.frame_table = getattr(steer, "_win", None) is not None
        self.episodes, self.commands = list(episodes), np.asarray(commands, dtype=np.int64)
        self.gamma, self.balance, self.return_scale = gamma, balance, return_scale
        self.T = steer.num_steps

    def __len__(self):
        return self.T

    @staticmethod
    def _storages(T, feature_dims, seq_length, hidden_size, gamma, device):
        from .ppo_agent.storage import RolloutStorage
        steer, throttle = (RolloutStorage(T, 1, feature_dims, seq_length, hidden_size, True, gamma, 1.0, device=device)
                           for _ in range(2))
        throttle._obs, throttle.obs = steer._obs, steer.obs          # one copy of the window rows serves both heads
        return steer, throttle

    @classmethod
    def from_episodes(cls, agent, paths_or_dicts, gamma, balance="command", return_scale=1.0, frame_table=False):
        """paths_or_dicts: replay record paths (or loaded record dicts), one per episode, in order.  frame_table: keep
        frame rows and window indices (FrameStorage) instead of materialised window rows, which are then never allocated."""
        if not isinstance(frame_table, bool):
            raise ValueError("DemoSet.from_episodes: frame_table must be a bool (got %r)" % (frame_table,))
        eps = [replay.load_episode(p) if isinstance(p, (str, os.PathLike)) else p for p in paths_or_dicts]
        if not eps:
            raise ValueError("DemoSet.from_episodes: no episodes")
        enc, dev, a = agent.vae_model, agent.device, agent.arena
        S = int(eps[0]["window"].shape[1])
        if S != agent.learner.S or any(int(ep["window"].shape[1]) != S for ep in eps):
            raise ValueError("DemoSet.from_episodes: records hold windows of %s frames, the agent's nets take %d"
                             % (sorted({int(ep["window"].shape[1]) for ep in eps}), agent.learner.S))
        lat, win, n_frames, bounds = [], [], 0, []
        t0 = 0
        for ep in eps:
            rgb = torch.from_numpy(np.ascontiguousarray(ep["rgb"])).to(agent.vae_device)
            route = torch.from_numpy(np.ascontiguousarray(ep["route"])).to(agent.vae_device)
            lat.append(enc.latent(rgb, route).to(dev))               # chunks of enc.max_frames; batch-invariant bits
            w = np.asarray(ep["window"], dtype=np.int64)
            if w.min() < 0 or w.max() >= rgb.shape[0]:
                raise ValueError("DemoSet.from_episodes: a window index outside the record's %d frames" % rgb.shape[0])
            win.append(w + n_frames)
            n_frames += int(rgb.shape[0])
            bounds.append((t0, t0 + w.shape[0]))
            t0 += w.shape[0]
        T = t0
        chunks = _gae_chunks(T)
        latent = torch.cat(lat) if len(lat) > 1 else lat[0]
        del lat
        meas = torch.from_numpy(np.ascontiguousarray(np.concatenate([ep["measurements"] for ep in eps]), dtype=np.float64)).to(dev)
        window = torch.from_numpy(np.concatenate(win).astype(np.int32)).to(dev)
        if frame_table:
            # one row per FRAME: cadre_demo_rows over n_frames "windows" of one frame each, the identity for ids; the
            # record's own window indices become the storages' `_win` (row T, which no minibatch reads: -1)
            from .frames import frame_pair
            win = torch.cat([window.view(T, S), torch.full((1, S), -1, dtype=torch.int32, device=dev)])
            steer, throttle = frame_pair(T, agent.lstm_input, S, agent.lstm_input, gamma, dev, win=win, frame_capacity=n_frames)
            steer.n_frames = throttle.n_frames = n_frames
            ident = torch.arange(n_frames, dtype=torch.int32, device=dev)
            hip.check(hip.lib().cadre_demo_rows(hip.ptr(latent), latent.stride(0), n_frames, hip.ptr(ident), hip.ptr(meas),
                                                n_frames, 1, hip.ptr(steer._frames), steer._ldo, hip.stream()), "cadre_demo_rows")
        else:
            steer, throttle = cls._storages(T, agent.lstm_input, S, agent.lstm_input, gamma, dev)
            hip.check(hip.lib().cadre_demo_rows(hip.ptr(latent), latent.stride(0), n_frames, hip.ptr(window), hip.ptr(meas), T, S,
                                                hip.ptr(steer._obs), steer._ldo, hip.stream()), "cadre_demo_rows")
        cmd = np.concatenate([np.asarray(ep["command"], dtype=np.int64).reshape(-1) for ep in eps])
        act = np.concatenate([np.asarray(ep["action"], dtype=np.int64).reshape(-1, 2) for ep in eps])
        rew = np.concatenate([np.asarray(ep["reward"], dtype=np.float32).reshape(-1, 2) for ep in eps])
        done = np.concatenate([np.asarray(ep["done"]).reshape(-1, 2) for ep in eps])
        masks = episode_masks(done, [e for _b, e in bounds])
        cmd_d = torch.from_numpy(cmd.astype(np.int32)).to(dev)
        for h, st in enumerate((steer, throttle)):
            st.command[:T, 0].copy_(cmd_d)
            st.action[:T, 0].copy_(torch.from_numpy(np.ascontiguousarray(act[:, h])).to(dev))
            st.rewards[:T, 0].copy_(torch.from_numpy(np.ascontiguousarray(rew[:, h])).to(dev))
            st.masks[:T, 0].copy_(torch.from_numpy(np.ascontiguousarray(masks[:, h])).to(dev))
        cls._mc_returns(steer, throttle, chunks, gamma, return_scale)
        weights = torch.from_numpy(balance_weights(cmd, balance)).to(dev).view(T, 1)
        return cls(steer, throttle, weights, bounds, cmd, gamma, balance, return_scale)

    @staticmethod
    def _mc_returns(steer, throttle, chunks, gamma, return_scale):
        """returns[t] = r_t + gamma m_t returns[t + 1] per head: the strict fp32 scan of cadre_gae with V = 0 and tau = 1.
        Sets of more than GAE_MAX_T rows are scanned in chunks from the back; a chunk bootstraps from the first return of
        the chunk behind it, which for masks of exactly 0 or 1 gives the bits of one long scan."""
        g32 = float(np.float32(gamma))
        L = hip.lib()
        for lo, hi in chunks:
            rows = [[hip.ptr(s.rewards) + 4 * lo, hip.ptr(s.value_preds) + 4 * lo, hip.ptr(s.masks) + 4 * lo,
                     hip.ptr(s.returns) + 4 * hi, hip.ptr(s.returns) + 4 * lo, hip.ptr(s.advantages) + 4 * lo, 0]
                    for s in (steer, throttle)]                       # (returns[T] of a storage is its zero)
            table = torch.tensor(rows, dtype=torch.int64).to(steer.device)
            hip.check(L.cadre_gae_multi(hip.ptr(table), 2, hi - lo, g32, g32, 0, None, 0.0, hip.stream()), "cadre_gae_multi")
        for s in (steer, throttle):
            s.value_preds.zero_()                                     # (the scan parks each chunk's bootstrap value there)
            s.advantages.zero_()
            if float(return_scale) != 1.0:
                s.returns.mul_(float(return_scale))

    # ------------------------------------------------------------------ subsets
    def _subset(self, episode_ids):
        rows = np.concatenate([np.arange(*self.episodes[e]) for e in episode_ids])
        dev = self.steer.device
        idx = torch.from_numpy(rows).to(dev)
        T = int(rows.size)
        s0 = self.steer
        if self.frame_table:                              # the windows of the rows; the frames are shared, not copied
            from .frames import frame_pair
            win = torch.cat([s0._win.index_select(0, idx), torch.full((1, s0.seq_length), -1, dtype=torch.int32, device=dev)])
            steer, throttle = frame_pair(T, s0.z_dims, s0.seq_length, s0.hid_size, self.gamma, dev, frames=s0._frames, win=win,
                                         n_frames=s0.n_frames)
        else:
            steer, throttle = self._storages(T, s0.z_dims, s0.seq_length, s0.hid_size, self.gamma, dev)
            steer._obs[:T].copy_(s0._obs.index_select(0, idx))
        for src, dst in ((self.steer, steer), (self.throttle, throttle)):
            for k in ("command", "action", "rewards", "masks", "returns"):
                getattr(dst, k)[:T].copy_(getattr(src, k).index_select(0, idx))
        bounds, t0 = [], 0
        for e in episode_ids:
            n = self.episodes[e][1] - self.episodes[e][0]
            bounds.append((t0, t0 + n))
            t0 += n
        cmd = self.commands[rows]
        weights = torch.from_numpy(balance_weights(cmd, self.balance)).to(dev).view(T, 1)
        return DemoSet(steer, throttle, weights, bounds, cmd, self.gamma, self.balance, self.return_scale)

    def split(self, fraction, seed):
        """(training set, validation set), split BY EPISODE: round(fraction * episodes) validation episodes (at least one on
        each side) picked by a seeded permutation.  Returns are per episode, so they carry over; the balance weights are
        formed again per side."""
        train, val = split_episodes(len(self.episodes), fraction, seed)
        return self._subset(train), self._subset(val)

    def batch(self, idx):
        """The `batches` argument of CadreAgent.imitate_from_storages for rows `idx` (a CPU int64 tensor)."""
        return [(self.steer, idx, self.weights, self.throttle, idx, self.weights)]


# ----------------------------------------------------------------------------- the loop
def _optimizer_hyper(agent, target):
    if target is None:
        return (0.9, 0.999), 1e-8
    arena = getattr(target, "arena", None)
    if arena is not None:                       # a Shared_grad_buffers: it must stand for the agent's own nets
        if arena is not agent.arena:
            raise hip.CadreHipError("pretrain: the shared gradient buffers belong to another parameter arena")
        return (0.9, 0.999), 1e-8
    g = target.param_groups[0]
    return tuple(g.get("betas", (0.9, 0.999))), g.get("eps", 1e-8)


def reset_adam(agent):
    """Adam moments and step count of the agent's arena back to zero, and everything cached from the parameters re-derived."""
    a, lrn = agent.arena, agent.learner
    if a.exp_avg is not None:
        a.exp_avg.zero_()
        a.exp_avg_sq.zero_()
    a.step = 0
    a.step_dev.zero_()
    lrn.invalidate_parameter_caches()            # (the step count is part of the key the packed weights are cached under)


def pretrain(agent, demo, optimizer_or_shared, epochs, minibatch, lr, max_grad_norm, label_smoothing=0.0, validation=None,
             reset_optimizer=True, log=None, bc_coeff=1.0):
    """Behaviour cloning on `demo` (a DemoSet) before PPO starts.  Per epoch one permutation of the rows from the global
    torch CPU generator (as RolloutStorage.sample_indices draws), cut into minibatches of `minibatch` rows with the tail
    dropped (one B, one captured graph); each step is CadreAgent.imitate_from_storages followed by the learner's clip +
    Adam step with `lr` / `max_grad_norm` (betas and eps of `optimizer_or_shared` when it is an optimizer; None and a
    Shared_grad_buffers of the agent's own arena give Adam's defaults — the step is rank-local, no collective runs).
    Per epoch one pass over `validation` (a DemoSet) with the evaluation form of the loss.  Returns the per-epoch records:
    dicts with epoch, steps, train_nll / train_accuracy / train_value_error / train_entropy and, with a validation set,
    val_nll / val_accuracy / val_value_error — (steer, throttle) pairs, means over the epoch's steps.  One host sync per
    epoch.  reset_optimizer: the Adam moments and the step count are zero again on return, so PPO starts its own
    optimiser history.  `log`: a callable (or an object with .log) that gets one line per epoch."""
    B = int(minibatch)
    if B < 1 or B > demo.T:
        raise ValueError("pretrain: minibatch %d for a demonstration set of %d rows" % (B, demo.T))
    if int(epochs) < 0:
        raise ValueError("pretrain: epochs=%r" % (epochs,))
    betas, eps = _optimizer_hyper(agent, optimizer_or_shared)
    lrn, dev, F = agent.learner, agent.arena.device, hip.BC_STATS_FIELDS
    emit = None if log is None else (log.log if hasattr(log, "log") else log)
    prev = lrn.loss_begin("bc", label_smoothing=label_smoothing, bc_coeff=bc_coeff)
    records = []
    try:
        for epoch in range(int(epochs)):
            perm = torch.randperm(demo.T)
            steps = demo.T // B
            rows = torch.zeros(steps, 2, F, device=dev)
            for i in range(steps):
                agent.imitate_from_storages(demo.batch(perm[i * B:(i + 1) * B]), stats_row=rows[i], sync=False)
                lrn.clip_adam(lr=lr, max_grad_norm=max_grad_norm, betas=betas, eps=eps)
            parts = [rows.mean(0)]
            if validation is not None:
                parts.append(evaluate(agent, validation, B, _device=True))
            host = torch.stack(parts).cpu().tolist()
            rec = dict(epoch=epoch, steps=steps)
            for name, r in zip(("train", "val"), host):
                rec[name + "_accuracy"], rec[name + "_nll"] = (r[0][0], r[1][0]), (r[0][1], r[1][1])
                rec[name + "_entropy"], rec[name + "_value_error"] = (r[0][2], r[1][2]), (r[0][3], r[1][3])
            records.append(rec)
            if emit is not None:
                line = "Pretrain epoch: {}, nll: {:.4f}/{:.4f}, accuracy: {:.4f}/{:.4f}, value error: {:.4f}/{:.4f}".format(
                    epoch, *(rec["train_nll"] + rec["train_accuracy"] + rec["train_value_error"]))
                if validation is not None:
                    line += ", validation nll: {:.4f}/{:.4f}, accuracy: {:.4f}/{:.4f}".format(*(rec["val_nll"] + rec["val_accuracy"]))
                emit(line)
    finally:
        lrn.loss_restore(prev)
        if reset_optimizer:
            reset_adam(agent)
    return records


def evaluate(agent, demo, minibatch, _device=False):
    """One pass over `demo` with the evaluation form of the imitation loss (no gradient, nothing moves), in order, in
    minibatches of min(minibatch, rows) with the tail dropped: the statistics [2][hip.BC_STATS_FIELDS] averaged over the
    minibatches (a list of lists; the learner's current imitation settings)."""
    B = min(int(minibatch), demo.T)
    steps = demo.T // B
    rows = torch.zeros(steps, 2, hip.BC_STATS_FIELDS, device=agent.arena.device)
    order = torch.arange(demo.T)
    for i in range(steps):
        agent.imitate_from_storages(demo.batch(order[i * B:(i + 1) * B]), stats_row=rows[i], sync=False, evaluate=True)
    out = rows.mean(0)
    return out if _device else out.cpu().tolist()


# ----------------------------------------------------------------------------- train_cfg["pretrain"]
def pretrain_config(train_cfg_value):
    """train_cfg["pretrain"]: absent / None -> None; else a dict {"episodes": DIR or a list of record paths, "epochs",
    "minibatch", "lr", "label_smoothing", "balance", "validation_fraction", "max_grad_norm", "return_scale", "seed",
    "frame_table" (False; True: the set keeps frame rows and window indices, DemoSet.from_episodes(frame_table=True))} -> the dict with
    defaults filled in (max_grad_norm None: train_cfg's)."""
    cfg = train_cfg_value
    if cfg is None:
        return None
    if not isinstance(cfg, dict):
        raise ValueError("train_cfg.pretrain: expected None or a dict (got %r)" % (cfg,))
    unknown = sorted(set(cfg) - set(PRETRAIN_KEYS + FRAME_KEYS))
    if unknown or "episodes" not in cfg:
        raise ValueError("train_cfg.pretrain: needs episodes; known keys %r (unknown: %r)" % (PRETRAIN_KEYS, unknown))
    out = dict(episodes=cfg["episodes"], epochs=int(cfg.get("epochs", 1)), minibatch=int(cfg.get("minibatch", 64)),
               lr=float(cfg.get("lr", 3e-4)), label_smoothing=float(cfg.get("label_smoothing", 0.0)),
               balance=cfg.get("balance", "command"), validation_fraction=cfg.get("validation_fraction"),
               max_grad_norm=cfg.get("max_grad_norm"), return_scale=float(cfg.get("return_scale", 1.0)),
               seed=int(cfg.get("seed", 0)))
    if "frame_table" in cfg:
        out["frame_table"] = _frame_table_value("pretrain", cfg["frame_table"])
    if out["epochs"] < 0 or out["minibatch"] < 1 or not out["lr"] > 0.0 or not 0.0 <= out["label_smoothing"] < 1.0:
        raise ValueError("train_cfg.pretrain: need epochs >= 0, minibatch >= 1, lr > 0, 0 <= label_smoothing < 1 (got %r)" % (cfg,))
    if out["balance"] not in (None, "command"):
        raise ValueError("train_cfg.pretrain: balance must be \"command\" or None (got %r)" % (out["balance"],))
    vf = out["validation_fraction"]
    if vf is not None and not 0.0 <= float(vf) < 1.0:
        raise ValueError("train_cfg.pretrain: validation_fraction must be in [0, 1) (got %r)" % (vf,))
    out["validation_fraction"] = None if not vf else float(vf)
    return out


def pretrain_from_config(agent, cfg, gamma, max_grad_norm, shared_grad_buffers=None, rank=0, logger=None):
    """The `pretrain` key of train() / train_vec(), once before the first rollout: record directory -> DemoSet -> (split)
    -> pretrain.  With several ranks it runs on rank 0 only and the parameters are then broadcast from rank 0 (multi-rank
    pretraining is not built).  Returns the per-epoch records (None on the other ranks)."""
    cfg = pretrain_config(cfg)
    if cfg is None:
        return None
    world = shared_grad_buffers.dist_world() if shared_grad_buffers is not None else 0
    records = None
    if rank == 0:
        # (a set train_cfg["demo_mix"] built from the same records and parameters is shared: frames are encoded once)
        demo = demo_set_for(agent, cfg["episodes"], gamma, cfg["balance"], cfg["return_scale"],
                            frame_table=cfg.get("frame_table", False))
        val = None
        if cfg["validation_fraction"] is not None and len(demo.episodes) >= 2:
            demo, val = demo.split(cfg["validation_fraction"], cfg["seed"])
        records = pretrain(agent, demo, None, cfg["epochs"], min(cfg["minibatch"], demo.T), cfg["lr"],
                           max_grad_norm if cfg["max_grad_norm"] is None else float(cfg["max_grad_norm"]),
                           label_smoothing=cfg["label_smoothing"], validation=val, log=logger if rank == 0 else None)
    if world > 1:
        import torch.distributed as dist
        dist.broadcast(agent.arena.params, src=0)
        agent.learner.invalidate_parameter_caches()
    return records


# ----------------------------------------------------------------------------- train_cfg["demo_mix"]: DAPG-style mixing
def _episode_paths(src):
    return replay.list_episodes(src) if isinstance(src, (str, os.PathLike)) else list(src)


def _demo_key(src, gamma, balance, return_scale, frame_table=False):
    paths = _episode_paths(src)
    if not all(isinstance(p, (str, os.PathLike)) for p in paths):
        return None                                      # loaded record dicts: nothing to key a shared set on
    return (tuple(os.fspath(p) for p in paths), float(gamma), balance, float(return_scale), bool(frame_table))


def demo_set_for(agent, src, gamma, balance, return_scale, keep=False, frame_table=False):
    """The DemoSet of record directory / path list `src` with these parameters.  keep: the set stays with the agent, so a
    later call that names the same records and parameters (train_cfg.pretrain beside train_cfg.demo_mix) gets the same
    object instead of encoding every frame again."""
    key = _demo_key(src, gamma, balance, return_scale, frame_table)
    kept = agent.__dict__.setdefault("_demo_sets", {})
    if key is not None and key in kept:
        return kept[key]
    demo = DemoSet.from_episodes(agent, _episode_paths(src), gamma, balance=balance, return_scale=return_scale,
                                 frame_table=frame_table)
    if keep and key is not None:
        kept[key] = demo
    return demo


class DemoMixer(object):
    """The demonstration rows of each mixed PPO step (CadreAgent.update_policy_from_storages(..., demo=)).
    entries(Bw, episode, step) -> `blocks` entries of Bw demonstration rows each, of the form DemoSet.batch returns.
    The draw is STATELESS: the row indices are a pure function of (seed, rank, episode, step, Bw, blocks, len(demo_set)),
    drawn from a private torch.Generator seeded from exactly those values — never from the global CPU generator, whose
    stream belongs to the PPO sampler and act().  A resumed run therefore draws the rows the uninterrupted run would have
    drawn, with nothing added to a checkpoint (the DemoSet is rebuilt from the record directory).  Sampling is a prefix of
    a permutation of the set, or with replacement when blocks * Bw exceeds its size.
    coeff / value_coeff / label_smoothing ride along for the training loop (demo_mix_config)."""

    def __init__(self, demo_set, blocks=1, seed=0, rank=0, coeff=1.0, value_coeff=0.0, label_smoothing=0.0):
        if isinstance(blocks, bool) or int(blocks) != blocks or int(blocks) < 1:
            raise ValueError("DemoMixer: blocks=%r" % (blocks,))
        if len(demo_set) < 1:
            raise ValueError("DemoMixer: an empty demonstration set")
        self.demo, self.blocks, self.seed, self.rank = demo_set, int(blocks), int(seed), int(rank)
        self.coeff, self.value_coeff, self.label_smoothing = coeff, float(value_coeff), float(label_smoothing)

    def indices(self, Bw, episode, step):
        """int64 [blocks * Bw] row indices of the draw with this key."""
        Bw, T = int(Bw), len(self.demo)
        if Bw < 1 or int(episode) < 0 or int(step) < 0:
            raise ValueError("DemoMixer: Bw=%r, episode=%r, step=%r" % (Bw, episode, step))
        key = [self.seed & 0xFFFFFFFFFFFFFFFF, self.rank, int(episode), int(step), Bw, self.blocks, T]
        lo, hi = np.random.SeedSequence(key).generate_state(2, dtype=np.uint32)
        g = torch.Generator()
        g.manual_seed(((int(hi) << 32) | int(lo)) & 0x7FFFFFFFFFFFFFFF)
        n = self.blocks * Bw
        if n > T:
            return torch.randint(0, T, (n,), generator=g, dtype=torch.int64)
        return torch.randperm(T, generator=g)[:n]

    def entries(self, Bw, episode, step):
        idx = self.indices(Bw, episode, step)
        Bw = int(Bw)
        return [self.demo.batch(idx[i * Bw:(i + 1) * Bw])[0] for i in range(self.blocks)]


def demo_mix_config(train_cfg_value):
    """train_cfg["demo_mix"]: absent / None -> None; else a dict {"episodes": DIR or a list of record paths (required),
    "coeff": a number, ("linear", start, end) or a callable of episode / max_episode (ppo_agent.train.schedule_value; 1.0),
    "value_coeff" (0.0), "blocks" (1), "label_smoothing" (0.0), "balance" ("command"), "return_scale" (1.0), "seed" (0),
    "frame_table" (False; as in train_cfg["pretrain"])} -> the dict with defaults filled in.  value_coeff defaults to 0
    because the Monte-Carlo returns of a demonstrator and the
    GAE returns of the rollouts (under reward scaling) live on different scales: whoever sets it also sets return_scale."""
    cfg = train_cfg_value
    if cfg is None:
        return None
    if not isinstance(cfg, dict):
        raise ValueError("train_cfg.demo_mix: expected None or a dict (got %r)" % (cfg,))
    unknown = sorted(set(cfg) - set(DEMO_MIX_KEYS + FRAME_KEYS))
    if unknown or "episodes" not in cfg:
        raise ValueError("train_cfg.demo_mix: needs episodes; known keys %r (unknown: %r)" % (DEMO_MIX_KEYS, unknown))
    coeff = cfg.get("coeff", 1.0)
    if not callable(coeff):
        ok = (isinstance(coeff, (tuple, list)) and len(coeff) == 3 and coeff[0] == "linear"
              and all(_is_number(v) for v in coeff[1:])) or _is_number(coeff)
        if not ok:
            raise ValueError("train_cfg.demo_mix: coeff must be a number, (\"linear\", start, end) or a callable (got %r)" % (coeff,))
        coeff = tuple(coeff) if isinstance(coeff, (tuple, list)) else float(coeff)
    blocks = cfg.get("blocks", 1)
    for name in ("value_coeff", "label_smoothing", "return_scale"):
        if name in cfg and not _is_number(cfg[name]):
            raise ValueError("train_cfg.demo_mix: %s=%r is not a finite number" % (name, cfg[name]))
    if isinstance(blocks, bool) or not isinstance(blocks, (int, np.integer)) or blocks < 1:
        raise ValueError("train_cfg.demo_mix: blocks must be an integer >= 1 (got %r)" % (blocks,))
    seed = cfg.get("seed", 0)
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)):
        raise ValueError("train_cfg.demo_mix: seed must be an integer (got %r)" % (seed,))
    out = dict(episodes=cfg["episodes"], coeff=coeff, value_coeff=float(cfg.get("value_coeff", 0.0)), blocks=int(blocks),
               label_smoothing=float(cfg.get("label_smoothing", 0.0)), balance=cfg.get("balance", "command"),
               return_scale=float(cfg.get("return_scale", 1.0)), seed=int(seed))
    if "frame_table" in cfg:
        out["frame_table"] = _frame_table_value("demo_mix", cfg["frame_table"])
    if not 0.0 <= out["label_smoothing"] < 1.0:
        raise ValueError("train_cfg.demo_mix: need 0 <= label_smoothing < 1 (got %r)" % (cfg["label_smoothing"],))
    if out["balance"] not in (None, "command"):
        raise ValueError("train_cfg.demo_mix: balance must be \"command\" or None (got %r)" % (out["balance"],))
    return out


def _frame_table_value(where, v):
    if not isinstance(v, bool):
        raise ValueError("train_cfg.%s: frame_table must be a bool (got %r): True keeps the demonstration set as frame rows "
                         "and window indices" % (where, v))
    return v


def _is_number(v):
    return (not isinstance(v, bool)) and isinstance(v, (int, float, np.integer, np.floating)) and bool(np.isfinite(v))


def demo_mixer_from_config(agent, cfg, gamma, rank=0):
    """train_cfg["demo_mix"] (already through demo_mix_config) -> a DemoMixer over the DemoSet of its records.  The set is
    kept with the agent (demo_set_for(keep=True)) so that train_cfg.pretrain on the same records shares it."""
    demo = demo_set_for(agent, cfg["episodes"], gamma, cfg["balance"], cfg["return_scale"], keep=True,
                        frame_table=cfg.get("frame_table", False))
    return DemoMixer(demo, blocks=cfg["blocks"], seed=cfg["seed"], rank=rank, coeff=cfg["coeff"],
                     value_coeff=cfg["value_coeff"], label_smoothing=cfg["label_smoothing"])
