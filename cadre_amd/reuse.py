"""Sample reuse: the last M rollouts ride in the PPO step under V-trace.

GePPO (Queeney et al. 2021) with the V-trace targets of Espeholt et al. (2018): every minibatch step of a learner section
carries, behind the live workers' entries, one entry per stale storage of the last `rollouts` sections.  The GePPO
surrogate with rho = pi / mu and clip centre pi_k / mu equals (pi_k / mu) min(r A, clip(r, 1 - eps, 1 + eps) A) with
r = pi / pi_k, so the loss kernels run unchanged once a stale row's old_logp is its log-probability under the policy at the
start of the update and its advantage carries the truncated weight min(rho_bar, pi_k / mu).  The pieces:

    win = ReuseWindow(agent, rollouts=M, num_envs=N, num_steps=T)
    learner_section_multi(agent, rollouts, dones, ..., reuse=win, episode=e)    # refresh() + entries() inside
    win.append(rollouts, dones)                                                   # after the section

refresh() re-evaluates every stale row under the current nets (gather -> the update's forward -> cadre_reuse_record) and
turns that into value targets, advantages and importance weights for all stale storages in ONE cadre_vtrace_multi launch.
train_cfg["sample_reuse"] (reuse_config) wires it into train() / train_vec().
"""
import numpy as np
import torch

from . import hip
from .phasic import _is_int, _is_number, record_starts

REUSE_KEYS = ("rollouts", "rho_bar", "c_bar", "seed")
DIAG_FIELDS = ("ratio_mean", "truncated", "max_abs_log_ratio", "effective_sample_share")


def reuse_permutation(seed, rank, episode, epoch, slot, storage, T):
    """The row order of one stale storage in one epoch: a permutation of its T rows that is a pure function of its key, drawn
    from a private torch.Generator seeded through np.random.SeedSequence (as phasic.epoch_permutation) — never from the global
    CPU generator, whose stream belongs to the PPO sampler and act()."""
    key = [int(seed) & 0xFFFFFFFFFFFFFFFF, int(rank), int(episode), int(epoch), int(slot), int(storage), int(T)]
    if min(key[1:]) < 0 or int(T) < 1:
        raise ValueError("reuse_permutation: rank=%r, episode=%r, epoch=%r, slot=%r, storage=%r, T=%r"
                         % (rank, episode, epoch, slot, storage, T))
    lo, hi = np.random.SeedSequence(key).generate_state(2, dtype=np.uint32)
    g = torch.Generator()
    g.manual_seed(((int(hi) << 32) | int(lo)) & 0x7FFFFFFFFFFFFFFF)
    return torch.randperm(int(T), generator=g)


class ReuseWindow(object):
    """The storages of the last `rollouts` learner sections on the device.  A slot is a verbatim copy of all T + 1 rows of
    each of the 2 N storages of a section (the bootstrap row obs[-1] / command[-1] and whatever the modulo-(T + 1) cursor
    left in it included), so slot m, environment i occupies rows (m N + i)(T + 1) .. of ONE pair of RolloutStorage objects
    (`steer`, `throttle`) that share one `_obs`, as the AuxBuffer's.  Per row: the window, hn / cn, command, action, raw
    reward, mask, time-limit flag; `mu` float32 [2][R + 1] holds the behaviour policy's log-probabilities (the rollouts'
    action_log_probs) and `boot_keep` one float per slot and environment (0 when the rollout ended in `done`).  The big
    storages' action_log_probs / value_preds are the tables cadre_reuse_record writes (logp_now, value_now) and their
    returns / advantages what cadre_vtrace_multi writes — exactly the tensors the step's gather reads as old_logp, old_values,
    returns and advantages.  Memory: about 17 KB per row, as the AuxBuffer."""

    def __init__(self, agent, rollouts, num_envs, num_steps, rho_bar=1.0, c_bar=1.0, seed=0, rank=0, record_minibatch=128,
                 _device=None):
        for name, v, lo in (("rollouts", rollouts, 1), ("num_envs", num_envs, 1), ("num_steps", num_steps, 2),
                            ("record_minibatch", record_minibatch, 1)):
            if not _is_int(v) or v < lo:
                raise ValueError("ReuseWindow: %s must be an integer >= %d (got %r)" % (name, lo, v))
        for name, v in (("rho_bar", rho_bar), ("c_bar", c_bar)):
            if not _is_number(v) or not v > 0:
                raise ValueError("ReuseWindow: %s must be a finite number > 0 (got %r)" % (name, v))
        if not _is_int(seed) or not _is_int(rank) or rank < 0:
            raise ValueError("ReuseWindow: seed=%r, rank=%r" % (seed, rank))
        self.agent = agent
        self.M, self.N, self.T = int(rollouts), int(num_envs), int(num_steps)
        self.rho_bar, self.c_bar, self.seed, self.rank = float(rho_bar), float(c_bar), int(seed), int(rank)
        self.record_minibatch = int(record_minibatch)
        self.P = self.T + 1                      # rows of one storage
        self.R = self.M * self.N * self.P
        self.filled = 0                          # slots that hold a rollout
        self.next = 0                            # the slot the next append() writes
        self.gamma = self.tau = None             # the rollouts' own, taken at the first append
        dev = agent.arena.device if _device is None else _device
        self.device = torch.device(dev)
        from .imitation import DemoSet
        self.steer, self.throttle = DemoSet._storages(self.R, agent.lstm_input, agent.learner.S, agent.lstm_input, 0.0, dev)
        z = lambda *s: torch.zeros(*s, device=dev)
        # the tables of the record pass, [2][R + 1] head-major, seen by the two storages as their own columns
        self.logp_now, self.value_now = z(2, self.R + 1, 1), z(2, self.R + 1, 1)
        for h, s in enumerate((self.steer, self.throttle)):
            s.action_log_probs, s.value_preds = self.logp_now[h], self.value_now[h]
        self.mu = z(2, self.R + 1, 1)
        self.ratio = z(2, self.R + 1, 1)
        self.boot_keep = z(self.M * self.N)
        self.diag = z(self.M * 2 * self.N, hip.VTRACE_DIAG_FIELDS)
        self._table = None
        self._perms = (None, None)

    def base(self, slot, env):
        """First row of the storages of slot `slot`, environment `env`."""
        return (slot * self.N + env) * self.P

    def append(self, rollouts, dones):
        """rollouts = [(steer_storage, throttle_storage), ...] of one learner section, after it ran; dones[i] = environment
        i's last `done`.  Device-to-device copies into the next slot; once all slots are filled the oldest is overwritten.
        Not a hot path, no host sync."""
        if len(rollouts) != self.N or len(dones) != self.N:
            raise ValueError("ReuseWindow.append: %d storage pairs and %d dones for %d environments"
                             % (len(rollouts), len(dones), self.N))
        big = (self.steer, self.throttle)
        for s, t in rollouts:
            if (s.num_steps != self.T or t.num_steps != self.T
                    or (s._ldo, s.seq_length, s._ldh) != (self.steer._ldo, self.steer.seq_length, self.steer._ldh)):
                raise ValueError("ReuseWindow.append: a storage pair whose geometry differs from the window's")
            if (self.gamma, self.tau) not in ((None, None), (s.gamma, s.tau)) or (s.gamma, s.tau) != (t.gamma, t.tau):
                raise ValueError("ReuseWindow.append: storages of different gamma / tau")
            self.gamma, self.tau = s.gamma, s.tau
        slot, P = self.next, self.P
        for i, pair in enumerate(rollouts):
            lo = self.base(slot, i)
            self.steer._obs[lo:lo + P].copy_(pair[0]._obs)
            for h, (src, dst) in enumerate(zip(pair, big)):
                for name in ("_hn", "_cn", "command", "action", "rewards", "masks", "time_limits"):
                    getattr(dst, name)[lo:lo + P].copy_(getattr(src, name))
                self.mu[h, lo:lo + P].copy_(src.action_log_probs)
        keep = torch.tensor([0.0 if d else 1.0 for d in dones], dtype=torch.float32)
        self.boot_keep[slot * self.N:(slot + 1) * self.N].copy_(keep, non_blocking=True)
        self.next = (slot + 1) % self.M
        self.filled = min(self.M, self.filled + 1)
        self._perms = (None, None)

    # ------------------------------------------------------------------ refresh: record pass + V-trace scan
    def rows_filled(self):
        return self.filled * self.N * self.P

    def record_batches(self):
        """The index vectors of the record pass: the filled rows in order, record_minibatch at a time (phasic.record_starts)."""
        Rf = self.rows_filled()
        B = min(self.record_minibatch, Rf)
        order = torch.arange(Rf)
        return [order[lo:lo + B] for lo in record_starts(Rf, B)]

    def entry(self, idx):
        """The one-entry gather argument for rows `idx` (a CPU int64 tensor) of the big storages."""
        return [(self.steer, idx, self.steer.advantages, self.throttle, idx, self.throttle.advantages)]

    def _vtrace_table(self):
        if self._table is None:
            rows = []
            for slot in range(self.M):
                for i in range(self.N):
                    lo = self.base(slot, i)
                    for h, s in enumerate((self.steer, self.throttle)):
                        p = lambda t: hip.ptr(t) + 4 * lo
                        rows.append([p(s.rewards), p(s.masks), p(s.time_limits), p(self.value_now[h]),
                                     hip.ptr(self.boot_keep) + 4 * (slot * self.N + i), p(self.mu[h]), p(self.logp_now[h]),
                                     p(s.returns), p(s.advantages), p(self.ratio[h]),
                                     hip.ptr(self.diag) + 4 * hip.VTRACE_DIAG_FIELDS * ((slot * self.N + i) * 2 + h)])
            self._table = torch.tensor(rows, dtype=torch.int64).to(self.device)
        return self._table

    def refresh(self, normalise, reward_scaler=None):
        """Before a section's first step: (a) the record pass over all rows of the filled slots (bootstrap rows included) —
        CadreAgent.reuse_record_from_storages in minibatches in row order; (b) ONE cadre_vtrace_multi launch over every
        stale storage: ratio, V-trace returns, and advantages normalised per storage, then times min(rho_bar, ratio).
        With a ReturnScaler the scan reads the scaler's CURRENT scales; cadre_return_stats is not rerun for stale rewards.
        Nothing is read back.  A no-op while the window is empty."""
        if not self.filled:
            return
        if reward_scaler is not None and 2 * reward_scaler.n_envs != 2 * self.N:
            raise ValueError("ReuseWindow.refresh: a ReturnScaler for %d environments, a window for %d"
                             % (reward_scaler.n_envs, self.N))
        for idx in self.record_batches():
            self.agent.reuse_record_from_storages(self.entry(idx), self.logp_now, self.value_now)
        g32 = float(np.float32(self.gamma))
        gt32 = float(np.float32(self.gamma * self.tau))          # double product, then one rounding (storage.py:75)
        state = None if reward_scaler is None else reward_scaler.state
        hip.check(hip.lib().cadre_vtrace_multi(hip.ptr(self._vtrace_table()), self.filled * 2 * self.N, self.T, g32, gt32,
                                               1 if normalise else 0, hip.ptr(state),
                                               float(reward_scaler.clip) if reward_scaler is not None else 0.0,
                                               self.rho_bar, self.c_bar, hip.stream()), "cadre_vtrace_multi")

    # ------------------------------------------------------------------ the step's entries
    def entries(self, episode, epoch, step, Bw):
        """The gather entries of the stale storages for minibatch step `step` of epoch `epoch`: one per filled slot and
        environment, `Bw` rows each, in slot order.  Each stale storage has its own permutation of its T rows per epoch
        (reuse_permutation, keyed by (seed, rank, episode, epoch, slot, storage)), cut as RolloutStorage.sample_indices cuts."""
        if not self.filled:
            return []
        key = (int(episode), int(epoch))
        if self._perms[0] != key:
            self._perms = (key, {(m, k): reuse_permutation(self.seed, self.rank, episode, epoch, m, k, self.T)
                                 for m in range(self.filled) for k in range(2 * self.N)})
        perms, out = self._perms[1], []
        Bw, lo = int(Bw), int(step) * int(Bw)
        if Bw < 1 or lo < 0 or lo + Bw > self.T:
            raise ValueError("ReuseWindow.entries: step %r of %r rows in storages of %d rows" % (step, Bw, self.T))
        for m in range(self.filled):
            for i in range(self.N):
                b = self.base(m, i)
                out.append((self.steer, perms[(m, 2 * i)][lo:lo + Bw] + b, self.steer.advantages,
                            self.throttle, perms[(m, 2 * i + 1)][lo:lo + Bw] + b, self.throttle.advantages))
        return out

    def stats(self):
        """The diag rows of the last refresh: device float32 [filled * 2 N][VTRACE_DIAG_FIELDS], storage k of head k & 1."""
        return self.diag[:self.filled * 2 * self.N]

    def summary(self):
        """The "reuse" entry of a section's `stats`: `filled` and, per DIAG_FIELDS name, the (steer, throttle) pair of means
        over the stale storages.  One small device-to-host copy."""
        out = dict(filled=self.filled)
        if self.filled:
            d = self.stats().double().view(-1, 2, hip.VTRACE_DIAG_FIELDS).mean(0).cpu().tolist()
            for k, name in enumerate(DIAG_FIELDS):
                out[name] = (d[0][k], d[1][k])
        return out


def reuse_stats_text(stats):
    """What stats_line appends for a section that ran with a window."""
    r = stats["reuse"]
    if not r["filled"]:
        return ", reuse: 0 rollouts"
    return (", reuse: {} rollouts, ratio: {:.4f}/{:.4f}, truncated: {:.4f}/{:.4f}, max |log ratio|: {:.4f}/{:.4f}, "
            "effective samples: {:.4f}/{:.4f}").format(r["filled"], *(r["ratio_mean"] + r["truncated"] + r["max_abs_log_ratio"]
                                                                      + r["effective_sample_share"]))


# ----------------------------------------------------------------------------- train_cfg["sample_reuse"]
def reuse_config(train_cfg_value):
    """train_cfg["sample_reuse"]: absent / None -> None (nothing runs, nothing is allocated, nothing is drawn); else a dict
    {"rollouts": M (required, an integer >= 1), "rho_bar" (1.0), "c_bar" (1.0), "seed" (0)} -> the dict with defaults."""
    cfg = train_cfg_value
    if cfg is None:
        return None
    if not isinstance(cfg, dict):
        raise ValueError("train_cfg.sample_reuse: expected None or a dict (got %r)" % (cfg,))
    unknown = sorted(set(cfg) - set(REUSE_KEYS))
    if unknown or "rollouts" not in cfg:
        raise ValueError("train_cfg.sample_reuse: needs rollouts; known keys %r (unknown: %r)" % (REUSE_KEYS, unknown))
    M, seed = cfg["rollouts"], cfg.get("seed", 0)
    if not _is_int(M) or M < 1:
        raise ValueError("train_cfg.sample_reuse: rollouts must be an integer >= 1 (got %r)" % (M,))
    if not _is_int(seed):
        raise ValueError("train_cfg.sample_reuse: seed must be an integer (got %r)" % (seed,))
    for name in ("rho_bar", "c_bar"):
        if name in cfg and (not _is_number(cfg[name]) or not cfg[name] > 0):
            raise ValueError("train_cfg.sample_reuse: %s=%r is not a finite number > 0" % (name, cfg[name]))
    return dict(rollouts=int(M), rho_bar=float(cfg.get("rho_bar", 1.0)), c_bar=float(cfg.get("c_bar", 1.0)), seed=int(seed))


class ReuseRunner(object):
    """train_cfg["sample_reuse"] inside train() / train_vec(): window_for(rollouts) is the `reuse` argument of the learner
    section (the window is allocated at the first call, from the rollouts' geometry), after_section appends to it."""

    def __init__(self, agent, cfg, rank=0):
        self.agent, self.cfg, self.rank = agent, cfg, int(rank)
        self.window = None

    def window_for(self, rollouts):
        if self.window is None:
            c = self.cfg
            self.window = ReuseWindow(self.agent, c["rollouts"], len(rollouts), int(rollouts[0][0].num_steps), rho_bar=c["rho_bar"],
                                      c_bar=c["c_bar"], seed=c["seed"], rank=self.rank)
        return self.window

    def after_section(self, rollouts, dones):
        self.window_for(rollouts).append(rollouts, dones)


def reuse_runner(agent, train_cfg_value, shared_grad_buffers=None, rank=0, in_process_chief=True, fused_gather=True,
                 checkpoint_interval=None, resume_from=None):
    """The ReuseRunner of a training loop, or None when the key is absent / None.  Refused at start-up: a chief in another
    process (the window lives on this process's device and feeds its own steps), several ranks (not built: nothing here can
    test it), fused_gather=False (stale rows enter through the storage gather), and checkpoint_interval / resume_from (the
    window is not part of a checkpoint)."""
    cfg = reuse_config(train_cfg_value)
    if cfg is None:
        return None
    if not in_process_chief:
        raise hip.CadreHipError("train_cfg.sample_reuse needs the in-process chief: the window feeds this process's own steps")
    world = shared_grad_buffers.dist_world() if shared_grad_buffers is not None else 0
    if world > 1:
        raise hip.CadreHipError("train_cfg.sample_reuse needs a single rank (world size %d): the multi-rank form is not built"
                                % world)
    if not fused_gather:
        raise ValueError("train_cfg.sample_reuse needs fused_gather=True: stale rows enter through the storage gather of "
                         "update_policy_from_storages, not through the tuple path")
    if checkpoint_interval is not None or resume_from is not None:
        raise ValueError("train_cfg.sample_reuse excludes checkpoint_interval / resume_from: the window is not part of a "
                         "checkpoint, and a resumed run would not continue with the bits of the uninterrupted one")
    return ReuseRunner(agent, cfg, rank)
