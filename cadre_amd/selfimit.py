"""Self-imitation learning: prioritised rows of the agent's own past rollouts in the PPO step.

Oh et al. 2018 ("Self-Imitation Learning"): keep the agent's past transitions and replay those whose realised return R beat
the critic, with weight w = max(R - v, 0): sil_coeff * mean(-log pi(a|s) w) + sil_value_coeff * mean(0.5 w^2).  The pieces:

    buf = SelfImitationBuffer(agent, rollouts=M, num_envs=N, num_steps=T)
    learner_section_multi(agent, rollouts, dones, ..., sil=buf, episode=e)     # entries() / after_step() inside
    buf.append(rollouts, dones, reward_scaler)                                 # after the section

append() copies the section's storages into the next slot of a ring and runs cadre_sil_prepare: realised returns, closed /
eligible flags and the first priorities.  entries() draws rows by priority ON THE DEVICE (cadre_sil_draw: the priorities
change after every optimiser step, a host-side draw would cost a device-to-host sync per minibatch step) and hands them to
CadreAgent.update_policy_from_storages(sil=); after_step() writes the priorities of the drawn rows back from the w the step
computed (cadre_sil_scatter).  train_cfg["self_imitation"] (sil_config) wires it into train() / train_vec().
"""
import numpy as np
import torch

from . import hip
from .phasic import _is_int, _is_number

SIL_KEYS = ("rollouts", "coeff", "value_coeff", "alpha", "prio_eps", "tail", "blocks", "seed")
TAILS = ("drop", "bootstrap")
STATS_FIELDS = ("w_mean", "positive_share", "nll", "value_error", "w_max", "rows")
U_BITS = 62                       # the random words of the draw: uniform in [0, 2^62)


def sil_words(seed, rank, episode, epoch, step, Bw, blocks):
    """int64 [2][blocks * Bw] non-negative random words of one step's draw: a pure function of the key, from a private
    torch.Generator seeded through np.random.SeedSequence (as DemoMixer.indices) — never from the global CPU generator, whose
    stream belongs to the PPO sampler and act()."""
    key = [int(seed) & 0xFFFFFFFFFFFFFFFF, int(rank), int(episode), int(epoch), int(step), int(Bw), int(blocks)]
    if min(key[1:]) < 0 or int(Bw) < 1 or int(blocks) < 1:
        raise ValueError("sil_words: rank=%r, episode=%r, epoch=%r, step=%r, Bw=%r, blocks=%r"
                         % (rank, episode, epoch, step, Bw, blocks))
    lo, hi = np.random.SeedSequence(key).generate_state(2, dtype=np.uint32)
    g = torch.Generator()
    g.manual_seed(((int(hi) << 32) | int(lo)) & 0x7FFFFFFFFFFFFFFF)
    return torch.randint(0, 1 << U_BITS, (2, int(blocks) * int(Bw)), generator=g, dtype=torch.int64)


class SelfImitationBuffer(object):
    """The storages of the last `rollouts` learner sections on the device, with a priority per head and row.  A slot ring as
    the ReuseWindow's: slot m, environment i occupies rows (m N + i)(T + 1) .. of ONE pair of RolloutStorage objects (`steer`,
    `throttle`) that share one `_obs`.  Per row: the window, hn / cn, command, action, raw reward, mask, time-limit flag and
    value_preds as collected; `returns` holds the realised return R (cadre_sil_prepare), `flags` int32 [2][R] closed |
    eligible << 1, `q` int32 [2][R] the priority (the kernels' uint32; at most 2^31 - 1, 0: never drawn — ineligible rows and
    the bootstrap row T of every storage).  action_log_probs and advantages stay zero: a SIL row reads neither.
    tail "drop": only rows whose episode ended inside the rollout by a true termination are eligible; "bootstrap": every row,
    the cut tails with the return bootstrapped from the stored value at the cut.  Memory: about 17 KB per row."""

    def __init__(self, agent, rollouts, num_envs, num_steps, alpha=0.6, prio_eps=1e-3, tail="drop", blocks=1, seed=0, rank=0,
                 _device=None):
        for name, v, lo in (("rollouts", rollouts, 1), ("num_envs", num_envs, 1), ("num_steps", num_steps, 2), ("blocks", blocks, 1)):
            if not _is_int(v) or v < lo:
                raise ValueError("SelfImitationBuffer: %s must be an integer >= %d (got %r)" % (name, lo, v))
        if not _is_number(alpha) or not alpha > 0:
            raise ValueError("SelfImitationBuffer: alpha must be a finite number > 0 (got %r)" % (alpha,))
        if not _is_number(prio_eps) or prio_eps < 0:
            raise ValueError("SelfImitationBuffer: prio_eps must be a finite number >= 0 (got %r)" % (prio_eps,))
        if tail not in TAILS:
            raise ValueError("SelfImitationBuffer: tail must be one of %r (got %r)" % (TAILS, tail))
        if not _is_int(seed) or not _is_int(rank) or rank < 0:
            raise ValueError("SelfImitationBuffer: seed=%r, rank=%r" % (seed, rank))
        self.agent = agent
        self.M, self.N, self.T = int(rollouts), int(num_envs), int(num_steps)
        self.alpha, self.prio_eps, self.tail = float(alpha), float(prio_eps), tail
        self.blocks, self.seed, self.rank = int(blocks), int(seed), int(rank)
        self.P = self.T + 1
        self.R = self.M * self.N * self.P
        self.filled = 0                          # slots that hold a rollout
        self.next = 0                            # the slot the next append() writes
        self.gamma = None                        # the rollouts' own, taken at the first append
        self.ready = False                       # both heads have an eligible row (decided at append: one small copy)
        dev = agent.arena.device if _device is None else _device
        self.device = torch.device(dev)
        from .imitation import DemoSet
        self.steer, self.throttle = DemoSet._storages(self.R, agent.lstm_input, agent.learner.S, agent.lstm_input, 0.0, dev)
        self.flags = torch.zeros(2, self.R, dtype=torch.int32, device=dev)
        self.q = torch.zeros(2, self.R, dtype=torch.int32, device=dev)
        self._scratch = torch.zeros(4 * ((self.R + 1023) // 1024) + 2, dtype=torch.int64, device=dev)
        self._tables = {}
        self._ring = None                        # staging of the random words and the drawn indices, a few steps deep
        self._last = None                        # (idx [2][n], n) of the step that ran last
        self._stats = None                       # device float32 [steps][2][SIL_STATS_FIELDS] of the section
        self._n_stats = 0

    def base(self, slot, env):
        """First row of the storages of slot `slot`, environment `env`."""
        return (slot * self.N + env) * self.P

    def rows_filled(self):
        return self.filled * self.N * self.P

    def _table(self, slot):
        if slot not in self._tables:
            rows = []
            for i in range(self.N):
                lo = self.base(slot, i)
                for h, s in enumerate((self.steer, self.throttle)):
                    p = lambda t: hip.ptr(t) + 4 * lo
                    rows.append([p(s.rewards), p(s.masks), p(s.time_limits), p(s.value_preds), p(s.returns),
                                 p(self.flags[h]), p(self.q[h])])
            self._tables[slot] = torch.tensor(rows, dtype=torch.int64).to(self.device)
        return self._tables[slot]

    def append(self, rollouts, dones, reward_scaler=None):
        """rollouts = [(steer_storage, throttle_storage), ...] of one learner section, after it ran; dones[i] = environment
        i's last `done` (unused: the masks say where episodes ended).  Device-to-device copies into the next slot (once all
        slots are filled the oldest is overwritten), then ONE cadre_sil_prepare launch over the slot's 2 N storages, with the
        reward scale finish_rollouts gave the section (the scaler's current one).  Not a hot path: one small device-to-host
        copy says whether both heads have an eligible row."""
        if len(rollouts) != self.N or len(dones) != self.N:
            raise ValueError("SelfImitationBuffer.append: %d storage pairs and %d dones for %d environments"
                             % (len(rollouts), len(dones), self.N))
        if reward_scaler is not None and reward_scaler.n_envs != self.N:
            raise ValueError("SelfImitationBuffer.append: a ReturnScaler for %d environments, a buffer for %d"
                             % (reward_scaler.n_envs, self.N))
        big = (self.steer, self.throttle)
        for s, t in rollouts:
            if (s.num_steps != self.T or t.num_steps != self.T
                    or (s._ldo, s.seq_length, s._ldh) != (self.steer._ldo, self.steer.seq_length, self.steer._ldh)):
                raise ValueError("SelfImitationBuffer.append: a storage pair whose geometry differs from the buffer's")
            if self.gamma not in (None, s.gamma) or s.gamma != t.gamma:
                raise ValueError("SelfImitationBuffer.append: storages of different gamma")
            self.gamma = s.gamma
        slot, P = self.next, self.P
        for i, pair in enumerate(rollouts):
            lo = self.base(slot, i)
            self.steer._obs[lo:lo + P].copy_(pair[0]._obs)
            for src, dst in zip(pair, big):
                for name in ("_hn", "_cn", "command", "action", "rewards", "masks", "time_limits", "value_preds"):
                    getattr(dst, name)[lo:lo + P].copy_(getattr(src, name))
        state = None if reward_scaler is None else reward_scaler.state
        hip.check(hip.lib().cadre_sil_prepare(hip.ptr(self._table(slot)), 2 * self.N, self.T, float(np.float32(self.gamma)),
                                              hip.ptr(state), float(reward_scaler.clip) if reward_scaler is not None else 0.0,
                                              TAILS.index(self.tail), self.alpha, self.prio_eps, hip.stream()),
                  "cadre_sil_prepare")
        self.next = (slot + 1) % self.M
        self.filled = min(self.M, self.filled + 1)
        self.ready = bool((self.q[:, :self.rows_filled()] > 0).any(1).all().item())

    # ------------------------------------------------------------------ the step's entries
    def _stage(self, n):
        if self._ring is None or self._ring["n"] != n:
            self._ring = dict(n=n, pos=0, slots=[
                [torch.empty(2, n, dtype=torch.int64).pin_memory(), torch.empty(2, n, dtype=torch.int64, device=self.device),
                 torch.zeros(2, n, dtype=torch.int64, device=self.device), None] for _ in range(8)])
        ring = self._ring
        stage = ring["slots"][ring["pos"]]
        ring["pos"] = (ring["pos"] + 1) % len(ring["slots"])
        if stage[3] is not None:
            stage[3].synchronize()               # (the copy that read the pinned words eight steps ago)
        return stage

    def entries(self, Bw, episode, epoch, step):
        """`blocks` gather entries of Bw SIL rows each, in the shape DemoSet.batch returns, for minibatch step `step` of epoch
        `epoch`: their index tensors live on the device and are filled by cadre_sil_draw from the words of sil_words(seed,
        rank, episode, epoch, step, Bw, blocks).  [] (and nothing is launched) while a head has no eligible row."""
        if not self.ready:
            self._last = None
            return []
        Bw = int(Bw)
        n = self.blocks * Bw
        stage = self._stage(n)
        stage[0].copy_(sil_words(self.seed, self.rank, episode, epoch, step, Bw, self.blocks))
        stage[1].copy_(stage[0], non_blocking=True)
        stage[3] = torch.cuda.Event()
        stage[3].record()
        idx = stage[2]
        hip.check(hip.lib().cadre_sil_draw(hip.ptr(self.q), self.R, self.rows_filled(), hip.ptr(stage[1]), n, hip.ptr(idx),
                                           hip.ptr(self._scratch), hip.stream()), "cadre_sil_draw")
        self._last = (idx, n)
        return [(self.steer, idx[0, k * Bw:(k + 1) * Bw], self.steer.advantages,
                 self.throttle, idx[1, k * Bw:(k + 1) * Bw], self.throttle.advantages) for k in range(self.blocks)]

    def after_step(self, B_ppo):
        """After the step that took the last entries(): the priorities of its drawn rows from the w it computed
        (cadre_sil_scatter through the update's `pos`).  B_ppo: the PPO rows of the step's minibatch."""
        if self._last is None:
            return
        idx, n = self._last
        self._last = None
        lrn = self.agent.learner
        B = int(B_ppo) + n
        w = lrn.workspace(B)
        srt = lrn.sorted_rows(B)
        hip.check(hip.lib().cadre_sil_scatter(hip.ptr(self.q), self.R, hip.ptr(idx), n, hip.ptr(w["sil_w"]),
                                              hip.ptr(w["pos"]) if srt else None, B, int(B_ppo), self.alpha, self.prio_eps,
                                              hip.stream()), "cadre_sil_scatter")

    # ------------------------------------------------------------------ statistics
    def begin_section(self, steps):
        """Before a section's first step: room for `steps` SIL statistics rows (0: none are kept)."""
        self._n_stats = 0
        if steps and (self._stats is None or self._stats.shape[0] < steps):
            self._stats = torch.zeros(int(steps), 2, hip.SIL_STATS_FIELDS, device=self.device)
        if not steps:
            self._stats = None

    def next_stats_row(self):
        if self._stats is None or self._n_stats >= self._stats.shape[0]:
            return None
        self._n_stats += 1
        return self._stats[self._n_stats - 1]

    def summary(self):
        """The "sil" entry of a section's `stats`: `filled`, `steps` (those that carried SIL rows) and, per STATS_FIELDS name,
        the (steer, throttle) pair over those steps (means; w_max the maximum).  One small device-to-host copy."""
        out = dict(filled=self.filled, steps=self._n_stats)
        if self._stats is not None and self._n_stats:
            rows = self._stats[:self._n_stats].double()
            d = torch.cat([rows.mean(0), rows.max(0).values], 1).cpu().tolist()      # [2][12]
            F = hip.SIL_STATS_FIELDS
            for k, name in enumerate(STATS_FIELDS):
                j = k + F if name == "w_max" else k
                out[name] = (d[0][j], d[1][j])
        return out


def sil_stats_text(stats):
    """What stats_line appends for a section that ran with a buffer."""
    r = stats["sil"]
    if "w_mean" not in r:
        return ", sil: %d rollouts, no rows" % r["filled"]
    return (", sil: {} rollouts, w: {:.4f}/{:.4f}, positive: {:.4f}/{:.4f}, nll: {:.4f}/{:.4f}, |R - v|: {:.4f}/{:.4f}"
            .format(r["filled"], *(r["w_mean"] + r["positive_share"] + r["nll"] + r["value_error"])))


# ----------------------------------------------------------------------------- train_cfg["self_imitation"]
def sil_config(train_cfg_value):
    """train_cfg["self_imitation"]: absent / None -> None (nothing runs, nothing is allocated, nothing is drawn); else a dict
    {"rollouts": M (required, an integer >= 1), "coeff" (required: a number, ("linear", start, end) or a callable of
    episode / max_episode — ppo_agent.train.schedule_value, written to the device block per episode as demo_mix's),
    "value_coeff" (0.01), "alpha" (0.6), "prio_eps" (1e-3), "tail" ("drop"), "blocks" (1), "seed" (0)} -> the dict with
    defaults.  The defaults are those of the paper's Atari runs (value_coeff, alpha) or plain choices (prio_eps, blocks): none
    has been tuned for this task."""
    cfg = train_cfg_value
    if cfg is None:
        return None
    if not isinstance(cfg, dict):
        raise ValueError("train_cfg.self_imitation: expected None or a dict (got %r)" % (cfg,))
    unknown = sorted(set(cfg) - set(SIL_KEYS))
    if unknown or "rollouts" not in cfg or "coeff" not in cfg:
        raise ValueError("train_cfg.self_imitation: needs rollouts and coeff; known keys %r (unknown: %r)" % (SIL_KEYS, unknown))
    M = cfg["rollouts"]
    if not _is_int(M) or M < 1:
        raise ValueError("train_cfg.self_imitation: rollouts must be an integer >= 1 (got %r)" % (M,))
    coeff = cfg["coeff"]
    if not callable(coeff):
        ok = (isinstance(coeff, (tuple, list)) and len(coeff) == 3 and coeff[0] == "linear"
              and all(_is_number(v) for v in coeff[1:])) or _is_number(coeff)
        if not ok:
            raise ValueError("train_cfg.self_imitation: coeff must be a number, (\"linear\", start, end) or a callable (got %r)"
                             % (coeff,))
        coeff = tuple(coeff) if isinstance(coeff, (tuple, list)) else float(coeff)
    vc, alpha, eps = cfg.get("value_coeff", 0.01), cfg.get("alpha", 0.6), cfg.get("prio_eps", 1e-3)
    if not _is_number(vc):
        raise ValueError("train_cfg.self_imitation: value_coeff=%r is not a finite number" % (vc,))
    if not _is_number(alpha) or not alpha > 0:
        raise ValueError("train_cfg.self_imitation: alpha=%r is not a finite number > 0" % (alpha,))
    if not _is_number(eps) or eps < 0:
        raise ValueError("train_cfg.self_imitation: prio_eps=%r is not a finite number >= 0" % (eps,))
    tail = cfg.get("tail", "drop")
    if tail not in TAILS:
        raise ValueError("train_cfg.self_imitation: tail must be one of %r (got %r)" % (TAILS, tail))
    blocks, seed = cfg.get("blocks", 1), cfg.get("seed", 0)
    if not _is_int(blocks) or blocks < 1:
        raise ValueError("train_cfg.self_imitation: blocks must be an integer >= 1 (got %r)" % (blocks,))
    if not _is_int(seed):
        raise ValueError("train_cfg.self_imitation: seed must be an integer (got %r)" % (seed,))
    return dict(rollouts=int(M), coeff=coeff, value_coeff=float(vc), alpha=float(alpha), prio_eps=float(eps), tail=tail,
                blocks=int(blocks), seed=int(seed))


class SilRunner(object):
    """train_cfg["self_imitation"] inside train() / train_vec(): buffer_for(rollouts) is the `sil` argument of the learner
    section (the buffer is allocated at the first call, from the rollouts' geometry), after_section appends to it."""

    def __init__(self, agent, cfg, rank=0):
        self.agent, self.cfg, self.rank = agent, cfg, int(rank)
        self.coeff, self.value_coeff = cfg["coeff"], cfg["value_coeff"]
        self.buffer = None

    def buffer_for(self, rollouts):
        if self.buffer is None:
            c = self.cfg
            self.buffer = SelfImitationBuffer(self.agent, c["rollouts"], len(rollouts), int(rollouts[0][0].num_steps),
                                              alpha=c["alpha"], prio_eps=c["prio_eps"], tail=c["tail"], blocks=c["blocks"],
                                              seed=c["seed"], rank=self.rank)
        return self.buffer

    def after_section(self, rollouts, dones, reward_scaler=None):
        self.buffer_for(rollouts).append(rollouts, dones, reward_scaler)


def sil_runner(agent, train_cfg_value, shared_grad_buffers=None, rank=0, in_process_chief=True, fused_gather=True,
               checkpoint_interval=None, resume_from=None, demo_mix=None, suggest=None, sample_reuse=None):
    """The SilRunner of a training loop, or None when the key is absent / None.  Refused at start-up: demo_mix and suggest (a
    row carries one kind array), sample_reuse (its stale entries and the SIL entries would both ride behind the workers'),
    checkpoint_interval / resume_from (the buffer and its priorities are not part of a checkpoint), fused_gather=False (SIL
    rows enter through the storage gather), several ranks and a chief in another process (the buffer feeds this process's own
    steps; the multi-rank form is not built)."""
    cfg = sil_config(train_cfg_value)
    if cfg is None:
        return None
    if demo_mix is not None or suggest is not None:
        raise ValueError("train_cfg.self_imitation excludes demo_mix and suggest: a row carries one kind array, and each of "
                         "the three puts its own meaning into it")
    if sample_reuse is not None:
        raise ValueError("train_cfg.self_imitation excludes sample_reuse: the SIL rows are the rows behind the PPO rows of a "
                         "minibatch, where the stale rows of the window ride")
    if checkpoint_interval is not None or resume_from is not None:
        raise ValueError("train_cfg.self_imitation excludes checkpoint_interval / resume_from: the buffer and its priorities "
                         "are not part of a checkpoint, and a resumed run would not continue with the bits of the "
                         "uninterrupted one")
    if not fused_gather:
        raise ValueError("train_cfg.self_imitation needs fused_gather=True: SIL rows enter through the storage gather of "
                         "update_policy_from_storages, not through the tuple path")
    if not in_process_chief:
        raise hip.CadreHipError("train_cfg.self_imitation needs the in-process chief: the buffer feeds this process's own steps")
    world = shared_grad_buffers.dist_world() if shared_grad_buffers is not None else 0
    if world > 1:
        raise hip.CadreHipError("train_cfg.self_imitation needs a single rank (world size %d): the multi-rank form is not "
                                "built" % world)
    return SilRunner(agent, cfg, rank)
