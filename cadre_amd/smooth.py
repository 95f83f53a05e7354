"""Temporal action smoothness: CAPS-style row pairs in the PPO step.

Mysore et al. 2021 ("Regularizing Action Policies for Smooth Control"), the temporal term: penalise the distance between the
policy's mean control at consecutive states, mu(s_t) and mu(s_{t+1}), and differentiate it into both rows.  Here mu is the
expected control of a head's bins, sum_k p_k c_k, the distance its square, and the successor rows ride behind the workers'
rows of every minibatch:

    sm = Smoothness(agent, coeff=0.1)
    learner_section_multi(agent, rollouts, dones, ..., smooth=sm, episode=e)    # begin_section() / step() inside

step() builds the successor entries of a minibatch step (row min(t + 1, T - 1) of the same storages, on the host),
cadre_smooth_mates places the pairs behind the gather / sort and cadre_ppo_smooth_loss runs where the PPO loss runs
(CadreAgent.update_policy_from_storages(smooth=)).  train_cfg["smoothness"] (smooth_config) wires it into train() /
train_vec().  The feature has no state of its own: the coefficient lives in the learner's device block and the pairs are a
function of the step's indices and the step number within the section.
"""
import numpy as np
import torch

from . import hip
from .phasic import _is_int, _is_number

SMOOTH_KEYS = ("coeff", "entries", "head_scale")
STATS_FIELDS = ("pairs", "abs_d", "max_abs_d", "d2")


def smooth_worker(step, E, nW, k):
    """The worker that successor entry `k` of step number `step` of a section belongs to: (step E + k) mod nW.  With E < nW the
    entries rotate over the workers, E per step."""
    if not (_is_int(step) and _is_int(E) and _is_int(nW) and _is_int(k)) or step < 0 or nW < 1 or not 1 <= E <= nW or not 0 <= k < E:
        raise ValueError("smooth_worker: step=%r, E=%r, nW=%r, k=%r (step >= 0, 1 <= E <= nW, 0 <= k < E)" % (step, E, nW, k))
    return (int(step) * int(E) + int(k)) % int(nW)


def control_values(steer, throttle):
    """float32 [2][64]: the control value of every bin — steer[k], and throttle_k - brake_k of throttle[k] = (throttle, brake) —
    formed in float64 and rounded once; columns >= K are zero."""
    steer, throttle = np.asarray(steer, np.float64), np.asarray(throttle, np.float64)
    if steer.ndim != 1 or throttle.ndim != 2 or throttle.shape[1] != 2 or not 1 <= steer.size <= 64 or not 1 <= throttle.shape[0] <= 64:
        raise ValueError("control_values: steer [K_steer], throttle [K_throttle][2] with 1 .. 64 bins each")
    if not (np.isfinite(steer).all() and np.isfinite(throttle).all()):
        raise ValueError("control_values: a control value is not finite")
    out = np.zeros((2, 64), np.float64)
    out[0, :steer.size] = steer
    out[1, :throttle.shape[0]] = throttle[:, 0] - throttle[:, 1]
    return out.astype(np.float32)


def smooth_tables(agent):
    """The control table of an agent's two heads for cadre_ppo_smooth_loss / cadre_action_jitter: device float32 [2][64] from
    its STEER_CONTROL / THROTTLE_CONTROL (ppo_agent.evaluate.control_tables)."""
    from .ppo_agent.evaluate import control_tables
    steer, thr = control_tables(agent, tuple(agent.arena.n_out))
    return torch.from_numpy(control_values(steer, thr)).to(agent.arena.device)


def successor_index(idx, T):
    """The index vector of a successor entry, on the host: min(t + 1, T - 1).  Row T is never used; a slot with t = T - 1 rides
    with its own row and is invalid."""
    return torch.clamp(idx.reshape(-1).to(torch.int64) + 1, max=int(T) - 1)


class Smoothness(object):
    """The runner of the temporal smoothness term for one agent.  coeff: a number, ("linear", start, end) or a callable of
    episode / max_episode (ppo_agent.train.schedule_value; apply_smooth writes the episode's value into the device block);
    entries: successor entries per step, 1 .. the number of workers (None: one per worker); head_scale: the two heads' factors.
    The storages of a section must hold their rows in time order in 0 .. T - 1: begin_section raises ValueError when a
    storage's cursor does not stand at T."""

    def __init__(self, agent, coeff, entries=None, head_scale=(1.0, 1.0)):
        cfg = smooth_config(dict(coeff=coeff, entries=entries, head_scale=head_scale))
        self.agent, self.coeff, self.entries, self.head_scale = agent, cfg["coeff"], cfg["entries"], cfg["head_scale"]
        self.ctrl = smooth_tables(agent)
        agent.learner.set_smooth_tables(self.ctrl, self.head_scale)
        self.step_no = 0                         # step number within the section, across epochs
        self._stats = None                       # device float32 [steps][2][SMOOTH_STATS_FIELDS] of the section
        self._n_stats = 0
        self._slots = 0                          # pair slots per step and head of the section's steps
        self._jitter = None                      # device float64 [2 N][3] of the section's storages
        self._tables = {}

    def begin_section(self, rollouts, steps=0):
        """Before the first step of a learner section.  rollouts = [(steer_storage, throttle_storage), ...]; steps: the stats
        rows to keep (0: none).  Checks the cursors, restarts the step count and runs cadre_action_jitter once on the
        section's storages."""
        flat = [s for pair in rollouts for s in pair]
        for s in flat:
            if s.step != s.num_steps:
                raise ValueError("smoothness: a storage's cursor stands at %d, not at T = %d: its rows 0 .. T - 1 are not one "
                                 "rollout in time order (rewind the cursor before the rollout: storage.step = 0)"
                                 % (s.step, s.num_steps))
        self.step_no = 0
        self._n_stats, self._slots = 0, 0
        dev = self.agent.arena.device
        self._stats = torch.zeros(int(steps), 2, hip.SMOOTH_STATS_FIELDS, device=dev) if steps else None
        self._jitter = self.jitter(flat)

    def jitter(self, storages):
        """cadre_action_jitter on the flat list [steer_0, throttle_0, ...]: device float64 [n][3] (valid pairs,
        sum |c[a_{t+1}] - c[a_t]|, max), one launch, no host sync."""
        a = self.agent.arena
        rows = tuple(p for s in storages for p in (hip.ptr(s.action), hip.ptr(s.masks),
                                                   hip.ptr(s.time_limits) if s._tl_used else 0, hip.ptr(s.command)))
        table = self._tables.get(rows)
        if table is None:
            if len(self._tables) > 16:
                self._tables.clear()
            table = self._tables[rows] = torch.tensor(rows, dtype=torch.int64).to(a.device)
        out = torch.zeros(len(storages), 3, dtype=torch.float64, device=a.device)
        hip.check(hip.lib().cadre_action_jitter(hip.ptr(table), len(storages), storages[0].num_steps, a.C, a.n_out[0], a.n_out[1],
                                                hip.ptr(self.ctrl), hip.ptr(out), hip.stream()), "cadre_action_jitter")
        return out

    def step(self, batches):
        """(entries, rotation) of the next step for update_policy_from_storages(smooth=): successor entry k carries the
        storages and advantages of worker (rotation + k) mod nW and the index vectors min(t + 1, T - 1)."""
        nW = len(batches)
        E = nW if self.entries is None else self.entries
        if E > nW:
            raise ValueError("smoothness: entries=%d with %d worker entries in the step" % (E, nW))
        rotation = self.step_no * E
        out = []
        for k in range(E):
            ss, si, sa, ts, ti, ta = batches[smooth_worker(self.step_no, E, nW, k)]
            out.append((ss, successor_index(si, ss.num_steps), sa, ts, successor_index(ti, ts.num_steps), ta))
        self.step_no += 1
        self._slots = E * batches[0][1].numel()
        return out, rotation

    def next_stats_row(self):
        if self._stats is None or self._n_stats >= self._stats.shape[0]:
            return None
        self._n_stats += 1
        return self._stats[self._n_stats - 1]

    def summary(self):
        """The "smooth" entry of a section's `stats`, (steer, throttle) pairs over the section's steps: `pairs` (valid pairs),
        `mean_abs_d` (over the valid pairs), `max_abs_d`, `d2` (mean over the pair slots, the loss before its coefficient), and
        `jitter`: what the section's rollouts did (pairs, mean and max |c[a_{t+1}] - c[a_t]|).  One small device-to-host copy."""
        out = dict(steps=self._n_stats)
        if self._stats is not None and self._n_stats:
            rows = self._stats[:self._n_stats].double()
            d = torch.cat([rows.sum(0), rows.max(0).values], 1).cpu().tolist()       # [2][8]
            F = hip.SMOOTH_STATS_FIELDS
            out["pairs"] = (d[0][0], d[1][0])
            out["mean_abs_d"] = tuple(d[h][1] * self._slots / d[h][0] if d[h][0] else 0.0 for h in range(2))
            out["max_abs_d"] = (d[0][F + 2], d[1][F + 2])
            out["d2"] = (d[0][3] / self._n_stats, d[1][3] / self._n_stats)
        if self._jitter is not None:
            j = self._jitter.view(-1, 2, 3)
            tot = torch.cat([j[:, :, :2].sum(0), j[:, :, 2:].max(0).values], 1).cpu().tolist()   # [2][3]
            out["jitter"] = dict(pairs=(tot[0][0], tot[1][0]),
                                 mean=tuple(tot[h][1] / tot[h][0] if tot[h][0] else 0.0 for h in range(2)),
                                 max=(tot[0][2], tot[1][2]))
        return out


def smooth_stats_text(stats):
    """What stats_line appends for a section that ran with the smoothness term."""
    r = stats["smooth"]
    if "pairs" not in r:
        return ", smooth: no rows"
    j = r.get("jitter", dict(mean=(0.0, 0.0)))
    return (", smooth: pairs {:.0f}/{:.0f}, |d|: {:.4f}/{:.4f}, max |d|: {:.4f}/{:.4f}, jitter: {:.4f}/{:.4f}"
            .format(*(r["pairs"] + r["mean_abs_d"] + r["max_abs_d"] + tuple(j["mean"]))))


# ----------------------------------------------------------------------------- train_cfg["smoothness"]
def smooth_config(train_cfg_value):
    """train_cfg["smoothness"]: absent / None -> None (every launch, tensor and bit is what it is without the key); else a dict
    {"coeff" (required: a number, ("linear", start, end) or a callable of episode / max_episode — ppo_agent.train.schedule_value,
    written to the device block per episode), "entries" (None: one successor entry per worker; else an integer >= 1, at most
    the number of workers — checked when a step is built), "head_scale" ((1.0, 1.0): two finite numbers >= 0)} -> the dict with
    defaults.  The defaults are plain choices: none has been tuned for this task."""
    cfg = train_cfg_value
    if cfg is None:
        return None
    if not isinstance(cfg, dict):
        raise ValueError("train_cfg.smoothness: expected None or a dict (got %r)" % (cfg,))
    unknown = sorted(set(cfg) - set(SMOOTH_KEYS))
    if unknown or "coeff" not in cfg:
        raise ValueError("train_cfg.smoothness: needs coeff; known keys %r (unknown: %r)" % (SMOOTH_KEYS, unknown))
    coeff = cfg["coeff"]
    if not callable(coeff):
        ok = (isinstance(coeff, (tuple, list)) and len(coeff) == 3 and coeff[0] == "linear"
              and all(_is_number(v) for v in coeff[1:])) or _is_number(coeff)
        if not ok:
            raise ValueError("train_cfg.smoothness: coeff must be a number, (\"linear\", start, end) or a callable (got %r)"
                             % (coeff,))
        coeff = tuple(coeff) if isinstance(coeff, (tuple, list)) else float(coeff)
    E = cfg.get("entries")
    if E is not None and (not _is_int(E) or E < 1):
        raise ValueError("train_cfg.smoothness: entries must be None or an integer >= 1 (got %r)" % (E,))
    hs = cfg.get("head_scale", (1.0, 1.0))
    if not (isinstance(hs, (tuple, list)) and len(hs) == 2 and all(_is_number(v) and v >= 0 for v in hs)):
        raise ValueError("train_cfg.smoothness: head_scale must be two finite numbers >= 0 (got %r)" % (hs,))
    return dict(coeff=coeff, entries=None if E is None else int(E), head_scale=(float(hs[0]), float(hs[1])))


def smooth_runner(agent, train_cfg_value, fused_gather=True, demo_mix=None, suggest=None, self_imitation=None, sample_reuse=None):
    """The Smoothness of a training loop, or None when the key is absent / None.  Refused at start-up: demo_mix, suggest and
    self_imitation (a row carries one kind array), sample_reuse (its stale entries and the successor entries would both ride
    behind the workers'), fused_gather=False (successor rows enter through the storage gather)."""
    cfg = smooth_config(train_cfg_value)
    if cfg is None:
        return None
    if demo_mix is not None or suggest is not None or self_imitation is not None:
        raise ValueError("train_cfg.smoothness excludes demo_mix, suggest and self_imitation: a row carries one kind array, and "
                         "each of them puts its own meaning into it")
    if sample_reuse is not None:
        raise ValueError("train_cfg.smoothness excludes sample_reuse: the successor rows are the rows behind the PPO rows of a "
                         "minibatch, where the stale rows of the window ride")
    if not fused_gather:
        raise ValueError("train_cfg.smoothness needs fused_gather=True: successor rows enter through the storage gather of "
                         "update_policy_from_storages, not through the tuple path")
    return Smoothness(agent, cfg["coeff"], cfg["entries"], cfg["head_scale"])
