"""Exploration suggestions: terminal-event priors in the PPO loss (Zhang et al. 2021, "End-to-End Urban Driving by Imitating a
Reinforcement Learning Coach", the exploration loss).

An episode of this task ends with a named event, and the environment says which head was at fault.  On the last `horizon`
rows before such an event the PPO loss of that head gains  coeff * KL(pi(.|s) || p_event)  towards a prior chosen for the
event: a collision pushes the throttle head towards the brake bin, a blocked car towards the throttle bin, a deviation
pushes the steer head towards a flat prior.  Nothing is built in: priors and horizons come from train_cfg["suggest"].

    train_cfg["suggest"] = {"coeff": number | ("linear", a, b) | callable,
                            "events": {name: {"head": "steer" | "throttle", "prior": [K probabilities], "horizon": rows}}}

The pieces: RolloutStorage records a code per row (insert(event=) / insert_batch(events=), cadre_suggest_note),
RolloutStorage.mark_suggestions turns the codes into a kind per row behind finish_rollouts (cadre_suggest_mark), every
minibatch step carries the kinds into the layout of the update (cadre_suggest_rows) and the loss launch is cadre_ppo_sug_loss
(PPOLearnerHIP.set_loss("ppo+suggest")).  With the key absent nothing runs, nothing is allocated, nothing is drawn."""
import math

import numpy as np
import torch

from . import hip

MAX_KINDS = 8
HEADS = ("steer", "throttle")
SUGGEST_KEYS = ("coeff", "events")
EVENT_KEYS = ("head", "prior", "horizon")
# the seven messages with which the reference's compute_reward ends an episode at the fault of one head -> the event's name
# as a (steer_event, throttle_event) pair
MESSAGE_EVENTS = {
    "collision static": ("collision_static", None),
    "route deviation": ("route_deviation", None),
    "outside route!": ("outside_route", None),
    "collision pedestrians!": (None, "collision_pedestrian"),
    "collision vehicles!": (None, "collision_vehicle"),
    "vehicle blocked": (None, "blocked"),
    "exceed speed": (None, "exceed_speed"),
}
STANDARD_EVENTS = frozenset(n for pair in MESSAGE_EVENTS.values() for n in pair if n is not None)


def events_from_message(msg):
    """The reference's `error_message` -> (steer_event, throttle_event) names, (None, None) for any other message
    ("success", "route completion ...", ""): the env-side change is  info["suggest_event"] = events_from_message(error_message)."""
    return MESSAGE_EVENTS.get(msg, (None, None))


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def _is_number(v):
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool) and math.isfinite(float(v))


def uniform_prior(K):
    """K equal probabilities."""
    if not _is_int(K) or not 1 <= K <= 64:
        raise ValueError("uniform_prior: K=%r (1 .. 64)" % (K,))
    return [1.0 / K] * int(K)


def peaked_prior(K, bin, mass):
    """`mass` on `bin`, the rest spread evenly over the other K - 1 bins (every bin keeps a probability > 0)."""
    if not _is_int(K) or not 1 <= K <= 64 or not _is_int(bin) or not 0 <= bin < K:
        raise ValueError("peaked_prior: K=%r, bin=%r" % (K, bin))
    if K == 1:
        return [1.0]
    if not _is_number(mass) or not 0.0 < mass < 1.0:
        raise ValueError("peaked_prior: mass=%r must be in (0, 1): a zero probability makes KL(pi || p) infinite" % (mass,))
    rest = (1.0 - float(mass)) / (K - 1)
    return [float(mass) if k == bin else rest for k in range(int(K))]


def log_prior(prior):
    """Probabilities -> the fp32 log-prior row the kernel reads: normalised in float64, then log, then rounded once."""
    p = np.asarray(prior, dtype=np.float64)
    return np.log(p / p.sum()).astype(np.float32)


def _check_coeff(spec):
    if callable(spec):
        return spec
    if isinstance(spec, (tuple, list)):
        if len(spec) != 3 or spec[0] != "linear" or not _is_number(spec[1]) or not _is_number(spec[2]):
            raise ValueError("train_cfg.suggest: coeff=%r is not a number, (\"linear\", a, b) or a callable" % (spec,))
        return ("linear", float(spec[1]), float(spec[2]))
    if not _is_number(spec):
        raise ValueError("train_cfg.suggest: coeff=%r is not a number, (\"linear\", a, b) or a callable" % (spec,))
    return float(spec)


def suggest_config(train_cfg_value):
    """train_cfg["suggest"]: absent / None -> None (nothing runs, nothing is allocated, nothing is drawn); else the dict
    above -> {"coeff", "events": {name: {"head", "prior" (normalised float64 list), "log_prior" (fp32 array), "horizon"}}}
    with the events in the order given: event i gets code i + 1."""
    cfg = train_cfg_value
    if cfg is None:
        return None
    if not isinstance(cfg, dict):
        raise ValueError("train_cfg.suggest: expected None or a dict (got %r)" % (cfg,))
    unknown = sorted(set(cfg) - set(SUGGEST_KEYS))
    if unknown or "coeff" not in cfg or "events" not in cfg:
        raise ValueError("train_cfg.suggest: needs coeff and events; known keys %r (unknown: %r)" % (SUGGEST_KEYS, unknown))
    coeff = _check_coeff(cfg["coeff"])
    events = cfg["events"]
    if not isinstance(events, dict) or not events:
        raise ValueError("train_cfg.suggest: events must be a non-empty dict name -> {head, prior, horizon}")
    if len(events) > MAX_KINDS:
        raise ValueError("train_cfg.suggest: %d events; at most %d kinds" % (len(events), MAX_KINDS))
    out = {}
    for name, ev in events.items():
        if not isinstance(name, str) or not name:
            raise ValueError("train_cfg.suggest: event name %r is not a non-empty string" % (name,))
        if not isinstance(ev, dict):
            raise ValueError("train_cfg.suggest: event %r: expected a dict {head, prior, horizon}" % (name,))
        unknown = sorted(set(ev) - set(EVENT_KEYS))
        missing = sorted(set(EVENT_KEYS) - set(ev))
        if unknown or missing:
            raise ValueError("train_cfg.suggest: event %r: known keys %r (unknown: %r, missing: %r)"
                             % (name, EVENT_KEYS, unknown, missing))
        if ev["head"] not in HEADS:
            raise ValueError("train_cfg.suggest: event %r: head=%r is not 'steer' or 'throttle'" % (name, ev["head"]))
        if not _is_int(ev["horizon"]) or ev["horizon"] < 1 or ev["horizon"] >= 2 ** 31:
            raise ValueError("train_cfg.suggest: event %r: horizon=%r is not an integer of rows >= 1" % (name, ev["horizon"]))
        prior = ev["prior"]
        if isinstance(prior, (str, bytes)) or not hasattr(prior, "__len__") or not 1 <= len(prior) <= 64:
            raise ValueError("train_cfg.suggest: event %r: prior must be a list of 1 .. 64 probabilities" % (name,))
        if not all(_is_number(p) for p in prior):
            raise ValueError("train_cfg.suggest: event %r: a prior entry is not a finite number" % (name,))
        if not all(float(p) > 0.0 for p in prior):
            raise ValueError("train_cfg.suggest: event %r: every prior probability must be > 0 (KL(pi || p) is infinite "
                             "where p is zero and pi is not)" % (name,))
        p = np.asarray([float(v) for v in prior], dtype=np.float64)
        out[name] = dict(head=ev["head"], prior=(p / p.sum()).tolist(), log_prior=log_prior(p), horizon=int(ev["horizon"]))
    return dict(coeff=coeff, events=out)


class Suggestions(object):
    """The device tables of a run with train_cfg["suggest"] and the name -> code map.
    prior   float32 [2][Z + 1][64]  raw log-priors per (head, kind) in columns < K of the head, zeros elsewhere
    horizon int32   [2][Z + 1]      rows marked per (head, kind); 0 for the head an event does not belong to
    n_out = (K_steer, K_throttle): a prior's length must be its head's K."""

    def __init__(self, cfg, n_out, device):
        cfg = suggest_config(cfg)            # (the raw train_cfg["suggest"] value)
        if cfg is None:
            raise ValueError("Suggestions: no configuration")
        self.coeff = cfg["coeff"]
        self.names = list(cfg["events"])
        self.Z = len(self.names)
        self.code = {n: i + 1 for i, n in enumerate(self.names)}
        self.head = {n: HEADS.index(cfg["events"][n]["head"]) for n in self.names}
        prior = np.zeros((2, self.Z + 1, 64), dtype=np.float32)
        horizon = np.zeros((2, self.Z + 1), dtype=np.int32)
        for n in self.names:
            ev, h, z = cfg["events"][n], self.head[n], self.code[n]
            if len(ev["log_prior"]) != n_out[h]:
                raise ValueError("train_cfg.suggest: event %r: a prior of %d bins for the %s head of %d"
                                 % (n, len(ev["log_prior"]), HEADS[h], n_out[h]))
            prior[h, z, :n_out[h]] = ev["log_prior"]
            horizon[h, z] = ev["horizon"]
        self.device = torch.device(device)
        self.prior = torch.from_numpy(prior).to(self.device).contiguous()
        self.horizon = torch.from_numpy(horizon).to(self.device).contiguous()
        self._rows = None        # device float32 [steps][2][SUG_STATS_FIELDS] of the running section
        self._n = 0

    def _one(self, name, head):
        if name is None:
            return 0
        if name not in self.code:
            if name in STANDARD_EVENTS:      # an event this run has no prior for
                return 0
            raise ValueError("suggest_event %r: not an event of train_cfg.suggest %r nor one of %r"
                             % (name, self.names, sorted(STANDARD_EVENTS)))
        return self.code[name] if self.head[name] == head else 0

    def codes(self, info):
        """info["suggest_event"] -> the (steer, throttle) code pair of the row: None / key absent -> (0, 0); a name -> its
        code for the head it was configured for; a (steer, throttle) pair of names (None: no event for that head) -> the
        code of each for its own slot, 0 where the name belongs to the other head."""
        ev = info.get("suggest_event") if isinstance(info, dict) else None
        if ev is None:
            return (0, 0)
        if isinstance(ev, str):
            return (self._one(ev, 0), self._one(ev, 1))
        if isinstance(ev, (tuple, list)) and len(ev) == 2 and all(e is None or isinstance(e, str) for e in ev):
            return (self._one(ev[0], 0), self._one(ev[1], 1))
        raise ValueError("suggest_event %r: expected None, a name or a (steer, throttle) pair of names" % (ev,))

    # -- one learner section
    def mark(self, storages):
        """The mark launch for the flat storage list of a section (after finish_rollouts / compute_returns)."""
        from .ppo_agent.storage import RolloutStorage
        RolloutStorage.mark_suggestions(storages, self.Z, self.horizon)

    def begin(self, learner, steps=0):
        """Switch the learner's loss for the section; `steps` > 0: collect the suggestion statistics of that many steps.  Returns
        what learner.loss_restore takes."""
        learner.set_suggest_tables(self.prior, self.Z)
        prev = learner.loss_begin("ppo+suggest")
        self._n = 0
        if steps:
            if self._rows is None or self._rows.shape[0] < steps:
                self._rows = torch.zeros(steps, 2, hip.SUG_STATS_FIELDS, device=self.device)
        else:
            self._rows = None
        return prev

    def collect(self, learner):
        if self._rows is not None and self._n < self._rows.shape[0] and learner._last_sug_stats is not None:
            self._rows[self._n].copy_(learner._last_sug_stats)
            self._n += 1

    def summary(self):
        """stats["suggest"]: per head (steer, throttle) over the section's steps — marked rows (total), kl (mean over the
        steps of the minibatch mean), max_kl (max), p_mode (mean over the steps that had marked rows)."""
        if self._rows is None or self._n == 0:
            return None
        r = self._rows[:self._n].double().cpu().numpy()
        has = r[:, :, 0] > 0
        pm = tuple(float(r[has[:, h], h, 3].mean()) if has[:, h].any() else 0.0 for h in (0, 1))
        return dict(marked_rows=(float(r[:, 0, 0].sum()), float(r[:, 1, 0].sum())),
                    kl=(float(r[:, 0, 1].mean()), float(r[:, 1, 1].mean())),
                    max_kl=(float(r[:, 0, 2].max()), float(r[:, 1, 2].max())), p_mode=pm, steps=int(self._n))


def suggest_stats_text(stats):
    """The suffix of stats_line for a section that ran with suggestions."""
    s = stats["suggest"]
    return ", suggest rows: {:.0f}/{:.0f}, suggest kl: {:.4f}/{:.4f}".format(s["marked_rows"][0], s["marked_rows"][1],
                                                                             s["kl"][0], s["kl"][1])


def suggest_runner(agent, train_cfg_value, fused_gather=True, demo_mix=None, checkpoint_interval=None, resume_from=None):
    """The Suggestions of a training loop, or None when the key is absent / None.  Refused at start-up: fused_gather=False (the
    kinds enter beside the storage gather), train_cfg.demo_mix (rows carry one kind array: composing the two is not built),
    and checkpoint_interval / resume_from (`events` is not part of a checkpoint)."""
    cfg = suggest_config(train_cfg_value)
    if cfg is None:
        return None
    if not fused_gather:
        raise ValueError("train_cfg.suggest needs fused_gather=True: the kinds of a minibatch enter beside the storage gather "
                         "of update_policy_from_storages, not through the tuple path")
    if demo_mix is not None:
        raise ValueError("train_cfg.suggest excludes train_cfg.demo_mix: a minibatch row carries one kind array, and composing "
                         "the demonstration rows with marked rows is not built")
    if checkpoint_interval is not None or resume_from is not None:
        raise ValueError("train_cfg.suggest excludes checkpoint_interval / resume_from: the storages' events are not part of a "
                         "checkpoint, and a resumed run would not continue with the bits of the uninterrupted one")
    return Suggestions(train_cfg_value, agent.arena.n_out, agent.device)
