"""Action masks: per-row allowed-bin sets in sampling and in the PPO loss (invalid-action masking: Huang & Ontañón 2020, "A Closer
Look at Invalid Action Masking in Policy Gradient Algorithms"; MaskablePPO).

Both policy heads are categorical over ordered bins.  A row of a head carries one 64-bit word `allowed`: bit k set means bin k may be
chosen in that state (no "accelerate" bin at a red light, no extreme steer bin at speed).  The mask changes the DISTRIBUTION the head
defines, in every layer at once: the act-time samplers draw among the allowed bins and return the masked log-probability, the storages
keep the word beside the row, and the fused loss + backward kernel takes softmax, entropy and gradient over the allowed bins only, so
old_logp, the ratio and the entropy bonus all belong to the distribution that was sampled from.  A word with no bit among the head's K
bins means "unmasked".  In this code base `masks` are the episode-continuation flags of RolloutStorage; the tensors of this feature are
called `allowed`, its entry points `_am`.

    train_cfg["action_mask"] = rule            or  {"rule": rule}
    rule(obs, info) -> (steer_word, throttle_word)      called before every act; info: the last step's info of that environment (None
                                                         after a reset)

No shield rule is built in: allowed_word / allowed_from_controls build words from bins or from the agent's own control tables.

The pieces: CadreAgent.act / act_batch(allowed=) (cadre_sample_am / cadre_sample_rows_am), RolloutStorage.insert(allowed=) /
insert_batch(allowed=) (cadre_allowed_note), every minibatch step carries the words into the layout of the update (cadre_allowed_rows)
and the loss launch is cadre_ppo_am_loss (PPOLearnerHIP.set_loss("ppo+mask")).  With the key absent and allowed=None everywhere nothing
runs, nothing is allocated, and every launch is what it was."""
import numpy as np
import torch

from . import hip

HEADS = ("steer", "throttle")
ACTMASK_KEYS = ("rule",)
WORD_MAX = 2 ** 64 - 1


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def _check_K(K, who):
    if not _is_int(K) or not 1 <= K <= 64:
        raise ValueError("%s: K=%r (1 .. 64)" % (who, K))
    return int(K)


def all_word(K):
    """Every one of the K bins allowed."""
    return (1 << _check_K(K, "all_word")) - 1


def allowed_word(bins, K):
    """The word that allows exactly `bins` (a non-empty iterable of bin indices 0 .. K-1) of a head with K bins, as a Python int
    (0 .. 2^64 - 1; bit 63 is bin 63)."""
    K = _check_K(K, "allowed_word")
    w = 0
    for b in bins:
        if not _is_int(b) or not 0 <= b < K:
            raise ValueError("allowed_word: bin %r is not an index 0 .. %d" % (b, K - 1))
        w |= 1 << int(b)
    if w == 0:
        raise ValueError("allowed_word: no bin allowed (a word without a bit means 'unmasked' to the kernels; pass all_word(K))")
    return w


def _control_value(v):
    if isinstance(v, (tuple, list, np.ndarray)):
        v = v[0]
    return float(v)


def allowed_from_controls(table, lo, hi, key=None):
    """The bins of a control table whose control value lies in [lo, hi].  table: the agent's STEER_CONTROL / THROTTLE_CONTROL (a dict
    bin -> value or a sequence indexed by bin); the value of a bin is the entry itself, the first element of a (throttle, brake) pair, or
    key(entry).  Raises ValueError when no bin qualifies."""
    items = sorted(table.items()) if isinstance(table, dict) else list(enumerate(table))
    K = len(items)
    if [k for k, _ in items] != list(range(K)):
        raise ValueError("allowed_from_controls: the table's bins must be 0 .. K-1")
    val = key or _control_value
    bins = [k for k, v in items if float(lo) <= val(v) <= float(hi)]
    if not bins:
        raise ValueError("allowed_from_controls: no bin of the table has a control value in [%r, %r]" % (lo, hi))
    return allowed_word(bins, K)


def check_word(w, K, what="allowed"):
    """A Python-int word for a head of K bins -> the int, refused when it is no 64-bit word or allows none of the K bins (the kernels
    would read it as 'unmasked', which is not what an empty set says)."""
    if not _is_int(w) or not -2 ** 63 <= w <= WORD_MAX:
        raise ValueError("%s=%r: expected an integer word of 64 bits" % (what, w))
    w = int(w) & WORD_MAX
    if w & all_word(K) == 0:
        raise ValueError("%s=0x%x allows none of the head's %d bins (bit k set: bin k may be chosen; all_word(K): unmasked)"
                         % (what, w, K))
    return w


def word_i64(w):
    """0 .. 2^64 - 1 -> the int64 bit pattern the tensors hold."""
    w = int(w) & WORD_MAX
    return w - 2 ** 64 if w >= 2 ** 63 else w


def word_pair(entry, n_out, what="allowed"):
    """One environment's `allowed` entry -> the checked (steer, throttle) words."""
    if isinstance(entry, (str, bytes)) or not hasattr(entry, "__len__") or len(entry) != 2:
        raise ValueError("%s: expected a (steer_word, throttle_word) pair per environment (got %r)" % (what, entry))
    return check_word(entry[0], n_out[0], what + " (steer)"), check_word(entry[1], n_out[1], what + " (throttle)")


def words_tensor(allowed, N, n_out, device):
    """The `allowed=` argument of act / act_batch for N environments -> device int64 [N][2].  A list of N (steer, throttle) pairs of
    Python ints (each checked: an empty set is refused), or a device int64 [N][2] tensor (taken as it is: no host check, a word without
    a bit among K is 'unmasked')."""
    if torch.is_tensor(allowed):
        if allowed.dtype != torch.int64 or tuple(allowed.shape) != (N, 2) or allowed.device != torch.device(device):
            raise ValueError("allowed: expected a device int64 [%d][2] tensor on %s (got %s %s on %s)"
                             % (N, device, allowed.dtype, tuple(allowed.shape), allowed.device))
        return allowed.contiguous()
    if isinstance(allowed, (str, bytes)) or not hasattr(allowed, "__len__") or len(allowed) != N:
        raise ValueError("allowed: expected %d (steer_word, throttle_word) pairs or a device int64 [%d][2] tensor" % (N, N))
    pairs = [word_pair(e, n_out) for e in allowed]
    return torch.tensor([[word_i64(s), word_i64(t)] for s, t in pairs], dtype=torch.int64).to(device)


def actmask_config(train_cfg_value):
    """train_cfg["action_mask"]: absent / None -> None (nothing runs, nothing is allocated); a callable -> {"rule": callable}; a dict
    {"rule": callable} -> itself, checked."""
    cfg = train_cfg_value
    if cfg is None:
        return None
    if callable(cfg):
        return dict(rule=cfg)
    if not isinstance(cfg, dict):
        raise ValueError("train_cfg.action_mask: expected None, a rule callable or a dict {'rule': callable} (got %r)" % (cfg,))
    unknown = sorted(set(cfg) - set(ACTMASK_KEYS))
    if unknown or "rule" not in cfg:
        raise ValueError("train_cfg.action_mask: needs rule; known keys %r (unknown: %r)" % (ACTMASK_KEYS, unknown))
    if not callable(cfg["rule"]):
        raise ValueError("train_cfg.action_mask: rule=%r is not callable (rule(obs, info) -> (steer_word, throttle_word))" % (cfg["rule"],))
    return dict(rule=cfg["rule"])


class ActionMasks(object):
    """The section object of a run with train_cfg["action_mask"]: the rule, and the mask statistics of a learner section.
    n_out = (K_steer, K_throttle)."""

    def __init__(self, cfg, n_out, device):
        cfg = actmask_config(cfg)
        if cfg is None:
            raise ValueError("ActionMasks: no configuration")
        self.rule = cfg["rule"]
        self.n_out = (int(n_out[0]), int(n_out[1]))
        self.device = torch.device(device)
        self._rows = None        # device float32 [steps][2][AM_STATS_FIELDS] of the running section
        self._n = 0

    def words(self, obs, info=None):
        """rule(obs, info) -> the checked (steer, throttle) words of one environment's next act."""
        return word_pair(self.rule(obs, info), self.n_out, "action_mask rule")

    # -- one learner section
    def begin(self, learner, steps=0):
        """Switch the learner's loss for the section; `steps` > 0: collect the mask statistics of that many steps.  Returns what
        learner.loss_restore takes."""
        prev = learner.loss_begin("ppo+mask")
        self._n = 0
        if steps:
            if self._rows is None or self._rows.shape[0] < steps:
                self._rows = torch.zeros(steps, 2, hip.AM_STATS_FIELDS, device=self.device)
        else:
            self._rows = None
        return prev

    def step(self, learner):
        """After a minibatch step: keep its mask statistics (a device-to-device copy, no sync)."""
        if self._rows is not None and self._n < self._rows.shape[0] and learner._last_am_stats is not None:
            self._rows[self._n].copy_(learner._last_am_stats)
            self._n += 1

    def summary(self):
        """stats["actmask"]: per head (steer, throttle) over the section's steps — masked_share (rows with a proper mask), allowed_bins
        (mean number of allowed bins), pressure (the mass the unmasked head would put on forbidden bins), all means over the steps of
        the minibatch means; forced_rows (rows whose action bit had to be OR-ed in, total)."""
        if self._rows is None or self._n == 0:
            return None
        r = self._rows[:self._n].double().cpu().numpy()
        pair = lambda k, f: (float(f(r[:, 0, k])), float(f(r[:, 1, k])))
        return dict(masked_share=pair(0, np.mean), allowed_bins=pair(1, np.mean), pressure=pair(2, np.mean),
                    forced_rows=pair(3, np.sum), steps=int(self._n))


def actmask_stats_text(stats):
    """The suffix of stats_line for a section that ran with action masks."""
    s = stats["actmask"]
    return ", masked rows: {:.2f}/{:.2f}, allowed bins: {:.1f}/{:.1f}, mask pressure: {:.4f}/{:.4f}, forced: {:.0f}/{:.0f}".format(
        s["masked_share"][0], s["masked_share"][1], s["allowed_bins"][0], s["allowed_bins"][1], s["pressure"][0], s["pressure"][1],
        s["forced_rows"][0], s["forced_rows"][1])


def check_composition(fused_gather=True, demo_mix=None, suggest=None, self_imitation=None, smoothness=None, sample_reuse=None,
                      aux_phase=None, checkpoint_interval=None, resume_from=None):
    """What action masks are refused with, each with its one-line reason (the values: the train_cfg keys, or the section objects)."""
    for name, v in (("demo_mix", demo_mix), ("suggest", suggest), ("self_imitation", self_imitation), ("smoothness", smoothness),
                    ("sample_reuse", sample_reuse), ("aux_phase", aux_phase)):
        if v is not None:
            raise ValueError("train_cfg.action_mask excludes train_cfg.%s: its kernels do not read the rows' allowed-bin words yet, "
                             "and a loss that ignores the mask would train a distribution that was never sampled from" % name)
    if not fused_gather:
        raise ValueError("train_cfg.action_mask needs fused_gather=True: the words of a minibatch enter beside the storage gather "
                         "of update_policy_from_storages, not through the tuple path")
    if checkpoint_interval is not None or resume_from is not None:
        raise ValueError("train_cfg.action_mask excludes checkpoint_interval / resume_from: the storages' allowed words are not part "
                         "of a checkpoint, and a resumed run would not continue with the bits of the uninterrupted one")


def actmask_runner(agent, train_cfg_value, **composition):
    """The ActionMasks of a training loop, or None when the key is absent / None.  Refused at start-up: see check_composition."""
    cfg = actmask_config(train_cfg_value)
    if cfg is None:
        return None
    check_composition(**composition)
    return ActionMasks(train_cfg_value, agent.arena.n_out, agent.device)
