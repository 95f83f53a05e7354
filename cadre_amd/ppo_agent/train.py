"""Mirror of reference ppo_agent/train.py: `train(rank, ...)` worker loop with the learner
section (train.py:76-110) factored into `learner_section` so it can be driven by replayed /
synthetic rollouts (tests, bench.py) as well as by the live CARLA `EnvWrapper`."""
import os

import numpy as np
import torch

from .. import checkpoint as ckpt
from .. import hip
from .agent import CadreAgent
from .chief import chief_step
from .models import arena_of, get_vae_output
from .storage import ReturnScaler, RolloutStorage
from .utils import check_exist


def _get(cfg, key, default=None):
    try:
        return cfg[key]
    except (KeyError, TypeError, IndexError):
        return getattr(cfg, key, default)


def _default_logger():
    """The reference logs per-episode losses through utils.logger.logger (train.py:11,104-110); use it when
    the Cadre checkout is importable, else stay silent."""
    try:
        from utils.logger import logger
        return logger
    except Exception:
        return None


# ----------------------------------------------------------------------------- update diagnostics and the KL early stop
STAT_FIELDS = ("approx_kl", "old_approx_kl", "clip_fraction", "value_clip_fraction", "ratio_mean", "max_abs_log_ratio")


def _rank_consensus(train_cfg, shared_grad_buffers=None, in_process_chief=True):
    """train_cfg["rank_consensus"] (absent / None / False: off; True).  With it the KL early stop, the KL-adaptive lr and
    reward scaling are allowed with several ranks: the few numbers the ranks must agree on (the step's two approx_kl values,
    the per-rank return statistics) are SUMMED over the ranks by one small collective per optimiser step (per rollout for
    the statistics) and the decision is taken from the sum by a kernel that runs identically on every rank — R ranks with N
    workers each decide what one rank with R N workers decides.  Needs the in-process chief and the all-reduce exchange.
    Returns whether the key is set; the consensus path itself runs only where an exchange runs (_consensus_on)."""
    on = _get(train_cfg, "rank_consensus", False)
    if on is None:
        on = False
    if not isinstance(on, (bool, np.bool_)):
        raise ValueError("train_cfg.rank_consensus: expected None, False or True (got %r)" % (on,))
    if not on:
        return False
    if not in_process_chief:
        raise hip.CadreHipError("train_cfg.rank_consensus needs the in-process chief (the decision is taken on this process's "
                                "device, between the gradient exchange and the optimiser step)")
    mode = getattr(shared_grad_buffers, "exchange_mode", None)
    if mode is not None and shared_grad_buffers.dist_world() and mode() == "sharded":
        raise hip.CadreHipError("train_cfg.rank_consensus is not available with the sharded gradient exchange "
                                "(CADRE_GRAD_EXCHANGE=sharded): the sharded optimiser step has no gated form")
    return True


def _consensus_on(train_cfg, shared_grad_buffers, in_process_chief=True):
    """Whether the consensus path runs: the key is set AND a gradient exchange runs (dist_world() >= 1; world 1 is the forced
    form, CADRE_BENCH_FORCE_DIST=1).  Without an exchange the key changes nothing: the loss kernel decides as always."""
    return bool(_rank_consensus(train_cfg, shared_grad_buffers, in_process_chief) and shared_grad_buffers is not None
                and shared_grad_buffers.dist_world() >= 1)


def _target_kl(train_cfg, shared_grad_buffers, in_process_chief=True):
    """train_cfg["target_kl"] (absent / None: no gate).  The gate is a device flag of THIS rank: ranks would disagree on it,
    so it is refused with several ranks unless train_cfg["rank_consensus"] is set; a chief in another process does not see
    it either."""
    tkl = _get(train_cfg, "target_kl")
    if tkl is None:
        return None
    tkl = float(tkl)
    if not tkl > 0.0:
        raise ValueError("train_cfg.target_kl must be > 0 (got %r)" % (tkl,))
    cons = _rank_consensus(train_cfg, shared_grad_buffers, in_process_chief)
    if not cons and shared_grad_buffers is not None and shared_grad_buffers.dist_world() > 1:
        raise hip.CadreHipError("train_cfg.target_kl needs a single rank (world size %d): the KL gate is per rank and ranks "
                                "would disagree on it; the diagnostics (log_stats) work at any world size"
                                % shared_grad_buffers.dist_world())
    if not in_process_chief:
        raise hip.CadreHipError("train_cfg.target_kl needs the in-process chief (the gate lives on this process's device)")
    return tkl


# ----------------------------------------------------------------------------- reward scaling, time limits
def _check_scaler(reward_scaler, shared_grad_buffers, train_cfg=None):
    """A ReturnScaler grows the statistics of THIS rank's environments: like target_kl it is refused with several ranks
    unless train_cfg["rank_consensus"] is set (the scale then comes from the statistics of all ranks, merged)."""
    if reward_scaler is None:
        return
    cons = train_cfg is not None and _rank_consensus(train_cfg, shared_grad_buffers)
    if not cons and shared_grad_buffers is not None and shared_grad_buffers.dist_world() > 1:
        raise hip.CadreHipError("reward scaling needs a single rank (world size %d): each rank would grow its own return "
                                "statistics and scale its rewards differently" % shared_grad_buffers.dist_world())


def _scaler_consensus(cons, reward_scaler, shared_grad_buffers):
    """The `consensus=` argument of finish_rollouts, only where the consensus path runs with a scaler (every other call is
    exactly the call it was)."""
    return dict(consensus=shared_grad_buffers) if (cons and reward_scaler is not None) else {}


def _reward_scaling(train_cfg, shared_grad_buffers=None):
    """train_cfg["reward_scaling"]: absent / None / False (off), True, or {"clip", "epsilon"} -> None or the keyword
    arguments of ReturnScaler."""
    cfg = _get(train_cfg, "reward_scaling")
    if cfg is None or cfg is False:
        return None
    if cfg is True:
        cfg = {}
    elif not isinstance(cfg, dict):
        raise ValueError("train_cfg.reward_scaling: expected None, True or a dict with clip / epsilon (got %r)" % (cfg,))
    unknown = sorted(set(cfg) - {"clip", "epsilon"})
    if unknown:
        raise ValueError("train_cfg.reward_scaling: unknown keys %r (known: clip, epsilon)" % (unknown,))
    try:
        kw = dict(clip=float(cfg.get("clip", 10.0)), epsilon=float(cfg.get("epsilon", 1e-8)))
    except (TypeError, ValueError):
        raise ValueError("train_cfg.reward_scaling: clip / epsilon of %r are not numbers" % (cfg,))
    if not 0.0 < kw["clip"] < float("inf") or not 0.0 <= kw["epsilon"] < float("inf"):
        raise ValueError("train_cfg.reward_scaling: need a finite clip > 0 and a finite epsilon >= 0 (got %r)" % (cfg,))
    cons = _rank_consensus(train_cfg, shared_grad_buffers)
    if not cons and shared_grad_buffers is not None and shared_grad_buffers.dist_world() > 1:
        raise hip.CadreHipError("train_cfg.reward_scaling needs a single rank (world size %d): each rank would grow its "
                                "own return statistics" % shared_grad_buffers.dist_world())
    return kw


# ----------------------------------------------------------------------------- training checkpoints
def _checkpointing(train_cfg, shared_grad_buffers=None):
    """train_cfg["checkpoint_interval"] (absent / None / 0: off; else a positive integer of episodes) and
    train_cfg["resume_from"] (absent / None, or the path of a checkpoint) -> (interval or None, path or None).  Like
    target_kl both are refused with several ranks: the generators and scalers of the other ranks are not captured."""
    interval, path = _get(train_cfg, "checkpoint_interval"), _get(train_cfg, "resume_from")
    if interval is not None:
        if isinstance(interval, bool) or not isinstance(interval, (int, np.integer)) or interval < 0:
            raise ValueError("train_cfg.checkpoint_interval: expected None, 0 or a positive integer of episodes (got %r)"
                             % (interval,))
        interval = int(interval) or None
    if path is not None:
        if not isinstance(path, (str, os.PathLike)) or not os.fspath(path):
            raise ValueError("train_cfg.resume_from: expected None or the path of a checkpoint (got %r)" % (path,))
        path = os.fspath(path)
    for key, v in (("checkpoint_interval", interval), ("resume_from", path)):
        if v is not None and shared_grad_buffers is not None and shared_grad_buffers.dist_world() > 1:
            raise hip.CadreHipError("train_cfg.%s needs a single rank (world size %d): the checkpoint is per rank and the "
                                    "generators and scalers of the other ranks are not captured"
                                    % (key, shared_grad_buffers.dist_world()))
    return interval, path


class _Checkpointer:
    """The checkpoint side of train() / train_vec(): resume before the first episode, a capture after every `interval`-th
    episode.  A capture is written just before the next one is taken (and before the loop returns), so the copy to the
    host runs beside the next rollout and the loop never waits for it; the newest file is therefore one interval behind
    the newest capture."""

    def __init__(self, work_dir, interval, agent, rollouts, callback=None):
        self.interval, self.agent, self.rollouts, self.callback = interval, agent, rollouts, callback
        self.dir = os.path.join(work_dir, "checkpoints")
        self.pending = None
        if interval is not None:
            check_exist(self.dir)

    def resume(self, path):
        """restore() from `path`; returns the episode the loop continues at."""
        state = ckpt.load(path)
        if state.get("episode") is None:
            raise ValueError("train_cfg.resume_from: %s holds no episode number (it was not written by a training loop)" % path)
        ckpt.restore(self.agent, state, self.rollouts, self.agent.reward_scaler)
        return int(state["episode"]) + 1

    def flush(self):
        if self.pending is not None:
            episode, cap = self.pending
            self.pending = None
            path = cap.save(os.path.join(self.dir, "ckpt_{}.pt".format(episode)))
            if self.callback is not None:
                self.callback("checkpoint", episode=episode, path=path)

    def after_episode(self, episode):
        if self.interval is None or (episode + 1) % self.interval:
            return
        self.flush()
        self.pending = (episode, ckpt.capture(self.agent, self.rollouts, self.agent.reward_scaler, episode=episode))


def _pretrain(agent, train_cfg, rollout_cfg, shared_grad_buffers, rank, logger, resume_from, shared_model_list=None,
              traffic_light=None):
    """train_cfg["pretrain"] (absent / None: nothing runs, nothing is drawn from any generator): a behaviour-cloning warm
    start from recorded episodes, once before the first rollout (cadre_amd.imitation.pretrain_from_config: rank 0 only).
    Skipped when the run resumes from a checkpoint — the checkpoint's weights already hold it."""
    cfg = _get(train_cfg, "pretrain")
    if cfg is None or resume_from is not None:
        return None
    # the warm start trains the agent's own arena with the in-process optimiser step.  With a chief in another process, or
    # shared nets in another arena (the first update_model would overwrite the result), it would be lost without a word
    if traffic_light is not None:
        raise hip.CadreHipError("train_cfg.pretrain needs the in-process chief: with a chief process the other workers would "
                                "start their rollouts beside it; pretrain once (ppo_agent.imitation.pretrain) before the "
                                "processes start")
    if shared_model_list is not None and arena_of(shared_model_list) is not agent.arena:
        raise hip.CadreHipError("train_cfg.pretrain: shared_model_list lives in another parameter arena than the agent's nets, "
                                "so the first update_model would overwrite the warm start; pretrain the shared nets "
                                "(ppo_agent.imitation.pretrain) before train() is called")
    from ..imitation import pretrain_from_config
    return pretrain_from_config(agent, cfg, rollout_cfg.gamma, train_cfg["max_grad_norm"], shared_grad_buffers, rank, logger)


def _time_limit_pair(flag):
    """info["time_limit"]: a bool, or a (steer, throttle) pair -> (steer, throttle) bools."""
    if isinstance(flag, (tuple, list)):
        return bool(flag[0]), bool(flag[1])
    return bool(flag), bool(flag)


def _scale_stats(stats, reward_scaler):
    if stats is not None and reward_scaler is not None:
        stats["reward_scale"] = tuple(reward_scaler.scale().tolist())


def _reuse_stats(stats, reuse):
    """stats["reuse"] of a section that ran with a window: `filled` and, per head, the mean ratio, truncated share,
    max |log ratio| and effective-sample share of the refresh, averaged over the stale storages (ReuseWindow.summary)."""
    if stats is not None and reuse is not None:
        stats["reuse"] = reuse.summary()


# ----------------------------------------------------------------------------- hyper-parameter schedules, KL-adaptive lr
SCHEDULED = ("lr", "clip", "ent_coeff")


def schedule_value(spec, episode, max_episode):
    """Value of a schedule at `episode` (0 .. max_episode - 1), in float64 on the host.  spec: a number (constant),
    ("linear", start, end): start + (end - start) * episode / max_episode, or a callable f(episode / max_episode)."""
    if isinstance(max_episode, bool) or not isinstance(max_episode, (int, np.integer)) or max_episode < 1:
        raise ValueError("schedule: max_episode must be a positive integer (got %r)" % (max_episode,))
    if isinstance(episode, bool) or not isinstance(episode, (int, np.integer)) or not 0 <= episode < max_episode:
        raise ValueError("schedule: episode %r outside 0 .. %d" % (episode, max_episode - 1))
    frac = float(episode) / float(max_episode)
    if callable(spec):
        v = spec(frac)
    elif isinstance(spec, (tuple, list)):
        if len(spec) != 3 or spec[0] != "linear":
            raise ValueError("schedule: expected (\"linear\", start, end), got %r" % (spec,))
        try:
            start, end = float(spec[1]), float(spec[2])
        except (TypeError, ValueError):
            raise ValueError("schedule: start / end of %r are not numbers" % (spec,))
        v = start + (end - start) * float(episode) / float(max_episode)
    elif isinstance(spec, bool) or not isinstance(spec, (int, float, np.integer, np.floating)):
        raise ValueError("schedule: expected a number, (\"linear\", start, end) or a callable, got %r" % (spec,))
    else:
        v = spec
    try:
        v = float(v)
    except (TypeError, ValueError):
        raise ValueError("schedule: %r gave %r, not a number" % (spec, v))
    if not np.isfinite(v):
        raise ValueError("schedule: %r gave %r at episode %d" % (spec, v, episode))
    return v


def _schedules(train_cfg):
    sch = _get(train_cfg, "schedules")
    if sch is None:
        return {}
    sch = dict(sch)
    unknown = sorted(set(sch) - set(SCHEDULED))
    if unknown:
        raise ValueError("train_cfg.schedules: unknown keys %r (known: %r)" % (unknown, SCHEDULED))
    return sch


def _adaptive_lr(train_cfg, shared_grad_buffers, in_process_chief=True):
    """train_cfg["adaptive_lr"] = {"desired_kl", "factor", "min", "max"} (absent / None: nothing) as the keyword arguments of
    PPOLearnerHIP.set_adaptive_lr.  The controller is a device value of THIS rank: like target_kl it is refused with
    several ranks (unless train_cfg["rank_consensus"] is set) and with a chief in another process; it excludes a schedule
    for lr."""
    cfg = _get(train_cfg, "adaptive_lr")
    if cfg is None:
        return None
    cfg = dict(cfg)
    unknown = sorted(set(cfg) - {"desired_kl", "factor", "min", "max"})
    if unknown or "desired_kl" not in cfg:
        raise ValueError("train_cfg.adaptive_lr: needs desired_kl, optional factor / min / max (got %r)" % (sorted(cfg),))
    if "lr" in _schedules(train_cfg):
        raise ValueError("train_cfg.adaptive_lr excludes train_cfg.schedules[\"lr\"]: one of them owns the learning rate")
    kw = dict(desired_kl=float(cfg["desired_kl"]), factor=float(cfg.get("factor", 1.5)), lr_min=float(cfg.get("min", 1e-5)),
              lr_max=float(cfg.get("max", 1e-2)))
    if not kw["desired_kl"] > 0.0 or not kw["factor"] > 1.0 or not 0.0 < kw["lr_min"] <= kw["lr_max"]:
        raise ValueError("train_cfg.adaptive_lr: need desired_kl > 0, factor > 1, 0 < min <= max (got %r)" % (cfg,))
    cons = _rank_consensus(train_cfg, shared_grad_buffers, in_process_chief)
    if not cons and shared_grad_buffers is not None and shared_grad_buffers.dist_world() > 1:
        raise hip.CadreHipError("train_cfg.adaptive_lr needs a single rank (world size %d): the controller is per rank and "
                                "every rank would move its own lr" % shared_grad_buffers.dist_world())
    if not in_process_chief:
        raise hip.CadreHipError("train_cfg.adaptive_lr needs the in-process chief (the learning rate lives on this process's device)")
    return kw


def apply_schedules(agent, train_cfg, episode, max_episode=None):
    """train_cfg["schedules"] at `episode`: the learner goes to device-hyper mode and gets the episode's values in one
    set_hyper (an asynchronous copy; the captured graphs are replayed as they are).  Returns the values set."""
    sch = _schedules(train_cfg)
    if not sch:
        return {}
    max_episode = _get(train_cfg, "max_episode") if max_episode is None else max_episode
    vals = {k: schedule_value(spec, episode, max_episode) for k, spec in sch.items()}
    agent.learner.set_device_hyper(True)
    agent.learner.set_hyper(**vals)
    return vals


def demo_mixer(agent, train_cfg, rollout_cfg, rank=0, fused_gather=True):
    """train_cfg["demo_mix"] (absent / None: None, and nothing runs or is drawn): the DemoMixer of a run that keeps a
    demonstration term inside every PPO step (cadre_amd.imitation.demo_mix_config for the keys).  The DemoSet is built
    once, here, before train_cfg.pretrain runs — which shares it when it names the same records and parameters.  With
    several ranks every rank draws its own rows (`rank` is part of the draw's seed) and the demonstration gradient is summed
    over the ranks by the all-reduce that sums the PPO gradient."""
    from ..imitation import demo_mix_config, demo_mixer_from_config
    cfg = demo_mix_config(_get(train_cfg, "demo_mix"))
    if cfg is None:
        return None
    if not fused_gather:
        raise ValueError("train_cfg.demo_mix needs fused_gather=True: the demonstration rows enter through the storage "
                         "gather of update_policy_from_storages, not through the tuple path")
    return demo_mixer_from_config(agent, cfg, rollout_cfg.gamma, rank)


def apply_demo_mix(agent, demo, episode, max_episode):
    """The demonstration coefficient of `episode` (DemoMixer.coeff through schedule_value) into the learner's device
    hyper-parameter block, beside apply_schedules: the learner goes to device-hyper mode, so a decaying coefficient replays
    the captured graphs as they are.  Returns the coefficient set (None without a mixer)."""
    if demo is None:
        return None
    v = schedule_value(demo.coeff, episode, max_episode)
    agent.learner.set_device_hyper(True)
    agent.learner.set_hyper(demo_coeff=v, demo_value_coeff=demo.value_coeff)
    return v


def suggestions(agent, train_cfg, fused_gather=True, ck_interval=None, ck_resume=None):
    """train_cfg["suggest"] (absent / None: None — nothing runs, nothing is allocated, nothing is drawn): the Suggestions of a
    run with terminal-event priors in the PPO loss (cadre_amd.suggest.suggest_config for the keys, suggest_runner for what is
    refused at start-up and why)."""
    cfg = _get(train_cfg, "suggest")
    if cfg is None:
        return None
    from ..suggest import suggest_runner
    return suggest_runner(agent, cfg, fused_gather, _get(train_cfg, "demo_mix"), ck_interval, ck_resume)


def action_masks(agent, train_cfg, fused_gather=True, ck_interval=None, ck_resume=None):
    """train_cfg["action_mask"] (absent / None: None — nothing runs, nothing is allocated, every launch is what it was): the
    ActionMasks of a run whose rule restricts the bins of each act (cadre_amd.actmask.actmask_config for the value,
    check_composition for what is refused at start-up)."""
    cfg = _get(train_cfg, "action_mask")
    if cfg is None:
        return None
    from ..actmask import actmask_runner
    return actmask_runner(agent, cfg, fused_gather=fused_gather, demo_mix=_get(train_cfg, "demo_mix"),
                          suggest=_get(train_cfg, "suggest"), self_imitation=_get(train_cfg, "self_imitation"),
                          smoothness=_get(train_cfg, "smoothness"), sample_reuse=_get(train_cfg, "sample_reuse"),
                          aux_phase=_get(train_cfg, "aux_phase"), checkpoint_interval=ck_interval, resume_from=ck_resume)


def _check_actmask(actmask, demo, suggest, reuse, sil, smooth, fused_gather=True):
    """A section with action masks: the other loss twins do not read the mask, and the words enter beside the fused gather."""
    if actmask is not None:
        from ..actmask import check_composition
        check_composition(fused_gather=fused_gather, demo_mix=demo, suggest=suggest, self_imitation=sil, smoothness=smooth,
                          sample_reuse=reuse)


def _loss_end(agent, *tokens):
    """The learner's loss as it was before _suggest_begin / _actmask_begin switched it (None: that one did not)."""
    for token in tokens:
        if token is not None:
            agent.learner.loss_restore(token)


def _actmask_begin(agent, actmask, stats, steps):
    """The learner's loss becomes "ppo+mask" for the section.  Returns what _loss_end takes (None without masks)."""
    if actmask is None:
        return None
    return actmask.begin(agent.learner, steps if stats is not None else 0)


def _actmask_stats(stats, actmask):
    if stats is not None and actmask is not None:
        summary = actmask.summary()
        if summary is not None:
            stats["actmask"] = summary


def apply_suggest(agent, suggest, episode, max_episode):
    """The suggestion coefficient of `episode` (Suggestions.coeff through schedule_value) into the learner's device
    hyper-parameter block, beside apply_demo_mix: a moving coefficient replays the captured graphs as they are.  Returns
    the coefficient set (None without suggestions)."""
    if suggest is None:
        return None
    v = schedule_value(suggest.coeff, episode, max_episode)
    agent.learner.set_device_hyper(True)
    agent.learner.set_hyper(suggest_coeff=v)
    return v


def _suggest_begin(agent, suggest, storages, stats, steps):
    """After the storages of a section are finished: the mark launch, then the learner's loss becomes "ppo+suggest" for the
    section.  Returns what _loss_end takes (None without suggestions)."""
    if suggest is None:
        return None
    suggest.mark(storages)
    return suggest.begin(agent.learner, steps if stats is not None else 0)


def _suggest_stats(stats, suggest):
    if stats is not None and suggest is not None:
        summary = suggest.summary()
        if summary is not None:
            stats["suggest"] = summary


def self_imitation(agent, train_cfg, shared_grad_buffers=None, rank=0, in_process_chief=True, fused_gather=True,
                   ck_interval=None, ck_resume=None):
    """train_cfg["self_imitation"] (absent / None: None — nothing runs, nothing is allocated, nothing is drawn): the SilRunner
    of a run that replays its own past successes (cadre_amd.selfimit.sil_config for the keys, sil_runner for what is refused
    at start-up and why)."""
    cfg = _get(train_cfg, "self_imitation")
    if cfg is None:
        return None
    from ..selfimit import sil_runner
    return sil_runner(agent, cfg, shared_grad_buffers, rank, in_process_chief, fused_gather, ck_interval, ck_resume,
                      _get(train_cfg, "demo_mix"), _get(train_cfg, "suggest"), _get(train_cfg, "sample_reuse"))


def apply_sil(agent, sil, episode, max_episode):
    """The SIL coefficients of `episode` (SilRunner.coeff through schedule_value, value_coeff as it is) into the learner's
    device hyper-parameter block, beside apply_demo_mix: a moving coefficient replays the captured graphs as they are.
    Returns the coefficient set (None without self-imitation)."""
    if sil is None:
        return None
    v = schedule_value(sil.coeff, episode, max_episode)
    agent.learner.set_device_hyper(True)
    agent.learner.set_hyper(sil_coeff=v, sil_value_coeff=sil.value_coeff)
    return v


def smoothness(agent, train_cfg, fused_gather=True):
    """train_cfg["smoothness"] (absent / None: None — nothing runs, nothing is allocated): the Smoothness of a run with the
    temporal action-smoothness term in the PPO step (cadre_amd.smooth.smooth_config for the keys, smooth_runner for what is
    refused at start-up and why)."""
    cfg = _get(train_cfg, "smoothness")
    if cfg is None:
        return None
    from ..smooth import smooth_runner
    return smooth_runner(agent, cfg, fused_gather, _get(train_cfg, "demo_mix"), _get(train_cfg, "suggest"),
                         _get(train_cfg, "self_imitation"), _get(train_cfg, "sample_reuse"))


def apply_smooth(agent, smooth, episode, max_episode):
    """The smoothness coefficient of `episode` (Smoothness.coeff through schedule_value) into the learner's device
    hyper-parameter block, beside apply_sil: a moving coefficient replays the captured graphs as they are.  Returns the
    coefficient set (None without the term)."""
    if smooth is None:
        return None
    v = schedule_value(smooth.coeff, episode, max_episode)
    agent.learner.set_device_hyper(True)
    agent.learner.set_hyper(smooth_coeff=v)
    return v


def curiosity(agent, train_cfg, n_envs=1, shared_grad_buffers=None, fused_gather=True, ck_interval=None, ck_resume=None):
    """train_cfg["curiosity"] (absent / None: None — nothing runs, nothing is allocated): the Curiosity of a run with the random
    network distillation bonus (cadre_amd.curiosity.curiosity_config for the keys, curiosity_refusals for what is refused at
    start-up and why)."""
    cfg = _get(train_cfg, "curiosity")
    if cfg is None:
        return None
    from ..curiosity import curiosity_runner
    return curiosity_runner(agent, cfg, n_envs, reward_scaling=_get(train_cfg, "reward_scaling"),
                            self_imitation=_get(train_cfg, "self_imitation"), sample_reuse=_get(train_cfg, "sample_reuse"),
                            checkpoint_interval=ck_interval, resume_from=ck_resume,
                            world=shared_grad_buffers.dist_world() if shared_grad_buffers is not None else 1,
                            fused_gather=fused_gather)


def apply_curiosity(cur, episode, max_episode):
    """The bonus coefficient of `episode` (Curiosity.coeff through schedule_value) into the module's own device state block —
    the learner's 16-field block is full.  No launch depends on the value.  Returns the coefficient set (None without the
    module)."""
    if cur is None:
        return None
    return cur.set_coeff(schedule_value(cur.coeff, episode, max_episode))


def _check_curiosity(cur, reward_scaler, reuse, sil, shared_grad_buffers, fused_gather=True):
    if cur is None:
        return
    if reward_scaler is not None:
        raise ValueError("curiosity excludes reward_scaler (reward_scaling: its statistics would be taken from the mixed rewards)")
    if reuse is not None or sil is not None:
        raise ValueError("curiosity excludes reuse and sil (sample_reuse, self_imitation: they read storage.rewards)")
    if shared_grad_buffers is not None and shared_grad_buffers.dist_world() > 1:
        raise ValueError("curiosity needs a single rank: each rank would train its own predictor")
    if not fused_gather:
        raise ValueError("curiosity needs fused_gather=True")


def _curiosity_end(stats, cur):
    """Behind the PPO steps of a section: the predictor steps (with one more forward for the stats entry when one is wanted)."""
    if cur is not None:
        cur.update(stats=stats is not None)


def _curiosity_stats(stats, cur):
    if stats is not None and cur is not None:
        stats["curiosity"] = cur.summary()


def cost_constraint(agent, train_cfg, n_envs=1, shared_grad_buffers=None, fused_gather=True, ck_interval=None, ck_resume=None):
    """train_cfg["cost_constraint"] (absent / None: None — nothing runs, nothing is allocated): the CostConstraint of a run that
    holds the cost rate of each head under a budget (cadre_amd.constraint.constraint_config for the keys, constraint_refusals for
    what is refused at start-up and why)."""
    cfg = _get(train_cfg, "cost_constraint")
    if cfg is None:
        return None
    from ..constraint import constraint_runner
    return constraint_runner(agent, cfg, n_envs, sample_reuse=_get(train_cfg, "sample_reuse"),
                             self_imitation=_get(train_cfg, "self_imitation"), checkpoint_interval=ck_interval, resume_from=ck_resume,
                             world=shared_grad_buffers.dist_world() if shared_grad_buffers is not None else 1,
                             fused_gather=fused_gather, demo_mix=_get(train_cfg, "demo_mix"), suggest=_get(train_cfg, "suggest"),
                             smoothness=_get(train_cfg, "smoothness"), aux_phase=_get(train_cfg, "aux_phase"))


def _check_constraint(con, reuse, sil, shared_grad_buffers, fused_gather=True, demo=None, suggest=None, smooth=None):
    if con is None:
        return
    if reuse is not None or sil is not None:
        raise ValueError("constraint excludes reuse and sil (sample_reuse, self_imitation: their rows carry no costs)")
    if shared_grad_buffers is not None and shared_grad_buffers.dist_world() > 1:
        raise ValueError("constraint needs a single rank: each rank would own a multiplier")
    if not fused_gather:
        raise ValueError("constraint needs fused_gather=True")
    if demo is not None or suggest is not None or smooth is not None:
        raise ValueError("constraint excludes demo, suggest and smooth (demo_mix, suggest, smoothness: the combination is untested)")


def _constraint_end(stats, con):
    """Behind the PPO steps of a section: the cost critics' steps (with one more forward for the stats entry when one is wanted)."""
    if con is not None:
        con.update(stats=stats is not None)


def _constraint_stats(stats, con):
    if stats is not None and con is not None:
        stats["constraint"] = con.summary()


def weight_average_config(train_cfg, shared_grad_buffers=None, in_process_chief=True, agent=None):
    """train_cfg["weight_average"] (absent / None: None — nothing is built, launched or changed): the key's dict with defaults
    (cadre_amd.average.average_config) after its refusals (average_refusals), before anything is allocated.  With `agent`, one
    more ValueError naming the key: shared nets in another parameter arena than the agent's (the optimiser then steps that
    arena, and the average would follow nothing)."""
    cfg = _get(train_cfg, "weight_average")
    if cfg is None:
        return None
    from ..average import average_config, average_refusals
    cfg = average_config(cfg)
    average_refusals(shared_grad_buffers=shared_grad_buffers, in_process_chief=in_process_chief)
    if agent is not None and shared_grad_buffers is not None and getattr(shared_grad_buffers, "arena", agent.arena) is not agent.arena:
        raise ValueError("train_cfg.weight_average: the shared nets live in another parameter arena than the agent's; the average "
                         "follows the optimiser steps of the agent's own arena")       # (the optimiser steps THAT arena: as for aux_phase)
    return cfg


def weight_average(agent, cfg):
    """The WeightAverage of a run (cfg: what weight_average_config returned; None: None), set on the agent's learner: from here
    on every in-process optimiser step is followed by the average's update."""
    if cfg is None:
        return None
    from ..average import average_runner
    avg = average_runner(agent, cfg)
    agent.learner.set_weight_average(avg)
    return avg


def _average_snapshot(agent, avg, model_dir, episode):
    if avg is not None and avg.snapshot:
        agent.save_snapshot(os.path.join(model_dir, "ppo_model_{}_avg.pt".format(episode)), weights="average")


def _average_stats(stats, agent):
    avg = getattr(agent.learner, "_avg", None)
    if stats is not None and avg is not None:
        stats["weight_average"] = avg.summary()


def _cost_kw(con, info, head=None):
    """Keyword arguments of insert (head 0 / 1) for the step's info["cost"] ({} without the module: today's call)."""
    if con is None:
        return {}
    from ..constraint import cost_pair
    return dict(cost=cost_pair(info.get("cost", 0.0))[head])


def _rewind(smooth, rollouts):
    """With the smoothness term every rollout starts at row 0 of its storages, so that rows 0 .. T - 1 are one rollout in
    time order (without it the cursors keep the reference's modulo-(T + 1) drift)."""
    if smooth is not None:
        for pair in rollouts:
            for s in pair:
                s.step = 0


def _smooth_kw(smooth, batches):
    """Keyword arguments of update_policy_from_storages for the next step of the section ({} without the term)."""
    if smooth is None:
        return {}
    kw = dict(smooth=smooth.step(batches))
    row = smooth.next_stats_row()
    if row is not None:
        kw["smooth_stats_row"] = row
    return kw


def _smooth_stats(stats, smooth):
    if stats is not None and smooth is not None:
        stats["smooth"] = smooth.summary()


def _check_smooth(smooth, demo, suggest, reuse, sil, fused_gather=True):
    if smooth is None:
        return
    if demo is not None or suggest is not None or sil is not None:
        raise ValueError("smooth excludes demo, suggest and sil (a row carries one kind array)")
    if reuse is not None:
        raise ValueError("smooth excludes reuse (the successor rows are the rows behind the PPO rows, where the stale rows ride)")
    if not fused_gather:
        raise ValueError("smooth needs fused_gather=True")


def _sil_kw(sil, Bw, episode, epoch, step):
    """Keyword arguments of update_policy_from_storages for step `step` of epoch `epoch` ({} without a buffer, or while it
    has no eligible row: the step is then the plain PPO step, launch for launch)."""
    if sil is None:
        return {}
    entries = sil.entries(Bw, episode, epoch, step)
    if not entries:
        return {}
    kw = dict(sil=entries)
    row = sil.next_stats_row()
    if row is not None:
        kw["sil_stats_row"] = row
    return kw


def _sil_stats(stats, sil):
    if stats is not None and sil is not None:
        stats["sil"] = sil.summary()


def _demo_kw(demo, Bw, episode, step, sec):
    """Keyword arguments of update_policy_from_storages for step `step` of the section ({} without a mixer)."""
    if demo is None:
        return {}
    kw = dict(demo=demo.entries(Bw, episode, step), demo_label_smoothing=demo.label_smoothing)
    if sec is not None and sec.demo_rows is not None:
        kw["demo_stats_row"] = sec.demo_rows[step]
    return kw


def demo_stats_line(episode, stats):
    """The extra `log_stats` line of a run with train_cfg.demo_mix: the imitation statistics of the demonstration rows,
    means over the section's steps."""
    d = stats["demo"]
    return ("Episode: {}, demo nll: {:.4f}/{:.4f}, demo accuracy: {:.4f}/{:.4f}, demo value error: {:.4f}/{:.4f}").format(
        episode, d["nll"][0], d["nll"][1], d["accuracy"][0], d["accuracy"][1], d["value_error"][0], d["value_error"][1])


def _aux_runner(agent, train_cfg, shared_grad_buffers, rank, in_process_chief, ck_interval, first_episode,
                shared_model_list=None):
    """train_cfg["aux_phase"] (absent / None: None — nothing runs, nothing is allocated, nothing is drawn): the PPG auxiliary
    phase every `interval` rollouts (cadre_amd.phasic.aux_config for the keys, aux_runner for what is refused at start-up)."""
    cfg = _get(train_cfg, "aux_phase")
    if cfg is None:
        return None
    if shared_model_list is not None and arena_of(shared_model_list) is not agent.arena:      # (as for train_cfg.pretrain)
        raise hip.CadreHipError("train_cfg.aux_phase: shared_model_list lives in another parameter arena than the agent's nets; "
                                "the phase steps the agent's own arena")
    from ..phasic import aux_runner
    return aux_runner(agent, cfg, shared_grad_buffers, rank, in_process_chief, ck_interval, first_episode)


def _aux_after_section(aux, agent, train_cfg, episode, rollouts, shared_grad_buffers, optimizer, log):
    """After the learner section of `episode`: its rollouts go to the phase's buffer and, every interval-th episode, the
    phase runs with the optimiser settings of the section's steps.  Returns the phase's records when it ran, else None."""
    if aux is None:
        return None
    lrn = agent.learner
    lr = _get(train_cfg, "lr")
    if lrn.device_hyper and np.isfinite(lrn.hyper("lr")):   # (the block's lr: a schedule's value, or what the section set)
        lr = lrn.hyper("lr")
    s0 = rollouts[0][0]
    return aux.after_section(episode, rollouts, len(rollouts) * (s0.num_steps // s0.mini_batch_num), shared_grad_buffers,
                             optimizer, train_cfg["max_grad_norm"], lr, log=log)


def _reuse_runner(agent, train_cfg, shared_grad_buffers, rank, in_process_chief, ck_interval, ck_resume,
                  shared_model_list=None):
    """train_cfg["sample_reuse"] (absent / None: None — nothing runs, nothing is allocated, nothing is drawn): the last M
    rollouts ride in every PPO step under V-trace (cadre_amd.reuse.reuse_config for the keys, reuse_runner for what is
    refused at start-up).  The window is allocated before the first section and appended to after every section."""
    cfg = _get(train_cfg, "sample_reuse")
    if cfg is None:
        return None
    if shared_model_list is not None and arena_of(shared_model_list) is not agent.arena:      # (as for train_cfg.aux_phase)
        raise hip.CadreHipError("train_cfg.sample_reuse: shared_model_list lives in another parameter arena than the agent's "
                                "nets; the record pass evaluates the agent's own arena")
    from ..reuse import reuse_runner
    return reuse_runner(agent, cfg, shared_grad_buffers, rank, in_process_chief, True, ck_interval, ck_resume)


def aux_stats_line(episode, records):
    """The extra `log_stats` line of an episode whose auxiliary phase ran: first against last epoch."""
    from ..phasic import aux_summary_line
    return aux_summary_line(episode, records)


def _section_hyper(agent, train_cfg, shared_grad_buffers, in_process_chief, optimizer):
    """Before a learner section: arm the KL-adaptive lr from train_cfg (the adapted lr carries over from the section before
    when the settings are the same).  Returns the lr the section hands to chief_step: the scheduled one when
    train_cfg.schedules owns lr, else train_cfg.lr."""
    alr = _adaptive_lr(train_cfg, shared_grad_buffers, in_process_chief)
    lr = _get(train_cfg, "lr")
    if alr is not None:
        if optimizer is not None:
            lr = optimizer.param_groups[0]["lr"]
        want = (alr["desired_kl"], alr["factor"], alr["lr_min"], alr["lr_max"])
        cons = _consensus_on(train_cfg, shared_grad_buffers, in_process_chief)
        if agent.learner._adaptive != want or agent.learner._cons_adaptive != cons:
            first = agent.learner._adaptive is None
            agent.learner.set_adaptive_lr(lr=(3e-4 if lr is None else float(lr)) if first else None, consensus=cons, **alr)
    elif "lr" in _schedules(train_cfg):
        if optimizer is not None:
            raise ValueError("train_cfg.schedules[\"lr\"] with an optimizer: the optimizer's lr would override the schedule")
        if not agent.learner.device_hyper:
            raise hip.CadreHipError("train_cfg.schedules: call apply_schedules(agent, train_cfg, episode) before the section")
        lr = agent.learner.hyper("lr")
    return lr


class _SectionStats:
    """Device side of a section's diagnostics: one stats row per minibatch step, the explained variance of every storage,
    and the host-side dict filled after the section's single sync."""

    def __init__(self, agent, n_steps, n_storages, consensus_world=0, demo=False):
        lrn = agent.learner
        # demonstration mixing: the imitation statistics of every step's demonstration rows
        self.demo_rows = torch.zeros(n_steps, 2, hip.BC_STATS_FIELDS, device=agent.arena.device) if demo else None
        # rank consensus: the reduced (steer, throttle) approx_kl pair of every step, as cadre_kl_consensus read it
        self.world = consensus_world
        self.gkl = torch.zeros(n_steps, 2, device=agent.arena.device) if consensus_world else None
        self.agent, self.F = agent, lrn.stats_fields()
        dev = agent.arena.device
        self.rows = torch.zeros(n_steps, 2, self.F, device=dev)
        self.ev = torch.zeros(n_storages, dtype=torch.float64, device=dev)
        self.step0 = agent.arena.step
        self.i = 0

    def next_row(self):
        r = self.rows[self.i]
        if self.gkl is not None:
            self.agent.learner._kl_sink = self.gkl[self.i]
        self.i += 1
        return r

    def finish(self, stats, gated, losses=None):
        """One device->host copy of (losses,) rows and explained variances; the host step count follows the device's."""
        parts = ([losses.double().reshape(-1)] if losses is not None else []) + [self.rows.double().reshape(-1), self.ev]
        if self.demo_rows is not None:
            parts.append(self.demo_rows.double().mean(0).reshape(-1))
        if self.gkl is not None:
            parts.append(self.gkl.double().reshape(-1))
        host = torch.cat(parts).cpu()
        nl = 0 if losses is None else losses.numel()
        tab = host[nl:nl + self.rows.numel()].view(self.rows.shape)
        ev = host[nl + self.rows.numel():nl + self.rows.numel() + self.ev.numel()].view(-1, 2)
        o_demo = nl + self.rows.numel() + self.ev.numel()
        dm = None if self.demo_rows is None else host[o_demo:o_demo + 2 * hip.BC_STATS_FIELDS].view(2, -1).tolist()
        gkl = None if self.gkl is None else host[host.numel() - self.gkl.numel():].view(-1, 2).tolist()
        applied = [bool(r[0, 6] != 0) for r in tab]
        n_applied = sum(applied)
        a, lrn = self.agent.arena, self.agent.learner
        if gated:
            a.step = self.step0 + n_applied          # = step_dev: skipped steps did not count
            if n_applied < len(applied):             # (parameters frozen mid-round: re-derive every cached copy of them)
                lrn._wp_key = None
                lrn._adam_fresh = None
        if stats is not None:
            C, names = a.C, a.model_names()
            rows = []
            for i, r in enumerate(tab.tolist()):
                d = {f: (r[0][k], r[1][k]) for k, f in enumerate(STAT_FIELDS)}
                d["applied"] = r[0][6] != 0
                if gkl is not None:                # (the SUM over the ranks: what the gate and the lr rule compared)
                    d["global_approx_kl"] = tuple(gkl[i])
                if lrn.device_hyper:               # (the lr the step's optimiser used; 0 where the row never got a step)
                    d["lr"] = r[0][hip.PPO_STATS_LR]
                # model m = kind * 2C + head * C + c (arena segment order) -> row[head][FIELDS + kind * C + c]
                d["grad_norm"] = [r[(m % (2 * C)) // C][hip.PPO_STATS_FIELDS + (m // (2 * C)) * C + m % C]
                                  for m in range(len(names))]
                rows.append(d)
            stats.clear()
            stats.update(rows=rows, model_names=names, explained_variance=[tuple(e) for e in ev.tolist()],
                         updates_applied=n_applied, steps=len(applied),
                         stopped_at_step=None if n_applied == len(applied) else applied.index(False))
            if gkl is not None:
                stats["consensus_world"] = self.world
            if dm is not None:                     # means over the section's steps, (steer, throttle)
                stats["demo"] = dict(accuracy=(dm[0][0], dm[1][0]), nll=(dm[0][1], dm[1][1]), entropy=(dm[0][2], dm[1][2]),
                                     value_error=(dm[0][3], dm[1][3]), weight=(dm[0][4], dm[1][4]), rows=(dm[0][5], dm[1][5]))
        return None if losses is None else host[:nl].view(losses.shape)


def _steps_per_epoch(storage):
    T = storage.num_steps
    return len(range(0, T, T // storage.mini_batch_num))


def stats_line(episode, stats):
    """The `log_stats` line of train() / train_vec(): means over the section's steps, explained variance averaged over
    the workers."""
    rows = stats["rows"]
    mean = lambda f, h: float(np.mean([r[f][h] for r in rows]))
    ev = np.array(stats["explained_variance"], dtype=np.float64)
    line = ("Episode: {}, approx kl: {:.6f}/{:.6f}, clip fraction: {:.4f}/{:.4f}, explained variance: {:.4f}/{:.4f}, "
            "updates applied: {}/{}, max grad norm: {:.4f}").format(
        episode, mean("approx_kl", 0), mean("approx_kl", 1), mean("clip_fraction", 0), mean("clip_fraction", 1),
        float(np.mean(ev[:, 0])), float(np.mean(ev[:, 1])), stats["updates_applied"], stats["steps"],
        max(max(r["grad_norm"]) for r in rows))
    if "lr" in rows[-1]:                               # device-hyper mode: the lr of the section's last step
        line += ", lr: {:.3e}".format(rows[-1]["lr"])
    if "reward_scale" in stats:                        # reward scaling: the scales the section's scan used
        line += ", reward scale: {:.4e}/{:.4e}".format(*stats["reward_scale"])
    if "reuse" in stats:                               # sample reuse: the importance weights of the section's refresh
        from ..reuse import reuse_stats_text
        line += reuse_stats_text(stats)
    if "suggest" in stats:                             # exploration suggestions: marked rows and the KL towards the priors
        from ..suggest import suggest_stats_text
        line += suggest_stats_text(stats)
    if "actmask" in stats:                             # action masks: masked rows, allowed bins, pressure
        from ..actmask import actmask_stats_text
        line += actmask_stats_text(stats)
    if "sil" in stats:                                 # self-imitation: the weights of the section's SIL rows
        from ..selfimit import sil_stats_text
        line += sil_stats_text(stats)
    if "smooth" in stats:                              # temporal smoothness: the pairs' |d| and the realised jitter
        from ..smooth import smooth_stats_text
        line += smooth_stats_text(stats)
    if "curiosity" in stats:                           # curiosity: the predictor's error, its scale and the bonus paid
        from ..curiosity import curiosity_stats_text
        line += curiosity_stats_text(stats)
    if "constraint" in stats:                          # cost constraint: cost rate, multiplier, the two advantage terms
        from ..constraint import constraint_stats_text
        line += constraint_stats_text(stats)
    if "weight_average" in stats:                      # weight averaging: updates, the decay used, parameter-to-average distance
        from ..average import average_stats_text
        line += average_stats_text(stats)
    return line


def _check_sil(sil, demo, suggest, reuse, path_ok=True):
    if sil is None:
        return
    if demo is not None or suggest is not None:
        raise ValueError("sil excludes demo and suggest (a row carries one kind array)")
    if reuse is not None:
        raise ValueError("sil excludes reuse (the SIL rows are the rows behind the PPO rows, where the stale rows ride)")
    if not path_ok:
        raise ValueError("sil needs fused_gather=True and the in-process chief")


def learner_section(agent, steer_rollout, throttle_rollout, done, train_cfg, shared_grad_buffers,
                    optimizer=None, traffic_light=None, counter=None, shared_model_list=None, in_process_chief=True,
                    fused_gather=True, losses_on_device=False, step_events=None, stats=None, reward_scaler=None,
                    demo=None, episode=0, reuse=None, suggest=None, sil=None, smooth=None, curiosity=None, actmask=None,
                    constraint=None):
    """train.py:76-110.  Returns (value_loss_list, policy_loss_list, ent_loss_list).
    With `in_process_chief` (one process per GPU) the optimiser step runs right after the gradient
    all-reduce instead of waiting on a separate chief process.  `fused_gather` uses the storage ->
    workspace gather kernel and keeps the per-minibatch losses on the device until the end of the
    section (same numbers as the generator/tuple path, one host sync instead of eight).
    The stored command of the bootstrap observation stays on the device (`get_last(as_tensor=True)`): the reference's
    `.item()` (storage.py:88-91) would wait for every kernel enqueued so far — the whole encoder pass — before the host
    may enqueue the rest of the section (0.5-1.1 ms of idle GPU per round).  `losses_on_device` (needs fused_gather):
    return the [steps, 3] loss tensor instead of the three lists, so the caller chooses when to wait; `step_events`:
    a list that receives one timing event before every minibatch step and one after the last.
    `stats` (a dict): the update diagnostics of the section, filled after its one host sync (with `losses_on_device` the
    section then syncs once for them): "rows" (per minibatch step: approx_kl, old_approx_kl, clip_fraction,
    value_clip_fraction, ratio_mean, max_abs_log_ratio as (steer, throttle) pairs, "applied", and "grad_norm", the
    pre-clip norm of every model in "model_names" order), "explained_variance" [(steer, throttle)], "updates_applied",
    "steps" and "stopped_at_step" (None unless the KL gate fired).
    train_cfg["rank_consensus"] (optional, True): with several ranks, target_kl, adaptive_lr and reward scaling are decided
    from numbers SUMMED over the ranks (one extra small collective per optimiser step; see _rank_consensus); each stats row
    then carries "global_approx_kl" and `stats` "consensus_world".  Without a process group the key changes nothing.
    train_cfg["target_kl"] (optional, single rank unless rank_consensus): KL early stop.  When the approx KL of a minibatch exceeds
    1.5 * target_kl in either head, the optimiser step of that minibatch and of every later one of this section is skipped
    on the device (the Stable-Baselines3 rule).  The sampler still draws every epoch's permutations, so the global CPU
    generator — and every later act() sample — does not depend on the KL outcome; forward and backward still run for
    skipped steps (their losses are returned); only the optimiser work is gated, and the Adam step count equals the
    number of applied steps.
    `reward_scaler` (a ReturnScaler for one environment, single rank only): return-based reward scaling.  With it, or when
    a storage holds time-limit flags, the two storages are finished by RolloutStorage.finish_rollouts (see there);
    otherwise by today's two compute_returns calls.
    `demo` (a DemoMixer, needs fused_gather) with `episode`: every minibatch step also carries demo.entries(rows per
    minibatch, episode, step) — the mixed loss of update_policy_from_storages(demo=); `stats` then holds "demo" (accuracy,
    nll, entropy, value_error, weight, rows as (steer, throttle) means over the section's steps).  A step the KL gate
    stops skips the demonstration term with the rest of the update.
    `reuse` (a cadre_amd.reuse.ReuseWindow for one environment, needs fused_gather and the in-process chief) with
    `episode`: sample reuse, as in learner_section_multi.
    `suggest` (a cadre_amd.suggest.Suggestions, needs fused_gather, excludes `demo`): exploration suggestions, as in
    learner_section_multi.
    `sil` (a cadre_amd.selfimit.SelfImitationBuffer for one environment; needs fused_gather and the in-process chief,
    excludes `demo`, `suggest` and `reuse`) with `episode`: self-imitation, as in learner_section_multi.
    `smooth` (a cadre_amd.smooth.Smoothness; needs fused_gather, excludes `demo`, `suggest`, `sil` and `reuse`): the temporal
    smoothness term, as in learner_section_multi.  Raises ValueError when a storage's cursor does not stand at T.
    `curiosity` (a cadre_amd.curiosity.Curiosity for one environment; needs fused_gather and a single rank, excludes
    `reward_scaler`, `reuse` and `sil`): the random network distillation bonus, as in learner_section_multi; the two storages
    are then finished by RolloutStorage.finish_rollouts.
    `actmask` (a cadre_amd.actmask.ActionMasks; needs fused_gather, excludes `demo`, `suggest`, `sil`, `smooth` and `reuse`):
    action masks, as in learner_section_multi.
    `constraint` (a cadre_amd.constraint.CostConstraint for one environment; needs fused_gather and a single rank, excludes
    `reuse`, `sil`, `demo`, `suggest` and `smooth`): the cost constraint, as in learner_section_multi."""
    _check_constraint(constraint, reuse, sil, shared_grad_buffers, fused_gather, demo, suggest, smooth)
    _check_actmask(actmask, demo, suggest, reuse, sil, smooth, fused_gather)
    _check_smooth(smooth, demo, suggest, reuse, sil, fused_gather)
    _check_curiosity(curiosity, reward_scaler, reuse, sil, shared_grad_buffers, fused_gather)
    if demo is not None and not fused_gather:
        raise ValueError("demo needs fused_gather=True")
    _check_sil(sil, demo, suggest, reuse, fused_gather and in_process_chief)
    if suggest is not None and (not fused_gather or demo is not None):
        raise ValueError("suggest needs fused_gather=True and excludes demo (a row carries one kind array)")
    if reuse is not None and not (fused_gather and in_process_chief):
        raise ValueError("reuse needs fused_gather=True and the in-process chief")
    _check_scaler(reward_scaler, shared_grad_buffers, train_cfg)
    tkl = _target_kl(train_cfg, shared_grad_buffers, in_process_chief)
    cons = _consensus_on(train_cfg, shared_grad_buffers, in_process_chief)
    lr = _section_hyper(agent, train_cfg, shared_grad_buffers, in_process_chief, optimizer)
    use_adv_norm = train_cfg["use_adv_norm"]
    sec = None
    if stats is not None or tkl is not None:
        sec = _SectionStats(agent, train_cfg["ppo_epoch"] * _steps_per_epoch(steer_rollout), 2,
                            consensus_world=shared_grad_buffers.dist_world() if cons else 0,
                            demo=demo is not None and stats is not None)
        agent.learner.set_update_modes(stats=True, target_kl=tkl, consensus=cons)
    try:
        out = _learner_section(agent, steer_rollout, throttle_rollout, done, train_cfg, shared_grad_buffers, optimizer,
                               traffic_light, counter, shared_model_list, in_process_chief, fused_gather, losses_on_device,
                               step_events, use_adv_norm, sec, lr, reward_scaler, cons, demo, episode, reuse, suggest,
                               stats, sil, smooth, curiosity, actmask, constraint)
    finally:
        if sec is not None:
            agent.learner.set_update_modes()
    _curiosity_end(stats, curiosity)
    _constraint_end(stats, constraint)
    if sec is None:
        return out
    if losses_on_device:
        sec.finish(stats, tkl is not None)
        _scale_stats(stats, reward_scaler)
        _reuse_stats(stats, reuse)
        _suggest_stats(stats, suggest)
        _actmask_stats(stats, actmask)
        _sil_stats(stats, sil)
        _smooth_stats(stats, smooth)
        _curiosity_stats(stats, curiosity)
        _constraint_stats(stats, constraint)
        _average_stats(stats, agent)
        return out
    dev_losses, (vl, pl, el) = out
    host = sec.finish(stats, tkl is not None, losses=torch.stack(dev_losses) if dev_losses else None)
    _scale_stats(stats, reward_scaler)
    _reuse_stats(stats, reuse)
    _suggest_stats(stats, suggest)
    _actmask_stats(stats, actmask)
    _sil_stats(stats, sil)
    _smooth_stats(stats, smooth)
    _curiosity_stats(stats, curiosity)
    _constraint_stats(stats, constraint)
    _average_stats(stats, agent)
    if host is not None:
        for v, p, e in host.tolist():
            vl.append(v); pl.append(p); el.append(e)
    return vl, pl, el


def _learner_section(agent, steer_rollout, throttle_rollout, done, train_cfg, shared_grad_buffers, optimizer, traffic_light,
                     counter, shared_model_list, in_process_chief, fused_gather, losses_on_device, step_events, use_adv_norm,
                     sec, lr, reward_scaler=None, cons=False, demo=None, episode=0, reuse=None, suggest=None, stats=None,
                     sil=None, smooth=None, curiosity=None, actmask=None, constraint=None):
    if smooth is not None:                           # (the cursor check comes before any launch of the section)
        smooth.begin_section([(steer_rollout, throttle_rollout)],
                             train_cfg["ppo_epoch"] * _steps_per_epoch(steer_rollout) if stats is not None else 0)
    nv_s, nv_t = agent.get_value(done, steer_rollout.get_last(as_tensor=True), throttle_rollout.get_last(as_tensor=True))
    if curiosity is not None:
        curiosity.begin_section([(steer_rollout, throttle_rollout)])
    if constraint is not None:
        constraint.begin_section([(steer_rollout, throttle_rollout)], [done])
    if curiosity is not None or reward_scaler is not None or steer_rollout._tl_used or throttle_rollout._tl_used:
        steer_adv, throttle_adv = RolloutStorage.finish_rollouts(
            [steer_rollout, throttle_rollout], [nv_s.detach(), nv_t.detach()], normalise=use_adv_norm,
            reward_scaler=reward_scaler, explained_variance=None if sec is None else sec.ev,
            **_scaler_consensus(cons, reward_scaler, shared_grad_buffers),
            **({} if curiosity is None else dict(intrinsic=curiosity)))
    else:
        steer_adv = steer_rollout.compute_returns(nv_s.detach(), normalise=use_adv_norm,
                                                  explained_variance=None if sec is None else sec.ev[0:1])
        throttle_adv = throttle_rollout.compute_returns(nv_t.detach(), normalise=use_adv_norm,
                                                        explained_variance=None if sec is None else sec.ev[1:2])
    if constraint is not None:                       # (behind the reward advantages, whichever launch wrote them)
        constraint.mix([(steer_rollout, throttle_rollout)])
    if reuse is not None:
        reuse.refresh(use_adv_norm, reward_scaler)
    sug_prev = _suggest_begin(agent, suggest, [steer_rollout, throttle_rollout], stats,
                              train_cfg["ppo_epoch"] * _steps_per_epoch(steer_rollout))
    if sil is not None:
        sil.begin_section(train_cfg["ppo_epoch"] * _steps_per_epoch(steer_rollout) if stats is not None else 0)
    am_prev = _actmask_begin(agent, actmask, stats, train_cfg["ppo_epoch"] * _steps_per_epoch(steer_rollout))
    try:
        return _learner_steps(agent, steer_rollout, throttle_rollout, steer_adv, throttle_adv, train_cfg, shared_grad_buffers,
                              optimizer, traffic_light, counter, shared_model_list, in_process_chief, fused_gather,
                              losses_on_device, step_events, sec, lr, demo, episode, reuse, suggest, sil, smooth, actmask)
    finally:
        _loss_end(agent, sug_prev, am_prev)


def _learner_steps(agent, steer_rollout, throttle_rollout, steer_adv, throttle_adv, train_cfg, shared_grad_buffers, optimizer,
                   traffic_light, counter, shared_model_list, in_process_chief, fused_gather, losses_on_device, step_events, sec,
                   lr, demo, episode, reuse, suggest, sil=None, smooth=None, actmask=None):
    dev_losses = []
    vl, pl, el = [], [], []
    n_step = 0
    # several ranks, CADRE_GRAD_BUCKETS=1: gradient buckets leave as soon as they are final, beside the rest of the backward
    # (Shared_grad_buffers.overlap_hook) — only with the in-process chief, which collects them in chief_step, and only
    # when the agent's nets live in the arena behind `shared_grad_buffers` (a foreign worker arena is ADDED afterwards)
    hook = shared_grad_buffers.overlap_hook(arena_of(agent.model_dict)) if in_process_chief else None
    for epoch in range(train_cfg["ppo_epoch"]):
        if fused_gather:
            idx_s, idx_t = steer_rollout.sample_indices(), throttle_rollout.sample_indices()   # steer draws first
            steps = [("idx", a, b) for a, b in zip(idx_s, idx_t)]
        else:
            steps = [("tup", a, b) for a, b in zip(steer_rollout.feed_forward_generator(steer_adv),
                                                     throttle_rollout.feed_forward_generator(throttle_adv))]
        for j, (kind, a, b) in enumerate(steps):
            if step_events is not None:
                step_events.append(torch.cuda.Event(enable_timing=True)); step_events[-1].record()
            row = None if sec is None else sec.next_row()
            if kind == "idx":
                stale = [] if reuse is None else reuse.entries(episode, epoch, j, a.numel())
                live = [(steer_rollout, a, steer_adv, throttle_rollout, b, throttle_adv)]
                dev_losses.append(agent.update_policy_from_storages(
                    live + stale, sync=False, mlp_grads_ready=hook,
                    stats_row=row, **_demo_kw(demo, a.numel(), episode, n_step, sec),
                    **_sil_kw(sil, a.numel(), episode, epoch, j), **_smooth_kw(smooth, live),
                    **({} if actmask is None else dict(actmask=actmask))))
                if suggest is not None:
                    suggest.collect(agent.learner)
                if sil is not None:
                    sil.after_step(a.numel())
            else:
                v, p, e = agent.update_policy(a, b, stats_row=row)
                vl.append(v); pl.append(p); el.append(e)
            n_step += 1
            if in_process_chief:
                shared_grad_buffers.add_gradient(agent.model_dict)
                # (the next writer of the gradient arena is the next fused update, which overwrites every element)
                chief_step(shared_grad_buffers, optimizer, train_cfg["max_grad_norm"], lr=lr, zero_grads=False)
            else:
                signal_init = traffic_light.get()
                shared_grad_buffers.add_gradient(agent.model_dict)
                counter.increment()
                while traffic_light.get() == signal_init:
                    pass
            if shared_model_list is not None:
                agent.update_model(shared_model_list)
    if step_events is not None:
        step_events.append(torch.cuda.Event(enable_timing=True)); step_events[-1].record()
    if losses_on_device:
        if not dev_losses:
            raise ValueError("losses_on_device needs fused_gather=True")
        return torch.stack(dev_losses)
    if sec is not None:                              # (the caller syncs once for the losses and the diagnostics together)
        return dev_losses, (vl, pl, el)
    if dev_losses:
        for v, p, e in torch.stack(dev_losses).tolist():
            vl.append(v); pl.append(p); el.append(e)
    return vl, pl, el


def train(rank, train_cfg, agent_cfg, env_cfg, rollout_cfg, traffic_light=None, counter=None,
          shared_model_list=None, shared_grad_buffers=None, son_process_counter=None, env_cls=None, logger=None,
          recorder=None):
    if env_cls is None:
        from env_wrapper import EnvWrapper as env_cls        # needs the CARLA stack (reference env_wrapper.py)
    if logger is None:
        logger = _default_logger()
    env_cfg.rank = rank
    for k in ("port", "routes", "scenarios", "town"):
        env_cfg[k] = env_cfg[k][rank]
    env_cfg.seq_length = rollout_cfg.seq_length
    env = env_cls(env_cfg)
    model_dir = os.path.join(env.work_dir, "models")
    check_exist(model_dir)
    num_steps = rollout_cfg.num_steps
    hidden_size, _ = get_vae_output(agent_cfg.model_cfg)
    agent_cfg.rank = rank
    agent = CadreAgent(**agent_cfg)
    device = torch.device("cuda:" + str(agent_cfg.model_cfg.device_num))
    rollout_cfg.hidden_size = hidden_size
    steer_rollout = RolloutStorage(**rollout_cfg); steer_rollout.to(device)
    throttle_rollout = RolloutStorage(**rollout_cfg); throttle_rollout.to(device)
    if shared_grad_buffers is None:              # single-process use: the agent's own arena is the shared one
        from .models import Shared_grad_buffers
        shared_grad_buffers = Shared_grad_buffers(agent.model_dict, device)
    rs = _reward_scaling(train_cfg, shared_grad_buffers)
    agent.reward_scaler = None if rs is None else ReturnScaler(1, rollout_cfg.gamma, device=device, **rs)
    ck_interval, ck_resume = _checkpointing(train_cfg, shared_grad_buffers)
    # (refusals first: before a checkpoint is read or anything else is built)
    cur = agent.curiosity = curiosity(agent, train_cfg, 1, shared_grad_buffers, True, ck_interval, ck_resume)
    con = agent.constraint = cost_constraint(agent, train_cfg, 1, shared_grad_buffers, True, ck_interval, ck_resume)
    avg_cfg = weight_average_config(train_cfg, shared_grad_buffers, traffic_light is None, agent)
    ck, first_episode, avg = None, 0, None
    if ck_interval is not None or ck_resume is not None:
        ck = _Checkpointer(env.work_dir, ck_interval, agent, [(steer_rollout, throttle_rollout)])
        if ck_resume is not None:                # (the environment is the caller's: it restarts through reset())
            avg = weight_average(agent, avg_cfg)      # (before the restore, which fills it; no warm start runs)
            first_episode = ck.resume(ck_resume)
    suggest = suggestions(agent, train_cfg, True, ck_interval, ck_resume)      # (refusals first: before anything is loaded)
    actmask = action_masks(agent, train_cfg, True, ck_interval, ck_resume)
    demo = demo_mixer(agent, train_cfg, rollout_cfg, rank)          # (before the warm start, which shares its DemoSet)
    _pretrain(agent, train_cfg, rollout_cfg, shared_grad_buffers, rank, logger, ck_resume, shared_model_list, traffic_light)
    if ck_resume is None:                        # (behind the warm start: the average starts from its result)
        avg = weight_average(agent, avg_cfg)
    aux = _aux_runner(agent, train_cfg, shared_grad_buffers, rank, traffic_light is None, ck_interval, first_episode,
                      shared_model_list)
    reuse = _reuse_runner(agent, train_cfg, shared_grad_buffers, rank, traffic_light is None, ck_interval, ck_resume,
                          shared_model_list)
    sil = self_imitation(agent, train_cfg, shared_grad_buffers, rank, traffic_light is None, True, ck_interval, ck_resume)
    smooth = smoothness(agent, train_cfg)
    obs = env.reset()
    done = False
    info = None                                  # (the action-mask rule sees the last step's info; None after a reset)
    log_stats = bool(_get(train_cfg, "log_stats", False))
    for episode in range(first_episode, train_cfg.max_episode):
        _rewind(smooth, [(steer_rollout, throttle_rollout)])
        for _ in range(num_steps):
            command = obs["command"]
            raw = dict(obs, rgb=obs["rgb"].copy(), route_fig=obs["route_fig"].copy()) if recorder is not None else None
            words = None if actmask is None else actmask.words(obs, info)      # (key absent: today's call)
            feat, action, alp, values, hidden = agent.act(obs, **({} if words is None else dict(allowed=words)))
            obs, reward, done, info = env.step(agent.convert_action(action))
            ad = info["action_done"]
            if recorder is not None:            # cadre_amd.replay.RolloutRecorder
                recorder.step(raw, action, alp, values, reward, ad)
            tl = _time_limit_pair(info.get("time_limit", False))        # (key absent: no flag is ever written)
            ev = ({}, {}) if suggest is None else tuple(dict(event=c) for c in suggest.codes(info))   # (key absent: today's call)
            if words is not None:
                nS, nT = agent.arena.n_out
                ev = (dict(ev[0], allowed=words[0], allowed_bins=nS), dict(ev[1], allowed=words[1], allowed_bins=nT))
            steer_rollout.insert(feat, action[0], alp[0], values[0], reward[0],
                                 torch.tensor([[0.0] if ad[0] else [1.0]]), hidden, command, time_limit=tl[0],
                                 **ev[0], **_cost_kw(con, info, 0))
            throttle_rollout.insert(feat, action[1], alp[1], values[1], reward[1],
                                    torch.tensor([[0.0] if ad[1] else [1.0]]), hidden, command, time_limit=tl[1],
                                    **ev[1], **_cost_kw(con, info, 1))
            if done:
                obs, info = env.reset(), None
        if recorder is not None:
            recorder.end_episode()
        stats = {} if log_stats else None
        apply_schedules(agent, train_cfg, episode)
        apply_demo_mix(agent, demo, episode, train_cfg.max_episode)
        apply_suggest(agent, suggest, episode, train_cfg.max_episode)
        apply_sil(agent, sil, episode, train_cfg.max_episode)
        apply_smooth(agent, smooth, episode, train_cfg.max_episode)
        apply_curiosity(cur, episode, train_cfg.max_episode)
        vl, pl, el = learner_section(agent, steer_rollout, throttle_rollout, done, train_cfg, shared_grad_buffers,
                                     traffic_light=traffic_light, counter=counter,
                                     shared_model_list=shared_model_list,
                                     in_process_chief=traffic_light is None, stats=stats,   # no chief process -> step in-process
                                     reward_scaler=agent.reward_scaler, demo=demo, episode=episode,
                                     **({} if reuse is None else dict(reuse=reuse.window_for([(steer_rollout, throttle_rollout)]))),
                                     **({} if suggest is None else dict(suggest=suggest)),
                                     **({} if actmask is None else dict(actmask=actmask)),
                                     **({} if sil is None else dict(sil=sil.buffer_for([(steer_rollout, throttle_rollout)]))),
                                     **({} if smooth is None else dict(smooth=smooth)),
                                     **({} if cur is None else dict(curiosity=cur)),
                                     **({} if con is None else dict(constraint=con)))
        log_now = episode % train_cfg.log_interval == 0 and rank == 0 and logger is not None
        # (the auxiliary phase: before the log line, the snapshot and the checkpoint, which then see its result)
        aux_records = _aux_after_section(aux, agent, train_cfg, episode, [(steer_rollout, throttle_rollout)],
                                         shared_grad_buffers, None, logger if log_now else None)
        if reuse is not None:                    # (after the PPG buffer took its copy: the two are independent)
            reuse.after_section([(steer_rollout, throttle_rollout)], [done])
        if sil is not None:                      # (the section's rollouts become replayable from the next section on)
            sil.after_section([(steer_rollout, throttle_rollout)], [done], agent.reward_scaler)
        if log_now:
            logger.log("Episode: {}, value loss: {:.4f}, policy loss: {:.4f}, entropy loss: {:.4f}".format(
                episode, np.mean(vl), np.mean(pl), np.mean(el)))
            if log_stats:
                logger.log(stats_line(episode, stats))
                if demo is not None:
                    logger.log(demo_stats_line(episode, stats))
                if aux_records:
                    logger.log(aux_stats_line(episode, aux_records))
        if episode % train_cfg.save_interval == 0 and rank == 0:
            agent.save_snapshot(os.path.join(model_dir, "ppo_model_{}.pt".format(episode)))
            _average_snapshot(agent, avg, model_dir, episode)
        if ck is not None:                       # (after the snapshot: building its nn.Modules draws from the generator)
            ck.after_episode(episode)
    if ck is not None:
        ck.flush()
    if son_process_counter is not None:
        son_process_counter.increment()
    print("process {} finished.".format(rank))


# ----------------------------------------------------------------------------- N environments in one process
def learner_section_multi(agent, rollouts, dones, train_cfg, shared_grad_buffers, optimizer=None, losses_on_device=False,
                          stats=None, reward_scaler=None, demo=None, episode=0, reuse=None, suggest=None, sil=None,
                          smooth=None, curiosity=None, actmask=None, constraint=None):
    """train.py:76-110 for N workers that share one agent (`num_processes = N` on one GPU, chief.py:13-21 semantics):
    rollouts = [(steer_rollout, throttle_rollout), ...] per worker, dones[i] = worker i's last `done`.  Bootstrap values
    of all workers in one pass (get_values), GAE + advantage normalisation per storage, then for each ppo_epoch and
    minibatch ONE update over the N workers' minibatches (update_policy_from_storages: the losses and gradients are the
    SUM of the per-worker ones) followed by the in-process chief_step: one optimiser step per barrier.
    Sampler order: every epoch draws, from the global CPU generator, worker 0 steer, worker 0 throttle, worker 1 steer,
    ... — one torch.randperm(T) each.  (N processes each draw from their own generator; one process cannot reproduce
    that stream, so this is the documented order of the single-process form.)  Returns (value_loss_list,
    policy_loss_list, ent_loss_list), or the [steps, 3] loss tensor with `losses_on_device`.
    `stats` and train_cfg["target_kl"]: as in learner_section ("explained_variance" holds one (steer, throttle) pair per
    worker, all 2N storages in one launch after their GAE).  The diagnostics of a step are taken over the N workers'
    minibatches with the losses' denominator: like the losses, they are the SUM of the per-worker means.
    The 2N storages are finished by ONE RolloutStorage.finish_rollouts launch (bit-identical to 2N compute_returns calls
    when no time-limit flag was written and `reward_scaler`, a ReturnScaler for N environments, is None).
    `demo` (a DemoMixer) with `episode`: as in learner_section — demo.blocks entries of one worker minibatch's size behind
    the N workers' entries of every step.
    `reuse` (a cadre_amd.reuse.ReuseWindow for N environments) with `episode`: sample reuse.  After the live storages are
    finished, reuse.refresh() re-evaluates the window's rows under the current nets and runs the V-trace scan; every step's
    entries are then the N live ones followed by reuse.entries(episode, epoch, step, rows per minibatch), one per stale
    storage pair, ahead of any demonstration entries (whose n_ppo counts the stale rows).  Losses and gradients are the SUM
    over (1 + filled) N per-worker means, the convention above: the gradient scale grows with the window, to which Adam is
    indifferent up to max_grad_norm, whose clip engages earlier.  approx_kl keeps its meaning (movement within this
    update: a stale row's old_logp is its log-probability at the start of the update); explained variance and the KL
    gate are untouched.  `stats` gains "reuse" (see _reuse_stats; one more small device-to-host copy).  The caller appends
    the section's rollouts to the window afterwards (reuse.append).
    `suggest` (a cadre_amd.suggest.Suggestions; excludes `demo`): exploration suggestions.  After the storages are finished one
    launch marks their rows from the recorded events (RolloutStorage.mark_suggestions), the learner's loss becomes
    "ppo+suggest" for the section, and every step carries the kinds of its rows into the update's layout
    (cadre_suggest_rows) before the update; the rows of stale `reuse` entries get kind 0.  Marks are rank-local, and the
    gradient is summed by the exchange that sums the PPO gradient.  `stats` gains "suggest" (marked_rows, kl, max_kl,
    p_mode as (steer, throttle) pairs over the section's steps; one more small device-to-host copy).
    `sil` (a cadre_amd.selfimit.SelfImitationBuffer for N environments; excludes `demo`, `suggest` and `reuse`) with `episode`:
    self-imitation.  Every step draws sil.entries(rows per minibatch, episode, epoch, step) on the device (cadre_sil_draw), the
    entries ride behind the workers' and the step runs the mixed loss (update_policy_from_storages(sil=)), then
    sil.after_step() writes the drawn rows' priorities back from the w the step computed (cadre_sil_scatter).  While the buffer
    has no eligible row in a head the step is the plain PPO step, launch for launch.  `stats` gains "sil" (filled, steps,
    w_mean, positive_share, nll, value_error, w_max, rows as (steer, throttle) pairs; one more small device-to-host copy).  The
    caller appends the section's rollouts to the buffer afterwards (sil.append).
    `smooth` (a cadre_amd.smooth.Smoothness; excludes `demo`, `suggest`, `sil` and `reuse`): the temporal action-smoothness
    term.  Every step carries smooth.step(batches) — E successor entries (row min(t + 1, T - 1) of the storages of E of the N
    workers, rotating with the step number of the section) behind the workers' entries — and runs the mixed loss
    (update_policy_from_storages(smooth=)); the KL gate, the diagnostics and the adaptive lr see the PPO rows only.  The
    rows of every storage must lie in time order in 0 .. T - 1: ValueError when a storage's cursor does not stand at T when
    the section starts.  `stats` gains "smooth" (pairs, mean_abs_d, max_abs_d, d2 as (steer, throttle) pairs and "jitter",
    what the section's rollouts did: one cadre_action_jitter launch per section; one more small device-to-host copy).
    `curiosity` (a cadre_amd.curiosity.Curiosity for N environments; single rank, excludes `reward_scaler`, `reuse` and `sil`):
    the random network distillation bonus.  Before the storages are finished curiosity.begin_section(rollouts) scores the
    section's rows and writes every storage's `rewards_mixed`, which finish_rollouts(intrinsic=) hands to the GAE launch in
    place of `rewards`; behind the PPO steps curiosity.update() runs the predictor's steps.  `stats` gains "curiosity" (mean_e,
    max_e, sigma, beta, mean_abs_bonus, mean_abs_ext, steps, loss_before, loss_after; one more small device-to-host copy).
    `actmask` (a cadre_amd.actmask.ActionMasks; excludes `demo`, `suggest`, `sil`, `smooth` and `reuse`, whose kernels do not read
    the mask): action masks.  The learner's loss becomes "ppo+mask" for the section and every step carries the `allowed` words
    of its rows (what insert_batch(allowed=) stored beside them) into the update's layout (cadre_allowed_rows) before the
    update, whose loss launch is cadre_ppo_am_loss.  The loss is per rank and nothing new is exchanged.  `stats` gains
    "actmask" (masked_share, allowed_bins, pressure, forced_rows as (steer, throttle) pairs; one more small device-to-host
    copy).
    `constraint` (a cadre_amd.constraint.CostConstraint for N environments; single rank, excludes `reuse`, `sil`, `demo`, `suggest`
    and `smooth`): the cost constraint (PPO-Lagrangian).  Beside the bootstrap values constraint.begin_section(rollouts, dones)
    values the costs the storages recorded (insert_batch(costs=)), scans them with the reward scan's masks and cuts and steps the
    multiplier of each head; after the storages are finished as they are without it, constraint.mix(rollouts) rewrites every
    storage's `advantages` to (A_r - lambda (A_c - mean A_c)) / (1 + lambda) — nothing is stored for a head whose lambda is 0 —
    and behind the PPO steps constraint.update() runs the cost critics' steps.  The loss launches, the update's graphs and the
    sampler are untouched.  `stats` gains "constraint" (J, budget, lambda, costly_share, mean_abs_cost_term, mean_abs_reward_term,
    loss_before, loss_after, explained_variance as (steer, throttle) pairs, steps, lambda_updates; one more small device-to-host
    copy)."""
    _check_constraint(constraint, reuse, sil, shared_grad_buffers, True, demo, suggest, smooth)
    _check_actmask(actmask, demo, suggest, reuse, sil, smooth)
    _check_smooth(smooth, demo, suggest, reuse, sil)
    _check_curiosity(curiosity, reward_scaler, reuse, sil, shared_grad_buffers)
    if smooth is not None:                           # (the cursor check comes before any launch of the section)
        smooth.begin_section(rollouts, train_cfg["ppo_epoch"] * _steps_per_epoch(rollouts[0][0]) if stats is not None else 0)
    if suggest is not None and demo is not None:
        raise ValueError("suggest excludes demo (a row carries one kind array)")
    _check_sil(sil, demo, suggest, reuse)
    _check_scaler(reward_scaler, shared_grad_buffers, train_cfg)
    tkl = _target_kl(train_cfg, shared_grad_buffers)
    cons = _consensus_on(train_cfg, shared_grad_buffers)
    lr = _section_hyper(agent, train_cfg, shared_grad_buffers, True, optimizer)
    use_adv_norm = train_cfg["use_adv_norm"]
    nv = agent.get_values([(s.get_last(as_tensor=True), t.get_last(as_tensor=True)) for s, t in rollouts], dones)
    sec = None
    if stats is not None or tkl is not None:
        sec = _SectionStats(agent, train_cfg["ppo_epoch"] * _steps_per_epoch(rollouts[0][0]), 2 * len(rollouts),
                            consensus_world=shared_grad_buffers.dist_world() if cons else 0,
                            demo=demo is not None and stats is not None)
    if curiosity is not None:
        curiosity.begin_section(rollouts)
    if constraint is not None:
        constraint.begin_section(rollouts, dones)
    flat = RolloutStorage.finish_rollouts([x for pair in rollouts for x in pair], [v.detach() for pair in nv for v in pair],
                                          normalise=use_adv_norm, reward_scaler=reward_scaler,
                                          explained_variance=None if sec is None else sec.ev,
                                          **_scaler_consensus(cons, reward_scaler, shared_grad_buffers),
                                          **({} if curiosity is None else dict(intrinsic=curiosity)))
    advs = [(flat[2 * i], flat[2 * i + 1]) for i in range(len(rollouts))]
    if constraint is not None:
        constraint.mix(rollouts)
    if reuse is not None:
        reuse.refresh(use_adv_norm, reward_scaler)
    if sec is not None:
        agent.learner.set_update_modes(stats=True, target_kl=tkl, consensus=cons)
    dev_losses = []
    sug_prev = am_prev = None
    try:
        sug_prev = _suggest_begin(agent, suggest, [x for pair in rollouts for x in pair], stats,
                                  train_cfg["ppo_epoch"] * _steps_per_epoch(rollouts[0][0]))
        am_prev = _actmask_begin(agent, actmask, stats, train_cfg["ppo_epoch"] * _steps_per_epoch(rollouts[0][0]))
        if sil is not None:
            sil.begin_section(train_cfg["ppo_epoch"] * _steps_per_epoch(rollouts[0][0]) if stats is not None else 0)
        for epoch in range(train_cfg["ppo_epoch"]):
            idx = [(s.sample_indices(), t.sample_indices()) for s, t in rollouts]
            for j in range(len(idx[0][0])):
                batches = [(s, idx[i][0][j], advs[i][0], t, idx[i][1][j], advs[i][1]) for i, (s, t) in enumerate(rollouts)]
                smooth_kw = _smooth_kw(smooth, batches)
                if reuse is not None:
                    batches += reuse.entries(episode, epoch, j, batches[0][1].numel())
                dev_losses.append(agent.update_policy_from_storages(
                    batches, sync=False, stats_row=None if sec is None else sec.next_row(),
                    **_demo_kw(demo, batches[0][1].numel(), episode, len(dev_losses), sec),
                    **_sil_kw(sil, batches[0][1].numel(), episode, epoch, j), **smooth_kw,
                    **({} if actmask is None else dict(actmask=actmask))))
                if suggest is not None:
                    suggest.collect(agent.learner)
                if sil is not None:
                    sil.after_step(len(batches) * batches[0][1].numel())
                shared_grad_buffers.add_gradient(agent.model_dict)
                chief_step(shared_grad_buffers, optimizer, train_cfg["max_grad_norm"], lr=lr, zero_grads=False)
    finally:
        if sec is not None:
            agent.learner.set_update_modes()
        _loss_end(agent, sug_prev, am_prev)
    _curiosity_end(stats, curiosity)
    _constraint_end(stats, constraint)
    losses = torch.stack(dev_losses)
    if sec is not None and not losses_on_device:
        host = sec.finish(stats, tkl is not None, losses=losses)
        _scale_stats(stats, reward_scaler)
        _reuse_stats(stats, reuse)
        _suggest_stats(stats, suggest)
        _actmask_stats(stats, actmask)
        _sil_stats(stats, sil)
        _smooth_stats(stats, smooth)
        _curiosity_stats(stats, curiosity)
        _constraint_stats(stats, constraint)
        _average_stats(stats, agent)
        return tuple(list(c) for c in zip(*host.tolist()))
    if sec is not None:
        sec.finish(stats, tkl is not None)
        _scale_stats(stats, reward_scaler)
        _reuse_stats(stats, reuse)
        _suggest_stats(stats, suggest)
        _actmask_stats(stats, actmask)
        _sil_stats(stats, sil)
        _smooth_stats(stats, smooth)
        _curiosity_stats(stats, curiosity)
        _constraint_stats(stats, constraint)
        _average_stats(stats, agent)
    if losses_on_device:
        return losses
    vl, pl, el = [], [], []
    for v, p, e in losses.tolist():
        vl.append(v); pl.append(p); el.append(e)
    return vl, pl, el


def train_vec(rank, train_cfg, agent_cfg, env_cfg, rollout_cfg, num_envs, env_cls=None, logger=None,
              shared_grad_buffers=None, optimizer=None, callback=None):
    """`train()` for `num_envs` environments driven from ONE process with one agent: the vectorised-env form of the
    reference's `num_processes` workers on a GPU.  Environment i is worker w = rank * num_envs + i: it gets
    env_cfg[k][w] for the per-worker keys (port, routes, scenarios, town) and rank w, as train() does for its rank.
    Every env step is one `act_batch` over all environments, N `env.step` calls, one `RolloutStorage.insert_batch` into
    the 2N storages and a reset of the finished environments; every episode ends in `learner_section_multi` (see there
    for the sampler order).  Logging and snapshots as in train() (rank 0).
    `callback(event, **state)` (optional, for tests and tools): "start" before the first step, "rollout" after each
    rollout (before its learner section; episode, dones), "update" after each learner section, its log line and its
    snapshot (episode, losses; saving a snapshot builds nn.Modules, which draws from the global generator); every event
    also passes agent, envs, rollouts and reward_scaler.
    train_cfg["reward_scaling"] (None / absent, True, or {"clip", "epsilon"}; single rank only): return-based reward
    scaling through one ReturnScaler kept as `agent.reward_scaler`.  An environment that reports info["time_limit"] (a
    bool, or a (steer, throttle) pair) marks the row as cut by a step budget: see RolloutStorage.finish_rollouts.
    train_cfg["checkpoint_interval"] (absent / None / 0: off; single rank only): after every interval-th episode (its
    learner section, log line and snapshot) the training state is captured (cadre_amd.checkpoint.capture: one launch on
    the compute stream, no host sync) and written to <work_dir>/checkpoints/ckpt_<episode>.pt just before the next capture
    or before the loop returns; the callback then gets "checkpoint" (episode, path).  train_cfg["resume_from"] (a path):
    after agent, storages, scaler and environments are built, the checkpoint is restored and the loop continues at its
    episode + 1 (schedules see that episode).  Environment state is not part of a checkpoint: the environments are the
    caller's and restart through reset().  With both keys absent nothing of this runs.
    train_cfg["aux_phase"] (absent / None: nothing runs, is allocated or drawn; single rank only): the PPG auxiliary phase
    (cadre_amd.phasic) — after every learner section its storages are appended to an AuxBuffer, and after every interval-th
    episode, before the log line, snapshot and checkpoint, aux_phase runs over the buffer's rows with the section's optimiser
    settings; checkpoint_interval must be a multiple of the interval."""
    if env_cls is None:
        from env_wrapper import EnvWrapper as env_cls        # needs the CARLA stack (reference env_wrapper.py)
    if logger is None:
        logger = _default_logger()
    if num_envs < 1:
        raise ValueError("train_vec: num_envs=%r" % (num_envs,))
    envs = []
    for i in range(num_envs):
        w = rank * num_envs + i
        cfg = type(env_cfg)(env_cfg)
        cfg["rank"] = w
        for k in ("port", "routes", "scenarios", "town"):
            cfg[k] = env_cfg[k][w]
        cfg["seq_length"] = rollout_cfg.seq_length
        envs.append(env_cls(cfg))
    model_dir = os.path.join(envs[0].work_dir, "models")
    check_exist(model_dir)
    num_steps = rollout_cfg.num_steps
    hidden_size, _ = get_vae_output(agent_cfg.model_cfg)
    agent_cfg.rank = rank
    agent = CadreAgent(**agent_cfg)
    device = torch.device("cuda:" + str(agent_cfg.model_cfg.device_num))
    rollout_cfg.hidden_size = hidden_size
    rollouts = []
    for _ in range(num_envs):
        pair = (RolloutStorage(**rollout_cfg), RolloutStorage(**rollout_cfg))
        for s in pair:
            s.to(device)
        rollouts.append(pair)
    if shared_grad_buffers is None:              # single-process use: the agent's own arena is the shared one
        from .models import Shared_grad_buffers
        shared_grad_buffers = Shared_grad_buffers(agent.model_dict, device)
    rs = _reward_scaling(train_cfg, shared_grad_buffers)
    agent.reward_scaler = None if rs is None else ReturnScaler(num_envs, rollout_cfg.gamma, device=device, **rs)
    ck_interval, ck_resume = _checkpointing(train_cfg, shared_grad_buffers)
    # (refusals first: before a checkpoint is read or anything else is built)
    cur = agent.curiosity = curiosity(agent, train_cfg, num_envs, shared_grad_buffers, True, ck_interval, ck_resume)
    con = agent.constraint = cost_constraint(agent, train_cfg, num_envs, shared_grad_buffers, True, ck_interval, ck_resume)
    avg_cfg = weight_average_config(train_cfg, shared_grad_buffers, True, agent)
    ck, first_episode, avg = None, 0, None
    if ck_interval is not None or ck_resume is not None:
        ck = _Checkpointer(envs[0].work_dir, ck_interval, agent, rollouts, callback)
        if ck_resume is not None:                # (the environments are the caller's: they restart through reset())
            avg = weight_average(agent, avg_cfg)      # (before the restore, which fills it; no warm start runs)
            first_episode = ck.resume(ck_resume)
    suggest = suggestions(agent, train_cfg, True, ck_interval, ck_resume)      # (refusals first: before anything is loaded)
    actmask = action_masks(agent, train_cfg, True, ck_interval, ck_resume)
    demo = demo_mixer(agent, train_cfg, rollout_cfg, rank)          # (before the warm start, which shares its DemoSet)
    _pretrain(agent, train_cfg, rollout_cfg, shared_grad_buffers, rank, logger, ck_resume)
    if ck_resume is None:                        # (behind the warm start: the average starts from its result)
        avg = weight_average(agent, avg_cfg)
    aux = _aux_runner(agent, train_cfg, shared_grad_buffers, rank, True, ck_interval, first_episode)
    reuse = _reuse_runner(agent, train_cfg, shared_grad_buffers, rank, True, ck_interval, ck_resume)
    sil = self_imitation(agent, train_cfg, shared_grad_buffers, rank, True, True, ck_interval, ck_resume)
    smooth = smoothness(agent, train_cfg)
    obs = [env.reset() for env in envs]
    dones = [False] * num_envs
    infos = [None] * num_envs                    # (the action-mask rule sees the last step's info; None after a reset)
    log_stats = bool(_get(train_cfg, "log_stats", False))
    state = lambda: dict(agent=agent, envs=envs, rollouts=rollouts, reward_scaler=agent.reward_scaler)
    if callback is not None:
        callback("start", **state())
    for episode in range(first_episode, train_cfg.max_episode):
        _rewind(smooth, rollouts)
        for _ in range(num_steps):
            commands = [o["command"] for o in obs]
            words = None if actmask is None else [actmask.words(o, f) for o, f in zip(obs, infos)]
            outs = agent.act_batch(obs, **({} if words is None else dict(allowed=words)))      # (key absent: today's call)
            rewards, masks, tls, evs, costs = [], [], [], [], []
            for i, (env, out) in enumerate(zip(envs, outs)):
                obs[i], reward, dones[i], info = env.step(agent.convert_action(out[1]))
                infos[i] = info
                ad = info["action_done"]
                rewards.append(reward)
                masks.append([0.0 if ad[0] else 1.0, 0.0 if ad[1] else 1.0])
                tls.append(info.get("time_limit"))
                if suggest is not None:
                    evs.append(suggest.codes(info))
                if con is not None:
                    costs.append(info.get("cost", 0.0))
            RolloutStorage.insert_batch(rollouts, outs, rewards, masks, commands,
                                        time_limits=None if all(f is None for f in tls) else
                                        [_time_limit_pair(False if f is None else f) for f in tls],
                                        **({} if suggest is None else dict(events=evs)),
                                        **({} if words is None else dict(allowed=outs.allowed)),
                                        **({} if con is None else dict(costs=costs)))
            for i, env in enumerate(envs):
                if dones[i]:
                    obs[i], infos[i] = env.reset(), None
        if callback is not None:
            callback("rollout", episode=episode, dones=list(dones), **state())
        stats = {} if log_stats else None
        apply_schedules(agent, train_cfg, episode)
        apply_demo_mix(agent, demo, episode, train_cfg.max_episode)
        apply_suggest(agent, suggest, episode, train_cfg.max_episode)
        apply_sil(agent, sil, episode, train_cfg.max_episode)
        apply_smooth(agent, smooth, episode, train_cfg.max_episode)
        apply_curiosity(cur, episode, train_cfg.max_episode)
        vl, pl, el = learner_section_multi(agent, rollouts, dones, train_cfg, shared_grad_buffers, optimizer=optimizer,
                                           stats=stats, reward_scaler=agent.reward_scaler, demo=demo, episode=episode,
                                           **({} if reuse is None else dict(reuse=reuse.window_for(rollouts))),
                                           **({} if suggest is None else dict(suggest=suggest)),
                                           **({} if actmask is None else dict(actmask=actmask)),
                                           **({} if sil is None else dict(sil=sil.buffer_for(rollouts))),
                                           **({} if smooth is None else dict(smooth=smooth)),
                                           **({} if cur is None else dict(curiosity=cur)),
                                           **({} if con is None else dict(constraint=con)))
        log_now = episode % train_cfg.log_interval == 0 and rank == 0 and logger is not None
        # (the auxiliary phase: before the log line, the snapshot and the checkpoint, which then see its result)
        aux_records = _aux_after_section(aux, agent, train_cfg, episode, rollouts, shared_grad_buffers, optimizer,
                                         logger if log_now else None)
        if reuse is not None:                    # (after the PPG buffer took its copy: the two are independent)
            reuse.after_section(rollouts, dones)
        if sil is not None:                      # (the section's rollouts become replayable from the next section on)
            sil.after_section(rollouts, dones, agent.reward_scaler)
        if log_now:
            logger.log("Episode: {}, value loss: {:.4f}, policy loss: {:.4f}, entropy loss: {:.4f}".format(
                episode, np.mean(vl), np.mean(pl), np.mean(el)))
            if log_stats:
                logger.log(stats_line(episode, stats))
                if demo is not None:
                    logger.log(demo_stats_line(episode, stats))
                if aux_records:
                    logger.log(aux_stats_line(episode, aux_records))
        if episode % train_cfg.save_interval == 0 and rank == 0:
            agent.save_snapshot(os.path.join(model_dir, "ppo_model_{}.pt".format(episode)))
            _average_snapshot(agent, avg, model_dir, episode)
        if ck is not None:                       # (after the snapshot: building its nn.Modules draws from the generator)
            ck.after_episode(episode)
        if callback is not None:
            callback("update", episode=episode, losses=(vl, pl, el), **state())
    if ck is not None:
        ck.flush()
    print("process {} finished ({} environments).".format(rank, num_envs))
    return agent
