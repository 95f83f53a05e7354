"""Weight averaging on the device: an exponential moving average (Polyak average) of the parameter arena that follows every
optimiser step, the swap that lets the agent act and be saved with it, and the weight average ("soup") of several snapshots.

PPO's last iterate is a noisy one.  The trainer-side answer — as in PPG, Stable-Baselines-style trainers and every modern
supervised trainer — is to hand out an average of the iterates instead; the reference's own answer is an ensemble of 6 - 8
snapshots at evaluation time (eval.py, EnsembleEvaluator), which costs M LSTM + MLP chains per environment step.  Three uses:

    train_cfg["weight_average"] = {"decay": 0.999}          # train() / train_vec(): the average follows every step,
                                                            # ppo_model_<episode>_avg.pt beside every snapshot
    avg = WeightAverage(agent, decay=0.999)                  # by hand
    agent.learner.set_weight_average(avg)                    # clip_adam() now issues cadre_ema_update in its captured graph
    with agent.averaged_weights():                           # one cadre_arena_swap in, one out
        agent.act_batch(obs_list, deterministic=True)
    agent.save_snapshot(path, weights="average")

    soup(["ppo_model_40.pt", "ppo_model_50.pt", "ppo_model_60.pt"], into=agent)      # one cadre_arena_mean launch

The rule of an update (cadre_ema_update, csrc/average.hip): d = decay, with warm-up d = min(decay, (1 + n) / (10 + n)) after n
applied updates; e <- e + (1 - d) (p - e) in the lerp form, so an unchanged parameter leaves its average bit for bit.  The
update reads the same stop flag as the gated optimiser step: a step the target_kl gate skipped is skipped here too and
counted.  The decay lives in the module's device state block: set_decay is a small copy, no launch or graph depends on the
value.

Left out on purpose: a form fused into the clip + Adam kernels (it would save one read of the parameters, 4 of 12 bytes per
element, and add a twin to each optimiser entry point), averages of the Adam moments, acting from the average during
rollouts (they stay on-policy), averages of the curiosity and cost towers (the entry point takes any segment table; nothing
wires them), several ranks, tuned defaults."""
import contextlib
import math
import os

from .phasic import _is_number

AVERAGE_KEYS = ("decay", "warmup", "snapshot")
DEFAULTS = dict(warmup=True, snapshot=True)
LAYOUT_FIELDS = ("D", "C", "n_out", "hid", "ordinal_rank")
WARMUP_NUM, WARMUP_DEN = 1.0, 10.0


def _check_decay(decay, who):
    if not _is_number(decay) or not 0.0 < float(decay) < 1.0:
        raise ValueError("%s: decay must be a number in the open interval (0, 1) (got %r)" % (who, decay))
    return float(decay)


def average_config(train_cfg_value):
    """train_cfg["weight_average"]: absent / None -> None (nothing is built, launched or changed); else a dict {"decay"
    (required: a number in (0, 1)), "warmup" (True: the decay of update n is min(decay, (1 + n) / (10 + n)), so the initial
    copy fades fast), "snapshot" (True: every save_interval snapshot is followed by ppo_model_<episode>_avg.pt)} -> the dict
    with defaults.  The defaults are untuned."""
    cfg = train_cfg_value
    if cfg is None:
        return None
    if not isinstance(cfg, dict):
        raise ValueError("train_cfg.weight_average: expected None or a dict (got %r)" % (cfg,))
    unknown = sorted(set(cfg) - set(AVERAGE_KEYS))
    if unknown or "decay" not in cfg:
        raise ValueError("train_cfg.weight_average: needs decay; known keys %r (unknown: %r)" % (AVERAGE_KEYS, unknown))
    out = dict(DEFAULTS, **cfg)
    out["decay"] = _check_decay(out["decay"], "train_cfg.weight_average")
    for key in ("warmup", "snapshot"):
        if not isinstance(out[key], bool):
            raise ValueError("train_cfg.weight_average: %s must be True or False (got %r)" % (key, out[key]))
    return out


def average_refusals(shared_grad_buffers=None, in_process_chief=True):
    """What train_cfg["weight_average"] is refused with, each ValueError naming the key, before anything is allocated: several
    ranks (every rank would keep its own average of the same parameters; not built), a chief in another process (the update
    rides behind this process's optimiser step) and the sharded optimiser (it steps a shard per rank and has no captured
    graph to ride in).  Nothing else: the module only reads the parameters behind a step."""
    world = shared_grad_buffers.dist_world() if shared_grad_buffers is not None else 0
    if world > 1:
        raise ValueError("train_cfg.weight_average needs a single rank (world size %d): the multi-rank average is not built" % world)
    if not in_process_chief:
        raise ValueError("train_cfg.weight_average needs the in-process chief: the update follows this process's optimiser step")
    mode = getattr(shared_grad_buffers, "exchange_mode", None)
    if mode is not None and world and mode() == "sharded":
        raise ValueError("train_cfg.weight_average excludes the sharded optimiser (CADRE_GRAD_EXCHANGE=sharded): it steps one "
                         "shard of the arena per rank")


def warmup_decay(decay, n, warmup=True):
    """The decay update number n (0-based: n updates were applied before it) uses, in double as the kernel forms it."""
    decay = float(decay)
    return min(decay, (WARMUP_NUM + float(n)) / (WARMUP_DEN + float(n))) if warmup else decay


class WeightAverage(object):
    """The exponential moving average of an arena's parameters.  agent_or_arena: a CadreAgent or its PPOArena.  Owns `ema`
    (float32 [arena.total], a copy of arena.params at construction), the float64 state block (hip.EMA_*: decay, warm-up flag,
    updates applied, the decay the last one used, updates skipped, then the per-model squared distance between parameters and
    average after the last applied update) and the scratch `work` of cadre_ema_update.  `decay` and `warmup` stay the
    CONFIGURED settings — what a checkpoint's meta records and restore compares; set_decay moves the block's value only, which
    summary()["decay"] reads and a checkpoint carries in `ema_state`."""

    def __init__(self, agent_or_arena, decay=0.999, warmup=True):
        import torch
        from . import hip
        decay = _check_decay(decay, "WeightAverage")
        if not isinstance(warmup, bool):
            raise ValueError("WeightAverage: warmup must be True or False (got %r)" % (warmup,))
        arena = getattr(agent_or_arena, "arena", agent_or_arena)
        self.arena, self.decay, self.warmup = arena, decay, warmup
        self.device = arena.params.device
        self.n_models = int(arena.seg_off.numel()) - 1
        self.names = list(arena.model_names())
        self._offs = [int(v) for v in arena.seg_off.tolist()]
        self.ema = arena.params.clone()
        state = torch.zeros(hip.EMA_HEAD + self.n_models, dtype=torch.float64)
        state[hip.EMA_DECAY] = decay
        state[hip.EMA_WARMUP] = 1.0 if warmup else 0.0
        self.state = state.to(self.device)
        self.work = torch.zeros(hip.EMA_WORK_HEAD + self.n_models * hip.EMA_GRID, dtype=torch.float64, device=self.device)
        self._decay_set = decay
        self.snapshot = True        # (a training loop's setting: average_runner)

    def update(self, stop=None):
        """cadre_ema_update on the current stream (three launches, capturable).  stop: None, or the device int32 flag of the
        KL gate — while it is set the update only counts itself as skipped."""
        from . import hip
        a = self.arena
        hip.check(hip.lib().cadre_ema_update(hip.ptr(a.params), hip.ptr(self.ema), hip.ptr(a.seg_off), self.n_models,
                                             hip.ptr(self.state), hip.ptr(self.work), hip.ptr(stop), hip.stream()),
                  "cadre_ema_update")

    def set_decay(self, d):
        """d into the state block (one small asynchronous copy; no launch depends on the value)."""
        from . import hip
        d = _check_decay(d, "WeightAverage.set_decay")
        if d != self._decay_set:
            self.state[hip.EMA_DECAY:hip.EMA_DECAY + 1].fill_(d)
            self._decay_set = d
        return d

    def reset(self):
        """The average becomes a copy of the parameters again and the counts start over (in place: captured graphs hold the
        addresses)."""
        from . import hip
        self.ema.copy_(self.arena.params)
        self.state[hip.EMA_COUNT:].zero_()

    def views(self, model_name):
        """Parameter-shaped views of one model's average (PPOArena.views on `ema`)."""
        return self.arena.views(self.ema, model_name)

    def _host(self):
        import torch
        o = self._offs
        norms = torch.stack([torch.linalg.vector_norm(self.ema[o[m]:o[m + 1]], dtype=torch.float64) for m in range(self.n_models)])
        return torch.cat([self.state, norms]).cpu().tolist()

    def distance(self):
        """{model name: (||p - ema||, the same relative to ||ema|| of the model)} after the last applied update.  One small
        device-to-host copy."""
        return self.summary()["distance"]

    def summary(self):
        """The "weight_average" entry of a section's `stats`: updates applied, updates skipped by the gate, the configured decay
        and the one the last applied update used, and the per-model distances.  One small device-to-host copy."""
        from . import hip
        h = self._host()
        d2, norms = h[hip.EMA_HEAD:hip.EMA_HEAD + self.n_models], h[hip.EMA_HEAD + self.n_models:]
        dist = {n: (math.sqrt(v), math.sqrt(v) / e if e > 0.0 else 0.0) for n, v, e in zip(self.names, d2, norms)}
        return dict(updates=int(h[hip.EMA_COUNT]), skipped=int(h[hip.EMA_SKIPPED]), decay=h[hip.EMA_DECAY],
                    decay_used=h[hip.EMA_D], distance=dist)

    # ------------------------------------------------------------------ plain-tensor state
    def state_dict(self):
        import torch
        return dict(ema=self.ema.clone(), state=self.state.clone(),
                    dims=torch.tensor([int(self.ema.numel()), self.n_models], dtype=torch.int64))

    def load_state_dict(self, sd):
        missing = sorted({"ema", "state", "dims"} - set(sd))
        if missing:
            raise ValueError("WeightAverage.load_state_dict: missing %r" % (missing,))
        if sd["dims"].tolist() != [int(self.ema.numel()), self.n_models]:
            raise ValueError("WeightAverage.load_state_dict: a state for (elements, models) = %r does not fit %r"
                             % (sd["dims"].tolist(), [int(self.ema.numel()), self.n_models]))
        for k, dst in (("ema", self.ema), ("state", self.state)):
            if tuple(sd[k].shape) != tuple(dst.shape):
                raise ValueError("WeightAverage.load_state_dict: %s has shape %r, expected %r" % (k, tuple(sd[k].shape), tuple(dst.shape)))
            dst.copy_(sd[k].to(dst.device, dst.dtype))
        self._decay_set = None


def average_stats_text(stats):
    """What stats_line appends for a section that ran with the weight average."""
    c = stats["weight_average"]
    if not c["distance"]:
        return ", average: no models"
    worst = max(c["distance"], key=lambda n: c["distance"][n][1])
    return (", average: {} updates ({} skipped), decay {:.6f}, max relative distance {:.4e} ({})").format(
        c["updates"], c["skipped"], c["decay_used"], c["distance"][worst][1], worst)


def average_runner(agent, train_cfg_value, **refusal_args):
    """The WeightAverage of a training loop, or None when the key is absent / None.  average_refusals(**refusal_args) first."""
    cfg = average_config(train_cfg_value)
    if cfg is None:
        return None
    average_refusals(**refusal_args)
    avg = WeightAverage(agent, decay=cfg["decay"], warmup=cfg["warmup"])
    avg.snapshot = cfg["snapshot"]
    return avg


# ----------------------------------------------------------------------------- swap
def drop_derived(arena, learner=None):
    """After the CONTENTS of arena.params moved behind the learner's back: PPOLearnerHIP.invalidate_parameter_caches (the
    packed recurrent weights are forgotten and arena.params._version moves by an in-place no-op, as in load_snapshot)."""
    if learner is not None:
        learner.invalidate_parameter_caches()
    else:                                   # (a bare arena: nothing is derived from it here, the version still moves)
        arena.params[:0].zero_()


def swap_in(arena, avg, learner=None):
    """One cadre_arena_swap: the average where the parameters live and back (captured graphs hold addresses, so the contents
    move, not the pointers)."""
    from . import hip
    hip.check(hip.lib().cadre_arena_swap(hip.ptr(arena.params), hip.ptr(avg.ema), int(arena.params.numel()), hip.stream()),
              "cadre_arena_swap")
    drop_derived(arena, learner)


@contextlib.contextmanager
def averaged_weights(agent):
    """CadreAgent.averaged_weights: see there."""
    from . import hip
    lrn = agent.learner
    avg = getattr(lrn, "_avg", None)
    if avg is None:
        raise hip.CadreHipError("averaged_weights: no weight average is set (learner.set_weight_average(WeightAverage(agent)))")
    if lrn._avg_swapped:
        raise hip.CadreHipError("averaged_weights: the average is already swapped in (no nested entry)")
    swap_in(agent.arena, avg, lrn)
    lrn._avg_swapped = True
    try:
        yield avg
    finally:
        lrn._avg_swapped = False
        swap_in(agent.arena, avg, lrn)


# ----------------------------------------------------------------------------- soup
def _layout_of(arena):
    rank = getattr(arena, "ordinal_rank", None)
    return dict(D=int(arena.D), C=int(arena.C), n_out=tuple(int(v) for v in arena.n_out), hid=int(arena.hid),
                ordinal_rank=None if rank is None else [None if r is None else [int(x) for x in r] for r in rank])


def _snapshot_layout(model_dict):
    """What a snapshot file says about the layout: D and hid from the first tower, n_out per head, C from the names.  The rank
    tables of ordinal heads are not in the file."""
    out, C = {}, 0
    for name, m in model_dict.items():
        head, kind, c = name.split("_")
        C = max(C, int(c) + 1)
        sd = m.state_dict()
        if kind == "lstm":
            out["D"] = int(sd["rnn.weight_hh"].shape[1])
        else:
            out["hid"], out["D"] = (int(v) for v in sd["control.linear.0.weight"].shape)
            out.setdefault("n_out", {})[head] = int(sd["control.linear.4.weight"].shape[0])
    out["C"] = C
    return out


def check_soup_weights(weights, K):
    """The weights of soup(): K finite numbers >= 0 that sum to 1 within 1e-12 (None: 1 / K each) -> a list of floats."""
    if not 1 <= K <= 64:
        raise ValueError("soup: needs 1 .. 64 sources (got %d)" % K)
    if weights is None:
        return [1.0 / K] * K
    w = list(weights)
    if len(w) != K or not all(_is_number(v) and math.isfinite(v) and v >= 0.0 for v in w):
        raise ValueError("soup: weights must be %d finite numbers >= 0 (got %r)" % (K, weights))
    w = [float(v) for v in w]
    if abs(math.fsum(w) - 1.0) > 1e-12:
        raise ValueError("soup: weights must sum to 1 within 1e-12 (got %r, sum %r)" % (w, math.fsum(w)))
    return w


def check_soup_layouts(layouts, mine):
    """Every source's layout against the destination's; ValueError naming the field."""
    for k, lay in enumerate(layouts):
        for f in LAYOUT_FIELDS:
            if f not in lay:
                continue
            want = mine[f]
            if f == "n_out" and isinstance(lay[f], dict):          # (a snapshot file: the heads it holds)
                want = {h: mine[f][i] for i, h in enumerate(("steer", "throttle")) if h in lay[f]}
            if lay[f] != want:
                raise ValueError("soup: layout mismatch in %s: source %d has %r, the destination %r" % (f, k, lay[f], want))


def soup(sources, weights=None, into=None):
    """The weight average of K sources of one layout — CadreAgents, PPOArenas or snapshot paths — written into
    `into`.arena.params (default: the first agent among the sources) by ONE cadre_arena_mean launch: out = sum_k weights[k]
    src_k, accumulated in double in source order.  weights: None (1 / K each), or K finite numbers >= 0 that sum to 1 within
    1e-12.  A snapshot file is unpacked into a flat buffer of the destination's layout first; a model the file does not hold
    (the reference never writes throttle_lstm) keeps the destination's values there.  The destination may be one of the
    sources.  A layout mismatch (D, C, n_out, hid, ordinal_rank) is a ValueError naming the field.  Returns `into`."""
    sources = list(sources)
    w = check_soup_weights(weights, len(sources))
    is_path = [isinstance(s, (str, os.PathLike)) for s in sources]
    if into is None:
        agents = [s for s, p in zip(sources, is_path) if not p and hasattr(s, "arena")]
        if not agents:
            raise ValueError("soup: into= is needed when no source is an agent")
        into = agents[0]
    dst = getattr(into, "arena", into)
    dst_learner = getattr(into, "learner", None) or getattr(dst, "_learner", None)       # (an agent's, or the one its agent left on the arena)
    if getattr(dst_learner, "_avg_swapped", False):
        from .hip import CadreHipError
        raise CadreHipError("soup inside averaged_weights(): the destination arena holds the average")
    mine = _layout_of(dst)
    import torch
    loaded = [torch.load(os.fspath(s), map_location="cpu", weights_only=False) if p else None for s, p in zip(sources, is_path)]
    layouts = [_snapshot_layout(ld) if p else _layout_of(getattr(s, "arena", s)) for s, ld, p in zip(sources, loaded, is_path)]
    check_soup_layouts(layouts, mine)
    from . import hip
    bufs = []
    for s, ld, p in zip(sources, loaded, is_path):
        if not p:
            bufs.append(getattr(s, "arena", s).params)
            continue
        buf = dst.params.clone()
        for name, m in ld.items():
            v = dst.views(buf, name)
            for k, t in m.state_dict().items():
                v[k].copy_(t.to(buf.device))
        bufs.append(buf)
    n = int(dst.params.numel())
    for k, b in enumerate(bufs):
        if b.device != dst.params.device or int(b.numel()) != n:
            raise ValueError("soup: source %d holds %d elements on %s, the destination %d on %s"
                             % (k, b.numel(), b.device, n, dst.params.device))
    table = torch.tensor([hip.ptr(b) for b in bufs], dtype=torch.int64).to(dst.params.device)
    wdev = torch.tensor(w, dtype=torch.float64).to(dst.params.device)
    hip.check(hip.lib().cadre_arena_mean(hip.ptr(table), hip.ptr(wdev), len(bufs), hip.ptr(dst.params), n, hip.stream()),
              "cadre_arena_mean")
    drop_derived(dst, dst_learner)
    return into
