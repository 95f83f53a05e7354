"""Cost constraints on the device: PPO-Lagrangian with one cost critic per head.

Ray et al. 2019 ("Benchmarking Safe Exploration in Deep Reinforcement Learning"), Stooke et al. 2020: beside the reward every env
step records a cost c >= 0 per head; the expected cost of the policy is held under a budget by a multiplier lambda >= 0 that rises
while the cost is above the budget and falls while it is below.  The multiplier enters the update through the ADVANTAGES only:

    con = CostConstraint(agent, n_envs, budget=(0.02, 0.05))
    RolloutStorage.insert_batch(rollouts, outs, rewards, masks, commands, costs=[info.get("cost", 0.0) ...])
    learner_section_multi(agent, rollouts, dones, ..., constraint=con)

begin_section() runs, per head, cadre_cost_forward over rows 0 .. T of the head's storages (`cost_values`, row T the bootstrap,
multiplied by 0 for an environment whose section ended done), then ONE cadre_gae_multi launch over the 2N records {costs,
cost_values, masks, cost_next, cost_returns, cost_adv, time_limits} (normalise off, no reward scaling: the scan, the masks and the
time-limit cuts of the reward advantages) and cadre_cost_lambda (the cost rate J of each head and the multiplier's step).  After
RolloutStorage.finish_rollouts has written the reward advantages as it does without the module, mix() runs cadre_lag_mix:

    advantages <- (A_r - lambda (A_c - mean A_c)) / (1 + lambda)          per storage, lambda of its head

and with (float)lambda == 0 it stores nothing, so a run whose multiplier stays 0 is bit for bit the run without the module.
update() runs behind the PPO steps: epochs x minibatches critic steps (per head cadre_cost_forward with the activations kept and
cadre_cost_backward on contiguous runs of the (storage, time) order, then the arena's cadre_clip_adam_graph on the module's own
flat buffer, one segment per head, with its own moments and step counter).  No loss kernel, no graph of the update and no
snapshot changes.

Deliberate departures from the published implementations:
  * The constraint is on the cost RATE J = mean c over the section's N T rows of a head, not on a per-episode sum: the two heads
    close episodes at different rows, and a rate needs no episode definition.  An episode budget is rate x horizon.
  * Everything is per head: cost, budget, multiplier, cost critic.
  * The cost advantages are centred per storage, not scaled.

The defaults are plain choices; none has been tuned for this task.
"""
import math

import numpy as np
import torch

from . import hip
from .curiosity import _orthogonal
from .phasic import _is_int, _is_number

CONSTRAINT_KEYS = ("budget", "lambda_init", "lr_lambda", "lambda_max", "gamma", "tau", "hidden", "lr", "epochs", "minibatches",
                   "max_norm", "seed")
DEFAULTS = dict(lambda_init=0.0, lr_lambda=0.05, lambda_max=100.0, gamma=None, tau=None, hidden=128, lr=1e-3, epochs=4,
                minibatches=4, max_norm=1e30, seed=0)
HEADS = ("steer", "throttle")


def cost_tower_offsets(D, H):
    """Offsets of W1 [D][H], b1 [H], W2 [H][H], b2 [H], W3 [H], b3 [1] in a cost tower's flat buffer, and its size."""
    o = [0, D * H, D * H + H, D * H + H + H * H, D * H + 2 * H + H * H, D * H + 3 * H + H * H]
    return o, o[5] + 1


def init_cost_tower(D, H, gen):
    """One cost tower's flat float32 buffer: orthogonal weights (gain sqrt 2 for the hidden layers, 1 for the last), zero biases,
    every matrix stored input-major."""
    offs, P = cost_tower_offsets(D, H)
    p = torch.zeros(P, dtype=torch.float32)
    for o, (n_out, n_in, gain) in zip(offs[0::2], ((H, D, math.sqrt(2.0)), (H, H, math.sqrt(2.0)), (1, H, 1.0))):
        p[o:o + n_in * n_out] = _orthogonal(n_out, n_in, gain, gen).t().contiguous().reshape(-1).float()
    return p


def _pair(v, what, ok):
    """A number -> (v, v); a pair -> the pair; every entry a number that `ok` accepts."""
    p = tuple(v) if isinstance(v, (tuple, list)) else (v, v)
    if len(p) != 2 or not all(_is_number(x) and math.isfinite(x) and ok(x) for x in p):
        raise ValueError("%s (got %r)" % (what, v))
    return (float(p[0]), float(p[1]))


def cost_pair(c):
    """info["cost"] -> the (steer, throttle) pair of finite costs >= 0: a number goes to both heads."""
    return _pair(c, "a cost is a finite number >= 0 or a (steer, throttle) pair of them", lambda x: x >= 0)


def cost_from_message(msg, table):
    """The reference environment's `error_message` of a step ("collision static", "vehicle blocked", "route deviation", ...; ""
    for a step without an infraction) -> the (steer, throttle) cost pair of the step from `table`, a dict the user gives:
    message -> a cost or a (steer, throttle) pair.  A key is matched exactly first, then as a prefix of the message (the longest
    matching key wins), so "collision" covers "collision static", "collision vehicles!" and "collision pedestrians!".  A message
    no key matches costs (0, 0).  No table is built in: which infraction is charged to which head is the user's statement."""
    if not isinstance(table, dict):
        raise ValueError("cost_from_message: the table must be a dict of message -> cost (got %r)" % (table,))
    msg = "" if msg is None else str(msg)
    key = msg if msg in table else None
    if key is None:
        hits = [k for k in table if isinstance(k, str) and k and msg.startswith(k)]
        key = max(hits, key=len) if hits else None
    return (0.0, 0.0) if key is None else cost_pair(table[key])


def constraint_config(train_cfg_value):
    """train_cfg["cost_constraint"]: absent / None -> None (every launch, tensor and bit is what it is without the key); else a
    dict {"budget" (required: the bound on the cost rate, a number >= 0 or a (steer, throttle) pair), "lambda_init" (0.0) and
    "lr_lambda" (0.05; both a number >= 0 or a pair), "lambda_max" (100.0, > 0), "gamma" / "tau" (None: the storages'; else in
    [0, 1]) of the cost scan, "hidden" (128: a multiple of 32 up to 256), "lr" (1e-3), "epochs" (4) x "minibatches" (4) critic
    steps per section, "max_norm" (1e30: never clips), "seed" (0)} -> the dict with defaults.  The defaults are untuned."""
    cfg = train_cfg_value
    if cfg is None:
        return None
    if not isinstance(cfg, dict):
        raise ValueError("train_cfg.cost_constraint: expected None or a dict (got %r)" % (cfg,))
    unknown = sorted(set(cfg) - set(CONSTRAINT_KEYS))
    if unknown or "budget" not in cfg:
        raise ValueError("train_cfg.cost_constraint: needs budget; known keys %r (unknown: %r)" % (CONSTRAINT_KEYS, unknown))
    out = dict(DEFAULTS, **cfg)
    for key in ("budget", "lambda_init", "lr_lambda"):
        out[key] = _pair(out[key], "train_cfg.cost_constraint: %s must be a finite number >= 0 or a (steer, throttle) pair of them" % key,
                         lambda x: x >= 0)

    def number(key, lo, hi, lo_open=False):
        v = out[key]
        if not _is_number(v) or not (lo < v if lo_open else lo <= v) or not v <= hi:
            raise ValueError("train_cfg.cost_constraint: %s must be a number in %s%r, %r] (got %r)"
                             % (key, "(" if lo_open else "[", lo, hi, v))
        out[key] = float(v)
    number("lambda_max", 0.0, 1e30, lo_open=True)
    number("lr", 0.0, 1.0, lo_open=True)
    number("max_norm", 0.0, 1e300, lo_open=True)
    for key in ("gamma", "tau"):
        if out[key] is not None:
            number(key, 0.0, 1.0)
    if max(out["lambda_init"]) > out["lambda_max"]:
        raise ValueError("train_cfg.cost_constraint: lambda_init %r lies above lambda_max %r" % (out["lambda_init"], out["lambda_max"]))
    v = out["hidden"]
    if not _is_int(v) or v < 32 or v > 256 or v % 32:
        raise ValueError("train_cfg.cost_constraint: hidden must be a multiple of 32 in 32 .. 256 (got %r)" % (v,))
    out["hidden"] = int(v)
    for key in ("epochs", "minibatches"):
        v = out[key]
        if not _is_int(v) or not 1 <= v <= 1024:
            raise ValueError("train_cfg.cost_constraint: %s must be an integer 1 .. 1024 (got %r)" % (key, v))
        out[key] = int(v)
    if not _is_int(out["seed"]) or not 0 <= out["seed"] < 2 ** 32:
        raise ValueError("train_cfg.cost_constraint: seed must be an integer 0 .. 2^32 - 1 (got %r)" % (out["seed"],))
    out["seed"] = int(out["seed"])
    return out


def constraint_refusals(sample_reuse=None, self_imitation=None, checkpoint_interval=None, resume_from=None, world=1, fused_gather=True,
                        demo_mix=None, suggest=None, smoothness=None, aux_phase=None):
    """What train_cfg["cost_constraint"] is refused with, each ValueError naming its key, before anything is allocated or
    launched.  sample_reuse and self_imitation replay rows that carry no costs; a checkpoint does not hold the module; with several
    ranks each rank would own a multiplier.  demo_mix, suggest, smoothness and aux_phase touch nothing the mix touches, but the
    combination has not been tested, so it is refused too."""
    if sample_reuse is not None:
        raise ValueError("train_cfg.cost_constraint excludes sample_reuse: the stale rows carry no costs")
    if self_imitation is not None:
        raise ValueError("train_cfg.cost_constraint excludes self_imitation: the replayed rows carry no costs")
    if checkpoint_interval:
        raise ValueError("train_cfg.cost_constraint excludes checkpoint_interval: the checkpoint format does not hold the module")
    if resume_from is not None:
        raise ValueError("train_cfg.cost_constraint excludes resume_from: the checkpoint format does not hold the module")
    if world > 1:
        raise ValueError("train_cfg.cost_constraint needs a single rank (world size %d): each rank would own a multiplier" % world)
    if not fused_gather:
        raise ValueError("train_cfg.cost_constraint needs fused_gather=True")
    for key, v in (("demo_mix", demo_mix), ("suggest", suggest), ("smoothness", smoothness), ("aux_phase", aux_phase)):
        if v is not None:
            raise ValueError("train_cfg.cost_constraint excludes %s: the combination is untested" % key)


def costs_of(storage):
    """`costs` float32 [T + 1] of a storage (the cost of each row; 0: none), allocated the first time it is asked for."""
    c = getattr(storage, "costs", None)
    if c is None or c.device != storage.rewards.device:
        c = storage.costs = torch.zeros(storage.num_steps + 1, dtype=torch.float32, device=storage.rewards.device)
    return c


class CostConstraint(object):
    """PPO-Lagrangian for `n_envs` environments of two heads each.  agent_or_dims: a CadreAgent (its arena gives the feature width
    and the device) or the feature width D itself, 1 .. 1024 (then `device`).  The other arguments are the keys of
    constraint_config.  Owns the two cost towers (`params`: one flat float32 buffer of two segments, cost_tower_offsets), their
    Adam moments and step counter, the float64 state block (hip.LAG_*: per head lambda, budget, lr_lambda, lambda_max, the last J,
    the share of costly rows, the multiplier steps) and the section's arrays (`cost_values`, `cost_returns` [2][N][T + 1],
    `cost_adv` [2][N][T]: head-major, storage k = 2 w + h is [h][w]).  train(False) freezes multiplier and critics."""

    def __init__(self, agent_or_dims, n_envs, budget=None, device=None, **keys):
        cfg = constraint_config(dict(keys, budget=budget) if budget is not None else dict(keys))
        if _is_int(agent_or_dims):
            D, dev = int(agent_or_dims), torch.device("cuda" if device is None else device)
        else:
            D, dev = int(agent_or_dims.arena.D), agent_or_dims.arena.device if device is None else torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        if not 1 <= D <= 1024:
            raise ValueError("CostConstraint: the feature width must be 1 .. 1024 (got %r)" % (D,))
        if not _is_int(n_envs) or not 1 <= n_envs <= 32767:
            raise ValueError("CostConstraint: n_envs must be an integer 1 .. 32767 (got %r)" % (n_envs,))
        self.cfg, self.D, self.H, self.n_envs, self.device = cfg, D, cfg["hidden"], int(n_envs), dev
        self.training = True
        gen = torch.Generator()
        gen.manual_seed(cfg["seed"])
        self.offsets, self.P = cost_tower_offsets(D, self.H)
        self.params = torch.cat([init_cost_tower(D, self.H, gen), init_cost_tower(D, self.H, gen)]).to(dev)
        self.grads = torch.zeros(2 * self.P, device=dev)
        self.exp_avg = torch.zeros(2 * self.P, device=dev)
        self.exp_avg_sq = torch.zeros(2 * self.P, device=dev)
        self.step_dev = torch.zeros(1, dtype=torch.int32, device=dev)
        self._seg_off = torch.tensor([0, self.P, 2 * self.P], dtype=torch.int64).to(dev)
        self._norms2 = torch.zeros(4, dtype=torch.float64, device=dev)
        state = torch.zeros(2 * hip.LAG_STRIDE, dtype=torch.float64)
        for h in (0, 1):
            b = h * hip.LAG_STRIDE
            state[b + hip.LAG_LAMBDA], state[b + hip.LAG_BUDGET] = cfg["lambda_init"][h], cfg["budget"][h]
            state[b + hip.LAG_LR], state[b + hip.LAG_MAX] = cfg["lr_lambda"][h], cfg["lambda_max"]
        self.state = state.to(dev)
        self._tables = {}
        self._section = None        # (obs tables of the two heads, N, T, S, ldo) of the last begin_section
        self.cost_values = self.cost_returns = self.cost_adv = self.cost_next = None
        self._diag = None           # float64 [2N][2] of the last mix
        self._ws = None
        self._loss = None           # float32 [steps][2][2] of the last update(): loss and rows of every step, per head
        self._loss_spare = torch.zeros(2, 2, device=dev)
        self._after = None
        self._steps = 0
        self._rows = None
        self._mixed = False

    def train(self, mode=True):
        self.training = bool(mode)
        return self

    def tower(self, h):
        return self.params[h * self.P:(h + 1) * self.P]

    def _set(self, field, v, what, hi=float("inf")):
        p = _pair(v, "CostConstraint: %s must be a finite number in [0, %r] or a (steer, throttle) pair of them" % (what, hi),
                  lambda x: 0 <= x <= hi)
        self.state[field::hip.LAG_STRIDE] = torch.tensor(p, dtype=torch.float64).to(self.device)
        return p

    def set_budget(self, budget):
        """The budget of the cost rate into the state block (a number for both heads or a pair)."""
        return self._set(hip.LAG_BUDGET, budget, "the budget")

    def set_lambda(self, lam):
        """The multiplier into the state block (a number for both heads or a pair), within [0, lambda_max]."""
        return self._set(hip.LAG_LAMBDA, lam, "lambda", self.cfg["lambda_max"])

    def lambdas(self):
        return self.state[hip.LAG_LAMBDA::hip.LAG_STRIDE]

    # ------------------------------------------------------------------ the section's chain
    def _table(self, key, rows):
        t = self._tables.get(key)
        if t is None:
            if len(self._tables) > 16:
                self._tables.clear()
            t = self._tables[key] = torch.tensor(rows, dtype=torch.int64).to(self.device)
        return t

    def _check(self, rollouts):
        if len(rollouts) != self.n_envs:
            raise ValueError("CostConstraint: built for %d environments, the section has %d" % (self.n_envs, len(rollouts)))
        flat = [s for pair in rollouts for s in pair]
        s0 = flat[0]
        if any(getattr(s, "_win", None) is not None for s in flat):
            raise ValueError("CostConstraint: a frame-table storage keeps no window rows to read")
        geo = (s0.num_steps, s0.seq_length, s0._ldo, s0.z_dims, s0._obs.device, s0.gamma, s0.tau)
        if any((s.num_steps, s.seq_length, s._ldo, s.z_dims, s._obs.device, s.gamma, s.tau) != geo for s in flat):
            raise ValueError("CostConstraint: every storage needs the same geometry, gamma, tau and device")
        if s0.z_dims != self.D or s0._obs.device != self.state.device:
            raise ValueError("CostConstraint: built for %d features on %s, the storages hold %d on %s"
                             % (self.D, self.state.device, s0.z_dims, s0._obs.device))
        return flat, s0

    def begin_section(self, rollouts, dones=None):
        """rollouts = [(steer_storage, throttle_storage), ...] of the section, dones[i] = environment i's last `done` (default:
        none): the two critic launches, the bootstrap, the cost scan and the multiplier — five launches.  Afterwards `cost_values`,
        `cost_returns`, `cost_adv` and the state block's J, share and lambda are the section's.  A storage that never saw a cost
        gets its `costs` here (all zeros)."""
        flat, s0 = self._check(rollouts)
        N, T, S, ldo = self.n_envs, s0.num_steps, s0.seq_length, s0._ldo
        if dones is not None and len(dones) != N:
            raise ValueError("CostConstraint: %d environments, %d done flags" % (N, len(dones)))
        if self.cost_values is None or tuple(self.cost_values.shape) != (2, N, T + 1):
            z = lambda *s: torch.zeros(*s, device=self.device)
            self.cost_values, self.cost_returns, self.cost_adv, self.cost_next = z(2, N, T + 1), z(2, N, T + 1), z(2, N, T), z(2, N)
            self._diag = torch.zeros(2 * N, 2, dtype=torch.float64, device=self.device)
        otabs = []
        for h in (0, 1):
            obs = tuple(hip.ptr(pair[h]._obs) for pair in rollouts)
            otabs.append(self._table(("obs", h) + obs, list(obs)))
        self._section = (otabs, N, T, S, ldo)
        self._rows = flat
        for h in (0, 1):
            self._forward(h, T + 1, 0, N * (T + 1), self.cost_values[h], None)
        keep = tuple(0.0 if d else 1.0 for d in (dones if dones is not None else [False] * N))
        torch.mul(self.cost_values[:, :, T], self._keep(keep), out=self.cost_next)
        flags = any(s._tl_used for s in flat)
        E = 4                                                # bytes of a float
        rows = []
        for k, s in enumerate(flat):
            w, h = k >> 1, k & 1
            rows.append([hip.ptr(costs_of(s)), hip.ptr(self.cost_values) + E * (h * N + w) * (T + 1), hip.ptr(s.masks),
                         hip.ptr(self.cost_next) + E * (h * N + w), hip.ptr(self.cost_returns) + E * (h * N + w) * (T + 1),
                         hip.ptr(self.cost_adv) + E * (h * N + w) * T, hip.ptr(s.time_limits) if flags else 0])
        gtab = self._table(("gae",) + tuple(p for r in rows for p in r), rows)
        gamma = s0.gamma if self.cfg["gamma"] is None else self.cfg["gamma"]
        tau = s0.tau if self.cfg["tau"] is None else self.cfg["tau"]
        L = hip.lib()
        hip.check(L.cadre_gae_multi(hip.ptr(gtab), 2 * N, T, float(np.float32(gamma)), float(np.float32(gamma * tau)), 0, None, 0.0,
                                    hip.stream()), "cadre_gae_multi")
        cptrs = [r[0] for r in rows]
        ctab = self._table(("costs",) + tuple(cptrs), cptrs)
        hip.check(L.cadre_cost_lambda(hip.ptr(ctab), N, T, hip.ptr(self.state), 1 if self.training else 0, hip.stream()),
                  "cadre_cost_lambda")
        self._after, self._steps, self._mixed = None, 0, False
        return self.cost_adv

    def _keep(self, keep):
        t = self._tables.get(("keep",) + keep)
        if t is None:
            t = self._tables[("keep",) + keep] = torch.tensor(keep, dtype=torch.float32).to(self.device)
        return t

    def mix(self, rollouts):
        """After finish_rollouts wrote the reward advantages of the section begin_section opened: ONE cadre_lag_mix launch over the
        2N storages.  A head whose (float)lambda is 0 keeps every bit of its advantages."""
        if self._section is None:
            raise ValueError("CostConstraint.mix: no section is open (begin_section first)")
        flat, s0 = self._check(rollouts)
        if any(a is not b for a, b in zip(flat, self._rows)):
            raise ValueError("CostConstraint.mix: these are not the storages of the section begin_section opened")
        _otabs, N, T, _S, _ldo = self._section
        rows = [[hip.ptr(self.cost_adv) + 4 * ((k & 1) * N + (k >> 1)) * T, hip.ptr(s.advantages)] for k, s in enumerate(flat)]
        mtab = self._table(("mix",) + tuple(p for r in rows for p in r), rows)
        hip.check(hip.lib().cadre_lag_mix(hip.ptr(mtab), 2 * N, T, hip.ptr(self.state), hip.ptr(self._diag), hip.stream()),
                  "cadre_lag_mix")
        self._mixed = True
        return [s.advantages for s in flat]

    def _forward(self, h, Tr, row0, rows, values, ws):
        otabs, N, _T, S, ldo = self._section
        hip.check(hip.lib().cadre_cost_forward(hip.ptr(otabs[h]), N, Tr, S, ldo, self.D, self.H, row0, rows, hip.ptr(self.tower(h)),
                                               hip.ptr(values), None if ws is None else hip.ptr(ws["h1"][h]),
                                               None if ws is None else hip.ptr(ws["h2"][h]), hip.stream()), "cadre_cost_forward")

    def _workspace(self, rows):
        ws = self._ws
        if ws is None or ws["rows"] < rows:
            z = lambda *s: torch.zeros(*s, device=self.device)
            ws = self._ws = dict(rows=rows, values=z(2, rows), h1=z(2, rows, self.H), h2=z(2, rows, self.H),
                                 scratch=z(2, rows * (2 * self.H + 1)))
        return ws

    def backward(self, h, row0, rows):
        """cadre_cost_backward of head h on the activations the last saving forward left: the head's segment of the gradient
        buffer and loss[2] (the loss, the rows)."""
        otabs, N, T, S, ldo = self._section
        ws = self._ws
        loss = self._loss[self._steps, h] if self._loss is not None and self._steps < self._loss.shape[0] else self._loss_spare[h]
        hip.check(hip.lib().cadre_cost_backward(hip.ptr(otabs[h]), N, T, S, ldo, self.D, self.H, row0, rows, hip.ptr(self.tower(h)),
                                                hip.ptr(ws["values"][h]), hip.ptr(ws["h1"][h]), hip.ptr(ws["h2"][h]),
                                                hip.ptr(self.cost_returns[h]), T + 1, hip.ptr(self.grads[h * self.P:]), hip.ptr(loss),
                                                hip.ptr(ws["scratch"][h]), hip.stream()), "cadre_cost_backward")
        return loss

    def adam(self):
        """The existing optimiser step (cadre_clip_adam_graph, two models: one segment per head) on the module's flat buffer."""
        hip.check(hip.lib().cadre_clip_adam_graph(hip.ptr(self.params), hip.ptr(self.grads), hip.ptr(self.exp_avg), hip.ptr(self.exp_avg_sq),
                                                  hip.ptr(self._seg_off), 2, hip.ptr(self._norms2), self.cfg["max_norm"], self.cfg["lr"], 0.9,
                                                  0.999, 1e-8, hip.ptr(self.step_dev), hip.stream()), "cadre_clip_adam_graph")

    def _chunks(self, rows):
        mb = self.cfg["minibatches"]
        return [(j * rows // mb, (j + 1) * rows // mb) for j in range(mb)]

    def steps_per_section(self, rows):
        return self.cfg["epochs"] * sum(1 for lo, hi in self._chunks(rows) if hi > lo)

    def step(self, lo, hi):
        """One critic step on rows lo .. hi - 1 of the (storage, time) order: per head forward (activations kept) -> backward, then
        one optimiser step over both segments."""
        ws = self._workspace(hi - lo)
        for h in (0, 1):
            self._forward(h, self._section[2], lo, hi - lo, ws["values"][h], ws)
            self.backward(h, lo, hi - lo)
        self.adam()
        self._steps += 1

    def update(self, stats=False):
        """The critic steps of the section begin_section opened: `epochs` passes over the section's N T rows in `minibatches`
        contiguous runs of the (storage, time) order.  Nothing is drawn from any generator; nothing runs when frozen.  stats: one
        more forward per head afterwards, from which summary() reports the loss after the steps."""
        if self._section is None:
            raise ValueError("CostConstraint.update: no section is open (begin_section first)")
        if not self.training:
            return 0
        _otabs, N, T, _S, _ldo = self._section
        R = N * T
        self._loss = torch.zeros(self.steps_per_section(R), 2, 2, device=self.device)
        self._steps = 0
        self._workspace(max(hi - lo for lo, hi in self._chunks(R)))      # (sized once, for the section's largest run of rows)
        for _epoch in range(self.cfg["epochs"]):
            for lo, hi in self._chunks(R):
                if hi > lo:
                    self.step(lo, hi)
        if stats:
            self._after = torch.zeros(2, N, T + 1, device=self.device)
            for h in (0, 1):
                self._forward(h, T + 1, 0, N * (T + 1), self._after[h], None)
        return self._steps

    # ------------------------------------------------------------------ what it reports
    def summary(self):
        """The "constraint" entry of a section's `stats`, every value a (steer, throttle) pair: J, budget, lambda (after the
        section's multiplier step), costly_share, mean_abs_cost_term = mean |lambda (A_c - m)| / (1 + lambda) against
        mean_abs_reward_term = mean |A_r| / (1 + lambda) (None before mix()), the critic's loss 0.5 mean (v - cost_returns)^2
        before and after the steps (after: None unless update(stats=True) ran) and its explained variance 1 - Var(R - V) / Var(R)
        (NaN where the cost returns are constant); "steps", "lambda_updates".  One small device-to-host copy."""
        if self._section is None:
            return dict(steps=0)
        T = self._section[2]
        st = self.state.view(2, hip.LAG_STRIDE)
        R, V = self.cost_returns[:, :, :T].double().reshape(2, -1), self.cost_values[:, :, :T].double().reshape(2, -1)
        nan = st.new_full((2,), float("nan"))
        after = nan if self._after is None else 0.5 * ((self._after[:, :, :T].double().reshape(2, -1) - R) ** 2).mean(1)
        diag = self._diag.view(self.n_envs, 2, 2).mean(0) if self._mixed else torch.stack([nan, nan], 1)
        vals = torch.stack([st[:, hip.LAG_J], st[:, hip.LAG_BUDGET], st[:, hip.LAG_LAMBDA], st[:, hip.LAG_SHARE], diag[:, 0], diag[:, 1],
                            0.5 * ((V - R) ** 2).mean(1), after, 1.0 - (R - V).var(1, unbiased=False) / R.var(1, unbiased=False),
                            st[:, hip.LAG_UPDATES]]).cpu().tolist()
        opt = lambda p: None if math.isnan(p[0]) else tuple(p)
        return dict(steps=self._steps, J=tuple(vals[0]), budget=tuple(vals[1]), **{"lambda": tuple(vals[2])}, costly_share=tuple(vals[3]),
                    mean_abs_cost_term=opt(vals[4]), mean_abs_reward_term=opt(vals[5]), loss_before=tuple(vals[6]),
                    loss_after=opt(vals[7]), explained_variance=tuple(vals[8]), lambda_updates=tuple(int(v) for v in vals[9]))

    # ------------------------------------------------------------------ plain-tensor state
    def state_dict(self):
        return dict(params=self.params.clone(), exp_avg=self.exp_avg.clone(), exp_avg_sq=self.exp_avg_sq.clone(),
                    step=self.step_dev.clone(), state=self.state.clone(),
                    dims=torch.tensor([self.D, self.H, self.n_envs], dtype=torch.int64))

    def load_state_dict(self, sd):
        missing = sorted({"params", "exp_avg", "exp_avg_sq", "step", "state", "dims"} - set(sd))
        if missing:
            raise ValueError("CostConstraint.load_state_dict: missing %r" % (missing,))
        if sd["dims"].tolist() != [self.D, self.H, self.n_envs]:
            raise ValueError("CostConstraint.load_state_dict: a state for (features, hidden, environments) = %r does not fit %r"
                             % (sd["dims"].tolist(), [self.D, self.H, self.n_envs]))
        for k, dst in (("params", self.params), ("exp_avg", self.exp_avg), ("exp_avg_sq", self.exp_avg_sq), ("step", self.step_dev),
                       ("state", self.state)):
            if tuple(sd[k].shape) != tuple(dst.shape):
                raise ValueError("CostConstraint.load_state_dict: %s has shape %r, expected %r" % (k, tuple(sd[k].shape), tuple(dst.shape)))
            dst.copy_(sd[k].to(dst.device, dst.dtype))


def constraint_stats_text(stats):
    """What stats_line appends for a section that ran with the cost constraint."""
    c = stats["constraint"]
    if "J" not in c:
        return ", constraint: no rows"
    pair = lambda p, f="{:.4e}": "n/a" if p is None else "/".join(f.format(v) for v in p)
    return (", constraint: J {} (budget {}), lambda {}, costly rows {}, |cost term| {} vs |reward term| {}, cost critic loss {} -> {} in {} "
            "steps, ev {}").format(pair(c["J"]), pair(c["budget"]), pair(c["lambda"], "{:.4f}"), pair(c["costly_share"], "{:.3f}"),
                                   pair(c["mean_abs_cost_term"]), pair(c["mean_abs_reward_term"]), pair(c["loss_before"]),
                                   pair(c["loss_after"]), c["steps"], pair(c["explained_variance"], "{:.3f}"))


def constraint_runner(agent, train_cfg_value, n_envs, **refusal_args):
    """The CostConstraint of a training loop, or None when the key is absent / None.  constraint_refusals(**refusal_args) first."""
    cfg = constraint_config(train_cfg_value)
    if cfg is None:
        return None
    constraint_refusals(**refusal_args)
    return CostConstraint(agent, n_envs, **cfg)
