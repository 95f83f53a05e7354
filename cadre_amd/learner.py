"""PPO inner loop on MI355X: the math of `CadreAgent.update_policy` / `act` / `get_value`
(reference ppo_agent/agent.py:114-237) and of `chief` (ppo_agent/chief.py:13-21) as batched
HIP launches over the parameter arena (cadre_amd/arena.py).

The reference runs 8 (head x command) LSTM+MLP nets one after another, each through 8
LSTMCell calls, and lets autograd replay ~1000 tiny kernels.  Here the 8 nets are ONE strided
batch: the input projections of all 8 time steps and 4 command nets of a head are one GEMM,
each recurrent step is ONE launch for all 8 nets (product + cell math, csrc/ppo_update.hip), the
MLP towers three launches, the backward pass is written out explicitly (same formulas autograd
would apply) and writes straight into the flat gradient arena.  No autograd graph, no
per-parameter tensors, nothing on the host between launches — the whole update is 24 launches
on one stream, replayed as a hipGraph.
"""
import collections
import contextlib
import os

import numpy as np
import torch

from . import hip

_UPDATE_PARTS = ("all", "front", "mid", "back")

# One record per loss of the update step (PPOLearnerHIP.set_loss); everything the host does per mode is read from here.
#   launch       the method that enqueues the loss where the PPO loss stands; its docstring describes the mode
#   tag          first element of the mode's entry in the hipGraph keys (_mode_key); None: no entry
#   state        the attribute that holds the mode's scalars as a tuple, in the order of `scalars`
#   scalars      (set_loss keyword, field of the device-hyper block or None) each.  A scalar without a field goes by value always and
#                is part of the key always; one with a field lives in the block in device-hyper mode (set_hyper moves it, the key
#                leaves it out) and None keeps its current value
#   rows         the attribute of the PPO / other row split (set by "set" + rows); strict: 0 < B_ppo < B instead of 0 <= B_ppo <= B
#   table        (attribute, its part of the key while unset, the call that sets it): a tensor [2][R][64] or a (tensor, extras) pair
#                whose address is baked into captured graphs, so the key holds the address, then R or the extras
#   check        a refusal of set_loss and update (the mode runs outside the learner section)
#   own_stats    (workspace key, fields): the mode has no PPO diagnostics; update(stats_row=) copies these instead
#   last_stats   (attribute, workspace key): the statistics tensor of the step that ran last, for the section object
#   reads_allowed / one_geometry   the launch reads the rows' `allowed` words / the storages of a step must share one geometry
class LossMode(collections.namedtuple(
        "LossMode", "launch tag state scalars rows strict table check own_stats last_stats reads_allowed one_geometry",
        defaults=(None, None, (), None, False, None, None, None, None, False, False))):
    __slots__ = ()
    ppo = property(lambda m: m.own_stats is None, doc="the loss has the PPO ratio (it reads old_logp) and the PPO diagnostics")


LOSS_MODES = {
    "ppo": LossMode("_ppo_launch"),
    "bc": LossMode("_bc_launch", "bc", "_bc", (("label_smoothing", None), ("bc_coeff", None)), check="_check_bc_modes",
                   own_stats=("bc_stats", hip.BC_STATS_FIELDS)),
    "ppo+demo": LossMode("_demo_launch", "demo", "_demo", (("label_smoothing", None), ("demo_coeff", hip.HP_DEMO_COEFF),
                                                          ("demo_value_coeff", hip.HP_DEMO_VALUE_COEFF)), rows="_demo_rows"),
    "aux": LossMode("_aux_launch", "aux", "_aux", (("beta_clone", None), ("aux_value_coeff", None)),
                    table=("_aux_table", (None, 0), "set_aux_table(table)"), check="_check_aux_modes",
                    own_stats=("aux_stats", hip.AUX_STATS_FIELDS)),
    "ppo+suggest": LossMode("_sug_launch", "suggest", "_sug", (("suggest_coeff", hip.HP_SUGGEST_COEFF),),
                            table=("_sug_tables", (None, 0), "set_suggest_tables(prior, Z)"),
                            last_stats=("_last_sug_stats", "sug_stats"), one_geometry=True),
    "ppo+sil": LossMode("_sil_launch", "sil", "_sil", (("sil_coeff", hip.HP_SIL_COEFF), ("sil_value_coeff", hip.HP_SIL_VALUE_COEFF)),
                        rows="_sil_rows"),
    "ppo+smooth": LossMode("_smooth_launch", "smooth", "_smooth", (("smooth_coeff", hip.HP_SMOOTH_COEFF),), rows="_smooth_rows",
                           strict=True, table=("_smooth_tables", (None,), "set_smooth_tables(ctrl, head_scale)"), one_geometry=True),
    "ppo+mask": LossMode("_am_launch", "mask", last_stats=("_last_am_stats", "am_stats"), reads_allowed=True, one_geometry=True),
}
# the loss coefficients that can live in the block: keyword -> (state attribute, position in it, block field)
_HP_LOSS = {k: (m.state, i, field) for m in LOSS_MODES.values() for i, (k, field) in enumerate(m.scalars) if field is not None}
_KEEP = object()


def _loss_record(mode):
    """The record of a loss mode by name."""
    if mode not in LOSS_MODES:
        raise ValueError("set_loss: mode %r (known: %s)" % (mode, ", ".join(repr(k) for k in LOSS_MODES)))
    return LOSS_MODES[mode]


def _loss_scalars(m, given, current):
    """The scalars of mode `m` from set_loss's keywords, as the tuple its state attribute holds.  label_smoothing: in [0, 1).  Every
    other one is a coefficient: a finite number, no bool; None keeps the current value of a coefficient that can live in the block."""
    bad = ValueError("set_loss: " + ", ".join("%s=%r" % (k, given[k]) for k, _ in m.scalars if k != "label_smoothing"))
    out = []
    for (k, field), cur in zip(m.scalars, current):
        v = given[k]
        if k == "label_smoothing":
            v = float(v)
            if not 0.0 <= v < 1.0:
                raise ValueError("set_loss: label_smoothing must be in [0, 1) (got %r)" % (given[k],))
        else:
            if isinstance(v, bool):
                raise bad
            try:
                v = cur if (v is None and field is not None) else float(v)
            except (TypeError, ValueError):
                raise bad
            if not np.isfinite(v):
                raise bad
        out.append(v)
    return tuple(out)


def _hyper_property(attr, field):
    """clip / vc / cc / ec: the captured update graphs hold these BY VALUE.  In device-hyper mode an assignment goes to the
    block (set_hyper); otherwise a changed value drops the captured update graphs, so the next step runs — and is then
    re-captured — with the new value instead of silently replaying the old one."""
    def get(self):
        return getattr(self, attr)

    def set_(self, value):
        value = float(value)
        old = getattr(self, attr, None)
        setattr(self, attr, value)
        if old is None or value == old:
            return
        if self._hp_on:
            self.set_hyper(**{field: value})
        else:
            self._drop_update_graphs()
    return property(get, set_)


class PPOLearnerHIP:
    SORT_MIN_B = 64
    clip = _hyper_property("_clip", "clip")
    vc = _hyper_property("_vc", "value_coeff")
    cc = _hyper_property("_cc", "clip_coeff")
    ec = _hyper_property("_ec", "ent_coeff")
    _sug_coeff = property(lambda self: self._sug[0])
    _smooth_coeff = property(lambda self: self._smooth[0])

    def sorted_rows(self, B):
        """Row-sorted update (rows of a minibatch grouped by command; every kernel of the step then works on exactly
        the run of rows a command net owns).  At minibatch 64 a command net owns ~16 of the 64 rows, so the
        unsorted form spends 4x the fp32-MFMA time the update needs — and the recurrent steps are bound by
        exactly that (the matrix pipe on their critical path), not by the weight stream."""
        return self.use_sorted and B >= self.SORT_MIN_B and B % 32 == 0

    def __init__(self, arena, clip=0.1, value_coeff=0.1, clip_coeff=1.0, ent_coeff=0.01, seq_length=8):
        self.a = arena
        self._ws = {}
        self._graphs = {}
        # device-resident hyper-parameters (opt-in, set_device_hyper): the kernels read lr, clip, the loss coefficients and
        # max_grad_norm from a block in device memory, so the captured graphs stay static whatever the values do
        self._hp_on = False
        self._hp = None            # device float64 [hip.HP_FIELDS]; allocated once (captured graphs hold its address)
        self._hp_host = None       # host mirror (numpy float64): what the block holds, except lr while the controller moves it
        self._adaptive = None      # (desired_kl, factor, lr_min, lr_max) while the KL-adaptive learning rate is on
        self._hp_moved = False     # clip or a loss coefficient changed in device-hyper mode: by-value update graphs are stale
        self.clip, self.vc, self.cc, self.ec = float(clip), float(value_coeff), float(clip_coeff), float(ent_coeff)
        self.S = seq_length
        self._wp = None            # recurrent weights in MFMA fragment order (forward, backward), re-packed per optimiser step
        self._wp_key = None
        self.pack_outside_capture = False      # act() graphs: the copies are refreshed eagerly before each replay
        self.launches = {}
        self.use_graphs = os.environ.get("CADRE_HIP_GRAPHS", "1") != "0"
        self.use_sorted = os.environ.get("CADRE_SORTED_UPDATE", "1") != "0"
        # forward LSTM of the update as one persistent launch (cadre_lstm_seq_fwd) instead of one launch per time step:
        # opt-in, measured slower in place (C2 208 vs 192 us, C3 376 vs 295 us for the 8 steps)
        # (A/B build only: the default library does not export it)
        self.persistent_lstm = os.environ.get("CADRE_LSTM_PERSISTENT", "0") != "0" and hip.has_ab_kernels()
        # MLP towers of the update as three fused launches (cadre_mlp_fwd / _bwd / _dw) instead of 17 GEMM / column-sum /
        # mask launches; CADRE_FUSED_MLP=0 keeps the GEMM chain (A/B)
        self.fused_mlp = os.environ.get("CADRE_FUSED_MLP", "1") != "0"
        # CADRE_ADAM_PACK=1: the optimiser step writes the fragment-order copies of W_hh itself (cadre_clip_adam_pack_graph)
        # and the update that follows an in-process clip_adam() carries no packing launch.  Opt-in: bit-identical, one kernel
        # fewer (23 vs 24 per step) and 110 MB less traffic, but NOT faster — same box, C3: 0.987 / 0.992 vs 0.988 / 0.980 ms
        # per step: the 4 x 4-block thread mapping scatters its 16-byte stores into both copies
        self.fused_pack = os.environ.get("CADRE_ADAM_PACK", "0") != "0"
        self._adam_fresh = None    # _pkey() right after a fused optimiser step of THIS learner: the copies are current
        self._skip_pack = False
        self._mlp_offs = None
        # update diagnostics and the target_kl gate (opt-in, set per learner section by set_update_modes): the loss launch
        # becomes cadre_ppo_loss_stats, the optimiser step its gated twin.  Both modes are part of the hipGraph keys; with
        # both off every key, launch and bit is what it was without them.
        self.stats = False
        self.target_kl = None
        self._stop = None          # device int32: the gate's sticky flag for the current round
        self._norm_row = None      # stats row that receives the next optimiser step's per-model gradient norms
        # rank consensus (opt-in, several ranks): the gate and the adaptive lr are decided by cadre_kl_consensus from the KL
        # summed over the ranks (kl_consensus, between the gradient exchange and the optimiser step), not by the loss kernel
        self.consensus = False
        self._cons_modes = False   # asked for by set_update_modes (the section's gate / diagnostics)
        self._cons_adaptive = False  # asked for by set_adaptive_lr (stays on between sections)
        self._kl_buf = None        # device float32 [4]: approx_kl steer, throttle of the step (two spare slots), reduced in place
        self._kl_sink = None       # device float32 [2] that receives the next step's reduced pair (the section's table)
        self._last_stats = None    # the workspace stats row of the update that ran last
        # loss of the update (set_loss): "ppo", or "bc" — the imitation loss cadre_bc_loss in the place of the PPO loss
        # launch, everything behind it unchanged.  The mode and its two scalars are part of the hipGraph keys.
        self.loss_mode = "ppo"
        self._bc = (0.0, 1.0)      # (label_smoothing, bc_coeff) of the imitation loss
        # "ppo+demo": cadre_ppo_demo_loss — PPO rows and demonstration rows in one minibatch (DAPG-style mixing)
        self._demo = (0.0, 0.0, 0.0)   # (label_smoothing, demo_coeff, demo_value_coeff) of the mixed loss
        self._demo_rows = None     # B_ppo: the leading unsorted rows of the minibatch that are PPO rows (set_demo_rows)
        # "aux": cadre_aux_loss — the PPG auxiliary phase (critic at full weight, the policy held by a KL term against the
        # distributions recorded in the table of set_aux_table)
        self._aux = (1.0, 1.0)     # (beta_clone, aux_value_coeff)
        self._aux_table = None     # device float32 [2][R][64]; its address and R are part of the hipGraph keys
        # "ppo+suggest": cadre_ppo_sug_loss — the PPO loss plus KL(pi || prior of the row's terminal event) on marked rows
        self._sug = (0.0,)         # (suggest_coeff,)
        self._sug_tables = None   # (prior: device float32 [2][Z + 1][64], Z); the address and Z are part of the hipGraph keys
        self._sug_ord = None       # the rank table of two categorical heads (the entry point wants one), when the arena has none
        self._last_sug_stats = None  # workspace(B)["sug_stats"] of the "ppo+suggest" update that ran last
        # "ppo+sil": cadre_ppo_sil_loss — PPO rows and self-imitation rows (the agent's own past rollouts) in one minibatch
        self._sil = (0.0, 0.0)     # (sil_coeff, sil_value_coeff)
        self._sil_rows = None      # B_ppo: the leading unsorted rows of the minibatch that are PPO rows (set_sil_rows)
        # "ppo+smooth": cadre_ppo_smooth_loss — PPO rows and their successor rows in one minibatch, coupled in pairs
        self._smooth = (0.0,)      # (smooth_coeff,)
        self._smooth_rows = None   # B_ppo: the leading unsorted rows of the minibatch that are PPO rows (set_smooth_rows)
        self._smooth_tables = None  # (ctrl: device float32 [2][64], (scale_steer, scale_throttle)); the address is part of the graph keys
        # "ppo+mask": cadre_ppo_am_loss — the PPO loss under the rows' allowed-bin words (workspace(B)["allowed"])
        self._last_am_stats = None  # workspace(B)["am_stats"] of the "ppo+mask" update that ran last
        # weight averaging (opt-in, set_weight_average): clip_adam() issues the average's update behind the optimiser launches
        self._avg = None           # a cadre_amd.average.WeightAverage of this arena; part of the optimiser graphs' keys
        self._avg_swapped = False  # inside CadreAgent.averaged_weights(): the arena holds the average, nothing may step it
        hip.lib()

    # ------------------------------------------------------------------ weight averaging
    def set_weight_average(self, avg):
        """avg: a cadre_amd.average.WeightAverage of this learner's arena, or None.  While one is set clip_adam() issues
        cadre_ema_update directly behind the optimiser launches, in the same captured graph (the key gains one element; with
        none set the key and the body are what they are without the module), and passes the gate's flag exactly when the gated
        optimiser twin is used: a skipped step is skipped — and counted — there too.  Every in-process path that steps the
        arena goes through clip_adam(); clip_adam_sharded() refuses an average."""
        if avg is not None and avg.arena is not self.a:
            raise hip.CadreHipError("set_weight_average: the average was built for another arena")
        if self._avg_swapped:
            raise hip.CadreHipError("set_weight_average inside averaged_weights(): the arena holds the average")
        self._avg = avg

    def _check_not_swapped(self, what):
        if self._avg_swapped:
            raise hip.CadreHipError("%s inside averaged_weights(): the arena holds the average, not the parameters the optimiser "
                                    "state belongs to" % what)

    # ------------------------------------------------------------------ loss selection
    def set_loss(self, mode, label_smoothing=0.0, bc_coeff=1.0, demo_coeff=None, demo_value_coeff=None, beta_clone=1.0,
                 aux_value_coeff=1.0, suggest_coeff=None, sil_coeff=None, sil_value_coeff=None, smooth_coeff=None):
        """"ppo" (default): the clipped-surrogate loss.  Every other mode (LOSS_MODES) is described at its launch: "bc" _bc_launch,
        "ppo+demo" _demo_launch, "aux" _aux_launch, "ppo+suggest" _sug_launch, "ppo+sil" _sil_launch, "ppo+smooth" _smooth_launch,
        "ppo+mask" _am_launch.  The keywords are the scalars of the mode that is being selected; those of another mode are not read."""
        given = dict(locals())
        m = _loss_record(mode)
        if m.scalars:
            vals = _loss_scalars(m, given, getattr(self, m.state))
            if m.check:
                getattr(self, m.check)()
            setattr(self, m.state, vals)
            block = {k: v for (k, field), v in zip(m.scalars, vals) if field is not None}
            if block and self._hp_on:
                self.set_hyper(**block)
        self.loss_mode = mode

    def loss_begin(self, mode, rows=None, table=_KEEP, **scalars):
        """This loss until loss_restore(token): set_loss(mode, **scalars) where a None scalar keeps its current value, the row split
        `rows` of a mode that has one and the table `table` of one that has one.  Returns the token."""
        m = _loss_record(mode)
        saved = [(attr, getattr(self, attr)) for attr in (m.rows, m.state if scalars else None, m.table and m.table[0]) if attr]
        token = (self.loss_mode, m, saved)
        try:
            if table is not _KEEP:
                getattr(self, m.table[2].split("(")[0])(table)
            cur = dict(zip((k for k, _ in m.scalars), getattr(self, m.state))) if m.scalars else {}
            self.set_loss(mode, **{k: cur.get(k) if v is None else v for k, v in scalars.items()})
            if m.rows:
                self._set_rows(m.rows, rows)
        except Exception:
            self.loss_restore(token)
            raise
        return token

    def loss_restore(self, token):
        """Back to what loss_begin found: the mode, the row split and the table always; the scalars when the call gave any — except
        those of a mode whose coefficients live in the block, in device-hyper mode: values written to the block stay."""
        mode, m, saved = token
        self.loss_mode = mode
        for attr, value in saved:
            if not (attr == m.state and self._hp_on and any(field is not None for _, field in m.scalars)):
                setattr(self, attr, value)

    @contextlib.contextmanager
    def loss_scope(self, mode, **kw):
        """with learner.loss_scope(mode, ...): loss_begin / loss_restore around one call."""
        token = self.loss_begin(mode, **kw)
        try:
            yield self
        finally:
            self.loss_restore(token)

    def _set_rows(self, attr, B_ppo):
        if B_ppo is not None and int(B_ppo) < 0:
            raise ValueError("set%s: B_ppo=%r" % (attr, B_ppo))
        setattr(self, attr, None if B_ppo is None else int(B_ppo))

    def set_demo_rows(self, B_ppo):
        """"ppo+demo": unsorted rows 0 .. B_ppo - 1 of the next minibatches are PPO rows, the rest demonstration rows."""
        self._set_rows("_demo_rows", B_ppo)

    def set_sil_rows(self, B_ppo):
        """"ppo+sil": unsorted rows 0 .. B_ppo - 1 of the next minibatches are PPO rows, the rest SIL rows."""
        self._set_rows("_sil_rows", B_ppo)

    def set_smooth_rows(self, B_ppo):
        """"ppo+smooth": unsorted rows 0 .. B_ppo - 1 of the next minibatches are PPO rows, the rest successor rows."""
        self._set_rows("_smooth_rows", B_ppo)

    def _split(self, B):
        """B_ppo of the selected mode, checked against the minibatch."""
        m = LOSS_MODES[self.loss_mode]
        B_ppo = getattr(self, m.rows)
        if B_ppo is None or (not 0 < B_ppo < B if m.strict else B_ppo > B):
            raise hip.CadreHipError("the %r loss needs set%s(B_ppo) with %s (got %r, B = %d)"
                                    % (self.loss_mode, m.rows, "0 < B_ppo < B" if m.strict else "0 <= B_ppo <= B", B_ppo, B))
        return B_ppo

    def _table(self):
        """The table of the selected mode."""
        attr, _, setter = LOSS_MODES[self.loss_mode].table
        if getattr(self, attr) is None:
            raise hip.CadreHipError("the %r loss needs %s first" % (self.loss_mode, setter))
        return getattr(self, attr)

    # the runs of arguments the loss entry points share (every PPO-family one takes rows, scalars, gradients and the stats tail, in
    # that order); a launch puts its own between them
    def _tower_args(self, w, B):
        """Logits and values of the towers, each with its pitch and net stride."""
        O3, NP = w["O3"], self.a.NP
        return (hip.ptr(O3), NP, 2 * B * NP, hip.ptr(O3[1]), NP, 2 * B * NP)

    def _row_args(self, w, B):
        """The tower outputs, then the six row arrays of the minibatch."""
        return self._tower_args(w, B) + tuple(hip.ptr(w[k]) for k in ("actions", "commands", "old_values", "returns", "old_logp", "adv"))

    def _scalar_args(self, B, inv_b):
        """B, C, K0, K1, then the block (NULL: the four scalars that follow count), clip, vc, cc, ec and inv_b."""
        a = self.a
        return (B, a.C, a.n_out[0], a.n_out[1], hip.ptr(self._hp) if self._hp_on else None, self.clip, self.vc, self.cc, self.ec, inv_b)

    def _stats_args(self, w, B):
        """The stats row (NULL: no diagnostics), F, its scratch, target_kl of the launch and the gate's flag."""
        stats = self._loss_stats()
        srow, sscr = self._stats_ws(w, B) if stats else (None, None)
        return (hip.ptr(srow), srow.shape[1] if stats else 0, hip.ptr(sscr), self._loss_tkl(),
                hip.ptr(self._stop) if (stats and self.target_kl is not None) else None)

    def _grad_args(self, w, *scratch):
        """dO3 (dlogits, dvalues), the loss scratch, a mode's own scratch tensors and the sync word the launch clears."""
        dO3 = w["dO3"]
        return ((hip.ptr(dO3), hip.ptr(dO3[1]), hip.ptr(w["loss_scratch"])) + tuple(hip.ptr(w[k]) for k in scratch)
                + (hip.ptr(w["sync"][self.a.Z * self.S:]),))

    def _ord(self, marker=False):
        """The arena's rank table; marker: the table of two categorical heads where the arena has none."""
        ord_t = getattr(self.a, "ord", None)
        return self.marker_ord() if (ord_t is None and marker) else ord_t

    def _mix_kinds(self, w, B, B_ppo, sorted_rows):
        hip.check(hip.lib().cadre_mix_row_kinds(hip.ptr(w["pos"]) if sorted_rows else None, B, B_ppo, hip.ptr(w["row_kind"]),
                                                hip.stream()), "cadre_mix_row_kinds")

    # ------------------------------------------------------------------ demonstration mixing
    def _demo_ws(self, w, B):
        """The static tensors of the "ppo+demo" loss in workspace(B)."""
        if "row_kind" not in w:
            dev, nblk = self.a.device, (B + 15) // 16
            w["row_kind"] = torch.zeros(2, B, dtype=torch.int32, device=dev)
            w["demo_losses"] = torch.zeros(2, device=dev)
            w["demo_stats"] = torch.zeros(2, hip.BC_STATS_FIELDS, device=dev)
            w["demo_scratch"] = torch.zeros(2 * nblk * (2 + hip.BC_STATS_FIELDS), device=dev)

    def _demo_launch(self, w, B, inv_b, sorted_rows):
        """cadre_mix_row_kinds + cadre_ppo_demo_loss on the tower outputs in workspace(B), in the place of the PPO loss.
        "ppo+demo": the clipped-surrogate loss on the first set_demo_rows() unsorted rows of the minibatch and the imitation
        loss (weight `demo_coeff`, critic weight `demo_value_coeff`, `label_smoothing`, no entropy term, mean over the
        demonstration rows) on the rest, in ONE launch (cadre_ppo_demo_loss).  Diagnostics, the KL gate, the adaptive lr and
        rank consensus work as in "ppo" and see the PPO rows only; a stopped step skips the whole update, the demonstration
        term included.  In device-hyper mode the two demo coefficients live in the block (set_hyper(demo_coeff=, ...)):
        a changed value needs no new graph.  None keeps the current coefficient.  The demo losses / statistics of a step are
        in workspace(B)["demo_losses"] / ["demo_stats"]."""
        B_ppo = self._split(B)
        self._demo_ws(w, B)
        self._mix_kinds(w, B, B_ppo, sorted_rows)
        p = hip.ptr
        hip.check(hip.lib().cadre_ppo_demo_loss(
            *self._row_args(w, B), p(w["row_kind"]), *self._scalar_args(B, inv_b), *self._demo, 1.0 / (B - B_ppo) if B > B_ppo else 1.0,
            p(w["losses"]), p(w["demo_losses"]), *self._grad_args(w, "demo_scratch"), *self._stats_args(w, B), p(w["demo_stats"]),
            hip.BC_STATS_FIELDS, p(self._ord()), hip.stream()), "cadre_ppo_demo_loss")

    # ------------------------------------------------------------------ self-imitation
    def _sil_ws(self, w, B):
        """The static tensors of the "ppo+sil" loss in workspace(B)."""
        if "sil_w" not in w:
            dev, nblk = self.a.device, (B + 15) // 16
            if "row_kind" not in w:
                w["row_kind"] = torch.zeros(2, B, dtype=torch.int32, device=dev)
            w["sil_w"] = torch.zeros(2, B, device=dev)
            w["sil_losses"] = torch.zeros(2, device=dev)
            w["sil_stats"] = torch.zeros(2, hip.SIL_STATS_FIELDS, device=dev)
            w["sil_scratch"] = torch.zeros(2 * nblk * (2 + hip.SIL_STATS_FIELDS), device=dev)
        return w["sil_w"]

    def _sil_launch(self, w, B, inv_b, sorted_rows):
        """cadre_mix_row_kinds + cadre_ppo_sil_loss on the tower outputs in workspace(B), in the place of the PPO loss.
        "ppo+sil": the clipped-surrogate loss on the first set_sil_rows() unsorted rows of the minibatch and the
        self-imitation terms on the rest — w = max(R - v, 0) with R from the `returns` column, `sil_coeff` * mean(-lp w) +
        `sil_value_coeff` * mean(0.5 w^2) over the SIL rows — in ONE launch (cadre_ppo_sil_loss).  Diagnostics, the KL gate,
        the adaptive lr and rank consensus work as in "ppo" and see the PPO rows only.  In device-hyper mode the two
        coefficients live in the block (set_hyper(sil_coeff=, sil_value_coeff=)): a changed value needs no new graph.  None
        keeps the current coefficient.  The SIL losses / statistics / per-row w of a step are in workspace(B)["sil_losses"] /
        ["sil_stats"] / ["sil_w"] (static tensors, as the kinds in ["row_kind"])."""
        B_ppo = self._split(B)
        self._sil_ws(w, B)
        self._mix_kinds(w, B, B_ppo, sorted_rows)
        p = hip.ptr
        hip.check(hip.lib().cadre_ppo_sil_loss(
            *self._row_args(w, B), p(w["row_kind"]), *self._scalar_args(B, inv_b), *self._sil, 1.0 / (B - B_ppo) if B > B_ppo else 1.0,
            p(w["losses"]), p(w["sil_losses"]), p(w["sil_w"]), *self._grad_args(w, "sil_scratch"), *self._stats_args(w, B),
            p(w["sil_stats"]), hip.SIL_STATS_FIELDS, p(self._ord()), hip.stream()), "cadre_ppo_sil_loss")

    # ------------------------------------------------------------------ temporal smoothness
    def set_smooth_tables(self, ctrl, head_scale=(1.0, 1.0)):
        """The control tables of the "ppo+smooth" loss: device float32 [2][64], contiguous, the control value of bin k of head h
        in [h][k] (cadre_amd.smooth.smooth_tables; None: forget them), and the two head scales (finite, >= 0).  The table's
        address is baked into captured graphs, so it is part of their key, as the scales are."""
        if ctrl is None:
            self._smooth_tables = None
            return
        if (not ctrl.is_cuda or ctrl.dtype != torch.float32 or tuple(ctrl.shape) != (2, 64) or not ctrl.is_contiguous()):
            raise ValueError("set_smooth_tables: expected a contiguous device float32 tensor [2][64]")
        try:
            hs = (float(head_scale[0]), float(head_scale[1]))
            ok = len(head_scale) == 2 and all(np.isfinite(x) and x >= 0.0 for x in hs)
        except (TypeError, ValueError, IndexError):
            ok = False
        if not ok:
            raise ValueError("set_smooth_tables: head_scale=%r (two finite numbers >= 0)" % (head_scale,))
        self._smooth_tables = (ctrl, hs)

    def _smooth_ws(self, w, B):
        """The static tensors of the "ppo+smooth" loss in workspace(B): (row_kind, mate), which cadre_smooth_mates overwrites
        before every step."""
        if "mate" not in w:
            dev, nblk = self.a.device, (B + 15) // 16
            if "row_kind" not in w:
                w["row_kind"] = torch.zeros(2, B, dtype=torch.int32, device=dev)
            w["mate"] = torch.full((2, B), -1, dtype=torch.int32, device=dev)
            w["smooth_d"] = torch.zeros(2, B, device=dev)
            w["smooth_losses"] = torch.zeros(1, device=dev)
            w["smooth_stats"] = torch.zeros(2, hip.SMOOTH_STATS_FIELDS, device=dev)
            w["smooth_scratch"] = torch.zeros(2 * nblk * hip.SMOOTH_STATS_FIELDS, device=dev)
        return w["row_kind"], w["mate"]

    def _smooth_launch(self, w, B, inv_b, sorted_rows=False):
        """cadre_ppo_smooth_loss on the tower outputs in workspace(B), in the place of the PPO loss.
        "ppo+smooth": the clipped-surrogate loss on the first set_smooth_rows() unsorted rows of the minibatch, the rest being
        their successor rows (row t + 1 of the same storages), plus `smooth_coeff` * head_scale * mean over the pair slots of
        d^2, d the difference of the two rows' mean controls (CAPS's temporal term; set_smooth_tables gives the control tables)
        — in ONE launch (cadre_ppo_smooth_loss); the gradient goes into both rows of a pair.  Diagnostics, the KL gate, the
        adaptive lr and rank consensus work as in "ppo" and see the PPO rows only, without the term.  In device-hyper mode
        the coefficient lives in the block (set_hyper(smooth_coeff=)): a changed value needs no new graph.  None keeps the
        current coefficient.  The pairs of a step are in workspace(B)["row_kind"] / ["mate"] (cadre_smooth_mates writes them
        before the step), its smoothness loss / statistics / per-row d in ["smooth_losses"] / ["smooth_stats"] / ["smooth_d"]."""
        B_ppo = self._split(B)
        ctrl, hs = self._table()
        self._smooth_ws(w, B)
        p = hip.ptr
        hip.check(hip.lib().cadre_ppo_smooth_loss(
            *self._row_args(w, B), p(w["row_kind"]), p(w["mate"]), p(ctrl), *self._scalar_args(B, inv_b), self._smooth_coeff, hs[0],
            hs[1], 1.0 / (B - B_ppo), p(w["losses"]), p(w["smooth_losses"]), p(w["smooth_d"]), *self._grad_args(w, "smooth_scratch"),
            *self._stats_args(w, B), p(w["smooth_stats"]), hip.SMOOTH_STATS_FIELDS, p(self._ord()), hip.stream()),
            "cadre_ppo_smooth_loss")

    # ------------------------------------------------------------------ exploration suggestions
    def set_suggest_tables(self, prior, Z=None):
        """The prior table of the "ppo+suggest" loss: device float32 [2][Z + 1][64], contiguous, RAW log-priors in columns < K
        per (head, kind), row 0 unused (None: forget it).  Z: the number of kinds, 1 .. 8 (None: from the shape).  The
        table's address is baked into captured graphs, so it is part of their key."""
        if prior is None:
            self._sug_tables = None
            return
        if (not prior.is_cuda or prior.dtype != torch.float32 or prior.dim() != 3 or prior.shape[0] != 2
                or prior.shape[2] != 64 or not prior.is_contiguous()):
            raise ValueError("set_suggest_tables: expected a contiguous device float32 tensor [2][Z + 1][64]")
        Z = prior.shape[1] - 1 if Z is None else Z
        if isinstance(Z, bool) or not isinstance(Z, int) or not 1 <= Z <= 8 or prior.shape[1] != Z + 1:
            raise ValueError("set_suggest_tables: Z=%r with a table of %d rows per head (Z in 1 .. 8, Z + 1 rows)"
                             % (Z, prior.shape[1]))
        self._sug_tables = (prior, Z)

    def _sug_ws(self, w, B):
        """The static tensors of the "ppo+suggest" loss in workspace(B); sug_kind is zeroed once, here."""
        if "sug_kind" not in w:
            dev = self.a.device
            w["sug_kind"] = torch.zeros(2, B, dtype=torch.int32, device=dev)
            w["sug_losses"] = torch.zeros(1, device=dev)
            w["sug_stats"] = torch.zeros(2, hip.SUG_STATS_FIELDS, device=dev)
            w["sug_scratch"] = torch.zeros(2 * 4 * ((B + 15) // 16), device=dev)
        return w["sug_kind"]

    def _sug_launch(self, w, B, inv_b, sorted_rows=False):
        """cadre_ppo_sug_loss on the tower outputs in workspace(B), in the place of the PPO loss.
        "ppo+suggest": the clipped-surrogate loss plus, on the rows whose kind in workspace(B)["sug_kind"] (int32 [2][B] in
        workspace order, a static tensor that cadre_suggest_rows fills before the update) is z >= 1, `suggest_coeff` times
        KL(pi || prior z of the head) from the table of set_suggest_tables(), the mean taken over the minibatch rows
        (cadre_ppo_sug_loss, ONE launch).  Diagnostics, the KL gate, the adaptive lr and rank consensus work as in "ppo" and
        see what they see there.  In device-hyper mode the coefficient lives in the block (set_hyper(suggest_coeff=)): a
        changed value needs no new graph.  None keeps the current coefficient.  The suggestion loss / statistics of a step
        (hip.SUG_STATS_FIELDS per head) are in workspace(B)["sug_losses"] / ["sug_stats"]."""
        prior, Z = self._table()
        self._sug_ws(w, B)
        p = hip.ptr
        hip.check(hip.lib().cadre_ppo_sug_loss(
            *self._row_args(w, B), p(w["sug_kind"]), p(prior), Z, *self._scalar_args(B, inv_b), self._sug_coeff, p(w["losses"]),
            p(w["sug_losses"]), *self._grad_args(w, "sug_scratch"), *self._stats_args(w, B), p(w["sug_stats"]), hip.SUG_STATS_FIELDS,
            p(self._ord(marker=True)), hip.stream()), "cadre_ppo_sug_loss")

    # ------------------------------------------------------------------ action masks
    def _am_ws(self, w, B):
        """The static tensors of the "ppo+mask" loss in workspace(B); `allowed` is zeroed (every row unmasked) once, here."""
        if "allowed" not in w:
            dev = self.a.device
            w["allowed"] = torch.zeros(2, B, dtype=torch.int64, device=dev)
            w["am_stats"] = torch.zeros(2, hip.AM_STATS_FIELDS, device=dev)
            w["am_scratch"] = torch.zeros(2 * 5 * ((B + 15) // 16), device=dev)
        return w["allowed"]

    def marker_ord(self):
        """The rank table of two categorical heads (int32 [2][64] of -1) for the entry points that want a table when the arena has
        none: one per learner, shared by the suggestion loss, the masked loss and the agent's masked samplers."""
        if self._sug_ord is None:
            self._sug_ord = torch.full((2, 64), -1, dtype=torch.int32, device=self.a.device)
        return self._sug_ord

    def _am_launch(self, w, B, inv_b, sorted_rows=False):
        """cadre_ppo_am_loss on the tower outputs in workspace(B), in the place of the PPO loss.
        "ppo+mask": the clipped-surrogate loss under action masks (cadre_ppo_am_loss, ONE launch where the PPO loss stands): a
        row's word in workspace(B)["allowed"] (int64 [2][B] in workspace order, a static tensor that cadre_allowed_rows fills
        before the update; bit k set: bin k may be chosen, no bit among the head's bins: unmasked) restricts the softmax, the
        entropy and the gradient to the allowed bins; with every word unmasked the step is bit-identical to "ppo".  It has no
        scalar of its own: diagnostics, the KL gate, the adaptive lr, device hyper-parameters, ordinal heads and rank
        consensus work as in "ppo".  The mask statistics of a step (hip.AM_STATS_FIELDS per head) are in
        workspace(B)["am_stats"]."""
        self._am_ws(w, B)
        p = hip.ptr
        hip.check(hip.lib().cadre_ppo_am_loss(
            *self._row_args(w, B), *self._scalar_args(B, inv_b), p(w["losses"]), *self._grad_args(w), *self._stats_args(w, B),
            p(self._ord(marker=True)), p(w["allowed"]), p(w["am_stats"]), hip.AM_STATS_FIELDS, p(w["am_scratch"]), hip.stream()),
            "cadre_ppo_am_loss")

    # ------------------------------------------------------------------ PPG auxiliary phase
    def set_aux_table(self, table):
        """The table of recorded distributions the "aux" loss and aux_record work on: device float32 [2][R][64], contiguous
        (None: forget it).  Its address is baked into captured graphs, so it is part of their key."""
        if table is not None:
            if (not table.is_cuda or table.dtype != torch.float32 or table.dim() != 3 or table.shape[0] != 2
                    or table.shape[2] != 64 or table.shape[1] < 1 or not table.is_contiguous()):
                raise ValueError("set_aux_table: expected a contiguous device float32 tensor [2][R][64]")
        self._aux_table = table

    def _check_aux_modes(self):
        # (self.consensus also covers an adaptive lr armed with consensus=True, which stays on between sections: the
        #  optimiser step would then decide from a KL no auxiliary step reports)
        if self.stats or self.target_kl is not None or self.consensus:
            raise hip.CadreHipError("the auxiliary loss has no PPO diagnostics, KL gate or rank consensus: it runs outside "
                                    "the learner section (call set_update_modes() first)")

    def _aux_args(self, w, B, sorted_rows):
        self._table()
        if "aux_rows" not in w:
            w["aux_rows"] = torch.zeros(2, B, dtype=torch.int64, device=self.a.device)
            w["aux_stats"] = torch.zeros(2, hip.AUX_STATS_FIELDS, device=self.a.device)
            w["aux_scratch"] = torch.zeros(2 * hip.AUX_STATS_FIELDS * ((B + 15) // 16), device=self.a.device)
        return hip.ptr(w["pos"]) if sorted_rows else None, hip.ptr(w["aux_rows"]), hip.ptr(self._aux_table), self._aux_table.shape[1]

    def _aux_launch(self, w, B, inv_b, sorted_rows):
        """cadre_aux_loss on the tower outputs in workspace(B): losses[3], the stats row aux_stats [2][AUX_STATS_FIELDS] and
        dO3 (dlogits and dvalues).
        "aux": the PPG auxiliary loss (cadre_aux_loss) — aux_value_coeff * 0.5 * mean (v - R)^2 + beta_clone * mean
        KL(pi_old || pi), pi_old read from the table of set_aux_table() at the rows in workspace(B)["aux_rows"] (int64 [2][B]:
        the table row of each UNSORTED minibatch row; a static tensor the caller fills before the update).  The learner's own
        value_coeff / ent_coeff / clip are not used; actions, old_values, old_logp and adv are not read.  The two scalars go
        by value, yet the mode IS available in device-hyper mode: it reads nothing from the block and changes nothing in it
        (the optimiser step keeps reading lr / max_grad_norm there; the KL-adaptive controller lives in the PPO loss kernel
        and does not run).  Refused while set_update_modes(stats / target_kl / consensus) is armed.  The statistics of a step
        (hip.AUX_STATS_FIELDS per head) are in workspace(B)["aux_stats"]."""
        a, p = self.a, hip.ptr
        pos, rows, table, R = self._aux_args(w, B, sorted_rows)
        hip.check(hip.lib().cadre_aux_loss(
            *self._tower_args(w, B), p(w["commands"]), p(w["returns"]), pos, rows, table, R, B, a.C, a.n_out[0], a.n_out[1],
            *self._aux, inv_b, p(w["losses"]), *self._grad_args(w), p(w["aux_stats"]), hip.AUX_STATS_FIELDS, p(w["aux_scratch"]),
            p(self._ord()), hip.stream()), "cadre_aux_loss")

    def aux_record(self, B, sorted_rows=False):
        """Forward only on the packed minibatch in workspace(B) (eagerly, no captured graph: the record pass runs once per
        phase), then cadre_aux_record: the current policy's normalised log-probabilities of the minibatch rows go to the rows
        workspace(B)["aux_rows"] of the table (set_aux_table).  No gradient is written, no parameter moves."""
        if self.loss_mode != "aux":
            raise hip.CadreHipError("aux_record needs set_loss('aux')")
        self._check_aux_modes()
        a = self.a
        w = self.workspace(B)
        pos, rows, table, R = self._aux_args(w, B, sorted_rows)
        self._forward(w, B, (0, 1, a.Z), a.C, seg=w["seg"] if sorted_rows else None, fused_mlp=True)
        ord_t = getattr(a, "ord", None)
        hip.check(hip.lib().cadre_aux_record(hip.ptr(w["O3"]), a.NP, 2 * B * a.NP, hip.ptr(w["commands"]), pos, rows, B, a.C,
                                             a.n_out[0], a.n_out[1], hip.ptr(ord_t), table, R, hip.stream()),
                  "cadre_aux_record")

    # ------------------------------------------------------------------ sample reuse (cadre_amd.reuse)
    def reuse_record(self, B, logp_now, value_now, sorted_rows=False):
        """Forward only on the packed minibatch in workspace(B) (eagerly, as aux_record: the record pass runs once per
        section), then cadre_reuse_record: the current nets' log-probability of each row's stored action and critic output
        go to rows workspace(B)["reuse_rows"] (int64 [2][B], the table row of each UNSORTED minibatch row) of `logp_now` /
        `value_now`, device float32 [2][R] (trailing unit dimensions allowed), contiguous.  The forward is the update's own,
        so a step that gathers the same rows in the same order finds ratio == 1 exactly.  No gradient is written, no
        parameter moves; the loss mode plays no part."""
        for t in (logp_now, value_now):
            if (not t.is_cuda or t.dtype != torch.float32 or t.dim() < 2 or t.shape[0] != 2 or t.shape[1] < 1
                    or t.numel() != 2 * t.shape[1] or not t.is_contiguous()):
                raise ValueError("reuse_record: expected contiguous device float32 tables [2][R]")
        if logp_now.shape[1] != value_now.shape[1]:
            raise ValueError("reuse_record: logp_now and value_now differ in rows")
        a = self.a
        w = self.workspace(B)
        if "reuse_rows" not in w:
            raise hip.CadreHipError("reuse_record: workspace(B)['reuse_rows'] is filled by the gather (reuse_record_from_storages)")
        self._forward(w, B, (0, 1, a.Z), a.C, seg=w["seg"] if sorted_rows else None, fused_mlp=True)
        O3, NP = w["O3"], a.NP
        ord_t = getattr(a, "ord", None)
        hip.check(hip.lib().cadre_reuse_record(hip.ptr(O3), NP, 2 * B * NP, hip.ptr(O3[1]), NP, 2 * B * NP,
                                               hip.ptr(w["commands"]), hip.ptr(w["actions"]),
                                               hip.ptr(w["pos"]) if sorted_rows else None, hip.ptr(w["reuse_rows"]), B, a.C,
                                               a.n_out[0], a.n_out[1], hip.ptr(ord_t), hip.ptr(logp_now), hip.ptr(value_now),
                                               logp_now.shape[1], hip.stream()), "cadre_reuse_record")

    def _check_bc_modes(self):
        if self._hp_on:
            raise hip.CadreHipError("the imitation loss takes its scalars by value: it is not available in device-hyper mode "
                                    "(set_device_hyper(False), or pretrain before schedules / adaptive lr are armed)")
        if self._loss_stats() or self.consensus:
            raise hip.CadreHipError("the imitation loss has no PPO diagnostics, KL gate or rank consensus: call "
                                    "set_update_modes() first")

    def _bc_launch(self, w, B, inv_b, sorted_rows=False, grad=True):
        """cadre_bc_loss on the tower outputs in workspace(B): losses[3], the stats row bc_stats [2][BC_STATS_FIELDS] and,
        with `grad`, dO3 (dlogits and dvalues).  grad=False is the evaluation form.
        "bc": behaviour cloning — cross-entropy against the demonstrated bin
        (workspace `actions`; -1 = no label for that head) with `label_smoothing` in [0, 1) and weight `bc_coeff`, the critic
        regressed on workspace `returns`, the learner's own value_coeff / ent_coeff, per-row weights from the `adv` slot;
        old_values / old_logp are not read.  The imitation statistics of a step (hip.BC_STATS_FIELDS per head) are in
        workspace(B)["bc_stats"].  By-value scalars only: refused together with the device-hyper block."""
        a, p = self.a, hip.ptr
        if "bc_stats" not in w:
            w["bc_stats"] = torch.zeros(2, hip.BC_STATS_FIELDS, device=a.device)
            w["bc_scratch"] = torch.zeros(2 * hip.BC_STATS_FIELDS * ((B + 15) // 16), device=a.device)
        dl, dv, scratch, sync = self._grad_args(w)
        hip.check(hip.lib().cadre_bc_loss(
            *self._tower_args(w, B), p(w["actions"]), p(w["commands"]), p(w["returns"]), p(w["adv"]), B, a.C, a.n_out[0], a.n_out[1],
            *self._bc, self.vc, self.ec, inv_b, p(w["losses"]), dl if grad else None, dv if grad else None, scratch, sync,
            p(w["bc_stats"]), hip.BC_STATS_FIELDS, p(w["bc_scratch"]), p(self._ord()), hip.stream()), "cadre_bc_loss")

    def bc_evaluate(self, B, inv_b, sorted_rows=False, stats_row=None):
        """Forward + the evaluation form of the imitation loss on the packed minibatch in workspace(B): no gradient is
        written, no parameter moves.  The launch chain runs eagerly (no captured graph: a validation pass is bound by launch
        overhead, once per epoch).  Returns (losses[3], bc_stats [2][BC_STATS_FIELDS]) — the workspace tensors, which the
        next step overwrites; `stats_row` (device float32 [2][>= BC_STATS_FIELDS]) receives a copy of the statistics."""
        if self.loss_mode != "bc":
            raise hip.CadreHipError("bc_evaluate needs set_loss('bc')")
        self._check_bc_modes()
        a = self.a
        w = self.workspace(B)
        self._forward(w, B, (0, 1, a.Z), a.C, seg=w["seg"] if sorted_rows else None, fused_mlp=True)
        self._bc_launch(w, B, inv_b, grad=False)
        if stats_row is not None:
            stats_row[:, :hip.BC_STATS_FIELDS].copy_(w["bc_stats"])
        return w["losses"], w["bc_stats"]

    # ------------------------------------------------------------------ diagnostics / KL gate
    def stats_fields(self):
        """F of a stats row [2 heads][F]: hip.PPO_STATS_FIELDS loss diagnostics, then the head's 2 C gradient norms."""
        return hip.PPO_STATS_FIELDS + 2 * self.a.C

    def set_update_modes(self, stats=False, target_kl=None, consensus=False):
        """stats: the update writes its diagnostics (update(..., stats_row=)); target_kl (> 0): arm the KL gate and clear
        its flag — the round starts with the optimiser enabled.  set_update_modes() returns to the plain update.
        consensus (several ranks): the loss launch only reports the KL (it gets target_kl = 0 and reads the flag); the gate is
        decided by kl_consensus() from the KL summed over the ranks, which chief_step runs before the optimiser step."""
        if consensus and self._adaptive is not None and not self._cons_adaptive:
            raise hip.CadreHipError("rank consensus: the adaptive lr of this learner was armed without it "
                                    "(set_adaptive_lr(..., consensus=True)); one step cannot mix the two forms")
        if target_kl is not None:
            target_kl = float(target_kl)
            if not target_kl > 0.0:
                raise ValueError("target_kl must be > 0 (got %r)" % (target_kl,))
            if self._stop is None:
                self._stop = torch.zeros(1, dtype=torch.int32, device=self.a.device)
            else:
                self._stop.zero_()
        self.stats = bool(stats)
        self.target_kl = target_kl
        self._norm_row = None
        self._kl_sink = None
        self._cons_modes = bool(consensus)
        self.consensus = self._cons_modes or self._cons_adaptive

    def _loss_tkl(self):
        """target_kl of the loss launch: 0 (no check in the kernel) without a gate, and in consensus mode."""
        return 0.0 if (self.target_kl is None or self.consensus) else self.target_kl

    def kl_consensus(self, all_reduce_small):
        """Consensus mode, once per optimiser step, after the update and before clip_adam: the step's approx_kl pair (this
        rank's workspace stats row) -> `all_reduce_small` (SUM over the ranks, Shared_grad_buffers.all_reduce_small) ->
        cadre_kl_consensus on the sum: the stop flag, `applied` of the pending stats row and the adaptive lr, identically
        on every rank.  The collective is issued unconditionally: nothing here depends on a device value."""
        if not self.consensus:
            raise hip.CadreHipError("kl_consensus needs the consensus mode (set_update_modes / set_adaptive_lr with consensus=True)")
        if self._last_stats is None:
            raise hip.CadreHipError("kl_consensus: no update has run in a stats mode yet")
        if self._kl_buf is None:
            self._kl_buf = torch.zeros(4, device=self.a.device)
        buf = self._kl_buf
        buf[:2].copy_(self._last_stats[:, 0])
        all_reduce_small(buf)
        sink, self._kl_sink = self._kl_sink, None
        if sink is not None:
            sink.copy_(buf[:2])
        row = self._norm_row
        ad = self._adaptive if self._cons_adaptive else None
        hip.check(hip.lib().cadre_kl_consensus(hip.ptr(buf), 0.0 if self.target_kl is None else self.target_kl,
                                               hip.ptr(self._stop) if self.target_kl is not None else None,
                                               0.0 if ad is None else ad[0], hip.ptr(self._hp) if ad is not None else None,
                                               hip.ptr(row), 0 if row is None else row.shape[-1], hip.stream()),
                  "cadre_kl_consensus")

    def _loss_stats(self):
        return self.stats or self.target_kl is not None or self._adaptive is not None

    def _mode_key(self):
        """hipGraph key suffix of the update modes: () when all are off (today's graphs).  Device-hyper mode is a mode
        (("hp",)); the VALUES in the block are not part of any key.  Ordinal policy heads are a mode (("ord",)): the loss
        launch is then cadre_ppo_loss_ord.  Rank consensus is a mode (("consensus",)): the loss launch then decides nothing, so
        the graphs of the two forms never mix."""
        key = (("stats", self.target_kl),) if self._loss_stats() else ()
        key = key + ((("hp",),) if self._hp_on else ())
        key = key + ((("ord",),) if getattr(self.a, "ord", None) is not None else ())
        key = key + ((("consensus",),) if self.consensus else ())
        # a loss other than "ppo" is a mode: its graphs hold its launch and whatever that takes by value.  From its record: the
        # tag; the scalars that go by value always (label_smoothing, the imitation and auxiliary coefficients); B_ppo; the table's
        # address and R / Z / the head scales, which the graph holds; then the coefficients that can live in the block — unless
        # they do (device-hyper mode: a decaying coefficient replays one graph).  A mode without values is its tag alone
        m = LOSS_MODES[self.loss_mode]
        if m.tag is None:
            return key
        vals = getattr(self, m.state) if m.scalars else ()
        part = (m.tag,) + tuple(v for (_, field), v in zip(m.scalars, vals) if field is None)
        part += (getattr(self, m.rows),) if m.rows else ()
        if m.table:
            t = getattr(self, m.table[0])
            if t is None:
                part += m.table[1]
            elif isinstance(t, tuple):
                part += (t[0].data_ptr(),) + (t[1] if isinstance(t[1], tuple) else (t[1],))
            else:
                part += (t.data_ptr(), t.shape[1])
        if not self._hp_on:
            part += tuple(v for (_, field), v in zip(m.scalars, vals) if field is not None)
        return key + (part,)

    # ------------------------------------------------------------------ device-resident hyper-parameters
    def _drop_update_graphs(self, hp=False):
        """Forget the captured update graphs of the by-value (hp=False) or the device-hyper (hp=True) mode; the optimiser
        graphs are keyed on their values and stay.  Waits for the device first: a graph may still be replaying."""
        def mine(k):
            k = k[1:] if k and k[0] == "warm" else k
            return bool(k) and k[0] in _UPDATE_PARTS and (("hp",) in k) == hp
        drop = [k for k in self._graphs if mine(k)]
        if drop:
            torch.cuda.synchronize()
            for k in drop:
                del self._graphs[k]

    @property
    def device_hyper(self):
        return self._hp_on

    def set_device_hyper(self, on=True):
        """on: lr, clip, value_coeff, clip_coeff, ent_coeff and max_grad_norm live in a block of device memory (hip.HP) that
        the loss and optimiser kernels read when they RUN (the `_hp` entry points); set_hyper() changes them with one
        asynchronous copy, and captured graphs are replayed unchanged.  The block starts from the learner's current clip and
        coefficients, lr 3e-4 and max_grad_norm 250 (clip_adam's defaults; clip_adam(lr=, max_grad_norm=) updates them).
        With equal values every result is bit-identical to the by-value mode.  off: back to by-value arguments."""
        on = bool(on)
        if on == self._hp_on:
            return
        if not on:
            if self._adaptive is not None:
                self.set_adaptive_lr(None)
            self._hp_on = False
            if self._hp_moved:                 # (the by-value graphs were captured before the loss scalars moved)
                self._drop_update_graphs()
                self._hp_moved = False
            return
        if self._hp is None:
            self._hp = torch.zeros(hip.HP_FIELDS, dtype=torch.float64, device=self.a.device)
            self._hp_host = np.zeros(hip.HP_FIELDS, dtype=np.float64)
            # two pinned staging buffers, used in turn: one is rewritten only after the copy that last read it has finished
            self._hp_stage = [torch.zeros(hip.HP_FIELDS, dtype=torch.float64).pin_memory() for _ in range(2)]
            self._hp_events = [None, None]
            self._hp_i = 0
            self._hp_host[hip.HP["lr"]], self._hp_host[hip.HP["max_grad_norm"]] = 3e-4, 250.0
        m = self._hp_host
        m[hip.HP["clip"]], m[hip.HP["value_coeff"]] = self._clip, self._vc
        m[hip.HP["clip_coeff"]], m[hip.HP["ent_coeff"]] = self._cc, self._ec
        for state, i, field in _HP_LOSS.values():
            m[field] = getattr(self, state)[i]
        if np.isnan(m[hip.HP["lr"]]):
            m[hip.HP["lr"]] = 3e-4
        self._hp_on = True
        self._hp_upload(0, hip.HP_FIELDS)

    def _hp_upload(self, lo, hi):
        """Fields [lo, hi) of the mirror into the block: one asynchronous host-to-device copy on the current stream."""
        if torch.cuda.is_current_stream_capturing():
            raise hip.CadreHipError("set_hyper inside a stream capture: the copy would be baked into the graph")
        i = self._hp_i
        self._hp_i ^= 1
        if self._hp_events[i] is not None:
            self._hp_events[i].synchronize()   # (the upload before the last one: finished long ago in practice)
        stage = self._hp_stage[i]
        stage.numpy()[lo:hi] = self._hp_host[lo:hi]
        self._hp[lo:hi].copy_(stage[lo:hi], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._hp_events[i] = ev

    def hyper(self, name):
        """The host mirror's value of a block field (hip.HP).  "lr" is the last value SET while the KL-adaptive controller
        moves it on the device (the value each step used is in the step's stats row), NaN after set_adaptive_lr(None) until
        the next clip_adam / set_hyper supplies one."""
        self._need_hp("hyper")
        return float(self._hp_host[self._hp_index(name)])

    @staticmethod
    def _hp_index(name):
        """Block index of a named field: a loss coefficient's from its mode's record, every other from hip.HP."""
        return _HP_LOSS[name][2] if name in _HP_LOSS else hip.HP[name]

    def _need_hp(self, what):
        if not self._hp_on:
            raise hip.CadreHipError("%s needs device-hyper mode: call set_device_hyper() first" % what)

    def set_hyper(self, lr=None, clip=None, ent_coeff=None, value_coeff=None, clip_coeff=None, max_grad_norm=None,
                  demo_coeff=None, demo_value_coeff=None, suggest_coeff=None, sil_coeff=None, sil_value_coeff=None,
                  smooth_coeff=None):
        """New values for the given block fields: the mirror is updated and ONE asynchronous host-to-device copy (of the
        span of fields that changed) is enqueued on the current stream — no synchronisation, no new graph.  Steps enqueued
        afterwards use the new values.  An explicit lr also resets the KL-adaptive controller's current value.
        demo_coeff / demo_value_coeff: the two coefficients of the "ppo+demo" loss (read by cadre_ppo_demo_loss only).
        suggest_coeff: the coefficient of the "ppo+suggest" loss (read by cadre_ppo_sug_loss only).
        sil_coeff / sil_value_coeff: the two coefficients of the "ppo+sil" loss (read by cadre_ppo_sil_loss only).
        smooth_coeff: the coefficient of the "ppo+smooth" loss (read by cadre_ppo_smooth_loss only)."""
        new = {k: v for k, v in locals().items() if k != "self"}
        self._need_hp("set_hyper")
        idx = []
        for name, v in new.items():
            if v is None:
                continue
            v = float(v)
            if not np.isfinite(v):
                raise ValueError("set_hyper: %s=%r" % (name, v))
            i = self._hp_index(name)
            if v != self._hp_host[i]:             # (a NaN mirror entry — lr after the controller — always differs)
                self._hp_host[i] = v
                idx.append(i)
        # the learner's by-value attributes follow (set_device_hyper(False) continues from them)
        m = self._hp_host
        self._clip, self._vc = float(m[hip.HP["clip"]]), float(m[hip.HP["value_coeff"]])
        self._cc, self._ec = float(m[hip.HP["clip_coeff"]]), float(m[hip.HP["ent_coeff"]])
        for state, i, field in _HP_LOSS.values():
            vals = getattr(self, state)
            setattr(self, state, vals[:i] + (float(m[field]),) + vals[i + 1:])
        if any(hip.HP["clip"] <= i <= hip.HP["ent_coeff"] for i in idx):
            self._hp_moved = True
        if idx:
            # (fields between two changed ones equal the block's already — lr, which the controller moves, is field 0: it is
            #  inside the span only when it is itself being set)
            self._hp_upload(min(idx), max(idx) + 1)

    def set_adaptive_lr(self, desired_kl, factor=1.5, lr_min=1e-5, lr_max=1e-2, lr=None, consensus=False):
        """KL-adaptive learning rate, on the device (switches to device-hyper mode and implies the stats loss kernel): after
        a minibatch's loss and before its optimiser step, with kl = max(approx_kl steer, approx_kl throttle) of that
        minibatch,  kl > 2 desired_kl: lr = max(lr_min, lr / factor);  0 < kl < desired_kl / 2: lr = min(lr_max, lr * factor)
        (float64; the rsl_rl / RL-Games rule).  The target_kl gate is checked first: once it has fired, lr stays.  `lr`: the
        starting value (None: the block's current one — the adapted value carries over).  While the controller is on,
        clip_adam's `lr` argument is ignored.  set_adaptive_lr(None) switches it off; the next clip_adam(lr=) then sets lr.
        Refused with several ranks (each rank would move its own lr) and by the sharded optimiser step.
        consensus (several ranks, not refused): the block's desired_kl field stays 0, so the loss kernel does not adapt; the
        desired KL is kept on the host and handed by value to cadre_kl_consensus, which applies the same rule to the KL
        summed over the ranks (kl_consensus, run by chief_step before the optimiser step)."""
        if desired_kl is None:
            self._cons_adaptive = False
            self.consensus = self._cons_modes
            if self._adaptive is not None:
                self._adaptive = None
                self._hp_host[hip.HP["desired_kl"]] = 0.0
                self._hp_host[hip.HP["lr"]] = float("nan")      # (the device holds the adapted value: unknown here)
                self._hp_upload(hip.HP["desired_kl"], hip.HP["desired_kl"] + 1)
            return
        desired_kl, factor, lr_min, lr_max = float(desired_kl), float(factor), float(lr_min), float(lr_max)
        if not (desired_kl > 0.0 and np.isfinite(desired_kl)):
            raise ValueError("adaptive lr: desired_kl must be > 0 (got %r)" % (desired_kl,))
        if not (factor > 1.0 and np.isfinite(factor)):
            raise ValueError("adaptive lr: factor must be > 1 (got %r)" % (factor,))
        if not (0.0 < lr_min <= lr_max and np.isfinite(lr_max)):
            raise ValueError("adaptive lr: need 0 < lr_min <= lr_max (got %r, %r)" % (lr_min, lr_max))
        if lr is not None and not (float(lr) > 0.0 and np.isfinite(float(lr))):
            raise ValueError("adaptive lr: lr must be > 0 (got %r)" % (lr,))
        import torch.distributed as dist
        if not consensus and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise hip.CadreHipError("adaptive lr needs a single rank (world size %d): the controller is per rank and every "
                                    "rank would move its own lr" % dist.get_world_size())
        if getattr(self.a, "_shard", None) is not None:
            raise hip.CadreHipError("adaptive lr is not available for the sharded optimiser step (several ranks)")
        self.set_device_hyper(True)
        m = self._hp_host
        lo = hip.HP["desired_kl"]
        if lr is not None:                         # (None: whatever the block holds carries over)
            m[hip.HP["lr"]] = float(lr)
            lo = 0
        m[hip.HP["desired_kl"]], m[hip.HP["lr_factor"]] = (0.0 if consensus else desired_kl), factor
        m[hip.HP["lr_min"]], m[hip.HP["lr_max"]] = lr_min, lr_max
        self._adaptive = (desired_kl, factor, lr_min, lr_max)
        self._cons_adaptive = bool(consensus)
        self.consensus = self._cons_modes or self._cons_adaptive
        self._hp_upload(lo, hip.HP["lr_factor"] + 1)

    def _sync_hyper(self, lr, max_grad_norm):
        """Device-hyper mode: the optimiser step's lr / max_grad_norm arguments against the mirror; a difference becomes one
        set_hyper (a torch lr scheduler on the chief's optimizer just works, at replay speed)."""
        upd = {}
        if float(max_grad_norm) != self._hp_host[hip.HP["max_grad_norm"]]:
            upd["max_grad_norm"] = max_grad_norm
        if self._adaptive is None and float(lr) != self._hp_host[hip.HP["lr"]]:
            upd["lr"] = lr
        if upd:
            self.set_hyper(**upd)

    # ------------------------------------------------------------------ workspace
    def workspace(self, B, Z=None, S=None):
        a = self.a
        Z = a.Z if Z is None else Z
        S = self.S if S is None else S
        key = (B, Z, S)
        w = self._ws.get(key)
        if w is None:
            dev = a.device
            z = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype, device=dev)
            w = dict(
                X=z(2, S, B, a.DP), h0=z(2, B, a.DP), c0=z(2, B, a.DP),
                G=z(Z, S, B, a.H4P), dG=z(Z, S, B, a.H4P),         # gate rows [i f g o] x D, zero padded to 4 x 34 k-blocks
                Hs=z(Z, S + 1, B, a.DP), Cs=z(Z, S + 1, B, a.DP), TC=z(Z, S + 1, B, a.DP),
                A1=z(2 * Z, B, a.hid), A2=z(2 * Z, B, a.hid), O3=z(2 * Z, B, a.NP),
                dO3=z(2 * Z, B, a.NP), dA2=z(2 * Z, B, a.hid), dA1=z(2 * Z, B, a.hid),
                dH=z(Z, B, a.DP), dC=z(Z, B, a.DP), dGp=z(2, Z, (B + 15) // 16, 16 * a.H4P),
                actions=z(2, B, dtype=torch.int64), commands=z(2, B, dtype=torch.int32),
                old_values=z(2, B), returns=z(2, B), old_logp=z(2, B), adv=z(2, B),
                losses=z(3), loss_scratch=z(4 + 6 * ((B + 15) // 16)), sync=z(Z * S + 1, dtype=torch.int32),
                pos=z(2, B, dtype=torch.int32), seg=z(2 * a.C, 2, dtype=torch.int32),
            )
            if self.sorted_rows(B) and Z == a.Z:      # unsorted staging for gather -> sort -> permute
                w.update(Xu=z(2, S, B, a.DP), h0u=z(2, B, a.DP), c0u=z(2, B, a.DP),
                         actions_u=z(2, B, dtype=torch.int64), commands_u=z(2, B, dtype=torch.int32),
                         old_values_u=z(2, B), returns_u=z(2, B), old_logp_u=z(2, B), adv_u=z(2, B))
            self._ws[key] = w
        return w

    # ------------------------------------------------------------------ packed weights
    def packed_weights(self, g0, gs, Z):
        """Fragment-order copies of the recurrent weights of all 8 nets (cadre_pack_lstm_weights), refreshed when the
        parameters changed: the optimiser step count and `params._version` (in-place loads) key the copy.  Returns
        (forward copy of net g0, net stride gs nets)."""
        a = self.a
        key = self._pkey()
        self._alloc_wp()
        capturing = torch.cuda.is_current_stream_capturing()
        if capturing and self.pack_outside_capture:
            return self._wp[0, g0:], gs * self._wp.stride(1)     # (the caller refreshed the copies before the replay)
        if self._skip_pack:                                      # (update() checked: the last optimiser step left them current)
            return self._wp[0, g0:], gs * self._wp.stride(1)
        if key != self._wp_key or capturing:
            hip.check(hip.lib().cadre_pack_lstm_weights(hip.ptr(a.params[a.o_whh:]), a.size_L, a.DP, a.D, a.Z, hip.ptr(self._wp[0]),
                                                        hip.ptr(self._wp[1]), self._wp.stride(1), hip.stream()),
                      "cadre_pack_lstm_weights")
            self._wp_key = None if torch.cuda.is_current_stream_capturing() else key
        return self._wp[0, g0:], gs * self._wp.stride(1)

    def invalidate_parameter_caches(self):
        """The parameters were rewritten behind the optimiser's back (a broadcast, a reset of the step count): forget the
        packed recurrent weights and move `params._version`, which keys every other copy held of them (the stacked arenas
        of an EnsembleEvaluator).  The version moves through an in-place no-op on the arena, as load_snapshot does."""
        self._wp_key = None
        self._adam_fresh = None
        self.a.params[:0].zero_()

    def _pkey(self):
        a = self.a
        return (a.step, a.params._version, a.params.data_ptr())

    def _alloc_wp(self):
        a = self.a
        if self._wp is None:
            n = ((a.D + 15) // 16) * 4 * (a.DP // 16) * 256
            self._wp = torch.zeros(2, a.Z, n, device=a.device)

    # ------------------------------------------------------------------ forward
    def _forward(self, w, B, nets, x_div, S=None, mlp=True, seg=None, fused_mlp=False):
        """LSTM (S steps) + (optionally) both MLP towers for `Z` nets.  nets = (g0, g_stride, Z): arena net
        indices g0 + i*g_stride.  Net i reads inputs X[i // x_div], h0/c0[i // x_div]."""
        a = self.a
        S = self.S if S is None else S
        g0, gs, Z = nets
        P, st = a.params, hip.stream()
        L = hip.lib()
        DP, H4, H4P, hid, NP = a.DP, a.H4, a.H4P, a.hid, a.NP
        pL = P[g0 * a.size_L:]
        sL = gs * a.size_L
        X, G, Hs, Cs, TC = w["X"], w["G"], w["Hs"], w["Cs"], w["TC"]
        # h_{-1}, c_{-1} (hidden_state_batch, agent.py:166-175) into slot 0 of every net; dC <- 0 for the backward
        hip.check(L.cadre_lstm_init(hip.ptr(w["h0"]), hip.ptr(w["c0"]), hip.ptr(Hs), hip.ptr(Cs), hip.ptr(w["dC"]),
                                    B * DP, (S + 1) * B * DP, x_div, Z, st), "cadre_lstm_init")
        # all input projections x_t W_ih^T + b_ih: one GEMM [S*B, DP] x [DP, H4] per net
        sg1 = None if seg is None else (3, seg, B, 1)         # exactly each net's run of rows, step after step (compact M)
        sgp = None if seg is None else hip.ptr(seg)           # fused steps: the same rows
        hip.gemm(X, pL[a.o_wih:], G, S * B, H4, DP, DP, DP, H4P, shift=pL[a.o_bih:], batch=Z,
                 a_z=(x_div, 0, S * B * DP), b_z=(1, 0, sL), c_z=(1, 0, S * B * H4P), s_z=(1, 0, sL), seg=sg1)
        wpf, wps = self.packed_weights(g0, gs, Z)
        if self.persistent_lstm and Z == a.Z and gs == 1 and "sync" in w:
            # all S steps in one persistent launch: weights resident in registers, h_t exchanged through L2
            hip.check(L.cadre_lstm_seq_fwd(hip.ptr(wpf), wps, hip.ptr(pL[a.o_bhh:]), sL, hip.ptr(G), H4P, S * B * H4P, hip.ptr(Hs),
                                           hip.ptr(Cs), hip.ptr(TC), DP, (S + 1) * B * DP, B, a.D, S, Z, sgp, hip.ptr(w["sync"]), st),
                      "cadre_lstm_seq_fwd")
        for t in range(0 if not (self.persistent_lstm and Z == a.Z and gs == 1 and "sync" in w) else S, S):   # models.py:148-151
            # gates = x-projection + h_{t-1} W_hh^T + b_hh, cell math, h_t / c_t / tanh(c_t): one launch for all nets
            hip.check(L.cadre_lstm_step_fwd(hip.ptr(wpf), wps, hip.ptr(pL[a.o_bhh:]), sL, hip.ptr(G[:, t]), H4P,
                                            S * B * H4P, hip.ptr(Hs[:, t]), hip.ptr(Cs[:, t]), hip.ptr(Hs[:, t + 1]),
                                            hip.ptr(Cs[:, t + 1]), hip.ptr(TC[:, t + 1]), DP, (S + 1) * B * DP, B, a.D, Z,
                                            sgp, t & 1, st), "cadre_lstm_step_fwd")
        if mlp:
            self._mlp(w, B, nets, Hs[:, S], (S + 1) * B * DP, seg=seg, fused=fused_mlp)

    def mlp_offs(self):
        """(W1, b1, W2, b2, W3, b3) float offsets inside a tower, as the int32[6] the cadre_mlp_* entry points take."""
        if self._mlp_offs is None:
            import ctypes
            a = self.a
            self._mlp_offs = (ctypes.c_int32 * 6)(a.t_w1, a.t_b1, a.t_w2, a.t_b2, a.t_w3, a.t_b3)
        return self._mlp_offs

    def _mlp(self, w, B, nets, inp, inp_zstride, seg=None, fused=False):
        """actor (tower 0) + critic (tower 1) of each net on `inp` ([Z][B][DP] rows, net stride
        inp_zstride): z = 2*i + tower  (models.py:171-177, distributions.py:34-40)."""
        a = self.a
        g0, gs, Z = nets
        P = a.params
        DP, hid, NP = a.DP, a.hid, a.NP
        pP = P[a.P0 + g0 * a.size_P:]
        sT = a.size_T if gs == 1 else None
        A1, A2, O3 = w["A1"], w["A2"], w["O3"]
        if sT and fused and self.fused_mlp:
            hip.check(hip.lib().cadre_mlp_fwd(hip.ptr(pP), a.size_T, self.mlp_offs(), hip.ptr(inp), DP, inp_zstride, hip.ptr(A1),
                                              hip.ptr(A2), hip.ptr(O3), B, 2 * Z, None if seg is None else hip.ptr(seg), hip.stream()),
                      "cadre_mlp_fwd")
            return
        for tower in ((None,) if sT else (0, 1)):
            if sT:      # contiguous nets: 2Z towers with uniform stride
                pw, zb, nb, div, zs, cs = pP, 0, 2 * Z, 2, a.size_T, 1
            else:       # strided nets (act/get_value): one launch per tower
                pw, zb, nb, div, zs, cs = pP[tower * a.size_T:], tower, Z, 1, gs * a.size_P, 2
            sg = None if (seg is None or not sT) else (1, seg, B, 2)      # z = 2*net + tower
            hip.gemm(inp, pw[a.t_w1:], A1[zb:], B, hid, DP, DP, DP, hid, shift=pw[a.t_b1:], act=1, batch=nb,
                     a_z=(div, 0, inp_zstride), b_z=(1, 0, zs), c_z=(1, 0, cs * B * hid), s_z=(1, 0, zs), seg=sg)
            hip.gemm(A1[zb:], pw[a.t_w2:], A2[zb:], B, hid, hid, hid, hid, hid, shift=pw[a.t_b2:], act=1, batch=nb,
                     a_z=(1, 0, cs * B * hid), b_z=(1, 0, zs), c_z=(1, 0, cs * B * hid), s_z=(1, 0, zs), seg=sg)
            hip.gemm(A2[zb:], pw[a.t_w3:], O3[zb:], B, NP, hid, hid, hid, NP, shift=pw[a.t_b3:], batch=nb,
                     a_z=(1, 0, cs * B * hid), b_z=(1, 0, zs), c_z=(1, 0, cs * B * NP), s_z=(1, 0, zs), seg=sg)

    # ------------------------------------------------------------------ update_policy
    def update(self, B, inv_b, sorted_rows=False, mlp_grads_ready=None, stats_row=None, demo_stats_row=None):
        """Forward + loss + backward for the packed minibatch in workspace(B).  Gradients of all 16
        nets are written (not accumulated) into arena.grads.  Returns the device tensor
        losses[3] = (value_loss*vc, action_loss*cc, ent_loss*ec) (agent.py:226-237).
        The launch sequence has fixed shapes and pointers, so after one eager run it is captured
        into a hipGraph per (B, inv_b) and replayed (launch-bound otherwise: ~2 ms of host time).
        With `mlp_grads_ready` (a callable taking an arena range) the sequence is cut where gradient buckets become
        FINAL, and the callable runs at each cut with that bucket's element range — the data-parallel exchange starts the
        bucket's all-reduce there, beside the kernels that follow (Shared_grad_buffers.reduce_bucket_async):
          after the MLP-tower backward            arena[P0:]            (6 MB)   — beside the backward through time
          after the steer nets' weight gradients  arena[:4 size_L]      (37 MB)  — beside the throttle nets' lstm_dw
        the throttle nets' bucket arena[4 size_L:P0] is final when the step ends (the chief's all_reduce takes it).
        `stats_row` (device float32 [2][stats_fields()], needs set_update_modes(stats=True) or a target_kl): the step's
        diagnostics are copied there after the launch sequence (one device-to-device copy), and the next clip_adam writes its
        per-model gradient norms into the same row.  `demo_stats_row` ("ppo+demo" only; device float32
        [2][>= hip.BC_STATS_FIELDS]) receives the imitation statistics of the demonstration rows; `stats_row` keeps its
        meaning there (the diagnostics of the PPO rows)."""
        a = self.a
        self._check_not_swapped("update")
        m = LOSS_MODES[self.loss_mode]
        if demo_stats_row is not None and self.loss_mode != "ppo+demo":
            raise hip.CadreHipError("update(demo_stats_row=...) needs set_loss('ppo+demo')")
        if m.check:
            getattr(self, m.check)()
        if self.loss_mode == "aux":                      # (the record pass shares the refusal: before anything is enqueued)
            self._table()
        if stats_row is not None and m.ppo and not self._loss_stats():
            raise hip.CadreHipError("update(stats_row=...) needs set_update_modes(stats=True) (or a target_kl)")
        # The packed W_hh copies are current iff this learner's own fused optimiser step produced the parameters that are
        # in the arena now (a chief in another process, a broadcast or a checkpoint load change them behind our back: then
        # the update's graph carries the packing launch, as in round 3).
        self._skip_pack = bool(self.fused_pack and self._adam_fresh is not None and self._adam_fresh == self._pkey())
        try:
            if mlp_grads_ready is None:
                self._run("all", B, inv_b, sorted_rows)
                return self._stats_out(B, stats_row, demo_stats_row)
            half = (a.Z // 2) * a.size_L
            for part, rng in (("front", (a.P0, a.total)), ("mid", (0, half)), ("back", None)):
                self._run(part, B, inv_b, sorted_rows)
                if rng is not None:
                    # the hook's arity is read from its signature — never from a TypeError, which would also swallow one
                    # raised INSIDE the hook (a failed collective on this rank only: its peers would wait for ever)
                    if self._hook_takes_range(mlp_grads_ready):
                        mlp_grads_ready(*rng)
                    elif part == "front":                    # (a round-3 style hook without arguments: the MLP bucket only)
                        mlp_grads_ready()
            return self._stats_out(B, stats_row, demo_stats_row)
        finally:
            self._skip_pack = False                          # (act / get_value outside an update always check the copies)

    def _stats_out(self, B, stats_row, demo_stats_row=None):
        w = self.workspace(B)
        if demo_stats_row is not None:
            demo_stats_row[:, :hip.BC_STATS_FIELDS].copy_(w["demo_stats"])
        m = LOSS_MODES[self.loss_mode]
        if m.own_stats:                       # the mode's own statistics (imitation, auxiliary); no gradient norms follow
            if stats_row is not None:
                stats_row[:, :m.own_stats[1]].copy_(w[m.own_stats[0]])
            return w["losses"]
        self._last_stats = w.get("stats")
        if m.last_stats:
            setattr(self, m.last_stats[0], w.get(m.last_stats[1]))
        if stats_row is not None:
            stats_row.copy_(w["stats"])
            self._norm_row = stats_row
        return w["losses"]

    def _stats_ws(self, w, B):
        if "stats" not in w:
            w["stats"] = torch.zeros(2, self.stats_fields(), device=self.a.device)
            w["stats_scratch"] = torch.zeros(12 * ((B + 15) // 16), device=self.a.device)
        return w["stats"], w["stats_scratch"]

    @staticmethod
    def _hook_takes_range(hook):
        import inspect
        try:
            ps = [q for q in inspect.signature(hook).parameters.values()]
        except (TypeError, ValueError):
            return True
        if any(q.kind == q.VAR_POSITIONAL for q in ps):
            return True
        return sum(q.kind in (q.POSITIONAL_ONLY, q.POSITIONAL_OR_KEYWORD) for q in ps) >= 1

    def _run(self, part, B, inv_b, sorted_rows):
        if not self.use_graphs:
            return self._update_body(B, inv_b, sorted_rows, part)
        key = (part, B, inv_b, sorted_rows, self._skip_pack) + self._mode_key()
        g = self._graphs.get(key)
        if g is None:
            n0 = hip.N_CALLS
            self._update_body(B, inv_b, sorted_rows, part)          # eager warm-up (func attributes, lazy init)
            self.launches[(part, B)] = hip.N_CALLS - n0             # kernel launches of this part of the step (latest variant)
            if self._graphs.get(("warm",) + key):
                torch.cuda.synchronize()
                self._graphs[key] = self._capture(lambda: self._update_body(B, inv_b, sorted_rows, part))
            else:
                self._graphs[("warm",) + key] = True
            return
        g.replay()

    @staticmethod
    def _capture(fn):
        """Capture fn() into a hipGraph.  The cyclic garbage collector is held off for the duration:
        a finaliser that runs inside the capture window (an older agent's graphs or tensors being
        destroyed) issues HIP calls that are illegal while the stream is capturing and aborts the
        process from a destructor."""
        import gc
        g = torch.cuda.CUDAGraph()
        was = gc.isenabled()
        gc.collect()
        gc.disable()
        try:
            with torch.cuda.graph(g, capture_error_mode="thread_local"):
                fn()
        finally:
            if was:
                gc.enable()
        return g

    def _ppo_launch(self, w, B, inv_b, sorted_rows=False):
        """The PPO-loss launch of the plain, stats, device-hyper and ordinal modes: entry point and arguments from the flags.
        cadre_ppo_loss[_stats][_hp] take the block OR the four scalars, and the stats arguments only as `_stats`;
        cadre_ppo_loss_ord takes all of them (hp NULL = by-value scalars, stats row NULL = no diagnostics) and the rank table."""
        hp, stats, ord_t = self._hp_on, self._loss_stats(), self._ord()
        ordinal = ord_t is not None
        name = "cadre_ppo_loss_ord" if ordinal else "cadre_ppo_loss%s%s" % ("_stats" if stats else "", "_hp" if hp else "")
        scal = self._scalar_args(B, inv_b)               # (B, C, K0, K1 | block | clip, vc, cc, ec | inv_b)
        args = self._row_args(w, B) + scal[:4]
        if hp or ordinal:
            args += scal[4:5]
        if ordinal or not hp:
            args += scal[5:9]
        args += (inv_b, hip.ptr(w["losses"])) + self._grad_args(w)
        if stats or ordinal:
            args += self._stats_args(w, B)
        if ordinal:
            args += (hip.ptr(ord_t),)
        hip.check(getattr(hip.lib(), name)(*args, hip.stream()), name)

    def _update_body(self, B, inv_b, sorted_rows=False, part="all"):
        """part: "all", or the three cuts of the same launch sequence: "front" (forward, loss, MLP-tower backward, dh_S),
        "mid" (backward through time + the weight gradients of the steer nets, arena nets 0 .. Z/2 - 1), "back" (the weight
        gradients of the throttle nets)."""
        a, S = self.a, self.S
        w = self.workspace(B)
        Z, C = a.Z, a.C
        L, st = hip.lib(), hip.stream()
        DP, H4, hid, NP = a.DP, a.H4, a.hid, a.NP
        seg = w["seg"] if sorted_rows else None         # rows sorted by command: skip tiles a net does not own
        cmd = hip.ptr(w["commands"]) if sorted_rows else None
        sgM1 = None if seg is None else (1, seg, B, 1)  # M tiles, z = net
        sgM2 = None if seg is None else (1, seg, B, 2)  # M tiles, z = 2*net + tower
        sgK1 = None if seg is None else (2, seg, B, 1)  # k tiles (rows), z = net
        sgK2 = None if seg is None else (2, seg, B, 2)
        front, back = part in ("all", "front"), part in ("all", "mid", "back")
        O3, dO3 = w["O3"], w["dO3"]
        if front:
            self._forward(w, B, (0, 1, Z), C, seg=seg, fused_mlp=True)
        if front:   # the selected loss writes losses and dO3 (one launch, two with a row split to place): the rest is indifferent
            getattr(self, LOSS_MODES[self.loss_mode].launch)(w, B, inv_b, sorted_rows)
        # ---------------- backward: MLP towers (16 = 2Z batched)
        Gr = a.grads
        pP, gP = a.params[a.P0:], Gr[a.P0:]
        sT, nb = a.size_T, 2 * Z
        A1, A2, dA1, dA2 = w["A1"], w["A2"], w["dA1"], w["dA2"]
        Hs = w["Hs"]
        zT = (1, 0, sT)

        def layer_bwd(dY, n_y, Xin, ldx_, n_x, x_z, o_w, o_b, dX):
            # dW = dY^T X ; db = colsum(dY) ; dX = dY W
            hip.gemm(dY, Xin, gP[o_w:], n_y, n_x, B, n_y, ldx_, n_x, a_mode=1, b_mode=1, batch=nb,
                     a_z=(1, 0, B * n_y), b_z=x_z, c_z=zT, seg=sgK2)
            hip.check(L.cadre_colsum(hip.ptr(dY), n_y, B * n_y, hip.ptr(gP[o_b:]), sT, B, n_y, nb, 0, st), "cadre_colsum")
            if dX is not None:
                hip.gemm(dY, pP[o_w:], dX, B, n_x, n_y, n_y, n_x, n_x, b_mode=1, batch=nb,
                         a_z=(1, 0, B * n_y), b_z=zT, c_z=(1, 0, B * n_x), seg=sgM2)

        dH, dC = w["dH"], w["dC"]
        if front and self.fused_mlp:
            sgq = None if seg is None else hip.ptr(seg)
            hip.check(L.cadre_mlp_bwd(hip.ptr(pP), sT, self.mlp_offs(), hip.ptr(dO3), hip.ptr(A1), hip.ptr(A2), hip.ptr(dA1), hip.ptr(dA2),
                                      hip.ptr(dH), DP, B * DP, B, nb, sgq, st), "cadre_mlp_bwd")
            hip.check(L.cadre_mlp_dw(hip.ptr(dO3), hip.ptr(dA2), hip.ptr(dA1), hip.ptr(A2), hip.ptr(A1), hip.ptr(Hs[:, S]), DP,
                                     (S + 1) * B * DP, hip.ptr(gP), sT, self.mlp_offs(), B, nb, sgq, st), "cadre_mlp_dw")
        elif front:
            layer_bwd(dO3, NP, A2, hid, hid, (1, 0, B * hid), a.t_w3, a.t_b3, dA2)
            hip.check(L.cadre_relu_bwd(hip.ptr(A2), hip.ptr(dA2), nb * B * hid, cmd, B, hid, C, st), "cadre_relu_bwd")
            layer_bwd(dA2, hid, A1, hid, hid, (1, 0, B * hid), a.t_w2, a.t_b2, dA1)
            hip.check(L.cadre_relu_bwd(hip.ptr(A1), hip.ptr(dA1), nb * B * hid, cmd, B, hid, C, st), "cadre_relu_bwd")
            layer_bwd(dA1, hid, Hs[:, S], DP, DP, (2, 0, (S + 1) * B * DP), a.t_w1, a.t_b1, None)
            # dh_S = dZ1_actor W1_actor + dZ1_critic W1_critic   (two launches, second accumulates)
            for tower in (0, 1):
                hip.gemm(dA1[tower:], pP[tower * sT + a.t_w1:], dH, B, DP, hid, hid, DP, DP, b_mode=1, batch=Z,
                         a_z=(1, 0, 2 * B * hid), b_z=(1, 0, a.size_P), c_z=(1, 0, B * DP),
                         resid=dH if tower else None, ldr=DP, r_z=(1, 0, B * DP), seg=sgM1)
        if not back:
            return w["losses"]
        # ---------------- backward through time (autograd of models.py:148-151)
        G, dG, Cs, TC, X = w["G"], w["dG"], w["Cs"], w["TC"], w["X"]
        pL, gL, sL = a.params, Gr, a.size_L
        H4P = a.H4P
        sgp = None if seg is None else hip.ptr(seg)
        dGp = w["dGp"]                                      # dG of a step in fragment order: ping-pong pair
        gps = dGp.stride(1)
        if part != "back":
            for t in range(S, 0, -1):
                # t == S: dh_{S-1} = dH (MLP towers), no product; else dh_{t-1} = dG_t W_hh.  Then the cell backward of step
                # t-1 in the same launch: dG_{t-1} (row-major for the weight gradients, fragment order for the next step), dc_{t-2}
                src = None if t == S else hip.ptr(dGp[t & 1])
                hip.check(L.cadre_lstm_step_bwd(hip.ptr(self._wp[1]), self._wp[1].stride(0), src, hip.ptr(dGp[(t - 1) & 1]), gps,
                                                hip.ptr(dG[:, t - 1]), hip.ptr(G[:, t - 1]), H4P, S * B * H4P,
                                                hip.ptr(dH) if t == S else None, hip.ptr(dC), B * DP, hip.ptr(TC[:, t]),
                                                hip.ptr(Cs[:, t - 1]), DP, (S + 1) * B * DP, B, a.D, Z, cmd, C, sgp, t & 1, st),
                          "cadre_lstm_step_bwd")
        # dW_hh = sum_t dG_t^T h_{t-1} ; dW_ih = sum_t dG_t^T x_t ; db_ih = db_hh = colsum(dG): one launch for all nets, or —
        # when the exchange overlaps — one per head: nets [z0, z0 + nz) of the arena (X: one input block per head, x_div = C)
        z0, nz = {"all": (0, Z), "mid": (0, Z // 2), "back": (Z // 2, Z - Z // 2)}[part]
        gz = gL[z0 * sL:]
        hip.check(L.cadre_lstm_dw(hip.ptr(dG[z0:]), H4P, S * B * H4P, hip.ptr(Hs[z0:]), hip.ptr(X[z0 // C:]), DP, (S + 1) * B * DP,
                                  S * B * DP, C, hip.ptr(gz[a.o_whh:]), hip.ptr(gz[a.o_wih:]), hip.ptr(gz[a.o_bih:]),
                                  hip.ptr(gz[a.o_bhh:]), DP, sL, B, S, H4, DP, nz, None if seg is None else hip.ptr(seg[z0:]), st),
                  "cadre_lstm_dw")
        return w["losses"]

    # ------------------------------------------------------------------ optimiser (chief.py:13-21)
    def clip_adam(self, lr=3e-4, max_grad_norm=250.0, betas=(0.9, 0.999), eps=1e-8):
        """Three launches (prep, per-model square norms, Adam) with the step count in device memory,
        captured into a hipGraph per hyper-parameter set."""
        a = self.a
        self._check_not_swapped("clip_adam")
        a.ensure_adam()
        a.step += 1                 # (with the KL gate armed: steps attempted — the learner section reconciles it at its sync)
        fused = self.fused_pack
        gated = self.target_kl is not None
        hp = self._hp_on
        b1, b2, eps = float(betas[0]), float(betas[1]), float(eps)
        if hp:      # lr and max_grad_norm live in the block: a new value is a copy, not a new graph
            self._sync_hyper(lr, max_grad_norm)
            key = ("adam", "hp", b1, b2, eps, fused) + (("gated",) if gated else ())
        else:
            key = ("adam", float(lr), float(max_grad_norm), b1, b2, eps, fused) + (("gated",) if gated else ())
        avg = self._avg
        if avg is not None:         # (the average's buffers are baked into the graph: their addresses are the key's one more element)
            key = key + (("ema", avg.ema.data_ptr(), avg.state.data_ptr(), avg.work.data_ptr()),)
        if fused:
            self._alloc_wp()

        def body():
            # cadre_clip_adam_[pack_]graph[_hp][_gated]: the block stands where max_norm and lr stand by value
            L = hip.lib()
            scal = (hip.ptr(self._hp),) if hp else (float(max_grad_norm), float(lr))
            head = (hip.ptr(a.params), hip.ptr(a.grads), hip.ptr(a.exp_avg), hip.ptr(a.exp_avg_sq), hip.ptr(a.seg_off),
                    2 * a.Z, hip.ptr(a.norms2)) + scal + (b1, b2, eps, hip.ptr(a.step_dev))
            pack = (a.Z, a.size_L, a.o_whh, a.H4, a.DP, a.D, hip.ptr(self._wp[0]), hip.ptr(self._wp[1]),
                    self._wp.stride(1)) if fused else ()
            tail = ((hip.ptr(self._stop),) if gated else ()) + (hip.stream(),)
            name = "cadre_clip_adam_%sgraph%s%s" % ("pack_" if fused else "", "_hp" if hp else "", "_gated" if gated else "")
            hip.check(getattr(L, name)(*(head + pack + tail)), name)
            if avg is not None:     # cadre_ema_update behind the step, under the same flag as the gated twin
                avg.update(stop=self._stop if gated else None)

        def done():
            self._adam_fresh = self._pkey() if fused else None      # (the copies now match the stepped parameters)
            self._wp_key = self._adam_fresh if fused else self._wp_key
            self._write_norms()
        if not self.use_graphs:
            body()
            return done()
        g = self._graphs.get(key)
        if g is None:
            if self._graphs.get(("warm",) + key):
                torch.cuda.synchronize()
                g = self._capture(body)
                self._graphs[key] = g
                g.replay()
                return done()
            self._graphs[("warm",) + key] = True
            body()
            return done()
        g.replay()
        done()

    def clip_adam_sharded(self, lo, hi, all_reduce_norms, lr=3e-4, max_grad_norm=250.0, betas=(0.9, 0.999), eps=1e-8):
        """The same step on arena elements [lo, hi) only (data-parallel ranks after a reduce-scatter of the
        gradient arena, chief.py:13-21 semantics): partial per-model square norms of the shard ->
        `all_reduce_norms(norms2[:n_models])` (SUM of 16 doubles over the ranks) -> clip + Adam on the shard.
        The Adam moments exist for the shard only (1/N of the state and of the pass's HBM traffic)."""
        a = self.a
        self._check_not_swapped("clip_adam_sharded")
        if self._avg is not None:
            raise hip.CadreHipError("a weight average is not available for the sharded optimiser step: it steps one shard of the "
                                    "arena per rank (set_weight_average(None), or the all-reduce exchange)")
        if self.consensus:
            raise hip.CadreHipError("rank consensus is not available for the sharded optimiser step: it has no gated form "
                                    "(use the all-reduce exchange)")
        if self.target_kl is not None:
            raise hip.CadreHipError("target_kl: the KL gate is not available for the sharded optimiser step (several ranks)")
        if self._adaptive is not None:
            raise hip.CadreHipError("adaptive lr is not available for the sharded optimiser step (several ranks: each rank "
                                    "would move its own lr)")
        if getattr(a, "_shard", None) != (lo, hi):
            if a.step:
                raise hip.CadreHipError("the optimiser shard changed after %d steps (Adam state is per shard)" % a.step)
            a._shard = (lo, hi)
            a.exp_avg = torch.zeros(hi - lo, device=a.device)
            a.exp_avg_sq = torch.zeros(hi - lo, device=a.device)
        a.step += 1
        L, st, nm = hip.lib(), hip.stream(), 2 * a.Z
        hp, b1, b2 = self._hp_on, float(betas[0]), float(betas[1])
        if hp:      # the `_hp` pair: the block stands where lr (norms) and max_norm (apply) stand by value
            self._sync_hyper(lr, max_grad_norm)
        sfx = "_hp" if hp else ""
        lr_arg, norm_arg = (hip.ptr(self._hp), hip.ptr(self._hp)) if hp else (float(lr), float(max_grad_norm))
        hip.check(getattr(L, "cadre_clip_adam_norms" + sfx)(
            hip.ptr(a.grads), hip.ptr(a.seg_off), nm, hip.ptr(a.norms2), lr_arg, b1, b2, hip.ptr(a.step_dev), lo, hi, st),
            "cadre_clip_adam_norms" + sfx)
        all_reduce_norms(a.norms2[:nm])
        hip.check(getattr(L, "cadre_clip_adam_apply" + sfx)(
            hip.ptr(a.params), hip.ptr(a.grads), hip.ptr(a.exp_avg), hip.ptr(a.exp_avg_sq), hip.ptr(a.seg_off), nm,
            hip.ptr(a.norms2), norm_arg, b1, b2, float(eps), lo, hi, st), "cadre_clip_adam_apply" + sfx)
        self._write_norms()

    def _write_norms(self):
        """The per-model gradient norms of the optimiser step just enqueued into the pending stats row (one launch after
        the step's graph; nothing read on the host)."""
        row, self._norm_row = self._norm_row, None
        if row is not None:      # (`_hp`: also the learning rate the step used, field hip.PPO_STATS_LR of head 0)
            name = "cadre_grad_norms_hp" if self._hp_on else "cadre_grad_norms"
            blk = (hip.ptr(self._hp),) if self._hp_on else ()
            hip.check(getattr(hip.lib(), name)(hip.ptr(self.a.norms2), self.a.C, hip.ptr(row), row.shape[-1], *blk, hip.stream()), name)

    # ------------------------------------------------------------------ inference (act / get_value)
    def infer(self, feats, commands, h0=None, c0=None):
        """LSTM + both towers of net (steer, commands[0]) and (throttle, commands[1]) at batch 1.
        feats: [2][S][DP-padded] views or one shared [S][D] feature block.  Returns (O3 [4][1][NP]:
        rows (steer actor, steer critic, throttle actor, throttle critic))."""
        a, S = self.a, feats.shape[-2]
        w = self.workspace(1, 2, S)
        X = w["X"]
        if feats.dim() == 2:
            X[:, :, 0, :a.D].copy_(feats.unsqueeze(0).expand(2, S, a.D))
        else:
            X[:, :, 0, :a.D].copy_(feats)
        if h0 is None:
            w["h0"].zero_(); w["c0"].zero_()
        else:
            w["h0"][:, 0, :a.D].copy_(h0); w["c0"][:, 0, :a.D].copy_(c0)
        g_s, g_t = commands[0], a.C + commands[1]
        self._forward(w, 1, (g_s, g_t - g_s, 2), 1, S=S)
        return w["O3"], w["Hs"][:, S], w["Cs"][:, S]

    def infer_rows(self, feats):
        """LSTM + both towers of ALL command nets of both heads on W independent rows in one pass (zero initial
        state, agent.py:38-40): feats [2][W][S][D] (head, row).  Returns O3 [4*C][W][NP] (tower z = 2*net + t,
        net = head*C + c) — the caller picks each row's command.  One launch chain instead of W (get_value for every
        worker of a GPU, train.py:76-80)."""
        a, W, S = self.a, feats.shape[1], feats.shape[2]
        w = self.workspace(W, a.Z, S)
        w["X"].view(2, S, W, a.DP)[:, :, :, :a.D].copy_(feats.permute(0, 2, 1, 3))
        w["h0"].zero_(); w["c0"].zero_()
        self._forward(w, W, (0, 1, a.Z), a.C, S=S)
        return w["O3"]

    # ------------------------------------------------------------------ stand-alone module calls
    def lstm_module_forward(self, g, x, h0, c0):
        """`LSTM.forward` (models.py:139-152) of arena net g: x [T*N, D] time-major (or [N, D]), hidden
        [N, D] -> (h_T, c_T) [N, D].  Inference only."""
        a = self.a
        N = h0.shape[0]
        S = x.shape[0] // N
        w = self.workspace(N, 1, S)
        w["X"][0].view(S * N, a.DP)[:, :a.D].copy_(x)
        w["h0"][0][:, :a.D].copy_(h0)
        w["c0"][0][:, :a.D].copy_(c0)
        self._forward(w, N, (g, 1, 1), 1, S=S, mlp=False)
        return w["Hs"][0, S, :, :a.D].clone(), w["Cs"][0, S, :, :a.D].clone()

    def mlp_module_forward(self, g, feat):
        """critic + actor of arena net g on feat [B, D] -> (raw logits [B, NP], values [B, 1]) views."""
        a = self.a
        B = feat.shape[0]
        w = self.workspace(B, 1, 1)
        inp = w["Hs"][0, 1]
        inp[:, :a.D].copy_(feat)
        self._mlp(w, B, (g, 1, 1), w["Hs"][:, 1], 2 * B * a.DP)
        return w["O3"][0], w["O3"][1, :, :1]
