"""Mirror of reference ppo_agent/agent.py `CadreAgent`: same constructor, attributes and
method contracts (act / get_value / update_policy / update_model / convert_action / avg_action /
save_snapshot / load_snapshot), every tensor op on HIP kernels via cadre_amd.encoder and
cadre_amd.learner."""
import os

import numpy as np
import torch

from .. import hip
from ..learner import LOSS_MODES, PPOLearnerHIP
from .models import LSTM, Model, _cfg, arena_of, create_model, get_vae_output, ordinal_rank, resolve_ordinal  # noqa: F401


def command_rows(commands, command_num):
    """Rows of an act_batch pass sorted by command (stable: environments of one command keep their order).  Returns
    pos int32 [N] (the sorted row of environment e) and seg int32 [2 * command_num][2]: (first row, count) of net
    head * command_num + c — the row_seg the LSTM / MLP kernels take; a command without rows has count 0."""
    cmd = np.asarray(commands, dtype=np.int64).reshape(-1)
    if cmd.size < 1:
        raise ValueError("command_rows: no environments")
    if (cmd < 0).any() or (cmd >= command_num).any():
        raise ValueError("command_rows: commands %s outside 0 .. %d" % (cmd.tolist(), command_num - 1))
    counts = np.bincount(cmd, minlength=command_num)
    first = np.concatenate([[0], np.cumsum(counts)[:-1]])
    pos = np.empty(cmd.size, dtype=np.int32)
    pos[np.argsort(cmd, kind="stable")] = np.arange(cmd.size, dtype=np.int32)
    seg = np.tile(np.stack([first, counts], 1), (2, 1)).astype(np.int32)
    return pos, seg


def check_act_batch(obs_list, shifted, max_envs, device, vae_device, command_num):
    """Arguments of CadreAgent.act_batch, checked before any device work; raises hip.CadreHipError."""
    if vae_device != device:
        raise hip.CadreHipError("act_batch: the encoder (vae_device %s) and the nets (device_num %s) must share one GPU; "
                                "call act() per environment" % (vae_device, device))
    N = len(obs_list)
    if N < 1 or N > max_envs:
        raise hip.CadreHipError("act_batch: %d environments; 1 .. model_cfg.max_envs = %d per call" % (N, max_envs))
    if shifted is not None and len(shifted) != N:
        raise hip.CadreHipError("act_batch: %d `shifted` hints for %d environments" % (len(shifted), N))
    ref = obs_list[0]
    S = ref["rgb"].shape[0]
    want = (tuple(ref["rgb"].shape), tuple(ref["route_fig"].shape), (S, 3))
    for e, td in enumerate(obs_list):
        got = (tuple(td["rgb"].shape), tuple(td["route_fig"].shape), tuple(np.shape(td["measurements"])))
        if got != want or td["rgb"].dtype != np.uint8 or td["route_fig"].dtype != np.uint8:
            raise hip.CadreHipError("act_batch: observation %d has shapes rgb %s / route_fig %s / measurements %s (dtypes %s, "
                                    "%s); environment 0 has %s / %s / %s, uint8" % ((e,) + got + (td["rgb"].dtype,
                                                                                   td["route_fig"].dtype) + want))
        c = int(td["command"])
        if not 0 <= c < command_num:
            raise hip.CadreHipError("act_batch: observation %d has command %d; 0 .. %d" % (e, c, command_num - 1))


class ActBatch(list):
    """act_batch's return value: the list of N act() tuples, plus the device buffers they are views of (feat [N][S][DP],
    action i64 / logp / value f32 [N][2]) for RolloutStorage.insert_batch."""


class CadreAgent(object):
    def __init__(self, rank, model_cfg, frame, STEER_CONTROL, THROTTLE_CONTROL, ent_coeff, value_coeff, clip_coeff,
                 clip):
        self.rank = rank
        # ordinal policy heads (model_cfg["ordinal_policy"], opt-in): True orders a head by its control table; create_model
        # then gets the explicit permutations.  Absent / None / False: model_cfg goes through untouched.
        spec = _cfg(model_cfg, "ordinal_policy")
        if spec is not None and spec is not False:
            ranks = resolve_ordinal(spec, _cfg(model_cfg, "num_output"), {"steer": STEER_CONTROL, "throttle": THROTTLE_CONTROL})
            model_cfg = dict(model_cfg)
            model_cfg["ordinal_policy"] = None if ranks is None else {h: (False if r is None else r)
                                                                       for h, r in zip(("steer", "throttle"), ranks)}
        self.vae_model, self.model_dict = create_model(model_cfg, load_vae=True)
        self.use_lstm = _cfg(model_cfg, "use_lstm")
        self.command_num = _cfg(model_cfg, "command_num")
        self.device = torch.device("cuda:" + str(_cfg(model_cfg, "device_num")))
        self.vae_device = torch.device("cuda:" + str(_cfg(model_cfg, "vae_device")))
        self.STEER_CONTROL = STEER_CONTROL
        self.THROTTLE_CONTROL = THROTTLE_CONTROL
        self.ent_coeff, self.value_coeff, self.clip_coeff, self.clip = ent_coeff, value_coeff, clip_coeff, clip
        self.lstm_input, self.vae_params = get_vae_output(model_cfg)
        self.use_vae = True
        self.frame = frame
        self.pre_latent_feature = None
        self.hidden_state = (torch.zeros(1, self.lstm_input, device=self.device),
                             torch.zeros(1, self.lstm_input, device=self.device))
        self.arena = arena_of(self.model_dict)
        self.ordinal_rank = self.arena.ordinal_rank     # host copy: [steer, throttle] rank lists (None: categorical), or None
        self.learner = PPOLearnerHIP(self.arena, clip, value_coeff, clip_coeff, ent_coeff, seq_length=frame)
        self.arena._learner = self.learner
        self.mutate_route = _cfg(model_cfg, "mutate_route", True)
        self.latent_cache = _cfg(model_cfg, "latent_cache", True)
        self._cache = None
        # act() as one hipGraph per (window mode, command): ~150 launches of an env step replayed in one submission.
        # Opt-in (model_cfg.act_graph / CADRE_ACT_GRAPH=1): measured at 144x256 the env step is bound by the DEVICE time of
        # the one-frame launch chain, not by its host-side issue — 1.85 ms replayed vs 1.88 ms eager (tools/act_latency.py)
        import os
        self.act_graph = bool(_cfg(model_cfg, "act_graph", os.environ.get("CADRE_ACT_GRAPH", "0") != "0"))
        self._ag = None
        # act_batch(): at most `max_envs` environments per call (sizes the device ring of their latent windows)
        self.max_envs = int(_cfg(model_cfg, "max_envs", 32))
        self._vec = None
        self._decoder = None        # DANetDecoderHIP, built by the first decode / bc_controls / light_state call

    # ------------------------------------------------------------------ decoder branches (danet.py:164-361)
    def decoder(self):
        """The encoder checkpoint's decoder branches (cadre_amd/decoder.py), built on first use from the state create_model loaded."""
        if self._decoder is None:
            from ..decoder import DANetDecoderHIP
            state = getattr(self.vae_model, "source_state", None)
            if state is None:
                raise hip.CadreHipError("this agent's encoder keeps no checkpoint state to build the decoder from")
            self._decoder = DANetDecoderHIP(state, self.device)
        return self._decoder

    def decode(self, tick_data_or_latents, speed=None, want=("seg", "route", "light", "bc"), seg_logits=False):
        """DANetDecoderHIP.decode of an observation's window (a tick_data dict: its frames go through get_latent_feature) or of
        latent rows already on the device (storage rows, a FrameStorage table)."""
        x = tick_data_or_latents
        lat = self.get_latent_feature(x) if isinstance(x, dict) else x
        return self.decoder().decode(lat, speed=speed, want=want, seg_logits=seg_logits)

    def bc_controls(self, tick_data, speed=None):
        """danet.py:265-291 get_bc_actions -> (steer [S], throttle [S]): the controls the perception module was trained to predict."""
        bc = self.decode(tick_data, speed=speed, want=("bc",)).bc
        return bc[:, 0], bc[:, 1]

    def light_state(self, tick_data):
        """danet.py:334-361 get_light_state -> the 0 .. 3 traffic-light class of the window's first frame (a 0-d device tensor)."""
        return self.decode(tick_data, want=("light",)).light_state[0]

    # ------------------------------------------------------------------ observation -> feature
    def pre_process(self, tick_data, first=0):
        """agent.py:43-75 on device; returns the NHWC f32 tensor [S-first,H,W,4] (the reference returns
        NCHW numpy — same values, channels-last) and applies the in-place uint8 route quirk."""
        rgb = torch.from_numpy(np.ascontiguousarray(tick_data["rgb"][first:])).to(self.vae_device, non_blocking=True)
        route_np = tick_data["route_fig"]
        route = torch.from_numpy(np.ascontiguousarray(route_np[first:])).to(self.vae_device, non_blocking=True)
        rn = torch.empty_like(route) if self.mutate_route else None
        x = self.vae_model.preprocess(rgb, route, rn)
        if rn is not None:
            route_np[first:] = rn.cpu().numpy()         # agent.py:51-54 mutates the caller's dict
        return x

    def _window_shifted(self, tick_data):
        """True when frames 0..S-2 of this observation are frames 1..S-1 of the previous one (the env's
        sliding window, env_wrapper.py:899-904) — then only the newest frame needs encoding."""
        c = self._cache
        if c is None or not self.latent_cache:
            return False
        rgb, route = tick_data["rgb"], tick_data["route_fig"]
        if rgb.shape != c["rgb"].shape or route.shape != c["route_raw"].shape:
            return False
        if not np.array_equal(rgb[:-1], c["rgb"][1:]):
            return False
        return np.array_equal(route[:-1], c["route_raw"][1:]) or np.array_equal(route[:-1], c["route_norm"][1:])

    def get_latent_feature(self, tick_data):
        """agent.py:97-112 -> [S, 530] f32 device tensor (a view of a 544-pitch row buffer).
        Sliding-window latent cache: the encoder is per-frame in eval mode and the
        HIP kernels are batch-invariant bit for bit (tests/test_encoder_gpu.py), so re-using the 7
        latents already computed for the previous step changes no output bit and saves 7/8 of the
        encoder work the reference repeats."""
        S = tick_data["rgb"].shape[0]
        feat = torch.zeros(S, self.arena.DP, device=self.device)   # fresh rows: callers keep references
        shifted = self._window_shifted(tick_data)
        raw_rgb = tick_data["rgb"].copy() if self.latent_cache else None
        raw_route = tick_data["route_fig"].copy() if self.latent_cache else None
        if shifted:
            x = self.pre_process(tick_data, first=S - 1)
            if self.mutate_route:
                tick_data["route_fig"][:-1] = self._cache["route_norm"][1:]
            feat[:-1, :512].copy_(self._cache["latent"][1:])
            self.vae_model.forward_nhwc(x, feat[S - 1:])
        else:
            x = self.pre_process(tick_data)
            self.vae_model.forward_nhwc(x, feat)
        if self.latent_cache:
            self._cache = dict(rgb=raw_rgb, route_raw=raw_route, route_norm=tick_data["route_fig"].copy(),
                               latent=feat[:, :512].clone())
        meas = torch.from_numpy(np.ascontiguousarray(tick_data["measurements"], dtype=np.float64)).to(self.device)
        hip.check(hip.lib().cadre_append_measurements(hip.ptr(meas), hip.ptr(feat), feat.stride(0), S, hip.stream()),
                  "cadre_append_measurements")
        return feat[:, :self.lstm_input]

    # ------------------------------------------------------------------ act
    def _sample(self, O3, tower_row, K, q_host, allowed=None):
        q = q_host.to(self.device, non_blocking=True)
        action = torch.empty(1, dtype=torch.int64, device=self.device)
        logp = torch.empty(1, 1, device=self.device)
        self._sample_launch(O3, tower_row, K, q, action, logp, allowed)
        return action, logp

    def _am_ord(self):
        """The rank tables the `_am` samplers want: the arena's, or a marker table of two categorical heads."""
        ord_t = self.arena.ord
        return self.learner.marker_ord() if ord_t is None else ord_t

    def _sample_launch(self, O3, tower_row, K, q, action, logp, allowed=None):
        """cadre_sample on actor-tower row `tower_row` of O3 (0 steer, 2 throttle), or cadre_sample_ord with the head's rank
        table when the agent has ordinal heads; with `allowed` (a device int64 tensor of one word) cadre_sample_am."""
        L, ord_t = hip.lib(), self.arena.ord
        if allowed is not None:
            hip.check(L.cadre_sample_am(hip.ptr(O3[tower_row]), O3.shape[-1], hip.ptr(q), K, 1, K, hip.ptr(action), hip.ptr(logp),
                                        hip.ptr(self._am_ord()[tower_row // 2]), hip.ptr(allowed), hip.stream()), "cadre_sample_am")
        elif ord_t is not None:
            hip.check(L.cadre_sample_ord(hip.ptr(O3[tower_row]), O3.shape[-1], hip.ptr(q), K, 1, K, hip.ptr(action),
                                         hip.ptr(logp), hip.ptr(ord_t[tower_row // 2]), hip.stream()), "cadre_sample_ord")
        else:
            hip.check(L.cadre_sample(hip.ptr(O3[tower_row]), O3.shape[-1], hip.ptr(q), K, 1, K, hip.ptr(action),
                                     hip.ptr(logp), hip.stream()), "cadre_sample")

    def act(self, tick_data, deterministic=False, allowed=None):
        """agent.py:114-141.  Sampling consumes the global torch CPU generator exactly like the
        reference (one exponential_(1) draw of n_out floats per head, steer first).  The launch chain of an
        env step (packing, encoder, LSTM x 2, heads, sampling: ~150 kernels) has fixed shapes and pointers, so
        it is captured once per (window mode, command) into a hipGraph and replayed — same kernels, same order,
        same results; inputs and outputs go through static buffers.
        `deterministic=True`: the greedy action (the first largest probability) — the sampler's q is all ones (p / 1.0f is
        exact), nothing is drawn from the generator.
        `allowed` (action masks, cadre_amd.actmask): a (steer_word, throttle_word) pair of Python ints (bit k set: bin k may be
        chosen; an empty set is refused) or a device int64 [1][2] tensor.  The action is then argmax(p / q) over the allowed
        bins, the log-probability the masked one; the generator is consumed exactly as without (q is drawn for all bins).
        None launches exactly what is launched without the feature."""
        if allowed is not None:
            from ..actmask import words_tensor
            allowed = words_tensor([allowed] if not torch.is_tensor(allowed) else allowed, 1, self.arena.n_out, self.device).view(2)
        if self.act_graph and self.latent_cache and self.vae_device == self.device:
            return self._act_graphed(tick_data, deterministic, allowed)
        return self.act_from_feature(self.get_latent_feature(tick_data), tick_data["command"], deterministic, allowed)

    # ------------------------------------------------------------------ act() as a hipGraph
    def _act_static(self, S, H, W):
        """Static buffers of the captured act(): pinned host staging + device inputs, the feature rows, the latent
        cache, the sampler inputs / outputs."""
        dev, a = self.device, self.arena
        nS, nT = a.n_out
        pin = lambda *shape, dtype: torch.empty(*shape, dtype=dtype).pin_memory()
        st = dict(shape=(S, H, W),
                  h_rgb=pin(S, H, W, 3, dtype=torch.uint8), h_route=pin(S, W, H, dtype=torch.uint8),
                  h_rn=pin(S, W, H, dtype=torch.uint8), h_meas=pin(S, 3, dtype=torch.float64),
                  h_q=pin(2, 64, dtype=torch.float32),
                  d_rgb=torch.zeros(S, H, W, 3, dtype=torch.uint8, device=dev),
                  d_route=torch.zeros(S, W, H, dtype=torch.uint8, device=dev),
                  d_rn=torch.zeros(S, W, H, dtype=torch.uint8, device=dev),
                  d_meas=torch.zeros(S, 3, dtype=torch.float64, device=dev),
                  d_q=torch.ones(2, 64, device=dev),
                  feat=torch.zeros(S, a.DP, device=dev), lat=torch.zeros(S, 512, device=dev),
                  action=torch.zeros(2, dtype=torch.int64, device=dev), logp=torch.zeros(2, 1, device=dev),
                  graphs={}, warm=set(), gen=self.vae_model.ws_generation)
        return st

    def _act_body(self, st, shifted, command, masked=False):
        """The device work of one env step on the static buffers (eager or under capture); masked: the samplers read the
        static words st["d_allowed"]."""
        S = st["shape"][0]
        L, stream = hip.lib(), hip.stream()
        enc, feat, lat = self.vae_model, st["feat"], st["lat"]
        first = S - 1 if shifted else 0
        rn = st["d_rn"][first:] if self.mutate_route else None
        x = enc.preprocess(st["d_rgb"][first:], st["d_route"][first:], rn)
        if shifted:
            feat[:-1, :512].copy_(lat[1:])
        enc.forward_nhwc(x, feat[first:])
        lat.copy_(feat[:, :512])
        hip.check(L.cadre_append_measurements(hip.ptr(st["d_meas"]), hip.ptr(feat), feat.stride(0), S, stream),
                  "cadre_append_measurements")
        O3, _, _ = self.learner.infer(feat[:, :self.lstm_input], (command, command))
        nS, nT = self.arena.n_out
        for j, (row, K) in enumerate(((0, nS), (2, nT))):
            self._sample_launch(O3, row, K, st["d_q"][j], st["action"][j:], st["logp"][j:],
                                st["d_allowed"][j:] if masked else None)
        return O3

    def _act_graphed(self, tick_data, deterministic=False, allowed=None):
        rgb, route_np, command = tick_data["rgb"], tick_data["route_fig"], int(tick_data["command"])
        S, H, W = rgb.shape[0], rgb.shape[1], rgb.shape[2]
        st = self._ag
        if st is None or st["shape"] != (S, H, W):
            st = self._ag = self._act_static(S, H, W)
            self._cache = None
        if st["gen"] != self.vae_model.ws_generation:            # an encoder workspace tensor was replaced: addresses moved
            st["graphs"].clear(); st["warm"].clear()
            st["gen"] = self.vae_model.ws_generation
        if self._cache is not None and self._cache["latent"] is not st["lat"]:
            st["lat"].copy_(self._cache["latent"])                # the eager path (get_latent_feature) ran in between
        shifted = self._window_shifted(tick_data)
        first = S - 1 if shifted else 0
        raw_rgb, raw_route = rgb.copy(), route_np.copy()
        # inputs: numpy -> pinned staging -> static device buffers (only the newest frame when the window shifted).  The
        # pinned buffers are rewritten only after the previous call's asynchronous H2D copies have left them (a caller
        # that has not read the last action yet may call act() again)
        ev = st.get("h2d_done")
        if ev is not None:
            ev.synchronize()
        st["h_rgb"][first:].copy_(torch.from_numpy(np.ascontiguousarray(rgb[first:])))
        st["h_route"][first:].copy_(torch.from_numpy(np.ascontiguousarray(route_np[first:])))
        st["h_meas"].copy_(torch.from_numpy(np.ascontiguousarray(tick_data["measurements"], dtype=np.float64)))
        nS, nT = self.arena.n_out
        if deterministic:
            st["h_q"].fill_(1.0)
        else:
            st["h_q"][0, :nS] = torch.empty(1, nS).exponential_(1)[0]      # steer draws first (reference order)
            st["h_q"][1, :nT] = torch.empty(1, nT).exponential_(1)[0]
        st["d_rgb"][first:].copy_(st["h_rgb"][first:], non_blocking=True)
        st["d_route"][first:].copy_(st["h_route"][first:], non_blocking=True)
        st["d_meas"].copy_(st["h_meas"], non_blocking=True)
        st["d_q"].copy_(st["h_q"], non_blocking=True)
        if ev is None:
            ev = st["h2d_done"] = torch.cuda.Event()
        ev.record()
        lrn = self.learner
        lrn.packed_weights(0, 1, self.arena.Z)                    # refreshed here when the parameters changed, not in the graph
        masked = allowed is not None
        key = (shifted, command) + (("mask",) if masked else ())  # (a masked step is a graph of its own: another sampler)
        if masked:
            if "d_allowed" not in st:                             # static, as every pointer of a captured step
                st["d_allowed"] = torch.zeros(2, dtype=torch.int64, device=self.device)
            st["d_allowed"].copy_(allowed)
        g = st["graphs"].get(key)
        if g is not None:
            g.replay()
        else:
            self._act_body(st, shifted, command, masked)          # eager (also the warm-up of every lazily built buffer)
            if key in st["warm"] and lrn.use_graphs:
                torch.cuda.synchronize()
                lrn.pack_outside_capture = True
                try:
                    st["graphs"][key] = lrn._capture(lambda: self._act_body(st, shifted, command, masked))
                finally:
                    lrn.pack_outside_capture = False
            st["warm"].add(key)
        O3 = lrn.workspace(1, 2, S)["O3"]
        # outputs: fresh tensors (callers keep references), one host sync for the route the reference mutates in place
        feat = st["feat"][:, :self.lstm_input].clone()
        a_s, a_t = st["action"][0].clone(), st["action"][1].clone()
        lp_s, lp_t = st["logp"][0:1].clone(), st["logp"][1:2].clone()
        v_s, v_t = O3[1, :, :1].clone(), O3[3, :, :1].clone()
        if self.mutate_route:
            st["h_rn"][first:].copy_(st["d_rn"][first:], non_blocking=True)
            torch.cuda.current_stream().synchronize()
            if shifted:
                route_np[:-1] = self._cache["route_norm"][1:]
            route_np[first:] = st["h_rn"][first:].numpy()        # agent.py:51-54 mutates the caller's dict
        self._cache = dict(rgb=raw_rgb, route_raw=raw_route, route_norm=route_np.copy(), latent=st["lat"])
        ctl_s = self.model_dict["steer_ppo_%d" % command].control
        ctl_t = self.model_dict["throttle_ppo_%d" % command].control
        ctl_s._last_action, ctl_s._last_logp = a_s.view(1), lp_s
        ctl_t._last_action, ctl_t._last_logp = a_t.view(1), lp_t
        # the reference discards the new hidden state and returns the zeros (agent.py:123-124,141)
        return feat, [a_s, a_t], [lp_s, lp_t], [v_s, v_t], self.hidden_state

    def act_from_feature(self, ppo_feature, command, deterministic=False, allowed=None):
        """The part of `act` after the encoder (agent.py:116-141) on a given [S,530] feature window.  `allowed`: None, or a
        device int64 [2] tensor of the (steer, throttle) words (act() builds it)."""
        O3, _, _ = self.learner.infer(ppo_feature, (command, command))
        nS, nT = self.arena.n_out
        if deterministic:
            q_s, q_t = torch.ones(1, nS), torch.ones(1, nT)
        else:
            q_s = torch.empty(1, nS).exponential_(1)
            q_t = torch.empty(1, nT).exponential_(1)
        a_s, lp_s = self._sample(O3, 0, nS, q_s, None if allowed is None else allowed[0:])
        a_t, lp_t = self._sample(O3, 2, nT, q_t, None if allowed is None else allowed[1:])
        v_s = O3[1, :, :1].clone()
        v_t = O3[3, :, :1].clone()
        ctl_s = self.model_dict["steer_ppo_%d" % command].control
        ctl_t = self.model_dict["throttle_ppo_%d" % command].control
        ctl_s._last_action, ctl_s._last_logp = a_s, lp_s
        ctl_t._last_action, ctl_t._last_logp = a_t, lp_t
        # the reference discards the new hidden state and returns the zeros (agent.py:123-124,141)
        return ppo_feature, [a_s[0], a_t[0]], [lp_s, lp_t], [v_s, v_t], self.hidden_state

    # ------------------------------------------------------------------ act for N environments
    def act_batch(self, obs_list, shifted=None, deterministic=False, allowed=None):
        """`[self.act(o) for o in obs_list]` for N environments in ONE launch chain: one encoder pass over every fresh
        frame (the newest frame of each window that shifted, all S frames of the others), cadre_act_windows (the LSTM
        input rows of all windows, rows sorted by command), one LSTM + MLP pass over all 2C command nets
        (learner._forward with row_seg) and cadre_sample_rows.  Each environment keeps its own sliding-window cache
        (slot e of a device ring of latents); `shifted[e]` (optional) asserts that environment e's window moved by one
        frame since the last call, which skips the host-side comparison of the frames.  Global-RNG consumption is the
        loop's: one exponential_(1) draw per environment and head, env 0 steer, env 0 throttle, env 1 steer, ...
        The route quirk (agent.py:51-54: the caller's route_fig normalised in place) is kept per environment.
        `deterministic=True`: the greedy action of every (environment, head) — q stays all ones, nothing is drawn.
        `allowed` (action masks): per environment a (steer_word, throttle_word) pair of Python ints, or a device int64 [N][2]
        tensor; the sampling launch is then cadre_sample_rows_am and the result carries the words as `.allowed` (what
        RolloutStorage.insert_batch(allowed=) takes).  None launches exactly what is launched without the feature.
        Returns an ActBatch: N tuples in exactly act()'s format."""
        check_act_batch(obs_list, shifted, self.max_envs, self.device, self.vae_device, self.command_num)
        N = len(obs_list)
        if allowed is not None:                             # (checked before anything is drawn or launched)
            from ..actmask import words_tensor
            allowed = words_tensor(allowed, N, self.arena.n_out, self.device)
        a, enc, dev = self.arena, self.vae_model, self.device
        S, H, W = obs_list[0]["rgb"].shape[:3]
        L, stream = hip.lib(), hip.stream()
        vec = self._vec
        if vec is None or vec["shape"] != (S, H, W) or vec["ring"].shape[0] < self.max_envs:
            vec = self._vec = dict(shape=(S, H, W), ring=torch.zeros(self.max_envs, S, 512, device=dev),
                                   cache=[None] * self.max_envs)
        cache = vec["cache"]
        commands = [int(td["command"]) for td in obs_list]
        # window mode per environment, then the fresh frames of all of them in one host array
        modes, firsts, rgbs, routes = [], [], [], []
        nf = 0
        for e, td in enumerate(obs_list):
            c = cache[e]
            if c is None or not self.latent_cache:
                m = False
            elif shifted is not None:
                m = bool(shifted[e])
            else:
                m = self._window_shifted_vs(c, td)
            f = S - 1 if m else 0
            modes.append(1 if m else 0)
            firsts.append(nf)
            nf += S - f
            rgbs.append(td["rgb"][f:])
            routes.append(td["route_fig"][f:])
        rgb_d = torch.from_numpy(np.concatenate(rgbs)).to(dev)
        route_d = torch.from_numpy(np.concatenate(routes)).to(dev)
        rn_d = torch.empty_like(route_d) if self.mutate_route else None
        lat = torch.empty(nf, 512, device=dev)
        for s0 in range(0, nf, enc.max_frames):             # (the encoder's workspace is sized for max_frames)
            s1 = min(nf, s0 + enc.max_frames)
            x = enc.preprocess(rgb_d[s0:s1], route_d[s0:s1], None if rn_d is None else rn_d[s0:s1])
            enc.forward_nhwc(x, lat[s0:s1])
        # small inputs: descriptors + sort (int32), measurements (f64), sampler noise (f32) — one copy each
        pos, seg = command_rows(commands, self.command_num)
        ints = np.concatenate([seg.reshape(-1), np.asarray(modes, np.int32), np.asarray(firsts, np.int32), pos,
                               np.asarray(commands, np.int32)])
        ints_d = torch.from_numpy(ints).to(dev)
        nseg = seg.size
        seg_d = ints_d[:nseg]
        mode_d, first_d, pos_d, cmd_d = (ints_d[nseg + i * N:nseg + (i + 1) * N] for i in range(4))
        meas = np.stack([np.asarray(td["measurements"], dtype=np.float64) for td in obs_list])
        meas_d = torch.from_numpy(np.ascontiguousarray(meas)).to(dev)
        nS, nT = a.n_out
        q = torch.ones(N, 2, 64)
        for e in range(0 if deterministic else N):          # act()'s order: steer draws first, environment after environment
            q[e, 0, :nS] = torch.empty(1, nS).exponential_(1)[0]
            q[e, 1, :nT] = torch.empty(1, nT).exponential_(1)[0]
        q_d = q.to(dev)
        # LSTM input rows (sorted by command) + the per-environment feature windows, the ring advanced
        w = self.learner.workspace(N, a.Z, S)
        feat = torch.empty(N, S, a.DP, device=dev)            # fresh: callers keep references
        hip.check(L.cadre_act_windows(hip.ptr(vec["ring"]), vec["ring"].stride(0), vec["ring"].shape[0], hip.ptr(lat),
                                      lat.stride(0), nf, hip.ptr(mode_d), hip.ptr(first_d), hip.ptr(meas_d), hip.ptr(pos_d),
                                      N, S, hip.ptr(w["X"]), a.DP, a.DP, hip.ptr(feat), a.DP, stream), "cadre_act_windows")
        w["h0"].zero_(); w["c0"].zero_()
        # every net reads head block 0 of X (x_div = 2C): steer and throttle nets see the same window
        self.learner._forward(w, N, (0, 1, a.Z), 2 * a.C, S=S, seg=seg_d, fused_mlp=True)
        O3 = w["O3"]
        action = torch.empty(N, 2, dtype=torch.int64, device=dev)
        logp = torch.empty(N, 2, device=dev)
        value = torch.empty(N, 2, device=dev)
        if allowed is not None:
            hip.check(L.cadre_sample_rows_am(hip.ptr(O3), O3.stride(1), O3.stride(0), hip.ptr(pos_d), hip.ptr(cmd_d), N, a.C,
                                             hip.ptr(q_d), nS, nT, hip.ptr(action), hip.ptr(logp), hip.ptr(value),
                                             hip.ptr(self._am_ord()), hip.ptr(allowed), stream), "cadre_sample_rows_am")
        elif a.ord is not None:
            hip.check(L.cadre_sample_rows_ord(hip.ptr(O3), O3.stride(1), O3.stride(0), hip.ptr(pos_d), hip.ptr(cmd_d), N, a.C,
                                              hip.ptr(q_d), nS, nT, hip.ptr(action), hip.ptr(logp), hip.ptr(value),
                                              hip.ptr(a.ord), stream), "cadre_sample_rows_ord")
        else:
            hip.check(L.cadre_sample_rows(hip.ptr(O3), O3.stride(1), O3.stride(0), hip.ptr(pos_d), hip.ptr(cmd_d), N, a.C,
                                          hip.ptr(q_d), nS, nT, hip.ptr(action), hip.ptr(logp), hip.ptr(value), stream),
                      "cadre_sample_rows")
        # route quirk + window caches (one host sync for the normalised route, as act() has)
        rn_h = rn_d.cpu().numpy() if rn_d is not None else None
        out = ActBatch()
        for e, td in enumerate(obs_list):
            route_np = td["route_fig"]
            raw_rgb = td["rgb"].copy() if (self.latent_cache and shifted is None) else None
            raw_route = route_np.copy() if self.latent_cache else None
            if rn_h is not None:
                if modes[e]:
                    route_np[:-1] = cache[e]["route_norm"][1:]
                    route_np[S - 1:] = rn_h[firsts[e]:firsts[e] + 1]
                else:
                    route_np[:] = rn_h[firsts[e]:firsts[e] + S]
            if self.latent_cache:
                cache[e] = dict(rgb=raw_rgb, route_raw=raw_route, route_norm=route_np.copy())
            lp_s, lp_t = logp[e, 0:1].view(1, 1), logp[e, 1:2].view(1, 1)
            out.append((feat[e, :, :self.lstm_input], [action[e, 0], action[e, 1]], [lp_s, lp_t],
                        [value[e, 0:1].view(1, 1), value[e, 1:2].view(1, 1)], self.hidden_state))
            ctl_s = self.model_dict["steer_ppo_%d" % commands[e]].control
            ctl_t = self.model_dict["throttle_ppo_%d" % commands[e]].control
            ctl_s._last_action, ctl_s._last_logp = action[e, 0:1], lp_s
            ctl_t._last_action, ctl_t._last_logp = action[e, 1:2], lp_t
        out.feat, out.action, out.logp, out.value = feat, action, logp, value
        if allowed is not None:
            out.allowed = allowed
        return out

    @staticmethod
    def _window_shifted_vs(c, tick_data):
        """_window_shifted against one act_batch window cache (a cache written under a `shifted` hint holds no raw
        frames: the window is then encoded in full)."""
        if c["rgb"] is None:
            return False
        rgb, route = tick_data["rgb"], tick_data["route_fig"]
        if rgb.shape != c["rgb"].shape or route.shape != c["route_raw"].shape:
            return False
        if not np.array_equal(rgb[:-1], c["rgb"][1:]):
            return False
        return np.array_equal(route[:-1], c["route_raw"][1:]) or np.array_equal(route[:-1], c["route_norm"][1:])

    def get_value(self, done, steer_batch, throttle_batch):
        """agent.py:143-164."""
        if done:
            return torch.zeros(1), torch.zeros(1)
        s_obs, s_cmd = steer_batch
        t_obs, t_cmd = throttle_batch
        if torch.is_tensor(s_cmd) or torch.is_tensor(t_cmd):        # get_last(as_tensor=True): no host sync, net picked on the device
            return self.get_values([(steer_batch, throttle_batch)])[0]
        O3, _, _ = self.learner.infer(torch.stack([s_obs, t_obs]), (int(s_cmd), int(t_cmd)))
        return O3[1, :, :1].clone(), O3[3, :, :1].clone()

    def get_values(self, batches, dones=None):
        """get_value (agent.py:143-164) for several workers at once: batches = [(steer_batch, throttle_batch), ...] as
        `RolloutStorage.get_last()` returns them; dones[i] (default: none) is worker i's `done` flag — a finished
        episode bootstraps from zeros (agent.py:144-146).  One LSTM + critic pass over all command nets with one row
        per worker instead of one launch chain per worker; returns [(v_steer [1,1], v_throttle [1,1]), ...]."""
        feats = torch.stack([torch.stack([sb[0] for sb, _tb in batches]), torch.stack([tb[0] for _sb, tb in batches])])
        O3 = self.learner.infer_rows(feats).clone()
        C = self.arena.C
        dev_cmd = any(torch.is_tensor(sb[1]) or torch.is_tensor(tb[1]) for sb, tb in batches)
        if dev_cmd:
            # commands as device tensors (RolloutStorage.get_last(as_tensor=True)): every row's critic tower is picked by an
            # index computed on the device — no .item(), so the host runs ahead of the encoder pass still in flight
            dev = O3.device
            as_t = lambda c: c.reshape(()).to(dev, torch.int64) if torch.is_tensor(c) else torch.tensor(int(c), device=dev)
            cs = torch.stack([as_t(sb[1]) for sb, _tb in batches])
            ct = torch.stack([as_t(tb[1]) for _sb, tb in batches])
            rows = torch.arange(len(batches), device=dev)
            vs, vt = O3[2 * cs + 1, rows, 0], O3[2 * (C + ct) + 1, rows, 0]
        out = []
        for i, (sb, tb) in enumerate(batches):
            if dones is not None and dones[i]:
                out.append((torch.zeros(1), torch.zeros(1)))
            elif dev_cmd:
                out.append((vs[i:i + 1].view(1, 1), vt[i:i + 1].view(1, 1)))
            else:
                out.append((O3[2 * int(sb[1]) + 1, i:i + 1, :1], O3[2 * (C + int(tb[1])) + 1, i:i + 1, :1]))
        return out

    # ------------------------------------------------------------------ update
    def _pack(self, w, hd, samples):
        obs, act, old_v, ret, _masks, old_lp, adv, hidden, cmd = samples
        B = act.shape[0]
        S, D = self.learner.S, self.arena.D
        w["X"][hd].view(S * B, -1)[:, :D].copy_(obs)
        w["h0"][hd][:, :D].copy_(hidden[0])
        w["c0"][hd][:, :D].copy_(hidden[1])
        w["actions"][hd].copy_(act.reshape(-1))
        w["commands"][hd].copy_(cmd.reshape(-1))
        w["old_values"][hd].copy_(old_v.reshape(-1))
        w["returns"][hd].copy_(ret.reshape(-1))
        w["old_logp"][hd].copy_(old_lp.reshape(-1))
        w["adv"][hd].copy_(adv.reshape(-1))

    def update_policy(self, steer_samples, throttle_samples, workers=1, stats_row=None):
        """agent.py:166-237: fused forward + loss + explicit backward; `.grad` of every parameter in
        model_dict (views of the gradient arena) holds d total_loss afterwards.  With `workers` > 1
        the sample tuples are the row-concatenation of that many equal-size worker minibatches and
        the losses are the SUM of per-worker means.  `stats_row`: device float32
        [2][learner.stats_fields()] that receives the step's diagnostics (learner.set_update_modes(stats=True))."""
        B = steer_samples[1].shape[0]
        if throttle_samples[1].shape[0] != B:
            raise ValueError("steer/throttle minibatches differ in size")
        self.learner._check_not_swapped("update_policy")
        w = self.learner.workspace(B)
        self._pack(w, 0, steer_samples)
        self._pack(w, 1, throttle_samples)
        losses = self.learner.update(B, float(workers) / B, stats_row=stats_row)
        self.arena.attach_grads(self.model_dict)
        v, a, e = losses.tolist()
        return v, a, e

    def update_policy_from_storages(self, batches, sync=True, mlp_grads_ready=None, stats_row=None, evaluate=False,
                                    demo=None, demo_stats_row=None, demo_label_smoothing=None, demo_coeff=None,
                                    demo_value_coeff=None, sil=None, sil_stats_row=None, smooth=None,
                                    smooth_stats_row=None, actmask=None):
        """Fast path of the learner section: `batches` = [(steer_storage, steer_idx, steer_adv,
        throttle_storage, throttle_idx, throttle_adv), ...] one entry per worker (equal sizes).
        Same math as feed_forward_generator -> update_policy, but the minibatch gather writes
        straight into the update workspace (cadre_gather_minibatch) and the losses stay on the device
        unless `sync` (one host sync per round instead of one per minibatch).  `mlp_grads_ready`
        (callable, optional) is invoked between the MLP-tower backward and the LSTM backward, when the
        gradients of arena[P0:] are final (Shared_grad_buffers.reduce_bucket_async starts their all-reduce
        there, beside the LSTM backward).  `stats_row`: as in update_policy.  `evaluate` (imitation loss only, see
        imitate_from_storages): forward + the evaluation form of the loss on the gathered rows, no gradient.
        `demo` (DAPG-style mixing): a list of entries of the form DemoSet.batch(idx) returns, each with as many rows as a
        worker entry.  They are appended to the gather table behind the workers' entries and the step runs the mixed loss
        (PPOLearnerHIP.set_loss("ppo+demo"), for the duration of the call): total = the PPO loss, each worker's mean summed
        as always, + demo_coeff * mean over ALL demonstration rows of w CE + demo_value_coeff * 0.5 * mean of w (v - R)^2.
        The three floats returned are the PPO terms over the PPO rows; the two demo terms stay on the device in
        learner.workspace(B)["demo_losses"], the imitation statistics go to `demo_stats_row` (device float32
        [2][>= hip.BC_STATS_FIELDS]); `stats_row` receives the PPO rows' diagnostics.  demo_label_smoothing / demo_coeff /
        demo_value_coeff: None keeps the learner's current settings (in device-hyper mode the coefficients are the block's).
        `sil` (self-imitation): a list of entries of the same form whose rows are the agent's own past transitions
        (SelfImitationBuffer.entries: the index tensors live on the device, filled by the prioritised draw).  They are appended
        behind the workers' entries and the step runs the mixed loss (PPOLearnerHIP.set_loss("ppo+sil"), for the duration of
        the call) with the learner's current SIL coefficients: total = the PPO loss + sil_coeff * mean(-lp w) +
        sil_value_coeff * mean(0.5 w^2), w = max(R - v, 0), the means over ALL SIL rows.  The three floats returned are the
        PPO terms; the two SIL terms and the rows' w stay on the device in learner.workspace(B)["sil_losses"] / ["sil_w"],
        the SIL statistics go to `sil_stats_row` (device float32 [2][>= hip.SIL_STATS_FIELDS]).  Excludes `demo`.
        `smooth` (temporal smoothness): what cadre_amd.smooth.Smoothness.step(batches) returns — (entries, rotation): E <= nW
        successor entries of the same form (entry k: the storages and advantages of worker (rotation + k) mod nW, the index
        vectors min(t + 1, T - 1) on the host) and the step's rotation.  They are appended behind the workers' entries, one
        cadre_smooth_mates launch behind the gather / sort places the pairs, and the step runs the mixed loss
        (PPOLearnerHIP.set_loss("ppo+smooth"), for the duration of the call) with the learner's current coefficient and
        tables: total = the PPO loss + smooth_coeff * head_scale * mean over the pair slots of d^2.  The three floats returned
        are the PPO terms; the smoothness term and the rows' d stay on the device in learner.workspace(B)["smooth_losses"] /
        ["smooth_d"], the statistics go to `smooth_stats_row` (device float32 [2][>= hip.SMOOTH_STATS_FIELDS]).  Excludes
        `demo` and `sil`.
        `actmask` (action masks: a cadre_amd.actmask.ActionMasks, or True): the step runs the masked loss
        (PPOLearnerHIP.set_loss("ppo+mask"), for the duration of the call).  One cadre_allowed_rows launch behind the gather /
        sort carries the `allowed` words of the step's storages (a storage without the tensor: unmasked rows) into
        learner.workspace(B)["allowed"]; the mask statistics of the step stay on the device in workspace(B)["am_stats"] (an
        ActionMasks collects them).  Excludes `demo`, `sil`, `smooth` and `evaluate`: their kernels do not read the mask."""
        if actmask is not None and actmask is not False:
            if evaluate or demo or sil or smooth is not None:
                raise ValueError("update_policy_from_storages: actmask excludes demo, sil, smooth and evaluate (their kernels do "
                                 "not read the rows' allowed-bin words yet)")
            lrn = self.learner
            if lrn.loss_mode not in ("ppo", "ppo+mask"):
                raise ValueError("update_policy_from_storages: actmask with the learner's loss set to %r (its kernel does not "
                                 "read the rows' allowed-bin words yet)" % (lrn.loss_mode,))
            with lrn.loss_scope("ppo+mask"):
                out = self._update_from_storages(batches, sync, mlp_grads_ready, stats_row, False)
                if hasattr(actmask, "step"):
                    actmask.step(lrn)
                return out
        if smooth is not None:
            if evaluate or demo or sil:
                raise ValueError("update_policy_from_storages: successor rows have no evaluation form and exclude demo and sil "
                                 "rows (a row carries one kind array)")
            entries, rotation = smooth
            nW, E = len(batches), len(entries)
            if isinstance(rotation, bool) or not isinstance(rotation, int) or rotation < 0 or not 1 <= E <= nW:
                raise ValueError("update_policy_from_storages: smooth=(entries, rotation) with 1 <= len(entries) <= %d worker "
                                 "entries and an integer rotation >= 0 (got %d, %r)" % (nW, E, rotation))
            for k, e in enumerate(entries):
                b = batches[(rotation + k) % nW]
                if e[0] is not b[0] or e[3] is not b[3] or e[2] is not b[2] or e[5] is not b[5]:
                    raise ValueError("update_policy_from_storages: successor entry %d does not carry the storages and advantages "
                                     "of worker %d" % (k, (rotation + k) % nW))
            lrn = self.learner
            with lrn.loss_scope("ppo+smooth", rows=nW * batches[0][1].numel()):
                self._smooth_step = (nW, E, rotation)
                try:
                    out = self._update_from_storages(list(batches) + list(entries), sync, mlp_grads_ready, stats_row, False)
                    if smooth_stats_row is not None:
                        B = (nW + E) * batches[0][1].numel()
                        smooth_stats_row[:, :hip.SMOOTH_STATS_FIELDS].copy_(lrn.workspace(B)["smooth_stats"])
                    return out
                finally:
                    self._smooth_step = None
        if smooth_stats_row is not None:
            raise ValueError("update_policy_from_storages: smooth_stats_row without smooth entries")
        if sil:
            if evaluate or demo:
                raise ValueError("update_policy_from_storages: sil rows have no evaluation form and exclude demo rows "
                                 "(a row carries one kind array)")
            lrn = self.learner
            with lrn.loss_scope("ppo+sil", rows=len(batches) * batches[0][1].numel()):
                out = self._update_from_storages(list(batches) + list(sil), sync, mlp_grads_ready, stats_row, False)
                if sil_stats_row is not None:
                    B = (len(batches) + len(sil)) * batches[0][1].numel()
                    sil_stats_row[:, :hip.SIL_STATS_FIELDS].copy_(lrn.workspace(B)["sil_stats"])
                return out
        if sil_stats_row is not None:
            raise ValueError("update_policy_from_storages: sil_stats_row without sil entries")
        if demo:
            if evaluate:
                raise ValueError("update_policy_from_storages: demo rows have no evaluation form here (imitate_from_storages(evaluate=True))")
            with self.learner.loss_scope("ppo+demo", rows=len(batches) * batches[0][1].numel(), label_smoothing=demo_label_smoothing,
                                         demo_coeff=demo_coeff, demo_value_coeff=demo_value_coeff):
                return self._update_from_storages(list(batches) + list(demo), sync, mlp_grads_ready, stats_row, False,
                                                  demo_stats_row)
        if demo_stats_row is not None:
            raise ValueError("update_policy_from_storages: demo_stats_row without demo entries")
        return self._update_from_storages(batches, sync, mlp_grads_ready, stats_row, evaluate)

    def _update_from_storages(self, batches, sync, mlp_grads_ready, stats_row, evaluate, demo_stats_row=None, record=None):
        nW = len(batches)
        self.learner._check_not_swapped("update_policy_from_storages")
        mode = LOSS_MODES[self.learner.loss_mode]
        if (record is None and not evaluate and mode.ppo and not mode.reads_allowed
                and any(getattr(b[k], "allowed", None) is not None for b in batches for k in (0, 3))):
            raise ValueError("update_policy_from_storages: a storage of this step carries `allowed` words (its actions were sampled "
                             "under action masks) but the loss is %r, which does not read them: old_logp would belong to another "
                             "distribution than the ratio's; pass actmask= (learner_section(..., actmask=))" % (self.learner.loss_mode,))
        Bw = batches[0][1].numel()
        B = nW * Bw
        w = self.learner.workspace(B)
        L, st = hip.lib(), hip.stream()
        a = self.arena
        srt = self.learner.sorted_rows(B)
        u = "_u" if srt else ""                       # sorted mode: gather into staging, then sort + permute
        Xk, hk, ck = ("Xu", "h0u", "c0u") if srt else ("X", "h0", "c0")
        if any(b[1].numel() != Bw or b[4].numel() != Bw for b in batches):
            raise ValueError("update_policy_from_storages: every worker's steer and throttle minibatch must have the same "
                             "number of rows (the losses are the sum of per-worker means over equal minibatches)")
        aux = self.learner.loss_mode == "aux"          # the auxiliary loss / record: the step's indices are its table rows
        if aux:
            if nW != 1:
                raise ValueError("the auxiliary loss takes exactly one gather entry (got %d)" % nW)
            # a STATIC workspace tensor: the staging ring below hands out a different device pointer each step, and a
            # captured graph would replay a stale one
            self.learner._aux_args(w, B, srt)          # (refuses without a table; allocates the tensor)
            aux_rows = w["aux_rows"]
        if record is not None:                         # reuse_record_from_storages: the step's indices are the tables' rows
            aux = True
            if "reuse_rows" not in w:                  # (static, as aux_rows)
                w["reuse_rows"] = torch.zeros(2, B, dtype=torch.int64, device=self.device)
            aux_rows = w["reuse_rows"]
        s0 = batches[0][0]
        geo = (s0._ldo, s0.seq_length, s0._ldh)
        # a frame-table storage (cadre_amd.frames.FrameStorage) among the step's: the gathers' `_ft` twins, which take the
        # window ids of each source (none: a materialised one).  With no such storage the launches are what they always were
        ft = any(getattr(st_, "_win", None) is not None for b in batches for st_ in (b[0], b[3]))
        self._gather_entry = None                      # the gather entry point of the step (what the tests look at)
        if any((st_._ldo, st_.seq_length, st_._ldh) != geo for b in batches for st_ in (b[0], b[3])):
            # storages of different geometry (feature pitch / window length): one gather launch per storage with its
            # own strides (cadre_gather_minibatch) — the one-launch table below assumes a single geometry
            if mode.one_geometry:
                raise ValueError("the %r loss needs storages of one geometry: the kinds of the minibatch are placed "
                                 "by one launch beside the one-launch gather" % (self.learner.loss_mode,))
            self._gather_entry = "cadre_gather_minibatch_ft" if ft else "cadre_gather_minibatch"
            for i, (ss, si, sa, ts, ti, ta) in enumerate(batches):
                for hd, (stor, idx, adv) in enumerate(((ss, si, sa), (ts, ti, ta))):
                    idx_d = idx.reshape(-1).to(self.device)
                    if aux:
                        aux_rows[hd].copy_(idx_d)
                    rest = (stor._ldo, stor.seq_length, hip.ptr(stor._hn), hip.ptr(stor._cn), stor._ldh,
                            hip.ptr(stor.action), hip.ptr(stor.value_preds), hip.ptr(stor.returns),
                            hip.ptr(stor.action_log_probs), hip.ptr(stor.command), hip.ptr(adv), hip.ptr(idx_d), Bw, a.D, a.D,
                            B, i * Bw, hip.ptr(w[Xk][hd]), a.DP, hip.ptr(w[hk][hd]), hip.ptr(w[ck][hd]), a.DP,
                            hip.ptr(w["actions" + u][hd]), hip.ptr(w["commands" + u][hd]), hip.ptr(w["old_values" + u][hd]),
                            hip.ptr(w["returns" + u][hd]), hip.ptr(w["old_logp" + u][hd]), hip.ptr(w["adv" + u][hd]), st)
                    if ft:
                        hip.check(L.cadre_gather_minibatch_ft(*(self._ft_source(stor) + rest)), "cadre_gather_minibatch_ft")
                    else:
                        hip.check(L.cadre_gather_minibatch(hip.ptr(stor._obs), *rest), "cadre_gather_minibatch")
            return self._finish_update(w, B, nW, srt, sync, mlp_grads_ready, evaluate=evaluate, stats_row=stats_row,
                                       demo_stats_row=demo_stats_row, record=record)
        # ONE gather launch for all workers and both heads: a device table of the storages' pointers (built once per set
        # of storages / advantage tensors) and one host-to-device copy of the 2*nW index vectors
        pairs = [(stor, adv) for (ss, si, sa, ts, ti, ta) in batches for (stor, adv) in ((ss, sa), (ts, ta))]
        ptrs = [[hip.ptr(stor._obs), hip.ptr(stor._hn), hip.ptr(stor._cn), hip.ptr(stor.action), hip.ptr(stor.value_preds),
                 hip.ptr(stor.returns), hip.ptr(stor.action_log_probs), hip.ptr(stor.command), hip.ptr(adv)] for stor, adv in pairs]
        if ft:      # records of eleven words: the frame table in the first, then the window ids (0: materialised) and the frame count
            ptrs = [[src[0]] + row[1:] + [src[1] or 0, src[2]] for row, src in zip(ptrs, (self._ft_source(stor) for stor, _ in pairs))]
        key = (("ft",) if ft else ()) + tuple(p for row in ptrs for p in row)
        cache = self.__dict__.setdefault("_gather_tables", {})
        table = cache.get(key)
        if table is None:
            if len(cache) > 16:
                cache.clear()
            host = torch.tensor(ptrs, dtype=torch.int64).pin_memory()      # pinned: the copy does not stall the host
            table = torch.empty_like(host, device=self.device)
            table.copy_(host, non_blocking=True)
            cache[key] = table
            self.__dict__.setdefault("_gather_tables_host", []).append(host)   # alive until the copy has run
            del self._gather_tables_host[:-16]
        # (pinned staging buffers in a ring: a slot is rewritten only after the copy that last read it has completed —
        #  the caller may enqueue several minibatch steps without a host sync)
        ring = self.__dict__.get("_gather_idx")
        if ring is None or ring["shape"] != (2 * nW, Bw):
            ring = self._gather_idx = dict(shape=(2 * nW, Bw), pos=0, slots=[
                [torch.empty(2 * nW, Bw, dtype=torch.int64).pin_memory(),
                 torch.empty(2 * nW, Bw, dtype=torch.int64, device=self.device), None] for _ in range(8)])
        stage = ring["slots"][ring["pos"]]
        ring["pos"] = (ring["pos"] + 1) % len(ring["slots"])
        if stage[2] is not None:
            stage[2].synchronize()
        on_dev = []                                   # index vectors that are on the device already (a prioritised draw)
        for i, (ss, si, sa, ts, ti, ta) in enumerate(batches):
            for k, x in ((2 * i, si), (2 * i + 1, ti)):
                if x.is_cuda:
                    on_dev.append((k, x))
                else:
                    stage[0][k].copy_(x.reshape(-1))
        stage[1].copy_(stage[0], non_blocking=True)
        for k, x in on_dev:                           # behind the host-to-device copy: device-to-device, no sync
            stage[1][k].copy_(x.reshape(-1))
        if aux:
            aux_rows.copy_(stage[1])                  # (nW = 1: the index pair [steer; throttle] is row_id, head-major)
        if self.learner.loss_mode == "ppo+suggest" and record is None and not evaluate:
            # the `suggest` arrays of the step's storages, source by source (0: a storage without marks, e.g. a stale entry
            # of a ReuseWindow); the launch itself follows the gather / sort, which writes `pos`
            sptrs = tuple(hip.ptr(getattr(stor, "suggest", None)) or 0 for stor, _ in pairs)
            stable = cache.get(("suggest",) + sptrs)
            if stable is None:
                stable = cache[("suggest",) + sptrs] = torch.tensor(sptrs, dtype=torch.int64).to(self.device)
            self._suggest_src = (stable, stage[1], Bw, s0.num_steps)
        if self.learner.loss_mode == "ppo+mask" and record is None and not evaluate:
            # the `allowed` tensors of the step's storages, source by source (0: a storage that never saw a word: unmasked
            # rows); the launch itself follows the gather / sort, which writes `pos`
            sptrs = tuple(hip.ptr(getattr(stor, "allowed", None)) or 0 for stor, _ in pairs)
            stable = cache.get(("allowed",) + sptrs)
            if stable is None:
                stable = cache[("allowed",) + sptrs] = torch.tensor(sptrs, dtype=torch.int64).to(self.device)
            self._allowed_src = (stable, stage[1], Bw, s0.num_steps)
        if self.learner.loss_mode == "ppo+smooth" and record is None and not evaluate:
            # {masks, time_limits or 0, command} of the workers' storages, source by source; the launch itself follows the
            # gather / sort, which writes `pos`
            nWs = self._smooth_step[0]
            sptrs = tuple(p for stor, _ in pairs[:2 * nWs]
                          for p in (hip.ptr(stor.masks), hip.ptr(stor.time_limits) if stor._tl_used else 0, hip.ptr(stor.command)))
            stable = cache.get(("smooth",) + sptrs)
            if stable is None:
                stable = cache[("smooth",) + sptrs] = torch.tensor(sptrs, dtype=torch.int64).to(self.device)
            self._smooth_src = (stable, stage[1], Bw, s0.num_steps)
        stage[2] = torch.cuda.Event()
        stage[2].record()
        gs = getattr(self, "gather_sorted", None)     # None: CADRE_GATHER_SORTED decides (the default); True / False: this agent's switch
        if srt and (os.environ.get("CADRE_GATHER_SORTED", "1") != "0" if gs is None else gs):
            # rows sorted by command: gather, stable counting sort and placement in ONE launch (round 6; CADRE_GATHER_SORTED=0:
            # gather into staging rows, then cadre_sort_rows_by_command + cadre_permute_minibatch)
            name = self._gather_entry = "cadre_gather_sorted_multi_ft" if ft else "cadre_gather_sorted_multi"
            hip.check(getattr(L, name)(
                hip.ptr(table), 2 * nW, s0._ldo, s0.seq_length, s0._ldh, hip.ptr(stage[1]), Bw, a.D, a.D, B, a.C,
                hip.ptr(w["X"]), w["X"].stride(0), a.DP, hip.ptr(w["h0"]), hip.ptr(w["c0"]), w["h0"].stride(0), a.DP,
                hip.ptr(w["actions"]), hip.ptr(w["commands"]), hip.ptr(w["old_values"]),
                hip.ptr(w["returns"]), hip.ptr(w["old_logp"]), hip.ptr(w["adv"]), hip.ptr(w["pos"]), hip.ptr(w["seg"]), st), name)
            return self._finish_update(w, B, nW, srt, sync, mlp_grads_ready, evaluate=evaluate, placed=True, stats_row=stats_row,
                                       demo_stats_row=demo_stats_row, record=record)
        name = self._gather_entry = "cadre_gather_minibatch_multi_ft" if ft else "cadre_gather_minibatch_multi"
        hip.check(getattr(L, name)(
            hip.ptr(table), 2 * nW, s0._ldo, s0.seq_length, s0._ldh, hip.ptr(stage[1]), Bw, a.D, a.D, B,
            hip.ptr(w[Xk]), w[Xk].stride(0), a.DP, hip.ptr(w[hk]), hip.ptr(w[ck]), w[hk].stride(0), a.DP,
            hip.ptr(w["actions" + u]), hip.ptr(w["commands" + u]), hip.ptr(w["old_values" + u]),
            hip.ptr(w["returns" + u]), hip.ptr(w["old_logp" + u]), hip.ptr(w["adv" + u]), st), name)
        return self._finish_update(w, B, nW, srt, sync, mlp_grads_ready, evaluate=evaluate, stats_row=stats_row,
                                       demo_stats_row=demo_stats_row, record=record)

    @staticmethod
    def _ft_source(stor):
        """(rows pointer, window ids pointer or None, frame count) of a gather source for the `_ft` entry points."""
        win = getattr(stor, "_win", None)
        if win is None:
            return (hip.ptr(stor._obs), None, 0)
        return (hip.ptr(stor._frames), hip.ptr(win), int(stor.n_frames))

    def _finish_update(self, w, B, nW, srt, sync, mlp_grads_ready=None, placed=False, stats_row=None, evaluate=False,
                       demo_stats_row=None, record=None):
        """Row sort by command (sorted mode; placed: the gather already put every row at its sorted position), the fused update
        and the loss hand-back."""
        L, st, a = hip.lib(), hip.stream(), self.arena
        if srt and not placed:
            hip.check(L.cadre_sort_rows_by_command(hip.ptr(w["commands_u"]), B, a.C, hip.ptr(w["pos"]), hip.ptr(w["seg"]),
                                                   st), "cadre_sort_rows_by_command")
            hip.check(L.cadre_permute_minibatch(                   # both heads in one launch
                hip.ptr(w["pos"]), B, self.learner.S, hip.ptr(w["Xu"]), hip.ptr(w["X"]), a.DP,
                hip.ptr(w["h0u"]), hip.ptr(w["c0u"]), hip.ptr(w["h0"]), hip.ptr(w["c0"]), a.DP,
                hip.ptr(w["actions_u"]), hip.ptr(w["commands_u"]), hip.ptr(w["old_values_u"]),
                hip.ptr(w["returns_u"]), hip.ptr(w["old_logp_u"]), hip.ptr(w["adv_u"]),
                hip.ptr(w["actions"]), hip.ptr(w["commands"]), hip.ptr(w["old_values"]),
                hip.ptr(w["returns"]), hip.ptr(w["old_logp"]), hip.ptr(w["adv"]), 2, w["X"].stride(0), w["h0"].stride(0), st),
                "cadre_permute_minibatch")
        if record is not None:                           # reuse_record_from_storages: forward + the record launch only
            return self.learner.reuse_record(B, record[0], record[1], sorted_rows=srt)
        if self.learner.loss_mode == "ppo+suggest" and not evaluate:
            # the kinds of the minibatch's rows into the static workspace tensor the captured loss launch reads
            stable, idx_d, Bw, T = self._suggest_src
            hip.check(L.cadre_suggest_rows(hip.ptr(stable), 2 * nW, hip.ptr(idx_d), Bw, T, hip.ptr(w["pos"]) if srt else None, B,
                                           hip.ptr(self.learner._sug_ws(w, B)), st), "cadre_suggest_rows")
        if self.learner.loss_mode == "ppo+mask" and not evaluate:
            # the words of the minibatch's rows into the static workspace tensor the captured loss launch reads
            stable, idx_d, Bw, T = self._allowed_src
            hip.check(L.cadre_allowed_rows(hip.ptr(stable), 2 * nW, hip.ptr(idx_d), Bw, T, hip.ptr(w["pos"]) if srt else None, B,
                                           hip.ptr(self.learner._am_ws(w, B)), st), "cadre_allowed_rows")
        if self.learner.loss_mode == "ppo+smooth" and not evaluate:
            # the kinds and the partners of the minibatch's rows into the static workspace tensors the captured loss launch reads
            stable, idx_d, Bw, T = self._smooth_src
            nWs, E, rotation = self._smooth_step
            kinds, mates = self.learner._smooth_ws(w, B)
            hip.check(L.cadre_smooth_mates(hip.ptr(stable), hip.ptr(idx_d), nWs, E, Bw, T, a.C, rotation,
                                           hip.ptr(w["pos"]) if srt else None, B, hip.ptr(kinds), hip.ptr(mates), st),
                      "cadre_smooth_mates")
        if evaluate and self.learner.loss_mode == "aux":   # aux_record_from_storages: forward + the record launch only
            return self.learner.aux_record(B, sorted_rows=srt)
        if evaluate:                                     # imitate_from_storages(evaluate=True): forward + loss only
            losses, _ = self.learner.bc_evaluate(B, float(nW) / B, sorted_rows=srt, stats_row=stats_row)
            return tuple(losses.tolist()) if sync else losses.clone()
        # (nW counts the demonstration entries of a mixed step too: nW / B = 1 / rows per worker minibatch either way)
        kw = {} if demo_stats_row is None else dict(demo_stats_row=demo_stats_row)
        losses = self.learner.update(B, float(nW) / B, sorted_rows=srt, mlp_grads_ready=mlp_grads_ready, stats_row=stats_row, **kw)
        self.arena.attach_grads(self.model_dict)
        if sync:
            return tuple(losses.tolist())
        return losses.clone()

    def imitate_from_storages(self, batches, stats_row=None, sync=True, label_smoothing=None, bc_coeff=None, evaluate=False):
        """One behaviour-cloning step on demonstration rows: update_policy_from_storages (the same gather, sorted or
        unsorted, one launch, then the update) with the learner's loss switched to the imitation loss (PPOLearnerHIP.set_loss)
        for the duration of the call; the mode that was selected before is restored on exit.  `batches` as there, with the
        storages of a DemoSet (cadre_amd.imitation) and the row weights in the place of the advantages: storage.action is the
        demonstrated bin (-1: no label for that head), storage.returns the critic's target.  Gradients of all 16 nets are in
        `.grad` afterwards; the caller takes the optimiser step (chief_step / learner.clip_adam).
        `label_smoothing` / `bc_coeff`: None keeps the learner's current imitation settings.  `stats_row`: device float32
        [2][>= hip.BC_STATS_FIELDS] that receives the step's imitation statistics (accuracy, NLL, entropy, |v - R|, weight
        sum, rows counted).  `evaluate`: the evaluation form — losses and statistics only, no gradient, nothing moves."""
        with self.learner.loss_scope("bc", label_smoothing=label_smoothing, bc_coeff=bc_coeff):
            return self.update_policy_from_storages(batches, sync=sync, stats_row=stats_row, evaluate=bool(evaluate))

    # ------------------------------------------------------------------ PPG auxiliary phase (cadre_amd.phasic)
    @staticmethod
    def _aux_entry(entry):
        if len(entry) != 1:
            raise ValueError("the auxiliary phase takes exactly one gather entry (got %d): its index pair is the table's row ids"
                             % len(entry))
        return list(entry)

    def aux_record_from_storages(self, entry, table):
        """Record pass of the auxiliary phase: the gather of update_policy_from_storages (sorted or unsorted) for the ONE
        entry `entry` = [(steer_storage, steer_idx, steer_adv, throttle_storage, throttle_idx, throttle_adv)], the forward,
        then cadre_aux_record: table[head][idx] <- the current policy's normalised log-probabilities of row idx.  `table`:
        device float32 [2][R][64] with R >= every index + 1 (AuxBuffer.table).  Nothing moves; the loss mode that was
        selected before is restored on exit."""
        batches = self._aux_entry(entry)
        with self.learner.loss_scope("aux", table=table, beta_clone=None, aux_value_coeff=None):
            return self._update_from_storages(batches, False, None, None, True)

    def aux_from_storages(self, entry, table, stats_row=None, sync=True, beta_clone=None, value_coeff=None):
        """One step of the auxiliary phase on the ONE entry `entry` (as in aux_record_from_storages): the update's launch
        chain with the loss switched to cadre_aux_loss (PPOLearnerHIP.set_loss("aux")) for the duration of the call —
        value_coeff * 0.5 * mean (v - R)^2 against storage.returns + beta_clone * mean KL(table row || current policy).
        Gradients of all 16 nets are in `.grad` afterwards; the caller takes the optimiser step.  beta_clone / value_coeff:
        None keeps the learner's current settings.  `stats_row`: device float32 [2][>= hip.AUX_STATS_FIELDS] that receives
        the step's statistics (mean KL, max KL, |v - R|, entropy, (v - R)^2, rows counted).  Returns (value term, KL term, 0)."""
        batches = self._aux_entry(entry)
        with self.learner.loss_scope("aux", table=table, beta_clone=beta_clone, aux_value_coeff=value_coeff):
            return self._update_from_storages(batches, sync, None, stats_row, False)

    # ------------------------------------------------------------------ sample reuse (cadre_amd.reuse)
    def reuse_record_from_storages(self, entry, logp_now, value_now):
        """Record pass of sample reuse: the gather of update_policy_from_storages (sorted or unsorted) for the ONE entry
        `entry` = [(steer_storage, idx, steer_adv, throttle_storage, idx, throttle_adv)], the update's forward, then
        cadre_reuse_record: logp_now[head][idx] <- the current policy's log-probability of row idx's stored action,
        value_now[head][idx] <- the current critic's output.  Tables: device float32 [2][R] with R >= every index + 1
        (ReuseWindow's).  Nothing moves and the loss mode is not touched."""
        if len(entry) != 1:
            raise ValueError("the record pass takes exactly one gather entry (got %d): its index pair is the tables' row ids"
                             % len(entry))
        return self._update_from_storages(list(entry), False, None, None, True, record=(logp_now, value_now))

    def update_model(self, shared_model_list):
        """agent.py:239-243 (weight pull).  Same arena -> nothing to copy."""
        src = arena_of(shared_model_list)
        if src is not self.arena:
            self.arena.params.copy_(src.params)
        # shared arena (HIP-IPC): another process (the chief) has stepped the parameters — re-derive what is cached from them
        self.learner._wp_key = None

    # ------------------------------------------------------------------ controls
    def convert_action(self, discrete_action):
        steer = self.STEER_CONTROL[discrete_action[0].item()]
        throttle, brake = self.THROTTLE_CONTROL[discrete_action[1].item()]
        return [steer, throttle, brake]

    def avg_action(self, discrete_action_list):
        """agent.py:83-95 (eval-time ensemble)."""
        n = len(discrete_action_list)
        ctl = np.array([self.convert_action(a) for a in discrete_action_list]).mean(0).tolist()
        if n > 1 and ctl[-1] < 0.5:
            ctl[-1] = 0.0
        return ctl

    @staticmethod
    def ensemble_act(agent_group, tick_data):
        """eval.py:52-60's loop `[agent.act(obs) for agent in agent_group]` with ONE encoder pass: every
        agent of an evaluation ensemble loads the same frozen encoder checkpoint (models.py:54-70; the
        ppo_model snapshots hold no encoder), so the latent window is computed once by the first agent
        and the others run only their LSTM + heads.  Same outputs and the same global-RNG consumption
        order as the loop (agent 0 steer, agent 0 throttle, agent 1 steer, ...); refuses agents whose
        encoder weights differ.  Returns the list of `act` tuples."""
        lead = agent_group[0]
        for a in agent_group[1:]:
            if a.vae_model is not lead.vae_model and a.vae_model.fingerprint != lead.vae_model.fingerprint:
                raise ValueError("ensemble_act: agents hold different encoder weights; call act() per agent")
        feat = lead.get_latent_feature(tick_data)
        out = []
        for a in agent_group:
            f = feat if a.device == feat.device else feat.to(a.device)
            out.append(a.act_from_feature(f, tick_data["command"]))
        return out

    @staticmethod
    def ensemble_act_batch(agent_group, obs_list, shifted=None, deterministic=False, allowed=None):
        """`[CadreAgent.ensemble_act(agent_group, o) for o in obs_list]` plus `avg_action` per environment (`.controls`) in
        one launch chain per agent group: ppo_agent/evaluate.py EnsembleEvaluator.act, with one evaluator per agent group
        kept on the lead agent.  `allowed` (action masks) is refused: the ensemble sampler does not read masks.  Returns an
        EnsembleActBatch."""
        from .evaluate import ensemble_act_batch
        return ensemble_act_batch(agent_group, obs_list, shifted=shifted, deterministic=deterministic, allowed=allowed)

    # ------------------------------------------------------------------ snapshots
    def averaged_weights(self):
        """Context manager: inside it the arena holds the weight average set on the learner (cadre_amd.average.WeightAverage,
        learner.set_weight_average).  On entry ONE cadre_arena_swap puts the average where the parameters live — captured graphs
        hold addresses, so the contents move, not the pointers —, arena.params._version is bumped by an in-place no-op (as
        load_snapshot does) and the learner's packed recurrent weights are forgotten.  act, act_batch, get_value,
        ensemble_act_batch and save_snapshot work inside; update_policy*, clip_adam* and a nested entry raise CadreHipError.  On
        exit the swap is undone and the same caches are dropped, also when the body raises."""
        from ..average import averaged_weights
        return averaged_weights(self)

    def save_snapshot(self, model_path, fix_missing_lstm=False, weights="live"):
        """agent.py:245-260: pickled nn.Modules keyed by model name.  The reference writes
        steer_ppo twice and never throttle_lstm; `fix_missing_lstm=True` adds it.
        weights: "live" (the arena as it is), or "average": averaged_weights() is held around the same body, so the file has
        the reference's format unchanged and holds the weight average (CadreHipError when none is set)."""
        if weights not in ("live", "average"):
            raise ValueError("save_snapshot: weights=%r (\"live\" or \"average\")" % (weights,))
        if weights == "average" and not self.learner._avg_swapped:
            with self.averaged_weights():
                return self.save_snapshot(model_path, fix_missing_lstm)
        out = {}
        kinds = ["throttle_ppo_", "steer_ppo_", "steer_lstm_"] + (["throttle_lstm_"] if fix_missing_lstm else [])
        for c in range(self.command_num):
            for kind in kinds:
                name = kind + str(c)
                src = self.model_dict[name]
                if "lstm" in name:
                    m = LSTM(self.lstm_input, hid_size=self.lstm_input)
                else:
                    m = Model(self.lstm_input, src.control.num_outputs)
                m.load_state_dict({k: v.detach().cpu().contiguous() for k, v in src.state_dict().items()})
                out[name] = m
        torch.save(out, model_path)

    def load_snapshot(self, model_path, device):
        """agent.py:262-271."""
        if device is None:
            device = self.device
        try:
            model_dict = torch.load(model_path, map_location="cpu", weights_only=False)
            for name in model_dict:
                self.model_dict[name].load_state_dict(model_dict[name].state_dict())
            # the modules' parameters are arena views with version counters of their own: the in-place load does not move
            # arena.params._version, which keys the packed recurrent weights (learner.packed_weights) and the stacked copies
            # of an EnsembleEvaluator — an in-place no-op on the arena does
            self.arena.params[:0].zero_()
        except Exception as e:
            raise ImportError("load snapshot error due to {}".format(e))
