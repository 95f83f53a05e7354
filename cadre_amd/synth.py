"""Seeded synthetic weights / observations for parity tests and bench.py.

There is no network and the pretrained encoder is a Google-Drive download (reference
README.md:19), so every fixture, test and benchmark uses weights regenerated from seeds.
Generation is keyed by tensor *name* (crc32(name) ^ seed) so any subset can be rebuilt
independently and the golden generator, the tests and the bench all see identical arrays.

Encoder key names / shapes follow the reference state_dict
(carla_perception/Networks/danet.py:72-110, danet_blocks/resnet.py:103-166,
danet_blocks/da_att.py:24-29,58-61, danet_blocks/intertask_att.py:39-80) restricted to the
tensors `get_latent_feature` actually reads.
"""
import zlib

import numpy as np

EPS_BN = 1e-5


def _rs(name, seed):
    return np.random.RandomState((zlib.crc32(name.encode()) ^ (seed * 2654435761)) & 0x7FFFFFFF)


def encoder_spec(feat_h, feat_w, in_ch=4):
    """[(key, shape, kind)] for the act-time encoder at a layer-4 map of feat_h x feat_w."""
    spec = []

    def conv(name, co, ci, k, bias):
        spec.append((name + ".weight", (co, ci, k, k), "conv"))
        if bias:
            spec.append((name + ".bias", (co,), "bias"))

    def bn(name, c, wkind="bn_w"):
        spec.append((name + ".weight", (c,), wkind))
        spec.append((name + ".bias", (c,), "bias"))
        spec.append((name + ".running_mean", (c,), "bias"))
        spec.append((name + ".running_var", (c,), "bn_w"))

    conv("backbone.conv1", 64, in_ch, 7, True)          # resnet.py:111-112 (bias_first=True)
    bn("backbone.bn1", 64)
    inpl = 64
    for li, planes in enumerate((64, 128, 256, 512), start=1):
        for bi in range(2):
            pre = "backbone.layer%d.%d" % (li, bi)
            stride = 2 if (li > 1 and bi == 0) else 1
            conv(pre + ".conv1", planes, inpl, 3, False)
            bn(pre + ".bn1", planes)
            conv(pre + ".conv2", planes, planes, 3, False)
            bn(pre + ".bn2", planes)
            if stride != 1 or inpl != planes:
                conv(pre + ".downsample.0", planes, inpl, 1, False)
                bn(pre + ".downsample.1", planes)
            inpl = planes
    for nm, ci in (("conv5a", 512), ("conv5c", 512), ("conv51", 128), ("conv52", 128)):
        conv("da_head.%s.0" % nm, 128, ci, 3, False)
        # small BN gain in front of PAM/CAM keeps the attention energies O(1..10) so the
        # softmaxes are neither one-hot nor uniform (a trained net's statistics do the same)
        bn("da_head.%s.1" % nm, 128, "bn_w_att" if nm in ("conv5a", "conv5c") else "bn_w")
    spec.append(("da_head.sa.gamma", (1,), "gamma"))
    conv("da_head.sa.query_conv", 16, 128, 1, True)
    conv("da_head.sa.key_conv", 16, 128, 1, True)
    conv("da_head.sa.value_conv", 128, 128, 1, True)
    spec.append(("da_head.sc.gamma", (1,), "gamma"))
    conv("da_head.conv8.1", 512, 128, 1, True)
    conv("visual_conv", 512, 512, 1, True)
    conv("bc_conv", 512, 512, 1, True)
    in_dim = 512 * feat_h * feat_w
    for br in ("visual", "bc"):
        for role in ("query", "key", "value"):
            pre = "inter_task_att.%s_%s_layer" % (br, role)
            spec.append((pre + ".1.weight", (512, in_dim), "lin"))
            spec.append((pre + ".1.bias", (512,), "bias"))
            spec.append((pre + ".3.weight", (256, 512), "lin"))
            spec.append((pre + ".3.bias", (256,), "bias"))
    return spec


def make_tensor(name, shape, kind, seed):
    r = _rs(name, seed)
    if kind == "conv":
        fan_in = shape[1] * shape[2] * shape[3]
        # slightly below He-init so 8 residual blocks keep O(1) activations
        return (r.standard_normal(shape) * np.sqrt(1.6 / fan_in)).astype(np.float32)
    if kind == "lin":
        return (r.standard_normal(shape) * np.sqrt(1.0 / shape[1])).astype(np.float32)
    if kind == "bias":
        return (r.standard_normal(shape) * 0.1).astype(np.float32)
    if kind == "bn_w":
        return r.uniform(0.6, 1.4, shape).astype(np.float32)
    if kind == "bn_w_att":
        return r.uniform(0.1, 0.3, shape).astype(np.float32)
    if kind == "gamma":
        return np.full(shape, 0.5, np.float32)      # reference inits 0 (da_att.py:29,61): would hide PAM/CAM
    raise ValueError(kind)


def encoder_state(feat_h, feat_w, seed=0):
    """dict name -> float32 ndarray (reference state_dict layout, OIHW conv weights)."""
    return {k: make_tensor(k, s, kd, seed) for k, s, kd in encoder_spec(feat_h, feat_w)}


DECODER_DIMS = (512, 256, 128, 64, 32)      # visual_branch.py:69 hidden_dims, reversed: channels of the 5x8 ... 72x128 maps


def decoder_spec():
    """[(key, shape, kind)] of the decoder branches of the deployed configuration (auto_danet.py, output mode 12), in the
    reference's state_dict order: visual_branch.reverse_feature / reverse_image / reverse_route / reverse_lightState
    (visual_branch.py:86-163), in_bc_speed_fc (danet.py:98-104) and bc_branch.bc_model (bc_branch.py:56-61).  78 keys, 8 of
    them BatchNorm `num_batches_tracked` counters (kind "count": int64 zeros, dropped by the loader).  ConvTranspose2d
    weights are [Cin][Cout][3][3]."""
    spec = []

    def lin(name, out_f, in_f):
        spec.append((name + ".weight", (out_f, in_f), "lin"))
        spec.append((name + ".bias", (out_f,), "bias"))

    def reverse_module(name, out_c):
        d = DECODER_DIMS
        for i in range(4):
            spec.append(("%s.%d.weight" % (name, 3 * i), (d[i], d[i + 1], 3, 3), "deconv"))
            spec.append(("%s.%d.bias" % (name, 3 * i), (d[i + 1],), "bias"))
            bn = "%s.%d" % (name, 3 * i + 1)
            spec.append((bn + ".weight", (d[i + 1],), "bn_w"))
            spec.append((bn + ".bias", (d[i + 1],), "bias"))
            spec.append((bn + ".running_mean", (d[i + 1],), "bias"))
            spec.append((bn + ".running_var", (d[i + 1],), "bn_w"))
            spec.append((bn + ".num_batches_tracked", (), "count"))
        spec.append((name + ".12.weight", (d[4], out_c, 3, 3), "deconv"))
        spec.append((name + ".12.bias", (out_c,), "bias"))

    lin("visual_branch.reverse_feature.0", 512, 256)
    lin("visual_branch.reverse_feature.2", 512 * 5 * 8, 512)
    reverse_module("visual_branch.reverse_image", 8)
    reverse_module("visual_branch.reverse_route", 1)
    lin("visual_branch.reverse_lightState.1", 256, 512 * 5 * 8)
    lin("visual_branch.reverse_lightState.3", 64, 256)
    lin("visual_branch.reverse_lightState.5", 4, 64)
    lin("in_bc_speed_fc.1", 64, 1)
    lin("in_bc_speed_fc.3", 256, 64)
    lin("bc_branch.bc_model.1", 128, 256)
    lin("bc_branch.bc_model.3", 2, 128)
    return spec


def decoder_state(seed=0):
    """dict name -> ndarray for decoder_spec() (float32; the counters int64), seeded by name like encoder_state."""
    out = {}
    for k, s, kd in decoder_spec():
        if kd == "count":
            out[k] = np.zeros(s, np.int64)
        elif kd == "deconv":
            # an output pixel of a stride-2 transposed 3x3 sums 9/4 taps of Cin channels on average; He gain 2 for the leaky ReLU
            # keeps the activations' spread level (1.5 at every level of the reverse modules); the last layer (".12", no BatchNorm behind
            # it) a sixteenth of that, for logits of spread 0.6: the route sigmoid stays unsaturated, and its slope times the fp32
            # reference's own logit error stays inside the 1e-6 bar the golden generator holds float64 restatements to
            gain = 0.125 if k.endswith(".12.weight") else 2.0
            out[k] = (_rs(k, seed).standard_normal(s) * np.sqrt(gain / (s[0] * 2.25))).astype(np.float32)
        else:
            out[k] = make_tensor(k, s, kd, seed)
    return out


def feat_hw(H, W):
    """layer-4 map size of the ResNet-18 trunk for an HxW input (resnet.py:111-115,152-166)."""
    def down(n, k, s, p):
        return (n + 2 * p - k) // s + 1
    h, w = down(H, 7, 2, 3), down(W, 7, 2, 3)
    h, w = down(h, 3, 2, 1), down(w, 3, 2, 1)
    for _ in range(3):
        h, w = down(h, 3, 2, 1), down(w, 3, 2, 1)
    return h, w


# ----------------------------------------------------------------------------- PPO nets
HEADS = ("steer", "throttle")


def ppo_net_spec(obs_dim=530, n_out=None, command_num=4):
    """[(model_name, param_name, shape, kind)] in reference model_dict naming
    (ppo_agent/models.py:100-125, distributions.py:34-40)."""
    n_out = n_out or {"steer": 33, "throttle": 3}
    spec = []
    for c in range(command_num):
        for hd in HEADS:
            m = "%s_ppo_%d" % (hd, c)
            for tower, last in (("control.linear", n_out[hd]), ("critic", 1)):
                spec.append((m, tower + ".0.weight", (128, obs_dim), "lin"))
                spec.append((m, tower + ".0.bias", (128,), "bias"))
                spec.append((m, tower + ".2.weight", (128, 128), "lin"))
                spec.append((m, tower + ".2.bias", (128,), "bias"))
                spec.append((m, tower + ".4.weight", (last, 128), "lin"))
                spec.append((m, tower + ".4.bias", (last,), "bias"))
            m = "%s_lstm_%d" % (hd, c)
            spec.append((m, "rnn.weight_ih", (4 * obs_dim, obs_dim), "lin"))
            spec.append((m, "rnn.weight_hh", (4 * obs_dim, obs_dim), "lin"))
            spec.append((m, "rnn.bias_ih", (4 * obs_dim,), "bias"))
            spec.append((m, "rnn.bias_hh", (4 * obs_dim,), "bias"))
    return spec


def ppo_state(seed=0, obs_dim=530, n_out=None, command_num=4):
    """{model_name: {param_name: ndarray}} — random (not orthogonal) but well-scaled, non-zero
    biases so every gradient path is exercised."""
    out = {}
    for m, p, shape, kind in ppo_net_spec(obs_dim, n_out, command_num):
        out.setdefault(m, {})[p] = make_tensor(m + "." + p, shape, kind, seed)
    return out


# ----------------------------------------------------------------------------- observations
def synth_rollout(T, H, W, seq=8, seed=1234, done_p=0.02):
    """Synthetic rollout of SURVEY.md §8(d): sliding 8-frame window (env_wrapper.py:899-904),
    u8 RGB [S,H,W,3], u8 route mask [S,W,H] (stored transposed like the reference), f64
    measurements [S,3], command, per-head reward and done flags."""
    rng = np.random.RandomState(seed)
    rgb = rng.randint(0, 256, (seq, H, W, 3)).astype(np.uint8)
    route = ((rng.rand(seq, W, H) < 0.15) * 255).astype(np.uint8)
    meas = rng.rand(seq, 3)
    steps = []
    for t in range(T):
        if t > 0:
            rgb = np.concatenate([rgb[1:], rng.randint(0, 256, (1, H, W, 3)).astype(np.uint8)], 0)
            route = np.concatenate([route[1:], ((rng.rand(1, W, H) < 0.15) * 255).astype(np.uint8)], 0)
            meas = np.concatenate([meas[1:], rng.rand(1, 3)], 0)
        steps.append(dict(rgb=rgb, route_fig=route.copy(), measurements=meas,
                          command=int(rng.randint(0, 4)),
                          reward=rng.rand(2).astype(np.float32),
                          done=(rng.rand(2) < done_p)))
    return steps
