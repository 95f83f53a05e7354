"""Float64 restatement of the reference's decoder branches on torch CPU tensors: VisualBranch.forward (visual_branch.py:166-217),
BCBranch.forward (bc_branch.py:63-81) and the speed path of DANet.forward (danet.py:176-181), plus the per-stage helpers the GPU test
needs (value y64 and magnitude mag of one level from operands as stored).

The transposed convolution is written out as what it is, not taken from torch.nn.functional:  ConvTranspose2d(k 3, stride 2,
padding 1) puts input pixel i through kernel tap k at output 2 i - 1 + k, so

    out[2m]   = x[m] w[1]                         (one tap)
    out[2m+1] = x[m] w[2] + x[m+1] w[0]           (two taps; x[H] is outside the map and contributes nothing)

along each axis: four output-parity classes with 1, 2, 2 and 4 taps.  The output has 2 H - 1 + output_padding rows: the last odd
row exists only with output_padding 1 and then has the single in-range tap.  Weights are [Cin][Cout][3][3] as the reference stores
them; activations NHWC unless a function says otherwise.
"""
import numpy as np
import torch

from tests.bf16_parity import f64
from tests import f32_parity as fp

SLOPE = 0.01
EPS_BN = 1e-5
KTAP = {(0, 0): 1, (1, 0): 2, (1, 1): 0}          # (output parity, neighbour offset) -> kernel index
DIMS = (512, 256, 128, 64, 32)


def class_taps(py, px):
    return [(dy, dx, KTAP[(py, dy)], KTAP[(px, dx)]) for dy in range(py + 1) for dx in range(px + 1)]


def out_hw(H, W, oph, opw):
    return 2 * H - 1 + oph, 2 * W - 1 + opw


def deconv_acc(x, w, oph, opw, drop=None):
    """x [F][H][W][Cin], w [Cin][Cout][3][3] -> (sum, sum of |a||b|) float64 [F][Ho][Wo][Cout], as the four parity sums.
    drop = (py, px, dy, dx): that tap of that class is left out (a mutant for the tests of the bound)."""
    xd, wd = f64(x), f64(w)
    Fn, H, W, _ = xd.shape
    Cout = wd.shape[1]
    Ho, Wo = out_hw(H, W, oph, opw)
    acc = torch.zeros(Fn, Ho, Wo, Cout, dtype=torch.float64)
    mac = torch.zeros_like(acc)
    for py in (0, 1):
        for px in (0, 1):
            nr, nc = len(range(py, Ho, 2)), len(range(px, Wo, 2))          # outputs 2m+py < Ho, 2n+px < Wo
            for dy, dx, ky, kx in class_taps(py, px):
                if drop == (py, px, dy, dx):
                    continue
                rows, cols = min(nr, H - dy), min(nc, W - dx)             # neighbours inside the map
                if rows <= 0 or cols <= 0:
                    continue
                src = xd[:, dy:dy + rows, dx:dx + cols]
                wk = wd[:, :, ky, kx]
                acc[:, py::2, px::2][:, :rows, :cols] += torch.einsum("fmnc,co->fmno", src, wk)
                mac[:, py::2, px::2][:, :rows, :cols] += torch.einsum("fmnc,co->fmno", src.abs(), wk.abs())
    return acc, mac


def deconv_products(x, w, oph, opw):
    """-> (products(flat output indices) = [S][4 * Cin] fp32: the four neighbour slots (dy, dx) of the output's class, zeros where the
    class has no such tap or the neighbour is outside the map; K = 4 * Cin; n_out).  Output layout [F][Ho][Wo][Cout] flat."""
    xf = x.detach().cpu().float()
    Fn, H, W, Cin = xf.shape
    Cout = w.shape[1]
    Ho, Wo = out_hw(H, W, oph, opw)
    xp = torch.zeros(Fn, H + 1, W + 1, Cin)
    xp[:, :H, :W] = xf
    xp = xp.numpy()
    wt = np.zeros((2, 2, 2, 2, Cout, Cin), np.float32)                    # [py][px][dy][dx][co][ci]
    wn = w.detach().cpu().float().numpy()
    for py in (0, 1):
        for px in (0, 1):
            for dy, dx, ky, kx in class_taps(py, px):
                wt[py, px, dy, dx] = wn[:, :, ky, kx].T
    dyy, dxx = np.meshgrid(np.arange(2), np.arange(2), indexing="ij")

    def products(idx):
        co = idx % Cout
        ox = idx // Cout % Wo
        oy = idx // (Cout * Wo) % Ho
        f = idx // (Cout * Wo * Ho)
        patch = xp[f[:, None, None], (oy // 2)[:, None, None] + dyy, (ox // 2)[:, None, None] + dxx]      # [S][2][2][Cin]
        return (patch * wt[oy % 2, ox % 2, :, :, co]).reshape(len(idx), -1)
    return products, 4 * Cin, Fn * Ho * Wo * Cout


def level_ref(x, w, scale, shift, oph, opw, act=0, slope=SLOPE, drop=None):
    """One decoder level from operands as stored (fp32 x, the reference-layout fp32 weight, the folded fp32 scale / shift):
    -> (y64, mag) [F][Ho][Wo][Cout]."""
    acc, mac = deconv_acc(x, w, oph, opw, drop)
    return fp.epilogue32(acc, mac, scale, shift, None, act, slope)


def level_c_bar(x, w, y64, mag, scale, shift, oph, opw, act=0, slope=SLOPE, what=""):
    """(c_bar, cap) of one level: the sequential fp32 chain over the case's own products, K = 4 * Cin for the cap."""
    return fp.c_bar_direct([deconv_products(x, w, oph, opw)], y64, mag, scale, shift, None, act, slope, what=what)


def fold_bn64(bias, gamma, beta, mean, var, eps=EPS_BN):
    scale = f64(gamma) / torch.sqrt(f64(var) + eps)
    return scale, f64(beta) + (f64(bias) - f64(mean)) * scale


def leaky(t, slope=SLOPE):
    return torch.where(t < 0, t * slope, t)


def linear(x, sd, name):
    return x @ f64(sd[name + ".weight"]).t() + f64(sd[name + ".bias"])


def reverse_module(rf_nhwc, sd, name, taps=None):
    """build_reverse_module's Sequential (visual_branch.py:141-163) in eval mode, before the sigmoid: [F][5][8][512] ->
    [F][144][256][out].  taps: a dict that receives the level outputs "<name>.<level>"."""
    x = rf_nhwc
    for i in range(4):
        acc, _ = deconv_acc(x, sd["%s.%d.weight" % (name, 3 * i)], 0 if i == 0 else 1, 1)
        bn = "%s.%d" % (name, 3 * i + 1)
        sc, sh = fold_bn64(sd["%s.%d.bias" % (name, 3 * i)], sd[bn + ".weight"], sd[bn + ".bias"], sd[bn + ".running_mean"], sd[bn + ".running_var"])
        x = leaky(acc * sc + sh)
        if taps is not None:
            taps["%s.%d" % (name, i + 1)] = x
    acc, _ = deconv_acc(x, sd[name + ".12.weight"], 1, 1)
    return acc + f64(sd[name + ".12.bias"])


def decode(sd, latent, speed=None):
    """The decoder branches in float64.  sd: reference-named tensors (synth.decoder_state or a checkpoint), latent [F][>=512],
    speed None or [F].  -> dict of float64 tensors in the REFERENCE's layouts: rf [F][512][5][8], seg1 [F][256][9][16] (level-1 output
    of the segmentation module), seg [F][8][144][256] logits, route [F][1][144][256] after the sigmoid, light [F][4], steer [F],
    throttle [F]."""
    lat = f64(latent)
    vb = "visual_branch."
    av, ab = lat[:, :256], lat[:, 256:512]
    h = leaky(linear(av, sd, vb + "reverse_feature.0"))
    rf = linear(h, sd, vb + "reverse_feature.2").reshape(-1, 512, 5, 8)
    rf_nhwc = rf.permute(0, 2, 3, 1).contiguous()
    taps = {}
    seg = reverse_module(rf_nhwc, sd, vb + "reverse_image", taps)
    route = torch.sigmoid(reverse_module(rf_nhwc, sd, vb + "reverse_route"))
    flat = rf.reshape(rf.shape[0], -1)
    l = leaky(linear(flat, sd, vb + "reverse_lightState.1"))
    l = leaky(linear(l, sd, vb + "reverse_lightState.3"))
    light = linear(l, sd, vb + "reverse_lightState.5")
    if speed is not None:
        s = f64(speed).reshape(-1, 1)
        ab = ab + linear(leaky(linear(s, sd, "in_bc_speed_fc.1")), sd, "in_bc_speed_fc.3")
    bc = linear(leaky(linear(ab, sd, "bc_branch.bc_model.1")), sd, "bc_branch.bc_model.3")
    nchw = lambda t: t.permute(0, 3, 1, 2).contiguous()
    return dict(rf=rf, seg1=nchw(taps[vb + "reverse_image.1"]), seg=nchw(seg), route=nchw(route), light=light,
                steer=bc[:, 0], throttle=bc[:, 1])


# the golden's subsample of the large maps (tests/golden/make_decode_golden.py): both row parities, the first and last rows, whole
# rows (so the first and last columns); every fourth channel of the two intermediate maps
ROWS_OUT = np.array([0, 1, 2, 3, 70, 71, 72, 73, 142, 143])
CH_STEP = 4


def subsample(out):
    """dict of decode() (or the reference's arrays in the same layouts) -> the arrays the golden stores."""
    a = lambda t: t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return dict(rf=a(out["rf"])[:, ::CH_STEP], seg1=a(out["seg1"])[:, ::CH_STEP], seg=a(out["seg"])[:, :, ROWS_OUT],
                route=a(out["route"])[:, :, ROWS_OUT], light=a(out["light"]), steer=a(out["steer"]), throttle=a(out["throttle"]))


def rel_max(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def sigmoid_f32(v):
    """fp32 numpy emulation of the output kernel's sigmoid: e = exp(-|v|); 1 / (1 + e) for v >= 0, e / (1 + e) below."""
    v = np.asarray(v, np.float32)
    e = np.exp(-np.abs(v)).astype(np.float32)
    one = np.float32(1)
    r = np.where(v >= 0, one, e) / (one + e)
    assert r.dtype == np.float32
    return r
