"""DANetDecoderHIP — the frozen encoder's decoder branches on the device (reference danet.py:164-361): from a 512-d latent to
the camera segmentation, the route mask, the traffic-light state and the behaviour-cloning controls.

    att_visual = latent[:, :256] -> visual_branch (visual_branch.py:166-217)
        reverse_feature   Linear 256 -> 512, leaky, Linear 512 -> 512 x 5 x 8                     cadre_gemm_f32 x 2
        reverse_image     4 x (ConvTranspose2d 3x3 / s2 + BatchNorm + leaky), ConvTranspose2d -> 8  cadre_deconv3x3_s2 x 4 (both modules
        reverse_route     the same down to 1 channel, sigmoid                                       in one launch), cadre_deconv3x3_s2_out x 2
        reverse_lightState  Linear 20480 -> 256 (split-K) -> 64 -> 4, leaky between                cadre_gemm_f32 x 3, cadre_splitk_reduce, cadre_argmax_rows
    att_bc = latent[:, 256:512] (+ in_bc_speed_fc(speed): Linear 1 -> 64, leaky, Linear 64 -> 256)  cadre_bc_head, one fused kernel:
        bc_branch.bc_model  Linear 256 -> 128, leaky, Linear 128 -> 2 = (steer, throttle)          K = 1 .. 256 is too small for the GEMM

Everything is fp32.  The weights are folded and packed once by the host:
  * ConvTranspose bias + eval-mode BatchNorm -> per-channel scale / shift (fold_bn, float64 rounded once);
  * ConvTranspose weights -> the four parity classes in the order the kernel consumes them (pack_deconv);
  * reverse_feature.2 writes C-H-W order in the reference (Reshape(512, 5, 8)): its weight rows and bias are permuted so that the
    GEMM's output IS the NHWC map level 1 reads, and reverse_lightState.1's input columns are permuted to match (chw_rows_to_hwc,
    chw_cols_to_hwc).  No transpose kernel runs.
"""
from collections import namedtuple

import numpy as np
import torch

from . import hip, synth

LEAKY = 0.01                   # nn.LeakyReLU() default slope
FH, FW = 5, 8                  # the reverse feature's map (visual_branch.py:66-67)
OUT_H, OUT_W = 144, 256
LEVELS = [(512, 256, 5, 8, 0, 1), (256, 128, 9, 16, 1, 1), (128, 64, 18, 32, 1, 1), (64, 32, 36, 64, 1, 1)]   # Cin, Cout, H, W, oph, opw
PREFIXES = ("visual_branch.reverse_feature.", "visual_branch.reverse_image.", "visual_branch.reverse_route.",
            "visual_branch.reverse_lightState.", "in_bc_speed_fc.", "bc_branch.bc_model.")
# modules other configurations of the reference have and the deployed one does not (visual_branch.py:99-139): ignored, and listed
IGNORED_PREFIXES = ("visual_branch.reverse_left_image.", "visual_branch.reverse_right_image.", "visual_branch.reverse_lidar.",
                    "visual_branch.reverse_topdown_rgb.", "visual_branch.reverse_topdown_seg.", "visual_branch.reverse_lightDist.")
WANT = ("seg", "route", "light", "bc")
LS_K, LS_SPLIT = FH * FW * 512, 32      # reverse_lightState.1: K = 20480 in 32 slices of 20 k-tiles

Decoded = namedtuple("Decoded", "seg seg_logits route light_logits light_state bc")

# kernel row / column of the tap that output parity p takes from neighbour d: out[2m] = x[m] w[1]; out[2m+1] = x[m] w[2] + x[m+1] w[0]
TAP_K = {(0, 0): 1, (1, 0): 2, (1, 1): 0}


def class_taps(py, px):
    """[(dy, dx, ky, kx)] of parity class (py, px) in the kernel's tap order."""
    return [(dy, dx, TAP_K[(py, dy)], TAP_K[(px, dx)]) for dy in range(py + 1) for dx in range(px + 1)]


def pack_deconv(w):
    """ConvTranspose2d weight [Cin][Cout][3][3] -> flat [9 * Cin * Cout]: classes c = 2 py + px in turn, class c as [Cout][tap][Cin]."""
    w = torch.as_tensor(w)
    parts = []
    for py in (0, 1):
        for px in (0, 1):
            blk = torch.stack([w[:, :, ky, kx].t() for _, _, ky, kx in class_taps(py, px)], dim=1)      # [Cout][tap][Cin]
            parts.append(blk.reshape(-1))
    return torch.cat(parts).contiguous()


def unpack_deconv(flat, Cin, Cout):
    """Inverse of pack_deconv -> [Cin][Cout][3][3] (every kernel tap belongs to exactly one class)."""
    flat = torch.as_tensor(flat)
    w = torch.zeros(Cin, Cout, 3, 3, dtype=flat.dtype)
    o = 0
    for py in (0, 1):
        for px in (0, 1):
            taps = class_taps(py, px)
            blk = flat[o:o + Cout * len(taps) * Cin].reshape(Cout, len(taps), Cin)
            o += blk.numel()
            for t, (_, _, ky, kx) in enumerate(taps):
                w[:, :, ky, kx] = blk[:, t, :].t()
    return w


def out_channels_padded(Cout):
    return 1 if Cout == 1 else (2 if Cout == 2 else (4 if Cout <= 4 else 8))


def pack_deconv_out(w):
    """Last level's weight [32][Cout][3][3] -> [3][3][32][CO], CO = Cout rounded up to a power of two, zeros past Cout."""
    w = torch.as_tensor(w)
    Cin, Cout = w.shape[:2]
    p = torch.zeros(3, 3, Cin, out_channels_padded(Cout), dtype=w.dtype)
    p[..., :Cout] = w.permute(2, 3, 0, 1)
    return p.contiguous()


def unpack_deconv_out(p, Cout):
    return torch.as_tensor(p)[..., :Cout].permute(2, 3, 0, 1).contiguous()


def chw_rows_to_hwc(w, C=512, H=FH, W=FW):
    """Rows (or elements of a bias) indexed c * H * W + h * W + w  ->  (h * W + w) * C + c."""
    w = torch.as_tensor(w)
    return w.reshape(C, H, W, *w.shape[1:]).permute(1, 2, 0, *range(3, w.dim() + 2)).reshape(w.shape).contiguous()


def hwc_rows_to_chw(w, C=512, H=FH, W=FW):
    w = torch.as_tensor(w)
    return w.reshape(H, W, C, *w.shape[1:]).permute(2, 0, 1, *range(3, w.dim() + 2)).reshape(w.shape).contiguous()


def chw_cols_to_hwc(w, C=512, H=FH, W=FW):
    """Columns indexed c * H * W + h * W + w  ->  (h * W + w) * C + c."""
    w = torch.as_tensor(w)
    return w.reshape(w.shape[0], C, H, W).permute(0, 2, 3, 1).reshape(w.shape).contiguous()


def hwc_cols_to_chw(w, C=512, H=FH, W=FW):
    w = torch.as_tensor(w)
    return w.reshape(w.shape[0], H, W, C).permute(0, 3, 1, 2).reshape(w.shape).contiguous()


def fold_bn(bias, gamma, beta, mean, var, eps=synth.EPS_BN):
    """ConvTranspose bias + eval-mode BatchNorm -> fp32 (scale, shift): scale = gamma / sqrt(var + eps),
    shift = beta + (bias - mean) * scale, formed in float64 and rounded once."""
    d = lambda t: torch.as_tensor(t).double()
    scale = d(gamma) / torch.sqrt(d(var) + eps)
    shift = d(beta) + (d(bias) - d(mean)) * scale
    return scale.float(), shift.float()


def has_decoder(state_dict):
    """True when the checkpoint holds every tensor of the deployed decoder branches."""
    return _first_missing(state_dict) is None


def _first_missing(state_dict):
    for k, _s, kd in synth.decoder_spec():
        if kd != "count" and k not in state_dict:
            return k
    return None


class DANetDecoderHIP:
    """decode(latent) on the device.  Weights are folded and packed once, workspaces for `max_frames` latents allocated once."""

    def __init__(self, state_dict, device="cuda:0", max_frames=64):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise hip.CadreHipError("DANetDecoderHIP needs a HIP device; there is no CPU path")
        missing = _first_missing(state_dict)
        if missing is not None:
            raise hip.CadreHipError("checkpoint has no decoder branch: key %r is missing (DANetDecoderHIP needs visual_branch.*, "
                                    "in_bc_speed_fc.* and bc_branch.* of the deployed configuration)" % missing)
        if max_frames < 1:
            raise hip.CadreHipError("max_frames must be at least 1")
        self.max_frames = MF = int(max_frames)
        for Cin, Cout, H, W, oph, opw in LEVELS:
            if not hip.lib().cadre_deconv3x3_s2_supported(2, MF, H, W, Cin, Cout, oph, opw):
                raise hip.CadreHipError("max_frames = %d: a level map of both reverse modules must stay below 2 GiB (at most 910 frames a chunk)" % MF)
        self.ignored_keys = sorted(k for k in state_dict if k.startswith(IGNORED_PREFIXES))
        sd = {}
        for k, shape, kd in synth.decoder_spec():
            if kd == "count":
                continue
            v = state_dict[k]
            v = (v if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v))).detach().float().cpu()
            if tuple(v.shape) != tuple(shape):
                raise hip.CadreHipError("decoder key %r has shape %s, the deployed configuration has %s" % (k, tuple(v.shape), tuple(shape)))
            sd[k] = v
        dev = self.device
        up = lambda t: t.contiguous().to(dev)
        vb = "visual_branch."
        # ---- dense layers: (weight [N][K], bias [N])
        self.rf1 = (up(sd[vb + "reverse_feature.0.weight"]), up(sd[vb + "reverse_feature.0.bias"]))
        self.rf2 = (up(chw_rows_to_hwc(sd[vb + "reverse_feature.2.weight"])), up(chw_rows_to_hwc(sd[vb + "reverse_feature.2.bias"])))
        self.ls = [(up(chw_cols_to_hwc(sd[vb + "reverse_lightState.1.weight"])), up(sd[vb + "reverse_lightState.1.bias"])),
                   (up(sd[vb + "reverse_lightState.3.weight"]), up(sd[vb + "reverse_lightState.3.bias"])),
                   (up(sd[vb + "reverse_lightState.5.weight"]), up(sd[vb + "reverse_lightState.5.bias"]))]
        self.sp = [(up(sd["in_bc_speed_fc.1.weight"]), up(sd["in_bc_speed_fc.1.bias"])), (up(sd["in_bc_speed_fc.3.weight"]), up(sd["in_bc_speed_fc.3.bias"]))]
        self.bc = [(up(sd["bc_branch.bc_model.1.weight"]), up(sd["bc_branch.bc_model.1.bias"])),
                   (up(sd["bc_branch.bc_model.3.weight"]), up(sd["bc_branch.bc_model.3.bias"]))]
        # ---- reverse modules: z = 0 the segmentation, z = 1 the route
        mods = (vb + "reverse_image", vb + "reverse_route")
        self.lv_w, self.lv_scale, self.lv_shift = [], [], []
        for i, (Cin, Cout, _H, _W, _oph, _opw) in enumerate(LEVELS):
            ws, scs, shs = [], [], []
            for m in mods:
                bn = "%s.%d" % (m, 3 * i + 1)
                sc, sh = fold_bn(sd["%s.%d.bias" % (m, 3 * i)], sd[bn + ".weight"], sd[bn + ".bias"], sd[bn + ".running_mean"], sd[bn + ".running_var"])
                ws.append(pack_deconv(sd["%s.%d.weight" % (m, 3 * i)]))
                scs.append(sc)
                shs.append(sh)
            self.lv_w.append(up(torch.stack(ws)))
            self.lv_scale.append(up(torch.stack(scs)))
            self.lv_shift.append(up(torch.stack(shs)))
        self.out_w = [up(pack_deconv_out(sd[m + ".12.weight"])) for m in mods]
        self.out_b = [up(sd[m + ".12.bias"]) for m in mods]
        self.seg_classes = sd[mods[0] + ".12.weight"].shape[1]
        # ---- workspaces
        buf = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.float32)
        self.h1 = buf(MF, 512)
        self.rf = buf(MF, FH * FW * 512)                     # NHWC [MF][5][8][512]
        self.maps = None                                     # level outputs, room for [2][MF][Ho][Wo][Cout] each (a chunk of n frames
                                                             # lies dense, [Z][n][Ho][Wo][Cout]); allocated by the first image decode
        self.l1, self.l2 = buf(MF, 256), buf(MF, 64)
        self.ls_slabs = buf(LS_SPLIT, MF, 256)

    def _maps(self):
        if self.maps is None:
            self.maps = [torch.empty(2 * self.max_frames * (2 * H - 1 + oph) * (2 * W - 1 + opw) * Cout, device=self.device, dtype=torch.float32)
                         for (_Cin, Cout, H, W, oph, opw) in LEVELS]
        return self.maps

    @staticmethod
    def _lin(x, lda, wb, out, F, act=0):
        w, b = wb
        N, K = w.shape
        hip.gemm(x, w, out, F, N, K, lda, K, out.stride(0), shift=b, act=act, slope=LEAKY)

    def decode(self, latent, speed=None, want=WANT, seg_logits=False):
        """latent: device fp32 tensor of F rows whose first 512 columns are the latent (row stride >= 512 floats, a multiple of 4,
        16-byte aligned rows: a FrameStorage table or a rollout storage's rows go in without a copy).  speed: None, or F current
        speeds (the reference's bc_speed).  want: which of "seg", "route", "light", "bc" to compute; only those run.
        -> Decoded(seg u8 [F,144,256], seg_logits fp32 [F,144,256,8] or None, route fp32 [F,144,256], light_logits [F,4],
        light_state int32 [F], bc fp32 [F,2] = (steer, throttle)); what was not wanted is None."""
        want = tuple(want)
        for w in want:
            if w not in WANT:
                raise hip.CadreHipError("decode: unknown output %r (want takes %s)" % (w, ", ".join(WANT)))
        if not (isinstance(latent, torch.Tensor) and latent.is_cuda and latent.dtype == torch.float32 and latent.dim() == 2):
            raise hip.CadreHipError("decode: latent must be a 2-d fp32 device tensor")
        F, ld = latent.shape[0], latent.stride(0)
        if F < 1 or latent.shape[1] < 512 or latent.stride(1) != 1 or ld < 512 or ld % 4 or latent.data_ptr() % 16:
            raise hip.CadreHipError("decode: latent needs at least one row, 512 contiguous columns, a row stride that is a multiple of 4 floats "
                                    "and 16-byte alignment")
        if latent.device != self.device:
            raise hip.CadreHipError("decode: latent is on %s, the decoder on %s" % (latent.device, self.device))
        dev = self.device
        do_seg, do_route, do_light, do_bc = ("seg" in want), ("route" in want), ("light" in want), ("bc" in want)
        if seg_logits and not do_seg:
            raise hip.CadreHipError("decode: seg_logits needs \"seg\" in want")
        if speed is not None:
            speed = torch.as_tensor(speed, dtype=torch.float32).reshape(-1).to(dev)
            if speed.numel() != F:
                raise hip.CadreHipError("decode: %d speeds for %d latents" % (speed.numel(), F))
        new = lambda shape, dt: torch.empty(shape, device=dev, dtype=dt)
        seg = new((F, OUT_H, OUT_W), torch.uint8) if do_seg else None
        logits = new((F, OUT_H, OUT_W, self.seg_classes), torch.float32) if seg_logits else None
        route = new((F, OUT_H, OUT_W), torch.float32) if do_route else None
        ll = new((F, 4), torch.float32) if do_light else None
        lstate = new((F,), torch.int32) if do_light else None
        bc = new((F, 2), torch.float32) if do_bc else None
        L = hip.lib()
        with torch.cuda.device(dev):
            for s in range(0, F, self.max_frames):
                n = min(self.max_frames, F - s)
                lat = latent[s:s + n]
                if do_seg or do_route or do_light:
                    self._lin(lat, ld, self.rf1, self.h1, n, act=2)
                    self._lin(self.h1, 512, self.rf2, self.rf, n)
                if do_seg or do_route:
                    z0, Z = (0, 2) if (do_seg and do_route) else ((0, 1) if do_seg else (1, 1))
                    maps = self._maps()
                    x, zs = self.rf, 0
                    for i, (Cin, Cout, H, W, oph, opw) in enumerate(LEVELS):
                        hip.deconv3x3_s2(x, zs, self.lv_w[i][z0:], self.lv_scale[i][z0:], self.lv_shift[i][z0:], maps[i], Z, n, H, W, Cin, Cout,
                                         oph, opw, act=2, slope=LEAKY)
                        x, zs = maps[i], n * (2 * H - 1 + oph) * (2 * W - 1 + opw) * Cout      # module z of the chunk: dense behind module z - 1
                    if do_seg:
                        hip.deconv3x3_s2_out(maps[3], self.out_w[0], self.out_b[0], None if logits is None else logits[s:s + n], seg[s:s + n],
                                             None, n, 72, 128, self.seg_classes)
                    if do_route:
                        hip.deconv3x3_s2_out(maps[3][(Z - 1) * zs:], self.out_w[1], self.out_b[1], None, None, route[s:s + n], n, 72, 128, 1)
                if do_light:
                    # K = 20480 against N = 256: split-K (the slice count a constant, so a row's sum has one order for any batch)
                    w, b = self.ls[0]
                    hip.gemm(self.rf, w, self.ls_slabs, n, 256, LS_K, LS_K, LS_K, 256, split_k=LS_SPLIT)
                    hip.check(L.cadre_splitk_reduce(hip.ptr(self.ls_slabs), LS_SPLIT, n * 256, 256, hip.ptr(self.l1), 256, n, 256, None, hip.ptr(b),
                                                    2, LEAKY, None, 0, hip.stream()), "cadre_splitk_reduce")
                    self._lin(self.l1, 256, self.ls[1], self.l2, n, act=2)
                    self._lin(self.l2, 64, self.ls[2], ll[s:s + n], n)
                    hip.check(L.cadre_argmax_rows(hip.ptr(ll[s:s + n]), 4, n, 4, hip.ptr(lstate[s:s + n]), hip.stream()), "cadre_argmax_rows")
                if do_bc:
                    (sw1, sb1), (sw2, sb2), (bw1, bb1), (bw2, bb2) = self.sp + self.bc
                    hip.check(L.cadre_bc_head(hip.ptr(lat), ld, None if speed is None else hip.ptr(speed[s:s + n]), hip.ptr(sw1), hip.ptr(sb1),
                                              hip.ptr(sw2), hip.ptr(sb2), hip.ptr(bw1), hip.ptr(bb1), hip.ptr(bw2), hip.ptr(bb2),
                                              hip.ptr(bc[s:s + n]), n, LEAKY, hip.stream()), "cadre_bc_head")
        return Decoded(seg, logits, route, ll, lstate, bc)
