"""Latency of DANetDecoderHIP.decode for F = 1, 8, 64 and 1024 latents: all outputs, the class map only, and ("bc",), with the time
per level, beside the same chain written with torch.nn.functional.conv_transpose2d / linear on the device (in this tool only: the
product never runs it).

Each form is timed with HIP events around --reps back-to-back calls, --runs runs per form after a warm-up, the forms of one F
alternating; the median is reported with min and max.  The per-level times come from a separate pass with cadre_amd.hip.PROFILE
(HIP events around every launch, --runs medians), with the level kernels' rate by the tool's own count of EXECUTED FLOPs
(9 taps x Cin x Cout per input position and module: a tap the map's edge does not have is multiplied as zeros) against the fp32
matrix-pipe peak of MI355X_MICROARCH.md (v_mfma_f32_32x32x2_f32: 256 FLOP / clk / CU x 256 CUs x 2.4 GHz = 157.3 TFLOP/s).

    python tools/decode_bench.py [--runs 20] [--reps 10] [--out profiles/decode_latency.txt]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as Fn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_F32_MFMA = 157.3e12
SIZES = (1, 8, 64, 1024)


class TorchChain:
    """The decoder as library calls on the device (NCHW, eval-mode BatchNorm folded to scale / shift like the product)."""

    def __init__(self, sd, dev):
        t = lambda k: torch.from_numpy(np.ascontiguousarray(sd[k])).to(dev)
        self.t = t
        vb = "visual_branch."
        self.lin = {n: (t(n + ".weight"), t(n + ".bias")) for n in
                    [vb + "reverse_feature.0", vb + "reverse_feature.2", vb + "reverse_lightState.1", vb + "reverse_lightState.3",
                     vb + "reverse_lightState.5", "bc_branch.bc_model.1", "bc_branch.bc_model.3"]}
        from cadre_amd import decoder
        self.mods = {}
        for m in (vb + "reverse_image", vb + "reverse_route"):
            lv = []
            for i in range(4):
                bn = "%s.%d" % (m, 3 * i + 1)
                sc, sh = decoder.fold_bn(sd["%s.%d.bias" % (m, 3 * i)], sd[bn + ".weight"], sd[bn + ".bias"], sd[bn + ".running_mean"], sd[bn + ".running_var"])
                lv.append((t("%s.%d.weight" % (m, 3 * i)), sc.to(dev).view(1, -1, 1, 1), sh.to(dev).view(1, -1, 1, 1)))
            self.mods[m] = (lv, t(m + ".12.weight"), t(m + ".12.bias"))

    def module(self, m, rf):
        lv, w, b = self.mods[m]
        x = rf
        for i, (wi, sc, sh) in enumerate(lv):
            x = Fn.leaky_relu(Fn.conv_transpose2d(x, wi, None, 2, 1, (0, 1) if i == 0 else 1) * sc + sh)
        return Fn.conv_transpose2d(x, w, b, 2, 1, 1)

    def decode(self, lat, what):
        vb = "visual_branch."
        L = lambda x, n: Fn.linear(x, *self.lin[n])
        out = []
        if what != "bc":
            rf = L(Fn.leaky_relu(L(lat[:, :256], vb + "reverse_feature.0")), vb + "reverse_feature.2").view(-1, 512, 5, 8)
            out.append(self.module(vb + "reverse_image", rf).argmax(1).to(torch.uint8))
        if what == "all":
            out.append(torch.sigmoid(self.module(vb + "reverse_route", rf)))
            l = Fn.leaky_relu(L(rf.flatten(1), vb + "reverse_lightState.1"))
            out.append(L(Fn.leaky_relu(L(l, vb + "reverse_lightState.3")), vb + "reverse_lightState.5").argmax(1))
        if what in ("all", "bc"):
            out.append(L(Fn.leaky_relu(L(lat[:, 256:512], "bc_branch.bc_model.1")), "bc_branch.bc_model.3"))
        return out


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--max-frames", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("decode_bench needs an MI355X: a time taken elsewhere says nothing")
    from cadre_amd import decoder, hip, synth
    dev = torch.device("cuda:0")
    sd = synth.decoder_state(7)
    dec = decoder.DANetDecoderHIP(sd, dev, max_frames=args.max_frames)
    ref = TorchChain(sd, dev)
    lines = ["DANetDecoderHIP.decode latency (%s; max_frames %d; median of %d runs x %d back-to-back calls per form, forms alternating, HIP events; "
             "call-to-call time, launch overhead and output allocation included)" % (torch.cuda.get_device_name(0), args.max_frames, args.runs, args.reps)]
    forms = [("all", dict(want=("seg", "route", "light", "bc"))), ("seg", dict(want=("seg",))), ("bc", dict(want=("bc",)))]
    names = {"all": "all outputs", "seg": "class map only", "bc": '("bc",)'}
    for F in SIZES:
        lat = torch.from_numpy((np.random.RandomState(F).standard_normal((F, 544)) * 0.5).astype(np.float32)).to(dev)
        reps = max(1, args.reps // (16 if F >= 1024 else 1))
        calls = []
        for key, kw in forms:
            calls.append(("hip", key, (lambda kw=kw: dec.decode(lat, **kw))))
            calls.append(("torch", key, (lambda key=key: ref.decode(lat, key))))
        for _ in range(args.warmup):
            for _, _, fn in calls:
                fn()
        torch.cuda.synchronize()
        ts = {(a, b): [] for a, b, _ in calls}
        for _ in range(args.runs):
            for a, b, fn in calls:
                ts[(a, b)].append(timed(fn, reps))
        # the two chains agree (the tool's comparison is of like with like)
        mine, theirs = dec.decode(lat[:8]), ref.decode(lat[:8], "all")
        agree = float((mine.seg != theirs[0]).double().mean())
        lines.append("F = %d   (class maps of the two chains differ at %.4f %% of the pixels)" % (F, 100 * agree))
        for key, _ in forms:
            h, t = ts[("hip", key)], ts[("torch", key)]
            lines.append("  %-16s HIP %9.3f ms  (min %.3f max %.3f; %.3f ms / frame)   torch.nn.functional %9.3f ms  (min %.3f max %.3f)   ratio %.2f"
                         % (names[key], statistics.median(h), min(h), max(h), statistics.median(h) / F, statistics.median(t), min(t), max(t),
                            statistics.median(t) / statistics.median(h)))
        # per launch: a pass of its own with the profiling hook
        per = {}
        for _ in range(max(3, args.runs // 2)):
            hip.PROFILE = []
            dec.decode(lat)
            torch.cuda.synchronize()
            acc = {}
            for key, flops, e0, e1, shape, nbytes in hip.PROFILE:
                k = key if key[0] in ("deconv", "deconv_out") else ("gemm",) + tuple(shape[:3])
                a = acc.setdefault(k, [0.0, 0.0, 0])
                a[0] += e0.elapsed_time(e1)
                a[1] += flops
                a[2] += 1
            hip.PROFILE = None
            for k, a in acc.items():
                per.setdefault(k, []).append(a)
        lines.append("  per level, all outputs (events around every launch, summed over the call's %d chunk(s)):" % -(-F // args.max_frames))
        tot_t = tot_f = 0.0
        for k, runs in per.items():
            ms = statistics.median(r[0] for r in runs)
            fl, n = runs[0][1], runs[0][2]
            if k[0] == "deconv":
                tot_t, tot_f = tot_t + ms, tot_f + fl
                lines.append("    cadre_deconv3x3_s2 %3d -> %3d (both modules)   %8.3f ms in %d launch(es)   %6.2f TFLOP/s executed = %4.1f %% of the fp32 matrix pipe"
                             % (k[1], k[2], ms, n, fl / ms / 1e9, 100 * fl / (ms * 1e-3) / PEAK_F32_MFMA))
            elif k[0] == "deconv_out":
                lines.append("    cadre_deconv3x3_s2_out 32 -> %d               %8.3f ms in %d launch(es)" % (k[1], ms, n))
            else:
                lines.append("    cadre_gemm_f32 M %d N %d K %d                  %8.3f ms in %d launch(es)" % (k[1], k[2], k[3], ms, n))
        if tot_t:
            lines.append("    the four level kernels together: %.3f ms, %.2f TFLOP/s executed = %.1f %% of the fp32 matrix pipe (%.1f TFLOP/s)"
                         % (tot_t, tot_f / tot_t / 1e9, 100 * tot_f / (tot_t * 1e-3) / PEAK_F32_MFMA, PEAK_F32_MFMA / 1e12))
    lines.append("  (cadre_splitk_reduce behind the K = 20480 product, cadre_argmax_rows and cadre_bc_head carry no profiling hook: they are in the call times above, not in the per-level lists)")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
