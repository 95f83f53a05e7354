#!/usr/bin/env python3
"""Generate tests/golden/decode_native.npz: the UNMODIFIED reference DANet's decoder branches (forward / get_bc_actions,
danet.py:164-291) on the two native-size frames of enc_native.npz.  Build-container only, like make_golden.py:

    python -B tests/golden/make_decode_golden.py

The encoder weights are synth.encoder_state (as in enc_native.npz), the decoder keys are overwritten with synth.decoder_state.
The fixture holds data only: the list of decoder key names and shapes, the small outputs whole, and a subsample of the large maps
(tests/decode_ref.py subsample: rows of both parities with the first and last ones, whole rows; every fourth channel of the two
intermediate maps).  tests/decode_ref.py's float64 restatement is compared here; a mismatch aborts generation.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.dont_write_bytecode = True

import numpy as np
import torch

import make_golden as mg
from cadre_amd import synth
from oracle import encoder_ref
from tests import decode_ref

SPEEDS = (3.0, 0.5)
PREFIXES = ("visual_branch.", "in_bc_speed_fc.", "bc_branch.")


def main():
    enc = np.load(os.path.join(HERE, "enc_native.npz"))
    H, W, n = int(enc["H"]), int(enc["W"]), int(enc["n"])
    net, _, _ = mg.ref_danet(5, 8, int(enc["seed"]))
    dec = synth.decoder_state(int(enc["seed"]))
    sd = net.state_dict()
    ref_keys = [k for k in sd if k.startswith(PREFIXES)]
    assert ref_keys == [k for k, _, _ in synth.decoder_spec()], "decoder_spec() is not the reference's key list"
    for k, v in dec.items():
        assert tuple(sd[k].shape) == v.shape, (k, v.shape)
        sd[k] = torch.from_numpy(v)
    net.load_state_dict(sd)
    net.eval()
    rgb, route = mg.frames(n, H, W, int(enc["frame_seed"]))
    x, _ = encoder_ref.pre_process(rgb, route)
    xt = torch.from_numpy(x)
    speed = torch.tensor(SPEEDS, dtype=torch.float32).reshape(n, 1)
    with torch.no_grad():
        lat = net.get_latent_feature(xt, "concate")
        assert np.array_equal(lat.numpy(), enc["latent"]), "the latent is not enc_native.npz's"
        light, _, seg, _, _, rt, _, _, steer, throttle = net(xt, speed)
        steer0, throttle0 = net.get_bc_actions(xt, None)
        vb = net.visual_branch
        rf = vb.reverse_feature(lat[:, :256])
        seg1 = vb.reverse_image[:3](rf)
    ref = dict(rf=rf, seg1=seg1, seg=seg, route=rt, light=light, steer=steer, throttle=throttle)
    print("reference shapes:", {k: tuple(v.shape) for k, v in ref.items()})
    got = decode_ref.subsample(ref)
    o = decode_ref.decode(dec, lat, speed)
    o0 = decode_ref.decode(dec, lat, None)
    mine = decode_ref.subsample(o)
    for k in got:
        mg.close(mine[k], got[k], 1e-6, "decode " + k)
    mg.close(o0["steer"], steer0, 1e-6, "decode steer (no speed)")
    mg.close(o0["throttle"], throttle0, 1e-6, "decode throttle (no speed)")
    # share of segmentation positions whose float64 top-two margin is below 1e-5 of the largest logit
    top2 = torch.topk(o["seg"], 2, dim=1).values
    print("  seg top-two margin < 1e-5 max|logit|: %.4f %% of positions" %
          (100.0 * float(((top2[:, 0] - top2[:, 1]) < 1e-5 * o["seg"].abs().max()).double().mean())))
    spec = synth.decoder_spec()
    path = os.path.join(HERE, "decode_native.npz")
    np.savez_compressed(path, seed=int(enc["seed"]), speeds=np.array(SPEEDS, np.float32), keys=np.array([k for k, _, _ in spec]),
                        shapes=np.array([",".join(str(d) for d in s) for _, s, _ in spec]), rows_out=decode_ref.ROWS_OUT,
                        ch_step=decode_ref.CH_STEP, steer_nospeed=steer0.numpy(), throttle_nospeed=throttle0.numpy(),
                        light_state=light.argmax(1).numpy().astype(np.int32), **{k: np.ascontiguousarray(v) for k, v in got.items()})
    print("wrote %s (%.1f KB)" % (path, os.path.getsize(path) / 1024.0))
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(HERE, "enc_288.npz"))


if __name__ == "__main__":
    main()
