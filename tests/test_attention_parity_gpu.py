"""GPU: the attention kernels through the C ABI against float64 on the operands as stored, EVERY stored element, at the bound of
tests/attention_parity.py: |got - y64| <= err64, every output finite, an element whose bound is zero bit-equal.  Families, sizes and cases:
tests/attention_parity.py, the same the fp32 emulation passes on the CPU (tests/test_attention_parity_cpu.py).  The default forms
(cadre_pam: pam_large_kernel at every size; cadre_cam: cam_split_kernel up to 128 positions, cam_large_kernel above; cadre_intertask_att
with ldo = 544 and 512) are checked against the bound and print one line per case; the one-workgroup forms (pam_kernel, cam_kernel:
CADRE_PAM_LARGE=0 / CADRE_CAM_SPLIT=0, read once per process) run in ONE fresh child process for all sizes up to 128 and must give the
default forms' bits on the same cases, so the bound holds for them by equality; the bf16 outputs are the fp32 results rounded once.
Output buffers start filled with a sentinel: a guard band behind what the headers say is written keeps its bits, the inputs are not
written.  PAM's qkv is a given fp32 tensor (the fp32 rounding of the float64 projection, made on the host): the GEMM has its own parity
test."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import attention_parity as ap
from tests.attention_parity import F4, SENT

pytestmark = pytest.mark.gpu
GUARD = 4096                      # sentinel elements behind the last written one
BF = torch.bfloat16


@pytest.fixture(scope="module")
def hip():
    from cadre_amd import hip as h
    h.lib()
    return h


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same_bits(t, a):
    return np.array_equal(t.cpu().numpy().view(np.uint32), np.ascontiguousarray(a).view(np.uint32))


def launch_att(hip, c, bf16=False):
    """One launch of cadre_pam / cadre_cam (or the _bf16out twin) on a case -> the output [F][Np][128] as the kernel left it (torch, on
    the host), after asserting the guard band and the inputs untouched."""
    L, st = hip.lib(), hip.stream()
    n = c.F * c.Np * 128
    x = dev(c.x)
    y = torch.full((n + GUARD,), float(SENT), device="cuda", dtype=BF if bf16 else torch.float32)
    if c.kind == "pam":
        qkv = dev(c.qkv)
        fn = L.cadre_pam_bf16out if bf16 else L.cadre_pam
        hip.check(fn(x.data_ptr(), qkv.data_ptr(), float(c.gamma), y.data_ptr(), c.F, c.Np, st), "cadre_pam")
    else:
        fn = L.cadre_cam_bf16out if bf16 else L.cadre_cam
        hip.check(fn(x.data_ptr(), float(c.gamma), y.data_ptr(), c.F, c.Np, st), "cadre_cam")
    torch.cuda.synchronize()
    assert bool((y[n:] == float(SENT)).all()), "%s: the guard band behind F * Np * 128 was written" % c.tag()
    assert same_bits(x, c.x), "%s: x was written" % c.tag()
    if c.kind == "pam":
        assert same_bits(qkv, c.qkv), "%s: qkv was written" % c.tag()
    return y[:n].reshape(c.F, c.Np, 128).cpu()


# ----------------------------------------------------------------------------- the default forms against the bound
def _id(key):
    return "%s-%d-%s" % (key[0], key[1], "+".join(key[2]))


@pytest.mark.parametrize("key", ap.case_keys("pam") + ap.case_keys("cam"), ids=_id)
def test_pam_cam_every_element_inside_the_bound(hip, key):
    c, ref = ap.att_case(*key)
    ap.check_att(launch_att(hip, c).numpy(), ref, "cadre_%s %s" % (c.kind, c.tag()))


@pytest.mark.parametrize("ldo", [544, 512])
@pytest.mark.parametrize("fams,temp", ap.it_keys())
def test_intertask_every_element_inside_the_bound(hip, fams, temp, ldo):
    c, ref = ap.it_case(fams, temp)
    rows = c.F + 3                                                               # guard rows behind F
    qkv = dev(c.qkv)
    out = torch.full((rows, ldo), float(SENT), device="cuda")
    hip.check(hip.lib().cadre_intertask_att(qkv.data_ptr(), out.data_ptr(), ldo, c.F, float(F4(temp)), hip.stream()), "cadre_intertask_att")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[c.F:] == SENT).all(), "%s: rows behind F were written" % c.tag()
    assert (got[:c.F, 512:] == SENT).all(), "%s: columns 512 .. ldo-1 were written" % c.tag()
    assert same_bits(qkv, c.qkv), "%s: qkv was written" % c.tag()
    ap.check_att(got[:c.F, :512], ref, "cadre_intertask_att ldo %d %s" % (ldo, c.tag()))


# ----------------------------------------------------------------------------- the one-workgroup forms: the same bits
CHILD = """
import sys, torch
sys.path.insert(0, %r)
from cadre_amd import hip
L = hip.lib()
cases = torch.load(%r)
out = {}
for k, d in cases.items():
    x = d['x'].cuda(); y = torch.empty_like(x)
    if d['kind'] == 'pam':
        q = d['qkv'].cuda()
        hip.check(L.cadre_pam(x.data_ptr(), q.data_ptr(), d['gamma'], y.data_ptr(), d['F'], d['Np'], hip.stream()), 'pam')
    else:
        hip.check(L.cadre_cam(x.data_ptr(), d['gamma'], y.data_ptr(), d['F'], d['Np'], hip.stream()), 'cam')
    torch.cuda.synchronize()
    out[k] = y.cpu()
torch.save(out, %r)
"""


def test_one_workgroup_forms_give_the_default_forms_bits(hip, tmp_path):
    """pam_kernel and cam_kernel on every case up to 128 positions: one child process launches and saves, the parent compares."""
    cases, want = {}, {}
    for kind in ("pam", "cam"):
        for key in ap.case_keys(kind, small_only=True):
            if key[1] > 128:
                continue
            c, _ = ap.att_case(*key)
            name = "%s %d %s" % (kind, c.Np, "/".join(c.fams))
            want[name] = launch_att(hip, c)
            cases[name] = dict(kind=kind, x=torch.from_numpy(c.x), qkv=None if c.qkv is None else torch.from_numpy(c.qkv),
                               gamma=float(c.gamma), F=c.F, Np=c.Np)
    io_in, io_out = str(tmp_path / "in.pt"), str(tmp_path / "out.pt")
    torch.save(cases, io_in)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", CHILD % (root, io_in, io_out)], env=dict(os.environ, CADRE_PAM_LARGE="0", CADRE_CAM_SPLIT="0"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-300:], r.stderr[-500:])
    got = torch.load(io_out)
    assert sorted(got) == sorted(want)
    bad = [k for k in want if not torch.equal(got[k].view(torch.int32), want[k].view(torch.int32))]
    assert not bad, "one-workgroup forms differ from the default forms on: %s" % bad


# ----------------------------------------------------------------------------- the bf16 outputs
@pytest.mark.parametrize("Np", [33, 129])
@pytest.mark.parametrize("kind", ["pam", "cam"])
def test_bf16_outputs_are_the_fp32_results_rounded_once(hip, kind, Np):
    """cadre_pam_bf16out / cadre_cam_bf16out on the peaked and relu families (one in each of the size's two cases)."""
    for key in [k for k in ap.case_keys(kind) if k[1] == Np]:
        c, _ = ap.att_case(*key)
        y32, y16 = launch_att(hip, c), launch_att(hip, c, bf16=True)
        assert torch.equal(y16.view(torch.int16), y32.to(BF).view(torch.int16)), c.tag()
