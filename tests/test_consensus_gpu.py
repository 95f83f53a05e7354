"""GPU: rank consensus (train_cfg["rank_consensus"]) — the two kernels of csrc/consensus.hip against their host mirrors
(tests/consensus_ref.py), and the consensus path of the learner section with the collectives really issued: at world 1
against the loss kernel's own decision (bit for bit), at world 2 (two fresh processes on cuda:0 over gloo,
tests/consensus_ranks_driver.py) against ONE rank that holds both workers and decides in the loss kernel.  No run on two
GPUs exists: what is shown is that ranks that receive the same reduced bits decide alike, and decide what one rank would.

The driver is spawned once per world size (module-scoped fixtures); every scenario runs inside those two spawns."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import consensus_ref as ref
from tests import consensus_ranks_driver as drv

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KL_TOL = 2e-6             # 1e-6 (the bar of test_stats_match_oracle for one worker's approx_kl) per summed worker
PARAM_SUM_TOL = 1e-5      # per-model parameter sums: the bar of tests/test_dp_gpu.py for this same comparison
LOSS_TOL = 1e-4
PERM_SEED = 33
STORAGE_SEED = 21         # rank r: storages(64, 2, 21 + r); the conditioning asserts below hold for it


def rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def spawn(out_dir, world):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "CADRE_BENCH_FORCE_DIST"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, "-m", "tests.consensus_ranks_driver", str(out_dir), str(world)], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=drv.SPAWN_TIMEOUT + 60)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("CONSENSUS_RESULT ")]
    assert p.returncode == 0 and lines, "ranks failed rc=%s\nstdout:\n%s\nstderr:\n%s" % (p.returncode, p.stdout[-3000:], p.stderr[-8000:])
    assert json.loads(lines[-1][len("CONSENSUS_RESULT "):])["exitcodes"] == [0] * world
    return [np.load(os.path.join(str(out_dir), "rank%d.npz" % r)) for r in range(world)]


def scen(npz, name):
    return {k[len(name) + 1:]: npz[k] for k in npz.files if k.startswith(name + "/")}


# ----------------------------------------------------------------------------- 1. cadre_kl_consensus == the mirror
def test_kl_consensus_kernel_matches_the_mirror_bit_for_bit():
    """The whole decision table: stop flag, hp[LR] as float64 bits, field 6 of both heads; every other field of the row and
    of the block keeps its (NaN) filling."""
    from cadre_amd import hip
    L = hip.lib()
    F = hip.PPO_STATS_FIELDS + 8
    for name, kl, tkl, stop, desired, lr0 in ref.decision_table():
        hp_host = ref.hp_block(lr=lr0, fill=np.nan)
        want = ref.kl_rule(kl, tkl, stop, desired, hp_host)
        kl_d = torch.tensor([float(kl[0]), float(kl[1]), 0.0, 0.0], dtype=torch.float32, device="cuda:0")
        stop_d = None if stop is None else torch.tensor([stop], dtype=torch.int32, device="cuda:0")
        hp_d = torch.from_numpy(hp_host.copy()).cuda()
        row = torch.full((2, F), float("nan"), device="cuda:0")
        hip.check(L.cadre_kl_consensus(hip.ptr(kl_d), float(tkl), hip.ptr(stop_d), float(desired), hip.ptr(hp_d), hip.ptr(row), F,
                                       hip.stream()), "cadre_kl_consensus")
        torch.cuda.synchronize()
        if stop is not None:
            assert int(stop_d.item()) == want[0], name
        got_hp, got_row = hp_d.cpu().numpy(), row.cpu().numpy()
        assert got_hp[ref.HP_LR].view(np.int64) == np.float64(want[2]).view(np.int64), (name, got_hp[ref.HP_LR], want[2])
        assert got_row[0, 6] == got_row[1, 6] == want[1], name
        keep_hp = np.ones(16, bool); keep_hp[ref.HP_LR] = False
        assert np.array_equal(got_hp[keep_hp].view(np.int64), hp_host[keep_hp].view(np.int64)), name
        keep_row = np.ones((2, F), bool); keep_row[:, 6] = False
        assert np.isnan(got_row[keep_row]).all(), name
        assert np.array_equal(kl_d.cpu().numpy().view(np.int32), np.array([kl[0], kl[1], 0, 0], dtype=np.float32).view(np.int32))
        # without a row and without a block: the flag alone
        if stop is not None:
            stop2 = torch.tensor([stop], dtype=torch.int32, device="cuda:0")
            hip.check(L.cadre_kl_consensus(hip.ptr(kl_d), float(tkl), hip.ptr(stop2), 0.0, None, None, 0, hip.stream()),
                      "cadre_kl_consensus")
            assert int(stop2.item()) == want[0], name


# ----------------------------------------------------------------------------- 2. cadre_return_scale_merge
@pytest.mark.parametrize("world", [1, 2, 5])
def test_return_scale_merge(world):
    from cadre_amd import hip
    L = hip.lib()
    eps = 1e-8
    stats = ref.rank_stats(ref.merge_cases()[world])
    assert (stats[:, 0] == 0).any() or (stats[:, 3] == 0).any() or world == 1        # (one rank / head with count 0)
    want = ref.chan_merge(stats)
    n_state = hip.RS_CARRY + 4
    state = torch.full((n_state + 4,), float("nan"), dtype=torch.float64, device="cuda:0")     # NaN neighbourhood
    state[2 + hip.RS_SCALE:2 + hip.RS_CARRY] = 1.0
    view = state[2:2 + n_state]
    before = state.cpu().numpy().copy()
    merged = torch.full((6,), float("nan"), dtype=torch.float64, device="cuda:0")
    st_d = torch.from_numpy(stats).cuda()
    hip.check(L.cadre_return_scale_merge(hip.ptr(st_d), world, eps, hip.ptr(view), hip.ptr(merged), hip.stream()),
              "cadre_return_scale_merge")
    torch.cuda.synchronize()
    got_m, after = merged.cpu().numpy(), state.cpu().numpy()
    for g, w in zip(got_m, want):
        assert abs(g - w) <= 1e-12 * abs(w), (world, got_m, want)
    for h, w in enumerate(ref.scale_of(want, eps)):
        g = after[2 + hip.RS_SCALE + h]
        assert np.float32(g) == g, "the slot holds a float32 value"
        assert np.float32(g) in (w, np.nextafter(w, np.float32(0)), np.nextafter(w, np.float32(np.inf))), (world, h, g, w)
        assert np.float32(g) == np.float32(1.0 / np.sqrt(got_m[3 * h + 2] / got_m[3 * h] + eps))      # (from the device's own merge: exact)
    keep = np.ones(len(after), bool); keep[2 + hip.RS_SCALE:2 + hip.RS_CARRY] = False
    assert np.array_equal(after[keep].view(np.int64), before[keep].view(np.int64)), "state outside the two scale slots was written"
    assert np.array_equal(st_d.cpu().numpy(), stats)
    # merged may be NULL; all counts 0: the scale slots stay as they are
    view2 = torch.full((n_state,), 7.0, dtype=torch.float64, device="cuda:0")
    hip.check(L.cadre_return_scale_merge(hip.ptr(torch.zeros(world, 6, dtype=torch.float64, device="cuda:0")), world, eps,
                                         hip.ptr(view2), None, hip.stream()), "cadre_return_scale_merge")
    assert (view2.cpu() == 7.0).all()
    hip.check(L.cadre_return_scale_merge(hip.ptr(st_d), world, eps, hip.ptr(view2), None, hip.stream()), "cadre_return_scale_merge")
    assert torch.equal(view2[hip.RS_SCALE:hip.RS_CARRY].cpu(), torch.from_numpy(after[2 + hip.RS_SCALE:2 + hip.RS_CARRY]))


# ----------------------------------------------------------------------------- 3. world 1: the consensus kernel IS the loss kernel's rule
@pytest.fixture(scope="module")
def world1(tmp_path_factory):
    return spawn(tmp_path_factory.mktemp("consensus_w1"), 1)[0]


def test_world_one_consensus_equals_the_in_kernel_decision(world1):
    """A section where the gate fires mid-round and the adaptive lr moves, through the loss kernel's decision and with the
    key (collectives forced at world 1): every bit equal."""
    k = int(world1["k"])
    assert k >= 1, "no step exceeds the running maximum: %r" % (scen(world1, "free")["approx_kl"],)
    a, b = scen(world1, "kernel"), scen(world1, "consensus")
    print("k = %d, target_kl = %.6g, lr rows %s" % (k, float(world1["tkl"]), a["row_lr"]))
    assert int(a["stopped_at_step"]) == k and a["applied"].tolist() == [i < k for i in range(8)]       # fires mid-round
    assert len(set(a["row_lr"][:k].tolist())) == k and a["row_lr"][0] == np.float32(drv.LR0 * 1.5)      # lr moves
    assert int(a["consensus_world"]) == 0 and not bool(a["has_global"])
    assert int(b["consensus_world"]) == 1 and bool(b["has_global"])
    for key in ("params", "exp_avg", "exp_avg_sq", "rng"):
        assert str(a[key]) == str(b[key]), key
    for key in ("step_dev", "step", "stop", "lr_bits", "stopped_at_step", "updates_applied"):
        assert int(a[key]) == int(b[key]), key
    assert int(a["stop"]) == 1 and int(a["step_dev"]) == k
    for key in ("applied", "row_lr", "losses", "approx_kl"):
        assert np.array_equal(a[key], b[key]), key
    # world 1: the sum over the ranks is this rank's own KL, bit for bit
    assert np.array_equal(b["global_approx_kl"].astype(np.float32), b["approx_kl"].astype(np.float32))


# ----------------------------------------------------------------------------- 4. - 6. world 2
@pytest.fixture(scope="module")
def world2(tmp_path_factory):
    """The one-rank references (both workers, the loss kernel decides, run here), then the two ranks with the thresholds
    the free reference run places."""
    perms = drv.fixed_perms(PERM_SEED, 2)
    seeds = [STORAGE_SEED, STORAGE_SEED + 1]
    free = drv.run_multi(seeds, perms, dict(adaptive_lr=drv.AD))
    kl = [float(max(r)) for r in free["approx_kl"]]
    k, tkl, gap = drv.first_exceeding(kl)
    assert k is not None, "storage seed %d: no step exceeds the running maximum (%r); choose another seed" % (STORAGE_SEED, kl)
    gated = drv.run_multi(seeds, perms, dict(adaptive_lr=drv.AD, target_kl=tkl))
    out = tmp_path_factory.mktemp("consensus_w2")
    with open(os.path.join(str(out), "config.json"), "w") as f:
        json.dump(dict(perms=perms, target_kl=tkl), f)
    ranks = spawn(out, 2)
    return dict(free=free, gated=gated, k=k, tkl=tkl, gap=gap, kl=kl, ranks=ranks,
                scaling_ref=drv.scaling_run([0, 1], None))


def test_world_two_inputs_are_well_conditioned(world2):
    """The decisions compared below must not hinge on the last bits of a KL: the gate threshold sits midway in a gap of at
    least 100 x KL_TOL, and every step's KL is at least that far from 2 desired, desired / 2 and 0."""
    kl, k = world2["kl"], world2["k"]
    print("reference kl:", kl, "k:", k, "gap:", world2["gap"], "target_kl:", world2["tkl"])
    assert world2["gap"] >= 100 * KL_TOL
    d = drv.AD["desired_kl"]
    for x in kl:
        assert abs(x - 2 * d) >= 100 * KL_TOL and abs(x - d / 2) >= 100 * KL_TOL and x >= 100 * KL_TOL, x
    assert 1 <= k < 8


def test_world_two_ranks_agree(world2):
    for name in ("gate", "never", "plain"):
        a, b = (scen(r, name) for r in world2["ranks"])
        for key in ("params", "exp_avg", "exp_avg_sq"):
            assert str(a[key]) == str(b[key]), (name, key, "ranks diverged")
        for key in ("step_dev", "step", "stop", "lr_bits"):
            assert int(a[key]) == int(b[key]), (name, key)
        assert np.array_equal(a["applied"], b["applied"]) and np.array_equal(a["row_lr"], b["row_lr"]), name
        if name != "plain":
            assert bool(a["has_global"]) and bool(b["has_global"])
            assert np.array_equal(a["global_approx_kl"].view(np.int64), b["global_approx_kl"].view(np.int64)), name
        assert not np.array_equal(a["approx_kl"], b["approx_kl"]), "the ranks hold different workers"


def test_world_two_decisions_match_one_rank_with_both_workers(world2):
    want, k = world2["gated"], world2["k"]
    assert int(want["stopped_at_step"]) == k and int(want["consensus_world"]) == 0
    r0, r1 = (scen(r, "gate") for r in world2["ranks"])
    for got in (r0, r1):
        assert int(got["stopped_at_step"]) == k
        assert got["applied"].tolist() == want["applied"].tolist() == [i < k for i in range(8)]
        assert np.array_equal(got["row_lr"], want["row_lr"]), (got["row_lr"], want["row_lr"])       # the lr sequence, exactly
        assert int(got["lr_bits"]) == int(want["lr_bits"]) and int(got["stop"]) == int(want["stop"]) == 1
        assert int(got["step_dev"]) == int(want["step_dev"]) == k == int(got["step"])
    assert len(set(want["row_lr"][:k].tolist())) == k, "the adaptive lr moved at every applied step"
    # KL of every applied step (and of the step that fired): the sum over the ranks against the one-rank value
    err = np.abs(r0["global_approx_kl"][:k + 1] - want["approx_kl"][:k + 1]).max()
    own = np.abs((r0["approx_kl"] + r1["approx_kl"])[:k + 1] - r0["global_approx_kl"][:k + 1]).max()
    e_p = rel(r0["param_sums"], want["param_sums"])
    e_l = rel(r0["losses"] + r1["losses"], want["losses"])
    print("global kl vs one rank: %.2e (ranks' own kl summed vs reduced: %.2e), parameter sums rel %.2e, losses rel %.2e"
          % (err, own, e_p, e_l))
    assert err <= KL_TOL
    assert own <= np.spacing(np.float32(r0["global_approx_kl"].max()))      # (the float32 sum of the two float32 values the ranks reported)
    assert e_p < PARAM_SUM_TOL and e_l < LOSS_TOL


def test_world_two_gate_that_never_fires_changes_nothing(world2):
    for r in world2["ranks"]:
        a, b = scen(r, "never"), scen(r, "plain")
        for key in ("params", "exp_avg", "exp_avg_sq"):
            assert str(a[key]) == str(b[key]), key
        assert int(a["step_dev"]) == int(b["step_dev"]) == 8 and np.array_equal(a["losses"], b["losses"])
        assert a["applied"].all() and int(a["stopped_at_step"]) == -1 and int(a["stop"]) == 0


def test_world_two_reward_scaling(world2):
    """Three rollouts of T = 16, one environment per rank, against one rank with both environments: the same two scale bits
    on both ranks after every rollout, each the one-rank scale or its float32 neighbour, and returns equal to a numpy scan
    that uses the device's scales, bit for bit."""
    from tests.test_rollout_finish_gpu import np_scan
    f32 = np.float32
    want = world2["scaling_ref"]
    r0, r1 = (scen(r, "scaling") for r in world2["ranks"])
    assert np.array_equal(r0["scales"].view(np.int64), r1["scales"].view(np.int64))
    assert not np.array_equal(r0["stats"], r1["stats"]), "each rank keeps its own statistics"
    for ro in range(drv.SC_ROLLOUTS):
        merged = ref.chan_merge(np.stack([r0["stats"][ro], r1["stats"][ro]]))
        for h in (0, 1):
            g, w = f32(r0["scales"][ro][h]), f32(want["scales"][ro][h])
            assert g == r0["scales"][ro][h] and g != 1.0
            assert g in (w, np.nextafter(w, f32(0)), np.nextafter(w, f32(np.inf))), (ro, h, g, w)
            assert g == ref.scale_of(merged, 1e-8)[h], (ro, h)                 # the mirror on the ranks' own statistics
            assert merged[3 * h] == want["stats"][ro][3 * h] == 2 * drv.SC_T * (ro + 1)
        for e, got in enumerate((r0, r1)):
            for h in (0, 1):
                d = {k: v[:, 0].numpy() for k, v in drv.scaling_data(e, h, ro).items()}
                ret, _adv, _V = np_scan(d["rewards"], d["value_preds"], d["masks"], drv.scaling_next_value(e, h),
                                        scale=f32(got["scales"][ro][h]), clip=drv.SC_CLIP)
                assert np.array_equal(got["returns"][ro][h].view(np.int32), ret.view(np.int32)), (ro, e, h)


def test_world_two_training_loop_reports_the_consensus(world2):
    r0, r1 = (scen(r, "gate") for r in world2["ranks"])
    for got in (r0, r1):
        assert int(got["consensus_world"]) == 2 and bool(got["has_global"])
        assert np.isfinite(got["global_approx_kl"]).all() and got["global_approx_kl"].shape == (8, 2)
    assert int(r0["updates_applied"]) == int(r1["updates_applied"]) == world2["k"]
