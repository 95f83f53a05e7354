"""GPU: the PPG auxiliary phase — cadre_aux_loss and cadre_aux_record against float64 (tests/phasic_ref.py), the
equal-statements property (a row recorded from the logits it is trained on has KL and logit gradient exactly zero), one
auxiliary step per parameter through the agent, aux_phase on a synthetic buffer and train_cfg["aux_phase"] in train_vec."""
import functools
import os

import numpy as np
import pytest
import torch

from cadre_amd import synth
from tests import phasic_ref
from tests.test_imitation_gpu import CASES, make_agent, ord_table, rel, steer_rank

pytestmark = pytest.mark.gpu
F = phasic_ref.AUX_STATS_FIELDS
BETA, AVC = 0.8, 0.6
SENTINEL = 7.25                                    # rows of a table no launch addressed keep this bit pattern


# ----------------------------------------------------------------------------- inputs and references, once per case
@functools.lru_cache(maxsize=None)
def aux_case(B, C, nS, nT, scale, special=None):
    """Inputs (ldl = 64) shared by every variant of a case: logits and table rows drawn independently at `scale`, a table
    of R = 3 B rows, distinct random row ids per head, a random permutation `pos` per head.  special: "idle" — the last
    command owns no row; "out" — two commands and two row ids out of range."""
    g = torch.Generator().manual_seed(2000 * B + nS + int(scale))
    R = 3 * B
    logits = torch.zeros(2 * C, B, 64)
    logits[:C, :, :nS] = torch.randn(C, B, nS, generator=g) * scale
    logits[C:, :, :nT] = torch.randn(C, B, nT, generator=g) * scale
    values = torch.randn(2 * C, B, generator=g)
    cmds = torch.randint(0, C - 1 if special == "idle" else C, (2, B), generator=g, dtype=torch.int32)
    rets = torch.randn(2, B, generator=g)
    row_id = torch.stack([torch.randperm(R, generator=g)[:B] for _ in range(2)]).contiguous()
    table = torch.full((2, R, 64), float("-inf"))
    table[0, :, :nS] = torch.log_softmax(torch.randn(R, nS, generator=g) * scale, -1)
    table[1, :, :nT] = torch.log_softmax(torch.randn(R, nT, generator=g) * scale, -1)
    pos = torch.stack([torch.randperm(B, generator=g) for _ in range(2)]).to(torch.int32).contiguous()
    if special == "out":
        cmds[0, 1], cmds[1, 3] = C, -1
        row_id[0, 2], row_id[1, 0] = R, -1
    ranks = (steer_rank(nS, g), torch.randperm(nT, generator=g).tolist())
    return dict(logits=logits, values=values, cmds=cmds, rets=rets, row_id=row_id, table=table, pos=pos), ranks


def mode_ranks(ranks, ordmode):
    return {"cat": (None, None), "both": ranks, "steer": (ranks[0], None)}[ordmode]


@functools.lru_cache(maxsize=None)
def aux_ref(B, C, nS, nT, scale, ordmode, with_pos, special=None):
    """(losses[3], d total / d raw, d total / d value, stats [2][6]) in float64, once per variant."""
    inp, ranks = aux_case(B, C, nS, nT, scale, special)
    lg = inp["logits"].double().requires_grad_(True)
    vv = inp["values"].double().requires_grad_(True)
    tv, tk, total, stats = phasic_ref.aux_loss(lg, vv, inp["cmds"], inp["rets"], inp["table"].double(), inp["row_id"],
                                               inp["pos"] if with_pos else None, (nS, nT), mode_ranks(ranks, ordmode), C,
                                               BETA, AVC, 1.0 / B)
    total.backward()
    return torch.tensor([float(tv.detach()), float(tk.detach()), 0.0]), lg.grad, vv.grad, stats


def new_outputs(B, C):
    nblk = (B + 15) // 16
    out = dict(losses=torch.full((3,), 4.0, device="cuda"), dl=torch.full((2 * C, B, 64), 9.0, device="cuda"),
               dv=torch.full((2 * C, B), 9.0, device="cuda"), scratch=torch.full((4 + 6 * nblk,), 3.0, device="cuda"),
               stats=torch.full((2, F), 5.0, device="cuda"), sscr=torch.full((2 * F * nblk,), 3.0, device="cuda"))
    out["scratch"][0] = 0.0                                # the arrival counter: zero on first use, reset by every launch
    return out


def dev_inputs(inp):
    return {k: v.cuda() for k, v in inp.items()}


def run_loss(d, o, B, C, nS, nT, ord_t=None, with_pos=False, table=None, stats=True, poison=None, coeffs=(BETA, AVC)):
    from cadre_amd import hip
    table = d["table"] if table is None else table
    hip.check(hip.lib().cadre_aux_loss(
        d["logits"].data_ptr(), 64, B * 64, d["values"].data_ptr(), 1, B, d["cmds"].data_ptr(), d["rets"].data_ptr(),
        d["pos"].data_ptr() if with_pos else None, d["row_id"].data_ptr(), table.data_ptr(), table.shape[1], B, C, nS, nT,
        coeffs[0], coeffs[1], 1.0 / B, o["losses"].data_ptr(), o["dl"].data_ptr(), o["dv"].data_ptr(), o["scratch"].data_ptr(),
        None if poison is None else poison.data_ptr(), o["stats"].data_ptr() if stats else None, F,
        o["sscr"].data_ptr() if stats else None, None if ord_t is None else ord_t.data_ptr(), hip.stream()), "cadre_aux_loss")
    assert float(o["scratch"][0]) == 0.0                   # the counter is left zero


def run_record(d, table, B, C, nS, nT, ord_t=None, with_pos=False):
    from cadre_amd import hip
    hip.check(hip.lib().cadre_aux_record(
        d["logits"].data_ptr(), 64, B * 64, d["cmds"].data_ptr(), d["pos"].data_ptr() if with_pos else None,
        d["row_id"].data_ptr(), B, C, nS, nT, None if ord_t is None else ord_t.data_ptr(), table.data_ptr(), table.shape[1],
        hip.stream()), "cadre_aux_record")


def ord_for(ranks, ordmode):
    if ordmode == "cat":
        return None
    return ord_table(ranks if ordmode == "both" else (ranks[0], None))


def counted_rows(inp, hd, C, with_pos):
    """(workspace positions b, commands c, table rows r) of the rows that count for head hd."""
    B, R = inp["cmds"].shape[1], inp["table"].shape[1]
    _u, b, c, r = phasic_ref._rows(inp["cmds"], inp["row_id"], inp["pos"] if with_pos else None, hd, C, R)
    return b, c, r


def check_against_ref(case, scale, ordmode, with_pos, special=None):
    B, C, nS, nT = case
    inp, ranks = aux_case(B, C, nS, nT, scale, special)
    want_l, want_dl, want_dv, want_st = aux_ref(B, C, nS, nT, scale, ordmode, with_pos, special)
    ord_t = ord_for(ranks, ordmode)
    d, o = dev_inputs(inp), new_outputs(B, C)
    run_loss(d, o, B, C, nS, nT, ord_t, with_pos)
    e_l, e_dv, e_dl = rel(o["losses"], want_l), rel(o["dv"], want_dv), rel(o["dl"], want_dl)
    e_st = float((o["stats"].double().cpu() - want_st).abs().max())
    print("case %s scale %g %s pos %s %s: losses %.2e dvalues %.2e dlogits %.2e stats %.2e (mean kl %.3f/%.3f, max kl %.3f/%.3f)"
          % (case, scale, ordmode, with_pos, special, e_l, e_dv, e_dl, e_st, want_st[0, 0], want_st[1, 0], want_st[0, 1],
             want_st[1, 1]))
    # the bars cadre_bc_loss is held to (tests/test_imitation_gpu.check_against_ref): the kernels share every statement up to lg
    assert e_l < 1e-5 and e_dv < 1e-5 and e_dl < 2e-5, (e_l, e_dv, e_dl)
    assert e_st < 1e-5, e_st
    assert float(o["losses"][2]) == 0.0
    # exact zeros everywhere but a counted row's own net: lanes >= K, the other nets of a head, counted-out rows, an idle command
    zero_l, zero_v = torch.ones(2 * C, B, 64, dtype=torch.bool), torch.ones(2 * C, B, dtype=torch.bool)
    for hd, K in enumerate((nS, nT)):
        b, c, _r = counted_rows(inp, hd, C, with_pos)
        zero_l[hd * C + c, b, :K] = False
        zero_v[hd * C + c, b] = False
    assert float(o["dl"].cpu()[zero_l].abs().max()) == 0.0 and float(want_dl[zero_l].abs().max()) == 0.0
    assert float(o["dv"].cpu()[zero_v].abs().max() if zero_v.any() else 0.0) == 0.0
    return inp, d, o, ord_t


# ----------------------------------------------------------------------------- 1. cadre_aux_loss
@pytest.mark.parametrize("with_pos", [False, True])
@pytest.mark.parametrize("scale", [1.0, 4.0])
@pytest.mark.parametrize("case", CASES)
def test_aux_loss_fwd_bwd(case, scale, with_pos):
    """Losses 1e-5, dvalues 1e-5, dlogits 2e-5 (relative to the largest reference magnitude) and the statistics 1e-5 absolute
    against float64 autograd; exact zeros outside the counted rows' own nets; repeated launches bit-identical; no stats row:
    the same bits; poison gives NaN losses."""
    B, C, nS, nT = case
    inp, d, o, ord_t = check_against_ref(case, scale, "cat", with_pos)
    first = {k: o[k].clone() for k in ("losses", "dl", "dv", "stats")}
    for _ in range(3):                                     # partials combined in workgroup order
        run_loss(d, o, B, C, nS, nT, ord_t, with_pos)
        assert all(torch.equal(o[k], first[k]) for k in first)
    o2 = new_outputs(B, C)                                 # the -1 marker and no stats row: the same bits
    run_loss(d, o2, B, C, nS, nT, ord_table((None, None)), with_pos, stats=False)
    assert all(torch.equal(o2[k], first[k]) for k in ("losses", "dl", "dv")) and float((o2["stats"] - 5.0).abs().max()) == 0.0
    poison = torch.ones(1, dtype=torch.int32, device="cuda")   # a reported forward-pass timeout: NaN losses
    run_loss(d, o, B, C, nS, nT, ord_t, with_pos, poison=poison)
    assert bool(torch.isnan(o["losses"]).all()) and torch.equal(o["dl"], first["dl"]) and torch.equal(o["dv"], first["dv"])


@pytest.mark.parametrize("with_pos", [False, True])
@pytest.mark.parametrize("ordmode", ["both", "steer"])
@pytest.mark.parametrize("case", CASES)
def test_aux_loss_ordinal_heads(case, ordmode, with_pos):
    """Both heads ordinal (the non-monotone shipped steer table at 33 bins) and steer-only ordinal at scale 4 (saturating
    threshold units); the categorical throttle head of the mix is the categorical launch's, bit for bit."""
    B, C, nS, nT = case
    inp, d, o, ord_t = check_against_ref(case, 4.0, ordmode, with_pos)
    check_against_ref(case, 1.0, ordmode, with_pos)
    if ordmode == "steer":
        cat = new_outputs(B, C)
        run_loss(d, cat, B, C, nS, nT, None, with_pos)
        assert torch.equal(cat["dl"][C:], o["dl"][C:]) and torch.equal(cat["dv"], o["dv"])
        assert torch.equal(cat["stats"][1], o["stats"][1])


@pytest.mark.parametrize("with_pos", [False, True])
def test_aux_loss_idle_command_gets_exact_zeros(with_pos):
    case = (7, 3, 33, 3)
    B, C, nS, nT = case
    inp, d, o, _t = check_against_ref(case, 1.0, "cat", with_pos, special="idle")
    assert int(inp["cmds"].max()) == C - 2
    for hd in range(2):
        assert float(o["dl"][hd * C + C - 1].abs().max()) == 0.0 and float(o["dv"][hd * C + C - 1].abs().max()) == 0.0


@pytest.mark.parametrize("with_pos", [False, True])
@pytest.mark.parametrize("ordmode", ["cat", "both"])
def test_aux_loss_bad_commands_and_row_ids_count_out(ordmode, with_pos):
    case = (17, 4, 33, 3)
    B, C, nS, nT = case
    inp, d, o, _t = check_against_ref(case, 1.0, ordmode, with_pos, special="out")
    for hd in range(2):
        b, _c, _r = counted_rows(inp, hd, C, with_pos)
        # a bad command marks a workspace row, a bad row id an unsorted row: through `pos` the two may be one row
        assert (B - 2 <= b.numel() <= B - 1) if with_pos else b.numel() == B - 2
        assert abs(float(o["stats"][hd, 5]) - b.numel() / B) < 1e-6
        out = torch.ones(B, dtype=torch.bool)
        out[b] = False
        rows = torch.nonzero(out).view(-1).cuda()
        assert float(o["dl"][hd * C:(hd + 1) * C][:, rows].abs().max()) == 0.0
        assert float(o["dv"][hd * C:(hd + 1) * C][:, rows].abs().max()) == 0.0


# ----------------------------------------------------------------------------- 2. cadre_aux_record
def permuted(d, B, C):
    """The inputs of a case laid out in UNSORTED order: row u of head hd is workspace row pos[hd][u] of the original."""
    lg, cm = d["logits"].clone(), d["cmds"].clone()
    for hd in range(2):
        p = d["pos"][hd].long()
        lg[hd * C:(hd + 1) * C] = d["logits"][hd * C:(hd + 1) * C][:, p]
        cm[hd] = d["cmds"][hd][p]
    return dict(d, logits=lg.contiguous(), cmds=cm.contiguous())


@pytest.mark.parametrize("ordmode", ["cat", "both", "steer"])
@pytest.mark.parametrize("case", CASES)
def test_aux_record(case, ordmode):
    """Finite entries within 1e-5 absolute of the float64 log-softmax (the bar of the lg it shares), -inf in lanes >= K, rows
    not addressed keep their sentinel bits; a record through `pos` equals the record with NULL `pos` on the correspondingly
    permuted inputs bit for bit.
    The absolute bar holds wherever fp32 can express it: every categorical case at both scales and the ordinal heads at
    scale 1.  An ordinal head at scale 4 sums up to 64 log-sigmoids of magnitude up to 18 into bin logits z of magnitude
    above 64 (float64 reference: 78 to 174 here), where the spacing of fp32 is 7.6e-6 to 1.5e-5 — one unit in the last place
    of the intermediate z is the bar itself, and the statements are those of the loss kernels by design.  Those cases
    (chosen on the REFERENCE's max |z| >= 64, not on the result) are held to the bar test_ordinal_gpu.py holds the same
    quantity to, 1e-5 * max |lg|; measured on an MI355X: 6.1e-6 to 2.4e-5 absolute, the largest at max |z| = 174, where it is
    1.6 units in the last place of z.  The largest error under the absolute bar is 8.4e-6 (K = 64 ordinal,
    scale 1, max |z| = 63.8)."""
    from tests import ordinal_ref
    B, C, nS, nT = case
    for scale, special in ((1.0, None), (4.0, "out" if B >= 4 else None)):
        inp, ranks = aux_case(B, C, nS, nT, scale, special)
        rk, ord_t = mode_ranks(ranks, ordmode), ord_for(ranks, ordmode)
        d = dev_inputs(inp)
        R = 3 * B
        # the largest unnormalised bin logit of the float64 reference: the magnitude the kernel's intermediate sums reach
        zmax = max(float(ordinal_ref.ordinal_logits(inp["logits"][hd * C:(hd + 1) * C, :, :K].double(), rk[hd]).abs().max())
                   if rk[hd] is not None else float(inp["logits"][hd * C:(hd + 1) * C].abs().max())
                   for hd, K in enumerate((nS, nT)))
        for with_pos in (False, True):
            want = phasic_ref.record(inp["logits"].double(), inp["cmds"], inp["row_id"], inp["pos"] if with_pos else None,
                                     (nS, nT), rk, C, torch.full((2, R, 64), SENTINEL, dtype=torch.float64))
            got = torch.full((2, R, 64), SENTINEL, device="cuda")
            run_record(d, got, B, C, nS, nT, ord_t, with_pos)
            got = got.cpu()
            finite = torch.isfinite(want)
            err = float((got.double()[finite] - want[finite]).abs().max())
            written = finite & (want != SENTINEL)
            lgmax = float(want[written].abs().max())
            print("case %s scale %g %s pos %s: record %.2e (reference max |z| %.1f, max |lg| %.1f)"
                  % (case, scale, ordmode, with_pos, err, zmax, lgmax))
            assert zmax < 64 or (ordmode != "cat" and scale == 4.0)           # (only the saturating ordinal heads get there)
            assert err < (1e-5 if zmax < 64 else 1e-5 * lgmax)
            assert torch.equal(got[~finite], want[~finite].float())           # -inf exactly where the reference has it
            for hd, K in enumerate((nS, nT)):
                _b, _c, r = counted_rows(inp, hd, C, with_pos)
                assert bool(torch.isinf(got[hd, r, K:]).all()) if K < 64 else True
                keep = torch.ones(R, dtype=torch.bool)
                keep[r] = False
                assert torch.equal(got[hd, keep], torch.full((int(keep.sum()), 64), SENTINEL))
        through_pos = torch.full((2, R, 64), SENTINEL, device="cuda")
        run_record(d, through_pos, B, C, nS, nT, ord_t, True)
        direct = torch.full((2, R, 64), SENTINEL, device="cuda")
        run_record(permuted(d, B, C), direct, B, C, nS, nT, ord_t, False)
        assert torch.equal(through_pos.view(torch.int32), direct.view(torch.int32))


# ----------------------------------------------------------------------------- 3. the equal-statements property
@pytest.mark.parametrize("with_pos", [False, True])
@pytest.mark.parametrize("ordmode", ["cat", "both", "steer"])
@pytest.mark.parametrize("case", CASES)
def test_recorded_rows_have_exactly_zero_kl_and_gradient(case, ordmode, with_pos):
    """Record from logits X, then the loss on the same X and rows: p_old is formed from the stored lg by the statements that
    form p from lg, so losses[1], every dlogits element and kl_max are exactly 0.0 — not rounding noise."""
    B, C, nS, nT = case
    for scale in (1.0, 4.0):
        inp, ranks = aux_case(B, C, nS, nT, scale)
        ord_t = ord_for(ranks, ordmode)
        d = dev_inputs(inp)
        own = torch.full((2, 3 * B, 64), SENTINEL, device="cuda")
        run_record(d, own, B, C, nS, nT, ord_t, with_pos)
        o = new_outputs(B, C)
        run_loss(d, o, B, C, nS, nT, ord_t, with_pos, table=own)
        assert float(o["losses"][1]) == 0.0
        assert float(o["dl"].abs().max()) == 0.0
        assert float(o["stats"][:, 1].abs().max()) == 0.0 and float(o["stats"][:, 0].abs().max()) == 0.0
        assert float(o["losses"][0]) > 0.0 and float(o["dv"].abs().max()) > 0.0 and float(o["stats"][:, 3].min()) > 0.0


# ----------------------------------------------------------------------------- 4. one aux step through the agent
def random_buffer(agent, T, seed):
    """An AuxBuffer of one slot of T random feature rows (no encoder: what the float64 reference can be fed on the CPU),
    non-zero LSTM states, and a table of T independent random distributions."""
    from cadre_amd.phasic import AuxBuffer
    r = np.random.RandomState(seed)
    host = dict(obs=(r.standard_normal((T, 8, 530)) * 0.5).astype(np.float32), cmd=r.randint(0, 4, T).astype(np.int32),
                ret=r.standard_normal((T, 2)).astype(np.float32), hn=(r.standard_normal((T, 530)) * 0.1).astype(np.float32),
                cn=(r.standard_normal((T, 530)) * 0.1).astype(np.float32))
    buf = AuxBuffer(agent, 1, T)
    buf.steer.obs[:T].copy_(torch.from_numpy(host["obs"]))
    for hd, st in enumerate((buf.steer, buf.throttle)):
        st.command[:T, 0].copy_(torch.from_numpy(host["cmd"]))
        st.returns[:T, 0].copy_(torch.from_numpy(host["ret"][:, hd].copy()))
        st.hn[:T].copy_(torch.from_numpy(host["hn"]))
        st.cn[:T].copy_(torch.from_numpy(host["cn"]))
    buf.filled = 1
    table = torch.full((2, T, 64), float("-inf"))
    table[0, :, :33] = torch.log_softmax(torch.from_numpy(r.standard_normal((T, 33))).float(), -1)
    table[1, :, :3] = torch.log_softmax(torch.from_numpy(r.standard_normal((T, 3))).float(), -1)
    buf.table.copy_(table)
    host["table"] = table
    return buf, host


def reference_step(host, idx, beta, vc, C=4):
    """float64 autograd through the oracle's nets (oracle/ppo_ref.py) with the reference loss on rows idx (in unsorted
    order: the loss does not depend on the layout).  Returns (params, losses[2], stats)."""
    from oracle import ppo_ref
    params = {m: {k: p.double().requires_grad_(True) for k, p in d.items()}
              for m, d in ppo_ref.to_torch_params(synth.ppo_state(11)).items()}
    B = len(idx)
    x = torch.from_numpy(host["obs"][idx]).double().permute(1, 0, 2).reshape(-1, 530)          # time-major [S * B, 530]
    state = (torch.from_numpy(host["hn"][idx]).double(), torch.from_numpy(host["cn"][idx]).double())
    lg_rows, v_rows = [], []
    for hd, (head, K) in enumerate((("steer", 33), ("throttle", 3))):
        for c in range(C):
            h, _ = ppo_ref.lstm_forward(x, state, params["%s_lstm_%d" % (head, c)])
            raw = ppo_ref.mlp3(h, params["%s_ppo_%d" % (head, c)], "control.linear")
            lg_rows.append(torch.nn.functional.pad(raw, (0, 64 - K)))
            v_rows.append(ppo_ref.mlp3(h, params["%s_ppo_%d" % (head, c)], "critic").view(-1))
    logits, values = torch.stack(lg_rows), torch.stack(v_rows)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    rows = t(idx).view(1, -1).repeat(2, 1)
    tv, tk, total, stats = phasic_ref.aux_loss(logits, values, t(host["cmd"][idx]).view(1, -1).repeat(2, 1), t(host["ret"][idx].T),
                                               host["table"].double(), rows, None, (33, 3), (None, None), C, beta, vc, 1.0 / B)
    total.backward()
    for d in params.values():
        for p in d.values():
            if p.grad is None:
                p.grad = torch.zeros_like(p)
    return params, [float(tv.detach()), float(tk.detach()), 0.0], stats


@pytest.mark.parametrize("B,sort", [(24, False), (64, True), (64, False)])
def test_one_aux_step_matches_float64_autograd_per_param(tmp_path, B, sort):
    """Gradients of one auxiliary step within 2e-4 of each model's max |g| (the project's gradient bar, the method of
    test_one_imitation_step_matches_float64_autograd_per_param) of float64 autograd through the oracle's nets with the
    reference loss: eager (call 1), warm-up (call 2) and through the captured graph (call 3), bit-identical to each other.
    Then record and step on the same entry in the same order at value_coeff = 0: the whole gradient comes through the KL
    term, and it is exactly zero in every parameter."""
    agent = make_agent(tmp_path)
    agent.learner.use_sorted = sort
    assert agent.learner.sorted_rows(B) == sort
    buf, host = random_buffer(agent, B + 8, seed=B)
    idx = torch.from_numpy(np.random.RandomState(1).permutation(B + 8)[:B].astype(np.int64))
    params, want_l, want_st = reference_step(host, idx.numpy(), BETA, AVC)
    row = torch.zeros(2, F, device="cuda")
    calls = []
    for _ in range(3):
        got = agent.aux_from_storages(buf.entry(idx), buf.table, stats_row=row, beta_clone=BETA, value_coeff=AVC)
        calls.append((got, agent.arena.grads.clone(), row.clone()))
    lrn = agent.learner
    assert lrn.loss_mode == "ppo" and lrn._aux_table is None                  # the mode is restored on exit
    assert any(k[0] == "all" and ("aux", BETA, AVC, buf.table.data_ptr(), B + 8) in k for k in lrn._graphs if k[0] != "warm")
    for got, grads, st in calls[1:]:
        assert got == calls[0][0] and torch.equal(grads, calls[0][1]) and torch.equal(st, calls[0][2])
    assert torch.equal(lrn.workspace(B)["aux_rows"].cpu(), idx.view(1, -1).repeat(2, 1))
    print("B %d sorted %s: losses %s (float64 %s), mean kl %s" % (B, sort, calls[0][0], want_l, want_st[:, 0].tolist()))
    assert rel(calls[0][0], want_l) < 1e-4 and calls[0][0][2] == 0.0
    assert float((calls[0][2].double().cpu() - want_st).abs().max()) < 1e-4
    worst = 0.0
    for mn, d in params.items():
        gv = agent.arena.views(calls[2][1], mn)
        scale = max(float(p.grad.abs().max()) for p in d.values())
        assert scale > 0
        for k, p in d.items():
            err = float((gv[k].cpu().double() - p.grad).abs().max()) / scale
            worst = max(worst, err)
            assert err < 2e-4, (mn, k, err)
    print("B %d sorted %s: worst per-parameter gradient error (rel. to model max |g|): %.2e" % (B, sort, worst))
    # record, then step on the same entry in the same order: p_old == p bit for bit in every row
    before = buf.table.clone()
    assert agent.aux_record_from_storages(buf.entry(idx), buf.table) is None
    assert lrn.loss_mode == "ppo"
    changed = (buf.table != before).any(-1)
    mask = torch.zeros(B + 8, dtype=torch.bool)
    mask[idx] = True
    assert torch.equal(changed.cpu(), mask.view(1, -1).repeat(2, 1))          # exactly the entry's rows were rewritten
    for _ in range(3):                                                        # eager, warm-up and the captured graph
        v, k, z = agent.aux_from_storages(buf.entry(idx), buf.table, stats_row=row, beta_clone=1.0, value_coeff=0.0)
        assert v == 0.0 and k == 0.0 and z == 0.0
        assert float(agent.arena.grads.abs().max()) == 0.0
        assert float(row[:, 1].abs().max()) == 0.0 and float(row[:, 2].min()) > 0.0
    with pytest.raises(ValueError, match="exactly one"):
        agent.aux_from_storages(buf.entry(idx) * 2, buf.table)


def test_aux_mode_with_the_device_hyper_block_and_its_refusals(tmp_path):
    """Unlike "bc", "aux" runs in device-hyper mode: the step and the optimiser step after it leave the block as it was."""
    from cadre_amd import hip
    agent = make_agent(tmp_path)
    lrn = agent.learner
    buf, _host = random_buffer(agent, 32, seed=5)
    idx = torch.arange(24)
    plain = agent.aux_from_storages(buf.entry(idx), buf.table)
    g_plain = agent.arena.grads.clone()
    lrn.set_device_hyper(True)
    lrn.set_hyper(lr=2e-4, max_grad_norm=250.0)
    block = lrn._hp.clone()
    for _ in range(3):
        assert agent.aux_from_storages(buf.entry(idx), buf.table) == plain and torch.equal(agent.arena.grads, g_plain)
    lrn.clip_adam(lr=2e-4, max_grad_norm=250.0)
    torch.cuda.synchronize()
    assert torch.equal(lrn._hp.view(torch.int64), block.view(torch.int64)) and lrn.hyper("lr") == 2e-4
    assert ("hp",) in [k for k in lrn._graphs if k[0] == "all"][-1]
    lrn.set_device_hyper(False)
    lrn.set_update_modes(stats=True)
    with pytest.raises(hip.CadreHipError, match="auxiliary loss"):
        agent.aux_from_storages(buf.entry(idx), buf.table)
    assert lrn.loss_mode == "ppo"
    lrn.set_update_modes(target_kl=0.01)
    with pytest.raises(hip.CadreHipError, match="auxiliary loss"):
        lrn.set_loss("aux")
    lrn.set_update_modes()
    for bad in (dict(beta_clone=float("nan")), dict(aux_value_coeff=float("inf")), dict(beta_clone="x"), dict(beta_clone=True)):
        with pytest.raises(ValueError):
            lrn.set_loss("aux", **bad)
    lrn.set_loss("aux", beta_clone=0.5, aux_value_coeff=2.0)
    with pytest.raises(hip.CadreHipError, match="set_aux_table"):
        lrn.update(24, 1.0 / 24)
    lrn.set_aux_table(buf.table)
    assert ("aux", 0.5, 2.0, buf.table.data_ptr(), 32) in lrn._mode_key()
    lrn.set_aux_table(None)
    lrn.set_loss("ppo")
    assert lrn._mode_key() == ()
    with pytest.raises(ValueError):
        lrn.set_aux_table(torch.zeros(2, 8, 32, device="cuda"))


# ----------------------------------------------------------------------------- 5. aux_phase on a small synthetic buffer
EPOCHS = 10


def run_phase(tmp, beta, log=None):
    from cadre_amd.phasic import aux_phase
    from ppo_agent.models import Shared_grad_buffers
    agent = make_agent(tmp)
    buf, _host = random_buffer(agent, 128, seed=77)
    sgb = Shared_grad_buffers(agent.model_dict, agent.device)
    torch.manual_seed(4321)                                # (building an agent draws; the phase itself must not)
    state = torch.get_rng_state().clone()
    rec = aux_phase(agent, buf, epochs=EPOCHS, minibatch=32, shared_grad_buffers=sgb, optimizer=None, max_grad_norm=250.0, lr=1e-3,
                    beta_clone=beta, value_coeff=1.0, seed=5, rank=0, episode=3, log=log)
    assert torch.equal(torch.get_rng_state(), state)       # the global CPU generator is where it was
    return agent, buf, rec


def test_aux_phase_on_a_synthetic_buffer(tmp_path):
    """R = 128, B = 32, 10 epochs of 4 steps: the critic's error falls from the first epoch to the last, the KL clone holds the
    policy closer than no clone does (the same rows, the same seed), the global CPU generator is not touched.
    Why 10 epochs: the optimiser here starts from zero moments, and while they are young an Adam step moves every parameter
    that has a gradient by about lr, whatever the gradient's size.  The clone's corrections to the actor towers therefore put
    a floor of order lr^2 under the KL that does not grow with the number of steps n, while without the clone the actor
    towers never move and the trunk's drift grows the KL with n^2.  At 3 epochs (n = 12, measured on an MI355X) the two were
    still level: steer 4.9e-4 with the clone against 9.5e-4 without, throttle 1.5e-3 against 6.7e-4.  At n = 40 the drift is
    an order of magnitude past the floor: measured 9.9e-5 / 2.7e-4 with the clone against 1.6e-3 / 1.4e-3 without.  (In a
    training run the moments continue from the PPO steps and are not young.)
    The KL of the first training step comes from a record pass and a step that batch the rows differently (rows in order
    against a permutation): it is printed and only held to be finite.  Measured: exactly 0 in both heads, mean and maximum
    (B = 32 runs the unsorted form, whose forward gives a row the same bits wherever it stands in the batch)."""
    lines = []
    agent, buf, rec = run_phase(tmp_path / "a", 1.0, log=lines.append)
    assert len(rec) == EPOCHS and len(lines) == EPOCHS and all(r["steps"] == 4 for r in rec) and "aux epoch: 9" in lines[9]
    assert agent.arena.step == 4 * EPOCHS and agent.learner.loss_mode == "ppo" and buf.full
    for r in rec:
        print("beta 1 epoch %d: kl %s max %s value error %s value loss %s entropy %s"
              % (r["epoch"], r["kl"], r["kl_max"], r["value_error"], r["value_loss"], r["entropy"]))
    for hd in range(2):
        assert rec[-1]["value_error"][hd] < rec[0]["value_error"][hd]
        assert all(np.isfinite(r[k][hd]) for r in rec for k in ("kl", "kl_max", "value_error", "value_loss", "entropy"))
    _agent0, _buf0, rec0 = run_phase(tmp_path / "b", 0.0)
    for r in rec0:
        print("beta 0 epoch %d: kl %s value error %s" % (r["epoch"], r["kl"], r["value_error"]))
    print("final mean kl: beta 1 %s, beta 0 %s" % (rec[-1]["kl"], rec0[-1]["kl"]))
    for hd in range(2):
        assert rec[-1]["kl"][hd] < rec0[-1]["kl"][hd]
    # the first training step alone, on a fresh agent: record pass, then step 0 of epoch 0
    from cadre_amd.phasic import epoch_permutation, record_starts
    fresh = make_agent(tmp_path / "c")
    fbuf, _h = random_buffer(fresh, 128, seed=77)
    order = torch.arange(128)
    for lo in record_starts(128, 32):
        fresh.aux_record_from_storages(fbuf.entry(order[lo:lo + 32]), fbuf.table)
    row = torch.zeros(2, F, device="cuda")
    fresh.aux_from_storages(fbuf.entry(epoch_permutation(5, 0, 3, 0, 32, 128)[:32]), fbuf.table, stats_row=row)
    first = row[:, 0].tolist() + row[:, 1].tolist()
    print("first-step kl (mean steer, throttle, max steer, throttle): %s" % (first,))
    assert all(np.isfinite(v) for v in first)
    with pytest.raises(ValueError, match="minibatch"):
        from cadre_amd.phasic import aux_phase
        aux_phase(fresh, fbuf, 1, 129, None, None, 250.0, 1e-3)


# ----------------------------------------------------------------------------- 6. train_vec
class Lines(object):
    def __init__(self):
        self.lines = []

    def log(self, s):
        self.lines.append(s)


def run_train_vec(tmp, episodes=2, logger=None, env=None, callback=None, **extra):
    from ppo_agent.train import train_vec
    from tests.helpers import SyntheticEnv, topology_cfgs
    train_cfg, agent_cfg, env_cfg, rollout_cfg = topology_cfgs(str(tmp), T=8, episodes=episodes)
    env_cfg.update({k: extra.pop(k) for k in ("start_step", "seed_base") if k in extra})
    train_cfg.update(save_interval=10 ** 6, **extra)
    os.makedirs(str(tmp), exist_ok=True)
    agent = train_vec(0, train_cfg, agent_cfg, env_cfg, rollout_cfg, 1, env_cls=env or SyntheticEnv, logger=logger,
                      callback=callback)
    torch.cuda.synchronize()
    return agent


def test_train_vec_with_and_without_an_aux_phase_key(tmp_path):
    absent = run_train_vec(tmp_path / "a")
    none = run_train_vec(tmp_path / "b", aux_phase=None)
    assert torch.equal(absent.arena.params, none.arena.params) and absent.arena.step == none.arena.step == 4
    log = Lines()
    with_aux = run_train_vec(tmp_path / "c", logger=log, log_stats=True, aux_phase={"interval": 2, "minibatch": 8})
    # R = 2 rollouts x 8 rows, B = 8: 2 epochs x 2 steps behind the 4 PPO steps, after episode 1
    assert with_aux.arena.step == 8 and with_aux.learner.loss_mode == "ppo"
    assert not torch.equal(with_aux.arena.params, absent.arena.params) and bool(torch.isfinite(with_aux.arena.params).all())
    epochs = [s for s in log.lines if "aux epoch" in s]
    assert len(epochs) == 2 and all(s.startswith("Episode: 1, aux epoch") for s in epochs)
    assert sum("aux phase: 2 epochs x 2 steps" in s for s in log.lines) == 1
    at = [i for i, s in enumerate(log.lines) if "aux epoch" in s or s.startswith("Episode: 1, value loss")]
    assert log.lines[at[-1]].startswith("Episode: 1, value loss")             # the phase runs before the episode's log line


def test_train_vec_refuses_a_checkpoint_interval_off_the_aux_interval(tmp_path):
    with pytest.raises(ValueError, match="checkpoint_interval 3 is not a multiple of interval 2"):
        run_train_vec(tmp_path / "a", episodes=4, checkpoint_interval=3, aux_phase={"interval": 2})


def test_train_vec_aux_phase_resume_is_bit_exact(tmp_path):
    """4 episodes, phase and checkpoint every 2: the buffer is empty at the capture, so a fresh call from another seed
    resumed from the episode-1 checkpoint ends with the parameters and Adam moments of the uninterrupted run, bit for bit."""
    from tests.test_checkpoint_gpu import _resume_env, same
    Env = _resume_env()
    kw = dict(episodes=4, env=Env, checkpoint_interval=2, aux_phase={"interval": 2, "minibatch": 8, "epochs": 1})
    files = {}

    def cb(event, **st):
        if event == "checkpoint":
            files[st["episode"]] = st["path"]
    full = run_train_vec(tmp_path / "full", callback=cb, **kw)
    assert sorted(files) == [1, 3] and full.arena.step == 4 * 2 + 2 * 2
    res = run_train_vec(tmp_path / "res", resume_from=files[1], start_step=2 * 8, seed_base=31337, **kw)
    a, b = full.arena, res.arena
    assert same(a.params, b.params) and same(a.exp_avg, b.exp_avg) and same(a.exp_avg_sq, b.exp_avg_sq)
    assert same(a.step_dev, b.step_dev) and a.step == b.step
    with pytest.raises(ValueError, match="resumes at episode"):               # an interval the checkpoint's episode is off
        run_train_vec(tmp_path / "off", resume_from=files[1], start_step=2 * 8, episodes=4, env=Env,
                      aux_phase={"interval": 4})


def test_train_vec_aux_phase_in_device_hyper_mode(tmp_path):
    """A schedule puts the learner in device-hyper mode; the phase runs there and leaves the block's lr where the section set it."""
    from cadre_amd import hip
    agent = run_train_vec(tmp_path / "a", episodes=2, schedules={"clip": ("linear", 0.1, 0.05)},
                          aux_phase={"interval": 1, "minibatch": 8, "epochs": 1})
    lrn = agent.learner
    assert lrn.device_hyper and agent.arena.step == 2 * 2 + 2 * 1
    assert lrn.hyper("lr") == 3e-4 and float(lrn._hp[hip.HP["lr"]].item()) == 3e-4
    assert any(("hp",) in k and any(isinstance(e, tuple) and e and e[0] == "aux" for e in k) for k in lrn._graphs)
