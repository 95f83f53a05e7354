"""Launch-for-launch record of PPOLearnerHIP's host side: every C-ABI call of an update with its arguments, the hipGraph key
suffix, the workspace tensors a loss launch allocates and the learner's loss attributes, for every loss mode crossed with the update
modes, by-value / device-hyper scalars, categorical / ordinal heads, sorted / unsorted rows and two minibatch sizes — plus the set_loss /
set_hyper bookkeeping and the scoped loss switches.  Nothing runs on a device and the library is not loaded: hip.lib() is a recorder,
pointers are (name, byte offset) pairs.  The file holds every distinct value once, in a pool (class Pool); a case is an index into
it, and what the test reports on a mismatch is the case's name.  The record is compared with `==` against tests/golden/learner_launches.json, which
`python tests/test_learner_launches_cpu.py --write` regenerates byte for byte."""
import collections
import contextlib
import ctypes
import itertools
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "learner_launches.json")

MODES = ("ppo", "bc", "ppo+demo", "aux", "ppo+suggest", "ppo+sil", "ppo+smooth", "ppo+mask")
ATTRS = ("loss_mode", "_bc", "_demo", "_demo_rows", "_sil", "_sil_rows", "_smooth_coeff", "_smooth_rows", "_smooth_tables",
         "_sug_coeff", "_sug_tables", "_aux", "_aux_table")
COEFFS = {"ppo": {}, "bc": dict(label_smoothing=0.1, bc_coeff=0.7), "ppo+mask": {},
          "ppo+demo": dict(label_smoothing=0.05, demo_coeff=0.5, demo_value_coeff=0.25),
          "aux": dict(beta_clone=2.0, aux_value_coeff=0.75), "ppo+suggest": dict(suggest_coeff=0.3),
          "ppo+sil": dict(sil_coeff=0.4, sil_value_coeff=0.2), "ppo+smooth": dict(smooth_coeff=0.6)}
ROWS = {"ppo+demo": "set_demo_rows", "ppo+sil": "set_sil_rows", "ppo+smooth": "set_smooth_rows"}
TAKES_SORTED = ("ppo+demo", "aux", "ppo+sil")          # the launches that take sorted_rows
UPDATE_MODES = {"off": {}, "stats": dict(stats=True, target_kl=0.02), "consensus": dict(stats=True, target_kl=0.02, consensus=True)}
SIZES = ((32, 16), (40, 24))                           # (B, row split); 40 is no multiple of 16: every (B + 15) // 16 scratch size
MIRROR = [3e-4, 0.1, 0.1, 1.0, 0.01, 250.0] + [0.0] * 10   # the block's mirror of a fresh learner (recorded: what differs from it)


Ptr = collections.namedtuple("Ptr", "name offset")      # what the recording's hip.ptr returns


class DevTensor(object):
    """A CPU tensor that answers is_cuda, for the set_*_table(s) checks; everything else is the tensor's."""
    is_cuda = True

    def __init__(self, t):
        self.t = t

    def __getattr__(self, name):
        return getattr(self.t, name)


class Recorder(object):
    """hip.lib(), hip.ptr, hip.stream and hip.gemm of one recording.  `patch(obj, name, value)` is monkeypatch.setattr or the
    script's own."""

    def __init__(self, patch):
        from cadre_amd import hip
        from cadre_amd.arena import PPOArena
        self.calls, self.uploads, self.names, self.lrn, self.pool = [], [], {}, None, Pool()
        patch(hip, "lib", lambda: self)
        patch(hip, "stream", lambda: "stream")
        patch(hip, "ptr", self.ptr)
        patch(hip, "gemm", lambda *a, **k: self.calls.append(("gemm", self.enc(a) + self.enc(sorted(k.items())))))
        patch(torch.cuda, "is_current_stream_capturing", lambda: False)
        self.arena = PPOArena("cpu", 530, {"steer": 33, "throttle": 3}, 4)
        self.ord = torch.zeros(2, 64, dtype=torch.int32)
        self.base, self.wp = {}, None
        self.tables = dict(aux=DevTensor(torch.zeros(2, 50, 64)), prior=DevTensor(torch.zeros(2, 4, 64)),
                           ctrl=DevTensor(torch.zeros(2, 64)))

    def __getattr__(self, name):                       # every entry point: record (name, args), return 0
        def fn(*args):
            self.calls.append((name, self.enc(args)))
            return 0
        return fn

    # -- pointers by name
    def refresh(self):
        self.names = names = {}
        def add(name, v):
            if isinstance(v, tuple) and v:
                v = v[0]
            if hasattr(v, "untyped_storage"):
                names.setdefault(v.untyped_storage().data_ptr(), name)
        for k, v in self.tables.items():
            add(k, v)
        if self.lrn is not None:
            for w in self.lrn._ws.values():
                for k, v in w.items():
                    add("w." + k, v)
            for k, v in vars(self.lrn).items():
                add(k, v)
        for k, v in vars(self.arena).items():
            add("a." + k, v)

    def ptr(self, t):
        if t is None:
            return None
        base = t.untyped_storage().data_ptr()
        if base not in self.names:
            self.refresh()
        return Ptr(self.names[base], t.data_ptr() - base)

    def enc(self, x):
        """JSON form of an argument: a pointer is "name+offset" ("name" at offset 0); a raw address that is a known tensor's (the graph keys hold
        data_ptr() values) is its name."""
        if hasattr(x, "untyped_storage"):
            x = self.ptr(x)
        if isinstance(x, Ptr):
            return "%s+%d" % x if x[1] else x[0]
        if isinstance(x, (tuple, list)):
            return [self.enc(v) for v in x]
        if isinstance(x, ctypes.Array):
            return list(x)
        if isinstance(x, int) and not isinstance(x, bool) and x in self.names:
            return self.names[x]
        return x

    # -- a learner per case, on the shared arena; the mode-independent workspace tensors are shared too
    def learner(self, B, hp=False, ordinal=False, tables=True):
        from cadre_amd.learner import PPOLearnerHIP
        self.arena.ord = self.ord if ordinal else None
        lrn = self.lrn = PPOLearnerHIP(self.arena)
        lrn.use_graphs = False
        if B not in self.base:
            self.base[B] = dict(lrn.workspace(B))
            lrn._alloc_wp()
            self.wp = self.wp if self.wp is not None else lrn._wp
        lrn._ws = {(B, self.arena.Z, lrn.S): dict(self.base[B])}
        lrn._wp = self.wp
        lrn._hp_upload = lambda lo, hi: self.uploads.append([lo, hi])
        if tables:
            lrn.set_aux_table(self.tables["aux"])
            lrn.set_suggest_tables(self.tables["prior"], 3)
            lrn.set_smooth_tables(self.tables["ctrl"], (1.0, 0.5))
        if hp:
            self.block_on(lrn)
        del self.calls[:], self.uploads[:]
        self.refresh()
        self.fresh = {k: self.enc(getattr(lrn, k)) for k in ATTRS}
        return lrn

    def block_on(self, lrn):
        """Device-hyper mode without a device: the block and its mirror by hand, then set_device_hyper fills the mirror."""
        from cadre_amd import hip
        lrn._hp = torch.zeros(hip.HP_FIELDS, dtype=torch.float64)
        lrn._hp_host = np.zeros(hip.HP_FIELDS, dtype=np.float64)
        lrn._hp_host[hip.HP["lr"]], lrn._hp_host[hip.HP["max_grad_norm"]] = 3e-4, 250.0
        lrn.set_device_hyper(True)

    def state(self, lrn):
        """The loss attributes that differ from those learner() left (pooled), the graph key suffix, the _hp_upload spans since the last
        state and, under the block, the mirror's fields that differ from MIRROR."""
        attrs = {k: self.enc(getattr(lrn, k)) for k in ATTRS}
        out = dict(attrs=self.pool.add({k: v for k, v in attrs.items() if v != self.fresh[k]}), key=self.enc(lrn._mode_key()))
        if self.uploads:
            out["uploads"] = [list(u) for u in self.uploads]
        mirror = {str(i): float(v) for i, v in enumerate(lrn._hp_host) if float(v) != MIRROR[i]} if lrn._hp_on else {}
        if mirror:
            out["mirror"] = mirror
        del self.uploads[:]
        return out


class Pool(object):
    """The distinct values of a recording, each written once; a case holds indices.  A call (name, arguments) is written whole, or,
    where fewer than two thirds of its arguments differ from an earlier whole call of that entry point (the nearest one), as
    [name, index of that call, {position: argument}]."""

    def __init__(self):
        self.index, self.out, self.whole = {}, [], {}

    def add(self, v):
        k = json.dumps(v, sort_keys=True)
        if k not in self.index:
            self.index[k] = len(self.out)
            if isinstance(v, tuple) and len(v) == 2:
                args = [json.dumps(a) for a in v[1]]
                near = self.whole.setdefault((v[0], len(args)), [])
                diffs = [(sum(a != b for a, b in zip(args, ref)), base) for base, ref in near]
                if diffs and 3 * min(diffs)[0] < 2 * len(args):
                    base, ref = near[[b for _, b in diffs].index(min(diffs)[1])]
                    v = (v[0], base, {str(i): v[1][i] for i in range(len(args)) if args[i] != ref[i]})
                else:
                    near.append((len(self.out), args))
            self.out.append(v)
        return self.index[k]


def refusal(e):
    return dict(refused=[type(e).__name__, str(e)])


def record_case(rec, mode, um, hp, ordinal, srt, B, split, tables=True, rows=True, run="update"):
    from cadre_amd.hip import CadreHipError
    lrn = rec.learner(B, hp, ordinal, tables)
    base = set(lrn.workspace(B))
    try:
        lrn.set_update_modes(**UPDATE_MODES[um])
        lrn.set_loss(mode, **COEFFS[mode])
        if mode in ROWS and rows is not None:
            getattr(lrn, ROWS[mode])(split if rows is True else rows)
        args = () if run == "aux_record" else ((1.0 if B == 32 else 2.0) / B,)      # (the record pass takes no inv_b)
        getattr(lrn, run)(B, *args, sorted_rows=srt)
    except (ValueError, CadreHipError) as e:
        return rec.pool.add(dict(refusal(e), **rec.state(lrn)))
    w = lrn.workspace(B)
    pool = rec.pool                                    # (the case itself is pooled, and its call sequence like a call)
    return pool.add(dict(calls=pool.add(("calls", [pool.add(c) for c in rec.calls])), **rec.state(lrn),
                         ws=pool.add({k: [list(w[k].shape), str(w[k].dtype)] for k in sorted(set(w) - base)})))


@contextlib.contextmanager
def hand_written_scope(lrn, mode, rows, table, kw):
    """The save / switch / try / finally / restore that every caller of a learner without loss_scope() writes out itself (the golden
    file records its states; loss_scope must reproduce them)."""
    state = {"bc": "_bc", "ppo+demo": "_demo", "aux": "_aux"}.get(mode)
    names = {"bc": ("label_smoothing", "bc_coeff"), "ppo+demo": ("label_smoothing", "demo_coeff", "demo_value_coeff"),
             "aux": ("beta_clone", "aux_value_coeff")}.get(mode, ())
    rattr = None if rows is None else "_" + ROWS[mode][4:]
    prev = (lrn.loss_mode, state and getattr(lrn, state), rattr and getattr(lrn, rattr), lrn._aux_table)
    if mode == "aux":
        lrn.set_aux_table(table)
    if state == "_demo":                               # (label_smoothing: the current one; a None coefficient: set_loss keeps it)
        kw = dict(kw, label_smoothing=prev[1][0] if kw.get("label_smoothing") is None else kw["label_smoothing"])
    elif state:
        kw = {k: cur if kw.get(k) is None else kw[k] for k, cur in zip(names, prev[1])}
    lrn.set_loss(mode, **kw)
    if rows is not None:
        getattr(lrn, ROWS[mode])(rows)
    try:
        yield
    finally:
        lrn.loss_mode = prev[0]
        if rattr:
            setattr(lrn, rattr, prev[2])
        if state and not (mode == "ppo+demo" and lrn.device_hyper):
            setattr(lrn, state, prev[1])
        if mode == "aux":
            lrn._aux_table = prev[3]


def scope(lrn, mode, rows=None, table=None, **kw):
    if hasattr(lrn, "loss_scope"):
        return lrn.loss_scope(mode, rows=rows, **dict(kw, **({} if table is None else dict(table=table))))
    return hand_written_scope(lrn, mode, rows, table, kw)


def record_set_loss(rec):
    """set_loss with each coefficient given, then None, then under the block; set_hyper on every loss coefficient."""
    out = {}
    for mode in MODES:
        lrn = rec.learner(32, tables=False)
        seq = out[mode] = []
        lrn.set_loss(mode, **COEFFS[mode])
        seq.append(rec.state(lrn))
        keep = {k: None for k in COEFFS[mode] if k not in ("label_smoothing", "bc_coeff", "beta_clone", "aux_value_coeff")}
        lrn.set_loss(mode, **keep)
        seq.append(rec.state(lrn))
        rec.block_on(lrn)
        seq.append(rec.state(lrn))
        try:
            lrn.set_loss(mode, **{k: v + 1.0 if k != "label_smoothing" else v for k, v in COEFFS[mode].items()})
            seq.append(rec.state(lrn))
            lrn.set_loss(mode, **keep)
            seq.append(rec.state(lrn))
        except Exception as e:
            seq.append(dict(refusal(e), **rec.state(lrn)))
        lrn.set_hyper(demo_coeff=3.0, smooth_coeff=4.0)
        seq.append(rec.state(lrn))
        lrn.set_device_hyper(False)
        seq.append(rec.state(lrn))
    lrn, seq = rec.learner(32, hp=True, tables=False), []            # every loss coefficient through set_hyper, one by one
    for k in ("demo_coeff", "demo_value_coeff", "suggest_coeff", "sil_coeff", "sil_value_coeff", "smooth_coeff", "clip", "lr"):
        lrn.set_hyper(**{k: 0.125})
        seq.append(dict(rec.state(lrn), hyper=lrn.hyper(k)))
    return dict(out, set_hyper=seq)


def record_scopes(rec):
    """Each scoped switch, entered from "ppo+sil", by value and under the block: the state before / inside / after."""
    sites = (("ppo+mask", {}), ("ppo+smooth", dict(rows=24)), ("ppo+sil", dict(rows=24)), ("ppo+suggest", {}),
             ("ppo+demo", dict(rows=24, label_smoothing=None, demo_coeff=None, demo_value_coeff=None)),
             ("ppo+demo", dict(rows=24, label_smoothing=0.2, demo_coeff=0.9, demo_value_coeff=0.8)),
             ("bc", dict(label_smoothing=None, bc_coeff=None)), ("bc", dict(label_smoothing=0.3, bc_coeff=0.6)),
             ("aux", dict(table=rec.tables["aux"], beta_clone=None, aux_value_coeff=None)),
             ("aux", dict(table=rec.tables["aux"], beta_clone=3.0, aux_value_coeff=0.5)))
    out = []
    for (mode, kw), start, hp in itertools.product(sites, ("ppo+sil",), (False, True)):
        lrn = rec.learner(32, tables=False)
        lrn.set_loss("ppo+demo", **COEFFS["ppo+demo"])
        lrn.set_demo_rows(7)
        lrn.set_loss(start, **COEFFS[start])
        if hp:
            rec.block_on(lrn)
        row = dict(mode=mode, kw=[[k, rec.enc(v)] for k, v in sorted(kw.items())], start=start, hp=hp, before=rec.state(lrn))
        try:
            with scope(lrn, mode, **kw):
                row["inside"] = rec.state(lrn)
                if hp:                                 # a coefficient written to the block during the scope stays
                    lrn.set_hyper(demo_coeff=5.0, sil_coeff=6.0)
        except Exception as e:
            row.update(refusal(e))
        row["after"] = rec.state(lrn)
        out.append(row)
    return out


def record(patch):
    rec, cases = Recorder(patch), {}
    for mode, um, hp, ordinal, (B, split) in itertools.product(MODES, UPDATE_MODES, (False, True), (False, True), SIZES):
        for srt in ((False, True) if mode in TAKES_SORTED else (False,)):
            name = "%s|%s|%s|%s|%s|B%d" % (mode, um, "hp" if hp else "value", "ord" if ordinal else "cat", "sorted" if srt else "unsorted", B)
            cases[name] = record_case(rec, mode, um, hp, ordinal, srt, B, split)
    # what a launch refuses: the row split missing or out of bounds, the table missing
    for mode, kw in (("ppo+demo", dict(rows=None)), ("ppo+demo", dict(rows=41)), ("ppo+demo", dict(rows=40)), ("ppo+demo", dict(rows=0)),
                     ("ppo+sil", dict(rows=None)), ("ppo+sil", dict(rows=41)), ("ppo+sil", dict(rows=40)), ("ppo+sil", dict(rows=0)),
                     ("ppo+smooth", dict(rows=None)), ("ppo+smooth", dict(rows=40)), ("ppo+smooth", dict(rows=0)),
                     ("ppo+smooth", dict(tables=False)), ("aux", dict(tables=False)), ("ppo+suggest", dict(tables=False))):
        name = "%s|%s" % (mode, json.dumps(kw, sort_keys=True))
        cases[name] = record_case(rec, mode, "off", False, False, False, 40, 24, **kw)
    # the two forward-only passes that share a loss mode's arguments: the evaluation form of "bc", the record pass of "aux"
    for (mode, run), ordinal, srt in itertools.product((("bc", "bc_evaluate"), ("aux", "aux_record")), (False, True), (False, True)):
        name = "%s|%s|%s|%s" % (mode, run, "ord" if ordinal else "cat", "sorted" if srt else "unsorted")
        cases[name] = record_case(rec, mode, "off", False, ordinal, srt, 40, 24, run=run)
    set_loss, scopes = record_set_loss(rec), record_scopes(rec)
    return dict(pool=rec.pool.out, cases=cases, set_loss=set_loss, scopes=scopes)


def dumps(result):
    """Compact JSON, the entries of each part packed into lines of about 200 characters."""
    one = lambda v: json.dumps(v, sort_keys=True, separators=(",", ":"))

    def pack(items):
        lines = [""]
        for item in items:
            if lines[-1] and len(lines[-1]) + len(item) > 200:
                lines.append("")
            lines[-1] += ("," if lines[-1] else "") + item
        return ",\n".join(lines)
    pairs = lambda d: pack("%s:%s" % (json.dumps(k), one(v)) for k, v in d.items())
    return ('{"pool":[\n%s\n],\n"cases":{\n%s\n},\n"set_loss":{\n%s\n},\n"scopes":[\n%s\n]}\n'
            % (pack(map(one, result["pool"])), pairs(result["cases"]), pairs(result["set_loss"]), pack(map(one, result["scopes"]))))


def test_learner_launches_match_the_record(monkeypatch):
    got = json.loads(dumps(record(monkeypatch.setattr)))
    with open(GOLDEN) as f:
        want = json.load(f)
    assert sorted(got) == sorted(want) and list(got["cases"]) == list(want["cases"])

    def written_out(g, v):
        """A pooled value with its indices replaced by what they stand for (a partial call by the whole one)."""
        if isinstance(v, dict):
            return {k: written_out(g, g["pool"][x]) if k in ("attrs", "calls", "ws") else x for k, x in v.items()}
        if isinstance(v, list) and len(v) == 3 and isinstance(v[2], dict):
            args = list(g["pool"][v[1]][1])
            for i, a in v[2].items():
                args[int(i)] = a
            v = [v[0], args]
        return [written_out(g, g["pool"][i]) for i in v[1]] if isinstance(v, list) and v[0] == "calls" else v
    for name in want["cases"]:                          # (first by case and written out, so that a failure names what differs)
        assert written_out(got, got["pool"][got["cases"][name]]) == written_out(want, want["pool"][want["cases"][name]]), name
    for part in ("set_loss", "scopes"):
        assert got[part] == want[part], part
    assert got == want
    # the launch count of a step is the same for every mode that runs, whatever else varies within a (rows, sorted) family
    whole = lambda e: e[1] if isinstance(e[1], list) else got["pool"][e[1]][1]     # (a partial entry has its whole one's length)
    n = {name: len(whole(got["pool"][got["pool"][c]["calls"]])) for name, c in got["cases"].items() if "calls" in got["pool"][c]}
    n = {name: v for name, v in n.items() if name.split("|")[1] not in ("bc_evaluate", "aux_record")}
    assert n and all(v == n["ppo|off|value|cat|unsorted|B32"] + (name.split("|")[0] in ("ppo+demo", "ppo+sil")) for name, v in n.items())


if __name__ == "__main__":
    saved = []

    def patch(obj, name, value):
        saved.append((obj, name, getattr(obj, name)))
        setattr(obj, name, value)
    try:
        text = dumps(record(patch))
    finally:
        for obj, name, value in reversed(saved):
            setattr(obj, name, value)
    if "--write" in sys.argv:
        with open(GOLDEN, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)
