"""GPU: the truncated stochastic beam search picks (include/set_hip.h set_sbs_pick_opts_f32 / set_sbs_pick_ensemble_opts_f32,
csrc/sbs.hip sbs_rows_k<.., .., true>) against the float64 restatement tests/sbs_trunc_oracle.py, three chained steps each: shapes
on both row-read paths, top-k / top-p / both, dead slots under top_k = 2, hand-built rows, layout independence, neutral options
against the untruncated entries, the ensemble.  Fixtures, tolerance and gap: tests/sbs_trunc_fixtures.py; that no decision here
rests on a near tie or a boundary is asserted on the oracle alone by tests/test_sbs_trunc_cpu.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import sbs_fixtures as F
import sbs_oracle as SO
import sbs_trunc_fixtures as T
import sbs_trunc_oracle as TS
from test_hip_sbs_pick import DEV, OK, Device, _compare, _lib, _on_device

pytestmark = pytest.mark.gpu


class TruncDevice(Device):
    """the caller's side of the pick through the *_opts entries (old=True: the untruncated entries, for the neutral comparison)"""

    def __init__(self, NI, k, V, Lmax, seed, temperature=1.0, top_k=0, top_p=1.0, end=F.END, neutral_as_null=True, old=False):
        super().__init__(NI, k, V, Lmax, seed, end, temperature)
        from show_edit_tell_amd._lib import SampleOpts
        self.old = old
        if (top_k, top_p) != (0, 1.0) or not neutral_as_null:
            self.opts = SampleOpts(temperature=temperature, top_k=top_k, top_p=top_p)

    def step(self, logits, t, logits2=None):
        L, lib = _lib()
        a = self.a
        a.logits, a.ld, a.t = logits.data_ptr(), logits.stride(0), t
        a.seqs_in, a.seqs_out = self.seqs[0].data_ptr(), self.seqs[1].data_ptr()
        o, st = (C.byref(self.opts) if self.opts is not None else None), L.stream_of(torch.device(DEV))
        if logits2 is None:
            rc = (lib.set_sbs_pick_f32 if self.old else lib.set_sbs_pick_opts_f32)(C.byref(a), o, st)
        else:
            assert logits2.stride(0) == logits.stride(0)
            rc = (lib.set_sbs_pick_ensemble_f32 if self.old else lib.set_sbs_pick_ensemble_opts_f32)(C.byref(a), logits2.data_ptr(), o, st)
        assert rc == OK, rc
        torch.cuda.synchronize()
        self.seqs.reverse()
        return self.snapshot()


def _run(Ls, NI, k, V, ld, seed, temp, top_k, top_p, record=None, tol=None, end=F.END):
    """three chained steps on the device and on the oracle, every step compared; Ls: arrays (one model) or pairs (the ensemble)"""
    dev = TruncDevice(NI, k, V, len(Ls) + 1, seed, temp, top_k, top_p, end)
    states = [SO.Image(k) for _ in range(NI)]
    snaps = []
    for t, lg in enumerate(Ls):
        ens = isinstance(lg, tuple)
        snap = dev.step(_on_device(lg[0], ld), t, _on_device(lg[1], ld)) if ens else dev.step(_on_device(lg, ld), t)
        infos = []
        for i in range(NI):
            rows = slice(i * k, (i + 1) * k)
            if ens:
                states[i], info = TS.pick_ensemble(states[i], lg[0][rows], lg[1][rows], i, t, seed, T.OFFSET, end, temp, top_k, top_p)
            else:
                states[i], info = TS.pick(states[i], lg[rows], i, t, seed, T.OFFSET, end, F.inv_t(temp), top_k, top_p)
            infos.append(info)
        _compare(snap, states, infos, k, T.TOL if tol is None else tol, record)
        snaps.append(snap)
    return snaps, states


def _same_bytes(a, b):
    for x, y in zip(a, b):
        for n in x:
            assert x[n].tobytes() == y[n].tobytes(), n


# ------------------------------------------------------------------------------------------- 1. shapes and options
@pytest.mark.parametrize("name", sorted(T.DIRECT))
def test_pick_matches_the_oracle(name):
    V, ld, k, NI, temp, seed, top_k, top_p = T.DIRECT[name]
    err = {}
    snaps, states = _run(T.direct_logits(name), NI, k, V, ld, seed, temp, top_k, top_p, record=err)
    print(name, "max |dG| %.3g  max |dphi| %.3g" % (err["G"], err["phi"]))
    if name == "v255_k8_ni1_k2":                         # top_k = 2 under 8 slots: dead slots with G = phi = -inf, len 0
        s0 = snaps[0]
        assert (s0["G"][0, :2] > -np.inf).all() and (s0["G"][0, 2:] == -np.inf).all() and (s0["phi"][0, 2:] == -np.inf).all()
        assert (s0["len"][0, 2:] == 0).all() and (snaps[1]["G"][0, 4:] == -np.inf).all()
    _, lib = _lib()
    assert lib.set_last_hip_error() == 0


# ------------------------------------------------------------------------------------------- 2. hand-built rows
@pytest.mark.parametrize("path", ["reg", "generic"])
@pytest.mark.parametrize("name", sorted(T.SPECIAL))
def test_hand_built_rows(path, name):
    lg, V, ld, want = T.special_logits(path, name)
    _, top_k, top_p, _ = T.SPECIAL[name]
    assert T.is_reg(V, ld) == (path == "reg")
    snaps, _ = _run([lg], 1, T.SPECIAL_K, V, ld, T.SPECIAL_SEED[(path, name)], 1.0, top_k, top_p)
    s = snaps[0]
    live = s["G"][0] > -np.inf
    if want is not None:
        assert sorted(s["seqs"][0, live, 0].tolist()) == want          # the kept set, whole: every tie, both zeros, one word
    if name == "one_word_over_top_p":
        assert live.tolist() == [True] + [False] * 7
        assert s["phi"][0, 0].tobytes() == np.float32(0.0).tobytes() and s["G"][0, 0] == 0.0      # phi' = phi_j exactly


def test_rows_with_minus_inf_words():
    top_k, top_p = T.EDGE_OPTS
    for ld in (256, 255):
        snaps, _ = _run(F.edge_minus_inf(), 1, F.EDGE_K, F.EDGE_V, ld, T.EDGE_SEED, 1.0, top_k, top_p)
        for t, snap in enumerate(snaps):
            for s in range(F.EDGE_K):
                if snap["G"][0, s] > -np.inf:
                    w = snap["seqs"][0, s, t]
                    assert w % 2 == 1 and w != F.END and np.isfinite(snap["phi"][0, s])


# ------------------------------------------------------------------------------------------- 3. layout independence
@pytest.mark.parametrize("name", sorted(T.LAYOUT))
def test_both_row_read_paths_give_the_same_bytes(name):
    V, k, NI, temp, seed, ldp, top_k, top_p = T.LAYOUT[name]
    L = T.layout_logits(name)
    reg, _ = _run(L, NI, k, V, ldp, seed, temp, top_k, top_p)
    sca, _ = _run(L, NI, k, V, V, seed, temp, top_k, top_p)
    _same_bytes(reg, sca)


# ------------------------------------------------------------------------------------------- 4. neutral options
@pytest.mark.parametrize("ens", [False, True])
@pytest.mark.parametrize("ld", [1028, 1027])
def test_neutral_options_are_the_untruncated_entry_byte_for_byte(ens, ld):
    """NULL opts, {T, 0, 1} and top_k >= V through the new entry against the old entry on sbs_fixtures' logits"""
    V, k, NI, temp, seed = 1027, 3, 3, 0.5, 1
    L = [F.step_logits("neutral", t, V, NI * k, temp) for t in range(T.STEPS)]
    L2 = [F.step_logits("neutral2", t, V, NI * k, temp) for t in range(T.STEPS)]

    def run(**kw):
        dev = TruncDevice(NI, k, V, T.STEPS + 1, seed, temp, **kw)
        return [dev.step(_on_device(L[t], ld), t, _on_device(L2[t], ld) if ens else None) for t in range(T.STEPS)]

    old = run(old=True)
    for kw in (dict(), dict(neutral_as_null=False), dict(top_k=V), dict(top_k=V + 7)):
        _same_bytes(old, run(**kw))


# ------------------------------------------------------------------------------------------- 5. the ensemble
@pytest.mark.parametrize("name", sorted(T.ENS_DIRECT))
def test_ensemble_pick_matches_the_oracle_on_L(name):
    V, ld, k, NI, temp, seed, top_k, top_p = T.ENS_DIRECT[name]
    err = {}
    _run(T.ens_logits(name), NI, k, V, ld, seed, temp, top_k, top_p, record=err)
    print("ensemble", name, "max |dG| %.3g  max |dphi| %.3g" % (err["G"], err["phi"]))


def test_ensemble_paths_give_the_same_bytes():
    name, ld_a, ld_b = T.ENS_LAYOUT
    V, _, k, NI, temp, seed, top_k, top_p = T.ENS_DIRECT[name]
    L = T.ens_logits(name)
    a, _ = _run(L, NI, k, V, ld_a, seed, temp, top_k, top_p)
    b, _ = _run(L, NI, k, V, ld_b, seed, temp, top_k, top_p)
    _same_bytes(a, b)


# ------------------------------------------------------------------------------------------- 6. the recorded errors
def test_measured_errors_are_what_the_fixtures_record():
    """The largest |device - float64| of G and phi over every step of every direct fixture, one model and ensemble, measured
    here: the figures tests/sbs_trunc_fixtures.py records as G_MEASURED / PHI_MEASURED.  They must stay within TOL = 4 x the
    larger recorded one and cannot be vacuous."""
    err = {}
    for name in sorted(T.DIRECT):
        V, ld, k, NI, temp, seed, top_k, top_p = T.DIRECT[name]
        _run(T.direct_logits(name), NI, k, V, ld, seed, temp, top_k, top_p, record=err, tol=1e-4)
    for name in sorted(T.ENS_DIRECT):
        V, ld, k, NI, temp, seed, top_k, top_p = T.ENS_DIRECT[name]
        _run(T.ens_logits(name), NI, k, V, ld, seed, temp, top_k, top_p, record=err, tol=1e-4)
    print("MEASURED max |dG| = %.3g, max |dphi| = %.3g; recorded %.3g / %.3g, TOL %.3g" % (err["G"], err["phi"], T.G_MEASURED,
                                                                                    T.PHI_MEASURED, T.TOL))
    assert 0.0 < err["G"] <= T.TOL and 0.0 < err["phi"] <= T.TOL
