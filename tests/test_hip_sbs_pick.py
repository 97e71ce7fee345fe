"""GPU: the stochastic beam search pick (include/set_hip.h set_sbs_pick_f32, csrc/sbs.hip) against the float64 restatement
tests/sbs_oracle.py on chosen logits, three consecutive steps each: shapes on both row-read paths, edge rows, layout
independence, the refusals and the statistics of one launch.  Fixtures, tolerance and gap: tests/sbs_fixtures.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import gumbel_oracle as GO
import sbs_fixtures as F
import sbs_oracle as SO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OK, ARG = 0, 1


def _lib():
    from show_edit_tell_amd import _lib
    return _lib, _lib.load()


def _opts(t):
    from show_edit_tell_amd._lib import SampleOpts
    return None if t == 1.0 else SampleOpts(temperature=t, top_k=0, top_p=1.0)


class Device:
    """the caller's side of the pick for NI images x k slots"""

    def __init__(self, NI, k, V, Lmax, seed, end=F.END, temperature=1.0):
        L, lib = _lib()
        self.NI, self.k, self.V, self.Lmax = NI, k, V, Lmax
        z = lambda *s, dt=torch.int32: torch.zeros(*s, dtype=dt, device=DEV)
        self.phi = z(NI, k, dt=torch.float32)
        self.G = torch.full((NI, k), float("-inf"), device=DEV)
        self.G[:, 0] = 0.0
        self.fin, self.len, self.n_open = z(NI, k), z(NI, k), torch.ones(NI, dtype=torch.int32, device=DEV)
        self.seqs = [z(NI, k, Lmax, dt=torch.long), z(NI, k, Lmax, dt=torch.long)]
        self.words, self.rows = z(NI * k, dt=torch.long), z(NI * k)
        self.ws = torch.zeros(lib.set_sbs_workspace_bytes(NI, k), dtype=torch.uint8, device=DEV)
        self.opts = _opts(temperature)
        self.a = L.SbsArgs(end_idx=end, seed=seed, offset=F.OFFSET, phi=self.phi.data_ptr(), G=self.G.data_ptr(),
                           finished=self.fin.data_ptr(), len=self.len.data_ptr(), words=self.words.data_ptr(),
                           rows=self.rows.data_ptr(), n_open=self.n_open.data_ptr(), ws=self.ws.data_ptr(),
                           ws_bytes=self.ws.numel(), NI=NI, k=k, V=V, Lmax=Lmax)

    def step(self, logits, t):
        """logits: a (NI k, V) view of a device buffer (its row stride is the leading dimension)"""
        L, lib = _lib()
        a = self.a
        a.logits, a.ld, a.t = logits.data_ptr(), logits.stride(0), t
        a.seqs_in, a.seqs_out = self.seqs[0].data_ptr(), self.seqs[1].data_ptr()
        rc = lib.set_sbs_pick_f32(C.byref(a), C.byref(self.opts) if self.opts is not None else None,
                                  L.stream_of(torch.device(DEV)))
        assert rc == OK, rc
        torch.cuda.synchronize()
        self.seqs.reverse()
        return self.snapshot()

    def snapshot(self):
        return {n: getattr(self, n).cpu().numpy().copy() for n in ("phi", "G", "fin", "len", "n_open", "words", "rows")} | {
            "seqs": self.seqs[0].cpu().numpy().copy()}


def _on_device(lg, ld):
    """(rows, V) numpy -> a (rows, V) view with leading dimension ld; ld % 4 != 0 or an odd offset keeps it off the float4 path"""
    rows, V = lg.shape
    buf = torch.full((rows, ld), 123.0, dtype=torch.float32, device=DEV)
    buf[:, :V] = torch.from_numpy(lg).to(DEV)
    return buf[:, :V]


def _compare(snap, states, infos, k, tol, record=None):
    """every discrete output equals the oracle's; phi and G lie within tol.  record: a dict that collects the largest distances"""
    for i, (st, info) in enumerate(zip(states, infos)):
        for s in range(k):
            r = i * k + s
            dead = st.G[s] == -np.inf
            assert (snap["G"][i, s] == -np.inf) == dead, (i, s)
            assert snap["words"][r] == info["next_words"][s], (i, s, snap["words"][r], info)
            assert snap["rows"][r] == i * k + info["rows"][s], (i, s, snap["rows"][r], info)
            if info.get("noop"):
                continue
            assert bool(snap["fin"][i, s]) == bool(st.fin[s]) and snap["len"][i, s] == len(st.toks[s]), (i, s)
            assert snap["seqs"][i, s, :len(st.toks[s])].tolist() == st.toks[s], (i, s)
            if not dead:
                eg, ep = abs(float(snap["G"][i, s]) - st.G[s]), abs(float(snap["phi"][i, s]) - st.phi[s])
                if record is not None:
                    record["G"], record["phi"] = max(record.get("G", 0.0), eg), max(record.get("phi", 0.0), ep)
                assert eg <= tol and ep <= tol, (i, s, eg, ep)
        assert snap["n_open"][i] == st.n_open, i


def _run(L, NI, k, V, ld, seed, T, record=None, end=F.END):
    dev = Device(NI, k, V, len(L) + 1, seed, end, T)
    states = [SO.Image(k) for _ in range(NI)]
    snaps = []
    for t, lg in enumerate(L):
        before = dev.snapshot()
        snap = dev.step(_on_device(lg, ld), t)
        infos = []
        for i in range(NI):
            states[i], info = SO.pick(states[i], lg[i * k:(i + 1) * k], i, t, seed, F.OFFSET, end, F.inv_t(T))
            infos.append(info)
        _compare(snap, states, infos, k, F.TOL, record)
        # a finished slot's phi / G / tokens are carried bit for bit
        for i in range(NI):
            for s in range(k):
                p = infos[i]["parents"][s]
                if not infos[i].get("noop") and snap["G"][i, s] > -np.inf and before["fin"][i, p]:
                    assert snap["G"][i, s].tobytes() == before["G"][i, p].tobytes()
                    assert snap["phi"][i, s].tobytes() == before["phi"][i, p].tobytes()
                    n = before["len"][i, p]
                    assert snap["len"][i, s] == n and np.array_equal(snap["seqs"][i, s, :n], before["seqs"][i, p, :n])
        snaps.append(snap)
    return snaps, states


# ------------------------------------------------------------------------------------------- 1. shapes
@pytest.mark.parametrize("name", sorted(F.DIRECT))
def test_pick_matches_the_oracle(name):
    V, ld, k, NI, T, seed = F.DIRECT[name]
    err = {}
    snaps, states = _run(F.direct_logits(name), NI, k, V, ld, seed, T, record=err)
    if k > 1:
        assert any(st.fin.any() for st in states)
    print(name, "max |dG| %.3g  max |dphi| %.3g" % (err["G"], err["phi"]))
    _, lib = _lib()
    assert lib.set_last_hip_error() == 0


# ------------------------------------------------------------------------------------------- 2. edge rows
def test_minus_inf_words_are_never_picked():
    L = F.edge_minus_inf()
    snaps, states = _run(L, 1, F.EDGE_K, F.EDGE_V, 256, F.EDGE_SEED, 1.0)
    for t, snap in enumerate(snaps):
        for s in range(F.EDGE_K):
            if snap["G"][0, s] > -np.inf:
                w = snap["seqs"][0, s, t]
                assert w % 2 == 1 and w != F.END and np.isfinite(snap["phi"][0, s])


def test_one_possible_word_dead_slots_and_a_closed_image():
    """step 0 leaves one live slot and two dead ones (G = -inf); step 1 two; after step 2 every live slot is finished; the fourth
    step finds n_open == 0 and touches nothing but words / rows (identity) and the token copy"""
    L = F.edge_one_word()
    dev = Device(1, F.EDGE_K, F.EDGE_V, 8, F.EDGE_SEED)
    states = [SO.Image(F.EDGE_K)]
    for t in range(3):
        snap = dev.step(_on_device(L[t], 256), t)
        states[0], info = SO.pick(states[0], L[t], 0, t, F.EDGE_SEED, F.OFFSET, F.END)
        _compare(snap, states, [info], F.EDGE_K, F.TOL)
        live = int((snap["G"][0] > -np.inf).sum())
        assert live == (1, 2, 2)[t] and np.isinf(snap["phi"][0, live:]).all()
        if t == 0:
            assert snap["G"][0, 0] == 0.0 and snap["phi"][0, 0] == 0.0 and snap["seqs"][0, 0, 0] == 7
    assert snap["n_open"][0] == 0 and snap["fin"][0, :2].all()
    closed = dev.step(_on_device(L[3], 256), 3)
    for n in ("phi", "G", "fin", "len", "n_open", "seqs"):
        assert closed[n].tobytes() == snap[n].tobytes(), n
    assert (closed["words"] == 0).all() and closed["rows"].tolist() == [0, 1, 2]


def test_a_closed_image_next_to_an_open_one():
    """NI = 2 in one launch: image 0 closes after step 2 and is a no-op at step 3 (state and tokens byte for byte, words 0,
    identity rows) while image 1 is picked as usual, every step against the oracle"""
    L = F.edge_closed_and_open()
    k = F.EDGE_K
    dev = Device(2, k, F.EDGE_V, 8, F.MIXED_SEED)
    states = [SO.Image(k), SO.Image(k)]
    for t in range(4):
        before = dev.snapshot()
        snap = dev.step(_on_device(L[t], 256), t)
        infos = []
        for i in range(2):
            states[i], info = SO.pick(states[i], L[t][i * k:(i + 1) * k], i, t, F.MIXED_SEED, F.OFFSET, F.END)
            infos.append(info)
        _compare(snap, states, infos, k, F.TOL)
    assert infos[0].get("noop") and not infos[1].get("noop") and before["n_open"].tolist()[0] == 0 and before["n_open"][1] > 0
    for n in ("phi", "G", "fin", "len", "seqs"):
        assert snap[n][0].tobytes() == before[n][0].tobytes(), n
    assert (snap["words"][:k] == 0).all() and snap["rows"][:k].tolist() == list(range(k))
    assert snap["len"][1].max() == 4                     # image 1 went on


# ------------------------------------------------------------------------------------------- 3. layout independence
@pytest.mark.parametrize("name", sorted(F.LAYOUT))
def test_both_row_read_paths_give_the_same_bytes(name):
    V, k, NI, T, seed, ldp = F.LAYOUT[name]
    L = F.layout_logits(name)
    reg, _ = _run(L, NI, k, V, ldp, seed, T)
    sca, _ = _run(L, NI, k, V, V, seed, T)               # V % 4 != 0: the scalar path
    assert ldp % 4 == 0 and V % 4 != 0
    for a, b in zip(reg, sca):
        for n in a:
            assert a[n].tobytes() == b[n].tobytes(), n


# ------------------------------------------------------------------------------------------- 4. refusals
def test_refusals_leave_the_outputs_unwritten():
    L, lib = _lib()
    V, k, NI = 255, 3, 2
    lg = _on_device(F.step_logits("refuse", 0, V, NI * k), 256)
    big = 1 << 26

    def attempt(opts=None, **over):
        dev = Device(NI, k, V, 4, 5)
        for t_ in (dev.phi, dev.G, dev.fin, dev.len, dev.n_open, dev.seqs[0], dev.seqs[1], dev.words, dev.rows):
            t_.fill_(7)
        before = dev.snapshot() | {"other": dev.seqs[1].cpu().numpy().copy()}
        a = dev.a
        a.logits, a.ld, a.t = lg.data_ptr(), lg.stride(0), 0
        a.seqs_in, a.seqs_out = dev.seqs[0].data_ptr(), dev.seqs[1].data_ptr()
        for key, val in over.items():
            setattr(a, key, val)
        rc = lib.set_sbs_pick_f32(C.byref(a) if not over.get("null_args") else None, C.byref(opts) if opts is not None else None,
                                  L.stream_of(torch.device(DEV)))
        torch.cuda.synchronize()
        after = dev.snapshot() | {"other": dev.seqs[1].cpu().numpy().copy()}
        for n in before:
            assert before[n].tobytes() == after[n].tobytes(), (over, n)
        return rc

    from show_edit_tell_amd._lib import SampleOpts
    for field in ("logits", "phi", "G", "finished", "len", "seqs_in", "seqs_out", "words", "rows", "n_open", "ws"):
        assert attempt(**{field: None}) == ARG, field
    assert lib.set_sbs_pick_f32(None, None, None) == ARG
    for over in (dict(k=0), dict(k=9), dict(t=-1), dict(t=255), dict(V=big - 3, ld=big), dict(ld=V - 1), dict(NI=0), dict(Lmax=0),
                 dict(ws_bytes=16), dict(end_idx=-1), dict(end_idx=V), dict(end_idx=1 << 40)):
        assert attempt(**over) == ARG, over
    for o in (SampleOpts(temperature=1.0, top_k=5, top_p=1.0), SampleOpts(temperature=1.0, top_k=0, top_p=0.9),
              SampleOpts(temperature=0.0, top_k=0, top_p=1.0), SampleOpts(temperature=float("nan"), top_k=0, top_p=1.0)):
        assert attempt(o) == ARG
    assert attempt(SampleOpts(temperature=0.5, top_k=0, top_p=1.0), t=255) == ARG     # (a good temperature does not lift the others)
    assert lib.set_sbs_workspace_bytes(0, 3) == 0 and lib.set_sbs_workspace_bytes(2, 9) == 0 and lib.set_sbs_workspace_bytes(2, 0) == 0


# ------------------------------------------------------------------------------------------- 5. one-launch statistics
def test_one_launch_draws_ordered_pairs_without_replacement():
    """NI = 4000 images of the seven-word distribution, k = 2, step 0 in ONE launch: the 42 ordered (first, second) pairs follow
    p_a p_b / (1 - p_a).  The picks are the oracle's, pair for pair, outside near ties."""
    NI = F.STAT_NI
    lg = np.tile(GO.SEVEN_WORDS, (2 * NI, 1))
    dev = Device(NI, 2, 7, 2, F.STAT_SEED, end=6)
    snap = dev.step(_on_device(lg, 8), 0)
    pairs = snap["seqs"][:, :, 0]
    assert (pairs[:, 0] != pairs[:, 1]).all() and (snap["G"][:, 0] == 0.0).all() and (snap["G"][:, 1] < 0.0).all()
    counts, p = F.stat_counts(pairs)
    chi2, bins, pv = GO.chi_square_pvalue(counts, p)
    print("chi2 %.2f over %d bins, p = %.4f" % (chi2, bins, pv))
    assert pv > 1e-3
    either = 0
    for i in range(0, NI, 10):                           # every tenth image against the oracle
        st, info = SO.pick(SO.Image(2), lg[2 * i:2 * i + 2], i, 0, F.STAT_SEED, F.OFFSET, 6)
        if SO.margin(info) < F.GAP:
            either += 1
            continue
        assert pairs[i].tolist() == info["words"], i
        assert abs(float(snap["G"][i, 1]) - st.G[1]) <= F.TOL
    assert either <= F.NEAR_TIE_FRACTION * (NI // 10)


def test_measured_errors_are_what_the_fixtures_record():
    """The largest |device - float64| of G and phi over every step of every direct fixture, measured here: the figures
    tests/sbs_fixtures.py records as G_MEASURED / PHI_MEASURED (3.33e-6 / 2.2e-6 when written).  They must stay within TOL =
    4 x the larger recorded one — the room the recipe leaves for other boxes and compilers — and cannot be vacuous."""
    err = {}
    for name in sorted(F.DIRECT):
        V, ld, k, NI, T, seed = F.DIRECT[name]
        _run(F.direct_logits(name), NI, k, V, ld, seed, T, record=err)
    print("max |dG| = %.3g, max |dphi| = %.3g; recorded %.3g / %.3g, TOL %.3g" % (err["G"], err["phi"], F.G_MEASURED,
                                                                           F.PHI_MEASURED, F.TOL))
    assert 0.0 < err["G"] <= 4.0 * F.G_MEASURED and 0.0 < err["phi"] <= 4.0 * F.PHI_MEASURED
