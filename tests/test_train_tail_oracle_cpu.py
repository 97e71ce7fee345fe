"""CPU: the float64 oracle of the training tail (tests/train_tail_oracle.py) against torch in float64, and the properties
of the input families and case lists that tests/test_hip_train_tail.py relies on."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch.nn.utils.rnn import pack_padded_sequence

import train_tail_oracle as O

RTOL = 1e-12


def _close(got, ref, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, what
    if got.size:
        assert np.abs(got - ref).max() <= RTOL * max(1.0, np.abs(ref).max()), (what, np.abs(got - ref).max())


@pytest.mark.parametrize("name,B,T,V,lens", [("randn3", 4, 5, 37, [5, 4, 4, 1]), ("peak_off", 3, 2, 257, [2, 2, 1]),
                                             ("offset_p1000", 2, 3, 5, [3, 2]), ("ascending", 3, 2, 1003, [2, 1, 1]),
                                             ("underflow", 5, 64, 63, O.xe_lengths("ragged", 5, 64))])
def test_xe_rows_is_cross_entropy_over_the_packed_rows(name, B, T, V, lens):
    x, caps = O.xe_family(name, B, T, V)
    live = O.live_of(lens, T)
    loss, lse, grad = O.xe_rows(x, caps[:, 1:], live)
    xt = torch.from_numpy(x).double().requires_grad_(True)
    sc = pack_padded_sequence(xt, lens, batch_first=True).data
    tg = pack_padded_sequence(torch.from_numpy(caps[:, 1:]), lens, batch_first=True).data
    rows = F.cross_entropy(sc, tg, reduction="none")
    rows.sum().backward()
    packed = [(t, b) for t in range(T) for b in range(live[t])]              # the order pack_padded_sequence emits
    assert len(packed) == rows.shape[0] == sum(lens)
    _close([loss[t, b] for t, b in packed], rows.detach().numpy(), "loss")
    _close([lse[t, b] for t, b in packed], torch.logsumexp(sc, 1).detach().numpy(), "lse")
    _close(grad, xt.grad.numpy().transpose(1, 0, 2), "grad")                 # zero rows where torch packed nothing
    dead = np.arange(B)[None, :] >= np.array(live)[:, None]
    assert dead.any() and not loss[dead].any() and not lse[dead].any() and not grad[dead].any()


def test_xe_rows_marks_an_out_of_range_target():
    x, caps = O.xe_family("randn3", 3, 2, 5)
    caps[1, 1], caps[2, 2] = 5, -1
    loss, lse, grad = O.xe_rows(x, caps[:, 1:], [3, 3])
    bad = np.zeros((2, 3), bool)
    bad[0, 1] = bad[1, 2] = True
    assert np.array_equal(np.isnan(loss), bad) and np.isfinite(lse).all()
    assert np.array_equal(np.isnan(grad), np.broadcast_to(bad[:, :, None], grad.shape))


def test_mse_is_torch_in_double():
    a, b = O.mse_inputs(4099)
    ta, tb = (torch.from_numpy(v).double().requires_grad_(True) for v in (a, b))
    s = ((ta - tb) ** 2).sum()
    s.backward()
    got = O.mse(a, b)
    _close(got[0], float(s), "sum")
    _close(got[1], ta.grad.numpy(), "da")
    _close(got[2], tb.grad.numpy(), "db")


@pytest.mark.parametrize("max_norm", O.ADAM_MAX_NORMS)
@pytest.mark.parametrize("case", ["edges", "late"])
def test_clip_adam_is_clip_grad_norm_and_torch_adam_in_double(case, max_norm):
    groups = O.adam_groups(case)
    p, st = O.adam_params(case), O.adam_state(case)
    tp = [torch.nn.Parameter(torch.from_numpy(v).double()) for v in p]
    opt = torch.optim.Adam([dict({k: v for k, v in g.items() if k != "params"}, params=[tp[i] for i in g["params"]]) for g in groups])
    if case == "late":
        for q, s in zip(tp, st):
            opt.state[q] = dict(step=torch.tensor(float(s["step"])), exp_avg=torch.from_numpy(s["m"]).double(),
                                exp_avg_sq=torch.from_numpy(s["v"]).double())
    for it in range(O.ADAM_STEPS):
        g = O.adam_grads(case, it)
        for q, gi in zip(tp, g):
            q.grad = torch.from_numpy(gi).double()
        norm = torch.nn.utils.clip_grad_norm_(tp, max_norm)
        opt.step()
        p, st, total, clipped = O.clip_adam(p, g, st, groups, max_norm)
        _close(total, float(norm), "norm")
        for i, q in enumerate(tp):
            _close(p[i], q.detach().numpy(), ("p", it, i))
            _close(clipped[i], q.grad.numpy(), ("grad", it, i))
            if q.numel():
                _close(st[i]["m"], opt.state[q]["exp_avg"].numpy(), ("m", it, i))
                _close(st[i]["v"], opt.state[q]["exp_avg_sq"].numpy(), ("v", it, i))
                assert st[i]["step"] == int(opt.state[q]["step"])
    assert (max_norm < 1) == (total > max_norm)                              # 0.25 clips, 1e9 does not


def test_clip_adam_lets_a_nan_norm_through():
    groups, p, st = O.adam_groups("nan"), O.adam_params("nan"), O.adam_state("nan")
    g = O.adam_grads("nan", 0)
    g[1][7] = np.nan
    p, st, total, clipped = O.clip_adam(p, g, st, groups, 0.25)
    assert np.isnan(total) and all(np.isnan(q).all() for q in p)


# ------------------------------------------------------------------------------------------------
# what the families and case lists claim
# ------------------------------------------------------------------------------------------------
def test_xe_shape_list_covers_what_it_claims():
    assert tuple(s[2] for s in O.XE_SHAPES) == O.XE_VS and {v % 4 for v in O.XE_VS} == {0, 1, 2, 3}
    # waves 1 to 3 of the 256-thread workgroup: empty (V <= 64), partly filled, full (V >= 256)
    assert any(v <= 64 for v in O.XE_VS) and any(64 < v < 256 and v % 64 for v in O.XE_VS) and any(v >= 256 for v in O.XE_VS)
    assert {s[1] for s in O.XE_SHAPES} == set(O.XE_TS) and max(O.XE_TS) == O.XE_MAX_T
    assert {s[3] for s in O.XE_SHAPES} == set(O.XE_LAYOUTS) and {s[4] for s in O.XE_SHAPES} == set(O.XE_LENS)
    assert any(s[0] == 1 for s in O.XE_SHAPES) and all(s[0] <= 5 for s in O.XE_SHAPES)
    assert any(s[0] * s[1] > 256 for s in O.XE_SHAPES)                       # sum_rows_k takes its loop
    for B, T, V, layout, kind in O.XE_SHAPES:
        lens = O.xe_lengths(kind, B, T)
        live = O.live_of(lens, T)
        assert len(lens) == B and max(lens) >= 1 and all(lens[i] >= lens[i + 1] for i in range(B - 1))
        assert all(0 <= n <= B for n in live) and all(live[t] >= live[t + 1] for t in range(T - 1))
        if kind == "full":
            assert live == [B] * T
        if kind == "ragged":
            assert min(lens) < max(lens) or B == 1
        if kind == "dead":
            assert live[T - 1] == 0
        if layout == "slice":
            assert O.slice_width(V) > V and O.slice_width(V) % 4


@pytest.mark.parametrize("V", O.XE_FAMILY_VS)
def test_xe_families_are_what_their_names_say(V):
    B, T = O.XE_FAMILY_B, O.XE_FAMILY_T
    fam = {n: O.xe_family(n, B, T, V) for n in O.XE_FAMILIES}
    for n, (x, caps) in fam.items():
        assert x.dtype == np.float32 and x.shape == (B, T, V) and caps.shape == (B, T + 1)
        assert caps.min() >= 0 and caps.max() < V and not np.isnan(x).any()
    tg = {n: fam[n][1][:, 1:] for n in fam}
    assert (np.diff(fam["ascending"][0], axis=2) > 0).all() and (np.diff(fam["descending"][0], axis=2) < 0).all()
    assert fam["ascending"][0].min() == -100 and fam["ascending"][0].max() == 0
    assert len(np.unique(fam["equal"][0])) == 1
    x = fam["underflow"][0]
    e = np.exp(x - x.max(axis=2, keepdims=True), dtype=np.float32)
    assert e.dtype == np.float32 and ((e == 0).any(axis=2) & ((e > 0).sum(axis=2) >= 2)).all()
    for n in ("peak_on", "peak_off"):
        x = fam[n][0]
        top = np.sort(x, axis=2)
        assert (top[:, :, -1] - top[:, :, -2] > 50).all()
        on = np.take_along_axis(x, tg[n][:, :, None], 2)[:, :, 0] == top[:, :, -1]
        assert on.all() if n == "peak_on" else not on.any()
    assert fam["offset_p1000"][0].min() > 950 and fam["offset_m1000"][0].max() < -950
    for n, pos in (("max_at_0", 0), ("max_at_last", V - 1), ("max_at_255", min(255, V - 1)), ("max_at_256", min(256, V - 1))):
        x = fam[n][0]
        assert (x.argmax(axis=2) == pos).all() and ((x == x.max(axis=2, keepdims=True)).sum(axis=2) == 1).all()
    x = fam["neg_inf"][0]
    assert np.isneginf(x).any(axis=2).all() and np.isfinite(np.take_along_axis(x, tg["neg_inf"][:, :, None], 2)).all()
    loss, lse, grad = O.xe_rows(x, tg["neg_inf"], [B] * T)
    assert np.isfinite(loss).all() and not np.isnan(grad).any() and (grad.transpose(1, 0, 2)[np.isneginf(x)] == 0).all()
    assert np.abs(O.xe_rows(fam["equal"][0], tg["equal"], [B] * T)[0] - np.log(V)).max() < 1e-12


def test_mse_sizes_cover_what_they_claim():
    s = O.MSE_SIZES
    assert s[0] == 1 and {63, 64, 65, 1023, 1024, 1025, 4099} <= set(s)      # wave and workgroup (1024 threads) edges
    assert max(s) == 2048 * 256 + 5 and sum(1 for n in s if n > O.MSE_GRID_LIMIT) == 1


def test_adam_gradients_stay_inside_the_comparable_range():
    for case, c in O.ADAM_CASES.items():
        for it in range(O.ADAM_STEPS):
            for i, g in enumerate(O.adam_grads(case, it)):
                assert g.dtype == np.float32 and g.shape == (c["sizes"][i],)
                if i == c["zero_grad"]:
                    assert not g.any()
                elif g.size:
                    a = np.abs(g.astype(np.float64))
                    assert O.GRAD_MIN * (1 - 1e-6) <= a.min() and a.max() <= O.GRAD_MAX
                    assert (g * g > np.finfo(np.float32).tiny).all()         # g*g is a normal float32


def test_adam_case_lists_hit_the_chunk_table_and_tail_edges():
    K = O.OPT_CHUNK
    e = O.ADAM_CASES["edges"]["sizes"]
    assert {1, 2, 3, 4, 5, K - 1, K, K + 1, 2 * K + 1} <= set(e)
    assert {n % K for n in e if n >= K - 1} == {K - 1, 0, 1} and {n % 4 for n in e if n} == {0, 1, 2, 3}
    z = e.index(0)
    assert 0 < z < len(e) - 1                                                # the zero-element parameter sits in the middle
    assert O.ADAM_CASES["edges"]["zero_grad"] < O.ADAM_CASES["edges"]["n_a"] and O.ADAM_GROUP_A["weight_decay"] == 0
    assert len(O.adam_launch_plan(e)) == 1 and [r[0] for r in O.adam_launch_plan(e)[0][1]] == [i for i in range(len(e)) if i != z]

    s = O.ADAM_CASES["table40"]["sizes"]
    plan = O.adam_launch_plan(s)
    assert len(s) == 81 and [len(rows) for _, rows in plan] == [40, 40, 1]
    assert all(k == 1 for _, _, k in plan[0][1][:39]) and plan[0][1][39] == (39, 39, 3)      # multi-chunk tensor = 40th row
    assert plan[1][0] == 42 and plan[1][1][0] == (40, 0, 1)                  # first_chunk restarts, chunk_base carries on
    assert plan[2][0] == 42 + 40

    s = O.ADAM_CASES["table41"]["sizes"]
    plan = O.adam_launch_plan(s)
    assert [len(rows) for _, rows in plan] == [40, 6] and all(k == 1 for _, _, k in plan[0][1])
    assert plan[1][0] == 40 and plan[1][1][0] == (40, 0, 3) and plan[1][1][1] == (41, 3, 1)  # the 41st tensor opens launch 2

    for case, c in O.ADAM_CASES.items():
        assert 0 < c["n_a"] < len(c["sizes"]) or case == "table41"
    assert O.ADAM_CASES["table41"]["n_a"] == 41                              # both groups on both sides of the table edge
    assert O.ADAM_GROUP_A != O.ADAM_GROUP_B and all(O.ADAM_GROUP_A[k] != O.ADAM_GROUP_B[k] for k in ("lr", "betas", "eps", "weight_decay"))
    st = O.adam_state("late")
    assert all(s["step"] == O.LATE_STEP and (s["v"] > 0).all() for s in st)
    assert 1 - O.ADAM_GROUP_B["betas"][1] ** O.LATE_STEP == 1.0              # bias corrections are 1 to double precision
