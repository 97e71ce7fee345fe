"""Float64 restatements of the training tail (csrc/loss.hip, csrc/optim.hip) in numpy, and the input families and case
lists that tests/test_hip_train_tail.py runs.  Everything takes the float32 inputs as they are and computes in float64;
tests/test_train_tail_oracle_cpu.py holds it against torch in float64 on the CPU and asserts what the families claim."""
import numpy as np

XE_MAX_T = 64
OPT_CHUNK = 16384
OPT_MAX_TENSORS = 40
UNIT = 2.0 ** -24


# ------------------------------------------------------------------------------------------------
# the operations
# ------------------------------------------------------------------------------------------------
def xe_rows(scores, targets, live):
    """scores (B, T, V) float32, targets (B, T) integer, live[t] = number of rows b < live[t] that count at time t.
    Returns (loss, lse, grad) as float64 arrays (T, B), (T, B), (T, B, V): loss = lse - x[target], grad = softmax - onehot.
    A row with b >= live[t] gives 0 in all three; a target outside [0, V) gives a NaN loss and a NaN gradient row."""
    x = np.asarray(scores).astype(np.float64).transpose(1, 0, 2)          # (T, B, V)
    tg = np.asarray(targets).astype(np.int64).T[:x.shape[0]]              # (T, B)
    T, B, V = x.shape
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        m = x.max(axis=2, keepdims=True)
        lse = (m + np.log(np.exp(x - m).sum(axis=2, keepdims=True)))[:, :, 0]
        grad = np.exp(x - lse[:, :, None])
    bad = (tg < 0) | (tg >= V)
    tc = np.where(bad, 0, tg)
    ti, bi = np.meshgrid(np.arange(T), np.arange(B), indexing="ij")
    loss = lse - x[ti, bi, tc]
    grad[ti, bi, tc] -= 1.0
    loss[bad] = np.nan
    grad[bad] = np.nan
    dead = np.arange(B)[None, :] >= np.asarray(live, dtype=np.int64)[:, None]
    loss[dead], lse[dead], grad[dead] = 0.0, 0.0, 0.0
    return loss, lse, grad


def mse(a, b):
    """sum((a - b)^2) and its gradients to a and to b"""
    d = np.asarray(a).astype(np.float64) - np.asarray(b).astype(np.float64)
    return float((d * d).sum()), 2.0 * d, -2.0 * d


def clip_adam(params, grads, state, groups, max_norm):
    """torch.nn.utils.clip_grad_norm_(params, max_norm) followed by torch.optim.Adam.step() (L2 weight decay: the decay is
    added to the gradient).  params / grads: lists of arrays; state: one dict(step, m, v) per tensor; groups: dicts with
    "params" (indices into the lists), "lr", "betas", "eps", "weight_decay".  Returns (new params, new state, total norm,
    clipped gradients); nothing passed in is changed."""
    g64 = [np.asarray(g).astype(np.float64) for g in grads]
    total = float(np.sqrt(sum(float((g * g).sum()) for g in g64)))
    coef = max_norm / (total + 1e-6)
    coef = coef if (coef < 1.0 or coef != coef) else 1.0                   # torch.clamp(max=1.0) keeps a NaN
    clipped = [g * coef for g in g64]
    new_p, new_s = [None] * len(params), [None] * len(params)
    for grp in groups:
        lr, (b1, b2), eps, wd = grp["lr"], grp["betas"], grp["eps"], grp["weight_decay"]
        for i in grp["params"]:
            p = np.asarray(params[i]).astype(np.float64)
            step = int(state[i]["step"]) + 1
            g = clipped[i] + wd * p if wd != 0 else clipped[i]
            m = np.asarray(state[i]["m"]).astype(np.float64)
            v = np.asarray(state[i]["v"]).astype(np.float64)
            m = m + (g - m) * (1.0 - b1)
            v = v * b2 + (1.0 - b2) * g * g
            bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
            new_p[i] = p - (lr / bc1) * (m / (np.sqrt(v) / np.sqrt(bc2) + eps))
            new_s[i] = dict(step=step, m=m, v=v)
    return new_p, new_s, total, clipped


# ------------------------------------------------------------------------------------------------
# cross-entropy: shapes, layouts, lengths, row families
# ------------------------------------------------------------------------------------------------
XE_VS = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 511, 513, 1003, 9490)
XE_TS = (1, 2, 64)
XE_LAYOUTS = ("batch_major", "time_major", "slice")
XE_LENS = ("full", "ragged", "dead")
# (B, T, V, layout, lengths)
XE_SHAPES = (
    (3, 1, 1, "batch_major", "full"), (5, 2, 2, "time_major", "ragged"), (5, 64, 3, "slice", "dead"),
    (1, 2, 4, "slice", "full"), (4, 1, 5, "batch_major", "ragged"), (5, 64, 63, "time_major", "ragged"),
    (2, 2, 64, "batch_major", "dead"), (5, 1, 65, "time_major", "full"), (1, 64, 255, "batch_major", "dead"),
    (3, 2, 256, "slice", "ragged"), (5, 2, 257, "time_major", "dead"), (4, 64, 511, "slice", "full"),
    (5, 1, 513, "slice", "ragged"), (3, 2, 1003, "batch_major", "full"), (5, 64, 9490, "time_major", "ragged"),
)
XE_FAMILY_VS = (5, 257, 1003)
XE_FAMILIES = ("randn3", "equal", "peak_on", "peak_off", "offset_p1000", "offset_m1000", "ascending", "descending",
               "underflow", "max_at_0", "max_at_last", "max_at_255", "max_at_256", "neg_inf")
XE_FAMILY_B, XE_FAMILY_T = 3, 2


def xe_lengths(kind, B, T):
    """decode lengths, non-increasing over the batch.  full: all T.  ragged: from T down (T = 1: the second half of the
    batch has length 0).  dead: ragged, but nobody reaches the last timestep (live[T - 1] = 0)."""
    if kind == "full":
        return [T] * B
    lens = [T - (b * T) // B for b in range(B)] if T > 1 else [1 if b <= B // 2 else 0 for b in range(B)]
    if kind == "dead":
        assert T > 1
        lens = [min(l, T - 1) for l in lens]
    return lens


def live_of(lens, T):
    return [sum(1 for l in lens if l > t) for t in range(T)]


def slice_width(V):
    """row pitch of the wider buffer of the "slice" layout: more than V and no multiple of 4, so rows are not 16-byte aligned"""
    return V + 1 if (V + 1) % 4 else V + 2


def xe_family(name, B, T, V, seed=0):
    """(scores (B, T, V) float32, targets (B, T + 1) int64: the caption with its start word, targets are caps[:, 1:])"""
    rng = np.random.default_rng([17, XE_FAMILIES.index(name), B, T, V, seed])
    x = (rng.standard_normal((B, T, V)) * 3.0).astype(np.float32)
    caps = rng.integers(0, V, (B, T + 1))
    tg = caps[:, 1:]
    bi, ti = np.meshgrid(np.arange(B), np.arange(T), indexing="ij")
    if name == "equal":
        x[:] = 0.75
    elif name in ("peak_on", "peak_off"):
        x = (x / 3.0).astype(np.float32)
        peak = rng.integers(0, V, (B, T))
        x[bi, ti, peak] += np.float32(60.0)
        tg[:] = peak if name == "peak_on" else (peak + 1 + rng.integers(0, max(V - 1, 1), (B, T))) % V
    elif name == "offset_p1000":
        x += np.float32(1000.0)
    elif name == "offset_m1000":
        x -= np.float32(1000.0)
    elif name in ("ascending", "descending"):
        row = np.linspace(-100.0, 0.0, V).astype(np.float32)
        x[:] = row if name == "ascending" else row[::-1]
    elif name == "underflow":
        x[:, :, ::3] -= np.float32(200.0)
        x[:, :, 1 % V] = np.maximum(x[:, :, 1 % V], np.float32(0.0))
    elif name.startswith("max_at_"):
        pos = {"0": 0, "last": V - 1, "255": min(255, V - 1), "256": min(256, V - 1)}[name[7:]]     # clipped to the row at V = 5
        x[:, :, pos] = np.abs(x).max(axis=2) + np.float32(2.0)
    elif name == "neg_inf":
        drop = rng.random((B, T, V)) < 0.5
        drop[bi, ti, tg] = False
        drop[:, :, 0] |= (tg != 0)                                      # at least one wherever V > 1
        x[drop] = -np.inf
    return x, caps


# ------------------------------------------------------------------------------------------------
# MSE
# ------------------------------------------------------------------------------------------------
MSE_GRID_LIMIT = 2048 * 256                   # elements one pass of mse_bwd_k's grid covers
MSE_SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 4099, MSE_GRID_LIMIT + 5)


def mse_inputs(n, seed=0):
    rng = np.random.default_rng([23, n, seed])
    return rng.standard_normal(n).astype(np.float32), (rng.standard_normal(n) * 0.5 + 0.25).astype(np.float32)


# ------------------------------------------------------------------------------------------------
# clip + Adam: tensor lists, hyper-parameters, gradients
# ------------------------------------------------------------------------------------------------
ADAM_GROUP_A = dict(lr=4e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0)
ADAM_GROUP_B = dict(lr=1e-3, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.01)
ADAM_MAX_NORMS = (0.25, 1e9)
ADAM_STEPS = 4
GRAD_MIN, GRAD_MAX = 1e-8, 1e3
_SMALL = (1, 2, 3, 4, 5, 257, 7, 64)
# name -> dict(sizes, n_a = how many leading tensors are in group A, zero_grad = index of the tensor whose gradient is 0)
ADAM_CASES = {
    "edges": dict(sizes=(1, 2, 3, 4, 5, 16383, 0, 16384, 16385, 2 * OPT_CHUNK + 1, 7), n_a=6, zero_grad=4),
    # 39 one-chunk tensors, a three-chunk tensor as the 40th row of the first table, 41 more: 81 in all
    "table40": dict(sizes=tuple(_SMALL[i % 8] for i in range(39)) + (2 * OPT_CHUNK + 77,) + tuple(_SMALL[(i + 3) % 8] for i in range(41)),
                    n_a=20, zero_grad=None),
    # 40 one-chunk tensors fill the first table: the three-chunk tensor is the 41st, row 0 of the second launch
    "table41": dict(sizes=tuple(_SMALL[(i + 1) % 8] for i in range(40)) + (2 * OPT_CHUNK + 3,) + (5, 257, 1, 6, 2), n_a=41, zero_grad=None),
    "flat": dict(sizes=(5, 16385, 100, 3), n_a=2, zero_grad=None),
    "late": dict(sizes=(1000, 16385), n_a=1, zero_grad=None),
    "misaligned": dict(sizes=(37, 260), n_a=1, zero_grad=None),
    "nan": dict(sizes=(5, 300, 16), n_a=1, zero_grad=None),
}
LATE_STEP = 100000


def adam_groups(case):
    c = ADAM_CASES[case]
    n = len(c["sizes"])
    return [dict(ADAM_GROUP_A, params=list(range(c["n_a"]))), dict(ADAM_GROUP_B, params=list(range(c["n_a"], n)))]


def adam_params(case):
    c = ADAM_CASES[case]
    rng = np.random.default_rng([29, sorted(ADAM_CASES).index(case)])
    return [rng.standard_normal(n).astype(np.float32) for n in c["sizes"]]


def adam_state(case):
    c = ADAM_CASES[case]
    if case != "late":
        return [dict(step=0, m=np.zeros(n, np.float32), v=np.zeros(n, np.float32)) for n in c["sizes"]]
    rng = np.random.default_rng([31])
    return [dict(step=LATE_STEP, m=(rng.standard_normal(n) * 0.1).astype(np.float32),
                 v=(rng.standard_normal(n) ** 2 * 0.01 + 1e-6).astype(np.float32)) for n in c["sizes"]]


def adam_grads(case, it):
    """gradients of step `it`: scale 3 on even steps, 0.01 on odd ones, every magnitude inside [GRAD_MIN, GRAD_MAX]; the
    case's zero_grad tensor gets exact zeros"""
    c = ADAM_CASES[case]
    rng = np.random.default_rng([37, sorted(ADAM_CASES).index(case), it])
    out = []
    for i, n in enumerate(c["sizes"]):
        g = rng.standard_normal(n) * (0.01 if it % 2 else 3.0)
        g = (np.where(g < 0, -1.0, 1.0) * np.clip(np.abs(g), GRAD_MIN, GRAD_MAX)).astype(np.float32)
        if i == c["zero_grad"]:
            g[:] = 0.0
        out.append(g)
    return out


def adam_launch_plan(sizes):
    """how set_clip_adam_f32 cuts a tensor list into launches: [(chunk_base, [(tensor index, first_chunk, chunks), ...])];
    a zero-element tensor takes no table row"""
    plan, rows, base, c = [], [], 0, 0
    for i, n in enumerate(sizes):
        if n == 0:
            continue
        if len(rows) == OPT_MAX_TENSORS:
            plan.append((base, rows))
            base, rows, c = base + c, [], 0
        k = (n + OPT_CHUNK - 1) // OPT_CHUNK
        rows.append((i, c, k))
        c += k
    if rows:
        plan.append((base, rows))
    return plan


# ------------------------------------------------------------------------------------------------
# errors in units
# ------------------------------------------------------------------------------------------------
def row_units(got, ref, scores_tbv):
    """max over (t, b) of |got - ref| / (2^-24 max(1, max |finite x_row|, |ref|)); NaN where the reference is NaN must be NaN"""
    x = np.where(np.isfinite(scores_tbv), np.abs(scores_tbv.astype(np.float64)), 0.0).max(axis=2)
    got = np.asarray(got, dtype=np.float64)
    nan = np.isnan(ref)
    if not np.array_equal(np.isnan(got), nan):
        return float("inf")
    scale = UNIT * np.maximum(1.0, np.maximum(x, np.abs(np.where(nan, 0.0, ref))))
    return float((np.abs(np.where(nan, 0.0, got - ref)) / scale).max())


def grad_units(got, ref, dloss):
    """max |got - ref * dloss| / (2^-24 |dloss|)"""
    got = np.asarray(got, dtype=np.float64)
    nan = np.isnan(ref)
    if not np.array_equal(np.isnan(got), nan):
        return float("inf")
    return float((np.abs(np.where(nan, 0.0, got - ref * dloss)) / (UNIT * abs(dloss))).max()) if got.size else 0.0


def tensor_units(got, ref):
    """max |got - ref| / (2^-24 max(1, max |ref|)) of one tensor (or scalar)"""
    got, ref = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(ref, dtype=np.float64).reshape(-1)
    if got.size == 0:
        return 0.0
    if not np.isfinite(got).all():
        return float("inf")
    return float(np.abs(got - ref).max() / (UNIT * max(1.0, np.abs(ref).max())))
