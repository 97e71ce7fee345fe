"""Fixtures and the float64 restatement for the backward of the truncated log-prob (include/set_hip.h
set_sample_logp_bwd_opts_f32), shared by tests/test_truncated_logp_bwd_cpu.py (which asserts, on the oracle alone, that every row
keeps clear of the top-k and top-p boundaries) and tests/test_hip_truncated_logp_bwd.py (which may therefore demand exact kept
sets).  Built on tests/trunc_sample_oracle.py."""
import numpy as np

import trunc_sample_oracle as TS

ROWS = [1, 9, 15]                                           # 15 is logged as a 3 x 5 (T, B) block
SHAPES = [(203, 203), (204, 204), (1027, 1028), (12292, 12292)]      # (V, ld): scalar; float4; float4 with a tail; forward generic
# temperature alone (the key must be 0), top-k, top-p, both with a temperature, top_k >= V (off)
OPTS = [(0.5, 0, 1.0), (2.0, 0, 1.0), (1.0, 5, 1.0), (1.0, 0, 0.9), (0.7, 5, 0.9), (1.0, 10 ** 6, 1.0)]
K_MARGIN = 1e-3                # no word lies this close to the top-k boundary value without being equal to it
Y_MAX = 30.0


# (V, R) -> seed of rows() where seed 0 leaves a top-p target too close to a group boundary (asserted on the oracle alone by
# tests/test_truncated_logp_bwd_cpu.py)
SEED = {(203, 15): 1, (204, 9): 1, (12292, 15): 1}


def rows(V, R, seed=None):
    """R distinct rows of V logits: a head of 12 words 0.3 .. 1.2 apart from 4 downwards, which both top_k = 5 and the top-p
    targets cut through at well-separated values, above a tail around -12 that is clipped so that |x / T| <= 30 for T >= 0.5"""
    rng = np.random.default_rng([V, R, SEED.get((V, R), 0) if seed is None else seed])
    x = np.clip(rng.standard_normal((R, V)) - 12.0, -14.9, -10.5)
    for r in range(R):
        idx = rng.choice(V, 12, replace=False)
        x[r, idx] = 4.0 - np.cumsum(rng.uniform(0.3, 1.2, 12))
    return x.astype(np.float32)


def order_key(y):
    """csrc/epilogue.hip order_key on float32 values: a < b as floats <=> key(a) < key(b); both zeros share a key"""
    u = np.ascontiguousarray(y, np.float32).view(np.uint32)
    k = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    k[u == np.uint32(0x80000000)] = np.uint32(0x80000000)
    return k


def margins(x, opts):
    """(distance of the top-p target from a group boundary, distance of the top-k boundary value from the nearest other value)"""
    T, top_k, top_p = opts
    y = TS.scaled(x, T).astype(np.float64)
    _, dist = TS.kept_set(y, top_k, top_p)
    gap = np.inf
    if 0 < top_k < y.shape[1]:
        tk = -np.partition(-y, top_k - 1, axis=1)[:, top_k - 1]
        d = np.abs(y - tk[:, None])
        gap = float(np.where(d == 0, np.inf, d).min())
    return float(dist.min()), gap


def grad64(x, opts, raw, g):
    """float64 autograd of the masked log-softmax of the float32-scaled rows, gathered at raw (rows with raw < 0: zeros), times
    g; the chain through y = x * inv_t multiplies by the float32 reciprocal -> (d (R, V), kept (R, V), p (R, V), inv_t)"""
    import torch
    T, top_k, top_p = opts
    y32 = TS.scaled(x, T)
    kept, _ = TS.kept_set(y32, top_k, top_p)
    inv_t = float(np.float32(1.0) / np.float32(T))
    y = torch.from_numpy(y32.astype(np.float64)).requires_grad_(True)
    lsm = torch.log_softmax(torch.where(torch.from_numpy(kept), y, torch.full_like(y, -np.inf)), 1)
    live = torch.from_numpy(raw >= 0)
    pick = lsm.gather(1, torch.from_numpy(np.maximum(raw, 0))[:, None])[:, 0]
    (torch.where(live, pick, torch.zeros_like(pick)) * torch.from_numpy(g.astype(np.float64))).sum().backward()
    return y.grad.numpy() * inv_t, kept, np.exp(lsm.detach().numpy()), inv_t
