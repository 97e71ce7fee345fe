"""The shapes of tests/test_hip_prologue_stages.py and the route each of them is there for.

Which code the decode prologue (set_editnet_begin / set_dcnet_begin) runs depends on the dims, the row count and two switches
that are read once per process (SET_ENC_PERSISTENT, SET_ENC_PERSISTENT_MAXB): the GPU test runs one child process per SETTING.
The predicates below restate the host-side conditions; tests/test_prologue_stage_oracle_cpu.py asserts that every grid entry
still reaches the route named in its id and that the entries together reach every tile variant of the persistent encoder, so a
retuned threshold fails there, on the CPU, and the shape is to be changed.
"""
import numpy as np

SETTINGS = {"default": {}, "maxb128": {"SET_ENC_PERSISTENT_MAXB": "128"}, "off": {"SET_ENC_PERSISTENT": "0"}}
SCALES = dict(emb_scale=3.0, fc_scale=8.0, gain=3.0)             # the weight scales of tests/test_hip_shapes.py


def setting_switches(setting):
    """(SET_ENC_PERSISTENT, SET_ENC_PERSISTENT_MAXB) under a setting — csrc/encoder_persistent.hip:380-381, defaults 1 and 32"""
    env = SETTINGS[setting]
    return int(env.get("SET_ENC_PERSISTENT", 1)), int(env.get("SET_ENC_PERSISTENT_MAXB", 32))


def fused(D):
    """the fused per-step kernel (and, before it, the persistent one) is asked for — csrc/editnet.hip:189 `D % 128 == 0`,
    csrc/dcnet.hip:99 `C % 128 == 0` (SET_NO_FUSED = 0); csrc/gemm_fused.hip:519 refuses every other D"""
    return D % 128 == 0


def persistent_encoder_ok(B, D, on=1, maxb=32):
    """csrc/encoder_persistent.hip:375-386 (no earlier barrier fault, the device lock is ours)"""
    return bool(on) and 1 <= B <= maxb and ((B <= 128 and D in (512, 1024)) or (B <= 256 and D == 64))


def persistent(B, D, setting="default"):
    """csrc/editnet.hip:215 `fused && perm && enc_bar && persistent_encoder_ok(B, D, T)` (perm: :209, B <= 4096),
    csrc/dcnet.hip:120 `fused && B <= 4096 && persistent_encoder_ok(B, C, T)`"""
    return fused(D) and B <= 4096 and persistent_encoder_ok(B, D, *setting_switches(setting))


def instantiation(B, D):
    """(NT, KB) of encoder_persistent_k — csrc/encoder_persistent.hip:456-468: NT 16-row tiles held (2 up to 32 rows, 8 up to
    128; 16 only at D = 64), KB = D / 64 k-blocks per wave"""
    nt = (B + 15) // 16
    if D in (512, 1024):
        return (2 if nt <= 2 else 8), D // 64
    return (2 if nt <= 2 else (8 if nt <= 8 else 16)), 1


def tile_variant(NT, nactive):
    """tiles contracted in a step with `nactive` live rows — csrc/encoder_persistent.hip:158,166-173 (0: no contraction)"""
    nt_act = (nactive + 15) >> 4
    if nt_act == 0:
        return 0
    for n, above in ((16, 12), (12, 8), (8, 6), (6, 4), (4, 2)):
        if NT >= n and nt_act > above:
            return n
    return 2 if nt_act > 1 else 1


def editnet_table(D):
    """the prologue gathers the encoder's input projection from an attached token table — csrc/editnet.hip:191 `fused && ...`
    (the module attaches one at D % 64 == 0, editnet.py _token_table_supported; the unfused encoder ignores it)"""
    return fused(D)


def dcnet_table(D, C):
    """csrc/dcnet.hip:100 `tok_table && fused && D % 64 == 0`"""
    return fused(C) and D % 64 == 0


def row_list(B, T, D, adaptive):
    """the cap projections launch contracts the valid rows only — csrc/editnet.hip:300 `pro_rowlist && !adaptive &&
    gemm_row_list_ok(p, 4)`: csrc/gemm_f32.hip:697,800 every tile class but the <= 16-row one (SET_GEMM_BM16_UPTO = 16); the
    list is written by the row-ranking launch, which runs for the fused encoders only (csrc/editnet.hip:209-212)"""
    return fused(D) and B <= 4096 and not adaptive and B * T > 16


def editnet_pv(B, D, A, T, R, V, adaptive):
    """pd_pv is computed — csrc/editnet.hip:314 editnet_persistent_ok(d, 1): csrc/decode_persistent_wide.hip:832-836,777-786
    (PDW_MAXB = 16, PDEC_KB = 16, PDEC_TMAX = 32, PDEC_RREG = 36, PDEC_FC_TILES = 3; the LDS bound holds on this device)"""
    G = D // 4
    return (not adaptive and 1 <= B <= 16 and D == 1024 and A == 512 and T <= 32 and R <= 36 and R % 2 == 0 and T % 2 == 0
            and (V + G - 1) // G <= 48 and B * R <= 4 * G and B * T <= 4 * G)


def dcnet_pc(B, D, A, C, E, T, V):
    """pd_pc is computed — csrc/dcnet.hip:194 dcnet_persistent_ok(d, 1): csrc/decode_persistent.hip:700-708 (PDEC_MAXB = 8)"""
    G = D // 4
    return 1 <= B <= 8 and D == 1024 and E == D and 2 * C == D and A == 512 and T <= 32 and (V + G - 1) // G <= 48


# ---- lengths ---------------------------------------------------------------------------------------------------------------
def lengths(B, T, rule):
    """(B,) int64, every length >= 1 and the longest = T.
      "cycle"       1, 2, .. T, 1, 2, ..
      "ragged"      T, T-1, .. 1, T, ..   (row 0 has the full length whatever B is)
      "full"        every row T
      (n0, n1, ..)  nactive: #{b : len_b > t} = n_t, spread over the rows by a fixed shuffle: perm is not the identity, has ties"""
    if rule == "cycle":
        lens = 1 + np.arange(B) % T
    elif rule == "ragged":
        lens = T - np.arange(B) % T
    elif rule == "full":
        lens = np.full(B, T)
    else:
        n = list(rule) + [0]
        assert len(rule) == T and n[0] == B and all(a >= b for a, b in zip(n, n[1:])) and n[T - 1] >= 1
        lens = np.concatenate([np.full(n[t] - n[t + 1], t + 1) for t in range(T)])
        lens = lens[np.random.RandomState(1234 + B).permutation(B)]
    lens = lens.astype(np.int64)
    assert lens.shape == (B,) and lens.min() >= 1 and lens.max() == T
    return lens


def nactive_of(lens, T):
    return [int((lens > t).sum()) for t in range(T)]


def tokens(seed, B, T, V, lens):
    """(B,T) ids in [0, V), zero behind a row's length; 0 and V - 1 sit at valid positions"""
    from show_edit_tell_amd import synth
    seq = synth.integers(seed, "prologue.tok", (B, T), 0, V)
    if B >= 2:
        seq[0, 0], seq[1, 0] = 0, V - 1
    else:
        assert lens[0] >= 2
        seq[0, 0], seq[0, 1] = 0, V - 1
    seq = seq * (np.arange(T)[None, :] < lens[:, None])
    valid = seq[np.arange(T)[None, :] < lens[:, None]]
    assert (valid == 0).any() and (valid == V - 1).any()
    return seq.astype(np.int64)


# ---- the grid --------------------------------------------------------------------------------------------------------------
SMALL = dict(A=64, F=128, R=4, adaptive=0)
D128 = dict(SMALL, D=128, V=64)
D512 = dict(SMALL, D=512, V=150)
N128 = (128, 97, 96, 81, 80, 65, 64, 49, 48, 33, 32, 17, 16, 1)

# id -> dims, B, T, the lengths rule, the setting it runs under, and the route it must reach: enc = "unfused" / "fused" /
# "persistent", inst = (NT, KB), variants = the tile variants its steps take in order of first use
EDITNET_GRID = {
    "unfused_b5": dict(dims=dict(SMALL, D=64, V=64), B=5, T=9, lens="ragged", route=dict(enc="unfused", rows=False)),
    "unfused_b70": dict(dims=dict(SMALL, D=96, V=64), B=70, T=9, lens="ragged", route=dict(enc="unfused", rows=False)),
    "fused_b31": dict(dims=D128, B=31, T=7, lens="cycle", route=dict(enc="fused", rows=True)),
    "fused_b32": dict(dims=D128, B=32, T=7, lens="cycle", route=dict(enc="fused", rows=True)),
    "fused_b33": dict(dims=D128, B=33, T=7, lens="cycle", route=dict(enc="fused", rows=True)),
    "fused_b65": dict(dims=D128, B=65, T=7, lens="cycle", route=dict(enc="fused", rows=True)),
    "fused_t1": dict(dims=D128, B=3, T=1, lens="full", route=dict(enc="fused", rows=False)),
    "fused_d256_b40": dict(dims=dict(SMALL, D=256, V=64), B=40, T=5, lens="ragged", route=dict(enc="fused", rows=True)),
    # adaptive features: the region mask, and the row list switched off at a row count that would take it
    "fused_adaptive_b33": dict(dims=dict(D128, R=6, adaptive=1), B=33, T=7, lens="cycle", route=dict(enc="fused", rows=False)),
    "pers_b1": dict(dims=D512, B=1, T=5, lens="ragged", route=dict(enc="persistent", inst=(2, 8), variants=[1])),
    "pers_b16": dict(dims=D512, B=16, T=5, lens="ragged", route=dict(enc="persistent", inst=(2, 8), variants=[1])),
    "pers_b17": dict(dims=D512, B=17, T=4, lens=(17, 16, 1, 1), route=dict(enc="persistent", inst=(2, 8), variants=[2, 1])),
    "pers_b32": dict(dims=D512, B=32, T=6, lens="ragged", route=dict(enc="persistent", inst=(2, 8), variants=[2, 1])),
    "pers_t1": dict(dims=D512, B=4, T=1, lens="full", route=dict(enc="persistent", inst=(2, 8), variants=[1])),
    "pers_b33_default": dict(dims=D512, B=33, T=4, lens="ragged", route=dict(enc="fused", rows=True)),
    "pers8_b33": dict(dims=D512, B=33, T=3, lens=(33, 32, 1), setting="maxb128",
                      route=dict(enc="persistent", inst=(8, 8), variants=[4, 2, 1])),
    "pers8_b128": dict(dims=D512, B=128, T=14, lens=N128, setting="maxb128",
                       route=dict(enc="persistent", inst=(8, 8), variants=[8, 6, 4, 2, 1])),
    "pers8_b129": dict(dims=D512, B=129, T=3, lens="ragged", setting="maxb128", route=dict(enc="fused", rows=True)),
    "pers_d1024_b17": dict(dims=dict(SMALL, D=1024, V=150), B=17, T=4, lens="ragged",
                           route=dict(enc="persistent", inst=(2, 16), variants=[2, 1])),
    "fusedstep_d512_b17": dict(dims=D512, B=17, T=4, lens=(17, 16, 1, 1), setting="off", route=dict(enc="fused", rows=True)),
    "fusedstep_d512_b128": dict(dims=D512, B=128, T=14, lens=N128, setting="off", route=dict(enc="fused", rows=True)),
}
# set_caption_encoder_f32: the fused step without perm / nactive (order == NULL, csrc/ops.hip:534), no token table
OP_GRID = {"op_b33": dict(dims=dict(D=128, V=64), B=33, T=6, lens="ragged", route=dict(enc="fused"))}

# check_dims (csrc/dcnet.hip:38-40) ties the widths: D + 2C = 2E.  C = 128 with D = 64 gives E = 160; C = 512 with D = 64, E = 544
DC_SMALL = dict(D=64, A=32, C=32, E=64, V=203)                       # oracle.cases dcnet_small
DC128 = dict(D=64, A=64, C=128, E=160, V=64)
DC512 = dict(D=64, A=64, C=512, E=544, V=150)
DCNET_GRID = {
    "dc_unfused_b70": dict(dims=DC_SMALL, B=70, T=9, lens="ragged", route=dict(enc="unfused", table=False)),
    "dc_fused_b33": dict(dims=DC128, B=33, T=7, lens="ragged", route=dict(enc="fused", table=True)),
    "dc_pers_b17": dict(dims=DC512, B=17, T=5, lens="ragged", route=dict(enc="persistent", inst=(2, 8), variants=[2, 1], table=True)),
    "dc_pers_t1": dict(dims=DC512, B=3, T=1, lens="full", route=dict(enc="persistent", inst=(2, 8), variants=[1], table=True)),
    "dc_pers8_b100": dict(dims=DC512, B=100, T=8, lens=(100, 97, 80, 49, 48, 17, 16, 1), setting="maxb128",
                          route=dict(enc="persistent", inst=(8, 8), variants=[8, 6, 4, 2, 1], table=True)),
}
GRIDS = {"editnet": EDITNET_GRID, "op": OP_GRID, "dcnet": DCNET_GRID}


def entry(model, gid):
    e = dict(GRIDS[model][gid])
    e.setdefault("setting", "default")
    e["lens"] = lengths(e["B"], e["T"], e["lens"])
    return e


def enc_dim(model, dims):
    """the hidden width of the encoder's recurrence"""
    return dims["C"] if model == "dcnet" else dims["D"]


def route(model, gid):
    """what the prologue of a grid entry runs, by the predicates above"""
    e = entry(model, gid)
    dims, B, T = e["dims"], e["B"], e["T"]
    D = enc_dim(model, dims)
    r = {}
    if persistent(B, D, e["setting"]):
        NT, KB = instantiation(B, D)
        seen = []
        for n in nactive_of(e["lens"], T):
            v = tile_variant(NT, n)
            if v not in seen:
                seen.append(v)
        r.update(enc="persistent", inst=(NT, KB), variants=seen)
    else:
        r["enc"] = "fused" if fused(D) else "unfused"
    if model == "editnet":
        r["table"] = editnet_table(D)
        r["rows"] = row_list(B, T, D, dims["adaptive"])
        r["pv"] = editnet_pv(B, D, dims["A"], T, dims["R"], dims["V"], dims["adaptive"])
    elif model == "dcnet":
        r["table"] = dcnet_table(dims["D"], dims["C"])
        r["pc"] = dcnet_pc(B, dims["D"], dims["A"], dims["C"], dims["E"], T, dims["V"])
    else:
        r["table"] = False
    return r


def cases(setting=None):
    """(model, id, table) of every GPU case: each entry whose prologue takes a token table runs without and with one"""
    out = []
    for model, grid in GRIDS.items():
        for gid in grid:
            if setting is not None and entry(model, gid)["setting"] != setting:
                continue
            for table in ((False, True) if route(model, gid)["table"] else (False,)):
                out.append((model, gid, table))
    return out


def case_id(c):
    return "%s-%s%s" % (c[0], c[1], "-table" if c[2] else "")


def seed_of(model, gid):
    return 300 + 50 * sorted(GRIDS).index(model) + sorted(GRIDS[model]).index(gid)


def model_key(model, dims):
    """entries with the same key share one model (the operator's encoder sits in an EditNet of its own)"""
    return model + "".join("-%s%d" % (k, v) for k, v in sorted(dims.items()) if k != "R")


def state(model, dims):
    """the synthetic state_dict of an entry's dims (float32 numpy); the operator runs the encoder of an EditNet"""
    from show_edit_tell_amd import synth
    if model == "dcnet":
        return synth.dcnet_state(37, dims["V"], dims["D"], dims["A"], dims["C"], dims["E"], **SCALES)
    if model == "op":
        dims = dict(dims, A=32, F=32)
    return synth.editnet_state(31, dims["V"], dims["D"], dims["A"], dims["F"], **SCALES)


def inputs(model, gid):
    """seq (B,T), lens (B,), and for EditNet X (B,R,F) and the caller's image_mean (adaptive features) or None"""
    from show_edit_tell_amd import synth
    e = entry(model, gid)
    dims, B, T, seed = e["dims"], e["B"], e["T"], seed_of(model, gid)
    out = dict(lens=e["lens"], seq=tokens(seed, B, T, dims["V"], e["lens"]), X=None, mean=None)
    if model == "editnet":
        R, F = dims["R"], dims["F"]
        X = synth.features(seed, B, R, F)
        if dims["adaptive"]:
            nv = 1 + synth.integers(seed, "prologue.nvalid", (B,), 0, R)
            nv[0], nv[1] = 1, R                          # a row with one valid region and a row with all of them
            X = X * (np.arange(R)[None, :] < nv[:, None])[:, :, None].astype(np.float32)
            out["mean"] = (X.sum(1) / nv[:, None].astype(np.float32)).astype(np.float32)
        out["X"] = X
    return out
