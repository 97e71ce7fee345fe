"""The shapes of tests/test_hip_step_stages.py and the route each of them is there for.

Which code a decode timestep runs depends on the row count and the dimensions only (the SET_* switches are read once per
process and stay at their defaults in the suite).  The three predicates below restate the host-side conditions; the CPU test
tests/test_step_stage_oracle_cpu.py asserts that every grid entry still reaches the route named in its id, so a retune of a
threshold cannot silently empty a cell of the GPU grid: it fails there, and the shape is to be changed.
"""

BASE = dict(D=64, A=32, F=128, V=203, T=9, R=7, adaptive=0)
STEPS = 3


def vis_fsn(M, F, R=36):
    """feature slices of the 256-thread visual role — csrc/attention.hip:678-691 (vis_fsn), defaults SET_ATT_MIN_COLS = 2048,
    SET_ATT_SMALL_SLICES = 1"""
    small = M < 64
    mc = 128 if small else (1024 if R > 48 else 2048)
    want = 128 if small else 512
    fsn = 1
    while M * fsn < want and F // (fsn * 2) >= mc and F % (fsn * 2 * 4) == 0:
        fsn *= 2
    return fsn


def cap_dsn(M, Dh):
    """column slices of the 256-thread caption role — csrc/attention.hip:262-268 (cap_dsn), SET_ATT_SMALL_SLICES = 1"""
    dsn = 1
    if M >= 64:
        return 1
    while M * dsn < 128 and Dh // (dsn * 2) >= 128 and Dh % (dsn * 2 * 4) == 0:
        dsn *= 2
    return dsn


def editnet_route(bt, D, F, R):
    """what set_editnet_step launches for `bt` rows:
      v2       csrc/attention.hip:727   `v2 && M <= v2_maxm && F <= 2048 && Dh <= 1024` (SET_ATT_V2 = 1, SET_ATT_V2_MAXM = 64)
      fsn/dsn  csrc/attention.hip:704,733: only the 256-thread kernel slices (v2: one workgroup per row and role)
      fused    csrc/editnet.hip:384,438-439  `fusedk = D % 64 == 0`, `fused = fusedk && bt >= 17` (SET_FUSED_MIN_ROWS = 17)
      wide     csrc/editnet.hip:421,467  `if (bt > 64) ....bm_hint = ...` of phases B and F
      table    csrc/editnet.hip:384-385  a token table is used iff attached and `fusedk`"""
    v2 = bt <= 64 and F <= 2048 and D <= 1024
    fsn = 1 if v2 else vis_fsn(bt, F, R)
    return dict(v2=v2, fsn=fsn, fcols=F // fsn, dsn=1 if v2 else cap_dsn(bt, D), fused=D % 64 == 0 and bt >= 17,
                wide=bt > 64, table=D % 64 == 0)


def dcnet_route(bt, D, C):
    """what set_dcnet_step launches for `bt` rows:
      v2     csrc/attention.hip:284  `v2 && M <= v2_maxm && Dh <= 1024` of the stand-alone caption attention, Dh = 2C
      dsn    csrc/attention.hip:289
      table  csrc/dcnet.hip:216-218  `C % 128 == 0 && D % 64 == 0`"""
    v2 = bt <= 64 and 2 * C <= 1024
    return dict(v2=v2, dsn=1 if v2 else cap_dsn(bt, 2 * C), table=C % 128 == 0 and D % 64 == 0)


# id -> dims changed from BASE, the (B of the workspace, bt of the steps) runs, and the route every run must reach
EDITNET_GRID = {
    "rows1": dict(dims=dict(T=1, R=1, V=37), runs=[(1, 1)], route=dict(v2=True, fused=False, wide=False)),
    "rows16": dict(dims={}, runs=[(16, 16)], route=dict(v2=True, fused=False, wide=False)),
    "rows17": dict(dims={}, runs=[(17, 17)], route=dict(v2=True, fused=True, wide=False)),
    "rows64": dict(dims={}, runs=[(64, 64)], route=dict(v2=True, fused=True, wide=False)),
    "rows65": dict(dims={}, runs=[(65, 65)], route=dict(v2=False, fsn=1, dsn=1, fused=True, wide=True)),
    "rows130": dict(dims={}, runs=[(130, 130)], route=dict(v2=False, fsn=1, dsn=1, fused=True, wide=True)),
    "shrunk": dict(dims={}, runs=[(130, 70), (24, 17)], route=dict(fused=True)),
    # 9 rows: 16 slices of 256 columns; 5 rows: the floor of the small-batch rule, 32 slices of 128 columns
    "fslice_small": dict(dims=dict(D=256, F=4096), runs=[(9, 9), (5, 5)], route=dict(v2=False, dsn=2, fused=False, wide=False)),
    "fslice_mid": dict(dims=dict(F=4096), runs=[(70, 70)], route=dict(v2=False, fsn=2, fcols=2048, dsn=1, fused=True, wide=True)),
    "adaptive_mid": dict(dims=dict(R=49, F=2048, adaptive=1), runs=[(70, 70)],
                         route=dict(v2=False, fsn=2, fcols=1024, dsn=1, fused=True, wide=True)),
    "adaptive_small": dict(dims=dict(R=100, adaptive=1), runs=[(5, 5)], route=dict(v2=True, fused=False, wide=False)),
    "nofuse": dict(dims=dict(D=96), runs=[(17, 17)], route=dict(v2=True, fused=False, table=False)),
}
# what differs between the runs of one entry: the two runs of `shrunk` sit on different sides of the attention switch
RUN_ROUTES = {("shrunk", 130, 70): dict(v2=False, fsn=1, dsn=1, wide=True), ("shrunk", 24, 17): dict(v2=True, wide=False),
              ("fslice_small", 9, 9): dict(fsn=16, fcols=256), ("fslice_small", 5, 5): dict(fsn=32, fcols=128)}

DCNET_DIMS = dict(D=64, A=32, C=32, E=64, V=203, T=9)          # oracle.cases dcnet_small
DCNET_GRID = {
    "rows1": dict(dims=dict(T=1), runs=[(1, 1)], route=dict(v2=True)),
    "rows16": dict(dims={}, runs=[(16, 16)], route=dict(v2=True)),
    "rows17": dict(dims={}, runs=[(17, 17)], route=dict(v2=True)),
    "rows64": dict(dims={}, runs=[(64, 64)], route=dict(v2=True)),
    "rows65": dict(dims={}, runs=[(65, 65)], route=dict(v2=False, dsn=1)),
    "shrunk": dict(dims={}, runs=[(130, 70)], route=dict(v2=False, dsn=1)),
}


def editnet_dims(gid):
    return dict(BASE, **EDITNET_GRID[gid]["dims"])


def dcnet_dims(gid):
    return dict(DCNET_DIMS, **DCNET_GRID[gid]["dims"])


def editnet_cases():
    """(id, B, bt, table) of every GPU case: each entry without and with the inference token table, `nofuse` (D % 64 != 0: the
    kernels take no table) without only"""
    out = []
    for gid, e in EDITNET_GRID.items():
        for B, bt in e["runs"]:
            for table in ((False, True) if editnet_dims(gid)["D"] % 64 == 0 else (False,)):
                out.append((gid, B, bt, table))
    return out


def dcnet_cases():
    return [(gid, B, bt) for gid, e in DCNET_GRID.items() for B, bt in e["runs"]]


def case_id(c):
    return "%s-%dx%d%s" % (c[0], c[1], c[2], "-table" if len(c) > 3 and c[3] else "")
