"""The schedule behind the trunk (fp_nn.hip, plan_heads) asked on the host, no GPU: fpt_plan_heads returns what the refiner heads, the
scorer's feature pass and its cross-attention head would launch.  Every plan is held to the table written out below, for every batch
1..FP_MAX_BATCH in f16 and bf16, with the product's defaults and under every switch of the test build (HeadsOverride)."""
import ctypes as C

import numpy as np
import pytest

from foundationpose_cpp_amd import _lib

N_MAX = 2377                                   # include/foundationpose_amd.h FP_MAX_BATCH
F16, BF16, FP8 = 0, 1, 2                       # fp_nn.h DT_*
REFINER, FEATURES, HEAD = 0, 1, 2              # fp_nn.hip HeadsPass
QKV_LINEAR, QKV_TILE, QKV_GROUPED = 0, 1, 2    # QkvForm
ATT_32, ATT_SKV = 0, 1                         # AttKernel
TAIL_NONE, TAIL_ONE_1, TAIL_ONE_5, TAIL_GROUPED_CHAIN, TAIL_HEAD_CHAIN = range(5)                  # TailForm
POOL_TAIL_PDOT, POOL_LN_PMEAN, POOL_LN_MEAN, POOL_LN_TOKEN_MEAN, POOL_TOKEN_MEAN = range(5)        # PoolForm
RO_ENC_HEADS, RO_SMALL_LINEAR2_POSE, RO_SMALL_LINEAR2, RO_SMALL_LINEAR = range(4)                  # ReadoutKernel
FIELDS = ("qkv", "qkv_ablate", "qkv_grid", "qkv_lds", "att", "remap", "att_ablate", "B", "T", "pitch", "nq", "att_grid", "att_block",
          "att_lds", "tail", "pool", "readout", "fuse", "tail_tiles", "tail_grid", "tail_lds")

# the named thresholds of fp_nn.hip, restated
LDS_QKV_TILE = 16 * 80 * 64
LDS_ATT_SKV = 4 * 2 * (32 * 256 + 8 * 1056)
LDS_TAIL_1 = 16 * 16 * 64 + 2 * 8 * 16 * 4
LDS_TAIL_5 = 16 * 80 * 64 + 2 * 8 * 80 * 4 + 4 * 8192
# fpt_set_att_variant ids that remain -> (XCD remap, ablation bits)
ATT_VARIANTS = {1: (1, 0), 8: (0, 0), 16: (1, 16), 17: (1, 1), 18: (1, 2), 19: (1, 32), 20: (1, 4), 22: (1, 6), 24: (1, 8), 30: (1, 14), 31: (1, 15)}
RETIRED_ATT_VARIANTS = (2, 3, 5, 7, 9, 10)     # the round-1 kernel, 8 waves per workgroup, the lazy running maximum


class Planner:
    def __init__(self):
        self.L = _lib.test_lib()
        self.L.fpt_plan_heads.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        self.L.fpt_plan_heads.restype = C.c_int
        self.f = np.zeros(18, np.int32)
        self.t = np.zeros(3, np.int32)
        self.defaults()

    def defaults(self):
        L = self.L
        L.fpt_set_enc_tail(1); L.fpt_set_ln_pmean(1); L.fpt_set_fuse_pose(1); L.fpt_set_qkv_ablate(0); L.fpt_set_att_variant(1)

    def plan(self, kind, N, dt, offer=0):
        self.f[:] = -1
        self.t[:] = -1
        assert self.L.fpt_plan_heads(kind, N, dt, offer, self.f.ctypes.data, self.t.ctypes.data) == 0, (kind, N, dt, offer)
        return dict(zip(FIELDS, self.f.tolist() + self.t.tolist()))


@pytest.fixture()
def P():
    p = Planner()
    yield p
    p.defaults()


def attention(B, T, pitch, variant=1):
    """the attention launch of the table: attention32_kernel on 128-row query tiles, (tiles, head, sequence) workgroups of 256 threads;
    the split-key kernel (32-row tiles, dynamic LDS) when that grid would have at most 64 workgroups and the sequence is longer than 32
    tokens -- in the shipped form only"""
    remap, abl = ATT_VARIANTS.get(variant, ATT_VARIANTS[1])           # a retired id is IGNORED: the shipped kernel
    shipped = variant not in ATT_VARIANTS or variant == 1
    nq = -(-T // 128)
    if shipped and nq * 4 * B <= 64 and T > 32:
        nq = -(-T // 32)
        return dict(att=ATT_SKV, remap=1, att_ablate=0, B=B, T=T, pitch=pitch, nq=nq, att_grid=nq * 4 * B, att_block=256, att_lds=LDS_ATT_SKV)
    return dict(att=ATT_32, remap=remap, att_ablate=abl, B=B, T=T, pitch=pitch, nq=nq, att_grid=nq * 4 * B, att_block=256, att_lds=0)


NO_TILE = dict(qkv_ablate=0, qkv_grid=0, qkv_lds=0)
NO_TAIL = dict(tail_tiles=0, tail_grid=0, tail_lds=0)


def qkv_tile(N, ablate=0):
    return dict(qkv=QKV_TILE, qkv_ablate=ablate, qkv_grid=5 * N, qkv_lds=LDS_QKV_TILE)


def expected(kind, N, dt, offer, enc_tail=1, ln_pmean=1, fuse_pose=1, qkv_ablate=0, att_variant=1):
    """THE TABLE"""
    if kind == HEAD:           # cross-attention over ONE sequence of the N hypotheses; Linear layers around it, Linear(512, 1) in f32
        return dict(qkv=QKV_LINEAR, **NO_TILE, **attention(1, N, N, att_variant), tail=TAIL_NONE, pool=POOL_TOKEN_MEAN, readout=RO_SMALL_LINEAR,
                    fuse=0, **NO_TAIL)
    abl = qkv_ablate if dt == F16 and qkv_ablate in (1, 2, 3, 4, 7) else 0
    if kind == FEATURES:       # rows = 400 N on qkv_tile_kernel from 800 rows on, the token mean, out_proj as a GEMV
        q = qkv_tile(N, abl) if N >= 2 else dict(qkv=QKV_LINEAR, **NO_TILE)
        return dict(**q, **attention(N, 400, 400, att_variant), tail=TAIL_NONE, pool=POOL_TOKEN_MEAN, readout=RO_SMALL_LINEAR, fuse=0, **NO_TAIL)
    fuse = 1 if (N == 1 and offer and fuse_pose) else 0
    if N == 1:                 # Track: both heads grouped at pitch 512
        e = dict(qkv=QKV_GROUPED, **NO_TILE, **attention(2, 400, 512, att_variant), fuse=fuse)
        if enc_tail:
            return dict(**e, tail=TAIL_ONE_1, pool=POOL_TAIL_PDOT, readout=RO_ENC_HEADS, tail_tiles=25, tail_grid=50, tail_lds=LDS_TAIL_1)
        return dict(**e, tail=TAIL_GROUPED_CHAIN, pool=POOL_LN_PMEAN if ln_pmean else POOL_LN_TOKEN_MEAN,
                    readout=RO_SMALL_LINEAR2_POSE if fuse else RO_SMALL_LINEAR2, **NO_TAIL)
    if enc_tail:
        return dict(**qkv_tile(N, abl), **attention(N, 400, 400, att_variant), tail=TAIL_ONE_5, pool=POOL_TAIL_PDOT, readout=RO_ENC_HEADS, fuse=0,
                    tail_tiles=5 * N, tail_grid=10 * N, tail_lds=LDS_TAIL_5)
    return dict(qkv=QKV_LINEAR, **NO_TILE, **attention(N, 400, 400, att_variant), tail=TAIL_HEAD_CHAIN,
                pool=POOL_LN_MEAN if N >= 96 else POOL_LN_TOKEN_MEAN, readout=RO_SMALL_LINEAR, fuse=0, **NO_TAIL)


CASES = [(REFINER, 0), (REFINER, 1), (FEATURES, 0), (HEAD, 0)]


def test_the_product_schedule_at_every_batch(P):
    for dt in (F16, BF16):
        for kind, offer in CASES:
            for N in range(1, N_MAX + 1):
                assert P.plan(kind, N, dt, offer) == expected(kind, N, dt, offer), (kind, N, dt, offer)


def test_the_table_says_what_the_issue_says(P):
    """the table above, spot-checked against plain statements (so that a mistake shared by expected() and plan_heads still shows)"""
    p = lambda kind, N, offer=0: P.plan(kind, N, F16, offer)
    assert p(REFINER, 1)["qkv"] == QKV_GROUPED and all(p(REFINER, N)["qkv"] == QKV_TILE for N in (2, 3, 252, N_MAX))
    assert p(REFINER, 2)["qkv_grid"] == 10 and p(REFINER, 252)["qkv_grid"] == 1260
    assert [p(REFINER, N)["att"] for N in (1, 2, 4, 5, 252)] == [ATT_SKV, ATT_SKV, ATT_SKV, ATT_32, ATT_32]
    t = p(REFINER, 1)
    assert (t["B"], t["T"], t["pitch"], t["att_grid"], t["att_lds"]) == (2, 400, 512, 13 * 4 * 2, 133120)
    assert p(REFINER, 252)["att_grid"] == 4 * 4 * 252 and p(REFINER, 252)["att_lds"] == 0
    assert [p(HEAD, N)["att"] for N in (1, 32, 33, 2048, 2049, N_MAX)] == [ATT_32, ATT_32, ATT_SKV, ATT_SKV, ATT_32, ATT_32]
    assert all((p(HEAD, N)["B"], p(HEAD, N)["T"]) == (1, N) for N in (1, 33, N_MAX))
    assert p(REFINER, 1)["tail"] == TAIL_ONE_1 and all(p(REFINER, N)["tail"] == TAIL_ONE_5 for N in (2, 95, 96, N_MAX))
    assert p(REFINER, 1)["tail_lds"] == 17408 and p(REFINER, 2)["tail_lds"] == 119808 and p(REFINER, 2)["qkv_lds"] == 81920
    assert p(REFINER, 1, 1)["fuse"] == 1 and p(REFINER, 1, 0)["fuse"] == 0 and p(REFINER, 2, 1)["fuse"] == 0
    assert p(FEATURES, 1)["qkv"] == QKV_LINEAR and p(FEATURES, 2)["qkv"] == QKV_TILE and p(FEATURES, 1, 1)["fuse"] == 0


BOUNDARY_N = sorted(set(list(range(1, 8)) + [31, 32, 33, 34, 94, 95, 96, 97, 252, 2047, 2048, 2049, 2050, N_MAX]))


def test_the_switches_act_only_where_the_table_says(P):
    L = P.L
    for et in (0, 1):
        for pm in (0, 1):
            for fu in (0, 1):
                L.fpt_set_enc_tail(et); L.fpt_set_ln_pmean(pm); L.fpt_set_fuse_pose(fu)
                for dt in (F16, BF16):
                    for kind, offer in CASES:
                        for N in (range(1, 300) if et == 0 and pm == 1 and fu == 1 else BOUNDARY_N):
                            assert P.plan(kind, N, dt, offer) == expected(kind, N, dt, offer, et, pm, fu), (et, pm, fu, kind, N, dt, offer)
    P.defaults()
    # the chains: grouped at N = 1, per head above; layernorm_mean from 96 sequences on, layernorm + token_mean below
    L.fpt_set_enc_tail(0)
    assert P.plan(REFINER, 1, F16)["tail"] == TAIL_GROUPED_CHAIN and P.plan(REFINER, 2, F16)["tail"] == TAIL_HEAD_CHAIN
    assert P.plan(REFINER, 95, F16)["pool"] == POOL_LN_TOKEN_MEAN and P.plan(REFINER, 96, F16)["pool"] == POOL_LN_MEAN
    assert P.plan(REFINER, 2, F16)["qkv"] == QKV_LINEAR and P.plan(FEATURES, 2, F16)["qkv"] == QKV_TILE
    assert P.plan(REFINER, 1, F16, 1)["readout"] == RO_SMALL_LINEAR2_POSE and P.plan(REFINER, 1, F16, 0)["readout"] == RO_SMALL_LINEAR2
    P.defaults()
    # ln_pmean and fuse_pose change nothing of the product's one-launch forms except the fused RefinePostProcess of Track
    L.fpt_set_ln_pmean(0); L.fpt_set_fuse_pose(0)
    for N in BOUNDARY_N:
        for kind, offer in CASES:
            want = expected(kind, N, F16, offer)
            want["fuse"] = 0
            assert P.plan(kind, N, F16, offer) == want
    P.defaults()
    # the negative control of tests/test_layers_gpu.py and the timing ablations: qkv_tile_kernel in f16 only
    for a in range(0, 9):
        L.fpt_set_qkv_ablate(a)
        for dt in (F16, BF16):
            for kind, offer in CASES:
                for N in (1, 2, 252):
                    assert P.plan(kind, N, dt, offer) == expected(kind, N, dt, offer, qkv_ablate=a), (a, kind, N, dt)
    P.defaults()
    # the attention variants that remain never take the split-key kernel
    for v in ATT_VARIANTS:
        L.fpt_set_att_variant(v)
        for kind, offer in CASES:
            for N in BOUNDARY_N:
                got = P.plan(kind, N, F16, offer)
                assert got == expected(kind, N, F16, offer, att_variant=v), (v, kind, N)
                assert v == 1 or got["att"] == ATT_32


def test_retired_values_are_ignored(P):
    """STATED: a retired value is IGNORED, not refused -- the setter accepts it and the plan is the product's.  att_variant 2 / 3 / 5 / 7
    (the round-1 kernel), 9 (8 waves) and 10 (the lazy maximum) give the shipped attention; fuse_pose 2 (the token mean inside the read-out
    launch) acts as 1."""
    L = P.L
    for v in RETIRED_ATT_VARIANTS + (0, 4, 6, 11, 21, 32, -1):
        L.fpt_set_att_variant(v)
        for kind, offer in CASES:
            for N in BOUNDARY_N:
                assert P.plan(kind, N, F16, offer) == expected(kind, N, F16, offer), (v, kind, N)
    P.defaults()
    L.fpt_set_fuse_pose(2)
    for et, pm in ((1, 1), (0, 1), (0, 0)):
        L.fpt_set_enc_tail(et); L.fpt_set_ln_pmean(pm)
        for offer in (0, 1):
            for N in (1, 2):
                assert P.plan(REFINER, N, F16, offer) == expected(REFINER, N, F16, offer, et, pm, 1)
    assert not hasattr(L, "fpt_set_qkv_tile")


def test_queries_outside_the_domain_are_refused(P):
    f, t = P.f.ctypes.data, P.t.ctypes.data
    assert P.L.fpt_plan_heads(REFINER, 0, F16, 0, f, t) == 1
    assert P.L.fpt_plan_heads(REFINER, N_MAX + 1, F16, 0, f, t) == 1 and P.L.fpt_plan_heads(FEATURES, N_MAX + 1, F16, 0, f, t) == 1
    assert P.L.fpt_plan_heads(REFINER, 1, FP8, 0, f, t) == 1          # the transformer part has no 8-bit form
    assert P.L.fpt_plan_heads(3, 1, F16, 0, f, t) == 1
    assert P.L.fpt_plan_heads(HEAD, 8 * N_MAX, F16, 0, f, t) == 0     # the cross-attention takes the hypotheses of all shards
