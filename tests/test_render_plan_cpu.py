"""The render + crop schedule of fp_geometry.hip (plan_render) asked on the host, no GPU: fpt_plan_render returns what one
render_and_crop call would launch.  Over every batch 1..FP_MAX_BATCH, the three output modes, debug taps on / off, the profiler on / off,
both outputs / the rendered one alone / the observed one alone, meshes of 0, 1, 1280 and 20480 triangles and a row-range buffer that
just holds N * F entries / is one entry short, the plan must be the table of DESIGN.md section 4.1 and a sound one:
  * strip rows and threads by batch size, on both sides of 2 | 3, 25 | 26, 47 | 48 and 99 | 100; 256 threads whenever the mode is f32 or taps
    are attached;
  * strip rows divide the 160 rows of a crop;
  * lds = rows * 160 * 8 (+ 8192 * 4 + 16 with row ranges), at most 64 KB unless the plan asks for the opt-in, never above the 160 KB of a CU;
  * row ranges only for N <= 99, N * F <= capacity and F > 0; written by the front launch only when that is the fused one;
  * the fused front only for N <= 4 (4 | 5), both outputs, a 2-byte mode, no taps, profiler off;
  * crop_kernel is its own launch exactly when an observed output is wanted and the front is not the fused one;
  * each A/B switch the test build keeps changes the plan only in what it names."""
import ctypes as C
import itertools

import numpy as np
import pytest

from foundationpose_cpp_amd import _lib

N_MAX = 2377                                      # include/foundationpose_amd.h FP_MAX_BATCH
F32X6, F16X8, BF16X8 = range(3)                   # fp_internal.h OutMode
FRONT_SETUP, FRONT_SETUP_VERTEX, FRONT_FUSED = range(3)    # RenderFront
ROWS_NONE, ROWS_BY_FRONT, ROWS_OWN_LAUNCH = range(3)       # RowRanges
CROP, TRI_LIST_LDS = 160, 8192 * 4 + 16
Q_N, Q_MODE, Q_OUT_A, Q_OUT_B, Q_TAPS, Q_PROF, Q_F, Q_CAP = range(8)
P_FRONT, P_ROW_RANGES, P_ROWS, P_THREADS, P_LDS, P_OPTIN, P_CROP = range(7)


def _queries():
    rest = list(itertools.product((F32X6, F16X8, BF16X8), ((1, 1), (1, 0), (0, 1)), (0, 1), (0, 1), (0, 1, 1280, 20480), (0, 1)))
    q = np.zeros((N_MAX, len(rest), 8), np.int64)
    q[:, :, Q_N] = np.arange(1, N_MAX + 1)[:, None]
    for j, (mode, (out_a, out_b), taps, prof, F, short) in enumerate(rest):
        q[:, j, Q_MODE], q[:, j, Q_OUT_A], q[:, j, Q_OUT_B], q[:, j, Q_TAPS], q[:, j, Q_PROF], q[:, j, Q_F] = mode, out_a, out_b, taps, prof, F
        q[:, j, Q_CAP] = np.maximum(q[:, j, Q_N] * F - short, 0)          # holds N * F entries exactly / is one entry short
    return q.reshape(-1, 8)


@pytest.fixture(scope="module")
def planner():
    L = _lib.test_lib()
    L.fpt_plan_render.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong]
    L.fpt_plan_render.restype = None
    q = _queries()

    def plan():
        p = np.full((len(q), 7), -1, np.int32)
        L.fpt_plan_render(q.ctypes.data, p.ctypes.data, len(q))
        return p
    return L, q, plan


def _columns(a):
    return [a[:, i] for i in range(a.shape[1])]


def test_every_plan_is_the_table_and_sound(planner):
    _, q, plan = planner
    assert len(q) > 600000
    N, mode, out_a, out_b, taps, prof, F, cap = _columns(q)
    front, ranges, rows, threads, lds, optin, crop = _columns(plan())
    product = (mode != F32X6) & (taps == 0)        # the 2-byte network tensor without taps: the only path with wide workgroups
    # the table (issue / DESIGN.md section 4.1), written out per row
    exp_rows = np.where(product, np.select([N <= 2, N <= 47, N <= 99], [4, 8, 20], 80), np.where(N <= 47, 8, 20))
    exp_threads = np.where(product, np.select([N <= 25, N <= 47, N <= 99], [1024, 512, 256], 1024), 256)
    assert np.array_equal(rows, exp_rows) and np.array_equal(threads, exp_threads)
    for n, r, t in ((1, 4, 1024), (2, 4, 1024), (3, 8, 1024), (25, 8, 1024), (26, 8, 512), (47, 8, 512), (48, 20, 256), (99, 20, 256),
                    (100, 80, 1024), (252, 80, 1024), (N_MAX, 80, 1024)):
        sel = product & (N == n)
        assert sel.any() and (rows[sel] == r).all() and (threads[sel] == t).all(), (n, r, t)
    for n, r in ((1, 8), (47, 8), (48, 20), (99, 20), (100, 20), (N_MAX, 20)):
        sel = ~product & (N == n)
        assert sel.any() and (rows[sel] == r).all() and (threads[sel] == 256).all(), (n, r)
    assert (threads[(mode == F32X6) | (taps == 1)] == 256).all()
    assert np.isin(rows, (4, 8, 20, 80)).all() and (CROP % rows == 0).all()
    assert np.isin(threads, (256, 512, 1024)).all()
    # row ranges
    exp_ranges = (out_a == 1) & (N <= 99) & (F > 0) & (N * F <= cap)
    assert np.array_equal(ranges != ROWS_NONE, exp_ranges)
    assert (ranges[N >= 100] == ROWS_NONE).all() and (ranges[(N == 99) & exp_ranges] != ROWS_NONE).all()
    assert ((N * F <= cap) & (F > 0))[ranges != ROWS_NONE].all()
    # LDS
    assert np.array_equal(lds, rows * CROP * 8 + np.where(ranges != ROWS_NONE, TRI_LIST_LDS, 0))
    assert (lds[optin == 0] <= 64 * 1024).all() and (lds <= 160 * 1024).all()
    assert np.array_equal(optin == 1, rows == 80)  # (the instantiation, whichever way a launch uses it: 80 x 160 x 8 = 100 KB of z-buffer alone)
    # front, and who writes the row ranges
    exp_fused = (N <= 4) & (out_a == 1) & (out_b == 1) & product & (prof == 0)
    assert np.array_equal(front, np.where(out_a == 0, FRONT_SETUP, np.where(exp_fused, FRONT_FUSED, FRONT_SETUP_VERTEX)))
    assert (front[(N == 4) & exp_fused] == FRONT_FUSED).all() and (front[N == 5] != FRONT_FUSED).all()
    assert np.array_equal(ranges == ROWS_BY_FRONT, exp_ranges & (front == FRONT_FUSED))
    assert (front[ranges == ROWS_BY_FRONT] == FRONT_FUSED).all()
    # crop
    assert np.array_equal(crop == 1, (out_b == 1) & (front != FRONT_FUSED))


def _with(L, setter, value, default, plan):
    getattr(L, setter)(value)
    try:
        return plan()
    finally:
        getattr(L, setter)(default)


def _same_except(a, b, fields):
    keep = [i for i in range(7) if i not in fields]
    return np.array_equal(a[:, keep], b[:, keep])


def test_each_kept_switch_changes_only_what_it_names(planner):
    L, q, plan = planner
    N, mode, out_a, out_b, taps, prof, F, cap = _columns(q)
    base = plan()
    product = (mode != F32X6) & (taps == 0)
    # fpt_set_tri_rows(0): no row ranges (and with them no triangle list in LDS); nothing else
    p = _with(L, "fpt_set_tri_rows", 0, 1, plan)
    assert (p[:, P_ROW_RANGES] == ROWS_NONE).all() and np.array_equal(p[:, P_LDS], p[:, P_ROWS] * CROP * 8)
    assert _same_except(p, base, (P_ROW_RANGES, P_LDS))
    # fpt_set_raster_strip_threads: the threads of the product path's 8-row strips; nothing else, nowhere else
    wide8 = product & (base[:, P_ROWS] == 8)
    assert wide8.any()
    for t in (256, 512, 1024):
        p = _with(L, "fpt_set_raster_strip_threads", t, 0, plan)
        assert _same_except(p, base, (P_THREADS,))
        assert (p[wide8, P_THREADS] == t).all() and np.array_equal(p[~wide8, P_THREADS], base[~wide8, P_THREADS])
    # fpt_set_vertex_crop(2): the fused front stays, the row ranges become their own launch; nothing else
    p = _with(L, "fpt_set_vertex_crop", 2, 1, plan)
    assert _same_except(p, base, (P_ROW_RANGES,))
    assert np.array_equal(p[:, P_ROW_RANGES], np.where(base[:, P_ROW_RANGES] == ROWS_BY_FRONT, ROWS_OWN_LAUNCH, base[:, P_ROW_RANGES]))
    # fpt_set_vertex_crop(0): the fusion is undone -- vertex stage, row ranges and crop warp as their own launches; which row ranges
    # exist and the rasteriser's shape stay
    p = _with(L, "fpt_set_vertex_crop", 0, 1, plan)
    assert _same_except(p, base, (P_FRONT, P_ROW_RANGES, P_CROP))
    fused = base[:, P_FRONT] == FRONT_FUSED
    assert fused.any() and (p[fused, P_FRONT] == FRONT_SETUP_VERTEX).all() and np.array_equal(p[~fused, P_FRONT], base[~fused, P_FRONT])
    assert np.array_equal(p[:, P_ROW_RANGES], np.where(base[:, P_ROW_RANGES] == ROWS_BY_FRONT, ROWS_OWN_LAUNCH, base[:, P_ROW_RANGES]))
    assert np.array_equal(p[:, P_CROP], out_b)
    assert np.array_equal(plan(), base)            # the switches are back at the product's values
