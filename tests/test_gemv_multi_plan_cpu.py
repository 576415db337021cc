"""CPU: the planning of the multi-vector dual GEMV (multi_plan / dual_gemv_multi_scratch_floats through thip_test_gemv_multi_plan,
which launches nothing) against its restatement in tests/gemv_multi_plans.py and against the properties a launch relies on: for
every kernel instance, the default plan and every plan the autotune may pick, the grid covers the matrix exactly once, stays inside
the launch limits and the LDS limit, and inside the scratch a batch allocates per slot."""
import numpy as np
import pytest

from gemv_multi_plans import (BLK, CANDIDATES, INSTANCES, ITERS, MCW, PAIRS, PIN_SHAPE, TOLS, TUNE_SHAPE, VW, lp_data, plan, restated_plan,
                              restated_scratch)

README_SHAPES = [(20_000, 10_000), (100_000, 50_000), (12_500, 50_000), (400_000, 25_000)]
HINTS = [(0, 0)] + CANDIDATES
SIDE = 300_000
DISTINCT = PIN_SHAPE             # the shape the GPU tests pin every candidate on (tests/test_gpu_gemv_multi_tilings.py)


def _shapes():
    rng = np.random.default_rng(20250311)
    # uniform sizes, and log-uniform ones so that small and very unequal shapes are as frequent as large ones
    uni = [(int(a), int(b)) for a, b in rng.integers(1, SIDE + 1, (150, 2))]
    logu = [(int(a), int(b)) for a, b in np.exp(rng.uniform(0.0, np.log(float(SIDE)), (250, 2))).astype(np.int64).clip(1, SIDE)]
    edges = [(1, 1), (1, SIDE), (SIDE, 1), (SIDE, SIDE)] + [(m, n) for m in (1023, 1024, 1025, 2047, 2048, 2049) for n in (1, 40, 5000)]
    mb64 = [(4000, 3999), (4000, 4000), (4000, 4001)]          # 63.98, 64.0 and 64.02 MB: the least chunk width doubles at 64.0e6 bytes
    return README_SHAPES + edges + mb64 + uni + logu


def _r4(v):
    return (v + 3) // 4 * 4


@pytest.mark.parametrize("instance", INSTANCES)
def test_every_plan_covers_the_matrix_once_and_fits_the_scratch(instance):
    worst = 0.0
    for m, n in _shapes():
        scr_want = restated_scratch(m, n)
        for nj, tb in HINTS:
            p, scr = plan(m, n, instance, nj, tb)
            ctx = (m, n, instance, nj, tb, p)
            assert p == restated_plan(m, n, instance, nj, tb), (ctx, restated_plan(m, n, instance, nj, tb))
            assert scr == scr_want, (ctx, scr, scr_want)              # a function of the shape alone: the same under every hint
            assert p["vw"] == VW and p["nj"] == (2 if nj == 2 and instance < 8 else 1) and p["ku"] == 8 // p["nj"], ctx
            tile = BLK * VW * p["nj"]
            assert p["tiles"] * tile >= m > (p["tiles"] - 1) * tile, ctx
            cpc = p["cols_per_chunk"]
            assert p["chunks"] * cpc >= n > (p["chunks"] - 1) * cpc, ctx
            assert cpc % 8 == 0 and 16 <= cpc <= MCW, ctx
            assert cpc >= 32 or m * n * 4 < 64_000_000, ctx
            assert 1 <= p["chunks"] <= 65_535 and p["tiles"] >= 1, ctx
            assert p["m_load"] == _r4(m), ctx
            need = p["chunks"] * _r4(m) + p["tiles"] * _r4(n)
            assert need <= scr, ctx
            worst = max(worst, need / scr)
    print("NV=%d: largest share of a slot's scratch in use %.3f" % (instance, worst))


def test_both_sides_of_64_mb():
    # with a grid target that would ask for fewer columns, the least chunk width binds: 16 below 64.0e6 bytes, 32 from there on
    assert plan(4000, 3999, 2, 1, 8192)[0]["cols_per_chunk"] == 16
    assert plan(4000, 4000, 2, 1, 8192)[0]["cols_per_chunk"] == 32
    assert plan(4000, 4001, 8, 1, 8192)[0]["cols_per_chunk"] == 32


def test_the_candidates_are_distinct_plans_where_the_gpu_tests_pin_them():
    m, n = DISTINCT
    assert len(CANDIDATES) == 7 and len(set(CANDIDATES)) == 7
    assert len(PAIRS) == 17
    got = [plan(m, n, 4, nj, tb)[0] for nj, tb in CANDIDATES]
    assert [(p["nj"], p["cols_per_chunk"]) for p in got] == [(1, 40), (1, 80), (1, 152), (2, 40), (2, 80), (2, 152), (2, 256)], got
    assert len({(p["nj"], p["cols_per_chunk"], p["chunks"]) for p in got}) == 7
    # NV = 8 takes the hint's grid but never its two row groups
    for nj, tb in CANDIDATES:
        p8, p4 = plan(m, n, 8, nj, tb)[0], plan(m, n, 4, 1, tb)[0]
        assert p8 == p4, (nj, tb, p8, p4)
    # (the default plan there is that of (1, 2048): an untuned batch differs from every other pinned one)
    assert plan(m, n, 4)[0] == got[2]


def test_bad_arguments_are_refused():
    from totsu_amd import _lib
    for args in ((0, 5, 2, 0, 0), (5, 0, 2, 0, 0), (5, 5, 1, 0, 0), (5, 5, 3, 0, 0), (5, 5, 16, 0, 0), (5, 5, 0, 0, 0), (5, 5, 4, -1, 0),
                 (5, 5, 4, 0, -1), (2 ** 31, 5, 4, 0, 0), (5, 2 ** 31, 4, 0, 0)):
        with pytest.raises(_lib.ThipError) as e:
            plan(*args)
        assert e.value.code == _lib.E_INVALID, args
    from totsu_amd._lib import lib
    lib.thip_test_gemv_multi_plan(5, 5, 4, 0, 0, None, None)          # either pointer may be NULL


@pytest.mark.parametrize("shape", [PIN_SHAPE, TUNE_SHAPE])
def test_the_solver_level_shapes_are_fair_to_the_tolerance(shape):
    """the GPU tests hold the batch to the project's tolerances at iterates 0, 1, 9 on these LPs: the f32 reference itself
    (tests/state_numpy.py), against its own f64 run, stays below a quarter of each -- the tolerance is not what decides the test"""
    from state_numpy import CONE_RPOS, criteria_after
    m, n = shape
    a, bs, cs = lp_data(m, n)
    for it, tol in zip(ITERS, TOLS):
        got = [criteria_after(a, bs[0], cs[0], [(CONE_RPOS, m)], it + 1, dtype=dt, iterate=True)[1] for dt in (np.float32, np.float64)]
        x = [np.concatenate([s["xx"], s["xy"], s["xs"], [s["tau"]]]).astype(np.float64) for s in got]
        y = [np.concatenate([s["u"], s["v"], [s["kappa"]]]).astype(np.float64) for s in got]
        ex, ey = (np.abs(v[0] - v[1]).max() / max(np.abs(v[1]).max(), 1e-6) for v in (x, y))
        print("%d x %d iterate %d: f32 reference against f64  x %.1e  y %.1e  (tol %.0e)" % (m, n, it, ex, ey, tol))
        assert ex <= tol / 4 and ey <= tol / 4, (shape, it, ex, ey)
