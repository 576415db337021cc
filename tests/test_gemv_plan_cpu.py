"""CPU: the planning of the single-vector dual GEMV (make_plan / dual_gemv_scratch_floats / the split column, through
thip_test_gemv_plan, which launches nothing): every plan the autotune may pick, the default plan and the three vector widths keep
the grid covering the matrix exactly once, inside the launch limits and inside the scratch the solver allocates -- in the
one-launch form and in the column-split form of the pipeline, whose two half-launches re-chunk with the full grid target."""
import numpy as np
import pytest

from gemv_plans import BLK, CANDIDATES, MAXCW, plan

README_SHAPES = [(100_000, 50_000), (12_500, 50_000), (20_000, 10_000), (400_000, 25_000)]
HINTS = [(0, 0)] + CANDIDATES


def _shapes():
    rng = np.random.default_rng(20240607)
    # uniform sizes, and log-uniform ones so that small and very unequal shapes are as frequent as large ones
    uni = [(int(a), int(b)) for a, b in rng.integers(1, 70_001, (150, 2))]
    logu = [(int(a), int(b)) for a, b in np.exp(rng.uniform(0.0, np.log(70_000.0), (150, 2))).astype(np.int64).clip(1, 70_000)]
    edges = [(1, 1), (1, 70_000), (70_000, 1), (70_000, 70_000), (4096, 16), (4095, 15), (4097, 17), (65_536, 65_535)]
    return README_SHAPES + edges + uni + logu


def _r4(v):
    return (v + 3) // 4 * 4


def _want_nj_ku(m, vw, nj):
    if vw == 1:                                   # the unaligned fallback ignores the hint: tall tiles from 4096 rows on
        return (4, 4) if m >= BLK * 16 else (1, 8)
    return {0: (1, 8), 1: (1, 8), 2: (2, 4), 4: (4, 2)}[nj]


def test_every_candidate_is_a_hint_the_planner_honours():
    # the nine pairs: the row groups per lane as asked, and a grid of at most the target where neither the least nor the
    # largest chunk width binds (20 000 x 70 000: every candidate lands between 32 and 1024 columns per chunk)
    assert len(CANDIDATES) == 9 and len(set(CANDIDATES)) == 9
    for nj, tb in CANDIDATES:
        p, _, _ = plan(20_000, 70_000, 4, nj, tb)
        assert p["nj"] == nj and 32 < p["cols_per_chunk"] < MAXCW, (nj, tb, p)
        assert tb // 2 < p["tiles"] * p["chunks"] <= tb, (nj, tb, p)


@pytest.mark.parametrize("vw", [4, 8, 1])
def test_every_plan_covers_the_matrix_once_and_fits_the_scratch(vw):
    worst_one, worst_split = 0.0, 0.0
    for m, n in _shapes():
        scr_seen = None
        for nj, tb in HINTS:
            p, scr, split = plan(m, n, vw, nj, tb)
            ctx = (m, n, vw, nj, tb, p)
            assert scr_seen is None or scr == scr_seen, ctx          # the scratch is a function of the shape alone
            scr_seen = scr
            assert p["vw"] == vw and (p["nj"], p["ku"]) == _want_nj_ku(m, vw, nj), ctx
            tile = BLK * vw * p["nj"]
            assert p["tiles"] * tile >= m > (p["tiles"] - 1) * tile, ctx
            cpc = p["cols_per_chunk"]
            assert p["chunks"] * cpc >= n > (p["chunks"] - 1) * cpc, ctx
            assert cpc % 8 == 0 and 8 <= cpc <= MAXCW, ctx
            assert 1 <= p["chunks"] <= 65_535 and p["tiles"] >= 1, ctx
            assert p["m_load"] == (m if vw > 1 and m % vw == 0 else 0), ctx
            need = p["chunks"] * _r4(m) + p["tiles"] * _r4(n)
            assert need <= scr, ctx
            worst_one = max(worst_one, need / scr)
            # the column-split form at the solver's split column: the two ranges are planned on their own columns
            assert split == (0 if n < 16 else (n // 2) // 8 * 8), ctx
            if split == 0:
                continue
            assert split % 8 == 0 and 0 < split < n, ctx
            p1, _, _ = plan(m, n, vw, nj, tb, 0, split)
            p2, _, _ = plan(m, n, vw, nj, tb, split, n)
            for q, cols in ((p1, split), (p2, n - split)):
                assert (q["vw"], q["nj"], q["ku"], q["tiles"], q["m_load"]) == (p["vw"], p["nj"], p["ku"], p["tiles"], p["m_load"]), ctx
                assert q["chunks"] * q["cols_per_chunk"] >= cols > (q["chunks"] - 1) * q["cols_per_chunk"], (ctx, q)
                assert q["cols_per_chunk"] % 8 == 0 and q["cols_per_chunk"] <= MAXCW, (ctx, q)
            need2 = (p1["chunks"] + p2["chunks"]) * _r4(m) + p["tiles"] * _r4(n)
            assert need2 <= 2 * scr, (ctx, p1, p2)                   # what ensure_gemv_scratch allocates
            worst_split = max(worst_split, need2 / (2 * scr))
    print("vw=%d: largest share of the scratch in use: one launch %.3f of S, column split %.3f of 2 S" % (vw, worst_one, worst_split))


def test_bad_arguments_are_refused():
    from totsu_amd import _lib
    for args in ((0, 5, 4, 0, 0, 0, 5), (5, 0, 4, 0, 0, 0, 0), (5, 5, 3, 0, 0, 0, 5), (5, 5, 4, -1, 0, 0, 5), (5, 5, 4, 0, 0, 3, 3),
                 (5, 5, 4, 0, 0, 0, 6)):
        with pytest.raises(_lib.ThipError) as e:
            plan(*args[:5], col0=args[5], col1=args[6])
        assert e.value.code == _lib.E_INVALID
