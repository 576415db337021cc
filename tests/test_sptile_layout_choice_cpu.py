"""CPU: `totsu_amd.sparse.choose_layout` -- the rule that decides between the dense one-pass schedule and the tiled sparse copy for a
dense, mostly-zero A -- and the argument checks of FusedSolver(a_layout=...), which fire before any library call."""
import numpy as np
import pytest
import scipy.sparse as sp


def _rule(n_row, n_col, bytes_per_product):
    # per iteration: dense reads 4 m n bytes once at 0.90 of peak, tiled reads bytes_per_product twice at 0.53 (worst pattern): 1.7
    return "tiled" if 2 * 1.7 * bytes_per_product < 4 * n_row * n_col else "dense"


@pytest.mark.parametrize("shape", [(1000, 1000), (4096, 8192), (123, 45678)])
def test_choose_layout_on_either_side_of_the_rule(shape):
    from totsu_amd.sparse import choose_layout
    m, n = shape
    # an all-indexed store streams 8 bytes per entry: the crossover is at density 4 / (2 * 1.7 * 8) = 0.147; a store of dense tiles
    # alone streams 4: 0.294
    for per_entry, cross in ((8, 4 / (2 * 1.7 * 8)), (4, 4 / (2 * 1.7 * 4))):
        for density in (0.0, 0.001, 0.5 * cross, 0.95 * cross, 1.05 * cross, 2 * cross, 1.0):
            nnz = int(density * m * n)
            assert choose_layout(m, n, per_entry * nnz) == _rule(m, n, per_entry * nnz), (per_entry, density)
        assert choose_layout(m, n, per_entry * int(0.95 * cross * m * n)) == "tiled"
        assert choose_layout(m, n, per_entry * int(1.05 * cross * m * n)) == "dense"
    assert choose_layout(m, n, 0) == "tiled" and choose_layout(m, n, 8 * m * n) == "dense"
    # the same matrix can be worth tiling as dense tiles and not as indexed entries
    nnz = int(0.2 * m * n)
    assert choose_layout(m, n, 4 * nnz) == "tiled" and choose_layout(m, n, 8 * nnz) == "dense"


class _Reached(Exception):
    pass


def test_refused_combinations_fire_before_any_library_call(monkeypatch):
    import totsu_amd as T
    from totsu_amd import _lib
    from totsu_amd.sparse import SpTile

    def reached():
        raise _Reached()
    monkeypatch.setattr(_lib, "ensure_init", reached)
    a = np.zeros(6, np.float32)
    args = (2, 3, a, np.zeros(3, np.float32), np.zeros(2, np.float32), [1], [3])
    for layout in ("tiled", "auto"):
        for kw in ({"a_storage": "bf16"}, {"a_storage": "f16"}, {"col_shard": True}):
            with pytest.raises(AssertionError):
                T.FusedSolver(*args, a_layout=layout, **kw)
        for mat in (sp.csc_matrix((3, 2), dtype=np.float32), sp.csr_matrix(np.eye(3, 2, dtype=np.float32)), SpTile.__new__(SpTile)):
            with pytest.raises(AssertionError):
                T.FusedSolver(2, 3, mat, *args[3:], a_layout=layout)
        # an accepted combination gets as far as the library
        with pytest.raises(_Reached):
            T.FusedSolver(*args, a_layout=layout)
    with pytest.raises(AssertionError):
        T.FusedSolver(*args, a_layout="sparse")
    # the default is today's path: nothing is checked that was not checked before
    with pytest.raises(_Reached):
        T.FusedSolver(*args, a_storage="bf16", col_shard=True)
