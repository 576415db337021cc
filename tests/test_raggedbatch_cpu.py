"""CPU: what the ragged batch decides without a device -- the shape rule (thip_raggedbatch_fits is thip_sdpbatch_fits problem by
problem and names the first problem refused), the launch plan (thip_test_raggedbatch_plan: the class split, the classes' LDS, the
order of the live lists, the layout tables, the packed arena), where from_dense puts the arrays, the Python-side refusals -- and
that conic_batch refuses differing shapes as before."""
import numpy as np
import pytest

from test_midbatch_cpu import _dense
from test_sdpbatch_cpu import REQUIRED, _fits_rc, rule, tri

from totsu_amd import _lib
from totsu_amd import raggedbatch as RB
from totsu_amd import sdpbatch as SP

RPOS, PSD, ZERO, SOC = _lib.CONE_RPOS, _lib.CONE_PSD, _lib.CONE_ZERO, _lib.CONE_SOC


class _Shape:
    """what fits and plan read of a problem"""

    def __init__(self, n, m, seg_type, seg_len):
        self.n, self.m, self.seg_type, self.seg_len = n, m, list(seg_type), list(seg_len)


# taken: the boundary shapes of tests/test_midbatch_cpu.py and tests/test_sdpbatch_cpu.py, on the accepting side
TAKEN = [_Shape(n, m, st, sl) for m, n, st, sl, _ in REQUIRED] + [
    _Shape(1000, 2019, [RPOS], [2019]),                  # exactly 163 840 bytes
    _Shape(1000, 2000, [RPOS], [2000]),
    _Shape(4096, 100, [RPOS], [100]),
    _Shape(1, 2520, [RPOS], [2520]),
    _Shape(1, 1, [RPOS], [1]),
    _Shape(40, 80, [RPOS, ZERO], [80, 0]),
    _Shape(128, 65, [RPOS], [65]),
    _Shape(60, 400, [2, 2, 2, 2, 3, 0], [200, 130, 2, 1, 60, 7]),
    _Shape(836, 1176, [PSD], [1176]),                    # order 48 at its largest n
    _Shape(46, tri(57), [PSD], [tri(57)]),               # the largest order whose vectors fit
    _Shape(5, tri(3) + tri(33) + tri(6), [PSD] * 3, [tri(3), tri(33), tri(6)]),
]
# refused, with a word of the rule's message
REFUSED = [(_Shape(8, 4097, [RPOS], [4097]), "4096"), (_Shape(4097, 8, [RPOS], [8]), "4096"),
           (_Shape(1000, 2020, [RPOS], [2020]), "LDS"), (_Shape(1, 1, [RPOS, RPOS], [1, 1]), "cover"),
           (_Shape(3, 7, [RPOS], [6]), "cover"), (_Shape(0, 4, [RPOS], [4]), "4096"), (_Shape(4, 0, [RPOS], [0]), "4096"),
           (_Shape(3, 6, [7], [6]), "bad cone segment"), (_Shape(3, 6, [RPOS], [-6]), "bad cone segment"),
           (_Shape(3, 7, [PSD], [7]), "triangular"), (_Shape(3, 4, [RPOS, PSD], [4, 0]), "triangular"),
           (_Shape(3, 2145, [PSD], [2145]), "above 64"), (_Shape(837, 1176, [PSD], [1176]), "LDS"),
           (_Shape(47, tri(57), [PSD], [tri(57)]), "LDS"), (_Shape(1, tri(60), [PSD], [tri(60)]), "LDS"),
           (_Shape(3, 6, [PSD], [3]), "cover"), (_Shape(3, 6, [], []), "cover")]


def test_fits_is_the_sdp_batch_s_rule_problem_by_problem():
    got = RB.fits(TAKEN)
    assert len(got) == len(TAKEN)
    for d, (lds, thr) in zip(TAKEN, got):
        rc, want_lds, want_thr, _ = _fits_rc(d.n, d.m, d.seg_type, d.seg_len)
        assert rc == 0 and (lds, thr) == (want_lds, want_thr) == SP.fits(d.n, d.m, d.seg_type, d.seg_len), (d.n, d.m)
        assert thr == (256 if d.n * d.m <= 8192 else 1024)
    assert got[0][0] == rule(6, 45, 9)


@pytest.mark.parametrize("k", range(len(REFUSED)))
def test_fits_reports_the_first_refused_index_in_the_rule_s_words(k):
    bad, word = REFUSED[k]
    rc, _, _, msg = _fits_rc(bad.n, bad.m, bad.seg_type, bad.seg_len)
    assert rc == _lib.E_INVALID and word in msg
    core = msg.split(": ", 1)[1].split(" -> ")[0]        # the rule's words, without the place and the code
    for at in (0, 3, len(TAKEN)):
        with pytest.raises(ValueError) as e:
            RB.fits(TAKEN[:at] + [bad] + TAKEN[at:] + [REFUSED[(k + 1) % len(REFUSED)][0]])
        assert e.value.problem == at
        assert "problem %d:" % at in str(e.value) and core in str(e.value), (str(e.value), core)


def test_fits_refuses_no_problem_and_bad_lists():
    with pytest.raises(ValueError, match="1 .. 1048576"):
        RB.fits([])
    with pytest.raises(ValueError, match="problem 1"):
        RB.fits([TAKEN[0], _Shape(3, 6, [PSD, RPOS], [6])])
    with pytest.raises(ValueError, match="problem 0"):
        RB.fits([_Shape(-3, 6, [PSD], [6])])
    with pytest.raises(ValueError, match="256 or 1024"):
        RB.plan(TAKEN, force_threads=64)


def test_class_split_follows_the_thread_rule():
    """both sides of m n = 8192, and the classes' LDS: the largest map of the members"""
    ds = [_Shape(64, 128, [RPOS], [128]),                # 8192: 256 threads
          _Shape(2731, 3, [RPOS], [3]),                  # 8193 = 3 x 2731: 1024 (2731 rows would not fit LDS; 3 rows do)
          _Shape(1, 1, [RPOS], [1]), _Shape(4096, 2, [RPOS], [2]), _Shape(4096, 3, [RPOS], [3]), _Shape(6, 45, [PSD], [45]),
          _Shape(5, tri(40), [PSD], [tri(40)]),          # 4100 entries, 256 threads, with the operand tail
          _Shape(1000, 2000, [RPOS], [2000])]
    pl = RB.plan(ds)
    per = RB.fits(ds)
    assert pl["cls"] == [0, 1, 0, 0, 1, 0, 0, 1] == [int(t == 1024) for _, t in per]
    info = pl["info"]
    assert info["n_prob"] == 8 and [c["n_prob"] for c in info["classes"]] == [5, 3]
    assert [c["threads"] for c in info["classes"]] == [256, 1024]
    for c in (0, 1):
        assert info["classes"][c]["lds_bytes"] == max(l for (l, _), k in zip(per, pl["cls"]) if k == c)
    assert info["classes"][0]["lds_bytes"] == rule(4096, 2, 0) > rule(5, tri(40), 40) > rule(64, 128, 0)
    assert info["classes"][1]["lds_bytes"] == rule(1000, 2000, 0) == 162832
    assert info["a_bytes_per_iter"] == sum(8 * d.n * d.m for d in ds)
    # a forced size puts every problem in one class, with the largest map of all
    for force, c in ((256, 0), (1024, 1)):
        f = RB.plan(ds, force_threads=force)
        assert f["cls"] == [c] * 8 and f["info"]["classes"][c]["n_prob"] == 8 and f["info"]["classes"][1 - c]["n_prob"] == 0
        assert f["info"]["classes"][c]["lds_bytes"] == max(l for l, _ in per) and f["info"]["classes"][1 - c]["lds_bytes"] == 0
        assert sorted(f["order"][c]) == list(range(8)) and f["order"][1 - c] == []


def test_live_order_is_descending_size_with_ties_by_index():
    shapes = [(4, 10), (8, 5), (2, 3), (40, 1), (5, 8), (100, 100), (1, 1), (2000, 1000), (100, 100), (10, 4), (90, 100)]
    ds = [_Shape(n, m, [RPOS], [m]) for m, n in shapes]
    pl = RB.plan(ds)
    for c in (0, 1):
        mine = [p for p in range(len(ds)) if pl["cls"][p] == c]
        assert pl["order"][c] == sorted(mine, key=lambda p: (-ds[p].m * ds[p].n, p))
    assert pl["order"][0] == [0, 1, 3, 4, 9, 2, 6] and pl["order"][1] == [7, 5, 8, 10]


def test_layouts_are_deduplicated_on_m_and_segments():
    ds = [_Shape(6, 45, [PSD], [45]), _Shape(9, 45, [PSD], [45]),           # another n: the same table
          _Shape(6, 45, [RPOS], [45]), _Shape(6, 45, [RPOS, RPOS], [40, 5]),  # the same class bytes, other segments: not merged
          _Shape(6, 45, [PSD], [45]), _Shape(6, 46, [PSD, ZERO], [45, 1]), _Shape(6, 45, [SOC], [45]), _Shape(6, 45, [RPOS], [45]),
          _Shape(6, 45, [RPOS, ZERO], [45, 0])]
    pl = RB.plan(ds)
    assert pl["layout"] == [0, 0, 1, 2, 0, 3, 4, 1, 5] and pl["info"]["n_layouts"] == 6
    assert pl["info"]["n_layouts"] == len({(d.m, tuple(d.seg_type), tuple(d.seg_len)) for d in ds})
    same = RB.plan([ds[0]] * 7)
    assert same["info"]["n_layouts"] == 1 and same["layout"] == [0] * 7


def test_the_arena_is_packed():
    ds = TAKEN
    pl = RB.plan(ds)
    strides = [6 * d.n + 10 * d.m for d in ds]
    assert pl["arena_at"] == [int(v) for v in np.cumsum([0] + strides[:-1])]
    assert pl["info"]["arena_bytes"] == 4 * sum(strides)


def _mix():
    return [_dense(20, 40, [RPOS], [40], seed=1), _dense(7, 13, [RPOS, ZERO], [12, 1], rowabs=True, seed=2),
            _dense(6, 45, [PSD], [45], seed=3), _dense(3, 102, [SOC, RPOS], [100, 2], rowabs=True, seed=4),
            _dense(1, 1, [RPOS], [1], seed=5), _dense(5, 9, [RPOS], [9], seed=6)]


def test_from_dense_packs_every_array_at_a_multiple_of_4_floats():
    ds = _mix()
    packed = RB.pack(ds)
    for kind in ("mat_a", "vec_b", "vec_c", "vec_b_rowabs"):
        buf, at = packed[kind]
        end = 0
        for d, a in zip(ds, at):
            v = getattr(d, kind)
            if v is None:
                assert kind == "vec_b_rowabs" and a == -1
                continue
            v = np.asarray(v, np.float32).ravel()
            assert a % 4 == 0 and a >= end, (kind, a, end)                 # aligned, and no two overlap
            assert np.array_equal(buf[a:a + v.size], v)
            end = a + v.size
        assert buf.size >= end
    assert packed["vec_b_rowabs"][1] == [-1, 0, -1, 16, -1, -1]            # a mix with and without row sums
    assert packed["mat_a"][1][:3] == [0, 800, 800 + 92]


class _Stop(Exception):
    pass


def test_constructor_refusals_come_before_the_device(monkeypatch):
    """the shape rule and the array lengths are checked before thip_init is needed; a mix that passes reaches the device"""
    S = RB.RaggedBatchSolver

    def stop():
        raise _Stop()
    monkeypatch.setattr(_lib, "ensure_init", stop)
    with pytest.raises(_Stop):
        S.from_dense(_mix())
    with pytest.raises(ValueError, match="1 .. 1048576 problems, not 0"):
        S([])
    for kind, cut in (("mat_a", 1), ("vec_b", 1), ("vec_c", 1), ("vec_b_rowabs", 2)):
        ds = _mix()
        setattr(ds[3], kind, np.asarray(getattr(ds[3], kind))[:-cut])
        with pytest.raises(ValueError, match="problem 3: %s" % kind):
            S.from_dense(ds)
    ds = _mix()
    ds[2].vec_c = None
    with pytest.raises(ValueError, match="problem 2: vec_c is needed"):
        S(ds)
    for bad, word in REFUSED[:4] + REFUSED[9:12]:
        z = np.zeros(max(bad.n * bad.m, 0), np.float32)
        d = _dense(1, 1, [RPOS], [1])
        d.n, d.m, d.seg_type, d.seg_len = bad.n, bad.m, bad.seg_type, bad.seg_len
        d.mat_a, d.vec_b, d.vec_c = z, z[:bad.m], z[:bad.n]
        with pytest.raises(ValueError, match="problem 4"):
            S(_mix()[:4] + [d])
    import totsu_amd
    assert totsu_amd.ragged_batch is RB.ragged_batch and totsu_amd.RaggedBatchSolver is S


def test_conic_batch_still_refuses_differing_shapes():
    a, b = _dense(6, 45, [PSD], [45]), _dense(6, 45, [RPOS], [45])
    with pytest.raises(ValueError, match="problem 1 has another cone layout than problem 0"):
        SP.conic_batch([a, b])
    with pytest.raises(ValueError, match="problem 1 is 46 x 6 where problem 0 is 45 x 6"):
        SP.conic_batch([a, _dense(6, 46, [PSD, ZERO], [45, 1])])
    with pytest.raises(ValueError, match="differ in whether they carry vec_b_rowabs"):
        SP.conic_batch([b, _dense(6, 45, [RPOS], [45], rowabs=True)])
    RB.fits([a, b, _dense(6, 46, [PSD, ZERO], [45, 1])])                    # ... which the ragged batch takes
