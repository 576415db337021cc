"""Every instance of the one-pass kernel (sweep_k, thip_sweep_kernel.h) the plan autotune can pick, PINNED -- which of them a solve
runs is decided by timings on the box, so a test that leaves the choice to the library checks a different kernel from day to day.

The kernel alone (thip_test_sweep with pin_w / pin_g): every (element kind, columns per panel, slots per thread) of the dispatch
tables (sweep_plans.INSTANCES), each with a member's rows on the edges of its last slot; for 16-bit storage every body of the row
deal (stream(NSLOT) .. stream(0), selected per wave by the slots that hold rows) and both ends of f16's balance window; every group
size with a short last member and with members without rows; a group's columns on the seams of the fill / steady / drain loops; the
flags.  Each case runs both helpers of test_gpu_sweep.py: numpy f64 on the stored matrix (5e-6 of the largest entry; 2e-5 on the sums
over n) and the bit-for-bit Fast2Sum check on exact data -- and asserts from host_info that the pinned geometry is the one that ran.
Shapes are a member's rows x about 100 columns: the pin goes below the planner's few-columns rule, whose groups without columns idle.
(Planner-reachable geometries without a pin: test_gpu_sweep.py test_sweep_kernel_vs_numpy and ..._two_columns_per_panel for f32,
test_gpu_bf16.py test_sweep_kernel_on_a_16_bit_matrix_vs_numpy for one, two and four columns of 16-bit entries.)

The solver: each candidate geometry of sweep_candidates pinned by index (thip_test_solver_pin_sweep_plan) on the smallest LPs that
offer six f32 candidates (sweep_plans.six_candidate_shapes), iterates 0, 1, 2, 9 and the criteria against the f64 oracle, two pinned
solvers bit for bit, the library's own choice, a SOCP with block cones under a two-column and a larger-group candidate.

THIP_SWEEP_INSTANCE_TABLE=<file>: the kernel-alone cases append what ran (from host_info) to that file, one line each; NOTEBOOK.md's
table of instance against cases is made from it."""
import json
import os
import time

import numpy as np
import pytest

import oracle as O
import sweep_plans as P
from sweep_plans import BF16, EPV, F16, F32, INSTANCES, KIND, LAGT, MAX_SLOTS, SLOT
from test_gpu_sweep import _check_sweep_iterates, _exact_sweep_case, _socp, _sweep_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def T():
    import totsu_amd
    from totsu_amd import _lib
    _lib.init()
    return totsu_amd


SIXTEEN = (BF16, F16)


def _run(T, label, elem, w, G, m, n, flags=((0, 1),), lda=None, exact=True):
    """both helpers on one pinned geometry; the geometry that ran must be the pinned one with the slots the rows need"""
    t0 = time.time()
    g = P.plan(m, n, elem, w, members=G, lda=lda)
    assert g is not None, (label, elem, w, G, m, n)
    for first, comp in flags:
        info = _sweep_case(m, n, first, comp, seed=m + 3 * n + 7 * w + elem + first + 2 * comp, lda=lda, elem=elem, pin=(w, G))
        assert (info[1], info[2], info[3], info[4], info[7]) == (G, 256 // G, g["npan"], g["nslot"], w), (label, list(info), g)
    if exact:
        assert _exact_sweep_case(T, m, n, elem, pin=(w, G)) == (G, 256 // G, g["nslot"]), label
    path = os.environ.get("THIP_SWEEP_INSTANCE_TABLE")
    if path:
        rpm = g["rows_per_member"]
        # 16-bit: the bodies the members' waves select, and whether the shortest member with rows (the only one, or the last) deals
        # balanced, by the restatement of the row deal
        bodies, bal = set(), None
        for r in sorted({max(0, min(m, (k + 1) * rpm) - k * rpm) for k in range(G)}, reverse=True) if elem else []:
            b, sl = P.wave_slots_16(elem, g["nslot"], r)
            bodies |= set(sl)
            bal = b if r > 0 else bal
        with open(path, "a") as f:
            f.write(json.dumps(dict(label=label, elem=KIND[elem], w=info[7], nslot=info[4], G=info[1], npan=info[3], m=m, n=n,
                                    bodies=sorted(bodies), bal=bal, sec=round(time.time() - t0, 2))) + "\n")
    return g


def _ids(cases):
    return ["%s-w%d-s%d-%s" % (KIND[c[0]], c[1], c[2], c[3]) for c in cases]


# ---- every instance, a one-member group's rows on the edges of the last slot ------------------------------------------------------

EDGE = [(e, w, ns, "r%d" % r, r) for e in P.ELEMS for w, ns in INSTANCES[e] for r in P.slot_edges(e, ns)]


@pytest.mark.parametrize("elem,w,ns,tag,r", EDGE, ids=_ids(EDGE))
def test_every_instance_on_the_edges_of_its_last_slot(T, elem, w, ns, tag, r):
    """last slot exactly full, one lane in it, one lane short of full (one slot: a single lane of rows)"""
    g = _run(T, "edge " + tag, elem, w, 1, r, 40 * w * 2 + w + 1)
    assert g["nslot"] == ns


# ---- 16-bit: every body of the row deal, both ends of the balance window ----------------------------------------------------------

DEAL = [(e, w, ns, tag, r) for e in SIXTEEN for w, ns in INSTANCES[e] for tag, r in P.wave3_rows(e, ns).items()
        if r != ns * SLOT[e]]                                   # (wave 3 full: the full last slot above)


@pytest.mark.parametrize("elem,w,ns,tag,r", DEAL, ids=_ids(DEAL))
def test_16_bit_row_deal_leaves_wave_3_each_number_of_slots(T, elem, w, ns, tag, r):
    """the last wave of the deal holds NSLOT - 1 .. 0 whole slots, or a partly filled one (f16 deals some of these balanced:
    sweep_plans.wave_slots_16 has what each wave then holds; tests/test_sweep_plan_cpu.py checks that every body is reached)"""
    g = _run(T, "deal " + tag, elem, w, 1, r, 40 * w + 3 * w + 1)
    assert g["nslot"] == ns


BAL = [(e, w, ns, tag, r) for e in SIXTEEN for w, ns in INSTANCES[e] if ns > 1 for tag, r in P.bal_rows(ns).items()]


@pytest.mark.parametrize("elem,w,ns,tag,r", BAL, ids=_ids(BAL))
def test_f16_balance_window_ends(T, elem, w, ns, tag, r):
    """rem one lane-slot outside and on both ends of [0, 64 NSLOT]; the same rows for bf16, which never balances"""
    g = _run(T, "bal " + tag, elem, w, 1, r, 40 * w + 3 * w + 1)
    assert g["nslot"] == ns and P.wave_slots_16(elem, ns, r)[0] == (elem == F16 and 0 <= int(tag[4:]) <= 64 * ns)


BAL_LAST = [(e, 1, 4, tag.replace(" ", "-"), G, m) for e in SIXTEEN for tag, (G, m) in P.bal_rows_last_member().items()]


@pytest.mark.parametrize("elem,w,ns,tag,G,m", BAL_LAST, ids=_ids(BAL_LAST))
def test_four_slot_window_lower_end_in_a_short_last_member(T, elem, w, ns, tag, G, m):
    """four slots: rem <= 0 is what three slots hold, so only a short LAST member of a four-slot group gets there -- wave 3 of it
    is left without rows (stream(0)), balanced (f16, rem = 0) and plain"""
    g = _run(T, "bal " + tag, elem, w, G, m, 40 * w + 3 * w + 1)
    assert g["nslot"] == ns


# ---- group sizes --------------------------------------------------------------------------------------------------------------------

def _group_cases():
    out = []
    k = 0
    for cls, w in ((F32, 1), (F32, 2), (BF16, 1), (BF16, 2), (BF16, 4)):
        for ns in (1, MAX_SLOTS[cls, w]):
            for G in (2, 4, 8, 16, 32):
                elem = cls if cls == F32 else SIXTEEN[k % 2]       # the 16-bit families: bf16 and f16 in turn
                k += 1
                e, S = EPV[elem], SLOT[elem]
                # every member but the last: ns slots, the last of them 40 lanes short; the last member one lane shorter
                rpm = ns * S - 40 * e
                out.append((elem, w, ns, "G%d" % G, G, G * rpm - e))
    for elem in P.ELEMS:
        out.append((elem, 1, 1, "G32-m100", 32, 100 if elem == F32 else 104))       # 25 / 13 members with one lane, the others without rows
    return out


GROUPS = _group_cases()


@pytest.mark.parametrize("elem,w,ns,tag,G,m", GROUPS, ids=_ids(GROUPS))
def test_every_group_size_with_a_short_last_member(T, elem, w, ns, tag, G, m):
    """2 .. 32 members per group at one slot and at the family's most, m not a multiple of G x the rows per lane; 256 / G groups of
    which two have columns (one member per group: the edge cases above)"""
    assert m % (G * EPV[elem]) != 0
    g = _run(T, "group " + tag, elem, w, G, m, 40 * w + 2 * w + 1)
    assert g["nslot"] == ns and G * g["rows_per_member"] > m


# ---- columns: the seams of the fill / steady / drain loops --------------------------------------------------------------------------

def _column_cases():
    out = []
    k = 0
    for cls, w in ((F32, 1), (F32, 2), (BF16, 1), (BF16, 2), (BF16, 4)):
        tail = [("min", 8, 40 * w)] + [("last%d" % c, 8, 2 * 40 * w + c) for c in (1, w, w + 1, LAGT * w - 1)]
        # eight groups of 41 and 42 panels (40: every case above), the last one with a partial last panel
        tail += [("npan41", 32, 8 * 41 * w - 3), ("npan42", 32, 8 * 42 * w - 1)]
        for tag, G, n in tail:
            elem = cls if cls == F32 else SIXTEEN[k % 2]
            k += 1
            out.append((elem, w, 1 if G == 32 else 2, tag, G, n))
    return out


COLUMNS = _column_cases()


@pytest.mark.parametrize("elem,w,ns,tag,G,n", COLUMNS, ids=_ids(COLUMNS))
def test_columns_on_the_seams_of_the_panel_loops(T, elem, w, ns, tag, G, n):
    """the fewest columns; a last active group of 1, W, W + 1 and LAGT W - 1 columns (fewer panels than the loads run ahead, a
    last panel with fewer than W real columns: the min(j, jmax) clamp) behind two full groups of 40 panels; 41 and 42 panels per
    group (40, 41, 42 = 1, 2, 0 mod the 3 register stages)"""
    e = EPV[elem]
    m = G * ((ns - 1) * SLOT[elem] + 37 * e) - e
    g = _run(T, "cols " + tag, elem, w, G, m, n)
    want = {"min": 40, "npan41": 41, "npan42": 42}.get(tag, 40)
    assert (g["nslot"], g["npan"]) == (ns, want), g
    if tag.startswith("npan"):
        assert w == 1 or n % w != 0


# ---- flags, leading dimension -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("elem", P.ELEMS, ids=[KIND[e] for e in P.ELEMS])
def test_flags_and_padded_leading_dimension(T, elem):
    """first = 0 / 1 x with and without the Kahan pointers, at lda = m and at lda > m (the rows behind m hold non-zero entries)"""
    e, w = EPV[elem], 2
    m, n = 2 * (SLOT[elem] + 21 * e) - e, 40 * w * 2 + 3
    flags = ((0, 0), (0, 1), (1, 0), (1, 1))
    _run(T, "flags", elem, w, 2, m, n, flags=flags)
    _run(T, "lda", elem, w, 2, m, n, flags=flags, lda=m + 5 * e, exact=False)


def test_pins_the_kernel_cannot_run_launch_nothing(T):
    """THIP_E_INVALID from thip_test_sweep itself (the planning's refusals: tests/test_sweep_plan_cpu.py)"""
    from totsu_amd import _lib
    for elem, w, G, m, n in ((F32, 1, 1, 7 * 1792 + 4, 100), (F32, 2, 1, 3 * 1792 + 4, 100), (F32, 4, 1, 1792, 200), (F32, 1, 3, 1792, 100),
                             (F32, 1, 64, 1792, 100), (F32, 2, 2, 1792, 79), (F32, 1, 1, 1790, 100), (BF16, 2, 1, 4 * 3584, 100),
                             (BF16, 4, 1, 3584, 159), (F16, 1, 2, 3580, 100)):
        with pytest.raises(_lib.ThipError) as err:
            _sweep_case(m, n, 1, 0, seed=1, elem=elem, pin=(w, G))
        assert err.value.code == _lib.E_INVALID, (elem, w, G, m, n)
    _run(T, "after refusals", F32, 1, 1, 1792, 100)


# ---- the solver under each pinned candidate ---------------------------------------------------------------------------------------

ITERS, TOLS = [0, 1, 2, 9], [2e-5, 2e-5, 2e-5, 1e-4]          # test_sweep_iterates_lp / _socp and test_gpu_bf16.py, to iterate 9


class _Lp:
    """an inequality-form LP of m rows and n columns (A x <= b: one non-negative cone), as the stacked dense description"""

    def __init__(self, m, n, seed):
        from totsu_amd import _lib
        rng = np.random.default_rng(seed)
        self.n, self.m = n, m
        self.mat_a = (rng.standard_normal(m * n, dtype=np.float32) / np.float32(np.sqrt(n)))       # column-major m x n
        self.vec_b = rng.uniform(0.5, 1.5, m).astype(np.float32)
        self.vec_c = -rng.uniform(0, 1, n).astype(np.float32)
        self.seg_type, self.seg_len = [_lib.CONE_RPOS], [m]
        self.vec_b_rowabs = None


def _stored(dense, kind):
    """the problem the 16-bit storage solves: the same with the rounded (bf16) / dequantised (f16) matrix"""
    import copy
    from test_gpu_bf16 import bf16_round, f16_quantize
    d = copy.copy(dense)
    if kind == "bf16":
        d.mat_a = bf16_round(np.asarray(dense.mat_a, np.float32))
    elif kind == "f16":
        A = np.asarray(dense.mat_a, np.float32).reshape((dense.n, dense.m)).T
        d.mat_a = np.asfortranarray(f16_quantize(A)[2]).ravel(order="F")
    return d


def _oracle(dense):
    return O.solve_matop_cones(O.param(max_iter=max(ITERS) + 2, eps_acc=1e-30), dense.vec_c, dense.mat_a, dense.vec_b, dense.seg_type,
                               dense.seg_len, snap_iters=ITERS, trace_cap=max(ITERS) + 3, use_ql=True)


@pytest.fixture(scope="module")
def lps():
    """the two LPs (sweep_plans.six_candidate_shapes) and the oracle's runs on them, made once: name -> (dense, {storage: oracle})"""
    small, two_up = P.six_candidate_shapes()
    out = {}
    for name, (m, n) in (("small", small), ("two_up", two_up)):
        d = _Lp(m, n, seed=m + n)
        out[name] = (d, {})
    return out


def _lp_oracle(lps, name, kind):
    d, ros = lps[name]
    if kind not in ros:
        ros[kind] = _oracle(_stored(d, kind))
    return d, ros[kind]


def _m_eff(m, elem):
    return -(-m // EPV[elem]) * EPV[elem]         # the library's own copy has zero rows up to a whole 16-byte slot


def _key(c):
    return (c["members"], c["cols_per_panel"], c["nslot"])


def _bitwise_twins(T, dense, pin, a_storage, expect):
    """two solvers pinned to the same candidate agree bit for bit after 10 iterations"""
    p = T.SolverParam()
    p.eps_acc = 1e-30
    res = []
    for _ in range(2):
        fs = T.FusedSolver.from_dense(dense, p, "sweep", sweep_min_bytes=0, a_storage=a_storage)
        fs.pin_sweep_plan(pin)
        plan = fs.sweep_plan()
        assert (plan["workgroups_per_column_group"], plan["columns_per_panel"], plan["slots_per_thread"]) == expect
        fs.run(10, poll_every=10)
        res.append(fs.iterate())
        assert fs.schedule_in_use() == "sweep" and fs.sweep_faults()["faults"] == 0
        fs.destroy()
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1]), (pin, expect)


# (storage, LP, candidate): six each for f32; the 16-bit forms offer four on the larger LP
SOLVER = [("f32", lp, i) for lp in ("small", "two_up") for i in range(6)] + [(k, "two_up", i) for k in ("bf16", "f16") for i in range(4)]


@pytest.mark.parametrize("kind,lp,idx", SOLVER, ids=["%s-%s-c%d" % c for c in SOLVER])
def test_solver_under_each_pinned_candidate(T, lps, kind, lp, idx):
    elem = {"f32": F32, "bf16": BF16, "f16": F16}[kind]
    dense, ro = _lp_oracle(lps, lp, kind)
    cands = P.candidates(_m_eff(dense.m, elem), dense.n, elem)
    assert len(cands) == (6 if elem == F32 else 4), cands          # (the parametrisation above lists every candidate)
    expect = _key(cands[idx])
    assert _check_sweep_iterates(T, dense, ITERS, TOLS, ro=ro, pin=idx, expect=expect, a_storage=kind) == expect
    _bitwise_twins(T, dense, idx, kind, expect)


@pytest.mark.parametrize("kind", ["f32", "bf16", "f16"])
def test_solver_unpinned_again_runs_the_librarys_choice(T, lps, kind):
    """pin, then -1: the plan autotune's own pick -- one of the candidates -- runs and passes the same comparison"""
    elem = {"f32": F32, "bf16": BF16, "f16": F16}[kind]
    dense, ro = _lp_oracle(lps, "two_up", kind)
    cands = [_key(c) for c in P.candidates(_m_eff(dense.m, elem), dense.n, elem)]
    p = T.SolverParam()
    p.eps_acc = 1e-30
    fs = T.FusedSolver.from_dense(dense, p, "sweep", sweep_min_bytes=0, a_storage=kind)
    fs.pin_sweep_plan(len(cands) - 1)
    plan = fs.sweep_plan()
    assert (plan["workgroups_per_column_group"], plan["columns_per_panel"], plan["slots_per_thread"]) == cands[-1]
    fs.destroy()
    geom = _check_sweep_iterates(T, dense, ITERS, TOLS, ro=ro, pin=-1, a_storage=kind)
    assert geom in cands, (geom, cands)


def test_solver_refuses_a_candidate_the_matrix_does_not_offer_and_stays_usable(T, lps):
    from totsu_amd import _lib
    dense, ro = _lp_oracle(lps, "small", "f32")
    p = T.SolverParam()
    p.eps_acc = 1e-30
    fs = T.FusedSolver.from_dense(dense, p, "sweep", sweep_min_bytes=0)
    fs.pin_sweep_plan(4)
    before = fs.sweep_plan()
    for bad in (6, 7, 100, -2):
        with pytest.raises(_lib.ThipError) as err:
            fs.pin_sweep_plan(bad)
        assert err.value.code == _lib.E_INVALID
    after = fs.sweep_plan()
    assert {k: after[k] for k in after if k != "autotune_ms_per_sweep"} == {k: before[k] for k in before if k != "autotune_ms_per_sweep"}
    assert after["workgroups_per_column_group"] == 2 and after["columns_per_panel"] == 2
    fs.run(10, poll_every=10)
    x, y = fs.iterate()
    N = dense.n + 2 * dense.m + 1
    rx, ry = ro.snaps[3][:N], ro.snaps[3][N:]
    assert np.abs(x - rx).max() <= TOLS[3] * max(np.abs(rx).max(), 1e-6) and np.abs(y - ry).max() <= TOLS[3] * max(np.abs(ry).max(), 1e-6)
    fs.destroy()
    # a solver the one-pass kernel does not run for has nothing to pin
    fc = T.FusedSolver.from_dense(dense, p, "carried")
    with pytest.raises(_lib.ThipError) as err:
        fc.pin_sweep_plan(0)
    assert err.value.code == _lib.E_INVALID
    fc.pin_sweep_plan(-1)
    fc.destroy()


def test_solver_socp_with_block_cones_under_pinned_candidates(T):
    """second-order cones of up to 1000 rows (longer than a wave per cone takes: the m-tail is the three-launch form) on 5120 columns,
    where the planner offers a two-column candidate and one-column candidates at two and four times the smallest group"""
    # (an instance whose d_i are all positive: the oracle is handed b as a MatOp and takes |b| into its row sums, the library the
    # signed d_i -- see test_sweep_iterates_socp_rows_not_a_multiple_of_4; with seed 3 the row of the empty cone has d = -0.27 and
    # every schedule alike is 1e-4 off the oracle in that row's preconditioner)
    from problems import random_socp
    cones, seed = [5, 1, 0, 17, 999, 3, 32, 131], 4
    assert min(random_socp(5120, cones, seed=seed)[4]) > 0
    socp = _socp(T, 5120, cones, seed=seed)
    dense = socp.dense()
    assert dense.m % 4 == 0
    cands = [_key(c) for c in P.candidates(dense.m, dense.n, F32)]
    two_col = next(i for i, c in enumerate(cands) if c[1] == 2)
    bigger = next(i for i, c in enumerate(cands) if c[1] == 1 and c[0] > cands[0][0])
    ro = _oracle(dense)
    iters, tols = [0, 1, 2, 9], [2e-5, 2e-5, 2e-5, 1e-4]          # test_sweep_iterates_socp's, to iterate 9
    for idx in (two_col, bigger):
        assert _check_sweep_iterates(T, dense, iters, tols, ro=ro, pin=idx, expect=cands[idx]) == cands[idx]
    p = T.SolverParam()
    p.eps_acc = 1e-30
    fs = T.FusedSolver.from_dense(dense, p, "sweep", sweep_min_bytes=0)
    fs.pin_sweep_plan(two_col)
    fs.run(3, poll_every=3)
    assert fs.kahan_terms()[1] == 3                           # the three-launch m-tail
    fs.destroy()
