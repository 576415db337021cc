"""CPU: the planning of the one-pass kernel (sweep_plan_one / sweep_candidates / sweep_gran_words through thip_test_sweep_plan, which
launches nothing and assumes 256 CUs): every geometry a plan can return is one the kernel has an instance for and covers the matrix,
every refusal the kernel relies on is made, and the row counts tests/test_gpu_sweep_instances.py uses do reach every body of the
16-bit row deal and both ends of f16's balance window."""
import pytest

import sweep_plans as P
from sweep_plans import BF16, CAND, ELEMS, EPV, F16, F32, GROUP_SIZES, INSTANCES, MAX_SLOTS, SLOT, WIDTHS

SW_RING = 32            # granule slots per group (thip_sweep_kernel.h)


def _ceil(a, b):
    return -(-a // b)


def _rows_of(m, G, e):
    return _ceil(_ceil(m, G), e) * e


def _check(g, m, n, elem, w):
    e, S = EPV[elem], SLOT[elem]
    ctx = (m, n, elem, w, g)
    G, ng, rpm, cpg = g["members"], g["ngroups"], g["rows_per_member"], g["cols_per_group"]
    assert G in GROUP_SIZES and G * ng == 256, ctx
    assert rpm == _rows_of(m, G, e) and G * rpm >= m and rpm % e == 0, ctx
    assert 1 <= g["nslot"] <= MAX_SLOTS[elem, w] and g["nslot"] == _ceil(rpm, S), ctx
    assert (w, g["nslot"]) in INSTANCES[elem] and g["cols_per_panel"] == w and g["elem"] == elem, ctx
    assert cpg % w == 0 and g["npan"] == cpg // w and g["npan"] >= 40, ctx
    assert ng * cpg >= n, ctx
    assert cpg == max(40 * w, _ceil(_ceil(n, ng), w) * w), ctx          # no more columns per group than the matrix needs
    assert g["mpad"] >= m and g["mpad"] % 64 == 0 and g["mpad"] < m + 64, ctx
    # a granule per member, quantity (2 W) and ring entry of every group, and a spare 128-byte line per workgroup
    assert g["gran_words"] == ng * SW_RING * G * 2 * w + 256 * 16, ctx


def _row_counts(elem, w):
    """m around every multiple of the slot size up to the family's cap, for every group size"""
    e, S = EPV[elem], SLOT[elem]
    out = {e, 2 * e, 100 // e * e + e}
    for G in GROUP_SIZES:
        for k in range(1, MAX_SLOTS[elem, w] + 1):
            out |= {G * k * S - e, G * k * S, G * k * S + e, G * k * S - G * e, G * k * S + G * e}
    return sorted(v for v in out if v > 0)


@pytest.mark.parametrize("elem", ELEMS)
def test_every_plan_is_an_instance_and_covers_the_matrix(elem):
    e = EPV[elem]
    seen, count = set(), 0
    for w in WIDTHS[elem]:
        cap = 32 * MAX_SLOTS[elem, w] * SLOT[elem]
        for m in _row_counts(elem, w):
            for n in (40 * w, 40 * w + 1, 1000, 5120 * w - 1, 10240 * w - 1, 10240 * w, 30011):
                for gmul in (1, 2, 4, 8):
                    g = P.plan(m, n, elem, w, gmul)
                    fits = _rows_of(m, 32, e) <= MAX_SLOTS[elem, w] * SLOT[elem]
                    if gmul == 1:
                        assert (g is not None) == fits, (m, n, elem, w)      # every shape whose rows fit 32 members is taken
                    assert g is None or m <= cap
                    if g is None:
                        continue
                    count += 1
                    _check(g, m, n, elem, w)
                    seen.add((w, g["nslot"]))
                    # the fewest members the rows fit, times gmul; more only under the few-columns rule, and only for gmul = 1
                    g_rows = min(G for G in GROUP_SIZES if _rows_of(m, G, e) <= MAX_SLOTS[elem, w] * SLOT[elem])
                    g_cols = min([G for G in GROUP_SIZES if 256 // G * 40 * w <= n] or [32])
                    want = max(g_rows, g_cols) if gmul == 1 else g_rows * gmul
                    assert g["members"] == want, (m, n, elem, w, gmul, g)
                    assert gmul == 1 or g_rows * gmul >= g_cols
    assert seen == set(INSTANCES[elem]), (elem, seen ^ set(INSTANCES[elem]))       # and every instance is planned for some shape
    assert count > 300


@pytest.mark.parametrize("elem", ELEMS)
def test_pinned_group_sizes(elem):
    """force_members > 0 is the exact group size: any power of two the rows fit, also below the few-columns rule"""
    e, S = EPV[elem], SLOT[elem]
    for w in WIDTHS[elem]:
        for ns in range(1, MAX_SLOTS[elem, w] + 1):
            for G in GROUP_SIZES:
                for rpm in P.slot_edges(elem, ns):
                    for m in {G * rpm, G * rpm - e * (G > 1)}:
                        n = 40 * w + 7
                        g = P.plan(m, n, elem, w, members=G)
                        assert g is not None, (m, n, elem, w, G)
                        _check(g, m, n, elem, w)
                        assert (g["members"], g["nslot"], g["npan"]) == (G, ns, 40), (m, w, G, g)
                # one lane more than the family's slots hold: refused at this group size, taken by the next
                m = G * MAX_SLOTS[elem, w] * S + e
                assert P.plan(m, 200, elem, w, members=G) is None
                assert G == 32 or P.plan(m, 200, elem, w, members=2 * G)["nslot"] == _ceil(_rows_of(m, 2 * G, e), S)


def test_refusals():
    for elem in ELEMS:
        e, S = EPV[elem], SLOT[elem]
        for w in WIDTHS[elem]:
            ok = dict(m=2 * S, n=40 * w, elem=elem, w=w, members=2)
            assert P.plan(**ok) is not None
            assert P.plan(**dict(ok, n=40 * w - 1)) is None                   # fewer than 40 panels' columns
            assert P.plan(**dict(ok, n=40 * w - 1, members=0)) is None
            assert P.plan(**dict(ok, m=2 * S + e // 2)) is None               # rows not a multiple of the rows per slot
            assert P.plan(**dict(ok, m=2 * S + e // 2, members=0)) is None
            assert P.plan(**dict(ok, lda=2 * S + e // 2)) is None             # columns that do not start on 16 bytes
            assert P.plan(**dict(ok, lda=2 * S - e)) is None                  # lda < m
            for G in (3, 5, 6, 12, 24, 33, 48, 64):
                assert P.plan(**dict(ok, members=G)) is None                  # not a power of two up to 32
            assert P.plan(**dict(ok, m=32 * MAX_SLOTS[elem, w] * S + e, members=32)) is None       # the rows do not fit 32 members
            assert P.plan(**dict(ok, m=32 * MAX_SLOTS[elem, w] * S + e, members=0)) is None
        for w in (0, 3, 5, 8):
            assert P.plan(2 * S, 400, elem, w) is None and P.plan(2 * S, 400, elem, w, members=2) is None
    assert P.plan(1792, 400, F32, 4) is None and P.plan(1792, 400, F32, 4, members=1) is None      # four columns: 16-bit only
    # the instance the build guard refuses (4 slots x 2 columns at 16-bit) cannot be planned: the rows go to the next group size
    for elem in (BF16, F16):
        assert P.plan(4 * SLOT[elem], 400, elem, 2, members=1) is None
        assert P.plan(4 * SLOT[elem], 20480, elem, 2)["members"] == 2
    assert P.plan(0, 400, F32, 1) is None and P.plan(1792, 0, F32, 1) is None


@pytest.mark.parametrize("elem", ELEMS)
def test_candidates_are_distinct_instances(elem):
    e = EPV[elem]
    most = 0
    for w in WIDTHS[elem]:
        for m in _row_counts(elem, w)[::3]:
            for n in (40, 80, 160, 1000, 5120, 10240, 20480, 40960, 50000):
                cs = P.candidates(m, n, elem)
                most = max(most, len(cs))
                keys = [(c["members"], c["cols_per_panel"], c["nslot"]) for c in cs]
                assert len(set(keys)) == len(keys) <= 6, (m, n, elem, cs)
                for c in cs:
                    _check(c, m, n, elem, c["cols_per_panel"])
                # the list is what the (W, gmul) pairs of sweep_candidates plan, in order, without repeats
                want = []
                for w_, gm in CAND[elem]:
                    g = P.plan(m, n, elem, w_, gm)
                    if g is not None and (g["members"], w_, g["nslot"]) not in [(x["members"], x["cols_per_panel"], x["nslot"]) for x in want]:
                        want.append(g)
                assert cs == want, (m, n, elem)
    assert most == 6                                  # (all six pairs do give distinct geometries on some shape)


def test_smallest_shapes_with_six_f32_candidates():
    (m0, n0), (m1, n1) = P.six_candidate_shapes()
    # fewest entries of all: any row count with 20 480 columns (256 one-member groups of 40 two-column panels)
    assert (m0, n0) == (4, 20480)
    assert [(c["members"], c["cols_per_panel"], c["nslot"]) for c in P.candidates(m0, n0, F32)] == \
        [(1, 1, 1), (2, 1, 1), (4, 1, 1), (1, 2, 1), (2, 2, 1), (8, 1, 1)]
    # with the two-column family starting at two members: rows just above three slots, 10 240 columns
    assert (m1, n1) == (3 * SLOT[F32] + 4, 10240)
    assert [(c["members"], c["cols_per_panel"], c["nslot"]) for c in P.candidates(m1, n1, F32)] == \
        [(1, 1, 4), (2, 1, 2), (4, 1, 1), (2, 2, 2), (4, 2, 1), (8, 1, 1)]
    # one row or one column less loses a candidate
    assert len(P.candidates(m1 - 4, n1, F32)) < 6 and len(P.candidates(m1, n1 - 1, F32)) < 6 and len(P.candidates(m0, n0 - 1, F32)) < 6


@pytest.mark.parametrize("elem", (BF16, F16))
def test_the_row_counts_of_the_gpu_tests_reach_every_body_of_the_16_bit_deal(elem):
    for w, ns in INSTANCES[elem]:
        rows = dict(P.wave3_rows(elem, ns))
        if ns > 1:
            rows.update(P.bal_rows(ns))
        bodies = set()
        for tag, r in rows.items():
            g = P.plan(r, 40 * w, elem, w, members=1)
            assert g is not None and g["nslot"] == ns, (elem, w, ns, tag, r, g)
            bal, slots = P.wave_slots_16(elem, ns, r)
            assert sum(slots) * 64 * EPV[elem] >= r > (sum(slots) - 1) * 64 * EPV[elem] - (64 * EPV[elem] if bal else 0), (tag, slots)
            bodies |= set(slots)
            if tag.startswith("w3=") and not bal:
                k = tag[3:]
                assert slots[3] == (ns if k == "part" else int(k)) and slots[:3] + slots[4:] == [ns] * 6, (tag, slots)
            if tag.startswith("rem="):
                rem = int(tag[4:])
                assert bal == (elem == F16 and 0 <= rem <= 64 * ns), (tag, bal)
                if bal:
                    assert slots[:3] == [ns] * 3 and slots[4:] == [ns - 1] * 3 and slots[3] == _ceil(rem, 64), (tag, slots)
        if ns == 4:
            for tag, (G, m) in P.bal_rows_last_member().items():
                g = P.plan(m, 40 * w, elem, w, members=G)
                assert g is not None and g["nslot"] == ns, (elem, tag, g)
                last = m - (G - 1) * g["rows_per_member"]
                bal, slots = P.wave_slots_16(elem, ns, last)
                assert last == 8 * (1344 if tag.endswith("=0") else 1343) and bal == (elem == F16 and tag.endswith("=0")), (tag, last, bal)
                assert slots[3] == 0, (tag, slots)
                bodies |= set(slots)
        assert bodies == set(range(ns + 1)), (elem, w, ns, bodies)          # stream(ns) .. stream(0) each run in some case
