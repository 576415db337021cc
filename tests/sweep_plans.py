"""Shared by tests/test_sweep_plan_cpu.py and tests/test_gpu_sweep_instances.py: the instances of the one-pass kernel restated as
data (the dispatch tables of sweep_launch in totsu_amd/csrc/thip_sweep.hip and of sweep_launch16 in thip_sweep16.hip), the planning
hook (thip_test_sweep_plan, which needs no GPU), and the row counts that put a member on the edges of the kernel's row deal."""
import ctypes as C

F32, BF16, F16 = 0, 1, 2
ELEMS = (F32, BF16, F16)
KIND = {F32: "f32", BF16: "bf16", F16: "f16"}
CW, CT = 7, 448                                  # streaming waves and streaming threads of a workgroup (SW_CW, SW_CT)
EPV = {F32: 4, BF16: 8, F16: 8}                  # rows per 16-byte slot
SLOT = {e: CT * EPV[e] for e in ELEMS}           # rows one slot of all streaming threads holds: 1792 / 3584
WIDTHS = {F32: (1, 2), BF16: (1, 2, 4), F16: (1, 2, 4)}
# (elem, W) -> the slot counts sweep_launch / sweep_launch16 have an instance for
MAX_SLOTS = {(F32, 1): 7, (F32, 2): 3, (BF16, 1): 4, (BF16, 2): 3, (BF16, 4): 2, (F16, 1): 4, (F16, 2): 3, (F16, 4): 2}
INSTANCES = {e: [(w, ns) for w in WIDTHS[e] for ns in range(1, MAX_SLOTS[e, w] + 1)] for e in ELEMS}
GROUP_SIZES = (1, 2, 4, 8, 16, 32)
LAGT = 5                                         # panels a load runs ahead of its axpy: 2 register stages + 3 LDS panels (every
#                                                  instance but <2 slots, 4 columns>, which parks 2 panels: 4)
# the (W, gmul) pairs sweep_candidates tries, in its order
CAND = {F32: [(1, 1), (1, 2), (1, 4), (2, 1), (2, 2), (1, 8)], BF16: [(1, 1), (4, 1), (2, 1), (2, 2), (4, 2), (1, 2)]}
CAND[F16] = CAND[BF16]

_FIELDS = ("members", "ngroups", "rows_per_member", "cols_per_group", "npan", "nslot", "cols_per_panel", "elem", "mpad", "gran_words")


def _rec(r):
    return {k: int(getattr(r, k)) for k in _FIELDS}


def plan(m, n, elem, w, gmul=1, members=0, lda=None):
    """thip_test_sweep_plan: the geometry as a dict, or None where the kernel has no instance for it (THIP_E_INVALID).
    members > 0: exactly that group size (the pin of thip_sweep_test); else the planner's, times gmul."""
    from totsu_amd import _lib
    rec = _lib.SweepPlanRec()
    try:
        _lib.lib.thip_test_sweep_plan(m, n, m if lda is None else lda, elem, w, gmul, members, C.byref(rec), None, None)
    except _lib.ThipError as e:
        assert e.code == _lib.E_INVALID, e
        return None
    return _rec(rec)


def candidates(m, n, elem, lda=None):
    """the geometries the solver's plan autotune would time on an m x n matrix, in its order (sweep_candidates)"""
    from totsu_amd import _lib
    recs = (_lib.SweepPlanRec * 6)()
    k = C.c_int(0)
    _lib.lib.thip_test_sweep_plan(m, n, m if lda is None else lda, elem, 1, 1, 0, None, recs, C.byref(k))
    return [_rec(recs[i]) for i in range(k.value)]


def six_candidate_shapes():
    """The smallest LP shapes (fewest entries m n, m a multiple of 4) on which sweep_candidates offers six distinct f32 geometries,
    by search over the seams of the planner -- n at the multiples of 40 W 256 / G where the few-columns rule lets go, m just above the
    multiples of the slot size where a family needs the next group size.  Two of them: the smallest of all, and the smallest on which
    the two-column family starts at two members per group (so that instances with more than one slot are among the six)."""
    ns = sorted({256 // g * 40 * w for g in GROUP_SIZES for w in (1, 2)})
    ms = sorted({4} | {g * k * SLOT[F32] + 4 for g in GROUP_SIZES for k in range(1, 8)})
    six = [(m * n, m, n) for m in ms for n in ns if len(candidates(m, n, F32)) == 6]
    smallest = min(six)
    two_up = min(s for s in six if next(c for c in candidates(s[1], s[2], F32) if c["cols_per_panel"] == 2)["members"] == 2)
    return smallest[1:], two_up[1:]


# ---- rows per member on the edges of the row deal ---------------------------------------------------------------------------------

def slot_edges(elem, nslot):
    """rows of a one-member group whose last slot is exactly full, holds one lane, and lacks one lane"""
    S, e = SLOT[elem], EPV[elem]
    return sorted({nslot * S, (nslot - 1) * S + e, nslot * S - e})


def wave3_rows(elem, nslot):
    """16-bit: rows r of a one-member group, keyed by what the last wave of the plain deal (wave 3, after waves 0 1 2 4 5 6 took
    64 nslot lane-slots each) is left with: k = nslot .. 0 whole slots, and (nslot - 1) slots + half a slot ("part").  r needs nslot
    slots per thread whenever it exceeds (nslot - 1) S, which 6 full waves do for nslot > 1; nslot = 1, k = 0 is a member that fills
    six waves exactly."""
    e = EPV[elem]
    out = {}
    for k in range(nslot, -1, -1):
        out["w3=%d" % k] = e * 64 * (6 * nslot + k)
    out["w3=part"] = e * (64 * (6 * nslot + nslot - 1) + 32)
    return out


def bal_rows(nslot):
    """f16's balanced deal applies when rem = lane-slots - 64 (3 nslot + 3 (nslot - 1)) lies in [0, 64 nslot]: rows with rem just
    outside and just inside both ends of the window (nslot > 1).  Four slots: rem <= 0 is 1344 lane-slots or fewer, which three
    slots hold (3 x 448) -- the window's lower end is the instance's own, and its first row count inside is rem = 1."""
    base = 64 * (3 * nslot + 3 * (nslot - 1))
    rems = [rem for rem in (-1, 0, 1, 64 * nslot, 64 * nslot + 1) if base + rem > (nslot - 1) * CT]
    if 0 in rems:
        rems.remove(1)
    return {"rem=%d" % rem: 8 * (base + rem) for rem in rems}


def bal_rows_last_member():
    """The lower end of the four-slot window, reached by the SHORT last member of a group (it lacks fewer lane-slots than the group
    has members): the others' 1345 lane-slots need four slots, the last one is left with 1344 (rem = 0: balanced, wave 3 without
    rows) or 1343 (rem = -1: plain deal).  tag -> (members, m)"""
    return {"last rem=0": (2, 8 * (2 * 1345 - 1)), "last rem=-1": (4, 8 * (4 * 1345 - 2))}


def wave_slots_16(elem, nslot, rows):
    """restatement of sweep_k's 16-bit row deal for one member of `rows` rows: (balanced?, slots holding rows per streaming wave
    0 .. 6) -- the `my_slots` each wave selects its body by"""
    e = EPV[elem]
    tls = (rows + e - 1) // e
    rem = tls - 64 * (3 * nslot + 3 * (nslot - 1))
    bal = elem == F16 and nslot > 1 and 0 <= rem <= 64 * nslot
    got = []
    for wave in range(CW):
        pos = CW - 1 if wave == 3 else (wave - 1 if wave > 3 else wave)
        base = pos * 64 * nslot
        short = False
        if bal:
            base = pos * 64 * nslot if pos <= 3 else 64 * (3 * nslot + (pos - 3) * (nslot - 1))
            short = 3 <= pos < 6
        got.append(sum(1 for sl in range(nslot) if not (short and sl == nslot - 1) and e * (base + sl * 64) + e <= rows))
    return bal, got
