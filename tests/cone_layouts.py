"""Cone layouts for the iterate-vs-oracle tests of every loop that projects on second-order and rotated second-order cones
(tests/test_cone_layouts_cpu.py, tests/test_gpu_cone_layouts.py): named layouts of (cone type, length) segments, a constructive
generator that makes the f64 oracle itself visit all three branches of the projection (cone_soc.rs:49-61: polar to zero, inside
unchanged, outside scaled to the boundary) on every block cone, the classification of an oracle snapshot into those branches, and
the oracle runs, computed once per session and never changed.  A plain module, like tests/ownbatch_cases.py: no fixtures, no device."""
import zlib

import numpy as np

import oracle as O
from ownbatch_cases import F, ITERS, SDP_ITERS, SDP_TOLS, TOLS, _D, _oracle, _psd_block, tri

Z, P, S, R, PSD = O.CONE_ZERO, O.CONE_RPOS, O.CONE_SOC, O.CONE_ROTSOC, O.CONE_PSD
KIND = {S: "soc", R: "rot"}
SQ2 = np.sqrt(2.0)

# the block cones of `small`: SOC 0, 1, 2, 3, 64, 65, 66, 129, 130, rotated 1, 2, 3, 4, 65, 66, 129, 130 (around a wave of 64
# lanes, its two slots + head, and the 64-stride loop on a later pass); the short ones and SOC 64 twice, side by side or apart; zero
# and nonnegative rows so that block cones start at every offset mod 4; a zero segment in the middle and one at the end; m = 950
_RAGGED = [(P, 1), (S, 3), (S, 3), (R, 2), (R, 2), (S, 0), (S, 1), (R, 1), (S, 64), (R, 65), (Z, 2), (S, 65), (R, 66), (P, 2), (S, 66),
           (R, 3), (R, 3), (R, 4), (R, 4), (S, 2), (S, 2), (R, 129), (S, 129), (P, 1), (R, 130), (S, 130), (S, 64), (P, 3), (Z, 3)]
# `mid` has the room for a second cone of every long length as well; m = 1733
_RAGGED2 = _RAGGED[:-2] + [(R, 65), (S, 65), (P, 1), (R, 66), (S, 66), (R, 129), (P, 2), (S, 129), (R, 130), (S, 130)] + _RAGGED[-2:]
_SHORT = [(S, 5), (S, 0), (S, 1), (S, 2), (S, 128), (S, 129), (S, 17), (S, 2), (S, 64), (S, 3)]
# PSD orders 2, 1, 3, 32, 33 behind three nonnegative rows: the blocks start at rows 3, 6, 7, 13, 541
_PSD_HEAD, _PSD_TAIL = [(P, 3), (PSD, tri(2)), (PSD, tri(1)), (PSD, tri(3)), (PSD, tri(32)), (PSD, tri(33))], \
    [(S, 17), (R, 5), (R, 1), (R, 2), (R, 2), (Z, 2)]

# name -> n, the segments, the seeds in use (seed: its own A; several seeds: the problems of one own-A batch), the instances of a
# seed (instance: its own x0, s0, y0 over the seed's A -- the members of one BatchSolver), `turn`: which target the first block
# cone gets (targets()); seeds and turn are tuned until the oracle alone covers every branch (tests/test_cone_layouts_cpu.py).
# strict: it does so without the snapshot of iterate 0, where every block is the projection of the zero vector.  Where cones of
# hundreds of rows have a hundred iterations (long) or the problem is scaled down (psd*), no block of those cones is sent to zero
# again that soon, and the zero branch of those lengths is the one of iterate 0; `scale`: see build()
LAYOUTS = {
    "small": dict(n=24, segs=_RAGGED, seeds=(0, 1, 2, 3), instances=(0, 1, 2), turn=0, strict=True),
    "mid": dict(n=96, segs=_RAGGED2, seeds=(3, 4, 5, 6), instances=(0,), turn=0, strict=True),
    "short_soc": dict(n=96, segs=_SHORT, seeds=(9,), instances=(0,), turn=0, strict=True),
    "short_soc_rot": dict(n=96, segs=_SHORT + [(R, 2)], seeds=(13,), instances=(0,), turn=0, strict=True),
    "long": dict(n=100, segs=[(P, 3), (S, 2048), (R, 1), (R, 2049), (S, 2), (S, 2049), (S, 300), (R, 2048), (R, 2), (S, 1), (R, 300),
                              (S, 2), (R, 300), (P, 2)], seeds=(3,), instances=(0, 1, 2), turn=0, strict=False),
    "psd": dict(n=96, segs=_PSD_HEAD + _PSD_TAIL, seeds=(0, 1, 2, 3), instances=(0,), turn=0, strict=False, scale=(0.02, 0.1)),
    # the largest order the one-workgroup chain takes (64) and the next one above it
    "psd_big": dict(n=96, segs=_PSD_HEAD + [(PSD, tri(64)), (PSD, tri(65))] + _PSD_TAIL, seeds=(0,), instances=(0,), turn=0,
                    strict=False, scale=(0.02, 0.1)),
}


def segments(layout):
    """(seg_type, seg_len, first row of every segment)"""
    st, sl = [t for t, _ in LAYOUTS[layout]["segs"]], [l for _, l in LAYOUTS[layout]["segs"]]
    return st, sl, [int(b) for b in np.cumsum([0] + sl)[:-1]]


def has_psd(layout):
    return any(t == PSD for t, _ in LAYOUTS[layout]["segs"])


def iters_tols(layout):
    """the project's iterates and tolerances (tests/ownbatch_cases.py)"""
    return (SDP_ITERS, SDP_TOLS) if has_psd(layout) else (ITERS, TOLS)


def _rng(layout, *key):
    return np.random.default_rng([zlib.crc32(layout.encode())] + [int(k) for k in key])


def rot(x):
    """the change of variables of cone_rotsoc.rs:38-65 on the first two entries (its own inverse): (r, s) -> ((r + s), (r - s)) / sqrt 2"""
    x = np.array(x, dtype=np.float64)
    if x.size >= 2:
        x[0], x[1] = (x[0] + x[1]) / SQ2, (x[0] - x[1]) / SQ2
    return x


def _soc_pair(rng, l, target):
    """(s0, y0) of one second-order cone of l >= 1 rows.  target 0: s0 strictly inside, y0 = 0; 1: s0 = 0, y0 strictly inside;
    2: both on the boundary and complementary, y0 = a (s_0, -s_tail)"""
    v = rng.standard_normal(l - 1)
    nv = np.linalg.norm(v)
    if l == 1:                                    # the half line: one of the two is positive
        w = np.array([rng.uniform(0.1, 1.1)])
        return (w, np.zeros(1)) if target != 1 else (np.zeros(1), w)
    if target == 2:
        s = np.concatenate([[nv], v])
        return s, rng.uniform(0.5, 1.5) * np.concatenate([[nv], -v])
    w = np.concatenate([[rng.uniform(1.5, 2.5) * nv + rng.uniform(0.1, 1.1)], v])      # well inside: the margin grows with the cone
    return (w, np.zeros(l)) if target == 0 else (np.zeros(l), w)


def targets(layout):
    """segment index -> target (0, 1, 2) of every block cone with rows: the first cone of a (type, length) gets 0 or 1 in
    alternation, beginning at the layout's `turn`, and a later one of the same (type, length) gets 2.  (A cone of target 0 or 1
    passes through the boundary branch on its way and ends inside or at zero; one of target 2 ends on the boundary and is seldom
    inside on its way.  With 0, 1, 2 in plain rotation a third of the (type, length) pairs never showed "inside" at four iterates.)"""
    out, q, seen = {}, LAYOUTS[layout]["turn"], set()
    for i, (t, l) in enumerate(LAYOUTS[layout]["segs"]):
        if t in (S, R) and l > 0:
            if (t, l) in seen:
                out[i] = 2
                continue
            out[i] = q % 2
            q += 1
            seen.add((t, l))
    return out


def _point(layout, seed, instance):
    """x0 and, for every segment that is no PSD cone, (s0, y0): a primal- and dual-feasible, complementary pair"""
    L = LAYOUTS[layout]
    rng = _rng(layout, seed, instance, 1)
    x0 = rng.standard_normal(L["n"])
    tg = targets(layout)
    s0, y0 = [], []
    for i, (t, l) in enumerate(L["segs"]):
        if t == Z:
            s, y = np.zeros(l), rng.standard_normal(l)
        elif t == P:
            pick = rng.uniform(size=l) < 0.5
            w = rng.uniform(0.1, 1.1, l)
            s, y = np.where(pick, w, 0.0), np.where(pick, 0.0, w)
        elif t == PSD or l == 0:
            s, y = np.zeros(l), np.zeros(l)
        else:
            s, y = _soc_pair(rng, l, tg[i])
            if t == R:
                s, y = rot(s), rot(y)
        s0.append(s)
        y0.append(y)
    return x0, np.concatenate(s0), np.concatenate(y0)


_A = {}


def _matrix(T, layout, seed):
    """(A in f32, the PSD rows' b, their c): what the instances of a seed share"""
    if (layout, seed) in _A:
        return _A[layout, seed]
    L = LAYOUTS[layout]
    n = L["n"]
    st, sl, beg = segments(layout)
    m = sum(sl)
    rng = _rng(layout, seed, 0)
    A = (rng.standard_normal((m, n)) / np.sqrt(n)).astype(F)
    b_psd, c_psd, q = np.zeros(m, F), np.zeros(n, F), 0
    for t, l, b0 in zip(st, sl, beg):
        if t == PSD:                              # as tests/ownbatch_cases.py::_mixed_dense builds them
            k = int(round((np.sqrt(8 * l + 1) - 1) / 2))
            A[b0:b0 + l], b_psd[b0:b0 + l], c = _psd_block(T, n, k, 10 + q + 100 * seed)
            c_psd += c
            q += 1
    if q:
        c_psd /= q
    _A[layout, seed] = (A, b_psd, c_psd)
    return _A[layout, seed]


def build(layout, seed, instance=0, T=None):
    """the dense problem (the fields of Prob*.dense()) with x0, s0, y0 and the f64 b and c beside it.  Without PSD blocks
    b = A x0 + s0 and c = -A^T y0 over A = randn / sqrt(n) in f32, (s0, y0) per block cone one of three targets (targets(),
    _soc_pair; the rotated cone the same after its change of variables), nonnegative rows split at random between s0 > 0 and
    y0 > 0, zero-cone rows with a free y0.  `instance` changes x0, s0, y0 and not A.  PSD rows (T = totsu_amd is needed for
    them; no device) come from _psd_block.  A layout's `scale` (the PSD layouts) multiplies b -- x0, s0 and the PSD rows' b -- by
    scale[0] and c -- y0 and the mean of the PSD blocks' c -- by scale[1]: each PSD block stays strictly feasible at scale[0]
    times its own x0, and as the blocks come, with n near 100, tau falls to zero within ten iterations, which is the subject of
    tests/test_gpu_tau_zero.py and not of these"""
    if T is None and has_psd(layout):
        import totsu_amd as T
    A, b_psd, c_psd = _matrix(T, layout, seed)
    x0, s0, y0 = _point(layout, seed, instance)
    st, sl, beg = segments(layout)
    A64 = A.astype(np.float64)
    other = np.concatenate([np.full(l, t != PSD) for t, l in zip(st, sl)] + [np.zeros(0, bool)])
    sb, sc = LAYOUTS[layout].get("scale", (1.0, 1.0))
    x0, s0, y0 = sb * x0, sb * s0, sc * y0
    b = np.where(other, A64 @ x0 + s0, sb * b_psd.astype(np.float64))
    c = -A64.T @ y0 + sc * c_psd
    d = _D(A, b, c, st, sl)
    d.x0, d.s0, d.y0, d.b64, d.c64, d.layout = x0, s0, y0, b, c, layout
    return d


def classify(kind, x):
    """one projected block-cone segment of a snapshot: 'zero', 'inside' (s0 > ||v||; a cone of one row: 'positive'), 'boundary'
    (|s0 - ||v||| <= 1e-9 max(|s0|, ||v||)), in f64 after the rotated change of variables -- or 'outside', which no projected
    iterate is"""
    x = np.asarray(x, dtype=np.float64)
    if x.size == 1:
        return "zero" if x[0] == 0.0 else "positive" if x[0] > 0.0 else "outside"
    if kind == R:
        x = rot(x)
    t, nv = x[0], np.linalg.norm(x[1:])
    mx = max(abs(t), nv)
    if mx == 0.0:
        return "zero"
    if abs(t - nv) <= 1e-9 * mx:
        return "boundary"
    return "inside" if t > nv else "outside"


def branches(layout, snapshot):
    """from an oracle snapshot alone: [(segment index, kind 'soc' / 'rot', length, 'y' / 's', branch)] of every second-order and
    rotated segment with rows, of x_y and of x_s"""
    n = LAYOUTS[layout]["n"]
    st, sl, beg = segments(layout)
    m = sum(sl)
    out = []
    for which, base in (("y", n), ("s", n + m)):
        for i, (t, l, b0) in enumerate(zip(st, sl, beg)):
            if t in (S, R) and l > 0:
                out.append((i, KIND[t], l, which, classify(t, snapshot[base + b0:base + b0 + l])))
    return out


def coverage(layout, ro, iters=None, strict=False):
    """(kind, length) -> the set of branches the oracle run ro visits over its snapshots.  strict: the snapshot of iterate 0 does
    not count -- there every block is the projection of the zero vector, which any arm of any copy maps to zero"""
    iters = iters_tols(layout)[0] if iters is None else iters
    cov = {}
    for it, snap in zip(iters, ro.snaps):
        for _, kind, l, _, br in branches(layout, snap):
            if it > 0 or not strict:
                cov.setdefault((kind, l), set()).add(br)
    return cov


def wanted(length):
    return {"zero", "positive"} if length == 1 else {"zero", "inside", "boundary"}


_ORACLES = {}


def oracle(layout, seed=0, instance=0, iters=None, T=None):
    """(the dense problem, its oracle run): O.solve_matop_cones with use_ql=True and eps_acc = 1e-30, snapshots at `iters` (default:
    the layout's iterates), computed once per session"""
    iters = list(iters_tols(layout)[0] if iters is None else iters)
    key = (layout, seed, instance, tuple(iters))
    if key not in _ORACLES:
        d = build(layout, seed, instance, T)
        _ORACLES[key] = (d, _oracle(d, iters))
    return _ORACLES[key]
