"""The set of tests/test_gpu_raggedsparse.py and tests/test_raggedsparse_cpu.py: sparse problems of different shapes, cone layouts
and patterns that one RaggedSparseBatchSolver holds, all from constructions that exist (tests/sparse_cases.py,
tests/ownbatch_cases.py), and the plan of such a batch restated in numpy.  A plain module, like tests/sparse_cases.py.

The set (m x n):
    sparse_problem    lp40x30, lp257x129, lp300x200, mixed145x40, mixed700x300, lp1000x700, lp2000x1000 -- the last two are too big to
                      reside: resident and streamed members share one class; lp2000x1000 is also the largest map
    lengths_problem   both orientations: rows and columns of 0, 1, 31, 32, 33, 63, 64, 65, 128, 129, 140 entries
    tiny_problem      1 x 1, 1 x 300, 300 x 1
    zero_problem, identity_problem
    part22, part23, part34, part48 [0]   PSD orders 4, 6, 12, 32: graphs of different size
    mixed [0]         eight PSD orders with second-order cones, fully dense
The last five are built through the package's problem builders, which need the device; the CPU test plans them by their shapes
(DEVICE_BUILT), which the GPU test asserts to be the real ones."""
import numpy as np

from ownbatch_cases import ITERS, MIXED_ORDERS, SDP_ITERS, SDP_TOLS, TOLS, tri
from sparse_cases import SHAPES, csc_of, identity_problem, lengths_problem, sparse_family, sparse_problem, tiny_problem, zero_problem

ZERO, RPOS, SOC, ROT, PSD = 0, 1, 2, 3, 4
LDS_MAX = 163840

# (kind, argument) in the order of the batch
SET = [("sparse", "lp40x30"), ("sparse", "lp257x129"), ("sparse", "lp300x200"), ("sparse", "mixed145x40"), ("sparse", "mixed700x300"),
       ("sparse", "lp1000x700"), ("sparse", "lp2000x1000"), ("lengths", False), ("lengths", True), ("tiny", (1, 1)), ("tiny", (1, 300)),
       ("tiny", (300, 1)), ("zero", None), ("identity", None), ("part", "part22"), ("part", "part23"), ("part", "part34"),
       ("part", "part48"), ("part", "mixed")]


class Shape:
    """what fits and plan read of a problem given by its shape alone"""

    def __init__(self, n, m, seg_type, seg_len, nnz):
        self.n, self.m, self.seg_type, self.seg_len, self.nnz = n, m, list(seg_type), list(seg_len), nnz


def _part_shape(l):
    """partitioning_sdp on l vertices: one PSD cone of order l over tri(l) unknowns, l equality rows, one entry per row"""
    return Shape(tri(l), tri(l) + l, [PSD, ZERO], [tri(l), l], tri(l) + l)


_MIXED_M = 3 + sum(tri(k) for k in MIXED_ORDERS) + 17 + 5
DEVICE_BUILT = {"part22": _part_shape(4), "part23": _part_shape(6), "part34": _part_shape(12), "part48": _part_shape(32),
                "mixed": Shape(5, _MIXED_M, [RPOS] + [PSD] * len(MIXED_ORDERS) + [SOC, ROT], [3] + [tri(k) for k in MIXED_ORDERS] + [17, 5],
                               5 * _MIXED_M)}
_HOST = {}


def host_problem(j):
    """problem j of the set as numpy builds it (a dense problem), or None for the five the device builds"""
    kind, arg = SET[j]
    if kind == "part":
        return None
    if j not in _HOST:
        _HOST[j] = (sparse_problem(arg, 0) if kind == "sparse" else lengths_problem(arg, 0) if kind == "lengths" else
                    tiny_problem(arg[0], arg[1], 0) if kind == "tiny" else zero_problem() if kind == "zero" else identity_problem(0))
    return _HOST[j]


def problems(T):
    """the set as dense problems (needs the device for the last five)"""
    from ownbatch_cases import family
    return [family(T, SET[j][1])[0][0] if SET[j][0] == "part" else host_problem(j) for j in range(len(SET))]


def shapes():
    """the set as (n, m, layout, entry count) records, without the device"""
    out = []
    for j, (kind, arg) in enumerate(SET):
        if kind == "part":
            out.append(DEVICE_BUILT[arg])
        else:
            d = host_problem(j)
            out.append(Shape(d.n, d.m, d.seg_type, d.seg_len, int(csc_of(d)[0][-1])))
    return out


def oracle_run(T, j):
    """(dense problem, oracle run, iterates, tolerances) of problem j at what its family is held to (tests/test_gpu_sparsebatch.py),
    or None (identity: the exact products have their own test)"""
    from ownbatch_cases import family
    kind, arg = SET[j]
    if kind == "identity":
        return None
    if kind == "part":
        ds, ros = family(T, arg)
        return ds[0], ros[0], SDP_ITERS, SDP_TOLS
    name = (arg if kind == "sparse" else ("cols" if arg else "rows") if kind == "lengths" else "tiny%dx%d" % arg if kind == "tiny" else "zero")
    ds, ros, iters = sparse_family(name)
    tols = [TOLS[ITERS.index(i)] for i in iters]
    return ds[0], ros[0], iters, tols


# ---- the plan, restated --------------------------------------------------------------------------------------------------------

def capacity_bytes(n, m, cap):
    return (16 * cap + 4 * (2 * (m + n) + 4) + 15) & ~15


def psd_orders(d):
    out = []
    for t, l in zip(d.seg_type, d.seg_len):
        if t == PSD:
            k = int(round((np.sqrt(8 * l + 1) - 1) / 2))
            assert tri(k) == l
            out.append(k)
    return out


def vector_bytes(d):
    """the LDS of the problem's own vectors: the scratch (64 + 4096 + 2048 floats), 8 n + 13 m floats, the class bytes, and the
    three operands an order above 32 adds"""
    tail = 3 * 64 * 65 * 4 if max(psd_orders(d), default=0) > 32 else 0
    return 4 * (64 + 4096 + 2048 + 8 * d.n + 13 * d.m) + ((d.m + 3) & ~3) + tail


def restate(ds, nnz, caps=None, force_threads=None, force_resident=None):
    """the plan of a batch of the problems ds (n, m, seg_type, seg_len) with nnz[p] entries in slots of caps[p] (None: the own count)"""
    P = len(ds)
    caps = [c or k for c, k in zip(caps or [0] * P, nnz)]
    capb = [capacity_bytes(d.n, d.m, c) for d, c in zip(ds, caps)]
    vec = [vector_bytes(d) for d in ds]
    resident = [int(force_resident != 0 and v + c <= LDS_MAX) for v, c in zip(vec, capb)]
    threads = [force_threads or (256 if max(d.m, d.n) <= 1024 and c <= 8192 else 1024) for d, c in zip(ds, caps)]
    cls = [int(t == 1024) for t in threads]
    lds = [v + (c if r else 0) for v, c, r in zip(vec, capb, resident)]
    order = [sorted((p for p in range(P) if cls[p] == c), key=lambda p: (-nnz[p], p)) for c in (0, 1)]
    keys, layout = {}, []
    for d in ds:
        layout.append(keys.setdefault((d.m, tuple(d.seg_type), tuple(d.seg_len)), len(keys)))
    strides = [6 * d.n + 10 * d.m for d in ds]
    classes = [{"n_prob": cls.count(c), "threads": (256, 1024)[c], "lds_bytes": max([lds[p] for p in range(P) if cls[p] == c], default=0),
                "n_resident": sum(resident[p] for p in range(P) if cls[p] == c)} for c in (0, 1)]
    return {"cls": cls, "order": order, "layout": layout, "arena_at": [int(v) for v in np.cumsum([0] + strides[:-1])],
            "blob_at": [int(v) for v in np.cumsum([0] + capb[:-1])], "lds_at": [v // 4 for v in vec], "resident": resident,
            "info": {"n_prob": P, "n_layouts": len(keys), "n_resident": sum(resident), "arena_bytes": 4 * sum(strides),
                     "nnz_total": sum(nnz), "blob_bytes": sum(capb), "max_psd_order": max((k for d in ds for k in psd_orders(d)), default=0),
                     "n_psd": sum(len(psd_orders(d)) for d in ds), "classes": classes}}


def check_plan(got, want):
    """a plan from the library against the restated one: every per-problem list, and the fields of info the restatement has"""
    for k in ("cls", "order", "layout", "arena_at", "blob_at", "lds_at", "resident"):
        assert got[k] == want[k], (k, got[k], want[k])
    for k, v in want["info"].items():
        if k != "classes":
            assert got["info"][k] == v, (k, got["info"][k], v)
    for g, w in zip(got["info"]["classes"], want["info"]["classes"]):
        for k, v in w.items():
            assert g[k] == v, (k, g[k], v)
        assert g["lds_bytes"] <= LDS_MAX
