"""Records the bits of the main solver's loops (FusedSolver on every schedule, BatchSolver) into tests/golden/step_bits.json: per
case and run a SHA-256 of the iterate and of the solution after 40 iterations with a launch cut inside (25, then 15), the status,
cri / tau / kappa as float hex and schedule_in_use().  tests/test_gpu_step_bits.py recomputes the record and compares it field by
field.  Every run has gemv_autotune=False and sweep_min_bytes=0 (no timing decides a plan; "sweep" whenever the kernel takes the shape).

The cases are the smallest shapes that reach each kernel of the step (totsu_amd/csrc/thip_step.h holds its arithmetic):
    small           950 x 24    reference, fused, carried; carried also "plain": xupdate_k, ycrit_k, post_k, status_k, soc_k<false>
    long            9107 x 100  carried: soc_k<true>, cones of 2049 rows
    short_soc       351 x 96    sweep, compensated and plain: sw_cone_k with the folded termination test
    short_soc_rot   353 x 96    sweep: sw_xm_k<false>, soc_k, sw_vm_k, status_k
    lp64            128 x 64    sweep, dense LP: sw_xm_k<true> (merged)
    sparse_lp       80 x 61     sweep, scipy-sparse LP: sw_xm_k<true, true> (one thread per row), the tiled copy's epilogue
    psd             1131 x 96   carried: rows of class 3
    F1              128 x 64    carried and sweep, run to the verdict: the tau -> 0 arm of the criteria and of the verdict
    batch           950 x 24    BatchSolver over three instances of small

The solvers are driven through the public Python API alone (beside it: the cone constants of totsu_amd._lib and
totsu_amd.problem._Dense to hold the tau -> 0 family); the problems come from the generators of tests/problems.py and
tests/tau_zero_problems.py and from the layouts of tests/cone_layouts.py; no oracle.  The layouts and their generator below are
copies of those in tests/cone_layouts.py on purpose: the script has to run unchanged on the commit whose bits it first recorded.  If
the two drift apart, the record's "inputs" hash says so.  Needs a gfx950 GPU.  Run on a commit whose arithmetic is meant to be pinned:
    python tests/golden/make_step_bits_fixture.py
"""
import hashlib
import json
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DST = os.path.join(HERE, "step_bits.json")
F = np.float32
Z, P, S, R, PSD = 0, 1, 2, 3, 4                   # totsu_amd._lib.CONE_*
SQ2 = np.sqrt(2.0)


def tri(k):
    return k * (k + 1) // 2


_RAGGED = [(P, 1), (S, 3), (S, 3), (R, 2), (R, 2), (S, 0), (S, 1), (R, 1), (S, 64), (R, 65), (Z, 2), (S, 65), (R, 66), (P, 2), (S, 66),
           (R, 3), (R, 3), (R, 4), (R, 4), (S, 2), (S, 2), (R, 129), (S, 129), (P, 1), (R, 130), (S, 130), (S, 64), (P, 3), (Z, 3)]
_SHORT = [(S, 5), (S, 0), (S, 1), (S, 2), (S, 128), (S, 129), (S, 17), (S, 2), (S, 64), (S, 3)]
_PSD_HEAD, _PSD_TAIL = [(P, 3), (PSD, tri(2)), (PSD, tri(1)), (PSD, tri(3)), (PSD, tri(32)), (PSD, tri(33))], \
    [(S, 17), (R, 5), (R, 1), (R, 2), (R, 2), (Z, 2)]
# name -> n, the segments, the seed, which target the first block cone gets, the scale of (b, c): tests/cone_layouts.py
LAYOUTS = {
    "small": dict(n=24, segs=_RAGGED, seed=0, turn=0),
    "short_soc": dict(n=96, segs=_SHORT, seed=9, turn=0),
    "short_soc_rot": dict(n=96, segs=_SHORT + [(R, 2)], seed=13, turn=0),
    "long": dict(n=100, segs=[(P, 3), (S, 2048), (R, 1), (R, 2049), (S, 2), (S, 2049), (S, 300), (R, 2048), (R, 2), (S, 1), (R, 300),
                              (S, 2), (R, 300), (P, 2)], seed=3, turn=0),
    "psd": dict(n=96, segs=_PSD_HEAD + _PSD_TAIL, seed=0, turn=0, scale=(0.02, 0.1)),
}
# (case id, problem, [(label, schedule, settings)]): plain -- state_arith; verdict -- default eps, run until the problem stops
CASES = [("small", "small", [("reference", "reference", {}), ("fused", "fused", {}), ("carried", "carried", {}),
                             ("carried-plain", "carried", {"plain": True})]),
         ("long", "long", [("carried", "carried", {})]),
         ("short_soc", "short_soc", [("sweep", "sweep", {}), ("sweep-plain", "sweep", {"plain": True})]),
         ("short_soc_rot", "short_soc_rot", [("sweep", "sweep", {})]),
         ("lp64", "lp64", [("sweep", "sweep", {})]),
         ("sparse_lp", "sparse_lp", [("sweep", "sweep", {})]),
         ("psd", "psd", [("carried", "carried", {})]),
         ("F1", "F1", [("carried-verdict", "carried", {"verdict": True}), ("sweep-verdict", "sweep", {"verdict": True})]),
         ("batch", "small", [("batch", None, {})])]
CASE_IDS = [cid for cid, _, _ in CASES]


class _D:
    """the fields of Prob*.dense() for problems built from arrays"""

    def __init__(self, a, b, c, seg_type, seg_len):
        a = np.asarray(a, F)
        self.m, self.n = a.shape
        self.mat_a, self.vec_b, self.vec_c = np.asfortranarray(a).ravel(order="F"), np.asarray(b, F), np.asarray(c, F)
        self.seg_type, self.seg_len, self.vec_b_rowabs = list(seg_type), list(seg_len), None


def _mb(T, typ):
    return T.MatBuild(T.F32HIP, typ)


def _psd_block(T, n, k, seed):
    """(the k (k + 1) / 2 rows of A, of b, the share of c) of one PSD cone of order k: tests/ownbatch_cases.py"""
    from problems import random_sdp
    c, syms = random_sdp(n, k, seed=seed)
    sdp = T.ProbSDP(_mb(T, T.MatType.General(n, 1)).set_array(c.reshape(-1, 1)),
                    [_mb(T, T.MatType.SymPack(k)).set_array(s) for s in syms],
                    _mb(T, T.MatType.General(0, n)), _mb(T, T.MatType.General(0, 1)), 1e-12)
    d = sdp.dense()
    sdp.drop()
    sk = tri(k)
    return np.asarray(d.mat_a, dtype=F).reshape((n, d.m)).T[:sk], np.asarray(d.vec_b, dtype=F)[:sk], np.asarray(d.vec_c, dtype=F)


def _rng(layout, *key):
    return np.random.default_rng([zlib.crc32(layout.encode())] + [int(k) for k in key])


def _rot(x):
    x = np.array(x, dtype=np.float64)
    if x.size >= 2:
        x[0], x[1] = (x[0] + x[1]) / SQ2, (x[0] - x[1]) / SQ2
    return x


def _soc_pair(rng, l, target):
    v = rng.standard_normal(l - 1)
    nv = np.linalg.norm(v)
    if l == 1:
        w = np.array([rng.uniform(0.1, 1.1)])
        return (w, np.zeros(1)) if target != 1 else (np.zeros(1), w)
    if target == 2:
        s = np.concatenate([[nv], v])
        return s, rng.uniform(0.5, 1.5) * np.concatenate([[nv], -v])
    w = np.concatenate([[rng.uniform(1.5, 2.5) * nv + rng.uniform(0.1, 1.1)], v])
    return (w, np.zeros(l)) if target == 0 else (np.zeros(l), w)


def _targets(layout):
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
    L = LAYOUTS[layout]
    rng = _rng(layout, seed, instance, 1)
    x0 = rng.standard_normal(L["n"])
    tg = _targets(layout)
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
                s, y = _rot(s), _rot(y)
        s0.append(s)
        y0.append(y)
    return x0, np.concatenate(s0), np.concatenate(y0)


_A = {}


def _matrix(T, layout, seed):
    if (layout, seed) in _A:
        return _A[layout, seed]
    L = LAYOUTS[layout]
    n = L["n"]
    st, sl = [t for t, _ in L["segs"]], [l for _, l in L["segs"]]
    beg = [int(b) for b in np.cumsum([0] + sl)[:-1]]
    m = sum(sl)
    rng = _rng(layout, seed, 0)
    A = (rng.standard_normal((m, n)) / np.sqrt(n)).astype(F)
    b_psd, c_psd, q = np.zeros(m, F), np.zeros(n, F), 0
    for t, l, b0 in zip(st, sl, beg):
        if t == PSD:
            k = int(round((np.sqrt(8 * l + 1) - 1) / 2))
            A[b0:b0 + l], b_psd[b0:b0 + l], c = _psd_block(T, n, k, 10 + q + 100 * seed)
            c_psd += c
            q += 1
    if q:
        c_psd /= q
    _A[layout, seed] = (A, b_psd, c_psd)
    return _A[layout, seed]


def build(T, layout, instance=0):
    """tests/cone_layouts.py::build on the layout's seed"""
    L = LAYOUTS[layout]
    seed = L["seed"]
    A, b_psd, c_psd = _matrix(T, layout, seed)
    x0, s0, y0 = _point(layout, seed, instance)
    st, sl = [t for t, _ in L["segs"]], [l for _, l in L["segs"]]
    A64 = A.astype(np.float64)
    other = np.concatenate([np.full(l, t != PSD) for t, l in zip(st, sl)] + [np.zeros(0, bool)])
    sb, sc = L.get("scale", (1.0, 1.0))
    x0, s0, y0 = sb * x0, sb * s0, sc * y0
    b = np.where(other, A64 @ x0 + s0, sb * b_psd.astype(np.float64))
    c = -A64.T @ y0 + sc * c_psd
    return _D(A, b, c, st, sl)


_PROBLEMS = {}


def problems(T, name):
    """the problems of one name, built once: one, or (small) the three instances over one A"""
    if name not in _PROBLEMS:
        if name in LAYOUTS:
            ds = [build(T, name, inst) for inst in ((0, 1, 2) if name == "small" else (0,))]
        elif name == "lp64":
            from problems import benchmark_lp
            c, G, h = benchmark_lp(64, seed=0)
            ds = [_D(G, h, c, [P], [128])]
        elif name == "sparse_lp":
            from problems import l1reg_lp
            c, G, h = l1reg_lp(20, seed=1)
            ds = [_D(G, h, c, [P], [h.size])]
        else:
            assert name == "F1", name
            import tau_zero_problems as TZ
            from totsu_amd.problem import _Dense
            ds = [_Dense(*TZ.family("F1").args())]
        _PROBLEMS[name] = ds
    return _PROBLEMS[name]


def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, dtype=F).tobytes())
    return h.hexdigest()


def _fields(it, sol, st, schedule):
    return {"iterate": _sha(*it), "solution": _sha(*sol), "status": [int(st.state), int(st.iters), int(st.kind)],
            "cri": [float(v).hex() for v in st.cri], "tau": float(st.tau).hex(), "kappa": float(st.kappa).hex(), "schedule": schedule}


def _param(T, kw):
    p = T.SolverParam()
    if kw.get("verdict"):
        p.max_iter = 100_000
    else:
        p.eps_acc = 1e-30
    if kw.get("plain"):
        p.state_arith = "plain"
    return p


def record(T, case_id):
    """the record of one case: {"inputs": sha, "runs": {label: {field: value}}} (the batch: one run per instance)"""
    _, name, runs = CASES[CASE_IDS.index(case_id)]
    ds = problems(T, name)
    inputs = _sha(*([d.mat_a for d in ds] + [d.vec_b for d in ds] + [d.vec_c for d in ds]))
    out = {}
    for label, schedule, kw in runs:
        d = ds[0]
        if schedule is None:
            bt = T.BatchSolver.from_dense(d, [q.vec_b for q in ds], [q.vec_c for q in ds], _param(T, kw), gemv_autotune=False)
            try:
                bt.run(25, poll_every=25)
                bt.run(15, poll_every=5)
                for i in range(len(ds)):
                    out["%s-%d" % (label, i)] = _fields(bt.iterate(i), bt.solution(i), bt.status(i), "batch")
            finally:
                bt.destroy()
            continue
        mat_a = d.mat_a
        if name == "sparse_lp":
            import scipy.sparse as sp
            mat_a = sp.csr_matrix(np.asarray(d.mat_a, F).reshape((d.n, d.m)).T)
        fs = T.FusedSolver(d.n, d.m, mat_a, d.vec_b, d.vec_c, d.seg_type, d.seg_len, _param(T, kw), schedule,
                           gemv_autotune=False, sweep_min_bytes=0)
        try:
            in_use = fs.schedule_in_use()
            if kw.get("verdict"):
                fs.run(-1, poll_every=25)
            else:
                fs.run(25, poll_every=25)
                fs.run(15, poll_every=5)
            out[label] = _fields(fs.iterate(), fs.solution(), fs.status(), in_use)
        finally:
            fs.destroy()
    return {"inputs": inputs, "runs": out}


def main():
    root = os.path.dirname(os.path.dirname(HERE))
    for p in (root, os.path.join(root, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import totsu_amd as T
    from totsu_amd import _lib
    _lib.init()
    out = {"what": "the main solver's step bits on gfx950; tests/golden/make_step_bits_fixture.py", "cases": {}}
    for cid in CASE_IDS:
        out["cases"][cid] = record(T, cid)
        print(cid, [(k, r["schedule"], r["status"]) for k, r in out["cases"][cid]["runs"].items()])
    dst = sys.argv[1] if len(sys.argv) > 1 else DST
    with open(dst, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", dst, len(out["cases"]), "cases")


if __name__ == "__main__":
    main()
