"""Records the bits of the three own-A batch families (SmallBatchSolver, MidBatchSolver, SdpBatchSolver) into
tests/golden/ownbatch_bits.json: per case and problem a SHA-256 of the iterate, the preconditioner and the solution after 40
iterations with launch cuts inside, the status, and cri / tau / kappa as float hex.  tests/test_gpu_ownbatch_bits.py recomputes
the record and compares it field by field.

The solvers are driven through the public Python API alone (beside it: the cone constants of totsu_amd._lib and
totsu_amd.problem._Dense to hold a tau -> 0 family); the problems come from the generators of tests/problems.py and
tests/tau_zero_problems.py; no oracle.  The builders below (_D, _socp, _sdp, _mixed) are copies of those in tests/ownbatch_cases.py on
purpose: the script has to run unchanged on a commit that has no such module, such as the one whose bits it first recorded.  If the
two drift apart, the record's "inputs" hash says so.  Needs a gfx950 GPU.  Run on a commit whose arithmetic is meant to be pinned:
    python tests/golden/make_ownbatch_bits_fixture.py
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DST = os.path.join(HERE, "ownbatch_bits.json")
F = np.float32
MIXED_ORDERS = [3, 6, 6, 12, 6, 33, 12, 1]
# (family, case id, problems, settings): replace -- slot 1 takes the fourth problem between the two runs; verdict -- default
# eps, run until the problem stops
CASES = [("small", "lp20", "lp20", {}),
         ("small", "lp20-1024", "lp20", {"force_threads": 1024}),
         ("small", "socp", "socp", {}),
         ("small", "lp40-plain", "lp40", {"state_arith": "plain"}),
         ("small", "lp20-replace", "lp20", {"replace": True}),
         ("mid", "lp80", "lp80", {}),
         ("mid", "lp20-256", "lp20", {"force_threads": 256}),
         ("mid", "socp60", "socp60", {}),
         ("mid", "lp80-plain", "lp80", {"state_arith": "plain"}),
         ("mid", "F1-verdict", "F1", {"verdict": True}),
         ("mid", "lp80-replace", "lp80", {"replace": True}),
         ("sdp", "sdp9", "sdp9", {}),
         ("sdp", "sdp33", "sdp33", {}),
         ("sdp", "mixed", "mixed", {}),
         ("sdp", "sdp9-plain", "sdp9", {"state_arith": "plain"}),
         ("sdp", "lp80", "lp80", {})]
CASE_IDS = ["%s-%s" % (fam, cid) for fam, cid, _, _ in CASES]


class _D:
    """the fields of Prob*.dense() for problems built from arrays"""

    def __init__(self, a, b, c, seg_type, seg_len):
        a = np.asarray(a, F)
        self.m, self.n = a.shape
        self.mat_a, self.vec_b, self.vec_c = np.asfortranarray(a).ravel(order="F"), np.asarray(b, F), np.asarray(c, F)
        self.seg_type, self.seg_len, self.vec_b_rowabs = list(seg_type), list(seg_len), None


def _mb(T, typ):
    return T.MatBuild(T.F32HIP, typ)


def _lp(sz, seed):
    from problems import benchmark_lp
    c, G, h = benchmark_lp(sz, seed=seed)
    return _D(G, h, c, [1], [2 * sz])


def _socp(T, n, cones, seed):
    from problems import random_socp
    f, Gs, hs, cs, d = random_socp(n, cones, seed=seed)
    socp = T.ProbSOCP(_mb(T, T.MatType.General(n, 1)).set_array(f.reshape(-1, 1)),
                      [_mb(T, T.MatType.General(G.shape[0], n)).set_array(G) for G in Gs],
                      [_mb(T, T.MatType.General(len(h_), 1)).set_array(h_.reshape(-1, 1)) for h_ in hs],
                      [_mb(T, T.MatType.General(n, 1)).set_array(c_.reshape(-1, 1)) for c_ in cs], d,
                      _mb(T, T.MatType.General(0, n)), _mb(T, T.MatType.General(0, 1)))
    dn = socp.dense()
    assert dn.vec_b_rowabs is not None
    return dn


def _sdp(T, n, k, seed):
    from problems import random_sdp
    c, syms = random_sdp(n, k, seed=seed)
    sdp = T.ProbSDP(_mb(T, T.MatType.General(n, 1)).set_array(c.reshape(-1, 1)),
                    [_mb(T, T.MatType.SymPack(k)).set_array(s) for s in syms],
                    _mb(T, T.MatType.General(0, n)), _mb(T, T.MatType.General(0, 1)), 1e-12)
    d = sdp.dense()
    sdp.drop()
    return d


def _mixed(T, seed):
    """3 nonnegative rows, PSD cones of eight orders, a second-order cone of 17 rows and a rotated one of 5"""
    from totsu_amd import _lib
    n = 5
    rng = np.random.default_rng(99 + seed)
    blocks = [rng.standard_normal((3, n)).astype(F)]
    bs, st, sl = [np.abs(rng.standard_normal(3)).astype(F) + 1.0], [_lib.CONE_RPOS], [3]
    c0 = np.zeros(n, F)
    for q, k in enumerate(MIXED_ORDERS):
        d = _sdp(T, n, k, 10 + q + 100 * seed)
        sk = k * (k + 1) // 2
        blocks.append(np.asarray(d.mat_a, dtype=F).reshape((n, d.m)).T[:sk])
        bs.append(np.asarray(d.vec_b, dtype=F)[:sk])
        st.append(_lib.CONE_PSD)
        sl.append(sk)
        c0 = c0 + np.asarray(d.vec_c, dtype=F)
    for t, rows in ((_lib.CONE_SOC, 17), (_lib.CONE_ROTSOC, 5)):
        blocks.append((rng.standard_normal((rows, n)) / 4).astype(F))
        b = (rng.standard_normal(rows) / 4).astype(F)
        b[0] = 3.0
        if t == _lib.CONE_ROTSOC:
            b[1] = 3.0
        bs.append(b)
        st.append(t)
        sl.append(rows)
    return _D(np.vstack(blocks), np.concatenate(bs), c0 / len(MIXED_ORDERS), st, sl)


_PROBLEMS = {}


def problems(T, name):
    """the problems of one family (the fourth of an LP family is what a replace case puts into slot 1), built once"""
    if name not in _PROBLEMS:
        if name in ("lp20", "lp40", "lp80"):
            ds = [_lp(int(name[2:]), seed) for seed in range(4)]
        elif name == "socp":
            ds = [_socp(T, 12, [5, 1, 0, 17, 70, 3], seed) for seed in range(3)]
        elif name == "socp60":
            ds = [_socp(T, 60, [5, 1, 0, 17, 140, 250, 3], seed) for seed in range(3)]
        elif name == "F1":
            import tau_zero_problems as Z
            from totsu_amd.problem import _Dense
            ds = [_Dense(*Z.family("F1").args())]
        elif name in ("sdp9", "sdp33"):
            ds = [_sdp(T, 6, int(name[3:]), seed) for seed in range(3)]
        else:
            assert name == "mixed", name
            ds = [_mixed(T, seed) for seed in range(3)]
        _PROBLEMS[name] = ds
    return _PROBLEMS[name]


def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, dtype=F).tobytes())
    return h.hexdigest()


def record(T, case_id):
    """the record of one case: {"inputs": sha, "problems": [{field: value}]}"""
    fam, _, name, kw = CASES[CASE_IDS.index(case_id)]
    cls = {"small": T.SmallBatchSolver, "mid": T.MidBatchSolver, "sdp": T.SdpBatchSolver}[fam]
    ds = problems(T, name)
    batch, extra = (ds[:3], ds[3]) if kw.get("replace") else (ds[:3], None)
    p = T.SolverParam()
    if kw.get("verdict"):
        p.max_iter = 100_000
    else:
        p.eps_acc = 1e-30
    if "state_arith" in kw:
        p.state_arith = kw["state_arith"]
    used = batch + ([extra] if extra is not None else [])
    rowabs = [d.vec_b_rowabs for d in used if d.vec_b_rowabs is not None]
    inputs = _sha(*([d.mat_a for d in used] + [d.vec_b for d in used] + [d.vec_c for d in used] + rowabs))
    ctor = {"force_threads": kw["force_threads"]} if "force_threads" in kw else {}
    sb = cls.from_dense(batch, p, **ctor)
    try:
        if kw.get("verdict"):
            sb.run(-1, poll_every=25)
        else:
            sb.run(25, poll_every=25)
            if extra is not None:
                sb.replace(1, extra.mat_a, extra.vec_b, extra.vec_c)
            sb.run(15, poll_every=5)
        out = []
        for i in range(len(batch)):
            (ix, iy), (pt, ps), (sx, sy), st = sb.iterate(i), sb.precond(i), sb.solution(i), sb.status(i)
            out.append({"iterate_x": _sha(ix), "iterate_y": _sha(iy), "precond_tau": _sha(pt), "precond_sigma": _sha(ps),
                        "solution_x": _sha(sx), "solution_y": _sha(sy), "status": [int(st.state), int(st.iters), int(st.kind)],
                        "cri": [float(v).hex() for v in st.cri], "tau": float(st.tau).hex(), "kappa": float(st.kappa).hex()})
    finally:
        sb.destroy()
    return {"inputs": inputs, "problems": out}


def main():
    root = os.path.dirname(os.path.dirname(HERE))
    for p in (root, os.path.join(root, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import totsu_amd as T
    from totsu_amd import _lib
    _lib.init()
    out = {"what": "own-A batch bits on gfx950; tests/golden/make_ownbatch_bits_fixture.py", "cases": {}}
    for cid in CASE_IDS:
        out["cases"][cid] = record(T, cid)
        print(cid, [q["status"] for q in out["cases"][cid]["problems"]])
    dst = sys.argv[1] if len(sys.argv) > 1 else DST
    with open(dst, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", dst, len(out["cases"]), "cases")


if __name__ == "__main__":
    main()
